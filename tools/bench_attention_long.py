"""attention beyond 320 keys: forward and backward timings (device events after warm-up) of the streaming kernels
(attention.hip attn_long_kernel / attn_kvl_kernel) next to the short path they extend.  FLOPs as SURVEY counts them: forward
4 B H Sq Sk dh, backward 2.5 x that; the fraction is of the 2.5 PF/s bf16 MFMA peak.  Random (gaussian) data, no mask, no dropout.
usage: python tools/bench_attention_long.py [--reps N]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import gpv1_amd.hip as hip  # noqa: E402

DEV = 'cuda'
PEAK = 2.5e15
SHAPES = [  # B, H, Sq, Sk, dh, dtype, what it stands for
    (32, 8, 300, 300, 32, torch.bfloat16, 'short path (encoder, 480x640)'),
    (32, 8, 400, 400, 32, torch.bfloat16, 'encoder, 640x640'),
    (32, 8, 1200, 1200, 32, torch.bfloat16, 'encoder, DC5 480x640'),
    (32, 8, 100, 1200, 32, torch.bfloat16, 'decoder cross-attention, DC5'),
    (1, 8, 850, 850, 32, torch.bfloat16, 'encoder, one 800x1088 image'),
    (1, 8, 850, 850, 32, torch.float32, 'encoder, one 800x1088 image, precise'),
]


def timeit(fn, reps):
    for _ in range(5):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def case(B, H, Sq, Sk, dh, dtype, reps):
    D = H * dh
    g = torch.Generator().manual_seed(7)
    q = torch.randn(B * Sq, D, generator=g).to(DEV).to(dtype)
    k = torch.randn(B * Sk, D, generator=g).to(DEV).to(dtype)
    v = torch.randn(B * Sk, D, generator=g).to(DEV).to(dtype)
    do = torch.randn(B * Sq, D, generator=g).to(DEV).to(dtype)
    o, dq, dk, dv = torch.empty_like(q), torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    lse = torch.empty(B, H, Sq, device=DEV)
    st = ((Sq * D, D), (Sk * D, D), (Sk * D, D), (Sq * D, D))
    sc = 1.0 / math.sqrt(dh)
    fwd = lambda: hip.attention_fwd(q, k, v, o, st, B, H, Sq, Sk, dh, sc, lse=lse)
    bwd = lambda: hip.attention_bwd(q, k, v, o, do, dq, dk, dv, st, (Sq * D, D), B, H, Sq, Sk, dh, sc, lse=lse)
    tf = timeit(fwd, reps)
    tb = timeit(bwd, reps)
    fl = 4.0 * B * H * Sq * Sk * dh
    return tf, fl / tf / 1e6, tb, 2.5 * fl / tb / 1e6


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--reps', type=int, default=50)
    args = ap.parse_args()
    hip.lib()
    print('%-5s %-30s %-22s %10s %8s %7s %10s %8s %7s' % ('dtype', 'shape (B, H, Sq, Sk, dh)', 'stands for', 'fwd us', 'TF/s', 'peak', 'bwd us', 'TF/s', 'peak'))
    res = {}
    for B, H, Sq, Sk, dh, dtype, what in SHAPES:
        tf, rf, tb, rb = case(B, H, Sq, Sk, dh, dtype, args.reps)
        res[(B, H, Sq, Sk, dtype)] = (rf, rb)
        print('%-5s %-30s %-22s %10.1f %8.1f %6.1f%% %10.1f %8.1f %6.1f%%' % (
            'bf16' if dtype == torch.bfloat16 else 'fp32', str((B, H, Sq, Sk, dh)), what[:22], tf, rf, 100 * rf * 1e12 / PEAK,
            tb, rb, 100 * rb * 1e12 / PEAK), flush=True)
    short = res[(32, 8, 300, 300, torch.bfloat16)][0]
    f, b = res[(32, 8, 1200, 1200, torch.bfloat16)]
    print('(32, 8, 1200, 1200) bf16: forward %.2f x, backward %.2f x the short forward rate (%.1f TF/s); target >= 1, floor 0.5'
          % (f / short, b / short, short))


if __name__ == '__main__':
    main()
