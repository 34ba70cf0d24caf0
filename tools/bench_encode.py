"""What the device JPEG encoder costs and what it replaces, at 15 and at 32 pictures of 480 x 640, quality 90, 4:2:0:
  (a) the device path end to end: DeviceJpegEncoder.encode_batch on a pipeline batch with five boxes per picture -- four launches, the
      read-back of sizes and status, the copy of the bytes used; and the four launches alone, by device events;
  (b) the host alternative: the uint8 pictures copied back and encoded by Pillow on one thread and on 16;
  (c) the loader-fed bs32 train step (tools/bench_loader.py's tree) with training visualisations every 50 steps against none: 100
      steps each, alternating, and what one visualize() call of 15 samples costs.
Warm-up first, five runs each, median and spread reported.  One JSON document on stdout.
--labels N: (a) with N labelled boxes per picture (labels); --device-only --lib PATH: (a) alone through another build of
libgpv_enc.so, one process per run, for interleaved comparisons of two builds (profiles/r21_labels.txt).
usage: python tools/bench_encode.py [--no-step] [--steps 100] [--vis-step 50] [--labels N] [--device-only [--lib PATH]]      (GPU box)"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpv1_amd import hip_enc, jpeg_encode                         # noqa: E402
from gpv1_amd.inference import IMAGENET_MEAN, IMAGENET_STD        # noqa: E402
from gpv1_amd.input_pipeline import DeviceImagePipeline           # noqa: E402

RUNS = 5


def stats(ms):
    return {'median_ms': sorted(ms)[len(ms) // 2], 'min_ms': min(ms), 'max_ms': max(ms)}


def pictures(n, H=480, W=640):
    """photograph-like content: smooth structure plus texture (tools/bench_input.py's files are made the same way)"""
    rng = np.random.default_rng(0)
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        base = 128 + 80 * np.sin(xx / (20 + 3 * i)) * np.cos(yy / (31 + i)) + 30 * np.sin((xx + yy) / 7.0)
        img = np.stack([base, np.roll(base, 17 * i, 1), base[::-1]], -1) + rng.normal(0, 6, (H, W, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def encode_numbers(n, labels=0, host=True, bare=5):
    """labels = 0: `bare` boxes per picture without labels; labels = N: N boxes per picture, each with a label (a score above or `GT` below)"""
    imgs = pictures(n)
    nested = DeviceImagePipeline(train=False)(imgs)
    rng = np.random.default_rng(1)
    nb = labels or bare
    boxes = [np.concatenate([rng.uniform(0.3, 0.7, (nb, 2)), rng.uniform(0.1, 0.5, (nb, 2))], 1).astype(np.float32) for _ in range(n)]
    colours = [[(255, 0, 0)] * nb for _ in range(n)]
    texts = [[f'{rng.uniform():.2f}' if k % 2 == 0 else ('GT', 'below') for k in range(nb)] for _ in range(n)] if labels else None
    enc = jpeg_encode.DeviceJpegEncoder(quality=90, subsampling='4:2:0')
    run = lambda: enc.encode_batch(nested, IMAGENET_MEAN, IMAGENET_STD, boxes=boxes, colours=colours, **({'labels': texts} if labels else {}))
    files = run()
    run()
    res = {'pictures': n, 'boxes_per_picture': nb, 'labels_per_picture': labels, 'library': hip_enc._LIB_PATH,
           'file_bytes_mean': float(np.mean([len(f) for f in files])), 'device_end_to_end': stats([wall(run) for _ in range(RUNS)])}
    # the four launches alone: the raw entry point between two events, descriptors as encode_batch fills them
    import ctypes as C
    x = nested.tensors
    Hp, Wp = x.shape[1:3]
    pinned = torch.zeros(n * C.sizeof(hip_enc.EncDesc), dtype=torch.uint8).pin_memory()
    descs = (hip_enc.EncDesc * n).from_address(pinned.data_ptr())
    keep = []
    for i, d in enumerate(descs):
        d.src = x.data_ptr() + ((i * Hp + 3) * Wp + 3) * 4 * x.element_size()
        d.H, d.W, d.pitch, d.kind = 480, 640, Wp, hip_enc.SRC_BF16 if x.dtype == torch.bfloat16 else hip_enc.SRC_F32
        d.mean[:], d.std[:] = IMAGENET_MEAN, IMAGENET_STD
        packed, nbytes = jpeg_encode.pack_labels(colours[i], texts[i] if labels else None)
        b, c = torch.as_tensor(boxes[i]).cuda(), torch.from_numpy(packed).cuda()
        keep += [b, c]
        d.boxes, d.colours, d.nboxes, d.labels = b.data_ptr(), c.data_ptr(), nb, nbytes
    count = hip_enc.block_count(480, 640, '4:2:0')
    capacity = (hip_enc.HEADER_BYTES + 2 + 64 * count + 15) & ~15
    ws = torch.empty(hip_enc.workspace_bytes(n, n * count), dtype=torch.uint8, device='cuda')
    out, sizes, status = torch.empty(n * capacity, dtype=torch.uint8, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')
    launch = lambda: hip_enc.encode(descs, n, 90, '4:2:0', ws, out, capacity, sizes, status)
    launch()
    torch.cuda.synchronize()
    assert not status.any() and sizes.tolist() == [len(f) for f in files]
    ms = []
    for _ in range(RUNS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            launch()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / 10)
    res['device_four_launches'] = stats(ms)
    if not host:
        return res
    # (b) the pictures as uint8 on the device (what a host encoder would be handed), copied back and encoded by Pillow
    from PIL import Image
    dev_u8 = torch.stack([torch.from_numpy(jpeg_encode.denormalise_host(x[i, 3:483, 3:643, :3].cpu(), IMAGENET_MEAN, IMAGENET_STD)) for i in range(n)]).cuda()

    def pillow(a):
        buf = io.BytesIO()
        Image.fromarray(a).save(buf, 'JPEG', quality=90, subsampling='4:2:0')
        return buf.getvalue()
    for threads in (1, 16):
        pool = ThreadPoolExecutor(threads)

        def host():
            arr = dev_u8.cpu().numpy()
            return list(pool.map(pillow, arr))
        host()
        res[f'host_copy_back_and_pillow_{threads}_threads'] = stats([wall(host) for _ in range(RUNS)])
        pool.shutdown()
    return res


def step_numbers(a):
    from bench_loader import V, write_tree
    from gpv1_amd import synthetic
    from gpv1_amd.bert import WordPieceTokenizer
    from gpv1_amd.datasets import CocoCaptioning, DeviceLoader
    from gpv1_amd.gpv import GPV
    from gpv1_amd.misc import AttrDict
    from gpv1_amd.train import FlatTrainer
    from gpv1_amd.train_distr import shard_indices
    from gpv1_amd.visualize import visualize
    with tempfile.TemporaryDirectory() as root:
        words = synthetic.write_wordpiece_vocab(os.path.join(root, 'vocab.txt'))
        tree = write_tree(root, 128, words)
        ds, vis_ds = CocoCaptioning(tree, 'train'), CocoCaptioning(tree, 'train')
        g = torch.Generator().manual_seed(0)
        model = GPV(synthetic.model_cfg(vocab=synthetic.make_vocab(V), vocab_embed=0.1 * torch.randn(V, 768, generator=g)))
        model.bert.tokenizer = WordPieceTokenizer(os.path.join(root, 'vocab.txt'))
        model.to('cuda').train()
        tr = FlatTrainer(model)
        loader, vis_loader = DeviceLoader(ds, 32, threads=8, prefetch=1), DeviceLoader(vis_ds, 32, threads=8, prefetch=0)
        cfg = AttrDict.wrap({'exp_dir': os.path.join(root, 'exp'), 'training': {'num_vis_samples': 15}})

        def vis(step):
            for subset in ('train', 'val'):
                visualize(model, vis_loader.eval_batches(32), cfg, step, subset)

        def window(steps, vis_step):
            n, e = 0, 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            while n < steps:
                for samples, qs, tg in loader.batches(shard_indices(len(ds), e, 0, 1), e):
                    tr.train_step(samples, qs, tg)
                    if vis_step and n % vis_step == 0:
                        vis(n)
                    n += 1
                    if n == steps:
                        break
                e += 1
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / steps * 1e3
        window(16, 0)                                         # warm-up: eager step, captures, slots
        vis(0)
        captures = tr.capture_count
        off, on = [], []
        for _ in range(3):
            off.append(window(a.steps, 0))
            on.append(window(a.steps, a.vis_step))
        res = {'steps_per_window': a.steps, 'vis_step': a.vis_step, 'step_ms_visualize_off': stats(off), 'step_ms_visualize_device': stats(on),
               'one_visualize_call_train_and_val_ms': stats([wall(lambda: vis(1)) for _ in range(RUNS)]),
               'recaptures_during_timing': tr.capture_count - captures}
        loader.close()
        vis_loader.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--no-step', action='store_true', help='(a) and (b) only')
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--vis-step', type=int, default=50)
    ap.add_argument('--labels', type=int, default=0, help='(a) with N labelled boxes per picture instead of five bare ones')
    ap.add_argument('--device-only', action='store_true', help='(a) only, at 32 pictures')
    ap.add_argument('--boxes', type=int, default=5, help='with --device-only and without --labels: bare boxes per picture')
    ap.add_argument('--lib', default=None, help='(a) through another libgpv_enc.so, e.g. one built from the parent commit (same ABI, no labels)')
    a = ap.parse_args()
    if a.lib:
        hip_enc._LIB_PATH = os.path.abspath(a.lib)
    if a.device_only:
        print(json.dumps(encode_numbers(32, a.labels, host=False, bare=a.boxes)))
        return
    res = {'encode': [encode_numbers(n, a.labels) for n in (15, 32)]}
    if not a.no_step:
        res['train_step'] = step_numbers(a)
    print(json.dumps(res, indent=1))


if __name__ == '__main__':
    main()
