"""Issue every case of tests/route_cases.py once at its real shape, through hip.gemm / hip.conv2d / hip.set_option only, so that a kernel
trace of the run lists what each call launched:
    rocprofv3 --kernel-trace --output-format csv -d OUT -- python tools/route_sweep.py [--tree DIR] [--log FILE]
--tree DIR imports gpv1_amd from another checkout (a built copy of an earlier commit): the same file then traces that commit's
launches for the same cases, which is how a change of the dispatcher is shown to move nothing (profiles/r17_routes.txt).
Between two cases one torch fill of a marker tensor runs: in the trace the launches between fill i and fill i + 1 belong to case i of
the log (FILE: one `index name status` line per case; status = ok | refused, the call raised).  Operand contents are zeros: only the
launches matter."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument('--tree', default=ROOT)
ap.add_argument('--log', default=None)
args = ap.parse_args()
sys.path.insert(0, ROOT)
from tests import route_cases  # noqa: E402
sys.path.insert(0, os.path.abspath(args.tree))
import torch  # noqa: E402
import gpv1_amd.hip as hip  # noqa: E402

assert os.path.abspath(hip.__file__).startswith(os.path.abspath(args.tree)), hip.__file__
dev = torch.device('cuda:0')
hip.lib()
DT = {0: torch.bfloat16, 1: torch.float32}
MB = 1 << 20
bufs = {n: torch.zeros(mb * MB + 64, dtype=torch.uint8, device=dev) for n, mb in (('A', 400), ('B', 400), ('C', 400), ('res', 400), ('mask', 400), ('bits', 24))}
bias = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
rowsum = torch.zeros(1 << 16, dtype=torch.float32, device=dev)
marker = torch.zeros(64, dtype=torch.float32, device=dev)


def take(name, dtype, n, off=0):
    """n elements of `dtype` from buffer `name`, `off` elements past its 16-byte aligned base"""
    v = bufs[name].view(dtype)
    assert off + n <= v.numel(), (name, n)
    return v[off:off + n]


def run_gemm(c):
    din, dout = DT[c['din']], DT[c['dout']]
    M, N, K, la, lb, batch = c['M'], c['N'], c['K'], c['la'], c['lb'], c['batch']
    lda = c['lda'] or (M if la else K)
    ldb = c['ldb'] or (N if lb else K)
    ldc = c['ldc'] or N
    sA, sB, sC = (K if la else M) * lda, (K if lb else N) * ldb, M * ldc
    A, B, Cm = take('A', din, sA * batch, c['offA']), take('B', din, sB * batch, c['offB']), take('C', dout, sC * batch)
    kw = dict(layoutA=la, layoutB=lb, batch=batch, sA=sA, sB=sB, sC=sC, alpha=c['alpha'], act=c['act'], drop_p=0.1 if c['drop'] else 0.0, seed=1,
              accumulate=bool(c['acc']), split_k=c['split_k'], kpad_finite=bool(c['kpad']))
    if c['bias']:
        kw['bias'] = bias[:N]
    if c['res']:
        kw.update(res=take('res', dout, sC * batch), ldr=ldc, sR=sC)
    if c['mask']:
        kw.update(relu_mask=take('mask', dout, sC * batch), ldm=ldc)
    if c['rowsum']:
        kw['a_rowsum'] = rowsum[:M]
    if c['nosmall']:
        with hip.gemm_flags(hip.GEMM_NO_PIPE_SMALL):
            hip.gemm(A, B, Cm, M, N, K, lda, ldb, ldc, **kw)
    else:
        hip.gemm(A, B, Cm, M, N, K, lda, ldb, ldc, **kw)


def run_conv(c):
    din, dout = DT[c['din']], DT[c['dout']]
    g = [c[k] for k in ('B', 'IH', 'IW', 'Cs', 'Cin', 'OH', 'OW', 'Cout', 'KH', 'KW', 'SH', 'SW', 'PH', 'PW')]
    B, IH, IW, Cs, Cin, OH, OW, Cout, KH, KW = g[:10]
    x = take('A', din, B * IH * IW * Cs, c['offx'])
    if c['mode'] == 2:
        w, y = take('B', din, B * OH * OW * Cout), take('C', dout, Cout * KH * KW * Cin)
    else:
        w, y = take('B', din, Cout * KH * KW * Cin), take('C', dout, B * OH * OW * Cout)
    kw = dict(act=c['act'], split_k=c['split_k'])
    if c['bias']:
        kw['bias'] = bias[:Cout]
    if c['res']:
        kw['res'] = take('res', dout, B * OH * OW * Cout)
    if c['mask']:
        kw['relu_mask'] = take('mask', dout, B * OH * OW * Cout)
    if c['bits']:
        kw['y_mask_bits' if c['bits'] == 1 else 'relu_mask_bits'] = take('bits', torch.int32, B * OH * OW * Cout // 32).view(B * OH * OW, Cout // 32)
    hip.conv2d(c['mode'], x, w, y, *g, **kw)


# grow the shared split-reduction workspace to its full size first (a weight gradient asks for all of it): every later call that is
# lent a workspace is lent WS_MAX bytes, which is what the cases state
run_conv(route_cases.conv('warmup', 2, 1, 30, 40, 64, 64, 1, 1))
torch.cuda.synchronize()
log = open(args.log, 'w') if args.log else sys.stdout
cases = [c for c in route_cases.CASES if c['gpu']]
for i, c in enumerate(cases):
    marker.fill_(float(i))
    prev = {o: hip.set_option(o, v) for o, v in c['opts'].items()}
    try:
        (run_gemm if c['ep'] == 'gemm' else run_conv)(c)
        status = 'ok'
    except RuntimeError as e:
        status = 'refused'
    finally:
        for o, v in prev.items():
            hip.set_option(o, v)
    log.write('%d %s %s\n' % (i, c['name'], status))
marker.fill_(-1.0)
torch.cuda.synchronize()
log.write('done %d\n' % len(cases))
log.flush()
print('route_sweep: %d cases issued from %s' % (len(cases), os.path.abspath(args.tree)))
