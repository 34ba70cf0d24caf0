"""Exact-arithmetic checks of the GEMM / convolution kernel families -- TEST INFRASTRUCTURE (plain module, no fixtures).

With small-integer operands every product and every partial sum of a GEMM or a convolution is an integer multiple of a power of
two that fp32 represents exactly, so the result does not depend on summation order, tiling, split reductions, atomics or workspace
passes: a correct kernel returns the float64 result bit for bit, and the bf16 store is round-to-nearest-even of it.  Every
comparison here is therefore `torch.equal`; what the `max|out - ref| / max|ref| < tol` criterion of tests/test_kernels_gpu.py cannot
see (a truncating bf16 store, an fp32 result that went through bf16 once, one product dropped for a handful of outputs) fails it.

THE PRECONDITION is analytic: `exact_bound(case) < 2 ** 24` for every case of every table below (tests/test_exact_cases_cpu.py
asserts it; no test skips or filters a case to satisfy it -- `fit` CHOOSES the integer ranges of a case from its shape, which is part
of defining the case).  exact_bound is an upper bound of every value that can appear, in units of the smallest step that can appear.

Not exact, and left to the tolerance tests: GELU, softmax (the attention core), LayerNorm statistics, AdamW.

The check functions take the backend module as their first argument: gpv1_amd.hip on the GPU, tests.cpu_shim on the CPU (which proves
the references, layouts and epilogue order of these checks independently of any kernel).  tools/fuzz_kernels.py calls them with random
shapes.
"""
import contextlib
import math

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU = 0, 1
KMAJOR, TRANS = 0, 1
LIMIT = 2 ** 24
BF, F32 = torch.bfloat16, torch.float32
SENTINEL = 7.0                     # padding columns / guard rows of an output buffer: must be unchanged after the launch
ALPHAS = (0.5, 1.0, 2.0)
DROP_P = 0.5                       # keep threshold 2^31 and scale 2: both exact


def device(hip):
    """'cuda' for gpv1_amd.hip, 'cpu' for tests.cpu_shim (and wrappers of it)"""
    return 'cuda' if hasattr(hip, 'lib') else 'cpu'


def ints(*shape, lo=-3, hi=3, seed=0, dtype=torch.float64, dev='cpu'):
    """integer-valued tensor drawn on the CPU generator (the style of test_kernels_gpu.rnd)"""
    g = torch.Generator(device='cpu').manual_seed(seed + sum(shape))
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64).to(dev).to(dtype)


def pow2(n, seed=0, dev='cpu'):
    """rowscale: signed powers of two in [1/4, 4], fp32"""
    g = torch.Generator(device='cpu').manual_seed(seed + n)
    e = torch.randint(-2, 3, (n,), generator=g).double()
    s = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    return (s * 2.0 ** e).float().to(dev)


def sign_pattern(*shape, seed=0, dtype=BF, dev='cpu'):
    """a saved activation for relu_mask: integers in [-2, 2], so that zeros (NOT > 0) are a fifth of it"""
    return ints(*shape, lo=-2, hi=2, seed=seed, dtype=dtype, dev=dev)


def exact_bound(c):
    """upper bound of every intermediate and final value of a case, divided by the granularity of the values:
    (K max|a| max|b| max(1, |alpha|, |alpha| max|rowscale|) + max|bias| + max|res| + max|C0|) * dropout scale / granularity"""
    alpha = abs(c.get('alpha', 1.0))
    v = c['K'] * c['amax'] * c['bmax'] * max(1.0, alpha, alpha * c.get('rsmax', 1.0)) + c.get('bias', 0) + c.get('res', 0) + c.get('c0', 0)
    v *= c.get('dscale', 1.0)
    gran = min(1.0, alpha) * min(1.0, c.get('rsmin', 1.0))
    return v / gran


def fit(c, bound=exact_bound):
    """choose the integer ranges of a case: the widest (3, 2, 1, or what the case starts from) with which `bound` keeps the precondition"""
    c = dict(c)
    i = 0
    while bound(c) >= LIMIT and (c['amax'] > 1 or c['bmax'] > 1):
        k = ('amax', 'bmax')[i % 2]
        if c[k] > 1:
            c[k] = c[k] // 2 if c[k] > 8 else c[k] - 1
        i += 1
    return c


def assert_exact(got, ref, what):
    """torch.equal, with the pattern of the differing elements in the message"""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return
    g, r = got.double(), ref.double()
    bad = ~((g == r) | (torch.isnan(g) & torch.isnan(r)))
    idx = bad.nonzero()
    d = (g - r)[bad]
    ulp = (d.abs() / (2.0 ** (torch.floor(torch.log2(r[bad].abs().clamp_min(1e-30))) - (7 if got.dtype == BF else 23)))).max().item()
    rows = sorted(set(idx[:, -2].tolist()))[:12] if idx.shape[1] >= 2 else []
    cols = sorted(set(idx[:, -1].tolist()))[:12]
    raise AssertionError('%s: %d of %d elements differ (NaN left: %d); max |diff| %g = %.1f ulp; rows %s cols %s; first %s got %s want %s' % (
        what, int(bad.sum()), bad.numel(), int(torch.isnan(g).sum()), d.abs().max().item(), ulp, rows, cols,
        idx[:4].tolist(), g[bad][:4].tolist(), r[bad][:4].tolist()))


def to_out(y64, dtype):
    """float64 reference -> float32 -> the output dtype (torch rounds to nearest even)"""
    return y64.float().to(dtype)


@contextlib.contextmanager
def small_workspace(hip):
    """launches inside the block get a 16-byte workspace: too small for any split, so a split reduction takes the fp32-atomic path
    (include/gpv_hip.h: the workspace is optional)"""
    if not hasattr(hip, '_workspace'):
        yield
        return
    real, tiny = hip._workspace, {}

    def fake(dev, nbytes):
        return tiny.setdefault(str(dev), torch.zeros(16, dtype=torch.uint8, device=dev))
    hip._workspace = fake
    try:
        yield
    finally:
        hip._workspace = real


def seed_epoch():
    """the device seed epoch, if a trainer of this process installed one (csrc/common.h eff_seed)"""
    import gpv1_amd.ops as ops
    return None if ops.RT.seed_dev is None else int(ops.RT.seed_dev.item())


def keep_mask(seed, n, dev):
    from tests import dropout_ref as R
    return torch.from_numpy(R.keep_flat(R.eff_seed(seed, seed_epoch()), np.arange(n, dtype=np.uint64), DROP_P)).to(dev)


# =============================================================================================================== gpv_gemm
def gemm_case(family, M, N, K, **kw):
    """a gpv_gemm case.  out: output dtype; la / lb: operand layouts; epi: the exact epilogue terms, letters of 'sbrm' = rowscale, bias, res,
    relu_mask (True = all four), next to alpha and act; drop: dropout p = 0.5; acc: accumulate into an integer C0 with split_k, ws = with / without a workspace; rowsum:
    a_rowsum into an integer vector; kpitch: row pitch of a k-major A with zero padding + GPV_GEMM_KPAD_FINITE; precise: fp32 operands
    ('A' | 'B' = the operand that holds 12-bit integers, the other one [-7, 7]); pad: padding columns of C / res / mask rows"""
    c = dict(family=family, M=M, N=N, K=K, out=BF, la=KMAJOR, lb=KMAJOR, batch=1, epi='', alpha=1.0, act=ACT_NONE, drop=False, acc=False,
             split_k=1, ws=True, rowsum=False, kpitch=None, precise=None, pad=0, amax=3, bmax=3, seed=0, opts={}, counter=None, expect=None)
    c.update(kw)
    c['epi'] = 'sbrm' if c['epi'] is True else (c['epi'] or '')
    if c['acc']:
        c['out'] = F32
    if c['precise']:
        c['out'] = F32
        c['amax'], c['bmax'] = (2047, 7) if c['precise'] == 'A' else (7, 2047)
        return c                                        # (no fit: the lo halves need the 12 bits; the tables keep K within the bound)
    return fit(c, gemm_bound)


def gemm_bound(c):
    t = dict(K=c['K'], amax=c['amax'], bmax=c['bmax'], alpha=c['alpha'])
    if 's' in c['epi']:
        t.update(rsmax=4.0, rsmin=0.25)
    if 'b' in c['epi']:
        t.update(bias=8)
    if 'r' in c['epi']:
        t.update(res=16)
    if c['acc']:
        t.update(c0=8)
    if c['drop']:
        t.update(dscale=2.0)
    return exact_bound(t)


def _operand(logical, layout, ld, dtype, dev, poison):
    """logical [batch, rows, K] (float64) -> storage [batch, rows, ld] (k-major) or [batch, K, ld] (reduction-major); padding poisoned"""
    bt, rows, K = logical.shape
    if layout == KMAJOR:
        buf = torch.full((bt, rows, ld), poison, dtype=dtype, device=dev)
        buf[:, :, :K] = logical.to(dtype)
    else:
        buf = torch.full((bt, K, ld), poison, dtype=dtype, device=dev)
        buf[:, :, :rows] = logical.transpose(1, 2).to(dtype)
    return buf


def check_gemm(hip, c):
    assert gemm_bound(c) < LIMIT, ('precondition', gemm_bound(c), c)
    dev = device(hip)
    M, N, K, bt, sd = c['M'], c['N'], c['K'], c['batch'], c['seed']
    din, dout = (F32 if c['precise'] else BF), c['out']
    A = ints(bt, M, K, lo=-c['amax'], hi=c['amax'], seed=sd + 1, dev=dev)
    B = ints(bt, N, K, lo=-c['bmax'], hi=c['bmax'], seed=sd + 2, dev=dev)
    lda = (c['kpitch'] or K) if c['la'] == KMAJOR else M
    ldb = K if c['lb'] == KMAJOR else N
    Ab = _operand(A, c['la'], lda, din, dev, 0.0 if c['kpitch'] else float('nan'))
    Bb = _operand(B, c['lb'], ldb, din, dev, float('nan'))
    ld = N + c['pad']
    Cb = torch.full((bt, M, ld), float('nan'), dtype=dout, device=dev)
    Cb[:, :, N:] = SENTINEL
    y = c['alpha'] * (A @ B.transpose(1, 2))
    kw = {}
    mask = None
    if 's' in c['epi']:
        rs = pow2(M, sd + 3, dev)
        kw.update(rowscale=rs)
        y = y * rs.double()[None, :, None]
    if 'b' in c['epi']:
        bias = ints(N, lo=-8, hi=8, seed=sd + 4, dtype=F32, dev=dev)
        kw.update(bias=bias)
        y = y + bias.double()
    if 'r' in c['epi']:
        res = torch.full((bt, M, ld), float('nan'), dtype=dout, device=dev)
        res[:, :, :N] = ints(bt, M, N, lo=-16, hi=16, seed=sd + 5, dtype=dout, dev=dev)
        kw.update(res=res, ldr=ld, sR=M * ld)
        y = y + res[:, :, :N].double()
    if 'm' in c['epi']:
        mask = torch.full((M, ld), float('nan'), dtype=dout, device=dev)
        mask[:, :N] = sign_pattern(M, N, seed=sd + 6, dtype=dout, dev=dev)
        kw.update(relu_mask=mask, ldm=ld)
    if c['act'] == ACT_RELU:
        y = y.clamp_min(0)
    if c['drop']:
        seed = 0x5EED00 + sd
        kw.update(drop_p=DROP_P, seed=seed)
        y = y * keep_mask(seed, bt * M * N, dev).view(bt, M, N) * 2.0
    if mask is not None:
        y = y * (mask[:, :N].double() > 0)
    rowsum = ref_rowsum = None
    if c['acc']:
        c0 = ints(bt, M, N, lo=-8, hi=8, seed=sd + 7, dtype=F32, dev=dev)
        Cb[:, :, :N] = c0
        y = y + c0.double()
        kw.update(accumulate=True, split_k=c['split_k'])
        if c['rowsum']:
            rowsum = ints(M, lo=-8, hi=8, seed=sd + 8, dtype=F32, dev=dev)
            ref_rowsum = (rowsum.double() + A[0].sum(1)).float()
            kw.update(a_rowsum=rowsum)
    ref = to_out(y, dout)
    with contextlib.ExitStack() as st:
        if not c['ws']:
            st.enter_context(small_workspace(hip))
        hip.gemm(Ab, Bb, Cb, M, N, K, lda, ldb, ld, layoutA=c['la'], layoutB=c['lb'], batch=bt, sA=Ab[0].numel(), sB=Bb[0].numel(), sC=M * ld,
                 alpha=c['alpha'], act=c['act'], kpad_finite=bool(c['kpitch']), **kw)
    what = 'gemm %s' % {k: v for k, v in c.items() if k not in ('opts',)}
    assert_exact(Cb[:, :, :N], ref, what)
    assert bool((Cb[:, :, N:] == SENTINEL).all()), what + ': padding columns written'
    if rowsum is not None:
        assert_exact(rowsum, ref_rowsum, what + ' a_rowsum')


def _variants(family, M, N, K, f32_out=True, epi=True, pad=0, **kw):
    """plain bf16, plain fp32 output (strided), the full epilogue with ReLU"""
    out = [gemm_case(family, M, N, K, pad=pad, **kw)]
    if f32_out:
        out.append(gemm_case(family, M, N, K, out=F32, pad=8, seed=10, **kw))
    if epi:
        out.append(gemm_case(family, M, N, K, epi=True, alpha=0.5, act=ACT_RELU, pad=pad, seed=20, **kw))
    return out


PLAIN_SHAPES = [(300, 256, 256), (2048, 512, 768), (130, 70, 96), (64, 2, 256), (100, 48, 300), (9600, 256, 2048), (33, 200, 40)]      # test_gemm_nt_plain
RAGGED_SHAPES = [(257, 131, 100), (70, 66, 72), (129, 65, 104), (513, 100, 328), (77, 9, 20), (191, 257, 1000)]      # M, N off the tiles; K % 64, % 32, % 8 != 0
GLDS_SHAPES = [(300, 256, 256), (2048, 512, 768), (1000, 128, 192), (257, 130, 64), (9600, 256, 2048), (70, 384, 128), (513, 100, 320)]      # test_glds_gemm_plain
PIPE_CFGS = [(256, 128), (192, 128), (128, 128), (160, 256), (128, 256), (96, 256), (64, 64), (32, 64)]     # gemm_pipe.hip kCfgs (as tests/test_kernels_gpu.py)
PIPE_SHAPES = [(300, 256, 256), (2048, 512, 768), (1000, 128, 192), (70, 384, 128), (257, 768, 64), (192, 768, 768), (640, 2304, 768), (1, 768, 3072)]
SKINNY_SHAPES = [(192, 768, 768), (192, 768, 3072), (640, 2304, 768), (70, 130, 200), (1, 768, 768), (640, 768, 10000), (65, 64, 128), (300, 100, 8),
                 (300, 256, 2048), (100, 768, 3072), (640, 768, 768), (33, 40, 136)]                               # test_skinny_gemm
SKINNY_BT_SHAPES = [(3200, 256, 2048), (640, 768, 768), (3200, 256, 256), (70, 136, 200), (1, 768, 2048), (300, 64, 72)]      # test_skinny_gemm_reduction_major_b
GEMV_SHAPES = [(1, 768, 768), (1, 2304, 768), (1, 2048, 768), (1, 768, 2048), (1, 10000, 768), (2, 768, 3072), (3, 100, 96), (5, 2049, 520), (8, 4099, 768),
               (6, 768, 768), (1, 3, 8)]                                                                           # test_gemm_few_rows
C1S_LINEAR_SHAPES = [(9600, 2048), (3200, 2048), (9600, 1536), (2049, 1024)]                                       # the streaming kernel as a linear GEMM, K = 256
ACC_SHAPES = [(256, 2048, 9600), (768, 768, 3200), (72, 136, 777), (2304, 768, 192),                               # test_gemm_trans_layouts_and_splitk (M, N, K = rows)
              (256, 256, 9600), (768, 3072, 640), (2, 256, 3200), (100, 72, 333), (2048, 256, 3200)]               # test_gemm_wgrad_with_fused_bias_grad
REG = dict(GLDS=0, PIPE=0, SKINNY=0)
# the layout pairs gpv_gemm computes; the fourth, (TRANS, KMAJOR), has no kernel: the library returns hipErrorInvalidValue before any launch
# (csrc/gemm.hip gpv_gemm), which tests/test_exact_gpu.py asserts
LAYOUTS = [(KMAJOR, KMAJOR), (KMAJOR, TRANS), (TRANS, TRANS)]


def _gemm_table():
    t = []
    # register-staged kernel (gemm.hip) alone, and the default dispatch, on the plain and the ragged shapes
    for M, N, K in PLAIN_SHAPES + RAGGED_SHAPES:
        t += _variants('reg', M, N, K, pad=8, opts=REG)
        t += _variants('default', M, N, K, f32_out=False, pad=0)
    t.append(gemm_case('reg', 200, 192, 160, batch=3, epi=True, alpha=2.0, act=ACT_RELU, pad=8, opts=REG))
    t.append(gemm_case('reg', 200, 192, 160, batch=3, out=F32, epi=True, alpha=0.5, pad=8, opts=REG))
    for la, lb in LAYOUTS:
        t.append(gemm_case('reg', 300, 256, 100, la=la, lb=lb, batch=2, pad=8, seed=30, opts=REG))
        t.append(gemm_case('default', 100, 2048, 304, la=la, lb=lb, epi=True, alpha=2.0, seed=31))
    for fam, opts in (('reg', REG), ('default', {})):      # RoI pooling: K = 300 of a 320 pitch, the caller's promise of finite padding
        t.append(gemm_case(fam, 100, 2048, 300, lb=TRANS, kpitch=320, opts=opts))
        t.append(gemm_case(fam, 100, 2048, 300, lb=TRANS, kpitch=320, batch=2, out=F32, pad=8, opts=opts))
        t.append(gemm_case(fam, 100, 256, 300, kpitch=320, opts=opts))
        t.append(gemm_case(fam, 512, 512, 64, drop=True, opts=opts))
        t.append(gemm_case(fam, 200, 192, 160, drop=True, act=ACT_RELU, batch=2, seed=3, opts=opts))
    # direct-to-LDS kernels (gemm_glds.hip): 2 = 8 waves, 3 = 4 waves 128 x 128
    for mode in (2, 3):
        o = dict(GLDS=mode, SKINNY=0, PIPE=0)
        for M, N, K in GLDS_SHAPES:
            t.append(gemm_case('glds%d' % mode, M, N, K, opts=o, counter='GLDS', expect=1))
            t.append(gemm_case('glds%d' % mode, M, N, K, out=F32, pad=8, opts=o, counter='GLDS', expect=1))
            t.append(gemm_case('glds%d' % mode, M, N, K, epi=True, alpha=0.5, act=ACT_RELU, opts=o, counter='GLDS', expect=1))
        t.append(gemm_case('glds%d' % mode, 200, 192, 192, batch=3, epi=True, alpha=2.0, opts=o, counter='GLDS', expect=1))
        t.append(gemm_case('glds%d' % mode, 512, 256, 128, drop=True, opts=o, counter='GLDS', expect=1))
    # pipelined kernel (gemm_pipe.hip): every tile configuration
    for i, (bm, bn) in enumerate(PIPE_CFGS):
        o = dict(PIPE=100 + i, SKINNY=0)
        for M, N, K in PIPE_SHAPES + ([(9600, 256, 2048)] if i in (0, 3) else []):
            legal = int(N % bn == 0 and K >= 128)
            fam = 'pipe%dx%d' % (bm, bn)
            t.append(gemm_case(fam, M, N, K, opts=o, counter='PIPE', expect=legal))
            t.append(gemm_case(fam, M, N, K, epi=True, alpha=0.5, act=ACT_RELU, opts=o, counter='PIPE', expect=legal))
            if M <= 300:
                t.append(gemm_case(fam, M, N, K, drop=True, opts=o, counter='PIPE', expect=legal))
                t.append(gemm_case(fam, M, N, K, batch=3, epi=True, alpha=2.0, seed=4, opts=o, counter='PIPE'))
    # small-M kernel (gemm_skinny.hip), both B layouts
    o = dict(SKINNY=2, GLDS=0)
    for M, N, K in SKINNY_SHAPES:
        t += _variants('skinny', M, N, K, opts=o)
        if K >= 64:
            t.append(gemm_case('skinny', M, N, K, drop=True, seed=5, opts=o))
    for M, N, K in SKINNY_BT_SHAPES:
        t.append(gemm_case('skinny_bt', M, N, K, lb=TRANS, opts=o))
        t.append(gemm_case('skinny_bt', M, N, K, lb=TRANS, epi=True, alpha=2.0, seed=6, opts=o))
        t.append(gemm_case('skinny_bt', M, N, K, lb=TRANS, out=F32, pad=8, seed=7, opts=o))
    # few-row kernel (gemv.hip): declines rowscale / relu_mask / dropout, so its epilogue cases are alpha + bias + res + ReLU below
    for M, N, K in GEMV_SHAPES:
        took = 0 if (M > 2 and N >= 4096) else 1
        t.append(gemm_case('gemv', M, N, K, pad=24, counter='GEMV', expect=took))
        t.append(gemm_case('gemv', M, N, K, out=F32, pad=8, seed=8, counter='GEMV', expect=took))
        t.append(gemm_case('gemv', M, N, K, epi='br', alpha=0.5, act=ACT_RELU, pad=24, seed=9, counter='GEMV', expect=took))
    # streaming 1x1 kernel as a linear GEMM (conv1x1_stream.hip), K = 256
    for M, N in C1S_LINEAR_SHAPES:
        o = dict(C1S=2)
        t.append(gemm_case('c1s_linear', M, N, 256, epi='b', opts=o, counter='C1S', expect=1))
        t.append(gemm_case('c1s_linear', M, N, 256, epi='b', act=ACT_RELU, drop=True, seed=11, opts=o, counter='C1S', expect=1))
        t.append(gemm_case('c1s_linear', M, N, 256, epi='m', alpha=2.0, seed=12, opts=o, counter='C1S', expect=1))
        t.append(gemm_case('c1s_linear', M, N, 256, epi='brm', alpha=0.5, act=ACT_RELU, seed=13, opts=o, counter='C1S', expect=1))
    # accumulate into a nonzero integer C: split_k x {workspace, atomics}, a_rowsum, direct-to-LDS weight-gradient kernel off / forced
    for j, (M, N, K) in enumerate(ACC_SHAPES):
        for split in (1, 3, 8):
            for ws in (True, False):
                t.append(gemm_case('acc', M, N, K, la=TRANS, lb=TRANS, acc=True, split_k=split, ws=ws, rowsum=j >= 4, pad=8 if j % 2 else 0, seed=j))
    for M, N, K in [(256, 256, 9600), (768, 3072, 3200), (2048, 256, 3200), (256, 2048, 9600), (1536, 768, 3392), (768, 768, 10000), (128, 384, 1000)]:
        for mode in (0, 2):                                                                  # test_gemm_wgrad_direct_to_lds
            t.append(gemm_case('acc_glds_wgrad%d' % mode, M, N, K, la=TRANS, lb=TRANS, acc=True, split_k=8, rowsum=True, opts=dict(GLDS_WGRAD=mode)))
    t.append(gemm_case('acc', 300, 256, 256, acc=True, alpha=0.5, pad=8, opts=REG))                                     # k-major accumulate (C += through the epilogue)
    t.append(gemm_case('acc', 300, 256, 2048, acc=True, split_k=4, alpha=2.0, opts=REG))
    t.append(gemm_case('acc', 300, 256, 2048, acc=True, split_k=4, ws=False, opts=REG))
    # precise mode (fp32 operands split hi + lo on the fly): 12-bit integers x [-7, 7] and the swap; K keeps the bound
    for wide in ('A', 'B'):
        for M, N, K in [(300, 256, 256), (130, 70, 96), (64, 2, 256), (100, 48, 300), (33, 200, 40), (257, 131, 100), (2048, 512, 768)]:
            t.append(gemm_case('precise', M, N, K, precise=wide, pad=8, opts=REG))
        for M, N, K in [(1, 768, 768), (1, 2304, 768), (3, 100, 96), (5, 2049, 520), (8, 4099, 768), (6, 768, 768), (1, 3, 8)]:
            t.append(gemm_case('precise_gemv', M, N, K, precise=wide, counter='GEMV', expect=0 if (M > 2 and N >= 4096) else 1))
        t.append(gemm_case('precise', 100, 2048, 300, precise=wide, lb=TRANS, kpitch=320, opts=REG))
        t.append(gemm_case('precise', 72, 136, 777, precise=wide, la=TRANS, lb=TRANS, acc=True, split_k=3, opts=REG))
    return t


GEMM_CASES = _gemm_table()


# =============================================================================================================== gpv_conv2d
def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def conv_case(family, Cin, Cout, k, s, p, H, W, Bn=3, **kw):
    """a gpv_conv2d case over modes 0 (bias + res + ReLU [+ relu_mask]), 1 (res + relu_mask) and 2 (rowscale, integer dw to add to).
    bits: 'y' = the forward also writes y_mask_bits, 'm' = the backward-data reads relu_mask_bits"""
    c = dict(family=family, Cin=Cin, Cout=Cout, k=k, s=s, p=p, H=H, W=W, Bn=Bn, modes=(0, 1, 2), dtype=BF, res=True, mask=True, fwd_mask=False, act=ACT_RELU,
             bits='', split_k=0, amax=3, bmax=3, opts={}, counter=None, expect=None, seed=0)
    c.update(kw)
    if c['dtype'] == F32:
        c['amax'], c['bmax'] = 127, 7                   # precise mode: integers of at most 8 bits
    return fit(c, conv_bound)


def conv_geometry(c):
    OH, OW = (c['H'] + 2 * c['p'] - c['k']) // c['s'] + 1, (c['W'] + 2 * c['p'] - c['k']) // c['s'] + 1
    return OH, OW


def conv_bounds(c):
    """the bound of each mode the case runs: activations and gradients in [-amax, amax], weights in [-bmax, bmax]"""
    OH, OW = conv_geometry(c)
    T = c['k'] * c['k']
    b = {}
    if 0 in c['modes']:
        b[0] = exact_bound(dict(K=T * c['Cin'], amax=c['amax'], bmax=c['bmax'], bias=8, res=16 if c['res'] else 0))
    if 1 in c['modes']:
        b[1] = exact_bound(dict(K=T * c['Cout'], amax=c['amax'], bmax=c['bmax'], res=16 if c['res'] else 0))
    if 2 in c['modes']:
        b[2] = exact_bound(dict(K=c['Bn'] * OH * OW, amax=c['amax'], bmax=c['amax'], rsmax=4.0, rsmin=0.25, c0=8))
    return b


def conv_bound(c):
    return max(conv_bounds(c).values())


def conv_operands(c, dev):
    """integer x, w, dy (float64, NCHW / OIHW) of a case"""
    OH, OW = conv_geometry(c)
    sd = c['seed']
    x = ints(c['Bn'], c['Cin'], c['H'], c['W'], lo=-c['amax'], hi=c['amax'], seed=sd + 20, dev=dev)
    w = ints(c['Cout'], c['Cin'], c['k'], c['k'], lo=-c['bmax'], hi=c['bmax'], seed=sd + 21, dev=dev)
    dy = ints(c['Bn'], c['Cout'], OH, OW, lo=-c['amax'], hi=c['amax'], seed=sd + 25, dev=dev)
    return x, w, dy


def conv64(x, w, s, p):
    """F.conv2d on float64 tensors, spelled as unfold + matmul (every backend has both in float64; the values are exact integers, so
    the spelling does not matter)"""
    Bn, Cin, H, W = x.shape
    Cout, _, k, _ = w.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    cols = F.unfold(x, k, padding=p, stride=s)                          # [Bn, Cin k k, OH OW]
    return (w.reshape(Cout, Cin * k * k) @ cols).view(Bn, Cout, OH, OW)


def conv_refs(c, x, w, dy):
    """float64 forward product, input gradient and weight gradient"""
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    with torch.enable_grad():
        y = conv64(xr, wr, c['s'], c['p'])
        need = [t for t, m in ((xr, 1), (wr, 2)) if m in c['modes']]
        grads = torch.autograd.grad(y, need, dy) if need else ()
    grads = list(grads)
    gx = grads.pop(0) if 1 in c['modes'] else None
    gw = grads.pop(0) if 2 in c['modes'] else None
    return y.detach(), gx, gw


def _guarded(rows, cols, dtype, dev, fill=float('nan')):
    """[rows + 3, cols]: the launch gets the first `rows`, the three guard rows keep the sentinel"""
    buf = torch.full((rows + 3, cols), fill, dtype=dtype, device=dev)
    buf[rows:] = SENTINEL
    return buf


def pack_bits(y):
    from tests.test_kernels_gpu import _pack_bits
    return _pack_bits(y)


def check_conv(hip, c):
    assert conv_bound(c) < LIMIT, ('precondition', conv_bound(c), c)
    dev, dt = device(hip), c['dtype']
    Cin, Cout, k, s, p, H, W, Bn, sd = (c[n] for n in ('Cin', 'Cout', 'k', 's', 'p', 'H', 'W', 'Bn', 'seed'))
    OH, OW = conv_geometry(c)
    x, w, dy = conv_operands(c, dev)
    y64, gx, gw = conv_refs(c, x, w, dy)
    xn, dyn = nhwc(x).to(dt), nhwc(dy).to(dt)
    what = 'conv %s' % {n: v for n, v in c.items() if n != 'opts'}
    if 0 in c['modes']:
        wn = w.permute(0, 2, 3, 1).contiguous().to(dt)                 # [Cout][kh][kw][Cin]
        bias = ints(Cout, lo=-8, hi=8, seed=sd + 23, dtype=F32, dev=dev)
        res = nhwc(ints(Bn, Cout, OH, OW, lo=-16, hi=16, seed=sd + 24, dev=dev)).to(dt) if c['res'] else None
        msk = nhwc(sign_pattern(Bn, Cout, OH, OW, seed=sd + 28, dtype=dt, dev=dev)) if c['fwd_mask'] else None
        ref = nhwc(y64) + bias.double() + (res.double() if res is not None else 0)
        if c['act'] == ACT_RELU:
            ref = ref.clamp_min(0)
        if msk is not None:
            ref = ref * (msk.double() > 0)
        ref = to_out(ref, dt)
        px = Bn * OH * OW
        yb = _guarded(px, Cout, dt, dev)
        kw = {}
        if 'y' in c['bits']:
            bits = torch.full((px + 3, Cout // 32), 0x5a5a5a5a, device=dev, dtype=torch.int32)
            kw['y_mask_bits'] = bits[:px]
        hip.conv2d(0, xn, wn, yb[:px].view(Bn, OH, OW, Cout), Bn, H, W, Cin, Cin, OH, OW, Cout, k, k, s, s, p, p, bias=bias, res=res, relu_mask=msk,
                   act=c['act'], **kw)
        assert_exact(yb[:px].view(Bn, OH, OW, Cout), ref, what + ' forward')
        assert bool((yb[px:] == SENTINEL).all()), what + ': forward wrote past the output'
        if 'y' in c['bits']:
            assert torch.equal(bits[:px], pack_bits(ref.view(px, Cout))) and bool((bits[px:] == 0x5a5a5a5a).all()), what + ' y_mask_bits'
    if 1 in c['modes']:
        wd = w.permute(1, 2, 3, 0).contiguous().to(dt)                 # [Cin][kh][kw][Cout]
        add = nhwc(ints(Bn, Cin, H, W, lo=-16, hi=16, seed=sd + 26, dev=dev)).to(dt) if c['res'] else None
        saved = nhwc(sign_pattern(Bn, Cin, H, W, seed=sd + 27, dtype=dt, dev=dev)) if c['mask'] else None
        ref = nhwc(gx) + (add.double() if add is not None else 0)
        if saved is not None:
            ref = ref * (saved.double() > 0)
        ref = to_out(ref, dt)
        px = Bn * H * W
        dxb = _guarded(px, Cin, dt, dev)
        kw = dict(relu_mask=saved)
        if 'm' in c['bits']:
            kw = dict(relu_mask_bits=pack_bits(saved.view(px, Cin)))
        hip.conv2d(1, dyn, wd, dxb[:px].view(Bn, H, W, Cin), Bn, OH, OW, Cout, Cout, H, W, Cin, k, k, s, s, p, p, res=add, **kw)
        assert_exact(dxb[:px].view(Bn, H, W, Cin), ref, what + ' backward-data')
        assert bool((dxb[px:] == SENTINEL).all()), what + ': backward-data wrote past the output'
    if 2 in c['modes']:
        scale = pow2(Cout, sd + 22, dev)
        rows = Cout * k * k
        dwb = _guarded(rows, Cin, F32, dev)
        c0 = ints(Cout, k, k, Cin, lo=-8, hi=8, seed=sd + 29, dtype=F32, dev=dev)
        dwb[:rows] = c0.view(rows, Cin)
        ref = (c0.double() + (gw * scale.double().view(-1, 1, 1, 1)).permute(0, 2, 3, 1)).float()
        hip.conv2d(2, xn, dyn, dwb[:rows].view(Cout, k, k, Cin), Bn, H, W, Cin, Cin, OH, OW, Cout, k, k, s, s, p, p, rowscale=scale, split_k=c['split_k'])
        assert_exact(dwb[:rows].view(Cout, k, k, Cin), ref, what + ' weight gradient')
        assert bool((dwb[rows:] == SENTINEL).all()), what + ': weight gradient wrote past the output'


CONVS = [(64, 64, 1, 1, 0, 24, 32), (256, 128, 3, 2, 1, 24, 32), (128, 128, 3, 1, 1, 15, 20), (256, 512, 1, 2, 0, 30, 40), (512, 2048, 1, 1, 0, 15, 20),
         (64, 64, 3, 1, 1, 17, 23)]                                                                                        # tests/test_kernels_gpu.py CONVS
GCONVS = [(64, 128, 1, 1, 0, 24, 32), (256, 128, 3, 2, 1, 24, 32), (128, 128, 3, 1, 1, 15, 20), (256, 512, 1, 2, 0, 30, 40), (512, 2048, 1, 1, 0, 15, 20),
          (128, 256, 3, 2, 1, 17, 23), (128, 192, 3, 2, 1, 32, 32)]                                                        # ... GCONVS
HALO = [(256, 256, 30, 40, 32), (512, 512, 15, 20, 32), (128, 256, 29, 43, 32), (64, 256, 47, 47, 16), (192, 128, 9, 21, 240), (128, 128, 1, 47, 800),
        (128, 256, 40, 1, 900), (128, 128, 2, 2, 9600)]                                                                    # test_conv3x3_halo_image_kernel
C3S = [(64, 64, 1, 24, 32, 3), (64, 64, 1, 17, 23, 3), (128, 128, 1, 15, 20, 3), (128, 128, 2, 24, 32, 2), (128, 128, 2, 30, 34, 1), (64, 128, 2, 16, 62, 3),
       (64, 128, 2, 10, 64, 2), (64, 64, 1, 7, 61, 2), (128, 64, 1, 9, 40, 2), (64, 128, 1, 8, 8, 5)]                      # test_streaming_3x3_conv_kernel_forced
C1S_FWD = [(64, 256, 30, 40, 2, True, False, True), (64, 256, 30, 40, 2, False, False, True), (64, 64, 17, 23, 3, False, False, True),
           (256, 64, 30, 40, 2, False, True, False), (128, 512, 15, 20, 2, True, False, True), (128, 512, 15, 20, 2, True, True, False),
           (256, 128, 21, 19, 1, False, False, True), (256, 256, 9, 11, 5, True, True, True), (128, 128, 7, 5, 1, False, True, False),
           (512, 128, 15, 20, 2, False, False, True), (512, 128, 15, 20, 2, True, True, False), (512, 64, 9, 7, 3, False, True, False),
           (256, 1024, 15, 20, 2, True, False, True), (256, 1024, 9, 7, 1, True, True, False), (128, 2048, 5, 6, 1, False, False, True)]     # test_streaming_1x1_conv_kernel_forced
C1S_S2 = [(256, 512, 30, 40, 2), (512, 1024, 14, 18, 2), (64, 256, 9, 13, 3), (256, 128, 8, 6, 1)]                         # test_streaming_1x1_conv_stride2_forward
C1S_YBITS = [(128, 512, 4813), (256, 1024, 2400), (256, 512, 1000), (128, 512, 16), (256, 1024, 33)]                       # test_streaming_1x1_writes_one_bit_relu_masks (K, N, px)
C1S_MBITS = [(128, 512, 4813), (256, 1024, 2400), (256, 512, 777), (512, 1024, 1200), (512, 1024, 50)]                     # ..._backward_data_reads_one_bit_relu_masks
BATCH1 = [(512, 512, 3, 1, 15, 20), (256, 256, 3, 1, 30, 40), (256, 256, 3, 2, 60, 80), (128, 128, 3, 1, 60, 80), (1024, 256, 1, 1, 30, 40), (2048, 512, 1, 1, 15, 20),
          (512, 2048, 1, 1, 15, 20)]                                                                                       # test_conv_forward_at_batch_one
TWO_PER_CU = [(64, 256, 3, 50, 80, 8), (64, 512, 3, 30, 40, 8), (512, 256, 1, 50, 80, 8)]                                  # test_conv_two_tiles_per_cu_variants
WGRAD_GLDS = [(128, 128, 3, 1, 1, 30, 40, 4), (256, 256, 3, 2, 1, 30, 40, 4), (512, 128, 1, 1, 0, 15, 20, 5), (256, 512, 1, 2, 0, 30, 40, 3),
              (128, 256, 3, 1, 1, 8, 24, 6)]                                                                               # test_conv_wgrad_direct_to_lds_vs_register_staged
S2_DGRAD = [(256, 512, 32, 32, 4), (512, 1024, 32, 32, 4), (256, 512, 32, 64, 8), (1024, 2048, 16, 32, 8)]                 # test_conv1x1_stride2_dgrad_class_rows_multiple_of_tile


def _conv_table():
    t = []
    for a in CONVS:
        t.append(conv_case('default', *a))
        t.append(conv_case('precise', *a, dtype=F32))
        t.append(conv_case('reg', *a, opts=REG))
    for a in GCONVS:
        Cin, Cout, k = a[:3]
        for i, (bm, bn) in enumerate(PIPE_CFGS[:6]):
            want = int(Cout % bn == 0 and k * k * Cin >= 128) + int(Cin % bn == 0 and k * k * Cout >= 128)
            t.append(conv_case('pipe%dx%d' % (bm, bn), *a, modes=(0, 1), opts=dict(PIPE=100 + i, SKINNY=0), counter='PIPE', expect=want))
        for mode in (2, 3):
            t.append(conv_case('glds%d' % mode, *a, modes=(0, 1), opts=dict(GLDS=mode, SKINNY=0, PIPE=0), counter='GLDS', expect=int(Cout > 64) + int(Cin > 64)))
    for Cin, Cout, H, W, Bn in S2_DGRAD:
        for fam, opts in (('default', {}), ('glds3', dict(PIPE=0, GLDS=3)), ('glds2', dict(PIPE=0, GLDS=2)), ('reg', dict(PIPE=0, GLDS=0))):
            t.append(conv_case(fam, Cin, Cout, 1, 2, 0, H, W, Bn, modes=(1,), opts=opts))
    for Cin, Cout, k, H, W, Bn in TWO_PER_CU:
        t.append(conv_case('two_per_cu', Cin, Cout, k, 1, k // 2, H, W, Bn, modes=(0, 1), counter='GLDS', expect='>=1'))
    for mode in (1, 2):
        for Cin, Cout, H, W, Bn in HALO:
            t.append(conv_case('halo%d' % mode, Cin, Cout, 3, 1, 1, H, W, Bn, modes=(0, 1), opts=dict(C3_HALO=mode), counter='C3_HALO',
                               expect=('>=1' if mode == 2 or (Cin, Cout) == (256, 256) else None)))
    for Cin, Cout, s, H, W, Bn in C3S:
        bwd = s == 1 or (Cout == 128 and H % 2 == 0 and W % 2 == 0)
        t.append(conv_case('c3s', Cin, Cout, 3, s, 1, H, W, Bn, modes=(0, 1), res=False, opts=dict(C3S=2), counter='C3S', expect=int(s == 1) + int(bwd)))
        t.append(conv_case('c3s', Cin, Cout, 3, s, 1, H, W, Bn, modes=(1,), res=False, mask=False, act=ACT_NONE, seed=1, opts=dict(C3S=2), counter='C3S', expect=int(bwd)))
    for Bn, OH, OW in [(2, 16, 24), (1, 9, 33), (3, 30, 40)]:                  # stride-2 3x3 backward-data over 128 channels reading one-bit masks
        t.append(conv_case('c3s_bits', 128, 128, 3, 2, 1, 2 * OH, 2 * OW, Bn, modes=(1,), res=False, bits='m', opts=dict(C3S=2), counter='C3S', expect=1))
    for Cin, Cout, H, W, Bn, with_res, with_mask, relu in C1S_FWD:
        t.append(conv_case('c1s', Cin, Cout, 1, 1, 0, H, W, Bn, modes=(0,), res=with_res, fwd_mask=with_mask, act=ACT_RELU if relu else ACT_NONE,
                           opts=dict(C1S=2, SKINNY=0), counter='C1S', expect=1))
    for Cin, Cout, H, W, Bn in C1S_S2:
        t.append(conv_case('c1s_s2', Cin, Cout, 1, 2, 0, H, W, Bn, modes=(0,), res=False, act=ACT_NONE, opts=dict(C1S=2), counter='C1S', expect=1))
        t.append(conv_case('c1s_s2', Cin, Cout, 1, 2, 0, H, W, Bn, modes=(0,), res=True, act=ACT_RELU, seed=2, opts=dict(C1S=2)))
    for K, N, px in C1S_YBITS:
        t.append(conv_case('c1s_bits', K, N, 1, 1, 0, 1, px, 1, modes=(0,), bits='y', opts=dict(C1S=2), counter='C1S', expect=1))
    for K, N, px in C1S_MBITS:                                                 # backward-data of conv1: gathered tensor has K channels, dx N
        t.append(conv_case('c1s_bits', N, K, 1, 1, 0, 1, px, 1, modes=(1,), bits='m', opts=dict(C1S=2), counter='C1S', expect=1))
        t.append(conv_case('c1s_bits', N, K, 1, 1, 0, 1, px, 1, modes=(1,), res=False, seed=3, opts=dict(C1S=2)))
    for Cin, Cout, k, s, H, W in BATCH1:                                       # forward split reduction through the workspace (+ the small-M 1x1s)
        for Bn in (1, 2):
            t.append(conv_case('batch1', Cin, Cout, k, s, k // 2, H, W, Bn))
    for a in WGRAD_GLDS:
        for mode in (0, 2):
            for split in (0, 4):
                t.append(conv_case('wgrad_glds%d' % mode, *a, modes=(2,), split_k=split, opts=dict(GLDS_WGRAD=mode)))
    return t


CONV_CASES = _conv_table()


# =============================================================================================================== gpv_conv_wgrad_group
WGROUP_LISTS = {
    'mixed': [(512, 512, 3, 1, 1, 15, 20, 4), (256, 256, 3, 1, 1, 30, 40, 32), (128, 128, 3, 2, 1, 60, 80, 8), (512, 128, 1, 1, 0, 15, 20, 5),
              (256, 1024, 1, 1, 0, 30, 40, 16), (64, 128, 3, 1, 1, 30, 40, 4), (128, 256, 3, 1, 1, 8, 24, 6)],               # test_conv_wgrad_group_equals_single_launches
    'eight_phase': [(512, 512, 3, 1, 1, 15, 20, 4), (256, 256, 3, 1, 1, 30, 40, 32), (256, 256, 3, 2, 1, 60, 80, 8), (256, 512, 1, 1, 0, 15, 20, 5),
                    (1024, 256, 1, 1, 0, 30, 40, 16), (512, 1024, 1, 2, 0, 30, 40, 8), (256, 256, 3, 1, 1, 8, 24, 3), (256, 256, 1, 1, 0, 16, 32, 1)],
    'half_width': [(128, 128, 3, 1, 1, 60, 80, 2), (128, 128, 3, 1, 1, 60, 80, 8), (128, 128, 3, 2, 1, 120, 160, 2), (512, 128, 1, 1, 0, 60, 80, 4),
                   (128, 512, 1, 1, 0, 60, 80, 4), (256, 512, 1, 2, 0, 120, 160, 2), (256, 128, 1, 1, 0, 120, 160, 2), (128, 384, 3, 1, 1, 8, 24, 3),
                   (384, 128, 1, 1, 0, 16, 32, 1), (128, 256, 3, 1, 1, 15, 20, 5), (64, 128, 1, 1, 0, 24, 32, 2)]}           # (the last one: Cin = 64, refused by the grouped kernel)
WGROUP_CASES = {name: [conv_case('wgroup', *a[:7], a[7], modes=(2,), seed=100 + 7 * i) for i, a in enumerate(lst)] for name, lst in WGROUP_LISTS.items()}


def wgroup_problems(cases, dev):
    """operands and float64-derived references of a problem list (built once, the launches below accumulate into fresh copies)"""
    out = []
    for c in cases:
        x, w, dy = conv_operands(c, dev)
        _, _, gw = conv_refs(c, x, w, dy)
        scale = pow2(c['Cout'], c['seed'] + 22, dev)
        c0 = ints(c['Cout'], c['k'], c['k'], c['Cin'], lo=-8, hi=8, seed=c['seed'] + 29, dtype=F32, dev=dev)
        ref = (c0.double() + (gw * scale.double().view(-1, 1, 1, 1)).permute(0, 2, 3, 1)).float()
        out.append((c, nhwc(x).to(BF), nhwc(dy).to(BF), scale, c0, ref))
    return out


def check_wgrad_group(hip, prepared):
    probs, bufs = [], []
    for c, xn, dyn, scale, c0, ref in prepared:
        OH, OW = conv_geometry(c)
        rows = c['Cout'] * c['k'] * c['k']
        buf = _guarded(rows, c['Cin'], F32, c0.device)
        buf[:rows] = c0.view(rows, c['Cin'])
        bufs.append(buf)
        probs.append((xn, dyn, buf[:rows].view(c['Cout'], c['k'], c['k'], c['Cin']), scale, c['Bn'], c['H'], c['W'], c['Cin'], c['Cin'], OH, OW, c['Cout'],
                      c['k'], c['k'], c['s'], c['s'], c['p'], c['p']))
    hip.conv_wgrad_group(probs)
    for (c, *_r, ref), q, buf in zip(prepared, probs, bufs):
        what = 'conv_wgrad_group %s' % {n: c[n] for n in ('Cin', 'Cout', 'k', 's', 'H', 'W', 'Bn')}
        assert_exact(q[2], ref, what)
        assert bool((buf[q[2].numel() // c['Cin']:] == SENTINEL).all()), what + ': wrote past the gradient'


# =============================================================================================================== gpv_gemm_tt_group(_ws)
TT_SHAPES = {      # (K, M, N): dW[M, N] += dY[K, M]^T X[K, N]
    'plain': ([(192, 768, 768), (640, 768, 2048), (3200, 256, 256), (3200, 2048, 256), (100, 128, 384), (1000, 384, 128), (64, 128, 128), (3392, 1536, 768)], 7),
    'eight_phase': ([(9600, 256, 256), (9600, 256, 2048), (9600, 2048, 256), (9600, 512, 256), (3200, 768, 768), (3392, 1536, 768), (3200, 768, 3072), (640, 768, 768),
                     (192, 768, 768), (1000, 256, 256), (130, 256, 512), (3200, 256, 256), (3200, 256, 256), (3200, 256, 256)], 5)}


def tt_cases(name):
    shapes, reps = TT_SHAPES[name]
    return [fit(dict(K=K, M=M, N=N, amax=3, bmax=3, c0=8, seed=1000 + 20 * rep + i, bias_grad=i % 2 == 0))
            for rep in range(reps) for i, (K, M, N) in enumerate(shapes)]


def check_tt_group(hip, cases, dev=None):
    """dW is a row slice of a larger integer buffer whose other rows must stay; every second problem has a bias gradient"""
    dev = dev or device(hip)
    probs, refs = [], []
    for c in cases:
        K, M, N, sd = c['K'], c['M'], c['N'], c['seed']
        dy, x = ints(K, M, lo=-c['amax'], hi=c['amax'], seed=sd, dev=dev), ints(K, N, lo=-c['bmax'], hi=c['bmax'], seed=sd + 1, dev=dev)
        big = ints(M + 128, N, lo=-8, hi=8, seed=sd + 2, dtype=F32, dev=dev)
        bg = ints(M, lo=-8, hi=8, seed=sd + 3, dtype=F32, dev=dev) if c['bias_grad'] else None
        want = big.clone()
        want[64:64 + M] = (big[64:64 + M].double() + dy.t() @ x).float()
        refs.append((want, None if bg is None else (bg.double() + dy.sum(0)).float()))
        dyb, xb = dy.to(BF), x.to(BF)
        assert hip.tt_group_ok(dyb, xb, big[64:64 + M], M, N, K, M, N, N)
        probs.append((dyb, xb, big[64:64 + M], bg, M, N, K, M, N, N, big))
    hip.gemm_tt_group([q[:10] for q in probs])
    for q, (want, wantb), c in zip(probs, refs, cases):
        assert_exact(q[10], want, 'gemm_tt_group %s' % c)
        if wantb is not None:
            assert_exact(q[3], wantb, 'gemm_tt_group bias gradient %s' % c)


# =============================================================================================================== fused block tails
DUAL = [(64, 64, 256, 1, 24, 32, 3), (64, 64, 256, 1, 7, 9, 5), (128, 256, 512, 2, 15, 20, 3), (128, 256, 512, 2, 8, 6, 2)]      # test_fused_block_tail_conv3_plus_downsample
DUAL_CASES = [fit(dict(K1=K1, K2=K2, N=N, s2=s2, OH=OH, OW=OW, Bn=Bn, K=K1 + K2, amax=3, bmax=3, bias=8, bits=b))
              for (K1, K2, N, s2, OH, OW, Bn) in DUAL for b in ((False, True) if (K1, K2, N) == (128, 256, 512) else (False,))]


def check_dual(hip, c):
    dev = device(hip)
    K1, K2, N, s2, OH, OW, Bn = (c[n] for n in ('K1', 'K2', 'N', 's2', 'OH', 'OW', 'Bn'))
    IH = max(OH * s2 - (s2 - 1) * (OH % 2), (OH - 1) * s2 + 1)
    IW = OW * s2
    a2 = ints(Bn, OH, OW, K1, lo=-c['amax'], hi=c['amax'], seed=70, dev=dev)
    x = ints(Bn, IH, IW, K2, lo=-c['amax'], hi=c['amax'], seed=71, dev=dev)
    w3, wd = ints(N, K1, lo=-c['bmax'], hi=c['bmax'], seed=72, dev=dev), ints(N, K2, lo=-c['bmax'], hi=c['bmax'], seed=73, dev=dev)
    bias = ints(N, lo=-8, hi=8, seed=74, dtype=F32, dev=dev)
    px = Bn * OH * OW
    yb = _guarded(px, N, BF, dev)
    ref = to_out((a2 @ w3.t() + x[:, ::s2, ::s2][:, :OH, :OW] @ wd.t() + bias.double()).clamp_min(0), BF)
    kw = {}
    if c['bits']:
        bits = torch.full((px + 2, N // 32), 0x5a5a5a5a, device=dev, dtype=torch.int32)
        kw['y_mask_bits'] = bits[:px]
    assert hip.conv1x1_dual(a2.to(BF), w3.to(BF), x.to(BF), wd.to(BF), bias, yb[:px].view(Bn, OH, OW, N), Bn, OH, OW, K1, IH, IW, K2, s2, N, ACT_RELU, **kw)
    assert_exact(yb[:px].view(Bn, OH, OW, N), ref, 'conv1x1_dual %s' % c)
    assert bool((yb[px:] == SENTINEL).all())
    if c['bits']:
        assert torch.equal(bits[:px], pack_bits(ref.view(px, N))) and bool((bits[px:] == 0x5a5a5a5a).all()), 'conv1x1_dual_bits %s' % c


def chain_case(branch, N2, OH, OW, Bn, bits=False):
    """y = relu(a w3^T (+ x wd^T | + x) + b3) rounded to bf16, z = relu(y wn^T + bn): the rounded y are integers, |y| <= by (1 + 2^-8)"""
    c = dict(branch=branch, N2=N2, OH=OH, OW=OW, Bn=Bn, bits=bits, amax=3, bmax=3)
    while True:
        c['by'] = exact_bound(dict(K=64 * (2 if branch == 'downsample' else 1), amax=c['amax'], bmax=c['bmax'], bias=8, res=16 if branch == 'identity' else 0))
        c['bz'] = exact_bound(dict(K=256, amax=math.ceil(c['by'] * (1 + 2.0 ** -8)), bmax=c['bmax'], bias=8))
        if c['bz'] < LIMIT or c['bmax'] == 1:
            return c
        c['bmax'] -= 1


CHAIN_CASES = [chain_case(br, N2, OH, OW, Bn) for br in ('identity', 'downsample', 'plain') for (N2, OH, OW, Bn) in [(64, 24, 32, 3), (128, 7, 9, 5), (64, 120, 160, 2)]] + \
              [chain_case('identity', 128, 7, 9, 5, bits=True), chain_case('identity', 128, 24, 32, 3, bits=True)]


def check_chain(hip, c):
    dev = device(hip)
    K1, N, N2, OH, OW, Bn, br = 64, 256, c['N2'], c['OH'], c['OW'], c['Bn'], c['branch']
    a = ints(Bn, OH, OW, K1, lo=-c['amax'], hi=c['amax'], seed=170, dev=dev)
    w3 = ints(N, K1, lo=-c['bmax'], hi=c['bmax'], seed=171, dev=dev)
    b3, bn_ = ints(N, lo=-8, hi=8, seed=172, dtype=F32, dev=dev), ints(N2, lo=-8, hi=8, seed=174, dtype=F32, dev=dev)
    wn = ints(N2, N, lo=-c['bmax'], hi=c['bmax'], seed=173, dev=dev)
    x = ints(Bn, OH, OW, N if br == 'identity' else 64, lo=-16 if br == 'identity' else -c['amax'], hi=16 if br == 'identity' else c['amax'], seed=175, dev=dev)
    wd = ints(N, 64, lo=-c['bmax'], hi=c['bmax'], seed=176, dev=dev)
    y64 = a @ w3.t() + b3.double()
    if br == 'identity':
        y64 = y64 + x
    elif br == 'downsample':
        y64 = y64 + x @ wd.t()
    yref = to_out(y64.clamp_min(0), BF)
    assert float(yref.float().abs().max()) <= c['by'] * (1 + 2.0 ** -8)
    zref = to_out((yref.double() @ wn.t() + bn_.double()).clamp_min(0), BF)
    px = Bn * OH * OW
    yb, zb = _guarded(px, N, BF, dev), _guarded(px, N2, BF, dev)
    kw = {}
    if c['bits']:
        bits = torch.full((px + 2, N2 // 32), 0x5a5a5a5a, device=dev, dtype=torch.int32)
        kw['z_mask_bits'] = bits[:px]
    a2_, w2_ = (x.to(BF), wd.to(BF)) if br == 'downsample' else (None, None)
    assert hip.conv1x1_chain(a.to(BF), w3.to(BF), a2_, w2_, 1, x.to(BF) if br == 'identity' else None, b3, yb[:px].view(Bn, OH, OW, N), wn.to(BF), bn_,
                             zb[:px].view(Bn, OH, OW, N2), Bn, OH, OW, **kw)
    assert_exact(yb[:px].view(Bn, OH, OW, N), yref, 'conv1x1_chain y %s' % c)
    assert_exact(zb[:px].view(Bn, OH, OW, N2), zref, 'conv1x1_chain z %s' % c)
    assert bool((yb[px:] == SENTINEL).all()) and bool((zb[px:] == SENTINEL).all())
    if c['bits']:
        assert torch.equal(bits[:px], pack_bits(zref.view(px, N2))) and bool((bits[px:] == 0x5a5a5a5a).all()), 'conv1x1_chain_bits %s' % c


# =============================================================================================================== stem
STEM_CASES = [fit(dict(Bn=Bn, H=H, W=W, K=147, amax=8, bmax=3, bias=8)) for Bn, H, W in [(2, 96, 128), (3, 62, 90), (1, 480, 640), (2, 34, 30)]]


def check_stem(hip, c):
    """gpv_stem_pool, and the unfused conv + gpv_maxpool3x3s2 path, against float64 conv 7x7/2 + shift + ReLU (rounded) + max-pool"""
    dev = device(hip)
    Bn, H, W = c['Bn'], c['H'], c['W']
    img = ints(Bn, 3, H, W, lo=-c['amax'], hi=c['amax'], seed=30, dev=dev)
    w = ints(64, 3, 7, 7, lo=-c['bmax'], hi=c['bmax'], seed=31, dev=dev)
    bias = ints(64, lo=-8, hi=8, seed=32, dtype=F32, dev=dev)
    OH, OW = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    Hp, Wp = H + 6, ((max(W + 6, 2 * (OW - 1) + 8) + 7) // 8) * 8
    xin = torch.full((Bn, Hp, Wp, 4), float('nan'), device=dev, dtype=BF)
    hip.image_to_nhwc4(img.float(), xin, Bn, H, W, 3, Hp, Wp)
    want_in = torch.zeros(Bn, Hp, Wp, 4, device=dev, dtype=BF)
    want_in[:, 3:3 + H, 3:3 + W, :3] = img.permute(0, 2, 3, 1).to(BF)
    assert_exact(xin, want_in, 'image_to_nhwc4 %s' % c)
    ws = torch.zeros(64, 7, 8, 4, device=dev, dtype=torch.float64)
    ws[:, :, :7, :3] = w.permute(0, 2, 3, 1)
    ws = ws.reshape(64, 7, 32).to(BF).contiguous()
    conv = to_out((conv64(img, w, 2, 3) + bias.double().view(1, -1, 1, 1)).clamp_min(0), BF)
    ref = nhwc(F.max_pool2d(conv.double(), 3, 2, 1)).to(BF)
    PH, PW = (OH + 2 - 3) // 2 + 1, (OW + 2 - 3) // 2 + 1
    zb = _guarded(Bn * PH * PW, 64, BF, dev)
    z = zb[:Bn * PH * PW].view(Bn, PH, PW, 64)
    hip.stem_pool(xin, ws, bias, z, Bn, Hp, Wp, OH, OW, PH, PW)
    assert_exact(z, ref, 'stem_pool %s' % c)
    assert bool((zb[Bn * PH * PW:] == SENTINEL).all())
    yb = _guarded(Bn * OH * OW, 64, BF, dev)
    y = yb[:Bn * OH * OW].view(Bn, OH, OW, 64)
    hip.conv2d(0, xin, ws.view(64, 7, 1, 32), y, Bn, Hp, Wp, 4, 32, OH, OW, 64, 7, 1, 2, 2, 0, 0, bias=bias, act=ACT_RELU)
    assert_exact(y, nhwc(conv), 'stem conv %s' % c)
    assert bool((yb[Bn * OH * OW:] == SENTINEL).all())
    z2 = torch.full_like(z, float('nan'))
    hip.maxpool3x3s2(y, z2, Bn, OH, OW, 64, PH, PW)
    assert_exact(z2, ref, 'maxpool3x3s2 %s' % c)


# =============================================================================================================== exact outputs of fused launches
LINEAR_LN_CASES = [fit(dict(rows=r, K=256, amax=3, bmax=3, bias=8)) for r in (9600, 3200, 300, 100, 37, 16, 4099)]
QKV_CASES = [fit(dict(Bn=Bn, S=S, K=256, amax=2, bmax=2, bias=8)) for Bn, S in [(32, 300), (3, 300), (2, 100), (32, 100), (2, 37), (1, 320), (2, 129), (5, 16)]]


def check_linear_ln_s(hip, c):
    """the `s` output of gpv_linear_layernorm_fwd: projection + bias, rounded to bf16 (y and the statistics stay with the tolerance tests)"""
    dev, rows, D = device(hip), c['rows'], 256
    a, w = ints(rows, D, lo=-c['amax'], hi=c['amax'], seed=41, dev=dev), ints(D, D, lo=-c['bmax'], hi=c['bmax'], seed=43, dev=dev)
    bias = ints(D, lo=-8, hi=8, seed=44, dtype=F32, dev=dev)
    x = ints(rows, D, lo=-3, hi=3, seed=42, dtype=BF, dev=dev)
    gamma, beta = torch.ones(D, device=dev), torch.zeros(D, device=dev)
    sb = _guarded(rows, D, BF, dev)
    y = torch.full((rows, D), float('nan'), device=dev, dtype=BF)
    mean, rstd = torch.empty(rows, device=dev), torch.empty(rows, device=dev)
    hip.linear_layernorm_fwd(a.to(BF), w.to(BF), bias, x, gamma, beta, sb[:rows], y, mean, rstd, rows, 1e-5)
    assert_exact(sb[:rows], to_out(a @ w.t() + bias.double(), BF), 'linear_layernorm_fwd s %s' % c)
    assert bool((sb[rows:] == SENTINEL).all())


def check_attention_qkv(hip, c):
    """the q / k / v outputs of gpv_attention_qkv_fwd (o and lse stay with the tolerance tests)"""
    dev, Bn, S, H, dh, D = device(hip), c['Bn'], c['S'], 8, 32, 256
    M = Bn * S
    xp, x = ints(M, D, lo=-c['amax'], hi=c['amax'], seed=31, dev=dev), ints(M, D, lo=-c['amax'], hi=c['amax'], seed=32, dev=dev)
    w = ints(3 * D, D, lo=-c['bmax'], hi=c['bmax'], seed=33, dev=dev)
    bias = ints(3 * D, lo=-8, hi=8, seed=34, dtype=F32, dev=dev)
    qkb, vb = _guarded(M, 2 * D, BF, dev), _guarded(M, D, BF, dev)
    qk, v = qkb[:M], vb[:M]
    o = torch.full((M, D), float('nan'), device=dev, dtype=BF)
    lse = torch.empty(Bn, H, S, device=dev)
    st = ((S * 2 * D, 2 * D), (S * 2 * D, 2 * D), (S * D, D), (S * D, D))
    hip.attention_qkv_fwd(xp.to(BF), x.to(BF), w.to(BF), bias, qk[:, :D], qk[:, D:], v, o, st, Bn, H, S, dh ** -0.5, lse=lse)
    assert_exact(qk, to_out(xp @ w[:2 * D].t() + bias[:2 * D].double(), BF), 'attention_qkv_fwd q | k %s' % c)
    assert_exact(v, to_out(x @ w[2 * D:].t() + bias[2 * D:].double(), BF), 'attention_qkv_fwd v %s' % c)
    assert bool((qkb[M:] == SENTINEL).all()) and bool((vb[M:] == SENTINEL).all())


# =============================================================================================================== fp32 reductions
COLSUM_CASES = [fit(dict(rows=r, cols=cdim, ld=ld, dtype=dt, K=r, amax=(3 if dt == BF else 2000), bmax=1, c0=8))
                for r, cdim, ld, dt in [(777, 256, 256, BF), (32, 25600, 25600, BF), (9600, 256, 512, BF), (5, 24, 24, F32), (33, 100, 100, BF), (640, 768, 768, F32)]]
FOLD_CASES = [fit(dict(K=nblk, nblk=nblk, cols=cols, amax=2000, bmax=1, c0=8)) for nblk, cols in [(150, 256), (62, 768), (2, 2048), (1, 2048), (300, 256)]]
SUMSQ_CASES = [fit(dict(K=n, n=n, amax=3, bmax=3, c0=8)) for n in (10007, 4096, 1, 1 << 20)]
CLIP_CASES = [dict(n=n, max_norm=mx, amax=3, bmax=3, K=4 * ((n // 4 + 1023) // 1024)) for n, mx in [(4 * 1000 + 4, 0.1), (1 << 22, 0.1), (4096, 1e9), (8, 0.5)]]
#   (gpv_clip_scale: K = the elements of ONE of its 1024 fp32 partial sums; the partials are added in double)


def check_colsum(hip, c):
    dev = device(hip)
    x = ints(c['rows'], c['ld'], lo=-c['amax'], hi=c['amax'], seed=76, dev=dev)
    out = ints(c['cols'], lo=-8, hi=8, seed=77, dtype=F32, dev=dev)
    ref = (out.double() + x[:, :c['cols']].sum(0)).float()
    hip.colsum(x.to(c['dtype']), out, c['rows'], c['cols'], c['ld'])
    assert_exact(out, ref, 'colsum %s' % c)


def check_colsum_fold(hip, cases):
    dev = device(hip)
    probs, refs = [], []
    for c in cases:
        part = ints(c['nblk'], 2 * c['cols'], lo=-c['amax'], hi=c['amax'], seed=78, dtype=F32, dev=dev)
        o0, o1 = ints(c['cols'], lo=-8, hi=8, seed=79, dtype=F32, dev=dev), ints(c['cols'], lo=-8, hi=8, seed=80, dtype=F32, dev=dev)
        refs.append(((o0.double() + part[:, :c['cols']].double().sum(0)).float(), (o1.double() + part[:, c['cols']:].double().sum(0)).float()))
        probs.append((part, o0, o1, c['nblk'], c['cols']))
    hip.colsum_fold_group(probs)
    for q, (r0, r1), c in zip(probs, refs, cases):
        assert_exact(q[1], r0, 'colsum_fold_group out0 %s' % c)
        assert_exact(q[2], r1, 'colsum_fold_group out1 %s' % c)


def check_sumsq(hip, c):
    dev = device(hip)
    x = ints(c['n'], lo=-c['amax'], hi=c['amax'], seed=91, dtype=F32, dev=dev)
    acc = torch.full((1,), 5.0, device=dev)
    hip.sumsq(x, c['n'], acc)
    assert_exact(acc, (5.0 + x.double().pow(2).sum()).float().view(1), 'sumsq %s' % c)


def check_clip_scale(hip, c):
    """gscale = min(1, max_norm / (sqrt(S) + 1e-6)) evaluated in fp32 from the EXACT sum of squares S"""
    dev = device(hip)
    g = ints(c['n'], lo=-c['amax'], hi=c['amax'], seed=92, dtype=F32, dev=dev)
    ws = torch.zeros(1024, device=dev)
    sc = torch.full((1,), float('nan'), device=dev)
    hip.clip_scale(g, c['max_norm'], ws, sc)
    S = float(g.double().pow(2).sum())
    norm = np.float32(math.sqrt(S))
    want = min(np.float32(1.0), np.float32(c['max_norm']) / (norm + np.float32(1e-6)))
    assert_exact(sc.cpu(), torch.tensor([float(want)], dtype=F32), 'clip_scale %s (S = %d)' % (c, S))


def all_bounds():
    """(table, case, exact_bound) of every case of every table above: what tests/test_exact_cases_cpu.py holds against 2^24"""
    for c in GEMM_CASES:
        yield 'gemm', c, gemm_bound(c)
    for c in CONV_CASES:
        yield 'conv', c, conv_bound(c)
    for name, cases in WGROUP_CASES.items():
        for c in cases:
            yield 'wgrad_group ' + name, c, conv_bound(c)
    for name in TT_SHAPES:
        for c in tt_cases(name):
            yield 'tt_group ' + name, c, exact_bound(c)
    for c in CHAIN_CASES:
        yield 'chain y', c, c['by']
        yield 'chain z', c, c['bz']
    for name, table in (('dual', DUAL_CASES), ('stem', STEM_CASES), ('linear_ln', LINEAR_LN_CASES), ('qkv', QKV_CASES), ('colsum', COLSUM_CASES),
                        ('fold', FOLD_CASES), ('sumsq', SUMSQ_CASES), ('clip', CLIP_CASES)):
        for c in table:
            yield name, c, exact_bound(c)
