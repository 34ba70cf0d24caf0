"""The exact-arithmetic cases of tests/exact_cases.py, without a GPU: (1) the analytic precondition exact_bound < 2^24 for every case of
every table tests/test_exact_gpu.py parametrises over; (2) the check functions through tests/cpu_shim.py on the small cases -- equality
there proves the references, layouts and epilogue order of the checks independently of any kernel; (3) mutation checks: the shim's gemm /
conv2d damaged in the three ways the tolerance criterion of tests/test_kernels_gpu.py cannot see (bf16 store rounded toward zero, an fp32
result that went through bf16 once, one product dropped for one output) -- the exact check must fail each, and for the first two the
tolerance criterion is shown to pass on the same data."""
import types

import pytest
import torch

from tests import cpu_shim as S
from tests import exact_cases as E

TOL_BF16, TOL_DW = 1.2e-2, 3e-3           # tests/test_kernels_gpu.py: TOL[bf16], and what it allows on the fp32 dw of bf16 operands


def test_precondition_holds_for_every_case_of_every_table():
    n = 0
    for table, c, bound in E.all_bounds():
        assert bound < E.LIMIT, (table, bound, c)
        n += 1
    assert n > 900
    for c in E.CLIP_CASES:                  # the 1024 fp32 partial sums are added in double
        assert c['n'] * c['amax'] ** 2 < 2 ** 53


def test_case_tables_are_well_formed():
    for c in E.GEMM_CASES:
        assert c['alpha'] in E.ALPHAS and set(c['epi']) <= set('sbrm') and c['split_k'] in (1, 3, 4, 8)
        assert not (c['split_k'] > 1 and (not c['acc'] or c['epi'] or c['act'] or c['drop']))          # include/gpv_hip.h: linear epilogue
        assert c['amax'] <= 256 or c['precise']                                                       # bf16 holds integers up to 256 exactly
    assert torch.equal(E.pow2(4096).abs().unique(), torch.tensor([0.25, 0.5, 1.0, 2.0, 4.0])) and bool((E.pow2(4096) < 0).any())
    m = E.sign_pattern(64, 64)
    assert bool((m == 0).any()) and bool((m < 0).any()) and bool((m > 0).any())
    families = {c['family'] for c in E.GEMM_CASES} | {c['family'] for c in E.CONV_CASES}
    for f in ('reg', 'glds2', 'glds3', 'skinny', 'skinny_bt', 'gemv', 'c1s_linear', 'acc', 'precise', 'precise_gemv', 'halo1', 'halo2', 'c3s', 'c1s', 'c1s_s2',
              'c1s_bits', 'batch1', 'two_per_cu', 'wgrad_glds0', 'wgrad_glds2') + tuple('pipe%dx%d' % q for q in E.PIPE_CFGS):
        assert f in families, f
    assert all(len(E.tt_cases(n)) > 48 for n in E.TT_SHAPES)


def test_integer_results_exercise_the_bf16_rounding():
    """a third of the results of a K = 9600 product of [-3, 3] integers are not bf16 numbers, a fifth are exact ties: every launch of such a
    case tests the rounding mode of the store; and fp32 equals float64 on it whatever the summation order"""
    a, b = E.ints(64, 9600), E.ints(96, 9600, seed=1)
    y64 = a @ b.t()
    assert torch.equal((a.float() @ b.float().t()).double(), y64)
    perm = torch.randperm(9600, generator=torch.Generator().manual_seed(0))
    assert torch.equal((a[:, perm].float() @ b[:, perm].float().t()).double(), y64)
    assert float((a.abs() @ b.abs().t()).max()) < E.LIMIT
    lossy = y64.float().bfloat16().double() != y64
    assert lossy.double().mean() > 0.2
    up = (y64.float().view(torch.int32) & 0xFFFF) == 0x8000                 # exactly half way between two bf16 numbers
    assert up.double().mean() > 0.1
    # 12-bit integers split into hi + lo bf16 halves exactly, lo != 0 for most of them
    v = E.ints(4096, lo=-2047, hi=2047).float()
    hi = v.bfloat16().float()
    lo = (v - hi).bfloat16().float()
    assert torch.equal(hi + lo, v) and (lo != 0).double().mean() > 0.5


# ------------------------------------------------------------------------------------------- the check functions through the shim
def _small_gemm(c):
    return not c['drop'] and c['M'] * c['N'] * c['K'] * c['batch'] <= 3e8           # (the shim has no dropout)


def _small_conv(c):
    OH, OW = E.conv_geometry(c)
    return not c['bits'] and c['Bn'] * OH * OW * c['Cin'] * c['Cout'] * c['k'] ** 2 <= 1.5e9


def _gid(c):
    return '-'.join(str(c[k]) for k in ('family', 'M', 'N', 'K')) + ('-%s' % c['seed'])


def _cid(c):
    return '-'.join(str(c[k]) for k in ('family', 'Cin', 'Cout', 'k', 's', 'H', 'W', 'Bn', 'seed'))


SMALL_GEMM = [c for c in E.GEMM_CASES if _small_gemm(c)]
SMALL_CONV = [c for c in E.CONV_CASES if _small_conv(c)]


def test_most_cases_are_small_enough_for_the_shim():
    assert len(SMALL_GEMM) > 300 and len(SMALL_CONV) > 150


@pytest.mark.parametrize('chunk', range(8))
def test_gemm_checks_pass_on_the_shim(chunk):
    for c in SMALL_GEMM[chunk::8]:
        E.check_gemm(S, c)


@pytest.mark.parametrize('chunk', range(8))
def test_conv_checks_pass_on_the_shim(chunk):
    for c in SMALL_CONV[chunk::8]:
        E.check_conv(S, c)


@pytest.mark.parametrize('name', sorted(E.WGROUP_CASES))
def test_wgrad_group_check_passes_on_the_shim(name):
    cases = [c for c in E.WGROUP_CASES[name] if c['Bn'] * c['H'] * c['W'] <= 20000]
    assert len(cases) >= 5
    E.check_wgrad_group(S, E.wgroup_problems(cases, 'cpu'))


def test_fused_launch_and_reduction_checks_pass_on_the_shim():
    for c in E.STEM_CASES:
        if c['H'] <= 100:
            E.check_stem(S, c)
    for c in E.LINEAR_LN_CASES:
        E.check_linear_ln_s(S, c)
    for c in E.QKV_CASES:
        if c['Bn'] * c['S'] <= 1000:
            E.check_attention_qkv(S, c)
    for c in E.COLSUM_CASES:
        E.check_colsum(S, c)
    for c in E.SUMSQ_CASES:
        E.check_sumsq(S, c)
    for c in E.CLIP_CASES:
        E.check_clip_scale(S, c)


# ------------------------------------------------------------------------------------------- mutation checks
def _trunc_bf16(f):
    """fp32 -> bf16 rounded toward zero"""
    return (f.view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _rel(a, ref):
    """the criterion of tests/test_kernels_gpu.py"""
    a, ref = a.float(), ref.float()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-12)).item()


def _mutant(kind):
    """tests.cpu_shim with gemm and conv2d damaged; .rel = the tolerance criterion of the last damaged result against the undamaged fp32 one"""
    m = types.SimpleNamespace(**{n: getattr(S, n) for n in dir(S) if not n.startswith('__')})
    m.rel, m.hits = None, 0

    def gemm(A, B, Cm, M, N, K, lda, ldb, ldc, **kw):
        bt, sC = kw.get('batch', 1), kw.get('sC', 0)
        view = lambda t: S._sv(t, (bt, M, N), (sC, ldc, 1))
        if kind == 'trunc' and Cm.dtype == torch.bfloat16:
            Cf = Cm.float()
            S.gemm(A, B, Cf, M, N, K, lda, ldb, ldc, **kw)
            Cm.copy_(_trunc_bf16(Cf))
            m.rel, m.hits = _rel(view(Cm), view(Cf)), m.hits + 1
        elif kind == 'via_bf16' and Cm.dtype == torch.float32 and kw.get('accumulate'):
            Cz = torch.zeros_like(Cm)
            S.gemm(A, B, Cz, M, N, K, lda, ldb, ldc, **dict(kw, a_rowsum=None))
            if kw.get('a_rowsum') is not None:
                kw['a_rowsum'][:M] += S._mat(A, M, K, lda, kw.get('layoutA', 0)).float()[0].sum(1)
            exact = view(Cm) + view(Cz)
            Cm += Cz.bfloat16().float()
            m.rel, m.hits = _rel(view(Cm), exact), m.hits + 1
        elif kind == 'drop_product':
            Cf = Cm.float()
            S.gemm(A, B, Cf, M, N, K, lda, ldb, ldc, **kw)
            assert not kw.get('bias') and kw.get('alpha', 1.0) == 1.0 and not kw.get('act') and kw.get('rowscale') is None
            a = S._mat(A, M, K, lda, kw.get('layoutA', 0)).float()[0, M // 2]
            b = S._mat(B, N, K, ldb, kw.get('layoutB', 0)).float()[0, N // 2]
            k0 = int((a * b != 0).nonzero()[0])
            view(Cf)[0, M // 2, N // 2] -= a[k0] * b[k0]
            Cm.copy_(Cf.to(Cm.dtype))
            m.hits += 1
        else:
            S.gemm(A, B, Cm, M, N, K, lda, ldb, ldc, **kw)

    def conv2d(mode, x, w, y, B, IH, IW, Cs, Cin, OH, OW, Cout, KH, KW, SH, SW, PH, PW, **kw):
        args = (B, IH, IW, Cs, Cin, OH, OW, Cout, KH, KW, SH, SW, PH, PW)
        if kind == 'trunc' and mode in (0, 1) and y.dtype == torch.bfloat16:
            yf = y.float()
            S.conv2d(mode, x, w, yf, *args, **kw)
            y.copy_(_trunc_bf16(yf))
            m.rel, m.hits = _rel(y, yf), m.hits + 1
        elif kind == 'via_bf16' and mode == 2:
            z = torch.zeros_like(y)
            S.conv2d(2, x, w, z, *args, **kw)
            exact = y + z
            y += z.bfloat16().float()
            m.rel, m.hits = _rel(y, exact), m.hits + 1
        elif kind == 'drop_product' and mode == 2:
            S.conv2d(2, x, w, y, *args, **kw)
            co, ci, r, s_ = Cout // 2, Cin // 2, KH // 2, KW // 2
            assert PH == KH // 2 and PW == KW // 2                       # the centre tap reads pixel (oh * SH, ow * SW): always inside
            prod = w.float()[:, :, :, co] * x.float()[:, ::SH, ::SW, ci][:, :OH, :OW]
            b0, oh, ow = (prod != 0).nonzero()[0].tolist()
            y[co, r, s_, ci] -= kw['rowscale'][co] * prod[b0, oh, ow]
            m.hits += 1
        else:
            S.conv2d(mode, x, w, y, *args, **kw)
    m.gemm, m.conv2d = gemm, conv2d
    return m


MUT_GEMM = {
    'trunc': [E.gemm_case('mutation', 300, 256, 2048), E.gemm_case('mutation', 300, 256, 2048, epi=True, alpha=0.5, act=E.ACT_RELU, pad=8, seed=1),
              E.gemm_case('mutation', 200, 192, 1024, batch=2, lb=E.TRANS, seed=2)],
    'via_bf16': [E.gemm_case('mutation', 128, 136, 9600, la=E.TRANS, lb=E.TRANS, acc=True, split_k=8, rowsum=True),
                 E.gemm_case('mutation', 72, 136, 2000, la=E.TRANS, lb=E.TRANS, acc=True, split_k=3, ws=False, pad=8, seed=1)],
    'drop_product': [E.gemm_case('mutation', 130, 70, 96), E.gemm_case('mutation', 130, 70, 96, out=E.F32, pad=8, seed=1),
                     E.gemm_case('mutation', 256, 256, 2048, la=E.TRANS, lb=E.TRANS, acc=True, split_k=8, seed=2)]}
MUT_CONV = {
    'trunc': [E.conv_case('mutation', 128, 128, 3, 1, 1, 15, 20, modes=(0,)), E.conv_case('mutation', 256, 128, 3, 2, 1, 24, 32, modes=(1,))],
    'via_bf16': [E.conv_case('mutation', 128, 128, 3, 1, 1, 15, 20, modes=(2,)), E.conv_case('mutation', 256, 512, 1, 2, 0, 30, 40, modes=(2,))],
    'drop_product': [E.conv_case('mutation', 128, 128, 3, 1, 1, 15, 20, modes=(2,)), E.conv_case('mutation', 64, 64, 1, 1, 0, 24, 32, modes=(2,))]}


@pytest.mark.parametrize('kind', ['trunc', 'via_bf16', 'drop_product'])
def test_exact_checks_catch_what_the_tolerance_criterion_cannot(kind):
    for table, check in ((MUT_GEMM, E.check_gemm), (MUT_CONV, E.check_conv)):
        for c in table[kind]:
            check(S, c)                                   # control: the undamaged shim passes
            m = _mutant(kind)
            with pytest.raises(AssertionError, match='elements differ'):
                check(m, c)
            assert m.hits == 1, (kind, c)
            if kind == 'trunc':                           # the blind spot, recorded: one bf16 ulp of an element is below 1.2e-2 of the largest
                assert 0 < m.rel < TOL_BF16, (m.rel, c)
            elif kind == 'via_bf16':                      # 2^-9 of an element is below the 3e-3 allowed on dw
                assert 0 < m.rel < TOL_DW, (m.rel, c)


def test_a_dropped_product_in_one_output_passes_the_tolerance_criterion():
    """K = 2048: the criterion allows 1.2e-2 of max|ref| (about 3 in absolute terms), one product is at most 9 / typically 2"""
    c = E.gemm_case('mutation', 300, 256, 2048, out=E.F32)
    a, b = E.ints(300, 2048, seed=1).float(), E.ints(256, 2048, seed=2).float()
    ref = a @ b.t()
    bad = ref.clone()
    k0 = int((a[150] * b[128] != 0).nonzero()[0])
    bad[150, 128] -= a[150, k0] * b[128, k0]
    assert not torch.equal(bad, ref) and _rel(bad.bfloat16(), ref) < TOL_BF16
    with pytest.raises(AssertionError, match='1 of'):
        E.check_gemm(_mutant('drop_product'), c)


def test_conv64_is_conv2d_in_float64():
    """the convolution reference of the exact checks is F.conv2d on float64 tensors, spelled as unfold + matmul: same bits"""
    import torch.nn.functional as F
    x, w = E.ints(2, 8, 9, 11), E.ints(5, 8, 3, 3, seed=1)
    for s, p in ((1, 1), (2, 1), (2, 0), (1, 0)):
        assert torch.equal(E.conv64(x, w, s, p), F.conv2d(x, w, stride=s, padding=p))
    w7 = E.ints(4, 3, 7, 7, seed=2)
    assert torch.equal(E.conv64(E.ints(1, 3, 34, 30), w7, 2, 3), F.conv2d(E.ints(1, 3, 34, 30), w7, stride=2, padding=3))
