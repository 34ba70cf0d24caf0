"""Exact-arithmetic GPU tests of every GEMM / convolution kernel family (cases, references and check functions: tests/exact_cases.py).

Integer operands make every product and partial sum exact in fp32, so each result must EQUAL the float64 reference rounded once
(torch.equal; bf16 outputs: round to nearest even) -- whatever the tiling, split, atomics or workspace pass.  Every output buffer is
NaN-filled (or holds the integers it accumulates into) before the launch, padding columns / guard rows carry a sentinel that must
survive, and a kernel family forced with gpv_set_option is asserted through its launch counter to have run.
tests/test_exact_cases_cpu.py holds the precondition (exact_bound < 2^24 for every case here) and proves the checks on the CPU.
Not covered (not exact): the attention core, softmax, LayerNorm statistics, GELU, AdamW -- tests/test_kernels_gpu.py."""
import contextlib

import pytest
import torch

from tests import exact_cases as E

pytestmark = pytest.mark.gpu


def hip():
    import gpv1_amd.hip as h
    h.lib()
    return h


class _Launches:
    n = None


@contextlib.contextmanager
def forced(h, opts, counter=None):
    """set the kernel-selection options {name: value} (hip.OPT_<name>) for the block, restore them afterwards whatever happens, and
    count the launches of <counter>_LAUNCHES inside it (-> .n, read after the block's work has been enqueued)"""
    prev, box = {}, _Launches()
    try:
        for name, v in opts.items():
            prev[name] = h.set_option(getattr(h, 'OPT_' + name), v)
        if counter:
            h.set_option(getattr(h, 'OPT_%s_LAUNCHES' % counter), 0)
        yield box
        if counter:
            torch.cuda.synchronize()
            box.n = h.set_option(getattr(h, 'OPT_%s_LAUNCHES' % counter), 0)
    finally:
        for name, v in reversed(list(prev.items())):
            h.set_option(getattr(h, 'OPT_' + name), v)


def _expect(box, c, what):
    want = c.get('expect')
    if want is None:
        return
    if want == '>=1':
        assert box.n >= 1, (what, 'the forced kernel family did not run', box.n)
    else:
        assert box.n == want, (what, 'launches of the forced kernel family', box.n, want)


def _gid(c):
    flags = ''.join(f for f, on in (('f32', c['out'] == E.F32), ('T', c['la']), ('t', c['lb']), ('b%d' % c['batch'], c['batch'] > 1), ('e' + c['epi'], c['epi']),
                                    ('relu', c['act']), ('drop', c['drop']), ('acc%d' % c['split_k'], c['acc']), ('atomic', not c['ws']), ('rowsum', c['rowsum']),
                                    ('kpad', c['kpitch']), ('wide' + str(c['precise']), c['precise'])) if on)
    return '%s-%dx%dx%d-%s-a%g-s%d' % (c['family'], c['M'], c['N'], c['K'], flags or 'plain', c['alpha'], c['seed'])


def _cid(c):
    return '%s-%dto%d-k%ds%d-%dx%dx%d-m%s-%s%s-s%d' % (c['family'], c['Cin'], c['Cout'], c['k'], c['s'], c['Bn'], c['H'], c['W'], ''.join(map(str, c['modes'])),
                                                      'f32' if c['dtype'] == E.F32 else 'bf16', ('-bits' + c['bits']) if c['bits'] else '', c['seed'] + 10 * c['split_k'] +
                                                      100 * int(c['res']) + 200 * int(c['mask']) + 400 * int(c['fwd_mask']) + 800 * c['act'])


@pytest.mark.parametrize('c', E.GEMM_CASES, ids=_gid)
def test_gemm_exact(c):
    h = hip()
    with forced(h, c['opts'], c['counter']) as box:
        E.check_gemm(h, c)
    _expect(box, c, _gid(c))


@pytest.mark.parametrize('c', E.CONV_CASES, ids=_cid)
def test_conv_exact(c):
    h = hip()
    with forced(h, c['opts'], c['counter']) as box:
        E.check_conv(h, c)
    _expect(box, c, _cid(c))


def test_gemm_reduction_major_a_with_k_major_b_is_refused_before_any_launch():
    """of the four layout pairs gpv_gemm computes three (E.LAYOUTS, all in the tables above); (GPV_TRANS, GPV_KMAJOR) has no kernel:
    hipErrorInvalidValue, and nothing is written"""
    h = hip()
    A, B = E.ints(100, 300, dtype=E.BF, dev='cuda'), E.ints(256, 100, seed=1, dtype=E.BF, dev='cuda')
    Cm = torch.full((300, 256), float('nan'), device='cuda', dtype=E.BF)
    with pytest.raises(RuntimeError, match='hipError 1'):
        h.gemm(A, B, Cm, 300, 256, 100, 300, 100, 256, layoutA=E.TRANS, layoutB=E.KMAJOR)
    torch.cuda.synchronize()
    assert bool(torch.isnan(Cm.float()).all())


_PREPARED = {}


@pytest.mark.parametrize('wg8h', [0, 1])
@pytest.mark.parametrize('wg8', [0, 2])
@pytest.mark.parametrize('name', sorted(E.WGROUP_CASES))
def test_conv_wgrad_group_exact(name, wg8, wg8h):
    """the mixed problem lists of the three grouped weight-gradient tests (incl. problems the grouped kernel refuses), accumulated into
    nonzero integer gradients, on the 128 x 128 kernel and the eight-phase 256 x 256 / half-width kernels"""
    h = hip()
    if name not in _PREPARED:
        _PREPARED[name] = E.wgroup_problems(E.WGROUP_CASES[name], 'cuda')
    with forced(h, dict(WG8=wg8, WG8H=wg8h), 'WG8') as box:
        E.check_wgrad_group(h, _PREPARED[name])
    if (name == 'eight_phase' and wg8 == 2) or (name == 'half_width' and wg8h == 1):
        assert box.n >= 1, (name, wg8, wg8h, box.n)
    if wg8 == 0 and wg8h == 0:
        assert box.n == 0, box.n


@pytest.mark.parametrize('w8l', [0, 1])
@pytest.mark.parametrize('name', sorted(E.TT_SHAPES))
def test_gemm_tt_group_exact(name, w8l):
    """more than 48 problems per call; dW a row slice of a larger buffer whose other rows must stay; bias gradients; sliced reductions
    through the workspace + the grouped reduce pass (W8L = 1) and whole reductions added in place"""
    h = hip()
    with forced(h, dict(W8L=w8l), 'WG8') as box:
        E.check_tt_group(h, E.tt_cases(name))
    if w8l == 0:
        assert box.n == 0, box.n
    elif name == 'eight_phase':
        assert box.n >= 2, box.n


@pytest.mark.parametrize('c', E.DUAL_CASES, ids=lambda c: '%d+%dto%d-s%d-%dx%dx%d%s' % (c['K1'], c['K2'], c['N'], c['s2'], c['Bn'], c['OH'], c['OW'], '-bits' if c['bits'] else ''))
def test_conv1x1_dual_exact(c):
    E.check_dual(hip(), c)


@pytest.mark.parametrize('c', E.CHAIN_CASES, ids=lambda c: '%s-%d-%dx%dx%d%s' % (c['branch'], c['N2'], c['Bn'], c['OH'], c['OW'], '-bits' if c['bits'] else ''))
def test_conv1x1_chain_exact(c):
    """y and z against float64 math (not against the two launches); z is a second product of the ROUNDED y, which are integers"""
    h = hip()
    with forced(h, dict(C1S=2)):
        E.check_chain(h, c)


@pytest.mark.parametrize('c', E.STEM_CASES, ids=lambda c: '%dx%dx%d' % (c['Bn'], c['H'], c['W']))
def test_stem_pool_exact(c):
    E.check_stem(hip(), c)


@pytest.mark.parametrize('c', E.LINEAR_LN_CASES, ids=lambda c: 'rows%d' % c['rows'])
def test_linear_layernorm_projection_exact(c):
    E.check_linear_ln_s(hip(), c)


@pytest.mark.parametrize('c', E.QKV_CASES, ids=lambda c: '%dx%d' % (c['Bn'], c['S']))
def test_attention_in_projection_exact(c):
    E.check_attention_qkv(hip(), c)


@pytest.mark.parametrize('c', E.COLSUM_CASES, ids=lambda c: '%dx%d-ld%d-%s' % (c['rows'], c['cols'], c['ld'], 'f32' if c['dtype'] == E.F32 else 'bf16'))
def test_colsum_exact(c):
    E.check_colsum(hip(), c)


def test_colsum_fold_group_exact():
    E.check_colsum_fold(hip(), E.FOLD_CASES)


@pytest.mark.parametrize('c', E.SUMSQ_CASES, ids=lambda c: 'n%d' % c['n'])
def test_sumsq_exact(c):
    E.check_sumsq(hip(), c)


@pytest.mark.parametrize('c', E.CLIP_CASES, ids=lambda c: 'n%d-%g' % (c['n'], c['max_norm']))
def test_clip_scale_norm_exact(c):
    E.check_clip_scale(hip(), c)
