"""libgpv_beam.so on the GPU: gpv_beam_step against the host rule (bit-equal, the device's lse handed to the rule), its lse against a
float64 logsumexp, gpv_beam_reorder against index_select, and GPV.forward_beam_search(impl='device') on the small fixture against the
reference's golden search and against the torch path."""
import json
import os

import numpy as np
import pytest
import torch

from tests.beam_cases import make_case, same, PLANTS
from tests.test_model_cpu import build_small, nested, GOLD, V, B, H, W, Tl, PAD
from tests import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _device_step(case, mode, T, pitch_tv, state=None):
    """one gpv_beam_step on the case; logits either dense (pitch V) or column t of a [K*B, T, V] buffer whose other columns hold +1e4
    (a wrong pitch would pick them up).  -> (result dict of numpy arrays, lse numpy)"""
    from gpv1_amd import hip_beam
    lg = case['logits']
    R, Vc = lg.shape
    t = case['t']
    if pitch_tv:
        buf = torch.full((R, T, Vc), 1e4, dtype=lg.dtype, device=DEV)
        buf[:, t] = lg.to(DEV)
        view = buf[:, t]
    else:
        view = lg.to(DEV).contiguous()
    st = state or {k: torch.from_numpy(case[k]).to(DEV) for k in ('seq_lp', 'seqs', 'finished', 'length')}
    K, Bc = st['seqs'].shape[:2]
    lse = torch.zeros(R, device=DEV)
    tok = torch.full((R,), -1, dtype=torch.long, device=DEV)
    parent = torch.full((Bc, K), -1, dtype=torch.int32, device=DEV)
    dv = lambda a: None if a is None else torch.from_numpy(a).to(DEV)
    hip_beam.step(view, lse, st['seq_lp'], st['seqs'], tok, parent, st['finished'], st['length'], t, mode, case['pad_id'], case['stop_id'],
                  inv_pen=dv(case['inv_pen']), vocab_mask=dv(case['vocab_mask']))
    torch.cuda.synchronize()
    out = {'parent': parent, 'tok': tok, 'seqs': st['seqs'], 'seq_lp': st['seq_lp'], 'finished': st['finished'], 'length': st['length']}
    return {k: v.cpu().numpy() for k, v in out.items()}, lse.cpu().numpy(), st


def _host_step(case, lse, mode):
    from gpv1_amd import beam as rule
    return rule.beam_step_host(case['x'], lse, case['seq_lp'], case['seqs'], case['finished'], case['length'], case['t'], mode,
                               case['pad_id'], case['stop_id'], inv_pen=case['inv_pen'], vocab_mask=case['vocab_mask'])


SHAPES = [(1, 1, 37, 4, torch.float32, False), (3, 5, 1003, 6, torch.bfloat16, True), (2, 8, 300, 5, torch.bfloat16, False),
          (4, 3, 40, 6, torch.float32, True),
          (1, 2, 2049, 4, torch.bfloat16, True)]            # beyond the issue's table: one element into the second batch of eight loads per lane


@pytest.mark.parametrize('Bc,K,Vc,T,dtype,pitch_tv', SHAPES)
def test_one_step_equals_the_host_rule_bit_for_bit(Bc, K, Vc, T, dtype, pitch_tv):
    """every output of one step -- parent, tok, seqs, seq_lp, finished, length -- equals beam_step_host fed with the device's own lse;
    t = 0, 1, T-2; both modes; plain, every planted situation, a mask leaving K + 2 finite entries, a penalty table"""
    from gpv1_amd import beam as rule
    variants = [dict(), dict(plants=PLANTS), dict(masked=True), dict(penalty=0.6, plants=('mixed_fin', 'stop_top')),
                dict(plants=PLANTS, masked=True, penalty=2.0)]
    n = 0
    for t in sorted({0, 1, T - 2}):
        for vi, var in enumerate(variants):
            case = make_case(100 * t + vi + 17 * K, Bc, K, Vc, T, t, dtype, **var)
            for mode in (rule.EXTEND, rule.FREEZE):
                got, lse, _ = _device_step(case, mode, T, pitch_tv)
                want = _host_step(case, lse, mode)
                ok, what = same(got, want)
                assert ok, (what, t, var, mode, got[what], want[what])
                n += 1
    assert n == len({0, 1, T - 2}) * 10


@pytest.mark.parametrize('mode_name', ['extend', 'freeze'])
def test_five_chained_steps_equal_the_host_rule_after_every_step(mode_name):
    """(B, K, V) = (3, 5, 1003), T = 7: the device state is carried in place from step to step, the host rule from its own outputs"""
    from gpv1_amd import beam as rule
    mode = rule.MODES[mode_name]
    Bc, K, Vc, T = 3, 5, 1003, 7
    pad_id, stop_id = Vc - 4, Vc - 2
    host = {'seq_lp': np.zeros((Bc, K), np.float32), 'seqs': np.zeros((K, Bc, T), np.int64), 'finished': np.zeros((Bc, K), np.int32),
            'length': np.zeros((Bc, K), np.int32)}
    state = None
    inv_pen = rule.length_table(T, 0.6)
    for t in range(5):
        case = make_case(900 + t, Bc, K, Vc, T, t, torch.bfloat16, plants=('stop_top', 'dupmax'))
        case['logits'][:, stop_id] += 1.5                     # __stop__ often near the top: hypotheses do finish along the way
        case['x'] = case['logits'].float().numpy().copy()
        case.update(host, inv_pen=inv_pen)
        got, lse, state = _device_step(case, mode, T, True, state)
        want = _host_step(case, lse, mode)
        ok, what = same(got, want)
        assert ok, (what, t, got[what], want[what])
        host = {k: want[k] for k in host}
    if mode == rule.FREEZE:
        assert host['finished'].any()


@pytest.mark.parametrize('Vc', [37, 300, 1003, 2048, 10000, 16384])
def test_lse_against_float64_logsumexp(Vc):
    """|lse - float64 logsumexp| <= (n_chain + 4) * 2^-24 + 2 ulp_fp32(|lse|), n_chain(V) = ceil(V / 256) + 9 (include/gpv_beam.h): the
    sum's chain of additions, the exponentials and the logarithm (one ulp each and the rounding of x - m), the final add.  The CPU
    emulation of the 256-lane strided sum plus tree stays at 0.29 of this bound for V up to 16384 and logit scales 1 - 12: a failure
    is a defect, not noise."""
    from gpv1_amd import beam as rule
    worst = 0.0
    for si, scale in enumerate((1.0, 4.0, 12.0)):
        for dtype in (torch.float32, torch.bfloat16):
            case = make_case(50 + si, 2, 2, Vc, 4, 1, dtype, masked=(si == 1 and Vc > 4))
            case['logits'] = (case['logits'].float() * (scale / 3.0)).to(dtype)
            case['x'] = case['logits'].float().numpy().copy()
            _, lse, _ = _device_step(case, rule.EXTEND, 4, False)
            x = case['x'].astype(np.float64) + (0.0 if case['vocab_mask'] is None else case['vocab_mask'].astype(np.float64)[None, :])
            m = x.max(1)
            ref = m + np.log(np.exp(x - m[:, None]).sum(1))
            bound = (rule.n_chain(Vc) + 4) * 2.0 ** -24 + 2 * np.spacing(np.abs(lse).astype(np.float32)).astype(np.float64)
            err = np.abs(lse.astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            print('LSE V=%d scale=%g %s: max err %.3e, bound %.3e' % (Vc, scale, dtype, err.max(), bound.min()))
            assert (err <= bound).all(), (Vc, scale, dtype, err.max(), bound.min())
    print('LSE V=%d worst err / bound = %.3f' % (Vc, worst))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32])
@pytest.mark.parametrize('K,Bc', [(5, 3), (3, 5)])
def test_reorder_equals_index_select_and_touches_nothing_else(dtype, K, Bc):
    """D = 64, T = 6, L = 3, K*B = 15: every element carries a code of (layer, row, position, column) as its bit pattern; random,
    identity and all-zero parents, upto in {1, T-1}: the k | v columns of positions < upto equal index_select bit for bit, positions
    >= upto and the q columns keep their bits"""
    from gpv1_amd import hip_beam
    D, T, L = 64, 6, 3
    R = K * Bc
    idt = torch.int16 if dtype == torch.bfloat16 else torch.int32
    code = torch.arange(L * R * T * 3 * D, dtype=torch.int64).reshape(L, R, T, 3 * D)
    g = torch.Generator().manual_seed(5)
    parents = [torch.randint(0, K, (Bc, K), generator=g), torch.arange(K).repeat(Bc, 1), torch.zeros(Bc, K, dtype=torch.long),
               torch.randint(0, K, (Bc, K), generator=g)]
    for parent in parents:
        for upto in (1, T - 1):
            bits = [(code[l] - (32768 if idt == torch.int16 else 0)).to(idt).to(DEV) for l in range(L)]
            caches = [b.view(dtype) for b in bits]
            hip_beam.reorder(caches, parent.to(torch.int32).to(DEV), upto)
            torch.cuda.synchronize()
            perm = (parent.t() * Bc + torch.arange(Bc)[None, :]).reshape(R)
            for l in range(L):
                before = (code[l] - (32768 if idt == torch.int16 else 0)).to(idt)
                want = before.clone()
                want[:, :upto, D:] = before[:, :upto, D:].index_select(0, perm)
                assert torch.equal(caches[l].view(idt).cpu(), want), (l, upto, parent.tolist())


def test_bad_extents_are_refused_before_a_launch():
    from gpv1_amd import hip_beam
    case = make_case(1, 2, 3, 40, 6, 1)
    st = {k: torch.from_numpy(case[k]).to(DEV) for k in ('seq_lp', 'seqs', 'finished', 'length')}
    lg = case['logits'].to(DEV)
    z = lambda *s, d=torch.int32: torch.zeros(*s, dtype=d, device=DEV)
    args = lambda t=1, lg=lg: (lg, z(6, d=torch.float32), st['seq_lp'], st['seqs'], z(6, d=torch.long), z(2, 3), st['finished'], st['length'], t, 0, 36, 38)
    with pytest.raises(ValueError, match='step 5 outside'):
        hip_beam.step(*args(t=5))
    with pytest.raises(ValueError, match='beam size 3 exceeds'):
        hip_beam.step(*args(lg=lg[:, :2].contiguous()))
    with pytest.raises(ValueError, match='unit column stride'):
        hip_beam.step(*args(lg=lg.t().contiguous().t()))
    with pytest.raises(RuntimeError, match='GPU'):
        hip_beam.step(*args(lg=lg.cpu()))
    with pytest.raises(ValueError, match='upto'):
        hip_beam.reorder([torch.zeros(6, 6, 192, device=DEV)], z(2, 3), 7)
    # the C entry points themselves: hipErrorInvalidValue (1), nothing launched
    import ctypes as C
    a = hip_beam.BeamArgs(B=2, K=9, V=40, T=6, t=1)
    assert hip_beam.lib().gpv_beam_step(C.byref(a), None) == 1
    r = hip_beam.ReorderArgs(L=9, B=2, K=3, T=6, D=64, upto=1)
    assert hip_beam.lib().gpv_beam_reorder(C.byref(r), None) == 1


# ---- model level: small fixture, precise mode, K = 3 -----------------------------------------------------------------------
@pytest.fixture(scope='module')
def small_model():
    import gpv1_amd.ops as ops
    import gpv1_amd.hip as hip
    hip.lib()
    ops.RT.set_precise(True)
    model, _ = build_small()
    model.to(DEV).eval()
    images, mask, ids, attn = synth.synth_batch(B, H, W, Tl, V, pad_to=PAD)
    yield model, (nested(images.to(DEV), mask.to(DEV)), (ids.to(DEV), attn.to(DEV)))
    # this model owns several whole-search hipGraphs, each with a stream of its own: retire them the way the model itself does on an
    # eviction (graphs first, then -- the device idle -- their streams) instead of leaving them to the cycle collector, which would
    # destroy them in the middle of the next module's first capture set-up and leave their streams behind
    torch.cuda.synchronize()
    for key in list(model._igraphs):
        model._drop_igraph(key)
    model._kvdec.clear()
    del model
    import gc
    gc.collect()
    torch.cuda.synchronize()
    ops.RT.set_precise(False)


def _raw(model, batch, **kw):
    """seqs [K,B,T], seq_lp [B,K], lengths, finished of one eager search"""
    with torch.no_grad():
        o = model._beam_device(batch[0], batch[1], 3, **kw)
    torch.cuda.synchronize()
    return o['_beam_seqs'].cpu(), o['_beam_lp'].cpu(), o.get('beam_lengths'), o.get('beam_finished')


def test_model_device_path_reproduces_the_golden_and_the_torch_path(small_model):
    """answers = small_beam.json, probabilities within the 1e-3 of test_model_gpu.py; seqs identical to the torch path's on the same
    model.  seq_lp cannot be bit-identical to torch's: torch forms lp = (x - m) - log s, the rule x - (m + log s), and the two sums of
    exponentials have other orders.  Per step the two lp differ by at most 2 * (n_chain + 4) * 2^-24 (both lse errors, the bound of the
    lse test) + 4 roundings of half an ulp of numbers no larger than M = max(|x|, |seq_lp|); T - 1 steps add up."""
    from gpv1_amd import beam as rule
    model, batch = small_model
    ref = json.load(open(os.path.join(GOLD, 'small_beam.json')))
    model.cfg['graph_inference'] = False
    with torch.no_grad():
        od = model.forward_beam_search(batch[0], batch[1], beam_size=3, impl='device')
    assert od['answers'] == ref['answers']
    got, want = torch.tensor(od['answer_probs']), torch.tensor(ref['answer_probs'])
    assert ((got - want).abs().max() / want.abs().max()).item() < 1e-3
    sd, ld, _, _ = _raw(model, batch, impl='device')
    st, lt, _, _ = _raw(model, batch, impl='torch')
    assert torch.equal(sd, st)
    T = sd.shape[2]
    M = max(float(lt.abs().max()), 30.0)                      # (|logit| of this fixture stays far below 30)
    bound = (T - 1) * (2 * (rule.n_chain(V) + 4) * 2.0 ** -24 + 4 * 2.0 ** -24 * M)
    print('BEAM seq_lp device vs torch: max diff %.3e, bound %.3e' % (float((ld - lt).abs().max()), bound))
    assert float((ld - lt).abs().max()) <= bound


def test_model_graphed_equals_eager_and_freeze_equals_extend_when_nothing_finishes(small_model):
    model, batch = small_model
    res = {}
    with torch.no_grad():
        for graphed in (False, True, True):                   # eager, capture + first replay, replay
            model.cfg['graph_inference'] = graphed
            for fin in ('extend', 'freeze'):
                o = model.forward_beam_search(batch[0], batch[1], beam_size=3, impl='device', finished=fin)
                res.setdefault((graphed, fin), []).append((o['answers'], o['answer_probs'], o['beam_lengths'].cpu(), o['beam_finished'].cpu()))
    model.cfg['graph_inference'] = False
    a0, p0, l0, f0 = res[(False, 'extend')][0]
    assert not f0.any() and (l0 == model.cfg.max_text_len - 1).all()
    for key, runs in res.items():
        for a, p, l, f in runs:
            assert a == a0 and p == p0 and torch.equal(l, l0) and torch.equal(f, f0), key      # probabilities compared as Python floats: bit-identical


@pytest.mark.parametrize('alpha', [0.0, 0.6])
def test_model_vocabulary_mask_freeze_and_key_order(small_model, alpha):
    """a mask that leaves {w1, w2, __stop__}: __stop__ appears, a row holds only __pad__ behind it, the K hypotheses of a sample are
    pairwise different and come out in non-increasing key order (key = seq_lp * inv_pen[length], one fp32 multiply)"""
    from gpv1_amd import beam as rule
    model, batch = small_model
    w = model.word_to_idx
    vm = torch.full((V,), -10000.0, device=DEV)
    for name in ('w1', 'w2', '__stop__'):
        vm[w[name]] = 0.0
    seqs, lp, length, fin = _raw(model, batch, impl='device', finished='freeze', alpha=alpha, vocab_mask=vm)
    K, Bc, T = seqs.shape
    body = seqs[:, :, :T - 1]
    assert set(body.unique().tolist()) <= {w['w1'], w['w2'], w['__stop__'], w['__pad__']}
    assert (body == w['__stop__']).any()
    for b in range(Bc):
        rows = [tuple(body[k, b].tolist()) for k in range(K)]
        assert len(set(rows)) == K, rows
        for k, row in enumerate(rows):
            if w['__stop__'] in row:
                i = row.index(w['__stop__'])
                assert all(x == w['__pad__'] for x in row[i + 1:]), row
                assert int(fin[b, k]) == 1 and int(length[b, k]) == i + 1
            else:
                assert int(fin[b, k]) == 0 and int(length[b, k]) == T - 1 and w['__pad__'] not in row
    keys = lp.numpy()
    if alpha:
        keys = (keys * rule.length_table(T, alpha)[length.cpu().numpy()]).astype(np.float32)
    assert (keys[:, :-1] >= keys[:, 1:]).all(), keys
    # the public call reports the same search
    with torch.no_grad():
        o = model.forward_beam_search(batch[0], batch[1], beam_size=3, impl='device', finished='freeze', length_penalty=alpha, vocab_mask=vm)
    assert all(set(a) <= {'w1', 'w2', 'w0'} for per in o['answers'] for a in per)       # ('w0': the never-written slot T - 1, see the CPU test)
