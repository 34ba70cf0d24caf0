"""The constraints of gpv_beam_step on the GPU (no repeated n-gram, minimum length, repetition penalty): one step and chains of steps
against the host rule bit for bit (the device's lse handed to the rule), lse against a float64 logsumexp of the penalised rows, the
constrained instantiation with nothing to ban against the plain one, the refusals of the C entry point and of the binding, and
GPV.forward_beam_search / metrics.cap_metrics with the options on the small fixture."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from tests.beam_cases import same
from tests.beam_constraint_cases import make_constrained_case, PLANTS
from tests.test_model_cpu import build_small, nested, V, B, H, W, Tl, PAD
from tests import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _device_step(case, mode, T, pitch_tv, state=None, constr=None):
    """one gpv_beam_step on the case with the case's constraints (or `constr`); logits dense (pitch V) or column t of a [K*B, T, V]
    buffer whose other columns hold +1e4.  -> (result dict of numpy arrays, lse numpy, the device state)"""
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
                  inv_pen=dv(case['inv_pen']), vocab_mask=dv(case['vocab_mask']), **(case['constr'] if constr is None else constr))
    torch.cuda.synchronize()
    out = {'parent': parent, 'tok': tok, 'seqs': st['seqs'], 'seq_lp': st['seq_lp'], 'finished': st['finished'], 'length': st['length']}
    return {k: v.cpu().numpy() for k, v in out.items()}, lse.cpu().numpy(), st


def _host_step(case, lse, mode, constr=None):
    from gpv1_amd import beam as rule
    return rule.beam_step_host(case['x'], lse, case['seq_lp'], case['seqs'], case['finished'], case['length'], case['t'], mode,
                               case['pad_id'], case['stop_id'], inv_pen=case['inv_pen'], vocab_mask=case['vocab_mask'],
                               **(case['constr'] if constr is None else constr))


# (B, K, V, T, dtype, pitch T*V, the steps): the last one's t = 62 is the longest history; V = 2100 takes two batches of the unrolled loop
SHAPES = [(1, 1, 37, 4, torch.float32, False, (0, 1, 2)), (3, 5, 1003, 6, torch.bfloat16, True, (0, 2, 4)),
          (2, 8, 300, 5, torch.bfloat16, False, (0, 1, 3)), (2, 3, 2100, 64, torch.float32, False, (0, 62))]


@pytest.mark.parametrize('Bc,K,Vc,T,dtype,pitch_tv,steps', SHAPES)
def test_one_constrained_step_equals_the_host_rule_bit_for_bit(Bc, K, Vc, T, dtype, pitch_tv, steps):
    """every output equals beam_step_host fed with the device's own lse.  n in {1, 2, 3} x min_len in {0, 3, T} x penalty off / 1.3 / 0.8
    at every step of the shape; both modes, mask on and off, every plant (all together, and one at a time), finished parents and a
    length-penalty table cycle through the settings"""
    from gpv1_amd import beam as rule
    seen = set()
    for idx, (t, n, ml, theta) in enumerate(itertools.product(steps, (1, 2, 3), (0, 3, T), (None, 1.3, 0.8))):
        mode = (rule.EXTEND, rule.FREEZE)[idx % 2]
        masked = (idx // 2) % 2 == 1
        plants = PLANTS if idx % 3 else (PLANTS[(idx // 3) % len(PLANTS)],)
        base = ('mixed_fin',) if idx % 4 >= 2 else ()
        ml = min(ml, T)
        case = make_constrained_case(1000 * K + idx, Bc, K, Vc, T, t, dtype, plants=plants, masked=masked, n=n, min_len=ml, theta=theta,
                                     mode=mode, base_plants=base, penalty=0.6 if idx % 5 == 0 else None)
        got, lse, _ = _device_step(case, mode, T, pitch_tv)
        want = _host_step(case, lse, mode)
        ok, what = same(got, want)
        assert ok, (what, t, n, ml, theta, mode, masked, plants, got[what], want[what])
        assert np.isfinite(lse).all()
        seen.add((mode, masked))
    assert len(seen) == 4 and idx + 1 == len(steps) * 27


def test_lse_with_a_banned_maximum_and_the_penalty_stays_inside_the_bound():
    """|lse - float64 logsumexp| <= (n_chain + 4) * 2^-24 + 2 ulp_fp32(|lse|), the bound of test_beam_gpu.py: the reference is taken
    from the fp32 values after step 1b, banned tokens included.  The banned maximum is 100 above the rest: with m from the first pop
    the sum would overflow."""
    from gpv1_amd import beam as rule
    worst = 0.0
    for Vc, dtype, theta, masked in ((300, torch.float32, 1.3, False), (1003, torch.bfloat16, 0.8, True), (2100, torch.float32, None, False),
                                     (10000, torch.bfloat16, 1.3, False)):
        for seed in range(3):
            case = make_constrained_case(70 + seed, 2, 3, Vc, 8, 6, dtype, plants=('ban_max', 'seen_both_signs'), masked=masked, n=2, min_len=8,
                                         theta=theta)
            _, lse, _ = _device_step(case, rule.EXTEND, 8, False)
            x = case['x'] if case['vocab_mask'] is None else case['x'] + case['vocab_mask'][None, :]
            x = rule.penalised_rows(x, case['seqs'], case['finished'], 6, rule.EXTEND, case['constr']['repetition']).astype(np.float64)
            m = x.max(1)
            assert (m - np.sort(x, 1)[:, -2] > 50).any()             # (the plant is there)
            ref = m + np.log(np.exp(x - m[:, None]).sum(1))
            bound = (rule.n_chain(Vc) + 4) * 2.0 ** -24 + 2 * np.spacing(np.abs(lse).astype(np.float32)).astype(np.float64)
            err = np.abs(lse.astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            print('LSE constrained V=%d %s theta=%s: max err %.3e, bound %.3e' % (Vc, dtype, theta, err.max(), bound.min()))
            assert (err <= bound).all(), (Vc, dtype, theta, err.max(), bound.min())
    print('LSE constrained worst err / bound = %.3f' % worst)


@pytest.mark.parametrize('Bc,K,Vc,dtype,pitch_tv', [(3, 5, 1003, torch.bfloat16, True), (2, 3, 2100, torch.float32, False)])
def test_constraints_that_ban_nothing_equal_the_plain_step_with_the_bits_of_lse(Bc, K, Vc, dtype, pitch_tv):
    """n = 8 at t = 3, min_len = 0, no penalty: the constrained instantiation runs and bans nothing.  Every output AND the bits of lse
    equal the plain call's: the summation order is the pinned one, and m is the row maximum either way"""
    from gpv1_amd import beam as rule
    T = 6
    for seed, mode, masked in ((1, rule.EXTEND, False), (2, rule.FREEZE, True), (3, rule.FREEZE, False)):
        case = make_constrained_case(seed, Bc, K, Vc, T, 3, dtype, masked=masked, n=8, base_plants=('mixed_fin', 'dupmax', 'stop_top'), penalty=0.6)
        plain, lse0, _ = _device_step(case, mode, T, pitch_tv, constr={})
        got, lse1, _ = _device_step(case, mode, T, pitch_tv)
        ok, what = same(got, plain)
        assert ok, what
        assert np.array_equal(lse0.view(np.uint32), lse1.view(np.uint32))


def _chain(mode, Bc, K, Vc, T, nsteps, constr, seed, stop_boost=12.0):
    """nsteps chained steps: the device state is carried in place, the host rule from its own outputs; three boosted tokens and a
    boosted __stop__ make repeats and finished hypotheses frequent"""
    from gpv1_amd import beam as rule
    from tests.beam_cases import make_case
    stop_id = Vc - 2
    host = {'seq_lp': np.zeros((Bc, K), np.float32), 'seqs': np.zeros((K, Bc, T), np.int64), 'finished': np.zeros((Bc, K), np.int32),
            'length': np.zeros((Bc, K), np.int32)}
    state = None
    inv_pen = rule.length_table(T, 0.6)
    rs = np.random.RandomState(seed)
    hot = rs.choice(Vc - 4, 3, replace=False)
    for t in range(nsteps):
        case = make_case(seed + t, Bc, K, Vc, T, t, torch.bfloat16)
        case['logits'][:, hot] += 14.0
        case['logits'][:, stop_id] += stop_boost
        case['x'] = case['logits'].float().numpy().copy()
        case.update(host, inv_pen=inv_pen, constr=constr)
        got, lse, state = _device_step(case, mode, T, True, state)
        want = _host_step(case, lse, mode)
        ok, what = same(got, want)
        assert ok, (what, t, got[what], want[what])
        host = {k: want[k] for k in host}
    return host, hot, stop_id


@pytest.mark.parametrize('mode_name', ['extend', 'freeze'])
def test_five_chained_constrained_steps_equal_the_host_rule_after_every_step(mode_name):
    from gpv1_amd import beam as rule
    host, hot, stop_id = _chain(rule.MODES[mode_name], 3, 5, 1003, 7, 5, dict(no_repeat_ngram=2, min_length=3, repetition=rule.rep_factors(1.3)), 900)
    body = host['seqs'][:, :, :5]
    assert np.isin(body, hot).mean() > 0.5                            # (the history does draw from the boosted tokens)
    assert not (body[:, :, :3] == stop_id).any()
    if mode_name == 'freeze':
        assert host['finished'].any()


def test_a_chain_of_all_63_steps_equals_the_host_rule_after_every_step():
    from gpv1_amd import beam as rule
    host, hot, stop_id = _chain(rule.FREEZE, 2, 3, 300, 64, 63, dict(no_repeat_ngram=3, min_length=10, repetition=rule.rep_factors(1.2)), 1700,
                                stop_boost=3.0)
    assert host['finished'].any() and (host['length'] == 63).any()   # (frozen parents along the way, and histories of every length)
    for k, b in itertools.product(range(3), range(2)):
        h = host['seqs'][k, b, :int(host['length'][b, k])].tolist()
        grams = list(zip(h, h[1:], h[2:]))
        assert len(set(grams)) == len(grams), h
        assert stop_id not in h[:10]


def test_bad_constraints_are_refused_before_a_launch():
    """V = 65537 with a constraint on, no_repeat = 9, min_len = -1, rep_neg without rep_pos: hipErrorInvalidValue (1) from the C entry
    point through a raw BeamArgs whose pointers are all valid, ValueError from hip_beam.step; nothing is written"""
    from gpv1_amd import hip_beam
    K, Bc, T = 2, 1, 6
    for Vc, fields, kw in ((65537, dict(no_repeat=1), dict(no_repeat_ngram=1)), (65537, dict(min_len=2), dict(min_length=2)),
                           (40, dict(no_repeat=9), dict(no_repeat_ngram=9)), (40, dict(min_len=-1), dict(min_length=-1)),
                           (40, dict(min_len=T + 1), dict(min_length=T + 1)), (40, dict(rep_neg=1.3, rep_pos=0.0), dict(repetition=(1.3, 0.0))),
                           (40, dict(rep_neg=0.0, rep_pos=1.3), dict(repetition=(0.0, 1.3))),
                           (40, dict(rep_neg=float('inf'), rep_pos=1.0), dict(repetition=(float('inf'), 1.0)))):
        lg = torch.randn(K * Bc, Vc, device=DEV)
        lse = torch.full((K * Bc,), 7.0, device=DEV)
        seq_lp = torch.full((Bc, K), -1.0, device=DEV)
        seqs = torch.full((K, Bc, T), 5, dtype=torch.long, device=DEV)
        tok = torch.full((K * Bc,), -1, dtype=torch.long, device=DEV)
        i32 = lambda v: torch.full((Bc, K), v, dtype=torch.int32, device=DEV)
        parent, fin, length = i32(-1), i32(0), i32(2)
        outs = (lse, seq_lp, seqs, tok, parent, fin, length)
        before = [o.clone() for o in outs]
        a = hip_beam.BeamArgs(logits=lg.data_ptr(), pitch=Vc, lse=lse.data_ptr(), seq_lp=seq_lp.data_ptr(), seqs=seqs.data_ptr(), tok=tok.data_ptr(),
                              parent=parent.data_ptr(), finished=fin.data_ptr(), length=length.data_ptr(), B=Bc, K=K, V=Vc, T=T, t=2, mode=0,
                              pad_id=36, stop_id=38, dtype=1, **fields)
        assert hip_beam.lib().gpv_beam_step(C.byref(a), None) == 1, fields
        with pytest.raises(ValueError):
            hip_beam.step(lg, lse, seq_lp, seqs, tok, parent, fin, length, 2, 0, 36, 38, **kw)
        torch.cuda.synchronize()
        assert all(torch.equal(o, b) for o, b in zip(outs, before)), fields
    # the same struct with the constraint taken off is accepted (so the refusals above were the constraints')
    a.rep_neg, a.rep_pos = 0.0, 0.0
    assert hip_beam.lib().gpv_beam_step(C.byref(a), None) == 0
    torch.cuda.synchronize()
    assert int(parent.min()) >= 0


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
    # retire the captured searches the way tests/test_beam_gpu.py does: graphs first, then -- the device idle -- their streams
    torch.cuda.synchronize()
    for key in list(model._igraphs):
        model._drop_igraph(key)
    model._kvdec.clear()
    del model
    import gc
    gc.collect()
    torch.cuda.synchronize()
    ops.RT.set_precise(False)


def _search(model, batch, **kw):
    with torch.no_grad():
        o = model.forward_beam_search(batch[0], batch[1], beam_size=3, impl='device', **kw)
    return o['answers'], o['answer_probs'], o['beam_lengths'].cpu(), o['beam_finished'].cpu()


def _raw(model, batch, **kw):
    """seqs [K,B,T], lengths, finished of one eager search through the public options"""
    model.cfg['graph_inference'] = False
    constr = model._beam_constraints(3, 'device', kw.get('vocab_mask'), None, kw.pop('no_repeat_ngram', None), kw.pop('min_length', None),
                                     kw.pop('repetition_penalty', None))
    with torch.no_grad():
        o = model._beam_device(batch[0], batch[1], 3, impl='device', constraints=constr, **kw)
    torch.cuda.synchronize()
    return o['_beam_seqs'].cpu(), o['beam_lengths'].cpu(), o['beam_finished'].cpu()


def _eq(a, b):
    return a[0] == b[0] and a[1] == b[1] and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


def test_model_graphed_equals_eager_and_a_replay_keeps_its_own_settings(small_model):
    model, batch = small_model
    vm = torch.zeros(V, device=DEV)
    vm[model.word_to_idx['w1']] = 20.0                                # (one favoured word: the unconstrained search repeats it)
    one = dict(no_repeat_ngram=2, min_length=3, repetition_penalty=1.3, finished='freeze', vocab_mask=vm)
    two = dict(no_repeat_ngram=1, finished='freeze', vocab_mask=vm)
    model.cfg['graph_inference'] = False
    eager = {'one': _search(model, batch, **one), 'two': _search(model, batch, **two), 'plain': _search(model, batch, finished='freeze', vocab_mask=vm)}
    assert not _eq(eager['one'], eager['two']) and not _eq(eager['two'], eager['plain'])           # (the settings do change the search)
    model.cfg['graph_inference'] = True
    n0 = len(model._igraphs)
    assert _eq(_search(model, batch, **one), eager['one'])           # capture + first replay
    assert _eq(_search(model, batch, **one), eager['one'])           # second replay
    assert _eq(_search(model, batch, **two), eager['two'])           # other settings: a graph of their own
    assert _eq(_search(model, batch, finished='freeze', vocab_mask=vm), eager['plain'])
    assert _eq(_search(model, batch, **one), eager['one'])           # a replay after calls with other settings: still its own result
    assert len(model._igraphs) == n0 + 3
    # the configuration's group is the fallback of a missing argument
    model.cfg['beam'] = {'no_repeat_ngram': 2, 'min_length': 3, 'repetition_penalty': 1.3}
    assert _eq(_search(model, batch, finished='freeze', vocab_mask=vm), eager['one'])
    del model.cfg['beam']
    model.cfg['graph_inference'] = False


@pytest.mark.parametrize('fin', ['extend', 'freeze'])
def test_model_no_repeat_with_a_mask_of_exactly_k_plus_t_tokens(small_model, fin):
    """a mask that leaves exactly K + T tokens (__stop__ among them): with n = 1 no hypothesis repeats a token -- under extend in
    seqs[..., :T-1], under freeze up to its length -- and the same inputs without the constraint do repeat"""
    model, batch = small_model
    w = model.word_to_idx
    K, T = 3, model.cfg.max_text_len
    keep = [w['__stop__']] + [w['w%d' % i] for i in range(1, K + T)]
    assert len(keep) == K + T
    vm = torch.full((V,), -float('inf'), device=DEV)
    vm[keep] = 0.0
    vm[keep[1]] = 20.0                                                # (one favoured word: the unconstrained search repeats it)
    seqs, length, _ = _raw(model, batch, finished=fin, vocab_mask=vm, no_repeat_ngram=1)
    plain, plen, _ = _raw(model, batch, finished=fin, vocab_mask=vm)
    repeats = lambda s, ln: sum(len(set(s[k, b, :int(ln[b, k])].tolist())) < int(ln[b, k]) for k in range(K) for b in range(s.shape[1]))
    full = torch.full_like(length, T - 1)
    assert repeats(seqs, full if fin == 'extend' else length) == 0
    assert set(seqs[:, :, :T - 1].unique().tolist()) <= set(keep) | {w['__pad__']}
    assert repeats(plain, full if fin == 'extend' else plen) > 0
    with pytest.raises(ValueError, match='at least beam_size'):
        vm[keep[-1]] = -float('inf')
        _raw(model, batch, finished=fin, vocab_mask=vm, no_repeat_ngram=1)


@pytest.mark.parametrize('m', [2, 4])
def test_model_min_length_keeps_stop_behind_position_m(small_model, m):
    model, batch = small_model
    w = model.word_to_idx
    T = model.cfg.max_text_len
    vm = torch.zeros(V, device=DEV)
    vm[w['__stop__']] = 30.0                                          # __stop__ wins wherever it is allowed
    for fin in ('extend', 'freeze'):
        seqs, length, finished = _raw(model, batch, finished=fin, vocab_mask=vm, min_length=m)
        first = lambda row: row.index(w['__stop__']) if w['__stop__'] in row else T
        firsts = [first(seqs[k, b, :T - 1].tolist()) for k in range(3) for b in range(seqs.shape[1])]
        assert min(firsts) == m, firsts
        seqs0, _, _ = _raw(model, batch, finished=fin, vocab_mask=vm)
        assert min(first(seqs0[k, b, :T - 1].tolist()) for k in range(3) for b in range(seqs.shape[1])) == 0


def test_cap_metrics_by_beam_search_returns_the_direct_call_s_captions(small_model):
    from gpv1_amd import metrics
    from gpv1_amd.inference import detokenize
    model, batch = small_model
    beam = {'impl': 'device', 'finished': 'freeze', 'no_repeat_ngram': 2, 'min_length': 2, 'repetition_penalty': 1.2}
    samples = [{'cap_id': 100 + i} for i in range(B)]
    model.cfg['graph_inference'] = False
    with torch.no_grad():
        direct = model.forward_beam_search(batch[0], batch[1], beam_size=3, impl='device', finished='freeze', no_repeat_ngram=2, min_length=2,
                                           repetition_penalty=1.2)
        greedy = metrics.cap_metrics(model, [(batch[0], batch[1], None)], samples)[1]
        _, preds = metrics.cap_metrics(model, [(batch[0], batch[1], None)], samples, beam_size=3, beam=beam)
    assert [preds[str(100 + i)]['answer'] for i in range(B)] == [detokenize(direct['answers'][i][0]) for i in range(B)]
    assert sorted(greedy) == sorted(preds)
