"""Mode GPV_BEAM_SAMPLE of gpv_beam_step on the GPU (csrc/sample_step.hip): one step and five chained steps against the host rule
(bit-equal, the device's lse and cand_w handed to the rule), cand_w and lse against float64, the seed read on the device, the C entry
point's refusals, and GPV.forward_sample on the small fixture against the greedy decoder, captured against eager, and the driver."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.sample_cases import make_sample_case, same
from tests.test_model_cpu import build_small, nested, V, B, H, W, Tl, PAD
from tests import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
F32 = np.float32
STATE = ('seq_lp', 'seqs', 'finished', 'length')


def _device_step(case, T, pitch_tv, seed, top_p=None, temperature=None, state=None, seed_t=None):
    """one sampled step on the case; logits dense or column t of a [K*B, T, V] buffer whose other columns hold +1e4.
    -> (result dict of numpy arrays incl. cand_v, lse, cand_w, the device state, the seed tensor)"""
    from gpv1_amd import hip_beam
    lg = case['logits']
    R, Vc = lg.shape
    t, Ck = case['t'], case['top_k']
    if pitch_tv:
        buf = torch.full((R, T, Vc), 1e4, dtype=lg.dtype, device=DEV)
        buf[:, t] = lg.to(DEV)
        view = buf[:, t]
    else:
        view = lg.to(DEV).contiguous()
    st = state or {k: torch.from_numpy(case[k]).to(DEV) for k in STATE}
    K, Bc = st['seqs'].shape[:2]
    lse = torch.zeros(R, device=DEV)
    tok = torch.full((R,), -1, dtype=torch.long, device=DEV)
    parent = torch.full((Bc, K), -1, dtype=torch.int32, device=DEV)
    cand_v = torch.full((R, Ck), -1, dtype=torch.int32, device=DEV)
    cand_w = torch.full((R, Ck), -1.0, device=DEV)
    if seed_t is None:
        seed_t = torch.tensor([seed - (1 << 64) if seed >= (1 << 63) else seed], dtype=torch.long, device=DEV)
    vm = None if case['vocab_mask'] is None else torch.from_numpy(case['vocab_mask']).to(DEV)
    hip_beam.sample_step(view, lse, st['seq_lp'], st['seqs'], tok, parent, st['finished'], st['length'], t, case['pad_id'], case['stop_id'],
                         seed_t, cand_v, cand_w, Ck, top_p=top_p, temperature=temperature, vocab_mask=vm)
    torch.cuda.synchronize()
    out = {'parent': parent, 'tok': tok, 'seqs': st['seqs'], 'seq_lp': st['seq_lp'], 'finished': st['finished'], 'length': st['length'],
           'cand_v': cand_v}
    return {k: v.cpu().numpy() for k, v in out.items()}, lse.cpu().numpy(), cand_w.cpu().numpy(), st, seed_t


def _host_step(case, lse, cand_w, seed, top_p=None, temperature=None):
    from gpv1_amd import beam as rule
    return rule.sample_step_host(case['x'], lse, cand_w, case['seq_lp'], case['seqs'], case['finished'], case['length'], case['t'],
                                 case['pad_id'], case['stop_id'], seed, case['top_k'], top_p=top_p,
                                 inv_temp=rule.inv_temperature(temperature), vocab_mask=case['vocab_mask'])


# (B, K, V, C, dtype, pitch T*V view, the C largest of every row in one lane)
SHAPES = [(1, 1, 37, 37, torch.float32, False, False), (3, 5, 1003, 17, torch.bfloat16, True, False),
          (2, 8, 300, 64, torch.bfloat16, False, False), (2, 3, 3000, 12, torch.float32, False, True),
          (1, 2, 5000, 20, torch.bfloat16, True, True)]         # beyond the issue's table: twenty in one lane, its list runs out twice


@pytest.mark.parametrize('Bc,K,Vc,Ck,dtype,pitch_tv,one_lane', SHAPES)
def test_one_step_equals_the_host_rule_bit_for_bit(Bc, K, Vc, Ck, dtype, pitch_tv, one_lane):
    """parent, tok, seqs, seq_lp, finished, length and cand_v equal sample_step_host fed with the device's own lse and cand_w;
    temperature off and 0.7, top_p off, 0.9 and 1e-6, masked and unmasked; planted: equal logits across the rank C-1 / C boundary, a
    finished slot, __stop__ as a row's top candidate; in the last two shapes the C largest values sit at v = 3, 259, ..., in one lane"""
    T, n = 6, 0
    for temperature in (None, 0.7):
        for pi, top_p in enumerate((None, 0.9, 1e-6)):
            for masked in (False, True):
                t = (0, 1, T - 2)[(n + pi) % 3]
                case = make_sample_case(500 + n + 31 * K, Bc, K, Vc, T, t, Ck, dtype, masked=masked, one_lane=one_lane and not masked)
                seed = (0xABCDEF12 << 32) + 1000 + n
                got, lse, w, _, _ = _device_step(case, T, pitch_tv, seed, top_p, temperature)
                want = _host_step(case, lse, w, seed, top_p, temperature)
                ok, what = same(got, want)
                assert ok, (what, temperature, top_p, masked, t, got[what], want[what])
                assert (got['parent'] == np.arange(K)[None, :]).all() and (want['n'] >= 1).all()
                if one_lane and not masked:
                    assert ((got['cand_v'] % 256 == 3).sum(1) >= Ck - 1).all()       # (the planted __stop__ may take one rank of one row)
                n += 1
    assert n == 12


def test_five_chained_steps_equal_the_host_rule_after_every_step():
    """(B, K, V, C) = (3, 5, 1003, 17), T = 7, bf16, pitch T*V: the device state is carried in place from step to step, the host rule
    from its own outputs; __stop__ is pushed towards the top so that slots finish along the way"""
    Bc, K, Vc, Ck, T = 3, 5, 1003, 17, 7
    stop_id = Vc - 2
    host = {'seq_lp': np.zeros((Bc, K), F32), 'seqs': np.zeros((K, Bc, T), np.int64), 'finished': np.zeros((Bc, K), np.int32),
            'length': np.zeros((Bc, K), np.int32)}
    state, seed = None, 77
    for t in range(5):
        case = make_sample_case(900 + t, Bc, K, Vc, T, t, Ck, torch.bfloat16, plants=False)
        case['logits'][:, stop_id] += 4.0
        case['x'] = case['logits'].float().numpy().copy()
        case.update(host)
        got, lse, w, state, _ = _device_step(case, T, True, seed, 0.9, 0.8, state)
        want = _host_step(case, lse, w, seed, 0.9, 0.8)
        ok, what = same(got, want)
        assert ok, (what, t, got[what], want[what])
        host = {k: want[k] for k in host}
    assert host['finished'].any() and not host['finished'].all()


@pytest.mark.parametrize('Vc,Ck', [(37, 37), (300, 64), (1003, 17), (10000, 64)])
def test_cand_w_and_lse_against_float64(Vc, Ck):
    """|w_j - exp(float64(lp_j))| <= 2 ulp_fp32(w_j) for lp_j >= -80: one ulp for expf, as test_lse_against_float64_logsumexp counts it,
    and one for rounding the reference.  lse is held to that test's own bound, over the rows as they stand after step 1."""
    from gpv1_amd import beam as rule
    for si, (dtype, temperature, masked) in enumerate(((torch.float32, None, False), (torch.bfloat16, 0.7, False), (torch.float32, 0.7, True))):
        case = make_sample_case(60 + si, 2, 2, Vc, 4, 1, Ck, dtype, masked=masked and Vc > Ck)
        got, lse, w, _, _ = _device_step(case, 4, False, 5, None, temperature)
        want = _host_step(case, lse, w, 5, None, temperature)
        ok, what = same(got, want)
        assert ok, what
        lp = want['lp'].astype(np.float64)
        use = lp >= -80.0
        ref = np.exp(np.where(use, lp, 0.0))
        err = np.abs(w.astype(np.float64) - ref)
        ulp = np.spacing(w.astype(F32)).astype(np.float64)
        print('CAND_W V=%d C=%d %s: max err / ulp %.3f over %d weights' % (Vc, Ck, dtype, float((err / ulp)[use].max()), int(use.sum())))
        assert use.sum() >= Ck and (err[use] <= 2 * ulp[use]).all(), float((err / ulp)[use].max())
        inv = rule.inv_temperature(temperature)
        x = case['x'] if inv is None else case['x'] * inv
        x = x.astype(np.float64) + (0.0 if case['vocab_mask'] is None else case['vocab_mask'].astype(np.float64)[None, :])
        m = x.max(1)
        ref = m + np.log(np.exp(x - m[:, None]).sum(1))
        bound = (rule.n_chain(Vc) + 4) * 2.0 ** -24 + 2 * np.spacing(np.abs(lse).astype(F32)).astype(np.float64)
        assert (np.abs(lse.astype(np.float64) - ref) <= bound).all(), (Vc, np.abs(lse - ref).max(), bound.min())


def test_the_seed_is_read_on_the_device():
    """the same seed tensor: identical outputs; the tensor rewritten, the same launch arguments: what the rule predicts for the new seed,
    which differs from the first"""
    Bc, K, Vc, Ck, T = 3, 5, 300, 17, 6
    case = make_sample_case(7, Bc, K, Vc, T, 2, Ck, torch.float32, plants=False)
    a, lse, w, _, seed_t = _device_step(case, T, False, 11)
    b, _, _, _, _ = _device_step(case, T, False, None, seed_t=seed_t)
    assert same(a, b)[0] and same(a, _host_step(case, lse, w, 11))[0]
    new = 0xF00D000000000000 + 12                                    # (the high word and the sign bit of the int64 are part of the seed)
    seed_t.fill_(new - (1 << 64))
    c, lse, w, _, _ = _device_step(case, T, False, None, seed_t=seed_t)
    ok, what = same(c, _host_step(case, lse, w, new))
    assert ok, what
    assert not np.array_equal(a['tok'], c['tok'])


def test_c_entry_refusals_return_1_and_launch_nothing():
    from gpv1_amd import hip_beam
    from gpv1_amd import beam as rule
    Bc, K, Vc, Ck, T = 2, 3, 40, 5, 6
    case = make_sample_case(1, Bc, K, Vc, T, 1, Ck)
    st = {k: torch.from_numpy(case[k]).to(DEV) for k in STATE}
    lg = case['logits'].to(DEV)
    R = K * Bc
    lse, tok, parent = torch.zeros(R, device=DEV), torch.zeros(R, dtype=torch.long, device=DEV), torch.zeros(Bc, K, dtype=torch.int32, device=DEV)
    cand_v, cand_w = torch.full((R, 64), -7, dtype=torch.int32, device=DEV), torch.zeros(R, 64, device=DEV)
    seed_t, pen = torch.tensor([3], dtype=torch.long, device=DEV), torch.ones(T + 1, device=DEV)

    def args(**kw):
        f = dict(logits=lg.data_ptr(), pitch=Vc, lse=lse.data_ptr(), seq_lp=st['seq_lp'].data_ptr(), seqs=st['seqs'].data_ptr(),
                 tok=tok.data_ptr(), parent=parent.data_ptr(), finished=st['finished'].data_ptr(), length=st['length'].data_ptr(),
                 seed=seed_t.data_ptr(), cand_v=cand_v.data_ptr(), cand_w=cand_w.data_ptr(), B=Bc, K=K, V=Vc, T=T, t=1, mode=rule.SAMPLE,
                 pad_id=case['pad_id'], stop_id=case['stop_id'], dtype=1, top_k=Ck, inv_temp=0.0, top_p=0.0)
        f.update(kw)
        return hip_beam.BeamArgs(**f)
    step = lambda a: hip_beam.lib().gpv_beam_step(C.byref(a), None)
    faults = [dict(top_k=65), dict(top_k=41), dict(top_k=0), dict(inv_temp=-1.0), dict(inv_temp=float('inf')), dict(top_p=1.5), dict(seed=None),
              dict(cand_v=None), dict(cand_w=None), dict(no_repeat=2), dict(inv_pen=pen.data_ptr()), dict(min_len=1),
              dict(rep_neg=1.3, rep_pos=0.7), dict(mode=3),
              # and the other modes refuse the sampler's fields
              dict(mode=rule.EXTEND), dict(mode=rule.FREEZE, seed=None, cand_v=None, cand_w=None, top_k=0, top_p=0.5)]
    for kw in faults:
        assert step(args(**kw)) == 1, kw
    torch.cuda.synchronize()
    assert (cand_v == -7).all() and (tok == 0).all()                # nothing was launched
    for kw in (dict(), dict(inv_temp=1.25, top_p=0.5), dict(top_k=40)):       # the same struct with the fault removed is accepted
        assert step(args(**kw)) == 0, kw
    torch.cuda.synchronize()
    flat = cand_v.view(-1)                                           # (the last launch wrote [R, 40] with its own pitch into the buffer)
    assert (flat[:R * 40] >= 0).all() and (flat[:R * 40] < Vc).all() and (flat[R * 40:] == -7).all()
    with pytest.raises(ValueError, match='mode must be EXTEND'):   # hip_beam.step keeps refusing any mode but 0 and 1
        hip_beam.step(lg, lse, st['seq_lp'], st['seqs'], tok, parent, st['finished'], st['length'], 1, rule.SAMPLE, case['pad_id'], case['stop_id'])


# ---- model level: small fixture, precise mode, N = 3 -----------------------------------------------------------------------
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
    # retire this model's whole-search hipGraphs the way the model itself does on an eviction (see tests/test_beam_gpu.py)
    torch.cuda.synchronize()
    for key in list(model._igraphs):
        model._drop_igraph(key)
    model._kvdec.clear()
    del model
    import gc
    gc.collect()
    torch.cuda.synchronize()
    ops.RT.set_precise(False)


def test_top_k_one_is_the_greedy_path(small_model):
    """forward_sample(num_samples=3, top_k=1): all three samples hold the greedy decoder's tokens up to the first __stop__ and __pad__
    behind it, whatever the seed -- an independent check against the existing decoder"""
    model, batch = small_model
    w = model.word_to_idx
    model.cfg['graph_inference'] = False
    with torch.no_grad():
        greedy = model(batch[0], batch[1], None)['answer_logits'][-1].float().argmax(-1).cpu()      # [B, T]
        o = model.forward_sample(batch[0], batch[1], num_samples=3, top_k=1, seed=123)
    seqs = o['_beam_seqs'].cpu()
    K, Bc, T = seqs.shape
    assert (K, Bc) == (3, B) and len(o['answers']) == B and all(len(a) == 3 for a in o['answers'])
    for b in range(Bc):
        want = greedy[b, :T - 1].tolist()
        if w['__stop__'] in want:
            i = want.index(w['__stop__'])
            want = want[:i + 1] + [w['__pad__']] * (T - 2 - i)
        for k in range(K):
            assert seqs[k, b, :T - 1].tolist() == want, (b, k)
    assert (o['beam_lengths'].cpu() <= T - 1).all()


def test_graphed_equals_eager_and_a_replay_with_another_seed_samples_anew(small_model):
    model, batch = small_model
    kw = dict(num_samples=3, top_k=8, temperature=0.9, top_p=0.9)
    runs = {}
    with torch.no_grad():
        for graphed, seed in ((False, 5), (True, 5), (True, 5), (True, 6), (False, 6)):      # eager, capture + first replay, replay, new seed
            model.cfg['graph_inference'] = graphed
            o = model.forward_sample(batch[0], batch[1], seed=seed, **kw)
            runs.setdefault(seed, []).append((o['_beam_seqs'].cpu(), o['_beam_lp'].cpu()))
    model.cfg['graph_inference'] = False
    assert sum(1 for k in model._igraphs if k[0] == 'sample') == 1
    for seed, rs in runs.items():
        for s, lp in rs[1:]:
            assert torch.equal(s, rs[0][0]) and torch.equal(lp, rs[0][1]), seed
    assert not torch.equal(runs[5][0][0], runs[6][0][0])
    # torch.manual_seed makes an unseeded run repeatable
    with torch.no_grad():
        torch.manual_seed(9)
        a = model.forward_sample(batch[0], batch[1], **kw)['_beam_seqs'].cpu()
        torch.manual_seed(9)
        b = model.forward_sample(batch[0], batch[1], **kw)['_beam_seqs'].cpu()
    assert torch.equal(a, b)


def test_predict_with_sample_returns_n_answers(small_model):
    from gpv1_amd import inference as inf
    model, batch = small_model
    img = (np.random.RandomState(0).rand(64, 96, 3) * 255).astype(np.uint8)
    q = (batch[1][0][:1], batch[1][1][:1])
    pred = inf.predict(model, [img], q, num_output_boxes=3, sample={'num': 3, 'temperature': 0.8, 'top_k': 20, 'top_p': 0.9, 'seed': 1})[0]
    assert len(pred['samples']) == 3 and all(isinstance(s, str) and 0.0 <= p <= 1.0 for s, p in pred['samples'])
    assert pred['answer'] == pred['samples'][0][0] and pred['answer_prob'] == pred['samples'][0][1]
