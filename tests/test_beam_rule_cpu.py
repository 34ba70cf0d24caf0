"""The beam step rule on the host (gpv1_amd.beam), no GPU: against a second restatement (tests/beam_ref.py), against a case worked out
by hand, against the reference's golden search (small_beam.json) through the oracle's decoder; the constants of include/gpv_beam.h (exports and
struct layouts: tests/test_abi_cpu.py); the drivers' beam.* keys reaching hip_beam; the three ValueErrors of the torch path."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import synth, cpu_shim, beam_ref
from tests.beam_cases import make_case, same, PLANTS
from tests.test_model_cpu import build_small, GOLD, V, B, H, W, Tl, PAD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gpv_beam.h')


def _host(case, mode):
    from gpv1_amd import beam as rule
    lse = rule.lse_host(case['x'], case['vocab_mask'])
    args = (case['x'], lse, case['seq_lp'], case['seqs'], case['finished'], case['length'], case['t'], mode, case['pad_id'], case['stop_id'])
    kw = dict(inv_pen=case['inv_pen'], vocab_mask=case['vocab_mask'])
    return rule.beam_step_host(*args, **kw), beam_ref.step(*args, **kw)


def test_host_rule_equals_second_restatement_exactly():
    """>= 200 random cases over K in {1,2,3,5,8}, V in {K,37,300}, B in {1,3}, both modes, with / without penalty table and mask, the
    planted situations one by one and all together; every output equal, seq_lp as bit patterns"""
    from gpv1_amd import beam as rule
    rs = np.random.RandomState(0)
    n = 0
    plant_sets = [(), PLANTS] + [(p,) for p in PLANTS]
    for K in (1, 2, 3, 5, 8):
        for Vc in (K, 37, 300):
            for Bc in (1, 3):
                for rep in range(8):
                    T = int(rs.randint(3, 9))
                    t = int(rs.choice([0, 1, T - 2]))
                    dtype = torch.bfloat16 if rep % 2 else torch.float32
                    case = make_case(1000 * n + 7, Bc, K, Vc, T, t, dtype, plants=plant_sets[(n + rep) % len(plant_sets)],
                                     masked=rep % 4 >= 2, penalty=[None, 0.6, None, 2.0][(rep + n) % 4])
                    for mode in (rule.EXTEND, rule.FREEZE):
                        a, b = _host(case, mode)
                        ok, what = same(a, b)
                        assert ok, (what, K, Vc, Bc, T, t, rep, mode)
                        if mode == rule.EXTEND:
                            assert not np.any(a['finished'])
                        n += 1
    assert n >= 200, n


def test_planted_situations_do_what_the_rule_says():
    from gpv1_amd import beam as rule
    # a duplicated row maximum: the lower index is the better candidate
    x = np.full((1, 6), -3.0, np.float32)
    x[0, 4] = x[0, 1] = 2.0
    z = lambda *s, d=np.int32: np.zeros(s, d)
    o = rule.beam_step_host(np.repeat(x, 2, 0), rule.lse_host(np.repeat(x, 2, 0)), z(1, 2, d=np.float32), z(2, 1, 4, d=np.int64), z(1, 2), z(1, 2),
                            0, rule.EXTEND, 0, 5)
    assert o['tok'].tolist() == [1, 4] and o['parent'].tolist() == [[0, 0]]
    # two parents with identical rows and identical seq_lp (t > 0): candidates tie across k1, the lower k1*K + k2 wins
    o = rule.beam_step_host(np.repeat(x, 2, 0), rule.lse_host(np.repeat(x, 2, 0)), z(1, 2, d=np.float32), z(2, 1, 4, d=np.int64), z(1, 2),
                            np.ones((1, 2), np.int32), 1, rule.EXTEND, 0, 5)
    assert o['parent'].tolist() == [[0, 0]] and o['tok'].tolist() == [1, 4]
    # __stop__ as top-1 finishes the slot in FREEZE only
    for mode, fin in ((rule.FREEZE, [[1, 0]]), (rule.EXTEND, [[0, 0]])):
        o = rule.beam_step_host(np.repeat(x, 2, 0), rule.lse_host(np.repeat(x, 2, 0)), z(1, 2, d=np.float32), z(2, 1, 4, d=np.int64), z(1, 2),
                                z(1, 2), 0, mode, 0, 1)
        assert o['finished'].tolist() == fin and o['length'].tolist() == [[1, 1]]


# ---- the case worked out by hand: K = 2, V = 4 (0 __pad__, 1 __stop__, 2 a, 3 b), T = 4, B = 1, three steps.  Every logit is a dyadic
# ---- fraction and every row's lse is handed in as 0, so the logits ARE the log-probabilities and every score below is exact.
PAD_, STOP_, A_, B_ = 0, 1, 2, 3
ROW0 = [-8.0, -0.5, -0.625, -4.0]                 # t = 0, both rows (parent 1 is killed by -1e9): __stop__ -0.5, a -0.625
AFTER_STOP_1 = [-0.25, -3.0, -5.0, -2.0]          # t = 1 behind [__stop__]: junk, mostly __pad__
AFTER_A_1 = [-8.0, -6.0, -0.0625, -3.0]           # t = 1 behind [a]: a again
AFTER_AA_2 = [-8.0, -0.0625, -2.0, -3.0]          # t = 2 behind [a, a]: __stop__
AFTER_STOP_PAD_2 = [-0.125, -4.0, -5.0, -6.0]     # t = 2 behind [__stop__, __pad__]: junk
HAND = {
    # FREEZE, no penalty: the finished hypothesis keeps -0.5 bit for bit, is followed by __pad__ and stays first
    ('freeze', 0.0): {
        'rows': [[ROW0, ROW0], [AFTER_STOP_1, AFTER_A_1], [AFTER_STOP_PAD_2, AFTER_AA_2]],
        'steps': [dict(parent=[[0, 0]], seqs=[[STOP_, 0, 0, 0], [A_, 0, 0, 0]], seq_lp=[[-0.5, -0.625]], finished=[[1, 0]], length=[[1, 1]]),
                  dict(parent=[[0, 1]], seqs=[[STOP_, PAD_, 0, 0], [A_, A_, 0, 0]], seq_lp=[[-0.5, -0.6875]], finished=[[1, 0]], length=[[1, 2]]),
                  dict(parent=[[0, 1]], seqs=[[STOP_, PAD_, PAD_, 0], [A_, A_, STOP_, 0]], seq_lp=[[-0.5, -0.75]], finished=[[1, 1]], length=[[1, 3]])]},
    # FREEZE, alpha = 2: inv_pen = 1, (6/7)^2 = 0.7347, (3/4)^2 = 0.5625 at lengths 1, 2, 3.  Step 1: -0.6875 * 0.7347 = -0.5051 < -0.5, not yet;
    # step 2: -0.75 * 0.5625 = -0.421875 > -0.5: the longer hypothesis overtakes the finished one, whose raw score is still -0.5
    ('freeze', 2.0): {
        'rows': [[ROW0, ROW0], [AFTER_STOP_1, AFTER_A_1], [AFTER_STOP_PAD_2, AFTER_AA_2]],
        'steps': [dict(parent=[[0, 0]], seqs=[[STOP_, 0, 0, 0], [A_, 0, 0, 0]], seq_lp=[[-0.5, -0.625]], finished=[[1, 0]], length=[[1, 1]]),
                  dict(parent=[[0, 1]], seqs=[[STOP_, PAD_, 0, 0], [A_, A_, 0, 0]], seq_lp=[[-0.5, -0.6875]], finished=[[1, 0]], length=[[1, 2]]),
                  dict(parent=[[1, 0]], seqs=[[A_, A_, STOP_, 0], [STOP_, PAD_, PAD_, 0]], seq_lp=[[-0.75, -0.5]], finished=[[1, 1]], length=[[3, 1]])]},
    # EXTEND: the hypothesis that emitted __stop__ keeps collecting junk (-0.5 -> -0.75 -> -0.875), nothing is ever finished, and the
    # longer one passes it already at step 1 on raw scores
    ('extend', 0.0): {
        'rows': [[ROW0, ROW0], [AFTER_STOP_1, AFTER_A_1], [AFTER_AA_2, AFTER_STOP_PAD_2]],
        'steps': [dict(parent=[[0, 0]], seqs=[[STOP_, 0, 0, 0], [A_, 0, 0, 0]], seq_lp=[[-0.5, -0.625]], finished=[[0, 0]], length=[[1, 1]]),
                  dict(parent=[[1, 0]], seqs=[[A_, A_, 0, 0], [STOP_, PAD_, 0, 0]], seq_lp=[[-0.6875, -0.75]], finished=[[0, 0]], length=[[2, 2]]),
                  dict(parent=[[0, 1]], seqs=[[A_, A_, STOP_, 0], [STOP_, PAD_, PAD_, 0]], seq_lp=[[-0.75, -0.875]], finished=[[0, 0]], length=[[3, 3]])]},
}


@pytest.mark.parametrize('which', list(HAND))
@pytest.mark.parametrize('impl', ['host', 'ref'])
def test_hand_computed_case(which, impl):
    from gpv1_amd import beam as rule
    finished_mode, alpha = which
    mode = rule.MODES[finished_mode]
    inv_pen = rule.length_table(4, alpha) if alpha else None
    if alpha:
        assert inv_pen[1] == 1.0 and inv_pen[3] == np.float32(0.5625) and abs(float(inv_pen[2]) - 36 / 49) < 1e-7
    st = {'seq_lp': np.zeros((1, 2), np.float32), 'seqs': np.zeros((2, 1, 4), np.int64), 'finished': np.zeros((1, 2), np.int32),
          'length': np.zeros((1, 2), np.int32)}
    for t, (rows, want) in enumerate(zip(HAND[which]['rows'], HAND[which]['steps'])):
        x = np.asarray(rows, np.float32)
        lse = np.zeros(2, np.float32)
        if impl == 'host':
            o = rule.beam_step_host(x, lse, st['seq_lp'], st['seqs'], st['finished'], st['length'], t, mode, PAD_, STOP_, inv_pen=inv_pen)
        else:
            o = beam_ref.step(x, lse, st['seq_lp'], st['seqs'].tolist(), st['finished'].tolist(), st['length'].tolist(), t, mode, PAD_, STOP_,
                              inv_pen=inv_pen)
        assert np.asarray(o['parent']).tolist() == want['parent'], (t, o['parent'])
        assert np.asarray(o['seqs'])[:, 0].tolist() == want['seqs'], (t, o['seqs'])
        assert np.array_equal(np.asarray(o['seq_lp'], np.float32).view(np.uint32), np.asarray(want['seq_lp'], np.float32).view(np.uint32)), (t, o['seq_lp'])
        assert np.asarray(o['finished']).tolist() == want['finished'] and np.asarray(o['length']).tolist() == want['length'], (t, o)
        assert np.asarray(o['tok']).tolist() == [want['seqs'][0][t], want['seqs'][1][t]]
        st = {k: np.asarray(o[k], dtype=st[k].dtype) for k in st}


def test_search_through_the_oracle_decoder_reproduces_the_reference_golden():
    """beam_search_host (EXTEND, no penalty, K = 3) driven by the oracle's text decoder on the small fixture, set up like
    tests/test_oracle_golden.py::test_beam: the answers of small_beam.json, probabilities to that test's 1e-4.  (Smallest gap between
    a selected candidate and the next in this search: 3.0e-3; inside a row's top-(K+1): 5.1e-4 -- far above lp's rounding.)"""
    from oracle import gpv_oracle as O
    from gpv1_amd import beam as rule
    man = json.load(open(os.path.join(GOLD, 'small_manifest.json')))
    Pm = synth.synth_state(man['manifest'])
    Pm['pos_enc'] = torch.zeros(1, 30, 768)
    cfg = synth.small_cfg(dropout=0.0)
    cfg['_cls_id'] = V - 3
    images, mask, ids, attn = synth.synth_batch(B, H, W, Tl, V, pad_to=PAD)
    ref = json.load(open(os.path.join(GOLD, 'small_beam.json')))
    vocab = synth.make_vocab(V)
    K, T = 3, cfg['max_text_len']
    with torch.no_grad():
        _, memory = O.gpv_encode(Pm, cfg, images, mask, ids, attn)

        def step_logits(t, tok):
            rows = [O.decode_text(Pm, cfg, O.answer_input_embed(Pm, torch.as_tensor(tok[k])), memory)[:, -1] for k in range(K)]
            return torch.cat(rows, 0).numpy()
        out = rule.beam_search_host(step_logits, B, K, T, V - 3, V - 4, V - 2, mode=rule.EXTEND)
    answers = []
    for b in range(B):
        answers.append([])
        for k in range(K):
            words = []
            for t in range(T):
                wd = vocab[int(out['seqs'][k, b, t])]
                if wd in ('__stop__', '__pad__'):
                    break
                words.append(wd)
            answers[b].append(words)
    assert answers == ref['answers']
    probs, want = np.exp(out['seq_lp'].astype(np.float64)), np.asarray(ref['answer_probs'])
    assert np.abs(probs - want).max() <= 1e-4 * max(np.abs(want).max(), 1.0)
    assert not out['finished'].any() and (out['length'] == T - 1).all()
    assert not (out['seqs'] == V - 2).any()          # this search never emits __stop__: finishing is covered by the synthetic cases


def test_header_declares_exactly_the_exports_and_the_library_has_them():
    """exports, header and nm: tests/test_abi_cpu.py, for every library; here the constants of the beam library's own header"""
    import gpv1_amd.hip_beam as hip_beam
    # the constants the Python side repeats
    src = open(HEADER).read()
    consts = {k: int(v) for k, v in re.findall(r'#define (GPV_BEAM_\w+) (\d+)', src)}
    from gpv1_amd import beam as rule
    assert (consts['GPV_BEAM_MAX_K'], consts['GPV_BEAM_MAX_T'], consts['GPV_BEAM_MAX_LAYERS'], consts['GPV_BEAM_LANES']) == \
        (rule.MAX_K, rule.MAX_T, hip_beam.MAX_LAYERS, rule.LANES)
    assert (consts['GPV_BEAM_EXTEND'], consts['GPV_BEAM_FREEZE']) == (rule.EXTEND, rule.FREEZE)
    assert (consts['GPV_BEAM_BF16'], consts['GPV_BEAM_F32']) == (hip_beam._DTYPES[torch.bfloat16], hip_beam._DTYPES[torch.float32])
    assert rule.n_chain(10000) == 40 + 9 and rule.n_chain(256) == 1 + 9 and rule.n_chain(257) == 2 + 9


# ---- host emulation of the two entry points (CPU tensors, the host rule): what the drivers reach through hip_beam ----
def _emulate(monkeypatch, calls):
    import gpv1_amd.hip_beam as hip_beam
    from gpv1_amd import beam as rule

    def step(logits, lse, seq_lp, seqs, tok, parent, finished, length, t, mode, pad_id, stop_id, inv_pen=None, vocab_mask=None):
        x = logits.float().numpy()
        vm = None if vocab_mask is None else vocab_mask.numpy()
        l = rule.lse_host(x, vm)
        o = rule.beam_step_host(x, l, seq_lp.numpy(), seqs.numpy(), finished.numpy(), length.numpy(), t, mode, pad_id, stop_id,
                                inv_pen=None if inv_pen is None else inv_pen.numpy(), vocab_mask=vm)
        lse.copy_(torch.from_numpy(l))
        for dst, k in ((seq_lp, 'seq_lp'), (seqs, 'seqs'), (tok, 'tok'), (parent, 'parent'), (finished, 'finished'), (length, 'length')):
            dst.copy_(torch.from_numpy(o[k]))
        calls.append(('step', t, mode, inv_pen is not None, vocab_mask is not None))

    def reorder(caches, parent, upto):
        Bc, K = parent.shape
        D = caches[0].shape[2] // 3
        perm = (parent.t().long() * Bc + torch.arange(Bc)[None, :]).reshape(K * Bc)
        for c in caches:
            c[:, :upto, D:] = c[:, :upto, D:].index_select(0, perm)
        calls.append(('reorder', upto))
    monkeypatch.setattr(hip_beam, 'step', step)
    monkeypatch.setattr(hip_beam, 'reorder', reorder)


@pytest.fixture()
def shim():
    import gpv1_amd.ops as ops
    undo = cpu_shim.install()
    ops.RT.set_precise(True)
    yield
    ops.RT.set_precise(False)
    undo()


def _query():
    g = torch.Generator().manual_seed(0)
    return (torch.randint(1000, 30000, (1, 5), generator=g), torch.ones(1, 5, dtype=torch.long))


def test_predict_passes_the_beam_keys_through_to_hip_beam(shim, monkeypatch):
    from gpv1_amd import inference as inf
    from gpv1_amd import beam as rule
    model, _ = build_small()
    model.eval()
    calls = []
    _emulate(monkeypatch, calls)
    img = (np.random.RandomState(0).rand(64, 96, 3) * 255).astype(np.uint8)
    T = model.cfg.max_text_len
    pt = inf.predict(model, [img], _query(), beam_size=2, num_output_boxes=3)[0]                  # default: the torch path
    assert not calls
    pd = inf.predict(model, [img], _query(), beam_size=2, num_output_boxes=3, beam={'impl': 'device'})[0]
    steps = [c for c in calls if c[0] == 'step']
    assert [c[1] for c in steps] == list(range(T - 1)) and all(c[2:] == (rule.EXTEND, False, False) for c in steps)
    assert [c[1] for c in calls if c[0] == 'reorder'] == list(range(1, T - 1))
    assert pd['answer'] == pt['answer'] and abs(pd['answer_prob'] - pt['answer_prob']) <= 1e-5 * pt['answer_prob']
    del calls[:]
    inf.predict(model, [img], _query(), beam_size=2, beam={'impl': 'device', 'finished': 'freeze', 'length_penalty': 0.6})
    steps = [c for c in calls if c[0] == 'step']
    assert len(steps) == T - 1 and all(c[2:] == (rule.FREEZE, True, False) for c in steps)
    # the same keys as the model's own configuration and as the environment's default
    del calls[:]
    model.cfg['beam'] = {'impl': 'device', 'finished': 'freeze'}
    inf.predict(model, [img], _query(), beam_size=2)
    assert len([c for c in calls if c[0] == 'step' and c[2] == rule.FREEZE]) == T - 1
    del model.cfg['beam']
    del calls[:]
    monkeypatch.setenv('GPV_BEAM', 'device')
    inf.predict(model, [img], _query(), beam_size=2)
    assert len([c for c in calls if c[0] == 'step']) == T - 1
    # compute_predictions: beam search with the classification mask reaches the device step with the mask
    from gpv1_amd import compute_predictions as cp
    del calls[:]
    _, vm = cp.create_vocab_mask(model, classes=('w2', 'w6'))
    batch = [([inf.preprocess_image(img)], _query(), ['s0'])]
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        preds, _, _ = cp.make_predictions(model, batch, d, 'CocoClassification', vocab_mask=vm, beam_size=2, beam={'impl': 'device', 'finished': 'freeze'})
    assert all(c[2:] == (rule.FREEZE, False, True) for c in calls if c[0] == 'step') and len(calls) > 0
    # (slot T - 1 of a hypothesis is never written and reads as id 0 = 'w0' when nothing stopped before it: the reference's quirk, kept)
    assert set(preds['s0']['answer'].split()[:T - 1]) <= {'w2', 'w6'}


def test_device_impl_without_a_gpu_is_an_error_not_a_fallback(shim):
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    model, _ = build_small()
    model.eval()
    imgs = nested_tensor_from_tensor_list([torch.zeros(3, 64, 96)])
    with pytest.raises(RuntimeError, match='GPU'):                       # CPU tensors: hip_beam refuses, nothing falls back to torch
        model.forward_beam_search(imgs, _query(), beam_size=2, impl='device')
    model.cfg['kv_decode'] = False
    with pytest.raises(RuntimeError, match='KV-cached'):
        model.forward_beam_search(imgs, _query(), beam_size=2, impl='device')


def test_torch_path_refuses_the_new_rules(shim):
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    model, _ = build_small()
    model.eval()
    imgs = nested_tensor_from_tensor_list([torch.zeros(3, 64, 96)])
    with pytest.raises(ValueError, match="finished='freeze'"):
        model.forward_beam_search(imgs, _query(), beam_size=2, impl='torch', finished='freeze')
    with pytest.raises(ValueError, match='length penalty'):
        model.forward_beam_search(imgs, _query(), beam_size=2, impl='torch', length_penalty=0.6)
    with pytest.raises(ValueError, match='vocabulary mask'):
        model.forward_beam_search(imgs, _query(), beam_size=2, vocab_mask=torch.zeros(V))
    with pytest.raises(ValueError, match='impl must be'):
        model.forward_beam_search(imgs, _query(), beam_size=2, impl='triton')
