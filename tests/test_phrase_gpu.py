"""libgpv_phrase.so on the GPU: gpv_phrase_step against the host rule (bit-equal, the device's lse handed to the rule), chained steps, its
lse against a float64 logsumexp, and GPV.forward_beam_search(phrases=) / GPV.choose / make_predictions(answer_set='phrases') on the
small fixture."""
import json
import os

import numpy as np
import pytest
import torch

from tests.phrase_cases import make_case, make_set, same, ids, VARIANTS, INT_KEYS
from tests.test_model_cpu import build_small, nested, GOLD, V, B, H, W, Tl, PAD
from tests import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
STATE = ('seq_lp', 'seqs', 'node', 'phrase', 'length')


def _device_step(case, T, pitch_tv, state=None):
    """one gpv_phrase_step on the case; logits either dense (pitch V) or column t of a [K*B, T, V] buffer whose other columns hold +1e4
    (a wrong pitch would pick them up).  -> (result dict of numpy arrays, lse numpy, the device state)"""
    from gpv1_amd import hip_phrase
    lg = case['logits']
    R, Vc = lg.shape
    t = case['t']
    if pitch_tv:
        buf = torch.full((R, T, Vc), 1e4, dtype=lg.dtype, device=DEV)
        buf[:, t] = lg.to(DEV)
        view = buf[:, t]
    else:
        view = lg.to(DEV).contiguous()
    st = state or {k: torch.from_numpy(case[k]).to(DEV) for k in STATE}
    K, Bc = st['seqs'].shape[:2]
    lse = torch.full((R,), -7.0, device=DEV)
    tok = torch.full((R,), -1, dtype=torch.long, device=DEV)
    parent = torch.full((Bc, K), -1, dtype=torch.int32, device=DEV)
    inv_pen = None if case['inv_pen'] is None else torch.from_numpy(case['inv_pen']).to(DEV)
    hip_phrase.step(view, lse, st['seq_lp'], st['seqs'], tok, parent, st['node'], st['phrase'], st['length'], t, case['pset'], inv_pen=inv_pen)
    torch.cuda.synchronize()
    out = dict(st, parent=parent, tok=tok)
    return {k: v.cpu().numpy() for k, v in out.items()}, lse.cpu().numpy(), st


def _host_step(case, lse):
    from gpv1_amd import phrases as P
    return P.phrase_step_host(case['x'], lse, case['seq_lp'], case['seqs'], case['node'], case['phrase'], case['length'], case['t'],
                              case['pad_id'], case['stop_id'], case['pset'], inv_pen=case['inv_pen'])


def _rows_read(case):
    """the rows whose lse the step computes: live parents (at t == 0 slot 0 only); every other row's lse is 0"""
    K, Bc = case['seqs'].shape[:2]
    return np.asarray([case['node'][b, k] >= 0 and (case['t'] > 0 or k == 0) for k in range(K) for b in range(Bc)])


SHAPES = [(1, 1, 37, 4, torch.float32, False), (3, 5, 1003, 6, torch.bfloat16, True), (2, 8, 300, 5, torch.bfloat16, False),
          (1, 2, 2049, 4, torch.bfloat16, True)]


@pytest.mark.parametrize('Bc,K,Vc,T,dtype,pitch_tv', SHAPES)
def test_one_step_equals_the_host_rule_bit_for_bit(Bc, K, Vc, T, dtype, pitch_tv):
    """every output of one step -- parent, tok, seqs, seq_lp, node, phrase, length -- equals phrase_step_host fed with the device's own
    lse; t = 0, 1, T-2; every trie and state variant of tests/phrase_cases.py (a root with 300 children -- V - 3 where the vocabulary
    has fewer --, a chain of one-child nodes, terminal nodes with children, fewer phrases than K, live / DONE / VOID parents mixed,
    twin parents, __stop__ on top, a penalty table)"""
    n = 0
    for t in sorted({0, 1, T - 2}):
        for vi, var in enumerate(VARIANTS):
            case = make_case(100 * t + vi + 17 * K, Bc, K, Vc, T, t, dtype, variant=var)
            if var == 'wide_root':
                root = int(case['pset'].child_off[1])
                assert root == min(300, Vc - 3) and (Vc < 1003 or root > 256)
            got, lse, _ = _device_step(case, T, pitch_tv)
            want = _host_step(case, lse)
            ok, what = same(got, want)
            assert ok, (what, t, var, got[what], want[what])
            read = _rows_read(case)
            assert (lse[~read] == 0).all() and np.isfinite(lse[read]).all(), (t, var, lse)
            n += 1
    assert n == len({0, 1, T - 2}) * len(VARIANTS)


def test_five_chained_steps_equal_the_host_rule_after_every_step():
    """(B, K, V) = (3, 5, 1003), T = 7: the device state is carried in place from step to step, the host rule from its own outputs"""
    from gpv1_amd import beam, phrases as P
    Bc, K, Vc, T = 3, 5, 1003, 7
    pset = make_set('prefix', Vc, K, 5, seed=3)                  # phrases of up to three tokens
    pad_id, stop_id, _ = ids(Vc)
    host = P.initial_state(Bc, K, T)
    state = None
    inv_pen = beam.length_table(T, 0.6)
    g = torch.Generator().manual_seed(77)
    for t in range(5):
        logits = (3.0 * torch.randn(K * Bc, Vc, generator=g)).to(torch.bfloat16)
        case = dict(host, pset=pset, logits=logits, x=logits.float().numpy().copy(), inv_pen=inv_pen, pad_id=pad_id, stop_id=stop_id, t=t)
        got, lse, state = _device_step(case, T, True, state)
        want = _host_step(case, lse)
        ok, what = same(got, want)
        assert ok, (what, t, got[what], want[what])
        host = {k: want[k] for k in STATE}
    assert (host['node'] == P.DONE).any() and (host['phrase'] >= 0).any()
    assert ((host['node'] == P.DONE) == (host['phrase'] >= 0)).all()


@pytest.mark.parametrize('Vc', [37, 1003, 2049, 10000])
def test_lse_against_float64_logsumexp(Vc):
    """|lse - float64 logsumexp over the whole vocabulary| <= (n_chain + 4) * 2^-24 + 2 ulp_fp32(|lse|), the derived bound of
    include/gpv_beam.h and tests/test_beam_gpu.py: the sum's chain of additions, the exponentials and the logarithm, the final add"""
    from gpv1_amd import beam
    worst = 0.0
    for si, scale in enumerate((1.0, 4.0, 12.0)):
        for dtype in (torch.float32, torch.bfloat16):
            case = make_case(50 + si, 2, 2, Vc, 4, 1, dtype, variant='prefix')
            case['logits'] = (case['logits'].float() * (scale / 3.0)).to(dtype)
            case['x'] = case['logits'].float().numpy().copy()
            _, lse, _ = _device_step(case, 4, False)
            read = _rows_read(case)
            assert read.any()
            x = case['x'].astype(np.float64)[read]
            m = x.max(1)
            ref = m + np.log(np.exp(x - m[:, None]).sum(1))
            got = lse[read]
            bound = (beam.n_chain(Vc) + 4) * 2.0 ** -24 + 2 * np.spacing(np.abs(got).astype(np.float32)).astype(np.float64)
            err = np.abs(got.astype(np.float64) - ref)
            worst = max(worst, float((err / bound).max()))
            print('PHRASE LSE V=%d scale=%g %s: max err %.3e, bound %.3e' % (Vc, scale, dtype, err.max(), bound.min()))
            assert (err <= bound).all(), (Vc, scale, dtype, err.max(), bound.min())
    print('PHRASE LSE V=%d worst err / bound = %.3f' % (Vc, worst))


def test_bad_arguments_are_refused_before_a_launch():
    from gpv1_amd import hip_phrase
    case = make_case(1, 2, 3, 40, 6, 1)
    st = {k: torch.from_numpy(case[k]).to(DEV) for k in STATE}
    lg = case['logits'].to(DEV)
    z = lambda *s, d=torch.int32: torch.zeros(*s, dtype=d, device=DEV)
    args = lambda t=1, lg=lg, pset=case['pset']: (lg, z(6, d=torch.float32), st['seq_lp'], st['seqs'], z(6, d=torch.long), z(2, 3), st['node'],
                                                  st['phrase'], st['length'], t, pset)
    with pytest.raises(ValueError, match='step 5 outside'):
        hip_phrase.step(*args(t=5))
    with pytest.raises(ValueError, match='vocabulary of 40'):
        hip_phrase.step(*args(lg=lg[:, :30].contiguous()))
    with pytest.raises(ValueError, match='unit column stride'):
        hip_phrase.step(*args(lg=lg.t().contiguous().t()))
    with pytest.raises(RuntimeError, match='GPU'):
        hip_phrase.step(*args(lg=lg.cpu()))
    with pytest.raises(ValueError, match='longest phrase'):
        hip_phrase.step(*args(pset=make_set('one_child', 40, 3, 8)))
    before = {k: v.clone() for k, v in st.items()}
    assert all(torch.equal(st[k], before[k]) for k in st)


# ---- model level: small fixture, precise mode -----------------------------------------------------------------------------
PHRASES = ['w1', 'w1 w2', 'w3 w4', 'w3 w5', 'w6 w6 w7', 'w8']


@pytest.fixture(scope='module')
def small_model():
    import gpv1_amd.ops as ops
    import gpv1_amd.hip as hip
    from gpv1_amd.phrases import PhraseSet
    hip.lib()
    ops.RT.set_precise(True)
    model, _ = build_small()
    model.to(DEV).eval()
    images, mask, ids_, attn = synth.synth_batch(B, H, W, Tl, V, pad_to=PAD)
    pset = PhraseSet.from_texts(model, PHRASES)
    yield model, (nested(images.to(DEV), mask.to(DEV)), (ids_.to(DEV), attn.to(DEV))), pset
    # retire the whole-search hipGraphs the way the model itself does on an eviction (see tests/test_beam_gpu.py)
    torch.cuda.synchronize()
    for key in list(model._igraphs):
        model._drop_igraph(key)
    model._kvdec.clear()
    del model
    import gc
    gc.collect()
    torch.cuda.synchronize()
    ops.RT.set_precise(False)


def _search(model, batch, pset, K, graphed=False, **kw):
    model.cfg['graph_inference'] = graphed
    try:
        with torch.no_grad():
            o = model.forward_beam_search(batch[0], batch[1], beam_size=K, phrases=pset, **kw)
    finally:
        model.cfg['graph_inference'] = False
    torch.cuda.synchronize()
    return o


def test_model_returns_every_phrase_with_the_models_own_log_probability(small_model):
    """K = 8 >= N = 6: every slot's sequence spells exactly the phrase '_beam_phrase' names, then __stop__, then __pad__; all N phrases
    appear once, the other slots are VOID; '_beam_lp' equals the sum over the slot's tokens of (logit - float64 logsumexp), the logits
    those of the model's own KV decoder step for that prefix (every row walks its final sequence alone: no gpv_phrase_step, no
    reorder).  Tolerance, as tests/test_beam_gpu.py derives it: per step 2 * (n_chain + 4) * 2^-24 (the lse bound, granted twice
    there) + 4 roundings of half an ulp of numbers no larger than M = max(|logit|, |seq_lp|); T - 1 steps add up."""
    from gpv1_amd import beam
    model, batch, pset = small_model
    K, N = 8, len(PHRASES)
    o = _search(model, batch, pset, K)
    seqs, lp, phrase, length = o['_beam_seqs'], o['_beam_lp'].cpu(), o['_beam_phrase'].cpu(), o['beam_lengths']
    w = model.word_to_idx
    T = seqs.shape[2]
    assert phrase.dtype == torch.int32 and tuple(phrase.shape) == (B, K)
    with torch.no_grad():
        _, memory = model._encode(batch[0], batch[1], None)
        kv = [d for k, d in model._kvdec.items() if k[0] == K * B and k[-1] == 'beam'][0]
        kv.memory.copy_(memory.repeat(K, 1, 1).reshape(K * B * memory.shape[1], -1))
        kv._prepare()
        kv.tok.fill_(w['__cls__'])
        want = torch.zeros(K * B, dtype=torch.float64, device=DEV)
        steps = length.t().reshape(K * B)                                   # row k*B + b walks slot (b, k)
        for t in range(T - 1):
            lg = kv._step_core(t).double()
            nxt = seqs[:, :, t].reshape(K * B)
            lsm = lg.gather(1, nxt[:, None])[:, 0] - torch.logsumexp(lg, 1)
            want += torch.where(t < steps, lsm, torch.zeros_like(lsm))
            kv.tok.copy_(nxt)
    want = want.reshape(K, B).t().cpu()
    seqs = seqs.cpu()
    M = max(float(lp[:, :N].abs().max()), 30.0)                      # (|logit| of this fixture stays far below 30)
    bound = (T - 1) * (2 * (beam.n_chain(V) + 4) * 2.0 ** -24 + 4 * 2.0 ** -24 * M)
    for b in range(B):
        assert sorted(phrase[b, :N].tolist()) == list(range(N)) and (phrase[b, N:] == -1).all()
        assert (lp[b, N:] == -1e9).all() and (lp[b, :N - 1] >= lp[b, 1:N]).all()
        for k in range(N):
            toks = list(pset.token_ids[int(phrase[b, k])]) + [w['__stop__']]
            assert seqs[k, b, :T - 1].tolist() == toks + [w['__pad__']] * (T - 1 - len(toks))
            assert o['answers'][b][k] == PHRASES[int(phrase[b, k])].split()
    diff = (lp[:, :N].double() - want[:, :N]).abs()
    print('PHRASE seq_lp against the decoder\'s own logits: max diff %.3e, bound %.3e' % (float(diff.max()), bound))
    assert float(diff.max()) <= bound
    probs = torch.tensor(o['answer_probs'])[:, :N].double()
    assert float((probs - want[:, :N].exp()).abs().max()) <= bound


def test_model_graphed_equals_eager_and_choose_returns_slot_0(small_model):
    model, batch, pset = small_model
    runs = [_search(model, batch, pset, 4, graphed=g, length_penalty=a) for a in (None, 0.6) for g in (False, True, True)]
    for i in (0, 3):
        e = runs[i]
        for r in runs[i + 1:i + 3]:
            for key in ('_beam_seqs', '_beam_lp', '_beam_phrase', 'beam_lengths'):
                assert torch.equal(e[key].cpu(), r[key].cpu()), key           # (fp32 compared for equality: bit-identical or a NaN, and there is none)
            assert e['answers'] == r['answers'] and e['answer_probs'] == r['answer_probs']
    assert not torch.isnan(runs[0]['_beam_lp']).any()
    assert sum(1 for k in model._igraphs if k[0] == 'phrases' and k[3] == pset.digest) == 2
    for graphed in (False, True):
        model.cfg['graph_inference'] = graphed
        try:
            idx, lp = model.choose(batch[0], batch[1], pset, beam_size=4)
        finally:
            model.cfg['graph_inference'] = False
        assert idx.dtype == torch.int64 and lp.dtype == torch.float32 and idx.is_cuda and tuple(idx.shape) == (B,)
        assert torch.equal(idx.cpu(), runs[0]['_beam_phrase'][:, 0].long().cpu()) and torch.equal(lp.cpu(), runs[0]['_beam_lp'][:, 0].cpu())
    # K = 1 is the greedy walk: slot 0 of a wider beam can only be as good or better
    one = _search(model, batch, pset, 1)
    assert (one['_beam_phrase'] >= 0).all() and (runs[0]['_beam_lp'][:, 0] >= one['_beam_lp'][:, 0]).all()


def test_model_refusals(small_model):
    from gpv1_amd.phrases import PhraseSet
    model, batch, pset = small_model
    vm = torch.zeros(V, device=DEV)
    for kw, what in ((dict(vocab_mask=vm), 'vocab_mask'), (dict(impl='torch'), "impl='torch'"), (dict(finished='extend'), "finished='extend'")):
        with pytest.raises(ValueError, match=what):
            model.forward_beam_search(batch[0], batch[1], beam_size=2, phrases=pset, **kw)
    with pytest.raises(ValueError, match='beam size'):
        model.forward_beam_search(batch[0], batch[1], beam_size=9, phrases=pset)
    with pytest.raises(ValueError, match='longest phrase'):
        model.forward_beam_search(batch[0], batch[1], beam_size=2, phrases=PhraseSet.from_texts(model, ['w1 w2 w3 w4 w5']))
    with pytest.raises(ValueError, match='another vocabulary'):
        model.forward_beam_search(batch[0], batch[1], beam_size=2, phrases=make_set('prefix', 300, 2, 6))
    with pytest.raises(ValueError, match='PhraseSet'):
        model.forward_beam_search(batch[0], batch[1], beam_size=2, phrases=PHRASES)


def test_classification_answers_are_class_names_and_the_token_mask_path_is_unchanged(small_model, tmp_path):
    """make_predictions(answer_set='phrases') writes only class names (a synonym answers with its class's name through cls_metrics);
    answer_set='tokens' writes what the default does, which is the recorded output of tests/golden/harness.json (the file
    tests/test_harness_golden.py holds the default path to)"""
    from gpv1_amd import compute_predictions as cp, metrics
    model, _, _ = small_model
    images, mask, ids_, attn = synth.synth_batch(B, H, W, Tl, V, pad_to=PAD)
    ref = json.load(open(os.path.join(GOLD, 'harness.json')))['pred_CocoClassification']
    sids = ref['sample_ids']
    batches = lambda: [(nested(images[i:i + 2].to(DEV), mask[i:i + 2].to(DEV)), (ids_[i:i + 2].to(DEV), attn[i:i + 2].to(DEV)), sids[i:i + 2])
                       for i in (0, 2)]
    classes = ('w2 w9', 'w6', 'w2', 'w11 w3')
    preds, jpath, _ = cp.make_predictions(model, batches(), str(tmp_path / 'p'), 'CocoClassification', answer_set='phrases', classes=classes)
    assert sorted(map(str, preds)) == sorted(map(str, sids)) and all(v['answer'] in classes for v in preds.values())
    assert json.load(open(jpath)) == {str(k): v for k, v in preds.items()}
    tok, _, _ = cp.make_predictions(model, batches(), str(tmp_path / 't'), 'CocoClassification', answer_set='tokens')
    dflt, _, _ = cp.make_predictions(model, batches(), str(tmp_path / 'd'), 'CocoClassification')
    assert {str(k): v for k, v in tok.items()} == ref['predictions'] == {str(k): v for k, v in dflt.items()}
    with pytest.raises(ValueError, match='not in the vocabulary'):
        cp.make_predictions(model, batches(), str(tmp_path / 'x'), 'CocoClassification', answer_set='phrases')    # the COCO names: not this vocabulary's
    # cls_metrics: the same picks through GPV.choose; with synonyms several phrases answer for one class
    samples = [{'id': s, 'answer': preds[s]['answer']} for s in sids]
    assert metrics.cls_metrics(model, batches(), samples, answer_set='phrases', classes=classes) == 1.0
    pset, owner = cp.create_phrase_set(model, classes, synonyms={'w6': ['w6', 'w7 w7'], 'w2': ['w2']}, use_syns=True)
    assert pset.N == 3 and owner == [1, 1, 2]
    with pytest.raises(ValueError, match="names both 'w6' and 'w2'"):
        cp.create_phrase_set(model, classes, synonyms={'w6': ['w6', 'w2'], 'w2': ['w2']}, use_syns=True)


def test_inference_predict_answers_from_a_callers_own_list(small_model):
    """inference.predict(..., answers=[...]): the answer is one of the texts, with its log-probability and the runners-up, best first"""
    from gpv1_amd import inference as inf
    model, _, _ = small_model
    _, _, ids_, attn = synth.synth_batch(B, H, W, Tl, V, pad_to=PAD)
    img = (np.random.RandomState(0).rand(64, 96, 3) * 255).astype(np.uint8)
    answers = ['w2 w9', 'w6', 'w2']
    p = inf.predict(model, [img], (ids_[:1].to(DEV), attn[:1].to(DEV)), answers=answers, num_output_boxes=3)[0]
    ranked = [(p['answer'], p['answer_log_prob'])] + list(p['runners_up'])
    assert sorted(a for a, _ in ranked) == sorted(answers) and p['boxes'].shape == (3, 4)
    lps = [l for _, l in ranked]
    assert all(l <= 0.0 for l in lps) and lps == sorted(lps, reverse=True)
    assert abs(p['answer_prob'] - np.exp(p['answer_log_prob'])) < 1e-6
    with pytest.raises(ValueError, match="'zebra'"):
        inf.predict(model, [img], (ids_[:1].to(DEV), attn[:1].to(DEV)), answers=['w1', 'zebra'])
