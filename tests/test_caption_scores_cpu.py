"""Caption scoring on the CPU: the host rule (gpv1_amd.evaluators.caption_scores_host) against closed forms and against the independent
restatement tests/caption_ref.py, the CocoCaptioning pairing, the tokenizer, CaptionScorer(host=True) through the metric loop and the
training driver, and the ABI of libgpv_cap.so.  (The device scorer needs the GPU: tests/test_caption_scores_gpu.py.)

Bound of the host rule against the restatement, 1e-12 per entry: both sides are float64 on the same two tables; every sum has at most
64 non-negative terms (a caption has at most 64 windows), so summing in another order moves a sum by at most 64 * 2^-53 = 7e-15 of
its value, and the handful of sums, two square roots and one division behind an entry score of at most 10 stay below 1e-13."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from tests import caption_ref, cpu_shim
from tests.test_det_metrics_cpu import _EvalSet, _driver_cfg
from tests.test_model_cpu import build_small

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ['Bleu1', 'Bleu2', 'Bleu3', 'Bleu4', 'Cider']


@pytest.fixture(scope='module')
def shim():
    import gpv1_amd.ops as ops
    undo = cpu_shim.install()
    ops.RT.set_precise(True)
    yield
    ops.RT.set_precise(False)
    undo()


def W(s):
    return s.split()


def test_cider_closed_forms():
    from gpv1_amd.evaluators import caption_scores_host as score
    # two entries, each its own single reference: every n-gram has df 1, hypothesis = reference -> cosine 1 at all four orders
    out = score([W('a b c d'), W('e f g h')], [[W('a b c d')], [W('e f g h')]])
    assert out['cider_entries'].tolist() == [10.0, 10.0] and out['Cider'] == 10.0
    assert out['cider_entries'].dtype == np.float64
    # three words: no 4-gram, that norm is 0 and the order contributes 0
    out = score([W('a b c'), W('e f g')], [[W('a b c')], [W('e f g')]])
    assert out['cider_entries'].tolist() == [7.5, 7.5] and out['Cider'] == 7.5
    # a single entry: every weight is log(1) - log(1) = 0
    out = score([W('a b c d')], [[W('a b c d')]])
    assert out['cider_entries'].tolist() == [0.0] and out['Cider'] == 0.0
    # hypothesis a b c d e against a b c d: the shared n-grams are 4, 3, 2, 1 of the hypothesis' 5, 4, 3, 2 (all weights equal, 'e'
    # occurs in the other entry's reference and has the same df 1), cosines 4/sqrt(5*4), 3/sqrt(4*3), 2/sqrt(3*2), 1/sqrt(2*1); the
    # bigram counts differ by 1
    out = score([W('a b c d e'), W('e f g h')], [[W('a b c d')], [W('e f g h')]])
    want = 10 * math.exp(-1 / 72) * (2 / math.sqrt(5) + math.sqrt(3) / 2 + 2 / math.sqrt(6) + 1 / math.sqrt(2)) / 4
    assert abs(want - 8.0968983911967) < 1e-12
    assert abs(out['cider_entries'][0] - want) < 1e-12 and out['cider_entries'][1] == 10.0
    assert abs(out['Cider'] - (want + 10.0) / 2) < 1e-12


def test_bleu_cases():
    from gpv1_amd.evaluators import caption_scores_host as score
    # the clipping example of the Bleu paper
    out = score([W('the the the the the the the')], [[W('the cat is on the mat'), W('there is a cat on the mat')]])
    assert out['bleu_totals'] == {'testlen': 7, 'reflen': 7, 'guess': [7, 6, 5, 4], 'correct': [2, 0, 0, 0]}
    assert abs(out['Bleu1'] - 2 / 7) < 1e-9
    assert out['bleu_entries']['correct'].tolist() == [[2, 0, 0, 0]] and out['bleu_entries']['reflen'].tolist() == [7]
    # 5 words against 4 and 6: the tie goes to the shorter reference, and 5 > 4 means no brevity penalty
    for refs in ([W('a b c d'), W('u v w x y z')], [W('u v w x y z'), W('a b c d')]):
        out = score([W('a b c d e')], [refs])
        assert out['bleu_totals']['reflen'] == 4 and out['bleu_totals']['correct'] == [4, 3, 2, 1]
        b, want = 1.0, []
        for k, (c, g) in enumerate(zip([4, 3, 2, 1], [5, 4, 3, 2])):
            b *= c / g
            want.append(b ** (1 / (k + 1)))
        assert all(abs(out[f'Bleu{k + 1}'] - want[k]) < 1e-9 for k in range(4))
    # a hypothesis shorter than its reference pays exp(1 - reflen / testlen)
    out = score([W('a b c')], [[W('a b c d e f')]])
    assert abs(out['Bleu1'] - math.exp(1 - 6 / 3)) < 1e-9
    # an empty hypothesis: zeros, no exception
    out = score([[]], [[W('a b c')]])
    assert [out[k] for k in KEYS] == [0.0] * 5
    assert out['bleu_totals'] == {'testlen': 0, 'reflen': 3, 'guess': [0, 0, 0, 0], 'correct': [0, 0, 0, 0]}
    with pytest.raises(ValueError):
        score([W('a')], [[]])


@pytest.fixture(scope='module')
def random_case():
    """257 entries, a 5-word vocabulary, hypotheses of 0..20 words, 1..8 references of 0..64 words: computed once, read by the tests"""
    from gpv1_amd.evaluators import caption_scores_host
    hyps, refs = caption_ref.random_case(257, [3, 1, 4, 15, 9], seed=20240531)
    return hyps, refs, caption_scores_host(hyps, refs), caption_ref.scores(hyps, refs)


def test_host_rule_equals_the_independent_restatement(random_case):
    hyps, refs, host, ref = random_case
    assert sorted({len(h) for h in hyps}) == list(range(21)) and {len(rs) for rs in refs} == set(range(1, 9))
    assert {0, 64} <= {len(r) for rs in refs for r in rs}
    for k in ('testlen', 'reflen', 'guess', 'correct'):
        assert np.array_equal(host['bleu_entries'][k], ref[k]), k
        assert np.array_equal(np.asarray(host['bleu_totals'][k]), ref[k].sum(0)), k
    worst = float(np.abs(host['cider_entries'] - ref['cider']).max())
    print('Cider %.6f   entries %.4f .. %.4f   Bleu4 %.6f   worst |host - restatement| %.3e' %
          (host['Cider'], host['cider_entries'].min(), host['cider_entries'].max(), host['Bleu4'], worst))
    assert worst <= 1e-12
    for k in KEYS:
        assert abs(host[k] - ref[k]) <= 1e-12, k
    # not degenerate: scores spread out, clipping happens, and the brevity penalty is not what decides Bleu
    assert 0.1 < host['Cider'] < 5 and host['cider_entries'].min() == 0.0 and host['cider_entries'].max() > 2 and 0.05 < host['Bleu4'] < 0.9
    # the document frequencies: the dict of the host rule against the restatement's array, position by position
    df = host['df']
    for i in (0, 100, 256):
        for j, r in enumerate(refs[i]):
            for n in range(1, 5):
                for p in range(len(r) - n + 1):
                    assert ref['ref_df'][i, j, n - 1, p] == df[tuple(r[p:p + n])]
    assert 200 < df[(3,)] <= 257 and max(df.values()) <= 257


def test_coco_captioning_pairing():
    from gpv1_amd.evaluators import CocoCaptioning, caption_scores_host
    img = lambda i, subset='val2014': {'image_id': i, 'subset': subset}
    samples = [{'cap_id': 1, 'answer': 'A dog runs.', 'image': img(7), 'coco_categories': {'seen': ['dog'], 'unseen': []}},
               {'cap_id': 2, 'answer': 'a brown dog is running', 'image': img(7), 'coco_categories': {'seen': ['dog'], 'unseen': []}},
               {'cap_id': 3, 'answer': 'Two cats sleep', 'image': img(8), 'coco_categories': {'seen': [], 'unseen': ['cat']}},
               {'cap_id': 4, 'answer': 'a train', 'image': img(7, 'train2014'), 'coco_categories': {'seen': ['train'], 'unseen': []}}]
    preds = {'1': {'answer': 'A DOG RUNS'}, '3': {'answer': 'two cats'}, '4': {'answer': 'a bus'}}
    seen = {}

    def spy(hyps, refs):
        seen['hyps'], seen['refs'] = hyps, refs
        return caption_scores_host(hyps, refs)
    m = CocoCaptioning(samples, preds, None, scores=spy).evaluate()
    assert set(m) == {'absent', 'total', 'scores'} and m['absent'] == 1 and m['total'] == 3 and list(m['scores']) == KEYS
    assert seen['hyps'] == [W('a dog runs'), W('two cats'), W('a bus')]
    # cap 1 is scored against BOTH captions of image 7 of its subset (its own included), not against the train2014 image 7
    assert seen['refs'] == [[W('a dog runs'), W('a brown dog is running')], [W('two cats sleep')], [W('a train')]]
    direct = caption_scores_host(seen['hyps'], seen['refs'])
    assert all(m['scores'][k] == direct[k] for k in KEYS) and m['scores']['Cider'] > 0
    held = CocoCaptioning(samples, preds, None).evaluate('held_out_concepts')
    assert held['total'] == 1 and held['absent'] == 0 and held['scores']['Cider'] == 0.0          # one entry: every weight is 0
    # only the given samples supply references
    alone = CocoCaptioning(samples[:1], preds, None, scores=spy).evaluate()
    assert alone['total'] == 1 and seen['refs'] == [[W('a dog runs')]]
    # nothing predicted: zeros in the reference's layout
    empty = CocoCaptioning(samples, {}, None).evaluate()
    assert empty == {'absent': 4, 'total': 0, 'scores': {k: 0 for k in KEYS}}
    # a caller's tokenizer is used on both sides
    m2 = CocoCaptioning(samples, preds, None, tokenize=lambda s: list(s.replace(' ', '')), scores=spy).evaluate()
    assert seen['hyps'][2] == list('abus') and m2['total'] == 3


def test_simple_caption_tokenize():
    from gpv1_amd.evaluators import simple_caption_tokenize as tok, CAP_PUNCTUATION
    assert tok('A man, riding a WAVE on a surfboard.') == W('a man riding a wave on a surfboard')
    assert tok("  ``Hello'' -- said the cat ... ; really ?! ") == W('hello said the cat really')
    assert tok('a sign -LRB- red -RRB- : stop') == W('a sign red stop')
    assert tok('dog,cat;bird') == W('dog cat bird')
    assert tok("the dog's well-known trick -") == ["the", "dog's", 'well-known', 'trick']       # clitics and hyphens are NOT split
    assert tok("`quoted' words") == W('quoted words')
    assert tok('') == [] and tok(' . , ') == []
    for mark in CAP_PUNCTUATION:
        assert tok(f'a {mark} b') == ['a', 'b'] and tok(f'a{mark} b') == ['a', 'b'], mark


def test_caption_scorer_host_through_the_metric_loop_and_the_driver(shim, tmp_path, monkeypatch):
    from gpv1_amd import metrics
    from gpv1_amd import train_distr as td
    from gpv1_amd.caption_scorer import CaptionScorer
    from gpv1_amd.evaluators import CocoCaptioning
    model, _ = build_small()
    ds = _EvalSet(5)
    for i, s in enumerate(ds.samples):
        s['answer'] = ['w3 w5 w7', 'w3', 'w5 w7 w9 w11', 'w1 w3 w5', 'w7'][i]
        s['image'] = dict(s['image'], image_id=i // 2, subset='val2014')
    scores, preds = metrics.cap_metrics(model, td.eval_batches(ds, 2, 'cpu'), ds.samples, 4, scorer=CaptionScorer(host=True))
    assert list(scores) == KEYS and all(isinstance(v, float) and 0.0 <= v for v in scores.values()) and sorted(preds) == ['500', '501', '502', '503']
    assert scores == {k: float(v) for k, v in CocoCaptioning(ds.samples, preds, None).evaluate()['scores'].items()}
    # through the driver: training.caption_scorer='host' puts the Cider term into the sum, and the note about a missing scorer is gone
    monkeypatch.setitem(td.EVAL_FNS, 'coco_vqa', lambda m, b, d, limit: 0.25)
    seen = {}
    real = metrics.cap_metrics

    def spy(model, batches, samples, limit=None, scorer=None):
        out = real(model, batches, samples, limit, scorer=scorer)
        seen['scorer'], seen['scores'] = scorer, out[0]
        return out
    monkeypatch.setattr(metrics, 'cap_metrics', spy)
    logs = []
    cfg = _driver_cfg(tmp_path, caption_scorer='host')
    total = td.evaluate_subset(model, {'coco_vqa': ds, 'coco_cap': ds}, 'val', cfg, 0, 'cpu', logs.append)
    assert isinstance(seen['scorer'], CaptionScorer) and seen['scorer'].host
    assert total == 0.25 + seen['scores']['Cider'] and not any('no caption scorer' in l for l in logs)
    assert any('Cider: %s' % seen['scores']['Cider'] in l for l in logs)
    # the dataset's own scorer wins over the key; without either the old line and cider = 0 stay
    ds.scorer = lambda s, p: {'Cider': 0.5}
    assert td.evaluate_subset(model, {'coco_cap': ds}, 'val', cfg, 0, 'cpu', logs.append) == 0.5
    del ds.scorer
    logs2 = []
    assert td.evaluate_subset(model, {'coco_cap': ds}, 'val', _driver_cfg(tmp_path), 0, 'cpu', logs2.append) == 0
    assert sum('no caption scorer' in l for l in logs2) == 1
    with pytest.raises(ValueError, match='caption_scorer'):
        td.evaluate_subset(model, {'coco_cap': ds}, 'val', _driver_cfg(tmp_path, caption_scorer='gpu'), 0, 'cpu', logs2.append)
    from gpv1_amd.default_config import default_tree
    assert 'caption_scorer' not in default_tree()['training']


def test_cap_library_exports_exactly_the_declared_entry_points():
    """exports, header and nm: tests/test_abi_cpu.py, for every library; here what is the caption library's own"""
    import gpv1_amd.hip_cap as hip_cap
    from tests import abi_probe
    header, src = abi_probe.header_path('cap'), abi_probe.source('cap')
    # plain C: the header compiles as C99 on its own, and the mirror's limits are the header's
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', header], check=True)
    limits = dict(re.findall(r'#define\s+(GPV_CAP_\w+)\s+(\d+)', src))
    assert (int(limits['GPV_CAP_MAX_LEN']), int(limits['GPV_CAP_MAX_REFS']), int(limits['GPV_CAP_MAX_WORD']), int(limits['GPV_CAP_ORDERS'])) == \
        (hip_cap.MAX_LEN, hip_cap.MAX_REFS, hip_cap.MAX_WORD, hip_cap.ORDERS)
    assert hip_cap.MAX_LEN >= 64 and hip_cap.MAX_REFS >= 8
    assert {int(limits[k]) for k in limits if k.startswith('GPV_CAP_ERR_')} == set(hip_cap.ERR_BITS)


def test_mirror_and_scorer_refuse_what_the_device_cannot_take():
    import gpv1_amd.hip_cap as hip_cap
    from gpv1_amd.caption_scorer import CaptionScorer, caption_scores_device, encode_captions
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt)
    f = lambda n: torch.zeros(n, dtype=torch.float64)
    # no CPU path: host tensors are refused before anything is launched
    with pytest.raises(RuntimeError, match='GPU'):
        hip_cap.caption_scores(z(2, 5), z(2), z(2, 3, 6), z(2, 3), z(2), f(3), f(6))
    # over the limits: refused with the limit's name, whatever the device
    with pytest.raises(ValueError, match='GPV_CAP_MAX_LEN'):
        hip_cap.caption_scores(z(2, 65), z(2), z(2, 3, 6), z(2, 3), z(2), f(3), f(65))
    with pytest.raises(ValueError, match='GPV_CAP_MAX_LEN'):
        hip_cap.caption_scores(z(2, 5), z(2), z(2, 3, 65), z(2, 3), z(2), f(3), f(65))
    with pytest.raises(ValueError, match='GPV_CAP_MAX_REFS'):
        hip_cap.caption_scores(z(2, 5), z(2), z(2, 9, 6), z(2, 9), z(2), f(3), f(6))
    with pytest.raises(ValueError, match='pen'):
        hip_cap.caption_scores(z(2, 5), z(2), z(2, 3, 6), z(2, 3), z(2), f(3), f(5))
    with pytest.raises(RuntimeError, match='table is full'):
        hip_cap.check_error(1)
    hip_cap.check_error(0)
    assert [hip_cap.table_capacity(n) for n in (0, 1, 2, 3, 1000)] == [2, 2, 4, 8, 2048]
    # the scorer never truncates: a caption of 65 words, 9 references or 65536 distinct words raise
    words = [f'w{i}' for i in range(70000)]
    with pytest.raises(ValueError, match='65 words'):
        encode_captions([words[:65]], [[words[:3]]])
    with pytest.raises(ValueError, match='9 references'):
        encode_captions([words[:3]], [[words[:3]] * 9])
    with pytest.raises(ValueError, match='distinct words'):
        encode_captions([words[i * 64:(i + 1) * 64] for i in range(1025)], [[words[:3]]] * 1025)
    hyp, hyp_len, ref, ref_len, ref_count, occ = encode_captions([W('a b'), []], [[W('a b c'), W('b')], [W('c a b a b')]])
    assert hyp.tolist() == [[1, 2], [0, 0]] and hyp_len.tolist() == [2, 0] and ref_count.tolist() == [2, 1]
    assert ref.tolist() == [[[1, 2, 3, 0, 0], [2, 0, 0, 0, 0]], [[3, 1, 2, 1, 2], [0, 0, 0, 0, 0]]] and ref_len.tolist() == [[3, 1], [5, 0]]
    assert occ == (3 + 2 + 1) + 1 + (5 + 4 + 3 + 2) and all(a.dtype == np.int32 for a in (hyp, hyp_len, ref, ref_len, ref_count))
    if not torch.cuda.is_available():
        with pytest.raises(RuntimeError):                                   # no fallback to the host rule
            CaptionScorer()([{'cap_id': 1, 'answer': 'a b', 'image': {'image_id': 1}}], {'1': {'answer': 'a'}})
        with pytest.raises(RuntimeError, match='GPU'):
            caption_scores_device([W('a')], [[W('a')]], device='cpu')
