"""The device caption scorer (csrc/caption_score.hip through gpv1_amd.hip_cap / gpv1_amd.caption_scorer) against the host rule
(gpv1_amd.evaluators.caption_scores_host) and against the independent restatement (tests/caption_ref.py) -- never against itself.

Bounds, none of them taken from what the kernel gives:
  * testlen, reflen, guess, correct and the document frequency at every reference position: equal as integers, no case left out;
  * per-entry CIDEr: 1e-12 -- both sides are float64 on the same two tables, float64 square root and division are correctly rounded,
    so only the order of summation differs: at most 64 non-negative terms per sum (7e-15 of its value), a handful of such sums behind
    a score of at most 10;
  * the final dict: 1e-12 on each value (Bleu comes from equal integers through the same host arithmetic);
  * two calls: bit-identical outputs."""
import numpy as np
import pytest
import torch

from tests import caption_ref, synth
from tests.test_model_cpu import build_small, V, H, W, Tl

pytestmark = pytest.mark.gpu
DEV = 'cuda'
KEYS = ['Bleu1', 'Bleu2', 'Bleu3', 'Bleu4', 'Cider']
# vocabulary (word = its id on the device) and a word outside it for the hypothesis no reference holds
VOCABS = {'three': ([1, 2, 3], 4), 'fifty': (list(range(1, 51)), 51), 'top': (list(range(65535 - 49, 65536)), 65535 - 50)}
SIZES = [1, 2, 3, 64, 257]


def pack(hyps, refs):
    """integer words as they are -> the scorer's arrays (R, LH, LR: the largest present, at least 1)"""
    N = len(hyps)
    R = max(len(rs) for rs in refs)
    LH = max([len(h) for h in hyps] + [1])
    LR = max([len(r) for rs in refs for r in rs] + [1])
    hyp, hyp_len = np.zeros((N, LH), np.int32), np.zeros(N, np.int32)
    ref, ref_len, ref_count = np.zeros((N, R, LR), np.int32), np.zeros((N, R), np.int32), np.zeros(N, np.int32)
    for i in range(N):
        hyp[i, :len(hyps[i])], hyp_len[i], ref_count[i] = hyps[i], len(hyps[i]), len(refs[i])
        for j, r in enumerate(refs[i]):
            ref[i, j, :len(r)], ref_len[i, j] = r, len(r)
    return hyp, hyp_len, ref, ref_len, ref_count


def run_kernel(hyps, refs, occurrences=None):
    from gpv1_amd import hip_cap
    from gpv1_amd.evaluators import caption_tables
    arrays = pack(hyps, refs)
    N, LH = arrays[0].shape
    LR = arrays[2].shape[2]
    weight, pen = caption_tables(N, max(LH, LR))
    dev = [torch.from_numpy(a).to(DEV) for a in arrays + (weight, pen)]
    out = hip_cap.caption_scores(*dev, occurrences=occurrences, ref_df=True)
    torch.cuda.synchronize()
    names = ('testlen', 'reflen', 'guess', 'correct', 'cider', 'err', 'ref_df')
    return {k: v.cpu().numpy() for k, v in zip(names, out)}


_CASES = {}


def case(vocab, N):
    """(hyps, refs, host rule, restatement) of a vocabulary and a size: computed once, shared, never modified"""
    from gpv1_amd.evaluators import caption_scores_host
    if (vocab, N) not in _CASES:
        words, stranger = VOCABS[vocab]
        hyps, refs = caption_ref.edge_case(N, words, seed=100 * N + len(words), stranger=stranger)
        _CASES[vocab, N] = (hyps, refs, caption_scores_host(hyps, refs), caption_ref.scores(hyps, refs))
    return _CASES[vocab, N]


def df_array(refs, df, shape):
    """the host rule's {n-gram: df} laid out like the kernel's ref_df"""
    out = np.zeros(shape, dtype=np.int64)
    for i, rs in enumerate(refs):
        for j, r in enumerate(rs):
            for n in range(1, 5):
                for p in range(len(r) - n + 1):
                    out[i, j, n - 1, p] = df[tuple(r[p:p + n])]
    return out


def check(got, hyps, refs, host, ref):
    assert got['err'].tolist() == [0]
    for k in ('testlen', 'reflen', 'guess', 'correct'):
        assert np.array_equal(got[k], host['bleu_entries'][k]), (k, 'host rule')
        assert np.array_equal(got[k], ref[k]), (k, 'restatement')
    assert got['ref_df'].shape == ref['ref_df'].shape
    assert np.array_equal(got['ref_df'], ref['ref_df']), 'ref_df: restatement'
    assert np.array_equal(got['ref_df'], df_array(refs, host['df'], got['ref_df'].shape)), 'ref_df: host rule'
    assert got['cider'].dtype == np.float64
    worst_h = float(np.abs(got['cider'] - host['cider_entries']).max())
    worst_r = float(np.abs(got['cider'] - ref['cider']).max())
    print('N %d   Cider %.6f   entries %.4f .. %.4f   worst |device - host| %.3e   |device - restatement| %.3e   correct %s' %
          (len(hyps), host['Cider'], host['cider_entries'].min(), host['cider_entries'].max(), worst_h, worst_r, host['bleu_totals']['correct']))
    assert worst_h <= 1e-12 and worst_r <= 1e-12


@pytest.mark.parametrize('N', SIZES)
@pytest.mark.parametrize('vocab', list(VOCABS))
def test_kernel_equals_the_host_rule_and_the_restatement(vocab, N):
    hyps, refs, host, ref = case(vocab, N)
    check(run_kernel(hyps, refs), hyps, refs, host, ref)


def test_the_cases_hold_what_they_are_meant_to():
    """the situations of caption_ref.edge_case are really in the inputs (checked on the host side: nothing here runs the kernel)"""
    for vocab in VOCABS:
        words, stranger = VOCABS[vocab]
        hyps, refs, host, ref = case(vocab, 257)
        N = 257
        assert {len(rs) for rs in refs} == set(range(1, 9))                                  # ragged R
        assert {len(r) for rs in refs for r in rs} == {0, 1, 2, 3, 4, 5, 20, 64}
        assert {len(h) for h in hyps} >= {0, 1, 2, 3, 4, 5, 20, 64}
        common = tuple(refs[0][0][:4])
        assert host['df'][common] == N and host['df'][common[:1]] == N                    # in every entry: weight exactly 0
        assert hyps[0] in refs[0]                                                          # hypothesis = a reference
        assert len(refs[1]) >= 2 and all(r == refs[1][0] for r in refs[1])                # identical references
        assert stranger in hyps[2] and (stranger,) not in host['df']                       # df 0
        assert len(hyps[3]) == 4 and [len(r) for r in refs[3]] == [5, 3] and host['bleu_entries']['reflen'][3] == 3   # the tie
        assert host['cider_entries'].max() > (1 if vocab != 'three' else 0) and host['bleu_totals']['correct'][3] > 0
    assert max(w for h in case('top', 64)[0] for w in h) == 65535


def test_small_sizes_hold_the_tie_and_the_hand_cases():
    """N = 2: the closed forms of the CPU test and the tie in the closest reference length, on the device"""
    a, b, c, d, e, f, g, h = range(65528, 65536)
    got = run_kernel([[a, b, c, d], [e, f, g, h]], [[[a, b, c, d]], [[e, f, g, h]]])
    assert np.abs(got['cider'] - 10.0).max() < 1e-12 and got['correct'].tolist() == [[4, 3, 2, 1]] * 2 and got['err'].tolist() == [0]
    got = run_kernel([[a, b, c, d, e], [e, f, g, h]], [[[a, b, c, d]], [[e, f, g, h]]])
    want = 10 * np.exp(-1 / 72) * (2 / np.sqrt(5) + np.sqrt(3) / 2 + 2 / np.sqrt(6) + 1 / np.sqrt(2)) / 4
    assert abs(got['cider'][0] - want) < 1e-12 and abs(got['cider'][1] - 10.0) < 1e-12
    got = run_kernel([[a, b, c, d, e], [a] * 7], [[[a, b, c, d, e, f], [a, b, c, d]], [[a, b, c, a, d, a], [e, a, b, f, g, a, h]]])
    assert got['reflen'].tolist() == [4, 7] and got['testlen'].tolist() == [5, 7] and got['guess'].tolist() == [[5, 4, 3, 2], [7, 6, 5, 4]]
    assert got['correct'].tolist() == [[5, 4, 3, 2], [3, 0, 0, 0]]                       # clipped at the most one reference holds
    got = run_kernel([[a, b]], [[[a, b]]])                                                # N = 1: every weight is 0
    assert got['cider'].tolist() == [0.0] and got['ref_df'][0, 0, :, :2].tolist() == [[1, 1], [1, 0], [0, 0], [0, 0]]


def test_two_calls_give_the_same_bits_and_a_small_table_is_reported():
    from gpv1_amd import hip_cap
    hyps, refs, _, _ = case('fifty', 257)
    first, second = run_kernel(hyps, refs), run_kernel(hyps, refs)
    for k in first:
        assert first[k].tobytes() == second[k].tobytes(), k
    # the exact number of occurrences sizes the table as the scorer does it: same results as with the bound of the shape
    occ = sum(max(0, len(r) - n) for rs in refs for r in rs for n in range(4))
    exact = run_kernel(hyps, refs, occurrences=occ)
    for k in first:
        assert first[k].tobytes() == exact[k].tobytes(), k
    # a table too small for the references: the call completes (every probe loop is bounded by the capacity) and says so
    small = run_kernel(hyps, refs, occurrences=16)
    assert small['err'][0] & 1
    with pytest.raises(RuntimeError, match='table is full'):
        hip_cap.check_error(small['err'][0])
    # a word id outside 1..65535 inside a caption's length is reported, not scored
    bad = run_kernel([[1, 70000, 2]], [[[1, 2]]])
    assert bad['err'][0] & 2
    bad = run_kernel([[1, 2]], [[[1, 0, 2]]])
    assert bad['err'][0] & 2


def as_samples(hyps, refs):
    """entries -> caption samples (one image per entry, one sample per reference) and the predictions of their first cap_id"""
    samples, preds = [], {}
    text = lambda ws: ' '.join(f'w{w}' for w in ws)
    for i, (h, rs) in enumerate(zip(hyps, refs)):
        for j, r in enumerate(rs):
            samples.append({'cap_id': 10 * i + j, 'answer': text(r).upper() if i % 2 else text(r), 'image': {'image_id': i, 'subset': 'val2014'}})
        preds[str(10 * i)] = {'answer': text(h) + (' .' if i % 3 == 0 else '')}
    return samples, preds


@pytest.mark.parametrize('vocab,N', [('three', 64), ('fifty', 257), ('fifty', 1)])
def test_caption_scorer_device_equals_host(vocab, N):
    from gpv1_amd.caption_scorer import CaptionScorer
    hyps, refs, host, _ = case(vocab, N)
    samples, preds = as_samples(hyps, refs)
    dev, cpu = CaptionScorer(), CaptionScorer(host=True)
    got, want = dev(samples, preds), cpu(samples, preds)
    print(got, want)
    assert list(got) == KEYS == list(want) and all(isinstance(v, float) for v in got.values())
    for k in KEYS:
        assert abs(got[k] - want[k]) <= 1e-12, k
        assert abs(want[k] - host[k]) <= 1e-12, k                    # the pairing hands the scorer the entries the case was built from
    assert dev(samples, preds) == got                                # twice: the same bits
    full = dev.evaluate(samples, preds)
    assert full['total'] == N and full['absent'] == len(samples) - N
    assert dev(samples, {}) == {k: 0.0 for k in KEYS}


def test_cap_metrics_with_the_device_scorer_on_the_small_model(monkeypatch):
    """metrics.cap_metrics(..., scorer=CaptionScorer()) end to end, against the host scorer on the same predictions"""
    import gpv1_amd.hip as hip
    import gpv1_amd.ops as ops
    from gpv1_amd import metrics
    from gpv1_amd import train_distr as td
    from gpv1_amd.caption_scorer import CaptionScorer
    from gpv1_amd.train_distr import SyntheticCocoDataset
    hip.lib()
    ops.RT.set_precise(True)
    try:
        model, _ = build_small()
        model.to(DEV).eval()
        n = 7

        class Set:
            items = SyntheticCocoDataset(n, synth.make_vocab(V), image_size=(H, W), query_len=Tl, seed=5, tasks=('CocoCaptioning',))
            samples = [{'cap_id': 500 + i, 'answer': 'w3 w5', 'image': {'image_id': i // 2, 'subset': 'val2014'}} for i in range(n)]

            def __len__(self):
                return n

            def __getitem__(self, i):
                return self.items[i]
        ds = Set()
        batches = lambda: td.eval_batches(ds, 3, DEV)
        _, first = metrics.cap_metrics(model, batches(), ds.samples, None)
        # references cut from the predictions themselves (a random model says nothing a fixed caption holds): the answer without its
        # last word, and the next sample's answer
        said = [first[str(s['cap_id'])]['answer'].split() or ['w3'] for s in ds.samples]
        for i, s in enumerate(ds.samples):
            s['answer'] = ' '.join((said[i][:-1] or said[i]) if i % 2 else said[(i + 1) % n]).upper()
        scores, preds = metrics.cap_metrics(model, batches(), ds.samples, 6, scorer=CaptionScorer())
        want = CaptionScorer(host=True)(ds.samples, preds)
        print(scores, want)
        assert sorted(preds) == [str(500 + i) for i in range(6)] and list(scores) == KEYS
        for k in KEYS:
            assert abs(scores[k] - want[k]) <= 1e-12, k
        assert scores['Cider'] > 0 and scores['Bleu1'] > 0
        # and through the driver: training.caption_scorer='device'
        from gpv1_amd.config import from_dict
        cfg = from_dict({'batch_size': 3, 'training': {'batch_size': 3, 'num_val_samples': {'coco_cap': 6}, 'caption_scorer': 'device'}})
        logs, seen = [], {}
        real = metrics.cap_metrics

        def spy(model, batches_, samples, limit=None, scorer=None):
            out = real(model, batches_, samples, limit, scorer=scorer)
            seen['scorer'], seen['preds'] = scorer, out[1]
            return out
        monkeypatch.setattr(metrics, 'cap_metrics', spy)
        total = td.evaluate_subset(model, {'coco_cap': ds}, 'val', cfg, 0, DEV, logs.append)
        assert isinstance(seen['scorer'], CaptionScorer) and not seen['scorer'].host and sorted(seen['preds']) == sorted(preds)
        assert abs(total - CaptionScorer(host=True)(ds.samples, seen['preds'])['Cider']) <= 1e-12
        assert not any('no caption scorer' in l for l in logs) and any('Cider' in l for l in logs)
    finally:
        ops.RT.set_precise(False)
