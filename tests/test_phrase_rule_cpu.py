"""The phrase set and the phrase-constrained beam rule on the host (gpv1_amd.phrases): the pinned trie numbering, the refusals, and
phrase_search_host against searches walked by hand."""
import numpy as np
import pytest

from gpv1_amd import beam
from gpv1_amd import phrases as P
from tests.phrase_cases import prefix_logits

F32 = np.float32
V = 24
PAD, STOP, CLS = V - 4, V - 2, V - 3
a, b, c, d, e = 3, 5, 8, 11, 13


def pset_of(phr):
    return P.PhraseSet(phr, V, PAD, STOP, CLS)


def walk(fn, bi, B, K, phrase_ids):
    """the score of one phrase followed by __stop__, walked alone: the same left-to-right fp32 adds as the rule"""
    tok = np.full((K, B, 1), CLS, np.int64)
    score = F32(0)
    for t, w in enumerate(list(phrase_ids) + [STOP]):
        x = np.asarray(fn(t, tok), dtype=F32)
        lse = beam.lse_host(x)
        score = F32(score + F32(x[bi, w] - lse[bi]))              # slot 0 of batch element bi is row 0*B + bi
        tok = np.concatenate((tok, np.full((K, B, 1), w, np.int64)), -1)
    return score


def test_trie_numbering_of_the_hand_written_example():
    s = pset_of([[a], [a, b], [c, d], [c, e]])
    assert (s.M, s.E, s.N, s.max_len) == (6, 5, 4, 2)
    assert s.child_off.tolist() == [0, 2, 3, 5, 5, 5, 5]
    assert s.child_tok.tolist() == [a, c, b, d, e]
    assert s.child_node.tolist() == [1, 2, 3, 4, 5]
    assert s.terminal.tolist() == [-1, 0, -1, 1, 2, 3]
    assert all(x.dtype == np.int32 for x in (s.child_off, s.child_tok, s.child_node, s.terminal))
    # the order of the phrases changes the phrase indices, not the numbering of the nodes
    s2 = pset_of([[c, e], [c, d], [a, b], [a]])
    assert s2.child_tok.tolist() == s.child_tok.tolist() and s2.child_node.tolist() == s.child_node.tolist()
    assert s2.terminal.tolist() == [-1, 3, -1, 2, 1, 0]
    assert s.digest != s2.digest and s.digest == pset_of([[a], [a, b], [c, d], [c, e]]).digest
    assert s.allowed(1) == [(b, 3, -1), (STOP, P.DONE, 0)] and s.allowed(0) == [(a, 1, -1), (c, 2, -1)]


def test_refusals():
    for bad, what in (([[a], [PAD]], 'pad_id'), ([[STOP, a]], 'stop_id'), ([[a, CLS]], 'cls_id'), ([[a], []], 'phrase 1 is empty'),
                      ([[a, b], [c], [a, b]], 'phrases 0 and 2 are equal'), ([[V]], 'outside the vocabulary'), ([[-1]], 'outside'), ([], 'at least one')):
        with pytest.raises(ValueError, match=what):
            pset_of(bad)
    s = pset_of([[a, b, c]])
    fn = prefix_logits(V, 1)
    for K, T in ((0, 6), (9, 6), (2, 1), (2, 65), (2, 4)):           # T = 4 leaves room for two tokens and __stop__
        with pytest.raises(ValueError):
            P.phrase_search_host(fn, 1, K, T, s)
    P.phrase_search_host(fn, 1, 2, 5, s)

    class Model:
        vocab = ['w%d' % i for i in range(V - 4)] + ['__pad__', '__cls__', '__stop__', '__unk__']
        word_to_idx = {w: i for i, w in enumerate(vocab)}
    t = P.PhraseSet.from_texts(Model, ['w1', 'w2 w3'])
    assert t.token_ids == [(1,), (2, 3)] and (t.pad_id, t.cls_id, t.stop_id, t.V) == (PAD, CLS, STOP, V)
    with pytest.raises(ValueError, match="'w2 zebra'.*'zebra'"):
        P.PhraseSet.from_texts(Model, ['w1', 'w2 zebra'])


@pytest.mark.parametrize('phr', [[[a], [a, b], [c, d], [c, e]], [[a, b, c], [a, b], [a], [e], [d, d], [d, a]], [[b]], [[a, a, a], [b, b]]])
@pytest.mark.parametrize('alpha', [0.0, 0.6])
def test_every_phrase_comes_back_ranked_as_walked_alone(phr, alpha):
    """K >= N: the search returns EVERY phrase, its score bit-equal to the phrase walked alone, in the order of the keys"""
    s = pset_of(phr)
    B, K, T = 2, 6, 6
    fn = prefix_logits(V, 11)
    o = P.phrase_search_host(fn, B, K, T, s, alpha=alpha)
    inv = beam.length_table(T, alpha) if alpha else None
    for bi in range(B):
        want = []
        for i, p in enumerate(phr):
            sc = walk(fn, bi, B, K, p)
            want.append((sc if inv is None else F32(sc * inv[len(p) + 1]), sc, i))
        want.sort(key=lambda w: -float(w[0]))
        n = len(phr)
        assert o['phrase'][bi, :n].tolist() == [w[2] for w in want]
        assert o['seq_lp'][bi, :n].view(np.uint32).tolist() == [int(w[1].view(np.uint32)) for w in want]
        assert o['keys'][bi, :n].view(np.uint32).tolist() == [int(F32(w[0]).view(np.uint32)) for w in want]
        assert (o['node'][bi, :n] == P.DONE).all() and (o['node'][bi, n:] == P.VOID).all()
        for k in range(n):
            p = list(phr[o['phrase'][bi, k]])
            assert o['seqs'][k, bi, :T - 1].tolist() == p + [STOP] + [PAD] * (T - 2 - len(p))
            assert o['length'][bi, k] == len(p) + 1
        # N < K: exactly K - N VOID slots at -1e9, in the last slots
        assert o['seq_lp'][bi, n:].view(np.uint32).tolist() == [int(F32(-1e9).view(np.uint32))] * (K - n)
        assert (o['phrase'][bi, n:] == -1).all() and (o['length'][bi, n:] == 0).all()


def test_beam_of_one_follows_the_greedy_path():
    phr = [[a, b, c], [a, b], [a], [e], [d, d], [d, a]]
    s = pset_of(phr)
    T = 6
    fn = prefix_logits(V, 5)
    for bi in range(2):
        n, tok, path = 0, np.full((1, 2, 1), CLS, np.int64), []
        for t in range(T - 1):
            x = fn(t, tok)[bi]
            w, n2, ph = max(s.allowed(n), key=lambda q: (float(x[q[0]]), -q[0]))
            path.append(w)
            tok = np.concatenate((tok, np.full((1, 2, 1), w, np.int64)), -1)
            if n2 == P.DONE:
                break
            n = n2
        o = P.phrase_search_host(fn, 2, 1, T, s)
        assert o['seqs'][0, bi, :len(path)].tolist() == path and path[-1] == STOP
        assert o['phrase'][bi, 0] == ph and tuple(path[:-1]) == s.token_ids[ph]


def logits_table(rows):
    """step_logits_fn from {prefix tuple (without __cls__): {token: logit}}; everything else -20"""
    def fn(t, tok):
        K, B, _ = tok.shape
        out = np.full((K * B, V), -20.0, np.float32)
        for k in range(K):
            for bb in range(B):
                for w, x in rows.get(tuple(int(v) for v in tok[k, bb, 1:]), {}).items():
                    out[k * B + bb, w] = x
        return out
    return fn


def test_a_prefix_phrase_and_its_extension_both_finish():
    s = pset_of([[a], [a, b]])
    o = P.phrase_search_host(logits_table({(): {a: 2.0}, (a,): {b: 1.0, STOP: 1.5}, (a, b): {STOP: 3.0}}), 1, 2, 5, s)
    assert o['phrase'][0].tolist() == [0, 1] and o['node'][0].tolist() == [P.DONE, P.DONE]
    assert o['seqs'][0, 0, :4].tolist() == [a, STOP, PAD, PAD] and o['seqs'][1, 0, :4].tolist() == [a, b, STOP, PAD]
    assert o['length'][0].tolist() == [2, 3]


def test_planted_ties_go_to_the_lower_token_and_the_lower_candidate():
    # one step, two allowed tokens with equal logits: the lower token is rank 0
    s = pset_of([[e], [b], [c]])
    x = np.full((2, V), -1.0, np.float32)
    x[:, [e, b]] = 4.0
    st = P.initial_state(1, 2, 4)
    o = P.phrase_step_host(x, beam.lse_host(x), st['seq_lp'], st['seqs'], st['node'], st['phrase'], st['length'], 0, PAD, STOP, s)
    assert o['tok'].tolist() == [b, e] and o['parent'][0].tolist() == [0, 0]
    assert o['node'][0].tolist() == [1, 3]                        # (children of the root in ascending token order: b, c, e)
    # two identical parents: equal keys go to the lower k1*K + k2 -- parent 0's two candidates before parent 1's
    s = pset_of([[a, b], [a, c], [a, d]])
    x = np.full((3, V), -1.0, np.float32)
    x[:, b], x[:, c], x[:, d] = 4.0, 3.0, 2.0
    st = P.initial_state(1, 3, 5)
    st['node'][0] = [1, 1, P.VOID]
    st['seq_lp'][0] = [-1.0, -1.0, P.VOID_LP]
    st['length'][0] = [1, 1, 0]
    st['seqs'][:2, 0, 0] = a
    o = P.phrase_step_host(x, beam.lse_host(x), st['seq_lp'], st['seqs'], st['node'], st['phrase'], st['length'], 1, PAD, STOP, s)
    assert o['parent'][0].tolist() == [0, 1, 0] and o['tok'].tolist() == [b, b, c]
    assert o['seq_lp'][0, 0] == o['seq_lp'][0, 1] > o['seq_lp'][0, 2]


def test_length_penalty_reorders_a_one_word_and_a_two_word_phrase():
    """Every row below is a normalised distribution up to the 22 fillers at -20 (their mass, 5e-8, moves no figure here), so lse = 0
    and lp = logit.  'a' __stop__: -2.0 + 0 = -2.0.  'c d' __stop__: log(1 - e^-2) - (2.1 + log(1 - e^-2)) + 0 = -2.1.  Without a
    penalty 'a' leads.  With alpha = 0.6 the keys are -2.0 * (7/6)^-0.6 = -2.0 * 0.911661 = -1.823322 for length 2 and
    -2.1 * (8/6)^-0.6 = -2.1 * 0.841466 = -1.767078 for length 3: 'c d' leads; the reported scores stay the raw ones."""
    s = pset_of([[a], [c, d]])
    q = float(np.log1p(-np.exp(-2.0)))                               # log P(c) = -0.145413
    lp_d = -2.1 - q                                                  # log P(d | c) = -1.954587
    rows = {(): {a: -2.0, c: q}, (a,): {STOP: 0.0}, (c,): {d: lp_d, e: float(np.log1p(-np.exp(lp_d)))}, (c, d): {STOP: 0.0}}
    fn = logits_table(rows)
    T = 6
    plain = P.phrase_search_host(fn, 1, 2, T, s)
    pen = P.phrase_search_host(fn, 1, 2, T, s, alpha=0.6)
    assert plain['phrase'][0].tolist() == [0, 1]
    assert abs(float(plain['seq_lp'][0, 0]) + 2.0) < 1e-5 and abs(float(plain['seq_lp'][0, 1]) + 2.1) < 1e-5
    assert pen['phrase'][0].tolist() == [1, 0] and pen['length'][0].tolist() == [3, 2]
    assert abs(float(pen['keys'][0, 0]) + 1.767078) < 1e-5 and abs(float(pen['keys'][0, 1]) + 1.823322) < 1e-5
    assert pen['seq_lp'][0].tolist() == plain['seq_lp'][0, ::-1].tolist()           # the reported score stays the raw one


def test_create_phrase_set_maps_phrases_to_classes():
    from gpv1_amd import compute_predictions as cp

    class Model:
        vocab = ['w%d' % i for i in range(V - 4)] + ['__pad__', '__cls__', '__stop__', '__unk__']
        word_to_idx = {w: i for i, w in enumerate(vocab)}
    classes = ('w2 w9', 'w6', 'w2')
    s, owner = cp.create_phrase_set(Model, classes)
    assert s.token_ids == [(2, 9), (6,), (2,)] and owner == [0, 1, 2] and s.max_len == 2
    s, owner = cp.create_phrase_set(Model, classes, synonyms={'w6': ['w6', 'w7 w7', 'w6'], 'w2': ['w2']}, use_syns=True)
    assert s.token_ids == [(6,), (7, 7), (2,)] and owner == [1, 1, 2]            # a class without an entry is left out, as in the mask
    with pytest.raises(ValueError, match="names both 'w6' and 'w2'"):
        cp.create_phrase_set(Model, classes, synonyms={'w6': ['w6', 'w2'], 'w2': ['w2']}, use_syns=True)
    with pytest.raises(ValueError, match="'hot dog'.*'hot'"):
        cp.create_phrase_set(Model, ('w1', 'hot dog'))
    assert len(cp.create_vocab_mask(Model, classes=('w1', 'hot dog'))[0]) == 3     # ...which the flat mask drops without a word
