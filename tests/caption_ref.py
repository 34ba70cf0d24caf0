"""Independent restatement (numpy) of the caption scoring rule -- TEST INFRASTRUCTURE, the checker only.

gpv1_amd.evaluators.caption_scores_host states the rule the way pycocoevalcap does: dicts keyed by tuples of words.  This file states
it again from the rule's text in another shape, so that a slip in one statement does not hide in the other: words become integers
(np.unique), an n-gram of order n becomes the integer sum_j id_j * base^(n-1-j), the n-grams of one entry become columns
(np.unique again) of a dense count matrix with one row per caption, and every sum is a numpy reduction over such a matrix.  Document
frequencies come from a sort-and-count (np.unique with counts) over the per-entry distinct codes.  No dict, no tuple, no Counter.
The two float64 tables are taken from evaluators.caption_tables: the rule says every side reads the SAME tables.

Also the generators of the random cases the CPU and GPU tests share.
"""
import math

import numpy as np

ORDERS = 4


def _word_ids(hyps, refs):
    """every word -> 1 + its rank among the distinct words"""
    flat = [w for h in hyps for w in h] + [w for rs in refs for r in rs for w in r]
    vocab = np.unique(np.asarray(flat)) if flat else np.asarray([])
    enc = lambda c: (np.searchsorted(vocab, np.asarray(c)) + 1).astype(np.int64) if len(c) else np.zeros(0, dtype=np.int64)
    return [enc(h) for h in hyps], [[enc(r) for r in rs] for rs in refs], len(vocab) + 1


def _codes(ids, n, base):
    """the integer of every window of n words"""
    m = len(ids) - n + 1
    if m <= 0:
        return np.zeros(0, dtype=np.int64)
    c = np.zeros(m, dtype=np.int64)
    for j in range(n):
        c = c * base + ids[j:j + m]
    return c


def scores(hyps, refs, R=None, LR=None):
    """-> {'testlen' [N], 'reflen' [N], 'guess' [N,4], 'correct' [N,4] int64, 'cider' [N] float64, 'ref_df' [N,R,4,LR] int64 (0 where no
    n-gram starts), 'Bleu1'..'Bleu4', 'Cider'}"""
    from gpv1_amd.evaluators import caption_tables
    N = len(hyps)
    H, Rf, base = _word_ids(hyps, refs)
    assert base ** ORDERS < 2 ** 62
    R = max(len(rs) for rs in refs) if R is None else R
    LR = max([len(r) for rs in refs for r in rs] + [1]) if LR is None else LR
    longest = max([len(h) for h in hyps] + [len(r) for rs in refs for r in rs] + [1])
    weight, pen = caption_tables(N, longest)
    # document frequencies: per order, the sorted distinct codes of the corpus and in how many entries each occurs
    df_keys, df_counts = [], []
    for n in range(1, ORDERS + 1):
        per_entry = [np.unique(np.concatenate([_codes(r, n, base) for r in rs])) for rs in Rf]
        k, c = np.unique(np.concatenate(per_entry), return_counts=True)
        df_keys.append(k)
        df_counts.append(c.astype(np.int64))

    def df_of(n, codes):
        k, c = df_keys[n - 1], df_counts[n - 1]
        if len(k) == 0:
            return np.zeros(len(codes), dtype=np.int64)
        at = np.minimum(np.searchsorted(k, codes), len(k) - 1)
        return np.where(k[at] == codes, c[at], 0)

    testlen = np.asarray([len(h) for h in H], dtype=np.int64)
    reflen = np.zeros(N, dtype=np.int64)
    guess = np.maximum(0, testlen[:, None] - np.arange(ORDERS)[None, :])
    correct = np.zeros((N, ORDERS), dtype=np.int64)
    cider = np.zeros(N, dtype=np.float64)
    ref_df = np.zeros((N, R, ORDERS, LR), dtype=np.int64)
    for i in range(N):
        lens = np.asarray([len(r) for r in Rf[i]], dtype=np.int64)
        gap = np.abs(lens - testlen[i])
        reflen[i] = lens[gap == gap.min()].min()
        bigrams_h = max(0, int(testlen[i]) - 1)
        acc = 0.0
        for n in range(1, ORDERS + 1):
            rows = [_codes(H[i], n, base)] + [_codes(r, n, base) for r in Rf[i]]
            for j, rc in enumerate(rows[1:]):
                ref_df[i, j, n - 1, :len(rc)] = df_of(n, rc)
            cols, inv = np.unique(np.concatenate(rows), return_inverse=True)
            if len(cols) == 0:
                continue
            M = np.zeros((len(rows), len(cols)), dtype=np.int64)
            row_of = np.concatenate([np.full(len(c), j, dtype=np.int64) for j, c in enumerate(rows)])
            np.add.at(M, (row_of, inv.reshape(-1)), 1)
            correct[i, n - 1] = np.minimum(M[0], M[1:].max(axis=0)).sum()
            vec = M.astype(np.float64) * weight[df_of(n, cols)][None, :]
            norm = np.sqrt((vec * vec).sum(axis=1))
            for j in range(1, len(rows)):
                val = (np.minimum(vec[0], vec[j]) * vec[j]).sum()
                if norm[0] != 0 and norm[j] != 0:
                    val = val / (norm[0] * norm[j])
                acc += val * pen[abs(bigrams_h - max(0, int(lens[j - 1]) - 1))]
        cider[i] = 10.0 * acc / ORDERS / len(Rf[i])
    out = {'testlen': testlen, 'reflen': reflen, 'guess': guess, 'correct': correct, 'cider': cider, 'ref_df': ref_df}
    b, tl, rl = 1.0, int(testlen.sum()), int(reflen.sum())
    brevity = (tl + 1e-15) / (rl + 1e-9)
    for k in range(ORDERS):
        b *= (int(correct[:, k].sum()) + 1e-15) / (int(guess[:, k].sum()) + 1e-9)
        out[f'Bleu{k + 1}'] = b ** (1.0 / (k + 1)) * (math.exp(1 - 1 / brevity) if brevity < 1 else 1.0)
    out['Cider'] = float(cider.mean()) if N else 0.0
    return out


def random_case(N, vocab, seed, hyp_lens=tuple(range(21)), ref_lens=tuple(range(65)), max_refs=8):
    """N entries of integer 'words' drawn from `vocab` (a sequence of ints): hypothesis lengths from hyp_lens, 1..max_refs references
    with lengths from ref_lens, uniformly.  -> (hyps, refs) as lists of lists of python ints"""
    rs = np.random.RandomState(seed)
    vocab = np.asarray(vocab)
    draw = lambda lens: [int(w) for w in vocab[rs.randint(0, len(vocab), size=lens[rs.randint(0, len(lens))])]]
    hyps = [draw(hyp_lens) for _ in range(N)]
    refs = [[draw(ref_lens) for _ in range(rs.randint(1, max_refs + 1))] for _ in range(N)]
    return hyps, refs


def edge_case(N, vocab, seed, lens=(0, 1, 2, 3, 4, 5, 20, 64), stranger=None):
    """random_case with lengths from `lens` on both sides, plus the situations the device scorer must get right, as far as N admits:
      every entry : reference 0 has at least 4 words and starts with the same 4 words (df = N: weight exactly 0)
      entry 0     : hypothesis = one of its references
      entry 1     : all references identical (they add 1 to a document frequency, not R)
      entry 2     : the hypothesis holds `stranger`, a word no reference holds (df 0), when one is given
      entry 3     : a tie in the closest reference length: hypothesis of 4 words, references of 5 and 3 (reflen 3)"""
    hyps, refs = random_case(N, vocab, seed, hyp_lens=lens, ref_lens=lens)
    rs = np.random.RandomState(seed + 1)
    vocab = [int(v) for v in vocab]
    common = [vocab[0], vocab[-1], vocab[len(vocab) // 2], vocab[0]]
    long_lens = [l for l in lens if l >= 4]
    for i in range(N):
        r0 = refs[i][0]
        if len(r0) < 4:
            r0 = [vocab[rs.randint(0, len(vocab))] for _ in range(long_lens[rs.randint(0, len(long_lens))])]
        refs[i][0] = common + r0[4:]
    hyps[0] = list(refs[0][rs.randint(0, len(refs[0]))])
    if N > 1:
        refs[1] = [list(refs[1][0]) for _ in range(max(2, len(refs[1])))]
    if N > 2 and stranger is not None:
        hyps[2] = (hyps[2] + [int(stranger), vocab[0], int(stranger)])[-20:]
    if N > 3:
        hyps[3] = [vocab[rs.randint(0, len(vocab))] for _ in range(4)]
        refs[3] = [common + [vocab[-1]], common[:3]]
    return hyps, refs
