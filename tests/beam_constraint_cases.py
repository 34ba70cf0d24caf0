"""TEST-ONLY inputs of one CONSTRAINED beam step (no repeated n-gram, minimum length, repetition penalty), shared by
tests/test_beam_constraints_rule_cpu.py and tests/test_beam_constraints_gpu.py: beam_cases.make_case with the history redrawn from a
three-token alphabet (uniform draws from V almost never repeat, these repeat n-grams and ban one token several times), the alphabet
taken among word and lane boundaries of the kernel's bitmaps and loads, and the planted situations the constrained rule has to get
right."""
import numpy as np
import torch

from tests.beam_cases import make_case

PLANTS = ('ban_max', 'ban_tie', 'stop_top', 'seen_both_signs')
BOUNDARY = (31, 32, 255, 256)            # last / first bit of a bitmap word, last / first lane of the strided loads (and V - 1)


def banned_of(case, r, n, min_len, mode):
    """the banned set of row r = k1*B + b by the rule (empty for a frozen parent)"""
    from gpv1_amd import beam as rule
    K, B, _ = case['seqs'].shape
    k1, b = r // B, r % B
    if mode == rule.FREEZE and case['finished'][b, k1]:
        return set()
    banned = rule.banned_tokens(case['seqs'][k1, b, :case['t']], n)
    if case['length'][b, k1] < min_len:
        banned.add(case['stop_id'])
    return banned


def make_constrained_case(seed, B, K, V, T, t, dtype=torch.float32, plants=(), masked=False, penalty=None, n=0, min_len=0, theta=None,
                          mode=0, base_plants=()):
    """make_case(seed, ..., plants=base_plants, penalty=penalty) plus: seqs[:, :, :t] from a three-token alphabet; masked: a mask that
    leaves K + T + 4 finite entries (the alphabet, pad and stop among them; the rule's caller condition wants K + T); the PLANTS.
    -> the case dict with 'constr' = the keywords of beam_step_host / hip_beam.step and 'alphabet'"""
    from gpv1_amd import beam as rule
    case = make_case(seed, B, K, V, T, t, dtype, plants=base_plants, masked=False, penalty=penalty)
    rs = np.random.RandomState(seed + 7919)
    logits = case['logits']
    pool = sorted({v for v in BOUNDARY + (V - 1,) if 0 <= v < V} | set(rs.choice(V, 3, replace=False).tolist()))
    alphabet = rs.choice(pool, 3, replace=False)
    case['seqs'][:, :, :t] = alphabet[rs.randint(0, 3, (K, B, t))]
    case['alphabet'] = alphabet
    repetition = rule.rep_factors(theta)
    seen_of = lambda r: sorted(set(case['seqs'][r // B, r % B, :t].tolist()))
    rows = rs.permutation(K * B)
    if 'seen_both_signs' in plants:                         # seen tokens with positive, negative, zero and -inf values (every row; the
        cycle = [2.5, -1.5, 0.0, -np.inf]                   # cycle starts at another value per row)
        for r in range(K * B):
            for i, v in enumerate(seen_of(r)):
                logits[r, v] = cycle[(r + i) % 4]
    if 'stop_top' in plants:                                # __stop__ as a row's top-1 (banned while length < min_len)
        r = int(rows[0])
        logits[r, case['stop_id']] = logits[r][torch.isfinite(logits[r])].max() + 2
    if 'ban_tie' in plants:                                 # a banned token equals an allowed token of higher index in value, at the top
        for r in rows:                                      # (with the penalty on both are seen or both unseen: equal after 1b as well)
            banned, seen = banned_of(case, int(r), n, min_len, mode), set(seen_of(int(r)))
            live = not (mode == rule.FREEZE and case['finished'][r % B, r // B])
            pairs = [(w, u) for w in sorted(banned) for u in range(w + 1, V)
                     if u not in banned and (repetition is None or not live or (w in seen) == (u in seen))]
            if pairs:
                w, u = pairs[rs.randint(len(pairs))]
                logits[r, w] = logits[r, u] = logits[r][torch.isfinite(logits[r])].max() + 1
                break
    if 'ban_max' in plants:                                 # the row maximum is a banned token, 100 above the rest: expf overflows
        for r in rows[::-1]:                                # unless m is the true maximum
            banned = banned_of(case, int(r), n, min_len, mode)
            if banned:
                w = sorted(banned)[rs.randint(len(banned))]
                logits[r, w] = logits[r][torch.isfinite(logits[r])].max() + 100
                break
    if masked:
        keep = set(alphabet.tolist()) | {case['pad_id'], case['stop_id']}
        rest = [v for v in rs.permutation(V).tolist() if v not in keep]
        keep = sorted(keep | set(rest[:max(K + T + 4 - len(keep), 0)]))
        vm = np.full(V, -np.inf, np.float32)
        vm[keep] = (rs.rand(len(keep)) < 0.5).astype(np.float32) * -0.5
        case['vocab_mask'] = vm
    case['x'] = logits.float().numpy().copy()
    case['constr'] = dict(no_repeat_ngram=n, min_length=min_len, repetition=repetition)
    return case
