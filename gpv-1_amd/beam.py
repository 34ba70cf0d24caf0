"""The beam search step, stated once on the host (numpy, fp32 arithmetic in a fixed order): the rule that csrc/beam_step.hip runs on the
device and that include/gpv_beam.h repeats word for word.

Step t (0 <= t < T-1), batch element b, parent k1 = 0..K-1, logits row r = k1*B + b:
 1. x_v = fp32(logit[r, v]) + vocab_mask[v]: one fp32 add; no add when the mask is absent.
 2. lse_r = m + logf(sum_v expf(x_v - m)), m = max_v x_v, fp32.  The summation order is the kernel's own; lse is an OUTPUT of the device
    step ([K*B] fp32) and an INPUT here, so no transcendental is evaluated on both sides and everything below is bit-exact.
 3. The row's candidates are its K largest x_v, ties to the lower v; k2 is the rank.  lp = x_v - lse_r: one fp32 subtract.
 4. score(k1,k2) = seq_lp[b,k1] + lp: one fp32 add.  t == 0 and k1 > 0: score = -1e9 exactly.  Mode FREEZE with finished[b,k1] set: the
    parent has exactly one candidate, k2 = 0, token pad_id, score = seq_lp[b,k1] unchanged; its other candidates do not exist.
 5. key = score * inv_pen[len']: one fp32 multiply, len' = length[b,k1] + (finished[b,k1] ? 0 : 1) (in either mode; clamped to 0 .. T,
    T the table's last entry).  inv_pen None: key = score.  inv_pen[n] = fp32(((5 + n) / 6) ** -alpha) (length_table).
 6. Selection: the first K of the candidates sorted by key descending, ties to the lower k1*K + k2 (a stable sort).  With only
    c < K candidates (gpv1_amd.phrases; never here) the slots c..K-1 take the caller's default: parent 0, its token and state.
 7. Slot k with the chosen (k1, k2, w): parent[b,k] = k1; seq_lp'[b,k] = score (raw, not the key); seqs'[k,b,:t] = seqs[k1,b,:t],
    seqs'[k,b,t] = w (positions behind t are left alone); tok[k*B+b] = w; length'[b,k] = len'; the search's own state, here
    finished'[b,k] = FREEZE ? (finished[b,k1] | (w == stop_id)) : 0.
Steps 5-7 are select_slots, shared with gpv1_amd.phrases (on the device: csrc/beam_core.h select_by_rank and write_slots).
Mode EXTEND without penalty and mask is the reference's search (exp/gpv/models/gpv.py:209-362: finished hypotheses keep extending, no
length normalisation); the only difference to GPV._beam_device's torch path is the last bit of lp (torch forms x - m - log s).
Caller conditions: 1 <= K <= MAX_K, K <= V, T <= MAX_T; a mask leaves at least K finite entries per row; a NaN logit gives an undefined
selection.

THE CONSTRAINTS (no_repeat, min_len, rep_neg / rep_pos; all zero: off, and the rule is the one above).  They add to steps 1-3;
steps 4-7 are unchanged.  h = seqs[k1, b, 0:t] is the history of the row's parent: the tokens written so far (__cls__ is not part
of it; special tokens in it count like any other token).  A frozen parent (mode FREEZE with finished[b,k1] set) is exempt from
everything below; it still has its single pad_id candidate.
 1b. Repetition penalty, on when rep_neg and rep_pos are non-zero, after the mask add: for every v that occurs in h,
     x_v = x_v < 0 ? x_v * rep_neg : x_v * rep_pos: one fp32 multiply, applied once however often v occurs.  rep_neg = fp32(theta),
     rep_pos = fp32(1 / theta), computed in float64 on the host (gpv1_amd.beam.rep_factors): a multiply, not a divide, so that host
     and device round the same way.  -inf stays -inf.
 2.  m and lse_r are taken over ALL v of the row as it stands after 1b, banned tokens included: bans do not renormalise.  The first
     pop is no longer the row maximum when the maximum is banned, so m has a reduction of its own.  The summation order is the
     one the header pins, unchanged.
 3a. The banned set of the row.  (i) n = no_repeat >= 1 and t >= n - 1: with p = h[t-n+1 : t] (n - 1 tokens, empty for n = 1),
     for every i in 0 .. t-n with h[i : i+n-1] == p the token h[i+n-1] is banned (at most t - n + 1 bans; t = 0 bans nothing).
     (ii) stop_id is banned while length[b,k1] < min_len: at least min_len tokens precede __stop__.
 3.  The row's candidates are its K largest x_v AMONG THE TOKENS THAT ARE NOT BANNED, ties to the lower v; lp = x_v - lse_r.
Caller condition with a constraint on: every row keeps at least K entries that are finite and not banned (a row bans fewer than T
tokens, so a mask that leaves K + T finite entries, or V >= K + T without one, suffices).  Below it the selection is undefined
(every index written stays inside its array; no loop bound depends on the data).  Extents: 0 <= no_repeat <= GPV_BEAM_MAX_NGRAM,
0 <= min_len <= T, rep_neg and rep_pos both zero or both finite and positive, and with any constraint on V <= GPV_BEAM_MAX_CONSTR_V
(a "seen" and a "banned" bitmap of V bits each in LDS, 16 KB together).
"""
import math

import numpy as np

EXTEND, FREEZE = 0, 1
MODES = {'extend': EXTEND, 'freeze': FREEZE}
MAX_K, MAX_T = 8, 64          # GPV_BEAM_MAX_K, GPV_BEAM_MAX_T
MAX_NGRAM, MAX_CONSTR_V = 8, 65536      # GPV_BEAM_MAX_NGRAM, GPV_BEAM_MAX_CONSTR_V
LANES = 256                   # GPV_BEAM_LANES
F32 = np.float32


def length_table(T, alpha):
    """inv_pen[n] = fp32(((5 + n) / 6) ** -alpha) for n = 0..T, computed in float64: the table both the host rule and the kernel read"""
    n = np.arange(T + 1, dtype=np.float64)
    return (((5.0 + n) / 6.0) ** (-float(alpha))).astype(np.float32)


def n_chain(V):
    """longest chain of dependent fp32 additions of the kernel's sum of exponentials (include/gpv_beam.h)"""
    return -(-int(V) // LANES) + 6 + 3


def check_extents(K, V, T, t=None):
    if not 1 <= K <= MAX_K:
        raise ValueError(f'beam: 1 <= beam size <= {MAX_K} is supported (GPV_BEAM_MAX_K), got {K}')
    if K > V:
        raise ValueError(f'beam: beam size {K} exceeds the vocabulary ({V})')
    if not 2 <= T <= MAX_T:
        raise ValueError(f'beam: 2 <= max_text_len <= {MAX_T} is supported (GPV_BEAM_MAX_T), got {T}')
    if t is not None and not 0 <= t < T - 1:
        raise ValueError(f'beam: step {t} outside 0 .. {T - 2}')


def rep_factors(theta):
    """(rep_neg, rep_pos) = (fp32(theta), fp32(1 / theta)) of step 1b, computed in float64; None for theta None or 1.0 (off)"""
    if theta is None or float(theta) == 1.0:
        return None
    theta = float(theta)
    if not (math.isfinite(theta) and theta > 0.0):
        raise ValueError(f'beam: the repetition penalty must be finite and positive, got {theta!r}')
    return F32(theta), F32(1.0 / theta)


def banned_tokens(history, n):
    """step 3a (i): the tokens that would complete an n-gram the history already holds -> a set (empty for n < 1 or len(history) < n - 1)"""
    h = [int(w) for w in history]
    t = len(h)
    if n < 1 or t < n - 1:
        return set()
    p = h[t - n + 1:t]
    return {h[i + n - 1] for i in range(t - n + 1) if h[i:i + n - 1] == p}


def check_constraints(V, T, no_repeat_ngram=0, min_length=0, repetition=None):
    """the extents of the constraints -> True when one of them is on"""
    n, m = int(no_repeat_ngram), int(min_length)
    if not 0 <= n <= MAX_NGRAM:
        raise ValueError(f'beam: 0 <= no_repeat_ngram <= {MAX_NGRAM} is supported (GPV_BEAM_MAX_NGRAM), got {no_repeat_ngram}')
    if not 0 <= m <= T:
        raise ValueError(f'beam: 0 <= min_length <= max_text_len = {T}, got {min_length}')
    if repetition is not None:
        neg, pos = (float(r) for r in repetition)
        if not (math.isfinite(neg) and math.isfinite(pos) and neg > 0.0 and pos > 0.0):
            raise ValueError(f'beam: repetition must be a pair of finite positive factors (rep_factors) or None, got {repetition!r}')
    on = n > 0 or m > 0 or repetition is not None
    if on and V > MAX_CONSTR_V:
        raise ValueError(f'beam: a constrained search supports a vocabulary of at most {MAX_CONSTR_V} (GPV_BEAM_MAX_CONSTR_V), got {V}')
    return on


def penalised_rows(x, seqs, finished, t, mode, repetition):
    """step 1b on the masked rows x [K*B, V] fp32 -> a new array: every token of a live parent's history multiplied once"""
    x = np.array(x, dtype=F32)
    if repetition is None:
        return x
    K, B, _ = seqs.shape
    neg, pos = F32(repetition[0]), F32(repetition[1])
    for k1 in range(K):
        for b in range(B):
            if mode == FREEZE and finished[b, k1]:
                continue
            v = np.unique(np.asarray(seqs[k1, b, :t], dtype=np.int64))
            xv = x[k1 * B + b, v]
            x[k1 * B + b, v] = np.where(xv < 0, xv * neg, xv * pos)                # one fp32 multiply each
    return x


def select_slots(out, b, cands, seqs, t, inv_pen=None, default=None):
    """Steps 5-7 for batch element b.  cands: the candidates in k1*K + k2 order, each a dict of k1, w and what the slot takes under
    the names of `out`: seq_lp (the score), length (len') and the search's own state words.  default: the candidate (k1 = 0) that the
    slots behind the last candidate take.  Writes out[...][b, k], out['seqs'][k, b] and out['tok'][k*B + b]."""
    K, B, T = seqs.shape

    def key(c):
        pen = None if inv_pen is None else F32(inv_pen[min(max(int(c['length']), 0), T)])
        return c['seq_lp'] if pen is None else F32(c['seq_lp'] * pen)            # one fp32 multiply
    chosen = sorted(cands, key=lambda c: -float(key(c)))[:K]                     # stable; float(fp32) is exact, so is its negation
    for k, c in enumerate(chosen + [default] * (K - len(chosen))):
        out['parent'][b, k] = c['k1']
        out['seqs'][k, b, :t] = seqs[c['k1'], b, :t]
        out['seqs'][k, b, t] = c['w']
        out['tok'][k * B + b] = c['w']
        for name, v in c.items():
            if name not in ('k1', 'w'):
                out[name][b, k] = v


def beam_step_host(logits, lse, seq_lp, seqs, finished, length, t, mode, pad_id, stop_id, inv_pen=None, vocab_mask=None,
                   no_repeat_ngram=0, min_length=0, repetition=None):
    """One step.  logits [K*B, V] (values exactly representable in fp32: fp32 or widened bf16), lse [K*B] fp32 (the device's, or any
    log-sum-exp of the rows as they stand after steps 1 and 1b), seq_lp [B,K] fp32, seqs [K,B,T] int64, finished [B,K] 0/1, length [B,K]
    int; the constraints: no_repeat_ngram (n), min_length, repetition (the (rep_neg, rep_pos) pair of rep_factors or None).  Nothing is
    modified.
    -> dict(parent [B,K] int32, tok [K*B] int64, seqs [K,B,T] int64, seq_lp [B,K] fp32, finished [B,K] int32, length [B,K] int32)"""
    x = np.asarray(logits, dtype=F32)
    K, B, T = seqs.shape
    V = x.shape[1]
    check_extents(K, V, T, t)
    if x.shape[0] != K * B:
        raise ValueError(f'beam: logits must have K*B = {K * B} rows, got {x.shape[0]}')
    if mode not in (EXTEND, FREEZE):
        raise ValueError(f'beam: mode must be EXTEND or FREEZE, got {mode!r}')
    if vocab_mask is not None:
        x = x + np.asarray(vocab_mask, dtype=F32)[None, :]                       # step 1
    constrained = check_constraints(V, T, no_repeat_ngram, min_length, repetition)
    if repetition is not None:
        x = penalised_rows(x, seqs, finished, t, mode, repetition)               # step 1b
    lse = np.asarray(lse, dtype=F32)
    seq_lp = np.asarray(seq_lp, dtype=F32)
    order = np.argsort(-x, axis=1, kind='stable')                                # step 3: K largest, ties to the lower v
    if constrained:                                                              # step 3a: ... among the tokens that are not banned
        order = [_without_banned(order[k1 * B + b], K, seqs[k1, b, :t], no_repeat_ngram, stop_id if length[b, k1] < min_length else None,
                                 mode == FREEZE and bool(finished[b, k1])) for k1 in range(K) for b in range(B)]
    else:
        order = order[:, :K]
    out = {'parent': np.zeros((B, K), np.int32), 'tok': np.zeros(K * B, np.int64), 'seqs': np.array(seqs, dtype=np.int64),
           'seq_lp': np.zeros((B, K), F32), 'finished': np.zeros((B, K), np.int32), 'length': np.zeros((B, K), np.int32)}
    for b in range(B):
        cands = []                                                               # in k1*K + k2 order
        for k1 in range(K):
            r = k1 * B + b
            fin = bool(finished[b, k1])
            ln = int(length[b, k1]) + (0 if fin else 1)
            for k2 in range(K):
                if mode == FREEZE and fin:
                    if k2 > 0:
                        continue
                    w, score = pad_id, seq_lp[b, k1]
                else:
                    w = int(order[r][k2])
                    lp = F32(x[r, w] - lse[r])                                   # one fp32 subtract
                    score = F32(seq_lp[b, k1] + lp)                              # one fp32 add
                    if t == 0 and k1 > 0:
                        score = F32(-1e9)
                cands.append({'k1': k1, 'w': w, 'seq_lp': score, 'length': ln,
                              'finished': int(mode == FREEZE and (fin or w == stop_id))})
        select_slots(out, b, cands, seqs, t, inv_pen)                            # steps 5-7
    return out


def _without_banned(order, K, history, n, stop_banned, frozen):
    """the first K tokens of a row's order that step 3a does not ban (a frozen parent is exempt: its row is not read anyway)"""
    if frozen:
        return order[:K]
    banned = banned_tokens(history, n)
    if stop_banned is not None:
        banned.add(int(stop_banned))
    return [int(v) for v in order if int(v) not in banned][:K]


def lse_host(logits, vocab_mask=None):
    """a log-sum-exp of the masked rows for beam_search_host when no device is at hand: m + log(sum exp(x - m)) in float64, rounded to
    fp32 (the device's own differs by its summation order, within the bound of tests/test_beam_gpu.py)"""
    x = np.asarray(logits, dtype=F32)
    if vocab_mask is not None:
        x = x + np.asarray(vocab_mask, dtype=F32)[None, :]
    m = x.max(axis=1).astype(np.float64)
    return (m + np.log(np.exp(x.astype(np.float64) - m[:, None]).sum(axis=1))).astype(F32)


def beam_search_host(step_logits_fn, B, K, T, cls_id, pad_id, stop_id, mode=EXTEND, alpha=0.0, vocab_mask=None,
                     no_repeat_ngram=0, min_length=0, repetition=None):
    """The chained search: step_logits_fn(t, tok [K,B,t+1] int64) -> logits [K*B, V] of the newest position (row k*B + b continues the
    hypothesis in slot k of batch element b; tok[:, :, 0] = cls_id).  -> dict(seqs [K,B,T], seq_lp [B,K], finished, length, keys [B,K])"""
    inv_pen = length_table(T, alpha) if alpha else None
    constr = dict(no_repeat_ngram=no_repeat_ngram, min_length=min_length, repetition=repetition)
    seqs = np.zeros((K, B, T), np.int64)
    seq_lp = np.zeros((B, K), F32)
    finished = np.zeros((B, K), np.int32)
    length = np.zeros((B, K), np.int32)
    tok = np.full((K, B, 1), cls_id, np.int64)
    bi = np.arange(B)
    for t in range(T - 1):
        logits = np.asarray(step_logits_fn(t, tok), dtype=F32)
        if repetition is None:
            lse = lse_host(logits, vocab_mask)
        else:                                                                     # (the lse of the rows as they stand after step 1b)
            masked = logits if vocab_mask is None else logits + np.asarray(vocab_mask, dtype=F32)[None, :]
            lse = lse_host(penalised_rows(masked, seqs, finished, t, mode, repetition))
        o = beam_step_host(logits, lse, seq_lp, seqs, finished, length, t, mode, pad_id, stop_id,
                           inv_pen=inv_pen, vocab_mask=vocab_mask, **constr)
        par = o['parent'].T                                                       # [K,B]
        tok = np.concatenate((tok[par, bi[None, :]], o['tok'].reshape(K, B, 1)), axis=-1)
        seqs, seq_lp, finished, length = o['seqs'], o['seq_lp'], o['finished'], o['length']
    keys = seq_lp if inv_pen is None else (seq_lp * inv_pen[np.clip(length, 0, T)]).astype(F32)
    return {'seqs': seqs, 'seq_lp': seq_lp, 'finished': finished, 'length': length, 'keys': keys}
