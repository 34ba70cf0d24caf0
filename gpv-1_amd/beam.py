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

THE SAMPLER (mode GPV_BEAM_SAMPLE: N draws per batch element in place of a beam).  Step t, batch element b, slot k = 0..K-1: the slots
are the N samples of b, so N = K <= GPV_BEAM_MAX_K; logits row r = k*B + b.  lse, cand_v and cand_w are written for every row, finished
or not.
 1. Temperature and mask.  x_v = fp32(logit[r, v]) * inv_temp: one fp32 multiply; inv_temp = fp32(1 / temperature), computed in
    float64 on the host; field value 0 means temperature 1: no multiply.  Then + vocab_mask[v]: one fp32 add; no add when the mask
    is absent.
 2. Normalisation.  m and lse_r are taken over all v of the row as it stands after step 1, in the summation order pinned below.  lse
    is an OUTPUT of the device and an INPUT of the host rule.
 3. Candidates: the C = top_k largest x_v, ties to the lower v, rank j = 0..C-1; 1 <= C <= GPV_BEAM_MAX_C, C <= V.
    lp_j = x_j - lse_r: one fp32 subtract.  w_j = expf(lp_j) is evaluated on the device only.  cand_v[r, j] (int32) and cand_w[r, j]
    (fp32), both [K*B, C], are OUTPUTS of the step; cand_w is an INPUT of the host rule, which recomputes cand_v and lp itself.
 4. Nucleus.  c_j = c_{j-1} + w_j, c_{-1} = 0: serial fp32 additions in rank order.  n = 1 + #{ j in 0..C-2 : c_j < top_p }.  Field
    value 0 means off: n = C.  Otherwise 0 < top_p < 1.
 5. Draw.  bits = hash_u32(seed, ((uint64) t * B + b) * K + k), the function of csrc/common.h.  seed is read from a DEVICE pointer
    that holds one value: the caller rewrites it between replays, so a captured search draws anew each time.
    u = fp32(bits >> 8) * 2^-24, which is exact.  tau = u * c_{n-1}: one fp32 multiply.  j* = the first j < n with c_j > tau; if there
    is none, j* = n - 1.
 6. Finished slots behave as FREEZE does: with finished[b,k] set the token is pad_id, seq_lp and length stay unchanged.
 7. Write.  parent[b,k] = k.  seq_lp'[b,k] = seq_lp[b,k] + lp_{j*}: one fp32 add.  seqs'[k,b,t] = tok[k*B+b] = cand_v[r, j*].
    length' = length + 1.  finished' = finished | (token == stop_id).  No -1e9 rule at t = 0: the K slots differ by their draw.
Caller conditions: a mask leaves at least C finite entries per row; inv_pen, no_repeat, min_len and rep_* must be off in this mode
and are refused otherwise.  The reported seq_lp is the model's log-probability of the sequence at that temperature, over the whole
vocabulary -- what the beam search reports -- not the probability under the truncated sampler.  The sampler is truncated to at most
GPV_BEAM_MAX_C candidates; pure sampling over all of V does not exist.
"""
import math

import numpy as np

EXTEND, FREEZE, SAMPLE = 0, 1, 2          # GPV_BEAM_EXTEND, GPV_BEAM_FREEZE, GPV_BEAM_SAMPLE
MODES = {'extend': EXTEND, 'freeze': FREEZE}
MAX_K, MAX_T = 8, 64          # GPV_BEAM_MAX_K, GPV_BEAM_MAX_T
MAX_C = 64                    # GPV_BEAM_MAX_C
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


# ---- THE SAMPLER -------------------------------------------------------------------------------------------------------------------
def hash_u32(seed, idx):
    """csrc/common.h hash_u32 on numpy integers (lowbias32 finalizer on index ^ seed, high words folded in) -> uint64 array < 2^32"""
    M = np.uint64(0xFFFFFFFF)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    idx = np.asarray(idx).astype(np.uint64)
    x = (idx & M) ^ np.uint64(seed & 0xFFFFFFFF)
    x = x ^ ((((idx >> np.uint64(32)) & M) ^ np.uint64(seed >> 32)) * np.uint64(0x9E3779B9) & M)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7FEB352D)) & M
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846CA68B)) & M
    return x ^ (x >> np.uint64(16))


def draw_u(seed, t, b, k, B, K):
    """step 5: u = fp32(bits >> 8) * 2^-24 of slot (t, b, k), exact"""
    bits = int(hash_u32(seed, (int(t) * int(B) + int(b)) * int(K) + int(k)))
    return F32(bits >> 8) * F32(2.0 ** -24)


def inv_temperature(temperature):
    """inv_temp = fp32(1 / temperature) of step 1, computed in float64; None for temperature None or 1.0 (no multiply)"""
    if temperature is None or float(temperature) == 1.0:
        return None
    temperature = float(temperature)
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f'sampler: the temperature must be finite and positive, got {temperature!r} (use top_k=1 for the arg-max)')
    return F32(1.0 / temperature)


def check_sampler(K, V, T, t, top_k, top_p=None, inv_temp=None, inv_pen=None, no_repeat_ngram=0, min_length=0, repetition=None):
    """the extents of one sampled step; the beam's own rules (a length penalty table, the constraints) are refused in this mode"""
    check_extents(K, V, T, t)
    C = int(top_k)
    if not 1 <= C <= MAX_C:
        raise ValueError(f'sampler: 1 <= top_k <= {MAX_C} is supported (GPV_BEAM_MAX_C; sampling over the whole vocabulary does not exist), got {top_k}')
    if C > V:
        raise ValueError(f'sampler: top_k {C} exceeds the vocabulary ({V})')
    if top_p is not None and not 0.0 < float(F32(top_p)) < 1.0:
        raise ValueError(f'sampler: top_p must lie strictly between 0 and 1 (None: off), got {top_p!r}')
    if inv_temp is not None and not (math.isfinite(float(inv_temp)) and float(F32(inv_temp)) > 0.0 and math.isfinite(float(F32(inv_temp)))):
        raise ValueError(f'sampler: inv_temp must be finite and positive (inv_temperature; None: temperature 1), got {inv_temp!r}')
    if inv_pen is not None:
        raise ValueError('sampler: a length penalty does not combine with sampling (nothing is ranked; a follow-up)')
    if int(no_repeat_ngram) != 0 or int(min_length) != 0 or repetition is not None:
        raise ValueError('sampler: no_repeat_ngram / min_length / repetition do not combine with sampling (the sampled step is not taught '
                         'the constraints; a follow-up)')


def sample_step_host(logits, lse, cand_w, seq_lp, seqs, finished, length, t, pad_id, stop_id, seed, top_k, top_p=None, inv_temp=None,
                     vocab_mask=None, u=None):
    """One sampled step (THE SAMPLER above).  logits [K*B, V] (values exactly representable in fp32), lse [K*B] fp32 (the device's, or
    any log-sum-exp of the rows as they stand after step 1), cand_w [K*B, C] fp32 (the device's expf(lp), or np.exp(lp) rounded to fp32),
    seq_lp [B,K] fp32, seqs [K,B,T] int64, finished [B,K] 0/1, length [B,K] int; top_p / inv_temp None: off.  u ([B,K] fp32 or None):
    the uniform numbers of step 5 in place of the hash (tests reach the fallback of step 5 with it).  Nothing is modified.
    seq_lp is the model's log-probability of the sequence at that temperature over the whole vocabulary, as the beam search reports it;
    it is NOT the probability under the truncated sampler.
    -> dict(parent, tok, seqs, seq_lp, finished, length as beam_step_host; cand_v [K*B, C] int32, lp [K*B, C] fp32, n [B,K], pick [B,K])"""
    x = np.asarray(logits, dtype=F32)
    K, B, T = seqs.shape
    V = x.shape[1]
    C = int(top_k)
    check_sampler(K, V, T, t, C, top_p, inv_temp)
    if x.shape[0] != K * B:
        raise ValueError(f'sampler: logits must have K*B = {K * B} rows, got {x.shape[0]}')
    if inv_temp is not None:
        x = x * F32(inv_temp)                                                    # step 1: one fp32 multiply
    if vocab_mask is not None:
        x = x + np.asarray(vocab_mask, dtype=F32)[None, :]                       # one fp32 add
    lse = np.asarray(lse, dtype=F32)
    w = np.asarray(cand_w, dtype=F32).reshape(K * B, C)
    seq_lp = np.asarray(seq_lp, dtype=F32)
    cand_v = np.argsort(-x, axis=1, kind='stable')[:, :C].astype(np.int32)       # step 3: C largest, ties to the lower v
    lp = (np.take_along_axis(x, cand_v.astype(np.int64), axis=1) - lse[:, None]).astype(F32)      # one fp32 subtract
    out = {'parent': np.tile(np.arange(K, dtype=np.int32), (B, 1)), 'tok': np.zeros(K * B, np.int64), 'seqs': np.array(seqs, dtype=np.int64),
           'seq_lp': np.zeros((B, K), F32), 'finished': np.zeros((B, K), np.int32), 'length': np.zeros((B, K), np.int32),
           'cand_v': cand_v, 'lp': lp, 'n': np.zeros((B, K), np.int32), 'pick': np.zeros((B, K), np.int32)}
    p = None if top_p is None else F32(top_p)
    for b in range(B):
        for k in range(K):
            r = k * B + b
            c = np.zeros(C, F32)
            acc = F32(0.0)
            for j in range(C):                                                   # step 4: serial fp32 additions in rank order
                acc = F32(acc + w[r, j])
                c[j] = acc
            n = C if p is None else 1 + int(np.sum(c[:C - 1] < p))
            uu = draw_u(seed, t, b, k, B, K) if u is None else F32(np.asarray(u)[b, k])
            tau = F32(uu * c[n - 1])                                             # step 5: one fp32 multiply
            over = np.nonzero(c[:n] > tau)[0]
            js = int(over[0]) if len(over) else n - 1
            fin = bool(finished[b, k])
            tokv = pad_id if fin else int(cand_v[r, js])                         # step 6
            out['n'][b, k], out['pick'][b, k] = n, js
            out['seq_lp'][b, k] = seq_lp[b, k] if fin else F32(seq_lp[b, k] + lp[r, js])        # step 7: one fp32 add
            out['seqs'][k, b, t] = tokv
            out['tok'][r] = tokv
            out['length'][b, k] = int(length[b, k]) + (0 if fin else 1)
            out['finished'][b, k] = int(fin or tokv == stop_id)
    return out


def sample_search_host(step_logits_fn, B, K, T, cls_id, pad_id, stop_id, seed, top_k, top_p=None, inv_temp=None, vocab_mask=None):
    """The chained sampled search: step_logits_fn(t, tok [K,B,t+1] int64) -> logits [K*B, V] of the newest position (tok[:, :, 0] =
    cls_id).  lse and cand_w are the host's (float64, rounded to fp32).  -> dict(seqs [K,B,T], seq_lp [B,K], finished, length)"""
    seqs = np.zeros((K, B, T), np.int64)
    seq_lp = np.zeros((B, K), F32)
    finished = np.zeros((B, K), np.int32)
    length = np.zeros((B, K), np.int32)
    tok = np.full((K, B, 1), cls_id, np.int64)
    for t in range(T - 1):
        logits = np.asarray(step_logits_fn(t, tok), dtype=F32)
        x = logits if inv_temp is None else logits * F32(inv_temp)
        lse = lse_host(x, vocab_mask)
        if vocab_mask is not None:
            x = x + np.asarray(vocab_mask, dtype=F32)[None, :]
        top = -np.sort(-x, axis=1, kind='stable')[:, :int(top_k)]
        cand_w = np.exp((top - lse[:, None]).astype(F32).astype(np.float64)).astype(F32)
        o = sample_step_host(logits, lse, cand_w, seq_lp, seqs, finished, length, t, pad_id, stop_id, seed, top_k, top_p=top_p,
                             inv_temp=inv_temp, vocab_mask=vocab_mask)
        tok = np.concatenate((tok, o['tok'].reshape(K, B, 1)), axis=-1)
        seqs, seq_lp, finished, length = o['seqs'], o['seq_lp'], o['finished'], o['length']
    return {'seqs': seqs, 'seq_lp': seq_lp, 'finished': finished, 'length': length}
