/* C ABI of libgpv_beam.so: one beam search step on the device and the KV-cache reorder of all decoder layers
 * (gpv-1_amd/csrc/beam_step.hip).  The host statement of the same rule is gpv1_amd.beam.beam_step_host.
 *
 * A library of its own beside libgpv_hip.so, libgpv_eval.so, libgpv_cap.so, libgpv_match.so and libgpv_health.so: those five
 * export lists are pinned.  Every function takes plain device pointers, returns a hipError_t as int (0 = ok), launches on
 * `stream`, never synchronises, allocates nothing and keeps no global state (capturable).  Anything outside the stated extents
 * returns hipErrorInvalidValue before a launch.
 *
 * THE RULE.  Step t (0 <= t < T-1), batch element b, parent k1 = 0..K-1, logits row r = k1*B + b:
 *  1. x_v = fp32(logit[r, v]) + vocab_mask[v]: one fp32 add; no add when the mask is absent.
 *  2. lse_r = m + logf(sum_v expf(x_v - m)), m = max_v x_v, fp32.  The summation order is the kernel's own (below); lse is an
 *     OUTPUT of the step ([K*B] fp32) and an INPUT of the host rule, so no transcendental is evaluated on both sides and
 *     everything below is bit-exact.
 *  3. The row's candidates are its K largest x_v, ties to the lower v; k2 is the rank.  lp = x_v - lse_r: one fp32 subtract.
 *  4. score(k1,k2) = seq_lp[b,k1] + lp: one fp32 add.  t == 0 and k1 > 0: score = -1e9 exactly.  Mode FREEZE with
 *     finished[b,k1] set: the parent has exactly one candidate, k2 = 0, token pad_id, score = seq_lp[b,k1] unchanged; its other
 *     candidates do not exist.
 *  5. key = score * inv_pen[len']: one fp32 multiply, len' = length[b,k1] + (finished[b,k1] ? 0 : 1) (in either mode; clamped to
 *     T, the table's last entry).  inv_pen == NULL: key = score.  inv_pen[n] = fp32(((5 + n) / 6) ** -alpha), n = 0..T, computed
 *     once in float64 on the host (gpv1_amd.beam.length_table); the host rule and the kernel read the same table.
 *  6. Selection: the first K of the candidates sorted by key descending, ties to the lower k1*K + k2 (a stable sort).
 *  7. Slot k with the chosen (k1, k2, w): parent[b,k] = k1; seq_lp'[b,k] = score (raw, not the key);
 *     seqs'[k,b,:t] = seqs[k1,b,:t], seqs'[k,b,t] = w (positions behind t are left alone); tok[k*B+b] = w;
 *     finished'[b,k] = FREEZE ? (finished[b,k1] | (w == stop_id)) : 0; length'[b,k] = len'.
 * Mode EXTEND without penalty and mask is the reference's search (finished hypotheses keep extending, no normalisation).
 * Caller conditions: 1 <= K <= GPV_BEAM_MAX_K, K <= V, T <= GPV_BEAM_MAX_T; a mask leaves at least K finite entries per row; a
 * NaN logit gives an undefined selection (every index written stays inside its array; no loop bound depends on the data).
 *
 * THE CONSTRAINTS (no_repeat, min_len, rep_neg / rep_pos; all zero: off, and the rule is the one above).  They add to steps 1-3;
 * steps 4-7 are unchanged.  h = seqs[k1, b, 0:t] is the history of the row's parent: the tokens written so far (__cls__ is not part
 * of it; special tokens in it count like any other token).  A frozen parent (mode FREEZE with finished[b,k1] set) is exempt from
 * everything below; it still has its single pad_id candidate.
 *  1b. Repetition penalty, on when rep_neg and rep_pos are non-zero, after the mask add: for every v that occurs in h,
 *      x_v = x_v < 0 ? x_v * rep_neg : x_v * rep_pos: one fp32 multiply, applied once however often v occurs.  rep_neg = fp32(theta),
 *      rep_pos = fp32(1 / theta), computed in float64 on the host (gpv1_amd.beam.rep_factors): a multiply, not a divide, so that host
 *      and device round the same way.  -inf stays -inf.
 *  2.  m and lse_r are taken over ALL v of the row as it stands after 1b, banned tokens included: bans do not renormalise.  The first
 *      pop is no longer the row maximum when the maximum is banned, so m has a reduction of its own.  The summation order is the
 *      one pinned below, unchanged.
 *  3a. The banned set of the row.  (i) n = no_repeat >= 1 and t >= n - 1: with p = h[t-n+1 : t] (n - 1 tokens, empty for n = 1),
 *      for every i in 0 .. t-n with h[i : i+n-1] == p the token h[i+n-1] is banned (at most t - n + 1 bans; t = 0 bans nothing).
 *      (ii) stop_id is banned while length[b,k1] < min_len: at least min_len tokens precede __stop__.
 *  3.  The row's candidates are its K largest x_v AMONG THE TOKENS THAT ARE NOT BANNED, ties to the lower v; lp = x_v - lse_r.
 * Caller condition with a constraint on: every row keeps at least K entries that are finite and not banned (a row bans fewer than T
 * tokens, so a mask that leaves K + T finite entries, or V >= K + T without one, suffices).  Below it the selection is undefined
 * (every index written stays inside its array; no loop bound depends on the data).  Extents: 0 <= no_repeat <= GPV_BEAM_MAX_NGRAM,
 * 0 <= min_len <= T, rep_neg and rep_pos both zero or both finite and positive, and with any constraint on V <= GPV_BEAM_MAX_CONSTR_V
 * (a "seen" and a "banned" bitmap of V bits each in LDS, 16 KB together).
 *
 * THE SAMPLER (mode GPV_BEAM_SAMPLE: N draws per batch element in place of a beam).  Step t, batch element b, slot k = 0..K-1: the slots
 * are the N samples of b, so N = K <= GPV_BEAM_MAX_K; logits row r = k*B + b.  lse, cand_v and cand_w are written for every row, finished
 * or not.
 *  1. Temperature and mask.  x_v = fp32(logit[r, v]) * inv_temp: one fp32 multiply; inv_temp = fp32(1 / temperature), computed in
 *     float64 on the host; field value 0 means temperature 1: no multiply.  Then + vocab_mask[v]: one fp32 add; no add when the mask
 *     is absent.
 *  2. Normalisation.  m and lse_r are taken over all v of the row as it stands after step 1, in the summation order pinned below.  lse
 *     is an OUTPUT of the device and an INPUT of the host rule.
 *  3. Candidates: the C = top_k largest x_v, ties to the lower v, rank j = 0..C-1; 1 <= C <= GPV_BEAM_MAX_C, C <= V.
 *     lp_j = x_j - lse_r: one fp32 subtract.  w_j = expf(lp_j) is evaluated on the device only.  cand_v[r, j] (int32) and cand_w[r, j]
 *     (fp32), both [K*B, C], are OUTPUTS of the step; cand_w is an INPUT of the host rule, which recomputes cand_v and lp itself.
 *  4. Nucleus.  c_j = c_{j-1} + w_j, c_{-1} = 0: serial fp32 additions in rank order.  n = 1 + #{ j in 0..C-2 : c_j < top_p }.  Field
 *     value 0 means off: n = C.  Otherwise 0 < top_p < 1.
 *  5. Draw.  bits = hash_u32(seed, ((uint64) t * B + b) * K + k), the function of csrc/common.h.  seed is read from a DEVICE pointer
 *     that holds one value: the caller rewrites it between replays, so a captured search draws anew each time.
 *     u = fp32(bits >> 8) * 2^-24, which is exact.  tau = u * c_{n-1}: one fp32 multiply.  j* = the first j < n with c_j > tau; if there
 *     is none, j* = n - 1.
 *  6. Finished slots behave as FREEZE does: with finished[b,k] set the token is pad_id, seq_lp and length stay unchanged.
 *  7. Write.  parent[b,k] = k.  seq_lp'[b,k] = seq_lp[b,k] + lp_{j*}: one fp32 add.  seqs'[k,b,t] = tok[k*B+b] = cand_v[r, j*].
 *     length' = length + 1.  finished' = finished | (token == stop_id).  No -1e9 rule at t = 0: the K slots differ by their draw.
 * Caller conditions: a mask leaves at least C finite entries per row; inv_pen, no_repeat, min_len and rep_* must be off in this mode
 * and are refused otherwise.  The reported seq_lp is the model's log-probability of the sequence at that temperature, over the whole
 * vocabulary -- what the beam search reports -- not the probability under the truncated sampler.  The sampler is truncated to at most
 * GPV_BEAM_MAX_C candidates; pure sampling over all of V does not exist.
 *
 * THE SUM OF STEP 2.  256 lanes; lane l adds expf(x_v - m) for v = l, l + 256, l + 512, ... in ascending v onto 0.f, the 64 lanes
 * of a wave are folded by xor butterflies (32, 16, 8, 4, 2, 1), the four wave sums are added one after the other in wave order.
 * The longest chain of dependent fp32 additions is therefore  n_chain(V) = ceil(V / 256) + 6 + 3. */
#ifndef GPV_BEAM_H
#define GPV_BEAM_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_BEAM_MAX_K 8        /* beams per batch element */
#define GPV_BEAM_MAX_T 64       /* max_text_len */
#define GPV_BEAM_MAX_LAYERS 8   /* decoder layers of one gpv_beam_reorder call */
#define GPV_BEAM_LANES 256      /* threads of a gpv_beam_step workgroup: the stride of the sum of step 2 */
#define GPV_BEAM_MAX_NGRAM 8    /* largest no_repeat */
#define GPV_BEAM_MAX_CONSTR_V 65536   /* largest V with a constraint on */
#define GPV_BEAM_MAX_C 64       /* largest top_k of the sampler */

#define GPV_BEAM_EXTEND 0       /* finished hypotheses keep extending (the reference) */
#define GPV_BEAM_FREEZE 1       /* a hypothesis that emitted stop_id keeps its score and is followed by pad_id */
#define GPV_BEAM_SAMPLE 2       /* THE SAMPLER: every slot draws its own next token; finished slots as in FREEZE */

#define GPV_BEAM_BF16 0         /* dtype codes, the values of GPV_BF16 / GPV_F32 in gpv_hip.h */
#define GPV_BEAM_F32 1

typedef struct gpv_beam_args {
  const void* logits;           /* [K*B, V] bf16 or fp32, row r at logits + r * pitch elements */
  int64_t pitch;                /* row pitch in elements, >= V (the decoder writes logits[:, t] with pitch T*V) */
  const float* vocab_mask;      /* [V] fp32 added to every row, or NULL */
  const float* inv_pen;         /* [T+1] fp32 length-penalty table, or NULL */
  float* lse;                   /* [K*B] out */
  float* seq_lp;                /* [B,K] in / out */
  int64_t* seqs;                /* [K,B,T] in / out */
  int64_t* tok;                 /* [K*B] out: the decoder's next input tokens */
  int* parent;                  /* [B,K] out */
  int* finished;                /* [B,K] in / out, 0 or 1 */
  int* length;                  /* [B,K] in / out */
  const uint64_t* seed;         /* the sampler's seed: ONE value in device memory, read by the kernel; NULL in the other modes */
  int* cand_v;                  /* [K*B, top_k] out, the sampler's candidates by rank; NULL in the other modes */
  float* cand_w;                /* [K*B, top_k] out, expf(lp) of the candidates; NULL in the other modes */
  int B, K, V, T, t;
  int mode;                     /* GPV_BEAM_EXTEND / GPV_BEAM_FREEZE / GPV_BEAM_SAMPLE */
  int pad_id, stop_id;          /* in [0, V) */
  int dtype;                    /* of logits: GPV_BEAM_BF16 / GPV_BEAM_F32 */
  int top_k;                    /* the sampler's C, 1 .. GPV_BEAM_MAX_C; 0 in the other modes */
  float inv_temp;               /* the sampler's step 1: fp32(1 / temperature); 0 = temperature 1 */
  float top_p;                  /* the sampler's step 4: 0 < top_p < 1; 0 = off */
  int no_repeat;                /* n of step 3a (i): no n-gram is written twice; 0 = off */
  int min_len;                  /* step 3a (ii): stop_id is banned while length < min_len; 0 = off */
  float rep_neg, rep_pos;       /* step 1b: fp32(theta), fp32(1 / theta); both 0 = off */
} gpv_beam_args;

/* One launch, one workgroup of GPV_BEAM_LANES threads per batch element.  Per row every thread keeps a sorted top-K list over
 * its strided elements, the workgroup pops K winners with (value, index) arg-max reductions (the first is the row maximum) and
 * sums the exponentials; the K*K candidates (one wave) are ranked by counting how many candidates beat each one; the workgroup
 * stages the K seqs rows of its b in LDS before it writes them back, so seqs, seq_lp, finished and length are updated in place.
 * Every load is from a clamped index and padded at use.  B = 0: nothing is launched.
 * With a constraint on, another instantiation runs: per row the workgroup marks the history's tokens in the seen bitmap and the row's
 * bans in the banned bitmap (LDS; the words it touched are zeroed again behind the row), applies 1b at every load of both passes, keeps
 * banned tokens out of the lane lists and reduces m over the whole row.  Still one launch.
 * Mode GPV_BEAM_SAMPLE (csrc/sample_step.hip): per row top_k pops; a lane's list holds eight entries, and when the owner of a pop has
 * used up its eight every lane rebuilds its list from the elements that come strictly behind the last popped (x, v) in the order "x
 * descending, v ascending" -- one scan of the row when the candidates are spread over the lanes, at most ceil(top_k / 8) -- and the sum pass;
 * thread k then does steps 4 - 7 of slot k on the at most 64 values of its row in LDS.  Still one launch; parent is the identity, so no
 * gpv_beam_reorder follows.  The sampler's fields (seed, cand_v, cand_w, top_k, inv_temp, top_p) all zero with mode EXTEND or FREEZE is
 * the step as it was; anything else in them is refused there.  They stand in front of the constraints' fields, which stay the last four. */
int gpv_beam_step(const gpv_beam_args* a, void* stream);

typedef struct gpv_beam_reorder_args {
  void* cache[GPV_BEAM_MAX_LAYERS];   /* L caches [K*B, T, 3*D] (q | k | v columns), 16-byte aligned */
  const int* parent;                  /* [B,K] of gpv_beam_step (values outside 0..K-1 are clamped) */
  int L, B, K, T, D;
  int upto;                           /* positions < upto move, 1 <= upto <= T */
  int dtype;                          /* GPV_BEAM_BF16 / GPV_BEAM_F32; D * element size must be a multiple of 16 */
} gpv_beam_reorder_args;

/* One launch for all L layers: for positions < upto and the k | v columns, row k*B+b becomes old row parent[b,k]*B+b.  A thread
 * owns one (layer, b, position, 16-byte column vector), reads its K values and then writes its K values: in place, no scratch.
 * Positions >= upto and the q columns are not touched. */
int gpv_beam_reorder(const gpv_beam_reorder_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
