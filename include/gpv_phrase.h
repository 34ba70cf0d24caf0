/* C ABI of libgpv_phrase.so: one phrase-constrained beam search step on the device (gpv-1_amd/csrc/phrase_step.hip): every
 * hypothesis walks a trie of allowed answers, so a search can only return one of N given phrases.  The host statement of the same
 * rule is gpv1_amd.phrases.phrase_step_host.
 *
 * A library of its own: the export lists of the others are pinned.  The function takes plain device pointers, returns a hipError_t
 * as int (0 = ok), launches on `stream`, never synchronises, allocates nothing and keeps no global state (capturable).  Anything
 * outside the stated extents returns hipErrorInvalidValue before a launch.  The KV-cache reorder that follows a step is
 * gpv_beam_reorder of libgpv_beam.so, fed with this step's `parent`.
 *
 * THE TRIE.  M nodes, E = M - 1 edges.  The root is node 0; nodes are numbered breadth first, the children of a node in ascending
 * token order.  The edges of node n are child_off[n] .. child_off[n+1] - 1: child_tok[e] is the token, child_node[e] the child.
 * terminal[n] is the index of the phrase that ends at n, or -1.  A terminal node may have children; every leaf is terminal.
 *
 * THE STATE per (b, k): node (>= 0 live, GPV_PHRASE_DONE has spelled a phrase and stopped, GPV_PHRASE_VOID holds no hypothesis),
 * phrase (the phrase index once DONE, else -1), seq_lp, seqs, length as in gpv_beam.h.  Every slot starts at the root with score 0.
 *
 * THE RULE.  Step t (0 <= t < T-1), batch element b, parent k1 = 0..K-1, logits row r = k1*B + b:
 *  1. x_v = fp32(logit[r, v]).  lse_r = m + logf(sum_v expf(x_v - m)), m = max_v x_v, fp32, over the WHOLE vocabulary (no mask), summed
 *     in the order gpv_beam.h pins (256 lanes, strided, butterflies, waves in order: n_chain(V) = ceil(V / 256) + 6 + 3).  lse is an
 *     OUTPUT of the step and an INPUT of the host rule, so no transcendental is evaluated on both sides and everything below is
 *     bit-exact.  Only the rows of live parents that have candidates are read; lse of every other row is written as 0.
 *  2. Live parent at node n: the allowed tokens are child_tok[child_off[n] .. child_off[n+1] - 1], and stop_id when terminal[n] >= 0.
 *     Its candidates are the min(K, |A|) largest x_v over that set, ties to the lower v; k2 is the rank.  lp = x_v - lse_r: one fp32
 *     subtract.  score = seq_lp[b,k1] + lp: one fp32 add.  len' = length + 1.  v == stop_id: node' = DONE, phrase' = terminal[n]; any
 *     other v: node' = that child, phrase' = -1.
 *  3. DONE parent: exactly one candidate, k2 = 0: token pad_id, score and length unchanged, node' = DONE, phrase' carried.
 *  4. VOID parent: no candidate.  t == 0: a parent k1 > 0 has no candidate.
 *  5. key = score * inv_pen[clamp(len', 0, T)]: one fp32 multiply.  inv_pen == NULL: key = score.
 *  6. Selection: the first K candidates by key descending, ties to the lower k1*K + k2.  With only c < K candidates the slots
 *     c..K-1 become VOID: parent 0, token pad_id, seq_lp = -1e9 exactly, node' = VOID, phrase' = -1, length' = 0.
 *  7. Slot k with the chosen (k1, k2, w) (a VOID slot: (0, -, pad_id)): parent[b,k] = k1; seq_lp'[b,k] = score (raw, not the key);
 *     seqs'[k,b,:t] = seqs[k1,b,:t], seqs'[k,b,t] = w (positions behind t are left alone); tok[k*B+b] = w; node', phrase', length'.
 * A malformed trie or state (offsets, nodes or tokens out of range, a NaN logit) can give a wrong answer, never an out-of-range
 * access or an unbounded loop: every index is clamped before use and every loop bound is a shape or a clamped child_off difference. */
#ifndef GPV_PHRASE_H
#define GPV_PHRASE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_PHRASE_MAX_K 8        /* GPV_BEAM_MAX_K */
#define GPV_PHRASE_MAX_T 64       /* GPV_BEAM_MAX_T */
#define GPV_PHRASE_LANES 256      /* GPV_BEAM_LANES: the stride of the sum of step 1 */
#define GPV_PHRASE_DONE (-1)
#define GPV_PHRASE_VOID (-2)
#define GPV_PHRASE_BF16 0         /* dtype codes, the values of GPV_BF16 / GPV_F32 in gpv_hip.h */
#define GPV_PHRASE_F32 1

typedef struct gpv_phrase_args {
  const void* logits;           /* [K*B, V] bf16 or fp32, row r at logits + r * pitch elements */
  int64_t pitch;                /* row pitch in elements, >= V */
  const float* inv_pen;         /* [T+1] fp32 length-penalty table, or NULL */
  float* lse;                   /* [K*B] out */
  float* seq_lp;                /* [B,K] in / out */
  int64_t* seqs;                /* [K,B,T] in / out */
  int64_t* tok;                 /* [K*B] out: the decoder's next input tokens */
  int* parent;                  /* [B,K] out */
  int* length;                  /* [B,K] in / out */
  int* node;                    /* [B,K] in / out */
  int* phrase;                  /* [B,K] in / out */
  const int* child_off;         /* [M+1] */
  const int* child_tok;         /* [E] */
  const int* child_node;        /* [E] */
  const int* terminal;          /* [M] */
  int B, K, V, T, t;
  int pad_id, stop_id;          /* in [0, V) */
  int dtype;                    /* of logits: GPV_PHRASE_BF16 / GPV_PHRASE_F32 */
  int M, E;                     /* M >= 2 nodes, E >= 1 edges */
} gpv_phrase_args;

/* One launch, one workgroup of GPV_PHRASE_LANES threads per batch element.  Per live row the workgroup takes the row maximum and
 * sums the exponentials over all V; every thread keeps a sorted top-K list over its strided share of the node's allowed tokens
 * (gathered through child_tok; a node may have more children than the workgroup has lanes) and the workgroup pops the winners with
 * arg-max reductions; the at most K*K candidates (one wave) are ranked by counting how many candidates beat each one; the K seqs rows
 * of the batch element are staged in LDS before they are written back, so every array is updated in place.  B = 0: nothing is
 * launched. */
int gpv_phrase_step(const gpv_phrase_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
