// One phrase-constrained beam search step (include/gpv_phrase.h states the rule; the host statement of the same rule is
// gpv1_amd.phrases.phrase_step_host).  One launch, one 256-thread workgroup per batch element b, the layout of beam_step.hip.  For each
// parent k1 that is live and has allowed tokens the workgroup walks row k1*B+b twice over the WHOLE vocabulary -- the row maximum m,
// then the sum of expf(x - m) in the order gpv_beam.h pins (lane l adds v = l, l + 256, ... in ascending v, xor butterflies fold a
// wave, lane 0 adds the four wave sums in wave order) -- and once over the node's allowed tokens: candidate i < cnt is the edge
// child_off[n] + i (token gathered through child_tok, logit gathered from the row, which the two passes have just pulled through the
// cache), candidate cnt is stop_id at a terminal node; lane l keeps a sorted top-K list over i = l, l + 256, ... (a node may have more
// children than the workgroup has lanes) and min(K, |A|) arg-max reductions pop the winners.  The rows of DONE and VOID parents are
// not read.  Wave 0 then forms the at most K*K candidates, ranks each by counting the candidates that beat it (no data-dependent
// sort), and the workgroup writes the K new slots after staging the parents' seqs rows in LDS -- only this workgroup touches b's
// rows, so everything is in place.
// Every load address is clamped into its array and the value padded at use: node into [0, M), edge into
// [0, E), token into [0, V).  Every loop bound is a shape or a clamped child_off difference.  A malformed trie or a NaN can only
// change WHICH in-range index is written.
// -ffp-contract=off: every score, key and lp is one separately rounded fp32 operation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/gpv_phrase.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = GPV_PHRASE_LANES;
constexpr int WAVES = LANES / 64;
constexpr int MAXK = GPV_PHRASE_MAX_K;
constexpr int MAXT = GPV_PHRASE_MAX_T;
constexpr int UN = 8;                      // loads of one lane in flight together
constexpr int NONE = 0x7fffffff;           // the token of an empty list entry: loses every tie, so it is behind every real entry
static_assert(MAXK * MAXK <= 64, "the candidates of one batch element are ranked by one wave");
static_assert(sizeof(gpv_phrase_args) == 160, "ABI of include/gpv_phrase.h");

// (a, ia) beats (b, ib): larger value, ties to the lower token
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <bool BF>
__device__ __forceinline__ float load_x(const void* row, int v) {
  if (BF) return __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(row)[v] << 16);   // bf16 -> fp32 is exact
  return reinterpret_cast<const float*>(row)[v];
}

// (x, v, i) enters the lane's list (value descending, token ascending) in front of the first entry it beats
__device__ __forceinline__ void insert(float (&lv)[MAXK], int (&li)[MAXK], int (&le)[MAXK], int K, float x, int v, int i) {
  bool carry = false;
  float cx = x;
  int ci = v, ce = i;
#pragma unroll
  for (int j = 0; j < MAXK; ++j) {
    if (j < K) {
      const bool in = carry || beats(cx, ci, lv[j], li[j]);
      const float ov = lv[j];
      const int oi = li[j], oe = le[j];
      lv[j] = in ? cx : ov;
      li[j] = in ? ci : oi;
      le[j] = in ? ce : oe;
      cx = in ? ov : cx;
      ci = in ? oi : ci;
      ce = in ? oe : ce;
      carry = in;
    }
  }
}

template <bool BF>
__global__ __launch_bounds__(LANES) void phrase_step_kernel(gpv_phrase_args a) {
  __shared__ float red_v[WAVES];
  __shared__ int red_i[WAVES];
  __shared__ int red_l[WAVES];
  __shared__ float win_x[MAXK * MAXK];        // x of candidate (k1, k2)
  __shared__ int win_v[MAXK * MAXK];          // its token
  __shared__ int win_e[MAXK * MAXK];          // its index among the node's allowed tokens (cnt: stop_id)
  __shared__ int win_ok[MAXK * MAXK];         // the candidate exists
  __shared__ int win_node[MAXK * MAXK], win_phr[MAXK * MAXK];
  __shared__ float lse_s[MAXK];
  __shared__ int done_s[MAXK];
  __shared__ float key_s[64];
  __shared__ int ok_s[64];
  __shared__ float sel_score[MAXK];
  __shared__ int sel_k1[MAXK], sel_w[MAXK], sel_node[MAXK], sel_phr[MAXK], sel_len[MAXK];
  __shared__ int64_t rows_s[MAXK * MAXT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int B = a.B, K = a.K, V = a.V, T = a.T, t = a.t, M = a.M, E = a.E;
  const int iters = (V + LANES - 1) / LANES;
  const float NINF = -INFINITY;

  if (tid < 64) win_ok[tid] = 0;
  if (tid < MAXK) {                            // a slot no candidate reaches is VOID
    sel_k1[tid] = 0; sel_w[tid] = a.pad_id; sel_score[tid] = -1e9f; sel_node[tid] = GPV_PHRASE_VOID; sel_phr[tid] = -1; sel_len[tid] = 0;
    done_s[tid] = 0; lse_s[tid] = 0.f;
  }
  __syncthreads();

  for (int k1 = 0; k1 < K; ++k1) {
    const int r = k1 * B + b;
    // the parent's state: the same words for every thread, so every branch on them is taken by the whole workgroup
    const int n = a.node[b * K + k1];
    const bool counts = !(t == 0 && k1 > 0);
    const bool live = counts && n >= 0;
    const int nc = clampi(n, 0, M - 1);
    const int e0 = clampi(a.child_off[nc], 0, E), e1 = clampi(a.child_off[nc + 1], 0, E);
    const int cnt = live && e1 > e0 ? e1 - e0 : 0;
    const int term = a.terminal[nc];
    const int na = cnt + (live && term >= 0 ? 1 : 0);          // |A| <= E + 1
    const int nk = na < K ? na : K;
    if (counts && n == GPV_PHRASE_DONE && tid == 0) {          // exactly one candidate: pad_id, score and length unchanged
      win_ok[k1 * K] = 1; win_v[k1 * K] = a.pad_id; win_x[k1 * K] = 0.f;
      win_node[k1 * K] = GPV_PHRASE_DONE; win_phr[k1 * K] = a.phrase[b * K + k1];
      done_s[k1] = 1;
    }
    if (na == 0) {
      if (tid == 0) a.lse[r] = 0.f;
      continue;
    }
    const void* row = BF ? (const void*)(reinterpret_cast<const uint16_t*>(a.logits) + (int64_t)r * a.pitch)
                         : (const void*)(reinterpret_cast<const float*>(a.logits) + (int64_t)r * a.pitch);
    // ---- pass 1: the row maximum ----
    float m = NINF;
    for (int it0 = 0; it0 < iters; it0 += UN) {
      float xs[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = (it0 + u) * LANES + tid;
        xs[u] = load_x<BF>(row, v < V ? v : V - 1);            // (an element behind V repeats the last one: the maximum is the same)
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) m = fmaxf(m, xs[u]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) red_v[wave] = m;
    __syncthreads();
    m = red_v[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) m = fmaxf(m, red_v[w]);
    __syncthreads();
    // ---- pass 2: sum of expf(x - m), the order gpv_beam.h pins ----
    float s = 0.f;
    for (int it0 = 0; it0 < iters; it0 += UN) {
      float xs[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = (it0 + u) * LANES + tid;
        xs[u] = load_x<BF>(row, v < V ? v : V - 1);
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const float e = expf(xs[u] - m);
        s = s + ((it0 + u) * LANES + tid < V ? e : 0.f);          // (s + 0.f is exact: an element behind V adds no rounding)
      }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off);
    if (lane == 0) red_v[wave] = s;
    __syncthreads();
    if (tid == 0) {
      float tot = red_v[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) tot = tot + red_v[w];
      const float lse = m + logf(tot);
      lse_s[k1] = lse;
      a.lse[r] = lse;
    }
    __syncthreads();
    // ---- the lane's top-K list over its share of the allowed tokens ----
    float lv[MAXK];
    int li[MAXK], le[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) { lv[j] = NINF; li[j] = NONE; le[j] = 0; }
    const int giters = (na + LANES - 1) / LANES;
    for (int it = 0; it < giters; ++it) {
      const int i = it * LANES + tid;
      const int e = clampi(e0 + i, 0, E - 1);
      int v = i < cnt ? a.child_tok[e] : a.stop_id;
      v = clampi(v, 0, V - 1);
      const float x = load_x<BF>(row, v);
      insert(lv, li, le, K, i < na ? x : NINF, i < na ? v : NONE, i);
    }
    // ---- nk pops: the workgroup's best head, its owner records it and shifts its list ----
    for (int k2 = 0; k2 < nk; ++k2) {
      float bv = lv[0];
      int bi = li[0], bl = tid;
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        const int ol = __shfl_xor(bl, off);
        const bool take = beats(ov, oi, bv, bi) || (ov == bv && oi == bi && ol < bl);
        bv = take ? ov : bv; bi = take ? oi : bi; bl = take ? ol : bl;
      }
      if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; red_l[wave] = bl; }
      __syncthreads();
      bv = red_v[0]; bi = red_i[0]; bl = red_l[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) {
        const float ov = red_v[w];
        const int oi = red_i[w], ol = red_l[w];
        const bool take = beats(ov, oi, bv, bi) || (ov == bv && oi == bi && ol < bl);
        bv = take ? ov : bv; bi = take ? oi : bi; bl = take ? ol : bl;
      }
      if (tid == bl) {
        const int c = k1 * K + k2;
        win_x[c] = lv[0]; win_v[c] = li[0]; win_e[c] = le[0];
        win_ok[c] = li[0] != NONE ? 1 : 0;                       // (a NaN logit never enters a list: the candidate is missing)
#pragma unroll
        for (int j = 0; j + 1 < MAXK; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; le[j] = le[j + 1]; }
        lv[MAXK - 1] = NINF; li[MAXK - 1] = NONE; le[MAXK - 1] = 0;
      }
      __syncthreads();
    }
    // ---- where each winner leads: a child of n, or DONE with the phrase that ends at n ----
    if (tid < nk) {
      const int c = k1 * K + tid;
      const int i = win_e[c];
      const bool edge = i < cnt;
      const int child = a.child_node[clampi(e0 + i, 0, E - 1)];
      win_node[c] = edge ? clampi(child, 0, M - 1) : GPV_PHRASE_DONE;
      win_phr[c] = edge ? -1 : term;
    }
  }
  __syncthreads();

  // ---- the K*K candidates: one wave, candidate c = k1*K + k2 ----
  const int KK = K * K;
  const int c = tid < KK ? tid : KK - 1;                 // (lanes behind the candidates compute the last one's and drop it)
  const int ck1 = c / K;
  const float slp = a.seq_lp[b * K + ck1];
  const int dn = done_s[ck1];
  const int len = a.length[b * K + ck1] + (dn ? 0 : 1);
  const float lp = win_x[c] - lse_s[ck1];
  float score = slp + lp;
  if (dn) score = slp;
  const bool ok = tid < KK && win_ok[c] != 0;
  const int lc = len < 0 ? 0 : (len > T ? T : len);
  const float key = a.inv_pen ? score * a.inv_pen[lc] : score;
  if (tid < 64) { key_s[tid] = key; ok_s[tid] = ok ? 1 : 0; }
  __syncthreads();
  if (tid < 64) {
    int rank = 0;
    for (int o = 0; o < KK; ++o) {
      const float ko = key_s[o];
      rank += (ok_s[o] && (ko > key || (ko == key && o < tid))) ? 1 : 0;
    }
    if (ok && rank < K) {
      sel_k1[rank] = ck1;
      sel_w[rank] = win_v[c];
      sel_score[rank] = score;
      sel_node[rank] = win_node[c];
      sel_phr[rank] = win_phr[c];
      sel_len[rank] = len;
    }
  }
  // ---- stage the K parents' rows of this b, then write the K slots in place ----
  for (int i = tid; i < K * t; i += LANES) {
    const int k = i / t, p = i - k * t;
    rows_s[k * MAXT + p] = a.seqs[((int64_t)k * B + b) * T + p];
  }
  __syncthreads();
  for (int i = tid; i < K * (t + 1); i += LANES) {
    const int k = i / (t + 1), p = i - k * (t + 1);
    const int k1 = clampi(sel_k1[k], 0, K - 1);
    const int w = clampi(sel_w[k], 0, V - 1);
    a.seqs[((int64_t)k * B + b) * T + p] = p < t ? rows_s[k1 * MAXT + p] : (int64_t)w;
  }
  if (tid < K) {
    a.parent[b * K + tid] = clampi(sel_k1[tid], 0, K - 1);
    a.seq_lp[b * K + tid] = sel_score[tid];
    a.node[b * K + tid] = sel_node[tid];
    a.phrase[b * K + tid] = sel_phr[tid];
    a.length[b * K + tid] = sel_len[tid];
    a.tok[tid * B + b] = (int64_t)clampi(sel_w[tid], 0, V - 1);
  }
}

}  // namespace

extern "C" int gpv_phrase_step(const gpv_phrase_args* a, void* stream) {
  if (!a || !a->logits || !a->lse || !a->seq_lp || !a->seqs || !a->tok || !a->parent || !a->length || !a->node || !a->phrase ||
      !a->child_off || !a->child_tok || !a->child_node || !a->terminal)
    return (int)hipErrorInvalidValue;
  if (a->B < 0 || a->K < 1 || a->K > MAXK || a->V < 1 || a->T < 2 || a->T > MAXT || a->t < 0 || a->t >= a->T - 1 || a->pitch < a->V)
    return (int)hipErrorInvalidValue;
  if (a->M < 2 || a->E < 1 || a->E > (1 << 30) || a->M > (1 << 30)) return (int)hipErrorInvalidValue;
  if (a->pad_id < 0 || a->pad_id >= a->V || a->stop_id < 0 || a->stop_id >= a->V) return (int)hipErrorInvalidValue;
  if (a->dtype != GPV_PHRASE_BF16 && a->dtype != GPV_PHRASE_F32) return (int)hipErrorInvalidValue;
  if ((int64_t)a->K * a->B > 0x7fffffff / 2 || a->V > (1 << 30)) return (int)hipErrorInvalidValue;   // (32-bit element indices in the kernel)
  if (a->B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a->B), block(LANES);
  if (a->dtype == GPV_PHRASE_BF16) phrase_step_kernel<true><<<grid, block, 0, st>>>(*a);
  else phrase_step_kernel<false><<<grid, block, 0, st>>>(*a);
  return (int)hipGetLastError();
}
