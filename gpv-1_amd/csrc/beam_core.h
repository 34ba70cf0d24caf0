// What the two beam search steps share (beam_step.hip: the whole vocabulary; phrase_step.hip: the tokens a trie allows), stated once:
// the tie rule, the lane's sorted list, the workgroup arg-max pop, the sum of exponentials in the order include/gpv_beam.h pins, the
// ranking of the K*K candidates by counting, the in-place slot write and the argument checks.  Both kernels are held bit for bit to a
// host rule (gpv1_amd.beam.select_slots is this file's ranking and slot write), so a change here changes both or neither.
// One 256-thread workgroup per batch element; every function below is called by all of its threads (the __syncthreads inside count on it).
// Every load address is clamped into its array and the value padded at use; no loop bound depends on the data.
// Include under `#pragma clang fp contract(off)`, after the public header of the kernel's own argument struct.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/gpv_beam.h"

namespace beam_core {

constexpr int LANES = GPV_BEAM_LANES;
constexpr int WAVES = LANES / 64;
constexpr int MAXK = GPV_BEAM_MAX_K;
constexpr int MAXT = GPV_BEAM_MAX_T;
constexpr int UN = 8;                      // loads of one lane in flight together
constexpr int NONE = 0x7fffffff;           // the token of an empty entry of a gathered list: loses every tie, so it is behind every real entry
static_assert(MAXK * MAXK <= 64, "the candidates of one batch element are ranked by one wave");

// the LDS both kernels use (each declares its own extra state beside it); rows_s first: no padding
struct Shared {
  int64_t rows_s[MAXK * MAXT];               // the parents' seqs rows of this b
  float red_v[WAVES];                        // the four wave heads of a reduction
  int red_i[WAVES], red_l[WAVES];
  float win_x[MAXK * MAXK];                  // x of candidate (k1, k2)
  int win_v[MAXK * MAXK];                    // its token
  float lse_s[MAXK];
  float key_s[64];
  int ok_s[64];
  float sel_score[MAXK];                     // the chosen candidate of slot k
  int sel_k1[MAXK], sel_w[MAXK], sel_len[MAXK];
};

// (a, ia) beats (b, ib): larger value, ties to the lower index
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }
__device__ __forceinline__ int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }

template <bool BF>
__device__ __forceinline__ const void* row_ptr(const void* logits, int r, int64_t pitch) {
  return BF ? (const void*)(reinterpret_cast<const uint16_t*>(logits) + (int64_t)r * pitch)
            : (const void*)(reinterpret_cast<const float*>(logits) + (int64_t)r * pitch);
}

template <bool BF>
__device__ __forceinline__ float load_x(const void* row, int v) {
  if (BF) return __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(row)[v] << 16);   // bf16 -> fp32 is exact
  return reinterpret_cast<const float*>(row)[v];
}

// UN loads of a lane in flight: x of v = (it0 + u) * LANES + tid clamped to V - 1 (an element behind V repeats the last one), mask added
template <bool BF, bool MASK>
__device__ __forceinline__ void load_un(const void* row, const float* mask, int it0, int tid, int V, float (&xs)[UN]) {
#pragma unroll
  for (int u = 0; u < UN; ++u) {
    const int v = (it0 + u) * LANES + tid;
    const int vc = v < V ? v : V - 1;
    xs[u] = load_x<BF>(row, vc);
    if (MASK) xs[u] = xs[u] + mask[vc];
  }
}

// The lane's sorted top-K list, value descending.  GATHER = false: the elements arrive in ascending index, so x enters in front of the
// first entry it is strictly greater than and equal values stay behind the earlier (lower) index.  GATHER = true: they arrive in any
// token order and carry a payload word e, so (x, v) enters in front of the first entry it beats.
template <bool GATHER>
struct LaneList {
  float lv[MAXK];
  int li[MAXK];
  int le[GATHER ? MAXK : 1];
  static constexpr int EMPTY = GATHER ? NONE : 0;

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int j = 0; j < MAXK; ++j) { lv[j] = -INFINITY; li[j] = EMPTY; if (GATHER) le[j] = 0; }
  }
  __device__ __forceinline__ void insert(int K, float x, int v, int e = 0) {
    bool carry = false;
    float cx = x;
    int ci = v, ce = e;
#pragma unroll
    for (int j = 0; j < MAXK; ++j) {
      if (j < K) {
        const bool in = carry || (GATHER ? beats(cx, ci, lv[j], li[j]) : cx > lv[j]);
        const float ov = lv[j];
        const int oi = li[j];
        lv[j] = in ? cx : ov;
        li[j] = in ? ci : oi;
        cx = in ? ov : cx;
        ci = in ? oi : ci;
        if (GATHER) { const int oe = le[j]; le[j] = in ? ce : oe; ce = in ? oe : ce; }
        carry = in;
      }
    }
  }
  // the owner of a popped head drops it
  __device__ __forceinline__ void shift() {
#pragma unroll
    for (int j = 0; j + 1 < MAXK; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; if (GATHER) le[j] = le[j + 1]; }
    lv[MAXK - 1] = -INFINITY; li[MAXK - 1] = EMPTY;
    if (GATHER) le[MAXK - 1] = 0;
  }
};

struct Best { float v; int i, lane; };

// (ov, oi, ol) replaces the best so far when it beats it; equal (value, index) go to the lower thread
__device__ __forceinline__ void fold_best(float ov, int oi, int ol, float& bv, int& bi, int& bl) {
  const bool take = beats(ov, oi, bv, bi) || (ov == bv && oi == bi && ol < bl);
  bv = take ? ov : bv; bi = take ? oi : bi; bl = take ? ol : bl;
}

// the workgroup's best head (v, i) and the thread that owns it: xor butterflies fold a wave, then the four wave heads in LDS.
// The caller's __syncthreads behind its use of the result frees red_* for the next call.
__device__ __forceinline__ Best pop_best(Shared& sh, int tid, float hv, int hi) {
  float bv = hv;
  int bi = hi, bl = tid;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(bv, off);
    const int oi = __shfl_xor(bi, off);
    const int ol = __shfl_xor(bl, off);
    fold_best(ov, oi, ol, bv, bi, bl);
  }
  if ((tid & 63) == 0) { sh.red_v[tid >> 6] = bv; sh.red_i[tid >> 6] = bi; sh.red_l[tid >> 6] = bl; }
  __syncthreads();
  bv = sh.red_v[0]; bi = sh.red_i[0]; bl = sh.red_l[0];
#pragma unroll
  for (int w = 1; w < WAVES; ++w) fold_best(sh.red_v[w], sh.red_i[w], sh.red_l[w], bv, bi, bl);
  return {bv, bi, bl};
}

// lse of one row with maximum m, to lse_s[k1] and *lse_out: the one statement of the order gpv_beam.h pins -- every lane adds
// expf(x - m) in ascending v, xor butterflies fold a wave, lane 0 adds the four wave sums in wave order (beam.n_chain bounds the chain)
// load(it0, xs): the UN values of the lane from iteration it0 on (load_un, plus whatever the kernel applies to a value on load)
template <class Load>
__device__ __forceinline__ void row_sum_exp_of(Shared& sh, int tid, Load load, float m, int V, int k1, float* lse_out) {
  const int iters = (V + LANES - 1) / LANES;
  float s = 0.f;
  for (int it0 = 0; it0 < iters; it0 += UN) {
    float xs[UN];
    load(it0, xs);
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const float e = expf(xs[u] - m);
      s = s + ((it0 + u) * LANES + tid < V ? e : 0.f);          // (s + 0.f is exact: an element behind V adds no rounding)
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off);
  if ((tid & 63) == 0) sh.red_v[tid >> 6] = s;
  __syncthreads();
  if (tid == 0) {
    float tot = sh.red_v[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) tot = tot + sh.red_v[w];
    const float lse = m + logf(tot);
    sh.lse_s[k1] = lse;
    *lse_out = lse;
  }
  __syncthreads();
}

template <bool BF, bool MASK>
__device__ __forceinline__ void row_sum_exp(Shared& sh, int tid, const void* row, const float* mask, float m, int V, int k1, float* lse_out) {
  row_sum_exp_of(sh, tid, [&](int it0, float (&xs)[UN]) { load_un<BF, MASK>(row, mask, it0, tid, V, xs); }, m, V, k1, lse_out);
}

// Thread tid < K*K holds candidate tid = k1*K + k2 (ok: it exists): key = score * inv_pen[len clamped], rank = the number of
// candidates that beat it (key descending, ties to the lower k1*K + k2; no data-dependent sort).  The first K fill sel_*; -> the
// candidate's slot, or -1.  A NaN key can leave a slot unwritten: write_slots clamps whatever LDS held.
__device__ __forceinline__ int select_by_rank(Shared& sh, int tid, int K, int T, const float* inv_pen, bool ok, int k1, int w,
                                               float score, int len) {
  const float key = inv_pen ? score * inv_pen[clampi(len, 0, T)] : score;
  if (tid < 64) { sh.key_s[tid] = key; sh.ok_s[tid] = ok ? 1 : 0; }
  __syncthreads();
  if (tid >= 64) return -1;
  int rank = 0;
  for (int o = 0; o < K * K; ++o) {
    const float ko = sh.key_s[o];
    rank += (sh.ok_s[o] && (ko > key || (ko == key && o < tid))) ? 1 : 0;
  }
  if (!ok || rank >= K) return -1;
  sh.sel_k1[rank] = k1;
  sh.sel_w[rank] = w;
  sh.sel_score[rank] = score;
  sh.sel_len[rank] = len;
  return rank;
}

// stage the K parents' seqs rows of this b, then write the K slots in place (only this workgroup touches b's rows); the kernel writes
// its own extra state beside it, behind the __syncthreads in here
template <class Args>
__device__ __forceinline__ void write_slots(Shared& sh, const Args& a, int tid, int b) {
  const int B = a.B, K = a.K, V = a.V, T = a.T, t = a.t;
  for (int i = tid; i < K * t; i += LANES) {
    const int k = i / t, p = i - k * t;
    sh.rows_s[k * MAXT + p] = a.seqs[((int64_t)k * B + b) * T + p];
  }
  __syncthreads();
  for (int i = tid; i < K * (t + 1); i += LANES) {
    const int k = i / (t + 1), p = i - k * (t + 1);
    const int k1 = clampi(sh.sel_k1[k], 0, K - 1);
    const int w = clampi(sh.sel_w[k], 0, V - 1);
    a.seqs[((int64_t)k * B + b) * T + p] = p < t ? sh.rows_s[k1 * MAXT + p] : (int64_t)w;
  }
  if (tid < K) {
    a.parent[b * K + tid] = clampi(sh.sel_k1[tid], 0, K - 1);
    a.seq_lp[b * K + tid] = sh.sel_score[tid];
    a.length[b * K + tid] = sh.sel_len[tid];
    a.tok[tid * B + b] = (int64_t)clampi(sh.sel_w[tid], 0, V - 1);
  }
}

// the argument checks both entry points make (min_V: the least vocabulary the step can fill its lists from)
template <class Args>
inline bool check_step_common(const Args* a, int min_V) {
  if (!a || !a->logits || !a->lse || !a->seq_lp || !a->seqs || !a->tok || !a->parent || !a->length) return false;
  if (a->B < 0 || a->K < 1 || a->K > MAXK || a->V < min_V || a->T < 2 || a->T > MAXT || a->t < 0 || a->t >= a->T - 1 || a->pitch < a->V)
    return false;
  if (a->pad_id < 0 || a->pad_id >= a->V || a->stop_id < 0 || a->stop_id >= a->V) return false;
  if (a->dtype != GPV_BEAM_BF16 && a->dtype != GPV_BEAM_F32) return false;
  return (int64_t)a->K * a->B <= 0x7fffffff / 2 && a->V <= (1 << 30);   // (32-bit element indices in the kernels)
}

// mode GPV_BEAM_SAMPLE of gpv_beam_step: its checks and its launch (sample_step.hip, libgpv_beam.so only)
__attribute__((visibility("hidden"))) int launch_sample(const gpv_beam_args* a, void* stream);

}  // namespace beam_core
