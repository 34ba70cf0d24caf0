// One beam search step and the KV-cache reorder of all decoder layers (include/gpv_beam.h states the rule; the host statement of
// the same rule is gpv1_amd.beam.beam_step_host).  Two launches per decoded token instead of the torch glue of GPV._beam_device:
//   step_kernel     one 256-thread workgroup per batch element b.  For each parent k1 the workgroup walks row k1*B+b twice:
//                   pass 1 -- every lane keeps a sorted top-K list (value descending, index ascending) over the elements v = lane,
//                   lane + 256, ...; K (value, index) arg-max reductions then pop the row's K winners, the first of which is the
//                   row maximum m; pass 2 -- the lanes add expf(x - m) in ascending v, xor butterflies fold a wave, lane 0 adds the
//                   four wave sums in wave order (the n_chain of the header).  Both passes keep eight loads of a lane in flight (163 -> 104 us
//                   at B = 64, K = 5, V = 10000; keeping the row in registers between the passes measured the same and was dropped).  Wave 0 then forms the K*K candidates, ranks each by
//                   counting the candidates that beat it (no data-dependent sort), and the workgroup writes the K new slots after
//                   staging the parents' seqs rows in LDS -- only this workgroup touches b's rows, so everything is in place.
//   reorder_kernel  one thread per (layer, b, position, 16-byte vector of the k | v columns): K loads, then K stores.
// Every load address is clamped into its array and the value padded at use; no loop bound depends on
// the data; a NaN anywhere can only change WHICH in-range index is written.
// -ffp-contract=off: every score, key and lp is one separately rounded fp32 operation.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/gpv_beam.h"

#pragma clang fp contract(off)

namespace {

constexpr int LANES = GPV_BEAM_LANES;
constexpr int WAVES = LANES / 64;
constexpr int MAXK = GPV_BEAM_MAX_K;
constexpr int MAXT = GPV_BEAM_MAX_T;
constexpr int UN = 8;                      // loads of one lane in flight together
static_assert(MAXK * MAXK <= 64, "the candidates of one batch element are ranked by one wave");
static_assert(sizeof(gpv_beam_args) == 128 && sizeof(gpv_beam_reorder_args) == 104, "ABI of include/gpv_beam.h");

// (a, ia) beats (b, ib): larger value, ties to the lower index
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) { return a > b || (a == b && ia < ib); }

template <bool BF>
__device__ __forceinline__ float load_x(const void* row, int v) {
  if (BF) return __uint_as_float((unsigned)reinterpret_cast<const uint16_t*>(row)[v] << 16);   // bf16 -> fp32 is exact
  return reinterpret_cast<const float*>(row)[v];
}

// x enters the lane's list (value descending; elements arrive in ascending v) when it is strictly greater than an entry: it goes in front
// of that entry, equal values stay behind the earlier (lower) index
__device__ __forceinline__ void insert(float (&lv)[MAXK], int (&li)[MAXK], int K, float x, int v) {
  bool carry = false;
  float cx = x;
  int ci = v;
#pragma unroll
  for (int j = 0; j < MAXK; ++j) {
    if (j < K) {
      const bool in = carry || cx > lv[j];
      const float ov = lv[j];
      const int oi = li[j];
      lv[j] = in ? cx : ov;
      li[j] = in ? ci : oi;
      cx = in ? ov : cx;
      ci = in ? oi : ci;
      carry = in;
    }
  }
}

template <bool BF, bool MASK>
__global__ __launch_bounds__(LANES) void step_kernel(gpv_beam_args a) {
  __shared__ float red_v[WAVES];
  __shared__ int red_i[WAVES];
  __shared__ int red_l[WAVES];
  __shared__ float win_x[MAXK * MAXK];        // x of candidate (k1, k2)
  __shared__ int win_v[MAXK * MAXK];          // its vocabulary index
  __shared__ float lse_s[MAXK];
  __shared__ float key_s[64];
  __shared__ int ok_s[64];
  __shared__ float sel_score[MAXK];
  __shared__ int sel_k1[MAXK], sel_w[MAXK], sel_fin[MAXK], sel_len[MAXK];
  __shared__ int64_t rows_s[MAXK * MAXT];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int B = a.B, K = a.K, V = a.V, T = a.T, t = a.t;
  const int iters = (V + LANES - 1) / LANES;
  const float NINF = -INFINITY;

  for (int k1 = 0; k1 < K; ++k1) {
    const int r = k1 * B + b;
    const void* row = BF ? (const void*)(reinterpret_cast<const uint16_t*>(a.logits) + (int64_t)r * a.pitch)
                         : (const void*)(reinterpret_cast<const float*>(a.logits) + (int64_t)r * a.pitch);
    // ---- pass 1: the lane's top-K list, value descending, index ascending (elements arrive in ascending v) ----
    float lv[MAXK];
    int li[MAXK];
#pragma unroll
    for (int j = 0; j < MAXK; ++j) { lv[j] = NINF; li[j] = 0; }
    for (int it0 = 0; it0 < iters; it0 += UN) {
      // UN loads in flight, then their insertions in ascending v (an element behind V is -inf and never enters)
      float xs[UN];
      int vs[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = (it0 + u) * LANES + tid;
        const int vc = v < V ? v : V - 1;
        float x = load_x<BF>(row, vc);
        if (MASK) x = x + a.vocab_mask[vc];
        xs[u] = v < V ? x : NINF;
        vs[u] = vc;
      }
#pragma unroll
      for (int u = 0; u < UN; ++u) insert(lv, li, K, xs[u], vs[u]);
    }
    // ---- K pops: the workgroup's best head, its owner shifts its list ----
    float m = 0.f;
    for (int k2 = 0; k2 < K; ++k2) {
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
      if (tid == 0) { win_x[k1 * K + k2] = bv; win_v[k1 * K + k2] = bi; }
      if (k2 == 0) m = bv;
      if (tid == bl) {
#pragma unroll
        for (int j = 0; j + 1 < MAXK; ++j) { lv[j] = lv[j + 1]; li[j] = li[j + 1]; }
        lv[MAXK - 1] = NINF; li[MAXK - 1] = 0;
      }
      __syncthreads();
    }
    // ---- pass 2: sum of expf(x - m), the order the header pins ----
    float s = 0.f;
    for (int it0 = 0; it0 < iters; it0 += UN) {
      float xs[UN];
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = (it0 + u) * LANES + tid;
        const int vc = v < V ? v : V - 1;
        float x = load_x<BF>(row, vc);
        if (MASK) x = x + a.vocab_mask[vc];
        xs[u] = x;
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
  }

  // ---- the K*K candidates: one wave, candidate c = k1*K + k2 ----
  const int KK = K * K;
  const int c = tid < KK ? tid : KK - 1;                 // (lanes behind the candidates compute the last one's and drop it)
  const int ck1 = c / K, ck2 = c - ck1 * K;
  const float slp = a.seq_lp[b * K + ck1];
  const int fin = a.finished[b * K + ck1] != 0;
  const int len = a.length[b * K + ck1] + (fin ? 0 : 1);
  const bool frozen = a.mode == GPV_BEAM_FREEZE && fin;
  const float lp = win_x[c] - lse_s[ck1];
  float score = slp + lp;
  if (t == 0 && ck1 > 0) score = -1e9f;
  if (frozen) score = slp;
  const int cw = frozen ? a.pad_id : win_v[c];
  const bool ok = tid < KK && (!frozen || ck2 == 0);
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
      sel_w[rank] = cw;
      sel_score[rank] = score;
      sel_fin[rank] = a.mode == GPV_BEAM_FREEZE ? (fin | (cw == a.stop_id ? 1 : 0)) : 0;
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
    int k1 = sel_k1[k];
    k1 = k1 < 0 ? 0 : (k1 >= K ? K - 1 : k1);          // (a NaN key can leave a slot unwritten: whatever LDS held stays in range)
    int w = sel_w[k];
    w = w < 0 ? 0 : (w >= V ? V - 1 : w);
    a.seqs[((int64_t)k * B + b) * T + p] = p < t ? rows_s[k1 * MAXT + p] : (int64_t)w;
  }
  if (tid < K) {
    int k1 = sel_k1[tid];
    k1 = k1 < 0 ? 0 : (k1 >= K ? K - 1 : k1);
    int w = sel_w[tid];
    w = w < 0 ? 0 : (w >= V ? V - 1 : w);
    a.parent[b * K + tid] = k1;
    a.seq_lp[b * K + tid] = sel_score[tid];
    a.finished[b * K + tid] = sel_fin[tid] != 0;
    a.length[b * K + tid] = sel_len[tid];
    a.tok[tid * B + b] = (int64_t)w;
  }
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));      // 16 bytes, one load / store each

template <int K>
__global__ __launch_bounds__(256) void reorder_kernel(gpv_beam_reorder_args a, int nvec, int row_vecs, int col0, int64_t total) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t gc = g < total ? g : total - 1;                     // clamped: the tail threads repeat the last item's loads, store nothing
  const int c = (int)(gc % nvec);
  int64_t q = gc / nvec;
  const int pos = (int)(q % a.upto);
  q /= a.upto;
  const int b = (int)(q % a.B);
  const int l = (int)(q / a.B);
  void* cache = a.cache[0];                                         // (a select chain: a run-time index would put the arguments in scratch)
#pragma unroll
  for (int i = 1; i < GPV_BEAM_MAX_LAYERS; ++i) cache = l == i ? a.cache[i] : cache;
  u32x4* base = reinterpret_cast<u32x4*>(cache);
  const int64_t off = (int64_t)pos * row_vecs + col0 + c;           // in 16-byte vectors inside one sequence's [T, 3D] block
  const int64_t seq_vecs = (int64_t)a.T * row_vecs;
  u32x4 val[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    int p = a.parent[b * K + k];
    p = p < 0 ? 0 : (p >= K ? K - 1 : p);
    val[k] = base[((int64_t)p * a.B + b) * seq_vecs + off];
  }
  if (g < total) {
#pragma unroll
    for (int k = 0; k < K; ++k) base[((int64_t)k * a.B + b) * seq_vecs + off] = val[k];
  }
}

}  // namespace

extern "C" int gpv_beam_step(const gpv_beam_args* a, void* stream) {
  if (!a || !a->logits || !a->lse || !a->seq_lp || !a->seqs || !a->tok || !a->parent || !a->finished || !a->length)
    return (int)hipErrorInvalidValue;
  if (a->B < 0 || a->K < 1 || a->K > MAXK || a->V < a->K || a->T < 2 || a->T > MAXT || a->t < 0 || a->t >= a->T - 1 || a->pitch < a->V)
    return (int)hipErrorInvalidValue;
  if (a->mode != GPV_BEAM_EXTEND && a->mode != GPV_BEAM_FREEZE) return (int)hipErrorInvalidValue;
  if (a->pad_id < 0 || a->pad_id >= a->V || a->stop_id < 0 || a->stop_id >= a->V) return (int)hipErrorInvalidValue;
  if (a->dtype != GPV_BEAM_BF16 && a->dtype != GPV_BEAM_F32) return (int)hipErrorInvalidValue;
  if ((int64_t)a->K * a->B > 0x7fffffff / 2 || a->V > (1 << 30)) return (int)hipErrorInvalidValue;   // (32-bit element indices in the kernel)
  if (a->B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a->B), block(LANES);
  const bool bf = a->dtype == GPV_BEAM_BF16, mask = a->vocab_mask != nullptr;
  if (bf && mask) step_kernel<true, true><<<grid, block, 0, st>>>(*a);
  else if (bf) step_kernel<true, false><<<grid, block, 0, st>>>(*a);
  else if (mask) step_kernel<false, true><<<grid, block, 0, st>>>(*a);
  else step_kernel<false, false><<<grid, block, 0, st>>>(*a);
  return (int)hipGetLastError();
}

extern "C" int gpv_beam_reorder(const gpv_beam_reorder_args* a, void* stream) {
  if (!a || !a->parent || a->L < 1 || a->L > GPV_BEAM_MAX_LAYERS || a->B < 0 || a->K < 1 || a->K > MAXK || a->T < 1 || a->D < 1 ||
      a->upto < 1 || a->upto > a->T)
    return (int)hipErrorInvalidValue;
  if (a->dtype != GPV_BEAM_BF16 && a->dtype != GPV_BEAM_F32) return (int)hipErrorInvalidValue;
  const int esz = a->dtype == GPV_BEAM_F32 ? 4 : 2;
  if (((int64_t)a->D * esz) % 16 != 0) return (int)hipErrorInvalidValue;
  for (int l = 0; l < a->L; ++l)
    if (!a->cache[l] || (reinterpret_cast<uintptr_t>(a->cache[l]) & 15)) return (int)hipErrorInvalidValue;
  if (a->B == 0) return 0;
  const int col0 = a->D * esz / 16, nvec = 2 * col0, row_vecs = 3 * col0;
  const int64_t total = (int64_t)a->L * a->B * a->upto * nvec;
  const int64_t blocks = (total + 255) / 256;
  if (blocks > 0x7fffffff) return (int)hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid((unsigned)blocks), block(256);
  switch (a->K) {                                                   // K registers of 16 bytes per thread: a compile-time count
    case 1: reorder_kernel<1><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    case 2: reorder_kernel<2><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    case 3: reorder_kernel<3><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    case 4: reorder_kernel<4><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    case 5: reorder_kernel<5><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    case 6: reorder_kernel<6><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    case 7: reorder_kernel<7><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
    default: reorder_kernel<8><<<grid, block, 0, st>>>(*a, nvec, row_vecs, col0, total); break;
  }
  return (int)hipGetLastError();
}
