// One beam search step and the KV-cache reorder of all decoder layers (include/gpv_beam.h states the rule; the host statement of
// the same rule is gpv1_amd.beam.beam_step_host).  Two launches per decoded token instead of the torch glue of GPV._beam_device:
//   step_kernel     one 256-thread workgroup per batch element b; what it shares with phrase_step.hip (the list, the pops, the sum, the
//                   ranking, the slot write) is beam_core.h.  For each parent k1 the workgroup walks row k1*B+b twice:
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
#include "../../include/gpv_beam.h"

#pragma clang fp contract(off)
#include "beam_core.h"

namespace {

using namespace beam_core;
static_assert(sizeof(gpv_beam_args) == 128 && sizeof(gpv_beam_reorder_args) == 104, "ABI of include/gpv_beam.h");

template <bool BF, bool MASK>
__global__ __launch_bounds__(LANES) void step_kernel(gpv_beam_args a) {
  __shared__ Shared sh;
  __shared__ int sel_fin[MAXK];

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int B = a.B, K = a.K, V = a.V, t = a.t;
  const int iters = (V + LANES - 1) / LANES;

  for (int k1 = 0; k1 < K; ++k1) {
    const int r = k1 * B + b;
    const void* row = row_ptr<BF>(a.logits, r, a.pitch);
    // ---- pass 1: the lane's top-K list over v = tid, tid + 256, ... (an element behind V is -inf and never enters) ----
    LaneList<false> list;
    list.clear();
    for (int it0 = 0; it0 < iters; it0 += UN) {
      float xs[UN];
      load_un<BF, MASK>(row, a.vocab_mask, it0, tid, V, xs);
#pragma unroll
      for (int u = 0; u < UN; ++u) {
        const int v = (it0 + u) * LANES + tid;
        list.insert(K, v < V ? xs[u] : -INFINITY, v < V ? v : V - 1);
      }
    }
    // ---- K pops: the workgroup's best head, its owner shifts its list; the first is the row maximum ----
    float m = 0.f;
    for (int k2 = 0; k2 < K; ++k2) {
      const Best best = pop_best(sh, tid, list.lv[0], list.li[0]);
      if (tid == 0) { sh.win_x[k1 * K + k2] = best.v; sh.win_v[k1 * K + k2] = best.i; }
      if (k2 == 0) m = best.v;
      if (tid == best.lane) list.shift();
      __syncthreads();
    }
    // ---- pass 2: the row's lse ----
    row_sum_exp<BF, MASK>(sh, tid, row, a.vocab_mask, m, V, k1, &a.lse[r]);
  }

  // ---- the K*K candidates: one wave, candidate c = k1*K + k2 ----
  const int KK = K * K;
  const int c = tid < KK ? tid : KK - 1;                 // (lanes behind the candidates compute the last one's and drop it)
  const int ck1 = c / K, ck2 = c - ck1 * K;
  const float slp = a.seq_lp[b * K + ck1];
  const int fin = a.finished[b * K + ck1] != 0;
  const int len = a.length[b * K + ck1] + (fin ? 0 : 1);
  const bool frozen = a.mode == GPV_BEAM_FREEZE && fin;
  const float lp = sh.win_x[c] - sh.lse_s[ck1];
  float score = slp + lp;
  if (t == 0 && ck1 > 0) score = -1e9f;
  if (frozen) score = slp;
  const int cw = frozen ? a.pad_id : sh.win_v[c];
  const int slot = select_by_rank(sh, tid, K, a.T, a.inv_pen, tid < KK && (!frozen || ck2 == 0), ck1, cw, score, len);
  if (slot >= 0) sel_fin[slot] = a.mode == GPV_BEAM_FREEZE ? (fin | (cw == a.stop_id ? 1 : 0)) : 0;
  write_slots(sh, a, tid, b);
  if (tid < K) a.finished[b * K + tid] = sel_fin[tid] != 0;
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
  if (!check_step_common(a, a ? a->K : 1) || !a->finished) return (int)hipErrorInvalidValue;    // (K <= V: a row fills K list entries)
  if (a->mode != GPV_BEAM_EXTEND && a->mode != GPV_BEAM_FREEZE) return (int)hipErrorInvalidValue;
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
