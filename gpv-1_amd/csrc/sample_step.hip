// Mode GPV_BEAM_SAMPLE of gpv_beam_step: N = K draws per batch element in place of a beam (include/gpv_beam.h, THE SAMPLER; the host
// statement of the same rule is gpv1_amd.beam.sample_step_host).  One launch, one 256-thread workgroup per batch element b, built
// from beam_core.h like step_kernel.  For each slot k the workgroup walks row k*B+b
//   1 .. ceil(C / 8) times for the C = top_k candidates: a lane's sorted list holds MAXK = 8 entries and one lane can own more than
//                   eight of the row's top C (lane l owns v = l, l + 256, ...).  The workgroup pops the candidates one by one; when the
//                   owner of a pop has used up the eight entries its list was built with, every lane rebuilds its list from the
//                   elements that come strictly behind the last popped (x, v) in the order "x descending, v ascending".  At least
//                   eight pops lie between two rebuilds, so there are at most ceil(C / 8) scans (the loop over the pops has the fixed
//                   bound C; whether a pop is preceded by a scan is a workgroup-uniform branch); rows whose top C are spread over the
//                   lanes, the usual case, take one.
//   once more       for the sum of exponentials in the pinned order (row_sum_exp_of), m = the first pop.
// Threads j < C then form lp_j = x_j - lse and w_j = expf(lp_j) and write cand_v / cand_w; behind the last row thread k does the
// nucleus, the draw and the write of slot k on the at most 64 values of its row in LDS.  The parent is the identity: no reorder follows.
// Every load address is clamped into its array and the value padded at use; no loop bound depends on the data; a NaN anywhere can only
// change WHICH in-range index is written.
// -ffp-contract=off: every x, lp, c, tau and score is one separately rounded fp32 operation.
#include "../../include/gpv_beam.h"

#pragma clang fp contract(off)
#include "beam_core.h"

namespace {

using namespace beam_core;
constexpr int MAXC = GPV_BEAM_MAX_C;
constexpr int CROW = MAXC + 1;                 // row pitch of the candidate arrays in LDS: threads k = 0..K-1 read column j of K rows together
static_assert(sizeof(gpv_beam_args) == 176, "ABI of include/gpv_beam.h");
static_assert(MAXC <= LANES, "one thread per candidate");

// csrc/common.h hash_u32, restated (this library does not include common.h): lowbias32 finalizer on index ^ seed, high words folded in
__device__ __forceinline__ uint32_t hash_u32(uint64_t seed, uint64_t idx) {
  uint32_t x = (uint32_t)idx ^ (uint32_t)seed;
  x ^= ((uint32_t)(idx >> 32) ^ (uint32_t)(seed >> 32)) * 0x9E3779B9u;
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}

// load_un without the mask, then step 1 of the sampler: one fp32 multiply (inv_temp = 1.f is exact: no multiply), one fp32 add
template <bool BF, bool MASK>
__device__ __forceinline__ void load_un_temp(const void* row, const float* mask, float inv_temp, int it0, int tid, int V, float (&xs)[UN]) {
  load_un<BF, false>(row, nullptr, it0, tid, V, xs);
#pragma unroll
  for (int u = 0; u < UN; ++u) {
    const int v = (it0 + u) * LANES + tid;
    xs[u] = xs[u] * inv_temp;
    if (MASK) xs[u] = xs[u] + mask[v < V ? v : V - 1];
  }
}

template <bool BF, bool MASK>
__global__ __launch_bounds__(LANES) void sample_kernel(gpv_beam_args a) {
  __shared__ Shared sh;
  __shared__ float lp_s[MAXK * CROW], w_s[MAXK * CROW], c_s[MAXK * CROW];      // of candidate j of slot k, at k * CROW + j
  __shared__ int v_s[MAXK * CROW];
  __shared__ int sel_fin[MAXK];
  __shared__ int refill_s;                       // the owner of the last pop used up its list: every lane rebuilds before the next pop

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int B = a.B, K = a.K, V = a.V, C = a.top_k, t = a.t;
  const int iters = (V + LANES - 1) / LANES;
  const float inv_temp = a.inv_temp == 0.f ? 1.f : a.inv_temp;
  const int L = C < MAXK ? C : MAXK;             // entries of a lane's list

  for (int k = 0; k < K; ++k) {
    const int r = k * B + b;
    const void* row = row_ptr<BF>(a.logits, r, a.pitch);
    float m = 0.f;
    // ---- the candidates.  (lx, lv): the last popped pair; in front of the first pop every element is behind it.  A lane's list is
    //      rebuilt (one scan of the row, by every lane) only when some lane's list has run out: `taken` pops since it was built ----
    float lx = INFINITY;
    int lv = -1, taken = 0;
    bool refill = true;                                              // (uniform: every thread reads refill_s behind the same barrier)
    LaneList<false> list;
    for (int j = 0; j < C; ++j) {
      if (refill) {
        list.clear();
        for (int it0 = 0; it0 < iters; it0 += UN) {
          float xs[UN];
          load_un_temp<BF, MASK>(row, a.vocab_mask, inv_temp, it0, tid, V, xs);
#pragma unroll
          for (int u = 0; u < UN; ++u) {
            const int v = (it0 + u) * LANES + tid;
            const bool behind = v < V && beats(lx, lv, xs[u], v);
            list.insert(L, behind ? xs[u] : -INFINITY, v < V ? v : V - 1);
          }
        }
        taken = 0;
      }
      const Best best = pop_best(sh, tid, list.lv[0], list.li[0]);
      if (tid == 0) { lp_s[k * CROW + j] = best.v; v_s[k * CROW + j] = best.i; }
      if (j == 0) m = best.v;
      lx = best.v; lv = best.i;
      if (tid == best.lane) { list.shift(); refill_s = ++taken == L ? 1 : 0; }      // (every pop has exactly one owner: written every time)
      __syncthreads();
      refill = refill_s != 0;
    }
    // ---- the row's lse in the pinned order, over the row as it stands after step 1 ----
    row_sum_exp_of(sh, tid, [&](int it0, float (&xs)[UN]) { load_un_temp<BF, MASK>(row, a.vocab_mask, inv_temp, it0, tid, V, xs); },
                   m, V, k, &a.lse[r]);
    // ---- step 3: lp and w of candidate j (row_sum_exp_of ends behind a __syncthreads: lse_s and the pops are visible) ----
    if (tid < C) {
      const float lp = lp_s[k * CROW + tid] - sh.lse_s[k];
      const float w = expf(lp);
      lp_s[k * CROW + tid] = lp;
      w_s[k * CROW + tid] = w;
      a.cand_v[(int64_t)r * C + tid] = clampi(v_s[k * CROW + tid], 0, V - 1);
      a.cand_w[(int64_t)r * C + tid] = w;
    }
  }
  __syncthreads();

  // ---- steps 4 - 7: thread k owns slot k ----
  if (tid < K) {
    const int k = tid;
    const float* w = &w_s[k * CROW];
    float* c = &c_s[k * CROW];
    float acc = 0.f;
    int n = 1;
    for (int j = 0; j < C; ++j) {
      acc = acc + w[j];
      c[j] = acc;
      n += (a.top_p != 0.f && j < C - 1 && acc < a.top_p) ? 1 : 0;
    }
    if (a.top_p == 0.f) n = C;
    n = clampi(n, 1, C);
    const uint32_t bits = hash_u32(a.seed[0], ((uint64_t)t * (uint64_t)B + (uint64_t)b) * (uint64_t)K + (uint64_t)k);
    const float u = (float)(bits >> 8) * 0x1p-24f;                  // 24 bits: the conversion and the power of two are exact
    const float tau = u * c[n - 1];
    int js = n - 1;
    for (int j = C - 1; j >= 0; --j) js = (j < n && c[j] > tau) ? j : js;
    const float slp = a.seq_lp[b * K + k];
    const int fin = a.finished[b * K + k] != 0;
    const int tokv = fin ? a.pad_id : v_s[k * CROW + js];
    sh.sel_k1[k] = k;
    sh.sel_w[k] = tokv;
    sh.sel_score[k] = fin ? slp : slp + lp_s[k * CROW + js];
    sh.sel_len[k] = a.length[b * K + k] + (fin ? 0 : 1);
    sel_fin[k] = fin | (tokv == a.stop_id ? 1 : 0);
  }
  __syncthreads();
  write_slots(sh, a, tid, b);
  if (tid < K) a.finished[b * K + tid] = sel_fin[tid] != 0;
}

}  // namespace

// the checks and the launch of mode GPV_BEAM_SAMPLE (gpv_beam_step in beam_step.hip sends the mode here)
int beam_core::launch_sample(const gpv_beam_args* a, void* stream) {
  if (!check_step_common(a, a ? a->K : 1) || !a->finished || a->mode != GPV_BEAM_SAMPLE) return (int)hipErrorInvalidValue;
  if (!a->seed || !a->cand_v || !a->cand_w) return (int)hipErrorInvalidValue;
  if (a->top_k < 1 || a->top_k > MAXC || a->top_k > a->V) return (int)hipErrorInvalidValue;
  if (!(a->inv_temp == 0.f || (a->inv_temp > 0.f && isfinite(a->inv_temp)))) return (int)hipErrorInvalidValue;
  if (!(a->top_p == 0.f || (a->top_p > 0.f && a->top_p < 1.f))) return (int)hipErrorInvalidValue;
  // the beam's own rules are off in this mode
  if (a->inv_pen || a->no_repeat != 0 || a->min_len != 0 || a->rep_neg != 0.f || a->rep_pos != 0.f) return (int)hipErrorInvalidValue;
  if (a->B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a->B), block(LANES);
  const bool bf = a->dtype == GPV_BEAM_BF16, mask = a->vocab_mask != nullptr;
  if (bf && mask) sample_kernel<true, true><<<grid, block, 0, st>>>(*a);
  else if (bf) sample_kernel<true, false><<<grid, block, 0, st>>>(*a);
  else if (mask) sample_kernel<false, true><<<grid, block, 0, st>>>(*a);
  else sample_kernel<false, false><<<grid, block, 0, st>>>(*a);
  return (int)hipGetLastError();
}
