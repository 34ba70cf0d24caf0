// One phrase-constrained beam search step (include/gpv_phrase.h states the rule; the host statement of the same rule is
// gpv1_amd.phrases.phrase_step_host).  One launch, one 256-thread workgroup per batch element b; everything the step shares with
// beam_step.hip is beam_core.h.  For each parent k1 that is live and has allowed tokens the workgroup walks row k1*B+b twice over the
// WHOLE vocabulary -- the row maximum m, then the sum of expf(x - m) (beam_core.h row_sum_exp) -- and once over the node's allowed
// tokens: candidate i < cnt is the edge child_off[n] + i (token gathered through child_tok, logit gathered from the row, which the two
// passes have just pulled through the cache), candidate cnt is stop_id at a terminal node; lane l keeps a sorted top-K list over
// i = l, l + 256, ... (a node may have more children than the workgroup has lanes) and min(K, |A|) arg-max reductions pop the winners.
// The rows of DONE and VOID parents are not read.  Wave 0 then ranks the at most K*K candidates and the workgroup writes the K slots.
// Every load address is clamped into its array and the value padded at use: node into [0, M), edge into
// [0, E), token into [0, V).  Every loop bound is a shape or a clamped child_off difference.  A malformed trie or a NaN can only
// change WHICH in-range index is written.
// -ffp-contract=off: every score, key and lp is one separately rounded fp32 operation.
#include "../../include/gpv_phrase.h"

#pragma clang fp contract(off)
#include "beam_core.h"

namespace {

using namespace beam_core;
static_assert(sizeof(gpv_phrase_args) == 160, "ABI of include/gpv_phrase.h");
static_assert(GPV_PHRASE_LANES == GPV_BEAM_LANES && GPV_PHRASE_MAX_K == GPV_BEAM_MAX_K && GPV_PHRASE_MAX_T == GPV_BEAM_MAX_T &&
              GPV_PHRASE_BF16 == GPV_BEAM_BF16 && GPV_PHRASE_F32 == GPV_BEAM_F32, "the limits and codes of beam_core.h are gpv_beam.h's");

// waves_per_eu(1, 5): the grid is one workgroup (one wave per SIMD) per batch element, so occupancy buys nothing; squeezed into the
// 64 registers of 7 waves the row passes run 15 % slower (t = 1 of a search: 37.4 against 31.6 us, profiles/r18_beam_core.txt)
template <bool BF>
__global__ __launch_bounds__(LANES) __attribute__((amdgpu_waves_per_eu(1, 5))) void phrase_step_kernel(gpv_phrase_args a) {
  __shared__ Shared sh;
  __shared__ int win_e[MAXK * MAXK];          // a candidate's index among the node's allowed tokens (cnt: stop_id)
  __shared__ int win_ok[MAXK * MAXK];         // the candidate exists
  __shared__ int win_node[MAXK * MAXK], win_phr[MAXK * MAXK];
  __shared__ int done_s[MAXK];
  __shared__ int sel_node[MAXK], sel_phr[MAXK];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.x;
  const int B = a.B, K = a.K, V = a.V, t = a.t, M = a.M, E = a.E;
  const int iters = (V + LANES - 1) / LANES;

  if (tid < 64) win_ok[tid] = 0;
  if (tid < MAXK) {                            // a slot no candidate reaches is VOID
    sh.sel_k1[tid] = 0; sh.sel_w[tid] = a.pad_id; sh.sel_score[tid] = -1e9f; sel_node[tid] = GPV_PHRASE_VOID; sel_phr[tid] = -1; sh.sel_len[tid] = 0;
    done_s[tid] = 0; sh.lse_s[tid] = 0.f;
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
      win_ok[k1 * K] = 1; sh.win_v[k1 * K] = a.pad_id; sh.win_x[k1 * K] = 0.f;
      win_node[k1 * K] = GPV_PHRASE_DONE; win_phr[k1 * K] = a.phrase[b * K + k1];
      done_s[k1] = 1;
    }
    if (na == 0) {
      if (tid == 0) a.lse[r] = 0.f;
      continue;
    }
    const void* row = row_ptr<BF>(a.logits, r, a.pitch);
    // ---- pass 1: the row maximum (an element behind V repeats the last one: the maximum is the same) ----
    float m = -INFINITY;
    for (int it0 = 0; it0 < iters; it0 += UN) {
      float xs[UN];
      load_un<BF, false>(row, nullptr, it0, tid, V, xs);
#pragma unroll
      for (int u = 0; u < UN; ++u) m = fmaxf(m, xs[u]);
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) sh.red_v[wave] = m;
    __syncthreads();
    m = sh.red_v[0];
#pragma unroll
    for (int w = 1; w < WAVES; ++w) m = fmaxf(m, sh.red_v[w]);
    __syncthreads();
    // ---- pass 2: the row's lse ----
    row_sum_exp<BF, false>(sh, tid, row, nullptr, m, V, k1, &a.lse[r]);
    // ---- the lane's top-K list over its share of the allowed tokens ----
    LaneList<true> list;
    list.clear();
    const int giters = (na + LANES - 1) / LANES;
    for (int it = 0; it < giters; ++it) {
      const int i = it * LANES + tid;
      const int e = clampi(e0 + i, 0, E - 1);
      int v = i < cnt ? a.child_tok[e] : a.stop_id;
      v = clampi(v, 0, V - 1);
      const float x = load_x<BF>(row, v);
      list.insert(K, i < na ? x : -INFINITY, i < na ? v : NONE, i);
    }
    // ---- nk pops: the workgroup's best head, its owner records it and shifts its list ----
    for (int k2 = 0; k2 < nk; ++k2) {
      const Best best = pop_best(sh, tid, list.lv[0], list.li[0]);
      if (tid == best.lane) {
        const int c = k1 * K + k2;
        sh.win_x[c] = list.lv[0]; sh.win_v[c] = list.li[0]; win_e[c] = list.le[0];
        win_ok[c] = list.li[0] != NONE ? 1 : 0;                   // (a NaN logit never enters a list: the candidate is missing)
        list.shift();
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
  const float lp = sh.win_x[c] - sh.lse_s[ck1];
  float score = slp + lp;
  if (dn) score = slp;
  const int slot = select_by_rank(sh, tid, K, a.T, a.inv_pen, tid < KK && win_ok[c] != 0, ck1, sh.win_v[c], score, len);
  if (slot >= 0) { sel_node[slot] = win_node[c]; sel_phr[slot] = win_phr[c]; }
  write_slots(sh, a, tid, b);
  if (tid < K) { a.node[b * K + tid] = sel_node[tid]; a.phrase[b * K + tid] = sel_phr[tid]; }
}

}  // namespace

extern "C" int gpv_phrase_step(const gpv_phrase_args* a, void* stream) {
  if (!check_step_common(a, 1) || !a->node || !a->phrase || !a->child_off || !a->child_tok || !a->child_node || !a->terminal)
    return (int)hipErrorInvalidValue;
  if (a->M < 2 || a->E < 1 || a->E > (1 << 30) || a->M > (1 << 30)) return (int)hipErrorInvalidValue;
  if (a->B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a->B), block(LANES);
  if (a->dtype == GPV_PHRASE_BF16) phrase_step_kernel<true><<<grid, block, 0, st>>>(*a);
  else phrase_step_kernel<false><<<grid, block, 0, st>>>(*a);
  return (int)hipGetLastError();
}
