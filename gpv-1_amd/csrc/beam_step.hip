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
//                   With a constraint on (no repeated n-gram, minimum length, repetition penalty: THE CONSTRAINTS of the header) the CONSTR
//                   instantiation runs instead: per row it marks the parent's history in a "seen" and the row's bans in a "banned" bitmap
//                   (LDS, V bits each, the touched words zeroed again behind the row), multiplies seen tokens on load in both passes,
//                   keeps banned tokens out of the lane lists and reduces m over the whole row.  With every constraint off the plain
//                   instantiations run, unchanged.
//   reorder_kernel  one thread per (layer, b, position, 16-byte vector of the k | v columns): K loads, then K stores.
// Mode GPV_BEAM_SAMPLE of gpv_beam_step (N draws per batch element in place of a beam) is sample_step.hip; the entry point below sends it there.
// Every load address is clamped into its array and the value padded at use; no loop bound depends on
// the data; a NaN anywhere can only change WHICH in-range index is written.
// -ffp-contract=off: every score, key and lp is one separately rounded fp32 operation.
#include "../../include/gpv_beam.h"

#pragma clang fp contract(off)
#include "beam_core.h"

namespace {

using namespace beam_core;
static_assert(sizeof(gpv_beam_args) == 176 && sizeof(gpv_beam_reorder_args) == 104, "ABI of include/gpv_beam.h");

// The bitmaps of the constrained step, V bits each, lane-major: token v = it * LANES + lane is bit (it & 31) of word (it >> 5) * LANES + lane,
// so a lane finds the bits of its own 32 next elements in ONE word (one LDS read per batch of UN loads, not one per element)
constexpr int BITW = GPV_BEAM_MAX_CONSTR_V / 32;
static_assert(32 % UN == 0 && BITW == (GPV_BEAM_MAX_CONSTR_V / LANES / 32) * LANES, "a batch of UN elements lies inside one word");
__device__ __forceinline__ int bit_word(int v) { return ((v / LANES) >> 5) * LANES + (v & (LANES - 1)); }
__device__ __forceinline__ unsigned bit_mask(int v) { return 1u << ((v / LANES) & 31); }
// the UN bits of the lane's batch that starts at iteration it0 (a multiple of UN), bit u in position u
__device__ __forceinline__ unsigned batch_bits(const unsigned* bits, int it0, int tid) { return bits[(it0 >> 5) * LANES + tid] >> (it0 & 31); }

// load_un, then step 1b of the rule on every value whose token the seen bitmap marks: one fp32 multiply (rep: the penalty is on)
template <bool BF, bool MASK>
__device__ __forceinline__ void load_un_rep(const void* row, const float* mask, int it0, int tid, int V, bool rep, const unsigned* seen,
                                            float rep_neg, float rep_pos, float (&xs)[UN]) {
  load_un<BF, MASK>(row, mask, it0, tid, V, xs);
  if (!rep) return;
  const unsigned sb = batch_bits(seen, it0, tid);                   // (an element behind V has no bit and is dropped at use anyway)
#pragma unroll
  for (int u = 0; u < UN; ++u) {
    const float x = xs[u];
    xs[u] = ((sb >> u) & 1u) ? (x < 0.f ? x * rep_neg : x * rep_pos) : x;
  }
}

// CONSTR: the instantiation that knows no_repeat / min_len / the repetition penalty (THE CONSTRAINTS of the header); without it
// the code is the plain step's
template <bool BF, bool MASK, bool CONSTR>
__global__ __launch_bounds__(LANES) void step_kernel(gpv_beam_args a) {
  __shared__ Shared sh;
  __shared__ int sel_fin[MAXK];
  __shared__ unsigned seen_s[CONSTR ? BITW : 1], ban_s[CONSTR ? BITW : 1];      // token v occurs in the history / is banned (bit_word, bit_mask)

  const int tid = threadIdx.x;
  const int b = blockIdx.x;
  const int B = a.B, K = a.K, V = a.V, t = a.t;
  const int iters = (V + LANES - 1) / LANES;
  const int ngram = a.no_repeat;
  const bool rep = CONSTR && a.rep_neg != 0.f;

  if constexpr (CONSTR) {
    // the K histories of this b (write_slots stages them again behind the selection) and two empty bitmaps
    for (int i = tid; i < K * t; i += LANES) {
      const int k = i / t, p = i - k * t;
      sh.rows_s[k * MAXT + p] = a.seqs[((int64_t)k * B + b) * a.T + p];
    }
    for (int i = tid; i < BITW; i += LANES) { seen_s[i] = 0u; ban_s[i] = 0u; }
    __syncthreads();
  }

  for (int k1 = 0; k1 < K; ++k1) {
    const int r = k1 * B + b;
    const void* row = row_ptr<BF>(a.logits, r, a.pitch);
    float m = 0.f;
    if constexpr (CONSTR) {
      // ---- the row's sets: thread p owns history position p (a frozen parent is exempt: its sets stay empty).  Every token is clamped
      //      into the vocabulary, t and ngram are uniform: no index leaves its array, no bound depends on the data ----
      const int64_t* h = &sh.rows_s[k1 * MAXT];
      const bool live = !(a.mode == GPV_BEAM_FREEZE && a.finished[b * K + k1] != 0);
      if (live) {
        for (int p = tid; p < t; p += LANES) {
          const int hp = clampi((int)h[p], 0, V - 1);
          if (rep) atomicOr(&seen_s[bit_word(hp)], bit_mask(hp));
          if (ngram >= 1 && p <= t - ngram) {                       // step 3a (i): i = p, the last n - 1 tokens against h[p : p+n-1]
            bool eq = true;
            for (int j = 0; j + 1 < ngram; ++j) eq = eq && h[p + j] == h[t - ngram + 1 + j];
            const int w = clampi((int)h[p + ngram - 1], 0, V - 1);
            if (eq) atomicOr(&ban_s[bit_word(w)], bit_mask(w));
          }
        }
        if (tid == 0 && a.length[b * K + k1] < a.min_len) atomicOr(&ban_s[bit_word(a.stop_id)], bit_mask(a.stop_id));      // step 3a (ii)
      }
      __syncthreads();
      // ---- pass 1: as below, banned tokens stay out of the lists; m is the maximum of the whole row, banned tokens included ----
      LaneList<false> list;
      list.clear();
      float mx = -INFINITY;
      for (int it0 = 0; it0 < iters; it0 += UN) {
        float xs[UN];
        load_un_rep<BF, MASK>(row, a.vocab_mask, it0, tid, V, rep, seen_s, a.rep_neg, a.rep_pos, xs);
        const unsigned bb = batch_bits(ban_s, it0, tid);
#pragma unroll
        for (int u = 0; u < UN; ++u) {
          const int v = (it0 + u) * LANES + tid;
          mx = fmaxf(mx, v < V ? xs[u] : -INFINITY);
          list.insert(K, v < V && !((bb >> u) & 1u) ? xs[u] : -INFINITY, v < V ? v : V - 1);
        }
      }
#pragma unroll
      for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
      if ((tid & 63) == 0) sh.red_v[tid >> 6] = mx;
      __syncthreads();
      m = sh.red_v[0];
#pragma unroll
      for (int w = 1; w < WAVES; ++w) m = fmaxf(m, sh.red_v[w]);
      __syncthreads();                                              // (pop_best writes red_v next)
      for (int k2 = 0; k2 < K; ++k2) {
        const Best best = pop_best(sh, tid, list.lv[0], list.li[0]);
        if (tid == 0) { sh.win_x[k1 * K + k2] = best.v; sh.win_v[k1 * K + k2] = best.i; }
        if (tid == best.lane) list.shift();
        __syncthreads();
      }
      // ---- pass 2: the row's lse in the pinned order, over the row as it stands after 1b ----
      row_sum_exp_of(sh, tid, [&](int it0, float (&xs)[UN]) {
        load_un_rep<BF, MASK>(row, a.vocab_mask, it0, tid, V, rep, seen_s, a.rep_neg, a.rep_pos, xs); }, m, V, k1, &a.lse[r]);
      // ---- undo: every bit set above lies in the word of a history token or of stop_id ----
      for (int p = tid; p < t; p += LANES) {
        const int w = bit_word(clampi((int)h[p], 0, V - 1));
        seen_s[w] = 0u;
        ban_s[w] = 0u;
      }
      if (tid == 0) ban_s[bit_word(a.stop_id)] = 0u;
      __syncthreads();
      continue;
    }
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
  if (a->mode == GPV_BEAM_SAMPLE) return launch_sample(a, stream);                              // THE SAMPLER of the header: sample_step.hip
  if (a->mode != GPV_BEAM_EXTEND && a->mode != GPV_BEAM_FREEZE) return (int)hipErrorInvalidValue;
  // the sampler's fields all zero is the step as it was; anything else in them is a caller's mistake
  if (a->seed || a->cand_v || a->cand_w || a->top_k != 0 || a->inv_temp != 0.f || a->top_p != 0.f) return (int)hipErrorInvalidValue;
  // the constraints: all four fields zero is off; the penalty's factors are both zero or both finite and positive
  const bool rep_off = a->rep_neg == 0.f && a->rep_pos == 0.f;
  const bool rep_on = a->rep_neg > 0.f && a->rep_pos > 0.f && isfinite(a->rep_neg) && isfinite(a->rep_pos);
  if (a->no_repeat < 0 || a->no_repeat > GPV_BEAM_MAX_NGRAM || a->min_len < 0 || a->min_len > a->T || !(rep_off || rep_on))
    return (int)hipErrorInvalidValue;
  const bool constr = a->no_repeat > 0 || a->min_len > 0 || rep_on;
  if (constr && a->V > GPV_BEAM_MAX_CONSTR_V) return (int)hipErrorInvalidValue;                 // (the two bitmaps of V bits)
  if (a->B == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 grid(a->B), block(LANES);
  const bool bf = a->dtype == GPV_BEAM_BF16, mask = a->vocab_mask != nullptr;
  if (constr) {
    if (bf && mask) step_kernel<true, true, true><<<grid, block, 0, st>>>(*a);
    else if (bf) step_kernel<true, false, true><<<grid, block, 0, st>>>(*a);
    else if (mask) step_kernel<false, true, true><<<grid, block, 0, st>>>(*a);
    else step_kernel<false, false, true><<<grid, block, 0, st>>>(*a);
  } else if (bf && mask) step_kernel<true, true, false><<<grid, block, 0, st>>>(*a);
  else if (bf) step_kernel<true, false, false><<<grid, block, 0, st>>>(*a);
  else if (mask) step_kernel<false, true, false><<<grid, block, 0, st>>>(*a);
  else step_kernel<false, false, false><<<grid, block, 0, st>>>(*a);
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
