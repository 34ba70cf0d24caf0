// Shared device helpers for the gfx950 kernels (wave = 64 lanes, MFMA 16x16x32 bf16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>

typedef __bf16 bf16;
typedef bf16 __attribute__((ext_vector_type(8))) bf16x8;
typedef bf16 __attribute__((ext_vector_type(4))) bf16x4;
typedef bf16 __attribute__((ext_vector_type(2))) bf16x2;
typedef float __attribute__((ext_vector_type(4))) f32x4;

#include "host_defs.h"      // tune_env, al16, drop_thresh: what the host-only routing header shares with the kernels

#define GPV_CHECK_LAUNCH() \
  do {                     \
    hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) return (int)e_; \
  } while (0)

// XCD-aware work order: workgroup b runs on XCD b % 8 (observed dispatch rule, used for speed only).  Give every
// XCD a CONTIGUOUS range of tiles so that the column tiles of one row panel (same A rows / same conv pixels) share
// one L2 instead of being fetched from HBM once per XCD.  Bijective for any grid size: workgroup `bid` of `nwg` -> item.
// With a split reduction (gridDim.y > 1) the GEMM kernels remap the (tile, split) plane as a whole, split-major: an XCD then
// runs ALL tiles of one reduction slice together, so the slice's dy / x rows are fetched from HBM once and shared
// through that XCD's L2 (wgrad of a 1x1 conv has only 4..32 output tiles: tile-only remapping left every XCD
// with one tile and all slices, i.e. no sharing at all: TCC hit rate 0.6 %).
__device__ __forceinline__ int xcd_contiguous(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, loc = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + loc;
}

// Accumulator-order channel map of the kernels that finish their outputs in registers: LDS row (= staged weight row / output column) L of
// a 32-row group holds channel 8 (r / 4) + 4 jj + (r % 4), jj = L / 16 % 2, r = L % 16, so that the MFMA tiles 2 t, 2 t + 1 leave lane
// (row, g) with the 8 CONSECUTIVE channels 32 t + 8 g .. + 7 of its row: bias / residual / mask / output are plain 16-byte accesses.
// NH > 0: NH channels per register pass, pass h = L / NH keeps its own NH channels; NH = 0: one pass (L < its channel count)
template <int NH = 0>
__device__ __forceinline__ int acc_chan(int L) {
  int h = 0;
  if constexpr (NH != 0) h = L / NH;
  const int w = L - h * NH, j = w >> 4, r = w & 15;      // pass h, then MFMA tile j and row r inside it
  return h * NH + (j >> 1) * 32 + (r >> 2) * 8 + (j & 1) * 4 + (r & 3);
}

// (y > 0) of eight STORED bf16 values (four dwords) as one byte, bit e = element e -- as 16-bit integers: > 0 (a stored -0 or negative
// is not; what a later (float)mask > 0.f test sees) -- in 13 instructions: packed min(., 1) / max(., 0) leave 0 | 1 per half, a byte
// permute gathers four halves' low bytes, a 4 x 8-bit dot product with (1, 2, 4, 8) makes the nibble.
// Inline asm because of a hipcc 7.2 miscompile: written with __builtin_elementwise_min / max on short2 values the compiler
// derived all four words' flags from the FIRST word -- v_cmp_lt_i16 on elements 0 and 1 only, seen in the ISA -- and every byte came out
// as 0x00 / 55 / aa / ff.  A fix or a compiler upgrade has this one place to change.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t positive_bits8(u32x4 w) {
  const uint32_t one2 = 0x00010001u, zero2 = 0u;
  uint32_t m[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t tq;
    asm("v_pk_min_i16 %0, %1, %2" : "=v"(tq) : "v"(w[q]), "v"(one2));
    asm("v_pk_max_i16 %0, %1, %2" : "=v"(m[q]) : "v"(tq), "v"(zero2));
  }
  const uint32_t b03 = __builtin_amdgcn_perm(m[1], m[0], 0x06040200u);      // bytes (m0.b0, m0.b2, m1.b0, m1.b2) = elements 0..3
  const uint32_t b47 = __builtin_amdgcn_perm(m[3], m[2], 0x06040200u);
  return __builtin_amdgcn_udot4(b03, 0x08040201u, 0u, false) | (__builtin_amdgcn_udot4(b47, 0x08040201u, 0u, false) << 4);
}

__device__ __forceinline__ float bf2f(bf16 x) { return (float)x; }
__device__ __forceinline__ bf16 f2bf(float x) { return (bf16)x; }

// split an fp32 value into hi + lo bf16 (hi = RNE(x), lo = RNE(x - hi)): |x - hi - lo| <~ 2^-17 |x|
__device__ __forceinline__ void split_bf16(float x, bf16& hi, bf16& lo) {
  hi = (bf16)x;
  lo = (bf16)(x - (float)hi);
}

// D(16x16) += A(16x32, row = lane&15, k = 8*(lane>>4)..+7) * B(32x16, col = lane&15, same k)
// result: lane holds D[row = 4*(lane>>4)+i][col = lane&15], i = 0..3
__device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// counter-based RNG for dropout: one 32-bit hash per element index.  32-bit arithmetic only: the previous fmix64
// (three 64x64 multiplies = 12 quarter-rate v_mul_lo/hi_u32 per element) made every dropout consumer VALU-bound --
// the encoder attention kernels spent 54 % of their wave cycles issuing ~3700 VALU instructions per wave for 20 MFMAs
// (PMC, tools/pmc_attn.py), the FFN GEMM epilogue hashes 19.6 M elements per layer.  This is the 2-multiply
// "lowbias32" finalizer on (index low word ^ seed), the high words folded in with one more multiply.
__device__ __forceinline__ uint32_t hash_u32(uint64_t seed, uint64_t idx) {
  uint32_t x = (uint32_t)idx ^ (uint32_t)seed;
  x ^= ((uint32_t)(idx >> 32) ^ (uint32_t)(seed >> 32)) * 0x9E3779B9u;
  x ^= x >> 16; x *= 0x7feb352du;
  x ^= x >> 15; x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
// Dropout keep decisions come in PAIRS of consecutive flat element indices: one 32-bit mix per pair, 16 bits per element
// (drop probability = floor(p * 65536) / 65536), and only one quarter-rate 32-bit multiply per pair -- the rest is shifts, xors
// and full-rate 24-bit multiplies.  (Round 1 hashed the 64-bit index of every element with three 32-bit multiplies: the
// LayerNorm kernels and the K = 256 FFN GEMM epilogues spent more on the mask than on their arithmetic.)  Every consumer of an
// (seed, flat index) mask -- GEMM epilogues, LayerNorm forward / backward, gpv_dropout -- uses these, so a mask drawn by one
// kernel is the mask another one reconstructs.
__device__ __forceinline__ uint32_t drop_pair_bits(uint64_t seed, uint64_t pair) {
  uint32_t x = (uint32_t)pair * 0x9E3779B9u + (uint32_t)seed;
  x += ((uint32_t)(pair >> 32) ^ (uint32_t)(seed >> 32)) * 0x85EBCA6Bu;
  x ^= x >> 16; x = __umul24(x, 0x85EBCBu);
  x ^= x >> 13; x = __umul24(x, 0xC2B2AFu);
  x ^= x >> 16;
  return x;
}
// element kept iff its 16 bits >= p * 2^16
__device__ __forceinline__ bool drop_keep(uint64_t seed, uint64_t idx, uint32_t thresh) {
  const uint32_t w = drop_pair_bits(seed, idx >> 1);
  return ((idx & 1) ? (w >> 16) : (w & 0xffffu)) >= (thresh >> 16);
}
// keep bits of the N (4 or 8) consecutive elements base .. base+N-1 (bit e = element base + e); N/2 mixes when base is even
template <int N>
__device__ __forceinline__ uint32_t drop_mask(uint64_t seed, uint64_t base, uint32_t thresh) {
  const uint32_t t16 = thresh >> 16;
  uint32_t m = 0u;
  if ((base & 1) == 0) {
#pragma unroll
    for (int q = 0; q < N / 2; ++q) {
      const uint32_t w = drop_pair_bits(seed, (base >> 1) + q);
      m |= ((w & 0xffffu) >= t16 ? 1u : 0u) << (2 * q);
      m |= ((w >> 16) >= t16 ? 1u : 0u) << (2 * q + 1);
    }
  } else {
#pragma unroll
    for (int e = 0; e < N; ++e) m |= (drop_keep(seed, base + e, thresh) ? 1u : 0u) << e;
  }
  return m;
}
// Device-resident seed epoch (gpv_set_seed_device): when a caller replays captured launches (hipGraph) the `seed` argument of a
// launch is frozen in the graph; the effective seed of every dropout consumer is then seed ^ mix(*epoch), the caller bumps the
// word once per step, and the forward / backward launches of one step see the same value.  NULL = the seed argument as given.
namespace gpvk { extern const uint64_t* g_seed_dev; }
__device__ __forceinline__ uint64_t eff_seed(uint64_t seed, const uint64_t* epoch) {
  return epoch ? seed ^ (*epoch * 0x9E3779B97F4A7C15ull) : seed;
}

// Weights resident in LDS, staged once per workgroup (the streaming kernels): U 16-byte loads of every thread are issued before the
// first LDS store.  The plain `for (idx ...) lds[dst(idx)] = glob[src(idx)]` loop compiles to load -> s_waitcnt vmcnt(0) -> ds_write
// per iteration: 16 DEPENDENT L2 round trips for a 128 KB matrix on 512 threads -- 10-20 us at the head of every launch of
// conv1x1_stream / _chain / _dual, conv3x3_stream and stem_pool (seen in the ISA; the A-fragment prefetch shares the counter).
// Round 5: the loads are UNCONDITIONAL (a thread beyond the end re-reads the last chunk); only the LDS stores are predicated.  With a
// `if (idx < total)` around each load hipcc branched around every load and put `s_waitcnt vmcnt(0)` in front of the next one (seen in
// the ISA of every user): the "eight loads in flight" were eight -- sixteen for a 128 KB matrix -- dependent round trips, 16 K cycles
// (7 us, timed with s_memtime) at the head of every streaming launch.
template <int NTHR, int U, typename SrcF, typename DstF>
__device__ __forceinline__ void stage_chunks16(int total, int tid, SrcF src, DstF dst) {
  for (int base = 0; base < total; base += NTHR * U) {
    bf16x8 tmp[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * NTHR + tid;
      tmp[u] = *reinterpret_cast<const bf16x8*>(src(idx < total ? idx : total - 1));
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * NTHR + tid;
      if (idx < total) *reinterpret_cast<bf16x8*>(dst(idx)) = tmp[u];
    }
  }
}

__device__ __forceinline__ float gelu_erf(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

template <typename T> struct Ld8;   // load / store 8 consecutive elements as float[8]
template <> struct Ld8<bf16> {
  static __device__ __forceinline__ void ld(const bf16* p, float* o) {
    bf16x8 v = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
  }
  static __device__ __forceinline__ void st(bf16* p, const float* o) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16)o[i];
    *reinterpret_cast<bf16x8*>(p) = v;
  }
  // non-temporal forms (streaming: do not displace what the next kernels will read from L2 / MALL)
  static __device__ __forceinline__ void ld_nt(const bf16* p, float* o) {
    const bf16x8 v = __builtin_bit_cast(bf16x8, __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)));
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = (float)v[i];
  }
  static __device__ __forceinline__ void st_nt(bf16* p, const float* o) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16)o[i];
    __builtin_nontemporal_store(__builtin_bit_cast(u32x4, v), reinterpret_cast<u32x4*>(p));
  }
};
template <> struct Ld8<float> {
  static __device__ __forceinline__ void ld(const float* p, float* o) {
    float4 a = *reinterpret_cast<const float4*>(p);
    float4 b = *reinterpret_cast<const float4*>(p + 4);
    o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
  }
  static __device__ __forceinline__ void st(float* p, const float* o) {
    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
    *reinterpret_cast<float4*>(p + 4) = make_float4(o[4], o[5], o[6], o[7]);
  }
  static __device__ __forceinline__ void ld_nt(const float* p, float* o) { ld(p, o); }     // (fp32 outputs have no streaming launches)
  static __device__ __forceinline__ void st_nt(float* p, const float* o) { st(p, o); }
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}
