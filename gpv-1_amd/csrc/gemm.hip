// MFMA bf16 GEMM / implicit-GEMM convolution for gfx950.
//
//   C[M,N] = epilogue( A[M,K] x B[N,K]^T )      256 threads = 4 waves (2x2), BMxBNx32 tiles,
//   register-staged double-buffered LDS, one barrier per k-tile, mfma_f32_16x16x32_bf16.
//
// Operand staging modes
//   A: PLAIN (k contiguous) | TRANS (reduction index is the slow dim; transposed through registers
//      on the way into LDS) | CONV (NHWC implicit-GEMM gather, forward or dgrad geometry)
//   B: PLAIN | TRANS | CONVT (wgrad: gathered activations, reduction = pixels)
// TIn = bf16 : operands are bf16 in HBM.
// TIn = float: "precise" mode, operands are fp32 in HBM and are split hi+lo bf16 while staged;
//              3 MFMAs per product (hi*hi + hi*lo + lo*hi) -> ~1e-6 relative error.
// The MFMA is issued with swapped operands (B fragment as the MFMA "A") so that a lane ends up
// holding 4 CONSECUTIVE columns of one C row -> 8/16-byte epilogue stores.
#include "gemm_common.h"
#include <cstdlib>

using namespace gpvk;

#ifndef GPV_PF
#define GPV_PF 2      /* register prefetch ring depth (tiles). Measured on the ResNet-50 conv shapes (tools/bench_conv.py): 1: 1968 us, 2: 1877 us, 3 (occupancy 3->2): 2136 us */
#endif

namespace {

// ---- 8 staged elements of one operand row -------------------------------------------------
template <typename T> struct Raw8;
__device__ __forceinline__ uint32_t bf_bits(float x) { return (uint32_t)__builtin_bit_cast(unsigned short, (bf16)x); }
template <> struct Raw8<bf16> {
  uint32_t w[4];   // 8 bf16 packed; kept as dwords so that element extraction stays in registers
  __device__ __forceinline__ void zero() { w[0] = w[1] = w[2] = w[3] = 0u; }
  __device__ __forceinline__ void load(const bf16* p) {
    uint4 t = *reinterpret_cast<const uint4*>(p);
    w[0] = t.x; w[1] = t.y; w[2] = t.z; w[3] = t.w;
  }
  __device__ __forceinline__ void load_n(const bf16* p, int n) {
    const unsigned short* q = reinterpret_cast<const unsigned short*>(p);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint32_t a = (2 * i < n) ? q[2 * i] : 0u, b = (2 * i + 1 < n) ? q[2 * i + 1] : 0u;
      w[i] = a | (b << 16);
    }
  }
  __device__ __forceinline__ uint32_t hi_bits(int i) const { return (w[i >> 1] >> ((i & 1) * 16)) & 0xffffu; }
  __device__ __forceinline__ float val(int i) const { return __builtin_bit_cast(float, (i & 1) ? (w[i >> 1] & 0xffff0000u) : (w[i >> 1] << 16)); }
  __device__ __forceinline__ uint32_t lo_bits(int) const { return 0u; }
  __device__ __forceinline__ void write(bf16* h, bf16*) const { *reinterpret_cast<uint4*>(h) = make_uint4(w[0], w[1], w[2], w[3]); }
};
template <> struct Raw8<float> {
  float v[8];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = 0.0f;
  }
  __device__ __forceinline__ void load(const float* p) {
    float4 a = *reinterpret_cast<const float4*>(p);
    float4 b = *reinterpret_cast<const float4*>(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
  }
  __device__ __forceinline__ void load_n(const float* p, int n) {
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = i < n ? p[i] : 0.0f;
  }
  __device__ __forceinline__ uint32_t hi_bits(int i) const { return bf_bits(v[i]); }
  __device__ __forceinline__ float val(int i) const { return v[i]; }
  __device__ __forceinline__ uint32_t lo_bits(int i) const { return bf_bits(v[i] - (float)(bf16)v[i]); }
  __device__ __forceinline__ void write(bf16* h, bf16* l) const {
    uint32_t a[4], b[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = hi_bits(2 * i) | (hi_bits(2 * i + 1) << 16);
      b[i] = lo_bits(2 * i) | (lo_bits(2 * i + 1) << 16);
    }
    *reinterpret_cast<uint4*>(h) = make_uint4(a[0], a[1], a[2], a[3]);
    *reinterpret_cast<uint4*>(l) = make_uint4(b[0], b[1], b[2], b[3]);
  }
};

// masking helpers (branch-free: select after an unconditional load from a safe address)
template <typename T> __device__ __forceinline__ void mask_raw(Raw8<T>& r, bool ok);
template <> __device__ __forceinline__ void mask_raw<bf16>(Raw8<bf16>& r, bool ok) {
  const uint32_t m = ok ? 0xffffffffu : 0u;
  r.w[0] &= m; r.w[1] &= m; r.w[2] &= m; r.w[3] &= m;
}
template <> __device__ __forceinline__ void mask_raw<float>(Raw8<float>& r, bool ok) {
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = ok ? r.v[i] : 0.0f;
}

// ---- K-contiguous operand (PLAIN or CONV gather): tile [ROWS][32] -------------------------
template <typename T, int ROWS, int MODE, bool VEC>
struct KStage {
  static constexpr int NIT = ROWS / 64;
  struct Buf { Raw8<T> raw[NIT]; bool okf[NIT]; };
  // bf16 16-byte path of the plain operand: buffer loads -- the per-lane byte offset is fixed for the tile (row * ld + slot),
  // the k-tile offset rides in the scalar soffset, rows beyond the operand get an out-of-range offset = hardware zeros
  // (no 64-bit address add, no safe-address select per load, no zero-masking pass before the LDS write)
  static constexpr bool BUF = VEC && MODE == OP_PLAIN && sizeof(T) == 2;
  static constexpr int OOB = 0x7ffffff0;
  const T* base[NIT];
  const T* safe;
  int oh[NIT], ow[NIT];
  bool rowok[NIT];
  __amdgpu_buffer_rsrc_t rs;
  int vo[NIT];

  __device__ __forceinline__ void init(const T* ptr, int64_t ld, int row0, int nrows, int k_begin, const ConvGeom& g) {
    const int tid = threadIdx.x;
    safe = ptr;
    if constexpr (BUF) {
      rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(ptr), (short)0, OOB, 0x00020000);
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int row = (tid + it * 256) >> 2, slot = (tid + it * 256) & 3;
        vo[it] = row0 + row < nrows ? ((row0 + row) * (int)ld + slot * 8) * 2 : OOB;
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      int row = (tid + it * 256) >> 2;
      int r = row0 + row;
      rowok[it] = r < nrows;
      if (MODE == OP_CONV) {
        int rr = conv_row_to_pixel(rowok[it] ? r : 0, g);
        int b = rr / (g.OH * g.OW);
        int rem = rr - b * (g.OH * g.OW);
        oh[it] = rem / g.OW;
        ow[it] = rem - oh[it] * g.OW;
        base[it] = ptr + (int64_t)b * g.IH * g.IW * g.Cs;
      } else {
        base[it] = ptr + (int64_t)(rowok[it] ? r : 0) * ld;
        oh[it] = ow[it] = 0;
      }
    }
  }
  __device__ __forceinline__ void load(int k0, int K, const ConvGeom& g, Buf& bf) {
    Raw8<T>(&raw)[NIT] = bf.raw; bool(&okf)[NIT] = bf.okf;
    const int tid = threadIdx.x;
    if constexpr (BUF) {
      const bool full = k0 + BK <= K;                      // uniform; K % 8 == 0 or finite padding (host): whole chunks
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int slot = (tid + it * 256) & 3;
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, (full || k0 + slot * 8 < K) ? vo[it] : OOB, k0 * 2, 0);
        raw[it].w[0] = t[0]; raw[it].w[1] = t[1]; raw[it].w[2] = t[2]; raw[it].w[3] = t[3];
        okf[it] = true;
      }
      return;
    }
    int tr = 0, ts = 0, c0 = k0;
    if (MODE == OP_CONV) {
      int tap = k0 / g.Cin;
      c0 = k0 - tap * g.Cin;
      tr = tap / g.KW;
      ts = tap - tr * g.KW;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      int slot = (tid + it * 256) & 3;
      int k = k0 + slot * 8;
      bool ok = rowok[it] && k < K;
      const T* p;
      if (MODE == OP_CONV) {
        int ih, iw;
        if (g.dgrad) {                       // strides are 1 or 2 (checked on the host)
          int th = oh[it] + g.PH - tr, tw = ow[it] + g.PW - ts;
          int sh = g.SH - 1, sw = g.SW - 1;  // shift amount == mask for stride in {1,2}
          ih = th >> sh; iw = tw >> sw;
          ok = ok && th >= 0 && tw >= 0 && ((th & sh) == 0) && ((tw & sw) == 0) && ih < g.IH && iw < g.IW;
        } else {
          ih = oh[it] * g.SH + tr - g.PH; iw = ow[it] * g.SW + ts - g.PW;
          ok = ok && ih >= 0 && iw >= 0 && ih < g.IH && iw < g.IW;
        }
        p = base[it] + ((int64_t)(ih * g.IW + iw)) * g.Cs + c0 + slot * 8;
      } else {
        p = base[it] + k;
      }
      if (VEC) {
        // unconditional 16-B load (from a safe address when masked); the zero-select is applied in
        // store(), AFTER the MFMAs of the current tile, so the load latency overlaps the math
        raw[it].load(ok ? p : safe);
        okf[it] = ok;
      } else {
        if (!ok) raw[it].zero();
        else raw[it].load_n(p, K - k);
      }
    }
  }
  __device__ __forceinline__ void store(bf16* hi, bf16* lo, bool, Buf& bf) {
    Raw8<T>(&raw)[NIT] = bf.raw; bool(&okf)[NIT] = bf.okf;
    const int tid = threadIdx.x;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      int i = tid + it * 256;
      int off = (i >> 2) * LDK + (i & 3) * 8;
      if (VEC) mask_raw<T>(raw[it], okf[it]);
      raw[it].write(hi + off, lo + off);
    }
  }
};

// ---- reduction-major operand (TRANS, or CONVT gather): memory tile [32 red][COLS] -------------------------
// Staged ROW-MAJOR exactly as it is loaded (16-B global loads, conflict-free ds_write_b128, pitch COLS+16), and
// consumed with the gfx950 LDS transpose read: one ds_read_b64_tr_b16 gives a lane 4 consecutive reduction rows of
// ITS column (verified on hardware by tools/probe/trread.hip); two of them = one 16x16x32 MFMA operand fragment.
template <typename T, int COLS, int MODE, bool VEC, bool SUM = false>
struct TStage {
  static constexpr int CHK = COLS / 8;            // 16-B chunks per reduction row
  static constexpr int NIT = (BK * CHK) / 256;    // chunks per thread
  static constexpr int PITCH = COLS + 16;         // elements; (PITCH/2) % 64 in {8, 40}: 8 rows hit distinct bank octets
  struct Buf { Raw8<T> raw[NIT]; bool okf[NIT]; };
  static constexpr bool BUF = VEC && MODE == OP_PLAIN && sizeof(T) == 2;    // see KStage
  static constexpr int OOB = 0x7ffffff0;
  __amdgpu_buffer_rsrc_t rs;
  int vo[NIT];
  const T* ptr; int64_t ld; int col0, ncols;
  int tap_r, tap_s, c0;
  int pb[NIT], poh[NIT], pow_[NIT];      // CONVT: (batch, oh, ow) of this thread's reduction rows, advanced per k-tile
  float csum[SUM ? NIT : 1][8];          // SUM: running sum over the reduction of this thread's 8 columns (bias gradient)
  bool do_sum;

  __device__ __forceinline__ void init(const T* p, int64_t ld_, int col0_, int ncols_, int k_begin, const ConvGeom& g) {
    ptr = p; ld = ld_; col0 = col0_; ncols = ncols_;
    tap_r = tap_s = c0 = 0;
    do_sum = false;
    if constexpr (BUF) {
      rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(p), (short)0, OOB, 0x00020000);
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int idx = threadIdx.x + it * 256;
        const int kr = idx / CHK, ch = idx - kr * CHK;
        vo[it] = col0 + ch * 8 < ncols ? (kr * (int)ld + col0 + ch * 8) * 2 : OOB;
      }
    }
    if constexpr (SUM) {
#pragma unroll
      for (int it = 0; it < NIT; ++it)
#pragma unroll
        for (int e = 0; e < 8; ++e) csum[it][e] = 0.f;
    }
    if (MODE == OP_CONV) {
      int tap = col0 / g.Cin;
      c0 = col0 - tap * g.Cin;
      tap_r = tap / g.KW;
      tap_s = tap - tap_r * g.KW;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        int k = k_begin + (threadIdx.x + it * 256) / CHK;
        pb[it] = k / (g.OH * g.OW);
        int rem = k - pb[it] * (g.OH * g.OW);
        poh[it] = rem / g.OW;
        pow_[it] = rem - poh[it] * g.OW;
      }
    }
  }
  __device__ __forceinline__ void load(int k0, int K, const ConvGeom& g, Buf& bf) {
    Raw8<T>(&raw)[NIT] = bf.raw; bool(&okf)[NIT] = bf.okf;
    if constexpr (BUF) {
      const bool full = k0 + BK <= K;                      // uniform
      const int soff = k0 * (int)ld * 2;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int kr = (threadIdx.x + it * 256) / CHK;
        const u32x4 t = __builtin_amdgcn_raw_buffer_load_b128(rs, (full || k0 + kr < K) ? vo[it] : OOB, soff, 0);
        raw[it].w[0] = t[0]; raw[it].w[1] = t[1]; raw[it].w[2] = t[2]; raw[it].w[3] = t[3];
        okf[it] = true;
      }
      return;
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = threadIdx.x + it * 256;
      const int kr = idx / CHK, ch = idx - kr * CHK;
      const int k = k0 + kr, col = col0 + ch * 8;
      bool ok = k < K && col < ncols;
      const T* src;
      if (MODE == OP_CONV) {
        int ih = poh[it] * g.SH + tap_r - g.PH, iw = pow_[it] * g.SW + tap_s - g.PW;
        ok = ok && ih >= 0 && iw >= 0 && ih < g.IH && iw < g.IW;
        src = ptr + ((int64_t)((pb[it] * g.IH + ih) * g.IW + iw)) * g.Cs + c0 + ch * 8;
        pow_[it] += BK;                           // advance this reduction row by BK pixels for the next k-tile
        while (pow_[it] >= g.OW) { pow_[it] -= g.OW; poh[it] += 1; }
        while (poh[it] >= g.OH) { poh[it] -= g.OH; pb[it] += 1; }
      } else {
        src = ptr + (int64_t)k * ld + col;
      }
      if (VEC) {                                  // host guarantees ncols % 8 == 0 for the VEC variant
        raw[it].load(ok ? src : ptr);
        okf[it] = ok;
      } else {
        if (!ok) raw[it].zero();
        else raw[it].load_n(src, ncols - col);
      }
    }
  }
  __device__ __forceinline__ void store(bf16* hi, bf16* lo, bool, Buf& bf) {
    Raw8<T>(&raw)[NIT] = bf.raw; bool(&okf)[NIT] = bf.okf;
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = threadIdx.x + it * 256;
      const int kr = idx / CHK, ch = idx - kr * CHK;
      if (VEC) mask_raw<T>(raw[it], okf[it]);
      if constexpr (SUM) {
        if (do_sum) {
#pragma unroll
          for (int e = 0; e < 8; ++e) csum[it][e] += raw[it].val(e);
        }
      }
      raw[it].write(hi + kr * PITCH + ch * 8, lo + kr * PITCH + ch * 8);
    }
  }
  // SUM: add this block's column sums (over its reduction range) to out[col0 + c]; threads with equal column chunk
  // are reduced with lane shuffles first, then one atomic per column and wave
  __device__ __forceinline__ void flush_sums(float* out) {
    if constexpr (SUM) {
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int ch = (threadIdx.x + it * 256) % CHK;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = csum[it][e];
#pragma unroll
          for (int s = CHK; s < 64; s <<= 1) v += __shfl_xor(v, s);
          const int col = col0 + ch * 8 + e;
          if ((threadIdx.x & 63) < CHK && col < ncols) atomicAdd(out + col, v);
        }
      }
    }
  }
  // fragment for the 16 columns starting at `cbase` of the staged tile: lane (col = lane&15, g = lane>>4) receives
  // reduction rows 8g..8g+7
  static __device__ __forceinline__ bf16x8 frag(const bf16* tile, int cbase, int lane) {
    typedef short __attribute__((ext_vector_type(4))) s16x4;
    typedef __attribute__((address_space(3))) s16x4 lds_s16x4;
    const int g = lane >> 4, i = lane & 15;
    const bf16* p0 = tile + (8 * g + (i >> 2)) * PITCH + cbase + (i & 3) * 4;
    s16x4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0));
    s16x4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4*)(p0 + 4 * PITCH));
    typedef short __attribute__((ext_vector_type(8))) s16x8;
    s16x8 r = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    return __builtin_bit_cast(bf16x8, r);
  }
};

template <typename TIn, typename TOut, int AMODE, int BMODE, int BM, int BN, bool VEC, bool NTIO = false>
__device__ __forceinline__ void gemm_body(const GemmK& p) {
  constexpr bool PRECISE = sizeof(TIn) == 4;
  constexpr int FM = BM / 32, FN = BN / 32;
  constexpr int A_ELEMS = BM * LDK, B_ELEMS = BN * LDK;
  constexpr int STAGE_ELEMS = (A_ELEMS + B_ELEMS) * (PRECISE ? 2 : 1);
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  bf16* smem = reinterpret_cast<bf16*>(smem_raw);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  // XCD-aware tile order (common.h xcd_contiguous); with a split reduction the (tile, split) plane is remapped as a whole, split-major
  int tile, ksplit;
  {
    const bool plane = gridDim.z == 1;
    const int gx = gridDim.x;
    const int nwg = plane ? gx * (int)gridDim.y : gx, bid = plane ? (int)blockIdx.x + gx * (int)blockIdx.y : (int)blockIdx.x;
    const int v = xcd_contiguous(bid, nwg);
    ksplit = plane ? v / gx : (int)blockIdx.y;
    tile = plane ? v - ksplit * gx : v;
  }
  int tm = tile / p.tilesN;
  const int tn = tile - tm * p.tilesN;
  if constexpr (AMODE == OP_CONV) {
    // parity-class-major dgrad: the four classes have different tap counts (0..4 taps); cycle the classes
    // through consecutive row panels so every XCD's contiguous tile range gets the same mix of work
    if (p.cg.cm && p.cg.cls_rows % BM == 0 && p.M == 4 * p.cg.cls_rows) {
      const int tpc = p.cg.cls_rows / BM;
      tm = (tm & 3) * tpc + (tm >> 2);
    }
  }
  const int row0 = tm * BM, col0 = tn * BN;
  const int batch = blockIdx.z;

  int kt_total = (p.K + BK - 1) / BK;
  // stride-2 dgrad with parity-class-major rows: a class-uniform tile only visits its own taps
  int cm_r0 = 0, cm_s0 = 0, cm_nS = 1, cm_cpt = 1;
  bool cm_on = false, cm_empty = false;
  __shared__ int s_rowpix[AMODE == OP_CONV ? BM : 1];   // class-major row -> output pixel (divisions done once per tile row)
  if constexpr (AMODE == OP_CONV) {
    if (p.cg.cm && threadIdx.x < BM) s_rowpix[threadIdx.x] = conv_row_to_pixel(min(row0 + (int)threadIdx.x, p.M - 1), p.cg);
  }
  if constexpr (AMODE == OP_CONV) {
    if (p.cg.cm) {
      const int c_lo = row0 / p.cg.cls_rows, c_hi = min(row0 + BM - 1, p.M - 1) / p.cg.cls_rows;
      if (c_lo == c_hi) {
        cm_on = true;
        cm_r0 = ((c_lo >> 1) + p.cg.PH) & 1;
        cm_s0 = ((c_lo & 1) + p.cg.PW) & 1;
        const int nR = (p.cg.KH - cm_r0 + 1) / 2;
        cm_nS = (p.cg.KW - cm_s0 + 1) / 2;
        cm_cpt = p.cg.Cin / BK;
        kt_total = nR * cm_nS * cm_cpt;
        if (kt_total == 0) { cm_empty = true; kt_total = 1; }   // no tap reaches this class: one fully masked k-tile, dx = res * mask
      }
    }
  }
  auto kmap = [&](int kt) -> int {      // k-tile index -> offset on the full [taps x Cin] reduction axis
    if (!cm_on) return kt * BK;
    if (cm_empty) return p.K;
    const int t = kt / cm_cpt, c = kt - t * cm_cpt;
    const int ri = t / cm_nS, si = t - ri * cm_nS;
    return ((cm_r0 + 2 * ri) * p.cg.KW + cm_s0 + 2 * si) * p.cg.Cin + c * BK;
  };
  const int kt0 = ksplit * p.kt_per_split;
  const int kt1 = min(kt_total, kt0 + p.kt_per_split);
  if (kt0 >= kt1) return;

  const TIn* Ap = reinterpret_cast<const TIn*>(p.A) + (int64_t)batch * p.sA;
  const TIn* Bp = reinterpret_cast<const TIn*>(p.B) + (int64_t)batch * p.sB;

  constexpr bool ASUM = AMODE == OP_TRANS && BMODE == OP_TRANS;     // linear wgrad: bias gradient = row sums of A (= dY^T)
  typedef typename std::conditional<AMODE == OP_TRANS, TStage<TIn, BM, OP_PLAIN, VEC, ASUM>, KStage<TIn, BM, AMODE, VEC>>::type AStage;
  typedef typename std::conditional<BMODE == OP_PLAIN, KStage<TIn, BN, OP_PLAIN, VEC>,
                                    TStage<TIn, BN, (BMODE == OP_CONV ? OP_CONV : OP_PLAIN), VEC>>::type BStage;
  AStage as; BStage bs;
  as.init(Ap, p.lda, row0, p.M, kt0 * BK, p.cg);
  if constexpr (ASUM) as.do_sum = p.a_rowsum != nullptr && tn == 0;
  bs.init(Bp, p.ldb, col0, p.N, kt0 * BK, p.cg);

  auto stage_ptr = [&](int s, int which) -> bf16* {  // which: 0 Ahi 1 Alo 2 Bhi 3 Blo
    bf16* b = smem + s * STAGE_ELEMS;
    if (PRECISE) {
      switch (which) { case 0: return b; case 1: return b + A_ELEMS; case 2: return b + 2 * A_ELEMS; default: return b + 2 * A_ELEMS + B_ELEMS; }
    }
    return which < 2 ? b : b + A_ELEMS;
  };
  // register prefetch ring, PF tiles deep: the global loads of tile t+PF-1 are issued while tile t is being
  // multiplied, so a load has PF-1 whole iterations (not one) to come back before its ds_write needs it.
  constexpr int PF = GPV_PF;
  typename AStage::Buf abuf[PF];
  typename BStage::Buf bbuf[PF];

  f32x4 acc[FM][FN];
#pragma unroll
  for (int i = 0; i < FM; ++i)
#pragma unroll
    for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

#pragma unroll
  for (int d = 0; d < PF - 1; ++d) {
    if (kt0 + d < kt1) {
      as.load(kmap(kt0 + d), p.K, p.cg, abuf[d]);
      bs.load(kmap(kt0 + d), p.K, p.cg, bbuf[d]);
    }
  }
  as.store(stage_ptr(0, 0), stage_ptr(0, 1), PRECISE, abuf[0]);
  bs.store(stage_ptr(0, 2), stage_ptr(0, 3), PRECISE, bbuf[0]);
  __syncthreads();

  int cur = 0;
  const int a_off = (wm * (BM / 2) + (lane & 15)) * LDK + (lane >> 4) * 8;
  const int b_off = (wn * (BN / 2) + (lane & 15)) * LDK + (lane >> 4) * 8;
  auto compute = [&](int st) {
    bf16x8 af[FM], bfr[FN];
    const bf16* At = stage_ptr(st, 0);
    const bf16* Bt = stage_ptr(st, 2);
#pragma unroll
    for (int i = 0; i < FM; ++i) {
      if constexpr (AMODE == OP_TRANS) af[i] = AStage::frag(At, wm * (BM / 2) + i * 16, lane);
      else af[i] = *reinterpret_cast<const bf16x8*>(At + a_off + i * 16 * LDK);
    }
#pragma unroll
    for (int j = 0; j < FN; ++j) {
      if constexpr (BMODE != OP_PLAIN) bfr[j] = BStage::frag(Bt, wn * (BN / 2) + j * 16, lane);
      else bfr[j] = *reinterpret_cast<const bf16x8*>(Bt + b_off + j * 16 * LDK);
    }
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
      for (int j = 0; j < FN; ++j) acc[i][j] = mfma16(bfr[j], af[i], acc[i][j]);
    if constexpr (PRECISE) {
      const bf16* Alt = stage_ptr(st, 1);
      const bf16* Blt = stage_ptr(st, 3);
      bf16x8 al[FM], bl[FN];
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        if constexpr (AMODE == OP_TRANS) al[i] = AStage::frag(Alt, wm * (BM / 2) + i * 16, lane);
        else al[i] = *reinterpret_cast<const bf16x8*>(Alt + a_off + i * 16 * LDK);
      }
#pragma unroll
      for (int j = 0; j < FN; ++j) {
        if constexpr (BMODE != OP_PLAIN) bl[j] = BStage::frag(Blt, wn * (BN / 2) + j * 16, lane);
        else bl[j] = *reinterpret_cast<const bf16x8*>(Blt + b_off + j * 16 * LDK);
      }
#pragma unroll
      for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          acc[i][j] = mfma16(bl[j], af[i], acc[i][j]);
          acc[i][j] = mfma16(bfr[j], al[i], acc[i][j]);
        }
    }
  };
  for (int kt = kt0; kt < kt1; kt += PF) {
#pragma unroll
    for (int d = 0; d < PF; ++d) {       // statically indexed ring slots (runtime indices would spill to scratch)
      const int t = kt + d;
      if (t < kt1) {
        if (t + PF - 1 < kt1) {
          as.load(kmap(t + PF - 1), p.K, p.cg, abuf[(d + PF - 1) % PF]);
          bs.load(kmap(t + PF - 1), p.K, p.cg, bbuf[(d + PF - 1) % PF]);
        }
        compute(cur);
        if (t + 1 < kt1) {
          as.store(stage_ptr(cur ^ 1, 0), stage_ptr(cur ^ 1, 1), PRECISE, abuf[(d + 1) % PF]);
          bs.store(stage_ptr(cur ^ 1, 2), stage_ptr(cur ^ 1, 3), PRECISE, bbuf[(d + 1) % PF]);
        }
        __syncthreads();
        cur ^= 1;
      }
    }
  }

  TOut* Cp = reinterpret_cast<TOut*>(p.C) + (int64_t)batch * p.sC;
  int64_t ldc = p.ldc;
  if (p.ws != nullptr) {            // split reduction through a workspace: this split's partial product is a dense [M,N] slab
    Cp = reinterpret_cast<TOut*>(p.ws) + (int64_t)ksplit * p.M * p.N;
    ldc = p.N;
  }
  const TOut* Rp = p.res ? reinterpret_cast<const TOut*>(p.res) + (int64_t)batch * p.sR : nullptr;
  const TOut* Mp = reinterpret_cast<const TOut*>(p.mask);

  if constexpr (ASUM) {
    if (as.do_sum) as.flush_sums(p.a_rowsum);
  }
  if (p.accumulate) {
    // ---------------- split-K / accumulate epilogue: fp32 atomics straight from the fragments ----------------
    if constexpr (sizeof(TOut) == 4) {
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int m = row0 + wm * (BM / 2) + i * 16 + (lane & 15);
        if (m >= p.M) continue;
        const float rs = p.rowscale ? p.rowscale[m] * p.alpha : p.alpha;
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int n = col0 + wn * (BN / 2) + j * 16 + (lane >> 4) * 4;
          float* dst = reinterpret_cast<float*>(Cp) + (int64_t)m * ldc + n;
#pragma unroll
          for (int r = 0; r < 4; ++r)
            if (n + r < p.N) atomicAdd(dst + r, acc[i][j][r] * rs);
        }
      }
    }
    return;
  }

  // ---------------- coalesced epilogue: fragments -> LDS (fp32, half a tile at a time) -> full rows ----------------
  // (a lane holds 4 consecutive columns of 16 different rows; writing that straight to HBM gives 32-byte
  //  row segments.  Through LDS every wave-store instruction covers whole 128/256-byte row runs.)
  float* ep = reinterpret_cast<float*>(smem_raw);
  constexpr int EPITCH = BN + 4;
  constexpr int HR = BM / 2;
  constexpr int CH = BN / 8;
  constexpr int NCH = (HR * CH) / 256;
  const bool v_st = (ldc % 8 == 0) && ((reinterpret_cast<uintptr_t>(Cp) & 15) == 0);
  const bool v_res = Rp && (p.ldr % 8 == 0) && ((reinterpret_cast<uintptr_t>(Rp) & 15) == 0);
  const bool v_msk = Mp && (p.ldm % 8 == 0) && ((reinterpret_cast<uintptr_t>(Mp) & 15) == 0);
  // every chunk this thread finishes covers the SAME 8 columns (256 % CH == 0): fetch their bias once
  // (per-element bias loads inside the readback loop cost more than the whole GEMM on the K=64 convs)
  float bv[8];
  {
    const int nb = col0 + (tid % CH) * 8;
    const bool vb = p.bias && nb + 8 <= p.N && ((reinterpret_cast<uintptr_t>(p.bias) & 15) == 0);
    if (vb) {
      const float4 b0 = *reinterpret_cast<const float4*>(p.bias + nb);
      const float4 b1 = *reinterpret_cast<const float4*>(p.bias + nb + 4);
      bv[0] = b0.x; bv[1] = b0.y; bv[2] = b0.z; bv[3] = b0.w; bv[4] = b1.x; bv[5] = b1.y; bv[6] = b1.z; bv[7] = b1.w;
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) bv[e] = (p.bias && nb + e < p.N) ? p.bias[nb + e] : 0.f;
    }
  }
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    if (half == 1) __syncthreads();      // (the main loop ended with a barrier)
    if (wm == half) {
#pragma unroll
      for (int i = 0; i < FM; ++i) {
        const int ml = i * 16 + (lane & 15);
#pragma unroll
        for (int j = 0; j < FN; ++j) {
          const int nl = wn * (BN / 2) + j * 16 + (lane >> 4) * 4;
          *reinterpret_cast<float4*>(ep + ml * EPITCH + nl) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
      }
    }
    __syncthreads();
    // readback in groups of EPG chunks: the residual / mask loads of a group are issued together (independent
    // loads in flight), then the staged accumulators are finished and stored as whole row runs.  Small groups
    // keep the epilogue's register footprint below the main loop's, so it does not cost occupancy.
    constexpr int EPG = NCH >= 2 ? 2 : 1;
#pragma unroll
    for (int c0 = 0; c0 < NCH; c0 += EPG) {
      float rv[EPG][8], mv[EPG][8];
#pragma unroll
      for (int g = 0; g < EPG; ++g) {
        const int idx = tid + (c0 + g) * 256;
        const int r = idx / CH, c8 = idx - r * CH;
        const int m = row0 + half * HR + r;
        const int n = col0 + c8 * 8;
        const bool inb = m < p.M && n < p.N;
        const bool full = n + 8 <= p.N;
        const int64_t mp = (AMODE == OP_CONV && p.cg.cm && inb) ? s_rowpix[m - row0] : m;     // output pixel of this GEMM row
        if (Rp) {
          if (inb && v_res && full) { if constexpr (NTIO) Ld8<TOut>::ld_nt(Rp + mp * p.ldr + n, rv[g]); else Ld8<TOut>::ld(Rp + mp * p.ldr + n, rv[g]); }
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) rv[g][e] = (inb && n + e < p.N) ? (float)Rp[mp * p.ldr + n + e] : 0.f;
          }
        }
        if (Mp) {
          if (inb && v_msk && full) Ld8<TOut>::ld(Mp + mp * p.ldm + n, mv[g]);
          else {
#pragma unroll
            for (int e = 0; e < 8; ++e) mv[g][e] = (inb && n + e < p.N) ? (float)Mp[mp * p.ldm + n + e] : 0.f;
          }
        }
      }
#pragma unroll
      for (int g = 0; g < EPG; ++g) {
        const int idx = tid + (c0 + g) * 256;
        const int r = idx / CH, c8 = idx - r * CH;
        const int m = row0 + half * HR + r;
        const int n = col0 + c8 * 8;
        if (m >= p.M || n >= p.N) continue;
        float v[8];
        {
          const float4 a = *reinterpret_cast<const float4*>(ep + r * EPITCH + c8 * 8);
          const float4 b = *reinterpret_cast<const float4*>(ep + r * EPITCH + c8 * 8 + 4);
          v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
        const float rs = p.rowscale ? p.rowscale[m] * p.alpha : p.alpha;
        const bool full = n + 8 <= p.N;
        const uint32_t keep8 = p.dthresh ? drop_mask<8>(p.seed, ((uint64_t)batch * p.M + m) * (uint64_t)p.N + n, p.dthresh) : 0xffu;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float x = v[e] * rs;
          x += bv[e];
          if (Rp) x += rv[g][e];
          if (p.act == GPV_ACT_RELU) x = fmaxf(x, 0.f);
          else if (p.act == GPV_ACT_GELU) x = gelu_erf(x);
          if (p.dthresh) x = ((keep8 >> e) & 1u) ? x * p.dscale : 0.f;
          if (Mp) x = mv[g][e] > 0.f ? x : 0.f;
          v[e] = x;
        }
        const int64_t mp = (AMODE == OP_CONV && p.cg.cm && m < p.M) ? s_rowpix[m - row0] : m;
        TOut* dst = Cp + mp * ldc + n;
        if (v_st && full) { if constexpr (NTIO) Ld8<TOut>::st_nt(dst, v); else Ld8<TOut>::st(dst, v); }   // (a run-time choice: the two stores are merged and lose the hint)
        else {
#pragma unroll
          for (int e = 0; e < 8; ++e)
            if (n + e < p.N) dst[e] = (TOut)v[e];
        }
      }
    }
  }
}

template <typename TIn, typename TOut, int AMODE, int BMODE, int BM, int BN, bool VEC>
__global__ __launch_bounds__(256) void gemm_kernel(GemmK p) {
  if (p.dthresh) p.seed = eff_seed(p.seed, p.seed_dev);
  gemm_body<TIn, TOut, AMODE, BMODE, BM, BN, VEC>(p);
}
// the same body under its own name for the backbone's 1x1 stride-1 convolutions (plain GEMMs over the pixel rows):
// profiles and PMC passes can then tell them from the transformer's Linear layers
template <typename TIn, typename TOut, int BM, int BN, bool VEC>
__global__ __launch_bounds__(256) void conv1x1_kernel(GemmK p) {
  if (p.dthresh) p.seed = eff_seed(p.seed, p.seed_dev);
  gemm_body<TIn, TOut, OP_PLAIN, OP_PLAIN, BM, BN, VEC>(p);
}
// ... with non-temporal epilogue stores / residual loads (GemmK::nt_io: outputs far larger than the MALL)
template <int BM, int BN>
__global__ __launch_bounds__(256) void conv1x1_nt_kernel(GemmK p) {
  gemm_body<bf16, bf16, OP_PLAIN, OP_PLAIN, BM, BN, true, true>(p);
}

// C[m, n] += sum_s ws[s][m][n]   (second pass of a workspace split reduction).  A group of G threads shares one run
// of 4 columns and strides over the splits (a layer2 1x1 wgrad has 96 slabs of 64K outputs: one thread per output
// quad walking 96 slabs was 64 blocks of serial latency), partial sums meet in LDS.
template <int G>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ ws, int nsplit, int M, int N, float* __restrict__ C,
                                                            int64_t ldc) {
  constexpr int QB = 256 / G;                      // quads per block
  __shared__ float4 part[G > 1 ? 256 : 1];
  const int64_t slab = (int64_t)M * N;
  const int nq = N >> 2;                           // host guarantees N % 4 == 0, ldc % 4 == 0, C 16-byte aligned
  const int64_t total = (int64_t)M * nq;
  const int ql = threadIdx.x % QB, g = threadIdx.x / QB;
  const int64_t i = (int64_t)blockIdx.x * QB + ql;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  int m = 0, n = 0;
  if (i < total) {
    m = (int)(i / nq); n = (int)(i - (int64_t)m * nq) * 4;
    const float* src = ws + (int64_t)m * N + n;
    for (int s = g; s < nsplit; s += G) {
      const float4 v = *reinterpret_cast<const float4*>(src + s * slab);
      a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
    }
  }
  if constexpr (G > 1) {
    part[threadIdx.x] = a;
    __syncthreads();
    if (g == 0) {
#pragma unroll
      for (int k = 1; k < G; ++k) {
        const float4 v = part[k * QB + ql];
        a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
      }
    }
  }
  if (g == 0 && i < total) {
    float4* dst = reinterpret_cast<float4*>(C + (int64_t)m * ldc + n);
    float4 c = *dst;
    c.x += a.x; c.y += a.y; c.z += a.z; c.w += a.w;
    *dst = c;
  }
}

}  // namespace

namespace gpvk {
// C[m,n] += sum over `split` dense [M,N] slabs of ws (N % 4 == 0, ldc % 4 == 0, C 16-byte aligned)
int launch_splitk_reduce(const float* ws, int split, int M, int N, float* C, int64_t ldc, hipStream_t st) {
  const int64_t quads = (int64_t)M * (N / 4);
  if (split >= 32) {
    hipLaunchKernelGGL(splitk_reduce_kernel<16>, dim3((unsigned)((quads + 15) / 16)), dim3(256), 0, st, ws, split, M, N, C, ldc);
  } else if (split >= 4) {
    hipLaunchKernelGGL(splitk_reduce_kernel<4>, dim3((unsigned)((quads + 63) / 64)), dim3(256), 0, st, ws, split, M, N, C, ldc);
  } else {
    hipLaunchKernelGGL(splitk_reduce_kernel<1>, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, ws, split, M, N, C, ldc);
  }
  GPV_CHECK_LAUNCH();
  return 0;
}
}  // namespace gpvk

namespace {

template <typename TIn, typename TOut, int AMODE, int BMODE, int BM, int BN, bool VEC>
int launch_cfg_v(const GemmK& k, const Route& r, hipStream_t st) {
  constexpr bool PRECISE = sizeof(TIn) == 4;
  constexpr size_t lds = (size_t)2 * (BM + BN) * LDK * 2 * (PRECISE ? 2 : 1);
  GemmK p = k;
  p.tilesN = r.tilesN;
  p.kt_per_split = r.kt_per_split;
  p.ws = nullptr;
  if (r.two_pass) {       // split reduction through the workspace (gemm_route.h tile_geometry): plain partial products, a second kernel adds the slabs to C
    p.ws = reinterpret_cast<float*>(k.ws_base);
    p.accumulate = 0; p.res = nullptr; p.mask = nullptr; p.bias = nullptr; p.act = 0; p.dthresh = 0;
  }
  auto fn = gemm_kernel<TIn, TOut, AMODE, BMODE, BM, BN, VEC>;
  if constexpr (AMODE == OP_PLAIN && BMODE == OP_PLAIN) {
    if (r.c11) fn = conv1x1_kernel<TIn, TOut, BM, BN, VEC>;
    if constexpr (std::is_same<TIn, bf16>::value && std::is_same<TOut, bf16>::value && VEC) {
      if (r.nt) fn = conv1x1_nt_kernel<BM, BN>;
    }
  }
  static bool attr_done[2] = {false, false};
  if (lds > 64 * 1024 && !attr_done[r.c11 ? 1 : 0]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { (void)hipGetLastError(); return (int)e; }      // (leave no stale error behind for the next launch check)
    attr_done[r.c11 ? 1 : 0] = true;
  }
  hipLaunchKernelGGL(fn, dim3(r.gx, r.gy, r.gz), dim3(r.block), lds, st, p);
  GPV_CHECK_LAUNCH();
  if (r.two_pass) {
    const int e = launch_splitk_reduce(p.ws, r.split, p.M, p.N, reinterpret_cast<float*>(p.C), p.ldc, st);
    if (e) return e;
  }
  return 0;
}

template <typename TIn, typename TOut, int AMODE, int BMODE, int BM, int BN>
int launch_cfg(const GemmK& k, const Route& r, hipStream_t st) {
  if (r.vec) return launch_cfg_v<TIn, TOut, AMODE, BMODE, BM, BN, true>(k, r, st);
  return launch_cfg_v<TIn, TOut, AMODE, BMODE, BM, BN, false>(k, r, st);
}

// Second pass of a split FORWARD convolution: y[m, n] = act(sum_s ws[s][m][n] + bias[n] + res[m, n]), four columns per thread.
__global__ __launch_bounds__(256) void conv_split_epilogue_kernel(const float* __restrict__ ws, int nsplit, int M, int N, const float* __restrict__ bias,
                                                                  const bf16* __restrict__ res, int act, bf16* __restrict__ y) {
  const int nq = N >> 2;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)M * nq) return;
  const int m = (int)(i / nq), n = (int)(i - (int64_t)m * nq) * 4;
  const int64_t slab = (int64_t)M * N, off = (int64_t)m * N + n;
  float4 a = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int sidx = 0; sidx < nsplit; ++sidx) {
    const float4 v = *reinterpret_cast<const float4*>(ws + sidx * slab + off);
    a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w;
  }
  float o[4] = {a.x, a.y, a.z, a.w};
  if (bias) {
    const float4 b = *reinterpret_cast<const float4*>(bias + n);
    o[0] += b.x; o[1] += b.y; o[2] += b.z; o[3] += b.w;
  }
  if (res) {
    const bf16x4 r = *reinterpret_cast<const bf16x4*>(res + off);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] += (float)r[e];
  }
  bf16x4 out;
#pragma unroll
  for (int e = 0; e < 4; ++e) out[e] = (bf16)(act == GPV_ACT_RELU ? fmaxf(o[e], 0.f) : o[e]);
  *reinterpret_cast<bf16x4*>(y + off) = out;
}

// FAM_CONV_SPLIT (gemm_route.h conv_split_select): the reduction split over grid.y into fp32 slabs of the caller's workspace, then the
// epilogue kernel above
int conv_split_launch(const GemmK& k, const Route& r, hipStream_t st) {
  GemmK p = k;
  p.tilesN = r.tilesN;
  p.kt_per_split = r.kt_per_split;
  p.split_k = r.split;
  p.ws = reinterpret_cast<float*>(k.ws_base);
  p.res = nullptr; p.bias = nullptr; p.act = 0;
  hipLaunchKernelGGL((gemm_kernel<bf16, float, OP_CONV, OP_PLAIN, 64, 64, true>), dim3(r.gx, r.gy, r.gz), dim3(r.block), (size_t)r.lds, st, p);
  GPV_CHECK_LAUNCH();
  const int64_t quads = (int64_t)k.M * (k.N / 4);
  hipLaunchKernelGGL(conv_split_epilogue_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, st, p.ws, r.split, k.M, k.N, k.bias,
                     reinterpret_cast<const bf16*>(k.res), k.act, reinterpret_cast<bf16*>(k.C));
  GPV_CHECK_LAUNCH();
  return 0;
}

template <typename TIn, typename TOut, int AMODE, int BMODE>
int launch_tiles(const GemmK& k, const Route& r, hipStream_t st) {
  if (r.bm == 128 && r.bn == 128) return launch_cfg<TIn, TOut, AMODE, BMODE, 128, 128>(k, r, st);
  if (r.bm == 128) return launch_cfg<TIn, TOut, AMODE, BMODE, 128, 64>(k, r, st);
  return launch_cfg<TIn, TOut, AMODE, BMODE, 64, 64>(k, r, st);
}

template <int AMODE, int BMODE>
int launch_dtype(const GemmK& k, const Route& r, hipStream_t st) {
  if (r.dt_in == GPV_BF16 && r.dt_out == GPV_BF16) return launch_tiles<bf16, bf16, AMODE, BMODE>(k, r, st);
#ifndef GPV_EXPERIMENT      /* trimmed instantiation set for kernel-tuning builds */
  if (r.dt_in == GPV_BF16 && r.dt_out == GPV_F32) return launch_tiles<bf16, float, AMODE, BMODE>(k, r, st);
  if (r.dt_in == GPV_F32 && r.dt_out == GPV_F32) return launch_tiles<float, float, AMODE, BMODE>(k, r, st);
#endif
  return (int)hipErrorInvalidValue;
}

// FAM_TILE: the register-staged kernel
int tile_launch(const GemmK& k, const Route& r, hipStream_t st) {
  if (r.bmode == OP_CONV) {       // conv weight gradient: bf16 on three tiles, fp32 ("precise") on 64 x 64
    if (r.dt_in == GPV_BF16) return launch_tiles<bf16, float, OP_TRANS, OP_CONV>(k, r, st);
    return launch_cfg<float, float, OP_TRANS, OP_CONV, 64, 64>(k, r, st);
  }
  if (r.amode == OP_CONV) return launch_dtype<OP_CONV, OP_PLAIN>(k, r, st);
  if (r.amode == OP_TRANS) return launch_dtype<OP_TRANS, OP_TRANS>(k, r, st);
  return r.bmode == OP_TRANS ? launch_dtype<OP_PLAIN, OP_TRANS>(k, r, st) : launch_dtype<OP_PLAIN, OP_PLAIN>(k, r, st);
}

// Backward-data of a 1x1 stride-2 convolution (the downsample projections): only output pixels with even row AND column receive a
// product; the other three quarters are dx = res * (mask > 0) (or 0).  The GEMM kernels take the first quarter (parity class 0 of
// the class-major row order); this element-wise kernel streams the rest.  (Routed through the GEMM epilogue -- one dummy k-tile
// per 64/128-row tile, LDS round trip -- those three quarters ran at 2 TB/s and were most of a 245 us launch.)
__global__ __launch_bounds__(256) void s2_dgrad_fill_kernel(bf16* __restrict__ dx, const bf16* __restrict__ res, const bf16* __restrict__ mask,
                                                            int64_t total_chunks, int OW, int OH, int C8) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total_chunks) return;
  const int64_t px = i / C8;
  const int ow = (int)(px % OW), oh = (int)((px / OW) % OH);
  if (((oh | ow) & 1) == 0) return;                    // class 0: written by the GEMM
  bf16x8 o = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
  if (res) {
    o = *reinterpret_cast<const bf16x8*>(res + i * 8);
    if (mask) {
      const bf16x8 m = *reinterpret_cast<const bf16x8*>(mask + i * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = (float)m[e] > 0.f ? o[e] : (bf16)0.f;
    }
  }
  *reinterpret_cast<bf16x8*>(dx + i * 8) = o;
}

}  // namespace

extern "C" int gpv_abi_version(void) { return 2; }

namespace gpvk { Knobs g_knobs; }
static_assert(kRouteInvalid == (int)hipErrorInvalidValue, "gemm_route.h names hipErrorInvalidValue by its value");

// one part of a routed call
static int launch_route(const GemmK& k, const Route& r, hipStream_t st) {
  switch (r.family) {
    case FAM_GEMV: return gemv_launch(k, r, st);
    case FAM_C1S: return c1s_launch(k, r, st);
    case FAM_C3S: return c3s_launch(k, r, st);
    case FAM_CONV_SPLIT: return conv_split_launch(k, r, st);
    case FAM_PIPE: return pipe_launch(k, r, st);
    case FAM_SKINNY: return skinny_launch(k, r, st);
    case FAM_GLDS: case FAM_HALO: return glds_launch(k, r, st);
    case FAM_GLDS_WGRAD: case FAM_GLDS_TT: return glds_tt_launch(k, r, st);
    case FAM_SKINNY_TT: return skinny_tt_launch(k, r, st);
    case FAM_TILE: return tile_launch(k, r, st);
    case FAM_S2_FILL:
      hipLaunchKernelGGL(s2_dgrad_fill_kernel, dim3(r.gx), dim3(r.block), 0, st, reinterpret_cast<bf16*>(k.C), reinterpret_cast<const bf16*>(k.res),
                         reinterpret_cast<const bf16*>(k.mask), (int64_t)k.M * r.ncols, k.cg.OW, k.cg.OH, r.ncols);
      GPV_CHECK_LAUNCH();
      return 0;
  }
  return (int)hipErrorInvalidValue;
}

static int launch_routed(Routed& rt, hipStream_t st) {
  if (rt.err) return rt.err;
  for (int i = 0; i < rt.nparts; ++i) {
    rt.k[i].seed_dev = gpvk::g_seed_dev;
    const int e = launch_route(rt.k[i], rt.r[i], st);
    if (e) return e;
  }
  return 0;
}

extern "C" int gpv_gemm(const gpv_gemm_args* a, void* stream) {
  Routed rt;
  route_gemm(a, g_knobs, &rt);
  return launch_routed(rt, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gpv_conv2d(const gpv_conv_args* a, void* stream) {
  Routed rt;
  route_conv2d(a, g_knobs, &rt);
  return launch_routed(rt, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int gpv_conv2d_mask_bits_ok(const gpv_conv_args* a) {
  if (!a || (!a->y_mask_bits && !a->relu_mask_bits)) return 0;
  Routed rt;
  route_conv2d(a, g_knobs, &rt);
  return rt.err == 0 ? 1 : 0;
}

namespace gpvk { int attn_bwd1_mode(int set); long attn_bwd1_launches(long set); }   // attention.hip

// option number -> Knobs field (a mode) or launch counter.  Returns the previous value, -1 for an unknown option.
extern "C" int gpv_set_option(int option, int value) {
  static const struct { int option; int Knobs::* mode; long Knobs::* count; } table[] = {
      {GPV_OPT_GLDS, &Knobs::glds, nullptr},           {GPV_OPT_GLDS_LAUNCHES, nullptr, &Knobs::n_glds},
      {GPV_OPT_SKINNY, &Knobs::skinny, nullptr},       {GPV_OPT_GLDS_WGRAD, &Knobs::wgrad, nullptr},
      {GPV_OPT_PIPE, &Knobs::pipe, nullptr},           {GPV_OPT_PIPE_LAUNCHES, nullptr, &Knobs::n_pipe},
      {GPV_OPT_C1S, &Knobs::c1s, nullptr},             {GPV_OPT_C1S_LAUNCHES, nullptr, &Knobs::n_c1s},
      {GPV_OPT_C3S, &Knobs::c3s, nullptr},             {GPV_OPT_C3S_LAUNCHES, nullptr, &Knobs::n_c3s},
      {GPV_OPT_GEMV, &Knobs::gemv, nullptr},           {GPV_OPT_GEMV_LAUNCHES, nullptr, &Knobs::n_gemv},
      {GPV_OPT_WG8, &Knobs::wg8, nullptr},             {GPV_OPT_WG8_LAUNCHES, nullptr, &Knobs::n_wg8},
      {GPV_OPT_W8L, &Knobs::w8l, nullptr},             {GPV_OPT_WG8H, &Knobs::wg8h, nullptr},
      {GPV_OPT_PIPE_SMALL, &Knobs::pipe_small, nullptr},
      {GPV_OPT_C3_HALO, &Knobs::halo, nullptr},        {GPV_OPT_C3_HALO_LAUNCHES, nullptr, &Knobs::n_halo},
  };
  if (option == GPV_OPT_ATTN_BWD1) return gpvk::attn_bwd1_mode(value);
  if (option == GPV_OPT_ATTN_BWD1_LAUNCHES) return (int)gpvk::attn_bwd1_launches(value);
  for (const auto& t : table) {
    if (t.option != option) continue;
    if (t.mode) { const int prev = g_knobs.*t.mode; g_knobs.*t.mode = value; return prev; }
    const long prev = g_knobs.*t.count;
    if (value >= 0 || option != GPV_OPT_PIPE_LAUNCHES) g_knobs.*t.count = value;      // (the pipe counter has always ignored a negative value)
    return (int)prev;
  }
  return -1;
}
