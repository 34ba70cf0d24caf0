// Which kernel does a gpv_gemm / gpv_conv2d call take?  The whole answer, host-only: plain C++17 with no HIP call and no device type, so
// that g++ compiles it on its own (tools/route_host_check.cpp, tests/test_routes_cpu.py).  For every kernel family one pure
// <family>_select: legality, the measured "where it wins" thresholds, the kernel instance and the launch geometry, written into a
// Route.  route_gemm / route_conv2d validate the arguments, prepare the GemmK and state the ORDER in which the families are tried --
// once, in route_try.  The .hip files keep <family>_launch(GemmK, Route, stream): template switch, attribute once-flags, counter, launch.
// A new kernel family adds its FAM_ value, its select here with its place in route_try, its launch in its .hip file, and its cases
// in tests/route_cases.py.
#pragma once
#include <stdint.h>
#include "../../include/gpv_hip.h"
#include "host_defs.h"

namespace gpvk {

enum { OP_PLAIN = 0, OP_TRANS = 1, OP_CONV = 2 };

struct ConvGeom {
  int IH, IW, Cs, Cin, OH, OW, KH, KW, SH, SW, PH, PW, dgrad;
  int cm;          // stride-2 dgrad: GEMM rows are ordered parity-class-major (4 classes of (OH/2)*(OW/2) pixels per image)
  int cls_rows;    // rows per parity class = batch * (OH/2) * (OW/2)
};

struct GemmK {
  const void* A; const void* B; void* C;
  int M, N, K;
  int64_t lda, ldb, ldc, sA, sB, sC;
  float alpha;
  const float* rowscale; const float* bias;
  const void* res; int64_t ldr, sR;
  const void* mask; int64_t ldm;
  int act; uint32_t dthresh; float dscale; uint64_t seed; const uint64_t* seed_dev;
  int accumulate, split_k, kt_per_split, tilesN;
  int vecA, vecB;
  int conv1x1;         // launched from gpv_conv2d as a plain GEMM: use the conv1x1_kernel name
  int depi;            // gemm_glds.hip: register epilogue over permuted output columns (Route::depi)
  int no_small;        // host side: gpv_gemm_args.flags & GPV_GEMM_NO_PIPE_SMALL (pipe_select skips its small-M configurations for this call)
  int nt_io;           // epilogue stores / residual loads non-temporal (outputs far larger than the 256 MB MALL: layer1's 314 MB maps)
  void* ws_base; int64_t ws_bytes;   // host side: caller workspace for split reductions
  float* ws;                         // kernel side: != NULL -> split s writes its partial product to ws[s][M][N]
  const uint32_t* mask_bits;   // conv1x1_stream.hip: the ReLU mask as ONE BIT per element, word [row][n >> 5] bit n & 31 (read instead of `mask`, which is then only non-NULL)
  uint32_t* out_bits;          // conv1x1_stream.hip: (output > 0) of a ReLU forward written in the same layout
  float* a_rowsum;     // TRANS x TRANS only: a_rowsum[m] += sum_k A[m,k]  (bias gradient fused into the weight-gradient GEMM)
  ConvGeom cg;
};

// ---- tile constants of the kernels (defined here once; the .hip files use them from here) ---------------------------------------
constexpr int BK = 32;        // gemm.hip: k-tile of the register-staged kernel
constexpr int LDK = 40;       // gemm.hip: LDS row pitch in elements (80 B: keeps ds_read_b128 16-B aligned, spreads banks)
constexpr int GBK = 64;       // gemm_glds.hip, gemm_pipe.hip: k-tile in elements
constexpr int ROWB = 128;     // ... bytes per staged operand row
constexpr int GBM = 256;      // gemm_glds.hip: rows of the 8-wave tile
constexpr int PIPE_THREADS = 512;     // gemm_pipe.hip: 8 waves
constexpr int SBM = 64, SBN = 64, SBK = 128, SPITCH = SBK + 8;     // gemm_skinny.hip; LDS row pitch 272 B: 16 rows cover all 64 banks
constexpr int TPITCH = SBN + 16;      // gemm_skinny.hip: reduction-major B tile [128 red][64 cols]: pitch 160 B (the transpose-read rule of gemm.hip)
constexpr int TBM = 128, TBN = 128, TBK = 64;       // gemm_glds_tt.hip
constexpr int ROWBYTES = 256;                      // ... one pixel row of a 128-column operand tile
constexpr int OP_BYTES = TBK * ROWBYTES;           // 16 KB
constexpr int TSTAGE = 2 * OP_BYTES;
constexpr int C3_OOB = 0x7ffffff0;      // conv3x3_stream.hip
constexpr int C3_NSL = 64;              // ... output channels per block
// gemm_pipe.hip tile configurations: index -> (BM, BN, WM, stages)
struct PipeCfg { int bm, bn, wm, ns; };
constexpr PipeCfg kCfgs[] = {{256, 128, 4, 3}, {192, 128, 4, 3}, {128, 128, 2, 3}, {160, 256, 2, 3}, {128, 256, 2, 3}, {96, 256, 2, 3},
                             {64, 64, 2, 6}, {32, 64, 2, 8}};     // the last two: small-M tiles, 6 / 8 stages, plain GEMMs only
constexpr int kNumBig = 6;
constexpr int kNumCfgs = sizeof(kCfgs) / sizeof(kCfgs[0]);
// conv1x1_stream.hip: output channels per block: the whole layer when its weights fit the LDS (K <= 128: up to 512 channels), else slices on gridDim.y
inline int c1s_cols(int K, int N) {
  const int cap = K <= 128 ? 512 : (K == 256 ? 256 : 128);
  return N < cap ? N : cap;
}

// ---- every mode gpv_set_option sets, and the launch counters it reads -------------------------------------------------------------
struct Knobs {
  int glds = tune_env("GPV_GLDS", 1);           // GPV_OPT_GLDS: 0 = never, 1 (default) = where it is expected to win, 2 / 3 = the 8-wave / 4-wave variant wherever legal
  int pipe = tune_env("GPV_PIPE", 1);           // GPV_OPT_PIPE: 0 off, 1 heuristic, 100+i: force configuration i wherever legal
  int pipe_small = tune_env("GPV_PIPE_SMALL", 1);   // GPV_OPT_PIPE_SMALL: the small-M configurations (64 x 64 / 32 x 64, 6 / 8 stages)
  int skinny = 1;                               // GPV_OPT_SKINNY: 0 never, 1 heuristic, 2 wherever legal
  int gemv = 1;                                 // GPV_OPT_GEMV: 0 never, 1 (default) wherever legal
  int c1s = 1;                                  // GPV_OPT_C1S: 0 never, 1 heuristic, 2 wherever legal (tests)
  int c3s = 1;                                  // GPV_OPT_C3S: 0 never, 1 heuristic, 2 wherever legal (tests)
  int halo = tune_env("GPV_C3_HALO", 1);        // GPV_OPT_C3_HALO: 0 never, 1 the 160-row tiles (where it wins), 2 the 96-row tiles as well
  int wgrad = tune_env("GPV_GLDS_WGRAD", 1);    // GPV_OPT_GLDS_WGRAD
  int wg8 = tune_env("GPV_WG8", 1);             // GPV_OPT_WG8: eight-phase 256 x 256 weight-gradient kernel
  int wg8h = tune_env("GPV_WG8H", 1);           // GPV_OPT_WG8H: the 128 x 256 | 256 x 128 eight-phase tiles for the problems with a 128-wide side (layer2)
  int w8l = tune_env("GPV_W8L", 0);             // GPV_OPT_W8L: the same kernel on the linear weight-gradient groups -- OFF by default: alone on the chip the step's 123
                                                // linear gradients take 810 instead of 885 us with it, inside the step nothing (16.63 / 16.60 ms off, 16.66 / 16.77 on, same box): its
                                                // 128 KB blocks take whole CUs from the backward chain they run beside
  int two_per_cu = tune_env("GPV_TWO_PER_CU", 1);   // two half-width tiles per CU in the direct-to-LDS GEMM (0: one 8-wave tile)
  int bm96_fill = tune_env("GPV_BM96", 1);      // 96-row tiles for <= 1024-row GEMMs (two_per_cu_bm)
  int skinny_tile = tune_env("GPV_SKINNY_TILE", 0);     // tuning build: 0 = by cost, 1 = 64 x 64, 2 = 32 x 64, 3 = 32 x 32
  long n_glds = 0, n_pipe = 0, n_halo = 0, n_c1s = 0, n_c3s = 0, n_gemv = 0, n_wg8 = 0;     // GPV_OPT_*_LAUNCHES
  // a kernel family is being forced (tests / tuning): the small-problem side paths step aside
  bool forced() const { return glds >= 2 || pipe >= 100; }
};
extern Knobs g_knobs;     // gemm.hip (the one definition)

// ---- a routing decision ---------------------------------------------------------------------------------------------------------
enum Family {
  FAM_GEMV, FAM_C1S, FAM_C3S, FAM_CONV_SPLIT, FAM_PIPE, FAM_SKINNY, FAM_GLDS, FAM_HALO, FAM_GLDS_WGRAD, FAM_GLDS_TT, FAM_SKINNY_TT,
  FAM_TILE, FAM_S2_FILL
};
inline const char* family_name(int f) {
  static const char* const names[] = {"gemv", "c1s", "c3s", "conv_split", "pipe", "skinny", "glds", "halo", "glds_wgrad", "glds_tt", "skinny_tt",
                                      "tile", "s2_fill"};
  return names[f];
}

struct Route {
  int family;
  // the kernel instance
  int amode, bmode;             // OP_*: how the A / B operand is staged
  int dt_in, dt_out;            // GPV_BF16 / GPV_F32
  int bm, bn;                   // tile (gemv: bm = rows per wave MR, bn = columns per wave NW)
  int cfg;                      // pipe: index into kCfgs; skinny: k-loop stages (1 | 2)
  int vec;                      // tile: 16-byte operand loads
  int c11, nt;                  // the conv1x1 kernel name; the non-temporal instance (tile, c1s)
  int ck, nh, np;               // c1s: K, channels per register pass, passes; c3s: ck = Cin
  int res, mask, lin, bits;     // c1s / c3s instance flags
  int dgrad, d2, waves;         // c3s: backward-data form, the stride-2 backward-data kernel, waves per block
  // the launch geometry
  unsigned gx, gy, gz, block;
  int64_t lds;                  // dynamic LDS bytes
  int tilesN, split, kt_per_split;
  int two_pass;                 // a second launch follows: split reduction (splitk_reduce) or the split forward conv's epilogue
  int depi;                     // GemmK::depi
  int ncols;                    // c1s: output channels per block
  int rows, nstrip, nseg, nitems;     // c3s: the kernels' work-item arguments
};

constexpr int kRouteInvalid = 1;      // == hipErrorInvalidValue (asserted in gemm.hip)

// what route_gemm / route_conv2d return: the prepared kernel arguments and the route of each part (two parts: the stride-2 pointwise
// backward-data split).  Lives on the caller's stack, no allocation.
struct Routed {
  int err;            // 0, or the value the entry point returns
  int nparts, batch;
  GemmK k[2];
  Route r[2];
};

// ---- two-per-CU tiles (gemm_glds.hip) -------------------------------------------------------------------------------------------
// tile height (160 | 96) with which (rows / h) x (N / 128) tiles fill the 512 two-per-CU slots in whole rounds (>= 90 % of the last
// round's slots, more than 384 tiles), 0 = none
inline int two_per_cu_bm(const GemmK& k, int batch, const Knobs& kn) {
  if (k.N % 128 != 0 || batch != 1) return 0;
  if (kn.bm96_fill && k.M <= 1024) {
    // round 5, measured (tools/bench_skinny_pf.py, GPV_BM96 in the tuning build): at <= 1024 rows the two-per-CU 96 x 128 direct-to-LDS kernel beats the
    // small-M kernel wherever 96-row tiles are more tiles than 128-row ones -- 640 x 768 x 2048 15.4 -> 10.6 us, 640 x 768 x 768 8.5 -> 6.6,
    // 100 x 768 x 768 7.9 -> 6.5 -- and loses on the 3200- / 9600-row GEMMs (9600 x 256 x 2048 23.6 -> 25.1, 3200 x 768 x 3072 32.1 -> 33.3)
    const int64_t t128 = (int64_t)((k.M + 127) / 128) * (k.N / 128), t96 = (int64_t)((k.M + 95) / 96) * (k.N / 128);
    if (t96 <= 256 && t96 * 10 >= t128 * 12) return 96;
  }
  int best = 0;
  double best_u = 0.0;
  const int heights[] = {160, 96};
  for (int bm : heights) {
    const int64_t t = (int64_t)((k.M + bm - 1) / bm) * (k.N / 128);
    if (t <= 384) continue;
    const double u = (double)t / (512.0 * ((t + 511) / 512));
    if ((t <= 512 || u >= 0.9) && u > best_u) { best = bm; best_u = u; }     // one round: every tile is resident at once, whatever the fill
  }
  return best;
}
inline bool glds_two_per_cu(const GemmK& k, int batch, const Knobs& kn) {
  return kn.two_per_cu && k.K >= 512 && (!k.cg.cm || k.cg.KH == 1) && two_per_cu_bm(k, batch, kn) != 0;      // (K = 256: measured, no gain)
}

// ---- gemv.hip: M <= 8 rows (the greedy decode step at small batch): a wave per 1..4 output columns, no LDS -------------------------
inline bool gemv_select(const GemmK& k, int dtype_in, int dtype_out, int batch, const Knobs& kn, Route* r) {
  if (kn.gemv == 0 || kn.forced() || k.M > 8 || batch != 1 || k.accumulate || k.split_k > 1) return false;
  if (k.rowscale || k.mask || k.dthresh || k.a_rowsum) return false;
  if (k.M > 2 && k.N >= 4096) return false;            // 4 columns x > 2 rows per wave: the tile kernels are faster (tools/bench_gemv.py)
  if (k.K % 8 != 0 || k.lda % 8 != 0 || k.ldb % 8 != 0 || !al16(k.A) || !al16(k.B)) return false;
  if (!((dtype_in == GPV_BF16 && (dtype_out == GPV_BF16 || dtype_out == GPV_F32)) || (dtype_in == GPV_F32 && dtype_out == GPV_F32))) return false;
  r->family = FAM_GEMV; r->dt_in = dtype_in; r->dt_out = dtype_out;
  r->bm = k.M == 1 ? 1 : (k.M == 2 ? 2 : (k.M <= 4 ? 4 : 8));
  // columns per wave: as few as keep >= 256 workgroups (one per CU) busy
  r->bn = k.N >= 4096 ? 4 : (k.N >= 2048 ? 2 : 1);
  r->gx = (unsigned)((k.N + 4 * r->bn - 1) / (4 * r->bn)); r->gy = r->gz = 1; r->block = 256; r->lds = 0;
  return true;
}

// ---- conv1x1_stream.hip: streaming kernel for the K <= 256 pointwise convolutions over >= 65536 pixels (weights resident in LDS,
// a wave per 16 pixels, register epilogue in a permuted channel order).  linear: called from gpv_gemm (plain rows, alpha / dropout allowed)
inline bool c1s_select(const GemmK& k, int dtype_in, int dtype_out, bool linear, const Knobs& kn, Route* r) {
  static const int env = tune_env("GPV_C1S", -1);
  const int mode = env >= 0 ? env : kn.c1s;
  if (mode == 0 || dtype_in != GPV_BF16 || dtype_out != GPV_BF16) return false;
  if (k.K != 64 && k.K != 128 && k.K != 256 && k.K != 512) return false;
  if (k.N != 64 && k.N != 128 && k.N != 256 && k.N != 512 && k.N != 1024 && k.N != 2048 && !(linear && k.N % 256 == 0 && k.N <= 2048)) return false;
  const int ncols = c1s_cols(k.K, k.N), nsl = k.N / ncols;
  if ((int64_t)ncols * (k.K + 8) * 2 + (int64_t)ncols * 4 > 150 * 1024 || nsl > 8) return false;
  if (k.rowscale || k.accumulate || k.split_k > 1 || k.a_rowsum) return false;
  if ((k.alpha != 1.0f || k.dthresh) && !(linear && k.K == 256 && k.N >= 256 && k.N % 256 == 0)) return false;
  if (linear && (k.cg.SH == 2 || k.cg.cm || k.nt_io)) return false;
  if (k.act != GPV_ACT_NONE && k.act != GPV_ACT_RELU) return false;
  if (k.lda % 8 || k.ldb != k.K || k.ldc % 8 || (k.res && k.ldr % 8) || (k.mask && k.ldm % 8)) return false;
  if (!al16(k.A) || !al16(k.B) || !al16(k.C) || (k.res && !al16(k.res)) || (k.mask && !al16(k.mask))) return false;
  if (linear) {      // gpv_gemm: 256 -> 2048 features over >= 2048 rows (the DETR feed-forward; tools/bench_c1s_linear.py: 1024 / 1536 outputs are faster on the tile kernels)
    if (mode == 1 && (k.K != 256 || k.N < 1536 || k.M < 2048)) return false;      // (1536: as graph nodes 20.8 against 26.8 us at 9600 rows, tools/tune_gemms.py --chain; 1024 stays on the tile kernels)
  } else if (mode == 1 && ((int64_t)k.M * nsl < 65536 || k.M < 32768)) return false;   // a streaming regime needs rows (x slices): the layer1-3 maps at training batch sizes
  // the instance: channels per block -> channels per register pass (K = 512: N <= 128 per block, the weights must fit the LDS)
  const int nh = ncols >= 256 ? 256 : ncols;
  if (nh == 256 && k.K > 256) return false;
  const bool res = k.res != nullptr, m = k.mask != nullptr, nt = k.nt_io != 0;
  bool lin = false, bits = false;
  // gpv_gemm's calls always take the LIN instances (alpha = 1 and no dropout are exact no-ops there): a linear layer's launch is then
  // told from a convolution's by its NAME -- profiles and bench.py's live HBM-traffic passes (tools/pmc_traffic.py) classify by it
  if (linear || k.alpha != 1.0f || k.dthresh) {     // linear-layer extras: instantiated for the 256 -> n x 256 shapes only
    if (!(k.K == 256 && nh == 256) || nt) return false;
    lin = true;
  } else if (k.mask_bits || k.out_bits) {
    // one-bit ReLU masks: the instances the ResNet body uses -- conv3 + residual + ReLU of layer2 / layer3 writes them (K = 128 | 256,
    // 256 channels per pass), conv1's backward-data (residual + mask) of layer2 / layer3 / layer4.0 reads them (+ K = 512 -> 128-wide passes)
    if (nt || !res || (k.mask_bits && k.out_bits) || k.N % 256 != 0) return false;
    if (!(((k.K == 128 || k.K == 256) && nh == 256) || (k.K == 512 && nh == 128 && !k.out_bits))) return false;
    if (k.out_bits && (m || k.act != GPV_ACT_RELU)) return false;
    bits = true;
  } else if (nt && m) {      // (non-temporal: the layer1 forwards -- never with a mask)
    return false;
  }
  const int np = ncols / nh;
  if (!(np == 1 || (np == 2 && k.K <= 128 && nh == 256 && !lin))) return false;
  r->family = FAM_C1S; r->dt_in = dtype_in; r->dt_out = dtype_out;
  r->ck = k.K; r->nh = nh; r->np = np; r->res = res; r->mask = bits ? (k.out_bits ? 0 : 1) : m; r->nt = nt; r->lin = lin; r->bits = bits;
  r->ncols = ncols;
  r->lds = (int64_t)ncols * k.K * 2 + (int64_t)ncols * (int64_t)sizeof(float);
  // persistent waves: two blocks of 8 waves per CU when the weights leave room for them, one otherwise
  const int ntile = (k.M + 15) / 16;
  static const int bpc = tune_env("GPV_C1S_BLOCKS", 0);
  int blocks = bpc > 0 ? bpc : (r->lds <= 72 * 1024 ? 512 : 256);
  blocks = (blocks + nsl - 1) / nsl;
  if (blocks * 8 > ntile) blocks = (ntile + 7) / 8;
  r->gx = (unsigned)blocks; r->gy = (unsigned)nsl; r->gz = 1; r->block = 512;
  return true;
}

// ---- conv3x3_stream.hip: streaming kernel for the 3x3 convolutions with 64 / 128 input channels over >= 65536 output pixels (weights
// of 64 output channels resident in LDS, a wave per 32 pixels, 32x32x16 MFMA, no barriers): forward, backward-data stride 1 and
// the stride-2 backward-data parity classes.
// k: the GemmK route_conv2d prepared for the implicit-GEMM path (A = input pixels, B = [N][9][Cin] weights, cg = geometry).
inline bool c3s_select(const GemmK& k, int dtype_in, int dtype_out, const Knobs& kn, Route* r) {
  static const int env = tune_env("GPV_C3S", -1);
  const int mode = env >= 0 ? env : kn.c3s;
  const ConvGeom& g = k.cg;
  if (mode == 0 || dtype_in != GPV_BF16 || dtype_out != GPV_BF16) return false;
  if (g.KH != 3 || g.KW != 3 || g.PH != 1 || g.PW != 1 || g.SH != g.SW) return false;
  if ((g.Cin != 64 && g.Cin != 128) || k.N % C3_NSL != 0 || k.N > 256 || k.K != 9 * g.Cin) return false;
  if (g.Cs % 8 != 0 || k.ldc % 8 != 0 || (k.mask && k.ldm % 8 != 0) || k.ldb != k.K) return false;
  if (k.res || k.rowscale || k.alpha != 1.0f || k.dthresh || k.accumulate || k.split_k > 1 || k.a_rowsum) return false;
  if (k.act != GPV_ACT_NONE && k.act != GPV_ACT_RELU) return false;
  if (!al16(k.A) || !al16(k.B) || !al16(k.C) || (k.mask && !al16(k.mask))) return false;
  const bool d2 = g.SH == 2 && g.dgrad && g.Cin == 128 && g.OH == 2 * g.IH && g.OW == 2 * g.IW && k.act == GPV_ACT_NONE && !k.bias;
  if (g.SH != 1 && !d2) return false;       // (the stride-2 forward stays on the tile kernels)
  // input extent addressed with 32-bit byte offsets (dgrad: the "input" is dy)
  const int64_t in_px = (int64_t)(k.M / (g.OH * g.OW)) * g.IH * g.IW;
  if (in_px * g.Cs * 2 >= (int64_t)C3_OOB) return false;
  // a streaming regime needs rows: the layer1 / layer2 maps at training batch sizes -- and layer1's 64-channel map of ONE image (19200
  // pixels, forward): 12.4 us as a graph node against 15.2 for the 64 x 64 tile kernel (tools/bench_c3_bs1.py); layer2's 4800 pixels: 20.9 against 18.2
  if (mode == 1 && k.M < 65536 && !(g.Cin == 64 && !g.dgrad && k.M >= 16384)) return false;
  if (k.out_bits || (k.mask_bits && !(d2 && k.N == 128 && al16(k.mask_bits)))) return false;      // mask bits: the stride-2 backward-data over 128 channels only
  r->family = FAM_C3S; r->dt_in = dtype_in; r->dt_out = dtype_out;
  r->ck = g.Cin; r->dgrad = g.dgrad != 0; r->d2 = d2; r->mask = k.mask != nullptr; r->bits = d2 && k.mask_bits != nullptr;
  const int KP = 9 * g.Cin + 8;
  const int nsl = k.N / C3_NSL, Bn = k.M / (g.OH * g.OW);
  int blocks, rows, nstrip;
  if (d2) {
    r->waves = 8;
    r->lds = (int64_t)C3_NSL * KP * 2;
    nstrip = (g.IW + 30) / 31;
    static const int env_rows = tune_env("GPV_C3D2_ROWS", 0);
    blocks = 256 / nsl;
    rows = env_rows > 0 ? env_rows : 2;
    if (env_rows <= 0) {
      const int64_t waves = (int64_t)blocks * r->waves;
      while (rows < 16 && (int64_t)Bn * nstrip * ((g.IH + rows + 1) / (rows + 2)) >= 2 * waves) rows += 2;
    }
    r->nseg = (g.IH + rows - 1) / rows;
  } else {
    static const int env_waves = tune_env("GPV_C3S_WAVES", 0);
    r->waves = env_waves == 4 ? 4 : (env_waves == 16 ? 16 : 8);
    r->lds = (int64_t)C3_NSL * KP * 2 + C3_NSL * (int64_t)sizeof(float);
    nstrip = (g.OW + 29) / 30;
    static const int env_blocks = tune_env("GPV_C3S_BLOCKS", 0);
    static const int env_rows = tune_env("GPV_C3R_ROWS", 0);
    blocks = env_blocks > 0 ? env_blocks : ((g.Cin == 64 ? 512 : 256) / nsl);
    // rows per item: a multiple of 3 such that the items fill the resident waves about twice (each segment re-reads two halo rows)
    rows = env_rows > 0 ? env_rows : 3;
    if (env_rows <= 0) {
      const int64_t waves = (int64_t)blocks * r->waves;
      while (rows < 30 && (int64_t)Bn * nstrip * ((g.OH + rows + 2) / (rows + 3)) >= 2 * waves) rows += 3;
    }
    r->nseg = (g.OH + rows - 1) / rows;
  }
  r->rows = rows; r->nstrip = nstrip;
  r->nitems = Bn * nstrip * r->nseg;
  while (blocks > 8 && (int64_t)(blocks - 8) * r->waves >= r->nitems) blocks -= 8;
  r->gx = (unsigned)blocks; r->gy = (unsigned)nsl; r->gz = 1; r->block = (unsigned)r->waves * 64;
  return true;
}

// ---- what the two direct-to-LDS tile kernels (gemm_pipe.hip, gemm_glds.hip) need of their operands -------------------------------
inline bool dlds_legal(const GemmK& k, int amode, int batch) {
  if (!al16(k.A) || !al16(k.B) || k.ldb % 8 != 0 || (batch > 1 && (k.sA % 8 != 0 || k.sB % 8 != 0))) return false;
  // 32-bit byte offsets into each operand (one buffer descriptor per operand and batch element)
  const int64_t lim = 0x7ffffff0ll / 2;
  if ((int64_t)k.N * k.ldb >= lim) return false;
  if (amode == OP_CONV) {
    if ((int64_t)k.cg.IH * k.cg.IW * k.cg.Cs * ((int64_t)k.M / ((int64_t)k.cg.OH * k.cg.OW) + 1) >= lim) return false;
    if (k.cg.Cin % GBK != 0 || k.cg.Cs % 8 != 0) return false;
  } else if (amode == OP_PLAIN) {
    if (k.lda % 8 != 0 || (int64_t)k.M * k.lda >= lim) return false;
  } else {
    return false;
  }
  return true;
}

// ---- gemm_pipe.hip: three-stage pipelined direct-to-LDS kernel, 8 waves, one block per CU, tile height picked per problem (bf16 -> bf16)
// rounds of 256 CUs a configuration needs, weighted by the tile's MFMA work; ties go to the larger tile (operand reuse)
inline int pipe_pick_cfg(const GemmK& k, int batch) {
  double best = 1e300;
  int bi = -1;
  for (int i = 0; i < kNumBig; ++i) {
    const int bm = kCfgs[i].bm, bn = kCfgs[i].bn;
    if (k.N % bn != 0) continue;
    const int64_t tiles = (int64_t)((k.M + bm - 1) / bm) * (k.N / bn) * batch;
    const int64_t rounds = (tiles + 255) / 256;
    // cost of a round ~ MFMA work of a tile + a term for the operand bytes it pulls from L2 (both per k-tile) + fixed per-tile overhead
    const double per_kt = (double)bm * bn / 16384.0 * 4.0 + (double)(bm + bn) * 128.0 / 56.0 / 16.0 * 0.5;
    const double cost = (double)rounds * (per_kt * (k.K / 64) + 40.0);
    if (cost < best - 1e-9) { best = cost; bi = i; }
  }
  return bi;
}

inline bool pipe_select(const GemmK& k, int amode, int dtype_in, int dtype_out, int batch, const Knobs& kn, Route* r) {
  const int mode = kn.pipe;
  if (mode == 0 || dtype_in != GPV_BF16 || dtype_out != GPV_BF16) return false;
  if (k.accumulate || k.split_k > 1) return false;
  if (k.K % GBK != 0 || k.K < 2 * GBK || k.N % 64 != 0) return false;
  if (!dlds_legal(k, amode, batch)) return false;
  if (mode < 100 && glds_two_per_cu(k, batch, kn)) return false;       // (gemm_glds.hip takes these: two half-width tiles per CU)
  int idx;
  if (mode >= 100) {
    idx = mode - 100;
    if (idx >= kNumCfgs || k.N % kCfgs[idx].bn != 0 || (idx >= kNumBig && amode != OP_PLAIN)) return false;
  } else if (kn.pipe_small && !k.no_small && amode == OP_PLAIN && !k.conv1x1 && k.K >= 256 &&
             (int64_t)((k.M + 63) / 64) * (k.N / 64) * batch <= 250 &&
             ((int64_t)((k.M + 63) / 64) * (k.N / 64) * batch >= 100 || k.K <= 1024)) {
    // small-M GEMMs (BERT and the co-attention text stream at M = 192, the text decoder at 640 rows): too few 64x64 tiles to
    // fill the chip.  6-8 k-tiles in flight through LDS-DMA instead of gemm_skinny.hip's one register-staged tile of
    // look-ahead: 9.0 -> 8.4 us (192x768x768), 10.6 -> 8.8 (192x2304x768), 19.0 -> 16.5 (3200x256x2048) -- modest: what
    // bounds these launches is the ~35 GB/s per CU of the operand path times the few CUs they occupy, not the look-ahead
    // (tools/bench_pipe.py small).  Very few tiles with a long reduction (192x768x3072) keep the in-block k-split of gemm_skinny.
    const int64_t t64 = (int64_t)((k.M + 63) / 64) * (k.N / 64) * batch;
    idx = t64 < 128 ? 7 : 6;
  } else {
    // Where it wins (tools/bench_pipe.py, B=32 shapes, round 2): reductions of >= 512 over 256..768-wide outputs of <= 40 k rows
    // (layer3/4 3x3 and long-K 1x1 convs fwd + dgrad, the DETR / co-attention GEMMs) and any width below 9600 rows.  N = 128
    // (layer2) and the >= 1024-wide outputs of >= 9600 rows stay on the two-blocks-per-CU 128x128 kernel (its 600-2400 tiles
    // balance better than 256-row rounds); the stride-2 dgrad parity classes are too uneven for one block per CU.
    if (k.K < 512 || k.M < 2048 || k.M > 40000 || k.N < 256) return false;
    if (amode == OP_CONV && k.cg.cm) return false;
    if (k.N >= 1024 && k.M >= 9600) return false;
    if ((int64_t)k.M * k.N * batch > (int64_t)24 << 20) return false;          // >= 1024 tiles of 256x256: the 8-wave 256x256 kernel (128 flop per operand byte)
    idx = pipe_pick_cfg(k, batch);
    if (idx < 0) return false;
  }
  if (idx < 0) return false;
  const PipeCfg& c = kCfgs[idx];
  r->family = FAM_PIPE; r->amode = amode; r->bmode = OP_PLAIN; r->dt_in = dtype_in; r->dt_out = dtype_out;
  r->cfg = idx; r->bm = c.bm; r->bn = c.bn;
  r->c11 = amode == OP_PLAIN && k.conv1x1;
  r->lds = (int64_t)c.ns * (c.bm + c.bn) * ROWB + (amode == OP_CONV ? (int64_t)c.bm * 4 : 0);
  r->tilesN = (k.N + c.bn - 1) / c.bn;
  static const int depi = tune_env("GPV_GLDS_DEPI", 1);
  r->depi = depi;
  r->gx = (unsigned)(((k.M + c.bm - 1) / c.bm) * r->tilesN); r->gy = 1; r->gz = (unsigned)batch; r->block = PIPE_THREADS;
  return true;
}

// ---- gemm_skinny.hip: 64x64 tiles with the reduction split across the block's four waves, for GEMMs whose tiles cannot
// fill the chip (M = 192..640 rows).  b_trans: B is reduction-major (GPV_TRANS): dX = dY W.
inline bool skinny_select(const GemmK& k, int b_trans, int dtype_in, int dtype_out, int batch, const Knobs& kn, Route* r) {
  if (kn.skinny == 0 || dtype_in != GPV_BF16 || batch != 1 || k.accumulate || k.split_k > 1) return false;
  if (k.K % 8 != 0 || k.lda % 8 != 0 || k.ldb % 8 != 0 || !al16(k.A) || !al16(k.B)) return false;
  if (b_trans && k.N % 8 != 0) return false;
  {   // 32-bit byte offsets into each operand
    const int64_t lim = 0x7ffffff0ll / 2;
    if ((int64_t)k.M * k.lda >= lim || (int64_t)(b_trans ? k.K : k.N) * k.ldb >= lim) return false;
  }
  if (kn.skinny == 1) {
    // measured on every forward GEMM shape of the step (tools/bench_step_gemms.py, SK=0 vs 2): it wins whenever the
    // 64x64 tiles cannot fill the chip (<= ~1.4 per CU), and up to 2.5 per CU when the reduction is long
    const int64_t tiles = (int64_t)((k.M + SBM - 1) / SBM) * ((k.N + SBN - 1) / SBN);
    // (the 360..640-tile, K >= 2048 launches -- 9600x256x2048, 3200x768x3072 -- go to the 4-wave direct-to-LDS kernel when B
    // is k-major: 54 -> 30 us, 52 -> 40 us; that kernel has no reduction-major B form, so dX = dY W keeps them here)
    if (!((tiles <= 360 && k.K >= 128) || (b_trans && tiles <= 640 && k.K >= 2048))) return false;
  }
  // Tile by measurement (tools/bench_skinny_pf.py, tools/ab_skinny_pf.sh; us at 64 x 64 | 32 x 64 | 32 x 32):
  //   300 x 256 x 2048 (20 tiles of 64 x 64) 14.2 | 10.4 | 7.8     100 x 768 x 3072 (24) 18.3 | 13.3 | 9.9     192 x 768 x 3072 (36) 18.3 | 13.2 | 11.3
  //   640 x 768 x 768 (120) 8.6 | 9.5 | 8.4     640 x 768 x 2048 (120) 15.3 | 15.6 | 15.3 (126 MB through L2 at 32 x 32: the L2s bound it)
  //   640 x 2304 x 768 (360) 12.5 | 11.0 | 12.3     640 x 2048 x 768 (320) 12.0 | 10.6 | 10.8     192 x 3072 x 768 (144) 8.4 | 9.1 | 8.4
  //   reduction-major B: 640 x 768 x 2048 16.8 | 12.6     640 x 768 x 2304 18.1 | 13.6     3200 x 256 x 2048 (200) 20.1 | 16.3
  // i.e. up to ~ 160 tiles of 64 x 64 the smallest tile (4 x as many CUs, half the bytes each), above that 32 x 64 (two co-resident blocks
  // per CU); batch-1 inference 4.88 -> 4.5 - 4.7 ms, train step -0.2 ms (same box, alternating twice).
  int pick = kn.skinny_tile;
  if (pick == 0) {
    const int64_t t64 = (int64_t)((k.M + 63) / 64) * ((k.N + 63) / 64);
    pick = (!b_trans && t64 <= 160) ? 3 : 2;
  }
  int bm = 64, bn = 64;
  if (pick == 2) { bm = 32; bn = 64; }
  else if (pick == 3 && !b_trans) { bm = 32; bn = 32; }
  r->family = FAM_SKINNY; r->amode = OP_PLAIN; r->bmode = b_trans ? OP_TRANS : OP_PLAIN; r->dt_in = dtype_in; r->dt_out = dtype_out == GPV_BF16 ? GPV_BF16 : GPV_F32;
  r->bm = bm; r->bn = bn;
  const int64_t stage = (int64_t)2 * (bm * SPITCH + (b_trans ? SBK * TPITCH : bn * SPITCH)) * 2;      // two stages x (A, B) tiles
  const int64_t redb = (int64_t)4 * bm * bn * 4;
  r->lds = stage > redb ? stage : redb;
  r->tilesN = (k.N + bn - 1) / bn;
  r->cfg = (k.K + SBK - 1) / SBK >= 2 ? 2 : 1;
  r->gx = (unsigned)(((k.M + bm - 1) / bm) * r->tilesN); r->gy = r->gz = 1; r->block = 256;
  return true;
}

// gemm_skinny.hip, weight-gradient form (both operands reduction-major), fp32 accumulate into C, optional a_rowsum
inline bool skinny_tt_select(const GemmK& k, int dtype_in, int dtype_out, int batch, const Knobs& kn, Route* r) {
  if (kn.skinny == 0 || dtype_in != GPV_BF16 || dtype_out != GPV_F32 || batch != 1 || !k.accumulate) return false;
  if (k.M % 8 != 0 || k.N % 8 != 0 || k.lda % 8 != 0 || k.ldb % 8 != 0 || k.ldc % 4 != 0) return false;
  if (!al16(k.A) || !al16(k.B) || !al16(k.C) || k.res || k.mask || k.bias || k.act || k.dthresh) return false;
  if ((int64_t)k.K * k.lda >= 0x7ffffff0ll / 2 || (int64_t)k.K * k.ldb >= 0x7ffffff0ll / 2) return false;   // 32-bit byte offsets
  const int64_t tiles = (int64_t)((k.M + SBM - 1) / SBM) * ((k.N + SBN - 1) / SBN);
  const int nk = (k.K + SBK - 1) / SBK;
  if (kn.skinny == 1 && (tiles > 256 || nk < 4)) return false;
  // enough splits for ~512 blocks, at least 3 k-steps of 128 each, within the lent workspace
  int split = (int)((512 + tiles - 1) / tiles);
  if (split > nk / 3) split = nk / 3;
  if (split < 1) split = 1;
  while (split > 1 && (k.ws_base == nullptr || (int64_t)split * k.M * k.N * 4 > k.ws_bytes)) --split;
  r->family = FAM_SKINNY_TT; r->amode = OP_TRANS; r->bmode = OP_TRANS; r->dt_in = dtype_in; r->dt_out = dtype_out;
  r->bm = SBM; r->bn = SBN;
  r->tilesN = (k.N + SBN - 1) / SBN;
  r->kt_per_split = (nk + split - 1) / split;
  r->split = (nk + r->kt_per_split - 1) / r->kt_per_split;
  r->two_pass = r->split > 1;
  const int64_t stage = (int64_t)2 * 2 * SBK * TPITCH * 2, redb = (int64_t)4 * SBM * SBN * 4;
  r->lds = stage > redb ? stage : redb;
  r->gx = (unsigned)tiles; r->gy = (unsigned)r->split; r->gz = 1; r->block = 256;
  return true;
}

// ---- gemm_glds.hip: 8-wave direct-to-LDS kernel, its 4-wave two-per-CU variants and the halo-image 3x3 kernel ---------------------
inline bool halo_ok(const GemmK& k, int dtype_out, int batch, const Knobs& kn) {
  const ConvGeom& g = k.cg;
  return kn.halo != 0 && dtype_out == GPV_BF16 && batch == 1 && g.KH == 3 && g.KW == 3 && g.SH == 1 && g.SW == 1 && g.PH == 1 && g.PW == 1 &&
         !g.cm && g.OH == g.IH && g.OW == g.IW && g.IW <= 47 && g.Cin % GBK == 0 && k.N % 128 == 0 && k.K == 9 * g.Cin &&
         k.M % (g.IH * g.IW) == 0 && k.ldc % 8 == 0 && al16(k.C) && (!k.res || (k.ldr % 8 == 0 && al16(k.res))) &&
         (!k.mask || (k.ldm % 8 == 0 && al16(k.mask))) && (!k.bias || al16(k.bias)) && !k.dthresh && k.act != GPV_ACT_GELU;
}

inline bool glds_select(const GemmK& k, int amode, int dtype_in, int dtype_out, int batch, const Knobs& kn, Route* r) {
  const int mode = kn.glds;     // 0 = never, 1 (default) = where it is expected to win, 2 / 3 = the 8-wave / 4-wave variant wherever legal
  if (mode == 0 || dtype_in != GPV_BF16) return false;
  if (k.accumulate || k.split_k > 1) return false;
  if (k.K % GBK != 0 || k.K < GBK || k.N <= 64) return false;
  if (!dlds_legal(k, amode, batch)) return false;
  int bm = 0, bn = 128;
  bool halo = false;
  // one-tile-per-CU launches (layer3 / layer4 at B = 32: 240 tiles of 160 x 256) serialise load ramp, main loop and store burst:
  // ~16 us of fixed cost on a 33-57 us kernel (tools/bench_ktile.py).  Half-width tiles at two blocks per CU (160 x 128: 480
  // tiles, 96 x 128 for the 9600-row maps) let one block's epilogue run under the other's main loop.
  if (glds_two_per_cu(k, batch, kn) && mode != 2 && mode != 3) {
    bm = two_per_cu_bm(k, batch, kn);
    // halo, 96-row tiles (layer4): forward 57.2 against 55.0 us, backward-data equal (tools/bench_c3_halo.py) -- tests only
    halo = amode == OP_CONV && halo_ok(k, dtype_out, batch, kn) && (bm == 160 || (bm == 96 && kn.halo >= 2));
  }
  if (bm == 0) {
    bn = k.N > 128 ? 256 : 128;
    bool small_tiles = mode == 3;
    if (mode == 1) {
      // Measured per shape on the ResNet-50 / transformer launches at B=32 (tools/bench_conv.py, bench_dgrad.py,
      // bench_gemm_sq.py with GPV_GLDS=0/2/3).  At 1-2 256-row tiles per CU the 8-wave kernel loses to kernels with 2-3
      // co-resident blocks (epilogues overlapped with other blocks' main loops, finer tail); it keeps the launches that fill the
      // chip several times over.  The 4-wave 128x128 variant wins wherever the reduction is long enough to amortise its
      // prologue/epilogue: every K >= 1024 conv / GEMM (layer3/4 3x3 fwd 94->82 / 150->76 us, their stride-2 dgrads
      // 194->139 / 161->101 us) and the K = 512 forward 1x1s; ReLU-mask (dgrad) epilogues need K >= 1024.
      const int64_t tiles = (int64_t)((k.M + GBM - 1) / GBM) * ((k.N + bn - 1) / bn) * batch;
      const bool huge = tiles >= 1024 && k.K >= 512 && !(amode == OP_CONV && k.cg.cm);   // parity classes: too unbalanced for 1 block/CU
      small_tiles = !huge && (k.K >= 1024 || (k.K >= 512 && !k.mask));
      if (!huge && !small_tiles) return false;
    }
    if (small_tiles) { bm = 128; bn = 128; }   // 4-wave 128x128 variant, two blocks per CU
    else bm = GBM;
  }
  r->amode = amode; r->bmode = OP_PLAIN; r->dt_in = dtype_in; r->bm = bm; r->bn = bn;
  r->gy = 1; r->gz = (unsigned)batch;
  if (halo) {
    r->family = FAM_HALO; r->dt_out = GPV_BF16;
    r->lds = (int64_t)(bm + 96) * ROWB + (int64_t)2 * 128 * ROWB;
    r->tilesN = k.N / 128;
    r->block = 256;
  } else {
    r->family = FAM_GLDS; r->dt_out = dtype_out == GPV_BF16 ? GPV_BF16 : GPV_F32;
    const int64_t stage = (int64_t)2 * (bm + bn) * ROWB, epi = (int64_t)(bm / 2) * (bn + 4) * 4;
    r->lds = stage > epi ? stage : epi;
    r->tilesN = (k.N + bn - 1) / bn;
    r->c11 = amode == OP_PLAIN && k.conv1x1;
    static const int depi = tune_env("GPV_GLDS_DEPI", 1);
    r->depi = depi;
    r->block = bm == 256 ? 512 : 256;
  }
  r->gx = (unsigned)(((k.M + bm - 1) / bm) * r->tilesN);
  return true;
}

// ---- gemm_glds_tt.hip: direct-to-LDS weight gradients (two-pass split reduction through k.ws_base) --------------------------------
// shared tail: split sizing over the workspace slabs
inline bool glds_tt_geometry(const GemmK& k, Route* r) {
  const int kt_total = (k.K + TBK - 1) / TBK;
  // two 64 KB blocks per CU = 512 resident blocks: size the split so that (tiles x splits) fills them once -- the 544 the
  // register-staged kernel (three blocks per CU) is tuned for would leave a second, almost empty round
  static const int target = tune_env("GPV_WGRAD_TARGET", 512);
  const int tiles = (k.M / TBM) * (k.N / TBN);
  int split = target / tiles;
  if (split > kt_total / 4) split = kt_total / 4;
  if (split < 2) return false;
  while (split > 2 && (int64_t)split * k.M * k.N * 4 > k.ws_bytes) --split;
  const int kt_per_split = (kt_total + split - 1) / split;
  split = (kt_total + kt_per_split - 1) / kt_per_split;
  if (split < 2 || (int64_t)split * k.M * k.N * 4 > k.ws_bytes) return false;
  r->split = split; r->kt_per_split = kt_per_split; r->two_pass = 1;
  r->tilesN = k.N / TBN;
  r->amode = OP_TRANS; r->dt_in = GPV_BF16; r->dt_out = GPV_F32; r->bm = TBM; r->bn = TBN;
  r->lds = 2 * TSTAGE;                    // 64 KB (the fp32 epilogue image needs 33 KB)
  r->gx = (unsigned)((k.M / TBM) * r->tilesN); r->gy = (unsigned)split; r->gz = 1; r->block = 256;
  return true;
}

// conv weight gradient (k as prepared by route_conv2d mode 2: A = dy [K][M], B = x NHWC, C = dw [M][N] fp32, split chosen)
inline bool glds_wgrad_select(const GemmK& k, int dtype_in, int dtype_out, const Knobs& kn, Route* r) {
  if (kn.wgrad == 0 || dtype_in != GPV_BF16 || dtype_out != GPV_F32) return false;
  const ConvGeom& g = k.cg;
  if (k.M % TBM != 0 || g.Cin % TBN != 0 || k.N % TBN != 0) return false;
  if (g.Cs % 8 != 0 || k.lda % 8 != 0 || !al16(k.A) || !al16(k.B)) return false;
  if (TBK / g.OW + 2 > g.OH || (int64_t)g.IH * g.IW * g.Cs * (k.K / (g.OH * g.OW)) >= (1ll << 30) ||
      (int64_t)k.K * k.lda >= (1ll << 30)) return false;
  if (!k.accumulate || k.ws_base == nullptr || !al16(k.C) || k.ldc % 4 != 0) return false;
  if (!glds_tt_geometry(k, r)) return false;
  r->family = FAM_GLDS_WGRAD; r->bmode = OP_CONV;
  return true;
}

// linear weight gradient dW[M][N] += dY^T X (A = dy [K][M], B = x [K][N], both reduction-major), optional a_rowsum (bias gradient)
inline bool glds_tt_select(const GemmK& k, int dtype_in, int dtype_out, int batch, const Knobs& kn, Route* r) {
  if (kn.wgrad == 0 || dtype_in != GPV_BF16 || dtype_out != GPV_F32 || batch != 1) return false;
  if (k.M % TBM != 0 || k.N % TBN != 0 || k.K < 8 * TBK) return false;
  if ((int64_t)k.K * k.lda >= (1ll << 30) || (int64_t)k.K * k.ldb >= (1ll << 30)) return false;
  // measured on every linear weight-gradient shape of the step (tools/bench_step_gemms.py, GPV_GLDS_WGRAD=0 vs 2): it wins
  // once there is enough work to fill the chip -- 768x3072 / 3072x768 over 3200 rows 52 -> 35 us, 1536x768 36 -> 26 us,
  // 2048x256 over 9600 rows 33 -> 27 us -- and loses on the 4..36-tile gradients of short reductions (skinny_tt's territory)
  if (kn.wgrad == 1 && (int64_t)(k.M / TBM) * (k.N / TBN) * ((k.K + TBK - 1) / TBK) < 3000) return false;
  if (k.lda % 8 != 0 || k.ldb % 8 != 0 || !al16(k.A) || !al16(k.B)) return false;
  if (!k.accumulate || k.ws_base == nullptr || !al16(k.C) || k.ldc % 4 != 0) return false;
  if (k.res || k.mask || k.bias || k.act || k.dthresh) return false;
  if (!glds_tt_geometry(k, r)) return false;
  r->family = FAM_GLDS_TT; r->bmode = OP_TRANS;
  return true;
}

// ---- gemm.hip: split forward convolution ------------------------------------------------------------------------------------------
// Forward convolutions over a few hundred to a few thousand output pixels (inference at batch 1: layer2-4 see 4800 / 1200 / 300
// pixels): 12..40 tiles of a 128-wide kernel walk K = 1152..4608 alone on a 256-CU chip.  The reduction is split over grid.y
// into fp32 slabs of the caller's workspace (64 x 64 tiles, ~300 workgroups of >= 8 k-tiles), a second launch sums the slabs and
// applies bias / residual / ReLU.
inline bool conv_split_select(const GemmK& k, int dtype_in, int dtype_out, const Knobs& kn, Route* r) {
  static const int on = tune_env("GPV_CONV_SPLIT", 1);
  if (!on || kn.forced() || dtype_in != GPV_BF16 || dtype_out != GPV_BF16 || !k.vecA || !k.vecB || !k.ws_base) return false;
  if (k.mask || k.rowscale || k.dthresh || k.accumulate || k.cg.dgrad || k.alpha != 1.0f || (k.act != 0 && k.act != GPV_ACT_RELU)) return false;
  if (k.N % 4 != 0 || k.ldc != k.N || (k.res && k.ldr != k.N) || !al16(k.C) || (k.res && !al16(k.res)) || (k.bias && !al16(k.bias))) return false;
  const int tiles = ((k.M + 63) / 64) * ((k.N + 63) / 64);
  const int kt_total = (k.K + BK - 1) / BK;
  if (tiles > 160 || kt_total < 32) return false;
  int split = (384 + tiles - 1) / tiles;
  if (split > kt_total / 8) split = kt_total / 8;
  if (split > 16) split = 16;
  while (split > 1 && (int64_t)split * k.M * k.N * 4 > k.ws_bytes) --split;
  if (split < 2) return false;
  r->family = FAM_CONV_SPLIT; r->amode = OP_CONV; r->bmode = OP_PLAIN; r->dt_in = GPV_BF16; r->dt_out = GPV_F32; r->bm = 64; r->bn = 64; r->vec = 1;
  r->tilesN = (k.N + 63) / 64;
  r->kt_per_split = (kt_total + split - 1) / split;
  r->split = (kt_total + r->kt_per_split - 1) / r->kt_per_split;
  r->two_pass = 1;
  r->lds = (int64_t)2 * (64 + 64) * LDK * 2;
  r->gx = (unsigned)tiles; r->gy = (unsigned)r->split; r->gz = 1; r->block = 256;
  return true;
}

// ---- gemm.hip: the register-staged 4-wave kernel, every mode incl. fp32 "precise": what nothing else took ---------------------------
// geometry of one BM x BN configuration: the split reduction and whether it goes through the workspace
inline void tile_geometry(const GemmK& k, int bm, int bn, int dtype_in, int dtype_out, int batch, Route* r) {
  r->bm = bm; r->bn = bn; r->dt_in = dtype_in; r->dt_out = dtype_out;
  r->vec = k.vecA && k.vecB;
  r->lds = (int64_t)2 * (bm + bn) * LDK * 2 * (dtype_in == GPV_F32 ? 2 : 1);
  const int tilesM = (k.M + bm - 1) / bm;
  r->tilesN = (k.N + bn - 1) / bn;
  const int kt_total = (k.K + BK - 1) / BK;
  int split = k.split_k < 1 ? 1 : k.split_k;
  if (split > kt_total) split = kt_total;
  r->kt_per_split = (kt_total + split - 1) / split;
  split = (kt_total + r->kt_per_split - 1) / r->kt_per_split;
  r->split = split;
  // Split reduction without atomics when the caller lent a workspace: every split writes its partial [M,N] product
  // with the normal coalesced epilogue, a second tiny kernel adds the slabs to C.  fp32 atomics on C cost
  // outputs x splits / ~94e9 s (67 us for the 128x512 gradient of a layer2 1x1 conv at its best split of 96).
  r->two_pass = k.accumulate && split > 1 && batch == 1 && k.ws_base != nullptr && dtype_out == GPV_F32 &&
                (int64_t)split * k.M * k.N * 4 <= k.ws_bytes && k.N % 4 == 0 && k.ldc % 4 == 0 && al16(k.C);
  const bool pp = r->amode == OP_PLAIN && r->bmode == OP_PLAIN;
  r->c11 = pp && k.conv1x1;
  r->nt = pp && dtype_in == GPV_BF16 && dtype_out == GPV_BF16 && r->vec && k.conv1x1 && k.nt_io && !k.dthresh && !r->two_pass;
  r->gx = (unsigned)(tilesM * r->tilesN); r->gy = (unsigned)split; r->gz = (unsigned)batch; r->block = 256;
}

inline bool tile_select(const GemmK& k, int amode, int bmode, int dtype_in, int dtype_out, int batch, const Knobs&, Route* r) {
  if (!((dtype_in == GPV_BF16 && (dtype_out == GPV_BF16 || dtype_out == GPV_F32)) || (dtype_in == GPV_F32 && dtype_out == GPV_F32))) return false;
  const int64_t sk = (k.split_k < 1 ? 1 : k.split_k);
  const int64_t t128 = (int64_t)((k.M + 127) / 128) * ((k.N + 127) / 128) * batch * sk;
  const int64_t t12864 = (int64_t)((k.M + 127) / 128) * ((k.N + 63) / 64) * batch * sk;
  static const int force = tune_env("GPV_FORCE_TILE", 0);   // tuning only
  int cfg;   // 0: 128x128, 1: 128x64, 2: 64x64
  if (force) cfg = force - 1;
  else if (k.K <= 256) cfg = (k.N >= 1024 && t128 >= 384 && !k.conv1x1) ? 0 : 2;   // <= 8 k-tiles: HBM/latency bound, 64x64 keeps more bytes in flight
                                                                      // (tools/bench_c3.py); the wide Linear outputs (FFN expansion) stay at 128x128, the
                                                                      // 1x1 convs since the buffer-load loaders do not: layer3 conv3 66 -> 61, conv1 dgrad 78 -> 65 us
  else if (k.N <= 64 && t12864 >= 384) cfg = 1;                       // N = 64 (layer1): 128x64, measured 100 vs 105 / 144 vs 151 us
  else if (k.N > 64 && t128 >= 384) cfg = 0;
  else if (t12864 >= 384) cfg = 1;
  else cfg = 2;
  r->family = FAM_TILE; r->amode = amode; r->bmode = bmode;
  tile_geometry(k, cfg == 0 ? 128 : (cfg == 1 ? 128 : 64), cfg == 0 ? 128 : 64, dtype_in, dtype_out, batch, r);
  return true;
}

// conv weight gradient on the register-staged kernel (B = gathered activations)
// CONVT needs every N tile inside one tap: BN divides Cin (64 always does here; 128 when Cin % 128 == 0)
inline bool tile_wgrad_select(const GemmK& k, int dtype_in, const Knobs&, Route* r) {
  static const int wforce = tune_env("GPV_FORCE_WGRAD_TILE", 0);   // tuning only
  int bm = 64, bn = 64;
  if (dtype_in == GPV_BF16) {
    const int split = k.split_k;
    const bool can128 = (k.cg.Cin % 128 == 0) && k.M >= 128;
    int cfg;   // 0: 128x128, 1: 128x64, 2: 64x64
    if (wforce) cfg = wforce - 1;
    else if (can128 && (int64_t)((k.M + 127) / 128) * (k.N / 128) * split >= 256) cfg = 0;
    else if (k.M >= 128 && (int64_t)((k.M + 127) / 128) * (k.N / 64) * split >= 384) cfg = 1;
    else cfg = 2;
    if (cfg == 0 && can128) { bm = 128; bn = 128; }
    else if (cfg <= 1 && k.M >= 128) { bm = 128; bn = 64; }
  }
  r->family = FAM_TILE; r->amode = OP_TRANS; r->bmode = OP_CONV;
  tile_geometry(k, bm, bn, dtype_in == GPV_BF16 ? GPV_BF16 : GPV_F32, GPV_F32, 1, r);
  return true;
}

// ---- the order in which the families are tried, stated once ---------------------------------------------------------------------------
// `tries`: the families the call site admits (bit FAM_*); the first admitted family whose select accepts takes the call.  A select
// writes into the Route only after its last reject, so a family that declines leaves the zeroed Route to the next one.
// ws / ws_bytes: the workspace a forward convolution lent (the split forward conv only; its GemmK then carries it).
struct RouteCall { int amode, bmode, dtype_in, dtype_out, batch; bool linear; void* ws; int64_t ws_bytes; };
inline bool route_try(GemmK* k, const RouteCall& c, unsigned tries, const Knobs& kn, Route* r) {
  auto on = [&](int f) { return (tries >> f) & 1u; };
  *r = Route{};
  if (on(FAM_GEMV) && gemv_select(*k, c.dtype_in, c.dtype_out, c.batch, kn, r)) return true;                 // M <= 8: matrix-vector products of the decode step
  if (on(FAM_C1S) && c1s_select(*k, c.dtype_in, c.dtype_out, c.linear, kn, r)) return true;                   // weights resident in LDS, rows streamed (K = 256 -> >= 1536 features from gpv_gemm)
  if (on(FAM_C3S) && c3s_select(*k, c.dtype_in, c.dtype_out, kn, r)) return true;                             // 3x3 with 64 / 128 input channels over the layer1 / layer2 maps: weights resident in LDS, barrier-free streaming kernel
  if (on(FAM_CONV_SPLIT)) {                                                                                   // few output pixels, long reduction (inference at batch 1): split + second pass
    GemmK ks = *k;
    ks.ws_base = c.ws; ks.ws_bytes = c.ws_bytes;
    if (conv_split_select(ks, c.dtype_in, c.dtype_out, kn, r)) { *k = ks; return true; }
  }
  if (on(FAM_PIPE) && pipe_select(*k, c.amode, c.dtype_in, c.dtype_out, c.batch, kn, r)) return true;         // pipelined direct-to-LDS kernel (big tiles, and the small-M 6-8 stage tiles)
  if (on(FAM_SKINNY) && skinny_select(*k, c.bmode == OP_TRANS, c.dtype_in, c.dtype_out, c.batch, kn, r)) return true;   // few tiles, long reduction: what the pipelined kernel does not take (fp32 outputs, ragged N); small backward-data GEMMs
  if (on(FAM_GLDS) && glds_select(*k, c.amode, c.dtype_in, c.dtype_out, c.batch, kn, r)) return true;         // 8-wave direct-to-LDS kernel when it qualifies (and its two-per-CU and halo forms)
  if (on(FAM_GLDS_WGRAD) && glds_wgrad_select(*k, c.dtype_in, c.dtype_out, kn, r)) return true;               // conv weight gradient: 128-multiples of Cout / Cin with a workspace split reduction
  if (on(FAM_GLDS_TT) && glds_tt_select(*k, c.dtype_in, c.dtype_out, c.batch, kn, r)) return true;            // linear weight gradient: 128-multiples, long reduction
  if (on(FAM_SKINNY_TT) && skinny_tt_select(*k, c.dtype_in, c.dtype_out, c.batch, kn, r)) return true;        // small weight gradients: reduction split over the block's waves
  if (on(FAM_TILE)) {
    if (c.bmode == OP_CONV) return tile_wgrad_select(*k, c.dtype_in, kn, r);
    return tile_select(*k, c.amode, c.bmode, c.dtype_in, c.dtype_out, c.batch, kn, r);
  }
  return false;
}
constexpr unsigned fam(int f) { return 1u << f; }
constexpr unsigned kDldsTiles = fam(FAM_PIPE) | fam(FAM_GLDS) | fam(FAM_TILE);      // the tile kernels every K-major x K-major call may end on

inline void route_fail(Routed* out, int err) { out->err = err; out->nparts = 0; }

// ---- gpv_gemm ------------------------------------------------------------------------------------------------------------------------
inline void route_gemm(const gpv_gemm_args* a, const Knobs& kn, Routed* out) {
  out->err = 0; out->nparts = 1;
  if (!a || !a->A || !a->B || !a->C || a->M <= 0 || a->N <= 0 || a->K <= 0 || a->batch <= 0) return route_fail(out, kRouteInvalid);
  if ((a->split_k > 1 || a->accumulate) && a->dtype_out != GPV_F32) return route_fail(out, kRouteInvalid);
  if (a->split_k > 1 && (!a->accumulate || a->bias || a->res || a->act || a->relu_mask || a->drop_p > 0.f)) return route_fail(out, kRouteInvalid);
  out->batch = a->batch;
  GemmK& k = out->k[0];
  k = GemmK{};
  k.A = a->A; k.B = a->B; k.C = a->C; k.M = a->M; k.N = a->N; k.K = a->K;
  k.lda = a->lda; k.ldb = a->ldb; k.ldc = a->ldc; k.sA = a->sA; k.sB = a->sB; k.sC = a->sC;
  k.alpha = a->alpha; k.rowscale = a->rowscale; k.bias = a->bias;
  k.res = a->res; k.ldr = a->ldr; k.sR = a->sR; k.mask = a->relu_mask; k.ldm = a->ldm;
  k.act = a->act; k.seed = a->seed;
  k.dthresh = a->drop_p > 0.f ? drop_thresh(a->drop_p) : 0u;
  k.dscale = a->drop_p > 0.f ? 1.0f / (1.0f - a->drop_p) : 1.0f;
  k.accumulate = a->accumulate; k.split_k = a->split_k;
  k.a_rowsum = a->a_rowsum;
  k.no_small = (a->flags & GPV_GEMM_NO_PIPE_SMALL) ? 1 : 0;
  k.ws_base = a->workspace; k.ws_bytes = a->workspace ? a->workspace_bytes : 0;
  if (k.a_rowsum && !(a->layoutA == GPV_TRANS && a->layoutB == GPV_TRANS && a->batch == 1)) return route_fail(out, kRouteInvalid);
  if (a->accumulate && a->split_k <= 1 && !a->res) {
    // one block owns every output element: C += acc as a coalesced read-modify-write through the LDS epilogue
    // (fp32 atomics run at ~70 G/s: a 10000x768 gradient costs 110 us in atomics alone)
    k.accumulate = 0; k.res = a->C; k.ldr = a->ldc; k.sR = a->sC;
  }
  const int esz = a->dtype_in == GPV_F32 ? 4 : 2;
  const int64_t vecel = 16 / esz;  // elements per 16 B
  auto vec_ok = [&](const void* ptr, int64_t ld, int64_t bs, int layout, int extent_contig) {
    bool ok = al16(ptr) && (ld % vecel == 0) && (a->batch == 1 || bs % vecel == 0);
    // 16-byte chunks: the contiguous extent must be a multiple of 8, or end inside the row pitch -- a reduction-major
    // operand's last chunk then only feeds outputs beyond M / N (discarded); a k-major operand's last chunk multiplies
    // masked rows of the other operand, so its padding must be finite (caller's promise: GPV_GEMM_KPAD_FINITE)
    if (layout == GPV_KMAJOR) ok = ok && (a->K % 8 == 0 || ((a->flags & GPV_GEMM_KPAD_FINITE) && ld >= ((int64_t)a->K + 7) / 8 * 8));
    else ok = ok && (extent_contig % 8 == 0 || ld >= ((int64_t)extent_contig + 7) / 8 * 8);
    return ok ? 1 : 0;
  };
  k.vecA = vec_ok(a->A, a->lda, a->sA, a->layoutA, a->M);
  k.vecB = vec_ok(a->B, a->ldb, a->sB, a->layoutB, a->N);
  {   // the 16-byte path addresses an operand (one batch element) with 32-bit byte offsets
    const int64_t lim = 0x7ffffff0ll / esz;
    if ((int64_t)(a->layoutA == GPV_KMAJOR ? a->M : a->K) * a->lda >= lim) k.vecA = 0;
    if ((int64_t)(a->layoutB == GPV_KMAJOR ? a->N : a->K) * a->ldb >= lim) k.vecB = 0;
  }
  const int la = a->layoutA, lb = a->layoutB;
  RouteCall c{OP_PLAIN, OP_PLAIN, a->dtype_in, a->dtype_out, a->batch, true, nullptr, 0};
  Route* r = &out->r[0];
  bool ok = false;
  if (la == GPV_KMAJOR && lb == GPV_KMAJOR) {
    static const bool c1s_linear = tune_env("GPV_C1S_LINEAR", 1) != 0;     // 0: A/B only
    ok = route_try(&k, c, fam(FAM_GEMV) | (a->batch == 1 && !kn.forced() && c1s_linear ? fam(FAM_C1S) : 0u) | fam(FAM_SKINNY) | kDldsTiles, kn, r);
  } else if (la == GPV_KMAJOR && lb == GPV_TRANS) {
    c.bmode = OP_TRANS;
    ok = route_try(&k, c, fam(FAM_SKINNY) | fam(FAM_TILE), kn, r);
  } else if (la == GPV_TRANS && lb == GPV_TRANS) {
    c.amode = OP_TRANS; c.bmode = OP_TRANS;
    if (a->accumulate) {
      GemmK kk = k;
      kk.accumulate = 1; kk.res = nullptr; kk.ldr = 0; kk.sR = 0;      // (the split==1 rewrite above turned C += into res = C)
      ok = route_try(&kk, c, fam(FAM_GLDS_TT) | fam(FAM_SKINNY_TT), kn, r);
      if (ok) k = kk;
    }
    if (!ok) ok = route_try(&k, c, fam(FAM_TILE), kn, r);
  }
  if (!ok) route_fail(out, kRouteInvalid);
}

// ---- gpv_conv2d (modes 0, 1, 2) ------------------------------------------------------------------------------------------------------
inline void route_conv2d(const gpv_conv_args* a, const Knobs& kn, Routed* out) {
  out->err = 0; out->nparts = 1; out->batch = 1;
  if (!a || !a->x || !a->w || !a->y) return route_fail(out, kRouteInvalid);
  if (a->Cin % 32 != 0) return route_fail(out, kRouteInvalid);
  if ((a->SH != 1 && a->SH != 2) || (a->SW != 1 && a->SW != 2)) return route_fail(out, kRouteInvalid);
  const bool want_bits = a->y_mask_bits != nullptr || a->relu_mask_bits != nullptr;
  const bool pw1 = a->KH == 1 && a->KW == 1 && a->SH == 1 && a->SW == 1 && a->PH == 0 && a->PW == 0 && a->IH == a->OH && a->IW == a->OW;
  if (want_bits) {
    // one-bit ReLU masks: the streaming 1x1 kernel only (stride 1, pointwise), forward with ReLU writes them, backward-data reads them
    const bool d3s2 = a->mode == 1 && a->KH == 3 && a->KW == 3 && a->SH == 2 && a->SW == 2 && a->PH == 1 && a->PW == 1 && a->Cout == 128 && !a->y_mask_bits;
    if (!pw1 && !d3s2) return route_fail(out, kRouteInvalid);
    if ((pw1 && a->Cout % 256 != 0) || (a->y_mask_bits && (a->mode != 0 || a->act != GPV_ACT_RELU || a->relu_mask)) || (a->relu_mask_bits && a->mode != 1)) return route_fail(out, kRouteInvalid);
    if ((reinterpret_cast<uintptr_t>(a->y_mask_bits) | reinterpret_cast<uintptr_t>(a->relu_mask_bits)) & 15) return route_fail(out, kRouteInvalid);
  }
  GemmK& k = out->k[0];
  k = GemmK{};
  k.alpha = 1.0f; k.rowscale = a->rowscale; k.bias = a->bias; k.act = a->act;
  k.cg = ConvGeom{a->IH, a->IW, a->Cs, a->Cin, a->OH, a->OW, a->KH, a->KW, a->SH, a->SW, a->PH, a->PW, a->mode == 1, 0, 0};
  if (a->mode == 1 && a->SH == 2 && a->SW == 2 && a->OH % 2 == 0 && a->OW % 2 == 0) {
    // stride-2 dgrad: only taps with r = (ih+PH) mod 2, s = (iw+PW) mod 2 contribute.  Order the rows by pixel parity
    // class so that a tile is class-uniform and skips the other taps (2.25 of 9 on average for a 3x3, 1 of 4 pixels for a 1x1)
    k.cg.cm = 1;
    k.cg.cls_rows = a->B * (a->OH / 2) * (a->OW / 2);
  }
  const int T = a->KH * a->KW;
  const int esz = a->dtype_in == GPV_F32 ? 4 : 2;
  const int64_t vecel = 16 / esz;
  RouteCall c{OP_CONV, OP_PLAIN, a->dtype_in, a->dtype_out, 1, false, nullptr, 0};
  Route* r = &out->r[0];
  if (a->mode == 0 || a->mode == 1) {
    // rows = B*OH*OW output positions, N = Cout, K = T*Cin ; A = gather(x), B = w [Cout][T*Cin]
    k.A = a->x; k.B = a->w; k.C = a->y;
    k.M = a->B * a->OH * a->OW; k.N = a->Cout; k.K = T * a->Cin;
    k.lda = 0; k.ldb = k.K; k.ldc = a->Cout;
    k.res = a->res; k.ldr = a->Cout; k.mask = a->relu_mask; k.ldm = a->Cout;
    k.vecA = al16(a->x) && (a->Cs % vecel == 0 || (a->Cs * esz) % 8 == 0) ? 1 : 0;
    // the stem reads 16-B runs at pixel granularity (Cs = 4 bf16 = 8 B): require 16-B aligned runs
    if ((a->Cs % vecel) != 0) k.vecA = ((a->SW * a->Cs) % vecel == 0 && (a->IW * a->Cs) % vecel == 0 && a->PW == 0) ? k.vecA : 0;
    k.vecB = al16(a->w) && (k.K % 8 == 0) ? 1 : 0;
    if (a->mode == 0 && a->KH == 1 && a->KW == 1 && a->SH == 2 && a->SW == 2 && a->PH == 0 && a->PW == 0 &&
        al16(a->x) && a->Cs % vecel == 0 && (int64_t)a->B * a->IH * a->IW * a->Cs * esz < 0x7ffffff0ll * 4ll) {
      // stride-2 pointwise projection (the downsample branches), forward: the streaming kernel reads every other pixel of every
      // other row (conv1x1_stream.hip); anything it does not take goes down the generic gather path below
      GemmK ks = k;
      ks.lda = a->Cs; ks.vecA = 1;
      if (route_try(&ks, c, fam(FAM_C1S), kn, r)) { k = ks; return; }
    }
    if (pw1) {
      // a 1x1 stride-1 convolution IS a GEMM over the pixel rows (row pitch Cs): no tap / pixel decoding per thread
      // (three integer divisions per staged row -- a third of the instructions of a K = 64 tile), and the GEMM-side
      // kernel choices apply
      k.lda = a->Cs;
      k.cg = ConvGeom{};
      k.cg.SH = k.cg.SW = 1;
      k.conv1x1 = 1;
      {
        // outputs far beyond the 256 MB MALL (layer1's 314 MB maps) are stored -- and their residual read -- non-temporally:
        // 64 -> 256 without a residual 150 -> 106 us, with one 177 -> 168 us; smaller outputs are better left cacheable for
        // the next convolution (layer3 conv3, 79 MB: 58 -> 72 us with non-temporal stores)   [tools/bench_c1.py]
        static const int64_t nt_min = (int64_t)tune_env("GPV_NT_MIN_MB", 200) << 20;
        k.nt_io = (int64_t)k.M * k.N * esz >= nt_min ? 1 : 0;
      }
      k.vecA = al16(a->x) && (a->Cs % vecel == 0) && (int64_t)k.M * a->Cs * esz < 0x7ffffff0ll ? 1 : 0;
      c.amode = OP_PLAIN;
      if (want_bits) {
        if (!k.vecA) return route_fail(out, kRouteInvalid);
        k.out_bits = reinterpret_cast<uint32_t*>(a->y_mask_bits);
        k.mask_bits = reinterpret_cast<const uint32_t*>(a->relu_mask_bits);
        if (k.mask_bits) { k.mask = a->relu_mask_bits; k.ldm = a->Cout; }      // (selects the masked instances; never dereferenced as bf16)
        if (!route_try(&k, c, fam(FAM_C1S), kn, r)) route_fail(out, kRouteInvalid);
        return;
      }
      // skinny: a few thousand pixels (inference at batch 1): 64x64 tiles, reduction split over the block's waves
      if (!route_try(&k, c, (k.vecA ? fam(FAM_C1S) : 0u) | (k.M <= 8192 && !kn.forced() ? fam(FAM_SKINNY) : 0u) | kDldsTiles, kn, r)) route_fail(out, kRouteInvalid);
      return;
    }
    static const bool s2_split = tune_env("GPV_S2_DGRAD_SPLIT", 1) != 0;
    if (s2_split && a->mode == 1 && k.cg.cm && a->KH == 1 && a->KW == 1 && a->PH == 0 && a->PW == 0 && a->dtype_in == GPV_BF16 &&
        a->dtype_out == GPV_BF16 && a->Cout % 8 == 0 && al16(a->y) && (!a->res || al16(a->res)) &&
        (!a->relu_mask || al16(a->relu_mask)) && k.vecA && k.vecB) {
      // pointwise stride-2 backward-data: class 0 (even row, even column) through the GEMM kernels, the rest element-wise
      // (gemm.hip s2_dgrad_fill_kernel: 8 channels per thread over all B * OH * OW pixels)
      out->k[1] = k;
      k.M = k.cg.cls_rows;
      if (!route_try(&k, c, kDldsTiles, kn, r)) return route_fail(out, kRouteInvalid);
      Route& f = out->r[1];
      f = Route{};
      f.family = FAM_S2_FILL; f.dt_in = f.dt_out = GPV_BF16;
      f.ncols = a->Cout / 8;
      f.gx = (unsigned)(((int64_t)a->B * a->OH * a->OW * f.ncols + 255) / 256); f.gy = f.gz = 1; f.block = 256;
      out->nparts = 2;
      return;
    }
    if (want_bits) {
      // (not the pointwise form, which returned above: the stride-2 3x3 backward-data over 128 channels on the streaming kernel, or nothing)
      if (!(a->KH == 3 && a->KW == 3 && k.vecA && k.vecB)) return route_fail(out, kRouteInvalid);
      k.mask_bits = reinterpret_cast<const uint32_t*>(a->relu_mask_bits);
      k.mask = a->relu_mask_bits; k.ldm = a->Cout;
      if (!route_try(&k, c, fam(FAM_C3S), kn, r)) route_fail(out, kRouteInvalid);
      return;
    }
    const bool vec = k.vecA && k.vecB;
    c.ws = a->workspace; c.ws_bytes = a->workspace_bytes;
    if (!route_try(&k, c, (a->KH == 3 && a->KW == 3 && vec ? fam(FAM_C3S) : 0u) | (vec && a->mode == 0 && a->workspace ? fam(FAM_CONV_SPLIT) : 0u) |
                              (vec ? fam(FAM_PIPE) | fam(FAM_GLDS) : 0u) | fam(FAM_TILE), kn, r)) route_fail(out, kRouteInvalid);
    return;
  }
  if (a->mode == 2) {
    // dw[Cout][T*Cin] += dy^T x_gather : M = Cout, N = T*Cin, K = B*OH*OW
    if (a->dtype_out != GPV_F32) return route_fail(out, kRouteInvalid);
    if (a->Cin % 64 != 0) return route_fail(out, kRouteInvalid);
    k.A = a->w /* dy */; k.B = a->x; k.C = a->y /* dw */;
    k.M = a->Cout; k.N = T * a->Cin; k.K = a->B * a->OH * a->OW;
    k.lda = a->Cout; k.ldb = 0; k.ldc = k.N;
    k.accumulate = 1;
    int split = a->split_k;
    if (split < 1) {
      const int kt = (k.K + BK - 1) / BK;
      int64_t want;
      if (a->workspace && a->Cin % 128 == 0 && k.M >= 128) {
        // two-pass reduction (no atomics): ~2 blocks of 128x128 per CU is the measured optimum on the layer2-4 shapes
        // (tools/bench_split_conv.py: 64..96 / 64 / 32 / 16 / 8 / 4 splits for 4 / 9 / 16 / 36 / 64 / 144 tiles)
        const int64_t t128 = (int64_t)((k.M + 127) / 128) * (k.N / 128);
        want = (544 + t128 / 2) / t128;
        if (want > 288) want = 288;
        while (want > 1 && want * (int64_t)k.M * k.N * 4 > a->workspace_bytes) --want;
      } else {
        const int64_t tiles = (int64_t)((k.M + 63) / 64) * ((k.N + 63) / 64);
        want = 1536 / (tiles > 0 ? tiles : 1);
      }
      if (want > kt / 8) want = kt / 8;
      split = want < 1 ? 1 : (int)want;
    }
    k.split_k = split;
    if (split <= 1) { k.accumulate = 0; k.res = a->y; k.ldr = k.ldc; }
    k.ws_base = a->workspace; k.ws_bytes = a->workspace ? a->workspace_bytes : 0;
    k.vecA = al16(a->w) && (a->Cout % vecel == 0) ? 1 : 0;
    k.vecB = al16(a->x) && (a->Cs % vecel == 0) ? 1 : 0;
    c.amode = OP_TRANS; c.bmode = OP_CONV;
    // direct-to-LDS kernel (gemm_glds_tt.hip): 128-multiples of Cout / Cin with a workspace split reduction; else the register-staged one
    if (!route_try(&k, c, fam(FAM_GLDS_WGRAD) | fam(FAM_TILE), kn, r)) route_fail(out, kRouteInvalid);
    return;
  }
  route_fail(out, kRouteInvalid);
}

}  // namespace gpvk
