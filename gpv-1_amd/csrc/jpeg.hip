// Baseline JPEG decoding for the device-side input pipeline: what `skio.imread(img_path)` does in the reference's
// 30 data-loader workers (datasets/coco_generic_dataset.py:54, datasets/coco_datasets.py:157 -> Pillow -> libjpeg-turbo with its
// defaults: accurate integer IDCT, "fancy" chroma upsampling, YCbCr -> RGB).
//
// The split follows the data: entropy decoding is a serial walk over a bit stream (one image per host thread, gpv_jpeg_parse: a
// few ms per COCO image; jpeg_host.h holds it, plain C++ shared with libgpv_huff.so's host pass), everything after it is per-block / per-pixel integer arithmetic and runs on the GPU for the whole batch
// in two launches (gpv_jpeg_decode):
//   jpeg_idct_kernel   quantised coefficients -> dequantise -> IJG jidctint.c 8x8 inverse DCT (8 lanes per block: a lane owns a
//                      column in pass 1, a row in pass 2, the transpose goes through LDS) -> component planes (uint8)
//   jpeg_color_kernel  per output pixel: chroma through the IJG triangle filter (h2v1 / h2v2 "fancy" upsampling, evaluated on the
//                      fly from the chroma planes) -> jdcolor.c fixed-point YCbCr -> RGB -> [H][W][3] uint8, the input of
//                      gpv_image_pipeline.  A single-component file is replicated to three channels (coco_generic_dataset.py:55-56).
// Bit-exact against the Pillow decoder on the fixtures of tests/golden/jpeg (tests/test_jpeg_gpu.py); oracle/jpeg_oracle.py is the
// CPU restatement.  Scope: baseline sequential (SOF0/SOF1 Huffman), 8 bit, one interleaved scan, 1 or 3 components, luma 1x1 / 2x1 /
// 2x2 over 1x1 chroma, restart intervals; anything else returns hipErrorNotSupported and the caller must convert the file.
#include "common.h"
#include "../../include/gpv_hip.h"
#include "jpeg_host.h"

extern "C" int gpv_jpeg_parse(const unsigned char* data, int64_t nbytes, gpv_jpeg_info* info, short* coefs, int64_t coefs_capacity) {
  static thread_local gpv_jpeg_host::Frame frame;        // (too large for the stack of a pool thread)
  return gpv_jpeg_host::parse(data, nbytes, info, coefs, coefs_capacity, frame);
}

// ------------------------------------------------------------------ device side ------------------------------------------------------
namespace {

constexpr int CB = 13, P1 = 2;
constexpr int F_0_298 = 2446, F_0_390 = 3196, F_0_541 = 4433, F_0_765 = 6270, F_0_899 = 7373, F_1_175 = 9633;
constexpr int F_1_501 = 12299, F_1_847 = 15137, F_1_961 = 16069, F_2_053 = 16819, F_2_562 = 20995, F_3_072 = 25172;

// IJG jidctint.c, one 1-D pass (32-bit arithmetic as in the C source: 8-bit samples keep every intermediate below 2^31)
template <int SHIFT>
__device__ __forceinline__ void idct_1d(const int* in, int* out) {
  int z1 = (in[2] + in[6]) * F_0_541;
  const int t2 = z1 - in[6] * F_1_847;
  const int t3 = z1 + in[2] * F_0_765;
  const int t0 = (in[0] + in[4]) << CB;
  const int t1 = (in[0] - in[4]) << CB;
  const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int o0 = in[7], o1 = in[5], o2 = in[3], o3 = in[1];
  z1 = o0 + o3;
  int z2 = o1 + o2, z3 = o0 + o2, z4 = o1 + o3;
  const int z5 = (z3 + z4) * F_1_175;
  o0 *= F_0_298; o1 *= F_2_053; o2 *= F_3_072; o3 *= F_1_501;
  z1 *= -F_0_899; z2 *= -F_2_562; z3 = z3 * -F_1_961 + z5; z4 = z4 * -F_0_390 + z5;
  o0 += z1 + z3; o1 += z2 + z4; o2 += z2 + z3; o3 += z1 + z4;
  constexpr int R = 1 << (SHIFT - 1);
  out[0] = (t10 + o3 + R) >> SHIFT; out[7] = (t10 - o3 + R) >> SHIFT;
  out[1] = (t11 + o2 + R) >> SHIFT; out[6] = (t11 - o2 + R) >> SHIFT;
  out[2] = (t12 + o1 + R) >> SHIFT; out[5] = (t12 - o1 + R) >> SHIFT;
  out[3] = (t13 + o0 + R) >> SHIFT; out[4] = (t13 - o0 + R) >> SHIFT;
}

// 256 threads = 32 blocks of 8x8; blockIdx.y = image
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const gpv_jpeg_desc* __restrict__ descs) {
  __shared__ int ws[32][8][9];
  const gpv_jpeg_desc& d = descs[blockIdx.y];
  const int tid = threadIdx.x, lb = tid >> 3, t = tid & 7;
  int nb[3], total = 0;
  for (int c = 0; c < d.ncomp; ++c) { nb[c] = d.bh[c] * d.bw[c]; total += nb[c]; }
  int b = blockIdx.x * 32 + lb;
  const bool live = b < total;
  int c = 0;
  if (live) { while (b >= nb[c]) { b -= nb[c]; ++c; } }
  if (live) {
    const short* blk = d.coefs + d.coef_off[c] + (int64_t)b * 64;
    int in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = (int)blk[k * 8 + t] * (int)d.quant[c][k * 8 + t];      // column t
    idct_1d<CB - P1>(in, out);
#pragma unroll
    for (int k = 0; k < 8; ++k) ws[lb][k][t] = out[k];
  }
  __syncthreads();
  if (live) {
    int in[8], out[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) in[k] = ws[lb][t][k];                                            // row t
    idct_1d<CB + P1 + 3>(in, out);
    const int by = b / d.bw[c], bx = b - by * d.bw[c];
    unsigned char* dst = d.planes + d.plane_off[c] + (int64_t)(by * 8 + t) * (d.bw[c] * 8) + bx * 8;
    uint2 v;
    unsigned char* q = reinterpret_cast<unsigned char*>(&v);
#pragma unroll
    for (int k = 0; k < 8; ++k) { const int s = out[k] + 128; q[k] = (unsigned char)(s < 0 ? 0 : (s > 255 ? 255 : s)); }
    *reinterpret_cast<uint2*>(dst) = v;                                                          // (rows of a plane are 8-byte aligned)
  }
}

__device__ __forceinline__ int chroma_at(const unsigned char* pl, int pitch, int cw, int ch, int hs, int vs, int y, int x) {
  if (hs == 1) return pl[(int64_t)y * pitch + x];
  const int c = x >> 1;
  if (cw <= 2) return pl[(int64_t)(vs == 2 ? y >> 1 : y) * pitch + c];     // jdsample.c: fancy upsampling needs downsampled_width > 2; replication below
  if (vs == 1) {                                       // h2v1 fancy: 3/4 nearer + 1/4 further column
    const unsigned char* r = pl + (int64_t)y * pitch;
    const int a = r[c];
    if (x & 1) return c == cw - 1 ? a : (a * 3 + r[c + 1] + 2) >> 2;
    return c == 0 ? a : (a * 3 + r[c - 1] + 1) >> 2;
  }
  const int r0 = y >> 1;                               // h2v2 fancy: the triangle filter in both directions
  int r1 = (y & 1) ? r0 + 1 : r0 - 1;
  r1 = r1 < 0 ? 0 : (r1 > ch - 1 ? ch - 1 : r1);
  const unsigned char* a = pl + (int64_t)r0 * pitch;
  const unsigned char* n = pl + (int64_t)r1 * pitch;
  const int cs = a[c] * 3 + n[c];
  if (x & 1) return c == cw - 1 ? (cs * 4 + 7) >> 4 : (cs * 3 + a[c + 1] * 3 + n[c + 1] + 7) >> 4;
  return c == 0 ? (cs * 4 + 8) >> 4 : (cs * 3 + a[c - 1] * 3 + n[c - 1] + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_color_kernel(const gpv_jpeg_desc* __restrict__ descs) {
  const gpv_jpeg_desc& d = descs[blockIdx.y];
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)d.width * d.height) return;
  const int y = (int)(i / d.width), x = (int)(i - (int64_t)y * d.width);
  const int Y = d.planes[d.plane_off[0] + (int64_t)y * (d.bw[0] * 8) + x];
  unsigned char* o = d.out + i * 3;
  if (d.ncomp == 1) { o[0] = o[1] = o[2] = (unsigned char)Y; return; }
  const int cw = (d.width + d.hmax - 1) / d.hmax, ch = (d.height + d.vmax - 1) / d.vmax;
  const int cb = chroma_at(d.planes + d.plane_off[1], d.bw[1] * 8, cw, ch, d.hmax, d.vmax, y, x) - 128;
  const int cr = chroma_at(d.planes + d.plane_off[2], d.bw[2] * 8, cw, ch, d.hmax, d.vmax, y, x) - 128;
  // jdcolor.c: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554, ONE_HALF = 32768
  const int r = Y + ((91881 * cr + 32768) >> 16);
  const int g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
  const int bl = Y + ((116130 * cb + 32768) >> 16);
  o[0] = (unsigned char)(r < 0 ? 0 : (r > 255 ? 255 : r));
  o[1] = (unsigned char)(g < 0 ? 0 : (g > 255 ? 255 : g));
  o[2] = (unsigned char)(bl < 0 ? 0 : (bl > 255 ? 255 : bl));
}

}  // namespace

extern "C" int gpv_jpeg_decode(const gpv_jpeg_desc* descs, int B, int max_blocks, int64_t max_pixels, void* stream) {
  if (!descs || B <= 0 || max_blocks <= 0 || max_pixels <= 0) return (int)hipErrorInvalidValue;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(jpeg_idct_kernel, dim3((max_blocks + 31) / 32, B), dim3(256), 0, st, descs);
  GPV_CHECK_LAUNCH();
  hipLaunchKernelGGL(jpeg_color_kernel, dim3((unsigned)((max_pixels + 255) / 256), B), dim3(256), 0, st, descs);
  GPV_CHECK_LAUNCH();
  return 0;
}
