// Shared between the GEMM / convolution sources: the kernel argument and the routing decision (gemm_route.h, host-only), the device
// helpers they share, and the launch functions gpv_gemm / gpv_conv2d (gemm.hip) dispatch a Route to.
#pragma once
#include "common.h"
#include "../../include/gpv_hip.h"
#include "gemm_route.h"

namespace gpvk {

// GEMM row -> output pixel (row of the NHWC output) ; identity unless the rows are parity-class-major
__device__ __forceinline__ int conv_row_to_pixel(int m, const ConvGeom& g) {
  if (!g.cm) return m;
  const int cls = m / g.cls_rows, rem = m - cls * g.cls_rows;
  const int hw2 = (g.OH >> 1) * (g.OW >> 1), w2 = g.OW >> 1;
  const int b = rem / hw2, r2 = rem - b * hw2;
  const int y2 = r2 / w2, x2 = r2 - y2 * w2;
  return (b * g.OH + 2 * y2 + (cls >> 1)) * g.OW + 2 * x2 + (cls & 1);
}


// Register epilogue of the direct-to-LDS kernels (gemm_glds.hip, gemm_pipe.hip): the B rows (= output columns) are staged PERMUTED, LDS row r
// holds output column depi_col_perm(r) -- common.h acc_chan's map, for any number of 32-column groups -- so that the accumulator tiles
// 2 t, 2 t + 1 leave lane (row, g) with the 8 consecutive columns 32 t + 8 g .. + 7 of its row
__device__ __forceinline__ int depi_col_perm(int r) { return (r & ~31) + ((r & 15) >> 2) * 8 + ((r >> 4) & 1) * 4 + (r & 3); }

// <family>_launch: the template switch over the Route's instance, the attribute once-flags, the launch counter and the launch -- no
// decision (those are gemm_route.h's <family>_select).  Returns 0 or a hipError_t.
int gemv_launch(const GemmK& k, const Route& r, hipStream_t st);          // gemv.hip
int c1s_launch(const GemmK& k, const Route& r, hipStream_t st);           // conv1x1_stream.hip
int c3s_launch(const GemmK& k, const Route& r, hipStream_t st);           // conv3x3_stream.hip
int pipe_launch(const GemmK& k, const Route& r, hipStream_t st);          // gemm_pipe.hip
int skinny_launch(const GemmK& k, const Route& r, hipStream_t st);        // gemm_skinny.hip
int skinny_tt_launch(const GemmK& k, const Route& r, hipStream_t st);
int glds_launch(const GemmK& k, const Route& r, hipStream_t st);          // gemm_glds.hip (FAM_GLDS and FAM_HALO)
int glds_tt_launch(const GemmK& k, const Route& r, hipStream_t st);       // gemm_glds_tt.hip (FAM_GLDS_WGRAD and FAM_GLDS_TT)

// gemm.hip: second pass of a workspace split reduction, C[m,n] += sum_s ws[s][m][n]
int launch_splitk_reduce(const float* ws, int split, int M, int N, float* C, int64_t ldc, hipStream_t st);

}  // namespace gpvk
