// Helpers shared by the device sources (through common.h) and the host-only headers that plain g++ compiles (gemm_route.h): no HIP call,
// no device type.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#ifdef __HIPCC__
#define GPV_HD __host__ __device__ __forceinline__
#else
#define GPV_HD inline
#endif

// Environment knobs of the kernels' launch heuristics (kernel family on / off, blocks per CU, rows per strip, forced tiles, split targets,
// timing ablations) exist for tools/ only: they are read iff the library was compiled with -DGPV_TUNING (`make tuning` ->
// libgpv_hip_tuning.so, loaded by gpv1_amd.hip when GPV_TUNING_LIB=1).  The production library (libgpv_hip.so) reads NO environment:
// every knob is its default, and the run-time switches tests need go through gpv_set_option ("no global state").
#ifdef GPV_TUNING
static inline int tune_env(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
#else
static inline int tune_env(const char*, int dflt) { return dflt; }
#endif

// 16-byte alignment of an operand base: the precondition of every 16-byte vector access and of the LDS-DMA loaders
GPV_HD bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

GPV_HD uint32_t drop_thresh(float p) {
  double t = (double)p * 4294967296.0;
  if (t < 0) t = 0;
  if (t > 4294967295.0) t = 4294967295.0;
  return (uint32_t)t;
}
