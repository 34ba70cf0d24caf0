// Per-segment tensor statistics, a device ring of them and a first-non-finite latch (include/gpv_health.h; the host statement of
// the same rule is gpv1_amd.health.segment_stats_host / ring_commit_host).  Three small launches, no atomics of any kind, no float
// crosses a workgroup except as a finished block sum:
//   block_kernel   one 256-thread workgroup per (segment, block of 16384 elements).  Lane t owns the groups of four elements
//                  j = 1024 i + 4 t + c (i < 16, c < 4) -- the header's lane (j >> 2) & 255 -- and walks them in ascending j: counts,
//                  first non-finite element (a key: index * 2 + is-inf, so that a minimum carries the kind along), largest finite |x|
//                  as its bit pattern (monotone for non-negative floats), the wrap-around sum of the raw bits and the float64 sum of
//                  squares.  The 256 lane partials are folded by the pinned tree in LDS, thread 0 stores one partial row.
//                  Aligned segments (16 bytes fp32, 8 bytes bf16) load a whole group at once; the last, incomplete group of a tail
//                  block and every element of an unaligned segment are loaded singly.  Every load address is clamped into the block
//                  and the value masked at use: nothing outside [ptr, ptr + n) is read, no load sits
//                  behind a predicate, no loop bound depends on the data.
//   fold_kernel    one wave per segment: the partial rows of its blocks, 64 at a time; the integer fields by butterflies, the block
//                  sums of squares one after the other in block order (every lane adds the same numbers: no broadcast at the end).
//   commit_kernel  one workgroup: rows -> ring slot cursor % R, stamp, cursor + 1, latch.
// -ffp-contract=off like the other scorer libraries: the square of an fp32 value is exact in float64, so a fused multiply-add would
// round the same -- the flag keeps that from being an argument.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <type_traits>
#include "../../include/gpv_health.h"

#pragma clang fp contract(off)

namespace {

constexpr int BLOCK = GPV_HEALTH_BLOCK;
constexpr int LANES = 256;
constexpr unsigned NO_KEY = 0xffffffffu;
static_assert(BLOCK == LANES * 64, "16 groups of four elements per lane");
static_assert(sizeof(gpv_health_row) == 64 && sizeof(gpv_health_seg) == 32 && sizeof(gpv_health_work) == 8, "ABI of include/gpv_health.h");

struct Acc {
    double s = 0.0;
    unsigned long long bits = 0;
    unsigned nan = 0, inf = 0, zero = 0, first = NO_KEY, amax = 0;
};

// one element: raw = its bit pattern zero-extended, j = its index in the block, ok = it exists
template <bool BF>
__device__ __forceinline__ void take(Acc& a, unsigned raw, bool ok, unsigned j) {
    const unsigned f = BF ? raw << 16 : raw;                 // bf16 -> fp32 is exact: the 16 bits are the high half
    const unsigned u = f & 0x7fffffffu;
    const bool isnan = u > 0x7f800000u, isinf = u == 0x7f800000u, fin = u < 0x7f800000u;
    a.bits += ok ? raw : 0u;
    a.nan += (ok && isnan) ? 1u : 0u;
    a.inf += (ok && isinf) ? 1u : 0u;
    a.zero += (ok && u == 0u) ? 1u : 0u;
    const unsigned key = (j << 1) | (isinf ? 1u : 0u);
    a.first = (ok && !fin && key < a.first) ? key : a.first;
    a.amax = (ok && fin && u > a.amax) ? u : a.amax;
    const double d = (double)__uint_as_float(f);
    const double sq = d * d;
    a.s = (ok && fin) ? a.s + sq : a.s;
}

template <bool BF>
__device__ __forceinline__ void block_stats(const void* base, unsigned cnt, bool aligned, Acc& a, unsigned t) {
    using E = typename std::conditional<BF, uint16_t, uint32_t>::type;
    using V = typename std::conditional<BF, uint2, uint4>::type;
    const E* p = static_cast<const E*>(base);
    const unsigned last = cnt - 1;                           // cnt >= 1: a block in the work list holds at least one element
    if (aligned) {
        const unsigned full = cnt >> 2;                      // complete groups of four in this block
        if (full > 0) {
            const V* pv = static_cast<const V*>(base);
#pragma unroll 8
            for (unsigned i = 0; i < 16; ++i) {
                const unsigned g = i * LANES + t;
                const bool ok = g < full;
                const V v = pv[ok ? g : full - 1];
                unsigned r[4];
                if (BF) {
                    const uint2 w = *reinterpret_cast<const uint2*>(&v);
                    r[0] = w.x & 0xffffu; r[1] = w.x >> 16; r[2] = w.y & 0xffffu; r[3] = w.y >> 16;
                } else {
                    const uint4 w = *reinterpret_cast<const uint4*>(&v);
                    r[0] = w.x; r[1] = w.y; r[2] = w.z; r[3] = w.w;
                }
#pragma unroll
                for (unsigned c = 0; c < 4; ++c) take<BF>(a, r[c], ok, 4 * g + c);
            }
        }
        // the incomplete group behind them (cnt & 3 elements): group `full`, which is the last one of its lane
        const unsigned rem = cnt & 3u;
        const bool mine = t == (full & (LANES - 1));
#pragma unroll
        for (unsigned c = 0; c < 3; ++c) {
            const unsigned j = 4 * full + c;
            const unsigned raw = p[j < last ? j : last];
            take<BF>(a, raw, mine && c < rem, j);
        }
    } else {
#pragma unroll 4
        for (unsigned i = 0; i < 16; ++i) {
#pragma unroll
            for (unsigned c = 0; c < 4; ++c) {
                const unsigned j = i * (4 * LANES) + 4 * t + c;
                const unsigned raw = p[j < last ? j : last];
                take<BF>(a, raw, j < cnt, j);
            }
        }
    }
}

__global__ __launch_bounds__(LANES) void block_kernel(const gpv_health_seg* __restrict__ segs, int S, const gpv_health_work* __restrict__ work,
                                                      gpv_health_row* __restrict__ ws) {
    __shared__ double s_sum[LANES];
    __shared__ unsigned long long s_bits[LANES];
    __shared__ unsigned s_nan[LANES], s_inf[LANES], s_zero[LANES], s_first[LANES], s_amax[LANES];
    const unsigned t = threadIdx.x;
    const gpv_health_work wk = work[blockIdx.x];
    if (wk.seg < 0 || wk.seg >= S || wk.block < 0) return;                 // (uniform: a malformed work list is skipped, not followed)
    const gpv_health_seg sg = segs[wk.seg];
    const long long start = (long long)wk.block * BLOCK;
    if (start >= sg.n) return;
    const long long left = sg.n - start;
    const unsigned cnt = left < BLOCK ? (unsigned)left : (unsigned)BLOCK;
    const bool bf = sg.dtype == GPV_HEALTH_BF16;
    const char* base = static_cast<const char*>(sg.ptr) + start * (bf ? 2 : 4);
    const bool aligned = (reinterpret_cast<uintptr_t>(base) & (bf ? 7u : 15u)) == 0;
    Acc a;
    if (bf) block_stats<true>(base, cnt, aligned, a, t);
    else block_stats<false>(base, cnt, aligned, a, t);
    s_sum[t] = a.s; s_bits[t] = a.bits; s_nan[t] = a.nan; s_inf[t] = a.inf; s_zero[t] = a.zero; s_first[t] = a.first; s_amax[t] = a.amax;
    for (unsigned stride = LANES / 2; stride >= 1; stride >>= 1) {        // the pinned tree: s[l] += s[l + stride]
        __syncthreads();
        if (t < stride) {
            s_sum[t] += s_sum[t + stride];
            s_bits[t] += s_bits[t + stride];
            s_nan[t] += s_nan[t + stride];
            s_inf[t] += s_inf[t + stride];
            s_zero[t] += s_zero[t + stride];
            s_first[t] = s_first[t + stride] < s_first[t] ? s_first[t + stride] : s_first[t];
            s_amax[t] = s_amax[t + stride] > s_amax[t] ? s_amax[t + stride] : s_amax[t];
        }
    }
    if (t == 0) {
        gpv_health_row r;
        r.n_nan = s_nan[0]; r.n_inf = s_inf[0]; r.n_zero = s_zero[0];
        const unsigned key = s_first[0];
        r.first_bad = key == NO_KEY ? -1 : start + (long long)(key >> 1);
        r.first_kind = key == NO_KEY ? 0u : ((key & 1u) ? (unsigned)GPV_HEALTH_INF : (unsigned)GPV_HEALTH_NAN);
        r.sumsq = s_sum[0];
        r.bits_sum = s_bits[0];
        r.absmax = __uint_as_float(s_amax[0]);
        r.reserved = 0;
        ws[blockIdx.x] = r;
    }
}

constexpr long long NO_FIRST = 0x7fffffffffffffffLL;

__global__ __launch_bounds__(64) void fold_kernel(const gpv_health_seg* __restrict__ segs, long long W, const gpv_health_row* __restrict__ ws,
                                                  gpv_health_row* __restrict__ rows) {
    const unsigned lane = threadIdx.x;
    const gpv_health_seg sg = segs[blockIdx.x];
    const long long nb = sg.n > 0 ? (sg.n + BLOCK - 1) / BLOCK : 0;
    const bool inside = sg.n >= 0 && sg.ws_first >= 0 && sg.ws_first <= W && nb <= W - sg.ws_first;
    long long nan = 0, inf = 0, zero = 0, first = NO_FIRST;               // first: first_bad * 4 + first_kind
    unsigned long long bits = 0;
    unsigned amax = 0;
    double total = 0.0;
    if (inside) {
        for (long long b0 = 0; b0 < nb; b0 += 64) {
            const long long b = b0 + lane;
            const bool ok = b < nb;
            const gpv_health_row r = ws[sg.ws_first + (ok ? b : nb - 1)];
            nan += ok ? r.n_nan : 0;
            inf += ok ? r.n_inf : 0;
            zero += ok ? r.n_zero : 0;
            bits += ok ? r.bits_sum : 0ull;
            const long long key = r.first_bad < 0 ? NO_FIRST : r.first_bad * 4 + (long long)r.first_kind;
            first = (ok && key < first) ? key : first;
            const unsigned am = __float_as_uint(r.absmax);
            amax = (ok && am > amax) ? am : amax;
            const long long here = nb - b0 < 64 ? nb - b0 : 64;
            for (int k = 0; k < 64; ++k) {                                // block sums in ascending block order, the same in every lane
                const double v = __shfl(r.sumsq, k);
                total = k < here ? total + v : total;
            }
        }
    }
    for (int m = 32; m >= 1; m >>= 1) {
        nan += __shfl_xor(nan, m);
        inf += __shfl_xor(inf, m);
        zero += __shfl_xor(zero, m);
        bits += __shfl_xor(bits, m);
        const long long of = __shfl_xor(first, m);
        first = of < first ? of : first;
        const unsigned oa = __shfl_xor(amax, m);
        amax = oa > amax ? oa : amax;
    }
    if (lane == 0) {
        gpv_health_row r;
        r.n_nan = nan; r.n_inf = inf; r.n_zero = zero;
        r.first_bad = !inside ? -2 : (first == NO_FIRST ? -1 : first >> 2);
        r.first_kind = (!inside || first == NO_FIRST) ? 0u : (unsigned)(first & 3);
        r.sumsq = total;
        r.bits_sum = bits;
        r.absmax = __uint_as_float(amax);
        r.reserved = 0;
        rows[blockIdx.x] = r;
    }
}

__global__ __launch_bounds__(LANES) void commit_kernel(const gpv_health_row* __restrict__ rows, int S, int R, long long* __restrict__ state,
                                                       long long* __restrict__ stamps, gpv_health_row* __restrict__ ring) {
    __shared__ int s_low[LANES];
    const int t = threadIdx.x;
    const long long c = state[GPV_HEALTH_ST_CURSOR];        // read by every thread before the barriers below, written behind them
    const long long slot = (long long)((unsigned long long)c % (unsigned long long)R);
    const uint4* src = reinterpret_cast<const uint4*>(rows);
    uint4* dst = reinterpret_cast<uint4*>(ring + slot * S);
    for (int i = t; i < S * 4; i += LANES) dst[i] = src[i];
    int low = 0x7fffffff;                                                  // lowest segment index that holds a non-finite value
    for (int s = t; s < S; s += LANES) {
        const bool bad = rows[s].n_nan + rows[s].n_inf > 0;
        low = (bad && s < low) ? s : low;
    }
    s_low[t] = low;
    for (int stride = LANES / 2; stride >= 1; stride >>= 1) {
        __syncthreads();
        if (t < stride) s_low[t] = s_low[t + stride] < s_low[t] ? s_low[t + stride] : s_low[t];
    }
    if (t == 0) {
        stamps[slot] = c;
        state[GPV_HEALTH_ST_CURSOR] = c + 1;
        const int s = s_low[0];
        if (s != 0x7fffffff) {
            state[GPV_HEALTH_ST_TRIPS] += 1;
            if (state[GPV_HEALTH_ST_LATCHED] == 0) {                       // the first trip wins
                state[GPV_HEALTH_ST_LATCHED] = 1;
                state[GPV_HEALTH_ST_TRIP_CURSOR] = c;
                state[GPV_HEALTH_ST_TRIP_SEG] = s;
                state[GPV_HEALTH_ST_TRIP_INDEX] = rows[s].first_bad;
                state[GPV_HEALTH_ST_KIND] = rows[s].first_kind;
            }
        }
    }
}

}  // namespace

extern "C" int gpv_health_stats(const gpv_health_seg* segs, int S, const gpv_health_work* work, int W, gpv_health_row* ws,
                                gpv_health_row* rows, void* stream) {
    if (S < 1 || W < 0 || !segs || !rows || (W > 0 && (!work || !ws))) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(segs) | reinterpret_cast<uintptr_t>(work)) & 7) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(ws) | reinterpret_cast<uintptr_t>(rows)) & 15) return (int)hipErrorInvalidValue;      // 16-byte row stores
    if (W > 0) {
        hipLaunchKernelGGL(block_kernel, dim3(W), dim3(LANES), 0, (hipStream_t)stream, segs, S, work, ws);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(fold_kernel, dim3(S), dim3(64), 0, (hipStream_t)stream, segs, (long long)W, ws, rows);
    return (int)hipGetLastError();
}

extern "C" int gpv_health_commit(const gpv_health_row* rows, int S, int R, long long* state, long long* stamps, gpv_health_row* ring,
                                 void* stream) {
    if (S < 1 || R < 1 || !rows || !state || !stamps || !ring) return (int)hipErrorInvalidValue;
    if ((reinterpret_cast<uintptr_t>(rows) | reinterpret_cast<uintptr_t>(ring)) & 15) return (int)hipErrorInvalidValue;    // uint4 copies
    if ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(stamps)) & 7) return (int)hipErrorInvalidValue;
    if ((long long)S * 4 > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(commit_kernel, dim3(1), dim3(LANES), 0, (hipStream_t)stream, rows, S, R, state, stamps, ring);
    return (int)hipGetLastError();
}
