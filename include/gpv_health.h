/* C ABI of libgpv_health.so: per-segment tensor statistics, a device ring of them and a first-non-finite latch
 * (gpv-1_amd/csrc/tensor_stats.hip) -- the training flight recorder of gpv1_amd.health.
 *
 * A library of its own beside libgpv_hip.so, libgpv_eval.so, libgpv_cap.so and libgpv_match.so: those four export lists are pinned.
 * Every function takes plain device pointers, returns a hipError_t as int (0 = ok), launches on `stream`, never synchronises,
 * allocates nothing, reads nothing back and keeps no global state: all of it can be captured in a graph.  Nothing here ever writes
 * to a watched segment.  Anything outside the stated shapes returns hipErrorInvalidValue before a launch.
 *
 * THE RULE (stated once on the host: gpv1_amd.health.segment_stats_host; the kernels equal it bit for bit, sumsq included).
 * A segment is n >= 0 consecutive elements of fp32 or bf16; a bf16 element is widened exactly to fp32 (its 16 bits become the high
 * half) before anything is computed from its value.  Its statistics are one gpv_health_row:
 *   n_nan, n_inf, n_zero   counts; -0.0 counts as zero, a denormal does not
 *   first_bad              index, relative to the segment start, of the first NaN or +-inf; -1 if there is none
 *   first_kind             GPV_HEALTH_NAN / GPV_HEALTH_INF: what the element at first_bad is; 0 if there is none
 *   absmax                 largest |x| over the finite elements, 0 if there are none; exact
 *   sumsq                  float64 sum of x * x over the finite elements in the PINNED ORDER below
 *   bits_sum               wrap-around (mod 2^64) sum of the raw element bit patterns, each 32-bit or 16-bit pattern zero-extended:
 *                          independent of order, exact -- a fingerprint of the segment's bits
 * Pinned order of sumsq: the segment is cut from its start into blocks of GPV_HEALTH_BLOCK = 16384 elements; in a block, element j
 * belongs to lane (j >> 2) & 255; a lane adds its squares in ascending j in float64, starting from +0.0 (the square of an fp32 value
 * is exact in float64: fused and unfused multiply-add round alike, only the order matters); the 256 lane sums are folded by the tree
 * s[l] += s[l + stride] for stride = 128, 64, ..., 1; the block sums s[0] are added in ascending block order, starting from +0.0.
 * n == 0 gives an all-zero row with first_bad = -1. */
#ifndef GPV_HEALTH_H
#define GPV_HEALTH_H
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_HEALTH_BLOCK 16384   /* elements per block of the pinned order: one 256-thread workgroup, 16 groups of 4 elements per lane */
#define GPV_HEALTH_F32 0         /* gpv_health_seg.dtype */
#define GPV_HEALTH_BF16 1
#define GPV_HEALTH_NAN 1         /* gpv_health_row.first_kind, state[GPV_HEALTH_ST_KIND] */
#define GPV_HEALTH_INF 2

typedef struct {                 /* 64 bytes */
    long long n_nan, n_inf, n_zero, first_bad;
    double sumsq;
    unsigned long long bits_sum;
    float absmax;
    unsigned int first_kind;
    unsigned long long reserved; /* written as 0 */
} gpv_health_row;

typedef struct {                 /* 32 bytes; built once on the host */
    const void* ptr;             /* first element; element-aligned (aligned to 16 bytes fp32 / 8 bytes bf16: vector loads) */
    long long n;                 /* elements, >= 0 */
    int dtype;                   /* GPV_HEALTH_F32 / GPV_HEALTH_BF16 */
    int pad;
    long long ws_first;          /* index of the segment's first block in the work list = of its first partial row in the workspace */
} gpv_health_seg;

typedef struct { int seg, block; } gpv_health_work;

/* The rows of S segments in two launches.
 * work[W] lists every (segment, block) pair with block * GPV_HEALTH_BLOCK < n, segment after segment, blocks ascending: entry
 * segs[s].ws_first + b is (s, b); a segment of n == 0 has no entry.  ws[W] is a caller-lent workspace: one partial row per entry.
 * Pass 1, one 256-thread workgroup per entry: per-lane integer and float64 partials, the pinned tree in LDS, one partial row into
 * ws[entry] -- no atomics.  Pass 2, one wave per segment: folds ws[ws_first .. ws_first + blocks) in block order into rows[s].
 * Every load is inside [ptr, ptr + n): heads, tails and unaligned segments load single elements from clamped indices and mask at
 * use.  No loop bound depends on the data.  An entry whose (seg, block) is outside its segment is skipped; a segment whose
 * ws_first .. ws_first + blocks is not inside [0, W) gets a row of first_bad = -2 instead of a read outside ws.
 * Shapes: S >= 1, W >= 0. */
int gpv_health_stats(const gpv_health_seg* segs /*[S]*/, int S, const gpv_health_work* work /*[W]*/, int W, gpv_health_row* ws /*[W]*/,
                     gpv_health_row* rows /*[S]*/, void* stream);

/* indices into state[GPV_HEALTH_STATE_WORDS] (long long, device resident, zeroed once by the caller) */
#define GPV_HEALTH_ST_CURSOR 0     /* commits so far; the next commit writes slot cursor % R */
#define GPV_HEALTH_ST_LATCHED 1    /* 0: the latch is empty; 1: words 2..5 hold the first trip */
#define GPV_HEALTH_ST_TRIP_CURSOR 2
#define GPV_HEALTH_ST_TRIP_SEG 3   /* lowest segment index with n_nan + n_inf > 0 in that commit */
#define GPV_HEALTH_ST_TRIP_INDEX 4 /* its first_bad */
#define GPV_HEALTH_ST_KIND 5       /* its first_kind */
#define GPV_HEALTH_ST_TRIPS 6      /* commits that held a non-finite value, the latched one included */
#define GPV_HEALTH_STATE_WORDS 8

/* One launch (one workgroup): copies rows[S] into slot c % R of ring[R][S] where c = state[CURSOR], sets stamps[c % R] = c, sets
 * state[CURSOR] = c + 1, and maintains the latch: if some row has n_nan + n_inf > 0, TRIPS += 1, and if the latch is empty it
 * records (c, lowest such segment index, its first_bad, its first_kind).  The first trip wins.  The cursor lives on the device so
 * that a captured graph advances it on every replay.  stamps[R] is filled with -1 by the caller before the first commit.
 * Shapes: S >= 1, R >= 1. */
int gpv_health_commit(const gpv_health_row* rows /*[S]*/, int S, int R, long long* state /*[GPV_HEALTH_STATE_WORDS]*/,
                      long long* stamps /*[R]*/, gpv_health_row* ring /*[R,S]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
