/* C ABI of libgpv_huff.so: the Huffman stream of a baseline JPEG file decoded on the device (gpv-1_amd/csrc/jpeg_huff.hip), bit for
 * bit what gpv_jpeg_parse (gpv_hip.h) writes.  The host statement of the same rule is gpv1_amd.jpeg_entropy.
 *
 * A library of its own beside libgpv_hip.so, libgpv_eval.so, libgpv_cap.so, libgpv_match.so, libgpv_health.so and libgpv_beam.so:
 * those six export lists are pinned.  gpv_huff_prepare is HOST code (thread-safe, no HIP call); the other two follow the rules of the
 * device libraries: plain device pointers, a hipError_t as int (0 = ok), launches on `stream`, never synchronise, allocate nothing,
 * keep no global state.  Anything outside the stated extents returns hipErrorInvalidValue before a launch.
 *
 * THE RULE.  Scope: baseline, one interleaved scan, no restart interval, the scan ended by EOI.
 *  - The stream is the entropy segment with the FF 00 stuffing removed, nbits = 8 * its bytes, cut into n_sub = ceil(nbits / S)
 *    subsequences of S bits; S is a multiple of 32, 64 <= S <= 4096.
 *  - A state is (bit position p, block index c inside the MCU, zigzag index z); z = 0: the next symbol is a DC symbol.  A symbol is a
 *    Huffman code and its extra bits (at most 16 + 15 bits).  A walk decodes symbols while p < limit; its end state is therefore the
 *    first symbol boundary at or after limit.  e_i is the end state of subsequence i, limit = min((i+1)*S, nbits).
 *  - Pass 0: every subsequence starts at bit i*S in state (c = 0, z = 0).  Subsequence 0 is therefore exact.
 *  - Pass k: a subsequence whose predecessor's state changed in pass k-1 is decoded again from e_{i-1} as pass k-1 left it (every
 *    state counts as changed in pass 0).  The iteration ends with the first pass after which no subsequence that has a successor
 *    changed: at most n_sub passes, pass 0 included.  The fixed point is the sequential decode, by induction from e_0.
 *  - Decoding from a wrong start is memory-safe and deterministic: a code that no table entry matches consumes 16 bits and decodes
 *    symbol 0; a DC category above 15 is 15; an AC run that takes z past 63 consumes its extra bits, stores nothing and ends the
 *    block; every index is clamped; reads past the padded stream give zero bits.  None of these conventions can show in the
 *    result: an error counts only if it is still there at the fixed point, in a block of the frame.
 *  - After convergence the blocks finished per subsequence are counted, an exclusive prefix gives each subsequence its first block
 *    in scan order, and a write pass decodes each subsequence once more from e_{i-1} and stores the AC values in natural order and
 *    the DC differences.  A per-component running sum in scan order turns the differences into DC values (32-bit sum, stored as
 *    int16, as gpv_jpeg_parse's cast does).  Blocks at or beyond the frame's block count are not written. */
#ifndef GPV_HUFF_H
#define GPV_HUFF_H
#include <stdint.h>
#include "gpv_hip.h"              /* gpv_jpeg_info */
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_HUFF_LOOK 9             /* bits of the look-up, as in jpeg.hip */
#define GPV_HUFF_ROUTE_DEVICE 0
#define GPV_HUFF_ROUTE_HOST 1       /* restart interval, or the scan is not ended by EOI: the file keeps gpv_jpeg_parse */
#define GPV_HUFF_MIN_S 64
#define GPV_HUFF_MAX_S 4096
#define GPV_HUFF_LANES 1024         /* threads of the workgroup that serves one image */
#define GPV_HUFF_MAX_STREAM (1 << 27)  /* stream bytes of a device-routed file: bit positions stay below 2^30 */
#define GPV_HUFF_WS_PER_SUB 48      /* workspace bytes per subsequence */
#define GPV_HUFF_ERR_CODE 1         /* status bits: a bad code / category / index in a block of the frame at the fixed point */
#define GPV_HUFF_ERR_SHORT 2        /*              the stream ends before the frame's last block */
#define GPV_HUFF_ERR_EXTENT 4       /*              nbits above the max_nbits of the call: nothing was decoded */

typedef struct gpv_huff_table {
  unsigned char look_nbits[1 << GPV_HUFF_LOOK];   /* code length of the code that starts these 9 bits, 0: longer than 9 */
  unsigned char look_sym[1 << GPV_HUFF_LOOK];
  int maxcode[18];                  /* largest code of length l, -1 if none; [17] = sentinel */
  int valoffset[17];                /* symbol index of the first code of length l, minus that code */
  unsigned char syms[256];
  int reserved;
} gpv_huff_table;

typedef struct gpv_huff_desc {
  const unsigned char* stream;      /* DEVICE, 16-byte aligned, stream_cap bytes: the un-stuffed stream, zero-padded (the caller sets it) */
  short* coefs;                     /* DEVICE, coef_count int16, 16-byte aligned: out, the layout of gpv_jpeg_parse (the caller sets it) */
  int* status;                      /* DEVICE, 2 ints: out, GPV_HUFF_ERR_* bits and the number of passes (the caller sets it) */
  int64_t coef_offset[3];           /* as gpv_jpeg_info */
  int64_t coef_count;
  int nbits;                        /* 8 * stream bytes */
  int stream_cap;                   /* padded bytes: a multiple of 16, at least stream bytes + 16 */
  int ncomp, mcus_x, mcus_y;
  int blocks_per_mcu;               /* 1, 3, 4 or 6 */
  int nblocks;                      /* mcus_x * mcus_y * blocks_per_mcu */
  int bh[3], bw[3];                 /* as gpv_jpeg_info */
  int comp_h[3], comp_v[3];         /* sampling factors */
  unsigned char blk_comp[8], blk_v[8], blk_h[8];   /* per block of an MCU: its component and its place inside the MCU */
  gpv_huff_table dc[3], ac[3];      /* per component */
} gpv_huff_desc;

/* HOST.  The byte-level pass of one file: markers, tables, un-stuffing.  Fills `info` exactly as gpv_jpeg_parse does, fills `desc`
 * (all but its three pointers), sets *stream_cap to the padded stream size and *route to GPV_HUFF_ROUTE_*.  out == NULL: sizes only.
 * Otherwise out (out_capacity >= *stream_cap bytes, lent by the caller) receives the un-stuffed stream and zeros up to stream_cap.
 * Returns 0, hipErrorInvalidValue (1: malformed, or out too small) or hipErrorNotSupported (801: what gpv_jpeg_parse refuses). */
int gpv_huff_prepare(const unsigned char* data, int64_t nbytes, gpv_jpeg_info* info, gpv_huff_desc* desc, unsigned char* out,
                     int64_t out_capacity, int64_t* stream_cap, int* route);

/* *bytes = the workspace a gpv_huff_decode call over B images with at most max_nbits stream bits each needs */
int gpv_huff_workspace_bytes(int B, int subseq_bits, int64_t max_nbits, int64_t* bytes);

/* DEVICE, one launch: descs = DEVICE array of B descriptors.  One workgroup of GPV_HUFF_LANES threads serves one image: it zeroes
 * the coefficients, its threads walk the subsequences in strides (states in `workspace`, tables in LDS), a workgroup-wide flag and a
 * barrier decide each pass; prefix, write pass and the DC sums follow in the same launch.  Every loop bound is an argument or a
 * constant: passes <= n_sub, symbols per walk <= S, scans over n_sub and the block count.  Every table and stream index is clamped. */
int gpv_huff_decode(const gpv_huff_desc* descs, int B, int subseq_bits, int64_t max_nbits, void* workspace, int64_t workspace_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif
