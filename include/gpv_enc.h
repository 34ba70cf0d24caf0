/* C ABI of libgpv_enc.so: a batch of pictures encoded as baseline JPEG files on the device (gpv-1_amd/csrc/jpeg_enc.hip), byte for
 * byte what the host rule writes (gpv1_amd.jpeg_encode.encode_host in numpy, gpv-1_amd/csrc/jpeg_enc_host.h in plain C++), which in
 * turn is the file Pillow writes for the same pixels.  DESIGN.md section 6h states the rule.
 *
 * A library of its own, listed in gpv1_amd._native.LIBRARIES and built by the Makefile's `all` like the others.  gpv_enc_header is HOST code (no HIP call); the other two follow the rules
 * of the device libraries: a hipError_t as int (0 = ok), launches on `stream`, never synchronise, allocate nothing, keep no global
 * state.  Anything outside the stated extents returns hipErrorInvalidValue (1) before a launch.
 *
 * One gpv_enc_encode call serves B pictures of any sizes with four launches, whatever B is:
 *   1. coefficients: one thread per block of the scan (dummy blocks included) reads its pixels (clamped indices: the edges repeat),
 *      overlays the box outlines and then the boxes' labels, converts, down-samples, transforms, quantises, writes the block's 64
 *      int16 in zigzag order and the bit count of its AC code;
 *   2. offsets: one workgroup per picture adds each block's DC code (the difference to the component's previous DC; a dummy block
 *      repeats the DC coded before it), scans the bit counts (wave64 scans), and zeroes the words the picture's bits will occupy;
 *   3. packing: one thread per block writes its bits at its offset, most significant bit first; the two words a block may share with
 *      its neighbours get a 32-bit atomicOr (OR does not depend on order: the bytes are deterministic), the others a plain store;
 *   4. bytes: one workgroup per picture writes the header, counts 0xFF per 16-byte chunk, scans, writes every byte of the scan with
 *      its 0x00 stuffing behind the header, then EOI, the picture's byte count and its status word.
 * Integer arithmetic only after the pixel is a uint8; -ffp-contract=off for the two fp32 rules in front of that (denormalise, box
 * corners), which round every operation on its own.
 *
 * Labels (gpv_enc_desc.labels > 0; the rule in numpy: gpv1_amd.jpeg_encode.label_plates / draw_labels_host, in C++: label_place /
 * draw_labels of jpeg_enc_host.h).  A label is a text of n <= GPV_ENC_MAX_LABEL characters in a fixed 6 x 11 cell (Pillow's
 * built-in bitmap font, bytes 32..126; any other byte is drawn as '?'), inked in the box's colour on a plate of colour (10, 10, 10)
 * that is w = 6 n + 2 wide and 13 high: a one-pixel margin all round.
 *   Storage: colours[4 i + 3] = L_i; L_i & 0x7F = the character count of box i (0 = no label), bit 7 = below the box instead of
 *   above.  The texts stand one behind the other at colours + 4 nboxes, box i's at offset sum_{j<i} (L_j & 0x7F); `labels` = their
 *   bytes in all.  The length bytes are device memory, so they are not checked but clamped: the offset to `labels`, the count to
 *   GPV_ENC_MAX_LABEL and to the bytes that remain behind the offset.  Nothing outside colours[0 .. 4 nboxes + labels) is read.
 *   Placement, from the box's (x1, y1, x2, y2), integers only: above: py = y1 - 13, and if py < 0 then py = y1 + 1; below:
 *   py = y2 + 1, and if py + 13 > H then py = y2 - 13; then py = clamp(py, 0, max(0, H - 13)).  px = x1; if px + w > W then
 *   px = W - w; if px < 0 then px = 0.  The plate is px <= x < px + w, py <= y < py + 13, clipped to the picture.
 *   Ink: with c = x - px - 1 and r = y - py - 1, a pixel of the plate is ink if 0 <= c < 6 n, 0 <= r < 11 and bit c % 6 of row r of
 *   the glyph of text byte c / 6 is set (bit 0 = the glyph's left column); every other pixel of the plate has the plate's colour.
 *   One exception, because Pillow's font is not quite a fixed cell: 29 glyphs (k, T, ...) are pasted one pixel to the left, over the
 *   last column of the character before them.  Where c % 6 = 5, character c / 6 + 1 exists and row r of ITS glyph has bit 7, the
 *   pixel is ink if that row has bit 6.  The first character's overhang is not drawn (Pillow clips it).
 *   Order: all outlines in box order, then all labels in box order; a later one overwrites an earlier one, so no outline cuts a label.
 * labels = 0 is the call as it was before labels existed, whatever the fourth colour bytes hold. */
#ifndef GPV_ENC_H
#define GPV_ENC_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define GPV_ENC_SRC_U8 0            /* src = [H][pitch][3] uint8: a window of a picture */
#define GPV_ENC_SRC_BF16 1          /* src = pixel (0, 0) of one picture of the stem's padded NHWC4 batch, bf16; pitch = Wp */
#define GPV_ENC_SRC_F32 2           /* the same, fp32 */
#define GPV_ENC_444 0               /* subsampling, numbered as Pillow numbers it */
#define GPV_ENC_422 1
#define GPV_ENC_420 2
#define GPV_ENC_MAX_BOXES 32
#define GPV_ENC_MAX_LABEL 32        /* characters of one box's label */
#define GPV_ENC_MAX_BLOCKS (1 << 20)   /* blocks of one picture (dummy blocks included): bit offsets stay below 2^31 */
#define GPV_ENC_MAX_TOTAL_BLOCKS (1 << 24)   /* of one call */
#define GPV_ENC_HEADER_BYTES 623
#define GPV_ENC_BLOCK_BYTES 208     /* a block codes to at most 20 + 63 * 26 = 1658 bits */
#define GPV_ENC_STATUS_CAPACITY 1   /* status bit: the file is longer than `capacity`; only its first `capacity` bytes were written */

typedef struct gpv_enc_desc {
  const void* src;                  /* DEVICE, see GPV_ENC_SRC_*; 8-byte aligned for bf16, 16-byte aligned for fp32 */
  const float* boxes;               /* DEVICE, nboxes x (cx, cy, w, h), normalised; may be NULL if nboxes = 0 */
  const unsigned char* colours;     /* DEVICE, nboxes x 4 bytes (R, G, B, L); later boxes overwrite earlier ones.  L is ignored when
                                       labels = 0; else it is the box's length byte and `labels` text bytes follow the colours */
  int H, W;                         /* 1..65535 */
  int pitch;                        /* source row length in pixels, >= W */
  int kind;                         /* GPV_ENC_SRC_* */
  int nboxes;                       /* 0..GPV_ENC_MAX_BOXES */
  float mean[3], std[3];            /* GPV_ENC_SRC_BF16 / _F32: uint8 = clamp(floor(255 * (mean + std * x) + 0.5)), each operation rounded */
  int block_base, nblocks;          /* OUT: written by gpv_enc_encode (the picture's first block in the call, its block count) */
  int labels;                       /* 0: no labels; else the text bytes behind the nboxes x 4 colour bytes, 1..nboxes * GPV_ENC_MAX_LABEL */
} gpv_enc_desc;

/* *bytes = the workspace of a call over B pictures with `blocks` blocks in all, dummy blocks included (a picture has
 * ceil(ceil(W / hs) / 8) * ceil(ceil(H / vs) / 8) * (hs * vs + 2) of them):
 *   B * 80 (descriptors) + B * 16 (bit and byte counts) + B * 32 (slack of the packed bits)
 *   + blocks * (128 coefficients + 4 bit offset + 4 DC difference + GPV_ENC_BLOCK_BYTES packed bits) + 32 (rounding of the arrays)
 *   = 128 B + 344 blocks + 32.
 * The packed bits are not stuffed yet; the doubling for stuffing is in the file's bound, which is what `capacity` needs to hold any
 * picture: GPV_ENC_HEADER_BYTES + 2 * GPV_ENC_BLOCK_BYTES * nblocks + 2. */
int gpv_enc_workspace_bytes(int B, int64_t blocks, int64_t* bytes);

/* DEVICE, four launches.  descs = HOST array of B descriptors: checked here, completed (block_base, nblocks) and copied to the head
 * of the workspace on `stream`; it must stay alive and unchanged until the stream has passed this call.  quality 1..100,
 * subsampling GPV_ENC_4xx.  workspace: DEVICE, 16-byte aligned, workspace_bytes >= gpv_enc_workspace_bytes.  out: DEVICE,
 * B * capacity bytes; picture i's file starts at out + i * capacity.  sizes, status: DEVICE, B ints each: the file's length (the
 * full length even where it exceeds capacity) and GPV_ENC_STATUS_* bits.  Refused like every other bad extent: labels < 0,
 * labels > nboxes * GPV_ENC_MAX_LABEL (so any labels without boxes).  Labels read caller memory only: the workspace is the same. */
int gpv_enc_encode(gpv_enc_desc* descs, int B, int quality, int subsampling, void* workspace, int64_t workspace_bytes,
                   unsigned char* out, int64_t capacity, int* sizes, int* status, void* stream);

/* HOST.  The GPV_ENC_HEADER_BYTES bytes in front of the scan (SOI, APP0, two DQT, SOF0, four DHT, SOS) into buf; *nbytes = their
 * number. */
int gpv_enc_header(int H, int W, int quality, int subsampling, unsigned char* buf, int* nbytes);

#ifdef __cplusplus
}
#endif
#endif
