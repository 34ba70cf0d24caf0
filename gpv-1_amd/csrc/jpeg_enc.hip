// libgpv_enc.so (include/gpv_enc.h): a batch of pictures encoded as baseline JPEG files on the device.  The arithmetic of the rule
// (colour, sampling, transform, quantiser, entropy code of a block, box corners, labels, denormalise) is jpeg_enc_host.h, compiled here for
// the device as it stands; this file adds the four kernels around it and the entry points.  Built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <stdint.h>

#define GPV_ENC_FN __host__ __device__ inline
#include "jpeg_enc_host.h"
#include "../../include/gpv_enc.h"

namespace R = gpv_enc_rule;

static_assert(GPV_ENC_HEADER_BYTES == R::HEADER_BYTES && GPV_ENC_MAX_BOXES == R::MAX_BOXES && GPV_ENC_MAX_LABEL == R::MAX_LABEL, "header constants");
static_assert(GPV_ENC_BLOCK_BYTES * 8 >= R::MAX_BLOCK_BITS && GPV_ENC_BLOCK_BYTES % 16 == 0, "packed bytes per block");
static_assert(sizeof(gpv_enc_desc) == 80, "descriptor size (workspace formula)");
static_assert((int64_t)GPV_ENC_MAX_BLOCKS * GPV_ENC_BLOCK_BYTES * 8 < ((int64_t)1 << 31), "bit offsets are 32-bit");

namespace {

__constant__ const R::Tables d_T = R::make_tables();
__constant__ const R::LabelFont d_font = R::make_label_font();
constexpr R::Tables h_T = R::make_tables();

constexpr int COEF_THREADS = 256, ROW = COEF_THREADS + 2;     // LDS row of one zigzag position: + 2 keeps the transposed read off one bank
constexpr int IMG_THREADS = 1024;                             // workgroup of the per-picture kernels: 16 waves
constexpr int CHUNK = 16;                                     // scan bytes per thread and round of the stuffing kernel

struct Header {
  uint8_t b[(R::HEADER_BYTES + 3) & ~3];
};

// where the parts of the workspace start, in bytes (include/gpv_enc.h states the sum)
struct Layout {
  int64_t counts, coefs, bits, diffs, packed, total;
};
__host__ __device__ inline Layout layout(int B, int64_t blocks) {
  Layout l;
  int64_t words = (blocks * 4 + 15) & ~(int64_t)15;
  l.counts = (int64_t)B * 80;
  l.coefs = l.counts + (int64_t)B * 16;
  l.bits = l.coefs + blocks * 128;
  l.diffs = l.bits + words;
  l.packed = l.diffs + words;
  l.total = (int64_t)B * 128 + blocks * 344 + 32;             // >= packed + blocks * 208 + B * 32
  return l;
}
// the packed bits of picture i: GPV_ENC_BLOCK_BYTES per block and 32 bytes of slack
__device__ inline uint32_t* packed_of(char* ws, const Layout& l, int i, int block_base) {
  return (uint32_t*)(ws + l.packed + (int64_t)block_base * GPV_ENC_BLOCK_BYTES + (int64_t)i * 32);
}
__device__ inline int packed_words(int nblocks) { return nblocks * (GPV_ENC_BLOCK_BYTES / 4) + 8; }

struct LdsColumn {                       // one thread's 64 values, one per LDS row
  int16_t* base;
  __device__ int16_t& operator[](int k) const { return base[k * ROW]; }
};

struct LabelStage {                      // what the workgroup stages of its picture's labels (LDS)
  R::Label label[R::MAX_BOXES];
  uint8_t glyph[R::MAX_BOXES * R::MAX_LABEL];   // glyph_of of every text byte
  R::LabelFont font;
};

// component `comp` of the pixel at (x, y), the box outlines drawn over the source and, with LABELS, the labels over the outlines.
// touched: bit n = the plate of box n reaches the footprint of the thread's block (labels_touching); others are not looked at.
template <bool LABELS>
struct Pixels {
  const void* src;
  int pitch, kind, nbox;
  float mean[3], std[3];
  const int (*rect)[4];
  const uint8_t (*colour)[4];
  const LabelStage* stage;
  uint32_t touched;
  __device__ int operator()(int x, int y, int comp) const {
    int64_t i = (int64_t)y * pitch + x;
    int r, g, b;
    if (kind == GPV_ENC_SRC_U8) {
      const uint8_t* p = (const uint8_t*)src + i * 3;
      r = p[0], g = p[1], b = p[2];
    } else {
      float fr, fg, fb;
      if (kind == GPV_ENC_SRC_BF16) {
        uint2 v = ((const uint2*)src)[i];
        fr = __uint_as_float(v.x << 16), fg = __uint_as_float(v.x & 0xFFFF0000u), fb = __uint_as_float(v.y << 16);
      } else {
        float4 v = ((const float4*)src)[i];
        fr = v.x, fg = v.y, fb = v.z;
      }
      r = R::denormalise(fr, mean[0], std[0]), g = R::denormalise(fg, mean[1], std[1]), b = R::denormalise(fb, mean[2], std[2]);
    }
    for (int n = 0; n < nbox; ++n)
      if (R::on_outline(rect[n], x, y)) r = colour[n][0], g = colour[n][1], b = colour[n][2];
    if constexpr (LABELS) {
      int last = -1;                                         // a later label overwrites an earlier one: only the last one shows
      for (uint32_t m = touched; m; m &= m - 1) {
        const int n = __builtin_ctz(m);
        if (R::on_plate(stage->label[n], x, y)) last = n;
      }
      if (last >= 0) {
        const bool ink = R::label_ink(stage->label[last], stage->font, stage->glyph, x, y);
        r = ink ? colour[last][0] : R::PLATE_RGB, g = ink ? colour[last][1] : R::PLATE_RGB, b = ink ? colour[last][2] : R::PLATE_RGB;
      }
    }
    return R::ycc(comp, r, g, b);
  }
};

// the plates that reach the source pixels block b samples: 8 x 8 for a full-resolution component, 8 hs x 8 vs for down-sampled
// chroma, the clamps of sample_block applied to both ends (they are monotone, so no sampled pixel lies outside)
__device__ inline uint32_t labels_touching(const LabelStage& st, int nbox, const R::Geometry& g, const R::Block& b, int H, int W) {
  const bool full = b.comp == 0 || (g.hs == 1 && g.vs == 1);
  const int sx = full ? 1 : 2, sy = full ? 1 : g.vs;
  int x0 = b.bx * 8 * sx, x1 = x0 + 8 * sx - 1, y0 = b.by * 8 * sy, y1 = y0 + 8 * sy - 1;
  x0 = x0 < W - 1 ? x0 : W - 1, x1 = x1 < W - 1 ? x1 : W - 1, y0 = y0 < H - 1 ? y0 : H - 1, y1 = y1 < H - 1 ? y1 : H - 1;
  uint32_t m = 0;
  for (int n = 0; n < nbox; ++n) {
    const R::Label& l = st.label[n];
    if (l.n > 0 && l.px <= x1 && l.px + R::CELL_W * l.n + 2 > x0 && l.py <= y1 && l.py + R::PLATE_H > y0) m |= 1u << n;
  }
  return m;
}

// 1. pixels -> quantised coefficients in zigzag order and the bit count of each block's AC code.  grid (blocks of the largest
// picture / 256, B); a thread whose block index is beyond its picture's count only helps with the barriers.
// LABELS (a compile-time tag: without it this is the kernel as it was): the pictures' labels are staged and drawn as well.
template <bool LABELS>
__global__ __launch_bounds__(COEF_THREADS) void gpv_enc_coef_kernel(char* ws, int B, int64_t blocks, R::Quant Q, int hs, int vs) {
  __shared__ int16_t s_zz[64 * ROW];
  __shared__ int s_rect[R::MAX_BOXES][4];
  __shared__ uint8_t s_colour[R::MAX_BOXES][4];
  const Layout l = layout(B, blocks);
  const gpv_enc_desc D = ((const gpv_enc_desc*)ws)[blockIdx.y];
  const int tid = threadIdx.x, first = blockIdx.x * COEF_THREADS, k = first + tid;
  if (first >= D.nblocks) return;                            // the whole workgroup leaves
  const int nbox = D.nboxes < 0 ? 0 : D.nboxes > R::MAX_BOXES ? R::MAX_BOXES : D.nboxes;
  if (tid < nbox) {
    R::box_rect(D.boxes + 4 * tid, D.H, D.W, s_rect[tid]);
    for (int c = 0; c < 4; ++c) s_colour[tid][c] = D.colours[4 * tid + c];
  }
  __syncthreads();
  const LabelStage* stage = nullptr;
  if constexpr (LABELS) {
    __shared__ LabelStage st;
    stage = &st;
    // the extents the host has checked, clamped again: no index below leaves colours[0 .. 4 nbox + nlab) or the glyph table
    const int most = nbox * R::MAX_LABEL, nlab = D.labels < 0 ? 0 : D.labels > most ? most : D.labels;
    if (tid == 0) {                                          // at most 32 boxes: a serial prefix sum over the length bytes
      int before = 0;
      for (int n = 0; n < nbox; ++n) {
        st.label[n] = R::label_place(s_rect[n], s_colour[n][3], before, nlab, D.H, D.W);
        before += s_colour[n][3] & 0x7F;
      }
    }
    for (int i = tid; i < nlab; i += COEF_THREADS) st.glyph[i] = (uint8_t)R::glyph_of(D.colours[4 * nbox + i]);
    if (nlab > 0)                                            // (a picture without labels in a call that has some: every n is 0)
      for (int i = tid; i < (int)sizeof(R::LabelFont); i += COEF_THREADS) ((uint8_t*)&st.font)[i] = ((const uint8_t*)&d_font)[i];
    __syncthreads();
  }
  const R::Geometry g = R::geometry(D.H, D.W, hs, vs);
  LdsColumn col{s_zz + tid};
  int acbits = 0;
  if (k < D.nblocks) {
    const R::Block b = R::block_at(g, k);
    const int t = b.comp ? 1 : 0;
    if (b.dummy) {
      for (int i = 0; i < 64; ++i) col[i] = 0;
    } else {
      Pixels<LABELS> px{D.src, D.pitch, D.kind, nbox, {D.mean[0], D.mean[1], D.mean[2]}, {D.std[0], D.std[1], D.std[2]}, s_rect, s_colour, stage, 0};
      if constexpr (LABELS) px.touched = labels_touching(*stage, nbox, g, b, D.H, D.W);
      R::sample_block(px, g, b, D.H, D.W, col);
      int d[64];
#pragma unroll
      for (int i = 0; i < 64; ++i) d[i] = col[i];
      R::fdct(d);
      constexpr R::Tables T = R::make_tables();
#pragma unroll
      for (int i = 0; i < 64; ++i) col[i] = (int16_t)R::quantise(d[T.zigzag[i]], Q.d[t][T.zigzag[i]], Q.m[t][T.zigzag[i]]);
    }
    R::CountBits count;
    R::code_block(d_T, col, 0, t, count);
    acbits = count.bits - d_T.dc_len[t][0];
    ((int*)(ws + l.bits))[D.block_base + k] = acbits;
  }
  __syncthreads();
  // the workgroup's blocks are one contiguous run of the coefficient array: written two values per thread and round
  uint32_t* out = (uint32_t*)(ws + l.coefs) + ((int64_t)D.block_base + first) * 32;
  const int have = D.nblocks - first < COEF_THREADS ? D.nblocks - first : COEF_THREADS;
  for (int w = tid; w < have * 32; w += COEF_THREADS) {
    int blk = w >> 5, kk = (w & 31) * 2;
    out[w] = (uint32_t)(uint16_t)s_zz[kk * ROW + blk] | ((uint32_t)(uint16_t)s_zz[(kk + 1) * ROW + blk] << 16);
  }
}

// inclusive scan over the workgroup's IMG_THREADS values: wave64 shuffles, then the 16 wave sums; *total = the sum of all
__device__ inline int block_scan(int v, int* s_wave, int* total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  __syncthreads();                                           // the previous round's readers of s_wave are done
  if (lane == 63) s_wave[wave] = v;
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < IMG_THREADS / 64; ++w) {
    before += w < wave ? s_wave[w] : 0;
    all += s_wave[w];
  }
  *total = all;
  return v + before;
}

// the DC value block k codes: its own, or for a dummy block that of the block coded before it in the MCU (block 0 is never a dummy)
__device__ inline int dc_of(const int16_t* coefs, const R::Geometry& g, int k) {
  while (R::block_at(g, k).dummy) --k;
  return coefs[(int64_t)k * 64];
}

// 2. per picture: DC differences, the exclusive scan of the blocks' bit counts, the bit and byte counts, the zeroed bit buffer
__global__ __launch_bounds__(IMG_THREADS) void gpv_enc_offsets_kernel(char* ws, int B, int64_t blocks, int hs, int vs) {
  __shared__ int s_wave[IMG_THREADS / 64];
  const Layout l = layout(B, blocks);
  const int img = blockIdx.x, tid = threadIdx.x;
  const gpv_enc_desc D = ((const gpv_enc_desc*)ws)[img];
  const R::Geometry g = R::geometry(D.H, D.W, hs, vs);
  const int16_t* coefs = (const int16_t*)(ws + l.coefs) + (int64_t)D.block_base * 64;
  int* bits = (int*)(ws + l.bits) + D.block_base;
  int* diffs = (int*)(ws + l.diffs) + D.block_base;
  const int nl = hs * vs;
  int carry = 0;
  for (int first = 0; first < D.nblocks; first += IMG_THREADS) {
    const int k = first + tid;
    int n = 0;
    if (k < D.nblocks) {
      const R::Block b = R::block_at(g, k);
      // the component's previous block in scan order: the luma block before it in the MCU, the last luma block of the MCU before,
      // the same chroma block of the MCU before
      int prev = b.comp == 0 ? (b.j > 0 ? k - 1 : k - g.per_mcu + nl - 1) : k - g.per_mcu;
      int diff = dc_of(coefs, g, k) - (prev >= 0 ? dc_of(coefs, g, prev) : 0);
      int t = b.comp ? 1 : 0, cat = R::bit_length(diff < 0 ? -diff : diff);
      cat = cat > 11 ? 11 : cat;                             // cannot happen (|DC| <= 1024); keeps the table index inside
      diffs[k] = diff;
      n = bits[k] + d_T.dc_len[t][cat] + cat;
    }
    int total, incl = block_scan(n, s_wave, &total);
    if (k < D.nblocks) bits[k] = carry + incl - n;
    carry += total;
  }
  const int nbytes = (carry + 7) >> 3;
  if (tid == 0) {
    int* counts = (int*)(ws + l.counts) + 4 * img;
    counts[0] = carry, counts[1] = nbytes;
  }
  uint32_t* packed = packed_of(ws, l, img, D.block_base);
  int words = (nbytes + 3) / 4 + 4, cap = packed_words(D.nblocks);
  words = words < cap ? words : cap;
  for (int w = tid; w < words; w += IMG_THREADS) packed[w] = 0;
}

struct Packer {                          // bits into 32-bit words, most significant bit first
  uint32_t* words;
  int cap, w, used;                      // word index, bits of `cur` in use
  uint32_t cur;
  bool shared;                           // the word may hold a neighbour's bits
  __device__ void flush() {
    if (w < cap) {
      if (shared) atomicOr(words + w, cur);
      else words[w] = cur;
    }
    ++w, cur = 0, used = 0, shared = false;
  }
  __device__ void operator()(uint32_t v, int n) {            // 1 <= n <= 16, v < 2^n
    if (used + n <= 32) {
      cur |= v << (32 - used - n);
      used += n;
      if (used == 32) flush();
    } else {
      int rest = used + n - 32;
      cur |= v >> rest;
      flush();
      cur = v << (32 - rest), used = rest;
    }
  }
};

// 3. every block's bits at its offset.  grid as kernel 1.
__global__ __launch_bounds__(COEF_THREADS) void gpv_enc_pack_kernel(char* ws, int B, int64_t blocks, int hs, int vs) {
  const Layout l = layout(B, blocks);
  const int img = blockIdx.y, k = blockIdx.x * COEF_THREADS + threadIdx.x;
  const gpv_enc_desc D = ((const gpv_enc_desc*)ws)[img];
  if (k >= D.nblocks) return;
  const R::Geometry g = R::geometry(D.H, D.W, hs, vs);
  const R::Block b = R::block_at(g, k);
  const int64_t at = (int64_t)D.block_base + k;
  const int16_t* zz = (const int16_t*)(ws + l.coefs) + at * 64;
  const int pos = ((const int*)(ws + l.bits))[at], diff = ((const int*)(ws + l.diffs))[at];
  Packer put{packed_of(ws, l, img, D.block_base), packed_words(D.nblocks), pos >> 5, pos & 31, 0, true};
  R::code_block(d_T, zz, diff, b.comp ? 1 : 0, put);
  if (k == D.nblocks - 1) {                                  // the last byte is filled with 1-bits
    int fill = (8 - (put.used & 7)) & 7;
    if (fill) put((1u << fill) - 1, fill);
  }
  put.shared = true;
  if (put.used) put.flush();
}

// 4. per picture: header, the scan's bytes with a 0x00 behind every 0xFF, EOI, the file's size and status
__global__ __launch_bounds__(IMG_THREADS) void gpv_enc_bytes_kernel(char* ws, int B, int64_t blocks, Header hdr, unsigned char* out, int64_t capacity,
                                                                    int* sizes, int* status) {
  __shared__ int s_wave[IMG_THREADS / 64];
  const Layout l = layout(B, blocks);
  const int img = blockIdx.x, tid = threadIdx.x;
  const gpv_enc_desc D = ((const gpv_enc_desc*)ws)[img];
  const int nbytes = ((const int*)(ws + l.counts))[4 * img + 1];
  const uint32_t* packed = packed_of(ws, l, img, D.block_base);
  const int cap_words = packed_words(D.nblocks);
  unsigned char* file = out + (int64_t)img * capacity;
  for (int i = tid; i < R::HEADER_BYTES; i += IMG_THREADS) {
    uint8_t v = hdr.b[i];
    if (i == R::HEADER_H_AT) v = (uint8_t)(D.H >> 8);
    if (i == R::HEADER_H_AT + 1) v = (uint8_t)D.H;
    if (i == R::HEADER_H_AT + 2) v = (uint8_t)(D.W >> 8);
    if (i == R::HEADER_H_AT + 3) v = (uint8_t)D.W;
    if (i < capacity) file[i] = v;
  }
  int64_t at = R::HEADER_BYTES;                              // where the round's first byte goes
  for (int first = 0; first < nbytes; first += IMG_THREADS * CHUNK) {
    const int mine = first + tid * CHUNK;
    uint32_t w[CHUNK / 4];
    int ff = 0;
    for (int i = 0; i < CHUNK / 4; ++i) {
      int idx = mine / 4 + i;
      w[i] = packed[idx < cap_words ? idx : cap_words - 1];  // a clamped load; bytes at or beyond nbytes are not used
      for (int j = 0; j < 4; ++j) ff += (mine + 4 * i + j < nbytes) && ((w[i] >> (24 - 8 * j)) & 255) == 255;
    }
    int total, incl = block_scan(ff, s_wave, &total);
    int64_t p = at + (mine - first) + (incl - ff);
    for (int i = 0; i < CHUNK; ++i) {
      if (mine + i >= nbytes) break;
      uint8_t v = (uint8_t)(w[i >> 2] >> (24 - 8 * (i & 3)));
      if (p < capacity) file[p] = v;
      ++p;
      if (v == 255) {
        if (p < capacity) file[p] = 0;
        ++p;
      }
    }
    int round_bytes = nbytes - first < IMG_THREADS * CHUNK ? nbytes - first : IMG_THREADS * CHUNK;
    at += round_bytes + total;
  }
  if (tid == 0) {
    if (at < capacity) file[at] = 0xFF;
    if (at + 1 < capacity) file[at + 1] = 0xD9;
    sizes[img] = (int)(at + 2);
    status[img] = at + 2 > capacity ? GPV_ENC_STATUS_CAPACITY : 0;
  }
}

bool factors(int subsampling, int* hs, int* vs) {
  if (subsampling != GPV_ENC_444 && subsampling != GPV_ENC_422 && subsampling != GPV_ENC_420) return false;
  *hs = subsampling == GPV_ENC_444 ? 1 : 2, *vs = subsampling == GPV_ENC_420 ? 2 : 1;
  return true;
}

}  // namespace

extern "C" {

int gpv_enc_workspace_bytes(int B, int64_t blocks, int64_t* bytes) {
  if (B < 1 || blocks < B || blocks > GPV_ENC_MAX_TOTAL_BLOCKS || !bytes) return hipErrorInvalidValue;
  *bytes = layout(B, blocks).total;
  return hipSuccess;
}

int gpv_enc_header(int H, int W, int quality, int subsampling, unsigned char* buf, int* nbytes) {
  int hs, vs;
  if (H < 1 || H > 65535 || W < 1 || W > 65535 || quality < 1 || quality > 100 || !factors(subsampling, &hs, &vs) || !buf || !nbytes)
    return hipErrorInvalidValue;
  R::write_header(h_T, R::make_quant(h_T, quality), H, W, hs, vs, buf);
  *nbytes = R::HEADER_BYTES;
  return hipSuccess;
}

int gpv_enc_encode(gpv_enc_desc* descs, int B, int quality, int subsampling, void* workspace, int64_t workspace_bytes,
                   unsigned char* out, int64_t capacity, int* sizes, int* status, void* stream) {
  int hs, vs;
  if (!descs || B < 1 || B > 65535 || quality < 1 || quality > 100 || !factors(subsampling, &hs, &vs) || !workspace ||
      ((uintptr_t)workspace & 15) || !out || capacity < 1 || !sizes || !status)
    return hipErrorInvalidValue;
  int64_t blocks = 0;
  int largest = 0;
  bool labelled = false;
  for (int i = 0; i < B; ++i) {
    gpv_enc_desc& d = descs[i];
    if (d.H < 1 || d.H > 65535 || d.W < 1 || d.W > 65535 || d.pitch < d.W || !d.src || d.nboxes < 0 || d.nboxes > GPV_ENC_MAX_BOXES ||
        (d.nboxes && (!d.boxes || !d.colours)) || d.kind < GPV_ENC_SRC_U8 || d.kind > GPV_ENC_SRC_F32 ||
        (d.kind == GPV_ENC_SRC_BF16 && ((uintptr_t)d.src & 7)) || (d.kind == GPV_ENC_SRC_F32 && ((uintptr_t)d.src & 15)) ||
        d.labels < 0 || d.labels > d.nboxes * GPV_ENC_MAX_LABEL)     // (labels > 0 with no boxes is the second one)
      return hipErrorInvalidValue;
    labelled |= d.labels > 0;
    int64_t n = (int64_t)((((d.W + hs - 1) / hs) + 7) / 8) * ((((d.H + vs - 1) / vs) + 7) / 8) * (hs * vs + 2);
    if (n > GPV_ENC_MAX_BLOCKS || blocks + n > GPV_ENC_MAX_TOTAL_BLOCKS) return hipErrorInvalidValue;
    blocks += n;
    largest = n > largest ? (int)n : largest;
  }
  if (workspace_bytes < layout(B, blocks).total) return hipErrorInvalidValue;
  blocks = 0;
  for (int i = 0; i < B; ++i) {                              // nothing is written before every check has passed
    descs[i].nblocks = R::geometry(descs[i].H, descs[i].W, hs, vs).nblocks;
    descs[i].block_base = (int)blocks;
    blocks += descs[i].nblocks;
  }
  hipStream_t s = (hipStream_t)stream;
  hipError_t err = hipMemcpyAsync(workspace, descs, (size_t)B * sizeof(gpv_enc_desc), hipMemcpyHostToDevice, s);
  if (err != hipSuccess) return err;
  const R::Quant Q = R::make_quant(h_T, quality);
  Header hdr{};
  R::write_header(h_T, Q, 0, 0, hs, vs, hdr.b);
  char* ws = (char*)workspace;
  const dim3 per_block((largest + COEF_THREADS - 1) / COEF_THREADS, B);
  if (labelled)                                              // a call without labels runs the kernel without them
    hipLaunchKernelGGL(gpv_enc_coef_kernel<true>, per_block, dim3(COEF_THREADS), 0, s, ws, B, blocks, Q, hs, vs);
  else
    hipLaunchKernelGGL(gpv_enc_coef_kernel<false>, per_block, dim3(COEF_THREADS), 0, s, ws, B, blocks, Q, hs, vs);
  hipLaunchKernelGGL(gpv_enc_offsets_kernel, dim3(B), dim3(IMG_THREADS), 0, s, ws, B, blocks, hs, vs);
  hipLaunchKernelGGL(gpv_enc_pack_kernel, per_block, dim3(COEF_THREADS), 0, s, ws, B, blocks, hs, vs);
  hipLaunchKernelGGL(gpv_enc_bytes_kernel, dim3(B), dim3(IMG_THREADS), 0, s, ws, B, blocks, hdr, out, capacity, sizes, status);
  return hipGetLastError();
}

}  // extern "C"
