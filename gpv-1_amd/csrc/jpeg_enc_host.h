// The JPEG encoding rule of gpv1_amd.jpeg_encode in plain C++ (no HIP): tables, header, colour, sampling, transform, quantiser and
// the entropy code of one block, and the labels of the boxes (tools/label_host_check.cpp).  jpeg_enc.hip compiles the same functions for the device (it defines GPV_ENC_FN as
// __host__ __device__ inline before including this file) and tools/enc_host_check.cpp includes it as it stands, so what the
// stand-alone check proves about these functions holds for the kernels' arithmetic too.  DESIGN.md section 6h.
#ifndef GPV_JPEG_ENC_HOST_H
#define GPV_JPEG_ENC_HOST_H
#include <stdint.h>
#include <vector>
#ifndef GPV_ENC_FN
#define GPV_ENC_FN inline
#endif

namespace gpv_enc_rule {

constexpr int HEADER_BYTES = 623;       // SOI 2, APP0 18, DQT 2 x 69, SOF0 19, DHT 2 x (33 + 183), SOS 14
constexpr int HEADER_H_AT = 163;        // H and W, two big-endian bytes each, inside SOF0
constexpr int MAX_BLOCK_BITS = 20 + 63 * 26;   // DC: 9-bit code + 11 bits; every AC value: 16-bit code + 10 bits
constexpr int MAX_BOXES = 32;
constexpr int MAX_ABS_COEF = 32767;     // |8 x DCT| <= 8 * 64 * 128 / 4 = 16384 before rounding; the quantiser is proved up to here

struct Tables {
  uint8_t zigzag[64];                   // natural index of zigzag position k
  uint8_t qbase[2][64];                 // Annex K quantisation tables, natural order
  uint8_t dc_bits[2][16], ac_bits[2][16], dc_vals[2][12], ac_vals[2][162];
  uint16_t dc_code[2][12], ac_code[2][256];
  uint8_t dc_len[2][12], ac_len[2][256];
};

constexpr Tables make_tables() {
  constexpr uint8_t zz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                              41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                              30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  constexpr uint8_t ql[64] = {16, 11, 10, 16, 24, 40, 51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                              69, 56, 14, 17, 22, 29, 51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                              81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,  95,  98,  112, 100, 103, 99};
  constexpr uint8_t qc[32] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99,
                              24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99};
  constexpr uint8_t dcb[2][16] = {{0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0}, {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0}};
  constexpr uint8_t acb[2][16] = {{0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125}, {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119}};
  constexpr uint8_t acv[2][162] = {
      {1,   2,   3,   0,   4,   17,  5,   18,  33,  49,  65,  6,   19,  81,  97,  7,   34,  113, 20,  50,  129, 145, 161, 8,   35,
       66,  177, 193, 21,  82,  209, 240, 36,  51,  98,  114, 130, 9,   10,  22,  23,  24,  25,  26,  37,  38,  39,  40,  41,  42,
       52,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,  100,
       101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133, 134, 135, 136, 137, 138, 146, 147, 148,
       149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185, 186, 194,
       195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 225, 226, 227, 228, 229, 230, 231, 232,
       233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250},
      {0,   1,   2,   3,   17,  4,   5,   33,  49,  6,   18,  65,  81,  7,   97,  113, 19,  34,  50,  129, 8,   20,  66,  145, 161,
       177, 193, 9,   35,  51,  82,  240, 21,  98,  114, 209, 10,  22,  36,  52,  225, 37,  241, 23,  24,  25,  26,  38,  39,  40,
       41,  42,  53,  54,  55,  56,  57,  58,  67,  68,  69,  70,  71,  72,  73,  74,  83,  84,  85,  86,  87,  88,  89,  90,  99,
       100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131, 132, 133, 134, 135, 136, 137, 138, 146,
       147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179, 180, 181, 182, 183, 184, 185,
       186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218, 226, 227, 228, 229, 230, 231,
       232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250}};
  Tables t{};
  for (int i = 0; i < 64; ++i) {
    t.zigzag[i] = zz[i];
    t.qbase[0][i] = ql[i];
    t.qbase[1][i] = i < 32 ? qc[i] : 99;
  }
  for (int c = 0; c < 2; ++c) {
    for (int i = 0; i < 16; ++i) t.dc_bits[c][i] = dcb[c][i], t.ac_bits[c][i] = acb[c][i];
    for (int i = 0; i < 12; ++i) t.dc_vals[c][i] = (uint8_t)i;
    for (int i = 0; i < 162; ++i) t.ac_vals[c][i] = acv[c][i];
    int code = 0, k = 0;                 // Annex C: codes of one length are consecutive, the next length starts at twice the next code
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < dcb[c][len - 1]; ++i, ++code, ++k) t.dc_code[c][k] = (uint16_t)code, t.dc_len[c][k] = (uint8_t)len;
      code <<= 1;
    }
    code = 0, k = 0;
    for (int len = 1; len <= 16; ++len) {
      for (int i = 0; i < acb[c][len - 1]; ++i, ++code, ++k) t.ac_code[c][acv[c][k]] = (uint16_t)code, t.ac_len[c][acv[c][k]] = (uint8_t)len;
      code <<= 1;
    }
  }
  return t;
}

// d = q << 3 per entry in natural order, [0] luma, [1] chroma; m = ceil(2^32 / d): the multiply-and-shift form of the division
struct Quant {
  uint16_t d[2][64];
  uint32_t m[2][64];
};

inline Quant make_quant(const Tables& T, int quality) {
  Quant Q;
  int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int c = 0; c < 2; ++c)
    for (int i = 0; i < 64; ++i) {
      int q = (T.qbase[c][i] * scale + 50) / 100;
      q = q < 1 ? 1 : q > 255 ? 255 : q;
      Q.d[c][i] = (uint16_t)(q << 3);
      Q.m[c][i] = (uint32_t)((((uint64_t)1 << 32) + (uint64_t)(q << 3) - 1) / (uint64_t)(q << 3));
    }
  return Q;
}

// the rule's quantiser: t = (|c| + (d >> 1)) / d, the sign put back
GPV_ENC_FN int quantise_div(int c, int d) {
  int a = c < 0 ? -c : c, t = (a + (d >> 1)) / d;
  return c < 0 ? -t : t;
}
// what the kernels run: equal to quantise_div for |c| <= MAX_ABS_COEF and d = 8 q, q = 1..255 (tools/enc_host_check.cpp tries them all)
GPV_ENC_FN int quantise(int c, uint32_t d, uint32_t m) {
  uint32_t a = (uint32_t)(c < 0 ? -c : c);
  int t = (int)(((uint64_t)(a + (d >> 1)) * m) >> 32);
  return c < 0 ? -t : t;
}

GPV_ENC_FN int bit_length(int a) {      // of a >= 0
  int n = 0;
  while (a) ++n, a >>= 1;
  return n;
}

// 16 fractional bits, FIX(x) = int(x * 65536 + 0.5); comp 0 / 1 / 2 = Y / Cb / Cr
GPV_ENC_FN int ycc(int comp, int r, int g, int b) {
  if (comp == 0) return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16;
  if (comp == 1) return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16;
  return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16;
}

GPV_ENC_FN int descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// one pass of jfdctint over 8 values at stride s: 13 constant bits, 2 pass-1 bits
GPV_ENC_FN void fdct_pass(int* d, int s, bool first) {
  int t0 = d[0] + d[7 * s], t7 = d[0] - d[7 * s], t1 = d[s] + d[6 * s], t6 = d[s] - d[6 * s];
  int t2 = d[2 * s] + d[5 * s], t5 = d[2 * s] - d[5 * s], t3 = d[3 * s] + d[4 * s], t4 = d[3 * s] - d[4 * s];
  int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
  int n = first ? 13 - 2 : 13 + 2;
  d[0] = first ? (t10 + t11) * 4 : descale(t10 + t11, 2);
  d[4 * s] = first ? (t10 - t11) * 4 : descale(t10 - t11, 2);
  int z1 = (t12 + t13) * 4433;
  d[2 * s] = descale(z1 + t13 * 6270, n);
  d[6 * s] = descale(z1 - t12 * 15137, n);
  z1 = t4 + t7;
  int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7, z5 = (z3 + z4) * 9633;
  t4 *= 2446, t5 *= 16819, t6 *= 25172, t7 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  d[7 * s] = descale(t4 + z1 + z3, n);
  d[5 * s] = descale(t5 + z2 + z4, n);
  d[3 * s] = descale(t6 + z2 + z3, n);
  d[s] = descale(t7 + z1 + z4, n);
}

// d[64] = sample - 128, row-major -> 8 x the transform: rows first, then columns
GPV_ENC_FN void fdct(int* d) {
#pragma unroll
  for (int i = 0; i < 8; ++i) fdct_pass(d + 8 * i, 1, true);
#pragma unroll
  for (int i = 0; i < 8; ++i) fdct_pass(d + i, 8, false);
}

struct Geometry {
  int hs, vs;                 // luma sampling factors
  int bw, bh;                 // luma block columns / rows: ceil(W / 8), ceil(H / 8)
  int cw, ch;                 // chroma samples: ceil(W / hs), ceil(H / vs)
  int mx, my;                 // MCU columns / rows = chroma block columns / rows
  int per_mcu;                // hs * vs + 2
  int nblocks;                // mx * my * per_mcu, dummy blocks included
};

GPV_ENC_FN Geometry geometry(int H, int W, int hs, int vs) {
  Geometry g;
  g.hs = hs, g.vs = vs;
  g.bw = (W + 7) / 8, g.bh = (H + 7) / 8;
  g.cw = (W + hs - 1) / hs, g.ch = (H + vs - 1) / vs;
  g.mx = (g.cw + 7) / 8, g.my = (g.ch + 7) / 8;
  g.per_mcu = hs * vs + 2;
  g.nblocks = g.mx * g.my * g.per_mcu;
  return g;
}

struct Block {
  int comp, bx, by;           // component and block position inside the component
  int mcu, j;                 // MCU index (row-major) and place inside the MCU
  bool dummy;                 // beyond the component's own block columns or rows
};

// block k of the scan: MCUs row-major; inside one, vs x hs luma blocks row-major, then Cb, then Cr
GPV_ENC_FN Block block_at(const Geometry& g, int k) {
  Block b;
  b.mcu = k / g.per_mcu, b.j = k % g.per_mcu;
  int my = b.mcu / g.mx, mx = b.mcu % g.mx, nl = g.hs * g.vs;
  if (b.j < nl) {
    b.comp = 0, b.by = my * g.vs + b.j / g.hs, b.bx = mx * g.hs + b.j % g.hs;
    b.dummy = b.bx >= g.bw || b.by >= g.bh;
  } else {
    b.comp = 1 + b.j - nl, b.by = my, b.bx = mx, b.dummy = false;
  }
  return b;
}

// The 64 samples (minus 128) of a real block into d[0..63] (anything with operator[]).  px(x, y, comp) = component `comp` of the pixel at 0 <= x < W, 0 <= y < H.
// Luma: the plane repeats its last column and row.  Chroma columns: the full-resolution plane repeats its last column as far as the
// blocks reach, the bias alternates along the output row.  Chroma rows: the full-resolution plane repeats its last row to a whole
// group of vs rows; below that the down-sampled plane repeats its own last row.
template <class Px, class D>
GPV_ENC_FN void sample_block(const Px& px, const Geometry& g, const Block& b, int H, int W, D& d) {
  bool full = b.comp == 0 || (g.hs == 1 && g.vs == 1);
  for (int i = 0; i < 8; ++i) {
    int row = b.by * 8 + i;
    int y0, y1;
    if (full) {
      y0 = y1 = row < H - 1 ? row : H - 1;
    } else {
      int cy = row < g.ch - 1 ? row : g.ch - 1;
      y0 = cy * g.vs, y1 = y0 + g.vs - 1;
      y0 = y0 < H - 1 ? y0 : H - 1, y1 = y1 < H - 1 ? y1 : H - 1;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      int col = b.bx * 8 + j, v;
      if (full) {
        v = px(col < W - 1 ? col : W - 1, y0, b.comp);
      } else {
        int x0 = 2 * col < W - 1 ? 2 * col : W - 1, x1 = 2 * col + 1 < W - 1 ? 2 * col + 1 : W - 1;
        if (g.vs == 2)
          v = (px(x0, y0, b.comp) + px(x1, y0, b.comp) + px(x0, y1, b.comp) + px(x1, y1, b.comp) + 1 + (col & 1)) >> 2;
        else
          v = (px(x0, y0, b.comp) + px(x1, y0, b.comp) + (col & 1)) >> 1;
      }
      d[8 * i + j] = v - 128;
    }
  }
}

// the entropy code of one block: zz[k] = the quantised values in zigzag order ([0] is not read; anything with operator[]), diff = DC minus the component's
// previous DC, t = 0 luma / 1 chroma tables.  put(value, bit count) receives the codes and the appended bits in order.
template <class Z, class Put>
GPV_ENC_FN void code_block(const Tables& T, const Z& zz, int diff, int t, Put& put) {
  int n = bit_length(diff < 0 ? -diff : diff);
  put(T.dc_code[t][n], T.dc_len[t][n]);
  if (n) put((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << n) - 1), n);
  int run = 0;
  for (int k = 1; k < 64; ++k) {
    int v = zz[k];
    if (v == 0) {
      ++run;
      continue;
    }
    for (; run > 15; run -= 16) put(T.ac_code[t][0xF0], T.ac_len[t][0xF0]);
    n = bit_length(v < 0 ? -v : v);
    put(T.ac_code[t][(run << 4) + n], T.ac_len[t][(run << 4) + n]);
    put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << n) - 1), n);
    run = 0;
  }
  if (run) put(T.ac_code[t][0], T.ac_len[t][0]);
}

struct CountBits {
  int bits = 0;
  GPV_ENC_FN void operator()(uint32_t, int n) { bits += n; }
};

// normalised (cx, cy, w, h) -> x1, y1, x2, y2 as vis_bbox clamps them, rounded half to even; fp32, every operation on its own
// (compile without contraction where the result is compared)
GPV_ENC_FN void box_rect(const float* box, int H, int W, int* rect) {
  float hw = box[2] * 0.5f, hh = box[3] * 0.5f;
  float x1 = (box[0] - hw) * (float)W, x2 = (box[0] + hw) * (float)W, y1 = (box[1] - hh) * (float)H, y2 = (box[1] + hh) * (float)H;
  float xm = (float)(W - 1), ym = (float)(H - 1);
  x1 = x1 < xm ? x1 : xm, x1 = x1 > 0.f ? x1 : 0.f;
  x2 = x2 < xm ? x2 : xm, x2 = x2 > x1 ? x2 : x1;
  y1 = y1 < ym ? y1 : ym, y1 = y1 > 0.f ? y1 : 0.f;
  y2 = y2 < ym ? y2 : ym, y2 = y2 > y1 ? y2 : y1;
  rect[0] = (int)__builtin_rintf(x1), rect[1] = (int)__builtin_rintf(y1), rect[2] = (int)__builtin_rintf(x2), rect[3] = (int)__builtin_rintf(y2);
}

GPV_ENC_FN bool on_outline(const int* r, int x, int y) {
  return x >= r[0] && x <= r[2] && y >= r[1] && y <= r[3] && (x == r[0] || x == r[2] || y == r[1] || y == r[3]);
}

// The labels of the boxes (include/gpv_enc.h states the rule): a text of n <= MAX_LABEL characters in the 6 x 11 cell of the glyph
// table, on a dark plate of (6 n + 2) x 13 pixels above or below its box.  Integers only.
#include "jpeg_label_font.h"
constexpr int MAX_LABEL = 32, CELL_W = 6, CELL_H = 11, PLATE_H = CELL_H + 2, PLATE_RGB = 10;

struct Label {
  int px, py;                 // the plate's top left corner
  int n;                      // characters; 0 = the box has no label
  int at;                     // where its text starts, in bytes behind the colours
};

// Box i's label from its length byte L (L & 0x7F characters, bit 7 = below the box) and `before` = the sum of the length bytes'
// counts of the boxes in front of it; labels = the text bytes there are.  The count is clamped to MAX_LABEL and to the bytes that
// remain, so that at + n <= labels whatever the length bytes hold.
GPV_ENC_FN Label label_place(const int* rect, int L, int before, int labels, int H, int W) {
  Label l;
  l.at = before < labels ? before : labels;
  l.n = L & 0x7F;
  l.n = l.n < MAX_LABEL ? l.n : MAX_LABEL;
  l.n = l.n < labels - l.at ? l.n : labels - l.at;
  const int w = CELL_W * l.n + 2;
  int py;
  if (L & 0x80) {
    py = rect[3] + 1;
    if (py + PLATE_H > H) py = rect[3] - PLATE_H;
  } else {
    py = rect[1] - PLATE_H;
    if (py < 0) py = rect[1] + 1;
  }
  const int top = H - PLATE_H > 0 ? H - PLATE_H : 0;
  l.py = py < 0 ? 0 : py > top ? top : py;
  int px = rect[0];
  if (px + w > W) px = W - w;
  l.px = px < 0 ? 0 : px;
  return l;
}

GPV_ENC_FN bool on_plate(const Label& l, int x, int y) {
  return l.n > 0 && x >= l.px && x < l.px + CELL_W * l.n + 2 && y >= l.py && y < l.py + PLATE_H;
}

// the glyph of a text byte: 0..94; a byte outside 32..126 is drawn as '?'
GPV_ENC_FN int glyph_of(int byte) { return byte >= 32 && byte <= 126 ? byte - 32 : '?' - 32; }

// of a pixel on the plate: ink (the box's colour) or plate.  glyph[k] = the glyph index (glyph_of) of the k-th text byte behind the
// colours.  The pixel belongs to the cell of character c / 6; in its last column the NEXT character has the say where its row has
// bit 7 (jpeg_label_font.h: Pillow pastes such a glyph one pixel to the left, over what the character before has left there).
template <class G>
GPV_ENC_FN bool label_ink(const Label& l, const LabelFont& font, const G& glyph, int x, int y) {
  const int c = x - l.px - 1, r = y - l.py - 1;
  if (c < 0 || c >= CELL_W * l.n || r < 0 || r >= CELL_H) return false;
  const int k = c / CELL_W, j = c % CELL_W;
  if (j == CELL_W - 1 && k + 1 < l.n) {
    const int next = font.rows[glyph[l.at + k + 1]][r];
    if (next & 0x80) return (next >> 6) & 1;
  }
  return (font.rows[glyph[l.at + k]][r] >> j) & 1;
}

// The labels of one picture drawn into rgb[H][pitch][3] over the outlines, in box order: rects = nboxes x (x1, y1, x2, y2) of box_rect,
// colours = nboxes x 4 bytes (R, G, B, length byte) with `labels` text bytes behind them.  false: arguments outside the rule's extents.
inline bool draw_labels(uint8_t* rgb, int H, int W, int pitch, const int* rects, const uint8_t* colours, int nboxes, int labels) {
  if (!rgb || H < 1 || W < 1 || pitch < W || nboxes < 0 || nboxes > MAX_BOXES || labels < 0 || labels > nboxes * MAX_LABEL ||
      (nboxes && (!rects || !colours)))
    return false;
  static constexpr LabelFont font = make_label_font();
  const uint8_t* text = colours + 4 * nboxes;
  uint8_t glyph[MAX_BOXES * MAX_LABEL];
  for (int k = 0; k < labels; ++k) glyph[k] = (uint8_t)glyph_of(text[k]);
  int before = 0;
  for (int i = 0; i < nboxes; ++i) {
    const int L = colours[4 * i + 3];
    const Label l = label_place(rects + 4 * i, L, before, labels, H, W);
    before += L & 0x7F;
    for (int y = l.py < 0 ? 0 : l.py; y < H && y < l.py + PLATE_H; ++y)
      for (int x = l.px < 0 ? 0 : l.px; x < W && on_plate(l, x, y); ++x) {
        const bool ink = label_ink(l, font, glyph, x, y);
        uint8_t* p = rgb + ((size_t)y * pitch + x) * 3;
        for (int ch = 0; ch < 3; ++ch) p[ch] = ink ? colours[4 * i + ch] : (uint8_t)PLATE_RGB;
      }
  }
  return true;
}

// std * x, + mean, * 255, + 0.5, floor, clamp to 0..255 (a NaN gives 0); fp32, every operation on its own
GPV_ENC_FN int denormalise(float x, float mean, float std) {
  float t = std * x;
  t = mean + t;
  t = 255.f * t;
  t = t + 0.5f;
  return t >= 255.f ? 255 : t > 0.f ? (int)t : 0;
}

// everything in front of the scan into out[HEADER_BYTES]
inline void write_header(const Tables& T, const Quant& Q, int H, int W, int hs, int vs, uint8_t* out) {
  uint8_t* p = out;
  auto seg = [&](int marker, int body) { *p++ = 0xFF, *p++ = (uint8_t)marker, *p++ = (uint8_t)((body + 2) >> 8), *p++ = (uint8_t)((body + 2) & 255); };
  *p++ = 0xFF, *p++ = 0xD8;
  seg(0xE0, 14);
  const uint8_t jfif[14] = {'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  for (uint8_t v : jfif) *p++ = v;
  for (int c = 0; c < 2; ++c) {
    seg(0xDB, 65);
    *p++ = (uint8_t)c;
    for (int k = 0; k < 64; ++k) *p++ = (uint8_t)(Q.d[c][T.zigzag[k]] >> 3);
  }
  seg(0xC0, 15);
  const uint8_t sof[15] = {8, (uint8_t)(H >> 8), (uint8_t)H, (uint8_t)(W >> 8), (uint8_t)W, 3, 1, (uint8_t)((hs << 4) | vs), 0, 2, 0x11, 1, 3, 0x11, 1};
  for (uint8_t v : sof) *p++ = v;
  for (int c = 0; c < 2; ++c) {
    seg(0xC4, 29);
    *p++ = (uint8_t)c;
    for (int i = 0; i < 16; ++i) *p++ = T.dc_bits[c][i];
    for (int i = 0; i < 12; ++i) *p++ = T.dc_vals[c][i];
    seg(0xC4, 179);
    *p++ = (uint8_t)(0x10 | c);
    for (int i = 0; i < 16; ++i) *p++ = T.ac_bits[c][i];
    for (int i = 0; i < 162; ++i) *p++ = T.ac_vals[c][i];
  }
  seg(0xDA, 10);
  const uint8_t sos[10] = {3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0};
  for (uint8_t v : sos) *p++ = v;
}

// most significant bit first into bytes, 0xFF followed by 0x00
struct ByteSink {
  std::vector<uint8_t>& out;
  uint32_t acc = 0;
  int fill = 0;
  void operator()(uint32_t v, int n) {
    for (int i = n - 1; i >= 0; --i) {
      acc = (acc << 1) | ((v >> i) & 1);
      if (++fill == 8) {
        out.push_back((uint8_t)acc);
        if ((uint8_t)acc == 0xFF) out.push_back(0);
        acc = 0, fill = 0;
      }
    }
  }
};

// the whole file of rgb[H][pitch][3]; subsampling 0 / 1 / 2 = 4:4:4 / 4:2:2 / 4:2:0.  false: arguments outside the rule's extents.
inline bool encode(const uint8_t* rgb, int H, int W, int pitch, int quality, int subsampling, std::vector<uint8_t>& out) {
  if (!rgb || H < 1 || H > 65535 || W < 1 || W > 65535 || pitch < W || quality < 1 || quality > 100 || subsampling < 0 || subsampling > 2) return false;
  static constexpr Tables T = make_tables();
  const Quant Q = make_quant(T, quality);
  const int hs = subsampling ? 2 : 1, vs = subsampling == 2 ? 2 : 1;
  const Geometry g = geometry(H, W, hs, vs);
  out.assign(HEADER_BYTES, 0);
  write_header(T, Q, H, W, hs, vs, out.data());
  auto px = [&](int x, int y, int comp) {
    const uint8_t* p = rgb + ((size_t)y * pitch + x) * 3;
    return ycc(comp, p[0], p[1], p[2]);
  };
  ByteSink sink{out};
  int pred[3] = {0, 0, 0}, prev = 0;
  for (int k = 0; k < g.nblocks; ++k) {
    const Block b = block_at(g, k);
    int16_t zz[64] = {0};
    int dc = prev;                       // a dummy block repeats the DC of the block coded just before it
    if (!b.dummy) {
      int d[64];
      sample_block(px, g, b, H, W, d);
      fdct(d);
      const int c = b.comp ? 1 : 0;
      for (int i = 0; i < 64; ++i) zz[i] = (int16_t)quantise(d[T.zigzag[i]], Q.d[c][T.zigzag[i]], Q.m[c][T.zigzag[i]]);
      dc = zz[0];
    }
    code_block(T, zz, dc - pred[b.comp], b.comp ? 1 : 0, sink);
    pred[b.comp] = prev = dc;
  }
  if (sink.fill) sink((1u << (8 - sink.fill)) - 1, 8 - sink.fill);
  out.push_back(0xFF), out.push_back(0xD9);
  return true;
}

}  // namespace gpv_enc_rule
#endif
