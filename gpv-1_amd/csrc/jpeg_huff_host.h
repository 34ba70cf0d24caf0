// The host-only half of libgpv_huff.so and the symbol walk both halves share (include/gpv_huff.h states the rule).  Plain C++: no HIP
// header, no HIP call -- a host compiler can include this file on its own (tools/huff_host_check.cpp does, under the sanitisers).
//   gpv_huff_host::prepare   markers, tables, un-stuffing, route: what gpv_huff_prepare exports
//   gpv_huff_host::walk      the symbols of one subsequence; jpeg_huff.hip runs it per thread, the check program sequentially
// The marker loop repeats jpeg.hip's (gpv_jpeg_parse) check for check, so that `info` and the refusals are the same.
#ifndef GPV_JPEG_HUFF_HOST_H
#define GPV_JPEG_HUFF_HOST_H
#include <stdint.h>
#include <string.h>
#include "../../include/gpv_huff.h"

#if defined(__HIPCC__)
#define GPV_HUFF_HD __host__ __device__ __forceinline__
#else
#define GPV_HUFF_HD inline
#endif

namespace gpv_huff_host {

constexpr int kInvalid = 1, kUnsupported = 801;        // hipErrorInvalidValue, hipErrorNotSupported
constexpr int LOOK = GPV_HUFF_LOOK;

GPV_HUFF_HD int zigzag(int k) {
  constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return kZigzag[k & 63];
}

inline bool build_table(const unsigned char* counts, const unsigned char* syms, int nsyms, gpv_huff_table& t) {
  memset(&t, 0, sizeof(t));
  memcpy(t.syms, syms, (size_t)nsyms);
  int code = 0, k = 0;
  for (int l = 1; l <= 16; ++l) {
    t.valoffset[l] = k - code;
    if (counts[l - 1]) {
      if (code + counts[l - 1] > (1 << l)) return false;
      for (int i = 0; i < counts[l - 1]; ++i, ++k, ++code) {
        if (l <= LOOK) {
          const int first = code << (LOOK - l);
          for (int f = 0; f < (1 << (LOOK - l)); ++f) { t.look_nbits[first + f] = (unsigned char)l; t.look_sym[first + f] = syms[k]; }
        }
      }
      t.maxcode[l] = code - 1;
    } else {
      t.maxcode[l] = -1;
    }
    code <<= 1;
  }
  t.maxcode[17] = 0x7fffffff;
  return k == nsyms;
}

inline int rd16(const unsigned char* q) { return (q[0] << 8) | q[1]; }

struct Tables {                                          // too large for a stack frame of a pool thread's caller to carry twice
  gpv_huff_table dc[4], ac[4];
  bool dc_ok[4], ac_ok[4];
};

// see gpv_huff_prepare (include/gpv_huff.h); `tabs` is scratch of the caller
inline int prepare(const unsigned char* data, int64_t nbytes, gpv_jpeg_info* info, gpv_huff_desc* desc, unsigned char* out,
                   int64_t out_capacity, int64_t* stream_cap, int* route, Tables& tabs) {
  if (!data || !info || !desc || !stream_cap || !route || nbytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return kInvalid;
  const unsigned char* end = data + nbytes;
  const unsigned char* p = data + 2;
  for (int i = 0; i < 4; ++i) tabs.dc_ok[i] = tabs.ac_ok[i] = false;
  unsigned short qt[4][64];
  bool qt_ok[4] = {false, false, false, false};
  int comp_id[3] = {0, 0, 0}, comp_h[3] = {1, 1, 1}, comp_v[3] = {1, 1, 1}, comp_tq[3] = {0, 0, 0}, comp_td[3] = {0, 0, 0}, comp_ta[3] = {0, 0, 0};
  int W = 0, H = 0, nf = 0, ri = 0;
  bool have_frame = false, adobe_rgb = false;
  for (;;) {
    while (p < end && *p != 0xFF) ++p;
    while (p < end && *p == 0xFF) ++p;
    if (p >= end) return kInvalid;
    const int m = *p++;
    if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;
    if (m == 0xD9) return kInvalid;
    if (end - p < 2) return kInvalid;
    const int ln = rd16(p);
    if (ln < 2 || end - p < ln) return kInvalid;
    const unsigned char* seg = p + 2;
    const int sl = ln - 2;
    if (m == 0xDB) {
      int q = 0;
      while (q < sl) {
        const int pq = seg[q] >> 4, tq = seg[q] & 15;
        if (pq) return kUnsupported;
        if (tq > 3 || q + 65 > sl) return kInvalid;
        for (int i = 0; i < 64; ++i) qt[tq][zigzag(i)] = seg[q + 1 + i];
        qt_ok[tq] = true;
        q += 65;
      }
    } else if (m == 0xC4) {
      int q = 0;
      while (q < sl) {
        if (q + 17 > sl) return kInvalid;
        const int tc = seg[q] >> 4, th = seg[q] & 15;
        int ns = 0;
        for (int i = 0; i < 16; ++i) ns += seg[q + 1 + i];
        if (tc > 1 || th > 3 || ns > 256 || q + 17 + ns > sl) return kInvalid;
        if (!build_table(seg + q + 1, seg + q + 17, ns, tc ? tabs.ac[th] : tabs.dc[th])) return kInvalid;
        (tc ? tabs.ac_ok : tabs.dc_ok)[th] = true;
        q += 17 + ns;
      }
    } else if (m == 0xC0 || m == 0xC1) {
      if (sl < 6) return kInvalid;
      if (seg[0] != 8) return kUnsupported;
      H = rd16(seg + 1); W = rd16(seg + 3); nf = seg[5];
      if (nf != 1 && nf != 3) return kUnsupported;
      if (sl < 6 + 3 * nf || W <= 0 || H <= 0) return kInvalid;
      for (int i = 0; i < nf; ++i) {
        comp_id[i] = seg[6 + 3 * i]; comp_h[i] = seg[7 + 3 * i] >> 4; comp_v[i] = seg[7 + 3 * i] & 15; comp_tq[i] = seg[8 + 3 * i];
        if (comp_tq[i] > 3) return kInvalid;
      }
      have_frame = true;
    } else if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) {
      return kUnsupported;
    } else if (m == 0xEE) {
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0 && seg[11] == 0) adobe_rgb = true;
    } else if (m == 0xDD) {
      if (sl < 2) return kInvalid;
      ri = rd16(seg);
    } else if (m == 0xDA) {
      if (!have_frame || sl < 1) return kInvalid;
      const int ns = seg[0];
      if (ns != nf) return kUnsupported;
      if (sl < 1 + 2 * ns + 3) return kInvalid;
      for (int i = 0; i < ns; ++i) {
        if (seg[1 + 2 * i] != comp_id[i]) return kUnsupported;
        comp_td[i] = seg[2 + 2 * i] >> 4; comp_ta[i] = seg[2 + 2 * i] & 15;
        if (comp_td[i] > 3 || comp_ta[i] > 3) return kInvalid;
      }
      p += ln;
      break;
    }
    p += ln;
  }
  if (nf == 3 && adobe_rgb) return kUnsupported;
  if (nf == 3) {
    const bool luma_ok = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2);
    if (!luma_ok || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return kUnsupported;
  } else {
    comp_h[0] = comp_v[0] = 1;
  }
  const int hmax = comp_h[0], vmax = comp_v[0];
  const int mx = (W + 8 * hmax - 1) / (8 * hmax), my = (H + 8 * vmax - 1) / (8 * vmax);
  memset(info, 0, sizeof(*info));
  memset(desc, 0, sizeof(*desc));
  info->width = W; info->height = H; info->ncomp = nf; info->hmax = hmax; info->vmax = vmax; info->mcus_x = mx; info->mcus_y = my;
  int64_t off = 0;
  for (int i = 0; i < nf; ++i) {
    if (!qt_ok[comp_tq[i]]) return kInvalid;
    info->bh[i] = my * comp_v[i]; info->bw[i] = mx * comp_h[i];
    info->coef_offset[i] = off;
    off += (int64_t)info->bh[i] * info->bw[i] * 64;
    for (int k = 0; k < 64; ++k) info->quant[i][k] = qt[comp_tq[i]][k];
  }
  info->coef_count = off;
  for (int i = 0; i < nf; ++i)
    if (!tabs.dc_ok[comp_td[i]] || !tabs.ac_ok[comp_ta[i]]) return kInvalid;
  // the entropy segment: up to the first FF that is not followed by 00
  const unsigned char* q = p;
  int64_t n = 0;
  int marker = -1;
  while (q < end) {
    const unsigned char* f = static_cast<const unsigned char*>(memchr(q, 0xFF, (size_t)(end - q)));
    if (!f) { n += end - q; q = end; break; }
    n += f - q;
    q = f;
    if (end - q >= 2 && q[1] == 0) { q += 2; ++n; continue; }
    marker = end - q >= 2 ? q[1] : -1;
    break;
  }
  const unsigned char* seg_end = q;
  const int64_t cap = (n + 15) / 16 * 16 + 16;
  *stream_cap = cap;
  *route = (ri == 0 && marker == 0xD9 && n <= GPV_HUFF_MAX_STREAM) ? GPV_HUFF_ROUTE_DEVICE : GPV_HUFF_ROUTE_HOST;
  desc->coef_count = off;
  desc->nbits = n <= GPV_HUFF_MAX_STREAM ? (int)(8 * n) : 0;
  desc->stream_cap = n <= GPV_HUFF_MAX_STREAM ? (int)cap : 0;
  desc->ncomp = nf; desc->mcus_x = mx; desc->mcus_y = my;
  int j = 0;
  for (int i = 0; i < nf; ++i) {
    desc->coef_offset[i] = info->coef_offset[i];
    desc->bh[i] = info->bh[i]; desc->bw[i] = info->bw[i];
    desc->comp_h[i] = comp_h[i]; desc->comp_v[i] = comp_v[i];
    desc->dc[i] = tabs.dc[comp_td[i]];
    desc->ac[i] = tabs.ac[comp_ta[i]];
    for (int v = 0; v < comp_v[i]; ++v)
      for (int h = 0; h < comp_h[i]; ++h, ++j) { desc->blk_comp[j] = (unsigned char)i; desc->blk_v[j] = (unsigned char)v; desc->blk_h[j] = (unsigned char)h; }
  }
  desc->blocks_per_mcu = j;
  desc->nblocks = (int)((int64_t)mx * my * j);
  if (!out) return 0;
  if (out_capacity < cap) return kInvalid;
  unsigned char* o = out;
  for (q = p; q < seg_end;) {
    const unsigned char* f = static_cast<const unsigned char*>(memchr(q, 0xFF, (size_t)(seg_end - q)));
    const size_t run = (size_t)((f ? f + 1 : seg_end) - q);     // up to and with the FF; its stuffed 00 is skipped
    memcpy(o, q, run);
    o += run;
    q += run + (f ? 1 : 0);
  }
  memset(o, 0, (size_t)(cap - n));
  return 0;
}

// ---- the walk ---------------------------------------------------------------------------------------------------------------
// The stream is read through a window of three 32-bit words (MSB first): w0 | w1 hold the 32 bits at p, w2 is loaded one word ahead
// so that no symbol waits for memory.  Words beyond the padded stream are zero, every load goes to a clamped index.
struct Window {
  uint32_t w0, w1, w2;
  int wi;                                                // w0 is word wi of the stream
};

GPV_HUFF_HD uint32_t load_word(const uint32_t* words, int nwords, int i) {
  const uint32_t v = __builtin_bswap32(words[i < 0 ? 0 : (i < nwords ? i : nwords - 1)]);
  return i >= 0 && i < nwords ? v : 0u;
}

GPV_HUFF_HD Window open_window(const uint32_t* words, int nwords, uint32_t p) {
  Window b;
  b.wi = (int)(p >> 5);
  b.w0 = load_word(words, nwords, b.wi); b.w1 = load_word(words, nwords, b.wi + 1); b.w2 = load_word(words, nwords, b.wi + 2);
  return b;
}

GPV_HUFF_HD uint32_t peek32(const Window& b, uint32_t p) {
  return (uint32_t)((((uint64_t)b.w0 << 32) | b.w1) >> (32 - (p & 31)));
}

// p moved on by one symbol (at most 31 bits): at most one word
GPV_HUFF_HD void advance(Window& b, const uint32_t* words, int nwords, uint32_t p) {
  if ((int)(p >> 5) != b.wi) {
    b.w0 = b.w1; b.w1 = b.w2; ++b.wi;
    b.w2 = load_word(words, nwords, b.wi + 2);
  }
}

GPV_HUFF_HD int extend(uint32_t w, int nb, int s) {     // the s extra bits behind an nb-bit code, 1 <= s <= 15: T.81 F.2.2.1 EXTEND
  const int r = (int)((w >> (32 - nb - s)) & ((1u << s) - 1));
  return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
}

// element offset of block `blk` (scan order) in the coefficient layout of gpv_jpeg_parse, clamped into the array
GPV_HUFF_HD int64_t block_address(const gpv_huff_desc& d, int bpm, int blk) {
  const int mcu = blk / bpm, j = blk - mcu * bpm;
  const int mx = d.mcus_x > 0 ? d.mcus_x : 1;
  const int y0 = mcu / mx, x0 = mcu - y0 * mx;
  const int c = d.blk_comp[j & 7] < 3 ? d.blk_comp[j & 7] : 2;
  int64_t a = d.coef_offset[c] + ((int64_t)(y0 * d.comp_v[c] + d.blk_v[j & 7]) * d.bw[c] + x0 * d.comp_h[c] + d.blk_h[j & 7]) * 64;
  const int64_t last = d.coef_count - 64;
  a = a > last ? last : a;
  return a < 0 ? 0 : a;
}

// Symbols while p < limit, at most S of them (every symbol takes at least one bit and a walk starts at or after its subsequence).
// (p, c, z) in / out; cnt += blocks finished.  WRITE: the AC values and DC differences of blocks < d.nblocks go to coefs, blk = the
// scan index of the block under way; err |= GPV_HUFF_ERR_CODE for a convention met inside such a block.
template <bool WRITE>
GPV_HUFF_HD void walk(const gpv_huff_desc& d, const uint32_t* words, int nwords, uint32_t& p, int& c, int& z, uint32_t limit, int S,
                      int& cnt, short* coefs, int blk, int& err) {
  const int bpm = d.blocks_per_mcu < 1 ? 1 : (d.blocks_per_mcu > 6 ? 6 : d.blocks_per_mcu);
  c = c < 0 ? 0 : (c >= bpm ? bpm - 1 : c);
  z = z < 0 ? 0 : (z > 63 ? 63 : z);
  int64_t base = 0;
  if (WRITE) base = block_address(d, bpm, blk);
  Window win = open_window(words, nwords, p);
  for (int it = 0; it < S && p < limit; ++it) {
    const uint32_t w = peek32(win, p);
    const int comp = d.blk_comp[c] < 3 ? d.blk_comp[c] : 2;
    const gpv_huff_table& t = z == 0 ? d.dc[comp] : d.ac[comp];
    const unsigned look = w >> (32 - LOOK);
    int nb = t.look_nbits[look], sym = t.look_sym[look], e = 0;
    if (nb == 0) {
      nb = 16; sym = 0; e = GPV_HUFF_ERR_CODE;
#pragma unroll
      for (int l = 16; l > LOOK; --l) {                  // the shortest length whose largest code is not below these bits
        const int code = (int)(w >> (32 - l));
        if (code <= t.maxcode[l]) { nb = l; sym = t.syms[(code + t.valoffset[l]) & 255]; e = 0; }
      }
    }
    if (z == 0) {
      int s = sym;
      if (s > 15) { s = 15; e = GPV_HUFF_ERR_CODE; }
      const int v = s ? extend(w, nb, s) : 0;
      p += (uint32_t)(nb + s);
      if (WRITE && blk < d.nblocks) coefs[base] = (short)v;
      z = 1;
    } else {
      const int r = sym >> 4, s = sym & 15;
      p += (uint32_t)(nb + s);
      if (s == 0) {
        z = r == 15 ? z + 16 : 64;
      } else {
        z += r;
        if (z > 63) {
          z = 64; e = GPV_HUFF_ERR_CODE;
        } else {
          if (WRITE && blk < d.nblocks) coefs[base + zigzag(z)] = (short)extend(w, nb, s);
          ++z;
        }
      }
    }
    advance(win, words, nwords, p);
    if (WRITE && blk < d.nblocks) err |= e;
    if (z >= 64) {
      z = 0; c = c + 1 < bpm ? c + 1 : 0; ++cnt; ++blk;
      if (WRITE) base = block_address(d, bpm, blk);
    }
  }
}

}  // namespace gpv_huff_host
#endif
