// The host-only half of libgpv_huff.so and the symbol walk both halves share (include/gpv_huff.h states the rule).  Plain C++: no HIP
// header, no HIP call -- a host compiler can include this file on its own (tools/huff_host_check.cpp does, under the sanitisers).
//   gpv_huff_host::prepare   un-stuffing, route, descriptor behind the shared header pass (jpeg_host.h): what gpv_huff_prepare exports
//   gpv_huff_host::walk      the symbols of one subsequence; jpeg_huff.hip runs it per thread, the check program sequentially
#ifndef GPV_JPEG_HUFF_HOST_H
#define GPV_JPEG_HUFF_HOST_H
#include "jpeg_host.h"

namespace gpv_huff_host {

using namespace gpv_jpeg_host;                           // Frame, parse_headers, fill_info, zigzag, LOOK, the error codes

// see gpv_huff_prepare (include/gpv_huff.h); `f` is scratch of the caller
inline int prepare(const unsigned char* data, int64_t nbytes, gpv_jpeg_info* info, gpv_huff_desc* desc, unsigned char* out,
                   int64_t out_capacity, int64_t* stream_cap, int* route, Frame& f) {
  if (!info || !desc || !stream_cap || !route) return kInvalid;
  if (const int e = parse_headers(data, nbytes, f)) return e;
  memset(desc, 0, sizeof(*desc));
  if (const int e = fill_info(f, info)) return e;
  if (!tables_present(f)) return kInvalid;
  const unsigned char* const p = f.scan;
  const unsigned char* const end = f.end;
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
  *route = (f.ri == 0 && marker == 0xD9 && n <= GPV_HUFF_MAX_STREAM) ? GPV_HUFF_ROUTE_DEVICE : GPV_HUFF_ROUTE_HOST;
  desc->coef_count = info->coef_count;
  desc->nbits = n <= GPV_HUFF_MAX_STREAM ? (int)(8 * n) : 0;
  desc->stream_cap = n <= GPV_HUFF_MAX_STREAM ? (int)cap : 0;
  desc->ncomp = f.nf; desc->mcus_x = info->mcus_x; desc->mcus_y = info->mcus_y;
  int j = 0;
  for (int i = 0; i < f.nf; ++i) {
    desc->coef_offset[i] = info->coef_offset[i];
    desc->bh[i] = info->bh[i]; desc->bw[i] = info->bw[i];
    desc->comp_h[i] = f.comp_h[i]; desc->comp_v[i] = f.comp_v[i];
    desc->dc[i] = f.dc[f.comp_td[i]];
    desc->ac[i] = f.ac[f.comp_ta[i]];
    for (int v = 0; v < f.comp_v[i]; ++v)
      for (int h = 0; h < f.comp_h[i]; ++h, ++j) { desc->blk_comp[j] = (unsigned char)i; desc->blk_v[j] = (unsigned char)v; desc->blk_h[j] = (unsigned char)h; }
  }
  desc->blocks_per_mcu = j;
  desc->nblocks = (int)((int64_t)info->mcus_x * info->mcus_y * j);
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
