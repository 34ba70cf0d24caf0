// The host's reading of a baseline JPEG file, once, for both host entry points: gpv_jpeg_parse (libgpv_hip.so, jpeg.hip) and
// gpv_huff_prepare (libgpv_huff.so, jpeg_huff_host.h).  Plain C++: no HIP header, no HIP call -- a host compiler can include this
// file on its own (tools/huff_host_check.cpp does, under the sanitisers).
//   parse_headers   the marker loop up to and with SOS, the Adobe RGB and sampling refusals -> Frame
//   fill_info       geometry, coefficient layout and quantisation tables of a Frame -> gpv_jpeg_info
//   decode_scan     the serial walk over the entropy segment (restart intervals included) -> coefficients
//   parse           the three in the order of gpv_jpeg_parse, which is this function plus its scratch
// Whether the Huffman tables a scan names were defined is asked by the callers (tables_present), never by parse_headers: the header
// pass of gpv_jpeg_parse does not ask, gpv_huff_prepare always does.
#ifndef GPV_JPEG_HOST_H
#define GPV_JPEG_HOST_H
#include <stdint.h>
#include <string.h>
#include "../../include/gpv_huff.h"

#if defined(__HIPCC__)
#define GPV_HUFF_HD __host__ __device__ __forceinline__
#else
#define GPV_HUFF_HD inline
#endif

namespace gpv_jpeg_host {

constexpr int kInvalid = 1, kUnsupported = 801;        // hipErrorInvalidValue, hipErrorNotSupported
constexpr int LOOK = GPV_HUFF_LOOK;

GPV_HUFF_HD int zigzag(int k) {
  constexpr unsigned char kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
  return kZigzag[k & 63];
}

inline int rd16(const unsigned char* q) { return (q[0] << 8) | q[1]; }

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

struct Frame {                                           // 12 KB: scratch of the caller, one `static thread_local` per entry point
  int W, H, nf, ri;                                      // frame size, components (1 or 3), restart interval
  int comp_h[3], comp_v[3], comp_tq[3], comp_td[3], comp_ta[3];
  unsigned short qt[4][64];                              // natural order
  bool qt_ok[4], dc_ok[4], ac_ok[4];
  gpv_huff_table dc[4], ac[4];
  const unsigned char* scan;                             // the first byte behind the SOS segment
  const unsigned char* end;                              // data + nbytes
};

// 0, kInvalid (malformed) or kUnsupported (outside the decoder's scope: see jpeg.hip)
inline int parse_headers(const unsigned char* data, int64_t nbytes, Frame& f) {
  if (!data || nbytes < 4 || data[0] != 0xFF || data[1] != 0xD8) return kInvalid;
  const unsigned char* end = data + nbytes;
  const unsigned char* p = data + 2;
  f.W = f.H = f.nf = f.ri = 0;
  for (int i = 0; i < 4; ++i) f.qt_ok[i] = f.dc_ok[i] = f.ac_ok[i] = false;
  for (int i = 0; i < 3; ++i) { f.comp_h[i] = f.comp_v[i] = 1; f.comp_tq[i] = f.comp_td[i] = f.comp_ta[i] = 0; }
  int comp_id[3] = {0, 0, 0};
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
        for (int i = 0; i < 64; ++i) f.qt[tq][zigzag(i)] = seg[q + 1 + i];
        f.qt_ok[tq] = true;
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
        if (!build_table(seg + q + 1, seg + q + 17, ns, tc ? f.ac[th] : f.dc[th])) return kInvalid;
        (tc ? f.ac_ok : f.dc_ok)[th] = true;
        q += 17 + ns;
      }
    } else if (m == 0xC0 || m == 0xC1) {
      if (sl < 6) return kInvalid;
      if (seg[0] != 8) return kUnsupported;
      f.H = rd16(seg + 1); f.W = rd16(seg + 3); f.nf = seg[5];
      if (f.nf != 1 && f.nf != 3) return kUnsupported;
      if (sl < 6 + 3 * f.nf || f.W <= 0 || f.H <= 0) return kInvalid;
      for (int i = 0; i < f.nf; ++i) {
        comp_id[i] = seg[6 + 3 * i]; f.comp_h[i] = seg[7 + 3 * i] >> 4; f.comp_v[i] = seg[7 + 3 * i] & 15; f.comp_tq[i] = seg[8 + 3 * i];
        if (f.comp_tq[i] > 3) return kInvalid;
      }
      have_frame = true;
    } else if (m == 0xC2 || m == 0xC3 || (m >= 0xC5 && m <= 0xC7) || (m >= 0xC9 && m <= 0xCB) || (m >= 0xCD && m <= 0xCF)) {
      return kUnsupported;                               // progressive / lossless / arithmetic coding
    } else if (m == 0xEE) {
      // Adobe APP14: transform 0 = the components are RGB (3) / CMYK (4), not YCbCr -- libjpeg then skips the colour conversion
      if (sl >= 12 && memcmp(seg, "Adobe", 5) == 0 && seg[11] == 0) adobe_rgb = true;
    } else if (m == 0xDD) {
      if (sl < 2) return kInvalid;
      f.ri = rd16(seg);
    } else if (m == 0xDA) {
      if (!have_frame || sl < 1) return kInvalid;
      const int ns = seg[0];
      if (ns != f.nf) return kUnsupported;               // non-interleaved scans
      if (sl < 1 + 2 * ns + 3) return kInvalid;
      for (int i = 0; i < ns; ++i) {
        if (seg[1 + 2 * i] != comp_id[i]) return kUnsupported;
        f.comp_td[i] = seg[2 + 2 * i] >> 4; f.comp_ta[i] = seg[2 + 2 * i] & 15;
        if (f.comp_td[i] > 3 || f.comp_ta[i] > 3) return kInvalid;
      }
      p += ln;
      break;
    }
    p += ln;
  }
  if (f.nf == 3 && adobe_rgb) return kUnsupported;       // RGB-coded file (no YCbCr transform)
  if (f.nf == 3) {
    const bool luma_ok = (f.comp_h[0] == 1 && f.comp_v[0] == 1) || (f.comp_h[0] == 2 && f.comp_v[0] == 1) || (f.comp_h[0] == 2 && f.comp_v[0] == 2);
    if (!luma_ok || f.comp_h[1] != 1 || f.comp_v[1] != 1 || f.comp_h[2] != 1 || f.comp_v[2] != 1) return kUnsupported;
  } else {
    f.comp_h[0] = f.comp_v[0] = 1;                       // a single-component scan is never interleaved (T.81 A.2.2)
  }
  f.scan = p;
  f.end = end;
  return 0;
}

// zeroes `info` and fills it; kInvalid if a component names a quantisation table that no DQT defined
inline int fill_info(const Frame& f, gpv_jpeg_info* info) {
  const int hmax = f.comp_h[0], vmax = f.comp_v[0];
  const int mx = (f.W + 8 * hmax - 1) / (8 * hmax), my = (f.H + 8 * vmax - 1) / (8 * vmax);
  memset(info, 0, sizeof(*info));
  info->width = f.W; info->height = f.H; info->ncomp = f.nf; info->hmax = hmax; info->vmax = vmax; info->mcus_x = mx; info->mcus_y = my;
  int64_t off = 0;
  for (int i = 0; i < f.nf; ++i) {
    if (!f.qt_ok[f.comp_tq[i]]) return kInvalid;
    info->bh[i] = my * f.comp_v[i]; info->bw[i] = mx * f.comp_h[i];
    info->coef_offset[i] = off;
    off += (int64_t)info->bh[i] * info->bw[i] * 64;
    for (int k = 0; k < 64; ++k) info->quant[i][k] = f.qt[f.comp_tq[i]][k];
  }
  info->coef_count = off;
  return 0;
}

// every Huffman table the scan names was defined by a DHT
inline bool tables_present(const Frame& f) {
  for (int i = 0; i < f.nf; ++i)
    if (!f.dc_ok[f.comp_td[i]] || !f.ac_ok[f.comp_ta[i]]) return false;
  return true;
}

struct BitReader {
  const unsigned char* p; const unsigned char* end;
  uint64_t acc; int n; bool marker;
  inline void fill() {
    while (n <= 56) {
      unsigned b = 0;
      if (!marker && p < end) {
        b = *p;
        if (b == 0xFF) {
          if (p + 1 < end && p[1] == 0) { p += 2; }
          else { marker = true; b = 0; }               // a marker: the stream continues with zero bits (T.81 F.2.2.5)
        } else {
          ++p;
        }
      }
      acc = (acc << 8) | b;
      n += 8;
    }
  }
  inline int decode(const gpv_huff_table& t) {
    if (n < 16) fill();
    const unsigned look = (unsigned)(acc >> (n - LOOK)) & ((1u << LOOK) - 1);
    const int nb = t.look_nbits[look];
    if (nb) { n -= nb; return t.look_sym[look]; }
    int l = LOOK + 1;
    int code = (int)((acc >> (n - l)) & ((1u << l) - 1));
    while (code > t.maxcode[l]) {                       // (never shifts by n - 17: a code longer than 16 bits does not exist)
      if (++l > 16) return -1;
      code = (int)((acc >> (n - l)) & ((1u << l) - 1));
    }
    n -= l;
    return t.syms[(code + t.valoffset[l]) & 255];
  }
  inline int receive_extend(int s) {
    if (n < s) fill();
    const int r = (int)((acc >> (n - s)) & ((1u << s) - 1));
    n -= s;
    return r < (1 << (s - 1)) ? r - (1 << s) + 1 : r;
  }
  bool restart() {
    acc = 0; n = 0; marker = false;
    while (p + 1 < end && !(p[0] == 0xFF && p[1] >= 0xD0 && p[1] <= 0xD7)) ++p;
    if (p + 1 >= end) return false;
    p += 2;
    return true;
  }
};

// The serial walk: coefs = info.coef_count zeroed int16 in the layout of `info`; the tables of the scan must be present.
inline int decode_scan(const Frame& f, const gpv_jpeg_info& info, short* coefs) {
  BitReader br{f.scan, f.end, 0, 0, false};
  int pred[3] = {0, 0, 0};
  const int mx = info.mcus_x, nmcu = mx * info.mcus_y;
  for (int mcu = 0; mcu < nmcu; ++mcu) {
    if (f.ri && mcu && mcu % f.ri == 0) {
      if (!br.restart()) return kInvalid;
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int y0 = mcu / mx, x0 = mcu - y0 * mx;
    for (int ci = 0; ci < f.nf; ++ci) {
      const gpv_huff_table& td = f.dc[f.comp_td[ci]];
      const gpv_huff_table& ta = f.ac[f.comp_ta[ci]];
      for (int v = 0; v < f.comp_v[ci]; ++v)
        for (int h = 0; h < f.comp_h[ci]; ++h) {
          short* blk = coefs + info.coef_offset[ci] + ((int64_t)(y0 * f.comp_v[ci] + v) * info.bw[ci] + x0 * f.comp_h[ci] + h) * 64;
          const int t = br.decode(td);
          if (t < 0 || t > 15) return kInvalid;
          if (t) pred[ci] += br.receive_extend(t);
          blk[0] = (short)pred[ci];
          int k = 1;
          while (k < 64) {
            const int rs = br.decode(ta);
            if (rs < 0) return kInvalid;
            const int r = rs >> 4, s = rs & 15;
            if (s == 0) {
              if (r != 15) break;
              k += 16;
              continue;
            }
            k += r;
            if (k > 63) return kInvalid;
            blk[zigzag(k)] = (short)br.receive_extend(s);
            ++k;
          }
        }
    }
  }
  return 0;
}

// see gpv_jpeg_parse (include/gpv_hip.h); `f` is scratch of the caller
inline int parse(const unsigned char* data, int64_t nbytes, gpv_jpeg_info* info, short* coefs, int64_t coefs_capacity, Frame& f) {
  if (!info) return kInvalid;
  if (const int e = parse_headers(data, nbytes, f)) return e;
  if (const int e = fill_info(f, info)) return e;
  if (!coefs) return 0;                                  // header pass: the caller sizes its buffers
  if (coefs_capacity < info->coef_count || !tables_present(f)) return kInvalid;
  memset(coefs, 0, (size_t)info->coef_count * sizeof(short));
  return decode_scan(f, *info, coefs);
}

}  // namespace gpv_jpeg_host
#endif
