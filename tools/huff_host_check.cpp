// Stand-alone check of the host code that reads JPEG files under the host sanitisers: the host-only half of libgpv_huff.so
// (gpv-1_amd/csrc/jpeg_huff_host.h) and the body of gpv_jpeg_parse with its serial entropy decoder (gpv-1_amd/csrc/jpeg_host.h).  No
// GPU, no Python.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/huff_host_check tools/huff_host_check.cpp
//   /tmp/huff_host_check tests/golden/jpeg/*.jpg
// Per file: gpv_huff_host::prepare on the file, on every truncation of it (a stride of 7 bytes), on copies with random bytes
// overwritten, and on random byte strings; then the subsequence iteration of the rule, run sequentially with the very walk the kernel
// compiles (S = 64, 256, 1024), on the file's stream and on random streams under the file's tables.  The fixed point must equal one
// walk over the whole stream (coefficients, states and block count) within n_sub passes.
// Every file variant also goes through gpv_jpeg_host::parse: the header pass, then the full decode into an exact-size heap buffer.
// The two entry points must agree: the same refusal, the same `info`, a missing table refused by the full decode as by prepare; and
// where prepare routes to the device and the sequential walk reports status 0, its coefficients (DC differences summed per
// component) must equal the serial decoder's.  Exit status 0 and "ok" = clean.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../gpv-1_amd/csrc/jpeg_huff_host.h"

using namespace gpv_huff_host;

static uint32_t rng_state = 12345;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

struct State { uint32_t p; int c, z, cnt; };

struct Prepared {
  gpv_jpeg_info info;
  gpv_huff_desc desc;
  std::vector<uint32_t> stream;                           // 4-byte aligned words hold the bytes
  int route, err;
};

static long serial_decodes = 0, device_compared = 0;

// gpv_jpeg_parse on the same bytes (header pass, then the full decode) against what prepare said
static void check_parse(const unsigned char* copy, int64_t n, const Prepared& p, Frame& tabs) {
  gpv_jpeg_info hi;
  const int he = parse(copy, n, &hi, nullptr, 0, tabs);
  if (he && p.err != he) { printf("header pass refuses with %d, prepare returns %d\n", he, p.err); exit(2); }
  if (!p.err && (he || memcmp(&hi, &p.info, sizeof(hi)))) { printf("prepare succeeds, the header pass differs (%d)\n", he); exit(2); }
  if (he || hi.coef_count > (1 << 22)) return;
  short* coefs = (short*)malloc(hi.coef_count ? (size_t)hi.coef_count * sizeof(short) : 1);   // exact size: a write past it is a report
  gpv_jpeg_info fi;
  const int fe = parse(copy, n, &fi, coefs, hi.coef_count, tabs);
  ++serial_decodes;
  if (memcmp(&fi, &hi, sizeof(fi))) { printf("the full decode fills another info than the header pass\n"); exit(2); }
  if (p.err && fe != p.err) { printf("prepare refuses with %d behind a good header pass, the full decode returns %d\n", p.err, fe); exit(2); }
  if (!p.err && p.route == GPV_HUFF_ROUTE_DEVICE) {
    const gpv_huff_desc& d = p.desc;
    std::vector<short> w((size_t)d.coef_count, 0);
    State s{0, 0, 0, 0};
    int status = 0;
    walk<true>(d, p.stream.data(), d.stream_cap / 4, s.p, s.c, s.z, (uint32_t)d.nbits, d.nbits + 1, s.cnt, w.data(), 0, status);
    if (s.cnt < d.nblocks) status |= GPV_HUFF_ERR_SHORT;                 // (as the kernel does: the serial decoder reads zero bits on)
    if (status == 0) {
      int run[3] = {0, 0, 0};
      for (int blk = 0; blk < d.nblocks; ++blk) {                        // DC differences -> values, per component in scan order
        const int c = d.blk_comp[blk % d.blocks_per_mcu];
        short& dc = w[(size_t)block_address(d, d.blocks_per_mcu, blk)];
        run[c] += dc;
        dc = (short)run[c];
      }
      if (fe || memcmp(w.data(), coefs, w.size() * sizeof(short))) { printf("the walk and the serial decoder differ (%d)\n", fe); exit(2); }
      ++device_compared;
    }
  }
  free(coefs);
}

static Prepared prep(const std::vector<unsigned char>& f, Frame& tabs) {
  Prepared p;
  int64_t cap = 0;
  // an exact-size heap copy: a read past the file is a sanitiser report
  unsigned char* copy = (unsigned char*)malloc(f.size() ? f.size() : 1);
  if (!f.empty()) memcpy(copy, f.data(), f.size());
  p.err = prepare(copy, (int64_t)f.size(), &p.info, &p.desc, nullptr, 0, &cap, &p.route, tabs);
  if (!p.err) {
    p.stream.assign((size_t)cap / 4, 0xdeadbeefu);
    gpv_jpeg_info i2;
    gpv_huff_desc d2;
    int64_t cap2 = 0;
    int r2 = 0;
    const int e2 = prepare(copy, (int64_t)f.size(), &i2, &d2, (unsigned char*)p.stream.data(), cap, &cap2, &r2, tabs);
    if (e2 || cap2 != cap || r2 != p.route || memcmp(&i2, &p.info, sizeof(i2)) || memcmp(&d2, &p.desc, sizeof(d2))) { printf("prepare: second call differs\n"); exit(2); }
    if (prepare(copy, (int64_t)f.size(), &i2, &d2, (unsigned char*)p.stream.data(), cap - 1, &cap2, &r2, tabs) != kInvalid) { printf("prepare: short buffer accepted\n"); exit(2); }
  }
  check_parse(copy, (int64_t)f.size(), p, tabs);
  free(copy);
  return p;
}

// the iteration of the rule, sequentially; returns the passes, fills coefs (DC as differences) and the status bits
static int iterate(const gpv_huff_desc& d, const uint32_t* words, int S, std::vector<short>& coefs, int& status, int& blocks) {
  const uint32_t nbits = (uint32_t)d.nbits;
  const int nwords = d.stream_cap / 4;
  int n_sub = (int)((nbits + S - 1) / S);
  if (n_sub < 1) n_sub = 1;
  std::vector<State> st(n_sub), nx(n_sub);
  std::vector<char> chg(n_sub, 1), nchg(n_sub);
  int passes = 0, dummy = 0;
  for (int k = 0; k < n_sub; ++k) {
    bool any = false;
    for (int i = 0; i < n_sub; ++i) {
      const uint32_t limit = (uint32_t)(i + 1) * S < nbits ? (uint32_t)(i + 1) * S : nbits;
      nx[i] = st[i]; nchg[i] = 0;
      if (k == 0 || (i > 0 && chg[i - 1])) {
        State s = k == 0 ? State{(uint32_t)i * S < nbits ? (uint32_t)i * S : nbits, 0, 0, 0} : State{st[i - 1].p, st[i - 1].c, st[i - 1].z, 0};
        walk<false>(d, words, nwords, s.p, s.c, s.z, limit, S, s.cnt, nullptr, 0, dummy);
        nchg[i] = k == 0 || s.p != st[i].p || s.c != st[i].c || s.z != st[i].z;
        nx[i] = s;
      }
      if (nchg[i] && i < n_sub - 1) any = true;
    }
    st.swap(nx); chg.swap(nchg);
    ++passes;
    if (!any) break;
  }
  coefs.assign((size_t)d.coef_count, 0);
  status = 0; blocks = 0;
  for (int i = 0; i < n_sub; ++i) {
    const uint32_t limit = (uint32_t)(i + 1) * S < nbits ? (uint32_t)(i + 1) * S : nbits;
    State s = i ? State{st[i - 1].p, st[i - 1].c, st[i - 1].z, 0} : State{0, 0, 0, 0};
    walk<true>(d, words, nwords, s.p, s.c, s.z, limit, S, s.cnt, coefs.data(), blocks, status);
    if (s.p != st[i].p || s.c != st[i].c || s.z != st[i].z || s.cnt != st[i].cnt) { printf("write pass left the fixed point\n"); exit(2); }
    blocks += s.cnt;
  }
  if (passes > n_sub) { printf("more passes than subsequences\n"); exit(2); }
  return passes;
}

static void check_stream(const gpv_huff_desc& d, const uint32_t* words, const char* what) {
  // the sequential decode: one walk over the whole stream (a symbol takes at least one bit: nbits symbols at most)
  std::vector<short> ref((size_t)d.coef_count, 0), got;
  State s{0, 0, 0, 0};
  int rstatus = 0;
  walk<true>(d, words, d.stream_cap / 4, s.p, s.c, s.z, (uint32_t)d.nbits, d.nbits + 1, s.cnt, ref.data(), 0, rstatus);
  for (int S : {64, 256, 1024}) {
    int status = 0, blocks = 0;
    iterate(d, words, S, got, status, blocks);
    if (got != ref || status != rstatus || blocks != s.cnt) { printf("%s: S = %d differs from the sequential decode\n", what, S); exit(2); }
  }
}

int main(int argc, char** argv) {
  static Frame tabs;
  long whole_compared = 0, prepared = 0, refused = 0, streams = 0;
  for (int a = 1; a < argc; ++a) {
    FILE* fp = fopen(argv[a], "rb");
    if (!fp) { printf("cannot open %s\n", argv[a]); return 2; }
    std::vector<unsigned char> f;
    for (int ch; (ch = fgetc(fp)) != EOF;) f.push_back((unsigned char)ch);
    fclose(fp);
    const long before = device_compared;
    Prepared whole = prep(f, tabs);
    if (whole.err) { printf("%s: prepare returned %d\n", argv[a], whole.err); return 2; }
    if (whole.route == GPV_HUFF_ROUTE_DEVICE && device_compared == before) { printf("%s: the walk reports an error on the whole file\n", argv[a]); return 2; }
    whole_compared += device_compared - before;
    check_stream(whole.desc, whole.stream.data(), argv[a]);
    ++streams;
    for (size_t cut = 0; cut < f.size(); cut += 7) {                     // truncated copies
      Prepared p = prep(std::vector<unsigned char>(f.begin(), f.begin() + cut), tabs);
      if (p.err) { ++refused; continue; }
      ++prepared;
      if (p.route != GPV_HUFF_ROUTE_HOST) { printf("%s cut at %zu: routed to the device\n", argv[a], cut); return 2; }
      if (p.desc.coef_count <= (1 << 22)) check_stream(p.desc, p.stream.data(), "truncated");
    }
    for (int t = 0; t < 200; ++t) {                                       // copies with random bytes overwritten
      std::vector<unsigned char> g = f;
      for (int k = 0; k < 1 + (int)(rnd() % 8); ++k) g[rnd() % g.size()] = (unsigned char)rnd();
      Prepared p = prep(g, tabs);
      if (p.err) { ++refused; continue; }
      ++prepared;
      if (p.desc.nbits <= (1 << 20) && p.desc.coef_count <= (1 << 22)) { check_stream(p.desc, p.stream.data(), "mutated"); ++streams; }
    }
    for (int t = 0; t < 50; ++t) {                                        // random streams under this file's tables and geometry
      gpv_huff_desc d = whole.desc;
      const int n = (int)(rnd() % 600);
      std::vector<uint32_t> w((size_t)((n + 15) / 16 * 16 + 16) / 4, 0);
      for (int i = 0; i < n; ++i) ((unsigned char*)w.data())[i] = (unsigned char)rnd();
      d.nbits = 8 * n; d.stream_cap = (int)w.size() * 4;
      check_stream(d, w.data(), "random stream");
      ++streams;
    }
  }
  for (int t = 0; t < 2000; ++t) {                                        // random byte strings as files
    std::vector<unsigned char> g(rnd() % 400);
    for (auto& b : g) b = (unsigned char)rnd();
    if (t % 2 && g.size() >= 2) { g[0] = 0xFF; g[1] = 0xD8; }
    Prepared p = prep(g, tabs);
    p.err ? ++refused : ++prepared;
  }
  printf("ok: %d files, %ld variants prepared, %ld refused, %ld streams iterated at S = 64, 256, 1024, %ld serial decodes, %ld device-routed "
         "variants equal to the serial decoder (%ld of them whole files)\n", argc - 1, prepared, refused, streams, serial_decodes, device_compared, whole_compared);
  return 0;
}
