// Stand-alone check of gpv-1_amd/csrc/jpeg_enc_host.h, the plain C++ statement of the JPEG encoding rule (no HIP, no Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I gpv-1_amd/csrc tools/enc_host_check.cpp -o enc_host_check
//   ./enc_host_check tests/golden/jpeg_enc
// 1. every <content>_<H>x<W>_q<quality>_s<subsampling>.rgb of the directory (raw RGB, H*W*3 bytes) encodes to the bytes of the .jpg
//    beside it, which Pillow wrote for the same pixels;
// 2. the multiply-and-shift quantiser equals the rule's division for every |c| <= MAX_ABS_COEF, either sign, and every q in 1..255;
// 3. the transform's output for the extreme blocks stays inside MAX_ABS_COEF.
// Exit status 0 only if all three hold.
#include <dirent.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <fstream>
#include <iterator>
#include <string>
#include <vector>

#include "jpeg_enc_host.h"

namespace R = gpv_enc_rule;

static std::vector<uint8_t> slurp(const std::string& path) {
  std::ifstream f(path, std::ios::binary);
  return std::vector<uint8_t>(std::istreambuf_iterator<char>(f), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <fixture directory>\n", argv[0]);
    return 2;
  }
  int failures = 0, files = 0;
  DIR* dir = opendir(argv[1]);
  if (!dir) {
    perror(argv[1]);
    return 2;
  }
  while (dirent* e = readdir(dir)) {
    std::string name = e->d_name;
    if (name.size() < 5 || name.substr(name.size() - 4) != ".rgb") continue;
    char content[64];
    int H, W, q, s;
    if (sscanf(name.c_str(), "%63[a-z]_%dx%d_q%d_s%d.rgb", content, &H, &W, &q, &s) != 5) {
      printf("FAIL %s: name does not parse\n", name.c_str());
      ++failures;
      continue;
    }
    std::string base = std::string(argv[1]) + "/" + name.substr(0, name.size() - 4);
    std::vector<uint8_t> rgb = slurp(base + ".rgb"), want = slurp(base + ".jpg"), got;
    bool ok = rgb.size() == (size_t)H * W * 3 && R::encode(rgb.data(), H, W, W, q, s, got) && got == want;
    printf("%s %s: %zu bytes, expected %zu\n", ok ? "ok  " : "FAIL", name.c_str(), got.size(), want.size());
    failures += !ok, ++files;
  }
  closedir(dir);
  if (!files) printf("FAIL no fixtures in %s\n", argv[1]), ++failures;

  // bad extents are refused
  std::vector<uint8_t> none;
  uint8_t one[3] = {1, 2, 3};
  bool refused = !R::encode(one, 0, 1, 1, 90, 2, none) && !R::encode(one, 1, 65536, 65536, 90, 2, none) && !R::encode(one, 1, 1, 1, 0, 2, none) &&
                 !R::encode(one, 1, 1, 1, 101, 2, none) && !R::encode(one, 1, 1, 1, 90, 3, none) && !R::encode(nullptr, 1, 1, 1, 90, 2, none) &&
                 !R::encode(one, 1, 2, 1, 90, 2, none);
  printf("%s bad extents refused\n", refused ? "ok  " : "FAIL");
  failures += !refused;

  long long tried = 0, wrong = 0;
  for (int q = 1; q <= 255; ++q) {
    uint32_t d = (uint32_t)q << 3, m = (uint32_t)((((uint64_t)1 << 32) + d - 1) / d);
    for (int c = -R::MAX_ABS_COEF; c <= R::MAX_ABS_COEF; ++c, ++tried) wrong += R::quantise(c, d, m) != R::quantise_div(c, (int)d);
  }
  printf("%s quantiser: multiply-and-shift == division on %lld (c, q) pairs, %lld differ\n", wrong ? "FAIL" : "ok  ", tried, wrong);
  failures += wrong != 0;

  // the largest outputs: every sample at an end of the range, in the sign pattern of each basis function
  int worst = 0;
  for (int u = 0; u < 8; ++u)
    for (int v = 0; v < 8; ++v) {
      int d[64];
      for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
          bool neg = ((((2 * i + 1) * u + 8) / 16) + (((2 * j + 1) * v + 8) / 16)) & 1;      // sign of cos((2i+1)u pi/16) cos((2j+1)v pi/16)
          d[8 * i + j] = neg ? -128 : 127;
        }
      R::fdct(d);
      for (int k = 0; k < 64; ++k) worst = abs(d[k]) > worst ? abs(d[k]) : worst;
    }
  printf("%s transform: largest |coefficient| over the 64 extreme blocks %d, bound %d\n", worst <= R::MAX_ABS_COEF ? "ok  " : "FAIL", worst, R::MAX_ABS_COEF);
  failures += worst > R::MAX_ABS_COEF;

  printf("%s: %d fixture files, %d failures\n", failures ? "FAILED" : "PASSED", files, failures);
  return failures ? 1 : 0;
}
