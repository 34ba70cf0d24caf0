// Stand-alone check of the label rule of gpv-1_amd/csrc/jpeg_enc_host.h (label_place, on_plate, label_ink, draw_labels: the text the
// device kernel compiles as well), in plain C++ (no HIP, no Python):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -ffp-contract=off -I gpv-1_amd/csrc tools/label_host_check.cpp -o label_host_check
//   ./label_host_check tests/golden/jpeg_labels
// Every <name>.txt of the directory (written by tools/gen_label_fixtures.py) states a case:
//   H W nboxes labels
//   nboxes lines: cx cy w h R G B L          (the box, its colour, its length byte)
//   one line: the `labels` text bytes in hex, or - if there are none
// <name>.rgb is the picture (raw RGB, H*W*3 bytes), <name>.out what the numpy rule made of it (draw_boxes_host, then
// draw_labels_host of what unpack_labels reads).  Here: box_rect, the outlines in box order, draw_labels; every byte must agree.
// The colours, length bytes and text lie in one exactly-sized heap block, as the device gets them, so that a read outside
// colours[0 .. 4 nboxes + labels) is an error under the sanitizer; some cases' length bytes claim more than is there.
// Exit status 0 only if every case agrees and bad extents are refused.
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

static bool run_case(const std::string& base, const char* name) {
  FILE* f = fopen((base + ".txt").c_str(), "r");
  if (!f) return false;
  int H = 0, W = 0, nboxes = -1, labels = -1;
  bool ok = fscanf(f, "%d %d %d %d", &H, &W, &nboxes, &labels) == 4 && H >= 1 && W >= 1 && nboxes >= 0 && nboxes <= R::MAX_BOXES &&
            labels >= 0 && labels <= nboxes * R::MAX_LABEL;
  std::vector<float> boxes(ok ? 4 * nboxes : 0);
  std::vector<int> rects(ok ? 4 * nboxes : 0);
  uint8_t* colours = ok ? (uint8_t*)malloc(4 * nboxes + labels + (nboxes + labels == 0)) : nullptr;      // exactly sized: see above
  for (int i = 0; ok && i < nboxes; ++i) {
    int c[4];
    ok = fscanf(f, "%f %f %f %f %d %d %d %d", &boxes[4 * i], &boxes[4 * i + 1], &boxes[4 * i + 2], &boxes[4 * i + 3], c, c + 1, c + 2, c + 3) == 8;
    for (int k = 0; ok && k < 4; ++k) colours[4 * i + k] = (uint8_t)c[k];
  }
  char hex[2 * R::MAX_BOXES * R::MAX_LABEL + 2] = {0};
  ok = ok && fscanf(f, "%2049s", hex) == 1 && (labels ? strlen(hex) == (size_t)2 * labels : !strcmp(hex, "-"));
  for (int k = 0; ok && k < labels; ++k) {
    unsigned v;
    ok = sscanf(hex + 2 * k, "%2x", &v) == 1;
    colours[4 * nboxes + k] = (uint8_t)v;
  }
  fclose(f);
  std::vector<uint8_t> rgb = slurp(base + ".rgb"), want = slurp(base + ".out");
  ok = ok && rgb.size() == (size_t)H * W * 3 && want.size() == rgb.size();
  if (ok) {
    for (int i = 0; i < nboxes; ++i) {
      R::box_rect(&boxes[4 * i], H, W, &rects[4 * i]);
      for (int y = 0; y < H; ++y)
        for (int x = 0; x < W; ++x)
          if (R::on_outline(&rects[4 * i], x, y))
            for (int ch = 0; ch < 3; ++ch) rgb[((size_t)y * W + x) * 3 + ch] = colours[4 * i + ch];
    }
    ok = R::draw_labels(rgb.data(), H, W, W, rects.data(), colours, nboxes, labels);
  }
  size_t differ = 0;
  for (size_t i = 0; ok && i < rgb.size(); ++i) differ += rgb[i] != want[i];
  free(colours);
  printf("%s %s: %d x %d, %d boxes, %d text bytes, %zu bytes differ\n", ok && !differ ? "ok  " : "FAIL", name, H, W, nboxes, labels, differ);
  return ok && !differ;
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
    if (name.size() < 5 || name.substr(name.size() - 4) != ".txt") continue;
    failures += !run_case(std::string(argv[1]) + "/" + name.substr(0, name.size() - 4), name.c_str()), ++files;
  }
  closedir(dir);
  if (!files) printf("FAIL no fixtures in %s\n", argv[1]), ++failures;

  // bad extents are refused, and nothing is written
  uint8_t px[3] = {1, 2, 3}, col[4 + 1] = {9, 9, 9, 1, 'A'};
  int rect[4] = {0, 0, 0, 0};
  bool refused = !R::draw_labels(px, 1, 1, 1, rect, col, 1, -1) && !R::draw_labels(px, 1, 1, 1, rect, col, 1, R::MAX_LABEL + 1) &&
                 !R::draw_labels(px, 1, 1, 1, rect, col, 0, 1) && !R::draw_labels(nullptr, 1, 1, 1, rect, col, 1, 1) &&
                 !R::draw_labels(px, 1, 1, 1, nullptr, col, 1, 1) && !R::draw_labels(px, 1, 1, 0, rect, col, 1, 1) &&
                 !R::draw_labels(px, 1, 1, 1, rect, col, R::MAX_BOXES + 1, 1) && px[0] == 1 && px[1] == 2 && px[2] == 3;
  printf("%s bad extents refused\n", refused ? "ok  " : "FAIL");
  failures += !refused;

  // every length byte against every extent of text: the clamps keep at + n inside the text, n inside MAX_LABEL
  long long tried = 0, outside = 0;
  for (int labels = 0; labels <= 2 * R::MAX_LABEL; ++labels)
    for (int before = 0; before <= 3 * R::MAX_LABEL; before += 7)
      for (int L = 0; L < 256; ++L, ++tried) {
        const R::Label l = R::label_place(rect, L, before, labels, 5, 5);
        outside += l.n < 0 || l.n > R::MAX_LABEL || l.at < 0 || l.at + l.n > labels || l.px < 0 || l.py < 0;
      }
  printf("%s clamps: %lld (length byte, offset, extent) triples, %lld leave the text\n", outside ? "FAIL" : "ok  ", tried, outside);
  failures += outside != 0;

  printf("%s: %d cases, %d failures\n", failures ? "FAILED" : "PASSED", files, failures);
  return failures ? 1 : 0;
}
