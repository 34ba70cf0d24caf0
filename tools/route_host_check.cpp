// Stand-alone run of the GEMM / convolution routing (gpv-1_amd/csrc/gemm_route.h) on the host: which kernel family, instance, grid,
// block and LDS size does a gpv_gemm / gpv_conv2d call take?  No GPU, no HIP, no Python.  Build and run from the repository root:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/route_host_check tools/route_host_check.cpp
//   python tests/route_cases.py | /tmp/route_host_check
// Input: one case per line, `gemm|conv <name> key=value ...` (tests/route_cases.py case_line).  Operands are fake addresses of the
// stated alignment (never dereferenced: routing reads shapes, pitches, alignments and whether an optional operand is there).
// Output: one line per case, `<name>: <route>` -- the route of each part, or `refused <code>`.  tests/test_routes_cpu.py compares the
// lines with tests/golden/routes/expected.txt.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include "../gpv-1_amd/csrc/gemm_route.h"

using namespace gpvk;

namespace gpvk { Knobs g_knobs; }

static void* fake(uintptr_t slot, long off_bytes) { return reinterpret_cast<void*>((slot << 32) + 0x1000 + (uintptr_t)off_bytes); }

static void print_route(const Route& r) {
  printf("%s", family_name(r.family));
  switch (r.family) {
    case FAM_GEMV: printf(" in%d out%d MR=%d NW=%d", r.dt_in, r.dt_out, r.bm, r.bn); break;
    case FAM_C1S: printf(" K=%d NH=%d RES=%d MASK=%d NT=%d LIN=%d NP=%d BITS=%d ncols=%d", r.ck, r.nh, r.res, r.mask, r.nt, r.lin, r.np, r.bits, r.ncols); break;
    case FAM_C3S: printf(" %s CIN=%d DGRAD=%d MASK=%d WAVES=%d BITS=%d rows=%d nstrip=%d nseg=%d nitems=%d", r.d2 ? "c3d2" : "c3r", r.ck, r.dgrad, r.mask, r.waves, r.bits,
                         r.rows, r.nstrip, r.nseg, r.nitems); break;
    case FAM_PIPE: printf(" A%d cfg=%d %dx%d WM=%d NS=%d c11=%d depi=%d", r.amode, r.cfg, r.bm, r.bn, kCfgs[r.cfg].wm, kCfgs[r.cfg].ns, r.c11, r.depi); break;
    case FAM_SKINNY: printf(" B%d out%d %dx%d NST=%d", r.bmode, r.dt_out, r.bm, r.bn, r.cfg); break;
    case FAM_GLDS: printf(" A%d out%d %dx%d c11=%d depi=%d", r.amode, r.dt_out, r.bm, r.bn, r.c11, r.depi); break;
    case FAM_HALO: printf(" BM=%d", r.bm); break;
    case FAM_TILE: printf(" A%d B%d in%d out%d %dx%d VEC=%d c11=%d nt=%d", r.amode, r.bmode, r.dt_in, r.dt_out, r.bm, r.bn, r.vec, r.c11, r.nt); break;
    case FAM_S2_FILL: printf(" C8=%d", r.ncols); break;
    default: break;
  }
  printf(" grid=(%u,%u,%u) block=%u lds=%lld", r.gx, r.gy, r.gz, r.block, (long long)r.lds);
  if (r.split || r.kt_per_split) printf(" split=%d kt_per_split=%d two_pass=%d", r.split, r.kt_per_split, r.two_pass);
}

int main() {
  char* line = nullptr;
  size_t cap = 0;
  long n = 0;
  while (getline(&line, &cap, stdin) > 0) {
    std::map<std::string, double> kv;
    std::string ep, name;
    int field = 0;
    for (char* tok = strtok(line, " \n"); tok; tok = strtok(nullptr, " \n"), ++field) {
      if (field == 0) { ep = tok; continue; }
      if (field == 1) { name = tok; continue; }
      char* eq = strchr(tok, '=');
      if (!eq) { printf("%s: bad token %s\n", name.c_str(), tok); return 2; }
      kv[std::string(tok, eq - tok)] = atof(eq + 1);
    }
    if (ep.empty()) continue;
    auto I = [&](const char* k) { auto it = kv.find(k); if (it == kv.end()) { printf("%s: key %s missing\n", name.c_str(), k); exit(2); } return (long)it->second; };
    Knobs kn;                                            // the library's defaults, then the case's options
    for (const auto& e : kv) {
      if (e.first.compare(0, 3, "opt") != 0) continue;
      const int o = atoi(e.first.c_str() + 3), v = (int)e.second;
      switch (o) {
        case GPV_OPT_GLDS: kn.glds = v; break;
        case GPV_OPT_SKINNY: kn.skinny = v; break;
        case GPV_OPT_GLDS_WGRAD: kn.wgrad = v; break;
        case GPV_OPT_PIPE: kn.pipe = v; break;
        case GPV_OPT_C1S: kn.c1s = v; break;
        case GPV_OPT_C3S: kn.c3s = v; break;
        case GPV_OPT_GEMV: kn.gemv = v; break;
        case GPV_OPT_PIPE_SMALL: kn.pipe_small = v; break;
        case GPV_OPT_C3_HALO: kn.halo = v; break;
        default: printf("%s: option %d is not a routing mode\n", name.c_str(), o); return 2;
      }
    }
    Routed rt;
    void* ws = I("ws") ? fake(7, 0) : nullptr;
    if (ep == "gemm") {
      gpv_gemm_args a;
      memset(&a, 0, sizeof(a));
      const int esz = I("din") ? 4 : 2;
      a.M = (int)I("M"); a.N = (int)I("N"); a.K = (int)I("K"); a.batch = (int)I("batch");
      a.layoutA = (int)I("la"); a.layoutB = (int)I("lb");
      a.lda = I("lda") ? I("lda") : (a.layoutA ? a.M : a.K);
      a.ldb = I("ldb") ? I("ldb") : (a.layoutB ? a.N : a.K);
      a.ldc = I("ldc") ? I("ldc") : a.N;
      a.sA = (int64_t)(a.layoutA ? a.K : a.M) * a.lda; a.sB = (int64_t)(a.layoutB ? a.K : a.N) * a.ldb; a.sC = (int64_t)a.M * a.ldc;
      a.A = fake(1, I("offA") * esz); a.B = fake(2, I("offB") * esz); a.C = fake(3, 0);
      a.dtype_in = (int)I("din"); a.dtype_out = (int)I("dout");
      a.alpha = (float)kv["alpha"];
      if (I("bias")) a.bias = (const float*)fake(4, 0);
      if (I("res")) { a.res = fake(5, 0); a.ldr = a.ldc; a.sR = a.sC; }
      if (I("mask")) { a.relu_mask = fake(6, 0); a.ldm = a.ldc; }
      if (I("rowsum")) a.a_rowsum = (float*)fake(8, 0);
      a.act = (int)I("act"); a.drop_p = I("drop") ? 0.1f : 0.f; a.seed = 1;
      a.accumulate = (int)I("acc"); a.split_k = (int)I("split_k");
      a.flags = (I("kpad") ? GPV_GEMM_KPAD_FINITE : 0) | (I("nosmall") ? GPV_GEMM_NO_PIPE_SMALL : 0);
      a.workspace = ws; a.workspace_bytes = I("ws");
      route_gemm(&a, kn, &rt);
    } else if (ep == "conv") {
      gpv_conv_args a;
      memset(&a, 0, sizeof(a));
      const int esz = I("din") ? 4 : 2;
      a.mode = (int)I("mode");
      a.B = (int)I("B"); a.IH = (int)I("IH"); a.IW = (int)I("IW"); a.Cs = (int)I("Cs"); a.Cin = (int)I("Cin"); a.OH = (int)I("OH"); a.OW = (int)I("OW"); a.Cout = (int)I("Cout");
      a.KH = (int)I("KH"); a.KW = (int)I("KW"); a.SH = (int)I("SH"); a.SW = (int)I("SW"); a.PH = (int)I("PH"); a.PW = (int)I("PW");
      a.x = fake(1, I("offx") * esz); a.w = fake(2, 0); a.y = fake(3, 0);
      a.dtype_in = (int)I("din"); a.dtype_out = (int)I("dout");
      if (I("bias")) a.bias = (const float*)fake(4, 0);
      if (I("res")) a.res = fake(5, 0);
      if (I("mask")) a.relu_mask = fake(6, 0);
      if (I("bits") == 1) a.y_mask_bits = fake(9, 0);
      if (I("bits") == 2) a.relu_mask_bits = fake(9, 0);
      a.act = (int)I("act"); a.split_k = (int)I("split_k");
      a.workspace = ws; a.workspace_bytes = I("ws");
      route_conv2d(&a, kn, &rt);
    } else {
      printf("%s: unknown entry point %s\n", name.c_str(), ep.c_str());
      return 2;
    }
    printf("%s: ", name.c_str());
    if (rt.err) printf("refused %d", rt.err);
    for (int i = 0; !rt.err && i < rt.nparts; ++i) {
      if (i) printf(" + ");
      print_route(rt.r[i]);
    }
    printf("\n");
    ++n;
  }
  free(line);
  fprintf(stderr, "ok: %ld cases routed\n", n);
  return 0;
}
