"""Calls of gpv_gemm / gpv_conv2d whose route (kernel family, instance, grid, block, LDS) is pinned: plain data, one dict per case.

Readers: tools/route_host_check.cpp (through case_line: one `key=value` line per case; prints the Route that gemm_route.h picks, no
GPU), tests/test_routes_cpu.py (compares those lines with tests/golden/routes/expected.txt) and tools/route_sweep.py (issues every
case with 'gpu' set once through hip.gemm / hip.conv2d / hip.set_option, for a kernel trace).

Keys of a gemm case: M N K, la lb (0 K-major, 1 reduction-major), batch, acc, split_k, res mask bias rowsum (0 / 1: operand present),
act, drop (0 / 1), alpha, din dout (0 bf16, 1 fp32), lda ldb ldc (0 = tight), offA offB (operand offset in ELEMENTS from a 16-byte
aligned base: 1 = misaligned), kpad (GPV_GEMM_KPAD_FINITE), nosmall (GPV_GEMM_NO_PIPE_SMALL).
Keys of a conv case: mode (0 forward, 1 backward-data, 2 weight gradient), B IH IW Cs Cin OH OW Cout KH KW SH SW PH PW, res mask bias,
act, bits (0 none, 1 y_mask_bits, 2 relu_mask_bits), split_k, din dout, offx.
Both: ws = workspace bytes the caller lends (what gpv1_amd.hip lends: its shared buffer, WS_MAX once grown, to accumulating GEMMs of
batch 1, to weight gradients, and to forward convolutions over <= 8192 pixels with K >= 1024), opts = {option number: value} set for
the call, gpu = the sweep issues it (the others state a workspace hip.py would not lend, or an operand it cannot build).
A new kernel family adds its rows here: the shapes it is for, and one case on each side of every threshold of its select."""
import json
import os

WS_MAX = 256 << 20
OPT = dict(GLDS=0, SKINNY=2, GLDS_WGRAD=3, PIPE=4, C1S=6, C3S=7, GEMV=9, PIPE_SMALL=17, C3_HALO=19)

GEMM_DEFAULTS = dict(ep='gemm', la=0, lb=0, batch=1, acc=0, split_k=1, res=0, mask=0, bias=0, rowsum=0, act=0, drop=0, alpha=1.0, din=0, dout=0,
                     lda=0, ldb=0, ldc=0, offA=0, offB=0, kpad=0, nosmall=0, ws=0, opts={}, gpu=1)
CONV_DEFAULTS = dict(ep='conv', mode=0, KH=1, KW=1, SH=1, SW=1, PH=0, PW=0, res=0, mask=0, bias=0, act=0, bits=0, split_k=0, din=0, dout=0, offx=0,
                     ws=0, opts={}, gpu=1)


def gemm(name, M, N, K, **kw):
    c = dict(GEMM_DEFAULTS, name=name, M=M, N=N, K=K)
    c.update(kw)
    if c['acc'] and c['batch'] == 1 and 'ws' not in kw:
        c['ws'] = WS_MAX
        c['dout'] = 1
    return c


def conv(name, mode, B, IH, IW, Cin, Cout, k=1, s=1, **kw):
    p = k // 2
    OH, OW = (IH + 2 * p - k) // s + 1, (IW + 2 * p - k) // s + 1
    if mode == 1:                          # backward-data: dx [IH, IW, Cin] from dy [OH, OW, Cout]; the library's "input" is dy
        c = dict(CONV_DEFAULTS, name=name, mode=1, B=B, IH=OH, IW=OW, Cs=Cout, Cin=Cout, OH=IH, OW=IW, Cout=Cin, KH=k, KW=k, SH=s, SW=s, PH=p, PW=p)
    else:
        c = dict(CONV_DEFAULTS, name=name, mode=mode, B=B, IH=IH, IW=IW, Cs=Cin, Cin=Cin, OH=OH, OW=OW, Cout=Cout, KH=k, KW=k, SH=s, SW=s, PH=p, PW=p)
    c.update(kw)
    if 'ws' not in kw:
        if mode == 2:
            c['ws'], c['dout'] = WS_MAX, 1
        elif mode == 0 and B * OH * OW <= 8192 and k * k * Cin >= 1024:
            c['ws'] = WS_MAX
    elif mode == 2:
        c['dout'] = 1
    return c


def _step_rows():
    """every row of tools/gemm_shapes_step.json (the gpv_gemm calls of one eager training step of the bench model)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools', 'gemm_shapes_step.json')
    out = []
    for i, (r, _count) in enumerate(json.load(open(path))):
        M, N, K, la, lb, batch, acc, res, mask, act, drop, f32, ntA, ntB, ntC = r
        ta, tb = (M if la else K), (N if lb else K)
        kw = dict(la=la, lb=lb, batch=batch, acc=acc, res=res, mask=mask, act=act, drop=drop, dout=f32, bias=int(not acc),
                  lda=3 * ta if ntA else 0, ldb=2 * tb if ntB else 0, ldc=2 * N if ntC else 0)     # (packed operands: the pitch of a wider row)
        if la and lb and acc and batch == 1:
            kw['rowsum'] = 1
        out.append(gemm('step%02d' % i, M, N, K, **kw))
    return out


def _resnet(tag, B, H, W):
    """the gpv_conv2d calls of the ResNet-50 body on an H x W image: per distinct convolution forward, backward-data and weight
    gradient, with the epilogues the backbone uses (bias + ReLU, + residual, ReLU mask, one-bit masks where they exist)"""
    out = []
    h, w, cin = H // 4, W // 4, 64
    for li, planes in enumerate((64, 128, 256, 512)):
        stride = 1 if li == 0 else 2
        oh, ow = h // stride, w // stride
        geoms = [('c1a', h, w, cin, planes, 1, 1), ('c2a', h, w, planes, planes, 3, stride), ('c3', oh, ow, planes, 4 * planes, 1, 1),
                 ('ds', h, w, cin, 4 * planes, 1, stride), ('c1', oh, ow, 4 * planes, planes, 1, 1), ('c2', oh, ow, planes, planes, 3, 1)]
        for g, ih, iw, ci, co, k, s in geoms:
            n = '%s.l%d.%s' % (tag, li + 1, g)
            pw = k == 1 and s == 1
            out.append(conv(n + '.fwd', 0, B, ih, iw, ci, co, k, s, bias=1, act=0 if g in ('c3', 'ds') else 1))
            if g == 'c3':
                out.append(conv(n + '.fwd.res', 0, B, ih, iw, ci, co, k, s, bias=1, res=1, act=1))
                out.append(conv(n + '.fwd.res.bits', 0, B, ih, iw, ci, co, k, s, bias=1, res=1, act=1, bits=1))
            out.append(conv(n + '.dgrad', 1, B, ih, iw, ci, co, k, s))
            out.append(conv(n + '.dgrad.mask', 1, B, ih, iw, ci, co, k, s, mask=1))
            if g in ('c1', 'c1a', 'ds'):
                out.append(conv(n + '.dgrad.res.mask', 1, B, ih, iw, ci, co, k, s, res=1, mask=1))
            if (pw and ci % 256 == 0 and g != 'c3') or (k == 3 and s == 2 and ci == 128):
                out.append(conv(n + '.dgrad.bits', 1, B, ih, iw, ci, co, k, s, res=int(pw), bits=2))
            out.append(conv(n + '.wgrad', 2, B, ih, iw, ci, co, k, s))
            out.append(conv(n + '.wgrad.nows', 2, B, ih, iw, ci, co, k, s, ws=0, gpu=0))
        h, w, cin = oh, ow, 4 * planes
    return out


def _decode():
    """the decode step's M <= 8 GEMMs (greedy decode at batch 1..8: projections, feed-forward, vocabulary)"""
    out = []
    for M in (1, 2, 4, 8):
        for N, K in ((768, 768), (2304, 768), (3072, 768), (768, 3072), (10000, 768)):
            out.append(gemm('decode.m%d.%dx%d' % (M, N, K), M, N, K, bias=1))
    out.append(gemm('decode.m1.f32out', 1, 10000, 768, dout=1))
    return out


def _thresholds():
    """one case on each side of the thresholds of gemm_route.h's selects"""
    o, G, C = [], gemm, conv
    # gemv: M <= 8; > 2 rows stop at N >= 4096; columns per wave at N = 2048 / 4096
    o += [G('gemv.m8', 8, 768, 768), G('gemv.m9', 9, 768, 768), G('gemv.m2.n4096', 2, 4096, 768), G('gemv.m3.n4096', 3, 4096, 768),
          G('gemv.m3.n4088', 3, 4088, 768), G('gemv.m1.n2040', 1, 2040, 768), G('gemv.m1.n2048', 1, 2048, 768), G('gemv.off', 4, 768, 768, opts={OPT['GEMV']: 0}),
          G('gemv.forced', 4, 768, 768, opts={OPT['GLDS']: 2})]
    # c1s from gpv_gemm: K = 256, N >= 1536, M >= 2048
    o += [G('c1s.lin.n1536', 9600, 1536, 256, bias=1, act=1), G('c1s.lin.n1280', 9600, 1280, 256, bias=1, act=1), G('c1s.lin.m2048', 2048, 2048, 256, bias=1),
          G('c1s.lin.m2047', 2047, 2048, 256, bias=1), G('c1s.lin.k512', 9600, 2048, 512, bias=1), G('c1s.lin.drop', 9600, 2048, 256, bias=1, act=1, drop=1),
          G('c1s.lin.legal', 640, 512, 256, bias=1, opts={OPT['C1S']: 2}), G('c1s.lin.off', 9600, 2048, 256, bias=1, opts={OPT['C1S']: 0})]
    # c1s from gpv_conv2d: M >= 32768 and M x slices >= 65536; the non-temporal instances from 200 MB of output
    o += [C('c1s.m32768', 0, 1, 128, 256, 256, 1024, bias=1), C('c1s.m32760', 0, 1, 130, 252, 256, 1024, bias=1), C('c1s.rows65536', 0, 1, 256, 256, 64, 256, bias=1),
          C('c1s.rows65280', 0, 1, 255, 256, 64, 256, bias=1),
          C('c1s.nt.200mb', 0, 32, 80, 160, 64, 256, bias=1, act=1), C('c1s.nt.199mb', 0, 32, 80, 159, 64, 256, bias=1, act=1),
          C('c1s.legal', 0, 1, 30, 40, 256, 1024, bias=1, opts={OPT['C1S']: 2}), C('c1s.k512.n256', 0, 32, 60, 80, 512, 256, bias=1),
          C('c1s.s2', 0, 32, 120, 160, 256, 512, 1, 2, bias=1)]
    # pipe: the small-M configurations (<= 250 tiles of 64 x 64, >= 100 or K <= 1024; 32 x 64 below 128 tiles), K >= 256
    # (N = 64: no 128-wide tile, so the two-per-CU fill of gemm_glds.hip does not turn these away first)
    o += [G('pipe.small.t36', 192, 768, 768), G('pipe.small.t36.k3072', 192, 768, 3072), G('pipe.small.t100.k3072', 6400, 64, 3072),
          G('pipe.small.t99.k3072', 6336, 64, 3072), G('pipe.small.t99.k1024', 6336, 64, 1024), G('pipe.small.t99.k1088', 6336, 64, 1088),
          G('pipe.small.t127', 8128, 64, 768), G('pipe.small.t128', 8192, 64, 768), G('pipe.small.t120', 640, 768, 2048, opts={OPT['GLDS']: 0}), G('pipe.small.t130', 640, 832, 768),
          G('pipe.small.t250', 640, 1600, 768), G('pipe.small.t260', 640, 1664, 768), G('pipe.small.k192', 192, 768, 192),
          G('pipe.small.off', 192, 768, 768, opts={OPT['PIPE_SMALL']: 0}), G('pipe.small.flag', 192, 768, 768, nosmall=1)]
    # pipe: the big tiles (K >= 512, 2048 <= M <= 40000, N >= 256, not N >= 1024 with M >= 9600, <= 24 Mi outputs)
    o += [G('pipe.big', 3200, 768, 768, opts={OPT['GLDS']: 0}), G('pipe.big.k448', 3200, 768, 448), G('pipe.big.m2048', 2048, 768, 1024), G('pipe.big.m1984', 1984, 768, 1024),
          G('pipe.big.m40000', 40000, 384, 1024), G('pipe.big.m40001', 40001, 384, 1024), G('pipe.big.n192', 9600, 192, 1024),     # (shapes whose 160- / 96-row tiles
          G('pipe.big.n1152.m9600', 9600, 1152, 1024), G('pipe.big.n1152.m9599', 9599, 1152, 1024),                                # fill no whole two-per-CU round)
          G('pipe.big.n1024.m10400', 10400, 1024, 1024), G('pipe.big.n896.m11700', 11700, 896, 1024),
          G('pipe.big.cost.k512', 16384, 768, 512), G('pipe.big.cost.k768', 16384, 768, 768),      # 256- against 128-row tiles: decided by the fixed cost per tile
          G('pipe.big.24mi', 32768, 768, 512), G('pipe.big.24mi+', 32832, 768, 512),
          G('pipe.off', 3200, 768, 768, opts={OPT['PIPE']: 0})]
    o += [G('pipe.cfg%d' % i, 2048, 768, 1024, opts={OPT['PIPE']: 100 + i}) for i in range(9)]
    # two-per-CU tiles of gemm_glds.hip: > 384 tiles in whole rounds, the 96-row fill at <= 1024 rows, K >= 512
    o += [G('two.bm96.fill', 640, 768, 2048), G('two.bm96.fill.noskinny', 640, 768, 2048, opts={OPT['SKINNY']: 0}), G('two.bm96.fill.m1024', 1024, 768, 2048), G('two.bm96.fill.m1056', 1056, 768, 2048), G('two.160', 9600, 1024, 1024),
          G('two.96', 9600, 512, 1024), G('two.k448', 9600, 1024, 448), G('two.t384', 7680, 1024, 1024), G('two.t385', 12320, 640, 1024), G('two.oneround.t480', 19200, 512, 1024),
          G('two.t513', 4320, 2432, 1024), G('two.u0894', 43968, 256, 512), G('two.u0904', 44448, 256, 512),      # 916 / 926 tiles of 96 rows in two rounds of 512
          G('two.bm96.fill.t256', 768, 4096, 1024), G('two.bm96.fill.t264', 768, 4224, 1024),                     # the fill: <= 256 tiles of 96 rows ...
          G('two.bm96.fill.r120', 576, 768, 2048), G('two.bm96.fill.r117', 672, 768, 2048)]                       # ... that are >= 1.2 x the 128-row ones (6 : 5, 7 : 6)
    # glds: huge (>= 1024 tiles of 256 rows, K >= 512), 4-wave tiles (K >= 1024, or K >= 512 without a mask), forced variants
    o += [G('glds.huge.t1024', 131072, 320, 512), G('glds.huge.t1023', 261888, 96, 512), G('glds.small.k1024.mask', 50000, 320, 1024, mask=1),
          G('glds.small.k960.mask', 50000, 320, 960, mask=1), G('glds.small.k512', 50000, 320, 512), G('glds.small.k448', 50000, 320, 448), G('glds.n64', 50000, 64, 1024),
          G('glds.mode2', 3200, 768, 768, opts={OPT['GLDS']: 2}), G('glds.mode3', 3200, 768, 768, opts={OPT['GLDS']: 3}), G('glds.f32out', 50000, 320, 1024, dout=1),
          G('glds.off', 50000, 320, 1024, opts={OPT['GLDS']: 0, OPT['PIPE']: 0})]
    # skinny: <= 360 tiles of 64 x 64 with K >= 128 (reduction-major B: <= 640 with K >= 2048); 32 x 32 tiles up to 160
    o += [G('skinny.t360', 1536, 960, 192), G('skinny.t375', 1600, 960, 192), G('skinny.k120', 640, 768, 120), G('skinny.k128', 640, 768, 128), G('skinny.t160', 640, 1024, 192),
          G('skinny.t170', 640, 1088, 192), G('skinny.bt.t640', 40960, 64, 2048, lb=1), G('skinny.bt.t641', 41024, 64, 2048, lb=1), G('skinny.bt.k1984', 3200, 768, 1984, lb=1),
          G('skinny.bt.small', 640, 768, 768, lb=1), G('skinny.f32out', 192, 768, 3072, dout=1), G('skinny.off', 192, 768, 3072, opts={OPT['SKINNY']: 0}),
          G('skinny.legal', 9600, 256, 2048, lb=1, opts={OPT['SKINNY']: 2}), G('skinny.k64', 192, 768, 64)]
    # weight gradients: glds_tt from 3000 tile-k-steps, skinny_tt up to 256 tiles with >= 4 k-steps of 128, else the tile kernel
    o += [G('tt.glds.3000', 768, 768, 5376, la=1, lb=1, acc=1), G('tt.glds.2988', 768, 768, 5312, la=1, lb=1, acc=1), G('tt.glds.legal', 256, 256, 9600, la=1, lb=1, acc=1, opts={OPT['GLDS_WGRAD']: 2}),
          G('tt.glds.off', 768, 3072, 3200, la=1, lb=1, acc=1, opts={OPT['GLDS_WGRAD']: 0}), G('tt.skinny.t256', 1024, 1024, 640, la=1, lb=1, acc=1),
          G('tt.skinny.t272', 1024, 1088, 640, la=1, lb=1, acc=1), G('tt.skinny.nk3', 256, 256, 384, la=1, lb=1, acc=1), G('tt.skinny.nk4', 256, 256, 512, la=1, lb=1, acc=1),
          G('tt.skinny.nows', 256, 256, 9600, la=1, lb=1, acc=1, ws=0, dout=1, gpu=0), G('tt.noacc', 256, 256, 9600, la=1, lb=1, dout=1), G('tt.splitk', 256, 256, 9600, la=1, lb=1, acc=1, split_k=8),
          G('tt.splitk.nows', 250, 250, 9600, la=1, lb=1, acc=1, split_k=8, ws=0, dout=1, gpu=0)]
    # the register-staged kernel's tiles: K <= 256 (64 x 64 unless N >= 1024 with >= 384 tiles of 128 x 128), N <= 64, >= 384 tiles
    o += [G('tile.k256.wide', 9600, 2048, 256, din=1, dout=1), G('tile.k256.t384', 6080, 1024, 256, din=1, dout=1), G('tile.k256.t380', 4864, 1280, 256, din=1, dout=1), G('tile.k257', 9600, 2048, 264, din=1, dout=1),
          G('tile.n64', 98304, 64, 576, din=1, dout=1), G('tile.n64.few', 49000, 64, 576, din=1, dout=1), G('tile.t128.384', 3072, 2048, 512, din=1, dout=1),
          G('tile.t128.368', 2944, 2048, 512, din=1, dout=1), G('tile.small', 300, 300, 512, din=1, dout=1), G('tile.bf16.f32', 300, 300, 300, dout=1, opts={OPT['SKINNY']: 0}),
          G('tile.batch', 100, 2048, 300, lb=1, batch=32), G('tile.batch.f32in.bf16out', 100, 100, 100, din=1, dout=0, gpu=0)]
    # c3s: >= 65536 output pixels, or the 64-channel forward from 16384; halo images up to 47 pixels wide; the split forward conv
    o += [C('c3s.m65536', 0, 1, 256, 256, 128, 128, 3, 1, bias=1, act=1), C('c3s.m65280', 0, 1, 255, 256, 128, 128, 3, 1, bias=1, act=1), C('c3s.c64.m16384', 0, 1, 128, 128, 64, 64, 3, 1, bias=1),
          C('c3s.c64.m16256', 0, 1, 127, 128, 64, 64, 3, 1, bias=1), C('c3s.c64.dgrad.m16384', 1, 1, 128, 128, 64, 64, 3, 1), C('c3s.legal', 0, 1, 30, 40, 128, 128, 3, 1, opts={OPT['C3S']: 2}),
          C('c3s.off', 0, 32, 120, 160, 64, 64, 3, 1, bias=1, opts={OPT['C3S']: 0}), C('c3s.n320', 0, 8, 120, 160, 64, 320, 3, 1, bias=1),
          C('halo.w47', 0, 32, 24, 47, 256, 256, 3, 1, bias=1, act=1), C('halo.w48', 0, 32, 24, 48, 256, 256, 3, 1, bias=1, act=1), C('halo.off', 0, 32, 30, 40, 256, 256, 3, 1, bias=1, opts={OPT['C3_HALO']: 0}),
          C('halo.96', 0, 32, 15, 20, 512, 512, 3, 1, bias=1, opts={OPT['C3_HALO']: 2}),
          C('split.t160', 0, 1, 64, 80, 128, 128, 3, 1, bias=1, act=1), C('split.t161', 0, 1, 32, 46, 128, 448, 3, 1, bias=1, act=1), C('split.t162', 0, 1, 64, 81, 128, 128, 3, 1, bias=1, act=1), C('split.kt32', 0, 1, 30, 40, 1024, 256, 1, 2, bias=1), C('split.kt31', 0, 1, 30, 40, 992, 256, 1, 2, bias=1, ws=WS_MAX, gpu=0),
          C('split.kt36', 0, 1, 30, 40, 128, 256, 3, 2, bias=1), C('split.smallws', 0, 1, 30, 40, 256, 256, 3, 1, bias=1, ws=3 * 1200 * 256 * 4, gpu=0),
          C('split.forced', 0, 1, 30, 40, 256, 256, 3, 1, bias=1, opts={OPT['PIPE']: 102}),
          C('split.cap16', 0, 1, 15, 20, 544, 256, 3, 1, bias=1), C('split.slots384', 0, 1, 24, 32, 256, 256, 3, 1, bias=1)]      # 20 tiles x 153 k-tiles; 48 tiles: 384 / 48 = 8 splits
    # weight-gradient tiles without / with too small a workspace, forced split
    o += [C('wgrad.smallws', 2, 32, 30, 40, 256, 256, 3, 1, ws=1 << 20, gpu=0), C('wgrad.split4', 2, 32, 30, 40, 256, 256, 3, 1, split_k=4), C('wgrad.c64', 2, 32, 120, 160, 64, 64, 1, 1),
          C('wgrad.f32', 2, 2, 30, 40, 64, 64, 3, 1, din=1), C('wgrad.off', 2, 32, 30, 40, 256, 256, 3, 1, opts={OPT['GLDS_WGRAD']: 0}),
          # the split of ONE 128 x 128 tile is capped at 288 (4896 = 17 x 288 and 4624 = 16 x 289 k-tiles: a cap one off splits them differently)
          C('wgrad.cap288.kt4896', 2, 32, 68, 72, 128, 128, 1, 1, opts={OPT['GLDS_WGRAD']: 0}), C('wgrad.cap288.kt4624', 2, 32, 68, 68, 128, 128, 1, 1, opts={OPT['GLDS_WGRAD']: 0}),
          # tiles of the register-staged kernel: 128 x 128 from 256 (tiles x splits), 128 x 64 from 384
          C('wgrad.tile.s256', 2, 32, 60, 80, 128, 128, 1, 1, split_k=256, opts={OPT['GLDS_WGRAD']: 0}), C('wgrad.tile.s255', 2, 32, 60, 80, 128, 128, 1, 1, split_k=255, opts={OPT['GLDS_WGRAD']: 0}),
          C('wgrad.tile.c64.s384', 2, 32, 60, 80, 64, 128, 1, 1, split_k=384), C('wgrad.tile.c64.s383', 2, 32, 60, 80, 64, 128, 1, 1, split_k=383),
          # the direct-to-LDS kernel stages 64 pixels = 64 / OW rows (+ 2) of one image at a time
          C('wgrad.oh10.ow8', 2, 32, 10, 8, 128, 128, 3, 1), C('wgrad.oh9.ow8', 2, 32, 9, 8, 128, 128, 3, 1)]
    return o


def _ragged():
    """one misaligned-operand and one ragged-K case per layout; refused calls"""
    o, G, C = [], gemm, conv
    for la, lb, tag in ((0, 0, 'kk'), (0, 1, 'kt'), (1, 1, 'tt')):
        o.append(G('misaligned.' + tag, 640, 768, 768, la=la, lb=lb, offA=1, offB=1, acc=int(la and lb), dout=int(la and lb)))
        o.append(G('raggedk.' + tag, 640, 768, 763, la=la, lb=lb, lda=0 if la else 768, ldb=0 if lb else 768, acc=int(la and lb), dout=int(la and lb)))
    o.append(G('raggedk.kk.kpad', 640, 768, 763, lda=768, ldb=768, kpad=1))
    o.append(G('raggedn.kt', 640, 765, 768, lb=1, ldb=768))
    o.append(C('misaligned.conv1x1', 0, 32, 30, 40, 1024, 256, offx=1, bias=1))
    o.append(C('misaligned.conv3x3', 0, 32, 30, 40, 256, 256, 3, 1, offx=1, bias=1))
    o.append(C('misaligned.wgrad', 2, 32, 30, 40, 256, 256, 3, 1, offx=1))
    o.append(G('refused.splitk.bf16', 256, 256, 9600, la=1, lb=1, acc=1, split_k=8, ws=0, dout=0, gpu=0))
    o.append(G('refused.rowsum.kk', 256, 256, 9600, rowsum=1, gpu=0))
    o.append(C('refused.cin48', 0, 1, 30, 40, 48, 64, 3, 1, gpu=0))
    o.append(C('refused.bits.cout128', 0, 32, 60, 80, 64, 128, bias=1, res=1, act=1, bits=1, gpu=0))
    o.append(C('refused.bits.nores', 0, 32, 60, 80, 128, 512, bias=1, act=1, bits=1, gpu=0))
    o.append(C('refused.bits.small', 0, 1, 30, 40, 256, 1024, bias=1, res=1, act=1, bits=1, gpu=0))
    return o


CASES = _step_rows() + _resnet('b32', 32, 480, 640) + _resnet('b1', 1, 480, 640) + _decode() + _thresholds() + _ragged()
assert len({c['name'] for c in CASES}) == len(CASES)


def case_line(c):
    """the case as tools/route_host_check.cpp reads it"""
    kv = ['%s=%s' % (k, v) for k, v in c.items() if k not in ('name', 'ep', 'opts', 'gpu')]
    kv += ['opt%d=%d' % (o, v) for o, v in sorted(c['opts'].items())]
    return '%s %s %s' % (c['ep'], c['name'], ' '.join(kv))


if __name__ == '__main__':
    for case in CASES:
        print(case_line(case))
