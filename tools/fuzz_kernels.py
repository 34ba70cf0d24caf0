"""Random-shape sweep of the round-3 kernels against the references the unit tests use (fp32 torch / the oracles): calls the tests'
own check functions with shapes no parametrisation lists.  A failure prints the shape and keeps going.
usage: python tools/fuzz_kernels.py [seed] [rounds]        (GPU box)"""
import os, sys, random, traceback
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import tests.test_kernels_gpu as T

seed = int(sys.argv[1]) if len(sys.argv) > 1 else 0
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 12
rng = random.Random(seed)
h = T.hip()
fails = []


out_of_range = 0


def run(name, fn, *a, **kw):
    global out_of_range
    try:
        fn(*a, **kw)
    except RuntimeError as e:
        if name in ('attention', 'attention_bwd1') and 'hipError 1' in str(e):   # K / V (+ Q) of a head beyond the LDS: refused before any launch (gpv_hip.h)
            out_of_range += 1
            return
        fails.append((name, a, kw, repr(e)[:200]))
        print('FAIL', name, a, kw, repr(e)[:300], flush=True)
    except Exception as e:                                   # noqa: BLE001
        fails.append((name, a, kw, repr(e)[:200]))
        print('FAIL', name, a, kw, repr(e)[:300], flush=True)
        torch.cuda.synchronize()


for it in range(rounds):
    # streaming 3x3 (forced on): strips of 30 columns, row segments of 3, both channel counts, stride-2 backward-data
    prev = h.set_option(h.OPT_C3S, 2)
    h.set_option(h.OPT_C3S_LAUNCHES, 0)
    Cin, Cout = rng.choice([(64, 64), (128, 128), (64, 128), (128, 64)])
    s = rng.choice([1, 1, 2])
    H, W = rng.randint(3, 40), rng.randint(3, 95)
    if s == 2:
        H, W = 2 * rng.randint(2, 18), 2 * rng.randint(2, 40)
    run('c3s', T.test_streaming_3x3_conv_kernel_forced.__wrapped__ if hasattr(T.test_streaming_3x3_conv_kernel_forced, '__wrapped__') else T.test_streaming_3x3_conv_kernel_forced,
        h, Cin, Cout, s, H, W, rng.randint(1, 4))
    h.set_option(h.OPT_C3S, prev)
    # fused stem
    run('stem', T.test_fused_stem_conv_bn_relu_maxpool, rng.randint(1, 3), rng.randint(20, 140), rng.randint(20, 200))
    # fused block tails
    K1, K2, N, s2 = rng.choice([(64, 64, 256, 1), (128, 256, 512, 2)])
    run('c1d', T.test_fused_block_tail_conv3_plus_downsample, K1, K2, N, s2, rng.randint(2, 33), rng.randint(2, 41), rng.randint(1, 4))
    # generic conv fwd / dgrad / wgrad on random shapes incl. the two-per-CU and pipelined kernels' territory
    Cin = rng.choice([64, 128, 256, 512])
    Cout = rng.choice([64, 128, 256, 512])
    k = rng.choice([1, 3])
    s = rng.choice([1, 2])
    run('conv', T.test_conv_fwd_dgrad_wgrad, torch.bfloat16, Cin, Cout, k, s, k // 2, rng.randint(6, 48), rng.randint(6, 64), Bn=rng.randint(1, 6))
# GEMM with the full epilogue under the DEFAULT dispatch (every kernel family gets its share of shapes, incl. the two-tiles-per-CU
# territory: 385..512 tiles of 160 x 128 / 96 x 128), and the dropout epilogue against the register-staged kernel
import torch.nn.functional as F


def gemm_case():
    M = rng.choice([rng.randint(1, 700), rng.randint(700, 12000), rng.randint(20000, 70000)])
    N = rng.choice([8 * rng.randint(1, 40), 64 * rng.randint(1, 16), 128 * rng.randint(1, 8)])
    K = rng.choice([8 * rng.randint(1, 40), 64 * rng.randint(1, 40)])
    if M * N > 40e6:
        N = 128 * rng.randint(1, 4)
    dtype = torch.bfloat16
    A, B = T.rnd(M, K, dtype=dtype, seed=1), T.rnd(N, K, dtype=dtype, seed=2)
    bias, rs = T.rnd(N, seed=5), T.rnd(M, seed=6)
    res, mask = T.rnd(M, N, dtype=dtype, seed=7), T.rnd(M, N, dtype=dtype, seed=8)
    ref0 = A.float() @ B.float().t()
    Cm = torch.empty(M, N, device=T.DEV, dtype=dtype)
    h.gemm(A, B, Cm, M, N, K, K, K, N)
    assert T.rel(Cm, ref0) < T.TOL[dtype], ('plain', M, N, K, T.rel(Cm, ref0))
    act, fn = rng.choice([(h.ACT_NONE, lambda x: x), (h.ACT_RELU, F.relu), (h.ACT_GELU, lambda x: F.gelu(x))])
    h.gemm(A, B, Cm, M, N, K, K, K, N, alpha=0.5, rowscale=rs, bias=bias, res=res, ldr=N, relu_mask=mask, ldm=N, act=act)
    r2 = fn(0.5 * ref0 * rs[:, None] + bias + res.float()) * (mask.float() > 0)
    assert T.rel(Cm, r2) < T.TOL[dtype], ('epilogue', M, N, K, act, T.rel(Cm, r2))
    c1, c2 = torch.empty(M, N, device=T.DEV, dtype=dtype), torch.empty(M, N, device=T.DEV, dtype=dtype)
    h.gemm(A, B, c1, M, N, K, K, K, N, drop_p=0.25, seed=77)
    m1, m2, m3 = h.set_option(h.OPT_PIPE, 0), h.set_option(h.OPT_GLDS, 0), h.set_option(h.OPT_SKINNY, 0)
    h.gemm(A, B, c2, M, N, K, K, K, N, drop_p=0.25, seed=77)
    h.set_option(h.OPT_PIPE, m1); h.set_option(h.OPT_GLDS, m2); h.set_option(h.OPT_SKINNY, m3)
    assert torch.equal(c1 == 0, c2 == 0) or float(((c1 == 0) != (c2 == 0)).float().mean()) < 1e-4, ('dropout pattern', M, N, K)
    assert T.rel(c1, c2.float()) < 2e-2, ('dropout values', M, N, K)


for it in range(rounds):
    run('gemm', gemm_case)
# attention (forward, dQ, dK/dV; strided fused-projection operands, key-padding masks, causal) and LayerNorm on random geometry
for it in range(rounds):
    dh = rng.choice([32, 48, 64, 96])
    H = rng.choice([8, 12, 16]) if dh != 96 else 8
    Sq, Sk = rng.randint(1, 320), rng.randint(2, 320)          # (Sk = 1: softmax is the constant 1, dQ = dK = 0 exactly: a relative error against ~0)
    causal = rng.random() < 0.2
    if causal:
        Sk = Sq = max(Sq, 2)                          # (causal 1 x 1 is the same degenerate case: the two r03 / r04 "failures")
    adt = rng.choice([torch.bfloat16, torch.bfloat16, torch.float32])
    if adt == torch.float32 and Sk * dh > 192 * 32 * 2:
        Sk = max(1, 192 * 32 * 2 // dh)              # fp32 ("precise") keeps K / V (backward: + Q) of a head in LDS as hi + lo bf16 pairs: capacity
        Sq = min(Sq, Sk) if causal else Sq
        Sk = Sq if causal else Sk
    # (causal + key padding is not a model shape: a padded key 0 leaves the first causal row without any key)
    run('attention', T.test_attention_fwd_bwd, adt, H, dh, Sq, Sk, causal, (not causal) and rng.random() < 0.5)
    run('layernorm', T.test_layernorm_fwd_bwd, rng.choice([torch.bfloat16, torch.float32]), rng.randint(1, 12000), 8 * rng.randint(1, 300))
    # round 4: the single-launch backward against the two launches (forced wherever instantiated), LayerNorm partial rows + grouped fold
    run('attention_bwd1', T.test_attention_bwd_single_launch_equals_the_two_launches, H, dh, Sq, Sk, causal, (not causal) and rng.random() < 0.5,
        rng.choice([0.0, 0.1, 0.25]))
    run('layernorm_fold', T.test_layernorm_bwd_partials_and_fold_group_equal_the_atomic_column_sums, rng.choice([torch.bfloat16, torch.float32]),
        rng.randint(1, 12000), 8 * rng.randint(1, 300), rng.choice([0.0, 0.1]))
# grouped weight gradients: random problem lists
import math
for it in range(max(rounds // 3, 2)):
    def one():
        probs, single = [], []
        for i in range(rng.randint(2, 9)):
            Cin, Cout = rng.choice([64, 128, 256, 512]), rng.choice([128, 256, 512])
            k = rng.choice([1, 3]); s = rng.choice([1, 2]); p = k // 2
            H, W, Bn = rng.randint(6, 40), rng.randint(6, 40), rng.randint(1, 9)
            OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
            x = T.nhwc(T.rnd(Bn, Cin, H, W, dtype=torch.bfloat16, seed=100 + i))
            dy = T.nhwc(T.rnd(Bn, Cout, OH, OW, dtype=torch.bfloat16, seed=200 + i))
            scale = T.rnd(Cout, seed=300 + i).abs() + 0.5
            g = torch.full((Cout, k, k, Cin), 0.25, device=T.DEV)
            g2 = g.clone()
            probs.append((x, dy, g, scale, Bn, H, W, Cin, Cin, OH, OW, Cout, k, k, s, s, p, p))
            h.conv2d(2, x, dy, g2, Bn, H, W, Cin, Cin, OH, OW, Cout, k, k, s, s, p, p, rowscale=scale)
            single.append(g2)
        h.conv_wgrad_group(probs)
        torch.cuda.synchronize()
        for q, ref in zip(probs, single):
            r = T.rel(q[2], ref)
            assert r < 1e-5, (q[4:], r)
    run('wgrad_group', one)
# round 5: the halo-image 3x3 tile kernel (stride 1, image width <= 47, enough pixels for the two-per-CU launch) on random image sizes
for it in range(max(rounds // 2, 3)):
    H, W = rng.randint(1, 47), rng.randint(1, 47)
    Cin, Cout = 64 * rng.randint(1, 8), 128 * rng.randint(1, 4)
    Bn = max(1, (rng.randint(31000, 42000) + H * W - 1) // (H * W))
    run('conv3x3_halo', T.test_conv3x3_halo_image_kernel, Cin, Cout, H, W, Bn, False)      # (whether a random shape fills the two-per-CU slots is not the point here)
# round 5: the fused in-projection attention and the projection + LayerNorm launch on random batch / sequence sizes, the small-M kernel's
# three tile shapes, the streaming 1x1 kernel (DMA-staged, swizzled weights) as a plain GEMM on every (K, N) it instantiates
for it in range(rounds):
    run('attention_qkv', T.test_attention_with_in_projection_equals_the_three_launches, rng.randint(1, 40), rng.randint(2, 320), rng.random() < 0.5,
        rng.choice([0.0, 0.1, 0.25]))
    run('linear_layernorm', T.test_linear_layernorm_one_launch_equals_gemm_then_layernorm, rng.randint(1, 12000), rng.choice([0.0, 0.1, 0.25]),
        rng.random() < 0.5, rng.random() < 0.8)
    prev = h.set_option(h.OPT_SKINNY, 2); prevg = h.set_option(h.OPT_GLDS, 0)
    run('skinny', T.test_skinny_gemm.__wrapped__ if hasattr(T.test_skinny_gemm, '__wrapped__') else T.test_skinny_gemm, h, rng.randint(1, 700), 8 * rng.randint(1, 300),
        8 * rng.randint(1, 400))
    run('skinny_bt', T.test_skinny_gemm_reduction_major_b.__wrapped__ if hasattr(T.test_skinny_gemm_reduction_major_b, '__wrapped__') else T.test_skinny_gemm_reduction_major_b,
        h, rng.randint(1, 3300), 8 * rng.randint(1, 100), 8 * rng.randint(1, 300))
    h.set_option(h.OPT_SKINNY, prev); h.set_option(h.OPT_GLDS, prevg)

    def c1s_case():
        K = rng.choice([64, 128, 256, 512])
        N = rng.choice([n for n in (64, 128, 256, 512, 1024, 2048) if n * (K + 8) <= 75 * 1024 * max(1, n // (512 if K <= 128 else 256 if K == 256 else 128))])
        M = rng.randint(1, 70000)
        A, B = T.rnd(M, K, dtype=torch.bfloat16, seed=3), T.rnd(N, K, dtype=torch.bfloat16, seed=4, scale=K ** -0.5)
        bias = T.rnd(N, seed=5)
        res = T.rnd(M, N, dtype=torch.bfloat16, seed=6) if rng.random() < 0.5 else None
        Cm = torch.full((M, N), float('nan'), device=T.DEV, dtype=torch.bfloat16)
        prevc = h.set_option(h.OPT_C1S, 2)
        h.set_option(h.OPT_C1S_LAUNCHES, 0)
        try:
            h.gemm(A, B, Cm, M, N, K, K, K, N, bias=bias, res=res, ldr=N, act=h.ACT_RELU)
        finally:
            used = h.set_option(h.OPT_C1S_LAUNCHES, 0)
            h.set_option(h.OPT_C1S, prevc)
        ref = F.relu(A.float() @ B.float().t() + bias + (res.float() if res is not None else 0))
        assert T.rel(Cm, ref) < T.TOL[torch.bfloat16], ('c1s', M, N, K, used, T.rel(Cm, ref))
    run('c1s_plain', c1s_case)
# exact-arithmetic checks (tests/exact_cases.py: integer operands, torch.equal against float64) on random shapes: GEMMs under the default
# dispatch and with each family forced, every layout, accumulate x split x {workspace, atomics}; convolutions forward / backward-data /
# weight gradient.  gemm_case / conv_case pick the integer ranges that keep the precondition; the check functions assert it.
import tests.exact_cases as E


def exact_gemm():
    M = rng.choice([rng.randint(1, 8), rng.randint(9, 700), rng.randint(700, 12000)])
    N = rng.choice([rng.randint(1, 300), 8 * rng.randint(1, 300), 128 * rng.randint(1, 16)])
    K = rng.choice([rng.randint(1, 400), 8 * rng.randint(1, 400), 64 * rng.randint(1, 48)])
    form = rng.choice(['plain', 'epi', 'drop', 'acc', 'precise'])
    la, lb = rng.choice(E.LAYOUTS)
    kw = dict(la=la, lb=lb, pad=rng.choice([0, 8]), seed=rng.randint(0, 1000))
    if form == 'epi':
        kw.update(epi=True, alpha=rng.choice(E.ALPHAS), act=rng.choice([E.ACT_NONE, E.ACT_RELU]), batch=rng.choice([1, 1, 3]))
    elif form == 'drop':
        kw.update(drop=True, act=rng.choice([E.ACT_NONE, E.ACT_RELU]))
    elif form == 'acc':
        kw.update(acc=True, split_k=rng.choice([1, 3, 8]), ws=rng.random() < 0.5, rowsum=kw['la'] == E.TRANS and kw['lb'] == E.TRANS)
    elif form == 'precise':
        kw.update(precise=rng.choice(['A', 'B']))
        K = min(K, 1000)                                   # 1000 * 2047 * 7 < 2^24
    else:
        kw.update(out=rng.choice([E.BF, E.F32]))
    opts = rng.choice([{}, {}, dict(GLDS=0, PIPE=0, SKINNY=0), dict(GLDS=2, PIPE=0, SKINNY=0), dict(GLDS=3, PIPE=0, SKINNY=0), dict(SKINNY=2, GLDS=0),
                       dict(PIPE=100 + rng.randint(0, 7), SKINNY=0), dict(C1S=2)])
    prev = {n: h.set_option(getattr(h, 'OPT_' + n), v) for n, v in opts.items()}
    try:
        E.check_gemm(h, E.gemm_case('fuzz', M, N, K, **kw))
    finally:
        for n, v in prev.items():
            h.set_option(getattr(h, 'OPT_' + n), v)


def exact_conv():
    Cin, Cout = rng.choice([64, 128, 256, 512]), rng.choice([64, 128, 256, 512])
    k = rng.choice([1, 3])
    opts = rng.choice([{}, {}, dict(GLDS=0, PIPE=0, SKINNY=0), dict(GLDS=rng.choice([2, 3]), PIPE=0), dict(PIPE=100 + rng.randint(0, 5)), dict(C1S=2), dict(C3S=2),
                       dict(C3_HALO=2), dict(GLDS_WGRAD=rng.choice([0, 2]))])
    c = E.conv_case('fuzz', Cin, Cout, k, rng.choice([1, 2]), k // 2, rng.randint(6, 48), rng.randint(6, 64), rng.randint(1, 6), seed=rng.randint(0, 1000),
                    res=rng.random() < 0.5, mask=rng.random() < 0.5, split_k=rng.choice([0, 0, 4]))
    prev = {n: h.set_option(getattr(h, 'OPT_' + n), v) for n, v in opts.items()}
    try:
        E.check_conv(h, c)
    finally:
        for n, v in prev.items():
            h.set_option(getattr(h, 'OPT_' + n), v)


for it in range(rounds):
    run('exact_gemm', exact_gemm)
    run('exact_gemm', exact_gemm)
    run('exact_conv', exact_conv)
print('fuzz done: %d failures (%d attention shapes refused as out of range)' % (len(fails), out_of_range))
for f in fails:
    print(f)
