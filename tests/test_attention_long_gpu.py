"""Attention beyond 320 keys (attention.hip attn_long_kernel / attn_kvl_kernel), kernel level, against an independent float64
reference on the host over the FULL tensors (attn_ref of test_kernels_gpu in float64).  Tolerances are test_attention_fwd_bwd's:
forward 3e-5 (precise) / 1.2e-2 (bf16) of max|ref|, backward 1e-4 / 2.5e-2.  Every case with more than 320 keys was refused
(hipErrorInvalidValue) before the streaming kernels existed."""
import math

import numpy as np
import pytest
import torch

from tests.test_kernels_gpu import attn_ref, _attention_keep_mask, _epoch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
FTOL = {torch.float32: 3e-5, torch.bfloat16: 1.2e-2}
BTOL = {torch.float32: 1e-4, torch.bfloat16: 2.5e-2}
LTOL = {torch.float32: 1e-4, torch.bfloat16: 1e-2}
DTYPES = [torch.float32, torch.bfloat16]


def hip():
    import gpv1_amd.hip as h
    h.lib()
    return h


def rel(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).abs().max() / ref.abs().max().clamp_min(1e-30)).item()


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def run(h, dtype, qkv, H, dh, Sq, Sk, kpm=None, causal=False, do=None, drop_p=0.0, seed=0):
    """q / k / v = column slices of one [B, max(Sq, Sk), 3 D] buffer (row stride 3 D); returns o, lse, dq, dk, dv (dq.. None without do)"""
    Bn, D = qkv.shape[0], H * dh
    buf = qkv.to(DEV).to(dtype)
    q, k, v = buf[:, :Sq, :D], buf[:, :Sk, D:2 * D], buf[:, :Sk, 2 * D:]
    st = ((buf.stride(0), buf.stride(1)),) * 3 + ((Sq * D, D),)
    scale = 1.0 / math.sqrt(dh)
    km = None if kpm is None else kpm.to(DEV)
    o = torch.full((Bn, Sq, D), float('nan'), device=DEV, dtype=dtype)
    lse = torch.full((Bn, H, Sq), float('nan'), device=DEV)
    h.attention_fwd(q, k, v, o, st, Bn, H, Sq, Sk, dh, scale, kpm=km, causal=causal, drop_p=drop_p, seed=seed, lse=lse)
    if do is None:
        return o, lse, None, None, None
    dob = do.to(DEV).to(dtype).contiguous()
    g = torch.full_like(buf, float('nan'))
    dq, dk, dv = g[:, :Sq, :D], g[:, :Sk, D:2 * D], g[:, :Sk, 2 * D:]
    h.attention_bwd(q, k, v, o, dob, dq, dk, dv, st, (Sq * D, D), Bn, H, Sq, Sk, dh, scale, kpm=km, causal=causal, drop_p=drop_p,
                    seed=seed, lse=lse)
    torch.cuda.synchronize()
    return o, lse, dq, dk, dv


def reference(dtype, qkv, H, dh, Sq, Sk, kpm, causal, do):
    """float64 on the host from the inputs as the kernel sees them (rounded to dtype)"""
    D = H * dh
    x = qkv.to(dtype).double()
    q, k, v = (t.contiguous().requires_grad_(True) for t in (x[:, :Sq, :D], x[:, :Sk, D:2 * D], x[:, :Sk, 2 * D:]))
    o, lse = attn_ref(q, k, v, H, kpm, causal, 1.0 / math.sqrt(dh))
    gq, gk, gv = torch.autograd.grad(o, (q, k, v), do.to(dtype).double())
    return o.detach(), lse.detach(), gq, gk, gv


def check(dtype, got, want, tag=''):
    o, lse, dq, dk, dv = got
    ro, rl, gq, gk, gv = want
    for name, a, b in (('o', o, ro), ('dq', dq, gq), ('dk', dk, gk), ('dv', dv, gv)):
        assert torch.isfinite(a.float()).all(), (tag, name)
    e = {'o': rel(o, ro), 'lse': rel(lse, rl), 'dq': rel(dq, gq), 'dk': rel(dk, gk), 'dv': rel(dv, gv)}
    assert e['o'] < FTOL[dtype] and e['lse'] < LTOL[dtype], (tag, e)
    assert e['dq'] < BTOL[dtype] and e['dk'] < BTOL[dtype] and e['dv'] < BTOL[dtype], (tag, e)


def key_mask(Bn, Sk):
    kpm = torch.zeros(Bn, Sk, dtype=torch.uint8)
    kpm[0, ::5] = 1
    if Bn > 1:
        kpm[1, Sk - Sk // 3:] = 1
    return kpm


def parity(dtype, Bn, H, dh, Sq, Sk, use_kpm=False, causal=False, seed=0):
    h = hip()
    D = H * dh
    qkv = rnd(Bn, max(Sq, Sk), 3 * D, seed=seed)
    do = rnd(Bn, Sq, D, seed=seed + 1)
    kpm = key_mask(Bn, Sk) if use_kpm else None
    got = run(h, dtype, qkv, H, dh, Sq, Sk, kpm=kpm, causal=causal, do=do)
    check(dtype, got, reference(dtype, qkv, H, dh, Sq, Sk, kpm, causal, do), (Bn, H, dh, Sq, Sk, use_kpm, causal))


LONG = [  # Bn, H, dh, Sq, Sk, kpm, causal: Sq in {1, 100, Sk} per Sk, every dh at two key lengths, one causal case
    (2, 8, 32, 1, 321, False, False), (2, 8, 96, 100, 321, True, False), (2, 8, 32, 321, 321, True, False),
    (2, 4, 48, 1, 400, True, False), (2, 4, 64, 100, 400, False, False), (2, 4, 48, 400, 400, True, False),
    (2, 4, 64, 400, 400, False, True),
    (1, 2, 96, 1, 850, False, False), (1, 2, 48, 100, 850, True, False), (1, 2, 96, 850, 850, True, False),
    (1, 2, 64, 1, 1201, False, False), (1, 2, 32, 100, 1201, True, False), (1, 2, 64, 1201, 1201, True, False),
    (1, 1, 32, 1, 4100, False, False), (1, 1, 32, 100, 4100, True, False), (1, 1, 32, 4100, 4100, False, False)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Bn,H,dh,Sq,Sk,use_kpm,causal', LONG)
def test_long_attention_fwd_bwd_vs_float64(dtype, Bn, H, dh, Sq, Sk, use_kpm, causal):
    parity(dtype, Bn, H, dh, Sq, Sk, use_kpm, causal, seed=Sq + Sk + dh)


@pytest.mark.parametrize('dtype', DTYPES)
def test_321_keys_with_the_last_masked_equal_the_320_key_short_path(dtype):
    """the first length past the short kernels against the last one they serve: key 320 masked is the 320-key problem"""
    h = hip()
    Bn, H, dh, S = 2, 8, 32, 321
    D = H * dh
    qkv = rnd(Bn, S, 3 * D, seed=5)
    do = rnd(Bn, 300, D, seed=6)
    kpm = torch.zeros(Bn, S, dtype=torch.uint8)
    kpm[:, 320] = 1
    a = run(h, dtype, qkv, H, dh, 300, 321, kpm=kpm, do=do)
    b = run(h, dtype, qkv[:, :320], H, dh, 300, 320, do=do)
    assert rel(a[0], b[0]) < FTOL[dtype] and rel(a[1], b[1]) < LTOL[dtype]
    assert rel(a[2], b[2]) < BTOL[dtype], rel(a[2], b[2])
    assert rel(a[3][:, :320], b[3]) < BTOL[dtype] and rel(a[4][:, :320], b[4]) < BTOL[dtype]
    assert a[3][:, 320].float().abs().max() == 0 and a[4][:, 320].float().abs().max() == 0     # the masked key gets no gradient


def test_precise_mode_past_the_short_kernels_lds():
    """fp32, dh = 64, 250 keys: the short forward holds K / V (141 KB of LDS), its dQ would need 215 KB -- refused until the
    streaming backward took it"""
    parity(torch.float32, 2, 4, 64, 250, 250, use_kpm=True, seed=250)
    parity(torch.float32, 2, 4, 64, 60, 250, seed=251)


def forced(dtype, qkv, Bn, H, dh, S, kpm=None, tag=''):
    h = hip()
    D = H * dh
    do = rnd(Bn, S, D, seed=99)
    got = run(h, dtype, qkv, H, dh, S, S, kpm=kpm, do=do)
    check(dtype, got, reference(dtype, qkv, H, dh, S, S, kpm, False, do), tag)


def bf16_exact(x):
    return x.to(torch.bfloat16).double()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('key', [1190, 700, 3])
def test_online_softmax_rescale_at_a_spiked_key(dtype, key):
    """one key row = 4 x a query row: that query's running max jumps at the key's tile -- the last tile, a middle one, the first"""
    Bn, H, dh, S = 1, 2, 32, 1201
    D = H * dh
    qkv = rnd(Bn, S, 3 * D, seed=key)
    qkv[:, :, :2 * D] = bf16_exact(qkv[:, :, :2 * D])
    for qi in (0, 517, 1200):
        qkv[0, key, D:2 * D] = 4 * qkv[0, qi, :D]
        forced(dtype, qkv, Bn, H, dh, S, tag=(key, qi))


@pytest.mark.parametrize('dtype', DTYPES)
def test_scores_near_plus_minus_80(dtype):
    """scale Q K^T up to |80|: exp without the max subtracted overflows fp32 partial sums"""
    Bn, H, dh, S = 1, 2, 32, 850
    D = H * dh
    qkv = rnd(Bn, S, 3 * D, seed=80)
    x = qkv.view(Bn, S, 3, H, dh)
    s = torch.einsum('bqhd,bkhd->bhqk', x[:, :, 0], x[:, :, 1]) / math.sqrt(dh)
    f = math.sqrt(80.0 / s.abs().max().item())
    qkv[:, :, :2 * D] = bf16_exact(qkv[:, :, :2 * D] * f)
    xs = qkv.view(Bn, S, 3, H, dh)
    smax = (torch.einsum('bqhd,bkhd->bhqk', xs[:, :, 0], xs[:, :, 1]) / math.sqrt(dh)).abs().max().item()
    assert 70 < smax < 90, smax
    forced(dtype, qkv, Bn, H, dh, S)


@pytest.mark.parametrize('dtype', DTYPES)
def test_first_128_keys_masked(dtype):
    """the running max starts at -inf for every query and stays there through the first tile(s)"""
    Bn, H, dh, S = 2, 2, 32, 400
    kpm = torch.zeros(Bn, S, dtype=torch.uint8)
    kpm[:, :128] = 1
    forced(dtype, rnd(Bn, S, 3 * H * dh, seed=128), Bn, H, dh, S, kpm=kpm)


@pytest.mark.parametrize('dtype', DTYPES)
def test_padding_layouts_of_a_640x640_pair(dtype):
    """nested_tensor_from_tensor_list pads a 480x640 and a 640x480 image to 640x640 (20 x 20 C5 cells, 400 tokens): the first
    loses its last 5 rows (the last 100 keys), the second its last 5 columns (5 of every 20 keys)"""
    Bn, H, dh, S = 2, 8, 32, 400
    kpm = torch.zeros(Bn, S, dtype=torch.uint8)
    kpm[0, 300:] = 1
    kpm[1] = (torch.arange(S) % 20 >= 15).to(torch.uint8)
    forced(dtype, rnd(Bn, S, 3 * H * dh, seed=640), Bn, H, dh, S, kpm=kpm)


@pytest.mark.parametrize('Sk', [400, 1201])
def test_long_dropout_mask_equals_the_specification(Sk):
    """the keep pattern of the streaming forward is tests/dropout_ref.keep_attention bit for bit (one-hot V probes)"""
    from tests import dropout_ref as R
    h = hip()
    Bn, H, dh, drop, seed = 2, 2, 32, 0.1, 4242
    keep = _attention_keep_mask(h, Bn, H, dh, Sk, Sk, drop, seed).cpu().numpy()
    ref = R.keep_attention(R.eff_seed(seed, _epoch()), Bn, H, Sk, Sk, drop)
    assert np.array_equal(keep, ref), (int((keep != ref).sum()), keep.mean(), ref.mean())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('Sq,Sk', [(400, 400), (100, 1201)])
def test_long_dropout_backward_against_fp32_autograd_with_that_mask(dtype, Sq, Sk):
    """forward and backward with dropout on, against autograd of dropout(softmax(Q K^T)) V fed the specification's keep mask"""
    from tests import dropout_ref as R
    h = hip()
    Bn, H, dh, drop, seed = 2, 4, 32, 0.1, 777
    D = H * dh
    keep = torch.from_numpy(R.keep_attention(R.eff_seed(seed, _epoch()), Bn, H, Sq, Sk, drop)).double()
    qkv = rnd(Bn, max(Sq, Sk), 3 * D, seed=Sk)
    do = rnd(Bn, Sq, D, seed=Sk + 1)
    kpm = key_mask(Bn, Sk)
    o, lse, dq, dk, dv = run(h, dtype, qkv, H, dh, Sq, Sk, kpm=kpm, do=do, drop_p=drop, seed=seed)
    x = qkv.to(dtype).double()
    q, k, v = (t.contiguous().requires_grad_(True) for t in (x[:, :Sq, :D], x[:, :Sk, D:2 * D], x[:, :Sk, 2 * D:]))
    sc = (q.view(Bn, Sq, H, dh).transpose(1, 2) @ k.view(Bn, Sk, H, dh).transpose(1, 2).transpose(-1, -2)) / math.sqrt(dh)
    sc = sc.masked_fill(kpm[:, None, None, :].bool(), float('-inf'))
    pd = sc.softmax(-1) * keep / (1 - float(np.float32(drop)))
    oref = (pd @ v.view(Bn, Sk, H, dh).transpose(1, 2)).transpose(1, 2).reshape(Bn, Sq, D)
    assert rel(o, oref) < (1e-4 if dtype == torch.float32 else 1.5e-2), rel(o, oref)
    gq, gk, gv = torch.autograd.grad(oref, (q, k, v), do.to(dtype).double())
    for name, got, want in (('dq', dq, gq), ('dk', dk, gk), ('dv', dv, gv)):
        assert torch.isfinite(got.float()).all(), name
        assert rel(got, want) < BTOL[dtype], (name, rel(got, want))
