"""C-ABI checks of libgpv_enc.so that need no GPU and are its own: the header's constants, the size the workspace formula counts on,
the host-only header entry point and the refusal of bad extents.  (Exports, prototypes, struct layout, Makefile: tests/test_abi_cpu.py.)"""
import ctypes
import re

import pytest

from gpv1_amd import _native
from tests import abi_probe as probe

KEY = 'enc'


def module():
    return probe.module(KEY)


def built():
    return probe.built(KEY)


def test_header_constants_are_the_mirrors():
    mod = module()
    assert ctypes.sizeof(mod.EncDesc) == 80                  # the workspace formula of the header counts on it
    from gpv1_amd import jpeg_encode as E
    src = open(_native.header_path(KEY)).read()
    const = {k: int(eval(v)) for k, v in re.findall(r'#define (GPV_ENC_\w+) (\([^)]*\)|\d+)', src)}
    assert (const['GPV_ENC_SRC_U8'], const['GPV_ENC_SRC_BF16'], const['GPV_ENC_SRC_F32']) == (mod.SRC_U8, mod.SRC_BF16, mod.SRC_F32)
    assert {k: const['GPV_ENC_' + k.replace(':', '')] for k in mod.SUBSAMPLING} == mod.SUBSAMPLING
    assert (const['GPV_ENC_MAX_BOXES'], const['GPV_ENC_MAX_BLOCKS'], const['GPV_ENC_MAX_TOTAL_BLOCKS']) == (mod.MAX_BOXES, mod.MAX_BLOCKS, mod.MAX_TOTAL_BLOCKS)
    assert (const['GPV_ENC_HEADER_BYTES'], const['GPV_ENC_BLOCK_BYTES'], const['GPV_ENC_STATUS_CAPACITY']) == (mod.HEADER_BYTES, mod.BLOCK_BYTES, mod.STATUS_CAPACITY)
    assert mod.MAX_BOXES == E.MAX_BOXES and mod.HEADER_BYTES == len(E.header(8, 8, 90, '4:2:0'))
    assert mod.BLOCK_BYTES * 8 >= 20 + 63 * 26               # the most bits a block can code to
    for H, W, s in ((1, 1, '4:2:0'), (17, 33, '4:2:0'), (33, 17, '4:2:2'), (480, 640, '4:4:4')):
        assert mod.block_count(H, W, s) == sum(1 for _ in _scan_blocks(H, W, s))


def _scan_blocks(H, W, subsampling):
    from gpv1_amd import jpeg_encode as E
    hs, vs = E.subsampling_factors(subsampling)
    for _ in range(-(-(-(-H // vs)) // 8) * -(-(-(-W // hs)) // 8)):
        yield from range(hs * vs + 2)


def test_the_host_only_header_entry_point_writes_the_rules_header():
    from gpv1_amd import jpeg_encode as E
    mod = module()
    built()
    for H, W, q, s in ((1, 1, 90, '4:2:0'), (480, 640, 75, '4:2:2'), (3, 65535, 5, '4:4:4'), (65535, 2, 100, '4:2:0')):
        assert mod.header(H, W, q, s) == E.header(H, W, q, s)
    for H, W, q in ((0, 1, 90), (1, 65536, 90), (1, 1, 0), (1, 1, 101)):
        with pytest.raises(ValueError):
            mod.header(H, W, q, '4:2:0')


def test_bad_extents_are_refused_before_a_launch():
    """the C entry points return hipErrorInvalidValue (1) without touching a device; the Python mirror raises ValueError first"""
    mod = module()
    lib = ctypes.CDLL(built())
    lib.gpv_enc_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.gpv_enc_encode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                   ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    lib.gpv_enc_header.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    n = ctypes.c_int64(-1)
    assert lib.gpv_enc_workspace_bytes(2, 100, ctypes.byref(n)) == 0 and n.value == 128 * 2 + 344 * 100 + 32
    for B, blocks in ((0, 10), (2, 1), (1, (1 << 24) + 1), (-1, 5)):
        assert lib.gpv_enc_workspace_bytes(B, blocks, ctypes.byref(n)) == 1, (B, blocks)
    assert lib.gpv_enc_workspace_bytes(1, 10, None) == 1

    def desc(**kw):
        d = (mod.EncDesc * 1)()
        d[0].src, d[0].H, d[0].W, d[0].pitch, d[0].kind = 4096, 16, 16, 16, mod.SRC_U8
        for k, v in kw.items():
            setattr(d[0], k, v)
        return d

    def call(d, B=1, quality=90, sub=2, ws=4096, ws_bytes=1 << 20, out=4096, cap=1 << 16, sizes=4096, status=4096):
        return lib.gpv_enc_encode(d, B, quality, sub, ws, ws_bytes, out, cap, sizes, status, None)
    good = desc()
    for bad in (desc(H=0), desc(H=65536), desc(W=0), desc(W=65536), desc(pitch=15), desc(nboxes=33), desc(nboxes=-1), desc(src=None),
                desc(nboxes=1), desc(kind=3), desc(kind=mod.SRC_BF16, src=4100), desc(kind=mod.SRC_F32, src=4104),
                desc(H=65535, W=65535)):
        assert call(bad) == 1
    assert call(None) == 1 and call(good, B=0) == 1
    assert call(good, quality=0) == 1 and call(good, quality=101) == 1 and call(good, sub=3) == 1 and call(good, sub=-1) == 1
    assert call(good, ws=None) == 1 and call(good, ws=4104) == 1                 # no workspace, not 16-byte aligned
    need = 128 + 344 * mod.block_count(16, 16, '4:2:0') + 32
    assert call(good, ws_bytes=need - 1) == 1                                    # one byte short
    assert call(good, out=None) == 1 and call(good, cap=0) == 1 and call(good, sizes=None) == 1 and call(good, status=None) == 1
    assert (good[0].block_base, good[0].nblocks) == (0, 0)                       # a refused call has written nothing
    with pytest.raises(ValueError):
        mod.workspace_bytes(0, 10)
    with pytest.raises(ValueError):
        mod.workspace_bytes(4, 3)
    with pytest.raises(ValueError):
        mod.block_count(8, 8, '4:1:1')


def test_encoder_refuses_to_run_without_the_library(monkeypatch, tmp_path):
    """no CPU / eager fallback: a missing library is an error"""
    mod = module()
    monkeypatch.setattr(mod, '_LIB', None)
    monkeypatch.setattr(mod, '_LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(RuntimeError, match='no CPU/eager fallback'):
        mod.lib()
