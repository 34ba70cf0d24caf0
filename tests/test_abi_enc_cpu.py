"""C-ABI checks of the extension library libgpv_enc.so that need no GPU: what tests/test_abi_cpu.py checks for the seven libraries
of gpv1_amd._native.LIBRARIES (exports == header == binding, prototypes, struct layout, no environment reads), that the seven stay
seven, that the Makefile builds the extension by a target of its own, the header's constants, and the refusal of bad extents."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry
from gpv1_amd import _native
from tests import abi_probe as probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 'enc'
PINNED = ['gpv_enc_encode', 'gpv_enc_header', 'gpv_enc_workspace_bytes']
STRUCTS = {'gpv_enc_desc': 'EncDesc'}
SIGNATURES = {'gpv_enc_workspace_bytes': 'iqP', 'gpv_enc_encode': 'PiiiPqPqPPP', 'gpv_enc_header': 'iiiiPP'}


def module():
    import importlib
    return importlib.import_module(_native.module_name(KEY))


def built():
    if not os.path.exists(module()._LIB_PATH):
        entry.build()
    return module()._LIB_PATH


def test_the_seven_libraries_stay_seven_and_the_extension_has_a_table_of_its_own():
    assert len(_native.LIBRARIES) == 7 and KEY not in _native.LIBRARIES
    assert list(_native.EXTENSIONS) == [KEY]
    l = _native.EXTENSIONS[KEY]
    assert (l.file, l.header, l.prefix) == ('libgpv_enc.so', 'gpv_enc.h', 'gpv_enc_')
    assert _native.module_name(KEY) == 'gpv1_amd.hip_enc'
    assert _native.lib_path(KEY).endswith('gpv-1_amd/csrc/libgpv_enc.so') and _native.header_path(KEY).endswith('include/gpv_enc.h')
    assert _native.lib_path('huff').endswith('libgpv_huff.so')                # the loader still finds the seven


def test_makefile_links_the_extension_by_its_own_target():
    csrc = os.path.join(ROOT, 'gpv-1_amd', 'csrc')
    def links(target):
        dry = subprocess.run(['make', '-n', '-B', '-C', csrc, target], capture_output=True, text=True, check=True).stdout.splitlines()
        return {l.split()[-1]: l.split() for l in dry if ' -shared ' in l}
    assert sorted(links('all')) == sorted(l.file for l in _native.LIBRARIES.values()) and len(links('all')) == 7
    ext = links('extensions')
    assert list(ext) == ['libgpv_enc.so'] and 'jpeg_enc.o' in ext['libgpv_enc.so']
    compile_line = [l for l in subprocess.run(['make', '-n', '-B', '-C', csrc, 'extensions'], capture_output=True, text=True, check=True).stdout.splitlines()
                    if ' -c jpeg_enc.hip' in l]
    assert len(compile_line) == 1 and '-ffp-contract=off' in compile_line[0] and '--offload-arch=gfx950' in compile_line[0]
    clean = subprocess.run(['make', '-n', '-C', csrc, 'clean'], capture_output=True, text=True, check=True).stdout.split()
    assert 'libgpv_enc.so' in clean and 'jpeg_enc.o' in clean


def test_library_exports_exactly_the_declared_entry_points():
    l, mod = _native.EXTENSIONS[KEY], module()
    names = entry._declared(_native.header_path(KEY), l.prefix)
    assert names == PINNED == sorted(mod.EXPORTS)
    path = built()
    assert entry._exported(path) == names
    for other in _native.LIBRARIES.values():                 # no entry point of the seven carries this prefix, and none here theirs
        assert not other.prefix.startswith(l.prefix), other.prefix
        if other.key != 'hip':
            assert not any(n.startswith(other.prefix) for n in names), other.prefix
    hot = entry._declared(_native.header_path('hip'), 'gpv_')
    assert not any(n.startswith(l.prefix) for n in hot)
    assert not re.search(r'\bgetenv\b', probe.imports(path)), 'libgpv_enc.so reads the environment'


def test_argtypes_are_the_header_prototypes():
    mod = module()
    src = entry._header_source(_native.header_path(KEY))
    protos = {}
    for name, params in re.findall(r'\bint\s+(gpv_enc_\w+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = ''.join('P' if '*' in p else probe._C_CLASS[' '.join(p.replace('const ', ' ').split()[:-1])] for p in params.split(','))
    assert protos == SIGNATURES
    built()
    for name, sig in protos.items():
        fn = getattr(mod.lib(), name)
        assert fn.restype is ctypes.c_int and probe.argtypes_classes(fn) == sig, name


def test_ctypes_structs_match_the_c_layout(tmp_path):
    mod = module()
    pairs = [(cname, getattr(mod, mirror)) for cname, mirror in STRUCTS.items()]
    layout = probe.c_layout(tmp_path, [_native.header_path(KEY)], pairs)
    for cname, cls in pairs:
        assert layout[cname] == probe.ctypes_layout(cls), (cname, layout[cname], probe.ctypes_layout(cls))
    mirrors = {n for n, v in vars(mod).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == mod.__name__}
    assert mirrors == set(STRUCTS.values())
    assert ctypes.sizeof(mod.EncDesc) == 80                  # the workspace formula of the header counts on it


def test_header_constants_are_the_mirrors():
    mod = module()
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
