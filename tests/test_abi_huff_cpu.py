"""C-ABI checks of libgpv_huff.so that need no GPU: the library exports exactly what include/gpv_huff.h declares and
gpv1_amd.hip_huff.EXPORTS lists, the ctypes mirrors have the C layout (a gcc-compiled probe, as tests/test_abi_cpu.py does for
libgpv_hip.so), the header's constants are the rule module's, and bad extents are refused before any launch."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gpv_huff.h')


def declared():
    src = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r'\bint\s+(gpv_\w+)\s*\(', src)))


def lib_path():
    import gpv1_amd.hip_huff as hh
    if not os.path.exists(hh._LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hh._LIB_PATH


def test_library_exports_exactly_the_declared_entry_points():
    import gpv1_amd.hip_huff as hh
    names = declared()
    assert names == ['gpv_huff_decode', 'gpv_huff_prepare', 'gpv_huff_workspace_bytes'] == sorted(hh.EXPORTS)
    out = subprocess.run(['nm', '-D', '--defined-only', lib_path()], capture_output=True, text=True, check=True).stdout
    exported = sorted({l.split()[-1] for l in out.splitlines() if l.split() and l.split()[-1].startswith('gpv_')})
    assert exported == names
    und = subprocess.run(['nm', '-D', '--undefined-only', lib_path()], capture_output=True, text=True).stdout
    assert not re.search(r'\bgetenv\b', und), 'libgpv_huff.so reads the environment'


def test_the_seven_libraries_are_listed_by_the_makefile():
    mk = open(os.path.join(ROOT, 'gpv-1_amd', 'csrc', 'Makefile')).read()
    all_line = re.search(r'^all:(.*)$', mk, re.M).group(1).split()
    assert len(all_line) == 7 and 'libgpv_huff.so' in all_line
    assert re.search(r'^HUFF_SRCS\s*=\s*jpeg_huff\.hip$', mk, re.M) and 'HUFF_HDRS' in mk and 'HUFF_OBJS' in mk
    assert 'libgpv_huff.so' in re.search(r'^clean:\n\t(.*)$', mk, re.M).group(1)


def test_ctypes_structs_match_the_c_layout(tmp_path):
    import gpv1_amd.hip_huff as hh
    pairs = (('gpv_huff_table', hh.HuffTable), ('gpv_huff_desc', hh.HuffDesc))
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{HEADER}"', 'int main(void) {']
    for cname, cls in pairs:
        prog.append(f'  printf("{cname} %zu", sizeof({cname}));')
        for f, _ in cls._fields_:
            prog.append(f'  printf(" %zu", offsetof({cname}, {f}));')
        prog.append('  printf("\\n");')
    prog += ['  return 0;', '}']
    c = tmp_path / 'probe.c'
    c.write_text('\n'.join(prog))
    exe = tmp_path / 'probe'
    subprocess.run(['gcc', '-std=c99', '-o', str(exe), str(c)], check=True)
    lines = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()
    for (cname, cls), line in zip(pairs, lines):
        vals = line.split()
        assert vals[0] == cname
        assert int(vals[1]) == ctypes.sizeof(cls), (cname, vals[1], ctypes.sizeof(cls))
        assert [int(v) for v in vals[2:]] == [getattr(cls, f).offset for f, _ in cls._fields_], cname
    assert ctypes.sizeof(hh.HuffDesc) % 8 == 0                                    # the kernel copies it to LDS in 8-byte words


def test_header_constants_are_the_rule_modules():
    import gpv1_amd.hip_huff as hh
    from gpv1_amd import jpeg_entropy as E
    src = open(HEADER).read()
    const = {k: int(eval(v)) for k, v in re.findall(r'#define (GPV_HUFF_\w+) (\([^)]*\)|\d+)', src)}
    assert (const['GPV_HUFF_LOOK'], const['GPV_HUFF_MIN_S'], const['GPV_HUFF_MAX_S'], const['GPV_HUFF_MAX_STREAM']) == (E.LOOK, E.MIN_S, E.MAX_S, E.MAX_STREAM)
    assert (const['GPV_HUFF_ERR_CODE'], const['GPV_HUFF_ERR_SHORT'], const['GPV_HUFF_ERR_EXTENT']) == (E.ERR_CODE, E.ERR_SHORT, E.ERR_EXTENT)
    assert (const['GPV_HUFF_ROUTE_DEVICE'], const['GPV_HUFF_ROUTE_HOST']) == (hh.ROUTE_DEVICE, hh.ROUTE_HOST)
    # the workspace holds two states (8 bytes), two counts, two change words and one first-block word per subsequence
    assert const['GPV_HUFF_WS_PER_SUB'] >= 2 * 8 + 5 * 4 and const['GPV_HUFF_WS_PER_SUB'] % 16 == 0


def test_bad_extents_are_refused_before_a_launch():
    """the C entry points return hipErrorInvalidValue (1) without touching the device; the Python mirror raises ValueError first"""
    import gpv1_amd.hip_huff as hh
    lib = ctypes.CDLL(lib_path())
    lib.gpv_huff_workspace_bytes.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.gpv_huff_decode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p]
    n = ctypes.c_int64(-1)
    assert lib.gpv_huff_workspace_bytes(2, 1024, 10000, ctypes.byref(n)) == 0 and n.value == 2 * (10000 // 1024 + 1) * 48
    for B, S, bits in ((0, 1024, 100), (1, 32, 100), (1, 8192, 100), (1, 1000, 100), (1, 1024, -1), (1, 1024, (1 << 30) + 1)):
        assert lib.gpv_huff_workspace_bytes(B, S, bits, ctypes.byref(n)) == 1, (B, S, bits)
    assert lib.gpv_huff_workspace_bytes(1, 1024, 100, None) == 1
    assert lib.gpv_huff_decode(None, 1, 1024, 100, 16, 1 << 20, None) == 1        # no descriptors
    assert lib.gpv_huff_decode(16, 1, 1024, 100, None, 1 << 20, None) == 1        # no workspace
    assert lib.gpv_huff_decode(16, 1, 1000, 100, 16, 1 << 20, None) == 1          # subsequence length
    assert lib.gpv_huff_decode(16, 1, 1024, 100, 16, 47, None) == 1               # workspace too small
    assert lib.gpv_huff_decode(16, 1, 1024, 100, 24, 1 << 20, None) == 1          # workspace not 16-byte aligned
    with pytest.raises(ValueError):
        hh.workspace_bytes(1, 1000, 100)
    with pytest.raises(ValueError):
        hh.workspace_bytes(0, 1024, 100)
    with pytest.raises(ValueError):
        hh.workspace_bytes(1, 1024, -5)


def test_decoder_keyword_is_validated_and_the_default_is_the_host_path():
    from gpv1_amd.jpeg import DeviceJpegDecoder
    assert DeviceJpegDecoder(device='cpu', threads=1).entropy == 'host'
    dec = DeviceJpegDecoder(device='cpu', threads=1, entropy='device')
    assert (dec.entropy, dec.subseq_bits) == ('device', 1024) and dec.stats == {'device': 0, 'host': 0, 'bytes_uploaded': 0}
    with pytest.raises(ValueError):
        DeviceJpegDecoder(device='cpu', threads=1, entropy='gpu')
    with pytest.raises(ValueError):
        DeviceJpegDecoder(device='cpu', threads=1, entropy='device', subseq_bits=100)
