"""C-ABI checks that need no GPU, for every native library of gpv1_amd._native.LIBRARIES: it loads, exports exactly the entry points
its public header declares and its binding module lists, the ctypes mirrors have the C layout (sizes and field offsets, via a
gcc-compiled probe), the argtypes are the header's prototypes, the constants of gpv-1_amd/hip.py are the header's, and the Makefile
builds exactly the table's libraries, each from its own sources with its own flags.

A new library adds rows to PINNED, SIGNATURES and (if it has structs) STRUCTS below; the test bodies stay as they are."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from tests import abi_probe as probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'gpv_hip.h')
# the pinned export lists (the hot path's by its count: hip.EXPORTS spells the names)
PINNED = {'hip': 52,
          'eval': ['gpv_eval_det_ap'],
          'cap': ['gpv_cap_scores'],
          'match': ['gpv_match_boxes', 'gpv_match_lsap', 'gpv_match_set_loss'],
          'health': ['gpv_health_commit', 'gpv_health_stats'],
          'beam': ['gpv_beam_reorder', 'gpv_beam_step'],
          'huff': ['gpv_huff_decode', 'gpv_huff_prepare', 'gpv_huff_workspace_bytes'],
          'enc': ['gpv_enc_encode', 'gpv_enc_header', 'gpv_enc_workspace_bytes'],
          'phrase': ['gpv_phrase_step']}
NO_GETENV = ('hip', 'huff', 'enc', 'phrase')          # libraries that must not read the environment
FP_CONTRACT_OFF = ('eval', 'cap', 'match', 'health', 'beam', 'enc', 'phrase')      # compiled with -ffp-contract=off: a host rule rounds every operation
# C struct -> its ctypes mirror in the binding module
STRUCTS = {'hip': {'gpv_gemm_args': 'GemmArgs', 'gpv_conv_args': 'ConvArgs', 'gpv_attn_args': 'AttnArgs', 'gpv_tt_problem': 'TTProblem',
                   'gpv_fold_problem': 'FoldProblem', 'gpv_tc_problem': 'TCProblem', 'gpv_image_desc': 'ImageDesc',
                   'gpv_conv_wgrad_problem': 'ConvWgradProblem', 'gpv_jpeg_info': 'JpegInfo', 'gpv_jpeg_desc': 'JpegDesc'},
           'beam': {'gpv_beam_args': 'BeamArgs', 'gpv_beam_reorder_args': 'ReorderArgs'},
           'huff': {'gpv_huff_table': 'HuffTable', 'gpv_huff_desc': 'HuffDesc'},
           'enc': {'gpv_enc_desc': 'EncDesc'},
           'phrase': {'gpv_phrase_args': 'PhraseArgs'}}
# one letter per parameter: P pointer, i int, f float, q int64_t / long long.  The side libraries only: the hot path's entry points
# carry no argtypes (hip.lib).
SIGNATURES = {'gpv_match_set_loss': 'PPPPPPPPiiiiiifPPPPPPP', 'gpv_match_boxes': 'PPPPPiiiiiifffPPPPPP', 'gpv_match_lsap': 'PPiiiiPPPPP',
              'gpv_eval_det_ap': 'PPPPiiifPPPPP', 'gpv_cap_scores': 'PPPPPiiiiPPiPPqPPPPPPPP', 'gpv_health_stats': 'PiPiPPP',
              'gpv_health_commit': 'PiiPPPP', 'gpv_huff_prepare': 'PqPPPqPP', 'gpv_huff_workspace_bytes': 'iiqP',
              'gpv_huff_decode': 'PiiqPqP', 'gpv_beam_step': 'PP', 'gpv_beam_reorder': 'PP', 'gpv_enc_workspace_bytes': 'iqP',
              'gpv_enc_encode': 'PiiiPqPqPPP', 'gpv_enc_header': 'iiiiPP', 'gpv_phrase_step': 'PP'}
SIDE = [k for k in probe.LIBRARIES if k != 'hip']


def lib_path():
    return probe.built('hip')


@pytest.mark.parametrize('key', list(probe.LIBRARIES))
def test_library_exports_exactly_the_declared_entry_points(key):
    l, mod, names = probe.LIBRARIES[key], probe.module(key), probe.declared(key)
    assert (len(names) if isinstance(PINNED[key], int) else names) == PINNED[key], names
    assert sorted(mod.EXPORTS) == names
    path = probe.built(key)
    lib = ctypes.CDLL(path)
    for n in names:
        assert hasattr(lib, n), f'{n} declared in include/{l.header} but not exported'
    # every other exported gpv_* symbol is declared
    exported = probe.exported(path)
    assert exported == names, set(exported) ^ set(names)
    # no entry point carries the prefix of another, more specific library: the pinned lists stay apart
    for other in probe.LIBRARIES.values():
        if other.key != key and other.prefix.startswith(l.prefix):
            assert not any(n.startswith(other.prefix) for n in names), other.prefix
    if key in NO_GETENV:
        assert not re.search(r'\bgetenv\b', probe.imports(path)), f'{l.file} reads the environment'


def _make(*args):
    csrc = os.path.join(ROOT, 'gpv-1_amd', 'csrc')
    return subprocess.run(['make', '-n', '-C', csrc] + list(args), capture_output=True, text=True, check=True).stdout


@pytest.mark.parametrize('key', list(probe.LIBRARIES))
def test_makefile_builds_the_library_from_its_own_sources(key):
    """what the Makefile builds, not what it says: a dry run of `all` links exactly the files of LIBRARIES, this one from the objects of
    its own sources, each compiled for gfx950 and with -ffp-contract=off exactly where a host rule is repeated bit for bit; `clean`
    names every library and object"""
    import __graft_entry__ as entry
    dry = _make('-B', 'all').splitlines()
    links = {l.split()[-1]: l.split() for l in dry if ' -shared ' in l}
    assert sorted(links) == sorted(l.file for l in probe.LIBRARIES.values())
    objs = [os.path.basename(s)[:-4] + '.o' for s in entry._make_lists(key)[0]]
    line = links[probe.LIBRARIES[key].file]
    assert [w for w in line if w.endswith('.o') and w != 'build_id.o'] == objs
    assert ('build_id.o' in line) == (key == 'hip')
    others = {o for k in probe.LIBRARIES if k != key for o in (os.path.basename(s)[:-4] + '.o' for s in entry._make_lists(k)[0])}
    assert not others & set(objs)
    for o in objs:
        compile_line = [l for l in dry if f' -c {o[:-2]}.hip ' in l]
        assert len(compile_line) == 1 and '--offload-arch=gfx950' in compile_line[0].split()
        assert ('-ffp-contract=off' in compile_line[0].split()) == (key in FP_CONTRACT_OFF), compile_line[0]
    clean = _make('clean').split()
    assert set(links) <= set(clean) and set(objs) <= set(clean)


def test_abi_version_is_one_number():
    """the library, the mirror's loader and the header's comment carry the same version: an older mirror passes shorter structs"""
    import gpv1_amd.hip as hip
    lib = ctypes.CDLL(lib_path())
    lib.gpv_abi_version.restype = ctypes.c_int
    assert lib.gpv_abi_version() == hip.ABI_VERSION == 2
    assert re.search(r'int gpv_abi_version\(void\); /\* = (\d+)\b', open(HEADER).read()).group(1) == str(hip.ABI_VERSION)


@pytest.mark.parametrize('key', SIDE)
def test_argtypes_are_the_header_prototypes(key):
    """class by class, position by position: a hand-counted run of argtypes that is one short shifts every later argument"""
    mod, protos = probe.module(key), probe.prototypes(key)
    assert sorted(protos) == sorted(mod.EXPORTS)
    probe.built(key)
    for name, sig in protos.items():
        assert sig == SIGNATURES[name], name
        fn = getattr(mod.lib(), name)
        assert fn.restype is ctypes.c_int and probe.argtypes_classes(fn) == sig, name


def test_header_constants_are_the_mirrors():
    """every #define GPV_<NAME> <int> of include/gpv_hip.h that gpv1_amd.hip repeats as <NAME> has the header's value"""
    import gpv1_amd.hip as hip
    consts = {k: int(v) for k, v in re.findall(r'#define\s+GPV_(\w+)\s+(\d+)\b', probe.source('hip'))}
    found = {k: v for k, v in consts.items() if type(getattr(hip, k, None)) is int}
    assert {k: getattr(hip, k) for k in found} == found
    assert sum(k.startswith('OPT_') for k in consts) == sum(k.startswith('OPT_') for k in found) == 21
    assert {'BF16', 'F32', 'ACT_NONE', 'ACT_RELU', 'ACT_GELU', 'KMAJOR', 'TRANS'} <= set(found)


def test_production_library_has_no_tuning_code():
    """the timing-ablation instances of the weight-gradient kernel ("results wrong by construction"), the environment
    reads of the launch heuristics and the kernels that did not pay live in the -DGPV_TUNING build only (libgpv_hip_tuning.so)."""
    path = lib_path()
    assert path.endswith('libgpv_hip.so')
    syms = subprocess.run(['nm', '-C', path], capture_output=True, text=True).stdout
    assert '_abl' not in syms and 'ffn_fused' not in syms
    # the library never calls getenv (nm -D --undefined-only lists its imports)
    und = subprocess.run(['nm', '-D', '--undefined-only', path], capture_output=True, text=True).stdout
    assert not re.search(r'\bgetenv\b', und), 'libgpv_hip.so reads the environment'


def test_every_switch_is_documented():
    """INTEGRATION.md section 3 lists every GPV_* switch the tree reads (os.environ in the Python layer, tune_env in
    the native sources) -- regenerate the table with `python tools/list_knobs.py` when this fails."""
    names = subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'list_knobs.py'), '--names'], capture_output=True, text=True).stdout.split()
    assert len(names) > 60
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    table = doc[doc.index('<!-- knobs:begin -->'):doc.index('<!-- knobs:end -->')]
    listed = set(re.findall(r'^\| `(GPV_[A-Z0-9_]+)` \|', table, flags=re.M))
    assert sorted(listed) == sorted(names), (sorted(set(names) - listed), sorted(listed - set(names)))


@pytest.mark.parametrize('key', list(STRUCTS))
def test_ctypes_structs_match_the_c_layout(key, tmp_path):
    pairs = [(cname, getattr(probe.module(key), mirror)) for cname, mirror in STRUCTS[key].items()]
    layout = probe.c_layout(tmp_path, [probe.header_path(key)], pairs)
    for cname, cls in pairs:
        assert layout[cname] == probe.ctypes_layout(cls), (cname, layout[cname], probe.ctypes_layout(cls))


@pytest.mark.parametrize('key', list(probe.LIBRARIES))
def test_every_ctypes_mirror_is_probed(key):
    mod = probe.module(key)
    mirrors = {n for n, v in vars(mod).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == mod.__name__}
    assert mirrors == set(STRUCTS.get(key, {}).values())


def test_product_refuses_to_run_without_the_library(monkeypatch, tmp_path):
    """no CPU / eager fallback: a missing library or a CPU tensor is an error, not a silent detour"""
    import importlib
    import torch
    import gpv1_amd.hip as hip
    monkeypatch.setattr(hip, '_LIB', None)
    monkeypatch.setattr(hip, '_LIB_PATH', str(tmp_path / 'nope.so'))
    try:
        hip.lib()
        raise AssertionError('expected RuntimeError')
    except RuntimeError as e:
        assert 'no CPU/eager fallback' in str(e)
    monkeypatch.undo()
    try:
        hip._p(torch.zeros(4))
        raise AssertionError('expected RuntimeError')
    except RuntimeError as e:
        assert 'GPU' in str(e)


def test_the_mirror_refuses_short_epilogue_vectors():
    """The C ABI takes plain pointers and cannot see a short rowscale / bias; the Python mirror has the tensors and refuses before any
    launch (hip.check_epilogue_extents; include/gpv_hip.h gpv_conv_args: rowscale is per output ROW -- per PIXEL in conv modes 0 / 1,
    per Cout in mode 2).  Round 6: a tool passed a [Cout] rowscale to a forward convolution and the kernel read 19200 floats from 64."""
    import pytest
    import torch
    import gpv1_amd.hip as hip
    B, OH, OW, Cout, Cin = 1, 120, 160, 64, 64
    hip.check_epilogue_extents('conv2d mode 0', B * OH * OW, Cout, torch.ones(B * OH * OW), torch.zeros(Cout))
    hip.check_epilogue_extents('conv2d mode 2', Cout, Cin, torch.ones(Cout), None)
    hip.check_epilogue_extents('gemm', 192, 768, None, None)
    with pytest.raises(ValueError, match='rowscale has 64 elements.*19200 needed'):
        hip.check_epilogue_extents('conv2d mode 0', B * OH * OW, Cout, torch.ones(Cout), torch.zeros(Cout))
    with pytest.raises(ValueError, match='bias has 32 elements.*64 needed'):
        hip.check_epilogue_extents('conv2d mode 0', B * OH * OW, Cout, None, torch.zeros(32))
    with pytest.raises(ValueError, match='rowscale'):
        hip.check_epilogue_extents('gemm', 192, 768, torch.ones(191), torch.zeros(768))
