"""C-ABI checks of the addon library libgpv_phrase.so that need no GPU, modelled on tests/test_abi_enc_cpu.py: exports == header ==
binding, prototypes, struct layout, no environment reads, a Makefile target of its own that leaves `all` and `extensions` what they
were, the header's constants, and the refusal of bad extents."""
import ctypes
import os
import re
import subprocess

import pytest

import __graft_entry__ as entry
from gpv1_amd import _native
from tests import abi_probe as probe

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 'phrase'
PINNED = ['gpv_phrase_step']
STRUCTS = {'gpv_phrase_args': 'PhraseArgs'}
SIGNATURES = {'gpv_phrase_step': 'PP'}


def module():
    import importlib
    return importlib.import_module(_native.module_name(KEY))


def built():
    if not os.path.exists(module()._LIB_PATH):
        entry.build()
    return module()._LIB_PATH


def test_the_addon_has_a_table_of_its_own_and_the_seven_and_the_extension_are_untouched():
    assert len(_native.LIBRARIES) == 7 and KEY not in _native.LIBRARIES
    assert list(_native.EXTENSIONS) == ['enc']
    assert list(_native.ADDONS) == [KEY]
    l = _native.ADDONS[KEY]
    assert (l.file, l.header, l.prefix) == ('libgpv_phrase.so', 'gpv_phrase.h', 'gpv_phrase_')
    assert _native.library(KEY) is l
    assert _native.module_name(KEY) == 'gpv1_amd.hip_phrase'
    assert _native.lib_path(KEY).endswith('gpv-1_amd/csrc/libgpv_phrase.so') and _native.header_path(KEY).endswith('include/gpv_phrase.h')
    assert _native.lib_path('huff').endswith('libgpv_huff.so') and _native.lib_path('enc').endswith('libgpv_enc.so')
    with pytest.raises(KeyError):
        _native.library('nope')


def test_makefile_links_the_addon_by_its_own_target():
    csrc = os.path.join(ROOT, 'gpv-1_amd', 'csrc')

    def dry(target):
        return subprocess.run(['make', '-n', '-B', '-C', csrc, target], capture_output=True, text=True, check=True).stdout.splitlines()

    def links(target):
        return {l.split()[-1]: l.split() for l in dry(target) if ' -shared ' in l}
    add = links('addons')
    assert list(add) == ['libgpv_phrase.so'] and 'phrase_step.o' in add['libgpv_phrase.so']
    assert sorted(links('all')) == sorted(l.file for l in _native.LIBRARIES.values()) and len(links('all')) == 7
    assert list(links('extensions')) == ['libgpv_enc.so']
    compile_line = [l for l in dry('addons') if ' -c phrase_step.hip' in l]
    assert len(compile_line) == 1 and '-ffp-contract=off' in compile_line[0] and '--offload-arch=gfx950' in compile_line[0]
    clean = subprocess.run(['make', '-n', '-C', csrc, 'clean'], capture_output=True, text=True, check=True).stdout.split()
    assert 'libgpv_phrase.so' in clean and 'phrase_step.o' in clean and 'libgpv_enc.so' in clean and 'libgpv_beam.so' in clean


def test_library_exports_exactly_the_declared_entry_point():
    l, mod = _native.ADDONS[KEY], module()
    names = entry._declared(_native.header_path(KEY), l.prefix)
    assert names == PINNED == sorted(mod.EXPORTS)
    path = built()
    assert entry._exported(path) == names
    for other in list(_native.LIBRARIES.values()) + list(_native.EXTENSIONS.values()):
        assert not other.prefix.startswith(l.prefix), other.prefix
        if other.key != 'hip':
            assert not any(n.startswith(other.prefix) for n in names), other.prefix
    hot = entry._declared(_native.header_path('hip'), 'gpv_')
    assert not any(n.startswith(l.prefix) for n in hot)
    assert not re.search(r'\bgetenv\b', probe.imports(path)), 'libgpv_phrase.so reads the environment'


def test_argtypes_are_the_header_prototypes():
    mod = module()
    src = entry._header_source(_native.header_path(KEY))
    protos = {}
    for name, params in re.findall(r'\bint\s+(gpv_phrase_\w+)\s*\(([^)]*)\)\s*;', src):
        protos[name] = ''.join('P' if '*' in p else probe._C_CLASS[' '.join(p.replace('const ', ' ').split()[:-1])] for p in params.split(','))
    assert protos == SIGNATURES
    built()
    for name, sig in protos.items():
        fn = getattr(mod.lib(), name)
        assert fn.restype is ctypes.c_int and probe.argtypes_classes(fn) == sig, name


def test_ctypes_struct_matches_the_c_layout(tmp_path):
    mod = module()
    pairs = [(cname, getattr(mod, mirror)) for cname, mirror in STRUCTS.items()]
    layout = probe.c_layout(tmp_path, [_native.header_path(KEY)], pairs)
    for cname, cls in pairs:
        assert layout[cname] == probe.ctypes_layout(cls), (cname, layout[cname], probe.ctypes_layout(cls))
    mirrors = {n for n, v in vars(mod).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v.__module__ == mod.__name__}
    assert mirrors == set(STRUCTS.values())
    assert ctypes.sizeof(mod.PhraseArgs) == 160                 # the static_assert of phrase_step.hip


def test_header_constants_are_the_mirrors_and_the_beam_headers():
    mod = module()
    from gpv1_amd import beam, phrases
    const = lambda path, pre: {k: int(eval(v)) for k, v in re.findall(r'#define (' + pre + r'\w+) +(\(-?\d+\)|\d+)', open(path).read())}
    c = const(_native.header_path(KEY), 'GPV_PHRASE_')
    bm = const(_native.header_path('beam'), 'GPV_BEAM_')
    assert (c['GPV_PHRASE_MAX_K'], c['GPV_PHRASE_MAX_T'], c['GPV_PHRASE_LANES']) == (bm['GPV_BEAM_MAX_K'], bm['GPV_BEAM_MAX_T'], bm['GPV_BEAM_LANES'])
    assert (c['GPV_PHRASE_MAX_K'], c['GPV_PHRASE_MAX_T'], c['GPV_PHRASE_LANES']) == (mod.MAX_K, mod.MAX_T, beam.LANES)
    assert (c['GPV_PHRASE_DONE'], c['GPV_PHRASE_VOID']) == (phrases.DONE, phrases.VOID) == (mod.DONE, mod.VOID) == (-1, -2)
    assert (c['GPV_PHRASE_BF16'], c['GPV_PHRASE_F32']) == (bm['GPV_BEAM_BF16'], bm['GPV_BEAM_F32'])


def test_bad_extents_are_refused_before_a_launch():
    """the C entry point returns hipErrorInvalidValue (1) without touching a device, and writes nothing"""
    mod = module()
    lib = ctypes.CDLL(built())
    lib.gpv_phrase_step.argtypes = [ctypes.c_void_p, ctypes.c_void_p]

    def args(**kw):
        a = mod.PhraseArgs(B=2, K=3, V=40, T=6, t=1, pad_id=36, stop_id=38, dtype=1, M=4, E=3, pitch=40)
        for f, _ in mod.PhraseArgs._fields_[:15]:
            if f not in ('pitch', 'inv_pen'):
                setattr(a, f, 4096)                                  # (never dereferenced: every call below is refused first)
        for k, v in kw.items():
            setattr(a, k, v)
        return a
    bad = [dict(K=0), dict(K=9), dict(V=0), dict(T=1), dict(T=65), dict(t=-1), dict(t=5), dict(pitch=39), dict(B=-1), dict(M=1), dict(E=0),
           dict(M=-3), dict(pad_id=40), dict(pad_id=-1), dict(stop_id=40), dict(stop_id=-1), dict(dtype=2), dict(dtype=-1),
           dict(B=1 << 29, K=8)]
    bad += [{f: None} for f, _ in mod.PhraseArgs._fields_[:15] if f not in ('pitch', 'inv_pen')]
    for kw in bad:
        a = args(**kw)
        before = bytes(a)
        assert lib.gpv_phrase_step(ctypes.byref(a), None) == 1, kw
        assert bytes(a) == before
    assert lib.gpv_phrase_step(None, None) == 1
    assert lib.gpv_phrase_step(ctypes.byref(args(B=0)), None) == 0   # an empty batch: nothing is launched


def test_step_refuses_to_run_without_the_library(monkeypatch, tmp_path):
    """no CPU / eager fallback: a missing library is an error"""
    mod = module()
    monkeypatch.setattr(mod, '_LIB', None)
    monkeypatch.setattr(mod, '_LIB_PATH', str(tmp_path / 'nope.so'))
    with pytest.raises(RuntimeError, match='no CPU/eager fallback'):
        mod.lib()
