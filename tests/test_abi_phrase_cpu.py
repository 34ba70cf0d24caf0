"""C-ABI checks of libgpv_phrase.so that need no GPU and are its own: the header's constants against the mirrors and against
gpv_beam.h, the struct size the kernel asserts, and the refusal of bad extents.  (Exports, prototypes, struct layout, Makefile:
tests/test_abi_cpu.py.)"""
import ctypes
import re

import pytest

from gpv1_amd import _native
from tests import abi_probe as probe

KEY = 'phrase'


def module():
    return probe.module(KEY)


def built():
    return probe.built(KEY)


def test_header_constants_are_the_mirrors_and_the_beam_headers():
    mod = module()
    from gpv1_amd import beam, phrases
    assert ctypes.sizeof(mod.PhraseArgs) == 160                 # the static_assert of phrase_step.hip
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
