"""The native libraries of the package, described once: the table of libraries, the one loader and the one tensor check that the
binding modules (``hip`` and ``hip_<key>``) share.  No torch import: ``__graft_entry__.build()`` and the ABI tests read the table too.

Same rule for every library: no CPU / eager fallback -- a missing library or a CPU tensor is an error.
"""
import ctypes as C
import os
from collections import namedtuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# key: the binding module is gpv1_amd.hip for 'hip' and gpv1_amd.hip_<key> otherwise; file: under gpv-1_amd/csrc; header: the one
# public header under include/ that declares the entry points; prefix: what every entry point starts with (no other library's
# entry point may); noun: names the library in the "not found" message.
Library = namedtuple('Library', 'key file header prefix noun')
LIBRARIES = {l.key: l for l in (
    Library('hip', 'libgpv_hip.so', 'gpv_hip.h', 'gpv_', 'HIP'),
    Library('eval', 'libgpv_eval.so', 'gpv_eval.h', 'gpv_eval_', 'evaluation'),
    Library('cap', 'libgpv_cap.so', 'gpv_cap.h', 'gpv_cap_', 'caption scoring'),
    Library('match', 'libgpv_match.so', 'gpv_match.h', 'gpv_match_', 'matching'),
    Library('health', 'libgpv_health.so', 'gpv_health.h', 'gpv_health_', 'flight-recorder'),
    Library('beam', 'libgpv_beam.so', 'gpv_beam.h', 'gpv_beam_', 'beam search'),
    Library('huff', 'libgpv_huff.so', 'gpv_huff.h', 'gpv_huff_', 'JPEG entropy'),
    Library('enc', 'libgpv_enc.so', 'gpv_enc.h', 'gpv_enc_', 'JPEG encoder'),
    Library('phrase', 'libgpv_phrase.so', 'gpv_phrase.h', 'gpv_phrase_', 'phrase search'),
)}


def module_name(key):
    return 'gpv1_amd.hip' if key == 'hip' else 'gpv1_amd.hip_' + key


def header_path(key):
    return os.path.join(ROOT, 'include', LIBRARIES[key].header)


def lib_path(key):
    return os.path.join(ROOT, 'gpv-1_amd', 'csrc', LIBRARIES[key].file)


def load(key, signatures, path=None):
    """CDLL of library `key` (at `path`, default lib_path(key)).  signatures = {entry point: argtypes}: each listed entry point gets
    restype int (a hipError_t) and those argtypes."""
    path = path or lib_path(key)
    if not os.path.exists(path):
        raise RuntimeError(
            f'gpv1_amd: {LIBRARIES[key].noun} kernel library not found at {path}. Build it with '
            f'`python -c "import __graft_entry__ as g; g.build()"` (make -C gpv-1_amd/csrc). '
            f'There is no CPU/eager fallback by design.')
    lib = C.CDLL(path)
    for name, argtypes in signatures.items():
        fn = getattr(lib, name)
        fn.restype = C.c_int
        fn.argtypes = argtypes
    return lib


def want(where, name, t, dtype, shape):
    """the device address of tensor `t` after checking that it lives on the GPU and is a contiguous `dtype` tensor of `shape`"""
    if not t.is_cuda:
        raise RuntimeError(f'gpv1_amd: {where}: {name} must live on the GPU (no CPU fallback exists)')
    if t.dtype != dtype or tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise ValueError(f'{where}: {name} must be a contiguous {dtype} tensor of shape {tuple(shape)}, got {t.dtype} {tuple(t.shape)}')
    return t.data_ptr()
