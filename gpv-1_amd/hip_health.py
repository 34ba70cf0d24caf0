"""ctypes binding of libgpv_health.so (C ABI in include/gpv_health.h): per-segment tensor statistics, their device ring and the
first-non-finite latch -- the kernels of the training flight recorder (``gpv1_amd.health``).

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.  Nothing here synchronises,
allocates or reads back; every call can be captured in a graph.
"""
import ctypes as C

import numpy as np
import torch

from . import _native
from .hip import _chk, _stream

EXPORTS = ['gpv_health_commit', 'gpv_health_stats']
BLOCK = 16384          # GPV_HEALTH_BLOCK: elements per block of the pinned summation order
F32, BF16 = 0, 1       # GPV_HEALTH_F32 / GPV_HEALTH_BF16
NAN, INF = 1, 2        # GPV_HEALTH_NAN / GPV_HEALTH_INF
STATE_WORDS = 8        # GPV_HEALTH_STATE_WORDS
ST_CURSOR, ST_LATCHED, ST_TRIP_CURSOR, ST_TRIP_SEG, ST_TRIP_INDEX, ST_KIND, ST_TRIPS = range(7)
# numpy mirrors of gpv_health_row (64 bytes), gpv_health_seg (32 bytes) and gpv_health_work (8 bytes)
ROW = np.dtype([('n_nan', '<i8'), ('n_inf', '<i8'), ('n_zero', '<i8'), ('first_bad', '<i8'), ('sumsq', '<f8'), ('bits_sum', '<u8'),
                ('absmax', '<f4'), ('first_kind', '<u4'), ('reserved', '<u8')])
SEG = np.dtype([('ptr', '<u8'), ('n', '<i8'), ('dtype', '<i4'), ('pad', '<i4'), ('ws_first', '<i8')])
WORK = np.dtype([('seg', '<i4'), ('block', '<i4')])
assert ROW.itemsize == 64 and SEG.itemsize == 32 and WORK.itemsize == 8
_LIB = None
_LIB_PATH = _native.lib_path('health')
_SIGNATURES = {'gpv_health_stats': [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p],
               'gpv_health_commit': [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]}


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('health', _SIGNATURES, _LIB_PATH)
    return _LIB


def _bytes(name, t, nbytes):
    return _native.want('hip_health', name, t, torch.uint8, (nbytes,))


def stats(segs, S, work, W, ws, rows):
    """gpv_health_stats on the current stream, two launches, no sync.  All operands are uint8 device tensors holding the C structs:
    segs [S * 32] (gpv_health_seg), work [W * 8] (gpv_health_work), ws [W * 64] and rows [S * 64] (gpv_health_row).  The segment
    pointers inside `segs` are the caller's promise: n elements of the stated dtype are readable there."""
    _chk(lib().gpv_health_stats(_bytes('segs', segs, S * SEG.itemsize), S, _bytes('work', work, W * WORK.itemsize) if W else None, W,
                                _bytes('ws', ws, W * ROW.itemsize) if W else None, _bytes('rows', rows, S * ROW.itemsize), _stream()),
         'gpv_health_stats')


def commit(rows, S, R, state, stamps, ring):
    """gpv_health_commit on the current stream, one launch, no sync.  rows [S * 64], state [STATE_WORDS * 8], stamps [R * 8],
    ring [R * S * 64]: uint8 device tensors (views of one buffer are fine)."""
    _chk(lib().gpv_health_commit(_bytes('rows', rows, S * ROW.itemsize), S, R, _bytes('state', state, STATE_WORDS * 8),
                                 _bytes('stamps', stamps, R * 8), _bytes('ring', ring, R * S * ROW.itemsize), _stream()),
         'gpv_health_commit')
