"""ctypes binding of libgpv_huff.so (C ABI in include/gpv_huff.h): the JPEG Huffman stream decoded on the device.

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.  ``prepare`` is host code (no HIP
call, the GIL released); ``decode`` neither synchronises nor allocates.  The rule is stated in ``gpv1_amd.jpeg_entropy``.
"""
import ctypes as C

import torch

from . import _native
from . import jpeg_entropy as rule
from .hip import JpegInfo, JpegUnsupported, _chk, _stream

EXPORTS = ['gpv_huff_decode', 'gpv_huff_prepare', 'gpv_huff_workspace_bytes']
ROUTE_DEVICE, ROUTE_HOST = 0, 1                           # GPV_HUFF_ROUTE_*
MAX_BITS = rule.MAX_STREAM * 8
_LIB = None
_LIB_PATH = _native.lib_path('huff')


class HuffTable(C.Structure):
    _fields_ = [('look_nbits', C.c_ubyte * 512), ('look_sym', C.c_ubyte * 512), ('maxcode', C.c_int * 18), ('valoffset', C.c_int * 17),
                ('syms', C.c_ubyte * 256), ('reserved', C.c_int)]


class HuffDesc(C.Structure):
    _fields_ = [('stream', C.c_void_p), ('coefs', C.c_void_p), ('status', C.c_void_p), ('coef_offset', C.c_int64 * 3),
                ('coef_count', C.c_int64), ('nbits', C.c_int), ('stream_cap', C.c_int), ('ncomp', C.c_int), ('mcus_x', C.c_int),
                ('mcus_y', C.c_int), ('blocks_per_mcu', C.c_int), ('nblocks', C.c_int), ('bh', C.c_int * 3), ('bw', C.c_int * 3),
                ('comp_h', C.c_int * 3), ('comp_v', C.c_int * 3), ('blk_comp', C.c_ubyte * 8), ('blk_v', C.c_ubyte * 8),
                ('blk_h', C.c_ubyte * 8), ('dc', HuffTable * 3), ('ac', HuffTable * 3)]


_SIGNATURES = {'gpv_huff_prepare': [C.c_char_p, C.c_int64, C.POINTER(JpegInfo), C.POINTER(HuffDesc), C.c_void_p, C.c_int64,
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int)],
               'gpv_huff_workspace_bytes': [C.c_int, C.c_int, C.c_int64, C.POINTER(C.c_int64)],
               'gpv_huff_decode': [C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p]}


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('huff', _SIGNATURES, _LIB_PATH)
    return _LIB


def prepare(data, out=None, desc=None):
    """gpv_huff_prepare (host side, releases the GIL): data = bytes; out = None (sizes only) or a writable uint8 buffer (numpy array /
    CPU tensor) of at least stream_cap bytes that receives the un-stuffed, zero-padded stream.
    -> (JpegInfo, HuffDesc, stream_cap, route: 'device' | 'host')"""
    info, desc = JpegInfo(), (desc if desc is not None else HuffDesc())
    cap, route = C.c_int64(0), C.c_int(0)
    if out is None:
        ptr, n = None, 0
    elif torch.is_tensor(out):
        if out.is_cuda or out.dtype != torch.uint8 or not out.is_contiguous():
            raise TypeError('hip_huff.prepare: out must be a contiguous CPU uint8 tensor')
        ptr, n = out.data_ptr(), out.numel()
    else:
        ptr, n = out.ctypes.data, out.size
    err = lib().gpv_huff_prepare(data, len(data), C.byref(info), C.byref(desc), ptr, n, C.byref(cap), C.byref(route))
    if err == 801:
        raise JpegUnsupported('gpv_huff_prepare: not a baseline 8-bit 1- or 3-component JPEG with 4:4:4 / 4:2:2 / 4:2:0 sampling')
    if err:
        raise ValueError(f'gpv_huff_prepare: malformed JPEG (hipError {err})')
    return info, desc, int(cap.value), ('device' if route.value == ROUTE_DEVICE else 'host')


def workspace_bytes(B, subseq_bits, max_nbits):
    rule.check_subseq_bits(subseq_bits)
    if B <= 0 or not 0 <= max_nbits <= MAX_BITS:
        raise ValueError(f'hip_huff.workspace_bytes: B >= 1 and 0 <= max_nbits <= {MAX_BITS} are supported, got {B}, {max_nbits}')
    n = C.c_int64(0)
    _chk(lib().gpv_huff_workspace_bytes(B, subseq_bits, max_nbits, C.byref(n)), 'gpv_huff_workspace_bytes')
    return int(n.value)


def decode(descs_dev, B, subseq_bits, max_nbits, workspace):
    """gpv_huff_decode on the current stream: one launch, no sync.  descs_dev = uint8 device tensor holding B packed HuffDesc structs
    (their stream / coefs / status pointers set), workspace = uint8 device tensor of at least workspace_bytes(...) bytes."""
    for name, t in (('descs', descs_dev), ('workspace', workspace)):
        _native.want('hip_huff.decode', name, t, torch.uint8, t.shape)          # any shape: the sizes are checked in bytes below
    need = workspace_bytes(B, subseq_bits, max_nbits)
    if descs_dev.numel() < B * C.sizeof(HuffDesc):
        raise ValueError(f'hip_huff.decode: descs holds {descs_dev.numel()} bytes, {B * C.sizeof(HuffDesc)} needed for {B} descriptors')
    if workspace.numel() < need:
        raise ValueError(f'hip_huff.decode: workspace holds {workspace.numel()} bytes, {need} needed')
    if workspace.data_ptr() % 16 or descs_dev.data_ptr() % 8:
        raise ValueError('hip_huff.decode: workspace must be 16-byte aligned and descs 8-byte aligned')
    _chk(lib().gpv_huff_decode(descs_dev.data_ptr(), B, subseq_bits, max_nbits, workspace.data_ptr(), workspace.numel(), _stream()),
         'gpv_huff_decode')
