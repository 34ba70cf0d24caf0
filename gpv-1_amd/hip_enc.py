"""ctypes binding of libgpv_enc.so (C ABI in include/gpv_enc.h): a batch of pictures encoded as baseline JPEG files on the device.

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.  ``header`` is host code (no HIP
call); ``encode`` neither synchronises nor allocates.  The rule is stated in ``gpv1_amd.jpeg_encode``.
"""
import ctypes as C

import torch

from . import _native
from .hip import _chk, _stream

EXPORTS = ['gpv_enc_encode', 'gpv_enc_header', 'gpv_enc_workspace_bytes']
SRC_U8, SRC_BF16, SRC_F32 = 0, 1, 2                       # GPV_ENC_SRC_*
SUBSAMPLING = {'4:4:4': 0, '4:2:2': 1, '4:2:0': 2}        # GPV_ENC_4xx
MAX_BOXES, MAX_BLOCKS, MAX_TOTAL_BLOCKS = 32, 1 << 20, 1 << 24
MAX_LABEL = 32                                            # characters of one box's label
HEADER_BYTES, BLOCK_BYTES, STATUS_CAPACITY = 623, 208, 1
_LIB = None
_LIB_PATH = _native.lib_path('enc')


class EncDesc(C.Structure):
    _fields_ = [('src', C.c_void_p), ('boxes', C.c_void_p), ('colours', C.c_void_p), ('H', C.c_int), ('W', C.c_int), ('pitch', C.c_int),
                ('kind', C.c_int), ('nboxes', C.c_int), ('mean', C.c_float * 3), ('std', C.c_float * 3), ('block_base', C.c_int),
                ('nblocks', C.c_int), ('labels', C.c_int)]


_SIGNATURES = {'gpv_enc_workspace_bytes': [C.c_int, C.c_int64, C.POINTER(C.c_int64)],
               'gpv_enc_encode': [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                  C.c_void_p, C.c_void_p],
               'gpv_enc_header': [C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]}


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('enc', _SIGNATURES, _LIB_PATH)
    return _LIB


def _sub(subsampling):
    if subsampling not in SUBSAMPLING:
        raise ValueError(f'hip_enc: subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}')
    return SUBSAMPLING[subsampling]


def block_count(H, W, subsampling):
    """blocks of one picture's scan, dummy blocks included"""
    hs, vs = ((1, 1), (2, 1), (2, 2))[_sub(subsampling)]
    return -(-(-(-W // hs)) // 8) * -(-(-(-H // vs)) // 8) * (hs * vs + 2)


def file_bound(nblocks):
    """no file of a picture with `nblocks` blocks is longer"""
    return HEADER_BYTES + 2 * BLOCK_BYTES * nblocks + 2


def header(H, W, quality, subsampling):
    buf, n = (C.c_ubyte * HEADER_BYTES)(), C.c_int(0)
    if lib().gpv_enc_header(H, W, quality, _sub(subsampling), buf, C.byref(n)):
        raise ValueError(f'hip_enc.header: H and W must be 1..65535 and quality 1..100, got {H} x {W}, quality {quality}')
    return bytes(buf[:n.value])


def workspace_bytes(B, blocks):
    if B < 1 or not B <= blocks <= MAX_TOTAL_BLOCKS:
        raise ValueError(f'hip_enc.workspace_bytes: B >= 1 and B <= blocks <= {MAX_TOTAL_BLOCKS} are supported, got {B}, {blocks}')
    n = C.c_int64(0)
    _chk(lib().gpv_enc_workspace_bytes(B, blocks, C.byref(n)), 'gpv_enc_workspace_bytes')
    return int(n.value)


def encode(descs, B, quality, subsampling, workspace, out, capacity, sizes, status):
    """gpv_enc_encode on the current stream: four launches, no sync.  descs = an (EncDesc * B) array in host memory that stays alive
    and unchanged until the stream has passed the call (pinned memory keeps the copy asynchronous); the extents are checked here
    first, so that a refusal names its reason."""
    if not 1 <= quality <= 100:
        raise ValueError(f'hip_enc.encode: quality must be 1..100, got {quality}')
    blocks = 0
    for i in range(B):
        d = descs[i]
        if not (1 <= d.H <= 65535 and 1 <= d.W <= 65535 and d.pitch >= d.W and 0 <= d.nboxes <= MAX_BOXES):
            raise ValueError(f'hip_enc.encode: picture {i}: H and W must be 1..65535, pitch >= W and at most {MAX_BOXES} boxes, got '
                             f'{d.H} x {d.W}, pitch {d.pitch}, {d.nboxes} boxes')
        if not 0 <= d.labels <= d.nboxes * MAX_LABEL:
            raise ValueError(f'hip_enc.encode: picture {i}: at most {MAX_LABEL} label bytes per box, got {d.labels} for {d.nboxes} boxes')
        n = block_count(d.H, d.W, subsampling)
        if n > MAX_BLOCKS:
            raise ValueError(f'hip_enc.encode: picture {i} has {n} blocks, at most {MAX_BLOCKS} are supported')
        blocks += n
    need = workspace_bytes(B, blocks)
    _native.want('hip_enc.encode', 'workspace', workspace, torch.uint8, workspace.shape)
    _native.want('hip_enc.encode', 'out', out, torch.uint8, (B * capacity,))
    _native.want('hip_enc.encode', 'sizes', sizes, torch.int32, (B,))
    _native.want('hip_enc.encode', 'status', status, torch.int32, (B,))
    if workspace.numel() < need or workspace.data_ptr() % 16:
        raise ValueError(f'hip_enc.encode: workspace holds {workspace.numel()} bytes, {need} needed, 16-byte aligned')
    _chk(lib().gpv_enc_encode(C.addressof(descs), B, quality, _sub(subsampling), workspace.data_ptr(), workspace.numel(), out.data_ptr(),
                              capacity, sizes.data_ptr(), status.data_ptr(), _stream()), 'gpv_enc_encode')
