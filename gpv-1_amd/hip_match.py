"""ctypes binding of libgpv_match.so (C ABI in include/gpv_match.h): device-side Hungarian matching and set criterion for box batches.

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.  Nothing here synchronises: the
caller reads ``status`` after its own device-to-host copy (``check_status``).
"""
import ctypes as C
from functools import partial

import torch

from . import _native
from .hip import _chk, _p, _stream

EXPORTS = ['gpv_match_boxes', 'gpv_match_lsap', 'gpv_match_set_loss']
MAX_DIM = 256          # GPV_MATCH_MAX_DIM: max(Q, Gmax)
TILE = 1280            # GPV_MATCH_TILE: Q * Gmax up to which match_boxes needs no cost workspace
MAX_CLASSES = 64       # GPV_MATCH_MAX_CLASSES: C + 1
ERR_BITS = {1: 'the matching cost has a NaN or -inf entry (or a label outside the classes)',
            2: 'the matching cost is infeasible (a search found only +inf)',
            4: 'a predicted or target box is degenerate (x1 < x0 or y1 < y0)'}
_LIB = None
_LIB_PATH = _native.lib_path('match')
_SIGNATURES = {'gpv_match_lsap': [C.c_void_p] * 2 + [C.c_int] * 4 + [C.c_void_p] * 5,
               'gpv_match_boxes': [C.c_void_p] * 5 + [C.c_int] * 6 + [C.c_float] * 3 + [C.c_void_p] * 6,
               'gpv_match_set_loss': [C.c_void_p] * 8 + [C.c_int] * 6 + [C.c_float] + [C.c_void_p] * 7}
_want = partial(_native.want, 'hip_match')


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('match', _SIGNATURES, _LIB_PATH)
    return _LIB


def supported(Q, Gmax):
    """whether one problem of Q predictions and up to Gmax targets fits the solver (GPV_MATCH_MAX_DIM)"""
    return 1 <= Q <= MAX_DIM and 1 <= Gmax <= MAX_DIM


def check_status(status):
    """raise if any status word of a finished call (host integers, after the device-to-host copy) is not 0"""
    bits = 0
    for s in status:
        bits |= int(s)
    if bits:
        raise RuntimeError('gpv1_amd: the device matcher reported: ' + '; '.join(m for b, m in ERR_BITS.items() if bits & b))


def _index_outputs(P, K, dev):
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    return i32(P, K), i32(P, K), i32(P), i32(P)


def lsap(cost, g_count):
    """gpv_match_lsap on the current stream, one launch, no sync.  cost [P,Q,Gmax] fp32, g_count [P] int32 (<= 0: an empty problem).
    -> (pred_idx [P,K], tgt_idx [P,K], n_pairs [P], status [P]) int32 with K = min(Q, Gmax); rows are sorted by pred_idx, -1 behind
    n_pairs."""
    if not cost.is_cuda:
        raise RuntimeError('gpv1_amd: hip_match: cost must live on the GPU (no CPU fallback exists for the device matcher)')
    if cost.dim() != 3:
        raise ValueError(f'hip_match.lsap: cost must be [P,Q,Gmax], got {tuple(cost.shape)}')
    P, Q, G = cost.shape
    if not supported(Q, G):
        raise ValueError(f'hip_match.lsap: problems of up to {MAX_DIM} x {MAX_DIM} are supported (GPV_MATCH_MAX_DIM), got {Q} x {G}; '
                         f'nothing is truncated')
    K = min(Q, G)
    pred, tgt, n, st = _index_outputs(P, K, cost.device)
    _chk(lib().gpv_match_lsap(_want('cost', cost, torch.float32, (P, Q, G)), _want('g_count', g_count, torch.int32, (P,)), P, Q, G, K,
                              _p(pred), _p(tgt), _p(n), _p(st), _stream()), 'gpv_match_lsap')
    return pred, tgt, n, st


def _box_args(logits, boxes, tgt_boxes, tgt_labels, g_count):
    if not logits.is_cuda:
        raise RuntimeError('gpv1_amd: hip_match: logits must live on the GPU (no CPU fallback exists for the device matcher)')
    if logits.dim() != 4 or tgt_boxes.dim() != 3:
        raise ValueError(f'hip_match: logits must be [L,B,Q,C+1] and tgt_boxes [B,Gmax,4], got {tuple(logits.shape)} {tuple(tgt_boxes.shape)}')
    L, B, Q, C1 = logits.shape
    G = tgt_boxes.shape[1]
    if not supported(Q, G):
        raise ValueError(f'hip_match: problems of up to {MAX_DIM} x {MAX_DIM} are supported (GPV_MATCH_MAX_DIM), got {Q} x {G}; '
                         f'nothing is truncated')
    if not 2 <= C1 <= MAX_CLASSES:
        raise ValueError(f'hip_match: 2..{MAX_CLASSES} classes (C + 1) are supported (GPV_MATCH_MAX_CLASSES), got {C1}')
    ptrs = (_want('logits', logits, torch.float32, (L, B, Q, C1)), _want('boxes', boxes, torch.float32, (L, B, Q, 4)),
            _want('tgt_boxes', tgt_boxes, torch.float32, (B, G, 4)), _want('tgt_labels', tgt_labels, torch.int32, (B, G)),
            _want('g_count', g_count, torch.int32, (B,)))
    return ptrs, (L, B, Q, C1, G)


def match_boxes(logits, boxes, tgt_boxes, tgt_labels, g_count, w_class, w_bbox, w_giou, cost_out=False):
    """gpv_match_boxes on the current stream: cost and assignment of L * B problems in one launch, no sync.  logits [L,B,Q,C+1],
    boxes [L,B,Q,4] cxcywh, tgt_boxes [B,Gmax,4] fp32, tgt_labels [B,Gmax], g_count [B] int32 (-1: the image takes no part, 0: no
    boxes).  cost_out=True also returns the [L,B,Q,Gmax] cost (for the tests; columns behind g_count hold zeros); a problem too large
    for the LDS tile (Q * Gmax > GPV_MATCH_TILE) gets that buffer as its workspace either way.
    -> (pred_idx [L*B,K], tgt_idx [L*B,K], n_pairs [L*B], status [L*B], cost or None)"""
    ptrs, (L, B, Q, C1, G) = _box_args(logits, boxes, tgt_boxes, tgt_labels, g_count)
    K = min(Q, G)
    pred, tgt, n, st = _index_outputs(L * B, K, logits.device)
    cost = None
    if cost_out or Q * G > TILE:
        cost = torch.zeros(L, B, Q, G, dtype=torch.float32, device=logits.device)
    _chk(lib().gpv_match_boxes(*ptrs, L, B, Q, C1, G, K, float(w_class), float(w_bbox), float(w_giou), _p(cost),
                               _p(pred), _p(tgt), _p(n), _p(st), _stream()), 'gpv_match_boxes')
    return pred, tgt, n, st, (cost if cost_out else None)


def set_loss(logits, boxes, tgt_boxes, tgt_labels, g_count, pred_idx, tgt_idx, n_pairs, status, eos_coef):
    """gpv_match_set_loss on the current stream, one launch, no sync: the four per-(l, b) sums and the unnormalised gradients.
    -> (partial [L,B,4] float64 = {weighted CE numerator, weight sum, L1 sum, (1 - giou) sum}, dlogits [L,B,Q,C+1], dboxes_l1 [L,B,Q,4],
    dboxes_giou [L,B,Q,4] fp32, num_boxes [1] float64 = max(sum max(g_count, 0), 1))"""
    ptrs, (L, B, Q, C1, G) = _box_args(logits, boxes, tgt_boxes, tgt_labels, g_count)
    K = pred_idx.shape[1]
    dev = logits.device
    partial = torch.empty(L, B, 4, dtype=torch.float64, device=dev)
    dlogits = torch.empty_like(logits)
    dl1 = torch.empty_like(boxes)
    dgi = torch.empty_like(boxes)
    nb = torch.empty(1, dtype=torch.float64, device=dev)
    _chk(lib().gpv_match_set_loss(*ptrs, _want('pred_idx', pred_idx, torch.int32, (L * B, K)), _want('tgt_idx', tgt_idx, torch.int32, (L * B, K)),
                                  _want('n_pairs', n_pairs, torch.int32, (L * B,)), L, B, Q, C1, G, K, float(eos_coef),
                                  _p(partial), _p(dlogits), _p(dl1), _p(dgi), _p(nb), _want('status', status, torch.int32, (L * B,)),
                                  _stream()), 'gpv_match_set_loss')
    return partial, dlogits, dl1, dgi, nb
