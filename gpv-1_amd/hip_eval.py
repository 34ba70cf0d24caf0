"""ctypes binding of libgpv_eval.so (C ABI in include/gpv_eval.h): device-side scoring for train-time evaluation.

Evaluation is outside the hot-path boundary of libgpv_hip.so, whose entry points are pinned (``hip.EXPORTS``).  Same rules as
``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.
"""
import ctypes as C
from functools import partial

import torch

from . import _native
from .hip import _chk, _stream

EXPORTS = ['gpv_eval_det_ap']
MAX_Q = 1024
_LIB = None
_LIB_PATH = _native.lib_path('eval')
_SIGNATURES = {'gpv_eval_det_ap': [C.c_void_p] * 4 + [C.c_int] * 3 + [C.c_float] + [C.c_void_p] * 5}
_want = partial(_native.want, 'det_ap')


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('eval', _SIGNATURES, _LIB_PATH)
    return _LIB


def det_ap(rel_logits, boxes, gt, gt_count, iou_thresh=0.5, score=None, order=None, tp=None, ap=None):
    """gpv_eval_det_ap on the current stream, one launch, no sync.  rel_logits [B,Q,2] fp32, boxes [B,Q,4] fp32 cxcywh,
    gt [B,G,4] fp32 xywh normalised, gt_count [B] int32 (0..G).  Outputs (allocated when not given; views of preallocated buffers
    work as long as they are contiguous): score [B,Q] fp32 sorted descending, order [B,Q] int32, tp [B,Q] uint8, ap [B] fp64.
    -> (score, order, tp, ap)"""
    if rel_logits.dim() != 3 or rel_logits.shape[2] != 2:
        raise ValueError(f'det_ap: rel_logits must be [B,Q,2], got {tuple(rel_logits.shape)}')
    B, Q, _ = rel_logits.shape
    if gt.dim() != 3 or gt.shape[0] != B or gt.shape[2] != 4:
        raise ValueError(f'det_ap: gt must be [B,G,4] with B = {B}, got {tuple(gt.shape)}')
    G = gt.shape[1]
    dev = rel_logits.device
    score = torch.empty(B, Q, dtype=torch.float32, device=dev) if score is None else score
    order = torch.empty(B, Q, dtype=torch.int32, device=dev) if order is None else order
    tp = torch.empty(B, Q, dtype=torch.uint8, device=dev) if tp is None else tp
    ap = torch.empty(B, dtype=torch.float64, device=dev) if ap is None else ap
    args = (_want('rel_logits', rel_logits, torch.float32, (B, Q, 2)), _want('boxes', boxes, torch.float32, (B, Q, 4)),
            _want('gt', gt, torch.float32, (B, G, 4)) if G > 0 else None, _want('gt_count', gt_count, torch.int32, (B,)),
            B, Q, G, float(iou_thresh),
            _want('score', score, torch.float32, (B, Q)), _want('order', order, torch.int32, (B, Q)),
            _want('tp', tp, torch.uint8, (B, Q)), _want('ap', ap, torch.float64, (B,)))
    _chk(lib().gpv_eval_det_ap(*args, _stream()), 'gpv_eval_det_ap')
    return score, order, tp, ap
