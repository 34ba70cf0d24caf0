"""ctypes binding of libgpv_phrase.so (C ABI in include/gpv_phrase.h): the phrase-constrained beam search step on the device.

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.  Nothing here synchronises or
allocates: the call is capturable.  The rule is stated in ``gpv1_amd.phrases``; the cache reorder behind a step is ``hip_beam.reorder``.
"""
import ctypes as C
from functools import partial

import torch

from . import _native, hip_beam
from . import phrases as rule
from .hip import _chk, _stream

EXPORTS = ['gpv_phrase_step']
MAX_K, MAX_T = rule.MAX_K, rule.MAX_T                     # GPV_PHRASE_MAX_K, GPV_PHRASE_MAX_T
DONE, VOID = rule.DONE, rule.VOID                         # GPV_PHRASE_DONE, GPV_PHRASE_VOID
_LIB = None
_LIB_PATH = _native.lib_path('phrase')
_want = partial(_native.want, 'hip_phrase')


class PhraseArgs(C.Structure):
    _fields_ = [('logits', C.c_void_p), ('pitch', C.c_int64), ('inv_pen', C.c_void_p), ('lse', C.c_void_p), ('seq_lp', C.c_void_p),
                ('seqs', C.c_void_p), ('tok', C.c_void_p), ('parent', C.c_void_p), ('length', C.c_void_p), ('node', C.c_void_p),
                ('phrase', C.c_void_p), ('child_off', C.c_void_p), ('child_tok', C.c_void_p), ('child_node', C.c_void_p),
                ('terminal', C.c_void_p), ('B', C.c_int), ('K', C.c_int), ('V', C.c_int), ('T', C.c_int), ('t', C.c_int),
                ('pad_id', C.c_int), ('stop_id', C.c_int), ('dtype', C.c_int), ('M', C.c_int), ('E', C.c_int)]


_SIGNATURES = {'gpv_phrase_step': [C.POINTER(PhraseArgs), C.c_void_p]}


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('phrase', _SIGNATURES, _LIB_PATH)
    return _LIB


def step(logits, lse, seq_lp, seqs, tok, parent, node, phrase, length, t, pset, inv_pen=None):
    """gpv_phrase_step on the current stream: one launch, no sync, everything in place.  logits [K*B, V] bf16 / fp32 with unit column
    stride (any row pitch >= V: a view of the decoder's [K*B, T, V] buffer), lse [K*B] fp32 out, seq_lp [B,K] fp32, seqs [K,B,T] int64,
    tok [K*B] int64 out, parent [B,K] int32 out, node / phrase / length [B,K] int32; pset a phrases.PhraseSet; inv_pen [T+1] fp32 or None."""
    def extents(K, V, T):
        rule.check_extents(K, T, pset, t)
        if V != pset.V:
            raise ValueError(f'hip_phrase.step: the phrase set was compiled for a vocabulary of {pset.V}, the logits have {V} columns')
    f, K, B, T, V = hip_beam.step_fields('hip_phrase', logits, lse, seq_lp, seqs, tok, parent, length, inv_pen, extents)
    off, ctok, cnode, term = pset.device_arrays(logits.device)
    M, E = pset.M, pset.E
    a = PhraseArgs(node=_want('node', node, torch.int32, (B, K)), phrase=_want('phrase', phrase, torch.int32, (B, K)),
                   child_off=_want('child_off', off, torch.int32, (M + 1,)), child_tok=_want('child_tok', ctok, torch.int32, (E,)),
                   child_node=_want('child_node', cnode, torch.int32, (E,)), terminal=_want('terminal', term, torch.int32, (M,)),
                   t=t, pad_id=pset.pad_id, stop_id=pset.stop_id, M=M, E=E, **f)
    _chk(lib().gpv_phrase_step(C.byref(a), _stream()), 'gpv_phrase_step')
