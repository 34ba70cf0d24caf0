"""ctypes binding of libgpv_beam.so (C ABI in include/gpv_beam.h): the beam search step, the sampled step (one more mode of the same
entry point) and the KV-cache reorder on the device.

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.  Nothing here synchronises or
allocates: all three calls are capturable.  The rule is stated in ``gpv1_amd.beam``.
"""
import ctypes as C
from functools import partial

import torch

from . import _native
from . import beam as rule
from .hip import _chk, _stream

EXPORTS = ['gpv_beam_reorder', 'gpv_beam_step']
MAX_K, MAX_T, MAX_LAYERS = rule.MAX_K, rule.MAX_T, 8      # GPV_BEAM_MAX_K, GPV_BEAM_MAX_T, GPV_BEAM_MAX_LAYERS
_DTYPES = {torch.bfloat16: 0, torch.float32: 1}           # GPV_BEAM_BF16, GPV_BEAM_F32
_LIB = None
_LIB_PATH = _native.lib_path('beam')
_want = partial(_native.want, 'hip_beam')


class BeamArgs(C.Structure):
    _fields_ = [('logits', C.c_void_p), ('pitch', C.c_int64), ('vocab_mask', C.c_void_p), ('inv_pen', C.c_void_p), ('lse', C.c_void_p),
                ('seq_lp', C.c_void_p), ('seqs', C.c_void_p), ('tok', C.c_void_p), ('parent', C.c_void_p), ('finished', C.c_void_p),
                ('length', C.c_void_p), ('seed', C.c_void_p), ('cand_v', C.c_void_p), ('cand_w', C.c_void_p),
                ('B', C.c_int), ('K', C.c_int), ('V', C.c_int), ('T', C.c_int), ('t', C.c_int),
                ('mode', C.c_int), ('pad_id', C.c_int), ('stop_id', C.c_int), ('dtype', C.c_int),
                ('top_k', C.c_int), ('inv_temp', C.c_float), ('top_p', C.c_float),         # (the sampler's; the constraints' stay the last four)
                ('no_repeat', C.c_int), ('min_len', C.c_int), ('rep_neg', C.c_float), ('rep_pos', C.c_float)]


class ReorderArgs(C.Structure):
    _fields_ = [('cache', C.c_void_p * MAX_LAYERS), ('parent', C.c_void_p), ('L', C.c_int), ('B', C.c_int), ('K', C.c_int),
                ('T', C.c_int), ('D', C.c_int), ('upto', C.c_int), ('dtype', C.c_int)]


_SIGNATURES = {'gpv_beam_step': [C.POINTER(BeamArgs), C.c_void_p], 'gpv_beam_reorder': [C.POINTER(ReorderArgs), C.c_void_p]}


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('beam', _SIGNATURES, _LIB_PATH)
    return _LIB


def step_fields(module, logits, lse, seq_lp, seqs, tok, parent, length, inv_pen, extents):
    """What gpv_beam_step and gpv_phrase_step take alike, checked and packed once: -> (fields of the argument struct, K, B, T, V).
    module names the binding in the messages ('hip_beam' / 'hip_phrase'); extents(K, V, T) is its rule's own check of the shapes."""
    want = partial(_native.want, module)
    if not logits.is_cuda:
        raise RuntimeError(f'gpv1_amd: {module}: logits must live on the GPU (no CPU fallback exists for the device '
                           f'{module[4:]} step)')
    if logits.dim() != 2 or seqs.dim() != 3:
        raise ValueError(f'{module}.step: logits must be [K*B, V] and seqs [K,B,T], got {tuple(logits.shape)} {tuple(seqs.shape)}')
    K, B, T = seqs.shape
    R, V = logits.shape
    extents(K, V, T)
    if R != K * B:
        raise ValueError(f'{module}.step: logits must have K*B = {K * B} rows, got {R}')
    if logits.dtype not in _DTYPES:
        raise ValueError(f'{module}.step: logits must be bfloat16 or float32, got {logits.dtype}')
    if logits.stride(1) != 1 or (R > 1 and logits.stride(0) < V):
        raise ValueError(f'{module}.step: logits need unit column stride and a row pitch >= V, got strides {tuple(logits.stride())}')
    return dict(logits=logits.data_ptr(), pitch=logits.stride(0) if R > 1 else V,
                inv_pen=None if inv_pen is None else want('inv_pen', inv_pen, torch.float32, (T + 1,)),
                lse=want('lse', lse, torch.float32, (R,)), seq_lp=want('seq_lp', seq_lp, torch.float32, (B, K)),
                seqs=want('seqs', seqs, torch.int64, (K, B, T)), tok=want('tok', tok, torch.int64, (R,)),
                parent=want('parent', parent, torch.int32, (B, K)), length=want('length', length, torch.int32, (B, K)),
                B=B, K=K, V=V, T=T, dtype=_DTYPES[logits.dtype]), K, B, T, V


def step(logits, lse, seq_lp, seqs, tok, parent, finished, length, t, mode, pad_id, stop_id, inv_pen=None, vocab_mask=None,
         no_repeat_ngram=0, min_length=0, repetition=None):
    """gpv_beam_step on the current stream: one launch, no sync, everything in place.  logits [K*B, V] bf16 / fp32 with unit column
    stride (any row pitch >= V: a view of the decoder's [K*B, T, V] buffer), lse [K*B] fp32 out, seq_lp [B,K] fp32, seqs [K,B,T] int64,
    tok [K*B] int64 out, parent [B,K] int32 out, finished / length [B,K] int32; inv_pen [T+1] fp32 or None, vocab_mask [V] fp32 or None.
    The constraints of the rule: no_repeat_ngram (n, 0 = off), min_length (0 = off), repetition (the (rep_neg, rep_pos) pair of
    beam.rep_factors, None = off)."""
    def extents(K, V, T):
        rule.check_extents(K, V, T, t)
        rule.check_constraints(V, T, no_repeat_ngram, min_length, repetition)
    f, K, B, T, V = step_fields('hip_beam', logits, lse, seq_lp, seqs, tok, parent, length, inv_pen, extents)
    rep_neg, rep_pos = (0.0, 0.0) if repetition is None else repetition
    if mode not in (rule.EXTEND, rule.FREEZE):
        raise ValueError(f'hip_beam.step: mode must be EXTEND (0) or FREEZE (1), got {mode!r}')
    if not (0 <= pad_id < V and 0 <= stop_id < V):
        raise ValueError(f'hip_beam.step: pad_id / stop_id must lie in the vocabulary, got {pad_id} / {stop_id} of {V}')
    a = BeamArgs(vocab_mask=None if vocab_mask is None else _want('vocab_mask', vocab_mask, torch.float32, (V,)),
                 finished=_want('finished', finished, torch.int32, (B, K)), t=t, mode=mode, pad_id=pad_id, stop_id=stop_id,
                 no_repeat=int(no_repeat_ngram), min_len=int(min_length), rep_neg=float(rep_neg), rep_pos=float(rep_pos), **f)
    _chk(lib().gpv_beam_step(C.byref(a), _stream()), 'gpv_beam_step')


def sample_step(logits, lse, seq_lp, seqs, tok, parent, finished, length, t, pad_id, stop_id, seed, cand_v, cand_w, top_k, top_p=None,
                temperature=None, vocab_mask=None):
    """gpv_beam_step in mode GPV_BEAM_SAMPLE on the current stream (THE SAMPLER of gpv1_amd.beam): one launch, no sync, everything in
    place.  The tensors of `step`, the K slots being the K samples of a batch element; seed: ONE int64 on the device, read by the kernel
    (rewrite it between the replays of a captured search); cand_v [K*B, top_k] int32 and cand_w [K*B, top_k] fp32 out (the candidates by
    rank and expf of their log-probabilities); top_p None: off; temperature None: 1.  parent comes back as the identity: no reorder
    follows.  seq_lp is the model's log-probability of the sequence at that temperature, not the truncated sampler's."""
    inv_temp = rule.inv_temperature(temperature)
    f, K, B, T, V = step_fields('hip_beam', logits, lse, seq_lp, seqs, tok, parent, length, None,
                                lambda K, V, T: rule.check_sampler(K, V, T, t, top_k, top_p, inv_temp))
    if not (0 <= pad_id < V and 0 <= stop_id < V):
        raise ValueError(f'hip_beam.sample_step: pad_id / stop_id must lie in the vocabulary, got {pad_id} / {stop_id} of {V}')
    C_ = int(top_k)
    a = BeamArgs(vocab_mask=None if vocab_mask is None else _want('vocab_mask', vocab_mask, torch.float32, (V,)),
                 finished=_want('finished', finished, torch.int32, (B, K)), t=t, mode=rule.SAMPLE, pad_id=pad_id, stop_id=stop_id,
                 seed=_want('seed', seed, torch.int64, (1,)), cand_v=_want('cand_v', cand_v, torch.int32, (K * B, C_)),
                 cand_w=_want('cand_w', cand_w, torch.float32, (K * B, C_)), top_k=C_, inv_temp=0.0 if inv_temp is None else float(inv_temp),
                 top_p=0.0 if top_p is None else float(rule.F32(top_p)), **f)
    _chk(lib().gpv_beam_step(C.byref(a), _stream()), 'gpv_beam_step')


def reorder(caches, parent, upto):
    """gpv_beam_reorder on the current stream: one launch for all layers, in place, no sync.  caches: L contiguous [K*B, T, 3D] tensors
    of one dtype (q | k | v columns), parent [B,K] int32: for positions < upto and the k | v columns row k*B+b becomes old row
    parent[b,k]*B+b."""
    B, K = parent.shape
    L = len(caches)
    if not 1 <= L <= MAX_LAYERS:
        raise ValueError(f'hip_beam.reorder: 1 .. {MAX_LAYERS} layers per call (GPV_BEAM_MAX_LAYERS), got {L}')
    if not 1 <= K <= MAX_K:
        raise ValueError(f'hip_beam.reorder: 1 <= beam size <= {MAX_K} is supported (GPV_BEAM_MAX_K), got {K}')
    c0 = caches[0]
    if c0.dim() != 3 or c0.shape[0] != K * B or c0.shape[2] % 3 != 0 or c0.dtype not in _DTYPES:
        raise ValueError(f'hip_beam.reorder: caches must be [K*B = {K * B}, T, 3D] bfloat16 or float32, got {c0.dtype} {tuple(c0.shape)}')
    T, D = c0.shape[1], c0.shape[2] // 3
    if not 1 <= upto <= T:
        raise ValueError(f'hip_beam.reorder: upto must lie in 1 .. T = {T}, got {upto}')
    if (D * c0.element_size()) % 16 != 0:
        raise ValueError(f'hip_beam.reorder: the hidden size ({D} x {c0.element_size()} bytes) must be a multiple of 16 bytes')
    a = ReorderArgs(parent=_want('parent', parent, torch.int32, (B, K)), L=L, B=B, K=K, T=T, D=D, upto=upto, dtype=_DTYPES[c0.dtype])
    for l, c in enumerate(caches):
        a.cache[l] = _want(f'caches[{l}]', c, c0.dtype, c0.shape)
        if a.cache[l] % 16 != 0:
            raise ValueError(f'hip_beam.reorder: caches[{l}] is not 16-byte aligned')
    _chk(lib().gpv_beam_reorder(C.byref(a), _stream()), 'gpv_beam_reorder')
