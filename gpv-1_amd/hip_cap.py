"""ctypes binding of libgpv_cap.so (C ABI in include/gpv_cap.h): device-side Bleu / CIDEr-D caption scoring.

Same rules as ``hip``: no CPU / eager fallback -- a missing library or a CPU tensor is an error.
"""
import ctypes as C
from functools import partial

import torch

from . import _native
from .hip import _chk, _p, _stream

EXPORTS = ['gpv_cap_scores']
ORDERS = 4
MAX_LEN = 64          # GPV_CAP_MAX_LEN: words per caption
MAX_REFS = 8          # GPV_CAP_MAX_REFS: references per entry
MAX_WORD = 65535      # GPV_CAP_MAX_WORD: largest word id (0 is padding)
ERR_BITS = {1: 'the n-gram table is full (capacity too small for the references)',
            2: f'a word id inside a caption is outside 1..{MAX_WORD}',
            4: 'a reference n-gram was not found in the table'}
_LIB = None
_LIB_PATH = _native.lib_path('cap')
_SIGNATURES = {'gpv_cap_scores': ([C.c_void_p] * 5 + [C.c_int] * 4 + [C.c_void_p] * 2 + [C.c_int] + [C.c_void_p] * 2 + [C.c_longlong] +
                                  [C.c_void_p] * 8)}
_want = partial(_native.want, 'caption_scores')


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _native.load('cap', _SIGNATURES, _LIB_PATH)
    return _LIB


def table_capacity(occurrences):
    """the power of two >= max(2, 2 * occurrences): slots of the n-gram table for that many reference n-gram occurrences"""
    cap = 2
    while cap < 2 * int(occurrences):
        cap *= 2
    return cap


def check_error(err_word):
    """raise if the error word of a finished call (a Python int, after the device-to-host copy) is not 0"""
    if int(err_word) != 0:
        raise RuntimeError('gpv1_amd: gpv_cap_scores reported: ' + '; '.join(m for b, m in ERR_BITS.items() if int(err_word) & b))


def caption_scores(hyp, hyp_len, ref, ref_len, ref_count, weight, pen, occurrences=None, testlen=None, reflen=None, guess=None, correct=None,
                   cider=None, err=None, ref_df=False):
    """gpv_cap_scores on the current stream: two memsets-and-launches, no sync.  hyp [N,LH] int32 word ids (0 = padding), hyp_len [N],
    ref [N,R,LR], ref_len [N,R], ref_count [N] int32; weight [N+1], pen [>= max(LH, LR)] float64 (evaluators.caption_tables).
    occurrences: an upper bound of the number of reference n-gram occurrences (the table gets >= twice as many slots); default: the
    bound of the shape, N * R * 4 * LR.  Outputs are allocated when not given (contiguous views of one buffer work);
    ref_df=True also returns the [N,R,4,LR] document frequencies (for the tests).
    -> (testlen [N], reflen [N], guess [N,4], correct [N,4] int32, cider [N] float64, err [1] int32, ref_df or None).
    The caller checks ``err`` after its device-to-host copy (``check_error``): nothing is synchronised here."""
    if hyp.dim() != 2 or ref.dim() != 3 or ref.shape[0] != hyp.shape[0]:
        raise ValueError(f'caption_scores: hyp must be [N,LH] and ref [N,R,LR], got {tuple(hyp.shape)} {tuple(ref.shape)}')
    N, LH = hyp.shape
    _, R, LR = ref.shape
    if not (1 <= LH <= MAX_LEN and 1 <= LR <= MAX_LEN):
        raise ValueError(f'caption_scores: captions of up to {MAX_LEN} words are supported (GPV_CAP_MAX_LEN), got LH = {LH}, LR = {LR}; '
                         f'nothing is truncated')
    if not 1 <= R <= MAX_REFS:
        raise ValueError(f'caption_scores: 1..{MAX_REFS} references per entry are supported (GPV_CAP_MAX_REFS), got R = {R}')
    if pen.dim() != 1 or pen.shape[0] < max(LH, LR):
        raise ValueError(f'caption_scores: pen must hold at least max(LH, LR) = {max(LH, LR)} entries, got {tuple(pen.shape)}')
    bound = N * R * ORDERS * LR
    capacity = table_capacity(bound if occurrences is None else min(int(occurrences), bound))
    dev = hyp.device
    args_in = (_want('hyp', hyp, torch.int32, (N, LH)), _want('hyp_len', hyp_len, torch.int32, (N,)),
               _want('ref', ref, torch.int32, (N, R, LR)), _want('ref_len', ref_len, torch.int32, (N, R)),
               _want('ref_count', ref_count, torch.int32, (N,)), N, LH, R, LR,
               _want('weight', weight, torch.float64, (N + 1,)), _want('pen', pen, torch.float64, (pen.shape[0],)), int(pen.shape[0]))
    i32 = lambda *s: torch.empty(*s, dtype=torch.int32, device=dev)
    testlen = i32(N) if testlen is None else testlen
    reflen = i32(N) if reflen is None else reflen
    guess = i32(N, ORDERS) if guess is None else guess
    correct = i32(N, ORDERS) if correct is None else correct
    cider = torch.empty(N, dtype=torch.float64, device=dev) if cider is None else cider
    err = torch.zeros(1, dtype=torch.int32, device=dev) if err is None else err
    df_out = i32(N, R, ORDERS, LR) if ref_df else None
    keys = torch.empty(capacity, dtype=torch.int64, device=dev)
    counts = i32(capacity)
    args = args_in + (_p(keys), _p(counts), capacity,
                      _want('testlen', testlen, torch.int32, (N,)), _want('reflen', reflen, torch.int32, (N,)),
                      _want('guess', guess, torch.int32, (N, ORDERS)), _want('correct', correct, torch.int32, (N, ORDERS)),
                      _want('cider', cider, torch.float64, (N,)), None if df_out is None else _p(df_out), _want('err', err, torch.int32, (1,)))
    _chk(lib().gpv_cap_scores(*args, _stream()), 'gpv_cap_scores')
    return testlen, reflen, guess, correct, cider, err, df_out
