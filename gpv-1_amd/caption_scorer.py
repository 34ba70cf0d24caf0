"""Caption scorer for train-time evaluation: Bleu1..4 and CIDEr-D of a set of predictions, on the device.

``CaptionScorer()`` is the hook ``metrics.cap_metrics(..., scorer=)`` and an evaluation dataset's ``scorer`` attribute take:
``scorer(samples, predictions) -> {'Bleu1', 'Bleu2', 'Bleu3', 'Bleu4', 'Cider'}``.  Pairing and tokenisation are
``evaluators.CocoCaptioning``'s; the rule is ``evaluators.caption_scores_host`` (module docstring there), which ``host=True`` runs as
it stands -- the comparison path.  The device path (csrc/caption_score.hip through ``hip_cap``) maps the words of everything being
scored to ids 1.. on the host, uploads the id arrays and the two float64 tables in ONE copy, launches on the current stream and
reads every per-entry result back in ONE copy; the corpus Bleu (from int64 sums) and the CIDEr mean are finished on the host in
float64 by the same ``evaluators.caption_result`` the host rule ends in.  No CPU fallback: without the library or a GPU the device
path raises.
"""
import numpy as np
import torch

from . import evaluators

ORDERS = evaluators.CAP_ORDERS


def encode_captions(hyps, refs):
    """words -> ids over everything being scored: hyp [N,LH], hyp_len [N], ref [N,R,LR], ref_len [N,R], ref_count [N] (int32 numpy,
    0 = padding, ids from 1 in order of first appearance) and the number of reference n-gram occurrences.  Raises where a limit of
    include/gpv_cap.h is exceeded: nothing is truncated."""
    from . import hip_cap
    N = len(hyps)
    if len(refs) != N or any(len(r) == 0 for r in refs):
        raise ValueError('CaptionScorer: every entry needs a hypothesis and at least one reference')
    longest = max([len(h) for h in hyps] + [len(r) for rs in refs for r in rs] + [1])
    R = max([len(rs) for rs in refs] + [1])
    if longest > hip_cap.MAX_LEN:
        raise ValueError(f'CaptionScorer: a caption has {longest} words, the device scorer takes up to {hip_cap.MAX_LEN} '
                         f'(GPV_CAP_MAX_LEN); use host=True for such captions')
    if R > hip_cap.MAX_REFS:
        raise ValueError(f'CaptionScorer: an entry has {R} references, the device scorer takes up to {hip_cap.MAX_REFS} '
                         f'(GPV_CAP_MAX_REFS); use host=True for such entries')
    LH = max([len(h) for h in hyps] + [1])
    LR = max([len(r) for rs in refs for r in rs] + [1])
    ids = {}
    hyp, hyp_len = np.zeros((N, LH), dtype=np.int32), np.zeros(N, dtype=np.int32)
    ref, ref_len, ref_count = np.zeros((N, R, LR), dtype=np.int32), np.zeros((N, R), dtype=np.int32), np.zeros(N, dtype=np.int32)
    encoded = {}                                     # a reference list shared by several entries (one image) is encoded once
    occurrences = 0
    for i, (h, rs) in enumerate(zip(hyps, refs)):
        hyp[i, :len(h)] = [ids.setdefault(w, len(ids) + 1) for w in h]
        hyp_len[i] = len(h)
        got = encoded.get(id(rs))
        if got is None:
            rows, lens = np.zeros((R, LR), dtype=np.int32), np.zeros(R, dtype=np.int32)
            for j, r in enumerate(rs):
                rows[j, :len(r)] = [ids.setdefault(w, len(ids) + 1) for w in r]
                lens[j] = len(r)
            occ = int(sum(max(0, len(r) - n) for r in rs for n in range(ORDERS)))
            got = encoded[id(rs)] = (rows, lens, occ)
        ref[i], ref_len[i], ref_count[i] = got[0], got[1], len(rs)
        occurrences += got[2]
    if len(ids) > hip_cap.MAX_WORD:
        raise ValueError(f'CaptionScorer: {len(ids)} distinct words, the device scorer packs an n-gram into 64 bits and takes up to '
                         f'{hip_cap.MAX_WORD} (GPV_CAP_MAX_WORD); use host=True')
    return hyp, hyp_len, ref, ref_len, ref_count, occurrences


def caption_scores_device(hyps, refs, device=None, ref_df=False):
    """``evaluators.caption_scores_host`` on the device: the same arguments, the same result dict (without 'df'; with 'ref_df'
    [N,R,4,LR] when asked).  One upload, the launches on the current stream, one device-to-host copy."""
    from . import hip_cap
    hip_cap.lib()
    dev = torch.device('cuda' if device is None else device)
    if dev.type != 'cuda':
        raise RuntimeError('gpv1_amd: the device caption scorer needs a GPU (no CPU path exists); CaptionScorer(host=True) is the host rule')
    hyp, hyp_len, ref, ref_len, ref_count, occurrences = encode_captions(hyps, refs)
    N, LH = hyp.shape
    _, R, LR = ref.shape
    if N == 0:
        return evaluators.caption_result([], [], [], [], [])
    weight, pen = evaluators.caption_tables(N, max(LH, LR))
    # one upload: the float64 tables first (8-byte aligned), then the int32 arrays
    parts = [weight, pen, hyp, hyp_len, ref, ref_len, ref_count]
    blob = np.concatenate([np.ascontiguousarray(a).reshape(-1).view(np.uint8) for a in parts])
    with torch.cuda.device(dev):
        dblob = torch.from_numpy(blob).to(dev)
        views, at = [], 0
        for a in parts:
            views.append(dblob[at:at + a.nbytes].view(torch.float64 if a.dtype == np.float64 else torch.int32).view(a.shape))
            at += a.nbytes
        d_weight, d_pen, d_hyp, d_hyp_len, d_ref, d_ref_len, d_ref_count = views
        # one result buffer: cider [N] float64, then testlen [N], reflen [N], guess [N,4], correct [N,4], err [1] int32
        out = torch.empty(8 * N + 4 * (10 * N + 1), dtype=torch.uint8, device=dev)
        cider = out[:8 * N].view(torch.float64)
        ints = out[8 * N:].view(torch.int32)
        testlen, reflen = ints[:N], ints[N:2 * N]
        guess, correct = ints[2 * N:6 * N].view(N, ORDERS), ints[6 * N:10 * N].view(N, ORDERS)
        err = ints[10 * N:10 * N + 1]
        res = hip_cap.caption_scores(d_hyp, d_hyp_len, d_ref, d_ref_len, d_ref_count, d_weight, d_pen, occurrences=occurrences,
                                     testlen=testlen, reflen=reflen, guess=guess, correct=correct, cider=cider, err=err, ref_df=ref_df)
        host = out.cpu().numpy()                                        # the one device-to-host copy (waits for the stream)
        df_host = res[6].cpu().numpy() if ref_df else None              # (tests only)
    h_cider = host[:8 * N].view(np.float64)
    h_ints = host[8 * N:].view(np.int32)
    hip_cap.check_error(h_ints[10 * N])
    result = evaluators.caption_result(h_ints[:N], h_ints[N:2 * N], h_ints[2 * N:6 * N].reshape(N, ORDERS),
                                       h_ints[6 * N:10 * N].reshape(N, ORDERS), h_cider.copy())
    if ref_df:
        result['ref_df'] = df_host
    return result


class CaptionScorer:
    """scorer(samples, predictions) -> {'Bleu1', 'Bleu2', 'Bleu3', 'Bleu4', 'Cider'} (python floats).
    device: where the kernels run (default: the current CUDA device); host=True: evaluators.caption_scores_host instead;
    tokenize: str -> list of words (default evaluators.simple_caption_tokenize -- NOT the PTB tokenizer, see there)."""

    def __init__(self, device=None, host=False, tokenize=evaluators.simple_caption_tokenize):
        self.device, self.host, self.tokenize = device, bool(host), tokenize

    def scores(self, hyps, refs):
        """(hyps, refs) of word lists -> the full result dict of the chosen path"""
        if self.host:
            return evaluators.caption_scores_host(hyps, refs)
        return caption_scores_device(hyps, refs, self.device)

    def evaluate(self, samples, predictions, novelty='everything'):
        """-> the reference's layout {'absent', 'total', 'scores'}"""
        return evaluators.CocoCaptioning(samples, predictions, None, tokenize=self.tokenize, scores=self.scores).evaluate(novelty)

    def __call__(self, samples, predictions):
        return {k: float(v) for k, v in self.evaluate(samples, predictions)['scores'].items()}
