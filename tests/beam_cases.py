"""TEST-ONLY inputs of one beam step, shared by tests/test_beam_rule_cpu.py and tests/test_beam_gpu.py: random logits (3 * randn rounded
to the logits dtype, so bf16 brings natural ties) and a consistent search state, with the planted situations the rule has to get right."""
import numpy as np
import torch

PLANTS = ('dupmax', 'twins', 'stop_top', 'mixed_fin')


def ids(V):
    """(pad_id, stop_id) laid out like the model's vocabulary (specials last), folded into tiny vocabularies"""
    return max(V - 4, 0), max(V - 2, 0)


def make_case(seed, B, K, V, T, t, dtype=torch.float32, plants=(), masked=False, penalty=None):
    """-> dict: logits (torch, dtype, [K*B, V]), x (the same values as fp32 numpy), seq_lp, seqs, finished, length (numpy), vocab_mask,
    inv_pen (numpy fp32 or None), pad_id, stop_id, t"""
    from gpv1_amd import beam as rule
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    logits = (3.0 * torch.randn(K * B, V, generator=g)).to(dtype)
    pad_id, stop_id = ids(V)
    seq_lp = np.zeros((B, K), np.float32) if t == 0 else (-5.0 * rs.rand(B, K)).astype(np.float32)
    seqs = np.zeros((K, B, T), np.int64)
    seqs[:, :, :t] = rs.randint(0, V, (K, B, t))
    finished = np.zeros((B, K), np.int32)
    length = np.full((B, K), t, np.int32)
    if 'mixed_fin' in plants and t > 0:
        finished = (rs.rand(B, K) < 0.5).astype(np.int32)
        finished[0, 0] = 1
        finished[0, K - 1] = 0 if K > 1 else 1
        length = np.where(finished != 0, rs.randint(1, t + 1, (B, K)), t).astype(np.int32)
    if 'dupmax' in plants and V > 1:                       # the row maximum twice: the lower index is rank 0, the other rank 1
        r = rs.randint(0, K * B)
        i, j = rs.choice(V, 2, replace=False)
        logits[r, i] = logits[r, j] = logits[r].max() + 1
    if 'twins' in plants and K > 1:                         # two parents with identical rows and identical seq_lp: ties across k1
        b = rs.randint(0, B)
        logits[(K - 1) * B + b] = logits[0 * B + b]
        seq_lp[b, K - 1] = seq_lp[b, 0]
        finished[b, K - 1], length[b, K - 1] = finished[b, 0], length[b, 0]
    if 'stop_top' in plants:                                # __stop__ as a row's top-1
        r = rs.randint(0, K * B)
        logits[r, stop_id] = logits[r].max() + 2
    vocab_mask = None
    if masked:                                              # leaves K + 2 finite entries (as many as the vocabulary has, if fewer)
        keep = rs.choice(V, min(V, K + 2), replace=False)
        vocab_mask = np.full(V, -np.inf, np.float32)
        vocab_mask[keep] = (rs.rand(len(keep)) < 0.5).astype(np.float32) * -0.5
    inv_pen = None if penalty is None else rule.length_table(T, penalty)
    return {'logits': logits, 'x': logits.float().numpy().copy(), 'seq_lp': seq_lp, 'seqs': seqs, 'finished': finished, 'length': length,
            'vocab_mask': vocab_mask, 'inv_pen': inv_pen, 'pad_id': pad_id, 'stop_id': stop_id, 't': t}


def same(a, b):
    """bit-equality of two step results (dicts of arrays / nested lists): integers equal, floats equal as bit patterns"""
    for k in ('parent', 'tok', 'seqs', 'finished', 'length'):
        if not np.array_equal(np.asarray(a[k], dtype=np.int64), np.asarray(b[k], dtype=np.int64)):
            return False, k
    x, y = np.asarray(a['seq_lp'], dtype=np.float32), np.asarray(b['seq_lp'], dtype=np.float32)
    if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
        return False, 'seq_lp'
    return True, None
