"""Answers from a closed set: the phrase set (a trie with a pinned numbering) and the phrase-constrained beam step, stated once on the
host (numpy, fp32 arithmetic in a fixed order): the rule that csrc/phrase_step.hip runs on the device and that include/gpv_phrase.h
repeats.

THE TRIE.  N >= 1 token-id sequences, each of length >= 1, ids in [0, V) and none of pad_id / stop_id / cls_id, pairwise different.  The
root is node 0; nodes are numbered breadth first, the children of a node in ascending token order.  child_off int32 [M+1], child_tok /
child_node int32 [E] (E = M - 1: the edges of node n are child_off[n] .. child_off[n+1] - 1), terminal int32 [M]: the index of the phrase
that ends at the node, or -1.  A phrase may be a prefix of another (a terminal node with children); every leaf is terminal, so a live
hypothesis always has a continuation.

THE STATE per (b, k): node int32 (>= 0 live, DONE = -1 has spelled a phrase and stopped, VOID = -2 holds no hypothesis), phrase int32
(the phrase index once DONE, else -1), seq_lp, seqs, length as in gpv1_amd.beam.  Every slot starts at the root with score 0.

THE RULE.  Step t (0 <= t < T-1), batch element b, parent k1 = 0..K-1, logits row r = k1*B + b:
 1. x_v = fp32(logit[r, v]).  lse_r = m + logf(sum_v expf(x_v - m)), m = max_v x_v, over the WHOLE vocabulary (no mask): an OUTPUT of
    the device step and an INPUT here, exactly as in gpv1_amd.beam, summed in the order include/gpv_beam.h pins (beam.n_chain(V) bounds
    it).  The whole vocabulary, not the allowed set: the score is then the model's log-probability of the phrase followed by __stop__,
    comparable across images and sets.  Only the rows of live parents that have candidates are read; the lse of every other row is 0.
 2. Live parent at node n: the allowed tokens are child_tok[child_off[n] : child_off[n+1]], and stop_id when terminal[n] >= 0.  Its
    candidates are the min(K, |A|) largest x_v over that set, ties to the lower v; k2 is the rank.  lp = x_v - lse_r: one fp32
    subtract.  score = seq_lp[b,k1] + lp: one fp32 add.  len' = length + 1.  v == stop_id: node' = DONE, phrase' = terminal[n]; any
    other v: node' = that child, phrase' = -1.
 3. DONE parent: exactly one candidate, k2 = 0: token pad_id, score and length unchanged, node' = DONE, phrase' carried.
 4. VOID parent: no candidate.  t == 0: a parent k1 > 0 has no candidate (all slots start at the root; only slot 0 counts).
 5-7. Key, selection and slot write are steps 5-7 of gpv1_amd.beam (beam.select_slots), the search's own state being node' and
    phrase'.  With only c < K candidates the slots c..K-1 become VOID: parent 0, token pad_id, seq_lp = -1e9 exactly, node' = VOID,
    phrase' = -1, length' = 0.
Caller conditions: 1 <= K <= 8, 2 <= T <= 64, pset.max_len <= T - 2 (so __stop__ always fits).  Slots come out best first; the finished
slots of one batch element name pairwise different phrases (trie paths are unique).
"""
import hashlib

import numpy as np

from . import beam as _beam

DONE, VOID = -1, -2
VOID_LP = np.float32(-1e9)
F32 = np.float32
MAX_K, MAX_T = _beam.MAX_K, _beam.MAX_T


class PhraseSet:
    """the compiled set: child_off, child_tok, child_node, terminal (numpy int32), M, E, N, max_len, digest"""

    def __init__(self, token_ids, V, pad_id, stop_id, cls_id):
        seqs = [tuple(int(v) for v in s) for s in token_ids]
        if len(seqs) < 1:
            raise ValueError('PhraseSet: at least one phrase is needed')
        self.V, self.pad_id, self.stop_id, self.cls_id = int(V), int(pad_id), int(stop_id), int(cls_id)
        special = {self.pad_id: 'pad_id', self.stop_id: 'stop_id', self.cls_id: 'cls_id'}
        seen = {}
        for i, s in enumerate(seqs):
            if len(s) == 0:
                raise ValueError(f'PhraseSet: phrase {i} is empty')
            for v in s:
                if not 0 <= v < self.V:
                    raise ValueError(f'PhraseSet: phrase {i} holds id {v} outside the vocabulary [0, {self.V})')
                if v in special:
                    raise ValueError(f'PhraseSet: phrase {i} holds id {v}, which is {special[v]}')
            if s in seen:
                raise ValueError(f'PhraseSet: phrases {seen[s]} and {i} are equal')
            seen[s] = i
        self.token_ids = seqs
        self.N = len(seqs)
        self.max_len = max(len(s) for s in seqs)
        # a dict trie first, then the breadth-first numbering
        root = {'kids': {}, 'term': -1}
        for i, s in enumerate(seqs):
            n = root
            for v in s:
                n = n['kids'].setdefault(v, {'kids': {}, 'term': -1})
            n['term'] = i
        order, q = [root], 0
        child_off, child_tok, child_node, terminal = [0], [], [], []
        while q < len(order):
            n = order[q]
            q += 1
            terminal.append(n['term'])
            for v in sorted(n['kids']):
                child_tok.append(v)
                child_node.append(len(order))
                order.append(n['kids'][v])
            child_off.append(len(child_tok))
        self.M, self.E = len(order), len(child_tok)
        self.child_off = np.asarray(child_off, np.int32)
        self.child_tok = np.asarray(child_tok, np.int32)
        self.child_node = np.asarray(child_node, np.int32)
        self.terminal = np.asarray(terminal, np.int32)
        h = hashlib.sha256(repr((self.V, self.pad_id, self.stop_id, self.cls_id, seqs)).encode())
        self.digest = h.hexdigest()[:16]
        self._device = {}

    @classmethod
    def from_texts(cls, model, texts):
        """tokenised with compute_predictions.word_tokenize and model.word_to_idx; a word outside the vocabulary is an error"""
        from .compute_predictions import word_tokenize
        w2i = model.word_to_idx
        ids = []
        for text in texts:
            words = word_tokenize(text)
            for w in words:
                if w not in w2i:
                    raise ValueError(f'PhraseSet.from_texts: {text!r}: the word {w!r} is not in the vocabulary')
            ids.append([w2i[w] for w in words])
        pset = cls(ids, len(model.vocab), w2i['__pad__'], w2i['__stop__'], w2i['__cls__'])
        pset.texts = list(texts)
        return pset

    def device_arrays(self, device):
        """(child_off, child_tok, child_node, terminal) as int32 tensors on `device`, made once per device"""
        import torch
        key = str(torch.device(device))
        got = self._device.get(key)
        if got is None:
            got = self._device[key] = tuple(torch.from_numpy(a.copy()).to(device) for a in
                                            (self.child_off, self.child_tok, self.child_node, self.terminal))
        return got

    def allowed(self, n):
        """-> [(token, node', phrase')] of node n, __stop__ included at a terminal node"""
        e0, e1 = int(self.child_off[n]), int(self.child_off[n + 1])
        out = [(int(self.child_tok[e]), int(self.child_node[e]), -1) for e in range(e0, e1)]
        if self.terminal[n] >= 0:
            out.append((self.stop_id, DONE, int(self.terminal[n])))
        return out


def check_extents(K, T, pset, t=None):
    if not 1 <= K <= MAX_K:
        raise ValueError(f'phrases: 1 <= beam size <= {MAX_K} is supported, got {K}')
    if not 2 <= T <= MAX_T:
        raise ValueError(f'phrases: 2 <= max_text_len <= {MAX_T} is supported, got {T}')
    if pset.max_len > T - 2:
        raise ValueError(f'phrases: the longest phrase has {pset.max_len} tokens, max_text_len {T} leaves room for {T - 2} and __stop__')
    if t is not None and not 0 <= t < T - 1:
        raise ValueError(f'phrases: step {t} outside 0 .. {T - 2}')


def phrase_step_host(logits, lse, seq_lp, seqs, node, phrase, length, t, pad_id, stop_id, pset, inv_pen=None):
    """One step.  logits [K*B, V] (values exactly representable in fp32), lse [K*B] fp32 (the device's, or beam.lse_host), seq_lp [B,K]
    fp32, seqs [K,B,T] int64, node / phrase / length [B,K] int.  Nothing is modified.
    -> dict(parent, tok, seqs, seq_lp, node, phrase, length), shapes and dtypes as the device writes them"""
    x = np.asarray(logits, dtype=F32)
    K, B, T = seqs.shape
    V = x.shape[1]
    check_extents(K, T, pset, t)
    if x.shape[0] != K * B or V != pset.V:
        raise ValueError(f'phrases: logits must be [K*B = {K * B}, V = {pset.V}], got {x.shape}')
    if (pad_id, stop_id) != (pset.pad_id, pset.stop_id):
        raise ValueError(f'phrases: pad_id / stop_id {pad_id} / {stop_id} are not the set\'s ({pset.pad_id} / {pset.stop_id})')
    lse = np.asarray(lse, dtype=F32)
    seq_lp = np.asarray(seq_lp, dtype=F32)
    out = {'parent': np.zeros((B, K), np.int32), 'tok': np.zeros(K * B, np.int64), 'seqs': np.array(seqs, dtype=np.int64),
           'seq_lp': np.zeros((B, K), F32), 'node': np.zeros((B, K), np.int32), 'phrase': np.zeros((B, K), np.int32),
           'length': np.zeros((B, K), np.int32)}
    void = {'k1': 0, 'w': pad_id, 'seq_lp': VOID_LP, 'length': 0, 'node': VOID, 'phrase': -1}
    for b in range(B):
        cands = []                                                   # in k1*K + k2 order
        for k1 in range(K):
            r = k1 * B + b
            n = int(node[b, k1])
            if n == VOID or (t == 0 and k1 > 0):
                continue
            if n == DONE:
                found = [(pad_id, seq_lp[b, k1], int(length[b, k1]), DONE, int(phrase[b, k1]))]
            else:
                al = sorted(pset.allowed(n), key=lambda c: (-float(x[r, c[0]]), c[0]))[:K]     # K largest, ties to the lower v
                found = []
                for w, n2, p2 in al:
                    lp = F32(x[r, w] - lse[r])                       # one fp32 subtract
                    found.append((w, F32(seq_lp[b, k1] + lp), int(length[b, k1]) + 1, n2, p2))     # one fp32 add
            cands += [{'k1': k1, 'w': w, 'seq_lp': score, 'length': ln, 'node': n2, 'phrase': p2} for w, score, ln, n2, p2 in found]
        _beam.select_slots(out, b, cands, seqs, t, inv_pen, default=void)   # steps 5-7
    return out


def initial_state(B, K, T):
    """every slot at the root with score 0"""
    return {'seq_lp': np.zeros((B, K), F32), 'seqs': np.zeros((K, B, T), np.int64), 'node': np.zeros((B, K), np.int32),
            'phrase': np.full((B, K), -1, np.int32), 'length': np.zeros((B, K), np.int32)}


def phrase_search_host(step_logits_fn, B, K, T, pset, alpha=0.0):
    """The chained search: step_logits_fn(t, tok [K,B,t+1] int64) -> logits [K*B, V] of the newest position (row k*B + b continues the
    hypothesis in slot k of batch element b; tok[:, :, 0] = cls_id).  -> dict(seqs, seq_lp, node, phrase, length, keys [B,K])"""
    check_extents(K, T, pset)
    inv_pen = _beam.length_table(T, alpha) if alpha else None
    st = initial_state(B, K, T)
    tok = np.full((K, B, 1), pset.cls_id, np.int64)
    bi = np.arange(B)
    for t in range(T - 1):
        logits = np.asarray(step_logits_fn(t, tok), dtype=F32)
        o = phrase_step_host(logits, _beam.lse_host(logits), st['seq_lp'], st['seqs'], st['node'], st['phrase'], st['length'], t,
                             pset.pad_id, pset.stop_id, pset, inv_pen=inv_pen)
        tok = np.concatenate((tok[o['parent'].T, bi[None, :]], o['tok'].reshape(K, B, 1)), axis=-1)
        st = {k: o[k] for k in st}
    keys = st['seq_lp'] if inv_pen is None else (st['seq_lp'] * inv_pen[np.clip(st['length'], 0, T)]).astype(F32)
    return dict(st, keys=keys)
