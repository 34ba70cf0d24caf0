"""TEST-ONLY inputs of the phrase-constrained beam step, shared by tests/test_phrase_rule_cpu.py and tests/test_phrase_gpu.py: phrase
sets with the trie shapes the rule has to get right, random logits (3 * randn rounded to the logits dtype, so bf16 brings natural
ties), a consistent search state and the planted situations."""
import numpy as np
import torch

VARIANTS = ('wide_root', 'one_child', 'prefix', 'few', 'mixed', 'twins', 'stop_top', 'penalty')


def ids(V):
    """(pad_id, stop_id, cls_id) laid out like the model's vocabulary (specials last)"""
    return V - 4, V - 2, V - 3


def ordinary(V):
    pad_id, stop_id, cls_id = ids(V)
    return [v for v in range(V) if v not in (pad_id, stop_id, cls_id)]


def make_set(variant, V, K, T, seed=0):
    """a PhraseSet (phrases of at most T - 2 tokens) of the trie shape `variant` names"""
    from gpv1_amd.phrases import PhraseSet
    rs = np.random.RandomState(seed)
    words = ordinary(V)
    L = T - 2
    if variant == 'wide_root':                 # 300 children of the root (as many as the vocabulary has, if fewer): more than 256 lanes
        first = rs.permutation(words)[:300].tolist()
        phrases = [[w] for w in first]
        if L > 1:
            phrases += [[first[0], first[1]], [first[0], first[2]], [first[5], first[5]]]
    elif variant == 'one_child':               # a chain: every inner node has exactly one child
        a, b, c = rs.permutation(words)[:3].tolist()
        phrases = [[a] * L, [b] + [c] * (L - 1)] if L > 1 else [[a], [b]]
    elif variant == 'few':                     # fewer phrases than K: VOID slots
        phrases = [[w] for w in rs.permutation(words)[:max(1, K - 2)].tolist()]
    else:                                      # terminal nodes that also have children, a dozen phrases of mixed length
        base = rs.permutation(words)[:8].tolist()
        phrases = [[w] for w in base[:5]]
        if L > 1:
            phrases += [[base[0], base[1]], [base[0], base[2]], [base[1], base[0]], [base[5], base[6]], [base[5], base[7]], [base[6], base[6]]]
        if L > 2:
            phrases += [[base[0], base[1], base[3]], [base[5], base[6], base[0]]]
    pad_id, stop_id, cls_id = ids(V)
    return PhraseSet(phrases, V, pad_id, stop_id, cls_id)


def nodes_at_depth(pset):
    depth = np.zeros(pset.M, np.int64)
    for n in range(pset.M):
        for e in range(pset.child_off[n], pset.child_off[n + 1]):
            depth[pset.child_node[e]] = depth[n] + 1
    return depth


def make_case(seed, B, K, V, T, t, dtype=torch.float32, variant='prefix'):
    """-> dict: pset, logits (torch, dtype, [K*B, V]), x (the same values as fp32 numpy), seq_lp, seqs, node, phrase, length (numpy),
    inv_pen (numpy fp32 or None), pad_id, stop_id, t.  The state is one a search can reach: at t == 0 every slot at the root, later
    live slots at a node of depth <= t that still has room for its longest continuation, with DONE and VOID slots for 'mixed'."""
    from gpv1_amd import beam, phrases as P
    pset = make_set(variant if variant in ('wide_root', 'one_child', 'few') else 'prefix', V, K, T, seed)
    g = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    logits = (3.0 * torch.randn(K * B, V, generator=g)).to(dtype)
    pad_id, stop_id, _ = ids(V)
    st = P.initial_state(B, K, T)
    seq_lp, seqs, node, phrase, length = st['seq_lp'], st['seqs'], st['node'], st['phrase'], st['length']
    if t > 0:
        depth = nodes_at_depth(pset)
        # a live node at depth d after t steps needs d == t; deeper steps than the trie has leave only DONE and VOID slots
        at = [n for n in range(pset.M) if depth[n] == t]
        term = [n for n in range(pset.M) if pset.terminal[n] >= 0 and depth[n] < t]
        for b in range(B):
            for k in range(K):
                kind = rs.randint(0, 3) if variant == 'mixed' else (0 if at else 1)
                if variant == 'few' and k >= pset.N:
                    kind = 2
                if kind == 0 and at:
                    node[b, k], length[b, k] = at[rs.randint(len(at))], t
                    seq_lp[b, k] = -5.0 * rs.rand()
                elif kind <= 1 and term:
                    n = term[rs.randint(len(term))]
                    node[b, k], phrase[b, k], length[b, k] = P.DONE, pset.terminal[n], depth[n] + 1
                    seq_lp[b, k] = -5.0 * rs.rand()
                else:
                    node[b, k], phrase[b, k], length[b, k], seq_lp[b, k] = P.VOID, -1, 0, P.VOID_LP
        if variant == 'mixed' and K >= 3 and at and term:            # one of each kind for certain
            n = term[0]
            node[0, 0], phrase[0, 0], length[0, 0], seq_lp[0, 0] = P.DONE, pset.terminal[n], depth[n] + 1, -1.5
            node[0, 1], phrase[0, 1], length[0, 1], seq_lp[0, 1] = at[0], -1, t, -2.5
            node[0, 2], phrase[0, 2], length[0, 2], seq_lp[0, 2] = P.VOID, -1, 0, P.VOID_LP
        seqs[:, :, :t] = rs.randint(0, V, (K, B, t))
    live = [(b, k) for b in range(B) for k in range(K) if node[b, k] >= 0 and (t > 0 or k == 0)]
    if variant == 'twins' and K > 1 and t > 0 and live:             # two parents with identical rows, nodes and scores: ties across k1
        b = live[0][0]
        logits[(K - 1) * B + b] = logits[0 * B + b]
        for arr in (seq_lp, node, phrase, length):
            arr[b, K - 1] = arr[b, 0]
    if variant == 'stop_top' and live:                              # __stop__ above everything in the rows of the live parents
        for b, k in live:
            logits[k * B + b, stop_id] = logits[k * B + b].max() + 2
    if live and pset.E > 1:                                         # and a tie between two allowed tokens of one live parent
        b, k = live[-1]
        al = [c[0] for c in pset.allowed(int(node[b, k]))]
        if len(al) > 1:
            logits[k * B + b, al[-1]] = logits[k * B + b, al[0]] = logits[k * B + b, al].max() + 1
    inv_pen = beam.length_table(T, 0.6) if variant == 'penalty' else None
    return {'pset': pset, 'logits': logits, 'x': logits.float().numpy().copy(), 'seq_lp': seq_lp, 'seqs': seqs, 'node': node, 'phrase': phrase,
            'length': length, 'inv_pen': inv_pen, 'pad_id': pad_id, 'stop_id': stop_id, 't': t}


INT_KEYS = ('parent', 'tok', 'seqs', 'node', 'phrase', 'length')


def same(a, b):
    """bit-equality of two step results: integers equal, floats equal as bit patterns"""
    for k in INT_KEYS:
        if not np.array_equal(np.asarray(a[k], dtype=np.int64), np.asarray(b[k], dtype=np.int64)):
            return False, k
    x, y = np.asarray(a['seq_lp'], dtype=np.float32), np.asarray(b['seq_lp'], dtype=np.float32)
    if not np.array_equal(x.view(np.uint32), y.view(np.uint32)):
        return False, 'seq_lp'
    return True, None


def prefix_logits(V, seed, dtype=np.float32):
    """a prefix-dependent step_logits_fn for phrase_search_host: the row of a hypothesis is a deterministic function of its tokens"""
    def fn(t, tok):
        K, B, _ = tok.shape
        out = np.zeros((K * B, V), np.float32)
        for k in range(K):
            for b in range(B):
                h = seed + 7919 * b
                for w in tok[k, b]:
                    h = (h * 1000003 + int(w) + 1) % 2147483647
                out[k * B + b] = (3.0 * np.random.RandomState(h % (2 ** 31 - 1)).randn(V)).astype(np.float32)
        return out
    return fn
