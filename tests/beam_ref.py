"""TEST-ONLY second restatement of the beam step rule (gpv1_amd.beam.beam_step_host / include/gpv_beam.h) in another shape: no array
operations, plain Python tuples, `sorted` with an explicit key, numpy fp32 scalars for the four roundings (mask add, subtract, add,
multiply).  Written from the rule's text, not from beam.py: the two are compared exactly in tests/test_beam_rule_cpu.py."""
import numpy as np

f32 = np.float32
EXTEND, FREEZE = 0, 1


def step(logits, lse, seq_lp, seqs, finished, length, t, mode, pad_id, stop_id, inv_pen=None, vocab_mask=None):
    K, B, T = len(seqs), len(seqs[0]), len(seqs[0][0])
    V = len(logits[0])
    new_seqs = [[[int(seqs[k][b][p]) for p in range(T)] for b in range(B)] for k in range(K)]
    parent = [[0] * K for _ in range(B)]
    new_lp = [[f32(0)] * K for _ in range(B)]
    new_fin = [[0] * K for _ in range(B)]
    new_len = [[0] * K for _ in range(B)]
    tok = [0] * (K * B)
    for b in range(B):
        pool = []
        for k1 in range(K):
            r = k1 * B + b
            done = int(finished[b][k1]) != 0
            grown = int(length[b][k1]) + (0 if done else 1)
            if mode == FREEZE and done:
                pool.append({'k1': k1, 'k2': 0, 'w': pad_id, 'score': f32(seq_lp[b][k1]), 'len': grown})
                continue
            row = [f32(logits[r][v]) if vocab_mask is None else f32(f32(logits[r][v]) + f32(vocab_mask[v])) for v in range(V)]
            best = sorted(range(V), key=lambda v: (-float(row[v]), v))[:K]
            for k2, v in enumerate(best):
                lp = f32(row[v] - f32(lse[r]))
                score = f32(f32(seq_lp[b][k1]) + lp)
                if t == 0 and k1 > 0:
                    score = f32(-1e9)
                pool.append({'k1': k1, 'k2': k2, 'w': v, 'score': score, 'len': grown})
        for c in pool:
            c['key'] = c['score'] if inv_pen is None else f32(c['score'] * f32(inv_pen[min(max(c['len'], 0), T)]))
        ranked = sorted(pool, key=lambda c: (-float(c['key']), c['k1'] * K + c['k2']))
        for k, c in enumerate(ranked[:K]):
            parent[b][k] = c['k1']
            new_lp[b][k] = c['score']
            for p in range(t):
                new_seqs[k][b][p] = int(seqs[c['k1']][b][p])
            new_seqs[k][b][t] = c['w']
            tok[k * B + b] = c['w']
            new_fin[b][k] = 1 if (mode == FREEZE and (int(finished[b][c['k1']]) != 0 or c['w'] == stop_id)) else 0
            new_len[b][k] = c['len']
    return {'parent': parent, 'tok': tok, 'seqs': new_seqs, 'seq_lp': new_lp, 'finished': new_fin, 'length': new_len}
