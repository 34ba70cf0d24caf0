"""TEST-ONLY inputs of one sampled step (mode GPV_BEAM_SAMPLE), shared by tests/test_sample_rule_cpu.py and tests/test_sample_gpu.py:
the logits and the state of tests/beam_cases.make_case with the situations the sampler has to get right planted on top."""
import numpy as np
import torch

from tests.beam_cases import make_case, same as same_state


def make_sample_case(seed, B, K, V, T, t, C, dtype=torch.float32, masked=False, plants=True, one_lane=False):
    """-> the dict of beam_cases.make_case plus top_k.  plants: equal logits across the rank C-1 / C boundary of one row (the lower v
    is the last candidate, the other is none), one finished slot, __stop__ as one row's top candidate.  masked: a mask that leaves
    C + 2 finite entries (as many as the vocabulary has, if fewer).  one_lane: the C largest values of every row sit at v = 3,
    3 + 256, ..., all owned by lane 3 of the kernel (a lane's list holds eight: the case a one-scan kernel gets wrong)."""
    case = make_case(seed, B, K, V, T, t, dtype)
    rs = np.random.RandomState(seed + 1)
    lg = case['logits']
    R = K * B
    if one_lane:
        assert 3 + 256 * (C - 1) < V
        for r in range(R):
            top = float(lg[r].max())
            for i in range(C):                                       # descending in i with one tie pair (ranks 4 and 5: the lower v first)
                lg[r, 3 + 256 * i] = top + 1.0 + 0.25 * (C - (i if i != 5 else 4))
    keep = None
    if masked:
        keep = rs.choice(V, min(V, C + 2), replace=False)
        vm = np.full(V, -np.inf, np.float32)
        vm[keep] = (rs.rand(len(keep)) < 0.5).astype(np.float32) * -0.5
        case['vocab_mask'] = vm
    if plants:
        if C < V and not one_lane and not masked:                    # a tie across the boundary of the candidate set
            r = int(rs.randint(0, R))
            order = np.argsort(-lg[r].float().numpy(), kind='stable')
            lg[r, order[C]] = lg[r, order[C - 1]]
        r = int(rs.randint(0, R))                                    # __stop__ as a row's top candidate (inside the mask's kept set, if any)
        if keep is None or case['stop_id'] in keep:
            lg[r, case['stop_id']] = lg[r].max() + 2
        case['finished'][0, 0] = 1                                   # one finished slot: emits pad_id, keeps score and length
        case['length'][0, 0] = max(t - 1, 0)
    case['x'] = lg.float().numpy().copy()
    case['top_k'] = C
    return case


def host_inputs(case, inv_temp=None):
    """(lse, cand_w) of the case as a host computes them: float64 log-sum-exp of the rows after step 1 and np.exp(lp), both rounded to fp32"""
    from gpv1_amd import beam as rule
    F32 = np.float32
    x = case['x'] if inv_temp is None else case['x'] * F32(inv_temp)
    lse = rule.lse_host(x, case['vocab_mask'])
    if case['vocab_mask'] is not None:
        x = x + case['vocab_mask'][None, :]
    top = -np.sort(-x, axis=1, kind='stable')[:, :case['top_k']]
    lp = (top - lse[:, None]).astype(F32)
    return lse, np.exp(lp).astype(F32)


def same(a, b):
    """bit-equality of two sampled-step results: the state of beam_cases.same and the candidates"""
    ok, what = same_state(a, b)
    if ok and not np.array_equal(np.asarray(a['cand_v'], dtype=np.int64), np.asarray(b['cand_v'], dtype=np.int64)):
        return False, 'cand_v'
    return ok, what
