"""The matching rule on the host (gpv1_amd.criterion.lsap_host / match_cost_host), which csrc/set_match.hip restates on the device:
against scipy on matrices full of ties, against the real reference's golden matching, and the configuration / error behaviour of the
device option that needs no GPU.  (The kernels need the GPU: tests/test_match_gpu.py.)"""
import os
import re
import subprocess

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')


def tie_matrices(n, seed, lo=1, hi=14):
    """n matrices of lo..hi x lo..hi in the four value kinds: {0,1}, {0,1,2}, fp32 uniforms, integers with one duplicated row and one
    duplicated column"""
    rng = np.random.default_rng(seed)
    for it in range(n):
        nr, nc = (int(v) for v in rng.integers(lo, hi + 1, 2))
        kind = it % 4
        if kind == 0:
            c = rng.integers(0, 2, (nr, nc)).astype(np.float32)
        elif kind == 1:
            c = rng.integers(0, 3, (nr, nc)).astype(np.float32)
        elif kind == 2:
            c = rng.random((nr, nc), dtype=np.float32)
        else:
            c = rng.integers(0, 5, (nr, nc)).astype(np.float32)
            c[rng.integers(nr)] = c[rng.integers(nr)]
            c[:, rng.integers(nc)] = c[:, rng.integers(nc)]
        yield c


def test_lsap_host_equals_scipy_on_ties_in_both_orientations():
    from gpv1_amd.criterion import lsap_host
    n = 0
    for c in tie_matrices(2400, seed=7):
        for m in (c, c.T):
            r, k = lsap_host(m)
            sr, sk = linear_sum_assignment(m)
            assert r.dtype == k.dtype == np.int64
            assert np.array_equal(r, sr) and np.array_equal(k, sk), (m, r, k, sr, sk)
            n += 1
    assert n == 4800


def test_lsap_host_refuses_what_scipy_refuses():
    from gpv1_amd.criterion import lsap_host
    c = np.ones((3, 4))
    for bad in (np.nan, -np.inf):
        m = c.copy()
        m[1, 2] = bad
        with pytest.raises(ValueError):
            linear_sum_assignment(m)
        with pytest.raises(ValueError, match='invalid numeric'):
            lsap_host(m)
    m = c.copy()
    m[1, :] = np.inf                                      # +inf is a legal entry; a row of them is infeasible
    with pytest.raises(ValueError):
        linear_sum_assignment(m)
    with pytest.raises(ValueError, match='infeasible'):
        lsap_host(m)
    m = c.copy()
    m[1, :3] = np.inf
    assert [a.tolist() for a in lsap_host(m)] == [a.tolist() for a in linear_sum_assignment(m)]
    assert [a.tolist() for a in lsap_host(np.zeros((0, 3)))] == [[], []]


def golden_matcher():
    g = dict(np.load(os.path.join(GOLD, 'matcher.npz')))
    sizes = g['sizes'].tolist()
    assert sizes == [4, 1, 12]
    return g, sizes, np.split(g['tgt_boxes'], np.cumsum(sizes)[:-1])


def test_host_rule_reproduces_the_reference_matching():
    """the real reference's assignment on tests/golden/matcher.npz (ties from a duplicated query row in sample 1 and a duplicated
    target in sample 2): cost by match_cost_host, solved by lsap_host, exact"""
    from gpv1_amd.criterion import lsap_host, match_cost_host
    g, sizes, tgt = golden_matcher()
    pred, tg = [], []
    for i, n in enumerate(sizes):
        cost = match_cost_host(g['logits'][i], g['boxes'][i], tgt[i], np.zeros(n, np.int64), 1.0, 5.0, 2.0)      # the weights the golden was made with
        assert cost.dtype == np.float32 and cost.shape == (12, n)
        r, k = lsap_host(cost)
        pred.append(r)
        tg.append(k)
    assert np.array_equal(np.concatenate(pred), g['pred_idx'])
    assert np.array_equal(np.concatenate(tg), g['tgt_idx'])


def test_match_cost_host_is_the_matcher_formula():
    """against HungarianMatcher.forward's torch expression in float64: both are evaluations of one formula, fp32 apart"""
    from gpv1_amd.criterion import box_cxcywh_to_xyxy, generalized_box_iou, match_cost_host
    g = torch.Generator().manual_seed(3)
    worst = 0.0
    for C1 in (2, 4):
        logits = torch.randn(100, C1, generator=g)
        boxes = torch.cat((0.25 + 0.5 * torch.rand(100, 2, generator=g), 0.05 + 0.3 * torch.rand(100, 2, generator=g)), 1)
        tb = torch.cat((0.25 + 0.5 * torch.rand(10, 2, generator=g), 0.05 + 0.3 * torch.rand(10, 2, generator=g)), 1)
        labels = torch.randint(0, C1 - 1, (10,), generator=g)
        got = match_cost_host(logits.numpy(), boxes.numpy(), tb.numpy(), labels.numpy(), 1.0, 5.0, 2.0)
        b64, t64 = boxes.double(), tb.double()
        ref = 5.0 * torch.cdist(b64, t64, p=1) - logits.double().softmax(-1)[:, labels] - \
            2.0 * generalized_box_iou(box_cxcywh_to_xyxy(b64), box_cxcywh_to_xyxy(t64))
        worst = max(worst, float((torch.from_numpy(got).double() - ref).abs().max()))
    # |cost| < 5 * 4 + 1 + 2; a dozen fp32 roundings of terms below 8 each: 12 * 8 * 2^-24 = 5.7e-6
    assert worst <= 5.7e-6, worst


def _loc_cfg(**over):
    from gpv1_amd.misc import AttrDict
    c = synth.model_cfg()['losses']['Localization']
    c.update(over)
    return AttrDict({k: (AttrDict(v) if isinstance(v, dict) else v) for k, v in c.items()})


def test_matcher_option_values_and_no_cpu_fallback(monkeypatch):
    from gpv1_amd.criterion import Localization
    monkeypatch.delenv('GPV_MATCHER', raising=False)
    assert Localization(_loc_cfg()).matcher_mode == 'host'
    assert Localization(_loc_cfg(matcher='device')).matcher_mode == 'device'
    with pytest.raises(ValueError, match="'host' or 'device'"):
        Localization(_loc_cfg(matcher='gpu'))
    monkeypatch.setenv('GPV_MATCHER', 'device')                       # the environment overrides the key
    assert Localization(_loc_cfg(matcher='host')).matcher_mode == 'device'
    monkeypatch.setenv('GPV_MATCHER', 'somewhere')
    with pytest.raises(ValueError, match="'host' or 'device'"):
        Localization(_loc_cfg())
    monkeypatch.delenv('GPV_MATCHER')
    g = torch.Generator().manual_seed(0)
    outputs = {'pred_relevance_logits': torch.randn(2, 10, 2, generator=g), 'pred_boxes': torch.rand(2, 10, 4, generator=g)}
    targets = [{'boxes': torch.tensor([[0.5, 0.5, 0.2, 0.2]]), 'labels': torch.zeros(1, dtype=torch.long)}, {'answer': 'w1'}]
    host = Localization(_loc_cfg())(outputs, targets)
    assert all(torch.isfinite(v) for v in host.values())
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        Localization(_loc_cfg(matcher='device'))(outputs, targets)
    # no sample with boxes: nothing to match on either path
    assert Localization(_loc_cfg(matcher='device'))(outputs, [{'answer': 'w1'}] * 2) == {'loss_ce': None, 'loss_bbox': None, 'loss_giou': None}


def test_mirror_refuses_cpu_tensors_and_shapes_outside_the_limits():
    from gpv1_amd import hip_match
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip_match.lsap(torch.zeros(1, 3, 3), torch.zeros(1, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        hip_match.match_boxes(torch.zeros(1, 1, 3, 2), torch.zeros(1, 1, 3, 4), torch.zeros(1, 2, 4), torch.zeros(1, 2, dtype=torch.int32),
                              torch.zeros(1, dtype=torch.int32), 1, 1, 1)
    assert hip_match.supported(256, 256) and not hip_match.supported(257, 3) and not hip_match.supported(3, 257)
    with pytest.raises(RuntimeError, match='infeasible'):
        hip_match.check_status([0, 2])
    hip_match.check_status([0, 0])


def test_match_library_exports_exactly_the_declared_entry_points():
    """exports, header and nm: tests/test_abi_cpu.py, for every library; here what is the matching library's own"""
    import gpv1_amd.hip_match as hip_match
    from tests import abi_probe
    header, src = abi_probe.header_path('match'), abi_probe.source('match')
    # plain C: the header compiles as C99 on its own, and the mirror's limits are the header's
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', header], check=True)
    limits = dict(re.findall(r'#define\s+(GPV_MATCH_\w+)\s+(\d+)', src))
    assert (int(limits['GPV_MATCH_MAX_DIM']), int(limits['GPV_MATCH_TILE']), int(limits['GPV_MATCH_MAX_CLASSES'])) == \
        (hip_match.MAX_DIM, hip_match.TILE, hip_match.MAX_CLASSES)
    assert hip_match.MAX_DIM >= 256
    assert {int(limits[k]) for k in limits if k.startswith('GPV_MATCH_ERR_')} == set(hip_match.ERR_BITS)
