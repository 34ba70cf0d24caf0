"""The device matcher and set criterion (csrc/set_match.hip through gpv1_amd.hip_match / ops.device_set_criterion / Localization with
matcher='device') against scipy, against the host path (HungarianMatcher / SetCriterion) and against the real reference's golden
vectors -- never against itself.

Bounds, none of them taken from what the kernels give:
  * indices and pair counts: equal as integers, no case left out;
  * the fused cost against a float64 evaluation of the same formula: twice the largest error of the EXISTING fp32 torch expression
    of HungarianMatcher.forward against that float64 evaluation on the same inputs (both are fp32 evaluations of one formula), measured
    inside the test;
  * losses 1e-5, gradients 1e-5 of the largest gradient entry: the project's fp32 parity bar (the kernel sums in float64; the
    reference, SetCriterion, casts its inputs to fp32 itself, a few 1e-7 on values of order 1);
  * the train step: last_indices equal, the loss within 1e-5 of max(|loss|, 1) (tests.test_model_cpu.close's convention), the flat
    gradient within the 1e-2 of its largest entry that the eager-vs-graphed tests of tests/test_model_gpu.py use.
"""
import json
import os

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

from tests import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def draw_boxes(g, *shape):
    """cxcywh boxes as bench.py draws its detection targets"""
    return torch.cat((0.25 + 0.5 * torch.rand(*shape, 2, generator=g), 0.05 + 0.3 * torch.rand(*shape, 2, generator=g)), -1)


def check_against_scipy(cost, g_count, pred, tgt, n_pairs, status):
    """every problem of a batch: cost [P,Q,G] numpy, the kernel's outputs as numpy"""
    P, Q, _ = cost.shape
    assert status.tolist() == [0] * P
    for p in range(P):
        g = max(int(g_count[p]), 0)
        r, c = linear_sum_assignment(cost[p, :, :g])
        n = int(n_pairs[p])
        assert n == len(r) == min(Q, g), (p, n, len(r))
        assert pred[p, :n].tolist() == r.tolist() and tgt[p, :n].tolist() == c.tolist(), (p, g, pred[p], tgt[p], r, c)
        assert (pred[p, n:] == -1).all() and (tgt[p, n:] == -1).all()


def counts_for(rng, P, G):
    """mixed g_count: the full width, an empty problem (0), a sample that takes no part (-1), the rest random in 1..G"""
    c = rng.integers(1, G + 1, P)
    c[0] = G
    if P >= 4:
        c[1], c[2] = 0, -1
    return c.astype(np.int32)


# ------------------------------------------------------------------------------------------------ 1. the solver alone
@pytest.mark.parametrize('Q,G', [(1, 1), (2, 3), (3, 2), (12, 12), (64, 5), (65, 7), (100, 1), (100, 10), (100, 100), (100, 130),
                                 (128, 128), (129, 3), (256, 256)])
def test_solver_equals_scipy_on_small_integer_costs(Q, G):
    """values from {0, 1, 2} in fp32: ties everywhere, so the tie rule decides almost every pick.  P = 1, 4, 5, 70: partly filled
    workgroups (four problems each) and mixed g_count, 0 and -1 included"""
    from gpv1_amd import hip_match
    rng = np.random.default_rng(1000 * Q + G)
    for P in (1, 4, 5, 70):
        cost = rng.integers(0, 3, (P, Q, G)).astype(np.float32)
        g_count = counts_for(rng, P, G)
        out = hip_match.lsap(torch.from_numpy(cost).to(DEV), torch.from_numpy(g_count).to(DEV))
        torch.cuda.synchronize()
        pred, tgt, n_pairs, status = (t.cpu().numpy() for t in out)
        assert pred.shape == tgt.shape == (P, min(Q, G))
        check_against_scipy(cost, g_count, pred, tgt, n_pairs, status)


def test_solver_reports_invalid_and_infeasible_costs_and_goes_on():
    from gpv1_amd import hip_match
    cost = np.ones((5, 6, 4), np.float32)
    cost[1, 2, 3] = np.nan
    cost[2, 0, 0] = -np.inf
    cost[3, :, 1] = np.inf                   # 6 x 4 is solved transposed: a column of the input is a row of the problem
    cost[4, 2, :3] = np.inf                  # +inf entries with a way round them are legal
    g_count = np.full(5, 4, np.int32)
    out = hip_match.lsap(torch.from_numpy(cost).to(DEV), torch.from_numpy(g_count).to(DEV))
    torch.cuda.synchronize()
    pred, tgt, n_pairs, status = (t.cpu().numpy() for t in out)
    assert status.tolist() == [0, 1, 1, 2, 0] and n_pairs.tolist() == [4, 0, 0, 0, 4]
    assert (pred[1:4] == -1).all() and (tgt[1:4] == -1).all()
    for p in (0, 4):
        r, c = linear_sum_assignment(cost[p])
        assert pred[p].tolist() == r.tolist() and tgt[p].tolist() == c.tolist()
    with pytest.raises(RuntimeError, match='NaN or -inf'):
        hip_match.check_status(status[:2])


# ------------------------------------------------------------------------------------------------ 2. / 3. the fused cost
def box_problem(seed, L, B, Q, n_max, C1):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(L, B, Q, C1, generator=g)
    boxes = draw_boxes(g, L, B, Q)
    counts = torch.randint(1, n_max + 1, (B,), generator=g).tolist()
    counts[0] = n_max
    targets = [{'boxes': draw_boxes(g, n), 'labels': torch.randint(0, C1 - 1, (n,), generator=g)} for n in counts]
    tgt_boxes = torch.zeros(B, n_max, 4)
    tgt_labels = torch.zeros(B, n_max, dtype=torch.int32)
    for b, t in enumerate(targets):
        tgt_boxes[b, :counts[b]] = t['boxes']
        tgt_labels[b, :counts[b]] = t['labels'].to(torch.int32)
    return logits, boxes, targets, tgt_boxes, tgt_labels, torch.tensor(counts, dtype=torch.int32)


def matcher_cost(logits, boxes, tb, labels, w, dtype):
    """the expression of HungarianMatcher.forward for one image in `dtype`"""
    from gpv1_amd.criterion import box_cxcywh_to_xyxy, generalized_box_iou
    lg, bx, tb = logits.to(dtype), boxes.to(dtype), tb.to(dtype)
    return w[1] * torch.cdist(bx, tb, p=1) + w[0] * -lg.softmax(-1)[:, labels.long()] + \
        w[2] * -generalized_box_iou(box_cxcywh_to_xyxy(bx), box_cxcywh_to_xyxy(tb))


W_COST = (1.0, 5.0, 2.0)


@pytest.mark.parametrize('Q,n_max,C1', [(100, 10, 2), (100, 10, 4), (100, 20, 2), (7, 20, 4), (12, 12, 2)])
def test_fused_cost_and_its_own_assignment(Q, n_max, C1):
    """(100, 20) and up is past the LDS tile: the solver reads the cost back from the buffer"""
    from gpv1_amd import hip_match
    L, B = 2, 5
    logits, boxes, targets, tgt_boxes, tgt_labels, g_count = box_problem(17 + Q + n_max + C1, L, B, Q, n_max, C1)
    out = hip_match.match_boxes(logits.to(DEV), boxes.to(DEV), tgt_boxes.to(DEV), tgt_labels.to(DEV), g_count.to(DEV), *W_COST, cost_out=True)
    torch.cuda.synchronize()
    pred, tgt, n_pairs, status, cost = (t.cpu().numpy() for t in out)
    torch_err = kernel_err = 0.0
    for l in range(L):
        for b in range(B):
            n = int(g_count[b])
            ref = matcher_cost(logits[l, b], boxes[l, b], targets[b]['boxes'], targets[b]['labels'], W_COST, torch.float64)
            f32 = matcher_cost(logits[l, b], boxes[l, b], targets[b]['boxes'], targets[b]['labels'], W_COST, torch.float32)
            torch_err = max(torch_err, float((f32.double() - ref).abs().max()))
            kernel_err = max(kernel_err, float((torch.from_numpy(cost[l, b, :, :n]).double() - ref).abs().max()))
    print(f'COST Q={Q} G={n_max} C1={C1}: torch fp32 vs float64 {torch_err:.3e}, kernel vs float64 {kernel_err:.3e}')
    assert kernel_err <= 2 * torch_err, (kernel_err, torch_err)
    check_against_scipy(cost.reshape(L * B, Q, n_max), np.tile(g_count.numpy(), L), pred, tgt, n_pairs, status)


@pytest.mark.parametrize('Q,n_max', [(100, 10), (12, 12), (7, 20)])
@pytest.mark.parametrize('C1', [2, 4])
def test_same_decisions_as_the_host_matcher(Q, n_max, C1):
    from gpv1_amd import hip_match
    from gpv1_amd.criterion import HungarianMatcher
    L, B = 2, 6
    logits, boxes, targets, tgt_boxes, tgt_labels, g_count = box_problem(5 + Q + n_max + C1, L, B, Q, n_max, C1)
    dev_t = [{k: v.to(DEV) for k, v in t.items()} for t in targets]
    out = hip_match.match_boxes(logits.to(DEV), boxes.to(DEV), tgt_boxes.to(DEV), tgt_labels.to(DEV), g_count.to(DEV), *W_COST)
    pred, tgt, n_pairs, status = (t.cpu() for t in out[:4])
    assert status.tolist() == [0] * (L * B) and out[4] is None
    hm = HungarianMatcher(*W_COST)
    for l in range(L):
        host = hm({'pred_relevance_logits': logits[l].to(DEV), 'pred_boxes': boxes[l].to(DEV)}, dev_t)
        for b, (r, c) in enumerate(host):
            p = l * B + b
            n = int(n_pairs[p])
            assert n == len(r) and pred[p, :n].tolist() == r.tolist() and tgt[p, :n].tolist() == c.tolist(), (l, b)


# ------------------------------------------------------------------------------------------------ 4. the golden
def test_reference_golden_matching_and_losses():
    import gpv1_amd.ops as ops
    g = dict(np.load(os.path.join(GOLD, 'matcher.npz')))
    sizes = g['sizes'].tolist()
    tb = np.split(g['tgt_boxes'], np.cumsum(sizes)[:-1])
    B, Q, G = 3, 12, 12
    tgt_boxes = torch.zeros(B, G, 4)
    for b, t in enumerate(tb):
        tgt_boxes[b, :sizes[b]] = torch.from_numpy(t)
    logits, boxes = torch.from_numpy(g['logits'])[None].to(DEV), torch.from_numpy(g['boxes'])[None].to(DEV)
    ce, bbox, giou, pred, tgt, n_pairs, status = ops.device_set_criterion(
        logits, boxes, tgt_boxes.to(DEV), torch.zeros(B, G, dtype=torch.int32, device=DEV), torch.tensor(sizes, dtype=torch.int32, device=DEV),
        (1.0, 5.0, 2.0), 0.1)
    assert status.tolist() == [0, 0, 0] and n_pairs.tolist() == sizes
    assert torch.cat([pred[b, :sizes[b]] for b in range(B)]).tolist() == g['pred_idx'].tolist()
    assert torch.cat([tgt[b, :sizes[b]] for b in range(B)]).tolist() == g['tgt_idx'].tolist()
    for name, got in (('ce', ce), ('bbox', bbox), ('giou', giou)):
        assert got.shape == (1,) and got.dtype == torch.float32
        assert abs(float(got) - float(g['sc_loss_' + name])) <= 1e-5, (name, float(got), float(g['sc_loss_' + name]))


# ------------------------------------------------------------------------------------------------ 5. losses and gradients
def host_losses(logits, boxes, targets, sel, indices, C1, eos):
    """SetCriterion.loss_labels / loss_boxes for one layer, fed the given indices, float64 inputs with gradients"""
    from gpv1_amd.criterion import SetCriterion
    sc = SetCriterion(C1 - 1, None, None, eos, ['labels', 'boxes'])
    out = {'pred_relevance_logits': logits[sel], 'pred_boxes': boxes[sel]}
    tg = [targets[b] for b in sel]
    num_boxes = max(float(sum(len(t['labels']) for t in tg)), 1.0)
    r = sc.loss_labels(out, tg, indices, num_boxes)
    r.update(sc.loss_boxes(out, tg, indices, num_boxes))
    return r


@pytest.mark.parametrize('L', [1, 6])
@pytest.mark.parametrize('counts', [[3], [4, 10], [10, -1, 0, 2, 7], [0, 0]], ids=['B1', 'B2', 'B5-mixed', 'all-empty'])
def test_losses_and_gradients_equal_the_set_criterion(L, counts):
    import gpv1_amd.ops as ops
    B, Q, G, C1, eos = len(counts), 20, 10, 3, 0.1
    g = torch.Generator().manual_seed(31 * L + B)
    logits = torch.randn(L, B, Q, C1, generator=g)
    boxes = draw_boxes(g, L, B, Q)
    targets = [{'boxes': draw_boxes(g, max(n, 0)), 'labels': torch.randint(0, C1 - 1, (max(n, 0),), generator=g)} for n in counts]
    sel = [b for b, n in enumerate(counts) if n >= 0]
    tgt_boxes, tgt_labels = torch.zeros(B, G, 4), torch.zeros(B, G, dtype=torch.int32)
    for b in sel:
        tgt_boxes[b, :counts[b]] = targets[b]['boxes']
        tgt_labels[b, :counts[b]] = targets[b]['labels'].to(torch.int32)
    lg, bx = logits.to(DEV).requires_grad_(True), boxes.to(DEV).requires_grad_(True)
    ce, bbox, giou, pred, tgt, n_pairs, status = ops.device_set_criterion(
        lg, bx, tgt_boxes.to(DEV), tgt_labels.to(DEV), torch.tensor(counts, dtype=torch.int32, device=DEV), W_COST, eos)
    wl = torch.linspace(1.0, 2.0, L)                       # different upstream gradients per layer and per loss
    (ce * wl.to(DEV)).sum().add((bbox * (5 * wl).to(DEV)).sum()).add((giou * (2 * wl).to(DEV)).sum()).backward()
    assert status.tolist() == [0] * (L * B)
    assert n_pairs.view(L, B).tolist() == [[max(n, 0) for n in counts]] * L
    pred, tgt = pred.cpu().long(), tgt.cpu().long()
    rl, rb = logits.double().requires_grad_(True), boxes.double().requires_grad_(True)
    total = 0
    for l in range(L):
        ind = [(pred[l * B + b, :counts[b]], tgt[l * B + b, :counts[b]]) for b in sel]
        ref = host_losses(rl[l], rb[l], targets, sel, ind, C1, eos)
        for name, got, wt in (('loss_ce', ce, 1.0), ('loss_bbox', bbox, 5.0), ('loss_giou', giou, 2.0)):
            assert abs(float(got[l].detach()) - float(ref[name].detach())) <= 1e-5, (l, name, float(got[l].detach()), float(ref[name].detach()))
            total = total + wt * wl[l] * ref[name]
    total.backward()
    for name, got, ref in (('dlogits', lg.grad, rl.grad), ('dboxes', bx.grad, rb.grad)):
        ref = torch.zeros(got.shape, dtype=torch.float64) if ref is None else ref       # no matched pair: no path to the boxes
        err, top = float((got.cpu().double() - ref).abs().max()), float(ref.abs().max())
        assert err <= 1e-5 * top or (top == 0.0 and err == 0.0), (name, err, top)
    if -1 in counts:                                      # the sample that takes no part gets no gradient at all
        b = counts.index(-1)
        assert not lg.grad[:, b].any() and not bx.grad[:, b].any()


def test_a_failed_problem_makes_its_loss_nan_and_is_reported():
    """a degenerate predicted box (negative width): the host path asserts on it; here the status word says so and the loss is NaN"""
    import gpv1_amd.ops as ops
    from gpv1_amd import hip_match
    g = torch.Generator().manual_seed(2)
    logits, boxes = torch.randn(1, 2, 8, 2, generator=g), draw_boxes(g, 1, 2, 8)
    boxes[0, 1, 3, 2] = -0.1
    ce, bbox, giou, _, _, _, status = ops.device_set_criterion(
        logits.to(DEV), boxes.to(DEV), draw_boxes(g, 2, 3).to(DEV), torch.zeros(2, 3, dtype=torch.int32, device=DEV),
        torch.tensor([3, 2], dtype=torch.int32, device=DEV), W_COST, 0.1)
    assert status[0] == 0 and status[1] & 4 and torch.isnan(ce).all() and torch.isnan(bbox).all() and torch.isnan(giou).all()
    with pytest.raises(RuntimeError, match='degenerate'):
        hip_match.check_status(status.tolist())


# ------------------------------------------------------------------------------------------------ 6. determinism and capture
def criterion_batch(seed, L=3, B=4, Q=20, G=6, C1=2):
    g = torch.Generator().manual_seed(seed)
    counts = torch.randint(0, G + 1, (B,), generator=g).to(torch.int32)
    return (torch.randn(L, B, Q, C1, generator=g).to(DEV), draw_boxes(g, L, B, Q).to(DEV), draw_boxes(g, B, G).to(DEV),
            torch.zeros(B, G, dtype=torch.int32, device=DEV), counts.to(DEV))


def run_criterion(logits, boxes, tgt_boxes, tgt_labels, g_count):
    import gpv1_amd.ops as ops
    logits.grad = boxes.grad = None
    out = ops.device_set_criterion(logits, boxes, tgt_boxes, tgt_labels, g_count, W_COST, 0.1)
    (out[0].sum() + 5 * out[1].sum() + 2 * out[2].sum()).backward()
    return out


def bits(out, logits, boxes):
    return [t.detach().cpu().numpy().tobytes() for t in tuple(out) + (logits.grad, boxes.grad)]


def test_two_calls_give_the_same_bits_and_a_captured_graph_equals_the_eager_call():
    first, second = criterion_batch(1), criterion_batch(2)
    lg, bx = first[0].clone().requires_grad_(True), first[1].clone().requires_grad_(True)
    a = bits(run_criterion(lg, bx, *first[2:]), lg, bx)
    b = bits(run_criterion(lg, bx, *first[2:]), lg, bx)
    assert a == b
    # capture forward + backward on one stream, over static buffers
    static = [t.clone() for t in first]
    s_lg, s_bx = static[0].requires_grad_(True), static[1].requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run_criterion(s_lg, s_bx, *static[2:])
    torch.cuda.current_stream().wait_stream(side)
    s_lg.grad = s_bx.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        s_out = run_criterion(s_lg, s_bx, *static[2:])
    graph.replay()
    assert bits(s_out, s_lg, s_bx) == a
    with torch.no_grad():                                   # a second batch through the static buffers: targets, counts and predictions
        for dst, src in zip(static, second):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    e_lg, e_bx = second[0].clone().requires_grad_(True), second[1].clone().requires_grad_(True)
    eager = bits(run_criterion(e_lg, e_bx, *second[2:]), e_lg, e_bx)
    assert bits(s_out, s_lg, s_bx) == eager
    assert eager != a


# ------------------------------------------------------------------------------------------------ 7. end to end
def small_model(matcher, aux_loss):
    from gpv1_amd.gpv import GPV
    from tests.test_model_cpu import V
    man = json.load(open(os.path.join(GOLD, 'small_manifest.json')))
    cfg = synth.small_cfg(dropout=0.0)
    cfg['detr']['aux_loss'] = aux_loss
    cfg['losses']['Localization']['matcher'] = matcher
    cfg['vocab'] = synth.make_vocab(V)
    cfg['vocab_embed'] = synth.synth_tensor('answer_head.vocab_embed', (V, 768))
    cfg['bert_layers'] = 2
    model = GPV(cfg)
    model.load_state_dict(synth.synth_state(man['manifest']), strict=False)
    model.to(DEV).train()
    model.bert.model.p = 0.0
    return model


def test_localization_with_aux_outputs_equals_the_host_path(monkeypatch):
    """Localization on outputs with two aux layers and a mixed batch (boxes, no boxes, no 'boxes' key at all): the device path
    against the host path on the same tensors -- indices equal, the three sums within 1e-5 of max(|sum|, 1), gradients within 1e-5 of
    the largest entry (the host path is fp32 torch, the kernel float64 inside: a few 1e-7 apart)"""
    from gpv1_amd.criterion import Localization
    from gpv1_amd.misc import AttrDict
    monkeypatch.delenv('GPV_MATCHER', raising=False)
    cfg = synth.model_cfg()['losses']['Localization']
    B, Q, g = 5, 30, torch.Generator().manual_seed(11)
    counts = [3, None, 0, 7, 1]
    targets = [{'task': 'CocoCaptioning', 'answer': 'w1'} if n is None else
               {'task': 'CocoDetection', 'boxes': draw_boxes(g, n).to(DEV), 'labels': torch.zeros(n, dtype=torch.long, device=DEV)} for n in counts]
    base = [(torch.randn(B, Q, 2, generator=g), draw_boxes(g, B, Q)) for _ in range(3)]
    res = {}
    for matcher in ('host', 'device'):
        loc = Localization(AttrDict({k: (AttrDict(v) if isinstance(v, dict) else v) for k, v in dict(cfg, matcher=matcher).items()})).to(DEV)
        layers = [{'pred_relevance_logits': a.to(DEV).requires_grad_(True), 'pred_boxes': b.to(DEV).requires_grad_(True)} for a, b in base]
        outputs = dict(layers[-1], aux_outputs=layers[:-1])
        r = loc(outputs, targets)
        (r['loss_ce'] + 5 * r['loss_bbox'] + 2 * r['loss_giou']).backward()
        ind = [(a.tolist(), b.tolist()) for a, b in loc.set_criterion.last_indices]
        res[matcher] = ({k: float(v.detach()) for k, v in r.items()}, [t.grad.cpu() for l in layers for t in l.values()], ind)
    (l0, g0, i0), (l1, g1, i1) = res['host'], res['device']
    assert i0 == i1 and [len(a) for a, _ in i1] == [3, 0, 7, 1]
    for k in l0:
        assert abs(l0[k] - l1[k]) <= 1e-5 * max(abs(l0[k]), 1.0), (k, l0[k], l1[k])
    top = max(float(t.abs().max()) for t in g0)
    assert max(float((a - b).abs().max()) for a, b in zip(g0, g1)) <= 1e-5 * top
    assert not any(t[1].any() for t in g1)                 # the caption sample: no gradient


@pytest.mark.parametrize('aux_loss', [False, True])
@pytest.mark.parametrize('graphs', [False, True])
def test_train_step_with_the_device_matcher_equals_the_host_path(graphs, aux_loss, monkeypatch):
    """a mixed batch (two detection samples, one of them with two boxes, a detection sample with no boxes, a caption sample), three
    steps at learning rate 0 (with graphs on: the eager step, the capture, a replay), the last one compared"""
    import gpv1_amd.ops as ops
    from gpv1_amd.train import FlatTrainer
    from tests.test_model_cpu import nested, B, H, W, Tl, PAD, V
    monkeypatch.delenv('GPV_MATCHER', raising=False)
    ops.RT.set_precise(False)
    images, mask, ids, attn = (t.to(DEV) for t in synth.synth_batch(B, H, W, Tl, V, pad_to=PAD))
    det = lambda rows: {'task': 'CocoDetection', 'boxes': torch.tensor(rows, device=DEV).view(-1, 4),
                        'labels': torch.zeros(len(rows), dtype=torch.long, device=DEV)}
    targets = [det([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.1]]), det([]), {'task': 'CocoCaptioning', 'answer': 'w1 w2 w3 w4'},
               det([[0.4, 0.45, 0.3, 0.2]])]
    layers_seen = []
    real = ops.device_set_criterion
    monkeypatch.setattr(ops, 'device_set_criterion', lambda logits, *a: (layers_seen.append(logits.shape[0]), real(logits, *a))[1])
    res = {}
    for matcher in ('host', 'device'):
        model = small_model(matcher, aux_loss)
        loc = model.criterion.localization_criterion
        assert loc.matcher_mode == matcher
        tr = FlatTrainer(model, lr=0.0, lr_backbone=0.0, graphs=graphs)
        for _ in range(3):
            loss = tr.train_step(nested(images, mask), (ids, attn), [dict(t) for t in targets])
        ind = [(a.tolist(), b.tolist()) for a, b in loc.set_criterion.last_indices]
        assert all(a.dtype == torch.int64 and not a.is_cuda for pair in loc.set_criterion.last_indices for a in pair)
        res[matcher] = (float(loss), tr.G.detach().clone().cpu(), ind, len(tr._bodies))
        del tr, model
    (l0, g0, i0, n0), (l1, g1, i1, n1) = res['host'], res['device']
    print(f'TRAIN STEP graphs={graphs} aux={aux_loss}: host loss {l0!r} device loss {l1!r} '
          f'grad diff {float((g0 - g1).abs().max()):.3e} of {float(g0.abs().max()):.3e}')
    assert n0 == n1 == (1 if graphs else 0)
    # one call per step.  (With the RoI head the decoder hands out its last layer only, as in the reference, so aux_loss adds no layer
    # here; Localization with real aux outputs: test_localization_with_aux_outputs_equals_the_host_path)
    assert layers_seen == [1] * 3
    assert i0 == i1 and [len(a) for a, _ in i1] == [2, 0, 1]
    assert abs(l0 - l1) <= 1e-5 * max(abs(l0), 1.0), (l0, l1)
    assert float((g0 - g1).abs().max()) <= 1e-2 * float(g0.abs().max())
