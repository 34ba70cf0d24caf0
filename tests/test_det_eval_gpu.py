"""The device scorer of train-time evaluation (csrc/det_ap.hip through gpv1_amd.hip_eval) against the host rule
(gpv1_amd.evaluators.det_ap_host), det_metrics end to end on the small model, and an evaluation between graphed training steps.

Bounds, none of them taken from what the kernel gives:
  * score: 1e-6 of a float64 softmax -- a few float32 roundings (subtract, exp, add, divide) of values below 1, 6e-8 each;
  * order: exactly the stable descending sort of the kernel's own scores;
  * decisions: the host rule fed the kernel's scores gives the same order and the same true-positive flags, no case left out -- the
    float32 IoU is the same sequence of correctly rounded operations on both sides (the file is compiled without contraction);
  * AP: 1e-12 -- both sides are float64 from the same integers, at most Q + 2 additions of terms <= 1 (2e-16 each)."""
import os

import numpy as np
import pytest
import torch

from tests import synth
from tests.test_model_cpu import build_small, nested, V, B, H, W, Tl, PAD

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture()
def rt():
    import gpv1_amd.ops as ops
    import gpv1_amd.hip as hip
    import gpv1_amd.hip_eval as hip_eval
    hip.lib()
    hip_eval.lib()                              # fail loudly if the library is missing
    yield ops.RT
    ops.RT.set_precise(False)


def make_case(Bn, Q, G, seed):
    """logits with repeated rows and values, boxes near / on / far from the ground truth, zero-area boxes, boxes outside 0..1,
    ragged gt_count including 0"""
    rs = np.random.RandomState(seed)
    logits = rs.randn(Bn, Q, 2).astype(np.float32) * 2
    coarse = rs.rand(Bn, Q) < 0.4
    logits[coarse] = np.round(logits[coarse])                       # few distinct values: equal scores across queries
    if Q > 3:
        logits[:, 3] = logits[:, 0]                                 # repeated rows
        logits[:, Q - 1] = logits[:, 1]
    gt = np.concatenate([rs.uniform(-0.05, 0.7, (Bn, G, 2)), rs.uniform(0.05, 0.4, (Bn, G, 2))], -1).astype(np.float32)
    count = rs.randint(0, G + 1, size=Bn).astype(np.int32)
    count[0] = G
    if Bn > 1:
        count[1] = 0
    if Bn > 2:
        gt[2, 1:] = gt[2, :1]                                       # identical ground-truth boxes: the first maximum wins
    boxes = np.concatenate([rs.uniform(-0.2, 1.2, (Bn, Q, 2)), rs.uniform(0.02, 0.5, (Bn, Q, 2))], -1).astype(np.float32)
    for b in range(Bn):
        for q in range(Q):
            kind = rs.randint(0, 6)
            g = gt[b, rs.randint(0, G)]
            if kind == 0:                                           # the ground-truth box itself
                boxes[b, q] = [g[0] + np.float32(0.5) * g[2], g[1] + np.float32(0.5) * g[3], g[2], g[3]]
            elif kind in (1, 2):                                    # jittered around it: IoUs on both sides of the threshold
                j = rs.uniform(-0.25, 0.25, 4).astype(np.float32)
                boxes[b, q] = [g[0] + 0.5 * g[2] + j[0] * g[2], g[1] + 0.5 * g[3] + j[1] * g[3], g[2] * (1 + j[2]), g[3] * (1 + j[3])]
            elif kind == 3 and q % 2:
                boxes[b, q, 2] = 0.0                                # zero area
    return logits, boxes, gt, count


def run_kernel(logits, boxes, gt, count, thresh=0.5):
    from gpv1_amd import hip_eval
    out = hip_eval.det_ap(torch.from_numpy(logits).to(DEV), torch.from_numpy(boxes).to(DEV), torch.from_numpy(gt).to(DEV),
                          torch.from_numpy(count).to(DEV), thresh)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


def check_against_host(logits, boxes, gt, count, score, order, tp, ap, thresh=0.5):
    from gpv1_amd.evaluators import det_ap_host
    Bn, Q, _ = logits.shape
    l64 = logits.astype(np.float64)
    soft = 1.0 / (1.0 + np.exp(l64[..., 1] - l64[..., 0]))
    worst_s = worst_ap = 0.0
    for b in range(Bn):
        assert sorted(order[b].tolist()) == list(range(Q)), (b, 'order is not a permutation')
        worst_s = max(worst_s, float(np.abs(score[b] - soft[b][order[b]]).max()))
        # a stable descending sort of the kernel's own scores
        s, o = score[b], order[b]
        assert np.all((s[:-1] > s[1:]) | ((s[:-1] == s[1:]) & (o[:-1] < o[1:]))), (b, 'not a stable descending sort')
        own = np.empty(Q, dtype=np.float32)
        own[o] = s                                                   # the kernel's scores in query order
        h_ap, h_order, h_tp = det_ap_host(own, boxes[b], gt[b, :count[b]], thresh)
        assert np.array_equal(h_order, o), (b, 'order')
        assert np.array_equal(h_tp, tp[b]), (b, 'tp', np.nonzero(h_tp != tp[b])[0])
        worst_ap = max(worst_ap, abs(h_ap - ap[b]))
        if count[b] == 0:
            assert ap[b] == 0.0 and not tp[b].any()
    print('worst |score - softmax64| %.3e   worst |ap - host| %.3e   mean ap %.4f   true positives %d' %
          (worst_s, worst_ap, float(ap.mean()), int(tp.sum())))
    assert worst_s <= 1e-6, worst_s
    assert worst_ap <= 1e-12, worst_ap


@pytest.mark.parametrize('G', [1, 2, 17, 100])
@pytest.mark.parametrize('Q', [1, 7, 100, 300])
@pytest.mark.parametrize('Bn', [1, 3, 64])
def test_kernel_equals_the_host_rule(rt, Bn, Q, G):
    case = make_case(Bn, Q, G, seed=1000 * Bn + 10 * Q + G)
    check_against_host(*case, *run_kernel(*case))


def test_kernel_limits_thresholds_and_refused_shapes(rt):
    from gpv1_amd import hip_eval
    # the largest Q, more ground-truth boxes than lanes, other thresholds
    case = make_case(2, 1024, 200, seed=7)
    for thresh in (0.5, 0.75, 0.05):
        check_against_host(*case, *run_kernel(*case, thresh=thresh), thresh=thresh)
    # G = 0: every sample scores 0
    logits, boxes, _, _ = make_case(3, 9, 1, seed=8)
    score, order, tp, ap = run_kernel(logits, boxes, np.zeros((3, 0, 4), np.float32), np.zeros(3, np.int32))
    assert not ap.any() and not tp.any() and np.all(np.diff(score, axis=1) <= 0)
    # refused before anything is launched: Q out of range, wrong dtypes / shapes, views that are not contiguous
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    with pytest.raises(RuntimeError, match='hipError 1'):                     # hipErrorInvalidValue
        hip_eval.det_ap(z(1, 1025, 2), z(1, 1025, 4), z(1, 1, 4), z(1, dt=torch.int32))
    with pytest.raises(RuntimeError, match='hipError 1'):
        hip_eval.det_ap(z(1, 0, 2), z(1, 0, 4), z(1, 1, 4), z(1, dt=torch.int32))
    with pytest.raises(ValueError):
        hip_eval.det_ap(z(2, 5, 2), z(2, 5, 4), z(2, 3, 4), z(2, dt=torch.int64))
    with pytest.raises(ValueError):
        hip_eval.det_ap(z(2, 5, 2), z(2, 6, 4), z(2, 3, 4), z(2, dt=torch.int32))
    with pytest.raises(ValueError):
        hip_eval.det_ap(z(2, 5, 2), z(2, 5, 8)[..., :4], z(2, 3, 4), z(2, dt=torch.int32))
    torch.cuda.synchronize()


class Replay:
    """the model's outputs of a first pass, handed out again in a second: the two scoring paths are compared on the SAME forward
    results (two forwards of one batch need not agree to 1e-12)"""

    def __init__(self, model):
        self.model, self.outs, self.at = model, [], None

    def __getattr__(self, name):
        return getattr(self.model, name)

    def eval(self):
        self.model.eval()
        return self

    def rewind(self):
        self.at = 0

    def __call__(self, images, queries, answer_token_ids, vocab_mask=None):
        if self.at is None:
            self.outs.append(self.model(images, queries, answer_token_ids, vocab_mask=vocab_mask))
            return self.outs[-1]
        self.at += 1
        return self.outs[self.at - 1]


def eval_set(n, size=(H, W)):
    from gpv1_amd.train_distr import SyntheticCocoDataset

    class Set:
        items = SyntheticCocoDataset(n, synth.make_vocab(V), image_size=size, query_len=Tl, seed=5, tasks=('CocoDetection',))
        samples = []

        def __len__(self):
            return n

        def __getitem__(self, i):
            return self.items[i]
    ds = Set()
    for i in range(n):
        b = ds.items[i][2]['boxes'].numpy().astype(np.float64)
        xywh = np.stack([(b[:, 0] - b[:, 2] / 2) * size[1], (b[:, 1] - b[:, 3] / 2) * size[0], b[:, 2] * size[1], b[:, 3] * size[0]], 1)
        ds.samples.append({'id': 700 + i, 'sent_id': 900 + i, 'boxes': xywh.tolist() if i != 2 else [], 'category_name': 'dog',
                           'image': {'W': size[1], 'H': size[0], 'image_id': i}, 'coco_categories': {'seen': ['dog'], 'unseen': []}})
    return ds


def load_boxes(path_h5py):
    path = path_h5py if os.path.exists(path_h5py) else os.path.splitext(path_h5py)[0] + '.npz'
    if path.endswith('.npz'):
        z = np.load(path)
        return {k.split('/')[0]: {'boxes': z[k.split('/')[0] + '/boxes'], 'relevance': z[k.split('/')[0] + '/relevance']} for k in z.files}
    import h5py
    with h5py.File(path, 'r') as f:
        return {k: {'boxes': f[k]['boxes'][()], 'relevance': f[k]['relevance'][()]} for k in f}


@pytest.mark.parametrize('precise', [True, False])
def test_det_metrics_device_path_equals_host_path(rt, precise, tmp_path):
    from gpv1_amd import metrics, compute_predictions as cp
    from gpv1_amd import train_distr as td
    rt.set_precise(precise)
    model, _ = build_small()
    model.to(DEV).eval()
    ds = eval_set(7)
    rp = Replay(model)
    batches = lambda: td.eval_batches(ds, 3, DEV)                  # 3 + 3 + 1: a short last batch
    with torch.no_grad():
        for im, q, _ in batches():                                 # the one real forward pass; every scoring path below replays it
            rp(im, q, None)
    assert len(rp.outs) == 3
    # ground truth cut from the predictions themselves (a random model finds no synthetic box: every AP would be 0 on both paths):
    # two predicted boxes, the second widened by a fifth, and one box nothing predicts; sample 2 keeps no box at all
    pred = torch.cat([o['pred_boxes'].float() for o in rp.outs]).cpu().numpy().astype(np.float64)
    for i, s in enumerate(ds.samples):
        if i == 2:
            continue
        picks = pred[i, [1, pred.shape[1] // 2]] * [1, 1, 1, 1.2]
        xywh = np.stack([(picks[:, 0] - picks[:, 2] / 2) * W, (picks[:, 1] - picks[:, 3] / 2) * H, picks[:, 2] * W, picks[:, 3] * H], 1)
        s['boxes'] = xywh.tolist() + [[0.0, 0.0, 2.0, 2.0]]
    dpath = str(tmp_path / 'dev' / 'det_val_boxes.h5py')
    os.makedirs(os.path.dirname(dpath))
    rp.rewind()
    m_dev = metrics.det_metrics(rp, batches(), ds.samples, None, boxes_path=dpath)
    rp.rewind()
    m_host = metrics.det_metrics(rp, batches(), ds.samples, None, host='kernel_scores')
    rp.rewind()
    m_torch = metrics.det_metrics(rp, batches(), ds.samples, None, host=True)
    print('mAP device %.17g   host rule on the kernel scores %.17g   host rule on torch softmax %.17g' % (m_dev, m_host, m_torch))
    assert 0.0 < m_dev < 1.0 and abs(m_dev - m_host) <= 1e-12
    # limit: the first 4 samples only (a cut inside the second batch), refexp keyed by sent_id scores the same
    rp.rewind()
    m4 = metrics.det_metrics(rp, batches(), ds.samples, 4)
    rp.rewind()
    h4 = metrics.refexp_metrics(rp, batches(), ds.samples, 4, host='kernel_scores')
    assert rp.at == 2 and abs(m4 - h4) <= 1e-12
    # the boxes file: what make_predictions writes for the same outputs, up to the score tolerance
    rp.rewind()
    ids = [[str(s['id']) for s in ds.samples[i:i + 3]] for i in range(0, 7, 3)]
    _, _, ppath = cp.make_predictions(rp, ((im, q, ids[k]) for k, (im, q, _) in enumerate(batches())), str(tmp_path / 'pred'), 'CocoDetection')
    ours, theirs = load_boxes(dpath), load_boxes(ppath)
    assert sorted(ours) == sorted(theirs) == sorted(str(s['id']) for s in ds.samples)
    for k in ours:
        a, b = ours[k], theirs[k]
        assert a['boxes'].dtype == b['boxes'].dtype == np.float32 and a['boxes'].shape == b['boxes'].shape and a['relevance'].shape == b['relevance'].shape
        assert np.abs(a['relevance'] - b['relevance']).max() <= 1e-6
        for r in np.nonzero((a['boxes'] != b['boxes']).any(1))[0]:      # rows may swap only where the scores tie within the tolerance
            near = [abs(float(a['relevance'][r]) - float(a['relevance'][j])) for j in (r - 1, r + 1) if 0 <= j < len(a['relevance'])]
            assert min(near) <= 1e-6, (k, r)


def test_evaluation_between_graphed_training_steps_leaves_training_alone(rt):
    """three steps, one evaluation, three more steps on a graphed FlatTrainer: the dropout seed-epoch word, torch's CPU and device
    RNG states, the optimizer's per-parameter step counts and every parameter are torch.equal before and after the evaluation, and
    the steps after it replay the graphs captured before it.  (Weights are not compared across runs: tests/test_model_gpu.py,
    test_coattention_language_branch_changes_nothing, documents why graphed training runs are not bitwise repeatable.)"""
    from gpv1_amd.train import FlatTrainer
    from gpv1_amd import train_distr as td
    from gpv1_amd.config import from_dict
    import gpv1_amd.ops as ops
    rt.set_precise(False)
    model, _ = build_small(dropout=0.1)
    model.to(DEV).train()
    tr = FlatTrainer(model, lr=1e-3, lr_backbone=1e-4, graphs=True)
    images, mask, ids, attn = (t.to(DEV) for t in synth.synth_batch(B, H, W, Tl, V, pad_to=PAD))
    det = [{'task': 'CocoDetection', 'boxes': torch.tensor([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.1]], device=DEV)[: 1 + i % 2],
            'labels': torch.zeros(1 + i % 2, dtype=torch.long, device=DEV)} for i in range(B)]
    step = lambda: float(tr.train_step(nested(images, mask), (ids, attn), [dict(t) for t in det]))
    losses = [step() for _ in range(3)]
    torch.cuda.synchronize()
    assert tr.capture_count >= 2 and tr.graph_steps >= 1, (tr.capture_count, tr.graph_steps)      # a forward body and a backward variant
    captures, graph_steps = tr.capture_count, tr.graph_steps

    def state():
        torch.cuda.synchronize()
        return {'seed_epoch': ops.RT.seed_dev.clone(), 'cpu_rng': torch.get_rng_state(), 'cuda_rng': torch.cuda.get_rng_state(),
                'pstep': tr.pstep.clone(), 'P': tr.P.clone(), 'M': tr.M.clone(), 'V': tr.V.clone(),
                'params': [p.detach().clone() for p in model.parameters()], 'buffers': [b.detach().clone() for b in model.buffers()],
                'step_count': tr.step_count, 'host_ctr': ops.RT._ctr}
    before = state()
    cfg = from_dict({'batch_size': 3, 'training': {'batch_size': 3, 'num_val_samples': {'coco_det': 5}}})
    logs = []
    metric = td.evaluate_subset(model, {'coco_det': eval_set(7)}, 'val', cfg, 0, DEV, logs.append)
    after = state()
    assert model.training and 0.0 <= metric <= 1.0 and any('mAP' in l for l in logs), logs
    for k in before:
        a, b = before[k], after[k]
        if isinstance(a, list):
            assert len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b)), k
        elif torch.is_tensor(a):
            assert torch.equal(a, b), k
        else:
            assert a == b, k
    losses += [step() for _ in range(3)]
    torch.cuda.synchronize()
    assert tr.capture_count == captures, (tr.capture_count, captures)         # replayed, not recaptured
    assert tr.graph_steps == graph_steps + 3 and tr.step_count == 6
    assert int(tr.pstep.max()) == 6 and all(np.isfinite(losses)), losses
