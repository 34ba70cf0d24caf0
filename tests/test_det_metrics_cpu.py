"""Train-time evaluation on the CPU: the detection scoring rule (gpv1_amd.evaluators.det_ap_host: hand cases, an independent AP,
the IoU against the reference's utils/bbox_utils.py fixture), the CocoDetection / RefCocop classes, the export list of
libgpv_eval.so, the metric loops on the small model (kernels emulated by tests/cpu_shim.py) and best-checkpoint selection in the
training driver."""
import json
import os
import random
import subprocess

import numpy as np
import pytest
import torch

from tests import synth, cpu_shim
from tests.test_model_cpu import build_small, V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def shim():
    import gpv1_amd.ops as ops
    undo = cpu_shim.install()
    ops.RT.set_precise(True)
    yield
    ops.RT.set_precise(False)
    undo()


def cxcywh(x, y, w, h):
    """the prediction box that covers the ground-truth (x, y, w, h)"""
    return [x + 0.5 * w, y + 0.5 * h, w, h]


GT_A, GT_B = [0.125, 0.125, 0.25, 0.25], [0.5, 0.5, 0.25, 0.375]        # exact in float32
FAR = [0.9375, 0.9375, 0.03125, 0.03125]


def test_hand_computed_cases():
    from gpv1_amd.evaluators import det_ap_host
    # one exact hit
    ap, order, tp = det_ap_host([0.9], [cxcywh(*GT_A)], [GT_A])
    assert ap == 1.0 and order.tolist() == [0] and tp.tolist() == [1]
    # two ground-truth boxes, detections TP, FP, TP: recall 0.5 at precision 1, recall 1 at precision 2/3
    ap, order, tp = det_ap_host([0.9, 0.8, 0.7], [cxcywh(*GT_A), FAR, cxcywh(*GT_B)], [GT_A, GT_B])
    assert tp.tolist() == [1, 0, 1] and abs(ap - (0.5 * 1 + 0.5 * (2 / 3))) < 1e-15
    # a second detection on a taken box is a false positive (and visiting order is by score, not by query index)
    ap, order, tp = det_ap_host([0.5, 0.75], [cxcywh(*GT_A), cxcywh(*GT_A)], [GT_A, GT_B])
    assert order.tolist() == [1, 0] and tp.tolist() == [1, 0] and ap == 0.5
    # nothing over the threshold: the overlap is a quarter of the box, IoU = 0.25 / 1.75
    shifted = cxcywh(GT_A[0] + 0.125, GT_A[1] + 0.125, 0.25, 0.25)
    ap, _, tp = det_ap_host([0.9], [shifted], [GT_A])
    assert ap == 0.0 and tp.tolist() == [0]
    assert det_ap_host([0.9], [shifted], [GT_A], iou_thresh=0.125)[0] == 1.0
    # equal scores keep query order: query 0 takes the box, query 1 is the duplicate
    ap, order, tp = det_ap_host([0.5, 0.5, 0.5], [cxcywh(*GT_A), cxcywh(*GT_A), cxcywh(*GT_B)], [GT_A, GT_B])
    assert order.tolist() == [0, 1, 2] and tp.tolist() == [1, 0, 1]
    # no ground truth: 0, and counted
    ap, order, tp = det_ap_host([0.2, 0.9], [cxcywh(*GT_A), FAR], np.zeros((0, 4)))
    assert ap == 0.0 and order.tolist() == [1, 0] and tp.tolist() == [0, 0]
    # the candidate is the box of largest IoU even when it is taken: the detection does not fall back to the second best
    big = [0.125, 0.125, 0.25, 0.3125]                                     # IoU 0.8 with GT_A, contains it
    ap, _, tp = det_ap_host([0.9, 0.8], [cxcywh(*GT_A), cxcywh(*GT_A)], [GT_A, big])
    assert tp.tolist() == [1, 0] and ap == 0.5
    # the first maximum wins among equal IoUs
    ap, _, tp = det_ap_host([0.9, 0.8], [cxcywh(*GT_A), cxcywh(*GT_A)], [GT_A, GT_A])
    assert tp.tolist() == [1, 0]


def envelope_area(tp, npos):
    """independent O(n^2) statement of the AP: the area under p(r) = max precision at any recall >= r, by exact fractions"""
    from fractions import Fraction
    if npos == 0:
        return 0.0
    points, c = [], 0
    for i, t in enumerate(tp):
        c += int(t)
        points.append((Fraction(c, npos), Fraction(c, i + 1)))
    area = Fraction(0)
    for k in range(1, npos + 1):                        # the recall interval ((k - 1) / npos, k / npos]
        reach = [p for r, p in points if r >= Fraction(k, npos)]
        if reach:
            area += Fraction(1, npos) * max(reach)
    return float(area)


def test_ap_equals_the_area_under_the_precision_envelope():
    from gpv1_amd.evaluators import voc_ap
    rnd = random.Random(5)
    for case in range(200):
        npos = rnd.randint(0, 12)
        n = rnd.randint(1, 40)
        tp, left = [], npos
        for _ in range(n):
            hit = left > 0 and rnd.random() < 0.4
            left -= hit
            tp.append(int(hit))
        assert abs(voc_ap(tp, npos) - envelope_area(tp, npos)) < 1e-12, (case, tp, npos)


def test_iou_against_the_reference_fixture():
    """tests/golden/detection_iou.json: utils/bbox_utils.py compute_iou(fmt='xyxy') (tools/gen_golden_detection.py).  The reference
    divides by union + 1e-6: |delta| <= iou * 1e-6 / union, at most 1e-4 for boxes of area >= 0.01."""
    from gpv1_amd.evaluators import iou_one_to_many
    gold = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'detection_iou.json')))
    assert len(gold['cases']) >= 100
    worst = 0.0
    for c in gold['cases']:
        x, y, w, h = (np.float32(v) for v in c['a_xywh'])
        assert w * h >= 0.01 and c['b_xywh'][2] * c['b_xywh'][3] >= 0.01
        iou = iou_one_to_many((x, y, x + w, y + h, w, h), [c['b_xywh']])
        assert iou.dtype == np.float32 and iou.shape == (1,)
        d = abs(float(iou[0]) - c['iou'])
        worst = max(worst, d)
        assert d <= 1e-4, (c, float(iou[0]))
    print('worst |iou - reference|', worst)
    assert any(c['iou'] == 0 for c in gold['cases']) and any(c['iou'] > 0.99 for c in gold['cases'])


def _det_samples(task):
    key = 'sent_id' if task == 'RefCocop' else 'id'
    samples, boxes, preds = [], {}, {}
    W, H = 640, 480
    for i in range(6):
        gt = [[64 + 8 * i, 48, 160, 120], [320, 240, 128, 96 + 8 * i]][:1 + i % 2]
        s = {key: 100 + i, 'boxes': gt, 'image': {'W': W, 'H': H, 'image_id': i}, 'category_name': 'dog' if i < 4 else 'cat',
             'coco_categories': {'seen': ['dog'], 'unseen': (['cat'] if i >= 4 else [])}}
        samples.append(s)
        if i == 3:
            continue                                           # no prediction: absent
        g = np.asarray(gt, dtype=np.float32) / np.asarray([W, H, W, H], dtype=np.float32)
        pb = [cxcywh(*g[0]), FAR] if i % 3 else [FAR, cxcywh(*g[0])]     # sample 0: the hit comes second
        boxes[str(100 + i)] = {'boxes': np.asarray(pb, dtype=np.float32), 'relevance': np.asarray([0.9, 0.6], dtype=np.float32)}
        preds[str(100 + i)] = {'answer': ''}
    return samples, preds, boxes


@pytest.mark.parametrize('task', ['CocoDetection', 'RefCocop'])
def test_detection_evaluator_classes(task, tmp_path):
    from gpv1_amd import evaluators as E
    from gpv1_amd.compute_predictions import BoxesWriter
    samples, preds, boxes = _det_samples(task)
    ev = getattr(E, task)(samples, preds, boxes)
    assert ev.task == task and ev.task_id_name == ('sent_id' if task == 'RefCocop' else 'id')
    m = ev.evaluate()
    assert set(m) == {'absent', 'total', 'mAP'} and m['absent'] == 1 and m['total']['all'] == 5
    # per sample: 0: FP, TP of 1 gt -> 0.5; 1: TP of 2 gt -> 0.5; 2: TP -> 1; 4: 1 (1 gt); 5: 0.5
    assert abs(m['mAP'] - np.mean([0.5, 0.5, 1.0, 1.0, 0.5])) < 1e-15
    if task == 'CocoDetection':
        assert m['total']['dog'] == 3 and m['total']['cat'] == 2
    else:
        assert set(m['total']) == {'all'}
    held = ev.evaluate('held_out_concepts')
    assert held['total']['all'] == 2 and held['absent'] == 0 and abs(held['mAP'] - 0.75) < 1e-15
    seen = ev.evaluate('seen_concepts')
    assert seen['total']['all'] == 3 and seen['absent'] == 1 and abs(seen['mAP'] - np.mean([0.5, 0.5, 1.0])) < 1e-15
    assert ev.evaluate(iou_thresh=1.0)['mAP'] <= m['mAP']
    # the file compute_predictions.BoxesWriter writes is accepted as it is
    w = BoxesWriter(str(tmp_path / 'det_val_boxes.h5py'))
    for k, v in boxes.items():
        w.add(k, v['boxes'], v['relevance'])
    path = w.close()
    if path.endswith('.npz'):
        opened = np.load(path)
    else:
        import h5py
        opened = h5py.File(path, 'r')
    assert getattr(E, task)(samples, preds, opened).evaluate()['mAP'] == m['mAP']
    # the evaluator leaves the caller's arrays alone (the reference converts cxcywh in place)
    assert np.array_equal(boxes['101']['boxes'], _det_samples(task)[2]['101']['boxes'])


def test_eval_library_exports_exactly_the_declared_entry_points():
    """exports, header and nm: tests/test_abi_cpu.py, for every library; here what is the evaluation library's own"""
    import gpv1_amd.hip_eval as hip_eval
    # plain C: the header compiles as C99 on its own
    subprocess.run(['gcc', '-std=c99', '-fsyntax-only', '-x', 'c', os.path.join(ROOT, 'include', 'gpv_eval.h')], check=True)
    # no CPU path: the mirror refuses host tensors before anything is launched
    with pytest.raises(RuntimeError, match='GPU'):
        hip_eval.det_ap(torch.zeros(1, 3, 2), torch.zeros(1, 3, 4), torch.zeros(1, 1, 4), torch.zeros(1, dtype=torch.int32))


class _EvalSet:
    """an evaluation dataset: (image, query, target) items and the sample dicts beside them"""

    def __init__(self, n, size=(64, 96)):
        from gpv1_amd.train_distr import SyntheticCocoDataset
        self.items = SyntheticCocoDataset(n, synth.make_vocab(V), image_size=size, query_len=5, seed=3, tasks=('CocoDetection',))
        H, W = size
        self.samples = []
        for i in range(n):
            b = self.items[i][2]['boxes'].numpy().astype(np.float64)            # cxcywh 0..1 -> absolute xywh
            xywh = np.stack([(b[:, 0] - b[:, 2] / 2) * W, (b[:, 1] - b[:, 3] / 2) * H, b[:, 2] * W, b[:, 3] * H], 1)
            self.samples.append({'id': 700 + i, 'sent_id': 900 + i, 'question_id': 300 + i, 'cap_id': 500 + i, 'boxes': xywh.tolist(),
                                 'image': {'W': W, 'H': H, 'image_id': i}, 'category_name': 'dog', 'answer': 'w3',
                                 'all_answers': {'w3': 3, 'w5 w7': 1}, 'coco_categories': {'seen': ['dog'], 'unseen': []}})

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i]


def test_metric_loops_on_the_small_model(shim, tmp_path):
    """the (model, batches, samples, limit) functions end to end on the CPU shim; detection through host=True (the device scorer
    needs the GPU: tests/test_det_eval_gpu.py)"""
    from gpv1_amd import metrics
    from gpv1_amd import train_distr as td
    model, _ = build_small()
    ds = _EvalSet(5)

    def batches():
        return td.eval_batches(ds, 2, 'cpu')
    assert [len(t) for _, _, t in batches()] == [2, 2, 1]                           # the short last batch is kept
    acc = metrics.vqa_accuracy(model, batches(), ds.samples, 3)
    assert 0.0 <= acc <= 1.0 and not model.training
    scores, preds = metrics.cap_metrics(model, batches(), ds.samples, 4)
    assert scores == {} and sorted(preds) == ['500', '501', '502', '503'] and all(isinstance(p['answer'], str) for p in preds.values())
    scores, _ = metrics.cap_metrics(model, batches(), ds.samples, 4, scorer=lambda s, p: {'Cider': 0.25 * len(p)})
    assert scores == {'Cider': 1.0}
    cls = metrics.cls_metrics(model, batches(), ds.samples, None, synonyms={'w3': ['w3', 'w4'], 'dog': ['w5']})
    assert 0.0 <= cls <= 1.0
    bpath = str(tmp_path / 'det_val_boxes.h5py')
    m_all = metrics.det_metrics(model, batches(), ds.samples, None, host=True, boxes_path=bpath)
    m_3 = metrics.det_metrics(model, batches(), ds.samples, 3, host=True)
    r_3 = metrics.refexp_metrics(model, batches(), ds.samples, 3, host=True)
    assert 0.0 <= m_all <= 1.0 and m_3 == r_3
    wrote = bpath if os.path.exists(bpath) else os.path.splitext(bpath)[0] + '.npz'
    if wrote.endswith('.npz'):
        z = np.load(wrote)
        assert sorted({k.split('/')[0] for k in z.files}) == [str(700 + i) for i in range(5)]
        assert np.all(np.diff(z['702/relevance']) <= 0) and z['702/boxes'].shape == (len(z['702/relevance']), 4)
    with pytest.raises(RuntimeError, match='GPU'):                                  # the device path has no CPU fallback
        metrics.det_metrics(model, batches(), ds.samples, 2)


def _driver_cfg(tmp_path, **training):
    from gpv1_amd.config import from_dict
    m = synth.small_cfg(dropout=0.0)
    m['vocab'] = synth.make_vocab(V)
    m['vocab_embed'] = synth.synth_tensor('answer_head.vocab_embed', (V, 768))
    m['bert_layers'] = 2
    m['bert_dropout'] = 0.0
    tr = {'ckpt': None, 'freeze': False, 'frozen_epochs': 1, 'frozen_batch_size': 2, 'num_epochs': 3, 'batch_size': 2, 'log_step': 1,
          'ckpt_step': 1000, 'lr': 1e-3, 'lr_backbone': 1e-4, 'weight_decay': 1e-4, 'lr_warmup': True, 'lr_linear_decay': True,
          'lr_warmup_fraction': 0.25, 'clip_max_norm': 0.1, 'run_eval_at_launch': True, 'num_val_samples': {'coco_det': 3, 'coco_vqa': 2}}
    tr.update(training)
    return from_dict({'ckpt_dir': str(tmp_path / 'ckpts'), 'model': m, 'training': tr, 'synthetic_samples': 2})


def _train_set():
    from gpv1_amd.train_distr import SyntheticCocoDataset
    return SyntheticCocoDataset(2, synth.make_vocab(V), image_size=(64, 96), query_len=5)


def test_driver_selects_the_best_checkpoint(shim, tmp_path, monkeypatch):
    from gpv1_amd import train_distr as td
    seq = iter([0.3, 0.5, 0.4, 0.45, 0.7])
    calls, saves = [], []

    def stub(model, batches_, ds, limit):
        assert not model.training and not torch.is_grad_enabled()
        calls.append(limit)
        return next(seq)
    monkeypatch.setitem(td.EVAL_FNS, 'coco_det', stub)
    real_save = td.save_checkpoint

    def spy(path, model, trainer, epoch, step, metric=0.0):
        saves.append((os.path.basename(path), epoch, step, metric))
        real_save(path, model, trainer, epoch, step, metric)
    monkeypatch.setattr(td, 'save_checkpoint', spy)
    logs = []
    torch.manual_seed(0)
    cfg = _driver_cfg(tmp_path / 'a')
    evals = {'val': {'coco_det': _EvalSet(3)}}
    model, tr, step = td.train_worker(cfg, dataset=_train_set(), device='cpu', log=logs.append, eval_datasets=evals)
    assert step == 3 and calls == [3, 3, 3] and model.training
    # model.pth at the first and second evaluation only (0.3, then 0.5; 0.4 does not improve); model_last.pth after every epoch
    assert saves == [('model.pth', -1, 0, 0.3), ('model_last.pth', 0, 1, 0.3), ('model.pth', 0, 1, 0.5), ('model_last.pth', 1, 2, 0.5),
                     ('model_last.pth', 2, 3, 0.5)]
    best = torch.load(os.path.join(cfg.ckpt_dir, 'model.pth'), weights_only=False)
    last = torch.load(os.path.join(cfg.ckpt_dir, 'model_last.pth'), weights_only=False)
    assert set(best) == {'model', 'optimizer', 'epoch', 'step', 'lr', 'model_selection_metric', 'warmup_scheduler'} == set(last)
    assert best['model_selection_metric'] == 0.5 and best['epoch'] == 0 and best['step'] == 1
    assert last['epoch'] == 2 and last['step'] == 3 and last['model_selection_metric'] == 0.5
    assert sum('Saving checkpoint' in l for l in logs) == 2 and any('mAP: 0.4' in l for l in logs)
    # resume: best continues from the checkpoint's 0.5 -- 0.45 does not replace model.pth, 0.7 does
    del saves[:]
    cfg2 = _driver_cfg(tmp_path / 'a', ckpt=os.path.join(cfg.ckpt_dir, 'model.pth'), num_epochs=3)
    td.train_worker(cfg2, dataset=_train_set(), device='cpu', log=logs.append, eval_datasets=evals)
    assert [s for s in saves if s[0] == 'model.pth'] == [('model.pth', 1, 2, 0.7)]            # epochs 1 (0.45) and 2 (0.7) ran
    assert torch.load(os.path.join(cfg.ckpt_dir, 'model.pth'), weights_only=False)['model_selection_metric'] == 0.7


def test_driver_metric_sum_train_subset_and_missing_scorer(shim, tmp_path, monkeypatch):
    """model_selection_metric = vqa_acc + cider + det_map + cls_acc on 'val' only; refcocop is logged, not added; a caption dataset
    without a scorer contributes 0 and the log says so once; run_eval_at_launch=False skips the evaluation before the first epoch"""
    from gpv1_amd import train_distr as td
    seen = []
    for name, value in (('coco_vqa', 0.25), ('coco_cls', 0.125), ('coco_det', 0.5), ('refcocop', 0.0625)):
        monkeypatch.setitem(td.EVAL_FNS, name, lambda m, b, ds, limit, name=name, value=value: (seen.append((name, limit)), value)[1])
    monkeypatch.setitem(td.EVAL_FNS, 'coco_cap', lambda m, b, ds, limit: {})
    logs = []
    ds = _EvalSet(2)
    sets = {name: ds for name in ('coco_vqa', 'coco_cls', 'coco_cap', 'coco_det', 'refcocop')}
    cfg = _driver_cfg(tmp_path, num_epochs=3, run_eval_at_launch=False)
    td.train_worker(cfg, dataset=_train_set(), device='cpu', log=logs.append, eval_datasets={'train': sets, 'val': sets})
    assert len(seen) == 2 * 2 * 4 and ('coco_det', 3) in seen and ('coco_vqa', 2) in seen and ('coco_cls', None) in seen
    best = torch.load(os.path.join(cfg.ckpt_dir, 'model.pth'), weights_only=False)
    assert best['model_selection_metric'] == 0.25 + 0.5 + 0.125 and best['epoch'] == 0
    assert sum('no caption scorer' in l for l in logs) == 1
    assert sum('Subset: train' in l for l in logs) == sum('Subset: val' in l for l in logs) == 2 * 4


def test_driver_without_eval_datasets_writes_what_it_wrote(shim, tmp_path):
    from gpv1_amd import train_distr as td
    cfg = _driver_cfg(tmp_path, num_epochs=2)
    td.train_worker(cfg, dataset=_train_set(), device='cpu', log=lambda s: None)
    assert os.listdir(cfg.ckpt_dir) == ['model.pth']
    ck = torch.load(os.path.join(cfg.ckpt_dir, 'model.pth'), weights_only=False)
    assert ck['epoch'] == 1 and ck['step'] == 2 and ck['model_selection_metric'] == 0.0
