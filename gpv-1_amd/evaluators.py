"""Task metrics of the evaluation harness, the part that needs neither COCO nor the pycocoevalcap / detection_metrics packages
(offline remainder): the scoring rules of exp/gpv/evaluators.py:32-127,210-365 and exp/gpv/metrics.py:15-66.

  * CocoVqa.evaluate              (evaluators.py:36-82)    soft VQA accuracy min(#annotators / 3, 1) on the lower-cased answer, broken
                                                            down by answer_type / question_type, percentages rounded to 2 places
  * CocoClassification.evaluate   (evaluators.py:89-127)   correct iff the lower-cased prediction is one of the class's synonyms
  * vqa_accuracy_from_predictions (metrics.py:49-65)       the train-time variant: NO lower-casing, fraction rounded to 4 places

  * CocoDetection / RefCocop      (evaluators.py:210-365)  one AP per sample from the boxes file, mAP = np.mean(APs)

Captioning (Bleu / Cider) calls third-party scorers the reference keeps under third_party/ (empty in the checkout: un-vendored); its
input is the prediction file gpv1_amd.compute_predictions writes in the reference's layout, so the reference's evaluator consumes
it as it is.

Detection / referring-expression AP: the reference hands every sample to third_party/detection_metrics, which is un-vendored too, so
the per-sample rule is restated here (``det_ap_host``) and is the specification of the device scorer (csrc/det_ap.hip):
  * prediction box: x1 = cx - 0.5 w, y1 = cy - 0.5 h, x2 = x1 + w, y2 = y1 + h; ground truth (x, y, w, h) / (W, H, W, H), x2 = x + w,
    y2 = y + h; everything float32;
  * IoU in float32, in this order, no fused multiply-add: iw = max(0, min(ax2, bx2) - max(ax1, bx1)), ih likewise, inter = iw ih,
    union = (aw ah + bw bh) - inter, iou = inter / union if union > 0 else 0;
  * detections in descending score order, equal scores in query order (the reference's stable ``sorted(..., reverse=True)``); a
    detection's candidate is the ground-truth box of largest IoU (first maximum, an IoU of 0 is never a candidate); true positive
    iff that IoU >= iou_thresh and no earlier detection took the box, else false positive;
  * AP = PASCAL VOC all-point interpolation in float64 from the integer counts: rec_i = tp_i / npos, prec_i = tp_i / (tp_i + fp_i),
    padded with (0, 0) in front and (1, 0) behind, precision replaced by its running maximum from the right, sum of
    (rec_i - rec_{i-1}) prec_i over the points where recall changes; a sample without a ground-truth box scores 0 and is counted.
NOT reproduced, and not measurable here: the un-vendored scorer may use a pixel convention -- it rounds relative boxes to pixels of
the (W, H) image and measures widths, heights and areas with ``+ 1`` -- so its APs can differ from this rule's near the threshold.

Pinned by tests/golden/evaluators.json, produced by the reference's own classes (tools/gen_golden_evaluators.py); the IoU by
tests/golden/detection_iou.json, produced by the reference's utils/bbox_utils.py compute_iou (tools/gen_golden_detection.py)."""
from collections import Counter

import numpy as np

TASK_TO_ID = {'CocoVqa': 'question_id', 'CocoClassification': 'id', 'CocoCaptioning': 'cap_id', 'CocoDetection': 'id', 'RefCocop': 'sent_id'}
EPS = 1e-6


class CocoEval:
    """evaluators.py:17-29: samples keyed by str(sample[<task id>]); predictions = {key: {'answer': str}}"""

    def __init__(self, samples, predictions, boxes, task):
        self.task = task
        self.task_id_name = TASK_TO_ID[task]
        self.samples = {str(s[self.task_id_name]): s for s in samples}
        self.predictions = predictions
        self.boxes = boxes

    def sample_novelty(self, sample):
        return 'held_out_concepts' if len(sample['coco_categories']['unseen']) > 0 else 'seen_concepts'

    def _selected(self, novelty):
        """-> (key, sample) of the samples that count, and the number of selected samples without a prediction"""
        absent, picked = 0, []
        for k, sample in self.samples.items():
            if novelty != 'everything' and self.sample_novelty(sample) != novelty:
                continue
            if k not in self.predictions:
                absent += 1
                continue
            picked.append((k, sample))
        return picked, absent


class CocoVqa(CocoEval):
    def __init__(self, samples, predictions, boxes=None, task='CocoVqa'):
        super().__init__(samples, predictions, boxes, task)

    def evaluate(self, novelty='everything'):
        correct = {'all': 0, 'answer_type': Counter(), 'question_type': Counter()}
        total = {'all': 0, 'answer_type': Counter(), 'question_type': Counter()}
        picked, absent = self._selected(novelty)
        for k, sample in picked:
            pred = self.predictions[k]['answer'].lower()
            gt = {a.lower(): n for a, n in sample['all_answers'].items()}      # (later duplicates after lower-casing win, as in the reference)
            at, qt = sample['anno']['answer_type'], sample['anno']['question_type']
            if pred in gt:
                c = min(gt[pred] / 3, 1)
                correct['all'] += c
                correct['answer_type'][at] += c
                correct['question_type'][qt] += c
            total['all'] += 1
            total['answer_type'][at] += 1
            total['question_type'][qt] += 1
        accuracy = {'all': round(100 * correct['all'] / (EPS + total['all']), 2)}
        for key in ('answer_type', 'question_type'):
            accuracy[key] = {a: round(100 * correct[key][a] / (EPS + total[key][a]), 2) for a in total[key]}
        return {'correct': correct, 'total': total, 'absent': absent, 'accuracy': accuracy}


class CocoClassification(CocoEval):
    """synonyms: {coco class: [names]} -- the reference's data/coco/synonyms.py table (data the caller supplies; every class maps at
    least to itself there)"""

    def __init__(self, samples, predictions, boxes=None, task='CocoClassification', synonyms=None):
        super().__init__(samples, predictions, boxes, task)
        if synonyms is None:
            raise ValueError('CocoClassification needs the class -> synonyms table (data/coco/synonyms.py SYNONYMS)')
        self.synonyms = synonyms

    def evaluate(self, novelty='everything'):
        correct, total = Counter(), Counter()
        overall_correct = overall_total = 0
        picked, absent = self._selected(novelty)
        for k, sample in picked:
            pred = self.predictions[k]['answer'].lower()
            if pred in self.synonyms[sample['answer']]:
                overall_correct += 1
                correct[sample['answer']] += 1
            overall_total += 1
            total[sample['answer']] += 1
        return {'correct': correct, 'overall_correct': overall_correct, 'total': total, 'overall_total': overall_total, 'absent': absent,
                'accuracy': {k: round(correct[k] / (EPS + total[k]), 4) for k in total},
                'overall_accuracy': round(overall_correct / (EPS + overall_total), 4)}


def vqa_accuracy_from_predictions(pred_answers, samples, limit=None):
    """metrics.py:49-65 (the train-time VQA number): pred_answers[i] = the detokenised greedy answer of samples[i]; exact-case match
    against samples[i]['all_answers'] (no lower-casing here, unlike CocoVqa.evaluate), soft score min(n / 3, 1), at most `limit`
    samples; -> round(correct / (total + 1e-6), 4)"""
    correct, total = 0, 0
    for pred, sample in zip(pred_answers, samples):
        if limit is not None and total >= limit:
            break
        answers = sample['all_answers']
        if pred in answers:
            correct += min(answers[pred] / 3, 1)
        total += 1
    return round(correct / (total + 1e-6), 4)


def pred_xyxy(boxes):
    """[Q,4] cxcywh -> x1, y1, x2, y2, w, h (float32 columns): x1 = cx - 0.5 w, x2 = x1 + w"""
    b = np.asarray(boxes, dtype=np.float32).reshape(-1, 4)
    w, h = b[:, 2], b[:, 3]
    x1, y1 = b[:, 0] - np.float32(0.5) * w, b[:, 1] - np.float32(0.5) * h
    return x1, y1, x1 + w, y1 + h, w, h


def iou_one_to_many(a, gt):
    """float32 IoU of one box a = (x1, y1, x2, y2, w, h) with the ground-truth boxes gt [G,4] (x, y, w, h): the order of operations
    of the module docstring, every intermediate rounded to float32 (numpy never fuses)"""
    ax1, ay1, ax2, ay2, aw, ah = (np.float32(v) for v in a)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    bx1, by1, bw, bh = gt[:, 0], gt[:, 1], gt[:, 2], gt[:, 3]
    bx2, by2 = bx1 + bw, by1 + bh
    zero = np.float32(0)
    iw = np.maximum(zero, np.minimum(ax2, bx2) - np.maximum(ax1, bx1))
    ih = np.maximum(zero, np.minimum(ay2, by2) - np.maximum(ay1, by1))
    inter = iw * ih
    union = (aw * ah + bw * bh) - inter
    with np.errstate(divide='ignore', invalid='ignore'):
        iou = np.where(union > 0, inter / np.where(union > 0, union, np.float32(1)), zero)
    return iou.astype(np.float32)


def voc_ap(tp, npos):
    """all-point interpolated AP (float64) of the true-positive flags ``tp`` (detection order) against npos ground-truth boxes"""
    if npos <= 0:
        return 0.0
    ctp = np.cumsum(np.asarray(tp, dtype=np.int64))
    n = np.arange(1, len(ctp) + 1, dtype=np.int64)                       # tp_i + fp_i
    mrec = np.concatenate([[0.0], ctp / np.float64(npos), [1.0]])
    mpre = np.concatenate([[0.0], ctp / n.astype(np.float64), [0.0]])
    for i in range(len(mpre) - 2, -1, -1):
        mpre[i] = max(mpre[i], mpre[i + 1])
    ap = 0.0
    for i in range(1, len(mrec)):
        if mrec[i] != mrec[i - 1]:
            ap += (mrec[i] - mrec[i - 1]) * mpre[i]
    return float(ap)


def det_ap_host(scores, boxes, gt, iou_thresh=0.5):
    """the per-sample rule (module docstring).  scores [Q] float32, boxes [Q,4] cxcywh, gt [G,4] (x, y, w, h) normalised, G >= 0
    -> (ap float, order [Q] int32: query index per visited position, tp [Q] uint8 per visited position)"""
    scores = np.asarray(scores, dtype=np.float32).reshape(-1)
    gt = np.asarray(gt, dtype=np.float32).reshape(-1, 4)
    order = np.asarray(sorted(range(len(scores)), key=lambda i: scores[i], reverse=True), dtype=np.int32)   # stable
    cols = pred_xyxy(boxes)
    thresh = np.float32(iou_thresh)
    taken = np.zeros(len(gt), dtype=bool)
    tp = np.zeros(len(scores), dtype=np.uint8)
    if len(gt):
        for r, q in enumerate(order):
            iou = iou_one_to_many([c[q] for c in cols], gt)
            g = int(np.argmax(iou))                                      # first maximum
            if iou[g] > 0 and iou[g] >= thresh and not taken[g]:
                taken[g] = True
                tp[r] = 1
    return voc_ap(tp, len(gt)), order, tp


def gt_boxes_normalised(sample):
    """sample['boxes'] absolute (x, y, w, h) / the image's (W, H, W, H) -> float32 [G,4]"""
    W, H = sample['image']['W'], sample['image']['H']
    gt = np.asarray(sample['boxes'], dtype=np.float32).reshape(-1, 4)
    return gt / np.asarray([W, H, W, H], dtype=np.float32)


def _box_entry(boxes, key):
    """boxes[key] -> (boxes [Q,4], relevance [Q]) from an open h5py file / a dict of groups, or from the .npz BoxesWriter writes
    without h5py ('<key>/boxes', '<key>/relevance')"""
    try:
        grp = boxes[key]
        return np.array(grp['boxes'][()], dtype=np.float32), np.array(grp['relevance'][()], dtype=np.float32)
    except KeyError:
        return np.array(boxes[f'{key}/boxes'], dtype=np.float32), np.array(boxes[f'{key}/relevance'], dtype=np.float32)


class CocoDetection(CocoEval):
    """evaluators.py:210-287: per-sample AP of the boxes file against sample['boxes'], mAP = np.mean(APs); `boxes` is what
    compute_predictions.BoxesWriter wrote (h5py file or np.load of the .npz) or any {key: {'boxes', 'relevance'}}"""
    per_category = True

    def __init__(self, samples, predictions, boxes, task='CocoDetection'):
        super().__init__(samples, predictions, boxes, task)

    def evaluate(self, novelty='everything', iou_thresh=0.5):
        total, APs = Counter(), []
        picked, absent = self._selected(novelty)
        for k, sample in picked:
            pred_boxes, scores = _box_entry(self.boxes, k)
            APs.append(det_ap_host(scores, pred_boxes, gt_boxes_normalised(sample), iou_thresh)[0])
            total['all'] += 1
            if self.per_category:
                total[sample['category_name']] += 1
        return {'absent': absent, 'total': total, 'mAP': np.mean(APs)}


class RefCocop(CocoDetection):
    """evaluators.py:289-365: the same scoring keyed by sent_id, totals under 'all' only"""
    per_category = False

    def __init__(self, samples, predictions, boxes, task='RefCocop'):
        super().__init__(samples, predictions, boxes, task)
