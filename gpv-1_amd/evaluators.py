"""Task metrics of the evaluation harness, the part that needs neither COCO nor the pycocoevalcap / detection_metrics packages
(offline remainder): the scoring rules of exp/gpv/evaluators.py:32-127,210-365 and exp/gpv/metrics.py:15-66.

  * CocoVqa.evaluate              (evaluators.py:36-82)    soft VQA accuracy min(#annotators / 3, 1) on the lower-cased answer, broken
                                                            down by answer_type / question_type, percentages rounded to 2 places
  * CocoClassification.evaluate   (evaluators.py:89-127)   correct iff the lower-cased prediction is one of the class's synonyms
  * vqa_accuracy_from_predictions (metrics.py:49-65)       the train-time variant: NO lower-casing, fraction rounded to 4 places

  * CocoDetection / RefCocop      (evaluators.py:210-365)  one AP per sample from the boxes file, mAP = np.mean(APs)

  * CocoCaptioning.evaluate       (evaluators.py:130-207)  Bleu1..4 and CIDEr-D of the lower-cased prediction against every caption of
                                                            the same image among the given samples

Captioning: the reference calls pycocoevalcap's Bleu and Cider (third_party/, empty in the checkout: un-vendored), so the rule is
restated here from the published algorithm (bleu_scorer.py, cider_scorer.py) -- ``caption_scores_host`` -- and is the specification
of the device scorer (csrc/caption_score.hip).  hyps[i]: a list of words, refs[i]: a non-empty list of such lists, N = len(hyps):
  * n-grams: every contiguous window of 1..4 words of a caption, counted with multiplicity;
  * Bleu (option 'closest', corpus level), per entry: testlen = len(hyp); reflen = the reference length closest to testlen, the
    shorter one on a tie (min((abs(l - testlen), l) for l in reflens)[1]); guess[k] = max(0, testlen - k), k = 0..3; correct[k] =
    sum over the hypothesis' distinct (k+1)-grams of min(count in hyp, max over refs of the count in that ref).  The totals over the
    entries are integers; with b = 1, for k = 0..3: b *= (correct[k] + 1e-15) / (guess[k] + 1e-9), Bleu_{k+1} = b ** (1 / (k + 1));
    ratio = (testlen + 1e-15) / (reflen + 1e-9); if ratio < 1 every Bleu_k is multiplied by exp(1 - 1 / ratio);
  * CIDEr-D (n = 4, sigma = 6): df[g] = the number of entries in which n-gram g occurs in at least one reference; the weight table
    w[d] = log(N) - log(max(1, d)), d = 0..N, float64, computed ONCE with numpy (``caption_tables``) and read by the host rule and by
    the kernel alike -- neither recomputes a logarithm; the vector of a caption at order n is tf(g) * w[df[g]] over its distinct
    n-grams (an n-gram no reference holds has df 0), its norm the square root of the sum of squares; the caption's ``length`` is the
    number of its BIGRAM occurrences, max(0, len - 1) (a quirk of the original, kept); for a hypothesis h and a reference r,
    val[n] = sum over h's distinct n-grams of min(vec_h[g], vec_r[g]) * vec_r[g], divided by norm_h[n] * norm_r[n] only if both are
    non-zero, times pen[|length_h - length_r|], pen[d] = e ** (-(d * d) / (2 * 36)), again one shared float64 table; the entry scores
    10 * (sum over n of the sum over refs of val[n]) / 4 / len(refs); Cider = the float64 mean of the entry scores.  With N = 1 every
    weight is 0 and so is the score.
NOT reproduced: the Stanford PTB tokenizer (a Java program).  ``simple_caption_tokenize`` lower-cases, splits on whitespace and drops
the punctuation of pycocoevalcap's removal list; it does not split clitics (n't, 's), so a figure that depends on that splitting --
any published COCO caption score -- is not reproduced to the digit.  Pass ``tokenize=`` to use the real tool.

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
import math
import re
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


CAP_ORDERS = 4
CAP_SIGMA = 6.0
CAP_KEYS = ('Bleu1', 'Bleu2', 'Bleu3', 'Bleu4', 'Cider')
# pycocoevalcap's PUNCTUATIONS (ptbtokenizer.py), lower-cased: tokens the PTB tokenizer's output is filtered by
CAP_PUNCTUATION = ("''", "'", '``', '`', '-lrb-', '-rrb-', '-lcb-', '-rcb-', '.', '?', '!', ',', ':', '-', '--', '...', ';')
_CAP_BRACKETS = re.compile(r'-(?:lrb|rrb|lcb|rcb)-')
_CAP_ANYWHERE = re.compile(r"\.\.\.|--|``|''|[.?!,:;]")


def simple_caption_tokenize(text):
    """str -> list of words: lower-cased, split on whitespace, the marks of CAP_PUNCTUATION split off the words and dropped.
    `. ? ! , : ; ... -- `` ''` and the bracket names split a word wherever they stand; `'`, '`' and `-` are taken off a word's ends
    only, so "don't" and "well-known" stay one word each.
    NOT reproduced: the Stanford PTB tokenizer the reference runs -- no clitic splitting ("don't" -> "do n't", "dog's" -> "dog 's"),
    no number handling ("3.5" becomes "3", "5" here) -- and so any figure that depends on it."""
    words = []
    for tok in str(text).lower().split():
        for part in _CAP_ANYWHERE.sub(' ', _CAP_BRACKETS.sub(' ', tok)).split():
            part = part.strip("'`-")
            if part:
                words.append(part)
    return words


def caption_tables(n_entries, max_len):
    """the two float64 tables both the host rule and the kernel read: weight[d] = log(N) - log(max(1, d)) for d = 0..N, and
    pen[d] = e ** (-(d * d) / (2 * sigma^2)) for d = 0..max(1, max_len) - 1 (d: a difference of bigram counts)"""
    d = np.arange(n_entries + 1, dtype=np.float64)
    weight = np.log(np.float64(max(n_entries, 1))) - np.log(np.maximum(1.0, d))
    k = np.arange(max(1, int(max_len)), dtype=np.float64)
    pen = np.e ** (-(k * k) / (2 * CAP_SIGMA ** 2))
    return weight, pen


def _ngram_counts(words):
    """{n-gram tuple: occurrences}, orders 1..4"""
    c = Counter()
    for n in range(1, CAP_ORDERS + 1):
        for p in range(len(words) - n + 1):
            c[tuple(words[p:p + n])] += 1
    return c


def bleu_from_totals(testlen, reflen, guess, correct):
    """corpus Bleu1..4 from the integer totals (module docstring) -> list of 4 floats"""
    bleus, b = [], 1.0
    for k in range(CAP_ORDERS):
        b *= (float(correct[k]) + 1e-15) / (float(guess[k]) + 1e-9)
        bleus.append(b ** (1.0 / (k + 1)))
    ratio = (float(testlen) + 1e-15) / (float(reflen) + 1e-9)
    if ratio < 1:
        factor = math.exp(1 - 1 / ratio)                               # underflows to 0.0 for an empty hypothesis corpus
        bleus = [x * factor for x in bleus]
    return bleus


def caption_result(testlen, reflen, guess, correct, cider):
    """the finish both paths share: per-entry integers [N], [N], [N,4], [N,4] and per-entry CIDEr [N] float64 -> the result dict
    (int64 sums, float64 mean)"""
    testlen, reflen = np.asarray(testlen, dtype=np.int64).reshape(-1), np.asarray(reflen, dtype=np.int64).reshape(-1)
    guess, correct = np.asarray(guess, dtype=np.int64).reshape(-1, CAP_ORDERS), np.asarray(correct, dtype=np.int64).reshape(-1, CAP_ORDERS)
    cider = np.asarray(cider, dtype=np.float64).reshape(-1)
    totals = {'testlen': int(testlen.sum()), 'reflen': int(reflen.sum()), 'guess': [int(v) for v in guess.sum(0)],
              'correct': [int(v) for v in correct.sum(0)]}
    if len(cider) == 0:
        bleus, mean = [0.0] * CAP_ORDERS, 0.0
    else:
        bleus, mean = bleu_from_totals(totals['testlen'], totals['reflen'], totals['guess'], totals['correct']), float(np.mean(cider))
    out = {f'Bleu{k + 1}': bleus[k] for k in range(CAP_ORDERS)}
    out.update(Cider=mean, cider_entries=cider, bleu_totals=totals,
               bleu_entries={'testlen': testlen, 'reflen': reflen, 'guess': guess, 'correct': correct})
    return out


def caption_scores_host(hyps, refs):
    """the rule of the module docstring, as pycocoevalcap states it (dicts of n-gram tuples).  hyps[i]: list of words, refs[i]:
    non-empty list of lists of words -> {'Bleu1'..'Bleu4', 'Cider', 'cider_entries': float64 [N], 'bleu_totals': {'testlen',
    'reflen', 'guess' [4], 'correct' [4]} ints, 'bleu_entries': the same per entry, 'df': {n-gram tuple: document frequency}}"""
    N = len(hyps)
    if len(refs) != N or any(len(r) == 0 for r in refs):
        raise ValueError('caption_scores_host: every entry needs a hypothesis and at least one reference')
    hyp_c = [_ngram_counts(h) for h in hyps]
    ref_c = [[_ngram_counts(r) for r in rs] for rs in refs]
    df = Counter()
    for rcs in ref_c:
        for g in set().union(*rcs):
            df[g] += 1
    max_len = max([len(h) for h in hyps] + [len(r) for rs in refs for r in rs] + [1])
    weight, pen = caption_tables(N, max_len)

    def vector(counts):
        vec = [{} for _ in range(CAP_ORDERS)]
        for g, tf in counts.items():
            vec[len(g) - 1][g] = float(tf) * weight[df.get(g, 0)]
        return vec, [math.sqrt(sum(v * v for v in o.values())) for o in vec]

    testlen, reflen, guess, correct, cider = [], [], [], [], []
    for i in range(N):
        tl = len(hyps[i])
        testlen.append(tl)
        reflen.append(min((abs(len(r) - tl), len(r)) for r in refs[i])[1])
        guess.append([max(0, tl - k) for k in range(CAP_ORDERS)])
        cor = [0] * CAP_ORDERS
        for g, c in hyp_c[i].items():
            cor[len(g) - 1] += min(c, max(rc.get(g, 0) for rc in ref_c[i]))
        correct.append(cor)
        vec_h, norm_h = vector(hyp_c[i])
        length_h = max(0, tl - 1)
        total = [0.0] * CAP_ORDERS
        for r, rc in zip(refs[i], ref_c[i]):
            vec_r, norm_r = vector(rc)
            p = pen[abs(length_h - max(0, len(r) - 1))]
            for n in range(CAP_ORDERS):
                val = sum(min(v, vec_r[n].get(g, 0.0)) * vec_r[n].get(g, 0.0) for g, v in vec_h[n].items())
                if norm_h[n] != 0 and norm_r[n] != 0:
                    val /= norm_h[n] * norm_r[n]
                total[n] += val * p
        cider.append(10.0 * sum(total) / CAP_ORDERS / len(refs[i]))
    out = caption_result(testlen, reflen, guess, correct, cider)
    out['df'] = dict(df)
    return out


class CocoCaptioning(CocoEval):
    """evaluators.py:130-207: an entry is a cap_id with a prediction; its references are the lower-cased answers of every GIVEN sample
    of the same (image.subset, image.image_id); the hypothesis is the lower-cased prediction.  tokenize: str -> words
    (simple_caption_tokenize; the reference runs the PTB tokenizer); scores: (hyps, refs) -> the dict of caption_scores_host (the
    device scorer of gpv1_amd.caption_scorer has the same signature)."""

    def __init__(self, samples, predictions, boxes=None, task='CocoCaptioning', tokenize=None, scores=None):
        super().__init__(samples, predictions, boxes, task)
        self.tokenize = simple_caption_tokenize if tokenize is None else tokenize
        self.scores = caption_scores_host if scores is None else scores
        self.subset_imgid2gtcaps = {}
        for s in samples:
            self.subset_imgid2gtcaps.setdefault(self._image_key(s), []).append(s['answer'].lower())

    @staticmethod
    def _image_key(sample):
        return f"{sample['image'].get('subset')}_{str(sample['image']['image_id']).zfill(12)}"

    def evaluate(self, novelty='everything'):
        picked, absent = self._selected(novelty)
        cache = {}
        hyps, refs = [], []
        for k, sample in picked:
            key = self._image_key(sample)
            if key not in cache:
                cache[key] = [self.tokenize(c) for c in self.subset_imgid2gtcaps[key]]
            hyps.append(self.tokenize(self.predictions[k]['answer'].lower()))
            refs.append(cache[key])
        if hyps:
            full = self.scores(hyps, refs)
            scores = {k: full[k] for k in CAP_KEYS}
        else:
            scores = {k: 0 for k in CAP_KEYS}
        return {'absent': absent, 'total': len(hyps), 'scores': scores}
