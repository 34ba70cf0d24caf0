"""Train-time metrics: the numbers the training driver selects its checkpoint by.

Reference: exp/gpv/metrics.py -- ``vqa_accuracy`` :15-66, ``cap_metrics`` :68-119, ``cls_metrics`` :147-199, ``det_metrics`` :217-291,
``refexp_metrics`` :294-363.  Every function is ``(model, batches, samples, limit)``:
  * ``batches``: an iterable of ``(NestedTensor | list of CHW tensors, queries, targets)`` in dataset order (what
    ``train_distr.eval_batches`` yields; the targets are not read), ``samples``: the dataset's sample dicts in the same order
    (the reference's ``dataloader.dataset.samples``), ``limit``: at most that many samples are evaluated
    (``cfg.training.num_val_samples[name]``);
  * greedy forward ``model(imgs, queries, None)`` under ``model.eval()`` / ``torch.no_grad()``; the answer is the top-1 token row with
    every ``__stop__`` / ``__pad__`` removed, detokenised (the train-time loops filter, they do not cut at the first stop);
  * classification confines the answer with ``compute_predictions.create_vocab_mask``.

Detection / referring expressions: the reference writes every sample's sorted boxes to an HDF5 file, reads it back and scores
sample by sample in Python.  Here the per-sample AP is one launch per batch on the model's stream (``hip_eval.det_ap``, rule:
``evaluators.det_ap_host``) into a preallocated ``ap_all[N]`` device buffer; nothing is copied or synchronised per batch by the
scorer, and the dataset ends in one device-to-host copy and one float64 ``np.mean``.  ``host=True`` is the comparison path:
``inference.decode_outputs`` plus the ``evaluators`` classes, as the reference does it.

Captioning: ``cap_metrics`` returns the predictions and calls a scorer only if the caller supplies one;
``caption_scorer.CaptionScorer`` is that scorer (Bleu / CIDEr-D restated, on the device; the PTB tokenizer is not reproduced).
"""
import numpy as np
import torch

from . import evaluators
from .compute_predictions import BoxesWriter, TASK_TO_ID, create_vocab_mask
from .inference import decode_outputs, detokenize
from .misc import NestedTensor, nested_tensor_from_tensor_list


def _device(model):
    return model.vision_token.device


def _images(imgs, dev):
    return imgs if isinstance(imgs, NestedTensor) else nested_tensor_from_tensor_list([x.to(dev) for x in imgs])


def _greedy_answers(model, outputs):
    """metrics.py:43-53: top-1 tokens, every __stop__ / __pad__ dropped, detokenised"""
    top1 = torch.topk(outputs['answer_logits'][-1].float(), k=1, dim=-1).indices[..., 0].detach().cpu().numpy()
    return [detokenize([w for w in words if w not in ('__stop__', '__pad__')]) for words in model.token_ids_to_words(top1)]


def _answer_loop(model, batches, samples, limit, vocab_mask=None):
    """-> the greedy answers of the first min(limit, len(samples)) samples"""
    dev = _device(model)
    n = len(samples) if limit is None else min(int(limit), len(samples))
    if vocab_mask is not None:
        vocab_mask = torch.as_tensor(vocab_mask, dtype=torch.float32, device=dev)
    model.eval()
    answers = []
    for imgs, queries, _ in batches:
        if len(answers) >= n:
            break
        outputs = model(_images(imgs, dev), queries, None, vocab_mask=vocab_mask)
        answers.extend(_greedy_answers(model, outputs))
    return answers[:n]


def _beam_answers(model, batches, samples, limit, beam_size, beam=None):
    """-> slot 0 of GPV.forward_beam_search (the best hypothesis, its words up to __stop__ / __pad__) of the first min(limit,
    len(samples)) samples, detokenised"""
    from .inference import beam_options
    dev = _device(model)
    n = len(samples) if limit is None else min(int(limit), len(samples))
    model.eval()
    answers = []
    for imgs, queries, _ in batches:
        if len(answers) >= n:
            break
        outputs = model.forward_beam_search(_images(imgs, dev), queries, beam_size=beam_size, **beam_options(beam))
        answers.extend(detokenize(hyps[0]) for hyps in outputs['answers'])
    return answers[:n]


@torch.no_grad()
def vqa_accuracy(model, batches, samples, limit=None):
    """metrics.py:15-66 -> soft VQA accuracy, rounded to 4 places"""
    answers = _answer_loop(model, batches, samples, limit)
    return evaluators.vqa_accuracy_from_predictions(answers, samples, limit=len(answers))


@torch.no_grad()
def cap_metrics(model, batches, samples, limit=None, scorer=None, beam_size=None, beam=None):
    """metrics.py:68-119 -> (scores, predictions): predictions = {str(cap_id): {'answer': str}}; scores = scorer(samples, predictions)
    (the reference's {'Bleu1'.., 'Cider'}) or {} without a scorer.  beam_size / beam (added; the keys of inference.beam_options, among
    them no_repeat_ngram, min_length, repetition_penalty): the caption is the best hypothesis of GPV.forward_beam_search, cut at the
    first __stop__ / __pad__; the default stays the greedy decode, unchanged"""
    if beam_size:
        answers = _beam_answers(model, batches, samples, limit, int(beam_size), beam)
    else:
        answers = _answer_loop(model, batches, samples, limit)
    predictions = {str(s['cap_id']): {'answer': a} for s, a in zip(samples, answers)}
    return (scorer(samples, predictions) if scorer is not None else {}), predictions


@torch.no_grad()
def cls_metrics(model, batches, samples, limit=None, synonyms=None, answer_set='tokens', classes=None, beam_size=4):
    """metrics.py:147-199 -> overall accuracy.  synonyms: the reference's {class: [names]} table (data the caller supplies); without
    it every class answers to its own name only, in the mask and in the scoring.  answer_set (added): 'tokens' confines the greedy
    decode with the reference's flat vocabulary mask, unchanged; 'phrases' answers from the closed set of whole names
    (compute_predictions.create_phrase_set over `classes`, default the COCO classes; GPV.choose with `beam_size`): the answer is the
    class name of the chosen phrase"""
    if answer_set not in ('tokens', 'phrases'):
        raise ValueError(f"cls_metrics: answer_set must be 'tokens' or 'phrases', got {answer_set!r}")
    if answer_set == 'phrases':
        from .compute_predictions import COCO_CLASSES, create_phrase_set
        classes = COCO_CLASSES if classes is None else classes
        pset, owner = create_phrase_set(model, classes, synonyms=synonyms, use_syns=synonyms is not None)
        dev = _device(model)
        n = len(samples) if limit is None else min(int(limit), len(samples))
        model.eval()
        picks = []
        for imgs, queries, _ in batches:
            if sum(len(p) for p in picks) >= n:
                break
            picks.append(model.choose(_images(imgs, dev), queries, pset, beam_size=beam_size)[0])
        answers = [classes[owner[i]] for p in picks for i in p.cpu().tolist()][:n]
    else:
        _, mask = create_vocab_mask(model, synonyms=synonyms, use_syns=synonyms is not None)
        answers = _answer_loop(model, batches, samples, limit, vocab_mask=mask)
    predictions = {str(s['id']): {'answer': a} for s, a in zip(samples, answers)}
    if synonyms is None:
        synonyms = {s['answer']: [s['answer']] for s in samples}
    return evaluators.CocoClassification(samples, predictions, None, synonyms=synonyms).evaluate()['overall_accuracy']


def _gt_batch(samples, G, dev):
    """ground truth of a batch as the scorer reads it: [B,G,4] float32 (x, y, w, h) normalised, zero-padded, and the counts"""
    gt = np.zeros((len(samples), max(G, 1), 4), dtype=np.float32)
    count = np.zeros(len(samples), dtype=np.int32)
    for i, s in enumerate(samples):
        b = evaluators.gt_boxes_normalised(s)
        gt[i, :len(b)] = b
        count[i] = len(b)
    return torch.from_numpy(gt).to(dev, non_blocking=True), torch.from_numpy(count).to(dev, non_blocking=True)


@torch.no_grad()
def det_metrics(model, batches, samples, limit=None, host=False, boxes_path=None, iou_thresh=0.5, task='CocoDetection'):
    """metrics.py:217-291 -> mAP (float64 mean of the per-sample APs).
    host=False: the device scorer, one launch per batch, no per-batch copy or sync of its own.
    host=True: decode_outputs + evaluators.CocoDetection / RefCocop on the host (the comparison path).
    host='kernel_scores': the host path on the device scorer's scores and order (so that both paths rank the same float32 numbers:
    torch's softmax and the kernel's may differ in the last bit); IoU, matching and AP still on the host.
    boxes_path: also write the sorted boxes / relevance of every evaluated sample there (compute_predictions.BoxesWriter layout:
    what make_predictions writes; an .npz beside that name without h5py)."""
    from . import hip_eval
    dev = _device(model)
    id_name = TASK_TO_ID[task]
    n = len(samples) if limit is None else min(int(limit), len(samples))
    samples = list(samples[:n])
    G = max([len(s['boxes']) for s in samples], default=0)
    model.eval()
    ap_all = score_all = boxes_all = None
    host_boxes, done = {}, 0
    for imgs, queries, _ in batches:
        if done >= n:
            break
        outputs = model(_images(imgs, dev), queries, None)
        logits = outputs['pred_relevance_logits'].float()
        pred = outputs['pred_boxes'].float()
        B = min(logits.shape[0], n - done)
        Q = logits.shape[1]
        chunk = samples[done:done + B]
        if host is True:
            for s, d in zip(chunk, decode_outputs(outputs, model)):
                host_boxes[str(s[id_name])] = {'boxes': d['boxes'], 'relevance': d['relevance']}
        else:
            if ap_all is None:
                ap_all = torch.zeros(n, dtype=torch.float64, device=dev)
                if boxes_path is not None or host:
                    score_all = torch.empty(n, Q, dtype=torch.float32, device=dev)
                    boxes_all = torch.empty(n, Q, 4, dtype=torch.float32, device=dev)
            gt, count = _gt_batch(chunk, G, dev)
            pred_b = pred[:B].contiguous()
            score, order, _, _ = hip_eval.det_ap(logits[:B].contiguous(), pred_b, gt, count, iou_thresh,
                                                 score=None if score_all is None else score_all[done:done + B], ap=ap_all[done:done + B])
            if boxes_all is not None:
                torch.gather(pred_b, 1, order.long().unsqueeze(-1).expand(B, Q, 4), out=boxes_all[done:done + B])
        done += B
    predictions = {str(s[id_name]): {'answer': ''} for s in samples[:done]}
    if host is not True and score_all is not None:
        score_h, boxes_h = score_all[:done].cpu().numpy(), boxes_all[:done].cpu().numpy()
        host_boxes = {str(s[id_name]): {'boxes': boxes_h[i], 'relevance': score_h[i]} for i, s in enumerate(samples[:done])}
    if boxes_path is not None:
        writer = BoxesWriter(boxes_path)
        for k, v in host_boxes.items():
            writer.add(k, v['boxes'], v['relevance'])
        writer.close()
    if host:
        cls = evaluators.RefCocop if task == 'RefCocop' else evaluators.CocoDetection
        return float(cls(samples[:done], predictions, host_boxes, task=task).evaluate(iou_thresh=iou_thresh)['mAP'])
    if done == 0:
        return float('nan')
    return float(np.mean(ap_all[:done].cpu().numpy()))                  # the one device-to-host copy (waits for the stream)


def refexp_metrics(model, batches, samples, limit=None, host=False, boxes_path=None, iou_thresh=0.5):
    """metrics.py:294-363: det_metrics keyed by sent_id, scored by evaluators.RefCocop"""
    return det_metrics(model, batches, samples, limit, host=host, boxes_path=boxes_path, iou_thresh=iou_thresh, task='RefCocop')
