"""Batched prediction files for the reference's evaluators.

Reference: exp/gpv/compute_predictions.py -- ``make_predictions`` :30-85, ``create_coco_vocab_mask`` :88-109.
Reproduced:
  * the classification vocabulary mask (:88-109): -10000 on every vocabulary entry, 0 on the word tokens of the class
    names (optionally of their synonyms) that are in the vocabulary and on ``__stop__`` / ``__pad__``; passed to
    ``model(imgs, queries, None, vocab_mask=...)`` only for ``CocoClassification`` (:31-34);
  * the loop (:43-80): greedy forward, boxes sorted by ``softmax(relevance)[..., 0]`` descending (stable, all
    ``num_queries`` boxes kept), answer = top-1 tokens up to the first ``__stop__`` / ``__pad__``, detokenised;
    ``num_eval_batches`` stops AFTER batch index ``num_eval_batches`` like the reference's ``i > num_eval_batches``;
  * the two files (:36-38,72-85): ``<task>_<data_split>_<subset>_predictions.json`` = {sample_id: {'answer': str}} and the
    boxes file with one group per sample id holding ``boxes`` [Q,4] float32 and ``relevance`` [Q] float32.
Differences: the boxes file is HDF5 (``<task>_<subset>_boxes.h5py``, the reference's name) when ``h5py`` is importable and
an ``.npz`` with the keys ``'<sample_id>/boxes'`` / ``'<sample_id>/relevance'`` otherwise (this image has no h5py;
``boxes_to_h5py`` converts on a machine that has); dataset construction, image decoding and the evaluators themselves are
out of scope -- ``batches`` is any iterable of ``(NestedTensor | list of CHW tensors, queries, sample_ids)``.
The 80 class names are the public COCO detection categories (the reference reads them from data/coco/synonyms.py).
"""
import json
import os
import re

import numpy as np
import torch

from .inference import beam_options, decode_outputs
from .misc import NestedTensor, nested_tensor_from_tensor_list

TASK_TO_ID = {'CocoVqa': 'question_id', 'CocoCaptioning': 'cap_id', 'CocoClassification': 'id', 'CocoDetection': 'id',
              'RefCocop': 'sent_id'}                                   # exp/gpv/evaluators.py task_to_id

COCO_CLASSES = (
    'person', 'bicycle', 'car', 'motorcycle', 'airplane', 'bus', 'train', 'truck', 'boat', 'traffic light', 'fire hydrant',
    'stop sign', 'parking meter', 'bench', 'bird', 'cat', 'dog', 'horse', 'sheep', 'cow', 'elephant', 'bear', 'zebra',
    'giraffe', 'backpack', 'umbrella', 'handbag', 'tie', 'suitcase', 'frisbee', 'skis', 'snowboard', 'sports ball', 'kite',
    'baseball bat', 'baseball glove', 'skateboard', 'surfboard', 'tennis racket', 'bottle', 'wine glass', 'cup', 'fork',
    'knife', 'spoon', 'bowl', 'banana', 'apple', 'sandwich', 'orange', 'broccoli', 'carrot', 'hot dog', 'pizza', 'donut',
    'cake', 'chair', 'couch', 'potted plant', 'bed', 'dining table', 'toilet', 'tv', 'laptop', 'mouse', 'remote', 'keyboard',
    'cell phone', 'microwave', 'oven', 'toaster', 'sink', 'refrigerator', 'book', 'clock', 'vase', 'scissors', 'teddy bear',
    'hair drier', 'toothbrush')

COCO_CLASSES = tuple(sorted(COCO_CLASSES))      # the reference iterates data/coco/synonyms.py's table, whose keys are in alphabetical order

_WORD = re.compile(r"\w+|[^\w\s]")


def word_tokenize(text):
    """nltk.word_tokenize on class names: words and single punctuation marks"""
    return _WORD.findall(text)


def create_vocab_mask(model, classes=COCO_CLASSES, synonyms=None, use_syns=False):
    """compute_predictions.py:88-109 -> (tokens, float32 mask [V])"""
    mask = -10000.0 * np.ones([len(model.vocab)], dtype=np.float32)
    tokens = []
    for cls in classes:
        names = [cls]
        if use_syns and synonyms is not None:
            if cls not in synonyms:
                continue
            names = synonyms[cls]
        for name in names:
            for token in word_tokenize(name):
                if token in model.word_to_idx:
                    mask[model.word_to_idx[token]] = 0
                    tokens.append(token)
    for token in ('__stop__', '__pad__'):
        mask[model.word_to_idx[token]] = 0
        tokens.append(token)
    return tokens, mask


def create_phrase_set(model, classes=COCO_CLASSES, synonyms=None, use_syns=False):
    """the closed answer set of classification as whole phrases -> (phrases.PhraseSet, phrase_to_class): phrase i names
    classes[phrase_to_class[i]].  With synonyms (the table create_vocab_mask takes) several phrases map to one class and a class
    without an entry is left out, as in the mask.  Unlike the mask nothing is dropped silently: a word outside the model's
    vocabulary is a ValueError, and so is a name that two classes share."""
    from .phrases import PhraseSet
    texts, owner, seen = [], [], {}
    for ci, cls in enumerate(classes):
        names = [cls]
        if use_syns and synonyms is not None:
            if cls not in synonyms:
                continue
            names = synonyms[cls]
        for name in names:
            key = tuple(word_tokenize(name))
            if key in seen:
                if seen[key] != ci:
                    raise ValueError(f'create_phrase_set: {name!r} names both {classes[seen[key]]!r} and {cls!r}')
                continue
            seen[key] = ci
            texts.append(name)
            owner.append(ci)
    return PhraseSet.from_texts(model, texts), owner


class BoxesWriter:
    """one group per sample id: 'boxes' [Q,4] float32, 'relevance' [Q] float32"""

    def __init__(self, path_h5py):
        try:
            import h5py
            self.h5, self.path = h5py.File(path_h5py, 'w'), path_h5py
            self.arrays = None
        except ImportError:
            self.h5, self.path = None, os.path.splitext(path_h5py)[0] + '.npz'
            self.arrays = {}

    def add(self, sample_id, boxes, relevance):
        if self.h5 is not None:
            grp = self.h5.create_group(str(sample_id))
            grp.create_dataset('boxes', data=boxes)
            grp.create_dataset('relevance', data=relevance)
        else:
            self.arrays[f'{sample_id}/boxes'] = boxes
            self.arrays[f'{sample_id}/relevance'] = relevance

    def close(self):
        if self.h5 is not None:
            self.h5.close()
        else:
            np.savez(self.path, **self.arrays)
        return self.path


def boxes_to_h5py(npz_path, h5py_path):
    """the reference's boxes layout from the .npz fallback (needs h5py)"""
    import h5py
    z = np.load(npz_path)
    with h5py.File(h5py_path, 'w') as f:
        for sid in sorted({k.rsplit('/', 1)[0] for k in z.files}):
            grp = f.create_group(sid)
            grp.create_dataset('boxes', data=z[sid + '/boxes'])
            grp.create_dataset('relevance', data=z[sid + '/relevance'])


@torch.no_grad()
def make_predictions(model, batches, eval_dir, task, subset='val', data_split='original_split', num_eval_batches=None,
                     vocab_mask=None, beam_size=None, beam=None, answer_set=None, classes=COCO_CLASSES):
    """compute_predictions.py:30-85; returns (predictions dict, json path, boxes path).  beam_size / beam (added keys, as in
    inference.predict: beam.impl, beam.finished, beam.length_penalty, beam.no_repeat_ngram, beam.min_length,
    beam.repetition_penalty): answers by beam search instead of greedy decoding; a vocabulary
    mask then needs beam.impl = device (GPV.forward_beam_search).  answer_set (added): None / 'tokens' is the reference's flat
    vocabulary mask, unchanged; 'phrases' answers from the closed set of `classes` (create_phrase_set; GPV.forward_beam_search with
    phrases=, beam_size default 4): every answer written is one of the class names"""
    dev = model.vision_token.device
    if answer_set not in (None, 'tokens', 'phrases'):
        raise ValueError(f"make_predictions: answer_set must be 'tokens' or 'phrases', got {answer_set!r}")
    pset = owner = None
    if answer_set == 'phrases':
        if vocab_mask is not None:
            raise ValueError("make_predictions: answer_set='phrases' and vocab_mask exclude each other")
        pset, owner = create_phrase_set(model, classes)
    if vocab_mask is None and task == 'CocoClassification' and pset is None:
        vocab_mask = create_vocab_mask(model)[1]
    if vocab_mask is not None:
        vocab_mask = torch.as_tensor(vocab_mask, dtype=torch.float32, device=dev)
    os.makedirs(eval_dir, exist_ok=True)
    boxes_file = BoxesWriter(os.path.join(eval_dir, f'{task}_{subset}_boxes.h5py'))
    predictions = {}
    model.eval()
    for i, (imgs, queries, sample_ids) in enumerate(batches):
        if num_eval_batches is not None and i > num_eval_batches:
            break
        if not isinstance(imgs, NestedTensor):
            imgs = nested_tensor_from_tensor_list([x.to(dev) for x in imgs])
        chosen = None
        if pset is not None:
            outputs = model.forward_beam_search(imgs, queries, beam_size=beam_size or 4, phrases=pset,
                                                length_penalty=(beam or {}).get('length_penalty'))
            chosen = outputs['_beam_phrase'][:, 0].cpu().tolist()
        elif beam_size:
            outputs = model.forward_beam_search(imgs, queries, beam_size=beam_size, vocab_mask=vocab_mask, **beam_options(beam))
        else:
            outputs = model(imgs, queries, None, vocab_mask=vocab_mask)
        for j, (sid, d) in enumerate(zip(sample_ids, decode_outputs(outputs, model, num_output_boxes=None))):
            predictions[sid] = {'answer': d['answer'] if chosen is None else classes[owner[chosen[j]]]}
            boxes_file.add(sid, d['boxes'], d['relevance'])
    boxes_path = boxes_file.close()
    json_path = os.path.join(eval_dir, f'{task}_{data_split}_{subset}_predictions.json')
    with open(json_path, 'w') as f:
        json.dump(predictions, f, indent=4, sort_keys=True)            # utils/io.py dump_json_object
    return predictions, json_path, boxes_path
