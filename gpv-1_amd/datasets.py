"""Train from COCO sample files: the reference's datasets restated as one reader + a table of per-class rules, and a loader that
feeds the device input pipeline one batch ahead.

Reference: datasets/coco_generic_dataset.py (GenericCocoDataset), datasets/coco_datasets.py (CocoCaptioning, CocoDetection, CocoVqa,
CocoClassification, RefCocop), datasets/coco_multitask_dataset.py (CocoMultitaskDataset), configs/task/coco_learning_tasks.yaml.
Left out: CocoVqaTestOriginalSplitDataset and CocoCapTestOriginalSplitDataset (the test-server splits), and everything that WRITES
the sample files (downloading / preprocessing COCO, vocabulary building: DESIGN §7).

A sample file is a JSON list of dicts: ``image.subset`` / ``image.image_id`` (-> ``{image_dir}/{subset}/COCO_{subset}_{id:012d}.jpg``),
``query``, ``answer`` (captioning, classification, VQA), ``all_answers`` {answer: count} (VQA), ``boxes`` (a list of [x, y, w, h]:
detection, RefCOCO+; ONE [x, y, w, h]: classification).  Every other key stays untouched in ``ds.samples`` for the evaluators.

    ds = CocoMultitaskDataset(cfg.learning_datasets, cfg.task_configs, 'train')
    loader = DeviceLoader(ds, batch_size=32, device='cuda', size=(480, 640), threads=8)
    for samples, queries, targets in loader.batches(shard_indices(len(ds), epoch, rank, world), epoch):
        loss = trainer.train_step(samples, queries, targets)

What differs from the reference's DataLoader: the image never exists as fp32 on the host.  The host reads the file and walks its
Huffman stream (DeviceJpegDecoder.parse); inverse DCT, the classification crop (a window descriptor, no copy), resize, colour
jitter, flip, grey and normalisation run on the device (csrc/jpeg.hip, csrc/image_pipeline.hip).  Random decisions are drawn per
sample from ``random.Random(sample_seed(seed, epoch, index))`` in torchvision's order of draws, so a sample's augmentation and VQA
answer do not depend on batch composition, world size, prefetch depth or a resume.
"""
import bisect
import json
import os
import random
import weakref
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import torch

from .input_pipeline import JITTER, draw_params

GENERIC_JITTER = (0.2, 0.2, 0.2, 0.0)              # coco_generic_dataset.py:29
NO_TRANSFORM = (None, False, False)

# class -> (is this subset a training subset?, (jitter, flip, gray) on a training subset, classification crop?, VQA answer choice?)
# coco_generic_dataset.py:25-33, coco_datasets.py:29-38 (detection), :140-150 (classification), :202-211 (RefCOCO+: 'train' in subset)
RULES = {
    'CocoCaptioning': (lambda s: s == 'train', (GENERIC_JITTER, False, False), False, False),
    'CocoVqa': (lambda s: s == 'train', (GENERIC_JITTER, False, False), False, True),
    'CocoDetection': (lambda s: s == 'train', (JITTER, False, True), False, False),
    'CocoClassification': (lambda s: s == 'train', (JITTER, True, True), True, False),
    'RefCocop': (lambda s: 'train' in s, (JITTER, False, True), False, False),
}


def transform_spec(task, subset):
    """(jitter 4-tuple | None, flip, gray) of the reference's transform for this class on this subset"""
    is_train, spec, _, _ = RULES[task]
    return spec if is_train(subset) else NO_TRANSFORM


def sample_seed(seed, epoch, index):
    """seed of a sample's own random.Random: a fixed function of (dataset seed, epoch, index in the dataset the loader iterates)"""
    return (int(seed) * 1000003 + int(epoch)) * 1000003 + int(index)


def crop_window(x, y, w, h, H, W):
    """CocoClassification.read_image (coco_datasets.py:163-172): the box grown by 20 % on every side, at least 5 pixels wide and
    high before growing, truncated toward zero, clamped to the H x W image -> (y1, y2, x1, x2).  The reference would fail inside
    resize() on an empty window; here it is a ValueError."""
    w, h = max(w, 5), max(h, 5)
    x1, x2 = (min(max(0, int(z)), W) for z in (x - 0.2 * w, x + 1.2 * w))
    y1, y2 = (min(max(0, int(z)), H) for z in (y - 0.2 * h, y + 1.2 * h))
    if y2 <= y1 or x2 <= x1:
        raise ValueError(f'crop_window: box ({x}, {y}, {w}, {h}) leaves an empty window (rows {y1}:{y2}, columns {x1}:{x2}) of a {H} x {W} image')
    return y1, y2, x1, x2


def box_targets(boxes, H, W):
    """GenericCocoDataset.get_boxes('cxcywh') + normalize_bbox (coco_generic_dataset.py:64-83): [x + w/2, y + h/2, w, h] as float32,
    divided by (W, H, W, H) of the ORIGINAL image in float32 -> (boxes [n, 4] float32, labels [n] long zeros)"""
    b = torch.tensor([[x + 0.5 * w, y + 0.5 * h, w, h] for x, y, w, h in boxes], dtype=torch.float64).reshape(-1, 4).to(torch.float32)
    b = b / torch.tensor([W, H, W, H], dtype=torch.float32)
    return b, torch.zeros(b.shape[0], dtype=torch.long)


def vqa_answer(sample, rng):
    """CocoVqa.__getitem__ (coco_datasets.py:60-68): every answer given more than twice, repeated by its count; a random one of
    those, or `answer` when there is none"""
    pool = []
    for answer, freq in sample['all_answers'].items():
        if freq > 2:
            pool.extend([answer] * freq)
    return rng.choice(pool) if pool else sample['answer']


class CocoDataset:
    """one task's samples of one subset (the reference's GenericCocoDataset and its five subclasses: `task` selects the row of RULES).
    cfg: the task's subtree of task_configs (image_dir, image_size, read_image, samples, max_samples)."""
    task = None

    def __init__(self, cfg, subset, task=None, seed=0):
        self.task = task or self.task
        if self.task not in RULES:
            raise ValueError(f'CocoDataset: unknown task {self.task!r} (have {sorted(RULES)})')
        if cfg['read_image'] is not True:
            raise NotImplementedError(f'{self.task}: read_image: False (queries and targets without images) is not supported')
        self.cfg, self.subset, self.seed = cfg, subset, seed
        path = cfg['samples'][subset]
        if not os.path.isfile(str(path)):
            raise FileNotFoundError(f'{self.task}: no sample file {path} for subset {subset!r}')
        self.image_dir = str(cfg['image_dir'])
        if not os.path.isdir(self.image_dir):
            raise FileNotFoundError(f'{self.task}: no image directory {self.image_dir}')
        with open(path) as f:
            self.samples = json.load(f)
        self.size = (int(cfg['image_size']['H']), int(cfg['image_size']['W']))
        self.spec = transform_spec(self.task, subset)
        self.crop, self.vqa = RULES[self.task][2], RULES[self.task][3]

    def __len__(self):
        limit = (self.cfg.get('max_samples', None) or {}).get(self.subset, None)
        return len(self.samples) if limit is None else min(len(self.samples), int(limit))

    def locate(self, i):
        return self, i

    def image_path(self, i):
        im = self.samples[i]['image']
        return os.path.join(self.image_dir, im['subset'], f"COCO_{im['subset']}_{int(im['image_id']):012d}.jpg")

    def draw(self, i, rng, H, W):
        """the sample's random decisions and its target, given the H x W of its decoded image (from the JPEG header).
        -> (draw_params dict, crop (y1, y2, x1, x2) | None, query, target dict with host tensors).  Order of draws: the image
        transform's (draw_params), then the VQA answer."""
        s = self.samples[i]
        params = draw_params(self.task, rng, True, self.spec)
        crop = None
        if self.crop:
            try:
                crop = crop_window(*s['boxes'], H, W)
            except ValueError as e:
                raise ValueError(f'{self.task} sample {i} ({self.image_path(i)}): {e}') from None
        target = {}
        if self.vqa:
            target['answer'] = vqa_answer(s, rng)
        elif self.crop:
            target['answer'] = s['answer']
        else:
            if 'boxes' in s:
                target['boxes'], target['labels'] = box_targets(s['boxes'], H, W)
            if 'answer' in s:
                target['answer'] = s['answer']
        target['task'] = self.task
        return params, crop, s['query'], target


def _named(task_name):
    return type(task_name, (CocoDataset,), {'task': task_name, '__doc__': f'CocoDataset with the {task_name} row of RULES'})


CocoCaptioning, CocoVqa, CocoDetection, CocoClassification, RefCocop = (_named(t) for t in RULES)
DATASETS = {c.task: c for c in (CocoCaptioning, CocoVqa, CocoDetection, CocoClassification, RefCocop)}


class CocoMultitaskDataset:
    """coco_multitask_dataset.py:9-42: the datasets of `learning_datasets` ({class name: {task_config, name}}) concatenated in the
    mapping's order; datasets[name], dataset_names, locate(i) -> (dataset, local index)"""

    def __init__(self, learning_datasets, task_configs, subset, seed=0):
        self.datasets, self.sample_l, self.sample_u, self.subset, self.seed = {}, [], [], subset, seed
        for dataset_cls, info in learning_datasets.items():
            if dataset_cls not in DATASETS:
                raise ValueError(f'CocoMultitaskDataset: unknown dataset class {dataset_cls!r} (have {sorted(DATASETS)})')
            ds = self.datasets[info['name']] = DATASETS[dataset_cls](task_configs[info['task_config']], subset)
            lo = self.sample_u[-1] if self.sample_u else 0
            self.sample_l.append(lo)
            self.sample_u.append(lo + len(ds))
        self.dataset_names = list(self.datasets.keys())
        sizes = {ds.size for ds in self.datasets.values()}
        if len(sizes) > 1:
            raise ValueError(f'CocoMultitaskDataset: the tasks disagree on image_size: {sorted(sizes)}')
        self.size = sizes.pop() if sizes else None

    def __len__(self):
        return self.sample_u[-1] if self.sample_u else 0

    def locate(self, i):
        if not 0 <= i < len(self):
            raise IndexError(i)
        k = bisect.bisect_right(self.sample_u, i)
        return self.datasets[self.dataset_names[k]], i - self.sample_l[k]


class HostBatch:
    """what the host half leaves for the device half: the parsed JPEG coefficients and, per sample, the drawn parameters, the
    crop window, the query and the target (host tensors)"""

    def __init__(self, indices, paths, parsed, params, crops, queries, targets):
        self.indices, self.paths, self.parsed, self.params, self.crops, self.queries, self.targets = \
            indices, paths, parsed, params, crops, queries, targets


def _read(path):
    with open(path, 'rb') as f:
        return f.read()


class DeviceLoader:
    """batches of (NestedTensor in the prepared stem layout, query strings, target dicts with device tensors) from a CocoDataset /
    CocoMultitaskDataset -- what FlatTrainer.train_step and the metric functions accept.

    While the caller works on batch n, one worker thread prepares batch n + 1: file reads and DeviceJpegDecoder.parse on the pool,
    the per-sample draws and crops.  THE WORKER MAKES NO HIP CALL: the trainer captures hipGraphs in the default capture mode, where
    an allocating or synchronising call from any thread invalidates an open capture.  So the main thread owns the pinned slots and
    lends the worker one that is already allocated and idle; a batch that does not fit comes back in pageable memory and the main
    thread grows the slot.  Upload, decode and image pipeline of batch n + 1 are issued (asynchronously) by the main thread when
    the caller asks for that batch.  prefetch=0 is the same code without the thread.  device=None: the host half only (host_batches)."""

    def __init__(self, dataset, batch_size, device='cuda', size=None, threads=8, prefetch=1, entropy='host', subseq_bits=1024):
        """entropy / subseq_bits: DeviceJpegDecoder's -- 'device' moves the Huffman walk to the GPU; the worker's half (gpv_huff_prepare)
        still makes no HIP call"""
        from .jpeg import DeviceJpegDecoder
        self.dataset, self.batch_size, self.prefetch, self.threads = dataset, int(batch_size), int(prefetch), int(threads)
        self.device = None if device is None else torch.device(device)
        self.size = tuple(size) if size is not None else dataset.size
        self.dec = DeviceJpegDecoder(device=self.device if self.device is not None else 'cpu', threads=self.threads, entropy=entropy,
                                     subseq_bits=subseq_bits)
        self.pipe = None
        # pinned coefficient slots: [buffer | None, event of its last upload | None]; one per batch in flight + the one in use
        self._slots, self._turn = [[None, None] for _ in range(self.prefetch + 2)], 0
        self._live = weakref.WeakSet()
        dataset.loader = self

    # ---- host half (any thread; no HIP call) ----
    def _prepare(self, indices, epoch, lend=None):
        ds = self.dataset
        where = [ds.locate(i) for i in indices]
        paths = [d.image_path(k) for d, k in where]
        pool = self.dec.pool
        files = list(pool.map(_read, paths)) if pool is not None else [_read(p) for p in paths]
        try:
            parsed = self.dec.parse(files, into=None if lend is None else lend[0])
        except Exception:
            for path, f in zip(paths, files):                 # name the file the decoder refuses
                try:
                    self.dec.parse([f])
                except Exception as e:
                    raise type(e)(f'{path}: {e}') from None
            raise
        params, crops, queries, targets = [], [], [], []
        for i, (d, k), inf in zip(indices, where, parsed.infos):
            rng = random.Random(sample_seed(getattr(ds, 'seed', 0), epoch, i))
            p, c, q, t = d.draw(k, rng, inf.height, inf.width)
            params.append(p); crops.append(c); queries.append(q); targets.append(t)
        hb = HostBatch(list(indices), paths, parsed, params, crops, queries, targets)
        hb.slot = lend
        return hb

    def _lend(self):
        """main thread: the next pinned slot, idle (its last upload has finished), or None when it was never allocated"""
        if self.device is None or self.device.type != 'cuda':
            return None
        slot = self._slots[self._turn]
        self._turn = (self._turn + 1) % len(self._slots)
        if slot[1] is not None:
            slot[1].synchronize()
        return (slot[0], slot)

    def host_batches(self, index_batches, epoch=0):
        """HostBatch per index list, in order, prepared `prefetch` batches ahead on one worker thread"""
        gen = self._host_batches(index_batches, epoch)
        self._live.add(gen)
        return gen

    def _host_batches(self, index_batches, epoch):
        it = iter(index_batches)
        if self.prefetch <= 0:
            for ib in it:
                yield self._prepare(ib, epoch, self._lend())
            return
        worker = ThreadPoolExecutor(max_workers=1, thread_name_prefix='gpv-loader')
        pending = deque()
        try:
            for _ in range(self.prefetch):
                ib = next(it, None)
                if ib is not None:
                    pending.append(worker.submit(self._prepare, ib, epoch, self._lend()))
            while pending:
                hb = pending.popleft().result()               # a worker exception surfaces here, at the caller's next()
                ib = next(it, None)
                if ib is not None:
                    pending.append(worker.submit(self._prepare, ib, epoch, self._lend()))
                yield hb
        finally:                                              # exhausted, abandoned (close / garbage collection) or failed
            for f in pending:
                f.cancel()
            worker.shutdown(wait=True)

    # ---- device half (main thread) ----
    def _issue(self, hb):
        from .input_pipeline import DeviceImagePipeline
        from .misc import STAGER
        dev = self.device
        if self.pipe is None:
            self.pipe = DeviceImagePipeline(size=self.size, train=True, device=dev)
        parsed, lend = hb.parsed, hb.slot
        slot = lend[1] if lend is not None else self._slots[0]
        if not parsed.lent:                                   # did not fit (or nothing to lend yet): grow the slot, stage here
            n = parsed.coefs.numel()
            if slot[1] is not None:
                slot[1].synchronize()
            if slot[0] is None or slot[0].numel() < n:
                slot[0] = torch.empty(max(n + n // 4, 1 << 20), dtype=torch.int16).pin_memory()
            slot[0][:n].copy_(parsed.coefs)
            parsed.coefs, parsed.lent = slot[0][:n], True
        slot[1] = torch.cuda.Event()
        images = self.dec.issue(parsed, event=slot[1])
        samples = self.pipe(images, params=hb.params, crops=hb.crops)
        # targets: every box of the batch in one staged upload, views per sample
        counts = [t['boxes'].shape[0] if 'boxes' in t else 0 for t in hb.targets]
        if sum(counts):
            boxes = STAGER.to_device(torch.cat([t['boxes'] for t in hb.targets if 'boxes' in t]), torch.float32, dev)
            labels = torch.zeros(sum(counts), dtype=torch.long, device=dev)
        targets, at = [], 0
        for t, n in zip(hb.targets, counts):
            t = dict(t)
            if 'boxes' in t:
                t['boxes'], t['labels'] = boxes[at:at + n], labels[at:at + n]
                at += n
            targets.append(t)
        return samples, list(hb.queries), targets

    def batches(self, indices, epoch=0, batch_size=None):
        """full batches only, like train_distr.batches"""
        bs = int(batch_size or self.batch_size)
        return self._device_batches([list(indices[s:s + bs]) for s in range(0, len(indices) - bs + 1, bs)], epoch)

    def eval_batches(self, batch_size=None):
        """in order, the last batch may be short (train_distr.py:336-341 of the reference: shuffle=False)"""
        bs, n = int(batch_size or self.batch_size), len(self.dataset)
        return self._device_batches([list(range(s, min(n, s + bs))) for s in range(0, n, bs)], 0)

    def _device_batches(self, groups, epoch):
        inner = self.host_batches(groups, epoch)
        try:
            for hb in inner:
                yield self._issue(hb)
        finally:
            inner.close()                                     # abandoned mid-epoch: the worker is joined here

    def close(self):
        """join the worker of every iterator still alive (abandoned mid-epoch) and the parse pool's threads"""
        for gen in list(self._live):
            gen.close()
        if self.dec.pool is not None:
            self.dec.pool.shutdown(wait=True)
            self.dec.pool = ThreadPoolExecutor(max_workers=self.threads)      # (threads start on first use)
