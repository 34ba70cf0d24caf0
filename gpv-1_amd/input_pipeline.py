"""Device-side input pipeline: decoded uint8 images -> the stem's NHWC4 bf16 batch on the GPU.

Reference: datasets/coco_generic_dataset.py:49-62 (``resize(img, (imh, imw), anti_aliasing=True)``), datasets/coco_datasets.py
(:26-38 detection, :137-150 classification: ``ToPILImage -> RandomApply([ColorJitter(0.4, 0.4, 0.4, 0.1)], p=0.8) ->
[RandomHorizontalFlip] -> RandomGrayscale(p=0.2) -> ToTensor -> Normalize``; coco_generic_dataset.py:25-33, captioning and VQA on
the train subset: ``RandomApply([ColorJitter(0.2, 0.2, 0.2, 0.0)], p=0.8)``; every other subset: ToTensor -> Normalize only),
30 CPU worker processes (configs/exp/gpv.yaml:126).  ``DeviceImagePipeline(images, tasks)`` draws from the ``AUGMENT`` table below,
which knows the two box tasks only; the per-class, per-subset rules live in gpv1_amd.datasets, which passes a ``spec``.

Here the host only decodes (out of scope: JPEG) and draws the random parameters in torchvision's order; everything per pixel runs
in two HIP launches (csrc/image_pipeline.hip) and lands in the layout the fused stem kernel reads, so neither an fp32 NCHW batch
(118 MB per 32 images over PCIe) nor gpv_image_to_nhwc4 exists on this path:

    pipe = DeviceImagePipeline(size=(480, 640), train=True)
    samples = pipe(list_of_uint8_HWC_arrays, tasks)          # NestedTensor: .tensors = [B, H+6, Wp, 4] bf16, .mask [B, H, W] (all False)
    loss = trainer.train_step(samples, queries, targets)       # the backbone recognises the prepared stem input

Uploads go through pinned staging and are asynchronous; call it one batch ahead to hide the PCIe copy under the previous step.
"""
import ctypes as C
import math
import random

import numpy as np
import torch

from . import hip
from .misc import NestedTensor, upload_bytes
from .ops import RT

JITTER = (0.4, 0.4, 0.4, 0.1)            # brightness, contrast, saturation, hue  (coco_datasets.py:30,141)
AUGMENT = {'CocoDetection': ('jitter', 'gray'), 'CocoClassification': ('jitter', 'flip', 'gray')}


def draw_params(task, rng, train=True, spec=None):
    """the random decisions of the reference's transform for one sample, in torchvision's order of draws:
    RandomApply(p=0.8) -> ColorJitter.get_params (factors, then a random order of the steps) -> RandomHorizontalFlip(0.5)
    -> RandomGrayscale(0.2).  -> dict(jitter, order, brightness, contrast, saturation, hue, flip, gray)
    spec: None (the AUGMENT table's entry for `task`) or (jitter 4-tuple | None, flip, gray).  A jitter component of 0 draws nothing
    and contributes no step (torchvision 0.7's _check_input returns None for it), so `order` then has fewer than four entries."""
    p = {'jitter': 0, 'order': (0, 1, 2, 3), 'brightness': 1.0, 'contrast': 1.0, 'saturation': 1.0, 'hue': 0.0, 'flip': 0, 'gray': 0}
    if spec is None:
        aug = AUGMENT.get(task, ())
        spec = (JITTER if 'jitter' in aug else None, 'flip' in aug, 'gray' in aug)
    jitter, flip, gray = spec if train else (None, False, False)
    if jitter is not None and rng.random() < 0.8:
        p['jitter'] = 1
        order = []
        for step, (name, j) in enumerate(zip(('brightness', 'contrast', 'saturation', 'hue'), jitter)):
            if j:
                p[name] = rng.uniform(-j, j) if name == 'hue' else rng.uniform(max(0.0, 1 - j), 1 + j)
                order.append(step)
        rng.shuffle(order)
        p['order'] = tuple(order)
    if flip and rng.random() < 0.5:
        p['flip'] = 1
    if gray and rng.random() < 0.2:
        p['gray'] = 1
    return p


def stem_geometry(H, W):
    """padded NHWC4 extent the stem reads (backbone.ResNetBody.forward_nhwc)"""
    OW = (W + 6 - 7) // 2 + 1
    return H + 6, ((max(W + 6, 2 * (OW - 1) + 8) + 7) // 8) * 8


class DeviceImagePipeline:
    def __init__(self, size=(480, 640), train=True, seed=0, device='cuda'):
        self.size, self.train, self.rng, self.device = tuple(size), train, random.Random(seed), torch.device(device)
        self._scratch = {}

    def __call__(self, images, tasks=None, params=None, crops=None):
        """images: list of HxWx3 uint8 arrays / tensors (host or device); tasks: list[str] (which augmentation applies);
        params: optional list of draw_params() dicts (the datasets, tests) -- drawn here otherwise; `order` may have fewer than four
        entries; crops: optional list of None | (y1, y2, x1, x2) in source pixels: the sample is that window of its image (the
        classification crop) -- the kernel reads it in place through the descriptor's pitch: no copy, no extra launch"""
        B = len(images)
        H, W = self.size
        Hp, Wp = stem_geometry(H, W)
        dev = self.device
        if params is None:
            params = [draw_params(tasks[i] if tasks is not None else None, self.rng, self.train) for i in range(B)]
        if crops is None:
            crops = [None] * B
        if len(params) != B or len(crops) != B:
            raise ValueError('DeviceImagePipeline: one params entry and one crops entry per image')
        srcs, wins = [], []
        for i, (im, crop) in enumerate(zip(images, crops)):
            t = torch.as_tensor(im)
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError('DeviceImagePipeline: images must be HxWx3 uint8 (decode / grey->RGB on the host, as the reference does)')
            y1, y2, x1, x2 = (0, t.shape[0], 0, t.shape[1]) if crop is None else (int(v) for v in crop)
            if not (0 <= y1 < y2 <= t.shape[0] and 0 <= x1 < x2 <= t.shape[1]):
                raise ValueError(f'DeviceImagePipeline: window rows {y1}:{y2}, columns {x1}:{x2} of image {i} is empty or outside '
                                 f'its {t.shape[0]} x {t.shape[1]} image')
            if max((y2 - y1) / H, (x2 - x1) / W) > 9:
                raise ValueError('DeviceImagePipeline: more than 9x down-scaling is not supported')
            if not t.is_cuda:
                t = t.contiguous().pin_memory().to(dev, non_blocking=True)
            srcs.append(t.contiguous())
            wins.append((y1, y2, x1, x2))
        descs = (hip.ImageDesc * B)()
        for d, t, p, (y1, y2, x1, x2) in zip(descs, srcs, params, wins):
            d.src, d.H, d.W, d.pitch = t.data_ptr() + (y1 * t.shape[1] + x1) * 3, y2 - y1, x2 - x1, t.shape[1]
            if not (d.pitch == 0 or d.pitch >= d.W):         # (gpv_image_pipeline sees the descriptors in device memory only)
                raise ValueError('DeviceImagePipeline: pitch must be 0 or at least the window width')
            d.flip, d.gray, d.jitter = int(p['flip']), int(p['gray']), int(p['jitter'])
            order = [int(o) for o in p['order']]
            if len(order) > 4 or any(o > 3 for o in order):
                raise ValueError(f"DeviceImagePipeline: order {p['order']!r} is not a list of at most four steps 0..3")
            d.order[:] = order + [-1] * (4 - len(order))      # a negative entry is "no step"
            d.brightness, d.contrast, d.saturation, d.hue = p['brightness'], p['contrast'], p['saturation'], p['hue']
        raw = upload_bytes(bytes(descs), dev)
        key = (B, H, W)
        sc = self._scratch.get(key)
        if sc is None:
            sc = self._scratch[key] = (torch.empty(B * H * W * 3, dtype=torch.uint8, device=dev), torch.zeros(B, device=dev))
        out = torch.empty(B, Hp, Wp, 4, device=dev, dtype=RT.dtype)
        hip.image_pipeline(raw, B, sc[0], sc[1], out, H, W, 3, Hp, Wp)
        self._keep = (srcs, raw)                       # the sources must outlive the asynchronous launches
        mask = torch.zeros(B, H, W, dtype=torch.bool, device=dev)
        return NestedTensor(out, mask, True)
