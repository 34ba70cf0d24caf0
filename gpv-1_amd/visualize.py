"""Training visualisations (reference: ``visualize`` of exp/gpv/train_distr.py:40-133, called at :454-460): for the first
``training.num_vis_samples`` samples of a subset, the picture exactly as the model saw it with the top-5 predicted boxes and the
ground-truth boxes drawn, one JPEG file per sample, and an ``index.html`` with the query, the picture, the predicted answer, the
ground-truth answer and the relevance scores.

The pictures never leave the device as pixels: the batch the model consumed (the stem's padded NHWC4 batch of the device loader, or a
normalised NCHW batch, which ``gpv_image_to_nhwc4`` brings into that layout) is denormalised, overlaid with the box outlines and
encoded by ``DeviceJpegEncoder.encode_batch`` (csrc/jpeg_enc.hip), and what comes back is each sample's encoded file.  Deviations
from the reference: JPEG instead of PNG, the denormalised value is rounded instead of truncated, and
``vis_bbox``'s outline is our own statement of it (scikit-image's ``polygon_perimeter`` of an axis-aligned rectangle).
"""
import html
import os

import numpy as np
import torch

from . import jpeg_encode
from .inference import IMAGENET_MEAN, IMAGENET_STD
from .misc import NestedTensor, nested_tensor_from_tensor_list

RED, GREEN, BLUE = (255, 0, 0), (0, 255, 0), (0, 0, 255)
COLUMNS = ('query', 'detection', 'pred_answer', 'gt_answer', 'relevance_scores')
TOP_K = 5
PAD = jpeg_encode.DeviceJpegEncoder.PAD


def write_index(path, rows):
    """the reference's HtmlWriter, reduced to what visualize needs: a table with one header row and one row per sample; a
    `detection` cell is an image tag, every other cell is escaped text"""
    with open(path, 'w') as f:
        f.write('<!DOCTYPE html>\n<html>\n<body>\n<table border="1" style="table-layout: fixed;">\n')
        f.write('<tr>' + ''.join(f'<td>{html.escape(c)}</td>' for c in COLUMNS) + '</tr>\n')
        for row in rows:
            cells = [f'<img src="{html.escape(v, quote=True)}" height="224">' if c == 'detection' else html.escape(str(v)) for c, v in zip(COLUMNS, row)]
            f.write('<tr>' + ''.join(f'<td>{c}</td>' for c in cells) + '</tr>\n')
        f.write('</table>\n</body>\n</html>\n')


def box_lists(pred_boxes, order, gt_boxes):
    """the boxes of one sample in drawing order with their colours: of the top-5 predictions the first min(n_gt, 5) are red and the
    rest blue -- the blue ones are drawn first, as the reference draws them --, then the ground truth in green, last.
    pred_boxes [Q, 4], order = the top-5 indices, gt_boxes [n_gt, 4] or None; tensors stay on their device."""
    n_gt = 0 if gt_boxes is None else int(gt_boxes.shape[0])
    top = pred_boxes[order].float()
    k = min(n_gt, TOP_K)
    parts, colours = [top[k:], top[:k]], [BLUE] * (TOP_K - k) + [RED] * k
    if n_gt:
        room = jpeg_encode.MAX_BOXES - TOP_K                  # (more ground-truth boxes than the encoder overlays: the first ones)
        parts.append(gt_boxes[:room].float().to(top.device))
        colours += [GREEN] * min(n_gt, room)
    return torch.cat(parts), colours


def label_lists(scores, n_gt):
    """the labels of one sample's boxes in the drawing order of box_lists: every predicted box carries its relevance score, two
    decimals, above it, every ground-truth box `GT` below it (the reference's vis.add_box).  scores = the top-5 values, best first."""
    k = min(n_gt, TOP_K)
    order = list(range(k, TOP_K)) + list(range(k))
    return [f'{float(scores[i]):.2f}' for i in order] + [('GT', 'below')] * min(n_gt, jpeg_encode.MAX_BOXES - TOP_K)


def stem_layout(nested):
    """the batch in the stem's padded NHWC4 layout: the device loader's batches are in it already"""
    x = nested.tensors
    if x.dim() == 4 and x.shape[-1] == 4 and x.shape[1] != 3:
        return nested
    from . import hip
    from .input_pipeline import stem_geometry
    B, _, H, W = x.shape
    Hp, Wp = stem_geometry(H, W)
    out = torch.empty(B, Hp, Wp, 4, device=x.device, dtype=torch.float32)
    hip.image_to_nhwc4(x.float().contiguous(), out, B, H, W, PAD, Hp, Wp)
    return NestedTensor(out, torch.zeros(B, H, W, dtype=torch.bool, device=x.device), True)


def _host_pictures(nested, count):
    """what the host hook encodes: uint8 [H, W, 3] pictures by the host statement of the denormalise rule"""
    x = nested.tensors
    if x.dim() == 4 and x.shape[-1] == 4 and x.shape[1] != 3:
        H, W = nested.mask.shape[1:]
        x = x[:count, PAD:PAD + H, PAD:PAD + W, :3]
    else:
        x = x[:count].permute(0, 2, 3, 1)
    return [jpeg_encode.denormalise_host(p.detach().cpu(), IMAGENET_MEAN, IMAGENET_STD) for p in x]


@torch.no_grad()
def visualize(model, batches, cfg, step, subset, encoder=None, labels=False):
    """batches: an iterable of (images, queries, targets) as the evaluators read them.  encoder: None = a DeviceJpegEncoder on the
    model's device (quality 90, 4:2:0); or a callable picture -> bytes (uint8 [H, W, 3] array in, e.g. jpeg_encode.encode_host), for
    which the pictures are built on the host by denormalise_host, draw_boxes_host and draw_labels_host.  labels: every predicted
    box carries its relevance score above it and every ground-truth box `GT` below it (label_lists); with either encoder.  Leaves
    the model in the mode it was in.
    -> the directory written"""
    dev = model.vision_token.device
    vis_dir = os.path.join(cfg.exp_dir, 'training_visualizations', f'{subset}_{step:06d}')
    os.makedirs(vis_dir, exist_ok=True)
    limit = int(cfg.training.num_vis_samples)
    if encoder is None:
        encoder = jpeg_encode.DeviceJpegEncoder(quality=90, subsampling='4:2:0', device=dev)
    rows, count = [], 0
    was_training = model.training
    model.eval()
    try:
        for imgs, queries, targets in batches:
            if count >= limit:
                break
            nested = imgs if isinstance(imgs, NestedTensor) else nested_tensor_from_tensor_list([x.to(dev) for x in imgs])
            gt_answers, _ = model.encode_answers(targets)
            outputs = model(nested, queries, None)
            prob = outputs['pred_relevance_logits'].float().softmax(-1)[..., 0]
            top = torch.topk(prob, k=TOP_K, dim=1)
            top1 = torch.topk(outputs['answer_logits'][-1].float(), k=1, dim=-1).indices[..., 0].detach().cpu().numpy()
            pred_answers = model.token_ids_to_words(top1)
            take = min(prob.shape[0], limit - count)
            boxes, colours = zip(*[box_lists(outputs['pred_boxes'][b], top.indices[b], targets[b].get('boxes')) for b in range(take)])
            values = top.values.detach().cpu().numpy()         # for index.html, and for the labels: one copy serves both
            n_gt = [0 if targets[b].get('boxes') is None else int(targets[b]['boxes'].shape[0]) for b in range(take)]
            tags = [label_lists(values[b], n_gt[b]) for b in range(take)] if labels else None
            if hasattr(encoder, 'encode_batch'):
                files = encoder.encode_batch(stem_layout(nested), IMAGENET_MEAN, IMAGENET_STD, boxes=list(boxes), colours=list(colours), count=take,
                                             **({'labels': tags} if labels else {}))
            else:
                files = []
                for i, (p, b, c) in enumerate(zip(_host_pictures(nested, take), boxes, colours)):
                    p = jpeg_encode.draw_boxes_host(p, b.cpu().numpy(), c)
                    files.append(encoder(jpeg_encode.draw_labels_host(p, b.cpu().numpy(), c, tags[i]) if labels else p))
            texts = queries if isinstance(queries, (list, tuple)) and all(isinstance(q, str) for q in queries) else None   # else (ids, mask)
            for b in range(take):
                name = f'{step:06d}_{count + b:04d}.jpg'
                with open(os.path.join(vis_dir, name), 'wb') as f:
                    f.write(files[b])
                rows.append((texts[b] if texts is not None else '', name, ' '.join(pred_answers[b]), ' '.join(gt_answers[b]), np.round(values[b], 4)))
            count += take
    finally:
        model.train(was_training)
    write_index(os.path.join(vis_dir, 'index.html'), rows)
    return vis_dir
