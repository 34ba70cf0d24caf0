"""Host-side criterion: box algebra, Hungarian matcher, DETR set criterion and the task-filtered GPV
criterion.  north_star keeps these on the host ("Hungarian matching and set_criterion kept on
host"): they are small fp32 torch ops on (B,100,{2,4}) tensors plus scipy's LSAP; the only heavy
piece, the vocabulary cross-entropy, is the HIP kernel (ops.softmax_ce).

Reference: utils/box_ops.py, utils/matcher.py, utils/set_criterion.py, exp/gpv/models/losses.py.
"""
import os

import numpy as np
import torch
import torch.nn as nn
from scipy.optimize import linear_sum_assignment

from . import ops


# ---------------------------------------------------------------- box_ops.py:9-59
def box_cxcywh_to_xyxy(x):
    cx, cy, w, h = x.unbind(-1)
    return torch.stack((cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h), dim=-1)


def box_xyxy_to_cxcywh(x):
    x0, y0, x1, y1 = x.unbind(-1)
    return torch.stack(((x0 + x1) / 2, (y0 + y1) / 2, x1 - x0, y1 - y0), dim=-1)


def box_area(b):
    return (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])


def box_iou(b1, b2):
    a1, a2 = box_area(b1), box_area(b2)
    lt = torch.max(b1[:, None, :2], b2[:, :2])
    rb = torch.min(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    union = a1[:, None] + a2 - inter
    return inter / union, union


def generalized_box_iou(b1, b2):
    """pairwise (N,M) GIoU of xyxy boxes; degenerate boxes assert like box_ops.py:49-50."""
    assert (b1[:, 2:] >= b1[:, :2]).all()
    assert (b2[:, 2:] >= b2[:, :2]).all()
    iou, union = box_iou(b1, b2)
    lt = torch.min(b1[:, None, :2], b2[:, :2])
    rb = torch.max(b1[:, None, 2:], b2[:, 2:])
    wh = (rb - lt).clamp(min=0)
    area = wh[:, :, 0] * wh[:, :, 1]
    return iou - (area - union) / area



# ---------------------------------------------------------------- the matching rule, stated once on the host
def lsap_host(cost):
    """Linear sum assignment of one cost matrix, the rule csrc/set_match.hip runs on the device: scipy.optimize.linear_sum_assignment
    restated (shortest augmenting paths with dual variables u, v; plain numpy, float64), ties included.
      * more rows than columns: the transposed matrix is solved and the result is sorted by row;
      * every path search starts with ``remaining`` = the columns in REVERSE order (nc-1 ... 0), all path costs +inf, minVal 0;
      * one step of a search, for the current row i: first EVERY remaining column j gets r = minVal + c[i][j] - u[i] - v[j] (float64,
        in that order) and keeps it when r < its path cost (then path[j] = i); then ONE column is picked among those at the minimum
        path cost: the one at the LAST position of ``remaining`` that is unassigned, or, when none of them is unassigned, the one at
        the FIRST position.  It leaves ``remaining`` by ``remaining[index] = remaining[--num_remaining]``.  An unassigned pick ends the
        search (the sink); an assigned one makes its row the current row;
      * then u[cur] += minVal, u[i] += minVal - pathcost[col4row[i]] for every other visited row, v[j] -= minVal - pathcost[j] for
        every visited column, and the path is flipped from the sink back to the row the search started from.
    "Update all, then pick" is what scipy's serial scan computes, so the update may run in parallel.
    NaN or -inf in the cost raises ValueError (scipy does); a search that finds only +inf raises too.  -> (row_idx, col_idx) int64"""
    c = np.asarray(cost, dtype=np.float64)
    if c.ndim != 2:
        raise ValueError(f'lsap_host: expected a matrix, got {c.ndim} dimensions')
    if np.isnan(c).any() or np.isneginf(c).any():
        raise ValueError('lsap_host: the cost matrix contains invalid numeric entries')
    transpose = c.shape[1] < c.shape[0]
    if transpose:
        c = c.T
    nr, nc = c.shape
    if nr == 0 or nc == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    u, v = np.zeros(nr), np.zeros(nc)
    path = np.full(nc, -1, np.int64)
    col4row, row4col = np.full(nr, -1, np.int64), np.full(nc, -1, np.int64)
    for cur in range(nr):
        remaining = np.arange(nc - 1, -1, -1)
        num_remaining = nc
        spc = np.full(nc, np.inf)
        SR, SC = np.zeros(nr, bool), np.zeros(nc, bool)
        min_val, i, sink = 0.0, cur, -1
        while sink == -1:
            SR[i] = True
            js = remaining[:num_remaining]
            r = ((min_val + c[i, js]) - u[i]) - v[js]
            better = r < spc[js]
            path[js[better]] = i
            spc[js[better]] = r[better]
            vals = spc[js]
            min_val = vals.min()
            if min_val == np.inf:
                raise ValueError('lsap_host: the cost matrix is infeasible')
            at_min = np.flatnonzero(vals == min_val)
            free = at_min[row4col[js[at_min]] == -1]
            index = free[-1] if len(free) else at_min[0]
            j = js[index]
            if row4col[j] == -1:
                sink = j
            else:
                i = row4col[j]
            SC[j] = True
            num_remaining -= 1
            remaining[index] = remaining[num_remaining]
        u[cur] += min_val
        for r_ in np.flatnonzero(SR):
            if r_ != cur:
                u[r_] += min_val - spc[col4row[r_]]
        v[SC] -= min_val - spc[SC]
        j = sink
        while True:
            i = path[j]
            row4col[j] = i
            col4row[i], j = j, col4row[i]
            if i == cur:
                break
    if transpose:
        order = np.argsort(col4row, kind='stable')
        return col4row[order].astype(np.int64), order.astype(np.int64)
    return np.arange(nr, dtype=np.int64), col4row.astype(np.int64)


def match_cost_host(logits, boxes, tgt_boxes, labels, w_class, w_bbox, w_giou):
    """The matching cost of one image, the rule csrc/set_match.hip evaluates on the device: fp32, a FIXED order of operations, every
    product and sum rounded on its own (numpy float32 arrays do exactly that).  logits [Q,C+1], boxes [Q,4] and tgt_boxes [G,4]
    cxcywh, labels [G].
      p    = softmax(logits)[label]: e_k = exp(x_k - max_k x_k), summed in class order, p = e_label / sum
      l1   = ((|dcx| + |dcy|) + |dw|) + |dh|
      giou = from the corners (cx -+ 0.5 w, cy -+ 0.5 h), as generalized_box_iou orders it: union = (a1 + a2) - inter,
             iou = inter / union, area = enclosing box, giou = iou - (area - union) / area
      cost = (w_bbox * l1 + w_class * (-p)) + w_giou * (-giou)
    It is the same formula as HungarianMatcher.forward but not bit-equal to torch's cdist / softmax kernels, and is not meant to be:
    the device matcher has to agree with THIS statement.  -> [Q,G] float32"""
    f = np.float32
    x = np.asarray(logits, f)
    pb, tb = np.asarray(boxes, f), np.asarray(tgt_boxes, f)
    labels = np.asarray(labels, np.int64)
    e = np.exp(x - x.max(-1, keepdims=True))
    total = np.zeros(x.shape[0], f)
    for k in range(x.shape[1]):
        total = total + e[:, k]
    p = e[:, labels] / total[:, None]
    d = np.abs(pb[:, None, :] - tb[None, :, :])
    l1 = ((d[..., 0] + d[..., 1]) + d[..., 2]) + d[..., 3]
    half = f(0.5)

    def corners(b):
        return b[:, 0] - half * b[:, 2], b[:, 1] - half * b[:, 3], b[:, 0] + half * b[:, 2], b[:, 1] + half * b[:, 3]

    ax0, ay0, ax1, ay1 = (t[:, None] for t in corners(pb))
    bx0, by0, bx1, by1 = (t[None, :] for t in corners(tb))
    a1, a2 = (ax1 - ax0) * (ay1 - ay0), (bx1 - bx0) * (by1 - by0)
    zero = f(0)
    inter = np.maximum(np.minimum(ax1, bx1) - np.maximum(ax0, bx0), zero) * np.maximum(np.minimum(ay1, by1) - np.maximum(ay0, by0), zero)
    union = (a1 + a2) - inter
    iou = inter / union
    area = np.maximum(np.maximum(ax1, bx1) - np.minimum(ax0, bx0), zero) * np.maximum(np.maximum(ay1, by1) - np.minimum(ay0, by0), zero)
    giou = iou - (area - union) / area
    return ((f(w_bbox) * l1 + f(w_class) * (-p)) + f(w_giou) * (-giou)).astype(f)


# ---------------------------------------------------------------- matcher.py:32-77
class HungarianMatcher(nn.Module):
    def __init__(self, cost_class: float = 1, cost_bbox: float = 1, cost_giou: float = 1):
        super().__init__()
        assert cost_class != 0 or cost_bbox != 0 or cost_giou != 0, "all costs cant be 0"
        self.cost_class, self.cost_bbox, self.cost_giou = cost_class, cost_bbox, cost_giou

    @torch.no_grad()
    def forward(self, outputs, targets):
        logits = outputs['pred_relevance_logits'].float()
        bs, nq = logits.shape[:2]
        prob = logits.flatten(0, 1).softmax(-1)
        boxes = outputs['pred_boxes'].float().flatten(0, 1)
        tgt_ids = torch.cat([t['labels'] for t in targets])
        tgt_boxes = torch.cat([t['boxes'] for t in targets]).float()
        c_class = -prob[:, tgt_ids]
        c_bbox = torch.cdist(boxes, tgt_boxes, p=1)
        c_giou = -generalized_box_iou(box_cxcywh_to_xyxy(boxes), box_cxcywh_to_xyxy(tgt_boxes))
        cost = (self.cost_bbox * c_bbox + self.cost_class * c_class + self.cost_giou * c_giou).view(bs, nq, -1).cpu()
        sizes = [len(t['boxes']) for t in targets]
        out = []
        for i, c in enumerate(cost.split(sizes, -1)):
            r, cidx = linear_sum_assignment(c[i])
            out.append((torch.as_tensor(r, dtype=torch.int64), torch.as_tensor(cidx, dtype=torch.int64)))
        return out


# ---------------------------------------------------------------- set_criterion.py:44-97,150-191
class SetCriterion(nn.Module):
    def __init__(self, num_classes, matcher, weight_dict, eos_coef, losses):
        super().__init__()
        self.num_classes, self.matcher, self.weight_dict = num_classes, matcher, weight_dict
        self.eos_coef, self.losses = eos_coef, losses
        empty_weight = torch.ones(num_classes + 1)
        empty_weight[-1] = eos_coef
        self.register_buffer('empty_weight', empty_weight)

    @staticmethod
    def _src_idx(indices):
        batch_idx = torch.cat([torch.full_like(src, i) for i, (src, _) in enumerate(indices)])
        return batch_idx, torch.cat([src for src, _ in indices])

    def loss_labels(self, outputs, targets, indices, num_boxes):
        logits = outputs['pred_relevance_logits'].float()
        idx = self._src_idx(indices)
        dev = logits.device
        tgt_o = torch.cat([t['labels'][j.to(t['labels'].device)] for t, (_, j) in zip(targets, indices)]).to(dev)
        tgt = torch.full(logits.shape[:2], self.num_classes, dtype=torch.int64, device=dev)
        tgt[(idx[0].to(dev), idx[1].to(dev))] = tgt_o
        ew = self.empty_weight.to(dev)
        return {'loss_ce': nn.functional.cross_entropy(logits.transpose(1, 2), tgt, ew)}

    def loss_boxes(self, outputs, targets, indices, num_boxes):
        dev = outputs['pred_boxes'].device
        idx = self._src_idx(indices)
        src = outputs['pred_boxes'].float()[(idx[0].to(dev), idx[1].to(dev))]
        tgt = torch.cat([t['boxes'][i.to(t['boxes'].device)] for t, (_, i) in zip(targets, indices)], dim=0).float().to(dev)
        l1 = nn.functional.l1_loss(src, tgt, reduction='none').sum() / num_boxes
        giou = torch.diag(generalized_box_iou(box_cxcywh_to_xyxy(src), box_cxcywh_to_xyxy(tgt)))
        return {'loss_bbox': l1, 'loss_giou': (1 - giou).sum() / num_boxes}

    def forward(self, outputs, targets):
        base = {k: v for k, v in outputs.items() if k != 'aux_outputs'}
        indices = self.matcher(base, targets)
        # NOTE: local normalisation -- the cross-rank all_reduce of num_boxes is commented out in the
        # reference (set_criterion.py:165-168); reproduced as is.
        num_boxes = max(float(sum(len(t['labels']) for t in targets)), 1.0)
        fns = {'labels': self.loss_labels, 'boxes': self.loss_boxes}
        losses = {}
        for name in self.losses:
            losses.update(fns[name](outputs, targets, indices, num_boxes))
        if 'aux_outputs' in outputs:
            for i, aux in enumerate(outputs['aux_outputs']):
                ind = self.matcher(aux, targets)
                for name in self.losses:
                    losses.update({f'{k}_{i}': v for k, v in fns[name](aux, targets, ind, num_boxes).items()})
        self.last_indices = indices
        return losses


# ---------------------------------------------------------------- losses.py
class AnswerClassification(nn.Module):
    task = None
    key = 'loss_answer'

    def __init__(self, cfg):
        super().__init__()
        self.ignore_index = -100 if cfg.pad_idx is None else cfg.pad_idx

    def compute_ce_loss(self, logits, tgts):
        """logits (L,B',S,V) compute dtype; tgts list of (S,) int64.  losses.py:20-26:
        CE(reduction none) -> mean over batch, sum over positions and layers."""
        L, Bn, S, V = logits.shape
        t = torch.stack(tgts).to(logits.device)                           # (B',S)
        t = t.view(1, Bn, S).expand(L, Bn, S).reshape(-1)
        if self.ignore_index != -100:
            t = torch.where(t == self.ignore_index, torch.full_like(t, -100), t)
        rows = ops.softmax_ce(logits.reshape(L * Bn * S, V), t)          # HIP kernel, fp32 per-row loss
        return rows.view(L, Bn, S).mean(1).sum()

    def forward(self, outputs, targets):
        sel = [i for i, t in enumerate(targets) if 'answer' in t and (self.task is None or t['task'] == self.task)]
        if not sel:
            return {self.key: None}
        logits = outputs['answer_logits']
        if len(sel) != logits.shape[1]:                         # indexing with a host list = H2D copy + sync: only when a subset
            logits = logits[:, sel]
        return {self.key: self.compute_ce_loss(logits, [targets[i]['answer_token_ids'] for i in sel])}


class CaptionLoss(AnswerClassification):
    task, key = 'CocoCaptioning', 'loss_caption'


class VqaLoss(AnswerClassification):
    task, key = 'CocoVqa', 'loss_vqa'


class ClsLoss(AnswerClassification):
    task, key = 'CocoClassification', 'loss_cls'


class _DeviceIndices:
    """the main layer's matching of a device-matcher call, in SetCriterion.last_indices' format -- a list of (int64, int64) CPU
    pairs, one per localisation sample -- materialised when first read: that read is the device-to-host copy (the sync), and the place
    where the kernels' status words are checked"""

    def __init__(self, pred, tgt, n_pairs, status, sel):
        self._dev, self._sel, self._list = (pred, tgt, n_pairs, status), sel, None

    def _get(self):
        if self._list is None:
            from . import hip_match
            pred, tgt, n, status = (t.cpu() for t in self._dev)
            hip_match.check_status(status.tolist())
            self._list = [(pred[b, :int(n[b])].to(torch.int64), tgt[b, :int(n[b])].to(torch.int64)) for b in self._sel]
            self._dev = None
        return self._list

    def __iter__(self):
        return iter(self._get())

    def __len__(self):
        return len(self._sel)

    def __getitem__(self, i):
        return self._get()[i]


class Localization(nn.Module):
    """cfg.matcher (absent: 'host'; the environment variable GPV_MATCHER overrides it) chooses where box batches are matched:
    'host'   -- HungarianMatcher (cost on the device, .cpu(), scipy per image) + SetCriterion, the reference's path;
    'device' -- csrc/set_match.hip through ops.device_set_criterion: main and aux layers in one call, no host sync, fixed shapes."""

    def __init__(self, cfg):
        super().__init__()
        self.matcher = HungarianMatcher(cost_class=cfg.cost_wts.ce, cost_bbox=cfg.cost_wts.bbox,
                                        cost_giou=cfg.cost_wts.giou)
        self.set_criterion = SetCriterion(num_classes=cfg.num_classes, matcher=self.matcher, weight_dict=None,
                                          eos_coef=cfg.eos_coef, losses=['labels', 'boxes'])
        self.matcher_mode = os.environ.get('GPV_MATCHER') or cfg.get('matcher', 'host')     # device | host: where box batches are matched; overrides the loss config's `matcher` key
        if self.matcher_mode not in ('host', 'device'):
            raise ValueError(f"Localization: matcher must be 'host' or 'device', got {self.matcher_mode!r}")
        self.cost_wts = (float(cfg.cost_wts.ce), float(cfg.cost_wts.bbox), float(cfg.cost_wts.giou))

    def forward_device(self, outputs, targets, sel):
        """one ops.device_set_criterion call for the main and the aux layers.  Targets are padded to [B, Gmax]; g_count comes from the
        host-known lengths (-1: the sample has no 'boxes' key and takes no part), which is shape information and needs no sync."""
        from . import hip_match
        layers = [outputs] + list(outputs.get('aux_outputs', ()))
        logits = torch.stack([o['pred_relevance_logits'] for o in layers]).float()
        boxes = torch.stack([o['pred_boxes'] for o in layers]).float()
        if not logits.is_cuda:
            raise RuntimeError("gpv1_amd: matcher='device' needs the outputs on the GPU (no CPU fallback exists for the device matcher)")
        dev = logits.device
        B, Q = logits.shape[1], logits.shape[2]
        counts = [len(targets[i]['boxes']) if 'boxes' in targets[i] else -1 for i in range(B)]
        gmax = max(max(counts), 1)
        if not hip_match.supported(Q, gmax) or logits.shape[3] > hip_match.MAX_CLASSES:
            return None                                           # larger than the kernels take: the host path runs for this call
        rows = [b * gmax + k for b in sel for k in range(counts[b])]
        meta = torch.tensor(counts + rows, dtype=torch.int64).pin_memory().to(dev, non_blocking=True)
        g_count, rows = meta[:B].to(torch.int32), meta[B:]
        tgt_boxes = torch.zeros(B * gmax, 4, dtype=torch.float32, device=dev)
        tgt_labels = torch.zeros(B * gmax, dtype=torch.int32, device=dev)
        if rows.numel():
            tgt_boxes.index_copy_(0, rows, torch.cat([targets[b]['boxes'] for b in sel]).float().to(dev))
            tgt_labels.index_copy_(0, rows, torch.cat([targets[b]['labels'] for b in sel]).to(device=dev, dtype=torch.int32))
        ce, bbox, giou, pred, tgt, n_pairs, status = ops.device_set_criterion(
            logits, boxes, tgt_boxes.view(B, gmax, 4), tgt_labels.view(B, gmax), g_count, self.cost_wts, self.set_criterion.eos_coef)
        self.set_criterion.last_indices = _DeviceIndices(pred[:B], tgt[:B], n_pairs[:B], status, sel)
        return {'loss_ce': ce.sum(), 'loss_bbox': bbox.sum(), 'loss_giou': giou.sum()}

    def forward(self, outputs, targets):
        sel = [i for i, t in enumerate(targets) if 'boxes' in t]
        if not sel:
            return {'loss_ce': None, 'loss_bbox': None, 'loss_giou': None}
        if self.matcher_mode == 'device':
            ret = self.forward_device(outputs, targets, sel)
            if ret is not None:
                return ret
        fo = {'pred_relevance_logits': outputs['pred_relevance_logits'][sel], 'pred_boxes': outputs['pred_boxes'][sel]}
        if 'aux_outputs' in outputs:
            fo['aux_outputs'] = [{'pred_relevance_logits': a['pred_relevance_logits'][sel], 'pred_boxes': a['pred_boxes'][sel]}
                                 for a in outputs['aux_outputs']]
        losses = self.set_criterion(fo, [targets[i] for i in sel])
        ret = {'loss_ce': 0, 'loss_bbox': 0, 'loss_giou': 0}
        for name in ret:
            for k, v in losses.items():
                if name in k:
                    ret[name] = ret[name] + v
        return ret


_LOSS_MODULES = {'CaptionLoss': CaptionLoss, 'VqaLoss': VqaLoss, 'ClsLoss': ClsLoss, 'Localization': Localization,
                 'AnswerClassification': AnswerClassification}


class GPVCriterion(nn.Module):
    """losses.py:141-176"""

    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.criterion_names = []
        self.loss_wts = {}
        for module_name, loss_cfg in cfg.items():
            setattr(self, loss_cfg.name, _LOSS_MODULES[module_name](loss_cfg))
            self.criterion_names.append(loss_cfg.name)
            self.loss_wts.update(loss_cfg.loss_wts)

    def forward(self, outputs, targets):
        loss_dict = {}
        for name in self.criterion_names:
            loss_dict.update(getattr(self, name)(outputs, targets))
        if all(v is None for v in loss_dict.values()):
            return None, loss_dict
        total = 0
        for k, wt in self.loss_wts.items():
            if loss_dict[k] is not None:
                total = total + wt * loss_dict[k]
        return total, loss_dict
