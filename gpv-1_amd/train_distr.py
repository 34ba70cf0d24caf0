"""Training driver: the step loop around the hot path.

Reference: exp/gpv/train_distr.py (``train_worker`` :150-474, ``main`` :478-495) launched by scripts/train.sh.
What is reproduced -- everything between the data loader and the checkpoint file:
  * Hydra-style invocation: ``python -m gpv1_amd.train_distr [--config some.yaml] key=value ...``
    (config.py; the reference's own YAML loads too);
  * model construction ``GPV(cfg.model)``, optional ``load_pretr_detr()`` (:182-183), phase-1 freeze of the DETR
    parameters that came from the checkpoint (``freeze_detr_params`` :136-140, ``training.freeze`` -> ``frozen_epochs`` /
    ``frozen_batch_size`` :318-320,482-484);
  * the four AdamW groups, clip at ``clip_max_norm`` on DETR parameters, warm-up-linear schedule stepped every iteration
    (:228-253,298-313,421-428,468-469) -- all inside FlatTrainer;
  * one process per GPU (RANK / WORLD_SIZE / LOCAL_RANK from the launcher; the reference ``mp.spawn``s, :493), per-rank
    batch = ``batch_size // world`` (:490), DistributedSampler-style disjoint index shards reshuffled per epoch (:202,396-397);
  * checkpoints in the reference layout (:381-389): ``model`` with ``module.``-prefixed keys (what a DDP-wrapped model
    saves and ``inference.py:59-60`` strips), ``optimizer``, ``epoch``, ``step``, ``lr``, ``model_selection_metric``,
    ``warmup_scheduler``; resume takes every key whose name and size match (:264-271).
  * train-time evaluation and model selection (:325-395) when the caller passes ``eval_datasets``: at the start of every
    epoch (at launch only with ``training.run_eval_at_launch``) rank 0 evaluates every named dataset on the ``train`` and
    ``val`` subsets with gpv1_amd.metrics (at most ``training.num_val_samples[name]`` samples each), logs the figures, forms
    ``model_selection_metric = vqa_acc + cider + det_map + cls_acc`` on ``val`` and writes ``ckpt_dir/model.pth`` only when it
    exceeds the best so far; the periodic and epoch-end saves go to ``model_last.pth`` (carrying the best metric so far), a
    resume takes ``best_metric`` from the checkpoint (:283); the other ranks wait at a barrier.  Detection mAP is scored on
    the device (csrc/det_ap.hip).  ``cider`` comes from the dataset's caption ``scorer`` if it carries one, else from a
    ``caption_scorer.CaptionScorer`` when ``training.caption_scorer`` is ``'device'`` (csrc/caption_score.hip) or ``'host'``, else
    it is 0 and the log says so (the reference's pycocoevalcap is un-vendored); the reference leaves ``refcocop`` out of the
    sum, so its mAP is logged only.  Evaluation leaves the training state alone: ``model.eval()`` / ``no_grad`` /
    ``model.train()``, no RNG draw, the captured training graphs are replayed afterwards, not recaptured.
  * training visualisations (``visualize`` :40-133, called at :454-460) with the added key ``training.visualize: device`` (default
    ``off``: nothing here changes): every ``training.vis_step`` steps (at launch only with ``training.run_vis_at_launch``) rank 0
    writes ``exp_dir/training_visualizations/<subset>_<step>/`` for ``train`` and ``val`` -- the first
    ``training.num_vis_samples`` pictures as the model saw them, boxes drawn and JPEG-encoded on the device
    (gpv1_amd.visualize, csrc/jpeg_enc.hip), and an ``index.html``.  Between steps, outside any graph capture; the batches come from
    the evaluation datasets (``train`` falls back to the training dataset's first batches when there are none).  The added key
    ``training.vis_labels: true`` (default false) writes each predicted box's relevance score above it and ``GT`` below each
    ground-truth box, on the device as well.
Out of scope: dataset ETL (downloading / preprocessing COCO; READING what it wrote is gpv1_amd.datasets), TensorBoard.  Without ``eval_datasets`` this driver checkpoints every
``training.ckpt_step`` steps and at every epoch end into ``model.pth``.
The dataset is any sequence of ``(image[3,H,W] fp32 normalised, query str | (ids, mask), target dict)``;
``SyntheticCocoDataset`` provides BASELINE's synthetic COCO-shaped samples (``training.data_source: synthetic``, the default).
``training.data_source: files`` reads the reference's preprocessed sample files and the COCO image directory that ``task_configs``
names (gpv1_amd.datasets: ``CocoMultitaskDataset`` behind a ``DeviceLoader`` that prepares one batch ahead and feeds the
device-side JPEG decoder and image pipeline); ``eval_datasets`` then defaults to the same mix on ``train`` and ``val``.  An evaluation dataset is such a sequence with
a ``samples`` list beside it (the reference's ``dataset.samples``: the dicts the evaluators read), optionally ``synonyms``
(classification) and ``scorer`` (captioning).
"""
import argparse
import os
import sys
import time

import torch
import torch.distributed as dist

from .config import from_dict, load_config
from .default_config import default_tree, GROUP_OPTIONS
from .gpv import GPV
from .misc import nested_tensor_from_tensor_list
from .train import FlatTrainer


def freeze_detr_params(model, requires_grad=False):
    """train_distr.py:136-140"""
    for n, p in model.named_parameters():
        if n in model.init_detr_params:
            p.requires_grad = requires_grad


class SyntheticCocoDataset:
    """SURVEY §8(d) synthetic samples: N(0,1) images, random query ids, the four task target types round-robin."""

    def __init__(self, n, vocab, image_size=(480, 640), query_len=6, seed=0, tasks=('CocoCaptioning', 'CocoVqa', 'CocoClassification', 'CocoDetection')):
        self.n, self.vocab, self.size, self.tl, self.seed, self.tasks = n, vocab, image_size, query_len, seed, tasks

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed * 1000003 + i)
        img = torch.randn(3, *self.size, generator=g)
        ids = torch.randint(1000, 30000, (self.tl,), generator=g)
        task = self.tasks[i % len(self.tasks)]
        words = [self.vocab[int(j)] for j in torch.randint(0, len(self.vocab) - 4, (19 if task == 'CocoCaptioning' else 2,), generator=g)]
        t = {'task': task}
        if task == 'CocoDetection':
            nb = int(torch.randint(1, 11, (1,), generator=g))
            cxcy = 0.25 + 0.5 * torch.rand(nb, 2, generator=g)
            wh = 0.05 + 0.3 * torch.rand(nb, 2, generator=g)
            t.update(boxes=torch.cat([cxcy, wh], 1), labels=torch.zeros(nb, dtype=torch.long))
        else:
            t['answer'] = ' '.join(words)
        return img, (ids, torch.ones(self.tl, dtype=torch.long)), t


def shard_indices(n, epoch, rank, world, seed=0):
    """torch.utils.data.DistributedSampler(shuffle=True): permutation seeded by (seed + epoch), padded to a multiple of
    world by wrapping, rank takes every world-th element."""
    g = torch.Generator().manual_seed(seed + epoch)
    idx = torch.randperm(n, generator=g).tolist()
    total = -(-n // world) * world
    idx += idx[:total - n]
    return idx[rank:total:world]


def batches(dataset, indices, batch_size, device, epoch=0):
    loader = getattr(dataset, 'loader', None)
    if loader is not None:                     # gpv1_amd.datasets.DeviceLoader: files -> device-side decode and transform, one batch ahead
        yield from loader.batches(indices, epoch, batch_size)
        return
    for s in range(0, len(indices) - batch_size + 1, batch_size):
        items = [dataset[i] for i in indices[s:s + batch_size]]
        imgs = [it[0].to(device) for it in items]
        qs = [it[1] for it in items]
        if isinstance(qs[0], str):
            queries = qs
        else:
            queries = (torch.stack([q[0] for q in qs]).to(device), torch.stack([q[1] for q in qs]).to(device))
        targets = []
        for it in items:
            targets.append({k: (v.to(device) if torch.is_tensor(v) else v) for k, v in it[2].items()})
        yield nested_tensor_from_tensor_list(imgs), queries, targets


def eval_batches(dataset, batch_size, device):
    """the evaluation loader (train_distr.py:336-341: shuffle=False, the last batch may be short)"""
    loader = getattr(dataset, 'loader', None)
    if loader is not None:
        yield from loader.eval_batches(batch_size)
        return
    n = len(dataset)
    for s in range(0, n, batch_size):
        items = [dataset[i] for i in range(s, min(n, s + batch_size))]
        qs = [it[1] for it in items]
        queries = qs if isinstance(qs[0], str) else (torch.stack([q[0] for q in qs]).to(device), torch.stack([q[1] for q in qs]).to(device))
        yield nested_tensor_from_tensor_list([it[0].to(device) for it in items]), queries, [it[2] for it in items]


def _eval_vqa(model, batches_, ds, limit):
    from . import metrics
    return metrics.vqa_accuracy(model, batches_, ds.samples, limit)


def _eval_cls(model, batches_, ds, limit):
    from . import metrics
    return metrics.cls_metrics(model, batches_, ds.samples, limit, synonyms=getattr(ds, 'synonyms', None))


def _eval_cap(model, batches_, ds, limit, mode=None, caption_beam=None):
    """mode: cfg.training.caption_scorer -- 'device' | 'host' builds a caption_scorer.CaptionScorer when the dataset carries no scorer.
    caption_beam: cfg.training.caption_beam -- absent: greedy captions, as the reference; a group of `size` and the beam.* keys of
    inference.beam_options: captions by beam search (metrics.cap_metrics)"""
    from . import metrics
    scorer = getattr(ds, 'scorer', None)
    if scorer is None and mode is not None:
        if mode not in ('device', 'host'):
            raise ValueError(f"training.caption_scorer must be 'device' or 'host', got {mode!r}")
        from .caption_scorer import CaptionScorer
        scorer = CaptionScorer(device=None if mode == 'host' else metrics._device(model), host=mode == 'host')
    if caption_beam:
        beam = {k: v for k, v in dict(caption_beam).items() if k != 'size'}
        scores, _ = metrics.cap_metrics(model, batches_, ds.samples, limit, scorer=scorer, beam_size=int(dict(caption_beam).get('size') or 1),
                                        beam=beam)
    else:
        scores, _ = metrics.cap_metrics(model, batches_, ds.samples, limit, scorer=scorer)
    return scores


def _eval_det(model, batches_, ds, limit):
    from . import metrics
    return metrics.det_metrics(model, batches_, ds.samples, limit)


def _eval_refexp(model, batches_, ds, limit):
    from . import metrics
    return metrics.refexp_metrics(model, batches_, ds.samples, limit)


# dataset name -> (model, batches, dataset, limit) -> figure; the names of configs/learning_datasets/*.yaml
EVAL_FNS = {'coco_vqa': _eval_vqa, 'coco_cls': _eval_cls, 'coco_cap': _eval_cap, 'coco_det': _eval_det, 'refcocop': _eval_refexp}


def evaluate_subset(model, datasets, subset, cfg, epoch, device, log=print, said=None):
    """train_distr.py:328-380 for one subset: every named dataset through its metric function, figures logged;
    -> vqa_acc + cider + det_map + cls_acc (what is absent counts 0).  Leaves the model in the mode it was in and draws no random number.
    said: a set that remembers the notes already logged (the missing caption scorer is mentioned once per run)."""
    said = set() if said is None else said
    tr_cfg = cfg.training
    limits = tr_cfg.get('num_val_samples', None) or {}
    batch_size = int(cfg.get('batch_size', None) or tr_cfg.batch_size)
    vqa_acc = cls_acc = cider = det_map = 0
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for name, ds in datasets.items():
                fn = EVAL_FNS.get(name)
                if fn is None:
                    log(f'Eval not implemented for {name}')
                    continue
                if fn is _eval_cap:
                    out = fn(model, eval_batches(ds, batch_size, device), ds, limits.get(name, None), tr_cfg.get('caption_scorer', None),
                             tr_cfg.get('caption_beam', None))
                else:
                    out = fn(model, eval_batches(ds, batch_size, device), ds, limits.get(name, None))
                if name == 'coco_vqa':
                    vqa_acc = out
                    log(f'Dataset: {name} | Subset: {subset} | Epoch: {epoch} | Acc: {out}')
                elif name == 'coco_cls':
                    cls_acc = out
                    log(f'Dataset: {name} | Subset: {subset} | Epoch: {epoch} | Acc: {out}')
                elif name == 'coco_cap':
                    if 'Cider' in out:
                        cider = out['Cider']
                        log(f"Dataset: {name} | Subset: {subset} | Epoch: {epoch} | Bleu1: {out.get('Bleu1')} | Bleu4: {out.get('Bleu4')} | Cider: {cider}")
                    elif 'no_cider' not in said:
                        said.add('no_cider')
                        log(f'Dataset: {name}: no caption scorer was supplied (Bleu / CIDEr are not vendored): cider = 0 enters model_selection_metric')
                elif name == 'coco_det':
                    det_map = out
                    log(f'Dataset: {name} | Subset: {subset} | Epoch: {epoch} | mAP: {out}')
                else:
                    log(f'Dataset: {name} | Subset: {subset} | Epoch: {epoch} | mAP: {out} (not part of model_selection_metric)')
    finally:
        model.train(was_training)
    return vqa_acc + cider + det_map + cls_acc


def visualize_subsets(model, cfg, step, dataset, eval_datasets, batch_size, device, log=print):
    """train_distr.py:456-460 on rank 0: `train` and `val` through gpv1_amd.visualize.  A subset's batches are those of its
    evaluation datasets, one after the other (visualize stops after training.num_vis_samples); without evaluation datasets `train`
    reads the training dataset from its start (unless a loader feeds it: that loader is in the middle of the epoch) and `val` is left
    out."""
    import itertools
    from .visualize import visualize
    for subset in ('train', 'val'):
        sets = list((eval_datasets or {}).get(subset, {}).values()) or ([dataset] if subset == 'train' and getattr(dataset, 'loader', None) is None else [])
        if not sets:
            continue
        log(f'Visualizing {subset} ...')
        visualize(model, itertools.chain.from_iterable(eval_batches(ds, batch_size, device) for ds in sets), cfg, step, subset,
                  labels=bool(cfg.training.get('vis_labels', False)))


def save_checkpoint(path, model, trainer, epoch, step, metric=0.0):
    """train_distr.py:381-389 (DDP state dict => 'module.' prefix)"""
    sd = {'module.' + k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    tmp = path + '.tmp'
    torch.save({'model': sd, 'optimizer': trainer.state_dict(), 'epoch': epoch, 'step': step,
                'lr': list(trainer.current_lrs().values()), 'model_selection_metric': metric,
                'warmup_scheduler': {'last_epoch': trainer.step_count, 'warmup_steps': trainer.warmup_steps, 't_total': trainer.t_total}}, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, model, trainer=None, map_location='cpu'):
    """train_distr.py:262-285 -- keys with or without the 'module.' prefix, only name+size matches are taken"""
    ckpt = torch.load(path, map_location=map_location, weights_only=False)
    cur = model.state_dict()
    taken = 0
    for k, v in ckpt['model'].items():
        k = k[len('module.'):] if k.startswith('module.') else k
        if k in cur and cur[k].size() == v.size():
            cur[k] = v
            taken += 1
    model.load_state_dict(cur)
    if trainer is not None and ckpt.get('optimizer') is not None:
        trainer.load_state_dict(ckpt['optimizer'], step=ckpt.get('step'))      # torch.optim.AdamW layout (reference checkpoints) or round-1 layout
    return ckpt, taken


def file_datasets(cfg, batch_size, device, train=True, evals=True):
    """training.data_source: files -- the reference's datasets behind DeviceLoaders (gpv1_amd.datasets):
    -> (CocoMultitaskDataset(cfg.learning_datasets, cfg.task_configs, 'train') | None, {'train' | 'val': {name: dataset}} | None: the same
    mix per name as train_distr.py:163-166 / :328-341 build it).  A missing sample file or image directory raises, naming the path."""
    from .datasets import DATASETS, CocoMultitaskDataset, DeviceLoader
    tr_cfg = cfg.training
    kw = dict(device=device, threads=max(1, min(16, int(tr_cfg.get('num_workers', 8)))), prefetch=int(tr_cfg.get('prefetch', 1)),
              entropy=os.environ.get('GPV_JPEG_ENTROPY') or tr_cfg.get('jpeg_entropy', 'host'))    # 'device': Huffman walk on the GPU (opt-in)
    if 'task_configs' not in cfg:
        raise KeyError('training.data_source: files needs a task_configs tree (gpv1_amd.default_config)')
    train_ds, eval_ds = None, None
    if train:
        train_ds = CocoMultitaskDataset(cfg.learning_datasets, cfg.task_configs, 'train', seed=int(cfg.get('seed', 0) or 0))
        DeviceLoader(train_ds, batch_size, **kw)
    for subset in ('train', 'val') if evals else ():
        eval_ds = eval_ds or {}
        eval_ds[subset] = {}
        for cls_name, info in cfg.learning_datasets.items():
            ds = eval_ds[subset][info['name']] = DATASETS[cls_name](cfg.task_configs[info['task_config']], subset)
            DeviceLoader(ds, int(cfg.get('batch_size', None) or tr_cfg.batch_size), **kw)
    return train_ds, eval_ds


def train_worker(cfg, dataset=None, device=None, log=print, eval_datasets=None):
    """one rank of the reference's ``train_worker``; returns (model, trainer, step).
    eval_datasets: None, or {'train' | 'val': {'coco_vqa' | 'coco_cls' | 'coco_cap' | 'coco_det' | 'refcocop': dataset}} -- evaluation
    at every epoch start and best-metric checkpoints (module docstring)"""
    rank = int(os.environ.get('RANK', 0))
    world = int(os.environ.get('WORLD_SIZE', 1))
    local = int(os.environ.get('LOCAL_RANK', 0))
    if device is None:
        device = f'cuda:{local}'
    if str(device).startswith('cuda'):
        torch.cuda.set_device(local)
    if world > 1 and not dist.is_initialized():
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1')
        os.environ.setdefault('MASTER_PORT', '10001')                      # dist_url tcp://localhost:10001
        from .train import init_process_group
        init_process_group(rank, world, device)
    tr_cfg = cfg.training
    batch_size = tr_cfg.frozen_batch_size if tr_cfg.freeze else tr_cfg.batch_size
    per_rank = max(1, batch_size // world)
    epochs = tr_cfg.frozen_epochs if tr_cfg.freeze else tr_cfg.num_epochs

    model = GPV(cfg.model)
    if cfg.model.pretr_detr is not None and os.path.exists(str(cfg.model.pretr_detr)):
        model.load_pretr_detr()
    if tr_cfg.freeze:
        freeze_detr_params(model)
    model.to(device)
    source, own_loaders = tr_cfg.get('data_source', 'synthetic'), []
    if source not in ('synthetic', 'files'):
        raise ValueError(f"training.data_source must be 'synthetic' or 'files', got {source!r}")
    if dataset is None and source == 'files':
        dataset, auto_evals = file_datasets(cfg, per_rank, device, evals=eval_datasets is None)
        own_loaders.append(dataset.loader)
        if eval_datasets is None:
            eval_datasets = auto_evals
            own_loaders += [ds.loader for sub in auto_evals.values() for ds in sub.values()]
    if dataset is None:
        # the task mix: configs/learning_datasets/<name>.yaml selected by `learning_datasets=<name>` (scripts/train.sh:14-34),
        # CocoMultitaskDataset(cfg.learning_datasets, ...) in the reference (train_distr.py:163-166)
        tasks = tuple(cfg.get('learning_datasets', {}) or ()) or ('CocoCaptioning', 'CocoVqa', 'CocoClassification', 'CocoDetection')
        dataset = SyntheticCocoDataset(int(cfg.get('synthetic_samples', 4 * batch_size)), model.vocab, tasks=tasks)
    steps_per_epoch = (-(-len(dataset) // world)) // per_rank
    t_total = steps_per_epoch * epochs if tr_cfg.lr_linear_decay else 0
    have_ckpt = tr_cfg.ckpt is not None and os.path.exists(str(tr_cfg.ckpt))
    if not model.bert.pretrained and not have_ckpt:
        # the reference's query encoder is BertModel.from_pretrained('bert-base-uncased') (bert.py:8-9), frozen: training against
        # a random-init BERT is only meaningful for throughput / plumbing runs
        log(f'[rank {rank}] WARNING: BERT has random weights (no model.bert_weights / GPV_BERT_WEIGHTS and no checkpoint): '
            f'the frozen query encoder is NOT bert-base-uncased')
        if cfg.get('require_pretrained_bert', False):
            raise RuntimeError('training.require_pretrained_bert is set and no BERT weights were given')
    sched = {}
    if not tr_cfg.lr_linear_decay:                         # MultiStepLR per epoch x GradualWarmup over epoch 0 (train_distr.py:288-308)
        sched = {'lr_milestones': list(tr_cfg.get('lr_milestones', []) or []), 'lr_drop': tr_cfg.get('lr_drop', 0.1),
                 'warmup_iters': steps_per_epoch if tr_cfg.lr_warmup else 0}
    trainer = FlatTrainer(model, lr=tr_cfg.lr, lr_backbone=tr_cfg.lr_backbone, weight_decay=tr_cfg.weight_decay,
                          clip_max_norm=tr_cfg.clip_max_norm,
                          warmup_steps=int(tr_cfg.lr_warmup_fraction * t_total) if tr_cfg.lr_warmup else 0, t_total=t_total, **sched)
    # training.health (optional, not in the default tree): {every, ring, watch, on_nonfinite} -> the flight recorder (health.py)
    health_cfg, recorder = tr_cfg.get('health', None), None
    if health_cfg:
        from .health import FlightRecorder
        recorder = trainer.recorder = FlightRecorder(trainer, watch=tuple(health_cfg.get('watch', None) or ('G',)),
                                                     ring=int(health_cfg.get('ring', 64)), every=int(health_cfg.get('every', 1)),
                                                     on_nonfinite=health_cfg.get('on_nonfinite', 'raise'))
    step, last_epoch, best_metric, said = 0, -1, 0.0, set()
    if have_ckpt:
        ckpt, taken = load_checkpoint(tr_cfg.ckpt, model, trainer, map_location=device)
        step, last_epoch = ckpt['step'], ckpt['epoch']
        if eval_datasets is not None:
            best_metric = ckpt.get('model_selection_metric', 0.0) or 0.0   # a checkpoint is the best so far (train_distr.py:283)
        log(f'[rank {rank}] resumed {tr_cfg.ckpt}: {taken} tensors, end of epoch {last_epoch}, step {step}')
    best_path = os.path.join(cfg.ckpt_dir, 'model.pth')
    # with evaluators model.pth is the best model so far and the running state goes next to it
    ckpt_path = os.path.join(cfg.ckpt_dir, 'model_last.pth') if eval_datasets is not None else best_path
    if rank == 0:
        os.makedirs(cfg.ckpt_dir, exist_ok=True)
    max_steps = cfg.get('max_steps', None)
    vis_mode = tr_cfg.get('visualize', 'off')
    if vis_mode not in ('off', 'device'):
        raise ValueError(f"training.visualize must be 'off' or 'device', got {vis_mode!r}")
    t0 = time.time()
    launch = vis_launch = True
    for epoch in range(last_epoch + 1, epochs):
        if eval_datasets is not None and ((not launch) or tr_cfg.get('run_eval_at_launch', True)):
            if rank == 0:
                for subset in ('train', 'val'):
                    if subset not in eval_datasets:
                        continue
                    metric = evaluate_subset(model, eval_datasets[subset], subset, cfg, epoch, device, log, said)
                    if subset == 'val':
                        log(f'Epoch: {epoch} | model_selection_metric: {metric} | best so far: {best_metric}')
                        if metric > best_metric:
                            log('Saving checkpoint ...')
                            best_metric = metric
                            save_checkpoint(best_path, model, trainer, epoch - 1, step, metric)
            if world > 1:
                dist.barrier()                                   # the other ranks wait for rank 0's evaluation
                from .misc import note_sync_collective
                note_sync_collective()
        launch = False
        idx = shard_indices(len(dataset), epoch, rank, world)
        epoch_done = True                     # False: max_steps ended the epoch before its last batch
        batch_iter = iter(batches(dataset, idx, per_rank, device, epoch))
        for it, (imgs, queries, targets) in enumerate(batch_iter):
            trainer.set_epoch(epoch, it)
            loss = trainer.train_step(imgs, queries, targets)
            step += 1
            if vis_mode == 'device':
                # the reference tests the step count before its increment, after the step: the first step of a run visualises only
                # with run_vis_at_launch
                if rank == 0 and (step - 1) % tr_cfg.vis_step == 0 and ((not vis_launch) or tr_cfg.run_vis_at_launch):
                    visualize_subsets(model, cfg, step - 1, dataset, eval_datasets, per_rank, device, log)
                vis_launch = False
            if rank == 0 and step % tr_cfg.log_step == 0:
                line = (f'epoch {epoch} step {step} loss {float(loss.detach()) if loss is not None else float("nan"):.4f} '
                        f'lr {trainer.current_lrs()["others"]:.3e} {time.time() - t0:.1f}s')
                reading = recorder.read() if recorder is not None else None       # (behind the loss read above, which already waited)
                if reading is not None and reading.commits:
                    norms = reading.grad_norms()
                    if norms is not None:
                        line += ' gnorm ' + ' '.join(f'{g} {v:.4e}' for g, v in norms.items())
                log(line)
                if reading is not None and reading.trip is not None:
                    if not recorder._warned:
                        recorder.write_report(reading, os.path.join(cfg.ckpt_dir, 'nonfinite_report.json'))
                    recorder.check(reading)                                       # raises, or warns once (on_nonfinite)
            if rank == 0 and step % tr_cfg.ckpt_step == 0:
                # like the reference's mid-epoch save (train_distr.py:372-389: 'epoch': epoch-1 next to the CURRENT step): a
                # resume re-runs this epoch from its start while the schedule continues from `step` -- the reference's behaviour,
                # kept as is (with lr_linear_decay the tail of such a run sits at lr 0 once step passes t_total)
                save_checkpoint(ckpt_path, model, trainer, epoch - 1, step, best_metric)
            if max_steps is not None and step >= max_steps:
                epoch_done = next(batch_iter, None) is None      # stopped on the epoch's last batch: the epoch is complete
                break
        batch_iter.close()                    # (a loader's worker thread is joined here when max_steps left the epoch early)
        stopped = max_steps is not None and step >= max_steps
        if rank == 0:
            save_checkpoint(ckpt_path, model, trainer, epoch if epoch_done else epoch - 1, step, best_metric)
        if stopped:
            break
    for loader in own_loaders:                # the loaders this call built: their worker and pool threads end with it
        loader.close()
    if world > 1:
        dist.barrier()
        from .misc import note_sync_collective
        note_sync_collective()
    return model, trainer, step


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--config', default=None, help='YAML file (e.g. the reference configs/exp/gpv.yaml); default: gpv1_amd.default_config')
    ap.add_argument('overrides', nargs='*', help='Hydra-style key=value overrides')
    args = ap.parse_args(argv)
    cfg = load_config(args.config, args.overrides) if args.config else from_dict(default_tree(), args.overrides, group_options=GROUP_OPTIONS)
    train_worker(cfg)


if __name__ == '__main__':
    main(sys.argv[1:])
