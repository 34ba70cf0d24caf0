"""Windowed sources and three-step jitter in the device input pipeline (csrc/image_pipeline.hip), and gpv1_amd.datasets end to end on
the device: sample files -> DeviceLoader -> the stem's batch -> graphed train steps under the driver.  The image reference is
oracle/image_oracle.py on the Pillow decode of the golden files ("parity unpinned" against skimage / torchvision, as there)."""
import os
import random

import numpy as np
import pytest
import torch

from tests import coco_tree as CT
from tests.datasets_cases import CASES, ORACLE_CASES, P0, make_images

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EXPECTED = os.path.join(CT.GOLD, 'expected.npz')


@pytest.fixture()
def rt():
    import gpv1_amd.ops as ops
    import gpv1_amd.hip as hip
    hip.lib()
    yield ops.RT
    ops.RT.set_precise(False)


def as_rgb(a):
    return a if a.ndim == 3 else np.repeat(a[..., None], 3, 2)


def check_against_oracle(got, ref, dtype, what):
    """the rule of test_device_input_pipeline_vs_oracle: differences in uint8 steps <= 1 + tol for >= 99.5 % of the values, never
    more than 3 + tol; tol = 0.6 in fp32, 2.0 in bf16 (output rounding)"""
    from oracle import image_oracle as IO
    steps = np.abs(got - ref) * (255.0 * IO.STD)
    tol = 0.6 if dtype == torch.float32 else 2.0
    print('ORACLE', what, dtype, 'max %.3f' % float(steps.max()), 'within %.5f' % float((steps <= 1.0 + tol).mean()))
    assert (steps <= 1.0 + tol).mean() >= 0.995 and steps.max() <= 3.0 + tol, (what, dtype, float(steps.max()), float((steps <= 1 + tol).mean()))


@pytest.mark.parametrize('size', [(96, 128), (64, 96)])
def test_window_equals_copy_exactly_and_matches_the_oracle(rt, size):
    """pipe(images, crops=windows) == pipe(contiguous copies of the windows), bit for bit, in fp32 and bf16: the kernel addresses the
    window through the descriptor's pitch, mirrors at the WINDOW's borders and reads nothing outside it.  The last image of the
    batch lies inside a guard of 255s (and is the last allocation), so a tap outside the window would change the result.  The
    same outputs then against the oracle run on the sliced array."""
    from oracle import image_oracle as IO
    from gpv1_amd.input_pipeline import DeviceImagePipeline, stem_geometry
    H, W = size
    imgs = make_images()
    names = list(CASES)
    sources = [torch.from_numpy(imgs[CASES[n][0]]) for n in names]
    crops = [CASES[n][1] for n in names]
    params = [CASES[n][2] for n in names]
    copies = [s[y1:y2, x1:x2].contiguous() for s, (y1, y2, x1, x2) in zip(sources, crops)]
    # the guarded source: image 'e' in the middle of a frame of 255s; its window touches the image's bottom-right corner
    g = 24
    eh, ew = imgs['e'].shape[:2]
    guarded = torch.full((eh + 2 * g, ew + 2 * g, 3), 255, dtype=torch.uint8)
    guarded[g:g + eh, g:g + ew] = torch.from_numpy(imgs['e'])
    _, (y1, y2, x1, x2), pg = CASES['bottom_right_jitter']
    sources, crops, params = sources + [guarded], crops + [(g + y1, g + y2, g + x1, g + x2)], params + [pg]
    copies.append(torch.from_numpy(imgs['e'])[y1:y2, x1:x2].contiguous())
    names.append('guarded_bottom_right')
    pipe = DeviceImagePipeline(size=size, train=True)
    Hp, Wp = stem_geometry(H, W)
    for dtype in (torch.float32, torch.bfloat16):
        rt.set_precise(dtype == torch.float32)
        a = pipe(sources, params=params, crops=crops).tensors
        b = pipe(copies, params=params).tensors
        torch.cuda.synchronize()
        assert a.dtype == dtype and a.shape == (len(names), Hp, Wp, 4)
        for i, n in enumerate(names):
            assert torch.equal(a[i], b[i]), (n, dtype, int((a[i] != b[i]).sum()))
        out = a.float().cpu().numpy()
        frame = out.copy()
        frame[:, 3:3 + H, 3:3 + W, :3] = 0
        assert np.all(frame == 0)                                                   # padding ring + 4th channel exactly zero
        for i, n in enumerate(names):
            if n in ORACLE_CASES or n == 'guarded_bottom_right':
                ref = IO.pipeline(copies[i].numpy(), size, params[i]).transpose(1, 2, 0)
                check_against_oracle(out[i, 3:3 + H, 3:3 + W, :3], ref, dtype, n)


def test_three_step_orders_and_no_hue_round_trip(rt):
    """order[] with three entries (ColorJitter(0.2, 0.2, 0.2, 0) has no hue step): every permutation of (0, 1, 2) against the oracle,
    and -- where R = G = B, which a hue round trip through HSV would disturb -- exactly the image whose steps were applied by hand on
    the host (1.25 / 0.75 / 1.5: every product is exact in fp32)"""
    import itertools
    from oracle import image_oracle as IO
    from gpv1_amd.input_pipeline import DeviceImagePipeline
    H, W = 64, 96
    img = make_images()['b']                                                        # 60 x 90
    perms = list(itertools.permutations((0, 1, 2)))
    params = [dict(P0, jitter=1, order=o, brightness=1.25, contrast=0.75, saturation=1.5, flip=i % 2) for i, o in enumerate(perms)]
    pipe = DeviceImagePipeline(size=(H, W), train=True)
    for dtype in (torch.float32, torch.bfloat16):
        rt.set_precise(dtype == torch.float32)
        out = pipe([torch.from_numpy(img)] * len(perms), params=params).tensors.float().cpu().numpy()
        for i, p in enumerate(params):
            check_against_oracle(out[i, 3:3 + H, 3:3 + W, :3], IO.pipeline(img, (H, W), p).transpose(1, 2, 0), dtype, p['order'])
    # a grey-valued image at the output size (the resize is the identity): jitter on the device == jitter by hand + no jitter
    rt.set_precise(True)
    yy, xx = np.mgrid[0:H, 0:W]
    v = ((yy * 3 + xx * 2) % 256).astype(np.uint8)
    grey = np.stack([v, v, v], -1)
    for order in perms:
        x = v.astype(np.float32)
        for op in order:
            if op == 0:
                x = np.rint(np.clip(x * np.float32(1.25), 0, 255))
            elif op == 1:
                m = np.floor(x.astype(np.float64).mean() + 0.5)                     # L = x where R = G = B
                x = np.rint(np.clip(m + np.float32(0.75) * (x - m), 0, 255)).astype(np.float32)
            # saturation: L + s (x - L) = x where R = G = B
        hand = np.stack([x.astype(np.uint8)] * 3, -1)
        p = dict(P0, jitter=1, order=order, brightness=1.25, contrast=0.75, saturation=1.5)
        a = pipe([torch.from_numpy(grey)], params=[p]).tensors
        b = pipe([torch.from_numpy(hand)], params=[P0]).tensors
        assert torch.equal(a, b), order
        rgb = a[0, 3:3 + H, 3:3 + W, :3].cpu().numpy() * IO.STD + IO.MEAN
        assert np.abs(rgb - rgb[..., :1]).max() < 1e-6                               # still R = G = B


def _direct(ds, indices, epoch, dec, pipe, exp):
    """what the dataset rule gives for these samples, fed to decoder and pipeline directly"""
    from gpv1_amd.datasets import sample_seed
    files, params, crops, queries, targets = [], [], [], [], []
    for i in indices:
        d, k = ds.locate(i)
        files.append(open(d.image_path(k), 'rb').read())
        Hs, Ws = exp[CT.IMAGES[d.samples[k]['image']['image_id']]].shape[:2]
        p, c, q, t = d.draw(k, random.Random(sample_seed(ds.seed, epoch, i)), Hs, Ws)
        params.append(p); crops.append(c); queries.append(q); targets.append(t)
    return pipe(dec(files), params=params, crops=crops), params, crops, queries, targets


def test_files_to_batch_through_the_loader(rt, tmp_path):
    from oracle import image_oracle as IO
    from gpv1_amd.datasets import CocoMultitaskDataset, DeviceLoader
    from gpv1_amd.jpeg import DeviceJpegDecoder
    from gpv1_amd.input_pipeline import DeviceImagePipeline
    size = (64, 96)
    exp = np.load(EXPECTED)
    plan = {'cap': {'train': [2], 'val': [2, 3]}, 'det': {'train': [4], 'val': [4]}, 'cls': {'train': [1]}, 'vqa': {'train': [3]},
            'refcocop': {'train': [6]}}
    tc = CT.make_tree(tmp_path, plan, image_size=size)
    kinds = ('cap', 'det', 'cls', 'vqa', 'refcocop')
    ds = CocoMultitaskDataset(CT.learning_datasets(kinds), tc, 'train', seed=5)       # ids 2 (grey), 4, 1 (crop), 3 (29 x 43), 6
    assert len(ds) == 5
    dec, pipe = DeviceJpegDecoder(threads=2), DeviceImagePipeline(size=size, train=True)
    order = [3, 0, 2, 4, 1]
    for dtype in (torch.bfloat16, torch.float32):
        rt.set_precise(dtype == torch.float32)
        for prefetch in (1, 0):
            loader = DeviceLoader(ds, 5, device=DEV, threads=2, prefetch=prefetch)
            got = list(loader.batches(order, epoch=2))
            loader.close()
            assert len(got) == 1
            samples, queries, targets = got[0]
            want, params, crops, wq, wt = _direct(ds, order, 2, dec, pipe, exp)
            assert samples.tensors.dtype == dtype and torch.equal(samples.tensors, want.tensors) and not bool(samples.mask.any())
            assert queries == wq and crops[2] == (92, 120, 9, 16) and [c for i, c in enumerate(crops) if i != 2] == [None] * 4
            for t, w in zip(targets, wt):
                assert set(t) == set(w) and t['task'] == w['task'] and t.get('answer') == w.get('answer')
                if 'boxes' in w:
                    assert t['boxes'].is_cuda and t['labels'].is_cuda and t['labels'].dtype == torch.long and t['boxes'].dtype == torch.float32
                    assert torch.equal(t['boxes'].cpu(), w['boxes']) and torch.equal(t['labels'].cpu(), w['labels'])
            assert [t['task'] for t in targets] == ['CocoVqa', 'CocoCaptioning', 'CocoClassification', 'RefCocop', 'CocoDetection']
            x, y, w_, h = ds.datasets['coco_det'].samples[0]['boxes'][0]
            box = torch.tensor([[x + 0.5 * w_, y + 0.5 * h, w_, h]], dtype=torch.float64).float() / torch.tensor([64, 48, 64, 48], dtype=torch.float32)
            assert torch.equal(targets[4]['boxes'].cpu(), box)
        # independently of decoder and dataset code: the classification sample against the oracle on Pillow's decode, cropped by hand
        ref = IO.pipeline(exp['c420_big'][92:120, 9:16], size, params[2]).transpose(1, 2, 0)
        check_against_oracle(samples.tensors[2, 3:3 + size[0], 3:3 + size[1], :3].float().cpu().numpy(), ref, dtype, 'classification crop')
    assert any(p['jitter'] for p in params)
    # val: no augmentation, in order, a short last batch
    rt.set_precise(False)
    val = CocoMultitaskDataset(CT.learning_datasets(('cap', 'det')), tc, 'val')
    loader = DeviceLoader(val, 2, device=DEV, threads=2, prefetch=1)
    got = list(loader.eval_batches())
    loader.close()
    assert [g[0].tensors.shape[0] for g in got] == [2, 1] and [len(g[1]) for g in got] == [2, 1]
    files = [open(val.locate(i)[0].image_path(val.locate(i)[1]), 'rb').read() for i in range(3)]
    plain = pipe(dec(files), params=[P0] * 3).tensors
    assert torch.equal(torch.cat([g[0].tensors for g in got]), plain)
    assert got[1][2][0]['task'] == 'CocoDetection' and got[1][2][0]['boxes'].is_cuda


def test_driver_trains_from_files_under_graphs(rt, tmp_path, monkeypatch):
    """train_worker with training.data_source=files on the small model: the loader's worker thread runs beside graph capture and
    replay without disturbing them, prefetch 1 and 0 feed the same batches, and the auto-built evaluation datasets are read"""
    from tests.test_drivers_cpu import _driver_cfg
    from tests.test_model_cpu import GOLD
    from gpv1_amd import train_distr as td, datasets as D
    rt.set_precise(False)
    monkeypatch.setenv('GPV_BERT_VOCAB', os.path.join(GOLD, 'bert_vocab_synthetic.txt'))
    ids = [1, 2, 3, 4, 5, 6]
    plan = {k: {'train': ids[:n], 'val': ids[:2]} for k, n in (('det', 6), ('vqa', 5), ('cap', 5))}
    tc = CT.make_tree(tmp_path / 'data', plan, image_size=(64, 96))
    disabled = []
    monkeypatch.setattr(td.FlatTrainer, 'disable_graphs', lambda self, why: disabled.append(why))
    real_issue = D.DeviceLoader._issue
    sums = {}

    def issue(self, hb):
        out = real_issue(self, hb)
        if isinstance(self.dataset, D.CocoMultitaskDataset):
            sums[self.prefetch].append((hb.indices, int(out[0].tensors.view(torch.int16).long().sum()), out[1]))
        return out
    monkeypatch.setattr(D.DeviceLoader, '_issue', issue)
    for prefetch in (1, 0):
        sums[prefetch] = []
        cfg = _driver_cfg(tmp_path / f'run{prefetch}', data_source='files', batch_size=4, num_workers=2, prefetch=prefetch, num_epochs=4,
                          run_eval_at_launch=False)
        cfg.model['bert_dropout'] = None
        cfg['max_steps'] = 8
        cfg['learning_datasets'] = CT.learning_datasets(('det', 'vqa', 'cap'))
        cfg['task_configs'] = tc
        logs = []
        model, tr, step = td.train_worker(cfg, device=DEV, log=logs.append)
        losses = [float(l.split('loss ')[1].split()[0]) for l in logs if l.startswith('epoch')]
        print('FILES DRIVER prefetch %d: graph steps %d eager %d losses %s' % (prefetch, tr.graph_steps, tr.eager_steps, losses))
        assert step == 8 and len(losses) == 8 and all(np.isfinite(losses))
        assert tr.graph_steps >= 3, (tr.graph_steps, tr.eager_steps)
        assert not disabled and tr.graphs and not hasattr(tr, 'graphs_off_reason')
        assert not any(t.name.startswith('gpv-loader') for t in __import__('threading').enumerate())
        # the auto-built evaluation datasets were read at the start of epoch 1
        assert any('Dataset: coco_det | Subset: val' in l for l in logs) and any('Dataset: coco_vqa | Subset: train' in l for l in logs)
        assert any('model_selection_metric' in l for l in logs)
    assert len(sums[1]) >= 8 and sums[1][:8] == sums[0][:8]
    # and directly: evaluate_subset over datasets nobody supplied
    _, evals = td.file_datasets(cfg, 4, DEV, train=False)
    assert set(evals) == {'train', 'val'} and list(evals['val']) == ['coco_det', 'coco_vqa', 'coco_cap']
    assert len(evals['val']['coco_det'].samples) == 2 and 'all_answers' in evals['val']['coco_vqa'].samples[0]
    metric = td.evaluate_subset(model, evals['val'], 'val', cfg, 0, DEV, log=logs.append)
    assert np.isfinite(metric) and model.training
    for d in evals['val'].values():
        d.loader.close()
    # leave nothing of this run behind for the tests that follow in the process: graph bodies, pools, pending work
    del model, tr, evals
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def test_default_data_source_is_synthetic_on_the_device(rt, tmp_path, monkeypatch):
    from tests.test_drivers_cpu import _driver_cfg
    from tests.test_datasets_cpu import iterated_dataset_type
    from gpv1_amd import train_distr as td
    cfg = _driver_cfg(tmp_path)
    assert 'data_source' not in cfg.training
    assert iterated_dataset_type(cfg, DEV, monkeypatch) is td.SyntheticCocoDataset
