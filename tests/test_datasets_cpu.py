"""gpv1_amd.datasets on the CPU: the rules of the reference's dataset classes (crop window, box targets, order of random draws, VQA
answer choice, multitask index mapping), per-sample seeding, and the loader's host half (prefetch, shutdown, worker errors).
The reference's classes cannot run here (no skimage / torchvision), so the rules are pinned by hand-computed values."""
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from tests import coco_tree as CT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    """stand-in for random.Random that records every call; random() returns scripted values (then 0.1)"""

    def __init__(self, script=(), seed=0):
        self.calls, self.script, self.r = [], list(script), random.Random(seed)

    def random(self):
        self.calls.append(('random',))
        return self.script.pop(0) if self.script else 0.1

    def uniform(self, a, b):
        self.calls.append(('uniform', a, b))
        return self.r.uniform(a, b)

    def shuffle(self, x):
        self.calls.append(('shuffle', sorted(x)))
        self.r.shuffle(x)

    def choice(self, x):
        self.calls.append(('choice', list(x)))
        return self.r.choice(x)


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    root = tmp_path_factory.mktemp('coco')
    plan = {k: {'train': ids, 'val': ids[:2]} for k, ids in
            {'cap': [1, 2, 3], 'det': [4], 'cls': [1, 3], 'vqa': [2, 5], 'refcocop': [6]}.items()}
    return CT.make_tree(root, plan)


def test_crop_window_rule():
    from gpv1_amd.datasets import crop_window
    assert crop_window(10.7, 100.2, 3, 40, 120, 160) == (92, 120, 9, 16)          # the worked example: w -> 5, bottom clamped
    with pytest.raises(ValueError, match='empty window'):
        crop_window(165, 10, 20, 20, 120, 160)
    assert crop_window(40, 30, 20, 10, 120, 160) == (28, 42, 36, 64)              # fully inside: 30 - 2, 30 + 12, 40 - 4, 40 + 24
    assert crop_window(50, 60, 2, 1, 120, 160) == (59, 66, 49, 56)                # w, h < 5 -> 5: 60 - 1, 60 + 6, 50 - 1, 50 + 6
    assert crop_window(1, 2, 10, 20, 120, 160) == (0, 26, 0, 13)                  # negative x - 0.2 w and y - 0.2 h clamp to 0
    assert crop_window(150, 100, 30, 40, 120, 160) == (92, 120, 144, 160)         # past the right and bottom edges
    assert crop_window(0.9, 0.9, 5, 5, 120, 160) == (0, 6, 0, 6)                  # int(-0.1) truncates toward zero


@pytest.mark.parametrize('size', [(96, 128), (64, 96)])
def test_oracle_in_float32_stays_inside_the_comparison_rule_on_the_chosen_windows(size):
    """the windows tests/test_datasets_gpu.py compares against the oracle are ones where the oracle itself, held in float32, meets
    the rule of test_device_input_pipeline_vs_oracle against its float64 self (fp32 tolerance)"""
    from oracle import image_oracle as IO
    from tests.datasets_cases import CASES, ORACLE_CASES, make_images, oracle_f32
    imgs = make_images()
    for name in ORACLE_CASES:
        src, (y1, y2, x1, x2), p = CASES[name]
        w = imgs[src][y1:y2, x1:x2]
        steps = np.abs(oracle_f32(w, size, p) - IO.pipeline(w, size, p)).transpose(1, 2, 0) * (255.0 * IO.STD)
        assert (steps <= 1.6).mean() >= 0.995 and steps.max() <= 3.6, (name, float(steps.max()), float((steps <= 1.6).mean()))


def test_box_targets_are_float32_of_the_original_image():
    from gpv1_amd.datasets import box_targets
    b, l = box_targets([[10, 20, 30, 40]], 120, 160)
    assert b.dtype == torch.float32 and l.dtype == torch.long
    assert torch.equal(b, torch.tensor([[25 / 160, 40 / 120, 30 / 160, 40 / 120]], dtype=torch.float32))
    assert torch.equal(l, torch.zeros(1, dtype=torch.long))
    b, l = box_targets([], 120, 160)
    assert b.shape == (0, 4) and l.shape == (0,)


FROZEN = [                                       # draw_params(task, random.Random(seed), True) of the commit before `spec` existed
    ('CocoDetection', 1, {'jitter': 1, 'order': (0, 2, 1, 3), 'brightness': 1.2779469895497861, 'contrast': 1.211019695181291, 'saturation': 0.8040552205915373, 'hue': -0.000912982581611807, 'flip': 0, 'gray': 0}),
    ('CocoDetection', 4, {'jitter': 1, 'order': (0, 1, 2, 3), 'brightness': 0.6825328273845725, 'contrast': 0.9168465940885447, 'saturation': 0.7239778166419282, 'hue': -0.08669698086408202, 'flip': 0, 'gray': 0}),
    ('CocoDetection', 7, {'jitter': 1, 'order': (1, 0, 3, 2), 'brightness': 0.7206793391396015, 'contrast': 1.120747578431883, 'saturation': 0.6579490293340342, 'hue': 0.007176400861337834, 'flip': 0, 'gray': 0}),
    ('CocoClassification', 1, {'jitter': 1, 'order': (0, 2, 1, 3), 'brightness': 1.2779469895497861, 'contrast': 1.211019695181291, 'saturation': 0.8040552205915373, 'hue': -0.000912982581611807, 'flip': 0, 'gray': 1}),
    ('CocoClassification', 4, {'jitter': 1, 'order': (0, 1, 2, 3), 'brightness': 0.6825328273845725, 'contrast': 0.9168465940885447, 'saturation': 0.7239778166419282, 'hue': -0.08669698086408202, 'flip': 0, 'gray': 0}),
    ('CocoClassification', 7, {'jitter': 1, 'order': (1, 0, 3, 2), 'brightness': 0.7206793391396015, 'contrast': 1.120747578431883, 'saturation': 0.6579490293340342, 'hue': 0.007176400861337834, 'flip': 0, 'gray': 0}),
]


@pytest.mark.parametrize('task,seed,want', FROZEN)
def test_draw_params_without_spec_is_unchanged(task, seed, want):
    from gpv1_amd.input_pipeline import draw_params
    assert draw_params(task, random.Random(seed), True) == want
    assert draw_params(task, random.Random(seed), False)['jitter'] == 0
    for other in ('CocoCaptioning', 'CocoVqa', None):                  # the table gives those nothing, and draws nothing
        rec = Recorder()
        assert draw_params(other, rec, True)['jitter'] == 0 and rec.calls == []


GENERIC = [('random',), ('uniform', pytest.approx(0.8), pytest.approx(1.2)), ('uniform', pytest.approx(0.8), pytest.approx(1.2)),
           ('uniform', pytest.approx(0.8), pytest.approx(1.2)), ('shuffle', [0, 1, 2])]
FULL = [('random',), ('uniform', pytest.approx(0.6), pytest.approx(1.4)), ('uniform', pytest.approx(0.6), pytest.approx(1.4)),
        ('uniform', pytest.approx(0.6), pytest.approx(1.4)), ('uniform', pytest.approx(-0.1), pytest.approx(0.1)), ('shuffle', [0, 1, 2, 3])]


@pytest.mark.parametrize('kind,calls', [('cap', GENERIC), ('vqa', GENERIC + [('choice', ['w1'] * 5 + ['w2'] * 3)]),
                                        ('det', FULL + [('random',)]), ('cls', FULL + [('random',), ('random',)]),
                                        ('refcocop', FULL + [('random',)])])
def test_draw_sequence_per_class_and_subset(tree, kind, calls):
    """the exact list of calls on the sample's random.Random: RandomApply, ColorJitter.get_params (a zero component draws nothing
    and is no step), the shuffle of the steps, flip, grey, and -- VQA -- the answer choice after the image draws"""
    from gpv1_amd.datasets import DATASETS
    cls_name, cfg_name, _ = CT.TASKS[kind]
    ds = DATASETS[cls_name](tree[cfg_name], 'train')
    rec = Recorder()
    p, crop, query, target = ds.draw(0, rec, *CT.SIZES[ds.samples[0]['image']['image_id']])
    assert rec.calls == calls
    assert p['jitter'] == 1 and sorted(p['order']) == calls[[c[0] for c in calls].index('shuffle')][1]
    assert target['task'] == cls_name and query == ds.samples[0]['query']
    if kind in ('cap', 'vqa'):
        assert len(p['order']) == 3 and p['hue'] == 0.0 and 0.8 <= p['brightness'] <= 1.2
    val = DATASETS[cls_name](tree[cfg_name], 'val')
    rec = Recorder()
    p, _, _, target = val.draw(0, rec, *CT.SIZES[val.samples[0]['image']['image_id']])
    assert [c[0] for c in rec.calls] == (['choice'] if kind == 'vqa' else [])          # nothing drawn for the image on val
    assert (p['jitter'], p['flip'], p['gray']) == (0, 0, 0)


def test_flip_is_drawn_before_grey(tree):
    from gpv1_amd.datasets import CocoClassification, CocoDetection
    ds = CocoClassification(tree['coco_classification'], 'train')
    p = ds.draw(0, Recorder([0.1, 0.4, 0.5]), 120, 160)[0]              # jitter; 0.4 < 0.5 -> flip; 0.5 >= 0.2 -> colour
    assert (p['jitter'], p['flip'], p['gray']) == (1, 1, 0)
    p = ds.draw(0, Recorder([0.9, 0.6, 0.1]), 120, 160)[0]              # no jitter (nothing else drawn for it); no flip; grey
    assert (p['jitter'], p['flip'], p['gray']) == (0, 0, 1) and p['order'] == (0, 1, 2, 3)
    rec = Recorder([0.9, 0.1])
    p = CocoDetection(tree['coco_detection'], 'train').draw(0, rec, 48, 64)[0]
    assert (p['jitter'], p['flip'], p['gray']) == (0, 0, 1) and rec.calls == [('random',), ('random',)]


def test_refcocop_trains_on_every_subset_named_train(tree):
    from gpv1_amd.datasets import transform_spec, GENERIC_JITTER
    from gpv1_amd.input_pipeline import JITTER
    assert transform_spec('RefCocop', 'train_50') == (JITTER, False, True) and transform_spec('RefCocop', 'val') == (None, False, False)
    assert transform_spec('CocoDetection', 'train_50') == (None, False, False)
    assert transform_spec('CocoCaptioning', 'train') == (GENERIC_JITTER, False, False) == transform_spec('CocoVqa', 'train')
    assert transform_spec('CocoClassification', 'train') == (JITTER, True, True) and transform_spec('CocoClassification', 'test') == (None, False, False)


def test_vqa_answer_choice():
    from gpv1_amd.datasets import vqa_answer
    rec = Recorder()
    got = vqa_answer({'answer': 'c', 'all_answers': {'a': 5, 'b': 3, 'c': 2}}, rec)
    assert rec.calls == [('choice', ['a'] * 5 + ['b'] * 3)] and got in ('a', 'b')
    rec = Recorder()
    assert vqa_answer({'answer': 'c', 'all_answers': {'a': 2, 'b': 1, 'c': 2}}, rec) == 'c' and rec.calls == []


def test_targets_per_class(tree):
    from gpv1_amd.datasets import DATASETS
    det = DATASETS['CocoDetection'](tree['coco_detection'], 'val')
    _, crop, _, t = det.draw(0, random.Random(0), 48, 64)
    assert crop is None and set(t) == {'boxes', 'labels', 'task'} and t['boxes'].dtype == torch.float32 and t['labels'].dtype == torch.long
    x, y, w, h = det.samples[0]['boxes'][0]
    want = torch.tensor([[x + 0.5 * w, y + 0.5 * h, w, h]], dtype=torch.float64).float() / torch.tensor([64, 48, 64, 48], dtype=torch.float32)
    assert torch.equal(t['boxes'], want) and torch.equal(t['labels'], torch.zeros(1, dtype=torch.long))
    cls = DATASETS['CocoClassification'](tree['coco_classification'], 'val')
    _, crop, _, t = cls.draw(0, random.Random(0), 120, 160)
    assert crop == (92, 120, 9, 16) and t == {'answer': 'w4', 'task': 'CocoClassification'}         # one box: the crop, no box target
    cap = DATASETS['CocoCaptioning'](tree['coco_captioning'], 'val')
    assert cap.draw(1, random.Random(0), 45, 61)[3] == {'answer': 'w1 w2 w3', 'task': 'CocoCaptioning'}
    ref = DATASETS['RefCocop'](tree['refcocop'], 'val')
    assert set(ref.draw(0, random.Random(0), 50, 70)[3]) == {'boxes', 'labels', 'task'}
    assert cap.samples[0]['cap_id'] == 100 and det.samples[0]['category_name'] == 'dog'            # other keys stay for the evaluators


def test_an_empty_crop_names_the_sample(tree, tmp_path):
    from gpv1_amd.datasets import CocoClassification
    cfg = json.loads(json.dumps(tree['coco_classification']))
    samples = json.load(open(cfg['samples']['train']))
    samples[0]['boxes'] = [165, 10, 20, 20]
    cfg['samples']['train'] = str(tmp_path / 'train.json')
    json.dump(samples, open(cfg['samples']['train'], 'w'))
    ds = CocoClassification(cfg, 'train')
    with pytest.raises(ValueError, match=r'sample 0 .*COCO_train2014_000000000001\.jpg.*empty window'):
        ds.draw(0, random.Random(0), 120, 160)


def _multitask(tree, subset='train', kinds=('cap', 'det', 'vqa'), **kw):
    from gpv1_amd.datasets import CocoMultitaskDataset
    return CocoMultitaskDataset(CT.learning_datasets(kinds), tree, subset, **kw)


def test_multitask_mapping_lengths_paths_and_errors(tree, tmp_path):
    from gpv1_amd.datasets import CocoMultitaskDataset, CocoDetection
    ds = _multitask(tree)                                                  # lengths 3, 1, 2
    assert len(ds) == 6 and ds.dataset_names == ['coco_cap', 'coco_det', 'coco_vqa'] and list(ds.datasets) == ds.dataset_names
    where = [ds.locate(i) for i in range(6)]
    assert [(d.task, k) for d, k in where] == [('CocoCaptioning', 0), ('CocoCaptioning', 1), ('CocoCaptioning', 2), ('CocoDetection', 0),
                                               ('CocoVqa', 0), ('CocoVqa', 1)]
    assert where[3][0] is ds.datasets['coco_det']
    with pytest.raises(IndexError):
        ds.locate(6)
    assert ds.datasets['coco_cap'].image_path(2) == os.path.join(tree['image_dir'], 'train2014', 'COCO_train2014_000000000003.jpg')
    cfg = json.loads(json.dumps(tree))
    cfg['coco_captioning']['max_samples']['train'] = 2
    cfg['coco_vqa']['max_samples']['train'] = 5                            # more than there are: all of them
    lim = CocoMultitaskDataset(CT.learning_datasets(('cap', 'det', 'vqa')), cfg, 'train')
    assert len(lim) == 5 and [lim.locate(i)[0].task for i in (1, 2)] == ['CocoCaptioning', 'CocoDetection'] and len(lim.datasets['coco_vqa']) == 2
    cfg = json.loads(json.dumps(tree['coco_detection']))
    cfg['read_image'] = False
    with pytest.raises(NotImplementedError, match='not supported'):
        CocoDetection(cfg, 'train')
    cfg['read_image'], cfg['samples']['train'] = True, str(tmp_path / 'nowhere' / 'train.json')
    with pytest.raises(FileNotFoundError, match='nowhere/train.json'):
        CocoDetection(cfg, 'train')
    cfg = json.loads(json.dumps(tree['coco_detection']))
    cfg['image_dir'] = str(tmp_path / 'no_images')
    with pytest.raises(FileNotFoundError, match='no_images'):
        CocoDetection(cfg, 'train')


def test_default_tree_resolves_the_reference_layout():
    from gpv1_amd.config import from_dict
    from gpv1_amd.default_config import default_tree, GROUP_OPTIONS
    cfg = from_dict(default_tree(), ['learning_datasets=all', 'data_dir=/d', 'task_configs.refcocop.train_percent=50'], group_options=GROUP_OPTIONS)
    assert cfg.training.data_source == 'synthetic'
    tc = cfg.task_configs
    assert tc.coco_vqa.samples.testdev == '/d/learning_phase_data/vqa/gpv_split/testdev.json' and tc.refcocop.samples.train == '/d/learning_phase_data/refcocop/train_50.json'
    assert tc.coco_detection.image_dir == '/d/learning_phase_data/coco/images' and tc.coco_captioning.image_size == {'H': 480, 'W': 640}
    assert tc.coco_classification.read_image is True and tc.coco_classification.max_samples.train is None
    for info in cfg.learning_datasets.values():
        assert info.task_config in tc


def _host(loader, groups, epoch=0):
    out = {}
    for hb in loader.host_batches(groups, epoch):
        for i, p, c, q, t in zip(hb.indices, hb.params, hb.crops, hb.queries, hb.targets):
            out[i] = (p, c, q, {k: (v.tolist() if torch.is_tensor(v) else v) for k, v in t.items()})
    loader.close()
    return out


def test_a_samples_draws_depend_on_seed_epoch_and_index_only(tree):
    from gpv1_amd.datasets import DeviceLoader
    from gpv1_amd.train_distr import shard_indices
    ds = _multitask(tree, kinds=('cap', 'cls', 'vqa'), seed=3)             # 3 + 2 + 2 samples
    n = len(ds)
    base = _host(DeviceLoader(ds, 2, device=None, threads=1, prefetch=0), [[0, 1], [2, 3], [4, 5]], epoch=1)
    assert len(base) == 6 and any(p['jitter'] for p, _, _, _ in base.values())
    for bs, world, prefetch in ((3, 1, 1), (2, 2, 0), (3, 2, 1), (1, 1, 1)):
        got = {}
        for rank in range(world):
            idx = shard_indices(n, 1, rank, world)
            got.update(_host(DeviceLoader(ds, bs, device=None, threads=2, prefetch=prefetch),
                             [idx[s:s + bs] for s in range(0, len(idx) - bs + 1, bs)], epoch=1))
        assert got and all(base[i] == v for i, v in got.items() if i in base), (bs, world, prefetch)
    other = _host(DeviceLoader(ds, 2, device=None, threads=1, prefetch=0), [[0, 1], [2, 3], [4, 5]], epoch=2)
    assert [other[i][0] for i in range(6)] != [base[i][0] for i in range(6)]
    reseeded = _host(DeviceLoader(_multitask(tree, kinds=('cap', 'cls', 'vqa'), seed=4), 2, device=None, threads=1, prefetch=0), [[0, 1], [2, 3], [4, 5]], 1)
    assert [reseeded[i][0] for i in range(6)] != [base[i][0] for i in range(6)]


def test_loader_host_half_prefetch_order_shutdown_and_worker_errors(tree, tmp_path):
    import gpv1_amd.hip as hip
    from gpv1_amd.datasets import DeviceLoader
    before = set(threading.enumerate())        # (threads other tests left behind may end meanwhile: count ours)
    ds = _multitask(tree)
    groups = [[5, 0], [3, 1], [2, 4]]
    runs = {}
    for prefetch in (0, 1):
        loader = DeviceLoader(ds, 2, device=None, threads=2, prefetch=prefetch)
        runs[prefetch] = [(hb.indices, hb.paths, hb.parsed.coefs.clone(), list(hb.parsed.starts)) for hb in loader.host_batches(groups)]
        loader.close()
    assert [r[0] for r in runs[1]] == groups == [r[0] for r in runs[0]]
    for a, b in zip(runs[0], runs[1]):
        assert a[1] == b[1] and a[3] == b[3] and torch.equal(a[2], b[2])
    # the coefficients are the host decoder's, file by file
    idx, paths, coefs, starts = runs[1][0]
    for path, st in zip(paths, starts):
        data = open(path, 'rb').read()
        buf = np.empty(int(hip.jpeg_parse(data).coef_count), np.int16)
        hip.jpeg_parse(data, buf)
        assert np.array_equal(coefs[st:st + buf.size].numpy(), buf)
    # an iterator abandoned after one batch: closing it (or dropping it) joins the worker
    loader = DeviceLoader(ds, 2, device=None, threads=2, prefetch=1)
    it = loader.host_batches(groups)
    next(it)
    assert any(t.name.startswith('gpv-loader') for t in threading.enumerate())
    del it
    assert not any(t.name.startswith('gpv-loader') for t in threading.enumerate())
    it = loader.host_batches(groups)
    next(it)
    loader.close()
    assert not set(threading.enumerate()) - before
    # a worker exception (a truncated file) is raised by next(), with the file's path
    cfg = json.loads(json.dumps(tree))
    bad_dir = tmp_path / 'images'
    import shutil
    shutil.copytree(tree['image_dir'], bad_dir)
    victim = bad_dir / 'train2014' / 'COCO_train2014_000000000002.jpg'
    victim.write_bytes(victim.read_bytes()[:60])
    for k in ('coco_captioning', 'coco_detection', 'coco_vqa'):
        cfg[k]['image_dir'] = str(bad_dir)
    loader = DeviceLoader(_multitask(cfg), 2, device=None, threads=2, prefetch=1)
    it = loader.host_batches([[0, 2], [1, 3], [4, 5]])
    assert next(it).indices == [0, 2]
    with pytest.raises(ValueError, match='COCO_train2014_000000000002.jpg'):
        next(it)
    loader.close()
    assert not set(threading.enumerate()) - before


HOST_ONLY = r'''
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1])
import gpv1_amd.hip as hip
from gpv1_amd.jpeg import DeviceJpegDecoder
files = [open(p, 'rb').read() for p in sys.argv[2:]]
dec = DeviceJpegDecoder(threads=2)
pb = dec.parse(files)
assert not pb.lent and len(pb.infos) == len(files)
for f, st, inf in zip(files, pb.starts, pb.infos):
    buf = np.full(int(inf.coef_count), 7, np.int16)
    hip.jpeg_parse(f, buf)
    assert np.array_equal(pb.coefs[st:st + buf.size].numpy(), buf)
room = torch.full((pb.coefs.numel() + 5,), 9, dtype=torch.int16)
pb2 = dec.parse(files, into=room)
assert pb2.lent and pb2.coefs.data_ptr() == room.data_ptr() and torch.equal(pb2.coefs, pb.coefs) and bool((room[-5:] == 9).all())
assert not dec.parse(files, into=torch.empty(3, dtype=torch.int16)).lent
assert not torch.cuda.is_initialized()
print('HOST-ONLY OK')
'''


def test_parse_is_host_only():
    """DeviceJpegDecoder.parse in a fresh process: right coefficients, into pageable memory or a lent buffer, and torch.cuda never
    initialised (the loader's worker thread may run it while the trainer captures a graph)"""
    files = [os.path.join(CT.GOLD, n + '.jpg') for n in ('c420_big', 'gray_q80', 'c422_odd_q60', 'c444_rst_rows')]
    r = subprocess.run([sys.executable, '-c', HOST_ONLY, ROOT] + files, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and 'HOST-ONLY OK' in r.stdout, r.stdout + r.stderr


def test_pipeline_rejects_bad_windows_and_orders_before_any_device_work():
    from gpv1_amd.input_pipeline import DeviceImagePipeline
    pipe = DeviceImagePipeline(size=(8, 8), train=False, device='cpu')
    img = torch.zeros(20, 30, 3, dtype=torch.uint8)
    p0 = dict(jitter=0, order=(0, 1, 2), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, flip=0, gray=0)
    for crop in ((5, 5, 0, 10), (0, 21, 0, 10), (0, 10, -1, 10), (0, 10, 12, 8), (0, 10, 0, 31)):
        with pytest.raises(ValueError, match='empty or outside'):
            pipe([img], params=[p0], crops=[crop])
    with pytest.raises(ValueError, match='9x'):
        pipe([torch.zeros(100, 30, 3, dtype=torch.uint8)], params=[p0], crops=[(0, 80, 0, 30)])
    with pytest.raises(ValueError, match='crops entry per image'):
        pipe([img], params=[p0], crops=[])


class _Stop(Exception):
    pass


def iterated_dataset_type(cfg, device, monkeypatch):
    """the type of the dataset train_worker hands to batches() (the run is stopped there: no training needed)"""
    from gpv1_amd import train_distr as td
    seen = []

    def spy(dataset, *a, **k):
        seen.append(type(dataset))
        raise _Stop()
    monkeypatch.setattr(td, 'batches', spy)
    with pytest.raises(_Stop):
        td.train_worker(cfg, device=device, log=lambda s: None)
    return seen[0]


def test_default_data_source_is_synthetic(tmp_path, monkeypatch):
    """with training.data_source absent the driver still iterates a SyntheticCocoDataset; an unknown source and a missing sample
    file are errors (no silent fallback to synthetic data)"""
    from tests.test_drivers_cpu import _driver_cfg
    from gpv1_amd import train_distr as td
    cfg = _driver_cfg(tmp_path)
    assert 'data_source' not in cfg.training
    assert iterated_dataset_type(cfg, 'cpu', monkeypatch) is td.SyntheticCocoDataset
    assert iterated_dataset_type(_driver_cfg(tmp_path, data_source='synthetic'), 'cpu', monkeypatch) is td.SyntheticCocoDataset
    with pytest.raises(ValueError, match='data_source'):
        td.train_worker(_driver_cfg(tmp_path, data_source='tfrecords'), device='cpu', log=lambda s: None)
    missing = _driver_cfg(tmp_path, data_source='files')
    missing['learning_datasets'] = CT.learning_datasets(('det',))
    missing['task_configs'] = {'coco_detection': {'image_dir': str(tmp_path), 'image_size': {'H': 64, 'W': 96}, 'read_image': True,
                                                  'samples': {'train': str(tmp_path / 'absent.json')}, 'max_samples': {}}}
    with pytest.raises(FileNotFoundError, match='absent.json'):
        td.train_worker(missing, device='cpu', log=lambda s: None)
