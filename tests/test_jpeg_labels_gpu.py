"""The labels of the visualised boxes drawn by the device encoder (libgpv_enc.so, gpv_enc_desc.labels) on the GPU.  The host rule
(gpv1_amd.jpeg_encode.draw_labels_host, then encode_host) is the reference for every byte of every file;
tests/test_jpeg_labels_rule_cpu.py pins that rule to Pillow's drawing."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as K
from tests import jpeg_label_cases as L

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = [(1, 1), (7, 9), (17, 33), (48, 64)]
SETS = ('mixed', 'below32', 'above1', 'odd_bytes')           # odd plate origins and widths: plate edges inside chroma samples


def _encoder(quality, sampling):
    from gpv1_amd.jpeg_encode import DeviceJpegEncoder
    return DeviceJpegEncoder(quality=quality, subsampling=sampling, device=DEV)


def _want(img, boxes, cols, labels, quality, sampling):
    from gpv1_amd import jpeg_encode as E
    return E.encode_host(E.draw_labels_host(E.draw_boxes_host(img.copy(), boxes, cols), boxes, cols, labels), quality, sampling)


@pytest.mark.parametrize('sampling', K.SAMPLINGS)
def test_uint8_pictures_with_labels_are_the_host_rules_files(sampling):
    """every size with every label set in one call of 16 pictures; a picture of the call without labels, and a call without any"""
    sets = L.label_sets()
    cases = [(H, W, name) for H, W in SIZES for name in SETS]
    images = [K.picture('noise', H, W, seed=3) for H, W, _ in cases]
    cols = [L.colours(len(L.BOXES), H) for H, _, _ in cases]
    labels = [sets[name] for _, _, name in cases]
    enc = _encoder(90, sampling)
    files = enc.encode(images, boxes=[L.BOXES] * len(cases), colours=cols, labels=labels)
    for case, img, c, lab, got in zip(cases, images, cols, labels, files):
        assert got == _want(img, L.BOXES, c, lab, 90, sampling), (sampling, case)
    some = enc.encode(images[-2:], boxes=[L.BOXES] * 2, colours=cols[-2:], labels=[None, labels[-1]])
    none = enc.encode(images[-2:], boxes=[L.BOXES] * 2, colours=cols[-2:])
    assert some[1] == files[-1] and some[0] == none[0] and none[1] != files[-1]
    assert none == enc.encode(images[-2:], boxes=[L.BOXES] * 2, colours=cols[-2:], labels=[[None] * len(L.BOXES)] * 2)
    with pytest.raises(ValueError):
        enc.encode(images[:1], boxes=[L.BOXES], colours=cols[:1], labels=[['a']])
    with pytest.raises(ValueError):
        enc.encode(images[:2], boxes=[L.BOXES] * 2, colours=cols[:2], labels=[sets['mixed']])
    with pytest.raises(ValueError):
        enc.encode(images[:1], labels=[sets['mixed']])


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('sampling', K.SAMPLINGS)
def test_pipeline_batches_with_labels_are_the_host_rules_files(sampling, dtype):
    from gpv1_amd import jpeg_encode as E
    from tests.test_jpeg_encode_gpu import _pipeline_batch
    sets = L.label_sets()
    enc = _encoder(90, sampling)
    for H, W in SIZES:
        nested, x = _pipeline_batch(len(SETS), H, W, dtype, seed=H)
        cols = [L.colours(len(L.BOXES), H + i) for i in range(len(SETS))]
        labels = [sets[name] for name in SETS]
        files = enc.encode_batch(nested, MEAN, STD, boxes=[L.BOXES] * len(SETS), colours=cols, labels=labels)
        for b, name in enumerate(SETS):
            img = E.denormalise_host(x[b, 3:3 + H, 3:3 + W, :3], MEAN, STD)
            assert files[b] == _want(img, L.BOXES, cols[b], labels[b], 90, sampling), (sampling, dtype, H, W, name)


def _raw_call(images, boxes, packed, nbytes, sampling, quality=90, G=4096):
    """gpv_enc_encode itself on buffers cut out of larger allocations filled with 255: output, workspace, and each picture's colours +
    length bytes + text -> the files; the guards around all of them are checked"""
    from gpv1_amd import hip_enc
    B = len(images)
    dev_images = [torch.from_numpy(im).to(DEV) for im in images]
    counts = [hip_enc.block_count(im.shape[0], im.shape[1], sampling) for im in images]
    need, capacity = hip_enc.workspace_bytes(B, sum(counts)), hip_enc.file_bound(max(counts))
    ws_all = torch.full((G + need + G,), 255, dtype=torch.uint8, device=DEV)
    out_all = torch.full((G + B * capacity + G,), 255, dtype=torch.uint8, device=DEV)
    sizes, status = torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
    pinned = torch.zeros(B * C.sizeof(hip_enc.EncDesc), dtype=torch.uint8).pin_memory()
    descs = (hip_enc.EncDesc * B).from_address(pinned.data_ptr())
    keep = []
    for d, t, bx, p, n in zip(descs, dev_images, boxes, packed, nbytes):
        d.src, d.H, d.W, d.pitch, d.kind = t.data_ptr(), t.shape[0], t.shape[1], t.shape[1], hip_enc.SRC_U8
        assert len(p) == 4 * len(bx) + n
        col_all = torch.full((G + len(p) + G,), 255, dtype=torch.uint8)
        col_all[G:G + len(p)] = torch.from_numpy(np.asarray(p, np.uint8))
        col_all, bx = col_all.to(DEV), torch.from_numpy(np.asarray(bx, np.float32)).to(DEV).contiguous()
        keep += [col_all, bx]
        d.boxes, d.colours, d.nboxes, d.labels = bx.data_ptr(), col_all.data_ptr() + G, len(bx), n
    hip_enc.encode(descs, B, quality, sampling, ws_all[G:G + need], out_all[G:G + B * capacity], capacity, sizes, status)
    torch.cuda.synchronize()
    assert not status.any()
    for t, n in [(ws_all, need), (out_all, B * capacity)] + [(k, k.numel() - 2 * G) for k in keep[0::2]]:
        assert bool((t[:G] == 255).all()) and bool((t[G + n:] == 255).all())
    for k, p in zip(keep[0::2], packed):
        assert k[G:G + len(p)].cpu().numpy().tobytes() == np.asarray(p, np.uint8).tobytes()            # read, never written
    out = out_all[G:G + B * capacity].cpu().numpy().reshape(B, capacity)
    for i, n in enumerate(sizes.tolist()):
        assert (out[i, n:] == 255).all()
    return [out[i, :n].tobytes() for i, n in enumerate(sizes.tolist())]


@pytest.mark.parametrize('sampling', K.SAMPLINGS)
def test_one_call_of_three_kinds_and_the_guards(sampling):
    """three pictures of different sizes in one call: no labels with garbage in the fourth colour bytes; 32 boxes x 32 characters,
    the 1024-byte extent; length bytes that claim more text than there is (the clamps).  Guards around every buffer stay intact."""
    from gpv1_amd import jpeg_encode as E
    rng = np.random.default_rng(11)
    images = [K.picture('noise', 33, 17, seed=1), K.picture('noise', 48, 64, seed=2), K.picture('ramp', 40, 56)]
    full = rng.uniform(0.05, 0.95, (32, 4)).astype(np.float32)
    texts = [(''.join(chr(c) for c in rng.integers(32, 127, 32)), 'below' if i % 3 == 0 else 'above') for i in range(32)]
    p1, n1 = E.pack_labels(L.colours(32, 1), texts)
    assert n1 == 1024 == 32 * E.MAX_LABEL
    lengths = np.array([3, 0x80 | 127, 2, 40, 1], np.uint8)
    p2 = np.concatenate([np.concatenate([L.colours(5, 2), lengths[:, None]], 1).reshape(-1), np.frombuffer(L.LONG.encode()[:20], np.uint8)])
    garbage = np.concatenate([L.colours(9, 0), rng.integers(0, 256, (9, 1)).astype(np.uint8)], 1).reshape(-1)
    boxes = [L.BOXES, full, L.BOXES[[8, 6, 7, 5, 0]]]
    files = _raw_call(images, boxes, [garbage, p1, p2], [0, n1, 20], sampling)
    assert files[0] == E.encode_host(E.draw_boxes_host(images[0].copy(), L.BOXES, L.colours(9, 0)), 90, sampling)
    assert files[1] == _want(images[1], full, L.colours(32, 1), texts, 90, sampling)
    cols, claimed = E.unpack_labels(p2, 5, 20)
    assert [len(t) for t, _ in claimed] == [3, 17, 0, 0, 0]                                 # 127 -> the 17 bytes that remain; nothing behind them
    assert files[2] == _want(images[2], boxes[2], cols, claimed, 90, sampling)


def test_fourth_colour_byte_is_ignored_without_labels():
    rng = np.random.default_rng(5)
    img = K.picture('noise', 40, 56, seed=4)
    cols = L.colours(9, 7)
    files = [_raw_call([img], [L.BOXES], [np.concatenate([cols, fourth], 1).reshape(-1)], [0], '4:2:0')[0]
             for fourth in (np.zeros((9, 1), np.uint8), np.full((9, 1), 0x85, np.uint8), rng.integers(1, 256, (9, 1)).astype(np.uint8))]
    assert files[0] == files[1] == files[2] == _encoder(90, '4:2:0').encode([img], boxes=[L.BOXES], colours=[cols])[0]


class _Recording:
    """a DeviceJpegEncoder that remembers what visualize asked of it"""

    def __init__(self, enc):
        self.enc, self.calls = enc, []

    def encode_batch(self, nested, mean, std, **kw):
        files = self.enc.encode_batch(nested, mean, std, **kw)
        self.calls.append((nested, kw, files))
        return files


def test_visualize_through_the_real_model_with_labels(tmp_path):
    """the small model's own predictions, labelled: every file is the host rule's for the boxes, colours and texts visualize chose,
    the texts are the scores of index.html with two decimals above the predicted boxes and GT below the ground truth"""
    import re
    import gpv1_amd.ops as ops
    from gpv1_amd import jpeg_encode as E
    from gpv1_amd.misc import AttrDict
    from gpv1_amd.visualize import visualize
    from tests import synth
    from tests.test_model_cpu import build_small, nested, V, B, H, W, Tl, PAD
    ops.RT.set_precise(False)
    torch.manual_seed(0)
    model, _ = build_small(dropout=0.0)
    model.to(DEV).eval()
    images, mask, ids, attn = (t.to(DEV) for t in synth.synth_batch(B, H, W, Tl, V, pad_to=PAD))
    gt = torch.tensor([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.1]], device=DEV)
    targets = [{'task': 'CocoDetection', 'boxes': gt[: 1 + i % 2], 'labels': torch.zeros(1 + i % 2, dtype=torch.long, device=DEV)} for i in range(B)]
    del targets[B - 1]['boxes']
    cfg = AttrDict.wrap({'exp_dir': str(tmp_path), 'training': {'num_vis_samples': B}})
    rec = _Recording(E.DeviceJpegEncoder(quality=100, subsampling='4:4:4', device=DEV))
    out = visualize(model, [(nested(images, mask), (ids, attn), targets)], cfg, 3, 'val', encoder=rec, labels=True)
    (seen, kw, files), = rec.calls
    page = open(os.path.join(out, 'index.html')).read()
    rows = re.findall(r'<tr>(.*?)</tr>', page, flags=re.S)[1:]
    assert len(files) == len(rows) == B and kw['count'] == B
    x = seen.tensors.cpu()
    for b in range(B):
        n_gt = 0 if 'boxes' not in targets[b] else len(targets[b]['boxes'])
        scores = [float(v) for v in re.findall(r'<td>(.*?)</td>', rows[b], flags=re.S)[4].strip('[]').split()]
        k = min(n_gt, 5)
        texts = kw['labels'][b]
        assert len(texts) == 5 + n_gt and texts[5:] == [('GT', 'below')] * n_gt and all(re.fullmatch(r'[01]\.\d\d', t) for t in texts[:5])
        # index.html rounds the same scores to four decimals: two decimals of either differ by at most half a step and that rounding
        assert all(abs(float(t) - scores[i]) <= 0.005 + 0.00005 + 1e-9 for t, i in zip(texts, list(range(k, 5)) + list(range(k))))
        img = E.denormalise_host(x[b, 3:3 + H, 3:3 + W, :3], MEAN, STD)
        want = _want(img, kw['boxes'][b].cpu().numpy(), kw['colours'][b], kw['labels'][b], 100, '4:4:4')
        assert files[b] == want == open(os.path.join(out, f'000003_{b:04d}.jpg'), 'rb').read()
        assert want != E.encode_host(E.draw_boxes_host(img.copy(), kw['boxes'][b].cpu().numpy(), kw['colours'][b]), 100, '4:4:4')
    # labels stay off unless asked for
    plain = _Recording(rec.enc)
    visualize(model, [(nested(images, mask), (ids, attn), targets)], cfg, 4, 'val', encoder=plain)
    assert 'labels' not in plain.calls[0][1]


def test_inference_picture_with_labels_is_the_host_rules_file(tmp_path):
    from gpv1_amd import jpeg_encode as E
    from gpv1_amd.inference import write_vis
    img = K.picture('noise', 40, 56, seed=11)
    boxes = np.array([[0.5, 0.5, 0.5, 0.5], [0.2, 0.3, 0.3, 0.2]], np.float32)
    path = str(tmp_path / 'vis.jpg')
    answer = 'a black and white cat sitting on a kitchen table'
    write_vis(path, img, boxes, DEV, relevance=[0.931, 0.125], answer=answer)
    all_boxes = np.concatenate([np.array([[0.5, 0.5, 1, 1]], np.float32), boxes])
    cols = [(255, 255, 255), (255, 0, 0), (255, 0, 0)]
    assert open(path, 'rb').read() == _want(img, all_boxes, cols, [answer[:32], '0.93', '0.12'], 90, '4:2:0')
    write_vis(path, img, boxes, DEV)                         # and without labels the file of before
    assert open(path, 'rb').read() == E.encode_host(E.draw_boxes_host(img.copy(), boxes, [(255, 0, 0)] * 2), 90, '4:2:0')
