"""The device JPEG encoder (libgpv_enc.so, gpv1_amd.jpeg_encode.DeviceJpegEncoder) on the GPU.  Pillow's file is the reference for
every byte where Pillow can write the picture; where it cannot (box outlines, the denormalise path) the host rule encode_host is,
which tests/test_jpeg_encode_rule_cpu.py pins to Pillow."""
import io
import os

import numpy as np
import pytest
import torch

from tests import jpeg_enc_cases as K

pytestmark = pytest.mark.gpu
DEV = 'cuda'
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _encoder(quality, sampling):
    from gpv1_amd.jpeg_encode import DeviceJpegEncoder
    return DeviceJpegEncoder(quality=quality, subsampling=sampling, device=DEV)


@pytest.fixture(scope='module')
def big():
    return K.picture('noise', 480, 640, seed=7)              # 7200 blocks in 4:2:0: the scans cross workgroup and chunk boundaries


@pytest.mark.parametrize('sampling', K.SAMPLINGS)
def test_device_files_are_pillows_files(sampling, big):
    """The whole size / quality / content grid.  Quality belongs to the call, so a sampling mode goes through as one mixed-size batch
    of 60 pictures per quality (offsets between pictures are exercised in every one); the 480 x 640 noise picture joins the batch of
    quality 100."""
    for q in K.QUALITIES:
        cases = [c for c in K.grid() if c[3] == q]
        images = [K.picture(c, H, W) for c, H, W, _ in cases] + ([big] if q == 100 else [])
        files = _encoder(q, sampling).encode(images)
        assert len(files) == len(images)
        for i, (img, got) in enumerate(zip(images, files)):
            want = K.pillow_file(img, q, sampling)
            assert got == want, (sampling, q, cases[i] if i < len(cases) else 'big', len(got), len(want))


def _boxes(rng, n):
    b = rng.uniform(0.05, 0.95, (n, 4)).astype(np.float32)
    b[0] = (0.5, 0.5, 1.5, 1.5)                              # leaves the picture on every side
    b[1] = (0.3, 0.6, 0.0, 0.4)                              # zero width
    return b, rng.integers(0, 256, (n, 3)).astype(np.uint8)


def _pipeline_batch(B, H, W, dtype, seed):
    """a hand-made stem input: normalised pixels in the padded NHWC4 layout, the padding filled with a value that would show"""
    from gpv1_amd.input_pipeline import stem_geometry
    from gpv1_amd.misc import NestedTensor
    Hp, Wp = stem_geometry(H, W)
    g = torch.Generator().manual_seed(seed)
    x = torch.full((B, Hp, Wp, 4), 9.0)
    yy, xx = torch.meshgrid(torch.linspace(-2.2, 2.5, H), torch.linspace(-2.0, 2.6, W), indexing='ij')
    for b in range(B):
        smooth = torch.stack([yy, xx * (1 - 0.3 * b), (yy + xx) / 2], -1)                 # below 0 and above 255 after denormalising
        x[b, 3:3 + H, 3:3 + W, :3] = smooth + 0.05 * torch.randn(H, W, 3, generator=g)
    x = x.to(dtype)
    return NestedTensor(x.to(DEV), torch.zeros(B, H, W, dtype=torch.bool, device=DEV), True), x


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'fp32'])
@pytest.mark.parametrize('B,H,W', [(1, 480, 640), (3, 24, 40)])
def test_pipeline_batches_with_boxes_match_the_host_rule(dtype, B, H, W):
    from gpv1_amd import jpeg_encode as E
    nested, x = _pipeline_batch(B, H, W, dtype, seed=H)
    rng = np.random.default_rng(H + B)
    boxes, colours = zip(*[_boxes(rng, n) for n in ([5, 32, 2][:B])])
    enc = _encoder(90, '4:2:0')
    files = enc.encode_batch(nested, MEAN, STD, boxes=list(boxes), colours=list(colours))
    assert len(files) == B
    for b in range(B):
        img = E.denormalise_host(x[b, 3:3 + H, 3:3 + W, :3], MEAN, STD)
        assert img.min() == 0 and img.max() == 255           # both clamp ends occur
        E.draw_boxes_host(img, boxes[b], colours[b])
        assert files[b] == E.encode_host(img, 90, '4:2:0'), (b, dtype)
    # `count` cuts the batch; without boxes the file is Pillow's for the denormalised picture
    first = enc.encode_batch(nested, MEAN, STD, count=1)
    assert len(first) == 1
    assert first[0] == K.pillow_file(E.denormalise_host(x[0, 3:3 + H, 3:3 + W, :3], MEAN, STD), 90, '4:2:0')


def test_windows_with_unaligned_origin_and_wide_pitch():
    from gpv1_amd import jpeg_encode as E
    whole = torch.from_numpy(K.picture('noise', 61, 77, seed=3)).to(DEV)
    windows = [(5, 38, 3, 20), (1, 2, 0, 77), (0, 61, 76, 77), (7, 60, 11, 64)]            # odd origins: byte offsets 3 * odd
    views = [whole[y1:y2, x1:x2] for y1, y2, x1, x2 in windows]
    assert not views[0].is_contiguous()
    rng = np.random.default_rng(5)
    boxes, colours = zip(*[_boxes(rng, 3) for _ in views])
    for s in K.SAMPLINGS:
        plain = _encoder(75, s).encode(views)
        drawn = _encoder(75, s).encode(views, boxes=list(boxes), colours=list(colours))
        for v, a, b, bx, cl in zip(views, plain, drawn, boxes, colours):
            img = v.cpu().numpy().copy()
            assert a == K.pillow_file(img, 75, s)
            assert b == E.encode_host(E.draw_boxes_host(img, bx, cl), 75, s)


def test_guards_around_output_and_workspace_stay_untouched_and_sizes_are_exact():
    """the raw entry point on buffers cut out of larger allocations filled with 255; a capacity that is too small sets the status
    bit, reports the full size and writes nothing beyond the slot"""
    import ctypes as C
    from gpv1_amd import hip_enc
    images = [K.picture('noise', 33, 17), K.picture('binary', 23, 50), K.picture('flat', 1, 1)]
    want = [K.pillow_file(im, 100, '4:2:0') for im in images]
    B, G = len(images), 4096
    dev_images = [torch.from_numpy(im).to(DEV) for im in images]
    counts = [hip_enc.block_count(im.shape[0], im.shape[1], '4:2:0') for im in images]
    need = hip_enc.workspace_bytes(B, sum(counts))
    for capacity in (hip_enc.file_bound(max(counts)), 1000):
        ws_all = torch.full((G + need + G,), 255, dtype=torch.uint8, device=DEV)
        out_all = torch.full((G + B * capacity + G,), 255, dtype=torch.uint8, device=DEV)
        sizes, status = torch.full((B,), -1, dtype=torch.int32, device=DEV), torch.full((B,), -1, dtype=torch.int32, device=DEV)
        pinned = torch.zeros(B * C.sizeof(hip_enc.EncDesc), dtype=torch.uint8).pin_memory()
        descs = (hip_enc.EncDesc * B).from_address(pinned.data_ptr())
        for d, t in zip(descs, dev_images):
            d.src, d.H, d.W, d.pitch, d.kind = t.data_ptr(), t.shape[0], t.shape[1], t.shape[1], hip_enc.SRC_U8
        hip_enc.encode(descs, B, 100, '4:2:0', ws_all[G:G + need], out_all[G:G + B * capacity], capacity, sizes, status)
        torch.cuda.synchronize()
        assert sizes.tolist() == [len(w) for w in want]
        assert status.tolist() == [hip_enc.STATUS_CAPACITY if len(w) > capacity else 0 for w in want]
        assert [(d.block_base, d.nblocks) for d in descs] == [(sum(counts[:i]), counts[i]) for i in range(B)]
        for t in (ws_all, out_all):
            assert bool((t[:G] == 255).all()) and bool((t[-G:] == 255).all())
        out = out_all[G:G + B * capacity].cpu().numpy().reshape(B, capacity)
        for i, w in enumerate(want):
            n = min(len(w), capacity)
            assert out[i, :n].tobytes() == w[:n]
            assert (out[i, n:] == 255).all()                 # nothing behind the file inside its slot either


def test_round_trip_through_the_projects_decoder(big):
    from PIL import Image
    from gpv1_amd.jpeg import DeviceJpegDecoder
    images = [K.picture('noise', 17, 33), K.picture('ramp', 40, 56), big]
    for s in K.SAMPLINGS:
        files = _encoder(90, s).encode(images)
        decoded = DeviceJpegDecoder(device=DEV, threads=1)(files)
        for f, d in zip(files, decoded):
            assert np.array_equal(d.cpu().numpy(), np.asarray(Image.open(io.BytesIO(f)).convert('RGB')))


def test_a_second_call_on_the_same_workspace_gives_the_same_bytes(big):
    """the bit buffer is OR-ed into: a call that forgot to zero it would show the bits of the call before"""
    enc = _encoder(100, '4:4:4')
    small = [K.picture('binary', 23, 50), K.picture('checker', 16, 16)]
    first = enc.encode([big] + small)
    again = enc.encode([big] + small)
    other = enc.encode(small)                                # the same workspace, other offsets, over the bits of the calls before
    assert first == again
    assert other == first[1:] == [K.pillow_file(im, 100, '4:4:4') for im in small]
    assert enc.launches == 6                                 # noise at quality 100 is longer than one byte per sample: every call was repeated once


def test_cpu_tensors_of_a_pipeline_batch_are_refused():
    from gpv1_amd.misc import NestedTensor
    nested = NestedTensor(torch.zeros(1, 14, 24, 4), torch.zeros(1, 8, 8, dtype=torch.bool), True)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _encoder(90, '4:2:0').encode_batch(nested, MEAN, STD)


def _decode(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert('RGB')).astype(int)


def test_visualize_through_the_real_model_between_graphed_steps(tmp_path):
    """A small model takes three graphed steps on a detection batch of 4 and is then visualised; an identical model took four before.
      * files: four pictures that decode to the batch's extent, an index with four rows;
      * colours: against the same pictures encoded without boxes, every pixel that changed is red, green or blue (the channel of
        its colour above 192, the other two below 64: quality 100 at 4:4:4 moves a pixel by a few levels, tests/test_jpeg_encode_rule_cpu.py
        measures at most 3), all three occur (the fourth sample is shown without ground truth, so its five boxes are blue whatever
        the model predicts), and every ground-truth outline pixel is green (ground truth is drawn last);
      * training is left alone: parameters, optimizer state, the dropout seed word and the RNG states are torch.equal before and
        after, the next step replays its graphs, and its loss is the loss of the model that was never visualised.  The two runs are
        not bitwise repeatable (fp32 atomics in the weight gradients, documented in tests/test_model_gpu.py), and what they compute
        passes through bf16 activations (8 significant bits), so the bound is 2^-7 relative; the torch.equal of the state is the
        sharp half of the statement."""
    import gpv1_amd.ops as ops
    from gpv1_amd import jpeg_encode as E
    from gpv1_amd.misc import AttrDict
    from gpv1_amd.train import FlatTrainer
    from gpv1_amd.visualize import stem_layout, visualize
    from tests import synth
    from tests.test_model_cpu import build_small, nested, V, B, H, W, Tl, PAD
    assert B == 4
    ops.RT.set_precise(False)
    images, mask, ids, attn = (t.to(DEV) for t in synth.synth_batch(B, H, W, Tl, V, pad_to=PAD))
    gt = torch.tensor([[0.5, 0.5, 0.2, 0.3], [0.3, 0.6, 0.1, 0.1]], device=DEV)
    det = [{'task': 'CocoDetection', 'boxes': gt[: 1 + i % 2], 'labels': torch.zeros(1 + i % 2, dtype=torch.long, device=DEV)} for i in range(B)]
    def trained(steps):
        torch.manual_seed(0)
        model, _ = build_small(dropout=0.0)
        model.to(DEV).train()
        model.bert.model.p = 0.0                              # no dropout anywhere: the dropout seed word counts on across the two models
        tr = FlatTrainer(model, lr=1e-3, lr_backbone=1e-4, graphs=True)
        step = lambda: float(tr.train_step(nested(images, mask), (ids, attn), [dict(t) for t in det]))
        return model, tr, step, [step() for _ in range(steps)]
    # the model that is never visualised runs first and to its end: building a model moves ops.RT.static_epoch, which makes every
    # captured body of the process stale
    reference = trained(4)[3][-1]
    model, tr, step, _ = trained(3)
    torch.cuda.synchronize()
    captures, graph_steps = tr.capture_count, tr.graph_steps
    assert captures >= 2 and graph_steps >= 1

    def state():
        torch.cuda.synchronize()
        return [ops.RT.seed_dev.clone(), torch.get_rng_state(), torch.cuda.get_rng_state(), tr.pstep.clone(), tr.P.clone(), tr.M.clone(),
                tr.V.clone()] + [p.detach().clone() for p in model.parameters()] + [b.detach().clone() for b in model.buffers()]
    before = state()
    cfg = AttrDict.wrap({'exp_dir': str(tmp_path), 'training': {'num_vis_samples': 4}})
    enc = E.DeviceJpegEncoder(quality=100, subsampling='4:4:4', device=DEV)
    shown = [dict(t) for t in det]
    del shown[3]['boxes']                                    # a sample without ground truth: its five boxes are all blue
    batch = (nested(images, mask), (ids, attn), shown)
    out = visualize(model, [batch], cfg, 3, 'train', encoder=enc)
    assert model.training and all(torch.equal(a, b) for a, b in zip(before, state()))
    assert sorted(os.listdir(out)) == [f'000003_{i:04d}.jpg' for i in range(4)] + ['index.html']
    assert open(os.path.join(out, 'index.html')).read().count('<tr>') == 5
    plain = enc.encode_batch(stem_layout(nested(images, mask)), MEAN, STD)
    seen = set()
    for i in range(4):
        got, base = _decode(open(os.path.join(out, f'000003_{i:04d}.jpg'), 'rb').read()), _decode(plain[i])
        assert got.shape == base.shape == (H, W, 3)
        changed = np.abs(got - base).max(-1) > 16
        assert changed.any()
        px = got[changed]
        colour = px.argmax(-1)
        rest = np.sort(px, -1)[:, :2]
        assert (px.max(-1) > 192).all() and (rest < 64).all(), (i, px[(px.max(-1) <= 192) | (rest >= 64).any(-1)][:5])
        seen |= set(colour.tolist())
        for x1, y1, x2, y2 in E.box_rects(gt[: 1 + i % 2].cpu().numpy(), H, W) if 'boxes' in shown[i] else ():
            for y in (y1, y2):
                assert (got[y, x1:x2 + 1].argmax(-1) == 1).all() and (got[y, x1:x2 + 1, 1] > 192).all()
            for x in (x1, x2):
                assert (got[y1:y2 + 1, x].argmax(-1) == 1).all() and (got[y1:y2 + 1, x, 1] > 192).all()
    assert seen == {0, 1, 2}
    after = step()
    torch.cuda.synchronize()
    assert tr.capture_count == captures and tr.graph_steps == graph_steps + 1                # replayed, not recaptured
    assert np.isfinite(after) and abs(after - reference) <= 2.0 ** -7 * abs(reference), (after, reference)


def test_inference_picture_is_the_host_rules_file(tmp_path):
    from gpv1_amd import jpeg_encode as E
    from gpv1_amd.inference import preprocess_image, write_vis
    img = K.picture('noise', 40, 56, seed=11)
    boxes = np.array([[0.5, 0.5, 0.5, 0.5], [0.2, 0.3, 0.3, 0.2]], np.float32)
    path = str(tmp_path / 'vis.jpg')
    write_vis(path, img, boxes, DEV)
    seen = E.denormalise_host(preprocess_image(img).permute(1, 2, 0), MEAN, STD)
    assert np.array_equal(seen, img)                         # normalise, then denormalise with rounding: the picture itself
    assert open(path, 'rb').read() == E.encode_host(E.draw_boxes_host(seen, boxes, [(255, 0, 0)] * 2), 90, '4:2:0')
