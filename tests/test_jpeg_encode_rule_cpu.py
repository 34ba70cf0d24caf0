"""The host statement of the JPEG encoding rule (gpv1_amd.jpeg_encode) against Pillow, whole files, and the two rules in front of
it (box outlines, denormalise) and gpv1_amd.visualize on hand-computed cases.  No GPU."""
import io
import os
import re

import numpy as np
import pytest
import torch

from gpv1_amd import jpeg_encode as E
from tests import jpeg_enc_cases as K

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _scan(data):
    """the entropy-coded segment of a file of ours: between the SOS segment and EOI"""
    return data[len(E.header(8, 8, 90, '4:2:0')):-2]


@pytest.mark.parametrize('sampling', K.SAMPLINGS)
def test_host_rule_writes_pillows_file(sampling):
    """every byte of the file -- header, scan, EOI -- over sizes x qualities x contents"""
    bad = []
    for content, H, W, q in K.grid():
        img = K.picture(content, H, W)
        if E.encode_host(img, q, sampling) != K.pillow_file(img, q, sampling):
            bad.append((content, H, W, q))
    assert not bad, bad


def test_the_grid_has_long_zero_runs_and_the_largest_categories():
    """what the contents are for: ZRL symbols (more than 15 zeros in front of a value) and 10-bit AC values do occur in the grid"""
    zz = E.coefficients(K.picture('checker', 8, 8), 5, '4:4:4')[0][..., E.ZIGZAG].reshape(-1, 64)
    assert max(np.diff(np.flatnonzero(np.r_[1, b[1:]])).max() - 1 for b in zz if b[1:].any()) > 15
    assert max(np.abs(c[..., 1:]).max() for c in E.coefficients(K.picture('checker', 17, 33), 100, '4:4:4')) >= 512


def test_a_stuffed_ff_in_the_padded_last_byte():
    """the last byte is filled with 1-bits; where that makes it 0xFF it is followed by 0x00 like any other.  Found by search over
    seeds (a scan ends on a byte boundary minus 0 bits with the right tail about once in 256 files)."""
    found = None
    for seed in range(4000):
        img = K.picture('noise', 8, 8, seed=seed)
        data = E.encode_host(img, 75, '4:4:4')
        if data[-4:] == b'\xff\x00\xff\xd9':
            found = (seed, img, data)
            break
    assert found is not None
    seed, img, data = found
    assert data == K.pillow_file(img, 75, '4:4:4')
    assert _scan(data).count(b'\xff\x00') == _scan(data).count(b'\xff')          # no 0xFF of the scan goes unstuffed


def test_header_alone_at_the_extents():
    for H, W in ((1, 1), (3, 65535), (65535, 2)):
        for s, hv in (('4:4:4', 0x11), ('4:2:2', 0x21), ('4:2:0', 0x22)):
            h = E.header(H, W, 90, s)
            assert len(h) == 623 and h[:4] == b'\xff\xd8\xff\xe0' and h[6:11] == b'JFIF\x00'
            sof = h.index(b'\xff\xc0')
            assert h[sof + 4:sof + 10] == bytes([8, H >> 8, H & 255, W >> 8, W & 255, 3]) and h[sof + 11] == hv
            assert h[-14:] == b'\xff\xda\x00\x0c\x03\x01\x00\x02\x11\x03\x11\x00\x3f\x00'
    small = K.picture('noise', 1, 1)
    assert K.pillow_file(small, 90, '4:2:0').startswith(E.header(1, 1, 90, '4:2:0'))
    wide = np.zeros((1, 65500, 3), np.uint8)                 # the widest picture libjpeg writes; 65535 is checked field by field above
    assert K.pillow_file(wide, 90, '4:2:0').startswith(E.header(1, 65500, 90, '4:2:0'))
    for H, W in ((0, 1), (1, 0), (65536, 1), (1, 65536)):
        with pytest.raises(ValueError):
            E.header(H, W, 90, '4:2:0')
    for q in (0, 101):
        with pytest.raises(ValueError):
            E.header(8, 8, q, '4:2:0')
    with pytest.raises(ValueError):
        E.header(8, 8, 90, '4:1:1')


def _outline(img, colour):
    return {(int(y), int(x)) for y, x in zip(*np.nonzero((img == np.array(colour, np.uint8)).all(-1)))}


def _rect(x1, y1, x2, y2):
    return {(y, x) for y in range(y1, y2 + 1) for x in range(x1, x2 + 1) if y in (y1, y2) or x in (x1, x2)}


def test_draw_boxes_on_hand_computed_pixel_sets():
    H, W = 10, 20
    red, green = (255, 0, 0), (0, 255, 0)
    # a box leaving the picture on every side: clamped to the picture's own border
    img = E.draw_boxes_host(np.zeros((H, W, 3), np.uint8), [[0.5, 0.5, 2.0, 2.0]], [red])
    assert _outline(img, red) == _rect(0, 0, W - 1, H - 1)
    # zero width: x1 = x2 = 0.25 * 20 = 5, y from 0.5 * 10 -+ 0.2 * 10 = 3 .. 7: one column
    img = E.draw_boxes_host(np.zeros((H, W, 3), np.uint8), [[0.25, 0.5, 0.0, 0.4]], [red])
    assert _outline(img, red) == {(y, 5) for y in range(3, 8)}
    # half-way coordinates round to even.  Dyadic numbers, so every fp32 step is exact: on 8 x 16,
    # x1 = (0.40625 - 0.25) * 16 = 2.5 -> 2, x2 = 0.65625 * 16 = 10.5 -> 10, y1 = (0.4375 - 0.125) * 8 = 2.5 -> 2, y2 = 0.5625 * 8 = 4.5 -> 4
    box = [[0.40625, 0.4375, 0.5, 0.25]]
    assert E.box_rects(box, 8, 16).tolist() == [[2, 2, 10, 4]]
    assert E.box_rects([[0.46875, 0.4375, 0.5, 0.25]], 8, 16).tolist() == [[4, 2, 12, 4]]     # 3.5 -> 4 and 11.5 -> 12: to even, not down
    img = E.draw_boxes_host(np.zeros((8, 16, 3), np.uint8), box, [red])
    assert _outline(img, red) == _rect(2, 2, 10, 4)
    # two overlapping boxes: the later one wins where they cross
    a, b = [0.3, 0.5, 0.4, 0.6], [0.5, 0.5, 0.4, 0.6]        # x 2..10 and 6..14, y 2..8 both
    img = E.draw_boxes_host(np.zeros((H, W, 3), np.uint8), [a, b], [red, green])
    assert _outline(img, green) == _rect(6, 2, 14, 8)
    assert _outline(img, red) == _rect(2, 2, 10, 8) - _rect(6, 2, 14, 8)
    with pytest.raises(ValueError):
        E.draw_boxes_host(np.zeros((H, W, 3), np.uint8), np.zeros((33, 4)), np.zeros((33, 3)))
    with pytest.raises(ValueError):
        E.draw_boxes_host(np.zeros((H, W, 3), np.uint8), np.zeros((2, 4)), np.zeros((1, 3)))


def test_denormalise_on_hand_computed_values():
    """255 * (mean + std * x) + 0.5, floored, clamped; mean 0.5 and std 0.25 keep the hand arithmetic exact in fp32"""
    x = np.array([[-2.0, -2.0078125, -10.0], [2.0, 1.9921875, 10.0], [0.0, 0.0078125, float('nan')]], np.float32)
    # -2 -> 0 + 0.5 -> 0;  -2.0078125 -> 255 * -0.001953125 + 0.5 = 0.00195 -> 0;  -10 -> clamp 0
    #  2 -> 255.5 -> 255;   1.9921875 -> 255 * 0.998046875 + 0.5 = 255.00195 -> 255;  10 -> clamp 255
    #  0 -> 127.5 + 0.5 = 128;  0.0078125 -> 255 * 0.501953125 + 0.5 = 128.498 -> 128;  NaN -> 0
    out = E.denormalise_host(x, (0.5, 0.5, 0.5), (0.25, 0.25, 0.25))
    assert out.dtype == np.uint8 and out.tolist() == [[0, 0, 0], [255, 255, 255], [128, 128, 0]]
    # rounding, not truncation: a value that bf16 left just below an integer comes back to it
    v = torch.tensor([(100 / 255 - 0.485) / 0.229]).to(torch.bfloat16)
    exact = 255 * (0.485 + 0.229 * float(v))
    assert int(E.denormalise_host(v.reshape(1, 1).expand(1, 3), MEAN, (0.229,) * 3)[0, 0]) == int(np.floor(exact + 0.5)) == 100 > int(exact)
    # a bf16 tensor and its fp32 values give the same picture
    t = torch.randn(4, 5, 3, generator=torch.Generator().manual_seed(0)).to(torch.bfloat16)
    assert np.array_equal(E.denormalise_host(t, MEAN, STD), E.denormalise_host(t.float().numpy(), MEAN, STD))


class _StubModel:
    """what visualize asks of a model: a device, the mode switch, ground-truth tokens, the greedy forward and the vocabulary"""
    vocab = ['__pad__', '__cls__', '__stop__', 'cat', 'dog']

    def __init__(self, boxes):
        self.vision_token, self.training, self.boxes, self.calls = torch.zeros(1), True, boxes, 0

    def eval(self):
        self.training = False

    def train(self, mode=True):
        self.training = mode

    def encode_answers(self, targets):
        return [['__cls__', t['answer'], '__stop__'] for t in targets], None

    def token_ids_to_words(self, ids):
        return [[self.vocab[int(i)] for i in row] for row in ids]

    def __call__(self, images, queries, answer_token_ids):
        assert not self.training and answer_token_ids is None
        self.calls += 1
        B, Q = images.tensors.shape[0], self.boxes.shape[0]
        logits = torch.zeros(B, Q, 2)
        logits[:, :, 0] = torch.arange(Q, 0, -1).float()                          # query 0 is the most relevant, then 1, ...
        answers = torch.zeros(1, B, 3, len(self.vocab))
        answers[0, :, 0, 1] = answers[0, :, 1, 3] = answers[0, :, 2, 2] = 1                # __cls__ cat __stop__
        return {'pred_relevance_logits': logits, 'pred_boxes': self.boxes.expand(B, Q, 4), 'answer_logits': answers}


def _grey_batches(n_batches, B, H, W, gt, tokenised=False):
    from gpv1_amd.misc import NestedTensor
    x = torch.zeros(B, 3, H, W)                               # normalised 0 = the mean colour: (124, 116, 104)
    for _ in range(n_batches):
        queries = (torch.zeros(B, 5, dtype=torch.long), torch.ones(B, 5)) if tokenised else ['what is this?'] * B
        yield NestedTensor(x, torch.zeros(B, H, W, dtype=torch.bool), True), queries, \
            [{'answer': 'dog', **({'boxes': gt} if gt is not None else {})} for _ in range(B)]


def test_visualize_with_the_host_encoder_and_a_stub_model(tmp_path):
    from PIL import Image
    from gpv1_amd.misc import AttrDict
    from gpv1_amd.visualize import COLUMNS, visualize
    H, W = 32, 48
    # six queries, disjoint boxes in x: 0..5 at x = 4, 12, .. (w = 4 pixels); two ground-truth boxes lower in the picture
    pred = torch.tensor([[(4 + 8 * i) / W, 0.25, 4 / W, 0.25] for i in range(6)])
    gt = torch.tensor([[0.25, 0.75, 0.25, 0.25], [0.75, 0.75, 0.25, 0.25]])
    cfg = AttrDict.wrap({'exp_dir': str(tmp_path), 'training': {'num_vis_samples': 3}})
    model = _StubModel(pred)
    encode = lambda img: E.encode_host(img, 100, '4:4:4')
    out = visualize(model, _grey_batches(4, 2, H, W, gt), cfg, 50, 'val', encoder=encode)
    assert out == os.path.join(str(tmp_path), 'training_visualizations', 'val_000050')
    assert sorted(os.listdir(out)) == ['000050_0000.jpg', '000050_0001.jpg', '000050_0002.jpg', 'index.html']   # cut at num_vis_samples
    assert model.calls == 2 and model.training                # two batches of two were enough; the mode is put back
    page = open(os.path.join(out, 'index.html')).read()
    rows = re.findall(r'<tr>(.*?)</tr>', page)
    assert len(rows) == 4 and all(r.count('<td>') == 5 for r in rows)
    assert [c for c in re.findall(r'<td>(.*?)</td>', rows[0])] == list(COLUMNS)
    cells = re.findall(r'<td>(.*?)</td>', rows[2])
    assert cells[0] == 'what is this?' and 'src="000050_0001.jpg"' in cells[1] and cells[2] == '__cls__ cat __stop__' and cells[3] == '__cls__ dog __stop__'
    assert len(cells[4].strip('[]').split()) == 5
    # the colours.  Tolerance: what Pillow's own round trip (quality 100, 4:4:4) of the same drawn picture gives at those pixels
    grey = E.denormalise_host(np.zeros((H, W, 3), np.float32), MEAN, STD)
    assert grey[0, 0].tolist() == [124, 116, 104]
    red, green, blue = (255, 0, 0), (0, 255, 0), (0, 0, 255)
    boxes = np.concatenate([pred[2:5].numpy(), pred[:2].numpy(), gt.numpy()])               # blue 2..4, red 0..1, green last
    colours = [blue] * 3 + [red] * 2 + [green] * 2
    drawn = E.draw_boxes_host(grey.copy(), boxes, colours)
    round_trip = np.asarray(Image.open(io.BytesIO(K.pillow_file(drawn, 100, '4:4:4'))).convert('RGB')).astype(int)
    tol = int(np.abs(round_trip - drawn.astype(int))[(drawn != grey).any(-1)].max())
    assert tol <= 3
    got = np.asarray(Image.open(os.path.join(out, '000050_0001.jpg')).convert('RGB')).astype(int)
    assert got.shape == (H, W, 3)
    rects = E.box_rects(boxes, H, W)
    for (x1, y1, x2, y2), colour in zip(rects, colours):
        for y, x in _rect(int(x1), int(y1), int(x2), int(y2)):
            assert np.abs(got[y, x] - np.array(colour)).max() <= tol, (y, x, colour, got[y, x])
    assert np.abs(got[H - 1, W - 1] - grey[0, 0].astype(int)).max() <= tol                    # and a pixel no box touches stays grey
    assert {tuple(c) for c in colours} == {red, green, blue}
    # the query with the sixth-largest relevance is not drawn
    x6 = int(E.box_rects(pred[5:6].numpy(), H, W)[0, 0])
    assert np.abs(got[8, x6] - grey[0, 0].astype(int)).max() <= tol
    # without ground truth all five are blue; queries given as (ids, mask) tensors leave the query cell empty
    out = visualize(_StubModel(pred), _grey_batches(1, 3, H, W, None, tokenised=True), cfg, 7, 'train', encoder=encode)
    assert '<tr><td></td><td><img src="000007_0002.jpg"' in open(os.path.join(out, 'index.html')).read()
    got = np.asarray(Image.open(os.path.join(out, '000007_0000.jpg')).convert('RGB')).astype(int)
    for x1, y1, x2, y2 in E.box_rects(pred[:5].numpy(), H, W):
        assert np.abs(got[int(y1), int(x1)] - np.array(blue)).max() <= tol


from tests.test_drivers_cpu import shim, _driver_cfg, _dataset  # noqa: E402,F401  (the CPU shim fixture and the small driver configuration)


def test_driver_with_visualize_off_creates_no_directory(shim, tmp_path):
    from gpv1_amd import train_distr as td
    from gpv1_amd.default_config import default_tree
    from tests import synth
    from tests.test_model_cpu import V
    assert default_tree()['training']['visualize'] == 'off'
    cfg = _driver_cfg(tmp_path, vis_step=1, run_vis_at_launch=True, num_vis_samples=2)
    cfg['exp_dir'] = str(tmp_path)
    cfg['max_steps'] = 2
    torch.manual_seed(0)
    td.train_worker(cfg, dataset=_dataset(synth.make_vocab(V)), device='cpu', log=lambda s: None)
    assert not os.path.exists(os.path.join(str(tmp_path), 'training_visualizations'))
    assert sorted(os.listdir(str(tmp_path))) == ['ckpts']
    bad = _driver_cfg(tmp_path / 'b', visualize='host')
    with pytest.raises(ValueError, match='training.visualize'):
        td.train_worker(bad, dataset=_dataset(synth.make_vocab(V)), device='cpu', log=lambda s: None)
