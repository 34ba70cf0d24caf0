"""The label rule of the visualised boxes (gpv1_amd.jpeg_encode.label_plates / draw_labels_host, include/gpv_enc.h) against Pillow's
own drawing with its built-in bitmap font, the two committed glyph tables against that font, the C++ statement of the rule on the
fixtures, the descriptor's `labels` field, and gpv1_amd.visualize with labels.  No GPU."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from gpv1_amd import jpeg_encode as E
from tests import abi_probe as probe
from tests import jpeg_enc_cases as K
from tests import jpeg_label_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def test_both_glyph_tables_are_pillows_font():
    from PIL import ImageFont
    from gpv1_amd import jpeg_label_font as F
    font = ImageFont.load_default_imagefont()
    src = open(os.path.join(ROOT, 'gpv-1_amd', 'csrc', 'jpeg_label_font.h')).read()
    c_rows = [[int(v, 16) for v in re.findall(r'0x([0-9a-f]{2})', line)] for line in src.splitlines() if line.lstrip().startswith('{0x')]
    assert len(c_rows) == len(F.ROWS) == 95 and (F.FIRST, F.LAST, F.CELL_W, F.CELL_H) == (32, 126, E.CELL_W, E.CELL_H) == (32, 126, 6, 11)
    for c in range(32, 127):
        mask = font.getmask(chr(c))
        assert mask.size == (6, 11)
        px = np.frombuffer(bytes(mask), np.uint8).reshape(11, 6)
        assert set(np.unique(px)) <= {0, 255}
        want = [int(sum(1 << x for x in range(6) if row[x])) for row in px]
        assert [v & 0x3F for v in F.ROWS[c - 32]] == want and list(F.ROWS[c - 32]) == c_rows[c - 32], chr(c)
        assert all(v & 0x80 or not v & 0x40 for v in F.ROWS[c - 32])

    # A string's mask is its glyphs' masks side by side -- but for the last column of a cell, which the next glyph rewrites where
    # its rows have bit 7 (29 glyphs do: Pillow pastes them one pixel to the left).  Every pair of characters, against Pillow.
    def mask(s):
        m = font.getmask(s)
        return np.frombuffer(bytes(m), np.uint8).reshape(m.size[1], m.size[0]) == 255

    def cell(c):
        return (np.array(F.ROWS[c - 32])[:, None] >> np.arange(6)[None, :]) & 1 == 1
    assert sum(any(v & 0x80 for v in g) for g in F.ROWS) == 29
    for a in range(32, 127):
        for b in range(32, 127):
            want = np.concatenate([cell(a), cell(b)], 1)
            rows = np.array(F.ROWS[b - 32])
            want[rows & 0x80 != 0, 5] = rows[rows & 0x80 != 0] & 0x40 != 0
            assert np.array_equal(mask(chr(a) + chr(b)), want), (chr(a), chr(b))


@pytest.mark.parametrize('H,W', L.SIZES)
def test_host_rule_draws_what_pillow_draws(H, W):
    """every label set over the boxes of the grid, pixel for pixel; Pillow knows the plate's origin and nothing else of the rule"""
    img = K.picture('noise', H, W, seed=1)
    cols = L.colours(len(L.BOXES), H)
    for name, labels in L.label_sets().items():
        got = E.draw_labels_host(img.copy(), L.BOXES, cols, labels)
        assert np.array_equal(got, L.pillow_labels(img, L.BOXES, cols, labels)), (name, H, W)
        if name.endswith('0'):
            assert np.array_equal(got, img)                  # n = 0 draws nothing, not even a 2 x 13 plate
    # one box at a time as well: no label leans on a later one covering its mistakes
    for i in range(len(L.BOXES)):
        for where in ('above', 'below'):
            labels = [('%.2f' % (i / 8), where)]
            assert np.array_equal(E.draw_labels_host(img.copy(), L.BOXES[i:i + 1], cols[i:i + 1], labels),
                                  L.pillow_labels(img, L.BOXES[i:i + 1], cols[i:i + 1], labels)), (i, where, H, W)


def test_the_grid_reaches_every_path_of_the_placement():
    """what the sizes and boxes are for: both fallbacks, the clamp of a picture lower than a plate, the shift at the right edge, a
    plate wider than the picture, two labels that overlap"""
    H, W = 40, 56
    rects = E.box_rects(L.BOXES, H, W)
    above, below = E.label_plates(L.BOXES, [('abcd', 'above')] * 9, H, W), E.label_plates(L.BOXES, [('abcd', 'below')] * 9, H, W)
    assert (above[:, 1] == rects[:, 1] - 13).any() and (above[:, 1] == rects[:, 1] + 1).any()       # room above / not
    assert (below[:, 1] == rects[:, 3] + 1).any() and (below[:, 1] == rects[:, 3] - 13).any()
    assert (above[:, 0] == rects[:, 0]).any() and (above[:, 0] == W - 26).any()                        # pushed in from the right edge
    assert (E.label_plates(L.BOXES, [(L.LONG, 'above')] * 9, H, W)[:, 0] == 0).all() and 6 * 32 + 2 > W
    assert (E.label_plates(L.BOXES, [('a', 'below')] * 9, 7, 9)[:, 1] == 0).all()                        # H < 13: every plate starts at the top
    a, b = above[6], above[7]
    assert abs(a[0] - b[0]) < 26 and abs(a[1] - b[1]) < 13 and (a[:2] != b[:2]).any()


def test_three_placements_computed_by_hand():
    # 40 x 56, box (0.5, 0.5, 0.5, 0.5): x 14..42, y 10..30.  Four characters: w = 26.
    #   above: 10 - 13 < 0 -> inside, py = 11; px = 14, 14 + 26 <= 56.   below: 31 + 13 = 44 > 40 -> py = 30 - 13 = 17.
    assert E.box_rects([[0.5, 0.5, 0.5, 0.5]], 40, 56).tolist() == [[14, 10, 42, 30]]
    assert E.label_plates([[0.5, 0.5, 0.5, 0.5]] * 2, ['0.97', ('0.97', 'below')], 40, 56).tolist() == [[14, 11, 4], [14, 17, 4]]
    # 40 x 56, box (0.875, 0.75, 0.25, 0.25): x 42..(56 -> 55), y 25..35.  Five characters: w = 32.
    #   above: py = 25 - 13 = 12; px = 42, 42 + 32 = 74 > 56 -> px = 24.   32 characters: w = 194 > 56 -> px = 56 - 194 < 0 -> 0.
    #   below: 36 + 13 = 49 > 40 -> py = 35 - 13 = 22.
    box = [[0.875, 0.75, 0.25, 0.25]]
    assert E.box_rects(box, 40, 56).tolist() == [[42, 25, 55, 35]]
    assert E.label_plates(box * 3, ['hello', L.LONG, ('GT', 'below')], 40, 56).tolist() == [[24, 12, 5], [0, 12, 32], [42, 22, 2]]
    # 7 x 9, the whole picture: x 0..8, y 0..6.  above: -13 < 0 -> py = 1, clamped to max(0, 7 - 13) = 0.  below: 7 + 13 > 7 ->
    # py = 6 - 13 = -7 -> 0.  A longer text is cut to 32 characters, None and '' have no plate.
    assert E.label_plates([[0.5, 0.5, 1, 1]] * 4, ['a', ('a', 'below'), None, 'x' * 40], 7, 9).tolist() == [[0, 0, 1], [0, 0, 1], [0, 0, 0], [0, 0, 32]]
    # one whole plate: 40 x 40, box (0.5, 0.25, 0.5, 0.25): x 10..30, y 5..15; below: py = 16, 16 + 13 <= 40.  8 x 13 pixels: a
    # margin of one all round the glyph's 6 x 11 mask, nothing outside
    img = E.draw_labels_host(np.zeros((40, 40, 3), np.uint8), [[0.5, 0.25, 0.5, 0.25]], [(200, 100, 50)], [('1', 'below')])
    assert E.label_plates([[0.5, 0.25, 0.5, 0.25]], [('1', 'below')], 40, 40).tolist() == [[10, 16, 1]]
    px, py = 10, 16
    plate = img[py:py + 13, px:px + 8]
    ink = (plate == np.array([200, 100, 50], np.uint8)).all(-1)
    assert ((plate == 10).all(-1) | ink).all() and not ink[0].any() and not ink[-1].any() and not ink[:, 0].any() and not ink[:, -1].any()
    from PIL import ImageFont
    assert np.array_equal(ink[1:12, 1:7], np.frombuffer(bytes(ImageFont.load_default_imagefont().getmask('1')), np.uint8).reshape(11, 6) == 255)
    assert (img[:py] == 0).all() and (img[py + 13:] == 0).all() and (img[:, :px] == 0).all() and (img[:, px + 8:] == 0).all()


def test_entries_packing_and_refusals():
    assert E.label_entries(['aé\n', ('x' * 40, 'below'), None, ''], 4) == [(b'a??', False), (b'x' * 32, True), (b'', False), (b'', False)]
    for bad in (['a'], ['a', 'b', 'c'], [('a', 'left'), 'b'], [5, 'b'], [('a',), 'b']):
        with pytest.raises((ValueError, TypeError)):
            E.label_entries(bad, 2)
    with pytest.raises(ValueError):
        E.draw_labels_host(np.zeros((8, 8, 3), np.uint8), np.zeros((2, 4)), np.zeros((2, 3)), ['a'])
    packed, n = E.pack_labels([(1, 2, 3), (4, 5, 6), (7, 8, 9)], ['ab', None, ('c', 'below')])
    assert packed.tolist() == [1, 2, 3, 2, 4, 5, 6, 0, 7, 8, 9, 0x81, 97, 98, 99] and n == 3
    cols, labels = E.unpack_labels(packed, 3, 3)
    assert cols.tolist() == [[1, 2, 3], [4, 5, 6], [7, 8, 9]] and labels == [('ab', 'above'), ('', 'above'), ('c', 'below')]
    # length bytes that claim too much: the offset stops at the text's end, the count at MAX_LABEL and at what remains
    over = np.array([0, 0, 0, 2, 0, 0, 0, 0x80 | 100, 0, 0, 0, 3] + list(b'abcdefgh'), np.uint8)
    assert E.unpack_labels(over, 3, 8)[1] == [('ab', 'above'), ('cdefgh', 'below'), ('', 'above')]
    with pytest.raises(ValueError):
        E.unpack_labels(over, 3, 9)


def test_cpp_rule_on_the_fixtures(tmp_path):
    """tools/label_host_check.cpp, plain g++: the C++ statement of the rule (the text the kernel compiles) on every fixture, and the
    fixtures are still what the numpy rule writes"""
    gold = os.path.join(ROOT, 'tests', 'golden', 'jpeg_labels')
    cases = L.fixture_cases()
    assert sorted(os.listdir(gold)) == sorted(f'{c[0]}.{ext}' for c in cases for ext in ('out', 'rgb', 'txt'))
    for name, H, W, boxes, packed, nbytes in cases:
        img = np.fromfile(os.path.join(gold, name + '.rgb'), np.uint8).reshape(H, W, 3)
        cols, labels = E.unpack_labels(packed, len(boxes), nbytes)
        want = E.draw_labels_host(E.draw_boxes_host(img.copy(), boxes, cols), boxes, cols, labels)
        assert np.fromfile(os.path.join(gold, name + '.out'), np.uint8).tobytes() == want.tobytes(), name
    exe = str(tmp_path / 'label_host_check')
    subprocess.run(['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-I', os.path.join(ROOT, 'gpv-1_amd', 'csrc'),
                    os.path.join(ROOT, 'tools', 'label_host_check.cpp'), '-o', exe], check=True)
    run = subprocess.run([exe, gold], capture_output=True, text=True)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-1000:]
    assert f'PASSED: {len(cases)} cases, 0 failures' in run.stdout


def test_descriptor_keeps_its_size_and_refuses_bad_label_counts():
    mod = probe.module('enc')
    assert ctypes.sizeof(mod.EncDesc) == 80 and mod.EncDesc.labels.offset == 76 and mod.EncDesc.labels.size == 4
    assert mod.MAX_LABEL == E.MAX_LABEL == 32
    assert re.search(r'#define GPV_ENC_MAX_LABEL 32\b', open(probe.header_path('enc')).read())
    lib = ctypes.CDLL(probe.built('enc'))
    lib.gpv_enc_encode.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p,
                                   ctypes.c_int64, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]

    def refused(nboxes, labels):
        d = (mod.EncDesc * 1)()
        d[0].src, d[0].H, d[0].W, d[0].pitch, d[0].kind = 4096, 16, 16, 16, mod.SRC_U8
        d[0].nboxes, d[0].labels = nboxes, labels
        if nboxes:
            d[0].boxes = d[0].colours = 4096
        before = bytes(d)
        status = lib.gpv_enc_encode(d, 1, 90, 2, 4096, 1 << 20, 4096, 1 << 16, 4096, 4096, None)
        return status == 1 and bytes(d) == before            # hipErrorInvalidValue, and not a byte of the descriptor written
    assert refused(2, -1) and refused(2, 2 * 32 + 1) and refused(0, 1) and refused(32, 32 * 32 + 1)
    # the Python mirror names the reason first
    d = (mod.EncDesc * 1)()
    d[0].src, d[0].H, d[0].W, d[0].pitch, d[0].nboxes, d[0].labels = 4096, 16, 16, 16, 1, 33
    with pytest.raises(ValueError, match='label bytes'):
        mod.encode(d, 1, 90, '4:2:0', None, None, 1 << 16, None, None)


from tests.test_jpeg_encode_rule_cpu import _StubModel, _grey_batches  # noqa: E402  (the stub model and its grey batches)


def test_visualize_with_labels_writes_the_host_rules_files(tmp_path):
    from gpv1_amd.misc import AttrDict
    from gpv1_amd.visualize import label_lists, visualize
    H, W = 32, 48
    pred = torch.tensor([[(4 + 8 * i) / W, 0.5, 4 / W, 0.25] for i in range(6)])
    gt = torch.tensor([[0.25, 0.75, 0.25, 0.25], [0.75, 0.75, 0.25, 0.25]])
    encode = lambda img: E.encode_host(img, 100, '4:4:4')
    grey = E.denormalise_host(np.zeros((H, W, 3), np.float32), MEAN, STD)
    # the stub's relevance logits are (Q - i, 0) for query i: softmax's first entry, as visualize computes it
    logits = torch.zeros(6, 2)
    logits[:, 0] = torch.arange(6, 0, -1).float()
    scores = logits.softmax(-1)[:, 0].numpy()
    assert label_lists(scores[:5], 2) == ['%.2f' % scores[i] for i in (2, 3, 4, 0, 1)] + [('GT', 'below')] * 2
    assert label_lists(scores[:5], 0) == ['%.2f' % s for s in scores[:5]] and label_lists(scores[:5], 40)[5:] == [('GT', 'below')] * 27
    for with_gt in (True, False):
        boxes = np.concatenate([pred[2:5].numpy(), pred[:2].numpy(), gt.numpy()]) if with_gt else pred[:5].numpy()
        colours = [(0, 0, 255)] * 3 + [(255, 0, 0)] * 2 + [(0, 255, 0)] * 2 if with_gt else [(0, 0, 255)] * 5
        texts = ['%.2f' % scores[i] for i in ((2, 3, 4, 0, 1) if with_gt else range(5))] + ([('GT', 'below')] * 2 if with_gt else [])
        drawn = E.draw_boxes_host(grey.copy(), boxes, colours)
        plain, labelled = encode(drawn), encode(E.draw_labels_host(drawn.copy(), boxes, colours, texts))
        assert plain != labelled
        for labels, want in ((True, labelled), (False, plain)):
            cfg = AttrDict.wrap({'exp_dir': str(tmp_path / f'{with_gt}{labels}'), 'training': {'num_vis_samples': 3}})
            out = visualize(_StubModel(pred), _grey_batches(2, 2, H, W, gt if with_gt else None), cfg, 9, 'val', encoder=encode, labels=labels)
            files = sorted(f for f in os.listdir(out) if f.endswith('.jpg'))
            assert len(files) == 3
            for f in files:
                assert open(os.path.join(out, f), 'rb').read() == want, (with_gt, labels, f)
    cfg = AttrDict.wrap({'exp_dir': str(tmp_path / 'default'), 'training': {'num_vis_samples': 1}})
    out = visualize(_StubModel(pred), _grey_batches(1, 1, H, W, gt), cfg, 9, 'val', encoder=encode)                 # labels default to off
    assert open(os.path.join(out, '000009_0000.jpg'), 'rb').read() == encode(E.draw_boxes_host(grey.copy(), np.concatenate([pred[2:5].numpy(), pred[:2].numpy(), gt.numpy()]),
                                                                                                 [(0, 0, 255)] * 3 + [(255, 0, 0)] * 2 + [(0, 255, 0)] * 2))
    from gpv1_amd.default_config import default_tree
    assert default_tree()['training']['vis_labels'] is False


def test_inference_lists_put_the_answer_on_a_white_frame_first():
    from gpv1_amd.inference import vis_lists
    boxes = np.array([[0.5, 0.5, 0.5, 0.5], [0.2, 0.3, 0.3, 0.2]], np.float32)
    b, c, l = vis_lists(boxes)
    assert np.array_equal(b, boxes) and c == [(255, 0, 0)] * 2 and l is None
    b, c, l = vis_lists(boxes, relevance=[0.987, 0.5], answer='a very long answer that goes on and on and on')
    assert b.tolist() == [[0.5, 0.5, 1, 1]] + boxes.tolist() and c == [(255, 255, 255)] + [(255, 0, 0)] * 2
    assert l == ['a very long answer that goes on and on and on', '0.99', '0.50']
    # the frame is the picture's border and its label lands inside the top left corner, cut to 32 characters
    assert E.box_rects(b[:1], 40, 56).tolist() == [[0, 0, 55, 39]] and E.label_plates(b, l, 40, 56)[0].tolist() == [0, 1, 32]
    with pytest.raises(ValueError):
        vis_lists(boxes, relevance=[0.5])
