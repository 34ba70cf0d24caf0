"""The cases the label tests share (CPU rule test, GPU test, tools/gen_label_fixtures.py): boxes at the places where the placement
rule takes another path, texts of the lengths that matter, and the same labels drawn by Pillow.  Everything comes from seeds."""
import numpy as np

SIZES = [(1, 1), (7, 9), (13, 14), (17, 33), (40, 56)]       # (H, W): below the plate's height, just above it, odd, several blocks
LONG = ''.join(chr(33 + (7 * i) % 94) for i in range(32))    # 32 different printable characters
# normalised (cx, cy, w, h): the four corners, a point, the whole picture, two that overlap (their labels do too), one off centre
BOXES = np.array([[0.125, 0.125, 0.25, 0.25], [0.875, 0.125, 0.25, 0.25], [0.125, 0.875, 0.25, 0.25], [0.875, 0.875, 0.25, 0.25],
                  [0.5, 0.5, 0.0, 0.0], [0.5, 0.5, 1.0, 1.0], [0.4, 0.5, 0.3, 0.3], [0.45, 0.55, 0.3, 0.3], [0.6, 0.4, 0.35, 0.2]], np.float32)


def colours(n, seed=0):
    """n colours, none of them the plate's"""
    return np.random.default_rng([seed, n]).integers(64, 256, (n, 3)).astype(np.uint8)


def label_sets():
    """{name: one labels list for BOXES}: each length of 0, 1 and 32 above and below (a 32-character plate is wider than every
    picture here), a mix with a box left out, and characters outside 32..126"""
    n = len(BOXES)
    sets = {}
    for where in ('above', 'below'):
        for k, text in ((0, ''), (1, 'W'), (32, LONG)):
            sets[f'{where}{k}'] = [(text, where)] * n
    sets['mixed'] = [('0.97', 'above'), None, ('GT', 'below'), 'cat', ('a longer one, 21 chr', 'below'), ('whole', 'above'), '0.50', ('0.49', 'above'), ('', 'below')]
    sets['odd_bytes'] = [('café', 'above'), ('a\tb', 'below'), ('\x7f~ ', 'above'), None, ('€', 'below'), None, ('\x1f', 'above'), None, ('ok?', 'below')]
    return sets


def pillow_labels(img, boxes, cols, labels):
    """the labels as Pillow draws them into a copy of img: it is told where each plate starts (label_plates) and the text that is
    left after cutting and replacing (label_entries); rectangle and text, clipping and inking are its own"""
    from PIL import Image, ImageDraw, ImageFont
    from gpv1_amd import jpeg_encode as E
    font = ImageFont.load_default_imagefont()
    H, W = img.shape[:2]
    im = Image.fromarray(img.copy())
    draw = ImageDraw.Draw(im)
    for (px, py, n), (text, _), c in zip(E.label_plates(boxes, labels, H, W).tolist(), E.label_entries(labels, len(boxes)), np.asarray(cols).reshape(-1, 3)):
        if n == 0:
            continue
        draw.rectangle([px, py, px + 6 * n + 1, py + 12], fill=(10, 10, 10))
        draw.text((px + 1, py + 1), text.decode('ascii'), font=font, fill=tuple(int(v) for v in c))
    return np.asarray(im)


def fixture_cases():
    """(name, H, W, boxes, packed colours + length bytes + text, text bytes) of tests/golden/jpeg_labels: what the C++ rule is run
    on.  The last two are given as raw bytes: their length bytes claim more text than there is, or more than MAX_LABEL."""
    from gpv1_amd import jpeg_encode as E
    out = []
    for H, W in SIZES:
        for name in ('above1', 'below32', 'mixed', 'odd_bytes'):
            packed, nbytes = E.pack_labels(colours(len(BOXES), H), label_sets()[name])
            out.append((f'{name}_{H}x{W}', H, W, BOXES, packed, nbytes))
    for name, lengths, nbytes in (('overclaim', [3, 0x80 | 127, 2, 40, 1], 20), ('beyond', [40, 0x80 | 40, 5], 96)):
        text = np.frombuffer((LONG * 3).encode()[:nbytes], np.uint8)
        head = np.concatenate([colours(len(lengths), 3), np.array(lengths, np.uint8)[:, None]], 1)
        out.append((f'{name}_40x56', 40, 56, BOXES[[8, 6, 7, 5, 0][:len(lengths)]], np.concatenate([head.reshape(-1), text]), nbytes))
    return out
