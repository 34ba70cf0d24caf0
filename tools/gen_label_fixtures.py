"""Writes tests/golden/jpeg_labels: the cases tools/label_host_check.cpp runs the C++ label rule on (its header states the format).
Per case <name>.txt (extents, boxes, colours, length bytes, text), <name>.rgb (a noise picture, raw RGB) and <name>.out (the picture
after draw_boxes_host and draw_labels_host of the numpy rule, gpv1_amd.jpeg_encode).  The cases are tests/jpeg_label_cases.py's.
usage: python tools/gen_label_fixtures.py"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from gpv1_amd import jpeg_encode as E                          # noqa: E402
from tests import jpeg_enc_cases as K, jpeg_label_cases as L  # noqa: E402

OUT = os.path.join(ROOT, 'tests', 'golden', 'jpeg_labels')


def expected(img, boxes, packed, nbytes):
    cols, labels = E.unpack_labels(packed, len(boxes), nbytes)
    return E.draw_labels_host(E.draw_boxes_host(img.copy(), boxes, cols), boxes, cols, labels)


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    for name, H, W, boxes, packed, nbytes in L.fixture_cases():
        img = K.picture('noise', H, W, seed=len(name))
        lines = [f'{H} {W} {len(boxes)} {nbytes}']
        for b, c in zip(boxes, packed[:4 * len(boxes)].reshape(-1, 4)):
            lines.append(' '.join(f'{float(v):.9g}' for v in b) + ' ' + ' '.join(str(int(v)) for v in c))
        lines.append(packed[4 * len(boxes):].tobytes().hex() or '-')
        with open(os.path.join(OUT, name + '.txt'), 'w') as f:
            f.write('\n'.join(lines) + '\n')
        img.tofile(os.path.join(OUT, name + '.rgb'))
        expected(img, boxes, packed, nbytes).tofile(os.path.join(OUT, name + '.out'))
        print('wrote', name)
