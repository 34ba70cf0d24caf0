"""Golden fixture for the IoU of gpv1_amd.evaluators from the REFERENCE's own utils/bbox_utils.py compute_iou(fmt='xyxy').  Build
container only:

    python tools/gen_golden_detection.py      ->  tests/golden/detection_iou.json   (data only)

The reference module is imported from where it lies through tools/ref_harness.py (its path, its module stand-ins); bbox_utils
imports skimage.draw at module level for its drawing helpers, which compute_iou never touches: a stand-in when the image lacks it.
Boxes are (x, y, w, h) with float32-exact coordinates, x2 = float32(x + w), area >= 0.01: the reference divides by union + 1e-6, so
its IoU differs from inter / union by iou * 1e-6 / union <= 1e-4 on these."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, 'tests', 'golden')
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def import_reference_bbox_utils():
    import ref_harness
    try:
        import skimage.draw  # noqa: F401
    except ImportError:
        sk = ref_harness._mod('skimage')
        sk.draw = ref_harness._mod('skimage.draw')
    sys.path.insert(0, ref_harness.REF)
    import utils.bbox_utils as bu
    return bu


def make_boxes(n, seed=11):
    rs = np.random.RandomState(seed)
    xy = rs.uniform(-0.1, 0.7, size=(n, 2)).astype(np.float32)          # a few boxes start left of / above the image
    wh = rs.uniform(0.1, 0.6, size=(n, 2)).astype(np.float32)           # area >= 0.01
    return np.concatenate([xy, wh], 1)


def main():
    bu = import_reference_bbox_utils()
    a, b = make_boxes(160, 11), make_boxes(160, 12)
    b[:20] = a[:20]                                                     # identical boxes
    b[20:40, :2] = a[20:40, :2] + a[20:40, 2:]                          # touching corners / disjoint
    b[40:60, :2] = a[40:60, :2] + np.float32(0.25) * a[40:60, 2:]       # nested
    b[40:60, 2:] = np.float32(0.5) * a[40:60, 2:]
    b[40:60, 2:] = np.maximum(b[40:60, 2:], np.float32(0.1))
    cases = []
    for p, q in zip(a, b):
        pa = [float(p[0]), float(p[1]), float(np.float32(p[0] + p[2])), float(np.float32(p[1] + p[3]))]
        qa = [float(q[0]), float(q[1]), float(np.float32(q[0] + q[2])), float(np.float32(q[1] + q[3]))]
        iou, inter, union = bu.compute_iou(pa, qa, fmt='xyxy', verbose=True)
        cases.append({'a_xywh': [float(v) for v in p], 'b_xywh': [float(v) for v in q], 'iou': float(iou), 'union': float(union)})
    out = {'source': "utils/bbox_utils.py compute_iou(fmt='xyxy')", 'eps_in_denominator': 1e-6, 'cases': cases}
    path = os.path.join(GOLD, 'detection_iou.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
