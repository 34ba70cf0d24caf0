"""The pictures the JPEG encoder tests share (CPU rule test and GPU test): sizes, qualities, sampling modes and contents of the grid,
and Pillow's file for a picture.  Everything comes from seeds."""
import io

import numpy as np

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 33), (33, 17), (15, 31), (40, 56), (48, 64), (23, 50)]        # (H, W)
QUALITIES = [5, 50, 75, 90, 100]
SAMPLINGS = ['4:4:4', '4:2:2', '4:2:0']
CONTENTS = ['noise', 'ramp', 'flat', 'checker', 'checker_g', 'binary']


def picture(content, H, W, seed=0):
    rng = np.random.default_rng([seed, H, W, CONTENTS.index(content)])
    yy, xx = np.mgrid[0:H, 0:W]
    if content == 'noise':
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if content == 'ramp':
        return np.stack([(xx * 255) // max(W - 1, 1), (yy * 255) // max(H - 1, 1), ((xx + yy) * 5) % 256], -1).astype(np.uint8)
    if content == 'flat':
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (H, W, 3)).copy()
    if content in ('checker', 'checker_g'):                  # 0 / 255 at pixel pitch 1: runs of more than 15 zeros
        c = (((xx + yy) & 1) * 255).astype(np.uint8)
        return np.stack([c, 255 - c if content == 'checker_g' else c, c], -1)
    return (rng.integers(0, 2, (H, W, 3)) * 255).astype(np.uint8)            # binary noise: the largest categories


def pillow_file(img, quality, subsampling):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', quality=quality, subsampling=subsampling)
    return buf.getvalue()


def grid():
    """(content, H, W, quality) of every case of one sampling mode"""
    return [(c, H, W, q) for c in CONTENTS for (H, W) in SIZES for q in QUALITIES]
