"""TEST HELPER (not a test): the source images and windows tests/test_datasets_gpu.py runs the windowed input pipeline on."""
import numpy as np

P0 = dict(jitter=0, order=(0, 1, 2, 3), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, flip=0, gray=0)
SHAPES = {'a': (150, 131), 'b': (60, 90), 'c': (120, 160), 'd': (300, 420), 'e': (97, 128)}

# name -> (source image, window (y1, y2, x1, x2), params)
CASES = {
    'origin': ('a', (0, 100, 0, 90), P0),
    'odd_x1': ('b', (3, 46, 13, 76), dict(P0, jitter=1, order=(0, 1, 2, 3), brightness=1.3, contrast=0.7, saturation=1.2, hue=0.05, flip=1)),
    'downscale_all_borders': ('d', (25, 275, 10, 410), dict(P0, jitter=1, order=(3, 2, 1, 0), brightness=0.65, contrast=1.35, saturation=0.6, hue=-0.1)),
    'worked_example_7x28': ('c', (92, 120, 9, 16), P0),
    'bottom_right': ('e', (40, 97, 61, 128), dict(P0, flip=1, gray=1)),
    'bottom_right_jitter': ('e', (40, 97, 61, 128), dict(P0, jitter=1, order=(1, 0, 2, 3), brightness=0.9, contrast=1.2, saturation=1.1, hue=0.02)),
    'contrast_flip_grey': ('a', (30, 141, 21, 120), dict(P0, jitter=1, order=(1, 3, 0, 2), brightness=1.1, contrast=1.1, saturation=1.4, hue=0.08, flip=1, gray=1)),
    'three_steps': ('b', (3, 58, 10, 85), dict(P0, jitter=1, order=(2, 0, 1), brightness=0.85, contrast=1.15, saturation=0.9)),
    'one_row': ('b', (40, 41, 0, 90), P0),
    'one_column': ('b', (0, 60, 33, 34), dict(P0, jitter=1, order=(1, 0, 2), brightness=1.1, contrast=0.9, saturation=1.1)),
}
# the windows compared against oracle/image_oracle.py: those on which that oracle, re-run in float32 (oracle_f32 below), stays inside the
# comparison rule against itself (tests/test_datasets_cpu.py checks it) -- a float32 pipeline cannot be asked for more; e.g. rows 7:50,
# columns 13:80 of image b at 64 x 96 is not one: a hue-sector boundary there moves one value by four uint8 steps between fp32 and fp64
ORACLE_CASES = ('origin', 'odd_x1', 'downscale_all_borders', 'worked_example_7x28', 'bottom_right', 'bottom_right_jitter', 'contrast_flip_grey', 'three_steps')


def make_images(seed=3):
    """smooth images + noise, as test_device_input_pipeline_vs_oracle builds them (a pure-noise image makes every truncation a coin flip)"""
    rs = np.random.RandomState(seed)
    out = {}
    for k, (ih, iw) in SHAPES.items():
        yy, xx = np.mgrid[0:ih, 0:iw]
        base = np.stack([127 + 100 * np.sin(yy / 9.0 + c) * np.cos(xx / 13.0 - c) for c in range(3)], -1)
        out[k] = np.clip(base + rs.randn(ih, iw, 3) * 12, 0, 255).astype(np.uint8)
    return out


def oracle_f32(img, size, p):
    """oracle/image_oracle.py's pipeline with every intermediate held in float32: what ANY float32 implementation of the same
    formulas may differ from the float64 oracle by"""
    from scipy import ndimage as ndi
    from oracle import image_oracle as IO
    F = np.float32
    a = np.asarray(img).astype(F)
    factors = np.array([a.shape[0] / size[0], a.shape[1] / size[1], 1.0])
    sigma = np.maximum(0.0, (factors - 1.0) / 2.0)
    if sigma.max() > 0:
        a = ndi.gaussian_filter(a, sigma, mode='mirror').astype(F)
    a = ndi.zoom(a, 1.0 / factors, order=1, mode='mirror', grid_mode=True).astype(F)
    x = np.floor(np.clip(a, 0, 255)).astype(F)

    def r8(v):
        return np.rint(np.clip(v, F(0), F(255))).astype(F)
    for op in (p['order'] if p['jitter'] else ()):
        if op == 0:
            x = r8(x * F(p['brightness']))
        elif op == 1:
            m = F(np.floor(IO.grey(x.astype(np.uint8)).mean() + 0.5))
            x = r8(m + F(p['contrast']) * (x - m))
        elif op == 2:
            l = IO.grey(x.astype(np.uint8))[..., None].astype(F)
            x = r8(l + F(p['saturation']) * (x - l))
        else:
            r, g, b = (x[..., i] / F(255) for i in range(3))
            mx, mn = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
            df = mx - mn
            safe = np.where(df > 0, df, F(1))
            h = np.where(mx == r, (g - b) / safe, np.where(mx == g, F(2) + (b - r) / safe, F(4) + (r - g) / safe)) / F(6)
            h = np.where(df > 0, h - np.floor(h), F(0)).astype(F)
            s = np.where(mx > 0, df / np.where(mx > 0, mx, F(1)), F(0)).astype(F)
            h = h + F(p['hue'])
            h = h - np.floor(h)
            h6 = h * F(6)
            i = np.floor(h6).astype(np.int64) % 6
            f = h6 - np.floor(h6)
            pp, q, t = mx * (1 - s), mx * (1 - s * f), mx * (1 - s * (1 - f))
            x = r8(np.stack([np.choose(i, [mx, q, pp, pp, t, mx]), np.choose(i, [t, mx, mx, q, pp, pp]),
                             np.choose(i, [pp, pp, t, mx, mx, q])], -1).astype(F) * F(255))
    if p['flip']:
        x = x[:, ::-1]
    x = x.astype(np.float64)
    if p['gray']:
        l = IO.grey(x.astype(np.uint8))
        x = np.stack([l, l, l], -1)
    return ((x / 255.0 - IO.MEAN) / IO.STD).transpose(2, 0, 1)
