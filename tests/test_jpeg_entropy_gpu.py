"""JPEG entropy decoding on the device (csrc/jpeg_huff.hip through gpv1_amd.hip_huff and DeviceJpegDecoder(entropy='device')): the
coefficients against the host parser's, bit for bit, and the decoded images against Pillow's and against the host path's."""
import ctypes as C
import glob
import io
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg')
FILES = sorted(glob.glob(os.path.join(GOLD, '*.jpg')))
PLAIN = [f for f in FILES if '_rst' not in os.path.basename(f)]
DEV = 'cuda'


def as_rgb(a):
    return a if a.ndim == 3 else np.repeat(a[..., None], 3, 2)


def device_coefficients(datas, S):
    """gpv_huff_prepare + gpv_huff_decode on a batch of files, without the decoder class -> (per file int16 arrays, status [n, 2])"""
    from gpv1_amd import hip_huff
    heads = [hip_huff.prepare(d) for d in datas]
    assert all(h[3] == 'device' for h in heads)
    caps = [h[2] for h in heads]
    streams = np.zeros(sum(caps), np.uint8)
    at = np.concatenate([[0], np.cumsum(caps)]).astype(np.int64)
    for k, d in enumerate(datas):
        hip_huff.prepare(d, streams[at[k]:at[k + 1]], heads[k][1])
    counts = [int(h[0].coef_count) for h in heads]
    cat = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    sdev = torch.from_numpy(streams).to(DEV)
    coefs = torch.full((int(cat[-1]) + 64,), 0x5A5A, dtype=torch.int16, device=DEV)      # not zero: the launch zeroes; 64 guard elements
    status = torch.full((len(datas), 2), -1, dtype=torch.int32, device=DEV)
    descs = (hip_huff.HuffDesc * len(datas))()
    for k, h in enumerate(heads):
        C.memmove(C.byref(descs[k]), C.byref(h[1]), C.sizeof(h[1]))
        descs[k].stream = sdev.data_ptr() + int(at[k])
        descs[k].coefs = coefs.data_ptr() + 2 * int(cat[k])
        descs[k].status = status.data_ptr() + 8 * k
    raw = torch.frombuffer(bytearray(bytes(descs)), dtype=torch.uint8).to(DEV)
    max_nbits = max(h[1].nbits for h in heads)
    ws = torch.empty(hip_huff.workspace_bytes(len(datas), S, max_nbits), dtype=torch.uint8, device=DEV)
    hip_huff.decode(raw, len(datas), S, max_nbits, ws)
    torch.cuda.synchronize()
    out = coefs.cpu().numpy()
    assert np.all(out[cat[-1]:] == 0x5A5A)
    return [out[cat[k]:cat[k + 1]] for k in range(len(datas))], status.cpu().numpy()


def host_coefficients(d):
    import gpv1_amd.hip as hip
    ref = np.zeros(hip.jpeg_parse(d).coef_count, np.int16)
    hip.jpeg_parse(d, ref)
    return ref


@pytest.mark.parametrize('S', [64, 1024])
def test_device_coefficients_equal_the_host_parsers_on_the_fixtures_as_one_batch(S):
    from gpv1_amd import jpeg_entropy as E
    datas = [open(f, 'rb').read() for f in PLAIN]
    got, status = device_coefficients(datas, S)
    for f, d, g, st in zip(PLAIN, datas, got, status):
        assert np.array_equal(g, host_coefficients(d)), os.path.basename(f)
        n_sub = max(1, -(-E.prepare_host(d)['nbits'] // S))
        assert st[0] == 0 and 1 <= st[1] <= n_sub, (os.path.basename(f), st)
    if S == 64:                                                                   # the kernel's passes are the rule's
        big = [k for k, f in enumerate(PLAIN) if f.endswith('c420_big.jpg')][0]
        assert status[big][1] == E.decode_subsequences_host(E.prepare_host(datas[big]), 64)[1] > 10


def test_decoder_on_all_fixtures_equals_the_goldens_and_counts_both_routes():
    from gpv1_amd.jpeg import DeviceJpegDecoder
    exp = np.load(os.path.join(GOLD, 'expected.npz'))
    dec = DeviceJpegDecoder(entropy='device')
    outs = dec([open(f, 'rb').read() for f in FILES])
    torch.cuda.synchronize()
    dec.check_status()
    for f, o in zip(FILES, outs):
        e = as_rgb(exp[os.path.basename(f)[:-4]])
        assert o.dtype == torch.uint8 and tuple(o.shape) == e.shape
        assert np.array_equal(o.cpu().numpy(), e), os.path.basename(f)
    assert (dec.stats['device'], dec.stats['host']) == (11, 3) and dec.stats['bytes_uploaded'] > 0
    host = DeviceJpegDecoder()
    host([open(f, 'rb').read() for f in FILES])
    torch.cuda.synchronize()
    assert (host.stats['device'], host.stats['host']) == (0, 14)
    assert host.stats['bytes_uploaded'] == 2 * sum(int(host_coefficients(open(f, 'rb').read()).size) for f in FILES)


def test_random_files_property():
    """40 freshly encoded files of random size (1..200 pixels a side): grey, 4:4:4, 4:2:2 and 4:2:0, quality 5..99, default and
    optimised tables, smooth and noisy content, no restart markers -- all on the device route, every one bit-exact against Pillow"""
    from PIL import Image
    from gpv1_amd.jpeg import DeviceJpegDecoder
    r = np.random.RandomState(17)
    files, exp, kinds = [], [], set()
    for i in range(40):
        h, w = int(r.randint(1, 201)), int(r.randint(1, 201))
        grey = i % 7 == 3
        base = r.rand(h, w, 1 if grey else 3) * 255
        if i % 3 == 0:                                                            # smooth content: long zero runs, EOB-heavy blocks
            yy, xx = np.mgrid[0:h, 0:w]
            base = np.stack([(xx * 3 + yy * 2 + 40 * c) % 256 for c in range(base.shape[2])], -1).astype(np.float64)
        img = np.clip(base, 0, 255).astype(np.uint8)
        kw = dict(quality=int(r.randint(5, 100)), optimize=bool(i % 2))
        if not grey:
            kw['subsampling'] = i % 3 if i < 6 else int(r.randint(0, 3))
        kinds.add('grey' if grey else kw['subsampling'])
        buf = io.BytesIO()
        Image.fromarray(img[..., 0] if grey else img, 'L' if grey else 'RGB').save(buf, 'JPEG', **kw)
        files.append(buf.getvalue())
        exp.append(as_rgb(np.asarray(Image.open(io.BytesIO(buf.getvalue())))))
    assert kinds == {'grey', 0, 1, 2}
    dec = DeviceJpegDecoder(threads=4, entropy='device')
    outs = dec(files[:25])
    torch.cuda.synchronize()
    dec.check_status()
    outs += dec(files[25:])
    torch.cuda.synchronize()
    dec.check_status()
    assert (dec.stats['device'], dec.stats['host']) == (40, 0)
    for i, (o, e) in enumerate(zip(outs, exp)):
        assert tuple(o.shape) == e.shape and np.array_equal(o.cpu().numpy(), e), (i, e.shape)


def test_dataset_sized_files_at_the_default_subsequence_length():
    from PIL import Image
    from gpv1_amd.jpeg import DeviceJpegDecoder
    r = np.random.RandomState(5)
    files, exp = [], []
    for h, w, sub, q in ((480, 640, 2, 90), (640, 427, 2, 75)):
        yy, xx = np.mgrid[0:h, 0:w]
        img = np.stack([128 + 100 * np.sin(xx / 17.0) * np.cos(yy / 23.0), (xx * 255.0 / w), (yy * 255.0 / h)], -1) + r.randn(h, w, 3) * 12
        buf = io.BytesIO()
        Image.fromarray(np.clip(img, 0, 255).astype(np.uint8)).save(buf, 'JPEG', quality=q, subsampling=sub)
        files.append(buf.getvalue())
        exp.append(np.asarray(Image.open(io.BytesIO(buf.getvalue()))))
    dec = DeviceJpegDecoder(threads=2, entropy='device')
    assert dec.subseq_bits == 1024
    outs = dec(files)
    torch.cuda.synchronize()
    dec.check_status()
    assert dec.stats['device'] == 2
    for o, e in zip(outs, exp):
        assert np.array_equal(o.cpu().numpy(), e)
    got, status = device_coefficients(files, 1024)                                # and the coefficients themselves
    for d, g in zip(files, got):
        assert np.array_equal(g, host_coefficients(d))
    from gpv1_amd import hip_huff
    assert status[:, 0].tolist() == [0, 0]
    assert all(1 <= st[1] <= -(-hip_huff.prepare(d)[1].nbits // 1024) for d, st in zip(files, status))


def test_one_pixel_and_a_stream_shorter_than_one_subsequence():
    from PIL import Image
    from gpv1_amd import hip_huff
    from gpv1_amd.jpeg import DeviceJpegDecoder
    files, exp = [], []
    for img in (np.array([[[200, 30, 90]]], np.uint8), np.full((8, 8, 3), 77, np.uint8)):
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, 'JPEG', quality=80)
        files.append(buf.getvalue())
        exp.append(np.asarray(Image.open(io.BytesIO(buf.getvalue()))))
    assert all(hip_huff.prepare(f)[1].nbits < 1024 for f in files)                # one subsequence each
    for S in (1024, 4096, 64):
        dec = DeviceJpegDecoder(threads=1, entropy='device', subseq_bits=S)
        outs = dec(files)
        torch.cuda.synchronize()
        dec.check_status()
        assert dec.stats['device'] == 2
        for o, e in zip(outs, exp):
            assert np.array_equal(o.cpu().numpy(), e)
        assert dec.status[:, 1].max().item() <= max(1, -(-max(hip_huff.prepare(f)[1].nbits for f in files) // S))


def test_an_error_at_the_fixed_point_sets_the_status_word():
    """a stream that ends before the frame's last block (a scan cut short, then ended by EOI): the image's status word is set, the
    other image of the batch decodes"""
    from gpv1_amd.jpeg import DeviceJpegDecoder
    good = open(os.path.join(GOLD, 'c444_q90.jpg'), 'rb').read()
    cut = good[:-800]
    while cut[-1] == 0xFF:
        cut = cut[:-1]
    dec = DeviceJpegDecoder(threads=1, entropy='device')
    outs = dec([good, cut + b'\xff\xd9'])
    torch.cuda.synchronize()
    assert dec.stats['device'] == 2
    st = dec.status.cpu().numpy()
    assert st[0, 0] == 0 and st[1, 0] & 2
    with pytest.raises(ValueError, match='status'):
        dec.check_status()
    assert np.array_equal(outs[0].cpu().numpy(), np.load(os.path.join(GOLD, 'expected.npz'))['c444_q90'])


def test_loader_batches_equal_the_host_loaders(tmp_path):
    from tests import coco_tree as CT
    from gpv1_amd.datasets import CocoMultitaskDataset, DeviceLoader
    size = (64, 96)
    plan = {'cap': {'train': [2], 'val': [2, 3]}, 'det': {'train': [4], 'val': [4]}, 'cls': {'train': [1]}, 'vqa': {'train': [3]},
            'refcocop': {'train': [6]}}
    tc = CT.make_tree(tmp_path, plan, image_size=size)
    kinds = ('cap', 'det', 'cls', 'vqa', 'refcocop')
    order = [3, 0, 2, 4, 1, 0]
    got = {}
    for entropy in ('host', 'device'):
        ds = CocoMultitaskDataset(CT.learning_datasets(kinds), tc, 'train', seed=5)
        loader = DeviceLoader(ds, 2, device=DEV, threads=2, prefetch=1, entropy=entropy)
        got[entropy] = [(s.tensors.clone(), s.mask.clone(), q) for s, q, _ in loader.batches(order, epoch=2)]
        torch.cuda.synchronize()
        loader.dec.check_status()
        loader.close()
        assert loader.dec.stats[entropy] == 6 or entropy == 'device'
        if entropy == 'device':
            assert loader.dec.stats['device'] + loader.dec.stats['host'] == 6 and loader.dec.stats['device'] >= 1
    assert len(got['host']) == len(got['device']) == 3
    for (a, am, aq), (b, bm, bq) in zip(got['host'], got['device']):
        assert torch.equal(a, b) and torch.equal(am, bm) and aq == bq
