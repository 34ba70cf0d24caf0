"""The rule of device-side JPEG entropy decoding (gpv1_amd.jpeg_entropy; include/gpv_huff.h), CPU side: the subsequence iteration
against the product's sequential host parser (gpv_jpeg_parse), the byte-level pass against the oracle's parse and against its C
twin (gpv_huff_prepare), the routing, and arbitrary bytes as a stream."""
import glob
import os

import numpy as np
import pytest

from oracle import jpeg_oracle as J

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'jpeg')
FILES = sorted(glob.glob(os.path.join(GOLD, '*.jpg')))
NAMES = [os.path.basename(f)[:-4] for f in FILES]
PLAIN = [n for n in NAMES if '_rst' not in n]            # the restart-free fixtures
TABLE_KEYS = ('look_nbits', 'look_sym', 'maxcode', 'valoffset', 'syms')


def read(name):
    return open(os.path.join(GOLD, name + '.jpg'), 'rb').read()


def test_fixture_split():
    assert len(NAMES) == 14 and len(PLAIN) == 11


@pytest.mark.parametrize('S', [64, 256, 1024])
@pytest.mark.parametrize('name', PLAIN)
def test_subsequence_iteration_equals_the_host_parser(name, S):
    import gpv1_amd.hip as hip
    from gpv1_amd import jpeg_entropy as E
    data = read(name)
    prep = E.prepare_host(data)
    assert prep['route'] == 'device'
    ref = np.full(hip.jpeg_parse(data).coef_count, 7, np.int16)
    hip.jpeg_parse(data, ref)
    info = {}
    coefs, passes = E.decode_subsequences_host(prep, S, info)
    assert coefs.dtype == np.int16 and coefs.shape == ref.shape and np.array_equal(coefs, ref)
    assert info['n_sub'] == max(1, -(-prep['nbits'] // S)) and 1 <= passes <= info['n_sub']
    assert info['status'] == 0 and info['blocks'] >= prep['nblocks']


def test_small_subsequences_take_many_passes():
    """the iteration is exercised, not just pass 0 + a confirming pass: 64-bit subsequences on the largest fixture"""
    from gpv1_amd import jpeg_entropy as E
    _, passes = E.decode_subsequences_host(E.prepare_host(read('c420_big')), 64)
    assert passes > 10


@pytest.mark.parametrize('name', NAMES)
def test_prepare_host_agrees_with_the_oracle_on_tables_and_geometry(name):
    from gpv1_amd import jpeg_entropy as E
    data = read(name)
    prep, fr = E.prepare_host(data), J.parse(data)
    assert (prep['width'], prep['height'], prep['ncomp'], prep['hmax'], prep['vmax']) == (fr['width'], fr['height'], len(fr['comps']), fr['hmax'], fr['vmax'])
    assert (prep['mcus_x'], prep['mcus_y'], prep['restart_interval']) == (fr['mcus_x'], fr['mcus_y'], fr['restart_interval'])
    assert prep['blocks_per_mcu'] == sum(c['h'] * c['v'] for c in fr['comps'])
    assert prep['nblocks'] == sum(c['blocks'].shape[0] * c['blocks'].shape[1] for c in fr['comps'])
    order = [(ci, v, h) for ci, c in enumerate(fr['comps']) for v in range(c['v']) for h in range(c['h'])]
    assert list(zip(prep['blk_comp'], prep['blk_v'], prep['blk_h'])) == order
    off = 0
    for ci, c in enumerate(fr['comps']):
        assert (prep['bh'][ci], prep['bw'][ci]) == c['blocks'].shape[:2] and prep['coef_offset'][ci] == off
        assert (prep['comp_h'][ci], prep['comp_v'][ci]) == (c['h'], c['v'])
        off += c['blocks'].size
        assert np.array_equal(prep['quant'][ci], fr['qt'][c['tq']])
    assert prep['coef_count'] == off
    # the tables: every code of the oracle's canonical tables decodes to its symbol through the look-ahead form
    d = bytes(data)
    tabs, p = {}, 2
    while d[p + 1] != 0xDA:
        ln = (d[p + 2] << 8) | d[p + 3]
        if d[p + 1] == 0xC4:
            seg, q = d[p + 4:p + 2 + ln], 0
            while q < len(seg):
                counts = list(seg[q + 1:q + 17])
                tabs[(seg[q] >> 4, seg[q] & 15)] = J._Huff(counts, seg[q + 17:q + 17 + sum(counts)])
                q += 17 + sum(counts)
        p += 2 + ln
    for ci, c in enumerate(fr['comps']):
        for cls, key, sel in ((0, 'dc', c['td']), (1, 'ac', c['ta'])):
            h, t = tabs[(cls, sel)], prep[key][ci]
            for ln in range(1, 17):
                if h.maxcode[ln] < 0:
                    assert t['maxcode'][ln] == -1
                    continue
                assert t['maxcode'][ln] == h.maxcode[ln] and t['valoffset'][ln] == h.valptr[ln] - h.mincode[ln]
                for code in range(h.mincode[ln], h.maxcode[ln] + 1):
                    sym = h.symbols[h.valptr[ln] + code - h.mincode[ln]]
                    assert t['syms'][code + t['valoffset'][ln]] == sym
                    if ln <= E.LOOK:
                        first = code << (E.LOOK - ln)
                        assert set(t['look_nbits'][first:first + (1 << (E.LOOK - ln))]) == {ln}
                        assert set(t['look_sym'][first:first + (1 << (E.LOOK - ln))]) == {sym}


def test_routing():
    from gpv1_amd import jpeg_entropy as E
    for n in NAMES:
        assert E.prepare_host(read(n))['route'] == ('host' if '_rst' in n else 'device'), n
    for n in ('c420_big', 'c444_q90', 'gray_q80'):
        assert E.prepare_host(read(n)[:-100])['route'] == 'host'                 # cut 100 bytes short: no EOI behind the scan
        assert E.prepare_host(read(n)[:-2])['route'] == 'host'                   # only the EOI is missing
        assert E.prepare_host(read(n)[:-2] + b'\xff\xd0')['route'] == 'host'     # a marker other than EOI ends the data


def test_unsupported_files_raise_as_the_host_parser_does():
    import io
    import gpv1_amd.hip as hip
    from PIL import Image
    from gpv1_amd import jpeg_entropy as E
    img = (np.random.RandomState(0).rand(40, 56, 3) * 255).astype(np.uint8)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, 'JPEG', progressive=True)
    with pytest.raises(hip.JpegUnsupported):
        E.prepare_host(buf.getvalue())
    with pytest.raises(ValueError):
        E.prepare_host(b'not a jpeg at all')
    with pytest.raises(ValueError):
        E.prepare_host(read('c420_big')[:200])
    with pytest.raises(ValueError):
        E.decode_subsequences_host(E.prepare_host(read('c420_tiny')), 48)
    with pytest.raises(ValueError):
        E.decode_subsequences_host(E.prepare_host(read('c420_tiny')), 8192)


@pytest.mark.parametrize('name', NAMES)
def test_c_prepare_equals_prepare_host_byte_for_byte(name):
    import gpv1_amd.hip as hip
    from gpv1_amd import hip_huff
    from gpv1_amd import jpeg_entropy as E
    for data in (read(name), read(name)[:-100], read(name)[:-1]):
        try:
            prep = E.prepare_host(data)
        except ValueError as e:                                                  # (a small fixture cut inside its header)
            with pytest.raises(ValueError) as got:
                hip_huff.prepare(data)
            assert isinstance(got.value, hip.JpegUnsupported) == isinstance(e, hip.JpegUnsupported)
            continue
        info, desc, cap, route = hip_huff.prepare(data)                          # sizes only
        assert (route, cap) == (prep['route'], prep['stream_cap'])
        out = np.full(cap + 32, 0xAB, np.uint8)
        info2, desc2, cap2, route2 = hip_huff.prepare(data, out[:cap])
        assert bytes(info) == bytes(info2) == bytes(E.info_of(prep)) == bytes(hip.jpeg_parse(data))
        assert bytes(desc) == bytes(desc2) and (cap2, route2) == (cap, route)
        assert out[:cap].tobytes() == prep['stream'].tobytes() and set(out[cap:]) == {0xAB}
        assert (desc.nbits, desc.stream_cap, desc.ncomp, desc.mcus_x, desc.mcus_y, desc.blocks_per_mcu, desc.nblocks, desc.coef_count) == \
            (prep['nbits'], prep['stream_cap'], prep['ncomp'], prep['mcus_x'], prep['mcus_y'], prep['blocks_per_mcu'], prep['nblocks'], prep['coef_count'])
        assert (desc.stream, desc.coefs, desc.status) == (None, None, None)
        n, m = prep['ncomp'], prep['blocks_per_mcu']
        for field in ('bh', 'bw', 'comp_h', 'comp_v', 'coef_offset'):
            assert list(getattr(desc, field))[:n] == list(prep[field])[:n], field
        for field in ('blk_comp', 'blk_v', 'blk_h'):
            assert list(getattr(desc, field)) == list(prep[field]) + [0] * (8 - m), field
        for c in range(3):
            for key in ('dc', 'ac'):
                tab = getattr(desc, key)[c]
                if c < n:
                    for k in TABLE_KEYS:
                        assert bytes(getattr(tab, k)) == prep[key][c][k].tobytes(), (key, c, k)
                else:
                    assert not any(bytes(tab))
    with pytest.raises(ValueError):
        hip_huff.prepare(read(name), np.zeros(16, np.uint8))                     # a lent buffer that is too small


SMALL = [n for n in NAMES if os.path.getsize(os.path.join(GOLD, n + '.jpg')) <= 2100]


def _sos_offset(d):
    """offset of the FF of the SOS marker of a well-formed file (a walk over its segments, not a search for FF DA)"""
    p = 2
    while d[p + 1] != 0xDA:
        p += 2 + ((d[p + 2] << 8) | d[p + 3])
    return p


def _outcome(fn, *args):
    """(None, result) or (the refusal's class, None): JpegUnsupported against a plain ValueError"""
    import gpv1_amd.hip as hip
    try:
        return None, fn(*args)
    except ValueError as e:
        return (hip.JpegUnsupported if isinstance(e, hip.JpegUnsupported) else ValueError), None


def test_small_fixture_split():
    assert len(SMALL) == 12 and set(NAMES) - set(SMALL) == {'c420_big', 'c444_q90'}


@pytest.mark.parametrize('name', SMALL)
def test_the_two_host_entry_points_agree_on_damaged_headers(name):
    """gpv_jpeg_parse (header pass) and gpv_huff_prepare read the same headers: every cut and every single-byte change of the
    region up to the SOS marker + 16 gets the same refusal class from both or the same `info` bytes.  Where only prepare refuses
    (it asks for the Huffman tables at once), the full decode of gpv_jpeg_parse refuses in the same way."""
    import gpv1_amd.hip as hip
    from gpv1_amd import hip_huff
    data = read(name)
    region = min(len(data), _sos_offset(data) + 16)
    variants = [data[:cut] for cut in range(region + 1)]
    for i in range(region):
        for b in (0x00, 0xFF, (data[i] + 1) & 255):
            variants.append(data[:i] + bytes([b]) + data[i + 1:])
    assert len(variants) == 4 * region + 1
    skipped = accepted = 0
    for v in variants:
        e_parse, info = _outcome(hip.jpeg_parse, v)
        e_prep, prep = _outcome(hip_huff.prepare, v)
        where = (name, len(v), [i for i in range(min(len(v), region)) if v[i] != data[i]])
        if e_parse is not None:
            assert e_prep is e_parse, where                                      # both refuse, in the same way
        elif e_prep is None:
            assert bytes(info) == bytes(prep[0]), where                          # both accept
            accepted += 1
        elif info.coef_count > 1 << 22:                                          # only prepare refuses: so does the full decode
            skipped += 1
        else:
            e_full, _ = _outcome(hip.jpeg_parse, v, np.zeros(info.coef_count, np.int16))
            assert e_full is e_prep, where
    assert skipped <= 0.02 * len(variants), (skipped, len(variants))
    assert accepted > len(variants) // 4                                         # (most single-byte changes still parse)


def test_random_bytes_as_a_stream_end_within_the_pass_bound():
    from gpv1_amd import jpeg_entropy as E
    r = np.random.RandomState(7)
    preps = [E.prepare_host(read(n)) for n in ('c420_q75', 'c444_odd_q97', 'gray_q80', 'c420_opt_q30')]
    for t in range(200):
        raw = r.randint(0, 256, int(r.randint(0, 400)), dtype=np.uint8).tobytes()
        prep = E.with_stream(preps[t % 4], raw)
        S = (64, 96, 256, 1024)[t % 4]
        info = {}
        coefs, passes = E.decode_subsequences_host(prep, S, info)
        assert 1 <= passes <= info['n_sub'] and coefs.shape == (prep['coef_count'],)
        if t % 10 == 0:                                                          # the fixed point is the sequential decode
            one = {}
            whole, _ = E.decode_subsequences_host(prep, 4096, one) if prep['nbits'] <= 4096 else (coefs, 0)
            assert np.array_equal(whole, coefs) and (one.get('status', info['status']), one.get('blocks', info['blocks'])) == (info['status'], info['blocks'])
