"""The rule of device-side JPEG entropy decoding, stated once on the host in plain Python / numpy (include/gpv_huff.h repeats it word
for word, csrc/jpeg_huff.hip implements it, tests/test_jpeg_entropy_rule_cpu.py pins it against gpv_jpeg_parse).

A Huffman stream is serial: symbol boundaries are known only by decoding.  It is also self-synchronising: a decoder started at a
wrong bit falls into step with the true symbol sequence after a few symbols.  So the stream is cut into subsequences of S bits,
every subsequence is decoded from a guessed start, and a subsequence whose predecessor ended elsewhere than assumed is decoded
again from that end -- until nothing changes.  The fixed point is the sequential decode, by induction from subsequence 0, whose
start is known.

    prep = prepare_host(open(path, 'rb').read())             # byte-level pass: markers, tables, un-stuffing, route
    coefs, passes = decode_subsequences_host(prep, 1024)      # == the coefs of hip.jpeg_parse, bit for bit

Scope of the device route: baseline, one interleaved scan, no restart interval, the scan ended by EOI.  Other files that
gpv_jpeg_parse takes are routed 'host' and keep that parser; what it refuses is refused here in the same way."""
import numpy as np

from .hip import JpegInfo, JpegUnsupported
from .jpeg_encode import ZIGZAG as _ZIGZAG

LOOK = 9
MIN_S, MAX_S = 64, 4096
MAX_STREAM = 1 << 27
ERR_CODE, ERR_SHORT, ERR_EXTENT = 1, 2, 4
ZIGZAG = tuple(int(k) for k in _ZIGZAG)                   # plain ints: the walk below indexes with them symbol by symbol


def _bad(why):
    return ValueError(f'jpeg_entropy: malformed JPEG ({why})')


def build_table(counts, syms):
    """the look-ahead form of jpeg.hip's build_table: 9-bit look-up + maxcode / valoffset / syms; None when the counts are no code"""
    t = dict(look_nbits=np.zeros(1 << LOOK, np.uint8), look_sym=np.zeros(1 << LOOK, np.uint8), maxcode=np.zeros(18, np.int32),
             valoffset=np.zeros(17, np.int32), syms=np.zeros(256, np.uint8))
    t['syms'][:len(syms)] = np.frombuffer(bytes(syms), np.uint8)
    code = k = 0
    for l in range(1, 17):
        t['valoffset'][l] = k - code
        n = counts[l - 1]
        if n:
            if code + n > (1 << l):
                return None
            for _ in range(n):
                if l <= LOOK:
                    first = code << (LOOK - l)
                    t['look_nbits'][first:first + (1 << (LOOK - l))] = l
                    t['look_sym'][first:first + (1 << (LOOK - l))] = syms[k]
                k += 1
                code += 1
            t['maxcode'][l] = code - 1
        else:
            t['maxcode'][l] = -1
        code <<= 1
    t['maxcode'][17] = 0x7fffffff
    return t if k == len(syms) else None


def prepare_host(data):
    """one file (bytes) -> dict: stream (uint8, un-stuffed, zero-padded to stream_cap), nbits, dc / ac (per component, look-ahead
    form), the MCU geometry (blocks_per_mcu, blk_comp / blk_v / blk_h, nblocks, comp_h / comp_v, mcus_x / mcus_y and the width,
    height, ncomp, hmax, vmax, bh, bw, coef_offset, coef_count, quant of gpv_jpeg_info) and route: 'device' or 'host'"""
    d = bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise _bad('no SOI')
    p = 2
    dc, ac, qt = [None] * 4, [None] * 4, [None] * 4
    comp_id, comp_h, comp_v, comp_tq, comp_td, comp_ta = [0] * 3, [1] * 3, [1] * 3, [0] * 3, [0] * 3, [0] * 3
    W = H = nf = ri = 0
    have_frame = adobe_rgb = False
    while True:
        while p < n and d[p] != 0xFF:
            p += 1
        while p < n and d[p] == 0xFF:
            p += 1
        if p >= n:
            raise _bad('no scan')
        m = d[p]
        p += 1
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7:
            continue
        if m == 0xD9 or p + 2 > n:
            raise _bad('no scan')
        ln = (d[p] << 8) | d[p + 1]
        if ln < 2 or p + ln > n:
            raise _bad('segment length')
        seg = d[p + 2:p + ln]
        sl = ln - 2
        if m == 0xDB:
            q = 0
            while q < sl:
                pq, tq = seg[q] >> 4, seg[q] & 15
                if pq:
                    raise JpegUnsupported('jpeg_entropy: 16-bit quantisation table')
                if tq > 3 or q + 65 > sl:
                    raise _bad('DQT')
                t = np.zeros(64, np.uint16)
                t[list(ZIGZAG)] = np.frombuffer(seg[q + 1:q + 65], np.uint8)
                qt[tq] = t
                q += 65
        elif m == 0xC4:
            q = 0
            while q < sl:
                if q + 17 > sl:
                    raise _bad('DHT')
                tc, th = seg[q] >> 4, seg[q] & 15
                counts = list(seg[q + 1:q + 17])
                ns = sum(counts)
                if tc > 1 or th > 3 or ns > 256 or q + 17 + ns > sl:
                    raise _bad('DHT')
                tab = build_table(counts, seg[q + 17:q + 17 + ns])
                if tab is None:
                    raise _bad('DHT code')
                (ac if tc else dc)[th] = tab
                q += 17 + ns
        elif m in (0xC0, 0xC1):
            if sl < 6:
                raise _bad('SOF')
            if seg[0] != 8:
                raise JpegUnsupported('jpeg_entropy: sample precision')
            H, W, nf = (seg[1] << 8) | seg[2], (seg[3] << 8) | seg[4], seg[5]
            if nf not in (1, 3):
                raise JpegUnsupported('jpeg_entropy: component count')
            if sl < 6 + 3 * nf or W <= 0 or H <= 0:
                raise _bad('SOF')
            for i in range(nf):
                comp_id[i], comp_h[i], comp_v[i], comp_tq[i] = seg[6 + 3 * i], seg[7 + 3 * i] >> 4, seg[7 + 3 * i] & 15, seg[8 + 3 * i]
                if comp_tq[i] > 3:
                    raise _bad('SOF')
            have_frame = True
        elif m in (0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF):
            raise JpegUnsupported('jpeg_entropy: progressive / lossless / arithmetic coding')
        elif m == 0xEE:
            if sl >= 12 and seg[:5] == b'Adobe' and seg[11] == 0:
                adobe_rgb = True
        elif m == 0xDD:
            if sl < 2:
                raise _bad('DRI')
            ri = (seg[0] << 8) | seg[1]
        elif m == 0xDA:
            if not have_frame or sl < 1:
                raise _bad('SOS')
            ns = seg[0]
            if ns != nf:
                raise JpegUnsupported('jpeg_entropy: non-interleaved scans')
            if sl < 1 + 2 * ns + 3:
                raise _bad('SOS')
            for i in range(ns):
                if seg[1 + 2 * i] != comp_id[i]:
                    raise JpegUnsupported('jpeg_entropy: scan component order')
                comp_td[i], comp_ta[i] = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
                if comp_td[i] > 3 or comp_ta[i] > 3:
                    raise _bad('SOS')
            p += ln
            break
        p += ln
    if nf == 3 and adobe_rgb:
        raise JpegUnsupported('jpeg_entropy: RGB-coded file')
    if nf == 3:
        if (comp_h[0], comp_v[0]) not in ((1, 1), (2, 1), (2, 2)) or (comp_h[1], comp_v[1], comp_h[2], comp_v[2]) != (1, 1, 1, 1):
            raise JpegUnsupported('jpeg_entropy: sampling factors')
    else:
        comp_h[0] = comp_v[0] = 1
    hmax, vmax = comp_h[0], comp_v[0]
    mx, my = (W + 8 * hmax - 1) // (8 * hmax), (H + 8 * vmax - 1) // (8 * vmax)
    bh, bw, coef_offset, quant, off = [0] * 3, [0] * 3, [0] * 3, np.zeros((3, 64), np.uint16), 0
    for i in range(nf):
        if qt[comp_tq[i]] is None:
            raise _bad('quantisation table missing')
        bh[i], bw[i], coef_offset[i] = my * comp_v[i], mx * comp_h[i], off
        off += bh[i] * bw[i] * 64
        quant[i] = qt[comp_tq[i]]
    for i in range(nf):
        if dc[comp_td[i]] is None or ac[comp_ta[i]] is None:
            raise _bad('Huffman table missing')
    # the entropy segment: up to the first FF that is not followed by 00
    i, end, marker = p, n, None
    while True:
        i = d.find(b'\xff', i)
        if i < 0:
            break
        if i + 1 < n and d[i + 1] == 0:
            i += 2
            continue
        end, marker = i, (d[i + 1] if i + 1 < n else None)
        break
    raw = d[p:end].replace(b'\xff\x00', b'\xff')
    route = 'device' if (ri == 0 and marker == 0xD9 and len(raw) <= MAX_STREAM) else 'host'
    cap = (len(raw) + 15) // 16 * 16 + 16
    stream = np.zeros(cap, np.uint8)
    stream[:len(raw)] = np.frombuffer(raw, np.uint8)
    blk_comp, blk_v, blk_h = [], [], []
    for ci in range(nf):
        for v in range(comp_v[ci]):
            for h in range(comp_h[ci]):
                blk_comp.append(ci); blk_v.append(v); blk_h.append(h)
    return dict(route=route, stream=stream, nbits=8 * len(raw), stream_cap=cap, restart_interval=ri,
                dc=[dc[comp_td[i]] for i in range(nf)], ac=[ac[comp_ta[i]] for i in range(nf)],
                width=W, height=H, ncomp=nf, hmax=hmax, vmax=vmax, mcus_x=mx, mcus_y=my, bh=bh, bw=bw, comp_h=comp_h, comp_v=comp_v,
                coef_offset=coef_offset, coef_count=off, quant=quant, blocks_per_mcu=len(blk_comp), nblocks=mx * my * len(blk_comp),
                blk_comp=blk_comp, blk_v=blk_v, blk_h=blk_h)


def with_stream(prep, raw):
    """prep with another (already un-stuffed) stream: how the tests feed arbitrary bytes to the walk"""
    raw = bytes(raw)
    cap = (len(raw) + 15) // 16 * 16 + 16
    stream = np.zeros(cap, np.uint8)
    stream[:len(raw)] = np.frombuffer(raw, np.uint8)
    return dict(prep, stream=stream, nbits=8 * len(raw), stream_cap=cap)


def check_subseq_bits(S):
    if not (isinstance(S, (int, np.integer)) and MIN_S <= S <= MAX_S and S % 32 == 0):
        raise ValueError(f'jpeg_entropy: subseq_bits must be a multiple of 32 in {MIN_S} .. {MAX_S}, got {S!r}')


class _Walker:
    """one image's stream and tables as Python lists (the walk is symbol by symbol)"""

    def __init__(self, prep):
        self.buf = prep['stream'].tobytes() + bytes(8)
        self.cap = prep['stream_cap']
        self.nbits = prep['nbits']
        self.bpm = prep['blocks_per_mcu']
        self.nblocks = prep['nblocks']
        tabs = lambda ts: [tuple(t[k].tolist() for k in ('look_nbits', 'look_sym', 'maxcode', 'valoffset', 'syms')) for t in ts]
        self.dc = [tabs(prep['dc'])[c] for c in prep['blk_comp']]              # per block of the MCU
        self.ac = [tabs(prep['ac'])[c] for c in prep['blk_comp']]
        mx = prep['mcus_x']
        self.base = []                                                         # per block of the MCU: (coef_offset, bw, V, H, v, h)
        for c, v, h in zip(prep['blk_comp'], prep['blk_v'], prep['blk_h']):
            self.base.append((prep['coef_offset'][c], prep['bw'][c], prep['comp_v'][c], prep['comp_h'][c], v, h))
        self.mx = mx

    def address(self, blk):
        mcu, j = divmod(blk, self.bpm)
        y0, x0 = divmod(mcu, self.mx)
        off, bw, V, H, v, h = self.base[j]
        return off + ((y0 * V + v) * bw + x0 * H + h) * 64

    def walk(self, p, c, z, limit, S, out=None, blk=0):
        """symbols while p < limit (at most S of them) -> (p, c, z, blocks finished, error bits of blocks inside the frame)"""
        buf, cap, bpm = self.buf, self.cap, self.bpm
        cnt = err = 0
        c = min(max(c, 0), bpm - 1)
        for _ in range(S):
            if p >= limit:
                break
            i = p >> 3
            w = ((int.from_bytes(buf[i:i + 8], 'big') >> (32 - (p & 7))) & 0xFFFFFFFF) if i + 8 <= cap + 8 else 0
            look_nbits, look_sym, maxcode, valoffset, syms = self.dc[c] if z == 0 else self.ac[c]
            look = w >> (32 - LOOK)
            nb = look_nbits[look]
            e = 0
            if nb:
                sym = look_sym[look]
            else:
                nb, sym, e = 16, 0, ERR_CODE
                for l in range(LOOK + 1, 17):
                    code = w >> (32 - l)
                    if code <= maxcode[l]:
                        nb, sym, e = l, syms[(code + valoffset[l]) & 255], 0
                        break
            if z == 0:
                t = sym
                if t > 15:
                    t, e = 15, ERR_CODE
                v = 0
                if t:
                    v = (w >> (32 - nb - t)) & ((1 << t) - 1)
                    if v < (1 << (t - 1)):
                        v = v - (1 << t) + 1
                p += nb + t
                if out is not None and blk < self.nblocks:
                    out[self.address(blk)] = v
                z = 1
            else:
                r, s = sym >> 4, sym & 15
                p += nb + s
                if s == 0:
                    z = z + 16 if r == 15 else 64
                else:
                    z += r
                    if z > 63:
                        z, e = 64, ERR_CODE
                    else:
                        if out is not None and blk < self.nblocks:
                            v = (w >> (32 - nb - s)) & ((1 << s) - 1)
                            if v < (1 << (s - 1)):
                                v = v - (1 << s) + 1
                            out[self.address(blk) + ZIGZAG[z]] = v
                        z += 1
            if blk < self.nblocks:
                err |= e
            if z >= 64:
                z, c, cnt, blk = 0, (c + 1 if c + 1 < bpm else 0), cnt + 1, blk + 1
        return p, c, z, cnt, err


def decode_subsequences_host(prep, S, info=None):
    """the rule (module docstring; include/gpv_huff.h) -> (coefs [coef_count] int16, passes).  info: a dict that receives
    status (ERR_* bits), n_sub and blocks (finished, the stream's padding bits included)"""
    check_subseq_bits(S)
    wk = _Walker(prep)
    nbits = wk.nbits
    n_sub = max(1, -(-nbits // S))
    lim = [min((i + 1) * S, nbits) for i in range(n_sub)]
    state = [None] * n_sub
    changed = [True] * n_sub
    passes = 0
    for k in range(n_sub):                                   # at most n_sub passes
        nxt, chg = list(state), [False] * n_sub
        for i in range(n_sub):
            if k == 0:
                nxt[i] = wk.walk(min(i * S, nbits), 0, 0, lim[i], S)[:4]
                chg[i] = True
            elif i > 0 and changed[i - 1]:
                p, c, z, _ = state[i - 1]
                nxt[i] = wk.walk(p, c, z, lim[i], S)[:4]
                chg[i] = nxt[i][:3] != state[i][:3]
        state, changed = nxt, chg
        passes += 1
        if not any(changed[:n_sub - 1]):
            break
    first, total = [0] * n_sub, 0
    for i in range(n_sub):                                   # exclusive prefix of the blocks finished
        first[i] = total
        total += state[i][3]
    coefs = np.zeros(prep['coef_count'], np.int16)
    out = np.zeros(prep['coef_count'], np.int64)
    status = 0
    for i in range(n_sub):                                   # the write pass
        p, c, z = (0, 0, 0) if i == 0 else state[i - 1][:3]
        status |= wk.walk(p, c, z, lim[i], S, out, first[i])[4]
    if total < prep['nblocks']:
        status |= ERR_SHORT
    coefs[:] = out.astype(np.int16)
    # DC: running sum per component in scan order, int32, stored as int16
    nmcu = prep['mcus_x'] * prep['mcus_y']
    for ci in range(prep['ncomp']):
        js = [j for j in range(prep['blocks_per_mcu']) if prep['blk_comp'][j] == ci]
        addr = np.array([[wk.address(m * wk.bpm + j) for j in js] for m in range(nmcu)], np.int64).reshape(-1)
        coefs[addr] = np.cumsum(out[addr].astype(np.int32), dtype=np.int32).astype(np.int16)
    if info is not None:
        info.update(status=status, n_sub=n_sub, blocks=total)
    return coefs, passes


def info_of(prep):
    """the gpv_jpeg_info (hip.JpegInfo) of a prepared file"""
    inf = JpegInfo()
    inf.width, inf.height, inf.ncomp, inf.hmax, inf.vmax = prep['width'], prep['height'], prep['ncomp'], prep['hmax'], prep['vmax']
    inf.mcus_x, inf.mcus_y, inf.coef_count = prep['mcus_x'], prep['mcus_y'], prep['coef_count']
    for c in range(prep['ncomp']):
        inf.bh[c], inf.bw[c], inf.coef_offset[c] = prep['bh'][c], prep['bw'][c], prep['coef_offset'][c]
        for k in range(64):
            inf.quant[c][k] = int(prep['quant'][c][k])
    return inf
