"""The JPEG encoding rule, stated once on the host in numpy: what gpv-1_amd/csrc/jpeg_enc_host.h repeats in plain C++ and
gpv-1_amd/csrc/jpeg_enc.hip on the device, byte for byte.  DESIGN.md section 6h.

``encode_host`` writes the file Pillow writes for the same pixels (``Image.save(buf, 'JPEG', quality=q, subsampling=s)``: libjpeg's
slow-integer DCT, the Annex K tables, no optimisation): a baseline sequential JPEG, 8 bit, three components, one interleaved scan,
no restart markers.  ``draw_boxes_host`` and ``denormalise_host`` are the two rules in front of it: the one-pixel box outlines of
the reference's ``vis_bbox(..., modify=True, alpha=0)`` and the way from a normalised pipeline batch back to uint8.
``label_plates`` / ``draw_labels_host`` state the labels of the boxes (the reference's ``vis.add_box``): a short text in Pillow's
built-in bitmap font on a dark plate above or below its box, the pixels Pillow's ``rectangle`` + ``text`` draw.
"""
import numpy as np

SUBSAMPLING = {'4:4:4': (1, 1), '4:2:2': (2, 1), '4:2:0': (2, 2)}                # name -> (hs, vs) of the luma component
MAX_BOXES = 32
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])
# Annex K, natural order
Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51,
                   87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120,
                   101, 72, 92, 95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99,
                     99, 99, 99, 99] + [99] * 32)
DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
DC_VALS = (list(range(12)), list(range(12)))
AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 125], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 119])
AC_VALS = (
    [1, 2, 3, 0, 4, 17, 5, 18, 33, 49, 65, 6, 19, 81, 97, 7, 34, 113, 20, 50, 129, 145, 161, 8, 35, 66, 177, 193, 21, 82, 209, 240, 36,
     51, 98, 114, 130, 9, 10, 22, 23, 24, 25, 26, 37, 38, 39, 40, 41, 42, 52, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72, 73, 74,
     83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 131, 132, 133,
     134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170, 178, 179,
     180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216, 217, 218,
     225, 226, 227, 228, 229, 230, 231, 232, 233, 234, 241, 242, 243, 244, 245, 246, 247, 248, 249, 250],
    [0, 1, 2, 3, 17, 4, 5, 33, 49, 6, 18, 65, 81, 7, 97, 113, 19, 34, 50, 129, 8, 20, 66, 145, 161, 177, 193, 9, 35, 51, 82, 240, 21,
     98, 114, 209, 10, 22, 36, 52, 225, 37, 241, 23, 24, 25, 26, 38, 39, 40, 41, 42, 53, 54, 55, 56, 57, 58, 67, 68, 69, 70, 71, 72,
     73, 74, 83, 84, 85, 86, 87, 88, 89, 90, 99, 100, 101, 102, 103, 104, 105, 106, 115, 116, 117, 118, 119, 120, 121, 122, 130, 131,
     132, 133, 134, 135, 136, 137, 138, 146, 147, 148, 149, 150, 151, 152, 153, 154, 162, 163, 164, 165, 166, 167, 168, 169, 170,
     178, 179, 180, 181, 182, 183, 184, 185, 186, 194, 195, 196, 197, 198, 199, 200, 201, 202, 210, 211, 212, 213, 214, 215, 216,
     217, 218, 226, 227, 228, 229, 230, 231, 232, 233, 234, 242, 243, 244, 245, 246, 247, 248, 249, 250])


def _fix(x):
    return int(x * 65536 + 0.5)


def subsampling_factors(subsampling):
    if subsampling not in SUBSAMPLING:
        raise ValueError(f"subsampling must be one of {sorted(SUBSAMPLING)}, got {subsampling!r}")
    return SUBSAMPLING[subsampling]


def quant_tables(quality):
    """(luma, chroma) in natural order"""
    if not 1 <= quality <= 100:
        raise ValueError(f'quality must be 1..100, got {quality}')
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(np.clip((base * scale + 50) // 100, 1, 255) for base in (Q_LUMA, Q_CHROMA))


def huffman_codes(bits, vals):
    """{symbol: (code, length)} of a table given as Annex C states it"""
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return out


def header(H, W, quality, subsampling):
    """everything in front of the scan: SOI, APP0, two DQT, SOF0, four DHT, SOS"""
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f'H and W must be 1..65535, got {H} x {W}')
    hs, vs = subsampling_factors(subsampling)

    def seg(marker, body):
        return bytes([0xFF, marker, (len(body) + 2) >> 8, (len(body) + 2) & 255]) + bytes(body)
    out = b'\xff\xd8' + seg(0xE0, b'JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00')
    for t, q in enumerate(quant_tables(quality)):
        out += seg(0xDB, [t] + [int(v) for v in q[ZIGZAG]])
    out += seg(0xC0, [8, H >> 8, H & 255, W >> 8, W & 255, 3, 1, (hs << 4) | vs, 0, 2, 0x11, 1, 3, 0x11, 1])
    for t in (0, 1):
        out += seg(0xC4, [t] + DC_BITS[t] + DC_VALS[t]) + seg(0xC4, [0x10 | t] + AC_BITS[t] + AC_VALS[t])
    return out + seg(0xDA, [3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 0x3F, 0])


def rgb_to_ycc(rgb):
    r, g, b = (rgb[..., c].astype(np.int64) for c in range(3))
    y = (_fix(.299) * r + _fix(.587) * g + _fix(.114) * b + 32768) >> 16
    cb = (-_fix(.16874) * r - _fix(.33126) * g + _fix(.5) * b + (128 << 16) + 32767) >> 16
    cr = (_fix(.5) * r - _fix(.41869) * g - _fix(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def _downsample(p, hs, vs, bw, bh):
    """a full-resolution plane -> bh x bw blocks of its down-sampled plane.  Columns: the full-resolution plane repeats its last
    column as far as the blocks reach, and the bias alternates along the output row all the way.  Rows: the full-resolution plane
    repeats its last row to a whole group of vs rows; below that the down-sampled plane repeats its own last row."""
    H, W = p.shape
    xs = np.minimum(np.arange(bw * 8 * hs), W - 1)
    rows = -(-H // vs)
    ys = np.minimum(np.arange(rows * vs), H - 1)
    p = p[ys][:, xs]
    if (hs, vs) == (2, 2):
        bias = 1 + (np.arange(bw * 8) & 1)
        p = (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + bias) >> 2
    elif (hs, vs) == (2, 1):
        bias = np.arange(bw * 8) & 1
        p = (p[:, 0::2] + p[:, 1::2] + bias) >> 1
    return p[np.minimum(np.arange(bh * 8), rows - 1)]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of jfdctint along the last axis (13 constant bits, 2 pass-1 bits)"""
    d = [d[..., i] for i in range(8)]
    t0, t7, t1, t6, t2, t5, t3, t4 = d[0] + d[7], d[0] - d[7], d[1] + d[6], d[1] - d[6], d[2] + d[5], d[2] - d[5], d[3] + d[4], d[3] - d[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2] = _descale(z1 + t13 * 6270, n)
    o[6] = _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct(blocks):
    """[..., 8, 8] samples (0..255) -> the transform of sample - 128, scaled by 8: rows first, then columns"""
    d = _fdct_pass(blocks.astype(np.int64) - 128, True)
    return np.swapaxes(_fdct_pass(np.swapaxes(d, -1, -2), False), -1, -2)


def quantise(coefs, q):
    """[..., 64] natural order, q the natural-order table"""
    d = q.astype(np.int64) << 3
    t = (np.abs(coefs) + (d >> 1)) // d
    return np.where(coefs < 0, -t, t)


def plane_blocks(p, bw, bh):
    """[bh*8, bw*8] -> [bh, bw, 64] quantisation-ready blocks in natural order"""
    return p.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3)


def coefficients(rgb, quality, subsampling):
    """quantised blocks per component: [(bh, bw, 64 int in natural order)] * 3, real blocks only"""
    hs, vs = subsampling_factors(subsampling)
    H, W = rgb.shape[:2]
    y, cb, cr = rgb_to_ycc(rgb)
    ql, qc = quant_tables(quality)
    out = []
    for p, (h, v), q in ((y, (1, 1), ql), (cb, (hs, vs), qc), (cr, (hs, vs), qc)):
        bw, bh = -(-(-(-W // h)) // 8), -(-(-(-H // v)) // 8)
        blocks = plane_blocks(_downsample(p, h, v, bw, bh), bw, bh)
        out.append(quantise(fdct(blocks).reshape(bh, bw, 64), q))
    return out


def _pack(codes, lengths):
    """(value, bit count) pairs -> bytes, most significant bit first, the last byte filled with 1-bits"""
    codes, lengths = np.asarray(codes, np.int64), np.asarray(lengths, np.int64)
    shift = lengths[:, None] - 1 - np.arange(32)[None, :]
    bits = ((codes[:, None] >> np.maximum(shift, 0)) & 1)[shift >= 0].astype(np.uint8)
    bits = np.concatenate([bits, np.ones(-len(bits) % 8, np.uint8)])
    return np.packbits(bits).tobytes()


def scan(comps, hs, vs):
    """the entropy-coded segment of the three components' quantised blocks, stuffed"""
    (bh, bw), (cbh, cbw) = comps[0].shape[:2], comps[1].shape[:2]
    dc_codes = [huffman_codes(DC_BITS[t], DC_VALS[t]) for t in (0, 1)]
    ac_codes = [huffman_codes(AC_BITS[t], AC_VALS[t]) for t in (0, 1)]
    codes, lengths = [], []

    def put(v, n):
        codes.append(v)
        lengths.append(n)

    def value(v):
        n = int(abs(v)).bit_length()
        return n, (v if v >= 0 else v - 1) & ((1 << n) - 1)

    def block(zz, dc, pred, t):
        n, extra = value(dc - pred)
        put(*dc_codes[t][n])
        if n:
            put(extra, n)
        run = 0
        last = 0
        for k in np.flatnonzero(zz[1:]) + 1:
            run = k - last - 1
            while run > 15:
                put(*ac_codes[t][0xF0])
                run -= 16
            n, extra = value(int(zz[k]))
            put(*ac_codes[t][(run << 4) + n])
            put(extra, n)
            last = k
        if last < 63:
            put(*ac_codes[t][0])

    zero = np.zeros(64, np.int64)
    pred = [0, 0, 0]
    zz = [c[..., ZIGZAG] for c in comps]
    for my in range(cbh):
        for mx in range(cbw):
            prev = 0                                         # a dummy block repeats the DC of the block coded just before it
            for v in range(vs):
                for h in range(hs):
                    by, bx = my * vs + v, mx * hs + h
                    if by < bh and bx < bw:
                        b = zz[0][by, bx]
                        prev = int(b[0])
                        block(b, prev, pred[0], 0)
                    else:
                        block(zero, prev, pred[0], 0)
                    pred[0] = prev
            for c in (1, 2):
                b = zz[c][my, mx]
                block(b, int(b[0]), pred[c], 1)
                pred[c] = int(b[0])
    return _pack(codes, lengths).replace(b'\xff', b'\xff\x00')


def encode_host(rgb, quality=90, subsampling='4:2:0'):
    """rgb: uint8 [H, W, 3] (numpy array or CPU tensor) -> the bytes of the JPEG file"""
    rgb = np.ascontiguousarray(rgb.numpy() if hasattr(rgb, 'numpy') else rgb)
    if rgb.dtype != np.uint8 or rgb.ndim != 3 or rgb.shape[2] != 3:
        raise ValueError(f'encode_host: a uint8 [H, W, 3] image is needed, got {rgb.dtype} {rgb.shape}')
    hs, vs = subsampling_factors(subsampling)
    H, W = rgb.shape[:2]
    return header(H, W, quality, subsampling) + scan(coefficients(rgb, quality, subsampling), hs, vs) + b'\xff\xd9'


def box_rects(boxes, H, W):
    """normalised (cx, cy, w, h) rows -> integer (x1, y1, x2, y2) rows, as vis_bbox clamps them, rounded half to even.  fp32, every
    operation rounded on its own (the device repeats it)."""
    b = np.asarray(boxes, np.float32).reshape(-1, 4)
    half_w, half_h = b[:, 2] * np.float32(0.5), b[:, 3] * np.float32(0.5)
    x1, x2 = (b[:, 0] - half_w) * np.float32(W), (b[:, 0] + half_w) * np.float32(W)
    y1, y2 = (b[:, 1] - half_h) * np.float32(H), (b[:, 1] + half_h) * np.float32(H)
    x1 = np.maximum(np.float32(0), np.minimum(x1, np.float32(W - 1)))
    x2 = np.maximum(x1, np.minimum(x2, np.float32(W - 1)))
    y1 = np.maximum(np.float32(0), np.minimum(y1, np.float32(H - 1)))
    y2 = np.maximum(y1, np.minimum(y2, np.float32(H - 1)))
    return np.stack([np.rint(v).astype(np.int64) for v in (x1, y1, x2, y2)], 1)


def draw_boxes_host(img, boxes_ncxcywh, colours):
    """writes the one-pixel outline of every box into img (uint8 [H, W, 3], modified in place and returned), in the order given: a
    later box overwrites an earlier one"""
    H, W = img.shape[:2]
    rects = box_rects(boxes_ncxcywh, H, W)
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    if len(rects) != len(colours) or len(rects) > MAX_BOXES:
        raise ValueError(f'draw_boxes_host: one colour per box and at most {MAX_BOXES} boxes, got {len(rects)} boxes, {len(colours)} colours')
    for (x1, y1, x2, y2), c in zip(rects, colours):
        img[y1, x1:x2 + 1] = c
        img[y2, x1:x2 + 1] = c
        img[y1:y2 + 1, x1] = c
        img[y1:y2 + 1, x2] = c
    return img


MAX_LABEL, CELL_W, CELL_H, PLATE_H, PLATE_RGB = 32, 6, 11, 13, (10, 10, 10)


def label_entries(labels, n):
    """the labels of one picture's n boxes -> [(text bytes, below)]: an entry is None (no label), a str (above the box) or
    (str, 'above' | 'below').  A character outside ASCII 32..126 becomes '?', a longer text is cut to MAX_LABEL characters."""
    if labels is None:
        return [(b'', False)] * n
    if len(labels) != n:
        raise ValueError(f'labels: one entry per box is needed (None for a box without label), got {len(labels)} entries for {n} boxes')
    out = []
    for e in labels:
        text, where = (e, 'above') if e is None or isinstance(e, str) else e
        if not (text is None or isinstance(text, str)) or where not in ('above', 'below'):
            raise ValueError(f"labels: an entry is None, a str or (str, 'above' | 'below'), got {e!r}")
        text = bytes(ord(c) if 32 <= ord(c) <= 126 else ord('?') for c in (text or '')[:MAX_LABEL])
        out.append((text, where == 'below'))
    return out


def label_plates(boxes_ncxcywh, labels, H, W):
    """-> int rows (px, py, n), one per box: the top left corner of the label's plate and its character count (0: no label, nothing
    is drawn).  The plate is 6 n + 2 wide and 13 high.  Above the box, or inside it under its top edge where there is no room above;
    below, or inside over its bottom edge; kept inside the picture where it fits, left-aligned with the box."""
    rects = box_rects(boxes_ncxcywh, H, W)
    out = []
    for (x1, y1, x2, y2), (text, below) in zip(rects.tolist(), label_entries(labels, len(rects))):
        w = CELL_W * len(text) + 2
        if below:
            py = y2 + 1
            if py + PLATE_H > H:
                py = y2 - PLATE_H
        else:
            py = y1 - PLATE_H
            if py < 0:
                py = y1 + 1
        py = min(max(py, 0), max(0, H - PLATE_H))
        px = x1
        if px + w > W:
            px = W - w
        px = max(px, 0)
        out.append((px, py, len(text)))
    return np.array(out, np.int64).reshape(-1, 3)


def draw_labels_host(img, boxes_ncxcywh, colours, labels):
    """writes the labels of the boxes into img (uint8 [H, W, 3], modified in place and returned), after draw_boxes_host and in the
    order given: a later label overwrites an earlier one, and no outline cuts a label.  labels: see label_entries.  The text is
    inked in the box's colour, in the 6 x 11 cell of jpeg_label_font, on a plate of PLATE_RGB with one pixel of margin all round."""
    from .jpeg_label_font import ROWS
    H, W = img.shape[:2]
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    plates = label_plates(boxes_ncxcywh, labels, H, W)
    if len(plates) != len(colours) or len(plates) > MAX_BOXES:
        raise ValueError(f'draw_labels_host: one colour per box and at most {MAX_BOXES} boxes, got {len(plates)} boxes, {len(colours)} colours')
    for (px, py, n), (text, _), colour in zip(plates.tolist(), label_entries(labels, len(plates)), colours):
        if n == 0:
            continue
        plate = np.empty((PLATE_H, CELL_W * n + 2, 3), np.uint8)
        plate[:] = PLATE_RGB
        ink = np.zeros((CELL_H, CELL_W * n), bool)
        for k, byte in enumerate(text):                      # as Pillow pastes them: one after the other, each over what is there
            rows = np.array(ROWS[byte - 32], np.uint8)
            ink[:, CELL_W * k:CELL_W * (k + 1)] = (rows[:, None] >> np.arange(CELL_W)[None, :]) & 1
            if k:                                            # a glyph that starts one pixel left of its cell (bit 7), ink or not (bit 6)
                left = ink[:, CELL_W * k - 1]
                left[rows & 0x80 != 0] = (rows[rows & 0x80 != 0] & 0x40) != 0
        plate[1:1 + CELL_H, 1:-1][ink] = colour
        view = img[py:py + PLATE_H, px:px + plate.shape[1]]                 # the picture's edges clip the plate
        view[:] = plate[:view.shape[0], :view.shape[1]]
    return img


def pack_labels(colours, labels):
    """what the device reads at gpv_enc_desc.colours (include/gpv_enc.h): n x (R, G, B, L) and the texts behind them -> (uint8
    array, text bytes).  L = the character count, + 0x80 for a label below its box."""
    colours = np.asarray(colours, np.uint8).reshape(-1, 3)
    entries = label_entries(labels, len(colours))
    head = np.concatenate([colours, np.array([[len(t) | (0x80 if below else 0)] for t, below in entries], np.uint8).reshape(-1, 1)], 1)
    text = b''.join(t for t, _ in entries)
    return np.concatenate([head.reshape(-1), np.frombuffer(text, np.uint8)]), len(text)


def unpack_labels(packed, nboxes, nbytes):
    """the way back, as the device reads it: -> (colours [n, 3], labels as label_entries takes them).  The length bytes are not
    trusted: box i's text starts at min(sum of the counts in front of it, nbytes), and its count is clamped to MAX_LABEL and to
    the bytes that remain behind that."""
    packed = np.asarray(packed, np.uint8).reshape(-1)
    if not 0 <= nbytes <= nboxes * MAX_LABEL or len(packed) < 4 * nboxes + nbytes:
        raise ValueError(f'unpack_labels: {nboxes} boxes with {nbytes} text bytes need {4 * nboxes + nbytes} bytes and at most {MAX_LABEL} per box, got {len(packed)}')
    head, text = packed[:4 * nboxes].reshape(-1, 4), packed[4 * nboxes:4 * nboxes + nbytes].tobytes()
    labels, before = [], 0
    for L in head[:, 3].tolist():
        at = min(before, nbytes)
        n = min(L & 0x7F, MAX_LABEL, nbytes - at)
        before += L & 0x7F
        labels.append((''.join(chr(c) for c in text[at:at + n]), 'below' if L & 0x80 else 'above'))
    return head[:, :3].copy(), labels


def denormalise_host(x, mean, std):
    """x: [..., 3] normalised pixels (fp32 array, or a bf16 / fp32 tensor) -> uint8.  Per channel in fp32, every operation rounded
    on its own: std * x, + mean, * 255, + 0.5, floor, clamp to 0..255 (a NaN gives 0)."""
    if hasattr(x, 'numpy'):
        x = x.float().numpy()
    x = np.asarray(x, np.float32)
    t = np.asarray(std, np.float32) * x
    t = np.asarray(mean, np.float32) + t
    t = np.float32(255) * t
    t = t + np.float32(0.5)
    with np.errstate(invalid='ignore'):
        return np.where(t >= 255, 255, np.where(t > 0, np.floor(t), 0)).astype(np.uint8)


class DeviceJpegEncoder:
    """The same files written on the device (libgpv_enc.so, gpv1_amd.hip_enc): one call encodes a whole batch with four launches.
    There is no host fallback: without the library or a GPU the calls raise."""
    PAD = 3                                                  # of the stem's padded NHWC4 batch (input_pipeline.stem_geometry)

    def __init__(self, quality=90, subsampling='4:2:0', device='cuda'):
        subsampling_factors(subsampling)
        quant_tables(quality)
        self.quality, self.subsampling, self.device = int(quality), subsampling, device
        self._buffers = {}
        self.launches = 0                                    # calls of gpv_enc_encode so far (a second one per batch: see _run)

    def _buffer(self, name, n, dtype):
        import torch
        t = self._buffers.get(name)
        if t is None or t.numel() < n or t.dtype != dtype:
            t = self._buffers[name] = torch.empty(n, dtype=dtype, device=self.device)
        return t[:n]

    def _boxes(self, descs, boxes, colours, keep, labels=None):
        import torch
        if boxes is None:
            if labels is not None:
                raise ValueError('DeviceJpegEncoder: labels belong to boxes, and there are none')
            return
        if colours is None or len(boxes) != len(descs) or len(colours) != len(descs):
            raise ValueError('DeviceJpegEncoder: boxes and colours are lists with one entry per picture')
        if labels is not None and len(labels) != len(descs):
            raise ValueError(f'DeviceJpegEncoder: labels is a list with one entry per picture, got {len(labels)} for {len(descs)} pictures')
        for i, (d, b, c) in enumerate(zip(descs, boxes, colours)):
            b = torch.as_tensor(b, dtype=torch.float32).reshape(-1, 4)
            c = torch.as_tensor(c, dtype=torch.uint8).reshape(-1, 3)
            if len(b) != len(c) or len(b) > MAX_BOXES:
                raise ValueError(f'DeviceJpegEncoder: one colour per box and at most {MAX_BOXES} boxes per picture, got {len(b)} boxes, {len(c)} colours')
            if labels is not None and labels[i] is not None:
                # colours, length bytes and texts in the one tensor that is uploaded anyway (include/gpv_enc.h: Storage)
                packed, nbytes = pack_labels(c.cpu().numpy(), labels[i])             # (a list that does not match the boxes raises)
                if len(b) == 0:
                    continue
                c = torch.from_numpy(packed)
                d.labels = nbytes
            elif len(b) == 0:
                continue
            else:
                c = torch.cat([c, c[:, :1]], 1)
            b = b.to(self.device).contiguous()
            c = c.to(self.device).contiguous()
            keep += [b, c]
            d.boxes, d.colours, d.nboxes = b.data_ptr(), c.data_ptr(), len(b)

    def _run(self, B, fill):
        """fill(descs, keep) sets the pictures' descriptors -> list[bytes].  The files go to slots of a guessed size first (the
        largest picture's raw size, one byte per sample); if a status word reports a longer file, the call is repeated once with the bound that holds any file."""
        import ctypes as C
        import torch
        from . import hip_enc
        pinned = torch.empty(B * C.sizeof(hip_enc.EncDesc), dtype=torch.uint8).pin_memory()
        pinned.zero_()
        descs = (hip_enc.EncDesc * B).from_address(pinned.data_ptr())
        keep = [pinned]
        fill(descs, keep)
        counts = [hip_enc.block_count(d.H, d.W, self.subsampling) for d in descs]
        bound = hip_enc.file_bound(max(counts))
        workspace = self._buffer('workspace', hip_enc.workspace_bytes(B, sum(counts)), torch.uint8)
        sizes, status = self._buffer('sizes', 2 * B, torch.int32)[:B], self._buffer('sizes', 2 * B, torch.int32)[B:]
        with torch.cuda.device(self.device):
            for capacity in (min(bound, hip_enc.HEADER_BYTES + 2 + 64 * max(counts)), bound):
                capacity = (capacity + 15) & ~15
                out = self._buffer('out', B * capacity, torch.uint8)
                hip_enc.encode(descs, B, self.quality, self.subsampling, workspace, out, capacity, sizes, status)
                self.launches += 1
                host = self._buffers['sizes'][:2 * B].cpu()                # the one synchronising copy
                if not host[B:].any():
                    break
            else:
                raise RuntimeError(f'DeviceJpegEncoder: status words {host[B:].tolist()} with the capacity that holds any file')
            n = host[:B].tolist()
            used = torch.cat([out[i * capacity:i * capacity + n[i]] for i in range(B)]).cpu().numpy().tobytes()
        ends = np.cumsum(n)
        return [used[e - k:e] for e, k in zip(ends, n)]

    def encode(self, images, boxes=None, colours=None, labels=None):
        """images: list of uint8 [H, W, 3] tensors or arrays of any sizes; a device tensor that is a window of a larger picture
        (rows `pitch` pixels apart) is read in place.  boxes / colours: per picture, [n, 4] normalised (cx, cy, w, h) and [n, 3].
        labels: per picture, None or a list with one entry per box: None, a str (drawn above the box) or (str, 'above' | 'below');
        a text is cut to 32 characters and a character outside ASCII 32..126 becomes '?' (label_entries, draw_labels_host)."""
        import torch
        from . import hip_enc

        def fill(descs, keep):
            for d, im in zip(descs, images):
                t = torch.as_tensor(im)
                if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3 or 0 in t.shape:
                    raise ValueError(f'DeviceJpegEncoder.encode: uint8 [H, W, 3] pictures are needed, got {t.dtype} {tuple(t.shape)}')
                if not t.is_cuda:
                    t = t.contiguous().pin_memory().to(self.device, non_blocking=True)
                sy, sx, sc = t.stride()
                if not (sc == 1 and sx == 3 and sy % 3 == 0 and sy >= 3 * t.shape[1]):
                    t = t.contiguous()
                keep.append(t)
                d.src, d.H, d.W, d.pitch, d.kind = t.data_ptr(), t.shape[0], t.shape[1], t.stride(0) // 3, hip_enc.SRC_U8
            self._boxes(descs, boxes, colours, keep, labels)
        return self._run(len(images), fill)

    def encode_batch(self, nested, mean, std, boxes=None, colours=None, count=None, labels=None):
        """the first `count` pictures (default: all) of a pipeline batch: nested.tensors = the stem's padded NHWC4 batch
        [B, H + 6, Wp, 4] in bf16 or fp32, nested.mask = [B, H, W]; mean, std = the three normalisation constants each; labels as
        in encode"""
        import torch
        from . import hip_enc
        x = nested.tensors
        H, W = nested.mask.shape[1:]
        if not x.is_cuda:
            raise RuntimeError('gpv1_amd: DeviceJpegEncoder.encode_batch: the batch must live on the GPU (no CPU fallback exists)')
        if x.dim() != 4 or x.shape[3] != 4 or x.shape[1] != H + 2 * self.PAD or x.shape[2] < W + 2 * self.PAD or not x.is_contiguous() or \
                x.dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f'DeviceJpegEncoder.encode_batch: a contiguous padded NHWC4 batch in bf16 or fp32 is needed, got {x.dtype} {tuple(x.shape)} for {H} x {W} pictures')
        B = x.shape[0] if count is None else min(int(count), x.shape[0])
        Hp, Wp = x.shape[1:3]

        def fill(descs, keep):
            keep.append(x)
            for i, d in enumerate(descs):
                d.src = x.data_ptr() + ((i * Hp + self.PAD) * Wp + self.PAD) * 4 * x.element_size()
                d.H, d.W, d.pitch, d.kind = H, W, Wp, hip_enc.SRC_BF16 if x.dtype == torch.bfloat16 else hip_enc.SRC_F32
                d.mean[:], d.std[:] = [float(v) for v in mean], [float(v) for v in std]
            self._boxes(descs, None if boxes is None else boxes[:B], None if colours is None else colours[:B], keep,
                        None if labels is None else labels[:B])
        return self._run(B, fill)
