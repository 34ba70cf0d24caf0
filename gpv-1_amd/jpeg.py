"""JPEG files -> decoded uint8 RGB images on the GPU (the first stage of the device-side input pipeline).

Reference: `img = skio.imread(img_path)` + grey -> 3 channels in the loader workers (datasets/coco_generic_dataset.py:48-58,
datasets/coco_datasets.py:151-163, inference_util.py:9-16): Pillow / libjpeg-turbo on 30 CPU processes.  Here the host only walks the
entropy-coded bit stream (gpv_jpeg_parse, C++, one image per pool thread, the GIL released), the quantised coefficients (2 bytes per
sample position, mostly zero -- but a fixed-size upload) go to the GPU through pinned memory and everything per block / per pixel --
dequantisation, the 8x8 inverse DCT, chroma upsampling, YCbCr -> RGB -- runs there for the whole batch in two launches
(gpv_jpeg_decode, csrc/jpeg.hip), bit-exact against Pillow's decoder.

    dec = DeviceJpegDecoder()
    images = dec([open(p, 'rb').read() for p in paths])        # list of [H, W, 3] uint8 CUDA tensors
    samples = DeviceImagePipeline(train=True)(images, tasks)   # resize + augmentation + normalisation -> the stem's input

entropy='device' (opt-in) moves the Huffman walk to the GPU as well (gpv_huff_decode, csrc/jpeg_huff.hip; the rule is stated in
gpv1_amd.jpeg_entropy): the host keeps a byte-level pass per file (gpv_huff_prepare: markers, tables, un-stuffing) and uploads the
file's entropy bytes and a descriptor in place of its coefficients.  Files with restart markers, or whose scan is not ended by
EOI, are parsed on the host as before, inside the same batch.

Scope: baseline sequential Huffman JPEG, 8 bit, grey or YCbCr with 4:4:4 / 4:2:2 / 4:2:0 sampling, restart markers -- what COCO's
files are.  Anything else raises hip.JpegUnsupported (no silent CPU fallback).  EXIF orientation is not applied."""
import ctypes as C
from concurrent.futures import ThreadPoolExecutor

import torch

from . import hip
from .misc import upload_bytes


class ParsedBatch:
    """what DeviceJpegDecoder.parse leaves for issue: per file the header (hip.JpegInfo) and the start of its coefficients in
    `coefs` (CPU int16 tensor); lent: `coefs` is the caller's buffer (pinned by its owner), not pageable memory of our own"""

    def __init__(self, infos, starts, coefs, lent):
        self.infos, self.starts, self.coefs, self.lent = infos, starts, coefs, lent
        self.slot = None                                 # the decoder's own ring slot, when __call__ lent it
        # entropy='device': `coefs` holds the coefficients of the host-routed files and, behind them, the un-stuffed streams of the
        # device-routed ones (as int16 elements: one buffer, one upload).  huff: per device-routed file (index, hip_huff.HuffDesc,
        # byte offset of its stream in `coefs`); starts[i] of such a file counts in dev_total, the device-only coefficient buffer
        self.huff, self.dev_total = None, 0


class DeviceJpegDecoder:
    def __init__(self, device='cuda', threads=8, slots=3, max_pixels=64 << 20, entropy='host', subseq_bits=1024):
        """entropy: 'host' (default: gpv_jpeg_parse walks the Huffman stream on the pool) or 'device' (gpv_huff_decode walks it on the
        GPU in subsequences of subseq_bits bits, a multiple of 32 in 64 .. 4096); stats counts files per route and bytes uploaded.
        max_pixels: refuse files whose header declares more than this many pixels (default 64 MPix; COCO's largest is 0.4) BEFORE
        anything is sized from it -- a 300-byte file may declare 65535 x 65535 -- and keep every offset of gpv_jpeg_desc inside its
        32-bit fields (3 components x 64 MPix x 1 byte < 2^31)"""
        self.device = torch.device(device)
        self.max_pixels = int(min(max_pixels, 512 << 20))
        self.pool = ThreadPoolExecutor(max_workers=threads) if threads > 1 else None
        # pinned staging for the coefficients: a ring of buffers, each guarded by the event of its last upload (allocating
        # pinned memory per batch costs more than decoding the batch)
        self._stage, self._events, self._turn = [None] * slots, [None] * slots, 0
        self._keep = None
        if entropy not in ('host', 'device'):
            raise ValueError(f"DeviceJpegDecoder: entropy must be 'host' or 'device', got {entropy!r}")
        self.entropy, self.subseq_bits = entropy, int(subseq_bits)
        if entropy == 'device':
            from . import hip_huff
            hip_huff.rule.check_subseq_bits(self.subseq_bits)
            hip_huff.lib()                                    # a missing library is an error here, not at the first batch
        self.stats = {'device': 0, 'host': 0, 'bytes_uploaded': 0}
        self.status = None                                    # entropy='device': int32 [n, 2] (error bits, passes) of the last batch, on the device

    def _staging(self, n, slot=None):
        """-> (slot, its whole pinned buffer of at least n elements); slot: one this batch already holds (it grows), else the next in turn"""
        k = slot
        if k is None:
            k = self._turn
            self._turn = (k + 1) % len(self._stage)
            if self._events[k] is not None:
                self._events[k].synchronize()
        if self._stage[k] is None or self._stage[k].numel() < n:
            self._stage[k] = torch.empty(max(n, 1 << 22), dtype=torch.int16).pin_memory()
        return k, self._stage[k]

    def parse(self, files, into=None):
        """the HOST half: header pass + Huffman decoding of every file on the pool.  Makes no HIP call of any kind (no pinned
        allocation, no event, no copy), so a worker thread may run it while the main thread captures a graph.
        into: a CPU int16 tensor to decode into (the caller's pinned slot); when it is None or too small the coefficients go to
        pageable memory and issue() stages them.  Or a callable n -> such a tensor of n elements, called once the header pass
        knows the size: how __call__ takes a slot of its pinned ring (that one does make HIP calls: not for a worker thread).
        -> ParsedBatch"""
        if self.entropy == 'device':
            return self._parse_device(files, into)
        B = len(files)
        run = (lambda f, it: list(self.pool.map(f, it))) if self.pool is not None else (lambda f, it: [f(x) for x in it])
        infos = run(hip.jpeg_parse, files)                                            # header pass: sizes
        starts, total = [], 0
        for i, inf in enumerate(infos):
            if inf.width * inf.height > self.max_pixels or int(inf.coef_count) > 4 * self.max_pixels:
                raise ValueError(f'DeviceJpegDecoder: file {i} declares {inf.width} x {inf.height} pixels, more than max_pixels = {self.max_pixels}')
            starts.append(total)
            total += int(inf.coef_count)
        if callable(into):
            into = into(total)
        lent = into is not None and into.numel() >= total
        coefs = into[:total] if lent else torch.empty(total, dtype=torch.int16)
        run(lambda i: hip.jpeg_parse(files[i], coefs[starts[i]:starts[i] + int(infos[i].coef_count)]), range(B))
        return ParsedBatch(infos, starts, coefs, lent)

    def _parse_device(self, files, into):
        """parse() with entropy='device': gpv_huff_prepare per file on the pool (host code, no HIP call); the files it routes to the
        host get gpv_jpeg_parse as before"""
        from . import hip_huff
        B = len(files)
        run = (lambda f, it: list(self.pool.map(f, it))) if self.pool is not None else (lambda f, it: [f(x) for x in it])
        heads = run(hip_huff.prepare, files)                                          # sizes + route (+ tables and geometry)
        infos = [h[0] for h in heads]
        starts, host_total, dev_total, stream_at, stream_total = [], 0, 0, {}, 0
        for i, (inf, desc, cap, route) in enumerate(heads):
            if inf.width * inf.height > self.max_pixels or int(inf.coef_count) > 4 * self.max_pixels:
                raise ValueError(f'DeviceJpegDecoder: file {i} declares {inf.width} x {inf.height} pixels, more than max_pixels = {self.max_pixels}')
            if route == 'device':
                starts.append(dev_total)
                dev_total += int(inf.coef_count)
                stream_at[i] = stream_total
                stream_total += cap                                                  # (a multiple of 16)
            else:
                starts.append(host_total)
                host_total += int(inf.coef_count)
        total = host_total + stream_total // 2                                        # int16 elements; host_total is a multiple of 64
        if callable(into):
            into = into(total)
        lent = into is not None and into.numel() >= total
        blob = into[:total] if lent else torch.empty(total, dtype=torch.int16)
        streams = blob[host_total:].view(torch.uint8)

        def one(i):
            if i in stream_at:
                hip_huff.prepare(files[i], streams[stream_at[i]:stream_at[i] + heads[i][2]], heads[i][1])
            else:
                hip.jpeg_parse(files[i], blob[starts[i]:starts[i] + int(infos[i].coef_count)])
        run(one, range(B))
        parsed = ParsedBatch(infos, starts, blob, lent)
        parsed.huff = [(i, heads[i][1], 2 * host_total + at) for i, at in stream_at.items()]
        parsed.dev_total = dev_total
        return parsed

    def _issue_huff(self, parsed, blob):
        """upload the descriptors of the device-routed files and launch gpv_huff_decode -> the device-only coefficient buffer"""
        from . import hip_huff
        dev, n = self.device, len(parsed.huff)
        self.stats['host'] += len(parsed.infos) - n
        self.stats['device'] += n
        if n == 0:
            self.status = None
            return None, ()
        dcoefs = torch.empty(parsed.dev_total, dtype=torch.int16, device=dev)
        status = torch.empty(n, 2, dtype=torch.int32, device=dev)
        descs = (hip_huff.HuffDesc * n)()
        for k, (i, desc, at) in enumerate(parsed.huff):
            C.memmove(C.byref(descs[k]), C.byref(desc), C.sizeof(desc))
            descs[k].stream = blob.data_ptr() + at
            descs[k].coefs = dcoefs.data_ptr() + 2 * parsed.starts[i]
            descs[k].status = status.data_ptr() + 8 * k
        max_nbits = max(desc.nbits for _, desc, _ in parsed.huff)
        ws = torch.empty(hip_huff.workspace_bytes(n, self.subseq_bits, max_nbits), dtype=torch.uint8, device=dev)
        raw = upload_bytes(bytes(descs), dev)
        hip_huff.decode(raw, n, self.subseq_bits, max_nbits, ws)
        self.stats['bytes_uploaded'] += C.sizeof(descs)
        self.status = status
        return dcoefs, (raw, ws, status)

    def check_status(self):
        """entropy='device': read the status words of the last batch (synchronises) and raise if a stream did not decode"""
        if self.status is not None:
            bad = [(k, int(s)) for k, s in enumerate(self.status[:, 0].tolist()) if s]
            if bad:
                raise ValueError(f'DeviceJpegDecoder: gpv_huff_decode reports malformed entropy data (device-routed file, status bits): {bad}')

    def issue(self, parsed, event=None):
        """the DEVICE half: upload of the coefficients + the decode launches -> list of [H, W, 3] uint8 tensors on the device
        (asynchronous: ordered on the current stream).  Coefficients that parse() left in pageable memory are staged through
        the pinned ring here.  event: recorded behind the upload (the owner of a lent buffer waits on it before reusing it)."""
        infos, starts, B = parsed.infos, parsed.starts, len(parsed.infos)
        if B == 0:
            return []
        dev = self.device
        if parsed.lent:
            slot, stage = parsed.slot, parsed.coefs
        else:
            slot, stage = self._staging(parsed.coefs.numel(), parsed.slot)            # one pinned buffer, one upload
            stage = stage[:parsed.coefs.numel()]
            stage.copy_(parsed.coefs)
        coefs = stage.to(dev, non_blocking=True)
        ev = event if event is not None else torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        if slot is not None:
            self._events[slot] = ev
        self.stats['bytes_uploaded'] += 2 * stage.numel()
        dcoefs, keep, on_dev = None, (), set()
        if parsed.huff is not None:
            dcoefs, keep = self._issue_huff(parsed, coefs)
            on_dev = {i for i, _, _ in parsed.huff}
        elif self.entropy == 'host':
            self.stats['host'] += B
        pl_sizes = [sum(inf.bh[c] * inf.bw[c] * 64 for c in range(inf.ncomp)) for inf in infos]
        planes = torch.empty(sum(pl_sizes), dtype=torch.uint8, device=dev)
        outs = [torch.empty(inf.height, inf.width, 3, dtype=torch.uint8, device=dev) for inf in infos]
        descs = (hip.JpegDesc * B)()
        pl0 = 0
        for i, (d, inf, st, out, psz) in enumerate(zip(descs, infos, starts, outs, pl_sizes)):
            d.coefs = (dcoefs if i in on_dev else coefs).data_ptr() + 2 * st
            d.planes = planes.data_ptr() + pl0
            d.out = out.data_ptr()
            d.width, d.height, d.ncomp, d.hmax, d.vmax = inf.width, inf.height, inf.ncomp, inf.hmax, inf.vmax
            off = 0
            for c in range(inf.ncomp):
                d.bh[c], d.bw[c] = inf.bh[c], inf.bw[c]
                if int(inf.coef_offset[c]) >= 1 << 31 or off >= 1 << 31:        # (cannot happen under max_pixels; never truncate silently)
                    raise OverflowError('DeviceJpegDecoder: component offset does not fit gpv_jpeg_desc')
                d.coef_off[c] = int(inf.coef_offset[c])
                d.plane_off[c] = off
                off += inf.bh[c] * inf.bw[c] * 64
            C.memmove(d.quant, inf.quant, C.sizeof(inf.quant))
            pl0 += psz
        raw = upload_bytes(bytes(descs), dev)
        hip.jpeg_decode(raw, B, max(p // 64 for p in pl_sizes), max(inf.width * inf.height for inf in infos))
        self._keep = (coefs, planes, raw, dcoefs) + keep                   # operands of the asynchronous launches
        return outs

    def __call__(self, files):
        """files: list of bytes objects (whole .jpg files) -> list of [H, W, 3] uint8 tensors on the device (asynchronous: ordered on
        the current stream)"""
        if len(files) == 0:
            return []
        slot = []

        def ring(n):                                          # one pinned buffer of the ring, sized by the header pass
            k, stage = self._staging(n)
            slot.append(k)
            return stage
        parsed = self.parse(files, into=ring)
        parsed.slot = slot[0]
        return self.issue(parsed)
