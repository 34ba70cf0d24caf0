"""Training flight recorder: exact per-parameter tensor statistics every step, a device ring of them and a latch that remembers
where a non-finite value first appeared -- without a sync, an allocation or anything per parameter on the host in the step.

THE RULE is stated once, here, on the host (``segment_stats_host``, ``ring_commit_host``; the same text is in include/gpv_health.h)
and run as three small launches of libgpv_health.so (csrc/tensor_stats.hip, ``hip_health``), which equal it bit for bit.

A segment is n >= 0 consecutive elements of fp32 or bf16; a bf16 element is widened exactly to fp32 (its 16 bits become the high
half) before anything is computed from its value.  Its statistics are one fixed-size row (``hip_health.ROW``, 64 bytes):

  n_nan, n_inf, n_zero   int64 counts; -0.0 counts as zero, a denormal does not
  first_bad              int64 index, relative to the segment start, of the first NaN or +-inf; -1 if there is none
  first_kind             1 (NaN) or 2 (inf): what the element at first_bad is; 0 if there is none
  absmax                 fp32, largest |x| over the finite elements, 0 if there are none; exact
  sumsq                  float64 sum of x * x over the finite elements in the pinned order below
  bits_sum               uint64 wrap-around sum of the raw element bit patterns, each 32-bit or 16-bit pattern zero-extended:
                         independent of order and exact.  Two buffers with different bits almost surely differ in it -- a cheap
                         fingerprint for "did P change", "do two replicas hold the same bits", "did a checkpoint round-trip exactly"

Pinned order of sumsq: the segment is cut from its start into blocks of 16384 elements; in a block, element j belongs to lane
(j >> 2) & 255; a lane adds its squares in ascending j in float64, starting from +0.0; the 256 lane sums are folded by the tree
s[l] += s[l + stride] for stride = 128, 64, ..., 1; the block sums s[0] are added in ascending block order, starting from +0.0.
The square of an fp32 value is exact in float64, so fused and unfused multiply-add round alike: only the order matters.
n == 0 gives an all-zero row with first_bad = -1.

The ring and the latch (``ring_commit_host``): commit number c (the device-resident cursor, so that a captured graph advances it on
every replay) copies the S fresh rows into slot c % R of a ring [R][S], stamps the slot with c and advances the cursor.  If some row
of the commit has n_nan + n_inf > 0 the trip counter goes up by one, and if the latch is still empty it records (c, the lowest such
segment index, that row's first_bad and first_kind): the first trip wins.  Segments are registered in dataflow order -- watched
activations, then G, then P / M / V -- so the lowest segment index is the earliest place in the step.

The recorder observes and reports; it never writes to a watched buffer and changes no decision of the optimizer."""
import json
import os
import warnings

import numpy as np
import torch

from . import hip_health as hh

ROW = hh.ROW
BLOCK = hh.BLOCK
KINDS = {0: None, hh.NAN: 'nan', hh.INF: 'inf'}


class NonFiniteError(RuntimeError):
    """a watched tensor held a NaN or an inf: .step (the recorder's step, commit x every), .commit, .name, .buffer ('G', 'P', 'M',
    'V' or 'act'), .index (element, relative to the start of the named tensor), .kind ('nan' / 'inf'), .trips (commits with a
    non-finite value so far)"""

    def __init__(self, trip):
        self.trip = dict(trip)
        for k, v in trip.items():
            setattr(self, k, v)
        super().__init__('gpv1_amd.health: first non-finite value at recorded step %(step)d (commit %(commit)d): %(kind)s in %(buffer)s '
                         'of %(name)s at element %(index)d; %(trips)d recorded step(s) held one so far' % trip)


def _raw_bits(x, dtype=None):
    """-> (bit patterns as a 1-D uint32 or uint16 array, is_bf16).  x: numpy float32; numpy uint16 holding bf16 patterns
    (dtype='bf16'); a CPU torch tensor of float32 or bfloat16"""
    if torch.is_tensor(x):
        x = x.detach().reshape(-1).contiguous()
        if x.dtype == torch.bfloat16:
            return x.view(torch.int16).numpy().view(np.uint16), True
        if x.dtype != torch.float32:
            raise TypeError(f'health: fp32 or bf16 segments only, got {x.dtype}')
        return x.numpy().view(np.uint32), False
    x = np.ascontiguousarray(x).reshape(-1)
    if dtype == 'bf16':
        if x.dtype != np.uint16:
            raise TypeError('health: bf16 segments are given as their uint16 bit patterns')
        return x, True
    if x.dtype != np.float32:
        raise TypeError(f'health: fp32 or bf16 segments only, got {x.dtype}')
    return x.view(np.uint32), False


def segment_stats_host(x, dtype=None):
    """THE RULE (module docstring) in numpy: the row of one segment as a 0-d array of ``hip_health.ROW``"""
    raw, bf = _raw_bits(x, dtype)
    n = raw.size
    row = np.zeros((), ROW)
    row['first_bad'] = -1
    if n == 0:
        return row
    f = (raw.astype(np.uint32) << np.uint32(16)) if bf else raw
    u = f & np.uint32(0x7fffffff)
    isnan, isinf = u > np.uint32(0x7f800000), u == np.uint32(0x7f800000)
    fin = ~(isnan | isinf)
    row['n_nan'], row['n_inf'], row['n_zero'] = int(isnan.sum()), int(isinf.sum()), int((u == 0).sum())
    bad = np.flatnonzero(~fin)
    if bad.size:
        row['first_bad'] = int(bad[0])
        row['first_kind'] = hh.INF if isinf[bad[0]] else hh.NAN
    if fin.any():
        row['absmax'] = u[fin].max().view(np.float32)             # |x| orders like its bit pattern
    row['bits_sum'] = raw.astype(np.uint64).sum(dtype=np.uint64)   # wraps modulo 2^64
    # sumsq in the pinned order: [block][i][lane][c] with j = 1024 i + 4 lane + c; the elements a block lacks and the non-finite
    # ones enter as +0.0, which changes no partial sum (every partial sum is >= +0.0)
    nb = -(-n // BLOCK)
    v = np.zeros(nb * BLOCK, np.float64)
    v[:n] = np.where(fin, f.view(np.float32), np.float32(0)).astype(np.float64)
    sq = (v * v).reshape(nb, 16, 256, 4)
    lanes = np.zeros((nb, 256), np.float64)
    for i in range(16):                                            # a lane's own elements in ascending j
        for c in range(4):
            lanes = lanes + sq[:, i, :, c]
    stride = 128
    while stride >= 1:                                             # the tree s[l] += s[l + stride]
        lanes[:, :stride] = lanes[:, :stride] + lanes[:, stride:2 * stride]
        stride //= 2
    total = 0.0
    for b in range(nb):                                            # block sums in ascending block order
        total = total + float(lanes[b, 0])
    row['sumsq'] = total
    return row


def new_ring_host(R, S):
    """(state int64 [STATE_WORDS], stamps int64 [R], ring ROW [R, S]) as before the first commit"""
    return np.zeros(hh.STATE_WORDS, np.int64), np.full(R, -1, np.int64), np.zeros((R, S), ROW)


def ring_commit_host(state, stamps, ring, rows):
    """THE RULE of gpv_health_commit (module docstring), in place on the arrays of ``new_ring_host``"""
    R = ring.shape[0]
    c = int(state[hh.ST_CURSOR])
    ring[c % R] = rows
    stamps[c % R] = c
    state[hh.ST_CURSOR] = c + 1
    bad = np.flatnonzero(rows['n_nan'] + rows['n_inf'] > 0)
    if bad.size:
        state[hh.ST_TRIPS] += 1
        if state[hh.ST_LATCHED] == 0:
            s = int(bad[0])
            state[hh.ST_LATCHED], state[hh.ST_TRIP_CURSOR], state[hh.ST_TRIP_SEG] = 1, c, s
            state[hh.ST_TRIP_INDEX], state[hh.ST_KIND] = rows['first_bad'][s], rows['first_kind'][s]


class Reading:
    """one device-to-host copy of ring and latch, decoded: .cursor (commits so far), .commits (those still in the ring, ascending),
    .rows(commit) (ROW [S] in segment order), .row(name, buffer, commit), .grad_norms(commit), .trip, .steps"""

    def __init__(self, rec, state, stamps, ring):
        self._rec, self.state, self.stamps, self.ring = rec, state, stamps, ring
        self.cursor = int(state[hh.ST_CURSOR])
        self.trips = int(state[hh.ST_TRIPS])
        self.commits = sorted(int(c) for c in stamps if c >= 0)
        self._slot = {int(c): i for i, c in enumerate(stamps) if c >= 0}

    @property
    def latest(self):
        return self.commits[-1] if self.commits else None

    def rows(self, commit=None):
        commit = self.latest if commit is None else commit
        if commit not in self._slot:
            raise KeyError(f'health: commit {commit} is not in the ring (have {self.commits[:1]} .. {self.commits[-1:]})')
        return self.ring[self._slot[commit]]

    def row(self, name, buffer='G', commit=None):
        return self.rows(commit)[self._rec.index[(buffer, name)]]

    def grad_norms(self, commit=None):
        """per optimizer group of train.GROUPS the L2 norm of the averaged gradient, as the reference would log it from p.grad:
        sqrt(sum of the group's segment sumsq) x trainer.grad_scale (finite elements only; None when G is not watched)"""
        rec = self._rec
        if rec.trainer is None or not rec.group_segments:
            return None
        r = self.rows(commit)
        return {g: float(np.sqrt(r['sumsq'][idx].sum(dtype=np.float64)) * rec.trainer.grad_scale) if len(idx) else 0.0
                for g, idx in rec.group_segments.items()}

    @property
    def trip(self):
        """the latched first trip as a dict (NonFiniteError's fields), or None"""
        st = self.state
        if st[hh.ST_LATCHED] == 0:
            return None
        buffer, name = self._rec.segments[int(st[hh.ST_TRIP_SEG])][:2]
        c = int(st[hh.ST_TRIP_CURSOR])
        return {'step': c * self._rec.every, 'commit': c, 'name': name, 'buffer': buffer, 'segment': int(st[hh.ST_TRIP_SEG]),
                'index': int(st[hh.ST_TRIP_INDEX]), 'kind': KINDS.get(int(st[hh.ST_KIND])), 'trips': self.trips}

    @property
    def steps(self):
        """per recorded step still in the ring: {'commit', 'step', 'rows': {(buffer, name): row}, 'grad_norms'}"""
        return [{'commit': c, 'step': c * self._rec.every, 'grad_norms': self.grad_norms(c),
                 'rows': {key: self.rows(c)[i] for key, i in self._rec.index.items()}} for c in self.commits]


def row_dict(row):
    """a row as plain Python numbers (JSON)"""
    return {'n_nan': int(row['n_nan']), 'n_inf': int(row['n_inf']), 'n_zero': int(row['n_zero']), 'first_bad': int(row['first_bad']),
            'first_kind': KINDS.get(int(row['first_kind'])), 'absmax': float(row['absmax']), 'sumsq': float(row['sumsq']),
            'bits_sum': int(row['bits_sum'])}


class FlightRecorder:
    """FlightRecorder(trainer=None, watch=('G',), ring=64, device=None, every=1, on_nonfinite='raise')

    Builds the segment table from ``trainer.entries`` (name, offset, numel) over whichever of the trainer's flat ``P`` / ``G`` / ``M``
    / ``V`` buffers are named in `watch`; ``watch_tensor(name, t)`` adds any tensor whose storage is static (a captured body's
    outputs, say; buffer label 'act').  Registration order is dataflow order: watched activations, then G, then P / M / V, each in the
    trainer's flat order.  The step's loss is not watched: the trainer exposes no static loss tensor (a graphed body's loss scalar
    belongs to that body and is cloned before it is returned; an eager step makes a new one) -- register one with watch_tensor where
    a caller has it.  Descriptors, work list, workspace and ring are allocated and uploaded once, at ``prepare()`` or the first
    ``record()``; nothing can be registered after that.

    ``record()``   the three launches on the current stream: no sync, no allocation, capturable (after ``prepare()``).  With
                   every = k only every k-th call launches anything (the first one does).
    ``read()``     ONE device-to-host copy of ring and latch -> ``Reading``.
    ``check()``    raises ``NonFiniteError`` (or warns, on_nonfinite='warn') when the latch holds a trip.
    ``fingerprint(buffer)``  the bits_sum values of the latest slot for that buffer's segments, in flat order (uint64 array).

    ``FlatTrainer.recorder = rec`` makes ``train_step`` call ``rec.record()`` once the step's gradients are final (after the gradient
    exchange where there is one) and before the optimizer step."""

    def __init__(self, trainer=None, watch=('G',), ring=64, device=None, every=1, on_nonfinite='raise'):
        watch = tuple(watch)
        if any(b not in ('P', 'G', 'M', 'V') for b in watch) or (watch and trainer is None):
            raise ValueError(f"health: watch names the trainer's flat buffers 'P', 'G', 'M', 'V' (and needs a trainer), got {watch!r}")
        if on_nonfinite not in ('raise', 'warn'):
            raise ValueError(f"health: on_nonfinite is 'raise' or 'warn', got {on_nonfinite!r}")
        if int(ring) < 1 or int(every) < 1:
            raise ValueError('health: ring and every are at least 1')
        self.trainer, self.watch, self.R, self.every, self.on_nonfinite = trainer, watch, int(ring), int(every), on_nonfinite
        self.device = torch.device(device) if device is not None else (trainer.P.device if trainer is not None else torch.device('cuda'))
        if self.device.type != 'cuda':
            raise RuntimeError('gpv1_amd: the flight recorder runs on the GPU (no CPU fallback exists)')
        self._acts = []              # (name, tensor)
        self.segments = None         # after prepare(): (buffer, name, tensor, element offset, n) in segment order
        self.index, self.group_segments = {}, {}
        self.calls = 0
        self._warned = False

    # ---- registration ----
    def watch_tensor(self, name, t):
        if self.segments is not None:
            raise RuntimeError('health: the segment table is already on the device; register every tensor before prepare() / record()')
        if not t.is_cuda or t.dtype not in (torch.float32, torch.bfloat16) or not t.is_contiguous():
            raise ValueError(f'health: watch_tensor takes a contiguous fp32 or bf16 GPU tensor, got {t.dtype} {tuple(t.shape)} on {t.device}')
        if any(n == name for n, _ in self._acts):
            raise ValueError(f'health: {name!r} is watched already')
        self._acts.append((name, t))

    def prepare(self):
        """build and upload the tables (once); idempotent"""
        if self.segments is not None:
            return self
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('health: call prepare() (or one record()) before capturing record() in a graph')
        segs = [('act', name, t, 0, t.numel()) for name, t in self._acts]
        for b in [b for b in ('G', 'P', 'M', 'V') if b in self.watch]:
            flat = getattr(self.trainer, b)
            segs += [(b, n, flat, o, k) for (n, p, g, o, k) in self.trainer.entries]
        if not segs:
            raise ValueError('health: nothing is watched')
        self.segments = segs
        self.index = {(b, n): i for i, (b, n, t, o, k) in enumerate(segs)}
        if 'G' in self.watch:
            from .train import GROUPS
            self.group_segments = {g: np.array([self.index[('G', n)] for (n, p, gg, o, k) in self.trainer.entries if gg == g], np.int64)
                                   for g in GROUPS}
        S = self.S = len(segs)
        seg = np.zeros(S, hh.SEG)
        work = []
        for i, (b, n, t, o, k) in enumerate(segs):
            seg[i] = (t.data_ptr() + o * t.element_size(), k, hh.BF16 if t.dtype == torch.bfloat16 else hh.F32, 0, len(work))
            work += [(i, blk) for blk in range(-(-k // BLOCK))]
        W = self.W = len(work)
        up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).to(self.device)
        self._segs = up(seg)
        self._work = up(np.array(work, hh.WORK)) if W else None
        self._ws = torch.zeros(W * ROW.itemsize, dtype=torch.uint8, device=self.device) if W else None
        self._rows = torch.zeros(S * ROW.itemsize, dtype=torch.uint8, device=self.device)
        # state | stamps | ring in ONE buffer: read() is one copy
        state, stamps, ring = new_ring_host(self.R, S)
        self._o_stamps = hh.STATE_WORDS * 8
        self._o_ring = self._o_stamps + (self.R * 8 + 63) // 64 * 64
        image = np.zeros(self._o_ring + self.R * S * ROW.itemsize, np.uint8)
        image[self._o_stamps:self._o_stamps + self.R * 8] = np.frombuffer(stamps.tobytes(), np.uint8)
        self._buf = torch.from_numpy(image).to(self.device)
        self._state = self._buf[:self._o_stamps]
        self._stamps = self._buf[self._o_stamps:self._o_stamps + self.R * 8]
        self._ring = self._buf[self._o_ring:]
        return self

    # ---- the step ----
    def record(self):
        """statistics of every watched segment -> the next ring slot (three launches on the current stream); False when `every`
        skips this call"""
        self.calls += 1
        if (self.calls - 1) % self.every:
            return False
        if self.segments is None:
            self.prepare()
        hh.stats(self._segs, self.S, self._work, self.W, self._ws, self._rows)
        hh.commit(self._rows, self.S, self.R, self._state, self._stamps, self._ring)
        return True

    # ---- reading ----
    def read(self):
        self.prepare()
        host = self._buf.cpu().numpy()
        state = host[:self._o_stamps].view(np.int64)
        stamps = host[self._o_stamps:self._o_stamps + self.R * 8].view(np.int64)
        ring = host[self._o_ring:].view(ROW).reshape(self.R, self.S)
        return Reading(self, state, stamps, ring)

    def check(self, reading=None):
        """raise (or warn once) when the latch holds a trip; `reading`: a Reading already taken (else the 64 state bytes are copied)"""
        if reading is None:
            self.prepare()
            reading = Reading(self, self._state.cpu().numpy().view(np.int64), np.zeros(0, np.int64), None)
        trip = reading.trip
        if trip is None:
            return None
        err = NonFiniteError(trip)
        if self.on_nonfinite == 'raise':
            raise err
        if not self._warned:
            warnings.warn(str(err), RuntimeWarning, stacklevel=2)
            self._warned = True
        return trip

    def fingerprint(self, buffer, reading=None):
        reading = self.read() if reading is None else reading
        idx = [i for i, s in enumerate(self.segments) if s[0] == buffer]
        if not idx:
            raise KeyError(f'health: buffer {buffer!r} is not watched (watching {sorted({s[0] for s in self.segments})})')
        return reading.rows()['bits_sum'][idx].copy()

    def report(self, reading):
        """what the driver writes next to the checkpoints on a trip: the trip and the rows of the offending tensor for every step
        still in the ring"""
        trip = reading.trip
        if trip is None:
            return None
        i = trip['segment']
        return {'trip': trip, 'every': self.every, 'ring': self.R, 'numel': int(self.segments[i][4]),
                'rows': [dict(row_dict(reading.rows(c)[i]), commit=c, step=c * self.every) for c in reading.commits]}

    def write_report(self, reading, path):
        rep = self.report(reading)
        if rep is not None:
            tmp = path + '.tmp'
            with open(tmp, 'w') as f:
                json.dump(rep, f, indent=1)
            os.replace(tmp, path)
        return rep
