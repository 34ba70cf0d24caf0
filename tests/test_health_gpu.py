"""The flight recorder on the GPU (libgpv_health.so through gpv1_amd.hip_health / gpv1_amd.health): every row field equals the host
rule bit for bit, nothing is written outside the outputs, ring and latch follow the host model, record() replays from a captured
graph, and a trainer with the recorder on trains exactly as one without it.

Shapes are the smallest at which the kernels can go wrong (tests/health_cases.py): vector heads and tails, the block boundary, a
multi-block fold, segment starts 0, 1, 2, 3 and 5 elements off a 16-byte boundary, both dtypes, empty segments.  The host reference
of the 600 segments is computed once per module and shared."""
import json
import os
import re

import numpy as np
import pytest
import torch

from tests import synth
from tests.health_cases import BLOCK, LENGTHS, make_bits

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CANARY = 0xA5
GUARD = 256
OFFSETS = (0, 1, 2, 3, 5)
VARIANTS4 = ('plain', 'mixed', 'nan', 'den_max')


def _guarded(nbytes, fill=None):
    """(whole buffer, payload view): `nbytes` of payload between two GUARD-byte canary zones"""
    whole = torch.full((GUARD + nbytes + GUARD,), CANARY, dtype=torch.uint8, device=DEV)
    view = whole[GUARD:GUARD + nbytes]
    if fill is not None:
        view.copy_(torch.from_numpy(np.frombuffer(fill, np.uint8).copy()))
    return whole, view


def _guards_intact(whole, nbytes):
    h = whole.cpu().numpy()
    return bool((h[:GUARD] == CANARY).all() and (h[GUARD + nbytes:] == CANARY).all())


class Raw:
    """segments laid out in one canary-filled device buffer + the tables of gpv_health_stats, every output between canaries"""

    def __init__(self, segments):
        from gpv1_amd import hip_health as hh
        self.hh = hh
        pos, place = 0, []
        for bits, bf, off in segments:
            es = 2 if bf else 4
            start = (pos + 15) // 16 * 16 + 64 + off * es             # >= 64 canary bytes in front of every segment
            place.append(start)
            pos = start + bits.size * es + 64                         # and behind it
        self.image = np.full(pos + 64, CANARY, np.uint8)
        for (bits, bf, off), start in zip(segments, place):
            self.image[start:start + bits.nbytes] = np.frombuffer(bits.tobytes(), np.uint8)
        self.data = torch.from_numpy(self.image.copy()).to(DEV)
        self.place = place
        S = self.S = len(segments)
        seg, work = np.zeros(S, hh.SEG), []
        for i, ((bits, bf, off), start) in enumerate(zip(segments, place)):
            seg[i] = (self.data.data_ptr() + start, bits.size, hh.BF16 if bf else hh.F32, 0, len(work))
            work += [(i, b) for b in range(-(-bits.size // BLOCK))]
        W = self.W = len(work)
        self.segs = torch.from_numpy(np.frombuffer(seg.tobytes(), np.uint8).copy()).to(DEV)
        self.work = torch.from_numpy(np.frombuffer(np.array(work, hh.WORK).tobytes(), np.uint8).copy()).to(DEV) if W else None
        self.ws_whole, self.ws = _guarded(W * 64)
        self.rows_whole, self.rows = _guarded(S * 64)

    def stats(self):
        self.hh.stats(self.segs, self.S, self.work, self.W, self.ws if self.W else None, self.rows)
        return self.rows.cpu().numpy().view(self.hh.ROW)

    def write(self, i, index, bits32):
        """overwrite one fp32 element of segment i on the device and in the host image"""
        at = self.place[i] + 4 * index
        self.image[at:at + 4] = np.frombuffer(np.uint32(bits32).tobytes(), np.uint8)
        self.data[at:at + 4] = torch.from_numpy(self.image[at:at + 4].copy()).to(DEV)

    def host_rows(self, segments):
        from gpv1_amd import health
        out = np.zeros(len(segments), self.hh.ROW)
        for i, ((bits, bf, off), start) in enumerate(zip(segments, self.place)):
            cur = self.image[start:start + bits.nbytes].view(bits.dtype)
            out[i] = health.segment_stats_host(cur if bf else cur.view(np.float32), dtype='bf16' if bf else None)
        return out

    def untouched(self):
        return bool((self.data.cpu().numpy() == self.image).all()) and _guards_intact(self.ws_whole, self.W * 64) \
            and _guards_intact(self.rows_whole, self.S * 64)


def _explain(dev, ref, segments):
    bad = [i for i in range(len(ref)) if dev[i].tobytes() != ref[i].tobytes()]
    return [(i, segments[i][0].size, 'bf16' if segments[i][1] else 'fp32', segments[i][2], dev[i], ref[i]) for i in bad[:5]], len(bad)


@pytest.fixture(scope='module')
def cases():
    """600 segments: 15 lengths x 2 dtypes x 5 start offsets x 4 plantings (mixed dtypes, 39 of them empty), one empty one replaced by a
    segment of 40 blocks; and their rows by the host rule"""
    from gpv1_amd import health, hip_health as hh
    hh.lib()                                                       # fail loudly if the library is missing
    segments = []
    for n in LENGTHS:
        for off in OFFSETS:
            for bf in (False, True):
                for v, variant in enumerate(VARIANTS4):
                    segments.append((make_bits(n, bf, variant, seed=len(segments)), bf, off))
    assert len(segments) == 600
    segments[7] = (make_bits(40 * BLOCK - 3, False, 'mixed', seed=7), False, 0)
    ref = np.zeros(len(segments), hh.ROW)
    for i, (bits, bf, off) in enumerate(segments):
        ref[i] = health.segment_stats_host(bits if bf else bits.view(np.float32), dtype='bf16' if bf else None)
    return segments, ref


def test_600_segments_in_one_call_equal_the_host_rule_bit_for_bit(cases):
    segments, ref = cases
    raw = Raw(segments)
    dev = raw.stats()
    torch.cuda.synchronize()
    worst, n_bad = _explain(dev, ref, segments)
    assert n_bad == 0, (n_bad, worst)
    assert dev.tobytes() == ref.tobytes()                          # every field, sumsq and the reserved word included
    assert raw.untouched()                                         # canaries around every segment, the workspace and the rows
    assert int(ref['n_nan'].sum()) > 0 and int(ref['n_inf'].sum()) > 0 and float(ref['sumsq'].max()) > 0


@pytest.mark.parametrize('which', [0, 7, 150, 333, 415, 598, 599])
def test_one_segment_per_call_equals_the_host_rule(cases, which):
    """S = 1: an empty segment, the 40-block one, mid-sized ones of both dtypes at odd offsets, the multi-block tail"""
    segments, ref = cases
    raw = Raw([segments[which]])
    dev = raw.stats()
    assert dev[0].tobytes() == ref[which].tobytes(), (segments[which][0].size, segments[which][1:], dev[0], ref[which])
    assert raw.untouched()


def test_bad_arguments_are_refused_before_a_launch():
    from gpv1_amd import hip_health as hh
    z = torch.zeros(64, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):
        hh.stats(z, 3, None, 0, None, z)                           # 64 bytes are not three descriptors
    with pytest.raises(RuntimeError):
        hh.stats(z.cpu()[:32], 1, None, 0, None, z)                # no CPU path
    assert hh.lib().gpv_health_stats(None, 0, None, 0, None, None, None) != 0
    assert hh.lib().gpv_health_commit(None, 1, 0, None, None, None, None) != 0


def test_ring_of_64_wraps_after_70_commits_and_the_first_trip_wins():
    from gpv1_amd import health, hip_health as hh
    R, S, ncommit = 64, 3, 70
    segments = [(make_bits(300, False, 'plain', seed=1), False, 1), (make_bits(BLOCK + 9, False, 'plain', seed=2), False, 0),
                (make_bits(77, False, 'plain', seed=3), False, 3)]
    raw = Raw(segments)
    state_whole, state = _guarded(hh.STATE_WORDS * 8, fill=np.zeros(hh.STATE_WORDS, np.int64).tobytes())
    stamps_whole, stamps = _guarded(R * 8, fill=np.full(R, -1, np.int64).tobytes())
    ring_whole, ring = _guarded(R * S * 64, fill=bytes(R * S * 64))
    m_state, m_stamps, m_ring = health.new_ring_host(R, S)
    for c in range(ncommit):
        raw.write(0, 0, np.float32(c + 1).view(np.uint32))          # every commit sees other data
        if c == 5:                                                  # two segments at once: the lower index is latched
            raw.write(2, 7, 0x7fc00000)
            raw.write(1, BLOCK + 2, 0xff800000)
        if c == 9:
            raw.write(0, 11, 0x7fc00000)
        raw.hh.stats(raw.segs, raw.S, raw.work, raw.W, raw.ws, raw.rows)
        hh.commit(raw.rows, S, R, state, stamps, ring)
        health.ring_commit_host(m_state, m_stamps, m_ring, raw.host_rows(segments))
        if c in (5, 9):                                             # ordinary data again for the next commit
            raw.write(2, 7, 0x3f800000); raw.write(1, BLOCK + 2, 0x3f800000); raw.write(0, 11, 0x3f800000)
    d_state = state.cpu().numpy().view(np.int64)
    assert list(d_state) == list(m_state), (d_state, m_state)
    assert [int(d_state[i]) for i in (hh.ST_CURSOR, hh.ST_LATCHED, hh.ST_TRIP_CURSOR, hh.ST_TRIP_SEG, hh.ST_TRIP_INDEX, hh.ST_KIND,
                                      hh.ST_TRIPS)] == [70, 1, 5, 1, BLOCK + 2, hh.INF, 2]
    d_stamps = stamps.cpu().numpy().view(np.int64)
    assert list(d_stamps) == list(m_stamps) and sorted(d_stamps) == list(range(6, 70))
    assert ring.cpu().numpy().tobytes() == m_ring.tobytes()
    assert raw.untouched() and _guards_intact(state_whole, hh.STATE_WORDS * 8) and _guards_intact(stamps_whole, R * 8) \
        and _guards_intact(ring_whole, R * S * 64)


def test_record_replays_from_a_captured_graph_and_the_cursor_lives_on_the_device():
    """record() captured once (one stream, no parallel branches), replayed three times with other data each time"""
    from gpv1_amd import health
    g = torch.Generator().manual_seed(4)
    base = torch.randn(3 * BLOCK + 40, generator=g).to(DEV)
    tensors = {'odd': base[3:3 + 1025], 'blocks': base[2048:2048 + 2 * BLOCK + 5],
               'half': torch.randn(777, generator=g).to(DEV).to(torch.bfloat16)}
    rec = health.FlightRecorder(watch=(), ring=8, device=DEV)
    for k, t in tensors.items():
        rec.watch_tensor(k, t)
    rec.prepare()
    with pytest.raises(RuntimeError):
        rec.watch_tensor('late', base)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        rec.record()                                                # commit 0, eager (loads the code objects before the capture)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        rec.record()
    want = {0: {k: health.segment_stats_host(t.cpu()) for k, t in tensors.items()}}
    for r in range(1, 4):
        base.mul_(1.5).add_(float(r))
        tensors['half'].mul_(-2.0)
        if r == 2:
            tensors['half'][5] = float('inf')                       # ordinary data: the latch must name it
        graph.replay()
        want[r] = {k: health.segment_stats_host(t.cpu()) for k, t in tensors.items()}
    reading = rec.read()
    assert reading.cursor == 4 and reading.commits == [0, 1, 2, 3]  # the capture itself committed nothing; one per replay
    for c, rows in want.items():
        for k, row in rows.items():
            assert reading.row(k, 'act', c).tobytes() == row.tobytes(), (c, k, reading.row(k, 'act', c), row)
    trip = reading.trip
    assert (trip['commit'], trip['name'], trip['buffer'], trip['index'], trip['kind'], trip['trips']) == (2, 'half', 'act', 5, 'inf', 2)
    rec.on_nonfinite = 'warn'
    with pytest.warns(RuntimeWarning):
        assert rec.check()['name'] == 'half'


# ---- trainer ----

def _batch():
    from tests.test_model_cpu import B, H, W, Tl, V, PAD
    images, mask, ids, attn = synth.synth_batch(B, H, W, Tl, V, pad_to=PAD)
    return images.to(DEV), mask.to(DEV), ids.to(DEV), attn.to(DEV)


def _targets():
    from tests.test_model_cpu import B, V
    return synth.synth_targets(B, V, S=6, tasks=('CocoCaptioning', 'CocoVqa'))     # no box task: the box heads get no gradient


def _three_steps(recorder_watch):
    """a fresh smallest synthetic model, three eager bf16 steps without dropout from the same seed -> (model, trainer, recorder)"""
    import gpv1_amd.ops as ops
    from gpv1_amd import health
    from gpv1_amd.train import FlatTrainer
    from tests.test_model_cpu import build_small, nested
    ops.RT.set_precise(False)
    ops.RT.manual_seed(1234)
    torch.manual_seed(0)
    model, _ = build_small()
    model.to(DEV).train()
    model.bert.model.p = 0.0
    tr = FlatTrainer(model, lr=1e-3, lr_backbone=1e-4, graphs=False)
    rec = None
    if recorder_watch is not None:
        rec = tr.recorder = health.FlightRecorder(tr, watch=recorder_watch, ring=16)
    images, mask, ids, attn = _batch()
    for _ in range(3):
        loss = tr.train_step(nested(images, mask), (ids, attn), _targets())
        assert torch.isfinite(loss)
    return model, tr, rec


@pytest.fixture(scope='module')
def runs():
    """two runs with the recorder off and one with it on (P, G, M, V watched), then, on the recorder's trainer and in this order:
    the norms, a record() between two snapshots, a checkpoint round trip, one more step, a step with a NaN planted in G"""
    from gpv1_amd import health
    from tests.test_model_cpu import nested
    out = {}
    for tag in ('off_a', 'off_b'):
        _, tr, _ = _three_steps(None)
        out[tag] = {b: getattr(tr, b).clone() for b in 'PMV'}
        assert tr.recorder is None
        del tr
    model, tr, rec = _three_steps(('P', 'G', 'M', 'V'))
    out['on'] = {b: getattr(tr, b).clone() for b in 'PMV'}
    reading = rec.read()
    out['reading'], out['entries'], out['touched'] = reading, [(n, g, o, k) for (n, p, g, o, k) in tr.entries], tr.touched.clone()
    out['norms'] = reading.grad_norms()
    out['torch_norms'] = {g: float(tr.grad_norm(*tr.group_range[g])) for g in tr.group_range}
    out['host_G'] = tr.G.cpu()
    before = {b: getattr(tr, b).clone() for b in 'PGMV'}
    rec.record()
    out['record_wrote'] = [b for b in 'PGMV' if not torch.equal(before[b], getattr(tr, b))]
    out['fp0'] = {b: rec.fingerprint(b) for b in 'PMV'}
    msd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    osd = tr.state_dict()
    model.load_state_dict(msd)
    tr.load_state_dict(osd)
    rec.record()
    out['fp1'] = {b: rec.fingerprint(b) for b in 'PMV'}
    images, mask, ids, attn = _batch()
    tr.train_step(nested(images, mask), (ids, attn), _targets())
    rec.record()
    out['fp2'] = {b: rec.fingerprint(b) for b in 'PMV'}
    assert rec.check() is None                                     # nothing non-finite so far
    # a NaN in G at a known parameter's offset + k, once the step's gradients are final and before step()
    i = max(j for j in range(len(tr.entries)) if tr.touched[j] and tr.entries[j][4] > 40)
    name, _, _, off, numel = tr.entries[i]
    exchange = tr.allreduce_grads

    def exchange_then_plant():
        exchange()
        tr.G[off + 37] = float('nan')
    tr.allreduce_grads = exchange_then_plant
    tr.train_step(nested(images, mask), (ids, attn), _targets())
    out['planted'] = (name, 37, rec.read().cursor - 1)
    try:
        rec.check()
        out['raised'] = None
    except health.NonFiniteError as err:
        out['raised'] = err
    return out


def test_trainer_with_the_recorder_on_trains_as_without_it(runs):
    """P, M, V after three steps.  Two plain runs of this trainer are bit-equal only where no float atomics are involved (the grouped
    weight gradients use them), so the comparison is chosen by measurement and printed: torch.equal when the two recorder-off runs
    are bit-equal to each other, otherwise the recorder-on run may differ from either of them by at most 3 x what they differ by
    (the factor the suite uses elsewhere for a spread measured from one pair).  Independent of that, one record() between two
    snapshots changes no bit of P, G, M, V."""
    assert runs['record_wrote'] == []
    for b in 'PMV':
        a, bb, on = runs['off_a'][b], runs['off_b'][b], runs['on'][b]
        spread = float((a - bb).abs().max())
        if spread == 0.0:
            print(f'{b}: recorder-off runs bit-equal -> torch.equal')
            assert torch.equal(on, a), b
        else:
            d = max(float((on - a).abs().max()), float((on - bb).abs().max()))
            print(f'{b}: recorder-off runs differ by {spread:.3e} -> compared against that spread, on-vs-off {d:.3e}')
            assert d <= 3.0 * spread, (b, d, spread)


def test_group_norms_equal_the_trainers_and_rows_equal_the_host_rule_on_real_gradients(runs):
    from gpv1_amd import health
    from gpv1_amd.train import GROUPS
    norms = runs['norms']
    assert list(norms) == list(GROUPS)
    for g, ref in runs['torch_norms'].items():
        print(g, norms[g], ref)
        assert np.isfinite(norms[g]) and abs(norms[g] - ref) <= 1e-6 * ref, (g, norms[g], ref)
    reading, G = runs['reading'], runs['host_G']
    assert reading.commits == [0, 1, 2]
    for (n, g, o, k) in runs['entries'][::7]:                      # the last step's G is still in place: every 7th parameter
        assert reading.row(n, 'G').tobytes() == health.segment_stats_host(G[o:o + k]).tobytes(), n


def test_a_parameter_without_gradient_reads_all_zero(runs):
    dead = [e for e, t in zip(runs['entries'], runs['touched']) if not t]
    assert dead, 'the run was meant to leave the box heads without a gradient'
    for (n, g, o, k) in dead:
        row = runs['reading'].row(n, 'G')
        assert int(row['n_zero']) == k and float(row['sumsq']) == 0.0 and float(row['absmax']) == 0.0, (n, row)
    live = [e for e, t in zip(runs['entries'], runs['touched']) if t]
    assert any(int(runs['reading'].row(n, 'G')['n_zero']) < k for (n, g, o, k) in live)


def test_a_nan_in_G_is_named_by_parameter_buffer_index_and_kind(runs):
    from gpv1_amd import health
    err, (name, k, commit) = runs['raised'], runs['planted']
    assert isinstance(err, health.NonFiniteError)
    assert (err.name, err.buffer, err.index, err.kind, err.commit, err.step) == (name, 'G', k, 'nan', commit, commit)
    assert name in str(err)


def test_fingerprint_survives_a_checkpoint_round_trip_and_moves_with_a_step(runs):
    for b in 'PMV':
        assert runs['fp0'][b].dtype == np.uint64 and len(runs['fp0'][b]) == len(runs['entries'])
        assert np.array_equal(runs['fp0'][b], runs['fp1'][b]), b
    assert not np.array_equal(runs['fp1']['P'], runs['fp2']['P'])
    moved = runs['fp1']['P'] != runs['fp2']['P']
    dead = ~runs['touched'].numpy()
    assert dead.any() and not moved[dead].any() and moved[~dead].sum() > 0.9 * (~dead).sum()      # only parameters that took a step moved


# ---- driver ----

def test_driver_logs_four_group_norms_and_reports_a_planted_nan(tmp_path, monkeypatch):
    """training.health present: the log line carries four finite group norms; a NaN planted in G in step 3 is latched, written to
    ckpt_dir/nonfinite_report.json with the parameter's name, and raised (on_nonfinite = 'raise')"""
    import gpv1_amd.ops as ops
    from gpv1_amd import health, train_distr as td
    from gpv1_amd.train import FlatTrainer, GROUPS
    from tests.test_drivers_cpu import _driver_cfg, _dataset
    from tests.test_model_cpu import V
    ops.RT.set_precise(False)
    cfg = _driver_cfg(tmp_path, health={'every': 1, 'ring': 8, 'watch': ['G'], 'on_nonfinite': 'raise'})
    exchange, seen = FlatTrainer.allreduce_grads, {'steps': 0}

    def exchange_then_plant(self):
        exchange(self)
        seen['steps'] += 1
        if seen['steps'] == 3:
            name, _, _, off, numel = self.entries[-1]
            seen['name'] = name
            self.G[off + numel - 1] = float('nan')
    monkeypatch.setattr(FlatTrainer, 'allreduce_grads', exchange_then_plant)
    logs = []
    with pytest.raises(health.NonFiniteError) as info:
        td.train_worker(cfg, dataset=_dataset(synth.make_vocab(V)), device=DEV, log=logs.append)
    lines = [l for l in logs if l.startswith('epoch')]
    assert len(lines) == 3
    for l in lines[:2]:
        m = re.search(r's gnorm ' + ' '.join(g + r' (\S+)' for g in GROUPS) + '$', l)
        assert m, l
        assert all(np.isfinite(float(v)) for v in m.groups()), l
    rep = json.load(open(os.path.join(cfg.ckpt_dir, 'nonfinite_report.json')))
    assert rep['trip']['name'] == seen['name'] == info.value.name and rep['trip']['buffer'] == 'G' and rep['trip']['kind'] == 'nan'
    assert rep['trip']['commit'] == 2 and rep['trip']['index'] == rep['numel'] - 1
    assert [r['commit'] for r in rep['rows']] == [0, 1, 2] and [r['n_nan'] for r in rep['rows']] == [0, 0, 1]
