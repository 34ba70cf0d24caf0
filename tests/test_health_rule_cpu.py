"""The flight recorder's rule on the host (gpv1_amd.health.segment_stats_host, ring_commit_host) against a second, naive
restatement: one Python loop per element, math.fsum, np.isnan and plain Python integers.  The GPU test (test_health_gpu.py)
compares the kernels with the host rule bit for bit; this file is what makes the host rule worth comparing against."""
import math

import numpy as np
import pytest
import torch

from tests.health_cases import LENGTHS, VARIANTS, make_bits, widen


def naive_stats(bits):
    vals = [float(v) for v in widen(bits)]                       # fp32 -> Python float is exact
    n_nan = n_inf = n_zero = 0
    first_bad, first_kind = -1, None
    absmax = 0.0
    squares = []
    for j, v in enumerate(vals):
        if np.isnan(v):
            n_nan += 1
        elif np.isinf(v):
            n_inf += 1
        else:
            if v == 0.0:
                n_zero += 1
            absmax = max(absmax, abs(v))
            squares.append(v * v)                                # exact: 24 x 24 significand bits fit in 53
            continue
        if first_bad < 0:
            first_bad, first_kind = j, ('nan' if np.isnan(v) else 'inf')
    bits_sum = 0
    for b in bits:
        bits_sum += int(b)
    return {'n_nan': n_nan, 'n_inf': n_inf, 'n_zero': n_zero, 'first_bad': first_bad, 'first_kind': first_kind, 'absmax': absmax,
            'sumsq': math.fsum(squares), 'bits_sum': bits_sum % (1 << 64)}


@pytest.mark.parametrize('bf16', [False, True], ids=['fp32', 'bf16'])
@pytest.mark.parametrize('n', LENGTHS)
def test_host_rule_equals_naive_restatement(n, bf16):
    from gpv1_amd import health
    for k, variant in enumerate(VARIANTS):
        bits = make_bits(n, bf16, variant, seed=1000 * k + n % 997)
        row = health.segment_stats_host(bits if bf16 else bits.view(np.float32), dtype='bf16' if bf16 else None)
        ref = naive_stats(bits)
        tag = (n, bf16, variant)
        for f in ('n_nan', 'n_inf', 'n_zero', 'first_bad', 'bits_sum'):
            assert int(row[f]) == ref[f], (tag, f, int(row[f]), ref[f])
        assert health.KINDS[int(row['first_kind'])] == ref['first_kind'], tag
        assert float(row['absmax']) == ref['absmax'], (tag, float(row['absmax']), ref['absmax'])
        # float64, at most 2^27 terms, every term exact: far inside 1e-12 relative of the correctly rounded sum (not a measurement)
        assert abs(float(row['sumsq']) - ref['sumsq']) <= 1e-12 * ref['sumsq'], (tag, float(row['sumsq']), ref['sumsq'])
        assert int(row['reserved']) == 0
        if n == 0:
            assert row.tobytes() == np.array((0, 0, 0, -1, 0.0, 0, 0.0, 0, 0), health.ROW).tobytes()


def test_host_rule_takes_torch_tensors_and_classifies_the_planted_values():
    from gpv1_amd import health
    x = torch.tensor([1.0, -0.0, float('inf'), float('nan'), 3.0, 0.0, -float('inf')])
    for t in (x, x.to(torch.bfloat16)):
        r = health.segment_stats_host(t)
        assert (int(r['n_nan']), int(r['n_inf']), int(r['n_zero']), int(r['first_bad']), int(r['first_kind'])) == (1, 2, 2, 2, 2)
        assert float(r['absmax']) == 3.0 and float(r['sumsq']) == 10.0
    assert int(health.segment_stats_host(x)['bits_sum']) == sum(int(b) for b in x.numpy().view(np.uint32))
    xb = x.to(torch.bfloat16)                                    # (the cast picks its own NaN pattern: take the bits from the result)
    assert int(health.segment_stats_host(xb)['bits_sum']) == sum(int(b) for b in xb.view(torch.int16).numpy().view(np.uint16))
    with pytest.raises(TypeError):
        health.segment_stats_host(np.zeros(3, np.float64))


def test_bits_sum_wraps_modulo_2_64_and_ignores_order():
    from gpv1_amd import health
    bits = np.full(3, 0xffffffff, np.uint32)
    assert int(health.segment_stats_host(bits.view(np.float32))['bits_sum']) == 3 * 0xffffffff
    rs = np.random.RandomState(3)
    b = rs.randint(0, 1 << 32, 70000, dtype=np.uint64).astype(np.uint32)
    a = health.segment_stats_host(b.view(np.float32))
    c = health.segment_stats_host(b[rs.permutation(b.size)].view(np.float32))
    assert int(a['bits_sum']) == int(c['bits_sum']) == sum(int(v) for v in b) % (1 << 64)
    # the wrap itself, on the accumulator the rule uses
    assert int(np.array([(1 << 64) - 1, 5], np.uint64).sum(dtype=np.uint64)) == 4


def test_sumsq_order_is_the_pinned_one_not_just_close():
    """a case where the order shows in the last bits: the rule's result equals a literal per-element walk of the pinned order"""
    from gpv1_amd import health
    n = 2 * 16384 + 77
    rs = np.random.RandomState(5)
    x = (rs.standard_normal(n) * np.exp(rs.uniform(-20, 20, n))).astype(np.float32)
    total = 0.0
    for b0 in range(0, n, 16384):
        lanes = [0.0] * 256
        for j in range(min(16384, n - b0)):
            v = float(x[b0 + j])
            lanes[(j >> 2) & 255] += v * v
        stride = 128
        while stride >= 1:
            for l in range(stride):
                lanes[l] += lanes[l + stride]
            stride //= 2
        total += lanes[0]
    assert float(health.segment_stats_host(x)['sumsq']) == total


def _rows(S, bad=None):
    from gpv1_amd import health
    rows = np.zeros(S, health.ROW)
    rows['first_bad'] = -1
    rows['sumsq'] = np.random.RandomState(S).rand(S)
    for s, (idx, kind, n_nan, n_inf) in (bad or {}).items():
        rows[s]['first_bad'], rows[s]['first_kind'], rows[s]['n_nan'], rows[s]['n_inf'] = idx, kind, n_nan, n_inf
    return rows


def test_ring_and_latch_model_wraps_and_the_first_trip_wins():
    from gpv1_amd import health, hip_health as hh
    R, S = 4, 3
    state, stamps, ring = health.new_ring_host(R, S)
    assert list(stamps) == [-1] * R and not state.any()
    sent = []
    for c in range(10):
        bad = {5: {2: (7, hh.NAN, 1, 0), 1: (11, hh.INF, 0, 2)}, 9: {0: (3, hh.NAN, 4, 0)}}.get(c)
        rows = _rows(S, bad)
        rows['n_zero'] = c                                       # every commit's rows are distinguishable
        sent.append(rows.copy())
        health.ring_commit_host(state, stamps, ring, rows)
        assert int(state[hh.ST_CURSOR]) == c + 1
        if c < 5:
            assert int(state[hh.ST_LATCHED]) == 0 and int(state[hh.ST_TRIPS]) == 0
    # wrap-around: the ring holds the last R commits, each in slot c % R
    assert sorted(stamps) == [6, 7, 8, 9]
    for c in range(6, 10):
        assert stamps[c % R] == c and ring[c % R].tobytes() == sent[c].tobytes()
    # first trip wins (commit 5, lowest segment index 1, its first_bad and kind); later trips are only counted
    assert [int(state[i]) for i in (hh.ST_LATCHED, hh.ST_TRIP_CURSOR, hh.ST_TRIP_SEG, hh.ST_TRIP_INDEX, hh.ST_KIND, hh.ST_TRIPS)] == \
        [1, 5, 1, 11, hh.INF, 2]
    assert int(state[7]) == 0


def test_recorder_refuses_the_cpu():
    """no CPU fallback: the recorder is a GPU object (the host rule above is the CPU statement)"""
    from gpv1_amd import health
    with pytest.raises(RuntimeError):
        health.FlightRecorder(watch=(), device='cpu')
    with pytest.raises(ValueError):
        health.FlightRecorder(watch=('G',))                       # a flat buffer without a trainer
