"""The sampled step's rule on the host (gpv1_amd.beam, THE SAMPLER), no GPU: against a second restatement in plain Python lists and
loops, its hash against tests/dropout_ref.py, the arg-max of top_k = 1, the nucleus boundaries by hand, the frequencies of 20 000 draws,
finished slots, and every refusal of check_sampler, hip_beam.sample_step, GPV.forward_sample and inference.predict before anything runs."""
import math

import numpy as np
import pytest
import torch

from tests import cpu_shim, dropout_ref
from tests.sample_cases import make_sample_case, host_inputs, same
from tests.test_model_cpu import build_small, V

F32 = np.float32


def _ref_step(x, lse, cand_w, seq_lp, seqs, finished, length, t, pad_id, stop_id, seed, C, top_p, inv_temp, vocab_mask, u=None):
    """the second restatement: Python lists and loops, np.float32 scalars for every rounded operation"""
    K, B = len(seqs), len(seqs[0])
    Vc = len(x[0])
    out = {'parent': [[k for k in range(K)] for _ in range(B)], 'tok': [0] * (K * B), 'seqs': [[list(s) for s in per] for per in seqs],
           'seq_lp': [[0.0] * K for _ in range(B)], 'finished': [[0] * K for _ in range(B)], 'length': [[0] * K for _ in range(B)],
           'cand_v': [[0] * C for _ in range(K * B)]}
    for b in range(B):
        for k in range(K):
            r = k * B + b
            row = []
            for v in range(Vc):
                xv = F32(x[r][v])
                if inv_temp is not None:
                    xv = F32(xv * F32(inv_temp))
                if vocab_mask is not None:
                    xv = F32(xv + F32(vocab_mask[v]))
                row.append(xv)
            left = list(range(Vc))
            cand = []
            for _ in range(C):                                       # C times the arg-max of what is left, the lower v on a tie
                best = left[0]
                for v in left[1:]:
                    if row[v] > row[best]:
                        best = v
                cand.append(best)
                left.remove(best)
            out['cand_v'][r] = cand
            lp = [F32(row[v] - F32(lse[r])) for v in cand]
            c, acc = [], F32(0.0)
            for j in range(C):
                acc = F32(acc + F32(cand_w[r][j]))
                c.append(acc)
            n = C
            if top_p is not None:
                n = 1
                for j in range(C - 1):
                    if c[j] < F32(top_p):
                        n += 1
            if u is None:
                bits = int(dropout_ref.hash_u32(seed, (t * B + b) * K + k))
                uu = F32(bits >> 8) * F32(2.0 ** -24)
            else:
                uu = F32(u[b][k])
            tau = F32(uu * c[n - 1])
            js = n - 1
            for j in range(n):
                if c[j] > tau:
                    js = j
                    break
            fin = bool(finished[b][k])
            tokv = pad_id if fin else cand[js]
            out['seq_lp'][b][k] = F32(seq_lp[b][k]) if fin else F32(F32(seq_lp[b][k]) + lp[js])
            out['seqs'][k][b][t] = tokv
            out['tok'][r] = tokv
            out['length'][b][k] = int(length[b][k]) + (0 if fin else 1)
            out['finished'][b][k] = int(fin or tokv == stop_id)
    return out


def test_host_rule_equals_second_restatement_exactly():
    """>= 200 random cases over K in {1,3,8}, V in {C,37,300}, C in {1,5,8,9,17,64} with C <= V, with and without temperature, mask
    and top_p; cand_w = np.exp(lp) rounded to fp32; every output equal, seq_lp as bit patterns"""
    from gpv1_amd import beam as rule
    n = 0
    for K in (1, 3, 8):
        for C in (1, 5, 8, 9, 17, 64):
            for Vc in sorted({C, 37, 300}):
                if C > Vc or K > Vc:
                    continue
                for rep in range(5):
                    Bc, T = 1 + rep % 2, 3 + (n % 5)
                    t = [0, 1, T - 2][rep % 3]
                    dtype = torch.bfloat16 if rep % 2 else torch.float32
                    case = make_sample_case(3000 + n, Bc, K, Vc, T, t, C, dtype, masked=(rep in (1, 4)))
                    inv_temp = rule.inv_temperature([None, 0.7, 1.3, None, 0.7][rep])
                    top_p = [None, 0.9, 0.5, 1e-6, 0.9][(rep + n) % 5]
                    seed = (0x1234567 << 32 | 77) + n
                    lse, w = host_inputs(case, inv_temp)
                    args = (case['x'], lse, w, case['seq_lp'], case['seqs'], case['finished'], case['length'], t, case['pad_id'], case['stop_id'], seed, C)
                    a = rule.sample_step_host(*args, top_p=top_p, inv_temp=inv_temp, vocab_mask=case['vocab_mask'])
                    b = _ref_step(case['x'].tolist(), lse.tolist(), w.tolist(), case['seq_lp'].tolist(), case['seqs'].tolist(),
                                  case['finished'].tolist(), case['length'].tolist(), t, case['pad_id'], case['stop_id'], seed, C, top_p,
                                  inv_temp, None if case['vocab_mask'] is None else case['vocab_mask'].tolist())
                    ok, what = same(a, b)
                    assert ok, (what, K, C, Vc, rep, a[what], b[what])
                    assert (a['parent'] == np.arange(K)[None, :]).all()
                    n += 1
    assert n >= 200, n


def test_hash_is_the_dropout_hash():
    """10 000 (seed, index) pairs, high words of both included"""
    from gpv1_amd import beam as rule
    rs = np.random.RandomState(3)
    idx = rs.randint(0, 2 ** 63 - 1, 10000, dtype=np.int64).astype(np.uint64) * np.uint64(2) + rs.randint(0, 2, 10000).astype(np.uint64)
    idx[:100] = np.arange(100, dtype=np.uint64)
    for i, seed in enumerate((0, 1, 0xFFFFFFFFFFFFFFFF, 0x9E3779B97F4A7C15, 2 ** 32, 12345)):
        lo, hi = i * 1700, min((i + 1) * 1700, 10000) if i < 5 else 10000
        assert np.array_equal(rule.hash_u32(seed, idx[lo:hi]), dropout_ref.hash_u32(seed, idx[lo:hi]))
    # one pair at a time, as the rule calls it, and u is the top 24 bits scaled exactly
    for s, i in ((5, 7), (2 ** 40 + 3, 2 ** 35 + 1)):
        bits = int(dropout_ref.hash_u32(s, i))
        assert int(rule.hash_u32(s, i)) == bits
    assert float(rule.draw_u(5, 1, 2, 1, 4, 3)) == (int(dropout_ref.hash_u32(5, (1 * 4 + 2) * 3 + 1)) >> 8) / 2.0 ** 24


def _one_row(weights, x=None):
    """a single slot (B = K = 1) whose candidates have the given weights -> the positional arguments of sample_step_host up to top_k"""
    C = len(weights)
    x = np.asarray([list(range(C, 0, -1)) + [-50.0, -50.0]] if x is None else x, F32)
    z = lambda *s, d=np.int32: np.zeros(s, d)
    return [x, z(1, d=F32), np.asarray([weights], F32), z(1, 1, d=F32), z(1, 1, 4, d=np.int64), z(1, 1), z(1, 1), 0, C, C + 1, 9, C]


def test_top_k_one_is_the_arg_max_whatever_u_is():
    from gpv1_amd import beam as rule
    x = np.full((1, 9), -2.0, F32)
    x[0, 6] = x[0, 2] = 3.0                                          # the maximum twice: the lower v
    for u in (0.0, 0.5, 1.0 - 2.0 ** -24):
        a = _one_row([0.25], x)
        a[8], a[9] = 7, 8
        o = rule.sample_step_host(*a, u=np.asarray([[u]], F32))
        assert o['tok'].tolist() == [2] and o['cand_v'].tolist() == [[2]] and o['pick'].tolist() == [[0]]
    for seed in range(20):
        a = _one_row([0.25], x)
        a[8], a[9], a[10] = 7, 8, seed
        assert rule.sample_step_host(*a)['tok'].tolist() == [2]


def test_nucleus_boundaries():
    from gpv1_amd import beam as rule
    w = [0.5, 0.25, 0.125, 0.0625]                                   # dyadic: every c_j is exact (0.5, 0.75, 0.875, 0.9375)
    n_of = lambda p: int(rule.sample_step_host(*_one_row(w), top_p=p)['n'][0, 0])
    assert n_of(None) == 4
    assert n_of(0.75) == 2                                           # c_1 == top_p exactly: not below it, so rank 2 is out
    assert n_of(float(np.nextafter(F32(0.75), F32(1)))) == 3
    assert n_of(0.3) == 1 and n_of(1e-6) == 1                        # top_p below w_0
    assert n_of(0.99) == 4                                           # never beyond C: j runs over 0 .. C-2
    # the draw: tau = u * c_{n-1}, the first c_j > tau
    pick = lambda u, p=None: int(rule.sample_step_host(*_one_row(w), top_p=p, u=np.asarray([[u]], F32))['pick'][0, 0])
    assert pick(0.0) == 0
    assert pick(0.5, 0.75) == 0                                      # n = 2, tau = 0.375 < c_0
    assert pick(0.6875, 0.75) == 1                                   # tau = 0.515625: c_0 = 0.5 is not above it
    assert pick(0.9375) == 3                                         # n = 4, tau = 0.87890625: c_2 = 0.875 is not above it, c_3 is
    # the fallback: no c_j > tau (u = 1 cannot come from 24 bits; it is handed in): j* = n - 1
    assert pick(1.0) == 3 and pick(1.0, 0.75) == 1 and pick(1.0, 0.3) == 0
    # tau equal to c_0 exactly: not above it, the next one
    o = rule.sample_step_host(*_one_row([0.5, 0.5]), u=np.asarray([[0.5]], F32))
    assert int(o['pick'][0, 0]) == 1


def test_frequencies_of_twenty_thousand_draws():
    """one fixed 6-candidate distribution, top_p = 0.85 keeps n = 4 of them; 20 000 draws over 50 steps t x 50 b x 8 k with ONE seed: every
    candidate's count within 5 binomial standard deviations of w_j / c_{n-1}.  Deterministic: the seed below passes with the rule alone."""
    from gpv1_amd import beam as rule
    w = np.asarray([0.4, 0.25, 0.15, 0.1, 0.06, 0.04], F32)
    c = np.cumsum(w, dtype=F32)                                      # 0.4, 0.65, 0.8, 0.9, ...: three of the first five lie below 0.85
    n = 4
    Bc, K, T, seed = 50, 8, 64, 20240229
    x = np.tile(np.asarray([6, 5, 4, 3, 2, 1, -50, -50], F32), (K * Bc, 1))
    z = lambda *s, d=np.int32: np.zeros(s, d)
    counts = np.zeros(6, np.int64)
    for t in range(50):
        o = rule.sample_step_host(x, z(K * Bc, d=F32), np.tile(w, (K * Bc, 1)), z(Bc, K, d=F32), z(K, Bc, T, d=np.int64), z(Bc, K), z(Bc, K),
                                  t, 6, 7, seed, 6, top_p=0.85)
        assert (o['n'] == n).all()
        counts += np.bincount(o['pick'].ravel(), minlength=6)
    N = 50 * Bc * K
    assert N == 20000 and counts.sum() == N and counts[n:].sum() == 0
    p = w[:n].astype(np.float64) / float(c[n - 1])
    for j in range(n):
        sd = math.sqrt(N * p[j] * (1 - p[j]))
        print('FREQ candidate %d: %d draws, expected %.1f, %.2f sd' % (j, counts[j], N * p[j], (counts[j] - N * p[j]) / sd))
        assert abs(counts[j] - N * p[j]) <= 5 * sd, (j, counts.tolist(), N * p[j], sd)


def test_finished_slot_emits_pad_and_keeps_score_and_length():
    from gpv1_amd import beam as rule
    case = make_sample_case(11, 2, 3, 37, 6, 2, 5)
    case['finished'][:] = 0
    case['finished'][1, 2] = 1
    case['length'][1, 2] = 1
    lse, w = host_inputs(case)
    o = rule.sample_step_host(case['x'], lse, w, case['seq_lp'], case['seqs'], case['finished'], case['length'], 2, case['pad_id'],
                              case['stop_id'], 5, 5)
    assert o['tok'][2 * 2 + 1] == case['pad_id'] and o['seqs'][2, 1, 2] == case['pad_id']
    assert o['seq_lp'][1, 2].view(np.uint32) == case['seq_lp'][1, 2].view(np.uint32) and o['length'][1, 2] == 1 and o['finished'][1, 2] == 1
    live = o['length'] == case['length'] + 1
    live[1, 2] = True
    assert live.all() and (o['seqs'][:, :, :2] == case['seqs'][:, :, :2]).all()


def test_check_sampler_refusals():
    from gpv1_amd import beam as rule
    rule.check_sampler(3, 40, 6, 1, 17, 0.9, rule.inv_temperature(0.7))
    for kw, match in ((dict(top_k=65), 'GPV_BEAM_MAX_C'), (dict(top_k=0), 'top_k'), (dict(top_k=41), 'exceeds the vocabulary'),
                      (dict(top_p=1.5), 'top_p'), (dict(top_p=0.0), 'top_p'), (dict(top_p=1.0), 'top_p'), (dict(inv_temp=-1.0), 'inv_temp'),
                      (dict(inv_temp=float('inf')), 'inv_temp'), (dict(inv_pen=np.ones(7, F32)), 'length penalty'),
                      (dict(no_repeat_ngram=2), 'no_repeat_ngram'), (dict(min_length=1), 'min_length'), (dict(repetition=(1.3, 0.7)), 'repetition'),
                      (dict(K=9), 'GPV_BEAM_MAX_K'), (dict(t=5), 'step 5 outside')):
        a = dict(K=3, V=40, T=6, t=1, top_k=17)
        a.update(kw)
        with pytest.raises(ValueError, match=match):
            rule.check_sampler(**a)
    for bad in (0.0, -1.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='use top_k=1'):
            rule.inv_temperature(bad)
    assert rule.inv_temperature(None) is None and rule.inv_temperature(1.0) is None and rule.inv_temperature(0.5) == F32(2.0)
    assert (rule.SAMPLE, rule.MAX_C) == (2, 64)


def test_binding_refuses_before_it_touches_the_device():
    """extents first (a CPU tensor that claims to be on the GPU: only the checks run), then CPU tensors: 'GPU'"""
    from gpv1_amd import hip_beam
    z = lambda *s, d=torch.int32: torch.zeros(*s, dtype=d)

    class OnGpu(torch.Tensor):
        is_cuda = True
    lg = torch.zeros(6, 40)
    args = lambda lg, C=5: (lg, z(6, d=torch.float32), z(2, 3, d=torch.float32), z(3, 2, 6, d=torch.long), z(6, d=torch.long), z(2, 3), z(2, 3), z(2, 3),
                            1, 36, 38, z(1, d=torch.long), z(6, C), z(6, C, d=torch.float32), C)
    for C, kw, match in ((65, {}, 'GPV_BEAM_MAX_C'), (41, {}, 'exceeds the vocabulary'), (5, dict(top_p=1.5), 'top_p'),
                         (5, dict(temperature=0.0), 'use top_k=1'), (5, dict(temperature=float('nan')), 'use top_k=1')):
        with pytest.raises(ValueError, match=match):
            hip_beam.sample_step(*args(lg.as_subclass(OnGpu), C), **kw)
    with pytest.raises(RuntimeError, match='GPU'):
        hip_beam.sample_step(*args(lg))
    with pytest.raises(TypeError):                                  # the beam's keywords are not the sampler's
        hip_beam.sample_step(*args(lg), inv_pen=None)
    import ctypes
    assert [f[0] for f in hip_beam.BeamArgs._fields_ if f[0] in ('seed', 'cand_v', 'cand_w', 'top_k', 'inv_temp', 'top_p')] == \
        ['seed', 'cand_v', 'cand_w', 'top_k', 'inv_temp', 'top_p'] and ctypes.sizeof(hip_beam.BeamArgs) == 176


@pytest.fixture()
def shim():
    import gpv1_amd.ops as ops
    undo = cpu_shim.install()
    ops.RT.set_precise(True)
    yield
    ops.RT.set_precise(False)
    undo()


def _query():
    g = torch.Generator().manual_seed(0)
    return (torch.randint(1000, 30000, (1, 5), generator=g), torch.ones(1, 5, dtype=torch.long))


def test_model_and_driver_refuse_before_anything_runs(shim, monkeypatch):
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    from gpv1_amd.phrases import PhraseSet
    from gpv1_amd import inference as inf
    model, _ = build_small()
    model.eval()
    ran = []
    monkeypatch.setattr(model, '_encode', lambda *a, **k: ran.append('encode'))
    imgs = nested_tensor_from_tensor_list([torch.zeros(3, 64, 96)])
    q = _query()
    for kw, match in ((dict(temperature=0.0), 'use top_k=1'), (dict(temperature=float('inf')), 'use top_k=1'), (dict(top_k=65), 'GPV_BEAM_MAX_C'),
                      (dict(top_k=V + 1), 'exceeds the vocabulary'), (dict(top_p=1.5), 'top_p'), (dict(num_samples=9), 'GPV_BEAM_MAX_K'),
                      (dict(num_samples=0), 'GPV_BEAM_MAX_K'),
                      (dict(vocab_mask=torch.full((V,), -float('inf'))), 'finite entries'),
                      (dict(length_penalty=0.6), 'length_penalty'), (dict(no_repeat_ngram=2), 'no_repeat_ngram'), (dict(min_length=2), 'min_length'),
                      (dict(repetition_penalty=1.3), 'repetition_penalty'), (dict(beam_size=3), 'beam_size'),
                      (dict(phrases=PhraseSet.from_texts(model, ['w1', 'w2 w3'])), 'phrases')):
        with pytest.raises(ValueError, match=match):
            model.forward_sample(imgs, q, **{'num_samples': 2, **kw})
    model.cfg['sample'] = {'top_k': 99}                             # the configuration's values are checked like the arguments
    with pytest.raises(ValueError, match='GPV_BEAM_MAX_C'):
        model.forward_sample(imgs, q, num_samples=2)
    with torch.no_grad():                                           # an argument, else cfg['sample'], else the defaults
        model.cfg['sample'] = {'top_k': 4, 'temperature': 0.8, 'top_p': 0.9}
        assert model._sample_options(2, None, None, None, None, {}) == (2, (0.8, float(F32(1.0 / 0.8))), 4, float(F32(0.9)))
        assert model._sample_options(2, 1.0, 7, 1.0, None, {}) == (2, None, 7, None)
        del model.cfg['sample']
        assert model._sample_options(3, None, None, None, None, {}) == (3, None, min(64, V), None)
    model.cfg['kv_decode'] = False
    with pytest.raises(RuntimeError, match='KV-cached'):
        model.forward_sample(imgs, q, num_samples=2)
    model.cfg['kv_decode'] = True
    model.train()
    with pytest.raises(RuntimeError, match='KV-cached'):
        model.forward_sample(imgs, q, num_samples=2)
    model.eval()
    # the driver: sample excludes a beam, a closed answer set and the beam's options, each with a reason
    img = (np.random.RandomState(0).rand(64, 96, 3) * 255).astype(np.uint8)
    for kw, match in ((dict(beam_size=5), 'beam_size=5'), (dict(answers=['w1', 'w2']), 'answers'), (dict(beam={'length_penalty': 0.6}), 'length_penalty')):
        with pytest.raises(ValueError, match=match):
            inf.predict(model, [img], q, sample={'num': 3, 'top_k': 5}, **kw)
    assert not ran


def test_without_a_gpu_sampling_is_an_error_not_a_fallback(shim):
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    model, _ = build_small()
    model.eval()
    imgs = nested_tensor_from_tensor_list([torch.zeros(3, 64, 96)])
    with pytest.raises(RuntimeError, match='GPU'):
        model.forward_sample(imgs, _query(), num_samples=2, top_k=5, seed=1)


def test_plain_device_beam_search_still_calls_step_with_todays_keywords(shim, monkeypatch):
    """hip_beam.step replaced by a recorder of today's signature: positional arguments as before, keywords exactly inv_pen and vocab_mask,
    one reorder per step but the last"""
    import gpv1_amd.hip_beam as hip_beam
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    from gpv1_amd import beam as rule
    model, _ = build_small()
    model.eval()
    calls = []

    def step(logits, lse, seq_lp, seqs, tok, parent, finished, length, t, mode, pad_id, stop_id, inv_pen=None, vocab_mask=None,
             no_repeat_ngram=0, min_length=0, repetition=None, **unknown):
        calls.append(('step', t, mode, sorted(unknown)))
        x = logits.float().numpy()
        o = rule.beam_step_host(x, rule.lse_host(x), seq_lp.numpy(), seqs.numpy(), finished.numpy(), length.numpy(), t, mode, pad_id, stop_id)
        for dst, k in ((seq_lp, 'seq_lp'), (seqs, 'seqs'), (tok, 'tok'), (parent, 'parent'), (finished, 'finished'), (length, 'length')):
            dst.copy_(torch.from_numpy(o[k]))

    def kwstep(*a, **kw):
        assert len(a) == 12 and sorted(kw) == ['inv_pen', 'vocab_mask'], (len(a), sorted(kw))
        return step(*a, **kw)
    monkeypatch.setattr(hip_beam, 'step', kwstep)
    monkeypatch.setattr(hip_beam, 'reorder', lambda caches, parent, upto: calls.append(('reorder', upto)))
    monkeypatch.setattr(hip_beam, 'sample_step', lambda *a, **k: calls.append(('sample',)))
    imgs = nested_tensor_from_tensor_list([torch.zeros(3, 64, 96)])
    model.forward_beam_search(imgs, _query(), beam_size=2, impl='device')
    T = model.cfg.max_text_len
    assert [c[1] for c in calls if c[0] == 'step'] == list(range(T - 1)) and all(c[2] == rule.EXTEND and not c[3] for c in calls if c[0] == 'step')
    assert [c[1] for c in calls if c[0] == 'reorder'] == list(range(1, T - 1)) and ('sample',) not in calls
