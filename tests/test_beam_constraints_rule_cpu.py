"""The constraints of the beam step rule on the host (gpv1_amd.beam: no repeated n-gram, minimum length, repetition penalty), no GPU:
banned_tokens against a brute-force restatement and against the processors of `transformers` where that is installed, the three
switches off against the rule without them, one step worked out by hand, the penalty's arithmetic, whole searches on constant logits,
and every refusal the Python layer makes before anything touches the device."""
import itertools

import numpy as np
import pytest
import torch

from tests import cpu_shim
from tests.beam_cases import make_case, same, PLANTS as BASE_PLANTS
from tests.beam_constraint_cases import make_constrained_case, PLANTS
from tests.test_model_cpu import build_small, V


def _brute(h, n):
    """every n-gram of h + [w] that ends at the new token and already occurs in h bans w"""
    h = list(h)
    if n < 1:
        return set()
    grams = {tuple(h[i:i + n]) for i in range(len(h) - n + 1)}
    tail = tuple(h[len(h) - (n - 1):]) if n > 1 else ()
    if len(tail) != n - 1:
        return set()
    return {w for w in set(h) if tail + (w,) in grams}


def test_banned_tokens_equals_a_brute_force_restatement():
    from gpv1_amd import beam as rule
    rs = np.random.RandomState(0)
    hits = 0
    for _ in range(4000):
        Vc, t, n = rs.randint(2, 7), rs.randint(0, 14), rs.randint(0, 6)
        h = rs.randint(0, Vc, t).tolist()
        got = rule.banned_tokens(h, n)
        assert got == _brute(h, n), (h, n)
        assert len(got) <= max(t - n + 1, 0)
        hits += bool(got)
    assert hits > 1000                                              # (the small alphabets do repeat)
    assert rule.banned_tokens([], 1) == set() and rule.banned_tokens([5], 1) == {5} and rule.banned_tokens([5], 2) == set()
    assert rule.banned_tokens([1, 2, 1], 2) == {2} and rule.banned_tokens([1, 2, 3, 1, 2], 3) == {3}
    assert rule.banned_tokens(np.asarray([4, 4, 4], np.int64), 2) == {4}


def test_banned_tokens_and_min_length_equal_the_transformers_processors():
    tf = pytest.importorskip('transformers')
    from gpv1_amd import beam as rule
    rs = np.random.RandomState(1)
    for _ in range(1200):
        Vc, t, n = int(rs.randint(2, 7)), int(rs.randint(0, 14)), int(rs.randint(1, 5))
        h = rs.randint(0, Vc, t).tolist()
        scores = tf.NoRepeatNGramLogitsProcessor(n)(torch.tensor([h], dtype=torch.long), torch.zeros(1, Vc))
        assert set(torch.nonzero(torch.isinf(scores[0])).flatten().tolist()) == rule.banned_tokens(h, n), (h, n)
    # (ii): __stop__ is banned while length < min_len; the processor bans the end token while cur_len < min_length
    stop = 3
    for m in range(0, 6):
        proc = tf.MinLengthLogitsProcessor(m, eos_token_id=stop) if m > 0 else None
        for length in range(0, 7):
            banned = length < m
            if proc is not None:
                scores = proc(torch.zeros(1, length, dtype=torch.long), torch.zeros(1, 5))
                assert bool(torch.isinf(scores[0, stop])) == banned and torch.isinf(scores).sum() == int(banned)
            x = np.zeros((1, 5), np.float32)
            x[0, stop] = 1.0
            o = rule.beam_step_host(x, np.zeros(1, np.float32), np.zeros((1, 1), np.float32), np.zeros((1, 1, 8), np.int64), np.zeros((1, 1), np.int32),
                                    np.full((1, 1), length, np.int32), min(length, 6), rule.EXTEND, 0, stop, min_length=m)
            assert (int(o['tok'][0]) != stop) == banned


def test_all_three_off_is_the_rule_without_the_keywords_bit_for_bit():
    from gpv1_amd import beam as rule
    n = 0
    for K, Vc, Bc in ((1, 37, 1), (3, 300, 2), (5, 37, 3), (8, 300, 1)):
        for vi, var in enumerate((dict(), dict(plants=BASE_PLANTS), dict(masked=True), dict(penalty=0.6, plants=BASE_PLANTS, masked=True))):
            for t in (0, 1, 4):
                case = make_case(31 * K + vi + t, Bc, K, Vc, 6, t, torch.bfloat16 if vi % 2 else torch.float32, **var)
                lse = rule.lse_host(case['x'], case['vocab_mask'])
                for mode in (rule.EXTEND, rule.FREEZE):
                    args = (case['x'], lse, case['seq_lp'], case['seqs'], case['finished'], case['length'], t, mode, case['pad_id'], case['stop_id'])
                    kw = dict(inv_pen=case['inv_pen'], vocab_mask=case['vocab_mask'])
                    ok, what = same(rule.beam_step_host(*args, **kw), rule.beam_step_host(*args, no_repeat_ngram=0, min_length=0, repetition=None, **kw))
                    assert ok, what
                    n += 1
    assert n == 96
    assert rule.rep_factors(None) is None and rule.rep_factors(1.0) is None


def test_one_step_worked_out_by_hand():
    """V = 6 (0 __pad__, 1 __stop__, 2..5 words), K = 2, B = 1, T = 6, t = 3, lse handed in as 0 (the logits are the log-probabilities),
    theta = 2: rep_neg = 2, rep_pos = 0.5, every product exact.
    parent 0: h = [2, 3, 2], seq_lp -1, length 3.  n = 2: the tail [2] occurs at i = 0, followed by 3: banned {3}; min_len = 4 > 3 bans
      __stop__ too.  Row [-8, 3, 1, 2.5, -0.75, -2]: seen {2, 3} -> x_2 = 0.5, x_3 = 1.25; after the bans the best two are 2 (0.5) and
      4 (-0.75): scores -0.5 and -1.75.
    parent 1: h = [4, 5, 5], seq_lp -0.25, length 3.  the tail [5] occurs at i = 1, followed by 5: banned {5}, and __stop__.  Row
      [-8, -1, -0.5, -1.5, -0.25, 4]: seen {4, 5} -> x_4 = -0.5, x_5 = 2; the best two that are not banned: 2 (-0.5, the lower index
      of the tie with 4) and 4 (-0.5): scores -0.75 and -0.75.
    selection: (-0.5, parent 0, token 2), then the tie at -0.75 goes to the lower k1*K + k2: (parent 1, token 2)."""
    from gpv1_amd import beam as rule
    x = np.asarray([[-8, 3, 1, 2.5, -0.75, -2], [-8, -1, -0.5, -1.5, -0.25, 4]], np.float32)
    seqs = np.zeros((2, 1, 6), np.int64)
    seqs[0, 0, :3], seqs[1, 0, :3] = [2, 3, 2], [4, 5, 5]
    o = rule.beam_step_host(x, np.zeros(2, np.float32), np.asarray([[-1.0, -0.25]], np.float32), seqs, np.zeros((1, 2), np.int32),
                            np.full((1, 2), 3, np.int32), 3, rule.FREEZE, 0, 1, no_repeat_ngram=2, min_length=4, repetition=rule.rep_factors(2.0))
    assert rule.rep_factors(2.0) == (np.float32(2.0), np.float32(0.5))
    assert o['parent'].tolist() == [[0, 1]] and o['tok'].tolist() == [2, 2]
    assert o['seq_lp'].tolist() == [[-0.5, -0.75]]
    assert o['seqs'][:, 0].tolist() == [[2, 3, 2, 2, 0, 0], [4, 5, 5, 2, 0, 0]]
    assert o['finished'].tolist() == [[0, 0]] and o['length'].tolist() == [[4, 4]]
    # without the constraints the same state takes __stop__ (3.0) from parent 0 and token 5 (4.0) from parent 1
    o = rule.beam_step_host(x, np.zeros(2, np.float32), np.asarray([[-1.0, -0.25]], np.float32), seqs, np.zeros((1, 2), np.int32),
                            np.full((1, 2), 3, np.int32), 3, rule.FREEZE, 0, 1)
    assert o['tok'].tolist() == [5, 1] and o['seq_lp'].tolist() == [[3.75, 2.0]] and o['finished'].tolist() == [[0, 1]]


def test_penalty_is_one_multiply_per_distinct_seen_token():
    from gpv1_amd import beam as rule
    rep = rule.rep_factors(1.3)
    assert rep == (np.float32(1.3), np.float32(1.0 / 1.3)) and rule.rep_factors(0.8) == (np.float32(0.8), np.float32(1.25))
    x = np.asarray([[1.7, -2.3, 0.0, -np.inf, 5.1, -0.3, 0.9]], np.float32)
    seqs = np.zeros((1, 1, 8), np.int64)
    seqs[0, 0, :6] = [0, 1, 1, 2, 3, 0]                              # tokens 0 and 1 twice: still one multiply
    got = rule.penalised_rows(x, seqs, np.zeros((1, 1), np.int32), 6, rule.EXTEND, rep)
    want = x.copy()
    want[0, 0], want[0, 1], want[0, 2] = x[0, 0] * rep[1], x[0, 1] * rep[0], np.float32(0.0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and got[0, 3] == -np.inf
    assert np.array_equal(got[0, 4:], x[0, 4:])                     # unseen tokens untouched
    assert np.array_equal(x[0, :3], np.asarray([1.7, -2.3, 0.0], np.float32))        # (the input is not modified)
    # a frozen parent is exempt; positions behind t are not history
    assert np.array_equal(rule.penalised_rows(x, seqs, np.ones((1, 1), np.int32), 6, rule.FREEZE, rep), x)
    assert np.array_equal(rule.penalised_rows(x, seqs, np.ones((1, 1), np.int32), 6, rule.EXTEND, rep), got)
    assert np.array_equal(rule.penalised_rows(x, seqs, np.zeros((1, 1), np.int32), 1, rule.EXTEND, rep)[0, 1:], x[0, 1:])


def test_every_plant_of_the_helper_is_in_place():
    """the helper's plants do what their names say, so that the GPU test's cases are the ones it means"""
    from gpv1_amd import beam as rule
    from tests.beam_constraint_cases import banned_of
    found = dict.fromkeys(PLANTS, 0)
    for seed in range(12):
        case = make_constrained_case(seed, 2, 3, 300, 8, 6, torch.bfloat16, plants=PLANTS, masked=seed % 2 == 1, n=2, min_len=8, theta=1.3)
        assert set(np.unique(case['seqs'][:, :, :6])) <= set(case['alphabet'].tolist())
        x = case['x'] if case['vocab_mask'] is None else case['x'] + case['vocab_mask'][None, :]
        if case['vocab_mask'] is not None:
            assert np.isfinite(case['vocab_mask']).sum() >= 3 + 8
        xp = rule.penalised_rows(x, case['seqs'], case['finished'], 6, rule.EXTEND, case['constr']['repetition'])
        signs = set()
        for r in range(6):
            banned = banned_of(case, r, 2, 8, rule.EXTEND)
            assert case['stop_id'] in banned
            top = int(np.argmax(xp[r]))
            found['ban_max'] += top in banned and xp[r, top] - np.sort(xp[r])[-2] > 50
            found['stop_top'] += int(np.argmax(x[r])) == case['stop_id'] or x[r, case['stop_id']] >= np.sort(x[r])[-3]
            found['ban_tie'] += any(xp[r, w] == xp[r, u] and np.isfinite(xp[r, w]) for w in banned for u in range(w + 1, 300) if u not in banned)
            for v in set(case['seqs'][r // 2, r % 2, :6].tolist()):
                signs.add('inf' if np.isinf(case['x'][r, v]) else int(np.sign(case['x'][r, v])))
        found['seen_both_signs'] += signs >= {1, -1, 0, 'inf'}
    assert all(v >= 6 for v in found.values()), found


def _constant_search(**kw):
    from gpv1_amd import beam as rule
    Vc, K, T = 12, 3, 9
    pad, stop, cls = 0, 1, 2
    row = np.asarray([-9.0, -2.0, -9.0, 3.0, 2.5, 2.0, 1.0, 0.5, 0.0, -0.5, -1.0, -1.5], np.float32)
    return rule.beam_search_host(lambda t, tok: np.tile(row, (K * 2, 1)), 2, K, T, cls, pad, stop, **kw), stop, T


def test_searches_on_constant_logits():
    from gpv1_amd import beam as rule
    out, stop, T = _constant_search()
    body = out['seqs'][:, :, :T - 1]
    assert all(len(set(body[k, b].tolist())) < T - 1 for k in range(3) for b in range(2))           # unconstrained: the hypotheses repeat
    out, _, _ = _constant_search(no_repeat_ngram=1)
    body = out['seqs'][:, :, :T - 1]
    assert all(len(set(body[k, b].tolist())) == T - 1 for k in range(3) for b in range(2))          # n = 1: every token distinct
    out, _, _ = _constant_search(no_repeat_ngram=2)
    for k, b in itertools.product(range(3), range(2)):
        h = out['seqs'][k, b, :T - 1].tolist()
        grams = list(zip(h[:-1], h[1:]))
        assert len(set(grams)) == len(grams), h                                                     # n = 2: no bigram twice
        assert len(set(h)) < len(h)                                                                 # (tokens may repeat)
    # min_length: __stop__ made the best token, never before position m
    for m in (0, 3, 8):
        for mode in (rule.EXTEND, rule.FREEZE):
            Vc, K, T = 12, 3, 9
            row = np.asarray([-9.0, 4.0, -9.0, 3.0, 2.5, 2.0, 1.0, 0.5, 0.0, -0.5, -1.0, -1.5], np.float32)
            out = rule.beam_search_host(lambda t, tok: np.tile(row, (K, 1)), 1, K, T, 2, 0, 1, mode=mode, min_length=m)
            firsts = [h.index(1) if 1 in h else T for h in (out['seqs'][k, 0, :T - 1].tolist() for k in range(K))]
            assert min(firsts) >= m and (m == 8 or min(firsts) == m), (m, mode, firsts)
    # the penalty lowers a repeated token's logit step by step: fewer repeats than without it, scores as the rule computes them
    plain, _, _ = _constant_search()
    pen, _, _ = _constant_search(repetition=rule.rep_factors(4.0))
    count = lambda o: sum(len(set(o['seqs'][k, b, :T - 1].tolist())) for k in range(3) for b in range(2))
    assert count(pen) > count(plain)


def test_out_of_range_values_are_refused():
    from gpv1_amd import beam as rule
    case = make_case(3, 1, 2, 37, 6, 2)
    args = (case['x'], rule.lse_host(case['x']), case['seq_lp'], case['seqs'], case['finished'], case['length'], 2, rule.EXTEND, 33, 35)
    for kw, match in ((dict(no_repeat_ngram=9), 'no_repeat_ngram'), (dict(no_repeat_ngram=-1), 'no_repeat_ngram'), (dict(min_length=-1), 'min_length'),
                      (dict(min_length=7), 'min_length'), (dict(repetition=(1.3, 0.0)), 'repetition'), (dict(repetition=(0.0, 1.3)), 'repetition'),
                      (dict(repetition=(float('inf'), 1.0)), 'repetition'), (dict(repetition=(-1.0, -1.0)), 'repetition'),
                      (dict(repetition=(float('nan'), 1.0)), 'repetition')):
        with pytest.raises(ValueError, match=match):
            rule.beam_step_host(*args, **kw)
        with pytest.raises(ValueError, match=match):
            rule.check_constraints(37, 6, **kw)
    for theta in (0.0, -2.0, float('inf'), float('nan')):
        with pytest.raises(ValueError, match='repetition penalty'):
            rule.rep_factors(theta)
    with pytest.raises(ValueError, match='GPV_BEAM_MAX_CONSTR_V'):
        rule.check_constraints(65537, 6, no_repeat_ngram=1)
    assert rule.check_constraints(65537, 6) is False and rule.check_constraints(65536, 6, min_length=6) is True
    assert (rule.MAX_NGRAM, rule.MAX_CONSTR_V) == (8, 65536)


def test_hip_beam_step_refuses_before_it_touches_the_device():
    """the binding checks the constraints' extents with the shapes, before any pointer is taken (CPU tensors would be refused next)"""
    from gpv1_amd import hip_beam
    z = lambda *s, d=torch.int32: torch.zeros(*s, dtype=d)

    class OnGpu(torch.Tensor):                                       # a CPU tensor that claims to be on the GPU: only the checks run
        is_cuda = True
    lg = torch.zeros(6, 40).as_subclass(OnGpu)
    args = (lg, z(6, d=torch.float32), z(2, 3, d=torch.float32), z(3, 2, 6, d=torch.long), z(6, d=torch.long), z(2, 3), z(2, 3), z(2, 3), 1, 0, 36, 38)
    for kw, match in ((dict(no_repeat_ngram=9), 'no_repeat_ngram'), (dict(min_length=-1), 'min_length'), (dict(repetition=(1.3, 0.0)), 'repetition')):
        with pytest.raises(ValueError, match=match):
            hip_beam.step(*args, **kw)
    with pytest.raises(ValueError, match='GPV_BEAM_MAX_CONSTR_V'):
        hip_beam.step(torch.zeros(6, 65537).as_subclass(OnGpu), *args[1:], no_repeat_ngram=1)
    assert [f[0] for f in hip_beam.BeamArgs._fields_[-4:]] == ['no_repeat', 'min_len', 'rep_neg', 'rep_pos']


@pytest.fixture()
def shim():
    import gpv1_amd.ops as ops
    undo = cpu_shim.install()
    ops.RT.set_precise(True)
    yield
    ops.RT.set_precise(False)
    undo()


def test_model_refuses_before_anything_runs(shim):
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    from gpv1_amd.phrases import PhraseSet
    model, _ = build_small()
    model.eval()
    imgs = nested_tensor_from_tensor_list([torch.zeros(3, 64, 96)])
    g = torch.Generator().manual_seed(0)
    q = (torch.randint(1000, 30000, (1, 5), generator=g), torch.ones(1, 5, dtype=torch.long))
    T = model.cfg.max_text_len
    for kw in (dict(no_repeat_ngram=2), dict(min_length=2), dict(repetition_penalty=1.3)):
        with pytest.raises(ValueError, match="need impl='device'"):                      # the torch path is not taught new rules
            model.forward_beam_search(imgs, q, beam_size=2, impl='torch', **kw)
        with pytest.raises(ValueError, match='phrases and no_repeat_ngram'):
            model.forward_beam_search(imgs, q, beam_size=2, phrases=PhraseSet.from_texts(model, ['w3 w4', 'w5']), **kw)
    for kw, match in ((dict(no_repeat_ngram=9), 'no_repeat_ngram'), (dict(min_length=T + 1), 'min_length'), (dict(min_length=-1), 'min_length'),
                      (dict(repetition_penalty=0.0), 'repetition penalty'), (dict(repetition_penalty=-1.5), 'repetition penalty')):
        with pytest.raises(ValueError, match=match):
            model.forward_beam_search(imgs, q, beam_size=2, impl='device', **kw)
    # the caller condition: the mask leaves K + T finite entries
    vm = torch.full((V,), -float('inf'))
    vm[:2 + T - 1] = 0.0
    with pytest.raises(ValueError, match=f'at least beam_size \\+ max_text_len = {2 + T}'):
        model.forward_beam_search(imgs, q, beam_size=2, impl='device', vocab_mask=vm, no_repeat_ngram=1)
    # the configuration's group is the fallback; off values are off: the torch path runs as ever
    model.cfg['beam'] = {'no_repeat_ngram': 2}
    with pytest.raises(ValueError, match="need impl='device'"):
        model.forward_beam_search(imgs, q, beam_size=2)
    model.cfg['beam'] = {'no_repeat_ngram': 0, 'min_length': 0, 'repetition_penalty': 1.0}
    out = model.forward_beam_search(imgs, q, beam_size=2, repetition_penalty=None)
    assert len(out['answers'][0]) == 2
    # a constrained call reaches hip_beam (which refuses CPU tensors: no fallback), an unconstrained one passes no new keyword
    with pytest.raises(RuntimeError, match='GPU'):
        model.forward_beam_search(imgs, q, beam_size=2, impl='device', no_repeat_ngram=2)


def test_drivers_map_the_beam_keys():
    from gpv1_amd import inference as inf
    assert inf.beam_options({'no_repeat_ngram': 3, 'min_length': 2, 'repetition_penalty': 1.2, 'impl': 'device'}) == \
        {'no_repeat_ngram': 3, 'min_length': 2, 'repetition_penalty': 1.2, 'impl': 'device'}
    assert inf.beam_options({'finished': 'freeze'}) == {'finished': 'freeze'} and inf.beam_options(None) == {}
