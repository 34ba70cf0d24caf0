"""Beam-5 decode of 64 images (BASELINE.json configs[3], bench.py extra.beam5_bs64): the torch path against the device path
(GPV.forward_beam_search impl='torch' / 'device', gpv-1_amd/csrc/beam_step.hip), the whole search one hipGraph.

  python tools/bench_beam.py [--out profiles/r13_beam.txt] [--passes 5] [--reps 3] [--no-trace]
                             [--no-repeat N] [--min-length M] [--repetition-penalty THETA]
                             [--sample N --top-k C [--top-p P]]

The two paths alternate in one process, `--passes` passes of `--reps` searches each (per-search wall time incl. the host detokenisation,
as bench.py times it); median and min - max of the passes are reported.  Then ONE `rocprofv3 --kernel-trace` run of a fresh child process
(`--child`: eager searches, so that every launch is a kernel record) gives the kernel launches per decode step of each path and the
durations of the two new kernels.  How the launches are counted: a device-path search has exactly one step_kernel per step, so the
records between two consecutive step_kernels are one step (decoder core + 2); the child runs device, device, torch, device searches, and
the records between the last step_kernel of one device search and the first of the next are (tail + head) without and with a torch
search in between -- the difference is the torch search, from which the head (encoder, cross-attention K | V, the first step's core) and
T - 1 decoder cores are taken off.

A last section times gpv_beam_step alone with device events at the search's shapes (B = 64, K = 5, the model's vocabulary, bf16 logits
of pitch T*V, the longest history t = T - 2).  --no-repeat / --min-length / --repetition-penalty (the constraints of gpv1_amd.beam) add
a third path to the alternation, the device path with these options, and to that section each given option alone and all together.
--sample N --top-k C [--top-p P] adds the sampled search (GPV.forward_sample: N draws per image, no reorder launches) to the alternation
and the sampled step alone (mode GPV_BEAM_SAMPLE, K = N) at C in {8, 20, 64} and the given C to that section."""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
K, BATCH = 5, 64


def setup():
    import torch
    import bench
    import gpv1_amd.hip as hip
    import gpv1_amd.hip_beam as hip_beam
    from gpv1_amd.gpv import GPV
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    hip.lib()
    hip_beam.lib()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = GPV(bench.make_cfg())
    for n, buf in model.named_buffers():
        if n.endswith('running_var'):
            buf.uniform_(0.5, 1.5)
    model.to(dev).eval()
    images, mask, ids, attn, _ = bench.make_batch(0, BATCH, dev)
    return torch, model, nested_tensor_from_tensor_list(images), (ids, attn)


def child():
    """eager searches for the kernel trace: torch, device (warm-up), then device, device, torch, device"""
    torch, model, samples, q = setup()
    model.cfg['graph_inference'] = False
    with torch.no_grad():
        for impl in ('torch', 'device', 'device', 'device', 'torch', 'device'):
            model._beam_device(samples, q, K, impl=impl)
            torch.cuda.synchronize()
    print('child ok')


def analyse(trace_dir, T):
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        return ['kernel trace: no *kernel_trace.csv was written']
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    steps = [i for i, r in enumerate(rows) if 'step_kernel' in r['Kernel_Name']]
    reord = [r for r in rows if 'reorder_kernel' in r['Kernel_Name']]
    n = T - 1
    if len(steps) != 4 * n:
        return [f'kernel trace: expected {4 * n} step_kernel records (4 device searches of {n} steps), found {len(steps)}']
    s = [steps[i * n:(i + 1) * n] for i in range(4)]
    per_step_dev = sorted({b - a for se in s[1:] for a, b in zip(se[1:-1], se[2:])})       # step 1 .. T-3: core + step + reorder
    core = per_step_dev[0] - 2
    gap_plain = s[2][0] - s[1][-1] - 1                     # tail of a device search + head of the next
    gap_torch = s[3][0] - s[2][-1] - 1                     # the same with one torch search in between
    torch_total = gap_torch - gap_plain
    head = s[2][0] - s[1][-1] - 1                          # (the device search's tail is empty: nothing follows the last step_kernel)
    torch_glue = torch_total - (head - core) - n * core
    out = [f'kernel launches per decode step (eager child, rocprofv3 --kernel-trace, {len(rows)} records):',
           f'  decoder core                      {core}',
           f'  device path: core + 2           = {per_step_dev}   (gpv_beam_step + gpv_beam_reorder; the last step has no reorder)',
           f'  torch path:  core + {torch_glue / n:.1f}        = {core + torch_glue / n:.1f}   ({torch_glue} glue launches in {n} steps: log_softmax, topk, sort, gathers, cat, copies, '
           f'index_select + copy_ per layer; incl. the few fills before step 0)',
           f'  removed per step: {torch_glue / n - 2:.1f} launches']
    sk = [dur(rows[i]) for se in s[1:] for i in se]
    out.append(f'gpv_beam_step   (B = {BATCH}, K = {K}, bf16 logits): median {statistics.median(sk):.1f} us, min {min(sk):.1f}, max {max(sk):.1f}  ({len(sk)} launches)')
    rk = [dur(r) for r in reord]
    if rk:
        per = len(rk) // 4
        first = [rk[i * per] for i in range(1, 4)]
        last = [rk[i * per + per - 1] for i in range(1, 4)]
        out.append(f'gpv_beam_reorder (3 layers, D = 768): upto = 1: {statistics.median(first):.1f} us, upto = {per}: {statistics.median(last):.1f} us, '
                   f'sum over one search {sum(rk[per:]) / 3:.0f} us  ({len(rk)} launches)')
    return out


def step_times(torch, V, T, variants, runs=7, launches=200):
    """gpv_beam_step alone, device events around `launches` launches, `runs` times -> {name: [us per launch]}; the variants alternate"""
    import gpv1_amd.hip_beam as hip_beam
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(0)
    t = T - 2
    buf = (3.0 * torch.randn(K * BATCH, T, V, generator=g)).to(torch.bfloat16).to(dev)
    alphabet = torch.randint(0, V - 4, (3,), generator=g)
    seqs0 = alphabet[torch.randint(0, 3, (K, BATCH, T), generator=g)].to(dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    out = {name: [] for name in variants}
    for _ in range(runs + 1):                                                # (the first round is the warm-up)
        for name, kw in variants.items():
            seq_lp, seqs, lse = torch.zeros(BATCH, K, device=dev), seqs0.clone(), torch.zeros(K * BATCH, device=dev)
            tok, parent, fin, length = torch.zeros(K * BATCH, dtype=torch.long, device=dev), i32(BATCH, K), i32(BATCH, K), i32(BATCH, K) + t
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                hip_beam.step(buf[:, t], lse, seq_lp, seqs, tok, parent, fin, length, t, 0, V - 4, V - 2, **kw)
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / launches * 1e3)
    return {name: ts[1:] for name, ts in out.items()}


def sample_step_times(torch, V, T, N, Cs, top_p, runs=7, launches=200):
    """the sampled step alone at the search's shapes (B = BATCH, K = N), device events around `launches` launches -> {C: [us per launch]}"""
    import gpv1_amd.hip_beam as hip_beam
    dev = torch.device('cuda:0')
    g = torch.Generator(device='cpu').manual_seed(0)
    t = T - 2
    buf = (3.0 * torch.randn(N * BATCH, T, V, generator=g)).to(torch.bfloat16).to(dev)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=dev)
    seed = torch.tensor([1], dtype=torch.long, device=dev)
    out = {c: [] for c in Cs}
    for _ in range(runs + 1):                                                # (the first round is the warm-up)
        for c in Cs:
            seq_lp, seqs, lse = torch.zeros(BATCH, N, device=dev), torch.zeros(N, BATCH, T, dtype=torch.long, device=dev), torch.zeros(N * BATCH, device=dev)
            tok, parent, fin, length = torch.zeros(N * BATCH, dtype=torch.long, device=dev), i32(BATCH, N), i32(BATCH, N), i32(BATCH, N) + t
            cand_v, cand_w = i32(N * BATCH, c), torch.zeros(N * BATCH, c, device=dev)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(launches):
                hip_beam.sample_step(buf[:, t], lse, seq_lp, seqs, tok, parent, fin, length, t, V - 4, V - 2, seed, cand_v, cand_w, c, top_p=top_p)
            e1.record()
            torch.cuda.synchronize()
            out[c].append(e0.elapsed_time(e1) / launches * 1e3)
    return {c: ts[1:] for c, ts in out.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sample', type=int, default=0, help='N: add the sampled search of N draws per image (GPV.forward_sample)')
    ap.add_argument('--top-k', type=int, default=20, help='top_k of the sampled search')
    ap.add_argument('--top-p', type=float, default=None, help='top_p of the sampled search')
    ap.add_argument('--no-repeat', type=int, default=0, help='no_repeat_ngram of the constrained path')
    ap.add_argument('--min-length', type=int, default=0, help='min_length of the constrained path')
    ap.add_argument('--repetition-penalty', type=float, default=None, help='repetition_penalty of the constrained path')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r13_beam.txt'))
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child()
    torch, model, samples, q = setup()
    T = model.cfg.max_text_len
    times = {'torch': [], 'device': []}
    constr = {k: v for k, v in (('no_repeat_ngram', args.no_repeat), ('min_length', args.min_length),
                                ('repetition_penalty', args.repetition_penalty)) if v}
    paths = {'torch': dict(impl='torch'), 'device': dict(impl='device')}
    if constr:
        times['constrained'], paths['constrained'] = [], dict(impl='device', **constr)
    search = lambda impl: model.forward_beam_search(samples, q, beam_size=K, **paths[impl])
    if args.sample:
        times['sampled'] = []
        if args.sample != K:                                                 # the beam search of the same K, to set the sampled search against
            times[f'device K={args.sample}'] = []
        beam = search

        def search(impl):
            if impl == 'sampled':
                return model.forward_sample(samples, q, num_samples=args.sample, top_k=args.top_k, top_p=args.top_p, seed=1)
            if impl.startswith('device K='):
                return model.forward_beam_search(samples, q, beam_size=args.sample, impl='device')
            return beam(impl)
    with torch.no_grad():
        outs = {}
        for impl in times:                                                   # warm-up + capture of the graphs
            for _ in range(2):
                outs[impl] = search(impl)
        torch.cuda.synchronize()
        same = sum(a == b for x, y in zip(outs['torch']['answers'], outs['device']['answers']) for a, b in zip(x, y))
        for _ in range(args.passes):
            for impl in times:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    search(impl)
                torch.cuda.synchronize()
                times[impl].append((time.perf_counter() - t0) / args.reps * 1e3)
    lines = [f'# tools/bench_beam.py: forward_beam_search(beam_size={K}) of {BATCH} synthetic 480x640 images, bf16, V = {len(model.vocab)}, T = {T}, the whole search one hipGraph',
             f'# {args.passes} alternating passes of {args.reps} searches per path, per-search wall time incl. host detokenisation']
    for impl, ts in times.items():
        lines.append(f'{impl:11s} median {statistics.median(ts):.3f} ms   min {min(ts):.3f}   max {max(ts):.3f}   passes ' + ' '.join(f'{t:.3f}' for t in ts))
    variants = {'plain': {}}
    if constr:
        from gpv1_amd import beam as rule
        lines.insert(2, '# constrained = the device path with ' + ' '.join(f'{k}={v}' for k, v in constr.items()))
        single = {'no_repeat_ngram': dict(no_repeat_ngram=args.no_repeat), 'min_length': dict(min_length=args.min_length),
                  'repetition_penalty': dict(repetition=rule.rep_factors(args.repetition_penalty))}
        given = {k: single[k] for k in constr}
        variants.update({f'{k} alone': kw for k, kw in given.items()})
        if len(given) > 1:
            variants['all together'] = {k: v for kw in given.values() for k, v in kw.items()}
    V = len(model.vocab)
    step_lines = [f'gpv_beam_step alone (B = {BATCH}, K = {K}, V = {V}, bf16, pitch T*V, t = T - 2 = {T - 2}; device events, 7 runs of 200 launches, us per launch):']
    for name, ts in step_times(torch, V, T, variants).items():
        step_lines.append(f'  {name:24s} median {statistics.median(ts):.2f}   min {min(ts):.2f}   max {max(ts):.2f}')
    if args.sample:
        lines.insert(2, f'# sampled = forward_sample(num_samples={args.sample}, top_k={args.top_k}, top_p={args.top_p}): the sampled step, no reorder launches')
        Cs = sorted({8, 20, 64, args.top_k})
        step_lines.append(f'gpv_beam_step in mode SAMPLE alone (B = {BATCH}, K = N = {args.sample}, V = {V}, bf16, pitch T*V, top_p = {args.top_p}; us per launch; '
                          'C pops, 1 .. ceil(C / 8) scans of the row -- random logits: 1 -- and the sum pass, finished slots included):')
        for c, ts in sample_step_times(torch, V, T, args.sample, Cs, args.top_p).items():
            step_lines.append(f'  top_k = {c:<3d}                 median {statistics.median(ts):.2f}   min {min(ts):.2f}   max {max(ts):.2f}')
    spread = max(max(ts) - min(ts) for ts in times.values())
    d = statistics.median(times['device']) - statistics.median(times['torch'])
    lines.append(f'device - torch = {d:+.3f} ms (largest min - max spread of a path in this run: {spread:.3f} ms): '
                 + ('device path not slower than the spread' if d <= spread else 'DEVICE PATH SLOWER than the spread'))
    lines.append(f'hypotheses with identical words on both paths: {same} of {BATCH * K} (bf16 logits of random weights tie inside the top-(K+1) of a row in 40 % of the rows: the rule takes the lower index, torch.topk either; 320 of 320 in precise mode)')
    lines += step_lines
    del model, samples, q
    torch.cuda.empty_cache()
    if not args.no_trace:
        with tempfile.TemporaryDirectory() as d:
            cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', d, '-o', 'beam', '--', sys.executable, os.path.abspath(__file__), '--child']
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                lines.append(f'kernel trace: rocprofv3 exited with {r.returncode}: ' + (r.stderr or r.stdout)[-400:].replace('\n', ' | '))
            else:
                lines += analyse(d, T)
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
