"""Classification decode from a closed answer set: 64 images, 80 class names (65 of one word, 15 of two, the proportions of the COCO
table -- the bench vocabulary is synthetic), K = 4: GPV.choose (gpv-1_amd/csrc/phrase_step.hip) against the greedy decode under the
reference's flat vocabulary mask, each one hipGraph.  The greedy path is not touched by the phrase search (no file on its path differs
from the commit before it), so it is the parent's decode, measured in the same process.

  python tools/bench_phrases.py [--out profiles/r16_phrases.txt] [--passes 5] [--reps 3] [--no-trace]

The two paths alternate in one process, `--passes` passes of `--reps` calls each (wall time per call of 64 images); median and
min - max of the passes are reported.  Then ONE `rocprofv3 --kernel-trace` run of a fresh child process (`--child`: eager searches,
so that every launch is a kernel record) times gpv_phrase_step and gpv_beam_step where they run, in the chain of a search, at the
same (B, K, V): a phrase search and a beam search (finished='freeze') of K = 4 alternate."""
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
K, BATCH = 4, 64
CLASSES = tuple(f'w{100 + i}' for i in range(65)) + tuple(f'w{300 + i} w{400 + i // 3}' for i in range(15))


def setup():
    import torch
    import bench
    import gpv1_amd.hip as hip
    import gpv1_amd.hip_beam as hip_beam
    import gpv1_amd.hip_phrase as hip_phrase
    from gpv1_amd import compute_predictions as cp
    from gpv1_amd.gpv import GPV
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    hip.lib()
    hip_beam.lib()
    hip_phrase.lib()
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    model = GPV(bench.make_cfg())
    for n, buf in model.named_buffers():
        if n.endswith('running_var'):
            buf.uniform_(0.5, 1.5)
    model.to(dev).eval()
    images, mask, ids, attn, _ = bench.make_batch(0, BATCH, dev)
    pset, owner = cp.create_phrase_set(model, CLASSES)
    vm = torch.as_tensor(cp.create_vocab_mask(model, classes=CLASSES)[1], device=dev)
    return torch, model, nested_tensor_from_tensor_list(images), (ids, attn), pset, owner, vm


def child():
    """eager searches for the kernel trace: two of each as warm-up, then three of each, alternating"""
    torch, model, samples, q, pset, _, _ = setup()
    model.cfg['graph_inference'] = False
    with torch.no_grad():
        for _ in range(5):
            model._phrase_device(samples, q, K, pset)
            torch.cuda.synchronize()
            model._beam_device(samples, q, K, impl='device', finished='freeze')
            torch.cuda.synchronize()
    print('child ok')


def analyse(trace_dir, T):
    files = glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True)
    if not files:
        return ['kernel trace: no *kernel_trace.csv was written']
    rows = list(csv.DictReader(open(files[0])))
    rows.sort(key=lambda r: int(r['Start_Timestamp']))
    dur = lambda r: (int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3
    ph = [dur(r) for r in rows if 'phrase_step_kernel' in r['Kernel_Name']]
    bm = [dur(r) for r in rows if 'step_kernel' in r['Kernel_Name'] and 'phrase_step_kernel' not in r['Kernel_Name']]
    n = T - 1
    if len(ph) != 5 * n or len(bm) != 5 * n:
        return [f'kernel trace: expected {5 * n} records of each step kernel, found {len(ph)} phrase and {len(bm)} beam']
    ph, bm = ph[2 * n:], bm[2 * n:]                         # the last three searches of each
    out = [f'step kernels in the chain of an eager search (rocprofv3 --kernel-trace, B = {BATCH}, K = {K}, bf16 logits, 3 searches of {n} steps each):']
    for name, d in (('gpv_phrase_step', ph), ('gpv_beam_step', bm)):
        per = [sum(d[i * n:(i + 1) * n]) for i in range(3)]
        out.append(f'  {name:16s} median {statistics.median(d):.1f} us  min {min(d):.1f}  max {max(d):.1f};  sum over one search: '
                   + ' '.join(f'{p:.0f}' for p in per) + ' us')
    by_t = [statistics.median(ph[i * n + t] for i in range(3)) for t in range(n)]
    out.append('  gpv_phrase_step by step t (median of 3): ' + ' '.join(f'{x:.1f}' for x in by_t) +
               '   (t = 0 reads one row per image, later steps the rows of live parents only; a finished search reads none)')
    by_t = [statistics.median(bm[i * n + t] for i in range(3)) for t in range(n)]
    out.append('  gpv_beam_step   by step t (median of 3): ' + ' '.join(f'{x:.1f}' for x in by_t))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'r16_phrases.txt'))
    ap.add_argument('--passes', type=int, default=5)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--no-trace', action='store_true')
    ap.add_argument('--child', action='store_true')
    args = ap.parse_args()
    if args.child:
        return child()
    torch, model, samples, q, pset, owner, vm = setup()
    T = model.cfg.max_text_len
    runs = {'tokens': lambda: model(samples, q, None, vocab_mask=vm), 'phrases': lambda: model.choose(samples, q, pset, beam_size=K)}
    times = {k: [] for k in runs}
    with torch.no_grad():
        for name, fn in runs.items():                                        # warm-up + capture of both graphs
            for _ in range(2):
                out = fn()
        torch.cuda.synchronize()
        idx, lp = out
        top1 = model(samples, q, None, vocab_mask=vm)['answer_logits'][-1].float().argmax(-1).cpu()
        names = {tuple(c.split()) for c in CLASSES}
        greedy = [tuple(w for w in words if w not in ('__stop__', '__pad__')) for words in model.token_ids_to_words(top1.numpy())]
        legal = sum(g in names for g in greedy)
        for _ in range(args.passes):
            for name, fn in runs.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.reps * 1e3)
    lines = [f'# tools/bench_phrases.py: classification decode of {BATCH} synthetic 480x640 images, bf16, V = {len(model.vocab)}, T = {T}, {len(CLASSES)} class names '
             f'({sum(" " in c for c in CLASSES)} of two words), each path one hipGraph',
             f'# tokens = greedy decode under the flat vocabulary mask (the path of the commit before; untouched here), phrases = GPV.choose, beam_size = {K}',
             f'# {args.passes} alternating passes of {args.reps} calls per path, wall time per call']
    for name, ts in times.items():
        lines.append(f'{name:8s} median {statistics.median(ts):.3f} ms   min {min(ts):.3f}   max {max(ts):.3f}   passes ' + ' '.join(f'{t:.3f}' for t in ts))
    spread = max(max(ts) - min(ts) for ts in times.values())
    d = statistics.median(times['phrases']) - statistics.median(times['tokens'])
    lines.append(f'phrases - tokens = {d:+.3f} ms (largest min - max spread of a path in this run: {spread:.3f} ms); the phrase search decodes K = {K} '
                 f'hypotheses per image ({K * BATCH} decoder rows), the greedy decode one ({BATCH} rows)')
    lines.append(f'answers that are one of the {len(CLASSES)} names: tokens {legal} of {BATCH}, phrases {int((idx >= 0).sum())} of {BATCH} (random weights: this says what the '
                 f'flat mask lets through, not how accurate either is); mean log-probability of the chosen phrase {float(lp.mean()):.3f}')
    del model, samples, q
    torch.cuda.empty_cache()
    if not args.no_trace:
        with tempfile.TemporaryDirectory() as d:
            cmd = ['rocprofv3', '--kernel-trace', '--output-format', 'csv', '-d', d, '-o', 'phrases', '--', sys.executable, os.path.abspath(__file__), '--child']
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
