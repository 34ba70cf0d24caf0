"""Detection evaluation at batch 64, 480x640, synthetic data: metrics.det_metrics with the device scorer against host=True.

  measure:  python tools/bench_eval.py [--batches 8] [--repeats 5] [--out profiles/r08_eval.txt]
  trace:    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o e -- python tools/bench_eval.py --trace-run
            python tools/bench_eval.py --stats <dir> [--out profiles/r08_eval.txt]      (appends the scorer kernel's own time)

The dataset (images on the device, tokenised queries, 1..10 ground-truth boxes per sample) is built once; a pass is the whole
det_metrics call -- greedy forward per batch, scoring, the final copy -- ending in a device synchronise.  Two warm-up passes per
path (graph capture, kernel attributes), then the two paths ALTERNATE for `repeats` timed passes each; the spread reported is
(max - min) / median of a path's passes.  Forward time alone (the same loop without scoring) is printed for scale.

Caption pass:  python tools/bench_eval.py --captions [--repeats 5] [--out profiles/r09_cap_eval.txt]
5000 synthetic entries, five references of 8..15 words each, hypotheses of 6..14 words, a Zipf vocabulary of 3000 words (the input the
plain-Python scorers were timed on).  A pass is caption_scorer.CaptionScorer.scores(hyps, refs) on tokenised captions: for the device
path the word -> id encoding on the host, the one upload, the launches and the one copy back; for host=True the host rule.  The two
paths alternate; the device path's own share (hip_cap.caption_scores between two events) and the greedy forward of the detection
pass above (images/s, scaled to 5000 images) are printed beside them."""
import argparse
import csv
import glob
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
B, IMG = 64, (480, 640)


def build(nbatch, dev):
    import numpy as np
    import torch
    import bench
    import gpv1_amd.hip as hip
    import gpv1_amd.hip_eval as hip_eval
    from gpv1_amd.gpv import GPV
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    hip.lib()
    hip_eval.lib()
    torch.manual_seed(0)
    model = GPV(bench.make_cfg())
    for n, buf in model.named_buffers():
        if n.endswith('running_var'):
            buf.uniform_(0.5, 1.5)
    model.to(dev).eval()
    rs = np.random.RandomState(0)
    data, samples = [], []
    for k in range(nbatch):
        images, mask, ids, attn, _ = bench.make_batch(100 + k, B, dev)
        data.append((nested_tensor_from_tensor_list(list(images)), (ids, attn), None))
        for i in range(B):
            nb = rs.randint(1, 11)
            xy = rs.uniform(0.0, 0.6, (nb, 2)) * [IMG[1], IMG[0]]
            wh = rs.uniform(0.05, 0.4, (nb, 2)) * [IMG[1], IMG[0]]
            samples.append({'id': k * B + i, 'boxes': np.concatenate([xy, wh], 1).tolist(), 'category_name': 'dog',
                            'image': {'W': IMG[1], 'H': IMG[0], 'image_id': k * B + i}, 'coco_categories': {'seen': ['dog'], 'unseen': []}})
    return model, data, samples


def one_pass(model, data, samples, host):
    import torch
    from gpv1_amd import metrics
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    m = metrics.det_metrics(model, iter(data), samples, None, host=host)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, m


def forward_only(model, data):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.no_grad():
        for imgs, q, _ in data:
            model(imgs, q, None)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def stats(trace_dir):
    """the scorer kernel's own time from a rocprofv3 --kernel-trace run: calls, mean / min / max microseconds"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, '**', '*kernel_trace.csv'), recursive=True):
        rows += [r for r in csv.DictReader(open(f)) if 'det_ap_kernel' in r['Kernel_Name']]
    us = sorted((int(r['End_Timestamp']) - int(r['Start_Timestamp'])) / 1e3 for r in rows)
    if not us:
        return 'scorer kernel: no det_ap_kernel launch in the trace under %s' % trace_dir
    return ('scorer kernel det_ap_kernel (rocprofv3 --kernel-trace, batch %d x 100 queries): %d launches, mean %.2f us, median %.2f us, '
            'min %.2f us, max %.2f us' % (B, len(us), sum(us) / len(us), us[len(us) // 2], us[0], us[-1]))


def caption_entries(n=5000, refs_per_entry=5, vocab=3000, seed=0):
    import numpy as np
    rs = np.random.RandomState(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    words = np.asarray(['w%d' % i for i in range(vocab)])
    draw = lambda lo, hi: words[rs.choice(vocab, size=rs.randint(lo, hi + 1), p=p)].tolist()
    return [draw(6, 14) for _ in range(n)], [[draw(8, 15) for _ in range(refs_per_entry)] for _ in range(n)]


def caption_pass(args, dev):
    import numpy as np
    import torch
    from gpv1_amd import evaluators, hip_cap
    from gpv1_amd.caption_scorer import CaptionScorer, encode_captions
    hyps, refs = caption_entries()
    paths = {False: CaptionScorer(device=dev), True: CaptionScorer(host=True)}

    def one(host):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = paths[host].scores(hyps, refs)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out
    one(False)
    one(False)
    t, res = {False: [], True: []}, {}
    for _ in range(args.repeats):
        for host in (False, True):
            dt, res[host] = one(host)
            t[host].append(dt)
    # the device path's parts: the host-side encoding, and the launches alone between two events (arrays already on the device)
    t0 = time.perf_counter()
    arrays = encode_captions(hyps, refs)
    t_enc = time.perf_counter() - t0
    N, LH = arrays[0].shape
    LR = arrays[2].shape[2]
    tables = evaluators.caption_tables(N, max(LH, LR))
    d = [torch.from_numpy(a).to(dev) for a in arrays[:5] + tables]
    ev = []
    for _ in range(args.repeats + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        hip_cap.caption_scores(*d, occurrences=arrays[5])
        b.record()
        torch.cuda.synchronize()
        ev.append(a.elapsed_time(b))
    ev = ev[2:]
    med = lambda v: sorted(v)[len(v) // 2]
    fmt = lambda v: 'median %.1f ms   passes ms: %s   spread (max-min)/median %.1f%%' % (
        med(v) * 1e3, ' '.join('%.1f' % (x * 1e3) for x in v), 100 * (max(v) - min(v)) / med(v))
    worst = float(np.abs(res[False]['cider_entries'] - res[True]['cider_entries']).max())
    lines = ['caption scoring, %d entries x 5 references of 8..15 words, hypotheses of 6..14 words, Zipf vocabulary of 3000 words, %d alternating passes per path'
             % (N, args.repeats),
             '  %-58s %s' % ('device scorer (encode + upload + csrc/caption_score.hip + copy)', fmt(t[False])),
             '  %-58s %s' % ('host=True (evaluators.caption_scores_host)', fmt(t[True])),
             '  device path, parts: word -> id encoding on the host %.1f ms; memsets + two kernels between events: median %.3f ms (%s), table of %d slots'
             % (t_enc * 1e3, med(ev), ' '.join('%.3f' % x for x in ev), hip_cap.table_capacity(arrays[5])),
             '  host / device: %.1fx   Cider device %.12f host %.12f   Bleu4 device %.12f host %.12f   worst per-entry |difference| %.2e'
             % (med(t[True]) / med(t[False]), res[False]['Cider'], res[True]['Cider'], res[False]['Bleu4'], res[True]['Bleu4'], worst)]
    if not args.no_forward:
        model, data, _ = build(args.batches, dev)
        for _ in range(2):
            forward_only(model, data)
        fwd = [forward_only(model, data) for _ in range(args.repeats)]
        n = args.batches * B
        lines.append('  greedy forward alone, batch %d, %dx%d, %d batches: %.1f images/s (median of %d passes, spread %.1f%%): %d images take %.2f s'
                     % (B, IMG[0], IMG[1], args.batches, n / med(fwd), args.repeats, 100 * (max(fwd) - min(fwd)) / med(fwd), N, N * med(fwd) / n))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batches', type=int, default=8)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--trace-run', action='store_true', help='the short run meant to be traced: warm-up + two device-scored passes')
    ap.add_argument('--stats', default=None, help='rocprofv3 output directory to summarise')
    ap.add_argument('--captions', action='store_true', help='the caption scoring pass (device scorer against host=True) instead of detection')
    ap.add_argument('--no-forward', action='store_true', help='with --captions: skip the greedy forward beside the scorers')
    args = ap.parse_args()
    lines = []
    if args.stats:
        lines.append(stats(args.stats))
    elif args.captions:
        import torch
        assert torch.cuda.is_available(), 'bench_eval.py measures on the GPU only'
        lines += caption_pass(args, torch.device('cuda:0'))
    else:
        import torch
        assert torch.cuda.is_available(), 'bench_eval.py measures on the GPU only'
        dev = torch.device('cuda:0')
        nb = 2 if args.trace_run else args.batches
        model, data, samples = build(nb, dev)
        for _ in range(2):
            one_pass(model, data, samples, False)
        if args.trace_run:
            for _ in range(2):
                print('traced pass: %.1f ms' % (one_pass(model, data, samples, False)[0] * 1e3))
            return
        for _ in range(2):
            one_pass(model, data, samples, True)
        t = {False: [], True: []}
        maps = {}
        fwd = []
        for _ in range(args.repeats):
            for host in (False, True):
                dt, maps[host] = one_pass(model, data, samples, host)
                t[host].append(dt)
            fwd.append(forward_only(model, data))
        n = len(samples)
        med = lambda v: sorted(v)[len(v) // 2]
        lines.append('detection evaluation, batch %d, %dx%d, %d batches (%d samples, 100 queries, 1..10 ground-truth boxes), %d alternating passes per path'
                     % (B, IMG[0], IMG[1], nb, n, args.repeats))
        for host, name in ((False, 'device scorer (csrc/det_ap.hip)'), (True, 'host=True (decode_outputs + evaluators.CocoDetection)')):
            v = t[host]
            lines.append('  %-56s %8.1f images/s   median %.1f ms per pass, %.2f ms per batch   passes ms: %s   spread (max-min)/median %.1f%%   mAP %.6f'
                         % (name, n / med(v), med(v) * 1e3, med(v) * 1e3 / nb, ' '.join('%.1f' % (x * 1e3) for x in v), 100 * (max(v) - min(v)) / med(v), maps[host]))
        lines.append('  %-56s %8.1f images/s   median %.2f ms per batch   spread %.1f%%' % ('greedy forward alone (no scoring)', n / med(fwd), med(fwd) * 1e3 / nb,
                                                                                           100 * (max(fwd) - min(fwd)) / med(fwd)))
        lines.append('  scoring cost per batch over the forward alone: device %.2f ms, host %.2f ms' %
                     ((med(t[False]) - med(fwd)) * 1e3 / nb, (med(t[True]) - med(fwd)) * 1e3 / nb))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
