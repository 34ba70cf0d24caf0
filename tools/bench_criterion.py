"""Set criterion of box batches, host matcher against the device matcher (Localization matcher='host' | 'device'), on the
configs[4] batch of bench.py: B = 64, 480x640, 1..10 boxes per image (seed 99), 100 queries.

  measure:  python tools/bench_criterion.py [--repeats 5] [--steps 6] [--no-step] [--out profiles/r10_set_criterion.txt]

Three figures, every one a host clock around work that ends in a device synchronise or a pair of device events:
  * the criterion alone: Localization.forward + backward on fixed outputs of the batch's shape (logits randn, boxes drawn like the
    targets), with one layer (aux_loss off) and with six (aux_loss on);
  * the kernels alone: gpv_match_boxes and gpv_match_set_loss, each between two device events, and gpv_match_lsap on the worst shape
    the model has (Q = G = 100, costs from {0, 1, 2}: ties everywhere, the longest searches) for 1 and for 384 problems;
  * the full train step of bench.py's configs[4] (FlatTrainer.train_step, hipGraph body, eager criterion, AdamW).
The two paths ALTERNATE in one process, `repeats` passes each after two warm-up passes per path; the spread is (max - min) / median of
a path's passes.  Host synchronisations inside one criterion call are counted with torch.cuda.set_sync_debug_mode."""
import argparse
import os
import sys
import time
import warnings

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
B, Q = 64, 100


def targets_configs4(dev, rank=0):
    """the detection-only targets of bench.extra_configs"""
    import torch
    g = torch.Generator().manual_seed(99 + rank)
    tg = []
    for _ in range(B):
        n = 1 + int(torch.randint(0, 10, (1,), generator=g))
        cxcy = 0.25 + 0.5 * torch.rand(n, 2, generator=g)
        wh = 0.05 + 0.3 * torch.rand(n, 2, generator=g)
        tg.append({'task': 'CocoDetection', 'boxes': torch.cat((cxcy, wh), 1).to(dev), 'labels': torch.zeros(n, dtype=torch.long, device=dev)})
    return tg


def fixed_outputs(L, dev):
    import torch
    g = torch.Generator().manual_seed(5)
    draw = lambda: (torch.randn(B, Q, 2, generator=g).to(dev).requires_grad_(True),
                    torch.cat((0.25 + 0.5 * torch.rand(B, Q, 2, generator=g), 0.05 + 0.3 * torch.rand(B, Q, 2, generator=g)), -1).to(dev).requires_grad_(True))
    layers = [dict(zip(('pred_relevance_logits', 'pred_boxes'), draw())) for _ in range(L)]
    out = dict(layers[0])
    if L > 1:
        out['aux_outputs'] = layers[1:]
    return out


def med(v):
    return sorted(v)[len(v) // 2]


def fmt(v, unit='ms', scale=1e3):
    return 'median %.3f %s   passes: %s   spread (max-min)/median %.1f%%' % (
        med(v) * scale, unit, ' '.join('%.3f' % (x * scale) for x in v), 100 * (max(v) - min(v)) / med(v))


def criterion_alone(loc, outputs, targets, mode, calls=10):
    """seconds per call of forward + backward, `calls` calls back to back, one synchronise at the end"""
    import torch
    loc.matcher_mode = mode
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(calls):
        r = loc(outputs, targets)
        (r['loss_ce'] + 5 * r['loss_bbox'] + 2 * r['loss_giou']).backward()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / calls


def count_syncs(loc, outputs, targets, mode):
    import torch
    loc.matcher_mode = mode
    loc(outputs, targets)
    torch.cuda.synchronize()
    seen = []
    old = warnings.showwarning
    warnings.showwarning = lambda message, *a, **k: seen.append(str(message))
    warnings.simplefilter('always')
    torch.cuda.set_sync_debug_mode('warn')
    try:
        r = loc(outputs, targets)
        (r['loss_ce'] + 5 * r['loss_bbox'] + 2 * r['loss_giou']).backward()
    finally:
        torch.cuda.set_sync_debug_mode('default')
        warnings.showwarning = old
    torch.cuda.synchronize()
    return len(seen)


def events(fn, reps=20):
    """milliseconds between two device events around fn(), `reps` times after three warm-up calls"""
    import torch
    for _ in range(3):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def kernel_times(targets, dev):
    import numpy as np
    import torch
    from gpv1_amd import hip_match
    lines = []
    counts = [len(t['boxes']) for t in targets]
    gmax = max(counts)
    tb = torch.zeros(B, gmax, 4, device=dev)
    for b, t in enumerate(targets):
        tb[b, :counts[b]] = t['boxes']
    tl = torch.zeros(B, gmax, dtype=torch.int32, device=dev)
    gc = torch.tensor(counts, dtype=torch.int32, device=dev)
    for L in (1, 6):
        o = fixed_outputs(L, dev)
        layers = [o] + o.get('aux_outputs', [])
        lg = torch.stack([x['pred_relevance_logits'] for x in layers]).detach().contiguous()
        bx = torch.stack([x['pred_boxes'] for x in layers]).detach().contiguous()
        m = hip_match.match_boxes(lg, bx, tb, tl, gc, 1.0, 5.0, 2.0)
        lines.append('  gpv_match_boxes, %d x %d problems of %d x (1..%d), between events:   %s'
                     % (L, B, Q, gmax, fmt(events(lambda: hip_match.match_boxes(lg, bx, tb, tl, gc, 1.0, 5.0, 2.0)), 'us', 1e6)))
        lines.append('  gpv_match_set_loss, the same %d x %d problems, between events:        %s'
                     % (L, B, fmt(events(lambda: hip_match.set_loss(lg, bx, tb, tl, gc, m[0], m[1], m[2], m[3], 0.1)), 'us', 1e6)))
    rng = np.random.default_rng(0)
    for P in (1, 384):
        for name, cost in (('costs from {0,1,2}', rng.integers(0, 3, (P, 100, 100)).astype(np.float32)),
                           ('uniform fp32 costs', rng.random((P, 100, 100), dtype=np.float32))):
            c, n = torch.from_numpy(cost).to(dev), torch.full((P,), 100, dtype=torch.int32, device=dev)
            lines.append('  gpv_match_lsap, %3d problem(s) of 100 x 100, %s, between events:   %s'
                         % (P, name, fmt(events(lambda: hip_match.lsap(c, n)), 'us', 1e6)))
    return lines


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--steps', type=int, default=6, help='train steps per pass (bench.py times 6)')
    ap.add_argument('--no-step', action='store_true', help='skip the full train step (no model is built)')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), 'bench_criterion.py measures on the GPU only'
    import bench
    import gpv1_amd.hip as hip
    from gpv1_amd import hip_match
    from gpv1_amd.criterion import Localization
    from gpv1_amd.misc import AttrDict
    hip.lib()
    hip_match.lib()
    os.environ.pop('GPV_MATCHER', None)
    dev = 'cuda:0'
    targets = targets_configs4(dev)
    cfg = bench.make_cfg()['losses']['Localization']
    loc = Localization(AttrDict({k: (AttrDict(v) if isinstance(v, dict) else v) for k, v in cfg.items()})).to(dev)
    lines = ['set criterion of a box batch: B = %d, %d queries, 1..10 boxes per image (bench.py configs[4], seed 99), %d boxes in all; '
             '%d alternating passes per path' % (B, Q, sum(len(t['boxes']) for t in targets), args.repeats)]
    for L in (1, 6):
        outputs = fixed_outputs(L, dev)
        t = {'host': [], 'device': []}
        for mode in t:
            for _ in range(2):
                criterion_alone(loc, outputs, targets, mode, calls=3)
        for _ in range(args.repeats):
            for mode in t:
                t[mode].append(criterion_alone(loc, outputs, targets, mode))
        syncs = {mode: count_syncs(loc, outputs, targets, mode) for mode in t}
        lines.append(' criterion alone (forward + backward, 10 calls back to back per pass), %d layer(s):' % L)
        for mode in t:
            lines.append("  matcher='%s'%s %s   host synchronisations per call: %d" % (mode, ' ' * (7 - len(mode)), fmt(t[mode]), syncs[mode]))
        lines.append('  host / device: %.2fx' % (med(t['host']) / med(t['device'])))
    lines.append(' kernels alone:')
    lines += kernel_times(targets, dev)
    if not args.no_step:
        from gpv1_amd.gpv import GPV
        from gpv1_amd.misc import nested_tensor_from_tensor_list
        from gpv1_amd.ops import RT
        from gpv1_amd.train import FlatTrainer
        torch.manual_seed(0)
        model = GPV(bench.make_cfg())
        for n, buf in model.named_buffers():
            if n.endswith('running_var'):
                buf.uniform_(0.5, 1.5)
        model.to(dev)
        RT.manual_seed(1000)
        tr = FlatTrainer(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, clip_max_norm=0.1, warmup_steps=100, t_total=1000)
        images, mask, ids, attn, _ = bench.make_batch(11, B, dev)
        samples = nested_tensor_from_tensor_list(images)
        mloc = model.criterion.localization_criterion

        def one_pass(mode):
            mloc.matcher_mode = mode
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                tr.train_step(samples, (ids, attn), [dict(x) for x in targets])
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / args.steps
        t = {'host': [], 'device': []}
        for mode in t:
            one_pass(mode)
        for mode in t:
            one_pass(mode)
        for _ in range(args.repeats):
            for mode in t:
                t[mode].append(one_pass(mode))
        lines.append(' full train step (bench.py configs[4]: FlatTrainer.train_step, bf16, hipGraph body, eager criterion, AdamW), %d steps per pass:' % args.steps)
        for mode in t:
            lines.append("  matcher='%s'%s %s   %.1f images/s" % (mode, ' ' * (7 - len(mode)), fmt(t[mode]), B / med(t[mode])))
        lines.append('  host / device: %.3fx' % (med(t['host']) / med(t['device'])))
    print('\n'.join(lines))
    if args.out:
        with open(args.out, 'a') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
