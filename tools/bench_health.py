"""Cost of the training flight recorder (gpv1_amd.health) on the BASELINE train step: bench.py's workload (its model, batch, trainer
settings; not bench.py itself), one process, one trainer, three arms that ALTERNATE pass by pass:

  off    trainer.recorder = None -- the step as it is without the feature
  G      FlightRecorder(watch=('G',)): one more read of the flat gradient buffer per step
  PGMV   FlightRecorder(watch=('P', 'G', 'M', 'V')): all four flat buffers

  measure:  python tools/bench_health.py [--steps 20] [--repeats 5] [--out profiles/r11_health.txt]

Every pass is `steps` train steps under a host clock that ends in a device synchronise; `repeats` passes per arm after two warm-up
passes per arm; the spread is (max - min) / median of an arm's passes.  Then record() alone -- its three launches, nothing else on
the stream -- between two device events, per recorder, with the bytes it reads and the rate that makes."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))


def med(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--batch', type=int, default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    import torch
    import bench
    import gpv1_amd.hip as hip
    from gpv1_amd import health
    from gpv1_amd.gpv import GPV
    from gpv1_amd.misc import nested_tensor_from_tensor_list
    from gpv1_amd.ops import RT
    from gpv1_amd.train import FlatTrainer
    hip.lib()
    if not torch.cuda.is_available():
        raise SystemExit('bench_health.py measures on the GPU; there is none here')
    os.environ.setdefault('GPV_GRAPHS_STRICT', '1')
    dev = 'cuda:0'
    torch.cuda.set_device(0)
    torch.manual_seed(0)
    model = GPV(bench.make_cfg())
    for n, buf in model.named_buffers():
        if n.endswith('running_var'):
            buf.uniform_(0.5, 1.5)
    model.to(dev)
    RT.manual_seed(1000)
    tr = FlatTrainer(model, lr=1e-4, lr_backbone=1e-5, weight_decay=1e-4, clip_max_norm=0.1, warmup_steps=100, t_total=1000)
    B = args.batch or bench.BATCH
    images, mask, ids, attn, targets = bench.make_batch(0, B, dev)
    samples = nested_tensor_from_tensor_list(images)

    def run(k):
        for _ in range(k):
            loss = tr.train_step(samples, (ids, attn), [dict(t) for t in targets])
        torch.cuda.synchronize()
        return loss

    run(3)                                                           # eager step, capture, first replay
    recs = {'off': None, 'G': health.FlightRecorder(tr, watch=('G',)).prepare(),
            'PGMV': health.FlightRecorder(tr, watch=('P', 'G', 'M', 'V')).prepare()}
    times = {a: [] for a in recs}
    for p in range(2 + args.repeats):
        for arm, rec in recs.items():
            tr.recorder = rec
            t0 = time.perf_counter()
            loss = run(args.steps)
            dt = (time.perf_counter() - t0) / args.steps
            if p >= 2:
                times[arm].append(dt)
    tr.recorder = None
    lines = ['flight recorder on the BASELINE train step: batch %d, %d parameters in %d segments per buffer, flat buffer %.1f MB, '
             '%d steps per pass, %d passes per arm after 2 warm-up passes, arms alternating; last loss %.4f'
             % (B, tr.total, len(tr.entries), tr.total * 4 / 1e6, args.steps, args.repeats, float(loss))]
    base = med(times['off'])
    for arm, v in times.items():
        lines.append('step, recorder %-5s median %.3f ms   passes: %s   spread (max-min)/median %.2f%%   against off: %+.3f ms (%+.2f%%)'
                     % (arm, med(v) * 1e3, ' '.join('%.3f' % (x * 1e3) for x in v), 100 * (max(v) - min(v)) / med(v),
                        (med(v) - base) * 1e3, 100 * (med(v) - base) / base))
    for arm, rec in recs.items():
        if rec is None:
            continue
        ev = []
        for _ in range(24):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rec.record()
            e1.record()
            torch.cuda.synchronize()
            ev.append(e0.elapsed_time(e1) * 1e-3)
        ev = ev[4:]
        nbytes = sum(k * t.element_size() for (b, n, t, o, k) in rec.segments)
        lines.append('record() alone, %-5s median %.1f us (min %.1f, max %.1f) for %d segments, %d blocks, %.1f MB read: %.2f TB/s'
                     % (arm, med(ev) * 1e6, min(ev) * 1e6, max(ev) * 1e6, rec.S, rec.W, nbytes / 1e6, nbytes / med(ev) / 1e12))
        reading = rec.read()
        lines.append('   ring %d x %d rows = %.2f MB per read(); group norms of the last step: %s; latch: %s'
                     % (rec.R, rec.S, rec._buf.numel() / 1e6, ' '.join('%s %.4e' % kv for kv in reading.grad_norms().items()), reading.trip))
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
