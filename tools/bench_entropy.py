"""What moving the JPEG Huffman walk to the device costs and saves: the 128-file set of tools/bench_loader.py, batch 32,
DeviceJpegDecoder(entropy='host') against entropy='device', alternating in one process, five passes each, median and spread.
  - files -> stem input (decoder + image pipeline), wall clock per batch: 'host' at 1, 2 and 8 parse threads, 'device' at 1 and 2
  - host CPU time per batch (process time) of both paths
  - bytes uploaded per batch
  - gpv_huff_decode alone: device time per batch by events; passes per image (min / median / max)
  - the bs32 train step fed by the loader (bench_loader (b)) for both paths, in the same call
usage: python tools/bench_entropy.py [--files 128] [--batch 32] [--steps 24] [--no-step] [--out FILE]      (GPU box)"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_input import make_files                                # noqa: E402
from bench_loader import V, write_tree                            # noqa: E402
from gpv1_amd import synthetic                                    # noqa: E402
from gpv1_amd.datasets import CocoCaptioning, DeviceLoader       # noqa: E402
from gpv1_amd.input_pipeline import DeviceImagePipeline       # noqa: E402
from gpv1_amd.jpeg import DeviceJpegDecoder                       # noqa: E402
from gpv1_amd.train_distr import shard_indices                    # noqa: E402


def med(xs):
    return {'median': statistics.median(xs), 'min': min(xs), 'max': max(xs), 'spread': max(xs) - min(xs)}


def files_to_stem(files, a, configs, passes=5):
    """per configuration (entropy, threads): wall clock and process time per batch of files -> decoder -> image pipeline, synchronised
    per batch; the configurations alternate inside every pass"""
    tasks = ['CocoClassification'] * a.batch
    batches = [files[s:s + a.batch] for s in range(0, len(files) - a.batch + 1, a.batch)]
    pipe = DeviceImagePipeline(size=(480, 640), train=True)
    decs = {c: DeviceJpegDecoder(threads=c[1], entropy=c[0]) for c in configs}
    wall, cpu = {c: [] for c in configs}, {c: [] for c in configs}
    for p in range(passes + 1):                                   # pass 0 warms up: pinned ring, scratch, allocator
        for c in configs:
            dec = decs[c]
            torch.cuda.synchronize()
            t0, c0 = time.perf_counter(), time.process_time()
            for b in batches:
                pipe(dec(b), tasks)
                torch.cuda.synchronize()
            if p:
                wall[c].append((time.perf_counter() - t0) / len(batches) * 1e3)
                cpu[c].append((time.process_time() - c0) / len(batches) * 1e3)
    out = {}
    for c in configs:
        n = decs[c].stats['device'] + decs[c].stats['host']
        out[f'{c[0]}_threads{c[1]}'] = {'wall_ms_per_batch': med(wall[c]), 'cpu_ms_per_batch': med(cpu[c]),
                                        'bytes_uploaded_per_batch': decs[c].stats['bytes_uploaded'] * a.batch // n,
                                        'files_device_route': decs[c].stats['device'], 'files_host_route': decs[c].stats['host']}
    return out


def kernel_time(files, a, passes=5):
    """gpv_huff_decode alone by events: the decoder's issue() with the launch bracketed"""
    from gpv1_amd import hip_huff
    dec = DeviceJpegDecoder(threads=8, entropy='device')
    batches = [files[s:s + a.batch] for s in range(0, len(files) - a.batch + 1, a.batch)]
    times, npass = [], []
    inner = hip_huff.decode
    marks = []

    def timed(*args):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        inner(*args)
        e1.record()
        marks.append((e0, e1))
    hip_huff.decode = timed
    try:
        for p in range(passes + 1):
            per = []
            for b in batches:
                dec(b)
                torch.cuda.synchronize()
                dec.check_status()
                per.append(marks[-1][0].elapsed_time(marks[-1][1]))
                if p == 1:
                    npass += dec.status[:, 1].tolist()
            if p:
                times.append(statistics.mean(per))
    finally:
        hip_huff.decode = inner
    return {'gpv_huff_decode_ms_per_batch': med(times), 'subseq_bits': dec.subseq_bits,
            'passes_per_image': {'min': min(npass), 'median': statistics.median(npass), 'max': max(npass)}}


def loader_fed_step(root, words, a):
    """bench_loader (b) for both paths: one model, one trainer, the two loaders alternating over five timed runs of a.steps steps"""
    from gpv1_amd.bert import WordPieceTokenizer
    from gpv1_amd.gpv import GPV
    from gpv1_amd.train import FlatTrainer
    ds = CocoCaptioning(write_tree(root, a.files, words), 'train')
    g = torch.Generator().manual_seed(0)
    model = GPV(synthetic.model_cfg(vocab=synthetic.make_vocab(V), vocab_embed=0.1 * torch.randn(V, 768, generator=g)))
    model.bert.tokenizer = WordPieceTokenizer(os.path.join(root, 'vocab.txt'))
    model.to('cuda').train()
    tr = FlatTrainer(model)
    loaders = {e: DeviceLoader(ds, a.batch, threads=2, prefetch=1, entropy=e) for e in ('host', 'device')}
    runs = {e: [] for e in loaders}
    epoch = 0
    for r in range(6):                                            # run 0 warms up: eager step, capture, slots
        for e, loader in loaders.items():
            n, t0 = 0, None
            while n < a.steps:
                for samples, qs, tg in loader.batches(shard_indices(len(ds), epoch, 0, 1), epoch):
                    if t0 is None:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    tr.train_step(samples, qs, tg)
                    n += 1
                    if n == a.steps:
                        break
                epoch += 1
            torch.cuda.synchronize()
            if r:
                runs[e].append((time.perf_counter() - t0) / n * 1e3)
    for loader in loaders.values():
        loader.close()
    return {f'step_fed_by_loader_ms_{e}_threads2': med(v) for e, v in runs.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=128)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--steps', type=int, default=24)
    ap.add_argument('--no-step', action='store_true')
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    files = make_files(a.files)
    res = {'files': a.files, 'batch': a.batch, 'file_bytes_per_batch': sum(len(f) for f in files) * a.batch // len(files)}
    res['files_to_stem_input'] = files_to_stem(files, a, [('host', 1), ('host', 2), ('host', 8), ('device', 1), ('device', 2)])
    res['kernel'] = kernel_time(files, a)
    if not a.no_step:
        with tempfile.TemporaryDirectory() as root:
            words = synthetic.write_wordpiece_vocab(os.path.join(root, 'vocab.txt'))
            res.update(loader_fed_step(root, words, a))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
