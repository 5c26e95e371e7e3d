#!/usr/bin/env python3
"""Waveform augmentation on the device: what --wave-augment costs.

Whole epochs of submodel_trainer.py's real input path (get_dataloaders ->
DeviceModel.images -> Trainer.train_step, as tools/bench_train_input.py runs
them) over WAV files on disk with --device-ingest, in one process, alternating
between ``--wave-augment all`` and the flag absent (the path as it was before
the flag existed), with a warm page cache.  Sets: the 44.1 kHz stereo 30 s files
and the 32 kHz mono 8 s files of bench_train_input.py, each at --workers worker
processes (default 12, and 0).

Per set and worker count: files/s of both, their ratio, and the flag-absent
path's own repeat spread beside it.  Then, on batches taken from the augmenting
loader: the device time of the augmentation launches alone per batch (HIP
events around sad_wave_augment_run), and the phaser alone -- every file of the
batch as a phaser file -- as the chunked scan against one thread per file
walking the recurrence serially (sad_wave_phaser_serial_run), with the largest
difference between their outputs.  No figure is a target.  Writes --out
(default profiles/wave_augment_bench.json) and prints the same JSON on one line."""
import argparse
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'synthetic-audio-detection_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

import torch  # noqa: E402

from bench_train_input import SETS, epoch, write_set  # noqa: E402

BENCH_SETS = ('44k-stereo-s16-30s', '32k-mono-s16-8s')


def _events_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def kernel_times(loader, ti, n_batches, reps):
    """The augmentation launches alone, and the phaser as a scan and serially, on real batches."""
    from sad import _lib, ingest
    dev = ti.device
    aug_ms, scan_ms, serial_ms, kinds, diff = [], [], [], [0] * 6, 0.0
    for k, batch in enumerate(loader):
        if k >= n_batches:
            break
        if batch is None or batch.wave_off is None:
            continue
        d_arena = batch.arena.to(dev)
        for kind in batch.wave_table[:, 0].tolist():
            kinds[kind] += 1
        aug_ms.append(min(_events_ms(lambda: ti.wave_augment(batch, d_arena), reps)))
        # the same batch with every file a phaser file (rate 0.5 Hz, depth 0.7)
        ph = ingest.StoredBatch(batch.arena.clone(), batch.n_files, batch.n_tiles, batch.table_off, batch.tiles_off,
                                batch.rates, batch.targets, batch.aug, batch.seg_len, batch.wave_off,
                                batch.mono_table_off, batch.mono_bytes)
        wt = ph.wave_table
        wt[:, 0] = 4
        wt[:, 4] = int(torch.tensor([0.5, 0.7]).view(torch.int64).item())
        d_ph = ph.arena.to(dev)
        scan_ms.append(min(_events_ms(lambda: ti.wave_augment(ph, d_ph), reps)))
        mono = torch.empty(ph.mono_bytes, device=dev, dtype=torch.uint8)
        base = d_ph.data_ptr()

        def serial():
            _lib.call('sad_wave_phaser_serial_run', base, ph.table_off, ph.table.data_ptr(), base + ph.table_off,
                      ph.n_files, ph.wave_table.data_ptr(), base + ph.wave_off, mono.data_ptr(), ph.mono_bytes,
                      _lib.stream_handle(dev))

        serial_ms.append(min(_events_ms(serial, max(1, reps // 2))))
        a, b = ti.wave_augment(ph, d_ph).view(torch.float32), mono.view(torch.float32)
        for _, _, n_out, off in wt[:, :4].tolist():  # the files' frames only: the padding between them is not written
            diff = max(diff, float((a[off // 4:off // 4 + n_out] - b[off // 4:off // 4 + n_out]).abs().max()))
    if not aug_ms:
        return None
    mean = lambda v: round(sum(v) / len(v), 4)  # noqa: E731
    return {'batches': len(aug_ms), 'kinds_drawn': kinds, 'augment_ms_per_batch': mean(aug_ms),
            'augment_ms_per_batch_min_max': [round(min(aug_ms), 4), round(max(aug_ms), 4)],
            'phaser_scan_ms_per_batch': mean(scan_ms), 'phaser_serial_ms_per_batch': mean(serial_ms),
            'serial_over_scan': round(sum(serial_ms) / sum(scan_ms), 1), 'scan_vs_serial_max_abs_diff': diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=2048, help='training files per set')
    ap.add_argument('--distinct', type=int, default=8, help='different clips per class and set')
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--workers', default='12,0', help='DataLoader worker counts to run, each at most 16')
    ap.add_argument('--repeats', type=int, default=3, help='epochs per path and set (alternating)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'mixed', 'fp32'])
    ap.add_argument('--kernel-batches', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wave_augment_bench.json'))
    args = ap.parse_args()
    worker_counts = [int(w) for w in args.workers.split(',')]
    if not all(0 <= w <= 16 for w in worker_counts):
        ap.error('--workers must be in [0, 16]')
    import submodel_trainer as smt
    from sad import ingest
    from sad import train as st

    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(42)
    base, head = st.init_state_dict(42)
    trainer = st.Trainer(base, head, dev, args.dtype)
    model = smt.DeviceModel(trainer, st.TrainFrontEnd(dev, args.dtype))
    ti = ingest.TrainIngest(dev)
    out = {'batch_size': args.batch_size, 'workers': worker_counts, 'dtype': args.dtype, 'files_per_set': args.files,
           'repeats': args.repeats, 'cpus': len(os.sched_getaffinity(0)), 'sets': {}}
    paths = ('plain', 'augment')
    with tempfile.TemporaryDirectory() as tmp:
        for name in BENCH_SETS:
            sr, ch, seconds, _ = SETS[name]
            root = os.path.join(tmp, name)
            write_set(root, sr, ch, seconds, args.files, args.distinct)
            entry = {'sample_rate': sr, 'channels': ch, 'seconds': seconds, 'workers': {}}
            for workers in worker_counts:
                loaders = {}
                for p in paths:
                    a = smt.parse_args(['--data-dir', root, '--batch-size', str(args.batch_size), '--workers',
                                        str(workers), '--precision', args.dtype, '--device-ingest'] +
                                       (['--wave-augment', 'all'] if p == 'augment' else []))
                    loaders[p] = smt.get_dataloaders(a)[0]
                runs = {p: [] for p in paths}
                for p in paths:  # warm-up: the page cache, the resample plans, the allocator, the workers
                    epoch(loaders[p], model)
                for _ in range(args.repeats):
                    for p in paths:
                        runs[p].append(epoch(loaders[p], model))
                        print(f'{name} workers={workers} {p}: {runs[p][-1]}', file=sys.stderr, flush=True)
                fps = {p: [r['files_per_s'] for r in runs[p]] for p in paths}
                res = {'runs': runs, 'best_files_per_s': {p: max(fps[p]) for p in paths},
                       'augment_over_plain': round(max(fps['augment']) / max(fps['plain']), 3),
                       'plain_repeat_spread': round((max(fps['plain']) - min(fps['plain'])) / max(fps['plain']), 4),
                       'augment_repeat_spread': round((max(fps['augment']) - min(fps['augment'])) /
                                                      max(fps['augment']), 4),
                       'device_ms_per_step': {p: min(r['device_ms_per_step'] for r in runs[p]) for p in paths}}
                if workers == 0:
                    res['kernels'] = kernel_times(loaders['augment'], ti, args.kernel_batches, 5)
                    print(f'{name} kernels: {res["kernels"]}', file=sys.stderr, flush=True)
                del loaders  # stops the persistent workers
                entry['workers'][str(workers)] = res
            out['sets'][name] = entry
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:  # after every set: a long run leaves what it finished
                f.write(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
