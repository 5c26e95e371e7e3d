#!/usr/bin/env python3
"""Time stretch and pitch shift on the device: what --wave-stretch costs.

The twin of tools/bench_wave_augment.py.  Whole epochs of submodel_trainer.py's
real input path over WAV files on disk with --device-ingest, in one process,
alternating between ``--wave-stretch all`` and the flag absent, with a warm
page cache; sets: 44.1 kHz mono files of 8 s and of 30 s, each at --workers
worker processes (default 12, and 0).

Per set and worker count: files/s of both, their ratio, and the flag-absent
path's own repeat spread beside it.  Then, on batches taken from the stretching
loader: the device time of the stretch launches alone per batch (HIP events
around sad_wave_stretch_run) and the workspace they take, and the float64
contract's host seconds per file (tests/stretch_ref.py) on the same heads.  No
figure is a target.  Writes --out (default profiles/wave_stretch_bench.json) and
prints the same JSON on one line."""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'synthetic-audio-detection_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bench_train_input import epoch, write_set  # noqa: E402
from bench_wave_augment import _events_ms  # noqa: E402

BENCH_SETS = {'44k-mono-s16-8s': (44100, 1, 8), '44k-mono-s16-30s': (44100, 1, 30)}


def kernel_times(loader, ti, n_batches, reps, ref_files):
    import stretch_ref as R
    import ctypes

    from sad import _lib
    dev = ti.device
    ms, ws_mib, kinds, ref_s = [], [], [0] * 11, []
    for k, batch in enumerate(loader):
        if k >= n_batches:
            break
        if batch is None or batch.stretch_off is None:
            continue
        d_arena = batch.arena.to(dev)
        mono = torch.empty(max(batch.mono_bytes, 16), device=dev, dtype=torch.uint8)
        for kind in batch.stretch_table[:, 0].tolist():
            kinds[kind] += 1
        need = _lib.SZ()
        _lib.call('sad_wave_stretch_workspace_size', batch.table.data_ptr(), batch.stretch_table.data_ptr(),
                  batch.n_files, ctypes.byref(need))
        ws_mib.append(need.value / 2 ** 20)
        ms.append(min(_events_ms(lambda: ti.wave_stretch(batch, d_arena, mono), reps)))
        if k == 0:  # the contract on the host, on the heads this batch holds
            for f in range(min(ref_files, batch.n_files)):
                off, n_read, _, ch, enc, _ = batch.table[f].tolist()
                kind, rate, steps, n_out = batch.stretch_table[f, :4].tolist()
                if kind < 6:
                    continue
                raw = batch.arena[off:off + n_read * ch * (2 if enc == 0 else 4)].numpy()
                x = raw.view(np.int16).astype(np.float64) / 32768.0 if enc == 0 else raw.view(np.float32).astype(np.float64)
                y = x.reshape(n_read, ch).mean(axis=1)
                p = np.array([rate, steps], np.int64).view(np.float64)
                p0, p1 = (p[0], p[1]) if kind in (6, 7, 10) else (p[1], 0.0)
                t0 = time.perf_counter()
                R.apply(R.STRETCH_KINDS[kind - 6], y, p0, p1)
                ref_s.append(time.perf_counter() - t0)
    if not ms:
        return None
    mean = lambda v: round(sum(v) / len(v), 4)  # noqa: E731
    return {'batches': len(ms), 'kinds_drawn': kinds, 'stretch_ms_per_batch': mean(ms),
            'stretch_ms_per_batch_min_max': [round(min(ms), 4), round(max(ms), 4)],
            'workspace_mib_per_batch': mean(ws_mib),
            'float64_contract_host_s_per_file': mean(ref_s) if ref_s else None, 'contract_files': len(ref_s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=256, help='training files per set')
    ap.add_argument('--distinct', type=int, default=8, help='different clips per class and set')
    ap.add_argument('--batch-size', type=int, default=32)
    ap.add_argument('--workers', default='12,0', help='DataLoader worker counts to run, each at most 16')
    ap.add_argument('--repeats', type=int, default=2, help='epochs per path and set (alternating)')
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'mixed', 'fp32'])
    ap.add_argument('--kernel-batches', type=int, default=3)
    ap.add_argument('--contract-files', type=int, default=4)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'wave_stretch_bench.json'))
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
    paths = ('plain', 'stretch')
    with tempfile.TemporaryDirectory() as tmp:
        for name, (sr, ch, seconds) in BENCH_SETS.items():
            root = os.path.join(tmp, name)
            write_set(root, sr, ch, seconds, args.files, args.distinct)
            entry = {'sample_rate': sr, 'channels': ch, 'seconds': seconds, 'workers': {}}
            for workers in worker_counts:
                loaders = {}
                for p in paths:
                    a = smt.parse_args(['--data-dir', root, '--batch-size', str(args.batch_size), '--workers',
                                        str(workers), '--precision', args.dtype, '--device-ingest'] +
                                       (['--wave-stretch', 'all'] if p == 'stretch' else []))
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
                       'stretch_over_plain': round(max(fps['stretch']) / max(fps['plain']), 3),
                       'plain_repeat_spread': round((max(fps['plain']) - min(fps['plain'])) / max(fps['plain']), 4),
                       'stretch_repeat_spread': round((max(fps['stretch']) - min(fps['stretch'])) /
                                                      max(fps['stretch']), 4),
                       'device_ms_per_step': {p: min(r['device_ms_per_step'] for r in runs[p]) for p in paths}}
                if workers == 0:
                    res['kernels'] = kernel_times(loaders['stretch'], ti, args.kernel_batches, 5, args.contract_files)
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
