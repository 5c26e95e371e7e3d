#!/usr/bin/env python3
"""Catalogue scan against the one-file-at-a-time path, same process, same model.

Writes a seeded catalogue of WAV files to a temporary folder (default 512 files
of 30-240 s, 32 / 44.1 kHz and mono / stereo mixed, a silent stretch in every
fourth file), then times, alternating, whole-catalogue passes that end in a
device synchronise:

  (a) per file   the parent commit's way with the model loaded ONCE:
                 preprocess_waveform + select_windows + run_windows + summarize
                 per file (inference_runner.main's body without the checkpoint
                 load and the JSON file)
  (b) scanner    sad.scan.Scanner over the same list

Both paths are warmed first (a pass over the first --warm-files files, plus one
full scanner pass so its pinned and device buffers have their final size), use
the same windows-per-launch and micro-batch, and must return the same records
(checked: segments identical, percentages within 1e-3).  Prints one JSON line
per precision and writes them all to --out: files/s and segments/s for each
path, the scanner's host stages (header parse, waiting for reads, queueing the
upload / ingestion / selection, waiting for the device, queueing the batches,
building records, JSON text), its device stages between stream events (upload,
ingestion, selection, front end + ensemble, post-processing), and, with
--headline-json (a file holding bench.py's
result line of the same build), the engine's own segments/s beside the scanner's.
The yardstick is path (a); the scanner is never compared with itself.

    python tools/bench_scan.py [--files 512] [--precisions bf16,bf16x3,fp32] [--out profiles/scan_bench.json]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'synthetic-audio-detection_amd')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

DEFAULT_BATCH = {'bf16': 2048, 'bf16x3': 512, 'fp32': 128}


def write_catalogue(folder: str, n_files: int, min_s: float, max_s: float, seed: int):
    """Seeded WAVs cut from one noise + tone master per (rate, channels)."""
    from sad.audio import save_pcm16
    rs = np.random.RandomState(seed)
    masters = {}
    paths, seconds = [], 0.0
    for i in range(n_files):
        sr, ch = (32000, 44100)[rs.randint(2)], 1 + rs.randint(2)
        dur = rs.uniform(min_s, max_s)
        n = int(dur * sr)
        if (sr, ch) not in masters:
            T = int((max_s + 60) * sr)
            t = np.arange(T) / sr
            sig = 0.3 * np.sin(2 * np.pi * 440 * t) * (1 + 0.5 * np.sin(2 * np.pi * 0.1 * t)) + 0.05 * rs.randn(T)
            masters[(sr, ch)] = (np.stack([np.roll(sig, 11 * c) for c in range(ch)]) * 20000).astype(np.int16)
        m = masters[(sr, ch)]
        o = rs.randint(m.shape[1] - n)
        pcm = m[:, o:o + n].copy()
        if i % 4 == 3:  # 9 s of silence: at least one whole window is dropped
            q = rs.randint(max(1, n - 9 * sr))
            pcm[:, q:q + 9 * sr] = 0
        p = os.path.join(folder, f'clip_{i:05d}.wav')
        save_pcm16(p, pcm, sr)
        paths.append(p)
        seconds += dur
    return paths, seconds


def per_file_pass(ir, ingest, model, names, paths, batch):
    """(a): inference_runner.main's body per file, model loaded once."""
    audio_cfg = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=0.0, silence_threshold=1e-3)
    spec_cfg = ir.SpectrogramConfig()
    out, nseg = [], 0
    for p in paths:
        wf, sr = ir.preprocess_waveform(p, audio_cfg, model.device)
        starts, ts = ingest.select_windows(wf, sr, audio_cfg.window_size, audio_cfg.overlap,
                                           audio_cfg.silence_threshold)
        if not starts:
            out.append({'filename': p, 'segments': [], 'percentages': {}})
            continue
        logits = ir.run_windows(model, ingest.Windows(wf, starts, int(audio_cfg.window_size * sr)), sr, spec_cfg,
                                batch)
        out.append(ir.summarize(p, logits, ts, 0.5, names[:-1], names[-1], False, audio_cfg.window_size))
        nseg += len(starts)
    torch.cuda.synchronize()
    return out, nseg


def same_records(a, b):
    for x, y in zip(a, b):
        if x['filename'] != y['filename'] or x['segments'] != y['segments']:
            return False
        if set(x['percentages']) != set(y['percentages']):
            return False
        if any(abs(x['percentages'][k] - y['percentages'][k]) > 1e-3 for k in x['percentages']):
            return False
    return len(a) == len(b)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--files', type=int, default=512)
    ap.add_argument('--min-seconds', type=float, default=30.0)
    ap.add_argument('--max-seconds', type=float, default=240.0)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--precisions', default='bf16,bf16x3,fp32')
    ap.add_argument('--passes', type=int, default=2, help='timed passes per path, alternating (a), (b)')
    ap.add_argument('--warm-files', type=int, default=8)
    ap.add_argument('--pack-seconds', type=float, default=0.0, help='0: the scanner default')
    ap.add_argument('--workers', type=int, default=8)
    ap.add_argument('--headline-json', default='', help="file with bench.py's JSON line of the same build")
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'scan_bench.json'))
    args = ap.parse_args(argv)

    import inference_runner as ir
    from sad import ingest, scan
    from sad import weights as sw
    dev = torch.device('cuda', 0)
    folder = tempfile.mkdtemp(prefix='scan_bench_')
    try:
        t0 = time.perf_counter()
        paths, seconds = write_catalogue(folder, args.files, args.min_seconds, args.max_seconds, args.seed)
        t_write = time.perf_counter() - t0
        names = [f'Synthetic{chr(65 + i)}' for i in range(6)] + ['Real']
        stats = sw.load_bn_stats(os.path.join(ROOT, 'tests', 'golden', 'bn_stats_n6.npz'))
        ckpt = os.path.join(folder, 'merged_n6.pth')
        torch.save({'state_dict': sw.merged_state_dict(0, 6, False, bn_stats=stats),
                    'metadata': {'class_names': names}}, ckpt)
        headline = None
        if args.headline_json:
            with open(args.headline_json) as f:
                headline = [json.loads(s) for s in f.read().splitlines() if s.startswith('{')][-1]
        results = []
        for prec in args.precisions.split(','):
            batch = DEFAULT_BATCH[prec]
            model, _ = ir.load_merged_model(ckpt, dev, precision=prec)
            for bb in model.engine.backbones:
                bb.micro_batch = batch

            def scanner():
                kw = {'pack_seconds': args.pack_seconds} if args.pack_seconds else {}
                return scan.Scanner(model.engine, names, batch_size=batch, workers=args.workers, **kw)

            sc = scanner()
            per_file_pass(ir, ingest, model, names, paths[:args.warm_files], batch)
            sc.scan(paths[:args.warm_files])
            sc.scan(paths)  # buffers at their final size
            torch.cuda.synchronize()
            ta, tb, stages = [], [], None
            for _ in range(args.passes):
                t0 = time.perf_counter()
                ra, nseg_a = per_file_pass(ir, ingest, model, names, paths, batch)
                ta.append(time.perf_counter() - t0)
                sc.stats = {k: (0.0 if isinstance(v, float) else 0) for k, v in sc.stats.items()}
                t0 = time.perf_counter()
                rb = sc.scan(paths)
                torch.cuda.synchronize()
                tb.append(time.perf_counter() - t0)
                stages = dict(sc.stats)
            t0 = time.perf_counter()
            text = json.dumps(rb, indent=4)
            t_json = time.perf_counter() - t0
            a, b = min(ta), min(tb)
            rec = {
                'metric': 'catalogue scan vs one file at a time (model loaded once), whole-catalogue wall clock '
                          'ending in a device synchronise, best of the timed passes',
                'precision': prec, 'batch_size': batch, 'files': len(paths), 'audio_seconds': round(seconds, 1),
                'segments': stages['segments'], 'records_equal': same_records(ra, rb) and nseg_a == stages['segments'],
                'per_file': {'seconds': round(a, 4), 'files_per_s': round(len(paths) / a, 2),
                             'segments_per_s': round(nseg_a / a, 1), 'passes_s': [round(v, 4) for v in ta]},
                'scanner': {'seconds': round(b, 4), 'files_per_s': round(len(paths) / b, 2),
                            'segments_per_s': round(stages['segments'] / b, 1), 'passes_s': [round(v, 4) for v in tb],
                            'packs': stages['packs'], 'host_waits': stages['syncs'],
                            'stages_s_last_pass': {k: round(v, 4) for k, v in stages.items() if k.endswith('_s')},
                            'json_text_s': round(t_json, 4), 'json_bytes': len(text)},
                'speedup_scanner_over_per_file': round(a / b, 3),
                'catalogue_write_s': round(t_write, 2),
            }
            if headline is not None and prec == 'bf16':
                rec['bench_py_headline_segments_per_s'] = headline.get('value')
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del sc, model
            torch.cuda.empty_cache()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')
        return results
    finally:
        shutil.rmtree(folder, ignore_errors=True)


if __name__ == '__main__':
    main()
