#!/usr/bin/env python3
"""Live streams: S concurrent feeds through one StreamBank against the same
feeds handled one at a time, same process, same model.

Workload: S 44.1 kHz stereo int16 feeds deliver 100 ms (4410 frames) each per
tick, bf16 engine, n6 fixture model, at window overlap 0.85 (a decision every
0.6 s) and 0.0.  The audio is seeded (sad.synth): one stereo master, each feed
reading it from its own offset.  Before the clock starts every feed gets one
window of audio plus a stretch of its own length, so windows complete from the
first timed tick on and the feeds' windows complete on different ticks (as
unrelated feeds' do); --warm-ticks ticks then warm every shape.

  (a) bank      one StreamBank.push per tick for all S feeds: one upload, one
                sad_stream_push_run, one wait
  (b) per feed  the same feeds one at a time: one single-slot push per feed per
                tick (S uploads, launches and waits per tick), in a bank of its own

The two alternate in blocks of --block ticks.  A tick is timed with a host
clock around the push call(s), which end in the device wait.  (b) costs S
waits per tick, so it is timed for --compare-ticks ticks only.  Per S the tool
prints and writes to --out: the bank's tick time (p50 / p99 / max), the audio
seconds ingested per wall second, windows per tick, and the ratio of (b)'s mean
tick to the bank's.

The push kernel's own time comes from a profiler run of its own: run the tool
with --profile-only under `rocprofv3 --kernel-trace --stats --output-format csv
-d DIR/S<slots> -o run` at one overlap, then pass --kernel-stats-dir DIR (and
--kernel-stats-overlap) to the measuring run, which copies stream_push_kernel's
row into the records of that overlap; the others carry null.

    python tools/bench_stream.py [--slots 1,64,1024,8192] [--overlaps 0.85,0.0] [--out profiles/stream_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'synthetic-audio-detection_amd')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

RATE, CHANNELS, CHUNK_MS = 44100, 2, 100
CHUNK = RATE * CHUNK_MS // 1000  # frames per tick and feed


def master_audio(seed: int, seconds: float) -> np.ndarray:
    """Interleaved stereo int16 [frames * 2]: seeded segments of sad.synth, the
    right channel a delayed copy of the left."""
    from sad import synth
    n = int(seconds * RATE)
    segs = -(-n // synth.SEG_SAMPLES)
    left = np.concatenate([synth.synth_segment(seed, k) for k in range(segs)])[:n]
    return np.stack([left, np.roll(left, 37)], axis=1).reshape(-1)


class Feeds:
    """S feeds reading one master, each from its own frame offset, cyclically."""

    def __init__(self, master: np.ndarray, n: int, seed: int):
        self.master = np.concatenate([master, master[:2 * CHANNELS * RATE * 5]])  # 5 s of wrap-around
        self.frames = master.shape[0] // CHANNELS
        rs = np.random.RandomState(seed)
        self.pos = rs.randint(0, self.frames, size=n).astype(np.int64)

    def take(self, s: int, frames: int) -> np.ndarray:
        p = int(self.pos[s])
        self.pos[s] = (p + frames) % self.frames
        return self.master[p * CHANNELS:(p + frames) * CHANNELS]


def kernel_stats(path_dir: str, slots: int):
    """stream_push_kernel's row of a rocprofv3 --stats CSV under path_dir/S<slots>."""
    for f in glob.glob(os.path.join(path_dir, f'S{slots}', '**', '*kernel_stats.csv'), recursive=True):
        with open(f, newline='') as fh:
            for row in csv.DictReader(fh):
                if 'stream_push_kernel' in row.get('Name', ''):
                    return {'calls': int(row['Calls']), 'average_us': float(row['AverageNs']) / 1e3,
                            'min_us': float(row['MinNs']) / 1e3, 'max_us': float(row['MaxNs']) / 1e3}
    return None


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--slots', default='1,64,1024,8192')
    ap.add_argument('--overlaps', default='0.85,0.0')
    ap.add_argument('--precision', default='bf16')
    ap.add_argument('--ticks', type=int, default=200, help='timed bank ticks per (S, overlap)')
    ap.add_argument('--warm-ticks', type=int, default=45)
    ap.add_argument('--block', type=int, default=50, help='bank ticks per block; (b) runs between blocks')
    ap.add_argument('--compare-ticks', type=int, default=0,
                    help='per-feed ticks per (S, overlap); 0: max(4, min(ticks, 16384 // S))')
    ap.add_argument('--batch-size', type=int, default=2048)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--profile-only', action='store_true', help='bank ticks only, no comparison, no file written')
    ap.add_argument('--kernel-stats-dir', default='')
    ap.add_argument('--kernel-stats-overlap', type=float, default=0.85,
                    help='the overlap the profiler runs used: records of another overlap carry no kernel time')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stream_bench.json'))
    args = ap.parse_args(argv)

    import inference_runner as ir
    from sad import weights as sw
    from sad.engine import Engine
    from sad.stream import StreamBank
    dev = torch.device('cuda', 0)
    names = [f'Synthetic{chr(65 + i)}' for i in range(6)] + ['Real']
    stats = sw.load_bn_stats(os.path.join(ROOT, 'tests', 'golden', 'bn_stats_n6.npz'))
    eng = Engine(sw.merged_state_dict(0, 6, False, bn_stats=stats), dev, dtype=args.precision,
                 micro_batch=args.batch_size)
    master = master_audio(args.seed, 64.0)
    results = []
    for S in [int(v) for v in args.slots.split(',')]:
        for overlap in [float(v) for v in args.overlaps.split(',')]:
            cfg = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=overlap, silence_threshold=1e-3)

            def make():
                bank = StreamBank(eng, names, S, cfg, ir.SpectrogramConfig(), CHUNK, batch_size=args.batch_size)
                feeds = Feeds(master, S, args.seed + 1)
                slots = [bank.open(f'feed{s}', RATE, CHANNELS, np.int16) for s in range(S)]
                # one window of audio so that windows complete from the first timed tick on, plus a
                # phase of its own per feed, spread over one hop
                rs = np.random.RandomState(args.seed + 2)
                hop_frames = int(bank.hop * RATE / 32000)
                first = int(bank.window * RATE / 32000) + rs.randint(0, hop_frames, size=S)
                for lo in range(0, int(first.max()) + 1, CHUNK):  # in pieces of at most one chunk
                    bank.push({s: feeds.take(s, int(min(CHUNK, first[s] - lo))) for s in slots if first[s] > lo})
                return bank, feeds, slots

            bank, feeds, slots = make()

            def bank_tick():
                push = {s: feeds.take(s, CHUNK) for s in slots}
                t0 = time.perf_counter()
                ev = bank.push(push)
                return time.perf_counter() - t0, len(ev)

            for _ in range(args.warm_ticks):
                bank_tick()
            if args.profile_only:
                for _ in range(args.ticks):
                    bank_tick()
                print(json.dumps({'slots': S, 'overlap': overlap, 'profile_only': True, 'ticks': args.ticks}))
                del bank
                torch.cuda.empty_cache()
                continue
            one, feeds1, slots1 = make()

            def feed_tick():
                chunks = [feeds1.take(s, CHUNK) for s in slots1]
                t0 = time.perf_counter()
                n = 0
                for s, c in zip(slots1, chunks):
                    n += len(one.push({s: c}))
                return time.perf_counter() - t0, n

            n_cmp = args.compare_ticks or max(4, min(args.ticks, 16384 // S))
            for _ in range(min(args.warm_ticks, max(2, n_cmp // 2))):
                feed_tick()
            tb, wb, tf, wf = [], [], [], []
            blocks = -(-args.ticks // args.block)
            for b in range(blocks):
                for _ in range(min(args.block, args.ticks - len(tb))):
                    t, n = bank_tick()
                    tb.append(t)
                    wb.append(n)
                for _ in range(-(-n_cmp // blocks) if len(tf) < n_cmp else 0):
                    t, n = feed_tick()
                    tf.append(t)
                    wf.append(n)
            tb_ms, tf_ms = np.array(tb) * 1e3, np.array(tf) * 1e3
            rec = {
                'metric': 'live streams: S 44.1 kHz stereo int16 feeds, 100 ms chunks; host clock around one '
                          'StreamBank.push per tick (ends in its one device wait) vs one single-slot push per feed',
                'precision': args.precision, 'slots': S, 'overlap': overlap, 'batch_size': args.batch_size,
                'bank': {'ticks': len(tb), 'tick_ms_p50': round(float(np.percentile(tb_ms, 50)), 3),
                         'tick_ms_p99': round(float(np.percentile(tb_ms, 99)), 3),
                         'tick_ms_max': round(float(tb_ms.max()), 3), 'tick_ms_mean': round(float(tb_ms.mean()), 3),
                         'audio_s_per_wall_s': round(S * CHUNK_MS / 1e3 * len(tb) / float(np.sum(tb)), 1),
                         'windows_per_tick': round(float(np.mean(wb)), 2),
                         'p99_below_chunk': bool(np.percentile(tb_ms, 99) < CHUNK_MS)},
                'per_feed': {'ticks': len(tf), 'tick_ms_mean': round(float(tf_ms.mean()), 3),
                             'tick_ms_max': round(float(tf_ms.max()), 3),
                             'audio_s_per_wall_s': round(S * CHUNK_MS / 1e3 * len(tf) / float(np.sum(tf)), 1),
                             'windows_per_tick': round(float(np.mean(wf)), 2)},
                'ratio_per_feed_over_bank': round(float(tf_ms.mean() / tb_ms.mean()), 2),
                'push_kernel': kernel_stats(args.kernel_stats_dir, S)
                if args.kernel_stats_dir and overlap == args.kernel_stats_overlap else None,
            }
            print(json.dumps(rec), flush=True)
            results.append(rec)
            del bank, one
            torch.cuda.empty_cache()
    if not args.profile_only:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(results, f, indent=1)
            f.write('\n')
    return results


if __name__ == '__main__':
    main()
