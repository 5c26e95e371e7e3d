#!/usr/bin/env python3
"""bf16 against fp16 on the bench's workload, in one process: 2,048 synthesised
segments (sad_synth_pcm seed 0, bench.py's rank-0 batch), the 6-head n6
ensemble, micro-batch 2,048.  One engine per mode; the two alternate in blocks
of timed steps (bf16, fp16, bf16, fp16, ...: tools/bench_shared_trunk.py's
alternation), so that clock and thermal drift hit both alike.  A step is the
whole forward_pcm (front end, backbone, heads), timed with device events.

Per mode it prints and stores the per-block ms per step and segments/s, and the
sad_profile bracket per block-conv variant (total ms, kernel launches, TFLOP/s
of one backbone pass), which says which kernel pays for a difference.

  python tools/bench_precision.py --out profiles/fp16_bench.json
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'synthetic-audio-detection_amd'))

import torch  # noqa: E402

SEG = 128000
VARIANTS = (40, 43, 41, 44, 31)  # the bf16 / fp16 plan's kernels, in layer order (0: all of them)


def timed_steps(eng, pcm, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        eng.forward_pcm(pcm)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / steps


def brackets(eng, maps):
    """{variant: {ms, launches, tflops}} of one backbone pass (0 = every block-conv kernel)"""
    from sad import _lib
    out = {}
    for v in (0,) + VARIANTS:
        _lib.call('sad_profile_begin')
        eng.backbones[0](maps)
        ms, n, fl = _lib.ctypes.c_double(), _lib.I64(), _lib.ctypes.c_double()
        _lib.call('sad_profile_end', v, _lib.ctypes.byref(ms), _lib.ctypes.byref(n), _lib.ctypes.byref(fl))
        out[str(v)] = {'ms': round(ms.value, 3), 'launches': n.value,
                       'tflops': round(fl.value / ms.value / 1e9, 1) if ms.value > 0 else 0.0}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=2048, help='segments per step (bench.py: 2048)')
    ap.add_argument('--blocks', type=int, default=4, help='timed blocks per mode')
    ap.add_argument('--steps', type=int, default=20, help='timed steps per block')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--modes', nargs='+', default=['bf16', 'fp16'], choices=['bf16', 'fp16'])
    ap.add_argument('--out', default=None, help='JSON file for the results')
    args = ap.parse_args()
    from sad import _lib
    from sad import weights as sw
    from sad.engine import Engine
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    B = args.batch
    sd = sw.merged_state_dict(0, 6, False,
                              bn_stats=sw.load_bn_stats(os.path.join(ROOT, 'tests', 'golden', 'bn_stats_n6.npz')))
    pcm = torch.empty(B, SEG, dtype=torch.int16, device=dev)
    _lib.call('sad_synth_pcm', 0, 0, B, SEG, _lib.ptr(pcm), _lib.stream_handle(dev))
    engines = {m: Engine(sd, dev, dtype=m, micro_batch=B) for m in args.modes}
    for eng in engines.values():
        for _ in range(args.warmup):
            eng.forward_pcm(pcm)
    torch.cuda.synchronize()
    blocks = {m: [] for m in args.modes}
    for _ in range(args.blocks):
        for m in args.modes:
            blocks[m].append(timed_steps(engines[m], pcm, args.steps))
    maps = engines[args.modes[0]].frontend(pcm)
    results = []
    for m in args.modes:
        ms = blocks[m]
        rec = {'mode': m, 'batch': B, 'micro_batch': B, 'steps_per_block': args.steps,
               'block_ms_per_step': [round(x, 3) for x in ms],
               'block_segments_per_s': [round(B / x * 1e3, 1) for x in ms],
               'mean_segments_per_s': round(B / (sum(ms) / len(ms)) * 1e3, 1),
               'variant_brackets': brackets(engines[m], maps)}
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if len(results) == 2:
        lo = [min(r['block_ms_per_step']) for r in results]
        hi = [max(r['block_ms_per_step']) for r in results]
        print(f'{results[1]["mode"]} blocks {lo[1]:.3f} .. {hi[1]:.3f} ms, {results[0]["mode"]} blocks '
              f'{lo[0]:.3f} .. {hi[0]:.3f} ms per step')
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump({'device': torch.cuda.get_device_name(dev), 'results': results}, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
