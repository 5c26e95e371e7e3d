#!/usr/bin/env python3
"""Scan a folder or a list of WAV files in one run: the catalogue counterpart of
``inference_runner.py --audio ONE.wav`` (the reference's earlier tool had a
folder mode, legacy/source/inference_script.py ``--IsBatch``).

    python catalog_runner.py --merged-model merged.pth --audio-dir DIR --output-json out.json
    python catalog_runner.py --merged-model merged.pth --file-list files.txt --gpus 8

The checkpoint is loaded once; the windows of many files are packed into full
device batches; the device picks the windows to keep and does the per-file
smoothing, decisions and averages (sad/scan.py, csrc/scan.hip).  The output is
ONE JSON list holding, per file and in input order, the record that
``inference_runner.main`` writes for that file alone, or ``{'filename',
'error'}`` for a file that cannot be read.

``--gpus N`` splits the list by file: rank 0 reads the WAV headers and cuts the
list into N contiguous ranges balanced by candidate-window count, every rank
scans and post-processes its own range, rank 0 gathers the records and writes
the file.  Without a launcher the N ranks are started here (sad/launch.py).
"""
from __future__ import annotations

import argparse
import glob
import json
import os
import random
import sys

import numpy as np
import torch
import torch.distributed as dist

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import inference_runner as _ir  # noqa: E402
from sad import launch as _launch  # noqa: E402
from sad import scan as _scan  # noqa: E402
from sad import weights as _weights  # noqa: E402

DEFAULT_BATCH = {'bf16': 2048, 'fp16': 2048, 'bf16x3': 512, 'fp32': 128}  # as bench.py (fp16: bf16's)


def list_files(args) -> list:
    if args.audio_dir:
        return sorted(glob.glob(os.path.join(args.audio_dir, '*.wav')))
    with open(args.file_list, encoding='utf-8') as f:
        return [ln.strip() for ln in f if ln.strip()]


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description='Multi-head inference over many WAV files in one run.')
    p.add_argument('--merged-model', type=str, required=True, help='Path to merged .pth')
    src = p.add_mutually_exclusive_group(required=True)
    src.add_argument('--audio-dir', type=str, help='folder: its *.wav files, sorted')
    src.add_argument('--file-list', type=str, help='text file, one WAV path per line')
    p.add_argument('--output-json', type=str, default='results.json', help='one JSON list, a record per file')
    p.add_argument('--threshold', type=float, default=0.5, help='Threshold for deciding Real vs Synthetic')
    p.add_argument('--smooth', action='store_true', help='Apply smoothing across a file\'s windows.')
    p.add_argument('--precision', choices=['fp32', 'bf16x3', 'bf16', 'fp16'], default='fp32')
    p.add_argument('--model-name', default='resnet18', choices=list(_weights.ARCHS))
    p.add_argument('--batch-size', type=int, default=0,
                   help='windows per device batch (0: 2048 bf16 / fp16, 512 bf16x3, 128 fp32)')
    p.add_argument('--pack-seconds', type=float, default=_scan.DEFAULT_PACK_SECONDS,
                   help='seconds of 32 kHz audio per pack (one upload and one host wait each)')
    p.add_argument('--workers', type=int, default=_scan.DEFAULT_WORKERS,
                   help=f'file-reading threads (at most {_scan.MAX_WORKERS})')
    p.add_argument('--overlap', type=float, default=0.0, help='window overlap fraction (the reference\'s main: 0.0)')
    p.add_argument('--gpus', type=int, default=1)
    p.add_argument('--backend', default='nccl', choices=['nccl', 'gloo'], help='gloo: tests only')
    p.add_argument('--one-device', action='store_true', help='every rank on cuda:0 (2-rank test on one GPU)')
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    batch = args.batch_size or DEFAULT_BATCH[args.precision]
    if args.gpus > 1 and not _launch.under_launcher():
        rc = _launch.relaunch(args.gpus, os.path.abspath(__file__), sys.argv[1:] if argv is None else list(argv))
        if argv is None:
            sys.exit(rc)
        return rc
    world, rank, local = _launch.check_world(args.gpus)
    device = torch.device('cuda', 0 if args.one_device else local)
    torch.cuda.set_device(device)
    if world > 1:
        if args.backend == 'nccl':
            dist.init_process_group('nccl', device_id=device)
        else:
            dist.init_process_group('gloo')

    seed = 9
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    model, metadata = _ir.load_merged_model(args.merged_model, device, backbone_name=args.model_name,
                                            precision=args.precision)
    eng = model.engine
    for bb in eng.backbones:  # bench.py's micro-batch for the precision, not the single-file tool's 64
        bb.micro_batch = max(1, batch)
    scanner = _scan.Scanner(eng, metadata['class_names'], threshold=args.threshold, smooth=args.smooth,
                            batch_size=batch, pack_seconds=args.pack_seconds, workers=args.workers,
                            overlap=args.overlap)

    paths = list_files(args)
    lo, hi = 0, len(paths)
    if world > 1:
        ranges = [None]
        if rank == 0:  # headers only: the split needs the candidate counts, not the samples
            infos = [_scan.wav_info(p) for p in paths]
            counts = [0 if i.error else _scan.candidate_count(_scan.slot_len(i, scanner.sr, scanner.window),
                                                              scanner.window, scanner.hop) for i in infos]
            ranges = [_scan.split_ranks(counts, world)]
        dist.broadcast_object_list(ranges, src=0)
        lo, hi = ranges[0][rank]
    records = scanner.scan(paths[lo:hi])
    if world > 1:
        parts = [None] * world if rank == 0 else None
        dist.gather_object(records, parts, dst=0)
        if rank == 0:
            records = [r for part in parts for r in part]
        dist.barrier()
        dist.destroy_process_group()
    if rank != 0:
        return None
    with open(args.output_json, 'w', encoding='utf-8') as f:
        json.dump(records, f, indent=4)
    n_err = sum('error' in r for r in records)
    print(f'Scanned {len(records)} file(s), {scanner.stats["segments"]} segment(s) on rank 0, {n_err} unreadable; '
          f'wrote {args.output_json}')
    return records


if __name__ == '__main__':
    main()
