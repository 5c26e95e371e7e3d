#!/usr/bin/env python3
"""Detection on audio that is still arriving: ``inference_runner.py`` for a
live feed.

The feed is read chunk by chunk -- headerless samples from a file, a FIFO or
stdin (``--raw``), or a WAV fed in pieces of ``--chunk-ms`` (``--wav``) -- and
every 4 s window is decided as soon as its last sample exists: one JSON line
per window event on stdout.  At the end of the feed the record that
``inference_runner.py`` writes for the same samples as a file goes to
``--output-json``, bit for bit (sad/stream.py, csrc/stream.hip).

``--merged-model``, ``--precision``, ``--model-name``, ``--threshold``,
``--batch-size``, ``--smooth`` and ``--output-json`` behave as in
inference_runner.py.  ``--smooth`` needs eight later windows, so the final
record has the smoothed labels and the events do not.  One bank per process
and GPU; a service with many feeds uses ``sad.stream.StreamBank`` directly.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import inference_runner as _ir  # noqa: E402
from sad import audio as _audio  # noqa: E402
from sad import engine as _engine  # noqa: E402
from sad import weights as _weights  # noqa: E402
from sad.stream import StreamBank  # noqa: E402

RAW_FORMATS = {'s16le': np.dtype('<i2'), 'f32le': np.dtype('<f4')}  # the host is little-endian, as a WAV is
READ_BYTES = 1 << 16


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser(description='Multi-head inference on a live feed, window by window.')
    parser.add_argument('--merged-model', type=str, required=True, help='Path to merged .pth')
    src = parser.add_mutually_exclusive_group(required=True)
    src.add_argument('--raw', metavar='FILE|-', help='headerless interleaved samples from a file, a FIFO or stdin (-), '
                                                     'read as they arrive')
    src.add_argument('--wav', metavar='FILE', help='a WAV file, fed in pieces of --chunk-ms')
    parser.add_argument('--rate', type=int, default=32000, help='--raw: sample rate (Hz)')
    parser.add_argument('--channels', type=int, default=1, help='--raw: interleaved channels (1..64)')
    parser.add_argument('--format', choices=list(RAW_FORMATS), default='s16le', help='--raw: sample encoding')
    parser.add_argument('--chunk-ms', type=int, default=100, help='--wav: milliseconds of audio per push')
    parser.add_argument('--overlap', type=float, default=0.0,
                        help='window overlap: 0.0 is inference_runner.py\'s value; 0.85 (the reference dataclass\'s '
                             'default) gives a decision every 0.6 s')
    parser.add_argument('--silence-threshold', type=float, default=1e-3)
    parser.add_argument('--threshold', type=float, default=0.5, help='Threshold for deciding Real vs Synthetic')
    parser.add_argument('--device', type=str, default='cuda')
    parser.add_argument('--smooth', action='store_true', help='Apply smoothing across windows (final record only).')
    parser.add_argument('--output-json', type=str, default='results.json')
    parser.add_argument('--precision', choices=['fp32', 'bf16x3', 'bf16', 'fp16'], default='fp32')
    parser.add_argument('--batch-size', type=int, default=128, help='windows per device launch')
    parser.add_argument('--model-name', default='resnet18', choices=list(_weights.ARCHS))
    return parser


def raw_chunks(path: str, dtype: np.dtype, channels: int):
    """Whole frames of a headerless stream as they arrive.  A partial trailing
    frame stays on the host until its rest arrives; one left at the end of the
    stream is dropped."""
    fd = sys.stdin.fileno() if path == '-' else os.open(path, os.O_RDONLY)
    frame = dtype.itemsize * channels
    rest = b''
    try:
        while True:
            data = os.read(fd, READ_BYTES)
            if not data:
                break
            data = rest + data
            whole = len(data) // frame * frame
            rest = data[whole:]
            if whole:
                yield np.frombuffer(data[:whole], dtype=dtype)
    finally:
        if path != '-':
            os.close(fd)
    if rest:
        print(f'dropped {len(rest)} trailing bytes: not a whole frame', file=sys.stderr)


def wav_chunks(samples: np.ndarray, channels: int, rate: int, chunk_ms: int):
    step = max(1, rate * chunk_ms // 1000) * channels
    for pos in range(0, samples.shape[0], step):
        yield samples[pos:pos + step]


def main(argv=None):
    args = build_parser().parse_args(argv)
    device = _engine._dev(args.device)
    with contextlib.redirect_stdout(sys.stderr):  # stdout carries the event lines only
        model, metadata = _ir.load_merged_model(args.merged_model, device, backbone_name=args.model_name,
                                                precision=args.precision)
    class_names = metadata['class_names']
    audio_cfg = _ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=args.overlap,
                                silence_threshold=args.silence_threshold)
    spec_cfg = _ir.SpectrogramConfig(n_fft=2048, hop_length=512, n_mels=128, f_min=20, f_max=12000, top_db=80,
                                     norm='slaney')
    if args.wav:
        samples, channels, rate = _audio.read_wav(args.wav)
        if samples.dtype not in (np.int16, np.float32):
            samples = samples.astype(np.float32)
        samples = samples.reshape(-1)
        name, dtype = args.wav, samples.dtype
        chunks = wav_chunks(samples, channels, rate, args.chunk_ms)
        max_chunk = max(1, rate * args.chunk_ms // 1000)
    else:
        channels, rate, dtype = args.channels, args.rate, RAW_FORMATS[args.format]
        name = args.raw
        chunks = raw_chunks(args.raw, dtype, channels)
        max_chunk = max(1, READ_BYTES // (dtype.itemsize * channels))
    bank = StreamBank(model.engine, class_names, 1, audio_cfg, spec_cfg, max_chunk, threshold=args.threshold,
                      batch_size=args.batch_size)
    slot = bank.open(name, rate, channels, dtype)

    def emit(events):
        for ev in events:
            line = {'slot': ev['slot'], 'name': ev['name'], 'start_sec': ev['start_sec'], 'end_sec': ev['end_sec'],
                    'label': ev['label'], 'probs': [float(v) for v in ev['probs']],
                    'logits': [float(v) for v in ev['logits']]}
            print(json.dumps(line), flush=True)

    for chunk in chunks:
        emit(bank.push({slot: chunk}))
    out = bank.close(slot, smooth=args.smooth)
    emit(bank.last_events)
    with open(args.output_json, 'w', encoding='utf-8') as f:
        json.dump(out, f, indent=4)
    print('Wrote results to', args.output_json, file=sys.stderr)
    return out


if __name__ == '__main__':
    main()
