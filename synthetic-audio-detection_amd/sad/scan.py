"""Catalogue scan: a list or folder of WAV files in one run.

``inference_runner.main`` handles one file per process: one checkpoint load,
one host look at the window maxima, one Python loop over the rows.  Here many
files share the device batches:

  pack     files are read on a thread pool (sad.audio.read_wav) straight into a
           pinned buffer, uploaded as stored in ONE copy per pack, and turned
           into mono 32 kHz fp32 by the ingestion kernels, each into its own
           slot of one arena (slot = max(len, window) samples, zero tail: the
           reference's pad of a short file to one window)
  select   sad_scan_select_run: the device applies the silence test to every
           file's candidate windows and compacts the kept windows' arena
           offsets in file order, then time order
  infer    front end (windows read in place from the arena) + ensemble over the
           kept offsets, ``batch_size`` at a time: batches straddle files
  post     sad_scan_post_run: sigmoid, optional smoothing, labels and per-file
           means on the device; the host only formats the records

The host waits for the device once per pack: that wait delivers the previous
pack's results and this pack's kept-window count (which sizes its batches), and
the next pack's files are being read meanwhile.
"""
from __future__ import annotations

import math
import os
import struct
import time
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import audio as _audio
from . import ingest as _ingest

MAX_WORKERS = 16
DEFAULT_WORKERS = 8
DEFAULT_PACK_SECONDS = 16384.0  # 4096 windows at overlap 0: two bf16 batches of 2048


@dataclass
class FileInfo:
    """What the WAV header says about one file (no samples read)."""
    path: str
    frames: int = 0
    channels: int = 1
    sr: int = 0
    i16: bool = True           # stored as int16 (uploaded as is); else host-decoded fp32
    error: Optional[str] = None

    @property
    def raw_bytes(self) -> int:
        return self.frames * self.channels * (2 if self.i16 else 4)


def wav_info(path: str) -> FileInfo:
    """Header-only look at a WAV: frames, channels, rate and whether
    sad.audio.read_wav will return int16.  A file that cannot be parsed comes
    back with ``error`` set."""
    try:
        fmt, _, size = _audio._wav_layout(path)
        tag, ch, sr, _, _, bits = struct.unpack('<HHIIHH', fmt[:16])
        if tag == 0xFFFE and len(fmt) >= 26:
            tag = struct.unpack('<H', fmt[24:26])[0]
        if not ((tag == 1 and bits in (8, 16, 24, 32)) or (tag == 3 and bits in (32, 64))):
            raise ValueError(f'unsupported WAV format tag {tag:#x} / {bits} bits')
        if ch < 1 or ch > 64 or sr <= 0:
            raise ValueError(f'unsupported WAV layout: {ch} channels at {sr} Hz')
        return FileInfo(path, size // ((bits // 8) * ch), ch, sr, tag == 1 and bits == 16)
    except Exception as e:  # unreadable files become error records; the scan goes on
        return FileInfo(path, error=f'{type(e).__name__}: {e}')


def resampled_len(frames: int, sr: int, target_sr: int) -> int:
    """sad_resample_out_len: ceil(new * frames / orig), rates reduced by their gcd."""
    if sr == target_sr:
        return frames
    g = math.gcd(sr, target_sr)
    o, n = sr // g, target_sr // g
    return (n * frames + o - 1) // o


def slot_len(info: FileInfo, target_sr: int, window: int) -> int:
    """Samples of the file's arena slot: its 32 kHz length, at least one window."""
    return max(resampled_len(info.frames, info.sr, target_sr), window)


def candidate_count(n: int, window: int, hop: int) -> int:
    return len(_ingest.window_starts(n, window, hop))


def plan_packs(slots: Sequence[int], limit: int) -> List[List[int]]:
    """Consecutive files -> packs whose slots sum to at most `limit` samples.  A
    file is never split: one longer than the limit is a pack of its own."""
    packs, cur, used = [], [], 0
    for i, s in enumerate(slots):
        if cur and used + s > limit:
            packs.append(cur)
            cur, used = [], 0
        cur.append(i)
        used += s
    if cur:
        packs.append(cur)
    return packs


def split_ranks(counts: Sequence[int], world: int) -> List[Tuple[int, int]]:
    """Contiguous [start, stop) file ranges for `world` ranks, balanced by the
    files' candidate-window counts: rank r starts at the first file at which
    the running count reaches r / world of the total."""
    prefix = np.concatenate([[0], np.cumsum(np.asarray(counts, dtype=np.int64))])
    total, n = int(prefix[-1]), len(counts)
    cuts = [0]
    for r in range(1, world):
        c = int(np.searchsorted(prefix, -(-r * total // world), side='left')) if total else (r * n) // world
        cuts.append(min(max(c, cuts[-1]), n))
    cuts.append(n)
    return [(cuts[r], cuts[r + 1]) for r in range(world)]


def label_name(idx: int, synthetic_names: Sequence[str], real_name: str) -> str:
    if idx < 0:
        return real_name
    return synthetic_names[idx] if idx < len(synthetic_names) else f'Synthetic_{idx + 1}'


def assemble_records(filenames: Sequence[str], file_start, row_start, offsets, label, mean,
                     synthetic_names: Sequence[str], real_name: str, sr: int, window_size: float,
                     errors: Optional[Dict[int, str]] = None) -> List[dict]:
    """The per-file JSON records of inference_runner.summarize / main from the
    scan's arrays: file f owns rows [row_start[f], row_start[f+1]) of `offsets`
    (absolute arena samples) and `label` (-1 = Real, k = synthetic head k), and
    row f of `mean` ([n_files, N + 1] probabilities)."""
    errors = errors or {}
    out = []
    for f, name in enumerate(filenames):
        if f in errors:
            out.append({'filename': name, 'error': errors[f]})
            continue
        lo, hi = int(row_start[f]), int(row_start[f + 1])
        if hi <= lo:
            out.append({'filename': name, 'segments': [], 'percentages': {}})
            continue
        fs = int(file_start[f])
        segments = []
        for r in range(lo, hi):
            t = (int(offsets[r]) - fs) / sr
            segments.append({'start_sec': t, 'end_sec': t + window_size,
                             'label': label_name(int(label[r]), synthetic_names, real_name)})
        m = mean[f]
        pct = {label_name(i, synthetic_names, real_name): float(m[i] * 100) for i in range(len(m) - 1)}
        pct[real_name] = float(m[-1] * 100)
        out.append({'filename': name, 'segments': segments, 'percentages': pct})
    return out


def select_windows_arena(arena: torch.Tensor, file_start: torch.Tensor, file_len: torch.Tensor, window: int,
                         hop: int, silence_threshold: float, max_candidates: int,
                         offsets: Optional[torch.Tensor] = None):
    """sad_scan_select_run on device tensors -> (offsets [max_candidates] int64,
    row_start [n_files + 1] int64), both on the device; nothing is synchronised.
    `offsets`: the tensor to fill (entries past the kept count keep their values)."""
    dev = arena.device
    assert arena.dtype == torch.float32 and arena.dim() == 1 and arena.is_contiguous()
    for t in (file_start, file_len):
        assert t.dtype == torch.int64 and t.dim() == 1 and t.is_contiguous() and t.device == dev
    n = file_start.shape[0]
    assert file_len.shape[0] == n
    sz = _lib.SZ()
    _lib.call('sad_scan_select_workspace_size', n, int(max_candidates), _lib.ctypes.byref(sz))
    ws = torch.empty(max(sz.value, 8), dtype=torch.uint8, device=dev)
    if offsets is None:
        offsets = torch.empty(int(max_candidates), dtype=torch.int64, device=dev)
    assert offsets.dtype == torch.int64 and offsets.is_contiguous() and offsets.device == dev
    assert offsets.shape[0] >= int(max_candidates)
    row_start = torch.empty(n + 1, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        _lib.call('sad_scan_select_run', _lib.ptr(arena), arena.shape[0], _lib.ptr(file_start), _lib.ptr(file_len), n,
                  int(window), int(hop), float(silence_threshold), int(max_candidates), _lib.ptr(offsets),
                  _lib.ptr(row_start), _lib.ptr(ws), ws.numel(), _lib.stream_handle(dev))
    return offsets, row_start


def postprocess(logits: torch.Tensor, row_start: torch.Tensor, threshold: float, smooth: bool):
    """sad_scan_post_run -> (probs [B, C] fp32, label [B] int32, mean [n_files, C]
    float64) on the device; nothing is synchronised."""
    dev = logits.device
    assert logits.dtype == torch.float32 and logits.dim() == 2 and logits.is_contiguous()
    assert row_start.dtype == torch.int64 and row_start.dim() == 1 and row_start.is_contiguous()
    assert row_start.device == dev and row_start.shape[0] >= 1
    B, C = logits.shape
    n = row_start.shape[0] - 1
    sz = _lib.SZ()
    _lib.call('sad_scan_post_workspace_size', B, C, int(bool(smooth)), _lib.ctypes.byref(sz))
    ws = torch.empty(max(sz.value, 8), dtype=torch.uint8, device=dev)
    probs = torch.empty(B, C, dtype=torch.float32, device=dev)
    label = torch.empty(B, dtype=torch.int32, device=dev)
    mean = torch.empty(n, C, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.call('sad_scan_post_run', _lib.ptr(logits), B, C, _lib.ptr(row_start), n, float(threshold),
                  int(bool(smooth)), _lib.ptr(probs), _lib.ptr(label), _lib.ptr(mean), _lib.ptr(ws), ws.numel(),
                  _lib.stream_handle(dev))
    return probs, label, mean


def _align(v: int, a: int) -> int:
    return (v + a - 1) // a * a


class _Pack:
    """One pack in flight: its files, the pinned upload buffer's layout, and
    (after the device work is queued) the pinned result tensors."""

    def __init__(self, files: List[int], infos: Sequence[FileInfo], sr: int, window: int, hop: int):
        self.files = files
        self.slots = [slot_len(infos[i], sr, window) for i in files]
        self.starts, pos = [], 0
        for s in self.slots:
            self.starts.append(pos)
            pos = _align(pos + s, 4)  # float4-aligned slots
        self.arena_len = pos
        self.cap = sum(candidate_count(s, window, hop) for s in self.slots)
        n = len(files)
        self.byte_off, b = [], _align(16 * n, 16)  # [file_start | file_len] int64, then the files' samples
        for i in files:
            self.byte_off.append(b)
            b = _align(b + infos[i].raw_bytes, 16)
        self.nbytes = b
        self.reads = []
        self.errors: Dict[int, str] = {}
        self.n_kept = 0


class Scanner:
    """Scan WAV files with one engine.  ``scan(paths)`` returns one record per
    path, in input order: ``summarize``'s record, ``main``'s empty record for a
    file without a kept window, or ``{'filename', 'error'}``."""

    def __init__(self, engine, class_names: Sequence[str], threshold: float = 0.5, smooth: bool = False,
                 batch_size: int = 128, pack_seconds: float = DEFAULT_PACK_SECONDS, workers: int = DEFAULT_WORKERS,
                 overlap: float = 0.0, sample_rate: int = 32000, window_size: float = 4.0,
                 silence_threshold: float = 1e-3, keep_logits: bool = False):
        self.eng = engine
        self.dev = engine.device
        self.synthetic_names, self.real_name = list(class_names[:-1]), class_names[-1]
        self.threshold, self.smooth = float(threshold), bool(smooth)
        self.batch_size = max(1, int(batch_size))
        self.sr, self.window_size = int(sample_rate), float(window_size)
        self.window = int(window_size * sample_rate)
        self.hop = int((1 - overlap) * self.window)
        if self.hop <= 0:
            raise ValueError(f'hop of {self.hop} samples (overlap={overlap})')
        if self.window != engine.frontend.n_samples:
            raise ValueError(f'window of {self.window} samples, the engine front end takes {engine.frontend.n_samples}')
        self.silence_threshold = float(silence_threshold)
        self.pack_samples = max(self.window, int(pack_seconds * sample_rate))
        # threads, not processes: the reads release the GIL; never sized from the CPU count
        self.workers = max(1, min(int(workers), MAX_WORKERS))
        self.keep_logits = keep_logits
        self.logits: Dict[str, torch.Tensor] = {}  # keep_logits: path -> the file's merged logits (host)
        self.stats = {'files': 0, 'packs': 0, 'syncs': 0, 'segments': 0, 'candidates': 0, 'header_s': 0.0,
                      'read_wait_s': 0.0, 'stage_s': 0.0, 'sync_wait_s': 0.0, 'infer_enqueue_s': 0.0,
                      'records_s': 0.0, 'dev_upload_s': 0.0, 'dev_ingest_s': 0.0, 'dev_select_s': 0.0,
                      'dev_engine_s': 0.0, 'dev_post_s': 0.0}  # dev_*: device time between stream events
        self._pinned = [None, None]
        self._raw = self._arena = self._tmp = None

    # -- host buffers ------------------------------------------------------
    def _pinned_buf(self, slot: int, nbytes: int) -> torch.Tensor:
        if self._pinned[slot] is None or self._pinned[slot].numel() < nbytes:
            self._pinned[slot] = torch.empty(nbytes, dtype=torch.uint8, pin_memory=True)
        return self._pinned[slot]

    @staticmethod
    def _grown(t: Optional[torch.Tensor], n: int, dtype, dev) -> torch.Tensor:
        return t if t is not None and t.numel() >= n else torch.empty(n, dtype=dtype, device=dev)

    def _read_into(self, info: FileInfo, dst: np.ndarray) -> Optional[str]:
        """Reader thread: the file's samples as stored -> its bytes of the pinned buffer."""
        try:
            samples, ch, sr = _audio.read_wav(info.path)
            if samples.dtype not in (np.int16, np.float32):
                samples = samples.astype(np.float32)
            raw = samples.reshape(-1).view(np.uint8)
            if ch != info.channels or sr != info.sr or raw.shape[0] != dst.shape[0]:
                raise ValueError('samples do not match the WAV header')
            np.copyto(dst, raw)
            return None
        except Exception as e:
            return f'{type(e).__name__}: {e}'

    def _submit(self, pool: ThreadPoolExecutor, pack: _Pack, infos: Sequence[FileInfo], slot: int):
        buf = self._pinned_buf(slot, pack.nbytes)
        pack.host = buf
        view = buf.numpy()
        pack.reads = [pool.submit(self._read_into, infos[i], view[off:off + infos[i].raw_bytes])
                      for i, off in zip(pack.files, pack.byte_off)]

    # -- device stages -----------------------------------------------------
    def _stage(self, pack: _Pack, infos: Sequence[FileInfo]):
        """Wait for the pack's reads, then queue upload, ingestion and selection
        and the copy of row_start back to the host."""
        t0 = time.perf_counter()
        for j, fut in enumerate(pack.reads):
            err = fut.result()
            if err is not None:
                pack.errors[j] = err
        t1 = time.perf_counter()
        self.stats['read_wait_s'] += t1 - t0
        dev, n = self.dev, len(pack.files)
        head = pack.host[:16 * n].view(torch.int64)
        head[:n] = torch.tensor(pack.starts, dtype=torch.int64)
        head[n:] = torch.tensor(pack.slots, dtype=torch.int64)
        self._raw = self._grown(self._raw, pack.nbytes, torch.uint8, dev)
        self._arena = self._grown(self._arena, pack.arena_len, torch.float32, dev)
        raw = self._raw[:pack.nbytes]
        ev = pack.events = [torch.cuda.Event(enable_timing=True) for _ in range(7)]
        ev[0].record()
        raw.copy_(pack.host[:pack.nbytes], non_blocking=True)  # the pack's one upload
        ev[1].record()
        arena = self._arena[:pack.arena_len]
        resampled = [infos[i].frames for i in pack.files if infos[i].sr != self.sr]
        if resampled:
            self._tmp = self._grown(self._tmp, max(max(resampled), 1), torch.float32, dev)
        stream = _lib.stream_handle(dev)
        with torch.cuda.device(dev):
            for j, i in enumerate(pack.files):
                info, start, slot = infos[i], pack.starts[j], pack.slots[j]
                dst = arena.data_ptr() + 4 * start
                if j in pack.errors:  # an unread file is a silent slot; its record is the error
                    arena[start:start + slot].zero_()
                    continue
                src = raw.data_ptr() + pack.byte_off[j]
                fmt = _lib.SAD_PCM_I16 if info.i16 else _lib.SAD_PCM_F32
                if info.sr == self.sr:
                    _lib.call('sad_pcm_mono_run', src, fmt, info.frames, info.channels, dst, slot, stream)
                else:
                    _lib.call('sad_pcm_mono_run', src, fmt, info.frames, info.channels, _lib.ptr(self._tmp),
                              info.frames, stream)
                    plan = _ingest.resampler(info.sr, self.sr, dev)._plan  # one cached plan per rate pair
                    _lib.call('sad_resample_run', plan, _lib.ptr(self._tmp), info.frames, dst, slot, stream)
        ev[2].record()
        dhead = raw[:16 * n].view(torch.int64)
        pack.arena = arena
        pack.offsets, pack.row_start = select_windows_arena(arena, dhead[:n], dhead[n:], self.window, self.hop,
                                                            self.silence_threshold, pack.cap)
        pack.h_row_start = torch.empty(n + 1, dtype=torch.int64, pin_memory=True)
        pack.h_row_start.copy_(pack.row_start, non_blocking=True)
        ev[3].record()
        self.stats['stage_s'] += time.perf_counter() - t1
        self.stats['candidates'] += pack.cap

    def _infer(self, pack: _Pack):
        """The kept count is on the host now: queue the batches, the
        post-processing and the copy of the results."""
        t0 = time.perf_counter()
        eng, dev = self.eng, self.dev
        n_kept = pack.n_kept = int(pack.h_row_start[-1])
        C = eng.n_heads + 1
        logits = torch.empty(n_kept, C, dtype=torch.float32, device=dev)
        bs = self.batch_size
        pack.events[4].record()
        if n_kept:
            maps = torch.empty(min(bs, n_kept), eng.frontend.n_mels, eng.frontend.n_frames, dtype=torch.float32,
                               device=dev)
            per_head = torch.empty(min(bs, n_kept), eng.n_heads, 2, dtype=torch.float32, device=dev)
        for s in range(0, n_kept, bs):
            e = min(s + bs, n_kept)
            m = eng.frontend.windows(pack.arena, pack.offsets[s:e], out=maps[:e - s])
            eng.heads(eng.features(m), logits=per_head[:e - s], merged=logits[s:e])
        pack.events[5].record()
        _, label, mean = postprocess(logits, pack.row_start, self.threshold, self.smooth)
        pack.h_offsets = torch.empty(n_kept, dtype=torch.int64, pin_memory=True)
        pack.h_label = torch.empty(n_kept, dtype=torch.int32, pin_memory=True)
        pack.h_mean = torch.empty(len(pack.files), C, dtype=torch.float64, pin_memory=True)
        pack.h_offsets.copy_(pack.offsets[:n_kept], non_blocking=True)
        pack.h_label.copy_(label, non_blocking=True)
        pack.h_mean.copy_(mean, non_blocking=True)
        if self.keep_logits:
            pack.h_logits = torch.empty(n_kept, C, dtype=torch.float32, pin_memory=True)
            pack.h_logits.copy_(logits, non_blocking=True)
        pack.events[6].record()
        self.stats['infer_enqueue_s'] += time.perf_counter() - t0
        self.stats['segments'] += n_kept

    def _finish(self, pack: _Pack, infos: Sequence[FileInfo]) -> List[dict]:
        t0 = time.perf_counter()
        names = [infos[i].path for i in pack.files]
        rs = pack.h_row_start.numpy()
        recs = assemble_records(names, pack.starts, rs, pack.h_offsets.numpy(), pack.h_label.numpy(),
                                pack.h_mean.numpy(), self.synthetic_names, self.real_name, self.sr,
                                self.window_size, pack.errors)
        if self.keep_logits:
            for j, name in enumerate(names):
                self.logits[name] = pack.h_logits[int(rs[j]):int(rs[j + 1])].clone()
        ev = pack.events
        for key, a, b in (('dev_upload_s', 0, 1), ('dev_ingest_s', 1, 2), ('dev_select_s', 2, 3),
                          ('dev_engine_s', 4, 5), ('dev_post_s', 5, 6)):
            self.stats[key] += ev[a].elapsed_time(ev[b]) / 1e3
        self.stats['records_s'] += time.perf_counter() - t0
        return recs

    def _sync(self):
        t0 = time.perf_counter()
        torch.cuda.current_stream(self.dev).synchronize()
        self.stats['sync_wait_s'] += time.perf_counter() - t0
        self.stats['syncs'] += 1

    def scan(self, paths: Sequence[str]) -> List[dict]:
        paths = [os.fspath(p) for p in paths]
        records: List[Optional[dict]] = [None] * len(paths)
        with ThreadPoolExecutor(max_workers=self.workers) as pool:
            t0 = time.perf_counter()
            infos = list(pool.map(wav_info, paths))
            self.stats['header_s'] += time.perf_counter() - t0
            good = [i for i, inf in enumerate(infos) if inf.error is None]
            for i, inf in enumerate(infos):
                if inf.error is not None:
                    records[i] = {'filename': inf.path, 'error': inf.error}
            groups = plan_packs([slot_len(infos[i], self.sr, self.window) for i in good], self.pack_samples)
            packs = [_Pack([good[j] for j in g], infos, self.sr, self.window, self.hop) for g in groups]
            if packs:
                self._submit(pool, packs[0], infos, 0)
            prev = None
            for k, pack in enumerate(packs):
                if k + 1 < len(packs):  # the next pack's reads overlap this pack's device work
                    self._submit(pool, packs[k + 1], infos, (k + 1) % 2)
                self._stage(pack, infos)
                self._sync()  # the pack's one wait: the previous results and this pack's kept count
                if prev is not None:
                    for i, rec in zip(prev.files, self._finish(prev, infos)):
                        records[i] = rec
                self._infer(pack)
                prev = pack
            if prev is not None:
                self._sync()
                for i, rec in zip(prev.files, self._finish(prev, infos)):
                    records[i] = rec
        self.stats['files'] += len(paths)
        self.stats['packs'] += len(packs)
        return records
