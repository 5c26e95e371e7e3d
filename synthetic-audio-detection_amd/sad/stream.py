"""Live streams: chunk-by-chunk detection for many concurrent feeds.

``inference_runner.py`` and ``catalog_runner.py`` need the whole recording.
Here feeds deliver a few tens of milliseconds at a time, each in its own sample
rate and channel count, and every 4 s window gets its label as soon as its last
sample exists.  For any way of cutting a recording into chunks the stream gives
bit for bit what the whole-file path gives: the 32 kHz samples, the kept
windows, the timestamps, the merged logits and the final record.

  emission rule   pure host arithmetic (below): which 32 kHz samples a feed has
                  after F frames, and which windows are complete
  StreamIngest    the device bank (csrc/stream.hip, include/sad.h "streaming"):
                  per slot a mirrored ring of 32 kHz samples and the
                  resampler's carry; one upload and one launch per push
  StreamBank      StreamIngest + silence test (sad_scan_select_run over the
                  bank's arena) + front end + ensemble; one wait per push

Everything up to ``StreamIngest`` is numpy on the host and never loads libsad.
"""
from __future__ import annotations

import ctypes
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from . import ingest as _ingest
from .ingest import resample_geometry

STREAM_COLS = 10        # SB_COLS: push table columns (include/sad.h "streaming")
STREAM_CARRY = 8192     # SB_CARRY: floats per carry buffer
STREAM_MIN_ROOM = 4096  # SB_MIN_ROOM: CAP - window is at least this
STREAM_TILE = _ingest.TRAIN_TILE
STREAM_MAX_RATES = _ingest.TRAIN_MAX_RATES


# ------------------------------------------------------------------ emission rule
def frames_done(F: int, sr: int, target_sr: int = 32000) -> int:
    """J(F): the polyphase frames whose taps are all present after F input frames."""
    orig, _, width, _ = resample_geometry(sr, target_sr)
    return (F - width) // orig if F >= width else 0


def first_sample(start_frame: int, sr: int, target_sr: int = 32000) -> int:
    """g0: the first 32 kHz sample of a feed whose clock starts at start_frame."""
    orig, new, _, _ = resample_geometry(sr, target_sr)
    return start_frame // orig * new


def ready(F: int, sr: int, target_sr: int = 32000, start_frame: int = 0) -> int:
    """The 32 kHz samples emitted once the feed has F frames (absolute count,
    start_frame included): J(F) new, F at the feed's own rate; never below g0."""
    if int(sr) == int(target_sr):
        return int(F)
    orig, new, _, _ = resample_geometry(sr, target_sr)
    return max(frames_done(F, sr, target_sr), start_frame // orig) * new


def final_end(T: int, sr: int, window: int, target_sr: int = 32000, start_frame: int = 0) -> Tuple[int, int]:
    """End of a feed with T frames: (n_out, end).  Samples up to n_out =
    ceil(new T / orig) are the resampler's; zeros follow up to end = max(n_out,
    g0 + window), preprocess_waveform's pad."""
    n_out = _ingest.train_out_len(T, sr, target_sr)
    return n_out, max(n_out, first_sample(start_frame, sr, target_sr) + int(window))


def window_count(emitted: int, window: int, hop: int, first: int = 0) -> int:
    """Window starts first, first + hop, ... whose last sample is emitted."""
    return (emitted - window - first) // hop + 1 if emitted - window >= first else 0


def bank_cap(window: int, max_chunk_frames: int) -> int:
    """sad_stream_bank_size's CAP: window + max(4 max_chunk_frames, 4096), rounded up to 4."""
    return -(-(int(window) + max(4 * int(max_chunk_frames), STREAM_MIN_ROOM)) // 4) * 4


def rate_supported(sr: int, cap: int, window: int, target_sr: int = 32000) -> bool:
    """sad_stream_open_check's rate rules."""
    if sr <= 0:
        return False
    if int(sr) == int(target_sr):
        return True
    orig, new, width, K = resample_geometry(sr, target_sr)
    if K > STREAM_CARRY or not _ingest.train_rate_supported(sr, target_sr):
        return False
    return new * (2 + (width + orig - 1) // orig) <= cap - window


def piece_frames(sr: int, cap: int, window: int, max_chunk_frames: int, target_sr: int = 32000) -> int:
    """The most frames one launch takes from a feed: what it adds, at most
    (n // orig + 1) new samples, must fit CAP - window."""
    if int(sr) == int(target_sr):
        return min(int(max_chunk_frames), cap - window)
    orig, new, _, _ = resample_geometry(sr, target_sr)
    return min(int(max_chunk_frames), ((cap - window) // new - 1) * orig)


def _spans(geom, native: bool, start, fb, n, final, window: int):
    """sb_row (csrc/stream.hip) on int64 arrays -> (mA, mE): the global samples a row stores."""
    orig, new, width, _ = geom
    start, fb, n = (np.asarray(v, dtype=np.int64) for v in (start, fb, n))
    final = np.asarray(final, dtype=bool)
    F1 = fb + n
    if native:
        return fb.copy(), np.where(final, np.maximum(F1, start + window), F1)
    J0 = start // orig
    Ja = np.maximum(np.where(fb >= width, (fb - width) // orig, 0), J0)
    Jb = np.maximum(np.where(F1 >= width, (F1 - width) // orig, 0), J0)
    n_out = (new * F1 + orig - 1) // orig
    return Ja * new, np.where(final, np.maximum(n_out, J0 * new + window), Jb * new)


def _tiles(geom, native: bool, mA, mE, final):
    """sb_out_tiles + sb_carry_tiles on arrays."""
    _, new, _, K = geom
    A = mE - mA
    if native:
        return -(-A // STREAM_TILE)
    carry = np.where(np.asarray(final, dtype=bool), 0, -(-K // STREAM_TILE))
    if new < 64:
        return -(-A // STREAM_TILE) + carry
    return -(-(-(-A // new)) // _ingest.TRAIN_WIDE_FRAMES) * (-(-new // 64)) + carry


def push_span(sr: int, start_frame: int, frames_before: int, n_frames: int, final: bool, window: int,
              target_sr: int = 32000) -> Tuple[int, int]:
    """The global 32 kHz samples [first, end) one push stores (sad_stream_push_tiles)."""
    a, e = _spans(resample_geometry(sr, target_sr), int(sr) == int(target_sr), start_frame, frames_before, n_frames,
                  final, window)
    return int(a), int(e)


def push_tiles(sr: int, start_frame: int, frames_before: int, n_frames: int, final: bool, window: int,
               target_sr: int = 32000) -> int:
    """sad_stream_push_tiles: the workgroups of one table row."""
    g, native = resample_geometry(sr, target_sr), int(sr) == int(target_sr)
    a, e = _spans(g, native, start_frame, frames_before, n_frames, final, window)
    return int(_tiles(g, native, a, e, final))


# ------------------------------------------------------------------------ packing
def _align(n: int, a: int = 16) -> int:
    return -(-n // a) * a


class PushRow:
    """One slot's part of a launch: its chunk as stored (interleaved int16 /
    fp32, whole frames) and the host's counters for it."""
    __slots__ = ('slot', 'samples', 'frames', 'frames_before', 'final', 'sr', 'channels', 'start_frame', 'parity')

    def __init__(self, slot, samples, frames_before, final, sr, channels, start_frame=0, parity=0):
        assert samples.dtype in (np.int16, np.float32) and samples.ndim == 1
        assert samples.shape[0] % channels == 0
        self.slot, self.samples, self.frames = int(slot), samples, samples.shape[0] // int(channels)
        self.frames_before, self.final, self.sr, self.channels = int(frames_before), bool(final), int(sr), int(channels)
        self.start_frame, self.parity = int(start_frame), int(parity)


class PushPack:
    """A launch, ready for one upload.  `arena` (uint8) holds the chunks, each
    at a multiple of 16 bytes, then the table [n_rows, 10] int64 and the tile
    table [n_tiles, 2] int32; `rates[i]` is the sample rate behind rate index
    i; `spans` [n_rows, 2] the global samples each row stores."""

    def __init__(self, arena, n_rows, n_tiles, table_off, tiles_off, nbytes, rates, spans):
        self.arena, self.n_rows, self.n_tiles = arena, int(n_rows), int(n_tiles)
        self.table_off, self.tiles_off, self.nbytes = int(table_off), int(tiles_off), int(nbytes)
        self.rates, self.spans = tuple(rates), spans

    @property
    def table(self) -> np.ndarray:
        return self.arena[self.table_off:self.table_off + 8 * STREAM_COLS * self.n_rows].view(np.int64).reshape(
            self.n_rows, STREAM_COLS)

    @property
    def tiles(self) -> np.ndarray:
        return self.arena[self.tiles_off:self.tiles_off + 8 * self.n_tiles].view(np.int32).reshape(self.n_tiles, 2)


def pack_push(rows: Sequence[PushRow], window: int, target_sr: int = 32000, alloc=None) -> PushPack:
    """Rows of at most 8 distinct rates -> one PushPack.  `alloc(nbytes)`
    returns the uint8 numpy buffer to fill (a pinned one); default: a new array."""
    rates: List[int] = []
    for r in rows:
        if r.sr not in rates:
            rates.append(r.sr)
    if len(rates) > STREAM_MAX_RATES:
        raise ValueError(f'{len(rates)} distinct sample rates in one launch (at most {STREAM_MAX_RATES})')
    n = len(rows)
    table = np.zeros((n, STREAM_COLS), np.int64)
    table[:, 0] = [r.slot for r in rows]
    table[:, 2] = [r.frames for r in rows]
    table[:, 3] = [r.frames_before for r in rows]
    table[:, 4] = [r.final for r in rows]
    table[:, 5] = [rates.index(r.sr) for r in rows]
    table[:, 6] = [r.channels for r in rows]
    table[:, 7] = [_lib.SAD_PCM_I16 if r.samples.dtype == np.int16 else _lib.SAD_PCM_F32 for r in rows]
    table[:, 8] = [r.start_frame for r in rows]
    table[:, 9] = [r.parity for r in rows]
    nbytes = np.array([r.samples.nbytes for r in rows], np.int64)
    ends = np.cumsum(-(-nbytes // 16) * 16)
    table[:, 1] = ends - (-(-nbytes // 16) * 16)
    spans = np.zeros((n, 2), np.int64)
    ntile = np.zeros(n, np.int64)
    for i, sr in enumerate(rates):
        sel = table[:, 5] == i
        g, native = resample_geometry(sr, target_sr), sr == int(target_sr)
        a, e = _spans(g, native, table[sel, 8], table[sel, 3], table[sel, 2], table[sel, 4], window)
        spans[sel, 0], spans[sel, 1] = a, e
        ntile[sel] = _tiles(g, native, a, e, table[sel, 4])
    total = int(ntile.sum())
    tiles = np.empty((total, 2), np.int32)
    tiles[:, 0] = np.repeat(np.arange(n, dtype=np.int32), ntile)
    first = np.cumsum(ntile) - ntile
    tiles[:, 1] = np.arange(total, dtype=np.int64) - np.repeat(first, ntile)
    table_off = int(ends[-1]) if n else 0
    tiles_off = _align(table_off + table.nbytes)
    size = _align(tiles_off + tiles.nbytes)
    buf = alloc(size) if alloc is not None else np.zeros(size, np.uint8)
    for off, r in zip(table[:, 1], rows):
        if r.samples.nbytes:
            buf[off:off + r.samples.nbytes] = r.samples.view(np.uint8)
    buf[table_off:table_off + table.nbytes] = table.reshape(-1).view(np.uint8)
    buf[tiles_off:tiles_off + tiles.nbytes] = tiles.reshape(-1).view(np.uint8)
    return PushPack(buf, n, total, table_off, tiles_off, size, rates, spans)


# ------------------------------------------------------------------- device bank
class _Slot:
    __slots__ = ('name', 'sr', 'channels', 'dtype', 'start_frame', 'frames', 'parity', 'g0', 'emitted', 'next_start',
                 'closed', 'logits', 'times')

    def __init__(self, name, sr, channels, dtype, start_frame, g0):
        self.name, self.sr, self.channels, self.dtype = name, int(sr), int(channels), np.dtype(dtype)
        self.start_frame, self.frames, self.parity = int(start_frame), int(start_frame), 0
        self.g0 = self.emitted = self.next_start = int(g0)
        self.closed = False
        self.logits: List[torch.Tensor] = []
        self.times: List[float] = []


class StreamIngest:
    """The device bank: `slots` mirrored rings of `cap` 32 kHz samples and the
    resampler carries, fed by sad_stream_push_run.  `ingest` queues the upload
    and the launches of one push on the current stream and returns; it never
    waits for the device."""
    N_PINNED = 4  # upload buffers in rotation, each guarded by an event

    def __init__(self, slots: int, window: int, hop: int, max_chunk_frames: int, device='cuda',
                 target_sr: int = 32000):
        self.device = _ingest._dev(device)
        self.n_slots, self.window, self.hop = int(slots), int(window), int(hop)
        self.max_chunk_frames, self.target_sr = int(max_chunk_frames), int(target_sr)
        cap, alen, clen = _lib.I64(), _lib.I64(), _lib.I64()
        _lib.call('sad_stream_bank_size', self.n_slots, self.window, self.hop, self.max_chunk_frames, self.target_sr,
                  ctypes.byref(cap), ctypes.byref(alen), ctypes.byref(clen))
        self.cap = cap.value
        assert self.cap == bank_cap(self.window, self.max_chunk_frames)
        self.arena = torch.empty(alen.value, dtype=torch.float32, device=self.device)
        self.carry = torch.empty(clen.value, dtype=torch.float32, device=self.device)
        self.slots: List[Optional[_Slot]] = [None] * self.n_slots
        self._pinned = [None] * self.N_PINNED
        self._pin_event = [None] * self.N_PINNED
        self._pin_next = 0
        self._dbuf = None
        self.stats = {'uploads': 0, 'launches': 0, 'upload_bytes': 0}

    # -- slots ---------------------------------------------------------------
    def open(self, name: str, sample_rate: int, channels: int, dtype, start_frame: int = 0) -> int:
        dt = np.dtype(dtype)
        if dt not in (np.dtype(np.int16), np.dtype(np.float32)):
            raise ValueError(f'dtype must be int16 or float32 (got {dt})')
        g0 = _lib.I64()
        _lib.call('sad_stream_open_check', int(sample_rate), self.target_sr, int(channels), self.window, self.hop,
                  self.cap, int(start_frame), ctypes.byref(g0))
        for s, st in enumerate(self.slots):
            if st is None:
                self.slots[s] = _Slot(name, sample_rate, channels, dt, start_frame, g0.value)
                return s
        raise RuntimeError(f'all {self.n_slots} slots of the bank are open')

    def release(self, slot: int):
        self.slots[slot] = None

    def state(self, slot: int) -> _Slot:
        st = self.slots[slot]
        if st is None:
            raise KeyError(f'slot {slot} is not open')
        return st

    # -- uploads -------------------------------------------------------------
    def _alloc(self, nbytes: int) -> np.ndarray:
        k = self._pin_next
        self._pin_next = (k + 1) % self.N_PINNED
        if self._pin_event[k] is not None:
            self._pin_event[k].synchronize()  # the copy out of this buffer, N_PINNED uploads ago
        if self._pinned[k] is None or self._pinned[k].numel() < nbytes:
            self._pinned[k] = torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True)
        self._pin_k = k
        return self._pinned[k].numpy()[:nbytes]

    def _launch(self, rows: List[PushRow]):
        pack = pack_push(rows, self.window, self.target_sr, self._alloc)
        dev, k = self.device, self._pin_k
        if self._dbuf is None or self._dbuf.numel() < pack.nbytes:
            self._dbuf = torch.empty(max(pack.nbytes, 4096), dtype=torch.uint8, device=dev)
        d = self._dbuf[:pack.nbytes]
        d.copy_(self._pinned[k][:pack.nbytes], non_blocking=True)  # the launch's one upload
        ev = self._pin_event[k] = self._pin_event[k] or torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        plans = (ctypes.c_void_p * len(pack.rates))(*[
            None if sr == self.target_sr else _ingest.resampler(sr, self.target_sr, dev)._plan for sr in pack.rates])
        base = d.data_ptr()
        with torch.cuda.device(dev):
            _lib.call('sad_stream_push_run', base, pack.table_off, pack.table.ctypes.data, base + pack.table_off,
                      pack.n_rows, base + pack.tiles_off, pack.n_tiles, plans, len(pack.rates), _lib.ptr(self.arena),
                      _lib.ptr(self.carry), self.n_slots, self.cap, self.window, _lib.stream_handle(dev))
        self.stats['uploads'] += 1
        self.stats['launches'] += 1
        self.stats['upload_bytes'] += pack.nbytes
        for r, (a, e) in zip(rows, pack.spans):
            st = self.slots[r.slot]
            assert int(a) == st.emitted or int(e) == int(a), (r.slot, int(a), st.emitted)
            st.frames += r.frames
            st.parity ^= 1
            st.emitted = max(st.emitted, int(e))
            if r.final:
                st.closed = True

    def rounds(self, chunks: Dict[int, np.ndarray], final: Sequence[int] = ()):
        """One push as a generator: `chunks[slot]` are interleaved samples
        (whole frames, any length >= 0) in the slot's dtype; slots in `final`
        end after their chunk.  Each step queues ONE upload and launch and
        yields the slots it named.  A chunk longer than one launch takes is
        split over several launches, as is a push with more than 8 distinct
        rates.  A launch adds at most CAP - window samples to a ring, and a ring
        holds CAP: whoever reads windows in place must examine the newly
        complete ones after every step, before the next one overwrites them."""
        final = set(int(s) for s in final)
        pending = []
        for slot in list(chunks) + [s for s in final if s not in chunks]:
            st = self.state(slot)
            if st.closed:
                raise RuntimeError(f'slot {slot} ({st.name!r}) has ended')
            if slot not in chunks:
                continue  # ends without a last chunk: the final flush alone
            x = np.ascontiguousarray(chunks[slot]).reshape(-1)
            if x.dtype != st.dtype:
                raise TypeError(f'slot {slot} was opened as {st.dtype}, the chunk is {x.dtype}')
            if x.shape[0] % st.channels:
                raise ValueError(f'slot {slot}: {x.shape[0]} samples are not whole frames of {st.channels} channels')
            piece = piece_frames(st.sr, self.cap, self.window, self.max_chunk_frames, self.target_sr) * st.channels
            pending.append([slot, x, 0, piece])
        fin_left = set(final)
        while pending or fin_left:
            rows, rates, later = [], [], []
            for item in pending:
                slot, x, pos, piece = item
                st = self.slots[slot]
                if st.sr not in rates:
                    if len(rates) == STREAM_MAX_RATES:
                        later.append(item)
                        continue
                    rates.append(st.sr)
                part = x[pos:pos + piece]
                rows.append(PushRow(slot, part, st.frames, False, st.sr, st.channels, st.start_frame, st.parity))
                item[2] = pos + piece
                if item[2] < x.shape[0]:
                    later.append(item)
            if not rows:  # the chunks are in: the final flushes, each a row of its own without frames
                for slot in sorted(fin_left):
                    st = self.slots[slot]
                    if st.sr not in rates:
                        if len(rates) == STREAM_MAX_RATES:
                            continue
                        rates.append(st.sr)
                    rows.append(PushRow(slot, np.zeros(0, st.dtype), st.frames, True, st.sr, st.channels,
                                        st.start_frame, st.parity))
                fin_left -= {r.slot for r in rows}
            pending = later
            self._launch(rows)
            yield [r.slot for r in rows]

    def ingest(self, chunks: Dict[int, np.ndarray], final: Sequence[int] = ()) -> None:
        """Queue one push (every step of `rounds`) and return; nothing reads the rings in between."""
        for _ in self.rounds(chunks, final):
            pass

    def read(self, slot: int, first: int, count: int) -> torch.Tensor:
        """Debug accessor: the slot's samples [first, first + count) by global
        index (a copy; count <= CAP, and only what the ring still holds is meaningful)."""
        assert 0 <= count <= self.cap and first >= 0
        o = slot * 2 * self.cap + first % self.cap
        return self.arena[o:o + count].clone()

    def ring_offset(self, slot: int, g: int) -> int:
        """Arena offset at which the slot's samples from global index g on are contiguous."""
        return slot * 2 * self.cap + g % self.cap


class _PinnedPool:
    """Pinned host buffers handed out in consecutive regions between two device
    waits, then reused: a region is never rewritten while a copy may read it."""

    def __init__(self):
        self.buf, self.used, self.retired = {}, {}, []

    def take(self, n: int, dtype) -> torch.Tensor:
        b, u = self.buf.get(dtype), self.used.get(dtype, 0)
        if b is None or u + n > b.numel():
            if b is not None:
                self.retired.append(b)  # copies queued from it finish before it goes
            b = self.buf[dtype] = torch.empty(max(2 * (u + n), 1024), dtype=dtype, pin_memory=True)
            u = 0
        self.used[dtype] = u + n
        return b[u:u + n]

    def reset(self):
        """After a device wait: every region is free again."""
        self.used, self.retired = {}, []


class StreamBank:
    """Many live feeds through one engine.

    ``open`` reserves a slot, ``push`` takes one chunk per slot and returns the
    events of the windows that became complete, ``close`` ends a feed and
    returns the record ``inference_runner.py`` writes for the same samples as a
    file.  ``audio_cfg`` / ``spec_cfg`` are inference_runner's AudioConfig /
    SpectrogramConfig.  A slot keeps its feed's merged logits and timestamps on
    the host until ``close`` (7 floats per window): the record needs them all."""

    def __init__(self, engine, class_names: Sequence[str], slots: int, audio_cfg, spec_cfg, max_chunk_frames: int,
                 threshold: float = 0.5, batch_size: int = 128):
        import inference_runner as ir
        self._ir = ir
        self.eng, self.dev = engine, engine.device
        self.synthetic_names, self.real_name = list(class_names[:-1]), class_names[-1]
        self.threshold, self.batch_size = float(threshold), max(1, int(batch_size))
        self.sr, self.window_size = int(audio_cfg.sample_rate), float(audio_cfg.window_size)
        self.window = int(audio_cfg.window_size * audio_cfg.sample_rate)
        self.hop = int((1 - audio_cfg.overlap) * self.window)
        if self.hop <= 0:
            raise ValueError(f'hop of {self.hop} samples (overlap={audio_cfg.overlap})')
        self.silence_threshold = float(audio_cfg.silence_threshold)
        self.fe = ir._frontend(self.dev, spec_cfg, self.window, self.sr)
        self.bank = StreamIngest(slots, self.window, self.hop, max_chunk_frames, self.dev, self.sr)
        self.stats = {'pushes': 0, 'uploads': 0, 'launches': 0, 'waits': 0, 'windows': 0, 'skipped': 0}
        self._pin = _PinnedPool()
        self.last_events: List[dict] = []

    def open(self, name: str, sample_rate: int, channels: int, dtype, start_frame: int = 0) -> int:
        return self.bank.open(name, sample_rate, channels, dtype, start_frame)

    # -- one push ------------------------------------------------------------
    def _candidates(self, slots):
        """The emission rule on the host: each slot's newly complete windows
        -> (slot, first start, count), and the slot's next unexamined start."""
        out = []
        for s in slots:
            st = self.bank.slots[s]
            assert st.emitted - st.next_start <= self.bank.cap  # the ring still holds every unexamined sample
            c = window_count(st.emitted, self.window, self.hop, st.next_start)
            if c > 0:
                out.append((s, st.next_start, c))
                st.next_start += c * self.hop
        return out

    def _examine(self, touched):
        """Queue, for the slots one launch named, the silence test, the front
        end and the ensemble over their newly complete windows, and the copy of
        the results to pinned memory -> (cands, host tensors) or None."""
        bank, dev, pin = self.bank, self.dev, self._pin
        cands = self._candidates(touched)
        total = sum(c for _, _, c in cands)
        if not total:
            return None
        n = len(cands)
        head = pin.take(2 * n, torch.int64)
        hv = head.numpy()
        hv[:n] = [bank.ring_offset(s, w) for s, w, _ in cands]
        hv[n:] = [self.window + (c - 1) * self.hop for _, _, c in cands]
        dhead = head.to(dev, non_blocking=True)
        from .scan import select_windows_arena
        offsets = torch.zeros(total, dtype=torch.int64, device=dev)
        offsets, row_start = select_windows_arena(bank.arena, dhead[:n], dhead[n:], self.window, self.hop,
                                                  self.silence_threshold, total, offsets=offsets)
        C = self.eng.n_heads + 1
        logits = torch.empty(total, C, dtype=torch.float32, device=dev)
        # the kept count stays on the device: every candidate row is inferred (a skipped
        # window's row reads offset 0 and is dropped afterwards), so the push waits once
        for s in range(0, total, self.batch_size):
            e = min(s + self.batch_size, total)
            logits[s:e] = self.eng.forward_maps(self.fe.windows(bank.arena, offsets[s:e]))[1]
        host = (pin.take(total, torch.int64), pin.take(n + 1, torch.int64),
                pin.take(total * C, torch.float32).view(total, C))
        for h, d in zip(host, (offsets, row_start, logits)):
            h.copy_(d, non_blocking=True)
        return cands, host

    def _run(self, chunks, final) -> List[dict]:
        bank, dev = self.bank, self.dev
        before = dict(bank.stats)
        queued = []
        # a long chunk is several launches: the windows each one completes are examined
        # (queued on the stream) before the next launch may overwrite their samples
        for touched in bank.rounds(chunks, final):
            q = self._examine(touched)
            if q is not None:
                queued.append(q)
        torch.cuda.current_stream(dev).synchronize()  # the push's one wait
        self.stats['pushes'] += 1
        self.stats['waits'] += 1
        self.stats['uploads'] += bank.stats['uploads'] - before['uploads']
        self.stats['launches'] += bank.stats['launches'] - before['launches']
        events = []
        for cands, (h_off, h_rows, h_logits) in queued:
            h_off, h_rows = h_off.numpy(), h_rows.numpy()
            rows = h_logits.clone()  # out of the pinned buffer, which the next push reuses
            for f, (s, w, c) in enumerate(cands):
                st = bank.slots[s]
                base = bank.ring_offset(s, w) - w
                lo, hi = int(h_rows[f]), int(h_rows[f + 1])
                self.stats['windows'] += hi - lo
                self.stats['skipped'] += c - (hi - lo)
                for r in range(lo, hi):
                    row = rows[r]
                    t = (int(h_off[r]) - base) / self.sr
                    label, probs = self._ir.interpret_multihead_logits(row, threshold=self.threshold,
                                                                       synthetic_names=self.synthetic_names,
                                                                       real_name=self.real_name)
                    st.logits.append(row)
                    st.times.append(t)
                    events.append({'slot': s, 'name': st.name, 'start_sec': t, 'end_sec': t + self.window_size,
                                   'label': label, 'probs': probs, 'logits': row})
        self._pin.reset()
        return events

    def push(self, chunks: Dict[int, np.ndarray]) -> List[dict]:
        """One chunk per slot (interleaved np.int16 / np.float32, whole frames,
        any length >= 0) -> one event per kept window that became complete:
        slot, name, start_sec, end_sec, label, probs (sigmoid) and logits (merged).
        A chunk longer than `max_chunk_frames` costs several uploads and
        launches, with the windows examined in between, and still one wait."""
        return self._run(dict(chunks), ())

    def close(self, slot: int, smooth: bool = False) -> dict:
        """End of feed: the record of inference_runner.summarize over all of
        the feed's windows (``--smooth`` included).  The events of the windows
        the flush completed (the padded window of a short clip among them) are
        left in ``self.last_events``: read them before the next ``close``."""
        self.last_events = self._run({}, (slot,))
        st = self.bank.state(slot)
        self.bank.release(slot)
        if not st.logits:
            return {'filename': st.name, 'segments': [], 'percentages': {}}
        return self._ir.summarize(st.name, torch.stack(st.logits), st.times, self.threshold, self.synthetic_names,
                                  self.real_name, smooth, self.window_size)
