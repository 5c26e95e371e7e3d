"""Device-side ingestion of long audio files.

The reference's ``preprocess_waveform`` + ``slice_waveform`` + per-window
``waveform_to_spectrogram`` (inference_runner.py:144-190, 276-289) turn one WAV
into a list of 4 s host tensors.  Here the file's samples go to HBM once, as
stored (int16, or host-decoded fp32 for other encodings), and the rest runs on
libsad (csrc/ingest.hip, include/sad.h "ingestion"):

  load_waveform   interleaved PCM -> mono fp32 -> (resample to 32 kHz) -> pad
  select_windows  window starts at the reference's hop; the silence test on the
                  device (max |x| per window); the host sees one float per window
  Windows         the kept windows' start offsets on the device, read in place
                  by the front end (sad_frontend_run_windows)

The host work left is the WAV header parse and the keep/skip decision over the
per-window maxima (the same fp32 comparison as ``piece.abs().max() < thr``).

The trainer's batched twin is at the end of the module ("trainer ingestion"):
stored samples of a whole batch -> the [2B, seg_len] training segments in one
upload and one launch (``TrainIngest``, ``collate_stored``).  With waveform
augmentation rows (``submodel_trainer.py --wave-augment``) the same upload also
carries one augmentation row per file, and a stage in front of that launch
(``sad_wave_augment_run``, csrc/waveaug.hip) writes an augmented fp32 mono arena
that the unchanged launch then reads.  Files that drew a time-stretch or
pitch-shift kind (``--wave-stretch``) go through ``sad_wave_stretch_run``
(csrc/stretch.hip) into the same arena.
"""
from __future__ import annotations

import ctypes
import math
from typing import List, Tuple

import numpy as np
import torch

from . import _lib
from . import audio as _audio
from . import augment as _augment


def _dev(device) -> torch.device:
    d = torch.device(device)
    if d.type != 'cuda':
        raise RuntimeError(f'libsad runs on an MI355X only (device={device!r}); there is no CPU path')
    return d if d.index is not None else torch.device('cuda', torch.cuda.current_device())


class Resampler:
    """torchaudio.transforms.Resample(orig_freq, new_freq) (sinc_interp_hann,
    width 6, rolloff 0.99) on the device: inference_runner.py:148."""

    def __init__(self, orig_freq: int, new_freq: int, device='cuda'):
        self.device = _dev(device)
        self.orig_freq, self.new_freq = int(orig_freq), int(new_freq)
        self._plan = _lib.P()
        with torch.cuda.device(self.device):
            _lib.call('sad_resample_plan_create', self.orig_freq, self.new_freq, ctypes.byref(self._plan))

    def out_len(self, n_in: int) -> int:
        n = _lib.I64()
        _lib.call('sad_resample_out_len', self._plan, int(n_in), ctypes.byref(n))
        return n.value

    def __call__(self, x: torch.Tensor, min_len: int = 0) -> torch.Tensor:
        """x [T] fp32 on the device -> [max(ceil(new*T/orig), min_len)] (zero tail)."""
        assert x.dtype == torch.float32 and x.dim() == 1 and x.is_contiguous() and x.device == self.device
        n_out = self.out_len(x.shape[0])
        y = torch.empty(max(n_out, int(min_len)), device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            _lib.call('sad_resample_run', self._plan, _lib.ptr(x), x.shape[0], _lib.ptr(y), y.shape[0],
                      _lib.stream_handle(self.device))
        return y

    def __del__(self):
        try:
            if getattr(self, '_plan', None):
                _lib.load().sad_resample_plan_destroy(self._plan)
        except Exception:
            pass


_RESAMPLERS = {}


def resampler(orig_freq: int, new_freq: int, device='cuda') -> Resampler:
    d = _dev(device)
    key = (int(orig_freq), int(new_freq), str(d))
    if key not in _RESAMPLERS:
        _RESAMPLERS[key] = Resampler(orig_freq, new_freq, d)
    return _RESAMPLERS[key]


def mono(pcm: torch.Tensor, channels: int, out_len: int = 0) -> torch.Tensor:
    """Interleaved [frames * channels] int16 / fp32 on the device -> mono fp32
    [max(frames, out_len)]: torchaudio.load scaling + waveform.mean(dim=0) + zero pad."""
    assert pcm.dim() == 1 and pcm.is_contiguous() and pcm.dtype in (torch.int16, torch.float32)
    frames = pcm.shape[0] // channels
    dev = pcm.device
    out = torch.empty(max(frames, int(out_len)), device=dev, dtype=torch.float32)
    fmt = _lib.SAD_PCM_I16 if pcm.dtype == torch.int16 else _lib.SAD_PCM_F32
    with torch.cuda.device(dev):
        _lib.call('sad_pcm_mono_run', _lib.ptr(pcm), fmt, frames, int(channels), _lib.ptr(out), out.shape[0],
                  _lib.stream_handle(dev))
    return out


def waveform_from_samples(samples: np.ndarray, channels: int, sr: int, target_sr: int = 32000,
                          min_len: int = 0, device='cuda') -> Tuple[torch.Tensor, int]:
    """preprocess_waveform (inference_runner.py:144-155) from decoded WAV
    samples: upload as stored, mono, resample when sr != target_sr, zero-pad
    to min_len samples (the window) -> (fp32 [T] on the device, target_sr)."""
    dev = _dev(device)
    if samples.dtype not in (np.int16, np.float32):
        samples = samples.astype(np.float32)
    pcm = torch.from_numpy(np.ascontiguousarray(samples.reshape(-1))).to(dev)
    if int(sr) == int(target_sr):
        return mono(pcm, channels, min_len), int(sr)
    wf = mono(pcm, channels)
    return resampler(sr, target_sr, dev)(wf, min_len), int(target_sr)


def load_waveform(path: str, target_sr: int = 32000, min_len: int = 0, device='cuda') -> Tuple[torch.Tensor, int]:
    """WAV file -> (mono fp32 [T] at target_sr on the device, target_sr)."""
    samples, ch, sr = _audio.read_wav(path)
    return waveform_from_samples(samples, ch, sr, target_sr, min_len, device)


def window_absmax(wf: torch.Tensor, window: int, hop: int, n_windows: int) -> torch.Tensor:
    """max |wf[w*hop : w*hop + window]| for w < n_windows (device fp32 [n_windows])."""
    assert wf.dtype == torch.float32 and wf.dim() == 1 and wf.is_contiguous()
    out = torch.empty(max(int(n_windows), 0), device=wf.device, dtype=torch.float32)
    with torch.cuda.device(wf.device):
        _lib.call('sad_window_absmax_run', _lib.ptr(wf), wf.shape[0], int(window), int(hop), int(n_windows),
                  _lib.ptr(out), _lib.stream_handle(wf.device))
    return out


def window_starts(n: int, window: int, hop: int) -> range:
    """slice_waveform's start indices: range(0, n - window + 1, hop) (inference_runner.py:180)."""
    return range(0, n - window + 1, hop)


def select_windows(wf: torch.Tensor, sr: int, window_size: float, overlap: float,
                   silence_threshold: float) -> Tuple[List[int], List[float]]:
    """slice_waveform (inference_runner.py:176-190) on a device waveform: the
    kept windows' start samples and start times (s).  A window is skipped when
    its max |x| < silence_threshold, compared in fp32 as torch compares a
    float32 tensor with a Python float."""
    window = int(window_size * sr)
    hop = int((1 - overlap) * window)
    if hop <= 0:
        raise ValueError(f'hop of {hop} samples (overlap={overlap}): range() would reject it too')
    starts = window_starts(wf.shape[0], window, hop)
    if len(starts) == 0:
        return [], []
    mx = window_absmax(wf, window, hop, len(starts)).cpu().numpy()
    keep = ~(mx < np.float32(silence_threshold))
    kept = [s for s, k in zip(starts, keep) if k]
    return kept, [s / sr for s in kept]


class Windows:
    """The kept windows of one device waveform: the waveform, the window length
    and the start offsets (int64, on the device) that the front end reads
    them at."""

    def __init__(self, wf: torch.Tensor, starts: List[int], window: int):
        self.wf, self.window = wf, int(window)
        self.starts = list(starts)
        if any(s < 0 or s + self.window > wf.shape[0] for s in self.starts):
            raise ValueError('window start out of range')
        self.offsets = torch.tensor(self.starts, dtype=torch.int64).to(wf.device)

    def __len__(self):
        return len(self.starts)


# ------------------------------------------------------------ trainer ingestion
# The trainer's second input path (submodel_trainer.py --device-ingest): the
# DataLoader workers read only the head of each file that the two 4 s training
# segments need, as stored; one upload per batch carries the samples and the
# tables; one launch (sad_train_ingest_run, csrc/ingest.hip) turns them into the
# [2B, seg_len] fp32 segments TrainFrontEnd takes.  Everything up to the upload
# is numpy / torch on the host and never loads libsad, so it runs in workers.
TRAIN_TILE = 1024      # TI_TILE: outputs per tile (native and per-output forms)
TRAIN_SPAN = 8192      # TI_SPAN: the per-output form's input span in LDS
TRAIN_MAX_RATES = 8    # TI_MAX_RATES: distinct source rates in one launch
TRAIN_COLS = 6         # file table columns (include/sad.h "trainer ingestion")
TRAIN_WIDE_FRAMES = 64  # RS_WAVES * RS_R: frames per tile of the wide form
WAVE_SUB = 32          # WA_SUB (csrc/waveaug.hip): frames a lane walks serially
WAVE_CHUNK = 2048      # WA_CHUNK: frames per workgroup, the phaser scan's chunk
WAVE_COLS = 8          # augmentation table columns (include/sad.h "waveform augmentation")
STRETCH_CODE0 = _augment.STRETCH_CODE0   # the first kind code of sad_wave_stretch_run (include/sad.h "time and pitch")
# sad_wave_stretch_geometry (tests/test_stretch_reference.py ties them to the library): n_fft, hop, the
# vocoder scan's chunk in output frames, the batch entry's launch bound
STRETCH_N_FFT, STRETCH_HOP, STRETCH_CHUNK, STRETCH_MAX_LAUNCHES = 2048, 512, 64, 17


def resample_geometry(sr: int, target_sr: int = 32000):
    """(orig, new, width, K) of sad_resample_plan_create: the rates reduced by
    their gcd, torchaudio's filter half-width and the taps per output."""
    g = math.gcd(int(sr), int(target_sr))
    orig, new = int(sr) // g, int(target_sr) // g
    width = math.ceil(6 * orig / (min(orig, new) * 0.99))
    return orig, new, width, 2 * width + orig


def train_out_len(frames: int, sr: int, target_sr: int = 32000) -> int:
    """The file's length at target_sr: ceil(new * frames / orig) (sad_resample_out_len)."""
    if int(sr) == int(target_sr):
        return int(frames)
    orig, new, _, _ = resample_geometry(sr, target_sr)
    return (new * int(frames) + orig - 1) // orig


def train_need_frames(sr: int, seg_len: int, target_sr: int = 32000) -> int:
    """sad_train_ingest_need_frames: the frames the first 2 seg_len output
    samples read.  The last of them, m = 2 seg_len - 1 = j new + p, reads
    inputs up to j orig + K - 1 - width = j orig + orig + width - 1."""
    if int(sr) == int(target_sr):
        return 2 * int(seg_len)
    orig, new, width, _ = resample_geometry(sr, target_sr)
    return (2 * int(seg_len) - 1) // new * orig + orig + width


def train_segment_rule(n: int, seg_len: int, min_length_ratio: float = 0.9):
    """segment_waveform's decision (submodel_trainer.py:155-187) from the 32 kHz
    length alone: 'two' segments, the 'first' one twice, the zero-'pad'ded
    file twice, or None (too short)."""
    if n >= 2 * seg_len:
        return 'two'
    if n >= seg_len:
        return 'first'
    if n >= seg_len * min_length_ratio:
        return 'pad'
    return None


def train_file_tiles(sr: int, total_frames: int, seg_len: int, target_sr: int = 32000) -> int:
    """sad_train_ingest_file_tiles: workgroups of one file (0: the rate is refused)."""
    n_out = train_out_len(total_frames, sr, target_sr)
    m = seg_len if n_out < 2 * seg_len else 2 * seg_len
    if int(sr) == int(target_sr):
        return -(-m // TRAIN_TILE)
    orig, new, _, K = resample_geometry(sr, target_sr)
    if new < 64:
        if ((TRAIN_TILE - 1) // new + 1) * orig + K > TRAIN_SPAN:
            return 0
        return -(-m // TRAIN_TILE)
    return -(-(-(-m // new)) // TRAIN_WIDE_FRAMES) * (-(-new // 64))


def train_rate_supported(sr: int, target_sr: int = 32000) -> bool:
    return sr > 0 and train_file_tiles(sr, 1, 1, target_sr) > 0


class StoredFile:
    """One training file as its DataLoader worker leaves it: the first
    `frames_read` frames as stored (int16, or fp32 decoded from another
    encoding), the header's metadata, the label and the augmentation rows.
    `wave` is the file's waveform augmentation draw (kind code, p0, p1, key:
    sad.augment.wave_aug_params), or None without --wave-augment."""
    __slots__ = ('samples', 'frames_read', 'frames', 'channels', 'sr', 'target', 'aug', 'wave')

    def __init__(self, samples: np.ndarray, frames: int, channels: int, sr: int, target: int, aug: torch.Tensor,
                 wave=None):
        assert samples.dtype in (np.int16, np.float32) and samples.ndim == 1
        self.samples, self.frames, self.channels, self.sr = samples, int(frames), int(channels), int(sr)
        self.frames_read = samples.shape[0] // self.channels
        self.target, self.aug, self.wave = int(target), aug, wave


class StoredBatch:
    """A batch of stored files, ready for one upload.  `arena` (uint8) holds the
    files' samples, each starting at a multiple of 16 bytes, then the file
    table [n_files, 6] int64 and the tile table [n_tiles, 2] int32
    (include/sad.h "trainer ingestion").  `rates[i]` is the sample rate behind
    rate index i; targets int64 [B]; aug int32 [B, 2, 8].

    With waveform augmentation (a file drew another kind than 'original') the
    arena also carries, at wave_off, the augmentation table [n_files, 8] int64
    and, at mono_table_off, the file table of the fp32 mono arena that
    sad_wave_augment_run writes (mono_bytes long; made on the device, never
    uploaded); both offsets are None otherwise."""

    def __init__(self, arena, n_files, n_tiles, table_off, tiles_off, rates, targets, aug, seg_len,
                 wave_off=None, mono_table_off=None, mono_bytes=0, stretch_off=None):
        self.arena, self.n_files, self.n_tiles = arena, int(n_files), int(n_tiles)
        self.table_off, self.tiles_off = int(table_off), int(tiles_off)
        self.rates, self.targets, self.aug, self.seg_len = tuple(rates), targets, aug, int(seg_len)
        self.wave_off, self.mono_table_off, self.mono_bytes = wave_off, mono_table_off, int(mono_bytes)
        self.stretch_off = stretch_off  # the stretch table [n_files, 8] (a file drew a kind >= 6), or None

    @property
    def table(self) -> torch.Tensor:
        return self.arena[self.table_off:self.table_off + 8 * TRAIN_COLS * self.n_files].view(torch.int64).view(
            self.n_files, TRAIN_COLS)

    @property
    def tiles(self) -> torch.Tensor:
        return self.arena[self.tiles_off:self.tiles_off + 8 * self.n_tiles].view(torch.int32).view(self.n_tiles, 2)

    def _rows(self, off, cols) -> torch.Tensor:
        return self.arena[off:off + 8 * cols * self.n_files].view(torch.int64).view(self.n_files, cols)

    @property
    def wave_table(self) -> torch.Tensor:
        return self._rows(self.wave_off, WAVE_COLS)

    @property
    def stretch_table(self) -> torch.Tensor:
        return self._rows(self.stretch_off, WAVE_COLS)

    @property
    def mono_table(self) -> torch.Tensor:
        return self._rows(self.mono_table_off, TRAIN_COLS)

    def pin_memory(self):
        """DataLoader(pin_memory=True) calls this: the arena is the upload."""
        self.arena = self.arena.pin_memory()
        return self

    def __len__(self):
        return self.n_files


def _align(n: int, a: int = 16) -> int:
    return -(-n // a) * a


def collate_stored(files, seg_len: int = 128000, target_sr: int = 32000):
    """Collate for the stored-sample dataset: drops None (as custom_collate_fn
    does), packs the rest into one StoredBatch, or returns None."""
    files = [f for f in files if f is not None]
    if not files:
        return None
    rates = []
    for f in files:
        if f.sr not in rates:
            rates.append(f.sr)
    if len(rates) > TRAIN_MAX_RATES:
        raise ValueError(f'{len(rates)} distinct sample rates in one batch (at most {TRAIN_MAX_RATES})')
    table = np.zeros((len(files), TRAIN_COLS), np.int64)
    tiles, off = [], 0
    for i, f in enumerate(files):
        nt = train_file_tiles(f.sr, _out_frames(f), seg_len, target_sr)
        if nt <= 0:
            raise ValueError(f'sample rate {f.sr} Hz is not supported by the batched ingestion kernel')
        table[i] = (off, f.frames_read, f.frames, f.channels,
                    _lib.SAD_PCM_I16 if f.samples.dtype == np.int16 else _lib.SAD_PCM_F32, rates.index(f.sr))
        tiles.append(np.stack((np.full(nt, i, np.int32), np.arange(nt, dtype=np.int32)), axis=1))
        off = _align(off + f.samples.nbytes)
    tiles = np.concatenate(tiles)
    table_off = off
    tiles_off = _align(table_off + table.nbytes)
    end = _align(tiles_off + tiles.nbytes)
    wave = _wave_tables(files, table, seg_len, target_sr)
    extra = {}
    if wave is not None:  # a batch of 'original' draws is the plain path
        wave_table, mono_table, mono_bytes, stretch_table = wave
        extra = dict(wave_off=end, mono_table_off=_align(end + wave_table.nbytes), mono_bytes=mono_bytes)
        end = _align(extra['mono_table_off'] + mono_table.nbytes)
        if stretch_table is not None:
            extra['stretch_off'] = end
            end = _align(end + stretch_table.nbytes)
    buf = np.zeros(end, np.uint8)
    for row, f in zip(table, files):
        buf[row[0]:row[0] + f.samples.nbytes] = f.samples.view(np.uint8)
    buf[table_off:table_off + table.nbytes] = table.reshape(-1).view(np.uint8)
    buf[tiles_off:tiles_off + tiles.nbytes] = tiles.reshape(-1).view(np.uint8)
    if wave is not None:
        buf[extra['wave_off']:extra['wave_off'] + wave_table.nbytes] = wave_table.reshape(-1).view(np.uint8)
        o = extra['mono_table_off']
        buf[o:o + mono_table.nbytes] = mono_table.reshape(-1).view(np.uint8)
        if stretch_table is not None:
            o = extra['stretch_off']
            buf[o:o + stretch_table.nbytes] = stretch_table.reshape(-1).view(np.uint8)
    return StoredBatch(torch.from_numpy(buf), len(files), tiles.shape[0], table_off, tiles_off, rates,
                       torch.tensor([f.target for f in files]), torch.stack([f.aug for f in files]), seg_len, **extra)


# ---- time and pitch: the lengths of tests/stretch_ref.py (the float64 contract)
def pitch_rate(steps: float) -> float:
    return 2.0 ** (-float(steps) / 12.0)


def stretch_rates(kind: int, p0: float, p1: float):
    """(stretch rate or None, pitch rate or None) of a kind code 6..10."""
    k = kind - STRETCH_CODE0
    if k in (0, 1):
        return float(p0), None
    if k in (2, 3):
        return None, pitch_rate(p0)
    return float(p0), pitch_rate(p1)


def stretch_out_len(kind: int, frames: int, p0: float, p1: float = 0.0) -> int:
    """The kind's output length: round(frames / rate); a pitch shift keeps its input's."""
    rate, _ = stretch_rates(kind, p0, p1)
    return int(frames) if rate is None else int(round(int(frames) / rate))


def _stretch_need(rate: float, n_out: int) -> int:
    """Output sample m sums the synthesis frames t <= (m + 1024) // 512; step t
    reads the analysis frames int(t rate), int(t rate) + 1; frame f the samples
    below 512 f + 1024."""
    if n_out <= 0:
        return 0
    t = (n_out - 1 + STRETCH_N_FFT // 2) // STRETCH_HOP
    return (int(t * float(rate)) + 1) * STRETCH_HOP + STRETCH_N_FFT // 2


def _resample_need(rho: float, n_out: int) -> int:
    if n_out <= 0:
        return 0
    return max(int(math.ceil((n_out - 1) / float(rho) + 6.0 / (0.99 * min(1.0, rho)))), 0)


def stretch_need_frames(kind: int, p0: float, p1: float, n_out: int) -> int:
    """The input frames the first n_out output frames of the kind depend on
    (tests/stretch_ref.py need_frames): what a worker reads of the file."""
    rate, prate = stretch_rates(kind, p0, p1)
    n = int(n_out)
    if prate is not None:
        n = _stretch_need(prate, _resample_need(prate, n))
    return n if rate is None else _stretch_need(rate, n)


def _f64bits(v: float) -> int:
    return int(np.array([v], np.float64).view(np.int64)[0])


def wave_chunks(n_out: int) -> int:
    return -(-int(n_out) // WAVE_CHUNK)


def _is_stretch(f) -> bool:
    return f.wave is not None and f.wave[0] >= STRETCH_CODE0


def _out_frames(f) -> int:
    """The file's length after its waveform augmentation: a stretch changes it."""
    return stretch_out_len(f.wave[0], f.frames, f.wave[1], f.wave[2]) if _is_stretch(f) else f.frames


def _wave_tables(files, table, seg_len, target_sr):
    """(augmentation table [B, 8], the mono arena's file table [B, 6], the mono
    arena's bytes, stretch table [B, 8] or None) of include/sad.h "waveform
    augmentation" and "time and pitch", or None when every file drew 'original'
    (kind 0) or none has a draw.  File f's output holds its first min(total,
    need) frames: what the two segments read.  A file of a stretch kind (code
    >= 6) is an empty 'original' row of the augmentation table and the other way
    round, so the two entries fill one arena between them."""
    if all(f.wave is None or f.wave[0] == 0 for f in files):
        return None
    wave = np.zeros((len(files), WAVE_COLS), np.int64)
    mono = np.zeros((len(files), TRAIN_COLS), np.int64)
    stretch = np.zeros((len(files), WAVE_COLS), np.int64) if any(_is_stretch(f) for f in files) else None
    off = chunks = 0
    for i, f in enumerate(files):
        kind, p0, p1, key = f.wave if f.wave is not None else (0, 0.0, 0.0, 0)
        if kind >= STRETCH_CODE0:
            total = _out_frames(f)
            n_out = min(total, train_need_frames(f.sr, seg_len, target_sr))
            rate, prate = stretch_rates(kind, p0, p1)
            steps = p0 if rate is None else p1
            stretch[i] = (kind, _f64bits(rate or 0.0), _f64bits(steps if prate is not None else 0.0), n_out, off,
                          _f64bits(prate or 0.0), 0, 0)
            wave[i, :4] = (0, f.sr, 0, off)
            wave[i, 6] = chunks
            mono[i] = (off, n_out, total, 1, _lib.SAD_PCM_F32, table[i, 5])
            off = _align(off + 4 * n_out)
            continue
        n_out = min(f.frames, f.frames_read, train_need_frames(f.sr, seg_len, target_sr))
        params = np.array([p0, p1], np.float32).view(np.uint32).astype(np.uint64)
        wave[i, :4] = (kind, f.sr, n_out, off)
        wave[i, 4:6] = np.array([params[0] | (params[1] << np.uint64(32)), int(key) & 0xFFFFFFFFFFFFFFFF],
                                np.uint64).view(np.int64)
        wave[i, 6] = chunks
        mono[i] = (off, n_out, f.frames, 1, _lib.SAD_PCM_F32, table[i, 5])
        off = _align(off + 4 * n_out)
        chunks += wave_chunks(n_out)
    return wave, mono, off, stretch


class TrainIngest:
    """StoredBatch -> the batch's training segments on the device, fp32
    [2B, seg_len] with file f's two segments in rows 2f and 2f + 1: one upload
    and one launch per batch, queued on the current stream."""

    def __init__(self, device='cuda', target_sr: int = 32000):
        self.device = _dev(device)
        self.target_sr = int(target_sr)

    def need_frames(self, sr: int, seg_len: int) -> int:
        n = _lib.I64()
        _lib.call('sad_train_ingest_need_frames', int(sr), self.target_sr, int(seg_len), ctypes.byref(n))
        return n.value

    def file_tiles(self, sr: int, total_frames: int, seg_len: int) -> int:
        n = _lib.I64()
        _lib.call('sad_train_ingest_file_tiles', int(sr), self.target_sr, int(total_frames), int(seg_len),
                  ctypes.byref(n))
        return n.value

    def __call__(self, batch: StoredBatch) -> torch.Tensor:
        dev = self.device
        plans = (ctypes.c_void_p * len(batch.rates))(*[
            None if sr == self.target_sr else resampler(sr, self.target_sr, dev)._plan for sr in batch.rates])
        d_arena = batch.arena.to(dev, non_blocking=True)  # pinned by the DataLoader: asynchronous
        out = torch.empty(2 * batch.n_files, batch.seg_len, device=dev, dtype=torch.float32)
        base = d_arena.data_ptr()
        with torch.cuda.device(dev):
            src, src_bytes, table, d_table = base, batch.table_off, batch.table, base + batch.table_off
            if batch.wave_off is not None:  # stage one: augment into an fp32 mono arena, then ingest that
                mono = self.wave_augment(batch, d_arena)
                if batch.stretch_off is not None:  # the files of the stretch kinds, into the same arena
                    self.wave_stretch(batch, d_arena, mono)
                src, src_bytes, table, d_table = mono.data_ptr(), batch.mono_bytes, batch.mono_table, \
                    base + batch.mono_table_off
            _lib.call('sad_train_ingest_run', src, src_bytes, table.data_ptr(), d_table,
                      batch.n_files, base + batch.tiles_off, batch.n_tiles, plans, len(batch.rates), batch.seg_len,
                      _lib.ptr(out), _lib.stream_handle(dev))
        return out

    def wave_augment(self, batch: StoredBatch, d_arena: torch.Tensor) -> torch.Tensor:
        """sad_wave_augment_run on an uploaded batch: the fp32 mono arena (uint8
        [mono_bytes]; file f at batch.wave_table[f, 3], batch.wave_table[f, 2] frames)."""
        dev, base = self.device, d_arena.data_ptr()
        need = _lib.SZ()
        _lib.call('sad_wave_augment_workspace_size', batch.wave_table.data_ptr(), batch.n_files, ctypes.byref(need))
        mono = torch.empty(max(batch.mono_bytes, 16), device=dev, dtype=torch.uint8)
        ws = torch.empty(max(need.value, 16), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.call('sad_wave_augment_run', base, batch.table_off, batch.table.data_ptr(), base + batch.table_off,
                      batch.n_files, batch.wave_table.data_ptr(), base + batch.wave_off, mono.data_ptr(),
                      batch.mono_bytes, ws.data_ptr(), need.value, _lib.stream_handle(dev))
        return mono

    def wave_stretch(self, batch: StoredBatch, d_arena: torch.Tensor, mono: torch.Tensor) -> torch.Tensor:
        """sad_wave_stretch_run on an uploaded batch, into the arena wave_augment made
        (file f at batch.stretch_table[f, 4], batch.stretch_table[f, 3] frames)."""
        dev, base = self.device, d_arena.data_ptr()
        need = _lib.SZ()
        _lib.call('sad_wave_stretch_workspace_size', batch.table.data_ptr(), batch.stretch_table.data_ptr(),
                  batch.n_files, ctypes.byref(need))
        ws = torch.empty(max(need.value, 16), device=dev, dtype=torch.uint8)
        with torch.cuda.device(dev):
            _lib.call('sad_wave_stretch_run', base, batch.table_off, batch.table.data_ptr(), base + batch.table_off,
                      batch.n_files, batch.stretch_table.data_ptr(), base + batch.stretch_off, mono.data_ptr(),
                      batch.mono_bytes, ws.data_ptr(), need.value, _lib.stream_handle(dev))
        return mono

    def segments(self, batch: StoredBatch) -> torch.Tensor:
        """The rows in the host path's order: every file's first segment, then
        every file's second (DeviceModel.images' torch.cat((input1, input2)))."""
        out = self(batch)
        return out.view(batch.n_files, 2, batch.seg_len).transpose(0, 1).reshape(2 * batch.n_files, batch.seg_len)
