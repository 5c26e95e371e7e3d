"""GPU: the time-stretch and pitch-shift kernels (csrc/stretch.hip) against the
float64 contract (tests/stretch_ref.py).

Per stage, on identical fp32 inputs, each element against a bar written from
the stage's arithmetic before anything was measured:

  stft / istft  an element's path through the radix-2 FFT is 11 butterflies of a
      complex multiply (4 mul, 2 add) and an add (2): 88 operations, plus the
      window and the 11 rounded twiddles: 100 roundings of 2^-24, each relative to
      at most the frame's 2-norm (the istft's 1 / N scaling applied to it).
      The overlap-add weighs a frame's bar by its window and divides by the
      window sum; 8 x 2^-24 |ref| covers the sum and the division.
  vocoder  relative to the reference magnitude; per angle, in turns: atan2f is
      within 2 ulp of a value below 4 rad (2^-21 rad, HIP's documented bound),
      times 1 / 2 pi, the fp32 product's rounding below 0.5 (2^-25, the
      constant's included) and the Q0.32 quantisation (2^-33).  Step t has summed
      2 t + 1 angles.  On top, once: the accumulator's rounding to fp32 half-turns
      (pi 2^-25 rad), sincospif (2 ulp) and the magnitude's hypotf (2 ulp each)
      and interpolation (3 roundings): 12 x 2^-24.
  resample  a dot product of n taps: (n + 10) 2^-24 sum |x_j h_j|, where 10 is the
      tap weight's own roundings, plus the fp32 rounding of u and c inside h,
      |dh| <= 2 c^2 |u| 2^-24 per tap, three times (u, c, c u).

Whole chain: bit-equality with the stage entries one after another, with a
second run, with a file run alone; against float64 on white noise within 4 x the
contract's own float32 twin's distance; tones keep or move their peak.

Every test prints the ratio it measured ("stretch ratio ...") before it asserts;
profiles/stretch_tests_ratios.txt holds those lines of one run, taken with
pytest -s -m gpu on this file and tests/test_gpu_stretch_train.py."""
import ctypes

import numpy as np
import pytest
import torch

import stretch_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
U = 2.0 ** -24


def _al(n):
    return -(-n // 16) * 16


def _bits(v):
    return int(np.array([v], np.float64).view(np.int64)[0])


def _note(name, ratio):
    print(f'stretch ratio {name}: {ratio:.3g}')


# ------------------------------------------------------------------ signals
def _signal(n, kind, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    if kind == 'noise':
        x = rng.uniform(-0.7, 0.7, n)
    elif kind == 'tone':
        x = 0.5 * np.sin(2 * np.pi * 1000.0 * t / 22050) + 0.2 * np.sin(2 * np.pi * 3300.0 * t / 22050 + 1.0)
    elif kind == 'bursts':   # speech-like: int16-quantised bursts between stretches of exact zeros
        env = (np.sin(2 * np.pi * t / 3000.0) > 0.2).astype(np.float64)
        x = np.round(env * rng.normal(0, 0.15, n) * np.sin(2 * np.pi * 180.0 * t / 22050) * 32768) / 32768
    else:
        x = np.zeros(n)
    return x.astype(np.float32)


LENGTHS = (1, 511, 512, 513, 2047, 2048, 2049, 20000)
KINDS = ('noise', 'tone', 'bursts', 'noise', 'bursts', 'tone', 'noise', 'bursts')


@pytest.fixture(scope='module')
def signals():
    xs = [_signal(n, k, 10 + i) for i, (n, k) in enumerate(zip(LENGTHS, KINDS))]
    xs.append(np.zeros(3000, np.float32))
    xs.append(_signal(20000, 'tone', 31))
    return xs


# ------------------------------------------------------- the stage entries
def _pack(arrays, dtype):
    """arrays -> (device uint8 buffer, byte offsets): each starts at a multiple of 16."""
    offs, off = [], 0
    for a in arrays:
        offs.append(off)
        off = _al(off + a.size * a.itemsize)
    buf = np.zeros(max(off, 16), np.uint8)
    for a, o in zip(arrays, offs):
        buf[o:o + a.size * a.itemsize] = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    return torch.from_numpy(buf).to(DEV), offs


def _stage(name, inputs, rows, out_sizes, out_dtype, ws_name=None):
    """Run one stage entry on a batch: inputs (numpy arrays), rows (count in, count
    out, rate, flags) per file; returns the outputs as numpy arrays."""
    from sad import _lib
    d_in, in_offs = _pack(inputs, None)
    out_offs, off = [], 0
    for n in out_sizes:
        out_offs.append(off)
        off = _al(off + n)
    table = np.zeros((len(rows), 8), np.int64)
    for f, (n_in, n_out, rate, flags) in enumerate(rows):
        table[f] = (in_offs[f], n_in, out_offs[f], n_out, _bits(rate), flags, 0, 0)
    ws = None
    need = _lib.SZ()
    if ws_name:
        wso = 0
        for f in range(len(rows)):
            one = np.ascontiguousarray(table[f:f + 1])
            _lib.call(ws_name, one.ctypes.data, 1, ctypes.byref(need))
            table[f, 6] = wso
            wso += need.value
        _lib.call(ws_name, table.ctypes.data, len(rows), ctypes.byref(need))
        assert need.value == wso
        ws = torch.full((max(wso, 16),), 0xA5, device=DEV, dtype=torch.uint8)
    d_table = torch.from_numpy(table).to(DEV)
    d_out = torch.full((max(off, 16),), 0xA5, device=DEV, dtype=torch.uint8)
    args = [d_in.data_ptr(), d_in.numel(), table.ctypes.data, d_table.data_ptr(), len(rows), d_out.data_ptr(), off]
    if ws_name:
        args += [ws.data_ptr(), need.value]
    _lib.call(name, *args, _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    return [host[o:o + n].view(out_dtype).copy() for o, n in zip(out_offs, out_sizes)]


def dev_stft(xs):
    T = [R.n_frames(len(x)) for x in xs]
    out = _stage('sad_stft2048_run', xs, [(len(x), t, 0.0, 0) for x, t in zip(xs, T)], [t * R.BINS * 8 for t in T],
                 np.complex64)
    return [o.reshape(t, R.BINS) for o, t in zip(out, T)]


def dev_vocoder(Ds, rates, counts=None):
    n = [R.n_steps(D.shape[0], r) for D, r in zip(Ds, rates)] if counts is None else counts
    out = _stage('sad_phase_vocoder_run', Ds, [(D.shape[0], k, r, 0) for D, k, r in zip(Ds, n, rates)],
                 [k * R.BINS * 8 for k in n], np.complex64, 'sad_phase_vocoder_workspace_size')
    return [o.reshape(k, R.BINS) for o, k in zip(out, n)]


def dev_istft(Ss, lengths, clip=False):
    return _stage('sad_istft2048_run', Ss, [(S.shape[0], n, 0.0, int(clip)) for S, n in zip(Ss, lengths)],
                  [4 * n for n in lengths], np.float32, 'sad_istft2048_workspace_size')


def dev_resample(xs, rhos, n_outs, clip=False):
    return _stage('sad_resample_ratio_run', xs, [(len(x), n, r, int(clip)) for x, n, r in zip(xs, n_outs, rhos)],
                  [4 * n for n in n_outs], np.float32)


def dev_mono(x):
    from sad import ingest
    return ingest.mono(torch.from_numpy(np.ascontiguousarray(x.reshape(-1))).to(DEV), x.shape[1]).cpu().numpy()


def dev_stretch(ys, rates, clip=False):
    Ds = dev_stft(ys)
    Ss = dev_vocoder(Ds, rates)
    return dev_istft(Ss, [R.stretch_len(len(y), r) for y, r in zip(ys, rates)], clip)


def compose(x, kind, p0, p1):
    """The stage entries one after another on one file alone, whole-file sizes."""
    y = dev_mono(x)
    name = R.STRETCH_KINDS[kind - 6]
    if name in ('speed_up', 'slow_down'):
        return dev_stretch([y], [p0], clip=True)[0]
    if name == 'time_pitch_shift':
        y, steps = dev_stretch([y], [p0])[0], p1
    else:
        steps = p0
    r = R.pitch_rate(steps)
    return dev_resample(dev_stretch([y], [r]), [r], [len(y)], clip=True)[0]


# ---------------------------------------------------------- per-stage bars
FFT_ROUNDINGS = 100


def test_stft_per_element(signals):
    got = dev_stft(signals)
    worst = 0.0
    for x, D in zip(signals, got):
        ref = R.stft(x.astype(np.float64))
        norm = np.linalg.norm(R._frames(x.astype(np.float64), np.float64), axis=1)
        bar = FFT_ROUNDINGS * U * norm[:, None]
        err = np.abs(D.astype(np.complex128) - ref)
        assert np.all(err[bar[:, 0] == 0] == 0)   # exact zeros in, exact zeros out
        worst = max(worst, (err / np.maximum(bar, 1e-300)).max() if bar.max() > 0 else 0.0)
    _note('stft', worst)
    assert worst <= 1.0


def _istft_bar(S, length):
    nf = R.istft_frames(length, S.shape[0])
    w = R.hann()
    full = np.concatenate([np.abs(S[:nf]), np.abs(S[:nf, 1:-1][:, ::-1])], axis=1)
    fbar = FFT_ROUNDINGS * U * np.linalg.norm(full, axis=1) / R.N_FFT
    n = R.N_FFT + R.HOP * (nf - 1) if nf else 0
    num, wsum = np.zeros(n), np.zeros(n)
    for t in range(nf):
        num[t * R.HOP:t * R.HOP + R.N_FFT] += fbar[t] * w
        wsum[t * R.HOP:t * R.HOP + R.N_FFT] += w * w
    ok = wsum > np.finfo(np.float32).tiny
    num[ok] /= wsum[ok]
    out = np.zeros(length)
    m = min(max(n - R.PAD, 0), length)
    out[:m] = num[R.PAD:R.PAD + m]
    return out


def test_istft_per_element(signals):
    Ds = dev_stft(signals)
    lengths = [len(x) for x in signals]
    lengths[3] = 700     # zero-padded past the frames
    lengths[7] = 15000   # cropped: only the first ceil((length + 2048) / 512) frames are read
    got = dev_istft(Ds, lengths)
    worst = 0.0
    for D, n, y in zip(Ds, lengths, got):
        ref = R.istft(D.astype(np.complex128), n)
        bar = _istft_bar(D.astype(np.complex128), n) + 8 * U * np.abs(ref)
        err = np.abs(y.astype(np.float64) - ref)
        assert np.all(err[bar == 0] == 0)
        worst = max(worst, (err[bar > 0] / bar[bar > 0]).max() if (bar > 0).any() else 0.0)
    _note('istft', worst)
    assert worst <= 1.0


ANGLE_TURNS = 2.0 ** -21 / (2 * np.pi) + 2.0 ** -25 + 2.0 ** -33


def _vocoder_bar(ref):
    t = np.arange(ref.shape[0])[:, None]
    return np.abs(ref) * (2 * np.pi * (2 * t + 1) * ANGLE_TURNS + 12 * U) + 1e-30


def test_vocoder_per_element(signals):
    chunk = 64
    Ds = dev_stft(signals[4:])   # 2047 .. 20000 samples, zeros, tone
    rates = [0.5, 0.83, 1.0, 1.37, 1.5, 0.5][:len(Ds)]
    long = dev_stft([_signal(300000, 'noise', 77)])[0]
    Ds, rates = Ds + [long, long[:chunk + 2], long[:chunk + 2], long[:chunk + 2]], rates + [0.5, 1.0, 1.0, 1.0]
    counts = [R.n_steps(D.shape[0], r) for D, r in zip(Ds, rates)]
    counts[-3:] = [chunk - 1, chunk, chunk + 1]
    assert counts[-4] > 16 * chunk   # the scan crosses many chunks
    got = dev_vocoder(Ds, rates, counts)
    worst = 0.0
    for D, r, k, S in zip(Ds, rates, counts, got):
        ref = R.phase_vocoder(D.astype(np.complex128), r)[:k]
        worst = max(worst, (np.abs(S.astype(np.complex128) - ref) / _vocoder_bar(ref)).max())
    _note('vocoder', worst)
    assert worst <= 1.0


def test_resample_per_element(signals):
    xs = [signals[7], signals[9], signals[4], signals[0], signals[7]]
    rhos = [R.pitch_rate(2), R.pitch_rate(-2), R.pitch_rate(-0.5), 0.9, 0.25]
    n_outs = [len(xs[0]), 21000, 2047, 3, 5100]
    got = dev_resample(xs, rhos, n_outs)
    worst = 0.0
    for x, rho, n, y in zip(xs, rhos, n_outs, got):
        x64 = x.astype(np.float64)
        ref = R.resample_ratio(x64, rho, n)
        c, half = R._taps(rho)
        pos = np.arange(n) / rho
        j = np.floor(pos - half).astype(np.int64)[:, None] + np.arange(int(np.ceil(2 * half)) + 2)[None, :]
        u = pos[:, None] - j
        h = c * np.sinc(c * u) * np.cos(np.pi * u * c / 12) ** 2
        inside = (np.abs(u) < half) & (j >= 0) & (j < len(x))
        xa = np.where(inside, np.abs(x64[np.clip(j, 0, len(x) - 1)]), 0.0)
        taps = inside.sum(axis=1)
        bar = (taps + 10) * U * (xa * np.abs(h)).sum(axis=1) + 3 * 2 * c * c * U * (xa * np.abs(u)).sum(axis=1)
        err = np.abs(y.astype(np.float64) - ref)
        assert np.all(err[bar == 0] == 0)
        worst = max(worst, (err[bar > 0] / bar[bar > 0]).max())
    _note('resample', worst)
    assert worst <= 1.0


# -------------------------------------------------------------- whole chain
def _pcm(frames, ch, seed, dtype=np.int16):
    rng = np.random.default_rng(seed)
    if dtype == np.int16:
        return rng.integers(-20000, 20000, size=(frames, ch)).astype(np.int16)
    return rng.uniform(-0.6, 0.6, size=(frames, ch)).astype(np.float32)


def run_batch(files, garbage=0xA5):
    """sad_wave_stretch_run on files = [(x [frames, ch], total, kind, p0, p1, n_out)];
    x holds the frames present.  Returns each file's n_out samples."""
    from sad import _lib, ingest
    d_arena, offs = _pack([f[0] for f in files], None)
    ft = np.zeros((len(files), 6), np.int64)
    st = np.zeros((len(files), 8), np.int64)
    out_offs, off = [], 0
    for i, (x, total, kind, p0, p1, n_out) in enumerate(files):
        rate, prate = ingest.stretch_rates(kind, p0, p1)
        ft[i] = (offs[i], x.shape[0], total, x.shape[1], 0 if x.dtype == np.int16 else 1, 0)
        st[i] = (kind, _bits(rate or 0.0), _bits((p0 if rate is None else p1) if prate else 0.0), n_out, off,
                 _bits(prate or 0.0), 0, 0)
        out_offs.append(off)
        off = _al(off + 4 * n_out)
    need = _lib.SZ()
    _lib.call('sad_wave_stretch_workspace_size', ft.ctypes.data, st.ctypes.data, len(files), ctypes.byref(need))
    ws = torch.full((need.value,), garbage, device=DEV, dtype=torch.uint8)
    mono = torch.full((max(off, 16),), garbage, device=DEV, dtype=torch.uint8)
    d_ft, d_st = torch.from_numpy(ft).to(DEV), torch.from_numpy(st).to(DEV)
    _lib.call('sad_wave_stretch_run', d_arena.data_ptr(), d_arena.numel(), ft.ctypes.data, d_ft.data_ptr(), len(files),
              st.ctypes.data, d_st.data_ptr(), mono.data_ptr(), off, ws.data_ptr(), need.value,
              _lib.stream_handle(DEV))
    torch.cuda.synchronize()
    host = mono.cpu().numpy()
    return [host[o:o + 4 * f[5]].view(np.float32).copy() for o, f in zip(out_offs, files)]


def _file(frames, ch, seed, dtype, kind, p0, p1, n_want):
    """A file of which the worker read what the first n_want outputs need."""
    from sad import ingest
    x = _pcm(frames, ch, seed, dtype)
    n_out = min(ingest.stretch_out_len(kind, frames, p0, p1), n_want)
    keep = min(frames, ingest.stretch_need_frames(kind, p0, p1, n_out))
    return (np.ascontiguousarray(x[:keep]), frames, kind, p0, p1, n_out), x


def _chain_files():
    """Seven files, every kind, both encodings, 1-3 channels, the odd lengths,
    heads of 8 kHz (2 x 4000 x 8 / 32 = 2000 frames) and 44.1 kHz (11025) files."""
    spec = [(20000, 1, np.int16, 6, 1.37, 0.0, 11025), (2049, 2, np.float32, 7, 0.5, 0.0, 11025),
            (30000, 3, np.int16, 8, 2.0, 0.0, 2000), (513, 1, np.int16, 9, -2.0, 0.0, 2000),
            (40000, 2, np.float32, 10, 0.83, -0.5, 11025), (1, 1, np.int16, 6, 1.5, 0.0, 2000),
            (2047, 1, np.float32, 10, 1.2, 1.0, 11025)]
    return [_file(n, ch, 60 + i, dt, k, p0, p1, want) for i, (n, ch, dt, k, p0, p1, want) in enumerate(spec)]


def test_batch_equals_the_stage_entries_bit_for_bit_and_does_not_depend_on_neighbours():
    files = _chain_files()
    got = run_batch([f for f, _ in files])
    for (f, x), y in zip(files, got):
        ref = compose(x, f[2], f[3], f[4])[:f[5]]
        assert len(y) == f[5] and np.array_equal(y, ref), (f[1:],)
        assert np.abs(y).max() <= 1.0
    again = run_batch([f for f, _ in files], garbage=0x3C)   # other garbage in the workspace and the arena
    assert all(np.array_equal(a, b) for a, b in zip(got, again))
    for i in (0, 4, 5):   # alone, and in a batch of other neighbours
        assert np.array_equal(run_batch([files[i][0]])[0], got[i])
    sub = run_batch([files[4][0], files[2][0], files[0][0]])
    assert np.array_equal(sub[0], got[4]) and np.array_equal(sub[1], got[2]) and np.array_equal(sub[2], got[0])


def test_a_long_file_whose_scan_crosses_many_chunks_and_frame_counts_at_the_chunk():
    x = _pcm(300000, 1, 90)
    got = run_batch([(x, 300000, 7, 0.5, 0.0, 600000)])[0]
    assert np.array_equal(got, compose(x, 7, 0.5, 0.0))
    # n_out for which the entry computes chunk - 1, chunk and chunk + 1 synthesis frames
    x = _pcm(40000, 2, 91)
    for frames in (63, 64, 65):
        n_out = (frames - 1) * 512 - 1023
        got = run_batch([(x, 40000, 6, 1.0, 0.0, n_out)])[0]
        assert np.array_equal(got, compose(x, 6, 1.0, 0.0)[:n_out]), frames


def test_rows_of_the_other_entry_are_left_alone():
    (f, x), = [_file(5000, 1, 95, np.int16, 6, 1.2, 0.0, 3000)]
    other = (_pcm(100, 1, 96), 100, 3, 0.0, 0.0, 0)
    got = run_batch([other, f, other])
    assert got[0].size == 0 and np.array_equal(got[1], run_batch([f])[0])


@pytest.mark.parametrize('sr_frames', [2000, 11025])
def test_white_noise_against_float64_within_four_times_the_f32_twin(sr_frames):
    cases = [(6, 1.37, 0.0), (6, 1.5, 0.0), (7, 0.5, 0.0), (7, 0.83, 0.0), (6, 1.0, 0.0), (8, 2.0, 0.0), (9, -2.0, 0.0),
             (9, -0.5, 0.0), (10, 0.83, -0.5), (10, 1.2, 1.0)]
    files = [_file(20000, 1 + i % 3, 120 + i, np.int16 if i % 2 else np.float32, k, p0, p1, sr_frames)
             for i, (k, p0, p1) in enumerate(cases)]
    worst = 0.0
    for lo in range(0, len(files), 5):
        got = run_batch([f for f, _ in files[lo:lo + 5]])
        for (f, x), y in zip(files[lo:lo + 5], got):
            mono = dev_mono(x)
            name = R.STRETCH_KINDS[f[2] - 6]
            ref = R.apply(name, mono.astype(np.float64), f[3], f[4])[:f[5]]
            twin = R.apply_f32(name, mono, f[3], f[4])[:f[5]]
            d_twin = np.abs(twin.astype(np.float64) - ref).max()
            d_dev = np.abs(y.astype(np.float64) - ref).max()
            _note(f'chain kind {f[2]} p {f[3]} {f[4]} n_out {f[5]}', d_dev / d_twin)
            worst = max(worst, d_dev / d_twin)
            assert d_dev <= 4 * d_twin, (f[1:], d_dev, d_twin)
    _note(f'chain worst n_out {sr_frames}', worst)


def test_tones_keep_or_move_their_peak():
    from test_stretch_reference import BIN, SR, _peak_hz, _tone
    x = np.round(_tone(1000.0, 24000) * 32767).astype(np.int16)[:, None]
    cases = [(7, 0.5), (7, 0.8), (6, 1.5), (9, -2.0), (8, 1.0), (8, 2.0)]
    files = [(x, 24000, k, p, 0.0, R.out_len(R.STRETCH_KINDS[k - 6], 24000, p)) for k, p in cases]
    got = run_batch(files[:3]) + run_batch(files[3:])
    for (k, p), y in zip(cases, got):
        want = 1000.0 if k < 8 else 1000.0 * 2 ** (p / 12)
        assert abs(_peak_hz(y.astype(np.float64), SR) - want) <= BIN, (k, p)
