"""The float64 contract of the time-stretch and pitch-shift augmentation
(submodel_trainer.py --wave-stretch, csrc/stretch.hip, include/sad.h "time and
pitch"): the five kinds of the reference's audio_augmneter.py that go through
librosa (speed_up, slow_down, pitch_up, pitch_down, time_pitch_shift; :55-76,
:140-145, the clip of :190).

It restates what librosa >= 0.10 documents for effects.time_stretch and
effects.pitch_shift (stft -> phase_vocoder -> istft, then a resample for the
pitch).  librosa and soxr are not installed where this was written, so NOTHING
HERE IS PINNED TO THEM: this file is the definition.  Known departures:

  * the resampler of pitch_shift is not librosa's soxr_hq, which cannot be
    restated, but the Hann-windowed sinc family the ingestion already uses
    (torchaudio's sinc_interp_hann, width 6, rolloff 0.99) evaluated at an
    arbitrary ratio: resample_ratio below;
  * the tool's resample to 44.1 kHz before augmenting and its 16-bit file round
    trip after it are not part of the contract (as for the six other kinds).

numpy only.  The *_f32 twins at the end run the same stages in float32 /
complex64 with the phase kept as an unsigned 32-bit fraction of a turn, as the
device does; the GPU tests use their distance from float64 as a yardstick.
"""
import math

import numpy as np

N_FFT = 2048
HOP = 512
BINS = N_FFT // 2 + 1
PAD = N_FFT // 2
LPW = 6          # the resampler's lowpass_filter_width
ROLLOFF = 0.99

STRETCH_KINDS = ('speed_up', 'slow_down', 'pitch_up', 'pitch_down', 'time_pitch_shift')
# audio_augmneter.py:55-76 (rate / n_steps), :140-145 (time_pitch_shift)
RANGES = {'speed_up': (1.0, 1.5), 'slow_down': (0.5, 1.0), 'pitch_up': (0.0, 2.0), 'pitch_down': (-2.0, 0.0),
          'time_pitch_shift': ((0.8, 1.2), (-1.0, 1.0))}


def hann(dtype=np.float64):
    """scipy.signal.get_window('hann', 2048, fftbins=True): periodic."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N_FFT) / N_FFT)).astype(dtype)


def n_frames(length):
    return 1 + int(length) // HOP


def _frames(y, dtype):
    y = np.asarray(y, dtype)
    yp = np.concatenate([np.zeros(PAD, dtype), y, np.zeros(PAD, dtype)])
    idx = np.arange(n_frames(len(y)))[:, None] * HOP + np.arange(N_FFT)[None, :]
    return yp[idx] * hann(dtype)[None, :]


def stft(y):
    """[T][1025] complex128, T = 1 + len(y) // 512: center=True, zero padding."""
    return np.fft.rfft(_frames(y, np.float64), axis=1)


# ---- the pieces the sharpness test swaps out
def _lerp(a, m0, m1):
    return (1.0 - a) * m0 + a * m1


def _dphase(ang1, ang0, phi):
    d = ang1 - ang0 - phi
    return d - 2.0 * np.pi * np.round(d / (2.0 * np.pi))   # wrap to [-pi, pi]


def _normalise(y, wsum, tiny):
    ok = wsum > tiny
    y = y.copy()
    y[ok] /= wsum[ok]
    return y


def _cutoff(rho):
    return ROLLOFF * min(1.0, rho)


def n_steps(T, rate):
    """len(arange(0, T, rate))."""
    return int(math.ceil(T / float(rate)))


def phase_vocoder(D, rate):
    """librosa.phase_vocoder on D [T][1025] -> [ceil(T / rate)][1025].

    The accumulator's update  acc += phi + wrap(angle(D[i+1]) - angle(D[i]) - phi)
    equals  acc += angle(D[i+1]) - angle(D[i])  modulo 2 pi (wrap() removes whole
    turns, phi cancels), so acc_t is a prefix sum of per-step angle differences
    modulo one turn: what the device computes in 32-bit fixed point."""
    D = np.asarray(D)
    T = D.shape[0]
    steps = np.arange(0, T, rate, dtype=np.float64)
    phi = 2.0 * np.pi * HOP * np.arange(BINS) / N_FFT
    Dp = np.concatenate([D, np.zeros((2, BINS), D.dtype)])
    out = np.zeros((len(steps), BINS), np.complex128)
    acc = np.angle(D[0]).astype(np.float64)
    for t, s in enumerate(steps):
        i = int(s)
        a = s % 1.0
        mag = _lerp(a, np.abs(Dp[i]), np.abs(Dp[i + 1]))
        out[t] = mag * np.exp(1j * acc)
        acc = acc + phi + _dphase(np.angle(Dp[i + 1]), np.angle(Dp[i]), phi)
    return out


def istft_frames(length, available):
    return min(int(available), -(-(int(length) + N_FFT) // HOP))


def istft(S, length):
    """librosa.istft(S, hop 512, center=True, length=length)."""
    S = np.asarray(S)
    nf = istft_frames(length, S.shape[0])
    w = hann()
    fr = np.fft.irfft(S[:nf], n=N_FFT, axis=1) * w[None, :]
    n = N_FFT + HOP * (nf - 1) if nf else 0
    y = np.zeros(max(n, 0))
    wsum = np.zeros(max(n, 0))
    for t in range(nf):
        y[t * HOP:t * HOP + N_FFT] += fr[t]
        wsum[t * HOP:t * HOP + N_FFT] += w * w
    y = _normalise(y, wsum, np.finfo(np.float32).tiny)[PAD:]
    out = np.zeros(int(length))
    m = min(len(y), int(length))
    out[:m] = y[:m]
    return out


def stretch_len(length, rate):
    return int(round(int(length) / float(rate)))


def time_stretch_raw(y, rate):
    return istft(phase_vocoder(stft(y), rate), stretch_len(len(y), rate))


def _taps(rho):
    c = _cutoff(rho)
    return c, LPW / c


def resample_ratio(x, rho, n_out):
    """out[i] = sum_j x[j] h(i / rho - j), h(u) = c sinc(c u) cos^2(pi u c / 12)
    for |u| < 6 / c, c = 0.99 min(1, rho): the ingestion's windowed sinc at an
    arbitrary ratio rho = output rate / input rate."""
    x = np.asarray(x, np.float64)
    c, half = _taps(rho)
    pos = np.arange(int(n_out), dtype=np.float64) / float(rho)
    j0 = np.floor(pos - half).astype(np.int64)
    W = int(math.ceil(2 * half)) + 2
    j = j0[:, None] + np.arange(W)[None, :]
    u = pos[:, None] - j
    h = c * np.sinc(c * u) * np.cos(np.pi * u * c / (2 * LPW)) ** 2
    h[np.abs(u) >= half] = 0.0
    ok = (j >= 0) & (j < len(x))
    xv = np.where(ok, x[np.clip(j, 0, max(len(x) - 1, 0))] if len(x) else 0.0, 0.0)
    return (xv * h).sum(axis=1)


def pitch_rate(steps):
    return 2.0 ** (-float(steps) / 12.0)


def pitch_shift_raw(y, steps):
    r = pitch_rate(steps)
    return resample_ratio(time_stretch_raw(y, r), r, len(y))


def _clip(y):
    return np.clip(y, -1.0, 1.0)


def time_stretch(y, rate):
    return _clip(time_stretch_raw(y, rate))


def pitch_shift(y, steps):
    return _clip(pitch_shift_raw(y, steps))


def time_pitch_shift(y, rate, steps):
    return _clip(pitch_shift_raw(time_stretch_raw(y, rate), steps))


def apply(kind, y, p0, p1=0.0):
    """kind by name; p0 = rate (speed_up, slow_down, time_pitch_shift) or steps
    (pitch_up, pitch_down); p1 = steps of time_pitch_shift."""
    if kind in ('speed_up', 'slow_down'):
        return time_stretch(y, p0)
    if kind in ('pitch_up', 'pitch_down'):
        return pitch_shift(y, p0)
    assert kind == 'time_pitch_shift', kind
    return time_pitch_shift(y, p0, p1)


def out_len(kind, length, p0, p1=0.0):
    return int(length) if kind in ('pitch_up', 'pitch_down') else stretch_len(length, p0)


# ---- how much of a file's head the first n_out output samples depend on
def _stretch_need(rate, n_out, tight=False):
    """Output sample m sits at m + 1024 of the padded overlap-add, so it sums the
    synthesis frames t <= (m + 1024) // 512.  Step t reads the analysis frames
    int(t rate) and int(t rate) + 1 (and, through the accumulator, earlier ones);
    analysis frame f reads the samples below 512 f + 1024.  tight: a synthesis
    frame met at its first sample weighs 0 (periodic Hann), and a whole-numbered
    step does not read its second frame."""
    if n_out <= 0:
        return 0
    p = n_out - 1 + PAD
    t = p // HOP
    if tight and p % HOP == 0 and t > 0:
        t -= 1
    s = t * float(rate)
    f = int(s) + 1
    if tight and s == int(s):
        f -= 1
    return f * HOP + PAD


def _resample_need(rho, n_out):
    """The last output reads x[j] for |(n_out - 1) / rho - j| < 6 / c."""
    if n_out <= 0:
        return 0
    _, half = _taps(rho)
    return max(int(math.ceil((n_out - 1) / float(rho) + half)), 0)


def need_frames(kind, p0, p1, n_out, tight=False):
    """The input frames the first n_out output frames of the kind depend on
    (derived from the frame geometry above; a file may of course be shorter)."""
    if kind in ('speed_up', 'slow_down'):
        return _stretch_need(p0, n_out, tight)
    steps = p0 if kind != 'time_pitch_shift' else p1
    r = pitch_rate(steps)
    n = _stretch_need(r, _resample_need(r, n_out), tight)
    return n if kind != 'time_pitch_shift' else _stretch_need(p0, n, tight)


# ------------------------------------------------------------- float32 twins
_BITREV = np.array([int(format(i, '011b')[::-1], 2) for i in range(N_FFT)])


def _fft_f32(x, inverse=False):
    """Radix-2 decimation in time on [..., 2048] complex64, every butterfly in
    float32 (numpy's own FFT computes in double on many versions)."""
    x = np.asarray(x, np.complex64)[..., _BITREV]
    lead = x.shape[:-1]
    sign = 1.0 if inverse else -1.0
    for s in range(11):
        half = 1 << s
        w = np.exp(sign * 2j * np.pi * np.arange(half) / (2 * half)).astype(np.complex64)
        x = x.reshape(lead + (N_FFT // (2 * half), 2, half))
        a, b = x[..., 0, :], (x[..., 1, :] * w).astype(np.complex64)
        x = np.stack((a + b, a - b), axis=-2).astype(np.complex64).reshape(lead + (N_FFT,))
    return x


def stft_f32(y):
    return _fft_f32(_frames(y, np.float32).astype(np.complex64))[:, :BINS]


def _turns_q32(c):
    t = (np.arctan2(c.imag, c.real).astype(np.float32) * np.float32(1.0 / (2.0 * np.pi))).astype(np.float32)
    return np.round(t.astype(np.float64) * 4294967296.0).astype(np.int64) & 0xFFFFFFFF


def phase_vocoder_f32(D, rate):
    D = np.asarray(D, np.complex64)
    T = D.shape[0]
    steps = np.arange(0, T, rate, dtype=np.float64)
    Dp = np.concatenate([D, np.zeros((2, BINS), np.complex64)])
    q = _turns_q32(Dp)
    mag = np.abs(Dp).astype(np.float32)
    out = np.zeros((len(steps), BINS), np.complex64)
    acc = q[0].copy()
    for t, s in enumerate(steps):
        i = int(s)
        a = np.float32(s - i)
        m = ((np.float32(1) - a) * mag[i] + a * mag[i + 1]).astype(np.float32)
        half_turns = (np.where(acc >= 2 ** 31, acc - 2 ** 32, acc).astype(np.float32) * np.float32(2.0 ** -31))
        ang = half_turns.astype(np.float64) * np.pi
        out[t] = (m * np.cos(ang).astype(np.float32) + 1j * (m * np.sin(ang).astype(np.float32))).astype(np.complex64)
        acc = (acc + q[i + 1] - q[i]) & 0xFFFFFFFF
    return out


def istft_f32(S, length):
    S = np.asarray(S, np.complex64)
    nf = istft_frames(length, S.shape[0])
    w = hann(np.float32)
    full = np.zeros((nf, N_FFT), np.complex64)
    full[:, :BINS] = S[:nf]
    full[:, 0] = full[:, 0].real
    full[:, N_FFT // 2] = full[:, N_FFT // 2].real
    full[:, BINS:] = np.conj(S[:nf, 1:N_FFT // 2][:, ::-1])
    fr = (_fft_f32(full, inverse=True).real * np.float32(1.0 / N_FFT)).astype(np.float32) * w[None, :]
    n = N_FFT + HOP * (nf - 1) if nf else 0
    y = np.zeros(max(n, 0), np.float32)
    wsum = np.zeros(max(n, 0), np.float32)
    for t in range(nf):
        y[t * HOP:t * HOP + N_FFT] += fr[t]
        wsum[t * HOP:t * HOP + N_FFT] += w * w
    ok = wsum > np.finfo(np.float32).tiny
    y[ok] /= wsum[ok]
    y = y[PAD:]
    out = np.zeros(int(length), np.float32)
    m = min(len(y), int(length))
    out[:m] = y[:m]
    return out


def time_stretch_raw_f32(y, rate):
    return istft_f32(phase_vocoder_f32(stft_f32(y), rate), stretch_len(len(y), rate))


def resample_ratio_f32(x, rho, n_out):
    x = np.asarray(x, np.float32)
    c, half = _taps(rho)
    pos = np.arange(int(n_out), dtype=np.float64) / float(rho)
    j0 = np.floor(pos - half).astype(np.int64)
    W = int(math.ceil(2 * half)) + 2
    j = j0[:, None] + np.arange(W)[None, :]
    u64 = pos[:, None] - j
    u = u64.astype(np.float32)
    cf = np.float32(c)
    h = (cf * np.sinc((cf * u).astype(np.float32)).astype(np.float32)
         * np.cos((np.float32(np.pi) * u * cf / np.float32(2 * LPW)).astype(np.float32)).astype(np.float32) ** 2)
    h = h.astype(np.float32)
    h[np.abs(u64) >= half] = 0
    ok = (j >= 0) & (j < len(x))
    xv = np.where(ok, x[np.clip(j, 0, max(len(x) - 1, 0))] if len(x) else np.float32(0), np.float32(0))
    out = np.zeros(int(n_out), np.float32)
    for k in range(W):   # ascending taps, one rounding per tap
        out = (out + xv[:, k].astype(np.float32) * h[:, k]).astype(np.float32)
    return out


def apply_f32(kind, y, p0, p1=0.0):
    y = np.asarray(y, np.float32)
    if kind in ('speed_up', 'slow_down'):
        out = time_stretch_raw_f32(y, p0)
    else:
        if kind == 'time_pitch_shift':
            y, steps = time_stretch_raw_f32(y, p0), p1
        else:
            steps = p0
        r = pitch_rate(steps)
        out = resample_ratio_f32(time_stretch_raw_f32(y, r), r, len(y))
    return np.clip(out, np.float32(-1), np.float32(1))
