"""Float64 reference of the trainer's waveform augmentation, with a-priori
rounding bars (no GPU work here; tests/test_waveaug_reference.py checks this
file on the CPU against tests/golden/golden_waveaug.npz, which the reference's
own functions wrote; tests/test_gpu_waveaug_kernel.py compares the kernels of
csrc/waveaug.hip with it).

The contract: six of the eleven kinds of the reference's audio_augmneter.py
(:79-137, and :190 for the clip), stated from the operation.  `y` is the mono
mix of one file, `sr` its stored sample rate, `L` its total frame count.

  original                       y
  dynamic_range_compression(a)   sign(y) |y|^a
  tremolo(rate, depth)           y ((1 - depth) + depth sin(2 pi rate t_i)),
                                 t = linspace(0, L / sr, num=L): t_i = i (L / sr) / (L - 1),
                                 the last one L / sr, t = [0] for L = 1 -- the step
                                 depends on the file's length and is not 1 / sr
  phaser(rate, depth)            lfo_i = depth sin(2 pi rate i / sr); for f0 in 500, 1500,
                                 2500 Hz in this order: w = 2 pi f0 / sr, al = sin(w) / 2,
                                 b = [al, 0, -al], a = [1 + al, -2 cos w, 1 - al],
                                 y_f = lfilter(b, a, y_p) from a zero state at frame 0,
                                 y_p <- y_p + lfo y_f: each stage filters the previous
                                 stage's output.  sr <= 5000 is refused: al <= 0 there
                                 and the pole leaves the unit circle
  time_shift(s)                  s = int(shift sr), truncated toward zero:
                                 out_i = y_{i-s} if s != 0 and 0 <= i - s < L, else 0.
                                 s = 0 gives an all-zero signal, as the reference's
                                 y_shifted[0:] = 0 does (reproduced on purpose)
  add_white_noise(amp, key)      y_i + amp rms n_i; rms over the first n_rms frames (the
                                 frames the trainer reads; the reference takes the whole
                                 file -- the two agree for files no longer than that);
                                 n_i a standard normal of (key, i) alone, see normal()
  every kind                     then clip(., -1, 1)

Not reproduced: the reference's resample to 44.1 kHz before augmenting, its
round trip through a 16-bit stereo file afterwards, and numpy's own normal
generator (the noise is this project's counter-based one).

Bars for an fp32 implementation, u = 2^-24 (one fp32 rounding), per element,
evaluated in float64 and written down before any run (bars()):
  power     |y|^a = exp(a ln|y|): the logarithm's rounding times the exponent, and
            the result's own: u |ref| (4 + 2 a |ln|y||)
  LFO       sin(2 pi t) from a phase t reduced to [-1/2, 1/2] turns in float64 and
            rounded once to fp32: the argument's rounding times the derivative,
            2 pi u |t|, + 3 u |sin| for the sine and the product with depth, + 2^-40
            for the float64 evaluation order of the phase
  tremolo   |y| (d_lfo + u |1 - depth| + u |gain|) + u |out|
  noise     |amp rms n| u (6 + (WA_SUB + 10) / 2) + u |out|: ln, sqrt, cos(2 pi u2) with an
            exact argument and two products; the rms is an fp32 sum of squares of WA_SUB
            terms per lane followed by a 6-level tree, finished in float64
  phaser    per stage, the transposed direct form II recurrence
              y_n = b0 x_n + z1;  z1 <- -a1 y_n + z2;  z2 <- -b0 x_n - a2 y_n
            rounds each of its three results once: an error of u |result| injected at
            frame n reaches later outputs through the recursive part's impulse response
            h; -b0 x_n is a rounded product of its own.  With
            m_n = (|a1| + |a2|) |y_n| + |z1_n| + |z2_n| + |b0 x_n|,
              d_yf = 2 u (|y_f| + (|h| * (m + m0))_{n-1}) + |h_full| * d_x + 2^-126
            where m0 is the same magnitude for the zero-state run of each WA_SUB-frame
            run (the scan's first pass, whose end states carry their own roundings),
            d_x the previous stage's bar, h_full the filter's impulse response, and the
            factor 2 covers the state's conversion to fp32 at each run's start and the
            second-order terms, and 2^-126 the results below fp32's normal range (an
            absolute 2^-150 each, times sum |h| < 2^14 and three stages).  The stage's
            update adds |lfo| d_yf + |y_f| d_lfo + u |y_p|.
            This is tighter than the recurrence run on absolute values and absolute
            coefficients, which it never exceeds (|h| is that recurrence's response).
  original, time_shift   0: these are copies
Every element is compared; none is left out.
"""
import numpy as np
from scipy.signal import fftconvolve, lfilter

U = 2.0 ** -24
KINDS = ('original', 'dynamic_range_compression', 'add_white_noise', 'tremolo', 'phaser', 'time_shift')
UNSUPPORTED = ('speed_up', 'slow_down', 'pitch_up', 'pitch_down', 'time_pitch_shift')
PHASER_F0 = (500.0, 1500.0, 2500.0)
PHASER_MIN_SR = 5000          # al <= 0 at and below this rate
M64 = 0xFFFFFFFFFFFFFFFF
GOLD = 0x9E3779B97F4A7C15


def clip(x):
    return np.clip(np.asarray(x, np.float64), -1.0, 1.0)


def dynamic_range_compression(y, amount):
    y = np.asarray(y, np.float64)
    return np.sign(y) * np.abs(y) ** float(amount)


def tremolo_times(n, sr, L):
    """linspace(0, L / sr, num=L)[:n] without building L values."""
    L = int(L)
    if L == 1:
        return np.zeros(min(n, 1))
    step = (L / sr) / (L - 1)
    t = np.arange(min(n, L), dtype=np.float64) * step
    if n >= L:
        t[L - 1] = L / sr
    return t


def tremolo(y, sr, rate, depth, L=None):
    y = np.asarray(y, np.float64)
    t = tremolo_times(y.shape[0], sr, y.shape[0] if L is None else L)
    return y * ((1 - depth) + depth * np.sin(2 * np.pi * rate * t))


def phaser_coefficients(f0, sr):
    if sr <= PHASER_MIN_SR:
        raise ValueError(f'phaser needs a sample rate above {PHASER_MIN_SR} Hz (got {sr})')
    omega = 2 * np.pi * f0 / sr
    alpha = np.sin(omega) / 2
    return [alpha, 0.0, -alpha], [1 + alpha, -2 * np.cos(omega), 1 - alpha]


def phaser_lfo(n, sr, rate, depth):
    return depth * np.sin(2 * np.pi * rate * (np.arange(n) / sr))


def phaser(y, sr, rate, depth, stage_dtype=np.float64):
    """stage_dtype=np.float32 rounds each stage's result as the reference's
    in-place += into a float32 array does."""
    yp = np.asarray(y, np.float64).copy()
    lfo = phaser_lfo(yp.shape[0], sr, rate, depth)
    for f0 in PHASER_F0:
        b, a = phaser_coefficients(f0, sr)
        yp = (yp + lfo * lfilter(b, a, yp)).astype(stage_dtype).astype(np.float64)
    return yp


def shift_samples(shift, sr):
    return int(shift * sr)


def time_shift(y, s, L=None, n_out=None):
    """y: the frames present (zeros count past them, up to L)."""
    y = np.asarray(y, np.float64)
    L = y.shape[0] if L is None else int(L)
    n_out = L if n_out is None else int(n_out)
    out = np.zeros(n_out)
    if s == 0:
        return out
    i = np.arange(n_out)
    src = i - int(s)
    ok = (src >= 0) & (src < L) & (src < y.shape[0])
    out[ok] = y[src[ok]]
    return out


def mix64(z):
    z = z.astype(np.uint64, copy=True)
    z ^= z >> np.uint64(30)
    z *= np.uint64(0xBF58476D1CE4E5B9)
    z ^= z >> np.uint64(27)
    z *= np.uint64(0x94D049BB133111EB)
    z ^= z >> np.uint64(31)
    return z


def normal_uniforms(key, i):
    """The two uniforms of frame i: the splitmix64 finaliser of key + GOLD (i + 1)
    (the dropout hash of csrc/headtrain.hip); u1 in (0, 1] from its top 24 bits,
    u2 in [0, 1) from bits 16..39."""
    i = np.asarray(i).astype(np.uint64)
    with np.errstate(over='ignore'):
        z = mix64(np.uint64(int(key) & M64) + np.uint64(GOLD) * (i + np.uint64(1)))
    u1 = ((z >> np.uint64(40)).astype(np.float64) + 1.0) * 2.0 ** -24
    u2 = ((z >> np.uint64(16)) & np.uint64(0xFFFFFF)).astype(np.float64) * 2.0 ** -24
    return u1, u2


def normal(key, i):
    """n_i: Box-Muller on normal_uniforms; a function of (key, i) alone."""
    u1, u2 = normal_uniforms(key, i)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)


def rms(y, n_rms=None):
    y = np.asarray(y, np.float64)
    n = y.shape[0] if n_rms is None else int(n_rms)
    return float(np.sqrt(np.mean(y[:n] ** 2))) if n else 0.0


def add_white_noise(y, amp_rel, key, n_rms=None):
    y = np.asarray(y, np.float64)
    return y + amp_rel * rms(y, n_rms) * normal(key, np.arange(y.shape[0]))


def augment(kind, y, sr, L, p0=0.0, p1=0.0, key=0, n_out=None):
    """The first n_out frames of the augmented, clipped file.  y: the mono mix
    of the frames present; p0, p1: (amount) | (amp_rel) | (rate, depth) |
    (rate, depth) | (s)."""
    y = np.asarray(y, np.float64)
    n_out = min(int(L), y.shape[0]) if n_out is None else int(n_out)
    head = y[:n_out]
    if kind == 'original':
        out = head
    elif kind == 'dynamic_range_compression':
        out = dynamic_range_compression(head, p0)
    elif kind == 'add_white_noise':
        out = add_white_noise(head, p0, key, n_out)
    elif kind == 'tremolo':
        out = tremolo(head, sr, p0, p1, L)
    elif kind == 'phaser':
        out = phaser(head, sr, p0, p1)
    elif kind == 'time_shift':
        out = time_shift(y, int(p0), L, n_out)
    else:
        raise ValueError(f'unknown kind {kind!r}; supported: {", ".join(KINDS)}')
    return clip(out)


# ------------------------------------------------------------------------ bars
def _lfo_bar(turns, depth):
    t = turns - np.rint(turns)
    return depth * (U * (2 * np.pi * np.abs(t) + 3 * np.abs(np.sin(2 * np.pi * t))) + 2.0 ** -40)


def _conv(h, x):
    """(h * x)[:n] of non-negative sequences; the FFT's own rounding (relative to the
    largest value) is added, so the result never falls below the true sum."""
    n = x.shape[0]
    if not n:
        return x
    c = np.maximum(fftconvolve(h, x)[:n], 0.0)
    return c + 1e-13 * c.max()


def _stage_magnitudes(b0, a1, a2, x):
    """m_n of a transposed direct form II run from a zero state."""
    yf = lfilter([b0, 0.0, -b0], [1.0, a1, a2], x)
    z2 = -b0 * x - a2 * yf
    z1 = np.append(yf[1:] - b0 * x[1:], -a1 * yf[-1:] + (z2[-2:-1] if x.shape[0] > 1 else 0.0))
    return yf, (abs(a1) + abs(a2)) * np.abs(yf) + np.abs(z1) + np.abs(z2) + np.abs(b0 * x)


def phaser_bar(y, sr, rate, depth, sub):
    yp = np.asarray(y, np.float64).copy()
    n = yp.shape[0]
    dx = np.zeros(n)
    i = np.arange(n)
    lfo = phaser_lfo(n, sr, rate, depth)
    dlfo = _lfo_bar(rate * i / sr, depth)
    imp = np.zeros(n)
    imp[:1] = 1.0
    for f0 in PHASER_F0:
        b, a = phaser_coefficients(f0, sr)
        b0, a1, a2 = b[0] / a[0], a[1] / a[0], a[2] / a[0]
        h = np.abs(lfilter([1.0], [1.0, a1, a2], imp))
        hfull = np.abs(lfilter([b0, 0.0, -b0], [1.0, a1, a2], imp))
        yf, m = _stage_magnitudes(b0, a1, a2, yp)
        m0 = np.concatenate([_stage_magnitudes(b0, a1, a2, yp[c:c + sub])[1] for c in range(0, n, sub)])
        inj = _conv(h, m + m0)
        dyf = 2 * U * (np.abs(yf) + np.append(0.0, inj[:-1])) + _conv(hfull, dx) + 2.0 ** -126
        yp = yp + lfo * yf
        dx = dx + np.abs(lfo) * dyf + np.abs(yf) * dlfo + U * np.abs(yp)
    return dx


def bars(kind, y, sr, L, p0=0.0, p1=0.0, key=0, n_out=None, sub=32):
    """Per-element bar of an fp32 implementation against augment() (module docstring)."""
    y = np.asarray(y, np.float64)
    n_out = min(int(L), y.shape[0]) if n_out is None else int(n_out)
    head = y[:n_out]
    if kind in ('original', 'time_shift'):
        return np.zeros(n_out)
    if kind == 'dynamic_range_compression':
        ref = np.abs(head) ** float(p0)
        ln = np.abs(np.log(np.where(head == 0, 1.0, np.abs(head))))
        return np.where(head == 0, 0.0, U * ref * (4 + 2 * p0 * ln))
    if kind == 'add_white_noise':
        term = np.abs(p0 * rms(head, n_out) * normal(key, np.arange(n_out)))
        return term * U * (6 + (sub + 10) / 2) + U * (np.abs(head) + term)
    if kind == 'tremolo':
        t = tremolo_times(n_out, sr, L)
        gain = (1 - p1) + p1 * np.sin(2 * np.pi * p0 * t)
        return np.abs(head) * (_lfo_bar(p0 * t, p1) + U * abs(1 - p1) + U * np.abs(gain)) + U * np.abs(head * gain)
    if kind == 'phaser':
        return phaser_bar(head, sr, p0, p1, sub)
    raise ValueError(kind)
