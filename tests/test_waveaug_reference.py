"""CPU: the float64 contract of the waveform augmentation (tests/waveaug_ref.py)
against tests/golden/golden_waveaug.npz, which the reference's own functions
wrote (tests/golden/make_golden_waveaug.py).

Bars, stated before the comparison, from the reference's own fp32 storage
(u = 2^-24 bounds a half-ulp of an fp32 value v by u |v|):
  time_shift   0: a copy.
  tremolo      the reference computes it in float64 from the same formula: only
               float64 evaluation order, 2^-45.
  dynamic_range_compression
               the reference evaluates |y| ** amount in fp32 (libm's powf, within
               1 ulp) on an fp32 array and stores fp32; the contract is exact in
               float64: 2 ulp = 4 u |out|.
  phaser       each stage's y_p += lfo y_f is computed in float64 and stored into an
               fp32 array: u |y_p| per stage, carried through the later stages by
               d <- d + |lfo| (|h| * d) + u |y_p| with h the stage filter's impulse
               response; + 2^-45.  With the stage rounding restated
               (stage_dtype=float32) the distance is 0.
"""
import os

import numpy as np
import pytest
from scipy.signal import lfilter

import waveaug_ref as wr

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_waveaug.npz')
U = 2.0 ** -24
F64 = 2.0 ** -45


@pytest.fixture(scope='module')
def gold():
    fx = np.load(GOLD)
    p = {k[6:]: float(fx[k]) for k in fx.files if k.startswith('param_')}
    sigs = {str(n): (int(fx[f'{n}/sr']), fx[f'{n}/y'].astype(np.float64)) for n in fx['names']}
    return fx, p, sigs


def _phaser_storage_bar(y, sr, rate, depth):
    yp = np.asarray(y, np.float64).copy()
    n = yp.shape[0]
    lfo = np.abs(wr.phaser_lfo(n, sr, rate, depth))
    imp = np.zeros(n)
    imp[:1] = 1.0
    d = np.zeros(n)
    for f0 in wr.PHASER_F0:
        b, a = wr.phaser_coefficients(f0, sr)
        h = np.abs(lfilter(b, a, imp))
        yp = yp + wr.phaser_lfo(n, sr, rate, depth) * lfilter(b, a, yp)
        d = d + lfo * np.convolve(h, d)[:n] + U * np.abs(yp)
    return d + F64


def _distances(fx, p, sigs, mod=wr):
    """[(label, worst distance / bar, worst distance)] over every signal and kind; a bar of 0 demands equality."""
    rows = []

    def add(label, got, want, bar):
        err = np.abs(got - want.astype(np.float64))
        bar = np.broadcast_to(bar, err.shape)
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
        rows.append((label, float(ratio.max()) if err.size else 0.0, float(err.max()) if err.size else 0.0))

    for name, (sr, y) in sigs.items():
        L = y.shape[0]
        out = mod.augment('dynamic_range_compression', y, sr, L, p['amount'])
        add(f'{name}/drc', out, fx[f'{name}/dynamic_range_compression'], 4 * U * np.abs(out))
        add(f'{name}/tremolo', mod.augment('tremolo', y, sr, L, p['trem_rate'], p['trem_depth']),
            fx[f'{name}/tremolo'], F64)
        add(f'{name}/phaser', mod.augment('phaser', y, sr, L, p['ph_rate'], p['ph_depth']), fx[f'{name}/phaser'],
            _phaser_storage_bar(y, sr, p['ph_rate'], p['ph_depth']))
        for k, s in enumerate(fx['shifts']):
            add(f'{name}/time_shift{k}', mod.augment('time_shift', y, sr, L, wr.shift_samples(float(s), sr)),
                fx[f'{name}/time_shift{k}'], 0.0)
    return rows


def test_contract_matches_the_reference_fixture(gold):
    rows = _distances(*gold)
    print()
    for label, ratio, err in rows:
        print(f'{label:<28} distance {err:.3e}  distance / bar {ratio:.3f}')
    assert len(rows) == 5 * (3 + 6)
    assert all(r <= 1.0 for _, r, _ in rows), [x for x in rows if x[1] > 1.0]
    # the fixture exercises what it claims to
    fx, _, sigs = gold
    assert any(np.abs(fx[f'{n}/phaser']).max() == 1.0 for n in sigs), 'no clipped phaser output in the fixture'
    assert {wr.shift_samples(float(s), 32000) for s in fx['shifts']} >= {0, 320, -320}


def test_phaser_with_the_stage_rounding_is_exact(gold):
    fx, p, sigs = gold
    for name, (sr, y) in sigs.items():
        got = wr.clip(wr.phaser(y, sr, p['ph_rate'], p['ph_depth'], stage_dtype=np.float32))
        assert np.array_equal(got, fx[f'{name}/phaser'].astype(np.float64)), name


def test_exact_cases():
    y = np.linspace(-0.9, 0.9, 11)
    assert not wr.augment('time_shift', y, 8000, 11, 0).any()                       # s = 0: all zeros
    assert wr.shift_samples(1e-6, 44100) == 0 and wr.shift_samples(-1e-6, 44100) == 0
    assert wr.shift_samples(-0.49999, 8000) == -3999                                 # truncation toward zero
    assert np.array_equal(wr.augment('time_shift', y, 8000, 11, 3), np.concatenate((np.zeros(3), y[:8])))
    assert np.array_equal(wr.augment('time_shift', y, 8000, 11, -3), np.concatenate((y[3:], np.zeros(3))))
    assert not wr.augment('time_shift', y, 8000, 11, 11).any() and not wr.augment('time_shift', y, 8000, 11, -40).any()
    # a left shift reads the margin past n_out, and zeros past the frames present
    assert np.array_equal(wr.augment('time_shift', y, 8000, 20, -3, n_out=9), np.concatenate((y[3:], [0.0])))
    one = np.array([0.625])
    for kind, p0, p1 in (('tremolo', 4.5, 0.4), ('phaser', 0.7, 0.8), ('dynamic_range_compression', 0.3, 0.0)):
        assert wr.augment(kind, one, 32000, 1, p0, p1).shape == (1,)
    assert wr.augment('tremolo', one, 32000, 1, 4.5, 0.4)[0] == 0.625 * (1 - 0.4)   # t = [0]
    assert np.array_equal(wr.tremolo_times(7, 44100, 7), np.linspace(0, 7 / 44100, num=7))
    assert np.array_equal(wr.tremolo_times(5, 44100, 9), np.linspace(0, 9 / 44100, num=9)[:5])
    assert np.array_equal(wr.augment('original', 2 * y, 8000, 11), np.clip(2 * y, -1, 1))
    with pytest.raises(ValueError):
        wr.augment('phaser', y, 5000, 11, 0.5, 0.5)
    with pytest.raises(ValueError):
        wr.augment('speed_up', y, 8000, 11)


def test_noise_generator_statistics():
    N = 1 << 20
    n = wr.normal(0x1234ABCD5678EF01, np.arange(N))
    se = 1.0 / np.sqrt(N)
    mean, var = n.mean(), n.var()
    kurt = ((n - mean) ** 4).mean() / var ** 2
    acs = [float((n[:-k] * n[k:]).mean() / var) for k in range(1, 9)]
    print(f'\nmean {mean:.3e} (6 se {6 * se:.3e})  var-1 {var - 1:.3e} (6 se {6 * np.sqrt(2.0 / N):.3e})  '
          f'kurt-3 {kurt - 3:.3e} (6 se {6 * np.sqrt(24.0 / N):.3e})  max |ac| {max(map(abs, acs)):.3e}')
    assert abs(mean) <= 6 * se
    assert abs(var - 1) <= 6 * np.sqrt(2.0 / N)
    assert abs(kurt - 3) <= 6 * np.sqrt(24.0 / N)
    assert all(abs(a) <= 6 * se for a in acs)
    assert np.isfinite(n).all()
    other = wr.normal(0x1234ABCD5678EF02, np.arange(N))
    assert abs(float((n * other).mean())) <= 6 * se and (n != other).mean() > 0.99
    # n_i is a function of (key, i): any cut of the range gives the same values
    cuts = [0, 1, 63, 64, 4097, 300000, N]
    parts = [wr.normal(0x1234ABCD5678EF01, np.arange(a, b)) for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(np.concatenate(parts), n)
    assert np.array_equal(wr.normal(0x1234ABCD5678EF01, np.arange(N)[::-1])[::-1], n)


def test_white_noise_uses_the_rms_of_the_frames_read():
    rng = np.random.default_rng(5)
    y = 0.2 * rng.standard_normal(500)
    got = wr.add_white_noise(y[:300], 0.05, 77, 300)
    assert np.array_equal(got, y[:300] + 0.05 * np.sqrt(np.mean(y[:300] ** 2)) * wr.normal(77, np.arange(300)))


# ------------------------------------------------------------------- sharpness
class _Mutant:
    """waveaug_ref with one function replaced."""

    def __init__(self, **repl):
        self._repl = repl

    def __getattr__(self, name):
        return self._repl.get(name, getattr(wr, name))

    def augment(self, kind, y, sr, L, p0=0.0, p1=0.0, key=0, n_out=None):
        y = np.asarray(y, np.float64)
        fn = self._repl.get(kind)
        if fn is None:
            return wr.augment(kind, y, sr, L, p0, p1, key, n_out)
        return fn(y, sr, L, p0, p1)


def _trem_step_is_one_over_sr(y, sr, L, rate, depth):
    return wr.clip(y * ((1 - depth) + depth * np.sin(2 * np.pi * rate * np.arange(L) / sr)))


def _phaser_parallel(y, sr, L, rate, depth):
    lfo = wr.phaser_lfo(L, sr, rate, depth)
    out = y.copy()
    for f0 in wr.PHASER_F0:
        out = out + lfo * lfilter(*wr.phaser_coefficients(f0, sr), y)
    return wr.clip(out)


def _phaser_lfo_before_filter(y, sr, L, rate, depth):
    lfo = wr.phaser_lfo(L, sr, rate, depth)
    yp = y.copy()
    for f0 in wr.PHASER_F0:
        yp = yp + lfilter(*wr.phaser_coefficients(f0, sr), lfo * yp)
    return wr.clip(yp)


def _shift_wraps(y, sr, L, s, _):
    return wr.clip(np.roll(y, int(s))) if int(s) else np.zeros(L)


MUTANTS = {
    'tremolo step 1/sr': dict(tremolo=_trem_step_is_one_over_sr),
    'phaser stages in parallel': dict(phaser=_phaser_parallel),
    'phaser LFO before the filter': dict(phaser=_phaser_lfo_before_filter),
    'time shift wraps around': dict(time_shift=_shift_wraps),
    'no clip': dict(phaser=lambda y, sr, L, r, d: wr.phaser(y, sr, r, d)),
}


@pytest.mark.parametrize('name', list(MUTANTS))
def test_mutated_contracts_fail_the_fixture(gold, name):
    rows = _distances(*gold, mod=_Mutant(**MUTANTS[name]))
    bad = [r for r in rows if r[1] > 1.0]
    print(f'\n{name}: {len(bad)} of {len(rows)} comparisons fail, worst distance {max(r[2] for r in rows):.3e}')
    assert bad, name
