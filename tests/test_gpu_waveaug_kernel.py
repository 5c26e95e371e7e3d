"""GPU: the waveform augmentation kernels (sad_wave_augment_run, csrc/waveaug.hip)
against the float64 contract of tests/waveaug_ref.py, over every element.

The grid -- every kind x int16 / fp32 x 1-3 channels x 8, 32, 44.1 and 192 kHz x
lengths 1, 2, 3, chunk - 1, chunk, chunk + 1 and 3 chunk + 1 (and the same
around the run a lane walks serially) -- runs as ONE batch, so one launch maps
workgroups to mixed files; the special cases ride in the same batch.  The bars
are waveaug_ref.bars(): a priori, per element, in float64 (its docstring
derives them); a bar of 0 demands equality.  The worst error / bar per kind
and rate is printed, and written to the file named by SAD_WAVEAUG_REPORT when
set (profiles/waveaug_tests_ratios.txt is one such run)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import waveaug_ref as wr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RATES = (8000, 32000, 44100, 192000)
KEY = 0x0123456789ABCDEF


def _params(kind, sr, i):
    """fp32-exact parameters inside the reference's ranges, varied with i."""
    f = lambda v: float(np.float32(v))  # noqa: E731
    k = i % 5
    return {'original': (0.0, 0.0), 'dynamic_range_compression': (f(0.01 + 0.12 * k), 0.0),
            'add_white_noise': (f(0.001 + 0.012 * k), 0.0), 'tremolo': (f(3.0 + 0.7 * k), f(0.2 + 0.07 * k)),
            'phaser': (f(0.1 + 0.22 * k), f(0.5 + 0.1 * k)),
            'time_shift': (float((-1) ** i * (1 + 7 * k)), 0.0)}[kind]


def _signal(frames, ch, fmt, seed, scale=0.45):
    rng = np.random.default_rng(seed)
    if fmt == 'i16':
        return np.clip(np.rint(scale * 32768 * rng.standard_normal((frames, ch))), -32768, 32767).astype(np.int16)
    return (scale * rng.standard_normal((frames, ch))).astype(np.float32)


def _mono32(x):
    """ti_mono's value in numpy fp32: channels summed in order, then a true division."""
    x = np.asarray(x)
    s = x.astype(np.float32) * np.float32(1.0 / 32768.0 if x.dtype == np.int16 else 1.0)
    m = s[:, 0].copy()
    for c in range(1, s.shape[1]):
        m = m + s[:, c]
    return m if s.shape[1] == 1 else m / np.float32(s.shape[1])


def _file(name, x, sr, kind, p0=0.0, p1=0.0, key=KEY, total=None, n_out=None):
    x = np.asarray(x)
    total = x.shape[0] if total is None else total
    return dict(name=name, x=x, sr=sr, kind=kind, p0=p0, p1=p1, key=key, total=total,
                n_out=min(x.shape[0], total) if n_out is None else n_out)


def _grid(chunk, sub):
    files = []
    lengths = (1, 2, 3, chunk - 1, chunk, chunk + 1, 3 * chunk + 1)
    i = 0
    for kind in wr.KINDS:
        for fmt in ('i16', 'f32'):
            for ch in (1, 2, 3):
                for sr in RATES:
                    for n in lengths:
                        i += 1
                        p0, p1 = _params(kind, sr, i)
                        files.append(_file(f'{kind}-{fmt}-{ch}ch-{sr}-n{n}', _signal(n, ch, fmt, i), sr, kind, p0, p1,
                                           key=KEY + i))
    for n in (sub - 1, sub, sub + 1, 3 * sub + 1, chunk + sub, 2 * chunk - 1):  # the seams of a lane's run
        for sr in RATES:
            i += 1
            files.append(_file(f'phaser-run-seam-{sr}-n{n}', _signal(n, 1, 'f32', i), sr, 'phaser', *_params('phaser', sr, i)))
    return files


def _special(chunk, sub):
    files = []
    n = 3 * chunk + 1
    imp = np.zeros((n, 1), np.float32)
    imp[[chunk - 1, chunk, 2 * chunk + sub], 0] = (1.0, -0.5, 0.75)         # impulses on the seams
    step = np.zeros((n, 1), np.float32)
    step[chunk:, 0] = 0.5                                                   # the step's edge on a chunk seam
    sq = np.where((np.arange(n) // chunk) % 2 == 0, 32767, -32768).astype(np.int16)[:, None]  # full scale
    sq2 = np.where((np.arange(n) // sub) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None]     # edges on run seams
    for nm, x in (('impulse', imp), ('step', step), ('square-chunk', sq), ('square-run', sq2)):
        for k, kind in enumerate(wr.KINDS):
            for sr in (8000, 44100):
                files.append(_file(f'{nm}-{kind}-{sr}', x, sr, kind, *_params(kind, sr, k + 2)))
    # the power at |y| = 0, 1/32768 and 1; the clip at outputs of exactly +-1
    edge = np.array([0, 1, -1, 32767, -32768, 0, 16384], np.int16)[:, None]
    for a in (0.01, 0.3, 0.5):
        files.append(_file(f'power-edges-{a}', edge, 32000, 'dynamic_range_compression', float(np.float32(a))))
    files.append(_file('clip-i16', edge, 32000, 'original'))
    big = np.array([1.0, -1.0, 1.5, -2.0, 0.99999994, -1.0000001, 0.0], np.float32)[:, None]
    files.append(_file('clip-f32', big, 32000, 'original'))
    files.append(_file('clip-f32-tremolo', big, 32000, 'tremolo', 3.0, 0.5))
    # shifts 0, +-1, +-int(0.5 sr), |s| >= the frames present
    for sr, n in ((8000, 5000), (44100, 2 * chunk + 77)):
        x = _signal(n, 2, 'i16', sr)
        for s in (0, 1, -1, int(0.5 * sr), -int(0.5 * sr), n, -n, n + 5, -(n + 5), n - 1, -(n - 1)):
            files.append(_file(f'shift-{sr}-s{s}', x, sr, 'time_shift', float(s)))
    # a file present only in part: total > frames present; the left shift reads the margin past n_out
    x = _signal(chunk + 500, 2, 'i16', 77)
    for k, kind in enumerate(wr.KINDS):
        files.append(_file(f'partial-{kind}', x, 44100, kind, *_params(kind, 44100, k), total=10 * chunk, n_out=chunk + 100))
    files.append(_file('partial-left-shift-into-margin', x, 44100, 'time_shift', -300.0, total=10 * chunk, n_out=chunk + 100))
    files.append(_file('partial-left-shift-past-margin', x, 44100, 'time_shift', -450.0, total=10 * chunk, n_out=chunk + 100))
    files.append(_file('partial-right-shift', x, 44100, 'time_shift', 300.0, total=10 * chunk, n_out=chunk + 100))
    return files


def _run(files, serial=False):
    """sad_wave_augment_run (or the serial phaser yardstick) on the files as one
    batch -> [fp32 numpy [n_out]] per file."""
    from sad import _lib, ingest
    n = len(files)
    ft, at = np.zeros((n, 6), np.int64), np.zeros((n, 8), np.int64)
    off = moff = chunks = 0
    for i, f in enumerate(files):
        x = f['x']
        ft[i] = (off, x.shape[0], f['total'], x.shape[1], _lib.SAD_PCM_I16 if x.dtype == np.int16 else _lib.SAD_PCM_F32, 0)
        prm = np.array([f['p0'], f['p1']], np.float32).view(np.uint32).astype(np.uint64)
        at[i, :4] = (wr.KINDS.index(f['kind']), f['sr'], f['n_out'], moff)
        at[i, 4:6] = np.array([prm[0] | (prm[1] << np.uint64(32)), f['key']], np.uint64).view(np.int64)
        at[i, 6] = chunks
        off = ingest._align(off + x.nbytes)
        moff = ingest._align(moff + 4 * f['n_out'])
        chunks += ingest.wave_chunks(f['n_out'])
    buf = np.zeros(off + ft.nbytes + at.nbytes, np.uint8)
    for row, f in zip(ft, files):
        buf[row[0]:row[0] + f['x'].nbytes] = f['x'].reshape(-1).view(np.uint8)
    buf[off:off + ft.nbytes] = ft.reshape(-1).view(np.uint8)
    buf[off + ft.nbytes:] = at.reshape(-1).view(np.uint8)
    d = torch.from_numpy(buf).to(DEV)
    need = _lib.SZ()
    _lib.call('sad_wave_augment_workspace_size', at.ctypes.data, n, ctypes.byref(need))
    assert need.value == chunks * (16 + 16 + 8 + 64 * 8)
    mono = torch.full((max(moff, 16) // 4,), float('nan'), device=DEV)
    ws = torch.empty(max(need.value, 16), device=DEV, dtype=torch.uint8)
    base = d.data_ptr()
    with torch.cuda.device(DEV):
        if serial:
            _lib.call('sad_wave_phaser_serial_run', base, off, ft.ctypes.data, base + off, n, at.ctypes.data,
                      base + off + ft.nbytes, mono.data_ptr(), moff, _lib.stream_handle(DEV))
        else:
            _lib.call('sad_wave_augment_run', base, off, ft.ctypes.data, base + off, n, at.ctypes.data,
                      base + off + ft.nbytes, mono.data_ptr(), moff, ws.data_ptr(), need.value,
                      _lib.stream_handle(DEV))
    out = mono.cpu().numpy()
    return [out[at[i, 3] // 4:at[i, 3] // 4 + f['n_out']].copy() for i, f in enumerate(files)]


@pytest.fixture(scope='module')
def batch():
    from sad import _lib, ingest
    chunk, sub = _lib.I32(), _lib.I32()
    _lib.call('sad_wave_augment_geometry', ctypes.byref(chunk), ctypes.byref(sub))
    assert (chunk.value, sub.value) == (ingest.WAVE_CHUNK, ingest.WAVE_SUB)
    files = _grid(chunk.value, sub.value) + _special(chunk.value, sub.value)
    assert len(files) < 65536
    out = _run(files)
    return dict(files=files, out=out, chunk=chunk.value, sub=sub.value)


def test_float64_parity_over_every_element(batch):
    worst, lines = {}, []
    failures = []
    for f, got in zip(batch['files'], batch['out']):
        y = _mono32(f['x']).astype(np.float64)
        ref = wr.augment(f['kind'], y, f['sr'], f['total'], f['p0'], f['p1'], f['key'], f['n_out'])
        bar = wr.bars(f['kind'], y, f['sr'], f['total'], f['p0'], f['p1'], f['key'], f['n_out'], sub=batch['sub'])
        assert got.shape == ref.shape == bar.shape == (f['n_out'],) and np.isfinite(got).all(), f['name']
        err = np.abs(got.astype(np.float64) - ref)
        ratio = np.where(bar > 0, err / np.where(bar > 0, bar, 1.0), np.where(err > 0, np.inf, 0.0))
        r = float(ratio.max())
        key = (f['kind'], f['sr'])
        if r >= worst.get(key, (-1.0,))[0]:
            i = int(ratio.argmax())
            worst[key] = (r, f['name'], float(err[i]), float(bar[i]), i)
        if r > 1.0:
            failures.append((f['name'], r))
    for (kind, sr), (r, name, e, b, i) in sorted(worst.items()):
        lines.append(f'{kind:<26} sr {sr:>6}  worst error / bar {r:.3f}  (error {e:.3e}, bar {b:.3e}, frame {i} of {name})')
    text = '\n'.join(lines)
    print('\n' + text)
    path = os.environ.get('SAD_WAVEAUG_REPORT')
    if path:
        with open(path, 'w') as fh:
            fh.write(f'{len(batch["files"])} files in one batch, {sum(f["n_out"] for f in batch["files"])} elements, '
                     'every one compared\n' + text + '\n')
    assert not failures, failures[:10]


def test_the_cases_exercise_what_they_claim(batch):
    by = {f['name']: (f, o) for f, o in zip(batch['files'], batch['out'])}
    f, o = by['clip-i16']
    assert o.tolist() == [0.0, 1 / 32768, -1 / 32768, 32767 / 32768, -1.0, 0.0, 0.5]
    assert by['clip-f32'][1].tolist() == [1.0, -1.0, 1.0, -1.0, np.float32(0.99999994), -1.0, 0.0]
    for a in (0.01, 0.3, 0.5):
        o = by[f'power-edges-{a}'][1]
        assert o[0] == 0.0 and o[5] == 0.0 and o[4] == -1.0 and o[1] == -o[2] > 0  # 0 -> 0, -1 -> -1, odd
    assert any(np.abs(o).max() == 1.0 for f, o in zip(batch['files'], batch['out']) if f['kind'] == 'phaser')
    for sr, n in ((8000, 5000), (44100, 2 * batch['chunk'] + 77)):
        assert not by[f'shift-{sr}-s0'][1].any() and not by[f'shift-{sr}-s{n}'][1].any()
        assert not by[f'shift-{sr}-s{-n - 5}'][1].any()
        assert by[f'shift-{sr}-s{n - 1}'][1][-1] != 0 and not by[f'shift-{sr}-s{n - 1}'][1][:-1].any()
    f, o = by['partial-left-shift-into-margin']
    assert o[-1] != 0  # frames past n_out that were read
    assert not by['partial-left-shift-past-margin'][1][-50:].any()  # frames that were not read count as 0


def test_original_is_the_mono_mix_then_the_clip_bit_for_bit(batch):
    from sad import ingest
    seen = 0
    for f, got in zip(batch['files'], batch['out']):
        if f['kind'] != 'original':
            continue
        pcm = torch.from_numpy(np.ascontiguousarray(f['x'].reshape(-1))).to(DEV)
        ref = ingest.mono(pcm, f['x'].shape[1]).clamp(-1.0, 1.0).cpu().numpy()[:f['n_out']]
        assert np.array_equal(got, ref), f['name']
        seen += 1
    assert seen >= 2 * 3 * 4 * 7


def test_a_file_alone_equals_the_file_inside_the_batch_and_runs_repeat(batch):
    files, out = batch['files'], batch['out']
    again = _run(files)
    assert all(np.array_equal(a, b, equal_nan=False) for a, b in zip(out, again))
    n_long = 3 * batch['chunk'] + 1
    picks = {}
    for i, f in enumerate(files):  # the longest file of every kind and rate, and every partial one
        if f['n_out'] == n_long and f['x'].shape[1] == 2:
            picks.setdefault((f['kind'], f['sr']), i)
        if f['name'].startswith('partial-'):
            picks[f['name']] = i
    assert len(picks) >= 6 * 4 + 6
    for i in picks.values():
        assert np.array_equal(_run([files[i]])[0], out[i]), files[i]['name']
    order = list(picks.values())[::-1]  # another batch composition and order
    for i, got in zip(order, _run([files[i] for i in order])):
        assert np.array_equal(got, out[i]), files[i]['name']


def test_the_serial_yardstick_computes_the_same_phaser(batch):
    """sad_wave_phaser_serial_run (one thread per file; what tools/bench_wave_augment.py
    times the scan against) is an fp32 evaluation of the same contract: within the bar."""
    picks = [(f, o) for f, o in zip(batch['files'], batch['out'])
             if f['kind'] == 'phaser' and f['n_out'] > batch['chunk']][::7]
    others = [f for f in batch['files'] if f['kind'] == 'tremolo'][:2]
    assert len(picks) >= 8
    got = _run([f for f, _ in picks] + others, serial=True)
    for (f, scan), ser in zip(picks, got):
        y = _mono32(f['x']).astype(np.float64)
        ref = wr.augment('phaser', y, f['sr'], f['total'], f['p0'], f['p1'], f['key'], f['n_out'])
        bar = wr.bars('phaser', y, f['sr'], f['total'], f['p0'], f['p1'], f['key'], f['n_out'], sub=batch['sub'])
        assert np.all(np.abs(ser.astype(np.float64) - ref) <= bar), f['name']
    assert all(np.isnan(o).all() for o in got[len(picks):])  # the other kinds are left alone
