"""CPU: the float64 contract of the time-stretch and pitch-shift augmentation
(tests/stretch_ref.py) checked against what a stretch and a shift must do, its
need_frames bound, the mutations those checks have to catch, and what the new
entries and the trainer's --wave-stretch decide without a device."""
import ctypes

import numpy as np
import pytest
import torch

import stretch_ref as R

SR = 22050


def _noise(n, seed=0):
    return np.random.default_rng(seed).uniform(-0.5, 0.5, n)


def _tone(freq, n, sr=SR, amp=0.5):
    return amp * np.sin(2 * np.pi * freq * np.arange(n) / sr)


def _peak_hz(y, sr=SR):
    """The spectral peak of the middle half of y (Hann, zero-padded 8 x)."""
    n = len(y)
    mid = y[n // 4:3 * n // 4]
    spec = np.abs(np.fft.rfft(mid * np.hanning(len(mid)), 8 * len(mid)))
    return np.argmax(spec) * sr / (8 * len(mid))


BIN = SR / R.N_FFT   # one analysis bin


def check_identity():
    y = _noise(30000, 1)
    assert np.abs(R.time_stretch(y, 1.0) - y).max() <= 1e-9 * np.abs(y).max()


def check_lengths():
    y = _noise(5000, 2)
    for rate in (0.5, 0.83, 1.37, 1.5):
        assert len(R.time_stretch(y, rate)) == round(5000 / rate)
        assert len(R.time_pitch_shift(y, rate, 0.5)) == round(5000 / rate)
    for steps in (-2, 1):
        assert len(R.pitch_shift(y, steps)) == 5000


def check_tones():
    y = _tone(1000.0, 24000)
    for rate in (0.5, 0.8, 1.5):
        assert abs(_peak_hz(R.time_stretch(y, rate)) - 1000.0) <= BIN, rate
    for steps in (-2, 1, 2):
        assert abs(_peak_hz(R.pitch_shift(y, steps)) - 1000.0 * 2 ** (steps / 12)) <= BIN, steps
    # Two steps up resample by rho = 0.891: the filter's cutoff 0.99 rho / 2 = 0.441 of the
    # stretched signal's rate.  A tone at 0.49 of it lies 11 % above the cutoff, where the
    # Hann-windowed sinc of 6 zero crossings is past the middle of its transition band
    # (gain 1/2 at the cutoff, falling): it must come out below half its amplitude.  Left
    # at 0.495 (no cutoff scaling) the tone would pass and alias.
    rho = R.pitch_rate(2)
    x = _tone(0.49 * SR, 12000)
    out = R.resample_ratio(x, rho, int(12000 * rho) - 20)
    assert np.sqrt(np.mean(out[200:-200] ** 2)) < 0.5 * np.sqrt(np.mean(x ** 2))


CASES = [('slow_down', 0.5, 0.0), ('speed_up', 1.37, 0.0), ('speed_up', 1.5, 0.0), ('pitch_up', 2.0, 0.0),
         ('pitch_down', -2.0, 0.0), ('time_pitch_shift', 0.83, -0.5), ('time_pitch_shift', 1.2, 1.0)]


def check_head_against_whole(cases=CASES):
    y = _noise(30000, 3)
    n_out = 6000
    for kind, p0, p1 in cases:
        whole = R.apply(kind, y, p0, p1)[:n_out]
        need = R.need_frames(kind, p0, p1, n_out)
        assert need < len(y)
        assert np.array_equal(R.apply(kind, y[:need], p0, p1)[:n_out], whole), (kind, p0, p1)
        tight = R.need_frames(kind, p0, p1, n_out, tight=True)
        assert tight <= need
        assert np.array_equal(R.apply(kind, y[:tight], p0, p1)[:n_out], whole), (kind, p0, p1)
        assert not np.array_equal(R.apply(kind, y[:tight - 1], p0, p1)[:n_out], whole), (kind, p0, p1)


def test_identity():
    check_identity()


def test_lengths():
    check_lengths()


def test_tones_keep_or_move_their_peak():
    check_tones()


def test_the_head_need_frames_names_gives_the_whole_files_samples():
    check_head_against_whole()


def test_the_accumulator_is_a_prefix_sum_of_angle_differences_modulo_a_turn():
    D = R.stft(_noise(9000, 4))
    for rate in (0.5, 1.37):
        out = R.phase_vocoder(D, rate)
        steps = np.arange(0, D.shape[0], rate)
        Dp = np.concatenate([D, np.zeros((2, R.BINS))])
        ang = np.angle(Dp)
        i = steps.astype(np.int64)
        acc = ang[0] + np.concatenate([np.zeros((1, R.BINS)), np.cumsum(ang[i + 1] - ang[i], axis=0)[:-1]])
        mag = np.abs(out)
        d = np.angle(out * np.exp(-1j * acc))
        assert np.abs(d[mag > 1e-6 * mag.max()]).max() < 1e-8


def _all_checks():
    check_identity()
    check_lengths()
    check_tones()
    check_head_against_whole(CASES[:1])


@pytest.mark.parametrize('name', ['phase_sign', 'lerp_swapped', 'no_window_sum', 'no_cutoff_scaling'])
def test_the_checks_catch_a_mutated_contract(monkeypatch, name):
    if name == 'phase_sign':
        real = R._dphase
        monkeypatch.setattr(R, '_dphase', lambda a1, a0, phi: real(a0, a1, phi))
    elif name == 'lerp_swapped':
        real = R._lerp
        monkeypatch.setattr(R, '_lerp', lambda a, m0, m1: real(a, m1, m0))
    elif name == 'no_window_sum':
        monkeypatch.setattr(R, '_normalise', lambda y, wsum, tiny: y)
    else:
        monkeypatch.setattr(R, '_cutoff', lambda rho: R.ROLLOFF)
    with pytest.raises(AssertionError):
        _all_checks()


def test_f32_twins_are_close_to_the_contract():
    y = _noise(6000, 5)
    D, Df = R.stft(y), R.stft_f32(y)
    assert np.abs(D - Df).max() <= 1e-5 * np.abs(D).max()
    for rate in (0.5, 1.37):
        ref = R.time_stretch_raw(y, rate)
        assert np.abs(R.time_stretch_raw_f32(y, rate) - ref).max() <= 1e-4 * np.abs(ref).max()
    x = _noise(3000, 6)
    assert np.abs(R.resample_ratio_f32(x, 0.9, 2500) - R.resample_ratio(x, 0.9, 2500)).max() <= 1e-5


def test_host_need_frames_is_the_contracts():
    from sad import augment, ingest
    assert augment.STRETCH_KINDS == R.STRETCH_KINDS
    for k, kind in enumerate(R.STRETCH_KINDS):
        for p0, p1 in ((0.5, -1.0), (0.83, 0.5), (1.0, 0.0), (1.37, 1.0), (1.5, -0.5), (2.0, 2.0), (-2.0, 0.0)):
            if kind in ('speed_up', 'slow_down', 'time_pitch_shift') and p0 <= 0:
                continue
            for n_out in (0, 1, 511, 512, 513, 8000, 352800):
                assert ingest.stretch_need_frames(6 + k, p0, p1, n_out) == R.need_frames(kind, p0, p1, n_out)
            assert ingest.stretch_out_len(6 + k, 12345, p0, p1) == R.out_len(kind, 12345, p0, p1)
    r = augment.STRETCH_RANGES
    assert (r['speed_up'], r['slow_down'], r['pitch_up'], r['pitch_down']) == tuple(R.RANGES[k] for k in R.STRETCH_KINDS[:4])
    assert (r['tps_rate'], r['tps_steps']) == R.RANGES['time_pitch_shift']


# ----------------------------------------------------- the C entries' refusals
def _bits(v):
    return int(np.array([v], np.float64).view(np.int64)[0])


def test_the_stage_entries_refuse_bad_tables():
    from sad import _lib
    lib = _lib.load()
    fake = 0x1000

    def bad(rc, word):
        assert rc == -1 and word in lib.sad_last_error().decode(), (rc, lib.sad_last_error())

    g = [_lib.I32() for _ in range(4)]
    assert lib.sad_wave_stretch_geometry(*[ctypes.byref(v) for v in g]) == 0
    assert [v.value for v in g] == [2048, 512, 64, 17]
    from sad import augment, ingest
    assert [v.value for v in g] == [ingest.STRETCH_N_FFT, ingest.STRETCH_HOP, ingest.STRETCH_CHUNK,
                                    ingest.STRETCH_MAX_LAUNCHES] == [R.N_FFT, R.HOP, 64, 17]
    assert ingest.STRETCH_CODE0 == augment.STRETCH_CODE0 == len(augment.WAVE_KINDS) == 6
    bad(lib.sad_wave_stretch_geometry(None, None, None, None), 'null')

    def run(name, row, in_bytes=1 << 20, out_bytes=1 << 30, ws_bytes=1 << 30, inp=fake, out=fake, ws=fake, n=1,
            table=True):
        t = np.array([row], np.int64)
        args = [inp, in_bytes, t.ctypes.data if table else None, fake if table else None, n, out, out_bytes]
        if name in ('sad_phase_vocoder_run', 'sad_istft2048_run'):
            args += [ws, ws_bytes]
        return getattr(lib, name)(*args, None)

    stft = [0, 1000, 0, 2, 0, 0, 0, 0]
    bad(run('sad_stft2048_run', stft, inp=None), 'null')
    bad(run('sad_stft2048_run', stft, table=False), 'null')
    bad(run('sad_stft2048_run', stft, in_bytes=3999), 'input lies past')
    bad(run('sad_stft2048_run', stft, out_bytes=2 * 1025 * 8 - 1), 'output lies past')
    bad(run('sad_stft2048_run', [8, 1000, 0, 2, 0, 0, 0, 0]), 'multiples of 16')
    bad(run('sad_stft2048_run', [0, -1, 0, 2, 0, 0, 0, 0]), 'counts')
    bad(run('sad_stft2048_run', [0, 1000, 0, 2, 0, 1, 0, 0]), 'flag')
    bad(run('sad_stft2048_run', stft, inp=0x1004), 'aligned')
    bad(run('sad_stft2048_run', stft, n=65536), 'n_files')
    pv = [0, 3, 0, 5, _bits(0.5), 0, 0, 0]
    bad(run('sad_phase_vocoder_run', pv[:4] + [_bits(0.2)] + pv[5:]), 'rate')
    bad(run('sad_phase_vocoder_run', pv[:4] + [_bits(4.5)] + pv[5:]), 'rate')
    bad(run('sad_phase_vocoder_run', pv[:4] + [_bits(float('nan'))] + pv[5:]), 'rate')
    bad(run('sad_phase_vocoder_run', pv, ws=None), 'workspace')
    bad(run('sad_phase_vocoder_run', pv, ws_bytes=3 * 1025 * 8 + 1025 * 4 - 100), 'workspace too small')
    bad(run('sad_phase_vocoder_run', pv, in_bytes=3 * 1025 * 8 - 1), 'input lies past')
    need = _lib.SZ()
    t = np.array([pv, [0, 3, 0, 65, _bits(0.5), 0, 0, 0]], np.int64)
    assert lib.sad_phase_vocoder_workspace_size(t.ctypes.data, 2, ctypes.byref(need)) == 0
    al = lambda v: -(-v // 16) * 16  # noqa: E731
    assert need.value == 2 * al(3 * 1025 * 8) + al(1025 * 4) + al(2 * 1025 * 4)
    ist = [0, 5, 0, 1000, 0, 1, 0, 0]
    bad(run('sad_istft2048_run', ist, ws_bytes=5 * 2048 * 4 - 16), 'workspace too small')
    bad(run('sad_istft2048_run', ist, out_bytes=3999), 'output lies past')
    bad(run('sad_istft2048_run', ist[:5] + [2, 0, 0]), 'flag')
    t = np.array([ist, [0, 50, 0, 1000, 0, 0, 0, 0]], np.int64)
    assert lib.sad_istft2048_workspace_size(t.ctypes.data, 2, ctypes.byref(need)) == 0
    assert need.value == (5 + 6) * 2048 * 4   # ceil((1000 + 2048) / 512) = 6 of the 50 frames are read
    bad(lib.sad_istft2048_workspace_size(t.ctypes.data, 2, None), 'null')
    rs = [0, 1000, 0, 900, _bits(0.9), 1, 0, 0]
    bad(run('sad_resample_ratio_run', rs[:4] + [_bits(5.0)] + rs[5:]), 'rate')
    bad(run('sad_resample_ratio_run', rs, in_bytes=3999), 'input lies past')
    bad(run('sad_resample_ratio_run', rs, out_bytes=3599), 'output lies past')
    t2 = np.array([rs, rs], np.int64)   # two files on one output
    bad(lib.sad_resample_ratio_run(fake, 1 << 20, t2.ctypes.data, fake, 2, fake, 1 << 20, None), 'overlap')
    for name in ('sad_stft2048_run', 'sad_resample_ratio_run'):
        assert getattr(lib, name)(None, 0, None, None, 0, None, 0, None) == 0   # nothing to do


def test_the_batch_entry_refuses_bad_tables():
    from sad import _lib
    lib = _lib.load()
    fake = 0x1000

    def bad(rc, word):
        assert rc == -1 and word in lib.sad_last_error().decode(), (rc, lib.sad_last_error())

    good_file = [0, 3000, 5000, 1, 0, 0]
    good = [6, _bits(1.25), 0, 2000, 0, 0, 0, 0]

    def run(file=good_file, row=good, arena=fake, arena_bytes=1 << 16, mono=fake, mono_bytes=1 << 16, ws=fake,
            ws_bytes=1 << 30, tables=True, d_tables=True, n_files=1):
        ft, st = np.array([file], np.int64), np.array([row], np.int64)
        return lib.sad_wave_stretch_run(arena, arena_bytes, ft.ctypes.data if tables else None,
                                        fake if d_tables else None, n_files, st.ctypes.data if tables else None,
                                        fake if d_tables else None, mono, mono_bytes, ws, ws_bytes, None)

    def row(**kw):
        cols = dict(kind=0, rate=1, steps=2, n_out=3, off=4, prate=5)
        r = list(good)
        for k, v in kw.items():
            r[cols[k]] = v
        return r

    bad(run(arena=None), 'null')
    bad(run(mono=None), 'null')
    bad(run(tables=False), 'null')
    bad(run(d_tables=False), 'null')
    bad(run(ws=None), 'workspace')
    bad(run(ws_bytes=64), 'workspace too small')
    bad(run(ws=0x1008), 'aligned')
    bad(run(row=row(kind=11)), 'kind')
    bad(run(row=row(kind=-1)), 'kind')
    bad(run(row=row(rate=_bits(0.2))), 'rate')
    bad(run(row=row(rate=_bits(4.01))), 'rate')
    bad(run(row=row(rate=_bits(float('nan')))), 'rate')
    bad(run(row=row(kind=8, steps=_bits(12.5), prate=_bits(2 ** (-12.5 / 12)))), 'steps')
    bad(run(row=row(kind=8, steps=_bits(2.0), prate=_bits(0.9))), 'pitch rate')
    bad(run(row=row(kind=10, rate=_bits(5.0), steps=_bits(1.0), prate=_bits(2 ** (-1 / 12)))), 'rate')
    bad(run(row=row(n_out=4001)), 'frames out')          # round(5000 / 1.25) = 4000
    bad(run(row=row(kind=8, steps=_bits(2.0), prate=_bits(2 ** (-2 / 12)), n_out=5001)), 'frames out')
    bad(run(row=row(n_out=-1)), 'frames out')
    bad(run(row=row(off=8)), 'multiple of 16')
    bad(run(mono_bytes=7999), 'too small')
    bad(run(file=[8, 3000, 5000, 1, 0, 0]), 'multiple of 16')
    bad(run(file=[0, 3000, 5000, 0, 0, 0]), 'channels')
    bad(run(file=[0, 3000, 5000, 1, 2, 0]), 'encoding')
    bad(run(file=[0, 6000, 5000, 1, 0, 0]), 'frames read')
    bad(run(arena_bytes=5999), 'past the end of the arena')
    bad(run(n_files=65536), 'n_files')
    need = _lib.SZ()
    ft, st = np.array([good_file], np.int64), np.array([good], np.int64)
    assert lib.sad_wave_stretch_workspace_size(ft.ctypes.data, st.ctypes.data, 1, ctypes.byref(need)) == 0
    assert need.value > 7 * 64
    bad(lib.sad_wave_stretch_workspace_size(ft.ctypes.data, st.ctypes.data, 1, None), 'null')
    # nothing to do: no file, or only files of the other entry
    assert run(n_files=0, tables=False, d_tables=False, arena=None, mono=None, ws=None) == 0
    assert run(row=row(kind=3), arena=None, mono=None, ws=None, d_tables=False) == 0


# ---------------------------------------------------------- parser and draws
def test_cli_parser(capsys):
    import submodel_trainer as smt
    from sad import augment

    def err(argv):
        with pytest.raises(SystemExit) as e:
            smt.parse_args(argv)
        assert e.value.code == 2
        return capsys.readouterr().err

    assert '--device-ingest' in err(['--wave-stretch', 'all'])
    msg = err(['--device-ingest', '--wave-stretch', 'speed_up,reverb'])
    assert 'reverb' in msg and all(k in msg for k in augment.STRETCH_KINDS)
    assert '--wave-augment' in err(['--device-ingest', '--wave-stretch', 'tremolo'])
    assert 'supported' in err(['--device-ingest', '--wave-stretch', ','])
    a = smt.parse_args(['--device-ingest', '--wave-stretch', 'all'])
    assert a.wave_stretch == augment.STRETCH_KINDS and a.wave_augment is None
    a = smt.parse_args(['--device-ingest', '--wave-stretch', 'pitch_down, speed_up', '--wave-augment', 'phaser'])
    assert a.wave_stretch == ('speed_up', 'pitch_down') and a.wave_augment == ('phaser',)
    assert smt.parse_args(['--device-ingest']).wave_stretch is None and smt.parse_args([]).wave_stretch is None
    assert '--wave-stretch' in err(['--device-ingest', '--wave-augment', 'speed_up'])  # the refusal points to the flag


def test_draws_cover_the_union_and_stay_in_the_ranges():
    from sad import augment
    g = torch.Generator().manual_seed(7)
    seen = {}
    for _ in range(2000):
        kind, p0, p1, key = augment.wave_stretch_params(augment.WAVE_KINDS, augment.STRETCH_KINDS, 44100, g)
        name = (augment.WAVE_KINDS + augment.STRETCH_KINDS)[kind]
        seen.setdefault(name, []).append((p0, p1))
    assert set(seen) == set(augment.WAVE_KINDS) | set(augment.STRETCH_KINDS)
    assert all(100 < len(v) < 270 for v in seen.values())   # uniform over 11: 182 +- 6 sigma (12.9)
    for name in ('speed_up', 'slow_down', 'pitch_up', 'pitch_down'):
        lo, hi = R.RANGES[name]
        assert all(lo <= p0 <= hi and p1 == 0.0 for p0, p1 in seen[name]), name
        assert max(p0 for p0, _ in seen[name]) - min(p0 for p0, _ in seen[name]) > 0.8 * (hi - lo)
    (rlo, rhi), (slo, shi) = R.RANGES['time_pitch_shift']
    assert all(rlo <= p0 <= rhi and slo <= p1 <= shi for p0, p1 in seen['time_pitch_shift'])
    # the stretch kinds alone; and time_pitch_shift draws its rate before its steps
    g = torch.Generator().manual_seed(9)
    assert {augment.wave_stretch_params(None, augment.STRETCH_KINDS, 8000, g)[0] for _ in range(300)} == set(range(6, 11))
    g = torch.Generator().manual_seed(5)
    _, p0, p1, _ = augment.wave_stretch_params(None, ('time_pitch_shift',), 44100, g)
    g = torch.Generator().manual_seed(5)
    a = torch.empty(1).uniform_(0.8, 1.2, generator=g).item()
    b = torch.empty(1).uniform_(-1.0, 1.0, generator=g).item()
    assert (p0, p1) == (a, b)


def test_without_the_flag_the_draws_are_todays():
    from sad import augment
    g1, g2 = torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)
    for _ in range(200):
        assert augment.wave_stretch_params(augment.WAVE_KINDS, None, 44100, g1) == \
            augment.wave_aug_params(augment.WAVE_KINDS, 44100, g2)
    assert torch.equal(g1.get_state(), g2.get_state())
    # pinned: the first draws of seed 21, recorded from wave_aug_params of the commit before --wave-stretch existed
    g = torch.Generator().manual_seed(21)
    assert [augment.wave_aug_params(augment.WAVE_KINDS, 44100, g) for _ in range(12)] == BEFORE_WAVE_STRETCH


BEFORE_WAVE_STRETCH = [
    (3, 4.84079647064209, 0.20362190902233124, 0), (4, 0.32842549681663513, 0.7269542813301086, 0),
    (2, 0.03085760958492756, 0.0, -5424767459647638942), (1, 0.08078248798847198, 0.0, 0), (0, 0.0, 0.0, 0),
    (0, 0.0, 0.0, 0), (0, 0.0, 0.0, 0), (5, 16638.0, 0.0, 0), (1, 0.20569036900997162, 0.0, 0),
    (3, 5.430495738983154, 0.3502882122993469, 0), (0, 0.0, 0.0, 0), (2, 0.0063690426759421825, 0.0, 5008472707362821094)]


def test_the_dataset_reads_what_the_drawn_kind_needs(monkeypatch, tmp_path):
    import submodel_trainer as smt
    from sad import augment, ingest
    from test_train_ingest_host import SEG, _pcm, _write_wav
    from test_waveaug_args import _tree
    monkeypatch.setattr(smt, 'SEGMENT_LENGTH', SEG)
    frames = _tree(tmp_path, frames=(6 * SEG, 6 * SEG + 10, 5 * SEG))
    ds = smt.StoredSampleDataset(str(tmp_path), 'train', transform='train', class_names=['Real', 'Class1'])
    assert ds.stretch_kinds is None
    plain = []
    for i in range(len(frames)):
        torch.manual_seed(50 + i)
        plain.append(ds[i])
    ds.stretch_kinds = augment.STRETCH_KINDS
    need = ingest.train_need_frames(32000, SEG)
    for i in range(len(frames)):
        torch.manual_seed(50 + i)
        f = ds[i]
        assert torch.equal(f.aug, plain[i].aug)   # the SpecAugment and crop draws come first, as without the flag
        assert 6 <= f.wave[0] <= 10
        assert f.frames_read == min(frames[i], ingest.stretch_need_frames(f.wave[0], f.wave[1], f.wave[2], need))
    os_tree = tmp_path / 'test' / 'Real'
    os_tree.mkdir(parents=True)
    _write_wav(str(os_tree / 'v.wav'), _pcm(2 * SEG, 1, 9), 32000)
    args = smt.parse_args(['--data-dir', str(tmp_path), '--workers', '0', '--device-ingest', '--wave-stretch', 'all'])
    tr, va = smt.get_dataloaders(args)
    assert tr.dataset.stretch_kinds == augment.STRETCH_KINDS and va.dataset.stretch_kinds is None
    assert tr.dataset.wave_kinds is None and va.dataset.wave_kinds is None


def test_collate_splits_the_batch_into_the_two_tables():
    from sad import _lib, ingest
    from test_train_ingest_host import SEG, _pcm
    z = torch.zeros(2, 8, dtype=torch.int32)
    need = ingest.train_need_frames(32000, SEG)
    a = ingest.StoredFile(_pcm(9000, 2, 1).reshape(-1), 9000, 2, 32000, 0, z, (6, 1.5, 0.0, 0))
    b = ingest.StoredFile(_pcm(1000, 1, 2).reshape(-1), 1000, 1, 32000, 1, z, (3, 4.0, 0.3, 0))
    c = ingest.StoredFile(_pcm(5 * SEG, 1, 3).reshape(-1), 5 * SEG, 1, 32000, 1, z, (10, 0.8, 1.0, 0))
    batch = ingest.collate_stored([a, b, c], SEG)
    st, wt, mt = batch.stretch_table, batch.wave_table, batch.mono_table
    assert batch.stretch_off % 16 == 0 and batch.stretch_off > batch.mono_table_off
    na, nc = min(6000, need), min(round(5 * SEG / 0.8), need)
    offs = [0, ingest._align(4 * na), ingest._align(4 * na) + 4000]
    assert st[:, 0].tolist() == [6, 0, 10] and wt[:, 0].tolist() == [0, 3, 0]
    assert wt[:, 2].tolist() == [0, 1000, 0] and st[:, 3].tolist() == [na, 0, nc]
    assert wt[:, 3].tolist() == offs and st[0, 4].item() == offs[0] and st[2, 4].item() == offs[2]
    assert st[0, 1].item() == _bits(1.5) and st[2, 1].item() == _bits(0.8) and st[2, 2].item() == _bits(1.0)
    assert st[2, 5].item() == _bits(2.0 ** (-1.0 / 12.0)) and st[0, 5].item() == _bits(0.0)
    assert mt.tolist() == [[offs[0], na, 6000, 1, _lib.SAD_PCM_F32, 0], [offs[1], 1000, 1000, 1, _lib.SAD_PCM_F32, 0],
                           [offs[2], nc, round(5 * SEG / 0.8), 1, _lib.SAD_PCM_F32, 0]]
    assert batch.table[:, 2].tolist() == [9000, 1000, 5 * SEG]   # the stored-sample table keeps the files' own lengths
    # no stretch kind in the batch: the upload of today, byte for byte
    plain = ingest.collate_stored([ingest.StoredFile(f.samples, f.frames, f.channels, f.sr, f.target, f.aug, (3, 4.0, 0.3, 0))
                                   for f in (a, b, c)], SEG)
    assert plain.stretch_off is None
