"""CPU: what the waveform augmentation decides without a device: the C entry's
refusals (sad_wave_augment_run checks its host tables before any device work),
the trainer's --wave-augment parser errors, and the per-file draws
(sad.augment.wave_aug_params, StoredSampleDataset, collate_stored)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from test_train_ingest_host import SEG, _pcm, _write_wav


def _f32bits(p0, p1=0.0):
    lo, hi = np.array([p0, p1], np.float32).view(np.uint32).astype(np.uint64)
    return int(np.array([lo | (hi << np.uint64(32))], np.uint64).view(np.int64)[0])


def test_the_c_entry_refuses_bad_tables():
    from sad import _lib, ingest
    lib = _lib.load()
    fake = 0x1000  # a non-null "device" pointer: the checks return before any device work

    def bad(rc, word):
        assert rc == -1 and word in lib.sad_last_error().decode(), (rc, lib.sad_last_error())

    chunk, sub = _lib.I32(), _lib.I32()
    assert lib.sad_wave_augment_geometry(ctypes.byref(chunk), ctypes.byref(sub)) == 0
    assert (chunk.value, sub.value) == (ingest.WAVE_CHUNK, ingest.WAVE_SUB) and chunk.value == 64 * sub.value
    bad(lib.sad_wave_augment_geometry(None, ctypes.byref(sub)), 'null')

    good_file = [0, 100, 1500, 1, 0, 0]
    good_aug = [0, 32000, 100, 0, _f32bits(0.3), 0, 0, 0]

    def run(file=good_file, aug=good_aug, arena=fake, arena_bytes=4096, mono=fake, mono_bytes=4096, ws=fake,
            ws_bytes=1 << 20, tables=True, d_tables=True, n_files=1):
        ft, at = np.array([file], np.int64), np.array([aug], np.int64)
        return lib.sad_wave_augment_run(arena, arena_bytes, ft.ctypes.data if tables else None,
                                        fake if d_tables else None, n_files, at.ctypes.data if tables else None,
                                        fake if d_tables else None, mono, mono_bytes, ws, ws_bytes, None)

    def aug(**kw):
        cols = dict(kind=0, sr=1, n_out=2, off=3, params=4, key=5, base=6)
        row = list(good_aug)
        for k, v in kw.items():
            row[cols[k]] = v
        return row

    bad(run(arena=None), 'null')
    bad(run(mono=None), 'null')
    bad(run(tables=False), 'null')
    bad(run(d_tables=False), 'null')
    bad(run(ws=None, aug=aug(kind=4)), 'workspace')
    bad(run(aug=aug(kind=6)), 'kind')
    bad(run(aug=aug(kind=-1)), 'kind')
    bad(run(aug=aug(kind=4, sr=5000)), 'phaser')
    bad(run(aug=aug(kind=4, sr=4000)), 'phaser')
    bad(run(aug=aug(sr=0)), 'sample rate')
    bad(run(aug=aug(off=8)), 'multiple of 16')
    bad(run(file=[8, 100, 1500, 1, 0, 0]), 'multiple of 16')
    bad(run(mono_bytes=399), 'too small')
    bad(run(aug=aug(off=4096)), 'too small')
    bad(run(file=[0, 100, 1500, 0, 0, 0]), 'channels')
    bad(run(file=[0, 100, 1500, 65, 0, 0]), 'channels')
    bad(run(file=[0, 100, 1500, 1, 2, 0]), 'encoding')
    bad(run(file=[0, 3000, 1500, 1, 0, 0]), 'frames read')
    bad(run(arena_bytes=199), 'past the end of the arena')
    bad(run(aug=aug(n_out=1501)), 'frames out')
    bad(run(aug=aug(kind=1, params=_f32bits(0.0))), 'exponent')
    bad(run(aug=aug(kind=1, params=_f32bits(float('nan')))), 'finite')
    bad(run(aug=aug(kind=5, params=_f32bits(2.5))), 'whole number')
    bad(run(aug=aug(base=1)), 'column 6')
    bad(run(ws_bytes=8, aug=aug(kind=4)), 'workspace too small')
    bad(run(n_files=65536), 'n_files')
    need = _lib.SZ()
    at = np.array([aug(n_out=ingest.WAVE_CHUNK + 1), aug(n_out=1)], np.int64)
    assert lib.sad_wave_augment_workspace_size(at.ctypes.data, 2, ctypes.byref(need)) == 0
    assert need.value == 3 * (16 + 16 + 8 + 64 * 8)
    bad(lib.sad_wave_augment_workspace_size(at.ctypes.data, 2, None), 'null')
    assert run(n_files=0, tables=False, d_tables=False, arena=None, mono=None) == 0  # nothing to do


def test_cli_parser_errors(capsys):
    import submodel_trainer as smt
    from sad import augment

    def err(argv):
        with pytest.raises(SystemExit) as e:
            smt.parse_args(argv)
        assert e.value.code == 2
        return capsys.readouterr().err

    assert '--device-ingest' in err(['--wave-augment', 'all'])
    msg = err(['--device-ingest', '--wave-augment', 'tremolo,reverb'])
    assert 'reverb' in msg and all(k in msg for k in augment.WAVE_KINDS)
    for name in augment.WAVE_UNSUPPORTED:
        msg = err(['--device-ingest', '--wave-augment', f'phaser,{name}'])
        assert name in msg and 'not supported' in msg and all(k in msg for k in augment.WAVE_KINDS)
    assert 'supported' in err(['--device-ingest', '--wave-augment', ','])
    assert len(augment.WAVE_UNSUPPORTED) == 5 and len(augment.WAVE_KINDS) == 6
    assert smt.parse_args(['--device-ingest', '--wave-augment', 'all']).wave_augment == augment.WAVE_KINDS
    assert smt.parse_args(['--device-ingest', '--wave-augment', 'phaser, original']).wave_augment == \
        ('original', 'phaser')
    assert smt.parse_args(['--device-ingest']).wave_augment is None and smt.parse_args([]).wave_augment is None


def test_draws_are_in_the_reference_ranges():
    from sad import augment
    g = torch.Generator().manual_seed(11)
    seen = {}
    for _ in range(3000):
        kind, p0, p1, key = augment.wave_aug_params(augment.WAVE_KINDS, 44100, g)
        seen.setdefault(augment.WAVE_KINDS[kind], []).append((p0, p1, key))
    assert set(seen) == set(augment.WAVE_KINDS)
    assert all(350 < len(v) < 650 for v in seen.values())  # uniform over six kinds: 500 +- 6 sigma (20.4)
    rng = lambda name, col: (min(r[col] for r in seen[name]), max(r[col] for r in seen[name]))  # noqa: E731
    assert all(r == (0.0, 0.0, 0) for r in seen['original'])
    lo, hi = rng('dynamic_range_compression', 0)
    assert 0.01 <= lo < 0.05 and 0.45 < hi <= 0.5
    lo, hi = rng('add_white_noise', 0)
    assert 0.001 <= lo < 0.005 and 0.045 < hi <= 0.05
    assert len({r[2] for r in seen['add_white_noise']}) == len(seen['add_white_noise'])  # a fresh key each
    assert any(r[2] < 0 for r in seen['add_white_noise']) and any(r[2] > 2 ** 62 for r in seen['add_white_noise'])
    lo, hi = rng('tremolo', 0)
    assert 3.0 <= lo < 3.2 and 5.8 < hi <= 6.0
    lo, hi = rng('tremolo', 1)
    assert 0.2 <= lo < 0.22 and 0.48 < hi <= 0.5
    lo, hi = rng('phaser', 0)
    assert 0.1 <= lo < 0.15 and 0.95 < hi <= 1.0
    lo, hi = rng('phaser', 1)
    assert 0.5 <= lo < 0.52 and 0.88 < hi <= 0.9
    lo, hi = rng('time_shift', 0)
    assert -22050 <= lo < -21000 and 21000 < hi <= 22050 and all(r[0] == int(r[0]) for r in seen['time_shift'])
    # a rate at which the phaser is refused draws among the other kinds; alone it falls back to the original
    g = torch.Generator().manual_seed(3)
    kinds = {augment.wave_aug_params(augment.WAVE_KINDS, 4000, g)[0] for _ in range(400)}
    assert kinds == {0, 1, 2, 3, 5}
    assert augment.wave_aug_params(('phaser',), 5000, g)[0] == 0


def test_phaser_draws_depth_before_rate_and_tremolo_rate_before_depth():
    from sad import augment
    for name, first, second in (('phaser', 'ph_depth', 'ph_rate'), ('tremolo', 'trem_rate', 'trem_depth')):
        g = torch.Generator().manual_seed(5)
        _, p0, p1, _ = augment.wave_aug_params((name,), 44100, g)
        g = torch.Generator().manual_seed(5)  # (a one-kind list draws no kind)
        a = torch.empty(1).uniform_(*augment.WAVE_RANGES[first], generator=g).item()
        b = torch.empty(1).uniform_(*augment.WAVE_RANGES[second], generator=g).item()
        assert (p1, p0) == (a, b) if name == 'phaser' else (p0, p1) == (a, b)


def _tree(tmp_path, sr=32000, frames=(2 * SEG + 2000, 2 * SEG + 10, SEG + 3)):
    d = tmp_path / 'train' / 'Real'
    os.makedirs(d)
    for i, n in enumerate(frames):
        _write_wav(str(d / f'{i}.wav'), _pcm(n, 1 + i % 2, i), sr)
    return frames


def test_specaugment_and_crop_draws_do_not_move_and_no_draw_without_the_flag(monkeypatch, tmp_path):
    import submodel_trainer as smt
    from sad import augment, ingest
    monkeypatch.setattr(smt, 'SEGMENT_LENGTH', SEG)
    frames = _tree(tmp_path)
    ds = smt.StoredSampleDataset(str(tmp_path), 'train', transform='train', class_names=['Real', 'Class1'])
    assert ds.wave_kinds is None
    calls = []
    real = augment.wave_aug_params
    monkeypatch.setattr(augment, 'wave_aug_params', lambda *a, **k: calls.append(a) or real(*a, **k))
    plain, state_plain = [], []
    for i in range(len(frames)):
        torch.manual_seed(100 + i)
        plain.append(ds[i])
        state_plain.append(torch.get_rng_state())
    assert not calls and all(f.wave is None for f in plain)  # the flag absent: not one extra draw
    ds.wave_kinds = augment.WAVE_KINDS
    need = ingest.train_need_frames(32000, SEG)
    for i in range(len(frames)):
        torch.manual_seed(100 + i)
        f = ds[i]
        assert torch.equal(f.aug, plain[i].aug)  # same SpecAugment masks and crop from the same state
        assert not torch.equal(torch.get_rng_state(), state_plain[i])
        assert f.wave is not None and 0 <= f.wave[0] < 6
        assert f.frames_read == min(frames[i], need + 16000)  # the left shift's margin is read
        assert np.array_equal(f.samples[:plain[i].samples.shape[0]], plain[i].samples)
    assert len(calls) == len(frames)
    ds.wave_kinds = ('tremolo', 'phaser')
    assert ds[0].frames_read == min(frames[0], need)  # no time_shift in the list: today's read
    # validation is never augmented
    os.makedirs(tmp_path / 'test' / 'Real')
    _write_wav(str(tmp_path / 'test' / 'Real' / 'v.wav'), _pcm(2 * SEG, 1, 9), 32000)
    args = smt.parse_args(['--data-dir', str(tmp_path), '--workers', '0', '--device-ingest', '--wave-augment', 'all'])
    tr, va = smt.get_dataloaders(args)
    assert tr.dataset.wave_kinds == augment.WAVE_KINDS and va.dataset.wave_kinds is None


def test_collate_packs_the_augmentation_rows_into_the_upload():
    from sad import _lib, ingest
    z = torch.zeros(2, 8, dtype=torch.int32)
    need = ingest.train_need_frames(44100, SEG)
    a = ingest.StoredFile(_pcm(need + 500, 2, 1).reshape(-1), 9000, 2, 44100, 0, z, (5, -300.0, 0.0, 0))
    b = ingest.StoredFile(_pcm(1000, 1, 2).reshape(-1), 1000, 1, 32000, 1, z, (2, 0.25, 0.0, -2))
    c = ingest.StoredFile(_pcm(2 * SEG, 1, 3).reshape(-1), 5000, 1, 32000, 1, z, None)
    batch = ingest.collate_stored([a, b, c], SEG)
    assert batch.wave_off % 16 == 0 and batch.mono_table_off % 16 == 0 and batch.wave_off >= batch.tiles_off
    wt, mt = batch.wave_table, batch.mono_table
    offs = [0, ingest._align(4 * need), ingest._align(4 * need) + 4000]
    assert wt[:, :4].tolist() == [[5, 44100, need, offs[0]], [2, 32000, 1000, offs[1]], [0, 32000, 2 * SEG, offs[2]]]
    assert wt[:, 6].tolist() == [0, ingest.wave_chunks(need), ingest.wave_chunks(need) + 1] and not wt[:, 7].any()
    assert wt[0, 4].item() == _f32bits(-300.0) and wt[1, 4].item() == _f32bits(0.25) and wt[1, 5].item() == -2
    assert mt.tolist() == [[offs[0], need, 9000, 1, _lib.SAD_PCM_F32, 0], [offs[1], 1000, 1000, 1, _lib.SAD_PCM_F32, 1],
                           [offs[2], 2 * SEG, 5000, 1, _lib.SAD_PCM_F32, 1]]
    assert batch.mono_bytes == offs[2] + 4 * 2 * SEG
    assert batch.table[0, 1].item() == need + 500  # the margin stays in the stored-sample table
    # every file 'original' (or no draw at all): the plain batch, byte for byte
    plain = ingest.collate_stored([ingest.StoredFile(f.samples, f.frames, f.channels, f.sr, f.target, f.aug)
                                   for f in (a, b, c)], SEG)
    orig = ingest.collate_stored([ingest.StoredFile(f.samples, f.frames, f.channels, f.sr, f.target, f.aug,
                                                    (0, 0.0, 0.0, 0)) for f in (a, b, c)], SEG)
    assert plain.wave_off is None and orig.wave_off is None and torch.equal(plain.arena, orig.arena)
    assert torch.equal(batch.arena[:plain.arena.numel()], plain.arena)


def test_original_alone_draws_nothing():
    from sad import augment
    g = torch.Generator().manual_seed(1)
    state = g.get_state()
    assert augment.wave_aug_params(('original',), 32000, g) == (0, 0.0, 0.0, 0)
    assert torch.equal(g.get_state(), state)
