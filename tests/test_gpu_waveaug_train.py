"""GPU: the waveform augmentation inside the trainer's device ingestion
(sad.ingest.TrainIngest with augmentation rows; submodel_trainer.py
--device-ingest --wave-augment).  Everything here is bit-equality: stage one
writes an fp32 mono arena, and the unchanged sad_train_ingest_run reads it."""
import math
import os

import numpy as np
import pytest
import torch

from test_gpu_train_ingest import _clip_dataset

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEG = 4000  # need = 8000 frames at 32 kHz: four chunks of the phaser scan per file
Z = torch.zeros(2, 8, dtype=torch.int32)


def _pcm(frames, ch, seed):
    return np.random.default_rng(seed).integers(-20000, 20000, size=(frames, ch)).astype(np.int16)


def _stored(x, sr, wave, total=None, extra=0):
    """The worker's view of the file: the first min(total, need + extra) frames."""
    from sad import ingest
    total = x.shape[0] if total is None else total
    keep = min(total, ingest.train_need_frames(sr, SEG) + extra)
    return ingest.StoredFile(np.ascontiguousarray(x[:keep].reshape(-1)), total, x.shape[1], sr, 0, Z, wave)


def _specs():
    """(sr, channels, frames): int16 at 32 and 44.1 kHz, mono and stereo, shorter and longer than two segments."""
    from sad import ingest
    need44 = ingest.train_need_frames(44100, SEG)
    return [(32000, 1, 2 * SEG + 3000), (32000, 2, 2 * SEG - 1), (32000, 1, SEG + 17), (32000, 2, 3700),
            (44100, 1, need44 + 4000), (44100, 2, need44 - 300), (44100, 2, 6000), (44100, 1, 5100),
            (32000, 2, 5 * SEG), (44100, 1, 3 * need44), (32000, 1, 2 * SEG), (44100, 2, need44)]


WAVES = [(1, 0.3, 0.0, 0), (2, 0.04, 0.0, 0x5EED), (3, 4.5, 0.4, 0), (4, 0.7, 0.8, 0), (5, -37.0, 0.0, 0),
         (0, 0.0, 0.0, 0), (4, 0.2, 0.6, 0), (5, 211.0, 0.0, 0), (3, 3.1, 0.25, 0), (2, 0.01, 0.0, -9), (1, 0.05, 0.0, 0),
         (4, 1.0, 0.9, 0)]


def _rows_of_mono(wf, sr, total):
    """The existing mono / Resampler / segment path on one fp32 mono head."""
    from sad import ingest
    wf = ingest.mono(wf.contiguous(), 1)
    if sr != 32000:
        wf = ingest.resampler(sr, 32000, DEV)(wf)
    n = ingest.train_out_len(total, sr)
    rule = ingest.train_segment_rule(n, SEG)
    if rule == 'two':
        return torch.stack((wf[:SEG], wf[SEG:2 * SEG]))
    first = wf[:SEG] if rule == 'first' else torch.cat((wf[:n], wf.new_zeros(SEG - n)))
    return torch.stack((first, first))


def test_composition_adds_nothing_and_original_files_equal_the_plain_path():
    from sad import ingest
    ti = ingest.TrainIngest(DEV)
    xs = [_pcm(n, ch, 40 + i) for i, (_, ch, n) in enumerate(_specs())]
    files = [_stored(x, sr, w) for x, (sr, _, _), w in zip(xs, _specs(), WAVES)]
    batch = ingest.collate_stored(files, SEG)
    assert batch.wave_off is not None and {w[0] for w in WAVES} == set(range(6))
    rows = ti(batch)
    mono = ti.wave_augment(batch, batch.arena.to(DEV)).view(torch.float32)
    wt = batch.wave_table
    for f, (sr, ch, n) in enumerate(_specs()):
        head = mono[wt[f, 3] // 4:wt[f, 3] // 4 + wt[f, 2]]
        assert torch.equal(rows[2 * f:2 * f + 2], _rows_of_mono(head, sr, n)), (f, sr, ch, n)
    # every file as 'original', forced through stage one by one phaser file at the end: the rows of today's path
    plain = ti(ingest.collate_stored([_stored(x, sr, None) for x, (sr, _, _) in zip(xs, _specs())], SEG))
    forced = ingest.collate_stored([_stored(x, sr, (0, 0.0, 0.0, 0)) for x, (sr, _, _) in zip(xs, _specs())] +
                                   [_stored(xs[0], 32000, (4, 0.5, 0.5, 0))], SEG)
    assert forced.wave_off is not None
    assert torch.equal(ti(forced)[:-2], plain)
    # and a batch in which every file drew 'original' skips stage one altogether
    allorig = ingest.collate_stored([_stored(x, sr, (0, 0.0, 0.0, 0)) for x, (sr, _, _) in zip(xs, _specs())], SEG)
    assert allorig.wave_off is None and torch.equal(ti(allorig), plain)
    assert torch.equal(ti.segments(batch), rows.view(len(files), 2, SEG).transpose(0, 1).reshape(-1, SEG))
    assert not torch.equal(rows[:10], plain[:10])  # the augmentation did something


def test_the_left_shifts_margin_is_read():
    from sad import ingest
    ti = ingest.TrainIngest(DEV)
    x = _pcm(30000, 1, 5)
    s = int(-0.5 * 32000)
    with_margin = ti(ingest.collate_stored([_stored(x, 32000, (5, float(s), 0.0, 0), extra=16000)], SEG))
    without = ti(ingest.collate_stored([_stored(x, 32000, (5, float(s), 0.0, 0))], SEG))
    shifted = ti(ingest.collate_stored([_stored(x[-s:], 32000, None)], SEG))  # the file that starts 0.5 s later
    assert torch.equal(with_margin, shifted) and with_margin[1, -100:].abs().min() >= 0 and with_margin[1, -100:].any()
    assert not without.any()  # out_i = y_{i + 16000}: none of those frames was read


def _main(smt, monkeypatch, data, ck, extra):
    seen = {}
    real_train = smt.train

    def spy_train(args, loader, model, *a, **k):
        res = real_train(args, loader, model, *a, **k)
        seen['loss'] = res[0]
        seen['steps'] = res[2]
        seen['sd'] = {n: v.detach().cpu().clone() for n, v in model.trainer.net.state_dict().items()}
        seen['kinds'] = getattr(loader.dataset, 'wave_kinds', None)
        return res

    monkeypatch.setattr(smt, 'train', spy_train)
    smt.main(['--data-dir', data, '--epochs', '1', '--batch-size', '2', '--workers', '0', '--precision', 'fp32',
              '--checkpoint-dir', ck, '--device-ingest', '--max-steps', '2'] + extra)
    monkeypatch.setattr(smt, 'train', real_train)
    return seen


def test_trainer_runs_with_every_kind_and_original_alone_changes_nothing(tmp_path, monkeypatch):
    import submodel_trainer as smt
    from sad import augment
    monkeypatch.chdir(tmp_path)
    _clip_dataset(str(tmp_path / 'ds'))
    drawn = []
    real = augment.wave_aug_params
    monkeypatch.setattr(augment, 'wave_aug_params', lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    aug = _main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_all'), ['--wave-augment', 'all'])
    assert aug['kinds'] == augment.WAVE_KINDS and aug['steps'] == 2
    assert math.isfinite(aug['loss']) and aug['loss'] > 0
    assert len(drawn) == 4 and any(d[0] != 0 for d in drawn), drawn  # one draw per training file, none for validation
    plain = _main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_plain'), [])
    orig = _main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_orig'), ['--wave-augment', 'original'])
    assert plain['kinds'] is None and orig['kinds'] == ('original',)
    assert plain['loss'] == orig['loss'] and list(plain['sd']) == list(orig['sd'])
    for name in plain['sd']:
        assert torch.equal(plain['sd'][name], orig['sd'][name]), name
    assert any(not torch.equal(plain['sd'][n], aug['sd'][n]) for n in plain['sd'])
