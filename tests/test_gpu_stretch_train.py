"""GPU: the time-stretch and pitch-shift kinds inside the trainer's device
ingestion (sad.ingest.TrainIngest with a stretch table; submodel_trainer.py
--device-ingest --wave-stretch): bit-equality with the stage entries and with
the paths that exist without the flag, then two steps of the trainer."""
import math

import numpy as np
import pytest
import torch

from test_gpu_stretch_kernels import compose
from test_gpu_train_ingest import _clip_dataset
from test_gpu_waveaug_train import _pcm, _rows_of_mono

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SEG = 4000
Z = torch.zeros(2, 8, dtype=torch.int32)


def _stored(x, sr, wave):
    """The worker's view of the file: what the drawn kind needs of it."""
    from sad import ingest
    need = ingest.train_need_frames(sr, SEG)
    if wave is not None and wave[0] >= 6:
        need = ingest.stretch_need_frames(wave[0], wave[1], wave[2], need)
    keep = min(x.shape[0], need)
    return ingest.StoredFile(np.ascontiguousarray(x[:keep].reshape(-1)), x.shape[0], x.shape[1], sr, 0, Z, wave)


SPECS = [(8000, 1, 9000), (44100, 2, 30000), (8000, 3, 1500), (44100, 1, 9000), (32000, 2, 2 * SEG + 500),
         (44100, 1, 40000), (8000, 2, 5000)]
WAVES = [(6, 1.37, 0.0, 0), (7, 0.5, 0.0, 0), (8, 2.0, 0.0, 0), (3, 4.5, 0.4, 0), (10, 0.83, -0.5, 0),
         (9, -2.0, 0.0, 0), (4, 0.7, 0.8, 0)]


def test_rows_are_the_stage_entries_then_the_unchanged_ingestion():
    from sad import ingest
    ti = ingest.TrainIngest(DEV)
    xs = [_pcm(n, ch, 70 + i) for i, (_, ch, n) in enumerate(SPECS)]
    files = [_stored(x, sr, w) for x, (sr, _, _), w in zip(xs, SPECS, WAVES)]
    batch = ingest.collate_stored(files, SEG)
    assert batch.stretch_off is not None and batch.wave_off is not None
    rows = ti(batch)
    assert torch.isfinite(rows).all()   # (resampling a clipped head to 32 kHz may overshoot 1: no bound here)
    for f, ((sr, ch, n), w, x) in enumerate(zip(SPECS, WAVES, xs)):
        if w[0] < 6:
            continue
        whole = compose(x, w[0], w[1], w[2])
        head = torch.from_numpy(whole[:int(batch.stretch_table[f, 3])]).to(DEV)
        assert torch.equal(rows[2 * f:2 * f + 2], _rows_of_mono(head, sr, len(whole))), (f, sr, ch, n, w)
    # the files of the six other kinds: as in a batch without any stretch file
    others = [f for f, w in enumerate(WAVES) if w[0] < 6]
    alone = ti(ingest.collate_stored([files[f] for f in others], SEG))
    for i, f in enumerate(others):
        assert torch.equal(rows[2 * f:2 * f + 2], alone[2 * i:2 * i + 2])


def test_a_batch_without_a_stretch_kind_is_the_batch_without_the_flag():
    from sad import ingest
    ti = ingest.TrainIngest(DEV)
    xs = [_pcm(n, ch, 80 + i) for i, (_, ch, n) in enumerate(SPECS)]
    waves = [(3, 4.5, 0.4, 0), None, (0, 0.0, 0.0, 0), (1, 0.3, 0.0, 0), (5, 100.0, 0.0, 0), (2, 0.04, 0.0, 7), None]
    batch = ingest.collate_stored([_stored(x, sr, w) for x, (sr, _, _), w in zip(xs, SPECS, waves)], SEG)
    assert batch.stretch_off is None
    calls = []
    real = ti.wave_stretch
    ti.wave_stretch = lambda *a, **k: calls.append(1) or real(*a, **k)
    rows = ti(batch)
    assert not calls
    mono = ti.wave_augment(batch, batch.arena.to(DEV)).view(torch.float32)
    wt = batch.wave_table
    for f, (sr, _, n) in enumerate(SPECS):
        head = mono[wt[f, 3] // 4:wt[f, 3] // 4 + wt[f, 2]]
        assert torch.equal(rows[2 * f:2 * f + 2], _rows_of_mono(head, sr, n))


def _main(smt, monkeypatch, data, ck, extra):
    from sad import ingest
    seen = {'rows': []}
    real_train, real_call = smt.train, ingest.TrainIngest.__call__

    def spy_train(args, loader, model, *a, **k):
        res = real_train(args, loader, model, *a, **k)
        seen['loss'], seen['steps'] = res[0], res[2]
        return res

    def spy_call(self, batch):
        rows = real_call(self, batch)
        seen['rows'].append((batch.stretch_off is not None, rows.detach().cpu().clone()))
        return rows

    monkeypatch.setattr(smt, 'train', spy_train)
    monkeypatch.setattr(ingest.TrainIngest, '__call__', spy_call)
    smt.main(['--data-dir', data, '--epochs', '1', '--batch-size', '2', '--workers', '0', '--precision', 'fp32',
              '--checkpoint-dir', ck, '--device-ingest', '--max-steps', '2'] + extra)
    monkeypatch.setattr(smt, 'train', real_train)
    monkeypatch.setattr(ingest.TrainIngest, '__call__', real_call)
    return seen


def test_trainer_runs_two_steps_with_every_stretch_kind(tmp_path, monkeypatch):
    import submodel_trainer as smt
    from sad import augment
    monkeypatch.chdir(tmp_path)
    _clip_dataset(str(tmp_path / 'ds'))
    drawn = []
    real = augment.wave_stretch_params
    monkeypatch.setattr(augment, 'wave_stretch_params', lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    aug = _main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_s'), ['--wave-stretch', 'all'])
    print('kinds drawn:', [(augment.STRETCH_KINDS[d[0] - 6], round(d[1], 3), round(d[2], 3)) for d in drawn])
    assert len(drawn) == 4 and all(6 <= d[0] <= 10 for d in drawn)   # one per training file, none for validation
    assert aug['steps'] == 2 and math.isfinite(aug['loss']) and aug['loss'] > 0
    train_rows = [r for s, r in aug['rows'] if s]
    assert len(train_rows) == 2
    for r in train_rows:
        assert torch.isfinite(r).all() and r.abs().max() <= 1.0 and r.abs().max() > 0
    plain = _main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_p'), [])
    assert not any(s for s, _ in plain['rows'])
    val, val_plain = [r for s, r in aug['rows'] if not s], [r for _, r in plain['rows'][plain['steps']:]]
    assert len(val) == len(val_plain) > 0 and all(torch.equal(a, b) for a, b in zip(val, val_plain))
    assert not any(torch.equal(a, b) for a, (_, b) in zip(train_rows, plain['rows']))
