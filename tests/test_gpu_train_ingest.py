"""GPU: the trainer's device ingestion (sad_train_ingest_run, csrc/ingest.hip;
sad.ingest.TrainIngest; submodel_trainer.py --device-ingest).

Kernel cases run at seg_len = 640 with every file in ONE batch, so one launch
maps workgroups to mixed files: six sample rates (all three kernel forms), 1-3
channels, int16 and fp32 storage, the three segment rules and their boundary
lengths, files shorter than `need`, pad-rule files at other rates than 32 kHz.

Bars.  (1), (3), (4) are bit-equality.  (2) compares with a float64 evaluation
of the same polyphase sum over float64 mono inputs and the fp32-rounded table;
the a-priori bar per sample is (K + C + 2) * 2^-24 * sum_k |x_k w_k| (an fp32
FMA chain over K taps on inputs that carry the mono stage's C roundings).  A
32 kHz file has no polyphase sum: its bar is the mono stage's own, C - 1
additions and one division, each rounded relative to at most sum_c |x_c| / C:
(C + 1) * 2^-24 * sum_c |x_c| / C.  The largest error / bar ratio per case is
printed, and written to the file named by SAD_TRAIN_INGEST_REPORT when set
(profiles/train_ingest_tests.txt is one such run)."""
import math
import os

import numpy as np
import pytest
import torch

from test_train_ingest_host import SEG, _frames_for, _write_wav

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LO = math.ceil(0.9 * SEG)


def _samples(frames, ch, kind, seed):
    rng = np.random.default_rng(seed)
    if kind == 'i16':
        return rng.integers(-20000, 20000, size=frames * ch).astype(np.int16)
    return (0.3 * rng.standard_normal(frames * ch)).astype(np.float32)


def _case_list():
    """(name, sr, channels, storage, 32 kHz length n); the first and last files are 44.1 kHz."""
    c = [('44k-two-first-in-batch', 44100, 1, 'i16', 2 * SEG + 300),
         ('32k-n=2seg', 32000, 1, 'i16', 2 * SEG),
         ('32k-n=2seg-1', 32000, 1, 'f32', 2 * SEG - 1),
         ('32k-n=seg', 32000, 2, 'i16', SEG),
         ('32k-n=seg-1', 32000, 3, 'f32', SEG - 1),
         ('32k-n=0.9seg', 32000, 1, 'i16', LO),
         ('32k-long-3ch', 32000, 3, 'i16', 5 * SEG),
         ('22k-long-3ch', 22050, 3, 'i16', 6 * SEG),
         ('22k-n=2seg-1', 22050, 1, 'f32', 2 * SEG - 1),
         ('16k-two-2ch', 16000, 2, 'f32', 3 * SEG),
         ('16k-n=seg-1', 16000, 1, 'i16', SEG - 1),
         ('48k-first', 48000, 1, 'i16', SEG + 211),
         ('48k-pad-2ch', 48000, 2, 'f32', 600),
         ('96k-two-3ch', 96000, 3, 'i16', 2 * SEG + 1),
         ('96k-pad', 96000, 1, 'f32', LO),
         ('44k-short-of-need', 44100, 3, 'f32', 2 * SEG + 2),   # two segments, frames < need
         ('44k-pad-2ch', 44100, 2, 'i16', LO + 7)]
    c += [(f'44k-n={n}', 44100, 1, 'i16', n) for n in (2 * SEG, 2 * SEG - 1, SEG, SEG - 1, LO)]
    c += [('44k-two-last-in-batch', 44100, 2, 'i16', 4 * SEG)]
    return c


def _stored(samples, frames, ch, sr, seg, truncate):
    from sad import ingest
    keep = min(frames, ingest.train_need_frames(sr, seg)) if truncate else frames
    return ingest.StoredFile(samples[:keep * ch], frames, ch, sr, 0, torch.zeros(2, 8, dtype=torch.int32))


def _reference_rows(samples, ch, sr, seg):
    """The existing device path on the whole file, sliced by the segment rule."""
    from sad import ingest
    wf, _ = ingest.waveform_from_samples(samples, ch, sr, device=DEV)
    n = wf.shape[0]
    rule = ingest.train_segment_rule(n, seg)
    if rule == 'two':
        return torch.stack((wf[:seg], wf[seg:2 * seg]))
    first = wf[:seg] if rule == 'first' else torch.cat((wf, wf.new_zeros(seg - n)))
    return torch.stack((first, first))


def _frames_upto(n, sr):
    """(frames, length): the longest file at sr whose 32 kHz length is at most n
    (an upsampling rate does not reach every length)."""
    from sad import ingest
    f = n * sr // 32000 + 2
    while ingest.train_out_len(f, sr) > n:
        f -= 1
    return f, ingest.train_out_len(f, sr)


def _build_cases():
    from sad import ingest
    cases = []
    for i, (name, sr, ch, kind, n) in enumerate(_case_list()):
        frames, n_got = _frames_upto(n, sr)
        assert ingest.train_segment_rule(n_got, SEG) == ingest.train_segment_rule(n, SEG) is not None, name
        if sr in (32000, 44100, 48000, 96000):  # every length exists at these rates
            assert n_got == n, name
        cases.append(dict(name=name, sr=sr, ch=ch, kind=kind, n=n_got, frames=frames,
                          x=_samples(frames, ch, kind, 100 + i)))
    assert any(c['frames'] < ingest.train_need_frames(c['sr'], SEG) and c['n'] >= 2 * SEG and c['sr'] != 32000
               for c in cases)
    assert cases[0]['sr'] == cases[-1]['sr'] == 44100
    return cases


@pytest.fixture(scope='module')
def kernel_run():
    from sad import ingest
    cases = _build_cases()
    ti = ingest.TrainIngest(DEV)
    for sr in (44100, 48000, 16000, 22050, 96000, 32000):  # the library's formulas are the mirrored ones
        assert ti.need_frames(sr, SEG) == ingest.train_need_frames(sr, SEG)
    trunc = ingest.collate_stored([_stored(c['x'], c['frames'], c['ch'], c['sr'], SEG, True) for c in cases], SEG)
    whole = ingest.collate_stored([_stored(c['x'], c['frames'], c['ch'], c['sr'], SEG, False) for c in cases], SEG)
    assert trunc.arena.numel() < whole.arena.numel()
    out_t, out_w = ti(trunc), ti(whole)
    ref = torch.cat([_reference_rows(c['x'], c['ch'], c['sr'], SEG) for c in cases])
    torch.cuda.synchronize()
    return dict(cases=cases, ti=ti, out=out_t.cpu(), out_whole=out_w.cpu(), ref=ref.cpu())


def test_bit_identical_with_the_two_kernel_path(kernel_run):
    out, ref = kernel_run['out'], kernel_run['ref']
    assert out.shape == ref.shape == (2 * len(kernel_run['cases']), SEG)
    for f, c in enumerate(kernel_run['cases']):
        assert torch.equal(out[2 * f:2 * f + 2], ref[2 * f:2 * f + 2]), c['name']
        if c['n'] < SEG:  # the pad: exact zeros past n_out, whatever the FIR tail would be
            assert out[2 * f, c['n'] - 1] != 0 and not out[2 * f:2 * f + 2, c['n']:].any(), c['name']
        if c['n'] < 2 * SEG:
            assert torch.equal(out[2 * f], out[2 * f + 1]), c['name']


def test_truncated_upload_equals_whole_file_upload(kernel_run):
    assert torch.equal(kernel_run['out'], kernel_run['out_whole'])


def test_batch_of_one_and_other_batch_orders(kernel_run):
    from sad import ingest
    cases, ti, out = kernel_run['cases'], kernel_run['ti'], kernel_run['out']
    one = ingest.collate_stored([_stored(cases[-1]['x'], cases[-1]['frames'], cases[-1]['ch'], cases[-1]['sr'], SEG,
                                         True)], SEG)
    assert torch.equal(ti(one).cpu(), out[-2:])
    order = list(range(len(cases)))[::-1]
    rev = ingest.collate_stored([_stored(cases[i]['x'], cases[i]['frames'], cases[i]['ch'], cases[i]['sr'], SEG, True)
                                 for i in order], SEG)
    got = ti(rev).cpu().view(len(cases), 2, SEG)
    assert torch.equal(got, out.view(len(cases), 2, SEG)[order])
    seg_rows = ti.segments(one).cpu()  # the host path's row order: first segments, then second segments
    assert torch.equal(seg_rows, out[-2:])


def _float64_rows(c, seg):
    """(rows [M] float64, bars [M]) of file c: the definition in float64."""
    from sad import audio
    ch, sr, n = c['ch'], c['sr'], c['n']
    x = c['x'].astype(np.float64) * (1.0 / 32768.0 if c['kind'] == 'i16' else 1.0)
    x = x.reshape(-1, ch)
    mono = x.sum(axis=1) / ch
    M = 2 * seg if n >= 2 * seg else seg
    m = np.arange(M)
    if sr == 32000:
        val = np.zeros(M)
        bar = np.zeros(M)
        k = min(M, n)
        val[:k] = mono[:k]
        bar[:k] = (ch + 1) * 2.0 ** -24 * np.abs(x[:k]).sum(axis=1) / ch
        return val, bar
    g = math.gcd(sr, 32000)
    kern, width = audio._sinc_resample_kernel(sr, 32000, g)
    kern = kern[:, 0, :].double().numpy()  # [new, K]
    orig, new, K = sr // g, 32000 // g, kern.shape[1]
    j, p = m // new, m % new
    idx = j[:, None] * orig + np.arange(K)[None, :] - width
    ok = (idx >= 0) & (idx < mono.shape[0])
    xk = np.where(ok, mono[np.clip(idx, 0, mono.shape[0] - 1)], 0.0)
    terms = xk * kern[p]
    val = terms.sum(axis=1)
    bar = (K + ch + 2) * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    val[m >= n] = 0.0
    bar[m >= n] = 0.0
    return val, bar


def test_float64_parity(kernel_run):
    lines, worst = [], 0.0
    for f, c in enumerate(kernel_run['cases']):
        val, bar = _float64_rows(c, SEG)
        M = val.shape[0]
        got = kernel_run['out'][2 * f:2 * f + 2].reshape(-1)[:M].double().numpy()
        err = np.abs(got - val)
        assert np.all(got[bar == 0.0] == 0.0), c['name']
        nz = bar > 0
        ratio = float((err[nz] / bar[nz]).max()) if nz.any() else 0.0
        i = int(np.argmax(np.where(nz, err / np.where(nz, bar, 1.0), -1.0)))
        lines.append(f"{c['name']:<26} sr {c['sr']:>6} ch {c['ch']} {c['kind']} n {c['n']:>5} frames {c['frames']:>6}  "
                     f"elements {M:>5}  worst err {err[i]:.3e}  its bar {bar[i]:.3e}  ratio {ratio:.3f}")
        worst = max(worst, ratio)
    text = '\n'.join(lines)
    print('\n' + text)
    path = os.environ.get('SAD_TRAIN_INGEST_REPORT')
    if path:
        with open(path, 'w') as fh:
            fh.write(text + '\n')
    assert worst <= 1.0, text


def test_bit_identical_with_the_host_dataset(kernel_run, tmp_path, monkeypatch):
    """32 kHz mono files, int16 and fp32: the rows are what SpectrogramDataset.__getitem__ returns today."""
    import submodel_trainer as smt
    monkeypatch.setattr(smt, 'SEGMENT_LENGTH', SEG)
    picks = [(f, c) for f, c in enumerate(kernel_run['cases']) if c['sr'] == 32000 and c['ch'] == 1]
    assert {c['kind'] for _, c in picks} == {'i16', 'f32'} and len(picks) >= 3
    d = tmp_path / 'train' / 'Real'
    os.makedirs(d)
    for k, (_, c) in enumerate(picks):
        _write_wav(str(d / f'{k}.wav'), c['x'].reshape(-1, 1), 32000, c['kind'])
    host = smt.SpectrogramDataset(str(tmp_path), 'train', transform='train', class_names=['Real', 'Class1'])
    stored = smt.StoredSampleDataset(str(tmp_path), 'train', transform='train', class_names=['Real', 'Class1'])
    items = [stored[k] for k in range(len(picks))]
    rows = kernel_run['ti'](smt.stored_collate_fn(items)).cpu()
    for k, (f, c) in enumerate(picks):
        s1, _, s2, _, _ = host[k]
        assert torch.equal(rows[2 * k], s1) and torch.equal(rows[2 * k + 1], s2), c['name']
        assert torch.equal(rows[2 * k:2 * k + 2], kernel_run['out'][2 * f:2 * f + 2])


def test_production_shape_and_frontend_handoff():
    """seg_len = 128000: the production indices, and the rows feed TrainFrontEnd.maps."""
    from sad import ingest
    from sad import train as st
    seg = 128000
    spec = [(32000, 1, 'i16', 2 * seg + 4321), (44100, 2, 'i16', 2 * seg + 999), (32000, 1, 'f32', 120000),
            (48000, 1, 'i16', seg + 70001)]
    files, refs = [], []
    for i, (sr, ch, kind, n) in enumerate(spec):
        frames = _frames_for(n, sr) if sr != 32000 else n
        x = _samples(frames, ch, kind, 900 + i)
        files.append(_stored(x, frames, ch, sr, seg, True))
        refs.append(_reference_rows(x, ch, sr, seg))
    ti = ingest.TrainIngest(DEV)
    batch = ingest.collate_stored(files, seg)
    out = ti(batch)
    ref = torch.cat(refs)
    assert torch.equal(out, ref)
    fe = st.TrainFrontEnd(DEV, 'fp32')
    order = [0, 2, 4, 6, 1, 3, 5, 7]
    assert torch.equal(ti.segments(batch), ref[order])
    assert torch.equal(fe.maps(ti.segments(batch)), fe.maps(ref[order].contiguous()))


# ------------------------------------------------------------------- end to end
def _clip_dataset(root, n_train=2, n_test=1):
    from sad import audio as sa
    from sad.synth import synth_labelled_clip
    k = 0
    for mode, n in (('train', n_train), ('test', n_test)):
        for label, cls in enumerate(('Real', 'Class1')):
            d = os.path.join(root, mode, cls)
            os.makedirs(d, exist_ok=True)
            for i in range(n):
                k += 1
                sa.save_pcm16(os.path.join(d, f'{cls}_{i}.wav'), synth_labelled_clip(3, k, label))


def _run_main(smt, monkeypatch, data, ck, flag):
    """One epoch of submodel_trainer.main; returns (epoch loss, final state dict, first-step images)."""
    seen = {}
    real_train, real_images = smt.train, smt.DeviceModel.images

    def spy_train(args, loader, model, *a, **k):
        res = real_train(args, loader, model, *a, **k)
        seen['loss'] = res[0]
        seen['sd'] = {n: v.detach().cpu().clone() for n, v in model.trainer.net.state_dict().items()}
        return res

    def spy_images(self, batch, train):
        img, tg = real_images(self, batch, train)
        if train and 'img' not in seen:
            seen['img'], seen['tg'] = img.detach().cpu().clone(), tg.clone()
        return img, tg

    monkeypatch.setattr(smt, 'train', spy_train)
    monkeypatch.setattr(smt.DeviceModel, 'images', spy_images)
    smt.main(['--data-dir', data, '--epochs', '1', '--batch-size', '2', '--workers', '0', '--precision', 'fp32',
              '--checkpoint-dir', ck] + (['--device-ingest'] if flag else []))
    monkeypatch.setattr(smt, 'train', real_train)
    monkeypatch.setattr(smt.DeviceModel, 'images', real_images)
    return seen


def test_trainer_end_to_end_both_input_paths(tmp_path, monkeypatch):
    """One epoch over 32 kHz mono s16 clips with and without --device-ingest:
    the same images at the first step, the same epoch loss, the same weights
    (and the same model_best.pth when the epoch's validation wrote one)."""
    import submodel_trainer as smt
    monkeypatch.chdir(tmp_path)
    _clip_dataset(str(tmp_path / 'ds'))
    host = _run_main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_host'), False)
    dev = _run_main(smt, monkeypatch, str(tmp_path / 'ds'), str(tmp_path / 'ck_dev'), True)
    assert torch.equal(host['tg'], dev['tg']) and torch.equal(host['img'], dev['img'])
    assert host['loss'] == dev['loss'] and math.isfinite(host['loss'])
    assert list(host['sd']) == list(dev['sd'])
    for name in host['sd']:
        assert torch.equal(host['sd'][name], dev['sd'][name]), name
    pa, pb = tmp_path / 'ck_host' / 'model_best.pth', tmp_path / 'ck_dev' / 'model_best.pth'
    assert pa.exists() == pb.exists()
    if pa.exists():
        a = torch.load(pa, map_location='cpu', weights_only=True)
        b = torch.load(pb, map_location='cpu', weights_only=True)
        assert all(torch.equal(a['state_dict'][n], b['state_dict'][n]) for n in a['state_dict'])
        assert a['best_acc'] == b['best_acc']


def test_mixed_formats_train_with_the_flag(tmp_path, monkeypatch, caplog):
    """A stereo 44.1 kHz file and a 24-bit file train with --device-ingest; the
    host path skips the stereo file with its warning (today's behaviour)."""
    import logging

    import submodel_trainer as smt
    from sad.synth import synth_labelled_clip
    monkeypatch.chdir(tmp_path)
    ds = tmp_path / 'ds'
    _clip_dataset(str(ds), n_train=0, n_test=1)
    a = synth_labelled_clip(4, 1, 0, n=9 * 44100).astype(np.int32)
    b = synth_labelled_clip(4, 2, 1).astype(np.int32)
    _write_wav(str(ds / 'train' / 'Real' / 'stereo44.wav'), np.stack((a, a // 2), axis=1), 44100, 'i16')
    _write_wav(str(ds / 'train' / 'Class1' / 'pcm24.wav'), (b * 256)[:, None], 32000, 'i24')
    caplog.set_level(logging.WARNING)
    dev = _run_main(smt, monkeypatch, str(ds), str(tmp_path / 'ck1'), True)
    assert not [r for r in caplog.records if r.levelno >= logging.WARNING and 'Error' in r.getMessage()]
    assert dev['img'].shape[0] == 4 and math.isfinite(dev['loss']) and dev['loss'] > 0
    caplog.clear()
    host = _run_main(smt, monkeypatch, str(ds), str(tmp_path / 'ck2'), False)
    assert any('expected mono audio, got 2 channels' in r.getMessage() for r in caplog.records)
    assert host['img'].shape[0] == 2
