"""GPU: StreamBank end to end on the catalogue-scan folder, n6 fixture model.

Every readable file is fed chunk by chunk (37 ms and 1 s), all files in one
bank at once so their windows share batches, each file in two slots (one closed
plain, one with smoothing).  The yardstick is the whole-file path:
inference_runner.main for the records and the events' times and labels,
ingest.select_windows + inference_runner.run_windows for the merged logits.
Every comparison is exact.
"""
import json

import numpy as np
import pytest
import torch

import scan_catalogue as cat

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PRECISIONS = ['fp32', 'bf16']


@pytest.fixture(scope='module')
def setup(tmp_path_factory):
    import inference_runner as ir
    from sad import audio
    root = tmp_path_factory.mktemp('stream')
    folder = root / 'wavs'
    folder.mkdir()
    paths = cat.write_catalogue(folder)[:5]  # the four readable files and the silent one
    model_path = cat.write_model(root / 'merged_n6.pth')
    files = {p: audio.read_wav(p) for p in paths}  # samples (interleaved int16), channels, rate
    models = {}
    for prec in PRECISIONS:
        models[prec] = ir.load_merged_model(model_path, torch.device(DEV), precision=prec)
    return {'model': model_path, 'paths': paths, 'files': files, 'models': models, 'root': root}


@pytest.fixture(scope='module')
def oracle(setup):
    """inference_runner.main per file, precision and --smooth, and the
    whole-file logits; computed once (the checkpoint loads are shared, main is
    otherwise untouched) and never modified."""
    import inference_runner as ir
    from sad import ingest
    real_load = ir.load_merged_model
    ir.load_merged_model = lambda path, device, backbone_name='resnet18', precision='fp32': setup['models'][precision]
    out = {}
    cfg, spec = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=0.0, silence_threshold=1e-3), \
        ir.SpectrogramConfig()
    try:
        for prec in PRECISIONS:
            for p in setup['paths']:
                for smooth in (False, True):
                    o = str(setup['root'] / 'single.json')
                    ir.main(['--merged-model', setup['model'], '--audio', p, '--output-json', o, '--precision', prec]
                            + (['--smooth'] if smooth else []))
                    out[(prec, p, smooth)] = json.load(open(o))
                wf, sr = ir.preprocess_waveform(p, cfg, DEV)
                starts, _ = ingest.select_windows(wf, sr, cfg.window_size, cfg.overlap, cfg.silence_threshold)
                model = setup['models'][prec][0]
                out[(prec, p, 'logits')] = ir.run_windows(model, ingest.Windows(wf, starts, 128000), sr, spec, 128) \
                    if starts else torch.empty(0, 7)
    finally:
        ir.load_merged_model = real_load
    return out


def _bank(setup, prec, slots, overlap=0.0, max_chunk=44100, batch_size=4):
    import inference_runner as ir
    from sad.stream import StreamBank
    model, meta = setup['models'][prec]
    cfg = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=overlap, silence_threshold=1e-3)
    return StreamBank(model.engine, meta['class_names'], slots, cfg, ir.SpectrogramConfig(), max_chunk,
                      batch_size=batch_size)


def _feed_all(bank, feeds, chunk_ms):
    """feeds: {slot: (samples, channels, rate)} -> the events per slot, pushing
    one chunk of chunk_ms per slot and tick until every feed is through."""
    events = {s: [] for s in feeds}
    pos = {s: 0 for s in feeds}
    step = {s: max(1, sr * chunk_ms // 1000) * ch for s, (_, ch, sr) in feeds.items()}
    while True:
        push = {s: x[pos[s]:pos[s] + step[s]] for s, (x, _, _) in feeds.items() if pos[s] < x.shape[0]}
        if not push:
            return events
        for s in push:
            pos[s] += step[s]
        for ev in bank.push(push):
            events[ev['slot']].append(ev)


@pytest.mark.parametrize('chunk_ms', [37, 1000])
@pytest.mark.parametrize('prec', PRECISIONS)
def test_stream_equals_the_whole_file_path(setup, oracle, prec, chunk_ms):
    paths = setup['paths']
    bank = _bank(setup, prec, 2 * len(paths))
    feeds, of = {}, {}
    for smooth in (False, True):
        for p in paths:
            x, ch, sr = setup['files'][p]
            s = bank.open(p, sr, ch, x.dtype)
            feeds[s], of[s] = (x.reshape(-1), ch, sr), (p, smooth)
    events = _feed_all(bank, feeds, chunk_ms)
    pushes = bank.stats['pushes']
    assert bank.stats['uploads'] == bank.stats['launches'] == bank.stats['waits'] == pushes > 5
    checked = 0
    for s, (p, smooth) in of.items():
        rec = bank.close(s, smooth=smooth)
        events[s] += bank.last_events
        ref = oracle[(prec, p, smooth)]
        assert rec == ref and list(rec) == list(ref), (p, smooth)
        plain = oracle[(prec, p, False)]
        # the events: main's segments (times and the unsmoothed labels), in order
        assert [(e['start_sec'], e['end_sec'], e['label']) for e in events[s]] == \
            [(g['start_sec'], g['end_sec'], g['label']) for g in plain['segments']], p
        want = oracle[(prec, p, 'logits')]
        got = torch.stack([e['logits'] for e in events[s]]) if events[s] else torch.empty(0, 7)
        assert got.shape == want.shape and torch.equal(got, want), (p, (got - want).abs().max().item())
        for e in events[s]:
            assert e['name'] == p and np.array_equal(e['probs'], torch.sigmoid(e['logits']).numpy())
        checked += 1
    assert checked == 10
    assert bank.stats['uploads'] == bank.stats['launches'] == bank.stats['waits'] == bank.stats['pushes'] == pushes + 10
    by = {of[s]: events[s] for s in of}
    a, b, c, d, e = paths
    assert [ev['start_sec'] for ev in by[(a, False)]] == [0.0, 4.0, 8.0]
    starts_c = [ev['start_sec'] for ev in by[(c, False)]]  # 8-12 s is silent: no event
    assert 8.0 not in starts_c and 0.0 in starts_c and 16.0 in starts_c and len(starts_c) < 5
    assert [ev['start_sec'] for ev in by[(d, False)]] == [0.0]  # the short clip: one padded window
    assert len(by[(b, True)]) == 1 and by[(e, False)] == []
    assert oracle[(prec, e, False)] == {'filename': e, 'segments': [], 'percentages': {}}
    kept = sum(len(oracle[(prec, q, False)]['segments']) for q in paths)
    # candidates: 3 (12 s), 1 (5.8 s), 5 (20 s), 1 (the padded clip), 1 (6.25 s of silence)
    assert bank.stats['windows'] == 2 * kept and bank.stats['skipped'] == 2 * (11 - kept) and kept < 10


def test_overlap_085_equals_select_windows_and_run_windows(setup):
    import inference_runner as ir
    from sad import ingest
    p = setup['paths'][0]  # 12 s at 32 kHz
    x, ch, sr = setup['files'][p]
    bank = _bank(setup, 'fp32', 1, overlap=0.85, max_chunk=4000, batch_size=3)
    s = bank.open(p, sr, ch, x.dtype)
    events = _feed_all(bank, {s: (x.reshape(-1), ch, sr)}, 100)[s]
    rec = bank.close(s)
    events += bank.last_events
    cfg = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=0.85, silence_threshold=1e-3)
    wf, _ = ir.preprocess_waveform(p, cfg, DEV)
    starts, times = ingest.select_windows(wf, 32000, 4.0, 0.85, 1e-3)
    want = ir.run_windows(setup['models']['fp32'][0], ingest.Windows(wf, starts, 128000), 32000,
                          ir.SpectrogramConfig(), 128)
    assert len(starts) == 14 and [e['start_sec'] for e in events] == times
    assert torch.equal(torch.stack([e['logits'] for e in events]), want)
    assert [g['start_sec'] for g in rec['segments']] == times


def test_feed_joined_at_a_start_frame_past_2_to_32(setup, oracle):
    p = setup['paths'][0]
    x, ch, sr = setup['files'][p]
    bank = _bank(setup, 'fp32', 2)
    start = 128000 * 40000  # a multiple of the hop, past 2^32
    assert start > 1 << 32
    with pytest.raises(RuntimeError, match='multiple of hop'):
        bank.open('misaligned', sr, ch, x.dtype, start_frame=start + 1)
    s = bank.open('late', sr, ch, x.dtype, start_frame=start)
    events = _feed_all(bank, {s: (x.reshape(-1)[:2 * 128000], ch, sr)}, 1000)[s]
    assert [e['start_sec'] for e in events] == [start / 32000, (start + 128000) / 32000]
    assert torch.equal(torch.stack([e['logits'] for e in events]), oracle[('fp32', p, 'logits')][:2])
    rec = bank.close(s)
    assert bank.last_events == [] and len(rec['segments']) == 2


@pytest.mark.parametrize('overlap', [0.0, 0.85])
def test_chunks_many_times_max_chunk_frames(setup, overlap):
    """A chunk longer than one launch takes is split by push into several
    launches, never refused, and the windows each launch completes are examined
    before the next one overwrites the ring (CAP = 128000 + 17640 samples here):
    the whole 12 s file in ONE push (88 launches), the 44.1 kHz stereo file in
    3 s pushes, and an 8 kHz feed (4 outputs per frame) in 2.5 s pushes."""
    import os
    import inference_runner as ir
    from conftest import GOLDEN
    from sad import audio, ingest
    model, meta = setup['models']['fp32']
    names = meta['class_names']
    pcm = np.load(os.path.join(GOLDEN, 'golden_frontend.npz'))['pcm']
    p8 = str(setup['root'] / 'g_8k.wav')
    audio.save_pcm16(p8, np.concatenate([pcm[2][:40000], pcm[1][:37001]]), 8000)  # 9.6 s: 308,004 samples at 32 kHz
    a, b = setup['paths'][0], setup['paths'][1]
    plan = {a: None, b: 3 * 44100, p8: 20000}  # frames per push; None: everything at once
    cfg = ir.AudioConfig(sample_rate=32000, window_size=4.0, overlap=overlap, silence_threshold=1e-3)
    bank = _bank(setup, 'fp32', 3, overlap=overlap, max_chunk=4410, batch_size=5)
    feeds, step = {}, {}
    for p, frames in plan.items():
        x, ch, sr = audio.read_wav(p)
        s = bank.open(p, sr, ch, x.dtype)
        feeds[s], step[s] = (p, x.reshape(-1), ch), (x.shape[0] if frames is None else frames * ch)
        assert step[s] // ch > 4 * 4410
    events = {s: [] for s in feeds}
    pos = 0
    while True:
        push = {s: x[pos * step[s]:(pos + 1) * step[s]] for s, (_, x, _) in feeds.items() if pos * step[s] < x.shape[0]}
        if not push:
            break
        for ev in bank.push(push):
            events[ev['slot']].append(ev)
        pos += 1
    assert bank.stats['waits'] == bank.stats['pushes'] == 4  # 1, 2 and 4 pushes for the three feeds
    assert bank.stats['launches'] == bank.stats['uploads'] >= 88
    checked = 0
    for s, (p, _, _) in feeds.items():
        rec = bank.close(s)
        events[s] += bank.last_events
        wf, sr = ir.preprocess_waveform(p, cfg, DEV)
        starts, times = ingest.select_windows(wf, sr, cfg.window_size, cfg.overlap, cfg.silence_threshold)
        want = ir.run_windows(model, ingest.Windows(wf, starts, 128000), sr, ir.SpectrogramConfig(), 128)
        ref = ir.summarize(p, want, times, 0.5, names[:-1], names[-1], False, 4.0)
        assert len(starts) == ({a: 3, b: 1, p8: 2} if overlap == 0.0 else {a: 14, b: 4, p8: 10})[p]
        assert [e['start_sec'] for e in events[s]] == times, p
        assert torch.equal(torch.stack([e['logits'] for e in events[s]]), want), p
        assert rec == ref, p
        checked += 1
    assert checked == 3
