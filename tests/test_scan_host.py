"""CPU: the host side of the catalogue scan (sad/scan.py) -- header-only
candidate counts, pack planning, the split over ranks, record assembly -- and
the argument checks of the scan entry points (no GPU: they fail before any
device work)."""
import ctypes

import numpy as np
import pytest

from sad import scan as sc
from sad.audio import save_pcm16
from sad.ingest import window_starts

W = 128000


def _wav(tmp_path, name, frames, ch=1, sr=32000):
    p = str(tmp_path / name)
    save_pcm16(p, np.zeros((ch, frames), np.int16), sr)
    return p


@pytest.mark.parametrize('frames,ch,sr', [(0, 1, 32000), (77777, 1, 32000), (128000, 1, 32000), (128001, 2, 32000),
                                          (3 * 128000 + 5, 1, 32000), (200000, 2, 44100), (176401, 1, 44100),
                                          (64001, 1, 16000), (500000, 1, 48000)])
@pytest.mark.parametrize('hop', [128000, 19200])
def test_candidate_count_from_header(tmp_path, frames, ch, sr, hop):
    """What the header gives equals what select_windows would enumerate on the
    preprocessed waveform: torchaudio's resampled length, padded to one window."""
    import math
    info = sc.wav_info(_wav(tmp_path, 'a.wav', frames, ch, sr))
    assert info.error is None and (info.frames, info.channels, info.sr, info.i16) == (frames, ch, sr, True)
    assert info.raw_bytes == frames * ch * 2
    n = max(int(math.ceil(32000 * frames / sr)), W)  # torchaudio's target length, then the pad to a window
    assert sc.slot_len(info, 32000, W) == n
    assert sc.candidate_count(n, W, hop) == len(window_starts(n, W, hop))
    assert sc.candidate_count(n, W, hop) >= 1


def test_wav_info_reports_garbage(tmp_path):
    p = tmp_path / 'g.wav'
    p.write_bytes(bytes(range(256)) * 9)
    info = sc.wav_info(str(p))
    assert info.error and 'RIFF' in info.error
    assert sc.wav_info(str(tmp_path / 'missing.wav')).error


def test_plan_packs_respects_limit_and_keeps_files_whole():
    rng = np.random.RandomState(0)
    slots = [int(v) for v in rng.randint(W, 40 * W, size=200)] + [500 * W] + [W] * 5
    limit = 64 * W
    packs = sc.plan_packs(slots, limit)
    assert [i for p in packs for i in p] == list(range(len(slots)))  # every file once, in order, never split
    for p in packs:
        assert sum(slots[i] for i in p) <= limit or len(p) == 1
    for a, b in zip(packs, packs[1:]):  # a pack closes only when the next file would not fit
        assert sum(slots[i] for i in a) + slots[b[0]] > limit
    assert sc.plan_packs([], limit) == []


@pytest.mark.parametrize('world', [1, 2, 3, 8])
def test_split_ranks_is_contiguous_and_balanced(world):
    rng = np.random.RandomState(1)
    counts = [int(v) for v in rng.randint(0, 60, size=100)]
    ranges = sc.split_ranks(counts, world)
    assert len(ranges) == world and ranges[0][0] == 0 and ranges[-1][1] == len(counts)
    for (a, b), (c, d) in zip(ranges, ranges[1:]):
        assert a <= b == c <= d
    loads = [sum(counts[a:b]) for a, b in ranges]
    assert sum(loads) == sum(counts)
    assert max(loads) - sum(counts) / world <= max(counts)  # no rank exceeds its share by more than one file
    # degenerate inputs still cover every file once
    for cs in ([], [0, 0, 0], [5]):
        rr = sc.split_ranks(cs, world)
        assert rr[0][0] == 0 and rr[-1][1] == len(cs) and all(a <= b for a, b in rr)
        assert all(x[1] == y[0] for x, y in zip(rr, rr[1:]))


def test_records_have_summarize_shape():
    """Records from given arrays == inference_runner.summarize's for logits that
    give those labels (keys, label names, timestamps, percentages)."""
    import inference_runner as ir
    import torch
    syn, real = ['A', 'B'], 'Real'
    logits = torch.tensor([[3.0, -2.0, -3.0], [-3.0, -2.0, 4.0], [-1.0, 2.0, -3.0], [0.5, 0.25, 5.0]])
    starts = [1000, 1000 + 4 * W]  # arena offsets of two files
    offsets = np.array([1000, 1000 + W, 1000 + 3 * W, starts[1] + 19200], np.int64)
    row_start = np.array([0, 3, 3, 4, 4], np.int64)  # q.wav kept nothing; bad.wav could not be read
    label = np.array([0, -1, 1, 0], np.int32)
    probs = torch.sigmoid(logits).double().numpy()
    mean = np.stack([probs[:3].mean(0), np.zeros(3), probs[3:].mean(0), np.zeros(3)])
    recs = sc.assemble_records(['a.wav', 'q.wav', 'b.wav', 'bad.wav'], [1000, 1000 + 3 * W + W, starts[1], 0],
                               row_start, offsets, label, mean, syn, real, 32000, 4.0,
                               errors={3: 'ValueError: not a RIFF/WAVE file'})
    ref_a = ir.summarize('a.wav', logits[:3], [0.0, 4.0, 12.0], 0.5, syn, real, False, 4.0)
    ref_b = ir.summarize('b.wav', logits[3:], [0.6], 0.5, syn, real, False, 4.0)
    for rec, ref in ((recs[0], ref_a), (recs[2], ref_b)):
        assert list(rec) == list(ref) == ['filename', 'segments', 'percentages']
        assert rec['segments'] == ref['segments']
        assert list(rec['percentages']) == list(ref['percentages'])
        for k, v in ref['percentages'].items():
            assert abs(rec['percentages'][k] - v) <= 1e-4
    assert recs[1] == {'filename': 'q.wav', 'segments': [], 'percentages': {}}
    assert recs[3] == {'filename': 'bad.wav', 'error': 'ValueError: not a RIFF/WAVE file'}
    assert sc.label_name(5, syn, real) == 'Synthetic_6'


def test_scan_entry_points_reject_bad_arguments():
    from sad import _lib
    lib = _lib.load()
    sz = _lib.SZ()
    one = ctypes.c_void_p(64)  # never dereferenced: every call below fails its argument check first

    def bad(rc, word):
        assert rc == -1 and word in lib.sad_last_error(), (rc, lib.sad_last_error())

    bad(lib.sad_scan_select_workspace_size(1, 1, None), b'null')
    bad(lib.sad_scan_select_workspace_size(-1, 1, ctypes.byref(sz)), b'n_files')
    bad(lib.sad_scan_select_workspace_size(1, -1, ctypes.byref(sz)), b'max_candidates')
    assert lib.sad_scan_select_workspace_size(3, 10, ctypes.byref(sz)) == 0 and sz.value >= 4 * 8 + 10 * 20
    sel = lambda **k: lib.sad_scan_select_run(*[k.get(n, d) for n, d in (
        ('wav', one), ('wav_len', 1000), ('file_start', one), ('file_len', one), ('n_files', 1), ('window', 100),
        ('hop', 100), ('thr', 1e-3), ('cap', 10), ('offsets', one), ('row_start', one), ('ws', one),
        ('ws_bytes', 1 << 20), ('stream', None))])
    bad(sel(wav=None), b'null')
    bad(sel(file_start=None), b'null')
    bad(sel(file_len=None), b'null')
    bad(sel(offsets=None), b'null')
    bad(sel(row_start=None), b'null')
    bad(sel(ws=None), b'null')
    bad(sel(n_files=-1), b'n_files')
    bad(sel(cap=-1), b'max_candidates')
    bad(sel(wav_len=-1), b'wav_len')
    bad(sel(window=0), b'window')
    bad(sel(hop=0), b'hop')
    assert sel(ws_bytes=8) == -4 and b'workspace' in lib.sad_last_error()

    bad(lib.sad_scan_post_workspace_size(4, 7, 1, None), b'null')
    bad(lib.sad_scan_post_workspace_size(-1, 7, 1, ctypes.byref(sz)), b'B')
    bad(lib.sad_scan_post_workspace_size(4, 1, 1, ctypes.byref(sz)), b'C')
    bad(lib.sad_scan_post_workspace_size(4, 129, 1, ctypes.byref(sz)), b'C')
    assert lib.sad_scan_post_workspace_size(4, 7, 1, ctypes.byref(sz)) == 0 and sz.value >= 4 * 7 * 4
    assert lib.sad_scan_post_workspace_size(4, 7, 0, ctypes.byref(sz)) == 0 and sz.value == 0
    post = lambda **k: lib.sad_scan_post_run(*[k.get(n, d) for n, d in (
        ('logits', one), ('B', 4), ('C', 7), ('row_start', one), ('n_files', 2), ('thr', 0.5), ('smooth', 1),
        ('probs', one), ('label', one), ('mean', one), ('ws', one), ('ws_bytes', 1 << 20), ('stream', None))])
    bad(post(logits=None), b'null')
    bad(post(row_start=None), b'null')
    bad(post(probs=None), b'null')
    bad(post(label=None), b'null')
    bad(post(mean=None), b'null')
    bad(post(ws=None), b'null')
    bad(post(B=-1), b'B')
    bad(post(C=0), b'C')
    bad(post(n_files=-1), b'n_files')
    assert post(ws_bytes=8) == -4 and b'workspace' in lib.sad_last_error()
