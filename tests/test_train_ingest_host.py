"""CPU: the host half of the trainer's device ingestion (submodel_trainer.py
--device-ingest): the segment rule decided from the WAV header, the `need`
formula for truncated reads, read_wav's frame limit, the batch arena with its
file and tile tables, the augmentation draws, and the argument checks of the
new C entries (no device work: there is no GPU here)."""
import ctypes
import math
import os
import struct

import numpy as np
import pytest
import torch

SEG = 640  # small segment length for the file-level cases (production: 128000)
RATES_NEED = {44100: 1773, 48000: 1930, 16000: 647, 22050: 889, 8000: 327, 96000: 3859}


def _write_wav(path, x, sr, fmt='i16'):
    """x [frames, channels] -> a WAV file: 'i16' (PCM 16), 'i24' (PCM 24), 'f32' (IEEE float)."""
    x = np.asarray(x)
    frames, ch = x.shape
    if fmt == 'i16':
        tag, bits, raw = 1, 16, x.astype('<i2').tobytes()
    elif fmt == 'i24':
        v = x.astype(np.int32).reshape(-1)
        b = np.stack([(v >> s) & 0xFF for s in (0, 8, 16)], axis=1).astype(np.uint8)
        tag, bits, raw = 1, 24, b.tobytes()
    else:
        tag, bits, raw = 3, 32, x.astype('<f4').tobytes()
    width = bits // 8
    head = struct.pack('<4sI4s4sIHHIIHH4sI', b'RIFF', 36 + len(raw), b'WAVE', b'fmt ', 16, tag, ch, sr,
                       sr * ch * width, ch * width, bits, b'data', len(raw))
    with open(path, 'wb') as f:
        f.write(head + raw)


def _pcm(frames, ch=1, seed=0):
    return np.random.default_rng(seed).integers(-20000, 20000, size=(frames, ch)).astype(np.int16)


def _frames_for(n, sr):
    """A frame count at sr whose 32 kHz length is exactly n."""
    from sad import ingest
    f = n * sr // 32000
    while ingest.train_out_len(f, sr) < n:
        f += 1
    while ingest.train_out_len(f - 1, sr) >= n:
        f -= 1
    assert ingest.train_out_len(f, sr) == n
    return f


def _boundaries(seg):
    lo = math.ceil(0.9 * seg)
    return [2 * seg, 2 * seg - 1, seg, seg - 1, lo, lo - 1]


def _rule_of_segments(segs):
    if segs is None:
        return None
    if segs[0] is not segs[1] and not torch.equal(segs[0], segs[1]):
        return 'two'
    return 'dup'


# ------------------------------------------------------------------ segment rule
def test_rule_matches_segment_waveform_at_32k():
    import submodel_trainer as smt
    from sad import ingest
    seg = smt.SEGMENT_LENGTH
    want = ['two', 'first', 'first', 'pad', 'pad', None]
    for n, w in zip(_boundaries(seg), want):
        assert ingest.train_segment_rule(n, seg) == w, n
        segs = smt.segment_waveform(torch.arange(n, dtype=torch.float32)[None] + 1.0)
        assert (segs is None) == (w is None), n
        if w == 'two':
            assert segs[1][0, 0].item() == seg + 1.0
        elif w is not None:
            assert segs[0] is segs[1] and segs[0].shape[1] == seg
            assert (w == 'pad') == (n < seg)


def test_rule_through_44k_frame_counts(monkeypatch):
    """The 32 kHz length comes from ceil(320 * frames / 441): the header-only
    length equals the resampled waveform's, on both sides of every boundary."""
    import submodel_trainer as smt
    from sad import audio, ingest
    monkeypatch.setattr(smt, 'SEGMENT_LENGTH', SEG)
    want = ['two', 'first', 'first', 'pad', 'pad', None]
    for n, w in zip(_boundaries(SEG), want):
        for frames in (_frames_for(n, 44100), _frames_for(n, 44100) - 1):
            wf = audio.resample(torch.from_numpy(_pcm(frames)[:, 0].astype(np.float32) / 32768.0)[None], 44100, 32000)
            n_hdr = ingest.train_out_len(frames, 44100)
            assert n_hdr == wf.shape[1]
            segs = smt.segment_waveform(wf)
            rule = ingest.train_segment_rule(n_hdr, SEG)
            assert (rule is None) == (segs is None), (n, frames)
            if rule is not None:
                assert (rule == 'two') == (segs[0] is not segs[1])
        assert ingest.train_segment_rule(n, SEG) == w


def _dataset(monkeypatch, tmp_path, files):
    """A StoredSampleDataset over tmp_path/train/Real/<name>.wav at SEG."""
    import submodel_trainer as smt
    monkeypatch.setattr(smt, 'SEGMENT_LENGTH', SEG)
    d = tmp_path / 'train' / 'Real'
    os.makedirs(d, exist_ok=True)
    for name, write in files:
        write(str(d / name))
    return smt.StoredSampleDataset(str(tmp_path), 'train', transform='train', class_names=['Real', 'Class1'])


def test_short_empty_corrupt_files_are_dropped_without_reading_samples(monkeypatch, tmp_path):
    from sad import audio
    lo = math.ceil(0.9 * SEG)

    def corrupt(path):
        with open(path, 'wb') as f:
            f.write(b'RIFFxxxxWAVEjunk')

    ds = _dataset(monkeypatch, tmp_path, [
        ('a_short.wav', lambda p: _write_wav(p, _pcm(lo - 1), 32000)),
        ('b_short44.wav', lambda p: _write_wav(p, _pcm(_frames_for(lo - 1, 44100), 2), 44100)),
        ('c_empty.wav', lambda p: _write_wav(p, _pcm(0), 32000)),
        ('d_corrupt.wav', corrupt),
        ('e_ok.wav', lambda p: _write_wav(p, _pcm(lo), 32000)),
    ])

    def no_read(*a, **k):
        raise AssertionError('the data chunk was read')

    monkeypatch.setattr(audio, 'read_wav', no_read)
    monkeypatch.setattr(np, 'fromfile', no_read)
    assert [ds[i] for i in range(4)] == [None] * 4
    monkeypatch.undo()
    import submodel_trainer as smt
    monkeypatch.setattr(smt, 'SEGMENT_LENGTH', SEG)
    item = ds[4]
    assert item is not None and item.frames == item.frames_read == lo  # need <= frames honoured: a short file whole


# ------------------------------------------------------------------ need formula
def _polyphase_fixed_order(x, sr, n):
    """The first n samples of resample(x, sr, 32000) summed tap by tap in ascending
    k, fp32 (x zero outside its range), and the float64 products [n, K]."""
    from sad import audio
    g = math.gcd(sr, 32000)
    kern, width = audio._sinc_resample_kernel(sr, 32000, g)
    kern = kern[:, 0, :].numpy()
    orig, new, K = sr // g, 32000 // g, kern.shape[1]
    m = np.arange(n)
    j, p = m // new, m % new
    idx = j[:, None] * orig + np.arange(K)[None, :] - width
    xk = np.where((idx >= 0) & (idx < x.shape[0]), x[np.clip(idx, 0, x.shape[0] - 1)], np.float32(0))
    acc = np.zeros(n, np.float32)
    for k in range(K):
        acc = acc + xk[:, k] * kern[p, k]
    return acc, xk.astype(np.float64) * kern[p].astype(np.float64)


@pytest.mark.parametrize('sr', sorted(RATES_NEED))
def test_need_frames_reproduce_the_full_resample(sr):
    """The first `need` frames give the first 2 seg samples of the full-file
    resample.  (a) With the sum taken in a fixed order the two are equal bit
    for bit at every rate.  (b) Through sad.audio.resample they are equal bit
    for bit only where the CPU's conv1d sums a given output in the same order
    for both input lengths: on an 8-thread x86 build host all six rates are
    equal, on an MI355X node's host CPU 16 / 44.1 / 48 kHz differ by one ulp of
    the output (max |d| 6.0e-8, 6.0e-8, 3.0e-8 with 16 threads; 44.1 kHz also
    with one thread, oneDNN on or off).  That order is the CPU library's, not the
    formula's, so (b) asserts the bound that holds for any two fp32 summation
    orders of the same K products, 2 K 2^-24 sum_k |x_k w_k| per sample, and
    prints the figure; (a) carries the exactness."""
    from sad import _lib, audio, ingest
    need = ingest.train_need_frames(sr, SEG)
    assert need == RATES_NEED[sr]
    c = _lib.I64()
    assert _lib.load().sad_train_ingest_need_frames(sr, 32000, SEG, ctypes.byref(c)) == 0 and c.value == need
    x = torch.from_numpy(_pcm(need + 777, seed=sr)[:, 0].astype(np.float32) / 32768.0)[None]
    # (a) the polyphase sum in a fixed order (ascending k, fp32): exactly equal, so
    # no sample past `need` is read by the first 2 seg outputs
    fixed_full, terms = _polyphase_fixed_order(x[0].numpy(), sr, 2 * SEG)
    fixed_head, _ = _polyphase_fixed_order(x[0, :need].numpy(), sr, 2 * SEG)
    assert np.array_equal(fixed_head, fixed_full)
    # (b) sad.audio.resample itself
    full = audio.resample(x, sr, 32000)
    assert full.shape[1] >= 2 * SEG
    head = audio.resample(x[:, :need], sr, 32000)
    assert head.shape[1] >= 2 * SEG
    err = (head[0, :2 * SEG] - full[0, :2 * SEG]).abs().double().numpy()
    bar = 2 * terms.shape[1] * 2.0 ** -24 * np.abs(terms).sum(axis=1)
    print(f'sr {sr}: resample(head) vs resample(full): max |d| {err.max():.3e}, max d/bar {(err / bar).max():.3e}')
    assert np.all(err <= bar)
    assert np.abs(full[0, :2 * SEG].double().numpy() - fixed_full).max() <= bar.max()


def test_need_at_the_target_rate_and_tile_counts_agree_with_the_library():
    from sad import _lib, ingest
    lib = _lib.load()
    assert ingest.train_need_frames(32000, SEG) == 2 * SEG
    c = _lib.I64()
    for sr in (32000,) + tuple(RATES_NEED):
        for frames in (1, 700, 1500, 5000, 400000):
            for seg in (SEG, 128000):
                assert lib.sad_train_ingest_file_tiles(sr, 32000, frames, seg, ctypes.byref(c)) == 0
                assert c.value == ingest.train_file_tiles(sr, frames, seg) > 0
    assert not ingest.train_rate_supported(384000) and ingest.train_rate_supported(192000)
    assert lib.sad_train_ingest_file_tiles(384000, 32000, 1000, SEG, ctypes.byref(c)) == -1


def test_dataset_reads_need_frames_only(monkeypatch, tmp_path):
    from sad import ingest
    pcm = _pcm(9000, 2, seed=3)
    ds = _dataset(monkeypatch, tmp_path, [('a.wav', lambda p: _write_wav(p, pcm, 44100)),
                                          ('b.wav', lambda p: _write_wav(p, pcm[:1200], 44100))])
    a, b = ds[0], ds[1]
    need = ingest.train_need_frames(44100, SEG)
    assert (a.frames, a.frames_read, a.channels, a.sr) == (9000, need, 2, 44100)
    assert a.samples.dtype == np.int16 and np.array_equal(a.samples, pcm[:need].reshape(-1))
    assert (b.frames, b.frames_read) == (1200, 1200)  # shorter than need: the whole file


# ---------------------------------------------------------- reading and collation
@pytest.mark.parametrize('fmt', ['i16', 'i24', 'f32'])
def test_truncated_read_is_the_head_of_the_full_read(tmp_path, fmt):
    from sad import audio
    rng = np.random.default_rng(5)
    if fmt == 'f32':
        x = rng.standard_normal((1000, 2)).astype(np.float32)
    else:
        x = rng.integers(-(1 << 22) if fmt == 'i24' else -30000, (1 << 22) if fmt == 'i24' else 30000, size=(1000, 2))
    path = str(tmp_path / f'{fmt}.wav')
    _write_wav(path, x, 44100, fmt)
    full, ch, sr = audio.read_wav(path)
    assert (ch, sr, full.shape[0]) == (2, 44100, 2000)
    assert full.dtype == (np.int16 if fmt == 'i16' else np.float32)
    for limit in (0, 1, 333, 1000, 5000):
        part, ch2, sr2 = audio.read_wav(path, max_frames=limit)
        assert (ch2, sr2) == (2, 44100) and part.dtype == full.dtype
        assert np.array_equal(part, full[:min(limit, 1000) * 2])
    assert audio.wav_header(path)[:3] == (1000, 2, 44100)


def test_collate_offsets_alignment_and_tables(monkeypatch, tmp_path):
    from sad import _lib, ingest
    import submodel_trainer as smt
    pa, pb, pc = _pcm(1501, 1, 1), _pcm(5000, 3, 2), np.random.default_rng(3).standard_normal((1283, 2))
    ds = _dataset(monkeypatch, tmp_path, [('a.wav', lambda p: _write_wav(p, pa, 32000)),
                                          ('b.wav', lambda p: _write_wav(p, pb, 44100)),
                                          ('bad.wav', lambda p: _write_wav(p, _pcm(10), 32000)),
                                          ('c.wav', lambda p: _write_wav(p, pc, 32000, 'f32'))])
    items = [ds[i] for i in range(4)]
    assert items[2] is None
    batch = smt.stored_collate_fn(items)
    assert isinstance(batch, ingest.StoredBatch) and len(batch) == 3 and batch.seg_len == SEG
    assert batch.rates == (32000, 44100)
    need44 = ingest.train_need_frames(44100, SEG)
    sizes = [2 * SEG * 2, need44 * 3 * 2, 2 * SEG * 2 * 4]  # bytes read per file
    offs = [0]
    for s in sizes:
        offs.append(-(-(offs[-1] + s) // 16) * 16)
    tab = batch.table.numpy()
    assert tab.tolist() == [[offs[0], 2 * SEG, 1501, 1, _lib.SAD_PCM_I16, 0],
                            [offs[1], need44, 5000, 3, _lib.SAD_PCM_I16, 1],
                            [offs[2], 2 * SEG, 1283, 2, _lib.SAD_PCM_F32, 0]]
    assert all(o % 16 == 0 for o in tab[:, 0]) and batch.table_off == offs[3] and batch.tiles_off % 16 == 0
    raw = batch.arena.numpy()
    assert np.array_equal(raw[offs[1]:offs[1] + sizes[1]].view(np.int16), pb[:need44].reshape(-1))
    assert np.array_equal(raw[offs[2]:offs[2] + sizes[2]].view(np.float32),
                          pc[:2 * SEG].astype(np.float32).reshape(-1))
    # the tile table: every (file, tile) once, file by file
    counts = [ingest.train_file_tiles(sr, fr, SEG) for sr, fr in ((32000, 1501), (44100, 5000), (32000, 1283))]
    assert counts == [2, 5, 2]  # 2 x 640 outputs / 1024; one 64-frame tile x 5 phase blocks
    want = [[f, t] for f, c in enumerate(counts) for t in range(c)]
    assert batch.tiles.tolist() == want and batch.n_tiles == len(want)
    assert batch.targets.tolist() == [0, 0, 0] and batch.aug.shape == (3, 2, 8) and batch.aug.dtype == torch.int32
    assert smt.stored_collate_fn([None, None]) is None


def test_augmentation_rows_equal_the_host_datasets(monkeypatch, tmp_path):
    import submodel_trainer as smt
    files = [(f'{i}.wav', (lambda p, i=i: _write_wav(p, _pcm(2 * SEG + 10 * i, 1, i), 32000))) for i in range(3)]
    ds = _dataset(monkeypatch, tmp_path, files)
    host = smt.SpectrogramDataset(str(tmp_path), 'train', transform='train', class_names=['Real', 'Class1'])
    torch.manual_seed(7)
    rows_host = [host[i][4] for i in range(3)]
    torch.manual_seed(7)
    rows_new = [ds[i].aug for i in range(3)]
    for a, b in zip(rows_host, rows_new):
        assert torch.equal(a, b)
    assert not torch.equal(rows_new[0], rows_new[1])


def test_loader_with_a_worker_process_delivers_the_same_batches(tmp_path):
    """get_dataloaders with --device-ingest and a worker (fork server, persistent):
    the batches that cross the process boundary equal the in-process ones."""
    import submodel_trainer as smt
    from sad import ingest
    for mode in ('train', 'test'):
        d = tmp_path / mode / 'Real'
        os.makedirs(d)
        for i in range(3):
            _write_wav(str(d / f'{i}.wav'), _pcm(2 * smt.SEGMENT_LENGTH + 5 + i, 1 + i % 2, i), 32000)
    got = {}
    for workers in (0, 1):
        args = smt.parse_args(['--data-dir', str(tmp_path), '--batch-size', '2', '--workers', str(workers),
                               '--device-ingest'])
        val = smt.get_dataloaders(args)[1]  # not shuffled
        assert (val.multiprocessing_context is not None) == bool(workers) and val.persistent_workers == bool(workers)
        got[workers] = list(val)
        del val
    assert len(got[0]) == len(got[1]) == 2
    for a, b in zip(got[0], got[1]):
        assert isinstance(b, ingest.StoredBatch) and (a.n_files, a.n_tiles, a.rates) == (b.n_files, b.n_tiles, b.rates)
        assert torch.equal(a.arena, b.arena) and torch.equal(a.table, b.table) and torch.equal(a.tiles, b.tiles)
        assert torch.equal(a.targets, b.targets) and torch.equal(a.aug, b.aug)
    host_args = smt.parse_args(['--data-dir', str(tmp_path), '--batch-size', '2', '--workers', '1'])
    host_val = smt.get_dataloaders(host_args)[1]  # the default path keeps the DataLoader defaults
    assert host_val.multiprocessing_context is None and not host_val.persistent_workers


# ---------------------------------------------------------------- argument errors
def test_argument_errors_of_the_new_entries():
    from sad import _lib
    lib = _lib.load()
    c = _lib.I64()

    def bad(rc, word):
        assert rc == -1 and word in lib.sad_last_error().decode(), lib.sad_last_error()

    bad(lib.sad_train_ingest_need_frames(44100, 32000, SEG, None), 'null')
    bad(lib.sad_train_ingest_need_frames(0, 32000, SEG, ctypes.byref(c)), 'positive')
    bad(lib.sad_train_ingest_need_frames(44100, 32000, 0, ctypes.byref(c)), 'seg_len')
    bad(lib.sad_train_ingest_file_tiles(44100, 32000, 10, SEG, None), 'null')
    bad(lib.sad_train_ingest_file_tiles(44100, 32000, -1, SEG, ctypes.byref(c)), 'total_frames')
    bad(lib.sad_train_ingest_file_tiles(44100, 32000, 10, 0, ctypes.byref(c)), 'seg_len')

    plans = (ctypes.c_void_p * 1)(None)  # rate 0: the target rate (no plan, no device memory)
    fake = 0x1000  # a non-null "device" pointer: the checks return before any device work

    def run(row, arena_bytes=4096, n_files=1, n_tiles=2, seg=SEG, arena=fake, out=fake, n_rates=1, table=True):
        t = np.array([row], np.int64)
        return lib.sad_train_ingest_run(arena, arena_bytes, t.ctypes.data if table else None, fake, n_files, fake,
                                        n_tiles, plans, n_rates, seg, out, None)

    good = [0, 100, 1500, 1, 0, 0]
    bad(run(good, seg=0), 'seg_len')
    bad(run(good, arena=None), 'null')
    bad(run(good, out=None), 'null')
    bad(run(good, table=False), 'null')
    bad(run(good, n_rates=0), 'n_rates')
    bad(run([0, 100, 1500, 0, 0, 0]), 'channels')
    bad(run([0, 100, 1500, 65, 0, 0]), 'channels')
    bad(run([0, 100, 1500, 1, 2, 0]), 'encoding')
    bad(run([0, 100, 1500, 1, 0, 1]), 'rate index')
    bad(run([0, 100, 1500, 1, 0, -1]), 'rate index')
    bad(run([8, 100, 1500, 1, 0, 0]), 'multiple of 16')
    bad(run([4112, 0, 1500, 1, 0, 0]), 'past the end')
    bad(run([4000, 100, 1500, 1, 0, 0]), 'past the end')
    bad(run([0, 1501, 1500, 1, 0, 0]), 'frames read')
    bad(run(good, n_tiles=3), 'n_tiles')
