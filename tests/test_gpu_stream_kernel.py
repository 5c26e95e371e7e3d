"""GPU: sad_stream_push_run against the whole-file ingestion, bit for bit.

A small bank (window 4096, hop 613, chunks of at most 1024 frames: CAP 8192)
makes the rings wrap many times within 30k frames.  For every feed,
concatenating what the pushes emitted -- the tail after the final push and the
zero pad of a feed shorter than one window included -- must equal
sad_pcm_mono_run + sad_resample_run on the same samples
(ingest.waveform_from_samples, itself pinned to the oracle by
tests/test_gpu_ingest.py), for every way of cutting the feed into chunks.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WINDOW, HOP, MAX_CHUNK = 4096, 613, 1024
RATES = (32000, 48000, 16000, 8000, 96000, 44100, 22050, 11025)  # native; per-output x4; wide x3
FORMATS = [(np.int16, 1), (np.int16, 2), (np.int16, 3), (np.float32, 1), (np.float32, 2), (np.float32, 3)]
LONG, SHORT = 30011, 1500  # frames: LONG wraps the ring many times; SHORT keeps the tiny chunkings quick, and its
# feeds are opened at a start frame whose first sample lies 100-400 samples before a ring wrap (_wrap_start)
CHUNKINGS = ['one', 'width-1', 'width', 'width+1', 'orig', 'K', '997', 'max', 'zero-mid', 'random']
SMALL = ('one', 'width-1', 'width', 'width+1', 'orig')


def _signal(sr, dtype, ch, frames):
    rng = np.random.default_rng(sr + 7 * ch + (dtype == np.float32))
    if dtype == np.int16:
        return rng.integers(-20000, 20000, size=frames * ch).astype(np.int16)
    return (0.5 * rng.standard_normal(frames * ch)).astype(np.float32)


@pytest.fixture(scope='module')
def feeds():
    """Every (rate, encoding, channels) feed at both lengths, with its
    whole-file result (computed once, shared by all chunkings, never modified)."""
    from sad import ingest
    out = {}
    for frames in (LONG, SHORT):
        for sr in RATES:
            for dtype, ch in FORMATS:
                x = _signal(sr, dtype, ch, frames)
                ref, _ = ingest.waveform_from_samples(x, ch, sr, 32000, WINDOW, DEV)
                out[(frames, sr, dtype, ch)] = (x, ref)
    torch.cuda.synchronize()
    return out


def _chunks(name, sr, frames, rng):
    from sad.ingest import resample_geometry
    orig, new, width, K = resample_geometry(sr)
    if name == 'zero-mid':
        sizes = [997, 0] + [MAX_CHUNK] * ((frames - 997) // MAX_CHUNK)
        return sizes + [frames - sum(sizes)]
    if name == 'random':
        sizes = []
        while sum(sizes) < frames:
            sizes.append(int(min(frames - sum(sizes), rng.integers(0, MAX_CHUNK + 1))))
        return sizes
    c = {'one': 1, 'width-1': width - 1, 'width': width, 'width+1': width + 1, 'orig': orig, 'K': K, '997': 997,
         'max': MAX_CHUNK}[name]
    return [c] * (frames // c) + ([frames % c] if frames % c else [])


def _wrap_start(sr, cap):
    """A start frame (a multiple of orig whose first 32 kHz sample g0 is a
    multiple of the hop) with g0 mod CAP in [CAP - 400, CAP - 100]: even the
    500 samples of the short 96 kHz feed cross the ring's wrap."""
    from sad.ingest import resample_geometry
    orig, new, _, _ = resample_geometry(sr)
    for k in range(1, 100000):
        g0 = HOP * k * new
        if cap - 400 <= g0 % cap <= cap - 100:
            return HOP * k * orig, g0
    raise AssertionError(sr)


class _Reader:
    """Collects what a slot emitted, reading the ring before it can be overwritten."""

    def __init__(self, bank, slot):
        self.bank, self.slot, self.pos, self.parts = bank, slot, bank.state(slot).emitted, []

    def take(self, force=False):
        e = self.bank.state(self.slot).emitted
        assert e - self.pos <= self.bank.cap
        if e - self.pos >= 1024 or (force and e > self.pos):
            self.parts.append(self.bank.read(self.slot, self.pos, e - self.pos))
            self.pos = e

    def result(self):
        return torch.cat(self.parts) if self.parts else torch.empty(0, device=DEV)


def _run_feeds(bank, plan, shuffle=None):
    """plan: {slot: (samples, channels, chunk sizes in frames)}; pushes one chunk
    per slot and tick until every feed is through, then ends them all -> {slot: emitted}."""
    readers = {s: _Reader(bank, s) for s in plan}
    pos = {s: 0 for s in plan}
    idx = {s: 0 for s in plan}
    ticks = 0
    while any(idx[s] < len(plan[s][2]) for s in plan):
        order = [s for s in plan if idx[s] < len(plan[s][2])]
        if shuffle is not None:
            order = [order[i] for i in shuffle.permutation(len(order))]
        push = {}
        for s in order:
            x, ch, sizes = plan[s]
            c = sizes[idx[s]]
            push[s] = x[pos[s] * ch:(pos[s] + c) * ch]
            pos[s] += c
            idx[s] += 1
        bank.ingest(push)
        ticks += 1
        for s in order:
            readers[s].take()
    for s in plan:
        assert pos[s] * plan[s][1] == plan[s][0].shape[0]
        readers[s].take(force=True)
    bank.ingest({}, final=list(plan))
    for s in plan:
        readers[s].take(force=True)
    return {s: readers[s].result() for s in plan}, ticks


@pytest.mark.parametrize('chunking', CHUNKINGS)
def test_every_chunking_equals_the_whole_file_path(feeds, chunking):
    from sad.stream import StreamIngest
    frames = SHORT if chunking in SMALL else LONG
    bank = StreamIngest(len(RATES) * len(FORMATS), WINDOW, HOP, MAX_CHUNK, DEV)
    assert bank.cap == 8192
    rng = np.random.default_rng(5)
    plan, refs, wraps = {}, {}, []
    for sr in RATES:
        for dtype, ch in FORMATS:
            x, ref = feeds[(frames, sr, dtype, ch)]
            start, g0 = _wrap_start(sr, bank.cap) if frames == SHORT else (0, 0)
            s = bank.open(f'{sr}-{np.dtype(dtype).name}-{ch}', sr, ch, dtype, start_frame=start)
            plan[s] = (x, ch, _chunks(chunking, sr, frames, rng))
            refs[s] = (sr, dtype, ch, ref)
            wraps.append((g0 + ref.shape[0]) // bank.cap - g0 // bank.cap)
    assert min(wraps) >= 1  # every feed of every chunking crosses the ring's wrap at least once
    got, _ = _run_feeds(bank, plan)
    torch.cuda.synchronize()
    checked = 0
    for s, (sr, dtype, ch, ref) in refs.items():
        assert got[s].shape == ref.shape and ref.shape[0] >= WINDOW, (sr, dtype, ch, got[s].shape, ref.shape)
        assert torch.equal(got[s], ref), (chunking, sr, dtype, ch, (got[s] - ref).abs().max().item())
        checked += 1
    assert checked == 48
    if frames == SHORT:  # 96 kHz: 500 samples, then the zero pad, written by the final push
        s96 = [s for s, v in refs.items() if v[0] == 96000][0]
        assert got[s96].shape[0] == WINDOW and not got[s96][500:].any() and got[s96][:500].any()


def test_nine_slots_in_one_launch_shuffled_table(feeds):
    from sad.stream import StreamIngest
    bank = StreamIngest(9, WINDOW, HOP, MAX_CHUNK, DEV)
    rng = np.random.default_rng(9)
    plan, refs = {}, {}
    for i, sr in enumerate(RATES + (44100,)):  # eight rates, 44.1 kHz twice
        dtype, ch = FORMATS[(2 * i + 1) % 6]
        x, ref = feeds[(LONG, sr, dtype, ch)]
        s = bank.open(f'feed{i}', sr, ch, dtype)
        # a different chunk length per slot, and empty chunks (nothing on that tick) here and there
        sizes = [c for k in range(200) for c in ((0, 300 + 77 * i) if (k + i) % 5 == 0 else (300 + 77 * i,))]
        keep, total = [], 0
        for c in sizes:
            c = min(c, LONG - total)
            keep.append(c)
            total += c
            if total == LONG:
                break
        plan[s], refs[s] = (x, ch, keep), ref
    got, ticks = _run_feeds(bank, plan, shuffle=rng)
    torch.cuda.synchronize()
    assert bank.stats['launches'] == bank.stats['uploads'] == ticks + 1  # one launch per tick, and the final one
    for s, ref in refs.items():
        assert torch.equal(got[s], ref), s
    assert len(got) == 9


def test_reopened_slot_does_not_see_its_previous_occupant(feeds):
    from sad.stream import StreamIngest
    bank = StreamIngest(1, WINDOW, HOP, MAX_CHUNK, DEV)
    checked = 0
    for sr in (44100, 48000, 32000):
        loud, ref_loud = feeds[(LONG, sr, np.int16, 1)]
        s = bank.open('loud', sr, 1, np.int16)
        got, _ = _run_feeds(bank, {s: (loud, 1, _chunks('997', sr, LONG, None))})
        assert torch.equal(got[s], ref_loud)
        bank.release(s)
        from sad import ingest
        clip = _signal(sr + 1, np.int16, 1, 1000)
        ref, _ = ingest.waveform_from_samples(clip, 1, sr, 32000, WINDOW, DEV)
        s2 = bank.open('clip', sr, 1, np.int16)
        assert s2 == s
        got, _ = _run_feeds(bank, {s2: (clip, 1, [400, 600])})
        n_out = -(-32000 * 1000 // sr)
        assert got[s2].shape[0] == WINDOW and torch.equal(got[s2], ref)
        assert not got[s2][n_out:].any() and got[s2][:n_out].any()
        # the window the front end would read in place is the same memory
        assert torch.equal(bank.arena[bank.ring_offset(s2, 0):bank.ring_offset(s2, 0) + WINDOW], ref)
        bank.release(s2)
        checked += 1
    assert checked == 3


def test_start_frame_past_2_to_32(feeds):
    from sad import stream
    from sad.ingest import resample_geometry
    bank = stream.StreamIngest(len(RATES), WINDOW, HOP, MAX_CHUNK, DEV)
    plan, refs = {}, {}
    for sr in RATES:
        orig, new, width, K = resample_geometry(sr)
        J0 = (1 << 32) // orig + 1
        while (J0 * new) % HOP:
            J0 += 1
        assert J0 * orig > 1 << 32
        x, ref = feeds[(LONG, sr, np.int16, 2)]
        with pytest.raises(RuntimeError, match='multiple of'):
            bank.open('misaligned', sr, 2, np.int16, start_frame=J0 * orig + orig)
        s = bank.open(f'late{sr}', sr, 2, np.int16, start_frame=J0 * orig)
        st = bank.state(s)
        assert st.g0 == st.emitted == st.next_start == J0 * new == stream.first_sample(J0 * orig, sr)
        plan[s], refs[s] = (x, 2, _chunks('997', sr, LONG, None)), (ref, J0 * new)
    got, _ = _run_feeds(bank, plan)
    for s, (ref, g0) in refs.items():
        assert torch.equal(got[s], ref), s  # the samples from global index J0 new on
        assert bank.state(s).emitted == g0 + ref.shape[0]
    assert len(got) == 8


def test_two_pushes_without_a_wait_equal_two_with_one(feeds):
    """The carry is double-buffered: a push may be queued while the previous
    one is still running."""
    from sad.stream import StreamIngest
    outs = []
    for wait in (False, True):
        bank = StreamIngest(3, WINDOW, HOP, MAX_CHUNK, DEV)
        slots, xs = [], []
        for sr in (44100, 48000, 32000):
            x, _ = feeds[(LONG, sr, np.int16, 2)]
            slots.append(bank.open(str(sr), sr, 2, np.int16))
            xs.append(x)
        for k in range(4):
            bank.ingest({s: x[k * 2 * 1000:(k + 1) * 2 * 1000] for s, x in zip(slots, xs)})
            if wait:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        outs.append([bank.read(s, 0, bank.state(s).emitted) for s in slots])
        assert all(o.shape[0] > 2000 for o in outs[-1])
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    for (sr, o) in zip((44100, 48000, 32000), outs[0]):
        assert torch.equal(o, feeds[(LONG, sr, np.int16, 2)][1][:o.shape[0]])
