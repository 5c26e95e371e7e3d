"""CPU: the host half of live streams (sad/stream.py): the emission rule against
a brute-force enumeration of tap indices, its parity with sad.audio.resample,
the push arena with its tables, and the argument checks of the new C entries
(no device work: there is no GPU here)."""
import ctypes
import math

import numpy as np
import torch

RATES = (44100, 22050, 48000, 16000, 8000, 96000, 11025, 32000)
PAST_2_32 = [(1 << 32) + 1, (1 << 32) + 12345, (1 << 33) + 7, (1 << 35) - 3, 86400 * 96000 + 11]


def _brute_frames_done(F, orig, width, K):
    """Polyphase frames whose K tap indices j orig - width + k all lie below F,
    by looking at the tap indices of the frames around F / orig."""
    lo = max(0, F // orig - -(-K // orig) - 2)
    taps = lambda j: [j * orig - width + k for k in range(K)]
    assert lo == 0 or max(taps(lo - 1)) < F  # every earlier frame is complete: the last tap index grows with j
    complete = [max(taps(j)) < F for j in range(lo, F // orig + 3)]
    done = lo
    for c in complete:
        if not c:
            break
        done += 1
    assert not any(complete[done - lo:])  # monotone: no later frame is complete
    return done


def test_emission_rule_against_brute_force_tap_enumeration():
    from sad import stream
    from sad.ingest import resample_geometry
    cases = 0
    window, hop = 4096, 613
    for sr in RATES:
        orig, new, width, K = resample_geometry(sr)
        assert K == 2 * width + orig and width == math.ceil(6 * orig / (min(orig, new) * 0.99))
        values = list(range(0, 3 * K + 1)) + PAST_2_32
        for F in values:
            if sr == 32000:
                assert stream.ready(F, sr) == F
                emitted = F
            else:
                J = _brute_frames_done(F, orig, width, K)
                assert stream.frames_done(F, sr) == J, (sr, F)
                assert stream.ready(F, sr) == J * new, (sr, F)
                emitted = J * new
            # windows whose last sample is emitted: slice_waveform's range over what exists so far
            assert stream.window_count(emitted, window, hop) == len(range(0, emitted - window + 1, hop)), (sr, F)
            cases += 1
        # a feed joined at start_frame: nothing below g0, the same frames from there on
        J0 = 5 * hop
        start = J0 * orig
        assert stream.first_sample(start, sr) == J0 * new
        for F in (start, start + 1, start + width, start + K, start + 3 * K):
            want = F if sr == 32000 else max(_brute_frames_done(F, orig, width, K), J0) * new
            assert stream.ready(F, sr, start_frame=start) == want, (sr, F)
            cases += 1
    assert cases == sum(3 * resample_geometry(sr)[3] + 1 + len(PAST_2_32) + 5 for sr in RATES)
    # incremental counting: the windows found tick by tick are the whole range's
    first, found = 0, 0
    for emitted in range(0, 30000, 777):
        c = stream.window_count(emitted, window, hop, first)
        first += c * hop
        found += c
    assert found == len(range(0, 29526 - window + 1, hop)) and 29526 == max(range(0, 30000, 777))


def _polyphase64(x, sr):
    """resample(x, sr, 32000) with the float64 kernel, summed tap by tap in ascending k."""
    from sad import audio
    g = math.gcd(sr, 32000)
    kern, width = audio._sinc_resample_kernel(sr, 32000, g)
    kern = kern[:, 0, :].double().numpy()
    orig, new, K = sr // g, 32000 // g, kern.shape[1]
    n_out = -(-new * x.shape[0] // orig)
    m = np.arange(n_out)
    j, p = m // new, m % new
    xp = np.concatenate([np.zeros(width), x.astype(np.float64), np.zeros(width + orig + K)])
    acc = np.zeros(n_out)
    for k in range(K):
        acc = acc + xp[j * orig + k] * kern[p, k]
    return acc


def test_ready_outputs_do_not_change_when_input_is_appended():
    from sad import audio, stream
    from sad.ingest import resample_geometry
    rng = np.random.default_rng(11)
    cases = 0
    for sr in RATES:
        if sr == 32000:
            continue
        orig, new, width, K = resample_geometry(sr)
        T = 4 * K + 3 * orig + 17
        x = rng.standard_normal(T).astype(np.float32)
        full = _polyphase64(x, sr)
        ref = audio.resample(torch.from_numpy(x)[None], sr, 32000)[0]
        n_out, end = stream.final_end(T, sr, 4096)
        assert ref.shape[0] == full.shape[0] == n_out and end == max(n_out, 4096)
        # fp32 conv1d against the float64 sum of the same fp32 kernel: K products of |x| < 6, |w| < 1
        assert np.abs(ref.double().numpy() - full).max() <= 1e-4
        for F in (0, 1, width - 1, width, width + 1, width + orig, K, 2 * K + 1, T - 1, T):
            r = stream.ready(F, sr)
            assert r <= n_out
            head = _polyphase64(x[:F], sr)
            assert np.array_equal(head[:r], full[:r]), (sr, F)
            # and ready(F) is tight: with orig more frames the next polyphase frame is complete
            assert stream.ready(F + orig, sr) == r + new or F < width
            cases += 1
    assert cases == 70


def test_push_arena_alignment_and_tables_round_trip():
    from sad import _lib, stream
    rng = np.random.default_rng(2)
    rows = [stream.PushRow(5, rng.integers(-9, 9, 2 * 1001).astype(np.int16), 0, False, 44100, 2),
            stream.PushRow(0, rng.standard_normal(3 * 333).astype(np.float32), 4096, False, 32000, 3, 0, 1),
            stream.PushRow(2, np.zeros(0, np.int16), 7000, True, 44100, 1, 441, 0),
            stream.PushRow(7, rng.integers(-9, 9, 77).astype(np.int16), 48000 * 3, False, 48000, 1, 48000 * 3, 1)]
    pack = stream.pack_push(rows, 4096)
    assert pack.rates == (44100, 32000, 48000)
    tab = pack.table
    sizes = [2 * 1001 * 2, 3 * 333 * 4, 0, 77 * 2]
    offs = [0]
    for s in sizes:
        offs.append(-(-(offs[-1] + s) // 16) * 16)
    I16, F32 = _lib.SAD_PCM_I16, _lib.SAD_PCM_F32
    assert tab.tolist() == [[5, offs[0], 1001, 0, 0, 0, 2, I16, 0, 0],
                            [0, offs[1], 333, 4096, 0, 1, 3, F32, 0, 1],
                            [2, offs[2], 0, 7000, 1, 0, 1, I16, 441, 0],
                            [7, offs[3], 77, 48000 * 3, 0, 2, 1, I16, 48000 * 3, 1]]
    assert all(o % 16 == 0 for o in tab[:, 1]) and pack.table_off == offs[4] and pack.tiles_off % 16 == 0
    assert pack.nbytes % 16 == 0 and pack.arena.shape[0] == pack.nbytes
    for row, r in zip(tab, rows):
        raw = pack.arena[row[1]:row[1] + r.samples.nbytes]
        assert np.array_equal(raw.view(r.samples.dtype), r.samples)
    # the tile table: every (row, tile) once, row by row; counts and spans as the library gives them
    lib = _lib.load()
    a, e, c = _lib.I64(), _lib.I64(), _lib.I64()
    want = []
    for i, r in enumerate(rows):
        assert lib.sad_stream_push_tiles(r.sr, 32000, r.start_frame, r.frames_before, r.frames, int(r.final), 4096,
                                         ctypes.byref(a), ctypes.byref(e), ctypes.byref(c)) == 0
        assert (a.value, e.value) == tuple(pack.spans[i]) == stream.push_span(r.sr, r.start_frame, r.frames_before,
                                                                              r.frames, r.final, 4096)
        assert c.value == stream.push_tiles(r.sr, r.start_frame, r.frames_before, r.frames, r.final, 4096)
        want += [[i, t] for t in range(c.value)]
    assert pack.tiles.tolist() == want and pack.n_tiles == len(want) > 4
    # the final row of the 7000-frame feed stores up to ceil(320 * 7000 / 441) = 5080 samples
    assert pack.spans[2][1] == 5080 and pack.spans[1].tolist() == [4096, 4096 + 333]


def test_tile_counts_and_spans_agree_with_the_library():
    from sad import _lib, stream
    lib = _lib.load()
    a, e, c, cap, alen, clen = (_lib.I64() for _ in range(6))
    n = 0
    for sr in RATES:
        for fb, k, fin in ((0, 0, 0), (0, 1, 0), (0, 1024, 0), (5000, 997, 0), (5000, 0, 1), (5000, 13, 1),
                           (100, 0, 1), ((1 << 33) + 5, 1024, 0), ((1 << 33) + 5, 0, 1)):
            assert lib.sad_stream_push_tiles(sr, 32000, 0, fb, k, fin, 4096, ctypes.byref(a), ctypes.byref(e),
                                             ctypes.byref(c)) == 0
            assert (a.value, e.value) == stream.push_span(sr, 0, fb, k, bool(fin), 4096), (sr, fb, k, fin)
            assert c.value == stream.push_tiles(sr, 0, fb, k, bool(fin), 4096), (sr, fb, k, fin)
            if not fin:
                assert (a.value, e.value) == (stream.ready(fb, sr), stream.ready(fb + k, sr))
            else:
                assert e.value == stream.final_end(fb + k, sr, 4096)[1]
            n += 1
    assert n == 72
    for window, chunk in ((4096, 1024), (128000, 4410), (128000, 1), (4096, 100000)):
        assert lib.sad_stream_bank_size(3, window, 613, chunk, 32000, ctypes.byref(cap), ctypes.byref(alen),
                                        ctypes.byref(clen)) == 0
        assert cap.value == stream.bank_cap(window, chunk) >= window + 4096 and cap.value % 4 == 0
        assert alen.value == 3 * 2 * cap.value and clen.value == 3 * 2 * stream.STREAM_CARRY
        for sr in RATES + (384000, 12345):
            g0 = _lib.I64()
            ok = lib.sad_stream_open_check(sr, 32000, 1, window, 613, cap.value, 0, ctypes.byref(g0)) == 0
            assert ok == stream.rate_supported(sr, cap.value, window), (sr, window, chunk)
            if ok:
                assert stream.piece_frames(sr, cap.value, window, chunk) >= 1
    assert not stream.rate_supported(384000, 8192, 4096) and stream.rate_supported(44100, 8192, 4096)


def test_argument_errors_of_the_new_entries():
    from sad import _lib
    lib = _lib.load()
    v = [_lib.I64() for _ in range(3)]
    r = [ctypes.byref(x) for x in v]

    def bad(rc, word):
        assert rc == -1 and word in lib.sad_last_error().decode(), lib.sad_last_error()

    # bank size
    bad(lib.sad_stream_bank_size(4, 4096, 613, 1024, 32000, None, r[1], r[2]), 'null')
    bad(lib.sad_stream_bank_size(0, 4096, 613, 1024, 32000, *r), 'slots')
    bad(lib.sad_stream_bank_size(4, 0, 613, 1024, 32000, *r), 'window')
    bad(lib.sad_stream_bank_size(4, 4096, 5000, 1024, 32000, *r), 'hop')
    bad(lib.sad_stream_bank_size(4, 4096, 613, 0, 32000, *r), 'max_chunk_frames')
    # opening a feed
    bad(lib.sad_stream_open_check(44100, 32000, 2, 4096, 613, 8192, 0, None), 'null')
    bad(lib.sad_stream_open_check(44100, 32000, 0, 4096, 613, 8192, 0, r[0]), 'channels')
    bad(lib.sad_stream_open_check(44100, 32000, 65, 4096, 613, 8192, 0, r[0]), 'channels')
    bad(lib.sad_stream_open_check(0, 32000, 2, 4096, 613, 8192, 0, r[0]), 'positive')
    bad(lib.sad_stream_open_check(384000, 32000, 2, 4096, 613, 8192, 0, r[0]), 'not supported by the batched kernel')
    bad(lib.sad_stream_open_check(11025, 32000, 2, 4096, 613, 4096 + 2000, 0, r[0]), 'not supported by this bank')
    bad(lib.sad_stream_open_check(44100, 32000, 2, 4096, 613, 4092, 0, r[0]), 'window > CAP')
    bad(lib.sad_stream_open_check(44100, 32000, 2, 4096, 613, 8192, 440, r[0]), 'multiple of orig')
    bad(lib.sad_stream_open_check(44100, 32000, 2, 4096, 613, 8192, 441, r[0]), 'multiple of hop')
    bad(lib.sad_stream_open_check(32000, 32000, 2, 4096, 613, 8192, 612, r[0]), 'multiple of hop')
    assert lib.sad_stream_open_check(44100, 32000, 2, 4096, 613, 8192, 441 * 613, r[0]) == 0
    assert v[0].value == 320 * 613
    # tile helper
    bad(lib.sad_stream_push_tiles(44100, 32000, 0, 0, 10, 0, 4096, None, None, None), 'null')
    bad(lib.sad_stream_push_tiles(384000, 32000, 0, 0, 10, 0, 4096, None, None, r[0]), 'not supported')
    bad(lib.sad_stream_push_tiles(44100, 32000, 441, 440, 10, 0, 4096, None, None, r[0]), 'frames')
    bad(lib.sad_stream_push_tiles(44100, 32000, 0, 0, -1, 0, 4096, None, None, r[0]), 'frames')
    bad(lib.sad_stream_push_tiles(44100, 32000, 7, 7, 1, 0, 4096, None, None, r[0]), 'multiple of orig')
    # the launch: rate 0 is the target rate (no plan, no device memory)
    plans = (ctypes.c_void_p * 1)(None)
    fake = 0x1000  # a non-null "device" pointer: the checks return before any device work

    def run(rows, chunk_bytes=8192, n_tiles=1, chunks=fake, arena=fake, carry=fake, n_rates=1, table=True, slots=4,
            cap=8192, window=4096):
        t = np.array(rows, np.int64)
        return lib.sad_stream_push_run(chunks, chunk_bytes, t.ctypes.data if table else None, fake, len(rows), fake,
                                       n_tiles, plans, n_rates, arena, carry, slots, cap, window, None)

    good = [1, 0, 100, 0, 0, 0, 1, 0, 0, 0]

    def row(**kw):
        cols = ['slot', 'off', 'n', 'fb', 'final', 'ri', 'ch', 'enc', 'start', 'par']
        out = list(good)
        for k, val in kw.items():
            out[cols.index(k)] = val
        return out

    bad(run([good], chunks=None), 'null')
    bad(run([good], arena=None), 'null')
    bad(run([good], carry=None), 'null')
    bad(run([good], table=False), 'null')
    bad(run([good], n_rates=0), 'n_rates')
    bad(run([good], n_rates=9), 'n_rates')
    bad(run([good], window=8196), 'window > CAP')
    bad(run([good], cap=8190, window=4096), 'multiple of 4')
    bad(run([good], slots=0), 'slots')
    bad(run([row(slot=4)]), 'slot out of range')
    bad(run([row(slot=-1)]), 'slot out of range')
    bad(run([good, good], n_tiles=2), 'twice')
    bad(run([row(ch=0)]), 'channels')
    bad(run([row(ch=65)]), 'channels')
    bad(run([row(enc=2)]), 'encoding')
    bad(run([row(ri=1)]), 'rate index')
    bad(run([row(final=2)]), 'final')
    bad(run([row(par=2)]), 'parity')
    bad(run([row(off=8)]), 'multiple of 16')
    bad(run([row(off=8192, n=1)]), 'past the end')
    bad(run([row(off=8000)]), 'past the end')
    bad(run([row(n=-1)]), 'frames')
    bad(run([row(fb=5, start=6)]), 'frames')
    bad(run([row(fb=8192, n=4097)], chunk_bytes=1 << 20, n_tiles=5), 'CAP - window')
    bad(run([good], n_tiles=2), 'n_tiles')
    bad(run([good] * 5, slots=4), 'n_rows')
