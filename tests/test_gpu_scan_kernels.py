"""GPU: the catalogue-scan kernels (csrc/scan.hip).

* sad_scan_select_run over an arena of several files == sad.ingest.select_windows
  run per file on the same samples: kept offsets and CSR row ranges, exactly
  (the maximum is exact, the test is one fp32 compare).
* sad_scan_post_run == inference_runner.summarize per file: probabilities within
  1e-6, percentages within 1e-3 percent units, identical labels on every row
  (no oracle row lies within 1e-5 of a decision boundary), zeros for a file
  without rows, identical bytes from run to run.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
WIN = 4096
THR = 1e-3


def _files():
    """Six files (fp32, already padded as the scanner pads them)."""
    rng = np.random.RandomState(7)
    thr = np.float32(THR)
    below = np.nextafter(thr, np.float32(0))
    loud = lambda n: (rng.standard_normal(n) * 0.1).astype(np.float32)
    quiet = lambda n: (rng.standard_normal(n) * 1e-5).astype(np.float32)
    f0 = np.concatenate([loud(3000), np.zeros(WIN - 3000, np.float32)])  # shorter than a window, padded to one
    f1 = loud(WIN)                                                       # exactly one window
    f2 = np.concatenate([loud(WIN), quiet(WIN), loud(WIN + 1234)])       # a silent window in the middle
    f3 = np.concatenate([quiet(WIN), quiet(WIN)])
    f3[WIN - 1] = -thr            # window 0: max == threshold exactly -> kept
    f3[WIN + 17] = below          # window 1: max one ulp below -> dropped
    f4 = quiet(3 * WIN + 99)                                             # all silent
    f5 = loud(160 * WIN + 321)    # 1061 candidates at hop 614: the compaction passes a 1024-candidate tile
    for w in (3, 4, 5, 40, 41, 42, 43, 100, 158):
        f5[w * WIN:(w + 1) * WIN] = quiet(WIN)
    f5[41 * WIN + 5] = np.nan     # NaN propagates into the maximum: the window is kept
    return [f0, f1, f2, f3, f4, f5], (thr, below)


def _arena(files, gaps):
    """Files back to back with `gaps[i]` loud filler samples before file i (so a
    read past a file's end would change a decision)."""
    parts, starts, pos = [], [], 0
    for f, g in zip(files, gaps):
        parts.append(np.full(g, 10.0, np.float32))
        pos += g
        starts.append(pos)
        parts.append(f)
        pos += len(f)
    return np.concatenate(parts), starts


@pytest.mark.parametrize('hop,overlap', [(4096, 0.0), (614, 0.85)])
def test_select_matches_select_windows_per_file(hop, overlap):
    from sad import scan as sc
    from sad.ingest import select_windows
    files, (thr, below) = _files()
    assert int((1 - overlap) * WIN) == hop
    arena_np, starts = _arena(files, [0, 1, 2, 3, 4, 5])  # every float4 misalignment of a file start
    arena = torch.from_numpy(arena_np).to(DEV)
    want_off, want_rows = [], [0]
    for f, (x, s) in enumerate(zip(files, starts)):
        kept, _ = select_windows(arena[s:s + len(x)], WIN, 1.0, overlap, THR)  # sr = WIN: a 1 s window
        if hop == WIN:
            if f == 2:
                assert kept == [0, 2 * WIN]
            if f == 3:
                assert kept == [0]
            if f == 4:
                assert kept == []
        want_off += [s + k for k in kept]
        want_rows.append(len(want_off))
    cap = sum(sc.candidate_count(len(x), WIN, hop) for x in files)
    assert (cap > 1024) == (hop == 614)
    fs = torch.tensor(starts, dtype=torch.int64, device=DEV)
    fl = torch.tensor([len(x) for x in files], dtype=torch.int64, device=DEV)
    runs = []
    for _ in range(2):
        off, rows = sc.select_windows_arena(arena, fs, fl, WIN, hop, THR, cap)
        runs.append((off.cpu(), rows.cpu()))
    off, rows = runs[0]
    assert rows.tolist() == want_rows
    assert off[:rows[-1]].tolist() == want_off
    assert torch.equal(runs[1][1], rows) and torch.equal(runs[1][0][:rows[-1]], off[:rows[-1]])


def test_select_many_small_files_and_bad_extents():
    """More files than one block scans at once; files that do not lie inside the
    arena, or are shorter than a window, have no candidates and read nothing."""
    from sad import scan as sc
    rng = np.random.RandomState(3)
    n = 300
    loud = rng.rand(n) < 0.6
    arena_np = np.where(np.repeat(loud, WIN), 0.5, 0.0).astype(np.float32)
    starts = [i * WIN for i in range(n)]
    lens = [WIN] * n
    starts += [-4, n * WIN - 100, 0, 1 << 50]   # before the arena, past its end, short, far outside
    lens += [WIN, WIN, WIN - 1, WIN]
    arena = torch.from_numpy(arena_np).to(DEV)
    fs = torch.tensor(starts, dtype=torch.int64, device=DEV)
    fl = torch.tensor(lens, dtype=torch.int64, device=DEV)
    off, rows = sc.select_windows_arena(arena, fs, fl, WIN, WIN, THR, n)
    rows = rows.cpu()
    kept = [i * WIN for i in range(n) if loud[i]]
    assert rows.tolist() == [0] + np.cumsum(loud).tolist() + [len(kept)] * 4
    assert off.cpu()[:len(kept)].tolist() == kept


# ---- post-processing ----------------------------------------------------------
LENS = [1, 2, 3, 0, 8, 9, 16, 17, 18, 33, 64, 65, 300]
_ORACLE = {}


def _oracle(C, smooth):
    """summarize per file (labels, percentages) and the probabilities it forms
    on the way, restated with the same calls (it does not return them)."""
    key = (C, smooth)
    if key in _ORACLE:
        return _ORACLE[key]
    import inference_runner as ir
    from scipy.ndimage import gaussian_filter1d
    g = torch.Generator().manual_seed(2)
    logits = torch.randn(sum(LENS), C, generator=g) * 3
    syn, real = [f'S{k}' for k in range(C - 1)], 'Real'
    ids = {name: k for k, name in enumerate(syn)}
    ids[real] = -1
    probs, labels, pct, lo = [], [], [], 0
    for n in LENS:
        rows = logits[lo:lo + n]
        lo += n
        if n == 0:
            pct.append(None)
            continue
        rec = ir.summarize('f', rows, [0.0] * n, 0.5, syn, real, smooth, 4.0)
        labels += [ids[s['label']] for s in rec['segments']]
        pct.append([rec['percentages'][k] for k in syn + [real]])
        p = np.array([ir.interpret_multihead_logits(r, 0.5, syn, real)[1] for r in rows])
        assert p.dtype == np.float32
        if smooth:
            for d in range(C):
                p[:, d] = gaussian_filter1d(p[:, d], sigma=2)
            for i in range(n):
                s = p[i].sum()
                if s > 0:
                    p[i] /= s
        probs.append(p)
    out = (logits, np.concatenate(probs), np.array(labels, np.int32), pct)
    _ORACLE[key] = out
    return out


@pytest.mark.parametrize('smooth', [False, True])
@pytest.mark.parametrize('C', [2, 7])
def test_post_matches_summarize(C, smooth):
    from sad import scan as sc
    logits, want_p, want_l, want_pct = _oracle(C, smooth)
    row_start = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int64, device=DEV)
    dl = logits.to(DEV)
    runs = []
    for _ in range(2):
        p, l, m = sc.postprocess(dl, row_start, 0.5, smooth)
        runs.append((p.cpu().numpy(), l.cpu().numpy(), m.cpu().numpy()))
    p, l, m = runs[0]
    err = np.abs(p.astype(np.float64) - want_p.astype(np.float64)).max()
    print(f'C={C} smooth={smooth}: max |dprob| = {err:.3e}')
    assert err <= 1e-6
    # rows near a decision boundary would be excluded from the label check: there are none
    thr_margin = np.abs(want_p - np.float32(0.5)).min(axis=1)
    ok = thr_margin > 1e-5
    if C > 2:
        top2 = np.sort(want_p[:, :-1], axis=1)[:, -2:]
        ok &= (top2[:, 1] - top2[:, 0]) > 1e-5
    assert ok.all()
    assert np.array_equal(l, want_l)
    for f, (n, ref) in enumerate(zip(LENS, want_pct)):
        if n == 0:
            assert (m[f] == 0).all()  # zeros, never NaN
            continue
        d = np.abs(m[f] * 100 - np.array(ref)).max()
        assert d <= 1e-3, (f, n, d)
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()


def test_post_smoothing_stops_at_file_boundaries():
    """A file's smoothed rows depend on its own rows only: the same rows in
    another neighbourhood, or alone, give the same bytes."""
    from sad import scan as sc
    logits, _, _, _ = _oracle(7, True)
    dl = logits.to(DEV)
    row_start = torch.tensor(np.concatenate([[0], np.cumsum(LENS)]), dtype=torch.int64, device=DEV)
    p, l, m = sc.postprocess(dl, row_start, 0.5, True)
    lo = sum(LENS[:9])  # the 33-row file, alone
    one = dl[lo:lo + 33].contiguous()
    p1, l1, m1 = sc.postprocess(one, torch.tensor([0, 33], dtype=torch.int64, device=DEV), 0.5, True)
    assert torch.equal(p1, p[lo:lo + 33]) and torch.equal(l1, l[lo:lo + 33]) and torch.equal(m1[0], m[9])
