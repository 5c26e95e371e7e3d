"""Host side of the evidence maps (include/sad.h "evidence"):
the axes of a [16, 16] map and the per-file timeline.  No device work here.

A map's rows follow the front end's map rows (row m of [n_mels, frames] is mel
filter m, lowest band first) through the stem's resize and the backbone's
strides: row y is centred on mel filter y n_mels / 16 (``row_filters``), column
x on second x window / 16 of the window.  ``col_sec`` and ``timeline`` use the
nominal grid, column x = [x, x + 1) window / 16.
"""
from __future__ import annotations

import numpy as np

GRID = 16  # layer4's output is 16 x 16 for a 512 x 512 image


def col_sec(window_sec: float) -> np.ndarray:
    """Start (s, within the window) of each of the 16 columns."""
    return np.arange(GRID, dtype=np.float64) * (float(window_sec) / GRID)


def row_filters(y: int, n_mels: int):
    """[lo, hi): the mel filters row y of a map is centred on.  Every strided
    layer of the backbone (7x7/2 pad 3, 3x3/2 pad 1 pool and convs) centres
    output i on input 2 i, so cell y of layer4 is centred on image row 32 y --
    map row y n_mels / 16 -- not on the middle of the image rows [32 y, 32 y +
    32): the cell's band is the n_mels / 16 filters AROUND that row, clipped at
    the ends (row 0 has only the upper half; the last row also takes the
    half band above it, which no cell is centred on)."""
    per = n_mels // GRID
    return max(0, y * per - per // 2), (n_mels if y == GRID - 1 else y * per + per // 2)


def row_hz(fbank, sample_rate: int) -> np.ndarray:
    """[16, 2] float64: the (lowest, highest) frequency in Hz that carries a
    non-zero weight in any mel filter of the row (``row_filters``), read off the filterbank the
    front-end plan was built with (fbank [n_freqs, n_mels], bin k at
    k (sample_rate / 2) / (n_freqs - 1) Hz).  Neighbouring rows overlap as the
    triangles do.  A row whose filters are all zero gets (nan, nan)."""
    fb = np.asarray(fbank, dtype=np.float64)
    n_freqs, n_mels = fb.shape
    if n_mels % GRID:
        raise ValueError(f'n_mels = {n_mels} is not a multiple of {GRID}')
    hz = np.arange(n_freqs, dtype=np.float64) * (sample_rate / 2.0) / (n_freqs - 1)
    per = n_mels // GRID
    out = np.full((GRID, 2), np.nan)
    for y in range(GRID):
        lo, hi = row_filters(y, n_mels)
        used = np.nonzero((fb[:, lo:hi] > 0).any(axis=1))[0]
        if used.size:
            out[y] = hz[used[0]], hz[used[-1]]
    return out


def timeline(evidence, timestamps, window_sec: float) -> np.ndarray:
    """Per-file view of evidence [W, N, 16, 16] whose windows start at
    timestamps [W] (s): [N, bins] float64, bin width window / 16.  A bin is the
    mean, over every (window, column) whose CENTRE falls in it, of the column's
    sum over the rows; overlapping windows average.  bins reaches the last
    window's end; a bin no column centre falls in is nan."""
    e = np.asarray(evidence, dtype=np.float64)
    ts = np.asarray(timestamps, dtype=np.float64)
    W, N = e.shape[0], e.shape[1]
    width = float(window_sec) / GRID
    if W == 0:
        return np.zeros((N, 0))
    centre = ts[:, None] + (np.arange(GRID) + 0.5) * width          # [W, 16]
    bin_of = np.floor(centre / width + 1e-9).astype(np.int64)
    bins = int(bin_of.max()) + 1
    cols = e.sum(axis=2)                                             # [W, N, 16]
    total = np.zeros((N, bins))
    count = np.zeros(bins)
    for w in range(W):
        for x in range(GRID):
            total[:, bin_of[w, x]] += cols[w, :, x]
            count[bin_of[w, x]] += 1
    with np.errstate(invalid='ignore', divide='ignore'):
        return np.where(count > 0, total / count, np.nan)
