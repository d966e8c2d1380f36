"""The tight cut of the wet-row table (round 8, csrc/gcmf_wet_cut.hpp: wet_cut_tight) restated in numpy -- shared by tests/test_wet_cut.py
(the planner header alone, compiled with g++) and tests/test_gpu_wet_tight.py (the launches).  Not an independent derivation: it pins the
geometry a mask must give, so that a change of the rules shows.

Rules, for a launch of S levels (windows own WI = 108 columns at S = 9, 112 at S <= 8) over the rows [0, ny) of a grid periodic in x and y:

  * the window grid starts at column xoff, one of 0, 2, .., WI - 2: window wx owns the columns [xoff + wx WI, min(xoff + (wx + 1) WI,
    xoff + nx)) mod nx;
  * row r of window wx is needed iff one of the window's OWNED columns holds a cell that exchanges with a neighbour;
  * runs = the maximal runs of needed rows; two runs of a window less than S + 1 rows apart are bridged; then a run shorter than 4 rows is
    extended upwards to 4 (and shifted down where it would pass the last row); runs that touch are merged; none is joined across the y wrap;
  * pairs_of(len, H) = max(1, min(len // 4, ceil(len / 2H))); H = the smallest at which all pairs fit 512 slots; runs are cut evenly;
  * of all offsets (those with more than 512 runs are out): the smallest march, then the fewest owned window-rows, then the smallest offset.
"""
import numpy as np

from gcm_filters_amd import testing as T


def exchanging(wet):
    """Bit 0 of the plan's land byte for kappa = 1 on a periodic grid: the cell is wet and so is one of its four neighbours."""
    return (wet == 1) & ~T.closed_in_cells(wet)


def window_width(S):
    return 128 - 4 * ((S + 1) // 2)


def zip_rows(need, S):
    """ringc_zip_rows (csrc/gcmf_ringc_cut.hpp): rows a zipped march of `need` rows runs."""
    ex = 2 if S <= 8 else 4
    return min(max(12, -(-need // ex) * ex), -(-need // 12) * 12)


def runs_of(need, S):
    """[lo, hi) runs of one window's needed rows."""
    ny = len(need)
    runs, r = [], 0
    while r < ny:
        if not need[r]:
            r += 1
            continue
        e = r
        while e < ny and need[e]:
            e += 1
        if runs and r - runs[-1][1] < S + 1:
            runs[-1][1] = e
        else:
            runs.append([r, e])
        r = e
    for run in runs:
        if run[1] - run[0] < 4:
            run[1] = run[0] + 4
            if run[1] > ny:
                run[0], run[1] = max(0, ny - 4), ny
    merged = []
    for lo, hi in sorted(runs):
        if merged and lo <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], hi)
        else:
            merged.append([lo, hi])
    return merged


def cut_at(csum, S, xoff):
    """(march, owned window-rows, pairs, tallest strip, twice the most pairs of a window) at one offset, or None (more than 512 runs);
    csum[r, i] = exchanging cells of row r in the columns [0, i)."""
    ny, nx = csum.shape[0], csum.shape[1] - 1
    WI = window_width(S)
    nwx = -(-nx // WI)
    runs = []
    for wx in range(nwx):
        c0 = xoff + wx * WI
        c1 = min(c0 + WI, xoff + nx)
        a, b = c0 % nx, c0 % nx + (c1 - c0)
        cnt = csum[:, b] - csum[:, a] if b <= nx else (csum[:, nx] - csum[:, a]) + csum[:, b - nx]
        runs += [(wx, hi - lo) for lo, hi in runs_of(cnt > 0, S)]
    if len(runs) > 512:
        return None
    pairs = lambda n, H: max(1, min(n // 4, -(-n // (2 * H))))
    H = 2
    while sum(pairs(n, H) for _, n in runs) > 512:
        H += 1
    per_window, tallest = {}, 0
    for wx, n in runs:
        k = pairs(n, H)
        per_window[wx] = per_window.get(wx, 0) + k
        for p in range(k):
            h = (p + 1) * n // k - p * n // k
            tallest = max(tallest, h - h // 2)
    return (zip_rows(tallest + S + 1, S), sum(n for _, n in runs), sum(per_window.values()), tallest, 2 * max(per_window.values(), default=0))


def model(wet, S, xoffs=None):
    """(pairs, tallest strip, nstrips, xoff, march) of the tight table of a launch of S levels over the whole grid."""
    opened = exchanging(wet)
    csum = np.concatenate([np.zeros((opened.shape[0], 1), np.int32), np.cumsum(opened, axis=1, dtype=np.int32)], axis=1)
    best = None
    for xoff in (range(0, window_width(S), 2) if xoffs is None else xoffs):
        c = cut_at(csum, S, xoff)
        if c is not None and (best is None or c[:2] < best[0][:2]):
            best = (c, xoff)
    (march, _, units, tallest, nstrips), xoff = best
    return units, tallest, nstrips, xoff, march
