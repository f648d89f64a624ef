"""Reference counts of the distinct Van Hove function (test infrastructure; the package never imports it).

Built on the C oracle's RDF (``oracle.clib.rdf_hist``) alone: frame k and frame k + m become ONE frame of 2N atoms in
frame k's cell and pbc, the second copy's species shifted by S.  The oracle's cross partial [a][S + b] then holds every pair
(i at k, j at k + m) through the canonical arithmetic, every image in reach included, and the atom's own pairs (i, i) too.
Those are taken back exactly with a batch of 2-atom frames (r_i(k), r_i(k + m)) through the same oracle.  Lag-major over
the work list of ``amof_amd.lags.work_list``; ``work_range`` selects entries of it."""

import numpy as np

from amof_amd.lags import work_list
from oracle import clib


def species(numbers):
    kinds = sorted(set(int(z) for z in numbers))
    return kinds, np.array([kinds.index(int(z)) for z in numbers], dtype=np.int32)


def distinct_hist(pos, cell, numbers, windows, rmax, nbins, origin_stride=1, pbc=(True, True, True), work_range=None):
    """``hist u64 [S][S][W][nbins]`` (species in sorted atomic-number order, the library's)"""
    pos = np.asarray(pos, dtype=np.float64)
    F, N = pos.shape[:2]
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    kinds, sp = species(numbers)
    S, W = len(kinds), len(windows)
    hist = np.zeros((S, S, W, nbins), dtype=np.int64)
    wl, kl = work_list(F, windows, origin_stride)
    lo, hi = (0, len(wl)) if work_range is None else work_range
    sp2 = np.concatenate([sp, sp + S]).astype(np.int32)
    for q in range(lo, hi):
        w, k = int(wl[q]), int(kl[q])
        km = k + int(windows[w])
        C = cells[0 if len(cells) == 1 else k]
        both = np.concatenate([pos[k], pos[km]])
        h, _ = clib.rdf_hist(both, C, sp2, 2 * S, rmax, nbins, pbc=pbc)
        cross = h[:S, S:].astype(np.int64)
        for a in range(S):
            sel = sp == a
            two = np.stack([pos[k][sel], pos[km][sel]], axis=1)            # [N_a][2][3]: one frame per atom
            h2, _ = clib.rdf_hist(two, C, np.array([0, 1], np.int32), 2, rmax, nbins, pbc=pbc)
            cross[a, a] -= h2[0, 1].astype(np.int64)
        hist[:, :, w] += cross
    assert hist.min() >= 0
    return hist.astype(np.uint64)


def numpy_hist(pos, cell, numbers, windows, rmax, nbins, origin_stride=1):
    """plain float64 double loop (minimum image by rint of the fractional difference; rmax below half every height, so no
    further image): the restatement the oracle construction is checked against on a few dozen atoms"""
    pos = np.asarray(pos, dtype=np.float64)
    F, N = pos.shape[:2]
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    kinds, sp = species(numbers)
    S, W = len(kinds), len(windows)
    dr = rmax / nbins
    hist = np.zeros((S, S, W, nbins), dtype=np.uint64)
    wl, kl = work_list(F, windows, origin_stride)
    for w, k in zip(wl, kl):
        C = cells[0 if len(cells) == 1 else k]
        inv = np.linalg.inv(C)
        km = k + int(windows[w])
        for i in range(N):
            for j in range(N):
                if i == j:
                    continue
                d0 = pos[km, j] - pos[k, i]
                d = d0 - np.rint(d0 @ inv) @ C
                d2 = float(d @ d)
                if d2 < rmax * rmax:
                    b = int(np.sqrt(d2) / dr)
                    if b < nbins:
                        hist[sp[i], sp[j], w, b] += 1
    return hist
