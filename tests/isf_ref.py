"""float64 numpy restatement of amof_isf_accumulate (include/amof_hip.h), on top of tests/sq_ref.py.  ``isf`` works from the
positions (fractional coordinates solve(cell.T, pos.T) in float64, not the library's u32 values); ``isf_from_modes`` builds,
from a table of rho the library itself returned, the int64 fixed-point sums the library must then produce bit for bit.
Test infrastructure only (the package never imports it)."""

import numpy as np

from tests import helpers as H
from tests import sq_ref


def origins(F, m, stride=1):
    """k = 1, 1 + s, ... <= F - m - 1"""
    return list(range(1, max(F - m, 1), stride))


def work_entries(F, windows, stride=1, work_range=None):
    """[(lag index, origin frame)] of the lag-major work list, cut to ``work_range``"""
    ent = [(w, k) for w, m in enumerate(windows) for k in origins(F, int(m), stride)]
    return ent if work_range is None else ent[work_range[0]:work_range[1]]


def pair_scale(scale_log2, S):
    """[S][S] exponent of the unordered pair {a, c} from the library's [P] list ((0,0), (0,1) .. (0,S-1), (1,1) ..)"""
    out, p = np.zeros((S, S), dtype=np.int64), 0
    for a in range(S):
        for c in range(a, S):
            out[a, c] = out[c, a] = scale_log2[p]
            p += 1
    return out


def _frac(pos, cell):
    return np.linalg.solve(np.asarray(cell, dtype=np.float64).T, np.asarray(pos, dtype=np.float64).T).T


def isf(packed, hkl, windows, dq, nbins, origin_stride=1, work_range=None):
    """(counts [W][nbins] int64, coh [S][S][W][nbins], self [S][W][nbins], beyond [W] int64, kinds)"""
    kinds, species = H.species_of(packed.numbers)
    S, W = len(kinds), len(windows)
    pos = np.asarray(packed.pos_host(), dtype=np.float64)
    F = len(pos)
    cell = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3)
    hkl = np.asarray(hkl).reshape(-1, 3)
    cell_of = lambda f: cell[f if len(cell) > 1 else 0]
    counts = np.zeros((W, nbins), dtype=np.int64)
    coh = np.zeros((S, S, W, nbins))
    selfs = np.zeros((S, W, nbins))
    beyond = np.zeros(W, dtype=np.int64)
    rho = {}

    def modes(f):
        if f not in rho:
            rho[f] = sq_ref.modes(pos[f], cell_of(f), species, S, hkl)
        return rho[f]

    for w, k in work_entries(F, windows, origin_stride, work_range):
        m = int(windows[w])
        b = sq_ref.bins(sq_ref.reciprocal(cell_of(k)), hkl, dq, nbins)
        ok = b < nbins
        beyond[w] += int((~ok).sum())
        counts[w] += np.bincount(b[ok], minlength=nbins)
        r0, r1 = modes(k), modes(k + m)
        for a in range(S):
            for c in range(S):
                t = r0[:, a].real * r1[:, c].real + r0[:, a].imag * r1[:, c].imag
                coh[a, c, w] += np.bincount(b[ok], weights=t[ok], minlength=nbins)
        # the phase of every atom's own displacement, in fractional coordinates of each frame's own cell
        ds = _frac(pos[k + m], cell_of(k + m)) - _frac(pos[k], cell_of(k))
        cs = np.cos(2.0 * np.pi * (hkl.astype(np.float64) @ ds.T))        # [K][N]
        for a in range(S):
            u = cs[:, species == a].sum(axis=1)
            selfs[a, w] += np.bincount(b[ok], weights=u[ok], minlength=nbins)
    return counts, coh, selfs, beyond, kinds


def isf_from_modes(rho, bins, scale_log2, windows, nbins, origin_stride=1, work_range=None):
    """(counts [W][nbins], coh [S][S][W][nbins] int64, beyond [W]): the library's integer sums from ITS rho table.

    rho: complex [F][K][S] (``Context.sq_modes`` of every frame); bins: int [F][K] or [1][K] (``sq_ref.bins`` per origin
    frame's reciprocal matrix, nbins = beyond); scale_log2: the [P] exponents the library returned.  Exactly
    (re_a * re_c) + (im_a * im_c), np.rint of the scaled value, int64 addition."""
    rho = np.asarray(rho)
    F, K, S = rho.shape
    W = len(windows)
    exp2 = pair_scale(scale_log2, S)
    counts = np.zeros((W, nbins), dtype=np.int64)
    coh = np.zeros((S, S, W, nbins), dtype=np.int64)
    beyond = np.zeros(W, dtype=np.int64)
    bins = np.asarray(bins)
    for w, k in work_entries(F, windows, origin_stride, work_range):
        m = int(windows[w])
        b = bins[k if len(bins) > 1 else 0]
        ok = b < nbins
        beyond[w] += int((~ok).sum())
        counts[w] += np.bincount(b[ok], minlength=nbins)
        for a in range(S):
            for c in range(S):
                t = (rho[k, :, a].real * rho[k + m, :, c].real) + (rho[k, :, a].imag * rho[k + m, :, c].imag)
                v = np.rint(t * np.ldexp(1.0, int(exp2[a, c]))).astype(np.int64)
                np.add.at(coh[a, c, w], b[ok], v[ok])
    return counts, coh, beyond
