"""numpy restatement of amof_vanhove_window (include/amof_hip.h): the displacements of oracle.numpy_oracle.window_msd,
binned.  Test infrastructure only (the package never imports it)."""

import numpy as np

from oracle import numpy_oracle as no
from tests import helpers as H

AMBIGUOUS = 1e-8       # Angstrom: a sample this close to a bin edge may land on either side (summation order of u)


def running_positions(packed, unwrap=False, remove_com=True):
    """u [F][N][3]: the running sums of the wrapped frame-to-frame displacements (u[0] = 0) of every atom, per species
    through oracle.numpy_oracle.get_delta_pos as window_msd forms them (centre of mass of ALL atoms removed first)"""
    pos = np.array(packed.pos_host(), dtype=np.float64)
    F = len(pos)
    cell = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3)
    cells = [cell[k if len(cell) > 1 else 0] for k in range(F)]
    pbc = tuple(bool(x) for x in packed.pbc)
    masses = np.asarray(packed.masses, dtype=np.float64)
    if unwrap:
        delta = no.get_delta_pos([pos[k].copy() for k in range(F)], cells, pbc)
        new_pos = pos[0].copy()
        for i in range(1, F):
            new_pos += delta[i]
            pos[i] = new_pos
    if remove_com:
        for k in range(F):
            pos[k] -= np.dot(masses, pos[k]) / masses.sum()
    _, sp = H.species_of(packed.numbers)
    u = np.zeros_like(pos)
    for s in np.unique(sp):
        sel = sp == s
        d = no.get_delta_pos([pos[k][sel] for k in range(F)], cells, pbc)
        d = np.array([np.zeros_like(d[0])] + [np.asarray(x) for x in d[1:]])
        u[:, sel] = np.cumsum(d, axis=0)
    return u


def vanhove(packed, windows, dr, nbins, unwrap=False, remove_com=True, atom_range=None):
    """(counts [S][W][nbins] u64, overflow [S][W] u64, moments [S][W][2], ambiguous [S][W][nbins], kinds) -- species in
    library order, atoms of ``atom_range`` only; ambiguous[s][w][b]: samples within AMBIGUOUS of an edge of bin b"""
    kinds, sp = H.species_of(packed.numbers)
    u = running_positions(packed, unwrap, remove_com)
    F, N = u.shape[0], u.shape[1]
    a0, a1 = (0, N) if atom_range is None else atom_range
    S, W = len(kinds), len(windows)
    counts = np.zeros((S, W, nbins), np.uint64)
    overflow = np.zeros((S, W), np.uint64)
    moments = np.zeros((S, W, 2))
    amb = np.zeros((S, W, nbins), np.int64)
    in_range = (np.arange(N) >= a0) & (np.arange(N) < a1)
    for s in range(S):
        us = u[:, (sp == s) & in_range]
        for w, m in enumerate(windows):
            m = int(m)
            d = us[m + 1:F] - us[1:F - m]          # origins k = 1 .. F-m-1
            r2 = ((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]).reshape(-1)
            moments[s, w] = (r2.sum(), (r2 * r2).sum())
            q = np.sqrt(r2) / dr
            inside = q < nbins
            counts[s, w] = np.bincount(q[inside].astype(np.int64), minlength=nbins)[:nbins]
            overflow[s, w] = int((~inside).sum())
            r = np.sqrt(r2)
            j = np.rint(r / dr).astype(np.int64)            # nearest edge
            near = np.abs(r - j * dr) < AMBIGUOUS
            for b in (j[near] - 1, j[near]):                # the bins on both sides of the edge
                b = b[(b >= 0) & (b < nbins)]
                np.add.at(amb[s, w], b, 1)
    return counts, overflow, moments, amb, kinds
