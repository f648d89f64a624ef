"""Dihedral angles of the chains of four bonded atoms, restated in numpy independently of the library
(amof_amd/csrc/dihedral_math.h, include/amof_hip.h: amof_dihedral_hist).

Bonds: tests/ring_ref.adjacency (float64 minimum image; it asserts that no pair lies within 1e-6 A of its cutoff).  Chains: an
unordered central bond {b, c}, a neighbour a of b, a neighbour d of c, a != c, d != b, a != d by atom index, each visited once.
Angle: with the minimum-image vectors b1 = r_b - r_a, b2 = r_c - r_b, b3 = r_d - r_c,

    phi = |atan2(|b2| b1 . (b2 x b3), (b1 x b2) . (b2 x b3))|  in degrees

-- deliberately NOT the kernels' acos of normalised cross products.  A chain is undefined iff the squared sine of one of its
two bond angles, s = |x|^2 / (|p|^2 |q|^2), is below 2^-40.  ``frame`` asserts that no s lies within a factor 4 of 2^-40 and
that no defined angle lies within 1e-7 degrees of a bin edge: whatever float64 arithmetic forms the angle then bins it the
same, so histograms and counts must be EQUAL integers.  (The edge 0 where it is the first one is left out of that assert:
phi >= 0 by construction on both sides, and the first bin is closed on the left -- the exact cis chains of a lattice sit there.)
Cosine sums: the library adds llrint(c 2^40) per chain, c within 2^-43 of cos(phi); ``check_cos`` allows one unit per chain.
"""

import numpy as np

from tests import ring_ref

E = 40
UNDEFINED_BELOW = 2.0 ** -40


class Frame(object):
    """hist [T][nb], n [T], undefined [T] (int64), cos [T] (float: sum of cos(phi) over the defined chains), and what the
    asserts looked at: chains (geometric), triangles (a == d met), edge_gap (smallest distance of a defined angle to an
    interior edge, degrees)"""


def _fits(pattern, s):
    return all(w < 0 or w == x for w, x in zip(pattern, s))


def chains_of(adj):
    """``[(a, b, c, d)]`` of a frame's neighbour lists, and the number of (a, b, c, d = a) met"""
    out, triangles = [], 0
    for b, row in enumerate(adj):
        for c in row:
            if c <= b:
                continue
            for a in row:
                if a == c:
                    continue
                for d in adj[c]:
                    if d == b:
                        continue
                    if d == a:
                        triangles += 1
                        continue
                    out.append((a, b, c, d))
    return out, triangles


def frame(pos, cell, numbers, cutoff, chains, edges, pbc=(True, True, True), adj=None):
    """one frame; ``chains``: [T][4] atomic numbers, -1 = any; ``cutoff``: the dictionary (applied symmetrically)"""
    pos = np.asarray(pos, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    numbers = np.asarray(numbers)
    edges = np.asarray(edges, dtype=np.float64)
    T, nb = len(chains), len(edges) - 1
    if adj is None:
        adj = ring_ref.adjacency(pos, cell, numbers, cutoff, pbc)
    quads, triangles = chains_of(adj)
    r = Frame()
    r.hist = np.zeros((T, nb), dtype=np.int64)
    r.n = np.zeros(T, dtype=np.int64)
    r.undefined = np.zeros(T, dtype=np.int64)
    r.cos = np.zeros(T, dtype=np.float64)
    r.chains, r.triangles, r.edge_gap = len(quads), triangles, np.inf
    r.adj = adj
    if not quads:
        return r
    q = np.array(quads)
    inv = np.linalg.inv(cell)
    mask = np.asarray(pbc, dtype=np.float64)

    def mic(i, j):
        s = (pos[j] - pos[i]) @ inv
        s -= np.rint(s) * mask
        return s @ cell

    b1, b2, b3 = mic(q[:, 0], q[:, 1]), mic(q[:, 1], q[:, 2]), mic(q[:, 2], q[:, 3])
    x1, x2 = np.cross(b1, b2), np.cross(b2, b3)
    l1, l2, l3 = (b1 ** 2).sum(1), (b2 ** 2).sum(1), (b3 ** 2).sum(1)
    s1, s2 = (x1 ** 2).sum(1) / (l1 * l2), (x2 ** 2).sum(1) / (l2 * l3)
    for s in (s1, s2):
        assert not ((s > UNDEFINED_BELOW / 4) & (s < UNDEFINED_BELOW * 4)).any(), "a bond angle within a factor 4 of the undefined threshold"
    defined = (s1 >= UNDEFINED_BELOW) & (s2 >= UNDEFINED_BELOW)
    phi = np.abs(np.degrees(np.arctan2(np.sqrt(l2) * (b1 * x2).sum(1), (x1 * x2).sum(1))))
    interior = edges[1:] if edges[0] == 0.0 else edges
    if defined.any():
        r.edge_gap = float(np.abs(phi[defined][:, None] - interior[None, :]).min())
        assert r.edge_gap > 1e-7, "a defined angle within 1e-7 degrees of a bin edge"
        assert phi[defined].min() >= edges[0] and phi[defined].max() < edges[-1]
    k = np.searchsorted(edges, phi, side="right") - 1
    sp = numbers[q]
    for t, pattern in enumerate(chains):
        hit = np.array([_fits(pattern, s) or _fits(pattern, s[::-1]) for s in sp.tolist()], dtype=bool)
        ok = hit & defined
        r.hist[t] = np.bincount(k[ok], minlength=nb)[:nb]
        r.n[t] = ok.sum()
        r.undefined[t] = (hit & ~defined).sum()
        r.cos[t] = np.cos(np.radians(phi[ok])).sum()
    return r


def trajectory(packed, cutoff, chains, edges):
    """``[Frame]`` of every frame of a PackedTrajectory"""
    pos = packed.pos_host()
    return [frame(pos[f], packed.cell[0 if packed.cell.shape[0] == 1 else f], packed.numbers, cutoff, chains, edges, tuple(packed.pbc))
            for f in range(pos.shape[0])]


def totals(frames):
    """``(hist [T][nb], n [T], undefined [T], frame_sums [F][T][2], cos [F][T])`` of a list of frames"""
    hist = sum(fr.hist for fr in frames)
    n = sum(fr.n for fr in frames)
    undefined = sum(fr.undefined for fr in frames)
    sums = np.stack([np.stack([fr.n, fr.undefined], axis=1) for fr in frames])
    cos = np.stack([fr.cos for fr in frames])
    return hist, n, undefined, sums, cos


def check(got, frames):
    """the library's ``(hist, n_dihedrals, n_undefined, frame_sums)`` against the restatement: equal integers, the cosine sums
    within one unit of 2^-40 per chain"""
    hist, n, undefined, sums, cos = totals(frames)
    g_hist, g_n, g_undef, g_sums = (np.asarray(x).astype(np.int64) for x in got)
    assert np.array_equal(g_hist, hist), "histograms differ"
    assert np.array_equal(g_n, n) and np.array_equal(g_undef, undefined), "counts differ"
    assert np.array_equal(g_sums[:, :, :2], sums), "per-frame counts differ"
    check_cos(g_sums[:, :, 2], cos, sums[:, :, 0])


def check_cos(got, cos, n):
    diff = np.abs(np.asarray(got, dtype=np.float64) - np.asarray(cos) * 2.0 ** E)
    assert np.all(diff <= np.asarray(n)), "cosine sums off by %g units, chains %s" % (diff.max(), np.asarray(n).max())
