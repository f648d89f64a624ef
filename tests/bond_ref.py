"""Float64 numpy restatement of the bond survival counters (include/amof_hip.h, amof_bond_survival), written from the
definitions; it never calls the product.

h_ij(f) = 1 iff sqrt(d2) < rc for the minimum image of r_j(f) - r_i(f) in frame f's cell (periodic axes only), i != j.  The
minimum image is found by brute force: the nearest of the 27 images around the rounded fractional difference, which is the
canonical one for every pair closer than half the smallest cell height.  A pair within 1e-9 rc of the cutoff is re-decided in
the canonical arithmetic itself, emulated with exact rationals (amof_cn_count's decision to the last bit)."""

import itertools
from fractions import Fraction

import numpy as np


def species(numbers):
    kinds = sorted(set(int(z) for z in numbers))
    return kinds, np.array([kinds.index(int(z)) for z in numbers], dtype=np.int64)


def origins(F, m, stride=1):
    return list(range(1, F - m, stride))        # k = 1, 1 + s, ... <= F - m - 1


def min_image_dist(pos_i, pos_j, cell, pbc):
    """[len(i)][len(j)] minimum-image distances of one frame (brute force over the 27 neighbouring images)"""
    d0 = pos_j[None, :, :] - pos_i[:, None, :]
    s = d0 @ np.linalg.inv(cell)
    n = np.rint(s) * np.asarray(pbc, dtype=np.float64)
    base = d0 - n @ cell
    best = np.full(d0.shape[:2], np.inf)
    ranges = [(-1, 0, 1) if pbc[x] else (0,) for x in range(3)]
    for sh in itertools.product(*ranges):
        d = base + np.asarray(sh, dtype=np.float64) @ cell
        # (differs from the canonical operation order by an ulp or two: bonded() re-decides the pairs that close to rc)
        best = np.minimum(best, np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]))
    return best


def _fma(a, b, c):
    """fma(a, b, c) correctly rounded (exact rational arithmetic; float() of a Fraction rounds to nearest even)"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def canonical_dist(pi, pj, cell, pbc):
    """sqrt(d2) of one pair in the canonical arithmetic of DESIGN §2, operation for operation: d0 = r_j - r_i, n = rint of
    the fractional difference (periodic axes), d = fma(-n2, c2, fma(-n1, c1, fma(-n0, c0, d0))) per component,
    d2 = fma(dz, dz, fma(dy, dy, dx dx)), correctly rounded sqrt"""
    d0 = [float(pj[x]) - float(pi[x]) for x in range(3)]
    n = np.rint(np.asarray(d0) @ np.linalg.inv(cell)) * np.asarray(pbc, dtype=np.float64)
    d = [_fma(-n[2], cell[2][x], _fma(-n[1], cell[1][x], _fma(-n[0], cell[0][x], d0[x]))) for x in range(3)]
    return float(np.sqrt(_fma(d[2], d[2], _fma(d[1], d[1], d[0] * d[0]))))


def bonded(pos, cell, numbers, a_number, b_number, rc, pbc=(True, True, True), centres=None):
    """h as a boolean [F][N_A][N_B] array; (h, atoms of A, atoms of B).  centres: (begin, end) atom range of the centres"""
    pos = np.asarray(pos, dtype=np.float64)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    numbers = np.asarray(numbers)
    ia = np.nonzero(numbers == a_number)[0]
    ib = np.nonzero(numbers == b_number)[0]
    if centres is not None:
        ia = ia[(ia >= centres[0]) & (ia < centres[1])]
    F = pos.shape[0]
    h = np.zeros((F, len(ia), len(ib)), dtype=bool)
    for f in range(F):
        c = cells[0 if len(cells) == 1 else f]
        d = min_image_dist(pos[f, ia], pos[f, ib], c, pbc)
        # within 1e-9 rc of the cutoff the last bit of the distance decides: those pairs in the canonical arithmetic
        for x, y in np.argwhere(np.abs(d - rc) <= 1e-9 * rc):
            d[x, y] = canonical_dist(pos[f, ia[x]], pos[f, ib[y]], c, pbc)
        h[f] = (d < rc) & (ia[:, None] != ib[None, :])
    return h, ia, ib


def counters(h, windows, stride=1):
    """[W][3] from h [F][N_A][N_B] by direct loops over lags and origins"""
    F = h.shape[0]
    out = np.zeros((len(windows), 3), dtype=np.uint64)
    for w, m in enumerate(windows):
        for k in origins(F, int(m), stride):
            out[w, 0] += np.uint64(h[k].sum())
            out[w, 1] += np.uint64((h[k] & h[k + m]).sum())
            out[w, 2] += np.uint64(np.all(h[k:k + m + 1], axis=0).sum())
    return out


def survival(pos, cell, numbers, sets, windows, stride=1, pbc=(True, True, True), centres=None):
    """[n_sets][W][3]; sets: [(A number, B number, rc)]"""
    return np.stack([counters(bonded(pos, cell, numbers, a, b, rc, pbc, centres)[0], windows, stride) for a, b, rc in sets])
