"""float64 numpy restatement of amof_sq_accumulate / amof_sq_modes (include/amof_hip.h).  Fractional coordinates are
solve(cell.T, pos.T) in float64, not the library's u32 values (the difference is far below the tests' tolerance).  Test
infrastructure only (the package never imports it)."""

import numpy as np

from tests import helpers as H


def reciprocal(cell):
    return 2.0 * np.pi * np.linalg.inv(np.asarray(cell, dtype=np.float64)).T


def bins(recip, hkl, dq, nbins):
    """bin of every vector (nbins where b >= nbins), the issue's operation order: no fma, sqrt correctly rounded"""
    R = np.asarray(recip, dtype=np.float64)
    h, k, l = (np.asarray(hkl, dtype=np.float64)[:, c] for c in range(3))
    qx = (h * R[0, 0] + k * R[1, 0]) + l * R[2, 0]
    qy = (h * R[0, 1] + k * R[1, 1]) + l * R[2, 1]
    qz = (h * R[0, 2] + k * R[1, 2]) + l * R[2, 2]
    qq = np.sqrt((qx * qx + qy * qy) + qz * qz) / dq
    return np.where(qq < nbins, np.floor(np.minimum(qq, nbins)), nbins).astype(np.int64)


def modes(pos, cell, species, S, hkl, chunk=4096):
    """rho [K][S] complex: sum over the atoms of species a of exp(2 pi i hkl . s)"""
    s = np.linalg.solve(np.asarray(cell, dtype=np.float64).T, np.asarray(pos, dtype=np.float64).T).T      # [N][3]
    hkl = np.asarray(hkl, dtype=np.float64).reshape(-1, 3)
    rho = np.zeros((len(hkl), S), dtype=np.complex128)
    for c0 in range(0, len(hkl), chunk):
        ph = 2.0 * np.pi * (hkl[c0:c0 + chunk] @ s.T)       # [k][N]
        e = np.exp(1j * ph)
        for a in range(S):
            rho[c0:c0 + chunk, a] = e[:, species == a].sum(axis=1)
    return rho


def sq(packed, hkl, dq, nbins, frames=None):
    """(counts [nbins], sums [P][nbins], beyond, kinds) over the frames (default: all)"""
    kinds, species = H.species_of(packed.numbers)
    S = len(kinds)
    pos = np.asarray(packed.pos_host(), dtype=np.float64)
    F = len(pos)
    frames = range(F) if frames is None else frames
    cell = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3)
    counts = np.zeros(nbins, dtype=np.int64)
    sums = np.zeros((S * (S + 1) // 2, nbins))
    beyond = 0
    for f in frames:
        c = cell[f if len(cell) > 1 else 0]
        b = bins(reciprocal(c), hkl, dq, nbins)
        rho = modes(pos[f], c, species, S, hkl)
        ok = b < nbins
        beyond += int((~ok).sum())
        counts += np.bincount(b[ok], minlength=nbins)
        p = 0
        for a in range(S):
            for d in range(a, S):
                t = rho[:, a].real * rho[:, d].real + rho[:, a].imag * rho[:, d].imag
                sums[p] += np.bincount(b[ok], weights=t[ok], minlength=nbins)
                p += 1
    return counts, sums, beyond, kinds


def normalised(counts, sums, kinds, numbers):
    """S columns to compare: X-X and every unordered pair's sums_ab / (counts sqrt(N_a N_b)) (NaN where counts == 0)"""
    numbers = np.asarray(numbers)
    n = np.array([(numbers == z).sum() for z in kinds], dtype=np.float64)
    c = np.where(counts > 0, counts, np.nan).astype(np.float64)
    out, p, tot = [], 0, 0.0
    for a in range(len(kinds)):
        for d in range(a, len(kinds)):
            out.append(sums[p] / (c * np.sqrt(n[a] * n[d])))
            tot = tot + (1.0 if a == d else 2.0) * sums[p]
            p += 1
    return np.vstack([tot / (c * n.sum())] + out)
