"""Float64 numpy restatement of the surface stage (include/amof_hip.h, amof_pore_surface), written from the definition; it never
calls the product.

Samples are the documented rule elementwise: rho_j = R_j + rp, s = r_j + rho_j u_m -- a product, then a sum, which numpy forms
with the library's own bits.  For a sample and an atom k != j, d is the nearest of the 27 images around the rounded fractional
difference of r_k - s (the canonical minimum image for every pair closer than half the smallest cell height,
tests/pore_ref.py), v_k = |d| - R_k, and the sample is exposed iff v_k >= rp for every k.  Only atoms whose own minimum-image
distance to atom j is below rho_j + R_k + rp + 1 A are looked at: by the triangle inequality every other atom has
v_k - rp > 1 A, neither a burial nor a near decision.

The error budget (derived, not tuned against the GPU) bounds |library v_k - this v_k| when both evaluations are correct: the
budget of tests/pore_ref.py for sqrt(d2) - R from one point,
    K eps M + 10 eps (|d| + R_k),     M = max_x |d0_x| + sum_k (|n_k| + 1) sum_x |C_kx|,  K = 16,  eps = 2^-52,
plus the sample's own two roundings, 2 eps (max_x |r_jx| + rho_j) -- both sides form the same bits there, the term is kept so
that the budget does not rest on that.  The tests require it to stay below 1e-10 A.

The corner rule is restated with numpy's inverse cell: f = s C^-1 wrapped into [0, 1) on periodic axes, t_k = f_k n_k - 0.5,
i_k = floor(t_k), corners i_k + {0, 1}.  The library's inverse is another evaluation: a sample with |t_k - rint(t_k)| < 1e-9
on some axis is a near decision (``near_decisions``)."""

import collections
import itertools

import numpy as np

EPS = 2.0 ** -52
K = 16.0
T_GUARD = 1e-9

Frame = collections.namedtuple("Frame", "exposed near worst samples")
# exposed, near bool [N][M]; worst: the largest budget; samples float64 [N][M][3]


def _min_image_d2(d0, cell, inv, per, shifts):
    n = np.rint(d0 @ inv) * per
    base = d0 - n @ cell
    best = np.full(d0.shape[:-1], np.inf)
    for sh in shifts:
        d = base + sh
        best = np.minimum(best, d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    return best, n


def frame(pos, cell, radius, rp, dirs, pbc):
    """one frame, one probe radius: ``radius [N]`` per atom, ``dirs [M][3]``"""
    pos = np.asarray(pos, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    radius = np.asarray(radius, dtype=np.float64)
    dirs = np.asarray(dirs, dtype=np.float64)
    rp = np.float64(rp)
    inv = np.linalg.inv(cell)
    per = np.asarray(pbc, dtype=np.float64)
    shifts = [np.asarray(sh, dtype=np.float64) @ cell for sh in itertools.product(*[(-1, 0, 1) if pbc[x] else (0,) for x in range(3)])]
    csum = np.abs(cell).sum(axis=1)
    N, M = len(pos), len(dirs)
    rho = radius + rp
    samples = pos[:, None, :] + rho[:, None, None] * dirs[None, :, :]
    atom_d2, _ = _min_image_d2(pos[None, :, :] - pos[:, None, :], cell, inv, per, shifts)
    atom_d = np.sqrt(atom_d2)
    exposed = np.ones((N, M), dtype=bool)
    near = np.zeros((N, M), dtype=bool)
    worst = 0.0
    for j in range(N):
        nb = np.nonzero((atom_d[j] < rho[j] + rho + 1.0) & (np.arange(N) != j))[0]
        if not len(nb):
            continue
        d0 = pos[nb][None, :, :] - samples[j][:, None, :]
        best, n = _min_image_d2(d0, cell, inv, per, shifts)
        dist = np.sqrt(best)
        v = dist - radius[nb][None, :]
        big = np.abs(d0).max(axis=-1) + (np.abs(n) + 1.0) @ csum
        b = K * EPS * big + 10.0 * EPS * (dist + radius[nb][None, :]) + 2.0 * EPS * (np.abs(pos[j]).max() + rho[j])
        exposed[j] = (v >= rp).all(axis=1)
        near[j] = (np.abs(v - rp) <= b + 4.0 * EPS * np.abs(v)).any(axis=1)
        worst = max(worst, float(b.max()))
    return Frame(exposed, near, worst, samples)


def corners(samples, cell, grid, pbc):
    """``(index int64 [..][8], near bool [..])``: the linear grid indices ``(i ny + j) nz + k`` of the 8 corners of every sample
    ``[..][3]`` (-1: dropped, outside the grid on an open axis) and whether some t_k lies within 1e-9 of an integer"""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    n = np.asarray(grid, dtype=np.int64)
    f = np.asarray(samples, dtype=np.float64) @ np.linalg.inv(cell)
    for k in range(3):
        if pbc[k]:
            f[..., k] = f[..., k] - np.floor(f[..., k])
    t = f * n.astype(np.float64) - 0.5
    near = (np.abs(t - np.rint(t)) < T_GUARD).any(axis=-1)
    i = np.floor(t).astype(np.int64)
    out = np.empty(f.shape[:-1] + (8,), dtype=np.int64)
    for c in range(8):
        x = i + np.array([(c >> 2) & 1, (c >> 1) & 1, c & 1])
        ok = np.ones(f.shape[:-1], dtype=bool)
        for k in range(3):
            if pbc[k]:
                x[..., k] = x[..., k] % n[k]
            ok &= (x[..., k] >= 0) & (x[..., k] < n[k])
        lin = (x[..., 0] * n[1] + x[..., 1]) * n[2] + x[..., 2]
        out[..., c] = np.where(ok, lin, -1)
    return out, near


def accessible(exposed, samples, cell, grid, pbc, channel_mask):
    """bool [N][M]: exposed and at least one corner in ``channel_mask`` (bool [nx][ny][nz]: the points of the channels of V(rp))"""
    idx, _ = corners(samples, cell, grid, pbc)
    flat = np.asarray(channel_mask, dtype=bool).reshape(-1)
    hit = (flat[np.maximum(idx, 0)] & (idx >= 0)).any(axis=-1)
    return exposed & hit


def near_decisions(fr, cell, grid, pbc):
    """``[(atom, sample, what)]`` of a ``Frame``: the samples within the budget of v_k = rp for some k ("sphere"), and the exposed
    ones with a corner coordinate within 1e-9 of a grid plane ("corner")"""
    out = [(int(j), int(m), "sphere") for j, m in np.argwhere(fr.near)]
    _, near_t = corners(fr.samples, cell, grid, pbc)
    out += [(int(j), int(m), "corner") for j, m in np.argwhere(near_t & fr.exposed)]
    return out


def by_species(flags, species, S):
    """``int64 [S]``: the samples flagged in ``flags [N][M]`` per species of their atom"""
    per_atom = np.asarray(flags).sum(axis=1).astype(np.int64)
    return np.bincount(np.asarray(species), weights=per_atom, minlength=S).astype(np.int64)
