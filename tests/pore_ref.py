"""Float64 numpy restatement of the pore field (include/amof_hip.h, amof_pore_field), written from the definition; it never
calls the product.

Grid points are amof_amd.pore.grid_points' rule restated here elementwise (``points``).  For a grid point p and an atom j,
d is the nearest of the 27 images around the rounded fractional difference of r_j - p (the canonical minimum image for
every pair closer than half the smallest cell height, tests/reorientation_ref.py ``vectors``), v_j = |d| - R_j, and the field
is min_j v_j where that is below dmax, else dmax.

The error budget (derived, not tuned against the GPU) bounds |library v_j - this v_j| when both evaluations are correct.
Both start from the same p (the grid rule is bit-exact) and the same d0 = fl(r_j - p), and subtract the same lattice vector
in different operation orders: as derived in tests/reorientation_ref.py the vectors differ by less than 13 eps M in norm,
    M = max_x |d0_x| + sum_k (|n_k| + 1) sum_x |C_kx|,      eps = 2^-52,
taken as K = 16.  The norm moves by at most that.  Its own arithmetic: three products and two sums under a root (library:
one product and two fma), relative to |d| under 4 eps on either side, and the subtraction of R half an eps of |v| <= |d| + R
on either side: 10 eps (|d| + R) in all.
    budget_j = K eps M + 10 eps (|d| + R_j)
The minimum over j moves by at most the largest budget_j, which is what a point gets.  The tests require it to stay below
1e-10 A (``worst``): a wrong image, a wrong radius or a missed atom moves a value by O(0.1) A."""

import collections
import itertools

import numpy as np

EPS = 2.0 ** -52
K = 16.0

Result = collections.namedtuple("Result", "field budget worst rows counts")
# field, budget [F][G] float64; worst: the largest budget; rows u64 [F][nbins + 2], counts int64 [F][n_t] by the documented rule


def points(cell, n):
    """``[G][3]`` grid points of one cell, element by element: f = (i + 0.5) / n per axis (IEEE division), p_c =
    (f_x C[0][c] + f_y C[1][c]) + f_z C[2][c]; linear index (i ny + j) nz + k"""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    nx, ny, nz = (int(x) for x in n)
    out = np.empty((nx * ny * nz, 3))
    for i in range(nx):
        fx = np.float64(i + 0.5) / np.float64(nx)
        for j in range(ny):
            fy = np.float64(j + 0.5) / np.float64(ny)
            for k in range(nz):
                fz = np.float64(k + 0.5) / np.float64(nz)
                for c in range(3):
                    out[(i * ny + j) * nz + k, c] = (fx * cell[0, c] + fy * cell[1, c]) + fz * cell[2, c]
    return out


def nbins_of(dr, dmax):
    return int(np.rint(dmax / dr))


def from_field(field, dr, dmax, thresholds):
    """``(rows u64 [F][nbins + 2], counts int64 [F][n_t], vmax [F], argmax [F])`` of a field ``[F][G]`` by the documented
    rule: [0] v < 0; [1 + b], b = (int)(v / dr) < nbins for 0 <= v < dmax; [nbins + 1] the rest; counts: v >= t; the largest
    value and the smallest index that has it"""
    field = np.asarray(field, dtype=np.float64)
    F = field.shape[0]
    field = field.reshape(F, -1)
    nbins = nbins_of(dr, dmax)
    rows = np.zeros((F, nbins + 2), dtype=np.uint64)
    counts = np.zeros((F, len(thresholds)), dtype=np.int64)
    for f in range(F):
        v = field[f]
        slot = np.full(v.shape, nbins + 1, dtype=np.int64)
        inside = v < 0.0
        mid = ~inside & (v < dmax)
        b = np.zeros(v.shape, dtype=np.int64)
        b[mid] = (v[mid] / np.float64(dr)).astype(np.int64)        # (truncation towards zero of a non-negative value)
        slot[mid & (b < nbins)] = 1 + b[mid & (b < nbins)]
        slot[inside] = 0
        rows[f] = np.bincount(slot, minlength=nbins + 2).astype(np.uint64)
        for t, thr in enumerate(thresholds):
            counts[f, t] = int((v >= np.float64(thr)).sum())
    vmax = field.max(axis=1) if field.shape[1] else np.zeros(F)
    argmax = field.argmax(axis=1).astype(np.int64) if field.shape[1] else np.zeros(F, dtype=np.int64)     # (first occurrence)
    return rows, counts, vmax, argmax


def frame_values(pos, cell, radius, p, pbc, chunk=2048):
    """(min_j v_j [G], budget [G]) of one frame: ``radius [N]`` per atom, ``p [G][3]``"""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    inv = np.linalg.inv(cell)
    per = np.asarray(pbc, dtype=np.float64)
    ranges = [(-1, 0, 1) if pbc[x] else (0,) for x in range(3)]
    csum = np.abs(cell).sum(axis=1)
    G = len(p)
    vmin = np.full(G, np.inf)
    bud = np.zeros(G)
    for g0 in range(0, G, chunk):
        q = p[g0:g0 + chunk]
        d0 = pos[None, :, :] - q[:, None, :]
        n = np.rint(d0 @ inv) * per
        base = d0 - n @ cell
        best = np.full(d0.shape[:2], np.inf)
        for sh in itertools.product(*ranges):
            d = base + np.asarray(sh, dtype=np.float64) @ cell
            r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
            best = np.minimum(best, r2)
        dist = np.sqrt(best)
        v = dist - radius[None, :]
        M = np.abs(d0).max(axis=-1) + (np.abs(n) + 1.0) @ csum
        b = K * EPS * M + 10.0 * EPS * (dist + radius[None, :])
        vmin[g0:g0 + chunk] = v.min(axis=1) if v.shape[1] else np.inf
        bud[g0:g0 + chunk] = b.max(axis=1) if b.shape[1] else 0.0
    return vmin, bud


def pore(pos, cell, numbers, radii, grid, dr, dmax, thresholds, pbc=(True, True, True)):
    """``(Result, raw minimum [F][G])`` of a trajectory: ``radii``: {atomic number: Angstrom}"""
    pos = np.asarray(pos, dtype=np.float64)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    radius = np.array([radii[int(z)] for z in numbers], dtype=np.float64)
    F = pos.shape[0]
    G = int(grid[0]) * int(grid[1]) * int(grid[2])
    raw, budget = np.zeros((F, G)), np.zeros((F, G))
    pts = None
    for f in range(F):
        c = cells[0 if len(cells) == 1 else f]
        if pts is None or len(cells) > 1:
            pts = points(c, grid)
        raw[f], budget[f] = frame_values(pos[f], c, radius, pts, pbc)
    # (``raw``: the minimum itself, also where it is not below dmax -- ``near_decisions`` needs its distance to dmax)
    capped = np.where(raw < dmax, raw, dmax)
    rows, counts, _, _ = from_field(capped, dr, dmax, thresholds)
    return Result(capped, budget, float(budget.max()) if budget.size else 0.0, rows, counts), raw


def near_decisions(raw, budget, dr, dmax, thresholds, slack=1.0):
    """``[(frame, point, what)]``: the points whose value (``raw``: the minimum itself, also where it is not below dmax) lies
    within ``slack`` x the budget of a decision -- 0, a bin edge, dmax, a threshold"""
    out = []
    nbins = nbins_of(dr, dmax)
    tol = slack * budget + 4.0 * EPS * np.abs(raw)
    hit = np.abs(raw) <= tol
    out += [(int(f), int(g), "zero") for f, g in np.argwhere(hit)]
    q = raw / dr
    k = np.rint(q)
    hit = (np.abs(q - k) * dr <= tol) & (k >= 1) & (k <= nbins) & (raw < dmax + tol)
    out += [(int(f), int(g), "edge") for f, g in np.argwhere(hit)]
    hit = np.abs(raw - dmax) <= tol
    out += [(int(f), int(g), "dmax") for f, g in np.argwhere(hit)]
    for t in thresholds:
        hit = np.abs(raw - t) <= tol
        out += [(int(f), int(g), "threshold") for f, g in np.argwhere(hit)]
    return out


def check_field(got, want):
    """the library's field ``[F][...]`` against a ``Result``: within the budget everywhere; returns the largest
    |difference| / budget"""
    got = np.asarray(got, dtype=np.float64).reshape(want.field.shape)
    diff = np.abs(got - want.field)
    assert np.all(diff <= want.budget), (float(diff.max()), np.argwhere(diff > want.budget)[:4].tolist())
    return float((diff / want.budget).max()) if diff.size else 0.0
