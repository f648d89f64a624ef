"""Test infrastructure (the package never imports it): one cell for every reachable variant of the general-cell tile
kernel ("rdf_tile_tri", amof_amd/csrc/tri_select.h), and trajectories whose pairs sit on the image decisions those
variants make.

The kernel works in the stored frame: axis order (ax0, ax1, axis) = (x, y, z), the lower factor L of the metric of the
rows in that order, and folded fractional coordinates x' = s_x + kx s_z, y' = s_y + ky s_z (kx = L20 / L00 - c10 L21 / L11,
ky = L21 / L11, c10 = L10 / L00), so that a pair vector is X = L00 (fx + c10 fy), Y = L11 fy, Z = L22 fz with
fz = wrap(ds_z), fy = wrap(ds_y + ky fz), fx = wrap(ds_x + kx fz).  Its decisions per pair, and what is planted on them:

  a  |fy| against the y near threshold rec[4] / 2^32 ~ 1/2 - tau_y  (second image along y: in range / the first / neither)
  b  |fz| against the z near threshold rec[5] dr / L22              (codes 3, 8)
  c  fx + c10 fy against +-1/2: the x wrap with the y term (XW codes: 5 .. 11), and fx against +-1/2, the wrap the other
     codes decide (counted apart as "cx").  Where half the x axis lies beyond the cutoff -- every code without the y
     term by the selection's own condition R / L00 + |c10| / 2 < 1/2, and code-5 cells such as c5_on (L00 / 2 = 8.13,
     rmax 7.894) -- both images of such a pair are out of range: there the category checks that neither is counted
     (a wrongly wrapped x can bring a candidate into range), not which of the two is the nearer
  d  which of the two twin candidates v, v -+ (B - k A) is nearer   (codes 4, 9, 10, 11): ties, across the cutoff, a bin apart
  e  |s| = 1/2 along the shortest axis at distance L / 2 (1 +- delta) where rmax = L / 2 (both images at the cutoff)

Offsets from a decision: exactly on it, a few grid units of 2^-32 (and the f32 granularity of the compare, 64 .. 256
units), log-uniform out to 1e-3 of the cell.  Every category also puts a distance of the pair at (k + delta) dr or at the
cutoff (edge_plant.offsets with the band of rdf_band), so that the image decision and the bin decision fall on the same
pair.  `realised` recomputes where every planted pair landed, in float64 from the positions alone; the floors on it are
asserted by tests/test_tri_select_cpu.py."""

import numpy as np

from amof_amd.frames import PackedTrajectory
from tests import cell_forms
from tests import edge_plant as E

TWO32 = 4294967296.0
S3 = float(np.sqrt(3.0) / 2.0)
WINDOW = 1e-3                   # of the cell: how far from a decision a planted pair may land


def _hex(a, c, sign, tilt=(0.0, 0.0)):
    return [[a, 0.0, 0.0], [sign * 0.5 * a, S3 * a, 0.0], [tilt[0], tilt[1], c]]


def _breathe(cell, scales):
    return [(np.asarray(cell, dtype=np.float64) * s).tolist() for s in scales]


# name -> cell rows (or a list of per-frame cells), rmax (None: the reference's default, half the shortest cell length in
# float64), AMOF_RDF_NOHALF, and what the selection takes: (code, ax0, ax1, axis, cull).  tests/test_tri_select_cpu.py
# pins the table to tri_select.h on the CPU; tests/test_gpu_tri_codes.py reads the code back from the library.
# Reachable (code, cull): 0 1 2 4 5 6 7 9 10 11 with and without culling, 3 and 8 without.  Near tests along z (3, 8)
# need a second image along the slab axis in range, rmax > h / 2, which contradicts culling's 2 * 1.05 * rmax < h.
# Code 4 needs a long x axis, L00 > 2 R + |L10|, and a twin along y; unculled it takes a strongly tilted third vector
# (large folds kx, ky), which keeps every perpendicular height below 2.1 rmax although L00 is long (c4_off).
# AMOF_RDF_NOCULL=1 runs the unculled instantiation of every code.
CASES = {
    "c0_off": dict(cell=[[18.95, 0, 0], [0.77, 15.66, 0], [-9.33, 1.97, 13.92]], rmax=7.606, expect=(0, 2, 1, 0, 0)),
    "c0_on": dict(cell=[[17.31, 0, 0], [2.93, 18.11, 0], [-1.71, 3.37, 29.53]], rmax=6.5, expect=(0, 0, 1, 2, 1)),
    "c1_off": dict(cell=[[16.01, 0, 0], [0.06, 16.11, 0], [0.0, 0.2, 15.87]], rmax=None, expect=(1, 0, 2, 1, 0)),
    "c1_on": dict(cell=[[13.01, 0, 0], [0.0, 13.02, 0], [-0.34, -0.24, 25.59]], rmax=None, expect=(1, 1, 0, 2, 1)),
    "c2_off": dict(cell=[[18.11, 0, 0], [0.32, 18.02, 0], [-0.14, -0.15, 17.46]], rmax=8.733, expect=(2, 1, 2, 0, 0)),
    "c2_on": dict(cell=[[16.9, 0, 0], [-1.48, 19.34, 0], [0.48, 1.36, 36.99]], rmax=8.452, expect=(2, 1, 0, 2, 1)),
    "c3_off": dict(cell=[[19.92, 0, 0], [3.53, 18.58, 0], [-5.41, 1.72, 18.74]], rmax=9.458, expect=(3, 2, 1, 0, 0)),
    "c4_on": dict(cell=[[35.17, 0, 0], [15.01, 5.45, 0], [1.43, -1.49, 12.97]], rmax=2.994, expect=(4, 0, 1, 2, 1)),
    "c4_off": dict(cell=[[43.3, 0, 0], [18.73, 9.01, 0], [-24.34, 7.93, 10.33]], rmax=5.0, expect=(4, 0, 1, 2, 0)),
    "c5_off": dict(cell=[[20.76, 0, 0], [-6.74, 17.07, 0], [8.94, 2.48, 17.56]], rmax=8.397, expect=(5, 0, 1, 2, 0)),
    "c5_on": dict(cell=[[18.44, 0, 0], [-1.43, 19.71, 0], [1.65, -9.37, 13.2]], rmax=7.894, expect=(5, 2, 1, 0, 1)),
    "c6_off": dict(cell=[[16.87, 0, 0], [0.99, 17.52, 0], [3.34, -3.68, 16.58]], rmax=None, expect=(6, 0, 2, 1, 0)),
    "c6_on": dict(cell=[[12.22, 0, 0], [3.52, 18.03, 0], [-2.41, -0.84, 33.61]], rmax=None, expect=(6, 0, 1, 2, 1)),
    "c7_off": dict(cell=[[17.44, 0, 0], [-1.05, 18.17, 0], [3.17, 3.94, 16.84]], rmax=8.694, expect=(7, 2, 0, 1, 0)),
    "c7_on": dict(cell=[[14.69, 0, 0], [4.19, 13.5, 0], [0.67, -3.08, 30.88]], rmax=7.066, expect=(7, 1, 0, 2, 1)),
    "c8_off": dict(cell=[[17.87, 0, 0], [8.38, 16.38, 0], [5.08, 3.47, 14.96]], rmax=8.085, expect=(8, 2, 0, 1, 0)),
    "c9_off": dict(cell=[[15.93, 0, 0], [-7.76, 14.02, 0], [0.37, -0.34, 16.03]], rmax=None, expect=(9, 0, 1, 2, 0)),
    "c9_on": dict(cell=[[17.77, 0, 0], [8.77, 15.89, 0], [-0.48, 0.68, 32.09]], rmax=None, expect=(9, 0, 1, 2, 1)),
    "c10_off": dict(cell=_hex(14.25, 14.886996194131935, 1, (-0.23974594844214175, -0.16369530866885773)), rmax=None,
                    expect=(10, 0, 1, 2, 0)),
    "c10_on": dict(cell=[[1.4 * 17.0, 0, 0], [0, 17.0, 0], [0, 0.5 * 17.0, S3 * 17.0]], rmax=None, expect=(10, 1, 2, 0, 1)),
    "c11_off": dict(cell=_hex(15.37, 15.598930288200437, -1), rmax=None, expect=(11, 0, 1, 2, 0)),
    "c11_on": dict(cell=_hex(17.0, 31.0, -1), rmax=None, expect=(11, 0, 1, 2, 1)),
    # the exact-half cells through the float-product form (AMOF_RDF_NOHALF=1)
    "c9_nohalf": dict(cell=_hex(17.0, 31.0, -1), rmax=None, nohalf=True, expect=(9, 0, 1, 2, 1)),
    "c4_nohalf": dict(cell=[[32.08, 0, 0], [16.04, 6.77, 0], [-0.97, 1.25, 13.54]], rmax=3.893, nohalf=True, expect=(4, 0, 1, 2, 1)),
    # per-frame (NPT) cells that breathe across the y threshold: tau_y <= 0 in one frame (threshold INFINITY), > 0 in another
    "npt2_on": dict(cell=_breathe([[16.9, 0, 0], [-1.48, 19.34, 0], [0.48, 1.36, 36.99]], (1.004, 0.996)), rmax=8.452,
                    expect=(2, 1, 0, 2, 1)),
    "npt7_on": dict(cell=_breathe([[14.69, 0, 0], [4.19, 13.5, 0], [0.67, -3.08, 30.88]], (1.0, 1.012)), rmax=7.066,
                    expect=(7, 1, 0, 2, 1)),
    "npt3_off": dict(cell=_breathe([[19.92, 0, 0], [3.53, 18.58, 0], [-5.41, 1.72, 18.74]], (1.0, 1.003)), rmax=9.458,
                     expect=(3, 2, 1, 0, 0)),
}
NBINS = (7, 999, 2310)
NBINS_BIG = {"c2_on": 31744, "c9_on": 31744}          # two cases at the LDS limit of the tile kernels
DEVICE_INPUT = ("c3_off", "c7_on", "c11_on")
# the cases that also run in a form of tests/cell_forms.py (tests/test_gpu_cell_forms.py): every case rotated, the per-frame
# cases rotated and mirrored, and the exact-half cells with the second row negated (the sign of c10, on which codes 10 and
# 11 key, changes); (name, form, nbins)
NPT_CASES = ("npt2_on", "npt7_on", "npt3_off")
HALF_CASES = ("c10_off", "c10_on", "c11_off", "c11_on", "c9_nohalf")


def form_params():
    return ([(n, "rot", 999) for n in CASES] + [("c2_on", "rot", 2310), ("c9_on", "rot", 2310)] +
            [(n, "rotmirror", 999) for n in NPT_CASES] + [(n, "negrow", 999) for n in HALF_CASES])


def case_cells(name, form=None):
    """the cells of a case, [F][3][3]; form: one of tests/cell_forms.py (None: as tabulated)"""
    c = np.asarray(CASES[name]["cell"], dtype=np.float64)
    return cell_forms.apply(c.reshape(-1, 3, 3), form)


def case_rmax(name, form=None):
    r = CASES[name]["rmax"]
    if r is None:       # the reference's default: half the shortest cell length, float64 (of the cell as stored)
        r = float(min(np.linalg.norm(c, axis=1).min() for c in case_cells(name, form)) / 2)
    return float(r)


def case_expect(name, form=None):
    """what the selection takes for a case in a form: (code, ax0, ax1, axis, cull).  A rigid motion or a mirror changes
    nothing; `perm` renames the rows; negating the second row flips the sign of c10 = L10 / L00 wherever exactly one of
    (ax0, ax1) is that row, on which the exact-half codes key: 10 and 11 change places (no other code reads the sign).
    tests/test_cell_forms_cpu.py pins this to tri_select.h."""
    code, cull = CASES[name]["expect"][0], CASES[name]["expect"][4]
    order = case_order(name, form)
    if form == "negrow" and code in (10, 11) and (order[0] == 1) != (order[1] == 1):
        code = 21 - code
    return (code,) + order + (cull,)


def case_order(name, form=None):
    """the stored axes (ax0, ax1, axis) of a case; they name rows, so they follow the rows of `perm`"""
    order = CASES[name]["expect"][1:4]
    if form == "perm":      # new row k is old row (1, 2, 0)[k]
        order = tuple((2, 0, 1)[o] for o in order)
    return tuple(order)


class Stored(object):
    """tri_select.h restated for one cell in a given stored order: L, c10, the folds, tau and the thresholds the kernel
    compares with (rounded down to f32 as the host does), as fractions of the cell"""

    def __init__(self, C, order, rmax, nbins, guard_f):
        self.order = tuple(order)
        rows = C[list(order)]
        self.L = L = np.linalg.cholesky(rows @ rows.T)
        self.dr = dr = rmax / nbins
        self.R = R = rmax * (1.0 + 4.0 * guard_f / nbins + 1e-6)
        R0 = rmax * (1.0 + 1e-12)
        self.c10 = L[1, 0] / L[0, 0]
        self.ky = L[2, 1] / L[1, 1]
        self.kx = L[2, 0] / L[0, 0] - self.c10 * self.ky
        self.tau_y_raw = R / L[1, 1] - 0.5 + 1e-9
        self.tau_z_raw = R / L[2, 2] - 0.5 + 1e-9
        self.tau_y = -1.0 if 0.5 * L[1, 1] >= R0 else self.tau_y_raw
        self.tau_z = -1.0 if 0.5 * L[2, 2] >= R0 else self.tau_z_raw
        tau_x = -1.0 if 0.5 * L[0, 0] >= R0 else R / L[0, 0] - 0.5 + 1e-9

        def down(v):
            if not np.isfinite(v):
                return np.inf
            f = np.float32(v)
            if float(f) > v:
                f = np.nextafter(f, np.float32(-np.inf))
            return float(f)
        self.rec4 = (0.5 - self.tau_y) * TWO32 * (1.0 - 1e-6) - 8.0 if self.tau_y > 0 else np.inf
        self.rec5 = (L[2, 2] - R) / dr * (1.0 - 1e-6) - 0.02 if self.tau_z > 0 else np.inf
        self.rec8 = (0.5 - tau_x) * TWO32 * (1.0 - 1e-6) - 1024.0 if tau_x > 0 else np.inf
        self.thr_y = down(self.rec4) / TWO32
        self.thr_z = down(self.rec5) * dr / L[2, 2]
        xr = L[1, 0] - L[0, 0] * np.rint(L[1, 0] / L[0, 0])
        self.V = np.array([xr, L[1, 1], 0.0])           # the twin candidates differ by +-V = +-(B - k A)
        self.Linv = np.linalg.inv(L)

    def rec(self):
        """the record of tri_select.h: L00 L10 L11 L22 (bins per 2^-32), thr_y, thr_z, kx, ky, thr_x"""
        L, s = self.L, 1.0 / TWO32 / self.dr
        return np.array([L[0, 0] * s, L[1, 0] * s, L[1, 1] * s, L[2, 2] * s, self.rec4, self.rec5, self.kx, self.ky, self.rec8])

    def to_cart(self, v, C):
        """pair vectors in the orthogonalised frame -> Cartesian"""
        sp = v @ self.Linv                            # stored fractional
        s = np.zeros_like(sp)
        s[:, list(self.order)] = sp
        return s @ C

    def folded(self, d0, C):
        """(fx, fy, fz) of Cartesian pair vectors, as the kernel forms them (float64, no grid)"""
        s = (d0 @ np.linalg.inv(C))[:, list(self.order)]
        fz = s[:, 2] - np.rint(s[:, 2])
        fy = s[:, 1] + self.ky * fz
        fy = fy - np.rint(fy)
        fx = s[:, 0] + self.kx * fz
        fx = fx - np.rint(fx)
        return fx, fy, fz


def stored_frames(name, nbins, form=None):
    cells = case_cells(name, form)
    rmax = case_rmax(name, form)
    g = E.rdf_band(cells, rmax, nbins)
    order = case_order(name, form)
    return [Stored(c, order, rmax, nbins, g) for c in cells], g


def numbers(n=2400, kinds=(1, 6, 7, 30, 8), weights=(0.35, 0.3, 0.25, 0.1, 0.0)):
    """five species, one of a single atom (weight 0)"""
    w = np.asarray(weights, dtype=float)
    counts = np.floor(w / w.sum() * (n - (w == 0).sum())).astype(int)
    counts[np.argmax(w)] += n - (w == 0).sum() - counts.sum()
    counts[w == 0] = 1
    return np.repeat(kinds, counts)


def dec_offsets(rng, n):
    """n signed offsets from an image decision, as fractions of the cell: 10 % exactly 0, 30 % +-1, 2, 8 grid units of
    2^-32 and +-64, 128, 256 (the f32 granularity of the compare), 60 % log-uniform from 1e-9 out to 1e-3"""
    kind = rng.uniform(0, 1, n)
    sign = np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)
    units = rng.choice([1.0, 2.0, 8.0, 1.0, 2.0, 8.0, 64.0, 128.0, 256.0], n) / TWO32
    log = 10.0 ** rng.uniform(-9.0, np.log10(WINDOW * 0.98), n)
    d = np.where(kind < 0.10, 0.0, np.where(kind < 0.40, units, log))
    return sign * d


def _edge_distance(rng, n, st, g, rmax, nbins, lo=0.0, cutoff_share=0.4):
    """distances at (k + delta) dr, k an edge above lo (Angstrom), or at the cutoff; delta as edge_plant.offsets"""
    dr = st.dr
    klo = np.minimum(nbins, np.maximum(1, np.ceil(np.broadcast_to(lo, (n,)) / dr + 1e-9))).astype(np.int64)
    k = klo + np.floor(rng.uniform(0, 1, n) * (nbins + 1 - klo)).astype(np.int64)
    k = np.where(rng.uniform(0, 1, n) < cutoff_share, nbins, np.minimum(k, nbins))
    t, sign = E.offsets(rng, n, g)
    return E._distances(k * dr, t, sign, g * dr)


def _disc(rng, rho2):
    """(u, w) with u^2 + w^2 = max(rho2, 0), random direction"""
    rho = np.sqrt(np.maximum(rho2, 0.0))
    phi = rng.uniform(0, 2 * np.pi, len(rho))
    return rho * np.cos(phi), rho * np.sin(phi)


def _near_axis(rng, n, st, g, rmax, nbins, axis):
    """categories a (axis = 1, y) and b (axis = 2, z): |f| of the pair at the near threshold + offset"""
    L = st.L
    Lk = L[axis, axis]
    thr = st.thr_y if axis == 1 else st.thr_z
    raw = st.tau_y_raw if axis == 1 else st.tau_z_raw
    nominal = min(0.5 - raw, 0.5 - 4.0 / TWO32)
    T = np.where((rng.uniform(0, 1, n) < 0.7) & np.isfinite(thr), thr if np.isfinite(thr) else nominal, nominal)
    f = np.clip(T + dec_offsets(rng, n), 0.25, 0.5 - 1.0 / TWO32)
    sgn = np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)
    sub = rng.integers(0, 3, n)
    row = L[axis]                                  # the lattice vector of this axis in the orthogonalised frame
    free = (0, 2) if axis == 1 else (0, 1)         # the components that carry the rest of the distance
    v = np.zeros((n, 3))
    v[:, axis] = sgn * f * Lk
    # sub 0: the second image v - sgn row at an edge / the cutoff; 1: the first; 2: anywhere (mostly neither in range)
    second = v[:, axis] - sgn * Lk
    for s_, comp in ((0, second), (1, v[:, axis])):
        d = _edge_distance(rng, n, st, g, rmax, nbins, lo=np.abs(comp))
        u, w = _disc(rng, d * d - comp * comp)
        m = sub == s_
        for q, val in zip(free, (u, w)):
            v[m, q] = (val + (sgn * row[q] if s_ == 0 else 0.0))[m]
    m = sub == 2
    v[m, 0] = rng.uniform(-0.5, 0.5, m.sum()) * L[0, 0]
    v[m, free[1]] = rng.uniform(-0.45, 0.45, m.sum()) * L[free[1], free[1]]
    if axis == 1:           # |Z| stays clear of the slab wrap, so that fy is what was planted
        v[:, 2] = np.clip(v[:, 2], -0.45 * L[2, 2], 0.45 * L[2, 2])
    return v, sub


def _xwrap(rng, n, st, g, rmax, nbins, xw=True):
    """category c: sub 0: fx + c10 fy = +-(1/2 + offset); sub 1: fx = +-(1/2 + offset) (the wrap without the y term)"""
    L = st.L
    sub = (rng.uniform(0, 1, n) < (0.3 if xw else 0.5)).astype(np.int64)
    sgn = np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)
    w = sgn * (0.5 + dec_offsets(rng, n))
    reach = min(st.R / L[1, 1], 0.499)
    fy = np.where(rng.uniform(0, 1, n) < 0.5, rng.uniform(-reach, reach, n), rng.uniform(-0.02, 0.02, n))
    X = np.where(sub == 0, w, w + st.c10 * fy) * L[0, 0]
    # where half the x axis is within the cutoff: the nearer of the two images at an edge / the cutoff
    Xn = np.minimum(np.abs(X), np.abs(np.abs(X) - L[0, 0]))
    d = _edge_distance(rng, n, st, g, rmax, nbins, lo=Xn, cutoff_share=0.7)
    y, z = _disc(rng, d * d - Xn * Xn)
    inr = (Xn < rmax * (1.0 + 1e-3)) & (np.abs(y) < 0.02 * L[1, 1])
    v = np.zeros((n, 3))
    v[:, 0] = X
    v[:, 1] = np.where(inr & (sub == 0), y, fy * L[1, 1])
    # (sub 0 pins fx + c10 fy = X / L00 whatever Y is; sub 1 pins fx = X / L00 - c10 fy: Y stays as drawn)
    v[:, 2] = np.where(inr & (sub == 0), z, rng.uniform(-0.3, 0.3, n) * np.where(rng.uniform(0, 1, n) < 0.5, 0.05, 1.0) * L[2, 2])
    v[:, 2] = np.clip(v[:, 2], -0.45 * L[2, 2], 0.45 * L[2, 2])
    return v, sub


def _twin(rng, n, st, g, rmax, nbins):
    """category d: candidates v and v - V at distances d1, d2: sub 0 ties (to 0 .. a few ulp), 1 either side of the
    cutoff, 2 the nearer a bin below the farther"""
    V = st.V
    lv = float(np.linalg.norm(V))
    vh = V / lv
    vp = np.array([-vh[1], vh[0], 0.0])
    sub = rng.choice([0, 0, 1, 2], n)
    # ties: alpha = |V| / 2 (1 + eps), the pair as close to the cutoff / an edge as the lattice allows
    eps = np.where(rng.uniform(0, 1, n) < 0.3, 0.0, np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0) *
                   10.0 ** rng.uniform(-16.0, np.log10(WINDOW * 0.45), n))
    d_tie = np.maximum(_edge_distance(rng, n, st, g, rmax, nbins, lo=0.5 * lv, cutoff_share=0.6), 0.5 * lv * (1.0 + 1e-15))
    # either side of the cutoff / a bin apart
    e1, e2 = 10.0 ** rng.uniform(-12, -3, n), 10.0 ** rng.uniform(-12, -3, n)
    d1 = np.where(sub == 1, rmax * (1.0 - e1), _edge_distance(rng, n, st, g, rmax, nbins, lo=0.55 * rmax, cutoff_share=0.0))
    d2 = np.where(sub == 1, rmax * (1.0 + e2), d1 + st.dr)
    d2 = np.maximum(d2, (lv - d1) * (1.0 + 1e-12))          # (|V| <= d1 + d2: the lattice allows nothing closer)
    alpha = np.where(sub == 0, 0.5 * lv * (1.0 + eps), (d1 * d1 - d2 * d2 + lv * lv) / (2.0 * lv))
    dd = np.where(sub == 0, np.maximum(d_tie, np.abs(alpha)), d1)
    beta, z = _disc(rng, dd * dd - alpha * alpha)
    v = alpha[:, None] * vh + beta[:, None] * vp
    v[:, 2] = z
    flip = rng.uniform(0, 1, n) < 0.5                       # either of the two may be the one the kernel minimised
    v = np.where(flip[:, None], -v, v)
    return v, sub


def _face(rng, n, C, rmax):
    """category e: +-A / 2 (1 + delta) along the shortest axis (|A| = 2 rmax): both images at the cutoff"""
    q = int(np.argmin(np.linalg.norm(C, axis=1)))
    kind = rng.uniform(0, 1, n)
    sign = np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)
    delta = sign * np.where(kind < 0.1, 0.0, np.where(kind < 0.3, rng.integers(1, 9, n) * 2.0 ** -52,
                                                      10.0 ** rng.uniform(-12.0, np.log10(WINDOW * 0.9), n)))
    s = np.where(rng.uniform(0, 1, n) < 0.5, -0.5, 0.5) * (1.0 + delta)
    return s[:, None] * C[q][None, :], np.zeros(n, dtype=np.int64)


CATS = "abcde"


def categories(name, sts, default_rmax):
    code = CASES[name]["expect"][0]
    cats = ["c"]
    if any(np.isfinite(st.thr_y) for st in sts) and code not in (4, 9, 10, 11):
        cats.append("a")
    if any(np.isfinite(st.thr_z) for st in sts):
        cats.append("b")
    if code in (4, 9, 10, 11):
        cats.append("d")
    if default_rmax:
        cats.append("e")
    return sorted(cats)


class TriPlanted(object):
    def __init__(self, name, nbins, packed, sts, frame, i, j, cat, sub):
        self.name, self.nbins, self.packed, self.sts = name, nbins, packed, sts
        self.frame, self.i, self.j, self.cat, self.sub = frame, i, j, cat, sub

    def realised(self):
        """per planted pair, from the positions alone (float64): the signed offset of the pair from its decision (fractions
        of the cell; d: the difference of the two candidates' lengths over the shortest cell length) and which side"""
        pos = self.packed.pos
        cells = self.packed.cell.reshape(-1, 3, 3)
        off = np.full(len(self.i), np.nan)
        for f, st in enumerate(self.sts):
            C = cells[f if len(cells) > 1 else 0]
            m = self.frame == f
            d0 = pos[f, self.j[m]] - pos[f, self.i[m]]
            fx, fy, fz = st.folded(d0, C)
            cat, sub = self.cat[m], self.sub[m]
            o = np.full(m.sum(), np.nan)
            nominal_y = min(0.5 - st.tau_y_raw, 0.5 - 4.0 / TWO32)
            nominal_z = min(0.5 - st.tau_z_raw, 0.5 - 4.0 / TWO32)
            ty = st.thr_y if np.isfinite(st.thr_y) else nominal_y
            tz = st.thr_z if np.isfinite(st.thr_z) else nominal_z
            # a / b: the nearer of the threshold the kernel compares with and the nominal 1/2 - tau
            ay, az = np.abs(fy), np.abs(fz)
            o_a = np.where(np.abs(ay - ty) <= np.abs(ay - nominal_y), ay - ty, ay - nominal_y)
            o_b = np.where(np.abs(az - tz) <= np.abs(az - nominal_z), az - tz, az - nominal_z)
            o = np.where(cat == 0, o_a, o)
            o = np.where(cat == 1, o_b, o)
            w = np.where(sub == 0, fx + st.c10 * fy, fx)
            wf = w - np.floor(w)                        # in [0, 1): the wrap boundary at 1/2
            o = np.where(cat == 2, wf - 0.5, o)
            # d: candidate 1 (the y image the kernel minimised, x wrapped with it) against its twin
            L = st.L
            fy2 = fy - np.where(fy >= 0, 1.0, -1.0)
            x1 = fx + st.c10 * fy
            x1 = x1 - np.rint(x1)
            x2 = fx + st.c10 * fy2
            x2 = x2 - np.rint(x2)
            t1 = np.sqrt((L[0, 0] * x1) ** 2 + (L[1, 1] * fy) ** 2 + (L[2, 2] * fz) ** 2)
            t2 = np.sqrt((L[0, 0] * x2) ** 2 + (L[1, 1] * fy2) ** 2 + (L[2, 2] * fz) ** 2)
            o = np.where(cat == 3, (t1 - t2) / np.linalg.norm(C, axis=1).min(), o)
            q = int(np.argmin(np.linalg.norm(C, axis=1)))
            sq = (d0 @ np.linalg.inv(C))[:, q]
            o = np.where(cat == 4, (sq - np.floor(sq)) - 0.5, o)
            off[m] = o
        return off

    def counts(self):
        """category -> (pairs within WINDOW of their decision, below it, at or above it); "cx": the pairs of category c
        planted on fx = +-1/2, the x wrap without the y term"""
        off = self.realised()
        out = {}
        for k, c in enumerate(CATS):
            m = (self.cat == k)
            if c == "d":
                m &= self.sub < 2                       # ties and cutoff straddles; the bin-apart pairs are extra
            if c == "c":
                m &= self.sub == 0                      # the wrap with the y term; sub 1 (fx alone): "cx" below
            if not (self.cat == k).any():
                continue
            o = off[m]
            win = np.abs(o) <= WINDOW
            out[c] = (int(win.sum()), int((win & (o < 0)).sum()), int((win & (o >= 0)).sum()))
        o = off[(self.cat == CATS.index("c")) & (self.sub == 1)]
        win = np.abs(o) <= WINDOW
        out["cx"] = (int(win.sum()), int((win & (o < 0)).sum()), int((win & (o >= 0)).sum()))
        return out


def plant_tri(name, nbins, seed=0, n_atoms=2400, F=2, pair_share=0.92, form=None):
    """the planted trajectory of one case: F frames (per-frame cells: one per cell), most atoms in anchor-partner pairs
    split evenly over the categories that apply to the case, the rest random filler.  form: the case's cell in one of
    the forms of tests/cell_forms.py; the planting works from the metric of the cell as stored"""
    rng = np.random.default_rng(seed)
    cells = case_cells(name, form)
    F = len(cells) if len(cells) > 1 else F
    rmax = case_rmax(name, form)
    sts, g = stored_frames(name, nbins, form)
    default = CASES[name]["rmax"] is None
    cats = categories(name, sts, default)
    nums = numbers(n_atoms)
    N = len(nums)
    npair = int(pair_share * N) // 2
    frames, fr, ii, jj, cc, ss = [], [], [], [], [], []
    for f in range(F):
        C = cells[f if len(cells) > 1 else 0]
        st = sts[f if len(cells) > 1 else 0]
        perm = rng.permutation(N)
        a, b = perm[:npair], perm[npair:2 * npair]
        which = np.array([CATS.index(c) for c in cats])[np.arange(npair) % len(cats)]
        dpos = np.zeros((npair, 3))
        sub = np.zeros(npair, dtype=np.int64)
        for k in np.unique(which):
            m = which == k
            n = int(m.sum())
            if k == 0:
                v, s_ = _near_axis(rng, n, st, g, rmax, nbins, 1)
            elif k == 1:
                v, s_ = _near_axis(rng, n, st, g, rmax, nbins, 2)
            elif k == 2:
                v, s_ = _xwrap(rng, n, st, g, rmax, nbins, xw=CASES[name]["expect"][0] >= 5)
            elif k == 3:
                v, s_ = _twin(rng, n, st, g, rmax, nbins)
            if k == 4:
                d, s_ = _face(rng, n, C, rmax)
            else:
                d = st.to_cart(v, C)
            dpos[m] = d
            sub[m] = s_
        pos = (rng.uniform(0, 1, (N, 3)) + rng.integers(-1, 2, (N, 3))) @ C
        sa = E._anchor_frac(rng, npair)
        T = E._lattice_shift(rng, npair, False)
        mm = np.where(rng.uniform(0, 1, (npair, 1)) < 0.25, rng.integers(-1, 2, (npair, 3)), 0)
        ri = (sa + T) @ C
        pos[a] = ri
        pos[b] = ri + dpos + mm @ C
        frames.append(pos)
        fr.append(np.full(npair, f)); ii.append(a); jj.append(b); cc.append(which); ss.append(sub)
    packed = PackedTrajectory(np.stack(frames), cells if len(cells) > 1 else cells[0], nums)
    return TriPlanted(name, nbins, packed, sts if len(cells) > 1 else sts * F, np.concatenate(fr), np.concatenate(ii),
                      np.concatenate(jj), np.concatenate(cc), np.concatenate(ss))
