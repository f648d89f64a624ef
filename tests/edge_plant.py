"""Test infrastructure (the package never imports it): trajectories whose pairs sit just inside and just outside the
guard band of the fast pair paths.

Every fast kernel bins a pair by a cheap f32 candidate and re-decides it exactly only where the candidate lies within a
proven bound g of a decision: an RDF bin edge or the cutoff, a CN / BAD cutoff.  A band that is too narrow, or applied
wrongly, miscounts exactly the pairs planted here:

* RDF: anchor-partner pairs at d = (k + delta) dr, k an edge in 1 .. nbins (k = nbins is the cutoff);
* CN / BAD: pairs at d = rc (1 + delta) for every non-zero entry of the cutoff matrix, both species orders;
* BAD: a centre with two legs (inside the cutoff, or at rc (1 +- delta)) at angles theta = edge +- delta_theta;

delta signed and log-uniform over [0.01, 10] g, plus exact hits (delta = 0), one-ulp neighbours of the decision and a
tail down to 1e-12.  Anchors are non-dyadic random points, some within 1e-6 of a cell face (the partner wraps); a part
of the partners sits one lattice vector away; whole pairs are shifted by independent random lattice vectors, up to
|n| = 9000 where asked (below the 1e4 fallback of the fixed-point fold); directions are random unit vectors.

The band g restates the host's bounds: fast_guard_rel_rdf / fast_guard_rel (amof_amd/csrc/amof_internal.h, kappa from
guard_math.h) plus the fixed-point grid term g_m (rdf.hip, nbr.hip), checked against tests/native/guard_math_driver.cpp
by tests/test_guard_band_cpu.py.  It is the band of the plain tile / neighbour kernels; the ZF and TRI tile variants add
small terms of their own (fast_guard_zf / fast_guard_tri), the compact 16-bit frame records a coarser grid term
(guard_abs16), which `nbr_band(compact=True)` takes.  Every generator checks its own output: the planted pairs'
canonical distances, recomputed in float64, lie within 10 g of their decision, and pairs inside the band and pairs
outside it both exist -- a test cannot pass on a case that plants nothing."""

import numpy as np

from amof_amd.frames import PackedTrajectory

U = 2.0 ** -24
PERMS = ((0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (1, 0, 2), (2, 1, 0))


def _cells(cell):
    return np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)


def is_diagonal(cell):
    c = _cells(cell)
    return bool(np.all(c == c * np.eye(3)))


def kappa_lower(L):
    """guard_math.h kappa_lower: P = |L^-1| |L|, sqrt(||P||_1 ||P||_inf)"""
    P = np.abs(np.linalg.inv(L)) @ np.abs(L)
    return float(np.sqrt(P.sum(axis=0).max() * P.sum(axis=1).max()))


def kappa_rdf(cell):
    """guard_math.h kappa_rdf: the largest kappa of the metric's lower factor over the six stored axis orders"""
    k = 1.0
    for c in _cells(cell):
        for p in PERMS:
            rows = c[list(p)]
            k = max(k, kappa_lower(np.linalg.cholesky(rows @ rows.T)))
    return k


def kappa_cell(cell):
    """guard_math.h kappa_cell: P = |C^-1| |C| of the cell itself (the neighbour kernels' scale matrix)"""
    k = 1.0
    for c in _cells(cell):
        P = np.abs(np.linalg.inv(c)) @ np.abs(c)
        k = max(k, float(np.sqrt(P.sum(axis=0).max() * P.sum(axis=1).max())))
    return k


def csum(cell):
    """largest sum of the three cell-vector lengths: bounds how far the 2^-32 fixed-point grid moves a pair vector"""
    return float(max(np.linalg.norm(c, axis=1).sum() for c in _cells(cell)))


def rdf_eps(cell):
    """relative bound of the RDF tile paths' f32 chain (fast_guard_rel_rdf)"""
    if is_diagonal(cell):
        return 1.1 * (3.5 + 1.56) * U
    return 1.1 * (5.0 * kappa_rdf(cell) + 3.06) * U


def rdf_band(cell, rmax, nbins):
    """g_f = nbins eps_f + g_m in bins (rdf.hip, host side of the tile kernels)"""
    dr = rmax / nbins
    g_m = csum(cell) * 2.0 ** -31 / dr + nbins * 1e-12
    return nbins * rdf_eps(cell) + g_m


def nbr_band(cell, rc, compact=False):
    """rc guard_rel + guard_abs of the neighbour kernels (nbr.hip), relative to rc: fast_guard_rel + 3u (the cutoff in
    f32, r_in / r_out), the grid term csum 2^-31 (compact 16-bit records: csum 2^-15)"""
    if is_diagonal(cell):
        rel = 1.1 * (4.5 + 1.56) * U
    else:
        rel = 1.1 * (5.0 * kappa_cell(cell) + 3.06) * U
    rel += 3.0 * U
    g_abs = csum(cell) * (2.0 ** -15 if compact else 2.0 ** -31)
    return rel + g_abs / rc


def offsets(rng, n, g):
    """n signed offsets from a decision, in the units of g: 80 % log-uniform over [0.01, 10] g, 5 % exactly 0, 5 % one
    ulp either side (marked as nan: the caller steps the decision itself), 10 % a tail from 1e-12 up to 0.01 g"""
    kind = rng.uniform(0, 1, n)
    sign = np.where(rng.uniform(0, 1, n) < 0.5, -1.0, 1.0)
    t = sign * 10.0 ** rng.uniform(-2.0, 1.0, n)
    lo = np.log10(min(1e-12 / g, 1e-3))
    tail = sign * 10.0 ** rng.uniform(lo, -2.0, n)
    t = np.where(kind < 0.10, tail, t)
    t = np.where((kind >= 0.10) & (kind < 0.15), 0.0, t)
    t = np.where((kind >= 0.15) & (kind < 0.20), np.nan * sign, t)
    return t, sign


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1)[:, None]


def _anchor_frac(rng, n):
    """non-dyadic random fractional points, 15 % of them within 1e-6 of a cell face (either side)"""
    s = rng.uniform(0, 1, (n, 3))
    face = rng.uniform(0, 1, n) < 0.15
    ax = rng.integers(0, 3, n)
    near = rng.uniform(0, 1e-6, n)
    s[face, ax[face]] = np.where(rng.uniform(0, 1, face.sum()) < 0.5, near[face], 1.0 - near[face])
    return s


class Planted(object):
    """a PackedTrajectory plus what was planted in it: per planted pair its frame, atoms (i, j), the lattice offset m of
    the partner's planted image (pos_j - pos_i - m C is the planted vector), the decision D (Angstrom) and the band
    g_abs at D (Angstrom)"""

    def __init__(self, packed, frame, i, j, m, D, g_abs, g, kind):
        self.packed, self.frame, self.i, self.j, self.m = packed, frame, i, j, m
        self.D, self.g_abs, self.g, self.kind = D, g_abs, g, kind
        self.species = None

    def planted_distances(self):
        """canonical distances of the planted images, float64: d0 = r_j - r_i, minus the partner's lattice offset"""
        pos = self.packed.pos
        C = self.packed.cell if self.packed.cell.shape[0] > 1 else np.broadcast_to(self.packed.cell, (pos.shape[0], 3, 3))
        d = pos[self.frame, self.j] - pos[self.frame, self.i] - np.einsum("pk,pkc->pc", self.m, C[self.frame])
        return np.sqrt((d * d).sum(axis=1))

    def band_units(self):
        """signed offset of every planted pair from its decision, in units of the band"""
        return (self.planted_distances() - self.D) / self.g_abs

    def check(self, min_pairs=50):
        t = self.band_units()
        assert len(t) >= min_pairs, "only %d planted pairs" % len(t)
        near = np.abs(t) <= 10.0
        assert near.mean() >= 0.9, "only %.3f of the planted pairs within 10 g of a decision" % near.mean()
        inside = np.abs(t) <= 1.0
        assert inside.sum() >= 5 and (near & ~inside).sum() >= 5, (int(inside.sum()), int((near & ~inside).sum()))
        return self


def _lattice_shift(rng, n, far):
    """per pair: small shifts (|n| <= 2) for half of them; with far, the other half up to 9000 cells"""
    sh = rng.integers(-2, 3, (n, 3))
    if far:
        big = rng.uniform(0, 1, n) < 0.5
        sh[big] = rng.integers(-9000, 9001, (int(big.sum()), 3))
    return sh


def _place(rng, C, n_atoms, anchors, partners, dist, far, wrap_share=0.25):
    """positions of one frame: pairs (anchors[p], partners[p]) at dist[p] along random directions, every other atom a
    random point; returns (pos [N][3], m [P][3])"""
    P = len(anchors)
    pos = (rng.uniform(0, 1, (n_atoms, 3)) + rng.integers(-1, 2, (n_atoms, 3))) @ C
    sa = _anchor_frac(rng, P)
    T = _lattice_shift(rng, P, far)
    m = np.where(rng.uniform(0, 1, (P, 1)) < wrap_share, rng.integers(-1, 2, (P, 3)), 0)
    ri = (sa + T) @ C
    w = dist[:, None] * _unit(rng, P) + m @ C
    pos[anchors] = ri
    pos[partners] = ri + w
    return pos, m


def _distances(D, t, sign, g_abs):
    """planted distance at decision D with offset t (units of g_abs); nan: one ulp beside D"""
    ulp = np.where(sign > 0, np.nextafter(D, np.inf), np.nextafter(D, -np.inf))
    return np.where(np.isnan(t), ulp, D + np.nan_to_num(t) * g_abs)


def plant_rdf(cell, numbers, rmax, nbins, seed, F=None, pair_share=0.9, far=False):
    """RDF planting: the returned Planted's packed trajectory has F frames (or one per cell of an [F][3][3] cell); pairs
    at (k + delta) dr, k mostly in the upper half of the bins (where the f32 error is largest), 15 % at the cutoff"""
    rng = np.random.default_rng(seed)
    cells = _cells(cell)
    F = cells.shape[0] if F is None else F
    assert cells.shape[0] in (1, F)
    numbers = np.asarray(numbers)
    N = len(numbers)
    dr = rmax / nbins
    g = rdf_band(cells, rmax, nbins)
    npair = int(pair_share * N) // 2
    frames, fr, ii, jj, mm, DD = [], [], [], [], [], []
    for f in range(F):
        C = cells[f if cells.shape[0] > 1 else 0]
        perm = rng.permutation(N)
        a, b = perm[:npair], perm[npair:2 * npair]
        kmin = min(nbins, int(np.ceil(10.0 * g)) + 1)
        k = np.where(rng.uniform(0, 1, npair) < 0.7, rng.integers((nbins + 1) // 2, nbins + 1, npair),
                     rng.integers(1, nbins + 1, npair))
        k = np.where(rng.uniform(0, 1, npair) < 0.15, nbins, np.maximum(k, kmin))
        D = k * dr
        t, sign = offsets(rng, npair, g)
        pos, m = _place(rng, C, N, a, b, _distances(D, t, sign, g * dr), far)
        frames.append(pos)
        fr.append(np.full(npair, f)); ii.append(a); jj.append(b); mm.append(m); DD.append(D)
    packed = PackedTrajectory(np.stack(frames), cells, numbers)
    D = np.concatenate(DD)
    return Planted(packed, np.concatenate(fr), np.concatenate(ii), np.concatenate(jj), np.concatenate(mm), D,
                   np.full(len(D), g * dr), g, "rdf").check()


def _species(numbers):
    kinds = sorted(set(int(z) for z in numbers))
    return kinds, np.array([kinds.index(int(z)) for z in numbers], dtype=np.int32)


def _pair_up(rng, sp, rcm, n_wanted, taken):
    """anchor / partner atoms whose species pair carries a cutoff; atoms in `taken` are left alone"""
    S = rcm.shape[0]
    pools = {s: [int(x) for x in rng.permutation(np.nonzero((sp == s) & ~taken)[0])] for s in range(S)}
    a_out, b_out = [], []
    for i in rng.permutation(np.nonzero(~taken)[0]):
        if len(a_out) >= n_wanted:
            break
        i = int(i)
        si = sp[i]
        if i not in pools[si]:
            continue
        pools[si].remove(i)
        cand = [s for s in range(S) if rcm[si, s] > 0 and pools[s]]
        if not cand:
            pools[si].append(i)
            continue
        j = pools[cand[rng.integers(0, len(cand))]].pop()
        a_out.append(i); b_out.append(j)
    return np.array(a_out, dtype=np.int64), np.array(b_out, dtype=np.int64)


def plant_nbr(cell, numbers, rcm, seed, F=None, pair_share=0.6, far=False, compact=False, triples=None,
              angle_edges=None, triple_share=0.3):
    """CN / BAD planting: pairs at rc (1 + delta) for every species pair with a cutoff (rcm indexed by the species order
    of sorted atomic numbers).  triples: (A, B) centre / leg species -- a centre of A with two B legs (70 % of the legs
    inside the cutoff, 30 % at rc (1 +- delta)) at angles within 1e-7 degrees of an interior edge of angle_edges (some
    exactly on it).  The band is relative: nbr_band(compact) of each pair's cutoff."""
    rng = np.random.default_rng(seed)
    cells = _cells(cell)
    F = cells.shape[0] if F is None else F
    assert cells.shape[0] in (1, F)
    numbers = np.asarray(numbers)
    kinds, sp = _species(numbers)
    rcm = np.asarray(rcm, dtype=np.float64)
    N = len(numbers)
    frames, fr, ii, jj, mm, DD, GG, ang = [], [], [], [], [], [], [], []
    gmin = np.inf
    for f in range(F):
        C = cells[f if cells.shape[0] > 1 else 0]
        taken = np.zeros(N, bool)
        tri_atoms = []
        if triples:
            # centre + two legs per triple: 3 atoms each, drawn from the species the triple names
            n_tri = int(triple_share * N) // 3
            for _ in range(n_tri):
                A, B = triples[rng.integers(0, len(triples))]
                ca = np.nonzero((sp == A) & ~taken)[0]
                if len(ca) == 0:
                    continue
                c = int(rng.choice(ca))
                taken[c] = True
                cb = np.nonzero((sp == B) & ~taken)[0]
                if len(cb) < 2:
                    taken[c] = False
                    continue
                l1, l2 = (int(x) for x in rng.choice(cb, 2, replace=False))
                taken[[l1, l2]] = True
                tri_atoms.append((c, l1, l2, A, B))
        a, b = _pair_up(rng, sp, rcm, int(pair_share * N) // 2, taken)
        rc = rcm[sp[a], sp[b]]
        g = np.array([nbr_band(C, r, compact) for r in rc])
        t, sign = offsets(rng, len(a), float(np.median(g)) if len(g) else 1e-6)
        D = rc
        dist = _distances(D, t, sign, g * rc)
        pos, m = _place(rng, C, N, a, b, dist, far)
        fr.append(np.full(len(a), f)); ii.append(a); jj.append(b); mm.append(m); DD.append(D); GG.append(g * rc)
        if len(g):
            gmin = min(gmin, float(g.min()))
        # triples: legs along u1 and u2 = cos(theta) u1 + sin(theta) w, w a random unit vector normal to u1
        for (c, l1, l2, A, B) in tri_atoms:
            r = rcm[A, B]
            gl = nbr_band(C, r, compact)
            legs = []
            for _ in range(2):
                if rng.uniform() < 0.7:
                    legs.append(r * rng.uniform(0.55, 0.97))
                else:
                    tt, sg = offsets(rng, 1, gl)
                    legs.append(float(_distances(np.array([r]), tt, sg, gl * r)[0]))
            inner = np.asarray(angle_edges)[1:-1]
            inner = inner[(inner > 20.0) & (inner < 160.0)]
            e = float(rng.choice(inner))
            k = rng.uniform()
            theta = e if k < 0.2 else e + (1 if rng.uniform() < 0.5 else -1) * 10.0 ** rng.uniform(-13, -7)
            u1 = _unit(rng, 1)[0]
            w = _unit(rng, 1)[0]
            w = w - np.dot(w, u1) * u1
            w /= np.linalg.norm(w)
            th = np.radians(theta)
            u2 = np.cos(th) * u1 + np.sin(th) * w
            T = _lattice_shift(rng, 1, far)[0]
            rc_pos = (_anchor_frac(rng, 1)[0] + T) @ C
            pos[c] = rc_pos
            pos[l1] = rc_pos + legs[0] * u1
            pos[l2] = rc_pos + legs[1] * u2
            ang.append((f, c, l1, l2, e))
        frames.append(pos)
    packed = PackedTrajectory(np.stack(frames), cells, numbers)
    out = Planted(packed, np.concatenate(fr), np.concatenate(ii), np.concatenate(jj), np.concatenate(mm),
                  np.concatenate(DD), np.concatenate(GG), gmin, "nbr")
    out.species = sp
    out.angles = np.array(ang, dtype=np.float64).reshape(-1, 5)
    out.check()
    if triples:
        assert len(out.angles) >= 10, "only %d planted triples" % len(out.angles)
        f, c, l1, l2 = (out.angles[:, q].astype(np.int64) for q in range(4))
        p = packed.pos
        v1, v2 = p[f, l1] - p[f, c], p[f, l2] - p[f, c]
        cosv = (v1 * v2).sum(axis=1) / np.linalg.norm(v1, axis=1) / np.linalg.norm(v2, axis=1)
        theta = np.degrees(np.arccos(np.clip(cosv, -1.0, 1.0)))
        off = np.abs(theta - out.angles[:, 4])
        assert np.all(off < 1e-5), off.max()           # (shifts up to 9000 cells cost a few 1e-9 degrees)
    return out
