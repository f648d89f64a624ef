"""Float64 numpy restatement of the bond order parameters (include/amof_hip.h, amof_bond_order), written from the definition;
it never calls the product.

Neighbours are tests/bond_ref.py's ``bonded`` (amof_cn_count's decision), the vectors tests/reorientation_ref.py's ``vectors``
(the nearest of the 27 images around the rounded fractional difference: the canonical minimum image for every pair closer
than half the smallest cell height).  Per centre i of a set (A, B) with n neighbours, over the unordered pairs j < k of its
unit vectors:
    T_l = sum P_l(c_jk),    U = sum (c_jk + 1/3)^2,    c_jk = u_j . u_k clipped to [-1, 1]        (float64 sums)
    q_l = sqrt(max(0, n + 2 T_l)) / n   (n >= 1),      q_tet = 1 - 3/8 U   (n == 4)

The error budget (derived, not tuned against the GPU).  The library's term is llrint(P 2^E) 2^-E, E = 40, of ITS float64
evaluation of P; the budget of a term bounds |library term - this term| when both evaluations are correct:
  * the rounding to the fixed-point grid: 2^-(E + 1);
  * the cosine.  ``dcos`` is reorientation_ref's bound on the difference of the two evaluations' cosines of one pair of
    vectors, dcos = K eps M (1 / |a| + 1 / |b|) + 16 eps (derived there: both start from the same fl(r_j - r_i) and subtract
    the same lattice vector in different operation orders; M bounds every intermediate).  Since |P_l'(x)| <= l (l + 1) / 2 on
    [-1, 1], P_l moves by at most (l (l + 1) / 2) dcos;
  * the recurrence itself: l steps of three multiplications, a subtraction and a division on values of magnitude at most
    2 l + 1 relative to |P| <= 1 -- the Bonnet recurrence is forward stable on [-1, 1] -- under 2 l eps each side: 4 l eps.
  so  budget(P_l) = 2^-(E+1) + (l (l + 1) / 2) dcos + 4 l eps.
  * (c + 1/3)^2 has |d/dc| = 2 |c + 1/3| <= 8/3 and three roundings per side:
      budget((c + 1/3)^2) = 2^-(E+1) + (8/3) dcos + 4 eps.
The budget of T_l or U is the sum of its terms' budgets, plus p^2 eps / 2 for this restatement's own float64 summation of
p terms of magnitude at most 16/9.  A wrong image, a swapped atom or a missed neighbour moves a sum by O(0.1) per term; the
tests require every single term's budget to stay below 2^-30 (``worst``), which needs every bonded pair further apart than
about 0.05 A."""

import collections

import numpy as np

from tests import bond_ref
from tests import reorientation_ref

EPS = reorientation_ref.EPS
K = reorientation_ref.K
E = 40
QUANTUM = 2.0 ** -(E + 1)

Result = collections.namedtuple("Result", "n T U budget_T budget_U worst atoms")
# per set (a list over the sets): n [F][N_A] int64; T, budget_T [F][N_A][n_l]; U, budget_U [F][N_A]; atoms [N_A] (atom indices of
# the centres); worst: the largest budget of a single term over everything


def legendre(c, lmax):
    """[P_0 .. P_lmax](c) by the Bonnet recurrence (m + 1) P_{m+1} = (2m + 1) c P_m - m P_{m-1}"""
    c = np.asarray(c, dtype=np.float64)
    p = [np.ones_like(c), c.copy()]
    for m in range(1, lmax):
        p.append((((2 * m + 1) * c) * p[m] - m * p[m - 1]) / (m + 1))
    return p[:lmax + 1]


def shell(vectors, l):
    """(q_l for every l, q_tet or None) of ONE shell of neighbour vectors, in plain float64 (known-answer tests)"""
    v = np.asarray(vectors, dtype=np.float64)
    n = len(v)
    u = v / np.sqrt((v * v).sum(axis=1))[:, None]
    j, k = np.triu_indices(n, 1)
    c = np.clip((u[j] * u[k]).sum(axis=1), -1.0, 1.0)
    p = legendre(c, max(l))
    q = [float(np.sqrt(max(0.0, n + 2.0 * p[x].sum())) / n) for x in l]
    qtet = float(1.0 - 0.375 * ((c + 1.0 / 3.0) ** 2).sum()) if n == 4 else None
    return q, qtet


def order(pos, cell, numbers, sets, l, pbc=(True, True, True)):
    """``Result`` for sets [(A number, B number, rc)] and degrees l.  ZeroDivisionError for a zero-length bond vector"""
    pos = np.asarray(pos, dtype=np.float64)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    F = pos.shape[0]
    l = [int(x) for x in l]
    lmax = max(l)
    out = Result([], [], [], [], [], 0.0, [])
    worst = 0.0
    for a_number, b_number, rc in sets:
        if rc > 0.0:
            h, ia, ib = bond_ref.bonded(pos, cell, numbers, a_number, b_number, rc, pbc)
        else:
            ia = np.nonzero(np.asarray(numbers) == a_number)[0]
            ib = np.nonzero(np.asarray(numbers) == b_number)[0]
            h = np.zeros((F, len(ia), len(ib)), dtype=bool)
        n = h.sum(axis=2).astype(np.int64)
        T = np.zeros((F, len(ia), len(l)))
        U = np.zeros((F, len(ia)))
        bT = np.zeros((F, len(ia), len(l)))
        bU = np.zeros((F, len(ia)))
        for f in range(F):
            if not h[f].any():
                continue
            vec, M = reorientation_ref.vectors(pos[f, ia], pos[f, ib], cells[0 if len(cells) == 1 else f], pbc)
            for i in np.nonzero(n[f] >= 1)[0]:
                nb = np.nonzero(h[f, i])[0]
                v, m = vec[i, nb], M[i, nb]
                r = np.sqrt((v * v).sum(axis=1))
                if np.any(r == 0.0):
                    raise ZeroDivisionError("Undefined angle")
                if len(nb) < 2:
                    continue
                u = v / r[:, None]
                j, k = np.triu_indices(len(nb), 1)
                c = np.clip((u[j] * u[k]).sum(axis=1), -1.0, 1.0)
                dcos = K * EPS * np.maximum(m[j], m[k]) * (1.0 / r[j] + 1.0 / r[k]) + 16.0 * EPS
                p = legendre(c, lmax)
                own = 0.5 * len(c) * len(c) * EPS
                for x, lx in enumerate(l):
                    term = QUANTUM + 0.5 * lx * (lx + 1) * dcos + 4.0 * lx * EPS
                    T[f, i, x] = p[lx].sum()
                    bT[f, i, x] = term.sum() + own
                    worst = max(worst, float(term.max()))
                term = QUANTUM + (8.0 / 3.0) * dcos + 4.0 * EPS
                U[f, i] = ((c + 1.0 / 3.0) ** 2).sum()
                bU[f, i] = term.sum() + own
                worst = max(worst, float(term.max()))
        out.n.append(n)
        out.T.append(T)
        out.U.append(U)
        out.budget_T.append(bT)
        out.budget_U.append(bU)
        out.atoms.append(ia)
    return out._replace(worst=worst)


def check(per_atom, want):
    """the library's ``per_atom [F][n_sets][N][2 + n_l]`` against a ``Result``: n exactly (-1 off the centre species), T_l and
    U within the budget; returns the largest |difference| / budget seen"""
    pa = np.asarray(per_atom, dtype=np.int64)
    ratio = 0.0
    q = np.ldexp(1.0, -E)
    for s in range(len(want.n)):
        atoms = want.atoms[s]
        n_l = want.T[s].shape[-1]
        rows = pa[:, s][:, atoms]
        others = np.setdiff1d(np.arange(pa.shape[2]), atoms)
        assert np.all(pa[:, s][:, others][..., 0] == -1) and not pa[:, s][:, others][..., 1:].any(), s
        assert np.array_equal(rows[..., 0], want.n[s]), (s, np.argwhere(rows[..., 0] != want.n[s])[:4].tolist())
        dT = np.abs(rows[..., 1:1 + n_l].astype(np.float64) * q - want.T[s])
        dU = np.abs(rows[..., 1 + n_l].astype(np.float64) * q - want.U[s])
        assert np.all(dT <= want.budget_T[s]), (s, float(dT.max()), np.argwhere(dT > want.budget_T[s])[:4].tolist())
        assert np.all(dU <= want.budget_U[s]), (s, float(dU.max()), np.argwhere(dU > want.budget_U[s])[:4].tolist())
        with np.errstate(divide="ignore", invalid="ignore"):
            for d, b in ((dT, want.budget_T[s]), (dU, want.budget_U[s])):
                if d.size:
                    ratio = max(ratio, float(np.nanmax(np.where(b > 0, d / b, 0.0))))
    return ratio


def q_of(n, T, U):
    """(q_l [...][n_l], q_tet [...]) from the library's integers by the formulas of the header (IEEE sqrt, division, ldexp: the
    kernels' bits); NaN where undefined"""
    n = np.asarray(n, dtype=np.int64)
    T = np.asarray(T, dtype=np.int64)
    U = np.asarray(U, dtype=np.int64)
    Q = np.maximum(0, n[..., None] * (1 << E) + 2 * T)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.sqrt(np.ldexp(Q.astype(np.float64), -E)) / n[..., None].astype(np.float64)
    q = np.where(n[..., None] >= 1, q, np.nan)
    qt = np.where(n == 4, 1.0 - 0.375 * np.ldexp(U.astype(np.float64), -E), np.nan)
    return q, qt


def from_per_atom(per_atom, n_l, nbins, nbins_tet):
    """(hist [n_sets][n_l][nbins], hist_tet [n_sets][nbins_tet], frame_sums [F][n_sets][4 + n_l + 1]) that the definition
    gives for per-atom integers ``[F][n_sets][N][2 + n_l]`` -- bins and sums exactly as the header states them"""
    pa = np.asarray(per_atom, dtype=np.int64)
    F, S, N, _ = pa.shape
    hist = np.zeros((S, n_l, nbins), dtype=np.uint64)
    hist_tet = np.zeros((S, nbins_tet), dtype=np.uint64)
    sums = np.zeros((F, S, 4 + n_l + 1), dtype=np.int64)
    for s in range(S):
        n = pa[:, s, :, 0]
        centre = n >= 0
        q, qt = q_of(np.where(centre, n, 0), pa[:, s, :, 1:1 + n_l], pa[:, s, :, 1 + n_l])
        nn = np.where(centre, n, 0)
        sums[:, s, 0] = nn.sum(axis=1)
        sums[:, s, 1] = (nn >= 1).sum(axis=1)
        sums[:, s, 2] = (nn == 4).sum(axis=1)
        sums[:, s, 3] = (nn * (nn - 1) // 2).sum(axis=1)
        has = nn >= 1
        for x in range(n_l):
            qx = q[..., x][has]
            b = np.minimum((qx * float(nbins)).astype(np.int64), nbins - 1)
            hist[s, x] = np.bincount(b, minlength=nbins).astype(np.uint64)
            sums[:, s, 4 + x] = np.where(has, np.rint(np.where(has, q[..., x], 0.0) * 2.0 ** 30), 0.0).astype(np.int64).sum(axis=1)
        four = nn == 4
        b = np.minimum(((qt[four] + 3.0) * 0.25 * float(nbins_tet)).astype(np.int64), nbins_tet - 1)
        hist_tet[s] = np.bincount(b, minlength=nbins_tet).astype(np.uint64)
        sums[:, s, 4 + n_l] = np.where(four, np.rint(np.where(four, qt, 0.0) * 2.0 ** 30), 0.0).astype(np.int64).sum(axis=1)
    return hist, hist_tet, sums
