"""Float64 numpy restatement of the bond reorientation sums (include/amof_hip.h, amof_bond_reorientation), written from the
definition; it never calls the product.

h_ij(f) is tests/bond_ref.py's ``bonded``.  d_ij(f) is the nearest of the 27 images around the rounded fractional
difference of r_j - r_i (the canonical minimum image for every pair closer than half the smallest cell height).  Per set and
lag, over the lag's origins k and the ordered pairs with h(k) h(k + m) = 1:
    n = number of terms (exact),  sum P1 = sum cos,  sum P2 = sum (3 cos^2 - 1) / 2       (float64 sums)
with cos = a.b / sqrt(a.a b.b), clipped to [-1, 1], a = d(k), b = d(k + m).

The error budget (derived, not tuned against the GPU).  The library's term is rint(P 2^e) 2^-e of ITS float64 evaluation
of P; the budget of a term bounds |library term - this term| when both evaluations are correct:
  * the rounding to the fixed-point grid: 2^-(e + 1);
  * the two vectors.  Both evaluations start from the same d0 = fl(r_j - r_i) and subtract the same lattice vector n C
    from it in different operation orders.  Every intermediate of either is at most
        M = max_x |d0_x| + sum_k (|n_k| + 1) sum_x |C_kx|
    in magnitude, so every rounding costs at most eps/2 M (eps = 2^-52).  The library's chain rounds 3 times per component
    (three fma), this restatement at most 12 times (n @ C: 5, the subtraction: 1, the image shift @ C: 5, its addition: 1):
    the components differ by at most 7.5 eps M, the vectors by at most sqrt(3) 7.5 eps M < 13 eps M in norm.
    A unit vector moves by at most 2 |delta| / |a| when a moves by delta, and the cosine of two unit vectors by at most the
    sum of their moves: 26 eps M (1 / |a| + 1 / |b|), rounded up to K = 32 for the terms of second order.
  * the arithmetic of the cosine itself: three dot products (3 roundings each, relative to |a| |b| at most), a product, a
    square root and a division in either evaluation, under 8 eps each side: 16 eps.
  so  dcos = K eps M (1 / |a| + 1 / |b|) + 16 eps,   budget(P1) = 2^-(e+1) + dcos,
  and P2 = 1.5 cos^2 - 0.5 has |dP2| <= 3 |cos| dcos + 2 eps (its own two roundings per side):
      budget(P2) = 2^-(e+1) + 3 dcos + 2 eps.
The budget of a sum is the sum of its terms' budgets, plus n^2 eps / 2 for this restatement's own float64 summation (n
additions of partial sums of at most n in magnitude) and the conversion of the library's integer sum to float64.
A wrong image, a swapped atom or a missed term moves a sum by O(0.1) per term; the tests require every term's budget to stay
below 2^-30 (``worst``), which needs |d| above about 0.05 A for every bonded pair."""

import collections
import itertools

import numpy as np

from tests import bond_ref

EPS = 2.0 ** -52
K = 32.0

Result = collections.namedtuple("Result", "n sums budget worst")
# n [n_sets][W] int64; sums, budget [n_sets][W][2] float64 (P1, P2); worst: the largest budget of a single term


def scale_log2(n_a, n_b, n_0):
    """e_s = min(40, 62 - bit_length(n_A n_B n_0)); ValueError below 20"""
    e = min(40, 62 - (int(n_a) * int(n_b) * int(n_0)).bit_length())
    if e < 20:
        raise ValueError("scale below 2^20")
    return e


def scales(numbers, sets, F, stride=1):
    """e_s of every set [(A number, B number, rc)] of a trajectory with F frames"""
    numbers = np.asarray(numbers)
    n0 = len(bond_ref.origins(F, 0, stride))
    return [scale_log2(int((numbers == a).sum()), int((numbers == b).sum()), n0) for a, b, _ in sets]


def vectors(pos_i, pos_j, cell, pbc):
    """(d [len(i)][len(j)][3], M [len(i)][len(j)]) of one frame: the nearest of the 27 images and the magnitude bound M of the
    module docstring"""
    d0 = pos_j[None, :, :] - pos_i[:, None, :]
    n = np.rint(d0 @ np.linalg.inv(cell)) * np.asarray(pbc, dtype=np.float64)
    base = d0 - n @ cell
    best = np.full(d0.shape[:2], np.inf)
    vec = np.zeros_like(d0)
    ranges = [(-1, 0, 1) if pbc[x] else (0,) for x in range(3)]
    for sh in itertools.product(*ranges):
        d = base + np.asarray(sh, dtype=np.float64) @ cell
        r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        take = r2 < best
        best = np.where(take, r2, best)
        vec = np.where(take[..., None], d, vec)
    M = np.abs(d0).max(axis=-1) + (np.abs(n) + 1.0) @ np.abs(cell).sum(axis=1)
    return vec, M


def reorientation(pos, cell, numbers, sets, windows, stride=1, pbc=(True, True, True), centres=None, scale=None):
    """``Result`` for sets [(A number, B number, rc)]; scale: e_s per set (default: ``scales``).  ZeroDivisionError for a
    contributing term with a zero-length vector"""
    pos = np.asarray(pos, dtype=np.float64)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    F = pos.shape[0]
    if scale is None:
        scale = scales(numbers, sets, F, stride)
    W = len(windows)
    n_out = np.zeros((len(sets), W), dtype=np.int64)
    sums = np.zeros((len(sets), W, 2))
    budget = np.zeros((len(sets), W, 2))
    worst = 0.0
    for s, (a_number, b_number, rc) in enumerate(sets):
        h, ia, ib = bond_ref.bonded(pos, cell, numbers, a_number, b_number, rc, pbc, centres)
        if not h.any():
            continue
        vec = np.zeros(h.shape + (3,))
        M = np.zeros(h.shape)
        for f in range(F):
            vec[f], M[f] = vectors(pos[f, ia], pos[f, ib], cells[0 if len(cells) == 1 else f], pbc)
        quantum = 2.0 ** -(int(scale[s]) + 1)
        for w, m in enumerate(windows):
            ks = np.asarray(bond_ref.origins(F, int(m), stride), dtype=np.int64)
            if len(ks) == 0:
                continue
            mask = h[ks] & h[ks + m]
            a, b = vec[ks][mask], vec[ks + m][mask]
            n = len(a)
            n_out[s, w] = n
            if n == 0:
                continue
            aa, bb = np.einsum("ij,ij->i", a, a), np.einsum("ij,ij->i", b, b)
            if np.any(aa * bb == 0.0):
                raise ZeroDivisionError("Undefined angle")
            c = np.clip(np.einsum("ij,ij->i", a, b) / np.sqrt(aa * bb), -1.0, 1.0)
            p2 = 1.5 * c * c - 0.5
            Mt = np.maximum(M[ks][mask], M[ks + m][mask])
            dcos = K * EPS * Mt * (1.0 / np.sqrt(aa) + 1.0 / np.sqrt(bb)) + 16.0 * EPS
            b1, b2 = quantum + dcos, quantum + 3.0 * dcos + 2.0 * EPS
            sums[s, w] = (c.sum(), p2.sum())
            # (+ the float64 summation of this restatement: n additions of partial sums of at most n in magnitude)
            budget[s, w] = (b1.sum() + 0.5 * n * n * EPS, b2.sum() + 0.5 * n * n * EPS)
            worst = max(worst, float(b1.max()), float(b2.max()))
    return Result(n_out, sums, budget, worst)


def check(got, scale, want):
    """the library's ``out [n_sets][W][3]`` (int64) and ``scale_log2`` against a ``Result``: n exactly, the sums within the
    budget; returns the largest |difference| / budget seen"""
    got = np.asarray(got).view(np.int64) if np.asarray(got).dtype == np.uint64 else np.asarray(got, dtype=np.int64)
    assert got.shape == want.n.shape + (3,), (got.shape, want.n.shape)
    assert np.array_equal(got[:, :, 0], want.n), (got[:, :, 0].tolist(), want.n.tolist())
    q = np.ldexp(1.0, -np.asarray(scale, dtype=np.int64))[:, None, None]
    diff = np.abs(got[:, :, 1:].astype(np.float64) * q - want.sums)
    assert np.all(diff <= want.budget), (diff.max(), np.argwhere(diff > want.budget)[:4].tolist())
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.nanmax(np.where(want.budget > 0, diff / want.budget, 0.0))) if diff.size else 0.0
