"""Numpy restatement of the Lindemann sums (include/amof_hip.h, amof_lindemann), written from the definition; it never calls
the product and knows nothing of the kernels' chunk order.

Blocks: nb = (F - B) // S + 1, block b covers the frames [b S, b S + B).  h_ij(f) is tests/bond_ref.py's ``bonded`` (pairs within
1e-9 rc of the cutoff re-decided in the canonical arithmetic).  d_ij(f) is the length of the nearest of the 27 images around
the rounded fractional difference of r_j - r_i (tests/reorientation_ref.py's ``vectors``: the canonical minimum image for
every pair closer than half the smallest cell height, and the nearest image beyond).  Per pair of a block, in long double and
in two passes (mean first, then the mean of the squared deviations): delta = sqrt(var) / mean.

The error budget of a pair's delta (derived, not tuned against the GPU).  eps = 2^-52.
  * the distances.  Library and restatement start from the same d0 = fl(r_j - r_i) and subtract the same lattice vector in
    different operation orders: the vectors differ by at most 13 eps M in norm (reorientation_ref.py's derivation, M its
    magnitude bound); norm2 and the square root round about twice per side: Ed = max over the block of (13 eps M + 4 eps d).
  * the library's moments are sums of e = d - c with c = d(first frame), |e| <= E = max |d - c| + 2 Ed:
      m1 = S1 / B:  the perturbed distances move it by 2 Ed (d and c), B additions of partial sums of at most B E in
                    magnitude and the division by another B eps E:                     err_m1 = 2 Ed + B eps E
      q = S2 / B:   a term e^2 moves by 2 E 2 Ed, the fma chain and the division by B eps E^2:   err_q = 4 E Ed + B eps E^2
      var = q - m1^2:                                              err_var = err_q + 2 E err_m1 + 2 eps E^2
    (the two-pass long-double variance of this restatement has no cancellation and errs far below that).
  * sqrt: |sqrt(v') - sqrt(v)| <= min(|v' - v| / sqrt(v), sqrt(|v' - v|)):   err_sd = min(err_var / sd, sqrt(err_var))
  * mean = c + m1: err_mean = err_m1 + Ed + eps mean; the quotient and the root round once more each:
      budget = (err_sd + delta err_mean) / (mean - err_mean) + 4 eps delta
The library's term is llrint(delta 2^e) 2^-e: it lies within 2^-(e + 1) + budget of this delta.  The budget of a sum is the sum
over its terms, plus n^2 eps / 2 sqrt(B) for this restatement's own float64 summation.  A static pair has E = 0: budget 0, and
delta is exactly 0 on both sides.  A wrong image, a swapped atom, a missed frame or a wrong block moves delta by O(0.01); the
tests require every pair's budget to stay below 2^-30 (``worst``) and no delta within its budget of a histogram edge."""

import collections
import math

import numpy as np

from tests import bond_ref
from tests import reorientation_ref

EPS = 2.0 ** -52

Block = collections.namedtuple("Block", "i j delta budget")         # the pairs of a (block, set): atom indices, float64 arrays
Result = collections.namedtuple("Result", "blocks starts B worst")  # blocks[b][s]: Block


def block_starts(F, B, S):
    if B < 2 or B > F or S < 1:
        raise ValueError("bad block arithmetic")
    return [b * S for b in range((F - B) // S + 1)]


def scale_log2(n_a, n_b, B):
    """e_s = min(40, 62 - bit_length(n_A n_B ceil(sqrt(B)))); ValueError below 20"""
    r = math.isqrt(B)
    if r * r < B:
        r += 1
    e = min(40, 62 - (int(n_a) * int(n_b) * r).bit_length())
    if e < 20:
        raise ValueError("scale below 2^20")
    return e


def scales(numbers, sets, B):
    numbers = np.asarray(numbers)
    return [scale_log2(int((numbers == a).sum()), int((numbers == b).sum()), B) for a, b, _ in sets]


def series_delta(d, M=None):
    """(delta, budget) of distance series d [B][n] (float64), M [B][n] the magnitude bounds (default: the distances themselves)"""
    d = np.asarray(d, dtype=np.float64)
    B = d.shape[0]
    M = d if M is None else M
    ld = d.astype(np.longdouble)
    mean = ld.sum(axis=0) / B
    var = ((ld - mean) ** 2).sum(axis=0) / B
    sd = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore"):
        delta = np.where(var == 0, 0.0, sd / mean).astype(np.float64)
    Ed = (13.0 * EPS * M + 4.0 * EPS * d).max(axis=0)
    E = np.abs(d - d[0]).max(axis=0)
    E = np.where(E > 0, E + 2.0 * Ed, 0.0)
    err_m1 = np.where(E > 0, 2.0 * Ed + B * EPS * E, 0.0)
    err_var = 4.0 * E * Ed + B * EPS * E * E + 2.0 * E * err_m1 + 2.0 * EPS * E * E
    sdf, meanf = sd.astype(np.float64), mean.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        err_sd = np.where(sdf > 0, np.minimum(err_var / sdf, np.sqrt(err_var)), np.sqrt(err_var))
        err_mean = err_m1 + np.where(E > 0, Ed, 0.0) + EPS * meanf
        budget = np.where(E > 0, (err_sd + delta * err_mean) / (meanf - err_mean) + 4.0 * EPS * delta, 0.0)
    return delta, budget


def lindemann(pos, cell, numbers, sets, B, S=1, select=0, pbc=(True, True, True), centres=None, tables=None):
    """``Result`` for sets [(A number, B number, rc)]; select 0: the pairs bonded at the block start, 1: at frame 0.  tables
    (optional dict): the distance tables of a trajectory's species pairs, kept between calls that differ in the blocks only"""
    pos = np.asarray(pos, dtype=np.float64)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    numbers = np.asarray(numbers)
    F = pos.shape[0]
    starts = block_starts(F, B, S)
    hframes = [0] if select else starts
    out = [[None] * len(sets) for _ in starts]
    worst = 0.0
    for s, (a_number, b_number, rc) in enumerate(sets):
        empty = Block(np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0), np.zeros(0))
        if not rc > 0 or not (numbers == a_number).any() or not (numbers == b_number).any():
            for b in range(len(starts)):
                out[b][s] = empty
            continue
        hcells = cells if len(cells) == 1 else cells[hframes]
        h, ia, ib = bond_ref.bonded(pos[hframes], hcells, numbers, a_number, b_number, rc, pbc, centres)
        key = (a_number, b_number, centres)
        if tables is not None and key in tables:
            D, M = tables[key]
        else:
            D = np.zeros((F, len(ia), len(ib)))
            M = np.zeros((F, len(ia), len(ib)))
            for f in range(F):
                vec, M[f] = reorientation_ref.vectors(pos[f, ia], pos[f, ib], cells[0 if len(cells) == 1 else f], pbc)
                D[f] = np.sqrt(vec[..., 0] * vec[..., 0] + vec[..., 1] * vec[..., 1] + vec[..., 2] * vec[..., 2])
            if tables is not None:
                tables[key] = (D, M)
        for b, k in enumerate(starts):
            x, y = np.nonzero(h[0 if select else b])
            if len(x) == 0:
                out[b][s] = empty
                continue
            delta, budget = series_delta(D[k:k + B, x, y], M[k:k + B, x, y])
            out[b][s] = Block(ia[x], ib[y], delta, budget)
            worst = max(worst, float(budget.max()))
    return Result(out, starts, B, worst)


def pair_counts(want):
    return np.array([[len(blk.i) for blk in row] for row in want.blocks], dtype=np.int64).reshape(len(want.starts), -1)


def hist(want, ddelta, nbins):
    """[nb][n_sets][nbins] by the documented rule min((int)(delta / ddelta), nbins - 1)"""
    out = np.zeros((len(want.starts), len(want.blocks[0]) if want.blocks else 0, nbins), dtype=np.uint64)
    for b, row in enumerate(want.blocks):
        for s, blk in enumerate(row):
            k = np.minimum((blk.delta / ddelta).astype(np.int64), nbins - 1)
            np.add.at(out[b, s], k, np.uint64(1))
    return out


def near_edge(want, ddelta, nbins):
    """pairs whose delta lies within its budget of one of the edges k ddelta, k = 1 .. nbins - 1"""
    n = 0
    for row in want.blocks:
        for blk in row:
            if len(blk.delta) == 0:
                continue
            k = np.rint(blk.delta / ddelta)
            n += int(((np.abs(blk.delta - k * ddelta) <= blk.budget + 2.0 * EPS * blk.delta) & (k >= 1) & (k <= nbins - 1)).sum())
    return n


def check(got, scale, want):
    """the library's ``sums [nb][n_sets][2]`` (int64) and ``scale_log2`` against a ``Result``: the pair counts exactly, the
    fixed-point sums within the budget; returns the largest |difference| / budget seen"""
    got = np.asarray(got, dtype=np.int64)
    n = pair_counts(want)
    assert got.shape == n.shape + (2,), (got.shape, n.shape)
    assert np.array_equal(got[:, :, 0], n), (got[:, :, 0].tolist(), n.tolist())
    worst = 0.0
    for b, row in enumerate(want.blocks):
        for s, blk in enumerate(row):
            q = 2.0 ** -int(scale[s])
            m = len(blk.delta)
            total = float(np.sum(blk.delta.astype(np.longdouble)))
            budget = float(blk.budget.sum()) + m * 0.5 * q + 0.5 * m * m * EPS * math.sqrt(want.B)
            diff = abs(float(got[b, s, 1]) * q - total)
            assert diff <= budget, (b, s, diff, budget)
            if budget > 0:
                worst = max(worst, diff / budget)
    return worst


def per_atom(want, n_atoms, centres_of=None):
    """(n [nb][n_sets][N] int64, sum of delta [nb][n_sets][N], budget) per centre atom"""
    nb, ns = len(want.starts), len(want.blocks[0])
    n = np.zeros((nb, ns, n_atoms), dtype=np.int64)
    tot = np.zeros((nb, ns, n_atoms))
    bud = np.zeros((nb, ns, n_atoms))
    for b, row in enumerate(want.blocks):
        for s, blk in enumerate(row):
            np.add.at(n[b, s], blk.i, 1)
            np.add.at(tot[b, s], blk.i, blk.delta)
            np.add.at(bud[b, s], blk.i, blk.budget)
    return n, tot, bud
