"""CPU side of the guard-band tests (tests/edge_plant.py, tests/test_gpu_guard_band.py): the generator's band against
the host's own arithmetic (guard_math.h through tests/native/guard_math_driver.cpp), the generator's self-checks, and
the C oracle -- the yardstick of the GPU tests -- against an independent numpy float64 restatement of DESIGN.md §2 on
the very data those tests use."""

import os
import subprocess

import numpy as np
import pytest

from oracle import clib
from tests import edge_plant as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CELLS = {
    "diagonal": np.diag([17.31, 18.93, 41.77]),
    "sheared": np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 29.53]]),
    "high_kappa": np.array([[31.7, 0.0, 0.0], [0.0, 29.3, 0.0], [83.1, 79.7, 30.9]]),
    "rotated": np.array([[12.0, 5.1, -3.3], [-4.4, 14.2, 2.9], [3.1, -1.7, 19.6]]),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gb") / "guard_math_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off",
                        os.path.join(ROOT, "tests", "native", "guard_math_driver.cpp"), "-o", out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _ask(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return [float(l.split()[0]) for l in r.stdout.strip().splitlines()]


def _fmt(a):
    return " ".join("%.17g" % v for v in np.asarray(a).ravel())


def test_python_band_equals_the_host_arithmetic(driver):
    """kappa of both error models (the RDF tile paths' over six axis orders and NPT frames; the neighbour kernels'),
    restated in numpy, equals what guard_math.h computes for the same cells"""
    rng = np.random.default_rng(3)
    cells = list(CELLS.values())
    for _ in range(12):
        q, _r = np.linalg.qr(rng.normal(size=(3, 3)))
        cells.append((np.diag(rng.uniform(8, 40, 3)) + np.tril(rng.uniform(-9, 9, (3, 3)), -1)) @ q)
    npt = np.stack([CELLS["sheared"] * (1 + 0.01 * k) + np.tril(rng.uniform(-0.5, 0.5, (3, 3)), -1) for k in range(4)])
    rdf_lines = ["R 1 " + _fmt(c) for c in cells] + ["R 4 " + _fmt(npt)]
    got = _ask(driver, rdf_lines)
    for c, k in zip(cells + [npt], got):
        assert k == pytest.approx(E.kappa_rdf(c), rel=1e-11)
    got = _ask(driver, ["P " + _fmt(c) + " " + _fmt(np.linalg.inv(c)) for c in cells])
    for c, k in zip(cells, got):
        assert k == pytest.approx(E.kappa_cell(c), rel=1e-11)
    # the composition of the bound (fast_guard_rel_rdf, fast_guard_rel + 3u, g_m, guard_abs / guard_abs16)
    u = 2.0 ** -24
    c = CELLS["sheared"]
    cs = np.linalg.norm(c, axis=1).sum()
    assert E.rdf_band(c, 6.5, 2310) == pytest.approx(2310 * 1.1 * (5 * E.kappa_rdf(c) + 3.06) * u + cs * 2.0 ** -31 / (6.5 / 2310) + 2310e-12, rel=1e-14)
    d = CELLS["diagonal"]
    assert E.rdf_band(d, 8.0, 800) == pytest.approx(800 * 1.1 * 5.06 * u + np.trace(d) * 2.0 ** -31 / 0.01 + 800e-12, rel=1e-14)
    assert E.nbr_band(d, 2.5) == pytest.approx(1.1 * 6.06 * u + 3 * u + np.trace(d) * 2.0 ** -31 / 2.5, rel=1e-14)
    assert E.nbr_band(d, 2.5, compact=True) == pytest.approx(1.1 * 6.06 * u + 3 * u + np.trace(d) * 2.0 ** -15 / 2.5, rel=1e-14)
    # the high-kappa cell's band sits close to (but below) the tile paths' limit guard_f < 0.25 at the LDS limit
    g = E.rdf_band(CELLS["high_kappa"], 4.2, 31744)
    assert 0.05 < g < 0.25, g


@pytest.mark.parametrize("kind,nbins,far", [("diagonal", 2310, True), ("sheared", 999, False), ("high_kappa", 31744, False),
                                            ("diagonal", 1, True), ("rotated", 7, True)])
def test_rdf_planting_checks_itself(kind, nbins, far):
    c = CELLS[kind]
    h = abs(np.linalg.det(c)) / np.linalg.norm(np.cross(c[[1, 2, 0]], c[[2, 0, 1]]), axis=1)
    rmax = 0.45 * h.min()
    pl = E.plant_rdf(c, [8] * 700 + [30] * 300 + [1], rmax, nbins, seed=nbins, F=2, far=far)
    t = pl.band_units()
    assert np.all(np.abs(t) <= 10.0 + 1e-6)
    assert pl.packed.pos.shape == (2, 1001, 3)
    if far:
        frac = np.abs(np.linalg.solve(c.T, pl.packed.pos.reshape(-1, 3).T))
        assert 5000 < frac.max() < 1e4
    # a planting whose pairs sit far from every decision is refused by the same check
    pl.D = pl.D + 100.0 * pl.g_abs
    with pytest.raises(AssertionError):
        pl.check()


def test_nbr_planting_checks_itself():
    c = CELLS["sheared"]
    numbers = [30] * 300 + [7] * 500 + [6] * 400 + [1] * 200 + [8]
    kinds = sorted(set(numbers))
    S = len(kinds)
    rcm = np.zeros((S, S))
    zn, n, ch, h = (kinds.index(z) for z in (30, 7, 6, 1))
    rcm[zn, n] = rcm[n, zn] = 2.5
    rcm[ch, h] = rcm[h, ch] = 1.31
    rcm[n, n] = 2.2
    edges = np.sort(np.concatenate([[0.0, 180.0], np.random.default_rng(1).uniform(0, 180, 40)]))
    for compact in (False, True):
        pl = E.plant_nbr(c, numbers, rcm, seed=5, F=3, far=True, compact=compact, triples=[(zn, n), (n, n)], angle_edges=edges)
        sp = pl.species
        assert np.all(rcm[sp[pl.i], sp[pl.j]] > 0)
        pairs = set(zip(sp[pl.i].tolist(), sp[pl.j].tolist()))
        assert {(zn, n), (n, zn), (ch, h), (h, ch), (n, n)} <= pairs          # every cutoff, both species orders
        assert len(pl.angles) >= 50
    assert E.nbr_band(c, 2.5, compact=True) > 100 * E.nbr_band(c, 2.5)


# ------------------------------------------------------------- the oracle against a numpy restatement of §2 --

def _pairs_of_frame(pos, C, rows):
    """canonical pair vectors r_j - r_i of the centres `rows` against every atom (rint image, no fma), squared lengths"""
    inv = np.linalg.inv(C)
    d0 = pos[None, :, :] - pos[rows, None, :]
    s = d0 @ inv
    d = d0 - np.rint(s) @ C
    return (d * d).sum(axis=2)


def _np_rdf(pos, cells, sp, S, rmax, nbins):
    """ordered-pair histogram and the pairs within 1e-9 bins of an edge (edge index, species pair)"""
    F, N = pos.shape[:2]
    dr = rmax / nbins
    hist = np.zeros(S * S * nbins, dtype=np.int64)
    amb = []
    for f in range(F):
        C = cells[f if len(cells) > 1 else 0]
        for r0 in range(0, N, 256):
            rows = np.arange(r0, min(N, r0 + 256))
            d2 = _pairs_of_frame(pos[f], C, rows)
            d2[np.arange(len(rows)), rows] = 1e300                     # no self pair
            q = np.sqrt(np.minimum(d2, 4.0 * rmax * rmax)) / dr
            b = np.floor(q).astype(np.int64)
            live = (d2 < rmax * rmax) & (b < nbins)
            key = (sp[rows][:, None] * S + sp[None, :]) * nbins + b
            hist += np.bincount(key[live], minlength=S * S * nbins)
            e = np.rint(q)
            near = (np.abs(q - e) < 1e-9) & (e >= 1) & (e <= nbins) & (d2 < 4.0 * rmax * rmax)
            ii, jj = np.nonzero(near)
            amb += [(int(sp[rows[x]]), int(sp[y]), int(e[x, y])) for x, y in zip(ii, jj)]
    return hist.reshape(S, S, nbins), amb


def _agree_but_at_edges(got, ref, amb, nbins):
    diff = got.astype(np.int64) - ref.astype(np.int64)
    allowed = np.zeros(diff.shape, bool)
    for a, b, e in amb:
        allowed[a, b, e - 1] = True
        if e < nbins:
            allowed[a, b, e] = True
    assert not np.any(diff[~allowed]), np.argwhere(diff & ~allowed)[:10]
    assert np.abs(diff).sum() <= 2 * len(amb), (int(np.abs(diff).sum()), len(amb))


@pytest.mark.parametrize("kind,nbins", [("diagonal", 2310), ("sheared", 7), ("rotated", 999), ("npt", 31744)])
def test_oracle_rdf_equals_a_numpy_restatement_on_planted_pairs(kind, nbins):
    if kind == "npt":
        c = np.stack([CELLS["sheared"] * (1.0 + 0.013 * k) for k in range(3)])
    else:
        c = CELLS[kind][None]
    h = min(abs(np.linalg.det(x)) / np.linalg.norm(np.cross(x[[1, 2, 0]], x[[2, 0, 1]]), axis=1).max() for x in c)
    rmax = 0.49 * h                                               # no further images: the rint image is the only one
    numbers = [1] * 400 + [6] * 330 + [30] * 70 + [7]
    pl = E.plant_rdf(c, numbers, rmax, nbins, seed=11 + nbins, F=None if kind == "npt" else 2, far=True)
    kinds, sp = E._species(numbers)
    ref, _ = clib.rdf_hist(pl.packed.pos, pl.packed.cell, sp, len(kinds), rmax, nbins)
    mine, amb = _np_rdf(pl.packed.pos, pl.packed.cell, sp, len(kinds), rmax, nbins)
    assert len(amb) > 0                 # the exact hits are where the two may differ; their count bounds the difference
    _agree_but_at_edges(mine, ref, amb, nbins)
    assert ref.sum() > 0 and abs(int(ref.sum()) - int(mine.sum())) <= len(amb)


@pytest.mark.parametrize("kind", ["diagonal", "sheared"])
def test_oracle_cn_equals_a_numpy_restatement_on_planted_pairs(kind):
    c = CELLS[kind]
    numbers = [30] * 150 + [7] * 350 + [6] * 300 + [1] * 300 + [8]
    kinds, sp = E._species(numbers)
    S = len(kinds)
    zn, n, ch, h = (kinds.index(z) for z in (30, 7, 6, 1))
    rcm = np.zeros((S, S))
    rcm[zn, n] = rcm[n, zn] = 2.5
    rcm[ch, h] = rcm[h, ch] = 1.31
    rcm[n, n] = 2.2
    pl = E.plant_nbr(c, numbers, rcm, seed=17, F=2, far=True)
    sets = [(zn, n), (n, zn), (ch, h), (h, ch), (n, n), (h, h)]
    sums, pa = clib.cn_counts(pl.packed.pos, pl.packed.cell, sp, S, rcm, sets, per_atom=True)
    pos = pl.packed.pos
    N = pos.shape[1]
    n_amb = 0
    for f in range(pos.shape[0]):
        d2 = _pairs_of_frame(pos[f], c, np.arange(N))
        np.fill_diagonal(d2, np.inf)
        r = np.sqrt(d2)
        for k, (A, B) in enumerate(sets):
            rc = rcm[A, B]
            ca, cb = np.nonzero(sp == A)[0], np.nonzero(sp == B)[0]
            sub = r[np.ix_(ca, cb)]
            mine = (sub < rc).sum(axis=1)
            amb = (np.abs(sub / rc - 1.0) < 1e-12).sum(axis=1) if rc > 0 else np.zeros(len(ca), int)
            n_amb += int(amb.sum())
            assert np.all(np.abs(pa[f, k, ca] - mine) <= amb), (f, (A, B))
            assert np.all(pa[f, k, np.nonzero(sp != A)[0]] == -1)
            assert abs(int(sums[f, k]) - int(mine.sum())) <= int(amb.sum())
    assert sums.sum() > 0 and n_amb > 0
