"""The inputs of tests/test_gpu_bond_order.py, importable without a GPU: tests/test_bond_order_host.py runs the restatement
(tests/bond_order_ref.py) on every one that is held against it and asserts the cap on the per-term error budget.  The
walks are those of tests/test_gpu_bond.py's builder; every case is small (a few frames, a few hundred atoms at most)."""

import functools

import numpy as np

from amof_amd.frames import PackedTrajectory
from tests import bond_order_ref as ref
from tests import cell_forms
from tests import helpers as H
from tests import test_gpu_bond as B

DIAG, SHEARED = B.DIAG, B.SHEARED
L = (4, 6)
NBINS, NBINS_TET = 37, 53           # (odd, unequal: a swapped or mis-strided histogram shows)
FOUR_SETS = [(30, 7, 3.4), (7, 30, 3.4), (6, 6, 2.9), (1, 30, 3.0), (30, 30, 0.0), (30, 7, 3.4)]    # a zero cutoff; Zn-N twice
ZIF_SETS = [(30, 7, 2.5), (7, 30, 2.5)]
ZIF_CUT = {'Zn-N': 2.5, 'N-Zn': 2.5}
CLASS_CUT = {'Zn-N': 2.5, 'C-N': 1.6, 'Zn-Au': 3.0, 'Au-Zn': 3.0}
CLUSTER_COUNTS = (17, 40, 64, 3)

Case = type("Case", (), {})


def _case(packed, sets, l=L):
    c = Case()
    c.packed, c.sets, c.l = packed, sets, tuple(l)
    return c


def _npt(base, seed_cells, F=6):
    rng = np.random.default_rng(seed_cells)
    cells = np.stack([base * (1.0 + 0.01 * rng.normal()) for _ in range(F)])
    return B._walk(cells, B._numbers4(97), F, 15)


def zif4_rattled(F=5, sigma=0.05, seed=7):
    """the ZIF-4 fixture, every frame the crystal with independent Gaussian displacements of ``sigma`` per axis"""
    base = H.zif4_frame()
    rng = np.random.default_rng(seed)
    pos = base.positions[None] + rng.normal(scale=sigma, size=(F,) + base.positions.shape)
    return PackedTrajectory(pos, base.cell, base.numbers, pbc=base.pbc)


def lattice(kind, reps=3, F=2):
    """(packed, rc, neighbours, ideal shell vectors): a perfect one-species lattice, reps^3 conventional cells; rc midway
    between the first and the second shell"""
    if kind == "sc":
        a, basis, n = 3.0, [(0, 0, 0)], 6
        r1, r2 = a, a * np.sqrt(2.0)
        shell = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    elif kind == "fcc":
        a, basis, n = 4.0, [(0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0)], 12
        r1, r2 = a / np.sqrt(2.0), a
        shell = [s for s in [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)] if sum(abs(x) for x in s) == 2]
    elif kind == "diamond":
        a, n = 5.0, 4
        fcc = [(0, 0, 0), (0, .5, .5), (.5, 0, .5), (.5, .5, 0)]
        basis = fcc + [(x + .25, y + .25, z + .25) for x, y, z in fcc]
        r1, r2 = a * np.sqrt(3.0) / 4.0, a / np.sqrt(2.0)
        shell = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
    else:
        raise KeyError(kind)
    cellsites = np.array([(i, j, k) for i in range(reps) for j in range(reps) for k in range(reps)], dtype=np.float64)
    frac = (cellsites[:, None, :] + np.asarray(basis, dtype=np.float64)[None, :, :]).reshape(-1, 3)
    pos = np.repeat((frac * a)[None], F, axis=0)
    packed = PackedTrajectory(pos, np.diag([a * reps] * 3), np.full(len(frac), 30))
    return packed, 0.5 * (r1 + r2), n, np.asarray(shell, dtype=np.float64)


def cluster(counts=CLUSTER_COUNTS, seed=5, radius=2.0):
    """one frame: a Zn per entry of ``counts`` with that many N on a shell of ``radius`` +- 10 % around it (no two N of a
    shell closer than 0.2 A), the clusters 10 A apart in a 40 A box"""
    rng = np.random.default_rng(seed)
    pos, numbers = [], []
    for k, m in enumerate(counts):
        centre = np.array([5.0 + 10.0 * (k % 3), 5.0 + 10.0 * (k // 3), 20.0])
        pos.append(centre)
        numbers.append(30)
        pts = []
        while len(pts) < m:
            v = rng.normal(size=3)
            p = centre + v / np.sqrt(v @ v) * radius * rng.uniform(0.9, 1.1)
            if all(np.sqrt(((p - q) ** 2).sum()) > 0.2 for q in pts):
                pts.append(p)
        pos.extend(pts)
        numbers.extend([7] * m)
    return PackedTrajectory(np.asarray(pos)[None], np.diag([40.0, 40.0, 40.0]), np.asarray(numbers))


@functools.lru_cache(maxsize=None)
def case(name):
    """the case ``name``; "name@form" is the same case built in the cell cell_forms.apply(cell, form)"""
    name, _, form = name.partition("@")
    if form:
        assert name in ("rect", "four", "sheared", "npt_diag", "npt_sheared"), name
    return _build(name, cell_forms.apply(B.DIAG, form or None), cell_forms.apply(B.SHEARED, form or None))


def _build(name, DIAG, SHEARED):
    if name == "rect":
        # N = 150 and F = 7: neither a multiple of 64; the cutoff gives 0 .. 12 and more neighbours, 4 among them
        return _case(B._walk(DIAG, np.full(150, 30), 7, 13), [(30, 30, 3.9)], (3, 4, 6, 12))
    if name == "zif4":
        return _case(zif4_rattled(), ZIF_SETS)
    if name == "four":
        return _case(B._walk(DIAG, B._numbers4(203), 5, 12), FOUR_SETS)
    if name == "sheared":
        return _case(B._walk(SHEARED, B._numbers4(131), 5, 13), [(30, 7, 5.5), (6, 1, 5.0)])
    if name == "npt_diag":
        return _case(_npt(DIAG, 14), [(30, 7, 6.0), (7, 7, 5.2)])
    if name == "npt_sheared":
        return _case(_npt(SHEARED, 18), [(30, 7, 6.0), (7, 7, 5.2)])
    if name == "open":
        return _case(B._walk(DIAG, B._numbers4(120), 5, 16, pbc=(True, False, True)), [(30, 7, 6.0), (1, 6, 5.2)])
    if name == "cluster":
        return _case(cluster(), [(30, 7, 3.0)], (4, 6, 12))
    if name == "class":
        return _case(zif4_rattled(F=6, seed=9), [(30, 7, 2.5), (6, 7, 1.6)])
    raise KeyError(name)


NAMES = ["rect", "zif4", "four", "sheared", "npt_diag", "npt_sheared", "open", "cluster", "class"]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's ``Result`` of a case, computed once per process and left unchanged"""
    c = case(name)
    p = c.packed
    return ref.order(p.pos, p.cell, p.numbers, c.sets, c.l, pbc=tuple(p.pbc))


def coincident():
    """the "four" walk with an N put onto a Zn in frame 1: a bonded pair of coincident atoms"""
    p = case("four").packed
    pos = np.array(p.pos, copy=True)
    zn = int(np.nonzero(p.numbers == 30)[0][0])
    n = int(np.nonzero(p.numbers == 7)[0][0])
    pos[1, n] = pos[1, zn]
    return PackedTrajectory(pos, p.cell, p.numbers, pbc=p.pbc)
