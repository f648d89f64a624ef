"""The inputs of the ring tests (tests/test_ring_host.py, tests/test_ring_native_cpu.py, tests/test_gpu_ring.py), importable
without a GPU.  Every case: a PackedTrajectory, the cutoff dictionary, the search depth, which reference it is held against
and, where there is one, the known answer -- which the tests recompute with tests/ring_ref.py."""

import functools

import numpy as np

from amof_amd.frames import PackedTrajectory
from tests import helpers as H
from tests import ring_ref as ref

ZIF_CUT = {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
POLYGONS = (3, 4, 5, 8, 9, 12, 13)
TRICLINIC = np.array([[17.0, 0.0, 0.0], [2.5, 16.0, 0.0], [-1.5, 3.0, 15.0]])

Case = type("Case", (), {})


def _case(packed, cutoff, nmax, against, known=None, truncated=None):
    c = Case()
    c.packed, c.cutoff, c.nmax, c.against, c.known, c.truncated = packed, cutoff, nmax, against, known, truncated
    return c


def polygon(n, bond=1.5, box=40.0):
    """a planar regular n-gon of carbon atoms with bond length ``bond`` in the middle of a cubic box"""
    radius = bond / (2.0 * np.sin(np.pi / n))
    t = 2.0 * np.pi * np.arange(n) / n
    pos = np.stack([box / 2 + radius * np.cos(t), box / 2 + radius * np.sin(t), np.full(n, box / 2)], axis=1)
    return PackedTrajectory(pos[None], np.diag([box] * 3), np.full(n, 6))


def simple_cubic(L, a=3.0):
    sites = np.array([(i, j, k) for i in range(L) for j in range(L) for k in range(L)], dtype=np.float64)
    return PackedTrajectory((sites * a)[None], np.diag([a * L] * 3), np.full(len(sites), 30))


def graphene(nx=4, ny=6, d=1.42):
    """nx x ny rectangular cells of four atoms (armchair along x)"""
    ax, ay = 3.0 * d, np.sqrt(3.0) * d
    basis = np.array([(0.0, 0.0), (d, 0.0), (1.5 * d, 0.5 * ay), (2.5 * d, 0.5 * ay)])
    pos = np.array([(bx + i * ax, by + j * ay, 10.0) for i in range(nx) for j in range(ny) for bx, by in basis])
    return PackedTrajectory(pos[None], np.diag([nx * ax, ny * ay, 20.0]), np.full(len(pos), 6))


def random_network(cell, seed, N=150, F=3, mean_degree=3.0):
    """two species in ``cell``; one cutoff per species pair, set so that the frame's mean degree is about ``mean_degree`` and no
    pair lies within 1e-4 A of its cutoff (ring_ref.adjacency asserts 1e-6)"""
    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=np.float64)
    numbers = np.where(rng.uniform(size=N) < 0.4, 30, 7)
    pos = rng.uniform(0, 1, size=(F, N, 3)) @ cell
    volume = abs(np.linalg.det(cell))
    rc = (mean_degree * volume / N / (4.0 / 3.0 * np.pi)) ** (1.0 / 3.0)
    cutoff = {'Zn-N': round(1.05 * rc, 3), 'N-N': round(0.95 * rc, 3), 'Zn-Zn': round(1.0 * rc, 3)}
    packed = PackedTrajectory(pos, cell, numbers)
    return packed, cutoff


def zif4(reps=(1, 1, 1), F=1, sigma=0.0, seed=3):
    base = H.zif4_frame()
    if tuple(reps) != (1, 1, 1):
        base = H.replicate(base, reps)
    if F == 1 and sigma == 0.0:
        return PackedTrajectory(base.positions[None], base.cell, base.numbers, pbc=base.pbc)
    return H.random_walk(base, F, sigma, seed)


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("polygon"):
        n = int(name[7:])
        return _case(polygon(n), {'C-C': 1.6}, 12, "brute", {n: 1} if n <= 12 else {}, 0)
    if name == "sc7":
        return _case(simple_cubic(7), {'Zn-Zn': 3.3}, 6, "brute", {4: 1029, 6: 1372})
    if name == "sc5":
        return _case(simple_cubic(5), {'Zn-Zn': 3.3}, 6, "brute", {4: 375, 5: 75, 6: 500})
    if name == "graphene":
        return _case(graphene(), {'C-C': 1.6}, 10, "brute", {6: 48})
    if name == "zif4_16":
        return _case(zif4(), ZIF_CUT, 16, "brute", {5: 32, 16: 24})
    if name == "zif4_32":
        return _case(zif4(), ZIF_CUT, 32, "search", {5: 32, 16: 24, 24: 32, 32: 24})
    if name == "random_rect":
        packed, cut = random_network(np.diag([16.0, 17.5, 15.0]), 11)
        return _case(packed, cut, 8, "brute")
    if name == "random_tri":
        packed, cut = random_network(TRICLINIC, 12)
        return _case(packed, cut, 8, "brute")
    raise KeyError(name)


NAMES = tuple("polygon%d" % n for n in POLYGONS) + ("sc7", "sc5", "graphene", "zif4_16", "zif4_32", "random_rect", "random_tri")


@functools.lru_cache(maxsize=None)
def graphs(name):
    """the float64 bond graph of every frame of a case"""
    c = case(name)
    p = c.packed
    return [ref.adjacency(p.pos[f], p.cell[0 if p.cell.shape[0] == 1 else f], p.numbers, c.cutoff, tuple(p.pbc))
            for f in range(p.pos.shape[0])]


@functools.lru_cache(maxsize=None)
def reference(name):
    """per frame ``(c [N][nmax + 1], truncated)`` by ring_ref.search (tests/test_ring_host.py holds it against the brute force on
    the cases that name it); computed once, never changed"""
    c = case(name)
    out = []
    for adj in graphs(name):
        got, truncated, _ = ref.search(adj, c.nmax)
        got.setflags(write=False)
        out.append((got, truncated))
    return out
