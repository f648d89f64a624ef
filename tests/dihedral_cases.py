"""The inputs of the dihedral tests (tests/test_dihedral_host.py, tests/test_dihedral_native_cpu.py, tests/test_gpu_dihedral.py),
importable without a GPU: at most 8 frames and 400 atoms each (``test_dihedral_host`` holds every case to that).  Every case: a
PackedTrajectory, the cutoff dictionary, the chain patterns (strings) and dphi; ``reference(name)`` is tests/dihedral_ref.py on
it, computed once and never changed."""

import functools

import numpy as np

from amof_amd import dihedral as amdihedral
from amof_amd import atom as amatom
from amof_amd.frames import PackedTrajectory
from tests import cell_forms
from tests import dihedral_ref as ref
from tests import helpers as H

ZIF_CUT = {'Zn-N': 2.5, 'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}
SHEAR = np.array([[1.0, 0.0, 0.0], [0.12, 1.0, 0.0], [-0.07, 0.09, 1.0]])
FINE_CHAINS = ['H-C-H-C', 'H-C-C-H', 'H-C-C-C', 'H-C-C-N', 'H-C-N-C', 'H-C-N-Zn', 'C-C-N-C', 'C-C-N-Zn', 'C-N-C-N', 'C-N-Zn-N',
               'N-C-C-N', 'N-C-N-Zn', 'X-X-X-X', 'X-C-N-X', 'X-N-Zn-X', 'X-C-C-X', 'H-X-X-X', 'C-X-X-X', 'N-X-X-X', 'Zn-X-X-X',
               'H-C-X-X', 'X-N-C-X', 'Zn-N-X-X', 'X-X-N-Zn']
PLANTED = (35.0, 100.0, 165.0)
PLANTED_DPHI = 6.0              # 35, 100 and 165 lie inside bins 5, 16 and 27
PLANTED_BIN = {35.0: 5, 100.0: 16, 165.0: 27}

Case = type("Case", (), {})


def _case(packed, cutoff, chains, dphi):
    c = Case()
    c.packed, c.cutoff, c.chains, c.dphi = packed, cutoff, chains, dphi
    return c


def cubic(colour=False, L=4, a=2.0, F=2):
    """L^3 sites of a simple cubic lattice; ``colour``: rock salt (Zn where i + j + k is even, N elsewhere)"""
    sites = np.array([(i, j, k) for i in range(L) for j in range(L) for k in range(L)])
    numbers = np.where(sites.sum(axis=1) % 2 == 0, 30, 7) if colour else np.full(len(sites), 30)
    pos = np.repeat((sites * a).astype(np.float64)[None], F, axis=0)
    return PackedTrajectory(pos, np.diag([a * L] * 3), numbers)


def planted(phi, form=None, box=30.0):
    """one chain H-C-N-Zn of dihedral ``phi`` degrees with bond angles of 110 and 105 degrees, its central bond across the
    periodic face x = box; the cell in one of the forms of tests/cell_forms.py"""
    t1, t2, p = np.radians(110.0), np.radians(105.0), np.radians(phi)
    b = np.array([box - 0.5, 15.0, 14.0])
    c = b + np.array([1.45, 0.0, 0.0])
    a = b + 1.1 * np.array([np.cos(t1), np.sin(t1), 0.0])
    d = c + 1.9 * np.array([-np.cos(t2), np.sin(t2) * np.cos(p), np.sin(t2) * np.sin(p)])
    pos = np.stack([a, b, c, d])
    base = np.diag([box] * 3)
    cell = base if form is None else cell_forms.check(base, form)
    if form in ("rot", "mirror", "rotmirror"):
        pos = pos @ np.linalg.solve(base, cell)     # (the same rigid motion as the cell's)
    pos = pos - np.floor(pos @ np.linalg.inv(cell)) @ cell      # wrapped: c and d now lie across the face
    return PackedTrajectory(pos[None], cell, np.array([1, 6, 7, 30]))


PLANTED_CUT = {'C-H': 1.3, 'C-N': 1.7, 'Zn-N': 2.2}
PLANTED_CHAINS = ['H-C-N-Zn', 'Zn-N-C-H', 'X-C-N-X', 'X-X-X-X', 'H-C-C-H']


def zif4_frames(cell=None):
    """the crystal and two Gaussian rattles of it (sigma = 0.05 and 0.15 A, default_rng(7))"""
    base = H.zif4_frame()
    rng = np.random.default_rng(7)
    pos = np.stack([base.positions, base.positions + rng.normal(0.0, 0.05, base.positions.shape),
                    base.positions + rng.normal(0.0, 0.15, base.positions.shape)])
    return PackedTrajectory(pos, base.cell if cell is None else cell, base.numbers, pbc=base.pbc)


def zif4_sheared():
    """the same three frames sheared, cell and positions alike (r -> r M): a triclinic cell, bond lengths moved by a few
    percent, the kernels in their general-cell forms"""
    p = zif4_frames()
    return PackedTrajectory(p.pos_host() @ SHEAR, np.asarray(p.cell[0], dtype=np.float64) @ SHEAR, p.numbers, pbc=p.pbc)


def triangle():
    """a three-membered ring of carbon atoms with a tail of two: the chains that would return to their first atom are dropped"""
    pos = np.array([[10.0, 10.0, 10.0], [11.5, 10.0, 10.0], [10.75, 10.0 + 1.5 * np.sqrt(3.0) / 2.0, 10.0],
                    [10.75, 12.2, 11.1], [11.9, 12.9, 11.6]])
    return PackedTrajectory(pos[None], np.diag([20.0, 21.0, 22.0]), np.full(5, 6))


def crowded(n=17):
    """a Zn with ``n`` N neighbours on a sphere of 2 A (no N-N cutoff), each N with one H: 17 exceeds the capacity"""
    k = np.arange(n) + 0.5
    polar, azimuth = np.arccos(1.0 - 2.0 * k / n), np.pi * (1.0 + 5.0 ** 0.5) * k
    dirs = np.stack([np.cos(azimuth) * np.sin(polar), np.sin(azimuth) * np.sin(polar), np.cos(polar)], axis=1)
    centre = np.array([12.0, 12.5, 13.0])
    pos = np.concatenate([centre[None], centre + 2.0 * dirs, centre + 3.0 * dirs])
    return PackedTrajectory(pos[None], np.diag([24.0, 25.0, 26.0]), np.array([30] + [7] * n + [1] * n))


CROWDED_CUT = {'Zn-N': 2.5, 'H-N': 1.2}


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "cubic":
        return _case(cubic(), {'Zn-Zn': 2.4}, ['X-X-X-X'], 7.0)
    if name == "rocksalt":
        return _case(cubic(colour=True), {'Zn-N': 2.4}, ['Zn-N-Zn-N', 'N-Zn-N-Zn', 'Zn-Zn-X-X'], 7.0)
    if name.startswith("planted"):
        parts = name.split("_")         # planted_<phi>[_<form>]
        return _case(planted(float(parts[1]), parts[2] if len(parts) > 2 else None), PLANTED_CUT, PLANTED_CHAINS, PLANTED_DPHI)
    if name == "zif4":
        return _case(zif4_frames(), ZIF_CUT, None, 1.0)
    if name == "zif4_explicit":     # three explicit patterns: no pattern uses the C-C bonds, which stay in the graph
        return _case(zif4_frames(), ZIF_CUT, ['C-N-Zn-N', 'C-N-C-N', 'H-C-N-Zn'], 1.0)
    if name == "zif4_fine":         # 24 patterns x 1801 bins: more words than a workgroup's LDS histogram holds
        return _case(zif4_frames(), ZIF_CUT, FINE_CHAINS, 0.1)
    if name == "zif4_sheared":
        return _case(zif4_sheared(), ZIF_CUT, None, 1.0)
    if name == "triangle":
        return _case(triangle(), {'C-C': 1.7}, ['C-C-C-C', 'X-C-C-X'], 5.0)
    if name == "crowded16":
        return _case(crowded(16), CROWDED_CUT, ['X-X-X-X', 'H-N-Zn-N'], 1.0)
    raise KeyError(name)


PLANTED_NAMES = tuple("planted_%d" % p for p in PLANTED) + tuple("planted_%d_%s" % (p, f) for p in PLANTED for f in cell_forms.FORMS)
NAMES = ("cubic", "rocksalt", "zif4", "zif4_explicit", "zif4_fine", "zif4_sheared", "triangle", "crowded16") + PLANTED_NAMES


def patterns(c):
    """``(names, [T][4] atomic numbers)`` of a case: its chains, or the class's default ones"""
    if c.chains is None:
        numbers = amdihedral.default_chains(amatom.format_cutoff(c.cutoff, sort_pair=True), sorted(set(int(z) for z in c.packed.numbers)))
    else:
        numbers = [amdihedral.parse_chain(s) for s in c.chains]
    return [amdihedral.chain_name(z) for z in numbers], numbers


def abi_arguments(c):
    """``(cutoff matrix, [T][4] species indices, edges)`` as ``Context.dihedral_hist`` takes them (every pattern of a case names
    species that are present)"""
    kinds = sorted(set(int(z) for z in c.packed.numbers))
    rcm = amatom.cutoff_matrix(amatom.format_cutoff(c.cutoff, sort_pair=True), kinds)
    idx = [[-1 if z < 0 else kinds.index(z) for z in p] for p in patterns(c)[1]]
    return rcm, idx, amdihedral.bins(c.dphi)[0]


@functools.lru_cache(maxsize=None)
def reference(name):
    """``[dihedral_ref.Frame]`` of a case; computed once, never changed"""
    c = case(name)
    frames = ref.trajectory(c.packed, c.cutoff, patterns(c)[1], amdihedral.bins(c.dphi)[0])
    for fr in frames:
        for x in (fr.hist, fr.n, fr.undefined, fr.cos):
            x.setflags(write=False)
    return frames
