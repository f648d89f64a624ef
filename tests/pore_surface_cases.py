"""The inputs of tests/test_gpu_pore_surface.py, importable without a GPU: tests/test_pore_surface_host.py runs the restatement
(tests/pore_surface_ref.py) on every one and asserts the cap on its budget and that no sample is a near decision.  The
trajectories, grids and radii are those of tests/pore_cases.py; every case takes the probe radii (0, 1.2, 2) and 64 directions
-- "rect" 100 (a ragged last round of 64 lanes), "rect#1" one direction."""

import functools

import numpy as np

from amof_amd import pore as P
from amof_amd.frames import PackedTrajectory
from tests import pore_cases
from tests import pore_surface_ref as sref

THRESHOLDS = (0.0, 1.2, 2.0)
NAMES = ["rect", "zif4", "sheared", "npt_sheared", "open", "rect#1"]
FORMS = [n for n in pore_cases.FORMS if not n.startswith("planted")]
POINTS = {"rect": 100, "rect#1": 1}

Case = type("Case", (), {})


@functools.lru_cache(maxsize=None)
def case(name):
    base = pore_cases.case(name.partition("#")[0])
    c = Case()
    c.packed, c.grid, c.dr, c.dmax, c.radii, c.kinds, c.G = base.packed, base.grid, base.dr, base.dmax, base.radii, base.kinds, base.G
    c.thresholds = THRESHOLDS
    c.dirs = P.sphere_points(POINTS.get(name, 64))
    c.dirs.setflags(write=False)
    c.species = np.array([base.kinds.index(int(z)) for z in base.packed.numbers])
    return c


def _cell(packed, f):
    cells = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3)
    return cells[0 if len(cells) == 1 else f]


@functools.lru_cache(maxsize=None)
def reference(name):
    """``[F][n_t]`` of ``pore_surface_ref.Frame``, computed once per process and left unchanged"""
    c = case(name)
    p = c.packed
    radius = c.radii[c.species]
    out = []
    for f in range(p.pos.shape[0]):
        row = [sref.frame(p.pos[f], _cell(p, f), radius, rp, c.dirs, tuple(p.pbc)) for rp in c.thresholds]
        for fr in row:
            for a in (fr.exposed, fr.near, fr.samples):
                a.setflags(write=False)
        out.append(row)
    return out


def bytes_of(name):
    """uint8 [F][n_t][N][M]: 1 where the restatement has the sample exposed"""
    return np.array([[fr.exposed for fr in row] for row in reference(name)], dtype=np.uint8)


# ---- planted decisions ---------------------------------------------------------------------------------------------------
PLANT_M, PLANT_SAMPLE = 64, 24
PLANT_THR = (0.0, 1.2)
PLANT_HOME = np.array([4.1, 3.9, 4.2])
PLANT_REST = np.array([[12.0, 4.0, 2.0], [12.0, 12.0, 6.0], [4.0, 12.0, 2.0]])


def plant_deltas():
    """(2^-26 A, eps / 4): eps the bound the pore_surface_list path uses for the planted case"""
    from amof_amd import _hip
    return pore_cases.DELTA_SMALL, 0.25 * _hip.pore_surface_bound(pore_cases.PLANT_CELL, pore_cases.TABLE[30] + max(PLANT_THR))


def planted():
    """Eight frames of five Zn in pore_cases.PLANT_CELL.  Atom 0 sits at PLANT_HOME; atom 1 is placed so that sample PLANT_SAMPLE of
    atom 0 at the frame's probe radius rp lies at R + rp + s delta from it, in a direction 0.3 rad off the sample's own; atoms
    2 .. 4 are far from both.  ``plants``: [(frame, threshold index, s delta)] -- s > 0: that sample is exposed, s < 0: buried."""
    dirs = P.sphere_points(PLANT_M)
    R = pore_cases.TABLE[30]
    u = dirs[PLANT_SAMPLE]
    perp = np.cross(u, [0.0, 0.0, 1.0])
    perp /= np.sqrt(perp @ perp)
    w = np.cos(0.3) * u + np.sin(0.3) * perp
    w /= np.sqrt(w @ w)
    frames, plants = [], []
    for delta in plant_deltas():
        for sign in (1.0, -1.0):
            for k, rp in enumerate(PLANT_THR):
                s = PLANT_HOME + (R + np.float64(rp)) * u           # (the documented sample, bit for bit)
                frames.append(np.vstack([PLANT_HOME, s + w * (R + rp + sign * delta), PLANT_REST]))
                plants.append((len(frames) - 1, k, sign * delta))
    return PackedTrajectory(np.array(frames), pore_cases.PLANT_CELL, np.full(5, 30)), dirs, tuple(plants)


# ---- known answers --------------------------------------------------------------------------------------------------------
CUBE = np.diag([20.0, 20.0, 20.0])
CUBE_GRID, CUBE_DR, CUBE_DMAX = (10, 10, 10), 0.5, 4.0
PAIR_D, PAIR_RP, PAIR_M = 2.0, 1.2, 256


def one_atom():
    return PackedTrajectory(np.array([[[7.3, 8.1, 9.4]]]), CUBE, np.array([30]))


def two_atoms():
    """two Zn on the z axis PAIR_D apart, the lower one first"""
    return PackedTrajectory(np.array([[[9.0, 9.5, 8.0], [9.0, 9.5, 8.0 + PAIR_D]]]), CUBE, np.array([30, 30]))
