"""The inputs of tests/test_gpu_reorientation.py, importable without a GPU: tests/test_reorientation_host.py runs the
restatement (tests/reorientation_ref.py) on every one of them and asserts the cap on the per-term error budget.  The
trajectories are those of tests/test_gpu_bond.py (its builders, its seeds where they keep every bonded pair apart)."""

import functools

import numpy as np

from tests import cell_forms
from tests import helpers as H
from tests import reorientation_ref as ref
from tests import test_gpu_bond as B

DIAG, SHEARED = B.DIAG, B.SHEARED
RECT_LAGS = [0, 1, 2, 5, 63, 64, 65, 100, 129]
FOUR_SETS = [(30, 7, 3.4), (7, 30, 3.4), (6, 6, 2.9), (1, 30, 3.0), (30, 30, 0.0)]     # (a zero cutoff: never neighbours)
FOUR_LAGS = [0, 3, 7, 7, 1, 40, 68, 69]
PLANT_SETS = [(30, 7, 3.4), (7, 30, 3.4), (7, 7, 3.1), (30, 30, 2.9)]
COMP_SETS = [(30, 7, 3.4), (6, 6, 2.9), (1, 30, 3.0)]
COMP_LAGS = [0, 1, 9, 0]
CLASS_CUT = {'Zn-N': 2.5, 'C-N': 1.6, 'Zn-Au': 3.0}
CLASS_SETS = [(30, 7, 2.5), (6, 7, 1.6)]
RANK_CUT = {'Zn-N': 2.5, 'C-N': 1.6}

Case = type("Case", (), {})


def _case(packed, sets, lags, strides=(1,)):
    c = Case()
    c.packed, c.sets, c.lags, c.strides = packed, sets, lags, tuple(strides)
    return c


def _npt(base, seed_cells):
    """per-frame cells around ``base`` (test_gpu_bond.py's NPT recipe, every base with a generator of its own)"""
    rng = np.random.default_rng(seed_cells)
    F = 45
    cells = np.stack([base * (1.0 + 0.01 * rng.normal()) for _ in range(F)])
    return B._walk(cells, B._numbers4(97), F, 15)


def planted(where, seed, cell=DIAG):
    """test_gpu_bond.py's ``_planted`` -- four frames, the pairs edge_plant puts across the f32 guard band sit there in frame
    ``where`` and at half the planted vector in the others -- without its atoms thousands of cells away: at that distance
    float64 itself resolves a vector to 1e-10 only, and the restatement's budget (tests/reorientation_ref.py) is to stay
    below 2^-30 per term on every input that is held against it.  (``test_gpu_bond._planted`` itself, with those atoms, runs
    in the GPU test for the assertions that need no restatement.)"""
    from amof_amd.frames import PackedTrajectory
    from tests import edge_plant as E
    numbers = np.repeat([7, 30], [160, 140])
    rcm = np.array([[3.1, 3.4], [3.4, 2.9]])
    pl = E.plant_nbr(cell, numbers, rcm, seed, F=1, far=False)
    p0 = pl.packed.pos[0]
    vec = p0[pl.j] - p0[pl.i]
    near = p0.copy()
    near[pl.j] = p0[pl.i] + 0.5 * (vec - pl.m @ cell) + pl.m @ cell
    frames = [near.copy(), near.copy(), near.copy(), near.copy()]
    frames[where] = p0
    return PackedTrajectory(np.stack(frames), cell, numbers), pl


def class_windows(F, delta_time):
    from amof_amd.lags import window_setup
    return window_setup(F, delta_time, "half", 1)


def split(name):
    """"rect@mirror" -> ("rect", "mirror"): a case whose cell is stored in a form of tests/cell_forms.py"""
    base, _, form = name.partition("@")
    return base, form or None


@functools.lru_cache(maxsize=None)
def case(name):
    """the case ``name``; "name@form" is the same case built in the cell cell_forms.apply(cell, form)"""
    name, form = split(name)
    if form is not None:
        assert name in ("rect", "four", "sheared", "npt_diag", "npt_sheared") or name.startswith("planted"), name
    return _build(name, cell_forms.apply(B.DIAG, form), cell_forms.apply(B.SHEARED, form))


def _build(name, DIAG, SHEARED):
    if name == "rect":
        return _case(B._walk(DIAG, np.full(150, 30), 131, 11), [(30, 30, 3.1)], RECT_LAGS, (1, 3))
    if name == "four":
        return _case(B._walk(DIAG, B._numbers4(203), 70, 12), FOUR_SETS, FOUR_LAGS, (1, 3))
    if name == "sheared":
        return _case(B._walk(SHEARED, B._numbers4(131), 67, 13), [(30, 7, 3.3), (6, 1, 3.0)], [0, 1, 4, 30, 65])
    if name == "npt_diag":
        return _case(_npt(DIAG, 14), [(30, 7, 3.5), (7, 7, 3.2)], [0, 2, 9, 43], (2,))
    if name == "npt_sheared":
        return _case(_npt(SHEARED, 18), [(30, 7, 3.5), (7, 7, 3.2)], [0, 2, 9, 43], (2,))
    if name == "open":
        return _case(B._walk(DIAG, B._numbers4(120), 50, 16, pbc=(True, False, True)), [(30, 7, 3.5), (1, 6, 3.2)], [0, 1, 10, 48])
    if name == "open_thin":
        return _case(B._walk(np.diag([17.31, 5.0, 21.77]), B._numbers4(60), 20, 17, pbc=(True, False, True)), [(30, 7, 3.5)],
                     [0, 1, 5])
    if name.startswith("planted"):
        where = int(name[-1])
        return _case(planted(where, 40 + where, DIAG)[0], PLANT_SETS, [0, 1, 2])
    if name == "composition":
        return _case(B._walk(DIAG, B._numbers4(203), 70, 21), COMP_SETS, COMP_LAGS, (1, 4))
    if name == "class":
        tr = H.random_walk(H.zif4_frame(), 80, 0.05, 5)
        return _case(tr, CLASS_SETS, [int(m) for m in class_windows(80, 5)[0]], (2,))
    if name == "ranks":
        tr = H.random_walk(H.zif4_frame(), 30, 0.05, 5, cell_jitter=0.003)
        return _case(tr, CLASS_SETS, [int(m) for m in class_windows(30, 3)[0]])
    if name == "arguments":
        return _case(B._walk(DIAG, B._numbers4(64), 10, 22), [(30, 7, 3.0)], [0, 1])
    raise KeyError(name)


NAMES = ["rect", "four", "sheared", "npt_diag", "npt_sheared", "open", "open_thin", "planted1", "planted2", "planted3",
         "composition", "class", "ranks", "arguments"]
# (the zero-length-vector input of the GPU tests is the "arguments" walk with one atom moved onto another: an error return by
# construction, with no sums and no budget)


@functools.lru_cache(maxsize=None)
def reference(name, stride, centres=None):
    """the restatement's ``Result`` of a case, computed once per process and left unchanged"""
    c = case(name)
    p = c.packed
    return ref.reorientation(p.pos, p.cell, p.numbers, c.sets, c.lags, stride, pbc=tuple(p.pbc), centres=centres)


def coincident():
    """the "arguments" walk with N atom 0 of the set put onto its Zn centre in frame 1 (an origin frame)"""
    from amof_amd.frames import PackedTrajectory
    p = case("arguments").packed
    pos = np.array(p.pos, copy=True)
    zn = int(np.nonzero(p.numbers == 30)[0][0])
    n = int(np.nonzero(p.numbers == 7)[0][0])
    pos[1, n] = pos[1, zn]
    return PackedTrajectory(pos, p.cell, p.numbers, pbc=p.pbc)
