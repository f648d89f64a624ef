"""The saturating tail of the planned tile kernel's f32-slab slice (rdf_tile_kernel_fast<..., PLAN, AHEAD, SAT>, fast_bin<SAT>;
amof_amd/csrc/rdf_sat_math.h): no per-pair clamp, the histogram one word up in LDS, refinements that start from q' = q + g + 1.
Every case asserts the path rdf_tile_zf with the plan in use, and compares three integer histograms bit for bit: the default
build of the launch, AMOF_RDF_NOSAT=1 (the clamped tail inside the same binary) and the CPU oracle over every frame.

Two systems, 20 frames each (the host deals them in chunks of two; AMOF_RDF_FPC=16: one chunk of 16 frames and a ragged one):
  z222   ZIF-4 x 2x2x2 (2176 atoms, H and C 768 each: two tiles per species, ragged sub-tiles, diagonal and off-diagonal tile
         pairs, slab culling on the 36.9 A axis at the default cutoff).  Its sub-tiles span some 40 of the 256 slabs, so every
         step of it runs in integer form: it checks the launch around the new tail -- the LDS layout with the pad word, the
         integer slice beside a saturating slice that has nothing to do -- and not the tail itself.
  z226   ZIF-4 x 2x2x6 without one atom of every species (6524 atoms, ragged tiles): sub-tiles of H, C and N span fewer than
         16 slabs, their steps run on f32 slab coordinates -- the saturating tail -- next to Zn's in integer form.
plus the perfect lattice of tests/tile_ahead_cases.py (the construction of tests/test_gpu_paths.py: every distance on a bin
edge, every in-range pair refined from its q', the lanes' queues overflow).  Which form the steps take is counted on the CPU
(tests/tile_step_state_cases.py) before a histogram is relied on -- frame by frame where every frame has its own cell -- and
that the selection hands the launch the saturating tail (and AMOF_RDF_NOSAT=1 takes it away) is asked of rdf_select.h itself,
through tests/native/tile_sat_select_driver.cpp: both runs report the path rdf_tile_zf."""

import os
import subprocess

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from oracle import clib
from tests import helpers as H
from tests import tile_ahead_cases as T
from tests import tile_step_state_cases as C

pytestmark = pytest.mark.gpu

FRAMES = 20


def _walk(reps, delete, seed, cell_jitter=0.0):
    frame = T._zif(reps)
    if delete:
        frame = T._delete(frame, delete)
    return H.random_walk(frame, FRAMES, 0.05, seed, ortho=True, cell_jitter=cell_jitter)


def _close_pairs(packed):
    """two atoms of the first species on top of each other, two more 0.001 A apart, in every frame"""
    pos = np.asarray(packed.pos).copy()
    first = np.nonzero(packed.numbers == packed.numbers[0])[0]
    a, b, c, d = first[:4]
    pos[:, b] = pos[:, a]
    pos[:, d] = pos[:, c] + np.array([0.0006, -0.0008, 0.0])
    return PackedTrajectory(pos, np.asarray(packed.cell), packed.numbers, pbc=packed.pbc)


def _cells_per_frame(packed):
    cell = np.asarray(packed.cell).reshape(-1, 3, 3)[:1]
    return PackedTrajectory(np.asarray(packed.pos), np.repeat(cell, packed.pos.shape[0], axis=0), packed.numbers, pbc=packed.pbc)


def _system(name):
    reps, delete, seed = {"z222": ((2, 2, 2), 0, 1500), "z226": ((2, 2, 6), 1, 1510)}[name]
    return _walk(reps, delete, seed)


TRAJECTORIES = {
    "z222": lambda: _system("z222"),
    "z226": lambda: _system("z226"),
    "z222_close": lambda: _close_pairs(_system("z222")),
    "z226_close": lambda: _close_pairs(_system("z226")),
    "z222_cells": lambda: _walk((2, 2, 2), 0, 1501, cell_jitter=0.01),
    "z226_cells": lambda: _walk((2, 2, 6), 1, 1511, cell_jitter=0.01),
    "z226_equal_cells": lambda: _cells_per_frame(_system("z226")),
    "lattice": lambda: C.lattice()[0],
}

# name: (trajectory, nbins or None for rmax // 0.01, environment, steps on f32 slab coordinates expected; "frames": the same,
# counted frame by frame with the frame's own cell)
CASES = {}
for _s, _zf in (("z222", False), ("z226", True)):
    CASES.update({
        _s + "_walk": (_s, None, {}, _zf),
        _s + "_close_pairs": (_s + "_close", None, {}, _zf),
        _s + "_2310_bins": (_s, 2310, {}, _zf),                      # every low bit of C = nbins + 1/2 + lane mod 32 in play
        _s + "_31_bins": (_s, 31, {}, _zf),
        _s + "_cell_per_frame": (_s + "_cells", None, {}, "frames"),  # the lanes' constants are made again for every frame's cell
        _s + "_no_read_ahead": (_s, None, {"AMOF_RDF_NOAHEAD": "1"}, _zf),
        _s + "_fpc8": (_s, None, {"AMOF_RDF_FPC": "8"}, _zf),        # chunks of 8, 8 and 4 frames
        _s + "_fpc16": (_s, None, {"AMOF_RDF_FPC": "16"}, _zf),      # one chunk of 16 frames and a ragged one
        _s + "_batch7": (_s, None, {"AMOF_RDF_BATCH": "7"}, _zf),    # batches of 7, 7 and 6 frames: f_base != 0
    })
CASES["z226_equal_cell_per_frame"] = ("z226_equal_cells", None, {}, True)
CASES["lattice_on_bin_edges"] = ("lattice", 600, {}, True)
CASES["lattice_on_bin_edges_no_read_ahead"] = ("lattice", 600, {"AMOF_RDF_NOAHEAD": "1"}, True)

_traj, _ref = {}, {}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return T.build_driver(tmp_path_factory.mktemp("tile_sat"))


@pytest.fixture(scope="module")
def select_driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_sat_select") / "tile_sat_select_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-ffp-contract=off", os.path.join(T.ROOT, "tests", "native", "tile_sat_select_driver.cpp"),
                        "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def _selected(select_driver, packed, rmax, nbins, nosat):
    """(zf, cull, sat, guard) of the selection for this input"""
    L = np.asarray(packed.cell).reshape(-1, 3, 3)
    line = "%d %.17g %d %d %s\n" % (nbins, rmax, int(nosat), len(L), " ".join("%.17g" % v for c in L for v in np.diag(c)))
    w = subprocess.run([select_driver], input=line, capture_output=True, text=True, check=True).stdout.split()
    return int(w[0]), int(w[1]), int(w[2]), float(w[3])


def _census(packed, rmax, driver, env):
    nf = packed.pos.shape[0]
    batch = int(env.get("AMOF_RDF_BATCH", nf))
    seen = {}
    for lo in range(0, nf, batch):
        st, _, _ = C.steps(packed, rmax, driver, env, frames=(lo, min(nf, lo + batch)))
        for k, v in C.census(st).items():
            seen[k] = seen.get(k, 0) + v
    return seen


def _case(name):
    tname, nbins, env, zf = CASES[name]
    if tname not in _traj:
        _traj[tname] = TRAJECTORIES[tname]()
    packed = _traj[tname]
    rmax = 6.0 if tname == "lattice" else float(np.min(packed.cell_lengths()) / 2)
    nbins = nbins or int(rmax // 0.01)
    if (tname, nbins) not in _ref:
        kinds, sp = H.species_of(packed.numbers)
        ref, _ = clib.rdf_hist(packed.pos, np.asarray(packed.cell), sp, len(kinds), rmax, nbins, cell_list=True)
        ref.setflags(write=False)
        _ref[(tname, nbins)] = ref
    return packed, rmax, nbins, env, zf, _ref[(tname, nbins)]


def _run(hip_ctx, packed, rmax, nbins, env):
    env = dict(env, AMOF_RDF_NOCELL="1", AMOF_RDF_NORANGE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins)
        path = hip_ctx.last_path()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return h, path


@pytest.mark.parametrize("name", list(CASES))
def test_saturating_tail_against_the_clamped_one_and_the_oracle(hip_ctx, driver, select_driver, name):
    packed, rmax, nbins, env, zf, ref = _case(name)
    assert ref.sum(axis=2).min() > 0, (name, ref.sum(axis=2))
    # the plan is in use: slab culling (the host's 2 rmax 1.05 < longest height), a diagonal cell, chunks of at most 16 frames
    # (C.steps asserts the chunk size), no switch that takes the plan or the tail away
    L = np.asarray(packed.cell).reshape(-1, 3, 3)
    assert all(2.0 * rmax * 1.05 < np.diag(c).max() and not (c - np.diag(np.diag(c))).any() for c in L)
    assert not any(os.environ.get(k) for k in ("AMOF_RDF_NOPLAN", "AMOF_RDF_NOSAT", "AMOF_RDF_NOZF", "AMOF_RDF_NOCULL"))
    # the selection: f32 slab coordinates, culling and the saturating tail (its guard leaves room in a bin); not with the switch
    sel = _selected(select_driver, packed, rmax, nbins, False)
    print(name, "selection (zf, cull, sat, guard)", sel)
    assert sel[:3] == (1, 1, 1) and sel[3] < 0.25, (name, sel)
    assert _selected(select_driver, packed, rmax, nbins, True)[:3] == (1, 1, 0), name
    if zf == "frames":
        # a cell per frame, no two alike: every frame's steps from its own cell (the form of a step does not depend on the chunk)
        assert len(L) == packed.pos.shape[0] and len({tuple(np.diag(c)) for c in L}) == len(L)
        seen = {}
        for f in range(len(L)):
            one = PackedTrajectory(np.asarray(packed.pos)[f:f + 1], L[f:f + 1], packed.numbers, pbc=packed.pbc)
            for k, v in _census(one, rmax, driver, {}).items():
                seen[k] = seen.get(k, 0) + v
        zf = name.startswith("z226")
    else:
        seen = _census(packed, rmax, driver, env)
    print(name, seen)
    assert (seen["zf"] > 0) == zf and seen["integer"] > 0, (name, seen)
    got = {"default": _run(hip_ctx, packed, rmax, nbins, env),
           "nosat": _run(hip_ctx, packed, rmax, nbins, dict(env, AMOF_RDF_NOSAT="1"))}
    for mode, (h, path) in got.items():
        assert path == "rdf_tile_zf", (name, mode, path)
        print(name, mode, "bins", nbins, "pairs", int(h.sum()))
        assert np.array_equal(h, ref), (name, mode, int(h.sum()), int(ref.sum()),
                                        int(np.abs(h.astype(np.int64) - ref.astype(np.int64)).sum()))
    assert np.array_equal(got["default"][0], got["nosat"][0]), name
