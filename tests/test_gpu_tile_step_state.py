"""The planned tile kernel (rdf_tile_kernel_fast, PLAN) runs a grid of two z slices over one plan: slice 0 the steps in integer
form, slice 1 the steps on f32 slab coordinates, each with the body of its form alone.  In both the work item's constants
are re-made per step instead of being carried across the quad loops, a level-3 refinement addresses positions, cell record
and partner segment from the kernel's arguments at that point, and the next step's record is fetched behind the last quad
loop.  Every case compares three integer histograms bit for bit: the default path, AMOF_RDF_NOPLAN=1 (the kernel without a
plan, unchanged) and the CPU oracle over every frame.  The inputs and what their steps are: tests/tile_step_state_cases.py;
that `graded` holds work items with both forms and sub-tiles that change form inside a chunk is checked here on the CPU
before its histograms are relied on (and without a GPU in tests/test_tile_step_state_cpu.py)."""

import os

import numpy as np
import pytest

from oracle import clib
from tests import helpers as H
from tests import tile_ahead_cases as T
from tests import tile_step_state_cases as C

pytestmark = pytest.mark.gpu

# name: (trajectory, environment)
CASES = {
    "zif544": ("zif544", {}),                                        # 19 frames in chunks of two: the last chunk is ragged
    "zif544_fpc8": ("zif544", {"AMOF_RDF_FPC": "8"}),                # chunks of 6, 6 and 7 frames
    "zif544_batch7": ("zif544", {"AMOF_RDF_BATCH": "7"}),            # batches of 7, 7 and 5 frames: the plan is rebuilt, f_base != 0
    "zif544_no_read_ahead": ("zif544", {"AMOF_RDF_NOAHEAD": "1"}),
    "graded": ("graded", {}),
    "graded_fpc8": ("graded", {"AMOF_RDF_FPC": "8"}),
    "graded_batch7": ("graded", {"AMOF_RDF_BATCH": "7"}),
    "graded_no_read_ahead": ("graded", {"AMOF_RDF_NOAHEAD": "1"}),
    # every distance on a bin edge: level-3 refinements, which address the frame's positions from the batch's first frame
    # (batches of two frames) and the cell record by the frame (one cell per frame)
    "lattice_batch2": ("lattice", {"AMOF_RDF_BATCH": "2"}),
    "lattice_cell_per_frame": ("lattice_cells", {}),
}

_traj, _ref = {}, {}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return T.build_driver(tmp_path_factory.mktemp("tile_step_state"))


def _case(name):
    tname, env = CASES[name]
    if tname not in _traj:
        packed, rmax, nbins = C.TRAJECTORIES[tname]()
        kinds, sp = H.species_of(packed.numbers)
        ref, _ = clib.rdf_hist(packed.pos, np.asarray(packed.cell), sp, len(kinds), rmax, nbins, cell_list=True)
        ref.setflags(write=False)
        _traj[tname], _ref[tname] = (packed, rmax, nbins), ref
    return _traj[tname] + (env, _ref[tname])


def _run(hip_ctx, packed, rmax, nbins, env):
    env = dict(env, AMOF_RDF_NOCELL="1", AMOF_RDF_NORANGE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins)
        path = hip_ctx.last_path()         # (= _stats["path"] of the classes: amof_last_path)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return h, path


@pytest.mark.parametrize("name", list(CASES))
def test_two_slices_of_the_planned_kernel(hip_ctx, driver, name):
    packed, rmax, nbins, env, ref = _case(name)
    assert ref.sum(axis=2).min() > 0, (name, ref.sum(axis=2))
    # the plan is in use: slab culling (the host's 2 rmax 1.05 < longest height), a diagonal cell, chunks of at most 16 frames
    L = np.asarray(packed.cell).reshape(-1, 3, 3)
    assert all(2.0 * rmax * 1.05 < np.diag(c).max() for c in L) and not os.environ.get("AMOF_RDF_NOPLAN")
    nf = packed.pos.shape[0]
    batch = int(env.get("AMOF_RDF_BATCH", nf))
    # what the slices meet, batch by batch (a batch is planned and chunked on its own)
    seen = {}
    for lo in range(0, nf, batch):
        st, tiles, pairs = C.steps(packed, rmax, driver, env, frames=(lo, min(nf, lo + batch)))
        for k, v in C.census(st).items():
            seen[k] = seen.get(k, 0) + v
    print(name, seen)
    if CASES[name][0] == "graded":
        # both forms, next to each other in one work item; a sub-tile that takes both inside one chunk; work items that only
        # one of the slices has anything to do for, and dead steps
        assert all(seen[k] > 0 for k in ("zf", "integer", "dead", "mixed_items", "integer_only_items", "sub_in_both_forms")), (name, seen)
        assert len(tiles) == 5 and tiles[3][2] % 4 == 1 and tiles[3][2] % 128 and tiles[4][2] < 128      # ragged tile, thin species
    elif CASES[name][0] == "zif544":
        assert seen["zf"] == 0 and seen["integer"] > 0, (name, seen)
    else:
        assert seen["zf"] > 0, (name, seen)
    got = {"default": _run(hip_ctx, packed, rmax, nbins, env),
           "noplan": _run(hip_ctx, packed, rmax, nbins, dict(env, AMOF_RDF_NOPLAN="1"))}
    for mode, (h, path) in got.items():
        assert path == "rdf_tile_zf", (name, mode, path)
        print(name, mode, "bins", nbins, "pairs", int(h.sum()))
        assert np.array_equal(h, ref), (name, mode, int(h.sum()), int(ref.sum()),
                                        int(np.abs(h.astype(np.int64) - ref.astype(np.int64)).sum()))
    assert np.array_equal(got["default"][0], got["noplan"][0]), name
