"""rdf_tile_zf with slab culling runs from a plan of its steps: the quantiser's slab table gives every (frame, centre
sub-tile, partner tile) its partner window once (amof_amd/csrc/tile_plan.h, rdf_tile_plan_kernel), a step without a quad to
visit is skipped, a frame without a live step stages no partner tile and a work item without one returns at once.
AMOF_RDF_NOPLAN=1 restores the search over sampled quads in every step inside the same binary (AMOF_RDF_PLAN_NOSKIP=1: the
plan's windows, every step run).  All of them must give the oracle's integers, array for array."""

import os

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from oracle import clib
from tests import helpers as H

pytestmark = pytest.mark.gpu

BOX = np.array([14.0, 15.0, 48.0])
LONG = np.array([14.0, 15.0, 96.0])

MODES = (("default", {}), ("noplan", {"AMOF_RDF_NOPLAN": "1"}), ("noskip", {"AMOF_RDF_PLAN_NOSKIP": "1"}))


class _env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _run(hip_ctx, packed, rmax, nb, env, frame_range=None):
    with _env(AMOF_RDF_NOCELL="1", AMOF_RDF_NORANGE="1", **env):
        h, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nb, frame_range=frame_range)
        assert hip_ctx.last_path() == "rdf_tile_zf"
    return h


def _check(hip_ctx, packed, settings, extra_env=None):
    kinds, sp = H.species_of(packed.numbers)
    refs = []
    for rmax, nb in settings:
        ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), rmax, nb, cell_list=True)
        # (a case that leaves a species pair without in-range pairs would not test that pair's tiles)
        assert ref.sum(axis=2).min() > 0, (rmax, nb, ref.sum(axis=2))
        got = {name: _run(hip_ctx, packed, rmax, nb, dict(env, **(extra_env or {}))) for name, env in MODES}
        for name, h in got.items():
            assert np.array_equal(h, ref), (name, rmax, nb, int(h.sum()), int(ref.sum()),
                                            int(np.abs(h.astype(np.int64) - ref.astype(np.int64)).sum()))
        refs.append(ref)
    return refs


def test_plan_dead_steps_frames_and_work_items(hip_ctx):
    # one species of 2100 uniform atoms along a 96 A axis: five tiles, so that tile pairs two apart have no live step at
    # all; a second species of 300 atoms in a 4 A layer, which sits somewhere else in the middle frame (its work items go
    # live -> dead -> live); the last frame shifted by half the long axis (windows in two pieces)
    rng = np.random.default_rng(2100)
    n_a, n_b = 2100, 300
    pos = rng.uniform(0, 1, (n_a + n_b, 3)) * LONG
    pos[n_a:, 2] = 20.0 + rng.uniform(0, 4.0, n_b)
    mid = pos + rng.normal(0, 0.05, pos.shape)
    mid[n_a:, 2] += 50.0
    frames = np.stack([pos, mid, pos + np.array([0.0, 0.0, 0.5 * LONG[2]])])
    numbers = np.where(np.arange(n_a + n_b) < n_a, 6, 30)
    _check(hip_ctx, PackedTrajectory(frames, np.diag(LONG), numbers), [(7.0, 700), (3.0, 50)])


def test_plan_bunched_layers(hip_ctx):
    # a whole sub-tile inside one slab (130 atoms at one z), a whole partner tile inside one slab (520 at another), long
    # runs of empty slabs between the layers, atoms at z = 0 and at the last representable z below Lz
    rng = np.random.default_rng(78)
    Lz = BOX[2]
    z6 = np.concatenate([np.full(130, 3.0), np.full(520, 11.03), rng.normal(30.0, 0.4, 200), np.zeros(5),
                         np.full(5, np.nextafter(Lz, 0.0))])
    z1 = np.concatenate([rng.normal(c, 0.3, 75) for c in (2.0, 12.0, 31.0, 47.5)])
    z = np.concatenate([z6, z1])
    pos = np.column_stack([rng.uniform(0, 1, (len(z), 2)) * BOX[:2], z])
    numbers = np.where(np.arange(len(z)) < len(z6), 6, 1)
    shift = pos + np.array([0.0, 0.0, 0.5 * Lz])
    frames = np.stack([pos, pos + np.array([0.3, 0.2, 0.0]), shift])
    _check(hip_ctx, PackedTrajectory(frames, np.diag(BOX), numbers), [(7.0, 700), (6.5, 2310), (3.0, 50)])


@pytest.mark.parametrize("count", [64, 65, 128, 129, 513])
def test_plan_sub_tile_size_boundaries(hip_ctx, count):
    rng = np.random.default_rng(1000 + count)
    N = count + 700
    pos = rng.uniform(0, 1, (N, 3)) * BOX
    numbers = np.where(np.arange(N) < count, 7, 6)
    frames = np.stack([pos, pos + rng.normal(0, 0.05, pos.shape), pos + np.array([0.0, 0.0, 0.5 * BOX[2]])])
    _check(hip_ctx, PackedTrajectory(frames, np.diag(BOX), numbers), [(7.0, 700), (3.0, 50)])


def _walk(F, rng):
    N = 700
    pos = rng.uniform(0, 1, (N, 3)) * BOX
    frames = pos[None] + np.cumsum(rng.normal(0, 0.15, (F, N, 3)), axis=0)
    return frames, np.where(np.arange(N) < 500, 6, 7)


def test_plan_frame_bookkeeping(hip_ctx):
    # 40 frames: chunks of two frames by default, of unequal length (2 or 3) with three frames per chunk, batches of
    # 16 + 24 frames (batch-local frame indices); frame ranges cut inside a chunk add up to the whole
    rng = np.random.default_rng(40)
    frames, numbers = _walk(40, rng)
    packed = PackedTrajectory(frames, np.diag(BOX), numbers)
    (ref,) = _check(hip_ctx, packed, [(7.0, 350)])
    _check(hip_ctx, packed, [(7.0, 350)], {"AMOF_RDF_FPC": "3"})
    _check(hip_ctx, packed, [(7.0, 350)], {"AMOF_RDF_BATCH": "16"})
    for k in (13, 1):
        parts = _run(hip_ctx, packed, 7.0, 350, {}, (0, k)).astype(np.int64) + _run(hip_ctx, packed, 7.0, 350, {}, (k, 40))
        assert np.array_equal(parts, ref.astype(np.int64)), k


def test_plan_tail_rows(hip_ctx):
    # 43 frames in chunks of one: 40 chunks dealt over the XCDs and the 43 % 8 frames behind them, one grid row each
    rng = np.random.default_rng(43)
    frames, numbers = _walk(43, rng)
    _check(hip_ctx, PackedTrajectory(frames, np.diag(BOX), numbers), [(7.0, 350)], {"AMOF_RDF_FPC": "1"})


def test_plan_cell_changes_per_frame(hip_ctx):
    # +-1 % breathing of a diagonal cell: cull_gap differs from frame to frame
    rng = np.random.default_rng(5)
    F, N = 5, 900
    scale = 1.0 + 0.01 * np.sin(np.arange(F) * 1.3)
    cells = np.stack([np.diag(BOX * s) for s in scale])
    frac = rng.uniform(0, 1, (N, 3))
    frames = np.stack([(frac + rng.normal(0, 0.002, frac.shape)) * BOX * s for s in scale])
    frames[-1] += np.array([0.0, 0.0, 0.5 * BOX[2]])
    numbers = np.where(np.arange(N) < 600, 6, 7)
    _check(hip_ctx, PackedTrajectory(frames, cells, numbers), [(6.9, 690), (3.0, 50)])


def test_plan_lattice_pairs_on_bin_edges(hip_ctx):
    # a perfect lattice in its long box: every distance on a bin edge (provisional count + fix-up for every in-range pair)
    a, n = 2.0, (6, 6, 18)
    pos = np.array([[x, y, z] for x in range(n[0]) for y in range(n[1]) for z in range(n[2])], dtype=float) * a
    numbers = np.where(np.arange(len(pos)) % 5 == 0, 30, np.where(np.arange(len(pos)) % 2 == 0, 7, 6))
    cell = np.diag([n[0] * a, n[1] * a, n[2] * a])
    frames = np.stack([pos, pos + 0.25, pos + np.array([0.0, 0.0, 0.5 * n[2] * a])])
    _check(hip_ctx, PackedTrajectory(frames, cell, numbers), [(5.9, 59), (6.0, 600), (5.999, 2310)])
