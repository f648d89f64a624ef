"""rdf_tile_zf with slab culling keeps the j > i masks of a diagonal tile pair to the sub-tile's own 128-partner block
(everything behind it runs the unmasked loop and the ragged tail quad) and serves the pairs that find their lane's queue
full from one shared refinement body.  AMOF_RDF_NOREACH=1 masks every quad of a diagonal pair again inside the same
binary.  Both must give the oracle's integers, array for array: every case has three frames, one of them shifted by half
the long axis so that the partner window wraps into two pieces."""

import os

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from oracle import clib
from tests import helpers as H

pytestmark = pytest.mark.gpu

BOX = np.array([14.0, 15.0, 48.0])


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


def _check(hip_ctx, packed, settings):
    kinds, sp = H.species_of(packed.numbers)
    for rmax, nb in settings:
        ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), rmax, nb, cell_list=True)
        # (a case that leaves a species pair without in-range pairs would not test that pair's tiles)
        assert ref.sum(axis=2).min() > 0, (rmax, nb, ref.sum(axis=2))
        got = {}
        for name, env in (("default", {}), ("noreach", {"AMOF_RDF_NOREACH": "1"})):
            with _env(AMOF_RDF_NOCELL="1", AMOF_RDF_NORANGE="1", **env):
                got[name], _, _ = hip_ctx.rdf_accumulate(packed, rmax, nb)
                assert hip_ctx.last_path() == "rdf_tile_zf"
        for name, h in got.items():
            assert np.array_equal(h, ref), (name, rmax, nb, int(h.sum()), int(ref.sum()),
                                            int(np.abs(h.astype(np.int64) - ref.astype(np.int64)).sum()))
        assert np.array_equal(got["default"], got["noreach"])


def _shifted(pos, rng=None, sigma=0.05):
    """three frames: the positions, a slightly moved copy, and one shifted by half the long axis"""
    second = pos + 0.25 if rng is None else pos + rng.normal(0, sigma, pos.shape)
    return np.stack([pos, second, pos + np.array([0.0, 0.0, 0.5 * BOX[2]])])


def test_reach_lattice_pairs_on_bin_edges(hip_ctx):
    # a perfect lattice in its long box: every distance on a bin edge (provisional count + fix-up for every in-range
    # pair); 259 atoms of two species each: diagonal pairs of three sub-tiles, the last ragged
    a, n = 2.0, (6, 6, 18)
    pos = np.array([[x, y, z] for x in range(n[0]) for y in range(n[1]) for z in range(n[2])], dtype=float) * a
    numbers = np.where(np.arange(len(pos)) % 5 == 0, 30, np.where(np.arange(len(pos)) % 2 == 0, 7, 6))
    cell = np.diag([n[0] * a, n[1] * a, n[2] * a])
    frames = np.stack([pos, pos + 0.25, pos + np.array([0.0, 0.0, 0.5 * n[2] * a])])
    assert max(int((numbers == k).sum()) for k in (30, 7, 6)) > 128
    _check(hip_ctx, PackedTrajectory(frames, cell, numbers), [(5.9, 59), (6.0, 600), (6.0, 6), (5.999, 2310)])


@pytest.mark.parametrize("count", [63, 64, 65, 127, 128, 129, 193, 513, 640])
def test_reach_sub_tile_size_boundaries(hip_ctx, count):
    # half a sub-tile and less (<= 64 centres), the 64 / 65 boundary, ragged last sub-tiles, more than one tile per species, diagonal
    # tile pairs of 1 to 5 sub-tiles -- next to a second species of 700 atoms (two tiles)
    rng = np.random.default_rng(1000 + count)
    N = count + 700
    pos = rng.uniform(0, 1, (N, 3)) * BOX
    numbers = np.where(np.arange(N) < count, 7, 6)
    packed = PackedTrajectory(_shifted(pos, rng), np.diag(BOX), numbers)
    _check(hip_ctx, packed, [(7.0, 700), (3.0, 50)])


def test_reach_bunched_layers_and_rare_species(hip_ctx):
    # four thin layers along the long axis (a whole sub-tile inside one slab) plus a
    # rare species spread over all of it (its sub-tiles span more than 1/16 of the axis: integer slab differences
    # inside the same launch); two coincident atoms
    rng = np.random.default_rng(77)
    N = 2000
    z = np.concatenate([rng.normal(c, 0.4, 400) for c in (3.0, 11.0, 30.0, 41.0)])
    z = np.concatenate([z, rng.uniform(0, BOX[2], N - len(z))])
    pos = np.column_stack([rng.uniform(0, 1, (N, 2)) * BOX[:2], z])
    pos[7] = pos[3]
    numbers = np.where(np.arange(N) >= 1800, 30, np.where(np.arange(N) % 2 == 0, 6, 1))
    packed = PackedTrajectory(_shifted(pos, rng), np.diag(BOX), numbers)
    _check(hip_ctx, packed, [(7.0, 700), (6.5, 2310), (3.0, 50)])


def test_reach_own_block_masks(hip_ctx):
    # one species of 300 atoms: diagonal tile pairs only (three sub-tiles, the last ragged)
    rng = np.random.default_rng(300)
    pos = rng.uniform(0, 1, (300, 3)) * BOX
    packed = PackedTrajectory(_shifted(pos, rng), np.diag(BOX), np.full(300, 6))
    _check(hip_ctx, packed, [(7.0, 700)])
