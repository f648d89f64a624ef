"""The plan variant of the slab-culled tile kernel reads the partner records of a wave's next quad while it works on the
quad in hand (rdf_tile_kernel_fast, AHEAD; AMOF_RDF_NOAHEAD=1: the kernel without it, inside the same binary).  Histograms
must be the oracle's integers and the switched-off kernel's, array for array, on inputs whose windows have every shape the
read-ahead handles apart: tests/tile_ahead_cases.py, classified on the CPU by tests/test_tile_ahead_cpu.py.  `long_cell` has
14 pieces of fewer than 16 partners (some wave has no quad there and reads nothing) and 208 ragged last quads.

The plan is in use when the path is rdf_tile_zf with slab culling and a chunk holds at most 16 frames: the host's
conditions, restated by tile_ahead_cases.frames_per_chunk and asserted here (the library reports the path, not the plan)."""

import os

import numpy as np
import pytest

from oracle import clib
from tests import helpers as H
from tests import tile_ahead_cases as T

pytestmark = pytest.mark.gpu

_cache = {}


def _case(name):
    if name not in _cache:
        packed, rmax, nbins, env = T.CASES[name]()
        kinds, sp = H.species_of(packed.numbers)
        ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), rmax, nbins, cell_list=True)
        ref.setflags(write=False)
        _cache[name] = (packed, rmax, nbins, env, ref)
    return _cache[name]


def _run(hip_ctx, packed, rmax, nbins, env):
    env = dict(env, AMOF_RDF_NOCELL="1", AMOF_RDF_NORANGE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins)
        stats = hip_ctx.job_stats()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return h, stats


@pytest.mark.parametrize("setting", [s[0] for s in T.SETTINGS])
@pytest.mark.parametrize("name", sorted(T.CASES))
def test_read_ahead_matches_oracle(hip_ctx, name, setting):
    packed, rmax, nbins, env, ref = _case(name)
    assert ref.sum(axis=2).min() > 0, (name, ref.sum(axis=2))
    # the plan: slab culling (the host's 2 rmax 1.05 < longest height), diagonal cell, chunks of at most 16 frames
    L = np.diag(np.asarray(packed.cell).reshape(-1, 3, 3)[0])
    assert 2.0 * rmax * 1.05 < L.max() and not os.environ.get("AMOF_RDF_NOPLAN")
    kinds, sp = H.species_of(packed.numbers)
    ntiles = len(T.tiles_of([int((sp == s).sum()) for s in range(len(kinds))]))
    assert T.frames_per_chunk(packed.pos.shape[0], ntiles * (ntiles + 1) // 2, env) <= 16
    h, stats = _run(hip_ctx, packed, rmax, nbins, dict(env, **dict(T.SETTINGS)[setting]))
    assert stats["path"] == "rdf_tile_zf", stats
    print(name, setting, "pairs", int(h.sum()), "kernel ms", 1e3 * stats["kernel_s_dominant"])
    assert np.array_equal(h, ref), (name, setting, int(h.sum()), int(ref.sum()),
                                    int(np.abs(h.astype(np.int64) - ref.astype(np.int64)).sum()))
    if setting != "off":
        h_off, stats_off = _run(hip_ctx, packed, rmax, nbins, dict(env, **dict(T.SETTINGS)["off"]))
        assert stats_off["path"] == "rdf_tile_zf"
        assert np.array_equal(h, h_off), (name, setting)
