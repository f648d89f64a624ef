"""The planned tile kernel (rdf_tile_kernel_fast, PLAN) takes a lane's two centre atoms from the quantised frame in global
memory straight into registers; its LDS holds no centre buffers, so that six workgroups fit a CU at the headline's
histogram.  AMOF_RDF_NOPLAN=1 runs the kernel with centre buffers inside the same binary.  Every case compares three
integer histograms bit for bit: the default path, the same call without the plan, and the CPU oracle over every frame.

ZIF-4 x 2x2x6 (6528 atoms: H and C 2304 each, N 1536, Zn 384) is the smallest system with steps on f32 slab coordinates,
dead steps and wrapped windows (tests/tile_ahead_cases.py).  19 frames are neither a multiple of 8 nor of 16: chunks of
unequal length by default, and with eight frames per chunk (6, 6 and 7 frames, frame changes and dead steps inside a chunk).
Rows of one frame behind the chunks exist from 32 chunks on only: `tail_rows` has 33 frames in chunks of one (32 + 1)."""

import os

import numpy as np
import pytest

from amof_amd.frames import Frame
from oracle import clib
from tests import helpers as H
from tests import tile_ahead_cases as T

pytestmark = pytest.mark.gpu

REPS = (2, 2, 6)
FRAMES = 19


def _zif():
    return T._zif(REPS)


def _thinned():
    """one species with an odd count (N 1535: a last lane without its second centre), one with fewer than 64 atoms (Zn 50: a
    sub-tile whose second half is empty; H 2234 = 17 x 128 + 58 ends on such a sub-tile too), none a multiple of 128 (C 2301)"""
    fr = _zif()
    rng = np.random.default_rng(1313)
    keep = np.ones(len(fr.numbers), dtype=bool)
    for z, k in ((30, 334), (7, 1), (6, 3), (1, 70)):
        keep[rng.choice(np.nonzero(fr.numbers == z)[0], k, replace=False)] = False
    out = Frame(fr.numbers[keep], fr.positions[keep], fr.cell, fr.pbc)
    counts = {int(z): int((out.numbers == z).sum()) for z in (1, 6, 7, 30)}
    assert counts == {1: 2234, 6: 2301, 7: 1535, 30: 50} and all(c % 128 for c in counts.values())
    return out


def _walk(frame, F=FRAMES, **kw):
    return H.random_walk(frame, F, 0.05, 1300, ortho=True, **kw)


TRAJECTORIES = {
    "walk": lambda: _walk(_zif()),
    "walk33": lambda: _walk(_zif(), 33),
    "thinned": lambda: _walk(_thinned()),
    "breathing": lambda: _walk(_zif(), cell_jitter=0.004),     # n_cells = F
}

# name: (trajectory, dr, environment, frame range)
CASES = {
    "walk19": ("walk", 0.01, {}, None),
    "walk19_fpc8": ("walk", 0.01, {"AMOF_RDF_FPC": "8"}, None),
    "tail_rows": ("walk33", 0.01, {"AMOF_RDF_FPC": "1"}, None),
    "thinned": ("thinned", 0.01, {}, None),
    # 7 600 bins: three workgroups per CU at the most -- the result may not depend on how many are resident
    "fine_bins": ("walk", 0.002, {}, None),
    # the scales are read again in every step, next to the centre loads
    "cell_per_frame": ("breathing", 0.01, {}, None),
    "frame_range": ("walk", 0.01, {}, (3, 17)),                       # f_base != 0
    "no_read_ahead": ("walk", 0.01, {"AMOF_RDF_NOAHEAD": "1"}, None),     # the AHEAD = 0 instantiation
}

_traj, _ref = {}, {}


def _case(name):
    tname, dr, env, frange = CASES[name]
    if tname not in _traj:
        _traj[tname] = TRAJECTORIES[tname]()
    packed = _traj[tname]
    rmax = float(np.min(packed.cell_lengths()) / 2)
    nbins = int(rmax // dr)
    rkey = (tname, nbins, frange)
    if rkey not in _ref:
        kinds, sp = H.species_of(packed.numbers)
        lo, hi = frange or (0, packed.pos.shape[0])
        cell = np.asarray(packed.cell)
        ref, _ = clib.rdf_hist(packed.pos[lo:hi], cell[lo:hi] if len(cell) > 1 else cell, sp, len(kinds), rmax, nbins, cell_list=True)
        ref.setflags(write=False)
        _ref[rkey] = ref
    return packed, rmax, nbins, env, frange, _ref[rkey]


def _run(hip_ctx, packed, rmax, nbins, env, frange):
    env = dict(env, AMOF_RDF_NOCELL="1", AMOF_RDF_NORANGE="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        h, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins, frame_range=frange)
        path = hip_ctx.last_path()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return h, path


@pytest.mark.parametrize("name", list(CASES))
def test_centres_from_global_memory(hip_ctx, name):
    packed, rmax, nbins, env, frange, ref = _case(name)
    assert ref.sum(axis=2).min() > 0, (name, ref.sum(axis=2))
    # the plan is in use: slab culling (the host's 2 rmax 1.05 < longest height), a diagonal cell, chunks of at most 16 frames
    L = np.asarray(packed.cell).reshape(-1, 3, 3)
    assert all(2.0 * rmax * 1.05 < np.diag(c).max() for c in L) and not os.environ.get("AMOF_RDF_NOPLAN")
    kinds, sp = H.species_of(packed.numbers)
    ntiles = len(T.tiles_of([int((sp == s).sum()) for s in range(len(kinds))]))
    nf = (frange[1] - frange[0]) if frange else packed.pos.shape[0]
    assert T.frames_per_chunk(nf, ntiles * (ntiles + 1) // 2, env) <= 16
    got = {"default": _run(hip_ctx, packed, rmax, nbins, env, frange),
           "noplan": _run(hip_ctx, packed, rmax, nbins, dict(env, AMOF_RDF_NOPLAN="1"), frange)}
    for mode, (h, path) in got.items():
        assert path == "rdf_tile_zf", (name, mode, path)
        print(name, mode, "bins", nbins, "pairs", int(h.sum()))
        assert np.array_equal(h, ref), (name, mode, int(h.sum()), int(ref.sum()),
                                        int(np.abs(h.astype(np.int64) - ref.astype(np.int64)).sum()))
    assert np.array_equal(got["default"][0], got["noplan"][0]), name
