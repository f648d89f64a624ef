"""The lag/origin family's shared host side: ``DistinctVanHove``, ``IntermediateScattering``, ``CurrentCorrelation`` (what
those two share beyond this is amof_amd/lag_q.py), ``BondLifetime``, ``BondReorientation`` (and the windows of
``WindowVanHove``).

Lags m are the windows of ``WindowMsd``; the origins of lag m are the frames k = 1, 1 + s, 1 + 2s, ... <= F - m - 1 (s =
``origin_stride``).  The work list is every (lag, origin) pair, lag-major, origins ascending; ranks and devices take
contiguous index ranges of it.  The library states the same rule once, in amof_amd/csrc/lag_work.h ("The
lag/origin family: shared pieces"); tests/test_lag_work_cpu.py holds the two against each other.
"""

import logging

import numpy as np

from . import _setup

logger = logging.getLogger(__name__)


def window_setup(n_frames, delta_time=100, max_time="half", timestep=1):
    """windows (frames) and times (fs) of ``WindowMsd.from_trajectory`` (amof/msd.py:173-181)"""
    half_time = (n_frames // 2) * timestep
    if (isinstance(max_time, str) and max_time == "half") or max_time > half_time:
        max_time = half_time
    if delta_time < timestep:
        logger.exception("Delta_time should be larger than timestep")
    delta_m = delta_time // timestep
    window = np.arange(0, max_time // timestep, delta_m)
    return window, timestep * window


def check_origin_stride(x):
    """``origin_stride`` as an int; ValueError unless it is an integer >= 1"""
    if int(x) != x or x < 1:
        raise ValueError("origin_stride must be an integer >= 1")
    return int(x)


def origins(n_frames, lag, origin_stride=1):
    """origin frames k = 1, 1 + s, 1 + 2s, ... <= F - m - 1 of lag m (s = 1: ``WindowVanHove``'s origins)"""
    return np.arange(1, max(int(n_frames) - int(lag), 1), int(origin_stride), dtype=np.int64)


def n_origins(n_frames, windows, origin_stride=1):
    """``[W]`` number of origins of every lag (the library's n_w = floor((F - m - 2) / s) + 1, 0 for m > F - 2)"""
    m = np.asarray(windows, dtype=np.int64)
    return np.where(n_frames - m - 2 >= 0, (n_frames - m - 2) // int(origin_stride) + 1, 0).astype(np.int64)


def total_work(n_frames, windows, origin_stride=1):
    """length of the work list"""
    return int(n_origins(n_frames, windows, origin_stride).sum())


def work_list(n_frames, windows, origin_stride=1):
    """``(lag index, origin)`` arrays of the flattened work list in the library's order: lag-major, origins ascending"""
    w = [np.full(len(origins(n_frames, m, origin_stride)), i, dtype=np.int64) for i, m in enumerate(windows)]
    k = [origins(n_frames, m, origin_stride) for m in windows]
    return (np.concatenate(w) if w else np.zeros(0, np.int64)), (np.concatenate(k) if k else np.zeros(0, np.int64))


# (what every class decides before it shards its work is stated once, in _setup.py; the family finds it here)
Setup, pack, setup, begin_local = _setup.Setup, _setup.pack, _setup.setup, _setup.begin_local


def min_periodic_height(cells, pbc):
    """smallest perpendicular cell height over all cells (``[..][3][3]``, rows = cell vectors) on a periodic axis; inf
    without a periodic axis"""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    vol = np.abs(np.linalg.det(cells))
    best = np.inf
    for x in range(3):
        if not pbc[x]:
            continue
        area = np.linalg.norm(np.cross(cells[:, (x + 1) % 3], cells[:, (x + 2) % 3]), axis=1)
        best = min(best, float(np.min(vol / area)))
    return best


def neighbour_sets(packed, nb_set_and_cutoff):
    """What the bond analyses (``BondLifetime``, ``BondReorientation``) make of ``CoordinationNumber``'s dictionary:
    ``(cutoff matrix [S][S], names, live)`` -- names = [(set name, both species present)] in dictionary order, live = the
    (centre, neighbour) species indices of the present ones.  ValueError for a cutoff above half the smallest
    perpendicular cell height on a periodic axis (a pair could be bonded through two images)."""
    ns = _setup.neighbour_sets(packed, nb_set_and_cutoff)
    rcm, names, live = ns.cutoff, list(zip(ns.names, ns.present)), ns.live
    half = 0.5 * min_periodic_height(packed.cell, packed.pbc)
    for a, b in live:
        if rcm[a, b] > half:
            raise ValueError("cutoff %s exceeds half the smallest perpendicular cell height (%s): a pair could be bonded "
                             "through two images" % (rcm[a, b], half))
    return rcm, names, live
