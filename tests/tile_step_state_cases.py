"""Inputs of the tests of the planned tile kernel's two grid slices (rdf_tile_kernel_fast, PLAN: slice 0 runs the steps in
integer form, slice 1 the steps on f32 slab coordinates), and the CPU-side list of their steps: which form every step of an
input takes, from amof_amd/csrc/tile_plan.h through tests/native/tile_plan_driver.cpp over a slab table built as the
quantiser builds it (the method of tests/tile_ahead_cases.py).

A step = (frame, tile pair, centre sub-tile).  Its form depends on the centre sub-tile alone: f32 slab coordinates when
its 128 atoms span at most 16 of the 256 slabs of the frame, integer slab differences otherwise -- so it changes from
frame to frame with the atoms' positions.

  zif544   ZIF-4 x 1x1x2 (544 atoms: H and C 192, N 128, Zn 32) in its diagonal cell, 19 frames: the slab axis (36.8 A) is more
           than 2.1 rmax, so the plan is in use, and every sub-tile spans most of the axis: integer steps only
  lattice  tests/tile_ahead_cases.py: a perfect lattice, every distance on a bin edge -- every in-range pair goes through the
           refinement's third level; lattice_cells: the same with one (equal) cell per frame
  graded   the cell of zif544 with 2001 atoms of one species whose density along the slab axis varies by a factor of three, and
           whose dense part moves from frame to frame, next to 100 atoms of another: four tiles of the dense species (diagonal
           and off-diagonal tile pairs, the last tile ragged: 465 = 3 x 128 + 81 atoms, 1 modulo 4), sub-tiles of 8 to 24 slabs --
           both forms inside one work item, and one sub-tile in both forms in different frames of one chunk; the thin species'
           steps always in integer form
"""

import subprocess

import numpy as np

from amof_amd.frames import PackedTrajectory
from tests import helpers as H
from tests import tile_ahead_cases as T

FRAMES = 19


def default_cutoff(packed):
    rmax = float(np.min(packed.cell_lengths()) / 2)
    return rmax, int(rmax // 0.01)


def zif544():
    packed = H.random_walk(T._zif((1, 1, 2)), FRAMES, 0.05, 1400, ortho=True)
    return (packed,) + default_cutoff(packed)


def graded():
    cell = np.diag(np.diag(T._zif((1, 1, 2)).cell))
    L = np.diag(cell)
    rng = np.random.default_rng(1401)
    n_a, n_b = 2001, 100
    u = rng.uniform(0, 1, (n_a + n_b, 3))
    frames = np.empty((FRAMES, n_a + n_b, 3))
    for f in range(FRAMES):
        s = (u + rng.normal(0, 0.002, u.shape)) % 1.0
        # z = u + a sin(2 pi (u - phase)) / (2 pi): monotone for |a| < 1, density 1 / (1 + a cos(..)) -- between 2/3 and 2 of the mean
        a, phase = 0.5, 0.37 * f
        z = s[:n_a, 2]
        s[:n_a, 2] = (z + a * np.sin(2.0 * np.pi * (z - phase)) / (2.0 * np.pi)) % 1.0
        frames[f] = s * L
    numbers = np.where(np.arange(n_a + n_b) < n_a, 6, 30)
    packed = PackedTrajectory(frames, cell[None], numbers)
    return (packed,) + default_cutoff(packed)


def lattice():
    return T.lattice()[:3]


def lattice_cells():
    """the same lattice with its cell given frame by frame"""
    packed, rmax, nbins = lattice()
    cell = np.asarray(packed.cell).reshape(-1, 3, 3)[:1]
    return PackedTrajectory(np.asarray(packed.pos), np.repeat(cell, packed.pos.shape[0], axis=0), packed.numbers), rmax, nbins


TRAJECTORIES = {"zif544": zif544, "graded": graded, "lattice": lattice, "lattice_cells": lattice_cells}


def steps(packed, rmax, driver, env=None, frames=None):
    """[(tile pair, chunk, frame, sub, tile I, live, zf)] of every step of the input, in the kernel's order within a work item"""
    env = env or {}
    pos = np.asarray(packed.pos)
    if frames is not None:
        pos = pos[frames[0]:frames[1]]
    L = np.diag(np.asarray(packed.cell).reshape(-1, 3, 3)[0])
    axis = int(np.argmax(L))
    gap = int(min(4294967295.0, np.ceil(rmax / L[axis] * 4294967296.0 * (1.0 + 1e-6)) + 4.0))
    kinds, sp = H.species_of(packed.numbers)
    tiles = T.tiles_of([int((sp == s).sum()) for s in range(len(kinds))])
    pairs = [(i, j) for i in range(len(tiles)) for j in range(i, len(tiles))]
    F = pos.shape[0]
    fpc = T.frames_per_chunk(F, len(pairs), env)
    assert fpc <= 16, "the plan serves chunks of at most 16 frames"
    text, keys = [], []
    for f in range(F):
        frac = (pos[f][:, axis] / L[axis]) % 1.0
        slab = np.minimum((frac * 4294967296.0).astype(np.uint64), 4294967295) >> 24
        starts = [np.concatenate([[0], np.cumsum(np.bincount(slab[sp == s].astype(np.int64), minlength=256))]) for s in range(len(kinds))]
        prev = None
        for p, (i, j) in enumerate(pairs):
            (si, oi, ci), (sj, oj, cj) = tiles[i], tiles[j]
            if sj != prev:
                text.append("T " + " ".join(str(int(v)) for v in starts[sj]))
                prev = sj
            for sub in range((ci + T.SUB - 1) // T.SUB):
                k0, k1 = oi + sub * T.SUB, oi + min(ci, (sub + 1) * T.SUB) - 1
                s_first, s_last = (int(np.searchsorted(starts[si], k, side="right")) - 1 for k in (k0, k1))
                text.append("W %d %d %d %d %d %d %d" % (oj, cj, s_first, s_last, gap, int(i == j), sub))
                keys.append((p, f // fpc, f, sub, i))
    out = subprocess.run([driver], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[int(x) for x in l.split()] for l in out if l]
    assert len(rows) == len(keys)
    return [k + (v[1] > v[0] or v[3] > v[2], bool(v[6])) for k, v in zip(keys, rows)], tiles, pairs


def census(step_list):
    """what the two slices have to get right: counts of live steps by form, of work items (tile pair, chunk) with live steps
    of both forms, and of centre sub-tiles (tile I, sub) that take both forms in live steps of one work item"""
    live = [s for s in step_list if s[5]]
    items, subs = {}, {}
    for p, c, f, sub, ti, _, zf in live:
        items.setdefault((p, c), set()).add(zf)
        subs.setdefault((p, c, sub), set()).add(zf)
    return {"zf": sum(1 for s in live if s[6]), "integer": sum(1 for s in live if not s[6]),
            "dead": len(step_list) - len(live),
            "mixed_items": sum(1 for v in items.values() if len(v) == 2),
            "zf_only_items": sum(1 for v in items.values() if v == {True}),
            "integer_only_items": sum(1 for v in items.values() if v == {False}),
            "sub_in_both_forms": sum(1 for v in subs.values() if len(v) == 2)}
