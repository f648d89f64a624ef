"""Inputs of the tests of the plan kernel's read-ahead (rdf_tile_kernel_fast, AHEAD; AMOF_RDF_NOAHEAD), and the CPU-side
classification of their steps: which window classes the read-ahead has to get right occur in which input.

A step = (frame, tile pair, centre sub-tile); its partner window (two pieces of whole quads, dealt to the four waves by
quad index modulo four from the piece's first quad) comes from amof_amd/csrc/tile_plan.h through
tests/native/tile_plan_driver.cpp, over a slab table built as the quantiser builds it -- the method of
profiles/tools/tile_plan_steps.py.  Classes, per piece of a live step:
  empty_for_a_wave  1 .. 3 quads: a window of fewer than 16 partners, some wave has no quad in it and must read nothing
  ragged_tail       the piece ends with the tile's ragged last quad (count not a multiple of 4)
  tail_behind_plain ... and the wave that takes that quad has a plain quad in front of it
  own_plain_tail    a diagonal tile pair's piece runs from the own block through plain quads into the ragged quad
  two_pieces        both pieces have quads (wrapped reach); first_sub / last_sub: for the first / last sub-tile of a tile
  dead_between      a dead step between two live ones of the same work item and chunk (the step ahead is not s + 1)
  dead_frame        a frame without a live step between two frames with one
  zf / integer      steps on f32 slab coordinates / on integer slab differences; zf_int_zf and int_zf_int: such chains among
                    the live steps of one work item and chunk
"""

import os
import subprocess

import numpy as np

from amof_amd.frames import Frame, PackedTrajectory
from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER_SRC = os.path.join(ROOT, "tests", "native", "tile_plan_driver.cpp")
TILE, SUB = 512, 128

# the switch: the kernel without the read-ahead, and with it (the default)
SETTINGS = (("off", {"AMOF_RDF_NOAHEAD": "1"}), ("ahead", {}))


def build_driver(tmpdir):
    exe = os.path.join(str(tmpdir), "tile_plan_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", DRIVER_SRC, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def tiles_of(nsp):
    """(species, offset in the species segment, count) as build_tiles(t, 512, out, 128)"""
    out = []
    for s, n in enumerate(nsp):
        nt, ng = (n + TILE - 1) // TILE, (n + SUB - 1) // SUB
        off = 0
        for k in range(nt):
            cnt = min((ng // nt + (1 if k < ng % nt else 0)) * SUB, n - off)
            out.append((s, off, cnt))
            off += cnt
    return out


def frames_per_chunk(nf, npairs, env):
    """the host's choice (rdf.hip): ~80k workgroups per launch, between 2 and 16 frames"""
    fpc = max(2, min((nf * npairs + 40000) // 80000, 16))
    if "AMOF_RDF_FPC" in env:
        fpc = max(1, int(env["AMOF_RDF_FPC"]))
    fpc = min(fpc, max(1, nf))
    if nf >= 64:
        fpc = min(fpc, nf // 32)
    return fpc


def classify(packed, rmax, driver, env=None):
    """window classes of the whole input: {class: number of steps (pieces, chains) that show it}"""
    env = env or {}
    pos = np.asarray(packed.pos)
    L = np.diag(np.asarray(packed.cell).reshape(-1, 3, 3)[0])
    axis = int(np.argmax(L))
    gap = int(min(4294967295.0, np.ceil(rmax / L[axis] * 4294967296.0 * (1.0 + 1e-6)) + 4.0))
    kinds, sp = H.species_of(packed.numbers)
    nsp = [int((sp == s).sum()) for s in range(len(kinds))]
    tiles = tiles_of(nsp)
    pairs = [(i, j) for i in range(len(tiles)) for j in range(i, len(tiles))]
    F = pos.shape[0]
    fpc = frames_per_chunk(F, len(pairs), env)
    assert fpc <= 64 // 4, "the plan serves chunks of at most 16 frames"
    text, keys, prev = [], [], None
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
            nsub = (ci + SUB - 1) // SUB
            for sub in range(nsub):
                k0, k1 = oi + sub * SUB, oi + min(ci, (sub + 1) * SUB) - 1
                s_first, s_last = (int(np.searchsorted(starts[si], k, side="right")) - 1 for k in (k0, k1))
                text.append("W %d %d %d %d %d %d %d" % (oj, cj, s_first, s_last, gap, int(i == j), sub))
                keys.append((p, f, sub, nsub, cj, i == j))
    out = subprocess.run([driver], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [[int(x) for x in l.split()] for l in out if l]
    assert len(rows) == len(keys)
    c = dict.fromkeys(("steps", "live", "dead", "empty_for_a_wave", "ragged_tail", "tail_behind_plain", "own_plain_tail",
                       "two_pieces", "two_pieces_first_sub", "two_pieces_last_sub", "dead_between", "dead_frame", "zf", "integer",
                       "zf_int_zf", "int_zf_int"), 0)
    seq = {}                                     # (pair, chunk) -> [(frame, live, zf)] in step order
    for (p, f, sub, nsub, cj, diag), v in zip(keys, rows):
        qb, qe, zf = (v[0], v[2]), (v[1], v[3]), v[6]
        n = [max(0, qe[r] - qb[r]) // 4 for r in range(2)]
        live = n[0] + n[1] > 0
        c["steps"] += 1
        c["live" if live else "dead"] += 1
        seq.setdefault((p, f // fpc), []).append((f, live, zf))
        if not live:
            continue
        c["zf" if zf else "integer"] += 1
        full = cj & ~3
        for r in range(2):
            if n[r] == 0:
                continue
            if n[r] < 4:
                c["empty_for_a_wave"] += 1
            if full < cj and qe[r] > full:
                c["ragged_tail"] += 1
                # the wave of the ragged quad: residue of (full - qb) / 4 modulo four; a plain quad of its own in front of it
                own_end = min(qe[r], (sub + 1) * SUB) if diag else 0
                mine = [j for j in range(qb[r] + 4 * (((full - qb[r]) // 4) % 4), full, 16)]
                if any(j >= own_end for j in mine):
                    c["tail_behind_plain"] += 1
                    if any(j < own_end for j in mine):
                        c["own_plain_tail"] += 1
        if n[0] and n[1]:
            c["two_pieces"] += 1
            c["two_pieces_first_sub"] += int(sub == 0)
            c["two_pieces_last_sub"] += int(sub == nsub - 1)
    for steps in seq.values():
        lv = [s[1] for s in steps]
        if True in lv:
            a, b = lv.index(True), len(lv) - 1 - lv[::-1].index(True)
            c["dead_between"] += lv[a:b + 1].count(False)
            fr = sorted(set(s[0] for s in steps))
            alive = [any(s[1] for s in steps if s[0] == f) for f in fr]
            a, b = alive.index(True), len(alive) - 1 - alive[::-1].index(True)
            c["dead_frame"] += alive[a:b + 1].count(False)
        kinds_live = "".join("z" if s[2] else "i" for s in steps if s[1])
        c["zf_int_zf"] += int("ziz" in kinds_live)
        c["int_zf_int"] += int("izi" in kinds_live)
    return c


def _delete(frame, k):
    """the frame without the last k atoms of every species: counts = 0 - k modulo 4 where they were multiples of 4"""
    keep = np.ones(len(frame.numbers), dtype=bool)
    for z in set(int(x) for x in frame.numbers):
        keep[np.nonzero(frame.numbers == z)[0][-k:]] = False
    return Frame(frame.numbers[keep], frame.positions[keep], frame.cell, frame.pbc)


def _zif(reps):
    base = H.replicate(H.zif4_frame(), reps)
    return Frame(base.numbers, base.positions, np.diag(np.diag(base.cell)), base.pbc)


def _default(packed):
    rmax = float(np.min(packed.cell_lengths()) / 2)
    return rmax, int(rmax // 0.01)


def base():
    """ZIF-4 x 2x2x4 (4352 atoms: H and C three tiles each, N two, Zn one of 256), reach 0.42, 20 frames in two chunks of 10: a
    chunk end and frame changes inside a chunk.  (Its sub-tiles span more than 16 slabs: every step runs on integer slab
    differences; the steps on f32 slab coordinates and the chains of both kinds are in `long_cell`, `mix` and `lattice`.)"""
    packed = H.random_walk(_zif((2, 2, 4)), 20, 0.05, 901, ortho=True)
    return (packed,) + _default(packed) + ({"AMOF_RDF_FPC": "10"},)


def deleted(k):
    """the same system without k atoms of every species (counts = 3, 2, 1 modulo 4 for k = 1, 2, 3): ragged tail quads"""
    packed = H.random_walk(_delete(_zif((2, 2, 4)), k), 4, 0.05, 910 + k, ortho=True)
    return (packed,) + _default(packed) + ({},)


def long_cell():
    """ZIF-4 x 2x2x6 (6528 atoms), reach 0.28: dead steps and frames, windows of fewer than 16 partners; one atom of every
    species deleted (ragged tails in short windows)"""
    packed = H.random_walk(_delete(_zif((2, 2, 6)), 1), 4, 0.05, 920, ortho=True)
    return (packed,) + _default(packed) + ({},)


def mix():
    """ZIF-4 x 2x2x6 with 140 H and 141 C atoms taken out at random: their sub-tiles span 15 to 17 slabs, on both sides of the
    16 slabs up to which a step runs on f32 slab coordinates -- ZF and integer steps alternate inside a work item"""
    fr = _zif((2, 2, 6))
    rng = np.random.default_rng(7)
    keep = np.ones(len(fr.numbers), dtype=bool)
    for z in (1, 6):
        keep[rng.choice(np.nonzero(fr.numbers == z)[0], 140 + (1 if z == 6 else 0), replace=False)] = False
    packed = H.random_walk(Frame(fr.numbers[keep], fr.positions[keep], fr.cell, fr.pbc), 4, 0.05, 940, ortho=True)
    return (packed,) + _default(packed) + ({},)


def layers():
    """2100 uniform atoms along a 96 A axis (five tiles: pairs two apart have no live step) and 300 atoms in a 4 A layer that
    sits elsewhere in the middle frame: work items go live -> dead -> live, frames without a live step between live ones"""
    rng = np.random.default_rng(2100)
    box = np.array([14.0, 15.0, 96.0])
    n_a, n_b = 2100, 300
    pos = rng.uniform(0, 1, (n_a + n_b, 3)) * box
    pos[n_a:, 2] = 20.0 + rng.uniform(0, 4.0, n_b)
    mid = pos + rng.normal(0, 0.05, pos.shape)
    mid[n_a:, 2] += 50.0
    frames = np.stack([pos, mid, pos + np.array([0.0, 0.0, 0.5 * box[2]]), pos + 0.1])
    numbers = np.where(np.arange(n_a + n_b) < n_a, 6, 30)
    return PackedTrajectory(frames, np.diag(box), numbers), 7.0, 700, {"AMOF_RDF_FPC": "4"}


def wrapped():
    """ZIF-4 x 1x1x4 (1088 atoms, every species one tile, three of each with several sub-tiles), each frame displaced along
    the slab axis by another share of the cell: the windows of the first and the last sub-tile wrap into two pieces"""
    frame = _delete(_zif((1, 1, 4)), 1)
    walk = H.random_walk(frame, 6, 0.05, 930, wrap=False, ortho=True)
    Lz = float(np.diag(frame.cell)[2])
    pos = np.asarray(walk.pos).copy()
    for f, share in enumerate((0.0, 0.5, 0.13, 0.77, 0.31, 0.94)):
        pos[f, :, 2] += share * Lz
    cell = np.diag(np.diag(frame.cell))
    s = pos @ np.linalg.inv(cell)
    pos = (s - np.floor(s)) @ cell
    packed = PackedTrajectory(pos, cell[None], frame.numbers, pbc=frame.pbc)
    return (packed,) + _default(packed) + ({},)


def lattice():
    """a perfect lattice in a long box, every distance on a bin edge: every in-range pair is flagged, the lanes' queues
    overflow and the slow path reads partner records from LDS while a quad read ahead is in flight"""
    a, n = 2.0, (6, 6, 18)
    pos = np.array([[x, y, z] for x in range(n[0]) for y in range(n[1]) for z in range(n[2])], dtype=float) * a
    numbers = np.where(np.arange(len(pos)) % 5 == 0, 30, np.where(np.arange(len(pos)) % 2 == 0, 7, 6))
    keep = np.ones(len(pos), dtype=bool)
    keep[[3, 4, 10]] = False             # (species counts off the multiples of four)
    pos, numbers = pos[keep], numbers[keep]
    cell = np.diag([n[0] * a, n[1] * a, n[2] * a])
    frames = np.stack([pos, pos + 0.25, pos + np.array([0.0, 0.0, 0.5 * n[2] * a])])
    return PackedTrajectory(frames, cell, numbers), 6.0, 600, {}


CASES = {
    "base": base,
    "deleted1": lambda: deleted(1),
    "deleted2": lambda: deleted(2),
    "deleted3": lambda: deleted(3),
    "long_cell": long_cell,
    "mix": mix,
    "layers": layers,
    "wrapped": wrapped,
    "lattice": lattice,
}

# classes every input must show (tests/test_tile_ahead_cpu.py checks them before any GPU run)
REQUIRED = {
    "base": ("integer", "dead_between", "two_pieces", "empty_for_a_wave"),
    "deleted1": ("ragged_tail", "tail_behind_plain", "own_plain_tail"),
    "deleted2": ("ragged_tail", "tail_behind_plain", "own_plain_tail"),
    "deleted3": ("ragged_tail", "tail_behind_plain", "own_plain_tail"),
    "long_cell": ("zf", "integer", "dead", "dead_between", "empty_for_a_wave", "ragged_tail", "tail_behind_plain", "own_plain_tail"),
    "mix": ("zf", "integer", "zf_int_zf", "int_zf_int", "dead_between", "empty_for_a_wave", "ragged_tail"),
    "layers": ("dead", "dead_between", "dead_frame"),
    "wrapped": ("two_pieces", "two_pieces_first_sub", "two_pieces_last_sub", "ragged_tail"),
    "lattice": ("zf",),
}
LONG_CELL_COUNTS = (14, 208)      # (pieces of fewer than 16 partners, ragged last quads) of `long_cell`
