"""Step statistics of the slab-culled tile kernel on the bench system, on the CPU: how many (tile pair, sub-tile) steps of a
frame visit no quad, few quads, and the mean.  The fixture ZIF-4 x 3x3x4 (9792 atoms), intact and with every atom displaced
by a Gaussian (2.5 A by default), slab-sorted as the quantiser does it, tiles as build_tiles(.., 512, 128) makes them, windows
by amof_amd/csrc/tile_plan.h through tests/native/tile_plan_driver.cpp (built with g++ into a temporary directory).

    python3 profiles/tools/tile_plan_steps.py [sigma]
"""
import os
import subprocess
import sys
import tempfile

import numpy as np

sys.path.insert(0, os.getcwd())
from tests import helpers as H          # noqa: E402

TILE, SUB = 512, 128


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


def main():
    sigma = float(sys.argv[1]) if len(sys.argv) > 1 else 2.5
    base = H.replicate(H.zif4_frame(), (3, 3, 4))
    L = np.diag(base.cell)
    axis = int(np.argmax(L))
    rmax = float(np.min(L) / 2)
    gap = int(min(4294967295.0, np.ceil(rmax / L[axis] * 4294967296.0 * (1.0 + 1e-6)) + 4.0))
    kinds, sp = H.species_of(base.numbers)
    nsp = [int((sp == s).sum()) for s in range(len(kinds))]
    tiles = tiles_of(nsp)
    pairs = [(i, j) for i in range(len(tiles)) for j in range(i, len(tiles))]
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "tile_plan_driver")
    subprocess.check_call(["g++", "-std=c++17", "-O1", os.path.join("tests", "native", "tile_plan_driver.cpp"), "-o", exe])
    rng = np.random.default_rng(1)
    for name, pos in (("intact", base.positions), ("sigma %.1f A" % sigma, base.positions + rng.normal(0, sigma, base.positions.shape))):
        frac = (pos[:, axis] / L[axis]) % 1.0
        slab = np.minimum((frac * 4294967296.0).astype(np.uint64), 4294967295) >> 24
        starts = [np.concatenate([[0], np.cumsum(np.bincount(slab[sp == s].astype(np.int64), minlength=256))]) for s in range(len(kinds))]
        text, prev = [], None
        for i, j in pairs:
            (si, oi, ci), (sj, oj, cj) = tiles[i], tiles[j]
            if sj != prev:
                text.append("T " + " ".join(str(int(v)) for v in starts[sj]))
                prev = sj
            for sub in range((ci + SUB - 1) // SUB):
                k0, k1 = oi + sub * SUB, oi + min(ci, (sub + 1) * SUB) - 1
                s_first, s_last = (int(np.searchsorted(starts[si], k, side="right")) - 1 for k in (k0, k1))
                text.append("W %d %d %d %d %d %d %d" % (oj, cj, s_first, s_last, gap, int(i == j), sub))
        out = subprocess.run([exe], input="\n".join(text) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        quads = np.array([(max(0, v[1] - v[0]) + max(0, v[3] - v[2])) // 4 for v in ([int(x) for x in l.split()] for l in out if l)])
        print("%-14s steps %d  dead %d (%.1f %%)  1..15 quads %d  mean %.1f of 128 quads  reach 2 G / L = %.3f" % (
            name, len(quads), int((quads == 0).sum()), 100.0 * (quads == 0).mean(), int(((quads > 0) & (quads < 16)).sum()),
            quads.mean(), 2.0 * gap / 4294967296.0))


if __name__ == "__main__":
    main()
