"""The saturating tail of the planned f32-slab slice of the RDF tile kernel (amof_amd/csrc/rdf_sat_math.h: the functions the
kernel runs, here compiled with g++ through tests/native/tile_sat_driver.cpp) against the exact f64 distance of the same
fixed-point differences.  For random differences and for adversarial ones -- slab coordinates at the ends of the window the
f32 form admits, q around nbins, around 1 and around every lane's clamp value, coincident atoms, the largest differences,
every lane -- and with the root one ulp either side of sqrtf (v_sqrt_f32's accuracy):

  |q' - (q + 1 + g)| <= fast_guard_zf_sat        for every pair that does not saturate, q <= nbins + 1
  the counter of an unflagged pair is word floor(q) + 1; an unflagged pair out of range is counted behind the histogram
  a saturated pair lands in its lane's trash word, unflagged, and is out of range by a quarter of a bin at least
  no counter lies outside the words [1, nbins + 32] that the workgroup's LDS allocation holds (tile_lds)
The same test prints the flagged and in-range counts of its samples (uniform in q, with the adversarial ones: not a
trajectory's share).  The selection's side -- the thresholds' rounding, the switch, the LDS size with the pad word -- is asked of
rdf_select.h through tests/native/tile_sat_select_driver.cpp.
"""

import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_sat_driver.cpp")
SELECT_SRC = os.path.join(ROOT, "tests", "native", "tile_sat_select_driver.cpp")

# name: (cell lengths with the slab axis last, rmax, nbins)
CELLS = {
    "zif4_2x2x2": ((30.79, 30.62, 36.85), 15.31, 1531),
    "headline_2310": ((46.19, 45.93, 73.7), 23.1, 2310),           # a guard of the headline's size, every low bit of C in play
    "coarse_31": ((30.79, 30.62, 36.85), 15.31, 31),
    "long_axis": ((12.0, 12.0, 36.0), 6.0, 600),                  # the lattice of tests/tile_ahead_cases.py
    "fine_20000": ((30.79, 30.62, 80.0), 15.0, 20000),
}


def _build(tmp, flags, name, src=SRC):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [src, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _line(name, samples, seed):
    (lx, ly, lz), rmax, nb = CELLS[name]
    dr = rmax / nb
    two32 = 4294967296.0
    gfrac = (min(4294967295.0, -(-rmax / lz * two32 * (1.0 + 1e-6) // 1) + 4.0)) / two32          # cull_gap (rdf_select.h)
    guard_m = (lx + ly + lz) / 2147483648.0 / dr + nb * 1e-12
    return "%d %.17g %.17g %.17g %.17g %.17g %d %d" % (nb, lx / two32 / dr, ly / two32 / dr, lz / two32 / dr, gfrac, guard_m, samples, seed)


def _ask(exe, lines, timeout=300):
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    rows = [l.split() for l in r.stdout.strip().splitlines()]
    assert len(rows) == len(lines)
    keys = ("pairs", "in_range", "flagged", "saturated", "bad_bound", "bad_word", "bad_trash", "bad_lds")
    return [dict(zip(keys, (int(x) for x in w[:8])), max_ratio=float(w[8]), bound=float(w[9]), guard=float(w[10])) for w in rows]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("tile_sat"), ["-O2"], "tile_sat_driver")


@pytest.mark.parametrize("name", list(CELLS))
def test_chain_stays_inside_its_guard(driver, name):
    got = _ask(driver, [_line(name, 400000, 1500 + len(name))])[0]
    print(name, got)
    assert got["pairs"] > 1000000 and got["in_range"] > 0 and got["flagged"] > 0 and got["saturated"] > 0, got
    assert got["guard"] < 0.25
    assert got["bad_bound"] == 0 and got["max_ratio"] <= 1.0, got
    assert got["bad_word"] == 0 and got["bad_trash"] == 0 and got["bad_lds"] == 0, got


def test_selection_thresholds_switch_and_lds(tmp_path_factory):
    exe = _build(tmp_path_factory.mktemp("tile_sat_select"), ["-O1"], "tile_sat_select_driver", SELECT_SRC)
    lines, keys = [], []
    for name, ((lx, ly, lz), rmax, nb) in CELLS.items():
        for nosat in (0, 1):
            lines.append("%d %.17g %d 1 %.17g %.17g %.17g" % (nb, rmax, nosat, lx, ly, lz))
            keys.append((name, nb, nosat))
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    rows = [l.split() for l in r.stdout.strip().splitlines()]
    assert len(rows) == len(keys)
    for (name, nb, nosat), w in zip(keys, rows):
        zf, cull, sat = (int(x) for x in w[:3])
        g = float(w[3])
        one_p, two, two_below = (float(np.float32(x)) for x in w[4:7])          # (nine digits name a float32 uniquely)
        lds, lds_sat = int(w[7]), int(w[8])
        assert (zf, cull, sat) == (1, 1, 1 - nosat), (name, nosat, w)
        assert 0.0 < g < 0.25
        # 1 + g to nearest (its rounding is a term of the bound), 2 g never undercut
        assert one_p == float(np.float32(1.0 + g)) and two >= 2.0 * g > two_below, (name, w)
        # one more word, padded to 16 bytes: bin nbins - 1 and the 32 trash words end at word nbins + 32
        assert lds_sat - lds in (0, 16) and lds_sat - 2 * 512 * 16 >= 4 * (nb + 33), (name, w)
        if nb == 2310:
            assert lds_sat == 25776 and 6 * lds_sat <= 160 * 1024


def test_driver_under_sanitizers(tmp_path_factory):
    san = _build(tmp_path_factory.mktemp("tile_sat_san"), ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                 "tile_sat_driver_san")
    r = subprocess.run([san], input="\n".join(_line(n, 20000, 7) for n in CELLS) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
