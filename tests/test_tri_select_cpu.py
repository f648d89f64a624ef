"""The selection of the general-cell tile kernel's variant has one definition (amof_amd/csrc/tri_select.h, here through
tests/native/tri_select_driver.cpp): the table of cells in tests/tri_plant.py, one per reachable (code, culling), is
pinned to it on the CPU -- code, stored axes, culling, at every bin count the GPU test uses -- and so is the numpy
restatement the planting works from (lower factor, folds, thresholds).  Then the planting itself: where every planted
pair landed relative to its image decision is recomputed in float64 from the positions alone, and per case and category
at least 100 pairs lie within 1e-3 of the cell of the decision, at least 20 on either side."""

import os
import subprocess

import numpy as np
import pytest

from oracle import clib
from tests import edge_plant as E
from tests import tri_plant as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tri_select_driver.cpp")


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("ts")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O1"], "tri_select_driver")


def _line(cells, rmax, nbins, nohalf=False):
    c = np.asarray(cells, dtype=np.float64).reshape(-1, 9)
    return "C %d %d %.17g %d %s" % (int(nohalf), nbins, rmax, len(c), " ".join("%.17g" % v for v in c.ravel()))


def _ask(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    out = []
    for l in r.stdout.strip().splitlines():
        w = l.split()
        out.append(dict(ok=w[0] == "1", sel=tuple(int(x) for x in w[1:6]), share=float(w[6]), l10_bins=float(w[7]),
                        c10=float(w[8]), tau=float(w[9]), guard_f=float(w[10]), rec=np.array([float(x) for x in w[12:]]).reshape(-1, 9)))
    return out


def _all_nbins(name):
    return T.NBINS + ((T.NBINS_BIG[name],) if name in T.NBINS_BIG else ())


@pytest.fixture(scope="module")
def table(driver):
    keys = [(name, nb) for name in T.CASES for nb in _all_nbins(name)]
    got = _ask(driver, [_line(T.case_cells(n), T.case_rmax(n), nb, T.CASES[n].get("nohalf", False)) for n, nb in keys])
    return dict(zip(keys, got))


def test_every_cell_selects_its_variant(table):
    for (name, nb), g in table.items():
        assert g["ok"] and g["sel"] == T.CASES[name]["expect"], (name, nb, g["ok"], g["sel"])


def test_every_reachable_variant_has_a_cell():
    """(code, culling) as the selection takes them by itself; AMOF_RDF_NOCULL=1 gives the unculled form of the rest.
    3 and 8 (near tests along the slab axis) never come with culling: a second image along z in range, rmax > h / 2,
    contradicts 2 * 1.05 * rmax < h.  Every other code comes both ways (4 unculled: a long x axis under a strongly tilted
    third vector, so that every perpendicular height stays below 2.1 rmax)."""
    have = {(c["expect"][0], c["expect"][4]) for c in T.CASES.values()}
    want = {(code, cull) for code in (0, 1, 2, 4, 5, 6, 7, 9, 10, 11) for cull in (0, 1)} | {(3, 0), (8, 0)}
    assert have == want, (sorted(want - have), sorted(have - want))
    assert sum(T.case_cells(n).shape[0] > 1 for n in T.CASES) == 3
    assert sum(T.CASES[n]["rmax"] is None for n in T.CASES) >= 8        # the reference's default cutoff, float64


def test_guard_band_cells_take_the_plainest_variant(driver):
    """the two cells of tests/test_gpu_guard_band.py: code 0 with culling, at every bin count used there"""
    sheared = [[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 29.53]]
    high_kappa = [[31.7, 0.0, 0.0], [0.0, 29.3, 0.0], [83.1, 79.7, 30.9]]
    lines = [_line(sheared, 6.5, nb) for nb in (7, 999, 2310, 31744)] + [_line(high_kappa, 4.2, nb) for nb in (2310, 31744)]
    for g in _ask(driver, lines):
        assert g["ok"] and g["sel"][0] == 0 and g["sel"][4] == 1, g["sel"]


def test_switch_and_refusals(driver):
    hexc = T.CASES["c11_on"]["cell"]
    rm = T.case_rmax("c11_on")
    a, b = _ask(driver, [_line(hexc, rm, 999), _line(hexc, rm, 999, nohalf=True)])
    assert a["sel"][0] == 11 and b["sel"][0] == 9 and a["sel"][1:] == b["sel"][1:]
    assert np.array_equal(a["rec"], b["rec"])
    # beyond half the x axis the variant is refused; a skewed, non-reduced cell cannot take the integer x wrap
    big, skew = _ask(driver, [_line(hexc, 1.01 * rm, 800), _line([[5.0, 0, 0], [20.0, 7.0, 0], [0, 0, 30.0]], 2.4, 240)])
    assert not big["ok"] and not skew["ok"]


def test_numpy_restatement_equals_the_header(table):
    """what the planting takes from the selection -- L, the folds, the thresholds -- against the header's records"""
    for (name, nb), g in table.items():
        sts, band = T.stored_frames(name, nb)
        assert band == pytest.approx(g["guard_f"], rel=1e-9), (name, nb)
        assert len(sts) == len(g["rec"])
        for st, rec in zip(sts, g["rec"]):
            mine = st.rec()
            fin = np.isfinite(rec)
            assert np.array_equal(np.isfinite(mine), fin), (name, nb, mine, rec)
            assert np.allclose(mine[fin], rec[fin], rtol=1e-11, atol=1e-13), (name, nb, mine, rec)


def test_npt_cells_breathe_across_the_y_threshold(table):
    for name in T.CASES:
        if T.case_cells(name).shape[0] == 1:
            continue
        for nb in T.NBINS:
            thr = table[(name, nb)]["rec"][:, 4]
            assert np.isinf(thr).any() and np.isfinite(thr).any(), (name, nb, thr)


@pytest.mark.parametrize("name", list(T.CASES))
def test_planted_pairs_land_on_their_decisions(name):
    for nb in _all_nbins(name):
        pl = T.plant_tri(name, nb, seed=nb)
        sts, _ = T.stored_frames(name, nb)
        cats = T.categories(name, sts, T.CASES[name]["rmax"] is None)
        code = T.CASES[name]["expect"][0]
        assert "c" in cats and ("d" in cats) == (code in (4, 9, 10, 11)) and ("b" in cats) == (code in (3, 8))
        assert ("a" in cats) == (code in (1, 2, 3, 6, 7, 8) and any(np.isfinite(s.thr_y) for s in sts))
        assert "a" in cats or code not in (2, 7)
        counts = pl.counts()
        print(name, nb, counts)
        # "cx", the x wrap without the y term, is the decision the codes below 5 make: a floor of its own there
        cx = counts.pop("cx")
        assert sorted(counts) == cats
        if code < 5:
            counts["cx"] = cx
        for c, (within, below, above) in counts.items():
            assert within >= 100 and below >= 20 and above >= 20, (name, nb, c, within, below, above)
        assert pl.packed.pos.shape[1] == 2400 and pl.packed.pos.shape[0] in (2, 3)
        # no species pair idle, on the very trajectory the GPU test runs (the single atom of the fifth species has no
        # partner of its own kind: that entry alone is empty)
        kinds, sp = E._species(pl.packed.numbers)
        assert len(kinds) == 5 and min(np.bincount(sp)) == 1
        ref, _ = clib.rdf_hist(pl.packed.pos, pl.packed.cell, sp, len(kinds), T.case_rmax(name), nb, cell_list=True)
        per_pair = ref.sum(axis=2).astype(np.int64)
        single = int(np.argmin(np.bincount(sp)))
        assert per_pair[single, single] == 0
        per_pair[single, single] = 1
        assert per_pair.min() > 0, (name, nb, per_pair)


def test_realised_offsets_notice_a_planting_off_its_decision():
    """the floor check is not vacuous: pairs moved by 0.3 % of the cell are out of every window"""
    pl = T.plant_tri("c3_off", 999, seed=1)
    for f in range(pl.packed.pos.shape[0]):
        pl.packed.pos[f, pl.j[pl.frame == f]] += 0.003 * T.case_cells("c3_off")[0].sum(axis=0)
    assert all(v[0] < 100 for v in pl.counts().values())      # ("cx" included)


def test_driver_under_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "tri_select_driver_san")
    lines = [_line(T.case_cells(n), T.case_rmax(n), nb, T.CASES[n].get("nohalf", False)) for n in T.CASES for nb in (7, 2310)]
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
