"""The host decisions of the RDF entry point have one definition (amof_amd/csrc/rdf_select.h, here through
tests/native/rdf_select_driver.cpp): the f32 thresholds with directed rounding, the tile kernel's chunk rule, the
per-cell scale records and the selection of the kernel family -- pinned on the CPU for the very cells and cutoffs whose
GPU tests assert a path (tests/helpers.py: rdf_path_case).  The same driver runs once more under the address and
undefined-behaviour sanitizers."""

import os
import subprocess

import numpy as np
import pytest

from tests import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "rdf_select_driver.cpp")
MAX_BINS = 36864 - 5120                 # AMOF_MAX_LDS_BINS - 5120 (include/amof_hip.h)
SELECT_KEYS = ("plain", "img", "tri", "zf", "cull", "cell", "range", "axis", "nz2", "axis_y", "gy", "nk0", "nk1", "nk2")


def _build(tmp, flags, name):
    out = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++17", "-ffp-contract=off"] + flags + [SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("rs")


@pytest.fixture(scope="module")
def driver(tmp):
    return _build(tmp, ["-O1"], "rdf_select_driver")


def _ask(driver, lines, timeout=120):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == len(lines)
    return [l.split() for l in out]


# ---- guard_thresholds ----
def _guard_lines():
    guards = [1e-7, 3.3e-7, 1e-5, 1.234e-3, 0.01, 0.1, 0.2, 0.249]
    return [(nb, g) for nb in (1, 60, 2310, MAX_BINS) for g in guards]


def test_guard_thresholds_round_away_from_the_bound(driver):
    cases = _guard_lines()
    for (nb, g), w in zip(cases, _ask(driver, ["G %d %.17g" % c for c in cases])):
        hi, hi_below, half, half_above = (float(x) for x in w)
        assert hi == np.float32(hi) and half == np.float32(half)
        assert hi >= nb + g and hi_below < nb + g, (nb, g, hi, hi_below)
        assert half <= 0.5 - g and half_above > 0.5 - g, (nb, g, half, half_above)


# ---- tile_chunks ----
def _chunk_cases():
    return [(nf, npairs) for nf in list(range(1, 601)) + [625, 4999, 5000, 5003] for npairs in (1, 3, 10, 55, 210)]


def _chunk_lines(cases, fpc=0, notail=0):
    return ["T %d %d %d %d" % (nf, npairs, fpc, notail) for nf, npairs in cases]


def test_tile_chunks_cover_every_frame(driver):
    cases = _chunk_cases()
    seen = {"xcd": 0, "flat": 0, "tail": 0, "plan": 0, "noplan": 0}
    for (nf, npairs), w in zip(cases, _ask(driver, _chunk_lines(cases))):
        fpc, chunks, xcd_map, nf_tail, nf_main, plan_fits = (int(x) for x in w)
        ctx = (nf, npairs, w)
        assert nf_main + nf_tail == nf and fpc * chunks >= nf_main, ctx
        assert 1 <= fpc <= 16, ctx
        unpadded = -(-nf // fpc)
        assert xcd_map == int(unpadded >= 32), ctx
        if xcd_map:
            assert chunks % 8 == 0 and nf_main % 8 == 0, ctx
        else:
            assert nf_tail == 0 and chunks == unpadded, ctx
        # frames [c nf_main / chunks, (c + 1) nf_main / chunks) belong to chunk c: at most ceil(nf_main / chunks) of them
        per_item = -(-nf_main // chunks)
        if plan_fits:
            assert per_item <= 16, ctx
        seen["xcd"] += xcd_map
        seen["flat"] += not xcd_map
        seen["tail"] += nf_tail > 0
        seen["plan"] += plan_fits
        seen["noplan"] += not plan_fits
    assert min(seen[k] for k in ("xcd", "flat", "tail", "plan")) > 0, seen


def test_tile_chunks_switches(driver):
    cases = [(nf, 10) for nf in (1, 7, 63, 64, 100, 625, 5003)]
    for (nf, _), w in zip(cases, _ask(driver, _chunk_lines(cases, notail=1))):
        fpc, chunks, xcd_map, nf_tail, nf_main, _ = (int(x) for x in w)
        assert nf_tail == 0 and nf_main == nf and fpc * chunks >= nf, (nf, w)
    # AMOF_RDF_FPC names the frames per chunk, capped by the batch; beyond 16 frames a work item holds no plan
    for (nf, _), w in zip(cases, _ask(driver, _chunk_lines(cases, fpc=40))):
        fpc, chunks, xcd_map, nf_tail, nf_main, plan_fits = (int(x) for x in w)
        assert fpc == (min(40, nf) if nf < 64 else min(40, nf // 32)) and fpc * chunks >= nf_main, (nf, w)
        assert plan_fits == int(-(-nf_main // chunks) <= 16), (nf, w)


# ---- fill_frame_scales ----
def _fill(driver, ortho, ord_, dr, cell):
    w = _ask(driver, ["F %d %d %d %d %.17g %s" % (int(ortho), ord_[0], ord_[1], ord_[2], dr, " ".join("%.17g" % v for v in np.ravel(cell)))])[0]
    v = np.array([float(x) for x in w])
    return v[:9], v[9:].astype(np.float32)      # (nine digits name a float32 uniquely)


ORDERS = ((1, 2, 0), (0, 1, 2), (0, 2, 1))      # tile tier with slab axis 0 | cell tier | range tier (axis 1, axis_y 2)


def test_fill_frame_scales_diagonal_cell_as_general(driver):
    lengths, dr = np.array([30.8, 27.3, 55.3]), 0.01
    for ord_ in ORDERS + ((2, 0, 1),):
        s_o, f_o = _fill(driver, True, ord_, dr, np.diag(lengths))
        s_g, f_g = _fill(driver, False, ord_, dr, np.diag(lengths))
        want = lengths[list(ord_)] / 4294967296.0 / dr
        assert np.allclose(s_o[:3], want, rtol=1e-15, atol=0) and not s_o[3:].any()
        # the ortho form keeps the scales in [0..2]; the general form is the lower factor: the same numbers on its diagonal
        assert np.allclose(s_g[[0, 4, 8]], s_o[:3], rtol=1e-15, atol=0) and not s_g[[1, 2, 3, 5, 6, 7]].any()
        assert np.array_equal(f_o[:3], np.float32(s_o[:3])) and np.array_equal(f_o[3:6], np.float32(s_o[:3] ** 2))
        assert np.array_equal(f_g, np.float32(s_g))


def test_fill_frame_scales_axis_orders_permute_the_rows(driver):
    cell = np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 29.53]])
    dr = 0.0125
    for ord_ in ORDERS:
        s, f = _fill(driver, False, ord_, dr, cell)
        L = s.reshape(3, 3)
        rows = cell[list(ord_)] / 4294967296.0 / dr
        assert np.allclose(L @ L.T, rows @ rows.T, rtol=1e-12, atol=0), ord_        # the metric of the rows in stored order
        assert not L[np.triu_indices(3, 1)].any() and (np.diag(L) > 0).all()
        assert np.array_equal(f, np.float32(s))


# ---- the selection ----
def _select_line(packed, rmax, nb, switches=(), pbc=(1, 1, 1), max_img=0):
    _, sp = H.species_of(packed.numbers)
    nsp = np.bincount(sp)
    cells = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 9)
    return "S %d %.17g %d %d %d %s %d %d %d %d %s | %s ;" % (
        nb, rmax, max_img, len(packed.numbers), len(nsp), " ".join(str(int(v)) for v in nsp), pbc[0], pbc[1], pbc[2], len(cells),
        " ".join("%.17g" % v for v in cells.ravel()), " ".join(switches))


def _parse(w):
    d = dict(zip(SELECT_KEYS, (int(x) for x in w[:len(SELECT_KEYS)])))
    d["guard_f"] = float(w[len(SELECT_KEYS)])
    d["near_thr"] = [int(x) for x in w[len(SELECT_KEYS) + 1:]]
    return d


def _select_cases():
    """name -> (driver line, what the GPU test of the same input asserts as last_path())"""
    tile_only = ("nocell", "norange")
    el, tri, img, thin = (H.rdf_path_case(k) for k in ("elongated", "elongated_tri", "plain_img", "thin_long"))
    cel = H.rdf_path_case("cell_ortho")
    return {
        "zf_cull": (_select_line(*el, switches=tile_only), "rdf_tile_zf"),
        "plain": (_select_line(*el, switches=tile_only + ("nozf",)), "rdf_tile"),
        "tri": (_select_line(*tri, switches=tile_only), "rdf_tile_tri"),
        "tri_off": (_select_line(*tri, switches=tile_only + ("nozf", "notri")), "rdf_tile"),
        "force_img": (_select_line(*img, switches=tile_only + ("force_img",)), "rdf_tile_img"),
        "v1": (_select_line(*el, switches=("v1",)), "rdf_exact"),
        "thin_long": (_select_line(*thin), "rdf_range"),
        "thin_long_norange": (_select_line(*thin, switches=("norange",)), "rdf_tile_zf"),
        "partial_pbc": (_select_line(*el, pbc=(1, 1, 0)), "rdf_exact"),
        "force_cell": (_select_line(*cel, switches=("force_cell",)), "rdf_cell"),
        "force_range": (_select_line(*cel, switches=("force_range", "nocell")), "rdf_range"),
        "cell_tile": (_select_line(*cel, switches=tile_only), "rdf_tile_zf"),
    }


def _path(d):
    if d["cell"]:
        return "rdf_cell"
    if d["range"]:
        return "rdf_range"
    if d["tri"]:
        return "rdf_tile_tri"
    if d["img"]:
        return "rdf_tile_img"
    if d["plain"]:
        return "rdf_tile_zf" if d["zf"] else "rdf_tile"
    return "rdf_exact"


@pytest.fixture(scope="module")
def selected(driver):
    cases = _select_cases()
    got = _ask(driver, [line for line, _ in cases.values()])
    return {name: _parse(w) for name, w in zip(cases, got)}


def test_selection_takes_the_paths_the_gpu_tests_assert(selected):
    for name, (_, path) in _select_cases().items():
        assert _path(selected[name]) == path, (name, selected[name])
        assert selected[name]["guard_f"] < 0.25


def test_selection_details(selected):
    assert selected["zf_cull"]["cull"] == 1 and selected["zf_cull"]["axis"] == 2
    assert selected["tri"]["zf"] == 0 and selected["tri"]["img"] == 0
    f = selected["force_img"]
    assert f["img"] == 1 and f["plain"] == 0 and f["tri"] == 0 and f["cell"] == 0 and f["range"] == 0
    assert f["near_thr"] == [0x7fffffff] * 3
    for name in ("v1", "partial_pbc"):
        d = selected[name]
        assert not any(d[k] for k in ("plain", "img", "tri", "zf", "cell", "range")), (name, d)
    t, tn = selected["thin_long"], selected["thin_long_norange"]
    assert t["cell"] == 0 and t["nk0"] < 5                      # too thin along x for five cells of rmax / 2
    assert t["nz2"] >= 3 and t["gy"] > 1 and len({t["axis"], t["axis_y"], 0}) == 3
    assert tn["range"] == 0 and tn["zf"] == 1 and tn["cull"] == 1
    c = selected["force_cell"]
    assert min(c["nk0"], c["nk1"], c["nk2"]) >= 5 and c["nk0"] * c["nk1"] * c["nk2"] <= max(125, 3264 // 2)
    assert selected["cell_tile"]["cell"] == 0 and selected["force_range"]["cell"] == 0


def test_driver_under_sanitizers(tmp):
    san = _build(tmp, ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "rdf_select_driver_san")
    lines = ["G %d %.17g" % c for c in _guard_lines()] + _chunk_lines(_chunk_cases()[::11]) + _chunk_lines([(5003, 210)], fpc=40) + \
            [line for line, _ in _select_cases().values()]
    cell = np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 29.53]])
    lines += ["F 0 %d %d %d 0.0125 %s" % (o + (" ".join("%.17g" % v for v in cell.ravel()),)) for o in ORDERS]
    lines += ["F 1 %d %d %d 0.01 30.8 0 0 0 27.3 0 0 0 55.3" % o for o in ORDERS]
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
