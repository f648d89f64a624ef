"""The host plan of the velocity-autocorrelation entry point has one definition (amof_amd/csrc/vacf_select.h, here through
tests/native/vacf_select_driver.cpp): which kernel answers, the lag tiles, the LDS bytes -- on the CPU, at the edges of every
rule and as invariants over a sweep."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "vacf_select_driver.cpp")
LDS, GENERAL = 0, 1
BUDGET = 150 * 1024         # MSD_LDS_SERIES
CU = 160 * 1024             # the LDS of a CU: two buffers only where two workgroups of them fit


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vs") / "vacf_select_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _ask(driver, lines):
    r = subprocess.run([driver], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == len(lines)
    return [l.split() for l in out]


def _plans(driver, calls):
    """calls: (F, stride, switches, W, d); switches: 1 general + 2 nodb + 4 db"""
    plans = []
    for w in _ask(driver, ["P %d %d %d %d %d" % c for c in calls]):
        p = dict(zip(("kernel", "n_tiles", "lanes", "tile_lags", "tail", "series", "db", "lds"), (int(x) for x in w[:8])))
        p["path"] = w[8]
        rest = [int(x) for x in w[9:]]
        p["tiles"] = list(zip(rest[0::2], rest[1::2]))
        assert len(p["tiles"]) == p["n_tiles"]
        plans.append(p)
    return plans


@pytest.fixture(scope="module")
def consts(driver):
    group, R, lanes, budget = (int(x) for x in _ask(driver, ["K"])[0])
    assert R % 2 == 1 and lanes % 64 == 0 and budget == BUDGET and group >= 1
    return R, lanes


def _check_lds_plan(p, F, W, R, max_lanes, sw=0):
    assert p["path"] == "vacf_lds" and p["kernel"] == LDS
    assert p["lanes"] % 64 == 0 and 64 <= p["lanes"] <= max_lanes and p["tile_lags"] == p["lanes"] * R
    # the tiles cover every lag once, none is empty
    assert [m for first, n in p["tiles"] for m in range(first, first + n)] == list(range(W))
    assert all(0 < n <= p["tile_lags"] for _, n in p["tiles"])
    # what a lane reads stays inside the series: origin k + s <= F + R - 2, partner <= F + 65 R - 2
    assert p["series"] == F + p["tail"] and p["tail"] >= p["tile_lags"] + R and p["series"] > F + 65 * R - 2
    assert p["series"] * 8 <= BUDGET and p["lds"] <= BUDGET
    want_db = not sw & 2 and 2 * p["series"] * 8 <= BUDGET and (bool(sw & 4) or 4 * p["series"] * 8 <= CU)
    assert p["lds"] == (2 if p["db"] else 1) * p["series"] * 8 and p["db"] == int(want_db)


def test_fast_path_only_for_consecutive_lags_stride_one_and_a_series_that_fits(driver, consts):
    R, max_lanes = consts
    fast, strided, thinned, forced, long_series, fits_single = _plans(driver, [
        (1031, 1, 0, 515, 1), (1031, 1, 0, 128, 4), (1031, 3, 0, 515, 1), (1031, 1, 1, 515, 1), (19300, 1, 0, 64, 1), (15000, 1, 0, 64, 1)])
    _check_lds_plan(fast, 1031, 515, R, max_lanes)
    assert fast["db"] == 1 and fast["n_tiles"] == 1
    for p in (strided, thinned, forced, long_series):
        assert (p["kernel"], p["path"], p["n_tiles"], p["lds"]) == (GENERAL, "vacf_general", 0, 0)
    _check_lds_plan(fits_single, 15000, 64, R, max_lanes)
    assert fits_single["db"] == 0
    # the headline: 2500 lags of 5000 frames in one tile of four waves; one buffer, so that two workgroups share a CU
    head, head_db, fast_nodb = _plans(driver, [(5000, 1, 0, 2500, 1), (5000, 1, 4, 2500, 1), (1031, 1, 2, 515, 1)])
    _check_lds_plan(head, 5000, 2500, R, max_lanes)
    assert (head["n_tiles"], head["lanes"], head["db"]) == (1, 256, 0) and 2 * head["lds"] <= CU
    _check_lds_plan(head_db, 5000, 2500, R, max_lanes, sw=4)
    assert head_db["db"] == 1
    _check_lds_plan(fast_nodb, 1031, 515, R, max_lanes, sw=2)
    assert fast_nodb["db"] == 0
    # a single lag 0 is consecutive; a single lag elsewhere is not (d = 1 lists only start at 0: two lags 0, 2 are strided)
    one, two = _plans(driver, [(67, 1, 0, 1, 1), (67, 1, 0, 2, 2)])
    _check_lds_plan(one, 67, 1, R, max_lanes)
    assert two["kernel"] == GENERAL


def test_lag_tiles_at_the_edges(driver, consts):
    R, max_lanes = consts
    Ms = [1, R - 1, R, R + 1, 64 * R - 1, 64 * R, 64 * R + 1, max_lanes * R - 1, max_lanes * R, max_lanes * R + 1, 2 * max_lanes * R + 1]
    calls = [(2 * M + 2, 1, 0, M, 1) for M in Ms]
    for (F, _, _, M, _), p in zip(calls, _plans(driver, calls)):
        _check_lds_plan(p, F, M, R, max_lanes)
        assert p["n_tiles"] == -(-M // (max_lanes * R))         # (these series are short: the widest tiles fit)


def test_invariants_over_a_sweep(driver, consts):
    R, max_lanes = consts
    calls = [(F, 1, sw, M, 1) for F in list(range(2, 200, 7)) + [1000, 5000, 9000, 12000, 15000, 18000, 19000, 19136, 19200, 19201, 30000]
             for M in sorted({1, 2, F // 4 + 1, F // 2, max(F - 1, 1)}) for sw in (0, 2, 4)]
    kernels = set()
    for (F, _, sw, M, _), p in zip(calls, _plans(driver, calls)):
        kernels.add(p["kernel"])
        if p["kernel"] == LDS:
            _check_lds_plan(p, F, M, R, max_lanes, sw)
        else:
            # refused only where not even one wave of lanes fits behind the series
            assert (F + (64 * R + R + 1) // 2 * 2) * 8 > BUDGET, (F, M, p)
    assert kernels == {LDS, GENERAL}
    assert _plans(driver, [(1, 1, 0, 1, 1)])[0]["kernel"] == GENERAL        # one frame: no origin anywhere


def test_driver_under_sanitizers(tmp_path):
    san = str(tmp_path / "vacf_select_driver_san")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", san],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = ["K"] + ["P %d %d %d %d %d" % (F, s, sw, M, d) for F in (1, 2, 67, 1031, 5000, 19200, 19300) for s in (1, 3) for sw in (0, 1, 2, 4)
                     for M, d in ((0, 1), (1, 1), (F // 2 + 1, 1), (F, 1), (F // 8 + 1, 4))]
    r = subprocess.run([san], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    assert len(r.stdout.strip().splitlines()) == len(lines)
