"""The dynamic LDS of the tile kernel (tile_lds, amof_amd/csrc/rdf_select.h, here through tests/native/tile_lds_driver.cpp):
a planned launch has no centre buffers, so that six workgroups fit the 160 KiB of a CU at the headline's 2310 bins; every
other launch keeps its size."""

import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tile_lds_driver.cpp")
MAX_BINS = 36864 - 5120                 # AMOF_MAX_LDS_BINS - 5120 (include/amof_hip.h)
CU_LDS = 160 * 1024


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tl") / "tile_lds_driver")
    r = subprocess.run(["g++", "-std=c++17", "-O1", SRC, "-o", out], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return out


def _ask(driver, rows):
    r = subprocess.run([driver], input="".join("%d %d %d\n" % row for row in rows), capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    out = [tuple(int(x) for x in l.split()) for l in r.stdout.strip().splitlines()]
    assert len(out) == len(rows)
    return out


def test_headline_sizes(driver):
    ((unplanned, planned),) = _ask(driver, [(2310, 0, 0)])
    assert planned == 25760 and 6 * planned <= CU_LDS
    assert unplanned == 29856 and 5 * unplanned <= CU_LDS < 6 * unplanned


def test_planned_size_is_the_unplanned_one_without_centre_buffers(driver):
    rows = [(nb, 0, 0) for nb in range(1, MAX_BINS + 1)]
    for (nb, _, _), (unplanned, planned) in zip(rows, _ask(driver, rows)):
        assert planned == unplanned - 4096, nb
        # two partner tiles, two centre sub-tiles, the histogram with its 32 trash words and 2 spare, padded to 16 bytes
        assert unplanned == 2 * (512 + 128) * 16 + 4 * ((nb + 32 + 2 + 3) & ~3), nb


def test_queues_keep_their_size(driver):
    # the variants with parked pairs never run from a plan: their sizes as before
    for (nb, queue, defer), (unplanned, _) in zip([(999, 96, 1), (999, 1024, 0)], _ask(driver, [(999, 96, 1), (999, 1024, 0)])):
        assert unplanned == 2 * (512 + 128) * 16 + 4 * ((nb + 32 + 2 + 3) & ~3) + (2 if defer else 1) * queue * 8 + 16
