"""Before any GPU run of tests/test_gpu_tile_ahead.py: every window class the plan kernel's read-ahead has to get right
occurs in the input that is there for it (tests/tile_ahead_cases.py: empty for a wave, ragged tail behind a plain quad and
behind own block + plain quads, two pieces for the first and the last sub-tile, dead steps and frames between live ones,
chains of integer and ZF steps), counted on the CPU through tests/native/tile_plan_driver.cpp."""

import pytest

from tests import tile_ahead_cases as T


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return T.build_driver(tmp_path_factory.mktemp("ta"))


@pytest.mark.parametrize("name", sorted(T.CASES))
def test_window_classes_occur(driver, name):
    packed, rmax, nbins, env = T.CASES[name]()
    c = T.classify(packed, rmax, driver, env)
    print(name, c)
    assert c["live"] > 0
    for k in T.REQUIRED[name]:
        assert c[k] >= 1, (name, k, c)


def test_short_windows_counted(driver):
    # the numbers the GPU test states: steps of `long_cell` with a piece of fewer than 16 partners, and ragged last quads
    packed, rmax, nbins, env = T.CASES["long_cell"]()
    c = T.classify(packed, rmax, driver, env)
    assert (c["empty_for_a_wave"], c["ragged_tail"]) == T.LONG_CELL_COUNTS, c
