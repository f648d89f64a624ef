"""The inputs of tests/test_gpu_tile_step_state.py hold what the two grid slices of the planned tile kernel have to get right
(tests/tile_step_state_cases.py: the form of every step from amof_amd/csrc/tile_plan.h) -- checked here without a GPU."""

import pytest

from tests import tile_ahead_cases as T
from tests import tile_step_state_cases as C


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    return T.build_driver(tmp_path_factory.mktemp("tile_step_state_cpu"))


def test_zif544_has_integer_steps_only(driver):
    packed, rmax, nbins = C.zif544()
    for env in ({}, {"AMOF_RDF_FPC": "8"}):
        st, tiles, pairs = C.steps(packed, rmax, driver, env)
        seen = C.census(st)
        assert [t[2] for t in tiles] == [192, 192, 128, 32] and len(pairs) == 10
        assert seen["zf"] == 0 and seen["integer"] == 19 * (2 * 4 + 2 * 3 + 2 + 1) and seen["dead"] == 0, seen


def test_graded_mixes_the_forms(driver):
    packed, rmax, nbins = C.graded()
    st, tiles, pairs = C.steps(packed, rmax, driver)
    seen = C.census(st)
    assert [t[2] for t in tiles] == [512, 512, 512, 465, 100] and len(pairs) == 15
    assert min(seen["zf"], seen["integer"]) > 400 and seen["dead"] > 100, seen
    assert seen["mixed_items"] > 100 and seen["zf_only_items"] > 0 and seen["integer_only_items"] > 0, seen
    assert seen["sub_in_both_forms"] > 200, seen
    # the thin species' centres: integer form in every frame
    assert all(not zf for p, c, f, sub, ti, live, zf in st if ti == 4 and live)
    # chunks of eight frames and batches of seven: still both forms in one work item, sub-tiles in both forms in one chunk
    st8, _, _ = C.steps(packed, rmax, driver, {"AMOF_RDF_FPC": "8"})
    assert C.census(st8)["mixed_items"] > 0 and C.census(st8)["sub_in_both_forms"] > 0
    for lo in (0, 7, 14):
        sb, _, _ = C.steps(packed, rmax, driver, frames=(lo, min(19, lo + 7)))
        assert C.census(sb)["mixed_items"] > 0 and C.census(sb)["sub_in_both_forms"] > 0, lo
