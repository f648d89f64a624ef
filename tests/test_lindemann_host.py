"""Lindemann index without a GPU: the restatement (tests/lindemann_ref.py) on known answers and on every committed case of
tests/lindemann_cases.py -- the two conditions the GPU tests rest on --, the block arithmetic, the scale, the host side of the
class (amof_amd/lindemann.py) and the agreement of the header with the Python bindings."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import lindemann as L
from tests import lindemann_cases as cases
from tests import lindemann_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_static_trajectory_gives_zero():
    p = cases.static()
    want = ref.lindemann(p.pos, p.cell, p.numbers, cases.CLASS_SETS, 6, 6)
    assert ref.pair_counts(want).tolist() == [[64, 128]]           # 16 Zn x 4 N; 64 N with 2 C each
    for blk in want.blocks[0]:
        assert not blk.delta.any() and not blk.budget.any()
    ref.check(np.array([[[64, 0], [128, 0]]]), [40, 40], want)


def test_alternating_pair():
    p = cases.alternating(8)
    for B, S in ((8, 8), (4, 2), (2, 1)):
        want = ref.lindemann(p.pos, p.cell, p.numbers, [(30, 7, 3.5)], B, S)
        assert len(want.starts) == (8 - B) // S + 1
        for row in want.blocks:
            assert row[0].delta.tolist() == [0.2] and row[0].i.tolist() == [0] and row[0].j.tolist() == [1]
    assert int(np.rint(0.2 * 2.0 ** 40)) == cases.ALTERNATING_TERM
    # with the cutoff between the two distances, a block that starts on an odd frame has no pair
    want = ref.lindemann(p.pos, p.cell, p.numbers, [(30, 7, 2.5)], 4, 1)
    assert ref.pair_counts(want)[:, 0].tolist() == [1, 0, 1, 0, 1]
    want = ref.lindemann(p.pos, p.cell, p.numbers, [(30, 7, 2.5)], 4, 1, select=1)
    assert ref.pair_counts(want)[:, 0].tolist() == [1, 1, 1, 1, 1]


@pytest.mark.parametrize("B", [64, 130, 200])
def test_cosine_over_one_period(B):
    d, want = cases.cosine(B)
    delta, budget = ref.series_delta(d)
    assert np.all(np.abs(delta - want) <= 1e-12) and float(budget.max()) < 2.0 ** -30


def test_block_arithmetic_and_refusals():
    assert ref.block_starts(131, 131, 131) == [0] and ref.block_starts(131, 50, 27) == [0, 27, 54, 81]
    assert ref.block_starts(131, 64, 67) == [0, 67] and ref.block_starts(131, 20, 20) == [0, 20, 40, 60, 80, 100]
    for F, B, S in ((131, 131, 131), (131, 50, 27), (131, 64, 67), (131, 20, 20), (10, 2, 1), (200, 64, 64)):
        nb, starts, unused = L.blocks(F, B, S)
        assert nb == len(starts) and starts.tolist() == ref.block_starts(F, B, S) and unused == F - (starts[-1] + B) >= 0
    assert L.blocks(131, 50, 27)[2] == 0 and L.blocks(131, 64, 67)[2] == 0 and L.blocks(131, 20, 20)[2] == 11
    for bad in ((10, 1, 1), (10, 11, 1), (10, 5, 0), (10, 2.5, 1), (10, 0, 1)):
        with pytest.raises(ValueError):
            L.blocks(*bad)
    with pytest.raises(ValueError):
        ref.block_starts(10, 1, 1)
    p = cases.case("arguments").packed
    with pytest.raises(ValueError, match="half the smallest"):
        L.Lindemann.from_trajectory(p, {'Zn-N': 8.7}, block=5, device=0, distributed=False)       # > 17.31 / 2
    with pytest.raises(ValueError):
        L.Lindemann.from_trajectory(p, {'Zn-N': 3.0}, block=5, pairs="all", device=0, distributed=False)
    assert L.bin_count(0.5, 0.005) == 100 and L.bin_count(0.5, 0.3) == 2 and L.bin_count(0.004, 0.005) == 1


def test_scale():
    for na, nb, B in ((16, 64, 200), (150, 150, 131), (3000, 3000, 5000), (10 ** 6, 10 ** 6, 4), (1, 1, 2)):
        assert L.scale_log2(na, nb, B) == ref.scale_log2(na, nb, B) <= 40
    assert L.scale_log2(16, 64, 200) == 40 and L.scale_log2(10 ** 6, 10 ** 6, 4) == 21
    assert L.scale_log2(3000, 3000, 5000) == 62 - (3000 * 3000 * 71).bit_length()       # ceil(sqrt(5000)) = 71
    with pytest.raises(ValueError):
        L.scale_log2(3 * 10 ** 6, 10 ** 6, 4)
    with pytest.raises(ValueError):
        ref.scale_log2(3 * 10 ** 6, 10 ** 6, 4)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_keeps_the_gpu_tests_honest(name):
    c = cases.case(name)
    for B, S in c.blocks:
        for select in (0, 1):
            want = cases.reference(name, B, S, select)
            assert ref.pair_counts(want).sum() > 0
            assert want.worst < 2.0 ** -30, (name, B, S, want.worst)
            assert ref.near_edge(want, cases.DDELTA, cases.NBINS) == 0, (name, B, S)
    if name == "composition":
        want = cases.reference(name, 33, 18, 0, (61, 180))
        assert want.worst < 2.0 ** -30 and ref.near_edge(want, cases.DDELTA, cases.NBINS) == 0


def test_assemble_columns_nan_columns_onset_and_feather(tmp_path):
    names = [("Zn-N", True), ("Zn-Au", False), ("C-N", True)]
    sums = np.array([[[4, 4 << 33], [2, 3 << 30]], [[0, 0], [2, 1 << 34]], [[4, 9 << 33], [0, 0]]], dtype=np.int64)
    data = L.assemble(sums, [36, 35], names, [0.0, 50.0, 100.0])
    assert list(data.columns) == ["Time", "Zn-N", "Zn-N-n", "Zn-Au", "Zn-Au-n", "C-N", "C-N-n"]
    assert data["Zn-N"].tolist()[0] == 0.125 and np.isnan(data["Zn-N"][1]) and data["Zn-N"][2] == 0.28125
    assert data["Zn-N-n"].tolist()[0] == 4 and np.isnan(data["Zn-N-n"][1])
    assert data["C-N"].tolist()[:2] == [3 / 64, 0.25] and np.isnan(data["C-N"][2])
    assert data["Zn-Au"].isna().all() and data["Zn-Au-n"].isna().all()
    obj = L.Lindemann()
    obj.data = data
    onset = obj.onset()
    assert onset["Zn-N"] == 0.0 and onset["C-N"] == 50.0 and np.isnan(onset["Zn-Au"]) and set(onset) == {"Zn-N", "Zn-Au", "C-N"}
    assert obj.onset(0.2)["Zn-N"] == 100.0 and np.isnan(obj.onset(0.3)["C-N"])
    hist = np.zeros((3, 2, 4), dtype=np.uint64)
    hist[0, 0] = (1, 3, 0, 0)
    hist[2, 0] = (0, 0, 4, 0)
    h = L.assemble_hist(hist, names, 0.25)
    assert list(h.columns) == ["delta", "Zn-N", "C-N"] and h["delta"].tolist() == [0.125, 0.375, 0.625, 0.875]
    assert h["Zn-N"].tolist() == [0.5, 1.5, 2.0, 0.0] and h["C-N"].isna().all()
    path = str(tmp_path / "ramp")
    obj.write_to_file(path)
    assert os.path.exists(path + ".lind")
    assert L.Lindemann.from_file(path).data.equals(data)


def test_header_and_exports_agree():
    text = open(os.path.join(ROOT, "include", "amof_hip.h")).read()
    declared = set(re.findall(r"^(?:int|double|int64_t|const char \*)\s*\*?(amof_\w+)\(", text, flags=re.M))
    assert {"amof_lindemann", "amof_lindemann_dev"} <= declared
    assert {"amof_lindemann", "amof_lindemann_dev"} <= set(_hip.EXPORTS)
    assert re.search(r"#define AMOF_ABI_VERSION 4\b", text) and _hip.ABI_VERSION == 4
    lib = _hip.load_library()
    assert lib.amof_abi_version() == 4 and hasattr(lib, "amof_lindemann") and hasattr(lib, "amof_lindemann_dev")
