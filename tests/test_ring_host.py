"""Ring statistics without a GPU: the two references of tests/ring_ref.py against each other and against the known answers on
every case of tests/ring_cases.py, the host arithmetic of amof_amd/ring.py (``assemble``) on hand-made integers, the argument
checks, the entry point in the header and in ``_hip``, and the Dataset leg of the class with tests/fake_xarray.py."""

import os
import sys

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import ring as amring
from amof_amd.ring import Ring, assemble
from tests import fake_xarray
from tests import ring_cases as cases
from tests import ring_ref as ref
from tests.conftest import ROOT


@pytest.mark.parametrize("name", cases.NAMES)
def test_search_equals_brute_force_and_the_known_answers(name):
    c = cases.case(name)
    for adj, (got, truncated) in zip(cases.graphs(name), cases.reference(name)):
        if c.against == "brute":
            assert np.array_equal(got, ref.brute(adj, c.nmax))
        if c.known is not None:
            assert ref.rings(got) == c.known
        if c.truncated is not None:
            assert truncated == c.truncated
        assert not got[:, :3].any()
        ref.rings(got)                  # every column sum is a multiple of its ring size


def test_the_cases_are_what_they_claim():
    deg = np.bincount([len(a) for a in cases.graphs("zif4_16")[0]])
    assert deg.tolist() == [0, 96, 0, 160, 16]
    assert ref.search(cases.graphs("zif4_32")[0], 32)[2] == 24
    assert ref.search(cases.graphs("zif4_32")[0], 32)[1] > 0 and ref.search(cases.graphs("polygon13")[0], 12)[1] == 0
    for name in ("random_rect", "random_tri"):
        p = cases.case(name).packed
        assert p.n_atoms == 150 and p.n_frames == 3 and len(set(p.numbers.tolist())) == 2
        degs = np.concatenate([[len(a) for a in adj] for adj in cases.graphs(name)])
        assert set(range(7)) <= set(degs.tolist()) and degs.max() <= 16 and 2.0 < degs.mean() < 4.5
        assert any(ref.rings(c) for c, _ in cases.reference(name))
    assert not np.allclose(cases.case("random_tri").packed.cell[0], np.diag(np.diag(cases.case("random_tri").packed.cell[0])))
    # the 5^3 lattice has what the 7^3 one has per atom, plus the five-rings that wind around the cell
    assert ref.rings(cases.reference("sc5")[0][0])[5] == 75 and 5 not in ref.rings(cases.reference("sc7")[0][0])


def test_counts_at_a_size_do_not_depend_on_the_depth():
    for name in ("zif4_16", "random_rect", "graphene"):
        adj = cases.graphs(name)[0]
        small, large = ref.search(adj, 8)[0], ref.search(adj, 12)[0]
        assert np.array_equal(small[:, :9], large[:, :9])


def test_assemble_on_hand_made_integers():
    nmax, N = 6, 10
    counts = np.zeros((2, 4, nmax + 1), dtype=np.int64)
    # frame 0: two 3-rings over 5 atoms (one shared), one 6-ring; frame 1: nothing
    counts[0, 0, 3], counts[0, 1, 3], counts[0, 2, 3], counts[0, 3, 3] = 6, 5, 5, 4
    counts[0, 0, 6], counts[0, 1, 6], counts[0, 2, 6], counts[0, 3, 6] = 6, 6, 5, 6
    table, mean, report = assemble(counts, [3, 0], N, [10, 15], nmax)
    assert list(table.columns) == ["Step", "ring_size", "rings", "Rc(n)", "Pn(n)", "Pmax(n)", "Pmin(n)"]
    assert table["Step"].tolist() == [10] * 4 + [15] * 4 and table["ring_size"].tolist() == [3, 4, 5, 6] * 2
    assert table["rings"].tolist() == [2, 0, 0, 1, 0, 0, 0, 0]
    row3, row4, row6 = table.iloc[0], table.iloc[1], table.iloc[3]
    assert (row3["Rc(n)"], row3["Pn(n)"], row3["Pmin(n)"], row3["Pmax(n)"]) == (2 / 10, 5 / 10, 5 / 5, 4 / 5)
    assert (row6["Rc(n)"], row6["Pn(n)"], row6["Pmin(n)"], row6["Pmax(n)"]) == (1 / 10, 6 / 10, 5 / 6, 6 / 6)
    assert row4["Rc(n)"] == 0.0 and row4["Pn(n)"] == 0.0 and np.isnan(row4["Pmin(n)"]) and np.isnan(row4["Pmax(n)"])
    assert np.isnan(table["Pmax(n)"].values[4:]).all() and not table["Rc(n)"].values[4:].any()
    assert mean.index.tolist() == [3, 4, 5, 6] and mean.loc[3, "Rc(n)"] == 0.1 and mean.loc[3, "Pmin(n)"] == 1.0
    assert np.isnan(mean.loc[4, "Pmin(n)"]) and mean.loc[6, "rings"] == 0.5
    assert report.index.tolist() == [10, 15] and report["max_search_depth"].tolist() == [6, 6]
    assert report["Truncated sources"].tolist() == [3, 0]
    assert report["Rings statistics computed with potentially undiscovered rings"].tolist() == [True, False]
    # a membership sum that its ring size does not divide is an internal error, never rounded
    counts[0, 0, 6] = 7
    with pytest.raises(_hip.AmofError, match="size 6"):
        assemble(counts, [3, 0], N, [10, 15], nmax)
    with pytest.raises(ValueError):
        assemble(counts[:, :, :-1], [3, 0], N, [10, 15], nmax)


def test_assemble_on_the_fixture():
    c, truncated = cases.reference("zif4_32")[0]
    table, mean, report = assemble(ref.counts(c)[None], [truncated], 272, [0], 32)
    found = {int(n): int(r) for n, r in zip(table["ring_size"], table["rings"]) if r}
    assert found == {5: 32, 16: 24, 24: 32, 32: 24}
    assert table.loc[table["ring_size"] == 5, "Pn(n)"].item() == 160 / 272      # the atoms of the 32 imidazolate rings
    assert bool(report[amring.UNDISCOVERED].iloc[0])


def test_argument_checks():
    for bad in (2, 33, 0, -1, 7.5):
        with pytest.raises(ValueError):
            amring.check_depth(bad)
        with pytest.raises(ValueError):
            Ring.from_trajectory(cases.case("polygon3").packed, {'C-C': 1.6}, max_search_depth=bad)
    assert amring.check_depth(3) == 3 and amring.check_depth(32) == 32 and amring.check_depth(16.0) == 16
    with pytest.raises(ValueError):
        Ring.from_trajectory(cases.case("polygon3").packed, {})


def test_entry_point_in_the_header_and_in_hip():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        header = fh.read()
    assert "int amof_ring_stats(amof_ctx *ctx, const amof_traj *traj, const double *cutoff" in header
    assert "int amof_ring_search_stats(" in header and "#define AMOF_ABI_VERSION 4" in header
    assert "amof_ring_stats" in _hip.EXPORTS and "amof_ring_search_stats" in _hip.EXPORTS
    assert callable(_hip.Context.ring_stats) and callable(_hip.MultiContext.ring_stats)
    with open(os.path.join(ROOT, "amof_amd", "csrc", "ring_search.h")) as fh:
        text = fh.read()
    assert "#define RING_MAX_DEGREE 16" in text and "#define RING_MAX_PATHS 1024" in text and "hip/" not in text


def test_dataset_leg_with_a_stand_in_xarray(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "xarray", fake_xarray)
    c, truncated = cases.reference("zif4_16")[0]
    counts = np.stack([ref.counts(c), ref.counts(np.zeros_like(c))])
    obj = Ring(max_search_depth=16)
    obj._assemble(counts, np.array([truncated, 0]), None, 272, [100, 150], 16)
    ds = obj.data
    assert isinstance(ds, fake_xarray.Dataset) and list(ds.data_vars) == ["ring"]
    xa = ds["ring"]
    assert xa.dims == ("Step", "ring_size", "ring_var")
    assert list(xa.coords["Step"]) == [100, 150] and list(xa.coords["ring_size"]) == list(range(3, 17))
    assert list(xa.coords["ring_var"]) == ["rings", "Rc(n)", "Pn(n)", "Pmax(n)", "Pmin(n)"]
    assert xa.sel(Step=100, ring_var="rings").values.tolist() == [0, 0, 32] + [0] * 10 + [24]
    assert xa.sel(Step=100, ring_size=16, ring_var="Rc(n)").values == 24 / 272
    assert not xa.sel(Step=150, ring_var="rings").values.any() and np.isnan(xa.sel(Step=150, ring_var="Pmin(n)").values).all()
    np.testing.assert_array_equal(xa.values.reshape(-1, 5), obj.table[list(amring.RING_VARS)].values)
    path = str(tmp_path / "rings")
    obj.write_to_file(path)
    assert os.path.exists(path + ".ring") and os.path.exists(path + ".report_search.csv")
    again = Ring.from_file(path)
    np.testing.assert_array_equal(again.data["ring"].values, xa.values)
    import pandas as pd
    back = pd.read_csv(path + ".report_search.csv").set_index("Step")
    assert back["Truncated sources"].tolist() == [truncated, 0] and back[amring.UNDISCOVERED].tolist() == [True, False]


def test_without_xarray_data_is_none_and_writing_raises(monkeypatch, tmp_path):
    monkeypatch.setitem(sys.modules, "xarray", None)        # (import xarray then raises ImportError)
    c, truncated = cases.reference("polygon5")[0]
    obj = Ring(max_search_depth=12)
    obj._assemble(ref.counts(c)[None], np.array([truncated]), None, 5, [0], 12)
    assert obj.data is None and obj.table["rings"].sum() == 1 and obj.counts.shape == (1, 4, 13)
    with pytest.raises(ImportError):
        obj.write_to_file(str(tmp_path / "x"))
