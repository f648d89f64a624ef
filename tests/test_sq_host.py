"""StructureFactor without a GPU: the choice of vectors, the bin count, the host assembly of the DataFrame from raw outputs,
weighting, the file round trip, argument checks and the C ABI declarations."""

import os
import re

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip
from amof_amd import structure_factor as sf
from amof_amd.frames import PackedTrajectory
from tests import sq_ref as ref
from tests.conftest import ROOT

TRICLINIC = np.array([[9.0, 0.0, 0.0], [2.5, 8.5, 0.0], [-1.5, 2.0, 9.5]])


def _ball(cell, qmax):
    """every half-space triple with |q| < qmax for one cell, by brute force over a generous box"""
    n = int(np.ceil(qmax * np.sqrt((np.asarray(cell) ** 2).sum(axis=1)).max() / (2 * np.pi))) + 3
    r = np.arange(-n, n + 1)
    t = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    t = t[sf.half_space(t)]
    return {tuple(x) for x in t[sf.q_norms(ref.reciprocal(cell), t) < qmax]}


def test_half_space_rule():
    t = np.array([[1, -3, 2], [0, 1, -5], [0, 0, 1], [0, 0, 0], [-1, 2, 2], [0, -1, 4], [0, 0, -2]])
    assert sf.half_space(t).tolist() == [True, True, True, False, False, False, False]


def test_enumeration_is_the_half_ball_of_a_constant_cell():
    hkl = sf.enumerate_hkl(TRICLINIC, 3.0)
    assert hkl.dtype == np.int32 and hkl.shape[1] == 3
    got = {tuple(x) for x in hkl}
    assert len(got) == len(hkl)                             # no duplicates
    assert sf.half_space(hkl).all()
    assert got == _ball(TRICLINIC, 3.0)                     # a constant cell: exactly the ball
    # no vector and its opposite together: rho(-k) = conj rho(k) is left out
    assert not any((-a, -b, -c) in got for a, b, c in got)


def test_enumeration_is_a_superset_under_a_varying_cell():
    rng = np.random.default_rng(3)
    cells = np.array([TRICLINIC * (1.0 + 0.04 * rng.normal()) + 0.3 * rng.normal(size=(3, 3)) for _ in range(6)])
    got = {tuple(x) for x in sf.enumerate_hkl(cells, 2.5)}
    for c in cells:
        assert _ball(c, 2.5) <= got
    assert len(got) < 3 * max(len(_ball(c, 2.5)) for c in cells)      # (and not a box of everything)


def test_max_points_subsample_is_seeded():
    full = sf.enumerate_hkl(TRICLINIC, 4.0)
    a = sf.enumerate_hkl(TRICLINIC, 4.0, dq=0.1, max_points=5, seed=7)
    b = sf.enumerate_hkl(TRICLINIC, 4.0, dq=0.1, max_points=5, seed=7)
    c = sf.enumerate_hkl(TRICLINIC, 4.0, dq=0.1, max_points=5, seed=8)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, c)
    assert {tuple(x) for x in a} <= {tuple(x) for x in full}
    bins_full = np.bincount((sf.q_norms(ref.reciprocal(TRICLINIC), full) / 0.1).astype(int))
    bins_a = np.bincount((sf.q_norms(ref.reciprocal(TRICLINIC), a) / 0.1).astype(int), minlength=len(bins_full))
    assert (bins_a == np.minimum(bins_full, 5)).all()     # full bins untouched, crowded ones cut to max_points
    with pytest.raises(ValueError):
        sf.enumerate_hkl(TRICLINIC, 4.0, max_points=5)


def test_bin_count_edge_cases():
    assert sf.n_bins(5.0, 0.02) == int(5.0 // 0.02) == 249      # float floor-division, as Rdf
    assert sf.n_bins(1.0, 0.1) == 9
    assert sf.n_bins(0.3, 0.1) == 2
    assert sf.n_bins(0.5, 1.0) == 0


def _packed(pbc=(True, True, True)):
    rng = np.random.default_rng(1)
    return PackedTrajectory(rng.random((2, 6, 3)) * 8.0, np.diag([8.0, 8.0, 8.0]), [8, 8, 1, 1, 1, 1], pbc=pbc)


def test_argument_errors_need_no_gpu():
    with pytest.raises(ValueError):
        sf.StructureFactor.from_trajectory(_packed(pbc=(True, True, False)), distributed=False)
    with pytest.raises(ValueError):
        sf.StructureFactor.from_trajectory(_packed(), dq=0.0, distributed=False)
    with pytest.raises(ValueError):
        sf.StructureFactor.from_trajectory(_packed(), dq=1.0, qmax=0.5, distributed=False)
    with pytest.raises(ValueError):
        sf.density_modes(_packed(pbc=(False, True, True)), [[1, 0, 0]])


def _synthetic(seed=2, nbins=12):
    rng = np.random.default_rng(seed)
    kinds = [1, 8, 30]
    sc = {1: 6, 8: 3, 30: 1}
    counts = rng.integers(1, 5, size=nbins).astype(np.uint64)
    counts[[0, 5]] = 0
    sums = rng.normal(size=(6, nbins)) * counts
    return counts, sums, kinds, sc


def test_assembly_from_counts_and_sums():
    counts, sums, kinds, sc = _synthetic()
    data = sf.assemble(counts, sums, kinds, [30, 8, 1], sc, 0.05)
    names = ["Zn", "O", "H"]
    assert list(data.columns) == ["q", "X-X"] + [a + "-" + b for a in names for b in names]
    np.testing.assert_array_equal(data["q"].values, np.arange(12) * 0.05)
    # library pairs (0,0)=H-H (0,1)=H-O (0,2)=H-Zn (1,1)=O-O (1,2)=O-Zn (2,2)=Zn-Zn
    c = counts.astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        xx = (sums[0] + sums[3] + sums[5] + 2 * (sums[1] + sums[2] + sums[4])) / (c * 10)
        np.testing.assert_allclose(data["X-X"].values, xx, rtol=1e-14)
        np.testing.assert_allclose(data["O-Zn"].values, sums[4] / (c * np.sqrt(3.0)), rtol=1e-14)
        np.testing.assert_allclose(data["H-H"].values, sums[0] / (c * 6.0), rtol=1e-14)
    np.testing.assert_array_equal(data["Zn-O"].values, data["O-Zn"].values)
    assert np.isnan(data.iloc[[0, 5], 1:].values).all()
    assert np.isfinite(data.drop(index=[0, 5]).values).all()
    # the restatement's normalisation agrees
    want = ref.normalised(counts.astype(np.int64), sums, kinds, [1] * 6 + [8] * 3 + [30])
    np.testing.assert_allclose(data["X-X"].values, want[0], rtol=1e-14)


def _object(counts, sums, kinds, sc, dq=0.05):
    obj = sf.StructureFactor()
    obj.kinds, obj.counts, obj.sums, obj.dq, obj.species_counts = kinds, counts, sums, dq, sc
    obj.data = sf.assemble(counts, sums, kinds, [30, 8, 1], sc, dq)
    return obj


def test_weighted_with_equal_weights_is_x_x():
    counts, sums, kinds, sc = _synthetic()
    obj = _object(counts, sums, kinds, sc)
    for w in (1.0, 2.5):
        got = obj.weighted({"H": w, "O": w, "Zn": w})
        np.testing.assert_allclose(got["S"].values, obj.data["X-X"].values, rtol=1e-12)
    # callables of q and atomic-number keys; a single nonzero weight picks that species' partial
    got = obj.weighted({1: lambda q: 0.0 * q, 8: 0.0, 30: lambda q: 1.0 + q})
    np.testing.assert_allclose(got["S"].values, obj.data["Zn-Zn"].values, rtol=1e-12)
    np.testing.assert_array_equal(got["q"].values, obj.data["q"].values)
    with pytest.raises(KeyError):
        obj.weighted({"H": 1.0, "O": 1.0})


def test_feather_round_trip(tmp_path):
    counts, sums, kinds, sc = _synthetic()
    obj = _object(counts, sums, kinds, sc)
    path = os.path.join(str(tmp_path), "run")
    obj.write_to_file(path)
    assert os.path.exists(path + ".sq")
    back = sf.StructureFactor.from_file(path)
    pd.testing.assert_frame_equal(back.data, obj.data)


def test_restatement_of_a_two_atom_cell():
    # two atoms at s = 0 and s = (1/2, 0, 0): rho(h, k, l) = 1 + (-1)^h
    packed = PackedTrajectory(np.array([[[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]]]), np.diag([4.0, 5.0, 6.0]), [6, 6])
    hkl = np.array([[1, 0, 0], [2, 0, 0], [0, 1, 0]])
    rho = ref.modes(packed.pos_host()[0], packed.cell[0], np.zeros(2, dtype=int), 1, hkl)
    np.testing.assert_allclose(rho[:, 0], [0.0, 2.0, 2.0], atol=1e-12)
    counts, sums, beyond, _ = ref.sq(packed, hkl, 0.5, 4)      # |q| = 2 pi / 4 * h, 2 pi / 5
    assert beyond == 1 and counts.tolist() == [0, 0, 1, 1]
    np.testing.assert_allclose(sums[0], [0, 0, 4.0, 0.0], atol=1e-12)


def test_abi_declares_and_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "amof_hip.h")).read()
    declared = set(re.findall(r"\b(amof_[a-z0-9_]+)\s*\(", header))
    for name in ("amof_sq_accumulate", "amof_sq_accumulate_dev", "amof_sq_modes"):
        assert name in declared and name in _hip.EXPORTS
        assert hasattr(_hip.load_library(), name)
    doc = header[header.index("kernel family that produced the result of the last call"):header.index("const char *amof_last_path")]
    assert '"sq"' in doc and '"sq_bin_global"' in doc
