"""WindowVanHove without a GPU: the numpy restatement against the MSD oracle, the window rule, the host assembly of the
DataFrames from raw outputs, the file round trip and the C ABI declarations."""

import os
import re

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip
from amof_amd import lags
from amof_amd import vanhove as vh
from amof_amd.frames import PackedTrajectory
from oracle import numpy_oracle as no
from tests import helpers as H
from tests import vanhove_ref as ref
from tests.conftest import ROOT


def _small_walk(seed, F=40, n=30, sigma=0.4):
    rng = np.random.default_rng(seed)
    cell = np.diag([6.0, 7.0, 8.0])
    p0 = rng.random((n, 3)) @ cell
    pos = p0 + np.cumsum(rng.normal(scale=sigma, size=(F, n, 3)), axis=0)
    pos = (pos / np.diag(cell)) % 1.0 * np.diag(cell)      # wrapped: atoms cross faces
    numbers = np.array([30, 7, 6][:3] * (n // 3) + [1] * (n % 3))
    return PackedTrajectory(pos, cell, numbers)


@pytest.mark.parametrize("unwrap", [False, True])
def test_restatement_second_moment_is_the_window_msd(unwrap):
    packed = _small_walk(3)
    F = len(packed)
    window, _ = no.msd_window_setup(F, delta_time=3, timestep=1)
    counts, overflow, moments, _, kinds = ref.vanhove(packed, window, 0.05, 40, unwrap=unwrap)
    elements, msd = no.window_msd(packed.pos_host(), packed.cell, packed.numbers, packed.masses, window, unwrap=unwrap)
    for e, m_ref in zip(elements, msd):
        s = kinds.index(int(e))
        n_s = int((packed.numbers == e).sum())
        np.testing.assert_allclose(moments[s, :, 0] / n_s / (F - window), m_ref, rtol=1e-12, atol=1e-15)
        # every sample is counted once
        assert np.array_equal(counts[s].sum(axis=1) + overflow[s], n_s * (F - window - 1))


def test_windows_follow_window_msd():
    for F, kw in [(5000, dict(delta_time=100)), (37, dict(delta_time=4, timestep=2)), (100, dict(delta_time=5, max_time=30)),
                  (9, dict(delta_time=1, max_time=1000))]:
        w, t = lags.window_setup(F, **kw)
        w_ref, t_ref = no.msd_window_setup(F, **kw)
        assert np.array_equal(w, w_ref) and np.array_equal(t, t_ref)
    assert len(lags.window_setup(5000)[0]) == 25


def _synthetic(seed=1, W=4, nbins=50, dr=0.1):
    rng = np.random.default_rng(seed)
    kinds = [1, 6, 30]
    species_counts = {1: 5, 6: 3, 30: 1}
    F = 20
    window = np.arange(W) * 2
    counts = np.zeros((3, W, nbins), np.uint64)
    overflow = np.zeros((3, W), np.uint64)
    for s, z in enumerate(kinds):
        for w, m in enumerate(window):
            n = species_counts[z] * (F - m - 1)
            k = rng.integers(0, n + 1)
            counts[s, w] = np.bincount(rng.integers(0, nbins, size=k), minlength=nbins)
            overflow[s, w] = n - k
    moments = rng.random((3, W, 2)) + 0.5
    moments[:, 0] = 0.0                     # m = 0: every displacement is zero
    return counts, overflow, moments, kinds, species_counts, F, window, dr


def test_assembly_normalisation_and_pooling():
    counts, overflow, moments, kinds, sc, F, window, dr = _synthetic()
    elements = [30, 6, 1]
    data, alpha2 = vh.assemble(counts, overflow, moments, kinds, elements, sc, F, window, window * 2, dr)
    nbins = counts.shape[2]
    assert list(data.columns) == ["Time", "r", "Zn", "C", "H", "X"]
    assert list(alpha2.columns) == ["Time", "Zn", "C", "H", "X"]
    assert len(data) == len(window) * nbins and len(alpha2) == len(window)
    np.testing.assert_array_equal(data["r"].values[:nbins], np.arange(nbins) * dr)
    np.testing.assert_array_equal(data["Time"].values, np.repeat(window * 2, nbins))
    for s, z in enumerate(kinds):
        name = {1: "H", 6: "C", 30: "Zn"}[z]
        P = data[name].values.reshape(len(window), nbins)
        n = sc[z] * (F - window - 1)
        np.testing.assert_allclose((P * dr).sum(axis=1), 1.0 - overflow[s] / n, rtol=1e-12)
    X = data["X"].values.reshape(len(window), nbins)
    n_all = sum(sc.values()) * (F - window - 1)
    np.testing.assert_allclose(X, counts.sum(axis=0) / (n_all * dr)[:, None], rtol=1e-15)
    np.testing.assert_allclose(X.sum(axis=1) * dr, 1.0 - overflow.sum(axis=0) / n_all, rtol=1e-12)
    assert np.isnan(alpha2.iloc[0, 1:].values.astype(float)).all()
    assert np.isfinite(alpha2.iloc[1:, 1:].values.astype(float)).all()


def test_alpha2_vanishes_for_gaussian_moments():
    # a 3-D Gaussian displacement: <r^4> = (5/3) <r^2>^2
    counts, overflow, moments, kinds, sc, F, window, dr = _synthetic()
    for s, z in enumerate(kinds):
        n = sc[z] * (F - window - 1)
        msd = 0.3 * (1 + np.arange(len(window)))
        moments[s, :, 0] = n * msd
        moments[s, :, 1] = n * (5.0 / 3.0) * msd ** 2
    moments[:, 0] = 0.0
    _, alpha2 = vh.assemble(counts, overflow, moments, kinds, [1, 6, 30], sc, F, window, window, dr)
    vals = alpha2[["H", "C", "Zn", "X"]].values
    assert np.isnan(vals[0]).all()
    np.testing.assert_allclose(vals[1:], 0.0, atol=1e-14)


def test_empty_window_list_gives_the_columns():
    counts = np.zeros((2, 0, 10), np.uint64)
    data, alpha2 = vh.assemble(counts, np.zeros((2, 0), np.uint64), np.zeros((2, 0, 2)), [6, 30], [30, 6], {6: 2, 30: 1}, 5,
                               np.zeros(0, np.int64), np.zeros(0, np.int64), 0.1)
    assert list(data.columns) == ["Time", "r", "Zn", "C", "X"] and len(data) == 0
    assert list(alpha2.columns) == ["Time", "Zn", "C", "X"] and len(alpha2) == 0


def test_feather_round_trip(tmp_path):
    counts, overflow, moments, kinds, sc, F, window, dr = _synthetic()
    obj = vh.WindowVanHove()
    obj.data, obj.alpha2 = vh.assemble(counts, overflow, moments, kinds, [30, 6, 1], sc, F, window, window, dr)
    path = os.path.join(str(tmp_path), "run")
    obj.write_to_file(path)
    assert os.path.exists(path + ".vanhove") and os.path.exists(path + ".ngp")
    back = vh.WindowVanHove.from_file(path)
    pd.testing.assert_frame_equal(back.data, obj.data)
    pd.testing.assert_frame_equal(back.alpha2, obj.alpha2)


def test_abi_declares_and_exports_both_entry_points():
    header = open(os.path.join(ROOT, "include", "amof_hip.h")).read()
    declared = set(re.findall(r"\b(amof_[a-z0-9_]+)\s*\(", header))
    for name in ("amof_vanhove_window", "amof_vanhove_window_dev"):
        assert name in declared and name in _hip.EXPORTS
        assert hasattr(_hip.load_library(), name)
    doc = header[header.index("kernel family that produced the result of the last call"):header.index("const char *amof_last_path")]
    assert '"msd_vanhove"' in doc and '"msd_vanhove_global"' in doc


def test_restatement_counts_bins_by_the_definition():
    # two atoms of one species, steps of exactly known length along x (no cell crossing, no centre of mass removal)
    pos = np.zeros((4, 2, 3))
    pos[:, 0, 0] = [1.0, 1.25, 1.5, 2.0]
    pos[:, 1, 0] = [3.0, 3.0, 3.0, 3.0]
    packed = PackedTrajectory(pos, np.diag([10.0, 10.0, 10.0]), [6, 6])
    counts, overflow, moments, amb, kinds = ref.vanhove(packed, [0, 1, 2], 0.1, 4, remove_com=False)
    # m = 1: origins k = 1, 2: atom 0 moves 0.25, 0.5 (overflow: 0.5 / 0.1 = 5 >= 4); atom 1 stays
    assert counts[0, 1].tolist() == [2, 0, 1, 0] and overflow[0, 1] == 1
    assert counts[0, 0].tolist() == [6, 0, 0, 0] and overflow[0, 0] == 0      # m = 0: k = 1 .. 3
    assert counts[0, 2].tolist() == [1, 0, 0, 0] and overflow[0, 2] == 1       # k = 1: 0.75 and 0
    np.testing.assert_allclose(moments[0, 2], [0.75 ** 2, 0.75 ** 4])
    assert amb[0, 0, 0] == 6        # r = 0 sits on the left edge of bin 0
