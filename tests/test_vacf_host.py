"""VelocityAutocorrelation without a GPU: the host assembly from raw sums, the numpy restatement on cases known by hand, the
Fourier transform of an analytic C(t), the file round trip and the C ABI declarations."""

import os
import re

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip
from amof_amd import lags
from amof_amd import vacf
from amof_amd.frames import PackedTrajectory
from tests import vacf_ref as ref
from tests.conftest import ROOT


def _synthetic(W=5, seed=2):
    rng = np.random.default_rng(seed)
    kinds = [1, 6, 30]
    species_counts = {1: 5, 6: 3, 30: 1}
    F = 12
    window = np.arange(W) * 2
    n = lags.n_origins(F, window)
    sums = rng.normal(size=(3, W))
    return sums, n, kinds, species_counts, window


def test_assembly_columns_division_and_pooling():
    sums, n, kinds, sc, window = _synthetic()
    data = vacf.assemble(sums, n, kinds, [30, 6, 1], sc, window * 2, 2)
    assert list(data.columns) == ["Time", "Zn", "C", "H", "X"] and len(data) == len(window)
    np.testing.assert_array_equal(data["Time"].values, window * 2)
    for s, (z, name) in enumerate(zip(kinds, ("H", "C", "Zn"))):
        np.testing.assert_allclose(data[name].values, sums[s] / (sc[z] * n) / 4.0, rtol=1e-15)
    np.testing.assert_allclose(data["X"].values, sums.sum(axis=0) / (9 * n) / 4.0, rtol=1e-15)
    # X is the number-weighted mean of the element columns
    np.testing.assert_allclose(data["X"].values, (5 * data["H"] + 3 * data["C"] + data["Zn"]).values / 9, rtol=1e-13)


def test_assembly_nan_without_origins_and_empty_window_list():
    sums, _, kinds, sc, _ = _synthetic(W=3)
    data = vacf.assemble(sums, [4, 0, 1], kinds, [1, 6, 30], sc, [0, 1, 2], 1)
    assert np.isnan(data.iloc[1, 1:].values.astype(float)).all()
    assert np.isfinite(data.iloc[[0, 2], 1:].values.astype(float)).all()
    empty = vacf.assemble(np.zeros((2, 0)), np.zeros(0, np.int64), [6, 30], [30, 6], {6: 2, 30: 1}, np.zeros(0, np.int64), 1)
    assert list(empty.columns) == ["Time", "Zn", "C", "X"] and len(empty) == 0


def test_restatement_on_a_case_computed_by_hand():
    # atom 0 steps 0.25, 0.25, 0.5 along x, atom 1 rests: no cell crossing, no centre of mass
    pos = np.zeros((4, 2, 3))
    pos[:, 0, 0] = [1.0, 1.25, 1.5, 2.0]
    pos[:, 1, 0] = 3.0
    packed = PackedTrajectory(pos, np.diag([10.0, 10.0, 10.0]), [6, 6])
    sums, n, abs_sums, kinds = ref.vacf(packed, [0, 1, 2, 3], remove_com=False)
    assert kinds == [6] and n.tolist() == [3, 2, 1, 0]
    # lag 0: k = 1, 2, 3; lag 1: d1 d2 + d2 d3; lag 2: d1 d3; lag 3: no origin
    np.testing.assert_allclose(sums[0], [0.0625 + 0.0625 + 0.25, 0.0625 + 0.125, 0.125, 0.0], rtol=1e-14)
    np.testing.assert_allclose(abs_sums, sums, rtol=1e-14)
    # every second origin
    sums2, n2, _, _ = ref.vacf(packed, [0, 1], origin_stride=2, remove_com=False)
    assert n2.tolist() == [2, 1]
    np.testing.assert_allclose(sums2[0], [0.0625 + 0.25, 0.0625], rtol=1e-14)
    # velocity mode: the values themselves, frame 0 never an origin; the mean of equal masses removed
    vel = np.zeros((3, 2, 3))
    vel[:, 0, 1] = [5.0, 1.0, 3.0]
    vel[:, 1, 1] = [7.0, -1.0, 1.0]
    vp = PackedTrajectory(vel, np.eye(3), [6, 6])
    s, n, a, _ = ref.vacf(vp, [0, 1], velocity_mode=True, remove_com=False)
    assert n.tolist() == [2, 1]
    np.testing.assert_allclose(s[0], [1 + 9 + 1 + 1, 3 - 1]), np.testing.assert_allclose(a[0], [12, 4])
    s, _, _, _ = ref.vacf(vp, [0, 1], velocity_mode=True, remove_com=True)       # x = +-1, +-1 about the means 0, 2
    np.testing.assert_allclose(s[0], [4.0, 2.0])


def test_restatement_ballistic_known_answer():
    v = np.array([0.031, -0.052, 0.017])
    F = 41
    start = np.array([[1.0, 5.0, 3.0], [4.0, 6.0, 2.0], [7.5, 4.0, 6.0]])
    pos = start[None] + np.arange(F)[:, None, None] * v[None, None, :]
    packed = PackedTrajectory(pos, np.diag([20.0, 20.0, 20.0]), [8, 8, 1])
    window, time = lags.window_setup(F, 2, "half", 2)
    sums, n, _, kinds = ref.vacf(packed, window, remove_com=False)
    data = vacf.assemble(sums, n, kinds, [1, 8], {1: 1, 8: 2}, time, 2)
    for name in ("H", "O", "X"):
        np.testing.assert_allclose(data[name].values, v @ v / 4.0, rtol=1e-11)


def _analytic(M=400, dt=2.0, period=37.0):
    obj = vacf.VelocityAutocorrelation()
    t = dt * np.arange(M)
    c = np.cos(2 * np.pi * t / period)
    obj.data = pd.DataFrame({"Time": t, "O": c, "X": c})
    obj.timestep = dt
    return obj, 1.0 / period


def test_vdos_peak_of_an_analytic_cosine():
    obj, nu0 = _analytic()
    for kw in (dict(), dict(window=None, pad=1), dict(fd_correction=False, pad=2)):
        d = obj.vdos(**kw)
        assert list(d.columns) == ["Frequency_THz", "Wavenumber_cm-1", "O", "X"]
        f = d["Frequency_THz"].values
        assert abs(f[np.argmax(d["O"].values)] - nu0 * 1e3) <= f[1] - f[0]
        np.testing.assert_allclose(d["Wavenumber_cm-1"].values, f * 33.3564095, rtol=1e-8)
        assert len(d) == kw.get("pad", 4) * len(obj.data) + 1


def test_vdos_discrete_sum_rule():
    obj, _ = _analytic(M=257, dt=0.5, period=11.3)
    obj.data["O"] = obj.data["O"] * 0.37 + 0.02
    for pad in (1, 3):
        d = obj.vdos(window=None, pad=pad, fd_correction=False)
        dnu = (d["Frequency_THz"].values[1] - d["Frequency_THz"].values[0]) / 1e3      # 1 / fs
        for name in ("O", "X"):
            D = d[name].values
            total = 2.0 * dnu * (D.sum() - 0.5 * (D[0] + D[-1]))
            assert abs(total - obj.data[name].values[0]) <= 1e-12 * abs(obj.data[name].values[0])


def test_vdos_weights_and_correction():
    obj, _ = _analytic()
    obj.data["H"] = np.cos(2 * np.pi * obj.data["Time"].values / 9.0)
    obj.data = obj.data[["Time", "O", "H", "X"]]
    obj.weights = {"O": 16.0, "H": 2.0}
    plain, corrected = obj.vdos(fd_correction=False), obj.vdos(fd_correction=True)
    np.testing.assert_allclose(plain["X"].values, (16.0 * plain["O"].values + 2.0 * plain["H"].values) / 18.0, rtol=1e-13, atol=1e-13)
    nu = plain["Frequency_THz"].values / 1e3
    np.testing.assert_allclose(corrected["O"].values * np.sinc(nu * 2.0) ** 2, plain["O"].values, rtol=1e-12, atol=1e-12)
    assert obj.normalised()["H"].values[0] == 1.0


def test_vdos_refuses_uneven_lags():
    obj, _ = _analytic(M=6)
    for t in ([0, 2, 4, 7, 8, 10], [2, 4, 6, 8, 10, 12]):
        obj.data["Time"] = np.array(t, dtype=float)
        with pytest.raises(ValueError):
            obj.vdos()


def test_diffusion_is_a_third_of_the_trapezoid_integral():
    obj = vacf.VelocityAutocorrelation()
    obj.data = pd.DataFrame({"Time": [0.0, 2.0, 4.0], "O": [3.0, 1.0, -1.0], "X": [6.0, 0.0, 0.0]})
    assert obj.diffusion() == {"O": (4.0 + 0.0) / 3.0, "X": 6.0 / 3.0}


def test_feather_round_trip(tmp_path):
    sums, n, kinds, sc, window = _synthetic()
    obj = vacf.VelocityAutocorrelation()
    obj.data = vacf.assemble(sums, n, kinds, [30, 6, 1], sc, window, 1)
    path = os.path.join(str(tmp_path), "run")
    obj.write_to_file(path)
    assert os.path.exists(path + ".vacf")
    back = vacf.VelocityAutocorrelation.from_file(path)
    pd.testing.assert_frame_equal(back.data, obj.data)


def test_abi_declares_and_exports_both_entry_points():
    header = open(os.path.join(ROOT, "include", "amof_hip.h")).read()
    declared = set(re.findall(r"\b(amof_[a-z0-9_]+)\s*\(", header))
    for name in ("amof_vacf_window", "amof_vacf_window_dev"):
        assert name in declared and name in _hip.EXPORTS
        assert hasattr(_hip.load_library(), name)
    doc = header[header.index("kernel family that produced the result of the last call"):header.index("const char *amof_last_path")]
    assert '"vacf_lds"' in doc and '"vacf_general"' in doc
    assert _hip.ABI_VERSION == 4 and "#define AMOF_ABI_VERSION 4" in header
