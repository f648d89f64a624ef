"""IntermediateScattering without a GPU: the C ABI declarations, the float64 restatement (tests/isf_ref.py) against S(q)'s
at lag 0 and against a rigid translation's closed form, and the host assembly of the DataFrame from raw sums."""

import os
import re

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip
from amof_amd import intermediate_scattering as isc
from amof_amd.frames import PackedTrajectory
from tests import helpers as H
from tests import isf_ref
from tests import sq_ref
from tests.conftest import ROOT

TRICLINIC = np.array([[9.0, 0.0, 0.0], [2.5, 8.5, 0.0], [-1.5, 2.0, 9.5]])


def test_abi_declares_and_exports_the_entry_points():
    header = open(os.path.join(ROOT, "include", "amof_hip.h")).read()
    declared = set(re.findall(r"\b(amof_[a-z0-9_]+)\s*\(", header))
    for name in ("amof_isf_accumulate", "amof_isf_accumulate_dev"):
        assert name in declared and name in _hip.EXPORTS
        assert hasattr(_hip.load_library(), name)
    doc = header[header.index("kernel family that produced the result of the last call"):header.index("const char *amof_last_path")]
    assert '"isf"' in doc and '"isf_global"' in doc
    assert "#define AMOF_ABI_VERSION 4" in header


def _gas(F=6, seed=1, jitter=0.0):
    rng = np.random.default_rng(seed)
    numbers = [30] * 2 + [7] * 9 + [6] * 5
    cells = np.array([TRICLINIC * (1.0 + jitter * rng.normal()) for _ in range(F)]) if jitter else TRICLINIC
    frac = rng.random((F, len(numbers), 3))
    pos = np.einsum("fnk,fkc->fnc", frac, cells) if jitter else frac @ TRICLINIC
    return PackedTrajectory(pos, cells, numbers)


@pytest.mark.parametrize("jitter,stride", [(0.0, 1), (0.02, 1), (0.0, 2)])
def test_lag_zero_is_the_structure_factor_of_the_origin_frames(jitter, stride):
    packed = _gas(jitter=jitter)
    hkl = np.array([[1, 0, 0], [0, 1, 0], [1, -1, 2], [2, 1, 0], [0, 0, 3], [3, -2, 1], [2, 2, 2]])
    dq, nbins = 0.4, 6
    counts, coh, selfs, beyond, kinds = isf_ref.isf(packed, hkl, [0, 2], dq, nbins, origin_stride=stride)
    c0, s0, b0, k0 = sq_ref.sq(packed, hkl, dq, nbins, frames=range(1, len(packed), stride))
    assert list(kinds) == list(k0)
    assert np.array_equal(counts[0], c0) and beyond[0] == b0 and counts[0].sum() > 0
    p = 0
    for a in range(len(kinds)):
        for c in range(a, len(kinds)):
            np.testing.assert_allclose(coh[a, c, 0], s0[p], rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(coh[c, a, 0], s0[p], rtol=1e-12, atol=1e-12)
            p += 1
    # no displacement at lag 0: every atom contributes cos(0)
    n = np.array([(np.asarray(packed.numbers) == z).sum() for z in kinds], dtype=np.float64)
    np.testing.assert_allclose(selfs[:, 0], n[:, None] * counts[0][None, :], rtol=1e-12)
    # lag 2 has fewer origins
    assert counts[1].sum() + beyond[1] == len(isf_ref.origins(len(packed), 2, stride)) * len(hkl)


def test_rigid_translation_pins_sign_and_order():
    """every atom moved by f d per frame: rho_a(k + m) = rho_a(k) exp(i theta), theta = q . d m, so with z = rho_a rho_c*
    of the origin frame (invariant under the translation) coh_ac = n_w (Re z cos theta + Im z sin theta) and
    coh_ca carries the opposite sign on the sine term; self_a = n_w N_a cos theta"""
    rng = np.random.default_rng(5)
    numbers = [8] * 7 + [1] * 12
    F = 7
    base = rng.random((len(numbers), 3)) @ TRICLINIC
    d = np.array([0.31, -0.17, 0.23])
    pos = base[None] + np.arange(F)[:, None, None] * d[None, None, :]
    packed = PackedTrajectory(pos, TRICLINIC, numbers)
    hkl = np.array([[1, 0, 0], [1, 1, 0], [2, -1, 1], [3, 0, -2]])        # |q| = 0.70, 1.01, 1.65, 2.50: alone in their bins
    dq, nbins = 0.1, 30
    R = sq_ref.reciprocal(TRICLINIC)
    b = sq_ref.bins(R, hkl, dq, nbins)
    assert len(set(b.tolist())) == len(hkl) and (b < nbins).all()
    windows = [0, 1, 3]
    counts, coh, selfs, beyond, kinds = isf_ref.isf(packed, hkl, windows, dq, nbins)
    _, sp = H.species_of(numbers)
    rho = sq_ref.modes(pos[1], TRICLINIC, sp, 2, hkl)
    n = np.array([(sp == a).sum() for a in range(2)], dtype=np.float64)
    q = hkl.astype(np.float64) @ R                                         # rows of R are the reciprocal vectors
    sines = []
    for w, m in enumerate(windows):
        n_w = len(isf_ref.origins(F, m))
        theta = (q @ d) * m
        assert (counts[w][b] == n_w).all() and beyond[w] == 0
        for a in range(2):
            np.testing.assert_allclose(selfs[a, w][b], n_w * n[a] * np.cos(theta), atol=1e-9 * n[a] * n_w)
            for c in range(2):
                z = rho[:, a] * np.conj(rho[:, c])
                want = n_w * (z.real * np.cos(theta) + z.imag * np.sin(theta))
                np.testing.assert_allclose(coh[a, c, w][b], want, atol=1e-9 * n[a] * n[c] * n_w)
        z = rho[:, 0] * np.conj(rho[:, 1])
        sines.append(np.abs(z.imag * np.sin(theta)).max())
        # coh_01 - coh_10 = 2 n_w Im z sin theta: the order (origin, origin + lag) is visible
        np.testing.assert_allclose(coh[0, 1, w][b] - coh[1, 0, w][b], 2 * n_w * z.imag * np.sin(theta), atol=1e-9 * n[0] * n[1] * n_w)
    assert sines[0] == 0.0 and min(sines[1:]) > 1.0            # (the sine term is not accidentally absent)


def _synthetic(seed=2, W=3, nbins=5):
    rng = np.random.default_rng(seed)
    kinds = [1, 8, 30]
    sc = {1: 6, 8: 3, 30: 1}
    counts = rng.integers(1, 5, size=(W, nbins)).astype(np.uint64)
    counts[:, 0] = 0
    counts[1, 3] = 0
    coh = rng.normal(size=(3, 3, W, nbins)) * counts
    coh[:, :, 0] = 0.5 * (coh[:, :, 0] + coh[:, :, 0].transpose(1, 0, 2)) + 3.0 * counts[0]     # lag 0: symmetric, nonzero
    selfs = rng.random(size=(3, W, nbins)) * counts * np.array([6.0, 3.0, 1.0])[:, None, None]
    selfs[:, 0] = np.array([6.0, 3.0, 1.0])[:, None] * counts[0]
    return counts, coh, selfs, kinds, sc


def test_assembly_from_raw_sums():
    counts, coh, selfs, kinds, sc = _synthetic()
    time = [0.0, 100.0, 200.0]
    data = isc.assemble(counts, coh, selfs, kinds, [30, 8, 1], sc, time, 0.05)
    names = ["Zn", "O", "H"]
    assert list(data.columns) == (["Time", "q", "X-X"] + [a + "-" + b for a in names for b in names] +
                                  [a + "-self" for a in names] + ["X-self"])
    assert list(data.columns) == isc.column_names([30, 8, 1])
    assert len(data) == 3 * 5
    np.testing.assert_array_equal(data["Time"].values, np.repeat(time, 5))
    np.testing.assert_array_equal(data["q"].values, np.tile(np.arange(5) * 0.05, 3))
    c = counts.astype(float)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_allclose(data["X-X"].values, (coh.sum(axis=(0, 1)) / (c * 10)).reshape(-1), rtol=1e-14)
        # library order H, O, Zn: "O-Zn" is O at the origin = coh[1][2]; "Zn-O" = coh[2][1] (not the same at t > 0)
        np.testing.assert_allclose(data["O-Zn"].values, (coh[1, 2] / (c * np.sqrt(3.0))).reshape(-1), rtol=1e-14)
        np.testing.assert_allclose(data["Zn-O"].values, (coh[2, 1] / (c * np.sqrt(3.0))).reshape(-1), rtol=1e-14)
        np.testing.assert_allclose(data["H-self"].values, (selfs[0] / (c * 6.0)).reshape(-1), rtol=1e-14)
        np.testing.assert_allclose(data["X-self"].values, (selfs.sum(axis=0) / (c * 10)).reshape(-1), rtol=1e-14)
    empty = (counts == 0).reshape(-1)
    assert np.isnan(data.iloc[empty, 2:].values).all() and np.isfinite(data.iloc[~empty].values).all()
    # X-X is the c-weighted sum of the Ashcroft-Langreth partials; X-self of the self columns
    n = {"H": 6.0, "O": 3.0, "Zn": 1.0}
    xx = sum(np.sqrt(n[a] * n[b]) / 10.0 * data[a + "-" + b].values for a in names for b in names)
    xs = sum(n[a] / 10.0 * data[a + "-self"].values for a in names)
    np.testing.assert_allclose(xx[~empty], data["X-X"].values[~empty], rtol=1e-12)
    np.testing.assert_allclose(xs[~empty], data["X-self"].values[~empty], rtol=1e-12)
    # without the self part the columns are absent
    short = isc.assemble(counts, coh, None, kinds, [30, 8, 1], sc, time, 0.05)
    assert list(short.columns) == isc.column_names([30, 8, 1], self_part=False) == list(data.columns)[:12]


def _object(window=(0, 100, 200)):
    counts, coh, selfs, kinds, sc = _synthetic()
    obj = isc.IntermediateScattering()
    obj.kinds, obj.counts, obj.coh, obj.self_sums, obj.dq, obj.species_counts = kinds, counts, coh, selfs, 0.05, sc
    obj.window, obj.time = np.asarray(window), np.asarray(window, dtype=float)
    obj.data = isc.assemble(counts, coh, selfs, kinds, [30, 8, 1], sc, obj.time, 0.05)
    return obj


def test_normalised_and_weighted():
    obj = _object()
    nrm = obj.normalised()
    assert list(nrm.columns) == list(obj.data.columns)
    np.testing.assert_array_equal(nrm["Time"].values, obj.data["Time"].values)
    np.testing.assert_array_equal(nrm["q"].values, obj.data["q"].values)
    ok = (np.asarray(obj.counts) > 0)
    first = nrm.iloc[:5]
    assert (first["X-X"].values[ok[0]] == 1.0).all() and (first["H-self"].values[ok[0]] == 1.0).all()
    v = obj.data["O-O"].values.reshape(3, 5)
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_allclose(nrm["O-O"].values.reshape(3, 5)[2], v[2] / v[0], rtol=1e-14)
    with pytest.raises(ValueError):
        _object(window=(100, 200, 300)).normalised()
    for w in (1.0, 2.5):
        got = obj.weighted({"H": w, "O": w, "Zn": w})
        assert list(got.columns) == ["Time", "q", "F"]
        np.testing.assert_allclose(got["F"].values, obj.data["X-X"].values, rtol=1e-12)
    got = obj.weighted({1: lambda q: 0.0 * q, 8: 0.0, 30: lambda q: 1.0 + q})
    np.testing.assert_allclose(got["F"].values, obj.data["Zn-Zn"].values, rtol=1e-12)
    with pytest.raises(KeyError):
        obj.weighted({"H": 1.0, "O": 1.0})


def test_feather_round_trip(tmp_path):
    obj = _object()
    path = os.path.join(str(tmp_path), "run")
    obj.write_to_file(path)
    assert os.path.exists(path + ".isf")
    pd.testing.assert_frame_equal(isc.IntermediateScattering.from_file(path).data, obj.data)


def test_argument_errors_need_no_gpu():
    rng = np.random.default_rng(1)

    def packed(pbc=(True, True, True)):
        return PackedTrajectory(rng.random((4, 6, 3)) * 8.0, np.diag([8.0, 8.0, 8.0]), [8, 8, 1, 1, 1, 1], pbc=pbc)
    kw = dict(delta_time=1, distributed=False)
    with pytest.raises(ValueError):
        isc.IntermediateScattering.from_trajectory(packed(pbc=(True, True, False)), **kw)
    with pytest.raises(ValueError):
        isc.IntermediateScattering.from_trajectory(packed(), dq=0.0, **kw)
    with pytest.raises(ValueError):
        isc.IntermediateScattering.from_trajectory(packed(), dq=1.0, qmax=0.5, **kw)
    with pytest.raises(ValueError):
        isc.IntermediateScattering.from_trajectory(packed(), origin_stride=0, **kw)
    with pytest.raises(ValueError):
        isc.IntermediateScattering().compute_isf(packed(), [0, 4], [0.0, 4.0], distributed=False)      # lag >= F


def test_layout_of_the_merged_tensor():
    lay = _hip.isf_layout(3, 4, 10, True)
    assert lay == {"counts": 0, "beyond": 40, "coh": 44, "self": 44 + 360, "size": 44 + 360 + 120}
    assert _hip.isf_layout(3, 4, 10, False)["size"] == 44 + 360
