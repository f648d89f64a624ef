"""Bond survival without a GPU: the ABI surface, the restatement of tests/bond_ref.py against closed forms, and the host
side of ``BondLifetime`` (columns, NaN rule, lifetime, refusal)."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import bond_lifetime as bl
from amof_amd.frames import PackedTrajectory
from amof_amd.lags import n_origins
from tests import bond_ref as ref
from tests import helpers as H
from tests.conftest import ROOT


def _header():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        return fh.read()


def test_abi_surface():
    text = _header()
    for name in ("amof_bond_survival", "amof_bond_survival_dev"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _hip.EXPORTS
    declared = set(re.findall(r"\b(amof_[a-z0-9_]+)\s*\(", text))
    assert declared == set(_hip.EXPORTS)
    comment = text[text.index("kernel family that produced"):text.index("const char *amof_last_path")]
    assert '"bond_series"' in comment and '"bond_series_exact"' in comment
    assert "#define AMOF_ABI_VERSION 4" in text and _hip.ABI_VERSION == 4


def test_restatement_against_closed_forms():
    # one Zn - N pair in a big box; the N oscillates across rc with period p: bonded for the first q frames of a period
    p, q, F, rc = 7, 4, 40, 2.5
    pos = np.zeros((F, 2, 3))
    pos[:, 0] = (5.0, 5.0, 5.0)
    inside = (np.arange(F) % p) < q
    pos[:, 1] = pos[:, 0] + np.where(inside, 2.0, 3.0)[:, None] * np.array([1.0, 0.0, 0.0])
    windows = np.arange(0, 3 * p + 1)
    got = ref.survival(pos, np.diag([30.0, 30.0, 30.0]), [30, 7], [(30, 7, rc)], windows)[0]
    for w, m in enumerate(windows):
        ks = [k for k in range(1, F - m) if inside[k]]
        assert got[w, 0] == len(ks)
        # intermittent: bonded again whenever (k + m) mod p < q -- the full count recurs at every multiple of p
        assert got[w, 1] == sum(1 for k in ks if (k + m) % p < q)
        if m % p == 0:
            assert got[w, 1] == got[w, 0]
        # continuous: the bond survives m frames only inside its own stretch, never beyond the first crossing
        assert got[w, 2] == sum(1 for k in ks if (k % p) + m < q)
        if m >= q:
            assert got[w, 2] == 0
    assert np.all(got[:, 2] <= got[:, 1]) and np.all(got[:, 1] <= got[:, 0])
    # stride 3 picks the origins 1, 4, 7, ...
    got3 = ref.survival(pos, np.diag([30.0, 30.0, 30.0]), [30, 7], [(30, 7, rc)], [0, 2], stride=3)[0]
    assert got3[0, 0] == sum(1 for k in range(1, F, 3) if inside[k])
    assert got3[1, 2] == sum(1 for k in range(1, F - 2, 3) if (k % p) + 2 < q)


def test_fixture_tie_static_zif4():
    z = H.zif4_frame()
    F = 6
    pos = np.repeat(z.positions[None], F, axis=0)
    windows = [0, 1, 2, 4]
    got = ref.survival(pos, z.cell, z.numbers, [(30, 7, 2.5)], windows, pbc=tuple(z.pbc))[0]
    n = n_origins(F, windows)
    assert np.array_equal(got[:, 0], 64 * n.astype(np.uint64))      # 16 Zn with four N each
    assert np.array_equal(got[:, 1], got[:, 0]) and np.array_equal(got[:, 2], got[:, 0])     # C = S = 1 at every lag


def test_zif4_walk_breaks_and_reforms_bonds():
    # the fixture of the GPU test: the seed and length must give a lag with 0 < continuous < intermittent < bonds
    tr = H.random_walk(H.zif4_frame(), 80, 0.05, 5)
    got = ref.survival(tr.pos, tr.cell, tr.numbers, [(30, 7, 2.5)], [0, 5, 20, 40], pbc=tuple(tr.pbc))[0]
    assert any(0 < c[2] < c[1] < c[0] for c in got), got.tolist()


def test_host_assembly_columns_nan_rule_and_lifetime():
    counts = np.array([[[10, 10, 10], [8, 6, 4], [0, 0, 0]],
                       [[4, 4, 4], [4, 2, 2], [4, 1, 0]]], dtype=np.uint64)
    time = np.array([0.0, 100.0, 200.0])
    names = [("Zn-N", True), ("Zn-Au", False), ("C-N", True)]
    data = bl.assemble(counts, names, time)
    assert list(data.columns) == ["Time", "Zn-N", "Zn-N-continuous", "Zn-Au", "Zn-Au-continuous", "C-N", "C-N-continuous"]
    assert np.array_equal(data["Time"].values, time)
    assert data["Zn-N"].values[:2].tolist() == [1.0, 6 / 8] and np.isnan(data["Zn-N"].values[2])
    assert data["Zn-N-continuous"].values[:2].tolist() == [1.0, 4 / 8] and np.isnan(data["Zn-N-continuous"].values[2])
    assert np.all(np.isnan(data["Zn-Au"].values)) and np.all(np.isnan(data["Zn-Au-continuous"].values))
    assert data["C-N"].values.tolist() == [1.0, 0.5, 0.25] and data["C-N-continuous"].values.tolist() == [1.0, 0.5, 0.0]
    obj = bl.BondLifetime()
    obj.data = data
    tau = obj.lifetime()
    assert tau["Zn-N"] == 100.0 * 0.5 * (1.0 + 0.5)                 # the NaN lag ends the integral
    assert tau["C-N"] == 100.0 * 0.5 * (1.0 + 0.5) + 100.0 * 0.5 * (0.5 + 0.0)
    assert np.isnan(tau["Zn-Au"])


def test_min_periodic_height():
    sheared = np.array([[10.0, 0.0, 0.0], [5.0, 8.0, 0.0], [0.0, 0.0, 30.0]])
    assert bl.min_periodic_height(sheared, (True, True, True)) == pytest.approx(8.0)
    assert bl.min_periodic_height(sheared, (True, False, True)) == pytest.approx(80.0 / np.hypot(5.0, 8.0))
    assert bl.min_periodic_height(np.stack([sheared, 0.5 * sheared]), (False, False, True)) == pytest.approx(15.0)
    assert bl.min_periodic_height(sheared, (False, False, False)) == np.inf


def test_refusal_cutoff_above_half_height():
    rng = np.random.default_rng(3)
    packed = PackedTrajectory(rng.uniform(0, 4, (5, 6, 3)), np.diag([4.0, 9.0, 9.0]), np.array([30, 30, 7, 7, 7, 7]))
    with pytest.raises(ValueError):
        bl.BondLifetime.from_trajectory(packed, {'Zn-N': 2.5}, delta_time=1, timestep=1, device=0, distributed=False)
