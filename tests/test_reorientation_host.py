"""Bond reorientation without a GPU: the ABI surface, the restatement of tests/reorientation_ref.py against closed forms,
the scale rule, the host side of ``BondReorientation`` (columns, NaN rule, relaxation time, feather, refusal), and the cap on
the restatement's per-term error budget for every input of the GPU tests."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import bond_lifetime as bl
from amof_amd import bond_reorientation as br
from amof_amd import lags
from amof_amd.frames import PackedTrajectory
from tests import bond_ref
from tests import reorientation_cases as cases
from tests import reorientation_ref as ref
from tests.conftest import ROOT

BOX = np.diag([30.0, 30.0, 30.0])


def test_abi_surface():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        text = fh.read()
    for name in ("amof_bond_reorientation", "amof_bond_reorientation_dev"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _hip.EXPORTS
    comment = text[text.index("kernel family that produced"):text.index("const char *amof_last_path")]
    assert '"bond_reorient"' in comment and '"bond_reorient_exact"' in comment
    assert "#define AMOF_ABI_VERSION 4" in text and _hip.ABI_VERSION == 4
    assert hasattr(_hip.Context, "bond_reorientation")


def _rotor(F, omega, centre, radius=None):
    """one Zn at ``centre`` and one N on a circle about z around it, turned by omega per frame"""
    t = omega * np.arange(F)
    r = np.full(F, 2.0) if radius is None else radius
    pos = np.zeros((F, 2, 3))
    pos[:, 0] = centre
    pos[:, 1] = pos[:, 0] + np.stack([r * np.cos(t), r * np.sin(t), np.zeros(F)], axis=1)
    return pos


def test_restatement_rotating_pair_closed_form():
    F, omega = 40, 0.23
    windows = np.arange(0, 20)
    got = ref.reorientation(_rotor(F, omega, (15.0, 15.0, 15.0)), BOX, [30, 7], [(30, 7, 2.5)], windows)
    for w, m in enumerate(windows):
        n = F - m - 1
        assert got.n[0, w] == n
        c = np.cos(omega * m)
        assert got.sums[0, w, 0] / n == pytest.approx(c, abs=1e-14)
        assert got.sums[0, w, 1] / n == pytest.approx(0.5 * (3.0 * c * c - 1.0), abs=1e-14)
    assert got.sums[0, 0].tolist() == [F - 1.0, F - 1.0]       # lag 0: cos = 1 exactly
    assert 0.0 < got.worst < 2.0 ** -30


def test_restatement_intermittent_pair_counts_as_bond_ref():
    # the same pair leaves the cutoff periodically: bonded for the first q frames of every period p
    F, omega, p, q = 40, 0.1, 7, 4
    inside = (np.arange(F) % p) < q
    pos = _rotor(F, omega, (15.0, 15.0, 15.0), radius=np.where(inside, 2.0, 3.0))
    windows = np.arange(0, 3 * p + 1)
    got = ref.reorientation(pos, BOX, [30, 7], [(30, 7, 2.5)], windows)
    surv = bond_ref.survival(pos, BOX, [30, 7], [(30, 7, 2.5)], windows)
    assert np.array_equal(got.n[0], surv[0, :, 1].astype(np.int64))
    for w, m in enumerate(windows):
        assert got.n[0, w] == sum(1 for k in range(1, F - m) if inside[k] and inside[k + m])
        if got.n[0, w]:
            assert got.sums[0, w, 0] / got.n[0, w] == pytest.approx(np.cos(omega * m), abs=1e-14)
    got3 = ref.reorientation(pos, BOX, [30, 7], [(30, 7, 2.5)], [0, 2], stride=3)
    assert got3.n[0, 1] == sum(1 for k in range(1, F - 2, 3) if inside[k] and inside[k + 2])


def test_restatement_rotation_across_a_periodic_boundary():
    F, omega = 30, 0.31
    windows = [0, 1, 4, 11]
    inner = ref.reorientation(_rotor(F, omega, (15.0, 15.0, 15.0)), BOX, [30, 7], [(30, 7, 2.5)], windows)
    pos = _rotor(F, omega, (29.5, 0.25, 15.0))          # the N crosses two faces of the box while it turns
    pos -= np.floor(pos / 30.0) * 30.0
    assert np.any(np.abs(pos[:, 1] - pos[:, 0]) > 15.0)
    edge = ref.reorientation(pos, BOX, [30, 7], [(30, 7, 2.5)], windows)
    assert np.array_equal(edge.n, inner.n)
    np.testing.assert_allclose(edge.sums, inner.sums, rtol=0, atol=1e-12)


def test_scale_rule():
    for fn in (br.scale_log2, ref.scale_log2):
        assert fn(1, 1, 1) == 40 and fn(0, 5, 9) == 40
        assert fn(16, 64, 39) == 40                      # bit_length(39936) = 16: 62 - 16 = 46 -> capped
        assert fn(1 << 11, 1 << 11, 1) == 39             # 2^22 has 23 bits
        assert fn(576, 2304, 4999) == 62 - (576 * 2304 * 4999).bit_length() == 29
        assert fn(1 << 21, 1 << 20, 1) == 20             # 2^41: 42 bits
        assert fn((1 << 21) - 1, 1 << 21, 1) == 20
        with pytest.raises(ValueError):
            fn(1 << 21, 1 << 21, 1)                      # 2^42: 43 bits -> 19
        with pytest.raises(ValueError):
            fn(1 << 31, 1 << 31, 1 << 20)                # beyond 64 bits


def test_host_assembly_columns_nan_rule_and_relaxation_time():
    e = [20, 30]
    counts = np.array([[[10, 10 << 20, 10 << 20], [8, 4 << 20, -(2 << 20)], [0, 0, 0]],
                       [[4, 4 << 30, 4 << 30], [4, 2 << 30, 1 << 30], [4, -(1 << 30), 0]]], dtype=np.int64)
    time = np.array([0.0, 100.0, 200.0])
    names = [("Zn-N", True), ("Zn-Au", False), ("C-N", True)]
    data = br.assemble(counts, e, names, time)
    assert list(data.columns) == ["Time", "Zn-N-P1", "Zn-N-P2", "Zn-Au-P1", "Zn-Au-P2", "C-N-P1", "C-N-P2"]
    assert np.array_equal(data["Time"].values, time)
    assert data["Zn-N-P1"].values[:2].tolist() == [1.0, 0.5] and np.isnan(data["Zn-N-P1"].values[2])
    assert data["Zn-N-P2"].values[:2].tolist() == [1.0, -0.25] and np.isnan(data["Zn-N-P2"].values[2])
    assert np.all(np.isnan(data["Zn-Au-P1"].values)) and np.all(np.isnan(data["Zn-Au-P2"].values))
    assert data["C-N-P1"].values.tolist() == [1.0, 0.5, -0.25] and data["C-N-P2"].values.tolist() == [1.0, 0.25, 0.0]
    obj = br.BondReorientation()
    obj.data = data
    tau = obj.relaxation_time()
    assert tau["Zn-N"] == 100.0 * 0.5 * (1.0 - 0.25)                # the NaN lag ends the integral
    assert tau["C-N"] == 100.0 * 0.5 * (1.0 + 0.25) + 100.0 * 0.5 * (0.25 + 0.0)
    assert np.isnan(tau["Zn-Au"])
    tau1 = obj.relaxation_time(rank=1)
    assert tau1["C-N"] == 100.0 * 0.5 * (1.0 + 0.5) + 100.0 * 0.5 * (0.5 - 0.25)
    with pytest.raises(ValueError):
        obj.relaxation_time(rank=3)


def test_feather_round_trip(tmp_path):
    counts = np.array([[[5, 5 << 25, 5 << 25], [5, 1 << 25, -(1 << 25)]]], dtype=np.int64)
    obj = br.BondReorientation()
    obj.data = br.assemble(counts, [25], [("Zn-N", True), ("Zn-Au", False)], [0.0, 50.0])
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".reor")
    assert br.BondReorientation.from_file(path).data.equals(obj.data)


def test_shared_bookkeeping_is_bond_lifetimes():
    assert bl.min_periodic_height is lags.min_periodic_height
    rng = np.random.default_rng(3)
    packed = PackedTrajectory(rng.uniform(0, 4, (5, 6, 3)), np.diag([9.0, 9.0, 9.0]), np.array([30, 30, 7, 7, 7, 7]))
    rcm, names, live = lags.neighbour_sets(packed, {'Zn-N': 2.5, 'Zn-Au': 3.0, 'N-Zn': 2.5})
    assert names == [('Zn-N', True), ('Zn-Au', False), ('N-Zn', True)] and live == [(1, 0), (0, 1)]
    assert rcm[0, 1] == rcm[1, 0] == 2.5


def test_refusal_cutoff_above_half_height():
    rng = np.random.default_rng(3)
    packed = PackedTrajectory(rng.uniform(0, 4, (5, 6, 3)), np.diag([4.0, 9.0, 9.0]), np.array([30, 30, 7, 7, 7, 7]))
    with pytest.raises(ValueError):
        br.BondReorientation.from_trajectory(packed, {'Zn-N': 2.5}, delta_time=1, timestep=1, device=0, distributed=False)


@pytest.mark.parametrize("name", cases.NAMES)
def test_budget_cap_of_every_gpu_input(name):
    # a condition on the restatement's DERIVED budget, not a measurement: below 2^-30 per term nothing of O(0.1) can hide
    c = cases.case(name)
    for stride in c.strides:
        got = cases.reference(name, stride)
        assert got.n.sum() > 0
        assert 0.0 < got.worst < 2.0 ** -30, (name, stride, got.worst)
        assert np.all(got.budget[got.n > 0] < got.n[got.n > 0][:, None] * 2.0 ** -30)


def test_coincident_atoms_raise_in_the_restatement():
    p = cases.coincident()
    with pytest.raises(ZeroDivisionError):
        ref.reorientation(p.pos, p.cell, p.numbers, [(30, 7, 3.0)], [0, 1], pbc=tuple(p.pbc))


def test_rect_case_is_not_trivial():
    got = cases.reference("rect", 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        c2 = got.sums[0, :, 1] / got.n[0]
    assert np.any((c2 > 0.0) & (c2 < 0.9)), c2.tolist()
