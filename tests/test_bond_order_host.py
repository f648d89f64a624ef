"""Bond order parameters without a GPU: the ABI surface, the restatement of tests/bond_order_ref.py against the literature
values of ideal shells, the host side of ``BondOrder`` (``assemble``: means, f4, densities, NaN rules; feather), and the cap on
the restatement's per-term error budget for every input of the GPU tests."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import bond_order as bo
from tests import bond_order_cases as cases
from tests import bond_order_ref as ref
from tests.conftest import ROOT

TETRA = [(1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)]
SC = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
FCC = [s for s in [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)] if sum(abs(x) for x in s) == 2]


def test_abi_surface():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        text = fh.read()
    for name in ("amof_bond_order", "amof_bond_order_dev"):
        assert re.search(r"\bint %s\(" % name, text), name
        assert name in _hip.EXPORTS
    comment = text[text.index("kernel family that produced"):text.index("const char *amof_last_path")]
    assert '"order_frame"' in comment and '"order_exact"' in comment
    assert "#define AMOF_ABI_VERSION 4" in text and _hip.ABI_VERSION == 4
    assert hasattr(_hip.Context, "bond_order") and hasattr(_hip.MultiContext, "bond_order")


def test_restatement_literature_values_of_ideal_shells():
    q, qtet = ref.shell(TETRA, (3, 4, 6))
    assert q == pytest.approx([0.745356, 0.509175, 0.628539], abs=1e-6)
    assert q == pytest.approx([np.sqrt(5.0) / 3.0, np.sqrt(7.0 / 27.0), 4.0 * np.sqrt(2.0) / 9.0], abs=1e-12)
    assert qtet == pytest.approx(1.0, abs=1e-14)
    q, qtet = ref.shell(SC, (4, 6))
    assert q == pytest.approx([0.763763, 0.353553], abs=1e-6) and qtet is None
    assert q == pytest.approx([np.sqrt(7.0 / 12.0), np.sqrt(1.0 / 8.0)], abs=1e-12)
    q, _ = ref.shell(FCC, (4, 6))
    assert len(FCC) == 12 and q == pytest.approx([0.190941, 0.574524], abs=1e-6)
    assert q == pytest.approx([np.sqrt(7.0 / 192.0), np.sqrt(169.0 / 512.0)], abs=1e-12)


def test_restatement_odd_l_vanishes_on_centrosymmetric_shells_and_one_neighbour_gives_one():
    for shell in (SC, FCC):
        q, _ = ref.shell(shell, (1, 3, 5, 7, 9, 11))
        assert np.all(np.abs(q) < 1e-6), q            # sqrt of a float64 sum that cancels to ~1e-15
    rng = np.random.default_rng(2)
    for l in range(1, 13):
        q, qtet = ref.shell([rng.normal(size=3)], (l,))
        assert q == [1.0] and qtet is None


def test_restatement_qtet_range_on_random_quadruples():
    rng = np.random.default_rng(4)
    lo = 1.0
    for _ in range(300):
        q, qtet = ref.shell(rng.normal(size=(4, 3)), (4,))
        assert -3.0 <= qtet <= 1.0 and 0.0 <= q[0] <= 1.0 + 1e-15
        lo = min(lo, qtet)
    assert lo < 0.5
    v = np.array([1.0, 0.2, -0.4])
    _, qtet = ref.shell([v, v * 1.1, v * 0.7, v * 2.0], (4,))       # four neighbours in one direction: the lower end
    assert qtet == pytest.approx(-3.0, abs=1e-14)


def test_restatement_on_a_lattice_case_and_the_integer_formulas():
    packed, rc, n, shell = cases.lattice("diamond")
    got = ref.order(packed.pos, packed.cell, packed.numbers, [(30, 30, rc)], (3, 4, 6))
    assert np.all(got.n[0] == 4)
    want, _ = ref.shell(shell, (3, 4, 6))
    q = np.sqrt(np.maximum(0.0, 4 + 2.0 * got.T[0])) / 4
    assert np.all(np.abs(q - np.asarray(want)) < 1e-12) and np.all(np.abs(got.U[0]) < 1e-14)
    # the header's integer formulas (q_of, from_per_atom) and BondOrder's own copy (values) on hand-made integers
    one = 1 << 40
    pa = np.zeros((1, 1, 5, 4), dtype=np.int64)
    pa[0, 0, 0] = (-1, 0, 0, 0)                                     # not a centre
    pa[0, 0, 1] = (0, 0, 0, 0)                                      # no neighbour
    pa[0, 0, 2] = (1, 0, 0, 0)                                      # one: q = 1, the last bin
    pa[0, 0, 3] = (4, -one, 6 * one, 0)                             # Q = (2, 16) 2^40: q = (sqrt 2 / 4, 1); q_tet = 1
    pa[0, 0, 4] = (4, -2 * one - 1, 0, 8 * one)                     # Q clamps to 0; q_tet = 1 - 3 = -2
    for fn in (ref.q_of, bo.values):
        q, qt = fn(pa[0, 0, :, 0].clip(0), pa[0, 0, :, 1:3], pa[0, 0, :, 3])
        assert np.isnan(q[1]).all() and q[2].tolist() == [1.0, 1.0] and q[3].tolist() == [np.sqrt(2.0) / 4.0, 1.0]
        assert q[4].tolist() == [0.0, 0.5] and qt[3] == 1.0 and qt[4] == -2.0 and np.isnan(qt[2])
    hist, hist_tet, sums = ref.from_per_atom(pa, 2, 10, 8)
    assert hist[0, 0].tolist() == [1, 0, 0, 1, 0, 0, 0, 0, 0, 1] and hist[0, 1].tolist() == [0, 0, 0, 0, 0, 1, 0, 0, 0, 2]
    assert hist_tet[0].tolist() == [0, 0, 1, 0, 0, 0, 0, 1]         # (-2 + 3) / 4 * 8 = 2; q_tet = 1: right-closed
    assert sums[0, 0, :4].tolist() == [9, 3, 2, 12]
    assert sums[0, 0, 4:].tolist() == [(1 << 30) + int(np.rint(np.sqrt(2.0) / 4.0 * 2 ** 30)), (1 << 30) * 2 + (1 << 29),
                                       (1 << 30) - (2 << 30)]


def test_host_assembly_means_f4_densities_and_nan_rules():
    s30 = 1 << 30
    # two live sets (rows 0, 1), l = (4, 6), 4 bins / 2 bins, 3 frames; "Zn-Au": only B absent; "Au-Zn": A absent
    fs = np.zeros((3, 2, 7), dtype=np.int64)
    fs[0, 0] = (16, 4, 4, 24, 2 * s30, 3 * s30, 3 * s30)            # four centres, all with four neighbours
    fs[1, 0] = (5, 2, 1, 6, s30, s30 // 2, -s30)
    fs[2, 0] = (0, 0, 0, 0, 0, 0, 0)                                # nobody has a neighbour
    fs[:, 1] = (3, 3, 0, 0, 3 * s30, 3 * s30, 0)                    # three centres with one neighbour each
    counts = np.array([[[1, 2, 3, 0], [0, 0, 0, 6]], [[0, 0, 0, 9], [0, 0, 0, 9]]], dtype=np.uint64)
    counts_tet = np.array([[1, 4], [0, 0]], dtype=np.uint64)
    names = [("Zn-N", 4, True), ("Zn-Au", 4, False), ("N-Zn", 8, True), ("Au-Zn", 0, False)]
    data, hist, hist_tet = bo.assemble(counts, counts_tet, fs, names, (4, 6), np.arange(10, 40, 10))
    assert list(data.columns) == ["Step"] + [n + s for n in ("Zn-N", "Zn-Au", "N-Zn", "Au-Zn") for s in ("-q4", "-q6", "-qtet", "-f4")]
    assert data["Step"].tolist() == [10, 20, 30]
    assert data["Zn-N-q4"].tolist()[:2] == [0.5, 0.5] and np.isnan(data["Zn-N-q4"][2])
    assert data["Zn-N-q6"].tolist()[:2] == [0.75, 0.25] and np.isnan(data["Zn-N-q6"][2])
    assert data["Zn-N-qtet"].tolist()[:2] == [0.75, -1.0] and np.isnan(data["Zn-N-qtet"][2])
    assert data["Zn-N-f4"].tolist() == [1.0, 0.25, 0.0]
    assert data["N-Zn-q4"].tolist() == [1.0] * 3 and np.isnan(data["N-Zn-qtet"]).all() and data["N-Zn-f4"].tolist() == [0.0] * 3
    for col in ("-q4", "-q6", "-qtet"):
        assert np.isnan(data["Zn-Au" + col]).all() and np.isnan(data["Au-Zn" + col]).all()
    assert data["Zn-Au-f4"].tolist() == [0.0] * 3 and np.isnan(data["Au-Zn-f4"]).all()
    assert hist["q"].tolist() == [0.125, 0.375, 0.625, 0.875]
    assert hist["Zn-N-q4"].tolist() == [4.0 / 6, 8.0 / 6, 12.0 / 6, 0.0] and hist["Zn-N-q6"].tolist() == [0, 0, 0, 4.0]
    for col in ("Zn-N-q4", "Zn-N-q6", "N-Zn-q4", "N-Zn-q6"):
        assert np.sum(hist[col].values) * 0.25 == pytest.approx(1.0, abs=1e-15)
    assert np.isnan(hist["Zn-Au-q4"]).all() and np.isnan(hist["Au-Zn-q6"]).all()
    assert hist_tet["q"].tolist() == [-2.0, 0.0]
    assert hist_tet["Zn-N-qtet"].tolist() == [0.1, 0.4] and np.sum(hist_tet["Zn-N-qtet"].values) * 2.0 == pytest.approx(1.0)
    assert np.isnan(hist_tet["N-Zn-qtet"]).all()                    # nothing counted: no density


def test_feather_round_trip(tmp_path):
    fs = np.zeros((2, 1, 7), dtype=np.int64)
    fs[:, 0] = (8, 2, 2, 12, 1 << 30, 1 << 29, 1 << 30)
    obj = bo.BondOrder()
    obj.data = bo.assemble(np.ones((1, 2, 3), dtype=np.uint64), np.ones((1, 5), dtype=np.uint64), fs,
                           [("Zn-N", 2, True), ("Zn-Au", 2, False)], (4, 6), [0, 1])[0]
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".order")
    assert bo.BondOrder.from_file(path).data.equals(obj.data)


def test_arguments_refused_before_any_device_work():
    from amof_amd.frames import PackedTrajectory
    packed = PackedTrajectory(np.zeros((1, 2, 3)), np.diag([9.0, 9.0, 9.0]), np.array([30, 7]))
    for l in ((), (1, 2, 3, 4, 5), (0,), (13,)):
        with pytest.raises(ValueError):
            bo.BondOrder.from_trajectory(packed, {'Zn-N': 2.5}, l=l, device=0, distributed=False)


@pytest.mark.parametrize("name", cases.NAMES)
def test_budget_cap_of_every_gpu_input(name):
    # a condition on the restatement's DERIVED budget, not a measurement: below 2^-30 per term nothing of O(0.1) can hide
    got = cases.reference(name)
    assert sum(int(n.sum()) for n in got.n) > 0
    assert 0.0 < got.worst < 2.0 ** -30, (name, got.worst)


def test_cases_have_the_shapes_the_gpu_tests_rely_on():
    n = cases.reference("rect").n[0]
    assert n.shape == (7, 150) and n.min() == 0 and n.max() >= 12 and (n == 4).any() and n.max() <= 16
    zn, nz = cases.reference("zif4").n
    assert np.all(nz <= 1) and (nz == 1).mean() > 0.9 and (zn == 4).mean() > 0.9
    four = cases.reference("four")
    assert not four.n[4].any() and np.array_equal(four.n[0], four.n[5]) and four.n[0].sum() == four.n[1].sum() > 0
    assert sorted(cases.reference("cluster").n[0][0].tolist()) == sorted(cases.CLUSTER_COUNTS)
    for name in ("sheared", "npt_diag", "npt_sheared", "open"):     # shells of a few neighbours, four among them, none beyond 16
        counts = np.concatenate([x.ravel() for x in cases.reference(name).n])
        assert (counts == 4).sum() >= 5 and counts.max() <= 16 and (counts >= 2).mean() > 0.5, (name, np.bincount(counts).tolist())
    for kind, want in (("sc", 6), ("fcc", 12), ("diamond", 4)):
        packed, rc, nn, shell = cases.lattice(kind)
        assert nn == want == len(shell) and rc < 0.5 * packed.cell[0, 0, 0]


def test_coincident_atoms_raise_in_the_restatement():
    p = cases.coincident()
    with pytest.raises(ZeroDivisionError):
        ref.order(p.pos, p.cell, p.numbers, [(30, 7, 3.4)], (4,), pbc=tuple(p.pbc))
