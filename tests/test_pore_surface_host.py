"""Host side of the surface stage, no GPU: the restatement (tests/pore_surface_ref.py) on every case of
tests/pore_surface_cases.py -- the cap on its budget, and that NO sample is a near decision, so that the GPU tests may ask for
exact equality (a condition, not a measurement: with about 1e5 samples and 30 neighbours each, a budget of 1e-13 A and a
spread of the values over an Angstrom, of order 1e-6 accidental hits are expected; a seed that produces one is changed) --
``sphere_points``, ``surface_columns``, the header's declarations and the unchanged defaults of ``pore_names``."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from tests import pore_cases
from tests import pore_surface_cases as scases
from tests import pore_surface_ref as sref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", scases.NAMES + scases.FORMS)
def test_restatement_budget_and_no_near_decisions(name):
    c = scases.case(name)
    p = c.packed
    ref = scases.reference(name)
    assert len(ref) == p.pos.shape[0] and len(ref[0]) == 3
    total = 0
    for f, row in enumerate(ref):
        for fr in row:
            assert fr.worst <= 1e-10, (name, f, fr.worst)
            assert sref.near_decisions(fr, scases._cell(p, f), c.grid, tuple(p.pbc)) == [], name
            assert fr.exposed.shape == (len(p.numbers), len(c.dirs))
            total += int(fr.exposed.sum())
    # the cases decide something: samples of both kinds on the van der Waals surface, fewer exposed ones at the largest probe
    if len(c.dirs) > 1:
        first = ref[0][0].exposed
        assert 0 < first.sum() < first.size
        assert first.sum() > ref[0][-1].exposed.sum()
    assert total > 0


def test_planted_samples_are_decided_by_the_construction():
    packed, dirs, plants = scases.planted()
    d_small, d_band = scases.plant_deltas()
    assert d_small == 2.0 ** -26 and 1e-7 < d_band < 1e-5
    R = np.full(5, pore_cases.TABLE[30])
    for f, k, sd in plants:
        fr = sref.frame(packed.pos[f], pore_cases.PLANT_CELL, R, scases.PLANT_THR[k], dirs, (True, True, True))
        assert fr.worst <= 1e-10 and abs(sd) > 1e4 * fr.worst
        assert bool(fr.exposed[0, scases.PLANT_SAMPLE]) == (sd > 0), (f, k, sd)
        assert sref.near_decisions(fr, pore_cases.PLANT_CELL, pore_cases.PLANT_GRID, (True, True, True)) == []
        # the planted distance is what the construction says, to rounding
        s = fr.samples[0, scases.PLANT_SAMPLE]
        d = np.sqrt(((packed.pos[f, 1] - s) ** 2).sum())
        assert abs(d - (R[0] + scases.PLANT_THR[k] + sd)) < 1e-14
        # atoms 2 .. 4 meet nobody
        assert fr.exposed[2:].all()


def test_known_answers_of_the_restatement():
    one = scases.one_atom()
    fr = sref.frame(one.pos[0], scases.CUBE, [1.39], 1.2, P.sphere_points(64), (True, True, True))
    assert fr.exposed.all()
    two = scases.two_atoms()
    dirs = P.sphere_points(scases.PAIR_M)
    rho = 1.39 + scases.PAIR_RP
    edge = scases.PAIR_D / (2.0 * rho)
    assert np.abs(dirs[:, 2] - edge).min() > 1e-6
    fr = sref.frame(two.pos[0], scases.CUBE, [1.39, 1.39], scases.PAIR_RP, dirs, (True, True, True))
    assert np.array_equal(fr.exposed[0], dirs[:, 2] <= edge) and np.array_equal(fr.exposed[1], dirs[:, 2] >= -edge)
    want = scases.PAIR_M * (1.0 + edge) / 2.0
    assert abs(fr.exposed[0].sum() - want) <= 1 and abs(fr.exposed[1].sum() - want) <= 1


def test_corner_rule():
    cell = np.diag([4.0, 6.0, 8.0])
    grid = (4, 3, 8)
    # the point (i + 0.5) / n of the grid is corner (0, 0, 0) of a sample a little beyond it
    s = np.array([[1.6, 1.1, 0.6], [0.1, 0.1, 0.1], [3.9, 5.9, 7.9]])
    idx, near = sref.corners(s, cell, grid, (True, True, True))
    assert not near.any()
    lin = lambda i, j, k: (i * 3 + j) * 8 + k
    assert idx[0].tolist() == [lin(1 + a, 0 + b, 0 + c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    assert idx[1].tolist() == [lin((3 + a) % 4, (2 + b) % 3, (7 + c) % 8) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    assert sorted(idx[2].tolist()) == sorted(idx[1].tolist())
    # an open axis drops the corners outside the grid
    idx, _ = sref.corners(s, cell, grid, (True, False, True))
    assert (idx[1].reshape(2, 2, 2)[:, 0, :] == -1).all() and (idx[1].reshape(2, 2, 2)[:, 1, :] >= 0).all()
    assert (idx[2].reshape(2, 2, 2)[:, 1, :] == -1).all()
    # a sample on a grid plane is a near decision
    _, near = sref.corners(np.array([[1.5, 1.1, 0.6]]), cell, grid, (True, True, True))
    assert near.all()
    mask = np.zeros(grid, dtype=bool)
    mask[2, 1, 1] = True
    exposed = np.array([[True, True, False]])
    got = sref.accessible(exposed, s[None], cell, grid, (True, True, True), mask)
    assert got.tolist() == [[True, False, False]]


def test_sphere_points():
    for M in (1, 2, 64, 100, 256, 4096):
        u = P.sphere_points(M)
        assert u.shape == (M, 3) and u.dtype == np.float64 and u.flags.c_contiguous
        assert np.abs((u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2] - 1.0).max() <= 1e-12
        assert np.allclose(u[:, 2], 1.0 - (2.0 * np.arange(M) + 1.0) / M, rtol=0, atol=1e-15)
        if M > 1:
            assert np.allclose(np.diff(u[:, 2]), -2.0 / M, rtol=0, atol=1e-14)
        assert np.abs(u.sum(axis=0)[2]) < 1e-12
    phi = np.arctan2(P.sphere_points(64)[:, 1], P.sphere_points(64)[:, 0])
    step = np.pi * (3.0 - np.sqrt(5.0))
    assert np.allclose(np.exp(1j * phi), np.exp(1j * step * np.arange(64)), atol=1e-12)
    for bad in (0, 4097, -3):
        with pytest.raises(ValueError):
            P.sphere_points(bad)


def test_surface_columns():
    radii = np.array([1.7, 1.39])
    probes = [0.0, 1.2]
    M = 64
    exposed = np.array([[[10, 20], [30, 5]], [[0, 64], [7, 0]]], dtype=np.int64)
    access = np.array([[[4, 20], [0, 5]], [[0, 1], [7, 0]]], dtype=np.int64)
    volume, mass = np.array([1000.0, 1250.0]), 500.0
    cols = P.surface_columns(exposed, access, radii, volume, mass, probes, M)
    assert list(cols) == [n + u + "-" + p for p in ("0", "1.2") for n in ("SA", "ASA", "NASA") for u in ("_A^2", "_m^2/cm^3", "_m^2/g")]
    for k, rp in enumerate(probes):
        lab = P.probe_label(rp)
        want = sum(4.0 * np.pi * (radii[s] + rp) ** 2 * exposed[:, k, s] / M for s in range(2))
        assert cols["SA_A^2-" + lab] == pytest.approx(want, rel=1e-15)
        assert np.array_equal(cols["SA_m^2/cm^3-" + lab], cols["SA_A^2-" + lab] * 1e4 / volume)
        assert np.array_equal(cols["SA_m^2/g-" + lab], cols["SA_A^2-" + lab] * 6022.14076 / mass)
        assert cols["ASA_A^2-" + lab] + cols["NASA_A^2-" + lab] == pytest.approx(cols["SA_A^2-" + lab], rel=1e-15)
        assert np.array_equal(cols["NASA_A^2-" + lab], P.surface_area((exposed - access)[:, k], radii, rp, M))
    # units: one A^2 per A^3 is 1e4 m^2/cm^3; one A^2 per (g/mol) is 1e-20 N_A m^2/g
    assert P.SURFACE_PER_GRAM == pytest.approx(1e-20 * 6.02214076e23, rel=1e-15)
    # a whole sphere: 4 pi rho^2, by the host formula to the last bit
    full = P.surface_area(np.array([[M]]), [1.39], 1.2, M)
    rho = np.float64(1.39) + np.float64(1.2)
    assert full[0] == (4.0 * np.pi) * rho * rho * np.float64(M) / np.float64(M) and full[0] == pytest.approx(4 * np.pi * 2.59 ** 2, rel=1e-15)
    plain = P.surface_columns(exposed, None, radii, volume, mass, probes, M)
    assert list(plain) == [n for n in cols if n.startswith("SA_")] and all(np.array_equal(plain[n], cols[n]) for n in plain)
    with pytest.raises(ValueError):
        P.surface_columns(exposed, exposed + 1, radii, volume, mass, probes, M)


def test_header_declares_the_surface_symbols_and_names_the_method():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        header = fh.read()
    for symbol in ("amof_pore_surface", "amof_pore_surface_bound", "amof_pore_surface_stats"):
        assert re.search(r"\b(int|double) %s\(" % symbol, header), symbol
        assert symbol in _hip.EXPORTS
    assert "Shrake-Rupley" in header and "does not reproduce Zeo++'s numbers" in header
    assert "pore_surface_list" in header and "pore_surface_exact" in header and "which = 6 the surface stage" in header
    # the five places that said the surface area was missing say so no longer
    for name, phrase in (("README.md", "still missing is the surface area"), ("DESIGN.md", "*Not done:* surface area"),
                         ("SURVEY.md", "remain missing"), (os.path.join("amof_amd", "pore.py"), "Not computed: surface areas")):
        with open(os.path.join(ROOT, name)) as fh:
            assert phrase not in fh.read(), name


def test_pore_names_defaults_are_the_old_tuples():
    n = _hip.pore_names
    assert n() == ("hist", "counts", "vmax", "argmax")
    assert n(per_point=True) == ("hist", "counts", "vmax", "argmax", "field")
    assert n(labelled=True, free_sphere=True, labels=True, per_point=True) == ("hist", "counts", "vmax", "argmax", "access", "free_sphere",
                                                                               "field", "labels")
    assert n(True, True, True, True, True, True) == ("hist", "counts", "vmax", "argmax", "access", "free_sphere", "field", "labels",
                                                      "psd_hist", "po_counts", "po_access", "cover")
    assert n(psd=True) == ("hist", "counts", "vmax", "argmax", "psd_hist", "po_counts")
    assert n(surface=True) == n() + ("exposed",)
    assert n(surface=True, accessibility=True, labelled=True) == ("hist", "counts", "vmax", "argmax", "access", "exposed", "exposed_access")
    assert n(surface=True, per_point=True)[-2:] == ("exposed", "samples")
    assert _hip.PoreResult._fields[:12] == ("hist", "counts", "vmax", "argmax", "access", "free_sphere", "field", "labels", "psd_hist",
                                            "po_counts", "po_access", "cover")
    assert _hip.PoreResult._fields[12:] == ("exposed", "exposed_access", "samples")
