"""Dihedral without a GPU: the ABI surface, the restatement (tests/dihedral_ref.py) on the known answers, the host assembly, the
default patterns, the files, the arguments refused before any device work, and the size cap on every input of the GPU tests."""

import os
import re

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import atom as amatom
from amof_amd import dihedral as amdihedral
from amof_amd.dihedral import Dihedral
from tests import dihedral_cases as cases
from tests import dihedral_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_surface():
    import amof_amd
    header = open(os.path.join(ROOT, "include", "amof_hip.h")).read()
    assert re.search(r"#define AMOF_ABI_VERSION 4\b", header) and _hip.ABI_VERSION == 4
    for symbol in ("amof_dihedral_hist", "amof_dihedral_hist_dev"):
        assert re.search(r"\bint %s\(amof_ctx \*ctx, const amof_traj \*traj," % symbol, header) and symbol in _hip.EXPORTS
    for text in ("a != d BY ATOM", "s1 < 2^-40 or s2 < 2^-40", "dihedral_frame", "dihedral_exact", "AMOF_DIHEDRAL_ROWS_MB",
                 "frame_sums int64 [F][n_chains][3]", "llrint(c * 2^40)"):
        assert text in header, text
    assert hasattr(_hip.Context, "dihedral_hist") and hasattr(_hip.MultiContext, "dihedral_hist")
    assert amof_amd.Dihedral is Dihedral
    makefile = open(os.path.join(ROOT, "amof_amd", "csrc", "Makefile")).read()
    assert "dihedral_math.h" in makefile and "angle_math.h" in makefile


def test_simple_cubic_known_answer():
    frames = cases.reference("cubic")
    assert len(frames) == 2
    for fr in frames:
        assert fr.chains == 4800 and fr.triangles == 0
        want = np.zeros(26, dtype=np.int64)
        want[[0, 12, 25]] = 768, 1536, 768
        assert np.array_equal(fr.hist[0], want) and fr.n[0] == 3072 and fr.undefined[0] == 1728
        assert abs(fr.cos[0]) < 1e-9


def test_rock_salt_counts_every_chain_once_in_both_directions():
    for fr in cases.reference("rocksalt"):
        assert fr.n.tolist() == [3072, 3072, 0] and fr.undefined.tolist() == [1728, 1728, 0]
        assert np.array_equal(fr.hist[0], fr.hist[1]) and fr.hist[0, [0, 12, 25]].tolist() == [768, 1536, 768]
    c = cases.case("rocksalt")
    hist, n, undefined, sums, _ = ref.totals(cases.reference("rocksalt"))
    edges, phi = amdihedral.bins(c.dphi)
    data, _ = amdihedral.assemble(hist, n, undefined, np.concatenate([sums, np.zeros_like(sums[:, :, :1])], axis=2), c.chains, edges, phi, [0, 1])
    assert list(data.columns) == ["phi", "Zn-N-Zn-N", "N-Zn-N-Zn"]            # the pattern without a dihedral is omitted


@pytest.mark.parametrize("name", cases.PLANTED_NAMES)
def test_planted_chain_lands_in_its_bin(name):
    fr, = cases.reference(name)
    phi = float(name.split("_")[1])
    want = np.zeros(31, dtype=np.int64)
    want[cases.PLANTED_BIN[phi]] = 1
    assert fr.chains == 1 and fr.n.tolist() == [1, 1, 1, 1, 0] and not fr.undefined.any()
    for t in range(4):
        assert np.array_equal(fr.hist[t], want)
    assert abs(fr.cos[0] - np.cos(np.radians(phi))) < 1e-12
    p = cases.case(name).packed
    frac = p.pos_host()[0] @ np.linalg.inv(p.cell[0])
    assert np.rint(frac[2] - frac[1]).any()                 # the central bond crosses a periodic face


def test_zif4_fixture():
    crystal, mild, strong = cases.reference("zif4")
    names, _ = cases.patterns(cases.case("zif4"))
    per_type = dict(zip(names, crystal.n.tolist()))
    assert int(crystal.n.sum()) == 1024 and not crystal.undefined.any() and crystal.triangles == 0
    assert per_type["C-N-Zn-N"] == 384 and per_type["C-N-C-N"] == 64 and sum(1 for v in per_type.values() if v) == 10
    for fr in (mild, strong):
        assert not fr.undefined.any() and fr.triangles == 0
    # the rattles of dihedral_cases.zif4_frames (one default_rng(7), sigma = 0.05 drawn first, then 0.15): a change of the
    # seed or of its use shows here
    assert int(mild.n.sum()) == 1004 and int(strong.n.sum()) == 619
    explicit = cases.reference("zif4_explicit")
    assert [int(fr.n[0]) for fr in explicit] == [int(fr.n[names.index("C-N-Zn-N")]) for fr in (crystal, mild, strong)]
    assert np.array_equal(explicit[0].hist[1], crystal.hist[names.index("C-N-C-N")])
    assert explicit[0].n.tolist() == [384, 64, per_type["H-C-N-Zn"]] and per_type["H-C-N-Zn"] > 0
    fine = cases.reference("zif4_fine")
    assert fine[0].hist.size > 36864 and int(fine[0].n[12]) == 1024        # X-X-X-X: every chain
    sheared = cases.reference("zif4_sheared")
    assert np.array_equal(sheared[0].n, crystal.n)          # a shear of a few percent breaks no bond of the crystal ...
    assert not np.array_equal(sheared[0].hist, crystal.hist)                # ... and moves its angles
    assert np.count_nonzero(cases.case("zif4_sheared").packed.cell[0]) == 6
    assert cases.reference("triangle")[0].triangles > 0


def test_default_chains_and_the_refusal_of_too_many():
    cut = amatom.format_cutoff(cases.ZIF_CUT, sort_pair=True)
    chains = amdihedral.default_chains(cut, [1, 6, 7, 30])
    names = [amdihedral.chain_name(c) for c in chains]
    assert len(set(chains)) == len(chains) <= 32 and all(c <= c[::-1] for c in chains) and chains == sorted(chains)
    assert "Zn-N-C-N" not in names and "N-C-N-Zn" in names and "C-N-Zn-N" in names and "C-N-C-N" in names and "H-C-N-Zn" in names
    assert all((min(c[k], c[k + 1]), max(c[k], c[k + 1])) in cut for c in chains for k in range(3))
    everything = {"%s-%s" % (a, b): 2.0 for a in ("H", "C", "N", "Zn") for b in ("H", "C", "N", "Zn")}
    with pytest.raises(ValueError, match="chains="):
        amdihedral.default_chains(amatom.format_cutoff(everything, sort_pair=True), [1, 6, 7, 30])
    assert amdihedral.parse_chain("C-N-Zn-X") == (6, 7, 30, -1) and amdihedral.chain_name((6, 7, 30, -1)) == "C-N-Zn-X"


def test_assemble_densities_omitted_columns_and_nan():
    edges, phi = amdihedral.bins(60.0)
    assert edges.tolist() == [0.0, 60.0, 120.0, 180.0, 240.0] and phi.tolist() == [30.0, 90.0, 150.0, 210.0]
    hist = np.array([[1, 2, 1, 0], [0, 0, 0, 0]], dtype=np.uint64)
    sums = np.array([[[4, 1, 2 << 40], [0, 0, 0]], [[0, 2, 0], [0, 0, 0]]], dtype=np.int64)
    data, frames = amdihedral.assemble(hist, [4, 0], [3, 0], sums, ["C-N-Zn-N", "X-X-X-X"], edges, phi, [10, 20])
    assert list(data.columns) == ["phi", "C-N-Zn-N"]
    want, _ = np.histogram([10.0, 70.0, 80.0, 130.0], bins=edges, density=True)
    assert np.array_equal(data["C-N-Zn-N"].to_numpy(), want)
    assert frames["Step"].tolist() == [10, 20] and frames["C-N-Zn-N-n"].tolist() == [4, 0]
    assert frames["C-N-Zn-N-undefined"].tolist() == [1, 2] and frames["C-N-Zn-N-cos"][0] == 0.5
    assert np.isnan(frames["C-N-Zn-N-cos"][1]) and np.isnan(frames["X-X-X-X-cos"]).all()


def test_feather_round_trip(tmp_path):
    edges, phi = amdihedral.bins(60.0)
    dh = Dihedral()
    dh._assemble((np.array([[1, 2, 1, 0]], dtype=np.uint64), np.array([4], dtype=np.uint64), np.array([0], dtype=np.uint64),
                  np.array([[[4, 0, 1 << 40]]], dtype=np.int64)), ["C-N-Zn-N"], edges, phi, [0])
    dh.write_to_file(tmp_path / "out")
    assert (tmp_path / "out.dihedral").exists() and (tmp_path / "out.dihedral_frames").exists()
    back = Dihedral.from_file(tmp_path / "out")
    assert back.data.equals(dh.data) and back.frames.equals(dh.frames) and back.chains == ["C-N-Zn-N"]


@pytest.mark.parametrize("kwargs, text", [
    (dict(nb_set_and_cutoff={'C-C': 1.7}, dphi=0.0), "dphi"),
    (dict(nb_set_and_cutoff={'C-C': 1.7}, dphi=float("nan")), "dphi"),
    (dict(nb_set_and_cutoff={'C-C': 1.7}, dphi=181.0), "dphi"),
    (dict(nb_set_and_cutoff={}), "no pair"),
    (dict(nb_set_and_cutoff={'C-Qq': 1.7}), "unknown chemical symbol"),
    (dict(nb_set_and_cutoff={'C-C': 1.7}, chains=['C-C-C']), "four species"),
    (dict(nb_set_and_cutoff={'C-C': 1.7}, chains=['C-C-C-Qq']), "unknown chemical symbol"),
    (dict(nb_set_and_cutoff={'C-C': 1.7}, chains=[]), "1 to 32"),
    (dict(nb_set_and_cutoff={'C-C': 1.7}, chains=['C-C-C-C'] * 33), "1 to 32"),
])
def test_arguments_are_refused_before_device_work(kwargs, text, monkeypatch):
    from amof_amd import _setup

    def no_device(*a, **k):
        raise AssertionError("device work before the arguments were checked")
    monkeypatch.setattr(_setup, "pack", no_device)
    monkeypatch.setattr(_setup, "setup", no_device)
    with pytest.raises(ValueError, match=text):
        Dihedral.from_trajectory(cases.triangle(), **kwargs)


def test_every_gpu_input_is_small():
    for name in cases.NAMES:
        p = cases.case(name).packed
        assert p.n_frames <= 8 and p.n_atoms <= 400, name
    assert cases.crowded(17).n_atoms <= 400
