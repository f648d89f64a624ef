"""Fragments without a GPU: tests/fragment_ref.py against the hand-known answers of tests/fragment_cases.py, and what
amof_amd.fragment makes of the library's integers -- ``assemble``, kinds, Hill formulas, dummy symbols, argument refusals, the
feather round trip -- on planted integers."""

import os

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip
from amof_amd import fragment as amfrag
from amof_amd.fragment import Fragments, assemble
from tests import fragment_cases as cases
from tests import ring_cases
from tests import ring_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_crystal_is_sixteen_zinc_and_thirty_two_imidazolates():
    e, fr = cases.expected("crystal"), cases.frames("crystal")[0]
    assert e.formulas == ["C3H3N2", "Zn"] and e.census.tolist() == [[32, 16, 0]]
    assert e.summary.tolist() == [[48, 8, 0, 0, 0]]                     # nothing winds, no Zn-N bond inside a fragment
    assert e.hist[0, 1] == 16 and e.hist[0, 8] == 32 and e.hist[0].sum() == 48
    assert len({int(l) for l, s in zip(fr.label, fr.shift) if s.any()}) == 8 and int(fr.shift.any(axis=1).sum()) == 20
    assert e.links[0].tolist() == [[0, 64, 0], [64, 0, 0], [0, 0, 0]]   # 4 link bonds per Zn, 2 per imidazolate
    # made whole, every imidazolate is a ring of bonded atoms: no bond is longer than its cutoff
    c = cases.case("crystal").packed
    whole = c.pos[0] + fr.shift @ c.cell[0]
    assert max(np.linalg.norm(whole[j] - whole[i]) for (i, j) in fr.images) < 1.6


def test_the_full_network_is_one_fragment_that_winds():
    e = cases.expected("network")
    assert e.summary.tolist() == [[1, 272, 1, 0, 0]] and e.formulas == ["C96H96N64Zn16"] and e.hist[0, -1] == 1


def test_rigid_fragments_move_as_imposed():
    c, e = cases.case("rigid"), cases.expected("rigid")
    assert c.packed.n_frames == 12 and (e.summary[:, 3] == 0).all() and (e.summary[:, 2] == 0).all()
    inv = np.linalg.inv(c.packed.cell[0])
    for f in range(12):
        s = (e.com[f] - e.com[0] - c.translation[f]) @ inv
        assert np.abs(s - np.rint(s)).max() < 1e-12         # the frame-0 centre plus the translation, modulo the lattice
    assert (np.abs(e.shift).max(axis=(1, 2)) == 1).all() and len(np.unique(e.shift.any(axis=2).sum(axis=1))) > 3     # atoms cross faces
    loose = cases.expected("rigid_loose")
    intact = loose.summary[:, 3] == 0
    assert intact[:5].all() and not intact[5:].any()        # the looser walk: fragments meet from frame 5 on
    assert np.isnan(loose.com[5:]).all() and not np.isnan(loose.com[:5]).any()


def test_breaking_fragments_regroup_atoms():
    e = cases.expected("breaking")
    assert e.summary[:, 3].tolist() == [0, 0, 1, 2, 2, 4]
    assert e.census[:, 2].tolist()[:2] == [0, 0] and (e.census[2:, 2] > 0).all()
    assert np.isnan(e.com[2:]).all() and not np.isnan(e.com[:2]).any()


def test_ring_cases_and_the_chain():
    assert cases.expected("polygon8").summary.tolist() == [[1, 8, 0, 0, 0]]
    for name in ("graphene", "sc5"):
        assert cases.expected(name).summary[0, :3].tolist() == [1, cases.case(name).packed.n_atoms, 1]
    for name in ("random_rect", "random_tri"):
        e = cases.expected(name)
        assert (e.summary[:, 0] > 5).all() and len(e.formulas) > 3
    tri = cases.expected("random_tri")
    assert np.abs(tri.shift[1]).max() == 2 and tri.summary[:, 2].tolist() == [1, 1, 0]      # (two cells along the search tree of a winding fragment)
    c, e = cases.case("chain"), cases.expected("chain")
    assert e.summary.tolist() == [[1, 300, 0, 0, 0]] and np.abs(e.shift).max() >= 2
    # no pair within 1e-4 A of the cutoff
    ring_ref.adjacency(c.packed.pos[0], c.packed.cell[0], c.packed.numbers, c.cutoff, margin=1e-4)
    order = cases.chain()[1]
    site = np.empty(300, dtype=int)
    site[:] = order
    assert all(sorted(site[j] for j in row) == [s for s in (site[i] - 1, site[i] + 1) if 0 <= s < 300]
               for i, row in enumerate(cases.frames("chain")[0].adj))
    for name in cases.NAMES:
        p = cases.case(name).packed
        assert p.n_frames <= 12 and p.n_atoms < 400


def test_every_case_keeps_clear_of_its_cutoffs():
    for name in cases.NAMES:
        c = cases.case(name)
        p = c.packed
        for f in range(p.n_frames):
            for d in (c.cutoff, c.links):
                if d:
                    ring_ref.adjacency(p.pos[f], cases.cell_of(p, f), p.numbers, d, tuple(p.pbc), margin=1e-6)


def test_hill_formulas_kinds_and_dummy_symbols():
    assert amfrag.hill((3, 3, 2, 0), [6, 1, 7, 30]) == "C3H3N2" and amfrag.hill((0, 0, 0, 1), [6, 1, 7, 30]) == "Zn"
    assert amfrag.hill((4, 1, 1), [1, 7, 8]) == "H4NO" and amfrag.hill((1, 4, 0), [6, 1, 8]) == "CH4"
    e, c = cases.expected("crystal"), cases.case("crystal")
    kinds, species = _hip.species_index(c.packed.numbers)
    table, formulas, kind_of_root = amfrag.kinds_of(e.ref_label, species, kinds)
    assert formulas == e.formulas and np.array_equal(table, e.kinds) and table.dtype == np.int32
    assert np.bincount(kind_of_root).tolist() == [32, 16] and len(kind_of_root) == 48
    assert amfrag.dummy_numbers(table, kinds) == [87, 30]                                   # Im -> Fr, Zn stays Zn
    assert amfrag.dummy_numbers([[0, 2], [1, 0], [1, 1]], [1, 8]) == [87, 1, 88]
    rt, rf, _ = amfrag.kinds_of(cases.expected("random_tri").ref_label, *_hip.species_index(cases.case("random_tri").packed.numbers)[::-1])
    assert rf == cases.expected("random_tri").formulas and np.array_equal(rt, cases.expected("random_tri").kinds)


def test_assemble_on_planted_integers():
    formulas = ["C3H3N2", "Zn"]
    summary = np.array([[48, 8, 0, 0, 0], [50, 8, 1, 3, 2]], dtype=np.int64)
    hist = np.zeros((2, 10), dtype=np.int64)
    hist[0, [1, 8]] = 16, 32
    hist[1, [1, 7, 8, 9]] = 18, 1, 30, 1
    census = np.array([[32, 16, 0], [30, 16, 4]], dtype=np.int64)
    links = np.zeros((2, 3, 3), dtype=np.int64)
    links[0, 0, 1] = links[0, 1, 0] = 64
    links[1, 0, 1] = links[1, 1, 0] = 60
    links[1, 2, 1] = links[1, 1, 2] = 2
    data, sizes, lk, report = assemble(summary, hist, census, links, formulas, [10, 15], 272)
    assert list(data.columns) == ["Step", "fragments", "largest", "winding", "C3H3N2", "Zn", "other"]
    assert data.iloc[1].tolist() == [15, 50, 8, 1, 30, 16, 4]
    assert list(sizes.columns) == ["Step"] + [str(n) for n in range(9)] + [">8"] and sizes[">8"].tolist() == [0, 1] and sizes["8"].tolist() == [32, 30]
    assert list(lk.columns) == ["Step", "C3H3N2-Zn", "Zn-C3H3N2", "Zn-other", "other-Zn"]
    assert lk["Zn-C3H3N2"].tolist() == [4.0, 3.75] and lk["C3H3N2-Zn"].tolist() == [2.0, 2.0]
    assert np.isnan(lk["other-Zn"][0]) and lk["other-Zn"][1] == 0.5 and lk["Zn-other"].tolist() == [0.0, 0.125]
    assert report.index.tolist() == [10, 15] and list(report.columns) == ["number_of_atoms", "number_of_nodes", "in_reduced_trajectory", "atoms_regrouped"]
    assert report["in_reduced_trajectory"].tolist() == [True, False] and report["atoms_regrouped"].tolist() == [0, 3]
    assert report["number_of_nodes"].tolist() == [48, 50] and report["number_of_atoms"].tolist() == [272, 272]
    # a partition like the reference frame's in which something winds is not in the reduced trajectory
    wound = summary.copy()
    wound[0, 2] = 1
    assert assemble(wound, hist, census, None, formulas, [0, 1], 272)[3]["in_reduced_trajectory"].tolist() == [False, False]
    assert assemble(summary, hist, census, None, formulas, [0, 1], 272)[2] is None
    bad = census.copy()
    bad[1, 2] = 5
    with pytest.raises(_hip.AmofError, match="frame 1"):
        assemble(summary, hist, bad, links, formulas, [10, 15], 272)
    with pytest.raises(ValueError):
        assemble(summary, hist, census[:, :2], links, formulas, [10, 15], 272)
    with pytest.raises(ValueError):
        assemble(summary, hist, census, links[:, :2], formulas, [10, 15], 272)


def _planted():
    e, c = cases.expected("breaking"), cases.case("breaking")
    kinds, species = _hip.species_index(c.packed.numbers)
    obj = Fragments(max_size=64)
    obj.names, obj.reduce, obj.species_numbers = {"C3H3N2": "Im"}, True, kinds
    table, formulas, kind_of_root = amfrag.kinds_of(e.ref_label, species, kinds)
    seen = {"label": e.ref_label, "winding": 0, "table": table, "formulas": formulas, "kind_of_root": kind_of_root,
            "cell": c.packed.cell, "pbc": c.packed.pbc}
    raw = (e.summary, e.hist, e.census, e.links, e.label, e.shift, e.com, e.mass)
    obj._assemble(raw, seen, True, True, c.packed.n_atoms, np.arange(0, 60, 10))
    return obj, e, c


def test_the_class_assembles_and_reduces_planted_results():
    obj, e, c = _planted()
    assert obj.report_search["in_reduced_trajectory"].tolist() == [True, True, False, False, False, False]
    assert obj.data["C3H3N2"].tolist() == e.census[:, 0].tolist() and obj.links["Zn-C3H3N2"][0] == 4.0 and obj.links["C3H3N2-Zn"][0] == 2.0
    assert np.array_equal(obj.label, e.label) and np.array_equal(obj.counts["summary"], e.summary)
    red = obj.reduced()
    assert red.n_frames == 2 and red.n_atoms == 48 and red.steps.tolist() == [0, 10] and red.symbols == {"Im": "Fr", "Zn": "Zn"}
    assert sorted(np.unique(red.numbers).tolist()) == [30, 87] and (red.numbers == 30).sum() == 16
    assert np.array_equal(red.pos, e.com[:2]) and np.array_equal(red.masses, e.mass) and np.array_equal(red.cell, c.packed.cell)
    zn = e.ref_label[c.packed.numbers == 30]
    assert np.array_equal(np.array(e.roots)[red.numbers == 30], zn)                 # a zinc atom is its own fragment, at its place
    obj.reduce = False
    with pytest.raises(ValueError, match="reduce=False"):
        obj.reduced()
    obj.reduce, obj.ref_winding = True, 1
    with pytest.raises(ValueError, match="winds"):
        obj.reduced()


def test_feather_round_trip(tmp_path):
    obj, _, _ = _planted()
    name = str(tmp_path / "units")
    obj.write_to_file(name)
    back = Fragments.from_file(name)
    assert back.data.equals(obj.data) and back.sizes.equals(obj.sizes) and back.links.equals(obj.links)
    assert back.report_search.equals(obj.report_search)
    obj.links = None
    other = str(tmp_path / "bare")
    obj.write_to_file(other)
    assert Fragments.from_file(other).links is None
    assert isinstance(Fragments().data, pd.DataFrame) and list(Fragments().data.columns) == ["Step"]


def test_argument_refusals():
    tr = ring_cases.zif4()
    for bad in (0, -1, 7.5, 65536):
        with pytest.raises(ValueError, match="max_size"):
            Fragments.from_trajectory(tr, cases.LIGAND_CUT, max_size=bad)
    with pytest.raises(ValueError, match="no pair"):
        Fragments.from_trajectory(tr, {})
    for bad in (1, -1, 0.5):
        with pytest.raises(ValueError, match="reference_frame"):
            Fragments.from_trajectory(tr, cases.LIGAND_CUT, reference_frame=bad)
    with pytest.raises(ValueError, match="links names a pair"):
        Fragments.from_trajectory(tr, cases.LIGAND_CUT, links={'N-C': 2.0})


def test_entry_point_in_the_header_and_in_hip():
    with open(os.path.join(ROOT, "include", "amof_hip.h")) as fh:
        header = fh.read()
    assert "int amof_fragment_stats(amof_ctx *ctx, const amof_traj *traj, const double *cutoff" in header
    assert "amof_fragment_stats" in _hip.EXPORTS and "amof_fragment_round_stats" in _hip.EXPORTS
    assert hasattr(_hip.Context, "fragment_stats") and hasattr(_hip.MultiContext, "fragment_stats")
