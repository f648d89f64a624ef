"""CPU side of tests/test_gpu_cell_forms.py: the cell forms are what they claim, the generators' own floors hold in every
form of the cells the GPU tests use, the C oracle -- their yardstick -- agrees with the numpy restatement of
test_guard_band_cpu.py in rotated, mirrored and negated cells and does not see the sign of a cell row, the selection of
the rdf_tile_tri variant is pinned per form to tri_select.h, and the band arithmetic of every form equals guard_math.h."""

import numpy as np
import pytest

from oracle import clib
from tests import cell_forms as CF
from tests import edge_plant as E
from tests import tri_plant as T
from tests.test_guard_band_cpu import _agree_but_at_edges, _ask as _ask_guard, _fmt, _np_rdf, _pairs_of_frame
from tests.test_guard_band_cpu import driver as guard_driver  # noqa: F401  (the guard_math_driver fixture)
from tests.test_tri_select_cpu import _all_nbins, _ask, _build, _line

ALL_FORMS = CF.ORTHO_FORMS + CF.GENERAL_FORMS
BASES = {"diagonal": CF.DIAG, "sheared": CF.SHEARED}
N = 1200


def _numbers(n=N):
    return T.numbers(n)


@pytest.fixture(scope="module")
def tri_driver(tmp_path_factory):
    return _build(tmp_path_factory.mktemp("cf"), ["-O1"], "tri_select_driver")


# ------------------------------------------------------------------------------------------------ the forms --

def test_rotation_is_proper_and_full():
    Q = CF.Q
    assert np.abs(Q @ Q.T - np.eye(3)).max() < 1e-15 and np.linalg.det(Q) == pytest.approx(1.0, abs=1e-15)
    assert np.abs(Q).min() >= 0.1


def test_forms_are_what_they_claim():
    for base in (CF.DIAG, CF.SHEARED, CF.HIGH_KAPPA, CF.THIN["sheared"], CF.WIDE["diagonal"], CF.nbr_cell("npt")):
        for form in CF.FORMS:
            CF.check(base, form)
    d = {f: CF.view(CF.apply(CF.DIAG, f)) for f in CF.FORMS}
    s = {f: CF.view(CF.apply(CF.SHEARED, f)) for f in CF.FORMS}
    # general forms with nine non-zero entries, right- and left-handed; ortho forms with a negative diagonal
    assert (s["rot"]["nonzero"], s["rot"]["hand"]) == (9, 1) and (s["rotmirror"]["nonzero"], s["rotmirror"]["hand"]) == (9, -1)
    assert (d["rot"]["nonzero"], d["rot"]["all_ortho"]) == (9, False)
    for f in ("mirror", "negrow", "negall"):
        assert d[f]["all_ortho"] and d[f]["neg_diag"] and d[f]["hand"] == -1 and s[f]["hand"] == -1 and not s[f]["all_ortho"]
    # an orthogonal cell that is not "ortho" to the library
    p = CF.apply(CF.DIAG, "perm")
    assert not d["perm"]["all_ortho"] and d["perm"]["nonzero"] == 3 and np.allclose(p @ p.T, np.diag(np.diag(p @ p.T)))
    assert [(b, f) for b, f in ALL_FORMS if CF.view(CF.apply(BASES[b], f))["all_ortho"]] == CF.ORTHO_FORMS
    # per-frame cells are transformed frame by frame
    c = CF.nbr_cell("npt")
    for f in CF.FORMS:
        assert np.array_equal(CF.apply(c, f), np.stack([CF.apply(x, f) for x in c]))


# ------------------------------------------------------------------------- the generators check themselves --

@pytest.mark.parametrize("base,form", ALL_FORMS, ids=["%s-%s" % p for p in ALL_FORMS])
def test_rdf_plantings_check_themselves(base, form):
    """plant_rdf asserts its floors (Planted.check) on every call; here in every (cell, form, cutoff, bin count) of
    the GPU tests, and the oracle's cell-list and brute-force forms agree bit for bit on the result"""
    cases = [(BASES[base], CF.RDF_RMAX[base]), (CF.THIN[base], CF.RMAX_THIN), (CF.WIDE[base], CF.RMAX_WIDE),
             (CF.npt(BASES[base], 3, 0.015, 4), CF.RDF_RMAX_NPT[base])]
    if (base, form) in CF.ORTHO_FORMS:
        cases.append((CF.DIAG, 0.505 * CF.DIAG[0, 0]))
    for k, (c0, rmax) in enumerate(cases):
        c = CF.check(c0, form)
        for nbins in CF.RDF_NBINS:
            pl = E.plant_rdf(c, _numbers(), rmax, nbins, seed=40 + nbins, F=None if c.ndim == 3 else 2, far=True)
            t = pl.band_units()
            assert np.all(np.abs(t) <= 10.0 + 1e-6) and (np.abs(t) <= 1.0).sum() >= 5
            if k == 0:
                kinds, sp = E._species(pl.packed.numbers)
                a, _ = clib.rdf_hist(pl.packed.pos, pl.packed.cell, sp, len(kinds), rmax, nbins, cell_list=True)
                b, _ = clib.rdf_hist(pl.packed.pos, pl.packed.cell, sp, len(kinds), rmax, nbins)
                assert a.sum() > 0 and np.array_equal(a, b), (base, form, nbins)


def _nbr_setup(n=N):
    from tests.test_gpu_guard_band import _nbr_setup as setup
    return setup(n)


@pytest.mark.parametrize("form", CF.FORMS)
@pytest.mark.parametrize("kind", ["diagonal", "sheared", "npt"])
def test_nbr_plantings_check_themselves(kind, form):
    from tests.test_gpu_guard_band import EDGES_RAGGED, EDGES_REGULAR
    c = CF.check(CF.nbr_cell(kind), form)
    numbers, rcm, sets, triples = _nbr_setup()
    for edges, compact in ((EDGES_REGULAR, False), (EDGES_RAGGED, False), (EDGES_REGULAR, True)):
        if compact and (kind == "npt" or form not in ("rot", "mirror")):
            continue
        pl = E.plant_nbr(c, numbers, rcm, seed=60, F=None if kind == "npt" else 2, far=True, compact=compact,
                         triples=triples, angle_edges=edges)
        assert len(pl.angles) >= 50 and np.abs(pl.band_units()).min() == 0.0


@pytest.mark.parametrize("name,form,nbins", T.form_params())
def test_tri_plantings_land_on_their_decisions(name, form, nbins):
    """the floors of test_tri_select_cpu.py on the plantings made in the transformed cells: per category at least 100
    pairs within 1e-3 of the cell of the decision, at least 20 on either side"""
    pl = T.plant_tri(name, nbins, seed=nbins, form=form)
    sts, _ = T.stored_frames(name, nbins, form)
    cats = T.categories(name, sts, T.CASES[name]["rmax"] is None)
    counts = pl.counts()
    cx = counts.pop("cx")
    assert sorted(counts) == cats
    if T.CASES[name]["expect"][0] < 5:
        counts["cx"] = cx
    for c, (within, below, above) in counts.items():
        assert within >= 100 and below >= 20 and above >= 20, (name, form, nbins, c, within, below, above)
    assert pl.packed.pos.shape[1] == 2400
    # the same categories and, to rounding, the same thresholds as the tabulated cell: the form changes the storage only
    base, _ = T.stored_frames(name, nbins)
    for a, b in zip(sts, base):
        fin = np.isfinite(b.rec())
        assert np.array_equal(np.isfinite(a.rec()), fin)
        # (negating a row changes signs of L10 and the folds, never a magnitude)
        assert np.allclose(np.abs(a.rec()[fin]), np.abs(b.rec()[fin]), rtol=1e-9, atol=1e-9), (name, form, a.rec(), b.rec())


# ------------------------------------------------------------------------------- the oracle as the yardstick --

@pytest.mark.parametrize("kind,form,nbins", [("sheared", "rot", 999), ("diagonal", "mirror", 2310), ("sheared", "negall", 7),
                                             ("diagonal", "negall", 999), ("npt", "rot", 31744), ("sheared", "mirror", 2310)])
def test_oracle_rdf_equals_a_numpy_restatement_on_planted_pairs(kind, form, nbins):
    """test_guard_band_cpu.py's comparison with the cell in a form: the independent float64 restatement of DESIGN.md §2
    agrees with the C oracle but where a pair sits within 1e-9 bins of an edge"""
    c0 = np.stack([CF.SHEARED * (1.0 + 0.013 * k) for k in range(3)]) if kind == "npt" else BASES[kind][None]
    c = CF.check(c0, form)
    h = min(abs(np.linalg.det(x)) / np.linalg.norm(np.cross(x[[1, 2, 0]], x[[2, 0, 1]]), axis=1).max() for x in c)
    rmax = 0.49 * h
    numbers = [1] * 400 + [6] * 330 + [30] * 70 + [7]
    pl = E.plant_rdf(c, numbers, rmax, nbins, seed=11 + nbins, F=None if kind == "npt" else 2, far=True)
    kinds, sp = E._species(numbers)
    ref, _ = clib.rdf_hist(pl.packed.pos, pl.packed.cell, sp, len(kinds), rmax, nbins)
    mine, amb = _np_rdf(pl.packed.pos, pl.packed.cell, sp, len(kinds), rmax, nbins)
    assert len(amb) > 0
    _agree_but_at_edges(mine, ref, amb, nbins)
    assert ref.sum() > 0 and abs(int(ref.sum()) - int(mine.sum())) <= len(amb)


def _cn_setup():
    numbers = [30] * 150 + [7] * 350 + [6] * 300 + [1] * 300 + [8]
    kinds, sp = E._species(numbers)
    S = len(kinds)
    zn, n, ch, h = (kinds.index(z) for z in (30, 7, 6, 1))
    rcm = np.zeros((S, S))
    rcm[zn, n] = rcm[n, zn] = 2.5
    rcm[ch, h] = rcm[h, ch] = 1.31
    rcm[n, n] = 2.2
    sets = [(zn, n), (n, zn), (ch, h), (h, ch), (n, n), (h, h)]
    return numbers, sp, S, rcm, sets, [(zn, n), (n, n)]


@pytest.mark.parametrize("kind,form", [("sheared", "rot"), ("diagonal", "mirror"), ("sheared", "negall"), ("diagonal", "negall")])
def test_oracle_cn_equals_a_numpy_restatement_on_planted_pairs(kind, form):
    """the CN loop of test_guard_band_cpu.py with the cell in a form; pairs within 1e-12 of a cutoff may differ"""
    c = CF.check(BASES[kind], form)
    numbers, sp, S, rcm, sets, _ = _cn_setup()
    pl = E.plant_nbr(c, numbers, rcm, seed=17, F=2, far=True)
    sums, pa = clib.cn_counts(pl.packed.pos, pl.packed.cell, sp, S, rcm, sets, per_atom=True)
    pos = pl.packed.pos
    n_atoms = pos.shape[1]
    n_amb = 0
    for f in range(pos.shape[0]):
        d2 = _pairs_of_frame(pos[f], c, np.arange(n_atoms))
        np.fill_diagonal(d2, np.inf)
        r = np.sqrt(d2)
        for k, (A, B) in enumerate(sets):
            rc = rcm[A, B]
            ca, cb = np.nonzero(sp == A)[0], np.nonzero(sp == B)[0]
            sub = r[np.ix_(ca, cb)]
            mine = (sub < rc).sum(axis=1)
            amb = (np.abs(sub / rc - 1.0) < 1e-12).sum(axis=1) if rc > 0 else np.zeros(len(ca), int)
            n_amb += int(amb.sum())
            assert np.all(np.abs(pa[f, k, ca] - mine) <= amb), (form, f, (A, B))
            assert np.all(pa[f, k, np.nonzero(sp != A)[0]] == -1)
            assert abs(int(sums[f, k]) - int(mine.sum())) <= int(amb.sum())
    assert sums.sum() > 0 and n_amb > 0


@pytest.mark.parametrize("kind", ["diagonal", "sheared"])
def test_oracle_does_not_see_the_sign_of_a_cell_row(kind):
    """negating any subset of the cell's rows leaves the lattice, and with it every count, as it is: RDF, CN (per atom)
    and BAD of the same positions are bit-equal"""
    c = BASES[kind]
    numbers, sp, S, rcm, sets, triples = _cn_setup()
    edges = np.arange(int(180 // 0.5) + 2) * 0.5
    rmax, nbins = CF.RDF_RMAX[kind], 2310
    rdf_pl = E.plant_rdf(c, numbers, rmax, nbins, seed=23, F=2, far=True)
    nbr_pl = E.plant_nbr(c, numbers, rcm, seed=24, F=2, far=True, triples=triples, angle_edges=edges)

    def results(signs):
        cs = np.asarray(signs, dtype=np.float64)[:, None] * c
        return (clib.rdf_hist(rdf_pl.packed.pos, cs[None], sp, S, rmax, nbins)[0],
                clib.rdf_hist(rdf_pl.packed.pos, cs[None], sp, S, rmax, nbins, cell_list=True)[0]) + \
            tuple(clib.cn_counts(nbr_pl.packed.pos, cs[None], sp, S, rcm, sets, per_atom=True)) + \
            tuple(clib.bad_hist(nbr_pl.packed.pos, cs[None], sp, S, rcm, triples, edges))
    ref = results((1, 1, 1))
    assert ref[0].sum() > 0 and ref[2].sum() > 0 and ref[5].sum() > 0
    for signs in ((1, -1, 1), (-1, -1, -1), (1, 1, -1), (-1, 1, 1)):
        for a, b in zip(results(signs), ref):
            assert np.array_equal(a, b), (kind, signs)


# ---------------------------------------------------------------------------------------------- the selection --

def _sel(tri_driver, keys):
    got = _ask(tri_driver, [_line(T.case_cells(n, f), T.case_rmax(n, f), nb, T.CASES[n].get("nohalf", False)) for n, f, nb in keys])
    return dict(zip(keys, got))


def test_rigid_motions_and_mirrors_select_the_same_variant(tri_driver):
    keys = [(n, f, nb) for n in T.CASES for f in ("rot", "mirror", "rotmirror") for nb in _all_nbins(n)]
    for (n, f, nb), g in _sel(tri_driver, keys).items():
        assert g["ok"] and g["sel"] == T.CASES[n]["expect"] == T.case_expect(n, f), (n, f, nb, g["ok"], g["sel"])


def test_negated_and_permuted_rows_are_pinned_to_the_header(tri_driver):
    """negating rows: the only change is that codes 10 and 11 change places in the four exact-half cases when the second
    row alone is negated (the sign of c10); -C selects what C does.  Permuted rows: the same code on the renamed rows"""
    keys = [(n, f, nb) for n in T.CASES for f in ("negrow", "negall", "perm") for nb in _all_nbins(n)]
    changed = set()
    for (n, f, nb), g in _sel(tri_driver, keys).items():
        assert g["ok"] and g["sel"] == T.case_expect(n, f), (n, f, nb, g["ok"], g["sel"], T.case_expect(n, f))
        if f != "perm" and g["sel"] != T.CASES[n]["expect"]:
            changed.add((n, f))
            assert g["sel"][1:] == T.CASES[n]["expect"][1:] and {g["sel"][0], T.CASES[n]["expect"][0]} == {10, 11}, (n, f, g["sel"])
    assert changed == {(n, "negrow") for n in ("c10_off", "c10_on", "c11_off", "c11_on")}
    for (n, f, nb) in keys:
        if f == "perm":
            e, p = T.CASES[n]["expect"], T.case_expect(n, f)
            assert p[0] == e[0] and p[4] == e[4] and [(1, 2, 0)[x] for x in p[1:4]] == list(e[1:4])


def test_cutoffs_of_the_gpu_tests_are_accepted_in_every_form(tri_driver):
    """the general cells of test_gpu_cell_forms.py take rdf_tile_tri at the cutoffs and bin counts used there: code 0 with
    culling, as the base cells do (test_tri_select_cpu.py)"""
    lines, keys = [], []
    for base, form in CF.GENERAL_FORMS:
        for nb in CF.RDF_NBINS:
            lines.append(_line(CF.apply(BASES[base], form), CF.RDF_RMAX[base], nb))
            keys.append((base, form, nb))
        lines.append(_line(CF.apply(CF.npt(BASES[base], 3, 0.015, 4), form), CF.RDF_RMAX_NPT[base], 999))
        keys.append((base, form, "npt"))
    lines.append(_line(CF.apply(CF.HIGH_KAPPA, "rot"), CF.RMAX_HIGH_KAPPA, 31744))
    keys.append(("high_kappa", "rot", 31744))
    for k, g in zip(keys, _ask(tri_driver, lines)):
        assert g["ok"] and g["sel"][0] == 0 and g["sel"][4] == 1, (k, g["ok"], g["sel"])
        assert g["guard_f"] < 0.25


# ------------------------------------------------------------------------------------------ guard arithmetic --

def test_band_arithmetic_of_every_form_equals_the_host(guard_driver):  # noqa: F811
    cells = []
    for base in (CF.DIAG, CF.SHEARED, CF.HIGH_KAPPA, CF.THIN["diagonal"], CF.THIN["sheared"], CF.WIDE["diagonal"],
                 CF.WIDE["sheared"], CF.nbr_cell("diagonal"), CF.nbr_cell("sheared")):
        cells += [CF.apply(base, f) for f in CF.FORMS]
    npt = [CF.apply(CF.nbr_cell("npt"), f) for f in CF.FORMS]
    got = _ask_guard(guard_driver, ["R 1 " + _fmt(c) for c in cells] + ["R %d " % len(c) + _fmt(c) for c in npt])
    for c, k in zip(cells + npt, got):
        assert k == pytest.approx(E.kappa_rdf(c), rel=1e-11)
    got = _ask_guard(guard_driver, ["P " + _fmt(c) + " " + _fmt(np.linalg.inv(c)) for c in cells])
    for c, k in zip(cells, got):
        assert k == pytest.approx(E.kappa_cell(c), rel=1e-11)
    # the tile paths work from the metric: a rotation or a mirror does not move their band; the neighbour kernels
    # multiply by the cell itself, and their kappa does move
    for base in (CF.DIAG, CF.SHEARED, CF.HIGH_KAPPA, CF.nbr_cell("npt")):
        for f in ("rot", "mirror", "rotmirror", "negrow", "negall"):
            assert E.kappa_rdf(CF.apply(base, f)) == pytest.approx(E.kappa_rdf(base), rel=1e-12), f
    assert E.kappa_cell(CF.apply(CF.nbr_cell("sheared"), "rot")) > 1.5 * E.kappa_cell(CF.nbr_cell("sheared"))
