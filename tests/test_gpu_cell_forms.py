"""The planted-pair tests of test_gpu_guard_band.py and test_gpu_tri_codes.py in the cell forms of tests/cell_forms.py:
rotated (all nine entries non-zero), left-handed, negated, and an orthogonal cell stored with permuted rows.

Every other GPU test stores its cell with a positive diagonal, either diagonal or lower-triangular and right-handed: there
three of the nine scale entries of the general-cell kernels only ever multiply 0.0, the f32 bound (5 kappa + 3.06) u is
exercised on one- and two-term rows, and no sign of a cell entry is ever negative.  Here the same plantings are made
directly in the transformed cell (the generators take any cell), every run forces its path with the switches of
test_gpu_paths.py and asserts that it ran, and every integer is compared bit for bit with the C oracle.  Each test
asserts through cell_forms.check that its cell is what the form claims (ortho flag, handedness, non-zero entries).
tests/test_cell_forms_cpu.py checks the plantings, the oracle and the pinned selections on the CPU."""

import functools
import re

import numpy as np
import pytest

from oracle import clib
from tests import cell_forms as CF
from tests import edge_plant as E
from tests import tri_plant as T
from tests.test_gpu_guard_band import (EDGES_RAGGED, EDGES_REGULAR, NBR_PATHS, TILE, _device, _env, _nbr_setup, _numbers)

pytestmark = pytest.mark.gpu

BASES = {"diagonal": CF.DIAG, "sheared": CF.SHEARED}
ZF_RUNS = [(TILE, "rdf_tile_zf"), (dict(TILE, AMOF_RDF_NOZF="1"), "rdf_tile")]
TRI_RUNS = [(TILE, "rdf_tile_tri"), (dict(TILE, AMOF_RDF_NOTRI="1"), "rdf_tile")]
EXACT_RUN = [({"AMOF_RDF_KERNEL": "v1"}, "rdf_exact")]
RANGE_RUN = [({"AMOF_RDF_FORCE_RANGE": "1", "AMOF_RDF_NOCELL": "1"}, "rdf_range")]
CELL_RUNS = [({"AMOF_RDF_FORCE_CELL": "1"}, "rdf_cell"), ({"AMOF_RDF_FORCE_CELL": "1", "AMOF_RDF_CELL_GATHER": "1"}, "rdf_cell")]
THREE = dict(kinds=(1, 6, 8), weights=(0.6, 0.4, 0.0))     # rdf_cell holds S (S + 1) / 2 histograms in LDS


def _ids(pairs):
    return ["%s-%s" % p for p in pairs]


def _rdf_case(hip_ctx, what, pl, rmax, nbins, runs, device=False):
    """runs: [(env, path)]: each forced path must run and equal the oracle bit for bit; `what` names the cell form"""
    packed = pl.packed
    kinds, sp = E._species(packed.numbers)
    ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), rmax, nbins, cell_list=True)
    assert ref.sum() > 0
    inputs = [("host", packed), ("device", _device(packed))] if device else [("host", packed)]
    for env, path in runs:
        for label, inp in inputs:
            with _env(**env):
                got, _, _ = hip_ctx.rdf_accumulate(inp, rmax, nbins)
                ran = hip_ctx.last_path()
            assert ran == path, (what, env, ran, path)
            bad = np.argwhere(got != ref)
            assert len(bad) == 0, (what, path, sorted(env), label, nbins,
                                   int(np.abs(got.astype(np.int64) - ref.astype(np.int64)).sum()), bad[:8].tolist())


# ------------------------------------------------------------------------------------------------------ RDF --

@pytest.mark.parametrize("nbins", CF.RDF_NBINS)
@pytest.mark.parametrize("form", [f for _, f in CF.ORTHO_FORMS])
def test_rdf_ortho_cells_with_negative_entries(hip_ctx, form, nbins):
    """a diagonal cell with negative entries keeps the ortho flag: rdf_tile_zf, rdf_tile, rdf_tile_img (forced, and chosen
    by rmax just over half the shortest cell length), rdf_exact"""
    c = CF.check(CF.DIAG, form)
    assert CF.view(c)["all_ortho"] and CF.view(c)["neg_diag"]
    what = "diagonal/" + form
    pl = E.plant_rdf(c, _numbers(2400), 8.0, nbins, seed=1100 + nbins, F=3, far=True)
    _rdf_case(hip_ctx, what, pl, 8.0, nbins, ZF_RUNS, device=nbins == 2310)
    _rdf_case(hip_ctx, what, pl, 8.0, nbins, [(dict(TILE, AMOF_RDF_FORCE_IMG="1"), "rdf_tile_img")] + EXACT_RUN)
    rmax = 0.505 * CF.DIAG[0, 0]
    pl = E.plant_rdf(c, _numbers(2400), rmax, nbins, seed=1110 + nbins, F=2, far=True)
    _rdf_case(hip_ctx, what, pl, rmax, nbins, [(TILE, "rdf_tile_img")])


@pytest.mark.parametrize("base,form", CF.ORTHO_FORMS + CF.GENERAL_FORMS, ids=_ids(CF.ORTHO_FORMS + CF.GENERAL_FORMS))
def test_rdf_range_kernel(hip_ctx, base, form):
    """rdf_range (2-level slab x y-bin list) on the thin long cell"""
    c = CF.check(CF.THIN[base], form)
    for nbins in CF.RDF_NBINS:
        pl = E.plant_rdf(c, _numbers(3000), CF.RMAX_THIN, nbins, seed=1200 + nbins, F=2, far=True)
        _rdf_case(hip_ctx, "thin %s/%s" % (base, form), pl, CF.RMAX_THIN, nbins, RANGE_RUN)


@pytest.mark.parametrize("base,form", CF.ORTHO_FORMS + CF.GENERAL_FORMS, ids=_ids(CF.ORTHO_FORMS + CF.GENERAL_FORMS))
def test_rdf_cell_list_kernels(hip_ctx, base, form):
    """rdf_cell, one wave per cell and the per-lane gather form (five species at 999 bins, three at 2310: the kernel's LDS)"""
    c = CF.check(CF.WIDE[base], form)
    for nbins, numbers in ((999, _numbers(4000)), (2310, _numbers(4000, **THREE))):
        pl = E.plant_rdf(c, numbers, CF.RMAX_WIDE, nbins, seed=1300 + nbins, F=2, far=True)
        _rdf_case(hip_ctx, "wide %s/%s" % (base, form), pl, CF.RMAX_WIDE, nbins, CELL_RUNS)


@pytest.mark.parametrize("base,form", CF.ORTHO_FORMS + CF.GENERAL_FORMS, ids=_ids(CF.ORTHO_FORMS + CF.GENERAL_FORMS))
def test_rdf_npt_cells(hip_ctx, base, form):
    """per-frame cells, every frame in the same form; device input"""
    c = CF.check(CF.npt(BASES[base], 3, 0.015, 4), form)
    ortho = (base, form) in CF.ORTHO_FORMS
    assert CF.view(c)["all_ortho"] == ortho
    rmax, nbins = CF.RDF_RMAX_NPT[base], 2310 if ortho else 999
    pl = E.plant_rdf(c, _numbers(2400), rmax, nbins, seed=1400, far=True)
    _rdf_case(hip_ctx, "npt %s/%s" % (base, form), pl, rmax, nbins, ZF_RUNS if ortho else TRI_RUNS, device=True)


@pytest.mark.parametrize("nbins", CF.RDF_NBINS)
@pytest.mark.parametrize("base,form", CF.GENERAL_FORMS, ids=_ids(CF.GENERAL_FORMS))
def test_rdf_general_cells(hip_ctx, base, form, nbins):
    """rdf_tile_tri, the plain general kernel (AMOF_RDF_NOTRI) and rdf_exact; the cutoffs are those the selection accepts
    for every form (tests/test_cell_forms_cpu.py)"""
    c = CF.check(BASES[base], form)
    assert not CF.view(c)["all_ortho"]
    rmax = CF.RDF_RMAX[base]
    pl = E.plant_rdf(c, _numbers(2400), rmax, nbins, seed=1500 + nbins, F=3, far=True)
    _rdf_case(hip_ctx, "%s/%s" % (base, form), pl, rmax, nbins, TRI_RUNS,
              device=nbins == 999 and form in ("rot", "negall"))
    _rdf_case(hip_ctx, "%s/%s" % (base, form), pl, rmax, nbins, EXACT_RUN)


def test_rdf_high_kappa_cell_rotated(hip_ctx):
    """the strongly sheared cell at the LDS limit of the tile kernels: a rotation leaves its band where it is, near the
    guard_f < 0.25 limit, and fills all nine entries"""
    c = CF.check(CF.HIGH_KAPPA, "rot")
    assert CF.view(c)["nonzero"] == 9
    rmax, nbins = CF.RMAX_HIGH_KAPPA, 31744
    g = E.rdf_band(c, rmax, nbins)
    assert g > 0.05 and g == pytest.approx(E.rdf_band(CF.HIGH_KAPPA, rmax, nbins), rel=1e-9), g
    pl = E.plant_rdf(c, _numbers(2400, weights=(0.6, 0.4, 0.0, 0.0, 0.0)), rmax, nbins, seed=1600, F=2, far=True)
    _rdf_case(hip_ctx, "high_kappa/rot", pl, rmax, nbins, TRI_RUNS)


# --------------------------------------------------------------------------------- the rdf_tile_tri variants --

TRI_ENV = dict(TILE, AMOF_RDF_DEBUG="1")
LINE = re.compile(r"rdf_tile_tri: code (\d+) \(near mode (\d), x wrap (\d)\) axes \((\d), (\d) \| (\d)\)")
TRI_PARAMS = T.form_params()


def test_tri_parametrisation_covers_every_reachable_variant():
    have = {(T.case_expect(n, f)[0], T.case_expect(n, f)[4]) for n, f, _ in TRI_PARAMS if f == "rot"}
    assert have == {(code, cull) for code in (0, 1, 2, 4, 5, 6, 7, 9, 10, 11) for cull in (0, 1)} | {(3, 0), (8, 0)}
    # negating the second row makes codes 10 and 11 change places; the float-product form stays code 9
    assert [T.case_expect(n, "negrow")[0] for n in T.HALF_CASES] == [11, 11, 10, 10, 9]


@pytest.mark.parametrize("name,form,nbins", TRI_PARAMS)
def test_rdf_tri_variant_in_a_cell_form(hip_ctx, capfd, name, form, nbins):
    """the planting of test_gpu_tri_codes.py made in the transformed cell; the code read back from the debug line equals
    the CPU pin (tri_plant.case_expect, checked against tri_select.h by tests/test_cell_forms_cpu.py)"""
    case = T.CASES[name]
    code, ax0, ax1, axis, cull = T.case_expect(name, form)
    v = CF.view(T.case_cells(name, form))
    assert v["hand"] == (1 if form == "rot" else -1) and not v["all_ortho"]
    assert v["nonzero"] == 9 or form == "negrow"
    rmax = T.case_rmax(name, form)
    packed = T.plant_tri(name, nbins, seed=nbins, form=form).packed
    kinds, sp = E._species(packed.numbers)
    ref, _ = clib.rdf_hist(packed.pos, packed.cell, sp, len(kinds), rmax, nbins, cell_list=True)
    assert ref.sum() > 0
    env = dict(TRI_ENV, AMOF_RDF_NOHALF="1") if case.get("nohalf") else TRI_ENV
    for extra in ({}, {"AMOF_RDF_NOCULL": "1"}) if cull else ({},):
        with _env(**dict(env, **extra)):
            capfd.readouterr()
            got, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins)
            ran = hip_ctx.last_path()
            err = capfd.readouterr().err
        assert ran == "rdf_tile_tri", (name, form, nbins, extra, ran)
        m = LINE.search(err)
        assert m, err
        assert int(m.group(1)) == code, (name, form, nbins, extra, m.group(0))
        assert (int(m.group(4)), int(m.group(5)), int(m.group(6))) == (ax0, ax1, axis), (name, form, m.group(0))
        bad = np.argwhere(got != ref)
        assert len(bad) == 0, (name, form, nbins, "NOCULL" if extra else "as selected", code,
                               int(np.abs(got.astype(np.int64) - ref.astype(np.int64)).sum()), bad[:8].tolist())


# ----------------------------------------------------------------------------------------------- CN and BAD --

@functools.lru_cache(maxsize=None)
def _base_paths(kind):
    """the planting of test_gpu_guard_band.py::test_cn_bad_paths in the base cell: what path each switch gives there"""
    numbers, rcm, sets, triples = _nbr_setup(2400)
    pl = E.plant_nbr(CF.nbr_cell(kind), numbers, rcm, seed=800, F=None if kind == "npt" else 2, far=True, triples=triples,
                     angle_edges=EDGES_REGULAR)
    return pl.packed, {}


def _base_path(hip_ctx, kind, env):
    packed, seen = _base_paths(kind)
    key = tuple(sorted(env.items()))
    if key not in seen:
        _, rcm, sets, triples = _nbr_setup(2400)
        with _env(**env):
            hip_ctx.cn_count(packed, rcm, sets)
            cn = hip_ctx.last_path()
            hip_ctx.bad_hist(packed, rcm, triples, EDGES_REGULAR)
            seen[key] = (cn, hip_ctx.last_path())
    return seen[key]


def _nbr_case(hip_ctx, what, kind, pl, rcm, sets, triples, edges, runs, device=False, by_cn=False):
    packed = pl.packed
    kinds, sp = E._species(packed.numbers)
    S = len(kinds)
    s_ref, pa_ref = clib.cn_counts(packed.pos, packed.cell, sp, S, rcm, sets, per_atom=True)
    h_ref, a_ref = clib.bad_hist(packed.pos, packed.cell, sp, S, rcm, triples, edges)
    assert s_ref.sum() > 0 and a_ref.sum() > 0
    if by_cn:
        hc_ref, ac_ref = clib.bad_hist_by_cn(packed.pos, packed.cell, sp, S, rcm, triples, edges, 8)
    inputs = [("host", packed), ("device", _device(packed))] if device else [("host", packed)]
    for env, path in runs:
        # the path is the one the same switches give the base cell
        assert _base_path(hip_ctx, kind, env) == ("cn_" + path, "bad_" + path), (what, env, _base_path(hip_ctx, kind, env))
        for label, inp in inputs:
            with _env(**env):
                s, pa = hip_ctx.cn_count(inp, rcm, sets, per_atom=True)
                ran = hip_ctx.last_path()
                assert ran == "cn_" + path, (what, env, ran)
                assert np.array_equal(s, s_ref) and np.array_equal(pa, pa_ref), \
                    (what, ran, label, int(np.abs(s - s_ref).sum()), np.argwhere(s != s_ref)[:4].tolist(),
                     np.argwhere(pa != pa_ref)[:8].tolist())
                hb, ab = hip_ctx.bad_hist(inp, rcm, triples, edges)
                ran = hip_ctx.last_path()
                assert ran == "bad_" + path, (what, env, ran)
                assert np.array_equal(ab, a_ref) and np.array_equal(hb, h_ref), \
                    (what, ran, label, int(np.abs(hb.astype(np.int64) - h_ref.astype(np.int64)).sum()),
                     np.argwhere(hb != h_ref)[:8].tolist())
                if by_cn:
                    hc, ac = hip_ctx.bad_hist_by_cn(inp, rcm, triples, edges, cn_max=8)
                    assert np.array_equal(ac, ac_ref) and np.array_equal(hc, hc_ref), \
                        (what, env, hip_ctx.last_path(), np.argwhere(hc != hc_ref)[:8].tolist())


@pytest.mark.parametrize("form", CF.FORMS)
@pytest.mark.parametrize("kind", ["diagonal", "sheared", "npt"])
def test_cn_bad_paths(hip_ctx, kind, form):
    """cn_ / bad_ fast, cell, frame, frame_slabs, exact in every form of the three cells of
    test_gpu_guard_band.py::test_cn_bad_paths: pairs at rc (1 + delta), triples at angle edges with legs at the cutoff,
    per-atom counts; on `rot` also ragged angle edges, bad_hist_by_cn and device input"""
    base = CF.nbr_cell(kind)
    c = CF.check(base, form)
    v = CF.view(c)
    assert v["all_ortho"] == (kind == "diagonal" and form in ("mirror", "negrow", "negall"))
    assert v["nonzero"] == 9 or form not in ("rot", "rotmirror")
    numbers, rcm, sets, triples = _nbr_setup(2400)
    cases = [(0, EDGES_REGULAR)] + ([(1, EDGES_RAGGED)] if form == "rot" else [])
    for k, edges in cases:
        pl = E.plant_nbr(c, numbers, rcm, seed=1800 + k, F=None if kind == "npt" else 3, far=True, triples=triples,
                         angle_edges=edges)
        _nbr_case(hip_ctx, "%s/%s" % (kind, form), kind, pl, rcm, sets, triples, edges, NBR_PATHS,
                  device=form == "rot" and k == 0, by_cn=k == 1 and kind != "npt")


@pytest.mark.parametrize("form", ["rot", "mirror"])
@pytest.mark.parametrize("kind", ["diagonal", "sheared"])
def test_frame_tier_compact_records(hip_ctx, kind, form):
    """the frame tier's compact 16-bit records (AMOF_NBR_COMPACT=1): the coarsest band (guard_abs16)"""
    c = CF.check(CF.nbr_cell(kind), form)
    numbers, rcm, sets, triples = _nbr_setup(2400)
    pl = E.plant_nbr(c, numbers, rcm, seed=1900, F=3, far=True, compact=True, triples=triples, angle_edges=EDGES_REGULAR)
    _nbr_case(hip_ctx, "%s/%s compact" % (kind, form), kind, pl, rcm, sets, triples, EDGES_REGULAR,
              [({"AMOF_NBR_COMPACT": "1"}, "frame")])


# --------------------------------------------------------------------- the analyses that reuse those decisions --
# One small case per analysis and form, built by the analysis' own case builder with the cell in the form, held against the
# reference module, the assertion and the tolerance of the analysis' own GPU test (imported from it).

ANALYSIS_FORMS = ("rot", "mirror", "negall")
NEG_DIAG = ("mirror", "negall")


def _small_cell(form, diag, sheared):
    """negative-diagonal forms of the diagonal cell (the fast paths), a rotation of the sheared one (the general kernels)"""
    c = CF.check(sheared if form == "rot" else diag, form)
    v = CF.view(c)
    assert (v["all_ortho"] and v["neg_diag"]) if form in NEG_DIAG else v["nonzero"] == 9
    return c


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_distinct_vanhove(hip_ctx, form):
    """rdf_distinct_tile on the negative-diagonal forms (a walk, and pairs planted across the guard band between two
    frames as test_gpu_vanhove_distinct.py plants them), rdf_distinct_exact / _global on the rotated cell"""
    from amof_amd.frames import PackedTrajectory
    from tests import test_gpu_vanhove_distinct as V
    c = _small_cell(form, V.DIAG, V.SHEARED)
    packed = V._walk(c, V._numbers4(263), 8, seed=21)
    windows = np.array([0, 1, 3, 4], dtype=np.int32)
    if form == "rot":
        V._case(hip_ctx, packed, windows, 8.0, 333, [({}, "rdf_distinct_exact"), (V.GLOBAL, "rdf_distinct_exact_global")], device=True)
        return
    V._case(hip_ctx, packed, windows, 8.0, 333, [({}, "rdf_distinct_tile"), (V.EXACT, "rdf_distinct_exact"),
                                                 (V.GLOBAL, "rdf_distinct_exact_global")], device=True)
    rmax, nbins = 8.0, 999
    numbers = np.repeat([1, 6, 7, 30], [700, 500, 420, 180])
    pl = E.plant_rdf(c, numbers, rmax, nbins, seed=1299, F=1, far=True)
    P = pl.packed.pos[0]
    rng = np.random.default_rng(nbins)
    perm = np.arange(len(numbers))
    for z in (1, 6, 7, 30):
        idx = np.nonzero(numbers == z)[0]
        perm[idx] = rng.permutation(idx)
    shift = np.where(rng.uniform(0, 1, (len(numbers), 1)) < 0.4, rng.integers(-3, 4, (len(numbers), 3)), 0)
    planted = PackedTrajectory(np.stack([P, P, P[perm] + shift @ c, P]), c, numbers)
    want = V._case(hip_ctx, planted, np.array([0, 1, 2], dtype=np.int32), rmax, nbins,
                   [({}, "rdf_distinct_tile"), (V.EXACT, "rdf_distinct_exact")])
    assert want[:, :, 1].sum() > 0 and want[:, :, 2].sum() > 0


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_bond_lifetime(hip_ctx, form):
    """bond_series on the negative-diagonal forms, bond_series_exact on the rotated cell; a walk and the planted
    guard-band case of test_gpu_bond.py"""
    from tests import test_gpu_bond as B
    c = _small_cell(form, B.DIAG, B.SHEARED)
    fast = form in NEG_DIAG
    packed = B._walk(c, B._numbers4(131), 67, 13)
    B._case(hip_ctx, packed, [(30, 7, 3.3), (6, 1, 3.0)], [0, 1, 4, 30, 65],
            B.FAST_RUNS if fast else [({}, "bond_series_exact"), (B.FRAMES, "bond_series_exact")], device=True)
    planted, pl = B._planted(2, 42, CF.check(B.DIAG, form))
    runs = [({}, "bond_series"), (B.EXACT, "bond_series_exact"), (B.FRAMES, "bond_series")] if fast else [({}, "bond_series_exact")]
    want = B._case(hip_ctx, planted, [(30, 7, 3.4), (7, 30, 3.4), (7, 7, 3.1), (30, 30, 2.9)], [0, 1, 2], runs)
    t = pl.band_units()
    assert int((t < -1e-3).sum()) >= 5 and int((t > 1e-3).sum()) >= 5 and int((np.abs(t) <= 1.0).sum()) >= 5
    assert int(want[:, 2, 2].sum()) >= 2 * int((t < -1e-3).sum())


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_bond_reorientation(hip_ctx, form):
    """bond_reorient on the negative-diagonal forms, bond_reorient_exact on the rotated cell, within the budget of
    tests/reorientation_ref.py; the planted guard-band case in the same form"""
    from tests import reorientation_cases as cases
    from tests import test_gpu_reorientation as R
    fast = form in NEG_DIAG
    name = ("rect@" if fast else "sheared@") + form
    _small_cell(form, cases.DIAG, cases.SHEARED)
    assert np.array_equal(cases.case(name).packed.cell[0], CF.apply(cases.DIAG if fast else cases.SHEARED, form))
    R._case(hip_ctx, name, R.FAST_RUNS if fast else R.EXACT_RUNS + [(R.FRAMES, "bond_reorient_exact")], device=True)
    runs = [({}, "bond_reorient"), (R.EXACT, "bond_reorient_exact"), (R.FRAMES, "bond_reorient")] if fast else R.EXACT_RUNS
    got, scale, want = R._case(hip_ctx, "planted2@" + form, runs)
    t = cases.planted(2, 42, CF.apply(cases.DIAG, form))[1].band_units()
    assert int((t < -1e-3).sum()) >= 5 and int((t > 1e-3).sum()) >= 5 and int((np.abs(t) <= 1.0).sum()) >= 5
    assert int(got[:, 2, 0].sum()) >= 2 * int((t < -1e-3).sum())


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_bond_order(hip_ctx, form):
    """order_frame and order_exact within the budget of bond_order_ref.check, n tied to cn_count (both in
    test_gpu_bond_order.py's _case)"""
    from tests import bond_order_cases as cases
    from tests import test_gpu_bond_order as O
    from tests.test_gpu_bond import _abi
    fast = form in NEG_DIAG
    name = ("rect@" if fast else "sheared@") + form
    _small_cell(form, cases.DIAG, cases.SHEARED)
    c = cases.case(name)
    assert np.array_equal(c.packed.cell[0], CF.apply(cases.DIAG if fast else cases.SHEARED, form))
    rcm, sets = _abi(c.packed, c.sets)
    base = cases.case(name.split("@")[0])
    frame = O._frame_tier_applies(hip_ctx, base.packed, *_abi(base.packed, base.sets))
    assert O._frame_tier_applies(hip_ctx, c.packed, rcm, sets) == frame, (form, frame)      # the tier the base cell takes
    assert frame or not fast
    hist, hist_tet, sums, pa = O._case(hip_ctx, name, [({}, "order_frame" if frame else "order_exact"), (O.EXACT, "order_exact")],
                                       device=True)
    assert sums[:, :, 3].sum() > 0 and hist_tet.sum() > 0


def _small_walk(form, F, seed):
    from tests import test_gpu_bond as B
    return B._walk(_small_cell(form, B.DIAG, B.SHEARED), B._numbers4(131), F, seed)


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_structure_factor_and_intermediate_scattering(hip_ctx, form):
    from amof_amd import structure_factor as sf
    from tests import test_gpu_isf as I
    from tests import test_gpu_sq as S
    packed = _small_walk(form, 6, 51)
    hkl = S._hkl(packed, 2.0)
    assert len(hkl) > 50
    S._check(hip_ctx, packed, hkl, 0.05, sf.n_bins(2.0, 0.05))
    assert hip_ctx.last_path() == "sq"
    I._check(hip_ctx, packed, hkl, [0, 1, 4], 0.05, sf.n_bins(2.0, 0.05))
    assert hip_ctx.last_path() == "isf"


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_window_vanhove(hip_ctx, form):
    """msd_vanhove against tests/vanhove_ref.py; unwrap=True on `mirror`"""
    from tests import test_gpu_vanhove as VH
    c = _small_cell(form, np.diag([5.0, 6.0, 7.0]), np.array([[9.0, 0.0, 0.0], [2.5, 8.5, 0.0], [-1.5, 2.0, 9.5]]))
    packed = VH._gas_walk(64, 100, c, [1] * 40 + [8] * 24, 0.6 if form == "mirror" else 0.15, 13)
    VH._check(hip_ctx, packed, [0, 1, 4, 10, 49], 0.05, 120, unwrap=form == "mirror")
    assert hip_ctx.last_path() == "msd_vanhove"


@pytest.mark.parametrize("form", ANALYSIS_FORMS)
def test_window_msd(hip_ctx, form):
    """msd_fused on the negative-diagonal forms (and unwrap=True on `mirror`); the stream, comb and group kernels on the
    rotated cell; numpy_oracle at the rtol = 1e-9 of test_gpu_msd_fused.py"""
    from amof_amd.frames import PackedTrajectory
    from oracle import numpy_oracle as no
    from tests import test_gpu_msd_fused as M
    base = np.diag([9.0, 10.0, 11.0])
    if form in NEG_DIAG:
        c = _small_cell(form, base, None)
        packed = M._walk(1000, 24, 77, c)
        window = (np.arange(8) * 100).astype(np.int32)
        got, kinds = hip_ctx.msd_window(packed, window)
        assert hip_ctx.last_path() == "msd_fused", form
        M._check_oracle(packed, window, got, kinds)
        if form == "mirror":
            got, kinds = hip_ctx.msd_window(packed, window, unwrap=True)
            elements, ref = no.window_msd_fast(packed.pos, packed.cell, packed.numbers, packed.masses, window, unwrap=True)
            for e, r in zip(elements, ref):
                g = got[kinds.index(int(e))] / (packed.numbers == e).sum() / (packed.n_frames - window)
                np.testing.assert_allclose(g, r, rtol=1e-9, atol=1e-12)
        return
    flat = M._walk(300, 12, 1, base)
    c = CF.check(base, "rot")
    assert CF.view(c)["nonzero"] == 9
    packed = PackedTrajectory(flat.pos @ CF.Q, c, flat.numbers)
    for window, want in ((np.arange(4) * 64, "msd_stream"), (np.arange(30) * 8, "msd_comb"), (np.array([0, 3, 50, 161]), "msd_group")):
        window = window.astype(np.int32)
        got, kinds = hip_ctx.msd_window(packed, window)
        assert hip_ctx.last_path() == want, (form, want)
        M._check_oracle(packed, window, got, kinds)


@pytest.mark.parametrize("form", NEG_DIAG)
def test_direct_msd_refuses_a_negative_diagonal(hip_ctx, form):
    from tests import test_gpu_msd_fused as M
    packed = M._walk(20, 12, 3, CF.check(np.diag([9.0, 10.0, 11.0]), form))
    with pytest.raises(ValueError, match="DirectMsd needs positive cell diagonals"):
        hip_ctx.msd_direct(packed)
