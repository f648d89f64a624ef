"""The pore field on the GPU (amof_pore_field, Pore): the field within the derived budget of tests/pore_ref.py everywhere and
bit-identical between every forced path, batch setting, input residence and frame range; the rows, probe counts, largest
value and its index exactly what numpy computes by the documented rule from the library's own field, the rows the
restatement's (no grid point of any input lies within the budget of a decision: tests/test_pore_host.py); the inside count
amof_cn_count's with the grid points appended as probe atoms; last_path() asserted per run.  Inputs: tests/pore_cases.py."""

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from tests import pore_cases as cases
from tests import pore_ref as ref
from tests.test_gpu_bond import _device, _env

pytestmark = pytest.mark.gpu

EXACT = {"AMOF_PORE_EXACT": "1"}
ONE_FRAME = {"AMOF_PORE_BATCH": "1"}


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and np.array_equal(x, y) for x, y in zip(a, b))


def _call(hip_ctx, c, inp, env, path, **kw):
    with _env(**env):
        got = hip_ctx.pore_field(inp, c.radii, c.grid, c.dr, c.dmax, c.thresholds, per_point=True, **kw)
        ran = hip_ctx.last_path()
    assert ran == path, (env, ran, path)
    return got


def _case(hip_ctx, name, fast="pore_brick"):
    """every forced path, a one-frame batch setting and host / device input on a case; returns the first result"""
    c = cases.case(name)
    want, _ = cases.reference(name)
    packed = c.packed
    F = packed.pos.shape[0]
    runs = [({}, fast), (EXACT, "pore_exact"), (ONE_FRAME, fast), (dict(EXACT, **ONE_FRAME), "pore_exact")]
    first = None
    for env, path in runs:
        for inp in (packed, _device(packed)):
            got = _call(hip_ctx, c, inp, env, path)
            hist, counts, vmax, argmax, field = got
            assert hist.shape == (F, c.nbins + 2) and hist.dtype == np.uint64 and counts.shape == (F, len(c.thresholds))
            assert field.shape == (F,) + c.grid and vmax.shape == argmax.shape == (F,)
            if first is None:
                first = got
                worst = ref.check_field(field, want)
                print("%s %s: largest |difference| / budget = %.3g" % (name, path, worst))
                # rows, probe counts, the largest value and its index by the documented rule from the library's own field
                assert _same(ref.from_field(field, c.dr, c.dmax, c.thresholds), (hist, counts, vmax, argmax))
                # no point of the restatement is within its budget of a decision: its rows are the library's
                assert np.array_equal(hist, want.rows) and np.array_equal(counts, want.counts)
                assert hist.sum(axis=1).tolist() == [c.G] * F
                # inside an atom <=> a neighbour of amof_cn_count with the grid points appended as probe atoms
                both, rcm, sets, is_probe = cases.with_probes(c)
                _, pa = hip_ctx.cn_count(both, rcm, sets, per_atom=True)
                inside = pa[:, :, is_probe].sum(axis=1) > 0
                assert np.array_equal(inside.reshape(field.shape), field < 0.0)
                assert np.array_equal(inside.sum(axis=1).astype(np.uint64), hist[:, 0])
            assert _same(got, first), (name, env, path)
            assert _same(hip_ctx.pore_field(inp, c.radii, c.grid, c.dr, c.dmax, c.thresholds), first[:4]) if env == {} else True
    # frame-range halves concatenate to the whole, the field included
    if F > 1:
        h = F // 2
        for env, path in runs[:2]:
            a = _call(hip_ctx, c, packed, env, path, frame_range=(0, h))
            b = _call(hip_ctx, c, packed, env, path, frame_range=(h, F))
            assert _same([np.concatenate([x, y]) for x, y in zip(a, b)], first), (name, env)
    return first


def test_rectangular_one_species_ragged_bricks(hip_ctx):
    hist, counts, vmax, argmax, field = _case(hip_ctx, "rect")
    stages = hip_ctx.last_stage_seconds()
    assert stages["rho"] >= 0 and stages["corr"] >= 0               # cell sort, field kernels
    assert (hist[:, 0] > 0).all() and (counts[:, 0] > counts[:, 1]).all() and (counts[:, 1] > counts[:, 2]).all()


def test_rattled_zif4_with_table_radii(hip_ctx):
    c = cases.case("zif4")
    assert np.array_equal(c.radii, P.species_radii(c.kinds))
    hist, counts, vmax, argmax, field = _case(hip_ctx, "zif4")
    assert 0.4 < hist[0, 0] / c.G < 0.6                              # about half of ZIF-4's cell lies inside a van der Waals sphere
    assert 2.0 < 2.0 * vmax[0] < 6.0                                 # its largest cavity: a few Angstrom across


@pytest.mark.parametrize("name", ["sheared", "npt_diag", "npt_sheared"])
def test_general_and_per_frame_cells(hip_ctx, name):
    _case(hip_ctx, name)


def test_open_axis_takes_the_exact_path(hip_ctx):
    _case(hip_ctx, "open", fast="pore_exact")


@pytest.mark.parametrize("name", cases.FORMS)
def test_rotated_left_handed_negated_and_permuted_cells(hip_ctx, name):
    _case(hip_ctx, name)


def test_planted_decisions_inside_the_candidate_guard_band(hip_ctx):
    c = cases.case("planted")
    d_small, d_band = cases.plant_deltas()
    assert _hip.pore_candidate_bound(cases.PLANT_CELL, c.dmax + c.radii.max()) == 4.0 * d_band
    hist, counts, vmax, argmax, field = _case(hip_ctx, "planted")
    want, raw = cases.reference("planted")
    flat = field.reshape(field.shape[0], -1)
    for f, g, what, e, sd in c.plants:
        # delta is a hundred budgets and a quarter (or a 600th) of the candidate's bound: only float64 decides these
        assert abs(flat[f, g] - min(e + sd, c.dmax)) <= 2.0 * want.budget[f, g], (f, g, what)
    assert (hist[:, -1] > 0).all() and (vmax == c.dmax).all() and (argmax == 0).all()     # overflow: the first point has it


def test_known_answer_simple_cubic(hip_ctx):
    from amof_amd.frames import PackedTrajectory
    a, R, reps, n = 4.0, 1.0, 3, 27
    sites = np.array([(i, j, k) for i in range(reps) for j in range(reps) for k in range(reps)], dtype=np.float64) * a
    packed = PackedTrajectory(sites[None], np.diag([a * reps] * 3), np.full(len(sites), 30))
    for env, path in (({}, "pore_brick"), (EXACT, "pore_exact")):
        with _env(**env):
            hist, counts, vmax, argmax = hip_ctx.pore_field(packed, [R], (n, n, n), 0.1, 3.0, (0.0,))
            assert hip_ctx.last_path() == path
        assert vmax[0] == pytest.approx(a * np.sqrt(3.0) / 2.0 - R, rel=1e-12)
        assert argmax[0] == (4 * n + 4) * n + 4                      # the first body centre in index order
        assert hist[0, -1] == 0 and hist.sum() == n ** 3


def test_refusals_and_capacity(hip_ctx):
    c = cases.case("rect")
    good = hip_ctx.pore_field(c.packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds)
    for kw in (dict(dmax=6.0), dict(radii=[-1.0]), dict(radii=[np.nan]), dict(thresholds=[np.inf])):
        args = dict(radii=c.radii, grid=c.grid, dr=c.dr, dmax=c.dmax, thresholds=c.thresholds)
        args.update(kw)
        with pytest.raises(ValueError):
            hip_ctx.pore_field(c.packed, **args)
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.pore_field(c.packed, c.radii, c.grid, 0.001, 4.0, c.thresholds)       # 4000 bins
    assert err.value.code == _hip.AMOF_ECAPACITY
    assert _same(hip_ctx.pore_field(c.packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds), good)     # the context works afterwards


def test_class_on_zif4(hip_ctx, monkeypatch, caplog):
    from tests import bond_order_cases as BO
    packed = BO.zif4_rattled(F=3, seed=9)
    kw = dict(spacing=0.5, dr=0.2, dmax=4.0, device=0, distributed=False)
    monkeypatch.setenv("AMOF_ASYNC", "0")
    seq = P.Pore.from_trajectory(packed, delta_Step=5, **kw)
    assert seq.__dict__.get("_pending") is None
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = P.Pore.from_trajectory(packed, delta_Step=5, **kw)
    assert obj.__dict__.get("_pending") is not None and obj._ctx is _hip.get_context(0, lane=1)
    assert obj.data.equals(seq.data) and obj.hist.equals(seq.hist) and np.array_equal(obj.counts, seq.counts)
    assert obj._stats["path"] == "pore_brick" and obj._stats["kernel_s_dominant"] > 0
    # .data is ``assemble`` of the ABI's integers
    grid = P.default_grid(packed.cell[0], 0.5)
    radii = P.species_radii([1, 6, 7, 30])
    hist, counts, vmax, argmax = hip_ctx.pore_field(packed, radii, grid, 0.2, 4.0, (0.0, 1.2))
    volume = np.full(3, abs(np.linalg.det(packed.cell[0])))
    data, h = P.assemble(hist, counts, vmax, np.arange(0, 15, 5), volume, packed.masses.sum(), [0.0, 1.2], grid, 0.2)
    assert obj.data.equals(data) and obj.hist.equals(h) and obj.grid == grid and obj.dmax == 4.0
    assert np.array_equal(obj.di_position, P.positions(argmax, packed.cell, grid))
    assert np.isfinite(obj.data["Di"]).all() and (obj.data["PCV_Volume_fraction-0"] > obj.data["PCV_Volume_fraction-1.2"]).all()
    # a dmax below the largest value: overflow points, Di = inf and a warning
    with caplog.at_level("WARNING", logger="amof_amd.pore"):
        low = P.Pore.from_trajectory(packed, **dict(kw, dmax=1.0))
        assert np.isinf(low.data["Di"]).all() and (low.counts[:, -1] > 0).all()
    assert any("raise dmax" in r.getMessage() for r in caplog.records)
    # per_point keeps the field; the default dmax is the rule's
    full = P.Pore.from_trajectory(packed, per_point=True, **dict(kw, dmax=None))
    assert full.field.shape == (3,) + grid
    assert full.dmax == P.default_dmax(packed.cell, packed.pbc, 1.70, 0.2)
    assert np.array_equal(ref.from_field(full.field, 0.2, full.dmax, (0.0, 1.2))[0], full.counts)
