"""The surface stage on the GPU (amof_pore_surface, Pore(surface=True)).  Exposure is a discrete function of (positions, radii,
probe, directions): every assertion is exact equality -- the per-sample bytes against the restatement of
tests/pore_surface_ref.py (tests/test_pore_surface_host.py asserts that no sample of any case lies within its budget of a
decision), "pore_surface_list" against "pore_surface_exact" bit for bit, last_path() asserted per run.  Inputs:
tests/pore_surface_cases.py."""

import functools

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from tests import pore_access_ref as aref
from tests import pore_cases
from tests import pore_surface_cases as scases
from tests import pore_surface_ref as sref
from tests.test_gpu_bond import _device, _env

pytestmark = pytest.mark.gpu

LIST, EXACT = "pore_surface_list", "pore_surface_exact"
FORCE = {"AMOF_PORE_SURFACE_EXACT": "1"}


def _same(a, b):
    return len(a) == len(b) and all(x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def _species_sums(flags, species, S):
    """int64 [F][n_t][S] from bool [F][n_t][N][M]"""
    per_atom = flags.sum(axis=3)
    return np.stack([per_atom[:, :, species == s].sum(axis=2) for s in range(S)], axis=2).astype(np.int64)


# ---- 1. every case, all paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", scases.NAMES + scases.FORMS)
def test_every_path_batching_residence_and_frame_range(hip_ctx, name):
    c = scases.case(name)
    packed = c.packed
    F, S = packed.pos.shape[0], len(c.kinds)
    periodic = all(packed.pbc)
    fast = LIST if periodic else EXACT
    args = (c.radii, c.grid, c.dr, c.dmax, c.thresholds)

    def run(inp, env, path, **kw):
        with _env(**env):
            got = hip_ctx.pore_surface(inp, *args, dirs=c.dirs, per_point=True, **kw)
            assert hip_ctx.last_path() == path, (env, hip_ctx.last_path())
        return got

    first = run(packed, {}, fast)
    hist, counts, vmax, argmax, field, exposed, samples = first
    assert exposed.dtype == np.int64 and samples.dtype == np.uint8
    assert samples.shape == (F, 3, len(packed.numbers), len(c.dirs)) and exposed.shape == (F, 3, S)
    # the bytes are the restatement's, the counts their sums per species
    assert np.array_equal(samples, scases.bytes_of(name)), (name, int((samples != scases.bytes_of(name)).sum()))
    assert np.array_equal(exposed, _species_sums(samples > 0, c.species, S))
    # the first outputs and the field are amof_pore_field's, bit for bit
    assert _same((hist, counts, vmax, argmax, field), hip_ctx.pore_field(packed, *args, per_point=True))
    stages = hip_ctx.last_stage_seconds(pore=True)
    hip_ctx.debug_poison()
    exact, one = {"AMOF_PORE_EXACT": "1"}, {"AMOF_PORE_BATCH": "1"}
    unsorted = {"AMOF_PORE_SURFACE_UNSORTED": "1"}         # (the neighbour records in the order of the gather)
    for env, path in ((FORCE, EXACT), (one, fast), (exact, fast), (dict(FORCE, **one), EXACT), (unsorted, fast)):
        assert _same(run(packed, env, path), first), (name, env)
    assert _same(run(_device(packed), {}, fast), first)
    assert _same(run(_device(packed), FORCE, EXACT), first)
    # without the per-sample bytes, and with everything else asked for: the same integers, the other outputs those of pore_psd
    assert _same(hip_ctx.pore_surface(packed, *args, dirs=c.dirs), first[:4] + (exposed,))
    if F > 1:
        h = F // 2
        a, b = run(packed, {}, fast, frame_range=(0, h)), run(packed, {}, fast, frame_range=(h, F))
        assert _same([np.concatenate([x, y]) for x, y in zip(a, b)], first)
        multi = _hip.MultiContext([0, 0])
        try:
            assert _same(multi.pore_surface(packed, *args, dirs=c.dirs, per_point=True), first)
        finally:
            multi.close()
    if name == "rect":
        hip_ctx.pore_surface(packed, *args, dirs=c.dirs)
        stages = hip_ctx.last_stage_seconds(pore=True)
        assert stages["surface"] > 0 and stages["corr"] > 0 and stages["cover"] == 0.0
        st = hip_ctx.pore_surface_stats()
        assert st["atoms"] == F * 3 * len(packed.numbers) and st["samples"] == st["atoms"] * len(c.dirs) and st["records"] > 0
        assert 0 < st["early_exits"] <= st["samples"]
    assert stages["surface"] >= 0


def test_with_psd_access_and_free_sphere_the_other_outputs_are_pore_psds(hip_ctx):
    c = scases.case("rect")
    args = (c.packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds)
    kw = dict(per_point=True, accessibility=True, free_sphere=True, labels=True)
    want = hip_ctx.pore_psd(*args, **kw)
    got = hip_ctx.pore_surface(*args, dirs=c.dirs, psd=True, **kw)
    assert hip_ctx.last_path() == LIST
    assert len(got) == len(want) + 3 and _same(got[:len(want)], want)
    assert np.array_equal((got[-1] > 0).astype(np.uint8), scases.bytes_of("rect"))
    # labelled without the covering stage: pore_access' outputs
    want = hip_ctx.pore_access(*args, per_point=True, free_sphere=True, labels=True)
    got2 = hip_ctx.pore_surface(*args, dirs=c.dirs, **kw)
    assert _same(got2[:len(want)], want) and _same(got2[len(want):], got[-3:])


# ---- 2. planted decisions -----------------------------------------------------------------------------------------------------
def test_planted_decisions_on_both_paths(hip_ctx):
    packed, dirs, plants = scases.planted()
    R = [pore_cases.TABLE[30]]
    args = (packed, R, pore_cases.PLANT_GRID, pore_cases.PLANT_DR, pore_cases.PLANT_DMAX, scases.PLANT_THR)
    got = {}
    for env, path in (({}, LIST), (FORCE, EXACT)):
        with _env(**env):
            got[path] = hip_ctx.pore_surface(*args, dirs=dirs, per_point=True)
            assert hip_ctx.last_path() == path
        samples = got[path][-1]
        for f, k, sd in plants:
            assert samples[f, k, 0, scases.PLANT_SAMPLE] == (1 if sd > 0 else 0), (path, f, k, sd)
            assert samples[f, k, 2:].all()
    assert _same(got[LIST], got[EXACT])
    # the planted samples are decided in float64: the list path re-decided at least one sample per planted frame
    hip_ctx.pore_surface(*args, dirs=dirs)
    assert hip_ctx.last_path() == LIST and hip_ctx.pore_surface_stats()["redecisions"] >= len(plants)


# ---- 3. known answers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env, path", [({}, LIST), (FORCE, EXACT)])
def test_one_atom_and_two_atoms(hip_ctx, env, path):
    R = [pore_cases.TABLE[30]]
    grid = (scases.CUBE_GRID, scases.CUBE_DR, scases.CUBE_DMAX)
    for M in (1, 64, 100):
        dirs = P.sphere_points(M)
        with _env(**env):
            exposed = hip_ctx.pore_surface(scases.one_atom(), R, *grid, (0.0, 1.2, 2.0), dirs=dirs)[-1]
            assert hip_ctx.last_path() == path
        assert exposed.tolist() == [[[M], [M], [M]]]
        for k, rp in enumerate((0.0, 1.2, 2.0)):
            rho = np.float64(R[0]) + np.float64(rp)
            assert P.surface_area(exposed[:, k], R, rp, M)[0] == (4.0 * np.pi) * rho * rho * np.float64(M) / np.float64(M)
    dirs = P.sphere_points(scases.PAIR_M)
    edge = scases.PAIR_D / (2.0 * (R[0] + scases.PAIR_RP))
    assert np.abs(dirs[:, 2] - edge).min() > 1e-6
    with _env(**env):
        res = hip_ctx.pore_surface(scases.two_atoms(), R, *grid, (scases.PAIR_RP,), dirs=dirs, per_point=True)
        assert hip_ctx.last_path() == path
    samples = res[-1][0, 0]
    assert np.array_equal(samples[0], (dirs[:, 2] <= edge).astype(np.uint8))
    assert np.array_equal(samples[1], (dirs[:, 2] >= -edge).astype(np.uint8))
    want = scases.PAIR_M * (1.0 + edge) / 2.0
    assert abs(int(samples[0].sum()) - want) <= 1 and abs(int(samples[1].sum()) - want) <= 1
    assert res[-2].tolist() == [[[int(samples.sum())]]]


# ---- 4. accessibility ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _channels(field_bytes, shape, thresholds, pbc):
    """bool [F][n_t][nx][ny][nz]: the points of the channels of V(rp), by the restatement on the LIBRARY's field"""
    field = np.frombuffer(field_bytes, dtype=np.float64).reshape(shape)
    out = np.zeros((shape[0], len(thresholds)) + shape[1:], dtype=bool)
    for f in range(shape[0]):
        for k, t in enumerate(thresholds):
            labels, comps = aref.components(field[f] >= np.float64(t), pbc)
            out[f, k] = np.isin(labels, [c[0] for c in comps if c[2] > 0])
    return out


@pytest.mark.parametrize("name", ["rect", "zif4"])
def test_accessible_samples_are_the_corner_rule(hip_ctx, name):
    c = scases.case(name)
    packed = c.packed
    pbc = tuple(bool(x) for x in packed.pbc)
    args = (packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds)
    got = {}
    for env, path in (({}, LIST), (FORCE, EXACT)):
        with _env(**env):
            got[path] = hip_ctx.pore_surface(*args, dirs=c.dirs, per_point=True, accessibility=True)
            assert hip_ctx.last_path() == path
    assert _same(got[LIST], got[EXACT])
    hist, counts, vmax, argmax, access, field, exposed, exposed_access, samples = got[LIST]
    assert _same((hist, counts, vmax, argmax, access, field), hip_ctx.pore_access(*args, per_point=True))
    chan = _channels(field.tobytes(), field.shape, c.thresholds, pbc)
    ref = scases.reference(name)
    want = np.zeros_like(samples)
    empty = []
    for f, row in enumerate(ref):
        for k, fr in enumerate(row):
            assert not sref.corners(fr.samples, scases._cell(packed, f), c.grid, pbc)[1][fr.exposed].any()
            acc = sref.accessible(fr.exposed, fr.samples, scases._cell(packed, f), c.grid, pbc, chan[f, k])
            want[f, k] = fr.exposed.astype(np.uint8) + acc.astype(np.uint8)
            assert bool(chan[f, k].any()) == bool(access[f, k, 1] > 0)
            if not chan[f, k].any():
                empty.append((f, k))
    assert np.array_equal(samples, want), int((samples != want).sum())
    S = len(c.kinds)
    assert np.array_equal(exposed, _species_sums(samples > 0, c.species, S))
    assert np.array_equal(exposed_access, _species_sums(samples == 2, c.species, S))
    assert (exposed_access <= exposed).all() and (samples == 2).any()
    # a void without a channel has no accessible sample
    for f, k in empty:
        assert not exposed_access[f, k].any()
    if name == "zif4":
        assert (0, 2) in empty and exposed[0, 2].sum() > 0
    # the counts without the bytes are the same
    assert _same(hip_ctx.pore_surface(*args, dirs=c.dirs, accessibility=True)[-2:], (exposed, exposed_access))


# ---- 5. fallback --------------------------------------------------------------------------------------------------------------
def test_a_short_list_sends_the_launch_to_the_exact_kernel(hip_ctx):
    c = scases.case("rect")
    args = (c.packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds)
    want = hip_ctx.pore_surface(*args, dirs=c.dirs, per_point=True)
    assert hip_ctx.last_path() == LIST
    launches = hip_ctx._lib.amof_last_kernel_launches(hip_ctx._h)
    with _env(AMOF_PORE_SURFACE_LIST_CAP="8"):
        got = hip_ctx.pore_surface(*args, dirs=c.dirs, per_point=True)
        assert hip_ctx.last_path() == EXACT
        assert hip_ctx._lib.amof_last_kernel_launches(hip_ctx._h) > launches
    assert _same(got, want)


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals_leave_zeros_and_a_usable_context(hip_ctx):
    c = scases.case("rect")
    args = (c.packed, c.radii, c.grid, c.dr, c.dmax)
    bad = np.array(c.dirs)
    bad[3] *= 1.0 + 1e-9
    with pytest.raises(ValueError, match="direction 3 is no unit vector"):
        hip_ctx.pore_surface(*args, c.thresholds, dirs=bad)
    with pytest.raises(ValueError, match="1 .. 4096 directions"):
        hip_ctx.pore_surface(*args, c.thresholds, dirs=np.zeros((0, 3)))
    with pytest.raises(ValueError, match="probe radii >= 0"):
        hip_ctx.pore_surface(*args, (0.0, -0.5), dirs=c.dirs)
    # 1.39 + 6 A above half the smallest height, 7.15 A, while dmax + 1.39 is not
    with pytest.raises(ValueError, match="would meet its own image"):
        hip_ctx.pore_surface(*args, (0.0, 6.0), dirs=c.dirs)
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.pore_surface(*args, np.zeros(120000), dirs=P.sphere_points(256), per_point=True)
    assert err.value.code == _hip.AMOF_ECAPACITY
    got = hip_ctx.pore_surface(*args, c.thresholds, dirs=c.dirs, per_point=True)
    assert np.array_equal(got[-1], scases.bytes_of("rect"))


# ---- 7. the class -------------------------------------------------------------------------------------------------------------
def test_class_on_rattled_zif4(hip_ctx):
    c = scases.case("zif4")
    packed = c.packed
    kw = dict(probe_radius=(0.0, 1.2), spacing=0.5, dr=0.2, dmax=4.0, distributed=False, device=hip_ctx.device)
    plain = P.Pore.from_trajectory(packed, psd=True, accessibility=True, free_sphere=True, **kw)
    off = P.Pore.from_trajectory(packed, psd=True, accessibility=True, free_sphere=True, surface=False, **kw)
    assert off.data.equals(plain.data) and not hasattr(off, "exposed")
    obj = P.Pore.from_trajectory(packed, psd=True, accessibility=True, free_sphere=True, per_point=True, surface=True, surface_points=64, **kw)
    base = list(plain.data.columns)
    assert obj.data[base].equals(plain.data)
    dirs = P.sphere_points(64)
    res = hip_ctx.pore_surface(packed, c.radii, obj.grid, 0.2, 4.0, (0.0, 1.2), dirs=dirs, per_point=True, accessibility=True,
                               free_sphere=True, labels=True, psd=True)
    exposed, exposed_access, samples = res[-3:]
    assert np.array_equal(obj.exposed, exposed) and np.array_equal(obj.exposed_access, exposed_access)
    assert np.array_equal(obj.surface_samples, samples) and obj.surface_points == 64
    mass = float(np.asarray(packed.masses, dtype=np.float64).sum())
    cols = P.surface_columns(exposed, exposed_access, c.radii, plain.data["Unitcell_volume"].to_numpy(), mass, [0.0, 1.2], 64)
    assert list(obj.data.columns) == base + list(cols)
    for name, col in cols.items():
        assert np.array_equal(obj.data[name].to_numpy(), col), name
    assert (obj.data["ASA_A^2-1.2"] + obj.data["NASA_A^2-1.2"]).to_numpy() == pytest.approx(obj.data["SA_A^2-1.2"].to_numpy(), rel=1e-14)
    assert obj.surface_by_species.shape == (1, 2 * len(c.kinds))
    assert obj.surface_by_species.filter(like="-1.2").sum(axis=1).to_numpy() == pytest.approx(obj.data["SA_A^2-1.2"].to_numpy(), rel=1e-14)
    # the surface alone, synchronous, and the default number of points
    with _env(AMOF_ASYNC="0"):
        alone = P.Pore.from_trajectory(packed, surface=True, **kw)
    assert alone.surface_points == 256 and not hasattr(alone, "exposed_access") and "ASA_A^2-0" not in alone.data
    want = hip_ctx.pore_surface(packed, c.radii, alone.grid, 0.2, 4.0, (0.0, 1.2), dirs=P.sphere_points(256))[-1]
    assert np.array_equal(alone.exposed, want) and alone.data["SA_A^2-0"][0] > alone.data["SA_A^2-1.2"][0] > 0


def test_class_through_a_stream(hip_ctx, tmp_path):
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    c = scases.case("rect")
    packed = c.packed
    path = str(tmp_path / "rect.xyz")
    T.write_xyz(path, packed, comment_lattice=False, fmt="%.17g")
    kw = dict(probe_radius=(0.0, 1.2), grid=c.grid, dr=c.dr, dmax=c.dmax, distributed=False, device=hip_ctx.device, surface=True,
              surface_points=64, accessibility=True)
    whole = P.Pore.from_trajectory(packed, **kw)
    streamed = P.Pore.from_trajectory(XyzStream(path, cell=packed.cell[0], batch_frames=2), **kw)
    assert np.array_equal(streamed.exposed, whole.exposed) and np.array_equal(streamed.exposed_access, whole.exposed_access)
    cols = [n for n in whole.data.columns if "SA_" in n]
    assert len(cols) == 18 and streamed.data[cols].equals(whole.data[cols])
