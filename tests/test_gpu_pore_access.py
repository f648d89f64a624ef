"""Accessibility of the pore field on the GPU (amof_pore_access, amof_pore_access_field, Pore(accessibility=, free_sphere=)).
Labelling is a discrete function of (field, thresholds): every assertion is exact equality -- labels, access rows and t* against
the restatement of tests/pore_access_ref.py (a breadth-first search that carries image offsets, another algorithm than the
library's), the LDS path against the all-in-device-memory path (AMOF_PORE_LABEL_GLOBAL=1) bit for bit, last_path() asserted
per run.  Inputs: tests/pore_access_cases.py (synthetic topologies, the simple-cubic frames) and tests/pore_cases.py (atoms)."""

import ctypes
import functools

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from amof_amd.frames import PackedTrajectory
from tests import pore_access_cases as acases
from tests import pore_access_ref as aref
from tests import pore_cases
from tests.test_gpu_bond import _device, _env

pytestmark = pytest.mark.gpu

TILE, GLOBAL = "pore_label_tile", "pore_label_global"
PATHS = [({}, TILE), ({"AMOF_PORE_LABEL_GLOBAL": "1"}, GLOBAL)]
THRESHOLDS = (0.0, 0.6, 1.2)


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y))
                                    for x, y in zip(a, b))


def _unzeroed(arrays):
    """the names of the arrays a refusal left something in"""
    return [k for k, v in arrays.items() if v.any()]


# ---- 1. synthetic fields ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", acases.NAMES)
def test_synthetic_topologies(hip_ctx, name):
    c = acases.case(name)
    want = acases.reference(name)
    got = {}
    for env, path in PATHS:
        with _env(**env):
            got[path] = hip_ctx.pore_access_field(c.field, c.pbc, c.thresholds, free_sphere=True, labels=True)
            assert hip_ctx.last_path() == path
        access, free, labels = got[path]
        assert access.dtype == np.int64 and labels.dtype == np.int32 and free.dtype == np.float64
        assert np.array_equal(labels, want[1]), (name, path)
        assert np.array_equal(access, want[0]), (name, path, access.tolist(), want[0].tolist())
        assert np.array_equal(free, want[2]), (name, path, free.tolist(), want[2].tolist())
    assert _same(got[TILE], got[GLOBAL])
    # the answers without the optional outputs are the same
    access, free, labels = hip_ctx.pore_access_field(c.field, c.pbc, c.thresholds)
    assert free is None and labels is None and np.array_equal(access, want[0])


def test_several_frames_and_scratch_left_by_other_calls(hip_ctx):
    """three fields of one grid as three frames, poisoned scratch in between: nothing depends on what a call left behind"""
    names = ["u_shape", "helix", "boxes"]
    field = np.concatenate([acases.case(n).field for n in names])
    want = [np.concatenate([acases.reference(n)[k] for n in names]) for k in (0, 2, 1)]         # access, free sphere, labels
    first = hip_ctx.pore_access_field(field, acases.PBC, (0.0,), free_sphere=True, labels=True)
    assert _same(first, want)
    hip_ctx.debug_poison()
    assert _same(hip_ctx.pore_access_field(field, acases.PBC, (0.0,), free_sphere=True, labels=True), first)


# ---- 2. atoms ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _restated(name, field_bytes, shape, dmax):
    """the restatement on the LIBRARY's field (passed as bytes: hashable), computed once per case"""
    field = np.frombuffer(field_bytes, dtype=np.float64).reshape(shape)
    pbc = tuple(bool(x) for x in pore_cases.case(name).packed.pbc)
    rows, labels, free = [], [], []
    for f in range(shape[0]):
        r, l = aref.access(field[f], THRESHOLDS, pbc)
        rows.append(r)
        labels.append(l)
        free.append(aref.free_sphere(field[f], pbc, dmax=dmax))
    return np.array(rows, dtype=np.int64), np.array(labels, dtype=np.int32), np.array(free, dtype=np.float64)


@pytest.mark.parametrize("name", ["rect", "zif4", "sheared", "npt_sheared", "open"])
def test_atoms_every_path_batching_residence_and_frame_range(hip_ctx, name):
    c = pore_cases.case(name)
    packed = c.packed
    F = packed.pos.shape[0]
    args = (c.radii, c.grid, c.dr, c.dmax, THRESHOLDS)
    plain = hip_ctx.pore_field(packed, *args, per_point=True)

    def run(inp, env, path, **kw):
        with _env(**env):
            got = hip_ctx.pore_access(inp, *args, per_point=True, free_sphere=True, labels=True, **kw)
            assert hip_ctx.last_path() == path, (env, hip_ctx.last_path())
        return got

    first = run(packed, {}, TILE)
    hist, counts, vmax, argmax, access, free, field, labels = first
    # the first outputs and the field are amof_pore_field's, bit for bit
    assert _same((hist, counts, vmax, argmax, field), plain)
    want = _restated(name, field.tobytes(), field.shape, c.dmax)
    assert np.array_equal(labels, want[1]) and np.array_equal(access, want[0]), (access.tolist(), want[0].tolist())
    assert np.array_equal(free, want[2]), (free.tolist(), want[2].tolist())
    assert np.array_equal(access[:, :, 0] <= counts, np.ones_like(counts, dtype=bool))
    hip_ctx.debug_poison()
    exact, one = {"AMOF_PORE_EXACT": "1"}, {"AMOF_PORE_BATCH": "1"}
    for env, path in (({}, TILE), (PATHS[1][0], GLOBAL), (exact, TILE), (one, TILE), (dict(exact, **one, **PATHS[1][0]), GLOBAL)):
        assert _same(run(packed, env, path), first), (name, env)
    assert _same(run(_device(packed), {}, TILE), first)
    assert _same(hip_ctx.pore_access(packed, *args), first[:5])
    if F > 1:
        h = F // 2
        a, b = run(packed, {}, TILE, frame_range=(0, h)), run(packed, {}, TILE, frame_range=(h, F))
        assert _same([np.concatenate([x, y]) for x, y in zip(a, b)], first)
        # two contexts of one device sharing the frames: the sharded twin concatenates every output
        multi = _hip.MultiContext([0, 0])
        try:
            assert _same(multi.pore_access(packed, *args, per_point=True, free_sphere=True, labels=True), first)
            assert _same(multi.pore_access(packed, *args), first[:5])
        finally:
            multi.close()


# ---- 3. the simple-cubic known answers, through the library -------------------------------------------------------------------
@pytest.mark.parametrize("c_over, want", [(None, [(1, 0, 3), (1, 0, 3), (0, 27, 0)]), (3.0, [(1, 0, 3), (9, 0, 1), (0, 27, 0)])])
def test_simple_cubic_free_sphere(hip_ctx, c_over, want):
    pos, cell, grid = acases.simple_cubic(c_over)
    packed = PackedTrajectory(pos, cell, np.full(27, 30))
    for env, path in PATHS:
        with _env(**env):
            hist, counts, vmax, argmax, access, free, field = hip_ctx.pore_access(packed, [acases.SC_R], grid, acases.SC_DR, acases.SC_DMAX,
                                                                                  acases.SC_PROBES, per_point=True, free_sphere=True)
            assert hip_ctx.last_path() == path
        assert [tuple(r[1:]) for r in access[0].tolist()] == want
        tstar, half_dif = free[0]
        window = field[0, 4, 4, 0]                   # the centre of four atoms of a face: (2.25, 2.25, 0.25)
        assert 2.0 * window == 2.0 * tstar and abs(tstar - (4.0 / np.sqrt(2.0) - 1.0)) < 1e-12
        assert half_dif == vmax[0] == field.max()
        assert abs(half_dif - ((2.0 * np.sqrt(3.0) if c_over is None else np.sqrt(10.25)) - 1.0)) < 1e-12
        # V(t*) has a channel and V(nextafter(t*)) has none
        at, _, _ = hip_ctx.pore_access_field(field, acases.PBC, (tstar, np.nextafter(tstar, np.inf)))
        assert at[0, 0, 1] >= 1 and at[0, 1, 1] == 0 and at[0, 1, 2] >= 1


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable(hip_ctx):
    ok = acases.case("helix")
    with pytest.raises(ValueError, match="periodic axis"):
        hip_ctx.pore_access_field(np.ones((1, 2, 5, 5)), acases.PBC, (0.0,))
    with pytest.raises(ValueError, match="periodic axis"):
        hip_ctx.pore_access_field(np.ones((1, 5, 5, 1)), acases.PBC, (0.0,))
    c = pore_cases.case("rect")
    with pytest.raises(ValueError, match="periodic axis"):
        hip_ctx.pore_access(c.packed, c.radii, (11, 2, 17), c.dr, c.dmax, THRESHOLDS)
    # want_free without a free_sphere array: the wrapper never does that, the library refuses it
    field, grid, per, thr = ok.field, _hip._i32(ok.grid), _hip._i32([1, 1, 1]), np.zeros(1)
    access = np.zeros((1, 1, 4), dtype=np.int64)
    rc = hip_ctx._lib.amof_pore_access_field(hip_ctx._h, _hip._ptr(field), 1, _hip._ptr(grid), _hip._ptr(per), _hip._ptr(thr), 1, 1,
                                             _hip._ptr(access), None, None)
    assert rc == _hip.AMOF_EINVAL
    with pytest.raises(ValueError, match="free_sphere"):
        hip_ctx._check(rc)
    # labels beyond 4 GiB per frame: refused by the wrapper before it allocates, and by the library
    many = np.zeros(80000)           # x 13965 points x 4 bytes > 2^32
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.pore_access_field(ok.field, acases.PBC, many, labels=True)
    assert err.value.code == _hip.AMOF_ECAPACITY
    big = np.zeros((1, len(many), 4), dtype=np.int64)
    rc = hip_ctx._lib.amof_pore_access_field(hip_ctx._h, _hip._ptr(field), 1, _hip._ptr(grid), _hip._ptr(per), _hip._ptr(many), len(many), 0,
                                             _hip._ptr(big), None, ctypes.c_void_p(16))     # (refused before anything is written)
    assert rc == _hip.AMOF_ECAPACITY
    with pytest.raises(ValueError):
        hip_ctx.pore_access_field(np.full((1, 4, 4, 4), np.nan), acases.PBC, (0.0,))
    # a refusal after the sizes are known leaves zeros in every array given ("zeros after an error", include/amof_hip.h)
    lib, h, ptr = hip_ctx._lib, hip_ctx._h, _hip._ptr
    th = hip_ctx._traj(c.packed)
    F, G, far = th.n_frames, c.G, 6.0                   # dmax + R = 7.39 above half the smallest height, 7.15
    nb = int(np.rint(far / c.dr))
    grid3, thr3, radii = _hip._i32(c.grid), np.array(THRESHOLDS), np.ascontiguousarray(c.radii, dtype=np.float64)

    def sevens():
        return dict(hist=np.full((F, nb + 2), 7, dtype=np.uint64), counts=np.full((F, 3), 7, dtype=np.int64), vmax=np.full(F, 7.0),
                    argmax=np.full(F, 7, dtype=np.int64), access=np.full((F, 3, 4), 7, dtype=np.int64), free=np.full((F, 2), 7.0),
                    field=np.full((F, G), 7.0), labels=np.full((F, 3, G), 7, dtype=np.int32))

    a = sevens()
    rc = lib.amof_pore_field(h, ctypes.byref(th.c), ptr(radii), ptr(grid3), c.dr, far, ptr(thr3), 3, ptr(a["hist"]), ptr(a["counts"]),
                             ptr(a["vmax"]), ptr(a["argmax"]), ptr(a["field"]))
    assert rc == _hip.AMOF_EINVAL
    assert _unzeroed({k: a[k] for k in ("hist", "counts", "vmax", "argmax", "field")}) == []
    a = sevens()
    rc = lib.amof_pore_access(h, ctypes.byref(th.c), ptr(radii), ptr(grid3), c.dr, far, ptr(thr3), 3, 1, ptr(a["hist"]), ptr(a["counts"]),
                              ptr(a["vmax"]), ptr(a["argmax"]), ptr(a["access"]), ptr(a["free"]), ptr(a["field"]), ptr(a["labels"]))
    assert rc == _hip.AMOF_EINVAL
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx._check(rc)
    assert _unzeroed(a) == []
    bad = ok.field.copy()
    bad[0, 1, 2, 3] = np.nan
    Gf = int(np.prod(ok.grid))
    access, free, labels = np.full((1, 1, 4), 7, dtype=np.int64), np.full((1, 2), 7.0), np.full((1, 1, Gf), 7, dtype=np.int32)
    rc = lib.amof_pore_access_field(h, ptr(bad), 1, ptr(grid), ptr(per), ptr(thr), 1, 1, ptr(access), ptr(free), ptr(labels))
    assert rc == _hip.AMOF_EINVAL
    assert _unzeroed(dict(access=access, free=free, labels=labels)) == []
    # valid calls follow: the known answers
    rows, _ = pore_cases.reference("rect")
    hist, counts, _, _ = hip_ctx.pore_field(c.packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds)
    assert np.array_equal(hist, rows.rows) and np.array_equal(counts, rows.counts)
    got = hip_ctx.pore_access(c.packed, c.radii, c.grid, c.dr, c.dmax, c.thresholds)
    assert np.array_equal(got[0], rows.rows) and np.array_equal(got[1], rows.counts) and (got[4][:, :, 0] <= counts).all()
    want = acases.reference("helix")
    assert _same(hip_ctx.pore_access_field(ok.field, ok.pbc, ok.thresholds, free_sphere=True, labels=True), (want[0], want[2], want[1]))


# ---- 5. the class -----------------------------------------------------------------------------------------------------------
def test_class_on_rattled_zif4(hip_ctx):
    c = pore_cases.case("zif4")
    packed = c.packed
    kw = dict(probe_radius=(0.0, 1.2), spacing=0.5, dr=0.2, dmax=4.0, distributed=False, device=hip_ctx.device)
    plain = P.Pore.from_trajectory(packed, **kw)
    obj = P.Pore.from_trajectory(packed, accessibility=True, free_sphere=True, per_point=True, **kw)
    with _env(AMOF_ASYNC="0"):
        sync = P.Pore.from_trajectory(packed, accessibility=True, free_sphere=True, per_point=True, **kw)
    base = list(plain.data.columns)
    assert base == ["Step", "Unitcell_volume", "Density", "PCV_Volume_fraction-0", "PCV_A^3-0", "PCV_cm^3/g-0",
                    "PCV_Volume_fraction-1.2", "PCV_A^3-1.2", "PCV_cm^3/g-1.2", "Di"]
    assert not hasattr(plain, "access") and not hasattr(plain, "free_sphere") and not hasattr(plain, "labels")
    assert obj.data.equals(sync.data) and np.array_equal(obj.labels, sync.labels) and np.array_equal(obj.free_sphere, sync.free_sphere)
    assert obj.data[base].equals(plain.data)
    res = hip_ctx.pore_access(packed, c.radii, obj.grid, 0.2, 4.0, (0.0, 1.2), per_point=True, free_sphere=True, labels=True)
    hist, counts, vmax, argmax, access, free, field, labels = res
    assert np.array_equal(obj.access, access) and np.array_equal(obj.free_sphere, free) and np.array_equal(obj.labels, labels)
    assert np.array_equal(obj.field, field) and obj.labels.shape == (1, 2) + obj.grid
    mass = float(np.asarray(packed.masses, dtype=np.float64).sum())
    cols = P.access_columns(access, counts, plain.data["Unitcell_volume"].to_numpy(), mass, [0.0, 1.2], obj.grid)
    cols.update(P.free_sphere_columns(free))
    assert list(obj.data.columns) == base + list(cols)
    for name, col in cols.items():
        assert np.array_equal(obj.data[name].to_numpy(), col), name
    assert (obj.data["AV_Volume_fraction-0"] + obj.data["NAV_Volume_fraction-0"]).to_numpy() == pytest.approx(
        obj.data["PCV_Volume_fraction-0"].to_numpy(), rel=1e-15)
    assert 0.0 <= obj.data["Df"][0] <= obj.data["Dif"][0] <= obj.data["Di"][0]
