"""The covering radius of the pore field on the GPU (amof_pore_psd, amof_pore_psd_field, Pore(psd=True)).  w is a discrete
function of (field, cell, grid): every assertion is exact equality -- against the restatement of tests/pore_cover_ref.py (one
gather over the whole grid per offset, another algorithm than the brick path) and between the two paths of the library,
"pore_cover_brick" and "pore_cover_exact" (AMOF_PORE_COVER_EXACT=1), bit for bit, last_path() asserted per run.
Inputs: single-centre fields with ties planted on the sphere, the synthetic topologies of tests/pore_access_cases.py and the
atoms of tests/pore_cases.py."""

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import pore as P
from tests import pore_access_cases as acases
from tests import pore_cases
from tests import pore_cover_ref as ref
from tests.test_gpu_bond import SHEARED, _device, _env
from tests.test_gpu_pore_access import _restated, _same, _unzeroed
from tests.test_pore_cover_host import CUBE, restated_rows

pytestmark = pytest.mark.gpu

BRICK, EXACT = "pore_cover_brick", "pore_cover_exact"
PATHS = [({}, BRICK), ({"AMOF_PORE_COVER_EXACT": "1"}, EXACT)]
THRESHOLDS = (0.0, 0.6, 1.2)
PBC = (True, True, True)
DR, DMAX = 0.25, 4.0


def _both(hip_ctx, field, cells, pbc=PBC, thresholds=(0.0,), access=False):
    """``pore_psd_field`` on both paths: the same bits, and those of the restatement.  Returns (psd_hist, po_counts, po_access, w)."""
    field = np.ascontiguousarray(field, dtype=np.float64)
    got = {}
    for env, path in PATHS:
        with _env(**env):
            got[path] = hip_ctx.pore_psd_field(field, cells, pbc, DR, DMAX, thresholds, accessibility=access, per_point=True)
            assert hip_ctx.last_path() == path, (env, hip_ctx.last_path())
    assert _same(got[BRICK], got[EXACT])
    want = restated_rows(field, cells, pbc, DR, DMAX, thresholds, access)
    for path in (BRICK, EXACT):
        hist, po, acc, w = got[path]
        assert hist.dtype == np.uint64 and po.dtype == np.int64 and w.dtype == np.float64 and w.shape == field.shape
        assert np.array_equal(w, want[3]), (path, np.argwhere(w != want[3])[:5].tolist())
        assert _same((hist, po, acc), want[:3]), path
        assert (hist.sum(axis=1) == field[0].size).all()
    # without the optional outputs the answers are the same
    hist, po, acc, w = hip_ctx.pore_psd_field(field, cells, pbc, DR, DMAX, thresholds)
    assert acc is None and w is None and _same((hist, po), want[:2])
    return got[BRICK]


def _single(n, at, v):
    f = np.full((1,) + tuple(n), -1.0)
    f[(0,) + tuple(at)] = v
    return f


# ---- 1. synthetic fields ----------------------------------------------------------------------------------------------------
def test_single_centre_ties_on_the_sphere(hip_ctx):
    """step 0.5: the 30 offsets with d2 = 6.25 exactly are covered by v = 2.5 and not by the next double below"""
    hist, po, _, w = _both(hip_ctx, _single((16, 16, 16), (8, 8, 8), 2.5), CUBE)
    assert (w == 2.5).sum() == 515 and po[0, 0] == 515 and w[0, 11, 12, 8] == 2.5
    hist, po, _, w = _both(hip_ctx, _single((16, 16, 16), (8, 8, 8), np.nextafter(2.5, 0.0)), CUBE)
    assert po[0, 0] == 485 and w[0, 11, 12, 8] == -1.0


@pytest.mark.parametrize("centre, offset", [((9, 8, 7), (3, 1, -2)),          # the covered point lies in the neighbouring brick
                                            ((1, 2, 1), (3, 0, 2)),           # ... on the far side of two cell faces
                                            ((17, 9, 9), (-2, 1, 1))])        # out of the last, ragged brick through the upper face
def test_ties_in_a_sheared_cell(hip_ctx, centre, offset):
    """v(c) = sqrt(d2(D)) rounded so that v v lies on either side of d2(D): the point c - D is covered by the one, not the other"""
    n = (19, 17, 15)
    d2 = ref.offset_d2(ref.step_vectors(SHEARED, n), *offset)
    hi = np.sqrt(d2)
    while hi * hi < d2:
        hi = np.nextafter(hi, np.inf)
    while np.nextafter(hi, 0.0) * np.nextafter(hi, 0.0) >= d2:
        hi = np.nextafter(hi, 0.0)
    lo = np.nextafter(hi, 0.0)
    assert lo * lo < d2 <= hi * hi
    p = tuple((c - d) % m for c, d, m in zip(centre, offset, n))
    assert any(a // 8 != b // 8 for a, b in zip(p, centre))
    for v, covered in ((hi, True), (lo, False)):
        _, _, _, w = _both(hip_ctx, _single(n, centre, v), SHEARED)
        assert w[(0,) + p] == (v if covered else -1.0) and w[(0,) + tuple(centre)] == v


def test_two_centres_the_larger_wins(hip_ctx):
    for first, second in (((8, 8, 8), (8, 8, 10)), ((8, 8, 10), (8, 8, 8))):
        f = _single((16, 16, 16), first, 1.0)
        f[(0,) + second] = 1.5
        _, _, _, w = _both(hip_ctx, f, CUBE)
        mid = (0, 8, 8, 9)
        assert w[mid] == 1.5 and w[(0,) + first] == 1.5 and w[(0,) + second] == 1.5


def test_ragged_bricks_thin_and_open_axes(hip_ctx):
    # a centre in the last, ragged brick of a grid that is no multiple of 8: it reaches back into full bricks and on through the faces
    cell = np.diag([11 * 0.7, 13 * 0.7, 17 * 0.7])
    _, po, _, w = _both(hip_ctx, _single((11, 13, 17), (10, 12, 16), 2.9), cell)          # four steps and a little
    assert w[0, 0, 0, 0] == 2.9 and w[0, 5, 12, 16] == -1.0 and w[0, 6, 12, 16] == 2.9 and po[0, 0] > 200
    # an axis of three points: half its height is 1.5 steps
    thin = np.array([[3.0, 0.0, 0.0], [0.4, 9.0, 0.0], [0.0, 0.3, 10.0]])
    f = _single((3, 18, 20), (1, 9, 10), 1.45)
    f[0, :, 9, 10] = 1.45                       # a column that winds through the three points: a channel
    f[0, 0, 2, 3] = 1.0                         # and a pocket
    _, po, acc, _ = _both(hip_ctx, f, thin, thresholds=(0.0, 1.2), access=True)
    assert (0 < acc).all() and (acc < po)[0, 0] and acc[0, 1] == po[0, 1]
    # an open axis with a centre next to the open face: nothing is covered through that face
    f = _single((16, 16, 16), (0, 8, 8), 2.5)
    _, po, _, w = _both(hip_ctx, f, CUBE, pbc=(False, True, True))
    assert (w[0, 8:] == -1.0).all() and w[0, 5, 8, 8] == 2.5 and po[0, 0] < 515
    # one layer, open along x (the labelling's slab): a disc
    f = _single((1, 24, 40), (0, 3, 38), 3.0)
    _both(hip_ctx, f, np.diag([1.0, 24.0, 40.0]), pbc=(False, True, True), thresholds=(0.0, 2.0), access=True)


@pytest.mark.parametrize("name", ["u_shape", "helix", "boxes", "inclusive"])
def test_synthetic_topologies_covered_from_channels(hip_ctx, name):
    """fields of +-1 over steps of 0.9, 0.8, 0.7 A: a void point covers its six neighbours; a pocket's points are covered, none
    of them from a channel"""
    c = acases.case(name)
    cell = np.diag([c.grid[0] * 0.9, c.grid[1] * 0.8, c.grid[2] * 0.7])
    _, po, acc, _ = _both(hip_ctx, c.field, cell, c.pbc, c.thresholds, access=True)
    rows = acases.reference(name)[0]
    assert ((acc > 0) == (rows[:, :, 1] > 0)).all() and (acc <= po).all() and (po > 0).all()


def test_several_frames_and_scratch_left_by_other_calls(hip_ctx):
    names = ["u_shape", "helix", "boxes"]
    field = np.concatenate([acases.case(n).field for n in names])
    grid = field.shape[1:]
    cell = np.diag([grid[0] * 0.9, grid[1] * 0.8, grid[2] * 0.7])
    first = _both(hip_ctx, field, cell, PBC, (0.0,), access=True)
    assert first[2][:, 0].tolist() != [0, 0, 0] and first[2][0, 0] == 0 and first[2][2, 0] == 0
    hip_ctx.debug_poison()
    for env, path in PATHS:
        with _env(**env):
            assert _same(hip_ctx.pore_psd_field(field, cell, PBC, DR, DMAX, (0.0,), accessibility=True, per_point=True), first)
            assert hip_ctx.last_path() == path
        hip_ctx.debug_poison()
    # per-frame cells: every frame decides with its own step vectors
    cells = np.stack([cell, cell * 1.3, cell * 0.8])
    _both(hip_ctx, field, cells, PBC, (0.0,), access=True)


def test_a_brick_list_too_short_sends_the_frame_to_the_exact_path(hip_ctx):
    """AMOF_PORE_COVER_SRC_CAP=4: a destination brick that keeps more than four source bricks raises the flag, the frame's
    results are discarded and the frame, its accessible passes included, runs on pore_cover_exact; a frame whose bricks
    keep four at most (one small centre: itself and its images across two faces) stays on the brick path"""
    names = ["helix", "boxes"]
    field = np.concatenate([acases.case(n).field for n in names])
    grid = field.shape[1:]
    cell = np.diag([grid[0] * 0.9, grid[1] * 0.8, grid[2] * 0.7])
    want = _both(hip_ctx, field, cell, PBC, (0.0,), access=True)
    with _env(AMOF_PORE_COVER_SRC_CAP="4"):
        got = hip_ctx.pore_psd_field(field, cell, PBC, DR, DMAX, (0.0,), accessibility=True, per_point=True)
        assert hip_ctx.last_path() == EXACT
        assert hip_ctx.pore_cover_stats()["bricks"] == 0.0              # no frame's full pass stood on the brick path
    assert _same(got, want)
    lone = _single((16, 16, 16), (3, 3, 3), 0.4)                        # one centre that reaches no other brick
    with _env(AMOF_PORE_COVER_SRC_CAP="4"):
        got = hip_ctx.pore_psd_field(lone, CUBE, PBC, DR, DMAX, (0.0,), per_point=True)
        assert hip_ctx.last_path() == BRICK and hip_ctx.pore_cover_stats()["bricks"] == 8.0
    assert np.array_equal(got[3], restated_rows(lone, CUBE, PBC, DR, DMAX, (0.0,), False)[3])


# ---- 2. atoms ---------------------------------------------------------------------------------------------------------------
# (what the test below printed when run against the library of the commit before the stage pipeline: the full call, and the
# labelling-only call whose count holds both rounds)
RESTART_REPORT = ("pore_cover_brick", 9, {"bricks": 36.0, "source_bricks": 1118.0, "records": 26334.0})
RESTART_LABELLINGS = ("pore_label_tile", 90)


def test_the_field_tiers_start_over_with_stages_attached(hip_ctx):
    """an atom 2 x 10^4 cells away (the cell sort calls 10^4 too far and raises its flag): pore_brick runs every batch, the
    labelling and the covering behind each, and is abandoned; pore_exact hands every frame to the stages once more.  Every
    output is the one of the call that starts on pore_exact, and so is what the call reports: the covering stage's counters
    start over with the tiers."""
    from amof_amd.frames import PackedTrajectory
    c = pore_cases.case("rect")
    pos = np.array(c.packed.pos[:3], dtype=np.float64)
    pos[1, 0, 0] += 2.0e4 * c.packed.cell.reshape(-1, 3, 3)[0, 0, 0]
    far = PackedTrajectory(pos, c.packed.cell, c.packed.numbers)
    args = (c.radii, c.grid, c.dr, c.dmax, THRESHOLDS)
    kw = dict(per_point=True, accessibility=True, free_sphere=True, labels=True)
    hip_ctx.pore_field(far, *args)
    assert hip_ctx.last_path() == "pore_exact"                  # (pore_brick gave up on this input, through its own flag)
    hip_ctx.pore_field(c.packed, *args)
    assert hip_ctx.last_path() == "pore_brick"
    seen = {}
    for env in ({}, {"AMOF_PORE_EXACT": "1"}):
        with _env(AMOF_PORE_BATCH="1", **env):
            got = hip_ctx.pore_psd(far, *args, **kw)
            seen[len(env)] = (got, hip_ctx.last_path(), hip_ctx.last_kernel_launches(), hip_ctx.pore_cover_stats())
    assert len(seen[0][0]) == 12 and _same(seen[0][0], seen[1][0])
    assert seen[0][1:] == seen[1][1:]
    assert seen[0][1:] == RESTART_REPORT
    # the labelling stage alone: its count of labellings goes on across the restart, both rounds are in it
    count = {}
    for env in ({}, {"AMOF_PORE_EXACT": "1"}):
        with _env(AMOF_PORE_BATCH="1", **env):
            got = hip_ctx.pore_access(far, *args, free_sphere=True)
            count[len(env)] = (hip_ctx.last_path(), hip_ctx.last_kernel_launches())
        assert _same(got, seen[0][0][:6])
    assert count[0] == ("pore_label_tile", 2 * count[1][1]) and count[0] == RESTART_LABELLINGS, count


@pytest.mark.parametrize("name", ["rect", "zif4", "sheared", "npt_sheared", "open", "planted"])
def test_atoms_every_path_batching_residence_and_frame_range(hip_ctx, name):
    c = pore_cases.case(name)
    packed = c.packed
    F = packed.pos.shape[0]
    pbc = tuple(bool(x) for x in packed.pbc)
    args = (c.radii, c.grid, c.dr, c.dmax, THRESHOLDS)
    full = dict(per_point=True, accessibility=True, free_sphere=True, labels=True)
    lean = dict(per_point=True, accessibility=True)
    access = hip_ctx.pore_access(packed, *args, per_point=True, free_sphere=True, labels=True)
    field = access[6]
    want = restated_rows(field, packed.cell, pbc, c.dr, c.dmax, THRESHOLDS, True)
    # the labelling's own answers on this field, shared with tests/test_gpu_pore_access.py
    rows, _, _ = _restated(name, field.tobytes(), field.shape, c.dmax)

    def run(inp, env, path, kw, **more):
        with _env(**env):
            got = hip_ctx.pore_psd(inp, *args, **kw, **more)
            assert hip_ctx.last_path() == path, (env, hip_ctx.last_path())
        return got

    results = {}
    for cover_env, path in PATHS:
        got = run(packed, cover_env, path, full)
        # amof_pore_access's outputs, bit for bit, then w and its integers as the restatement has them on the library's field
        assert _same(got[:8], access), (name, path)
        assert np.array_equal(got[4], rows)
        psd_hist, po, acc, w = got[8:]
        assert np.array_equal(w, want[3]), (name, path, np.argwhere(w != want[3])[:5].tolist())
        assert _same((psd_hist, po, acc), want[:3]), (name, path, po.tolist(), want[1].tolist(), acc.tolist(), want[2].tolist())
        assert (psd_hist.sum(axis=1) == c.G).all() and (po >= got[1]).all() and (acc <= po).all()
        assert (acc >= got[4][:, :, 0]).all()                   # a channel's points cover themselves
        results[path] = first = run(packed, cover_env, path, lean)
        assert _same(first, got[:5] + (got[6],) + got[8:])
        hip_ctx.debug_poison()
        for env in ({"AMOF_PORE_BATCH": "1"}, {"AMOF_PORE_EXACT": "1"}, {"AMOF_PORE_LABEL_GLOBAL": "1"}):
            assert _same(run(packed, dict(cover_env, **env), path, lean), first), (name, path, env)
        assert _same(run(_device(packed), cover_env, path, lean), first)
        # without accessibility the field tier alone runs underneath
        bare = run(packed, cover_env, path, dict(per_point=True))
        assert _same(bare, got[:4] + (got[6], psd_hist, po, w))
        assert _same(run(packed, cover_env, path, {}), got[:4] + (psd_hist, po))
        if F > 1:
            h = F // 2
            a, b = run(packed, cover_env, path, lean, frame_range=(0, h)), run(packed, cover_env, path, lean, frame_range=(h, F))
            assert _same([np.concatenate([x, y]) for x, y in zip(a, b)], first)
            multi = _hip.MultiContext([0, 0])
            try:
                with _env(**cover_env):
                    assert _same(multi.pore_psd(packed, *args, **lean), first)
            finally:
                multi.close()
    assert _same(results[BRICK], results[EXACT])


# ---- 3. the class -----------------------------------------------------------------------------------------------------------
def test_class_on_rattled_zif4(hip_ctx):
    c = pore_cases.case("zif4")
    packed = c.packed
    kw = dict(probe_radius=(0.0, 1.2), spacing=0.5, dr=0.2, dmax=4.0, distributed=False, device=hip_ctx.device)
    plain = P.Pore.from_trajectory(packed, **kw)
    off = P.Pore.from_trajectory(packed, psd=False, **kw)
    base = ["Step", "Unitcell_volume", "Density", "PCV_Volume_fraction-0", "PCV_A^3-0", "PCV_cm^3/g-0",
            "PCV_Volume_fraction-1.2", "PCV_A^3-1.2", "PCV_cm^3/g-1.2", "Di"]
    assert list(off.data.columns) == base and off.data.equals(plain.data) and not hasattr(off, "psd") and not hasattr(off, "po_counts")
    acc = P.Pore.from_trajectory(packed, accessibility=True, per_point=True, **kw)
    obj = P.Pore.from_trajectory(packed, psd=True, accessibility=True, per_point=True, **kw)
    with _env(AMOF_ASYNC="0"):
        sync = P.Pore.from_trajectory(packed, psd=True, accessibility=True, per_point=True, **kw)
    assert obj.data.equals(sync.data) and obj.psd.equals(sync.psd) and np.array_equal(obj.cover, sync.cover)
    before = list(acc.data.columns)
    assert obj.data[before].equals(acc.data) and np.array_equal(obj.field, acc.field) and np.array_equal(obj.labels, acc.labels)
    pbc = tuple(bool(x) for x in packed.pbc)
    hist, po, pa, w = restated_rows(obj.field, packed.cell, pbc, 0.2, 4.0, (0.0, 1.2), True)
    assert np.array_equal(obj.cover, w) and np.array_equal(obj.psd_counts, hist)
    assert np.array_equal(obj.po_counts, po) and np.array_equal(obj.po_access, pa)
    mass = float(np.asarray(packed.masses, dtype=np.float64).sum())
    cols, dist = P.psd_columns(hist, po, pa, plain.data["Unitcell_volume"].to_numpy(), mass, [0.0, 1.2], obj.grid, 0.2)
    assert list(obj.data.columns) == before + list(cols) and obj.psd.equals(dist)
    for name, col in cols.items():
        assert np.array_equal(obj.data[name].to_numpy(), col), name
    assert (obj.data["POV_Volume_fraction-1.2"] >= obj.data["PCV_Volume_fraction-1.2"]).all()
    assert (np.diff(obj.psd["cumulative"].to_numpy()) <= 0).all()
    bare = P.Pore.from_trajectory(packed, psd=True, **kw)
    assert list(bare.data.columns) == base + [x for x in cols if x.startswith("POV_")] and not hasattr(bare, "cover")
    assert np.array_equal(bare.po_counts, po) and bare.psd.equals(dist)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_leave_zeros_and_the_context_usable(hip_ctx):
    lib, h, ptr = hip_ctx._lib, hip_ctx._h, _hip._ptr
    n = (16, 16, 16)
    grid, per, thr = _hip._i32(n), _hip._i32([1, 1, 1]), np.array([0.0, 1.0])
    cells = np.ascontiguousarray(CUBE.reshape(1, 9))

    def outputs():
        return (np.full((1, 18), 7, dtype=np.uint64), np.full((1, 2), 7, dtype=np.int64), np.full((1, 2), 7, dtype=np.int64),
                np.full((1, 16 ** 3), 7.0))

    # a value above half a periodic height (4 A): its sphere would reach a point through two images
    field = _single(n, (8, 8, 8), 4.5)
    hist, po, acc, w = outputs()
    rc = lib.amof_pore_psd_field(h, ptr(field), ptr(cells), 1, ptr(grid), ptr(per), 0.25, 4.0, ptr(thr), 2, 1, ptr(hist), ptr(po), ptr(acc),
                                 ptr(w))
    assert rc == _hip.AMOF_EINVAL and not hist.any() and not po.any() and not acc.any() and not w.any()
    with pytest.raises(ValueError, match="half the smallest periodic cell height"):
        hip_ctx.pore_psd_field(field, CUBE, PBC, 0.25, 4.0, thr)
    # ... along an open axis there is no such limit
    open_x = np.diag([8.0, 20.0, 20.0])
    hip_ctx.pore_psd_field(_single(n, (8, 8, 8), 4.5), open_x, (False, True, True), 0.25, 4.0, thr)
    # half a height exactly passes
    hip_ctx.pore_psd_field(_single(n, (8, 8, 8), 4.0), CUBE, PBC, 0.25, 4.0, thr)
    # want_access without a po_access array
    field = _single(n, (8, 8, 8), 2.5)
    hist, po, acc, w = outputs()
    rc = lib.amof_pore_psd_field(h, ptr(field), ptr(cells), 1, ptr(grid), ptr(per), 0.25, 4.0, ptr(thr), 2, 1, ptr(hist), ptr(po), None, ptr(w))
    assert rc == _hip.AMOF_EINVAL and not hist.any() and not po.any() and not w.any()
    with pytest.raises(ValueError, match="po_access"):
        hip_ctx._check(rc)
    c = pore_cases.case("rect")
    th = hip_ctx._traj(c.packed)
    F, G, nb = th.n_frames, c.G, c.nbins
    grid3, thr3, radii = _hip._i32(c.grid), np.array(THRESHOLDS), np.ascontiguousarray(c.radii, dtype=np.float64)
    hist, counts = np.full((F, nb + 2), 7, dtype=np.uint64), np.full((F, 3), 7, dtype=np.int64)
    vmax, argmax, access = np.full(F, 7.0), np.full(F, 7, dtype=np.int64), np.full((F, 3, 4), 7, dtype=np.int64)
    psd_hist, po = np.full((F, nb + 2), 7, dtype=np.uint64), np.full((F, 3), 7, dtype=np.int64)
    import ctypes
    rc = lib.amof_pore_psd(h, ctypes.byref(th.c), ptr(radii), ptr(grid3), c.dr, c.dmax, ptr(thr3), 3, 1, 0, ptr(hist), ptr(counts), ptr(vmax),
                           ptr(argmax), ptr(access), None, None, None, ptr(psd_hist), ptr(po), None, None)
    assert rc == _hip.AMOF_EINVAL
    for a in (hist, counts, vmax, argmax, access, psd_hist, po):
        assert not a.any()
    # every array given, refused after the sizes are known (dmax + R = 7.39 above half the smallest height, 7.15): zeros in all twelve
    far = 6.0
    nb6 = int(np.rint(far / c.dr))
    a = dict(hist=np.full((F, nb6 + 2), 7, dtype=np.uint64), counts=np.full((F, 3), 7, dtype=np.int64), vmax=np.full(F, 7.0),
             argmax=np.full(F, 7, dtype=np.int64), access=np.full((F, 3, 4), 7, dtype=np.int64), free=np.full((F, 2), 7.0),
             field=np.full((F, G), 7.0), labels=np.full((F, 3, G), 7, dtype=np.int32), psd_hist=np.full((F, nb6 + 2), 7, dtype=np.uint64),
             po=np.full((F, 3), 7, dtype=np.int64), po_access=np.full((F, 3), 7, dtype=np.int64), cover=np.full((F, G), 7.0))
    rc = lib.amof_pore_psd(h, ctypes.byref(th.c), ptr(radii), ptr(grid3), c.dr, far, ptr(thr3), 3, 1, 1, *[ptr(v) for v in a.values()])
    assert rc == _hip.AMOF_EINVAL
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx._check(rc)
    assert _unzeroed(a) == []
    # ... and a valid call follows: the restatement's integers on the library's field
    got = hip_ctx.pore_psd(c.packed, c.radii, c.grid, c.dr, c.dmax, THRESHOLDS, per_point=True)
    want = restated_rows(got[4], c.packed.cell, (True, True, True), c.dr, c.dmax, THRESHOLDS, False)
    assert _same(got[5:7], want[:2]) and np.array_equal(got[7], want[3])
    # accessibility needs three points on a periodic axis, as the labelling does
    with pytest.raises(ValueError, match="periodic axis"):
        hip_ctx.pore_psd_field(np.ones((1, 2, 5, 5)), np.diag([4.0, 10.0, 10.0]), PBC, 0.25, 4.0, thr, accessibility=True)
    with pytest.raises(ValueError):
        hip_ctx.pore_psd_field(np.full((1, 4, 4, 4), np.nan), CUBE, PBC, 0.25, 4.0, thr)
    with pytest.raises(_hip.AmofError):
        hip_ctx.pore_psd_field(np.ones((1, 4, 4, 4)), np.zeros((3, 3)), PBC, 0.25, 4.0, thr)       # a singular cell
    # the context goes on
    _, po, _, w = _both(hip_ctx, _single(n, (8, 8, 8), 2.5), CUBE)
    assert po[0, 0] == 515
