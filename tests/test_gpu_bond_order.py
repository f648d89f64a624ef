"""Bond order parameters on the GPU (amof_bond_order[_dev], BondOrder): the neighbour counts bit-exact against amof_cn_count,
the fixed-point sums within the derived budget of tests/bond_order_ref.py and bit-identical between every forced path, the
histograms and frame sums exactly what numpy computes from the library's own per-atom integers; last_path() asserted per
run.  Inputs: tests/bond_order_cases.py."""

import ctypes
import os
import sys

import numpy as np
import pytest

from amof_amd import _hip
from tests import bond_order_cases as cases
from tests import bond_order_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_bond import _abi, _device, _env, _planted

pytestmark = pytest.mark.gpu

EXACT = {"AMOF_ORDER_EXACT": "1"}
ROWS = {"AMOF_ORDER_ROWS_MB": "1"}
ONE_FRAME = {"AMOF_ORDER_ROWS_MB": "0"}         # a frame per batch of neighbour rows
LANE_SUMS = {"AMOF_ORDER_SUMS": "lane"}         # the frame sums by per-lane atomics
NB, NT = cases.NBINS, cases.NBINS_TET
EDGES = np.arange(0, 182, 2.0)
L2 = (4, 6)


def _frame_tier_applies(hip_ctx, packed, rcm, sets):
    """the frame tier applies wherever BAD's does: ask BAD for the triples B-A-B of the sets"""
    triples = [(a, b) for a, b in sets if rcm[a, b] > 0]
    hip_ctx.bad_hist(packed, rcm, triples, EDGES)
    return hip_ctx.last_path() in ("bad_frame", "bad_frame_slabs")


def _tie_to_cn_and_bad(hip_ctx, packed, rcm, sets, sums, pa):
    """n is amof_cn_count's per-atom count, column 0 its sums, column 3 amof_bad_hist's n_angles of the triple B-A-B"""
    cn_sums, cn_pa = hip_ctx.cn_count(packed, rcm, sets, per_atom=True)
    assert np.array_equal(pa[..., 0], cn_pa.astype(np.int64))
    assert np.array_equal(sums[:, :, 0], cn_sums)
    _, nang = hip_ctx.bad_hist(packed, rcm, sets, EDGES)
    assert np.array_equal(sums[:, :, 3].sum(axis=0).astype(np.uint64), nang)


def _same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def _case(hip_ctx, name, runs, device=False, budget=True):
    """every forced path of ``runs`` on a case; returns (hist, hist_tet, frame_sums, per_atom) of the first"""
    c = cases.case(name)
    packed = c.packed
    rcm, sets = _abi(packed, c.sets)
    first = None
    for env, path in runs:
        for inp in ([packed, _device(packed)] if device else [packed]):
            with _env(**env):
                got = hip_ctx.bond_order(inp, rcm, sets, c.l, NB, NT, per_atom=True)
                ran = hip_ctx.last_path()
            assert ran == path, (name, env, ran, path)
            hist, hist_tet, sums, pa = got
            assert hist.shape == (len(sets), len(c.l), NB) and hist_tet.shape == (len(sets), NT)
            assert sums.shape == (packed.pos.shape[0], len(sets), 4 + len(c.l) + 1) and sums.dtype == np.int64
            if first is None:
                first = got
                _tie_to_cn_and_bad(hip_ctx, packed, rcm, sets, sums, pa)
                if budget:
                    worst = ref.check(pa, cases.reference(name))
                    print("%s %s: largest |difference| / budget = %.3g" % (name, path, worst))
                # bins and sums are exactly what the definition gives for the library's own per-atom integers
                assert _same(ref.from_per_atom(pa, len(c.l), NB, NT), (hist, hist_tet, sums))
                assert hist.sum(axis=2).tolist() == [[int(sums[:, s, 1].sum())] * len(c.l) for s in range(len(sets))]
                assert hist_tet.sum(axis=1).tolist() == sums[:, :, 2].sum(axis=0).tolist()
            assert _same(got, first), (name, env, path)
            assert _same(hip_ctx.bond_order(inp, rcm, sets, c.l, NB, NT)[:3], first[:3]) if env == {} else True
    return first


def test_rectangular_one_species_every_path(hip_ctx):
    # N = 150, F = 7: neither a multiple of 64 (ragged tiles); n spans 0 .. 12, 4 among them (asserted on the CPU)
    runs = [({}, "order_frame"), (EXACT, "order_exact"), (ROWS, "order_frame"), (ONE_FRAME, "order_frame"),
            (LANE_SUMS, "order_frame"), (dict(EXACT, **LANE_SUMS), "order_exact")]
    hist, hist_tet, sums, pa = _case(hip_ctx, "rect", runs, device=True)
    n = pa[:, 0, :, 0]
    assert n.min() == 0 and n.max() >= 12 and (n == 4).any()
    assert hist_tet.sum() == (n == 4).sum() > 0
    stages = hip_ctx.last_stage_seconds()
    assert stages["rho"] >= 0 and stages["corr"] >= 0           # list stage, order kernels


def test_rattled_zif4(hip_ctx):
    c = cases.case("zif4")
    rcm, sets = _abi(c.packed, c.sets)
    path = "order_frame" if _frame_tier_applies(hip_ctx, c.packed, rcm, sets) else "order_exact"
    hist, hist_tet, sums, pa = _case(hip_ctx, "zif4", [({}, path), (EXACT, "order_exact"), (ONE_FRAME, path)], device=True)
    is_n = c.packed.numbers == 7
    n_n = pa[:, 1][:, is_n][..., 0]
    assert set(np.unique(n_n).tolist()) <= {0, 1} and (n_n == 1).mean() > 0.9
    # every N with its one Zn has q_l = 1 exactly: the last, right-closed bin
    assert np.all(hist[1, :, -1] == (n_n == 1).sum()) and not hist[1, :, :-1].any() and not hist_tet[1].any()
    n_zn = pa[:, 0][:, c.packed.numbers == 30][..., 0]
    assert (n_zn == 4).mean() > 0.9
    four = sums[:, 0, 2].sum()
    assert sums[:, 0, -1].sum() * 2.0 ** -30 / four > 0.8         # mean q_tet of the rattled tetrahedra


def test_four_species_zero_cutoff_and_a_set_named_twice(hip_ctx):
    hist, hist_tet, sums, pa = _case(hip_ctx, "four", [({}, "order_frame"), (EXACT, "order_exact"), (ONE_FRAME, "order_frame")],
                                     device=True)
    assert np.array_equal(hist[0], hist[5]) and np.array_equal(sums[:, 0], sums[:, 5]) and np.array_equal(pa[:, 0], pa[:, 5])
    assert not hist[4].any() and not hist_tet[4].any() and not sums[:, 4].any()
    zn = cases.case("four").packed.numbers == 30
    assert np.all(pa[:, 4][:, zn] == 0) and np.all(pa[:, 4][:, ~zn][..., 0] == -1)
    assert sums[:, 0, 0].sum() == sums[:, 1, 0].sum() > 0                   # Zn-N and N-Zn: the same bonds


@pytest.mark.parametrize("name", ["sheared", "npt_diag", "npt_sheared", "open"])
def test_general_cells(hip_ctx, name):
    c = cases.case(name)
    rcm, sets = _abi(c.packed, c.sets)
    frame = _frame_tier_applies(hip_ctx, c.packed, rcm, sets)
    assert not (name == "open" and frame)
    runs = [({}, "order_frame" if frame else "order_exact"), (EXACT, "order_exact")]
    hist, hist_tet, sums, pa = _case(hip_ctx, name, runs, device=True)
    assert sums[:, :, 3].sum() > 0 and hist_tet.sum() > 0


@pytest.mark.parametrize("kind", ["sc", "fcc", "diamond"])
def test_perfect_lattices(hip_ctx, kind):
    packed, rc, n, shell = cases.lattice(kind)
    l = (3, 4, 6) if kind == "diamond" else (4, 6)
    want, _ = ref.shell(shell, l)
    rcm, sets = _abi(packed, [(30, 30, rc)])
    frame = _frame_tier_applies(hip_ctx, packed, rcm, sets)
    first = None
    for env, path in [({}, "order_frame" if frame else "order_exact"), (EXACT, "order_exact")]:
        with _env(**env):
            got = hip_ctx.bond_order(packed, rcm, sets, l, 100, 400, per_atom=True)
            assert hip_ctx.last_path() == path
        hist, hist_tet, sums, pa = got
        assert np.all(pa[:, 0, :, 0] == n)
        q, qt = ref.q_of(pa[:, 0, :, 0], pa[:, 0, :, 1:1 + len(l)], pa[:, 0, :, 1 + len(l)])
        assert np.all(np.abs(q - np.asarray(want)) < 1e-9), (kind, float(np.abs(q - np.asarray(want)).max()))
        assert _same(ref.from_per_atom(pa, len(l), 100, 400), (hist, hist_tet, sums))
        if kind == "diamond":
            assert np.all(np.abs(qt - 1.0) < 1e-9) and hist_tet[0, -1] == pa.shape[0] * pa.shape[2] and hist_tet.sum() == hist_tet[0, -1]
        else:
            assert not hist_tet.any()
        first = got if first is None else first
        assert _same(got, first)


def test_centres_with_17_to_64_neighbours_and_the_capacity(hip_ctx):
    hist, hist_tet, sums, pa = _case(hip_ctx, "cluster", [({}, "order_exact"), (EXACT, "order_exact")], device=True)
    zn = cases.case("cluster").packed.numbers == 30
    assert sorted(pa[0, 0][zn][:, 0].tolist()) == sorted(cases.CLUSTER_COUNTS)
    over = cases.cluster(counts=(65, 4), seed=6)
    rcm, sets = _abi(over, [(30, 7, 3.0)])
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.bond_order(over, rcm, sets, (4, 6), NB, NT)
    assert err.value.code == _hip.AMOF_ECAPACITY and hip_ctx.last_path() == "order_exact"
    # the context works afterwards
    assert _same(hip_ctx.bond_order(cases.case("cluster").packed, *_abi(cases.case("cluster").packed, [(30, 7, 3.0)]),
                                    (4, 6, 12), NB, NT), (hist, hist_tet, sums))


def test_no_set_with_a_live_pair_is_nothing_to_do(hip_ctx):
    """Two sets without a cutoff beside a species pair (N-N) that has one and that no set names: the list stage applies and finds
    nothing to do, no kernel of either tier runs (the path name stays the call's before), and the outputs are the exact
    kernel's and the restatement's -- no neighbour anywhere, zeros in the centres' rows, -1 off the centre species.
    2 frames of 64 atoms."""
    from tests import test_gpu_bond as B
    packed = B._walk(B.DIAG, B._numbers4(64), 2, 21)
    named = [(30, 30, 0.0), (1, 30, 0.0)]
    _, sets = _abi(packed, named)
    rcm, nn = _abi(packed, named + [(7, 7, 3.0)])
    hip_ctx.cn_count(packed, rcm, nn[2:])
    before = hip_ctx.last_path()
    assert before.startswith("cn_")
    got = hip_ctx.bond_order(packed, rcm, sets, L2, NB, NT, per_atom=True)
    assert hip_ctx.last_path() == before
    with _env(**EXACT):
        exact = hip_ctx.bond_order(packed, rcm, sets, L2, NB, NT, per_atom=True)
        assert hip_ctx.last_path() == "order_exact"
    assert _same(got, exact)
    ref.check(got[3], ref.order(packed.pos, packed.cell, packed.numbers, named, L2, pbc=tuple(packed.pbc)))
    assert _same(ref.from_per_atom(got[3], len(L2), NB, NT), got[:3])
    assert not got[0].any() and not got[1].any() and not got[2].any()
    zn, h = packed.numbers == 30, packed.numbers == 1
    assert zn.any() and h.any() and np.all(got[3][:, 0][:, zn] == 0) and np.all(got[3][:, 1][:, h] == 0)
    assert np.all(got[3][:, 0][:, ~zn][..., 0] == -1) and np.all(got[3][:, 1][:, ~h][..., 0] == -1)


def test_coincident_bonded_pair_is_an_error_and_leaves_zeros(hip_ctx):
    import torch
    p = cases.coincident()
    rcm, sets = _abi(p, [(30, 7, 3.4)])
    for env in ({}, EXACT):
        with _env(**env):
            with pytest.raises(ZeroDivisionError):
                hip_ctx.bond_order(p, rcm, sets, (4, 6), NB, NT, per_atom=True)
    # the host form through the C ABI: the caller's buffers hold zeros after the error
    th = hip_ctx._traj(p)
    rcm = np.ascontiguousarray(rcm, dtype=np.float64)
    sets_a = np.ascontiguousarray(sets, dtype=np.int32)
    l = np.array([4, 6], dtype=np.int32)
    hist = np.full((1, 2, NB), 9, dtype=np.uint64)
    hist_tet = np.full((1, NT), 9, dtype=np.uint64)
    sums = np.full((th.n_frames, 1, 7), 9, dtype=np.int64)
    hip_ctx.drain()
    with hip_ctx._lock:
        rc = hip_ctx._lib.amof_bond_order(hip_ctx._h, ctypes.byref(th.c), ctypes.c_void_p(rcm.ctypes.data),
                                          ctypes.c_void_p(sets_a.ctypes.data), 1, ctypes.c_void_p(l.ctypes.data), 2, NB, NT,
                                          ctypes.c_void_p(hist.ctypes.data), ctypes.c_void_p(hist_tet.ctypes.data),
                                          ctypes.c_void_p(sums.ctypes.data), None)
    assert rc == _hip.AMOF_EANGLE and not hist.any() and not hist_tet.any() and not sums.any()
    # the _dev form leaves its buffers untouched
    out = (torch.full((1, 2, NB), 5, dtype=torch.int64, device="cuda"), torch.full((1, NT), 5, dtype=torch.int64, device="cuda"))
    with pytest.raises(ZeroDivisionError):
        hip_ctx.bond_order(p, rcm, sets, (4, 6), NB, NT, out=out)
    assert int((out[0].cpu() != 5).sum()) == 0 and int((out[1].cpu() != 5).sum()) == 0
    # class level, as Bad
    from amof_amd.bond_order import BondOrder
    with pytest.raises(ZeroDivisionError):
        BondOrder.from_trajectory(p, {'Zn-N': 3.4}, device=0, distributed=False).data
    good = cases.case("four").packed                                # the context works afterwards
    assert hip_ctx.bond_order(good, rcm, sets, (4, 6), NB, NT)[2][:, 0, 0].sum() > 0


@pytest.mark.parametrize("where", [1, 2, 3])
def test_guard_band_pairs(hip_ctx, where):
    # pairs planted across the f32 guard band of rc (half of them thousands of cells away): n is amof_cn_count's on every path
    packed, pl = _planted(where, 40 + where)
    rcm, sets = _abi(packed, [(30, 7, 3.4), (7, 30, 3.4), (7, 7, 3.1), (30, 30, 2.9)])
    cn_sums, cn_pa = hip_ctx.cn_count(packed, rcm, sets, per_atom=True)
    frame = _frame_tier_applies(hip_ctx, packed, rcm, sets)
    path = "order_frame" if frame else "order_exact"
    first = None
    for env, want in [({}, path), (EXACT, "order_exact"), (ONE_FRAME, path)]:
        with _env(**env):
            got = hip_ctx.bond_order(packed, rcm, sets, (4, 6), NB, NT, per_atom=True)
            assert hip_ctx.last_path() == want
        assert np.array_equal(got[3][..., 0], cn_pa.astype(np.int64)), (where, env)
        assert np.array_equal(got[2][:, :, 0], cn_sums)
        first = got if first is None else first
        assert _same(got, first), (where, env)
    t = pl.band_units()
    assert int((t < -1e-3).sum()) >= 5 and int((t > 1e-3).sum()) >= 5 and int((np.abs(t) <= 1.0).sum()) >= 5


def test_frame_ranges_dev_form_poison_and_two_contexts(hip_ctx):
    import torch
    c = cases.case("rect")
    packed = c.packed
    rcm, sets = _abi(packed, c.sets)
    args = (rcm, sets, c.l, NB, NT)
    full = hip_ctx.bond_order(packed, *args, per_atom=True)
    assert hip_ctx.last_path() == "order_frame"
    a = hip_ctx.bond_order(packed, *args, frame_range=(0, 3), per_atom=True)
    b = hip_ctx.bond_order(_device(packed), *args, frame_range=(3, 7), per_atom=True)
    assert np.array_equal(a[0] + b[0], full[0]) and np.array_equal(a[1] + b[1], full[1])
    assert np.array_equal(np.concatenate([a[2], b[2]]), full[2]) and np.array_equal(np.concatenate([a[3], b[3]]), full[3])
    # the _dev form adds into pre-filled buffers; the rows stay host arrays
    out = (torch.full((1, len(c.l), NB), 7, dtype=torch.int64, device="cuda"), torch.full((1, NT), 7, dtype=torch.int64, device="cuda"))
    with _env(**EXACT):
        r1 = hip_ctx.bond_order(packed, *args, frame_range=(0, 3), out=out)
    r2 = hip_ctx.bond_order(packed, *args, frame_range=(3, 7), out=out)
    assert r1[0] is out[0] and np.array_equal(out[0].cpu().numpy().view(np.uint64), full[0] + np.uint64(7))
    assert np.array_equal(out[1].cpu().numpy().view(np.uint64), full[1] + np.uint64(7))
    assert np.array_equal(np.concatenate([r1[2], r2[2]]), full[2])
    # scratch left by one call means nothing to the next
    hip_ctx.debug_poison(0xA5)
    assert _same(hip_ctx.bond_order(packed, *args, per_atom=True), full)
    hip_ctx.debug_poison(0xA5)
    with _env(**EXACT):
        assert _same(hip_ctx.bond_order(packed, *args, per_atom=True), full)
    # two contexts of one device sharing the frames
    multi = _hip.MultiContext([0, 0])
    try:
        assert _same(multi.bond_order(packed, *args, per_atom=True), full)
        assert _same(multi.bond_order(packed, *args, frame_range=(3, 7)), b[:3])
    finally:
        multi.close()
    # arguments
    for bad in (dict(l=(0,)), dict(l=(13,)), dict(l=(1, 2, 3, 4, 5)), dict(nbins=0), dict(nbins_tet=0)):
        kw = dict(l=c.l, nbins=NB, nbins_tet=NT)
        kw.update(bad)
        with pytest.raises(ValueError):
            hip_ctx.bond_order(packed, rcm, sets, kw["l"], kw["nbins"], kw["nbins_tet"])
    big, _ = _abi(packed, [(30, 30, 8.7)])                            # > 17.31 / 2
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.bond_order(packed, big, sets, c.l, NB, NT)
    empty = hip_ctx.bond_order(packed, rcm, [], c.l, NB, NT)
    assert empty[0].shape == (0, len(c.l), NB) and empty[2].shape == (7, 0, 4 + len(c.l) + 1)


def test_class_data_hist_per_atom_stream_and_device_list(hip_ctx, tmp_path, monkeypatch):
    from amof_amd.bond_order import BondOrder
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    c = cases.case("class")
    tr = c.packed
    F = len(tr)
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = BondOrder.from_trajectory(tr, cases.CLASS_CUT, l=(4, 6), nbins=NB, nbins_tet=NT, delta_Step=5, first_frame=10,
                                    per_atom=True, device=0, distributed=False)
    data = obj.data
    assert obj.__dict__.get("_pending") is None and obj.sets == ['Zn-N', 'C-N']
    cols = [n + s for n in ("Zn-N", "C-N", "Zn-Au", "Au-Zn") for s in ("-q4", "-q6", "-qtet", "-f4")]
    assert list(data.columns) == ["Step"] + cols and data["Step"].tolist() == list(range(10, 10 + 5 * F, 5))
    rcm, sets = _abi(tr, c.sets)
    hist, hist_tet, sums, pa = hip_ctx.bond_order(tr, rcm, sets, (4, 6), NB, NT, per_atom=True)
    ref.check(pa, cases.reference("class"))
    assert np.array_equal(obj.counts, hist) and np.array_equal(obj.counts_tet, hist_tet) and np.array_equal(obj.frame_sums, sums)
    n_zn = int((tr.numbers == 30).sum())
    q, qt = ref.q_of(pa[:, 0, :, 0].clip(0), pa[:, 0, :, 1:3], pa[:, 0, :, 3])
    zn = tr.numbers == 30
    with np.errstate(invalid="ignore"):
        assert np.allclose(data["Zn-N-q4"].values, np.nanmean(q[:, zn, 0], axis=1), rtol=0, atol=1e-8)
        assert np.allclose(data["Zn-N-qtet"].values, np.nanmean(qt[:, zn], axis=1), rtol=0, atol=1e-8)
    assert np.array_equal(data["Zn-N-f4"].values, sums[:, 0, 2] / n_zn) and data["Zn-N-qtet"].mean() > 0.8
    assert np.isnan(data["Zn-Au-q4"]).all() and data["Zn-Au-f4"].tolist() == [0.0] * F and np.isnan(data["Au-Zn-f4"]).all()
    assert np.sum(obj.hist["Zn-N-q6"].values) / NB == pytest.approx(1.0, abs=1e-12)
    assert np.sum(obj.hist_tet["Zn-N-qtet"].values) * 4.0 / NT == pytest.approx(1.0, abs=1e-12)
    assert np.array_equal(obj.coordination["Zn-N"], pa[:, 0][:, zn][..., 0]) and obj.per_atom["Zn-N"].shape == (F, n_zn, 3)
    assert np.array_equal(obj.per_atom["Zn-N"][..., :2], q[:, zn], equal_nan=True)
    assert np.array_equal(obj.per_atom["Zn-N"][..., 2], qt[:, zn], equal_nan=True)
    assert np.isnan(obj.per_atom["Zn-Au"]).all() and obj.per_atom["Zn-Au"].shape == (F, n_zn, 3) and not obj.coordination["Zn-Au"].any()
    assert obj.per_atom["Au-Zn"].shape == (F, 0, 3)
    path = str(tmp_path / "walk")
    obj.write_to_file(path)
    assert os.path.exists(path + ".order") and BondOrder.from_file(path).data.equals(data)
    # synchronous, device-resident, the device list and a streamed source give the same
    monkeypatch.setenv("AMOF_ASYNC", "0")
    for inp, dev in ((_device(tr), 0), (tr, [0]), (tr, [0, 0])):
        again = BondOrder.from_trajectory(inp, cases.CLASS_CUT, l=(4, 6), nbins=NB, nbins_tet=NT, delta_Step=5, first_frame=10,
                                          device=dev, distributed=False)
        assert again.data.equals(data) and np.array_equal(again.counts, hist) and np.array_equal(again.counts_tet, hist_tet)
    xyz = str(tmp_path / "walk.xyz")
    T.write_xyz(xyz, tr, comment_lattice=False, fmt="%.17g")
    stream = XyzStream(xyz, cell=tr.cell[0], batch_frames=2)
    streamed = BondOrder.from_trajectory(stream, cases.CLASS_CUT, l=(4, 6), nbins=NB, nbins_tet=NT, device=0, distributed=False)
    assert np.array_equal(streamed.counts, hist) and np.array_equal(streamed.counts_tet, hist_tet)
    assert np.array_equal(streamed.frame_sums, sums)
    with pytest.raises(ValueError):
        BondOrder.from_trajectory(tr, {'Zn-N': 9.0}, device=0, distributed=False).data


def _run(packed, distributed):
    from amof_amd.bond_order import BondOrder
    obj = BondOrder.from_trajectory(packed, cases.CLASS_CUT, l=(4, 6), nbins=NB, nbins_tet=NT, per_atom=True, device=0,
                                    distributed=distributed)
    return obj.data, [np.asarray(obj.counts), np.asarray(obj.counts_tet), np.asarray(obj.frame_sums), obj.per_atom["Zn-N"],
                      obj.coordination["C-N"]]


def _save(out_dir, tag, data, arrays):
    data.to_pickle(os.path.join(out_dir, "order_%s.pkl" % tag))
    np.savez(os.path.join(out_dir, "order_%s.npz" % tag), *arrays)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _save(out_dir, "rank%d" % rank, *_run(cases.case("class").packed, None))     # None: shard the frames over the group
    dist.barrier()
    dist.destroy_process_group()


def _worker_rccl(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", AMOF_DIST_FORCE_MERGE="1")     # one rank, but every collective really runs
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    from amof_amd import dist as adist
    assert adist.merging(1) and adist.device_collectives()
    _save(out_dir, "rccl", *_run(cases.case("class").packed, None))
    dist.barrier()
    dist.destroy_process_group()


def _equal_to_single_process(out_dir, tags):
    import pandas as pd
    data, arrays = _run(cases.case("class").packed, False)
    assert arrays[2][:, 0, 2].sum() > 0
    for tag in tags:
        assert pd.read_pickle(os.path.join(out_dir, "order_%s.pkl" % tag)).equals(data)
        got = np.load(os.path.join(out_dir, "order_%s.npz" % tag))
        for k, want in enumerate(arrays):
            assert np.array_equal(got["arr_%d" % k], want, equal_nan=want.dtype.kind == "f"), (tag, k)


def test_two_ranks_equal_single_process(tmp_path):
    # the frames sharded over two ranks (gloo rendezvous; both on cuda:0 where the box has one GPU, as tests/test_gpu_bond.py):
    # the rows are gathered, the histograms all-reduced
    import torch.multiprocessing as mp
    port = 41600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    _equal_to_single_process(str(tmp_path), ("rank0", "rank1"))


def test_rccl_backend_single_rank(tmp_path):
    # the device branch of the class: amof_bond_order_dev into CUDA tensors, all-reduced in place, read back
    import torch.multiprocessing as mp
    port = 43600 + os.getpid() % 2000
    mp.spawn(_worker_rccl, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    _equal_to_single_process(str(tmp_path), ("rccl",))
