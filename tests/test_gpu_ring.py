"""Primitive ring statistics on the GPU (amof_ring_stats, Ring): per_atom, counts and truncated equal tests/ring_ref.py on every
case of tests/ring_cases.py, bit-identical between the wave kernel and the thread-per-source kernel, host and device-resident
input, one frame per batch and two frame ranges; last_path() asserted per run.  The bond graph is tied to amof_cn_count."""

import ctypes
import os
import sys

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import atom as amatom
from tests import helpers as H
from tests import ring_cases as cases
from tests import ring_ref as ref
from tests.conftest import ROOT
from tests.test_gpu_bond import _device, _env

pytestmark = pytest.mark.gpu

SIMPLE = {"AMOF_RING_SIMPLE": "1"}
ONE_FRAME = {"AMOF_RING_TABLE_MB": "0"}
RUNS = [({}, "ring_wave"), (SIMPLE, "ring_simple"), (ONE_FRAME, "ring_wave"), (dict(SIMPLE, **ONE_FRAME), "ring_simple")]


def _rcm(packed, cutoff):
    kinds, _ = H.species_of(packed.numbers)
    return amatom.cutoff_matrix(amatom.format_cutoff(cutoff, sort_pair=True), kinds)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _want(name):
    r = cases.reference(name)
    c = np.stack([x for x, _ in r])
    return np.stack([ref.counts(x) for x in c]), np.array([t for _, t in r], dtype=np.int64), c.astype(np.uint32)


def _neighbour_rows(name):
    nb = []
    for adj in cases.graphs(name):
        rows = np.full((len(adj), 17), -1, dtype=np.int32)
        for i, a in enumerate(adj):
            rows[i, 0] = len(a)
            rows[i, 1:1 + len(a)] = a
        nb.append(rows)
    return np.stack(nb)


@pytest.mark.parametrize("name", cases.NAMES)
def test_every_case_on_both_paths(hip_ctx, name):
    c = cases.case(name)
    packed, rcm = c.packed, _rcm(c.packed, c.cutoff)
    want = _want(name) + (_neighbour_rows(name),)
    F = packed.n_frames
    for env, path in RUNS:
        for inp in (packed, _device(packed)):
            with _env(**env):
                got = hip_ctx.ring_stats(inp, rcm, c.nmax, per_atom=True, neighbours=True)
                ran = hip_ctx.last_path()
            assert ran == path, (name, env, ran)
            assert got[0].shape == (F, 4, c.nmax + 1) and got[0].dtype == np.int64 and got[2].dtype == np.uint32
            for k, what in enumerate(("counts", "truncated", "per_atom", "neighbours")):
                assert np.array_equal(got[k], want[k]), (name, env, what)
            if c.known is not None:
                assert ref.rings(got[2][0]) == c.known
            with _env(**env):
                assert _same(hip_ctx.ring_stats(inp, rcm, c.nmax), want[:2])
    stats = hip_ctx.ring_search_stats()
    assert stats["sources"] == F * packed.n_atoms and stats["candidates"] >= stats["closed"] and (stats["closed"] > 0) == (want[0][:, 0].sum() > 0)
    stages = hip_ctx.last_stage_seconds()
    assert stages["rho"] >= 0 and stages["corr"] >= 0 and stages["self"] >= 0       # adjacency, BFS, search
    if F > 1:
        # two frame ranges concatenate; scratch left by one call means nothing to the next
        a = hip_ctx.ring_stats(packed, rcm, c.nmax, frame_range=(0, 1), per_atom=True, neighbours=True)
        hip_ctx.debug_poison(0xA5)
        with _env(**SIMPLE):
            b = hip_ctx.ring_stats(_device(packed), rcm, c.nmax, frame_range=(1, F), per_atom=True, neighbours=True)
        assert _same([np.concatenate([x, y]) for x, y in zip(a, b)], want)
        multi = _hip.MultiContext([0, 0])
        try:
            assert _same(multi.ring_stats(packed, rcm, c.nmax, per_atom=True, neighbours=True), want)
        finally:
            multi.close()


@pytest.mark.parametrize("name", ["zif4_16", "random_tri", "random_rect"])
def test_degrees_are_the_coordination_numbers(hip_ctx, name):
    c = cases.case(name)
    packed, rcm = c.packed, _rcm(c.packed, c.cutoff)
    S = rcm.shape[0]
    sets = [(a, b) for a in range(S) for b in range(S) if rcm[a, b] > 0]
    _, cn = hip_ctx.cn_count(packed, rcm, sets, per_atom=True)                  # [F][n_sets][N], -1: not a centre of the set
    nb = hip_ctx.ring_stats(packed, rcm, c.nmax, neighbours=True)[2]
    assert np.array_equal(nb[:, :, 0], np.maximum(cn, 0).sum(axis=1)) and nb[:, :, 0].sum() > 0
    rows = nb[:, :, 1:]
    assert np.all((rows >= 0).sum(axis=2) == nb[:, :, 0])
    assert np.all((np.diff(rows, axis=2) > 0) | (rows[:, :, 1:] < 0))         # ascending, then -1


@pytest.mark.parametrize("name", ["zif4_16", "random_rect", "graphene"])
def test_counts_do_not_depend_on_the_depth(hip_ctx, name):
    c = cases.case(name)
    rcm = _rcm(c.packed, c.cutoff)
    for env in ({}, SIMPLE):
        with _env(**env):
            small = hip_ctx.ring_stats(c.packed, rcm, 8, per_atom=True)
            large = hip_ctx.ring_stats(c.packed, rcm, 12, per_atom=True)
        assert np.array_equal(small[2], large[2][:, :, :9])
        assert np.array_equal(small[0][:, :2], large[0][:, :2, :9])           # (smallest / largest ring of an atom may move up)
    assert small[0][:, 0].sum() > 0


def test_capacity_refusals_leave_zeros_and_a_usable_context(hip_ctx):
    from tests import bond_order_cases
    good = cases.case("sc7")
    rcm7 = _rcm(good.packed, good.cutoff)
    want = _want("sc7")
    # a Zn with 17 N around it (16 pass)
    over, fits = bond_order_cases.cluster(counts=(17, 3), seed=6), bond_order_cases.cluster(counts=(16, 3), seed=6)
    cut = {'Zn-N': 3.0}
    for env in ({}, SIMPLE):
        with _env(**env):
            with pytest.raises(_hip.AmofError, match="frame 0: an atom has more than RING_MAX_DEGREE = 16 neighbours") as err:
                hip_ctx.ring_stats(over, _rcm(over, cut), 8)
            assert err.value.code == _hip.AMOF_ECAPACITY
            nb = hip_ctx.ring_stats(fits, _rcm(fits, cut), 8, neighbours=True)[2]
            assert nb[0, :, 0].max() == 16
            # more than 4 shortest paths: the antipodes at (1, 1, 1) have six
            with _env(AMOF_RING_MAX_PATHS="4"):
                with pytest.raises(_hip.AmofError, match="frame 0: more than RING_MAX_PATHS = 4 shortest paths") as err:
                    hip_ctx.ring_stats(good.packed, rcm7, 6)
                assert err.value.code == _hip.AMOF_ECAPACITY
            with _env(AMOF_RING_MAX_PATHS="5"):
                with pytest.raises(_hip.AmofError):
                    hip_ctx.ring_stats(good.packed, rcm7, 6)
            with _env(AMOF_RING_MAX_PATHS="6"):
                assert _same(hip_ctx.ring_stats(good.packed, rcm7, 6, per_atom=True), want)
            assert _same(hip_ctx.ring_stats(good.packed, rcm7, 6, per_atom=True), want)     # the context works afterwards
    # through the C ABI: the caller's arrays hold zeros after the refusal
    th = hip_ctx._traj(over)
    rcm = np.ascontiguousarray(_rcm(over, cut), dtype=np.float64)
    counts = np.full((1, 4, 9), 9, dtype=np.int64)
    truncated = np.full(1, 9, dtype=np.int64)
    pa = np.full((1, over.n_atoms, 9), 9, dtype=np.uint32)
    nb = np.full((1, over.n_atoms, 17), 9, dtype=np.int32)
    hip_ctx.drain()
    with hip_ctx._lock:
        rc = hip_ctx._lib.amof_ring_stats(hip_ctx._h, ctypes.byref(th.c), ctypes.c_void_p(rcm.ctypes.data), 8,
                                          ctypes.c_void_p(counts.ctypes.data), ctypes.c_void_p(truncated.ctypes.data),
                                          ctypes.c_void_p(pa.ctypes.data), ctypes.c_void_p(nb.ctypes.data))
    assert rc == _hip.AMOF_ECAPACITY and not counts.any() and not truncated.any() and not pa.any() and not nb.any()


def test_arguments(hip_ctx):
    c = cases.case("graphene")
    rcm = _rcm(c.packed, c.cutoff)
    for bad in (2, 33, 0):
        with pytest.raises(ValueError, match="max_size"):
            hip_ctx.ring_stats(c.packed, rcm, bad)
    with pytest.raises(ValueError, match="half the smallest cell height"):
        hip_ctx.ring_stats(c.packed, rcm * 5.0, 8)          # 8 A > 14.76 / 2
    two = cases.case("random_rect")
    m = _rcm(two.packed, two.cutoff)
    skew = m.copy()
    skew[0, 1] += 0.1
    with pytest.raises(ValueError, match="symmetric"):
        hip_ctx.ring_stats(two.packed, skew, 8)
    with pytest.raises(ValueError, match="finite and >= 0"):
        hip_ctx.ring_stats(two.packed, -m, 8)
    empty = hip_ctx.ring_stats(c.packed, rcm, 8, frame_range=(0, 0), per_atom=True)
    assert empty[0].shape == (0, 4, 9) and empty[2].shape == (0, 96, 9)
    none = hip_ctx.ring_stats(c.packed, rcm * 0.0, 8)       # no bonds: no rings, nothing truncated
    assert not none[0].any() and not none[1].any()


def _walk():
    return cases.zif4(reps=(2, 1, 1), F=4, sigma=0.02, seed=5)


def test_class_equals_the_library_call(hip_ctx, tmp_path, monkeypatch):
    from amof_amd.ring import Ring, assemble
    tr = _walk()
    F, N = len(tr), tr.n_atoms
    rcm = _rcm(tr, cases.ZIF_CUT)
    counts, truncated, pa = hip_ctx.ring_stats(tr, rcm, 32, per_atom=True)
    assert counts[:, 0, 5].tolist() == [5 * 64] * F                 # the imidazolate rings survive the rattle
    monkeypatch.setenv("AMOF_ASYNC", "1")
    obj = Ring.from_trajectory(tr, cases.ZIF_CUT, delta_Step=5, first_frame=10, per_atom=True, device=0, distributed=False)
    table = obj.table
    assert obj.__dict__.get("_pending") is None
    want_table, want_mean, want_report = assemble(counts, truncated, N, np.arange(10, 10 + 5 * F, 5), 32)
    assert table.equals(want_table) and obj.mean.equals(want_mean) and obj.report_search.equals(want_report)
    assert np.array_equal(obj.counts, counts) and np.array_equal(obj.truncated, truncated) and np.array_equal(obj.per_atom, pa)
    assert table["Step"].unique().tolist() == list(range(10, 10 + 5 * F, 5)) and table["ring_size"].unique().tolist() == list(range(3, 33))
    first = table[table["Step"] == 10]
    assert {int(n): int(r) for n, r in zip(first["ring_size"], first["rings"]) if r}.keys() >= {5, 16}
    try:
        import xarray  # noqa: F401
        assert obj.data is not None
    except ImportError:
        assert obj.data is None
        with pytest.raises(ImportError):
            obj.write_to_file(str(tmp_path / "rings"))
    # the single frame of the fixture at the default depth: the README's answer
    one = Ring.from_trajectory(cases.zif4(), cases.ZIF_CUT, device=0, distributed=False).table
    assert {int(n): int(r) for n, r in zip(one["ring_size"], one["rings"]) if r} == {5: 32, 16: 24, 24: 32, 32: 24}
    # synchronous, device-resident, the device list and a streamed source give the same
    monkeypatch.setenv("AMOF_ASYNC", "0")
    for inp, dev in ((_device(tr), 0), (tr, [0, 0])):
        again = Ring.from_trajectory(inp, cases.ZIF_CUT, delta_Step=5, first_frame=10, parallel=True, device=dev, distributed=False)
        assert again.table.equals(table) and np.array_equal(again.counts, counts)
    from amof_amd import trajectory as T
    from amof_amd.stream import XyzStream
    xyz = str(tmp_path / "walk.xyz")
    T.write_xyz(xyz, tr, comment_lattice=False, fmt="%.17g")
    streamed = Ring.from_trajectory(XyzStream(xyz, cell=tr.cell[0], batch_frames=3), cases.ZIF_CUT, delta_Step=5, first_frame=10,
                                    device=0, distributed=False)
    assert np.array_equal(streamed.counts, counts) and np.array_equal(streamed.truncated, truncated)
    with pytest.raises(ValueError):
        Ring.from_trajectory(tr, {'Zn-N': 9.0}, device=0, distributed=False).table


def _run(packed, distributed):
    from amof_amd.ring import Ring
    obj = Ring.from_trajectory(packed, cases.ZIF_CUT, max_search_depth=16, per_atom=True, device=0, distributed=distributed)
    return obj.table, [np.asarray(obj.counts), np.asarray(obj.truncated), np.asarray(obj.per_atom)]


def _save(out_dir, tag, table, arrays):
    table.to_pickle(os.path.join(out_dir, "ring_%s.pkl" % tag))
    np.savez(os.path.join(out_dir, "ring_%s.npz" % tag), *arrays)


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    import torch.distributed as dist
    dist.init_process_group("gloo", rank=rank, world_size=world)
    _save(out_dir, "rank%d" % rank, *_run(_walk(), None))       # None: shard the frames over the group
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
    _save(out_dir, "rccl", *_run(_walk(), None))
    dist.barrier()
    dist.destroy_process_group()


def _equal_to_single_process(out_dir, tags):
    import pandas as pd
    table, arrays = _run(_walk(), False)
    assert arrays[0][:, 0].sum() > 0
    for tag in tags:
        assert pd.read_pickle(os.path.join(out_dir, "ring_%s.pkl" % tag)).equals(table)
        got = np.load(os.path.join(out_dir, "ring_%s.npz" % tag))
        for k, want in enumerate(arrays):
            assert np.array_equal(got["arr_%d" % k], want), (tag, k)


def test_two_ranks_equal_single_process(tmp_path):
    # the frames sharded over two ranks (gloo rendezvous; both on cuda:0 where the box has one GPU, as tests/test_gpu_bond_order.py)
    import torch.multiprocessing as mp
    port = 45600 + os.getpid() % 2000
    mp.spawn(_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    _equal_to_single_process(str(tmp_path), ("rank0", "rank1"))


def test_rccl_backend_single_rank(tmp_path):
    # the rows gathered by tensor collectives over RCCL
    import torch.multiprocessing as mp
    port = 47600 + os.getpid() % 2000
    mp.spawn(_worker_rccl, args=(1, port, str(tmp_path)), nprocs=1, join=True)
    _equal_to_single_process(str(tmp_path), ("rccl",))
