"""The atom-sharded WindowMsd with device collectives (amof_amd/msd.py compute_msd: msd_shard_begin, one all-reduce of the
[F][3] table, msd_shard_finish on the lane; msd_com + msd_window(com, out) where the fused form does not apply) THROUGH
THE CLASS, over RCCL with the one rank a single GPU allows, in the orders in which other analyses share its lane.

amof_msd_shard_finish must be the call after its begin on the lane's context (csrc/msd.hip; pinned through the C ABI by
tests/test_gpu_msd_fused.py::test_sharded_halves_add_up_to_the_whole): every order runs once plainly and once behind a lane
that is held back while the objects are built, which is when a first half called from the constructor's thread would
overtake the queued jobs.  A spy counts the entry points per run -- a run that took another branch proves nothing --
and every result is compared with the float64 restatement of the reference's loops (oracle.numpy_oracle, 1e-9) and with the
same class in a single process (1e-12).  All runs share ONE spawned child: the process group is started once."""
import json
import os
import sys
import threading

import numpy as np
import pytest
import torch.multiprocessing as mp

from amof_amd.frames import Frame, PackedTrajectory
from oracle import numpy_oracle as no
from tests import helpers as H
from tests.conftest import ROOT
from tests.test_gpu_msd_fused import _walk

pytestmark = pytest.mark.gpu

CELL = np.diag([9.0, 10.0, 11.0])
CUT = {'Zn-N': 2.5}
FUSED_PATH, FALLBACK = (1, 1, 0, 0), (1, 0, 1, 1)      # calls of (msd_shard_begin, msd_shard_finish, msd_com, msd_window)

# run -> (objects built in this order: (name, class, trajectory, delta_time), reading order, calls of the four entry points)
ORDERS = {
    # the reference example's order: two other analyses are queued on the lane before the MSD
    "bad_cn_msd": ([("bad", "Bad", "FUSED", None), ("cn", "Cn", "FUSED", None), ("msd", "Msd", "FUSED", 16)], [0, 1, 2], FUSED_PATH),
    # two pairs with different keys (windows 0, 16, .. 112 and 0, 32, 64, 96), read in both orders
    "msd_msd": ([("msd16", "Msd", "FUSED", 16), ("msd32", "Msd", "FUSED", 32)], [0, 1], (2, 2, 0, 0)),
    "msd_msd_read_backwards": ([("msd16", "Msd", "FUSED", 16), ("msd32", "Msd", "FUSED", 32)], [1, 0], (2, 2, 0, 0)),
    # the fallback's msd_com of the next object after a begin
    "msd_then_general": ([("msd", "Msd", "FUSED", 16), ("general", "Msd", "GENERAL", 16)], [0, 1], (2, 1, 1, 1)),
    "msd_then_vanhove": ([("msd", "Msd", "FUSED", 16), ("vanhove", "VanHove", "FUSED", 16)], [0, 1], (1, 1, 1, 0)),
    # the RDF's reader finishes the MSD first (_lazy.Deferred._finish_followers_first)
    "rdf_msd_rdf_read_first": ([("rdf", "Rdf", "FUSED", None), ("msd", "Msd", "FUSED", 16)], [0, 1], FUSED_PATH),
}
SINGLES = {
    "npt": ([("msd", "Msd", "NPT", 16)], [0], FUSED_PATH),
    "general": ([("msd", "Msd", "GENERAL", 16)], [0], FALLBACK),
    "short": ([("msd", "Msd", "FUSED", 1)], [0], FALLBACK),
    "gas": ([("msd", "Msd", "GAS", 32)], [0], FUSED_PATH),
    "sync": ([("msd", "Msd", "FUSED", 16)], [0], FUSED_PATH),          # AMOF_ASYNC=0
}
RUNS = dict(SINGLES)
for _name, _run in ORDERS.items():
    RUNS[_name] = _run
    RUNS[_name + "_gated"] = _run


def _host_trajectories():
    """the host trajectories of the cases, the same in the child and in the parent (GENERAL is generated in HBM by the
    child and handed over as a file)"""
    fused = _walk(256, 50, 256 * 131 + 16, CELL)
    rng = np.random.default_rng(3)
    cells = np.array([CELL * (1 + 0.004 * rng.normal()) for _ in range(256)])
    npt = _walk(256, 50, 11, CELL, cells=cells)
    rng = np.random.default_rng(8)
    gas = PackedTrajectory(rng.uniform(0, 1, (400, 30, 3)) @ CELL, CELL, [1, 8] * 15)
    return {"FUSED": fused, "NPT": npt, "GAS": gas}


def _general_base():
    """24 atoms in a sheared cell: the base frame of GENERAL"""
    cell = np.array([[9.0, 0.0, 0.0], [1.5, 10.0, 0.0], [0.7, -1.2, 11.0]])
    rng = np.random.default_rng(5)
    return Frame([1, 1, 8, 30, 1, 8, 8, 30, 30, 1, 6, 7] * 2, rng.uniform(0, 1, (24, 3)) @ cell, cell)


def _construct(kind, traj, delta_time, distributed):
    from amof_amd.bad import Bad
    from amof_amd.cn import CoordinationNumber
    from amof_amd.msd import WindowMsd
    from amof_amd.rdf import Rdf
    from amof_amd.vanhove import WindowVanHove
    if kind == "Msd":
        return WindowMsd.from_trajectory(traj, delta_time=delta_time, timestep=1, device=0, distributed=distributed)
    if kind == "VanHove":
        return WindowVanHove.from_trajectory(traj, delta_time=delta_time, timestep=1, dr=0.05, device=0, distributed=distributed)
    if kind == "Bad":
        return Bad.from_trajectory(traj, CUT, dtheta=0.5, device=0, distributed=distributed)
    if kind == "Cn":
        return CoordinationNumber.from_trajectory(traj, CUT, device=0, distributed=distributed)
    return Rdf.from_trajectory(traj, dr=0.05, device=0, distributed=distributed)


def _child(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK="0", AMOF_DIST_FORCE_MERGE="1")     # one rank, but every collective really runs
    os.environ.pop("AMOF_ASYNC", None)
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    from amof_amd import _hip, dist as adist
    assert adist.merging(1) and adist.device_collectives()

    trajs = {k: v.to_device(0) for k, v in _host_trajectories().items()}
    base = _general_base()
    trajs["GENERAL"] = H.device_walk_cell(torch.device("cuda", 0), base, base.cell, 64, 0.05, 9)
    np.save(os.path.join(out_dir, "GENERAL.pos.npy"), trajs["GENERAL"].pos_host())

    # the spy: calls of the four entry points, whichever context they are made on
    calls = {}

    def spy(name):
        inner = getattr(_hip.Context, name)

        def wrapper(self, *a, **k):
            calls[name] = calls.get(name, 0) + 1
            return inner(self, *a, **k)
        setattr(_hip.Context, name, wrapper)
    names = ("msd_shard_begin", "msd_shard_finish", "msd_com", "msd_window")
    for name in names:
        spy(name)

    lanes = [_hip.get_context(0), _hip.get_context(0, lane=1)]
    _construct("Msd", trajs["FUSED"], 16, None).data          # warm-up: constructors take milliseconds afterwards
    report = {}
    for run, (objects, reading, _) in RUNS.items():
        calls.clear()
        gate = timer = None
        if run == "sync":
            os.environ["AMOF_ASYNC"] = "0"
        if run.endswith("_gated"):
            # the lane is busy while the objects are built (it frees itself whatever happens)
            gate = threading.Event()
            lanes[1].submit(lambda g=gate: g.wait(timeout=10))
            timer = threading.Timer(1.0, gate.set)
            timer.start()
        rec = report[run] = {"objects": {}}
        try:
            try:
                built = [(name, _construct(kind, trajs[tr], dt, None)) for name, kind, tr, dt in objects]
                rec["unread"] = [o.__dict__.get("_pending") is not None for _, o in built]
            finally:
                if gate is not None:
                    gate.set()
                    timer.cancel()
            for k in reading:
                name, obj = built[k]
                one = rec["objects"][name] = {"error": None}
                try:
                    values = obj.data.values
                except Exception as exc:        # (kept by the object; the parent's test reports it)
                    one["error"] = repr(exc)
                    continue
                one["columns"] = [str(c) for c in obj.data.columns]
                np.save(os.path.join(out_dir, "%s.%s.data.npy" % (run, name)), values)
                if hasattr(obj, "sumsq"):
                    np.save(os.path.join(out_dir, "%s.%s.sumsq.npy" % (run, name)), obj.sumsq)
                    one["path"] = obj._stats["path"]
                one["pending"] = obj.__dict__.get("_pending") is not None
        except Exception as exc:                # (a constructor raised)
            rec["error"] = repr(exc)
        finally:
            os.environ.pop("AMOF_ASYNC", None)
        for lane in lanes:
            lane.drain()
        rec["calls"] = [calls.get(name, 0) for name in names]
        rec["lanes_idle"] = [lane._jobs_finished == lane._jobs_submitted for lane in lanes]
    with open(os.path.join(out_dir, "report.json"), "w") as f:
        json.dump(report, f)
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def child(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("msd_shard_class"))
    port = 45600 + os.getpid() % 2000
    mp.spawn(_child, args=(1, port, out), nprocs=1, join=True)
    with open(os.path.join(out, "report.json")) as f:
        return out, json.load(f)


@pytest.fixture(scope="module")
def trajectories(child):
    host = _host_trajectories()
    base = _general_base()
    host["GENERAL"] = PackedTrajectory(np.load(os.path.join(child[0], "GENERAL.pos.npy")), base.cell, base.numbers)
    return host, {k: v.to_device(0) for k, v in host.items()}


@pytest.fixture(scope="module")
def single(trajectories):
    """the same class in this process with distributed=False, built once per (class, trajectory, delta_time)"""
    cache = {}

    def get(kind, tr, dt):
        if (kind, tr, dt) not in cache:
            cache[(kind, tr, dt)] = _construct(kind, trajectories[1][tr], dt, False)
        return cache[(kind, tr, dt)]
    return get


@pytest.fixture(scope="module")
def restated(trajectories):
    """``(window, elements, MSD per element)`` of oracle.numpy_oracle.window_msd_fast, once per (trajectory, delta_time)"""
    cache = {}

    def get(tr, dt):
        if (tr, dt) not in cache:
            p = trajectories[0][tr]
            window = np.arange(0, p.n_frames // 2, dt)
            elements, ref = no.window_msd_fast(p.pos, p.cell, p.numbers, p.masses, window)
            cache[(tr, dt)] = (window, [int(e) for e in elements], [np.asarray(r) for r in ref])
        return cache[(tr, dt)]
    return get


def _check_restated(packed, data, columns, sumsq, window, elements, ref):
    """sumsq in the manner of test_gpu_msd_fused.py::_check_oracle; the species columns and the formula-weighted X column of
    ``.data`` from the same restated values (amof/msd.py:259-268)"""
    from amof_amd import _hip, data as adata
    kinds, _ = _hip.packed_species(packed)
    F = packed.n_frames
    total = 0.0
    for e, r in zip(elements, ref):
        n_e = int((packed.numbers == e).sum())
        np.testing.assert_allclose(sumsq[kinds.index(e)] / n_e / (F - window), r, rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(data[:, columns.index(adata.chemical_symbols[e])], r, rtol=1e-9, atol=1e-12)
        total = total + n_e * r
    np.testing.assert_allclose(data[:, columns.index("X")], total / packed.n_atoms, rtol=1e-9, atol=1e-12)
    assert np.array_equal(data[:, columns.index("Time")], window)


@pytest.mark.parametrize("run", list(RUNS))
def test_sharded_msd_through_the_class(child, trajectories, single, restated, run):
    """one run of the child: nothing raised and nothing is left pending, the entry points that ran are the branch's, the
    lanes are idle, and every result equals the single process (1e-12) and, the MSDs, the float64 restatement (1e-9).

    Path of the record (``_stats``): a fused pair leaves "msd_fused"; GAS, whose finish answers through the transposed
    forms with the completed centre of mass (the wrap-again flag), leaves that form's name, "msd_comb" -- the record does
    tell the two apart."""
    out, report = child
    objects, reading, expected_calls = RUNS[run]
    rec = report[run]
    assert rec.get("error") is None, rec
    assert [rec["objects"][name]["error"] for name, _, _, _ in objects] == [None] * len(objects), rec
    if run != "sync":
        assert rec["unread"] == [True] * len(objects)             # (built unread, read afterwards)
    assert not any(o["pending"] for o in rec["objects"].values())
    assert tuple(rec["calls"]) == expected_calls, run
    assert rec["lanes_idle"] == [True, True]
    for name, kind, tr, dt in objects:
        one = rec["objects"][name]
        data = np.load(os.path.join(out, "%s.%s.data.npy" % (run, name)))
        ref = single(kind, tr, dt)
        assert one["columns"] == [str(c) for c in ref.data.columns]
        np.testing.assert_allclose(data, ref.data.values, rtol=1e-12, atol=1e-15, err_msg="%s %s" % (run, name))
        if kind != "Msd":
            continue
        sumsq = np.load(os.path.join(out, "%s.%s.sumsq.npy" % (run, name)))
        np.testing.assert_allclose(sumsq, ref.sumsq, rtol=1e-12, atol=1e-15, err_msg="%s %s" % (run, name))
        _check_restated(trajectories[0][tr], data, one["columns"], sumsq, *restated(tr, dt))
        if tr == "GAS":
            assert one["path"] == "msd_comb" and ref._stats["path"] != "msd_fused"
        elif tr in ("FUSED", "NPT") and dt >= 16:
            assert one["path"] == "msd_fused" == ref._stats["path"]
        else:
            assert one["path"] != "msd_fused"
