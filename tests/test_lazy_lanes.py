"""The asynchronous constructors (amof_amd/_lazy.py, the lanes of amof_amd/_hip.py) on a machine without a GPU:
the classes run on two oracle-backed stand-in lanes (tests/oracle_context.py -- test infrastructure), so what is
checked here is the host machinery: enqueue-and-return, wait at first access, the same exceptions at access (again
at every later access), pickling, AMOF_ASYNC=0, and results identical to the synchronous path."""
import pickle
import threading
import time

import numpy as np
import pandas as pd
import pytest

from amof_amd import _hip, _lazy
from amof_amd.bad import Bad
from amof_amd.cn import CoordinationNumber
from amof_amd.msd import WindowMsd
from amof_amd.rdf import Rdf
from tests import helpers as H
from tests import oracle_context


@pytest.fixture()
def lanes(monkeypatch):
    ls = oracle_context.install(monkeypatch)
    yield ls
    for ctx in ls.values():
        ctx.close_lane()


@pytest.fixture(scope="module")
def traj():
    return H.random_walk(H.zif4_frame(), 9, 0.05, 5)


def _four(traj):
    return (Rdf.from_trajectory(traj, dr=0.05, rmax=6.0, distributed=False),
            WindowMsd.from_trajectory(traj, delta_time=2, timestep=1, distributed=False),
            Bad.from_trajectory(traj, {'Zn-N': 2.5}, dtheta=0.5, distributed=False),
            CoordinationNumber.from_trajectory(traj, {'Zn-N': 2.5}, distributed=False))


def test_async_results_equal_the_synchronous_ones(lanes, traj, monkeypatch):
    monkeypatch.setenv("AMOF_ASYNC", "0")
    sync = _four(traj)
    assert all(o.__dict__.get("_pending") is None for o in sync)
    assert lanes[1].calls == [] and lanes[0].calls == ["rdf", "msd", "bad", "cn"]     # one context, in call order
    monkeypatch.setenv("AMOF_ASYNC", "1")
    lanes[0].calls.clear()
    # hold lane 0 back: the constructors must return with the RDF still queued
    gate = threading.Event()
    lanes[0].submit(gate.wait)
    t0 = time.perf_counter()
    objs = _four(traj)
    assert time.perf_counter() - t0 < 5.0
    assert objs[0].__dict__["_pending"] is not None and not objs[0].__dict__["_pending"][0].done()
    assert objs[0]._ctx is lanes[0] and all(o._ctx is lanes[1] for o in objs[1:])
    gate.set()
    for a, b in zip(objs, sync):
        assert a.data.equals(b.data)                      # bit for bit
        assert a.__dict__["_pending"] is None
    assert np.array_equal(objs[0].hist, sync[0].hist) and objs[0].rmax == sync[0].rmax
    assert np.array_equal(objs[1].sumsq, sync[1].sumsq)
    assert np.array_equal(objs[2].hist, sync[2].hist) and np.array_equal(objs[2].n_angles, sync[2].n_angles)
    assert lanes[0].calls == ["rdf"] and lanes[1].calls == ["msd", "bad", "cn"]
    assert objs[1]._stats["path"] == "msd"


def test_attributes_the_computation_sets_wait_for_it(lanes, traj):
    gate = threading.Event()
    lanes[0].submit(gate.wait)
    rdf = Rdf.from_trajectory(traj, dr=0.05, rmax=6.0, distributed=False)
    assert "hist" not in rdf.__dict__
    threading.Timer(0.2, gate.set).start()
    assert rdf.hist.shape == (4, 4, int(6.0 // 0.05))                  # (waited for the gate and the job)
    with pytest.raises(AttributeError):
        rdf.no_such_attribute
    # an object read back from a file has nothing pending: plain attribute errors, the stored frame
    blank = Rdf()
    with pytest.raises(AttributeError):
        blank.hist
    assert list(blank.data.columns) == ["r"] and len(blank.data) == 0


def test_errors_of_the_library_surface_at_access_every_time(lanes, traj, monkeypatch):
    def boom(*a, **k):
        raise _hip.AmofError(_hip.AMOF_ESINGULAR, "cell of frame 0 is singular")
    monkeypatch.setattr(lanes[0], "rdf_accumulate", boom)
    rdf = Rdf.from_trajectory(traj, dr=0.05, rmax=6.0, distributed=False)       # returns: nothing has been looked at
    for _ in range(2):
        with pytest.raises(_hip.AmofError) as e:
            rdf.data
        assert e.value.code == _hip.AMOF_ESINGULAR
    with pytest.raises(_hip.AmofError):
        rdf.hist
    with pytest.raises(_hip.AmofError):
        rdf.result()

    def zero(*a, **k):
        raise ZeroDivisionError("Undefined angle")
    monkeypatch.setattr(lanes[1], "bad_hist", zero)
    bad = Bad.from_trajectory(traj, {'Zn-N': 2.5}, dtheta=0.5, distributed=False)
    with pytest.raises(ZeroDivisionError):
        bad.data
    # argument errors are raised by the call itself, as in the reference
    with pytest.raises(ValueError):
        Rdf.from_trajectory(traj, dr=10.0, rmax=6.0, distributed=False)
    with pytest.raises(ValueError):
        Rdf.from_trajectory([], distributed=False)


def test_pickle_waits_and_old_pickles_keep_their_frame(lanes, traj):
    msd = WindowMsd.from_trajectory(traj, delta_time=2, timestep=1, distributed=False)
    again = pickle.loads(pickle.dumps(msd))               # (waits; futures and locks are not pickled)
    assert again.data.equals(msd.data) and np.array_equal(again.sumsq, msd.sumsq)
    assert "_pending" not in again.__dict__ and "_ctx" not in again.__dict__
    # an object pickled before `data` became a descriptor carries the plain key
    old = Rdf.__new__(Rdf)
    old.__dict__["data"] = pd.DataFrame({"r": [0.0, 0.1], "X-X": [0.0, 1.0]})
    back = pickle.loads(pickle.dumps(old))
    assert list(back.data.columns) == ["r", "X-X"] and len(back.data) == 2


def test_a_finishing_step_that_fails_is_not_run_twice():
    class Obj(_lazy.Deferred):
        pass
    lane = oracle_context.OracleContext("t")
    runs = []

    def finish(raw):
        runs.append(raw)
        raise RuntimeError("merge failed")
    o = Obj()
    o._defer(lane, lambda: 7, finish, collective=True)
    for _ in range(3):
        with pytest.raises(RuntimeError, match="merge failed"):
            o.result()
    assert runs == [7]
    lane.close_lane()


def test_lane_runs_jobs_in_order_and_drain_waits():
    lane = oracle_context.OracleContext("t2")
    seen = []
    futs = [lane.submit(lambda k=k: (time.sleep(0.01), seen.append(k))) for k in range(5)]
    lane.drain()
    assert seen == [0, 1, 2, 3, 4] and all(f.done() for f in futs)
    lane.submit(lambda: lane.drain())      # draining from the lane's own thread must not wait on itself
    lane.drain()
    lane.close_lane()


def _sharded_msd_pairs(lane, packed, first_half):
    """What WindowMsd.compute_msd does on its lane's context in an atom-sharded run with device collectives
    (amof_amd/msd.py), twice, with two window lists, behind a lane that is busy -- the first half through ``first_half(ctx,
    fn)``, the all-reduce (one rank: nothing to add), the second half submitted -- and an unrelated job of another class
    queued before each.  The stand-in's halves enforce the C side's rule: a finish is the next call after its begin.
    Returns the futures of the second halves and the tables they add into."""
    kinds, _ = _hip.packed_species(packed)
    whole = (0, packed.n_atoms)
    gate = threading.Event()
    lane.submit(lambda: gate.wait(timeout=10))          # (frees itself whatever happens)
    threading.Timer(1.0, gate.set).start()
    futs, outs = [], []
    for window in (np.array([0, 1, 2, 3], dtype=np.int32), np.array([0, 2], dtype=np.int32)):
        lane.submit(lambda: lane.cn_count(packed, np.full((len(kinds), len(kinds)), 2.5), [(0, 1)]))
        csum = np.empty((packed.n_frames, 3))
        out = np.zeros((len(kinds), len(window)))
        first_half(lane, lambda: lane.msd_shard_begin(packed, window, whole, csum))
        # (all_reduce_sum(csum): in the calling thread, no call of the context)
        futs.append(lane.submit(lambda w=window, c=csum, o=out: lane.msd_shard_finish(packed, w, whole, c, o)))
        outs.append((window, csum, out))
    gate.set()
    lane.drain()
    return futs, outs


def test_sharded_msd_halves_are_not_split_by_what_the_lane_has_queued(lanes, traj):
    """``_setup.on_lane`` runs the first half behind the queued jobs and waits, so every finish directly follows its begin:
    both succeed, with the sums of the one-call form.  (With the first half called directly from this thread -- the next
    test -- both finishes are refused.)"""
    from amof_amd import _setup
    lane = lanes[1]
    futs, outs = _sharded_msd_pairs(lane, traj, _setup.on_lane)
    assert lane.calls == ["cn", "msd_shard_begin", "msd_shard_finish"] * 2
    for fut, (window, csum, out) in zip(futs, outs):
        got, kinds = fut.result(timeout=10)
        assert got is out
        ref, _ = lane.msd_window(traj, window)
        assert np.array_equal(out, ref) and out.any()
        np.testing.assert_allclose(csum, (traj.pos_host() * traj.masses[None, :, None]).sum(axis=1), rtol=1e-14)
    assert lane._jobs_finished == lane._jobs_submitted


def test_the_stand_in_refuses_a_finish_that_does_not_follow_its_begin(lanes, traj, monkeypatch):
    """the stand-in's rule is the C side's (tests/test_gpu_msd_fused.py::test_sharded_halves_add_up_to_the_whole): the same
    sequence with the first half called from the constructing thread -- both begins run at once, the second replaces the
    first's ticket and key, the queued jobs follow -- and each finish raises.  on_lane itself calls directly where the
    classes run synchronously, where there is no lane, and from the lane's own thread."""
    from amof_amd import _setup
    lane = lanes[1]
    futs, outs = _sharded_msd_pairs(lane, traj, lambda ctx, fn: fn())
    assert lane.calls == ["msd_shard_begin", "msd_shard_begin", "cn", "msd_shard_finish", "cn", "msd_shard_finish"]
    for fut, (_, _, out) in zip(futs, outs):
        with pytest.raises(ValueError, match="must follow"):
            fut.result(timeout=10)
        assert not out.any()
    # a finish right after its begin, but with other arguments
    w = np.array([0, 1], dtype=np.int32)
    out = np.zeros((4, 2))
    lane.msd_shard_begin(traj, w, (0, 5), np.empty((traj.n_frames, 3)))
    with pytest.raises(ValueError, match="must follow"):
        lane.msd_shard_finish(traj, w, (0, 6), np.empty((traj.n_frames, 3)), out)
    # where on_lane does not queue
    here = threading.get_ident()
    submitted = lane._jobs_submitted
    monkeypatch.setenv("AMOF_ASYNC", "0")
    assert _setup.on_lane(lane, threading.get_ident) == here
    monkeypatch.setenv("AMOF_ASYNC", "1")
    assert _setup.on_lane(object(), threading.get_ident) == here
    assert lane._jobs_submitted == submitted
    assert _setup.on_lane(lane, threading.get_ident) == lane._lane_thread != here
    assert lane.submit(lambda: _setup.on_lane(lane, threading.get_ident)).result(timeout=10) == lane._lane_thread
    with pytest.raises(_hip.Unsupported):       # what the call raises is raised to the constructor
        _setup.on_lane(lane, lambda: (_ for _ in ()).throw(_hip.Unsupported(_hip.AMOF_EUNSUPPORTED, "general cell")))


def test_a_following_lane_without_a_gpu_context_runs_at_once():
    """Lane.follow_leader is a GPU matter (amof_amd/_hip.py Context.follow_leader): the stand-in lanes of the CPU suite have
    no leader, count their jobs all the same, and run a job as soon as it is submitted"""
    from tests.oracle_context import OracleContext
    lead, second = OracleContext("lead"), OracleContext("second")
    assert second._follows is None and second.device_calls() == 0
    import threading
    gate = threading.Event()
    f0 = lead.submit(lambda: gate.wait(5) and "lead done")
    f1 = second.submit(lambda: "second done")
    assert f1.result(timeout=5) == "second done" and not f0.done()
    gate.set()
    assert f0.result(timeout=5) == "lead done"
    assert (lead._jobs_submitted, lead._jobs_started, lead._jobs_finished) == (1, 1, 1)
    lead.close_lane()
    second.close_lane()


def test_reading_the_first_lanes_result_finishes_the_other_lanes_first(monkeypatch):
    """results merged in the calling thread (multi-rank runs): a look at the first lane's result first finishes the pending
    results of the lanes that follow it, oldest first; what one of them raises stays with it"""
    from amof_amd._lazy import Deferred
    from tests.oracle_context import OracleContext
    monkeypatch.setenv("AMOF_ASYNC", "1")
    lead, second = OracleContext("lead"), OracleContext("second")
    second._follows = lead

    class Result(Deferred):
        pass
    order = []
    a, b, c, d = Result(), Result(), Result(), Result()
    b._defer(second, lambda: "b", lambda raw: order.append(raw), collective=True)
    a._defer(lead, lambda: "a", lambda raw: order.append(raw), collective=True)

    def boom(raw):
        order.append(raw)
        raise ValueError("c failed")
    c._defer(second, lambda: "c", boom, collective=True)
    d._defer(second, lambda: order.append("d (wholly on its lane)"), lambda raw: None, collective=False)
    a.result()
    assert [x for x in order if len(x) == 1] == ["b", "c", "a"]
    assert b.__dict__["_pending"] is None and a.__dict__["_pending"] is None
    for _ in range(2):
        with pytest.raises(ValueError):
            c.result()
    assert [x for x in order if len(x) == 1] == ["b", "c", "a"]        # (the failed step is not run again)
    # a follower's own reader finishes nothing else
    e, f = Result(), Result()
    e._defer(lead, lambda: "e", lambda raw: order.append(raw), collective=True)
    f._defer(second, lambda: "f", lambda raw: order.append(raw), collective=True)
    f.result()
    assert e.__dict__["_pending"] is not None and order[-1] == "f"
    e.result()
    lead.close_lane()
    second.close_lane()
