"""Velocity autocorrelation on the GPU (amof_vacf_window) against the numpy restatement (tests/vacf_ref.py).

The raw sums cancel, so they are held against the sum that does not: |gpu - ref| <= 1e-9 * sum |x(k) x(k + m)| -- the
project's bound for the MSD's sums (tests/test_gpu_msd_fused.py: _check_oracle).  Where two GPU results must be the same
bits -- the two kernels, two identical calls -- they are compared with array_equal."""

import functools
import os
import sys

import numpy as np
import pytest

from amof_amd import lags
from amof_amd.frames import PackedTrajectory
from tests import helpers as H
from tests import vacf_ref as ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

TRICLINIC = np.array([[5.0, 0.0, 0.0], [1.5, 5.5, 0.0], [-1.0, 1.2, 6.0]])


class _env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _gas_walk(numbers, F, cell, sigma, seed, jitter=0.0):
    """Gaussian steps in a small cell, wrapped every frame into that frame's cell (jitter: a cell per frame): many face
    crossings"""
    rng = np.random.default_rng(seed)
    n = len(numbers)
    cell = np.asarray(cell, dtype=float)
    cells = cell[None] * (1.0 + jitter * rng.normal(size=(F, 1, 1))) if jitter else cell[None]
    p = rng.random((n, 3)) @ cell + np.cumsum(rng.normal(scale=sigma, size=(F, n, 3)), axis=0)
    pos = np.empty_like(p)
    for k in range(F):
        c = cells[k if jitter else 0]
        s = np.linalg.solve(c.T, p[k].T).T
        pos[k] = (s - np.floor(s)) @ c
    return PackedTrajectory(pos, cells if jitter else cell, numbers)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(trajectory, windows, origin stride, path): the shapes of the parity table"""
    small, ragged = [30] + [7] * 4, [30] + [7] * 3 + [6] * 9
    ortho = np.diag([4.0, 4.5, 5.0])
    if name == "a":         # fewer lags than one wave spans; a one-atom block
        tr = _gas_walk(small, 67, ortho, 0.3, 31)
    elif name == "b":       # F and M multiples of nothing; a ragged last block; the cell crossed many times
        tr = _gas_walk(ragged, 1031, ortho, 0.3, 32)
    elif name == "c":
        tr = _gas_walk(ragged, 1031, TRICLINIC, 0.3, 33)
    elif name == "d":
        tr = _gas_walk(ragged, 1031, ortho, 0.3, 34, jitter=0.01)
    elif name == "e":       # delta_time = 4 timestep, origin_stride = 3
        tr = _gas_walk(ragged, 1031, ortho, 0.3, 35)
        return tr, np.arange(0, 1031 // 2, 4, dtype=np.int32), 3, "vacf_general"
    elif name == "f":       # a series beyond the LDS budget
        return _gas_walk([8, 1, 1], 19300, ortho, 0.3, 36), np.arange(64, dtype=np.int32), 1, "vacf_general"
    return tr, np.arange(len(tr) // 2, dtype=np.int32), 1, "vacf_lds"


@functools.lru_cache(maxsize=None)
def _want(name):
    tr, windows, stride, _ = _case(name)
    return ref.vacf(tr, windows, origin_stride=stride)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
def test_parity_with_the_restatement(hip_ctx, name):
    tr, windows, stride, path = _case(name)
    want = _want(name)
    if name == "b":
        assert len(windows) == 515 and want[1].tolist() == lags.n_origins(1031, windows).tolist()
    got, kinds = hip_ctx.vacf_window(tr, windows, origin_stride=stride)
    assert hip_ctx.last_path() == path
    assert list(kinds) == list(want[3]) and got.shape == want[0].shape
    ref.check(got, want)


# every lag of the table's first shapes (two column buffers, one wave); two waves with two buffers; two lag tiles of three waves
# with one buffer, and with two (AMOF_VACF_DB); a series that leaves room for one buffer only
@pytest.mark.parametrize("name,shape", [("a", None), ("b", None), ("waves", (2400, 1200)), ("tiles", (6000, 3000)),
                                        ("tiles_db", (6000, 3000)), ("single", (12000, 64))])
def test_both_kernels_give_the_same_bits(hip_ctx, name, shape):
    if shape is None:
        tr, windows, _, _ = _case(name)
    else:
        tr, windows = _gas_walk([8, 1], shape[0], np.diag([4.0, 4.5, 5.0]), 0.3, 37), np.arange(shape[1], dtype=np.int32)
    with _env(**({"AMOF_VACF_DB": "1"} if name == "tiles_db" else {})):
        fast, _ = hip_ctx.vacf_window(tr, windows)
    assert hip_ctx.last_path() == "vacf_lds"
    if name in ("a", "b"):          # one buffer where two are the rule
        with _env(AMOF_VACF_NODB="1"):
            single, _ = hip_ctx.vacf_window(tr, windows)
        assert hip_ctx.last_path() == "vacf_lds" and np.array_equal(fast.view(np.uint64), single.view(np.uint64))
    with _env(AMOF_VACF_GENERAL="1"):
        general, _ = hip_ctx.vacf_window(tr, windows)
        assert hip_ctx.last_path() == "vacf_general"
    assert np.array_equal(fast.view(np.uint64), general.view(np.uint64))
    assert np.isfinite(fast).all() and (fast[:, 0] > 0).all()


def test_two_identical_calls_are_bit_identical(hip_ctx):
    tr, windows, _, _ = _case("b")
    for env in ({}, {"AMOF_VACF_GENERAL": "1"}):
        with _env(**env):
            a, _ = hip_ctx.vacf_window(tr, windows)
            hip_ctx.debug_poison()
            b, _ = hip_ctx.vacf_window(tr, windows)
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_atom_ranges_add_up_to_the_whole(hip_ctx):
    import torch
    tr, windows, _, _ = _case("b")
    want = _want("b")
    N, a = tr.n_atoms, 6
    dev = tr.to_device(0)
    com = torch.zeros((len(tr), 3), dtype=torch.float64, device="cuda:0")
    hip_ctx.msd_com(dev, (0, len(tr)), com)
    # the _dev form adds into a buffer that is not zero
    out = torch.full((len(want[3]), len(windows)), 2.5, dtype=torch.float64, device="cuda:0")
    hip_ctx.vacf_window(dev, windows, atom_range=(0, a), com=com, out=out)
    hip_ctx.vacf_window(dev, windows, atom_range=(a, N), com=com, out=out)
    # (two additions into 2.5 + s, each rounded to half an ulp of its result, beside the bound of the sums themselves)
    err = np.abs(out.cpu().numpy() - 2.5 - want[0])
    assert (err <= ref.REL * want[2] + 2.0 ** -52 * (2.5 + np.abs(want[0]))).all()
    # each range against the restatement of that range (the centre of mass still the whole system's)
    for rng in ((0, a), (a, N)):
        got, _ = hip_ctx.vacf_window(tr, windows, atom_range=rng)
        ref.check(got, ref.vacf(tr, windows, atom_range=rng))
    # two contexts of one device sharding the atoms (MultiContext)
    from amof_amd import _hip
    multi = _hip.MultiContext([0, 0])
    try:
        m, _ = multi.vacf_window(tr, windows)
    finally:
        multi.close()
    ref.check(m, want)


def _velocity_walk(seed, drift=None):
    rng = np.random.default_rng(seed)
    numbers = [30] + [7] * 3 + [6] * 9
    vel = rng.normal(scale=0.01, size=(1031, len(numbers), 3))
    vel = 0.9 * vel + 0.1 * np.cumsum(vel, axis=0) / 10.0
    if drift is not None:
        vel = vel + np.asarray(drift)[None, None, :]
    return PackedTrajectory(vel, np.eye(3), numbers)


def test_velocity_mode(hip_ctx):
    tr = _velocity_walk(41)
    windows = np.arange(515, dtype=np.int32)
    want = ref.vacf(tr, windows, velocity_mode=True)
    got, kinds = hip_ctx.vacf_window(tr, windows, velocities=True)
    assert hip_ctx.last_path() == "vacf_lds" and list(kinds) == list(want[3])
    ref.check(got, want)
    with _env(AMOF_VACF_GENERAL="1"):
        general, _ = hip_ctx.vacf_window(tr, windows, velocities=True)
    assert np.array_equal(got.view(np.uint64), general.view(np.uint64))
    # without the mean removed, and thinned origins of strided lags
    raw, _ = hip_ctx.vacf_window(tr, windows, velocities=True, remove_com=False)
    ref.check(raw, ref.vacf(tr, windows, velocity_mode=True, remove_com=False))
    some = np.arange(0, 515, 5, dtype=np.int32)
    thin, _ = hip_ctx.vacf_window(tr, some, origin_stride=2, velocities=True)
    ref.check(thin, ref.vacf(tr, some, origin_stride=2, velocity_mode=True))
    # a uniform drift goes with the frame's mean: the result without the drift, within the same bound
    drifting = _velocity_walk(41, drift=(0.03, -0.02, 0.05))
    moved, _ = hip_ctx.vacf_window(drifting, windows, velocities=True)
    ref.check(moved, want)
    # a device trajectory with the mean handed in
    import torch
    dev = tr.to_device(0)
    com = torch.zeros((len(tr), 3), dtype=torch.float64, device="cuda:0")
    hip_ctx.msd_com(dev, (0, len(tr)), com)
    res, _ = hip_ctx.vacf_window(dev, windows, velocities=True, com=com)
    ref.check(res.cpu().numpy(), want)


def test_ballistic_pair_across_the_cell():
    # two equal-mass atoms, opposite constant velocities, mirror positions: both cross a face in the same frame, so the centre
    # of mass rests.  Every step is v, every product |v|^2.
    from amof_amd.vacf import VelocityAutocorrelation
    F, L = 201, np.array([5.0, 6.0, 7.0])
    v = np.array([0.217, -0.113, 0.071])
    p = (np.array([1.03, 2.51, 3.77]) + np.arange(F)[:, None] * v) % L
    pos = np.stack([p, (L - p) % L], axis=1)
    assert (np.abs(np.diff(p, axis=0)) > 1.0).any()                 # the cell is crossed
    tr = PackedTrajectory(pos, np.diag(L), [8, 8])
    vacf = VelocityAutocorrelation.from_trajectory(tr, timestep=2, device=0, distributed=False)
    assert len(vacf.data) == 100 and list(vacf.data.columns) == ["Time", "O", "X"]
    np.testing.assert_allclose(vacf.data["O"].values, v @ v / 4.0, rtol=1e-9)
    np.testing.assert_allclose(vacf.data["X"].values, v @ v / 4.0, rtol=1e-9)
    np.testing.assert_allclose(vacf.diffusion()["O"], v @ v / 4.0 * 198.0 / 3.0, rtol=1e-9)


def test_antiphase_oscillators_peak_at_their_frequency():
    from amof_amd.vacf import VelocityAutocorrelation
    F, period, dt = 1031, 40, 2
    x = 0.2 * np.sin(2 * np.pi * np.arange(F) / period)
    pos = np.zeros((F, 2, 3))
    pos[:, 0] = [2.0, 2.0, 2.0]
    pos[:, 1] = [5.0, 5.0, 5.0]
    pos[:, 0, 0] += x
    pos[:, 1, 0] -= x
    tr = PackedTrajectory(pos, np.diag([8.0, 8.0, 8.0]), [8, 8])
    vacf = VelocityAutocorrelation.from_trajectory(tr, timestep=dt, device=0, distributed=False)
    assert vacf._stats["path"] == "vacf_lds" and len(vacf.data) == 515
    assert vacf.normalised()["O"].values[0] == 1.0 and vacf.normalised()["X"].values[0] == 1.0
    d = vacf.vdos()
    f = d["Frequency_THz"].values
    nu0 = 1.0e3 / (period * dt)                                     # THz
    for name in ("O", "X"):
        assert abs(f[np.argmax(d[name].values)] - nu0) <= f[1] - f[0]
    # the lags thinned: still evenly spaced from 0; thinned further by hand: refused
    coarse = VelocityAutocorrelation.from_trajectory(tr, delta_time=4 * dt, timestep=dt, origin_stride=3, device=0, distributed=False)
    assert coarse._stats["path"] == "vacf_general"
    fc = coarse.vdos()["Frequency_THz"].values
    assert abs(fc[np.argmax(coarse.vdos()["O"].values)] - nu0) <= fc[1] - fc[0]
    coarse.data = coarse.data.drop(index=3).reset_index(drop=True)
    with pytest.raises(ValueError):
        coarse.vdos()


def test_class_schema_is_window_msds(tmp_path):
    from amof_amd.msd import WindowMsd
    from amof_amd.vacf import VelocityAutocorrelation
    packed = H.random_walk(H.zif4_frame(), 60, 0.05, 20)
    vacf = VelocityAutocorrelation.from_trajectory(packed, delta_time=4, timestep=2, device=0, distributed=False)
    msd = WindowMsd.from_trajectory(packed, delta_time=4, timestep=2, device=0, distributed=False)
    assert list(vacf.data.columns) == list(msd.data.columns)
    np.testing.assert_array_equal(vacf.data["Time"].values, msd.data["Time"].values)
    assert vacf.data.dtypes.tolist() == msd.data.dtypes.tolist()
    # the raw values behind the columns
    window = (msd.data["Time"].values // 2).astype(np.int32)
    want = ref.vacf(packed, window)
    ref.check(vacf.sums, want)
    assert vacf.n_origins.tolist() == want[1].tolist() and list(vacf.kinds) == list(want[3])
    s = vacf.kinds.index(30)
    np.testing.assert_allclose(vacf.data["Zn"].values, vacf.sums[s] / ((packed.numbers == 30).sum() * vacf.n_origins) / 4.0, rtol=1e-15)
    # every lag by default
    every = VelocityAutocorrelation.from_trajectory(packed, timestep=2, device=0, distributed=False)
    assert len(every.data) == 30 and every.data["Time"].values[1] == 2
    vacf.write_to_file(os.path.join(str(tmp_path), "z"))
    assert VelocityAutocorrelation.from_file(os.path.join(str(tmp_path), "z")).data.equals(vacf.data)
    # no lag: the columns, no rows
    empty = VelocityAutocorrelation.from_trajectory(packed, timestep=2, max_time=0, device=0, distributed=False)
    assert list(empty.data.columns) == list(msd.data.columns) and len(empty.data) == 0


def _shard_walks():
    import torch
    return (H.device_walk(torch.device("cuda", 0), (1, 1, 2), 64, 0.05, 21),       # same seed on every rank
            H.random_walk(H.zif4_frame(), 40, 0.05, 22))


def _run_vacf(distributed):
    from amof_amd.vacf import VelocityAutocorrelation
    dev, host = _shard_walks()
    a = VelocityAutocorrelation.from_trajectory(dev, timestep=1, device=0, distributed=distributed)
    b = VelocityAutocorrelation.from_velocities(host, delta_time=2, timestep=1, origin_stride=2, device=0, distributed=distributed)
    return {"sums": np.asarray(a.sums), "data": a.data.values, "sums_v": np.asarray(b.sums), "data_v": b.data.values}


def _worker_vacf(rank, world, port, out_dir, backend):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    if backend == "nccl":
        os.environ["AMOF_DIST_FORCE_MERGE"] = "1"      # one rank, but every collective really runs
    import torch
    import torch.distributed as dist
    torch.cuda.set_device(0)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", 0))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    res = _run_vacf(None)
    for k, arr in res.items():
        np.save(os.path.join(out_dir, "%s_rank%d.npy" % (k, rank)), arr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_equal_single_process(tmp_path, backend, world):
    """atoms sharded over the ranks (two gloo ranks on cuda:0; one RCCL rank with every collective run: the device-resident
    path with the frame-sharded centre of mass): the single process's sums within the tolerance"""
    import torch.multiprocessing as mp
    port = 31700 + (os.getpid() + world) % 2000
    mp.spawn(_worker_vacf, args=(world, port, str(tmp_path), backend), nprocs=world, join=True)
    single = _run_vacf(False)
    dev, host = _shard_walks()
    host_dev = PackedTrajectory(dev.pos_host(), dev.cell, dev.numbers, dev.masses, dev.pbc)
    abs_sums = {"sums": ref.vacf(host_dev, np.arange(32))[2], "sums_v": ref.vacf(host, np.arange(0, 20, 2), origin_stride=2, velocity_mode=True)[2]}
    for rank in range(world):
        for k in ("sums", "sums_v"):
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            assert got.shape == single[k].shape and (np.abs(got - single[k]) <= ref.REL * abs_sums[k]).all(), k
        for k in ("data", "data_v"):         # (the columns are the host's arithmetic on the sums: the lags, the shape)
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            assert got.shape == single[k].shape and np.array_equal(got[:, 0], single[k][:, 0]) and np.isfinite(got).all()
