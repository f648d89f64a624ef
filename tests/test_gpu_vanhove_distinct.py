"""Distinct Van Hove function on the GPU (amof_vanhove_distinct[_dev], DistinctVanHove): every count bit-exact against
the oracle construction of tests/vanhove_distinct_ref.py, every forced path asserted through last_path()."""

import os
import sys

import numpy as np
import pytest

from amof_amd import lags
from amof_amd import vanhove_distinct as vd
from amof_amd.frames import Frame, PackedTrajectory
from amof_amd.lags import window_setup
from tests import edge_plant as E
from tests import helpers as H
from tests import vanhove_distinct_ref as ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

EXACT = {"AMOF_VANHOVE_DISTINCT_EXACT": "1"}
GLOBAL = {"AMOF_VANHOVE_DISTINCT_GLOBAL": "1"}
DIAG = np.diag([17.31, 18.93, 21.77])
SHEARED = np.array([[17.31, 0.0, 0.0], [2.93, 18.11, 0.0], [-1.71, 3.37, 19.53]])


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


def _device(packed):
    import torch
    return PackedTrajectory(torch.as_tensor(packed.pos).cuda(), packed.cell, packed.numbers, pbc=packed.pbc)


def _walk(cell, numbers, F, seed, sigma=0.3, pbc=(True, True, True)):
    """host random walk in any cell (or per-frame cells), positions wrapped into frame 0's cell then re-expressed"""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cell, dtype=np.float64).reshape(-1, 3, 3)
    N = len(numbers)
    s = rng.uniform(0, 1, (N, 3))
    pos = np.empty((F, N, 3))
    for f in range(F):
        pos[f] = (s - np.floor(s)) @ cells[0 if len(cells) == 1 else f]
        s = s + rng.normal(scale=sigma, size=(N, 3)) @ np.linalg.inv(cells[0])
    return PackedTrajectory(pos, cells if len(cells) > 1 else cells[0], np.asarray(numbers), pbc=pbc)


def _case(hip_ctx, packed, windows, rmax, nbins, runs, stride=1, device=False):
    """runs: [(env, path)]: each forced path must run and equal the oracle construction bit for bit"""
    want = ref.distinct_hist(packed.pos, packed.cell, packed.numbers, windows, rmax, nbins, stride, pbc=tuple(packed.pbc))
    assert want.sum() > 0
    inputs = [packed, _device(packed)] if device else [packed]
    for env, path in runs:
        for inp in inputs:
            with _env(**env):
                got, kinds = hip_ctx.vanhove_distinct(inp, windows, rmax, nbins, origin_stride=stride)
                ran = hip_ctx.last_path()
            assert ran == path, (env, ran, path)
            assert kinds == ref.species(packed.numbers)[0]
            bad = np.argwhere(got != want)
            assert len(bad) == 0, (path, int(np.abs(got.astype(np.int64) - want.astype(np.int64)).sum()), bad[:8].tolist())
    return want


def _numbers4(n):
    return np.repeat([1, 6, 7, 30], [n - 3 * (n // 4), n // 4, n // 4 - 1, n // 4 + 1])


@pytest.mark.parametrize("S", [1, 4])
def test_rectangular_cell_all_paths(hip_ctx, S):
    """N = 301 (no multiple of a tile), the largest lag max_time='half' allows with its last origin F - m - 1"""
    numbers = _numbers4(301) if S == 4 else np.full(301, 30)
    F = 14
    packed = _walk(DIAG, numbers, F, seed=10 + S)
    windows, _ = window_setup(F, 2)
    wl, kl = lags.work_list(F, windows)
    assert (len(windows) - 1, F - windows[-1] - 1) in set(zip(wl.tolist(), kl.tolist()))
    rmax, nbins = 8.6, 430
    _case(hip_ctx, packed, windows, rmax, nbins, [({}, "rdf_distinct_tile"), (EXACT, "rdf_distinct_exact"),
                                                   (GLOBAL, "rdf_distinct_exact_global")], device=S == 4)
    _case(hip_ctx, packed, windows, rmax, nbins, [({}, "rdf_distinct_tile")], stride=3)


def test_triclinic_npt_and_open_axis_take_the_exact_kernel(hip_ctx):
    numbers = _numbers4(263)
    windows = np.array([0, 1, 3, 4], dtype=np.int32)
    tri = _walk(SHEARED, numbers, 8, seed=21)
    _case(hip_ctx, tri, windows, 8.0, 333, [({}, "rdf_distinct_exact"), (GLOBAL, "rdf_distinct_exact_global")], device=True)
    # a sheared cell at the half-length clamp: a second image of some pairs in reach (image lists of frame k's cell)
    _case(hip_ctx, tri, windows, float(vd.clamp_rmax(np.linalg.norm(SHEARED, axis=1), "half_cell")), 400,
          [({}, "rdf_distinct_exact")])
    rng = np.random.default_rng(4)
    npt_cells = np.stack([DIAG * (1.0 + 0.03 * rng.uniform(-1, 1)) for _ in range(8)])
    npt = _walk(npt_cells, numbers, 8, seed=22)
    _case(hip_ctx, npt, windows, 8.0, 500, [({}, "rdf_distinct_exact")], stride=2, device=True)
    slab = _walk(DIAG, numbers, 8, seed=23, pbc=(True, True, False))
    _case(hip_ctx, slab, windows, 8.0, 500, [({}, "rdf_distinct_exact"), (GLOBAL, "rdf_distinct_exact_global")])
    assert hip_ctx.last_path() == "rdf_distinct_exact_global"


def test_npt_walk_in_hbm(hip_ctx):
    import torch
    base = H.replicate(H.zif4_frame(), (1, 1, 1))
    F = 10
    rng = np.random.default_rng(7)
    cells = np.stack([np.asarray(base.cell) * (1.0 + 0.02 * rng.uniform(-1, 1)) for _ in range(F)])
    packed = H.device_walk_cell(torch.device("cuda", 0), base, cells, F, 0.05, 8)
    host = PackedTrajectory(packed.pos.cpu().numpy(), packed.cell, packed.numbers)
    windows = np.array([0, 2, 5], dtype=np.int32)
    want = ref.distinct_hist(host.pos, host.cell, host.numbers, windows, 7.0, 700)
    got, _ = hip_ctx.vanhove_distinct(packed, windows, 7.0, 700)
    assert hip_ctx.last_path() == "rdf_distinct_exact"
    assert np.array_equal(got, want)


@pytest.mark.parametrize("nbins", [999, 2310])
def test_guard_band_across_frames(hip_ctx, nbins):
    """frame P with pairs planted within 0.01 .. 10 bands of a bin edge (tests/edge_plant.py); frame P' = P with the atoms
    permuted within each species and some shifted by lattice vectors: the planted pairs become (i at P, j at P') pairs"""
    rmax = 8.0
    numbers = np.repeat([1, 6, 7, 30], [700, 500, 420, 180])
    pl = E.plant_rdf(DIAG, numbers, rmax, nbins, seed=300 + nbins, F=1, far=True)
    P = pl.packed.pos[0]
    rng = np.random.default_rng(nbins)
    perm = np.arange(len(numbers))
    for z in (1, 6, 7, 30):
        idx = np.nonzero(numbers == z)[0]
        perm[idx] = rng.permutation(idx)
    shift = np.where(rng.uniform(0, 1, (len(numbers), 1)) < 0.4, rng.integers(-3, 4, (len(numbers), 3)), 0)
    P2 = P[perm] + shift @ DIAG
    packed = PackedTrajectory(np.stack([P, P, P2, P]), DIAG, numbers)
    windows = np.array([0, 1, 2], dtype=np.int32)
    want = _case(hip_ctx, packed, windows, rmax, nbins, [({}, "rdf_distinct_tile"), (EXACT, "rdf_distinct_exact")],
                 device=nbins == 2310)
    assert want[:, :, 1].sum() > 0 and want[:, :, 2].sum() > 0


def test_work_halves_add_up_and_calls_are_deterministic(hip_ctx):
    packed = _walk(DIAG, _numbers4(517), 16, seed=31)
    windows, _ = window_setup(16, 3)
    n = int(lags.n_origins(16, windows, 2).sum())
    for env, path in (({}, "rdf_distinct_tile"), (EXACT, "rdf_distinct_exact")):
        with _env(**env):
            whole, _ = hip_ctx.vanhove_distinct(packed, windows, 8.0, 800, origin_stride=2)
            assert hip_ctx.last_path() == path
            a, _ = hip_ctx.vanhove_distinct(packed, windows, 8.0, 800, origin_stride=2, work_range=(0, n // 2 + 1))
            b, _ = hip_ctx.vanhove_distinct(packed, windows, 8.0, 800, origin_stride=2, work_range=(n // 2 + 1, n))
            hip_ctx.debug_poison()
            again, _ = hip_ctx.vanhove_distinct(packed, windows, 8.0, 800, origin_stride=2)
        assert np.array_equal(a + b, whole) and np.array_equal(again, whole)
    want = ref.distinct_hist(packed.pos, packed.cell, packed.numbers, windows, 8.0, 800, 2)
    assert np.array_equal(whole, want)
    # the device form adds into the caller's buffer
    import torch
    out = torch.ones(whole.shape, dtype=torch.int64, device="cuda:0")
    hip_ctx.vanhove_distinct(_device(packed), windows, 8.0, 800, origin_stride=2, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), whole + 1)
    # two contexts of one device sharing the work list (MultiContext)
    from amof_amd import _hip
    multi = _hip.MultiContext([0, 0])
    try:
        m, _ = multi.vanhove_distinct(packed, windows, 8.0, 800, origin_stride=2)
    finally:
        multi.close()
    assert np.array_equal(m, whole)


def _lag_cuts(F, windows, stride):
    """the work list cut exactly on the first lag boundary, an empty piece there, a cut inside the second lag, the rest"""
    n = lags.n_origins(F, windows, stride)
    total = int(n.sum())
    assert len(n) == 3 and n[1] > 2
    return [(0, int(n[0])), (int(n[0]), int(n[0])), (int(n[0]), int(n[0]) + 2), (int(n[0]) + 2, total)], total


@pytest.mark.parametrize("F", [11, 12])
@pytest.mark.parametrize("exact", [False, True])
def test_work_list_cut_at_lag_boundaries(hip_ctx, monkeypatch, F, exact):
    """three species, 71 atoms, lags [0, 2, 5], every second origin: F = 11 has 5, 4 and 3 origins per lag, F = 12 has 6, 5
    and 3.  The pieces -- into host arrays (zeroed by every call) and into one device tensor (added into) -- sum to the
    single full call bit for bit."""
    import torch
    windows, stride, rmax, nbins = np.array([0, 2, 5], dtype=np.int32), 2, 5.0, 40
    numbers = np.repeat([1, 6, 30], [31, 24, 16])
    gas = H.random_gas(len(numbers), [11.3, 12.1, 13.7], numbers, 51)
    packed = H.random_walk(Frame(numbers, gas.pos[0], gas.cell[0], (True, True, True)), F, 0.2, 52, ortho=True)
    cuts, total = _lag_cuts(F, windows, stride)
    if F == 11:
        assert lags.n_origins(F, windows, stride).tolist() == [5, 4, 3] and cuts == [(0, 5), (5, 5), (5, 7), (7, 12)]
    if exact:
        monkeypatch.setenv("AMOF_VANHOVE_DISTINCT_EXACT", "1")      # (read per call)
    whole, _ = hip_ctx.vanhove_distinct(packed, windows, rmax, nbins, origin_stride=stride)
    assert hip_ctx.last_path() == ("rdf_distinct_exact" if exact else "rdf_distinct_tile")
    assert whole.sum() > 0 and whole.shape == (3, 3, 3, nbins)
    assert np.array_equal(whole, hip_ctx.vanhove_distinct(packed, windows, rmax, nbins, origin_stride=stride, work_range=(0, total))[0])
    parts = [hip_ctx.vanhove_distinct(packed, windows, rmax, nbins, origin_stride=stride, work_range=c)[0] for c in cuts]
    assert parts[1].sum() == 0 and all(parts[k].sum() > 0 for k in (0, 2, 3))
    assert parts[0][:, :, 1:].sum() == 0 and parts[2][:, :, 0].sum() == 0      # the cut sits exactly on the lag boundary
    assert np.array_equal(sum(parts), whole)
    out = torch.zeros(whole.shape, dtype=torch.int64, device="cuda:0")
    for c in cuts:
        hip_ctx.vanhove_distinct(packed, windows, rmax, nbins, origin_stride=stride, work_range=c, out=out)
    assert np.array_equal(out.cpu().numpy().view(np.uint64), whole)


def test_lag0_ties_to_the_rdf_at_the_headline_geometry(hip_ctx):
    """9792 atoms (ZIF-4 3x3x4 in HBM): the lag-0 counts equal amof_rdf_accumulate over frames 1 .. F-1 on both paths,
    and the t = 0 rows of DistinctVanHove.data equal Rdf on those frames"""
    import torch
    from amof_amd.rdf import Rdf
    F = 120
    packed = H.device_walk(torch.device("cuda", 0), (3, 3, 4), F, 0.05, 41)
    rmax = float(np.min(packed.cell_lengths()) / 2)
    nbins = int(rmax // 0.01)
    rdf, _, _ = hip_ctx.rdf_accumulate(packed, rmax, nbins, frame_range=(1, F))
    for env, path in (({}, "rdf_distinct_tile"), (EXACT, "rdf_distinct_exact")):
        with _env(**env):
            got, _ = hip_ctx.vanhove_distinct(packed, np.array([0], np.int32), rmax, nbins)
            assert hip_ctx.last_path() == path
        assert np.array_equal(got[:, :, 0], rdf), path
    vh = vd.DistinctVanHove.from_trajectory(packed, delta_time=40, timestep=1, device=0)
    r = Rdf.from_trajectory(PackedTrajectory(packed.pos[1:], packed.cell, packed.numbers), device=0)
    assert list(vh.data.columns) == ["Time"] + list(r.data.columns)
    t0 = vh.data.iloc[:nbins]
    for c in r.data.columns:
        np.testing.assert_allclose(t0[c].values, r.data[c].values, rtol=1e-12, atol=0)
    assert len(vh.data) == len(vh.n_origins) * nbins and list(vh.n_origins) == [F - 1, F - 41]
    # the first-shell peak of Zn-N decays with the lag
    zn_n = vh.data["Zn-N"].values.reshape(len(vh.n_origins), nbins)
    assert zn_n[1].max() < zn_n[0].max()


def _run_gd(distributed):
    import torch
    packed = H.device_walk(torch.device("cuda", 0), (1, 1, 2), 40, 0.05, 51)     # same seed on every rank
    vh = vd.DistinctVanHove.from_trajectory(packed, delta_time=6, timestep=1, dr=0.02, origin_stride=3, device=0,
                                            distributed=distributed)
    return {"hist": np.asarray(vh.hist).view(np.int64), "data": vh.data.values}


def _worker_gd(rank, world, port, out_dir, backend):
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
    res = _run_gd(None)
    for k, arr in res.items():
        np.save(os.path.join(out_dir, "%s_rank%d.npy" % (k, rank)), arr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_equal_single_process(tmp_path, backend, world):
    """the work list shared by the ranks (two gloo ranks on cuda:0; one RCCL rank with the collective run on the
    device-resident counts): counts and DataFrame identical to the single process"""
    import torch.multiprocessing as mp
    port = 33600 + (os.getpid() + world) % 2000
    mp.spawn(_worker_gd, args=(world, port, str(tmp_path), backend), nprocs=world, join=True)
    single = _run_gd(False)
    for k, want in single.items():
        for rank in range(world):
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            assert np.array_equal(got, want), k
