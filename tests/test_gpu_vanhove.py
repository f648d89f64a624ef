"""Self Van Hove function on the GPU (amof_vanhove_window) against the numpy restatement (tests/vanhove_ref.py): counts
exact up to samples within 1e-8 A of a bin edge (summation order of the running positions), moments to 1e-10."""

import os
import sys

import numpy as np
import pytest

from amof_amd.frames import PackedTrajectory
from oracle import numpy_oracle as no
from tests import helpers as H
from tests import vanhove_ref as ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu


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


def _half_cell_bins(packed, dr):
    return int(float(np.min(packed.cell_lengths()) / 2) // dr)


def _compare(got, want, n_frames, windows, numbers, kinds_want=None):
    counts, overflow, moments, kinds = got
    c_ref, o_ref, m_ref, amb, k_ref = want
    assert list(kinds) == list(k_ref)
    counts = np.asarray(counts, dtype=np.uint64)
    # every sample once: total + overflow = N_s (F - m - 1), exactly
    n_s = np.array([(np.asarray(numbers) == z).sum() for z in k_ref])
    expect = n_s[:, None] * (n_frames - np.asarray(windows)[None, :] - 1)
    np.testing.assert_array_equal(counts.sum(axis=2).astype(np.int64) + overflow.astype(np.int64), expect)
    diff = np.abs(counts.astype(np.int64) - c_ref.astype(np.int64))
    assert (diff <= amb).all(), "bins off by more than their edge samples: %s" % np.argwhere(diff > amb)[:5]
    edge = amb[..., -1] if amb.shape[2] else np.zeros_like(overflow, dtype=np.int64)      # (samples near rmax)
    assert (np.abs(overflow.astype(np.int64) - o_ref.astype(np.int64)) <= edge).all()
    np.testing.assert_allclose(moments, m_ref, rtol=1e-10, atol=1e-12)


def _check(ctx, packed, windows, dr, nbins, unwrap=False, atom_range=None):
    windows = np.asarray(windows, dtype=np.int32)
    got = ctx.vanhove_window(packed, windows, dr, nbins, unwrap=unwrap, atom_range=atom_range)
    sel = packed.numbers if atom_range is None else np.asarray(packed.numbers)[atom_range[0]:atom_range[1]]
    want = ref.vanhove(packed, windows, dr, nbins, unwrap=unwrap, atom_range=atom_range)
    _compare(got, want, len(packed), windows, sel)
    return got


def _gas_walk(n, F, cell, numbers, sigma, seed):
    """n atoms in a small cell, Gaussian steps, wrapped every frame: many face crossings"""
    rng = np.random.default_rng(seed)
    cell = np.asarray(cell, dtype=float)
    p = rng.random((n, 3)) @ cell + np.cumsum(rng.normal(scale=sigma, size=(F, n, 3)), axis=0)
    s = np.linalg.solve(cell.T, p.reshape(-1, 3).T).T
    s -= np.floor(s)
    return PackedTrajectory((s @ cell).reshape(F, n, 3), cell, numbers)


def test_zif4_orthorhombic_walk(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 120, 0.05, 7, ortho=True)
    windows, _ = no.msd_window_setup(120, delta_time=10)
    _check(hip_ctx, packed, windows, 0.01, _half_cell_bins(packed, 0.01))
    assert hip_ctx.last_path() == "msd_vanhove"


def test_sheared_cell(hip_ctx):
    cell = np.array([[9.0, 0.0, 0.0], [2.5, 8.5, 0.0], [-1.5, 2.0, 9.5]])
    packed = _gas_walk(150, 80, cell, [30] * 30 + [7] * 60 + [6] * 60, 0.15, 11)
    _check(hip_ctx, packed, [0, 3, 7, 20, 39], 0.02, 100)
    assert hip_ctx.last_path() == "msd_vanhove"
    # the same trajectory with a jittering cell per frame
    packed = H.random_walk(H.zif4_frame(), 60, 0.05, 12, cell_jitter=0.01)
    _check(hip_ctx, packed, [0, 5, 10, 29], 0.01, 300)


@pytest.mark.parametrize("remove_com", [True, False])
def test_unwrap_with_face_crossings(hip_ctx, remove_com):
    packed = _gas_walk(64, 100, np.diag([5.0, 6.0, 7.0]), [1] * 40 + [8] * 24, 0.6, 13)
    windows = np.array([0, 1, 4, 10, 49], dtype=np.int32)
    got = hip_ctx.vanhove_window(packed, windows, 0.05, 120, unwrap=True, remove_com=remove_com)
    want = ref.vanhove(packed, windows, 0.05, 120, unwrap=True, remove_com=remove_com)
    _compare(got, want, len(packed), windows, packed.numbers)
    assert want[1][:, -1].sum() > 0            # unwrapped displacements beyond the half cell: overflow is exercised
    assert hip_ctx.last_path() == "msd_vanhove"


def test_wrapped_steps_without_the_centre_of_mass(hip_ctx):
    # (the columns of the shared builder with neither unwrap nor a centre of mass, whole system and an atom range)
    packed = _gas_walk(64, 100, np.diag([5.0, 6.0, 7.0]), [1] * 40 + [8] * 24, 0.6, 13)
    windows = np.array([0, 1, 4, 10, 49], dtype=np.int32)
    for atom_range in (None, (9, 52)):
        got = hip_ctx.vanhove_window(packed, windows, 0.05, 120, remove_com=False, atom_range=atom_range)
        want = ref.vanhove(packed, windows, 0.05, 120, remove_com=False, atom_range=atom_range)
        sel = packed.numbers if atom_range is None else np.asarray(packed.numbers)[atom_range[0]:atom_range[1]]
        _compare(got, want, len(packed), windows, sel)
    assert hip_ctx.last_path() == "msd_vanhove"


def test_ragged_shapes_and_a_single_atom_species(hip_ctx):
    # F prime, N not a multiple of the 8-atom workgroup block, one Zn atom, unsorted windows incl. the last frame
    numbers = [30] + [7] * 17 + [6] * 19
    packed = _gas_walk(37, 211, np.diag([7.3, 8.1, 6.7]), numbers, 0.2, 14)
    _check(hip_ctx, packed, [17, 0, 210, 1, 104, 5, 63, 2, 9, 33, 150], 0.03, 111)
    assert hip_ctx.last_path() == "msd_vanhove"
    # more bins than a multi-lag tile holds (one lag per workgroup)
    _check(hip_ctx, packed, [0, 1, 50], 0.0002, 20000)
    assert hip_ctx.last_path() == "msd_vanhove"
    # no bins at all: everything overflows, the moments are unchanged
    _check(hip_ctx, packed, [0, 3], 0.05, 0)


def test_global_counters(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 50, 0.05, 15, ortho=True)
    windows = [0, 2, 7, 24]
    # dr = 0.001 over 40 A: 40 000 bins, beyond the LDS
    _check(hip_ctx, packed, windows, 0.001, 40000)
    assert hip_ctx.last_path() == "msd_vanhove_global"
    with _env(AMOF_VANHOVE_GLOBAL="1"):
        got = _check(hip_ctx, packed, windows, 0.01, _half_cell_bins(packed, 0.01))
        assert hip_ctx.last_path() == "msd_vanhove_global"
    lds = hip_ctx.vanhove_window(packed, np.array(windows, np.int32), 0.01, _half_cell_bins(packed, 0.01))
    assert np.array_equal(lds[0], got[0]) and np.array_equal(lds[1], got[1])


def test_device_resident_input_is_identical(hip_ctx):
    import torch
    packed = H.random_walk(H.zif4_frame(), 70, 0.05, 16)
    windows = np.array([0, 3, 10, 34], dtype=np.int32)
    host = hip_ctx.vanhove_window(packed, windows, 0.01, 500)
    dev = packed.to_device(0)
    res = hip_ctx.vanhove_window(dev, windows, 0.01, 500)
    for a, b in zip(host[:3], res[:3]):
        assert np.array_equal(a, b)
    # device outputs, added into
    S = len(host[3])
    out = (torch.zeros((S, 4, 500), dtype=torch.int64, device="cuda:0"), torch.zeros((S, 4), dtype=torch.int64, device="cuda:0"),
           torch.zeros((S, 4, 2), dtype=torch.float64, device="cuda:0"))
    hip_ctx.vanhove_window(dev, windows, 0.01, 500, out=out)
    hip_ctx.vanhove_window(dev, windows, 0.01, 500, out=out)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint64), 2 * host[0])
    assert np.array_equal(out[1].cpu().numpy().view(np.uint64), 2 * host[1])
    np.testing.assert_allclose(out[2].cpu().numpy(), 2 * host[2], rtol=1e-15)
    # a centre of mass handed in (amof_msd_com_dev) gives the same result
    com = torch.zeros((70, 3), dtype=torch.float64, device="cuda:0")
    hip_ctx.msd_com(dev, (0, 70), com)
    out2 = hip_ctx.vanhove_window(dev, windows, 0.01, 500, com=com)
    assert np.array_equal(out2[0].cpu().numpy().view(np.uint64), host[0])
    np.testing.assert_allclose(out2[2].cpu().numpy(), host[2], rtol=1e-13)


def test_second_moment_ties_to_the_window_msd(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 100, 0.05, 17)
    windows, _ = no.msd_window_setup(100, delta_time=5)
    for unwrap in (False, True):
        _, _, moments, kinds = hip_ctx.vanhove_window(packed, windows, 0.01, 300, unwrap=unwrap)
        sumsq, k2 = hip_ctx.msd_window(packed, windows, unwrap=unwrap)
        assert list(k2) == list(kinds)
        np.testing.assert_allclose(moments[:, :, 0], sumsq, rtol=1e-9, atol=1e-12)


def test_atom_halves_add_up_to_the_whole(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 90, 0.05, 18)
    windows = np.array([0, 4, 9, 44], dtype=np.int32)
    N = packed.n_atoms
    whole = hip_ctx.vanhove_window(packed, windows, 0.01, 400)
    a = hip_ctx.vanhove_window(packed, windows, 0.01, 400, atom_range=(0, N // 2 + 3))
    b = hip_ctx.vanhove_window(packed, windows, 0.01, 400, atom_range=(N // 2 + 3, N))
    assert np.array_equal(a[0] + b[0], whole[0]) and np.array_equal(a[1] + b[1], whole[1])
    np.testing.assert_allclose(a[2] + b[2], whole[2], rtol=1e-12)
    _check(hip_ctx, packed, windows, 0.01, 400, atom_range=(5, 101))
    # two contexts of one device sharding the atoms (MultiContext)
    from amof_amd import _hip
    multi = _hip.MultiContext([0, 0])
    try:
        m = multi.vanhove_window(packed, windows, 0.01, 400)
    finally:
        multi.close()
    assert np.array_equal(m[0], whole[0]) and np.array_equal(m[1], whole[1])
    np.testing.assert_allclose(m[2], whole[2], rtol=1e-12)


def test_two_identical_calls_are_bit_identical(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 80, 0.05, 19)
    windows = np.array([0, 1, 5, 13, 39], dtype=np.int32)
    for env in ({}, {"AMOF_VANHOVE_GLOBAL": "1"}):
        with _env(**env):
            a = hip_ctx.vanhove_window(packed, windows, 0.01, 600)
            hip_ctx.debug_poison()
            b = hip_ctx.vanhove_window(packed, windows, 0.01, 600)
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))


def test_class_schema_and_ties_to_window_msd(tmp_path):
    from amof_amd.msd import WindowMsd
    from amof_amd.vanhove import WindowVanHove
    packed = H.random_walk(H.zif4_frame(), 60, 0.05, 20)
    vh = WindowVanHove.from_trajectory(packed, delta_time=4, timestep=1, dr=0.02)
    msd = WindowMsd.from_trajectory(packed, delta_time=4, timestep=1)
    nbins = _half_cell_bins(packed, 0.02)
    elements = [int(z) for z in packed.unique_numbers()]
    from amof_amd import data as _data
    names = [_data.chemical_symbols[int(z)] for z in elements]
    assert list(vh.data.columns) == ["Time", "r"] + names + ["X"]
    assert list(vh.alpha2.columns) == ["Time"] + names + ["X"]
    W = len(msd.data)
    assert len(vh.data) == W * nbins
    np.testing.assert_array_equal(vh.alpha2["Time"].values, msd.data["Time"].values)
    np.testing.assert_array_equal(vh.data["Time"].values, np.repeat(msd.data["Time"].values, nbins))
    assert np.isnan(vh.alpha2.iloc[0, 1:].values.astype(float)).all()
    assert np.isfinite(vh.alpha2.iloc[1:, 1:].values.astype(float)).all()
    # the second moment reproduces WindowMsd
    F = len(packed)
    window = msd.data["Time"].values
    for z, name in zip(elements, names):
        s = vh.kinds.index(int(z))
        n_s = int((packed.numbers == z).sum())
        np.testing.assert_allclose(vh.sum2[s] / n_s / (F - window), msd.data[name].values, rtol=1e-9, atol=1e-12)
    # P integrates to one minus the overflow fraction
    for z, name in zip(elements, names):
        s = vh.kinds.index(int(z))
        n = (packed.numbers == z).sum() * (F - window - 1)
        P = vh.data[name].values.reshape(W, nbins)
        np.testing.assert_allclose(P.sum(axis=1) * 0.02, 1.0 - vh.overflow[s] / n, rtol=1e-12)
    # numeric rmax is not clamped to the cell
    wide = WindowVanHove.from_trajectory(packed, delta_time=4, timestep=1, dr=0.5, rmax=100.0)
    assert len(wide.data) == W * 200
    vh.write_to_file(os.path.join(str(tmp_path), "z"))
    back = WindowVanHove.from_file(os.path.join(str(tmp_path), "z"))
    assert back.data.equals(vh.data)
    # no window: the columns, no rows
    empty = WindowVanHove.from_trajectory(packed, delta_time=4, timestep=1, max_time=0)
    assert list(empty.data.columns) == ["Time", "r"] + names + ["X"] and len(empty.data) == 0


def _run_vh(distributed):
    from amof_amd.vanhove import WindowVanHove
    import torch
    packed = H.device_walk(torch.device("cuda", 0), (1, 1, 2), 64, 0.05, 21)     # same seed on every rank
    vh = WindowVanHove.from_trajectory(packed, delta_time=8, timestep=1, dr=0.02, device=0, distributed=distributed)
    host = H.random_walk(H.zif4_frame(), 40, 0.05, 22)
    vh2 = WindowVanHove.from_trajectory(host, delta_time=4, timestep=1, dr=0.02, unwrap=True, device=0, distributed=distributed)
    return {"data": vh.data.values, "alpha2": vh.alpha2.values, "counts": np.asarray(vh.counts), "data_u": vh2.data.values,
            "counts_u": np.asarray(vh2.counts)}


def _worker_vh(rank, world, port, out_dir, backend):
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
    res = _run_vh(None)
    for k, arr in res.items():
        np.save(os.path.join(out_dir, "%s_rank%d.npy" % (k, rank)), arr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_equal_single_process(tmp_path, backend, world):
    """atoms sharded over the ranks (two gloo ranks on cuda:0; one RCCL rank with every collective run: the device-resident
    path with the frame-sharded centre of mass); integer counts identical to the single process, moments to float order"""
    import torch.multiprocessing as mp
    port = 31600 + (os.getpid() + world) % 2000
    mp.spawn(_worker_vh, args=(world, port, str(tmp_path), backend), nprocs=world, join=True)
    single = _run_vh(False)
    for k, want in single.items():
        for rank in range(world):
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            if k.startswith("counts") or k.startswith("data"):
                assert np.array_equal(got, want), k
            else:
                np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-15)
