"""S(q) on the GPU (amof_sq_accumulate, amof_sq_modes, StructureFactor) against the float64 restatement (tests/sq_ref.py):
counts and beyond equal, every S column within 1e-5 max(1, |S_ref|)."""

import os
import sys

import numpy as np
import pytest

from amof_amd import structure_factor as sf
from amof_amd.frames import PackedTrajectory
from tests import helpers as H
from tests import sq_exact_ref as exact
from tests import sq_ref as ref
from tests.conftest import ROOT
from tests.sq_accuracy_cases import TERM_ERR     # the measured error of one v_cos_f32 / v_sin_f32 term

pytestmark = pytest.mark.gpu

TOL = 1e-5


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


def _compare_s(got, want, numbers):
    counts, sums, beyond, kinds = got
    c_ref, s_ref, b_ref, k_ref = want
    assert list(kinds) == list(k_ref)
    assert np.array_equal(np.asarray(counts, dtype=np.int64), c_ref) and int(beyond) == b_ref
    a = ref.normalised(np.asarray(counts, dtype=np.int64), sums, kinds, numbers)
    b = ref.normalised(c_ref, s_ref, k_ref, numbers)
    ok = c_ref > 0
    assert np.array_equal(np.isnan(a), np.isnan(b))
    err = np.abs(a[:, ok] - b[:, ok]) / np.maximum(1.0, np.abs(b[:, ok]))
    assert err.max() <= TOL, "S off by %.3g (relative)" % err.max()


def _check(ctx, packed, hkl, dq, nbins, frames=None, **kw):
    got = ctx.sq_accumulate(packed, hkl, dq, nbins, **kw)
    want = ref.sq(packed, hkl, dq, nbins, frames=frames)
    _compare_s(got, want, packed.numbers)
    return got


def _hkl(packed, qmax, dq=None, max_points=None):
    return sf.enumerate_hkl(packed.cell, qmax, dq=dq, max_points=max_points)


def _lattice(cell):
    g = (np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) / 8.0)
    return PackedTrajectory((g @ cell)[None], cell, [29] * 512)


def test_exact_known_answer_of_a_simple_cubic_lattice(hip_ctx):
    r = np.arange(-9, 10)
    hkl = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    hkl = hkl[np.abs(hkl).sum(axis=1) > 0]
    bragg = (hkl % 8 == 0).all(axis=1)
    for cell in (np.diag([16.0, 16.0, 16.0]), np.array([[16.0, 0.0, 0.0], [8.0, 16.0, 0.0], [-4.0, 2.0, 32.0]])):
        rho, kinds = sf.density_modes(_lattice(cell), hkl, device=0)
        assert kinds == [29] and rho.shape == (len(hkl), 1)
        assert (rho[bragg, 0] == 512.0).all()                     # every u a multiple of 2^29: exact phases, exact sum
        bound = exact.budget(512, hkl[~bragg], TERM_ERR, True)     # the derived budget of the f32 chain, per component ...
        assert (np.abs(rho[~bragg, 0].real) <= bound).all() and (np.abs(rho[~bragg, 0].imag) <= bound).all()
        assert np.abs(rho[~bragg, 0]).max() <= 1e-3               # ... (8 partials of 64: 9.9e-4 + 512 TERM_ERR) and the earlier bound
        assert hip_ctx.last_path() == "sq_modes"


def test_modes_match_the_restatement(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 3, 0.05, 3)
    hkl = np.array([[1, 0, 0], [0, 0, 1], [3, -2, 5], [-4, 1, 0], [0, 7, -7], [12, 11, -10], [1, 2, 3], [1, 2, 4]])
    kinds, sp = H.species_of(packed.numbers)
    for f in (0, 2):
        rho, k = hip_ctx.sq_modes(packed, hkl, frame=f)
        want = ref.modes(packed.pos_host()[f], packed.cell[0], sp, len(kinds), hkl)
        assert list(k) == kinds
        for a in range(len(kinds)):         # per species and component: the derived budget of the f32 chain
            bound = exact.budget(int((sp == a).sum()), hkl, TERM_ERR, False)
            assert (np.abs((rho - want)[:, a].real) <= bound).all() and (np.abs((rho - want)[:, a].imag) <= bound).all()
            assert bound.max() < 2e-4 * np.sqrt(packed.n_atoms)


def test_zif4_walk_and_a_sheared_supercell(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 20, 0.05, 4)
    _check(hip_ctx, packed, _hkl(packed, 3.0), 0.02, sf.n_bins(3.0, 0.02))
    assert hip_ctx.last_path() == "sq"
    base = H.zif4_frame()
    sheared = np.array(base.cell, dtype=float)
    sheared[1] += 0.2 * sheared[0]
    sheared[2] += -0.15 * sheared[0] + 0.1 * sheared[1]
    frac = np.linalg.solve(np.asarray(base.cell).T, base.positions.T).T
    from amof_amd.frames import Frame
    rep = H.replicate(Frame(base.numbers, frac @ sheared, sheared, base.pbc), (2, 2, 2))
    packed = H.random_walk(rep, 2, 0.05, 5)
    _check(hip_ctx, packed, _hkl(packed, 1.6), 0.05, sf.n_bins(1.6, 0.05))


def test_npt_bins_per_frame(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 12, 0.05, 6, cell_jitter=0.02)
    hkl = sf.enumerate_hkl(packed.cell, 2.5)
    got = _check(hip_ctx, packed, hkl, 0.03, sf.n_bins(2.5, 0.03))
    assert got[2] > 0            # the superset reaches beyond qmax in some frames


def test_unwrapped_and_shifted_input(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 6, 0.05, 7)
    hkl = _hkl(packed, 2.5)
    nb = sf.n_bins(2.5, 0.03)
    folded = hip_ctx.sq_accumulate(packed, hkl, 0.03, nb)
    rng = np.random.default_rng(8)
    shift = rng.integers(-3, 4, size=(len(packed), packed.n_atoms, 3)) @ packed.cell[0]
    moved = PackedTrajectory(packed.pos_host() + shift, packed.cell, packed.numbers)
    got = hip_ctx.sq_accumulate(moved, hkl, 0.03, nb)
    _compare_s(got, folded, packed.numbers)
    unwrapped = H.random_walk(H.zif4_frame(), 6, 0.05, 7, wrap=False)
    _check(hip_ctx, unwrapped, hkl, 0.03, nb)


def test_ragged_shapes(hip_ctx):
    rng = np.random.default_rng(9)
    numbers = [30] + [7] * 40 + [6] * 36              # N = 77, a one-atom species
    cell = np.array([[11.0, 0.0, 0.0], [1.0, 12.5, 0.0], [0.5, -1.0, 10.3]])
    packed = PackedTrajectory((rng.random((3, 77, 3)) @ cell), cell, numbers)
    hkl = _hkl(packed, 3.3)
    _check(hip_ctx, packed, hkl, 0.07, sf.n_bins(3.3, 0.07))
    # an arbitrary vector list: unsorted, duplicates, broken rows
    odd = np.array([[0, 0, 3], [1, -2, 4], [0, 0, 3], [5, 5, 5], [1, -2, 6], [1, -2, 5], [0, 1, -9]])
    _check(hip_ctx, packed, odd, 0.1, 40)
    # a frame beyond the LDS capacity of a frame-in-LDS design: N = 20 000, 2 frames, small K
    big = H.random_gas(20000, [60.0, 61.0, 62.0], [8] * 5000 + [1] * 15000, 10, F=2)
    _check(hip_ctx, big, sf.enumerate_hkl(big.cell, 0.6), 0.05, sf.n_bins(0.6, 0.05))


def test_global_counters_equal_the_lds_variant(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 5, 0.05, 11)
    hkl = _hkl(packed, 2.5)
    lds = hip_ctx.sq_accumulate(packed, hkl, 0.01, 250)
    assert hip_ctx.last_path() == "sq"
    with _env(AMOF_SQ_GLOBAL="1"):
        glo = _check(hip_ctx, packed, hkl, 0.01, 250)
        assert hip_ctx.last_path() == "sq_bin_global"
    assert np.array_equal(lds[0], glo[0]) and np.array_equal(lds[1].view(np.uint64), glo[1].view(np.uint64)) and lds[2] == glo[2]
    # more bins than the LDS budget: the global kernel by itself
    _check(hip_ctx, packed, hkl, 0.0002, 12500)
    assert hip_ctx.last_path() == "sq_bin_global"


def test_device_input_determinism_and_frame_halves(hip_ctx):
    import torch
    packed = H.random_walk(H.zif4_frame(), 10, 0.05, 12)
    hkl = _hkl(packed, 2.5)
    nb = sf.n_bins(2.5, 0.03)
    host = hip_ctx.sq_accumulate(packed, hkl, 0.03, nb)
    dev = packed.to_device(0)
    on_dev = hip_ctx.sq_accumulate(dev, hkl, 0.03, nb)
    hip_ctx.debug_poison()
    again = hip_ctx.sq_accumulate(dev, hkl, 0.03, nb)
    for x in (on_dev, again):
        assert np.array_equal(x[0], host[0]) and np.array_equal(x[1].view(np.uint64), host[1].view(np.uint64)) and x[2] == host[2]
    # frame halves into the same device buffers: fixed-point sums identical to the whole call
    S = len(host[3])
    P = S * (S + 1) // 2

    def fresh():
        return (torch.zeros(nb + 1, dtype=torch.int64, device="cuda:0"), torch.zeros((P, nb), dtype=torch.int64, device="cuda:0"))
    whole = hip_ctx.sq_accumulate(dev, hkl, 0.03, nb, out=fresh())
    halves = fresh()
    hip_ctx.sq_accumulate(dev, hkl, 0.03, nb, frame_range=(0, 4), out=halves)
    _, _, scale, _ = hip_ctx.sq_accumulate(dev, hkl, 0.03, nb, frame_range=(4, 10), out=halves)
    assert np.array_equal(scale, whole[2])
    assert torch.equal(halves[0], whole[0]) and torch.equal(halves[1], whole[1])
    sums = np.ldexp(whole[1].cpu().numpy().astype(np.float64), -whole[2].astype(np.int64)[:, None])
    assert np.array_equal(sums.view(np.uint64), host[1].view(np.uint64))
    assert np.array_equal(whole[0].cpu().numpy()[:nb].view(np.uint64), host[0]) and int(whole[0][nb]) == host[2]
    # host calls of the halves add up: counts exactly
    a = hip_ctx.sq_accumulate(packed, hkl, 0.03, nb, frame_range=(0, 4))
    b = hip_ctx.sq_accumulate(packed, hkl, 0.03, nb, frame_range=(4, 10))
    assert np.array_equal(a[0] + b[0], host[0]) and a[2] + b[2] == host[2]
    np.testing.assert_allclose(a[1] + b[1], host[1], rtol=1e-12, atol=1e-9)
    # frame stride
    _check(hip_ctx, packed, hkl, 0.03, nb, frames=range(1, 10, 3), frame_range=(1, 10), frame_stride=3)


def test_class_schema(tmp_path):
    from amof_amd import data as _data
    packed = H.random_walk(H.zif4_frame(), 8, 0.05, 13)
    s = sf.StructureFactor.from_trajectory(packed, dq=0.05, qmax=2.0, device=0)
    names = [_data.chemical_symbols[int(z)] for z in packed.unique_numbers()]
    assert list(s.data.columns) == ["q", "X-X"] + [a + "-" + b for a in names for b in names]
    assert len(s.data) == sf.n_bins(2.0, 0.05)
    np.testing.assert_array_equal(s.data["q"].values, np.arange(len(s.data)) * 0.05)
    want = ref.sq(packed, s.hkl, 0.05, len(s.data))
    assert np.array_equal(np.asarray(s.counts, dtype=np.int64), want[0]) and s.beyond == want[2]
    # X-X = sum over ordered pairs of sqrt(c_a c_b) S_ab (Ashcroft-Langreth)
    n = packed.species_counts()
    N = packed.n_atoms
    xx = sum(np.sqrt(n[int(a)] * n[int(b)]) / N * s.data[_data.chemical_symbols[int(a)] + "-" + _data.chemical_symbols[int(b)]].values
             for a in packed.unique_numbers() for b in packed.unique_numbers())
    ok = np.asarray(s.counts) > 0
    np.testing.assert_allclose(xx[ok], s.data["X-X"].values[ok], rtol=1e-10)
    assert np.isnan(s.data["X-X"].values[~ok]).all()
    w = s.weighted({z: 1.0 for z in packed.unique_numbers()})
    np.testing.assert_allclose(w["S"].values[ok], s.data["X-X"].values[ok], rtol=1e-12)
    # frame_stride and frame selection
    t = sf.StructureFactor.from_trajectory(packed, dq=0.05, qmax=2.0, first_frame=1, last_frame=7, frame_stride=2, device=0)
    want = ref.sq(packed, t.hkl, 0.05, len(t.data), frames=[1, 3, 5])
    _compare_s((t.counts, t.sums, t.beyond, t.kinds), want, packed.numbers)
    # subsampled vectors
    u = sf.StructureFactor.from_trajectory(packed, dq=0.05, qmax=2.0, max_points=4, device=0)
    assert np.asarray(u.counts).max() <= 4 * len(packed) and len(u.hkl) < len(s.hkl)
    s.write_to_file(os.path.join(str(tmp_path), "z"))
    assert sf.StructureFactor.from_file(os.path.join(str(tmp_path), "z")).data.equals(s.data)


def _run_sq(distributed):
    import torch
    packed = H.device_walk(torch.device("cuda", 0), (1, 1, 2), 9, 0.05, 21)     # same seed on every rank
    s = sf.StructureFactor.from_trajectory(packed, dq=0.04, qmax=2.0, device=0, distributed=distributed)
    host = H.random_walk(H.zif4_frame(), 7, 0.05, 22, cell_jitter=0.01)
    s2 = sf.StructureFactor.from_trajectory(host, dq=0.04, qmax=2.0, frame_stride=2, device=0, distributed=distributed)
    return {"data": s.data.values, "counts": np.asarray(s.counts), "sums": s.sums, "data_npt": s2.data.values,
            "sums_npt": s2.sums, "beyond_npt": np.array([s2.beyond])}


def _worker_sq(rank, world, port, out_dir, backend):
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
    res = _run_sq(None)
    for k, arr in res.items():
        np.save(os.path.join(out_dir, "%s_rank%d.npy" % (k, rank)), arr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_equal_single_process(tmp_path, backend, world):
    """frames sharded over the ranks (two gloo ranks on cuda:0; one RCCL rank with every collective run): the integer
    fixed-point sums add up exactly, so every output is identical to the single process"""
    import torch.multiprocessing as mp
    port = 32600 + (os.getpid() + world) % 2000
    mp.spawn(_worker_sq, args=(world, port, str(tmp_path), backend), nprocs=world, join=True)
    single = _run_sq(False)
    for k, want in single.items():
        for rank in range(world):
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            assert np.array_equal(got, want, equal_nan=True), k


def _gas_cube(N, L, F, seed, device):
    """N atoms of one species in an L-Angstrom cube, the same positions in each of F frames (device-resident)"""
    import torch
    rng = np.random.default_rng(seed)
    frame = torch.tensor(rng.random((N, 3)) * L, dtype=torch.float64, device=device)
    return PackedTrajectory(frame.expand(F, N, 3).contiguous(), np.diag([L, L, L]), [8] * N)


def _half_cube(n):
    r = np.arange(-n, n + 1, dtype=np.int32)
    t = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    return np.ascontiguousarray(t[sf.half_space(t)])


def test_scale_is_bounded_by_the_busiest_bin(hip_ctx):
    """the fixed-point scale follows the largest per-bin vector count, not the whole list: a shape that a bound by
    F * K refuses (quantum above 2^-20) runs, and frame 0 of the long trajectory equals the one-frame trajectory"""
    N, F = 2048, 2500
    packed = _gas_cube(N, 16.0, F, 20, "cuda:0")
    hkl = _half_cube(60)                                     # 885 780 vectors, |q| up to 40 / A
    K, dq, nbins = len(hkl), 0.25, 80                        # bins up to 20 / A: ~10^4 vectors in the busiest bin
    e = np.frexp(float(F) * K * (N * N + 0.5))[1]
    assert 2.0 ** -(62 - e) / N > 2.0 ** -20                 # what a bound by F * K would have refused
    got = hip_ctx.sq_accumulate(packed, hkl, dq, nbins, frame_range=(0, 1))
    one = PackedTrajectory(packed.pos[:1].contiguous(), packed.cell, packed.numbers)
    want = hip_ctx.sq_accumulate(one, hkl, dq, nbins)
    assert 0 < want[0].max() < K // 50
    assert np.array_equal(got[0], want[0]) and got[2] == want[2]
    _compare_s(got, (want[0].astype(np.int64), want[1], want[2], want[3]), packed.numbers)


def test_chunks_beyond_the_fixed_point_range(hip_ctx):
    """every vector in one bin: even the per-bin bound exceeds the fixed-point range for the whole trajectory
    (AMOF_ECAPACITY); the class's fallback accumulates sub-trajectories of the selected frames and adds them"""
    from amof_amd import _hip
    N, F = 1024, 2100
    packed = _gas_cube(N, 12.0, F, 21, "cuda:0")
    hkl = _half_cube(80)                                     # 2 091 440 vectors
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.sq_accumulate(packed, hkl, 1000.0, 1, frame_range=(0, 1))
    assert err.value.code == _hip.AMOF_ECAPACITY
    got = sf.accumulate_in_chunks(hip_ctx, packed, hkl, 1000.0, 1, (0, F), 1050)       # frames 0 and 1050
    two = PackedTrajectory(packed.pos[::1050].contiguous(), packed.cell, packed.numbers)
    want = hip_ctx.sq_accumulate(two, hkl, 1000.0, 1)
    assert int(got[0][0]) == 2 * len(hkl) and np.array_equal(got[0], want[0]) and got[2] == want[2] == 0
    _compare_s(got, (want[0].astype(np.int64), want[1], want[2], want[3]), packed.numbers)


def test_multi_context_equals_one_context(hip_ctx):
    from amof_amd import _hip
    packed = H.random_walk(H.zif4_frame(), 9, 0.05, 23, cell_jitter=0.01)
    hkl = sf.enumerate_hkl(packed.cell, 2.0)
    nb = sf.n_bins(2.0, 0.04)
    multi = _hip.MultiContext([0, 0])
    try:
        for fr, st in (((0, 9), 1), ((1, 9), 3)):
            one = hip_ctx.sq_accumulate(packed, hkl, 0.04, nb, frame_range=fr, frame_stride=st)
            m = multi.sq_accumulate(packed, hkl, 0.04, nb, frame_range=fr, frame_stride=st)
            assert np.array_equal(m[0], one[0]) and m[2] == one[2] and list(m[3]) == list(one[3])
            np.testing.assert_allclose(m[1], one[1], rtol=1e-12, atol=1e-9)
        dev = packed.to_device(0)
        m = multi.sq_accumulate(dev, hkl, 0.04, nb)
        one = hip_ctx.sq_accumulate(dev, hkl, 0.04, nb)
        assert np.array_equal(m[0], one[0]) and m[2] == one[2]
        np.testing.assert_allclose(m[1], one[1], rtol=1e-12, atol=1e-9)
    finally:
        multi.close()
