"""F(q, t) on the GPU (amof_isf_accumulate[_dev], IntermediateScattering): bit for bit against the library's own rho table,
the t = 0 identities with S(q), the float64 restatement (tests/isf_ref.py) within S(q)'s tolerance, a known answer of the
self part, and the invariances integer sums give."""

import os
import sys

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import intermediate_scattering as isc
from amof_amd import structure_factor as sf
from amof_amd.frames import Frame, PackedTrajectory
from tests import helpers as H
from tests import isf_ref as ref
from tests import sq_ref
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

TOL = 1e-5          # tests/test_gpu_sq.py: the project's S(q) contract


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


def _dev_call(ctx, packed, hkl, windows, dq, nbins, flat=None, self_part=True, **kw):
    """the `_dev` form into one int64 tensor: ({counts, beyond, coh, self} as int64 numpy, scale_log2, the tensor)"""
    import torch
    S, W = len(H.species_of(packed.numbers)[0]), len(windows)
    lay = _hip.isf_layout(S, W, nbins, self_part)
    if flat is None:
        flat = torch.zeros(lay["size"], dtype=torch.int64, device="cuda:0")
    _, scale, kinds = ctx.isf_accumulate(packed, hkl, windows, dq, nbins, self_part=self_part, out=flat, **kw)
    a = flat.cpu().numpy()
    n = W * nbins
    out = {"counts": a[:n].reshape(W, nbins), "beyond": a[lay["beyond"]:lay["beyond"] + W],
           "coh": a[lay["coh"]:lay["coh"] + S * S * n].reshape(S, S, W, nbins)}
    if self_part:
        out["self"] = a[lay["self"]:].reshape(S, W, nbins)
    return out, scale, flat


def _same_bits(a, b):
    """two host-form results (counts, coh, self, beyond, kinds) with identical bits"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and list(a[4]) == list(b[4])
    assert np.array_equal(a[1].view(np.uint64), b[1].view(np.uint64))
    assert (a[2] is None) == (b[2] is None)
    if a[2] is not None:
        assert np.array_equal(a[2].view(np.uint64), b[2].view(np.uint64))


def _bins_of(packed, hkl, dq, nbins):
    return np.array([sq_ref.bins(r, hkl, dq, nbins) for r in _hip.reciprocal(packed.cell)])


# ------------------------------------------------------------------------------------- 1: bit-exact against rho --
@pytest.mark.parametrize("jitter,stride", [(0.0, 1), (0.02, 1), (0.0, 3)])
def test_integer_sums_equal_the_correlation_of_the_librarys_own_modes(hip_ctx, jitter, stride):
    packed = H.random_walk(H.zif4_frame(), 12, 0.05, 31, cell_jitter=jitter)
    hkl = sf.enumerate_hkl(packed.cell, 2.5)
    dq, nbins = 0.03, sf.n_bins(2.5, 0.03)
    windows = [0, 1, 2, 5]
    got, scale, _ = _dev_call(hip_ctx, packed, hkl, windows, dq, nbins, origin_stride=stride)
    assert hip_ctx.last_path() == "isf"
    rho = np.array([hip_ctx.sq_modes(packed, hkl, frame=f)[0] for f in range(len(packed))])
    counts, coh, beyond = ref.isf_from_modes(rho, _bins_of(packed, hkl, dq, nbins), scale, windows, nbins, origin_stride=stride)
    assert counts.sum() > 0 and (counts.sum(axis=1) > 0).all()
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["beyond"], beyond)
    assert np.array_equal(got["coh"], coh)
    if jitter:
        assert beyond.sum() > 0          # the superset reaches beyond qmax in some frames


# ------------------------------------------------------------------------------------------ 2: t = 0 identities --
@pytest.mark.parametrize("stride", [1, 2])
def test_lag_zero_is_the_structure_factor_bit_for_bit(hip_ctx, stride):
    import torch
    packed = H.random_walk(H.zif4_frame(), 9, 0.05, 32, cell_jitter=0.01)
    F = len(packed)
    hkl = sf.enumerate_hkl(packed.cell[1::stride], 2.0)
    dq, nbins = 0.04, sf.n_bins(2.0, 0.04)
    windows = [3, 0]                    # lag 0 is not the first window
    got, scale, _ = _dev_call(hip_ctx, packed, hkl, windows, dq, nbins, origin_stride=stride)
    S = got["coh"].shape[0]
    P = S * (S + 1) // 2
    out = (torch.zeros(nbins + 1, dtype=torch.int64, device="cuda:0"), torch.zeros((P, nbins), dtype=torch.int64, device="cuda:0"))
    c, s, sq_scale, _ = hip_ctx.sq_accumulate(packed, hkl, dq, nbins, frame_range=(1, F), frame_stride=stride, out=out)
    c, s = c.cpu().numpy(), s.cpu().numpy()
    assert np.array_equal(scale, sq_scale)
    assert np.array_equal(got["counts"][1], c[:nbins]) and got["beyond"][1] == c[nbins]
    p = 0
    for a in range(S):
        for d in range(a, S):
            assert np.array_equal(got["coh"][a, d, 1], s[p]) and np.array_equal(got["coh"][d, a, 1], s[p])
            p += 1
    # self at lag 0: cos(0) is exact, the sum is N_a counts up to the fixed-point quantum (<= 2^-20 in S units)
    kinds, sp = H.species_of(packed.numbers)
    n = np.array([(sp == a).sum() for a in range(S)], dtype=np.float64)
    ok = got["counts"][1] > 0
    assert ok.any()
    for a in range(S):
        v = np.ldexp(got["self"][a, 1].astype(np.float64), -int(ref.pair_scale(scale, S)[a, a]))
        assert np.abs(v[ok] / (got["counts"][1][ok] * n[a]) - 1.0).max() <= 2.0 ** -20

    # the class against StructureFactor over the origin frames
    f = isc.IntermediateScattering.from_trajectory(packed, delta_time=3, dq=dq, qmax=2.0, origin_stride=stride, device=0,
                                                   distributed=False)
    s0 = sf.StructureFactor.from_trajectory(packed, dq=dq, qmax=2.0, first_frame=1, frame_stride=stride, device=0, distributed=False)
    assert f.window[0] == 0 and np.array_equal(f.hkl, s0.hkl)
    assert np.array_equal(np.asarray(f.counts)[0], np.asarray(s0.counts))
    t0 = f.data.iloc[:nbins]
    for name in s0.data.columns:
        np.testing.assert_allclose(t0[name].values, s0.data[name].values, rtol=1e-12, equal_nan=True)


# -------------------------------------------------------------------------------------------- 3: against float64 --
def _compare(got, want, numbers, windows):
    counts, coh, selfs, beyond, kinds = got
    c_ref, coh_ref, self_ref, b_ref, k_ref = want
    assert list(kinds) == list(k_ref)
    assert np.array_equal(np.asarray(counts, dtype=np.int64), c_ref) and np.array_equal(np.asarray(beyond, dtype=np.int64), b_ref)
    w0 = list(windows).index(0)
    numbers = np.asarray(numbers)
    n = np.array([(numbers == z).sum() for z in kinds], dtype=np.float64)
    assert (c_ref.sum(axis=1) > 0).all(), "a lag without a non-empty bin"
    worst = {"coh": 0.0, "self": 0.0}
    for w in range(len(windows)):
        ok = c_ref[w] > 0
        assert (c_ref[w0][ok] > 0).all()
        cw = c_ref[w][ok].astype(np.float64)
        c0 = c_ref[w0][ok].astype(np.float64)
        for a in range(len(kinds)):
            s_aa = coh_ref[a, a, w0][ok] / (c0 * n[a])
            e = np.abs(selfs[a, w][ok] - self_ref[a, w][ok]) / (cw * n[a])
            worst["self"] = max(worst["self"], float(e.max()))
            for c in range(len(kinds)):
                s_cc = coh_ref[c, c, w0][ok] / (c0 * n[c])
                e = np.abs(coh[a, c, w][ok] - coh_ref[a, c, w][ok]) / (cw * np.sqrt(n[a] * n[c]))
                worst["coh"] = max(worst["coh"], float((e / np.maximum(1.0, np.sqrt(s_aa * s_cc))).max()))
    print("F(q, t) against float64: coherent %.3g (of %g max(1, sqrt(S_aa S_cc))), self %.3g (of %g)"
          % (worst["coh"], TOL, worst["self"], TOL))
    assert worst["coh"] <= TOL and worst["self"] <= TOL


def _check(ctx, packed, hkl, windows, dq, nbins, **kw):
    got = ctx.isf_accumulate(packed, hkl, windows, dq, nbins, **kw)
    want = ref.isf(packed, hkl, windows, dq, nbins, origin_stride=kw.get("origin_stride", 1))
    _compare(got, want, packed.numbers, windows)
    return got


def test_zif4_walk_against_float64(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 10, 0.05, 33)
    _check(hip_ctx, packed, sf.enumerate_hkl(packed.cell, 3.0), [0, 1, 4], 0.02, sf.n_bins(3.0, 0.02))
    assert hip_ctx.last_path() == "isf"


def test_sheared_supercell_against_float64(hip_ctx):
    base = H.zif4_frame()
    sheared = np.array(base.cell, dtype=float)
    sheared[1] += 0.2 * sheared[0]
    sheared[2] += -0.15 * sheared[0] + 0.1 * sheared[1]
    frac = np.linalg.solve(np.asarray(base.cell).T, base.positions.T).T
    rep = H.replicate(Frame(base.numbers, frac @ sheared, sheared, base.pbc), (2, 2, 2))
    packed = H.random_walk(rep, 4, 0.05, 34)
    _check(hip_ctx, packed, sf.enumerate_hkl(packed.cell, 1.6), [0, 1, 2], 0.05, sf.n_bins(1.6, 0.05))


def test_ragged_shapes_against_float64(hip_ctx):
    rng = np.random.default_rng(35)
    numbers = [30] + [7] * 40 + [6] * 36              # N = 77, a one-atom species
    cell = np.array([[11.0, 0.0, 0.0], [1.0, 12.5, 0.0], [0.5, -1.0, 10.3]])
    packed = PackedTrajectory((rng.random((5, 77, 3)) @ cell), cell, numbers)
    _check(hip_ctx, packed, sf.enumerate_hkl(packed.cell, 3.3), [0, 2, 3], 0.07, sf.n_bins(3.3, 0.07))
    # an arbitrary vector list: unsorted, duplicates, broken rows
    odd = np.array([[0, 0, 3], [1, -2, 4], [0, 0, 3], [5, 5, 5], [1, -2, 6], [1, -2, 5], [0, 1, -9]])
    _check(hip_ctx, packed, odd, [0, 1], 0.1, 40, origin_stride=2)
    # N = 20 000, 4 frames, small K
    big = H.random_gas(20000, [60.0, 61.0, 62.0], [8] * 5000 + [1] * 15000, 10, F=4)
    _check(hip_ctx, big, sf.enumerate_hkl(big.cell, 0.6), [0, 1, 2], 0.05, sf.n_bins(0.6, 0.05))


# ------------------------------------------------------------------------------------------ 4: self known answer --
def test_self_part_of_a_uniformly_shifted_lattice(hip_ctx):
    """8^3 simple-cubic lattice, every atom shifted by f a1 / 4 per frame: the phase differences are exact multiples of
    2^30, so self / N = cos(2 pi h m / 4); phases are periodic, so wrapped, unwrapped and cell-shifted input agree bit for bit"""
    cell = np.diag([16.0, 16.0, 16.0])
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) / 8.0
    F, N = 7, 512
    pos = (g @ cell)[None] + np.arange(F)[:, None, None] * (cell[0] / 4.0)[None, None, :]
    hkl = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 1, 0], [2, 1, 1], [5, 2, 0]])
    dq, nbins = 0.05, 50
    b = sq_ref.bins(sq_ref.reciprocal(cell), hkl, dq, nbins)
    assert len(set(b.tolist())) == len(hkl) and (b < nbins).all()
    windows = [0, 1, 2, 3]
    unwrapped = PackedTrajectory(pos, cell, [29] * N)
    got = hip_ctx.isf_accumulate(unwrapped, hkl, windows, dq, nbins)
    for w, m in enumerate(windows):
        n_w = F - m - 1
        assert (got[0][w][b] == n_w).all()
        np.testing.assert_allclose(got[2][0, w][b] / (n_w * N), np.cos(2 * np.pi * hkl[:, 0] * m / 4.0), atol=1e-6)
    wrapped = PackedTrajectory(pos % 16.0, cell, [29] * N)
    rng = np.random.default_rng(36)
    moved = PackedTrajectory(pos + rng.integers(-3, 4, size=(F, N, 3)) @ cell, cell, [29] * N)
    for other in (wrapped, moved):
        _same_bits(hip_ctx.isf_accumulate(other, hkl, windows, dq, nbins), got)


# ----------------------------------------------------------------------------------------------- 5: invariances --
def test_invariances_bit_for_bit(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 10, 0.05, 37, cell_jitter=0.01)
    hkl = sf.enumerate_hkl(packed.cell, 2.5)
    dq, nbins = 0.03, sf.n_bins(2.5, 0.03)
    windows = [0, 1, 3, 4]
    host = hip_ctx.isf_accumulate(packed, hkl, windows, dq, nbins)
    assert hip_ctx.last_path() == "isf"
    one_chunk = hip_ctx.last_kernel_launches()
    stages = hip_ctx.last_stage_seconds()
    assert stages["rho"] > 0 and stages["corr"] > 0 and stages["self"] > 0
    dev = packed.to_device(0)
    on_dev = hip_ctx.isf_accumulate(dev, hkl, windows, dq, nbins)
    hip_ctx.debug_poison()
    again = hip_ctx.isf_accumulate(dev, hkl, windows, dq, nbins)
    _same_bits(on_dev, host)
    _same_bits(again, host)
    # global counters on request
    with _env(AMOF_ISF_GLOBAL="1"):
        glo = hip_ctx.isf_accumulate(dev, hkl, windows, dq, nbins)
        assert hip_ctx.last_path() == "isf_global"
    _same_bits(glo, host)
    # several vector chunks: 9 touched frames x 4 species x 16 B = 576 B per vector, 40 vectors per chunk
    assert len(hkl) > 200
    with _env(AMOF_ISF_RHO_BUDGET=str(576 * 40)):
        chunked = hip_ctx.isf_accumulate(dev, hkl, windows, dq, nbins)
        assert hip_ctx.last_kernel_launches() >= 3 * one_chunk
    _same_bits(chunked, host)
    # without the self part: the same coherent sums, no difference kernels
    plain = hip_ctx.isf_accumulate(dev, hkl, windows, dq, nbins, self_part=False)
    assert plain[2] is None and hip_ctx.last_stage_seconds()["self"] == 0.0
    assert np.array_equal(plain[0], host[0]) and np.array_equal(plain[1].view(np.uint64), host[1].view(np.uint64))
    # the work range split in two calls into the same device buffers == one call == the host form
    whole, scale, _ = _dev_call(hip_ctx, dev, hkl, windows, dq, nbins)
    total = int(sum(len(ref.origins(len(packed), m)) for m in windows))
    cut = total // 2 + 1                # inside a lag
    _, scale_a, flat = _dev_call(hip_ctx, dev, hkl, windows, dq, nbins, work_range=(0, cut))
    halves, scale_b, _ = _dev_call(hip_ctx, dev, hkl, windows, dq, nbins, flat=flat, work_range=(cut, total))
    assert np.array_equal(scale, scale_a) and np.array_equal(scale, scale_b)
    for k in whole:
        assert np.array_equal(whole[k], halves[k]), k
    S = whole["coh"].shape[0]
    exp2 = ref.pair_scale(scale, S)
    assert np.array_equal(np.ldexp(whole["coh"].astype(np.float64), -exp2[:, :, None, None]).view(np.uint64), host[1].view(np.uint64))
    assert np.array_equal(np.ldexp(whole["self"].astype(np.float64), -np.diag(exp2)[:, None, None]).view(np.uint64),
                          host[2].view(np.uint64))
    assert np.array_equal(whole["counts"].view(np.uint64), host[0]) and np.array_equal(whole["beyond"].view(np.uint64), host[3])


@pytest.mark.parametrize("F", [11, 12])
def test_work_list_cut_at_lag_boundaries(hip_ctx, F):
    """three species, 71 atoms, lags [0, 2, 5], every second origin (F = 11: 5, 4 and 3 origins per lag; F = 12: 6, 5 and
    3): the work list cut exactly on the first lag boundary, an empty piece there (it must add nothing to the device
    tensor), a cut inside the second lag, the rest -- added into one tensor, equal to the single full call bit for bit"""
    from amof_amd import lags
    windows, stride, dq, qmax = [0, 2, 5], 2, 0.1, 1.3
    numbers = np.repeat([1, 6, 30], [31, 24, 16])
    gas = H.random_gas(len(numbers), [11.3, 12.1, 13.7], numbers, 51)
    packed = H.random_walk(Frame(numbers, gas.pos[0], gas.cell[0], (True, True, True)), F, 0.2, 52, ortho=True)
    hkl = sf.enumerate_hkl(packed.cell, qmax)
    assert 24 <= len(hkl) <= 60
    nbins = sf.n_bins(qmax, dq)
    n = lags.n_origins(F, windows, stride)
    total = int(n.sum())
    cuts = [(0, int(n[0])), (int(n[0]), int(n[0])), (int(n[0]), int(n[0]) + 2), (int(n[0]) + 2, total)]
    if F == 11:
        assert n.tolist() == [5, 4, 3] and cuts == [(0, 5), (5, 5), (5, 7), (7, 12)]
    whole, scale, _ = _dev_call(hip_ctx, packed, hkl, windows, dq, nbins, origin_stride=stride)
    assert whole["counts"].sum() > 0 and np.abs(whole["coh"]).sum() > 0 and np.abs(whole["self"]).sum() > 0
    flat, snap = None, []
    for c in cuts:
        pieces, scale_c, flat = _dev_call(hip_ctx, packed, hkl, windows, dq, nbins, flat=flat, origin_stride=stride, work_range=c)
        assert np.array_equal(scale_c, scale)
        snap.append(flat.cpu().numpy().copy())
    assert np.array_equal(snap[1], snap[0]) and not np.array_equal(snap[2], snap[1])        # the empty piece added nothing
    assert pieces["counts"][1:].sum() > 0 and snap[0].reshape(-1)[nbins:3 * nbins].sum() == 0   # piece 0 ends with lag 0
    for k in whole:
        assert np.array_equal(whole[k], pieces[k]), k


def test_more_bins_than_the_lds_budget_take_global_counters(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 6, 0.05, 38)
    hkl = sf.enumerate_hkl(packed.cell, 2.4)
    windows = [0, 2]
    fine = hip_ctx.isf_accumulate(packed, hkl, windows, 0.004, 600)         # (1 + 16) 600 u64 > 64 KB
    assert hip_ctx.last_path() == "isf_global"
    coarse = hip_ctx.isf_accumulate(packed, hkl, windows, 0.04, 60)
    assert hip_ctx.last_path() == "isf"
    assert np.array_equal(fine[0].reshape(2, 60, 10).sum(axis=2), coarse[0])
    _compare(fine, ref.isf(packed, hkl, windows, 0.004, 600), packed.numbers, windows)


# ------------------------------------------------------------------------------------------------------ 6: class --
def test_class_schema(tmp_path):
    from amof_amd import data as _data
    packed = H.random_walk(H.zif4_frame(), 10, 0.05, 39)
    f = isc.IntermediateScattering.from_trajectory(packed, delta_time=2, dq=0.05, qmax=2.0, device=0, distributed=False)
    names = [_data.chemical_symbols[int(z)] for z in packed.unique_numbers()]
    assert list(f.data.columns) == (["Time", "q", "X-X"] + [a + "-" + b for a in names for b in names] +
                                    [a + "-self" for a in names] + ["X-self"])
    nbins = sf.n_bins(2.0, 0.05)
    assert f.window.tolist() == [0, 2, 4] and len(f.data) == 3 * nbins
    np.testing.assert_array_equal(f.data["Time"].values, np.repeat([0.0, 2.0, 4.0], nbins))
    np.testing.assert_array_equal(f.data["q"].values, np.tile(np.arange(nbins) * 0.05, 3))
    assert f.n_origins.tolist() == [9, 7, 5] and np.asarray(f.counts).shape == (3, nbins)
    want = ref.isf(packed, f.hkl, [0, 2, 4], 0.05, nbins)
    _compare((f.counts, f.coh, f.self_sums, f.beyond, f.kinds), want, packed.numbers, [0, 2, 4])
    ok = (np.asarray(f.counts) > 0).reshape(-1)
    assert np.isnan(f.data["X-X"].values[~ok]).all() and np.isfinite(f.data.values[ok]).all()
    w = f.weighted({z: 1.0 for z in packed.unique_numbers()})
    np.testing.assert_allclose(w["F"].values[ok], f.data["X-X"].values[ok], rtol=1e-12)
    nrm = f.normalised()
    assert np.abs(nrm["X-self"].values[:nbins][ok[:nbins]] - 1.0).max() == 0.0
    f.write_to_file(os.path.join(str(tmp_path), "z"))
    assert isc.IntermediateScattering.from_file(os.path.join(str(tmp_path), "z")).data.equals(f.data)
    # without the self part: no self columns, the same coherent columns
    ctx = _hip.lane_context(0, 0)
    g = isc.IntermediateScattering.from_trajectory(packed, delta_time=2, dq=0.05, qmax=2.0, self_part=False, device=0,
                                                   distributed=False)
    assert list(g.data.columns) == list(f.data.columns)[:3 + len(names) ** 2] and g.self_sums is None
    assert ctx.last_stage_seconds()["self"] == 0.0
    assert g.data.equals(f.data[list(g.data.columns)])


def _run_isf(distributed):
    import torch
    packed = H.device_walk(torch.device("cuda", 0), (1, 1, 2), 9, 0.05, 41)     # same seed on every rank
    f = isc.IntermediateScattering.from_trajectory(packed, delta_time=2, dq=0.04, qmax=2.0, device=0, distributed=distributed)
    host = H.random_walk(H.zif4_frame(), 8, 0.05, 42, cell_jitter=0.01)
    g = isc.IntermediateScattering.from_trajectory(host, delta_time=1, dq=0.04, qmax=2.0, origin_stride=2, device=0,
                                                   distributed=distributed)
    return {"data": f.data.values, "counts": np.asarray(f.counts), "coh": f.coh, "self": f.self_sums,
            "data_npt": g.data.values, "coh_npt": g.coh, "self_npt": g.self_sums, "beyond_npt": np.asarray(g.beyond)}


def _worker_isf(rank, world, port, out_dir, backend):
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
    res = _run_isf(None)
    for k, arr in res.items():
        np.save(os.path.join(out_dir, "%s_rank%d.npy" % (k, rank)), arr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_equal_single_process(tmp_path, backend, world):
    """the (lag, origin) work list shared over the ranks (two gloo ranks on cuda:0; one RCCL rank with every collective run):
    the integer fixed-point sums add up exactly, so every output is identical to the single process"""
    import torch.multiprocessing as mp
    port = 34600 + (os.getpid() + world) % 2000
    mp.spawn(_worker_isf, args=(world, port, str(tmp_path), backend), nprocs=world, join=True)
    single = _run_isf(False)
    for k, want in single.items():
        for rank in range(world):
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            assert np.array_equal(got, want, equal_nan=True), k


# ----------------------------------------------------------------------------------------------------- 7: errors --
def test_argument_errors(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 5, 0.05, 43)
    hkl = np.array([[1, 0, 0], [0, 2, 1]])

    def code(fn):
        with pytest.raises(ValueError):         # (how the binding raises AMOF_EINVAL)
            fn()
        return _hip.AMOF_EINVAL
    open_cell = PackedTrajectory(packed.pos_host(), packed.cell, packed.numbers, pbc=(True, True, False))
    assert code(lambda: hip_ctx.isf_accumulate(open_cell, hkl, [0, 1], 0.1, 20)) == _hip.AMOF_EINVAL
    assert code(lambda: hip_ctx.isf_accumulate(packed, hkl, [0, 1], 0.1, 20, origin_stride=0)) == _hip.AMOF_EINVAL
    assert code(lambda: hip_ctx.isf_accumulate(packed, hkl, [0, 5], 0.1, 20)) == _hip.AMOF_EINVAL            # lag >= F
    assert code(lambda: hip_ctx.isf_accumulate(packed, hkl, [0, -1], 0.1, 20)) == _hip.AMOF_EINVAL
    assert code(lambda: hip_ctx.isf_accumulate(packed, [[1, 0, 0], [0, 0, 0]], [0, 1], 0.1, 20)) == _hip.AMOF_EINVAL
    assert code(lambda: hip_ctx.isf_accumulate(packed, hkl, [0, 1], 0.1, 20, work_range=(0, 8))) == _hip.AMOF_EINVAL   # 4 + 3 entries
    assert code(lambda: hip_ctx.isf_accumulate(packed, hkl, [0, 1], 0.1, 20, work_range=(5, 4))) == _hip.AMOF_EINVAL
    assert code(lambda: hip_ctx.isf_accumulate(packed, hkl, [0, 1], 0.0, 20)) == _hip.AMOF_EINVAL
    # an empty range is fine and gives zeros
    got = hip_ctx.isf_accumulate(packed, hkl, [0, 1], 0.1, 20, work_range=(3, 3))
    assert got[0].sum() == 0 and not got[1].any() and got[3].sum() == 0
    with pytest.raises(ValueError):
        isc.IntermediateScattering.from_trajectory(open_cell, delta_time=1, device=0, distributed=False)
    with pytest.raises(ValueError):
        isc.IntermediateScattering.from_trajectory(packed, delta_time=1, origin_stride=0, device=0, distributed=False)


def test_capacity_surfaces_as_a_value_error(hip_ctx):
    """every vector in one bin over a long trajectory: the fixed-point quantum would exceed 2^-20 (AMOF_ECAPACITY); the class
    names the remedies instead of cutting the trajectory (chunks of frames would cut the lags)"""
    import torch
    N, F = 1024, 4200
    rng = np.random.default_rng(44)
    frame = torch.tensor(rng.random((N, 3)) * 12.0, dtype=torch.float64, device="cuda:0")
    packed = PackedTrajectory(frame.expand(F, N, 3).contiguous(), np.diag([12.0, 12.0, 12.0]), [8] * N)
    r = np.arange(-80, 81, dtype=np.int32)
    t = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    hkl = np.ascontiguousarray(t[sf.half_space(t)])
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.isf_accumulate(packed, hkl, [0], 1000.0, 1, work_range=(0, 1))
    assert err.value.code == _hip.AMOF_ECAPACITY
    with pytest.raises(ValueError, match="max_points"):
        # one bin with every vector up to 55 / Angstrom (2.4 million): the same overflow through the class
        isc.IntermediateScattering.from_trajectory(packed, delta_time=1000, dq=50.0, qmax=55.0, device=0, distributed=False).data
