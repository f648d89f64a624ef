"""C_L(q, t) and C_T(q, t) on the GPU (amof_current_modes, amof_current_accumulate[_dev], CurrentCorrelation): the modes
within the derived budget of tests/current_exact_ref.py, the integer sums bit for bit against a host correlation of the
library's own modes, known answers of a plane wave, continuity against the density kernel, the invariances integer sums give,
the velocity mode, the class and the ranks."""

import functools
import math
import os
import sys

import numpy as np
import pytest

from amof_amd import _hip
from amof_amd import current_correlation as cc
from amof_amd import structure_factor as sf
from amof_amd.frames import PackedTrajectory
from tests import current_exact_ref as CX
from tests import current_ref as ref
from tests import helpers as H
from tests import isf_ref
from tests import sq_exact_ref as X
from tests import sq_ref
from tests.conftest import ROOT
from tests.sq_accuracy_cases import TERM_ERR
from tests.test_gpu_vacf import TRICLINIC, _env, _gas_walk

pytestmark = pytest.mark.gpu

R = 4       # CUR_RUN (tests/test_current_plan_cpu.py pins it to the header)
# rows whose runs have length 1, R and R + 1, an unsorted tail with a duplicate: appended to the half space
ODD_ROWS = np.array([[7, 7, 1]] + [[7, 8, l] for l in range(2, 2 + R)] + [[8, 7, l] for l in range(-2, -2 + R + 1)] +
                    [[1, -2, 6], [1, -2, 4], [1, -2, 6]])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(PackedTrajectory, hkl, u32 coordinates)"""
    if name == "mixed":         # six species of 1, 63, 64, 65, 129 and 300 atoms (the f32 partial straddled), triclinic
        numbers = np.repeat([1, 6, 7, 8, 29, 30], [1, 63, 64, 65, 129, 300])
        np.random.default_rng(2).shuffle(numbers)
        packed = _gas_walk(numbers, 8, TRICLINIC, 0.04, 61)
        qmax = 4.0
    elif name == "five":        # five species
        packed = _gas_walk(np.repeat([1, 6, 7, 8, 30], [20, 30, 9, 40, 17]), 7, TRICLINIC, 0.04, 62)
        qmax = 3.0
    elif name == "npt":         # a cell per frame, four species
        packed = H.random_walk(H.zif4_frame(), 9, 0.04, 63, cell_jitter=0.01)
        qmax = 1.6
    elif name == "zif4":
        packed = H.random_walk(H.zif4_frame(), 12, 0.04, 64)
        qmax = 1.6
    elif name == "three":       # three species, a diagonal cell
        packed = _gas_walk(np.repeat([1, 8, 14], [33, 64, 21]), 6, np.diag([7.0, 8.0, 9.0]), 0.04, 65)
        qmax = 2.5
    elif name == "two":
        packed = _gas_walk(np.repeat([8, 14], [70, 35]), 6, np.diag([7.0, 8.0, 9.0]), 0.04, 66)
        qmax = 2.5
    hkl = np.vstack([sf.enumerate_hkl(packed.cell, qmax), ODD_ROWS]).astype(np.int32)
    assert len(hkl) % (64 * R) != 0
    return packed, hkl, ref.quantized(packed)


def _dev_call(ctx, packed, hkl, windows, dq, nbins, flat=None, **kw):
    """the `_dev` form into one int64 tensor: ({counts, beyond, long, trans} as int64 numpy, scale_log2, vmax, the tensor)"""
    import torch
    S, W = len(H.species_of(packed.numbers)[0]), len(windows)
    lay = _hip.current_layout(S, W, nbins)
    if flat is None:
        flat = torch.zeros(lay["size"], dtype=torch.int64, device="cuda:0")
    _, scale, vmax, kinds = ctx.current_accumulate(packed, hkl, windows, dq, nbins, out=flat, **kw)
    a = flat.cpu().numpy()
    n = W * nbins
    out = {"counts": a[:n].reshape(W, nbins), "beyond": a[lay["beyond"]:lay["beyond"] + W],
           "long": a[lay["long"]:lay["long"] + S * S * n].reshape(S, S, W, nbins),
           "trans": a[lay["trans"]:lay["trans"] + S * S * n].reshape(S, S, W, nbins)}
    return out, scale, vmax, flat


def _same_bits(a, b):
    """two host-form results with identical bits"""
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[3], b[3]) and np.array_equal(a[4], b[4]) and a[5] == b[5]
    assert list(a[6]) == list(b[6])
    for x in (1, 2):
        assert np.array_equal(a[x].view(np.uint64), b[x].view(np.uint64))


def _library_modes(ctx, packed, hkl, **kw):
    F = len(packed)
    S = len(H.species_of(packed.numbers)[0])
    jm = np.zeros((F, len(hkl), S, 3), dtype=np.complex128)
    for f in range(1, F):
        jm[f] = ctx.current_modes(packed, hkl, frame=f, **kw)[0]
    return jm


# ------------------------------------------------------------------------------------- 1: modes within the budget --
@pytest.mark.parametrize("name", ["mixed", "npt", "five"])
def test_modes_within_the_derived_budget(hip_ctx, name):
    packed, hkl, u = _case(name)
    kinds, species = H.species_of(packed.numbers)
    _, w, p = ref.samples(packed, u=u)
    worst = 0.0
    for f in (1, 2, len(packed) - 1):
        got, k = hip_ctx.current_modes(packed, hkl, frame=f)
        assert list(k) == kinds
        want = ref.modes(p[f], w[f], species, len(kinds), hkl)
        b = CX.budget(w[f], species, len(kinds), hkl, cell=ref._cell_of(packed, f))
        assert np.abs(want).max() > 100 * b.max()           # the budget is far below the signal
        frac = max(float((np.abs(got.real - want.real) / b).max()), float((np.abs(got.imag - want.imag) / b).max()))
        worst = max(worst, frac)
    print("current modes %s: worst error %.3f of the budget" % (name, worst))
    assert worst <= 1.0


# ------------------------------------------------------------------------------ 2: integer sums, bit for bit --
@pytest.mark.parametrize("name,stride", [("zif4", 1), ("npt", 1), ("npt", 2), ("mixed", 1), ("five", 2), ("three", 1), ("two", 2)])
def test_integer_sums_equal_the_correlation_of_the_librarys_own_modes(hip_ctx, name, stride):
    packed, hkl, _ = _case(name)
    dq, nbins = 0.05, 40
    windows = [0, 1, 3]
    got, scale, vmax, _ = _dev_call(hip_ctx, packed, hkl, windows, dq, nbins, origin_stride=stride)
    assert hip_ctx.last_path() == "current" and vmax > 0
    jm = _library_modes(hip_ctx, packed, hkl)
    counts, lng, trn, beyond = ref.correlate(jm, ref._recips(packed), hkl, windows, dq, nbins, stride, scale_log2=scale)
    assert counts.sum() > 0 and beyond.sum() > 0 and np.abs(lng).sum() > 0 and np.abs(trn).sum() > 0
    assert np.array_equal(got["counts"], counts) and np.array_equal(got["beyond"], beyond)
    assert np.array_equal(got["long"], lng)
    assert np.array_equal(got["trans"], trn)


# ------------------------------------------------------------------------------------------- 3: known answers --
CELL_W = np.diag([16.0, 18.0, 17.0])      # K = (0, 1, 0) is the shortest vector, alone in its bin
AMP, PERIOD = 0.02, 8


@functools.lru_cache(maxsize=None)
def _wave(polarisation, F=12):
    """the 8^3 lattice of 512 atoms (Z = 29) in the diagonal cell, displaced by AMP e^ cos(K . r0 - omega f), K = (0, 1, 0):
    (trajectory, omega, |K|, c = 2 A sin(omega / 2))"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) / 8.0
    r0 = (g + 0.013) @ CELL_W
    omega, kk = 2.0 * np.pi / PERIOD, 2.0 * np.pi / 18.0
    e = np.array([1.0, 0.0, 0.0]) if polarisation == "transverse" else np.array([0.0, 1.0, 0.0])
    theta = 2.0 * np.pi * g[:, 1]
    disp = AMP * np.cos(theta[None, :] - omega * np.arange(F)[:, None])
    pos = r0[None] + disp[:, :, None] * e[None, None, :]
    return PackedTrajectory(pos, CELL_W, [29] * 512), omega, kk, 2.0 * AMP * np.sin(omega / 2.0)


def _product_error(amp, d):
    """the error of Re(x conj y) for |x|, |y| <= amp whose real and imaginary parts are each known to d"""
    return 2.0 * amp * np.sqrt(2.0) * d + 2.0 * d * d


def _harmonic(n, eps):
    """bound on the amplitude of j(n K) of the longitudinal wave in units of c N / 2: sum over p = -(n + 1), -(n - 1) (mod 8)
    of (n eps / 2)^|p| / |p|! >= |J_p(n eps)| (|s| <= 4: the terms beyond are below 1e-40)"""
    x = n * eps / 2.0
    return sum(x ** abs(p) / math.factorial(abs(p)) for r in (n + 1, n - 1) for p in (-r + 8 * s for s in range(-4, 5)))


@pytest.mark.parametrize("polarisation", ["transverse", "longitudinal"])
def test_plane_wave_known_answer(hip_ctx, polarisation):
    """Transverse (e^ = x, K along y), vectors (0, k, l): v_x = c sin(theta - omega (f - 1/2)), the phase position does not
    move, j_x(K) = -(N / 2i) c e^{i omega tau} up to a constant phase: trans / counts / N = (c^2 N / 4) cos(omega m) in the
    bin of K, 0 elsewhere, and k^_x = 0 exactly: long is exactly 0.  Longitudinal (e^ = y), vectors (0, k, 0): the midpoint
    moves by eps cos(psi), eps = |K| A cos(omega / 2), and by the Jacobi-Anger expansion the amplitude is 2 J_1(eps) / eps =
    1 - eps^2 / 8 + ..: the product deviates by at most eps^2 / 4 relative (derived, not chosen); T = j - k^ (k^ . j) is
    exactly 0 for k^ = y and j_x = j_z = 0.  The moving midpoint also feeds the harmonics n K: their amplitude is c N / 2 times
    the sum of |J_p(n eps)| over the orders p = -(n + 1) and -(n - 1) modulo 8 (eight lattice planes along K alias the orders
    8 apart), each at most (n eps / 2)^|p| / |p|!: _harmonic."""
    packed, omega, kk, c = _wave(polarisation)
    N = 512
    if polarisation == "transverse":
        hkl = np.array([[0, k, l] for k in range(-3, 4) for l in range(0, 4) if (l > 0 or k > 0)], dtype=np.int32)
    else:
        hkl = np.array([[0, k, 0] for k in range(1, 6)], dtype=np.int32)
    dq, nbins = 0.004, 500
    rec = ref._recips(packed)[0]
    b = sq_ref.bins(rec, hkl, dq, nbins)
    iK = int(np.flatnonzero((hkl == [0, 1, 0]).all(axis=1))[0])
    assert (b < nbins).all() and (b == b[iK]).sum() == 1            # K alone in its bin
    windows = [0, 1, 3]
    counts, lng, trn, beyond, scale, vmax, kinds = hip_ctx.current_accumulate(packed, hkl, windows, dq, nbins)
    zero, wave = (lng, trn) if polarisation == "transverse" else (trn, lng)
    assert not zero.any() and beyond.sum() == 0
    # the budget of item 1 for the largest sample (|w| <= c: the budget grows with |w|), through the projection.  The known
    # answer is stated for the true positions, the library sees them truncated to the u32 grid: two units of 2^-32 of the
    # longest cell vector on every step, and one more quant() on every phase
    kinds_, species = H.species_of(packed.numbers)
    w = np.zeros((N, 3), dtype=np.float32)
    w[:, 0 if polarisation == "transverse" else 1] = c
    dl, dt = CX.projected(CX.budget(w, species, 1, hkl, cell=CELL_W))
    d = float(max(dl.max(), dt.max())) + N * 2 * 2.0 ** -32 * 18.0 + c * N * float(X.quant(hkl).max())
    quantum = 0.5 * 2.0 ** -float(scale[0])
    amp = c * N / 2.0
    eps = kk * AMP * np.cos(omega / 2.0)
    rel = 0.0 if polarisation == "transverse" else eps * eps / 4.0
    # in the bin of K: one component of amplitude amp known to d (real and imaginary parts), two of magnitude below sqrt(2) d;
    # elsewhere all three are below sqrt(2) d
    tol_k = (_product_error(amp, d) + 4 * d * d + quantum) / N + rel * c * c * N / 4.0
    for wi, m in enumerate(windows):
        n_w = len(packed) - m - 1
        assert counts[wi][b[iK]] == n_w and (counts[wi][b] % n_w == 0).all()
        got = wave[0, 0, wi] / (np.where(counts[wi] > 0, counts[wi], 1) * N)
        want = (c * c * N / 4.0) * np.cos(omega * m)
        print("%s wave, lag %d: %.9g against %.9g (tolerance %.3g)" % (polarisation, m, got[b[iK]], want, tol_k))
        assert abs(got[b[iK]] - want) <= tol_k
        for i in np.flatnonzero(b != b[iK]):
            n = int(hkl[i, 1])
            # one component of magnitude at most the harmonic's amplitude plus sqrt(2) d, two below sqrt(2) d (a bin's value is
            # a mean over its vectors)
            a_h = 0.0 if polarisation == "transverse" else _harmonic(n, eps) * amp
            assert abs(got[b[i]]) <= ((a_h + np.sqrt(2.0) * d) ** 2 + 4 * d * d + quantum) / N, (m, hkl[i])
    assert tol_k <= (1e-4 + rel) * c * c * N / 4.0            # the check resolves the answer


# ----------------------------------------------------------------------- 4: continuity against the density kernel --
def test_continuity_against_the_density_kernel(hip_ctx):
    """rho(k, f) - rho(k, f - 1) = sum_j e^{i k r_mid} 2 i sin(k . d_j / 2), so |k| L(k, f) + i (rho(f) - rho(f - 1)) is at most
    sum_j |k . d_j|^3 / 24, plus both kernels' budgets (the current's times |k|)."""
    numbers = np.repeat([8, 14], [65, 40])
    cell = np.diag([9.0, 10.0, 11.0])
    packed = _gas_walk(numbers, 4, cell, 0.004, 71)
    hkl = sf.enumerate_hkl(packed.cell, 1.5).astype(np.int32)
    kinds, species = H.species_of(packed.numbers)
    u = ref.quantized(packed)
    v, w, p = ref.samples(packed, remove_com=False, u=u)
    rec = ref._recips(packed)[0]
    kvec = hkl.astype(np.float64) @ rec
    knorm = np.linalg.norm(kvec, axis=1)
    for f in (1, 3):
        kd = kvec @ v[f].T                                          # [K][N]
        assert np.abs(kd).max() <= 0.05
        j, _ = hip_ctx.current_modes(packed, hkl, frame=f, remove_com=False)
        L, _ = ref.project(j, ref.khat(rec, hkl))
        rho1, _ = hip_ctx.sq_modes(packed, hkl, frame=f)
        rho0, _ = hip_ctx.sq_modes(packed, hkl, frame=f - 1)
        diff = knorm[:, None] * L + 1j * (rho1 - rho0)
        dl, _ = CX.projected(CX.budget(w[f], species, len(kinds), hkl, cell=cell))
        worst = 0.0
        for a in range(len(kinds)):
            n = int((species == a).sum())
            bound = (np.abs(kd[:, species == a]) ** 3).sum(axis=1) / 24.0 + knorm * dl[:, a] + 2.0 * X.budget(n, hkl, TERM_ERR, False)
            worst = max(worst, float((np.abs(diff[:, a].real) / bound).max()), float((np.abs(diff[:, a].imag) / bound).max()))
            assert np.abs(knorm * np.abs(L[:, a])).max() > 50 * bound.max()
        print("continuity, frame %d: worst %.3f of the bound" % (f, worst))
        assert worst <= 1.0


# ----------------------------------------------------------------------------------------------- 5: invariances --
def test_invariances_bit_for_bit(hip_ctx):
    packed, hkl, _ = _case("npt")
    dq, nbins = 0.05, 40
    windows = [0, 1, 3]
    host = hip_ctx.current_accumulate(packed, hkl, windows, dq, nbins)
    assert hip_ctx.last_path() == "current"
    one_chunk = hip_ctx.last_kernel_launches()
    stages = hip_ctx.last_current_stage_seconds()
    assert stages["records"] > 0 and stages["table"] > 0 and stages["corr"] > 0
    dev = packed.to_device(0)
    on_dev = hip_ctx.current_accumulate(dev, hkl, windows, dq, nbins)
    hip_ctx.debug_poison()
    again = hip_ctx.current_accumulate(dev, hkl, windows, dq, nbins)
    _same_bits(on_dev, host)
    _same_bits(again, host)
    # permuted vector order: the same sums (the bins are a function of the vector)
    perm = np.random.default_rng(5).permutation(len(hkl))
    _same_bits(hip_ctx.current_accumulate(dev, hkl[perm], windows, dq, nbins), host)
    jp, _ = hip_ctx.current_modes(dev, hkl[perm], frame=2)
    j0, _ = hip_ctx.current_modes(dev, hkl, frame=2)
    assert np.array_equal(jp.view(np.float64).view(np.uint64), j0[perm].view(np.float64).view(np.uint64))
    with _env(AMOF_CURRENT_GLOBAL="1"):
        glo = hip_ctx.current_accumulate(dev, hkl, windows, dq, nbins)
        assert hip_ctx.last_path() == "current_global"
    _same_bits(glo, host)
    # several vector chunks: 8 touched frames x 4 species x 48 B per vector, 30 vectors per chunk
    slots = len(packed) - 1
    assert len(hkl) > 100
    with _env(AMOF_CURRENT_RHO_BUDGET=str(slots * 4 * 48 * 30)):
        chunked = hip_ctx.current_accumulate(dev, hkl, windows, dq, nbins)
        assert hip_ctx.last_kernel_launches() >= 3 * one_chunk
    _same_bits(chunked, host)
    # the work range split into the same device buffers == one call == the host form, at the same scale
    whole, scale, vmax, _ = _dev_call(hip_ctx, dev, hkl, windows, dq, nbins)
    from amof_amd import lags
    n = lags.n_origins(len(packed), windows, 1)
    total = int(n.sum())
    flat, snaps = None, []
    for cut in [(0, int(n[0])), (int(n[0]), int(n[0])), (int(n[0]), int(n[0]) + 2), (int(n[0]) + 2, total)]:
        pieces, scale_c, vmax_c, flat = _dev_call(hip_ctx, dev, hkl, windows, dq, nbins, flat=flat, work_range=cut)
        assert np.array_equal(scale_c, scale) and vmax_c == vmax
        snaps.append(flat.cpu().numpy().copy())
    assert np.array_equal(snaps[1], snaps[0]) and not np.array_equal(snaps[2], snaps[1])    # the empty piece added nothing
    for k in whole:
        assert np.array_equal(whole[k], pieces[k]), k
    exp2 = isf_ref.pair_scale(scale, whole["long"].shape[0])
    assert np.array_equal(np.ldexp(whole["long"].astype(np.float64), -exp2[:, :, None, None]).view(np.uint64), host[1].view(np.uint64))
    assert np.array_equal(np.ldexp(whole["trans"].astype(np.float64), -exp2[:, :, None, None]).view(np.uint64), host[2].view(np.uint64))
    assert np.array_equal(whole["counts"].view(np.uint64), host[0]) and np.array_equal(scale, host[4]) and vmax == host[5]


def test_more_bins_than_the_lds_budget_take_global_counters(hip_ctx):
    packed, hkl, _ = _case("zif4")
    windows = [0, 2]
    fine = hip_ctx.current_accumulate(packed, hkl, windows, 0.005, 400)         # (1 + 32) 400 u64 > 64 KB
    assert hip_ctx.last_path() == "current_global"
    coarse = hip_ctx.current_accumulate(packed, hkl, windows, 0.05, 40)
    assert hip_ctx.last_path() == "current"
    assert np.array_equal(fine[0].reshape(2, 40, 10).sum(axis=2), coarse[0]) and fine[5] == coarse[5]
    for x in (1, 2):        # the same samples in finer bins at that call's own scale: equal up to half a quantum per sample
        np.testing.assert_allclose(fine[x].reshape(4, 4, 2, 40, 10).sum(axis=4), coarse[x], rtol=1e-12,
                                   atol=float(coarse[0].max()) * 2.0 ** -float(min(coarse[4].min(), fine[4].min())))


def test_a_trajectory_at_rest_gives_zero_sums_and_scale(hip_ctx):
    base = H.zif4_frame()
    packed = PackedTrajectory(np.repeat(base.positions[None], 5, axis=0), base.cell, base.numbers)
    hkl = sf.enumerate_hkl(packed.cell, 1.2)
    counts, lng, trn, beyond, scale, vmax, _ = hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.05, 24)
    assert vmax == 0.0 and not scale.any() and not lng.any() and not trn.any() and counts.sum() > 0


# ----------------------------------------------------------------------------------------------- 6: velocity mode --
def _sum_bound(jm_ref, dl, dt, recips, hkl, windows, dq, nbins, stride, quantum):
    """[S][S][W][nbins] bounds on |library - reference| of the long and of the trans sums: the mode budgets (dl [F][K][S],
    dt [F][K][S][3] on real and imaginary parts) through the products, summed over the samples of every bin, plus half a
    quantum per sample"""
    F, K, S, _ = jm_ref.shape
    W = len(windows)
    rec = lambda f: recips[f if len(recips) > 1 else 0]
    bl, bt = np.zeros((S, S, W, nbins)), np.zeros((S, S, W, nbins))
    r2 = np.sqrt(2.0)
    for wi, k in isf_ref.work_entries(F, windows, stride):
        m = int(windows[wi])
        b = sq_ref.bins(rec(k), hkl, dq, nbins)
        ok = b < nbins
        L0, T0 = ref.project(jm_ref[k], ref.khat(rec(k), hkl))
        L1, T1 = ref.project(jm_ref[k + m], ref.khat(rec(k + m), hkl))
        for a in range(S):
            for c in range(S):
                el = r2 * (np.abs(L0[:, a]) * dl[k + m][:, c] + np.abs(L1[:, c]) * dl[k][:, a]) + 2 * dl[k][:, a] * dl[k + m][:, c]
                et = sum(r2 * (np.abs(T0[:, a, x]) * dt[k + m][:, c, x] + np.abs(T1[:, c, x]) * dt[k][:, a, x]) +
                         2 * dt[k][:, a, x] * dt[k + m][:, c, x] for x in range(3))
                bl[a, c, wi] += np.bincount(b[ok], weights=(el + quantum[a, c])[ok], minlength=nbins)
                bt[a, c, wi] += np.bincount(b[ok], weights=(et + quantum[a, c])[ok], minlength=nbins)
    return bl, bt


def _check_against_reference(got, packed, hkl, windows, dq, nbins, stride, u, velocities=None, remove_com=True):
    counts, lng, trn, beyond, scale, vmax, kinds = got
    c_ref, l_ref, t_ref, b_ref, k_ref, vmax_ref = ref.current(packed, hkl, windows, dq, nbins, stride, velocities=velocities,
                                                              remove_com=remove_com, u=u)
    assert list(kinds) == list(k_ref) and np.array_equal(np.asarray(counts, dtype=np.int64), c_ref)
    assert np.array_equal(np.asarray(beyond, dtype=np.int64), b_ref) and abs(vmax - vmax_ref) <= 2.0 ** -22 * vmax_ref
    jm, w, _ = ref.all_modes(packed, hkl, velocities, remove_com, u)
    _, species = H.species_of(packed.numbers)
    S, F = len(kinds), len(packed)
    dl, dt = np.zeros((F, len(hkl), S)), np.zeros((F, len(hkl), S, 3))
    for f in range(1, F):
        dl[f], dt[f] = CX.projected(CX.budget(w[f], species, S, hkl, cell=None if velocities is not None else ref._cell_of(packed, f)))
    quantum = 0.5 * np.ldexp(1.0, -isf_ref.pair_scale(scale, S))
    bl, bt = _sum_bound(jm, dl, dt, ref._recips(packed), hkl, windows, dq, nbins, stride, quantum)
    fl = float((np.abs(lng - l_ref) / np.maximum(bl, 1e-300)).max())
    ft = float((np.abs(trn - t_ref) / np.maximum(bt, 1e-300)).max())
    print("sums against the reference: long %.3f, trans %.3f of the propagated budget" % (fl, ft))
    assert fl <= 1.0 and ft <= 1.0
    assert np.abs(l_ref).max() > 1e3 * bl.max() and np.abs(t_ref).max() > 1e3 * bt.max()       # far below the signal


def test_positions_mode_against_the_reference(hip_ctx):
    packed, hkl, u = _case("npt")
    got = hip_ctx.current_accumulate(packed, hkl, [0, 1, 3], 0.05, 40, origin_stride=2)
    _check_against_reference(got, packed, hkl, [0, 1, 3], 0.05, 40, 2, u)


def test_velocity_mode_against_the_reference(hip_ctx):
    packed, hkl, u = _case("five")
    rng = np.random.default_rng(81)
    vel = rng.normal(scale=0.01, size=(len(packed), packed.n_atoms, 3)) + np.array([0.02, -0.01, 0.005])
    vtraj = PackedTrajectory(vel, packed.cell, packed.numbers)
    windows = [0, 1, 3]
    got = hip_ctx.current_accumulate(packed, hkl, windows, 0.05, 40, velocities=vtraj)
    _check_against_reference(got, packed, hkl, windows, 0.05, 40, 1, u, velocities=vel)
    # device-resident velocities, and the integer sums from the library's own modes
    import torch
    vdev = PackedTrajectory(torch.tensor(vel, device="cuda:0"), packed.cell, packed.numbers)
    _same_bits(hip_ctx.current_accumulate(packed, hkl, windows, 0.05, 40, velocities=vdev), got)
    dev, scale, vmax, _ = _dev_call(hip_ctx, packed, hkl, windows, 0.05, 40, velocities=vtraj)
    jm = _library_modes(hip_ctx, packed, hkl, velocities=vtraj)
    counts, lng, trn, beyond = ref.correlate(jm, ref._recips(packed), hkl, windows, 0.05, 40, scale_log2=scale)
    assert np.array_equal(dev["long"], lng) and np.array_equal(dev["trans"], trn) and np.array_equal(dev["counts"], counts)
    # the class
    c = cc.CurrentCorrelation.from_velocities(packed, vel, delta_time=1, max_time=3, dq=0.05, qmax=2.0, device=0, distributed=False)
    nb = sf.n_bins(2.0, 0.05)
    assert not c.finite_difference and c.window.tolist() == [0, 1, 2]
    raw = hip_ctx.current_accumulate(packed, c.hkl, [0, 1, 2], 0.05, nb, velocities=vtraj)
    assert np.array_equal(np.asarray(c.long_sums).view(np.uint64), raw[1].view(np.uint64))


def test_uniform_velocity_is_the_density_mode(hip_ctx):
    """every velocity the same vector, remove_com off: j_a(k) = v rho_a(k), L = (k^ . v) rho within both budgets"""
    packed, hkl, u = _case("five")
    v = np.array([0.031, -0.017, 0.023])
    vel = np.broadcast_to(v, (len(packed), packed.n_atoms, 3)).copy()
    vtraj = PackedTrajectory(vel, packed.cell, packed.numbers)
    kinds, species = H.species_of(packed.numbers)
    rec = ref._recips(packed)[0]
    kh = ref.khat(rec, hkl)
    j, _ = hip_ctx.current_modes(packed, hkl, frame=3, velocities=vtraj, remove_com=False)
    rho, _ = hip_ctx.sq_modes(packed, hkl, frame=3)
    L, _ = ref.project(j, kh)
    kv = kh @ v.astype(np.float32).astype(np.float64)
    dl, _ = CX.projected(CX.budget(vel[3].astype(np.float32), species, len(kinds), hkl))
    worst = 0.0
    for a in range(len(kinds)):
        n = int((species == a).sum())
        bound = dl[:, a] + np.abs(kv) * X.budget(n, hkl, TERM_ERR, False)
        d = L[:, a] - kv * rho[:, a]
        worst = max(worst, float((np.abs(d.real) / bound).max()), float((np.abs(d.imag) / bound).max()))
    print("uniform velocity: worst %.3f of the bound" % worst)
    assert worst <= 1.0
    # with remove_com the same trajectory is at rest up to the rounding of the mean, a sum of N products rounded once each
    vm = hip_ctx.current_accumulate(packed, hkl, [0], 0.05, 40, velocities=vtraj)[5]
    assert vm <= packed.n_atoms * 2.0 ** -51 * np.abs(v).max()


# ------------------------------------------------------------------------------------------------------ 7: class --
def test_class_schema(tmp_path, hip_ctx):
    from amof_amd import data as _data
    packed, _, u = _case("zif4")
    c = cc.CurrentCorrelation.from_trajectory(packed, timestep=2, dq=0.05, qmax=1.6, device=0, distributed=False)
    names = [_data.chemical_symbols[int(z)] for z in packed.unique_numbers()]
    assert list(c.data.columns) == ["Time", "q", "X-X-L", "X-X-T"] + [a + "-" + b + "-" + p for a in names for b in names for p in "LT"]
    nbins = sf.n_bins(1.6, 0.05)
    assert c.window.tolist() == list(range(6)) and len(c.data) == 6 * nbins         # every lag up to F // 2
    np.testing.assert_array_equal(c.data["Time"].values, np.repeat(2.0 * np.arange(6), nbins))
    np.testing.assert_array_equal(c.data["q"].values, np.tile(np.arange(nbins) * 0.05, 6))
    assert c.n_origins.tolist() == [11, 10, 9, 8, 7, 6] and np.asarray(c.counts).shape == (6, nbins)
    assert c.finite_difference and c.vmax > 0
    raw = hip_ctx.current_accumulate(packed, c.hkl, c.window, 0.05, nbins)
    assert np.array_equal(np.asarray(c.long_sums).view(np.uint64), raw[1].view(np.uint64))
    assert np.array_equal(np.asarray(c.trans_sums).view(np.uint64), raw[2].view(np.uint64)) and np.array_equal(c.counts, raw[0])
    want = cc.assemble(raw[0], raw[1], raw[2], raw[6], packed.unique_numbers(), c.species_counts, 2.0 * np.arange(6), 0.05, timestep=2)
    assert c.data.equals(want)
    ok = (np.asarray(c.counts) > 0).reshape(-1)
    assert (~ok).any() and np.isnan(c.data["X-X-L"].values[~ok]).all() and np.isfinite(c.data.values[ok]).all()
    assert (c.data["X-X-L"].values[:nbins][ok[:nbins]] > 0).all() and (c.data["X-X-T"].values[:nbins][ok[:nbins]] > 0).all()
    w = c.weighted("number")
    np.testing.assert_allclose(w["L"].values[ok], c.data["X-X-L"].values[ok], rtol=1e-12)
    np.testing.assert_allclose(w["T"].values[ok], c.data["X-X-T"].values[ok], rtol=1e-12)
    wm = c.weighted()                                                               # 'mass'
    wd = c.weighted({s: c.mean_mass[z] for s, z in zip([_data.chemical_symbols[int(z)] for z in c.kinds], c.kinds)})
    np.testing.assert_allclose(wm["L"].values[ok], wd["L"].values[ok], rtol=1e-12)
    nrm = c.normalised()
    assert np.abs(nrm["X-X-L"].values[:nbins][ok[:nbins]] - 1.0).max() == 0.0
    sp = c.spectrum()
    assert list(sp.columns) == ["q", "Frequency_THz", "L", "T"] and len(sp) == nbins * (4 * 6 + 1)
    c.write_to_file(os.path.join(str(tmp_path), "z"))
    assert os.path.exists(os.path.join(str(tmp_path), "z.cqt"))
    assert cc.CurrentCorrelation.from_file(os.path.join(str(tmp_path), "z")).data.equals(c.data)


def test_spectrum_dispersion_and_sound_velocity_recover_the_plane_wave():
    """item 3's waves over 48 frames, every lag: the spectrum of the bin of K peaks at omega within one step of the frequency
    grid (pad 4 on 24 lags), the dispersion gives omega at |K|, and with K the only vector below q_fit the line through the
    origin gives omega / |K|"""
    for pol, col, key in (("transverse", "omega_T", "c_T"), ("longitudinal", "omega_L", "c_L")):
        packed, omega, kk, c = _wave(pol, F=48)
        r = cc.CurrentCorrelation.from_trajectory(packed, timestep=1, dq=0.004, qmax=0.45, device=0, distributed=False)
        assert r.window.tolist() == list(range(24))
        step = 2.0 * np.pi / (4 * 2 * 24)                   # rad / fs
        sp = r.spectrum()
        bK = int(kk / 0.004)
        blk = sp[sp["q"] == bK * 0.004]
        peak = blk["Frequency_THz"].values[int(np.argmax(blk["T" if pol == "transverse" else "L"].values))]
        assert abs(2.0 * np.pi * peak / 1e3 - omega) <= step
        d = r.dispersion()
        assert len(d) == 3 and abs(d["q"].values[0] - kk) < 1e-9          # (0, 1, 0), (0, 0, 1), (1, 0, 0)
        assert abs(d[col].values[0] - omega) <= step, (pol, d[col].values[0], omega)
        sv = r.sound_velocity(q_fit=0.36)
        assert sv["n_bins"] == 1 and abs(sv[key] - 1e5 * omega / kk) <= 1e5 * step / kk
        rho = 512 * 63.546 / (16.0 * 17.0 * 18.0) * cc.KG_PER_M3_PER_AMU_PER_A3
        assert sv["density"] == pytest.approx(rho, rel=1e-3) and sv["K"] == pytest.approx(sv["M"] - 4.0 * sv["G"] / 3.0)
        assert sv["M" if key == "c_L" else "G"] == pytest.approx(rho * sv[key] ** 2 * 1e-9)


def test_argument_errors(hip_ctx):
    packed = H.random_walk(H.zif4_frame(), 5, 0.05, 43)
    hkl = np.array([[1, 0, 0], [0, 2, 1]])
    open_cell = PackedTrajectory(packed.pos_host(), packed.cell, packed.numbers, pbc=(True, True, False))
    short = PackedTrajectory(packed.pos_host()[:4], packed.cell, packed.numbers)
    nan_vel = PackedTrajectory(np.full((5, packed.n_atoms, 3), np.nan), packed.cell, packed.numbers)
    bad = [lambda: hip_ctx.current_accumulate(open_cell, hkl, [0, 1], 0.1, 20),
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20, origin_stride=0),
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 5], 0.1, 20),                     # lag >= F
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, -1], 0.1, 20),
           lambda: hip_ctx.current_accumulate(packed, [[1, 0, 0], [0, 0, 0]], [0, 1], 0.1, 20),
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20, work_range=(0, 8)),  # 4 + 3 entries
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20, work_range=(5, 4)),
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.0, 20),
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20, velocities=short),
           lambda: hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20, velocities=nan_vel),
           lambda: hip_ctx.current_modes(packed, hkl, frame=0),
           lambda: hip_ctx.current_modes(packed, hkl, frame=5),
           lambda: hip_ctx.current_modes(packed, [[0, 0, 0]], frame=1),
           lambda: cc.CurrentCorrelation.from_trajectory(open_cell, device=0, distributed=False),
           lambda: cc.CurrentCorrelation.from_trajectory(packed, origin_stride=0, device=0, distributed=False),
           lambda: cc.CurrentCorrelation.from_trajectory(packed, dq=0.0, device=0, distributed=False),
           lambda: cc.CurrentCorrelation.from_velocities(packed, np.zeros((4, packed.n_atoms, 3)), device=0, distributed=False),
           lambda: cc.CurrentCorrelation().compute_current(packed, [0, 7], [0, 7], device=0, distributed=False)]         # a bad lag
    for fn in bad:
        with pytest.raises(ValueError):
            fn()
    got = hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20, work_range=(3, 3))          # an empty range: zeros, the scale
    full = hip_ctx.current_accumulate(packed, hkl, [0, 1], 0.1, 20)
    assert got[0].sum() == 0 and not got[1].any() and not got[2].any() and np.array_equal(got[4], full[4]) and got[5] == full[5]


def test_capacity_surfaces_as_a_value_error(hip_ctx):
    """every vector in one bin over a long trajectory: the fixed-point quantum would exceed 2^-20 (AMOF_ECAPACITY); the class
    names the remedies"""
    import torch
    N, F = 1024, 4200
    rng = np.random.default_rng(44)
    pos = torch.tensor(rng.random((N, 3)) * 12.0, dtype=torch.float64, device="cuda:0").expand(F, N, 3).contiguous()
    pos[1::2, :, 0] += 0.01                                  # a step of 0.01 Angstrom to and fro: vmax > 0
    packed = PackedTrajectory(pos, np.diag([12.0, 12.0, 12.0]), [8] * N)
    r = np.arange(-80, 81, dtype=np.int32)
    t = np.stack(np.meshgrid(r, r, r, indexing="ij"), axis=-1).reshape(-1, 3)
    hkl = np.ascontiguousarray(t[sf.half_space(t)])
    with pytest.raises(_hip.AmofError) as err:
        hip_ctx.current_accumulate(packed, hkl, [0], 1000.0, 1, work_range=(0, 1), remove_com=False)
    assert err.value.code == _hip.AMOF_ECAPACITY
    with pytest.raises(ValueError, match="max_points"):
        cc.CurrentCorrelation.from_trajectory(packed, delta_time=1000, dq=50.0, qmax=55.0, remove_com=False, device=0,
                                              distributed=False).data


# ------------------------------------------------------------------------------------------------------ 8: ranks --
def _run_current(distributed):
    import torch
    packed = H.device_walk(torch.device("cuda", 0), (1, 1, 2), 9, 0.05, 41)     # same seed on every rank
    f = cc.CurrentCorrelation.from_trajectory(packed, delta_time=2, dq=0.04, qmax=1.6, device=0, distributed=distributed)
    host = H.random_walk(H.zif4_frame(), 8, 0.05, 42, cell_jitter=0.01)
    g = cc.CurrentCorrelation.from_trajectory(host, dq=0.04, qmax=1.6, origin_stride=2, device=0, distributed=distributed)
    return {"data": f.data.values, "counts": np.asarray(f.counts), "long": f.long_sums, "trans": f.trans_sums,
            "data_npt": g.data.values, "long_npt": g.long_sums, "trans_npt": g.trans_sums, "beyond_npt": np.asarray(g.beyond)}


def _worker_current(rank, world, port, out_dir, backend):
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
    res = _run_current(None)
    for k, arr in res.items():
        np.save(os.path.join(out_dir, "%s_rank%d.npy" % (k, rank)), arr)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("backend,world", [("gloo", 2), ("nccl", 1)])
def test_ranks_equal_single_process(tmp_path, backend, world):
    """the (lag, origin) work list shared over the ranks (two gloo ranks on cuda:0; one RCCL rank with every collective run):
    every rank arrives at the trajectory's vmax and scale, the integer sums add up exactly"""
    import torch.multiprocessing as mp
    port = 36600 + (os.getpid() + world) % 2000
    mp.spawn(_worker_current, args=(world, port, str(tmp_path), backend), nprocs=world, join=True)
    single = _run_current(False)
    for k, want in single.items():
        for rank in range(world):
            got = np.load(os.path.join(str(tmp_path), "%s_rank%d.npy" % (k, rank)))
            assert np.array_equal(got, want, equal_nan=True), k
