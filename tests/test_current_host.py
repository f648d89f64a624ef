"""The host side of CurrentCorrelation without a GPU: ``assemble``, ``combine`` (weighted), ``normalise``, ``transform``
(spectrum) and the line fit on hand-made sums; the numpy restatement tests/current_ref.py against a brute-force double loop
over atoms on a 10-atom case, and its fixed-point form against its float64 form; the error budget's pieces."""

import numpy as np
import pytest

from amof_amd import current_correlation as cc
from tests import current_exact_ref as CX
from tests import current_ref as ref
from tests import helpers as H
from tests import sq_exact_ref as X


def _sums(S=2, W=3, nbins=4, seed=1):
    rng = np.random.default_rng(seed)
    counts = rng.integers(1, 9, size=(W, nbins)).astype(np.uint64)
    counts[:, 0] = 0                                                  # a bin without a vector
    return counts, rng.normal(size=(S, S, W, nbins)), rng.normal(size=(S, S, W, nbins))


def test_assemble_schema_and_normalisation():
    counts, lng, trn = _sums()
    kinds, elements, n = [6, 30], [30, 6], {6: 5, 30: 3}
    d = cc.assemble(counts, lng, trn, kinds, elements, n, [0.0, 2.0, 4.0], 0.1, timestep=2)
    assert list(d.columns) == cc.column_names(elements) == ["Time", "q", "X-X-L", "X-X-T", "Zn-Zn-L", "Zn-Zn-T", "Zn-C-L", "Zn-C-T",
                                                          "C-Zn-L", "C-Zn-T", "C-C-L", "C-C-T"]
    np.testing.assert_array_equal(d["Time"].values, np.repeat([0.0, 2.0, 4.0], 4))
    np.testing.assert_array_equal(d["q"].values, np.tile(np.arange(4) * 0.1, 3))
    c = counts.astype(float)
    ok = (c > 0).reshape(-1)
    assert np.isnan(d.values[~ok][:, 2:]).all() and np.isfinite(d.values[ok]).all()
    with np.errstate(divide="ignore", invalid="ignore"):
        np.testing.assert_allclose(d["X-X-L"].values[ok], (lng.sum(axis=(0, 1)) / (c * 8 * 4)).reshape(-1)[ok], rtol=1e-14)
        np.testing.assert_allclose(d["X-X-T"].values[ok], (0.5 * trn.sum(axis=(0, 1)) / (c * 8 * 4)).reshape(-1)[ok], rtol=1e-14)
        # Zn (kind 1) at the origin, C (kind 0) at the origin + lag
        np.testing.assert_allclose(d["Zn-C-L"].values[ok], (lng[1, 0] / (c * np.sqrt(15.0) * 4)).reshape(-1)[ok], rtol=1e-14)
        np.testing.assert_allclose(d["C-Zn-T"].values[ok], (0.5 * trn[0, 1] / (c * np.sqrt(15.0) * 4)).reshape(-1)[ok], rtol=1e-14)


def test_weighted_number_is_the_x_columns_and_mass_is_the_momentum_current():
    counts, lng, trn = _sums()
    n = [5, 3]
    d = cc.assemble(counts, lng, trn, [6, 30], [6, 30], {6: 5, 30: 3}, [0.0, 1.0, 2.0], 0.1)
    w = cc.combine(counts, lng, trn, [1.0, 1.0], n, [0.0, 1.0, 2.0], 0.1)
    np.testing.assert_allclose(w["L"].values, d["X-X-L"].values, rtol=1e-14, equal_nan=True)
    np.testing.assert_allclose(w["T"].values, d["X-X-T"].values, rtol=1e-14, equal_nan=True)
    m = np.array([12.0, 65.4])
    wm = cc.combine(counts, lng, trn, m, n, [0.0, 1.0, 2.0], 0.1)
    with np.errstate(divide="ignore", invalid="ignore"):
        want = sum(m[a] * m[c] * lng[a, c] for a in range(2) for c in range(2)) / (counts.astype(float) * (5 * 144.0 + 3 * 65.4 ** 2))
    ok = counts.reshape(-1) > 0
    np.testing.assert_allclose(wm["L"].values[ok], want.reshape(-1)[ok], rtol=1e-13)
    nrm = cc.normalise(d, [0, 1, 2])
    assert np.abs(nrm["X-X-L"].values[:4][ok[:4]] - 1.0).max() == 0.0
    with pytest.raises(ValueError):
        cc.normalise(d, [1, 2, 3])


def test_transform_finds_a_cosine_and_is_vdos_transform():
    from amof_amd import vacf
    M, dt, period = 64, 2.0, 16.0
    t = dt * np.arange(M)
    c = np.stack([np.cos(2 * np.pi * t / period), np.cos(2 * np.pi * t / (2 * period))])
    nu, D = cc.transform(c, dt, "hann", 4)
    assert D.shape == (2, 4 * M + 1) and abs(nu[np.argmax(D[0])] - 1 / period) <= 1 / (8 * M * dt)
    assert abs(nu[np.argmax(D[1])] - 1 / (2 * period)) <= 1 / (8 * M * dt)
    # the same numbers as VelocityAutocorrelation.vdos on the same series
    import pandas as pd
    v = vacf.VelocityAutocorrelation()
    v.data = pd.DataFrame({"Time": t, "X": c[0]})
    got = v.vdos(window="hann", pad=4, fd_correction=True)
    _, Dfd = cc.transform(c[0], dt, "hann", 4, timestep=dt)
    np.testing.assert_allclose(got["X"].values, Dfd, rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(got["Frequency_THz"].values, nu * 1e3, rtol=1e-14)
    for bad in ({"window": "box"}, {"pad": 0}, {"pad": 1.5}):
        with pytest.raises(ValueError):
            cc.transform(c, dt, **bad)
    with pytest.raises(ValueError):
        cc.lag_spacing([0.0, 1.0, 3.0])
    with pytest.raises(ValueError):
        cc.lag_spacing([1.0, 2.0])
    assert cc.fit_through_origin([0.0, 0.1, 0.2, np.nan], [5.0, 0.3, 0.6, 1.0]) == pytest.approx(3.0)


def _tiny(seed, F=5, jitter=0.0):
    numbers = [8] * 6 + [14] * 4
    cell = np.array([[6.0, 0.0, 0.0], [1.0, 5.5, 0.0], [-0.5, 0.7, 5.0]])
    gas = H.random_gas(10, cell, numbers, seed)
    from amof_amd.frames import Frame
    return H.random_walk(Frame(np.array(numbers), gas.pos[0], cell, (True, True, True)), F, 0.15, seed + 1, cell_jitter=jitter)


@pytest.mark.parametrize("jitter,remove_com", [(0.0, True), (0.02, False)])
def test_reference_against_a_double_loop_over_atoms(jitter, remove_com):
    packed = _tiny(3, jitter=jitter)
    hkl = np.array([[1, 0, 0], [0, 1, 1], [1, -1, 2], [0, 0, 1], [2, 1, 0]])
    windows, dq, nbins = [0, 1, 2], 0.7, 4
    c, lng, trn, bey, kinds, vmax = ref.current(packed, hkl, windows, dq, nbins, remove_com=remove_com)
    c2, l2, t2, b2, k2 = ref.brute(packed, hkl, windows, dq, nbins, remove_com=remove_com)
    assert kinds == k2 and np.array_equal(c, c2) and np.array_equal(bey, b2) and c.sum() > 0 and bey.sum() > 0
    scale = max(np.abs(l2).max(), np.abs(t2).max())
    assert np.abs(lng - l2).max() <= 1e-12 * scale and np.abs(trn - t2).max() <= 1e-12 * scale
    # |j|^2 = |L|^2 + |T|^2 at lag 0 per species pair: the projections lose nothing
    jm, w, _ = ref.all_modes(packed, hkl, remove_com=remove_com)
    assert vmax == float(np.abs(w[1:]).max()) and vmax > 0
    if remove_com:
        m = np.asarray(packed.masses)
        v, _, _ = ref.samples(packed)
        assert np.abs((m[None, :, None] * v[1:]).sum(axis=1)).max() <= 1e-12 * m.sum() * vmax


def test_fixed_point_form_of_the_reference_and_work_ranges():
    packed = _tiny(7, F=7)
    hkl = np.array([[1, 0, 0], [0, 1, 1], [1, -1, 2], [0, 0, 1]])
    windows, dq, nbins = [0, 2, 3], 0.5, 6
    jm, w, kinds = ref.all_modes(packed, hkl)
    rec = ref._recips(packed)
    f64 = ref.correlate(jm, rec, hkl, windows, dq, nbins)
    scale = [40, 41, 42]
    fixed = ref.correlate(jm, rec, hkl, windows, dq, nbins, scale_log2=scale)
    assert np.array_equal(f64[0], fixed[0]) and fixed[1].dtype == np.int64
    exp2 = np.array([[40, 41], [41, 42]])
    for x in (1, 2):
        got = np.ldexp(fixed[x].astype(np.float64), -exp2[:, :, None, None])
        # one rounding of half a quantum per sample
        assert np.abs(got - f64[x]).max() <= 0.5 * 2.0 ** -40 * f64[0].max() + 1e-15
    total = sum(len(ref.isf_ref.origins(7, m)) for m in windows)
    a = ref.correlate(jm, rec, hkl, windows, dq, nbins, work_range=(0, 4), scale_log2=scale)
    b = ref.correlate(jm, rec, hkl, windows, dq, nbins, work_range=(4, total), scale_log2=scale)
    assert all(np.array_equal(x + y, z) for x, y, z in zip(a, b, fixed))


def test_samples_are_the_minimum_image_steps_at_the_midpoint():
    packed = _tiny(11, F=4)
    u = ref.quantized(packed)
    v, w, p = ref.samples(packed, remove_com=False, u=u)
    pos = np.asarray(packed.pos_host())
    cell = np.asarray(packed.cell).reshape(3, 3)
    for f in range(1, 4):
        d = pos[f] - pos[f - 1]
        s = np.linalg.solve(cell.T, d.T).T
        d = (s - np.rint(s)) @ cell
        assert np.abs(v[f] - d).max() <= 1e-8                      # the u32 grid: 2^-32 of a cell vector per coordinate
        mid = u[f - 1].astype(np.float64) + 0.5 * (u[f] - u[f - 1]).view(np.int32)
        assert np.abs(((p[f].astype(np.float64) - mid + 2.0 ** 31) % 2.0 ** 32) - 2.0 ** 31).max() <= 0.5
    assert w.dtype == np.float32 and not v[0].any() and not p[0].any()
    vel = np.random.default_rng(1).normal(size=pos.shape)
    v2, _, p2 = ref.samples(packed, velocities=vel, remove_com=False, u=u)
    assert np.array_equal(v2[1:], vel[1:]) and np.array_equal(p2[1:], u[1:])


def test_budget_pieces():
    assert CX.acc(1) == CX.U and CX.acc(X.SQ_BLOCK) == CX.U * (X.SQ_BLOCK * (X.SQ_BLOCK + 1) // 2)
    assert CX.acc(X.SQ_BLOCK + 1) == CX.acc(X.SQ_BLOCK) + CX.U
    w = np.array([[0.5, -0.25, 0.0], [0.125, 0.25, 0.0]], dtype=np.float32)
    b = CX.budget(w, [0, 0], 1, [[1, 2, 3]], cell=np.diag([10.0, 20.0, 30.0]))
    want = 0.625 * (CX.TERM_ERR + 2.0 ** -23 + X.quant([[1, 2, 3]])[0]) + 0.5 * CX.acc(2) + 2 * 4 * 2.0 ** -32 * 10.0
    assert b.shape == (1, 1, 3) and b[0, 0, 0] == pytest.approx(want, rel=1e-14)
    assert b[0, 0, 2] == pytest.approx(2 * 4 * 2.0 ** -32 * 30.0, rel=1e-14)
    dl, dt = CX.projected(b)
    assert dl[0, 0] == pytest.approx(np.sqrt(3.0) * b.max()) and (dt >= b).all()
