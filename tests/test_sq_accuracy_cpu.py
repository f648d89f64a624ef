"""The accuracy budget of the density modes without a GPU: the exact-phase reference (tests/sq_exact_ref.py) against mpmath,
the numpy emulation of sq_rho_kernel's documented chain (correctly rounded functions) within the derived budget on every
case of tests/sq_accuracy_cases.py -- so the budget is a true bound on the chain and the inputs are admissible -- and the
emulated chain on the Bragg peaks of a shifted crystal within half of S(q)'s contract."""

import numpy as np
import pytest

from tests import sq_accuracy_cases as C
from tests import sq_exact_ref as X
from tests import sq_ref

TOL = 1e-5          # tests/test_gpu_sq.py: the project's S(q) contract


def _errors(got, want):
    d = got - want
    return np.abs(d.real), np.abs(d.imag)


def test_reference_against_mpmath():
    import mpmath as mp
    case = C.single_term()
    rng = np.random.default_rng(1)
    pick = np.concatenate([np.flatnonzero(~case["sweep"]), rng.choice(C.N_SWEEP, size=500, replace=False)])
    hkl = case["hkl"][pick]
    worst = 0.0
    with mp.workdps(40):
        for f in (0, 1):
            got = X.modes_exact(case["u"][f], case["species"], 1, hkl)[:, 0]
            ux, uy, uz = (int(v) for v in case["u"][f][0])
            for (h, k, l), z in zip(hkl.tolist(), got):
                phi = (h * ux + k * uy + l * uz) % (1 << 32)
                t = 2 * mp.pi * mp.mpf(phi) / mp.mpf(1 << 32)
                worst = max(worst, float(abs(mp.cos(t) - mp.mpf(z.real))), float(abs(mp.sin(t) - mp.mpf(z.imag))))
    assert worst <= 4e-16, "modes_exact off by %.3g per term" % worst
    # the points the GPU test asserts exactly
    c, s = X.unit(np.array([0, 1 << 30, 1 << 31, 3 << 30], dtype=np.uint64))
    assert c.tolist() == [1.0, 0.0, -1.0, 0.0] and s.tolist() == [0.0, 1.0, 0.0, -1.0]


def test_budget_constants():
    assert X.SQ_BLOCK == 64
    assert X.acc(1) == 0.0 and X.acc(2) == 2 * X.U and X.acc(64) == 2079 * X.U
    assert X.acc(65) == X.acc(64) and X.acc(129) == 2 * X.acc(64) and X.acc(512) == 8 * X.acc(64)
    assert X.acc(63) == (63 * 32 - 1) * X.U
    assert abs(X.MODEL_TERM / X.U - 2.0708) < 1e-4
    np.testing.assert_allclose(X.quant([[3, -4, 5]]), [2 * np.pi * 24 * 2.0 ** -32])
    assert X.MODEL_TERM <= C.TERM_ERR <= C.TERM_CEILING == 2.0 ** -19
    assert np.log2(C.TERM_ERR) == int(np.log2(C.TERM_ERR))


def _within_budget(case, frame, want, hkl=None, what=""):
    hkl = case["hkl"] if hkl is None else hkl
    got = X.model(case["u"][frame], case["species"], len(case["kinds"]), hkl)
    worst = 0.0
    for a, n in enumerate(case["counts"]):
        bound = X.budget(n, hkl, X.MODEL_TERM, case["dyadic"])
        for e in _errors(got[:, a], want[:, a]):
            worst = max(worst, float((e / n).max()) / X.U)
            assert (e <= bound).all(), "%s species %d (n = %d): %.3g above the budget" % (what, a, n, (e - bound).max())
    return worst


def test_model_within_budget_single_term():
    case = C.single_term()
    for f in (0, 1):
        want = X.modes_exact(case["u"][f], case["species"], 1, case["hkl"])
        worst = _within_budget(case, f, want, what="single_term frame %d" % f)
        print("single term, frame %d: %.2f units of 2^-24 (bound %.2f)" % (f, worst, X.MODEL_TERM / X.U))
        assert worst > 1.0          # the sweep reaches the conversion's share of the bound: the case exercises it


def _unsigned_chain(u, hkl):
    """the chain with the conversion a kernel must not use: (float)(uint32)phi, x in [0, 1]; one atom, correctly rounded"""
    r = (np.asarray(hkl, dtype=np.int64) % (1 << 32)).astype(np.uint32)
    phi = r[:, 0] * u[0] + r[:, 1] * u[1] + r[:, 2] * u[2]
    t = 2.0 * np.pi * (phi.astype(np.float32) * np.float32(2.0 ** -32)).astype(np.float64)
    return np.cos(t).astype(np.float32).astype(np.float64) + 1j * np.sin(t).astype(np.float32).astype(np.float64)


def test_exact_planted_phases_see_the_conversion():
    """on the planted phases f32 holds exactly the signed chain has no conversion error: correctly rounded functions stay
    within half a unit, inside TERM_ERR_EXACT; an unsigned conversion errs by pi units at -2^31 + 128 and breaks that bound,
    while it stays inside TERM_ERR everywhere -- so the exact phases are what pins the conversion"""
    case = C.single_term()
    planted = case["hkl"][~case["sweep"]][:-1]
    exact = C.exact_in_f32(planted[:, 0])
    assert 60 <= exact.sum() < len(planted) and exact[planted[:, 0].tolist().index(-2 ** 31 + 128)]
    assert X.MODEL_TERM > C.TERM_ERR_EXACT >= X.U / 2 and C.TERM_ERR_EXACT < np.pi * X.U
    with np.errstate(over="ignore"):
        for f in (0, 1):
            want = X.modes_exact(case["u"][f], case["species"], 1, planted[exact])[:, 0]
            d = X.model(case["u"][f], case["species"], 1, planted[exact])[:, 0] - want
            assert max(np.abs(d.real).max(), np.abs(d.imag).max()) <= X.U / 2
            d = _unsigned_chain(case["u"][f][0], planted[exact]) - want
            assert max(np.abs(d.real).max(), np.abs(d.imag).max()) > C.TERM_ERR_EXACT
            d = _unsigned_chain(case["u"][f][0], case["hkl"]) - X.modes_exact(case["u"][f], case["species"], 1, case["hkl"])[:, 0]
            assert max(np.abs(d.real).max(), np.abs(d.imag).max()) < C.TERM_ERR


def test_model_within_budget_coherent():
    case = C.coherent()
    want = X.modes_exact(case["u"][0], case["species"], len(case["kinds"]), case["hkl"])
    np.testing.assert_allclose(np.abs(want), np.broadcast_to(case["counts"], want.shape), rtol=1e-13)      # |rho_s| = n_s
    worst = _within_budget(case, 0, want, what="coherent")
    print("coherent: %.2f units of 2^-24 per atom (bound for 64 atoms %.2f)" % (worst, X.budget(64, [[1, 0, 0]], X.MODEL_TERM, True) / 64 / X.U))


def _binned(rho, case, cell):
    """rho [K][S] through the binning of sq_ref.sq: (counts, sums)"""
    nbins, S = case["nbins"], len(case["kinds"])
    b = sq_ref.bins(sq_ref.reciprocal(cell), case["hkl"], case["dq"], nbins)
    ok = b < nbins
    counts = np.bincount(b[ok], minlength=nbins)
    sums = []
    for a in range(S):
        for d in range(a, S):
            t = rho[:, a].real * rho[:, d].real + rho[:, a].imag * rho[:, d].imag
            sums.append(np.bincount(b[ok], weights=t[ok], minlength=nbins))
    return counts, np.array(sums)


@pytest.mark.parametrize("name", ["diagonal", "sheared"])
def test_shifted_lattice_model_and_bragg_peaks(name):
    case = C.shifted_lattice(name)
    packed = case["packed"]
    cell = packed.cell[0]
    assert case["bragg"].sum() >= 3
    want = sq_ref.modes(packed.pos_host()[0], cell, case["species"], 2, case["hkl"])
    np.testing.assert_allclose(np.abs(want[case["bragg"]]), 256.0, rtol=1e-12)      # every atom of a species in phase
    worst = _within_budget(case, 0, want, what="shifted_lattice " + name)
    print("shifted lattice (%s): %.2f units of 2^-24 per atom" % (name, worst))
    # the emulated chain on the peaks, through S(q)'s binning and normalisation: half the contract
    got = X.model(case["u"][0], case["species"], 2, case["hkl"])
    c_ref, s_ref, beyond, kinds = sq_ref.sq(packed, case["hkl"], case["dq"], case["nbins"])
    counts, sums = _binned(got, case, cell)
    assert np.array_equal(counts, c_ref)
    a = sq_ref.normalised(counts, sums, kinds, packed.numbers)
    b = sq_ref.normalised(c_ref, s_ref, kinds, packed.numbers)
    ok = c_ref > 0
    assert np.nanmax(b[:, ok]) > 100.0
    err = np.abs(a[:, ok] - b[:, ok]) / np.maximum(1.0, np.abs(b[:, ok]))
    peak = np.abs(b[:, ok]) > 100.0
    print("shifted lattice (%s): S off by %.3g relative, %.3g on the peaks (S up to %.0f)" % (name, err.max(), err[peak].max(), np.nanmax(b[:, ok])))
    assert err.max() <= TOL / 2


def test_case_sanity():
    single, coh = C.single_term(), C.coherent()
    for case in (single, coh):
        assert case["dyadic"] and (np.abs(case["hkl"]).sum(axis=1) > 0).all()
        pos = case["packed"].pos_host()
        for f in range(len(pos)):
            assert np.array_equal(X.quantize(pos[f], C.CELL), case["u"][f])
    assert np.array_equal(X.inverse(C.CELL), np.diag([0.0625] * 3))
    assert single["kinds"] == [29] and single["u"].shape == (2, 1, 3) and single["u"][0, 0].tolist() == [1, 0, C.G0]
    assert C.G0 % 2 == 1 and C.G1 % 2 == 1 and C.G0 != C.G1
    assert single["sweep"].sum() == C.N_SWEEP and 100 <= (~single["sweep"]).sum() <= 200
    h = single["hkl"][~single["sweep"]][:-1, 0]
    for must in (1, -3, 256, 2 ** 24 + 1, 2 ** 30, -2 ** 30, 2 ** 29 + 128, -2 ** 31, 2 ** 31 - 1, -2 ** 31 + 1, 2 ** 31 - 128):
        assert must in h
    assert np.abs(h).max() <= 2 ** 31 and h.min() == -2 ** 31 and single["hkl"][-1].tolist() == [0, 1, 0]
    assert coh["kinds"] == [1, 6, 7, 8, 29, 30] and coh["counts"].tolist() == [1, 63, 64, 65, 129, 512]
    assert not np.array_equal(np.sort(coh["species"]), coh["species"])          # the species permutation does work
    assert len(np.unique(coh["u"][0], axis=0)) == 6 and np.abs(coh["hkl"]).max() <= 64
    rows = coh["hkl"][C.N_RANDOM:]
    assert len(rows) == 200 * 21 - 1 and ((rows[:, :2] == 0).all(axis=1)).sum() == 20
    for name in ("diagonal", "sheared"):
        case = C.shifted_lattice(name)
        assert not case["dyadic"] and case["kinds"] == [7, 30] and case["counts"].tolist() == [256, 256]
        assert (np.abs(case["hkl"]).sum(axis=1) > 0).all() and [8, 0, 0] in case["hkl"].tolist()
        # the restated quantisation lies within the budget's two units of the real-number coordinates
        g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
        frac = (g / 8.0 + C.OFFSET) % 1.0
        d = (case["u"][0].astype(np.int64) - np.floor(frac * 2.0 ** 32).astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)
        assert np.abs(d).max() <= 2
