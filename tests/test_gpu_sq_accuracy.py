"""The f32 accuracy of sq_rho_kernel on the GPU (amof_sq_modes, amof_sq_accumulate, the self part of amof_isf_accumulate)
against the exact-phase reference and the derived budget of tests/sq_exact_ref.py, on the inputs of
tests/sq_accuracy_cases.py where f32 errors add up: single hardware evaluations, species stacked on one site, a crystal at a
generic offset (the documented 1e-5 max(1, |S|) contract on a Bragg peak), a generic uniform shift per frame."""

import numpy as np
import pytest

from tests import isf_ref
from tests import sq_accuracy_cases as C
from tests import sq_exact_ref as X
from tests import sq_ref
from tests.test_gpu_isf import _dev_call
from tests.test_gpu_sq import TOL, _compare_s

pytestmark = pytest.mark.gpu

TERM_ERR = C.TERM_ERR


def _assert_within(got, want, counts, hkl, dyadic, what):
    """every species and component of rho within budget(n, hkl, TERM_ERR, dyadic); returns the worst error per atom"""
    worst = 0.0
    for a, n in enumerate(counts):
        bound = X.budget(n, hkl, TERM_ERR, dyadic)
        for name, e in (("Re", np.abs((got - want)[:, a].real)), ("Im", np.abs((got - want)[:, a].imag))):
            worst = max(worst, float((e / n).max()))
            i = int(np.argmax(e - bound))
            assert (e <= bound).all(), ("%s: %s rho of species %d (n = %d) at hkl %s off by %.4g = %.2f x 2^-24 per atom, budget %.4g"
                                        % (what, name, a, n, hkl[i].tolist(), e[i], e[i] / n / X.U, np.broadcast_to(bound, e.shape)[i]))
    return worst


def test_single_terms(hip_ctx):
    """one atom: every component of rho is one v_cos_f32 / v_sin_f32 of the converted phase.  The maxima (cos and sin; swept
    phases, planted phases, and the planted phases f32 holds exactly) are the measurement behind TERM_ERR and TERM_ERR_EXACT
    (tests/sq_accuracy_cases.py)."""
    case = C.single_term()
    sweep, hkl = case["sweep"], case["hkl"]
    worst = {"sweep cos": 0.0, "sweep sin": 0.0, "planted cos": 0.0, "planted sin": 0.0, "exact cos": 0.0, "exact sin": 0.0}
    exact = ~sweep
    exact[~sweep] = np.append(C.exact_in_f32(hkl[~sweep][:-1, 0]), True)       # (and phase 0)
    assert 60 <= exact.sum() < (~sweep).sum()
    results = []
    for f in (0, 1):
        rho, kinds = hip_ctx.sq_modes(case["packed"], hkl, frame=f)
        assert hip_ctx.last_path() == "sq_modes" and list(kinds) == [29] and rho.shape == (len(hkl), 1)
        want = X.modes_exact(case["u"][f], case["species"], 1, hkl)
        d = (rho - want)[:, 0]
        for part, m in (("sweep", sweep), ("planted", ~sweep), ("exact", exact)):
            worst[part + " cos"] = max(worst[part + " cos"], float(np.abs(d.real[m]).max()))
            worst[part + " sin"] = max(worst[part + " sin"], float(np.abs(d.imag[m]).max()))
        results.append((rho[:, 0], d))
    report = ", ".join("%s %.4g = %.3f x 2^-24" % (k, v, v / X.U) for k, v in worst.items())
    print("single terms: " + report + "; TERM_ERR = 2^%d" % int(np.log2(TERM_ERR)))
    assert max(worst.values()) <= TERM_ERR, report
    # the planted phases f32 holds exactly: no conversion error under the signed chain, the instructions by themselves
    assert max(worst["exact cos"], worst["exact sin"]) <= C.TERM_ERR_EXACT, report
    for rho, d in results:
        assert (np.abs(d.real) <= TERM_ERR).all() and (np.abs(d.imag) <= TERM_ERR).all(), report
        at = {int(h): rho[C.N_SWEEP + i] for i, h in enumerate(hkl[~sweep][:-1, 0])}
        assert rho[-1] == 1.0 + 0.0j, report                                # phase 0: the vector (0, 1, 0)
        assert at[-2 ** 31].real == -1.0 and at[2 ** 31 - 1].real == -1.0, report
        assert abs(at[2 ** 30].real) <= TERM_ERR and abs(at[-2 ** 30].real) <= TERM_ERR, report
        # 128 away from -+1/2 revolution, exact in f32 as a signed integer: the sine is -+pi units of 2^-24, not the 0 of
        # +-1/2 itself (where a conversion that rounds the neighbour onto 2^31 would put it)
        assert at[-2 ** 31 + 128].imag < 0.0 < at[2 ** 31 - 128].imag, report


def test_coherent_species(hip_ctx):
    """six species of 1 .. 512 atoms, each stacked on one dyadic site: rho_s = n_s exp(i theta) exactly for every vector, the
    error of every term and of every f32 add has the same sign pattern along a partial, nothing averages away"""
    case = C.coherent()
    packed, hkl, S = case["packed"], case["hkl"], len(case["kinds"])
    rho, kinds = hip_ctx.sq_modes(packed, hkl)
    assert hip_ctx.last_path() == "sq_modes" and list(kinds) == case["kinds"]
    want = X.modes_exact(case["u"][0], case["species"], S, hkl)
    worst = _assert_within(rho, want, case["counts"], hkl, True, "coherent")
    print("coherent species: rho off by at most %.3g = %.2f x 2^-24 per atom" % (worst, worst / X.U))
    # S(q) of the same structure: every S_aa = n_a in every bin, a peak everywhere
    rand = hkl[:C.N_RANDOM]
    dq, nbins = 5.5, 8                      # |q| = (2 pi / 16) |hkl| < 43.6
    got = hip_ctx.sq_accumulate(packed, rand, dq, nbins)
    assert hip_ctx.last_path() == "sq"
    assert (np.asarray(got[0]) > 0).all() and int(got[2]) == 0 and int(np.asarray(got[0]).sum()) == C.N_RANDOM
    _compare_s(got, sq_ref.sq(packed, rand, dq, nbins), packed.numbers)


@pytest.mark.parametrize("name", ["diagonal", "sheared"])
def test_shifted_lattice_bragg_peaks(hip_ctx, name):
    """a rock-salt coloured 8^3 lattice at a generic offset: rho on the Bragg vectors (256 atoms in phase, a generic phase) and
    on 500 others within the budget, and S(q) -- peaks of 512 (diagonal cell) and 128 (sheared cell) -- within the contract"""
    case = C.shifted_lattice(name)
    packed = case["packed"]
    pick = C.modes_subset(case)
    hkl = case["hkl"][pick]
    assert case["bragg"].sum() >= 3 and case["bragg"][pick].sum() == case["bragg"].sum()
    rho, kinds = hip_ctx.sq_modes(packed, hkl)
    assert hip_ctx.last_path() == "sq_modes" and list(kinds) == [7, 30]
    want = sq_ref.modes(packed.pos_host()[0], packed.cell[0], case["species"], 2, hkl)
    worst = _assert_within(rho, want, case["counts"], hkl, False, "shifted lattice (%s)" % name)
    print("shifted lattice (%s): rho off by at most %.3g = %.2f x 2^-24 per atom" % (name, worst, worst / X.U))
    got = hip_ctx.sq_accumulate(packed, case["hkl"], case["dq"], case["nbins"])
    assert hip_ctx.last_path() == "sq"
    ref = sq_ref.sq(packed, case["hkl"], case["dq"], case["nbins"])
    b = sq_ref.normalised(ref[0], ref[1], ref[3], packed.numbers)
    assert np.nanmax(b) > 100.0
    a = sq_ref.normalised(np.asarray(got[0], dtype=np.int64), got[1], got[3], packed.numbers)
    ok = ref[0] > 0
    err = np.abs(a[:, ok] - b[:, ok]) / np.maximum(1.0, np.abs(b[:, ok]))
    print("shifted lattice (%s): S off by %.3g relative (of %g), %.3g on the peaks above 100" % (name, err.max(), TOL, err[b[:, ok] > 100.0].max()))
    _compare_s(got, ref, packed.numbers)


def test_isf_self_of_a_generic_shift(hip_ctx):
    """8^3 lattice, every atom moved by a non-dyadic fractional vector d per frame: every atom's displacement phase is the
    same generic value, self / (n_w N) = cos(2 pi m hkl . d) with 512 coherent terms (the existing known answer moves by a
    quarter cell: phases that are exact)"""
    packed = C.isf_shifted_lattice(F=7)
    F, N = 7, 512
    hkl = np.array([[1, 0, 0], [2, 0, 0], [3, 0, 0], [1, 1, 0], [2, 1, 1], [5, 2, 0]])
    dq, nbins = 0.05, 50
    b = sq_ref.bins(sq_ref.reciprocal(C.CELL), hkl, dq, nbins)
    assert len(set(b.tolist())) == len(hkl) and (b < nbins).all()
    windows = [0, 1, 2, 3]
    got, scale, _ = _dev_call(hip_ctx, packed, hkl, windows, dq, nbins)
    assert hip_ctx.last_path() == "isf"
    s = int(isf_ref.pair_scale(scale, 1)[0, 0])
    bound = TERM_ERR + 2.0 * X.quant(hkl) + X.acc(N) / N + 2.0 ** (-s - 1) / N
    worst, worst_abs = 0.0, 0.0
    for w, m in enumerate(windows):
        n_w = F - m - 1
        assert (got["counts"][w][b] == n_w).all()
        value = np.ldexp(got["self"][0, w][b].astype(np.float64), -s) / (n_w * N)
        e = np.abs(value - np.cos(2.0 * np.pi * m * (hkl @ C.ISF_SHIFT)))
        worst, worst_abs = max(worst, float((e / bound).max())), max(worst_abs, float(e.max()))
        assert (e <= bound).all(), "lag %d: self off by %s, bound %s" % (m, e, bound)
    print("self part of a generic shift: off by at most %.3g, %.3g of the bound" % (worst_abs, worst))
