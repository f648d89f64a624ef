"""The derived error budget of the current modes j_a(k) (amof_current_modes, current_rho_kernel in amof_amd/csrc/current.hip)
against the exact-phase reference tests/current_ref.py, built as tests/sq_exact_ref.budget is.  Test infrastructure only;
needs no GPU.

The kernel, per atom j and vector: the exact u32 phase phi of the midpoint -> (float)(int32)phi * 2^-32 -> v_cos_f32 /
v_sin_f32 -> p = fmaf(w_j, cos or sin, p), w_j the f32 sample, into an f32 partial that covers at most SQ_BLOCK atoms of one
species -> folded into f64.  The reference evaluates the same sum with the same u32 coordinates (quantize_atom restated), the
float32 samples and float64 functions.

Budget per real and imaginary part of component c of j_a(k), the species' atoms j = 1 .. n, W = sum_j |w_j|, M = max_j |w_j|:
    budget = W (term + round_w + quant(hkl)) + M acc(n) + n vquant
  term     the error of one evaluated cos or sin, conversion included: TERM_ERR of tests/sq_accuracy_cases.py, measured for
           these same instructions on these same arguments.  Every term is multiplied by |w_j| <= its share of W.
  round_w  the f32 rounding of the sample.  Kernel and reference both round to float32, but from float64 values that differ
           in their last bits (fma chain against products and adds, the order of the mean's sum): a value next to a rounding
           boundary may fall to the other side, one ulp of w: 2^-23 |w_j|.
  quant    quantize_atom's coordinates may differ from the restatement's by two units of 2^-32 each (sq_exact_ref.quant); the
           midpoint inherits at most that: the phase moves by quant(hkl), the term by |w_j| quant(hkl).
  acc      one rounding per fma: the k-th fmaf of a partial rounds a sum of magnitude <= k M, at most 2^-24 k M (the product
           inside an fma is exact, so this is the only rounding; unlike a plain add to zero the first one rounds too).  Over a
           partial of m terms 2^-24 M m (m + 1) / 2; partial lengths SQ_BLOCK, .., n mod SQ_BLOCK.  The f64 fold: nothing.
  vquant   positions mode: the step is the difference of two quantised coordinates, each up to two units of 2^-32 from the
           restatement's: four units per fractional component, 4 2^-32 sum_i |C[i][c]| in Cartesian component c, on each of
           the n terms (|cos|, |sin| <= 1).  Velocity mode: 0.
The projections are float64 on both sides: |dL| <= sum_c |k^_c| budget_c <= sqrt(3) max_c budget_c, and the same bound holds
for every component of dT = dj - k^ dL taken as |dj_c| + |k^_c| |dL|."""

import numpy as np

from tests import sq_exact_ref as X
from tests.sq_accuracy_cases import TERM_ERR

U = X.U
ROUND_W = 2.0 ** -23


def acc(n):
    """sum over the partials of m (m + 1) / 2, in units of 2^-24 M"""
    full, rest = divmod(int(n), X.SQ_BLOCK)
    return U * (full * (X.SQ_BLOCK * (X.SQ_BLOCK + 1) // 2) + rest * (rest + 1) // 2)


def vquant(cell):
    """[3]: the Cartesian error of a step from four units of 2^-32 per fractional component"""
    return 4.0 * 2.0 ** -32 * np.abs(np.asarray(cell, dtype=np.float64).reshape(3, 3)).sum(axis=0)


def budget(w, species, S, hkl, cell=None):
    """[K][S][3]: the bound on |got - reference| of the real and of the imaginary part of j_a(k)[c]; w: the float32 samples
    [N][3] of the frame; cell: the frame's cell in positions mode, None in velocity mode"""
    w = np.abs(np.asarray(w, dtype=np.float64))
    species = np.asarray(species)
    q = X.quant(hkl)                                                # [K]
    vq = vquant(cell) if cell is not None else np.zeros(3)
    out = np.zeros((len(q), S, 3))
    for a in range(S):
        sel = species == a
        n = int(sel.sum())
        if n == 0:
            continue
        W, M = w[sel].sum(axis=0), w[sel].max(axis=0)               # [3]
        out[:, a, :] = W[None, :] * (TERM_ERR + ROUND_W + q[:, None]) + (M * acc(n) + n * vq)[None, :]
    return out


def projected(b):
    """([K][S] bound on |dL| real or imaginary, [K][S][3] bound on |dT|) from budget b [K][S][3], for any unit vector k^"""
    dl = np.sqrt(3.0) * b.max(axis=2)
    return dl, b + dl[:, :, None]
