"""The exact-phase reference of the density modes rho_a(k) (amof_sq_modes, sq_rho_kernel in amof_amd/csrc/sq.hip), the
derived error budget of the kernel's f32 chain, and a numpy emulation of that chain.  Test infrastructure only (the package
never imports it); needs no GPU.

The kernel, per atom and vector: the exact u32 phase phi -> (float)(int32)phi * 2^-32 revolutions in [-1/2, 1/2] ->
v_cos_f32 / v_sin_f32 -> added into an f32 partial that covers at most SQ_BLOCK atoms of one species -> folded into f64.

Budget per real and imaginary component of rho_a(k), n atoms in the species:
    budget = n term + acc(n) [+ n quant(hkl) where the coordinates are not exact multiples of 2^-32]
  term   the error of one evaluated term, conversion included.  With correctly rounded functions (MODEL_TERM): half an ulp
         of a result <= 1, 2^-25, plus 2 pi times the conversion's 2^-26 revolutions (half an ulp of an integer below 2^31,
         2^6, times 2^-32): (1/2 + pi/2) 2^-24.  For the hardware: TERM_ERR of tests/sq_accuracy_cases.py, measured.
  acc    the k-th add of a partial (k = 2 .. m; the first one adds to zero and is exact) rounds a sum of magnitude <= k:
         at most 2^-24 k.  Over a partial of m terms: 2^-24 (m (m + 1) / 2 - 1); partial lengths SQ_BLOCK, .., n mod SQ_BLOCK.
         (The f64 fold adds <= 2^-53 n per partial: nothing.)
  quant  quantize_atom truncates a coordinate to 2^-32 after a float64 fma chain: two units of 2^-32 per coordinate, so
         2 pi 2 (|h| + |k| + |l|) 2^-32 per atom."""

import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24          # the unit the error figures are quoted in: one ulp of an f32 in [1/2, 1)
MODEL_TERM = (0.5 + np.pi / 2.0) * U


def _sq_block():
    with open(os.path.join(ROOT, "amof_amd", "csrc", "sq_plan.h")) as fh:
        m = re.search(r"constexpr\s+int\s+SQ_BLOCK\s*=\s*(\d+)\s*;", fh.read())
    assert m, "sq_plan.h no longer defines SQ_BLOCK as a plain constant: the budget must follow the kernel's partial length"
    return int(m.group(1))


SQ_BLOCK = _sq_block()      # atoms per f32 partial: the kernel's own constant, so that acc() follows a change of it


def acc(n):
    """bound on the f32 accumulation error of one species of n atoms, per component"""
    n = int(n)
    full, rest = divmod(n, SQ_BLOCK)
    adds = full * (SQ_BLOCK * (SQ_BLOCK + 1) // 2 - 1) + (rest * (rest + 1) // 2 - 1 if rest else 0)
    return U * adds


def quant(hkl):
    """[K]: the phase a vector can gain from the quantisation of one atom's coordinates (two units of 2^-32 each)"""
    hkl = np.asarray(hkl, dtype=np.float64).reshape(-1, 3)
    return 2.0 * np.pi * 2.0 * np.abs(hkl).sum(axis=1) * 2.0 ** -32


def budget(n, hkl, term, dyadic):
    """[K]: the bound on |got - exact| of Re and of Im rho_a(k) for a species of n atoms"""
    return n * float(term) + acc(n) + (0.0 if dyadic else n * quant(hkl))


def phases(u, hkl):
    """[K][N] uint64 in [0, 2^32): (h ux + k uy + l uz) mod 2^32 in exact integer arithmetic (negative indices reduced
    modulo 2^32 first: every product of two residues fits a uint64)"""
    u = np.asarray(u)
    assert u.dtype == np.uint32 and u.ndim == 2 and u.shape[1] == 3
    u = u.astype(np.uint64)
    m = np.uint64(0xffffffff)
    r = (np.asarray(hkl, dtype=np.int64).reshape(-1, 3) % (1 << 32)).astype(np.uint64)
    ph = np.zeros((len(r), len(u)), dtype=np.uint64)
    for c in range(3):
        ph += (r[:, c, None] * u[None, :, c]) & m
    return ph & m


def unit(ph):
    """(cos, sin) of 2 pi ph / 2^32 in float64 for exact integer phases ph in [0, 2^32).  The phase is split exactly into
    the nearest quarter revolution and a rest in [-2^29, 2^29): the functions see |argument| <= pi / 4, where the rounding of
    the argument is below 1e-16, and the quarter turns are swaps and signs -- about 2e-16 per value, exact on the axes."""
    ph = np.asarray(ph, dtype=np.uint64)
    q = (ph + np.uint64(1 << 29)) >> np.uint64(30)              # 0 .. 4
    r = ph.astype(np.int64) - (q.astype(np.int64) << 30)        # [-2^29, 2^29)
    a = r.astype(np.float64) * (np.pi * 2.0 ** -31)
    c, s = np.cos(a), np.sin(a)
    q = q & np.uint64(3)
    cos = np.where(q == 0, c, np.where(q == 1, -s, np.where(q == 2, -c, s)))
    sin = np.where(q == 0, s, np.where(q == 1, c, np.where(q == 2, -s, -c)))
    return cos + 0.0, sin + 0.0                                  # (no negative zeros)


def modes_exact(u, species, S, hkl, chunk=2048):
    """rho [K][S] complex128: sum over the atoms of species a of exp(2 pi i phi / 2^32) with the exact integer phase of the
    uint32 fractional coordinates u [N][3] (float64 sums of at most a few hundred terms of about 2e-16 each)"""
    species = np.asarray(species)
    hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3)
    rho = np.zeros((len(hkl), S), dtype=np.complex128)
    for c0 in range(0, len(hkl), chunk):
        c, s = unit(phases(u, hkl[c0:c0 + chunk]))
        for a in range(S):
            sel = species == a
            rho[c0:c0 + chunk, a] = c[:, sel].sum(axis=1) + 1j * s[:, sel].sum(axis=1)
    return rho


def model(u, species, S, hkl):
    """rho [K][S] complex128 of the documented chain with correctly rounded functions: u32 phase (wrap-around), signed
    int32 -> float32 (round to nearest even), times 2^-32 in float32, cos and sin of 2 pi x in float64 rounded to float32,
    sequential float32 partials of SQ_BLOCK atoms per species (the atoms of a species in input order, the library's stable
    species permutation), folded into float64."""
    u = np.asarray(u)
    assert u.dtype == np.uint32
    species = np.asarray(species)
    r = (np.asarray(hkl, dtype=np.int64).reshape(-1, 3) % (1 << 32)).astype(np.uint32)
    rev = np.float32(2.0 ** -32)
    rho = np.zeros((len(r), S), dtype=np.complex128)
    with np.errstate(over="ignore"):
        for a in range(S):
            atoms = np.flatnonzero(species == a)
            re, im = np.zeros(len(r)), np.zeros(len(r))
            for b0 in range(0, len(atoms), SQ_BLOCK):
                pr, pi = np.zeros(len(r), dtype=np.float32), np.zeros(len(r), dtype=np.float32)
                for j in atoms[b0:b0 + SQ_BLOCK]:
                    phi = r[:, 0] * u[j, 0] + r[:, 1] * u[j, 1] + r[:, 2] * u[j, 2]           # uint32: wraps
                    x = phi.view(np.int32).astype(np.float32) * rev
                    t = 2.0 * np.pi * x.astype(np.float64)
                    pr = pr + np.cos(t).astype(np.float32)
                    pi = pi + np.sin(t).astype(np.float32)
                assert pr.dtype == np.float32 and pi.dtype == np.float32
                re += pr.astype(np.float64)
                im += pi.astype(np.float64)
            rho[:, a] = re + 1j * im
    return rho


def inverse(cell):
    """inv(cell) [3][3] by cofactors over the determinant, the library's own formula (ctx.hip: geom_one)"""
    c = [float(x) for x in np.asarray(cell, dtype=np.float64).reshape(9)]
    m00 = c[4] * c[8] - c[5] * c[7]
    m01 = c[3] * c[8] - c[5] * c[6]
    m02 = c[3] * c[7] - c[4] * c[6]
    det = c[0] * m00 - c[1] * m01 + c[2] * m02
    inv = [(c[4] * c[8] - c[5] * c[7]) / det, (c[2] * c[7] - c[1] * c[8]) / det, (c[1] * c[5] - c[2] * c[4]) / det,
           (c[5] * c[6] - c[3] * c[8]) / det, (c[0] * c[8] - c[2] * c[6]) / det, (c[2] * c[3] - c[0] * c[5]) / det,
           (c[3] * c[7] - c[4] * c[6]) / det, (c[1] * c[6] - c[0] * c[7]) / det, (c[0] * c[4] - c[1] * c[3]) / det]
    return np.array(inv).reshape(3, 3)


def _fma(a, b, c):
    """float64 fma: the exact a b + c (rationals), rounded once"""
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def quantize(pos, cell):
    """uint32 [N][3]: quantize_atom (amof_internal.h) restated in float64, operation for operation:
    s_c = fma(z, inv[2][c], fma(y, inv[1][c], x inv[0][c])), s -= floor(s), u = trunc(s 2^32) (saturating)"""
    inv = inverse(cell)
    pos = np.asarray(pos, dtype=np.float64).reshape(-1, 3)
    out = np.zeros(pos.shape, dtype=np.uint32)
    for i, (x, y, z) in enumerate(pos.tolist()):
        for c in range(3):
            s = _fma(z, inv[2, c], _fma(y, inv[1, c], x * inv[0, c]))
            s = s - np.floor(s)
            t = s * 4294967296.0
            out[i, c] = 0xffffffff if t >= 4294967295.0 else int(t)
    return out
