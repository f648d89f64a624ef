"""The inputs of the accuracy tests of the density modes (tests/test_sq_accuracy_cpu.py, tests/test_gpu_sq_accuracy.py): the
structures on which f32 errors add up instead of averaging away, and TERM_ERR, the measured error of one evaluated term.
Test infrastructure only; needs no GPU.  The budget is derived in tests/sq_exact_ref.py.

A case is a dict: packed (PackedTrajectory), u (uint32 [F][N][3], the fractional coordinates the library quantises the
positions to), kinds, species ([N], index into kinds), counts ([S]), hkl (int64 [K][3]), dyadic (u is exact: the positions
are u 2^-28 Angstrom in the cell diag(16, 16, 16), whose inverse is exactly 1/16)."""

import functools

import numpy as np

from amof_amd import structure_factor as sf
from amof_amd.frames import PackedTrajectory
from tests import helpers as H
from tests import sq_exact_ref as X

# The error of one term of rho on the MI355X, conversion included: |Re, Im of rho - exact| of a one-atom structure, where rho
# is a single v_cos_f32 / v_sin_f32 of (float)(int32)phi * 2^-32 converted exactly to f64 (test_single_terms).  Measured
# maxima, in units of 2^-24, over the 2 x 262 144 swept phases l G mod 2^32 and the 2 x 128 planted ones:
#     sweep    cos 2.980 (1.776e-7)   sin 2.931 (1.747e-7)
#     planted  cos 1.017 (6.061e-8)   sin 0.814 (4.854e-8)
# Twice the largest is 3.55e-7, so TERM_ERR = 2^-21 = 4.77e-7 (8 units).  Up to pi / 2 = 1.57 units of a swept term are the
# int-to-float conversion's.  The planted phases that f32 holds exactly (exact_in_f32: 2^k, the eighths of a revolution, their
# +-128 neighbours, ...) have no conversion error at all, so on them the instructions are measured by themselves:
#     exact    cos 1.017 (6.061e-8)   sin 0.797 (4.750e-8)      (2 x 105 phases, phase 0 included)
# TERM_ERR_EXACT, asserted on these phases only, is the smallest power of two that is at least their maximum, 2^-23 (2
# units).  It carries no factor of two: that factor stands for the inputs a sweep does not visit, and here the asserted
# inputs are the measured ones, every one of them, on deterministic instructions.  A conversion that is not the signed one
# (unsigned, with x in [0, 1)) rounds -2^31 + 128 to 2^31 and so errs by 2 pi 128 2^-32 = pi units there, inside TERM_ERR
# (it measures 4.37 units on the sweep) but outside TERM_ERR_EXACT: the exact phases are what pins the conversion.
# TERM_ERR is the smallest power of two that is at least twice the largest of the four (the sweep samples 5e5 of the about
# 2^30 distinct inputs); it cannot come out below MODEL_TERM = 2.07 x 2^-24, the bound with correctly rounded functions, and
# must not exceed 2^-19: with acc(64) / 64 = 1.94e-6 per atom a coherent peak's S would err by 2 (TERM_ERR + 1.94e-6), and
# beyond 2^-19 that leaves the 1e-5 contract no room.
TERM_ERR = 2.0 ** -21
TERM_ERR_EXACT = 2.0 ** -23
TERM_CEILING = 2.0 ** -19

CELL = np.diag([16.0, 16.0, 16.0])
SHEARED = np.array([[16.0, 0.0, 0.0], [8.0, 16.0, 0.0], [-4.0, 2.0, 32.0]])      # test_gpu_sq's sheared lattice cell
OFFSET = np.array([0.1234567, 0.7654321, 0.3141592])                              # a generic fractional offset
G0, G1 = 0x9E3779B1, 0x85EBCA6B                                                   # odd: l G mod 2^32 visits every residue


def _wrap32(v):
    """integers (any size) as the int32 with the same residue modulo 2^32"""
    v = np.array([int(x) % (1 << 32) for x in v], dtype=np.uint64)
    return v.astype(np.uint32).view(np.int32).astype(np.int64)


def _dyadic(u):
    """positions (Angstrom, exact in float64) of the uint32 coordinates u in the cell diag(16, 16, 16)"""
    return np.asarray(u, dtype=np.float64) * 2.0 ** -28


def _case(packed, u, hkl, dyadic):
    kinds, species = H.species_of(packed.numbers)
    hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3)
    assert (np.abs(hkl).sum(axis=1) > 0).all()
    return {"packed": packed, "u": np.asarray(u, dtype=np.uint32), "kinds": kinds, "species": species,
            "counts": np.bincount(species, minlength=len(kinds)), "hkl": hkl, "dyadic": dyadic}


def planted_phases():
    """the phases of the planted vectors (h, 0, 0) of single_term, as int32 values: h itself"""
    h = [1, -1, 2, -2, 3, -3]
    for k in range(8, 31):
        h += [2 ** k - 1, 2 ** k, 2 ** k + 1, -2 ** k]
    h.append(2 ** 24 + 1)                       # the first integer f32 cannot hold
    for j in range(8):                          # the eighths of a revolution and their neighbours
        h += [j * 2 ** 29 - 2 ** 31 + d for d in (0, 1, -1, 128, -128)]
    h += [2 ** 31 - 1, -2 ** 31]                # rounds to +1/2 revolution; -1/2 revolution
    h = np.unique(_wrap32(h))
    return h[h != 0]                            # (phase 0 comes from the vector (0, 1, 0))


def exact_in_f32(h):
    """mask of the int32 phases that (float)(int32)phi holds exactly (at most 24 significant bits)"""
    h = np.asarray(h, dtype=np.int64)
    return h.astype(np.float32).astype(np.int64) == h


N_SWEEP = 262144


@functools.lru_cache(maxsize=None)
def single_term():
    """two frames of one atom (Z = 29) at u = (1, 0, G): the vectors (0, 0, l), l = 1 .. 262 144, sweep the phases
    l G mod 2^32 (runs of 16 vectors, phi += uz inside a run), the vectors (h, 0, 0) plant the phase h itself (runs of one),
    (0, 1, 0) plants phase 0.  K = 262 144 + 127 + 1.  case["sweep"]: the mask of the swept vectors."""
    u = np.array([[[1, 0, G0]], [[1, 0, G1]]], dtype=np.uint32)
    sweep = np.zeros((N_SWEEP, 3), dtype=np.int64)
    sweep[:, 2] = np.arange(1, N_SWEEP + 1)
    h = planted_phases()
    planted = np.zeros((len(h) + 1, 3), dtype=np.int64)
    planted[:len(h), 0] = h
    planted[len(h)] = (0, 1, 0)
    case = _case(PackedTrajectory(_dyadic(u), CELL, [29]), u, np.vstack([sweep, planted]), True)
    case["sweep"] = np.arange(len(case["hkl"])) < N_SWEEP
    return case


COHERENT_COUNTS = {1: 1, 6: 63, 7: 64, 8: 65, 29: 129, 30: 512}      # Z: atoms; straddles the 64-atom partial
N_RANDOM = 4096


@functools.lru_cache(maxsize=None)
def coherent():
    """every atom of a species at one dyadic position: rho_s(k) = n_s exp(i theta) exactly, so every vector is maximally
    coherent.  N = 834 in shuffled order.  Vectors: 4096 random ones in [-64, 64]^3 (case["hkl"][:N_RANDOM]), then 200 rows
    (h, k, -10 .. 10) -- full runs, partial runs, and the row h = k = 0 broken at l = 0."""
    rng = np.random.default_rng(20261)
    numbers = np.repeat(list(COHERENT_COUNTS), list(COHERENT_COUNTS.values()))
    rng.shuffle(numbers)
    kinds, species = H.species_of(numbers)
    site = rng.integers(0, 1 << 32, size=(len(kinds), 3), dtype=np.uint64).astype(np.uint32)
    u = site[species][None]
    rand = np.zeros((0, 3), dtype=np.int64)
    while len(rand) < N_RANDOM:
        t = rng.integers(-64, 65, size=(N_RANDOM, 3))
        rand = np.vstack([rand, t[np.abs(t).sum(axis=1) > 0]])[:N_RANDOM]
    hk = np.vstack([[[0, 0]], rng.integers(-64, 65, size=(199, 2))])
    rows = np.array([(h, k, l) for h, k in hk for l in range(-10, 11) if (h, k, l) != (0, 0, 0)], dtype=np.int64)
    return _case(PackedTrajectory(_dyadic(u), CELL, numbers), u, np.vstack([rand, rows]), True)


QMAX = 3.6                  # reaches (8, 0, 0) in both cells: |q| = pi in the diagonal one, 3.55 in the sheared one
# bins narrow enough that a Bragg vector dominates its bin (S above 100): the sheared cell has twice the vectors, many of
# them close in |q|
DQ = {"diagonal": 0.02, "sheared": 0.002}


@functools.lru_cache(maxsize=None)
def shifted_lattice(name):
    """the 8 x 8 x 8 simple-cubic lattice of test_exact_known_answer_of_a_simple_cubic_lattice, rock-salt coloured (Z = 30
    where i + j + k is even, Z = 7 elsewhere: 256 each), every atom moved by the fractional OFFSET: a crystal whose phases
    are generic.  name: "diagonal" or "sheared".  hkl: the half space up to QMAX (sf.enumerate_hkl), which holds the Bragg
    vectors (h, k, l all multiples of 8: case["bragg"]); positions are not dyadic, the budget takes quant()."""
    cell = {"diagonal": CELL, "sheared": SHEARED}[name]
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3)
    numbers = np.where(g.sum(axis=1) % 2 == 0, 30, 7)
    pos = (g / 8.0 + OFFSET) @ cell
    packed = PackedTrajectory(pos[None], cell, numbers)
    case = _case(packed, X.quantize(pos, cell)[None], sf.enumerate_hkl(packed.cell, QMAX), False)
    case["bragg"] = (case["hkl"] % 8 == 0).all(axis=1)
    case["dq"] = DQ[name]
    case["nbins"] = sf.n_bins(QMAX, DQ[name])
    return case


def modes_subset(case, n_other=500, seed=5):
    """indices into case["hkl"] of shifted_lattice: every Bragg vector and n_other others"""
    other = np.flatnonzero(~case["bragg"])
    pick = np.random.default_rng(seed).choice(other, size=n_other, replace=False)
    return np.concatenate([np.flatnonzero(case["bragg"]), np.sort(pick)])


ISF_SHIFT = np.array([0.1234567, 0.0345, 0.0071])       # fractional, per frame: not dyadic


def isf_shifted_lattice(F=7):
    """test_self_part_of_a_uniformly_shifted_lattice's 8^3 lattice (Z = 29), every atom moved by f ISF_SHIFT in frame f"""
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij"), axis=-1).reshape(-1, 3) / 8.0
    pos = (g @ CELL)[None] + np.arange(F)[:, None, None] * (ISF_SHIFT @ CELL)[None, None, :]
    return PackedTrajectory(pos, CELL, [29] * 512)
