"""float64 numpy restatement of amof_current_modes and amof_current_accumulate (include/amof_hip.h), operation by operation:
the samples (finite differences of the u32 coordinates of tests/sq_exact_ref.quantize, or a velocity trajectory), the exact
phases at the midpoint, the modes j_a(k), the projection on k^ and the binned correlation sums; ``correlate`` with ``scale_log2`` builds, from
a table of modes the library itself returned, the int64 fixed-point sums the library must then produce bit for bit; ``brute``
is a double loop over atoms for the smallest cases.  Test infrastructure only (the package never imports it); needs no GPU."""

import numpy as np

from tests import helpers as H
from tests import isf_ref
from tests import sq_exact_ref as X
from tests import sq_ref

REV = 2.0 ** -32


def _cell_of(packed, f):
    cell = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3)
    return cell[f if len(cell) > 1 else 0]


def quantized(packed):
    """uint32 [F][N][3]: quantize_atom of every frame in its own cell"""
    pos = np.asarray(packed.pos_host(), dtype=np.float64)
    return np.stack([X.quantize(pos[f], _cell_of(packed, f)) for f in range(len(pos))])


def samples(packed, velocities=None, remove_com=True, u=None):
    """(v float64 [F][N][3], w float32 [F][N][3], p uint32 [F][N][3]) of the frames 1 .. F - 1 (frame 0: zeros): the sample
    before and after the rounding to float32, and its phase position.  ``velocities``: float64 [F][N][3] (velocity mode);
    ``u``: quantized(packed) where the caller has it."""
    u = quantized(packed) if u is None else np.asarray(u)
    F, N, _ = u.shape
    masses = np.asarray(packed.masses, dtype=np.float64)
    v = np.zeros((F, N, 3))
    p = np.zeros((F, N, 3), dtype=np.uint32)
    for f in range(1, F):
        if velocities is not None:
            v[f] = np.asarray(velocities, dtype=np.float64)[f]
            p[f] = u[f]
        else:
            d = (u[f] - u[f - 1]).view(np.int32)                  # uint32 wrap-around, read as signed
            s = d.astype(np.float64) * REV
            c = _cell_of(packed, f)
            v[f] = s[:, 0:1] * c[0][None, :] + s[:, 1:2] * c[1][None, :] + s[:, 2:3] * c[2][None, :]
            p[f] = u[f - 1] + (d >> 1).view(np.uint32)
        if remove_com:
            v[f] -= (masses[:, None] * v[f]).sum(axis=0) / masses.sum()
    return v, v.astype(np.float32), p


def modes(p, w, species, S, hkl):
    """j [K][S][3] complex128 of one frame: sum over the atoms of a species of w_j exp(2 pi i phi_j / 2^32), exact phases"""
    species = np.asarray(species)
    hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3)
    c, s = X.unit(X.phases(np.asarray(p, dtype=np.uint32), hkl))           # [K][N]
    e = c + 1j * s
    w = np.asarray(w, dtype=np.float64)
    j = np.zeros((len(hkl), S, 3), dtype=np.complex128)
    for a in range(S):
        sel = species == a
        j[:, a, :] = e[:, sel] @ w[sel]
    return j


def khat(recip, hkl):
    """[K][3]: q / |q| in the library's operation order (float64, no fma)"""
    r = np.asarray(recip, dtype=np.float64).reshape(3, 3)
    h = np.asarray(hkl, dtype=np.float64).reshape(-1, 3)
    q = np.stack([(h[:, 0] * r[0, c] + h[:, 1] * r[1, c]) + h[:, 2] * r[2, c] for c in range(3)], axis=1)
    n = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
    return q / n[:, None]


def project(j, u):
    """(L [K][S] complex, T [K][S][3] complex) of j [K][S][3] on u [K][3]: real and imaginary parts separately, the
    library's order"""
    def part(x):
        L = (u[:, None, 0] * x[:, :, 0] + u[:, None, 1] * x[:, :, 1]) + u[:, None, 2] * x[:, :, 2]
        return L, x - u[:, None, :] * L[:, :, None]
    Lr, Tr = part(j.real)
    Li, Ti = part(j.imag)
    return Lr + 1j * Li, Tr + 1j * Ti


def products(L0, T0, L1, T1):
    """(t_L [K][S][S], t_T [K][S][S]) of an origin's and a partner's projections, a at the origin, c at the partner"""
    tl = L0.real[:, :, None] * L1.real[:, None, :] + L0.imag[:, :, None] * L1.imag[:, None, :]

    def dot(c):
        return T0.real[:, :, None, c] * T1.real[:, None, :, c] + T0.imag[:, :, None, c] * T1.imag[:, None, :, c]
    return tl, (dot(0) + dot(1)) + dot(2)


def _recips(packed):
    return sq_ref_reciprocals(np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3))


def sq_ref_reciprocals(cells):
    from amof_amd import _hip
    return np.ascontiguousarray(_hip.reciprocal(cells))


def correlate(jm, recips, hkl, windows, dq, nbins, origin_stride=1, work_range=None, scale_log2=None):
    """(counts [W][nbins] int64, long [S][S][W][nbins], trans [S][S][W][nbins], beyond [W] int64) from modes jm
    [F][K][S][3] (frame 0 unused).  scale_log2 None: float64 sums.  scale_log2 [P]: the library's int64 sums, rint of the
    product times 2^s of the unordered pair, from ITS modes bit for bit."""
    jm = np.asarray(jm)
    F, K, S, _ = jm.shape
    W = len(windows)
    recips = np.asarray(recips).reshape(-1, 3, 3)
    rec = lambda f: recips[f if len(recips) > 1 else 0]
    fixed = scale_log2 is not None
    scale = np.ldexp(1.0, isf_ref.pair_scale(scale_log2, S)) if fixed else None
    dtype = np.int64 if fixed else np.float64
    counts = np.zeros((W, nbins), dtype=np.int64)
    lng, trn = np.zeros((S, S, W, nbins), dtype=dtype), np.zeros((S, S, W, nbins), dtype=dtype)
    beyond = np.zeros(W, dtype=np.int64)
    proj = {}

    def projected(f):
        if f not in proj:
            proj[f] = project(jm[f], khat(rec(f), hkl))
        return proj[f]
    for w, k in isf_ref.work_entries(F, windows, origin_stride, work_range):
        m = int(windows[w])
        b = sq_ref.bins(rec(k), hkl, dq, nbins)
        ok = b < nbins
        beyond[w] += int((~ok).sum())
        counts[w] += np.bincount(b[ok], minlength=nbins)
        tl, tt = products(*(projected(k) + projected(k + m)))
        for a in range(S):
            for c in range(S):
                if fixed:
                    np.add.at(lng[a, c, w], b[ok], np.rint(tl[ok, a, c] * scale[a, c]).astype(np.int64))
                    np.add.at(trn[a, c, w], b[ok], np.rint(tt[ok, a, c] * scale[a, c]).astype(np.int64))
                else:
                    lng[a, c, w] += np.bincount(b[ok], weights=tl[ok, a, c], minlength=nbins)
                    trn[a, c, w] += np.bincount(b[ok], weights=tt[ok, a, c], minlength=nbins)
    return counts, lng, trn, beyond


def all_modes(packed, hkl, velocities=None, remove_com=True, u=None):
    """(jm [F][K][S][3] complex, w float32 [F][N][3], kinds): the reference modes of every frame (frame 0: zeros)"""
    kinds, species = H.species_of(packed.numbers)
    _, w, p = samples(packed, velocities, remove_com, u)
    F = len(w)
    jm = np.zeros((F, len(hkl), len(kinds), 3), dtype=np.complex128)
    for f in range(1, F):
        jm[f] = modes(p[f], w[f], species, len(kinds), hkl)
    return jm, w, kinds


def current(packed, hkl, windows, dq, nbins, origin_stride=1, work_range=None, velocities=None, remove_com=True, u=None):
    """(counts, long, trans, beyond, kinds, vmax): amof_current_accumulate in float64"""
    jm, w, kinds = all_modes(packed, hkl, velocities, remove_com, u)
    out = correlate(jm, _recips(packed), hkl, windows, dq, nbins, origin_stride, work_range)
    return out + (kinds, float(np.abs(w[1:]).max()) if len(w) > 1 and w[1:].size else 0.0)


def brute(packed, hkl, windows, dq, nbins, origin_stride=1, velocities=None, remove_com=True):
    """the same sums by a double loop over atoms (no modes): sum_ij of the projected velocities times
    cos(phase_i(k) - phase_j(k + m)), for the smallest cases"""
    kinds, species = H.species_of(packed.numbers)
    S, W = len(kinds), len(windows)
    _, w, p = samples(packed, velocities, remove_com)
    w = w.astype(np.float64)
    F, N, _ = w.shape
    hkl = np.asarray(hkl, dtype=np.int64).reshape(-1, 3)
    recips = _recips(packed)
    rec = lambda f: recips[f if len(recips) > 1 else 0]
    counts = np.zeros((W, nbins), dtype=np.int64)
    lng, trn = np.zeros((S, S, W, nbins)), np.zeros((S, S, W, nbins))
    beyond = np.zeros(W, dtype=np.int64)
    for wi, k in isf_ref.work_entries(F, windows, origin_stride):
        m = int(windows[wi])
        b = sq_ref.bins(rec(k), hkl, dq, nbins)
        u0, u1 = khat(rec(k), hkl), khat(rec(k + m), hkl)
        ph0 = X.phases(p[k], hkl).astype(np.float64) * (2.0 * np.pi * REV)       # [K][N]
        ph1 = X.phases(p[k + m], hkl).astype(np.float64) * (2.0 * np.pi * REV)
        for v in range(len(hkl)):
            if b[v] >= nbins:
                beyond[wi] += 1
                continue
            counts[wi, b[v]] += 1
            for i in range(N):
                li = float(u0[v] @ w[k, i])
                ti = w[k, i] - u0[v] * li
                for j in range(N):
                    lj = float(u1[v] @ w[k + m, j])
                    tj = w[k + m, j] - u1[v] * lj
                    c = np.cos(ph0[v, i] - ph1[v, j])
                    lng[species[i], species[j], wi, b[v]] += li * lj * c
                    trn[species[i], species[j], wi, b[v]] += float(ti @ tj) * c
    return counts, lng, trn, beyond, kinds
