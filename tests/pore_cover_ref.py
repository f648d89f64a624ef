"""Pure-numpy restatement of the covering radius of include/amof_hip.h (amof_pore_psd), written from the definitions; it never
calls the product, and it is another algorithm than the library's brick path: one gather over the WHOLE grid per integer
offset -- ``np.roll`` along periodic axes, a shift that lets nothing in along open ones -- for every offset of a bounding box
with one step of slack, with exactly the documented arithmetic:

    A_k[c] = C[k][c] / n_k,   s_c = (Di A_0[c] + Dj A_1[c]) + Dk A_2[c],   d2 = (s_x s_x + s_y s_y) + s_z s_z
    c = p + D covers p  iff  v(c) >= 0 and d2(D) <= v(c) v(c);   w(p) = max v(c) over the covering centres, v(p) without one
"""

import numpy as np


def step_vectors(cell, n):
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    return np.stack([cell[k] / np.float64(n[k]) for k in range(3)])


def offset_d2(A, di, dj, dk):
    s = (np.float64(di) * A[0] + np.float64(dj) * A[1]) + np.float64(dk) * A[2]
    return (s[0] * s[0] + s[1] * s[1]) + s[2] * s[2]


def reach(A, vmax):
    """per axis the largest |offset| a sphere of radius vmax can span, plus one step of slack"""
    faces = [np.cross(A[1], A[2]), np.cross(A[2], A[0]), np.cross(A[0], A[1])]
    vol = abs(float(A[0] @ faces[0]))
    return [int(np.ceil(vmax * np.sqrt(f @ f) / vol)) + 1 for f in faces]


def _shift(a, d, axis, periodic, fill):
    """``out[p] = a[p + d]`` along one axis: modulo n on a periodic axis, ``fill`` where an open axis has no such point"""
    out = np.roll(a, -d, axis=axis)
    if not periodic and d != 0:
        n = a.shape[axis]
        idx = [slice(None)] * a.ndim
        idx[axis] = slice(max(n - d, 0), None) if d > 0 else slice(0, min(-d, n))
        out[tuple(idx)] = fill
    return out


def covering(field, cell, pbc=(True, True, True), centres=None):
    """``best [nx][ny][nz]``: the largest v(c) over the centres that cover a point, -inf where none does.  ``centres``: a
    boolean mask of the grid points that may serve as centres (None: all)."""
    v = np.asarray(field, dtype=np.float64)
    n = v.shape
    A = step_vectors(cell, n)
    src = np.where(v >= 0.0, v, -1.0)               # (a negative value covers nothing)
    if centres is not None:
        src = np.where(np.asarray(centres, dtype=bool), src, -1.0)
    best = np.full(n, -np.inf)
    vmax = float(src.max())
    if vmax < 0.0:
        return best
    R = reach(A, vmax)
    top = np.float64(vmax) * np.float64(vmax)
    for di in range(-R[0], R[0] + 1):
        s0 = _shift(src, di, 0, pbc[0], -1.0)
        for dj in range(-R[1], R[1] + 1):
            s1 = _shift(s0, dj, 1, pbc[1], -1.0)
            for dk in range(-R[2], R[2] + 1):
                d2 = offset_d2(A, di, dj, dk)
                if not d2 <= top:
                    continue
                vc = _shift(s1, dk, 2, pbc[2], -1.0)
                hit = (vc >= 0.0) & (d2 <= vc * vc)
                best = np.where(hit & (vc > best), vc, best)
    return best


def cover(field, cell, pbc=(True, True, True)):
    """the covering radius w of one frame"""
    v = np.asarray(field, dtype=np.float64)
    best = covering(v, cell, pbc)
    return np.where(best >= 0.0, best, v)


def nbins_of(dr, dmax):
    return int(np.rint(dmax / dr))


def histogram(w, dr, dmax):
    """u64 [nbins + 2]: w < 0, b = (int)(w / dr) for 0 <= w < dmax (b < nbins), the rest"""
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    nbins = nbins_of(dr, dmax)
    row = np.zeros(nbins + 2, dtype=np.uint64)
    row[0] = (w < 0.0).sum()
    inside = w[(w >= 0.0) & (w < dmax)]
    b = (inside / np.float64(dr)).astype(np.int64)
    row[1:nbins + 1] = np.bincount(b[b < nbins], minlength=nbins)
    row[nbins + 1] = w.size - int(row[:nbins + 1].sum())
    return row


def covered_from_channels(field, cell, pbc, labels, comps):
    """points covered by at least one centre whose component (``labels``, ``comps`` of tests/pore_access_ref.py ``components``)
    is a channel"""
    channels = [c[0] for c in comps if c[2] > 0]
    if not channels:
        return 0
    best = covering(field, cell, pbc, centres=np.isin(labels, channels))
    return int((best >= 0.0).sum())


def psd(field, cell, pbc, dr, dmax, thresholds, access=False):
    """``(w, psd_hist u64 [nbins + 2], po_counts int64 [n_t], po_access int64 [n_t] or None)`` of one frame"""
    from tests import pore_access_ref
    v = np.asarray(field, dtype=np.float64)
    w = cover(v, cell, pbc)
    po = np.array([(w >= np.float64(t)).sum() for t in thresholds], dtype=np.int64)
    acc = None
    if access:
        acc = np.zeros(len(thresholds), dtype=np.int64)
        for k, t in enumerate(thresholds):
            labels, comps = pore_access_ref.components(v >= np.float64(t), tuple(bool(x) for x in pbc))
            acc[k] = covered_from_channels(v, cell, pbc, labels, comps)
    return w, histogram(w, dr, dmax), po, acc
