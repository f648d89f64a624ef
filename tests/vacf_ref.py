"""numpy restatement of amof_vacf_window (include/amof_hip.h): the wrapped steps of the window MSD (or a velocity trajectory
minus the frame's mean), multiplied at the family's lags and origins.  Test infrastructure only (the package never imports
it)."""

import numpy as np

from amof_amd import lags
from tests import helpers as H
from tests import vanhove_ref

REL = 1e-9      # |gpu - ref| <= REL * abs_sums: the MSD's bound for its sums, applied to the sum that does not cancel


def steps(packed, remove_com=True):
    """x [F][N][3]: x[k] the wrapped step from frame k - 1 to frame k (x[0] = 0), through the Van Hove restatement's
    running positions (oracle.numpy_oracle.get_delta_pos)"""
    u = vanhove_ref.running_positions(packed, remove_com=remove_com)
    x = np.zeros_like(u)
    x[1:] = np.diff(u, axis=0)
    return x


def velocities(packed, remove_com=True):
    """x [F][N][3]: the trajectory's own values minus the mass-weighted mean of every frame"""
    x = np.array(packed.pos_host(), dtype=np.float64)
    if remove_com:
        masses = np.asarray(packed.masses, dtype=np.float64)
        x = x - (np.einsum("a,kac->kc", masses, x) / masses.sum())[:, None, :]
    return x


def correlate(x, numbers, windows, origin_stride=1, atom_range=None):
    """(sums [S][W], n_origins [W], abs_sums [S][W], kinds): sums of x(k) x(k + m) and of |x(k) x(k + m)| over the atoms of
    ``atom_range``, the coordinates and lags.origins -- species in library order"""
    kinds, sp = H.species_of(numbers)
    F, N = x.shape[0], x.shape[1]
    a0, a1 = (0, N) if atom_range is None else atom_range
    S, W = len(kinds), len(windows)
    sums, abs_sums = np.zeros((S, W)), np.zeros((S, W))
    n = np.zeros(W, dtype=np.int64)
    in_range = (np.arange(N) >= a0) & (np.arange(N) < a1)
    for w, m in enumerate(windows):
        k = lags.origins(F, int(m), origin_stride)
        n[w] = len(k)
        prod = (x[k] * x[k + int(m)]).sum(axis=(0, 2)) if len(k) else np.zeros(N)
        aprod = np.abs(x[k] * x[k + int(m)]).sum(axis=(0, 2)) if len(k) else np.zeros(N)
        for s in range(S):
            sel = (sp == s) & in_range
            sums[s, w], abs_sums[s, w] = prod[sel].sum(), aprod[sel].sum()
    return sums, n, abs_sums, kinds


def vacf(packed, windows, origin_stride=1, velocity_mode=False, remove_com=True, atom_range=None):
    x = velocities(packed, remove_com) if velocity_mode else steps(packed, remove_com)
    return correlate(x, packed.numbers, windows, origin_stride, atom_range)


def check(got, want, rel=REL):
    """got [S][W] against (sums, n_origins, abs_sums, kinds)"""
    sums, _, abs_sums, _ = want
    err = np.abs(np.asarray(got) - sums)
    assert (err <= rel * abs_sums).all(), "worst error / abs_sums: %.3g" % float(np.max(err / np.maximum(abs_sums, 1e-300)))
