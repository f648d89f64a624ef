"""Current correlation functions C_L(q, t) and C_T(q, t) on MI355X, and what is read from them.

``CurrentCorrelation`` is the collective counterpart of ``VelocityAutocorrelation``: the time correlation of the particle
current j_a(k, t) = sum_j v_j(t) exp(i k . r_j(t)) on the reciprocal-lattice vectors of ``StructureFactor``, projected along k
(longitudinal) and across it (transverse), over the lags and origins of the dynamics family (amof_amd/lags.py).  The spectra
C_L(q, omega) and C_T(q, omega) carry the acoustic dispersion; the slopes of their maxima at small q are the longitudinal and
transverse sound velocities, and with the density the longitudinal, shear and bulk moduli -- an independent route to the
mechanical numbers of a trajectory.  The modes and the correlation run in the HIP kernels behind ``amof_current_accumulate``
(amof_amd/csrc/current.hip; exact u32 phases, int64 fixed-point sums); the host keeps the choice of vectors, the normalisation, the
Fourier transform and the DataFrames.  The reference has no such analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import data as _data
from . import lag_q
from . import lags
from .files import path as _path
from .frames import PackedTrajectory

logger = logging.getLogger(__name__)

THZ_PER_INVERSE_FS = 1.0e3
M_PER_S_PER_ANGSTROM_PER_FS = 1.0e5
KG_PER_M3_PER_AMU_PER_A3 = 1660.53906660


def column_names(elements):
    """``Time, q, X-X-L, X-X-T``, then ``A-B-L, A-B-T`` of every ordered pair (``IntermediateScattering``'s order)"""
    syms = [_data.chemical_symbols[int(z)] for z in elements]
    return ["Time", "q", "X-X-L", "X-X-T"] + [a + "-" + b + "-" + p for a in syms for b in syms for p in ("L", "T")]


def assemble(counts, long_sums, trans_sums, kinds, elements, species_counts, time, dq, timestep=1):
    """``.data`` from the raw outputs of ``amof_current_accumulate`` (counts [W][nbins], long_sums and trans_sums
    [S][S][W][nbins] in Angstrom^2 per frame^2, library species order ``kinds``); ``elements``: atomic numbers in column order;
    ``species_counts``: {atomic number: atoms}; ``timestep``: fs per frame (1 where the samples already are velocities).
      Time, q     the lag's time, the left bin edge b dq; W x nbins rows stacked by lag
      X-X-L       sum_ac long_ac / (counts N timestep^2): the number current per atom;  X-X-T the same of trans, halved
      A-B-L       long_AB / (counts sqrt(N_A N_B) timestep^2), A at the origin, B at the origin + lag (Ashcroft-Langreth);
      A-B-T       trans_AB likewise, halved (two transverse directions)
    Bins with no samples are NaN."""
    counts = np.asarray(counts, dtype=np.float64)
    lng, trn = np.asarray(long_sums, dtype=np.float64), np.asarray(trans_sums, dtype=np.float64)
    W, nbins = counts.shape
    N = float(sum(species_counts[int(z)] for z in kinds))
    denom = np.where(counts > 0, counts, np.nan) * float(timestep) ** 2
    idx = {int(z): k for k, z in enumerate(kinds)}
    cols = {"Time": np.repeat(np.asarray(time, dtype=np.float64), nbins),
            "q": np.tile(np.arange(nbins, dtype=np.float64) * dq, W)}
    cols["X-X-L"] = (lng.sum(axis=(0, 1)) / (denom * N)).reshape(-1)
    cols["X-X-T"] = (0.5 * trn.sum(axis=(0, 1)) / (denom * N)).reshape(-1)
    syms = [_data.chemical_symbols[int(z)] for z in elements]
    for i, zi in enumerate(elements):
        for j, zj in enumerate(elements):
            norm = np.sqrt(float(species_counts[int(zi)]) * float(species_counts[int(zj)]))
            a, c = idx[int(zi)], idx[int(zj)]
            cols[syms[i] + "-" + syms[j] + "-L"] = (lng[a, c] / (denom * norm)).reshape(-1)
            cols[syms[i] + "-" + syms[j] + "-T"] = (0.5 * trn[a, c] / (denom * norm)).reshape(-1)
    return pd.DataFrame(cols)


def combine(counts, long_sums, trans_sums, w, species_n, time, dq, timestep=1):
    """``DataFrame`` Time, q, L, T: sum over ordered pairs of w_a w_c sums_ac / (counts sum_a N_a w_a^2 timestep^2), T halved;
    w [S] weights and species_n [S] atoms in the order of the sums"""
    counts = np.asarray(counts, dtype=np.float64)
    W, nbins = counts.shape
    w = np.asarray(w, dtype=np.float64)
    ww = w[:, None] * w[None, :]
    norm = float((np.asarray(species_n, dtype=np.float64) * w * w).sum())
    with np.errstate(divide="ignore", invalid="ignore"):
        denom = np.where(counts > 0, counts, np.nan) * norm * float(timestep) ** 2
        L = (ww[:, :, None, None] * np.asarray(long_sums, dtype=np.float64)).sum(axis=(0, 1)) / denom
        T = 0.5 * (ww[:, :, None, None] * np.asarray(trans_sums, dtype=np.float64)).sum(axis=(0, 1)) / denom
    return pd.DataFrame({"Time": np.repeat(np.asarray(time, dtype=np.float64), nbins),
                         "q": np.tile(np.arange(nbins, dtype=np.float64) * dq, W), "L": L.reshape(-1), "T": T.reshape(-1)})


normalise = lag_q.normalise


def lag_spacing(time):
    """the spacing of evenly spaced lags from 0 (ValueError otherwise)"""
    t = np.asarray(time, dtype=np.float64)
    if len(t) < 2:
        raise ValueError("a spectrum needs at least two lags")
    dt = float(t[1] - t[0])
    if t[0] != 0 or not dt > 0 or not np.allclose(t, dt * np.arange(len(t)), rtol=0, atol=1e-9 * dt):
        raise ValueError("evenly spaced lags from 0 are required")
    return dt


def transform(c, dt, window="hann", pad=4, timestep=None):
    """(nu in 1/fs, [..][n // 2 + 1]): dt Re rfft of the even extension of w(m) c[..][m], m = 0 .. M - 1, zero-padded to pad
    2 M points -- ``VelocityAutocorrelation.vdos``'s transform along the last axis.  ``window``: "hann" (the half window
    0.5 (1 + cos(pi m / M))) or None; ``timestep`` (not None): divided by sinc^2(nu timestep), the transfer function of a
    finite difference over one frame."""
    if window not in ("hann", None):
        raise ValueError("window: 'hann' or None")
    if int(pad) != pad or pad < 1:
        raise ValueError("pad must be an integer >= 1")
    c = np.asarray(c, dtype=np.float64)
    M = c.shape[-1]
    n = int(pad) * 2 * M
    w = 0.5 * (1.0 + np.cos(np.pi * np.arange(M) / M)) if window == "hann" else np.ones(M)
    nu = np.arange(n // 2 + 1) / (n * dt)
    g = np.zeros(c.shape[:-1] + (n,))
    g[..., :M] = w * c
    g[..., n - M + 1:] = g[..., 1:M][..., ::-1]
    gain = np.sinc(nu * timestep) ** 2 if timestep is not None else 1.0
    return nu, dt * np.fft.rfft(g, axis=-1).real / gain


def fit_through_origin(q, omega):
    """slope of the least-squares line omega = c q through the origin (NaN without a point)"""
    q, omega = np.asarray(q, dtype=np.float64), np.asarray(omega, dtype=np.float64)
    ok = np.isfinite(q) & np.isfinite(omega) & (q > 0)
    return float((q[ok] * omega[ok]).sum() / (q[ok] * q[ok]).sum()) if ok.any() else float("nan")


class CurrentCorrelation(Deferred):
    """
    Longitudinal and transverse current correlation functions C_L(q, t), C_T(q, t) (window form)

    ``from_trajectory`` / ``from_velocities`` enqueue the analysis on the device's first lane and return; ``.data`` (and every
    other result) waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    Lags, origins and vectors are ``IntermediateScattering``'s; by default EVERY lag 0 .. F//2 - 1 is taken, as
    ``VelocityAutocorrelation`` does -- a spectrum needs them all.  The velocities are the finite differences of the positions
    (a sample lives on the half step, its phase at the midpoint) divided by the timestep, or a velocity trajectory.
      .data        Time, q, X-X-L, X-X-T (number current per atom), then A-B-L, A-B-T of every ordered pair (A at the
                   origin, B at the origin + lag; Ashcroft-Langreth); the T columns carry the 1/2 of the two transverse
                   directions; Angstrom^2 / fs^2; W x nbins rows stacked by lag; NaN in bins without a vector
      .counts [W][nbins], .long_sums and .trans_sums [S][S][W][nbins] (Angstrom^2 per frame^2, no 1/2), .beyond [W] in
      library species order ``.kinds``; .hkl the vectors; .n_origins [W]
    ``weighted``, ``normalised``, ``spectrum``, ``dispersion``, ``sound_velocity``: what is usually made of them.
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, delta_time=None, max_time="half", timestep=1, dq=0.02, qmax=2.0, max_points=None,
                        seed=0, origin_stride=1, remove_com=True, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory (periodic on all three axes)
            delta_time, max_time, timestep: the windows of ``WindowMsd.from_trajectory`` (fs); delta_time None = timestep,
                i.e. every lag
            dq, qmax: bin width and range in 1/Angstrom; nbins = int(qmax // dq)
            max_points: at most this many vectors per bin (a seeded subsample; None: every vector)
            origin_stride: every origin_stride-th origin (an integer >= 1)
            remove_com: subtract the mass-weighted mean velocity of every frame
            device: GPU index (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group (each holding the whole trajectory)
                take contiguous shares of the (lag, origin) work list and all-reduce the integer sums once; False -> single
                process
        """
        return cls._construct(trajectory, None, delta_time, max_time, timestep, dq, qmax, max_points, seed, origin_stride,
                              remove_com, device, distributed)

    @classmethod
    def from_velocities(cls, positions, velocities, delta_time=None, max_time="half", timestep=1, dq=0.02, qmax=2.0,
                        max_points=None, seed=0, origin_stride=1, remove_com=True, device=None, distributed=None):
        """the same with the velocities of the simulation itself: ``velocities`` is a trajectory of the same frames and atoms
        whose "positions" are velocities in Angstrom / fs (e.g. CP2K's ``-vel-1.xyz``), or an array ``[F][N][3]``; the phase
        is taken at the frame's own positions, nothing is differenced or divided by the timestep"""
        return cls._construct(positions, velocities, delta_time, max_time, timestep, dq, qmax, max_points, seed, origin_stride,
                              remove_com, device, distributed)

    @classmethod
    def _construct(cls, trajectory, velocities, delta_time, max_time, timestep, dq, qmax, max_points, seed, origin_stride,
                   remove_com, device, distributed):
        cc = cls()
        origin_stride = lags.check_origin_stride(origin_stride)
        window, time = lags.window_setup(len(trajectory), timestep if delta_time is None else delta_time, max_time, timestep)
        cc.compute_current(trajectory, window, time, timestep, dq, qmax, max_points, seed, origin_stride, remove_com, velocities,
                           device=device, distributed=distributed)
        return cc

    def compute_current(self, trajectory, window, time, timestep=1, dq=0.02, qmax=2.0, max_points=None, seed=0, origin_stride=1,
                        remove_com=True, velocities=None, device=None, distributed=None):
        def pack_velocities(packed):
            if velocities is None:
                return None
            if isinstance(velocities, np.ndarray) or _hip._is_torch_tensor(velocities):
                v = PackedTrajectory(velocities, packed.cell, packed.numbers)
            else:
                v = lags.pack(velocities, device)
            if v.n_frames != packed.n_frames or v.n_atoms != packed.n_atoms:
                raise ValueError("velocities: other frames or atoms than the positions")
            return v

        s = lag_q.setup("C(q, t)", logger, trajectory, window, dq, qmax, max_points, seed, origin_stride, device, distributed,
                        after_pack=pack_velocities)
        vel = s.own
        ctx, merge = s.st.ctx, s.st.merge
        lay = _hip.current_layout(s.S, s.W, s.nbins)

        def local():
            return lag_q.local("C(q, t)", s, lay, lambda flat: ctx.current_accumulate(
                s.packed, s.hkl, s.window, s.dq, s.nbins, origin_stride=s.origin_stride, work_range=s.work, velocities=vel,
                remove_com=remove_com, out=flat))

        def finish(raw):
            if merge:
                flat, scale, vmax, kinds = raw
                m = lag_q.Merged(s, lay, flat, scale)
                counts, beyond, lng, trn = m.counts, m.beyond, m.block("long"), m.block("trans")
            else:
                counts, lng, trn, beyond, scale, vmax, kinds = raw
            self._assemble(counts, lng, trn, beyond, kinds, s.hkl, s.packed, s.elements, s.n_orig, s.window, time, s.dq, timestep,
                           vel is not None, vmax)

        self._defer(ctx, local, finish, collective=merge)

    def _assemble(self, counts, lng, trn, beyond, kinds, hkl, packed, elements, n_orig, window, time, dq, timestep, velocities,
                  vmax):
        self.kinds = list(kinds)
        self.counts, self.long_sums, self.trans_sums, self.beyond, self.hkl = counts, lng, trn, beyond, hkl
        self.n_origins = n_orig
        self.window, self.time, self.dq, self.timestep = np.asarray(window), np.asarray(time), dq, timestep
        self.finite_difference = not velocities
        self.vmax = vmax
        self.n_atoms = packed.n_atoms
        self.species_counts = {int(z): int(n) for z, n in packed.species_counts().items()}
        self.elements = [int(z) for z in elements]
        masses, numbers = np.asarray(packed.masses, dtype=np.float64), np.asarray(packed.numbers)
        self.mean_mass = {int(z): float(masses[numbers == z].mean()) for z in self.kinds}
        cells = np.asarray(packed.cell, dtype=np.float64).reshape(-1, 3, 3)
        # amu / Angstrom^3 over the trajectory's mean volume
        self.density = float(masses.sum() / np.abs(np.linalg.det(cells)).mean()) if len(cells) else float("nan")
        # the mean |k| of the vectors of every bin in the first origin frame's cell: where a bin's spectrum sits on the q axis
        self.q_mean = self._bin_means(hkl, cells[min(1, len(cells) - 1)] if len(cells) else None, dq, np.asarray(counts).shape[1])
        self.data = assemble(counts, lng, trn, kinds, elements, self.species_counts, time, dq, 1 if velocities else timestep)

    @staticmethod
    def _bin_means(hkl, cell, dq, nbins):
        out = np.full(nbins, np.nan)
        if cell is None or not len(hkl):
            return out
        q = np.linalg.norm(np.asarray(hkl, dtype=np.float64) @ _hip.reciprocal(cell), axis=1)
        b = np.floor(q / dq).astype(np.int64)
        ok = b < nbins
        n = np.bincount(b[ok], minlength=nbins).astype(np.float64)
        s = np.bincount(b[ok], weights=q[ok], minlength=nbins)
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(n > 0, s / n, np.nan)

    # ---- what is made of C(q, t) ----
    def _weights(self, weights):
        if isinstance(weights, str):
            if weights == "number":
                return np.ones(len(self.kinds))
            if weights == "mass":
                return np.array([self.mean_mass[int(z)] for z in self.kinds])
            raise ValueError("weights: 'mass', 'number' or a dictionary")
        w = []
        for z in self.kinds:
            sym = _data.chemical_symbols[int(z)]
            w.append(float(weights[sym] if sym in weights else weights[int(z)]))
        return np.array(w)

    def weighted(self, weights="mass"):
        """``DataFrame`` Time, q, L, T: C_w = sum over ordered pairs (a, c) of w_a w_c sums_ac / (counts sum_a N_a w_a^2), T
        halved, in Angstrom^2 / fs^2.  ``weights``: ``'mass'`` -- every element's mean mass: the momentum current --,
        ``'number'`` -- equal weights: ``X-X-L`` and ``X-X-T`` --, or {element symbol or atomic number: float} for every
        element of the system.  Host only."""
        self.data                                           # (waits for a pending computation)
        n = [self.species_counts[int(z)] for z in self.kinds]
        return combine(self.counts, self.long_sums, self.trans_sums, self._weights(weights), n, self.time, self.dq,
                       self.timestep if self.finite_difference else 1)

    def normalised(self):
        """``.data`` divided by its own t = 0 rows (host only; needs lag 0 among the windows)"""
        return normalise(self.data, self.window)

    def spectrum(self, window="hann", pad=4, fd_correction=None, weights="mass"):
        """C_L(q, omega) and C_T(q, omega): ``DataFrame`` q (the left bin edge), Frequency_THz, L, T, nbins blocks of
        pad M + 1 frequencies stacked by q bin -- ``VelocityAutocorrelation.vdos``'s transform (even extension, half Hann
        window, zero padding) of ``weighted(weights)`` along the lags of every bin.  ``fd_correction`` (default: on where the
        velocities are finite differences of positions): divided by sinc^2(nu timestep).  Bins without a vector are NaN.
        Raises ValueError unless the lags are evenly spaced from 0."""
        w = self.weighted(weights)
        W = len(self.window)
        nbins = len(w) // W if W else 0
        dt = lag_spacing(self.time)
        if fd_correction is None:
            fd_correction = self.finite_difference
        ts = float(self.timestep) if fd_correction else None
        nu, L = transform(w["L"].to_numpy().reshape(W, nbins).T, dt, window, pad, ts)
        _, T = transform(w["T"].to_numpy().reshape(W, nbins).T, dt, window, pad, ts)
        return pd.DataFrame({"q": np.repeat(np.arange(nbins, dtype=np.float64) * self.dq, len(nu)),
                             "Frequency_THz": np.tile(nu * THZ_PER_INVERSE_FS, nbins), "L": L.reshape(-1), "T": T.reshape(-1)})

    def dispersion(self, **kw):
        """``DataFrame`` q (the mean |k| of the bin's vectors), L_THz, T_THz, omega_L, omega_T (rad / fs): the frequency of the
        maximum of each spectrum per q bin with a vector; ``kw``: ``spectrum``'s arguments"""
        sp = self.spectrum(**kw)
        nbins = len(self.q_mean)
        nf = len(sp) // nbins if nbins else 0
        nu = sp["Frequency_THz"].to_numpy()[:nf]
        rows = []
        for b in range(nbins):
            L, T = (sp[c].to_numpy()[b * nf:(b + 1) * nf] for c in ("L", "T"))
            if not (np.isfinite(L).all() and np.isfinite(T).all()):
                continue
            fl, ft = float(nu[int(np.argmax(L))]), float(nu[int(np.argmax(T))])
            rows.append((float(self.q_mean[b]), fl, ft, 2.0 * np.pi * fl / THZ_PER_INVERSE_FS, 2.0 * np.pi * ft / THZ_PER_INVERSE_FS))
        return pd.DataFrame(rows, columns=["q", "L_THz", "T_THz", "omega_L", "omega_T"])

    def sound_velocity(self, q_fit, **kw):
        """``dict``: c_L and c_T (m / s) from a least-squares line omega = c q through the origin over the dispersion's bins
        below ``q_fit`` (1 / Angstrom), and with the trajectory's mean density rho (kg / m^3) the longitudinal modulus
        M = rho c_L^2, the shear modulus G = rho c_T^2 and the bulk modulus K = M - 4 G / 3 in GPa; ``kw``: ``spectrum``'s
        arguments"""
        d = self.dispersion(**kw)
        d = d[d["q"] < float(q_fit)]
        if not len(d):
            raise ValueError("no q bin with a vector below q_fit")
        c_l = fit_through_origin(d["q"], d["omega_L"]) * M_PER_S_PER_ANGSTROM_PER_FS
        c_t = fit_through_origin(d["q"], d["omega_T"]) * M_PER_S_PER_ANGSTROM_PER_FS
        rho = self.density * KG_PER_M3_PER_AMU_PER_A3
        M, G = rho * c_l ** 2 * 1e-9, rho * c_t ** 2 * 1e-9
        return {"c_L": c_l, "c_T": c_t, "density": rho, "M": M, "G": G, "K": M - 4.0 * G / 3.0, "n_bins": int(len(d))}

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.cqt`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'cqt'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote (``.data`` only)"""
        cc = cls()
        cc.data = pd.read_feather(_path.append_suffix(path_to_file, 'cqt'))
        return cc
