"""Velocity autocorrelation function and vibrational density of states on MI355X.

``VelocityAutocorrelation`` is the vibrational member of the dynamics family: C(t) = <v(0) . v(t)> per species over the
family's lags and origins (amof_amd/lags.py; DESIGN.md, "The lag/origin family: shared pieces"), by default at EVERY lag
0 .. F//2 - 1 -- a spectrum needs them all.  The velocities are either the finite differences of the positions -- the wrapped
frame-to-frame steps of ``WindowMsd``, centre of mass removed, divided by the timestep -- or a velocity trajectory of the
simulation itself (``from_velocities``).  The sums of products come from the HIP kernels behind ``amof_vacf_window``; the
host keeps the normalisation, the Fourier transform and the DataFrames.  The reference has no such analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import _setup
from . import data as _data
from . import dist as _dist
from . import lags as _lags
from .files import path as _path

logger = logging.getLogger(__name__)

THZ_PER_INVERSE_FS = 1.0e3
WAVENUMBER_PER_THZ = 1.0e12 / 2.99792458e10        # cm^-1 per THz


def assemble(sums, n_origins, kinds, elements, species_counts, time, timestep):
    """``.data`` from the raw sums of ``amof_vacf_window`` (whole system: every atom's samples).

    sums [S][W] in library species order ``kinds``; n_origins [W]; ``elements``: atomic numbers in column order;
    ``species_counts``: {atomic number: atoms}.  Columns: Time, one per element C_e(t) = sums / (N_e n(m)) / timestep^2, and
    X over all atoms (number-weighted: the pooled sums over N n(m)); NaN where a lag has no origin."""
    sums = np.asarray(sums, dtype=np.float64)
    n = np.asarray(n_origins, dtype=np.float64)
    W = len(n)
    idx = {int(z): k for k, z in enumerate(kinds)}
    scale = float(timestep) ** 2

    def mean(s, atoms):
        with np.errstate(divide="ignore", invalid="ignore"):
            c = s / (atoms * n) / scale
        return np.where(n == 0, np.nan, c)

    cols = {"Time": np.asarray(time)}
    total, atoms_all = np.zeros(W), 0
    for e in elements:
        s = sums[idx[int(e)]]
        cols[_data.chemical_symbols[int(e)]] = mean(s, species_counts[int(e)])
        total = total + s
        atoms_all += species_counts[int(e)]
    cols["X"] = mean(total, atoms_all) if atoms_all else np.full(W, np.nan)
    return pd.DataFrame(cols)


class VelocityAutocorrelation(Deferred):
    """
    Velocity autocorrelation function C(t) and vibrational density of states

    ``from_trajectory`` / ``from_velocities`` enqueue the analysis on the device's second lane and return; ``.data`` (and every
    other result) waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).
      .data       Time (fs), <element>..., X: C_e(t) = <v(0) . v(t)> in Angstrom^2 / fs^2 (velocity mode: the input's units
                  squared), averaged over the atoms of the element and the origins of the lag; X over all atoms
      .sums [S][W], .n_origins [W] (species in ``.kinds`` order): raw sums of x(k) x(k + m) and the origins of every lag
      normalised(), vdos(), diffusion(): what is usually made of C(t)
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, delta_time=None, max_time="half", timestep=1, origin_stride=1, device=None,
                        distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory (positions)
            delta_time, max_time, timestep: the lags of ``WindowMsd.from_trajectory`` (fs); delta_time None = timestep, i.e.
                every lag
            origin_stride: every origin_stride-th time origin of a lag is taken
        """
        return cls._construct(trajectory, delta_time, max_time, timestep, origin_stride, device, distributed, False)

    @classmethod
    def from_velocities(cls, trajectory, delta_time=None, max_time="half", timestep=1, origin_stride=1, device=None,
                        distributed=None):
        """the same for a trajectory whose "positions" are velocities (e.g. CP2K's ``-vel-1.xyz`` through
        ``read_cp2k_traj``): no finite difference, no wrap, the cell is ignored; the mass-weighted mean of every frame is
        removed"""
        return cls._construct(trajectory, delta_time, max_time, timestep, origin_stride, device, distributed, True)

    @classmethod
    def _construct(cls, trajectory, delta_time, max_time, timestep, origin_stride, device, distributed, velocities):
        vacf = cls()
        origin_stride = _lags.check_origin_stride(origin_stride)
        window, time = _lags.window_setup(len(trajectory), timestep if delta_time is None else delta_time, max_time, timestep)
        vacf.compute_vacf(trajectory, window, time, timestep, origin_stride, velocities, device=device, distributed=distributed)
        return vacf

    def compute_vacf(self, trajectory, window, time, timestep=1, origin_stride=1, velocities=False, device=None, distributed=None):
        packed = _setup.pack(trajectory, device)      # (read whole: a lag couples frames half a trajectory apart)
        window = np.asarray(window, dtype=np.int32)
        elements = packed.unique_numbers()
        logger.info("Start computing the velocity autocorrelation at %s lags on a trajectory of %s frames", len(window), len(packed))

        st = _setup.setup(packed, device, distributed, lane=1, honour_local=True)
        rank, world, ctx, source, sharded = st.rank, st.world, st.ctx, st.source, st.sharded
        F = len(packed)
        atom_range = st.shard(packed.n_atoms)
        on_device = sharded and _dist.device_collectives()
        com = None
        if on_device and packed.on_device:
            # atoms are sharded; the centre of mass (the mean velocity) of every frame needs all of them: each rank computes
            # its FRAME share into a zeroed table (x + 0 = x, exact) and one all-reduce completes it -- here, in the calling
            # thread, as WindowVanHove does
            import torch
            com = torch.zeros((F, 3), dtype=torch.float64, device=torch.device("cuda", ctx.device))
            frames = _dist.shard_range(F, rank, world)
            _setup.on_lane(ctx, lambda: ctx.msd_com(packed, frames, com))
            _dist.all_reduce_sum(com)

        S = len(_hip.packed_species(packed)[0])
        W = len(window)

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            _setup.begin_local(source)
            if on_device:
                # the S x W sums stay in HBM from the kernels through their all-reduce
                import torch
                out = torch.zeros((S, W), dtype=torch.float64, device=torch.device("cuda", ctx.device))
                return ctx.vacf_window(packed, window, origin_stride=origin_stride, velocities=velocities, remove_com=True,
                                       atom_range=atom_range, com=com, out=out)
            return ctx.vacf_window(packed, window, origin_stride=origin_stride, velocities=velocities, remove_com=True,
                                   atom_range=atom_range)

        def finish(raw):
            sums, kinds = raw
            if on_device:
                _dist.all_reduce_sum(sums)
                sums = sums.cpu().numpy()
            elif sharded:
                sums = _dist.all_reduce_sum(sums, device=ctx.device)
            self._assemble(sums, kinds, packed, window, time, timestep, origin_stride, velocities, elements)

        self._defer(ctx, local, finish, collective=sharded)

    def _assemble(self, sums, kinds, packed, window, time, timestep, origin_stride, velocities, elements):
        self.kinds = list(kinds)
        self.sums = np.asarray(sums)
        self.n_origins = _lags.n_origins(len(packed), window, origin_stride)
        self.timestep = timestep
        self.finite_difference = not velocities
        counts = packed.species_counts()
        masses, numbers = np.asarray(packed.masses, dtype=np.float64), np.asarray(packed.numbers)
        # vdos(): the weight of an element in X is its atoms times their mean mass
        self.weights = {_data.chemical_symbols[int(e)]: float(masses[numbers == e].sum()) for e in elements}
        # (velocity mode: the samples already are velocities -- nothing to divide by)
        self.data = assemble(self.sums, self.n_origins, kinds, elements, counts, time, 1 if velocities else timestep)

    # ---- what is made of C(t) ----
    def _columns(self):
        return [c for c in self.data.columns if c != "Time"]

    def normalised(self):
        """C(t) / C(0), column by column"""
        out = self.data.copy()
        for c in self._columns():
            out[c] = out[c].values / out[c].values[0] if len(out) else out[c]
        return out

    def _lag_spacing(self):
        t = np.asarray(self.data["Time"].values, dtype=np.float64)      # (waits for a pending computation)
        if len(t) == 0:
            raise ValueError("no lag")
        dt = float(t[1] - t[0]) if len(t) > 1 else float(self.__dict__.get("timestep", 1))
        if t[0] != 0 or not dt > 0 or not np.array_equal(t, dt * np.arange(len(t))):
            raise ValueError("evenly spaced lags from 0 are required")
        return dt

    def vdos(self, window="hann", pad=4, fd_correction=None):
        """Vibrational density of states: DataFrame with Frequency_THz, Wavenumber_cm-1, one column per element and X.

        D(nu) = dt Re rfft of the even extension of w(m) C(m dt), m = 0 .. M - 1, zero-padded to pad 2 M points (dt: the
        spacing of the lags); ``window``: "hann" -- the half window w(m) = 0.5 (1 + cos(pi m / M)) -- or None.
        ``fd_correction`` (default: on where the velocities are finite differences of positions): D is divided by
        sinc^2(pi nu timestep), the transfer function of the difference over one frame.  X weights the elements by their
        atoms times their mean mass (an object read from a file has no masses: there X is the transform of ``.data``'s X).
        Raises ValueError unless the lags are evenly spaced from 0."""
        dt = self._lag_spacing()
        M = len(self.data)
        if window not in ("hann", None):
            raise ValueError("window: 'hann' or None")
        if int(pad) != pad or pad < 1:
            raise ValueError("pad must be an integer >= 1")
        timestep, weights = float(self.__dict__.get("timestep", dt)), self.__dict__.get("weights")
        if fd_correction is None:
            fd_correction = self.__dict__.get("finite_difference", True)
        n = int(pad) * 2 * M
        w = 0.5 * (1.0 + np.cos(np.pi * np.arange(M) / M)) if window == "hann" else np.ones(M)
        nu = np.arange(n // 2 + 1) / (n * dt)                   # 1 / fs
        gain = np.sinc(nu * timestep) ** 2 if fd_correction else 1.0

        def transform(c):
            g = np.zeros(n)
            g[:M] = w * c
            g[n - M + 1:] = g[1:M][::-1]
            return dt * np.fft.rfft(g).real / gain

        cols = {"Frequency_THz": nu * THZ_PER_INVERSE_FS, "Wavenumber_cm-1": nu * THZ_PER_INVERSE_FS * WAVENUMBER_PER_THZ}
        names = [c for c in self._columns() if c != "X"]
        for c in names:
            cols[c] = transform(np.asarray(self.data[c].values, dtype=np.float64))
        if weights is not None and names:
            total = sum(weights[c] for c in names)
            cols["X"] = sum(weights[c] * cols[c] for c in names) / total
        else:
            cols["X"] = transform(np.asarray(self.data["X"].values, dtype=np.float64))
        return pd.DataFrame(cols)

    def diffusion(self):
        """Green-Kubo diffusion coefficients {column: (1/3) integral of C dt} by the trapezoid rule over the lags, in
        Angstrom^2 / fs"""
        t = np.asarray(self.data["Time"].values, dtype=np.float64)

        def integral(c):
            return float(np.sum(0.5 * (c[1:] + c[:-1]) * np.diff(t)))
        return {c: integral(np.asarray(self.data[c].values, dtype=np.float64)) / 3.0 for c in self._columns()}

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.vacf`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'vacf'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote.  The file holds ``.data`` alone: ``vdos`` then takes finite
        differences over one lag spacing for granted (``fd_correction=False`` for a velocity trajectory)"""
        vacf = cls()
        vacf.data = pd.read_feather(_path.append_suffix(path_to_file, 'vacf'))
        return vacf
