"""Self Van Hove function and non-Gaussian parameter on MI355X.

``WindowVanHove`` is the dynamical companion of ``WindowMsd`` (amof_amd/msd.py): the same windows (``delta_time``,
``max_time``, ``timestep``), the same displacements -- wrapped frame-to-frame steps, centre of mass removed, optional unwrap,
time origins k = 1 .. F-m-1 (amof/msd.py:185-237) -- but every single-atom displacement is binned instead of summed.
The histograms and the moments sum r^2, sum r^4 come from the HIP kernels behind ``amof_vanhove_window``; the host keeps
the normalisation and the DataFrames.  The reference has no such analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import _setup
from . import data as _data
from . import dist as _dist
from .files import path as _path
from .lags import window_setup      # (defined there for the whole family; callers also find it here)

logger = logging.getLogger(__name__)


def assemble(counts, overflow, moments, kinds, elements, species_counts, n_frames, window, time, dr):
    """``(data, alpha2)`` DataFrames from the raw outputs of ``amof_vanhove_window`` (whole system: every atom's samples).

    counts [S][W][nbins], overflow [S][W], moments [S][W][2] (sum r^2, sum r^4) in library species order ``kinds``;
    ``elements``: atomic numbers in column order; ``species_counts``: {atomic number: atoms}.
      data:   Time, r (left bin edge b dr), one column per element P_s(r, t) = counts / (n_s dr) with n_s = N_s (F - m - 1)
              samples, and X (every atom pooled), W x nbins rows
      alpha2: Time, one column per element and X: 3 n sum4 / (5 sum2^2) - 1 (NaN where sum2 == 0: m = 0)
    """
    counts = np.asarray(counts)
    W = len(window)
    nbins = counts.shape[2] if counts.ndim == 3 else 0
    origins = (n_frames - np.asarray(window, dtype=np.int64) - 1).astype(np.float64)      # F - m - 1
    idx = {int(z): k for k, z in enumerate(kinds)}
    r = np.tile(np.arange(nbins, dtype=np.float64) * dr, W)
    cols = {"Time": np.repeat(np.asarray(time), nbins), "r": r}
    ngp = {"Time": np.asarray(time)}

    def density(c, n):
        with np.errstate(divide="ignore", invalid="ignore"):
            return (c.astype(np.float64) / (n * dr)[:, None]).reshape(-1)

    def alpha2(n, s2, s4):
        with np.errstate(divide="ignore", invalid="ignore"):
            a = 3.0 * n * s4 / (5.0 * s2 * s2) - 1.0
        return np.where(s2 == 0, np.nan, a)

    n_all = 0.0
    for e in elements:
        s = idx[int(e)]
        n = species_counts[int(e)] * origins
        n_all = n_all + n
        name = _data.chemical_symbols[int(e)]
        cols[name] = density(counts[s], n)
        ngp[name] = alpha2(n, moments[s, :, 0], moments[s, :, 1])
    n_all = np.asarray(n_all, dtype=np.float64) * np.ones(W)
    cols["X"] = density(counts.sum(axis=0) if counts.shape[0] else np.zeros((W, nbins)), n_all)
    tot = moments.sum(axis=0) if moments.shape[0] else np.zeros((W, 2))
    ngp["X"] = alpha2(n_all, tot[:, 0], tot[:, 1])
    return pd.DataFrame(cols), pd.DataFrame(ngp)


class WindowVanHove(Deferred):
    """
    Self Van Hove function and non-Gaussian parameter (window form)

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    For every window m of ``WindowMsd`` and every time origin k = 1 .. F-m-1 it bins the displacement
    r = |u_i(k+m) - u_i(k)| of every atom i (the positions ``WindowMsd`` uses: centre of mass removed, optional unwrap).
      .data    Time, r, <element>..., X: P_s(r, t) = counts / (n_s dr), the radial probability density of the
               displacement (n_s = N_s (F - m - 1) samples; P_s = 4 pi r^2 G_s(r, t), G_s the self Van Hove function;
               sum_b P dr = 1 minus the fraction beyond rmax).  r is the left bin edge b dr.  X pools every atom.
      .alpha2  Time, <element>..., X: alpha_2(t) = 3 <r^4> / (5 <r^2>^2) - 1, NaN at t = 0
      .counts [S][W][nbins], .overflow [S][W], .sum2 / .sum4 [S][W] (species in ``.kinds`` order): raw outputs
    Time is expressed in fs.
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, delta_time=100, max_time="half", timestep=1, dr=0.01, rmax="half_cell",
                        unwrap=False, parallel=False, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory
            delta_time, max_time, timestep: the windows of ``WindowMsd.from_trajectory`` (fs)
            dr: bin width in Angstrom
            rmax: 'half_cell' (half the shortest cell length, as ``Rdf``) or a float; a float is NOT clamped to the
                cell (displacements are not bounded by it).  nbins = int(rmax // dr); larger displacements are counted in
                ``.overflow`` and still enter ``.alpha2``
            unwrap: Boolean, unwrap the trajectory first (as ``WindowMsd``)
            parallel: accepted for compatibility
        """
        vh = cls()
        window, time = window_setup(len(trajectory), delta_time, max_time, timestep)
        vh.compute_vanhove(trajectory, window, time, dr, rmax, unwrap, device=device, distributed=distributed)
        return vh

    def compute_vanhove(self, trajectory, window, time, dr=0.01, rmax="half_cell", unwrap=False, device=None, distributed=None):
        packed = _setup.pack(trajectory, device)      # (read whole: a window couples frames half a trajectory apart)
        if isinstance(rmax, str):
            if rmax != "half_cell":
                raise ValueError("rmax: 'half_cell' or a number")
            rmax = float(np.min(packed.cell_lengths()) / 2) if len(packed) else 0.0
        dr = float(dr)
        if not dr > 0:
            raise ValueError("dr must be positive")
        nbins = int(float(rmax) // dr)
        window = np.asarray(window, dtype=np.int32)
        elements = packed.unique_numbers()
        logger.info("Start computing the self Van Hove function at %s times, %s bins, on a trajectory of %s frames",
                    len(window), nbins, len(packed))

        st = _setup.setup(packed, device, distributed, lane=1, honour_local=True)
        rank, world, ctx, source, sharded = st.rank, st.world, st.ctx, st.source, st.sharded
        F = len(packed)
        atom_range = st.shard(packed.n_atoms)
        on_device = sharded and _dist.device_collectives()
        com = None
        if on_device and not unwrap and packed.on_device:
            # atoms are sharded; the centre of mass of every frame needs all of them: each rank computes its FRAME share
            # into a zeroed table (x + 0 = x, exact) and one all-reduce completes it -- here, in the calling thread.  The
            # kernel call itself goes through the lane, behind whatever this context has queued (a begin / finish pair of
            # another analysis is never split).
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
                # counts and overflow in ONE int64 tensor, the moments in another: two all-reduces, results stay in HBM
                import torch
                d = torch.device("cuda", ctx.device)
                flat = torch.zeros(S * W * (nbins + 1), dtype=torch.int64, device=d)
                out = (flat[:S * W * nbins].view(S, W, nbins), flat[S * W * nbins:].view(S, W),
                       torch.zeros((S, W, 2), dtype=torch.float64, device=d))
                _, _, moments, kinds = ctx.vanhove_window(packed, window, dr, nbins, unwrap=bool(unwrap), remove_com=True,
                                                          atom_range=atom_range, com=com, out=out)
                return flat, moments, kinds
            return ctx.vanhove_window(packed, window, dr, nbins, unwrap=bool(unwrap), remove_com=True, atom_range=atom_range)

        def finish(raw):
            if on_device:
                flat, moments, kinds = raw
                _dist.all_reduce_sum(flat)
                _dist.all_reduce_sum(moments)
                flat = flat.cpu().numpy().view(np.uint64)
                counts, overflow = flat[:S * W * nbins].reshape(S, W, nbins), flat[S * W * nbins:].reshape(S, W)
                moments = moments.cpu().numpy()
            else:
                counts, overflow, moments, kinds = raw
                if sharded:
                    flat = _dist.all_reduce_sum(np.concatenate([counts.reshape(-1), overflow.reshape(-1)]), device=ctx.device)
                    counts, overflow = flat[:S * W * nbins].reshape(S, W, nbins), flat[S * W * nbins:].reshape(S, W)
                    moments = _dist.all_reduce_sum(moments, device=ctx.device)
            self._assemble(counts, overflow, moments, kinds, packed, window, time, dr, elements)

        self._defer(ctx, local, finish, collective=sharded)

    def _assemble(self, counts, overflow, moments, kinds, packed, window, time, dr, elements):
        F = len(packed)
        self.kinds = list(kinds)
        self.counts, self.overflow = counts, overflow
        self.sum2, self.sum4 = moments[:, :, 0], moments[:, :, 1]
        self.dr = dr
        total = float(packed.n_atoms) * float(np.sum(np.maximum(F - np.asarray(window, dtype=np.int64) - 1, 0)))
        if total > 0:
            logger.info("Van Hove: %.3g %% of the displacements lie beyond rmax", 100.0 * float(overflow.sum()) / total)
        self.data, self.alpha2 = assemble(counts, overflow, moments, kinds, elements, packed.species_counts(), F, window, time,
                                          dr)

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.vanhove`` and ``.alpha2`` to ``<path>.ngp`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'vanhove'))
        self.alpha2.to_feather(_path.append_suffix(path_to_output, 'ngp'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the files ``write_to_file`` wrote"""
        vh = cls()
        vh.data = pd.read_feather(_path.append_suffix(path_to_file, 'vanhove'))
        vh.alpha2 = pd.read_feather(_path.append_suffix(path_to_file, 'ngp'))
        return vh
