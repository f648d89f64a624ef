"""Intermediate scattering function F(q, t) on MI355X, coherent and self.

``IntermediateScattering`` is the reciprocal-space half of the dynamics family (``WindowVanHove``, ``DistinctVanHove``): for
the lags of ``WindowMsd`` it correlates rho_a(k, t0) with rho_c(k, t0 + t) on the reciprocal-lattice vectors
``StructureFactor`` sums over and bins the products by |k|.  At t = 0 the coherent part is S(q); its decay at the first sharp
diffraction peak is the structural relaxation time.  The self part is the phase sum of every atom's own displacement.  The
correlation runs in the HIP kernels behind ``amof_isf_accumulate`` (amof_amd/csrc/isf.hip; exact u32 phases, int64
fixed-point sums); the host keeps the choice of vectors, the origin bookkeeping, the normalisation and the DataFrame.  The
reference has no such analysis.
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

logger = logging.getLogger(__name__)


def column_names(elements, self_part=True):
    """``Time, q, X-X``, every ordered ``A-B`` (``StructureFactor``'s order), then ``A-self`` per element and ``X-self``"""
    syms = [_data.chemical_symbols[int(z)] for z in elements]
    names = ["Time", "q", "X-X"] + [a + "-" + b for a in syms for b in syms]
    if self_part:
        names += [a + "-self" for a in syms] + ["X-self"]
    return names


def assemble(counts, coh, self_sums, kinds, elements, species_counts, time, dq):
    """``.data`` from the raw outputs of ``amof_isf_accumulate`` (counts [W][nbins], coh [S][S][W][nbins], self_sums
    [S][W][nbins] or None, library species order ``kinds``); ``elements``: atomic numbers in column order;
    ``species_counts``: {atomic number: atoms}.
      Time, q     the lag's time, the left bin edge b dq; W x nbins rows stacked by lag
      X-X         sum_ac coh_ac / (counts N)
      A-B         coh_AB / (counts sqrt(N_A N_B)), A at the origin, B at the origin + lag (Ashcroft-Langreth)
      A-self      self_A / (counts N_A);  X-self = sum_a self_a / (counts N)
    Bins with no samples are NaN."""
    counts = np.asarray(counts, dtype=np.float64)
    coh = np.asarray(coh, dtype=np.float64)
    W, nbins = counts.shape
    N = float(sum(species_counts[int(z)] for z in kinds))
    denom = np.where(counts > 0, counts, np.nan)
    idx = {int(z): k for k, z in enumerate(kinds)}
    cols = {"Time": np.repeat(np.asarray(time, dtype=np.float64), nbins),
            "q": np.tile(np.arange(nbins, dtype=np.float64) * dq, W)}
    cols["X-X"] = (coh.sum(axis=(0, 1)) / (denom * N)).reshape(-1)
    syms = [_data.chemical_symbols[int(z)] for z in elements]
    for i, zi in enumerate(elements):
        for j, zj in enumerate(elements):
            norm = np.sqrt(float(species_counts[int(zi)]) * float(species_counts[int(zj)]))
            cols[syms[i] + "-" + syms[j]] = (coh[idx[int(zi)], idx[int(zj)]] / (denom * norm)).reshape(-1)
    if self_sums is not None:
        self_sums = np.asarray(self_sums, dtype=np.float64)
        for i, zi in enumerate(elements):
            cols[syms[i] + "-self"] = (self_sums[idx[int(zi)]] / (denom * float(species_counts[int(zi)]))).reshape(-1)
        cols["X-self"] = (self_sums.sum(axis=0) / (denom * N)).reshape(-1)
    return pd.DataFrame(cols)


normalise = lag_q.normalise


class IntermediateScattering(Deferred):
    """
    Intermediate scattering function F(q, t), coherent and self (window form)

    ``from_trajectory`` enqueues the analysis on its device's first lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    Lags m are the windows of ``WindowMsd`` (m = 0 included); origins are k = 1, 1 + s, ... <= F - m - 1 (s =
    ``origin_stride``), as ``DistinctVanHove``.  The vectors are ``StructureFactor(first_frame=1, frame_stride=s)``'s; the
    bin of a vector is decided on the origin frame's cell.
      .data        Time, q, X-X, A-B (ordered: A at the origin, B at the origin + lag; Ashcroft-Langreth), then A-self and
                   X-self; W x nbins rows stacked by lag; NaN in bins without a vector.  The t = 0 rows of the coherent
                   columns are ``StructureFactor.data`` over the origin frames; the self columns start at 1.
      .counts [W][nbins], .coh [S][S][W][nbins], .self_sums [S][W][nbins] (None without ``self_part``), .beyond [W] in
      library species order ``.kinds``; .hkl the vectors; .n_origins [W]
    ``weighted(weights)`` combines the partials with scattering lengths or form factors; ``normalised()`` divides by the
    t = 0 rows.  Time is expressed in fs.
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, delta_time=100, max_time="half", timestep=1, dq=0.02, qmax=5.0, max_points=None,
                        seed=0, origin_stride=1, self_part=True, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory (periodic on all three axes)
            delta_time, max_time, timestep: the windows of ``WindowMsd.from_trajectory`` (fs)
            dq, qmax: bin width and range in 1/Angstrom; nbins = int(qmax // dq)
            max_points: at most this many vectors per bin (a seeded subsample; None: every vector)
            origin_stride: every origin_stride-th origin (an integer >= 1)
            self_part: also the self intermediate scattering function (one phase sum per (lag, origin) where the coherent
                part costs one per frame: use a larger origin_stride for long trajectories)
            device: GPU index (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group (each holding the whole trajectory)
                take contiguous shares of the (lag, origin) work list and all-reduce the integer sums once; False -> single
                process
        """
        isf = cls()
        window, time = lags.window_setup(len(trajectory), delta_time, max_time, timestep)
        isf.compute_isf(trajectory, window, time, dq, qmax, max_points, seed, origin_stride, self_part, device=device,
                        distributed=distributed)
        return isf

    def compute_isf(self, trajectory, window, time, dq=0.02, qmax=5.0, max_points=None, seed=0, origin_stride=1, self_part=True,
                    device=None, distributed=None):
        s = lag_q.setup("F(q, t)", logger, trajectory, window, dq, qmax, max_points, seed, origin_stride, device, distributed)
        ctx, merge = s.st.ctx, s.st.merge
        lay = _hip.isf_layout(s.S, s.W, s.nbins, self_part)

        def local():
            return lag_q.local("F(q, t)", s, lay, lambda flat: ctx.isf_accumulate(
                s.packed, s.hkl, s.window, s.dq, s.nbins, origin_stride=s.origin_stride, work_range=s.work, self_part=self_part,
                out=flat))

        def finish(raw):
            if merge:
                # counts, beyond, coh and self in ONE int64 tensor: one all-reduce
                flat, scale, kinds = raw
                m = lag_q.Merged(s, lay, flat, scale)
                counts, beyond, coh = m.counts, m.beyond, m.block("coh")
                selfs = m.block("self", diagonal=True) if self_part else None
            else:
                counts, coh, selfs, beyond, kinds = raw
            self._assemble(counts, coh, selfs, beyond, kinds, s.hkl, s.packed, s.elements, s.n_orig, s.window, time, s.dq)

        self._defer(ctx, local, finish, collective=merge)

    def _assemble(self, counts, coh, selfs, beyond, kinds, hkl, packed, elements, n_orig, window, time, dq):
        self.kinds = list(kinds)
        self.counts, self.coh, self.self_sums, self.beyond, self.hkl = counts, coh, selfs, beyond, hkl
        self.n_origins = n_orig
        self.window, self.time, self.dq = np.asarray(window), np.asarray(time), dq
        self.n_atoms = packed.n_atoms
        self.species_counts = {int(z): int(n) for z, n in packed.species_counts().items()}
        self.elements = [int(z) for z in elements]
        self.data = assemble(counts, coh, selfs, kinds, elements, self.species_counts, time, dq)

    def weighted(self, weights):
        """``DataFrame`` Time, q, F: F_w(q, t) = sum over ordered pairs (a, c) of w_a w_c coh_ac / (counts sum_a N_a w_a^2),
        ``StructureFactor.weighted`` lag by lag.

        ``weights``: {element symbol or atomic number: float, or a callable of q in 1/Angstrom (evaluated at the bins'
        left edges)} -- neutron scattering lengths or X-ray form factors, for every element of the system.  Equal weights
        give ``X-X``.  Host only."""
        counts = np.asarray(self.counts, dtype=np.float64)
        W, nbins = counts.shape
        q = np.arange(nbins, dtype=np.float64) * self.dq
        w = []
        for z in self.kinds:
            sym = _data.chemical_symbols[int(z)]
            v = weights[sym] if sym in weights else weights[int(z)]
            w.append(np.asarray(v(q), dtype=np.float64) * np.ones_like(q) if callable(v) else np.full_like(q, float(v)))
        coh = np.asarray(self.coh, dtype=np.float64)
        num = np.zeros((W, nbins))
        norm = np.zeros(nbins)
        for a, z in enumerate(self.kinds):
            norm = norm + self.species_counts[int(z)] * w[a] * w[a]
            for c in range(len(self.kinds)):
                num = num + (w[a] * w[c])[None, :] * coh[a, c]
        with np.errstate(divide="ignore", invalid="ignore"):
            f = num / (np.where(counts > 0, counts, np.nan) * norm[None, :])
        return pd.DataFrame({"Time": np.repeat(np.asarray(self.time, dtype=np.float64), nbins), "q": np.tile(q, W),
                             "F": f.reshape(-1)})

    def normalised(self):
        """``.data`` divided by its own t = 0 rows, F(q, t) / F(q, 0) (host only; needs lag 0 among the windows)"""
        return normalise(self.data, self.window)

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.isf`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'isf'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote (``.data`` only)"""
        isf = cls()
        isf.data = pd.read_feather(_path.append_suffix(path_to_file, 'isf'))
        return isf
