"""Distinct Van Hove function G_d(r, t) on MI355X.

``DistinctVanHove`` is the pair half of ``WindowVanHove`` (amof_amd/vanhove.py): for the same lags (the windows of
``WindowMsd``) it histograms the distance between atom i at an origin frame k and every other atom j at frame k + m.  At
t = 0 this is g(r); the first-shell peak decays as bonds break and re-form.  The integer histograms come from the HIP kernels
behind ``amof_vanhove_distinct`` (amof_amd/csrc/vanhove_distinct.hip); the host keeps the origin bookkeeping, the RDF's
normalisation (``rdf.normalize_rdf``) and the DataFrame.  The reference has no dynamic pair analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import data as _data
from . import dist as _dist
from . import lags
from .files import path as _path
# (the origin bookkeeping is defined in lags.py for the whole family; callers also find it here)
from .lags import n_origins, origins, window_setup, work_list      # noqa: F401
from .rdf import normalize_rdf

logger = logging.getLogger(__name__)


def clamp_rmax(cell_lengths, rmax):
    """``Rdf.compute_rdf``'s rule: 'half_cell' or a float, clamped to half the shortest cell length over the trajectory"""
    half = float(np.min(cell_lengths) / 2)
    if isinstance(rmax, str):
        if rmax != "half_cell":
            raise ValueError("rmax: 'half_cell' or a number")
        return half
    if rmax > half:
        logger.info("Specified rmax %s is larger than half cell; will use half_cell rmax", rmax)
        return half
    return float(rmax)


def mean_volumes(cells, n_frames, windows, origin_stride=1):
    """``[W]`` mean cell volume over the origin frames of every lag (NaN for a lag without origins)"""
    vol = np.abs(np.linalg.det(np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)))
    out = np.full(len(windows), np.nan)
    for i, m in enumerate(windows):
        k = origins(n_frames, m, origin_stride)
        if len(k):
            out[i] = float(vol[0]) if len(vol) == 1 else float(np.mean(vol[k]))
    return out


def assemble(hist, kinds, elements, species_counts, n_atoms, n_orig, mean_volume, time, rmax, nbins, dr):
    """``.data`` from the raw ``hist [S][S][W][nbins]`` (library species order ``kinds``): columns Time, r, X-X, the
    ordered A-B partials, then A-X (``Rdf``'s order), W x nbins rows stacked by lag; r = b dr as ``Rdf``.  Lag w is
    ``Rdf``'s normalisation with ncount = n_origins(w) N_a, natoms = N and the mean volume over its origin frames."""
    hist = np.asarray(hist)
    W, nbins = len(time), int(nbins)
    idx = {int(z): k for k, z in enumerate(kinds)}
    sidx = [idx[int(z)] for z in elements]
    syms = [_data.chemical_symbols[int(z)] for z in elements]
    n_el = len(elements)
    names = ["Time", "r", "X-X"] + [a + "-" + b for a in syms for b in syms] + [a + "-X" for a in syms]
    table = np.empty((W, len(names), nbins), dtype=np.float64)
    counts = np.array([species_counts[int(z)] for z in kinds], dtype=np.float64)
    for w in range(W):
        table[w, 0] = time[w]
        table[w, 1] = np.arange(nbins) * dr
        h = hist[:, :, w, :]
        with np.errstate(divide="ignore", invalid="ignore"):
            table[w, 2] = normalize_rdf(h.sum(axis=(0, 1)), n_orig[w] * n_atoms, n_atoms, mean_volume[w], rmax, nbins)
            partial = normalize_rdf(h, (n_orig[w] * counts)[:, None, None], n_atoms, mean_volume[w], rmax, nbins)
        sub = partial[sidx][:, sidx]
        table[w, 3:3 + n_el * n_el] = sub.reshape(n_el * n_el, nbins)
        acc = 0      # the reference's sum([...]) of the A-X columns, in species order (as Rdf)
        for j in range(n_el):
            acc = acc + sub[:, j]
        table[w, 3 + n_el * n_el:] = acc
    return pd.DataFrame(table.transpose(0, 2, 1).reshape(W * nbins, len(names)), columns=names)


class DistinctVanHove(Deferred):
    """
    Distinct Van Hove function (window form)

    ``from_trajectory`` enqueues the analysis on its device's first lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    Lags m are the windows of ``WindowMsd`` / ``WindowVanHove`` (m = 0 included); origins are k = 1, 1 + s, ... <= F - m - 1
    (s = ``origin_stride``; s = 1 gives ``WindowVanHove``'s origins).  Every ordered pair (i, j), i != j, is counted with i at
    frame k and j at frame k + m: the distance is the RDF's canonical minimum image of r_j(k + m) - r_i(k) in frame k's cell,
    binned by the RDF's rule.  Unlike ``WindowVanHove``, no centre of mass is removed and nothing is unwrapped: pair
    distances are periodic, so neither is needed (a centre-of-mass-consistent G = G_s + G_d is not provided).
      .data        Time, r, X-X, A-B (ordered: A at the origin, B at the origin + lag), A-X; W x nbins rows stacked by lag.
                   Each lag is normalised like ``Rdf`` (ncount = n_origins(m) N_a, the mean volume over its origin frames),
                   so the t = 0 rows are ``Rdf.data`` of frames 1 .. F-1 (s = 1); at long times the columns tend to 1.
      .hist        u64 [S][S][W][nbins] in library species order ``.kinds`` (centre species first)
      .n_origins   [W],  .mean_volume [W],  .rmax
    Time is expressed in fs.
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, delta_time=100, max_time="half", timestep=1, dr=0.01, rmax="half_cell", origin_stride=1,
                        device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory
            delta_time, max_time, timestep: the windows of ``WindowMsd.from_trajectory`` (fs)
            dr: bin width in Angstrom
            rmax: 'half_cell' or a float, clamped to half the shortest cell length (as ``Rdf``); nbins = int(rmax // dr)
            origin_stride: every origin_stride-th origin (an integer >= 1)
            device: GPU index (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group (each holding the whole trajectory)
                take contiguous shares of the (lag, origin) work list and all-reduce the counts once; False -> single
                process
        """
        vh = cls()
        window, time = window_setup(len(trajectory), delta_time, max_time, timestep)
        vh.compute_distinct(trajectory, window, time, dr, rmax, origin_stride, device=device, distributed=distributed)
        return vh

    def compute_distinct(self, trajectory, window, time, dr=0.01, rmax="half_cell", origin_stride=1, device=None, distributed=None):
        dr = float(dr)
        if not dr > 0:
            raise ValueError("dr must be positive")
        origin_stride = lags.check_origin_stride(origin_stride)
        packed = lags.pack(trajectory, device)
        rmax = clamp_rmax(packed.cell_lengths(), rmax)
        nbins = int(rmax // dr)             # Python float floor-division, as Rdf
        if nbins <= 0:
            raise ValueError("rmax // dr gives no bin")
        window = np.asarray(window, dtype=np.int32)
        elements = packed.unique_numbers()
        n_orig = n_origins(len(packed), window, origin_stride)
        total = int(n_orig.sum())
        logger.info("Start computing the distinct Van Hove function at %s times, %s bins, %s (lag, origin) pairs", len(window),
                    nbins, total)

        st = lags.setup(packed, device, distributed)
        ctx, merge = st.ctx, st.merge
        work = _dist.shard_range(total, st.rank, st.world) if merge else (0, total)
        S = len(_hip.packed_species(packed)[0])
        W = len(window)

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            lags.begin_local(st.source)
            out = None
            if st.on_device:
                # the counts stay in HBM from the kernels through the RCCL all-reduce (amof_vanhove_distinct_dev)
                import torch
                out = torch.zeros((S, S, W, nbins), dtype=torch.int64, device=torch.device("cuda", ctx.device))
            return ctx.vanhove_distinct(packed, window, rmax, nbins, origin_stride=origin_stride, work_range=work, out=out)

        def finish(raw):
            # the ranks' merge (the calling thread: collectives in program order): ONE all-reduce of the integer counts;
            # the volumes come from the host's cells, so no float reduction is needed
            hist, kinds = raw
            hist = _dist.all_reduce_counts(hist, st.on_device, merge, ctx.device)
            self._assemble(hist, kinds, packed, elements, n_orig, window, time, rmax, nbins, dr, origin_stride)

        self._defer(ctx, local, finish, collective=merge)

    def _assemble(self, hist, kinds, packed, elements, n_orig, window, time, rmax, nbins, dr, origin_stride):
        self.hist = hist
        self.kinds = list(kinds)
        self.n_origins = n_orig
        self.rmax = rmax
        self.mean_volume = mean_volumes(packed.cell, len(packed), window, origin_stride)
        self.data = assemble(hist, kinds, elements, packed.species_counts(), packed.n_atoms, n_orig, self.mean_volume, time,
                             rmax, nbins, dr)

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.vanhove_distinct`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'vanhove_distinct'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote"""
        vh = cls()
        vh.data = pd.read_feather(_path.append_suffix(path_to_file, 'vanhove_distinct'))
        return vh
