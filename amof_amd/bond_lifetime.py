"""Bond survival correlations C(t) and S(t) on MI355X.

``BondLifetime`` is the dynamic twin of ``CoordinationNumber`` (amof_amd/cn.py): for the same neighbour sets and cutoffs and
for the lags of ``WindowMsd`` / ``DistinctVanHove`` it follows individual pairs through the trajectory.  ``DistinctVanHove``
shows the first-shell peak decay on average; this says whether the SAME Zn-N pair is still bonded a time t later.  The
integer counters come from the HIP kernels behind ``amof_bond_survival`` (amof_amd/csrc/bond.hip); the host keeps the
origin bookkeeping, two divisions and the DataFrame.  The reference has no dynamic neighbour analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import dist as _dist
from . import lags
from .files import path as _path

logger = logging.getLogger(__name__)


min_periodic_height = lags.min_periodic_height      # (its home is the family's shared module)


def assemble(counts, names, time):
    """``.data`` from the raw ``counts [n_sets][W][3]``: columns Time, then ``A-B`` = C(t) = counts[1] / counts[0] and
    ``A-B-continuous`` = S(t) = counts[2] / counts[0] per set of ``names`` = [(name, present)]; NaN where a lag has no bond at
    its origins, and throughout for a set with an absent species (it has no row in ``counts``)"""
    data = {"Time": np.asarray(time, dtype=np.float64)}
    k = 0
    for name, live in names:
        if live:
            c = np.asarray(counts[k], dtype=np.uint64).astype(np.float64)
            k += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                inter = np.where(c[:, 0] > 0, c[:, 1] / c[:, 0], np.nan)
                cont = np.where(c[:, 0] > 0, c[:, 2] / c[:, 0], np.nan)
        else:
            inter = cont = np.full(len(data["Time"]), np.nan)
        data[name] = inter
        data[name + "-continuous"] = cont
    return pd.DataFrame(data)


class BondLifetime(Deferred):
    """
    Bond survival correlations (window form)

    ``from_trajectory`` enqueues the analysis on its device's first lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    A set ``'A-B'`` with cutoff rc is an entry of ``CoordinationNumber``'s dictionary, ordered: centre species A, neighbour
    species B.  h_ij(f) = 1 iff j is a neighbour of i in frame f -- ``CoordinationNumber``'s decision (strict d < rc, minimum
    image in frame f's cell).  Lags m are the windows of ``WindowMsd`` (m = 0 included); origins are k = 1, 1 + s, ... <=
    F - m - 1 (s = ``origin_stride``), ``DistinctVanHove``'s.  Summed over the origins of a lag and all ordered pairs:
      counts[s][w][0] = sum h(k)                        bonds present at the origins
      counts[s][w][1] = sum h(k) h(k + m)               intermittent: bonded at both ends, whatever happened between
      counts[s][w][2] = sum prod_{f = k..k+m} h(f)      continuous: bonded at every frame of the trajectory from k to k + m
      .data        Time, ``A-B`` = C(t) = counts[1] / counts[0], ``A-B-continuous`` = S(t) = counts[2] / counts[0]; both are
                   1 at t = 0 and S <= C; NaN where a lag has no bond at its origins
      .counts      u64 [n_sets][W][3] (the sets whose species are present, in dictionary order: ``.sets``)
      .n_origins   [W]
    counts[s][0][0] is ``CoordinationNumber``'s integer sum over the frames 1, 1 + s, ..., F - 1.  A cutoff above half the
    smallest perpendicular cell height on a periodic axis is refused (a pair could be bonded through two images).
    Time is expressed in fs.
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, delta_time=100, max_time="half", timestep=1, origin_stride=1,
                        device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory
            nb_set_and_cutoff: dict, keys are str indicating pair of neighbours ('Zn-N': centre Zn, neighbour N), values
                are cutoffs float, in Angstrom (``CoordinationNumber.from_trajectory``'s dictionary)
            delta_time, max_time, timestep: the windows of ``WindowMsd.from_trajectory`` (fs)
            origin_stride: every origin_stride-th origin (an integer >= 1)
            device: GPU index (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group (each holding the whole trajectory)
                take contiguous shares of the centre atoms and all-reduce the counters once; False -> single process
        """
        bl = cls()
        window, time = lags.window_setup(len(trajectory), delta_time, max_time, timestep)
        bl.compute_survival(trajectory, nb_set_and_cutoff, window, time, origin_stride, device=device, distributed=distributed)
        return bl

    def compute_survival(self, trajectory, nb_set_and_cutoff, window, time, origin_stride=1, device=None, distributed=None):
        origin_stride = lags.check_origin_stride(origin_stride)
        packed = lags.pack(trajectory, device)
        window = np.asarray(window, dtype=np.int32)
        rcm, names, live = lags.neighbour_sets(packed, nb_set_and_cutoff)
        n_orig = lags.n_origins(len(packed), window, origin_stride)
        logger.info("Start computing bond survival at %s times for %s sets", len(window), len(live))

        st = lags.setup(packed, device, distributed)
        ctx, merge = st.ctx, st.merge
        atoms = _dist.shard_range(packed.n_atoms, st.rank, st.world) if merge else (0, packed.n_atoms)
        W = len(window)

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            lags.begin_local(st.source)
            if not live:
                return np.zeros((0, W, 3), dtype=np.uint64)
            out = None
            if st.on_device:
                # the counters stay in HBM from the kernels through the RCCL all-reduce (amof_bond_survival_dev)
                import torch
                out = torch.zeros((len(live), W, 3), dtype=torch.int64, device=torch.device("cuda", ctx.device))
            return ctx.bond_survival(packed, rcm, live, window, origin_stride=origin_stride, atom_range=atoms, out=out)

        def finish(counts):
            # the ranks' merge (the calling thread: collectives in program order): ONE all-reduce of the integer counters
            if live:
                counts = _dist.all_reduce_counts(counts, st.on_device, merge, ctx.device)
            self._assemble(counts, names, live, n_orig, time)

        self._defer(ctx, local, finish, collective=merge and bool(live))

    def _assemble(self, counts, names, live, n_orig, time):
        self.counts = counts
        self.sets = [name for name, ok in names if ok]
        self.n_origins = n_orig
        self.data = assemble(counts, names, time)

    def lifetime(self):
        """``{set: tau}``: the trapezoid integral of S(t) over ``Time`` (fs), per set.  A LOWER bound on the mean continuous
        bond lifetime when S has not decayed to zero by the last lag (the tail beyond it is not seen); NaN lags (no bond at
        the origins) end the integral."""
        d = self.data
        t = d["Time"].to_numpy(dtype=np.float64)
        out = {}
        for col in d.columns:
            if not col.endswith("-continuous"):
                continue
            s = d[col].to_numpy(dtype=np.float64)
            ok = np.isfinite(s)
            n = len(s) if ok.all() else int(np.argmin(ok))
            out[col[:-len("-continuous")]] = float(np.sum(0.5 * (s[1:n] + s[:n - 1]) * np.diff(t[:n]))) if n > 0 else float("nan")
        return out

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.bond`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'bond'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote"""
        bl = cls()
        bl.data = pd.read_feather(_path.append_suffix(path_to_file, 'bond'))
        return bl
