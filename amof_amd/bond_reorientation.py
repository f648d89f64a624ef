"""Bond reorientation correlations C1(t) and C2(t) on MI355X.

``BondReorientation`` is the rotational twin of ``BondLifetime`` (amof_amd/bond_lifetime.py): for the same neighbour sets,
cutoffs, lags and origins it follows the VECTOR of every pair that is bonded at both ends of a lag and averages the first
and second Legendre polynomials of the cosine between the two: C_l(t) = <P_l(u(0) . u(t))>.  C2 is what NMR relaxation
measures.  The integer sums come from the HIP kernels behind ``amof_bond_reorientation`` (amof_amd/csrc/bond.hip); the host
keeps the origin bookkeeping, the divisions and the DataFrame.  The reference has no dynamic neighbour analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import dist as _dist
from . import lags
from .files import path as _path

logger = logging.getLogger(__name__)

SCALE_MAX = 40      # e_s never exceeds it: a quantum of 2^-41 per term is far below the float64 error of a term's cosine
SCALE_MIN = 20      # below it the call is refused


def scale_log2(n_a, n_b, n_0):
    """the library's fixed-point exponent e_s = min(40, 62 - bit_length(n_A n_B n_0)) of a set with n_A centres and n_B
    neighbours in a trajectory with n_0 origins of lag 0: no sum of |terms| <= 2^e_s can leave int64.  ValueError below 20
    (the library refuses the call)"""
    e = min(SCALE_MAX, 62 - (int(n_a) * int(n_b) * int(n_0)).bit_length())
    if e < SCALE_MIN:
        raise ValueError("%d x %d pairs x %d origins leave a fixed-point quantum above 2^-%d: use a larger origin_stride or "
                         "fewer frames" % (n_a, n_b, n_0, SCALE_MIN))
    return e


def assemble(counts, scale, names, time):
    """``.data`` from the raw ``counts [n_sets][W][3]`` (int64) and ``scale [n_sets]``: columns Time, then ``A-B-P1`` =
    C1(t) = counts[1] 2^-e / counts[0] and ``A-B-P2`` = C2(t) = counts[2] 2^-e / counts[0] per set of ``names`` = [(name,
    present)]; NaN where a lag has no pair bonded at both ends, and throughout for a set with an absent species (it has no
    row in ``counts``)"""
    data = {"Time": np.asarray(time, dtype=np.float64)}
    k = 0
    for name, live in names:
        if live:
            c = np.asarray(counts[k], dtype=np.int64).astype(np.float64)
            q = np.ldexp(1.0, -int(scale[k]))
            k += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                p1 = np.where(c[:, 0] > 0, c[:, 1] * q / c[:, 0], np.nan)
                p2 = np.where(c[:, 0] > 0, c[:, 2] * q / c[:, 0], np.nan)
        else:
            p1 = p2 = np.full(len(data["Time"]), np.nan)
        data[name + "-P1"] = p1
        data[name + "-P2"] = p2
    return pd.DataFrame(data)


class BondReorientation(Deferred):
    """
    Reorientational correlation functions of bond vectors (window form)

    ``from_trajectory`` enqueues the analysis on its device's first lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    Sets, cutoffs, the bond indicator h_ij(f), lags and origins are ``BondLifetime``'s.  d_ij(f) is the minimum-image
    vector from i to j in frame f's cell.  Summed over the origins k of a lag m and all ordered pairs bonded at both ends:
      counts[s][w][0] = sum h(k) h(k + m)                               (``BondLifetime``'s intermittent counter)
      counts[s][w][1] = sum h(k) h(k + m) rint(P1(cos) 2^e_s)           cos: between d(k) and d(k + m)
      counts[s][w][2] = sum h(k) h(k + m) rint(P2(cos) 2^e_s)           P1 = x, P2 = (3 x^2 - 1) / 2
      .data        Time, ``A-B-P1`` = C1(t), ``A-B-P2`` = C2(t) = counts[l] 2^-e_s / counts[0]; both are exactly 1 at
                   t = 0; NaN where a lag has no pair bonded at both ends
      .counts      int64 [n_sets][W][3] (the sets whose species are present, in dictionary order: ``.sets``)
      .scale_log2  [n_sets] e_s (``scale_log2``): a function of the trajectory, the set and the stride alone
      .n_origins   [W]
    Only pairs bonded at BOTH ends enter a lag: C_l(t) is the reorientation of the bonds that exist (again) after t, not
    of a fixed set of pairs.  A bonded pair of coincident atoms raises ZeroDivisionError, as ``Bad`` does.
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
                take contiguous shares of the centre atoms and all-reduce the sums once; False -> single process
        """
        br = cls()
        window, time = lags.window_setup(len(trajectory), delta_time, max_time, timestep)
        br.compute_reorientation(trajectory, nb_set_and_cutoff, window, time, origin_stride, device=device, distributed=distributed)
        return br

    def compute_reorientation(self, trajectory, nb_set_and_cutoff, window, time, origin_stride=1, device=None, distributed=None):
        origin_stride = lags.check_origin_stride(origin_stride)
        packed = lags.pack(trajectory, device)
        window = np.asarray(window, dtype=np.int32)
        rcm, names, live = lags.neighbour_sets(packed, nb_set_and_cutoff)
        n_orig = lags.n_origins(len(packed), window, origin_stride)
        logger.info("Start computing bond reorientation at %s times for %s sets", len(window), len(live))

        st = lags.setup(packed, device, distributed)
        ctx, merge = st.ctx, st.merge
        atoms = _dist.shard_range(packed.n_atoms, st.rank, st.world) if merge else (0, packed.n_atoms)
        W = len(window)

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            lags.begin_local(st.source)
            if not live:
                return np.zeros((0, W, 3), dtype=np.int64), np.zeros(0, dtype=np.int32)
            out = None
            if st.on_device:
                # the sums stay in HBM from the kernels through the RCCL all-reduce (amof_bond_reorientation_dev)
                import torch
                out = torch.zeros((len(live), W, 3), dtype=torch.int64, device=torch.device("cuda", ctx.device))
            return ctx.bond_reorientation(packed, rcm, live, window, origin_stride=origin_stride, atom_range=atoms, out=out)

        def finish(res):
            # the ranks' merge (the calling thread: collectives in program order): ONE all-reduce of the integer buffer; the
            # scale is the same on every rank
            counts, scale = res
            if live:
                counts = np.asarray(_dist.all_reduce_counts(counts, st.on_device, merge, ctx.device)).view(np.int64)
            self._assemble(counts, scale, names, n_orig, time)

        self._defer(ctx, local, finish, collective=merge and bool(live))

    def _assemble(self, counts, scale, names, n_orig, time):
        self.counts = counts
        self.scale_log2 = scale
        self.sets = [name for name, ok in names if ok]
        self.n_origins = n_orig
        self.data = assemble(counts, scale, names, time)

    def relaxation_time(self, rank=2):
        """``{set: tau}``: the trapezoid integral of C_rank(t) over ``Time`` (fs), per set.  A LOWER bound on the
        correlation time when C has not decayed to zero by the last lag (the tail beyond it is not seen); NaN lags (no pair
        bonded at both ends) end the integral."""
        if rank not in (1, 2):
            raise ValueError("rank must be 1 or 2")
        suffix = "-P%d" % rank
        d = self.data
        t = d["Time"].to_numpy(dtype=np.float64)
        out = {}
        for col in d.columns:
            if not col.endswith(suffix):
                continue
            s = d[col].to_numpy(dtype=np.float64)
            ok = np.isfinite(s)
            n = len(s) if ok.all() else int(np.argmin(ok))
            out[col[:-len(suffix)]] = float(np.sum(0.5 * (s[1:n] + s[:n - 1]) * np.diff(t[:n]))) if n > 0 else float("nan")
        return out

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.reor`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'reor'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote"""
        br = cls()
        br.data = pd.read_feather(_path.append_suffix(path_to_file, 'reor'))
        return br
