"""Lindemann index of neighbour pairs on MI355X: has the framework melted, and which bonds went soft first?

``Lindemann`` follows the LENGTH of every bonded pair of ``CoordinationNumber``'s sets through blocks of frames and reports its
relative root-mean-square fluctuation delta = sqrt(<d^2> - <d>^2) / <d>: per pair (a histogram), per centre atom and per
species pair, block after block through a heating ramp.  A glass stays below about 0.1, a liquid does not.  The integer sums
come from the HIP kernels behind ``amof_lindemann`` (amof_amd/csrc/lindemann.hip); the host keeps the block bookkeeping, the
divisions and the DataFrame.  The reference has no analysis that follows a pair through time.
"""

import logging
import math

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import dist as _dist
from . import lags
from .files import path as _path

logger = logging.getLogger(__name__)

SCALE_MAX = 40      # e_s never exceeds it
SCALE_MIN = 20      # below it the call is refused
SELECT = {"block": 0, "first": 1}


def blocks(n_frames, block, block_stride):
    """``(nb, starts, unused)``: the nb = (F - B) // S + 1 blocks [b S, b S + B) of F frames, their first frames and the number
    of frames behind the last block.  ValueError unless 2 <= B <= F and S >= 1 are integers"""
    if int(block) != block or int(block_stride) != block_stride:
        raise ValueError("block and block_stride must be integers")
    F, B, S = int(n_frames), int(block), int(block_stride)
    if B < 2 or B > F:
        raise ValueError("block of %d frames outside 2..%d" % (B, F))
    if S < 1:
        raise ValueError("block_stride must be an integer >= 1")
    nb = (F - B) // S + 1
    starts = np.arange(nb, dtype=np.int64) * S
    return nb, starts, F - (int(starts[-1]) + B)


def scale_log2(n_a, n_b, block):
    """the library's fixed-point exponent e_s = min(40, 62 - bit_length(n_A n_B ceil(sqrt(B)))): delta is at most sqrt(B - 1),
    so no sum of terms over n_A n_B pairs leaves int64.  ValueError below 20 (the library refuses the call)"""
    r = math.isqrt(int(block))
    r += r * r < int(block)
    e = min(SCALE_MAX, 62 - (int(n_a) * int(n_b) * r).bit_length())
    if e < SCALE_MIN:
        raise ValueError("%d x %d pairs in blocks of %d frames leave a fixed-point quantum above 2^-%d" % (n_a, n_b, block, SCALE_MIN))
    return e


def bin_count(delta_max, ddelta):
    """nbins = max(1, ceil(delta_max / ddelta - 1e-9)); the last bin takes every delta above"""
    if not ddelta > 0 or not delta_max > 0:
        raise ValueError("ddelta and delta_max must be positive")
    return max(1, int(math.ceil(delta_max / ddelta - 1e-9)))


def assemble(sums, scale, names, time):
    """``.data`` from the raw ``sums [nb][n_sets][2]`` (int64) and ``scale [n_sets]``: columns Time, then per set of ``names``
    = [(name, present)] ``A-B`` = the mean of delta over the block's pairs = sums[1] 2^-e / sums[0] and ``A-B-n`` = sums[0];
    both NaN where a block has no pair, and throughout for a set with an absent species (it has no column in ``sums``)"""
    data = {"Time": np.asarray(time, dtype=np.float64)}
    k = 0
    for name, live in names:
        if live:
            c = np.asarray(sums, dtype=np.int64)[:, k, :].astype(np.float64)
            q = np.ldexp(1.0, -int(scale[k]))
            k += 1
            with np.errstate(divide="ignore", invalid="ignore"):
                index = np.where(c[:, 0] > 0, c[:, 1] * q / c[:, 0], np.nan)
            n = np.where(c[:, 0] > 0, c[:, 0], np.nan)
        else:
            index = n = np.full(len(data["Time"]), np.nan)
        data[name] = index
        data[name + "-n"] = n
    return pd.DataFrame(data)


def assemble_hist(hist, names, ddelta):
    """``.hist``: ``delta`` bin centres and per present set the density of delta over the pairs of all blocks (its integral
    over the bins is 1; NaN for a set without a pair)"""
    hist = np.asarray(hist, dtype=np.uint64)
    nbins = hist.shape[2]
    data = {"delta": (np.arange(nbins) + 0.5) * float(ddelta)}
    k = 0
    for name, live in names:
        if not live:
            continue
        h = hist[:, k, :].sum(axis=0).astype(np.float64)
        k += 1
        data[name] = h / (h.sum() * float(ddelta)) if h.sum() > 0 else np.full(nbins, np.nan)
    return pd.DataFrame(data)


class Lindemann(Deferred):
    """
    Lindemann index (bond-length fluctuation) of neighbour pairs, per block of frames

    ``from_trajectory`` enqueues the analysis on its device's first lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

    Blocks: F frames, a block length B (2 <= B <= F) and a block stride S >= 1 give nb = (F - B) // S + 1 blocks; block b
    covers the frames [b S, b S + B).  Frame 0 is used (this is no lag analysis); frames behind the last block are not used
    (their number is logged).
    Sets, cutoffs and the bond indicator h_ij(f) are ``CoordinationNumber``'s and ``BondLifetime``'s: strict d < cutoff on the
    minimum image, a cutoff above half the smallest perpendicular cell height refused, a zero cutoff an empty set.
    Pairs of a block: the ordered pairs (centre i of A, neighbour j of B) with
      pairs='block'   h_ij(first frame of the block) = 1: the bonds that exist when the block starts
      pairs='first'   h_ij(0) = 1 in every block: a fixed population, whose delta keeps growing as the initial network dissolves
    d_ij(f) is the minimum-image distance in frame f's own cell.  A pair that drifts beyond half the cell is measured to its
    nearest image: delta of such a pair only means "large".  Per pair, with c = d(first frame of the block), e_f = d_f - c,
    sums in chunks of 64 frames (p1 += e, p2 = fma(e, e, p2), the chunks added in order): m1 = S1 / B, mean = c + m1,
    var = max(0, S2 / B - m1^2), delta = sqrt(var) / mean (0 where var is 0).
      .data        Time (timestep x first frame of the block), per set ``A-B`` = the mean of delta over the block's pairs and
                   ``A-B-n`` = their number; NaN where a block has no pair or a species is absent
      .hist        ``delta`` bin centres and per set the density of delta over all blocks (bins of ``ddelta`` up to
                   ``delta_max``; the last bin takes everything above)
      .hist_counts u64 [nb][n_sets][nbins];  .counts int64 [nb][n_sets][2] = (pairs, sum of llrint(delta 2^e_s))
      .scale_log2  [n_sets] e_s (``scale_log2``): a function of the trajectory, the set and B alone
      .sets        the sets whose species are present, in dictionary order
      .per_atom    (``per_atom=True``) float [nb][n_sets][N]: the mean delta of the pairs of centre i, NaN without pairs
    Time is expressed in fs.
    """

    data = EmptyUntilComputed("Time")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, block=None, block_stride=None, timestep=1, pairs='block', ddelta=0.005,
                        delta_max=0.5, per_atom=False, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory
            nb_set_and_cutoff: dict, keys are str indicating pair of neighbours ('Zn-N': centre Zn, neighbour N), values
                are cutoffs float, in Angstrom (``CoordinationNumber.from_trajectory``'s dictionary)
            block: frames per block (default: the whole trajectory); block_stride: frames between block starts (default: block)
            timestep: fs per frame
            pairs: 'block' or 'first' (see the class)
            ddelta, delta_max: bin width and range of the histogram of delta
            per_atom: also the mean delta per centre atom
            device: GPU index (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group (each holding the whole trajectory)
                take contiguous shares of the centre atoms and all-reduce the integer buffers once; False -> single process
        """
        li = cls()
        li.compute_lindemann(trajectory, nb_set_and_cutoff, block, block_stride, timestep, pairs, ddelta, delta_max, per_atom,
                             device=device, distributed=distributed)
        return li

    def compute_lindemann(self, trajectory, nb_set_and_cutoff, block=None, block_stride=None, timestep=1, pairs='block', ddelta=0.005,
                          delta_max=0.5, per_atom=False, device=None, distributed=None):
        if pairs not in SELECT:
            raise ValueError("pairs must be 'block' or 'first'")
        packed = lags.pack(trajectory, device)
        F, N = len(packed), packed.n_atoms
        block = F if block is None else block
        block_stride = block if block_stride is None else block_stride
        nb, starts, unused = blocks(F, block, block_stride)
        block, block_stride = int(block), int(block_stride)
        nbins = bin_count(delta_max, ddelta)
        time = starts * timestep
        rcm, names, live = lags.neighbour_sets(packed, nb_set_and_cutoff)
        # the library's refusal of a fixed-point quantum above 2^-20, before anything is queued
        species = np.asarray(_hip.packed_species(packed)[1])
        for a, b in live:
            scale_log2(int((species == a).sum()), int((species == b).sum()), block)
        if unused:
            logger.info("%s frames behind the last block are not used", unused)
        logger.info("Start computing the Lindemann index of %s blocks of %s frames for %s sets", nb, block, len(live))

        st = lags.setup(packed, device, distributed)
        ctx, merge = st.ctx, st.merge
        atoms = _dist.shard_range(N, st.rank, st.world) if merge else (0, N)
        n1, n2 = nb * len(live) * 2, nb * len(live) * nbins

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            lags.begin_local(st.source)
            if not live:
                pa = np.zeros((nb, 0, N, 2), dtype=np.int64) if per_atom else None
                return np.zeros(n1 + n2, dtype=np.int64), np.zeros(0, dtype=np.int32), pa
            out = flat = None
            if st.on_device:
                # sums and histogram stay in HBM from the kernels through the RCCL all-reduce (amof_lindemann_dev): one buffer
                import torch
                flat = torch.zeros(n1 + n2, dtype=torch.int64, device=torch.device("cuda", ctx.device))
                out = (flat[:n1], flat[n1:])
            res = ctx.lindemann(packed, rcm, live, block, block_stride, nbins, ddelta, select=SELECT[pairs], atom_range=atoms,
                                per_atom=per_atom, out=out)
            pa = res[3] if per_atom else None
            if flat is None:
                flat = np.concatenate([res[0].reshape(-1), res[1].view(np.int64).reshape(-1)])
            return flat, res[2], pa

        def finish(res):
            # the ranks' merge (the calling thread: collectives in program order): ONE all-reduce of the integer buffer -- the
            # per-atom rows of the ranks are disjoint and ride along; the scale is the same on every rank
            flat, scale, pa = res
            if live and merge:
                if per_atom:
                    if st.on_device:
                        import torch
                        flat = torch.cat([flat, torch.as_tensor(pa.reshape(-1)).to(flat.device)])
                    else:
                        flat = np.concatenate([flat, pa.reshape(-1)])
                flat = np.asarray(_dist.all_reduce_counts(flat, st.on_device, merge, ctx.device)).view(np.int64)
                if per_atom:
                    pa = flat[n1 + n2:].reshape(pa.shape)
            elif st.on_device and live:
                flat = flat.cpu().numpy()
            flat = np.asarray(flat).view(np.int64)
            sums = flat[:n1].reshape(nb, len(live), 2)
            hist = flat[n1:n1 + n2].view(np.uint64).reshape(nb, len(live), nbins)
            self._assemble(sums, hist, scale, pa, names, time, ddelta)

        self._defer(ctx, local, finish, collective=merge and bool(live))

    def _assemble(self, sums, hist, scale, pa, names, time, ddelta):
        self.counts = sums
        self.hist_counts = hist
        self.scale_log2 = scale
        self.sets = [name for name, ok in names if ok]
        self.per_atom = None
        if pa is not None:
            q = np.ldexp(1.0, -np.asarray(scale, dtype=np.int64))[None, :, None]
            n = pa[..., 0].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                self.per_atom = np.where(n > 0, pa[..., 1].astype(np.float64) * q / n, np.nan)
        self.hist = assemble_hist(hist, names, ddelta)
        self.data = assemble(sums, scale, names, time)

    def onset(self, threshold=0.1):
        """``{set: the first Time whose index is >= threshold, or NaN}``: where the set crosses the Lindemann criterion"""
        d = self.data
        t = d["Time"].to_numpy(dtype=np.float64)
        out = {}
        for col in d.columns:
            if col == "Time" or col.endswith("-n"):
                continue
            hit = np.nonzero(d[col].to_numpy(dtype=np.float64) >= threshold)[0]
            out[col] = float(t[hit[0]]) if len(hit) else float("nan")
        return out

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.lind`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'lind'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote"""
        li = cls()
        li.data = pd.read_feather(_path.append_suffix(path_to_file, 'lind'))
        return li
