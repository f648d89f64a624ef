"""What the two reciprocal-space lag analyses, ``IntermediateScattering`` (F(q, t)) and ``CurrentCorrelation`` (C(q, t)),
decide and do alike on the host: the checks, vectors and work share before the kernels, and the merge of the ranks' one
int64 tensor (``_hip.lag_layout``) after them.  The lags, origins and the work list are amof_amd/lags.py's.
"""

import numpy as np

from . import _hip
from . import dist as _dist
from . import lags
from .structure_factor import enumerate_hkl, n_bins, pair_index


class Setup(object):
    """``packed``, ``dq``, ``nbins``, ``origin_stride``, ``window`` (i32), ``hkl``, ``elements``, ``n_orig [W]``, ``total``,
    ``st`` (``lags.setup``), ``work`` (this rank's range of the work list), ``S``, ``W``, ``own`` (what ``after_pack`` returned)"""


def setup(name, logger, trajectory, window, dq, qmax, max_points, seed, origin_stride, device, distributed, after_pack=None):
    """the front half of ``compute_isf`` / ``compute_current``; ``name``: "F(q, t)" / "C(q, t)" in the messages,
    ``logger``: the class's module's;
    ``after_pack(packed)``: the class's own inputs and checks, in their place behind the trajectory's"""
    s = Setup()
    s.dq, qmax = float(dq), float(qmax)
    if not s.dq > 0:
        raise ValueError("dq must be positive")
    s.nbins = n_bins(qmax, s.dq)
    if s.nbins < 1:
        raise ValueError("qmax // dq gives no bin")
    s.origin_stride = lags.check_origin_stride(origin_stride)
    s.packed = packed = lags.pack(trajectory, device)
    if not all(bool(x) for x in packed.pbc):
        raise ValueError("%s needs a cell periodic on all three axes" % name)
    s.own = after_pack(packed) if after_pack is not None else None
    s.window = np.asarray(window, dtype=np.int32)
    F = len(packed)
    if len(s.window) and (s.window.min() < 0 or s.window.max() >= max(F, 1)):
        raise ValueError("lag outside [0, n_frames)")
    # the origins of lag 0 (a superset of every lag's): StructureFactor(first_frame=1, frame_stride=s)'s frames
    frames = np.arange(1, max(1, F), s.origin_stride)
    cells = packed.cell if packed.cell.shape[0] == 1 else packed.cell[frames]
    s.hkl = enumerate_hkl(cells, qmax, dq=s.dq, max_points=max_points, seed=seed)
    s.elements = packed.unique_numbers()
    s.n_orig = lags.n_origins(F, s.window, s.origin_stride)
    s.total = int(s.n_orig.sum())
    logger.info("Start computing %s at %s times, %s vectors, %s bins, %s (lag, origin) pairs", name, len(s.window), len(s.hkl),
                s.nbins, s.total)
    s.st = lags.setup(packed, device, distributed)
    s.work = _dist.shard_range(s.total, s.st.rank, s.st.world) if s.st.merge else (0, s.total)
    s.S = len(_hip.packed_species(packed)[0])
    s.W = len(s.window)
    return s


def local(name, s, lay, accumulate):
    """this rank's kernels (a lane job: amof_amd/_lazy.py): ``accumulate(flat)``, flat the zeroed int64 tensor of ``lay`` the
    ranks all-reduce once (integer fixed-point sums at a scale every rank arrives at: the shares add up exactly, whatever
    the split), or None without a merge"""
    lags.begin_local(s.st.source)
    flat = None
    if s.st.merge:
        import torch
        flat = torch.zeros(lay["size"], dtype=torch.int64, device=torch.device("cuda", s.st.ctx.device))
    try:
        return accumulate(flat)
    except _hip.AmofError as e:
        if e.code != _hip.AMOF_ECAPACITY:
            raise
        # (no chunks of frames here: they would cut the lags)
        raise ValueError("%s: %s.  Remedies: fewer vectors per bin (max_points) or a larger dq; origin_stride "
                         "does not help (the scale is set by the trajectory's frame count)" % (name, e)) from e


def normalise(data, window):
    """``data`` divided, lag by lag, by its own t = 0 rows (every column but Time and q)"""
    window = np.asarray(window)
    zero = np.flatnonzero(window == 0)
    if not len(zero):
        raise ValueError("normalised() needs lag 0 among the windows")
    W = len(window)
    nbins = len(data) // W if W else 0
    out = data.copy()
    for name in data.columns:
        if name in ("Time", "q"):
            continue
        v = data[name].to_numpy(dtype=np.float64).reshape(W, nbins)
        with np.errstate(divide="ignore", invalid="ignore"):
            out[name] = (v / v[zero[0]][None, :]).reshape(-1)
    return out


class Merged(object):
    """the ranks' tensors added up, on the host: ``counts [W][nbins]``, ``beyond [W]`` (u64 views) and ``block(name)``"""

    def __init__(self, s, lay, flat, scale_log2):
        if s.st.on_device:
            _dist.all_reduce_sum(flat)          # (in HBM)
            flat = flat.cpu().numpy()
        else:
            flat = _dist.all_reduce_sum(flat.cpu().numpy(), device=s.st.ctx.device)
        self.flat, self.lay, self.S, self.W, self.nbins = flat, lay, s.S, s.W, s.nbins
        n = s.W * s.nbins
        self.counts = flat[lay["counts"]:lay["counts"] + n].reshape(s.W, s.nbins).view(np.uint64)
        self.beyond = flat[lay["beyond"]:lay["beyond"] + s.W].view(np.uint64)
        pidx = pair_index(s.S)
        self.exp2 = np.array([[scale_log2[pidx[(min(a, c), max(a, c))]] for c in range(s.S)] for a in range(s.S)], dtype=np.int64)

    def block(self, name, diagonal=False):
        """f64 ``[S][S][W][nbins]`` (``diagonal``: ``[S][W][nbins]``, the pairs (a, a)) of the fixed-point block ``name``"""
        S, W, nbins = self.S, self.W, self.nbins
        shape, exp2 = ((S, W, nbins), np.diag(self.exp2)[:, None, None]) if diagonal else ((S, S, W, nbins), self.exp2[:, :, None, None])
        at = self.lay[name]
        return np.ldexp(self.flat[at:at + int(np.prod(shape))].reshape(shape).astype(np.float64), -exp2)
