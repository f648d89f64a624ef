"""Static structure factor S(q) on MI355X, by direct summation over the reciprocal lattice of the periodic cell.

``StructureFactor`` sums rho_a(k) = sum_j exp(i k.r_j) over the atoms of every species a for every reciprocal-lattice vector
k = h b1 + k b2 + l b3 with |k| < qmax (half a space: rho(-k) = conj rho(k)) and bins the products Re rho_a rho_b* by |k|.
This is the exact S(q) of the periodic cell, free of the truncation ripples of a Fourier transform of g(r) cut at half the
cell.  The phase sums run in the HIP kernels behind ``amof_sq_accumulate`` (exact u32 phases, include/amof_hip.h); the
host keeps the choice of vectors, the normalisation and the DataFrames.  The reference has no such analysis.
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
from .frames import pack_trajectory

logger = logging.getLogger(__name__)

reciprocal = _hip.reciprocal


def n_bins(qmax, dq):
    """``int(qmax // dq)`` with Python float floor-division, as ``Rdf`` counts its bins"""
    return int(float(qmax) // float(dq))


def half_space(hkl):
    """mask of the triples whose first nonzero index is positive"""
    hkl = np.asarray(hkl).reshape(-1, 3)
    h, k, l = hkl[:, 0], hkl[:, 1], hkl[:, 2]
    return (h > 0) | ((h == 0) & (k > 0)) | ((h == 0) & (k == 0) & (l > 0))


def q_norms(recip, hkl):
    """|q| of every triple for one reciprocal matrix, in the library's operation order (no fma)"""
    R = np.asarray(recip, dtype=np.float64)
    h, k, l = (np.asarray(hkl, dtype=np.float64)[:, c] for c in range(3))
    qx = (h * R[0, 0] + k * R[1, 0]) + l * R[2, 0]
    qy = (h * R[0, 1] + k * R[1, 1]) + l * R[2, 1]
    qz = (h * R[0, 2] + k * R[1, 2]) + l * R[2, 2]
    return np.sqrt((qx * qx + qy * qy) + qz * qz)


def enumerate_hkl(cells, qmax, dq=None, max_points=None, seed=0):
    """int32 ``[K][3]``: the half-space triples that can reach |q| < qmax in some of ``cells`` (``[n][3][3]``, the selected
    frames' cells), sorted.

    The box is bounded by the largest cell lengths (|h| <= qmax |a1| / 2 pi); a triple is kept when |q| on the mean
    reciprocal matrix lies below qmax + d |hkl|, d the largest spectral norm of a frame's deviation from that mean -- a
    superset of every frame's ball (the kernel decides the bins per frame).  ``max_points``: a bin of width ``dq``
    (judged on the mean cell) with more vectors keeps a subsample of ``max_points`` of them, drawn with
    ``numpy.random.default_rng(seed)`` (the same for the same arguments)."""
    cells = np.asarray(cells, dtype=np.float64).reshape(-1, 3, 3)
    qmax = float(qmax)
    if qmax <= 0 or len(cells) == 0:
        return np.zeros((0, 3), dtype=np.int32)
    lengths = np.sqrt((cells ** 2).sum(axis=2)).max(axis=0)
    H = np.floor(qmax * lengths / (2.0 * np.pi)).astype(np.int64)
    R = reciprocal(cells)
    Rm = R.mean(axis=0)
    dev = max(float(np.linalg.norm(r - Rm, 2)) for r in R) if len(R) > 1 else 0.0
    out = []
    hs = np.arange(-H[0], H[0] + 1)
    ks = np.arange(-H[1], H[1] + 1)
    ls = np.arange(-H[2], H[2] + 1)
    kk, ll = np.meshgrid(ks, ls, indexing="ij")
    kk, ll = kk.reshape(-1), ll.reshape(-1)
    for h in hs:                           # one h plane at a time: memory O(box / (2H + 1))
        t = np.stack([np.full_like(kk, h), kk, ll], axis=1)
        t = t[half_space(t)]
        if not len(t):
            continue
        q = q_norms(Rm, t)
        keep = q < qmax + dev * np.sqrt((t.astype(np.float64) ** 2).sum(axis=1)) if dev else q < qmax
        out.append(t[keep])
    hkl = np.concatenate(out) if out else np.zeros((0, 3), dtype=np.int64)
    if max_points is not None and len(hkl):
        if dq is None:
            raise ValueError("max_points needs dq")
        b = (q_norms(Rm, hkl) / float(dq)).astype(np.int64)
        rng = np.random.default_rng(seed)
        order = np.argsort(b, kind="stable")
        starts = np.flatnonzero(np.r_[True, np.diff(b[order]) != 0])
        ends = np.r_[starts[1:], len(order)]
        keep = np.ones(len(hkl), dtype=bool)
        for s0, s1 in zip(starts, ends):
            if s1 - s0 > int(max_points):
                members = order[s0:s1]
                drop = np.ones(s1 - s0, dtype=bool)
                drop[rng.choice(s1 - s0, size=int(max_points), replace=False)] = False
                keep[members[drop]] = False
        hkl = hkl[keep]
    return np.ascontiguousarray(hkl, dtype=np.int32)


def pair_index(S):
    """``{(a, b): p}`` for a <= b in the library's pair order (0,0), (0,1) .. (0,S-1), (1,1) .."""
    idx, p = {}, 0
    for a in range(S):
        for b in range(a, S):
            idx[(a, b)] = p
            p += 1
    return idx


def assemble(counts, sums, kinds, elements, species_counts, dq):
    """``.data`` from the raw outputs of ``amof_sq_accumulate`` (counts [nbins], sums [P][nbins] in library species
    order ``kinds``); ``elements``: atomic numbers in column order; ``species_counts``: {atomic number: atoms}.
      q      left bin edge b dq
      X-X    (sum_a sums_aa + 2 sum_{a<b} sums_ab) / (counts N)
      A-B    sums_ab / (counts sqrt(N_A N_B)) for every ordered pair (Ashcroft-Langreth), named and ordered as ``Rdf.data``
    Bins with no samples are NaN."""
    counts = np.asarray(counts, dtype=np.float64)
    sums = np.asarray(sums, dtype=np.float64)
    nbins = len(counts)
    S = len(kinds)
    pidx = pair_index(S)
    N = float(sum(species_counts[int(z)] for z in kinds))
    denom = np.where(counts > 0, counts, np.nan)
    cols = {"q": np.arange(nbins, dtype=np.float64) * dq}
    tot = np.zeros(nbins)
    for (a, b), p in pidx.items():
        tot = tot + (sums[p] if a == b else 2.0 * sums[p])
    cols["X-X"] = tot / (denom * N)
    idx = {int(z): k for k, z in enumerate(kinds)}
    syms = [_data.chemical_symbols[int(z)] for z in elements]
    for i, zi in enumerate(elements):
        for j, zj in enumerate(elements):
            a, b = sorted((idx[int(zi)], idx[int(zj)]))
            norm = np.sqrt(float(species_counts[int(zi)]) * float(species_counts[int(zj)]))
            cols[syms[i] + "-" + syms[j]] = sums[pidx[(a, b)]] / (denom * norm)
    return pd.DataFrame(cols)


def density_modes(trajectory, hkl, frame=0, device=None):
    """``(rho, kinds)``: rho_a(k) = sum over the atoms of species a of exp(i k.r) of one frame, complex ``[K][S]``, for the
    integer triples ``hkl`` (any, but (0, 0, 0); k = h b1 + k b2 + l b3), species in ``kinds`` order (sorted atomic
    numbers) -- ``amof_sq_modes``: anisotropic S(k), single reflections."""
    packed = pack_trajectory(trajectory, device=device if device is not None else _hip.default_device())
    if getattr(packed, "is_stream", False):
        packed = packed.read_all()
    if not all(bool(x) for x in packed.pbc):
        raise ValueError("S(q) needs a cell periodic on all three axes")
    dev = device if device is not None else getattr(packed, "device_index", None)
    return _hip.get_context(dev).sq_modes(packed, hkl, frame=frame)


def accumulate_in_chunks(ctx, packed, hkl, dq, nbins, frame_range, stride):
    """``Context.sq_accumulate`` of the frames ``frame_range[0], + stride, ... < frame_range[1]`` for trajectories whose
    whole frame count exceeds the library's fixed-point range (AMOF_ECAPACITY): the selection is cut into 2, 4, 8 ...
    chunks, each passed as a trajectory of its own frames only (with its own fixed-point scale), and the float64 results
    are added in chunk order.  Returns ``(counts, sums, beyond, kinds)``."""
    from .frames import PackedTrajectory
    sel = np.arange(frame_range[0], frame_range[1], stride)
    kinds = _hip.packed_species(packed)[0]
    S = len(kinds)
    if not len(sel):
        return np.zeros(nbins, dtype=np.uint64), np.zeros((S * (S + 1) // 2, nbins)), 0, kinds
    n_chunks = 2
    while True:
        parts = [p for p in np.array_split(sel, min(n_chunks, len(sel))) if len(p)]
        try:
            total = None
            for p in parts:
                a, b = int(p[0]), int(p[-1]) + 1
                cell = packed.cell if packed.cell.shape[0] == 1 else packed.cell[a:b]
                sub = PackedTrajectory(packed.pos[a:b], cell, packed.numbers, packed.masses, packed.pbc)
                r = ctx.sq_accumulate(sub, hkl, dq, nbins, frame_stride=stride)
                total = r if total is None else (total[0] + r[0], total[1] + r[1], total[2] + r[2], r[3])
            return total
        except _hip.AmofError as e:
            if e.code != _hip.AMOF_ECAPACITY or len(parts) >= len(sel):
                raise
            n_chunks *= 2


class StructureFactor(Deferred):
    """
    Static structure factor S(q) by direct summation over reciprocal-lattice vectors

    ``from_trajectory`` enqueues the analysis on its device's first lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

      .data    q (left bin edge, 1/Angstrom), X-X, then every ordered pair A-B (Ashcroft-Langreth partials,
               S_AB = <Re rho_A rho_B*> / sqrt(N_A N_B)); NaN in bins without a vector
      .counts [nbins] vectors per bin (over the frames), .sums [P][nbins] sums of Re rho_a rho_b* (pairs a <= b of
      .kinds), .hkl the vectors, .beyond the (frame, vector) samples with |q| >= nbins dq
    ``weighted(weights)`` combines the partials with scattering lengths or form factors.
    """

    data = EmptyUntilComputed("q")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, dq=0.02, qmax=5.0, max_points=None, seed=0, first_frame=0, last_frame=None,
                        frame_stride=1, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, or a PackedTrajectory (periodic on all three axes)
            dq, qmax: bin width and range in 1/Angstrom; nbins = int(qmax // dq)
            max_points: at most this many vectors per bin (a seeded subsample; None: every vector)
            first_frame, last_frame, frame_stride: the frames first_frame, + frame_stride, ... < last_frame
            device: GPU index (default: LOCAL_RANK or 0)
            distributed: None -> shard the selected frames over the ranks of an initialised torch.distributed group
                (every rank holds the whole trajectory); False -> single process
        """
        sq = cls()
        sq.compute_sq(trajectory, dq, qmax, max_points, seed, first_frame, last_frame, frame_stride, device=device,
                      distributed=distributed)
        return sq

    def compute_sq(self, trajectory, dq=0.02, qmax=5.0, max_points=None, seed=0, first_frame=0, last_frame=None, frame_stride=1,
                   device=None, distributed=None):
        dq, qmax = float(dq), float(qmax)
        if not dq > 0:
            raise ValueError("dq must be positive")
        nbins = n_bins(qmax, dq)
        if nbins < 1:
            raise ValueError("qmax // dq gives no bin")
        packed = _setup.pack(trajectory, device)      # (read whole: not walked batch by batch)
        if not all(bool(x) for x in packed.pbc):
            raise ValueError("S(q) needs a cell periodic on all three axes")
        F = len(packed)
        f0, f1, stride = int(first_frame), F if last_frame is None else min(int(last_frame), F), int(frame_stride)
        if stride < 1 or f0 < 0:
            raise ValueError("bad frame selection")
        frames = np.arange(f0, max(f0, f1), stride)
        cells = packed.cell if packed.cell.shape[0] == 1 else packed.cell[frames]
        hkl = enumerate_hkl(cells, qmax, dq=dq, max_points=max_points, seed=seed)
        elements = packed.unique_numbers()
        logger.info("Start computing S(q) for %s frames, %s vectors, %s bins", len(frames), len(hkl), nbins)

        # (the selected frames are sharded whenever the ranks merge: 'local' has no meaning of its own here)
        st = _setup.setup(packed, device, distributed, lane=0, honour_local=False)
        ctx, merge, source = st.ctx, st.merge, st.source
        a, b = st.shard(len(frames))
        frame_range = (f0 + a * stride, min(f1, f0 + b * stride)) if b > a else (f0, f0)
        S = len(_hip.packed_species(packed)[0])
        P = S * (S + 1) // 2
        on_device = merge and _dist.device_collectives()

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            _setup.begin_local(source)
            try:
                if merge:
                    # integer fixed-point sums: the ranks' shares add up exactly, whatever the sharding.  Counts, beyond
                    # and sums in ONE int64 tensor: one all-reduce
                    import torch
                    flat = torch.zeros(nbins + 1 + P * nbins, dtype=torch.int64, device=torch.device("cuda", ctx.device))
                    out = (flat[:nbins + 1], flat[nbins + 1:].view(P, nbins))
                    _, _, scale, kinds = ctx.sq_accumulate(packed, hkl, dq, nbins, frame_range=frame_range, frame_stride=stride,
                                                           out=out)
                    return flat, scale, kinds
                return ctx.sq_accumulate(packed, hkl, dq, nbins, frame_range=frame_range, frame_stride=stride)
            except _hip.AmofError as e:
                # the whole trajectory exceeds the fixed-point range (the same on every rank: the scale depends on the
                # trajectory, the vectors and the bins only): chunks of frames, float64 sums
                if e.code != _hip.AMOF_ECAPACITY:
                    raise
                logger.info("S(q): %s; accumulating in chunks of frames", e)
                return ("chunked",) + accumulate_in_chunks(ctx, packed, hkl, dq, nbins, frame_range, stride)

        def finish(raw):
            if isinstance(raw[0], str):           # ("chunked", counts, sums, beyond, kinds)
                _, counts, sums, beyond, kinds = raw
                if merge:
                    counts = _dist.all_reduce_sum(counts, device=ctx.device)
                    sums = _dist.all_reduce_sum(sums, device=ctx.device)
                    beyond = int(_dist.all_reduce_sum(np.array([beyond], dtype=np.int64), device=ctx.device)[0])
            elif merge:
                flat, scale, kinds = raw
                if on_device:
                    _dist.all_reduce_sum(flat)          # (in HBM)
                    flat = flat.cpu().numpy()
                else:
                    flat = _dist.all_reduce_sum(flat.cpu().numpy(), device=ctx.device)
                beyond = int(flat[nbins])
                counts = flat[:nbins].view(np.uint64)
                sums = np.ldexp(flat[nbins + 1:].reshape(P, nbins).astype(np.float64), -np.asarray(scale, dtype=np.int64)[:, None])
            else:
                counts, sums, beyond, kinds = raw
            self._assemble(counts, sums, beyond, kinds, hkl, packed, elements, dq)

        self._defer(ctx, local, finish, collective=merge)

    def _assemble(self, counts, sums, beyond, kinds, hkl, packed, elements, dq):
        self.kinds = list(kinds)
        self.counts, self.sums, self.beyond, self.hkl = counts, sums, int(beyond), hkl
        self.dq = dq
        self.n_atoms = packed.n_atoms
        self.species_counts = {int(z): int(n) for z, n in packed.species_counts().items()}
        self.elements = [int(z) for z in elements]
        self.data = assemble(counts, sums, kinds, elements, self.species_counts, dq)

    def weighted(self, weights):
        """``DataFrame`` q, S: S_w(q) = sum over ordered pairs (a, b) of w_a w_b sums_ab / (counts sum_a N_a w_a^2).

        ``weights``: {element symbol or atomic number: float, or a callable of q in 1/Angstrom (evaluated at the bins'
        left edges)} -- neutron scattering lengths or X-ray form factors, for every element of the system.  Equal weights
        give ``X-X``.  Host only."""
        counts = np.asarray(self.counts, dtype=np.float64)
        q = np.arange(len(counts), dtype=np.float64) * self.dq
        w = []
        for z in self.kinds:
            sym = _data.chemical_symbols[int(z)]
            v = weights[sym] if sym in weights else weights[int(z)]
            w.append(np.asarray(v(q), dtype=np.float64) * np.ones_like(q) if callable(v) else np.full_like(q, float(v)))
        sums = np.asarray(self.sums, dtype=np.float64)
        num = np.zeros_like(q)
        for (a, b), p in pair_index(len(self.kinds)).items():
            num = num + (1.0 if a == b else 2.0) * w[a] * w[b] * sums[p]
        norm = np.zeros_like(q)
        for a, z in enumerate(self.kinds):
            norm = norm + self.species_counts[int(z)] * w[a] * w[a]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = num / (np.where(counts > 0, counts, np.nan) * norm)
        return pd.DataFrame({"q": q, "S": s})

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.sq`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'sq'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote (``.data`` only)"""
        sq = cls()
        sq.data = pd.read_feather(_path.append_suffix(path_to_file, 'sq'))
        return sq
