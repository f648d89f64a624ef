"""Bond order parameters of neighbour shells on MI355X: Steinhardt q_l and the tetrahedral order parameter q_tet.

``BondOrder`` gives every centre atom of a neighbour set (``'Zn-N': 2.5`` -- ``CoordinationNumber``'s dictionary) one number
per l that says how ordered its shell of neighbours is, and a four-coordinated centre its tetrahedrality.  Both are
non-linear functions of ALL the angles of a centre, which the angle histogram of ``Bad`` cannot give.  By the addition
theorem of the spherical harmonics

    q_l(i)^2 = (n + 2 sum_{j<k} P_l(cos theta_jk)) / n^2            n = neighbours of centre i
    q_tet(i) = 1 - 3/8 sum_{j<k} (cos theta_jk + 1/3)^2             n == 4

so the HIP kernels behind ``amof_bond_order`` (amof_amd/csrc/nbr.hip) need the cosines ``Bad`` forms and a Legendre
recurrence; they return integers (fixed-point sums, counts), the host keeps the divisions and the DataFrames.  The
reference has no such analysis.
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _setup
from . import dist as _dist
from . import trajectory as _trajectory
from .files import path as _path

logger = logging.getLogger(__name__)

E = 40              # the per-pair terms are rounded to 2^-E
SUM_SCALE = 30      # the per-frame sums hold llrint(q 2^SUM_SCALE)


def values(n, T, U):
    """``(q_l [...][n_l], q_tet [...])`` float64 from the library's per-atom integers ``n [...]``, ``T [...][n_l]`` and
    ``U [...]`` by the formulas of include/amof_hip.h (sqrt, division and ldexp are IEEE: the same bits as the kernels');
    NaN where undefined (q_l: n < 1, q_tet: n != 4)"""
    n = np.asarray(n, dtype=np.int64)
    T = np.asarray(T, dtype=np.int64)
    U = np.asarray(U, dtype=np.int64)
    Q = np.maximum(0, (n[..., None] << E) + 2 * T)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.sqrt(np.ldexp(Q.astype(np.float64), -E)) / n[..., None].astype(np.float64)
    q = np.where(n[..., None] >= 1, q, np.nan)
    qt = np.where(n == 4, 1.0 - 0.375 * np.ldexp(U.astype(np.float64), -E), np.nan)
    return q, qt


def assemble(counts, counts_tet, frame_sums, names, l, step):
    """``(data, hist, hist_tet)`` from the raw integers: ``counts [n_live][n_l][nbins]``, ``counts_tet [n_live][nbins_tet]``,
    ``frame_sums [F][n_live][4 + n_l + 1]`` (rows of the live sets, in order) and ``names`` = [(set name, number of A
    centres, live)] in dictionary order -- live: both species present (the set has a row); 0 centres: species A absent.
      data      Step, and per set ``A-B-q<l>`` (mean over the centres with a neighbour, NaN if there are none), ``A-B-qtet``
                (mean over the four-coordinated centres), ``A-B-f4`` (fraction of the A centres with exactly four
                neighbours; NaN where A is absent, 0 where only B is)
      hist      ``q`` (bin centres of [0, 1]) and one density column ``A-B-q<l>`` per set and l, integrating to 1 (NaN
                where nothing was counted)
      hist_tet  the same for q_tet over [-3, 1], columns ``A-B-qtet``"""
    counts = np.asarray(counts)
    counts_tet = np.asarray(counts_tet)
    frame_sums = np.asarray(frame_sums, dtype=np.int64)
    l = [int(x) for x in l]
    n_l = len(l)
    F = frame_sums.shape[0]
    nbins, nbins_tet = counts.shape[-1], counts_tet.shape[-1]
    data = {"Step": np.asarray(step)[:F]}
    hist = {"q": (np.arange(nbins) + 0.5) / nbins}
    hist_tet = {"q": -3.0 + (np.arange(nbins_tet) + 0.5) * (4.0 / nbins_tet)}
    scale = np.ldexp(1.0, -SUM_SCALE)

    def density(c, width):
        c = np.asarray(c, dtype=np.uint64).astype(np.float64)
        total = c.sum()
        return c / (total * width) if total > 0 else np.full(len(c), np.nan)

    k = 0
    for name, n_a, live in names:
        if live:
            fs = frame_sums[:, k].astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                for q, lq in enumerate(l):
                    data["%s-q%d" % (name, lq)] = np.where(fs[:, 1] > 0, fs[:, 4 + q] * scale / fs[:, 1], np.nan)
                    hist["%s-q%d" % (name, lq)] = density(counts[k, q], 1.0 / nbins)
                data[name + "-qtet"] = np.where(fs[:, 2] > 0, fs[:, 4 + n_l] * scale / fs[:, 2], np.nan)
            data[name + "-f4"] = fs[:, 2] / n_a
            hist_tet[name + "-qtet"] = density(counts_tet[k], 4.0 / nbins_tet)
            k += 1
        else:
            for lq in l:
                data["%s-q%d" % (name, lq)] = np.full(F, np.nan)
                hist["%s-q%d" % (name, lq)] = np.full(nbins, np.nan)
            data[name + "-qtet"] = np.full(F, np.nan)
            data[name + "-f4"] = np.zeros(F) if n_a > 0 else np.full(F, np.nan)
            hist_tet[name + "-qtet"] = np.full(nbins_tet, np.nan)
    return pd.DataFrame(data), pd.DataFrame(hist), pd.DataFrame(hist_tet)


class BondOrder(Deferred):
    """
    Steinhardt q_l and tetrahedral order parameter of the neighbour shells of a trajectory

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

      .data        per frame: Step, ``A-B-q<l>``, ``A-B-qtet``, ``A-B-f4`` (``assemble``)
      .hist        distribution of q_l over centres and frames; .hist_tet: of q_tet
      .counts      u64 [n_sets][n_l][nbins], .counts_tet u64 [n_sets][nbins_tet], .frame_sums int64 [F][n_sets][4 + n_l + 1]
                   (the sets whose species are present, in dictionary order: ``.sets``)
      per_atom=True: .per_atom[set] float64 [F][N_A][n_l + 1] = (q_l ..., q_tet), NaN where undefined, and
                   .coordination[set] int [F][N_A], the centres in atom order
    A neighbour is ``CoordinationNumber``'s; a cutoff above half the smallest perpendicular cell height raises ValueError,
    a bonded pair of coincident atoms ZeroDivisionError (as ``Bad``), a centre with more than 64 neighbours an AmofError.
    """

    data = EmptyUntilComputed("Step")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, l=(4, 6), nbins=100, nbins_tet=400, delta_Step=1, first_frame=0,
                        per_atom=False, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, a PackedTrajectory or an XyzStream
            nb_set_and_cutoff: dict, keys are str indicating pair of neighbours ('Zn-N': centre Zn, neighbour N), values
                are cutoffs float, in Angstrom
            l: up to four degrees, each in 1 .. 12
            nbins, nbins_tet: bins of [0, 1] for q_l and of [-3, 1] for q_tet
            per_atom: keep the values of every centre
            device: GPU index or list of indices (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group take contiguous shares of the frames;
                False -> single process
        """
        bo = cls()
        step = _trajectory.construct_step(delta_Step=delta_Step, first_frame=first_frame, number_of_frames=len(trajectory))
        bo.compute_order(trajectory, nb_set_and_cutoff, step, l, nbins, nbins_tet, per_atom, device=device, distributed=distributed)
        return bo

    def compute_order(self, trajectory, nb_set_and_cutoff, step, l=(4, 6), nbins=100, nbins_tet=400, per_atom=False,
                      device=None, distributed=None):
        l = [int(x) for x in l]
        if not 1 <= len(l) <= 4 or any(not 1 <= x <= 12 for x in l):
            raise ValueError("l: one to four degrees, each in 1 .. 12")
        nbins, nbins_tet = int(nbins), int(nbins_tet)
        packed = _setup.pack(trajectory, device, keep_stream=True)
        logger.info("Start computing bond order parameters for %s frames", len(packed))
        ns = _setup.neighbour_sets(packed, nb_set_and_cutoff)
        rcm, live, centres = ns.cutoff, ns.live, ns.centres
        names = list(zip(ns.names, ns.n_centres, ns.present))
        n_l, cols = len(l), 4 + len(l) + 1

        st = _setup.setup(packed, device, distributed, lane=1, keep_stream=True, honour_local=True)
        ctx, source, sharded = st.ctx, st.source, st.sharded
        F, N = len(packed), packed.n_atoms
        frame_range = st.shard(F)
        numbers = np.asarray(packed.numbers)

        def empty(nf):
            return (np.zeros((0, n_l, nbins), dtype=np.uint64), np.zeros((0, nbins_tet), dtype=np.uint64),
                    np.zeros((nf, 0, cols), dtype=np.int64), np.zeros((nf, 0, N, 2 + n_l), dtype=np.int64) if per_atom else None)

        def finish_host(raw):
            hist, hist_tet, sums, pa = raw
            self._assemble(np.asarray(hist).view(np.uint64), np.asarray(hist_tet).view(np.uint64), sums, pa, names, centres, numbers,
                           l, step)

        if _setup.streamed(st):
            def walk():
                if not live:
                    return empty(F)
                res = _setup.walk(source, lambda batch: ctx.bond_order(batch, rcm, live, l, nbins, nbins_tet, per_atom=per_atom),
                                  ("sum", "sum", "cat", "cat")[:3 + bool(per_atom)])
                return res if per_atom else res + (None,)

            self._defer(ctx, walk, finish_host)
            return
        on_device = bool(live) and sharded and _dist.device_collectives()
        nq, nt = len(live) * n_l * nbins, len(live) * nbins_tet

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            if not live:
                return empty(frame_range[1] - frame_range[0])
            out = None
            if on_device:
                # the histograms stay in HBM from the kernels through ONE RCCL all-reduce (amof_bond_order_dev)
                import torch
                both = torch.zeros(nq + nt, dtype=torch.int64, device=torch.device("cuda", ctx.device))
                out = (both[:nq], both[nq:])
            res = ctx.bond_order(packed, rcm, live, l, nbins, nbins_tet, frame_range=frame_range, per_atom=per_atom, out=out)
            if on_device:
                return (both, None, res[2], res[3] if per_atom else None)
            return (res[0], res[1], res[2], res[3] if per_atom else None)

        def finish(raw):
            hist, hist_tet, sums, pa = raw
            if live and sharded:
                if on_device:
                    both = _dist.all_reduce_counts(hist, True, True, ctx.device)
                    hist, hist_tet = both[:nq].reshape(len(live), n_l, nbins), both[nq:].reshape(len(live), nbins_tet)
                else:
                    hist = _dist.all_reduce_counts(hist, False, True, ctx.device)
                    hist_tet = _dist.all_reduce_counts(hist_tet, False, True, ctx.device)
                sums = _dist.all_gather_rows(sums, device=ctx.device)
                if per_atom:
                    pa = _dist.all_gather_rows(pa, device=ctx.device)
            finish_host((hist, hist_tet, sums, pa))

        self._defer(ctx, local, finish, collective=sharded and bool(live))

    def _assemble(self, counts, counts_tet, frame_sums, pa, names, centres, numbers, l, step):
        self.counts = counts
        self.counts_tet = counts_tet
        self.frame_sums = frame_sums
        self.sets = [name for name, _, ok in names if ok]
        self.l = list(l)
        if pa is not None:
            self.per_atom, self.coordination = {}, {}
            F, n_l = frame_sums.shape[0], len(l)
            k = 0
            for (name, _, ok), a in zip(names, centres):
                idx = np.nonzero(numbers == a)[0]
                if ok:
                    rows = pa[:, k][:, idx]                  # [F][N_A][2 + n_l]
                    q, qt = values(rows[..., 0], rows[..., 1:1 + n_l], rows[..., 1 + n_l])
                    self.per_atom[name] = np.concatenate([q, qt[..., None]], axis=-1)
                    self.coordination[name] = rows[..., 0].copy()
                    k += 1
                else:
                    self.per_atom[name] = np.full((F, len(idx), n_l + 1), np.nan)
                    self.coordination[name] = np.zeros((F, len(idx)), dtype=np.int64)
        self.data, self.hist, self.hist_tet = assemble(counts, counts_tet, frame_sums, names, l, step)

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.order`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'order'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the file ``write_to_file`` wrote"""
        bo = cls()
        bo.data = pd.read_feather(_path.append_suffix(path_to_file, 'order'))
        return bo
