"""Dihedral (torsion) angle distributions of chains of four bonded atoms on MI355X.

``Dihedral`` gives, for every pattern ``'A-B-C-D'`` of species, the distribution of the angle AROUND the bond b-c of every
chain a-b-c-d of bonded atoms: the angle between the planes (a, b, c) and (b, c, d), folded into 0 .. 180 degrees (0: cis,
180: trans).  ``Rdf`` stops at two bodies and ``Bad``, ``BondOrder`` at three; the rotation of an imidazolate about its Zn-N
bond (``C-N-Zn-N``), the planarity of a ring (``C-N-C-N``) or the conformation of a linker (``H-C-N-Zn``) are four-body
quantities.  The HIP kernels behind ``amof_dihedral_hist`` (amof_amd/csrc/nbr.hip, dihedral_math.h) return integers (bins,
counts, fixed-point cosine sums); the host keeps the divisions and the DataFrames.  The reference has no such analysis.
"""

import itertools
import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import _setup
from . import atom as amatom
from . import data as _data
from . import dist as _dist
from . import trajectory as _trajectory
from .files import path as _path

logger = logging.getLogger(__name__)

E = 40              # the per-chain cosines are rounded to 2^-E
MAX_CHAINS = 32


def bins(dphi):
    """``(edges [nb + 1], centres [nb])`` as ``Bad``'s: ``int(180 // dphi) + 1`` bins of width dphi from 0"""
    dphi = float(dphi)
    if not (np.isfinite(dphi) and 0.0 < dphi <= 180.0):
        raise ValueError("dphi must be a number of degrees in (0, 180], not %r" % (dphi,))
    n = int(180 // dphi)
    return np.arange(n + 2) * dphi, np.arange(n + 1) * dphi + dphi / 2


def parse_chain(text):
    """``'C-N-Zn-N'`` -> atomic numbers, ``'X'`` -> -1"""
    parts = str(text).split('-')
    if len(parts) != 4 or any(not p for p in parts):
        raise ValueError("a chain pattern names four species, 'A-B-C-D' with X for any: %r" % (text,))
    out = []
    for p in parts:
        if p == 'X':
            out.append(-1)
        elif p in _data.atomic_numbers:
            out.append(int(_data.atomic_numbers[p]))
        else:
            raise ValueError("unknown chemical symbol %r in chain pattern %r" % (p, text))
    return tuple(out)


def chain_name(numbers):
    return "-".join("X" if z < 0 else _data.chemical_symbols[z] for z in numbers)


def default_chains(cutoff_dict, present):
    """every pattern over the species ``present`` whose three consecutive pairs all have a cutoff, one of each reversal pair
    (the one whose tuple of atomic numbers sorts first), in sorted order"""
    bonded = set()
    for (a, b), rc in cutoff_dict.items():
        if rc > 0:
            bonded.add((a, b))
            bonded.add((b, a))
    kinds = sorted(int(z) for z in present)
    out = []
    for c in itertools.product(kinds, repeat=4):
        if c <= c[::-1] and all((c[k], c[k + 1]) in bonded for k in range(3)):
            out.append(c)
    if len(out) > MAX_CHAINS:
        raise ValueError("%d chain patterns follow from the dictionary, more than %d: name the ones wanted in chains=[...]"
                         % (len(out), MAX_CHAINS))
    return out


def assemble(hist, n_dihedrals, n_undefined, frame_sums, names, edges, phi, step):
    """``(data, frames)`` from the raw integers ``hist [T][nb]``, ``n_dihedrals [T]``, ``n_undefined [T]`` and
    ``frame_sums [F][T][3]``:
      data    ``phi`` (bin centres) and one density column per pattern, ``numpy.histogram(density=True)``'s as in ``Bad``;
              a pattern without any dihedral has no column
      frames  per Step and pattern ``name-n`` (defined chains), ``name-undefined`` and ``name-cos`` (the mean cosine of the
              frame's defined chains, NaN where there is none)"""
    hist = np.asarray(hist)
    frame_sums = np.asarray(frame_sums, dtype=np.int64)
    F = frame_sums.shape[0]
    width = np.array(np.diff(edges), float)
    cols = {"phi": phi}
    frames = {"Step": np.asarray(step)[:F]}
    for k, name in enumerate(names):
        if int(n_dihedrals[k]) != 0:
            n = hist[k].astype(np.int64)
            cols[name] = n / width / n.sum()
        fs = frame_sums[:, k]
        frames[name + "-n"] = fs[:, 0]
        frames[name + "-undefined"] = fs[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            frames[name + "-cos"] = np.where(fs[:, 0] > 0, np.ldexp(fs[:, 2].astype(np.float64), -E) / fs[:, 0], np.nan)
    return pd.DataFrame(cols), pd.DataFrame(frames)


class Dihedral(Deferred):
    """
    Torsion-angle distributions of the chains of four bonded atoms of a trajectory

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; ``.data`` (and every other result)
    waits for it (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

      .data      ``phi`` and one density column per pattern (``assemble``)
      .frames    per Step and pattern: ``name-n``, ``name-undefined``, ``name-cos``
      .counts    the raw integers: ``{"hist": u64 [T][nb], "n_dihedrals": u64 [T], "n_undefined": u64 [T],
                 "frame_sums": int64 [F][T][3]}``
      .chains    the pattern names, in order
    The bond graph is ``Ring``'s (symmetric: 'Zn-N' bonds N to Zn as well).  A cutoff above half the smallest perpendicular
    cell height raises ValueError, a bonded pair of coincident atoms ZeroDivisionError (as ``Bad``), an atom with more than
    16 neighbours an AmofError that names the frame.
    """

    data = EmptyUntilComputed("phi")

    def __init__(self):
        """default constructor"""
        self.data = None

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, chains=None, dphi=1.0, delta_Step=1, first_frame=0, device=None,
                        distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, a PackedTrajectory or an XyzStream
            nb_set_and_cutoff: dict, keys are str indicating pair of neighbours, values are cutoffs float, in Angstrom
                (symmetric, as ``Ring``'s)
            chains: list of 'A-B-C-D' patterns, X for any species; None: every pattern over the species present whose
                three consecutive pairs are all in the dictionary, one of each reversal pair
            dphi: bin width in degrees
            device: GPU index or list of indices (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group take contiguous shares of the frames;
                False -> single process
        """
        dh = cls()
        step = _trajectory.construct_step(delta_Step=delta_Step, first_frame=first_frame, number_of_frames=len(trajectory))
        dh.compute_dihedral(trajectory, nb_set_and_cutoff, step, chains, dphi, device=device, distributed=distributed)
        return dh

    def compute_dihedral(self, trajectory, nb_set_and_cutoff, step, chains=None, dphi=1.0, device=None, distributed=None):
        # arguments first: nothing below touches a device until they have passed
        edges, phi = bins(dphi)
        if not nb_set_and_cutoff:
            raise ValueError("nb_set_and_cutoff names no pair of neighbours")
        try:
            cutoff_dict = amatom.format_cutoff(nb_set_and_cutoff, sort_pair=True)
        except KeyError as e:
            raise ValueError("unknown chemical symbol %s in nb_set_and_cutoff" % (e,))
        if any(len(k) != 2 for k in cutoff_dict):
            raise ValueError("nb_set_and_cutoff: keys name a pair of species, 'A-B'")
        wanted = None if chains is None else [parse_chain(c) for c in chains]
        if wanted is not None and not 1 <= len(wanted) <= MAX_CHAINS:
            raise ValueError("chains: 1 to %d patterns, not %d" % (MAX_CHAINS, len(wanted)))
        packed = _setup.pack(trajectory, device, keep_stream=True)
        logger.info("Start computing dihedral distributions for %s frames with dphi = %s", len(packed), dphi)
        kinds, _ = _hip.packed_species(packed)
        if wanted is None:
            wanted = default_chains(cutoff_dict, kinds)
        names = [chain_name(c) for c in wanted]
        lut = {int(z): k for k, z in enumerate(kinds)}
        # a pattern that names an absent species matches nothing: it keeps its (zero) rows and gets no column
        live = [k for k, c in enumerate(wanted) if all(z < 0 or z in lut for z in c)]
        idx = [[-1 if z < 0 else lut[z] for z in wanted[k]] for k in live]
        rcm = amatom.cutoff_matrix(cutoff_dict, kinds)
        T, nb, TL = len(wanted), len(phi), len(live)

        st = _setup.setup(packed, device, distributed, lane=1, keep_stream=True, honour_local=True)
        ctx, source, sharded = st.ctx, st.source, st.sharded
        F = len(packed)
        frame_range = st.shard(F)

        def empty(nf):
            return (np.zeros((0, nb), dtype=np.uint64), np.zeros(0, dtype=np.uint64), np.zeros(0, dtype=np.uint64),
                    np.zeros((nf, 0, 3), dtype=np.int64))

        def finish_host(raw):
            hist, n_def, n_undef, sums = raw
            full = (np.zeros((T, nb), dtype=np.uint64), np.zeros(T, dtype=np.uint64), np.zeros(T, dtype=np.uint64),
                    np.zeros((np.asarray(sums).shape[0], T, 3), dtype=np.int64))
            if live:
                full[0][live] = np.asarray(hist).view(np.uint64).reshape(TL, nb)
                full[1][live] = np.asarray(n_def).view(np.uint64).reshape(TL)
                full[2][live] = np.asarray(n_undef).view(np.uint64).reshape(TL)
                full[3][:, live] = sums
            self._assemble(full, names, edges, phi, step)

        if _setup.streamed(st):
            def walk():
                if not live:
                    return empty(F)
                return _setup.walk(source, lambda batch: ctx.dihedral_hist(batch, rcm, idx, edges), ("sum", "sum", "sum", "cat"))

            self._defer(ctx, walk, finish_host)
            return
        on_device = bool(live) and sharded and _dist.device_collectives()
        nh = TL * nb

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            if not live:
                return empty(frame_range[1] - frame_range[0])
            if on_device:
                # the counts stay in HBM from the kernels through ONE RCCL all-reduce (amof_dihedral_hist_dev)
                import torch
                allc = torch.zeros(nh + 2 * TL, dtype=torch.int64, device=torch.device("cuda", ctx.device))
                res = ctx.dihedral_hist(packed, rcm, idx, edges, frame_range=frame_range,
                                        out=(allc[:nh], allc[nh:nh + TL], allc[nh + TL:]))
                return (allc, None, None, res[3])
            return ctx.dihedral_hist(packed, rcm, idx, edges, frame_range=frame_range)

        def finish(raw):
            hist, n_def, n_undef, sums = raw
            if live and sharded:
                if on_device:
                    allc = _dist.all_reduce_counts(hist, True, True, ctx.device)
                    hist, n_def, n_undef = allc[:nh].reshape(TL, nb), allc[nh:nh + TL], allc[nh + TL:]
                else:
                    hist = _dist.all_reduce_counts(hist, False, True, ctx.device)
                    n_def = _dist.all_reduce_counts(n_def, False, True, ctx.device)
                    n_undef = _dist.all_reduce_counts(n_undef, False, True, ctx.device)
                sums = _dist.all_gather_rows(sums, device=ctx.device)
            finish_host((hist, n_def, n_undef, sums))

        self._defer(ctx, local, finish, collective=sharded and bool(live))

    def _assemble(self, full, names, edges, phi, step):
        hist, n_def, n_undef, sums = full
        self.counts = {"hist": hist, "n_dihedrals": n_def, "n_undefined": n_undef, "frame_sums": sums}
        self.chains = list(names)
        self.data, self.frames = assemble(hist, n_def, n_undef, sums, names, edges, phi, step)

    def write_to_file(self, path_to_output):
        """writes ``.data`` to ``<path>.dihedral`` and ``.frames`` to ``<path>.dihedral_frames`` (feather)"""
        self.data.to_feather(_path.append_suffix(path_to_output, 'dihedral'))
        self.frames.to_feather(_path.append_suffix(path_to_output, 'dihedral_frames'))

    @classmethod
    def from_file(cls, path_to_file):
        """constructor from the files ``write_to_file`` wrote"""
        dh = cls()
        dh.data = pd.read_feather(_path.append_suffix(path_to_file, 'dihedral'))
        dh.frames = pd.read_feather(_path.append_suffix(path_to_file, 'dihedral_frames'))
        dh.chains = [c for c in dh.data.columns if c != "phi"]
        return dh
