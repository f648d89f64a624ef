"""Primitive ring statistics of bond networks on MI355X.

``Ring`` mirrors ``amof.ring.Ring`` (amof/ring/core.py), which writes every frame to a temporary directory, runs the
external Fortran program RINGS on it -- up to five times per frame, with search depths 16, 20, ... -- and reads the
counts of primitive rings back.  Here the bond graph of a frame (``CoordinationNumber``'s neighbour decision with the
reference's sorted-pair cutoffs; species pairs missing from the dictionary are never bonded) is searched by the HIP kernels
behind ``amof_ring_stats`` (amof_amd/csrc/ring.hip): a breadth-first search from every atom truncated at depth
``max_search_depth // 2``, then every pair of shortest paths that closes a primitive ring (Franzblau's shortest-path ring: a
simple cycle on which every pair of nodes is as far apart as in the graph).  One pass at ``max_search_depth`` replaces the
reference's reruns: the counts at a size do not depend on the depth once it covers that size.

The graph is the QUOTIENT graph of the periodic cell: a closed path that winds around a small cell is a ring of it, as it is
for RINGS on a periodic box; winding is not detected.

The library returns integers (include/amof_hip.h); ``assemble`` keeps the divisions.  The derived quantities follow RINGS'
definitions [3P-memory]: with N atoms and, per ring size n, rings(n) primitive rings, nodes(n) atoms on at least one of them,
nodes_min(n) / nodes_max(n) atoms whose smallest / largest ring has n nodes,
    Rc(n) = rings(n) / N      Pn(n) = nodes(n) / N      Pmin(n) = nodes_min(n) / nodes(n)      Pmax(n) = nodes_max(n) / nodes(n)
"""

import logging

import numpy as np
import pandas as pd

from ._lazy import Deferred, EmptyUntilComputed

from . import _hip
from . import _setup
from . import atom as amatom
from . import dist as _dist
from . import trajectory as _trajectory
from .files import path as _path

logger = logging.getLogger(__name__)

MIN_DEPTH, MAX_DEPTH = 3, 32
RING_VARS = ("rings", "Rc(n)", "Pn(n)", "Pmax(n)", "Pmin(n)")
UNDISCOVERED = "Rings statistics computed with potentially undiscovered rings"


def check_depth(max_search_depth):
    nmax = int(max_search_depth)
    if nmax != max_search_depth or not MIN_DEPTH <= nmax <= MAX_DEPTH:
        raise ValueError("max_search_depth must be an integer in %d .. %d" % (MIN_DEPTH, MAX_DEPTH))
    return nmax


def assemble(counts, truncated, n_atoms, step, nmax):
    """``(table, mean, report_search)`` from the library's integers ``counts [F][4][nmax + 1]`` and ``truncated [F]``:
      table          long: Step, ring_size 3 .. nmax, rings, Rc(n), Pn(n), Pmax(n), Pmin(n) (NaN where no atom is on an n-ring)
      mean           the trajectory averages per ring size (NaN entries skipped), indexed by ring_size
      report_search  indexed by Step: max_search_depth, Truncated sources, and whether larger rings cannot be excluded
    A sum over the atoms of the n-rings through them that n does not divide raises AmofError: never rounded."""
    counts = np.asarray(counts, dtype=np.int64)
    truncated = np.asarray(truncated, dtype=np.int64).reshape(-1)
    F = counts.shape[0]
    if counts.shape != (F, 4, nmax + 1) or truncated.shape != (F,):
        raise ValueError("counts must be [F][4][nmax + 1] and truncated [F]")
    step = np.asarray(step)[:F]
    sizes = np.arange(MIN_DEPTH, nmax + 1)
    total = counts[:, 0, MIN_DEPTH:]
    if (total % sizes[None, :]).any():
        f, k = np.argwhere(total % sizes[None, :])[0]
        raise _hip.AmofError(_hip.AMOF_EHIP, "internal error: frame %d counts %d ring memberships of size %d, not a multiple of it"
                             % (f, total[f, k], sizes[k]))
    rings = total // sizes[None, :]
    nodes = counts[:, 1, MIN_DEPTH:].astype(np.float64)
    N = float(n_atoms)
    with np.errstate(divide="ignore", invalid="ignore"):
        rc = rings / N if n_atoms else np.full(rings.shape, np.nan)
        pn = nodes / N if n_atoms else np.full(rings.shape, np.nan)
        pmin = np.where(nodes > 0, counts[:, 2, MIN_DEPTH:] / nodes, np.nan)
        pmax = np.where(nodes > 0, counts[:, 3, MIN_DEPTH:] / nodes, np.nan)
    table = pd.DataFrame({"Step": np.repeat(step, len(sizes)), "ring_size": np.tile(sizes, F), "rings": rings.reshape(-1),
                          "Rc(n)": rc.reshape(-1), "Pn(n)": pn.reshape(-1), "Pmax(n)": pmax.reshape(-1), "Pmin(n)": pmin.reshape(-1)})
    mean = table.drop(columns="Step").groupby("ring_size").mean()
    report = pd.DataFrame({"Step": step, "max_search_depth": np.full(F, nmax), "Truncated sources": truncated,
                           UNDISCOVERED: truncated > 0}).set_index("Step")
    return table, mean, report


class Ring(Deferred):
    """
    Primitive ring statistics of the bond network of every frame of a trajectory

    Search for primitive rings as defined by Le Roux & Jund, Comput. Mater. Sci. 49, 70 (2010), i.e. Franzblau's
    shortest-path rings (Phys. Rev. B 44, 4925 (1991)): a ring that contains a shortest path of the graph for each pair of
    its nodes.  The graph is the quotient graph of the cell: a path that winds around a small cell closes a ring.

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; every result waits for it
    (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

      .table          long DataFrame: Step, ring_size, rings, Rc(n), Pn(n), Pmax(n), Pmin(n) (``assemble``; [3P-memory])
      .mean           the trajectory averages per ring size
      .report_search  per Step: max_search_depth, Truncated sources (atoms whose search met unvisited neighbours at depth
                      max_search_depth // 2) and 'Rings statistics computed with potentially undiscovered rings'
      .counts         int64 [F][4][max_search_depth + 1], .truncated int64 [F]: the library's integers
      .per_atom       on request, u32 [F][N][max_search_depth + 1]: the n-rings through every atom
      .data           the reference's ``xarray.Dataset({'ring': ...})``, dims (Step, ring_size, ring_var), when xarray is
                      importable, else None
    A cutoff above half the smallest perpendicular cell height raises ValueError; more than 65535 atoms, an atom with more
    than 16 neighbours or more than 1024 shortest paths to one node raise AmofError (nothing is truncated silently).
    """

    table = EmptyUntilComputed("Step")

    def __init__(self, max_search_depth=None):
        """default constructor"""
        self.max_search_depth = max_search_depth

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, max_search_depth=32, delta_Step=1, first_frame=0, parallel=False,
                        per_atom=False, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, a PackedTrajectory or an XyzStream
            nb_set_and_cutoff: dict, keys are str indicating pair of neighbours, values are cutoffs float, in Angstrom
                (symmetric: 'Zn-N' bonds N to Zn as well, as the reference's ``format_cutoff(sort_pair=True)``)
            max_search_depth: int in 3 .. 32, largest ring size searched for
            parallel: accepted for the reference's signature and ignored
            per_atom: keep the ring counts of every atom
            device: GPU index or list of indices (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group take contiguous shares of the frames;
                False -> single process
        """
        ring_class = cls(max_search_depth=max_search_depth)
        step = _trajectory.construct_step(delta_Step=delta_Step, first_frame=first_frame, number_of_frames=len(trajectory))
        ring_class.compute_ring(trajectory, nb_set_and_cutoff, step, per_atom=per_atom, device=device, distributed=distributed)
        return ring_class

    def compute_ring(self, trajectory, nb_set_and_cutoff, step, per_atom=False, device=None, distributed=None):
        nmax = check_depth(self.max_search_depth)
        if not nb_set_and_cutoff:
            raise ValueError("nb_set_and_cutoff names no pair of neighbours")
        packed = _setup.pack(trajectory, device, keep_stream=True)
        logger.info("Start ring analysis for %s frames", len(packed))
        kinds, _ = _hip.packed_species(packed)
        rcm = amatom.cutoff_matrix(amatom.format_cutoff(nb_set_and_cutoff, sort_pair=True), kinds)

        st = _setup.setup(packed, device, distributed, lane=1, keep_stream=True, honour_local=True)
        ctx, source, sharded = st.ctx, st.source, st.sharded
        F, N = len(packed), packed.n_atoms
        frame_range = st.shard(F)
        rules = ("cat",) * (2 + bool(per_atom))

        def finish_host(raw):
            self._assemble(raw[0], raw[1], raw[2] if per_atom else None, N, step, nmax)

        if _setup.streamed(st):
            self._defer(ctx, lambda: _setup.walk(source, lambda batch: ctx.ring_stats(batch, rcm, nmax, per_atom=per_atom), rules),
                        finish_host)
            return

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            return ctx.ring_stats(packed, rcm, nmax, frame_range=frame_range, per_atom=per_atom)

        def finish(raw):
            if sharded:
                raw = tuple(_dist.all_gather_rows(x, device=ctx.device) for x in raw)
            finish_host(raw)

        self._defer(ctx, local, finish, collective=sharded)

    def _assemble(self, counts, truncated, per_atom, n_atoms, step, nmax):
        self.counts = np.asarray(counts)
        self.truncated = np.asarray(truncated)
        if per_atom is not None:
            self.per_atom = per_atom
        self.table, self.mean, self.report_search = assemble(counts, truncated, n_atoms, step, nmax)
        try:
            import xarray as xr
        except ImportError:
            self.data = None
            return
        F = self.counts.shape[0]
        values = self.table[list(RING_VARS)].to_numpy(dtype=np.float64).reshape(F, nmax + 1 - MIN_DEPTH, len(RING_VARS))
        xa = xr.DataArray(values, coords={"Step": np.asarray(step)[:F], "ring_size": np.arange(MIN_DEPTH, nmax + 1),
                                          "ring_var": np.array(RING_VARS)}, dims=("Step", "ring_size", "ring_var"))
        self.data = xr.Dataset({'ring': xa})

    def write_to_file(self, filename):
        """writes ``.data`` to ``<filename>.ring`` (netCDF) and ``.report_search`` to ``<filename>.report_search.csv``, as
        the reference"""
        if self.data is None:
            raise ImportError("xarray (netCDF) is needed to write a Ring file, as in the reference")
        self.data.to_netcdf(_path.append_suffix(filename, 'ring'))
        self.report_search.to_csv(_path.append_suffix(filename, 'report_search.csv'))

    @classmethod
    def from_file(cls, filename):
        """constructor of ring class from ring file"""
        ring_class = cls()
        ring_class.read_ring_file(filename)
        return ring_class

    def read_ring_file(self, filename):
        import xarray as xr
        self.data = xr.open_dataset(_path.append_suffix(filename, 'ring'))
