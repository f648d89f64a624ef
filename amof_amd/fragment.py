"""Molecular building units of every frame and the reduced trajectory on MI355X.

``Fragments`` stands where the reference's "Identify building units" example drives ``amof/coordination/reduce.py``,
``amof/coordination/core.py`` and ``ReducedTrajectory`` (``amof/trajectory.py``): every frame is cut into the connected
components of a chosen bond graph -- the FRAGMENTS, e.g. 16 Zn and 32 imidazolates in ZIF-4 with ``{'C-N': 1.6, 'C-C': 1.6,
'C-H': 1.2}`` -- and every fragment is replaced by its centre of mass.  ``Rdf``, ``WindowMsd``, ``CoordinationNumber`` and
``Ring`` then run on ``.reduced()``.  The reference does this with pymatgen neighbour lists, networkx and MOF-specific
heuristics, one frame at a time; here the HIP kernels behind ``amof_fragment_stats`` (amof_amd/csrc/fragment.hip) label the
components under periodic boundaries, find the lattice image of every atom that makes its fragment whole, decide whether a
fragment winds around the cell and reduce per fragment.  Not restated: ``zif.py``'s chemistry (covalent-radius margins,
re-attached hydrogens, cycle detection), mfpx files, and the cutoffs ``reduce_structure`` infers for the reduced structure.

The bond graph is ``CoordinationNumber``'s / ``Ring``'s neighbour decision with sorted-pair cutoffs; species pairs missing from
the dictionary are never bonded.  The partition and the kinds of fragments of ``reference_frame`` are the yardstick: a frame is
``in_reduced_trajectory`` iff its partition into fragments equals that frame's and none of its fragments winds.
"""

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
from .frames import PackedTrajectory

logger = logging.getLogger(__name__)

FIRST_DUMMY = 87        # Fr, Ra, Ac, ...: the symbols of multi-atom kinds in the reduced trajectory, in kind order


def hill(counts, kinds):
    """Hill formula of a species-count vector over the atomic numbers ``kinds``: C, H, then the others alphabetically; all
    alphabetically without carbon"""
    have = {_data.chemical_symbols[z]: int(n) for z, n in zip(kinds, counts) if n}
    order = (["C"] + (["H"] if "H" in have else [])) if "C" in have else []
    order += sorted(s for s in have if s not in order)
    return "".join(s + (str(have[s]) if have[s] > 1 else "") for s in order)


def kinds_of(label, species, kinds):
    """``(table int32 [K][S], formulas, kind_of_root int [M])`` of a frame's labels: the distinct species-count vectors of its
    fragments sorted by Hill formula, and per fragment (roots ascending) the index of its vector"""
    label, species = np.asarray(label), np.asarray(species)
    S = len(kinds)
    roots, slot = np.unique(label, return_inverse=True)
    counts = np.zeros((len(roots), S), dtype=np.int64)
    np.add.at(counts, (slot, species), 1)
    distinct = sorted(set(tuple(int(x) for x in row) for row in counts), key=lambda c: hill(c, kinds))
    table = np.array(distinct, dtype=np.int32).reshape(len(distinct), S)
    return table, [hill(c, kinds) for c in distinct], np.array([distinct.index(tuple(int(x) for x in row)) for row in counts], dtype=np.int64)


def dummy_numbers(table, kinds):
    """atomic number of every kind in the reduced trajectory: a single-atom kind keeps its own, the multi-atom kinds take Fr,
    Ra, Ac, ... in kind order"""
    out, nxt = [], FIRST_DUMMY
    for row in np.asarray(table):
        if int(row.sum()) == 1:
            out.append(int(kinds[int(np.argmax(row))]))
        else:
            if nxt >= len(_data.chemical_symbols):
                raise ValueError("more multi-atom kinds of fragments than dummy symbols")
            out.append(nxt)
            nxt += 1
    return out


def assemble(summary, size_hist, census, links, formulas, step, n_atoms):
    """``(data, sizes, links, report_search)`` from the library's integers ``summary [F][5]``, ``size_hist [F][max_size + 2]``,
    ``census [F][K + 1]`` and ``links [F][K + 1][K + 1]`` (or None):
      data           Step, fragments, largest, winding, one column per formula, other
      sizes          Step, then the fragments of 0 .. max_size atoms ('0', '1', ...) and of more ('>max_size')
      links          Step, then 'A-B' for every ordered pair of kinds with a link bond in some frame: link bonds from fragments
                     of kind A to fragments of kind B divided by the number of fragments of kind A (NaN where there is none);
                     it counts BONDS, not distinct partner fragments.  None without links.
      report_search  indexed by Step: number_of_atoms, number_of_nodes, in_reduced_trajectory, atoms_regrouped"""
    summary = np.asarray(summary, dtype=np.int64)
    size_hist = np.asarray(size_hist, dtype=np.int64)
    census = np.asarray(census, dtype=np.int64)
    F, K = summary.shape[0], len(formulas)
    if summary.shape != (F, 5) or census.shape != (F, K + 1) or size_hist.ndim != 2 or size_hist.shape[0] != F:
        raise ValueError("summary must be [F][5], census [F][K + 1] and size_hist [F][max_size + 2]")
    if (census.sum(axis=1) != summary[:, 0]).any() or (size_hist.sum(axis=1) != summary[:, 0]).any():
        f = int(np.argwhere((census.sum(axis=1) != summary[:, 0]) | (size_hist.sum(axis=1) != summary[:, 0]))[0, 0])
        raise _hip.AmofError(_hip.AMOF_EHIP, "internal error: frame %d counts %d fragments, its census %d and its size histogram %d"
                             % (f, summary[f, 0], census[f].sum(), size_hist[f].sum()))
    step = np.asarray(step)[:F]
    names = list(formulas) + ["other"]
    data = pd.DataFrame(dict([("Step", step), ("fragments", summary[:, 0]), ("largest", summary[:, 1]), ("winding", summary[:, 2])]
                             + [(name, census[:, k]) for k, name in enumerate(names)]))
    max_size = size_hist.shape[1] - 2
    sizes = pd.DataFrame(dict([("Step", step)] + [(str(n), size_hist[:, n]) for n in range(max_size + 1)]
                              + [(">%d" % max_size, size_hist[:, max_size + 1])]))
    table = None
    if links is not None:
        links = np.asarray(links, dtype=np.int64)
        if links.shape != (F, K + 1, K + 1):
            raise ValueError("links must be [F][K + 1][K + 1]")
        cols = [("Step", step)]
        with np.errstate(divide="ignore", invalid="ignore"):
            for a in range(K + 1):
                for b in range(K + 1):
                    if links[:, a, b].any():
                        cols.append(("%s-%s" % (names[a], names[b]), np.where(census[:, a] > 0, links[:, a, b] / census[:, a], np.nan)))
        table = pd.DataFrame(dict(cols))
    regrouped = summary[:, 3]
    report = pd.DataFrame({"Step": step, "number_of_atoms": np.full(F, int(n_atoms)), "number_of_nodes": summary[:, 0],
                           "in_reduced_trajectory": (regrouped == 0) & (summary[:, 2] == 0), "atoms_regrouped": regrouped}).set_index("Step")
    return data, sizes, table, report


class Fragments(Deferred):
    """
    Building units (fragments) of every frame of a trajectory and the reduced trajectory of their centres of mass

    ``from_trajectory`` enqueues the analysis on its device's second lane and returns; every result waits for it
    (amof_amd/_lazy.py; ``AMOF_ASYNC=0``: synchronous).

      .data           per Step: fragments, largest (atoms), winding (fragments that wind around the cell), the number of
                      fragments of every kind found in the reference frame (one column per Hill formula), other
      .sizes          per Step: fragments by atom count
      .links          with ``links``: per Step and ordered pair of kinds 'A-B', link bonds from A to B per fragment of kind A
                      (ZIF-4 crystal: 'Zn-C3H3N2' 4.0, 'C3H3N2-Zn' 2.0); bonds, not distinct partner fragments
      .report_search  per Step: number_of_atoms, number_of_nodes, in_reduced_trajectory (the partition equals the reference
                      frame's and nothing winds), atoms_regrouped (atoms whose fragment root differs from the reference frame's)
      .counts         the library's integers: {'summary', 'size_hist', 'census', 'links'}
      .formulas       the kinds, Hill formulas sorted; .kinds int32 [K][S] their species counts
      .label, .shift  with ``per_atom``: int32 [F][N] the smallest atom of every atom's fragment, int32 [F][N][3] the lattice
                      image that makes the fragment whole
      .reduced()      the reduced trajectory
    A cutoff above half the smallest perpendicular cell height raises ValueError; more than 65535 atoms, an atom with more than
    16 neighbours or a shift beyond its storage raise AmofError naming the frame (nothing is truncated silently).
    """

    data = EmptyUntilComputed("Step")

    def __init__(self, max_size=None):
        """default constructor"""
        self.max_size = max_size

    @classmethod
    def from_trajectory(cls, trajectory, nb_set_and_cutoff, links=None, names=None, reference_frame=0, max_size=64, reduce=True,
                        delta_Step=1, first_frame=0, per_atom=False, device=None, distributed=None):
        """
        Args:
            trajectory: list of ase.Atoms-like frames, a PackedTrajectory or an XyzStream
            nb_set_and_cutoff: dict, the bonds that hold a fragment together, e.g. ``{'C-N': 1.6, 'C-C': 1.6, 'C-H': 1.2}``
                (symmetric, as the reference's ``format_cutoff(sort_pair=True)``)
            links: dict or None, the bonds BETWEEN fragments, e.g. ``{'Zn-N': 2.5}``; no pair of ``nb_set_and_cutoff``
            names: dict formula -> name of the kind in ``.reduced().symbols``, e.g. ``{'C3H3N2': 'Im'}``
            reference_frame: the frame whose partition and kinds the others are held against (a stream: in its first batch)
            max_size: the size histogram counts fragments of up to so many atoms one by one
            reduce: compute the centres of mass (``.reduced()``)
            per_atom: keep the label and the shift of every atom
            device: GPU index or list of indices (default: LOCAL_RANK or 0)
            distributed: None -> the ranks of an initialised torch.distributed group take contiguous shares of the frames;
                False -> single process
        """
        obj = cls(max_size=max_size)
        step = _trajectory.construct_step(delta_Step=delta_Step, first_frame=first_frame, number_of_frames=len(trajectory))
        obj.compute_fragments(trajectory, nb_set_and_cutoff, step, links=links, names=names, reference_frame=reference_frame,
                              reduce=reduce, per_atom=per_atom, device=device, distributed=distributed)
        return obj

    def compute_fragments(self, trajectory, nb_set_and_cutoff, step, links=None, names=None, reference_frame=0, reduce=True,
                          per_atom=False, device=None, distributed=None):
        max_size = int(self.max_size)
        if max_size != self.max_size or not 1 <= max_size <= 65535:
            raise ValueError("max_size must be an integer in 1 .. 65535")
        if not nb_set_and_cutoff:
            raise ValueError("nb_set_and_cutoff names no pair of neighbours")
        ref = int(reference_frame)
        if ref != reference_frame or not 0 <= ref < max(len(trajectory), 1):
            raise ValueError("reference_frame must be a frame of the trajectory")
        bonds = amatom.format_cutoff(nb_set_and_cutoff, sort_pair=True)
        between = amatom.format_cutoff(links, sort_pair=True) if links else None
        if between and set(between) & set(bonds):
            raise ValueError("links names a pair that nb_set_and_cutoff names: %s" % sorted(set(between) & set(bonds)))
        packed = _setup.pack(trajectory, device, keep_stream=True)
        F, N = len(packed), packed.n_atoms
        logger.info("Start fragment analysis for %s frames", F)
        kinds, species = _hip.packed_species(packed)
        rcm = amatom.cutoff_matrix(bonds, kinds)
        lm = amatom.cutoff_matrix(between, kinds) if between else None
        self.names = dict(names or {})
        self.reduce = bool(reduce)
        self.species_numbers = list(kinds)

        st = _setup.setup(packed, device, distributed, lane=1, keep_stream=True, honour_local=True)
        ctx, source, sharded = st.ctx, st.source, st.sharded
        frame_range = st.shard(F)
        n_rows = 3 + (lm is not None) + 2 * bool(per_atom) + bool(reduce)      # per-frame outputs (the masses are not)
        seen = {}

        def reference(tr, r):
            # the reference frame alone: every rank does this itself, so no collective is needed
            alone = ctx.fragment_stats(tr, rcm, max_size=max_size, frame_range=(r, r + 1), per_atom=True)
            label = alone[3][0]
            seen["label"], seen["winding"] = label, int(alone[0][0, 2])
            seen["table"], seen["formulas"], seen["kind_of_root"] = kinds_of(label, species, kinds)

        def call(tr, fr=None):
            return ctx.fragment_stats(tr, rcm, link=lm, ref_label=seen["label"], kinds=seen["table"], max_size=max_size, frame_range=fr,
                                      per_atom=per_atom, com=reduce)

        def finish_host(raw):
            self._assemble(raw, seen, lm is not None, per_atom, N, step)

        if _setup.streamed(st):
            def stream():
                out, cells = [], []
                for batch in source.batches():
                    if not seen:
                        if ref >= len(batch):
                            raise ValueError("reference_frame must lie in the first batch of a streamed trajectory")
                        reference(batch, ref)
                    out.append(call(batch))
                    cells.append(np.broadcast_to(batch.cell, (len(batch), 3, 3)) if batch.cell.shape[0] == 1 else batch.cell)
                seen["cell"], seen["pbc"] = np.concatenate(cells), batch.pbc
                return _hip.merge_results(out, ("cat",) * n_rows + (("first",) if reduce else ()))
            self._defer(ctx, stream, finish_host)
            return
        seen["cell"], seen["pbc"] = packed.cell, packed.pbc

        def local():
            # this rank's kernels (a lane job: amof_amd/_lazy.py)
            reference(packed, ref)
            return call(packed, frame_range)

        def finish(raw):
            if sharded:
                raw = tuple(_dist.all_gather_rows(x, device=ctx.device) for x in raw[:n_rows]) + tuple(raw[n_rows:])
            finish_host(raw)

        self._defer(ctx, local, finish, collective=sharded)

    def _assemble(self, raw, seen, has_links, per_atom, n_atoms, step):
        raw = list(raw)
        summary, hist, census = raw[:3]
        del raw[:3]
        links = raw.pop(0) if has_links else None
        if per_atom:
            self.label, self.shift = raw.pop(0), raw.pop(0)
        if self.reduce:
            self.com, self.frag_mass = raw.pop(0), raw.pop(0)
        self.counts = {"summary": np.asarray(summary), "size_hist": np.asarray(hist), "census": np.asarray(census), "links": links}
        self.formulas, self.kinds, self.kind_of_root = seen["formulas"], seen["table"], seen["kind_of_root"]
        self.ref_label, self.ref_winding = seen["label"], seen["winding"]
        self._cell, self._pbc = np.asarray(seen["cell"]), np.asarray(seen["pbc"])
        self.data, self.sizes, self.links, self.report_search = assemble(summary, hist, census, links, self.formulas, step, n_atoms)

    def reduced(self):
        """the reduced trajectory: a ``PackedTrajectory`` of the frames with ``in_reduced_trajectory``; positions are the
        centres of mass of the reference frame's fragments (roots ascending; not wrapped into the cell), masses their masses,
        cells those of the kept frames.  A single-atom kind keeps its atomic number, the multi-atom kinds are Fr, Ra, Ac, ... in
        kind order.  ``.symbols``: name of the kind (``names`` applied to the formulas) -> symbol; ``.steps``: the Steps kept.
        ValueError without ``reduce`` or when a fragment of the reference frame winds."""
        self._wait()
        if not self.reduce:
            raise ValueError("the centres of mass were not computed (reduce=False)")
        keep = self.report_search["in_reduced_trajectory"].to_numpy()
        if self.ref_winding:
            raise ValueError("a fragment of the reference frame winds around the cell: it has no centre of mass")
        numbers_of_kind = dummy_numbers(self.kinds, self.species_numbers)
        numbers = np.array([numbers_of_kind[k] for k in self.kind_of_root], dtype=np.int64)
        cell = self._cell if self._cell.shape[0] == 1 else self._cell[keep]
        out = PackedTrajectory(np.ascontiguousarray(self.com[keep]), cell, numbers, masses=self.frag_mass, pbc=tuple(self._pbc))
        out.symbols = {self.names.get(f, f): _data.chemical_symbols[z] for f, z in zip(self.formulas, numbers_of_kind)}
        out.steps = self.report_search.index.to_numpy()[keep]
        return out

    def write_to_file(self, filename):
        """writes ``.data`` to ``<filename>.fragments``, ``.sizes`` to ``<filename>.fragment_sizes``, ``.report_search`` to
        ``<filename>.fragment_report`` and, with links, ``.links`` to ``<filename>.fragment_links`` (feather)"""
        self.data.to_feather(_path.append_suffix(filename, 'fragments'))
        self.sizes.to_feather(_path.append_suffix(filename, 'fragment_sizes'))
        self.report_search.reset_index().to_feather(_path.append_suffix(filename, 'fragment_report'))
        if self.links is not None:
            self.links.to_feather(_path.append_suffix(filename, 'fragment_links'))

    @classmethod
    def from_file(cls, filename):
        """constructor of fragments class from the files ``write_to_file`` wrote"""
        obj = cls()
        obj.read_fragment_file(filename)
        return obj

    def read_fragment_file(self, filename):
        import os
        self.data = pd.read_feather(_path.append_suffix(filename, 'fragments'))
        self.sizes = pd.read_feather(_path.append_suffix(filename, 'fragment_sizes'))
        self.report_search = pd.read_feather(_path.append_suffix(filename, 'fragment_report')).set_index("Step")
        links = _path.append_suffix(filename, 'fragment_links')
        self.links = pd.read_feather(links) if os.path.exists(links) else None
