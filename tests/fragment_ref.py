"""Fragments of a bond graph under periodic boundaries, independently of the library (amof_amd/csrc/fragment_math.h): breadth-first
components of ``ring_ref.adjacency``'s float64 graph, shifts along the search tree, winding by the bond relation, float64 centres of
mass, census, link counts and size histogram from the definitions of include/amof_hip.h (amof_fragment_stats).  Pure numpy."""

import collections

import numpy as np

from amof_amd import data as _data
from tests import ring_ref

Frame = collections.namedtuple("Frame", "label shift winds adj images")


def image(pos, inv, pbc, i, j):
    """n_ij: the lattice vector the minimum image subtracts for r_j - r_i (int [3])"""
    s = (pos[j] - pos[i]) @ inv
    assert np.all(np.abs(s - np.rint(s)) < 0.499), "a bonded pair at half a cell"
    return (np.rint(s) * pbc).astype(np.int64)


def frame(pos, cell, numbers, cutoff, pbc=(True, True, True)):
    """``Frame`` of one frame: label [N] (the smallest atom of the fragment), shift int [N][3] along the breadth-first tree from
    the root (shift[j] = shift[i] - n_ij), winds {root: bool} (a bond violates the relation), the graph and its images"""
    pos = np.asarray(pos, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    pbc = np.asarray(pbc, dtype=np.float64)
    adj = ring_ref.adjacency(pos, cell, numbers, cutoff, tuple(bool(x) for x in pbc))
    inv = np.linalg.inv(cell)
    N = len(adj)
    images = {(i, j): image(pos, inv, pbc, i, j) for i in range(N) for j in adj[i]}
    label = np.full(N, -1, dtype=np.int64)
    shift = np.zeros((N, 3), dtype=np.int64)
    for root in range(N):
        if label[root] >= 0:
            continue
        label[root] = root
        queue = collections.deque([root])
        while queue:
            i = queue.popleft()
            for j in adj[i]:
                if label[j] < 0:
                    label[j] = root
                    shift[j] = shift[i] - images[(i, j)]
                    queue.append(j)
    winds = {int(r): False for r in np.unique(label)}
    for (i, j), n in images.items():
        if not np.array_equal(shift[j], shift[i] - n):
            winds[int(label[i])] = True
    return Frame(label, shift, winds, adj, images)


def centres(pos, cell, masses, fr, roots=None):
    """float64 centres of mass [M][3] of the fragments rooted at ``roots`` (default: all, ascending), atoms made whole; NaN rows
    for the winding ones"""
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    roots = sorted(fr.winds) if roots is None else list(roots)
    out = np.full((len(roots), 3), np.nan)
    whole = np.asarray(pos, dtype=np.float64) + fr.shift @ cell
    for k, r in enumerate(roots):
        if fr.winds[r]:
            continue
        sel = fr.label == r
        out[k] = (masses[sel, None] * whole[sel]).sum(axis=0) / masses[sel].sum()
    return out


def species_counts(fr, numbers):
    """{root: tuple of counts per species (sorted atomic numbers)}"""
    kinds = sorted(set(int(z) for z in numbers))
    out = {}
    for r in sorted(fr.winds):
        z = np.asarray(numbers)[fr.label == r]
        out[r] = tuple(int((z == k).sum()) for k in kinds)
    return out


def hill(counts, kinds):
    """Hill formula of a species-count vector: C, H, then the others alphabetically; all alphabetically without carbon"""
    have = {_data.chemical_symbols[z]: n for z, n in zip(kinds, counts) if n}
    order = (["C"] + (["H"] if "H" in have else []) if "C" in have else [])
    order += sorted(s for s in have if s not in order)
    return "".join(s + (str(have[s]) if have[s] > 1 else "") for s in order)


def stats(fr, numbers, kinds_table, max_size, ref_label=None, link_adj=None):
    """the library's per-frame integers: (summary [5], size_hist [max_size + 2], census [K + 1], links [K + 1][K + 1] or None)"""
    K = len(kinds_table)
    table = [tuple(int(x) for x in row) for row in kinds_table]
    counts = species_counts(fr, numbers)
    kind_of = {r: (table.index(c) if c in table else K) for r, c in counts.items()}
    sizes = {r: int((fr.label == r).sum()) for r in counts}
    hist = np.zeros(max_size + 2, dtype=np.int64)
    census = np.zeros(K + 1, dtype=np.int64)
    for r in counts:
        hist[min(sizes[r], max_size + 1)] += 1
        census[kind_of[r]] += 1
    inside, links = 0, None
    if link_adj is not None:
        links = np.zeros((K + 1, K + 1), dtype=np.int64)
        for i, row in enumerate(link_adj):
            for j in row:
                if fr.label[i] == fr.label[j]:
                    inside += i < j
                else:
                    links[kind_of[int(fr.label[i])], kind_of[int(fr.label[j])]] += 1
    regrouped = -1 if ref_label is None else int((fr.label != np.asarray(ref_label)).sum())
    summary = np.array([len(counts), max(sizes.values()) if sizes else 0, sum(fr.winds.values()), regrouped, inside], dtype=np.int64)
    return summary, hist, census, links


def kinds_of(fr, numbers):
    """the distinct species-count vectors of a frame's fragments, sorted by Hill formula: (table int [K][S], formulas)"""
    kinds = sorted(set(int(z) for z in numbers))
    distinct = sorted(set(species_counts(fr, numbers).values()), key=lambda c: hill(c, kinds))
    return np.array(distinct, dtype=np.int32).reshape(len(distinct), len(kinds)), [hill(c, kinds) for c in distinct]


def tables(fr):
    """(adj int32 [N][16] padded with -1, deg int32 [N]): what the native driver reads"""
    rows, deg, _ = ring_ref.tables(fr.adj, 0)
    return rows, deg
