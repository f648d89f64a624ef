"""Primitive rings of a bond graph, twice and independently of the library (amof_amd/csrc/ring_search.h):

  brute(adj, nmax)    every simple cycle of up to nmax nodes, kept iff every pair of its nodes is as far apart in the graph (full
                      breadth-first distances) as on the cycle -- Franzblau's shortest-path ring, with no antipode argument
  search(adj, nmax)   the definition of DESIGN.md 4.3f restated: distances truncated at K = nmax // 2, all shortest paths to an
                      antipode (or to the two ends of an in-level edge) listed, every pair of them tested -- for the depths the
                      brute force cannot reach

and the float64 numpy bond decision (``adjacency``), which asserts that no pair lies within 1e-6 A of its cutoff: whatever
arithmetic decides the bonds then decides the same."""

import itertools

import numpy as np

from amof_amd import atom as amatom

FAR = 255


def adjacency(pos, cell, numbers, cutoff, pbc=(True, True, True), margin=1e-6):
    """neighbour lists (ascending) of one frame: i ~ j iff |minimum image of r_j - r_i| < rc of the species pair; pairs missing
    from the dictionary are never bonded"""
    pos = np.asarray(pos, dtype=np.float64)
    cell = np.asarray(cell, dtype=np.float64).reshape(3, 3)
    kinds = sorted(set(int(z) for z in numbers))
    rcm = amatom.cutoff_matrix(amatom.format_cutoff(cutoff), kinds)
    sp = np.array([kinds.index(int(z)) for z in numbers])
    d = pos[None, :, :] - pos[:, None, :]
    s = d @ np.linalg.inv(cell)
    s -= np.rint(s) * np.asarray(pbc, dtype=np.float64)
    r = np.sqrt(((s @ cell) ** 2).sum(axis=2))
    rc = rcm[sp[:, None], sp[None, :]]
    off = ~np.eye(len(pos), dtype=bool)
    assert not (off & (rc > 0) & (np.abs(r - rc) < margin)).any(), "a pair within %g of its cutoff" % margin
    bonded = off & (r < rc)
    assert np.array_equal(bonded, bonded.T)
    return [np.nonzero(row)[0].tolist() for row in bonded]


def distances(adj, limit=None):
    """all-pairs breadth-first distances int [N][N]; beyond ``limit`` (and unreachable): FAR"""
    N = len(adj)
    D = np.full((N, N), FAR, dtype=np.int64)
    for v in range(N):
        D[v, v] = 0
        frontier, level = [v], 0
        while frontier and (limit is None or level < limit):
            level += 1
            nxt = []
            for x in frontier:
                for u in adj[x]:
                    if D[v, u] == FAR:
                        D[v, u] = level
                        nxt.append(u)
            frontier = nxt
        assert level < FAR
    return D


def brute(adj, nmax):
    """c [N][nmax + 1]: c[v][n] = primitive n-rings through v, by enumeration of every simple cycle"""
    N = len(adj)
    D = distances(adj)
    c = np.zeros((N, nmax + 1), dtype=np.int64)
    nbr = [set(a) for a in adj]

    def close(path):
        n = len(path)
        for i in range(n):
            for j in range(i + 1, n):
                if D[path[i], path[j]] != min(j - i, n - (j - i)):
                    return
        for x in path:
            c[x, n] += 1

    for s in range(N):
        # cycles whose smallest node is s, each in one direction (second node < last node)
        path, on = [s], {s}

        def extend():
            u = path[-1]
            for w in adj[u]:
                if w <= s or w in on:
                    continue
                if len(path) + D[w, s] > nmax:        # cannot close within nmax nodes any more (a bound, not the ring test)
                    continue
                path.append(w)
                on.add(w)
                if len(path) >= 3 and s in nbr[w] and path[1] < w:
                    close(path)
                if len(path) < nmax:
                    extend()
                on.discard(path.pop())
        extend()
    return c


def _paths(adj, L, w):
    """every shortest path from the source to w, as the tuple of its nodes at levels 1 .. L[w]"""
    k = L[w]
    if k == 1:
        return [(w,)]
    out = []
    for u in adj[w]:
        if L[u] == k - 1:
            out.extend(p + (w,) for p in _paths(adj, L, u))
    return out


def search(adj, nmax):
    """``(c [N][nmax + 1], truncated, most shortest paths to one end node)`` by the definition's search"""
    N, K = len(adj), nmax // 2
    D = distances(adj, K)
    c = np.zeros((N, nmax + 1), dtype=np.int64)
    truncated, most = 0, 0

    def primitive(P1, P2, n, ka):
        for a in range(1, ka + 1):
            for b in range(1, ka + 1):
                if D[P1[a - 1], P2[b - 1]] != min(a + b, n - a - b):
                    return False
        return True

    for v in range(N):
        L = D[v]
        if any(L[x] == K and any(L[u] == FAR for u in adj[x]) for x in range(N)):
            truncated += 1
        for w in range(N):
            k = L[w]
            if k == 0 or k == FAR:
                continue
            if k >= 2 and 2 * k <= nmax:
                paths = _paths(adj, L, w)
                most = max(most, len(paths))
                for P1, P2 in itertools.combinations(paths, 2):
                    if primitive(P1, P2, 2 * k, k - 1):          # (two paths that meet below w are no pair: D == 0 there)
                        c[v, 2 * k] += 1
            if 2 * k + 1 <= nmax:
                for w2 in adj[w]:
                    if w2 > w and L[w2] == k:
                        first, second = _paths(adj, L, w), _paths(adj, L, w2)
                        most = max(most, len(first), len(second))
                        for P1 in first:
                            for P2 in second:
                                if primitive(P1, P2, 2 * k + 1, k):
                                    c[v, 2 * k + 1] += 1
    return c, truncated, most


def rings(c):
    """{n: number of n-rings} from c[v][n]; the division by n must be exact"""
    total = np.asarray(c).sum(axis=0)
    out = {}
    for n, t in enumerate(total):
        assert t % max(n, 1) == 0, (n, t)
        if t:
            out[n] = int(t) // n
    return out


def counts(c):
    """the library's per-frame integers [4][nmax + 1] from c[v][n] (include/amof_hip.h, amof_ring_stats)"""
    c = np.asarray(c, dtype=np.int64)
    nmax = c.shape[1] - 1
    out = np.zeros((4, nmax + 1), dtype=np.int64)
    out[0] = c.sum(axis=0)
    out[1] = (c > 0).sum(axis=0)
    for row in c:
        sizes = np.nonzero(row)[0]
        if len(sizes):
            out[2, sizes[0]] += 1
            out[3, sizes[-1]] += 1
    return out


def tables(adj, K):
    """(adj int32 [N][16] padded with -1, deg int32 [N], D u8 [N][N] truncated at K): what the native driver reads"""
    N = len(adj)
    rows = np.full((N, 16), -1, dtype=np.int32)
    deg = np.zeros(N, dtype=np.int32)
    for i, a in enumerate(adj):
        assert len(a) <= 16 and list(a) == sorted(a)
        rows[i, :len(a)] = a
        deg[i] = len(a)
    return rows, deg, distances(adj, K).astype(np.uint8)
