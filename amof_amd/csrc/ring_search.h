// Primitive-ring search on one frame's bond graph: the text that the GPU kernels (ring.hip: a lane per candidate on
// "ring_wave", a thread per source on "ring_simple") and the CPU driver (tests/native/ring_search_driver.cpp) all compile.
// Plain pointers, no HIP types.  Definition: DESIGN.md 4.3f, include/amof_hip.h (amof_ring_stats).
//
//   adj [N][RING_MAX_DEGREE] int32   neighbour rows, ascending in the atom index (unused entries are never read)
//   deg [N] int32                    0 .. RING_MAX_DEGREE
//   D   [N][N] u8                    graph distance truncated at K = nmax / 2: RING_FAR = farther than K
//   L   [N] u8                       the source's row of D (its BFS levels); the wave kernel keeps a copy in LDS
//
// A primitive ring of size n through the source v is a pair of shortest paths from v: to one antipode w at level k >= 2
// (n = 2k; the paths share v and w only) or to the two ends w1 < w2 of an edge inside level k >= 1 (n = 2k + 1; they share v
// only), such that every cross pair y = P1[a], z = P2[b] is at its ring distance: D[y][z] == min(a + b, n - a - b).  (Two
// nodes of one shortest path always are.)  A path is held by its nodes at levels 1 .. k, P[(level - 1) * stride] u16, so
// a path IS the state of its own enumeration: the next path is found by looking, level by level, for the next predecessor
// behind the current one in the (sorted) neighbour row.  Every loop is bounded: depth <= RING_MAX_K, rows <=
// RING_MAX_DEGREE, complete paths per end node <= the cap (checked before anything is enumerated).
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RING_HD __host__ __device__ __forceinline__
#else
#define RING_HD inline
#endif

#define RING_MAX_DEGREE 16
#define RING_MAX_PATHS 1024
#define RING_MIN_SIZE 3
#define RING_MAX_SIZE 32
#define RING_MAX_K (RING_MAX_SIZE / 2)
#define RING_MAX_ATOMS 65535
#define RING_FAR 255

namespace ring {

struct Graph {
    const int32_t *adj;
    const int32_t *deg;
    const uint8_t *D;
    int32_t N;
};

// a candidate: the end nodes of the two paths in one word (w1 == w2: an even ring's antipode)
RING_HD uint32_t pack_candidate(int w1, int w2) { return (uint32_t)w1 | ((uint32_t)w2 << 16); }

// the predecessor walk: the first neighbour u > after of a node at level lx with L[u] == lx - 1, or -1
RING_HD int next_pred(const int32_t *row, int deg, const uint8_t *L, int lx, int after)
{
    for (int q = 0; q < deg; q++) {
        const int u = row[q];
        if (u > after && (int)L[u] == lx - 1) return u;
    }
    return -1;
}

// The candidates that node x closes for the source whose levels are L:
//   even 2a:     x at level a >= 2 has at least two predecessors       (x was reached a second time)
//   odd 2a + 1:  an edge x < u inside level a >= 1; odd_candidate looks at entry q of x's row and returns u, or -1
RING_HD bool even_candidate(const Graph &g, const uint8_t *L, int x, int nmax)
{
    const int a = L[x];
    if (a < 2 || a == RING_FAR || 2 * a > nmax) return false;
    const int32_t *row = g.adj + (size_t)x * RING_MAX_DEGREE;
    const int deg = g.deg[x];
    const int first = next_pred(row, deg, L, a, -1);
    return first >= 0 && next_pred(row, deg, L, a, first) >= 0;
}

RING_HD int odd_candidate(const Graph &g, const uint8_t *L, int x, int nmax, int q)
{
    const int a = L[x];
    if (a == 0 || a == RING_FAR || 2 * a + 1 > nmax) return -1;
    const int u = g.adj[(size_t)x * RING_MAX_DEGREE + q];
    return u > x && (int)L[u] == a ? u : -1;
}

// number of shortest paths from the source to w (level k), counted up to cap + 1; P: scratch of k entries
RING_HD int count_paths(const Graph &g, const uint8_t *L, int w, int k, int cap, uint16_t *P, int st)
{
    if (k <= 1) return 1;
    int count = 0, j = k, after = -1;
    P[(k - 1) * st] = (uint16_t)w;
    for (;;) {
        const int x = P[(j - 1) * st];
        const int u = next_pred(g.adj + (size_t)x * RING_MAX_DEGREE, g.deg[x], L, j, after);
        if (u >= 0) {
            if (j == 2) {                   // u is at level 1: a complete path
                if (++count > cap) return count;
                after = u;
            } else {
                P[(j - 2) * st] = (uint16_t)u;
                j--;
                after = -1;
            }
        } else {
            if (j == k) return count;
            after = P[(j - 1) * st];
            j++;
        }
    }
}

// the per-level disjointness test: the two paths may not meet at level b
RING_HD bool disjoint_at(const uint16_t *P1, int st, int u, int b) { return (int)P1[(b - 1) * st] != u; }

// the cross-pair check of z = P2[b] against P1[1 .. ka]: all in row z of D
RING_HD bool cross_ok(const Graph &g, const uint16_t *P1, int st, int ka, int z, int b, int n)
{
    const uint8_t *Dz = g.D + (size_t)z * (size_t)g.N;
    for (int a = 1; a <= ka; a++) {
        const int rd = a + b < n - a - b ? a + b : n - a - b;
        if ((int)Dz[P1[(a - 1) * st]] != rd) return false;
    }
    return true;
}

// the second paths of a complete first path P1: number of primitive rings (P1, P2)
RING_HD int second_paths(const Graph &g, const uint8_t *L, int w2, int k, bool even, int n, const uint16_t *P1, uint16_t *P2, int st)
{
    const int ka = even ? k - 1 : k;
    if (!even && !cross_ok(g, P1, st, ka, w2, k, n)) return 0;
    if (k == 1) return 1;                   // (a triangle)
    int rings = 0, j = k;
    int after = even ? (int)P1[(k - 2) * st] : -1;     // unordered pairs: P2[k - 1] > P1[k - 1] (they differ there)
    P2[(k - 1) * st] = (uint16_t)w2;
    for (;;) {
        const int x = P2[(j - 1) * st];
        const int u = next_pred(g.adj + (size_t)x * RING_MAX_DEGREE, g.deg[x], L, j, after);
        if (u >= 0) {
            after = u;
            if (!disjoint_at(P1, st, u, j - 1) || !cross_ok(g, P1, st, ka, u, j - 1, n)) continue;
            if (j == 2) {
                rings++;
            } else {
                P2[(j - 2) * st] = (uint16_t)u;
                j--;
                after = -1;
            }
        } else {
            if (j == k) return rings;
            after = P2[(j - 1) * st];
            j++;
        }
    }
}

// One candidate of a source: the number of primitive rings it closes (of size *size), or -1 where an end node has more than
// cap shortest paths (the caller refuses the call).  P1, P2: RING_MAX_K entries each, strided.
RING_HD int search_candidate(const Graph &g, const uint8_t *L, uint32_t cand, int cap, uint16_t *P1, uint16_t *P2, int st, int *size)
{
    const int w1 = (int)(cand & 0xffffu), w2 = (int)(cand >> 16);
    const bool even = w1 == w2;
    const int k = L[w1];
    const int n = 2 * k + (even ? 0 : 1);
    *size = n;
    if (count_paths(g, L, w1, k, cap, P1, st) > cap) return -1;
    if (!even && count_paths(g, L, w2, k, cap, P2, st) > cap) return -1;
    P1[(k - 1) * st] = (uint16_t)w1;
    if (k == 1) return second_paths(g, L, w2, k, even, n, P1, P2, st);
    int rings = 0, j = k, after = -1;
    for (;;) {
        const int x = P1[(j - 1) * st];
        const int u = next_pred(g.adj + (size_t)x * RING_MAX_DEGREE, g.deg[x], L, j, after);
        if (u >= 0) {
            P1[(j - 2) * st] = (uint16_t)u;
            if (j == 2) {
                rings += second_paths(g, L, w2, k, even, n, P1, P2, st);
                after = u;
            } else {
                j--;
                after = -1;
            }
        } else {
            if (j == k) return rings;
            after = P1[(j - 1) * st];
            j++;
        }
    }
}

// Everything of one source v: c[n] += the primitive n-rings through v (c: nmax + 1 counters, zeroed by the caller).  Returns 0,
// or -1 for the path cap.  stats (optional): [0] += candidates, [1] += candidates that close at least one ring.
RING_HD int search_source(const Graph &g, int v, int nmax, int cap, uint16_t *P1, uint16_t *P2, int st, uint32_t *c, unsigned long long *stats)
{
    const uint8_t *L = g.D + (size_t)v * (size_t)g.N;
    int rc = 0;
    for (int x = 0; x < g.N; x++) {
        const int deg = g.deg[x];
        for (int q = -1; q < deg; q++) {            // q = -1: the even candidate
            int u = x;
            if (q < 0) {
                if (!even_candidate(g, L, x, nmax)) continue;
            } else if ((u = odd_candidate(g, L, x, nmax, q)) < 0) {
                continue;
            }
            int n = 0;
            const int r = search_candidate(g, L, pack_candidate(x, u), cap, P1, P2, st, &n);
            if (r < 0) rc = -1;
            else if (r > 0) c[n] += (uint32_t)r;
            if (stats) {
                stats[0]++;
                if (r > 0) stats[1]++;
            }
        }
    }
    return rc;
}

}  // namespace ring
