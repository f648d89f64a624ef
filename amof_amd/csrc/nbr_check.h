// The argument rules of the neighbour and bond family (amof_cn_count, amof_bad_hist[_dev|_by_cn], amof_bond_order[_dev],
// amof_dihedral_hist[_dev], amof_ring_stats, amof_fragment_stats, the bond lifetime and reorientation entry points), each once,
// host-only C++17 without HIP or amof_ctx (tests/native/nbr_check_driver.cpp asks them directly).  A rule returns the AMOF_E*
// code and the message (pore_check.h's Verdict); the .hip files pass both on to fail() (pore_refuse, amof_internal.h) and decide
// none of this themselves.  Two more host decisions stand here for the same reason: min_periodic_height and uniform_edge_step.
// The order of the checks per entry point (the first refusal wins; F = n_frames, N = n_atoms; NULL arguments stay with the callers):
//   amof_cn_count           validate_traj . NULL . sets_in_range . [n_sets == 0 or F == 0: done] . nbr_setup's
//   nbr_setup (all of nbr.hip, order.hip, dihedral.hip)   values_not_negative("cutoff") . symmetric
//   amof_bad_hist[_dev]     validate_traj . NULL . bad_bins . edges_increase . triples_in_range . [T == 0: done] . nbr_setup's
//   amof_bad_hist_by_cn     amof_bad_hist's . cn_max_range . nbr_setup's
//   amof_bond_order[_dev]   validate_traj . NULL . order_l_count . order_l . order_bins . NULL (outputs) . sets_in_range .
//                           values_not_negative("cutoff") . [n_sets == 0 or F == 0: done] . build_geometry .
//                           half_height_set(.., "a neighbour could be counted twice") per set . nbr_setup's
//   amof_dihedral_hist[_dev] validate_traj . NULL . chain_count . hist_bins . edges_increase . chains_in_range .
//                           bond_matrix("cutoff") . [F == 0 or N == 0: done] . build_geometry . half_height per matrix entry . nbr_setup's
//   amof_ring_stats         validate_traj . max_size . NULL . bond_matrix("cutoff") . atoms cap . [F == 0 or N == 0: done] .
//                           build_geometry . half_height per matrix entry
//   amof_fragment_stats     its own . bond_matrix("cutoff") . bond_matrix("link") . ... . build_geometry .
//                           half_height per entry of max(cutoff, link)
//   bond_run (bond.hip)     validate_traj . NULL . lags . atom range . frames . per set: bond_set_species, bond_set_cutoff . ... .
//                           build_geometry . half_height_set(.., "a pair could be bonded twice") per set
#pragma once
#include <math.h>
#include <stdint.h>

#include "pore_check.h"

namespace amof {
namespace nbr_check {
using pore_check::refuse_if;
using pore_check::Verdict;

// ---- species named by a call: sets [n][2] of species, triples [T][2] and chains [T][4] of species or -1 (any) ----
inline Verdict sets_in_range(const int32_t *sets, int32_t n_sets, int S)
{
    for (int s = 0; s < n_sets; s++)
        if (sets[2 * s] < 0 || sets[2 * s] >= S || sets[2 * s + 1] < 0 || sets[2 * s + 1] >= S)
            return refuse_if(true, AMOF_EINVAL, "set %d names a species out of range", s);
    return Verdict();
}
inline Verdict patterns_in_range(const int32_t *p, int32_t n, int width, int S, const char *what)
{
    for (int k = 0; k < width * n; k++)
        if (p[k] < -1 || p[k] >= S) return refuse_if(true, AMOF_EINVAL, "%s %d names a species out of range", what, k / width);
    return Verdict();
}
inline Verdict triples_in_range(const int32_t *triples, int32_t T, int S) { return patterns_in_range(triples, T, 2, S, "triple"); }
inline Verdict chains_in_range(const int32_t *chains, int32_t T, int S) { return patterns_in_range(chains, T, 4, S, "chain"); }
// the bond dynamics check a set's species and its cutoff together, set by set
inline Verdict bond_set_species(const int32_t *sets, int s, int S)
{
    return refuse_if(sets[2 * s] < 0 || sets[2 * s] >= S || sets[2 * s + 1] < 0 || sets[2 * s + 1] >= S, AMOF_EINVAL,
                     "set %d names a species outside 0..%d", s, S - 1);
}
inline Verdict bond_set_cutoff(double rc, int s) { return refuse_if(!(rc >= 0.0) || !isfinite(rc), AMOF_EINVAL, "cutoff of set %d must be finite and not negative", s); }

// ---- cutoffs [S][S]: finite and >= 0, symmetric.  what: "cutoff" or "link" ----
inline Verdict values_not_negative(const double *m, int n, const char *what)
{
    for (int k = 0; k < n; k++)
        if (!(m[k] >= 0.0) || !isfinite(m[k])) return refuse_if(true, AMOF_EINVAL, "%s must be finite and >= 0", what);
    return Verdict();
}
inline Verdict symmetric(const double *m, int S)        // (nbr_setup's, after values_not_negative over the whole matrix)
{
    for (int x = 0; x < S; x++)
        for (int y = 0; y < S; y++)
            if (m[x * S + y] != m[y * S + x]) return refuse_if(true, AMOF_EINVAL, "cutoff matrix must be symmetric");
    return Verdict();
}
// both rules entry by entry, row-major: the first offending entry decides which text the caller sees
inline Verdict bond_matrix(const double *m, int S, const char *what)
{
    for (int x = 0; x < S; x++)
        for (int y = 0; y < S; y++) {
            const double rc = m[x * S + y];
            if (!(rc >= 0.0) || !isfinite(rc)) return refuse_if(true, AMOF_EINVAL, "%s must be finite and >= 0", what);
            if (rc != m[y * S + x]) return refuse_if(true, AMOF_EINVAL, "the %s matrix must be symmetric", what);
        }
    return Verdict();
}

// ---- histograms: bin counts and edges [nb + 1] ----
inline Verdict bad_bins(int32_t nb) { return refuse_if(nb <= 0, AMOF_EINVAL, "nb must be positive"); }
inline Verdict hist_bins(int32_t nb) { return refuse_if(nb <= 0 || nb > (1 << 24), AMOF_EINVAL, "nb must be 1..2^24"); }
inline Verdict edges_increase(const double *edges, int32_t nb)
{
    for (int k = 0; k < nb; k++)
        if (!(edges[k + 1] > edges[k])) return refuse_if(true, AMOF_EINVAL, "edges must increase strictly");
    return Verdict();
}
inline Verdict order_bins(int32_t nbins, int32_t nbins_tet)
{
    return refuse_if(nbins < 1 || nbins > (1 << 24) || nbins_tet < 1 || nbins_tet > (1 << 24), AMOF_EINVAL, "nbins, nbins_tet must be 1..2^24");
}

// ---- counts: the l of the bond order parameters, the chains of a dihedral call, BadByCn's largest key ----
inline Verdict order_l_count(int32_t n_l, int max_l) { return refuse_if(n_l < 1 || n_l > max_l, AMOF_EINVAL, "n_l must be 1..%d", max_l); }
inline Verdict order_l(const int32_t *l, int32_t n_l, int l_top)
{
    for (int q = 0; q < n_l; q++)
        if (l[q] < 1 || l[q] > l_top) return refuse_if(true, AMOF_EINVAL, "l must be 1..%d", l_top);
    return Verdict();
}
inline Verdict chain_count(int32_t T, int max_chains) { return refuse_if(T < 1 || T > max_chains, AMOF_EINVAL, "n_chains must be 1..%d", max_chains); }
inline Verdict cn_max_range(int32_t cn_max) { return refuse_if(cn_max < 1 || cn_max > 65535, AMOF_EINVAL, "cn_max must be 1..65535"); }

// ---- one image at most.  hmin: the smallest perpendicular height over the periodic axes of every cell, +inf without one
// (which refuses nothing).  rec: build_geometry's records, GEOM_REC doubles a cell (= GEOM_STRIDE, amof_internal.h; nbr.hip
// asserts it) with the three heights from GEOM_HEIGHTS on.  No slack here, unlike pore_check's above_half_height.
constexpr int GEOM_REC = 24, GEOM_HEIGHTS = 18;
inline double min_periodic_height(const uint8_t *pbc /* [3], amof_traj's */, const double *rec, int64_t n_cells)
{
    double hmin = INFINITY;
    for (int64_t k = 0; k < n_cells; k++)
        for (int x = 0; x < 3; x++) {
            const double h = rec[(size_t)k * GEOM_REC + GEOM_HEIGHTS + x];
            if (pbc[x] && h < hmin) hmin = h;
        }
    return hmin;
}
inline Verdict half_height(double rc, double hmin)
{
    return refuse_if(rc > 0.5 * hmin, AMOF_EINVAL, "cutoff %g exceeds half the smallest cell height %g: a pair could be bonded twice", rc, hmin);
}
// tail: "a neighbour could be counted twice" (bond order) or "a pair could be bonded twice" (the bond dynamics)
inline Verdict half_height_set(double rc, int set, double hmin, const char *tail)
{
    return refuse_if(rc > 0.5 * hmin, AMOF_EINVAL, "cutoff %g of set %d exceeds half the smallest cell height %g: %s", rc, set, hmin, tail);
}

// ---- the step of uniform edges: edges[k] == (double)k * step exactly for k = 0 .. nb, one IEEE multiplication each as numpy
// and the kernels do it (volatile: no fused or extended-precision product), so that hist_bin may recompute the edges instead
// of reading the table.  0: read the table.
inline double uniform_edge_step(const double *edges, int32_t nb)
{
    if (edges[0] != 0.0) return 0.0;
    volatile double step = edges[1];
    for (int k = 0; k <= nb; k++) {
        volatile double e = (double)k * step;
        if (e != edges[k]) return 0.0;
    }
    return step;
}
}  // namespace nbr_check
}  // namespace amof
