// Which instantiation of the general-cell tile kernel (rdf.hip: rdf_tile_tri) answers a trajectory's cells, and the
// per-cell records it runs from.  Host only (no HIP dependency: the CPU test suite compiles it with g++,
// tests/test_tri_select_cpu.py through tests/native/tri_select_driver.cpp).
//
// TRI: general cells in the orthogonalised lattice frame (see fast_quad_tri).
// Stored order (x, y, z = slab axis): of the two orders of the other axes the one that leaves the x wrap the
// larger slack.  Conditions per cell, with R = rmax (1 + guards) and the lower factor L in Angstrom:
//   X: R / L00 + |L10| / (2 L00) < 1/2 - 1e-6     (the x wrap, decided without the c10 iy term, cannot lose an in-range image)
//   Y: tau_y = R / L11 - 1/2 <= 0: unique; else pairs with |iy| > 1/2 - tau_y are flagged near (<= 1.5 % of them)
//   Z: likewise with L22 (= the slab axis's perpendicular height)
#pragma once

#include <math.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "guard_math.h"

namespace amof {

struct TriSelect {
    bool ok = false;
    // code: near tests (0 none, 1 slow path only, 2 fast path y, 3 y + z, 4 y with its twin image) + 5 x (x wrap with the
    // y term); 10 / 11: near mode 4 with the exact-half x wrap, c10 = + 1/2 / - 1/2
    int code = 0, ax0 = -1, ax1 = -1, axis = 0;
    double share = 0.0, l10_bins = 0.0, c10 = 0.0, tau = 0.0;
    std::vector<double> fold;       // [nc][2] kx, ky
    std::vector<double> rec;        // [nc][9] L00 L10 L11 L22 (bins per 2^-32), thr_y (units), thr_z (bins), kx, ky, thr_x (units)
};

// cells: [nc][9] rows = lattice vectors; heights: [nc][3] perpendicular heights; guard_f, quant, dr as the host of the
// tile kernels has them; nohalf: never the exact-half x wrap (AMOF_RDF_NOHALF)
inline TriSelect tri_select(const double *cells, const double *heights, int64_t nc, double rmax, int nbins, double guard_f,
                            double quant, double dr, bool nohalf)
{
    TriSelect out;
    const double two32_ = 1.0 / 4294967296.0;
    double hmin3[3] = {1e300, 1e300, 1e300};
    for (int64_t k = 0; k < nc; k++)
        for (int x = 0; x < 3; x++) hmin3[x] = std::min(hmin3[x], heights[(size_t)k * 3 + x]);
    int tri_axis = 0;
    for (int x = 1; x < 3; x++)
        if (hmin3[x] > hmin3[tri_axis]) tri_axis = x;
    out.axis = tri_axis;
    const double R = rmax * (1.0 + 4.0 * guard_f / (double)nbins + 1e-6);
    double best_cost = 1e300;
    for (int sw = 0; sw < 2; sw++) {
        const int a0 = sw ? (tri_axis + 2) % 3 : (tri_axis + 1) % 3, a1 = sw ? (tri_axis + 1) % 3 : (tri_axis + 2) % 3;
        const int ordt[3] = {a0, a1, tri_axis};
        bool ok = true;
        double slack = 1e300, share = 0.0, l10b = 0.0, c10max = 0.0, tau_max = 0.0;
        int near = 0;
        bool twin = false, xw_wraps = false, twin_wraps = false, twin_short = false, half_p = true, half_m = true;
        std::vector<double> fold((size_t)nc * 2), rec((size_t)nc * 9);
        for (int64_t k = 0; k < nc && ok; k++) {
            const double *c = cells + 9 * k;
            double rows[9], L[9];
            for (int q = 0; q < 3; q++)
                for (int x = 0; x < 3; x++) rows[3 * q + x] = c[3 * ordt[q] + x];
            lower_factor(rows, L);
            if (!(L[0] > 0.0 && L[4] > 0.0 && L[8] > 0.0)) { ok = false; break; }
            // (no slack: the x wrap takes the c10 iy term along, XW -- two instructions more per pair)
            slack = std::min(slack, 0.5 - 1e-6 - (R / L[0] + 0.5 * fabs(L[3]) / L[0]));
            c10max = std::max(c10max, fabs(L[3]) / L[0]);
            double tau_y = R / L[4] - 0.5 + 1e-9, tau_z = R / L[8] - 0.5 + 1e-9;
            // (a second image along y up to 9 % of the pairs either side -- hexagonal cells: 7.7 % -- is evaluated by the
            //  slow path itself, near mode 4; along z only what the canonical queue can take)
            if (tau_y > 0.09 || tau_z > 0.0075) { ok = false; break; }
            if (tau_y > 0.0075) twin = true;
            // (near mode 4 counts the nearer of two candidates that differ by a lattice vector +-(B - k A), x wrapped:
            //  only where every such vector is at least 2 rmax long can the other one never be in range as well)
            {
                const double xr = L[3] - L[0] * rint(L[3] / L[0]);
                if (sqrt(L[4] * L[4] + xr * xr) * (1.0 + 1e-12) < 2.0 * rmax) twin_short = true;
            }
            tau_max = std::max(tau_max, std::max(tau_y, 0.0));
            // The x wrap of XW and of the twin image forms (int)(fy * c10), fy = the y difference in units of 2^-32 of the
            // cell: modular arithmetic only while |fy c10| < 2^31 (the conversion saturates beyond).  In range means
            // |fy| <= R / L11 cells (the twin: 1/2 + tau_y), so a skewed, non-reduced cell with |L10| >~ L00 cannot take
            // these variants: rdf_tile_img / rdf_exact answer it.
            if (fabs(L[3]) / L[0] * (R / L[4] + 1e-3) >= 0.5 - 1e-3) xw_wraps = true;
            if (fabs(L[3]) / L[0] * (0.5 + std::max(tau_y, 0.0) + 1e-3) >= 0.5 - 1e-3) twin_wraps = true;
            // A second image along y (z) can only be in range when L11 / 2 < R0 (canonical rmax with rounding slack);
            // then its in-plane components are below rho = sqrt(R0^2 - (L/2)^2), the evaluated image's differ from them
            // by at most the lattice offsets, so it lies between L - R0 and sqrt(D2max) from the origin.  When that
            // whole interval is within g_m / 2 of the cutoff the pair is flagged by the guard band of the last bin
            // edge anyway: no compare in the fast path (the slow path tests, and parks it).
            const double R0 = rmax * (1.0 + 1e-12), gband = 0.5 * (2.0 * quant / dr + (double)nbins * 1e-12);
            auto covered = [&](double Lk, double off_a, double off_b) {
                const double rho = sqrt(std::max(0.0, R0 * R0 - 0.25 * Lk * Lk));
                const double d2max = 0.25 * Lk * Lk + (rho + off_a) * (rho + off_a) + (rho + off_b) * (rho + off_b);
                return (Lk - R0) / dr >= (double)nbins - gband && sqrt(d2max) / dr <= (double)nbins + gband;
            };
            if (0.5 * L[4] >= R0) tau_y = -1.0;       // no second image along y at all
            else near = std::max(near, covered(L[4], fabs(L[3]), 0.0) ? 1 : 2);
            if (0.5 * L[8] >= R0) tau_z = -1.0;
            else near = std::max(near, covered(L[8], fabs(L[7]), fabs(L[6]) + fabs(L[3])) ? 1 : 3);
            // x: |A| >= 2 rmax whenever rmax is the reference's half shortest length; a larger rmax (the C ABI
            // takes any) would need a near test on x in the fast path: not this variant
            double tau_x = R / L[0] - 0.5 + 1e-9;
            if (0.5 * L[0] >= R0) tau_x = -1.0;
            else if (covered(L[0], 0.0, 0.0)) near = std::max(near, 1);
            else { ok = false; break; }
            share = std::max(share, tau_y > 0.0075 ? 0.012 : 2.0 * std::max(tau_y, 0.0) + 2.0 * std::max(tau_z, 0.0));
            l10b = std::max(l10b, fabs(L[3]) / dr);
            const double c10 = L[3] / L[0], r20 = L[6] / L[0], r21 = L[7] / L[4];
            // (c10 = +-1/2 to 2^-33: the exact-half x wrap of near mode 4, tri_q_twin<HALF>, is then right to one grid unit)
            if (fabs(c10 - 0.5) > 1e-10) half_p = false;
            if (fabs(c10 + 0.5) > 1e-10) half_m = false;
            fold[(size_t)k * 2] = r20 - c10 * r21;
            fold[(size_t)k * 2 + 1] = r21;
            double *r = &rec[(size_t)k * 9];
            r[0] = L[0] * two32_ / dr; r[1] = L[3] * two32_ / dr; r[2] = L[4] * two32_ / dr; r[3] = L[8] * two32_ / dr;
            // thresholds with room for the f32 conversions / coordinates of the fast path (flag a few more, never fewer)
            r[4] = tau_y > 0.0 ? (0.5 - tau_y) * 4294967296.0 * (1.0 - 1e-6) - 8.0 : INFINITY;
            r[5] = tau_z > 0.0 ? (L[8] - R) / dr * (1.0 - 1e-6) - 0.02 : INFINITY;
            r[6] = fold[(size_t)k * 2]; r[7] = fold[(size_t)k * 2 + 1];
            r[8] = tau_x > 0.0 ? (0.5 - tau_x) * 4294967296.0 * (1.0 - 1e-6) - 1024.0 : INFINITY;     // (f32 sum: 2^-23 of 2^31)
        }
        // cheaper order first: a near test costs a compare per pair, the x wrap two instructions in the chain
        // (measured: + 8 % per compare, + 24 % for the wrap, profiles/r04/tri_experiments.txt)
        if (twin) {
            if (near == 3) ok = false;      // (a common twin along y AND near tests along z: the image-aware / exact kernels)
            if (twin_wraps || twin_short) ok = false;
            near = 4;
        }
        if (!(slack > 0.0) && xw_wraps) ok = false;
        int code = near + (slack > 0.0 ? 0 : 5);
        if (near == 4 && (half_p || half_m) && !nohalf) code = half_p ? 10 : 11;
        const double cost = (near == 0 ? 0.0 : near == 1 ? 0.5 : near == 4 ? 6.0 : (double)(near - 1) * 1.5) +
                            (slack > 0.0 ? 0.0 : 2.5);
        if (ok && (!out.ok || cost < best_cost)) {
            best_cost = cost;
            out.ok = true; out.code = code; out.ax0 = a0; out.ax1 = a1; out.share = share; out.l10_bins = l10b; out.c10 = c10max;
            out.tau = tau_max;
            out.fold.swap(fold); out.rec.swap(rec);
        }
    }
    return out;
}

}  // namespace amof
