// Prints what amof_amd/csrc/tri_select.h selects for the cells on stdin (tests/test_tri_select_cpu.py).  The inputs the
// host hands the selection are formed as rdf.hip forms them: perpendicular heights from the inverse cell, csum, quant,
// guard_m and guard_f (general cells: fast_guard_rel_rdf = 1.1 (5 kappa_rdf + 3.06) u), and the selected variant passes
// the host's final check of its guard (fast_guard_tri) before it counts as taken.
//   line "C nohalf nbins rmax n c0 .. c(9n-1)" ->
//        "ok code ax0 ax1 axis cull share l10_bins c10 tau guard_f quant" then per cell "rec0 .. rec8" on the same line
// cull: what the host decides for the tile kernels, 2 rmax 1.05 < the smallest height along the slab axis.
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/tri_select.h"

static void heights_of(const double *c, double *h)
{
    const double det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6]);
    double inv[9];
    inv[0] = (c[4] * c[8] - c[5] * c[7]) / det;
    inv[1] = (c[2] * c[7] - c[1] * c[8]) / det;
    inv[2] = (c[1] * c[5] - c[2] * c[4]) / det;
    inv[3] = (c[5] * c[6] - c[3] * c[8]) / det;
    inv[4] = (c[0] * c[8] - c[2] * c[6]) / det;
    inv[5] = (c[2] * c[3] - c[0] * c[5]) / det;
    inv[6] = (c[3] * c[7] - c[4] * c[6]) / det;
    inv[7] = (c[1] * c[6] - c[0] * c[7]) / det;
    inv[8] = (c[0] * c[4] - c[1] * c[3]) / det;
    for (int k = 0; k < 3; k++) h[k] = 1.0 / sqrt(inv[k] * inv[k] + inv[3 + k] * inv[3 + k] + inv[6 + k] * inv[6 + k]);
}

int main()
{
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag != 'C') return 2;
        int nohalf, nbins;
        long long n;
        double rmax;
        if (scanf("%d %d %lf %lld", &nohalf, &nbins, &rmax, &n) != 4 || n < 1 || nbins < 1) return 1;
        std::vector<double> c((size_t)n * 9), h((size_t)n * 3);
        for (auto &v : c)
            if (scanf("%lf", &v) != 1) return 1;
        double csum = 0.0, hmin[3] = {1e300, 1e300, 1e300};
        for (long long k = 0; k < n; k++) {
            const double *r = &c[(size_t)k * 9];
            heights_of(r, &h[(size_t)k * 3]);
            for (int x = 0; x < 3; x++) hmin[x] = std::min(hmin[x], h[(size_t)k * 3 + x]);
            csum = std::max(csum, sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]) + sqrt(r[3] * r[3] + r[4] * r[4] + r[5] * r[5]) +
                                      sqrt(r[6] * r[6] + r[7] * r[7] + r[8] * r[8]));
        }
        const double dr = rmax / (double)nbins;
        const double quant = csum * (1.0 / 2147483648.0);
        const double guard_m = quant / dr + (double)nbins * 1e-12;
        const double u = 1.0 / 16777216.0;
        const double guard_f = (double)nbins * 1.1 * (5.0 * amof::kappa_rdf(c.data(), n) + 3.06) * u + guard_m;
        amof::TriSelect s;
        if (guard_f < 0.25) s = amof::tri_select(c.data(), h.data(), n, rmax, nbins, guard_f, quant, dr, nohalf != 0);
        if (s.ok) {
            double hb = 0.0;
            for (long long k = 0; k < n; k++) hb = std::max(hb, h[(size_t)k * 3 + s.axis] / dr);
            if (!(amof::fast_guard_tri(nbins, hb, 0.5, s.l10_bins) * (1.0 + 4.0 * s.tau) + 2.0 * quant / dr +
                  (1.0 + 256.0 * s.c10) * 1.5 * csum / 4294967296.0 / dr + (double)nbins * 1e-12 < 0.25)) s.ok = false;
        }
        int axis = 0;
        for (int x = 1; x < 3; x++)
            if (hmin[x] > hmin[axis]) axis = x;
        const int cull = 2.0 * rmax * 1.05 < hmin[axis] ? 1 : 0;
        printf("%d %d %d %d %d %d %.17g %.17g %.17g %.17g %.17g %.17g", s.ok ? 1 : 0, s.code, s.ax0, s.ax1, s.axis, cull, s.share,
               s.l10_bins, s.c10, s.tau, guard_f, quant);
        if (s.ok)
            for (double v : s.rec) printf(" %.17g", v);
        printf("\n");
    }
    return 0;
}
