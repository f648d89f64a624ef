// Driver for tests/test_pore_host.py: the float32 candidate arithmetic of amof_amd/csrc/pore_math.h against long double on
// random bricks, and the two sweeps of pore_brick_kernel restated with the header's own predicates.
// stdin, per line:  rcut hd R_lo R_hi atoms points seed
// stdout, per line: eps_c  worst |cand - v|  points whose true nearest atom the second sweep did not select  selected per point
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/pore_math.h"

static uint64_t state;
static double uniform()
{
    state = state * 6364136223846793005ULL + 1442695040888963407ULL;
    return (double)(state >> 11) / 9007199254740992.0;
}
static void direction(double v[3])
{
    for (;;) {
        double q = 0.0;
        for (int c = 0; c < 3; c++) {
            v[c] = 2.0 * uniform() - 1.0;
            q += v[c] * v[c];
        }
        if (q > 1e-3 && q <= 1.0) {
            for (int c = 0; c < 3; c++) v[c] /= sqrt(q);
            return;
        }
    }
}

int main()
{
    double rcut, hd, r_lo, r_hi;
    int atoms, points;
    unsigned long long seed;
    while (scanf("%lf %lf %lf %lf %d %d %llu", &rcut, &hd, &r_lo, &r_hi, &atoms, &points, &seed) == 7) {
        state = seed;
        const double cell[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // (the arithmetic part of the bound alone)
        const double eps = amof::pore_candidate_bound(cell, rcut);
        const float e2 = (float)(2.0 * eps) * (1.0f + 2.4e-7f);
        double worst = 0.0, selected = 0.0;
        long missed = 0;
        for (int p = 0; p < points; p++) {
            // one brick: images with |A| < rcut + hd around a point with |P| <= hd; a few pairs of near-ties among them
            std::vector<double> A((size_t)atoms * 3), R((size_t)atoms);
            double P[3], u[3];
            direction(u);
            const double pl = hd * cbrt(uniform());
            for (int c = 0; c < 3; c++) P[c] = u[c] * pl;
            for (int j = 0; j < atoms; j++) {
                R[j] = r_lo + (r_hi - r_lo) * uniform();
                direction(u);
                double len = (rcut + hd) * cbrt(uniform());
                if (j > 0 && j % 4 == 0) {
                    // (a near-tie with atom j - 1 at this point: the same value up to a few eps)
                    double prev = 0.0;
                    for (int c = 0; c < 3; c++) prev += (A[(size_t)(j - 1) * 3 + c] - P[c]) * (A[(size_t)(j - 1) * 3 + c] - P[c]);
                    const double want = sqrt(prev) - R[j - 1] + R[j] + (uniform() - 0.5) * 4.0 * eps;
                    for (int c = 0; c < 3; c++) A[(size_t)j * 3 + c] = P[c] + u[c] * fabs(want);
                    continue;
                }
                for (int c = 0; c < 3; c++) A[(size_t)j * 3 + c] = u[c] * len;
            }
            const float pf[3] = {(float)P[0], (float)P[1], (float)P[2]};
            std::vector<float> d2((size_t)atoms), r32((size_t)atoms);
            long double best = INFINITY;
            int arg = -1;
            float m = (float)rcut * (1.0f + 1.2e-7f);
            for (int j = 0; j < atoms; j++) {
                r32[j] = (float)R[j];
                d2[j] = amof::pore_cand_d2((float)A[(size_t)j * 3], (float)A[(size_t)j * 3 + 1], (float)A[(size_t)j * 3 + 2], pf[0], pf[1], pf[2]);
                long double q = 0.0L;
                for (int c = 0; c < 3; c++) {
                    const long double d = (long double)A[(size_t)j * 3 + c] - (long double)P[c];
                    q += d * d;
                }
                const long double v = sqrtl(q) - (long double)R[j];
                const double err = fabs((double)((long double)amof::pore_cand(d2[j], r32[j]) - v));
                if (sqrtl(q) <= (long double)(rcut + 2.0 * hd)) worst = err > worst ? err : worst;
                if (v < best) {
                    best = v;
                    arg = j;
                }
                if (amof::pore_could_lower(d2[j], m, r32[j])) m = fminf(m, amof::pore_cand(d2[j], r32[j]));
            }
            const float me = m + e2;
            bool hit = false;
            for (int j = 0; j < atoms; j++)
                if (amof::pore_selected(d2[j], me, r32[j])) {
                    selected += 1.0;
                    hit = hit || j == arg;
                }
            if (!hit && best < (long double)rcut - (long double)r_hi) missed++;      // (a value below dmax must be found)
        }
        printf("%.17g %.17g %ld %.17g\n", eps, worst, missed, selected / points);
    }
    return 0;
}
