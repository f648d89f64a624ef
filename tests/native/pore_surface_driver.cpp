// Driver for tests/test_pore_surface_native_cpu.py, a program of its own (nothing is loaded into Python):
// 1. the float32 decision of amof_amd/csrc/pore_surface_math.h against long double on random neighbourhoods
//      "bound reach r_lo atoms neighbours samples seed"
//      -> "eps  worst |float32 value - long double value|  decisions long double takes the other way  share inside the band
//          buried  clear"
// 2. the surface rules of amof_amd/csrc/pore_check.h, answered as tests/native/pore_check_driver.cpp does ("code <tab> value
//    <tab> message"; doubles read with %lf; a pointer argument is a 0 / 1)
//      "count n_dirs" | "dirs n x0 y0 z0 .." | "probes n t0 .." | "hhs rmax tmax hmin" | "scap n_t atoms n_dirs" |
//      "outputs F n_t want_access exposed exposed_access"
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../amof_amd/csrc/pore_check.h"
#include "../../amof_amd/csrc/pore_surface_math.h"

using namespace amof;
using pore_check::Verdict;

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

static int dummy;
static const void *ptr(long long given) { return given ? &dummy : nullptr; }
static void answer(const Verdict &v, double value) { printf("%d\t%.17g\t%s\n", v.code, value, v.text); }

static bool doubles(std::vector<double> &v, int per)
{
    long long n;
    if (scanf("%lld", &n) != 1 || n < 0 || n > 100000) return false;
    v.resize((size_t)n * per);
    for (double &x : v)
        if (scanf("%lf", &x) != 1) return false;
    return true;
}

static void bound_line(double reach, double r_lo, int atoms, int neighbours, int samples)
{
    const double cell[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};      // (the arithmetic part of the bound alone)
    const double eps = pore_surface_bound(cell, reach);
    const float eps32 = surf_eps32(eps);
    double worst = 0.0;
    long wrong = 0, band = 0, buried = 0, clear = 0, total = 0;
    for (int j = 0; j < atoms; j++) {
        // one wave: an atom with sphere radius rho_j, images with |A| < rho_j + rho_k around it
        const double rho_j = r_lo + (reach - r_lo) * uniform();
        std::vector<double> A((size_t)neighbours * 3), rho((size_t)neighbours);
        for (int k = 0; k < neighbours; k++) {
            double u[3];
            direction(u);
            rho[k] = r_lo + (reach - r_lo) * uniform();
            const double len = (rho_j + rho[k]) * cbrt(uniform());
            for (int c = 0; c < 3; c++) A[(size_t)k * 3 + c] = u[c] * len;
        }
        for (int m = 0; m < samples; m++) {
            double u[3], P[3];
            direction(u);
            for (int c = 0; c < 3; c++) P[c] = rho_j * u[c];
            // every other sample: one neighbour moved so that the sample lies within a few eps of its sphere
            if (m % 2 == 1) {
                const int k = m % neighbours;
                double w[3];
                direction(w);
                const double want = rho[k] + (uniform() - 0.5) * 8.0 * eps;
                for (int c = 0; c < 3; c++) A[(size_t)k * 3 + c] = P[c] + w[c] * want;
            }
            const float pf[3] = {(float)P[0], (float)P[1], (float)P[2]};
            for (int k = 0; k < neighbours; k++) {
                long double q = 0.0L;
                for (int c = 0; c < 3; c++) {
                    const long double d = (long double)A[(size_t)k * 3 + c] - (long double)P[c];
                    q += d * d;
                }
                if (sqrtl(q) > (long double)(3.02 * reach)) continue;       // (the wave keeps no such image)
                const long double v = sqrtl(q) - (long double)rho[k];
                const float r32 = (float)rho[k];
                const float d2 = surf_d2((float)A[(size_t)k * 3], (float)A[(size_t)k * 3 + 1], (float)A[(size_t)k * 3 + 2], pf[0], pf[1], pf[2]);
                const double err = fabs((double)((long double)sqrtf(d2) - (long double)r32 - v));
                worst = err > worst ? err : worst;
                const int dec = surf_decide(d2, r32, eps32);
                total++;
                band += dec == 0;
                buried += dec < 0;
                clear += dec > 0;
                if ((dec < 0 && !(v < 0.0L)) || (dec > 0 && !(v >= 0.0L))) wrong++;
            }
        }
    }
    printf("%.17g %.17g %ld %.17g %ld %ld\n", eps, worst, wrong, (double)band / (double)(total ? total : 1), buried, clear);
}

int main()
{
    char word[64];
    while (scanf(" %63s", word) == 1) {
        const std::string w(word);
        long long a[6];
        double x, y, z;
        std::vector<double> v;
        unsigned long long seed;
        int n1, n2, n3;
        if (w == "bound" && scanf("%lf %lf %d %d %d %llu", &x, &y, &n1, &n2, &n3, &seed) == 6) {
            state = seed;
            bound_line(x, y, n1, n2, n3);
        } else if (w == "count" && scanf("%lld", a) == 1) {
            answer(pore_check::direction_count((int32_t)a[0]), 0.0);
        } else if (w == "dirs" && doubles(v, 3)) {
            answer(pore_check::directions(v.data(), (int32_t)(v.size() / 3)), 0.0);
        } else if (w == "probes" && doubles(v, 1)) {
            answer(pore_check::probes_not_negative(v.data(), (int32_t)v.size()), 0.0);
        } else if (w == "hhs" && scanf("%lf %lf %lf", &x, &y, &z) == 3) {
            answer(pore_check::half_height_surface(x, y, z), 0.0);
        } else if (w == "scap" && scanf("%lld %lld %lld", a, a + 1, a + 2) == 3) {
            answer(pore_check::samples_cap((int32_t)a[0], a[1], (int32_t)a[2]), 0.0);
        } else if (w == "outputs" && scanf("%lld %lld %lld %lld %lld", a, a + 1, a + 2, a + 3, a + 4) == 5) {
            answer(pore_check::surface_outputs(a[0], (int32_t)a[1], (int32_t)a[2], ptr(a[3]), ptr(a[4])), 0.0);
        } else {
            fprintf(stderr, "bad question: %s\n", word);
            return 2;
        }
    }
    return 0;
}
