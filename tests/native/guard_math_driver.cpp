// Prints what amof_amd/csrc/guard_math.h computes for the inputs on stdin (tests/test_guard_math.py and
// tests/test_guard_band_cpu.py compare with numpy).
//   line "L r0 .. r8"                  -> the nine entries of lower_factor(rows) and kappa_lower(L)
//   line "Z nbins hb gfrac"            -> fast_guard_zf(nbins, hb, gfrac)
//   line "R n c0 .. c(9n-1)"           -> kappa_rdf(cells, n)
//   line "P c0 .. c8 i0 .. i8"         -> kappa_cell(cell, inv)
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/guard_math.h"

int main()
{
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'L') {
            double r[9], L[9];
            for (int k = 0; k < 9; k++)
                if (scanf("%lf", &r[k]) != 1) return 1;
            amof::lower_factor(r, L);
            for (int k = 0; k < 9; k++) printf("%.17g ", L[k]);
            printf("%.17g\n", amof::kappa_lower(L));
        } else if (tag == 'Z') {
            int nbins;
            double hb, gfrac;
            if (scanf("%d %lf %lf", &nbins, &hb, &gfrac) != 3) return 1;
            printf("%.17g\n", amof::fast_guard_zf(nbins, hb, gfrac));
        } else if (tag == 'R') {
            long long n;
            if (scanf("%lld", &n) != 1 || n < 1) return 1;
            std::vector<double> c((size_t)n * 9);
            for (auto &v : c)
                if (scanf("%lf", &v) != 1) return 1;
            printf("%.17g\n", amof::kappa_rdf(c.data(), n));
        } else if (tag == 'P') {
            double c[9], inv[9];
            for (int k = 0; k < 9; k++)
                if (scanf("%lf", &c[k]) != 1) return 1;
            for (int k = 0; k < 9; k++)
                if (scanf("%lf", &inv[k]) != 1) return 1;
            printf("%.17g\n", amof::kappa_cell(c, inv));
        } else {
            return 2;
        }
    }
    return 0;
}
