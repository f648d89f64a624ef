// Does the selection (amof_amd/csrc/rdf_select.h) hand the planned f32-slab slice its saturating tail?  For
// tests/test_gpu_tile_sat.py and tests/test_tile_sat_cpu.py.  Diagonal cells only; one request per line on stdin:
//   nbins rmax nosat n  lx ly lz (n times)
// one line on stdout:  zf cull sat guard_zf_sat one_p_guard two_guard two_guard_below lds_planned lds_planned_sat
// (two_guard_below: the float below two_guard; the tile tier runs the tail when sat is set and the batch is planned)
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/rdf_select.h"

using namespace amof;

int main()
{
    int nbins, nosat;
    long long n;
    double rmax;
    while (scanf("%d %lf %d %lld", &nbins, &rmax, &nosat, &n) == 4) {
        if (nbins < 1 || n < 1 || n > 100000) return 1;
        std::vector<double> c((size_t)n * 9, 0.0), h((size_t)n * 3);
        for (long long k = 0; k < n; k++)
            for (int x = 0; x < 3; x++) {
                if (scanf("%lf", &h[(size_t)k * 3 + x]) != 1) return 1;
                c[(size_t)k * 9 + 4 * x] = h[(size_t)k * 3 + x];
            }
        const uint8_t pbc[3] = {1, 1, 1};
        const int64_t nsp[1] = {4096};
        RdfSwitches sw;
        sw.nocell = sw.norange = true;
        sw.nosat = nosat != 0;
        const RdfSelect s = rdf_select(c.data(), h.data(), n, pbc, 1, nsp[0], nsp, nbins, rmax, 0, true, sw);
        printf("%d %d %d %.17g %.9g %.9g %.9g %zu %zu\n", s.zf, s.cull, s.sat, s.guard_zf_sat, (double)s.sat_thr.one_p_guard,
               (double)s.sat_thr.two_guard, (double)nextafterf(s.sat_thr.two_guard, -INFINITY), tile_lds(nbins, 0, 0, true, false),
               tile_lds(nbins, 0, 0, true, true));
    }
    return 0;
}
