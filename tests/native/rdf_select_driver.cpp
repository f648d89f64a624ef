// Answers questions about amof_amd/csrc/rdf_select.h on stdin (tests/test_rdf_select_cpu.py), one line each:
//   "G nbins guard"            -> nb_hi, half_m_guard, and for each the neighbouring float on the far side of the bound
//   "T nf npairs fpc notail"   -> fpc chunks xcd_map nf_tail nf_main plan_fits
//   "F ortho o0 o1 o2 dr c0..c8" -> sc64[0..8] sc[0..8] of fill_frame_scales for one cell
//   "S nbins rmax max_img N S nsp.. pbc0 pbc1 pbc2 n c.. | switch names .. ;"
//                              -> plain img tri zf cull cell range axis nz2 axis_y gy nk0 nk1 nk2 guard_f then near_thr ..
// The selection's inputs are formed as rdf.hip forms them: perpendicular heights from the inverse cell, all_ortho from the
// off-diagonal elements.
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../amof_amd/csrc/rdf_select.h"

using namespace amof;

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

static bool set_switch(RdfSwitches &sw, const std::string &name)
{
    struct { const char *n; bool RdfSwitches::*m; } tab[] = {
        {"v1", &RdfSwitches::v1}, {"noimg", &RdfSwitches::noimg}, {"force_img", &RdfSwitches::force_img},
        {"notri", &RdfSwitches::notri}, {"nohalf", &RdfSwitches::nohalf}, {"nocull", &RdfSwitches::nocull},
        {"nozf", &RdfSwitches::nozf}, {"nocell", &RdfSwitches::nocell}, {"force_cell", &RdfSwitches::force_cell},
        {"norange", &RdfSwitches::norange}, {"force_range", &RdfSwitches::force_range}};
    for (auto &e : tab)
        if (name == e.n) { sw.*(e.m) = true; return true; }
    return false;
}

static int select_line()
{
    int nbins, max_img, S, pbc_i[3];
    long long N, n;
    double rmax;
    if (scanf("%d %lf %d %lld %d", &nbins, &rmax, &max_img, &N, &S) != 5 || nbins < 1 || S < 1 || S > 64) return 1;
    std::vector<int64_t> nsp((size_t)S);
    for (auto &v : nsp) {
        long long x;
        if (scanf("%lld", &x) != 1) return 1;
        v = x;
    }
    if (scanf("%d %d %d %lld", &pbc_i[0], &pbc_i[1], &pbc_i[2], &n) != 4 || n < 1 || n > 100000) return 1;
    const uint8_t pbc[3] = {(uint8_t)pbc_i[0], (uint8_t)pbc_i[1], (uint8_t)pbc_i[2]};
    std::vector<double> c((size_t)n * 9), h((size_t)n * 3);
    for (auto &v : c)
        if (scanf("%lf", &v) != 1) return 1;
    bool all_ortho = true;
    for (long long k = 0; k < n; k++) {
        heights_of(&c[(size_t)k * 9], &h[(size_t)k * 3]);
        for (int q = 0; q < 9; q++)
            if (q % 4 != 0 && c[(size_t)k * 9 + q] != 0.0) all_ortho = false;
    }
    RdfSwitches sw;
    char word[64];
    if (scanf(" %63s", word) != 1 || strcmp(word, "|") != 0) return 1;
    while (scanf(" %63s", word) == 1 && strcmp(word, ";") != 0)
        if (!set_switch(sw, word)) return 3;
    const RdfSelect s = rdf_select(c.data(), h.data(), n, pbc, S, N, nsp.data(), nbins, rmax, max_img, all_ortho, sw);
    printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %.17g", s.plain, s.img, s.tri.ok, s.zf, s.cull, s.cell, s.range, s.axis, s.nz2,
           s.axis_y, s.gy, s.nk[0], s.nk[1], s.nk[2], s.guard_f);
    for (uint32_t v : s.near_thr) printf(" %u", v);
    printf("\n");
    return 0;
}

int main()
{
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'G') {
            int nbins;
            double g;
            if (scanf("%d %lf", &nbins, &g) != 2) return 1;
            const GuardThresholds t = guard_thresholds(nbins, g);
            printf("%.17g %.17g %.17g %.17g\n", (double)t.nb_hi, (double)nextafterf(t.nb_hi, -INFINITY), (double)t.half_m_guard,
                   (double)nextafterf(t.half_m_guard, INFINITY));
        } else if (tag == 'T') {
            long long nf, npairs;
            RdfSwitches sw;
            int notail;
            if (scanf("%lld %lld %d %d", &nf, &npairs, &sw.fpc, &notail) != 4 || nf < 1 || npairs < 1) return 1;
            sw.notail = notail != 0;
            const TileChunks c = tile_chunks(nf, npairs, sw);
            printf("%d %d %d %d %d %d\n", c.fpc, c.chunks, c.xcd_map, c.nf_tail, c.nf_main, c.plan_fits ? 1 : 0);
        } else if (tag == 'F') {
            int ortho, ord[3];
            double dr, c[9];
            if (scanf("%d %d %d %d %lf", &ortho, &ord[0], &ord[1], &ord[2], &dr) != 5) return 1;
            for (double &v : c)
                if (scanf("%lf", &v) != 1) return 1;
            for (int q = 0; q < 3; q++)
                if (ord[q] < 0 || ord[q] > 2) return 1;
            FrameScale r = {};
            fill_frame_scales(c, 1, ortho != 0, ord, dr, nullptr, nullptr, &r);
            for (double v : r.sc64) printf("%.17g ", v);
            for (float v : r.sc) printf("%.9g ", (double)v);
            printf("\n");
        } else if (tag == 'S') {
            const int rc = select_line();
            if (rc) return rc;
        } else {
            return 2;
        }
    }
    return 0;
}
