// amof_amd/csrc/lindemann_math.h on the CPU: the chunk order of the moments, delta, the fixed-point term, the bin rule and the
// scale, as both GPU traversals compile them.  stdin: "B n e nbins ddelta", then B rows of n distances (block-relative frame
// by frame); stdout per series: the term and bin of the chunk traversal (partials stored per chunk, added afterwards, as the
// moments and reduce kernels do), the term and bin of the simple traversal, and the bits of both deltas.  "scale na nb B" on
// the command line prints the scale instead.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../amof_amd/csrc/lindemann_math.h"

using namespace amof;

int main(int argc, char **argv)
{
    if (argc == 5 && !strcmp(argv[1], "scale")) {
        printf("%d\n", lindemann::scale_log2(atoll(argv[2]), atoll(argv[3]), atoll(argv[4])));
        return 0;
    }
    long long B = 0, n = 0;
    int e = 0, nbins = 0;
    double ddelta = 0.0;
    if (scanf("%lld %lld %d %d %lf", &B, &n, &e, &nbins, &ddelta) != 5 || B < 2 || n < 0 || nbins < 1) return 2;
    std::vector<double> d((size_t)B * (size_t)n);
    for (double &x : d)
        if (scanf("%lf", &x) != 1) return 2;
    const int nk = lindemann::chunk_count(B);
    std::vector<double> part((size_t)nk * 2);
    for (long long p = 0; p < n; p++) {
        auto dist = [&](int64_t f) { return d[(size_t)f * (size_t)n + (size_t)p]; };
        const double c = dist(0);
        // the chunk traversal: every chunk on its own, in descending order here (a lane per chunk knows no order), then the sum
        for (int k = nk - 1; k >= 0; k--) lindemann::chunk_partial(dist, c, k, B, part[(size_t)k * 2], part[(size_t)k * 2 + 1]);
        double S1 = 0.0, S2 = 0.0;
        for (int k = 0; k < nk; k++) {
            S1 += part[(size_t)k * 2];
            S2 += part[(size_t)k * 2 + 1];
        }
        const double dc = lindemann::delta(c, S1, S2, B);
        // the simple traversal
        double T1, T2;
        lindemann::block_sums(dist, c, B, T1, T2);
        const double ds = lindemann::delta(c, T1, T2, B);
        uint64_t bc, bs;
        memcpy(&bc, &dc, 8);
        memcpy(&bs, &ds, 8);
        printf("%lld %d %lld %d %" PRIx64 " %" PRIx64 "\n", lindemann::fixed_term(dc, e), lindemann::bin_of(dc, ddelta, nbins),
               lindemann::fixed_term(ds, e), lindemann::bin_of(ds, ddelta, nbins), bc, bs);
    }
    return 0;
}
