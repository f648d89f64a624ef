// CPU driver of amof_amd/csrc/fragment_math.h (tests/test_fragment_native_cpu.py): the text the GPU kernels compile, on rows the
// test writes.  stdin: "N ortho", the 24 doubles of a geometry record, N positions, N masses, N rows of 16 neighbour indices, N
// degrees.  stdout: "ok <rounds>", N lines "label sx sy sz winds" and, per root in ascending order, "root atoms mass cx cy cz"
// (nan for a winding fragment); or "capacity" where an image, a shift or a coordinate does not fit.
#include <cstdio>
#include <vector>

#include "../../amof_amd/csrc/fragment_math.h"

int main()
{
    int N = 0, ortho = 0;
    if (scanf("%d %d", &N, &ortho) != 2 || N < 0 || N > FRAG_MAX_ATOMS) return 2;
    double g[24];
    for (double &x : g)
        if (scanf("%lf", &x) != 1) return 2;
    std::vector<double> pos((size_t)N * 3), mass((size_t)N);
    std::vector<int32_t> adj((size_t)N * FRAG_MAX_DEGREE), deg((size_t)N);
    for (double &x : pos)
        if (scanf("%lf", &x) != 1) return 2;
    for (double &x : mass)
        if (scanf("%lf", &x) != 1 || !(x > 0.0) || !(x < FRAG_MASS_MAX)) return 2;
    for (int32_t &x : adj)
        if (scanf("%d", &x) != 1) return 2;
    for (int32_t &x : deg)
        if (scanf("%d", &x) != 1 || x < 0 || x > FRAG_MAX_DEGREE) return 2;
    for (int i = 0; i < N; i++)
        for (int q = 0; q < deg[(size_t)i]; q++)
            if (adj[(size_t)i * FRAG_MAX_DEGREE + q] < 0 || adj[(size_t)i * FRAG_MAX_DEGREE + q] >= N) return 2;
    bool over = false;
    std::vector<uint32_t> img((size_t)N * FRAG_MAX_DEGREE, 0u);
    for (int i = 0; i < N; i++)
        for (int q = 0; q < deg[(size_t)i]; q++) {
            const size_t j = (size_t)adj[(size_t)i * FRAG_MAX_DEGREE + q];
            double n[3];
            frag::pair_image(g, ortho != 0, pos[j * 3 + 0] - pos[(size_t)i * 3 + 0], pos[j * 3 + 1] - pos[(size_t)i * 3 + 1],
                             pos[j * 3 + 2] - pos[(size_t)i * 3 + 2], n);
            if (!frag::pack_image(n, &img[(size_t)i * FRAG_MAX_DEGREE + q])) over = true;
        }
    std::vector<frag::Rec> A((size_t)N), B((size_t)N);
    for (int i = 0; i < N; i++) A[(size_t)i] = frag::Rec{(uint16_t)i, {0, 0, 0}};
    int rounds = 0;
    while (rounds < N) {
        bool changed = false;
        for (int i = 0; i < N; i++)
            B[(size_t)i] = frag::relabel(A.data(), adj.data() + (size_t)i * FRAG_MAX_DEGREE, img.data() + (size_t)i * FRAG_MAX_DEGREE, deg[(size_t)i], i,
                                         &changed, &over);
        rounds++;
        A.swap(B);
        if (!changed) break;
    }
    std::vector<int> winds((size_t)N, 0), atoms((size_t)N, 0);
    std::vector<long long> sums((size_t)N * 6, 0);
    std::vector<double> total((size_t)N, 0.0);
    for (int i = 0; i < N; i++) {
        const frag::Rec r = A[(size_t)i];
        for (int q = 0; q < deg[(size_t)i]; q++)
            if (!frag::bond_holds(r, A[(size_t)adj[(size_t)i * FRAG_MAX_DEGREE + q]], img[(size_t)i * FRAG_MAX_DEGREE + q])) winds[r.label] = 1;
        double x[3];
        frag::whole_coord(g, pos.data() + (size_t)i * 3, r.s, x);
        for (int c = 0; c < 3; c++) {
            long long hi = 0, lo = 0;
            if (!frag::fixed_term(mass[(size_t)i], x[c], &hi, &lo)) over = true;
            sums[((size_t)r.label * 3 + c) * 2] += hi;
            sums[((size_t)r.label * 3 + c) * 2 + 1] += lo;
        }
        atoms[r.label]++;
        total[r.label] += mass[(size_t)i];
    }
    if (over) {
        printf("capacity\n");
        return 0;
    }
    printf("ok %d\n", rounds);
    for (int i = 0; i < N; i++) printf("%d %d %d %d %d\n", A[(size_t)i].label, A[(size_t)i].s[0], A[(size_t)i].s[1], A[(size_t)i].s[2], winds[A[(size_t)i].label]);
    for (int r = 0; r < N; r++) {
        if (A[(size_t)r].label != r) continue;
        printf("%d %d %.17g", r, atoms[(size_t)r], total[(size_t)r]);
        for (int c = 0; c < 3; c++) printf(" %.17g", winds[(size_t)r] ? (double)NAN : frag::centre(sums[((size_t)r * 3 + c) * 2], sums[((size_t)r * 3 + c) * 2 + 1], total[(size_t)r]));
        printf("\n");
    }
    return 0;
}
