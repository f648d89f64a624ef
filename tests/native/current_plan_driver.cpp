// Answers questions about amof_amd/csrc/current_plan.h on stdin (tests/test_current_plan_cpu.py), one line each:
//   "K"                                   -> CUR_RUN CUR_THREADS CUR_SMAX CUR_OPW CUR_LDS_BUDGET CUR_RHO_BUDGET
//   "V"                                   -> global rho_budget of CurSwitches::from_env
//   "R K h0 k0 l0 .."                     -> zero n_runs (h k l0 n start).. order[K]   (zero >= 0: "zero 0" alone)
//   "E S N F cap vmax species.."          -> bad bad_a bad_c nsp[S] sexp[P] scale[P], then (bad < 0) sexp2[S S] scale2[S S]
//   "H slots S budget K h0 k0 l0 .."      -> vec_bytes kc_max kc_top n_chunks (r0 r1 v0 nv).. order_local[K]
//   "P S nbins W global"                  -> tile_ctr global lags_per_pass lds path
//   "G nv range"                          -> vblocks opw gy
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/current_plan.h"

using namespace amof;

static bool read_ints(std::vector<int32_t> &v)
{
    for (auto &x : v)
        if (scanf("%d", &x) != 1) return false;
    return true;
}

static int runs_line()
{
    int K;
    if (scanf("%d", &K) != 1 || K < 0 || K > 10000000) return 1;
    std::vector<int32_t> hkl((size_t)K * 3);
    if (!read_ints(hkl)) return 1;
    SqPlan pl;
    const int32_t zero = current_cut_runs(hkl.data(), K, pl);
    printf("%d %zu", zero, pl.runs.size());
    for (const SqRun &r : pl.runs) printf(" %d %d %d %d %d", r.h, r.k, r.l0, r.n, r.start);
    for (int32_t v : pl.order) printf(" %d", v);
    printf("\n");
    return 0;
}

static int scales_line()
{
    int S;
    long long N, F, cap;
    double vmax;
    if (scanf("%d %lld %lld %lld %lf", &S, &N, &F, &cap, &vmax) != 5 || S < 1 || S > 64 || N < 0 || N > 10000000) return 1;
    std::vector<int32_t> sp((size_t)N);
    if (!read_ints(sp)) return 1;
    for (int32_t s : sp)
        if (s < 0 || s >= S) return 1;
    SqScales sc;
    const int bad = current_scales(sp.data(), N, S, F, cap, vmax, sc);
    printf("%d %d %d", bad, sc.bad_a, sc.bad_c);
    for (int64_t n : sc.nsp) printf(" %lld", (long long)n);
    for (int32_t e : sc.sexp) printf(" %d", e);
    for (double x : sc.scale) printf(" %.17g", x);
    if (bad < 0) {
        std::vector<double> scale2;
        std::vector<int32_t> sexp2;
        sq_expand_pairs(S, sc, scale2, sexp2);
        for (int32_t e : sexp2) printf(" %d", e);
        for (double x : scale2) printf(" %.17g", x);
    }
    printf("\n");
    return 0;
}

static int chunks_line()
{
    long long slots, budget;
    int S, K;
    if (scanf("%lld %d %lld %d", &slots, &S, &budget, &K) != 4 || slots < 1 || S < 1 || budget < 1 || K < 0 || K > 10000000) return 1;
    std::vector<int32_t> hkl((size_t)K * 3);
    if (!read_ints(hkl)) return 1;
    SqPlan pl;
    if (current_cut_runs(hkl.data(), K, pl) >= 0) return 1;
    IsfChunks ch;
    current_cut_chunks(pl.runs, K, (size_t)slots, S, (size_t)budget, ch);
    printf("%zu %zu %d %zu", ch.vec_bytes, ch.kc_max, ch.kc_top, ch.chunks.size());
    for (const IsfChunk &c : ch.chunks) printf(" %d %d %d %d", c.r0, c.r1, c.v0, c.nv);
    for (int32_t v : ch.order_local) printf(" %d", v);
    printf("\n");
    return 0;
}

int main()
{
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'K') {
            printf("%d %d %d %d %zu %zu\n", CUR_RUN, CUR_THREADS, CUR_SMAX, CUR_OPW, CUR_LDS_BUDGET, CUR_RHO_BUDGET);
        } else if (op == 'V') {
            const CurSwitches s = CurSwitches::from_env();
            printf("%d %zu\n", (int)s.global, s.rho_budget);
        } else if (op == 'R') {
            if (runs_line()) return 1;
        } else if (op == 'E') {
            if (scales_line()) return 1;
        } else if (op == 'H') {
            if (chunks_line()) return 1;
        } else if (op == 'P') {
            int S, nbins, W, global;
            if (scanf("%d %d %d %d", &S, &nbins, &W, &global) != 4 || S < 1 || nbins < 1 || W < 0) return 1;
            CurSwitches sw;
            sw.global = global != 0;
            const CurPass p = current_pass_plan(S, nbins, W, sw);
            printf("%zu %d %d %zu %s\n", p.tile_ctr, (int)p.global, p.lags_per_pass, p.lds, p.path);
        } else if (op == 'G') {
            int nv;
            long long range;
            if (scanf("%d %lld", &nv, &range) != 2 || nv < 1 || range < 1) return 1;
            const CurGrid g = current_grid(nv, range);
            printf("%d %d %u\n", g.vblocks, g.opw, g.gy);
        } else {
            return 1;
        }
    }
    return 0;
}
