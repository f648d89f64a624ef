// Answers questions about amof_amd/csrc/sq_plan.h on stdin (tests/test_sq_plan_cpu.py), one line each:
//   "V"                                   -> sq_global isf_global isf_rho_budget of SqSwitches::from_env
//   "O S N s0 .. sN-1"                    -> perm[N] sp_first[S + 1]
//   "R K h0 k0 l0 .."                     -> zero n_runs (h k l0 n start).. order[K]   (zero >= 0: "zero 0" alone)
//   "C n_cells K nbins dq recip.. hkl.."  -> sq_bin_capacity
//   "E S N F n_cells K nbins dq species.. recip.. hkl.."
//        -> bad bad_a bad_c cap nsp[S] sexp[P] scale[P], then (bad < 0) sexp2[S S] scale2[S S]
//   "B K S nbins n_selected sq_global"    -> nb_max rho_frame n_ctr global lds path
//   "N nb K"                              -> sq_sample_blocks
//   "T W F stride wb we w0 .. wW-1"       -> total omin omax n_sel fsel.. slot_of[F] n_entries (w k sk skm)..
//   "H slots S budget K h0 k0 l0 .."      -> vec_bytes kc_max kc_top n_runs n(run).. n_chunks (r0 r1 v0 nv).. order_local[K]
//   "P S nbins W isf_global"              -> tile_ctr global lags_per_pass lds path
//   "G nv range"                          -> vblocks opw gy
//   "F budget N K S n_entries"            -> isf_self_batch
//   "Q sums S nbins W global"             -> tile_ctr global lags_per_pass lds path of lag_pass_plan itself (paths "lds" / "glob")
//   "L nv range tile"                     -> vblocks opw gy of lag_grid itself
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/sq_plan.h"

using namespace amof;

static bool read_ints(std::vector<int32_t> &v)
{
    for (auto &x : v)
        if (scanf("%d", &x) != 1) return false;
    return true;
}

static bool read_doubles(std::vector<double> &v)
{
    for (auto &x : v)
        if (scanf("%lf", &x) != 1) return false;
    return true;
}

static int species_line()
{
    int S;
    long long N;
    if (scanf("%d %lld", &S, &N) != 2 || S < 1 || N < 0 || N > 10000000) return 1;
    std::vector<int32_t> sp((size_t)N);
    if (!read_ints(sp)) return 1;
    for (int32_t s : sp)
        if (s < 0 || s >= S) return 1;
    SqPlan pl;
    sq_species_order(sp.data(), N, S, pl);
    for (int32_t v : pl.perm) printf("%d ", v);
    for (int64_t v : pl.sp_first) printf("%lld ", (long long)v);
    printf("\n");
    return 0;
}

static int runs_line()
{
    int K;
    if (scanf("%d", &K) != 1 || K < 0 || K > 10000000) return 1;
    std::vector<int32_t> hkl((size_t)K * 3);
    if (!read_ints(hkl)) return 1;
    SqPlan pl;
    const int32_t zero = sq_cut_runs(hkl.data(), K, pl);
    printf("%d %zu", zero, pl.runs.size());
    for (const SqRun &r : pl.runs) printf(" %d %d %d %d %d", r.h, r.k, r.l0, r.n, r.start);
    for (int32_t v : pl.order) printf(" %d", v);
    printf("\n");
    return 0;
}

static int capacity_line(bool scales)
{
    int S = 1, K, nbins;
    long long N = 0, F = 1, n_cells;
    double dq;
    if (scales && (scanf("%d %lld %lld", &S, &N, &F) != 3 || S < 1 || S > 64 || N < 0 || N > 10000000)) return 1;
    if (scanf("%lld %d %d %lf", &n_cells, &K, &nbins, &dq) != 4 || n_cells < 1 || n_cells > 100000 || K < 0 || K > 10000000 ||
        nbins < 1 || nbins > 100000000 || !(dq > 0.0)) return 1;
    std::vector<int32_t> sp((size_t)N), hkl((size_t)K * 3);
    std::vector<double> recip((size_t)n_cells * 9);
    if ((scales && !read_ints(sp)) || !read_doubles(recip) || !read_ints(hkl)) return 1;
    if (!scales) {
        printf("%lld\n", (long long)sq_bin_capacity(recip.data(), n_cells, hkl.data(), K, dq, nbins));
        return 0;
    }
    SqScales sc;
    const int bad = sq_scales(sp.data(), N, S, F, recip.data(), n_cells, hkl.data(), K, dq, nbins, sc);
    printf("%d %d %d %lld", bad, sc.bad_a, sc.bad_c, (long long)sc.cap);
    for (int64_t v : sc.nsp) printf(" %lld", (long long)v);
    for (int32_t v : sc.sexp) printf(" %d", v);
    for (double v : sc.scale) printf(" %.17g", v);
    if (bad < 0) {
        std::vector<double> scale2;
        std::vector<int32_t> sexp2;
        sq_expand_pairs(S, sc, scale2, sexp2);
        for (int32_t v : sexp2) printf(" %d", v);
        for (double v : scale2) printf(" %.17g", v);
    }
    printf("\n");
    return 0;
}

static int touched_line()
{
    int W;
    long long F, stride, wb, we;
    if (scanf("%d %lld %lld %lld %lld", &W, &F, &stride, &wb, &we) != 5 || W < 1 || W > 100000 || F < 1 || F > 10000000 || stride < 1) return 1;
    std::vector<int32_t> win((size_t)W);
    if (!read_ints(win)) return 1;
    for (int32_t m : win)
        if (m < 0 || m >= F) return 1;
    std::vector<LagRange> iv((size_t)W);
    const int64_t total = lag_work_ranges(win.data(), W, F, stride, wb, we, iv.data());
    if (wb < 0 || we > total || wb > we) return 1;
    IsfFrames fr;
    isf_touched_frames(iv.data(), win.data(), W, F, stride, fr);
    std::vector<IsfEntry> ent;
    isf_self_entries(iv.data(), win.data(), W, stride, fr, ent);
    printf("%lld %d %d %zu", (long long)total, fr.omin, fr.omax, fr.fsel.size());
    for (int32_t v : fr.fsel) printf(" %d", v);
    for (int32_t v : fr.slot_of) printf(" %d", v);
    printf(" %zu", ent.size());
    for (const IsfEntry &e : ent) printf(" %d %d %d %d", e.w, e.k, e.sk, e.skm);
    printf("\n");
    return 0;
}

static int chunks_line()
{
    long long slots, budget;
    int S, K;
    if (scanf("%lld %d %lld %d", &slots, &S, &budget, &K) != 4 || slots < 1 || S < 1 || budget < 1 || K < 1 || K > 10000000) return 1;
    std::vector<int32_t> hkl((size_t)K * 3);
    if (!read_ints(hkl)) return 1;
    SqPlan pl;
    if (sq_cut_runs(hkl.data(), K, pl) >= 0) return 1;
    IsfChunks ch;
    isf_cut_chunks(pl.runs, K, (size_t)slots, S, (size_t)budget, ch);
    printf("%zu %zu %d %zu", ch.vec_bytes, ch.kc_max, ch.kc_top, pl.runs.size());
    for (const SqRun &r : pl.runs) printf(" %d", r.n);
    printf(" %zu", ch.chunks.size());
    for (const IsfChunk &c : ch.chunks) printf(" %d %d %d %d", c.r0, c.r1, c.v0, c.nv);
    for (int32_t v : ch.order_local) printf(" %d", v);
    printf("\n");
    return 0;
}

int main()
{
    char tag;
    while (scanf(" %c", &tag) == 1) {
        int rc = 0;
        if (tag == 'V') {
            const SqSwitches sw = SqSwitches::from_env();
            printf("%d %d %zu\n", sw.sq_global, sw.isf_global, sw.isf_rho_budget);
        } else if (tag == 'O') {
            rc = species_line();
        } else if (tag == 'R') {
            rc = runs_line();
        } else if (tag == 'C' || tag == 'E') {
            rc = capacity_line(tag == 'E');
        } else if (tag == 'B') {
            int K, S, nbins, glob;
            long long n_sel;
            if (scanf("%d %d %d %lld %d", &K, &S, &nbins, &n_sel, &glob) != 5 || K < 1 || S < 1 || nbins < 1 || n_sel < 1) return 1;
            SqSwitches sw;
            sw.sq_global = glob != 0;
            const SqBatchPlan b = sq_batch_plan(K, S, nbins, (size_t)n_sel, sw);
            printf("%d %zu %zu %d %zu %s\n", b.nb_max, b.rho_frame, b.n_ctr, b.global, b.lds, b.path);
        } else if (tag == 'N') {
            int nb, K;
            if (scanf("%d %d", &nb, &K) != 2 || nb < 1 || K < 1) return 1;
            printf("%u\n", sq_sample_blocks(nb, K));
        } else if (tag == 'T') {
            rc = touched_line();
        } else if (tag == 'H') {
            rc = chunks_line();
        } else if (tag == 'P') {
            int S, nbins, W, glob;
            if (scanf("%d %d %d %d", &S, &nbins, &W, &glob) != 4 || S < 1 || nbins < 1 || W < 0) return 1;
            SqSwitches sw;
            sw.isf_global = glob != 0;
            const IsfPass p = isf_pass_plan(S, nbins, W, sw);
            printf("%zu %d %d %zu %s\n", p.tile_ctr, p.global, p.lags_per_pass, p.lds, p.path);
        } else if (tag == 'G') {
            int nv;
            long long range;
            if (scanf("%d %lld", &nv, &range) != 2 || nv < 1 || range < 1) return 1;
            const IsfGrid g = isf_grid(nv, range);
            printf("%d %d %u\n", g.vblocks, g.opw, g.gy);
        } else if (tag == 'Q') {
            int sums, S, nbins, W, glob;
            if (scanf("%d %d %d %d %d", &sums, &S, &nbins, &W, &glob) != 5 || sums < 1 || S < 1 || nbins < 1 || W < 0) return 1;
            const LagPass p = lag_pass_plan(sums, S, nbins, W, glob != 0, "lds", "glob");
            printf("%zu %d %d %zu %s\n", p.tile_ctr, p.global, p.lags_per_pass, p.lds, p.path);
        } else if (tag == 'L') {
            int nv, tile;
            long long range;
            if (scanf("%d %lld %d", &nv, &range, &tile) != 3 || nv < 1 || range < 1 || tile < 1) return 1;
            const LagGrid g = lag_grid(nv, range, tile);
            printf("%d %d %u\n", g.vblocks, g.opw, g.gy);
        } else if (tag == 'F') {
            long long budget, N, n_entries;
            int K, S;
            if (scanf("%lld %lld %d %d %lld", &budget, &N, &K, &S, &n_entries) != 5 || budget < 1 || N < 0 || K < 1 || S < 1 || n_entries < 1)
                return 1;
            printf("%zu\n", isf_self_batch((size_t)budget, N, K, S, (size_t)n_entries));
        } else {
            return 2;
        }
        if (rc) return rc;
    }
    return 0;
}
