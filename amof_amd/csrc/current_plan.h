// The host decisions of the current correlation functions C_L(q, t) and C_T(q, t) (current.hip, amof_current_*): the runs a
// thread of current_rho_kernel owns, the fixed-point scales, the vector chunks and the counter tiles of
// current_corr_kernel -- and the constants those decisions share with the kernels.  Everything else (species order, bin
// capacity, touched frames, the work list) is sq_plan.h's and lag_work.h's, unchanged.  Host only (no HIP dependency: the
// CPU test suite compiles it with g++, tests/test_current_plan_cpu.py through tests/native/current_plan_driver.cpp).
#pragma once

#include "lag_work.h"
#include "sq_plan.h"

namespace amof {

// Vectors per thread of current_rho_kernel.  A vector costs six f32 partials and six f64 sums (18 VGPRs) where
// sq_rho_kernel's costs two and two (6): SQ_RUN = 16 would need 288 VGPRs for the sums alone.  The compiler's resource
// report (-Rpass-analysis=kernel-resource-usage), none with scratch: R = 2: 50 VGPRs, 8 waves per SIMD; 4: 88, 5 waves;
// 6: 125, 4 waves; 8: 163, 3 waves.  4 keeps five waves in flight for the two transcendentals per vector and amortises the
// three integer multiplies and the two scalar record loads of an atom over four vectors.
constexpr int CUR_RUN = 4;
constexpr int CUR_THREADS = LAG_THREADS;    // current_rho_kernel and current_corr_kernel
constexpr int CUR_SMAX = LAG_SMAX;          // species counts whose 2 S^2 sums current_corr_kernel keeps in registers
constexpr int CUR_OPW = LAG_OPW;
constexpr size_t CUR_LDS_BUDGET = LAG_LDS_BUDGET;
constexpr size_t CUR_RHO_BUDGET = (size_t)1 << 30;      // bytes of the table [slots][K_c][S][6] f64 of one vector chunk

struct CurSwitches {
    bool global = false;                    // AMOF_CURRENT_GLOBAL (set): current_corr_kernel adds straight into global memory
    size_t rho_budget = CUR_RHO_BUDGET;     // AMOF_CURRENT_RHO_BUDGET (bytes; ignored unless positive)

    static CurSwitches from_env()
    {
        CurSwitches s;
        s.global = getenv("AMOF_CURRENT_GLOBAL") != nullptr;
        if (const char *e = getenv("AMOF_CURRENT_RHO_BUDGET")) {
            const long long b = atoll(e);
            if (b > 0) s.rho_budget = (size_t)b;
        }
        return s;
    }
};

// sq_cut_runs's rule with runs of at most CUR_RUN vectors: sorted by (h, k, l, caller's index), rows of consecutive l at fixed
// (h, k), cut every CUR_RUN vectors from the row's start -- sq_cut_runs's runs, each cut into pieces (CUR_RUN divides SQ_RUN,
// so the pieces are the runs a direct cut would give).  Returns the index of the first (0, 0, 0) vector (the plan is then
// not made), or -1.
static_assert(SQ_RUN % CUR_RUN == 0, "a run of current_rho_kernel is a piece of a run of sq_rho_kernel");
inline int32_t current_cut_runs(const int32_t *hkl, int32_t K, SqPlan &pl)
{
    const int32_t zero = sq_cut_runs(hkl, K, pl);
    if (zero >= 0) return zero;
    std::vector<SqRun> pieces;
    pieces.reserve(pl.runs.size() * (SQ_RUN / CUR_RUN));
    for (const SqRun &r : pl.runs)
        for (int32_t i = 0; i < r.n; i += CUR_RUN)
            pieces.push_back(SqRun{r.h, r.k, r.l0 + i, std::min<int32_t>(CUR_RUN, r.n - i), r.start + i, {0, 0, 0}});
    pl.runs.swap(pieces);
    return -1;
}

// ---- the fixed-point scales ----
// Per unordered pair {a, c}: |L_a conj L_c| and |T_a . conj T_c| are at most |j_a| |j_c| <= 3 vmax^2 N_a N_c (every velocity
// component is at most vmax in magnitude), and a counter receives at most n = F * cap samples (S(q)'s bound: sq_bin_capacity):
// 2^s is the largest power of two with S(q)'s bound times 3 vmax^2, F cap (N_a N_c + 1/2) 3 vmax^2 2^s, below 2^62 -- the
// scale follows vmax^2, whatever the units of the velocities.  The rounded samples then add up to less than 2^62 + n / 2 <
// 2^63 (n < 2^62): no counter overflows.  vmax is the trajectory's, not the call's: ranks and work ranges arrive at the same
// exponents.  vmax == 0: every sum is zero, scale 0 (exponent 0).
// Returns -1, or the index of the first pair whose quantum 2^-s exceeds 2^-20 of 3 vmax^2 sqrt(N_a N_c).  The record is
// S(q)'s (SqScales; sq_expand_pairs gives the [S][S] tables).
inline int current_scales(const int32_t *species, int64_t N, int S, int64_t F, int64_t cap, double vmax, SqScales &out)
{
    const int P = S * (S + 1) / 2;
    out.nsp.assign((size_t)S, 0);
    for (int64_t i = 0; i < N; i++) out.nsp[species[i]]++;
    out.cap = cap;
    out.sexp.assign(P, 0);
    out.scale.assign(P, 0.0);
    if (!(vmax > 0.0)) return -1;
    const double v2 = 3.0 * vmax * vmax;
    int p = 0;
    for (int a = 0; a < S; a++)
        for (int c = a; c < S; c++, p++) {
            const double na = (double)std::max<int64_t>(out.nsp[a], 1), nc = (double)std::max<int64_t>(out.nsp[c], 1);
            const double bound = (double)std::max<int64_t>(F, 1) * (double)std::max<int64_t>(cap, 1) * (na * nc + 0.5) * v2;
            int e;
            frexp(bound, &e);               // bound < 2^e
            out.sexp[p] = std::min(62 - e, 1000);
            out.scale[p] = ldexp(1.0, out.sexp[p]);
            if (ldexp(1.0, -out.sexp[p]) / (sqrt(na * nc) * v2) > ldexp(1.0, -20)) {
                out.bad_a = a;
                out.bad_c = c;
                return p;
            }
        }
    return -1;
}

// Vector chunks: F(q, t)'s rule (whole runs, whole waves of runs) for a table of 3 S complex numbers per vector and slot
inline void current_cut_chunks(const std::vector<SqRun> &runs, int32_t K, size_t slots, int S, size_t budget, IsfChunks &ch)
{
    isf_cut_chunks(runs, K, slots, 3 * S, budget, ch);
}

// current_corr_kernel's counters: sq_plan.h's rule with two sums per pair (longitudinal and transverse).  Its grid is
// lag_grid's with an origin tile of 1: a lane walks its origins lag by lag
using CurPass = LagPass;
using CurGrid = LagGrid;
inline LagPass current_pass_plan(int S, int32_t nbins, int W, const CurSwitches &sw)
{
    return lag_pass_plan(2, S, nbins, W, sw.global, "current", "current_global");
}
inline LagGrid current_grid(int nv, int64_t range) { return lag_grid(nv, range, 1); }

}  // namespace amof
