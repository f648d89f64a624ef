// The host decisions of S(q) and density_modes (sq.hip) and of F(q, t) (isf.hip): the species and hkl orders and the runs a
// thread of sq_rho_kernel owns, the fixed-point scales, the S(q) frame batch, the frames a lag call touches, its vector
// chunks and self-part batches, the counter tiles and the grid of a lag correlation kernel (F(q, t)'s and, through
// current_plan.h, C(q, t)'s: one rule each) -- and the constants those decisions share with the kernels.  Host only (no HIP
// dependency, no amof_ctx: the CPU test suite compiles it with g++, tests/test_sq_plan_cpu.py through
// tests/native/sq_plan_driver.cpp).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "lag_work.h"

namespace amof {

constexpr int SQ_THREADS = 256;
constexpr int SQ_RUN = 16;                  // vectors per thread (registers: two f32 partials and two f64 sums each)
constexpr int SQ_BLOCK = 64;                // atoms per f32 partial
constexpr size_t SQ_LDS_BUDGET = 64 * 1024; // LDS counters of sq_bin_kernel (u64)
constexpr size_t SQ_RHO_BUDGET = (size_t)512 << 20;   // bytes of rho per batch of frames
constexpr int SQ_BIN_BLOCKS = 1024;         // workgroups of sq_bin_kernel (grid-stride over the samples)
constexpr size_t SQ_GRID_Y = 65535;         // frames (slots, entries) one launch of a kernel indexed by blockIdx.y can take

// the lag correlation kernels (isf_corr_kernel, current_corr_kernel): one launch shape, one counter budget
constexpr int LAG_THREADS = 256;
constexpr int LAG_SMAX = 4;                 // species counts with a register form
constexpr int LAG_OPW = 64;                 // at most this many origins per workgroup
constexpr size_t LAG_LDS_BUDGET = 64 * 1024;

constexpr int ISF_THREADS = LAG_THREADS;
constexpr int ISF_TILE = 4;                 // origins whose rows a lane holds in registers
constexpr int ISF_SMAX = LAG_SMAX;
// rho table of one vector chunk: 1 GiB, twice S(q)'s batch.  The table is streamed (1 + W) times whatever its size, but a
// thread of sq_rho_kernel owns a run of up to 16 vectors and a chunk is cut to whole waves of runs: on the headline shape
// (5000 frames, 4 species: 320 KB per vector) 512 MB hold ~126 runs -- one whole wave, 13 launches with a tail each, the
// table 14 % slower than S(q)'s -- where 1 GiB holds three.  Next to Q (16 N bytes per frame) a rank's scratch stays near
// 2 GB there.  AMOF_ISF_RHO_BUDGET (bytes) overrides it (tests: several chunks on a small case).
constexpr size_t ISF_RHO_BUDGET = (size_t)1 << 30;

// ---- the switches (tests / measurements), read once per call ----
struct SqSwitches {
    bool sq_global = false;                 // AMOF_SQ_GLOBAL (set): sq_bin_kernel adds straight into global memory
    bool isf_global = false;                // AMOF_ISF_GLOBAL (set): isf_corr_kernel likewise
    size_t isf_rho_budget = ISF_RHO_BUDGET; // AMOF_ISF_RHO_BUDGET (bytes; ignored unless positive)

    static SqSwitches from_env()
    {
        SqSwitches s;
        s.sq_global = getenv("AMOF_SQ_GLOBAL") != nullptr;
        s.isf_global = getenv("AMOF_ISF_GLOBAL") != nullptr;
        if (const char *e = getenv("AMOF_ISF_RHO_BUDGET")) {
            const long long b = atoll(e);
            if (b > 0) s.isf_rho_budget = (size_t)b;
        }
        return s;
    }
};

// ---- the species order and the runs ----
struct SqRun {
    int32_t h, k, l0, n;    // vectors (h, k, l0 + r), r < n
    int32_t start;          // into order[]: the callers' indices of the run's vectors
    int32_t _pad[3];
};

struct SqPlan {
    std::vector<int32_t> perm;          // atoms in species order (stable)
    std::vector<int64_t> sp_first;      // [S + 1]
    std::vector<SqRun> runs;
    std::vector<int32_t> order;         // [K]: the callers' index of every sorted vector
};

inline void sq_species_order(const int32_t *species, int64_t N, int S, SqPlan &pl)
{
    pl.sp_first.assign((size_t)S + 1, 0);
    for (int64_t i = 0; i < N; i++) pl.sp_first[species[i] + 1]++;
    for (int s = 0; s < S; s++) pl.sp_first[s + 1] += pl.sp_first[s];
    pl.perm.resize(N);
    std::vector<int64_t> cur(pl.sp_first.begin(), pl.sp_first.end() - 1);
    for (int64_t i = 0; i < N; i++) pl.perm[cur[species[i]]++] = (int32_t)i;
}

// The vectors sorted by (h, k, l, caller's index); rows of consecutive l at fixed (h, k), cut into runs of at most SQ_RUN.
// Returns the index of the first (0, 0, 0) vector (the plan is then not made), or -1.
inline int32_t sq_cut_runs(const int32_t *hkl, int32_t K, SqPlan &pl)
{
    for (int32_t m = 0; m < K; m++)
        if (hkl[3 * m] == 0 && hkl[3 * m + 1] == 0 && hkl[3 * m + 2] == 0) return m;
    pl.order.resize(K);
    std::iota(pl.order.begin(), pl.order.end(), 0);
    std::sort(pl.order.begin(), pl.order.end(), [&](int32_t x, int32_t y) {
        const int32_t *a = hkl + 3 * x, *b = hkl + 3 * y;
        if (a[0] != b[0]) return a[0] < b[0];
        if (a[1] != b[1]) return a[1] < b[1];
        if (a[2] != b[2]) return a[2] < b[2];
        return x < y;
    });
    pl.runs.clear();
    for (int32_t i = 0; i < K; i++) {
        const int32_t *v = hkl + 3 * pl.order[i];
        if (!pl.runs.empty()) {
            SqRun &r = pl.runs.back();
            if (r.n < SQ_RUN && r.h == v[0] && r.k == v[1] && (int64_t)r.l0 + r.n == (int64_t)v[2]) {
                r.n++;
                continue;
            }
        }
        pl.runs.push_back(SqRun{v[0], v[1], v[2], 1, i, {0, 0, 0}});
    }
    return -1;
}

// ---- the fixed-point scales ----
// The largest number of vectors one bin can receive in one frame of ANY of the n_cells cells: every vector is counted in
// each bin its |q| can reach.  |q_c| lies within delta |hkl| of |hkl . Rm|, Rm the mean reciprocal matrix and delta the
// largest Frobenius norm of R_c - Rm (>= the spectral norm); a relative margin of 1e-9 covers the rounding of both.  One
// pass over the vectors (a difference array over the bins): for a constant cell this is the per-bin count itself, give or
// take a vector on a bin edge.
inline int64_t sq_bin_capacity(const double *recip, int64_t n_cells, const int32_t *hkl, int32_t K, double dq, int32_t nbins)
{
    double Rm[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, delta = 0.0;
    for (int64_t c = 0; c < n_cells; c++)
        for (int i = 0; i < 9; i++) Rm[i] += recip[9 * c + i];
    for (int i = 0; i < 9; i++) Rm[i] /= (double)std::max<int64_t>(n_cells, 1);
    for (int64_t c = 0; c < n_cells; c++) {
        double f2 = 0.0;
        for (int i = 0; i < 9; i++) f2 += (recip[9 * c + i] - Rm[i]) * (recip[9 * c + i] - Rm[i]);
        delta = std::max(delta, sqrt(f2));
    }
    std::vector<int64_t> diff((size_t)nbins + 1, 0);
    for (int32_t m = 0; m < K; m++) {
        const double h = hkl[3 * m], k = hkl[3 * m + 1], l = hkl[3 * m + 2];
        const double qx = (h * Rm[0] + k * Rm[3]) + l * Rm[6];
        const double qy = (h * Rm[1] + k * Rm[4]) + l * Rm[7];
        const double qz = (h * Rm[2] + k * Rm[5]) + l * Rm[8];
        const double qm = sqrt((qx * qx + qy * qy) + qz * qz), r = delta * sqrt((h * h + k * k) + l * l);
        const double lo = (qm - r) * (1.0 - 1e-9) / dq, hi = (qm + r) * (1.0 + 1e-9) / dq;
        if (!(lo < (double)nbins)) continue;                // beyond in every cell
        const int32_t b0 = lo > 0.0 ? (int32_t)lo : 0;
        const int32_t b1 = hi < (double)nbins ? (int32_t)hi : nbins - 1;
        diff[b0]++;
        diff[(size_t)b1 + 1]--;
    }
    int64_t run = 0, best = 0;
    for (int32_t b = 0; b < nbins; b++) {
        run += diff[b];
        best = std::max(best, run);
    }
    return best;
}

struct SqScales {
    std::vector<int64_t> nsp;           // [S] atoms per species
    int64_t cap = 0;                    // sq_bin_capacity
    std::vector<int32_t> sexp;          // [P] pairs a <= c, row-major
    std::vector<double> scale;          // [P] 2^sexp
    int bad_a = -1, bad_c = -1;         // the pair sq_scales refused
};

// Per-pair fixed-point scale 2^s: the sum over the trajectory's frames (ANY selection of them) of |t_ab| + 1/2 in one bin
// stays below 2^62 -- |t_ab| <= N_a N_b, and a bin receives at most F * sq_bin_capacity samples.  The scale depends on
// the trajectory's frame count and cells, the vectors, the bins and the species counts only: frame ranges of one
// trajectory add up exactly (and F(q, t) -- at most F samples of a vector per lag -- shares S(q)'s scale).
// Returns -1, or the index of the first pair whose quantum 2^-s in S units (divided by sqrt(N_a N_b)) exceeds 2^-20.
inline int sq_scales(const int32_t *species, int64_t N, int S, int64_t F, const double *recip, int64_t n_cells, const int32_t *hkl,
                     int32_t K, double dq, int32_t nbins, SqScales &out)
{
    const int P = S * (S + 1) / 2;
    out.nsp.assign((size_t)S, 0);
    for (int64_t i = 0; i < N; i++) out.nsp[species[i]]++;
    out.cap = sq_bin_capacity(recip, n_cells, hkl, K, dq, nbins);
    out.sexp.assign(P, 0);
    out.scale.assign(P, 0.0);
    int p = 0;
    for (int a = 0; a < S; a++)
        for (int c = a; c < S; c++, p++) {
            const double bound = (double)std::max<int64_t>(F, 1) * (double)std::max<int64_t>(out.cap, 1) *
                                 ((double)std::max<int64_t>(out.nsp[a], 1) * (double)std::max<int64_t>(out.nsp[c], 1) + 0.5);
            int e;
            frexp(bound, &e);               // bound < 2^e
            out.sexp[p] = std::min(62 - e, 60);
            out.scale[p] = ldexp(1.0, out.sexp[p]);
            const double nab = sqrt((double)std::max<int64_t>(out.nsp[a], 1) * (double)std::max<int64_t>(out.nsp[c], 1));
            if (ldexp(1.0, -out.sexp[p]) / nab > ldexp(1.0, -20)) {
                out.bad_a = a;
                out.bad_c = c;
                return p;
            }
        }
    return -1;
}

// the P pair scales as symmetric [S][S] tables (F(q, t) keeps both orders of a pair)
inline void sq_expand_pairs(int S, const SqScales &sc, std::vector<double> &scale2, std::vector<int32_t> &sexp2)
{
    scale2.assign((size_t)S * S, 0.0);
    sexp2.assign((size_t)S * S, 0);
    int p = 0;
    for (int a = 0; a < S; a++)
        for (int c = a; c < S; c++, p++) {
            scale2[a * S + c] = scale2[c * S + a] = sc.scale[p];
            sexp2[a * S + c] = sexp2[c * S + a] = sc.sexp[p];
        }
}

// ---- S(q): batches of selected frames ----
struct SqBatchPlan {
    size_t rho_frame = 0;       // bytes of one frame's rho [K][S][2]
    int nb_max = 1;             // frames per batch: inside the rho budget and one launch's gridDim.y (no slicing in S(q))
    size_t n_ctr = 0;           // counters of sq_bin_kernel: counts, P sums, beyond
    bool global = false;
    size_t lds = 0;             // dynamic LDS of sq_bin_kernel<false>
    const char *path = "";
};
inline SqBatchPlan sq_batch_plan(int32_t K, int S, int32_t nbins, size_t n_selected, const SqSwitches &sw)
{
    const int P = S * (S + 1) / 2;
    SqBatchPlan b;
    b.rho_frame = (size_t)K * S * 2 * sizeof(double);
    b.nb_max = (int)std::max<size_t>(1, std::min<size_t>({SQ_RHO_BUDGET / b.rho_frame, n_selected, SQ_GRID_Y}));
    b.n_ctr = (size_t)(P + 1) * nbins + 1;
    b.global = b.n_ctr * sizeof(uint64_t) > SQ_LDS_BUDGET || sw.sq_global;
    b.lds = b.global ? 0 : b.n_ctr * sizeof(uint64_t);
    b.path = b.global ? "sq_bin_global" : "sq";
    return b;
}

// workgroups of the kernels that grid-stride over (frame or entry, vector) samples
inline unsigned sq_sample_blocks(int nb, int32_t K)
{
    const int64_t samples = (int64_t)nb * K;
    return (unsigned)std::min<int64_t>(SQ_BIN_BLOCKS, (samples + SQ_THREADS - 1) / SQ_THREADS);
}

// ---- F(q, t) ----
struct IsfEntry {
    int32_t w, k;           // lag index, origin frame
    int32_t sk, skm;        // slots of frames k and k + m in Q
};

// the frames the work range touches, ascending: slot s of Q and of the rho table holds frame fsel[s]
struct IsfFrames {
    std::vector<int32_t> slot_of;       // [F] (-1: not touched)
    std::vector<int32_t> fsel;
    int omin = 0x7fffffff, omax = 0;    // the origin indices of all lags lie in [omin, omax)
};
inline void isf_touched_frames(const LagRange *lagiv, const int32_t *windows, int W, int64_t F, int64_t stride, IsfFrames &fr)
{
    fr.slot_of.assign((size_t)F, -1);
    fr.fsel.clear();
    fr.omin = 0x7fffffff;
    fr.omax = 0;
    for (int w = 0; w < W; w++) {
        if (lagiv[w].o0 >= lagiv[w].o1) continue;
        fr.omin = std::min(fr.omin, lagiv[w].o0);
        fr.omax = std::max(fr.omax, lagiv[w].o1);
        for (int64_t o = lagiv[w].o0; o < lagiv[w].o1; o++) {
            const int64_t k = lag_origin_frame(o, stride);
            fr.slot_of[k] = 0;
            fr.slot_of[k + windows[w]] = 0;
        }
    }
    for (int64_t f = 0; f < F; f++)
        if (fr.slot_of[f] == 0) {
            fr.slot_of[f] = (int32_t)fr.fsel.size();
            fr.fsel.push_back((int32_t)f);
        }
}

// the self part's (lag, origin) entries, lag-major
inline void isf_self_entries(const LagRange *lagiv, const int32_t *windows, int W, int64_t stride, const IsfFrames &fr,
                             std::vector<IsfEntry> &entries)
{
    entries.clear();
    size_t n = 0;
    for (int w = 0; w < W; w++) n += (size_t)(lagiv[w].o1 - lagiv[w].o0);
    entries.reserve(n);
    for (int w = 0; w < W; w++)
        for (int64_t o = lagiv[w].o0; o < lagiv[w].o1; o++) {
            const int64_t k = lag_origin_frame(o, stride);
            entries.push_back(IsfEntry{w, (int32_t)k, fr.slot_of[k], fr.slot_of[k + windows[w]]});
        }
}

// Vector chunks: whole runs of the sorted list, at most kc_max vectors (at least one run); a chunk's rho table
// [slots][nv][S][2] stays inside the budget.  order_local numbers each chunk's vectors from 0 (what sq_rho_kernel takes as
// `order` when it fills a chunk's table).
struct IsfChunk {
    int r0, r1, v0, nv;     // runs [r0, r1); nv vectors from position v0 of the sorted list
};
struct IsfChunks {
    size_t vec_bytes = 0, kc_max = 1;
    std::vector<IsfChunk> chunks;
    std::vector<int32_t> order_local;   // [K]
    int kc_top = 0;                     // the largest nv
};
inline void isf_cut_chunks(const std::vector<SqRun> &runs, int32_t K, size_t slots, int S, size_t budget, IsfChunks &ch)
{
    ch.vec_bytes = slots * (size_t)S * 2 * sizeof(double);
    ch.kc_max = std::max<size_t>(1, budget / ch.vec_bytes);
    ch.chunks.clear();
    ch.order_local.assign((size_t)K, 0);
    const int n_runs_all = (int)runs.size();
    for (int r0 = 0; r0 < n_runs_all;) {
        int r1 = r0, nv = 0;
        while (r1 < n_runs_all && (r1 == r0 || (size_t)(nv + runs[r1].n) <= ch.kc_max)) nv += runs[r1++].n;
        // a thread of sq_rho_kernel owns a run: whole waves of runs, so that a chunk leaves no lane of its last wave idle
        if (r1 < n_runs_all && r1 - r0 > 64)
            while ((r1 - r0) % 64) nv -= runs[--r1].n;
        ch.chunks.push_back(IsfChunk{r0, r1, runs[r0].start, nv});
        for (int i = 0; i < nv; i++) ch.order_local[runs[r0].start + i] = i;
        r0 = r1;
    }
    ch.kc_top = 0;
    for (const IsfChunk &c : ch.chunks) ch.kc_top = std::max(ch.kc_top, c.nv);
}

// The counters of a lag correlation kernel (isf_corr_kernel, current_corr_kernel): per-lag LDS tiles of counts and
// sums_per_pair S^2 sums per bin, as many lags per pass as fit the budget, or global memory (a tile beyond the budget, or
// force_global); the two names are the paths the call reports
struct LagPass {
    size_t tile_ctr = 0;        // counters of one lag
    bool global = false;
    int lags_per_pass = 0;
    size_t lds = 0;
    const char *path = "";
};
inline LagPass lag_pass_plan(int sums_per_pair, int S, int32_t nbins, int W, bool force_global, const char *lds_path,
                             const char *global_path)
{
    LagPass p;
    p.tile_ctr = (size_t)(1 + sums_per_pair * S * S) * nbins;
    p.global = p.tile_ctr * sizeof(uint64_t) > LAG_LDS_BUDGET || force_global;
    p.lags_per_pass = p.global ? W : (int)std::min<size_t>(W, LAG_LDS_BUDGET / (p.tile_ctr * sizeof(uint64_t)));
    p.lds = (size_t)p.lags_per_pass * p.tile_ctr * sizeof(uint64_t);
    p.path = p.global ? global_path : lds_path;
    return p;
}
using IsfPass = LagPass;        // isf_corr_kernel's: one sum per pair
inline LagPass isf_pass_plan(int S, int32_t nbins, int W, const SqSwitches &sw)
{
    return lag_pass_plan(1, S, nbins, W, sw.isf_global, "isf", "isf_global");
}

// The grid of a lag correlation kernel over a chunk of nv vectors and `range` origin indices.  Origins per workgroup: a
// multiple of the origin tile a lane holds in registers (ISF_TILE; 1: none), enough workgroups to fill the GPU several times
// over, at most LAG_OPW origins each, and no more than 65535 workgroups along y.
struct LagGrid {
    int vblocks;
    int32_t opw;
    unsigned gy;
};
inline LagGrid lag_grid(int nv, int64_t range, int tile)
{
    LagGrid g;
    g.vblocks = (nv + LAG_THREADS - 1) / LAG_THREADS;
    int64_t opw = std::min<int64_t>(LAG_OPW, std::max<int64_t>(tile, range * g.vblocks / 2048 / tile * tile));
    opw = std::max<int64_t>(opw, ((range + 65534) / 65535 + tile - 1) / tile * tile);
    g.opw = (int32_t)opw;
    g.gy = (unsigned)((range + opw - 1) / opw);
    return g;
}
using IsfGrid = LagGrid;        // isf_corr_kernel's: origins ISF_TILE at a time
inline LagGrid isf_grid(int nv, int64_t range) { return lag_grid(nv, range, ISF_TILE); }

// self part: batches of entries inside the same budget -- D (16 N bytes) and rho_d (16 K S bytes) per entry
inline size_t isf_self_batch(size_t budget, int64_t N, int32_t K, int S, size_t n_entries)
{
    const size_t ent_bytes = (size_t)std::max<int64_t>(N, 1) * 16 + (size_t)K * S * 2 * sizeof(double);
    return std::max<size_t>(1, std::min<size_t>({budget / ent_bytes, n_entries, SQ_GRID_Y}));
}

}  // namespace amof
