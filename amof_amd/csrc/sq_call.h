// What S(q) (sq.hip), F(q, t) (isf.hip) and C_L/C_T(q, t) (current.hip) share on the host: the call record and its stage
// functions (defined in sq.hip, which also owns the quantiser and sq_rho_kernel: every kernel is launched from the file that
// defines it), and the scaffold of the two lag analyses -- one call record, one argument record for both correlation kernels,
// one chunk loop, one launch by species count, one finish.  The rules behind the launches are sq_plan.h's.
#pragma once

#include <vector>

#include "amof_internal.h"
#include "sq_plan.h"

namespace amof {

// What every stage of a call needs, filled in this order: the arguments (the entry point), S .. F (sq_check_traj), the scales
// (sq_call_scales), the plan (build_geometry, sq_call_plan), the device side (sq_stage).
struct SqCall {
    amof_ctx *ctx;
    const amof_traj *t;
    const double *recip;        // [n_cells][9]; NULL in amof_sq_modes and amof_current_modes, which bin nothing
    const int32_t *hkl;
    int32_t K;
    double dq;
    int32_t nbins;
    int S = 0, P = 0;
    int64_t N = 0, F = 0;
    SqSwitches sw = SqSwitches::from_env();
    SqScales sc;
    HostGeom hg;
    SqPlan pl;
    const double *pos_dev = nullptr;
    UploadPack pk;              // a form adds its own tables before sq_stage uploads everything at once
    int i_geom = -1, i_perm = -1, i_spf = -1, i_runs = -1, i_order = -1, i_hkl = -1, i_recip = -1, i_frames = -1;
    uint4 *d_Q = nullptr;       // SLOT_AUX0
    double *d_rho = nullptr;    // SLOT_AUX1
    int32_t *d_flag = nullptr;  // SLOT_FLAGS, zeroed
    SqCall(amof_ctx *ctx_, const amof_traj *t_, const double *recip_, const int32_t *hkl_, int32_t K_, double dq_, int32_t nbins_)
        : ctx(ctx_), t(t_), recip(recip_), hkl(hkl_), K(K_), dq(dq_), nbins(nbins_) {}
};

// The caller's counters.  Host form: u64, overwritten.  Device form: u64, added into.  An entry point fills one of the two;
// scale_log2 receives the pairs' exponents (S(q) and F(q, t): device form only).
struct SqCounters {
    uint64_t *counts = nullptr, *beyond = nullptr;
    uint64_t *counts_dev = nullptr, *beyond_dev = nullptr;
    int32_t *scale_log2 = nullptr;
    bool host() const { return counts != nullptr; }
};

int sq_check_traj(SqCall &c);
int sq_check_histogram(SqCall &c, size_t n_sums);
int sq_call_scales(SqCall &c, int32_t *scale_log2);
int sq_call_plan(SqCall &c);
// Q_dst[s] = the quantised frame frames[f0 + s] of the uploaded frame list, s < n
int sq_launch_quantize(SqCall &c, size_t f0, size_t n, uint4 *Q_dst);
// dst[s][d_order[..]][S][2] = rho of the coordinates src[s][N] (Q, or the self part's D), s < n, over the runs [r0, r0 + n_runs):
// Kc vectors, numbered by d_order.  *launches (optional) counts the launches
int sq_launch_rho(SqCall &c, const uint4 *src, size_t n, int r0, int n_runs, const int32_t *d_order, int Kc, double *dst,
                  int64_t *launches = nullptr);
// the quantiser's flag (complete on return: the stream is synchronised); timing_open: the call's timing ends before the error
int sq_fetch_flag(SqCall &c, bool timing_open = false);

// ---- the lag analyses: F(q, t) and C(q, t) ----
// A call keeps its own zeroed counters [counts | sum blocks .. | beyond] in either form: the host form fetches them, the
// device form adds them into the caller's at the end (so a call that fails leaves the caller's untouched).
struct LagCall : SqCall {
    const int32_t *windows = nullptr;
    int32_t W = 0;
    int64_t stride = 1;
    std::vector<LagRange> lagiv;        // this call's origin indices of every lag (the lag-major work list of amof_vanhove_distinct)
    int64_t n_entries = 0;              // (lag, origin) pairs of the work range
    size_t n_cnt = 0;                   // W nbins
    std::vector<double> scale2;         // [S][S] (sq_expand_pairs)
    std::vector<int32_t> sexp2;
    IsfFrames fr;
    IsfChunks ch;
    LagPass pass;
    int i_olocal = -1, i_slot = -1, i_win = -1, i_iv = -1;
    unsigned long long *cnt = nullptr, *sums = nullptr, *bey = nullptr;     // SLOT_OUT1
    StageSpans spans;
    LagCall(amof_ctx *ctx_, const amof_traj *t_, const double *recip_, const int32_t *hkl_, int32_t K_, double dq_, int32_t nbins_)
        : SqCall(ctx_, t_, recip_, hkl_, K_, dq_, nbins_), spans(ctx_) {}
};

// One block of fixed-point sums, in the order of the call's counters: [S][S][W][nbins] (exponent sexp2[a S + c]), or the
// diagonal [S][W][nbins] (sexp2[a S + a]).  The caller's destination: f64, overwritten (host form), or int64, added into.
struct LagSums {
    int64_t *out_dev;
    double *out_host;
    bool diagonal;
};
struct LagOutputs : SqCounters {
    std::vector<LagSums> blocks;
    size_t words(const LagCall &c, const LagSums &b) const { return (size_t)(b.diagonal ? c.S : c.S * c.S) * c.n_cnt; }
    size_t sum_words(const LagCall &c) const
    {
        size_t n = 0;
        for (const LagSums &b : blocks) n += words(c, b);
        return n;
    }
};

// what both correlation kernels take
struct LagArgs {
    const double *tab;          // [slots][Kc][S][2] (rho) or [slots][Kc][S][6] (j)
    const int32_t *slot_of;     // [F]: slot of a frame in Q and the table (-1: not touched)
    const int32_t *vec;         // [Kc]: the caller's index of the chunk's vectors
    const int32_t *hkl;         // [K][3]
    const double *recip;        // [n_cells][9]
    const double *scale2;       // [S][S]: 2^s of the unordered pair {a, c}
    const int32_t *windows;     // [W]
    const int2 *lagiv;          // [W]: origin indices [x, y) of lag w in this call's work range
    unsigned long long *counts, *sum0, *sum1, *beyond;      // sum0: coh or long; sum1: trans
    int64_t n_cells, stride;
    int32_t Kc, S, W, nbins, omin, omax, opw, lags_per_pass;
    double dq;
};

// sq_check_traj and the other arguments, the lag arguments in their place among them
int lag_check(LagCall &c);
// the work range [wb, we) of the lag-major work list: lagiv, n_entries, n_cnt
int lag_work(LagCall &c, int64_t wb, int64_t we);
// the host form's arrays, zeroed
void lag_zero_host(const LagCall &c, const LagOutputs &out);
// The four tables of a lag call behind whatever the analysis added to c.pk, sq_stage for the touched frames (a table of
// rho_bytes), and the call's counters, zeroed, with room for out's sum blocks (out = NULL: none, the modes call)
int lag_stage(LagCall &c, size_t rho_bytes, const LagOutputs *out);
// every field but the chunk's (Kc, vec, opw)
LagArgs lag_kernel_args(const LagCall &c, const double *d_scale2, unsigned long long *sum0, unsigned long long *sum1);
// device form: the call's counters into the caller's; host form: fetched and descaled.  Closes the call's timing.
int lag_finish(LagCall &c, const LagOutputs &out);

// Family::kernel<ST, GLOBAL>(): the correlation kernel for ST species in registers (0: any number) and its counters in
// LDS tiles or global memory
template <typename Family>
hipError_t lag_launch_corr(amof_ctx *ctx, const LagArgs &a, dim3 grid, const LagPass &pass)
{
    return with_flag(pass.global, [&](auto G) {
        return with_value<1, 2, 3, 4, 0>(a.S, [&](auto ST) {
            static_assert(LAG_SMAX == 4, "the register forms");
            auto kern = Family::template kernel<ST(), G()>();
            if (!G()) {
                hipError_t e = allow_max_lds((const void *)kern);
                if (e != hipSuccess) return e;
            }
            hipLaunchKernelGGL(kern, grid, dim3(LAG_THREADS), G() ? 0 : pass.lds, ctx->stream, a);
            return hipGetLastError();
        });
    });
}

// Per chunk of vectors: fill(chunk, &launches) makes its table for every touched frame (span span_fill), launch(args, grid)
// correlates it over all lags (span span_corr); tile: the origin tile of the kernel's grid rule
template <typename Fill, typename Launch>
int lag_chunk_loop(LagCall &c, LagArgs a, int tile, int span_fill, int span_corr, Fill fill, Launch launch)
{
    amof_ctx *ctx = c.ctx;
    timing_dom_begin(ctx, c.pass.path);
    int64_t launches = 0;
    for (const IsfChunk &k : c.ch.chunks) {
        c.spans.begin(span_fill);
        AMOF_TRY(fill(k, &launches));
        c.spans.end();
        c.spans.begin(span_corr);
        const LagGrid g = lag_grid(k.nv, (int64_t)c.fr.omax - c.fr.omin, tile);
        a.Kc = k.nv;
        a.vec = c.pk.ptr<int32_t>(c.i_order) + k.v0;
        a.opw = g.opw;
        AMOF_HIP_TRY(ctx, launch(a, dim3((unsigned)g.vblocks, g.gy)));
        launches++;
        c.spans.end();
    }
    timing_dom_end(ctx, launches);
    return AMOF_OK;
}

}  // namespace amof
