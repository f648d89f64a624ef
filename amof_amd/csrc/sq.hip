// Static structure factor S(q) by direct summation over reciprocal-lattice vectors (gfx950), and the host helpers F(q, t)
// (isf.hip) and the current correlations (current.hip) share with it (sq_call.h).
//
// Data path, per batch of selected frames:
//   pos --sq_quantize_kernel--> Q[nb][N] (quantize_atom's u32 fractional coordinates, species-permutation order)
//   Q --sq_rho_kernel--> rho[nb][K][S][2] (f64): rho_a(k) = sum over the atoms j of species a of exp(2 pi i phi_j / 2^32),
//                         phi_j = h ux_j + k uy_j + l uz_j (mod 2^32, u32 arithmetic: the exact phase)
//   rho --sq_bin_kernel--> counts[nbins], sums[P][nbins] (int64 fixed point), beyond      (amof_sq_accumulate[_dev])
//   rho -> host                                                                             (amof_sq_modes)
//
// sq_rho_kernel: a thread owns a RUN of up to SQ_RUN vectors (h, k, l0 + r) of one row; the host cuts the rows of the sorted
// hkl list into runs.  Per atom the thread forms phi0 = h ux + k uy + l0 uz once (three integer multiplies), and every
// further vector of the run costs one u32 add (phi += uz).  The atom's coordinates are the same for every lane of the
// wave: scalar loads from Q, no LDS and no atom tiles, for any N.  Per vector and atom: add, convert, scale,
// v_cos_f32 / v_sin_f32 (input in revolutions: (float)(int32)phi * 2^-32 in [-1/2, 1/2)), two f32 adds.  The f32 partials
// cover at most SQ_BLOCK atoms and are folded into f64, in a fixed order: two identical calls give identical bits.
//
// sq_bin_kernel: one (frame, vector) sample per thread.  q and its bin from the frame's reciprocal matrix in float64 with no
// fma; t_ab = Re rho_a Re rho_b + Im rho_a Im rho_b is rounded to int64 at the pair's scale 2^s_ab (chosen by the host so
// that no counter can overflow) and added with integer atomics -- LDS counters flushed to u64, or straight into global
// memory (sq_bin_global) when (P + 1) nbins counters do not fit the LDS budget, or on request (AMOF_SQ_GLOBAL=1).  Integer
// sums are independent of the order of the atomics, of the batching and of how frames are split across ranks.
//
// The rules behind every launch -- the constants, the species and hkl orders and the runs, the fixed-point scales, batches,
// chunks, grids and LDS sizes -- are sq_plan.h's (host only, pinned by tests/test_sq_plan_cpu.py); the host code, after the
// kernels, checks, stages, launches and fetches: one call record, one stage function each.  The quantiser and sq_rho_kernel
// also serve F(q, t), through sq_launch_quantize and sq_launch_rho; the last section is the scaffold of the two lag
// analyses (LagCall: work range, staging, kernel arguments, finish).
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "sq_call.h"

namespace amof {
namespace {

// Q[b][i] = quantize_atom of atom perm[i] of frame frames[b] (components in cell-vector order)
__global__ __launch_bounds__(256) void sq_quantize_kernel(const double *__restrict__ pos, const double *__restrict__ geom,
                                                          int64_t n_cells, const int32_t *__restrict__ perm, int64_t N,
                                                          const int32_t *__restrict__ frames, uint4 *__restrict__ Q,
                                                          int32_t *__restrict__ flag)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int f = frames[blockIdx.y];
    const double *g = geom + (size_t)(n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    const QAtom q = quantize_atom(pos, g, N, f, perm[i], 0, 1, 2, flag);
    Q[(size_t)blockIdx.y * N + i] = make_uint4(q.ux, q.uy, q.uz, 0u);
}

// rho[b][order[run.start + r]][s][0 / 1] = Re / Im rho_s(h, k, l0 + r) of frame b of the batch
__global__ __launch_bounds__(SQ_THREADS) void sq_rho_kernel(const uint4 *__restrict__ Q, int64_t N,
                                                            const int64_t *__restrict__ sp_first, int S,
                                                            const SqRun *__restrict__ runs, int n_runs,
                                                            const int32_t *__restrict__ order, int K,
                                                            double *__restrict__ rho)
{
    const int ri = blockIdx.x * SQ_THREADS + threadIdx.x;
    if (blockIdx.x * SQ_THREADS + (int)(threadIdx.x & ~63u) >= n_runs) return;     // a wave without a live lane (no barrier below)
    const bool live = ri < n_runs;
    const SqRun run = runs[live ? ri : n_runs - 1];     // (idle lanes of a live wave compute a copy of the last run and write nothing)
    const uint4 *__restrict__ q = Q + (size_t)blockIdx.y * N;
    double *__restrict__ out = rho + (size_t)blockIdx.y * K * S * 2;
    const uint32_t h = (uint32_t)run.h, k = (uint32_t)run.k, l0 = (uint32_t)run.l0;
    const float rev = 2.3283064365386963e-10f;         // 2^-32
    for (int s = 0; s < S; s++) {
        const int64_t a0 = sp_first[s], a1 = sp_first[s + 1];
        double re[SQ_RUN], im[SQ_RUN];
#pragma unroll
        for (int r = 0; r < SQ_RUN; r++) { re[r] = 0.0; im[r] = 0.0; }
        for (int64_t b0 = a0; b0 < a1; b0 += SQ_BLOCK) {
            const int64_t b1 = min(b0 + (int64_t)SQ_BLOCK, a1);
            float pr[SQ_RUN], pi[SQ_RUN];
#pragma unroll
            for (int r = 0; r < SQ_RUN; r++) { pr[r] = 0.0f; pi[r] = 0.0f; }
            for (int64_t j = b0; j < b1; j++) {        // j < sp_first[S] = N: no load past the frame
                const uint4 u = q[j];
                uint32_t phi = h * u.x + k * u.y + l0 * u.z;
#pragma unroll
                for (int r = 0; r < SQ_RUN; r++) {
                    const float x = (float)(int32_t)phi * rev;
                    pr[r] += __builtin_amdgcn_cosf(x);
                    pi[r] += __builtin_amdgcn_sinf(x);
                    phi += u.z;
                }
            }
#pragma unroll
            for (int r = 0; r < SQ_RUN; r++) { re[r] += (double)pr[r]; im[r] += (double)pi[r]; }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < SQ_RUN; r++) {
                if (r < run.n) {
                    double *o = out + ((size_t)order[run.start + r] * S + s) * 2;
                    o[0] = re[r];
                    o[1] = im[r];
                }
            }
        }
    }
}

// counters: [0][nbins] sample counts, [1 + p][nbins] fixed-point sums of pair p, then beyond (one word)
template <bool GLOBAL>
__global__ __launch_bounds__(SQ_THREADS) void sq_bin_kernel(const double *__restrict__ rho, int nb, int K, int S,
                                                            const int32_t *__restrict__ hkl, const double *__restrict__ recip,
                                                            int64_t n_cells, const int32_t *__restrict__ frames, double dq,
                                                            int nbins, const double *__restrict__ scale,
                                                            unsigned long long *__restrict__ counts,
                                                            unsigned long long *__restrict__ sums,
                                                            unsigned long long *__restrict__ beyond)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long *lc = reinterpret_cast<unsigned long long *>(lds_raw);
    const int P = S * (S + 1) / 2;
    const int n_ctr = (P + 1) * nbins + 1;
    if (!GLOBAL) {
        for (int i = threadIdx.x; i < n_ctr; i += SQ_THREADS) lc[i] = 0ull;
        __syncthreads();
    }
    const int64_t total = (int64_t)nb * K;
    const double fnb = (double)nbins;
    for (int64_t it = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x; it < total; it += (int64_t)gridDim.x * SQ_THREADS) {
        const int b = (int)(it / K), m = (int)(it % K);
        const double *R = recip + (size_t)(n_cells == 1 ? 0 : frames[b]) * 9;
        const double h = (double)hkl[3 * m], k = (double)hkl[3 * m + 1], l = (double)hkl[3 * m + 2];
        const double qx = (h * R[0] + k * R[3]) + l * R[6];
        const double qy = (h * R[1] + k * R[4]) + l * R[7];
        const double qz = (h * R[2] + k * R[5]) + l * R[8];
        const double qq = sqrt((qx * qx + qy * qy) + qz * qz) / dq;
        if (!(qq < fnb)) {          // (b >= nbins without converting a huge quotient)
            if (GLOBAL) atomicAdd(beyond, 1ull);
            else atomicAdd(&lc[n_ctr - 1], 1ull);
            continue;
        }
        const int bin = (int)qq;
        const double *r = rho + (size_t)it * S * 2;
        if (GLOBAL) atomicAdd(&counts[bin], 1ull);
        else atomicAdd(&lc[bin], 1ull);
        int p = 0;
        for (int a = 0; a < S; a++) {
            const double ra = r[2 * a], ia = r[2 * a + 1];
            for (int c = a; c < S; c++, p++) {
                const double t = ra * r[2 * c] + ia * r[2 * c + 1];
                const unsigned long long v = (unsigned long long)(long long)rint(t * scale[p]);
                if (GLOBAL) atomicAdd(&sums[(size_t)p * nbins + bin], v);
                else atomicAdd(&lc[(size_t)(p + 1) * nbins + bin], v);
            }
        }
    }
    if (!GLOBAL) {
        __syncthreads();
        for (int i = threadIdx.x; i < n_ctr; i += SQ_THREADS) {
            const unsigned long long v = lc[i];
            if (!v) continue;
            unsigned long long *dst = i == n_ctr - 1 ? beyond : (i < nbins ? counts + i : sums + (i - nbins));
            atomicAdd(dst, v);
        }
    }
}

// The arguments of amof_sq_accumulate[_dev] and of the lag analyses; range_check: the form's own frame or lag arguments, in
// their place among the others
template <typename RangeCheck>
int sq_check(SqCall &c, bool lag, RangeCheck range_check)
{
    AMOF_TRY(sq_check_traj(c));
    if (!c.recip && c.t->n_cells > 0) return fail(c.ctx, AMOF_EINVAL, "NULL recip");
    AMOF_TRY(range_check());
    if (!(c.dq > 0.0) || !isfinite(c.dq)) return fail(c.ctx, AMOF_EINVAL, "dq must be positive and finite");
    if (c.nbins < 1) return fail(c.ctx, AMOF_EINVAL, "nbins must be >= 1");
    if (lag && (c.F > 0x7fffffffLL || c.N > 0x7fffffffLL)) return fail(c.ctx, AMOF_EINVAL, "too many frames or atoms");
    for (int64_t i = 0; i < 9 * c.t->n_cells; i++)
        if (!isfinite(c.recip[i])) return fail(c.ctx, AMOF_EINVAL, "recip is not finite");
    return AMOF_OK;
}

// S(q)'s arrays beside the counters: sums f64 (host form) or int64 fixed point (device form)
struct SqOutputs : SqCounters {
    double *sums = nullptr;
    int64_t *sums_dev = nullptr;
};

}  // namespace

// --------------------------------------------------------------------------------------------- host code --
int sq_check_traj(SqCall &c)
{
    const amof_traj *t = c.t;
    AMOF_TRY(validate_traj(c.ctx, t, false));
    if (!t->pbc[0] || !t->pbc[1] || !t->pbc[2]) return fail(c.ctx, AMOF_EINVAL, "S(q) needs a cell periodic on all three axes");
    if (c.K < 0 || (c.K > 0 && !c.hkl)) return fail(c.ctx, AMOF_EINVAL, "bad hkl list");
    if (t->n_atoms > 0 && !t->species) return fail(c.ctx, AMOF_EINVAL, "NULL species");
    c.S = t->n_species;
    c.P = c.S * (c.S + 1) / 2;
    c.N = t->n_atoms;
    c.F = t->n_frames;
    return AMOF_OK;
}

int sq_check_histogram(SqCall &c, size_t n_sums)
{
    return n_sums > ((size_t)1 << 36) ? fail(c.ctx, AMOF_EINVAL, "histogram too large") : AMOF_OK;
}

int sq_call_scales(SqCall &c, int32_t *scale_log2)
{
    if (sq_scales(c.t->species, c.N, c.S, c.F, c.recip, c.t->n_cells, c.hkl, c.K, c.dq, c.nbins, c.sc) >= 0)
        return fail(c.ctx, AMOF_ECAPACITY, "S(q): %lld frames x %lld vectors per bin x %lld x %lld atoms exceed the "
                                           "fixed-point range (quantum above 2^-20): use fewer frames per call, a "
                                           "smaller dq or fewer vectors per bin (max_points)",
                    (long long)c.F, (long long)c.sc.cap, (long long)c.sc.nsp[c.sc.bad_a], (long long)c.sc.nsp[c.sc.bad_c]);
    if (scale_log2) std::copy(c.sc.sexp.begin(), c.sc.sexp.end(), scale_log2);
    return AMOF_OK;
}

int sq_call_plan(SqCall &c)
{
    sq_species_order(c.t->species, c.N, c.S, c.pl);
    const int32_t zero = sq_cut_runs(c.hkl, c.K, c.pl);
    return zero >= 0 ? fail(c.ctx, AMOF_EINVAL, "hkl %d is (0, 0, 0)", zero) : AMOF_OK;
}

// The two kernels below index the frame (slot, entry) by blockIdx.y, which ends at SQ_GRID_Y: the helpers cut a longer range
// into several launches.  S(q)'s batches and the self part's never need it (nb_max, isf_self_batch); F(q, t) quantises every
// touched frame and fills a chunk's table for all of them at once, and does.
int sq_launch_quantize(SqCall &c, size_t f0, size_t n, uint4 *Q_dst)
{
    if (c.N == 0) return AMOF_OK;
    for (size_t s0 = 0; s0 < n; s0 += SQ_GRID_Y) {
        const unsigned nb = (unsigned)std::min<size_t>(SQ_GRID_Y, n - s0);
        hipLaunchKernelGGL(sq_quantize_kernel, dim3((unsigned)((c.N + 255) / 256), nb), dim3(256), 0, c.ctx->stream, c.pos_dev,
                           c.pk.ptr<double>(c.i_geom), c.t->n_cells, c.pk.ptr<int32_t>(c.i_perm), c.N,
                           c.pk.ptr<int32_t>(c.i_frames) + f0 + s0, Q_dst + s0 * (size_t)c.N, c.d_flag);
        AMOF_HIP_TRY(c.ctx, hipGetLastError());
    }
    return AMOF_OK;
}

int sq_launch_rho(SqCall &c, const uint4 *src, size_t n, int r0, int n_runs, const int32_t *d_order, int Kc, double *dst,
                  int64_t *launches)
{
    for (size_t s0 = 0; s0 < n; s0 += SQ_GRID_Y) {
        const unsigned nb = (unsigned)std::min<size_t>(SQ_GRID_Y, n - s0);
        hipLaunchKernelGGL(sq_rho_kernel, dim3((unsigned)((n_runs + SQ_THREADS - 1) / SQ_THREADS), nb), dim3(SQ_THREADS), 0,
                           c.ctx->stream, src + s0 * (size_t)c.N, c.N, c.pk.ptr<int64_t>(c.i_spf), c.S, c.pk.ptr<SqRun>(c.i_runs) + r0,
                           n_runs, d_order, Kc, dst + s0 * (size_t)Kc * c.S * 2);
        AMOF_HIP_TRY(c.ctx, hipGetLastError());
        if (launches) ++*launches;
    }
    return AMOF_OK;
}

int sq_fetch_flag(SqCall &c, bool timing_open)
{
    int32_t flag = 0;
    AMOF_TRY(fetch(c.ctx, &flag, c.d_flag, sizeof(int32_t)));
    if (!flag) return AMOF_OK;
    if (timing_open) timing_end(c.ctx);
    return fail(c.ctx, AMOF_EINVAL, "positions lie more than 10^4 cells from the cell, or are not finite");
}

namespace {

// Positions, ONE upload of the plan's tables, the frame list and whatever the form added to c.pk, then the scratch every form
// has: Q for q_frames frames, the rho table, the flag (zeroed).  Opens the call's timing.
int sq_stage(SqCall &c, const int32_t *frames, size_t n_frames, size_t q_frames, size_t rho_bytes)
{
    amof_ctx *ctx = c.ctx;
    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    AMOF_TRY(stage_positions(ctx, c.t, &c.pos_dev));
    UploadPack &pk = c.pk;
    c.i_geom = pk.add(c.hg.rec.data(), c.hg.rec.size() * sizeof(double));
    c.i_perm = pk.add(c.pl.perm.data(), c.pl.perm.size() * sizeof(int32_t));
    c.i_spf = pk.add(c.pl.sp_first.data(), c.pl.sp_first.size() * sizeof(int64_t));
    c.i_runs = pk.add(c.pl.runs.data(), c.pl.runs.size() * sizeof(SqRun));
    c.i_order = pk.add(c.pl.order.data(), c.pl.order.size() * sizeof(int32_t));
    if (c.recip) {
        c.i_hkl = pk.add(c.hkl, (size_t)c.K * 3 * sizeof(int32_t));
        c.i_recip = pk.add(c.recip, (size_t)c.t->n_cells * 9 * sizeof(double));
    }
    c.i_frames = pk.add(frames, n_frames * sizeof(int32_t));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    void *d_Q = nullptr, *d_rho = nullptr, *d_flag = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, q_frames * (size_t)std::max<int64_t>(c.N, 1) * sizeof(uint4), &d_Q));
    AMOF_TRY(ensure(ctx, SLOT_AUX1, rho_bytes, &d_rho));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
    c.d_Q = (uint4 *)d_Q;
    c.d_rho = (double *)d_rho;
    c.d_flag = (int32_t *)d_flag;
    return AMOF_OK;
}

// n_ctr zeroed u64 counters of the call's own (SLOT_OUT1)
int sq_zeroed_counters(amof_ctx *ctx, size_t n_ctr, unsigned long long **out)
{
    void *d_ctr = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_OUT1, n_ctr * sizeof(uint64_t), &d_ctr));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, n_ctr * sizeof(uint64_t), ctx->stream));
    *out = (unsigned long long *)d_ctr;
    return AMOF_OK;
}

// rho of the frames frames[f0 .. f0 + nb) of the frame list, every vector: Q and the rho table from their starts
int sq_rho_batch(SqCall &c, size_t f0, int nb)
{
    AMOF_TRY(sq_launch_quantize(c, f0, (size_t)nb, c.d_Q));
    return sq_launch_rho(c, c.d_Q, (size_t)nb, 0, (int)c.pl.runs.size(), c.pk.ptr<int32_t>(c.i_order), c.K, c.d_rho);
}

// fixed point to f64
void sq_descale(const int64_t *raw, size_t n, int32_t sexp, double *out)
{
    for (size_t i = 0; i < n; i++) out[i] = ldexp((double)raw[i], -sexp);
}

// ---- S(q) ----
// The host form counts in zeroed scratch and fetches; the device form adds straight into the caller's counters.
int sq_run(SqCall &c, int64_t frame_begin, int64_t frame_end, int64_t frame_stride, const SqOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    AMOF_TRY(sq_check(c, false, [&] {
        return frame_stride < 1 || frame_begin < 0 || frame_end > c.F || frame_begin > frame_end
                   ? fail(ctx, AMOF_EINVAL, "bad frame range") : AMOF_OK;
    }));
    const int P = c.P, nbins = c.nbins;
    AMOF_TRY(sq_check_histogram(c, (size_t)(P + 1) * (size_t)nbins));
    AMOF_TRY(sq_call_scales(c, out.scale_log2));
    if (out.host()) {
        std::fill(out.counts, out.counts + nbins, (uint64_t)0);
        std::fill(out.sums, out.sums + (size_t)P * nbins, 0.0);
        *out.beyond = 0;
    }
    std::vector<int32_t> fsel;
    for (int64_t f = frame_begin; f < frame_end; f += frame_stride) fsel.push_back((int32_t)f);
    if (fsel.empty() || c.K == 0) return AMOF_OK;

    AMOF_TRY(build_geometry(ctx, c.t, c.hg));
    AMOF_TRY(sq_call_plan(c));
    const SqBatchPlan bp = sq_batch_plan(c.K, c.S, nbins, fsel.size(), c.sw);
    const int i_scale = c.pk.add(c.sc.scale.data(), c.sc.scale.size() * sizeof(double));
    AMOF_TRY(sq_stage(c, fsel.data(), fsel.size(), (size_t)bp.nb_max, (size_t)bp.nb_max * bp.rho_frame));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(out.counts_dev);
    unsigned long long *sm = reinterpret_cast<unsigned long long *>(out.sums_dev);
    unsigned long long *bey = reinterpret_cast<unsigned long long *>(out.beyond_dev);
    if (out.host()) {
        AMOF_TRY(sq_zeroed_counters(ctx, bp.n_ctr, &cnt));
        sm = cnt + nbins;
        bey = sm + (size_t)P * nbins;
    }
    if (!bp.global) AMOF_HIP_TRY(ctx, allow_max_lds((const void *)sq_bin_kernel<false>));
    timing_dom_begin(ctx, bp.path);
    int64_t launches = 0;
    for (size_t f0 = 0; f0 < fsel.size(); f0 += bp.nb_max) {
        const int nb = (int)std::min<size_t>(bp.nb_max, fsel.size() - f0);
        AMOF_TRY(sq_rho_batch(c, f0, nb));
        AMOF_HIP_TRY(ctx, with_flag(bp.global, [&](auto G) {
            hipLaunchKernelGGL(sq_bin_kernel<G()>, dim3(sq_sample_blocks(nb, c.K)), dim3(SQ_THREADS), bp.lds, ctx->stream,
                               (const double *)c.d_rho, nb, c.K, c.S, c.pk.ptr<int32_t>(c.i_hkl), c.pk.ptr<double>(c.i_recip),
                               c.t->n_cells, c.pk.ptr<int32_t>(c.i_frames) + f0, c.dq, (int)nbins, c.pk.ptr<double>(i_scale), cnt, sm,
                               bey);
            return hipGetLastError();
        }));
        launches += 3;
    }
    timing_dom_end(ctx, launches);
    timing_end(ctx);
    AMOF_TRY(sq_fetch_flag(c));
    if (out.host()) {
        std::vector<int64_t> raw((size_t)P * nbins);
        AMOF_TRY(fetch(ctx, out.counts, cnt, (size_t)nbins * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, raw.data(), sm, raw.size() * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.beyond, bey, sizeof(uint64_t)));
        for (int p = 0; p < P; p++) sq_descale(raw.data() + (size_t)p * nbins, (size_t)nbins, c.sc.sexp[p], out.sums + (size_t)p * nbins);
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}

}  // namespace

// ------------------------------------------------------------------- the lag analyses: F(q, t) and C(q, t) --
int lag_check(LagCall &c)
{
    return sq_check(c, true, [&] { return check_lag_args(c.ctx, c.windows, c.W, c.F, c.stride); });
}

int lag_work(LagCall &c, int64_t wb, int64_t we)
{
    static_assert(sizeof(LagRange) == sizeof(int2), "the kernels read the table as int2");
    const int32_t W = c.W;
    c.lagiv.assign(std::max(W, 1), LagRange{0, 0});
    const int64_t total = lag_work_ranges(c.windows, W, c.F, c.stride, wb, we, c.lagiv.data());
    c.n_entries = 0;
    for (int w = 0; w < W; w++) c.n_entries += c.lagiv[w].o1 - c.lagiv[w].o0;
    if (wb < 0 || we > total || wb > we) return fail(c.ctx, AMOF_EINVAL, "work range [%lld, %lld) outside [0, %lld)", (long long)wb,
                                                     (long long)we, (long long)total);
    c.n_cnt = (size_t)W * c.nbins;
    return AMOF_OK;
}

void lag_zero_host(const LagCall &c, const LagOutputs &out)
{
    if (!out.host()) return;
    std::fill(out.counts, out.counts + c.n_cnt, (uint64_t)0);
    for (const LagSums &b : out.blocks) std::fill(b.out_host, b.out_host + out.words(c, b), 0.0);
    std::fill(out.beyond, out.beyond + c.W, (uint64_t)0);
}

int lag_stage(LagCall &c, size_t rho_bytes, const LagOutputs *out)
{
    UploadPack &pk = c.pk;
    c.i_olocal = pk.add(c.ch.order_local.data(), c.ch.order_local.size() * sizeof(int32_t));
    c.i_slot = pk.add(c.fr.slot_of.data(), c.fr.slot_of.size() * sizeof(int32_t));
    c.i_win = pk.add(c.windows, (size_t)c.W * sizeof(int32_t));
    c.i_iv = pk.add(c.lagiv.data(), c.lagiv.size() * sizeof(LagRange));
    const size_t slots = c.fr.fsel.size();
    AMOF_TRY(sq_stage(c, c.fr.fsel.data(), slots, slots, rho_bytes));
    if (out) {
        const size_t sum_words = out->sum_words(c);
        AMOF_TRY(sq_zeroed_counters(c.ctx, c.n_cnt + sum_words + (size_t)c.W, &c.cnt));
        c.sums = c.cnt + c.n_cnt;
        c.bey = c.sums + sum_words;
    }
    return AMOF_OK;
}

LagArgs lag_kernel_args(const LagCall &c, const double *d_scale2, unsigned long long *sum0, unsigned long long *sum1)
{
    const UploadPack &pk = c.pk;
    LagArgs a;
    memset(&a, 0, sizeof a);
    a.tab = c.d_rho;
    a.slot_of = pk.ptr<int32_t>(c.i_slot);
    a.hkl = pk.ptr<int32_t>(c.i_hkl);
    a.recip = pk.ptr<double>(c.i_recip);
    a.scale2 = d_scale2;
    a.windows = pk.ptr<int32_t>(c.i_win);
    a.lagiv = pk.ptr<int2>(c.i_iv);
    a.counts = c.cnt;
    a.sum0 = sum0;
    a.sum1 = sum1;
    a.beyond = c.bey;
    a.n_cells = c.t->n_cells;
    a.stride = c.stride;
    a.S = c.S;
    a.W = c.W;
    a.nbins = c.nbins;
    a.omin = c.fr.omin;
    a.omax = c.fr.omax;
    a.lags_per_pass = c.pass.lags_per_pass;
    a.dq = c.dq;
    return a;
}

int lag_finish(LagCall &c, const LagOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    if (!out.host()) {
        // (the fixed-point sums are int64: two's complement, the same addition)
        AMOF_TRY(add_into(ctx, out.counts_dev, (const uint64_t *)c.cnt, c.n_cnt));
        const unsigned long long *src = c.sums;
        for (const LagSums &b : out.blocks) {
            AMOF_TRY(add_into(ctx, (uint64_t *)b.out_dev, (const uint64_t *)src, out.words(c, b)));
            src += out.words(c, b);
        }
        AMOF_TRY(add_into(ctx, out.beyond_dev, (const uint64_t *)c.bey, (size_t)c.W));
    }
    timing_end(ctx);
    if (out.host()) {
        std::vector<int64_t> raw((size_t)(c.bey - c.sums));
        AMOF_TRY(fetch(ctx, out.counts, c.cnt, c.n_cnt * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, raw.data(), c.sums, raw.size() * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.beyond, c.bey, (size_t)c.W * sizeof(uint64_t)));
        const int64_t *src = raw.data();
        for (const LagSums &b : out.blocks) {
            const int rows = b.diagonal ? c.S : c.S * c.S;
            for (int x = 0; x < rows; x++)
                sq_descale(src + (size_t)x * c.n_cnt, c.n_cnt, c.sexp2[b.diagonal ? x * c.S + x : x], b.out_host + (size_t)x * c.n_cnt);
            src += out.words(c, b);
        }
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    c.spans.collect();
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

extern "C" int amof_sq_accumulate(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                  int64_t frame_begin, int64_t frame_end, int64_t frame_stride, double dq, int32_t nbins,
                                  uint64_t *counts, double *sums, uint64_t *beyond)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !sums || !beyond) return fail(ctx, AMOF_EINVAL, "NULL argument");
    SqCall c(ctx, t, recip, hkl, K, dq, nbins);
    SqOutputs out;
    out.counts = counts;
    out.sums = sums;
    out.beyond = beyond;
    return sq_run(c, frame_begin, frame_end, frame_stride, out);
}

extern "C" int amof_sq_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                      int64_t frame_begin, int64_t frame_end, int64_t frame_stride, double dq, int32_t nbins,
                                      uint64_t *counts_dev, int64_t *sums_dev, uint64_t *beyond_dev, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !sums_dev || !beyond_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "NULL argument");
    SqCall c(ctx, t, recip, hkl, K, dq, nbins);
    SqOutputs out;
    out.counts_dev = counts_dev;
    out.sums_dev = sums_dev;
    out.beyond_dev = beyond_dev;
    out.scale_log2 = scale_log2;
    return sq_run(c, frame_begin, frame_end, frame_stride, out);
}

extern "C" int amof_sq_modes(amof_ctx *ctx, const amof_traj *t, int64_t frame, const int32_t *hkl, int32_t K, double *rho)
{
    if (!ctx) return AMOF_EINVAL;
    SqCall c(ctx, t, nullptr, hkl, K, 0.0, 0);
    AMOF_TRY(sq_check_traj(c));
    if (!rho && K > 0) return fail(ctx, AMOF_EINVAL, "NULL argument");
    if (frame < 0 || frame >= c.F) return fail(ctx, AMOF_EINVAL, "frame out of range");
    if (K == 0) return AMOF_OK;
    AMOF_TRY(sq_call_plan(c));
    const size_t rho_bytes = (size_t)K * c.S * 2 * sizeof(double);
    if (c.N == 0) {
        std::fill(rho, rho + (size_t)K * c.S * 2, 0.0);
        return AMOF_OK;
    }
    AMOF_TRY(build_geometry(ctx, t, c.hg));
    const int32_t fr = (int32_t)frame;
    AMOF_TRY(sq_stage(c, &fr, 1, 1, rho_bytes));
    timing_dom_begin(ctx, "sq_modes");
    AMOF_TRY(sq_rho_batch(c, 0, 1));
    timing_dom_end(ctx, 2);
    timing_end(ctx);
    AMOF_TRY(sq_fetch_flag(c));
    AMOF_TRY(fetch(ctx, rho, c.d_rho, rho_bytes));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}
