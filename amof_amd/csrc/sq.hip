// Static structure factor S(q) by direct summation over reciprocal-lattice vectors (gfx950).
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
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "amof_internal.h"

namespace amof {
namespace {

constexpr int SQ_THREADS = 256;
constexpr int SQ_RUN = 16;                  // vectors per thread (registers: two f32 partials and two f64 sums each)
constexpr int SQ_BLOCK = 64;                // atoms per f32 partial
constexpr size_t SQ_LDS_BUDGET = 64 * 1024; // LDS counters of sq_bin_kernel (u64)
constexpr size_t SQ_RHO_BUDGET = (size_t)512 << 20;   // bytes of rho per batch of frames
constexpr int SQ_BIN_BLOCKS = 1024;         // workgroups of sq_bin_kernel (grid-stride over the samples)

struct SqRun {
    int32_t h, k, l0, n;    // vectors (h, k, l0 + r), r < n
    int32_t start;          // into order[]: the callers' indices of the run's vectors
    int32_t _pad[3];
};

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

// The largest number of vectors one bin can receive in one frame of ANY of the n_cells cells: every vector is counted in
// each bin its |q| can reach.  |q_c| lies within delta |hkl| of |hkl . Rm|, Rm the mean reciprocal matrix and delta the
// largest Frobenius norm of R_c - Rm (>= the spectral norm); a relative margin of 1e-9 covers the rounding of both.  One
// pass over the vectors (a difference array over the bins): for a constant cell this is the per-bin count itself, give or
// take a vector on a bin edge.
int64_t sq_bin_capacity(const double *recip, int64_t n_cells, const int32_t *hkl, int32_t K, double dq, int32_t nbins)
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

// Per-pair fixed-point scale 2^s: the sum over the trajectory's frames (ANY selection of them) of |t_ab| + 1/2 in one bin
// stays below 2^62 -- |t_ab| <= N_a N_b, and a bin receives at most F * sq_bin_capacity samples.  The scale depends on
// the trajectory's frame count and cells, the vectors, the bins and the species counts only: frame ranges of one
// trajectory add up exactly (and F(q, t) -- at most F samples of a vector per lag -- shares S(q)'s scale).
int sq_scales(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K, double dq, int32_t nbins,
              std::vector<int32_t> &sexp, std::vector<double> &scale)
{
    const int S = t->n_species, P = S * (S + 1) / 2;
    const int64_t N = t->n_atoms, F = t->n_frames;
    std::vector<int64_t> nsp(S, 0);
    for (int64_t i = 0; i < N; i++) nsp[t->species[i]]++;
    const int64_t cap = sq_bin_capacity(recip, t->n_cells, hkl, K, dq, nbins);
    sexp.assign(P, 0);
    scale.assign(P, 0.0);
    int p = 0;
    for (int a = 0; a < S; a++)
        for (int c = a; c < S; c++, p++) {
            const double bound = (double)std::max<int64_t>(F, 1) * (double)std::max<int64_t>(cap, 1) *
                                 ((double)std::max<int64_t>(nsp[a], 1) * (double)std::max<int64_t>(nsp[c], 1) + 0.5);
            int e;
            frexp(bound, &e);               // bound < 2^e
            sexp[p] = std::min(62 - e, 60);
            scale[p] = ldexp(1.0, sexp[p]);
            // the quantum 2^-s in S units (divided by sqrt(N_a N_b)) must not exceed 2^-20
            const double nab = sqrt((double)std::max<int64_t>(nsp[a], 1) * (double)std::max<int64_t>(nsp[c], 1));
            if (ldexp(1.0, -sexp[p]) / nab > ldexp(1.0, -20))
                return fail(ctx, AMOF_ECAPACITY, "S(q): %lld frames x %lld vectors per bin x %lld x %lld atoms exceed the "
                                                 "fixed-point range (quantum above 2^-20): use fewer frames per call, a "
                                                 "smaller dq or fewer vectors per bin (max_points)",
                            (long long)F, (long long)cap, (long long)nsp[a], (long long)nsp[c]);
        }
    return AMOF_OK;
}

struct SqPlan {
    std::vector<int32_t> perm;          // atoms in species order (stable)
    std::vector<int64_t> sp_first;      // [S + 1]
    std::vector<SqRun> runs;
    std::vector<int32_t> order;         // [K]: the callers' index of every sorted vector
};

int sq_plan(amof_ctx *ctx, const amof_traj *t, const int32_t *hkl, int32_t K, SqPlan &pl)
{
    const int S = t->n_species;
    const int64_t N = t->n_atoms;
    pl.sp_first.assign(S + 1, 0);
    for (int64_t i = 0; i < N; i++) pl.sp_first[t->species[i] + 1]++;
    for (int s = 0; s < S; s++) pl.sp_first[s + 1] += pl.sp_first[s];
    pl.perm.resize(N);
    std::vector<int64_t> cur(pl.sp_first.begin(), pl.sp_first.end() - 1);
    for (int64_t i = 0; i < N; i++) pl.perm[cur[t->species[i]]++] = (int32_t)i;
    for (int32_t m = 0; m < K; m++)
        if (hkl[3 * m] == 0 && hkl[3 * m + 1] == 0 && hkl[3 * m + 2] == 0)
            return fail(ctx, AMOF_EINVAL, "hkl %d is (0, 0, 0)", m);
    // rows of consecutive l at fixed (h, k), cut into runs of at most SQ_RUN
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
    return AMOF_OK;
}

int sq_check_traj(amof_ctx *ctx, const amof_traj *t, const int32_t *hkl, int32_t K)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    if (!t->pbc[0] || !t->pbc[1] || !t->pbc[2]) return fail(ctx, AMOF_EINVAL, "S(q) needs a cell periodic on all three axes");
    if (K < 0 || (K > 0 && !hkl)) return fail(ctx, AMOF_EINVAL, "bad hkl list");
    if (t->n_atoms > 0 && !t->species) return fail(ctx, AMOF_EINVAL, "NULL species");
    return AMOF_OK;
}

// rho of the frames fsel[f0 .. f0 + nb) into d_rho [nb][K][S][2]
int sq_rho_batch(amof_ctx *ctx, const amof_traj *t, const double *pos_dev, const double *d_geom, const int32_t *d_perm,
                 const int64_t *d_spfirst, const SqRun *d_runs, int n_runs, const int32_t *d_order, int K,
                 const int32_t *d_frames, int nb, uint4 *d_Q, int32_t *d_flag, double *d_rho)
{
    const int64_t N = t->n_atoms;
    if (N > 0)
        hipLaunchKernelGGL(sq_quantize_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream, pos_dev,
                       d_geom, t->n_cells, d_perm, N, d_frames, d_Q, d_flag);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(sq_rho_kernel, dim3((unsigned)((n_runs + SQ_THREADS - 1) / SQ_THREADS), (unsigned)nb), dim3(SQ_THREADS), 0,
                       ctx->stream, (const uint4 *)d_Q, N, d_spfirst, t->n_species, d_runs, n_runs, d_order, K, d_rho);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    return AMOF_OK;
}

// host outputs (counts, sums: f64, beyond -- overwritten) or device outputs (counts_dev, sums_dev: int64 fixed point,
// beyond_dev -- added into; scale_log2 receives the pairs' exponents)
int sq_run(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K, int64_t frame_begin,
           int64_t frame_end, int64_t frame_stride, double dq, int32_t nbins, uint64_t *counts, double *sums, uint64_t *beyond,
           uint64_t *counts_dev, int64_t *sums_dev, uint64_t *beyond_dev, int32_t *scale_log2)
{
    AMOF_TRY(sq_check_traj(ctx, t, hkl, K));
    const int S = t->n_species, P = S * (S + 1) / 2;
    const int64_t N = t->n_atoms, F = t->n_frames;
    if (!recip && t->n_cells > 0) return fail(ctx, AMOF_EINVAL, "NULL recip");
    if (frame_stride < 1 || frame_begin < 0 || frame_end > F || frame_begin > frame_end)
        return fail(ctx, AMOF_EINVAL, "bad frame range");
    if (!(dq > 0.0) || !isfinite(dq)) return fail(ctx, AMOF_EINVAL, "dq must be positive and finite");
    if (nbins < 1) return fail(ctx, AMOF_EINVAL, "nbins must be >= 1");
    for (int64_t c = 0; c < 9 * t->n_cells; c++)
        if (!isfinite(recip[c])) return fail(ctx, AMOF_EINVAL, "recip is not finite");
    if ((size_t)(P + 1) * (size_t)nbins > ((size_t)1 << 36)) return fail(ctx, AMOF_EINVAL, "histogram too large");
    std::vector<int32_t> sexp;
    std::vector<double> scale;
    AMOF_TRY(sq_scales(ctx, t, recip, hkl, K, dq, nbins, sexp, scale));
    if (scale_log2) std::copy(sexp.begin(), sexp.end(), scale_log2);
    if (counts) {
        std::fill(counts, counts + nbins, (uint64_t)0);
        std::fill(sums, sums + (size_t)P * nbins, 0.0);
        *beyond = 0;
    }
    std::vector<int32_t> fsel;
    for (int64_t f = frame_begin; f < frame_end; f += frame_stride) fsel.push_back((int32_t)f);
    if (fsel.empty() || K == 0) return AMOF_OK;

    HostGeom hg;
    AMOF_TRY(build_geometry(ctx, t, hg));
    SqPlan pl;
    AMOF_TRY(sq_plan(ctx, t, hkl, K, pl));
    const size_t rho_frame = (size_t)K * S * 2 * sizeof(double);
    const int nb_max = (int)std::max<size_t>(1, std::min<size_t>({SQ_RHO_BUDGET / rho_frame, fsel.size(), (size_t)65535}));
    const size_t n_ctr = (size_t)(P + 1) * nbins + 1;
    const bool global = n_ctr * sizeof(uint64_t) > SQ_LDS_BUDGET || getenv("AMOF_SQ_GLOBAL");

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(hg.rec.data(), hg.rec.size() * sizeof(double));
    const int i_perm = pk.add(pl.perm.data(), pl.perm.size() * sizeof(int32_t));
    const int i_spf = pk.add(pl.sp_first.data(), pl.sp_first.size() * sizeof(int64_t));
    const int i_runs = pk.add(pl.runs.data(), pl.runs.size() * sizeof(SqRun));
    const int i_order = pk.add(pl.order.data(), pl.order.size() * sizeof(int32_t));
    const int i_hkl = pk.add(hkl, (size_t)K * 3 * sizeof(int32_t));
    const int i_recip = pk.add(recip, (size_t)t->n_cells * 9 * sizeof(double));
    const int i_frames = pk.add(fsel.data(), fsel.size() * sizeof(int32_t));
    const int i_scale = pk.add(scale.data(), scale.size() * sizeof(double));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    void *d_Q = nullptr, *d_rho = nullptr, *d_flag = nullptr, *d_ctr = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, (size_t)nb_max * std::max<int64_t>(N, 1) * sizeof(uint4), &d_Q));
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)nb_max * rho_frame, &d_rho));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts_dev);
    unsigned long long *sm = reinterpret_cast<unsigned long long *>(sums_dev);
    unsigned long long *bey = reinterpret_cast<unsigned long long *>(beyond_dev);
    if (counts) {       // host call: the counters start from zero in scratch
        AMOF_TRY(ensure(ctx, SLOT_OUT1, n_ctr * sizeof(uint64_t), &d_ctr));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, n_ctr * sizeof(uint64_t), ctx->stream));
        cnt = (unsigned long long *)d_ctr;
        sm = cnt + nbins;
        bey = sm + (size_t)P * nbins;
    }
    if (!global) AMOF_HIP_TRY(ctx, allow_max_lds((const void *)sq_bin_kernel<false>));
    const int n_runs = (int)pl.runs.size();
    timing_dom_begin(ctx, global ? "sq_bin_global" : "sq");
    int64_t launches = 0;
    for (size_t f0 = 0; f0 < fsel.size(); f0 += nb_max) {
        const int nb = (int)std::min<size_t>(nb_max, fsel.size() - f0);
        const int32_t *d_frames = pk.ptr<int32_t>(i_frames) + f0;
        AMOF_TRY(sq_rho_batch(ctx, t, pos_dev, pk.ptr<double>(i_geom), pk.ptr<int32_t>(i_perm), pk.ptr<int64_t>(i_spf),
                              pk.ptr<SqRun>(i_runs), n_runs, pk.ptr<int32_t>(i_order), K, d_frames, nb, (uint4 *)d_Q,
                              (int32_t *)d_flag, (double *)d_rho));
        const int64_t samples = (int64_t)nb * K;
        const unsigned blocks = (unsigned)std::min<int64_t>(SQ_BIN_BLOCKS, (samples + SQ_THREADS - 1) / SQ_THREADS);
        if (global)
            hipLaunchKernelGGL(sq_bin_kernel<true>, dim3(blocks), dim3(SQ_THREADS), 0, ctx->stream, (const double *)d_rho, nb, K, S,
                               pk.ptr<int32_t>(i_hkl), pk.ptr<double>(i_recip), t->n_cells, d_frames, dq, (int)nbins,
                               pk.ptr<double>(i_scale), cnt, sm, bey);
        else
            hipLaunchKernelGGL(sq_bin_kernel<false>, dim3(blocks), dim3(SQ_THREADS), n_ctr * sizeof(uint64_t), ctx->stream,
                               (const double *)d_rho, nb, K, S, pk.ptr<int32_t>(i_hkl), pk.ptr<double>(i_recip), t->n_cells,
                               d_frames, dq, (int)nbins, pk.ptr<double>(i_scale), cnt, sm, bey);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        launches += 3;
    }
    timing_dom_end(ctx, launches);
    timing_end(ctx);
    int32_t flag = 0;
    AMOF_TRY(fetch(ctx, &flag, d_flag, sizeof(int32_t)));
    if (flag) return fail(ctx, AMOF_EINVAL, "positions lie more than 10^4 cells from the cell, or are not finite");
    if (counts) {
        std::vector<int64_t> raw((size_t)P * nbins);
        AMOF_TRY(fetch(ctx, counts, cnt, (size_t)nbins * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, raw.data(), sm, raw.size() * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, beyond, bey, sizeof(uint64_t)));
        for (int p = 0; p < P; p++)
            for (int b = 0; b < nbins; b++) sums[(size_t)p * nbins + b] = ldexp((double)raw[(size_t)p * nbins + b], -sexp[p]);
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}

// ------------------------------------------------------------------------------------------------ F(q, t) --
// Intermediate scattering function: the time correlation of the rho table (amof_isf_accumulate[_dev]).
//
// Data path, per call:
//   pos --sq_quantize_kernel--> Q[slots][N]: every frame the work range touches, quantised ONCE
//   per chunk of K_c vectors (whole runs of the sorted list; the table [slots][K_c][S][2] f64 stays inside the budget):
//     Q --sq_rho_kernel--> rho[slot][v][s][2]                    (the kernel and atom order of amof_sq_modes: same bits)
//     rho --isf_corr_kernel--> counts[W][nbins], coh[S][S][W][nbins] (int64 fixed point, S(q)'s scales), beyond[W]
//   self part, per batch of (lag, origin) entries:
//     Q --isf_diff_kernel--> D[e][N] = Q[k + m] - Q[k] (u32 wrap-around: the exact phase of the displacement)
//     D --sq_rho_kernel--> rho_d[e][K][S][2];  Re rho_d --isf_self_bin_kernel--> self[S][W][nbins]
//
// isf_corr_kernel: a lane owns a vector of the chunk (consecutive lanes: consecutive 16 S-byte records of one frame's row),
// a workgroup a range of origin indices.  Origins are taken ISF_TILE at a time: their rows rho(k) and their bins are loaded
// into registers once and serve every lag of the pass; per lag the S^2 products of the tile's origins are rounded to int64
// and summed in registers while the bin stays the same (always, for a constant cell), then added with one atomic per
// (lane, lag, pair) and tile -- into per-lag LDS counter tiles ((1 + S^2) nbins u64 each; as many lags per pass as fit
// ISF_LDS_BUDGET, flushed to global memory after each pass) or straight into global memory ("isf_global").  S > ISF_SMAX
// takes a generic form of the same kernel (one atomic per sample, rows re-read through the caches).
constexpr int ISF_THREADS = 256;
constexpr int ISF_TILE = 4;                 // origins whose rows a lane holds in registers
constexpr int ISF_SMAX = 4;                 // species counts with a register form
constexpr int ISF_OPW = 64;                 // at most this many origins per workgroup
constexpr size_t ISF_LDS_BUDGET = 64 * 1024;
// rho table of one vector chunk: 1 GiB, twice S(q)'s batch.  The table is streamed (1 + W) times whatever its size, but a
// thread of sq_rho_kernel owns a run of up to 16 vectors and a chunk is cut to whole waves of runs: on the headline shape
// (5000 frames, 4 species: 320 KB per vector) 512 MB hold ~126 runs -- one whole wave, 13 launches with a tail each, the
// table 14 % slower than S(q)'s -- where 1 GiB holds three.  Next to Q (16 N bytes per frame) a rank's scratch stays near
// 2 GB there.  AMOF_ISF_RHO_BUDGET (bytes) overrides it (tests: several chunks on a small case).
constexpr size_t ISF_RHO_BUDGET = (size_t)1 << 30;

struct IsfEntry {
    int32_t w, k;           // lag index, origin frame
    int32_t sk, skm;        // slots of frames k and k + m in Q
};

struct IsfArgs {
    const double *rho;          // [slots][Kc][S][2]
    const int32_t *slot_of;     // [F]: slot of a frame in Q / rho (-1: not touched)
    const int32_t *vec;         // [Kc]: the caller's index of the chunk's vectors
    const int32_t *hkl;         // [K][3]
    const double *recip;        // [n_cells][9]
    const double *scale2;       // [S][S]: 2^s of the unordered pair {a, c}
    const int32_t *windows;     // [W]
    const int2 *lagiv;          // [W]: origin indices [x, y) of lag w in this call's work range
    unsigned long long *counts, *coh, *beyond;
    int64_t n_cells, stride;
    int32_t Kc, S, W, nbins, omin, omax, opw, lags_per_pass;
    double dq;
};

// the bin of amof_sq_accumulate (f64, no fma), -1 = beyond
__device__ __forceinline__ int isf_bin(const double *__restrict__ R, const int32_t *__restrict__ v, double dq, int nbins)
{
    const double h = (double)v[0], k = (double)v[1], l = (double)v[2];
    const double qx = (h * R[0] + k * R[3]) + l * R[6];
    const double qy = (h * R[1] + k * R[4]) + l * R[7];
    const double qz = (h * R[2] + k * R[5]) + l * R[8];
    const double qq = sqrt((qx * qx + qy * qy) + qz * qz) / dq;
    if (!(qq < (double)nbins)) return -1;
    return (int)qq;
}

template <int ST, bool GLOBAL>
__global__ __launch_bounds__(ISF_THREADS) void isf_corr_kernel(IsfArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long *lc = reinterpret_cast<unsigned long long *>(lds_raw);
    const int tid = threadIdx.x;
    const int S = ST ? ST : a.S;
    constexpr int SR = ST ? ST : 1;
    const int W = a.W, nbins = a.nbins, Kc = a.Kc;
    const int v = blockIdx.x * ISF_THREADS + tid;
    const bool live = v < Kc;
    const int ob = a.omin + (int)blockIdx.y * a.opw, oe = min(ob + a.opw, a.omax);
    const int tile = (1 + S * S) * nbins;
    const int L = GLOBAL ? W : a.lags_per_pass;
    const size_t row = (size_t)S * 2;
    const int32_t *hv = a.hkl + 3 * (size_t)a.vec[live ? v : 0];

    for (int w0 = 0; w0 < W; w0 += L) {
        const int w1 = min(w0 + L, W);
        if (!GLOBAL) {
            for (int i = tid; i < (w1 - w0) * tile; i += ISF_THREADS) lc[i] = 0ull;
            __syncthreads();
        }
        if (live) {
            for (int os = ob; os < oe; os += ISF_TILE) {
                // the tile's origin rows and bins: loaded once, used by every lag of the pass
                int bins[ISF_TILE];
                const double *orow[ISF_TILE];
                double ore[ISF_TILE][SR], oim[ISF_TILE][SR];
#pragma unroll
                for (int t = 0; t < ISF_TILE; t++) {
                    bins[t] = -1;
                    orow[t] = a.rho;
                    if (os + t < oe) {
                        const int64_t k = 1 + a.stride * (int64_t)(os + t);
                        bins[t] = isf_bin(a.recip + (a.n_cells == 1 ? 0 : (size_t)k * 9), hv, a.dq, nbins);
                        orow[t] = a.rho + ((size_t)a.slot_of[k] * Kc + v) * row;
                        if (ST) {
#pragma unroll
                            for (int s = 0; s < SR; s++) { ore[t][s] = orow[t][2 * s]; oim[t][s] = orow[t][2 * s + 1]; }
                        }
                    }
                }
                for (int w = w0; w < w1; w++) {
                    const int2 iv = a.lagiv[w];
                    const int lo = max(os, iv.x), hi = min(min(os + ISF_TILE, oe), iv.y);
                    if (lo >= hi) continue;
                    const int64_t m = a.windows[w];
                    unsigned long long *cw = GLOBAL ? a.counts + (size_t)w * nbins : lc + (size_t)(w - w0) * tile;
                    // coh of (a, c): cg + (a S + c) cstep
                    unsigned long long *cg = GLOBAL ? a.coh + (size_t)w * nbins : cw + nbins;
                    const size_t cstep = GLOBAL ? (size_t)W * nbins : (size_t)nbins;
                    unsigned long long nbey = 0;
                    if (ST) {
                        unsigned long long acc[SR * SR], cnt = 0;
                        int cur = -1;
#pragma unroll
                        for (int i = 0; i < SR * SR; i++) acc[i] = 0ull;
                        auto flush = [&]() {
                            if (!cnt) return;
                            atomicAdd(&cw[cur], cnt);
#pragma unroll
                            for (int i = 0; i < SR * SR; i++) {
                                if (acc[i]) atomicAdd(&cg[(size_t)i * cstep + cur], acc[i]);
                                acc[i] = 0ull;
                            }
                            cnt = 0;
                        };
#pragma unroll
                        for (int t = 0; t < ISF_TILE; t++) {
                            const int o = os + t;
                            if (o < lo || o >= hi) continue;
                            if (bins[t] < 0) { nbey++; continue; }
                            if (bins[t] != cur) { flush(); cur = bins[t]; }
                            const int64_t km = 1 + a.stride * (int64_t)o + m;
                            const double *__restrict__ pr = a.rho + ((size_t)a.slot_of[km] * Kc + v) * row;
                            double pre[SR], pim[SR];
#pragma unroll
                            for (int s = 0; s < SR; s++) { pre[s] = pr[2 * s]; pim[s] = pr[2 * s + 1]; }
                            cnt++;
#pragma unroll
                            for (int x = 0; x < SR; x++)
#pragma unroll
                                for (int c = 0; c < SR; c++) {
                                    const double tt = ore[t][x] * pre[c] + oim[t][x] * pim[c];
                                    acc[x * SR + c] += (unsigned long long)(long long)rint(tt * a.scale2[x * SR + c]);
                                }
                        }
                        flush();
                    } else {
#pragma unroll
                        for (int t = 0; t < ISF_TILE; t++) {
                            const int o = os + t;
                            if (o < lo || o >= hi) continue;
                            const int bin = bins[t];
                            if (bin < 0) { nbey++; continue; }
                            const int64_t km = 1 + a.stride * (int64_t)o + m;
                            const double *__restrict__ po = orow[t];
                            const double *__restrict__ pr = a.rho + ((size_t)a.slot_of[km] * Kc + v) * row;
                            atomicAdd(&cw[bin], 1ull);
                            for (int x = 0; x < S; x++) {
                                const double ra = po[2 * x], ia = po[2 * x + 1];
                                for (int c = 0; c < S; c++) {
                                    const double tt = ra * pr[2 * c] + ia * pr[2 * c + 1];
                                    atomicAdd(&cg[(size_t)(x * S + c) * cstep + bin],
                                              (unsigned long long)(long long)rint(tt * a.scale2[x * S + c]));
                                }
                            }
                        }
                    }
                    if (nbey) atomicAdd(&a.beyond[w], nbey);
                }
            }
        }
        if (!GLOBAL) {
            __syncthreads();
            for (int i = tid; i < (w1 - w0) * tile; i += ISF_THREADS) {
                const unsigned long long val = lc[i];
                if (!val) continue;
                const int w = w0 + i / tile, r = i % tile, j = r / nbins, b = r % nbins;
                atomicAdd(j == 0 ? &a.counts[(size_t)w * nbins + b] : &a.coh[((size_t)(j - 1) * W + w) * nbins + b], val);
            }
            __syncthreads();
        }
    }
}

// D[e][i] = Q[slot of k + m][i] - Q[slot of k][i], component by component in u32 wrap-around arithmetic
__global__ __launch_bounds__(256) void isf_diff_kernel(const uint4 *__restrict__ Q, int64_t N, const IsfEntry *__restrict__ ent,
                                                       uint4 *__restrict__ D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const IsfEntry e = ent[blockIdx.y];
    const uint4 q0 = Q[(size_t)e.sk * N + i], q1 = Q[(size_t)e.skm * N + i];
    D[(size_t)blockIdx.y * N + i] = make_uint4(q1.x - q0.x, q1.y - q0.y, q1.z - q0.z, 0u);
}

// self[a][w][bin] += rint(Re rho_d_a 2^s_aa): one (entry, vector) sample per thread, bin from the origin frame
__global__ __launch_bounds__(SQ_THREADS) void isf_self_bin_kernel(const double *__restrict__ rho, int nb, int K, int S, int W,
                                                                  const IsfEntry *__restrict__ ent, const int32_t *__restrict__ hkl,
                                                                  const double *__restrict__ recip, int64_t n_cells, double dq,
                                                                  int nbins, const double *__restrict__ scale2,
                                                                  unsigned long long *__restrict__ selfs)
{
    const int64_t total = (int64_t)nb * K;
    for (int64_t it = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x; it < total; it += (int64_t)gridDim.x * SQ_THREADS) {
        const int b = (int)(it / K), m = (int)(it % K);
        const IsfEntry e = ent[b];
        const int bin = isf_bin(recip + (n_cells == 1 ? 0 : (size_t)e.k * 9), hkl + 3 * (size_t)m, dq, nbins);
        if (bin < 0) continue;      // (counted in beyond by the coherent part)
        const double *r = rho + (size_t)it * S * 2;
        for (int s = 0; s < S; s++)
            atomicAdd(&selfs[((size_t)s * W + e.w) * nbins + bin],
                      (unsigned long long)(long long)rint(r[2 * s] * scale2[s * S + s]));
    }
}

template <bool GLOBAL>
hipError_t isf_launch_corr(amof_ctx *ctx, const IsfArgs &a, dim3 grid, size_t lds)
{
    auto go = [&](auto kern) -> hipError_t {
        if (!GLOBAL) {
            hipError_t e = allow_max_lds((const void *)kern);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(ISF_THREADS), GLOBAL ? 0 : lds, ctx->stream, a);
        return hipGetLastError();
    };
    switch (a.S <= ISF_SMAX ? a.S : 0) {
    case 1: return go(isf_corr_kernel<1, GLOBAL>);
    case 2: return go(isf_corr_kernel<2, GLOBAL>);
    case 3: return go(isf_corr_kernel<3, GLOBAL>);
    case 4: return go(isf_corr_kernel<4, GLOBAL>);
    default: return go(isf_corr_kernel<0, GLOBAL>);
    }
}

// host outputs (counts, coh, selfs: f64, beyond -- overwritten) or device outputs (int64 fixed point / u64, added into;
// scale_log2 receives the pairs' exponents).  want_self: the self part is computed (selfs / self_dev given)
int isf_run(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K, const int32_t *windows,
            int32_t W, int64_t stride, int64_t wb, int64_t we, double dq, int32_t nbins, bool want_self, uint64_t *counts,
            double *coh, double *selfs, uint64_t *beyond, uint64_t *counts_dev, int64_t *coh_dev, int64_t *self_dev,
            uint64_t *beyond_dev, int32_t *scale_log2)
{
    AMOF_TRY(sq_check_traj(ctx, t, hkl, K));
    const int S = t->n_species, P = S * (S + 1) / 2;
    const int64_t N = t->n_atoms, F = t->n_frames;
    if (!recip && t->n_cells > 0) return fail(ctx, AMOF_EINVAL, "NULL recip");
    AMOF_TRY(check_lag_args(ctx, windows, W, F, stride));
    if (!(dq > 0.0) || !isfinite(dq)) return fail(ctx, AMOF_EINVAL, "dq must be positive and finite");
    if (nbins < 1) return fail(ctx, AMOF_EINVAL, "nbins must be >= 1");
    if (F > 0x7fffffffLL || N > 0x7fffffffLL) return fail(ctx, AMOF_EINVAL, "too many frames or atoms");
    for (int64_t c = 0; c < 9 * t->n_cells; c++)
        if (!isfinite(recip[c])) return fail(ctx, AMOF_EINVAL, "recip is not finite");
    // this call's origin indices [o0, o1) of every lag (the lag-major work list of amof_vanhove_distinct)
    static_assert(sizeof(LagRange) == sizeof(int2), "the kernels read the table as int2");
    std::vector<LagRange> lagiv(std::max(W, 1), LagRange{0, 0});
    const int64_t total = lag_work_ranges(windows, W, F, stride, wb, we, lagiv.data());
    int64_t n_entries = 0;
    for (int w = 0; w < W; w++) n_entries += lagiv[w].o1 - lagiv[w].o0;
    if (wb < 0 || we > total || wb > we) return fail(ctx, AMOF_EINVAL, "work range [%lld, %lld) outside [0, %lld)", (long long)wb,
                                                     (long long)we, (long long)total);
    const size_t n_cnt = (size_t)W * nbins, n_coh = (size_t)S * S * n_cnt, n_self = want_self ? (size_t)S * n_cnt : 0;
    if (n_coh > ((size_t)1 << 36)) return fail(ctx, AMOF_EINVAL, "histogram too large");
    std::vector<int32_t> sexp;
    std::vector<double> scale;
    AMOF_TRY(sq_scales(ctx, t, recip, hkl, K, dq, nbins, sexp, scale));
    if (scale_log2) std::copy(sexp.begin(), sexp.end(), scale_log2);
    std::vector<double> scale2((size_t)S * S);
    std::vector<int32_t> sexp2((size_t)S * S);
    {
        int p = 0;
        for (int a = 0; a < S; a++)
            for (int c = a; c < S; c++, p++) {
                scale2[a * S + c] = scale2[c * S + a] = scale[p];
                sexp2[a * S + c] = sexp2[c * S + a] = sexp[p];
            }
    }
    if (counts) {
        std::fill(counts, counts + n_cnt, (uint64_t)0);
        std::fill(coh, coh + n_coh, 0.0);
        if (selfs) std::fill(selfs, selfs + n_self, 0.0);
        std::fill(beyond, beyond + W, (uint64_t)0);
    }
    if (n_entries == 0 || K == 0) return AMOF_OK;

    // the frames the range touches, ascending: slot s of Q and of the rho table holds frame fsel[s]
    std::vector<int32_t> slot_of(F, -1), fsel;
    int omin = 0x7fffffff, omax = 0;
    for (int w = 0; w < W; w++) {
        if (lagiv[w].o0 >= lagiv[w].o1) continue;
        omin = std::min(omin, lagiv[w].o0);
        omax = std::max(omax, lagiv[w].o1);
        for (int64_t o = lagiv[w].o0; o < lagiv[w].o1; o++) {
            const int64_t k = lag_origin_frame(o, stride);
            slot_of[k] = 0;
            slot_of[k + windows[w]] = 0;
        }
    }
    for (int64_t f = 0; f < F; f++)
        if (slot_of[f] == 0) {
            slot_of[f] = (int32_t)fsel.size();
            fsel.push_back((int32_t)f);
        }
    const size_t slots = fsel.size();

    HostGeom hg;
    AMOF_TRY(build_geometry(ctx, t, hg));
    SqPlan pl;
    AMOF_TRY(sq_plan(ctx, t, hkl, K, pl));
    // vector chunks: whole runs of the sorted list, at most kc_max vectors (at least one run)
    size_t budget = ISF_RHO_BUDGET;
    if (const char *e = getenv("AMOF_ISF_RHO_BUDGET")) {
        const long long b = atoll(e);
        if (b > 0) budget = (size_t)b;
    }
    const size_t vec_bytes = slots * (size_t)S * 2 * sizeof(double);
    const size_t kc_max = std::max<size_t>(1, budget / vec_bytes);
    struct Chunk { int r0, r1, v0, nv; };
    std::vector<Chunk> chunks;
    std::vector<int32_t> order_local(K);
    const int n_runs_all = (int)pl.runs.size();
    for (int r0 = 0; r0 < n_runs_all;) {
        int r1 = r0, nv = 0;
        while (r1 < n_runs_all && (r1 == r0 || (size_t)(nv + pl.runs[r1].n) <= kc_max)) nv += pl.runs[r1++].n;
        // a thread of sq_rho_kernel owns a run: whole waves of runs, so that a chunk leaves no lane of its last wave idle
        if (r1 < n_runs_all && r1 - r0 > 64)
            while ((r1 - r0) % 64) nv -= pl.runs[--r1].n;
        chunks.push_back(Chunk{r0, r1, pl.runs[r0].start, nv});
        for (int i = 0; i < nv; i++) order_local[pl.runs[r0].start + i] = i;
        r0 = r1;
    }
    int kc_top = 0;
    for (const Chunk &c : chunks) kc_top = std::max(kc_top, c.nv);

    const size_t tile_ctr = (size_t)(1 + S * S) * nbins;
    const bool global = tile_ctr * sizeof(uint64_t) > ISF_LDS_BUDGET || getenv("AMOF_ISF_GLOBAL");
    const int lags_per_pass = global ? W : (int)std::min<size_t>(W, ISF_LDS_BUDGET / (tile_ctr * sizeof(uint64_t)));

    std::vector<IsfEntry> entries;
    if (want_self) {
        entries.reserve(n_entries);
        for (int w = 0; w < W; w++)
            for (int64_t o = lagiv[w].o0; o < lagiv[w].o1; o++) {
                const int64_t k = lag_origin_frame(o, stride);
                entries.push_back(IsfEntry{w, (int32_t)k, slot_of[k], slot_of[k + windows[w]]});
            }
    }

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    StageSpans spans(ctx);      // rho table (with the quantisation), correlation, self
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(hg.rec.data(), hg.rec.size() * sizeof(double));
    const int i_perm = pk.add(pl.perm.data(), pl.perm.size() * sizeof(int32_t));
    const int i_spf = pk.add(pl.sp_first.data(), pl.sp_first.size() * sizeof(int64_t));
    const int i_runs = pk.add(pl.runs.data(), pl.runs.size() * sizeof(SqRun));
    const int i_order = pk.add(pl.order.data(), pl.order.size() * sizeof(int32_t));
    const int i_olocal = pk.add(order_local.data(), order_local.size() * sizeof(int32_t));
    const int i_hkl = pk.add(hkl, (size_t)K * 3 * sizeof(int32_t));
    const int i_recip = pk.add(recip, (size_t)t->n_cells * 9 * sizeof(double));
    const int i_frames = pk.add(fsel.data(), fsel.size() * sizeof(int32_t));
    const int i_slot = pk.add(slot_of.data(), slot_of.size() * sizeof(int32_t));
    const int i_scale2 = pk.add(scale2.data(), scale2.size() * sizeof(double));
    const int i_win = pk.add(windows, (size_t)W * sizeof(int32_t));
    const int i_iv = pk.add(lagiv.data(), lagiv.size() * sizeof(LagRange));
    const int i_ent = pk.add(entries.data(), entries.size() * sizeof(IsfEntry));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    void *d_Q = nullptr, *d_rho = nullptr, *d_flag = nullptr, *d_ctr = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, slots * (size_t)std::max<int64_t>(N, 1) * sizeof(uint4), &d_Q));
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)kc_top * vec_bytes, &d_rho));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
    // the call's own counters, zeroed: [counts | coh | self | beyond]; the device form adds them into the caller's at the end
    const size_t n_ctr = n_cnt + n_coh + n_self + (size_t)W;
    AMOF_TRY(ensure(ctx, SLOT_OUT1, n_ctr * sizeof(uint64_t), &d_ctr));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, n_ctr * sizeof(uint64_t), ctx->stream));
    unsigned long long *cnt = (unsigned long long *)d_ctr, *co = cnt + n_cnt, *se = co + n_coh, *bey = se + n_self;

    // every touched frame is quantised once
    spans.begin(0);
    if (N > 0)
        for (size_t s0 = 0; s0 < slots; s0 += 65535) {
            const unsigned nb = (unsigned)std::min<size_t>(65535, slots - s0);
            hipLaunchKernelGGL(sq_quantize_kernel, dim3((unsigned)((N + 255) / 256), nb), dim3(256), 0, ctx->stream, pos_dev,
                               pk.ptr<double>(i_geom), t->n_cells, pk.ptr<int32_t>(i_perm), N, pk.ptr<int32_t>(i_frames) + s0,
                               (uint4 *)d_Q + s0 * (size_t)N, (int32_t *)d_flag);
            AMOF_HIP_TRY(ctx, hipGetLastError());
        }
    spans.end();

    IsfArgs a;
    memset(&a, 0, sizeof a);
    a.rho = (const double *)d_rho;
    a.slot_of = pk.ptr<int32_t>(i_slot);
    a.hkl = pk.ptr<int32_t>(i_hkl);
    a.recip = pk.ptr<double>(i_recip);
    a.scale2 = pk.ptr<double>(i_scale2);
    a.windows = pk.ptr<int32_t>(i_win);
    a.lagiv = pk.ptr<int2>(i_iv);
    a.counts = cnt;
    a.coh = co;
    a.beyond = bey;
    a.n_cells = t->n_cells;
    a.stride = stride;
    a.S = S;
    a.W = W;
    a.nbins = nbins;
    a.omin = omin;
    a.omax = omax;
    a.lags_per_pass = lags_per_pass;
    a.dq = dq;
    const size_t lds = (size_t)lags_per_pass * tile_ctr * sizeof(uint64_t);

    timing_dom_begin(ctx, global ? "isf_global" : "isf");
    int64_t launches = 0;
    for (const Chunk &c : chunks) {
        spans.begin(0);
        const int n_runs = c.r1 - c.r0;
        for (size_t s0 = 0; s0 < slots; s0 += 65535) {
            const unsigned nb = (unsigned)std::min<size_t>(65535, slots - s0);
            hipLaunchKernelGGL(sq_rho_kernel, dim3((unsigned)((n_runs + SQ_THREADS - 1) / SQ_THREADS), nb), dim3(SQ_THREADS), 0,
                               ctx->stream, (const uint4 *)d_Q + s0 * (size_t)N, N, pk.ptr<int64_t>(i_spf), S,
                               pk.ptr<SqRun>(i_runs) + c.r0, n_runs, pk.ptr<int32_t>(i_olocal), c.nv,
                               (double *)d_rho + s0 * (size_t)c.nv * S * 2);
            AMOF_HIP_TRY(ctx, hipGetLastError());
            launches++;
        }
        spans.end();
        spans.begin(1);
        a.Kc = c.nv;
        a.vec = pk.ptr<int32_t>(i_order) + c.v0;
        const int vblocks = (c.nv + ISF_THREADS - 1) / ISF_THREADS;
        const int64_t range = (int64_t)omax - omin;
        // origins per workgroup: a multiple of the tile, enough workgroups to fill the GPU several times over
        int64_t opw = std::min<int64_t>(ISF_OPW, std::max<int64_t>(ISF_TILE, range * vblocks / 2048 / ISF_TILE * ISF_TILE));
        opw = std::max<int64_t>(opw, ((range + 65534) / 65535 + ISF_TILE - 1) / ISF_TILE * ISF_TILE);
        a.opw = (int32_t)opw;
        const dim3 grid((unsigned)vblocks, (unsigned)((range + opw - 1) / opw));
        AMOF_HIP_TRY(ctx, global ? isf_launch_corr<true>(ctx, a, grid, 0) : isf_launch_corr<false>(ctx, a, grid, lds));
        launches++;
        spans.end();
    }
    timing_dom_end(ctx, launches);

    if (want_self) {
        // batches of entries inside the same budget: D (16 N bytes) and rho_d (16 K S bytes) per entry
        const size_t ent_bytes = (size_t)std::max<int64_t>(N, 1) * sizeof(uint4) + (size_t)K * S * 2 * sizeof(double);
        const size_t nb_max = std::max<size_t>(1, std::min<size_t>({budget / ent_bytes, entries.size(), (size_t)65535}));
        void *d_D = nullptr, *d_rd = nullptr;
        AMOF_TRY(ensure(ctx, SLOT_AUX2, nb_max * (size_t)std::max<int64_t>(N, 1) * sizeof(uint4), &d_D));
        AMOF_TRY(ensure(ctx, SLOT_AUX3, nb_max * (size_t)K * S * 2 * sizeof(double), &d_rd));
        const int n_runs = (int)pl.runs.size();
        spans.begin(2);
        for (size_t e0 = 0; e0 < entries.size(); e0 += nb_max) {
            const int nb = (int)std::min<size_t>(nb_max, entries.size() - e0);
            const IsfEntry *d_ent = pk.ptr<IsfEntry>(i_ent) + e0;
            if (N > 0)
                hipLaunchKernelGGL(isf_diff_kernel, dim3((unsigned)((N + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream,
                                   (const uint4 *)d_Q, N, d_ent, (uint4 *)d_D);
            AMOF_HIP_TRY(ctx, hipGetLastError());
            hipLaunchKernelGGL(sq_rho_kernel, dim3((unsigned)((n_runs + SQ_THREADS - 1) / SQ_THREADS), (unsigned)nb), dim3(SQ_THREADS),
                               0, ctx->stream, (const uint4 *)d_D, N, pk.ptr<int64_t>(i_spf), S, pk.ptr<SqRun>(i_runs), n_runs,
                               pk.ptr<int32_t>(i_order), K, (double *)d_rd);
            AMOF_HIP_TRY(ctx, hipGetLastError());
            const int64_t samples = (int64_t)nb * K;
            const unsigned blocks = (unsigned)std::min<int64_t>(SQ_BIN_BLOCKS, (samples + SQ_THREADS - 1) / SQ_THREADS);
            hipLaunchKernelGGL(isf_self_bin_kernel, dim3(blocks), dim3(SQ_THREADS), 0, ctx->stream, (const double *)d_rd, nb, K, S, W,
                               d_ent, pk.ptr<int32_t>(i_hkl), pk.ptr<double>(i_recip), t->n_cells, dq, (int)nbins,
                               pk.ptr<double>(i_scale2), se);
            AMOF_HIP_TRY(ctx, hipGetLastError());
        }
        spans.end();
    }
    int32_t flag = 0;
    AMOF_TRY(fetch(ctx, &flag, d_flag, sizeof(int32_t)));
    if (flag) {
        timing_end(ctx);
        return fail(ctx, AMOF_EINVAL, "positions lie more than 10^4 cells from the cell, or are not finite");
    }
    if (counts_dev) {
        // (the fixed-point sums are int64: two's complement, the same addition)
        AMOF_TRY(add_into(ctx, counts_dev, (const uint64_t *)cnt, n_cnt));
        AMOF_TRY(add_into(ctx, (uint64_t *)coh_dev, (const uint64_t *)co, n_coh));
        if (want_self) AMOF_TRY(add_into(ctx, (uint64_t *)self_dev, (const uint64_t *)se, n_self));
        AMOF_TRY(add_into(ctx, beyond_dev, (const uint64_t *)bey, (size_t)W));
    }
    timing_end(ctx);
    if (counts) {
        std::vector<int64_t> raw(n_coh + n_self);
        AMOF_TRY(fetch(ctx, counts, cnt, n_cnt * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, raw.data(), co, raw.size() * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, beyond, bey, (size_t)W * sizeof(uint64_t)));
        for (int x = 0; x < S * S; x++)
            for (size_t i = 0; i < n_cnt; i++) coh[(size_t)x * n_cnt + i] = ldexp((double)raw[(size_t)x * n_cnt + i], -sexp2[x]);
        if (want_self)
            for (int s = 0; s < S; s++)
                for (size_t i = 0; i < n_cnt; i++)
                    selfs[(size_t)s * n_cnt + i] = ldexp((double)raw[n_coh + (size_t)s * n_cnt + i], -sexp2[s * S + s]);
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    (void)P;
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_sq_accumulate(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                  int64_t frame_begin, int64_t frame_end, int64_t frame_stride, double dq, int32_t nbins,
                                  uint64_t *counts, double *sums, uint64_t *beyond)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !sums || !beyond) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return sq_run(ctx, t, recip, hkl, K, frame_begin, frame_end, frame_stride, dq, nbins, counts, sums, beyond, nullptr, nullptr,
                  nullptr, nullptr);
}

extern "C" int amof_sq_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                      int64_t frame_begin, int64_t frame_end, int64_t frame_stride, double dq, int32_t nbins,
                                      uint64_t *counts_dev, int64_t *sums_dev, uint64_t *beyond_dev, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !sums_dev || !beyond_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return sq_run(ctx, t, recip, hkl, K, frame_begin, frame_end, frame_stride, dq, nbins, nullptr, nullptr, nullptr, counts_dev,
                  sums_dev, beyond_dev, scale_log2);
}

extern "C" int amof_sq_modes(amof_ctx *ctx, const amof_traj *t, int64_t frame, const int32_t *hkl, int32_t K, double *rho)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(sq_check_traj(ctx, t, hkl, K));
    if (!rho && K > 0) return fail(ctx, AMOF_EINVAL, "NULL argument");
    if (frame < 0 || frame >= t->n_frames) return fail(ctx, AMOF_EINVAL, "frame out of range");
    const int S = t->n_species;
    const int64_t N = t->n_atoms;
    if (K == 0) return AMOF_OK;
    SqPlan pl;
    AMOF_TRY(sq_plan(ctx, t, hkl, K, pl));
    if (N == 0) {
        std::fill(rho, rho + (size_t)K * S * 2, 0.0);
        return AMOF_OK;
    }
    HostGeom hg;
    AMOF_TRY(build_geometry(ctx, t, hg));
    const int32_t fr = (int32_t)frame;
    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(hg.rec.data(), hg.rec.size() * sizeof(double));
    const int i_perm = pk.add(pl.perm.data(), pl.perm.size() * sizeof(int32_t));
    const int i_spf = pk.add(pl.sp_first.data(), pl.sp_first.size() * sizeof(int64_t));
    const int i_runs = pk.add(pl.runs.data(), pl.runs.size() * sizeof(SqRun));
    const int i_order = pk.add(pl.order.data(), pl.order.size() * sizeof(int32_t));
    const int i_frames = pk.add(&fr, sizeof(int32_t));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    void *d_Q = nullptr, *d_rho = nullptr, *d_flag = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, (size_t)N * sizeof(uint4), &d_Q));
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)K * S * 2 * sizeof(double), &d_rho));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
    timing_dom_begin(ctx, "sq_modes");
    AMOF_TRY(sq_rho_batch(ctx, t, pos_dev, pk.ptr<double>(i_geom), pk.ptr<int32_t>(i_perm), pk.ptr<int64_t>(i_spf),
                          pk.ptr<SqRun>(i_runs), (int)pl.runs.size(), pk.ptr<int32_t>(i_order), K, pk.ptr<int32_t>(i_frames), 1,
                          (uint4 *)d_Q, (int32_t *)d_flag, (double *)d_rho));
    timing_dom_end(ctx, 2);
    timing_end(ctx);
    int32_t flag = 0;
    AMOF_TRY(fetch(ctx, &flag, d_flag, sizeof(int32_t)));
    if (flag) return fail(ctx, AMOF_EINVAL, "positions lie more than 10^4 cells from the cell, or are not finite");
    AMOF_TRY(fetch(ctx, rho, d_rho, (size_t)K * S * 2 * sizeof(double)));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}

extern "C" int amof_isf_accumulate(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                   const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                                   int64_t work_end, double dq, int32_t nbins, uint64_t *counts, double *coh, double *self_sums,
                                   uint64_t *beyond)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !coh || !beyond) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return isf_run(ctx, t, recip, hkl, K, windows, n_windows, origin_stride, work_begin, work_end, dq, nbins, self_sums != nullptr,
                   counts, coh, self_sums, beyond, nullptr, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int amof_isf_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                       const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                                       int64_t work_end, double dq, int32_t nbins, uint64_t *counts_dev, int64_t *coh_dev,
                                       int64_t *self_dev, uint64_t *beyond_dev, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !coh_dev || !beyond_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return isf_run(ctx, t, recip, hkl, K, windows, n_windows, origin_stride, work_begin, work_end, dq, nbins, self_dev != nullptr,
                   nullptr, nullptr, nullptr, nullptr, counts_dev, coh_dev, self_dev, beyond_dev, scale_log2);
}
