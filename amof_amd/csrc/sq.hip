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
    const bool live = ri < n_runs;
    const SqRun run = runs[live ? ri : n_runs - 1];     // (idle lanes compute a copy of the last run and write nothing)
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
    // per-pair fixed-point scale 2^s: the sum over the trajectory's frames (ANY selection of them) of |t_ab| + 1/2 in one bin
    // stays below 2^62 -- |t_ab| <= N_a N_b, and a bin receives at most F * sq_bin_capacity samples.  The scale depends on
    // the trajectory's frame count and cells, the vectors, the bins and the species counts only: frame ranges of one
    // trajectory add up exactly.
    std::vector<int64_t> nsp(S, 0);
    for (int64_t i = 0; i < N; i++) nsp[t->species[i]]++;
    const int64_t cap = sq_bin_capacity(recip, t->n_cells, hkl, K, dq, nbins);
    std::vector<int32_t> sexp(P);
    std::vector<double> scale(P);
    {
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
    }
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
