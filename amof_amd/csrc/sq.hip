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
//
// The rules behind every launch -- the constants, the species and hkl orders and the runs, the fixed-point scales, batches,
// chunks, grids and LDS sizes -- are sq_plan.h's (host only, pinned by tests/test_sq_plan_cpu.py); the host code, after the
// kernels, checks, stages, launches and fetches: one call record, one stage function each.
//
// F(q, t) and the current correlation functions C_L(q, t), C_T(q, t) (a velocity per atom in the phase sum; rules in
// current_plan.h) follow further down, each under its own heading, on the same host helpers.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "current_plan.h"
#include "sq_plan.h"

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

// --------------------------------------------------------------------------------------------- host code --
// What every stage of a call needs, filled in this order: the arguments (the entry point), S .. F (sq_check_traj), the scales
// (sq_call_scales), the plan (build_geometry, sq_call_plan), the device side (sq_stage).
struct SqCall {
    amof_ctx *ctx;
    const amof_traj *t;
    const double *recip;        // [n_cells][9]; NULL in amof_sq_modes, which bins nothing
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

// The caller's arrays.  Host form: counts, sums (F(q, t): coh), selfs, beyond -- f64, overwritten.  Device form: int64 fixed
// point / u64, added into, and scale_log2 receives the pairs' exponents.  An entry point fills one of the two.
struct SqOutputs {
    uint64_t *counts = nullptr, *beyond = nullptr;
    double *sums = nullptr, *selfs = nullptr;
    uint64_t *counts_dev = nullptr, *beyond_dev = nullptr;
    int64_t *sums_dev = nullptr, *self_dev = nullptr;
    int32_t *scale_log2 = nullptr;
    bool host() const { return counts != nullptr; }
};

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

// The arguments of amof_sq_accumulate[_dev] and amof_isf_accumulate[_dev]; range_check: the form's own frame or lag arguments,
// in their place among the others
template <typename RangeCheck>
int sq_check(SqCall &c, bool isf, RangeCheck range_check)
{
    AMOF_TRY(sq_check_traj(c));
    if (!c.recip && c.t->n_cells > 0) return fail(c.ctx, AMOF_EINVAL, "NULL recip");
    AMOF_TRY(range_check());
    if (!(c.dq > 0.0) || !isfinite(c.dq)) return fail(c.ctx, AMOF_EINVAL, "dq must be positive and finite");
    if (c.nbins < 1) return fail(c.ctx, AMOF_EINVAL, "nbins must be >= 1");
    if (isf && (c.F > 0x7fffffffLL || c.N > 0x7fffffffLL)) return fail(c.ctx, AMOF_EINVAL, "too many frames or atoms");
    for (int64_t i = 0; i < 9 * c.t->n_cells; i++)
        if (!isfinite(c.recip[i])) return fail(c.ctx, AMOF_EINVAL, "recip is not finite");
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

// The two kernels below index the frame (slot, entry) by blockIdx.y, which ends at SQ_GRID_Y: the helpers cut a longer range
// into several launches.  S(q)'s batches and the self part's never need it (nb_max, isf_self_batch); F(q, t) quantises every
// touched frame and fills a chunk's table for all of them at once, and does.
// Q_dst[s] = the quantised frame frames[f0 + s] of the uploaded frame list, s < n
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

// dst[s][d_order[..]][S][2] = rho of the coordinates src[s][N] (Q, or the self part's D), s < n, over the runs [r0, r0 + n_runs):
// Kc vectors, numbered by d_order.  *launches (optional) counts the launches
int sq_launch_rho(SqCall &c, const uint4 *src, size_t n, int r0, int n_runs, const int32_t *d_order, int Kc, double *dst,
                  int64_t *launches = nullptr)
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

// rho of the frames frames[f0 .. f0 + nb) of the frame list, every vector: Q and the rho table from their starts
int sq_rho_batch(SqCall &c, size_t f0, int nb)
{
    AMOF_TRY(sq_launch_quantize(c, f0, (size_t)nb, c.d_Q));
    return sq_launch_rho(c, c.d_Q, (size_t)nb, 0, (int)c.pl.runs.size(), c.pk.ptr<int32_t>(c.i_order), c.K, c.d_rho);
}

// the quantiser's flag (complete on return: the stream is synchronised); timing_open: the call's timing ends before the error
int sq_fetch_flag(SqCall &c, bool timing_open = false)
{
    int32_t flag = 0;
    AMOF_TRY(fetch(c.ctx, &flag, c.d_flag, sizeof(int32_t)));
    if (!flag) return AMOF_OK;
    if (timing_open) timing_end(c.ctx);
    return fail(c.ctx, AMOF_EINVAL, "positions lie more than 10^4 cells from the cell, or are not finite");
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
        void *d_ctr = nullptr;
        AMOF_TRY(ensure(ctx, SLOT_OUT1, bp.n_ctr * sizeof(uint64_t), &d_ctr));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, bp.n_ctr * sizeof(uint64_t), ctx->stream));
        cnt = (unsigned long long *)d_ctr;
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

// ---- F(q, t) ----
// The call keeps its own zeroed counters [counts | coh | self | beyond] in either form: the host form fetches them, the device
// form adds them into the caller's at the end (so a call that fails leaves the caller's untouched).
struct IsfCall : SqCall {
    const int32_t *windows = nullptr;
    int32_t W = 0;
    int64_t stride = 1;
    bool want_self = false;     // the self part is computed (selfs / self_dev given)
    std::vector<LagRange> lagiv;        // this call's origin indices of every lag (the lag-major work list of amof_vanhove_distinct)
    size_t n_cnt = 0, n_coh = 0, n_self = 0;
    std::vector<double> scale2;
    std::vector<int32_t> sexp2;
    IsfFrames fr;
    IsfChunks ch;
    IsfPass pass;
    std::vector<IsfEntry> entries;
    int i_olocal = -1, i_slot = -1, i_scale2 = -1, i_win = -1, i_iv = -1, i_ent = -1;
    unsigned long long *cnt = nullptr, *co = nullptr, *se = nullptr, *bey = nullptr;
    StageSpans spans;           // rho table (with the quantisation), correlation, self
    IsfCall(amof_ctx *ctx_, const amof_traj *t_, const double *recip_, const int32_t *hkl_, int32_t K_, double dq_, int32_t nbins_)
        : SqCall(ctx_, t_, recip_, hkl_, K_, dq_, nbins_), spans(ctx_) {}
};

void isf_plan(IsfCall &c)
{
    isf_touched_frames(c.lagiv.data(), c.windows, c.W, c.F, c.stride, c.fr);
    isf_cut_chunks(c.pl.runs, c.K, c.fr.fsel.size(), c.S, c.sw.isf_rho_budget, c.ch);
    c.pass = isf_pass_plan(c.S, c.nbins, c.W, c.sw);
    if (c.want_self) isf_self_entries(c.lagiv.data(), c.windows, c.W, c.stride, c.fr, c.entries);
}

int isf_stage(IsfCall &c)
{
    amof_ctx *ctx = c.ctx;
    UploadPack &pk = c.pk;
    c.i_olocal = pk.add(c.ch.order_local.data(), c.ch.order_local.size() * sizeof(int32_t));
    c.i_slot = pk.add(c.fr.slot_of.data(), c.fr.slot_of.size() * sizeof(int32_t));
    c.i_scale2 = pk.add(c.scale2.data(), c.scale2.size() * sizeof(double));
    c.i_win = pk.add(c.windows, (size_t)c.W * sizeof(int32_t));
    c.i_iv = pk.add(c.lagiv.data(), c.lagiv.size() * sizeof(LagRange));
    c.i_ent = pk.add(c.entries.data(), c.entries.size() * sizeof(IsfEntry));
    const size_t slots = c.fr.fsel.size();
    AMOF_TRY(sq_stage(c, c.fr.fsel.data(), slots, slots, (size_t)c.ch.kc_top * c.ch.vec_bytes));
    const size_t n_ctr = c.n_cnt + c.n_coh + c.n_self + (size_t)c.W;
    void *d_ctr = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_OUT1, n_ctr * sizeof(uint64_t), &d_ctr));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, n_ctr * sizeof(uint64_t), ctx->stream));
    c.cnt = (unsigned long long *)d_ctr;
    c.co = c.cnt + c.n_cnt;
    c.se = c.co + c.n_coh;
    c.bey = c.se + c.n_self;
    return AMOF_OK;
}

// every touched frame is quantised once
int isf_quantise(IsfCall &c)
{
    c.spans.begin(0);
    AMOF_TRY(sq_launch_quantize(c, 0, c.fr.fsel.size(), c.d_Q));
    c.spans.end();
    return AMOF_OK;
}

// per chunk of vectors: its rho table for every touched frame, then the correlation over all lags
int isf_coherent(IsfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const UploadPack &pk = c.pk;
    IsfArgs a;
    memset(&a, 0, sizeof a);
    a.rho = c.d_rho;
    a.slot_of = pk.ptr<int32_t>(c.i_slot);
    a.hkl = pk.ptr<int32_t>(c.i_hkl);
    a.recip = pk.ptr<double>(c.i_recip);
    a.scale2 = pk.ptr<double>(c.i_scale2);
    a.windows = pk.ptr<int32_t>(c.i_win);
    a.lagiv = pk.ptr<int2>(c.i_iv);
    a.counts = c.cnt;
    a.coh = c.co;
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
    timing_dom_begin(ctx, c.pass.path);
    int64_t launches = 0;
    for (const IsfChunk &k : c.ch.chunks) {
        c.spans.begin(0);
        AMOF_TRY(sq_launch_rho(c, c.d_Q, c.fr.fsel.size(), k.r0, k.r1 - k.r0, pk.ptr<int32_t>(c.i_olocal), k.nv, c.d_rho, &launches));
        c.spans.end();
        c.spans.begin(1);
        const IsfGrid g = isf_grid(k.nv, (int64_t)c.fr.omax - c.fr.omin);
        a.Kc = k.nv;
        a.vec = pk.ptr<int32_t>(c.i_order) + k.v0;
        a.opw = g.opw;
        const dim3 grid((unsigned)g.vblocks, g.gy);
        AMOF_HIP_TRY(ctx, c.pass.global ? isf_launch_corr<true>(ctx, a, grid, 0) : isf_launch_corr<false>(ctx, a, grid, c.pass.lds));
        launches++;
        c.spans.end();
    }
    timing_dom_end(ctx, launches);
    return AMOF_OK;
}

// per batch of (lag, origin) entries: the displacements D, their rho, the bins of the origin frames
int isf_self(IsfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const UploadPack &pk = c.pk;
    const size_t nb_max = isf_self_batch(c.sw.isf_rho_budget, c.N, c.K, c.S, c.entries.size());
    void *d_D = nullptr, *d_rd = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX2, nb_max * (size_t)std::max<int64_t>(c.N, 1) * sizeof(uint4), &d_D));
    AMOF_TRY(ensure(ctx, SLOT_AUX3, nb_max * (size_t)c.K * c.S * 2 * sizeof(double), &d_rd));
    c.spans.begin(2);
    for (size_t e0 = 0; e0 < c.entries.size(); e0 += nb_max) {
        const int nb = (int)std::min<size_t>(nb_max, c.entries.size() - e0);
        const IsfEntry *d_ent = pk.ptr<IsfEntry>(c.i_ent) + e0;
        if (c.N > 0)
            hipLaunchKernelGGL(isf_diff_kernel, dim3((unsigned)((c.N + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream,
                               (const uint4 *)c.d_Q, c.N, d_ent, (uint4 *)d_D);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        AMOF_TRY(sq_launch_rho(c, (const uint4 *)d_D, (size_t)nb, 0, (int)c.pl.runs.size(), pk.ptr<int32_t>(c.i_order), c.K, (double *)d_rd));
        hipLaunchKernelGGL(isf_self_bin_kernel, dim3(sq_sample_blocks(nb, c.K)), dim3(SQ_THREADS), 0, ctx->stream, (const double *)d_rd,
                           nb, c.K, c.S, c.W, d_ent, pk.ptr<int32_t>(c.i_hkl), pk.ptr<double>(c.i_recip), c.t->n_cells, c.dq,
                           (int)c.nbins, pk.ptr<double>(c.i_scale2), c.se);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    c.spans.end();
    return AMOF_OK;
}

// the flag; device form: the call's counters into the caller's; host form: fetched and descaled
int isf_finish(IsfCall &c, const SqOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    const size_t n_cnt = c.n_cnt, n_coh = c.n_coh, n_self = c.n_self;
    AMOF_TRY(sq_fetch_flag(c, true));
    if (!out.host()) {
        // (the fixed-point sums are int64: two's complement, the same addition)
        AMOF_TRY(add_into(ctx, out.counts_dev, (const uint64_t *)c.cnt, n_cnt));
        AMOF_TRY(add_into(ctx, (uint64_t *)out.sums_dev, (const uint64_t *)c.co, n_coh));
        if (c.want_self) AMOF_TRY(add_into(ctx, (uint64_t *)out.self_dev, (const uint64_t *)c.se, n_self));
        AMOF_TRY(add_into(ctx, out.beyond_dev, (const uint64_t *)c.bey, (size_t)c.W));
    }
    timing_end(ctx);
    if (out.host()) {
        std::vector<int64_t> raw(n_coh + n_self);
        AMOF_TRY(fetch(ctx, out.counts, c.cnt, n_cnt * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, raw.data(), c.co, raw.size() * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.beyond, c.bey, (size_t)c.W * sizeof(uint64_t)));
        for (int x = 0; x < c.S * c.S; x++) sq_descale(raw.data() + (size_t)x * n_cnt, n_cnt, c.sexp2[x], out.sums + (size_t)x * n_cnt);
        if (c.want_self)
            for (int s = 0; s < c.S; s++)
                sq_descale(raw.data() + n_coh + (size_t)s * n_cnt, n_cnt, c.sexp2[s * c.S + s], out.selfs + (size_t)s * n_cnt);
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    c.spans.collect();
    return AMOF_OK;
}

int isf_run(IsfCall &c, int64_t wb, int64_t we, const SqOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    const int32_t W = c.W;
    AMOF_TRY(sq_check(c, true, [&] { return check_lag_args(ctx, c.windows, W, c.F, c.stride); }));
    static_assert(sizeof(LagRange) == sizeof(int2), "the kernels read the table as int2");
    c.lagiv.assign(std::max(W, 1), LagRange{0, 0});
    const int64_t total = lag_work_ranges(c.windows, W, c.F, c.stride, wb, we, c.lagiv.data());
    int64_t n_entries = 0;
    for (int w = 0; w < W; w++) n_entries += c.lagiv[w].o1 - c.lagiv[w].o0;
    if (wb < 0 || we > total || wb > we) return fail(ctx, AMOF_EINVAL, "work range [%lld, %lld) outside [0, %lld)", (long long)wb,
                                                     (long long)we, (long long)total);
    c.n_cnt = (size_t)W * c.nbins;
    c.n_coh = (size_t)c.S * c.S * c.n_cnt;
    c.n_self = c.want_self ? (size_t)c.S * c.n_cnt : 0;
    AMOF_TRY(sq_check_histogram(c, c.n_coh));
    AMOF_TRY(sq_call_scales(c, out.scale_log2));
    sq_expand_pairs(c.S, c.sc, c.scale2, c.sexp2);
    if (out.host()) {
        std::fill(out.counts, out.counts + c.n_cnt, (uint64_t)0);
        std::fill(out.sums, out.sums + c.n_coh, 0.0);
        if (out.selfs) std::fill(out.selfs, out.selfs + c.n_self, 0.0);
        std::fill(out.beyond, out.beyond + W, (uint64_t)0);
    }
    if (n_entries == 0 || c.K == 0) return AMOF_OK;

    AMOF_TRY(build_geometry(ctx, c.t, c.hg));
    AMOF_TRY(sq_call_plan(c));
    isf_plan(c);
    AMOF_TRY(isf_stage(c));
    AMOF_TRY(isf_quantise(c));
    AMOF_TRY(isf_coherent(c));
    if (c.want_self) AMOF_TRY(isf_self(c));
    return isf_finish(c, out);
}

// ------------------------------------------------------------------------------- C_L(q, t) and C_T(q, t) --
// Current correlation functions: the time correlation of j_a(k) = sum_j v_j exp(i k . r_j), projected along and across k
// (amof_current_modes, amof_current_accumulate[_dev]).  No existing kernel or launch is touched.
//
// Data path, per call:
//   pos [, vel] --current_mean_kernel--> mean[F][3] (remove_com: the mass-weighted mean sample of every frame, f64, fixed order)
//   pos [, vel], mean --current_record_kernel--> vmax (every frame 1 .. F - 1: exact u32 max of the f32 |components|), and for
//       the frames the work range touches P[slot][N] (u32 phase position) and V[slot][N] (f32 sample), species-permutation order
//   per chunk of K_c vectors (whole runs of CUR_RUN; the table [slots][K_c][S][6] f64 stays inside the budget):
//     P, V --current_rho_kernel--> jtab[slot][v][s][x y z][Re Im]
//     jtab --current_corr_kernel--> counts[W][nbins], long[S][S][W][nbins], trans[S][S][W][nbins] (int64 fixed point), beyond[W]
//
// current_rho_kernel is sq_rho_kernel with a velocity: per (atom, vector) the same u32 add, conversion and v_cos_f32 /
// v_sin_f32, then six fmaf into f32 partials over at most SQ_BLOCK atoms, folded into f64 in a fixed order.
// current_corr_kernel: a lane owns a vector of the chunk, a workgroup a range of origin indices; per lag the lane walks its
// origins, projects both rows on the frames' own k^ (f64, no fma), rounds the 2 S^2 products to int64 and sums them in
// registers while the bin stays the same, then adds with one atomic per (lane, lag, pair, run of equal bins) -- into per-lag
// LDS counter tiles or global memory ("current_global").  S > CUR_SMAX walks once per ordered pair with two sums in registers.
struct CurRecArgs {
    const double *pos;          // [F][N][3]
    const double *vel;          // [F][N][3] or NULL (positions mode: finite differences)
    const double *geom;
    const double *mean;         // [F][3] or NULL
    const int32_t *perm;
    const int32_t *slot_of;     // [F]
    uint4 *P;
    float4 *V;
    uint32_t *vmax_bits;
    int32_t *flag;
    int64_t N, n_cells;
    int32_t f0;
};

// the sample of atom a on frame f >= 1 (f64, before the mean is removed) and its u32 phase position
__device__ __forceinline__ void current_sample(const CurRecArgs &r, int f, int64_t a, double v[3], uint32_t p[3])
{
    const double *g1 = r.geom + (size_t)(r.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    const QAtom q1 = quantize_atom(r.pos, g1, r.N, f, a, 0, 1, 2, r.flag);
    if (r.vel) {
        const double *w = r.vel + ((size_t)f * r.N + a) * 3;
        v[0] = w[0]; v[1] = w[1]; v[2] = w[2];
        p[0] = q1.ux; p[1] = q1.uy; p[2] = q1.uz;
        return;
    }
    const double *g0 = r.geom + (size_t)(r.n_cells == 1 ? 0 : f - 1) * GEOM_STRIDE;
    const QAtom q0 = quantize_atom(r.pos, g0, r.N, f - 1, a, 0, 1, 2, r.flag);
    const int32_t dx = (int32_t)(q1.ux - q0.ux), dy = (int32_t)(q1.uy - q0.uy), dz = (int32_t)(q1.uz - q0.uz);
    const double sx = (double)dx * 2.3283064365386963e-10, sy = (double)dy * 2.3283064365386963e-10,
                 sz = (double)dz * 2.3283064365386963e-10;
#pragma unroll
    for (int c = 0; c < 3; c++) v[c] = fma(sz, g1[6 + c], fma(sy, g1[3 + c], sx * g1[c]));
    p[0] = q0.ux + (uint32_t)(dx >> 1);
    p[1] = q0.uy + (uint32_t)(dy >> 1);
    p[2] = q0.uz + (uint32_t)(dz >> 1);
}

// mean[f][c] = sum_a mass_a v_a[c] / total_mass of frame f = f0 + blockIdx.x: thread t adds the atoms t, t + 256, ... in
// order (fma), the 256 partials fold pairwise in LDS -- a fixed order, no float atomics
__global__ __launch_bounds__(256) void current_mean_kernel(CurRecArgs r, const double *__restrict__ mass, double total_mass,
                                                           double *__restrict__ mean)
{
    __shared__ double part[3][256];
    const int f = r.f0 + (int)blockIdx.x, tid = threadIdx.x;
    double acc[3] = {0.0, 0.0, 0.0};
    for (int64_t a = tid; a < r.N; a += 256) {
        double v[3];
        uint32_t p[3];
        current_sample(r, f, a, v, p);
        const double m = mass[a];
#pragma unroll
        for (int c = 0; c < 3; c++) acc[c] = fma(m, v[c], acc[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) part[c][tid] = acc[c];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) {
#pragma unroll
            for (int c = 0; c < 3; c++) part[c][tid] += part[c][tid + h];
        }
        __syncthreads();
    }
    if (tid < 3) mean[3 * (size_t)f + tid] = part[tid][0] / total_mass;
}

// grid (atoms / 256, frames from f0): the sample with the mean removed, rounded to f32; its largest |component| into
// *vmax_bits (non-negative floats order as their bits: an exact max whatever the order); records where the frame is touched
__global__ __launch_bounds__(256) void current_record_kernel(CurRecArgs r)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int f = r.f0 + (int)blockIdx.y;
    uint32_t top = 0u;
    if (i < r.N) {
        double v[3];
        uint32_t p[3];
        current_sample(r, f, r.perm[i], v, p);
        float w[3];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            if (r.mean) v[c] -= r.mean[3 * (size_t)f + c];
            w[c] = (float)v[c];
            if (!(fabsf(w[c]) <= 3.0e38f)) *r.flag = 2;         // not finite, or beyond f32
            top = max(top, __float_as_uint(fabsf(w[c])));
        }
        const int slot = r.slot_of[f];
        if (slot >= 0) {
            r.P[(size_t)slot * r.N + i] = make_uint4(p[0], p[1], p[2], 0u);
            r.V[(size_t)slot * r.N + i] = make_float4(w[0], w[1], w[2], 0.0f);
        }
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) top = max(top, (uint32_t)__shfl_xor((int)top, s));
    if ((threadIdx.x & 63) == 0 && top) atomicMax(r.vmax_bits, top);
}

// jtab[b][order[run.start + r]][s][c][0 / 1] = Re / Im of component c of j_s(h, k, l0 + r) of slot b
__global__ __launch_bounds__(CUR_THREADS) void current_rho_kernel(const uint4 *__restrict__ P, const float4 *__restrict__ V,
                                                                  int64_t N, const int64_t *__restrict__ sp_first, int S,
                                                                  const SqRun *__restrict__ runs, int n_runs,
                                                                  const int32_t *__restrict__ order, int K,
                                                                  double *__restrict__ jtab)
{
    constexpr int R = CUR_RUN;
    const int ri = blockIdx.x * CUR_THREADS + threadIdx.x;
    if (blockIdx.x * CUR_THREADS + (int)(threadIdx.x & ~63u) >= n_runs) return;    // a wave without a live lane (no barrier below)
    const bool live = ri < n_runs;
    const SqRun run = runs[live ? ri : n_runs - 1];     // (idle lanes of a live wave compute a copy of the last run and write nothing)
    const uint4 *__restrict__ q = P + (size_t)blockIdx.y * N;
    const float4 *__restrict__ vv = V + (size_t)blockIdx.y * N;
    double *__restrict__ out = jtab + (size_t)blockIdx.y * K * S * 6;
    const uint32_t h = (uint32_t)run.h, k = (uint32_t)run.k, l0 = (uint32_t)run.l0;
    const float rev = 2.3283064365386963e-10f;         // 2^-32
    for (int s = 0; s < S; s++) {
        const int64_t a0 = sp_first[s], a1 = sp_first[s + 1];
        double acc[R][6];
#pragma unroll
        for (int r = 0; r < R; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) acc[r][c] = 0.0;
        for (int64_t b0 = a0; b0 < a1; b0 += SQ_BLOCK) {
            const int64_t b1 = min(b0 + (int64_t)SQ_BLOCK, a1);
            float p[R][6];
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int c = 0; c < 6; c++) p[r][c] = 0.0f;
            for (int64_t j = b0; j < b1; j++) {        // j < sp_first[S] = N: no load past the slot
                const uint4 u = q[j];
                const float4 w = vv[j];
                uint32_t phi = h * u.x + k * u.y + l0 * u.z;
#pragma unroll
                for (int r = 0; r < R; r++) {
                    const float x = (float)(int32_t)phi * rev;
                    const float co = __builtin_amdgcn_cosf(x), si = __builtin_amdgcn_sinf(x);
                    p[r][0] = fmaf(w.x, co, p[r][0]);
                    p[r][1] = fmaf(w.x, si, p[r][1]);
                    p[r][2] = fmaf(w.y, co, p[r][2]);
                    p[r][3] = fmaf(w.y, si, p[r][3]);
                    p[r][4] = fmaf(w.z, co, p[r][4]);
                    p[r][5] = fmaf(w.z, si, p[r][5]);
                    phi += u.z;
                }
            }
#pragma unroll
            for (int r = 0; r < R; r++)
#pragma unroll
                for (int c = 0; c < 6; c++) acc[r][c] += (double)p[r][c];
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < R; r++) {
                if (r < run.n) {
                    double *o = out + ((size_t)order[run.start + r] * S + s) * 6;
#pragma unroll
                    for (int c = 0; c < 6; c++) o[c] = acc[r][c];
                }
            }
        }
    }
}

struct CurArgs {
    const double *jtab;         // [slots][Kc][S][6]
    const int32_t *slot_of;     // [F]
    const int32_t *vec;         // [Kc]: the caller's index of the chunk's vectors
    const int32_t *hkl;         // [K][3]
    const double *recip;        // [n_cells][9]
    const double *scale2;       // [S][S]
    const int32_t *windows;     // [W]
    const int2 *lagiv;          // [W]
    unsigned long long *counts, *lng, *trn, *beyond;
    int64_t n_cells, stride;
    int32_t Kc, S, W, nbins, omin, omax, opw, lags_per_pass;
    double dq;
};

// the bin of amof_sq_accumulate (-1 = beyond) and k^ = q / |q| of the same q (f64, no fma)
__device__ __forceinline__ int current_khat(const double *__restrict__ R, const int32_t *__restrict__ v, double dq, int nbins,
                                            double u[3])
{
    const double h = (double)v[0], k = (double)v[1], l = (double)v[2];
    const double qx = (h * R[0] + k * R[3]) + l * R[6];
    const double qy = (h * R[1] + k * R[4]) + l * R[7];
    const double qz = (h * R[2] + k * R[5]) + l * R[8];
    const double n = sqrt((qx * qx + qy * qy) + qz * qz);
    u[0] = qx / n;
    u[1] = qy / n;
    u[2] = qz / n;
    const double qq = n / dq;
    if (!(qq < (double)nbins)) return -1;
    return (int)qq;
}

// L = k^ . j (complex), T = j - k^ L (complex 3-vector) of one species' row j[6]
__device__ __forceinline__ void current_project(const double *__restrict__ j, const double u[3], double L[2], double T[6])
{
    const double jx0 = j[0], jx1 = j[1], jy0 = j[2], jy1 = j[3], jz0 = j[4], jz1 = j[5];
    L[0] = (u[0] * jx0 + u[1] * jy0) + u[2] * jz0;
    L[1] = (u[0] * jx1 + u[1] * jy1) + u[2] * jz1;
    T[0] = jx0 - u[0] * L[0];
    T[1] = jx1 - u[0] * L[1];
    T[2] = jy0 - u[1] * L[0];
    T[3] = jy1 - u[1] * L[1];
    T[4] = jz0 - u[2] * L[0];
    T[5] = jz1 - u[2] * L[1];
}

// One lane's origins [lo, hi) of one lag: the NA x NA ordered pairs (sa + x, sc + c) of the S species.  first: this walk also
// counts the samples and the vectors beyond the bins (one walk per lag does).
template <int NA>
__device__ __forceinline__ void current_walk(const CurArgs &a, int v, const int32_t *__restrict__ hv, int lo, int hi, int64_t m,
                                             int sa, int sc, bool first, unsigned long long *cw, unsigned long long *lg,
                                             unsigned long long *tg, size_t cstep, unsigned long long &nbey)
{
    const int S = a.S, nbins = a.nbins;
    const size_t row = (size_t)S * 6;
    unsigned long long accL[NA * NA], accT[NA * NA], cnt = 0;
    int cur = -1;
#pragma unroll
    for (int i = 0; i < NA * NA; i++) { accL[i] = 0ull; accT[i] = 0ull; }
    auto flush = [&]() {
        if (!cnt) return;
        if (first) atomicAdd(&cw[cur], cnt);
#pragma unroll
        for (int x = 0; x < NA; x++)
#pragma unroll
            for (int c = 0; c < NA; c++) {
                const size_t pair = (size_t)(sa + x) * S + (sc + c);
                if (accL[x * NA + c]) atomicAdd(&lg[pair * cstep + cur], accL[x * NA + c]);
                if (accT[x * NA + c]) atomicAdd(&tg[pair * cstep + cur], accT[x * NA + c]);
                accL[x * NA + c] = 0ull;
                accT[x * NA + c] = 0ull;
            }
        cnt = 0;
    };
    double u0[3], u1[3];
    int bin0 = 0;
    if (a.n_cells == 1) {
        bin0 = current_khat(a.recip, hv, a.dq, nbins, u0);
#pragma unroll
        for (int c = 0; c < 3; c++) u1[c] = u0[c];
    }
    for (int o = lo; o < hi; o++) {
        const int64_t k = 1 + a.stride * (int64_t)o, km = k + m;
        int bin = bin0;
        if (a.n_cells != 1) {
            bin = current_khat(a.recip + (size_t)k * 9, hv, a.dq, nbins, u0);
            (void)current_khat(a.recip + (size_t)km * 9, hv, a.dq, nbins, u1);
        }
        if (bin < 0) { nbey++; continue; }
        if (bin != cur) { flush(); cur = bin; }
        cnt++;
        const double *__restrict__ j0 = a.jtab + ((size_t)a.slot_of[k] * a.Kc + v) * row + (size_t)sa * 6;
        const double *__restrict__ j1 = a.jtab + ((size_t)a.slot_of[km] * a.Kc + v) * row + (size_t)sc * 6;
        double L0[NA][2], T0[NA][6];
#pragma unroll
        for (int x = 0; x < NA; x++) current_project(j0 + 6 * x, u0, L0[x], T0[x]);
#pragma unroll
        for (int c = 0; c < NA; c++) {
            double L1[2], T1[6];
            current_project(j1 + 6 * c, u1, L1, T1);
#pragma unroll
            for (int x = 0; x < NA; x++) {
                const double sc2 = a.scale2[(sa + x) * S + (sc + c)];
                const double tl = L0[x][0] * L1[0] + L0[x][1] * L1[1];
                const double tt = ((T0[x][0] * T1[0] + T0[x][1] * T1[1]) + (T0[x][2] * T1[2] + T0[x][3] * T1[3])) +
                                  (T0[x][4] * T1[4] + T0[x][5] * T1[5]);
                accL[x * NA + c] += (unsigned long long)(long long)rint(tl * sc2);
                accT[x * NA + c] += (unsigned long long)(long long)rint(tt * sc2);
            }
        }
    }
    flush();
}

// LDS tile of one lag: [counts nbins | long S^2 nbins | trans S^2 nbins]
template <int ST, bool GLOBAL>
__global__ __launch_bounds__(CUR_THREADS) void current_corr_kernel(CurArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long *lc = reinterpret_cast<unsigned long long *>(lds_raw);
    const int tid = threadIdx.x;
    const int S = ST ? ST : a.S;
    const int W = a.W, nbins = a.nbins, Kc = a.Kc;
    const int v = blockIdx.x * CUR_THREADS + tid;
    const bool live = v < Kc;
    const int ob = a.omin + (int)blockIdx.y * a.opw, oe = min(ob + a.opw, a.omax);
    const int tile = (1 + 2 * S * S) * nbins;
    const int L = GLOBAL ? W : a.lags_per_pass;
    const int32_t *hv = a.hkl + 3 * (size_t)a.vec[live ? v : 0];

    for (int w0 = 0; w0 < W; w0 += L) {
        const int w1 = min(w0 + L, W);
        if (!GLOBAL) {
            for (int i = tid; i < (w1 - w0) * tile; i += CUR_THREADS) lc[i] = 0ull;
            __syncthreads();
        }
        if (live) {
            for (int w = w0; w < w1; w++) {
                const int2 iv = a.lagiv[w];
                const int lo = max(ob, iv.x), hi = min(oe, iv.y);
                if (lo >= hi) continue;
                const int64_t m = a.windows[w];
                unsigned long long *cw = GLOBAL ? a.counts + (size_t)w * nbins : lc + (size_t)(w - w0) * tile;
                unsigned long long *lg = GLOBAL ? a.lng + (size_t)w * nbins : cw + nbins;
                unsigned long long *tg = GLOBAL ? a.trn + (size_t)w * nbins : cw + (size_t)(1 + S * S) * nbins;
                const size_t cstep = GLOBAL ? (size_t)W * nbins : (size_t)nbins;
                unsigned long long nbey = 0, skip = 0;
                if (ST) {
                    current_walk<(ST ? ST : 1)>(a, v, hv, lo, hi, m, 0, 0, true, cw, lg, tg, cstep, nbey);
                } else {
                    for (int x = 0; x < S; x++)
                        for (int c = 0; c < S; c++)
                            current_walk<1>(a, v, hv, lo, hi, m, x, c, x == 0 && c == 0, cw, lg, tg, cstep, x == 0 && c == 0 ? nbey : skip);
                }
                if (nbey) atomicAdd(&a.beyond[w], nbey);
            }
        }
        if (!GLOBAL) {
            __syncthreads();
            const int S2 = S * S;
            for (int i = tid; i < (w1 - w0) * tile; i += CUR_THREADS) {
                const unsigned long long val = lc[i];
                if (!val) continue;
                const int w = w0 + i / tile, r = i % tile, j = r / nbins, b = r % nbins;
                unsigned long long *dst = j == 0 ? &a.counts[(size_t)w * nbins + b]
                                          : j <= S2 ? &a.lng[((size_t)(j - 1) * W + w) * nbins + b]
                                                    : &a.trn[((size_t)(j - 1 - S2) * W + w) * nbins + b];
                atomicAdd(dst, val);
            }
            __syncthreads();
        }
    }
}

template <bool GLOBAL>
hipError_t current_launch_corr(amof_ctx *ctx, const CurArgs &a, dim3 grid, size_t lds)
{
    auto go = [&](auto kern) -> hipError_t {
        if (!GLOBAL) {
            hipError_t e = allow_max_lds((const void *)kern);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(kern, grid, dim3(CUR_THREADS), GLOBAL ? 0 : lds, ctx->stream, a);
        return hipGetLastError();
    };
    switch (a.S <= CUR_SMAX ? a.S : 0) {
    case 1: return go(current_corr_kernel<1, GLOBAL>);
    case 2: return go(current_corr_kernel<2, GLOBAL>);
    case 3: return go(current_corr_kernel<3, GLOBAL>);
    case 4: return go(current_corr_kernel<4, GLOBAL>);
    default: return go(current_corr_kernel<0, GLOBAL>);
    }
}

// The caller's arrays of amof_current_accumulate (host form: f64, overwritten) or amof_current_accumulate_dev (device form:
// int64 fixed point / u64, added into)
struct CurOutputs {
    uint64_t *counts = nullptr, *beyond = nullptr;
    double *lng = nullptr, *trn = nullptr;
    uint64_t *counts_dev = nullptr, *beyond_dev = nullptr;
    int64_t *lng_dev = nullptr, *trn_dev = nullptr;
    int32_t *scale_log2 = nullptr;
    double *vmax = nullptr;
    bool host() const { return counts != nullptr; }
};

struct CurCall : SqCall {
    const amof_traj *vel = nullptr;
    bool remove_com = false;
    const int32_t *windows = nullptr;
    int32_t W = 0;
    int64_t stride = 1;
    CurSwitches csw = CurSwitches::from_env();
    std::vector<LagRange> lagiv;
    size_t n_cnt = 0, n_pair = 0;
    double total_mass = 0.0, vmax = 0.0;
    SqScales cs;
    std::vector<double> scale2;
    std::vector<int32_t> sexp2;
    IsfFrames fr;
    IsfChunks ch;
    CurPass pass;
    int i_olocal = -1, i_slot = -1, i_win = -1, i_iv = -1, i_mass = -1;
    const double *vel_dev = nullptr;
    float4 *d_V = nullptr;              // SLOT_AUX2
    double *d_mean = nullptr;           // SLOT_AUX3
    uint32_t *d_vmax = nullptr;         // SLOT_AUX4
    const double *d_scale2 = nullptr;   // SLOT_AUX6
    unsigned long long *cnt = nullptr, *lg = nullptr, *tr = nullptr, *bey = nullptr;
    StageSpans spans;                   // records (means and vmax included), table, correlation
    CurCall(amof_ctx *ctx_, const amof_traj *t_, const double *recip_, const int32_t *hkl_, int32_t K_, double dq_, int32_t nbins_)
        : SqCall(ctx_, t_, recip_, hkl_, K_, dq_, nbins_), spans(ctx_) {}
};

// the velocity trajectory and the masses, after sq_check_traj
int current_check_inputs(CurCall &c)
{
    amof_ctx *ctx = c.ctx;
    if (c.vel) {
        if (c.vel->n_frames != c.F || c.vel->n_atoms != c.N) return fail(ctx, AMOF_EINVAL, "velocities: other frames or atoms than the positions");
        if (c.F > 0 && c.N > 0 && !c.vel->pos) return fail(ctx, AMOF_EINVAL, "NULL velocities");
    }
    if (c.F > 0x7fffffffLL || c.N > 0x7fffffffLL) return fail(ctx, AMOF_EINVAL, "too many frames or atoms");
    if (c.remove_com) {
        if (c.N > 0 && !c.t->masses) return fail(ctx, AMOF_EINVAL, "masses required");
        c.total_mass = 0.0;
        for (int64_t i = 0; i < c.N; i++) c.total_mass += c.t->masses[i];
        if (c.N > 0 && (!(c.total_mass > 0.0) || !isfinite(c.total_mass))) return fail(ctx, AMOF_EINVAL, "the masses must add up to a positive number");
    }
    return AMOF_OK;
}

int current_call_plan(CurCall &c)
{
    sq_species_order(c.t->species, c.N, c.S, c.pl);
    const int32_t zero = current_cut_runs(c.hkl, c.K, c.pl);
    return zero >= 0 ? fail(c.ctx, AMOF_EINVAL, "hkl %d is (0, 0, 0)", zero) : AMOF_OK;
}

// uploads, scratch and the staged velocities; rho_bytes: the table; n_ctr: the call's own counters (0: none)
int current_stage(CurCall &c, size_t rho_bytes, size_t n_ctr)
{
    amof_ctx *ctx = c.ctx;
    UploadPack &pk = c.pk;
    c.i_olocal = pk.add(c.ch.order_local.data(), c.ch.order_local.size() * sizeof(int32_t));
    c.i_slot = pk.add(c.fr.slot_of.data(), c.fr.slot_of.size() * sizeof(int32_t));
    c.i_win = pk.add(c.windows, (size_t)c.W * sizeof(int32_t));
    c.i_iv = pk.add(c.lagiv.data(), c.lagiv.size() * sizeof(LagRange));
    if (c.remove_com) c.i_mass = pk.add(c.t->masses, (size_t)c.N * sizeof(double));
    const size_t slots = c.fr.fsel.size();
    AMOF_TRY(sq_stage(c, c.fr.fsel.data(), slots, slots, rho_bytes));
    c.vel_dev = nullptr;
    if (c.vel) {
        if (c.vel->pos_on_device) {
            c.vel_dev = c.vel->pos;
        } else {
            void *p = nullptr;
            AMOF_TRY(upload(ctx, SLOT_AUX5, c.vel->pos, (size_t)c.F * (size_t)c.N * 3 * sizeof(double), &p));
            c.vel_dev = (const double *)p;
        }
    }
    void *d_V = nullptr, *d_mean = nullptr, *d_vmax = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX2, slots * (size_t)std::max<int64_t>(c.N, 1) * sizeof(float4), &d_V));
    AMOF_TRY(ensure(ctx, SLOT_AUX3, (size_t)std::max<int64_t>(c.F, 1) * 3 * sizeof(double), &d_mean));
    AMOF_TRY(ensure(ctx, SLOT_AUX4, sizeof(uint32_t), &d_vmax));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_vmax, 0, sizeof(uint32_t), ctx->stream));
    c.d_V = (float4 *)d_V;
    c.d_mean = (double *)d_mean;
    c.d_vmax = (uint32_t *)d_vmax;
    if (n_ctr) {
        void *d_ctr = nullptr;
        AMOF_TRY(ensure(ctx, SLOT_OUT1, n_ctr * sizeof(uint64_t), &d_ctr));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_ctr, 0, n_ctr * sizeof(uint64_t), ctx->stream));
        c.cnt = (unsigned long long *)d_ctr;
        c.lg = c.cnt + c.n_cnt;
        c.tr = c.lg + c.n_pair;
        c.bey = c.tr + c.n_pair;
    }
    return AMOF_OK;
}

// the means (remove_com) and the records of the frames [f0, f0 + nf), f0 >= 1
int current_records(CurCall &c, int64_t f0, int64_t nf)
{
    amof_ctx *ctx = c.ctx;
    if (c.N == 0 || nf <= 0) return AMOF_OK;
    CurRecArgs r;
    memset(&r, 0, sizeof r);
    r.pos = c.pos_dev;
    r.vel = c.vel_dev;
    r.geom = c.pk.ptr<double>(c.i_geom);
    r.perm = c.pk.ptr<int32_t>(c.i_perm);
    r.slot_of = c.pk.ptr<int32_t>(c.i_slot);
    r.P = c.d_Q;
    r.V = c.d_V;
    r.vmax_bits = c.d_vmax;
    r.flag = c.d_flag;
    r.N = c.N;
    r.n_cells = c.t->n_cells;
    c.spans.begin(0);
    for (int64_t s0 = 0; s0 < nf; s0 += (int64_t)SQ_GRID_Y) {
        const unsigned nb = (unsigned)std::min<int64_t>((int64_t)SQ_GRID_Y, nf - s0);
        r.f0 = (int32_t)(f0 + s0);
        if (c.remove_com) {
            r.mean = nullptr;
            hipLaunchKernelGGL(current_mean_kernel, dim3(nb), dim3(256), 0, ctx->stream, r, c.pk.ptr<double>(c.i_mass), c.total_mass,
                               c.d_mean);
            AMOF_HIP_TRY(ctx, hipGetLastError());
            r.mean = c.d_mean;
        }
        hipLaunchKernelGGL(current_record_kernel, dim3((unsigned)((c.N + 255) / 256), nb), dim3(256), 0, ctx->stream, r);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    c.spans.end();
    return AMOF_OK;
}

// the quantiser's flag, the f32 range of the samples and vmax (complete on return: the stream is synchronised)
int current_fetch_vmax(CurCall &c)
{
    int32_t flag = 0;
    uint32_t bits = 0;
    AMOF_TRY(fetch(c.ctx, &flag, c.d_flag, sizeof(int32_t)));
    AMOF_TRY(fetch(c.ctx, &bits, c.d_vmax, sizeof(uint32_t)));
    if (flag) {
        timing_end(c.ctx);
        return fail(c.ctx, AMOF_EINVAL, flag == 2 ? "velocities are not finite or exceed the float32 range"
                                                  : "positions lie more than 10^4 cells from the cell, or are not finite");
    }
    float f;
    memcpy(&f, &bits, sizeof f);
    c.vmax = (double)f;
    return AMOF_OK;
}

int current_launch_rho(CurCall &c, int r0, int n_runs, const int32_t *d_order, int Kc, int64_t *launches = nullptr)
{
    const size_t n = c.fr.fsel.size();
    for (size_t s0 = 0; s0 < n; s0 += SQ_GRID_Y) {
        const unsigned nb = (unsigned)std::min<size_t>(SQ_GRID_Y, n - s0);
        hipLaunchKernelGGL(current_rho_kernel, dim3((unsigned)((n_runs + CUR_THREADS - 1) / CUR_THREADS), nb), dim3(CUR_THREADS), 0,
                           c.ctx->stream, (const uint4 *)c.d_Q + s0 * (size_t)c.N, (const float4 *)c.d_V + s0 * (size_t)c.N, c.N,
                           c.pk.ptr<int64_t>(c.i_spf), c.S, c.pk.ptr<SqRun>(c.i_runs) + r0, n_runs, d_order, Kc,
                           c.d_rho + s0 * (size_t)Kc * c.S * 6);
        AMOF_HIP_TRY(c.ctx, hipGetLastError());
        if (launches) ++*launches;
    }
    return AMOF_OK;
}

int current_correlate(CurCall &c)
{
    amof_ctx *ctx = c.ctx;
    const UploadPack &pk = c.pk;
    CurArgs a;
    memset(&a, 0, sizeof a);
    a.jtab = c.d_rho;
    a.slot_of = pk.ptr<int32_t>(c.i_slot);
    a.hkl = pk.ptr<int32_t>(c.i_hkl);
    a.recip = pk.ptr<double>(c.i_recip);
    a.scale2 = c.d_scale2;
    a.windows = pk.ptr<int32_t>(c.i_win);
    a.lagiv = pk.ptr<int2>(c.i_iv);
    a.counts = c.cnt;
    a.lng = c.lg;
    a.trn = c.tr;
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
    timing_dom_begin(ctx, c.pass.path);
    int64_t launches = 0;
    for (const IsfChunk &k : c.ch.chunks) {
        c.spans.begin(1);
        AMOF_TRY(current_launch_rho(c, k.r0, k.r1 - k.r0, pk.ptr<int32_t>(c.i_olocal), k.nv, &launches));
        c.spans.end();
        c.spans.begin(2);
        const CurGrid g = current_grid(k.nv, (int64_t)c.fr.omax - c.fr.omin);
        a.Kc = k.nv;
        a.vec = pk.ptr<int32_t>(c.i_order) + k.v0;
        a.opw = g.opw;
        const dim3 grid((unsigned)g.vblocks, g.gy);
        AMOF_HIP_TRY(ctx, c.pass.global ? current_launch_corr<true>(ctx, a, grid, 0) : current_launch_corr<false>(ctx, a, grid, c.pass.lds));
        launches++;
        c.spans.end();
    }
    timing_dom_end(ctx, launches);
    return AMOF_OK;
}

int current_finish(CurCall &c, const CurOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    if (!out.host()) {
        AMOF_TRY(add_into(ctx, out.counts_dev, (const uint64_t *)c.cnt, c.n_cnt));
        AMOF_TRY(add_into(ctx, (uint64_t *)out.lng_dev, (const uint64_t *)c.lg, c.n_pair));
        AMOF_TRY(add_into(ctx, (uint64_t *)out.trn_dev, (const uint64_t *)c.tr, c.n_pair));
        AMOF_TRY(add_into(ctx, out.beyond_dev, (const uint64_t *)c.bey, (size_t)c.W));
    }
    timing_end(ctx);
    if (out.host()) {
        std::vector<int64_t> raw(2 * c.n_pair);
        AMOF_TRY(fetch(ctx, out.counts, c.cnt, c.n_cnt * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, raw.data(), c.lg, raw.size() * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.beyond, c.bey, (size_t)c.W * sizeof(uint64_t)));
        for (int x = 0; x < c.S * c.S; x++) {
            sq_descale(raw.data() + (size_t)x * c.n_cnt, c.n_cnt, c.sexp2[x], out.lng + (size_t)x * c.n_cnt);
            sq_descale(raw.data() + c.n_pair + (size_t)x * c.n_cnt, c.n_cnt, c.sexp2[x], out.trn + (size_t)x * c.n_cnt);
        }
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    c.spans.collect();
    return AMOF_OK;
}

int current_run(CurCall &c, int64_t wb, int64_t we, const CurOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    const int32_t W = c.W;
    AMOF_TRY(sq_check(c, true, [&] { return check_lag_args(ctx, c.windows, W, c.F, c.stride); }));
    AMOF_TRY(current_check_inputs(c));
    c.lagiv.assign(std::max(W, 1), LagRange{0, 0});
    const int64_t total = lag_work_ranges(c.windows, W, c.F, c.stride, wb, we, c.lagiv.data());
    int64_t n_entries = 0;
    for (int w = 0; w < W; w++) n_entries += c.lagiv[w].o1 - c.lagiv[w].o0;
    if (wb < 0 || we > total || wb > we) return fail(ctx, AMOF_EINVAL, "work range [%lld, %lld) outside [0, %lld)", (long long)wb,
                                                     (long long)we, (long long)total);
    c.n_cnt = (size_t)W * c.nbins;
    c.n_pair = (size_t)c.S * c.S * c.n_cnt;
    AMOF_TRY(sq_check_histogram(c, 2 * c.n_pair));
    const int P = c.P;
    std::fill(out.scale_log2, out.scale_log2 + P, 0);
    *out.vmax = 0.0;
    if (out.host()) {
        std::fill(out.counts, out.counts + c.n_cnt, (uint64_t)0);
        std::fill(out.lng, out.lng + c.n_pair, 0.0);
        std::fill(out.trn, out.trn + c.n_pair, 0.0);
        std::fill(out.beyond, out.beyond + W, (uint64_t)0);
    }
    if (c.K == 0 || c.F < 2 || c.N == 0) return AMOF_OK;

    AMOF_TRY(build_geometry(ctx, c.t, c.hg));
    AMOF_TRY(current_call_plan(c));
    isf_touched_frames(c.lagiv.data(), c.windows, W, c.F, c.stride, c.fr);
    if (n_entries > 0) current_cut_chunks(c.pl.runs, c.K, c.fr.fsel.size(), c.S, c.csw.rho_budget, c.ch);
    else c.ch.order_local.assign((size_t)c.K, 0);
    c.pass = current_pass_plan(c.S, c.nbins, W, c.csw);
    AMOF_TRY(current_stage(c, n_entries > 0 ? (size_t)c.ch.kc_top * c.ch.vec_bytes : 0, c.n_cnt + 2 * c.n_pair + (size_t)W));
    // vmax is the whole trajectory's, whatever the work range: every frame from 1 passes the record kernel
    AMOF_TRY(current_records(c, 1, c.F - 1));
    AMOF_TRY(current_fetch_vmax(c));
    const int64_t cap = sq_bin_capacity(c.recip, c.t->n_cells, c.hkl, c.K, c.dq, c.nbins);
    if (current_scales(c.t->species, c.N, c.S, c.F, cap, c.vmax, c.cs) >= 0) {
        timing_end(ctx);
        return fail(ctx, AMOF_ECAPACITY, "C(q, t): %lld frames x %lld vectors per bin x %lld x %lld atoms exceed the fixed-point "
                                         "range (quantum above 2^-20): use fewer vectors per bin (max_points) or a smaller dq",
                    (long long)c.F, (long long)cap, (long long)c.cs.nsp[c.cs.bad_a], (long long)c.cs.nsp[c.cs.bad_c]);
    }
    std::copy(c.cs.sexp.begin(), c.cs.sexp.end(), out.scale_log2);
    *out.vmax = c.vmax;
    sq_expand_pairs(c.S, c.cs, c.scale2, c.sexp2);
    if (n_entries > 0) {                // (vmax == 0: scale 0, the samples are still counted)
        void *d_scale2 = nullptr;
        AMOF_TRY(upload(ctx, SLOT_AUX6, c.scale2.data(), c.scale2.size() * sizeof(double), &d_scale2));
        c.d_scale2 = (const double *)d_scale2;
        AMOF_TRY(current_correlate(c));
    }
    return current_finish(c, out);
}

int current_modes_run(CurCall &c, int64_t frame, double *j)
{
    amof_ctx *ctx = c.ctx;
    AMOF_TRY(sq_check_traj(c));
    AMOF_TRY(current_check_inputs(c));
    if (!j && c.K > 0) return fail(ctx, AMOF_EINVAL, "NULL argument");
    if (frame < 1 || frame >= c.F) return fail(ctx, AMOF_EINVAL, "frame out of range (a sample needs a frame >= 1)");
    if (c.K == 0) return AMOF_OK;
    AMOF_TRY(current_call_plan(c));
    const size_t n_out = (size_t)c.K * c.S * 6;
    if (c.N == 0) {
        std::fill(j, j + n_out, 0.0);
        return AMOF_OK;
    }
    AMOF_TRY(build_geometry(ctx, c.t, c.hg));
    c.fr.slot_of.assign((size_t)c.F, -1);
    c.fr.slot_of[(size_t)frame] = 0;
    c.fr.fsel.assign(1, (int32_t)frame);
    AMOF_TRY(current_stage(c, n_out * sizeof(double), 0));
    timing_dom_begin(ctx, "current_modes");
    AMOF_TRY(current_records(c, frame, 1));
    c.spans.begin(1);
    AMOF_TRY(current_launch_rho(c, 0, (int)c.pl.runs.size(), c.pk.ptr<int32_t>(c.i_order), c.K));
    c.spans.end();
    timing_dom_end(ctx, 2);
    AMOF_TRY(current_fetch_vmax(c));
    timing_end(ctx);
    AMOF_TRY(fetch(ctx, j, c.d_rho, n_out * sizeof(double)));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    c.spans.collect();
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

extern "C" int amof_isf_accumulate(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                   const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                                   int64_t work_end, double dq, int32_t nbins, uint64_t *counts, double *coh, double *self_sums,
                                   uint64_t *beyond)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !coh || !beyond) return fail(ctx, AMOF_EINVAL, "NULL argument");
    IsfCall c(ctx, t, recip, hkl, K, dq, nbins);
    c.windows = windows;
    c.W = n_windows;
    c.stride = origin_stride;
    c.want_self = self_sums != nullptr;
    SqOutputs out;
    out.counts = counts;
    out.sums = coh;
    out.selfs = self_sums;
    out.beyond = beyond;
    return isf_run(c, work_begin, work_end, out);
}

extern "C" int amof_isf_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                       const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                                       int64_t work_end, double dq, int32_t nbins, uint64_t *counts_dev, int64_t *coh_dev,
                                       int64_t *self_dev, uint64_t *beyond_dev, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !coh_dev || !beyond_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "NULL argument");
    IsfCall c(ctx, t, recip, hkl, K, dq, nbins);
    c.windows = windows;
    c.W = n_windows;
    c.stride = origin_stride;
    c.want_self = self_dev != nullptr;
    SqOutputs out;
    out.counts_dev = counts_dev;
    out.sums_dev = coh_dev;
    out.self_dev = self_dev;
    out.beyond_dev = beyond_dev;
    out.scale_log2 = scale_log2;
    return isf_run(c, work_begin, work_end, out);
}


extern "C" int amof_current_modes(amof_ctx *ctx, const amof_traj *t, const amof_traj *vel, int64_t frame, int32_t remove_com,
                                  const int32_t *hkl, int32_t K, double *j)
{
    if (!ctx) return AMOF_EINVAL;
    CurCall c(ctx, t, nullptr, hkl, K, 0.0, 0);
    c.vel = vel;
    c.remove_com = remove_com != 0;
    return current_modes_run(c, frame, j);
}

extern "C" int amof_current_accumulate(amof_ctx *ctx, const amof_traj *t, const amof_traj *vel, int32_t remove_com,
                                       const double *recip, const int32_t *hkl, int32_t K, const int32_t *windows,
                                       int32_t n_windows, int64_t origin_stride, int64_t work_begin, int64_t work_end, double dq,
                                       int32_t nbins, uint64_t *counts, double *long_sums, double *trans_sums, uint64_t *beyond,
                                       int32_t *scale_log2, double *vmax)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !long_sums || !trans_sums || !beyond || !scale_log2 || !vmax) return fail(ctx, AMOF_EINVAL, "NULL argument");
    CurCall c(ctx, t, recip, hkl, K, dq, nbins);
    c.vel = vel;
    c.remove_com = remove_com != 0;
    c.windows = windows;
    c.W = n_windows;
    c.stride = origin_stride;
    CurOutputs out;
    out.counts = counts;
    out.lng = long_sums;
    out.trn = trans_sums;
    out.beyond = beyond;
    out.scale_log2 = scale_log2;
    out.vmax = vmax;
    return current_run(c, work_begin, work_end, out);
}

extern "C" int amof_current_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const amof_traj *vel, int32_t remove_com,
                                           const double *recip, const int32_t *hkl, int32_t K, const int32_t *windows,
                                           int32_t n_windows, int64_t origin_stride, int64_t work_begin, int64_t work_end,
                                           double dq, int32_t nbins, uint64_t *counts_dev, int64_t *long_dev, int64_t *trans_dev,
                                           uint64_t *beyond_dev, int32_t *scale_log2, double *vmax)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !long_dev || !trans_dev || !beyond_dev || !scale_log2 || !vmax) return fail(ctx, AMOF_EINVAL, "NULL argument");
    CurCall c(ctx, t, recip, hkl, K, dq, nbins);
    c.vel = vel;
    c.remove_com = remove_com != 0;
    c.windows = windows;
    c.W = n_windows;
    c.stride = origin_stride;
    CurOutputs out;
    out.counts_dev = counts_dev;
    out.lng_dev = long_dev;
    out.trn_dev = trans_dev;
    out.beyond_dev = beyond_dev;
    out.scale_log2 = scale_log2;
    out.vmax = vmax;
    return current_run(c, work_begin, work_end, out);
}
