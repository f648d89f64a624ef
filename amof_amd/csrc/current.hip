// Current correlation functions C_L(q, t) and C_T(q, t): the time correlation of j_a(k) = sum_j v_j exp(i k . r_j), projected
// along and across k (gfx950; amof_current_modes, amof_current_accumulate[_dev]).
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
//
// The host code is the lag scaffold of sq_call.h (shared with isf.hip) around C(q, t)'s own stages: the records, vmax and the
// flag fetched BEFORE the correlation, because the scales depend on vmax (they are uploaded late, on their own).  Rules:
// current_plan.h.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "current_plan.h"
#include "sq_call.h"

namespace amof {
namespace {

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
__device__ __forceinline__ void current_walk(const LagArgs &a, int v, const int32_t *__restrict__ hv, int lo, int hi, int64_t m,
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
        const double *__restrict__ j0 = a.tab + ((size_t)a.slot_of[k] * a.Kc + v) * row + (size_t)sa * 6;
        const double *__restrict__ j1 = a.tab + ((size_t)a.slot_of[km] * a.Kc + v) * row + (size_t)sc * 6;
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
__global__ __launch_bounds__(CUR_THREADS) void current_corr_kernel(LagArgs a)
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
                unsigned long long *lg = GLOBAL ? a.sum0 + (size_t)w * nbins : cw + nbins;
                unsigned long long *tg = GLOBAL ? a.sum1 + (size_t)w * nbins : cw + (size_t)(1 + S * S) * nbins;
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
                                          : j <= S2 ? &a.sum0[((size_t)(j - 1) * W + w) * nbins + b]
                                                    : &a.sum1[((size_t)(j - 1 - S2) * W + w) * nbins + b];
                atomicAdd(dst, val);
            }
            __syncthreads();
        }
    }
}

struct CurCorr {
    template <int ST, bool GLOBAL> static auto kernel() { return current_corr_kernel<ST, GLOBAL>; }
};

// --------------------------------------------------------------------------------------------- host code --
// counters: [counts | long | trans | beyond]; spans: records (means and vmax included), table, correlation
struct CurCall : LagCall {
    using LagCall::LagCall;
    const amof_traj *vel = nullptr;
    bool remove_com = false;
    CurSwitches csw = CurSwitches::from_env();
    size_t n_pair = 0;
    double total_mass = 0.0, vmax = 0.0;
    SqScales cs;
    int i_mass = -1;
    const double *vel_dev = nullptr;
    float4 *d_V = nullptr;              // SLOT_AUX2
    double *d_mean = nullptr;           // SLOT_AUX3
    uint32_t *d_vmax = nullptr;         // SLOT_AUX4
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

// the masses, the lag call's uploads and counters (lag_stage), the staged velocities and C(q, t)'s own scratch
int current_stage(CurCall &c, size_t rho_bytes, const LagOutputs *out)
{
    amof_ctx *ctx = c.ctx;
    if (c.remove_com) c.i_mass = c.pk.add(c.t->masses, (size_t)c.N * sizeof(double));
    AMOF_TRY(lag_stage(c, rho_bytes, out));
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
    AMOF_TRY(ensure(ctx, SLOT_AUX2, c.fr.fsel.size() * (size_t)std::max<int64_t>(c.N, 1) * sizeof(float4), &d_V));
    AMOF_TRY(ensure(ctx, SLOT_AUX3, (size_t)std::max<int64_t>(c.F, 1) * 3 * sizeof(double), &d_mean));
    AMOF_TRY(ensure(ctx, SLOT_AUX4, sizeof(uint32_t), &d_vmax));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_vmax, 0, sizeof(uint32_t), ctx->stream));
    c.d_V = (float4 *)d_V;
    c.d_mean = (double *)d_mean;
    c.d_vmax = (uint32_t *)d_vmax;
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

// sq_launch_rho with the samples beside the positions and rows of 6
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

int current_run(CurCall &c, int64_t wb, int64_t we, const LagOutputs &out, double *vmax)
{
    amof_ctx *ctx = c.ctx;
    AMOF_TRY(lag_check(c));
    AMOF_TRY(current_check_inputs(c));
    AMOF_TRY(lag_work(c, wb, we));
    c.n_pair = (size_t)c.S * c.S * c.n_cnt;
    AMOF_TRY(sq_check_histogram(c, 2 * c.n_pair));
    std::fill(out.scale_log2, out.scale_log2 + c.P, 0);
    *vmax = 0.0;
    lag_zero_host(c, out);
    if (c.K == 0 || c.F < 2 || c.N == 0) return AMOF_OK;

    AMOF_TRY(build_geometry(ctx, c.t, c.hg));
    AMOF_TRY(current_call_plan(c));
    isf_touched_frames(c.lagiv.data(), c.windows, c.W, c.F, c.stride, c.fr);
    if (c.n_entries > 0) current_cut_chunks(c.pl.runs, c.K, c.fr.fsel.size(), c.S, c.csw.rho_budget, c.ch);
    else c.ch.order_local.assign((size_t)c.K, 0);
    c.pass = current_pass_plan(c.S, c.nbins, c.W, c.csw);
    AMOF_TRY(current_stage(c, c.n_entries > 0 ? (size_t)c.ch.kc_top * c.ch.vec_bytes : 0, &out));
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
    *vmax = c.vmax;
    sq_expand_pairs(c.S, c.cs, c.scale2, c.sexp2);
    if (c.n_entries > 0) {              // (vmax == 0: scale 0, the samples are still counted)
        void *d_scale2 = nullptr;
        AMOF_TRY(upload(ctx, SLOT_AUX6, c.scale2.data(), c.scale2.size() * sizeof(double), &d_scale2));
        AMOF_TRY(lag_chunk_loop(
            c, lag_kernel_args(c, (const double *)d_scale2, c.sums, c.sums + c.n_pair), 1, 1, 2,
            [&](const IsfChunk &k, int64_t *launches) {
                return current_launch_rho(c, k.r0, k.r1 - k.r0, c.pk.ptr<int32_t>(c.i_olocal), k.nv, launches);
            },
            [&](const LagArgs &a, dim3 grid) { return lag_launch_corr<CurCorr>(ctx, a, grid, c.pass); }));
    }
    return lag_finish(c, out);
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
    AMOF_TRY(current_stage(c, n_out * sizeof(double), nullptr));
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

// one of the two forms: host (f64, overwritten) or device (int64 fixed point / u64, added into)
int current_entry(amof_ctx *ctx, const amof_traj *t, const amof_traj *vel, int32_t remove_com, const double *recip,
                  const int32_t *hkl, int32_t K, const int32_t *windows, int32_t n_windows, int64_t origin_stride,
                  int64_t work_begin, int64_t work_end, double dq, int32_t nbins, LagOutputs &out, int32_t *scale_log2, double *vmax)
{
    CurCall c(ctx, t, recip, hkl, K, dq, nbins);
    c.vel = vel;
    c.remove_com = remove_com != 0;
    c.windows = windows;
    c.W = n_windows;
    c.stride = origin_stride;
    out.scale_log2 = scale_log2;
    return current_run(c, work_begin, work_end, out, vmax);
}

}  // namespace
}  // namespace amof

using namespace amof;

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
    LagOutputs out;
    out.counts = counts;
    out.beyond = beyond;
    out.blocks = {LagSums{nullptr, long_sums, false}, LagSums{nullptr, trans_sums, false}};
    return current_entry(ctx, t, vel, remove_com, recip, hkl, K, windows, n_windows, origin_stride, work_begin, work_end, dq, nbins,
                         out, scale_log2, vmax);
}

extern "C" int amof_current_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const amof_traj *vel, int32_t remove_com,
                                           const double *recip, const int32_t *hkl, int32_t K, const int32_t *windows,
                                           int32_t n_windows, int64_t origin_stride, int64_t work_begin, int64_t work_end,
                                           double dq, int32_t nbins, uint64_t *counts_dev, int64_t *long_dev, int64_t *trans_dev,
                                           uint64_t *beyond_dev, int32_t *scale_log2, double *vmax)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !long_dev || !trans_dev || !beyond_dev || !scale_log2 || !vmax) return fail(ctx, AMOF_EINVAL, "NULL argument");
    LagOutputs out;
    out.counts_dev = counts_dev;
    out.beyond_dev = beyond_dev;
    out.blocks = {LagSums{long_dev, nullptr, false}, LagSums{trans_dev, nullptr, false}};
    return current_entry(ctx, t, vel, remove_com, recip, hkl, K, windows, n_windows, origin_stride, work_begin, work_end, dq, nbins,
                         out, scale_log2, vmax);
}
