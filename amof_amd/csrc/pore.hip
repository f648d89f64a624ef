// Pore geometry on a grid (gfx950): the distance of every grid point of the cell to the nearest atomic surface,
//     v(p) = min_j sqrt(d2(r_j - p)) - R_j        (canonical minimum image, include/amof_hip.h amof_pore_field)
// and from it the per-frame histogram, the probe-centre counts and the largest included sphere.  The reference's Pore
// (amof/pore.py) writes a CIF per frame and starts the external Zeo++ binary on it; nothing of that is reproduced -- this is
// the deterministic grid version of the same geometric quantities.
//
//   pore_exact   one thread per grid point, every atom of the frame through LDS tiles, canonical float64 arithmetic
//   pore_brick   a workgroup owns a brick of 8 x 8 x 8 grid points.  It walks the cells of a 3-D cell list (launch_cell_sort)
//                within reach of the brick centre, every periodic image on its own, and keeps the images that can matter
//                to any point of the brick as float32 records (x, y, z relative to the centre, R) in LDS.  Every lane
//                sweeps the list twice for its two points: once for the float32 candidate minimum (pore_math.h: no root
//                unless the minimum moves), once to re-evaluate in the canonical float64 arithmetic, from the raw
//                positions, every atom whose candidate lies within 2 eps_c of that minimum.  The true nearest atom is
//                among those, so the field value is the canonical one: bit-identical to pore_exact.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "pore_math.h"

namespace amof {

constexpr int PORE_THREADS = 256;
constexpr int PORE_PPL = PORE_BRICK * PORE_BRICK * PORE_BRICK / PORE_THREADS;     // grid points per lane
constexpr int PORE_LIST_CAP = 2048;         // atom images a brick keeps (a fuller brick sends the call to pore_exact)
constexpr int PORE_CELL_EDGE_MAX = 32;      // cells per axis of the cell list
constexpr uint32_t PORE_ATOM_MASK = (1u << CELL_SPECIES_SHIFT) - 1u;
static_assert(PORE_PPL == 2, "pore_brick_kernel is written for two points per lane");
static_assert(AMOF_PORE_MAX_WORDS % 2 == 0, "the thresholds follow the counters in LDS, 8-byte aligned");

struct PoreArgs {
    const double *pos;
    const double *geom;
    const double *pcell;        // [n_cells][4]: half-diagonal, 2 eps_c (a float, rounded up), gather reach, keep radius
    const double *radii;        // [S]
    const double *thr;          // [n_t]
    const int32_t *species;     // [N]
    const QAtom *Q;             // [nf][N] cell-sorted records
    const uint32_t *start3;     // [nf][nkeys + 1]
    int64_t N;
    int64_t G;
    int32_t n_cells, S, f_base, nf;
    int32_t n[3];               // grid
    int32_t nb[3];              // bricks per axis
    int32_t nc[3];              // cell list
    int32_t nbins, n_t;
    double dr, dmax;
    unsigned long long *hist;   // [F][nbins + 2]
    unsigned long long *counts; // [F][n_t]
    double *part_v;             // [nf][workgroups] largest field value of a workgroup and its smallest linear index
    int32_t *part_i;
    double *field;              // [nf][G] or null
    int32_t *flags;             // [0] quantiser (far atoms, cell table), [1] a brick's list is full
};

// the documented rule: [0] v < 0, [1 + b] b = (int)(v / dr) < nbins for 0 <= v < dmax, [nbins + 1] everything else
__device__ __forceinline__ void pore_count(const PoreArgs &a, unsigned *lh, const double *lthr, double v)
{
    int slot = a.nbins + 1;
    if (v < 0.0) slot = 0;
    else if (v < a.dmax) {
        const int b = (int)(v / a.dr);
        if (b < a.nbins) slot = 1 + b;
    }
    atomicAdd(&lh[slot], 1u);
    for (int t = 0; t < a.n_t; t++)
        if (v >= lthr[t]) atomicAdd(&lh[a.nbins + 2 + t], 1u);
}

__device__ __forceinline__ void pore_better(double &bv, int &bi, double ov, int oi)
{
    if (ov > bv || (ov == bv && oi < bi)) {
        bv = ov;
        bi = oi;
    }
}

// end of a workgroup: its largest value (ties: smallest index) to the partial table, its counters to the frame's row
__device__ __forceinline__ void pore_finish(const PoreArgs &a, unsigned *lh, double *sv, int *si, int fl, double bv, int bi)
{
    const int tid = threadIdx.x;
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off, 64);
        const int oi = __shfl_down(bi, off, 64);
        pore_better(bv, bi, ov, oi);
    }
    if ((tid & 63) == 0) {
        sv[tid >> 6] = bv;
        si[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PORE_THREADS / 64; w++) pore_better(bv, bi, sv[w], si[w]);
        a.part_v[(size_t)fl * gridDim.x + blockIdx.x] = bv;
        a.part_i[(size_t)fl * gridDim.x + blockIdx.x] = bi;
    }
    const size_t f = (size_t)a.f_base + fl;
    for (int w = tid; w < a.nbins + 2 + a.n_t; w += PORE_THREADS) {
        const unsigned c = lh[w];
        if (!c) continue;
        if (w < a.nbins + 2) atomicAdd(&a.hist[f * (size_t)(a.nbins + 2) + w], (unsigned long long)c);
        else atomicAdd(&a.counts[f * (size_t)a.n_t + (w - a.nbins - 2)], (unsigned long long)c);
    }
}

__device__ __forceinline__ void pore_lds_init(const PoreArgs &a, unsigned *lh, double *lthr)
{
    for (int w = threadIdx.x; w < a.nbins + 2 + a.n_t; w += PORE_THREADS) lh[w] = 0u;
    for (int t = threadIdx.x; t < a.n_t; t += PORE_THREADS) lthr[t] = a.thr[t];
}

// grid point (i, j, k) of the frame's cell: plain products and sums in this order (numpy restates it bit for bit)
__device__ __forceinline__ void pore_point(const PoreArgs &a, const double *__restrict__ g, int i, int j, int k, double &px, double &py,
                                           double &pz)
{
    const double fx = ((double)i + 0.5) / (double)a.n[0], fy = ((double)j + 0.5) / (double)a.n[1], fz = ((double)k + 0.5) / (double)a.n[2];
    px = (fx * g[0] + fy * g[3]) + fz * g[6];
    py = (fx * g[1] + fy * g[4]) + fz * g[7];
    pz = (fx * g[2] + fy * g[5]) + fz * g[8];
}

// ---------------------------------------------------------------- exact ----
template <bool ORTHO>
__global__ __launch_bounds__(PORE_THREADS) void pore_exact_kernel(PoreArgs a)
{
    extern __shared__ __align__(16) unsigned char pore_raw[];
    unsigned *lh = reinterpret_cast<unsigned *>(pore_raw);
    double *lthr = reinterpret_cast<double *>(lh + AMOF_PORE_MAX_WORDS);
    __shared__ double tx[PORE_THREADS], ty[PORE_THREADS], tz[PORE_THREADS], tr[PORE_THREADS];
    __shared__ double sv[PORE_THREADS / 64];
    __shared__ int si[PORE_THREADS / 64];
    const int tid = threadIdx.x, fl = blockIdx.y, f = a.f_base + fl;
    const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
    pore_lds_init(a, lh, lthr);
    const int64_t lin = (int64_t)blockIdx.x * PORE_THREADS + tid;
    const bool valid = lin < a.G;
    double px = 0.0, py = 0.0, pz = 0.0;
    if (valid) {
        const int k = (int)(lin % a.n[2]);
        const int64_t ij = lin / a.n[2];
        pore_point(a, g, (int)(ij / a.n[1]), (int)(ij % a.n[1]), k, px, py, pz);
    }
    double m = INFINITY;
    for (int64_t j0 = 0; j0 < a.N; j0 += PORE_THREADS) {
        const int cnt = (int)min((int64_t)PORE_THREADS, a.N - j0);
        __syncthreads();
        if (tid < cnt) {
            tx[tid] = p[(j0 + tid) * 3 + 0];
            ty[tid] = p[(j0 + tid) * 3 + 1];
            tz[tid] = p[(j0 + tid) * 3 + 2];
            tr[tid] = a.radii[a.species[j0 + tid]];
        }
        __syncthreads();
        if (valid) {
            for (int j = 0; j < cnt; j++) {
                double dx, dy, dz;
                pair_base<ORTHO>(g, tx[j] - px, ty[j] - py, tz[j] - pz, dx, dy, dz);
                m = fmin(m, sqrt(norm2(dx, dy, dz)) - tr[j]);
            }
        }
    }
    __syncthreads();        // (the counters are zero even where N == 0)
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    if (valid) {
        const double v = m < a.dmax ? m : a.dmax;
        if (a.field) a.field[(size_t)fl * (size_t)a.G + (size_t)lin] = v;
        pore_count(a, lh, lthr, v);
        bv = v;
        bi = (int)lin;
    }
    __syncthreads();
    pore_finish(a, lh, sv, si, fl, bv, bi);
}

// ---------------------------------------------------------------- brick ----
__device__ __forceinline__ int pore_floor_div(int x, int n)
{
    const int q = x / n;
    return (x % n != 0 && x < 0) ? q - 1 : q;
}

template <bool ORTHO>
__global__ __launch_bounds__(PORE_THREADS) void pore_brick_kernel(PoreArgs a)
{
    extern __shared__ __align__(16) unsigned char pore_raw[];
    unsigned *lh = reinterpret_cast<unsigned *>(pore_raw);
    double *lthr = reinterpret_cast<double *>(lh + AMOF_PORE_MAX_WORDS);
    __shared__ float4 rec[PORE_LIST_CAP];            // image - centre (x, y, z) and the radius, float32
    __shared__ uint32_t ridx[PORE_LIST_CAP];         // species << CELL_SPECIES_SHIFT | atom
    __shared__ unsigned n_list;
    __shared__ double sv[PORE_THREADS / 64];
    __shared__ int si[PORE_THREADS / 64];
    const int tid = threadIdx.x, fl = blockIdx.y, f = a.f_base + fl;
    const int gi = a.n_cells == 1 ? 0 : f;
    const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
    const double *__restrict__ pc = a.pcell + (size_t)gi * 4;
    const double *__restrict__ pos = a.pos + (size_t)f * (size_t)a.N * 3;
    pore_lds_init(a, lh, lthr);
    if (tid == 0) n_list = 0u;

    const int wg = blockIdx.x;
    const int b2 = wg % a.nb[2], b1 = (wg / a.nb[2]) % a.nb[1], b0 = wg / (a.nb[2] * a.nb[1]);
    const int i0[3] = {b0 * PORE_BRICK, b1 * PORE_BRICK, b2 * PORE_BRICK};
    // centre of the (full) brick: fractional, Cartesian
    double fc[3], cc[3];
    for (int k = 0; k < 3; k++) fc[k] = ((double)i0[k] + 0.5 * PORE_BRICK) / (double)a.n[k];
    for (int c = 0; c < 3; c++) cc[c] = (fc[0] * g[c] + fc[1] * g[3 + c]) + fc[2] * g[6 + c];

    // ---- gather: the cells within reach of the centre, every periodic image by itself
    int lo[3], cnt[3];
    for (int k = 0; k < 3; k++) {
        const double rho = pc[2] / g[18 + k];
        lo[k] = (int)floor((fc[k] - rho) * (double)a.nc[k]);
        cnt[k] = (int)floor((fc[k] + rho) * (double)a.nc[k]) - lo[k] + 1;
    }
    const int total = cnt[0] * cnt[1] * cnt[2];
    const int nkeys = a.nc[0] * a.nc[1] * a.nc[2] * a.S;
    const uint32_t *__restrict__ st = a.start3 + (size_t)fl * (size_t)(nkeys + 1);
    const QAtom *__restrict__ Qf = a.Q + (size_t)fl * (size_t)a.N;
    __syncthreads();
    for (int e = tid; e < total; e += PORE_THREADS) {
        const int ex = lo[0] + e % cnt[0], ey = lo[1] + (e / cnt[0]) % cnt[1], ez = lo[2] + e / (cnt[0] * cnt[1]);
        const int sx = pore_floor_div(ex, a.nc[0]), sy = pore_floor_div(ey, a.nc[1]), sz = pore_floor_div(ez, a.nc[2]);
        const int cell = ((ez - sz * a.nc[2]) * a.nc[1] + (ey - sy * a.nc[1])) * a.nc[0] + (ex - sx * a.nc[0]);
        const uint32_t k0 = st[(size_t)cell * a.S];
        const uint32_t k1 = min(st[(size_t)(cell + 1) * a.S], (uint32_t)a.N);
        for (uint32_t k = k0; k < k1; k++) {
            const QAtom q = Qf[k];
            const int sp = min((int)(q.idx >> CELL_SPECIES_SHIFT), a.S - 1);
            const double d0 = ((double)q.ux * (1.0 / 4294967296.0) + (double)sx) - fc[0];
            const double d1 = ((double)q.uy * (1.0 / 4294967296.0) + (double)sy) - fc[1];
            const double d2 = ((double)q.uz * (1.0 / 4294967296.0) + (double)sz) - fc[2];
            const double Ax = (d0 * g[0] + d1 * g[3]) + d2 * g[6];
            const double Ay = (d0 * g[1] + d1 * g[4]) + d2 * g[7];
            const double Az = (d0 * g[2] + d1 * g[5]) + d2 * g[8];
            const double R = a.radii[sp];
            if (sqrt(Ax * Ax + Ay * Ay + Az * Az) - R < pc[3]) {
                const unsigned slot = atomicAdd(&n_list, 1u);
                if (slot < (unsigned)PORE_LIST_CAP) {
                    rec[slot] = make_float4((float)Ax, (float)Ay, (float)Az, (float)R);
                    ridx[slot] = q.idx;
                }
            }
        }
    }
    __syncthreads();
    int n = (int)n_list;
    if (n > PORE_LIST_CAP) {
        if (tid == 0) a.flags[1] = 1;       // (the host discards the call's results and runs pore_exact)
        n = PORE_LIST_CAP;
    }

    // ---- this lane's points
    bool valid[PORE_PPL];
    int lin[PORE_PPL];
    double P[PORE_PPL][3];
    float pf[PORE_PPL][3];
#pragma unroll
    for (int q = 0; q < PORE_PPL; q++) {
        const int l = tid + q * PORE_THREADS;
        const int i = i0[0] + (l >> 6), j = i0[1] + ((l >> 3) & 7), k = i0[2] + (l & 7);
        valid[q] = i < a.n[0] && j < a.n[1] && k < a.n[2];
        lin[q] = valid[q] ? (i * a.n[1] + j) * a.n[2] + k : 0x7fffffff;
        pore_point(a, g, i, j, k, P[q][0], P[q][1], P[q][2]);
#pragma unroll
        for (int c = 0; c < 3; c++) pf[q][c] = (float)(P[q][c] - cc[c]);
    }

    // ---- sweep 1: the candidate minimum.  An atom is looked at only if d2 < (m + R)^2, i.e. if it could lower m
    // (a spurious pass, m + R < 0, costs a root and changes nothing); m starts at dmax rounded up.
    const float m_init = (float)a.dmax * (1.0f + 1.2e-7f);
    float m0 = m_init, m1 = m_init;
    for (int j = 0; j < n; j++) {
        const float4 r = rec[j];
        const float q0 = pore_cand_d2(r.x, r.y, r.z, pf[0][0], pf[0][1], pf[0][2]);
        const float q1 = pore_cand_d2(r.x, r.y, r.z, pf[1][0], pf[1][1], pf[1][2]);
        if (pore_could_lower(q0, m0, r.w)) m0 = fminf(m0, pore_cand(q0, r.w));
        if (pore_could_lower(q1, m1, r.w)) m1 = fminf(m1, pore_cand(q1, r.w));
    }

    // ---- sweep 2: every atom whose candidate is within 2 eps_c of the minimum (pore_selected, pore_math.h) in canonical
    // float64 from the raw positions.  The atom with the smallest canonical value is among them: its candidate is at most
    // eps_c above its value, which is at most any other atom's value, which is at most eps_c above that atom's candidate.
    const float e2 = (float)pc[1];
    const float mm[PORE_PPL] = {m0 + e2, m1 + e2};
    double best[PORE_PPL] = {INFINITY, INFINITY};
    for (int j = 0; j < n; j++) {
        const float4 r = rec[j];
#pragma unroll
        for (int q = 0; q < PORE_PPL; q++) {
            const float d2 = pore_cand_d2(r.x, r.y, r.z, pf[q][0], pf[q][1], pf[q][2]);
            if (valid[q] && pore_selected(d2, mm[q], r.w)) {
                const uint32_t id = ridx[j];
                const int64_t at = min((int64_t)(id & PORE_ATOM_MASK), a.N - 1);
                const int sp = min((int)(id >> CELL_SPECIES_SHIFT), a.S - 1);
                double dx, dy, dz;
                pair_base<ORTHO>(g, pos[at * 3] - P[q][0], pos[at * 3 + 1] - P[q][1], pos[at * 3 + 2] - P[q][2], dx, dy, dz);
                best[q] = fmin(best[q], sqrt(norm2(dx, dy, dz)) - a.radii[sp]);
            }
        }
    }

    double bv = -INFINITY;
    int bi = 0x7fffffff;
#pragma unroll
    for (int q = 0; q < PORE_PPL; q++) {
        if (!valid[q]) continue;
        const double v = best[q] < a.dmax ? best[q] : a.dmax;
        if (a.field) a.field[(size_t)fl * (size_t)a.G + (size_t)lin[q]] = v;
        pore_count(a, lh, lthr, v);
        pore_better(bv, bi, v, lin[q]);
    }
    __syncthreads();
    pore_finish(a, lh, sv, si, fl, bv, bi);
}

// one workgroup per frame: the frame's largest value and its smallest index from the workgroups' partials
__global__ __launch_bounds__(PORE_THREADS) void pore_vmax_kernel(const double *__restrict__ part_v, const int32_t *__restrict__ part_i,
                                                                 int nwg, int f_base, double *__restrict__ vmax,
                                                                 long long *__restrict__ argmax)
{
    __shared__ double sv[PORE_THREADS / 64];
    __shared__ int si[PORE_THREADS / 64];
    const int tid = threadIdx.x, fl = blockIdx.x;
    double bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int w = tid; w < nwg; w += PORE_THREADS) pore_better(bv, bi, part_v[(size_t)fl * nwg + w], part_i[(size_t)fl * nwg + w]);
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_down(bv, off, 64);
        const int oi = __shfl_down(bi, off, 64);
        pore_better(bv, bi, ov, oi);
    }
    if ((tid & 63) == 0) {
        sv[tid >> 6] = bv;
        si[tid >> 6] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PORE_THREADS / 64; w++) pore_better(bv, bi, sv[w], si[w]);
        vmax[f_base + fl] = bv;
        argmax[f_base + fl] = (long long)bi;
    }
}

// ------------------------------------------------------------ host side ----
struct PoreCall {
    amof_ctx *ctx;
    const amof_traj *t;
    HostGeom geom;
    Stager stage;
    PoreArgs a;
    StageSpans *spans = nullptr;
    int64_t G = 0;
    size_t out_bytes = 0;       // rows, counts, vmax, argmax of all frames: one device buffer
    void *d_out = nullptr;
    double *d_vmax = nullptr;
    long long *d_argmax = nullptr;
    double *field_host = nullptr;
    int64_t batch_cap = 0;      // AMOF_PORE_BATCH (0: none)
    PoreStages *stages = nullptr;       // the batch's field stays on the device and goes through them frame by frame
};

static size_t pore_lds(const PoreArgs &a)
{
    return (size_t)AMOF_PORE_MAX_WORDS * sizeof(unsigned) + (size_t)a.n_t * sizeof(double);
}

template <typename Kernel>
static hipError_t pore_launch(Kernel kern, dim3 grid, size_t lds, hipStream_t stream, const PoreArgs &a)
{
    const hipError_t e = allow_max_lds((const void *)kern);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, dim3(PORE_THREADS), lds, stream, a);
    return hipGetLastError();
}

// frames per batch: the partial table, the field (if asked for) and `per_frame` more bytes of scratch within 1 GiB
static int64_t pore_batch(const PoreCall &c, int64_t nwg, size_t per_frame)
{
    per_frame += (size_t)nwg * (sizeof(double) + sizeof(int32_t)) + (c.field_host || c.stages ? (size_t)c.G * sizeof(double) : 0);
    const size_t budget = ((size_t)1 << 30) - std::min<size_t>(c.stages ? c.stages->fixed_bytes() : 0, (size_t)1 << 29);
    int64_t FB = std::max<int64_t>(1, (int64_t)budget / (int64_t)std::max<size_t>(1, per_frame));
    FB = std::min<int64_t>(std::min<int64_t>(FB, 32768), c.t->n_frames);
    if (c.batch_cap > 0) FB = std::min(FB, c.batch_cap);
    return FB;
}

// per batch: partial table and field buffer, the launch, the frame reduction, the field back to the host
template <typename Launch>
static int pore_batches(PoreCall &c, int64_t nwg, int64_t FB, Launch &&launch)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    PoreArgs &a = c.a;
    void *d_pv, *d_pi, *d_field = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX2, (size_t)FB * nwg * sizeof(double), &d_pv));
    AMOF_TRY(ensure(ctx, SLOT_AUX3, (size_t)FB * nwg * sizeof(int32_t), &d_pi));
    if (c.field_host || c.stages) AMOF_TRY(ensure(ctx, SLOT_OUT1, (size_t)FB * (size_t)c.G * sizeof(double), &d_field));
    a.part_v = (double *)d_pv;
    a.part_i = (int32_t *)d_pi;
    a.field = (double *)d_field;
    AMOF_HIP_TRY(ctx, hipMemsetAsync(c.d_out, 0, c.out_bytes, ctx->stream));
    int64_t launches = 0;
    for (int64_t fb = 0; fb < t->n_frames; fb += FB) {
        const int64_t nf = std::min<int64_t>(FB, t->n_frames - fb);
        AMOF_TRY(stager_need(c.stage, fb + nf));
        a.f_base = (int32_t)fb;
        a.nf = (int32_t)nf;
        AMOF_TRY(launch(fb, nf, launches == 0));
        hipLaunchKernelGGL(pore_vmax_kernel, dim3((unsigned)nf), dim3(PORE_THREADS), 0, ctx->stream, (const double *)a.part_v,
                           (const int32_t *)a.part_i, (int)nwg, (int)fb, c.d_vmax, c.d_argmax);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        launches++;
        if (c.field_host) AMOF_TRY(fetch(ctx, c.field_host + (size_t)fb * (size_t)c.G, d_field, (size_t)nf * (size_t)c.G * sizeof(double)));
        for (int64_t f = fb; c.stages && f < fb + nf; f++)
            AMOF_TRY(c.stages->frame(f, (const double *)d_field + (size_t)(f - fb) * (size_t)c.G, *c.spans));
    }
    timing_dom_end(ctx, launches);
    return AMOF_OK;
}

static int pore_exact_tier(PoreCall &c)
{
    amof_ctx *ctx = c.ctx;
    PoreArgs &a = c.a;
    const int64_t nwg = (c.G + PORE_THREADS - 1) / PORE_THREADS;
    const int64_t FB = pore_batch(c, nwg, 0);
    const bool ortho = c.geom.all_ortho;
    return pore_batches(c, nwg, FB, [&](int64_t, int64_t nf, bool first) {
        if (first) timing_dom_begin(ctx, "pore_exact");
        if (c.spans) c.spans->begin(1);
        const dim3 grid((unsigned)nwg, (unsigned)nf);
        AMOF_HIP_TRY(ctx, ortho ? pore_launch(pore_exact_kernel<true>, grid, pore_lds(a), ctx->stream, a)
                                : pore_launch(pore_exact_kernel<false>, grid, pore_lds(a), ctx->stream, a));
        if (c.spans) c.spans->end();
        return (int)AMOF_OK;
    });
}

// whether pore_brick applies, and its tables: pcell [n_cells][4], the cell list's grid
static bool pore_brick_plan(PoreCall &c, double rcut, std::vector<double> &pcell)
{
    const amof_traj *t = c.t;
    PoreArgs &a = c.a;
    if (!(t->pbc[0] && t->pbc[1] && t->pbc[2])) return false;       // (an open axis has no fractional coordinate to sort by)
    if (t->n_atoms < 1 || t->n_atoms >= (1ll << CELL_SPECIES_SHIFT) || t->n_species > 64) return false;      // (the cell sort's limits)
    double hmin[3] = {INFINITY, INFINITY, INFINITY};
    pcell.assign((size_t)t->n_cells * 4, 0.0);
    for (int64_t k = 0; k < t->n_cells; k++) {
        const double *rec = c.geom.rec.data() + (size_t)k * GEOM_STRIDE;
        const double hd = pore_brick_half_diag(rec, a.n);
        if (!(hd <= PORE_HALF_DIAG_MAX * rcut)) return false;
        for (int x = 0; x < 3; x++) hmin[x] = std::min(hmin[x], rec[18 + x]);
        const float e2 = (float)(2.0 * pore_candidate_bound(rec, rcut)) * (1.0f + 2.4e-7f);
        pcell[(size_t)k * 4 + 0] = hd;
        pcell[(size_t)k * 4 + 1] = (double)e2;
        pcell[(size_t)k * 4 + 2] = (rcut + hd) * (1.0 + 1e-6) + 1e-6;       // cells within this of the centre are walked
        pcell[(size_t)k * 4 + 3] = (a.dmax + hd) * (1.0 + 1e-6) + 1e-6;     // images with |A| - R below this are kept
    }
    for (int x = 0; x < 3; x++) {
        a.nc[x] = (int)std::max(1.0, std::min((double)PORE_CELL_EDGE_MAX, floor(hmin[x] / 3.0)));
        a.nb[x] = (a.n[x] + PORE_BRICK - 1) / PORE_BRICK;
    }
    return (int64_t)a.nb[0] * a.nb[1] * a.nb[2] <= 0x7fffffffLL;
}

static int pore_brick_tier(PoreCall &c, double rcut, bool &done)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    PoreArgs &a = c.a;
    std::vector<double> pcell;
    done = false;
    if (!pore_brick_plan(c, rcut, pcell)) return AMOF_OK;
    void *d_pcell, *d_Q, *d_start, *d_keys, *d_cursor;
    AMOF_TRY(upload(ctx, SLOT_AUX5, pcell.data(), pcell.size() * sizeof(double), &d_pcell));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));        // (pcell leaves scope with this function; the copy may be pageable)
    a.pcell = (const double *)d_pcell;
    const int64_t nkeys = (int64_t)a.nc[0] * a.nc[1] * a.nc[2] * a.S;
    const int64_t nwg = (int64_t)a.nb[0] * a.nb[1] * a.nb[2];
    const size_t per_frame = (size_t)t->n_atoms * (sizeof(QAtom) + sizeof(uint32_t)) + (size_t)(2 * nkeys + 1) * sizeof(uint32_t);
    const int64_t FB = pore_batch(c, nwg, per_frame);
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)FB * t->n_atoms * sizeof(QAtom), &d_Q));
    AMOF_TRY(ensure(ctx, SLOT_AUX7, (size_t)FB * (nkeys + 1) * sizeof(uint32_t), &d_start));
    AMOF_TRY(ensure(ctx, SLOT_AUX6, (size_t)FB * t->n_atoms * sizeof(uint32_t), &d_keys));
    AMOF_TRY(ensure(ctx, SLOT_AUX9, (size_t)FB * nkeys * sizeof(uint32_t), &d_cursor));
    a.Q = (const QAtom *)d_Q;
    a.start3 = (const uint32_t *)d_start;
    AMOF_HIP_TRY(ctx, hipMemsetAsync(a.flags, 0, 2 * sizeof(int32_t), ctx->stream));
    const bool ortho = c.geom.all_ortho;
    AMOF_TRY(pore_batches(c, nwg, FB, [&](int64_t fb, int64_t nf, bool first) {
        if (c.spans) c.spans->begin(0);
        AMOF_TRY(launch_cell_sort(ctx, a.pos, a.geom, (int)t->n_cells, a.species, a.S, t->n_atoms, (int)fb, (int)nf, a.nc[0], a.nc[1],
                                  a.nc[2], (QAtom *)d_Q, (uint32_t *)d_start, (uint32_t *)d_keys, (uint32_t *)d_cursor, a.flags));
        if (c.spans) c.spans->end();
        if (first) timing_dom_begin(ctx, "pore_brick");
        if (c.spans) c.spans->begin(1);
        const dim3 grid((unsigned)nwg, (unsigned)nf);
        AMOF_HIP_TRY(ctx, ortho ? pore_launch(pore_brick_kernel<true>, grid, pore_lds(a), ctx->stream, a)
                                : pore_launch(pore_brick_kernel<false>, grid, pore_lds(a), ctx->stream, a));
        if (c.spans) c.spans->end();
        return (int)AMOF_OK;
    }));
    int32_t flags[2];
    AMOF_TRY(fetch(ctx, flags, a.flags, sizeof flags));
    // atoms absurdly far from the cell, a cell table the sort could not build, a brick with more images than its list holds
    done = !flags[0] && !flags[1];
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

extern "C" double amof_pore_candidate_bound(const double *cell, double rcut)
{
    return cell ? pore_candidate_bound(cell, rcut) : -1.0;
}

// ---- field source 1: atoms.  amof_pore_field; with stages every batch's field stays in device memory and goes through them
int amof::pore_field_run(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out, PoreStages *stages)
{
    if (!ctx) return AMOF_EINVAL;
    PoreCall c;
    c.ctx = ctx;
    c.stages = stages;
    const amof_traj *t = c.t = in.t;
    double rmax = 0.0, nb = 0.0, hmin = INFINITY;       // hmin: the smallest perpendicular height on a periodic axis
    AMOF_TRY(validate_traj(ctx, t, false));
    AMOF_TRY(pore_refuse(ctx, pore_check::both_given(in.radii, in.grid)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_given(in.thresholds, in.n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::field_outputs(t->n_frames, in.n_t, out.hist, out.counts, out.vmax, out.argmax)));
    AMOF_TRY(pore_refuse(ctx, pore_check::grid(in.grid, nullptr)));
    AMOF_TRY(pore_refuse(ctx, pore_check::bin_width(in.dr, in.dmax, nb)));
    AMOF_TRY(pore_refuse(ctx, pore_check::radii(in.radii, t->n_species, rmax)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_finite(in.thresholds, in.n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::counter_words(nb, in.n_t, out.nbins)));
    out.sized(t->n_frames, in.grid, in.n_t);        // (whatever refuses from here on leaves zeros)
    const int64_t F = out.F;
    if (F == 0) return AMOF_OK;
    AMOF_TRY(build_geometry(ctx, t, c.geom));
    for (int64_t k = 0; k < t->n_cells; k++)
        for (int x = 0; x < 3; x++)
            if (t->pbc[x]) hmin = std::min(hmin, c.geom.rec[(size_t)k * GEOM_STRIDE + 18 + x]);
    AMOF_TRY(pore_refuse(ctx, pore_check::half_height_atoms(in.dmax, rmax, hmin)));
    if (out.field) AMOF_TRY(pore_refuse(ctx, pore_check::per_point_cap(out.G, "field")));
    const int S = t->n_species;
    const int32_t nbins = out.nbins, n_t = in.n_t;
    c.G = out.G;
    c.field_host = out.field;
    if (const char *be = getenv("AMOF_PORE_BATCH")) c.batch_cap = std::max(1, atoi(be));
    out.zero(false);

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    AMOF_TRY(stager_begin(ctx, t, true, c.stage));
    StageSpans spans(ctx);      // cell sort, field kernel, the stages' kernels
    c.spans = &spans;
    UploadPack pk;
    const int i_geom = pk.add(c.geom.rec.data(), c.geom.rec.size() * sizeof(double));
    const int i_rad = pk.add(in.radii, (size_t)S * sizeof(double));
    const int i_thr = pk.add(in.thresholds, (size_t)n_t * sizeof(double));
    const int i_sp = pk.add(t->species, (size_t)t->n_atoms * sizeof(int32_t));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    const size_t hist_bytes = (size_t)F * (nbins + 2) * sizeof(uint64_t), cnt_bytes = (size_t)F * n_t * sizeof(int64_t);
    c.out_bytes = hist_bytes + cnt_bytes + (size_t)F * (sizeof(double) + sizeof(long long));
    void *d_flags;
    AMOF_TRY(ensure(ctx, SLOT_OUT0, c.out_bytes, &c.d_out));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, 2 * sizeof(int32_t), &d_flags));
    PoreArgs &a = c.a;
    memset(&a, 0, sizeof a);
    a.pos = c.stage.dev;
    a.geom = pk.ptr<double>(i_geom);
    a.radii = pk.ptr<double>(i_rad);
    a.thr = pk.ptr<double>(i_thr);
    a.species = pk.ptr<int32_t>(i_sp);
    a.N = t->n_atoms;
    a.G = c.G;
    a.n_cells = (int32_t)t->n_cells;
    a.S = S;
    for (int k = 0; k < 3; k++) a.n[k] = in.grid[k];
    a.nbins = nbins;
    a.n_t = n_t;
    a.dr = in.dr;
    a.dmax = in.dmax;
    a.hist = (unsigned long long *)c.d_out;
    a.counts = (unsigned long long *)((unsigned char *)c.d_out + hist_bytes);
    c.d_vmax = (double *)((unsigned char *)c.d_out + hist_bytes + cnt_bytes);
    c.d_argmax = (long long *)(c.d_vmax + F);
    a.flags = (int32_t *)d_flags;
    const PoreAtoms atoms{a.pos, a.geom, a.radii, a.species, &c.geom, rmax, hmin};
    if (stages) AMOF_TRY(stages->setup(&atoms));

    bool done = false;
    const char *ex = getenv("AMOF_PORE_EXACT");
    if (!(ex && ex[0] == '1')) AMOF_TRY(pore_brick_tier(c, in.dmax + rmax, done));
    if (!done) {
        if (stages) stages->restart();      // (nothing to take back where pore_brick never started)
        AMOF_TRY(stager_need(c.stage, F));
        AMOF_TRY(pore_exact_tier(c));
    }
    timing_end(ctx);
    AMOF_TRY(fetch(ctx, out.hist, a.hist, hist_bytes));
    AMOF_TRY(fetch(ctx, out.counts, a.counts, cnt_bytes));
    AMOF_TRY(fetch(ctx, out.vmax, c.d_vmax, (size_t)F * sizeof(double)));
    AMOF_TRY(fetch(ctx, out.argmax, c.d_argmax, (size_t)F * sizeof(long long)));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    if (stages) stages->report();
    return AMOF_OK;
}

// ---- field source 2: a field the caller supplies (its arguments checked by the entry point)
int amof::pore_given_field_run(amof_ctx *ctx, const PoreInputs &in, const PoreOutputs &out, PoreStages &stages, const char *path)
{
    const size_t G = (size_t)out.G;
    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    AMOF_TRY(stages.setup());
    void *d_field;
    AMOF_TRY(ensure(ctx, SLOT_OUT1, G * sizeof(double), &d_field));
    StageSpans spans(ctx);
    timing_dom_begin(ctx, path);
    for (int64_t f = 0; f < out.F; f++) {
        AMOF_HIP_TRY(ctx, hipMemcpyAsync(d_field, in.field + (size_t)f * G, G * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        AMOF_TRY(stages.frame(f, (const double *)d_field, spans));
    }
    timing_dom_end(ctx, 0);
    timing_end(ctx);
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    stages.report();
    return AMOF_OK;
}

extern "C" int amof_pore_field(amof_ctx *ctx, const amof_traj *t, const double *radii, const int32_t *grid, double dr, double dmax,
                               const double *thresholds, int32_t n_t, uint64_t *hist, int64_t *counts, double *vmax, int64_t *argmax,
                               double *field)
{
    PoreOutputs out{hist, counts, vmax, argmax, field};
    return out.keep(pore_field_run(ctx, PoreInputs{t, radii, nullptr, nullptr, 0, grid, nullptr, dr, dmax, thresholds, n_t, 0, 0}, out, nullptr));
}
