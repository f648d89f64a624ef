// Bond order parameters (gfx950): amof_bond_order and amof_bond_order_dev.
//   order_rows_kernel  "order_frame": the unit vectors from the neighbour rows of the list stage (nbr.hip's lists_frame_kernel
//                      through frame_lists_tier, nbr_rows.h)
//   order_kernel       "order_exact": every tile of centres of a set against every partner, canonical float64 arithmetic
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "angle_math.h"
#include "nbr_rows.h"

namespace amof {

// --------------------------------------------------------------- bond order ----
// Steinhardt q_l and the tetrahedral order parameter q_tet of every centre of a set (A, B), from the unit vectors to its
// neighbours alone (include/amof_hip.h, amof_bond_order).  By the addition theorem of the spherical harmonics
//     q_l^2 = (n + 2 sum_{j<k} P_l(cos theta_jk)) / n^2,
// so a centre needs the cosines BAD forms and a Legendre recurrence, no spherical harmonic.  Every term is rounded to a
// fixed-point grid of 2^-40 (ORDER_E) and summed in int64: the sums are exact, order independent and the same on every
// path.  order_pair and order_centre are the ONE statement of the arithmetic both tiers call.
// Resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): order_rows_kernel 95 VGPRs, order_kernel<true / false> 84,
// 0 bytes of scratch per lane and no VGPR spill in either; the compiler parks 20 / 17 SGPRs in VGPR lanes, as it does for
// bad_rows_kernel.  No inline assembly.
constexpr int ORDER_E = 40;
constexpr int ORDER_MAX_L = 4;              // values of l per call
constexpr int ORDER_L_TOP = 12;             // each in 1 .. 12
constexpr int ORDER_CAP = 64;               // neighbours of a centre (more: AMOF_ECAPACITY); n 2^E + 2 T_l < 2^53 up to here
constexpr int ORDER_EXACT_LDS_BINS = 15360; // u32 bins beside the exact kernel's 96 KB of unit vectors

struct OrderArgs {
    int32_t n_l, l_top;             // l_top = the largest l asked for
    int32_t l[ORDER_MAX_L];         // (0: unused)
    int32_t nbins, nbins_tet;
    int32_t global_hist;            // 1: more bins than LDS holds -- u64 global atomics
    int32_t lane_sums;              // 1: per-lane atomics for the frame sums even where a wave shares one frame (measurements)
    int32_t cols;                   // 4 + n_l + 1 columns of frame_sums
    unsigned long long *hist;       // [n_sets][n_l][nbins]
    unsigned long long *hist_tet;   // [n_sets][nbins_tet]
    unsigned long long *frame_sums; // [F][n_sets][cols] (int64, two's complement)
    long long *per_atom;            // [F][n_sets][N][2 + n_l] or null
};

struct OrderSums {
    long long T[ORDER_MAX_L];       // sum over pairs of llrint(P_l(c) 2^E)
    long long U;                    // sum over pairs of llrint((c + 1/3)^2 2^E)
};

// one unordered pair of neighbours: BAD's clipped cosine (same expression, no contraction), the Bonnet recurrence in float64
__device__ __forceinline__ void order_pair(const OrderArgs &o, double ax, double ay, double az, double bx, double by, double bz,
                                           OrderSums &s)
{
    double c = ax * bx + ay * by + az * bz;
    if (c > 1.0) c = 1.0;
    if (c < -1.0) c = -1.0;
    double pm = 1.0, p = c;
    for (int m = 1;; m++) {
#pragma unroll
        for (int q = 0; q < ORDER_MAX_L; q++)
            if (o.l[q] == m) s.T[q] += llrint(p * 0x1p40);
        if (m >= o.l_top) break;
        const double pn = (((double)(2 * m + 1) * c) * p - (double)m * pm) / (double)(m + 1);
        pm = p;
        p = pn;
    }
    const double t = c + 1.0 / 3.0;
    s.U += llrint(t * t * 0x1p40);
}

// what a centre adds to its frame's sums: v[0..3] = n, n >= 1, n == 4, n (n - 1) / 2; ql[q] = llrint(q_l 2^30); qt = llrint(q_tet 2^30)
struct OrderRow {
    long long v[4];
    long long ql[ORDER_MAX_L];
    long long qt;
};

// a centre with n neighbours (0: none, or no centre at all) and its sums: the bins (lh: the workgroup's LDS histogram,
// [n_l][nbins] then [nbins_tet]; null: global atomics) and its row of the frame sums
__device__ __forceinline__ OrderRow order_centre(const OrderArgs &o, int set, int n, const OrderSums &s, unsigned *lh)
{
    OrderRow r;
    r.v[0] = n; r.v[1] = n >= 1 ? 1 : 0; r.v[2] = n == 4 ? 1 : 0; r.v[3] = (long long)n * (n - 1) / 2;
    r.qt = 0;
#pragma unroll
    for (int q = 0; q < ORDER_MAX_L; q++) {
        r.ql[q] = 0;
        if (n < 1 || q >= o.n_l) continue;
        long long Q = ((long long)n << ORDER_E) + 2 * s.T[q];
        if (Q < 0) Q = 0;
        const double ql = sqrt((double)Q * 0x1p-40) / (double)n;
        const int b = max(0, min((int)(ql * (double)o.nbins), o.nbins - 1));
        if (lh) atomicAdd(&lh[q * o.nbins + b], 1u);
        else atomicAdd(&o.hist[((size_t)set * o.n_l + q) * o.nbins + b], 1ull);
        r.ql[q] = llrint(ql * 0x1p30);
    }
    if (n == 4) {
        const double qt = 1.0 - 0.375 * ((double)s.U * 0x1p-40);
        const int b = max(0, min((int)((qt + 3.0) * 0.25 * (double)o.nbins_tet), o.nbins_tet - 1));
        if (lh) atomicAdd(&lh[o.n_l * o.nbins + b], 1u);
        else atomicAdd(&o.hist_tet[(size_t)set * o.nbins_tet + b], 1ull);
        r.qt = llrint(qt * 0x1p30);
    }
    return r;
}

// (n, T_l ..., U) of one centre
__device__ __forceinline__ void order_per_atom(const NbrArgs &a, const OrderArgs &o, int f, int set, int64_t atom, int n,
                                               const OrderSums &s)
{
    long long *pa = o.per_atom + (((size_t)f * a.n_sets + set) * (size_t)a.N + (size_t)atom) * (size_t)(2 + o.n_l);
    pa[0] = n;
#pragma unroll
    for (int q = 0; q < ORDER_MAX_L; q++)
        if (q < o.n_l) pa[1 + q] = s.T[q];
    pa[1 + o.n_l] = s.U;
}

// The rows of a wave's centres into frame_sums (called by all 64 lanes; f < 0: the lane has no centre).  A wave whose
// centres share one frame adds them up first -- one atomic per column; otherwise every lane adds its own row.
__device__ __forceinline__ void order_frame_sums(const OrderArgs &o, int n_sets, int f, int set, const OrderRow &r)
{
    const int f0 = __shfl(f, 0, 64);
    const bool shared = !o.lane_sums && __all(f == f0 || f < 0);
    const int lane = threadIdx.x & 63;
    auto column = [&](long long x, int col) {
        if (shared) {
            for (int off = 32; off > 0; off >>= 1) x += __shfl_down(x, off, 64);
            if (lane == 0 && f0 >= 0 && x) atomicAdd(&o.frame_sums[((size_t)f0 * n_sets + set) * o.cols + col], (unsigned long long)x);
        } else if (f >= 0 && x) {
            atomicAdd(&o.frame_sums[((size_t)f * n_sets + set) * o.cols + col], (unsigned long long)x);
        }
    };
#pragma unroll
    for (int k = 0; k < 4; k++) column(f >= 0 ? r.v[k] : 0, k);
#pragma unroll
    for (int q = 0; q < ORDER_MAX_L; q++)
        if (q < o.n_l) column(f >= 0 ? r.ql[q] : 0, 4 + q);
    column(f >= 0 ? r.qt : 0, 4 + o.n_l);
}

// the workgroup's LDS histogram into the global ones: one u64 atomic per non-empty bin
__device__ __forceinline__ void order_flush_hist(const OrderArgs &o, int set, const unsigned *lh, int threads)
{
    const int nq = o.n_l * o.nbins, nh = nq + o.nbins_tet;
    for (int k = threadIdx.x; k < nh; k += threads) {
        const unsigned v = lh[k];
        if (!v) continue;
        if (k < nq) atomicAdd(&o.hist[(size_t)set * nq + k], (unsigned long long)v);
        else atomicAdd(&o.hist_tet[(size_t)set * o.nbins_tet + (k - nq)], (unsigned long long)v);
    }
}

// per_atom before any kernel: (n, T_l ..., U) = (0, 0 ..., 0) for the atoms of a set's centre species (a set without a
// cutoff or without partners has no kernel work: its centres keep these), n = -1 for all others
__global__ __launch_bounds__(256) void order_init_kernel(long long *__restrict__ pa, const int32_t *__restrict__ species,
                                                         const int32_t *__restrict__ set_a, int n_sets, int64_t N, int width, size_t total)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < total; k += (size_t)gridDim.x * 256) {
        const size_t cell = k / (size_t)width;
        const int col = (int)(k - cell * (size_t)width);
        const int64_t atom = (int64_t)(cell % (size_t)N);
        const int set = (int)((cell / (size_t)N) % (size_t)n_sets);
        pa[k] = (col == 0 && species[atom] != set_a[set]) ? -1ll : 0ll;
    }
}

// Frame tier: work item (blockIdx.y) = (set, centre species, partner species, -); blockIdx.x strides over the tiles of 256
// (frame, centre) pairs of the batch, a lane owns its centre (as bad_rows_kernel); n <= 4 keeps the vectors in registers
__global__ __launch_bounds__(NBRF_TILE) void order_rows_kernel(NbrArgs a, NbrListArgs la, OrderArgs o, const int4 *__restrict__ aw,
                                                               const int64_t *__restrict__ sp_first, int f_base, int nf)
{
    extern __shared__ unsigned order_lh[];          // [n_l][nbins] | [nbins_tet] unless the counts go straight to global memory
    const int tid = threadIdx.x;
    const int4 w = aw[blockIdx.y];
    const int set = w.x, sa = w.y, sb = w.z;
    const int reg = la.region_of[sa * a.S + sb];
    const int64_t seg = sp_first[sa];
    const uint32_t nA = (uint32_t)(sp_first[sa + 1] - seg);
    const uint32_t total = (uint32_t)nf * nA;                             // (< 2^31: the host sizes the frame batch)
    const uint32_t tiles = (total + NBRF_TILE - 1) / NBRF_TILE;
    unsigned *lh = o.global_hist ? nullptr : order_lh;
    if (lh)
        for (int k = tid; k < o.n_l * o.nbins + o.nbins_tet; k += NBRF_TILE) lh[k] = 0u;
    __syncthreads();
    const size_t step = la.plane * (NBRL_EW / 2);
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t flat = tile * (uint32_t)NBRF_TILE + tid;
        const bool has = flat < total;
        const uint32_t fl = has ? flat / nA : 0u, r = has ? flat - fl * nA : 0u;
        const size_t cbase = (size_t)fl * la.R + r + (size_t)reg;
        int n = has ? (int)la.count[cbase] : 0;
        if (n > NBRL_CAP) { a.flags[1] = 1; n = 0; }        // (as bad_rows_kernel: a fuller centre -> the exact kernel)
        OrderSums s;
#pragma unroll
        for (int q = 0; q < ORDER_MAX_L; q++) s.T[q] = 0;
        s.U = 0;
        const double2 *__restrict__ e0 = reinterpret_cast<const double2 *>(la.rows + cbase * NBRL_EW);
        if (n >= 2 && n <= 4) {
            const double2 v0a = e0[0], v0b = e0[1], v1a = e0[step], v1b = e0[step + 1];
            order_pair(o, v0a.x, v0a.y, v0b.x, v1a.x, v1a.y, v1b.x, s);
            if (n > 2) {
                const double2 v2a = e0[2 * step], v2b = e0[2 * step + 1];
                order_pair(o, v0a.x, v0a.y, v0b.x, v2a.x, v2a.y, v2b.x, s);
                order_pair(o, v1a.x, v1a.y, v1b.x, v2a.x, v2a.y, v2b.x, s);
                if (n > 3) {
                    const double2 v3a = e0[3 * step], v3b = e0[3 * step + 1];
                    order_pair(o, v0a.x, v0a.y, v0b.x, v3a.x, v3a.y, v3b.x, s);
                    order_pair(o, v1a.x, v1a.y, v1b.x, v3a.x, v3a.y, v3b.x, s);
                    order_pair(o, v2a.x, v2a.y, v2b.x, v3a.x, v3a.y, v3b.x, s);
                }
            }
        } else if (n > 4) {
            for (int u = 0; u + 1 < n; u++) {
                const double2 a01 = e0[u * step], a2 = e0[u * step + 1];
                for (int v = u + 1; v < n; v++) {
                    const double2 b01 = e0[v * step], b2 = e0[v * step + 1];
                    order_pair(o, a01.x, a01.y, a2.x, b01.x, b01.y, b2.x, s);
                }
            }
        }
        const int f = has ? f_base + (int)fl : -1;
        const OrderRow row = order_centre(o, set, n, s, lh);
        if (o.per_atom && has) order_per_atom(a, o, f, set, a.perm[seg + r], n, s);
        order_frame_sums(o, a.n_sets, f, set, row);
    }
    __syncthreads();
    if (lh) order_flush_hist(o, set, lh, NBRF_TILE);
}

// Exact tier: bad_kernel<ORTHO, false>'s structure -- a lane per centre of a tile of 64, partner tiles staged through LDS,
// the canonical minimum image (pair_base) and the strict sqrt(d2) < rc of amof_cn_count, the unit vectors [slot][lane] in
// LDS, ORDER_CAP slots (96 KB).  Any cell, open axes, atoms anywhere.
template <bool ORTHO>
__global__ __launch_bounds__(BAD_TILE) void order_kernel(NbrArgs a, OrderArgs o)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double *ux = reinterpret_cast<double *>(lds_raw);
    double *uy = ux + ORDER_CAP * BAD_TILE;
    double *uz = uy + ORDER_CAP * BAD_TILE;
    double *tjx = uz + ORDER_CAP * BAD_TILE;
    double *tjy = tjx + BAD_TILE;
    double *tjz = tjy + BAD_TILE;
    int *tja = reinterpret_cast<int *>(tjz + BAD_TILE);
    unsigned *lh = o.global_hist ? nullptr : reinterpret_cast<unsigned *>(tja + BAD_TILE);

    const int tid = threadIdx.x;
    const int4 w = a.work[blockIdx.x];          // (set, centre tile, A, B)
    const int set = w.x, A = w.z, B = w.w;
    const Tile ti = a.tiles[w.y];
    const double rc = a.cutoff[A * a.S + B];
    const int64_t ai = tid < ti.count ? a.perm[ti.start + tid] : -1;
    const int f0 = blockIdx.y * a.frames_per_chunk;
    const int f1 = min(f0 + a.frames_per_chunk, a.F);
    const int tb0 = a.sp_first_tile[B], tb1 = tb0 + a.sp_ntiles[B];
    if (lh)
        for (int k = tid; k < o.n_l * o.nbins + o.nbins_tet; k += BAD_TILE) lh[k] = 0u;
    __syncthreads();

    for (int f = f0; f < f1; f++) {
        const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
        const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
        double xi = 0.0, yi = 0.0, zi = 0.0;
        if (ai >= 0) {
            xi = p[ai * 3 + 0];
            yi = p[ai * 3 + 1];
            zi = p[ai * 3 + 2];
        }
        int n = 0;
        if (rc > 0.0) {
            for (int tb = tb0; tb < tb1; tb++) {
                // partner tiles hold up to 256 atoms: stage them 64 at a time
                const Tile tj = a.tiles[tb];
                for (int base = 0; base < tj.count; base += BAD_TILE) {
                    const int cntj = min(BAD_TILE, tj.count - base);
                    __syncthreads();
                    if (tid < cntj) {
                        const int64_t aj = a.perm[tj.start + base + tid];
                        tjx[tid] = p[aj * 3 + 0];
                        tjy[tid] = p[aj * 3 + 1];
                        tjz[tid] = p[aj * 3 + 2];
                        tja[tid] = (int)aj;
                    }
                    __syncthreads();
                    if (ai < 0) continue;
                    for (int j = 0; j < cntj; j++) {
                        if (tja[j] == (int)ai) continue;
                        double dx, dy, dz;
                        pair_base<ORTHO>(g, tjx[j] - xi, tjy[j] - yi, tjz[j] - zi, dx, dy, dz);
                        if (!(sqrt(norm2(dx, dy, dz)) < rc)) continue;
                        double qx = 0.0, qy = 0.0, qz = 0.0;
                        if (!unit_vec(dx, dy, dz, qx, qy, qz)) a.flags[0] = 1;       // (the call fails: results are discarded)
                        if (n < ORDER_CAP) {
                            ux[n * BAD_TILE + tid] = qx;
                            uy[n * BAD_TILE + tid] = qy;
                            uz[n * BAD_TILE + tid] = qz;
                        } else {
                            a.flags[1] = 1;                                          // (AMOF_ECAPACITY)
                        }
                        n++;
                    }
                }
            }
        }
        const int nn = min(n, ORDER_CAP);
        OrderSums s;
#pragma unroll
        for (int q = 0; q < ORDER_MAX_L; q++) s.T[q] = 0;
        s.U = 0;
        for (int u = 0; u + 1 < nn; u++) {
            const double ax = ux[u * BAD_TILE + tid], ay = uy[u * BAD_TILE + tid], az = uz[u * BAD_TILE + tid];
            for (int v = u + 1; v < nn; v++)
                order_pair(o, ax, ay, az, ux[v * BAD_TILE + tid], uy[v * BAD_TILE + tid], uz[v * BAD_TILE + tid], s);
        }
        const OrderRow row = order_centre(o, set, ai >= 0 ? nn : 0, s, lh);
        if (o.per_atom && ai >= 0) order_per_atom(a, o, f, set, ai, nn, s);
        order_frame_sums(o, a.n_sets, ai >= 0 ? f : -1, set, row);
    }
    __syncthreads();
    if (lh) order_flush_hist(o, set, lh, BAD_TILE);
}

// ------------------------------------------------------------ bond order: host side ----
// the extents of a call's arrays, once for the check-to-fetch path and for the zeros the entry points leave
struct OrderShape {
    size_t words;               // histogram words of a set: n_l nbins + nbins_tet
    size_t hq, ht;              // hist [n_sets][n_l][nbins], hist_tet [n_sets][nbins_tet]
    size_t fs_words, pa_words;  // frame_sums [F][n_sets][4 + n_l + 1], per_atom [F][n_sets][N][2 + n_l]
    OrderShape(const amof_traj *t, int32_t n_sets, int32_t n_l, int32_t nbins, int32_t nbins_tet)
        : words((size_t)n_l * nbins + (size_t)nbins_tet), hq((size_t)n_sets * n_l * nbins), ht((size_t)n_sets * nbins_tet),
          fs_words((size_t)t->n_frames * n_sets * (4 + n_l + 1)), pa_words((size_t)t->n_frames * n_sets * (size_t)t->n_atoms * (size_t)(2 + n_l))
    {
    }
    void zero_host(int64_t *frame_sums, int64_t *per_atom) const
    {
        std::fill(frame_sums, frame_sums + fs_words, (int64_t)0);
        if (per_atom) std::fill(per_atom, per_atom + pa_words, (int64_t)0);
    }
};

struct OrderCall : HistCall {
    const int32_t *sets;
    int32_t n_sets;
    OrderArgs o;
    size_t words = 0;           // OrderShape::words
    void *d_pa = nullptr;
    size_t pa_words = 0;
    const int32_t *d_species = nullptr, *d_set_a = nullptr;
    int reset_outputs()         // the outputs as before the first tier: per_atom as order_init_kernel leaves it
    {
        AMOF_TRY(HistCall::reset_outputs());
        if (d_pa) {
            const unsigned blocks = (unsigned)std::min<size_t>((pa_words + 255) / 256, 8192);
            hipLaunchKernelGGL(order_init_kernel, dim3(blocks), dim3(256), 0, ctx->stream, (long long *)d_pa, d_species, d_set_a,
                               (int)n_sets, (int64_t)t->n_atoms, 2 + o.n_l, pa_words);
            AMOF_HIP_TRY(ctx, hipGetLastError());
        }
        return AMOF_OK;
    }
};

// whole-frame-in-LDS tier: BAD's list stage (one sort + LDS search per species pair into neighbour rows), every set from its rows
static int order_frame_tier(OrderCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    NbrSetup &st = c.st;
    const int S = t->n_species;
    std::vector<char> needed((size_t)S * S, 0);
    std::vector<int4> awork;
    for (int s2 = 0; s2 < c.n_sets; s2++) {
        const int A = c.sets[2 * s2], B = c.sets[2 * s2 + 1];
        if (!(c.cutoff[A * S + B] > 0.0) || st.tiles.nsp[A] == 0 || st.tiles.nsp[B] == 0) continue;     // (no centre has a neighbour)
        needed[(size_t)A * S + B] = 1;
        awork.push_back(make_int4(s2, A, B, 0));
    }
    c.o.global_hist = c.words > (size_t)AMOF_MAX_LDS_BINS ? 1 : 0;
    const size_t lds = c.o.global_hist ? 0 : c.words * sizeof(unsigned);
    auto order = [&](const RowsBatch &b) -> int {
        const int64_t nfr = b.nfr;
        // about eight workgroups per CU in all work items together, each striding over the tiles of its own (as bad_rows_kernel)
        int64_t widest = 0;
        for (const int4 &w : awork) widest = std::max<int64_t>(widest, (nfr * st.tiles.nsp[(size_t)w.y] + NBRF_TILE - 1) / NBRF_TILE);
        const int64_t gx = std::max<int64_t>(1, std::min<int64_t>(widest, (2048 + (int64_t)awork.size() - 1) / (int64_t)awork.size()));
        const dim3 grid((unsigned)gx, (unsigned)awork.size());
        AMOF_HIP_TRY(ctx, launch_lds(order_rows_kernel, grid, dim3(NBRF_TILE), lds, ctx->stream, st.a, b.la, c.o, (const int4 *)b.head, b.sp_first,
                                     b.f_base, (int)nfr));
        return AMOF_OK;
    };
    const ListsRequest rq{needed, reinterpret_cast<const int32_t *>(awork.data()), 4 * awork.size(), "AMOF_ORDER_ROWS_MB", true, FRAME_ORDER};
    ListsOutcome outcome;
    int32_t qflag;
    AMOF_TRY(frame_lists_tier(c, rq, order, outcome, qflag));
    return frame_lists_finish(c, outcome, qflag);     // (after a reset the exact kernel answers)
}

// exact kernel: every tile of centres of a set against every partner, canonical float64 arithmetic
static int order_exact_tier(OrderCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    NbrSetup &st = c.st;
    NbrArgs &a = st.a;
    std::vector<int4> work;
    for (int s = 0; s < c.n_sets; s++) {
        const int A = c.sets[2 * s], B = c.sets[2 * s + 1];
        for (int k = 0; k < st.tiles.sp_ntiles[A]; k++) work.push_back(make_int4(s, st.tiles.sp_first_tile[A] + k, A, B));
    }
    if (work.empty() || t->n_frames <= 0) return AMOF_OK;
    void *d_work;
    AMOF_TRY(upload(ctx, SLOT_PAIRS, work.data(), work.size() * sizeof(int4), &d_work));
    a.work = (const int4 *)d_work;
    c.o.global_hist = c.words > (size_t)ORDER_EXACT_LDS_BINS ? 1 : 0;
    const size_t lds = (size_t)(3 * ORDER_CAP * BAD_TILE + 3 * BAD_TILE) * sizeof(double) + BAD_TILE * sizeof(int) +
                       (c.o.global_hist ? 0 : c.words * sizeof(unsigned));
    unsigned chunks;
    pick_chunks(t->n_frames, work.size(), a.frames_per_chunk, chunks);
    timing_dom_begin(ctx, "order_exact");
    if (c.spans) c.spans->begin(1);
    const hipError_t e = with_flag(st.geom.all_ortho, [&](auto O) {
        return launch_lds(order_kernel<O()>, dim3((unsigned)work.size(), chunks), dim3(BAD_TILE), lds, ctx->stream, a, c.o);
    });
    AMOF_HIP_TRY(ctx, e);
    if (c.spans) c.spans->end();
    timing_dom_end(ctx, 1);
    int32_t flags[4];
    AMOF_TRY(c.read_flags(flags));
    if (flags[0]) return fail(ctx, AMOF_EANGLE, "Undefined angle");
    if (flags[1]) return fail(ctx, AMOF_ECAPACITY, "a centre has more than %d neighbours", ORDER_CAP);
    c.done = true;
    return AMOF_OK;
}

static int order_check(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets, const int32_t *l,
                       int32_t n_l, int32_t nbins, int32_t nbins_tet, const void *hist, const void *hist_tet, const void *frame_sums)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    if (!cutoff || n_sets < 0 || (n_sets > 0 && !sets) || !l) return fail(ctx, AMOF_EINVAL, "NULL argument");
    AMOF_TRY(pore_refuse(ctx, nbr_check::order_l_count(n_l, ORDER_MAX_L)));
    AMOF_TRY(pore_refuse(ctx, nbr_check::order_l(l, n_l, ORDER_L_TOP)));
    AMOF_TRY(pore_refuse(ctx, nbr_check::order_bins(nbins, nbins_tet)));
    if (n_sets > 0 && (!hist || !hist_tet || (t->n_frames > 0 && !frame_sums))) return fail(ctx, AMOF_EINVAL, "NULL argument");
    const int S = t->n_species;
    AMOF_TRY(pore_refuse(ctx, nbr_check::sets_in_range(sets, n_sets, S)));
    AMOF_TRY(pore_refuse(ctx, nbr_check::values_not_negative(cutoff, S * S, "cutoff")));
    if (n_sets == 0 || t->n_frames == 0) return AMOF_OK;
    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    const double hmin = nbr_check::min_periodic_height(t->pbc, geom.rec.data(), t->n_cells);
    for (int s = 0; s < n_sets; s++)
        AMOF_TRY(pore_refuse(ctx, nbr_check::half_height_set(cutoff[sets[2 * s] * S + sets[2 * s + 1]], s, hmin, "a neighbour could be counted twice")));
    return AMOF_OK;
}

// hist_dev / hist_tet_dev: device buffers to add into, or null (the call's own device buffers are then read back into
// hist_host / hist_tet_host); frame_sums and per_atom: host
static int order_run(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets, const int32_t *l,
                     int32_t n_l, int32_t nbins, int32_t nbins_tet, const OrderShape &sh, uint64_t *hist_dev, uint64_t *hist_tet_dev,
                     uint64_t *hist_host, uint64_t *hist_tet_host, int64_t *frame_sums, int64_t *per_atom)
{
    if (n_sets == 0 || t->n_frames == 0) return AMOF_OK;
    OrderCall c{{{ctx, t, cutoff}}, sets, n_sets};
    AMOF_TRY(nbr_setup(ctx, t, cutoff, BAD_TILE, c.st));
    StageSpans spans(ctx);      // list stage, order kernels
    c.spans = &spans;
    OrderArgs &o = c.o;
    memset(&o, 0, sizeof o);
    o.n_l = n_l;
    for (int q = 0; q < n_l; q++) {
        o.l[q] = l[q];
        o.l_top = std::max(o.l_top, l[q]);
    }
    o.nbins = nbins;
    o.nbins_tet = nbins_tet;
    o.cols = 4 + n_l + 1;
    const char *sv = getenv("AMOF_ORDER_SUMS");
    o.lane_sums = sv && !strcmp(sv, "lane") ? 1 : 0;
    c.words = sh.words;
    const size_t hq = sh.hq, ht = sh.ht;
    c.hs_words = hq + ht;
    c.fs_bytes = sh.fs_words * sizeof(int64_t);
    AMOF_TRY(c.alloc_outputs());
    if (per_atom) {
        c.pa_words = sh.pa_words;
        AMOF_TRY(ensure(ctx, SLOT_OUT1, c.pa_words * sizeof(int64_t), &c.d_pa));
        std::vector<int32_t> set_a((size_t)n_sets);
        for (int s = 0; s < n_sets; s++) set_a[(size_t)s] = sets[2 * s];
        UploadPack pk;
        const int i_sp = pk.add(t->species, (size_t)t->n_atoms * sizeof(int32_t));
        const int i_sa = pk.add(set_a.data(), set_a.size() * sizeof(int32_t));
        AMOF_TRY(upload_pack(ctx, SLOT_AUX3, pk));
        AMOF_HIP_TRY(ctx, sync_stream(ctx));        // (set_a leaves scope)
        c.d_species = pk.ptr<int32_t>(i_sp);
        c.d_set_a = pk.ptr<int32_t>(i_sa);
    }
    o.hist = (unsigned long long *)c.d_hs;
    o.hist_tet = o.hist + hq;
    o.frame_sums = (unsigned long long *)c.d_fs;
    o.per_atom = (long long *)c.d_pa;
    c.st.a.n_sets = n_sets;
    AMOF_TRY(c.reset_outputs());
    const char *ex = getenv("AMOF_ORDER_EXACT");
    if (!(ex && ex[0] == '1')) AMOF_TRY(order_frame_tier(c));
    AMOF_TRY(stager_need(c.st.stage, t->n_frames));   // (no-op unless the frame tier was skipped)
    if (!c.done) AMOF_TRY(order_exact_tier(c));
    // complete and valid: to the caller
    if (hist_dev) {
        AMOF_TRY(add_into(ctx, hist_dev, (const uint64_t *)o.hist, hq));
        AMOF_TRY(add_into(ctx, hist_tet_dev, (const uint64_t *)o.hist_tet, ht));
    }
    timing_end(ctx);
    if (!hist_dev) {
        AMOF_TRY(fetch(ctx, hist_host, o.hist, hq * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, hist_tet_host, o.hist_tet, ht * sizeof(uint64_t)));
    }
    AMOF_TRY(fetch(ctx, frame_sums, c.d_fs, c.fs_bytes));
    if (per_atom) AMOF_TRY(fetch(ctx, per_atom, c.d_pa, c.pa_words * sizeof(int64_t)));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

extern "C" int amof_bond_order(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets,
                               const int32_t *l, int32_t n_l, int32_t nbins, int32_t nbins_tet, uint64_t *hist, uint64_t *hist_tet,
                               int64_t *frame_sums, int64_t *per_atom)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(order_check(ctx, t, cutoff, sets, n_sets, l, n_l, nbins, nbins_tet, hist, hist_tet, frame_sums));
    // the host form overwrites: zeros first, so that a failing call leaves zeros (no set or no frame: nothing to zero)
    const OrderShape sh(t, n_sets, n_l, nbins, nbins_tet);
    std::fill(hist, hist + sh.hq, (uint64_t)0);
    std::fill(hist_tet, hist_tet + sh.ht, (uint64_t)0);
    sh.zero_host(frame_sums, per_atom);
    return order_run(ctx, t, cutoff, sets, n_sets, l, n_l, nbins, nbins_tet, sh, nullptr, nullptr, hist, hist_tet, frame_sums, per_atom);
}

extern "C" int amof_bond_order_dev(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                   const int32_t *l, int32_t n_l, int32_t nbins, int32_t nbins_tet, uint64_t *hist_dev,
                                   uint64_t *hist_tet_dev, int64_t *frame_sums, int64_t *per_atom)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(order_check(ctx, t, cutoff, sets, n_sets, l, n_l, nbins, nbins_tet, hist_dev, hist_tet_dev, frame_sums));
    const OrderShape sh(t, n_sets, n_l, nbins, nbins_tet);
    sh.zero_host(frame_sums, per_atom);
    return order_run(ctx, t, cutoff, sets, n_sets, l, n_l, nbins, nbins_tet, sh, hist_dev, hist_tet_dev, nullptr, nullptr, frame_sums, per_atom);
}
