// Covering radius of the pore field (gfx950): w(p) = the largest v(c) over the grid points c whose sphere of radius v(c) >= 0
// reaches p, d2(c - p) <= v(c)^2 (include/amof_hip.h amof_pore_psd has the definitions), v(p) where none does.  From it the
// Gelb-Gubbins pore size distribution (the histogram of w) and the probe-occupiable volume #{w >= rp}; with the labels and
// the marked channel roots of pore_access.hip the part of it that is covered from a channel.  A gather: every point takes the
// maximum over the centres that cover it, no atomics on w, the maximum of IEEE numbers does not depend on the order.
//
//   pc_brickmax_kernel  the largest v over the admissible centres of every brick of 8 x 8 x 8 grid points
//   pc_exact_kernel     ("pore_cover_exact") a lane per grid point walks the frame's offset stencil, every offset with
//                       d2 <= vmax^2, from a table the host builds per frame
//   pc_brick_kernel     ("pore_cover_brick") a workgroup owns a destination brick.  It walks the source bricks of the index
//                       box within reach of vmax -- every periodic image on its own, an image shift per axis --, keeps those
//                       whose maximum reaches the destination brick's bounding sphere (a workgroup-uniform list in LDS), and
//                       of those the centres whose own sphere does, as records (index triple relative to the brick, v) in
//                       LDS.  Every lane sweeps the records for its two points; the deciding compare d2 <= v v is the
//                       canonical float64 one, formed from the integer index difference -- the same bits as the stencil's.
//                       The record list is swept and emptied whenever the next source brick might not fit: it cannot overflow.
//   pc_count_kernel     histogram of w and the counts w >= thresholds[t]
// ACCESS variants: the centres are restricted to the points whose periodic root is a marked channel root, a point only needs
// to know whether any centre covers it, the covered points are counted.
// No kernel waits for another workgroup.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"

namespace amof {

constexpr int PC_THREADS = 256;
constexpr int PC_BRICK = 8;
constexpr int PC_POINTS = PC_BRICK * PC_BRICK * PC_BRICK;
constexpr int PC_PPL = PC_POINTS / PC_THREADS;          // grid points per lane
constexpr int PC_SRC_CAP = 2048;                        // source bricks a destination brick keeps (more: the frame goes to pc_exact_kernel)
constexpr int PC_REC_CAP = 2048;                        // centre records in LDS
constexpr int PC_REC_FLUSH = PC_REC_CAP - PC_POINTS;    // swept as soon as one more brick might not fit
constexpr int64_t PC_BOX_MAX = 32768;                   // source bricks of the reach box a workgroup is made to test
constexpr int64_t PC_STENCIL_MAX = (int64_t)1 << 24;    // offsets of the exact path's table (AMOF_ECAPACITY beyond)
constexpr int PC_COUNT_ROUNDS = 16;
static_assert(PC_PPL == 2, "a lane's points are l = tid and tid + 256");

struct PcFrame {
    double A[9];            // step vectors: A[3 k + c] = C[k][c] / (double)n_k
    double hd;              // half diagonal of a brick's index box (3.5 steps per axis), rounded up
    int32_t n[3], pbc[3], nb[3], R[3];      // grid, periodic flags, bricks per axis, largest |offset| per axis
    int32_t src_cap;        // source bricks a destination brick may keep: PC_SRC_CAP, or fewer (AMOF_PORE_COVER_SRC_CAP)
    int64_t G;
};

struct PcOffset {
    short d[3], pad;
    double d2;
};

// the canonical distance of an index offset: float64 in this order, no fma (the library is built with -ffp-contract=off)
__host__ __device__ inline double pc_d2(const double *A, double a, double b, double c)
{
    const double sx = (a * A[0] + b * A[3]) + c * A[6];
    const double sy = (a * A[1] + b * A[4]) + c * A[7];
    const double sz = (a * A[2] + b * A[5]) + c * A[8];
    return (sx * sx + sy * sy) + sz * sz;
}

__device__ __forceinline__ bool pc_admissible(double v, const int32_t *__restrict__ parent, const int32_t *__restrict__ mark, int64_t c,
                                              bool access)
{
    if (!(v >= 0.0)) return false;
    if (!access) return true;
    const int r = parent[c];
    return r >= 0 && mark[r] < 0;
}

template <bool ACCESS>
__global__ __launch_bounds__(PC_THREADS) void pc_brickmax_kernel(const double *__restrict__ field, const int32_t *__restrict__ parent,
                                                                 const int32_t *__restrict__ mark, PcFrame g, double *__restrict__ bmax)
{
    __shared__ double sv[PC_THREADS / 64];
    const int tid = threadIdx.x, wg = blockIdx.x;
    const int b2 = wg % g.nb[2], b1 = (wg / g.nb[2]) % g.nb[1], b0 = wg / (g.nb[2] * g.nb[1]);
    double m = -INFINITY;
#pragma unroll
    for (int q = 0; q < PC_PPL; q++) {
        const int l = tid + q * PC_THREADS;
        const int i = b0 * PC_BRICK + (l >> 6), j = b1 * PC_BRICK + ((l >> 3) & 7), k = b2 * PC_BRICK + (l & 7);
        if (i < g.n[0] && j < g.n[1] && k < g.n[2]) {
            const int64_t c = ((int64_t)i * g.n[1] + j) * g.n[2] + k;
            const double v = field[c];
            if (!ACCESS || pc_admissible(v, parent, mark, c, true)) m = fmax(m, v);
        }
    }
    for (int off = 32; off > 0; off >>= 1) m = fmax(m, __shfl_down(m, off, 64));
    if ((tid & 63) == 0) sv[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < PC_THREADS / 64; w++) m = fmax(m, sv[w]);
        bmax[wg] = m;
    }
}

// covered points of a wave into one counter
__device__ __forceinline__ void pc_add_covered(unsigned long long *covered, bool cov)
{
    const unsigned long long b = __ballot(cov);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd(covered, (unsigned long long)__popcll(b));
}

// ---------------------------------------------------------------- exact ----
template <bool ACCESS>
__global__ __launch_bounds__(PC_THREADS) void pc_exact_kernel(const double *__restrict__ field, const int32_t *__restrict__ parent,
                                                              const int32_t *__restrict__ mark, PcFrame g, const PcOffset *__restrict__ st,
                                                              int n_st, double *__restrict__ w, unsigned long long *__restrict__ covered)
{
    __shared__ PcOffset tile[PC_THREADS];
    const int tid = threadIdx.x;
    const int64_t lin = (int64_t)blockIdx.x * PC_THREADS + tid;
    const bool valid = lin < g.G;
    int i = 0, j = 0, k = 0;
    double vp = -1.0;
    if (valid) {
        k = (int)(lin % g.n[2]);
        const int64_t ij = lin / g.n[2];
        i = (int)(ij / g.n[1]);
        j = (int)(ij % g.n[1]);
        vp = field[lin];
    }
    // (best < 0: no centre covers the point.)  A point that is an admissible centre covers itself through offset 0.
    bool cov = valid && pc_admissible(vp, parent, mark, lin, ACCESS);
    double best = cov ? vp : -1.0;
    for (int s0 = 0; s0 < n_st; s0 += PC_THREADS) {
        const int cnt = min(PC_THREADS, n_st - s0);
        __syncthreads();
        if (tid < cnt) tile[tid] = st[s0 + tid];
        __syncthreads();
        if (!valid) continue;
        for (int e = 0; e < cnt; e++) {
            const PcOffset o = tile[e];
            int ti = i + o.d[0], tj = j + o.d[1], tk = k + o.d[2];
            // (|offset| <= n_k on a periodic axis, the host sees to that: one image shift at most)
            if (ti < 0 || ti >= g.n[0]) {
                if (!g.pbc[0]) continue;
                ti += ti < 0 ? g.n[0] : -g.n[0];
            }
            if (tj < 0 || tj >= g.n[1]) {
                if (!g.pbc[1]) continue;
                tj += tj < 0 ? g.n[1] : -g.n[1];
            }
            if (tk < 0 || tk >= g.n[2]) {
                if (!g.pbc[2]) continue;
                tk += tk < 0 ? g.n[2] : -g.n[2];
            }
            const int64_t c = ((int64_t)ti * g.n[1] + tj) * g.n[2] + tk;
            const double vc = field[c];
            if (ACCESS) {
                if (!cov && vc >= 0.0 && o.d2 <= vc * vc && pc_admissible(vc, parent, mark, c, true)) cov = true;
            } else if (vc >= 0.0 && vc > best && o.d2 <= vc * vc)
                best = vc;
        }
    }
    if (ACCESS) pc_add_covered(covered, cov);
    else if (valid) w[lin] = best >= 0.0 ? best : vp;
}

// ---------------------------------------------------------------- brick ----
__device__ __forceinline__ int pc_floor_div(int x, int n)
{
    const int q = x / n;
    return (x % n != 0 && x < 0) ? q - 1 : q;
}

// the segment of unwrapped index u: image m = floor(u / n), brick of the wrapped index; segments tile [-n, 2 n) in this order
__device__ __forceinline__ int pc_segment(int u, int n, int nb)
{
    const int m = pc_floor_div(u, n);
    return (m + 1) * nb + (u - m * n) / PC_BRICK;
}

struct PcSource {
    int sb[3];      // brick
    int u0[3];      // unwrapped index of its first point, relative to the destination brick's first point
};

__device__ __forceinline__ PcSource pc_source(const PcFrame &g, const int *alo, const int *cnt, const int *i0, int e)
{
    const int a[3] = {alo[0] + e / (cnt[1] * cnt[2]), alo[1] + (e / cnt[2]) % cnt[1], alo[2] + e % cnt[2]};
    PcSource s;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int m = a[k] / g.nb[k] - 1;
        s.sb[k] = a[k] % g.nb[k];
        s.u0[k] = s.sb[k] * PC_BRICK + m * g.n[k] - i0[k];
    }
    return s;
}

// flags[0]: more source bricks survive than the list holds; stats[0] += surviving source bricks, stats[1] += records
template <bool ACCESS>
__global__ __launch_bounds__(PC_THREADS) void pc_brick_kernel(const double *__restrict__ field, const int32_t *__restrict__ parent,
                                                              const int32_t *__restrict__ mark, PcFrame g, const double *__restrict__ bmax,
                                                              double *__restrict__ w, unsigned long long *__restrict__ covered,
                                                              unsigned long long *__restrict__ flags, unsigned long long *__restrict__ stats)
{
    __shared__ int src[PC_SRC_CAP];
    __shared__ double rv[PC_REC_CAP];
    __shared__ short4 rx[PC_REC_CAP];
    __shared__ unsigned n_src, n_rec;
    const int tid = threadIdx.x, wg = blockIdx.x;
    const int i0[3] = {(wg / (g.nb[2] * g.nb[1])) * PC_BRICK, ((wg / g.nb[2]) % g.nb[1]) * PC_BRICK, (wg % g.nb[2]) * PC_BRICK};
    if (tid == 0) {
        n_src = 0u;
        n_rec = 0u;
    }

    // ---- this lane's points
    const int li[PC_PPL] = {tid >> 6, (tid + PC_THREADS) >> 6}, lj = (tid >> 3) & 7, lk = tid & 7;
    bool valid[PC_PPL], cov[PC_PPL];
    int64_t lin[PC_PPL];
    double vp[PC_PPL], best[PC_PPL];
#pragma unroll
    for (int q = 0; q < PC_PPL; q++) {
        const int i = i0[0] + li[q], j = i0[1] + lj, k = i0[2] + lk;
        valid[q] = i < g.n[0] && j < g.n[1] && k < g.n[2];
        lin[q] = valid[q] ? ((int64_t)i * g.n[1] + j) * g.n[2] + k : 0;
        vp[q] = valid[q] ? field[lin[q]] : -1.0;
        // a point that is an admissible centre covers itself (offset 0): the sweep starts from that and only larger centres matter
        cov[q] = valid[q] && pc_admissible(vp[q], parent, mark, lin[q], ACCESS);
        best[q] = cov[q] ? vp[q] : -1.0;
    }

    // ---- the index box within reach, as a range of segments per axis
    int alo[3], cnt[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        int lo = i0[k] - g.R[k], hi = min(i0[k] + PC_BRICK - 1, g.n[k] - 1) + g.R[k];
        if (g.pbc[k]) {
            lo = max(lo, -g.n[k]);
            hi = min(hi, 2 * g.n[k] - 1);
        } else {
            lo = max(lo, 0);
            hi = min(hi, g.n[k] - 1);
        }
        alo[k] = pc_segment(lo, g.n[k], g.nb[k]);
        cnt[k] = pc_segment(hi, g.n[k], g.nb[k]) - alo[k] + 1;
    }
    const int total = cnt[0] * cnt[1] * cnt[2];         // (<= PC_BOX_MAX: pc_frame)
    __syncthreads();

    // ---- the source bricks whose largest centre reaches the bounding sphere of this brick: both bricks lie within hd of the
    // centres of their index boxes, which are an integer offset apart
    for (int e = tid; e < total; e += PC_THREADS) {
        const PcSource s = pc_source(g, alo, cnt, i0, e);
        const double M = bmax[((int64_t)s.sb[0] * g.nb[1] + s.sb[1]) * g.nb[2] + s.sb[2]];
        if (!(M >= 0.0)) continue;
        const double dist = sqrt(pc_d2(g.A, (double)s.u0[0], (double)s.u0[1], (double)s.u0[2]));
        if (M + 2.0 * g.hd >= dist) {
            const unsigned slot = atomicAdd(&n_src, 1u);
            if (slot < (unsigned)g.src_cap) src[slot] = e;
        }
    }
    __syncthreads();
    int ns = (int)n_src;
    if (ns > g.src_cap) {
        if (tid == 0) flags[0] = 1ull;          // (the host discards the frame's results and runs pc_exact_kernel)
        ns = g.src_cap;
    }

    auto sweep = [&](int n) {
        for (int r = 0; r < n; r++) {
            const double v = rv[r];
            const short4 x = rx[r];
            const double v2 = v * v;
#pragma unroll
            for (int q = 0; q < PC_PPL; q++) {
                if (!valid[q] || (ACCESS ? cov[q] : !(v > best[q]))) continue;
                const double d2 = pc_d2(g.A, (double)(x.x - li[q]), (double)(x.y - lj), (double)(x.z - lk));
                if (d2 <= v2) {
                    best[q] = v;
                    cov[q] = true;
                }
            }
        }
    };

    unsigned long long records = 0ull;
    for (int s = 0; s < ns; s++) {
        const PcSource sc = pc_source(g, alo, cnt, i0, src[s]);
        // ---- the centres of this source brick whose own sphere reaches the bounding sphere
#pragma unroll
        for (int q = 0; q < PC_PPL; q++) {
            const int ci = sc.sb[0] * PC_BRICK + li[q], cj = sc.sb[1] * PC_BRICK + lj, ck = sc.sb[2] * PC_BRICK + lk;
            if (ci >= g.n[0] || cj >= g.n[1] || ck >= g.n[2]) continue;
            const int64_t c = ((int64_t)ci * g.n[1] + cj) * g.n[2] + ck;
            const double v = field[c];
            if (!pc_admissible(v, parent, mark, c, ACCESS)) continue;
            const int u[3] = {sc.u0[0] + li[q], sc.u0[1] + lj, sc.u0[2] + lk};
            const double dist = sqrt(pc_d2(g.A, (double)u[0] - 3.5, (double)u[1] - 3.5, (double)u[2] - 3.5));
            if (v + g.hd >= dist) {
                const unsigned slot = atomicAdd(&n_rec, 1u);        // (< PC_REC_CAP: at most PC_REC_FLUSH before this brick)
                rv[slot] = v;
                rx[slot] = make_short4((short)u[0], (short)u[1], (short)u[2], 0);
            }
        }
        // Invariant: n_rec is read only between two barriers with no write to it in between -- the appends of this brick lie
        // before the first, the reset and the appends of the next brick behind the second -- so every lane reads the same
        // count and the decision to sweep is workgroup-uniform.
        __syncthreads();
        const int nr = (int)n_rec;
        const bool flush = nr > PC_REC_FLUSH || s == ns - 1;
        if (flush) {
            sweep(nr);
            records += (unsigned long long)nr;
        }
        __syncthreads();
        if (flush) {
            if (tid == 0) n_rec = 0u;
            __syncthreads();
        }
    }

    if (ACCESS) {
#pragma unroll
        for (int q = 0; q < PC_PPL; q++) pc_add_covered(covered, cov[q]);
    } else {
#pragma unroll
        for (int q = 0; q < PC_PPL; q++)
            if (valid[q]) w[lin[q]] = best[q] >= 0.0 ? best[q] : vp[q];
    }
    if (tid == 0) {
        atomicAdd(&stats[0], (unsigned long long)ns);
        atomicAdd(&stats[1], records);
    }
}

// out [nbins + 2 + n_t]: [0] w < 0, [1 + b] b = (int)(w / dr) < nbins for 0 <= w < dmax, [nbins + 1] the rest; then w >= thr[t]
__global__ __launch_bounds__(PC_THREADS) void pc_count_kernel(const double *__restrict__ w, int64_t G, int nbins, int n_t, double dr,
                                                              double dmax, const double *__restrict__ thr, unsigned long long *__restrict__ out)
{
    __shared__ unsigned lh[AMOF_PORE_MAX_WORDS];
    const int words = nbins + 2 + n_t;
    for (int x = threadIdx.x; x < words; x += PC_THREADS) lh[x] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * (PC_THREADS * PC_COUNT_ROUNDS);
    for (int r = 0; r < PC_COUNT_ROUNDS; r++) {
        const int64_t i = base + r * PC_THREADS + threadIdx.x;
        if (i >= G) break;
        const double v = w[i];
        int slot = nbins + 1;
        if (v < 0.0) slot = 0;
        else if (v < dmax) {
            const int b = (int)(v / dr);
            if (b < nbins) slot = 1 + b;
        }
        atomicAdd(&lh[slot], 1u);
        for (int t = 0; t < n_t; t++)
            if (v >= thr[t]) atomicAdd(&lh[nbins + 2 + t], 1u);
    }
    __syncthreads();
    for (int x = threadIdx.x; x < words; x += PC_THREADS)
        if (lh[x]) atomicAdd(&out[x], (unsigned long long)lh[x]);
}

// ------------------------------------------------------------ host side ----
struct CoverCall {
    amof_ctx *ctx = nullptr;
    int32_t n[3] = {0, 0, 0}, pbc[3] = {0, 0, 0};
    int64_t G = 0, nbk = 0;
    int32_t nbins = 0, n_t = 0;
    double dr = 0.0, dmax = 0.0;
    bool force_exact = false;
    int32_t src_cap = PC_SRC_CAP;       // AMOF_PORE_COVER_SRC_CAP=n (1 .. PC_SRC_CAP) shortens the brick list: the tests' way to the retry
    const double *cells = nullptr;      // host [n_cells][9]
    int64_t n_cells = 1;
    const PoreOutputs *out = nullptr;   // the caller's arrays: psd_hist, po_counts, po_access, cover
    // device
    double *d_w = nullptr, *d_bmax = nullptr, *d_thr = nullptr;
    PcOffset *d_st = nullptr;
    unsigned long long *d_out = nullptr;        // [words] histogram and counts, [1] covered, [1] flag, [2] statistics
    int words = 0;
    // the frame at hand
    PcFrame g;
    double vmax = 0.0, hstep[3] = {0.0, 0.0, 0.0};
    bool frame_exact = false;
    int64_t stencil_frame = -1;
    int n_st = 0;
    std::vector<double> h_bmax;
    std::vector<PcOffset> h_st;
    std::vector<unsigned long long> h_out;
    // the call
    const double *thresholds = nullptr;
    int64_t launches = 0;
    bool used_exact = false;
    double stat_src = 0.0, stat_rec = 0.0, stat_bricks = 0.0;     // sums over the full passes on pore_cover_brick
};

static unsigned pc_blocks(int64_t n, int64_t per) { return (unsigned)std::max<int64_t>(1, (n + per - 1) / per); }

// step vectors, perpendicular step heights, the brick's half diagonal.  false: the cell is singular
static bool pc_geometry(const double *C, const int32_t *n, double *A, double *hstep, double &hd)
{
    for (int k = 0; k < 3; k++)
        for (int c = 0; c < 3; c++) A[3 * k + c] = C[3 * k + c] / (double)n[k];
    double face[3][3];
    for (int k = 0; k < 3; k++) {
        const double *a = A + 3 * ((k + 1) % 3), *b = A + 3 * ((k + 2) % 3);
        face[k][0] = a[1] * b[2] - a[2] * b[1];
        face[k][1] = a[2] * b[0] - a[0] * b[2];
        face[k][2] = a[0] * b[1] - a[1] * b[0];
    }
    const double vol = fabs(A[0] * face[0][0] + A[1] * face[0][1] + A[2] * face[0][2]);
    if (!(vol > 0.0) || !isfinite(vol)) return false;
    for (int k = 0; k < 3; k++) {
        hstep[k] = vol / sqrt(face[k][0] * face[k][0] + face[k][1] * face[k][1] + face[k][2] * face[k][2]);
        if (!(hstep[k] > 0.0) || !isfinite(hstep[k])) return false;
    }
    hd = 0.0;
    for (int s = 0; s < 4; s++) {
        const double sb = (s & 1) ? -3.5 : 3.5, sc = (s & 2) ? -3.5 : 3.5;
        hd = std::max(hd, sqrt(pc_d2(A, 3.5, sb, sc)));
    }
    // the pre-tests compare float64 distances of a few hundred steps at most: their rounding is far below this margin
    hd = hd * (1.0 + 1e-6) + 1e-6;
    return true;
}

// what the call covers and where its answers go; no device work
static void pc_plan(CoverCall &c, amof_ctx *ctx, const PoreInputs &in, const PoreOutputs &out)
{
    const int32_t *grid = in.grid, *pbc = in.pbc;
    c.ctx = ctx;
    c.G = 1;
    c.nbk = 1;
    for (int k = 0; k < 3; k++) {
        c.n[k] = grid[k];
        c.pbc[k] = pbc[k] ? 1 : 0;
        c.G *= grid[k];
        c.nbk *= (grid[k] + PC_BRICK - 1) / PC_BRICK;
    }
    c.nbins = out.nbins;
    c.n_t = out.n_t;
    c.dr = in.dr;
    c.dmax = in.dmax;
    c.thresholds = in.thresholds;
    c.cells = in.t ? in.t->cell : in.cells;
    c.n_cells = in.t ? in.t->n_cells : in.n_frames;
    const char *ex = getenv("AMOF_PORE_COVER_EXACT");
    c.force_exact = ex && ex[0] == '1';
    if (const char *cap = getenv("AMOF_PORE_COVER_SRC_CAP")) c.src_cap = std::min(PC_SRC_CAP, std::max(1, atoi(cap)));
    c.words = c.nbins + 2 + c.n_t;
    c.out = &out;
}

int pore_cover_setup(CoverCall &c)
{
    amof_ctx *ctx = c.ctx;
    void *p;
    AMOF_TRY(ensure(ctx, SLOT_IMG, (size_t)c.G * sizeof(double), &p));
    c.d_w = (double *)p;
    AMOF_TRY(ensure(ctx, SLOT_NIMG, (size_t)c.nbk * sizeof(double), &p));
    c.d_bmax = (double *)p;
    // thresholds, then the counters of a frame
    c.h_out.assign((size_t)c.n_t + c.words + 4, 0ull);
    if (c.n_t > 0) memcpy(c.h_out.data(), c.thresholds, (size_t)c.n_t * sizeof(double));
    AMOF_TRY(upload(ctx, SLOT_QSPEC, c.h_out.data(), c.h_out.size() * sizeof(unsigned long long), &p));
    c.d_thr = (double *)p;
    c.d_out = (unsigned long long *)p + c.n_t;
    c.h_bmax.resize((size_t)c.nbk);
    return AMOF_OK;
}

// w, the brick maxima and the exact path's offset table, sized from the first cell
size_t pore_cover_fixed_bytes(const CoverCall &c)
{
    double A[9], hstep[3], hd;
    double offsets = 1e6;
    if (pc_geometry(c.cells, c.n, A, hstep, hd))
        offsets = std::min(1e8, 8.0 * (c.dmax / hstep[0] + 1.0) * (c.dmax / hstep[1] + 1.0) * (c.dmax / hstep[2] + 1.0));
    return (size_t)c.G * 8 + (size_t)(c.G / 64 + 64) * 8 + (size_t)offsets * sizeof(PcOffset);
}

// the field tiers start over: so do the call's counters
void pore_cover_restart(CoverCall &c)
{
    c.launches = 0;
    c.used_exact = false;
    c.stat_src = c.stat_rec = c.stat_bricks = 0.0;
}

// every offset with d2 <= vmax^2, for the frame at hand
static int pc_stencil(CoverCall &c, int64_t f)
{
    if (c.stencil_frame == f) return AMOF_OK;
    amof_ctx *ctx = c.ctx;
    c.h_st.clear();
    if (c.vmax >= 0.0) {
        const double v2 = c.vmax * c.vmax;
        for (int k = 0; k < 3; k++)
            if (c.g.R[k] > 32767 || (c.pbc[k] && c.g.R[k] > c.n[k]))
                return fail(ctx, AMOF_ECAPACITY, "pore covering: offsets of %d grid steps along axis %d", c.g.R[k], k);
        if ((2.0 * c.g.R[0] + 1.0) * (2.0 * c.g.R[1] + 1.0) * (2.0 * c.g.R[2] + 1.0) > 4e9)
            return fail(ctx, AMOF_ECAPACITY, "pore covering: the offset table of the exact path is too large");
        for (int a = -c.g.R[0]; a <= c.g.R[0]; a++)
            for (int b = -c.g.R[1]; b <= c.g.R[1]; b++)
                for (int d = -c.g.R[2]; d <= c.g.R[2]; d++) {
                    const double d2 = pc_d2(c.g.A, (double)a, (double)b, (double)d);
                    if (d2 <= v2) c.h_st.push_back(PcOffset{{(short)a, (short)b, (short)d}, 0, d2});
                }
        if ((int64_t)c.h_st.size() > PC_STENCIL_MAX)
            return fail(ctx, AMOF_ECAPACITY, "pore covering: %lld offsets exceed the exact path's table", (long long)c.h_st.size());
    }
    c.n_st = (int)c.h_st.size();
    void *p;
    AMOF_TRY(ensure(ctx, SLOT_SPEC, std::max<size_t>(16, c.h_st.size() * sizeof(PcOffset)), &p));
    c.d_st = (PcOffset *)p;
    if (c.n_st > 0) {
        AMOF_HIP_TRY(ctx, hipMemcpyAsync(c.d_st, c.h_st.data(), c.h_st.size() * sizeof(PcOffset), hipMemcpyHostToDevice, ctx->stream));
        AMOF_HIP_TRY(ctx, sync_stream(ctx));        // (the table is rebuilt for the next frame)
    }
    c.stencil_frame = f;
    return AMOF_OK;
}

template <bool ACCESS>
static int pc_brickmax(CoverCall &c, const double *d_field, const int32_t *parent, const int32_t *mark)
{
    hipLaunchKernelGGL(pc_brickmax_kernel<ACCESS>, dim3((unsigned)c.nbk), dim3(PC_THREADS), 0, c.ctx->stream, d_field, parent, mark, c.g,
                       c.d_bmax);
    AMOF_HIP_TRY(c.ctx, hipGetLastError());
    return AMOF_OK;
}

// one pass over the frame at hand on the path chosen for it; *overflow: pore_cover_brick's list was too short
template <bool ACCESS>
static int pc_pass(CoverCall &c, int64_t f, const double *d_field, const int32_t *parent, const int32_t *mark, bool exact)
{
    amof_ctx *ctx = c.ctx;
    unsigned long long *covered = c.d_out + c.words, *flags = covered + 1, *stats = flags + 1;
    if (exact) {
        AMOF_TRY(pc_stencil(c, f));
        hipLaunchKernelGGL(pc_exact_kernel<ACCESS>, dim3(pc_blocks(c.G, PC_THREADS)), dim3(PC_THREADS), 0, ctx->stream, d_field, parent, mark,
                           c.g, (const PcOffset *)c.d_st, c.n_st, c.d_w, covered);
    } else
        hipLaunchKernelGGL(pc_brick_kernel<ACCESS>, dim3((unsigned)c.nbk), dim3(PC_THREADS), 0, ctx->stream, d_field, parent, mark, c.g,
                           (const double *)c.d_bmax, c.d_w, covered, flags, stats);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    c.launches++;
    return AMOF_OK;
}

static int pc_read_out(CoverCall &c)
{
    c.h_out.resize((size_t)c.words + 4);
    return fetch(c.ctx, c.h_out.data(), c.d_out, c.h_out.size() * sizeof(unsigned long long));
}

static int pc_clear_out(CoverCall &c)
{
    AMOF_HIP_TRY(c.ctx, hipMemsetAsync(c.d_out, 0, ((size_t)c.words + 4) * sizeof(unsigned long long), c.ctx->stream));
    return AMOF_OK;
}

// w, its histogram and the occupiable counts of frame f, whose field lies on the device
int pore_cover_frame(CoverCall &c, int64_t f, const double *d_field, StageSpans &spans)
{
    amof_ctx *ctx = c.ctx;
    memset(&c.g, 0, sizeof c.g);
    c.g.src_cap = c.src_cap;
    if (!pc_geometry(c.cells + (size_t)(c.n_cells == 1 ? 0 : f) * 9, c.n, c.g.A, c.hstep, c.g.hd))
        return fail(ctx, AMOF_ESINGULAR, "pore covering: the cell of frame %lld is singular", (long long)f);
    for (int k = 0; k < 3; k++) {
        c.g.n[k] = c.n[k];
        c.g.pbc[k] = c.pbc[k];
        c.g.nb[k] = (c.n[k] + PC_BRICK - 1) / PC_BRICK;
    }
    c.g.G = c.G;
    spans.begin(3);
    AMOF_TRY(pc_brickmax<false>(c, d_field, nullptr, nullptr));
    AMOF_TRY(fetch(ctx, c.h_bmax.data(), c.d_bmax, (size_t)c.nbk * sizeof(double)));
    c.vmax = -INFINITY;
    for (double m : c.h_bmax) c.vmax = std::max(c.vmax, m);
    // |offset_k| hstep_k <= |offset| <= v(c) <= vmax for every covering centre
    double box = 1.0;
    bool fits = true;
    for (int k = 0; k < 3; k++) {
        const double r = c.vmax >= 0.0 ? floor(c.vmax / c.hstep[k] * (1.0 + 1e-9)) + 1.0 : 0.0;
        if (!(r < 1e9)) return fail(ctx, AMOF_ECAPACITY, "pore covering: the field reaches over %g grid steps", r);
        c.g.R[k] = (int32_t)r;
        fits = fits && c.g.R[k] <= 32000 && (!c.pbc[k] || c.g.R[k] <= c.n[k]);
        box *= (2.0 * r + PC_BRICK) / PC_BRICK + 5.0;        // (segments of 8 indices or fewer: the ragged ones at the image boundaries)
    }
    c.frame_exact = c.force_exact || !fits || box > (double)PC_BOX_MAX;
    for (int attempt = 0; attempt < 2; attempt++) {
        AMOF_TRY(pc_clear_out(c));
        AMOF_TRY(pc_pass<false>(c, f, d_field, nullptr, nullptr, c.frame_exact));
        hipLaunchKernelGGL(pc_count_kernel, dim3(pc_blocks(c.G, PC_THREADS * PC_COUNT_ROUNDS)), dim3(PC_THREADS), 0, ctx->stream,
                           (const double *)c.d_w, c.G, c.nbins, c.n_t, c.dr, c.dmax, (const double *)c.d_thr, c.d_out);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        AMOF_TRY(pc_read_out(c));
        if (c.frame_exact || !c.h_out[(size_t)c.words + 1]) break;
        c.frame_exact = true;           // the list of a brick was too short: the frame once more, on the exact path
    }
    spans.end();
    if (c.frame_exact) c.used_exact = true;
    else {
        c.stat_src += (double)c.h_out[(size_t)c.words + 2];
        c.stat_rec += (double)c.h_out[(size_t)c.words + 3];
        c.stat_bricks += (double)c.nbk;
    }
    for (int x = 0; x < c.nbins + 2; x++) c.out->psd_hist[(size_t)f * (c.nbins + 2) + x] = (uint64_t)c.h_out[(size_t)x];
    for (int t = 0; t < c.n_t; t++) c.out->po_counts[(size_t)f * c.n_t + t] = (int64_t)c.h_out[(size_t)c.nbins + 2 + t];
    if (c.out->cover) AMOF_TRY(fetch(ctx, c.out->cover + (size_t)f * (size_t)c.G, c.d_w, (size_t)c.G * sizeof(double)));
    return AMOF_OK;
}

// the points of frame f covered from a channel of V(thresholds[k])
int pore_cover_threshold(CoverCall &c, int64_t f, int32_t k, const double *d_field, const int32_t *parent, const int32_t *mark, bool channels,
                         StageSpans &spans)
{
    int64_t &out = c.out->po_access[(size_t)f * c.n_t + k];
    out = 0;
    if (!channels) return AMOF_OK;
    // On the path of the frame's full pass.  The channels' centres are a subset of all centres: a destination brick keeps no
    // more source bricks here than it did there, so a frame that stayed on pore_cover_brick cannot overflow the list now.
    spans.begin(3);
    AMOF_TRY(pc_clear_out(c));
    if (!c.frame_exact) AMOF_TRY(pc_brickmax<true>(c, d_field, parent, mark));
    AMOF_TRY(pc_pass<true>(c, f, d_field, parent, mark, c.frame_exact));
    AMOF_TRY(pc_read_out(c));
    spans.end();
    if (!c.frame_exact && c.h_out[(size_t)c.words + 1])
        return fail(c.ctx, AMOF_EHIP, "pore covering: the accessible pass of frame %lld kept more source bricks than the full pass", (long long)f);
    out = (int64_t)c.h_out[(size_t)c.words];
    return AMOF_OK;
}

// the checks both entry points share, in the order of pore_check.h; the record's sizes
static int pc_check(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out)
{
    double nb = 0.0;
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_given(in.thresholds, in.n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::bin_width(in.dr, in.dmax, nb)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_finite(in.thresholds, in.n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::counter_words(nb, in.n_t, out.nbins)));
    AMOF_TRY(pore_refuse(ctx, pore_check::grid(in.grid, nullptr)));
    AMOF_TRY(pore_refuse(ctx, pore_check::psd_outputs(in.n_frames, in.n_t, out.psd_hist, out.po_counts)));
    if (out.cover) AMOF_TRY(pore_refuse(ctx, pore_check::per_point_cap((int64_t)in.grid[0] * in.grid[1] * in.grid[2], "array")));
    out.sized(in.n_frames, in.grid, in.n_t);
    return pore_refuse(ctx, pore_check::po_access_given(out.F, in.n_t, in.want_access, out.po_access));
}

void pore_cover_report(const CoverCall &c)
{
    c.ctx->last_path = c.used_exact ? "pore_cover_exact" : "pore_cover_brick";
    c.ctx->dom_launches = c.launches;
    c.ctx->cover_stats[0] = c.stat_bricks;
    c.ctx->cover_stats[1] = c.stat_src;
    c.ctx->cover_stats[2] = c.stat_rec;
}

}  // namespace amof

using namespace amof;

extern "C" int amof_pore_psd(amof_ctx *ctx, const amof_traj *t, const double *radii, const int32_t *grid, double dr, double dmax,
                             const double *thresholds, int32_t n_t, int32_t want_access, int32_t want_free, uint64_t *hist, int64_t *counts,
                             double *vmax, int64_t *argmax, int64_t *access, double *free_sphere, double *field, int32_t *labels,
                             uint64_t *psd_hist, int64_t *po_counts, int64_t *po_access, double *cover)
{
    if (!ctx) return AMOF_EINVAL;
    const bool labelled = want_access || want_free;
    PoreOutputs out{hist, counts, vmax, argmax, field, labelled ? access : nullptr, labelled ? free_sphere : nullptr, labelled ? labels : nullptr,
                    psd_hist, po_counts, want_access ? po_access : nullptr, cover};     // (what the call does not ask for is not the record's)
    AMOF_TRY(pore_refuse(ctx, pore_check::both_given(t, grid)));
    const int32_t pbc[3] = {t->pbc[0], t->pbc[1], t->pbc[2]};
    const PoreInputs in{t, radii, nullptr, nullptr, t->n_frames, grid, pbc, dr, dmax, thresholds, n_t, want_access, want_free};
    AMOF_TRY(pc_check(ctx, in, out));
    CoverCall c;
    pc_plan(c, ctx, in, out);
    PoreStages stages{nullptr, &c};
    return out.keep(labelled ? pore_access_run(ctx, in, out, &c) : pore_field_run(ctx, in, out, &stages));
}

int amof::pore_psd_surface_run(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out, bool want_psd, SurfaceCall &surface)
{
    const bool labelled = in.want_access || in.want_free;
    CoverCall c;
    if (want_psd) {
        AMOF_TRY(pc_check(ctx, in, out));
        pc_plan(c, ctx, in, out);
    }
    PoreStages stages{nullptr, want_psd ? &c : nullptr, false, &surface, in.n_t};
    return labelled ? pore_access_run(ctx, in, out, want_psd ? &c : nullptr, &surface) : pore_field_run(ctx, in, out, &stages);
}

extern "C" int amof_pore_psd_field(amof_ctx *ctx, const double *field, const double *cells, int64_t n_frames, const int32_t *grid,
                                   const int32_t *pbc, double dr, double dmax, const double *thresholds, int32_t n_t, int32_t want_access,
                                   uint64_t *psd_hist, int64_t *po_counts, int64_t *po_access, double *cover)
{
    if (!ctx) return AMOF_EINVAL;
    PoreOutputs out{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, psd_hist, po_counts, po_access, cover};
    AMOF_TRY(pore_refuse(ctx, pore_check::given_field_inputs(grid, pbc, n_frames, field, true, cells)));
    const int32_t per[3] = {pbc[0] ? 1 : 0, pbc[1] ? 1 : 0, pbc[2] ? 1 : 0};
    const PoreInputs in{nullptr, nullptr, field, cells, n_frames, grid, per, dr, dmax, thresholds, n_t, want_access, 0};
    AMOF_TRY(pc_check(ctx, in, out));
    if (n_frames == 0) return AMOF_OK;
    const size_t G = (size_t)out.G;
    // one image at most: no value above half the smallest periodic perpendicular height of its frame's cell
    for (int64_t f = 0; f < n_frames; f++) {
        double A[9], hstep[3], hd;
        if (!pc_geometry(cells + (size_t)f * 9, grid, A, hstep, hd)) return fail(ctx, AMOF_ESINGULAR, "the cell of frame %lld is singular", (long long)f);
        double hmin = INFINITY, top;
        for (int k = 0; k < 3; k++)
            if (per[k]) hmin = std::min(hmin, hstep[k] * (double)grid[k]);
        AMOF_TRY(pore_refuse(ctx, pore_check::field_finite(field + (size_t)f * G, G, top)));
        AMOF_TRY(pore_refuse(ctx, pore_check::half_height_field(top, f, hmin)));
    }
    if (want_access) AMOF_TRY(pore_refuse(ctx, pore_check::grid(grid, per)));
    CoverCall c;
    pc_plan(c, ctx, in, out);
    out.zero(false);
    PoreStages stages{nullptr, &c};
    return out.keep(want_access ? pore_access_run(ctx, in, out, &c) : pore_given_field_run(ctx, in, out, stages, "pore_cover_brick"));
}

extern "C" int amof_pore_cover_stats(const amof_ctx *ctx, double *out3)
{
    if (!ctx || !out3) return AMOF_EINVAL;
    for (int k = 0; k < 3; k++) out3[k] = ctx->cover_stats[k];
    return AMOF_OK;
}
