// Bond survival correlations: intermittent C(t) and continuous S(t) counters of neighbour pairs (gfx950).
//
// h_ij(f) = 1 iff atom j (species B) is a neighbour of atom i (species A), i != j, in frame f: amof_cn_count's decision --
// the canonical minimum image of DESIGN §2 in frame f's cell, strict sqrt(d2) < rc.  The cutoff is at most half the smallest
// perpendicular cell height on every periodic axis (refused otherwise), so one image at most is in reach and h is 0 or 1.
// Per set (A, B) and lag m = windows[w], over the origins k = 1, 1 + s, ... <= F - m - 1 and the ordered pairs with the
// centre i in [atom_begin, atom_end):
//   counts[.][w][0] = sum h(k)    [1] = sum h(k) h(k + m)    [2] = sum prod_{f = k .. k + m} h(f)
// Stages of a call (one (set, slice of centres) piece at a time, so that no table grows with N^2):
//   bond_list_kernel     every origin frame of lag 0 (a superset of every lag's origins): centres x partners through LDS
//                        tiles, float64 canonical vector, d2 < rc^2 (1 + 1e-9) -- a superset of the bonded pairs is enough,
//                        a pair that is never bonded only carries an all-zero series -- into a bitmap [centre][partner
//                        rank]; bond_rowcount_kernel + a host prefix sum + bond_compact_kernel turn it into the table of
//                        pairs (i, j), sorted and free of duplicates by construction; the table is built
//                        for groups of whole rows of at most 2^25 pairs (256 MB; AMOF_BOND_PAIR_BUDGET, in pairs, overrides).
//                        The stage is bond_pair_groups (bond_pairs.h), which lindemann.hip calls too: the list kernel walks the
//                        frames first + stride o, with first = 1 for the analyses of this file.
//   bond_series_kernel   a lane owns a pair, a wave 64 pairs and one u64 word: 64 frames in a row, frame f's decision into
//                        bit f & 63.  The pairs are sorted by centre, so the lanes of a wave read neighbouring atoms of one
//                        frame.  (bond_series_frames_kernel, AMOF_BOND_LAYOUT=frames: a lane owns a frame, the word is the
//                        wave's ballot -- every lane then reads 24 B out of a different frame; kept for the comparison in
//                        profiles/bond/bond_timing.md.)
//     "bond_series"        constant diagonal cell, all axes periodic: fractional coordinates folded and quantised to 2^-32,
//                          f32 distance of the wrapped u32 differences (the chain of nbr.hip's nbr_fast_dist), pairs inside
//                          the guard band (fast_guard_rel + the fixed-point grid) re-decided by the canonical arithmetic
//     "bond_series_exact"  every other cell (general, per-frame, open axes), or AMOF_BOND_EXACT=1: canonical arithmetic only
//   bond_corr_kernel     a lane owns a pair and a range of its words: popcounts of h & origin mask and of
//                        h & (h >> m) & origin mask (word-crossing shift) per lag; the run of ones in front of every origin
//                        (ctz of the complement, carried across words) gives the number of lags it survives.  u64 counters
//                        in LDS, one global u64 atomic per counter and workgroup.
//   bond_final_kernel    sorted-lag counters -> counts[n_sets][W][3] (suffix sums of the survival histogram)
// AMOF_BOND_REPORT=1 prints the number of pairs of every piece to stderr (profiles/tools/bond_timing.py).
//
// Bond reorientation (amof_bond_reorientation[_dev]) shares the list, compaction and series stages -- unchanged, launched as
// above -- and replaces bond_corr_kernel / bond_final_kernel by
//   bond_vector_kernel   a lane owns a pair, a wave 64 frames (the series kernel's shape): the canonical float64 vector
//                        d_ij(f) of pair_base<ORTHO>, every path, into the table [F][3][Pc] (SLOT_AUX5); the chunk of pairs is
//                        sized so that the table stays within 256 MB (64 pairs at least).  The f32 fast form decides h only.
//   bond_reorient_kernel bond_corr_kernel's lanes and word ranges; per lag it walks the set bits of h & (h >> m) & origin
//                        mask, reads d(k) and d(k + m) (consecutive pairs: coalesced), cos = dot / sqrt(dot dot) clamped,
//                        P1 = cos, P2 = fma(1.5 cos, cos, -0.5), both as rint(P 2^e) in int64; n, sum P1, sum P2 reduced
//                        over the wave by shuffles into u64 LDS counters, one global u64 atomic per counter and workgroup.
//                        A term with a zero-length vector raises a flag: AMOF_EANGLE (host out: zeros; device out: untouched).
//   bond_reorient_final_kernel  sorted-lag counters -> out[n_sets][W][3]
// "bond_reorient" / "bond_reorient_exact" name the h decision that ran ("bond_series" / "bond_series_exact").  Stage spans:
// 0 the lists, 1 the series (both as the survival call), 2 the vector table and the reorientation correlations.
// LDS: bond_list_kernel 6 KB static; bond_corr_kernel and bond_reorient_kernel 28 B per lag of a launch (<= BC_LAGS = 2048
// lags: 56 KB); the series and vector kernels use none.  No kernel spills (checked with
// -Rpass-analysis=kernel-resource-usage).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "bond_pairs.h"
#include "nbr_check.h"

namespace amof {
namespace {

constexpr int BL_THREADS = BOND_LIST_TILE;      // bond_list_kernel: a centre per thread, partner tiles of 256 atoms
constexpr int BS_THREADS = 256;         // series kernels: four waves, four words
constexpr int BC_THREADS = 256;         // bond_corr_kernel: 64 pairs x four word ranges
constexpr int BC_LAGS = 2048;           // lags per launch of bond_corr_kernel
constexpr size_t BOND_BITMAP_BYTES = (size_t)256 << 20;     // bitmap of a piece (2^31 bits: a piece has < 2^31 pairs)
constexpr size_t BOND_WORDS_BYTES = (size_t)256 << 20;      // series words of a chunk of pairs
constexpr size_t BOND_PAIR_BYTES = (size_t)256 << 20;       // pair table of a group of rows (AMOF_BOND_PAIR_BUDGET, in pairs, overrides)
constexpr size_t BOND_VEC_BYTES = (size_t)256 << 20;        // reorientation: vector table of a chunk of pairs

struct BondListArgs {
    const double *pos;
    const double *geom;
    const int32_t *perm;
    unsigned *bitmap;           // [rows][wpr]
    int64_t N, first, stride;   // the frames first + stride o, o < n_origins (the bond analyses: first = 1)
    int32_t n_cells, n_origins, opc;
    int32_t seg_a, rows;        // centres perm[seg_a .. seg_a + rows)
    int32_t seg_b, nb;          // partners perm[seg_b .. seg_b + nb)
    int32_t self_off;           // same species: centre row r is partner rank r + self_off; else INT_MIN
    int32_t wpr;
    double rc2_hi;
};

template <bool ORTHO>
__global__ __launch_bounds__(BL_THREADS) void bond_list_kernel(BondListArgs a)
{
    __shared__ double tx[BL_THREADS], ty[BL_THREADS], tz[BL_THREADS];
    const int tid = threadIdx.x;
    const int row = blockIdx.x * BL_THREADS + tid;
    const bool has = row < a.rows;
    const int64_t ai = has ? a.perm[a.seg_a + row] : 0;
    const int self_rank = row + a.self_off;
    unsigned *__restrict__ brow = a.bitmap + (size_t)(has ? row : 0) * a.wpr;
    const int o0 = blockIdx.y * a.opc, o1 = min(o0 + a.opc, a.n_origins);
    for (int o = o0; o < o1; o++) {
        const int64_t f = a.first + a.stride * o;
        const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
        const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
        const double xi = p[ai * 3 + 0], yi = p[ai * 3 + 1], zi = p[ai * 3 + 2];
        for (int j0 = 0; j0 < a.nb; j0 += BL_THREADS) {
            const int nj = min(BL_THREADS, a.nb - j0);
            __syncthreads();
            if (tid < nj) {
                const int64_t aj = a.perm[a.seg_b + j0 + tid];
                tx[tid] = p[aj * 3 + 0];
                ty[tid] = p[aj * 3 + 1];
                tz[tid] = p[aj * 3 + 2];
            }
            __syncthreads();
            if (!has) continue;
            for (int j = 0; j < nj; j++) {
                double dx, dy, dz;
                pair_base<ORTHO>(g, tx[j] - xi, ty[j] - yi, tz[j] - zi, dx, dy, dz);
                if (norm2(dx, dy, dz) < a.rc2_hi && j0 + j != self_rank) {
                    const int b = j0 + j;
                    const unsigned bit = 1u << (b & 31);
                    // (the plain load only spares an atomic: a stale word costs one idempotent OR)
                    if (!(brow[b >> 5] & bit)) atomicOr(&brow[b >> 5], bit);
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void bond_rowcount_kernel(const unsigned *__restrict__ bitmap, int rows, int wpr,
                                                            unsigned *__restrict__ rowcnt)
{
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= rows) return;
    const unsigned *__restrict__ b = bitmap + (size_t)row * wpr;
    unsigned n = 0;
    for (int k = 0; k < wpr; k++) n += __popc(b[k]);
    rowcnt[row] = n;
}

// rows [row0, row0 + rows) of the bitmap; rowoff[k]: first pair of row row0 + k in this group's table
__global__ __launch_bounds__(256) void bond_compact_kernel(const unsigned *__restrict__ bitmap, int row0, int rows, int wpr,
                                                           const unsigned *__restrict__ rowoff, const int32_t *__restrict__ perm,
                                                           int seg_a, int seg_b, int2 *__restrict__ pairs)
{
    const int k0 = blockIdx.x * 256 + threadIdx.x;
    if (k0 >= rows) return;
    const int row = row0 + k0;
    const unsigned *__restrict__ b = bitmap + (size_t)row * wpr;
    const int ai = perm[seg_a + row];
    size_t o = rowoff[k0];
    for (int k = 0; k < wpr; k++) {
        unsigned v = b[k];
        while (v) {
            const int bit = __ffs(v) - 1;
            v &= v - 1;
            pairs[o++] = make_int2(ai, perm[seg_b + 32 * k + bit]);
        }
    }
}

}  // namespace

size_t bond_pair_budget()
{
    if (const char *e = getenv("AMOF_BOND_PAIR_BUDGET")) {
        const long long v = atoll(e);
        if (v > 0) return (size_t)v;
    }
    return BOND_PAIR_BYTES / sizeof(int2);
}

// the pair-table stage (bond_pairs.h): pieces of centres, groups of whole rows, each(table, pairs) per group
int bond_pair_groups(const BondPairCall &c, int s, int A, int B, double rc, int64_t atom_begin, int64_t atom_end,
                     const std::function<int(const int2 *, size_t)> &each)
{
    amof_ctx *ctx = c.ctx;
    StageSpans &spans = *c.spans;
    const HostTiles &tiles = *c.tiles;
    const std::vector<int64_t> &sp_first = tiles.sp_first;
    const int64_t nA = tiles.nsp[(size_t)A], nB = tiles.nsp[(size_t)B];
    if (!(rc > 0.0) || nA == 0 || nB == 0) return AMOF_OK;
    // centres of the atom range: the species segment of perm is ascending in the atom index
    const int32_t *seg = tiles.perm.data() + sp_first[(size_t)A];
    const int64_t a0 = std::lower_bound(seg, seg + nA, (int32_t)atom_begin) - seg;
    const int64_t a1 = std::lower_bound(seg, seg + nA, (int32_t)std::min<int64_t>(atom_end, 0x7fffffffLL)) - seg;
    if (a0 >= a1) return AMOF_OK;
    const int wpr = (int)((nB + 31) / 32);
    const int64_t rows_max = std::max<int64_t>(1, (int64_t)(BOND_BITMAP_BYTES / 4) / wpr);
    const int64_t n_origins = c.n_origins;
    for (int64_t c0 = a0; c0 < a1; c0 += rows_max) {
        const int rows = (int)std::min<int64_t>(rows_max, a1 - c0);
        // ---- the pairs bonded at any origin ----
        spans.begin(0);
        void *d_bitmap = nullptr, *d_rowcnt = nullptr;
        const size_t bm_bytes = (size_t)rows * wpr * sizeof(unsigned);
        AMOF_TRY(ensure(ctx, SLOT_AUX0, bm_bytes, &d_bitmap));
        AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)rows * sizeof(unsigned), &d_rowcnt));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_bitmap, 0, bm_bytes, ctx->stream));
        BondListArgs la;
        memset(&la, 0, sizeof la);
        la.pos = c.pos_dev;
        la.geom = c.d_geom;
        la.perm = c.d_perm;
        la.bitmap = (unsigned *)d_bitmap;
        la.N = c.N;
        la.first = c.first_frame;
        la.stride = c.stride;
        la.n_cells = c.n_cells;
        la.n_origins = (int32_t)n_origins;
        la.seg_a = (int32_t)(sp_first[(size_t)A] + c0);
        la.rows = rows;
        la.seg_b = (int32_t)sp_first[(size_t)B];
        la.nb = (int32_t)nB;
        la.self_off = A == B ? (int32_t)c0 : INT32_MIN / 2;
        la.wpr = wpr;
        la.rc2_hi = rc * rc * (1.0 + 1e-9);
        const int row_tiles = (rows + BL_THREADS - 1) / BL_THREADS;
        // origins per workgroup: enough workgroups to fill the GPU several times over, at most 65535 in y
        int64_t opc = std::max<int64_t>(1, std::min<int64_t>(16, n_origins * row_tiles / 2048));
        opc = std::max<int64_t>(opc, (n_origins + 65534) / 65535);
        la.opc = (int32_t)opc;
        const dim3 lgrid((unsigned)row_tiles, (unsigned)((n_origins + opc - 1) / opc));
        if (c.ortho) hipLaunchKernelGGL(bond_list_kernel<true>, lgrid, dim3(BL_THREADS), 0, ctx->stream, la);
        else hipLaunchKernelGGL(bond_list_kernel<false>, lgrid, dim3(BL_THREADS), 0, ctx->stream, la);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(bond_rowcount_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const unsigned *)d_bitmap, rows, wpr, (unsigned *)d_rowcnt);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        std::vector<unsigned> rowcnt((size_t)rows);
        AMOF_TRY(fetch(ctx, rowcnt.data(), d_rowcnt, (size_t)rows * sizeof(unsigned)));
        spans.end();
        if (getenv("AMOF_BOND_REPORT")) {
            size_t total = 0;
            for (unsigned n : rowcnt) total += n;
            fprintf(stderr, "amof_bond: set %d centres [%lld, %lld) of its species: %zu pairs\n", s, (long long)c0,
                    (long long)(c0 + rows), total);
        }
        // the pair table is bounded like the bitmap: groups of whole rows of at most pair_max pairs (one row, which has
        // fewer than 2^31, where a single row holds more)
        for (int r0 = 0; r0 < rows;) {
            std::vector<unsigned> rowoff;
            size_t P = 0;
            int r1 = r0;
            while (r1 < rows && (r1 == r0 || P + rowcnt[(size_t)r1] <= c.pair_max)) {
                rowoff.push_back((unsigned)P);
                P += rowcnt[(size_t)r1++];
            }
            const int gr0 = r0, grows = r1 - r0;
            r0 = r1;
            if (P == 0) continue;
            spans.begin(0);
            void *d_rowoff = nullptr, *d_pairs = nullptr;
            AMOF_TRY(upload(ctx, SLOT_AUX2, rowoff.data(), (size_t)grows * sizeof(unsigned), &d_rowoff));
            AMOF_TRY(ensure(ctx, SLOT_AUX3, P * sizeof(int2), &d_pairs));
            hipLaunchKernelGGL(bond_compact_kernel, dim3((unsigned)((grows + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const unsigned *)d_bitmap, gr0, grows, wpr, (const unsigned *)d_rowoff, c.d_perm, la.seg_a, la.seg_b,
                               (int2 *)d_pairs);
            AMOF_HIP_TRY(ctx, hipGetLastError());
            spans.end();
            // rowoff dies with this iteration: a copy too big for the staging ring has consumed it when upload returns, one
            // through the ring was copied there at once
            AMOF_TRY(each((const int2 *)d_pairs, P));
        }
    }
    return AMOF_OK;
}

namespace {

struct BondSeriesArgs {
    const double *pos;
    const double *geom;
    const int2 *pairs;                  // this chunk's pairs
    unsigned long long *words;          // [nwords][P]
    int64_t N;
    int32_t F, P, nwords, n_cells;
    double rc;
    double inv[3];                      // fast form: 1 / L_c
    float sc[3];                        // L_c 2^-32
    float r_in, r_out;
};

// fractional coordinate folded into [0, 1) and quantised to 2^-32 (quantize_atom's rule on a diagonal cell)
__device__ __forceinline__ uint32_t bond_q(double x, double inv, bool &far)
{
    double s = x * inv;
    if (!(fabs(s) < 1.0e4)) far = true;     // absurdly far from the cell (or NaN): the exact form decides
    s = s - floor(s);
    const double t = s * 4294967296.0;
    return t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
}

// h_ij(f): FAST -- f32 candidate from the wrapped fixed-point differences, the guard band re-decided exactly
template <bool FAST, bool ORTHO>
__device__ __forceinline__ bool bond_decide(const BondSeriesArgs &a, int f, int i, int j)
{
    const double *__restrict__ pi = a.pos + ((size_t)f * (size_t)a.N + (size_t)i) * 3;
    const double *__restrict__ pj = a.pos + ((size_t)f * (size_t)a.N + (size_t)j) * 3;
    const double xi = pi[0], yi = pi[1], zi = pi[2], xj = pj[0], yj = pj[1], zj = pj[2];
    if (FAST) {
        bool far = false;
        const float fx = (float)(int)(bond_q(xj, a.inv[0], far) - bond_q(xi, a.inv[0], far));
        const float fy = (float)(int)(bond_q(yj, a.inv[1], far) - bond_q(yi, a.inv[1], far));
        const float fz = (float)(int)(bond_q(zj, a.inv[2], far) - bond_q(zi, a.inv[2], far));
        const float dx = fx * a.sc[0], dy = fy * a.sc[1], dz = fz * a.sc[2];
        const float d = __builtin_amdgcn_sqrtf(fmaf(dz, dz, fmaf(dy, dy, dx * dx)));
        if (!far) {
            if (d < a.r_in) return true;
            if (!(d < a.r_out)) return false;
        }
    }
    const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    double dx, dy, dz;
    pair_base<ORTHO>(g, xj - xi, yj - yi, zj - zi, dx, dy, dz);
    return sqrt(norm2(dx, dy, dz)) < a.rc;
}

// a lane owns a pair; the wave's word is blockIdx.x * 4 + wave (frames 64 q .. 64 q + 63)
template <bool FAST, bool ORTHO>
__global__ __launch_bounds__(BS_THREADS) void bond_series_kernel(BondSeriesArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * (BS_THREADS / 64) + wave;
    const int p = blockIdx.y * 64 + lane;
    if (q >= a.nwords || p >= a.P) return;
    const int2 ij = a.pairs[p];
    const int f0 = q * 64, nf = min(64, a.F - f0);
    unsigned long long word = 0ull;
#pragma unroll 4
    for (int b = 0; b < nf; b++)
        if (bond_decide<FAST, ORTHO>(a, f0 + b, ij.x, ij.y)) word |= 1ull << b;
    a.words[(size_t)q * a.P + p] = word;
}

// a lane owns a frame; a wave owns a pair and walks four words
template <bool FAST, bool ORTHO>
__global__ __launch_bounds__(BS_THREADS) void bond_series_frames_kernel(BondSeriesArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.y * (BS_THREADS / 64) + wave;
    if (p >= a.P) return;
    const int2 ij = a.pairs[p];
    for (int q = blockIdx.x * 4; q < min(blockIdx.x * 4 + 4, a.nwords); q++) {
        const int f = q * 64 + lane;
        const bool h = f < a.F && bond_decide<FAST, ORTHO>(a, f, ij.x, ij.y);
        const unsigned long long word = __ballot(h);
        if (lane == 0) a.words[(size_t)q * a.P + p] = word;
    }
}

struct BondCorrArgs {
    const unsigned long long *words;    // [nwords][P]
    const unsigned long long *obase;    // [nwords] bit k set: k = 1 + s o (k < F)
    const int32_t *lags;                // sorted, distinct [Wu]
    unsigned long long *G;              // this set's counters [3][Wu]
    int32_t F, P, nwords, Wu, w0, w1;
};

__device__ __forceinline__ int bond_ctz(unsigned long long v) { return v ? __ffsll(v) - 1 : 64; }

__global__ __launch_bounds__(BC_THREADS) void bond_corr_kernel(BondCorrArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int nl = a.w1 - a.w0;
    unsigned long long *c_n0 = reinterpret_cast<unsigned long long *>(lds_raw);      // [nl] bonds at the origins
    unsigned long long *c_in = c_n0 + nl;                                             // [nl] intermittent
    unsigned long long *c_sv = c_in + nl;                                             // [nl] origins surviving exactly c + 1 lags
    int32_t *lag = reinterpret_cast<int32_t *>(c_sv + nl);                            // [nl]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < 3 * nl; k += BC_THREADS) c_n0[k] = 0ull;
    for (int k = tid; k < nl; k += BC_THREADS) lag[k] = a.lags[a.w0 + k];
    __syncthreads();

    const int p = blockIdx.x * 64 + lane;
    const bool has = p < a.P;
    const int R = gridDim.y * (BC_THREADS / 64), r = blockIdx.y * (BC_THREADS / 64) + wave;
    const int qa = (int)((long long)a.nwords * r / R), qb = (int)((long long)a.nwords * (r + 1) / R);
    const unsigned long long *__restrict__ hw = a.words + (has ? p : 0);
    const size_t P = (size_t)a.P;
    const int nwords = a.nwords;

    // bonds at the origins and intermittent pairs, lag by lag
    for (int w = 0; w < nl; w++) {
        const int m = lag[w];
        const int lim = a.F - m - 1;            // the last origin frame of this lag
        unsigned n0 = 0, ni = 0;
        if (has && lim >= 1) {
            const int mq = m >> 6, mr = m & 63;
            for (int q = qa; q < qb && q * 64 <= lim; q++) {
                unsigned long long om = a.obase[q];
                const int top = lim - q * 64;   // bits 0 .. top of this word are origins of the lag
                if (top < 63) om &= (2ull << top) - 1ull;
                const unsigned long long x = hw[(size_t)q * P] & om;
                if (!x) continue;
                const int q2 = q + mq;
                const unsigned long long lo = q2 < nwords ? hw[(size_t)q2 * P] : 0ull;
                unsigned long long sh = lo;
                if (mr) {
                    const unsigned long long hi = q2 + 1 < nwords ? hw[(size_t)(q2 + 1) * P] : 0ull;
                    sh = (lo >> mr) | (hi << (64 - mr));
                }
                n0 += __popcll(x);
                ni += __popcll(x & sh);
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            n0 += __shfl_down(n0, off, 64);
            ni += __shfl_down(ni, off, 64);
        }
        if (lane == 0) {
            if (n0) atomicAdd(&c_n0[w], (unsigned long long)n0);
            if (ni) atomicAdd(&c_in[w], (unsigned long long)ni);
        }
    }

    // continuous: the run of ones that starts at every origin; an origin with run L counts for the lags m < L
    if (has) {
        long long carry = 0;                    // ones in a row from bit 0 of word q + 1 on
        for (int q = qb; q < nwords; q++) {
            const unsigned long long v = hw[(size_t)q * P];
            if (v == ~0ull) { carry += 64; continue; }
            carry += bond_ctz(~v);
            break;
        }
        int last = 0;                           // run-length coding of the counter updates: neighbouring origins mostly agree
        unsigned pending = 0;
        for (int q = qb - 1; q >= qa; q--) {
            const unsigned long long v = hw[(size_t)q * P];
            unsigned long long x = v & a.obase[q];
            while (x) {
                const int b = 63 - __clzll(x);  // from the top: runs shrink monotonically inside a run of ones
                x &= ~(1ull << b);
                const int z = bond_ctz(~(v >> b));          // (v >> b shifts zeros in: z <= 64 - b)
                const long long L = z == 64 - b ? (long long)z + carry : (long long)z;
                // c = number of lags of this launch below L
                int lo = 0, hi = nl;
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if ((long long)lag[mid] < L) lo = mid + 1; else hi = mid;
                }
                if (lo != last) {
                    if (pending && last > 0) atomicAdd(&c_sv[last - 1], (unsigned long long)pending);
                    last = lo;
                    pending = 0;
                }
                pending++;
            }
            carry = v == ~0ull ? carry + 64 : (long long)bond_ctz(~v);
        }
        if (pending && last > 0) atomicAdd(&c_sv[last - 1], (unsigned long long)pending);
    }
    __syncthreads();
    for (int k = tid; k < 3 * nl; k += BC_THREADS) {
        const unsigned long long v = c_n0[k];
        if (v) atomicAdd(&a.G[(size_t)(k / nl) * a.Wu + a.w0 + (k % nl)], v);
    }
}

// counts[s][w][c] (+)= the sorted-lag counters; the continuous count of a lag is the suffix sum, inside its launch's lags,
// of the survival histogram
__global__ __launch_bounds__(256) void bond_final_kernel(const unsigned long long *__restrict__ G, const int32_t *__restrict__ map,
                                                         int n_sets, int W, int Wu, int add, unsigned long long *__restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sets * W) return;
    const int s = k / W, w = k % W, u = map[w];
    const unsigned long long *__restrict__ g = G + (size_t)s * 3 * Wu;
    const int end = min((u / BC_LAGS + 1) * BC_LAGS, Wu);
    unsigned long long cont = 0ull;
    for (int x = u; x < end; x++) cont += g[2 * (size_t)Wu + x];
    unsigned long long *__restrict__ o = out + (size_t)k * 3;
    if (add) {
        o[0] += g[u];
        o[1] += g[Wu + u];
        o[2] += cont;
    } else {
        o[0] = g[u];
        o[1] = g[Wu + u];
        o[2] = cont;
    }
}

// ---- reorientation ----
struct BondVecArgs {
    const double *pos;
    const double *geom;
    const int2 *pairs;                  // this chunk's pairs
    double *tab;                        // [F][3][P]
    int64_t N;
    int32_t F, P, nwords, n_cells;
};

// the series kernel's shape: a lane owns a pair, the wave frames 64 q .. 64 q + 63
template <bool ORTHO>
__global__ __launch_bounds__(BS_THREADS) void bond_vector_kernel(BondVecArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q = blockIdx.x * (BS_THREADS / 64) + wave;
    const int p = blockIdx.y * 64 + lane;
    if (q >= a.nwords || p >= a.P) return;
    const int2 ij = a.pairs[p];
    const int f0 = q * 64, nf = min(64, a.F - f0);
    const size_t P = (size_t)a.P;
    for (int b = 0; b < nf; b++) {
        const int f = f0 + b;
        const double *__restrict__ pi = a.pos + ((size_t)f * (size_t)a.N + (size_t)ij.x) * 3;
        const double *__restrict__ pj = a.pos + ((size_t)f * (size_t)a.N + (size_t)ij.y) * 3;
        const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
        double dx, dy, dz;
        pair_base<ORTHO>(g, pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2], dx, dy, dz);
        double *__restrict__ o = a.tab + (size_t)f * 3 * P + p;
        o[0] = dx;
        o[P] = dy;
        o[2 * P] = dz;
    }
}

struct BondReorArgs {
    const unsigned long long *words;    // [nwords][P]
    const unsigned long long *obase;    // [nwords]
    const int32_t *lags;                // sorted, distinct [Wu]
    const double *tab;                  // [F][3][P]
    unsigned long long *G;              // this set's counters [3][Wu]: n, sum rint(P1 2^e), sum rint(P2 2^e)
    int32_t *flag;                      // a contributing term had a zero-length vector
    int32_t F, P, nwords, Wu, w0, w1;
    double scale;                       // 2^e
};

__device__ __forceinline__ double bond_dot(double ax, double ay, double az, double bx, double by, double bz)
{
    return fma(az, bz, fma(ay, by, ax * bx));       // norm2's chain
}

__global__ __launch_bounds__(BC_THREADS) void bond_reorient_kernel(BondReorArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    const int nl = a.w1 - a.w0;
    unsigned long long *c_n = reinterpret_cast<unsigned long long *>(lds_raw);       // [nl] pairs bonded at both ends
    unsigned long long *c_p1 = c_n + nl;                                              // [nl]
    unsigned long long *c_p2 = c_p1 + nl;                                             // [nl]
    int32_t *lag = reinterpret_cast<int32_t *>(c_p2 + nl);                            // [nl]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int k = tid; k < 3 * nl; k += BC_THREADS) c_n[k] = 0ull;
    for (int k = tid; k < nl; k += BC_THREADS) lag[k] = a.lags[a.w0 + k];
    __syncthreads();

    const int p = blockIdx.x * 64 + lane;
    const bool has = p < a.P;
    const int R = gridDim.y * (BC_THREADS / 64), r = blockIdx.y * (BC_THREADS / 64) + wave;
    const int qa = (int)((long long)a.nwords * r / R), qb = (int)((long long)a.nwords * (r + 1) / R);
    const unsigned long long *__restrict__ hw = a.words + (has ? p : 0);
    const double *__restrict__ tab = a.tab + (has ? p : 0);
    const size_t P = (size_t)a.P;
    const int nwords = a.nwords;
    bool bad = false;

    for (int w = 0; w < nl; w++) {
        const int m = lag[w];
        const int lim = a.F - m - 1;            // the last origin frame of this lag
        unsigned n = 0;
        long long s1 = 0, s2 = 0;
        if (has && lim >= 1) {
            const int mq = m >> 6, mr = m & 63;
            for (int q = qa; q < qb && q * 64 <= lim; q++) {
                unsigned long long om = a.obase[q];
                const int top = lim - q * 64;   // bits 0 .. top of this word are origins of the lag
                if (top < 63) om &= (2ull << top) - 1ull;
                unsigned long long x = hw[(size_t)q * P] & om;
                if (!x) continue;
                const int q2 = q + mq;
                const unsigned long long lo = q2 < nwords ? hw[(size_t)q2 * P] : 0ull;
                unsigned long long sh = lo;
                if (mr) {
                    const unsigned long long hi = q2 + 1 < nwords ? hw[(size_t)(q2 + 1) * P] : 0ull;
                    sh = (lo >> mr) | (hi << (64 - mr));
                }
                x &= sh;
                n += __popcll(x);
                while (x) {
                    const int k = q * 64 + __ffsll(x) - 1;      // h(k) h(k + m) = 1: k + m <= F - 1
                    x &= x - 1;
                    const double *__restrict__ da = tab + (size_t)k * 3 * P;
                    const double *__restrict__ db = tab + (size_t)(k + m) * 3 * P;
                    const double ax = da[0], ay = da[P], az = da[2 * P];
                    const double bx = db[0], by = db[P], bz = db[2 * P];
                    const double den = bond_dot(ax, ay, az, ax, ay, az) * bond_dot(bx, by, bz, bx, by, bz);
                    if (!(den > 0.0)) {
                        bad = true;
                        continue;
                    }
                    double c = bond_dot(ax, ay, az, bx, by, bz) / sqrt(den);
                    c = fmin(fmax(c, -1.0), 1.0);
                    const double p2 = fma(1.5 * c, c, -0.5);
                    s1 += (long long)rint(c * a.scale);
                    s2 += (long long)rint(p2 * a.scale);
                }
            }
        }
        for (int off = 32; off > 0; off >>= 1) {
            n += __shfl_down(n, off, 64);
            s1 += __shfl_down(s1, off, 64);
            s2 += __shfl_down(s2, off, 64);
        }
        if (lane == 0 && n) {
            atomicAdd(&c_n[w], (unsigned long long)n);
            atomicAdd(&c_p1[w], (unsigned long long)s1);
            atomicAdd(&c_p2[w], (unsigned long long)s2);
        }
    }
    if (bad) *a.flag = 1;
    __syncthreads();
    for (int k = tid; k < 3 * nl; k += BC_THREADS) {
        const unsigned long long v = c_n[k];
        if (v) atomicAdd(&a.G[(size_t)(k / nl) * a.Wu + a.w0 + (k % nl)], v);
    }
}

// out[s][w][c] (+)= the sorted-lag counters
__global__ __launch_bounds__(256) void bond_reorient_final_kernel(const unsigned long long *__restrict__ G, const int32_t *__restrict__ map,
                                                                  int n_sets, int W, int Wu, int add, unsigned long long *__restrict__ out)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_sets * W) return;
    const int s = k / W, u = map[k % W];
    const unsigned long long *__restrict__ g = G + (size_t)s * 3 * Wu;
    unsigned long long *__restrict__ o = out + (size_t)k * 3;
    for (int c = 0; c < 3; c++) {
        const unsigned long long v = g[(size_t)c * Wu + u];
        o[c] = add ? o[c] + v : v;
    }
}

// e_s = min(40, 62 - bit_length(n_a n_b n_0)); < 20 (a product of 2^43 and more, or one beyond u64): refused by the caller
int reorient_scale_log2(int64_t n_a, int64_t n_b, int64_t n_0)
{
    unsigned long long ab = 0, abo = 0;
    if (__builtin_mul_overflow((unsigned long long)n_a, (unsigned long long)n_b, &ab) ||
        __builtin_mul_overflow(ab, (unsigned long long)n_0, &abo))
        return -1;
    const int bits = abo ? 64 - __builtin_clzll(abo) : 0;
    return std::min(40, 62 - bits);
}

// what a reorientation call adds to bond_run's arguments
struct Reorient {
    int64_t *out;           // host [n_sets][W][3], overwritten, or NULL
    int64_t *out_dev;       // device, added into, or NULL
    int32_t *scale_log2;    // host [n_sets]
};

// counts (host, overwritten) or counts_dev (device, added into); ro: the reorientation sums instead
int bond_run(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets, const int32_t *windows,
             int32_t W, int64_t stride, int64_t atom_begin, int64_t atom_end, uint64_t *counts, uint64_t *counts_dev, const Reorient *ro = nullptr)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    const int S = t->n_species;
    const int64_t N = t->n_atoms, F = t->n_frames;
    if (!cutoff || n_sets < 0 || (n_sets > 0 && !sets)) return fail(ctx, AMOF_EINVAL, "NULL argument");
    AMOF_TRY(check_lag_args(ctx, windows, W, F, stride));
    if (atom_begin < 0 || atom_end > N || atom_begin > atom_end)
        return fail(ctx, AMOF_EINVAL, "atom range [%lld, %lld) outside [0, %lld)", (long long)atom_begin, (long long)atom_end, (long long)N);
    if (F > 0x7fffff00LL - 64) return fail(ctx, AMOF_EINVAL, "too many frames");
    for (int s = 0; s < n_sets; s++) {
        AMOF_TRY(pore_refuse(ctx, nbr_check::bond_set_species(sets, s, S)));
        AMOF_TRY(pore_refuse(ctx, nbr_check::bond_set_cutoff(cutoff[sets[2 * s] * S + sets[2 * s + 1]], s)));
    }
    const size_t csize = (size_t)n_sets * W * 3;
    if (counts) std::fill(counts, counts + csize, (uint64_t)0);
    if (ro) {
        // the scale depends on the trajectory, the set and the stride alone: never on the atom range or the chunking.  (Counted
        // here and not taken from build_tiles below: a call that returns early -- no windows, one frame -- still reports it.)
        std::vector<int64_t> nsp((size_t)S, 0);
        for (int64_t i = 0; i < N; i++) nsp[(size_t)t->species[i]]++;
        const int64_t n0 = lag_origin_count(F, 0, stride);
        for (int s = 0; s < n_sets; s++) {
            const int e = reorient_scale_log2(nsp[(size_t)sets[2 * s]], nsp[(size_t)sets[2 * s + 1]], n0);
            if (e < 20)
                return fail(ctx, AMOF_EINVAL, "set %d: %lld x %lld pairs x %lld origins leave a fixed-point quantum above 2^-20: use a "
                                              "larger origin stride or fewer frames per call",
                            s, (long long)nsp[(size_t)sets[2 * s]], (long long)nsp[(size_t)sets[2 * s + 1]], (long long)n0);
            ro->scale_log2[s] = e;
        }
        if (ro->out) std::fill(ro->out, ro->out + csize, (int64_t)0);
    }
    if (csize == 0 || F < 2 || N < 2) return AMOF_OK;

    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    const double hmin = nbr_check::min_periodic_height(t->pbc, geom.rec.data(), t->n_cells);
    for (int s = 0; s < n_sets; s++)
        AMOF_TRY(pore_refuse(ctx, nbr_check::half_height_set(cutoff[sets[2 * s] * S + sets[2 * s + 1]], s, hmin, "a pair could be bonded twice")));
    HostTiles tiles;
    build_tiles(t, BL_THREADS, tiles);

    // sorted distinct lags and where every window finds its own
    std::vector<int32_t> lags(windows, windows + W);
    std::sort(lags.begin(), lags.end());
    lags.erase(std::unique(lags.begin(), lags.end()), lags.end());
    const int Wu = (int)lags.size();
    std::vector<int32_t> map((size_t)W);
    for (int w = 0; w < W; w++) map[(size_t)w] = (int32_t)(std::lower_bound(lags.begin(), lags.end(), windows[w]) - lags.begin());
    const int nwords = (int)((F + 63) / 64);
    const int64_t n_origins = lag_origin_count(F, 0, stride);      // lag 0's origins: a superset of every lag's
    if (n_origins > 0x7fffffffLL) return fail(ctx, AMOF_EINVAL, "too many frames");
    std::vector<unsigned long long> obase((size_t)nwords, 0ull);
    for (int64_t o = 0; o < n_origins; o++) {
        const int64_t k = lag_origin_frame(o, stride);
        obase[(size_t)(k >> 6)] |= 1ull << (k & 63);
    }

    // ---- path selection ----
    const char *env_exact = getenv("AMOF_BOND_EXACT");
    bool pbc_all = t->pbc[0] && t->pbc[1] && t->pbc[2];
    const bool fast = !(env_exact && env_exact[0] == '1') && t->n_cells == 1 && geom.all_ortho && pbc_all;
    const char *env_layout = getenv("AMOF_BOND_LAYOUT");
    const bool by_frames = env_layout && !strcmp(env_layout, "frames");
    const bool ortho = geom.all_ortho;

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    StageSpans spans(ctx);      // list, series, correlation
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(geom.rec.data(), geom.rec.size() * sizeof(double));
    const int i_perm = pk.add(tiles.perm.data(), tiles.perm.size() * sizeof(int32_t));
    const int i_lags = pk.add(lags.data(), lags.size() * sizeof(int32_t));
    const int i_map = pk.add(map.data(), map.size() * sizeof(int32_t));
    const int i_obase = pk.add(obase.data(), obase.size() * sizeof(unsigned long long));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    const size_t gsize = (size_t)n_sets * 3 * Wu;
    void *d_G = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_OUT1, gsize * sizeof(uint64_t), &d_G));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_G, 0, gsize * sizeof(uint64_t), ctx->stream));

    BondSeriesArgs sa;
    memset(&sa, 0, sizeof sa);
    sa.pos = pos_dev;
    sa.geom = pk.ptr<double>(i_geom);
    sa.N = N;
    sa.F = (int32_t)F;
    sa.nwords = nwords;
    sa.n_cells = (int32_t)t->n_cells;
    double grel = 0.0, gabs = 0.0;
    if (fast) {
        // the f32 chain's error (fast_guard_rel, + 3u: the cutoff rounded to f32 and the roundings of rc -+ g) and the
        // fixed-point grid, which moves a distance by < csum 2^-32 (x2 margin) -- as nbr.hip's fast kernels
        const double *c0 = t->cell;
        grel = fast_guard_rel(geom, 1) + 3.0 / 16777216.0;
        gabs = (fabs(c0[0]) + fabs(c0[4]) + fabs(c0[8])) * (1.0 / 2147483648.0);
        for (int x = 0; x < 3; x++) {
            sa.inv[x] = geom.rec[9 + 4 * x];
            sa.sc[x] = (float)(c0[4 * x] * (1.0 / 4294967296.0));
        }
    }
    const char *series_path = ro ? (fast ? "bond_reorient" : "bond_reorient_exact") : (fast ? "bond_series" : "bond_series_exact");
    void *d_flag = nullptr;
    if (ro) {
        AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
    }
    int64_t series_launches = 0;
    ctx->last_path = series_path;
    BondPairCall pc;
    pc.ctx = ctx;
    pc.spans = &spans;
    pc.pos_dev = pos_dev;
    pc.d_geom = pk.ptr<double>(i_geom);
    pc.d_perm = pk.ptr<int32_t>(i_perm);
    pc.tiles = &tiles;
    pc.N = N;
    pc.n_cells = (int32_t)t->n_cells;
    pc.ortho = ortho;
    pc.first_frame = 1;
    pc.stride = stride;
    pc.n_origins = n_origins;
    pc.pair_max = bond_pair_budget();

    for (int s = 0; s < n_sets; s++) {
        const int A = sets[2 * s], B = sets[2 * s + 1];
        const double rc = cutoff[A * S + B];
        sa.rc = rc;
        if (fast) {
            const float rcf = (float)rc;
            float g = (float)((double)rcf * grel + gabs);
            if ((double)g < (double)rcf * grel + gabs) g = nextafterf(g, INFINITY);
            sa.r_in = rcf - g;
            sa.r_out = rcf + g;
        }
        AMOF_TRY(bond_pair_groups(pc, s, A, B, rc, atom_begin, atom_end, [&](const int2 *d_pairs, size_t P) -> int {
            // ---- series and correlations, a chunk of pairs at a time ----
            size_t pc_max = std::max<size_t>(64, std::min<size_t>((size_t)65535 * 4, BOND_WORDS_BYTES / 8 / (size_t)nwords) / 64 * 64);
            if (ro) pc_max = std::max<size_t>(64, std::min<size_t>(pc_max, BOND_VEC_BYTES / 24 / (size_t)F) / 64 * 64);
            for (size_t p0 = 0; p0 < P; p0 += pc_max) {
                const int Pc = (int)std::min(pc_max, P - p0);
                void *d_words = nullptr;
                AMOF_TRY(ensure(ctx, SLOT_AUX4, (size_t)nwords * Pc * sizeof(uint64_t), &d_words));
                sa.pairs = (const int2 *)d_pairs + p0;
                sa.words = (unsigned long long *)d_words;
                sa.P = Pc;
                spans.begin(1);
                if (series_launches == 0) timing_dom_begin(ctx, series_path);
                auto launch = [&](auto lanes, auto frames) {
                    if (by_frames)
                        hipLaunchKernelGGL(frames, dim3((unsigned)((nwords + 3) / 4), (unsigned)((Pc + 3) / 4)), dim3(BS_THREADS), 0,
                                           ctx->stream, sa);
                    else
                        hipLaunchKernelGGL(lanes, dim3((unsigned)((nwords + 3) / 4), (unsigned)((Pc + 63) / 64)), dim3(BS_THREADS), 0,
                                           ctx->stream, sa);
                };
                if (fast) launch(bond_series_kernel<true, true>, bond_series_frames_kernel<true, true>);
                else if (ortho) launch(bond_series_kernel<false, true>, bond_series_frames_kernel<false, true>);
                else launch(bond_series_kernel<false, false>, bond_series_frames_kernel<false, false>);
                AMOF_HIP_TRY(ctx, hipGetLastError());
                series_launches++;
                timing_dom_end(ctx, series_launches);
                spans.end();

                // ---- correlations of the chunk: the survival counters, or the vector table and the reorientation sums ----
                spans.begin(2);
                // word ranges: four per workgroup; more workgroups while the pairs alone do not fill the GPU; BC_LAGS lags
                // per launch (both kernels: 28 B of LDS per lag)
                auto launch_lags = [&](auto kernel, auto &args) -> int {
                    const int pblocks = (Pc + 63) / 64;
                    const int ysplit = (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>((nwords + 3) / 4, 64), 2048 / pblocks));
                    AMOF_HIP_TRY(ctx, allow_max_lds((const void *)kernel));
                    for (int w0 = 0; w0 < Wu; w0 += BC_LAGS) {
                        args.w0 = w0;
                        args.w1 = std::min(w0 + BC_LAGS, Wu);
                        const size_t lds = (size_t)(args.w1 - args.w0) * (3 * sizeof(uint64_t) + sizeof(int32_t));
                        hipLaunchKernelGGL(kernel, dim3((unsigned)pblocks, (unsigned)ysplit), dim3(BC_THREADS), lds, ctx->stream, args);
                        AMOF_HIP_TRY(ctx, hipGetLastError());
                    }
                    return AMOF_OK;
                };
                if (ro) {
                    void *d_tab = nullptr;
                    AMOF_TRY(ensure(ctx, SLOT_AUX5, (size_t)F * 3 * Pc * sizeof(double), &d_tab));
                    BondVecArgs va;
                    memset(&va, 0, sizeof va);
                    va.pos = pos_dev;
                    va.geom = sa.geom;
                    va.pairs = sa.pairs;
                    va.tab = (double *)d_tab;
                    va.N = N;
                    va.F = (int32_t)F;
                    va.P = Pc;
                    va.nwords = nwords;
                    va.n_cells = (int32_t)t->n_cells;
                    const dim3 vgrid((unsigned)((nwords + 3) / 4), (unsigned)((Pc + 63) / 64));
                    if (ortho) hipLaunchKernelGGL(bond_vector_kernel<true>, vgrid, dim3(BS_THREADS), 0, ctx->stream, va);
                    else hipLaunchKernelGGL(bond_vector_kernel<false>, vgrid, dim3(BS_THREADS), 0, ctx->stream, va);
                    AMOF_HIP_TRY(ctx, hipGetLastError());
                    BondReorArgs ra;
                    memset(&ra, 0, sizeof ra);
                    ra.words = (const unsigned long long *)d_words;
                    ra.obase = pk.ptr<unsigned long long>(i_obase);
                    ra.lags = pk.ptr<int32_t>(i_lags);
                    ra.tab = (const double *)d_tab;
                    ra.G = (unsigned long long *)d_G + (size_t)s * 3 * Wu;
                    ra.flag = (int32_t *)d_flag;
                    ra.F = (int32_t)F;
                    ra.P = Pc;
                    ra.nwords = nwords;
                    ra.Wu = Wu;
                    ra.scale = ldexp(1.0, ro->scale_log2[s]);
                    AMOF_TRY(launch_lags(bond_reorient_kernel, ra));
                } else {
                    BondCorrArgs ca;
                    memset(&ca, 0, sizeof ca);
                    ca.words = (const unsigned long long *)d_words;
                    ca.obase = pk.ptr<unsigned long long>(i_obase);
                    ca.lags = pk.ptr<int32_t>(i_lags);
                    ca.G = (unsigned long long *)d_G + (size_t)s * 3 * Wu;
                    ca.F = (int32_t)F;
                    ca.P = Pc;
                    ca.nwords = nwords;
                    ca.Wu = Wu;
                    AMOF_TRY(launch_lags(bond_corr_kernel, ca));
                }
                spans.end();
            }
            return AMOF_OK;
        }));
    }
    if (ro) {
        // a zero-length vector among the terms: an error return; the host out holds the zeros it was given above, the device
        // buffer is untouched
        int32_t flag = 0;
        timing_end(ctx);
        AMOF_TRY(fetch(ctx, &flag, d_flag, sizeof flag));
        spans.collect();
        if (flag) return fail(ctx, AMOF_EANGLE, "a bonded pair has a zero-length vector: the angle is undefined");
        void *d_ro = ro->out_dev;
        if (!d_ro) AMOF_TRY(ensure(ctx, SLOT_OUT0, csize * sizeof(int64_t), &d_ro));
        hipLaunchKernelGGL(bond_reorient_final_kernel, dim3((unsigned)(((size_t)n_sets * W + 255) / 256)), dim3(256), 0, ctx->stream,
                           (const unsigned long long *)d_G, pk.ptr<int32_t>(i_map), (int)n_sets, (int)W, Wu, ro->out_dev ? 1 : 0,
                           (unsigned long long *)d_ro);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        if (ro->out) AMOF_TRY(fetch(ctx, ro->out, d_ro, csize * sizeof(int64_t)));
        AMOF_HIP_TRY(ctx, sync_stream(ctx));
        return AMOF_OK;
    }
    void *d_out = counts_dev;
    if (!counts_dev) AMOF_TRY(ensure(ctx, SLOT_OUT0, csize * sizeof(uint64_t), &d_out));
    hipLaunchKernelGGL(bond_final_kernel, dim3((unsigned)(((size_t)n_sets * W + 255) / 256)), dim3(256), 0, ctx->stream,
                       (const unsigned long long *)d_G, pk.ptr<int32_t>(i_map), (int)n_sets, (int)W, Wu, counts_dev ? 1 : 0,
                       (unsigned long long *)d_out);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    timing_end(ctx);
    if (counts) AMOF_TRY(fetch(ctx, counts, d_out, csize * sizeof(uint64_t)));
    // host tables above live on this stack frame: finish before returning
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_bond_survival(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                  const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t atom_begin,
                                  int64_t atom_end, uint64_t *counts)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts) return fail(ctx, AMOF_EINVAL, "counts is NULL");
    return bond_run(ctx, traj, cutoff, sets, n_sets, windows, n_windows, origin_stride, atom_begin, atom_end, counts, nullptr);
}

extern "C" int amof_bond_survival_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                      const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t atom_begin,
                                      int64_t atom_end, uint64_t *counts_dev)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev) return fail(ctx, AMOF_EINVAL, "counts is NULL");
    return bond_run(ctx, traj, cutoff, sets, n_sets, windows, n_windows, origin_stride, atom_begin, atom_end, nullptr, counts_dev);
}

extern "C" int amof_bond_reorientation(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                       const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t atom_begin,
                                       int64_t atom_end, int64_t *out, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!out || !scale_log2) return fail(ctx, AMOF_EINVAL, "out or scale_log2 is NULL");
    const Reorient ro = {out, nullptr, scale_log2};
    return bond_run(ctx, traj, cutoff, sets, n_sets, windows, n_windows, origin_stride, atom_begin, atom_end, nullptr, nullptr, &ro);
}

extern "C" int amof_bond_reorientation_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                           const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t atom_begin,
                                           int64_t atom_end, int64_t *out_dev, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!out_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "out or scale_log2 is NULL");
    const Reorient ro = {nullptr, out_dev, scale_log2};
    return bond_run(ctx, traj, cutoff, sets, n_sets, windows, n_windows, origin_stride, atom_begin, atom_end, nullptr, nullptr, &ro);
}
