// RDF pair-distance histogram kernels (gfx950).
//
// Replaces asap3's RawRDF as driven by the reference at amof/rdf.py:88-93.  Kernel families, picked per call by
// rdf_run (amof_last_path names the one that produced the result):
//   rdf_exact      rdf_tile_kernel<ORTHO,EXTRA> / rdf_tile_kernel_global: canonical float64 arithmetic per pair and
//                  per periodic image; partially periodic cells, large image shares, nbins beyond the LDS histogram
//   rdf_tile       rdf_tile_kernel_fast<ORTHO,CULL>: 32-bit fixed-point minimum image, f32 candidate bins with an
//                  exact re-decision near every edge, slab-sorted tiles by LDS-DMA (half-cell cutoffs); general cells
//                  on the lower-triangular factor of their metric (guard_math.h)
//   rdf_tile_zf    the same for diagonal cells (the headline): ZF = f32 slab-axis coordinates per step -- the slab-sorted
//                  axis needs no per-pair wrap (with culling: every visited partner; without: all but the band around
//                  the sub-tile's antipode) -- and the always-add LDS histogram (every lane adds to its candidate bin,
//                  out-of-range pairs to trash words, flagged pairs are fixed up by the refinement: no lane masks)
//   rdf_tile_img   the same with IMG = true: cutoffs beyond half a cell height (sheared cells at the default
//                  cutoff); pairs within reach of a cell face are parked and evaluated canonically, images included
//   rdf_range      rdf_range_kernel_fast: 2-level (slab x y-bin) cell list for small cutoffs
//   rdf_cell       rdf_cell_kernel: 3-D cell list, one lane per centre atom, for cutoffs far below the cell size
//
// Common decomposition of the tile kernels: atoms are sorted by species once per call (the species of an atom never
// change along a trajectory) and cut into species-pure tiles.  A workgroup owns ONE unordered tile pair (I <= J) and
// a chunk of consecutive frames; tile J is staged in LDS and read by broadcast, and the pair's species key is uniform
// per workgroup, so a single nbins-wide u32 histogram in LDS serves the whole workgroup.  It is flushed with u64
// global atomics once per frame chunk.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <tuple>
#include <type_traits>
#include <vector>

#include "amof_internal.h"
#include "rdf_select.h"
#include "rdf_sat_math.h"

namespace amof {

constexpr int RDF_TILE = 256;

struct RdfArgs {
    const double *pos;      // [F][N][3]
    const double *geom;     // [n_cells][GEOM_STRIDE]
    const double *img;      // [n_cells][max_img][3]
    const int32_t *nimg;    // [n_cells]
    const int32_t *perm;    // [N] species-sorted atom ids
    const Tile *tiles;
    const int2 *pairs;      // [n_pairs] (tile I, tile J), I <= J
    unsigned long long *U;  // [S*S][nbins] unordered-key histograms
    int64_t N;
    int32_t F;
    int32_t n_cells;
    int32_t frames_per_chunk;
    int32_t nbins;
    int32_t S;
    int32_t max_img;
    double rmax2;
    double dr;
};

__device__ __forceinline__ void rdf_count(unsigned *hist, double d2, double rmax2, double dr, int nbins)
{
    if (d2 < rmax2) {
        // exact IEEE sqrt and divide: the bin index is an integer result and
        // must equal the oracle's bit for bit
        int b = (int)(sqrt(d2) / dr);
        if (b < nbins) atomicAdd(&hist[b], 1u);
    }
}

template <bool ORTHO, bool EXTRA>
__global__ __launch_bounds__(RDF_TILE) void rdf_tile_kernel(RdfArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double *tjx = reinterpret_cast<double *>(lds_raw);
    double *tjy = tjx + RDF_TILE;
    double *tjz = tjy + RDF_TILE;
    unsigned *hist = reinterpret_cast<unsigned *>(tjz + RDF_TILE);

    const int tid = threadIdx.x;
    const int2 pr = a.pairs[blockIdx.x];
    const Tile ti = a.tiles[pr.x];
    const Tile tj = a.tiles[pr.y];
    const bool diag = pr.x == pr.y;

    for (int k = tid; k < a.nbins; k += RDF_TILE) hist[k] = 0u;

    const int f0 = blockIdx.y * a.frames_per_chunk;
    const int f1 = min(f0 + a.frames_per_chunk, a.F);
    const int64_t ai = tid < ti.count ? a.perm[ti.start + tid] : -1;
    const int64_t aj = tid < tj.count ? a.perm[tj.start + tid] : -1;
    const double rmax2 = a.rmax2, dr = a.dr;
    const int nbins = a.nbins;

    for (int f = f0; f < f1; f++) {
        const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
        const int gi = a.n_cells == 1 ? 0 : f;
        const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
        __syncthreads();  // previous frame's tile J fully consumed (and hist zeroed)
        if (aj >= 0) {
            tjx[tid] = p[aj * 3 + 0];
            tjy[tid] = p[aj * 3 + 1];
            tjz[tid] = p[aj * 3 + 2];
        }
        double xi = 0.0, yi = 0.0, zi = 0.0;
        if (ai >= 0) {
            xi = p[ai * 3 + 0];
            yi = p[ai * 3 + 1];
            zi = p[ai * 3 + 2];
        }
        __syncthreads();
        if (ai >= 0) {
            const int jbeg = diag ? tid + 1 : 0;
            const int ne = EXTRA ? a.nimg[gi] : 0;
            const double *__restrict__ E = EXTRA ? a.img + (size_t)gi * a.max_img * 3 : nullptr;
            for (int j = jbeg; j < tj.count; j++) {
                double dx, dy, dz;
                pair_base<ORTHO>(g, tjx[j] - xi, tjy[j] - yi, tjz[j] - zi, dx, dy, dz);
                rdf_count(hist, norm2(dx, dy, dz), rmax2, dr, nbins);
                if (EXTRA) {
                    for (int m = 0; m < ne; m++)
                        rdf_count(hist, norm2(dx + E[3 * m], dy + E[3 * m + 1], dz + E[3 * m + 2]), rmax2, dr,
                                  nbins);
                }
            }
        }
    }
    __syncthreads();
    // species key (lo, hi): tiles are species-sorted so ti.species <= tj.species
    unsigned long long *U = a.U + ((size_t)ti.species * a.S + tj.species) * (size_t)nbins;
    for (int k = tid; k < nbins; k += RDF_TILE) {
        unsigned v = hist[k];
        if (v) atomicAdd(&U[k], (unsigned long long)v);
    }
}

// Same decomposition with the histogram in global memory (nbins too large for
// LDS).  Slow path, kept for completeness of the API.
template <bool ORTHO, bool EXTRA>
__global__ __launch_bounds__(RDF_TILE) void rdf_tile_kernel_global(RdfArgs a)
{
    __shared__ double tjx[RDF_TILE], tjy[RDF_TILE], tjz[RDF_TILE];
    const int tid = threadIdx.x;
    const int2 pr = a.pairs[blockIdx.x];
    const Tile ti = a.tiles[pr.x];
    const Tile tj = a.tiles[pr.y];
    const bool diag = pr.x == pr.y;
    const int f0 = blockIdx.y * a.frames_per_chunk;
    const int f1 = min(f0 + a.frames_per_chunk, a.F);
    const int64_t ai = tid < ti.count ? a.perm[ti.start + tid] : -1;
    const int64_t aj = tid < tj.count ? a.perm[tj.start + tid] : -1;
    unsigned long long *U = a.U + ((size_t)ti.species * a.S + tj.species) * (size_t)a.nbins;
    for (int f = f0; f < f1; f++) {
        const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
        const int gi = a.n_cells == 1 ? 0 : f;
        const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
        __syncthreads();
        if (aj >= 0) {
            tjx[tid] = p[aj * 3 + 0];
            tjy[tid] = p[aj * 3 + 1];
            tjz[tid] = p[aj * 3 + 2];
        }
        double xi = 0.0, yi = 0.0, zi = 0.0;
        if (ai >= 0) {
            xi = p[ai * 3 + 0];
            yi = p[ai * 3 + 1];
            zi = p[ai * 3 + 2];
        }
        __syncthreads();
        if (ai >= 0) {
            const int jbeg = diag ? tid + 1 : 0;
            const int ne = EXTRA ? a.nimg[gi] : 0;
            const double *__restrict__ E = EXTRA ? a.img + (size_t)gi * a.max_img * 3 : nullptr;
            for (int j = jbeg; j < tj.count; j++) {
                double dx, dy, dz;
                pair_base<ORTHO>(g, tjx[j] - xi, tjy[j] - yi, tjz[j] - zi, dx, dy, dz);
                double d2 = norm2(dx, dy, dz);
                if (d2 < a.rmax2) {
                    int b = (int)(sqrt(d2) / a.dr);
                    if (b < a.nbins) atomicAdd(&U[b], 1ull);
                }
                if (EXTRA) {
                    for (int m = 0; m < ne; m++) {
                        double e2 = norm2(dx + E[3 * m], dy + E[3 * m + 1], dz + E[3 * m + 2]);
                        if (e2 < a.rmax2) {
                            int b = (int)(sqrt(e2) / a.dr);
                            if (b < a.nbins) atomicAdd(&U[b], 1ull);
                        }
                    }
                }
            }
        }
    }
}

// --------------------------------------------------------------------------
// Fast path (fully periodic cells whose cutoff needs no extra images).
//
// quantize_kernel folds every atom into the cell once per frame and stores its
// fractional coordinates as 32-bit fixed point, species-sorted (16 B / atom).
// In the pair loop the minimum image is then free -- the u32 difference wraps --
// and an f32 candidate bin q~ = sqrt(d2~)/dr is accepted only when it is
// provably the canonical one:  |q~ - q| <= g_f  with
//     g_f = nbins * eps_f + g_m,   g_m = quant / dr + nbins * 1e-12,   quant = 2^-31 * (|c0|+|c1|+|c2|)
// eps_f = fast_guard_rel() bounds the relative error of the f32 chain (cvt, scale, squares/fma and
// v_sqrt_f32; 3.3e-7 for diagonal cells, (5 kappa + 3.06) * 2^-24 * 1.1 for sheared ones); the
// fixed-point grid moves a distance by < quant.  A lane whose q~ lies within g_f of an integer (or
// of nbins) is refined: first with the f64 distance of the same integer differences (decides unless
// within g_m of the edge), then with the canonical f64 arithmetic and exact sqrt/divide.  At
// |s_k| = 1/2 the wrapped image and the canonical one may differ: in a diagonal cell both have the
// same length; sheared cells take the fast path only when the cutoff stays clear of every half
// height, so both images are out of range there.
// (the per-cell record of the fast path, FrameScale, and the sizes of the tile kernel: rdf_select.h)

struct RdfFastArgs {
    RdfArgs a;
    const QAtom *Q;          // [nf][N] species-sorted, slab-sorted
    const FrameScale *fs;    // [n_cells]
    int32_t f_base;          // first frame of this batch
    int32_t nf;              // frames in this batch
    float half_m_guard;      // 1/2 - g_f rounded DOWN (g_f in bins: the f32 candidate's error bound)
    float nb_hi;             // nbins + g_f rounded UP
    double guard64;          // g_m (bins): f64-from-fixed-point candidate
    double guard64_2;        // 2 g_m (1 + 1e-9), g_m^2 (1 + 1e-9): level 2 decides on T - e^2 against +-(2 e g_m + g_m^2)
    double guard64_sq;
    int32_t xcd_map;         // 1: chunk -> XCD affinity mapping of the grid
    int32_t n_chunks;        // tile kernel: frames [c nf_main / n_chunks, (c+1) nf_main / n_chunks) belong to chunk c
    int32_t nf_main;         // tile kernel: frames dealt in chunks (nf, or with the XCD mapping the multiple of 8 below it: the
                             // nf % 8 frames behind them are rows n_chunks .. of the grid, one frame each, on whatever XCD)
    int32_t img_queue;       // IMG variant: capacity of one parking buffer
    int32_t img_defer;       // 1: two small buffers, a step's parked pairs are evaluated at the start of the next step
                             // (no extra barrier); 0: one large buffer, evaluated at the end of the step
    int32_t noreach;         // rdf_tile_zf with slab culling: 1 = every quad of a diagonal tile pair masked (AMOF_RDF_NOREACH)
    int32_t plan_noskip;     // PLAN: 1 = steps without a quad to visit are run all the same (AMOF_RDF_PLAN_NOSKIP: measurements)
    const uint4 *plan;       // PLAN: [pairs][nf][4] one TilePlanRecord per step, pair-major (rdf_tile_plan_kernel, tile_plan.h)
    float sat_one_p_guard;   // SAT (rdf_sat_math.h): 1 + g rounded to nearest (that rounding is a term of g) and 2 g rounded UP,
                             // g the bound of the saturating chain (sat_thresholds)
    float sat_two_guard;
};

constexpr int FAST_THREADS = 256;

// a wave-uniform double, moved to scalar registers
__device__ __forceinline__ double uniform_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}

// candidate bin coordinate q~ = |r_j - r_i| / dr from the fixed-point fractional coordinates
template <bool ORTHO>
__device__ __forceinline__ float fast_q(const float *sc, int ix, int iy, int iz)
{
    const float fx = (float)ix, fy = (float)iy, fz = (float)iz;
    float t;
    if (ORTHO) {
        // squares first, then the squared scales sc[3..5]: 7u on t instead of 9u (see fast_guard_rel)
        const float x2 = fx * fx, y2 = fy * fy, z2 = fz * fz;
        t = fmaf(z2, sc[5], fmaf(y2, sc[4], x2 * sc[3]));
    } else {
        // general cell: the scales are the lower-triangular factor of the cell's metric (lower_factor, amof_internal.h)
        const float dx = fmaf(fz, sc[6], fmaf(fy, sc[3], fx * sc[0]));
        const float dy = fmaf(fz, sc[7], fy * sc[4]);
        const float dz = fz * sc[8];
        t = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
    }
    return __builtin_amdgcn_sqrtf(t);
}

// ZF form (diagonal cell, slab-culled tile pairs): the slab-axis difference needs no per-pair wrap -- the partners a
// step visits lie within reach of the centre sub-tile's slab range -- so it arrives as the difference dz of two f32
// values already in units of bins (partner and centre relative to the sub-tile's slab midpoint, one rounding each):
// v_sub_f32 + v_fmac_f32 instead of v_sub_u32 + v_cvt_f32_i32 + v_mul_f32 + v_fmac_f32.  Error bound: fast_guard_zf.
__device__ __forceinline__ float fast_q_zf(const float *sc, int ix, int iy, float dz)
{
    const float fx = (float)ix, fy = (float)iy;
    const float x2 = fx * fx, y2 = fy * fy;
    return __builtin_amdgcn_sqrtf(fmaf(dz, dz, fmaf(y2, sc[4], x2 * sc[3])));
}

// squared candidate coordinate (bins^2) in f64 from the fixed-point differences
template <bool ORTHO>
__device__ __forceinline__ double medium_t(const double *sc, int ix, int iy, int iz)
{
    const double fx = (double)ix, fy = (double)iy, fz = (double)iz;
    double dx, dy, dz;
    if (ORTHO) {
        dx = fx * sc[0]; dy = fy * sc[1]; dz = fz * sc[2];
    } else {
        dx = fma(fz, sc[6], fma(fy, sc[3], fx * sc[0]));
        dy = fma(fz, sc[7], fy * sc[4]);
        dz = fz * sc[8];
    }
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// Refinement of a pair whose f32 candidate q sits within g_f of the bin edge
// e = rint(q).  Level 2 decides on which side of e the pair lies from the f64
// squared distance T of the same fixed-point differences (error: the 2^-32 grid
// only): T >= (e+g_m)^2 -> bin e, T < (e-g_m)^2 -> bin e-1 (bin nbins = out of
// range).  Level 3 (|q - e| <= g_m, or coincident atoms): canonical arithmetic
// on the original float64 positions with exact sqrt and divide.
// (ZF kernels keep the partner's f32 slab coordinate in qj.w: the atom index then comes from the quantised frame, qseg[j])
// PROV: the fast path has already counted the pair in its candidate bin (int)q (always-add scheme): take that back.
// LATE (the planned tile kernels): level 3 -- a pair in a million -- addresses what it reads beyond the tile itself: the frame's
// positions, the cell record and the quantised partner segment, from the kernel's arguments read again at that point (scalar
// loads from the kernel-argument segment, which the empty statement keeps there) and the two words of `late`; g, p and qseg are
// not used.  As three pointers made at the head of every step they were carried through the quad loops in spilled scalar
// registers (profiles/r14/tile_step_state.txt).
// SAT (with PROV; rdf_sat_math.h): q is q' = q~ + g + 1 and `hist` the histogram one word up.  The edge is rint(q' - (1 + g)),
// and the provisional count is taken back at the word the fast path used: the same fma and mask on the same q', not (int)q.
struct LateRefs {
    int fl;          // frame of the step, relative to the batch
    int j_start;     // first atom of tile J in the species-sorted frame
};
typedef const RdfFastArgs __attribute__((address_space(4))) *rdf_kernarg_t;

template <bool ORTHO, bool ZF = false, bool PROV = false, bool LATE = false, bool SAT = false>
__device__ __forceinline__ void rdf_pair_refine(unsigned *hist, const RdfFastArgs &fa,
                                                const double *sc64, const double *__restrict__ g,
                                                float q, uint32_t uix, uint32_t uiy, uint32_t uiz, uint4 qj,
                                                const double *__restrict__ p, uint32_t idx_i,
                                                const QAtom *__restrict__ qseg = nullptr, int j = 0, const LateRefs *late = nullptr)
{
    const int ix = (int)(qj.x - uix), iy = (int)(qj.y - uiy), iz = (int)(qj.z - uiz);
    static_assert(!SAT || PROV, "SAT: the always-add scheme");
    const double T = medium_t<ORTHO>(sc64, ix, iy, iz);
    const float ef = rintf(SAT ? q - fa.sat_one_p_guard : q);
    const double e = (double)ef;
    // T >= (e + g_m)^2  <=>  D = T - e^2 >= 2 e g_m + g_m^2 =: band (D is exact: e^2 is an integer below 2^24 and T
    // - e^2 fits the significand); T < (e - g_m)^2 is implied by D < -band (stricter by 2 g_m^2: a few more level-3 pairs)
    const double D = fma(-e, e, T), band = fma(e, fa.guard64_2, fa.guard64_sq);
    const int ei = (int)ef;
    int b = -1;
    if (D >= band) b = ei;
    else if (D < -band && ei > 0) b = ei - 1;
    if (PROV) {
        const int cand = SAT ? (int)(sat_offset(q) >> 2) - 1 : (int)q;     // (a flagged candidate sits within the guard of an integer, so it
                                                                           //  is not the clamp value: !SAT (int)q is its word; SAT: the word may be a
                                                                           //  trash word -- an out-of-range q~ below the lane's C near an integer, as
                                                                           //  !SAT between nbins + 1/2 and clampv -- inside the allocation either way)
        if (b == cand) return;                         // the provisional count was right
        atomicAdd(&hist[cand], 0xffffffffu);           // (u32 counters wrap; the sum is what is flushed)
    }
    if (b >= 0) {
        if (b < fa.a.nbins) atomicAdd(&hist[b], 1u);
        return;
    }
    if constexpr (LATE) {
        static_assert(ZF, "LATE: the partner's atom index comes from the quantised frame");
        // (in three stages, each behind its own empty statement: the arguments of one stage have left their scalar registers before
        //  those of the next arrive, and the refinement bodies need few registers beyond what the quad loops hold)
        rdf_kernarg_t ka = (rdf_kernarg_t)__builtin_amdgcn_kernarg_segment_ptr();     // (the kernel's only argument: offset 0)
        asm volatile("" : "+s"(ka));
        uint32_t idx_j = ka->Q[(size_t)late->fl * (size_t)ka->a.N + (size_t)late->j_start + (size_t)j].idx;
        asm volatile("" : "+s"(ka), "+v"(idx_j));
        const double *pl = ka->a.pos + (size_t)(ka->f_base + late->fl) * (size_t)ka->a.N * 3;
        const double *pi = pl + (size_t)idx_i * 3, *pj = pl + (size_t)idx_j * 3;
        double ex = pj[0] - pi[0], ey = pj[1] - pi[1], ez = pj[2] - pi[2];
        asm volatile("" : "+s"(ka), "+v"(ex), "+v"(ey), "+v"(ez));
        const int gi = ka->a.n_cells == 1 ? 0 : ka->f_base + late->fl;
        double dx, dy, dz;
        pair_base<ORTHO>(ka->a.geom + (size_t)gi * GEOM_STRIDE, ex, ey, ez, dx, dy, dz);
        double d2 = norm2(dx, dy, dz);
        asm volatile("" : "+s"(ka), "+v"(d2));
        rdf_count(hist, d2, ka->a.rmax2, ka->a.dr, ka->a.nbins);
        return;
    }
    const uint32_t idx_j = ZF ? qseg[j].idx : qj.w;
    const double *pi = p + (size_t)idx_i * 3, *pj = p + (size_t)idx_j * 3;
    double dx, dy, dz;
    pair_base<ORTHO>(g, pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2], dx, dy, dz);
    rdf_count(hist, norm2(dx, dy, dz), fa.a.rmax2, fa.a.dr, fa.a.nbins);
}

// Canonical evaluation of a whole pair -- the base image and every listed further image, exactly as the exact
// kernels (and the oracle) do it.  Used by the IMG variant for the pairs that lie within reach of a cell face.
template <bool ORTHO>
__device__ __forceinline__ void rdf_pair_images(unsigned *hist, const RdfFastArgs &fa, const double *__restrict__ g,
                                                const double *__restrict__ p, uint32_t idx_i, uint32_t idx_j, int gi)
{
    const double *pi = p + (size_t)idx_i * 3, *pj = p + (size_t)idx_j * 3;
    double dx, dy, dz;
    pair_base<ORTHO>(g, pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2], dx, dy, dz);
    rdf_count(hist, norm2(dx, dy, dz), fa.a.rmax2, fa.a.dr, fa.a.nbins);
    const int ne = fa.a.max_img > 0 ? fa.a.nimg[gi] : 0;
    const double *__restrict__ E = fa.a.img + (size_t)gi * fa.a.max_img * 3;
    for (int m = 0; m < ne; m++)
        rdf_count(hist, norm2(dx + E[3 * m], dy + E[3 * m + 1], dz + E[3 * m + 2]), fa.a.rmax2, fa.a.dr, fa.a.nbins);
}

// One pair on the fast path.  With g = guard_f: a candidate whose fractional
// part is > g away from both bin edges is certainly in bin (int)q -- and if
// that bin is >= nbins the pair is certainly out of range; everything else
// below nbins + g is refined.  Returns true when the pair needs refinement.
// IMG: the cutoff reaches beyond half a cell height (or too close to it): pairs whose fractional difference lies
// within reach of a cell face (|i_k| > near_t[k]) can have a second image in range or an ambiguous base image --
// they are not touched here (near = true) and are evaluated canonically, images included; for every other pair the
// base image is unambiguous and the only one that can be in range.
// IMG variant: does the pair lie within reach of a cell face, |i_k| > near_t[k] on some axis?  Decided on the f32
// conversions with thresholds near_f[k] just below float(near_t[k]) (rounded down, then one ulp less): a pair beyond the
// integer threshold is always flagged, a few just below it may be too -- they take the canonical route, which is exact.
__device__ __forceinline__ bool near_pair(const float *near_f, int ix, int iy, int iz)
{
    return (fabsf((float)ix) > near_f[0]) | (fabsf((float)iy) > near_f[1]) | (fabsf((float)iz) > near_f[2]);
}

// The always-add scheme's clamp (see fast_bin<AA>): out-of-range and dead candidates go to the trash words -- and, for
// bin_count's conversion, candidates below a quarter of a bin are raised to 1/4 (such a pair is in bin 0 whatever a
// refinement would say: its true q is < 1/4 + guard).  One v_med3_f32 where a v_min_f32 stood.
__device__ __forceinline__ float clamp_candidate(float q, float clampv)
{
    return __builtin_amdgcn_fmed3f(q, 0.25f, clampv);
}

// hist[floor(q)] += 1 for a clamped candidate, 1/4 <= q < 2^20, without the half-rate conversion: 4 q - 1/2 + 2^23 (one fma,
// one rounding; the sum lies in [2^23, 2^24), where floats are the integers) rounds to floor(4 q) -- a tie exists only where
// 4 q is an integer, and goes to the even neighbour: 4 q itself or 4 q - 1, which lie above the same multiple of four unless q
// is an integer, and there the even neighbour IS 4 q -- so the low bits of the sum are floor(4 q) and (bits & 0x7ffffc) is
// the counter's byte offset 4 floor(q).  v_fmaak_f32 + v_and_b32 (2.2 issue cycles each) instead of v_cvt_i32_f32 +
// v_lshl_add_u32 (4.1 each): the headline launch 72.0 -> 69.9 ms with the base still added, the first move of this kernel since round 2
// (profiles/r05/tile_bin_address.txt; round 3 had tried 4 q through the conversion and an integer mask: slower).
typedef __attribute__((address_space(3))) unsigned lds_u32;
__device__ __forceinline__ void bin_count(unsigned *hist, float q)
{
    // (the histogram is the first thing in the kernel's dynamic LDS and the kernel has no static LDS: its byte offset IS its
    //  LDS address -- checked on the host before every launch, allow_max_lds_from_zero -- so no base is added)
    (void)hist;
    const unsigned off = __float_as_uint(fmaf(q, 4.0f, 8388607.5f)) & 0x007ffffcu;
    lds_u32 *p = (lds_u32 *)(uintptr_t)off;
    __hip_atomic_fetch_add(p, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// SAT (the planned f32-slab slice; rdf_sat_math.h): qj.w holds dz' = (z_j - z_i) / C already, half_m_guard carries 2 g and nb_hi
// 1 + g; q comes back as q' = q~ + g + 1.  No v_med3_f32 and no v_add_f32: 16 instructions per pair instead of 17
// (profiles/r15/tile_sat.txt).  A masked slot takes the saturated value 1 behind the clamp -- what +inf in front of it gives.
// (The two words travel in the parameters the clamped tail uses for 1/2 - g and nbins + g, which SAT has no use for, and are
//  named below; clampv is not read.)  Flagged here, harmlessly, are also: a coincident pair (Q = 0: fract(q') = g; the clamped
// tail raises it to 1/4 and leaves it in bin 0, where the refinement puts it too) and an out-of-range candidate below the
// lane's C that sits near an integer (its provisional count is in a trash word; the refinement takes it back and adds nothing).
template <bool ORTHO, bool IMG = false, bool ZF = false, bool AA = false, bool SAT = false>
__device__ __forceinline__ bool fast_bin(unsigned *hist, const float *sc, bool live, float half_m_guard,
                                         float nb_hi, uint32_t uix, uint32_t uiy, uint32_t uiz, uint4 qj,
                                         float &q, const float *near_f = nullptr, bool *near = nullptr,
                                         float zif = 0.0f, float clampv = 0.0f, bool live_all = false, const SatLane *sat = nullptr)
{
    static_assert(!SAT || (ZF && AA && !IMG), "SAT: the always-add tail on f32 slab coordinates");
    const int ix = (int)(qj.x - uix), iy = (int)(qj.y - uiy), iz = (int)(qj.z - uiz);
    if constexpr (SAT) {
        float t = sat_t(ix, iy, __uint_as_float(qj.w), sat->c3, sat->c4);
        if (!live_all) t = live ? t : 1.0f;
        const float two_guard = half_m_guard, one_p_guard = nb_hi;
        q = sat_candidate(__builtin_amdgcn_sqrtf(t), sat->C, one_p_guard);
        const bool unsafe = sat_unsafe(q, two_guard);
        bin_count(hist, q);
        return unsafe;
    }
    if (IMG) {
        // on the converted differences the candidate needs anyway: one compare per axis (thresholds rounded down, see
        // the kernel; axes that are clear of their half height carry +inf)
        const bool nr = near_pair(near_f, ix, iy, iz);
        *near = live && nr;
        live = live && !nr;
    }
    q = ZF ? fast_q_zf(sc, ix, iy, __uint_as_float(qj.w) - zif) : fast_q<ORTHO>(sc, ix, iy, iz);
    if (AA) {
        // Always add, fix up later (tile kernel): one LDS atomic costs the CU's LDS pipe the same whatever the number
        // of active lanes (profiles/r02/ubench_lds_atomic.txt), so nothing is gained by masking -- and the masks (two
        // compares, five scalar instructions and a skip branch per pair) were what the loop waited for.  Every lane
        // adds to the candidate bin of min(q, clampv): clampv = nbins + 1/2 + (lane mod 32) sends out-of-range (and
        // dead: q = inf) pairs to 32 trash words behind the histogram with a "safe" fractional part, so that `unsafe`
        // is "within the guard of a bin edge, and in range or between nbins + 1/2 and the lane's clampv" (the latter: a
        // count in a trash word, taken back for nothing); such a pair has been counted provisionally and
        // rdf_pair_refine<PROV> takes that count back before it adds the exact one.
        if (!live_all) q = live ? q : __builtin_inff();
        q = clamp_candidate(q, clampv);
        const bool unsafe = !(fabsf(__builtin_amdgcn_fractf(q) - 0.5f) < half_m_guard);
        bin_count(hist, q);
        return unsafe;
    }
    const bool in = live && (q < nb_hi);
    const bool safe = fabsf(__builtin_amdgcn_fractf(q) - 0.5f) < half_m_guard;
    if (in && safe) atomicAdd(&hist[(int)q], 1u);
    return in && !safe;
}

// a lane's two-deep queue of pairs that wait for their refinement (PARK; see fast_quad)
struct LaneQueue {
    unsigned pk0, pk1;      // (partner index in tile J) << 1 | (centre b?); QUEUE_EMPTY: free
    float pq0, pq1;         // the pair's clamped f32 candidate
};
constexpr unsigned QUEUE_EMPTY = 0xffffffffu;

// SLIM (with PARK): the pairs that find their lane's queue full share ONE refinement body, reached by a loop over the eight
// pair slots with the partner's record from LDS again, instead of eight inlined ones per quad loop -- the culled ZF kernel
// 10 423 -> 4 989 instructions, no scratch, 0.25 ms of the headline launch (profiles/r06/tile_reach.txt)
// PRE (the plan variant's quad loops, AHEAD): a quad's partner records arrive in registers (`pre`: x, y and the slab word --
// the f32 slab coordinate .w of a ZF quad, .z otherwise), read from LDS a whole quad earlier, and the record of partner u of the
// wave's next quad of the piece (LDS byte address pre_addr; the piece's last quad names itself) is read into the same registers
// behind partner u's subtractions -- no register rotation.  The compiler's own wait in front of the quad was lgkmcnt(0): the
// LDS returns in order, so the quad's reads queued behind the wave's last atomics.  Hence the reads are inline assembly, which
// the compiler does not count, and each partner waits with lgkmcnt(12): behind the read of partner u and in front of its next
// wait lie three more reads of two instructions and the six atomics of three partners, held there by the reads' "memory"
// clobbers, so at most 12 outstanding operations mean that it has arrived (more operations in between, the slow path's, only
// make the wait longer).  PRE = 2, the ragged tail quad: always the piece's last, it reads nothing and drains first.  The
// destination registers belong to the reads until pre_drain (rdf_tile_kernel_fast) at the end of the piece.
// (profiles/r09/tile_ahead.txt)
typedef uint32_t pre_u32x2 __attribute__((ext_vector_type(2)));
struct PreRec {
    pre_u32x2 xy;
    uint32_t s;
};
template <int U, bool ZF>
__device__ __forceinline__ void pre_read(PreRec &r, unsigned addr)
{
    asm volatile("ds_read_b64 %[xy], %[a] offset:%[o0]\n\tds_read_b32 %[s], %[a] offset:%[o1]"
                 : [xy] "=&v"(r.xy), [s] "=&v"(r.s)
                 : [a] "v"(addr), [o0] "n"(16 * U), [o1] "n"(16 * U + (ZF ? 12 : 8))
                 : "memory");
}
template <int N>
__device__ __forceinline__ void pre_wait(PreRec &r)
{
    // (the record is an input of the wait and passes through an empty statement behind it: whatever copy the compiler makes for a
    //  tied operand reads the registers after the wait, and no consumer is scheduled above it)
    asm volatile("s_waitcnt lgkmcnt(%[n])" : : "v"(r.xy), "v"(r.s), [n] "n"(N));
    asm volatile("" : "+v"(r.xy), "+v"(r.s));
}
// a piece's first quad: the four records and a full wait in one statement
// (the centres' records are operands although the text does not name them: the compiler waits for its own LDS reads of them
//  here, once, and not with an lgkmcnt(0) at their first use inside the quad loop)
template <bool ZF>
__device__ __forceinline__ void pre_prime(PreRec *r, unsigned addr, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t c4,
                                          uint32_t c5)
{
    asm volatile("ds_read_b64 %[xy0], %[a]\n\tds_read_b32 %[s0], %[a] offset:%[o]\n\t"
                 "ds_read_b64 %[xy1], %[a] offset:16\n\tds_read_b32 %[s1], %[a] offset:16+%[o]\n\t"
                 "ds_read_b64 %[xy2], %[a] offset:32\n\tds_read_b32 %[s2], %[a] offset:32+%[o]\n\t"
                 "ds_read_b64 %[xy3], %[a] offset:48\n\tds_read_b32 %[s3], %[a] offset:48+%[o]\n\t"
                 "s_waitcnt lgkmcnt(0)"
                 : [xy0] "=&v"(r[0].xy), [s0] "=&v"(r[0].s), [xy1] "=&v"(r[1].xy), [s1] "=&v"(r[1].s),
                   [xy2] "=&v"(r[2].xy), [s2] "=&v"(r[2].s), [xy3] "=&v"(r[3].xy), [s3] "=&v"(r[3].s)
                 : [a] "v"(addr), [o] "n"(ZF ? 12 : 8), "v"(c0), "v"(c1), "v"(c2), "v"(c3), "v"(c4), "v"(c5)
                 : "memory");
}
// every read of the piece has landed: only now are the registers anyone else's
__device__ __forceinline__ void pre_drain(PreRec *r)
{
    asm volatile("s_waitcnt lgkmcnt(0)"
                 :
                 : "v"(r[0].xy), "v"(r[0].s), "v"(r[1].xy), "v"(r[1].s), "v"(r[2].xy), "v"(r[2].s), "v"(r[3].xy), "v"(r[3].s)
                 : "memory");
    asm volatile("" : "+v"(r[0].xy), "+v"(r[0].s), "+v"(r[1].xy), "+v"(r[1].s), "+v"(r[2].xy), "+v"(r[2].s), "+v"(r[3].xy), "+v"(r[3].s));
}
// SAT (rdf_sat_math.h): zaf, zbf arrive as -z / C (sat_centre), and the slab word of a difference record is dz'
template <bool ORTHO, bool DIAG, bool TAIL, bool IMG = false, bool ZF = false, bool ZFK = false, bool AA = false, bool PARK = false,
          bool SLIM = false, int PRE = 0, bool LATE = false, bool SAT = false>
__device__ __forceinline__ void fast_quad(unsigned *hist, const RdfFastArgs &fa, const double *sc64,
                                          const double *__restrict__ g, const float *sc, const uint4 *tq,
                                          int j0, int cntj, bool has_a, bool has_b, int ia, int ib,
                                          float half_m_guard, float nb_hi, uint32_t uax, uint32_t uay,
                                          uint32_t uaz, uint32_t ida, uint32_t ubx, uint32_t uby, uint32_t ubz,
                                          uint32_t idb, const double *__restrict__ p,
                                          const float *near_f = nullptr, int gi = 0, uint2 *nq = nullptr,
                                          unsigned *nq_count = nullptr, unsigned nq_cap = 0,
                                          float zaf = 0.0f, float zbf = 0.0f, const QAtom *__restrict__ qseg = nullptr,
                                          float clampv = 0.0f, LaneQueue *lq = nullptr, PreRec *pre = nullptr, unsigned pre_addr = 0u,
                                          const LateRefs *late = nullptr, const SatLane *sat = nullptr)
{
    static_assert(!SAT || (ZF && SLIM && PARK && LATE), "SAT: the planned f32-slab slice");
    // ZF: this step uses the f32 slab coordinates; ZFK: the kernel is a ZF kernel (the .w of the LDS copies may have
    // been overwritten by an earlier step of the frame: atom indices always come from the quantised frame)
    // four partner atoms per trip, read by broadcast before any LDS atomic
    static_assert(PRE == 0 || (SLIM && PARK && !IMG), "PRE: the slow path reads the partner's record from LDS again");
    static_assert(!LATE || (SLIM && PARK), "LATE: one refinement body, rdf_pair_refine<LATE>");
    uint4 qj[4];
    if constexpr (PRE == 0) {
#pragma unroll
        for (int u = 0; u < 4; u++) qj[u] = tq[j0 + u];
    }
    if constexpr (PRE == 2) pre_drain(pre);
    float qa[4], qb[4];
    bool na[4], nb[4];   // per-pair "needs refinement" flags (kept as lane masks)
    bool anynear = false;   // IMG: some pair of this quad lies within reach of a cell face (one mask only: SGPRs are scarce)
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int j = j0 + u;
        const bool la = has_a && (!TAIL || j < cntj) && (!DIAG || j > ia);
        const bool lb = has_b && (!TAIL || j < cntj) && (!DIAG || j > ib);
        bool ma = false, mb = false;
        if constexpr (PRE != 0) {
            // (fast_bin subtracts zeros from the differences: folded away)
            uint4 da, db;
            auto diffs = [&](auto uc) {
                constexpr int U = decltype(uc)::value;
                if constexpr (PRE == 1) pre_wait<12>(pre[U]);
                const uint32_t qx = pre[U].xy.x, qy = pre[U].xy.y, qs = pre[U].s;
                if constexpr (SAT) {
                    da = make_uint4(qx - uax, qy - uay, 0u, __float_as_uint(sat_dz(__uint_as_float(qs), sat->invC, zaf)));
                    db = make_uint4(qx - ubx, qy - uby, 0u, __float_as_uint(sat_dz(__uint_as_float(qs), sat->invC, zbf)));
                } else {
                da = make_uint4(qx - uax, qy - uay, ZF ? 0u : qs - uaz, ZF ? __float_as_uint(__uint_as_float(qs) - zaf) : 0u);
                db = make_uint4(qx - ubx, qy - uby, ZF ? 0u : qs - ubz, ZF ? __float_as_uint(__uint_as_float(qs) - zbf) : 0u);
                }
                if constexpr (PRE == 1) {
                    // (the differences exist before the read overwrites the record: volatile statements keep their order)
                    if constexpr (ZF) asm volatile("" : "+v"(da.x), "+v"(da.y), "+v"(da.w), "+v"(db.x), "+v"(db.y), "+v"(db.w));
                    else asm volatile("" : "+v"(da.x), "+v"(da.y), "+v"(da.z), "+v"(db.x), "+v"(db.y), "+v"(db.z));
                    pre_read<U, ZF>(pre[U], pre_addr);
                }
            };
            if (u == 0) diffs(std::integral_constant<int, 0>{});
            else if (u == 1) diffs(std::integral_constant<int, 1>{});
            else if (u == 2) diffs(std::integral_constant<int, 2>{});
            else diffs(std::integral_constant<int, 3>{});
            na[u] = fast_bin<ORTHO, IMG, ZF, AA, SAT>(hist, sc, la, half_m_guard, nb_hi, 0u, 0u, 0u, da, qa[u], near_f, &ma, 0.0f,
                                                      clampv, ZF && !DIAG && !TAIL, sat);
            nb[u] = fast_bin<ORTHO, IMG, ZF, AA, SAT>(hist, sc, lb, half_m_guard, nb_hi, 0u, 0u, 0u, db, qb[u], near_f, &mb, 0.0f,
                                                      clampv, ZF && !DIAG && !TAIL, sat);
            continue;
        }
        if constexpr (SAT) {
            // (the records come from LDS here, AMOF_RDF_NOAHEAD=1: the slab word is made as the read-ahead form makes it)
            uint4 ra = qj[u], rb = qj[u];
            ra.w = __float_as_uint(sat_dz(__uint_as_float(qj[u].w), sat->invC, zaf));
            rb.w = __float_as_uint(sat_dz(__uint_as_float(qj[u].w), sat->invC, zbf));
            na[u] = fast_bin<ORTHO, IMG, ZF, AA, SAT>(hist, sc, la, half_m_guard, nb_hi, uax, uay, uaz, ra, qa[u], near_f, &ma, 0.0f,
                                                      clampv, ZF && !DIAG && !TAIL, sat);
            nb[u] = fast_bin<ORTHO, IMG, ZF, AA, SAT>(hist, sc, lb, half_m_guard, nb_hi, ubx, uby, ubz, rb, qb[u], near_f, &mb, 0.0f,
                                                      clampv, ZF && !DIAG && !TAIL, sat);
            continue;
        }
        // (ZF: centres that do not exist carry an infinite slab coordinate, so only DIAG / TAIL need a live mask)
        na[u] = fast_bin<ORTHO, IMG, ZF, AA>(hist, sc, la, half_m_guard, nb_hi, uax, uay, uaz, qj[u], qa[u], near_f, &ma, zaf,
                                             clampv, ZF && !DIAG && !TAIL);
        nb[u] = fast_bin<ORTHO, IMG, ZF, AA>(hist, sc, lb, half_m_guard, nb_hi, ubx, uby, ubz, qj[u], qb[u], near_f, &mb, zbf,
                                             clampv, ZF && !DIAG && !TAIL);
        anynear |= ma | mb;
    }
    if (na[0] | na[1] | na[2] | na[3] | nb[0] | nb[1] | nb[2] | nb[3]) {   // a few % of the pairs
        if (PARK) {
            // PARK: a flagged pair waits in its lane's two-deep register queue for the end of the step, where ONE body per
            // queue level serves every lane that has an entry (half the lanes at the first level) -- instead of one body per
            // pair slot of every quad that has a flagged lane (~0.5 bodies of ~100 issue cycles per quad, each for one or two
            // live lanes).  A lane whose queue is full keeps the old way for that pair (ovf).
            unsigned ovf = 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (na[u]) {
                    if (lq->pk1 != QUEUE_EMPTY) ovf |= 1u << (2 * u);
                    else { lq->pk1 = lq->pk0; lq->pq1 = lq->pq0; lq->pk0 = (unsigned)(j0 + u) << 1; lq->pq0 = qa[u]; }
                }
                if (nb[u]) {
                    if (lq->pk1 != QUEUE_EMPTY) ovf |= 2u << (2 * u);
                    else { lq->pk1 = lq->pk0; lq->pq1 = lq->pq0; lq->pk0 = ((unsigned)(j0 + u) << 1) | 1u; lq->pq0 = qb[u]; }
                }
            }
            if (SLIM) {
                if (ovf) {
#pragma unroll 1
                    for (int k = 0; k < 8; k++) {       // bit k of ovf: partner j0 + k / 2, centre b when k is odd
                        if (ovf & (1u << k)) {
                            const int u = k >> 1;
                            const bool cb = (k & 1) != 0;
                            const float qv = cb ? (u == 0 ? qb[0] : u == 1 ? qb[1] : u == 2 ? qb[2] : qb[3])
                                                : (u == 0 ? qa[0] : u == 1 ? qa[1] : u == 2 ? qa[2] : qa[3]);
                            rdf_pair_refine<ORTHO, ZFK, AA, LATE, SAT>(hist, fa, sc64, g, qv, cb ? ubx : uax, cb ? uby : uay, cb ? ubz : uaz,
                                                                  tq[j0 + u], p, cb ? idb : ida, qseg, j0 + u, late);
                        }
                    }
                }
            } else if (ovf) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (ovf & (1u << (2 * u))) rdf_pair_refine<ORTHO, ZFK, AA>(hist, fa, sc64, g, qa[u], uax, uay, uaz, qj[u], p, ida, qseg, j0 + u);
                    if (ovf & (2u << (2 * u))) rdf_pair_refine<ORTHO, ZFK, AA>(hist, fa, sc64, g, qb[u], ubx, uby, ubz, qj[u], p, idb, qseg, j0 + u);
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < 4; u++) {
                if (na[u]) rdf_pair_refine<ORTHO, ZFK, AA>(hist, fa, sc64, g, qa[u], uax, uay, uaz, qj[u], p, ida, qseg, j0 + u);
                if (nb[u]) rdf_pair_refine<ORTHO, ZFK, AA>(hist, fa, sc64, g, qb[u], ubx, uby, ubz, qj[u], p, idb, qseg, j0 + u);
            }
        }
    }
    if (IMG) {
        if (anynear) {   // rare: find the pairs again (cheap) and park them for the dense canonical pass of this step
#pragma unroll 1
            for (int u = 0; u < 4; u++) {
                const uint4 q = tq[j0 + u];      // (from LDS again: indexing the register copies would spill them)
                const int j = j0 + u;
                const bool la = has_a && (!TAIL || j < cntj) && (!DIAG || j > ia);
                const bool lb = has_b && (!TAIL || j < cntj) && (!DIAG || j > ib);
                auto is_near = [&](uint32_t ux, uint32_t uy, uint32_t uz) {
                    return near_pair(near_f, (int)(q.x - ux), (int)(q.y - uy), (int)(q.z - uz));
                };
                auto park = [&](uint32_t idc) {
                    const unsigned slot = atomicAdd(nq_count, 1u);
                    if (slot < nq_cap) nq[slot] = make_uint2(idc, q.w);
                    else rdf_pair_images<ORTHO>(hist, fa, g, p, idc, q.w, gi);   // queue full: evaluate in place
                };
                if (la && is_near(uax, uay, uaz)) park(ida);
                if (lb && is_near(ubx, uby, ubz)) park(idb);
            }
        }
    }
}

// --------------------------------------------------------------------------
// TRI: general (triclinic) cells in the orthogonalised lattice frame.
//
// With the cell vectors in stored order A, B, C (C the slab axis) and L the lower-triangular factor of their metric,
// an image of a pair has the components  Z = L22 fz,  Y = L11 (fy + r21 fz),  X = L00 (fx + c10 fy + r20 fz)
// (c10 = L10/L00, r20 = L20/L00, r21 = L21/L11).  quantize_kernel stores FOLDED coordinates x'' = x + kx z, y' = y + ky z
// (kx = r20 - c10 r21, ky = r21), so the wrapped u32 differences of a pair are  iy = fy + r21 fz  and
// ix = fx + r20 fz - c10 r21 fz, i.e.  Y = L11 iy,  X = L00 (ix + c10 iy)  -- one fma more than a diagonal cell -- of the
// image whose |Y| and |ix| are smallest (the slab difference is the minimum image by the culling window, or wrapped).
// The fold uses every atom's own z in [0, 1): a pair whose slab difference wraps m cells (m = -1, 0, 1) is corrected
// by m (Kx, Ky) -- per piece of the partner window on the centre's side where the slab difference comes from f32
// coordinates (ZF quads), per pair from the sign and the borrow of the slab subtraction otherwise (tri_int).
// Which pairs are decided here: an image with |d| < R has |Z|, |Y|, |X| < R.  The host admits the variant when
//   L22 >= 2R or near_z is flagged,  L11 >= 2R or near_y is flagged,  R / L00 + |c10| / 2 < 1/2
// (R = rmax with the guards): then the image above is the ONLY one that can be in range unless |Y| > L11 - R or
// |Z| > L22 - R ("near": flagged by one compare each, taken back and evaluated canonically with every listed image),
// and the x wrap -- decided on ix without the c10 iy term -- can only go wrong where both candidates are out of range.
// Levels: f32 candidate (always-add), f64 T of the same integers, canonical evaluation (parked, drained densely).
__device__ __forceinline__ void tri_int(const uint4 qj, uint32_t ux, uint32_t uy, uint32_t uz, uint32_t kx, uint32_t ky,
                                        int &ix, int &iy, int &iz)
{
    iz = (int)(qj.z - uz);
    // unwrapped slab difference = wrapped + m: m = (wrapped < 0) - (borrow)
    const uint32_t sgn = (uint32_t)(iz >> 31);           // all ones when the wrapped difference is negative
    const bool borrow = qj.z < uz;
    ix = (int)(qj.x - ux - (sgn & kx) + (borrow ? kx : 0u));
    iy = (int)(qj.y - uy - (sgn & ky) + (borrow ? ky : 0u));
}

// XW: the x wrap is decided WITH the c10 iy term (cells whose x axis has no slack, e.g. two equal in-plane lengths):
// the term joins the integer difference before it wraps (truncated product: the candidate moves by < 1 + 256 |c10| grid
// units, part of the guards; level 2 repeats the decision bit for bit and is exact for the image it picks)
template <bool XW>
__device__ __forceinline__ int tri_xwrap(float c10, int ix, float fy)
{
    return XW ? (int)((uint32_t)ix + (uint32_t)(int)(fy * c10)) : ix;
}

// squared distance of a candidate in bins^2 (f32) | its root
template <bool XW>
__device__ __forceinline__ float tri_t(const float *sc, float c10, int ix, float fy, float dz)
{
    const float dxf = XW ? (float)tri_xwrap<true>(c10, ix, fy) : fmaf(fy, c10, (float)ix);
    const float x2 = dxf * dxf, y2 = fy * fy;
    return fmaf(dz, dz, fmaf(y2, sc[4], x2 * sc[3]));
}

template <bool XW>
__device__ __forceinline__ float tri_q(const float *sc, float c10, int ix, float fy, float dz)
{
    return __builtin_amdgcn_sqrtf(tri_t<XW>(sc, c10, ix, fy, dz));
}

// near mode 4: the nearer of the pair's two candidates -- the image it minimised and the one a cell further along y, x wrapped
// again with the new y.  The host admits the mode only where the two differ by a lattice vector of length >= 2 rmax: then at
// most one of them is in range, and when the nearer one is clear of the last bin edge by the guard the other is out of range
// by the same margin (a pair inside that band is flagged and goes the canonical way with every listed image, like any pair on
// a bin edge).  One root, one clamp, one edge test, one histogram add per pair; the first version counted both candidates
// (the second into the trash words for the 85 % of pairs that have none): 2.3x the diagonal cell's cost per visited pair.
// HALF = +-1: c10 = +-1/2 exactly (hexagonal cells: two equal in-plane vectors at 120 or 60 degrees).  The y term of the x
// wrap is then iy / 2 -- an arithmetic shift and an integer add where the float product, its conversion and the add stood --
// and the twin image's x, a further half cell along, is the first candidate's with the top bit flipped (+-2^31 modulo 2^32);
// the twin's |y| is | |iy| - 2^32 |.  Exact to one grid unit (the float product: 1 + 256 |c10| units, which the guard keeps).
template <bool XW, int HALF>
__device__ __forceinline__ float tri_q_twin(const float *sc, float c10, int ix, int iy, float fy, float dz)
{
    if (HALF != 0) {
        const uint32_t h = (uint32_t)(iy >> 1);
        const uint32_t x1 = HALF > 0 ? (uint32_t)ix + h : (uint32_t)ix - h;
        const float f1 = (float)(int)x1, f2 = (float)(int)(x1 ^ 0x80000000u);
        const float y2 = fabsf(fy) - 4294967296.f;
        const float t1 = fmaf(dz, dz, fmaf(fy * fy, sc[4], (f1 * f1) * sc[3]));
        const float t2 = fmaf(dz, dz, fmaf(y2 * y2, sc[4], (f2 * f2) * sc[3]));
        return __builtin_amdgcn_sqrtf(__builtin_fminf(t1, t2));
    }
    const float t1 = tri_t<XW>(sc, c10, ix, fy, dz);
    const float t2 = tri_t<true>(sc, c10, ix, fy - copysignf(4294967296.f, fy), dz);
    return __builtin_amdgcn_sqrtf(__builtin_fminf(t1, t2));
}

struct TriConst {
    float c10, near_y, near_z, near_x;
    uint32_t kx, ky;
};

// one pair on the TRI fast path (always-add histogram, see fast_bin<AA>); returns "needs the slow path".
// ZF: (ux, uy) are the centre's folded coordinates already corrected for the piece's slab wrap, zif its f32 slab
// coordinate; else the raw folded ones (per-pair correction).  NEAR: 0 no second image possible anywhere; 1 only for pairs
// inside the guard band of the last bin edge, which are flagged anyway: the slow path tests, the fast path does not; 2 the
// fast path tests y, 3 y and z (the slow path always both: every instruction of its body costs, so NEAR = 0 has none);
// 4 for cells whose second image along y is COMMON (hexagonal: 15 % of the pairs): the fast path takes the nearer of the
// pair's two candidates (tri_q_twin), and a pair whose nearer candidate is inside the guard of a bin edge is parked for the
// canonical arithmetic (first version: the twin in the slow path, which then ran on every wave-level pair with a few live
// lanes: 4.4x the diagonal cell's cost per visited pair; second: both candidates counted, 2.3x).
template <bool ZF, int NEAR, bool XW, int HALF = 0>
__device__ __forceinline__ bool fast_bin_tri(unsigned *hist, const float *sc, const TriConst &tc, bool live, float half_m_guard,
                                             uint32_t ux, uint32_t uy, uint32_t uz, uint4 qj, float &q, float zif,
                                             float clampv, bool live_all)
{
    int ix, iy;
    float dz;
    if (ZF) {
        ix = (int)(qj.x - ux); iy = (int)(qj.y - uy);
        dz = __uint_as_float(qj.w) - zif;
    } else {
        int iz;
        tri_int(qj, ux, uy, uz, tc.kx, tc.ky, ix, iy, iz);
        dz = (float)iz * sc[8];
    }
    const float fy = (float)iy;
    static_assert(HALF == 0 || NEAR == 4, "the exact-half x wrap exists for near mode 4 only");
    q = NEAR == 4 ? tri_q_twin<XW, HALF>(sc, tc.c10, ix, iy, fy, dz) : tri_q<XW>(sc, tc.c10, ix, fy, dz);
    if (!live_all) q = live ? q : __builtin_inff();
    q = clamp_candidate(q, clampv);
    bool flag = !(fabsf(__builtin_amdgcn_fractf(q) - 0.5f) < half_m_guard);
    if (NEAR == 2) flag |= live && (fabsf(fy) > tc.near_y);
    if (NEAR == 3) flag |= live && ((fabsf(fy) > tc.near_y) | (fabsf(dz) > tc.near_z));
    bin_count(hist, q);
    return flag;
}

// slow path of a flagged TRI pair: the provisional count of candidate bin (int)q stands, moves, or is taken back and the
// pair parked for the canonical evaluation (near pairs: a second image may count; level 3: within g_m of a bin edge)
// (ZF quads: (ux, uy) carry the piece's slab wrap -- for a partner inside the window that is the pair's own; one outside it is
//  out of range by its slab distance alone, whatever the other two components come out as)
template <bool ZF, int NEAR, bool XW, typename Park>
__device__ __forceinline__ void rdf_pair_refine_tri(unsigned *hist, const RdfFastArgs &fa, const float *sc, const TriConst &tc,
                                                    const double *sc64, float q, uint32_t ux, uint32_t uy, uint32_t uz,
                                                    uint4 qj, float zif, float clampv, Park &&park)
{
    int ix, iy, iz;
    if (ZF) { ix = (int)(qj.x - ux); iy = (int)(qj.y - uy); iz = (int)(qj.z - uz); }
    else tri_int(qj, ux, uy, uz, tc.kx, tc.ky, ix, iy, iz);
    const int cand = (int)q;
    if (NEAR == 4) {
        // the nearer candidate is within the guard of a bin edge: its provisional count back, the pair goes the canonical way
        // with every listed image
        atomicAdd(&hist[cand], 0xffffffffu);
        park();
        return;
    }
    // (+inf on an axis without second image; x: only pairs inside the guard band of the last bin edge can matter)
    if (NEAR > 0 && ((fabsf((float)iy) > tc.near_y) | (fabsf((float)iz * sc[8]) > tc.near_z) |
                     (fabsf(XW ? (float)tri_xwrap<true>(tc.c10, ix, (float)iy) : fmaf((float)iy, tc.c10, (float)ix)) > tc.near_x))) {
        atomicAdd(&hist[cand], 0xffffffffu);
        park();
        return;
    }
    double fx = (double)ix;
    const double fy = (double)iy, fz = (double)iz;
    if (XW) {   // the image the fast path picked: the same f32 product decides the wrap, the shift is a whole cell
        const double it = (double)(int)((float)iy * tc.c10);
        fx += (double)tri_xwrap<true>(tc.c10, ix, (float)iy) - (fx + it);      // (-2^32, 0 or 2^32: exact)
    }
    const double dx = fma(fy, sc64[3], fx * sc64[0]), dy = fy * sc64[4], dz = fz * sc64[8];
    const double T = fma(dz, dz, fma(dy, dy, dx * dx));
    const float ef = rintf(q);
    const double e = (double)ef;
    const double D = fma(-e, e, T), band = fma(e, fa.guard64_2, fa.guard64_sq);
    const int ei = (int)ef;
    int b = -1;
    if (D >= band) b = ei;
    else if (D < -band && ei > 0) b = ei - 1;
    if (b == cand) return;
    atomicAdd(&hist[cand], 0xffffffffu);
    if (b >= 0) {
        if (b < fa.a.nbins) atomicAdd(&hist[b], 1u);
        return;
    }
    park();
}

// the atom index of partner j of the tile (wave-uniform address): a SCALAR load, so that the slow path holds no vector-memory
// operation that the compiler could make the quad loops wait for
__device__ __forceinline__ uint32_t scalar_idx(const QAtom *q)
{
    const unsigned long long a = (unsigned long long)q;
    const unsigned long long au = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(a >> 32)) << 32) |
                                  (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)a);
    uint32_t v;
    asm volatile("s_load_dword %0, %1, 0xc\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(au) : "memory");
    return v;
}

template <bool DIAG, bool TAIL, bool ZF, int NEAR, bool XW, int HALF = 0>
__device__ __forceinline__ void fast_quad_tri(unsigned *hist, const RdfFastArgs &fa, const double *sc64, const float *sc,
                                              const TriConst &tc, const uint4 *tq, int j0, int cntj, bool has_a, bool has_b,
                                              int ia, int ib, float half_m_guard,
                                              uint32_t uax, uint32_t uay, uint32_t uaz, uint32_t ida,
                                              uint32_t ubx, uint32_t uby, uint32_t ubz, uint32_t idb,
                                              uint2 *nq, unsigned *nq_count, unsigned nq_cap,
                                              const double *__restrict__ g, const double *__restrict__ p, int gi,
                                              float zaf, float zbf, const QAtom *__restrict__ qseg, float clampv)
{
    uint4 qj[4];
#pragma unroll
    for (int u = 0; u < 4; u++) qj[u] = tq[j0 + u];
    float qa[4], qb[4];
    bool na[4], nb[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int j = j0 + u;
        const bool la = has_a && (!TAIL || j < cntj) && (!DIAG || j > ia);
        const bool lb = has_b && (!TAIL || j < cntj) && (!DIAG || j > ib);
        na[u] = fast_bin_tri<ZF, NEAR, XW, HALF>(hist, sc, tc, la, half_m_guard, uax, uay, uaz, qj[u], qa[u], zaf, clampv, ZF && !DIAG && !TAIL);
        nb[u] = fast_bin_tri<ZF, NEAR, XW, HALF>(hist, sc, tc, lb, half_m_guard, ubx, uby, ubz, qj[u], qb[u], zbf, clampv, ZF && !DIAG && !TAIL);
    }
    if (na[0] | na[1] | na[2] | na[3] | nb[0] | nb[1] | nb[2] | nb[3]) {
        unsigned ovf = 0u;      // pairs of this lane that found the queue full: bit 2 u + (0: centre a, 1: centre b)
#pragma unroll
        for (int u = 0; u < 4; u++) {
            auto park = [&](uint32_t idc) {
                const uint32_t idj = scalar_idx(qseg + (j0 + u));
                const unsigned slot = atomicAdd(nq_count, 1u);
                if (slot < nq_cap) nq[slot] = make_uint2(idc, idj);
                else ovf |= 1u << (2 * u + (idc == idb ? 1 : 0));       // (evaluated below: ONE copy of the canonical body per quad loop, not eight)
            };
            // (the partner's record is read from LDS again here: four records held in registers across the eight slow-path
            //  bodies of a quad are 16 of the 96 VGPRs, and the TRI variants spilled 136 - 240 bytes per lane into these loops)
            if (na[u] | nb[u]) {
                const uint4 qr = tq[j0 + u];
                if (na[u]) rdf_pair_refine_tri<ZF, NEAR, XW>(hist, fa, sc, tc, sc64, qa[u], uax, uay, uaz, qr, zaf, clampv, [&]() { park(ida); });
                if (nb[u]) rdf_pair_refine_tri<ZF, NEAR, XW>(hist, fa, sc, tc, sc64, qb[u], ubx, uby, ubz, qr, zbf, clampv, [&]() { park(idb); });
            }
        }
        if (ovf) {      // queue full (perfect lattices: every pair on a bin edge): in place
#pragma unroll 1
            for (int k = 0; k < 8; k++)
                if ((ovf >> k) & 1u) rdf_pair_images<false>(hist, fa, g, p, (k & 1) ? idb : ida, scalar_idx(qseg + (j0 + (k >> 1))), gi);
        }
    }
}

// Work item = (tile I, 128-atom sub-tile of I, tile J) x a chunk of frames.  All four
// waves of the workgroup hold the SAME 128 centre atoms (two adjacent ones per lane) and
// share the quads of tile J round-robin, so the slab culling -- which depends only on the
// centre atoms' slab range -- removes the same share of work from every wave.
static_assert(QSLABS == TILE_PLAN_SLABS && CELL_SPECIES_SHIFT == RDF_CELL_ATOM_BITS, "tile_plan.h, rdf_select.h");

// One wave copies 64 x 16 B from per-lane global addresses to 1 KiB of LDS at `dst`
// (wave-uniform), without passing through registers (LDS-DMA, global_load_lds_dwordx4).
__device__ __forceinline__ void dma_1k(const QAtom *src_lane, uint4 *dst_wave)
{
    dma16(src_lane, dst_wave);
}

// (the body: rdf_tile_body.inc)
// KIND (PLAN only): the grid slice.  1 = this workgroup runs the steps its records flag ZF (f32 slab coordinates) and no others,
// 2 = the steps in integer form and no others; every step of the plan belongs to exactly one of the two, and integer histograms add.
// SAT: the kernel's LDS histogram has the saturating tail's layout, and slice 1 runs that tail (rdf_sat_math.h)
template <int AHEAD, int KIND, bool SAT>
__device__ __forceinline__ void rdf_tile_slice(const RdfFastArgs &fa)
{
    constexpr bool ORTHO = true, CULL = true, IMG = false, ZFK = true, PLAN = true;
    constexpr int TRI = -1;
#include "rdf_tile_body.inc"
}

// The kernel.  (five workgroups per CU, 96 VGPRs.  The TRI variants once spilled 136 - 240 bytes per lane at that budget -- 7x the vector-
//  memory instructions of the diagonal kernel -- and the ones with near tests in the fast path ran better at four workgroups
//  and 128 VGPRs; since their slow path reads the partner's record from LDS again and the canonical fallback of a full queue
//  exists once per quad loop instead of eight times, all of them fit: profiles/r04/tri_experiments.txt)
// (PLAN: six -- its centres go from global memory straight to registers, and without the centre buffers six workgroups'
//  LDS fits a CU at the headline's histogram: tile_lds, profiles/r13/tile_six.txt)
// PLAN: a grid of two z slices over the same work items.  Slice 0 runs the steps in integer form (on the headline the Zn-Zn
// tile pairs: 2 % of the pairs), slice 1 the steps on f32 slab coordinates; each is the body without the other's quad loops,
// refinement copies and scalar state, and a work item without a step of the slice's form returns after one ballot.  Slice 0
// is dispatched first: its few long work items run beside the others from the start.  As a launch of their own behind the
// others they took 2.5 ms of an otherwise idle GPU (profiles/r14/tile_step_state.txt).  Which form a step takes depends
// on the frame's slab table, so both slices always cover the whole grid.
template <bool ORTHO, bool CULL, bool IMG = false, bool ZFK = false, int TRI = -1, bool PLAN = false, int AHEAD = 0, bool SAT = false>
__global__ __launch_bounds__(FAST_THREADS, PLAN ? 6 : 5) void rdf_tile_kernel_fast(RdfFastArgs fa)
{
    if constexpr (PLAN) {
        static_assert(ORTHO && CULL && !IMG && ZFK && TRI < 0, "PLAN: the slab-culled diagonal-cell kernel on f32 slab coordinates");
        if (blockIdx.z == 0) rdf_tile_slice<AHEAD, 2, SAT>(fa);
        else rdf_tile_slice<AHEAD, 1, SAT>(fa);
    } else {
        static_assert(!SAT, "SAT: the plan variant");
        constexpr int KIND = 0;
#include "rdf_tile_body.inc"
    }
}

// Plan of the tile kernel's steps (PLAN), once per frame batch behind the quantiser: one workgroup per frame, the frame's
// slab table [S][257] in LDS.  First the slab range of every centre sub-tile (its first and last atom, by search in the
// table), then one thread per tile pair: the records of its (up to four) steps, plan[(pair nf + frame) 4 + sub] -- a work
// item of the tile kernel reads the records of its chunk as one contiguous run.
struct TilePlanArgs {
    const uint32_t *slab_start;     // [nf][S][257]
    const Tile *tiles;
    const int2 *pairs;
    const int64_t *sp_first;        // [S + 1]
    const FrameScale *fs;           // [n_cells]
    uint4 *plan;                    // [npairs][nf][4]
    int32_t S, ntiles, npairs, nf, f_base, n_cells;
};

constexpr int PLAN_THREADS = 256;

__global__ __launch_bounds__(PLAN_THREADS) void rdf_tile_plan_kernel(TilePlanArgs pa)
{
    extern __shared__ __align__(16) unsigned char plan_raw[];
    uint32_t *tab = reinterpret_cast<uint32_t *>(plan_raw);                  // [S][257]
    uint32_t *cslab = tab + (size_t)pa.S * (QSLABS + 1);                     // [ntiles][4]: s_first | s_last << 8
    const int fl = blockIdx.x, tid = threadIdx.x;
    const uint32_t *__restrict__ src = pa.slab_start + (size_t)fl * pa.S * (QSLABS + 1);
    for (int i = tid; i < pa.S * (QSLABS + 1); i += PLAN_THREADS) tab[i] = src[i];
    __syncthreads();
    for (int i = tid; i < pa.ntiles * TILE_PLAN_MAX_SUBS; i += PLAN_THREADS) {
        const Tile t = pa.tiles[i / TILE_PLAN_MAX_SUBS];
        const int sub = i % TILE_PLAN_MAX_SUBS;
        uint32_t v = 0u;
        if (sub * FAST_SUB < t.count) {
            const uint32_t *st = tab + (size_t)t.species * (QSLABS + 1);
            const uint32_t k0 = (uint32_t)(t.start - pa.sp_first[t.species]) + (uint32_t)(sub * FAST_SUB);
            const uint32_t k1 = k0 + (uint32_t)min(FAST_SUB, t.count - sub * FAST_SUB) - 1u;
            v = tile_plan_slab_of(st, k0) | tile_plan_slab_of(st, k1) << 8;
        }
        cslab[i] = v;
    }
    __syncthreads();
    const uint32_t G = pa.fs[pa.n_cells == 1 ? 0 : pa.f_base + fl].cull_gap;
    for (int p = tid; p < pa.npairs; p += PLAN_THREADS) {
        const int2 pr = pa.pairs[p];
        const Tile ti = pa.tiles[pr.x], tj = pa.tiles[pr.y];
        const uint32_t *st = tab + (size_t)tj.species * (QSLABS + 1);
        const int toff = (int)(tj.start - pa.sp_first[tj.species]);
        uint4 *out = pa.plan + ((size_t)p * (size_t)pa.nf + (size_t)fl) * TILE_PLAN_MAX_SUBS;
#pragma unroll 1
        for (int sub = 0; sub < TILE_PLAN_MAX_SUBS; sub++) {
            TilePlanRecord r = {0u, 0u, 0u, 0u};
            if (sub * FAST_SUB < ti.count) {
                const uint32_t c = cslab[pr.x * TILE_PLAN_MAX_SUBS + sub];
                const uint32_t s_first = c & 255u, s_last = (c >> 8) & 255u;
                r = tile_plan_pack(tile_plan_window(st, toff, tj.count, s_first, s_last, G, pr.x == pr.y, sub), s_first, s_last);
            }
            out[sub] = make_uint4(r.x, r.y, r.z, r.w);
        }
    }
}

// --------------------------------------------------------------------------
// Range kernel: small cutoffs in big cells (rmax <= a third of the slab axis).
//
// Frames come 2-level sorted (quantize2_kernel): nz slabs (>= rmax thick) x 256 y-bins.  One
// workgroup = one 128-atom centre sub-tile x one partner species; instead of meeting fixed
// partner tiles it walks the partner ranges itself: for each slab within one slab of the
// centres, the y-bins within rmax of the centres' y range give at most two contiguous index
// ranges (table start2), streamed through LDS 512 at a time.  Same-species pairs are counted
// once with a per-lane rule that needs no look-back: partner slab == centre slab + 1 (mod nz):
// every pair; same slab: partner index > centre index; anything else is the other atom's job
// (or farther than a whole slab: out of range).  Needs nz >= 3.
struct RdfRangeArgs {
    RdfFastArgs f;
    const uint32_t *start2;   // [nf][S][nz*256 + 1]
    const int64_t *sp_first;  // [S+1]
    const int4 *work;         // (centre species a, first centre c0, partner species b, 0)
    int32_t nz;
    int32_t gy_bins;          // y reach in bins (rmax / h_y * 256, rounded up, + 1)
};

template <bool ORTHO>
__global__ __launch_bounds__(FAST_THREADS, 5) void rdf_range_kernel_fast(RdfRangeArgs ra)
{
    const RdfFastArgs &fa = ra.f;
    const RdfArgs &a = fa.a;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint4 *tq = reinterpret_cast<uint4 *>(lds_raw);                  // [FAST_TILE] partner chunk
    unsigned *hist = reinterpret_cast<unsigned *>(tq + FAST_TILE);    // [nbins]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int4 w = ra.work[blockIdx.x];
    const int sa_ = w.x, c0 = w.y, sb_ = w.z;
    const bool same = sa_ == sb_;
    const int nz = ra.nz, nkeys = nz * 256;
    const int nbins = a.nbins;
    for (int k = tid; k < nbins; k += FAST_THREADS) hist[k] = 0u;
    const int64_t segA = ra.sp_first[sa_], segB = ra.sp_first[sb_];
    const int nA = (int)(ra.sp_first[sa_ + 1] - segA);
    const int cnt_c = min(FAST_SUB, nA - c0);
    const int la = 2 * lane, lb = la + 1;
    const bool has_a = la < cnt_c, has_b = lb < cnt_c;
    const float half_m_guard = fa.half_m_guard;
    const float nb_hi = fa.nb_hi;
    const int f0 = blockIdx.y * a.frames_per_chunk;
    const int f1 = min(f0 + a.frames_per_chunk, fa.nf);

    for (int fl = f0; fl < f1; fl++) {
        const int f = fa.f_base + fl;
        const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
        const QAtom *__restrict__ Qf = fa.Q + (size_t)fl * (size_t)a.N;
        const int gi = a.n_cells == 1 ? 0 : f;
        const FrameScale *__restrict__ fs = fa.fs + gi;
        const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
        float sc[9];
#pragma unroll
        for (int k = 0; k < 9; k++) sc[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->sc[k])));
        const uint32_t *__restrict__ stB = ra.start2 + ((size_t)fl * a.S + sb_) * (size_t)(nkeys + 1);
        // this lane's two centre atoms and their slabs
        const QAtom ca = Qf[segA + c0 + min(la, cnt_c - 1)], cb = Qf[segA + c0 + min(lb, cnt_c - 1)];
        const int za = (int)__umulhi(ca.uz, (unsigned)nz), zb = (int)__umulhi(cb.uz, (unsigned)nz);
        // slab / y-bin extent of the sub-tile (it is sorted by (slab, ybin): first and last atom)
        const QAtom cf = Qf[segA + c0], cl = Qf[segA + c0 + cnt_c - 1];
        const int s_first = (int)__umulhi(cf.uz, (unsigned)nz), s_last = (int)__umulhi(cl.uz, (unsigned)nz);
        const bool one_slab = s_first == s_last;
        int ylo = 0, yhi = 255;
        bool y_full = true;
        if (one_slab) {
            const int y0 = (int)(cf.uy >> 24) - ra.gy_bins, y1 = (int)(cl.uy >> 24) + ra.gy_bins;
            if (y1 - y0 + 1 < 256) { y_full = false; ylo = y0 & 255; yhi = y1 & 255; }
        }
        // partner slabs: [s_first - 1 (different species only), s_last + 1], each at most once
        int p_begin = same ? s_first : s_first - 1;
        int p_count = s_last + 1 - p_begin + 1;
        if (p_count > nz) { p_count = nz; }
        for (int pi = 0; pi < p_count; pi++) {
            const int ps = ((p_begin + pi) % nz + nz) % nz;
            // per-lane rule for this partner slab: threshold on the partner's sorted index
            //   -1: every partner counts, INT_MAX: none, i: partners with index > i
            auto thresh = [&](int zc, int iabs) {
                const int d = ((ps - zc) % nz + nz) % nz;
                if (same) return d == 1 ? -1 : (d == 0 ? iabs : 0x7fffffff);
                return (d <= 1 || d == nz - 1) ? -1 : 0x7fffffff;
            };
            const int tha = thresh(za, c0 + la), thb = thresh(zb, c0 + lb);
            // y ranges of this slab: [ylo, yhi] circular -> one or two index ranges
            int rb[2], re[2];
            const uint32_t *row = stB + ps * 256;
            if (y_full || ylo <= yhi) {
                rb[0] = (int)row[y_full ? 0 : ylo]; re[0] = (int)row[(y_full ? 255 : yhi) + 1];
                rb[1] = re[1] = 0;
            } else {
                rb[0] = (int)row[0]; re[0] = (int)row[yhi + 1];
                rb[1] = (int)row[ylo]; re[1] = (int)row[256];
            }
            for (int r = 0; r < 2; r++) {
                for (int base = rb[r]; base < re[r]; base += FAST_TILE) {
                    const int cntj = min(FAST_TILE, re[r] - base);
                    const int cntj4 = (cntj + 3) & ~3;
                    __syncthreads();
                    for (int k = tid; k < cntj4; k += FAST_THREADS) {
                        const QAtom q = Qf[segB + base + min(k, cntj - 1)];
                        tq[k] = make_uint4(q.ux, q.uy, q.uz, q.idx);
                    }
                    __syncthreads();
                    // per-lane thresholds relative to this chunk (fast_quad's "j > ia" form)
                    const int ia = tha == -1 ? -1 : (tha == 0x7fffffff ? 0x7fffffff : tha - base);
                    const int ib = thb == -1 ? -1 : (thb == 0x7fffffff ? 0x7fffffff : thb - base);
                    for (int j0 = 4 * wave; j0 < cntj4; j0 += 16)
                        fast_quad<ORTHO, true, true>(hist, fa, fs->sc64, g, sc, tq, j0, cntj, has_a, has_b, ia, ib, half_m_guard,
                                                     nb_hi, ca.ux, ca.uy, ca.uz, ca.idx, cb.ux, cb.uy, cb.uz, cb.idx, p);
                }
            }
        }
    }
    __syncthreads();
    const int lo = min(sa_, sb_), hi = max(sa_, sb_);
    unsigned long long *U = a.U + ((size_t)lo * a.S + hi) * (size_t)nbins;
    for (int k = tid; k < nbins; k += FAST_THREADS) {
        unsigned v = hist[k];
        if (v) atomicAdd(&U[k], (unsigned long long)v);
    }
}

// --------------------------------------------------------------------------
// Cell-list kernel: cutoffs far below the cell size (rmax <= h_k / 2.5 on every axis).
//
// Frames come sorted into a 3-D grid of cells at least rmax/2 thick (launch_cell_sort), x
// fastest, species-sorted inside a cell.  One lane = one centre atom; it walks the 13 rows
// (dz, dy) of the positive half shell -- (0,0), (0,1), (0,2), (1,-2..2), (2,-2..2) -- and in
// each row the x-contiguous run of cells cx-2 .. cx+2 (row (0,0): from its own successor to
// the end of cell cx+2), i.e. at most two index ranges per row (periodic wrap in x).  Every
// unordered pair of atoms within reach is met exactly once (the grid has >= 5 cells per axis, so
// +d and -d never name the same cell).  Partners are gathered from L2 (a frame's records fit in
// it and all workgroups of a frame are dealt to one XCD); the pair arithmetic is the fast
// path's three levels; the LDS histogram holds every unordered species pair.
struct RdfCellArgs {
    RdfFastArgs f;
    const uint32_t *start3;   // [nf][nkeys + 1]
    const uint32_t *keyoff;   // [S*S] offset of the pair (sa, sb) in the LDS histogram (pair key * nbins)
    const uint32_t *keyU;     // [npk] offset of pair key k in U ((lo * S + hi) * nbins)
    int32_t nx, ny, nz, npk;
    int32_t frames_grid;      // frame slots of the launch (rounded up to a multiple of 8 with the XCD mapping)
    int32_t fpc;              // frames per workgroup (round 4): the same block of atoms over fpc frames, ONE histogram flush
    int32_t cpt;              // centre atoms per thread (the workgroup covers 256 * cpt consecutive atoms)
    int32_t trim;             // 1: rows trimmed per lane to the cells within reach (AMOF_RDF_NOTRIM=1: the full 5-cell runs)
};

constexpr int CELL_THREADS = 512;
#ifndef CELL_UNROLL
#define CELL_UNROLL 4   // partners gathered per trip
#endif
constexpr uint32_t CELL_IDX_MASK = (1u << CELL_SPECIES_SHIFT) - 1u;

template <bool ORTHO>
__global__ __launch_bounds__(CELL_THREADS, 8) void rdf_cell_kernel(RdfCellArgs ca)
{
    const RdfFastArgs &fa = ca.f;
    const RdfArgs &a = fa.a;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned *hist = reinterpret_cast<unsigned *>(lds_raw);          // [npk * nbins]
    unsigned *koff = hist + (size_t)ca.npk * a.nbins;                // [S * S]
    const int tid = threadIdx.x;
    const int S = a.S, nbins = a.nbins;
    // all workgroups of a frame on one XCD (its quantised records stay in that L2).  A workgroup keeps its block of atoms
    // for a chunk of fpc frames (the XCD's own: slot, slot + 8, ...) and flushes its histogram once: flushing per frame was
    // ~2e6 u64 global atomics a frame on configs[4], 854 MB of the kernel's writes (profiles/r03/pmc_cfg4.json)
    unsigned chunk = blockIdx.y, bx = blockIdx.x, xcd = 0, fstep = 1;
    if (fa.xcd_map) {
        const unsigned long long lin = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;
        const unsigned long long kk = lin >> 3;
        xcd = (unsigned)(lin & 7ull);
        chunk = (unsigned)(kk / gridDim.x);
        bx = (unsigned)(kk % gridDim.x);
        fstep = 8;
    }
    if ((int)(chunk * (unsigned)ca.fpc * fstep + xcd) >= fa.nf) return;
    for (int k = tid; k < ca.npk * nbins; k += CELL_THREADS) hist[k] = 0u;
    for (int k = tid; k < S * S; k += CELL_THREADS) koff[k] = ca.keyoff[k];
    __syncthreads();
    const int N = (int)a.N;
    const int nx = ca.nx, ny = ca.ny, nz = ca.nz;
    const float half_m_guard = fa.half_m_guard, nb_hi = fa.nb_hi;

    for (int ff = 0; ff < ca.fpc; ff++) {
    const unsigned fl = (chunk * (unsigned)ca.fpc + (unsigned)ff) * fstep + xcd;
    if ((int)fl >= fa.nf) break;
    const int f = fa.f_base + (int)fl;
    const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
    const QAtom *__restrict__ Qf = fa.Q + (size_t)fl * (size_t)a.N;
    const int gi = a.n_cells == 1 ? 0 : f;
    const FrameScale *__restrict__ fs = fa.fs + gi;
    const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
    float sc[9];
#pragma unroll
    for (int k = 0; k < 9; k++) sc[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->sc[k])));
    const uint32_t *__restrict__ st = ca.start3 + (size_t)fl * ((size_t)nx * ny * nz * S + 1);

    for (int c = 0; c < ca.cpt; c++) {
        const int i = ((int)bx * ca.cpt + c) * CELL_THREADS + tid;
        const bool active = i < N;
        const QAtom own = Qf[active ? i : N - 1];
        const unsigned *krow = koff + (own.idx >> CELL_SPECIES_SHIFT) * S;
        const uint32_t ida = own.idx & CELL_IDX_MASK;
        const int cx = (int)__umulhi(own.ux, (unsigned)nx), cy = (int)__umulhi(own.uy, (unsigned)ny),
                  cz = (int)__umulhi(own.uz, (unsigned)nz);
        // Per-lane trimming of the rows (round 3).  The f32 scales are the lower-triangular factor of the cell's metric, so
        // the Cartesian z of a difference depends on its fractional z only and y on (y, z): from the atom's own place
        // inside its cell, the least |z| and |y| any partner of row (dz, dy) can have leave rho^2 = R^2 - z^2 - y^2 for x,
        // and only the cells of the row within that reach are walked (none if rho^2 < 0).  Bounds are conservative
        // (cell edges widened by 1e-5 of a cell + 1024 units, R by 1e-4 + 2 bins): no pair within rmax is skipped; the
        // visited volume drops from the 5 x 5 x 2.5 cells block to a shell about one cell thick around the half sphere.
        const float uxf = (float)own.ux, uyf = (float)own.uy, uzf = (float)own.uz;
        const float wx = 4294967296.f / (float)nx, wy = 4294967296.f / (float)ny, wz = 4294967296.f / (float)nz;
        const float ex = wx * 1e-5f + 1024.f, ey = wy * 1e-5f + 1024.f, ez = wz * 1e-5f + 1024.f;
        const float Rq = nb_hi * 1.0001f + 2.f;
        // (a diagonal cell's scales carry the signs of its entries; the bounds below take lengths: the metric's factor has
        //  a positive diagonal, a diagonal cell |entry|)
        const float s_xx = ORTHO ? fabsf(sc[0]) : sc[0], s_yx = ORTHO ? 0.f : sc[3], s_yy = ORTHO ? fabsf(sc[1]) : sc[4],
                    s_zx = ORTHO ? 0.f : sc[6], s_zy = ORTHO ? 0.f : sc[7], s_zz = ORTHO ? fabsf(sc[2]) : sc[8];
#pragma unroll 1
        for (int row = 0; row < 13; row++) {
            // rows of the positive half shell
            const int dz = row < 3 ? 0 : (row < 8 ? 1 : 2);
            const int dy = row < 3 ? row : (row < 8 ? row - 5 : row - 10);
            int cz2 = cz + dz, cy2 = cy + dy;
            if (cz2 >= nz) cz2 -= nz;
            if (cy2 >= ny) cy2 -= ny;
            if (cy2 < 0) cy2 += ny;
            const int rowbase = (cz2 * ny + cy2) * nx;
            int xlo = row == 0 ? cx : cx - 2, xhi = cx + 2;
            if (ca.trim) {
                const float zl = (float)(cz + dz) * wz - uzf - ez, zh = zl + wz + 2.f * ez;     // fractional z of the row's partners - mine
                const float yl = (float)(cy + dy) * wy - uyf - ey, yh = yl + wy + 2.f * ey;
                const float dzmin = (zl > 0.f ? zl : (zh < 0.f ? -zh : 0.f)) * s_zz;
                const float yc_lo = yl * s_yy + fminf(zl * s_zy, zh * s_zy), yc_hi = yh * s_yy + fmaxf(zl * s_zy, zh * s_zy);
                const float dymin = yc_lo > 0.f ? yc_lo : (yc_hi < 0.f ? -yc_hi : 0.f);
                const float rem = Rq * Rq - dzmin * dzmin - dymin * dymin;
                if (rem < 0.f) {
                    xhi = xlo - 1;      // nothing of this row is within reach of this atom
                } else {
                    const float rho = __builtin_amdgcn_sqrtf(rem) * 1.0001f + 1.f;
                    const float e_lo = fminf(yl * s_yx, yh * s_yx) + fminf(zl * s_zx, zh * s_zx);
                    const float e_hi = fmaxf(yl * s_yx, yh * s_yx) + fmaxf(zl * s_zx, zh * s_zx);
                    const float fx_lo = (-rho - e_hi) / s_xx, fx_hi = (rho - e_lo) / s_xx;
                    const float inv_wx = (float)nx * (1.f / 4294967296.f);
                    xlo = max(xlo, (int)floorf((uxf + fx_lo - ex) * inv_wx - 1e-3f));
                    xhi = min(xhi, (int)floorf((uxf + fx_hi + ex) * inv_wx + 1e-3f));
                }
            }
            // cells [xlo, xhi] with periodic wrap: at most two runs
            int xa0, xb0, xa1 = 0, xb1 = -1;
            if (xhi < 0) { xa0 = xlo + nx; xb0 = xhi + nx; }                  // (trimmed runs may lie wholly beyond an edge)
            else if (xlo >= nx) { xa0 = xlo - nx; xb0 = xhi - nx; }
            else if (xlo < 0) { xa0 = xlo + nx; xb0 = nx - 1; xa1 = 0; xb1 = xhi; }
            else if (xhi >= nx) { xa0 = xlo; xb0 = nx - 1; xa1 = 0; xb1 = xhi - nx; }
            else { xa0 = xlo; xb0 = xhi; }
            // both runs are looked up before either is walked (dependent global loads)
            int ja0 = 0, ja1 = 0, jb0 = 0, jb1 = 0;
            if (active && xlo <= xhi) {
                ja0 = (int)st[(size_t)(rowbase + xa0) * S];
                ja1 = (int)st[(size_t)(rowbase + xb0 + 1) * S];
                if (row == 0) ja0 = i + 1;                    // own cell: the partners after me
                if (xa1 <= xb1) {
                    jb0 = (int)st[(size_t)(rowbase + xa1) * S];
                    jb1 = (int)st[(size_t)(rowbase + xb1 + 1) * S];
                }
            }
#pragma unroll 1
            for (int seg = 0; seg < 2; seg++) {
                const int j0 = seg == 0 ? ja0 : jb0, j1 = seg == 0 ? ja1 : jb1;
                // several partners per trip, all loaded before any is evaluated (the gathers come from L2)
                for (int j = j0; __any(j < j1); j += CELL_UNROLL) {
                    uint4 qv[CELL_UNROLL];
#pragma unroll
                    for (int u = 0; u < CELL_UNROLL; u++)
                        qv[u] = j < j1 ? *reinterpret_cast<const uint4 *>(Qf + min(j + u, j1 - 1)) : make_uint4(0, 0, 0, 0);
                    // (round 4, measured and rejected: the tile kernel's always-add histogram with trash words per row -- every
                    //  lane adds, only candidates near a bin edge branch: 0.0606 -> 0.0692 ms / frame on configs[4]; three
                    //  quarters of the gathered candidates are out of range and now pay the binning tail too)
#pragma unroll
                    for (int u = 0; u < CELL_UNROLL; u++) {
                        if (j + u < j1) {
                            const uint4 qj = qv[u];
                            const int ix = (int)(qj.x - own.ux), iy = (int)(qj.y - own.uy), iz = (int)(qj.z - own.uz);
                            const float q = fast_q<ORTHO>(sc, ix, iy, iz);
                            if (q < nb_hi) {
                                unsigned *h = hist + krow[qj.w >> CELL_SPECIES_SHIFT];
                                if (fabsf(__builtin_amdgcn_fractf(q) - 0.5f) < half_m_guard) {
                                    atomicAdd(&h[(int)q], 1u);
                                } else {
                                    rdf_pair_refine<ORTHO>(h, fa, fs->sc64, g, q, own.ux, own.uy, own.uz,
                                                           make_uint4(qj.x, qj.y, qj.z, qj.w & CELL_IDX_MASK), p, ida);
                                }
                            }
                        }
                    }
                }
            }
        }
    }
    }   // frames of the chunk
    __syncthreads();
    for (int k = tid; k < ca.npk * nbins; k += CELL_THREADS) {
        const unsigned v = hist[k];
        if (v) atomicAdd(&a.U[(size_t)ca.keyU[k / nbins] + (size_t)(k % nbins)], (unsigned long long)v);
    }
}

// --------------------------------------------------------------------------
// Cell-list kernel, one WAVE per centre cell (round 5; the default of the "rdf_cell" family).
//
// rdf_cell_kernel above gives every lane its own centre atom and lets it gather its own partners: the lanes of a wave walk
// runs of different lengths (a wave lasts as long as its longest lane, row by row), every candidate is a 16-byte gather per
// lane, and the kernel runs at ~1e12 candidates/s where the LDS-broadcast tile kernel does 3.6e12 pair evaluations/s.
// Here the roles are swapped and the centre side is made wave-uniform:
//   * a wave owns one CELL of the same grid (>= rmax / 2 thick, ~8 atoms).  The partners of ALL its atoms are the same
//     13 half-shell rows, trimmed ONCE per cell to the cells within reach of the cell (the per-lane trim of the kernel above
//     with the cell's extent in place of the atom's point): up to 26 contiguous index runs, ~650 partners;
//   * the runs are concatenated (lanes 0 .. 12 compute one row each: bounds, table look-ups; a 16-lane scan gives the run
//     offsets, kept in LDS) and the LANES take consecutive partners of the concatenation, 64 at a time, by a five-step
//     binary search over the 32 run offsets: a dense, mostly contiguous load of 64 records, every lane busy but in the
//     last chunk of a cell;
//   * the cell's centre atoms are wave-uniform: their records come through the scalar cache into SGPRs, the pair arithmetic
//     reads them as scalar operands, and the "once" rule needs one compare only in the chunks that hold the cell's own atoms
//     (partner behind the centre in the sorted order; every other row of the half shell counts whole).
// Per centre the wave evaluates the cell's ~650 partners instead of the ~525 the per-lane trim leaves, but every evaluation
// is a dense broadcast one.  Same three-level pair arithmetic, same LDS histogram of every unordered species pair, same frame
// chunks and XCD mapping as the kernel above (RdfCellArgs; cpt = cell groups of 8 cells per workgroup).
#ifndef CW_THREADS_N
#define CW_THREADS_N 512
#endif
#ifndef CW_MIN_WAVES
#define CW_MIN_WAVES 4
#endif
constexpr int CW_THREADS = CW_THREADS_N;
constexpr int CW_WAVES = CW_THREADS / 64;
constexpr int CW_RUNS = 32;          // 13 rows x 2 runs, padded to a power of two with the total
constexpr int CW_QCAP = 126;         // flagged pairs a wave parks per cell (~40 on configs[4]); beyond: refined in place
constexpr int CW_WAVE_WORDS = 2 * CW_RUNS + 2 + 2 * CW_QCAP;     // LDS words per wave behind the histograms

template <bool ORTHO>
__global__ __launch_bounds__(CW_THREADS, CW_MIN_WAVES) void rdf_cellwave_kernel(RdfCellArgs ca)
{
    const RdfFastArgs &fa = ca.f;
    const RdfArgs &a = fa.a;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned *hist = reinterpret_cast<unsigned *>(lds_raw);          // [npk * nbins]
    unsigned *koff = hist + (size_t)ca.npk * a.nbins;                // [S * S]
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.S, nbins = a.nbins;
    // (per-wave tables on an even word: the queue entries are 8-byte pairs)
    unsigned *pre = hist + (((size_t)ca.npk * a.nbins + (size_t)S * S + 1) & ~(size_t)1) + wave * CW_WAVE_WORDS;   // [CW_RUNS] first element of run k
    unsigned *rbase = pre + CW_RUNS;                                 // [CW_RUNS] sorted index of the run's first atom
    unsigned *wq_count = rbase + CW_RUNS;                            // the wave's queue of flagged pairs: entries so far
    uint2 *wq = reinterpret_cast<uint2 *>(wq_count + 2);             // [CW_QCAP] (partner, centre) by sorted index
    unsigned chunk = blockIdx.y, bx = blockIdx.x, xcd = 0, fstep = 1;
    if (fa.xcd_map) {
        const unsigned long long lin = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;
        const unsigned long long kk = lin >> 3;
        xcd = (unsigned)(lin & 7ull);
        chunk = (unsigned)(kk / gridDim.x);
        bx = (unsigned)(kk % gridDim.x);
        fstep = 8;
    }
    if ((int)(chunk * (unsigned)ca.fpc * fstep + xcd) >= fa.nf) return;
    for (int k = tid; k < ca.npk * nbins; k += CW_THREADS) hist[k] = 0u;
    for (int k = tid; k < S * S; k += CW_THREADS) koff[k] = ca.keyoff[k];
    __syncthreads();
    const int nx = ca.nx, ny = ca.ny, nz = ca.nz;
    const int ncell = nx * ny * nz;
    const float half_m_guard = fa.half_m_guard, nb_hi = fa.nb_hi;

    for (int ff = 0; ff < ca.fpc; ff++) {
        const unsigned fl = (chunk * (unsigned)ca.fpc + (unsigned)ff) * fstep + xcd;
        if ((int)fl >= fa.nf) break;
        const int f = fa.f_base + (int)fl;
        const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
        const QAtom *__restrict__ Qf = fa.Q + (size_t)fl * (size_t)a.N;
        const int gi = a.n_cells == 1 ? 0 : f;
        const FrameScale *__restrict__ fs = fa.fs + gi;
        const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
        float sc[9];
#pragma unroll
        for (int k = 0; k < 9; k++) sc[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->sc[k])));
        const uint32_t *__restrict__ st = ca.start3 + (size_t)fl * ((size_t)ncell * S + 1);
        // the row bounds relative to the centre cell depend on the row and the frame's scales only (every cell has the same
        // extent): lanes 0 .. 12 hold them for the cells of this frame
        int rel_lo = -2, rel_hi = 2;
        const int row = lane < 13 ? lane : 12;
        const int rdz = row < 3 ? 0 : (row < 8 ? 1 : 2);
        const int rdy = row < 3 ? row : (row < 8 ? row - 5 : row - 10);
        if (row == 0) rel_lo = 0;
        if (ca.trim) {
            const float wx = 4294967296.f / (float)nx, wy = 4294967296.f / (float)ny, wz = 4294967296.f / (float)nz;
            const float ex = wx * 2e-5f + 2048.f, ey = wy * 2e-5f + 2048.f, ez = wz * 2e-5f + 2048.f;
            const float Rq = nb_hi * 1.0001f + 2.f;
            // (lengths, as in rdf_cell_kernel: a diagonal cell's scales carry the signs of its entries)
            const float s_xx = ORTHO ? fabsf(sc[0]) : sc[0], s_yx = ORTHO ? 0.f : sc[3], s_yy = ORTHO ? fabsf(sc[1]) : sc[4],
                        s_zx = ORTHO ? 0.f : sc[6], s_zy = ORTHO ? 0.f : sc[7], s_zz = ORTHO ? fabsf(sc[2]) : sc[8];
            // differences partner - centre in grid units: the partner anywhere in its cell, the centre anywhere in mine
            const float zl = (float)(rdz - 1) * wz - ez, zh = (float)(rdz + 1) * wz + ez;
            const float yl = (float)(rdy - 1) * wy - ey, yh = (float)(rdy + 1) * wy + ey;
            const float dzmin = (zl > 0.f ? zl : (zh < 0.f ? -zh : 0.f)) * s_zz;
            const float yc_lo = yl * s_yy + fminf(zl * s_zy, zh * s_zy), yc_hi = yh * s_yy + fmaxf(zl * s_zy, zh * s_zy);
            const float dymin = yc_lo > 0.f ? yc_lo : (yc_hi < 0.f ? -yc_hi : 0.f);
            const float rem = Rq * Rq - dzmin * dzmin - dymin * dymin;
            if (rem < 0.f) {
                rel_hi = rel_lo - 1;        // nothing of this row is within reach of any atom of the cell
            } else {
                const float rho = __builtin_amdgcn_sqrtf(rem) * 1.0001f + 1.f;
                const float e_lo = fminf(yl * s_yx, yh * s_yx) + fminf(zl * s_zx, zh * s_zx);
                const float e_hi = fmaxf(yl * s_yx, yh * s_yx) + fmaxf(zl * s_zx, zh * s_zx);
                // partner x - (my cell's lower edge) lies in [fx_lo - ex, wx + fx_hi + ex]
                const float fx_lo = (-rho - e_hi) / s_xx, fx_hi = (rho - e_lo) / s_xx;
                const float inv_wx = (float)nx * (1.f / 4294967296.f);
                rel_lo = max(rel_lo, (int)floorf((fx_lo - ex) * inv_wx - 1e-3f));
                rel_hi = min(rel_hi, (int)floorf((wx + fx_hi + ex) * inv_wx + 1e-3f));
                if (row == 0) rel_lo = 0;
            }
        }

        for (int cc = 0; cc < ca.cpt; cc++) {
            const int cell = (int)((bx * (unsigned)ca.cpt + (unsigned)cc) * CW_WAVES) + wave;      // wave-uniform
            if (cell >= ncell) break;
            const int c_begin = __builtin_amdgcn_readfirstlane((int)st[(size_t)cell * S]);
            const int c_end = __builtin_amdgcn_readfirstlane((int)st[(size_t)(cell + 1) * S]);
            const int nown = c_end - c_begin;
            if (nown <= 0) continue;
            const int cx = cell % nx, cy = (cell / nx) % ny, cz = cell / (nx * ny);
            // ---- the cell's partner runs: one row per lane (lanes 0 .. 12) ----
            int ja0 = 0, ja1 = 0, jb0 = 0, jb1 = 0;
            if (lane < 13) {
                int cz2 = cz + rdz, cy2 = cy + rdy;
                if (cz2 >= nz) cz2 -= nz;
                if (cy2 >= ny) cy2 -= ny;
                if (cy2 < 0) cy2 += ny;
                const int rowbase = (cz2 * ny + cy2) * nx;
                const int xlo = cx + rel_lo, xhi = cx + rel_hi;
                if (xlo <= xhi) {
                    int xa0, xb0, xa1 = 0, xb1 = -1;
                    if (xhi < 0) { xa0 = xlo + nx; xb0 = xhi + nx; }
                    else if (xlo >= nx) { xa0 = xlo - nx; xb0 = xhi - nx; }
                    else if (xlo < 0) { xa0 = xlo + nx; xb0 = nx - 1; xa1 = 0; xb1 = xhi; }
                    else if (xhi >= nx) { xa0 = xlo; xb0 = nx - 1; xa1 = 0; xb1 = xhi - nx; }
                    else { xa0 = xlo; xb0 = xhi; }
                    ja0 = (int)st[(size_t)(rowbase + xa0) * S];
                    ja1 = (int)st[(size_t)(rowbase + xb0 + 1) * S];
                    if (xa1 <= xb1) {
                        jb0 = (int)st[(size_t)(rowbase + xa1) * S];
                        jb1 = (int)st[(size_t)(rowbase + xb1 + 1) * S];
                    }
                }
            }
            const int la = ja1 - ja0, lb = jb1 - jb0;
            int incl = la + lb;
#pragma unroll
            for (int off = 1; off < 16; off <<= 1) {
                const int n = __shfl_up(incl, off, 64);
                if (lane >= off) incl += n;
            }
            const int T = __builtin_amdgcn_readlane(incl, 15);         // (lanes 13 .. 15 add nothing)
            if (lane < 16) {
                const int excl = incl - la - lb;
                pre[2 * lane] = (unsigned)excl;
                pre[2 * lane + 1] = (unsigned)(excl + la);
                rbase[2 * lane] = (unsigned)ja0;
                rbase[2 * lane + 1] = (unsigned)jb0;
            }
            // (the wave reads what its own lanes wrote: LDS operations of one wave complete in order)
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // row 0's first run starts with the cell's own atoms: elements 0 .. nown - 1 of the concatenation
            auto locate = [&](int e) {          // sorted index of element e of the concatenation (e < T)
                int k = 0;
#pragma unroll
                for (int step = CW_RUNS / 2; step > 0; step >>= 1)
                    if (pre[k + step] <= (unsigned)e) k += step;
                return (int)rbase[k] + (e - (int)pre[k]);
            };
            // a pair whose candidate lies within the guard of a bin edge is parked in the wave's LDS queue (partner and centre by
            // sorted index) and refined at the end of the cell, one pair per lane: refined in line, the ~150-instruction body ran
            // in 40 % of the centre steps for one or two live lanes (17 of 64 lanes are in range, ~3 % of those near an edge)
            if (lane == 0) *wq_count = 0u;
            int jn = lane < T ? locate(lane) : c_begin;
            uint4 qn = *reinterpret_cast<const uint4 *>(Qf + jn);
            for (int cb = 0; cb < T; cb += 64) {
                const int e = cb + lane;
                const bool alive = e < T;
                const int j = jn;
                const uint4 qj = qn;
                if (cb + 64 < T) {              // the next chunk's records are on their way while this one is evaluated
                    jn = e + 64 < T ? locate(e + 64) : c_begin;
                    qn = *reinterpret_cast<const uint4 *>(Qf + jn);
                }
                const unsigned *kp = koff + (qj.w >> CELL_SPECIES_SHIFT) * S;
                // a partner among the cell's own atoms counts for the centres before it; everything else for every centre
                const int e_own = !alive ? -1 : (e < nown ? e : 0x7fffffff);
                // the cell's atoms are sorted by species (the table has an entry per cell and species): one histogram per
                // species segment, its LDS offset read once -- the inner loop then holds no LDS read, so the NEXT centre's
                // record can be on its way through the scalar cache while this one is evaluated
                auto centres = [&](auto own_tag) {
                    constexpr bool OWN = decltype(own_tag)::value;
                    int seg_b = c_begin;
                    for (int s = 0; s < S; s++) {
                        const int seg_e = __builtin_amdgcn_readfirstlane((int)st[(size_t)cell * S + s + 1]);
                        if (seg_e > seg_b) {
                            unsigned *h = hist + kp[s];
                            QAtom own = Qf[seg_b];
                            for (int ci = seg_b; ci < seg_e; ci++) {
                                const QAtom nxt = Qf[min(ci + 1, seg_e - 1)];          // wave-uniform: scalar loads
                                const int ix = (int)(qj.x - own.ux), iy = (int)(qj.y - own.uy), iz = (int)(qj.z - own.uz);
                                const float q = fast_q<ORTHO>(sc, ix, iy, iz);
                                const bool live = OWN ? (e_own > ci - c_begin) : true;
                                if (live && q < nb_hi) {
                                    if (fabsf(__builtin_amdgcn_fractf(q) - 0.5f) < half_m_guard) {
                                        atomicAdd(&h[(int)q], 1u);
                                    } else {
                                        const unsigned slot = atomicAdd(wq_count, 1u);
                                        if (slot < (unsigned)CW_QCAP) wq[slot] = make_uint2((unsigned)j, (unsigned)ci);
                                        else        // queue full: in place
                                            rdf_pair_refine<ORTHO>(h, fa, fs->sc64, g, q, own.ux, own.uy, own.uz,
                                                                   make_uint4(qj.x, qj.y, qj.z, qj.w & CELL_IDX_MASK), p, own.idx & CELL_IDX_MASK);
                                    }
                                }
                                own = nxt;
                            }
                        }
                        seg_b = seg_e;
                    }
                };
                if (cb < nown) centres(std::true_type{});
                else if (alive) centres(std::false_type{});
            }
            // ---- the cell's flagged pairs: one per lane, the candidate evaluated again from the same records ----
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const int nflag = min((int)*wq_count, CW_QCAP);
            for (int k = lane; k < nflag; k += 64) {
                const uint2 pr = wq[k];
                const uint4 qb = *reinterpret_cast<const uint4 *>(Qf + pr.x);
                const uint4 qa = *reinterpret_cast<const uint4 *>(Qf + pr.y);
                unsigned *h = hist + koff[(qb.w >> CELL_SPECIES_SHIFT) * S + (qa.w >> CELL_SPECIES_SHIFT)];
                const float q = fast_q<ORTHO>(sc, (int)(qb.x - qa.x), (int)(qb.y - qa.y), (int)(qb.z - qa.z));
                rdf_pair_refine<ORTHO>(h, fa, fs->sc64, g, q, qa.x, qa.y, qa.z, make_uint4(qb.x, qb.y, qb.z, qb.w & CELL_IDX_MASK), p,
                                       qa.w & CELL_IDX_MASK);
            }
            __builtin_amdgcn_wave_barrier();     // (the next cell overwrites the run table)
        }
    }   // frames of the chunk
    __syncthreads();
    for (int k = tid; k < ca.npk * nbins; k += CW_THREADS) {
        const unsigned v = hist[k];
        if (v) atomicAdd(&a.U[(size_t)ca.keyU[k / nbins] + (size_t)(k % nbins)], (unsigned long long)v);
    }
}

// hist[a][b][k] += (a == b) ? 2*U[a][a][k] + nsp[a]*selfh[k] : U[min][max][k]
__global__ void rdf_finalize_kernel(const unsigned long long *U, const unsigned long long *selfh,
                                    const long long *nsp, unsigned long long *hist, int S, int nbins)
{
    size_t total = (size_t)S * S * nbins;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (size_t)gridDim.x * blockDim.x) {
        int k = (int)(idx % nbins);
        int ab = (int)(idx / nbins);
        int sa = ab / S, sb = ab % S;
        int lo = sa < sb ? sa : sb, hi = sa < sb ? sb : sa;
        unsigned long long u = U[((size_t)lo * S + hi) * nbins + k];
        unsigned long long add = (sa == sb) ? 2ull * u + (unsigned long long)nsp[sa] * selfh[k] : u;
        hist[idx] += add;
    }
}

// ---- host side: a call record and one function per tier; every decision and record fill is in rdf_select.h ----
struct RdfCall {
    amof_ctx *ctx;
    const amof_traj *t;
    double rmax, dr;
    int32_t nbins;
    HostGeom geom;
    std::vector<double> img;
    std::vector<int32_t> nimg;
    int max_img = 0;
    std::vector<unsigned long long> selfh;
    HostTiles tiles, ftiles;            // tiles of the exact kernels (RDF_TILE) | of the fast tiers (FAST_TILE)
    std::vector<int2> pairs, fpairs;
    std::vector<FrameScale> fsv;        // per-cell records in the tile kernel's axis order
    RdfSwitches sw;
    RdfSelect sel;
    Stager stage;
    void *d_geom, *d_perm, *d_U, *d_self, *d_nsp;
    void *d_ftiles, *d_fpairs, *d_spfirst, *d_fs;       // fast tiers (rdf_fast_prepare)
    size_t U_bytes;
    RdfArgs a;
    RdfFastArgs fa = {};
    bool done = false;                  // a fast tier has answered: no exact kernels
};

// The quantiser's far-atom flag (some atom lies > 1e4 cells away from the origin) behind a fast tier's launches: set, U is
// cleared and the exact kernels take over; clear, the call is done.
static int rdf_take_flag(RdfCall &c, const void *d_flag)
{
    int32_t flag = 0;
    AMOF_TRY(fetch(c.ctx, &flag, d_flag, sizeof flag));
    AMOF_HIP_TRY(c.ctx, sync_stream(c.ctx));
    if (flag) AMOF_HIP_TRY(c.ctx, hipMemsetAsync(c.d_U, 0, c.U_bytes, c.ctx->stream));
    else c.done = true;
    return AMOF_OK;
}

// geometry, images, the exact kernels' tiles; staging, the uploads every tier shares, U cleared
static int rdf_prepare(RdfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    const int S = t->n_species, nbins = c.nbins;
    AMOF_TRY(build_geometry(ctx, t, c.geom));
    AMOF_TRY(build_images(ctx, t, c.geom, c.rmax, c.img, c.nimg, c.max_img));
    const double dr = c.dr, rmax2 = c.rmax * c.rmax;

    // self-image pairs (i, i, E): position independent, histogrammed on the host
    c.selfh.assign((size_t)nbins, 0ull);
    for (int64_t f = 0; f < t->n_frames; f++) {
        size_t gi = t->n_cells == 1 ? 0 : (size_t)f;
        for (int m = 0; m < c.nimg[gi]; m++) {
            const double *E = &c.img[(gi * c.max_img + m) * 3];
            double d2 = fma(E[2], E[2], fma(E[1], E[1], E[0] * E[0]));
            if (d2 < rmax2) {
                int b = (int)(sqrt(d2) / dr);
                if (b < nbins) c.selfh[(size_t)b]++;
            }
        }
    }

    build_tiles(t, RDF_TILE, c.tiles);
    for (int i = 0; i < (int)c.tiles.tiles.size(); i++)
        for (int j = i; j < (int)c.tiles.tiles.size(); j++) c.pairs.push_back(make_int2(i, j));

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    AMOF_TRY(stager_begin(ctx, t, true, c.stage));
    void *d_img, *d_nimg, *d_tiles, *d_pairs;
    AMOF_TRY(upload(ctx, SLOT_GEOM, c.geom.rec.data(), c.geom.rec.size() * sizeof(double), &c.d_geom));
    AMOF_TRY(upload(ctx, SLOT_IMG, c.img.data(), c.img.size() * sizeof(double), &d_img));
    AMOF_TRY(upload(ctx, SLOT_NIMG, c.nimg.data(), c.nimg.size() * sizeof(int32_t), &d_nimg));
    AMOF_TRY(upload(ctx, SLOT_PERM, c.tiles.perm.data(), c.tiles.perm.size() * sizeof(int32_t), &c.d_perm));
    AMOF_TRY(upload(ctx, SLOT_TILES, c.tiles.tiles.data(), c.tiles.tiles.size() * sizeof(Tile), &d_tiles));
    AMOF_TRY(upload(ctx, SLOT_PAIRS, c.pairs.data(), c.pairs.size() * sizeof(int2), &d_pairs));
    AMOF_TRY(upload(ctx, SLOT_SELF, c.selfh.data(), c.selfh.size() * sizeof(unsigned long long), &c.d_self));
    AMOF_TRY(upload(ctx, SLOT_AUX0, c.tiles.nsp.data(), c.tiles.nsp.size() * sizeof(int64_t), &c.d_nsp));
    c.U_bytes = (size_t)S * S * nbins * sizeof(unsigned long long);
    AMOF_TRY(ensure(ctx, SLOT_HISTU, c.U_bytes, &c.d_U));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(c.d_U, 0, c.U_bytes, ctx->stream));

    RdfArgs &a = c.a;
    a.pos = c.stage.dev;
    a.geom = (const double *)c.d_geom;
    a.img = (const double *)d_img;
    a.nimg = (const int32_t *)d_nimg;
    a.perm = (const int32_t *)c.d_perm;
    a.tiles = (const Tile *)d_tiles;
    a.pairs = (const int2 *)d_pairs;
    a.U = (unsigned long long *)c.d_U;
    a.N = t->n_atoms;
    a.F = (int32_t)t->n_frames;
    a.n_cells = (int32_t)t->n_cells;
    a.frames_per_chunk = 1;
    a.nbins = nbins;
    a.S = S;
    a.max_img = c.max_img;
    a.rmax2 = rmax2;
    a.dr = dr;
    return AMOF_OK;
}

// what the cell, range and tile tiers share: tiles of FAST_TILE atoms, their pairs, the per-cell records and the guards
// ---- fast path: fixed-point minimum image + guarded candidate bins ----
static int rdf_fast_prepare(RdfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    const RdfSelect &sel = c.sel;
    HostTiles &ftiles = c.ftiles;
    build_tiles(t, FAST_TILE, ftiles, FAST_SUB);
    for (int i = 0; i < (int)ftiles.tiles.size(); i++)
        for (int j = i; j < (int)ftiles.tiles.size(); j++) c.fpairs.push_back(make_int2(i, j));
    // heavy tile pairs first: the drain tail of the launch is filled with the light ones
    auto cost = [&](const int2 &pr) {
        const double w = (double)ftiles.tiles[pr.x].count * (double)ftiles.tiles[pr.y].count;
        return pr.x == pr.y ? 0.5 * w : w;
    };
    std::stable_sort(c.fpairs.begin(), c.fpairs.end(), [&](const int2 &u, const int2 &v) { return cost(u) > cost(v); });
    AMOF_TRY(upload(ctx, SLOT_AUX2, ftiles.tiles.data(), ftiles.tiles.size() * sizeof(Tile), &c.d_ftiles));
    AMOF_TRY(upload(ctx, SLOT_AUX3, c.fpairs.data(), c.fpairs.size() * sizeof(int2), &c.d_fpairs));
    AMOF_TRY(upload(ctx, SLOT_AUX4, ftiles.sp_first.data(), ftiles.sp_first.size() * sizeof(int64_t), &c.d_spfirst));
    // per-cell records; fixed-point components are stored in the order (ax0, ax1, axis)
    const int ord[3] = {(sel.axis + 1) % 3, (sel.axis + 2) % 3, sel.axis};
    c.fsv.assign((size_t)t->n_cells, FrameScale{});
    fill_frame_scales(t->cell, t->n_cells, c.geom.all_ortho, ord, c.dr, sel.cull_gap.data(), sel.img ? sel.near_thr.data() : nullptr,
                      c.fsv.data());
    AMOF_TRY(upload(ctx, SLOT_AUX5, c.fsv.data(), c.fsv.size() * sizeof(FrameScale), &c.d_fs));
    RdfFastArgs &fa = c.fa;
    fa.a = c.a;
    fa.noreach = c.sw.noreach ? 1 : 0;
    fa.plan_noskip = c.sw.plan_noskip ? 1 : 0;
    fa.plan = nullptr;
    fa.a.tiles = (const Tile *)c.d_ftiles;
    fa.a.pairs = (const int2 *)c.d_fpairs;
    fa.fs = (const FrameScale *)c.d_fs;
    fa.nb_hi = sel.thr.nb_hi;
    fa.half_m_guard = sel.thr.half_m_guard;
    fa.guard64 = sel.guard_m;
    fa.guard64_2 = 2.0 * sel.guard_m * (1.0 + 1e-9);
    fa.guard64_sq = sel.guard_m * sel.guard_m * (1.0 + 1e-9);
    return AMOF_OK;
}

// ---- 3-D cell list for cutoffs far below the cell size (cell kernel) ----
static int rdf_cell_tier(RdfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    const int S = t->n_species, nbins = c.nbins;
    const int *nk = c.sel.nk;
    const bool ortho = c.geom.all_ortho;
    const int npk = S * (S + 1) / 2;
    const size_t lds3 = ((size_t)npk * nbins + (size_t)S * S) * sizeof(unsigned);
    const int nkeys = nk[0] * nk[1] * nk[2] * S;
    AMOF_TRY(stager_need(c.stage, t->n_frames));
    std::vector<FrameScale> fs3((size_t)t->n_cells);
    const int ord[3] = {0, 1, 2};
    fill_frame_scales(t->cell, t->n_cells, ortho, ord, c.dr, nullptr, nullptr, fs3.data());
    std::vector<uint32_t> ktab((size_t)S * S + npk);
    {
        int key = 0;
        for (int lo = 0; lo < S; lo++)
            for (int hi = lo; hi < S; hi++, key++) {
                ktab[(size_t)lo * S + hi] = ktab[(size_t)hi * S + lo] = (uint32_t)(key * nbins);
                ktab[(size_t)S * S + key] = (uint32_t)(((size_t)lo * S + hi) * nbins);
            }
    }
    void *d_fs3, *d_ktab, *d_spec, *d_Q3, *d_start3, *d_keys, *d_cursor, *d_flag3;
    AMOF_TRY(upload(ctx, SLOT_AUX5, fs3.data(), fs3.size() * sizeof(FrameScale), &d_fs3));
    AMOF_TRY(upload(ctx, SLOT_AUX8, ktab.data(), ktab.size() * sizeof(uint32_t), &d_ktab));
    AMOF_TRY(upload(ctx, SLOT_SPEC, t->species, (size_t)t->n_atoms * sizeof(int32_t), &d_spec));
    const size_t per_frame = (size_t)t->n_atoms * (sizeof(QAtom) + sizeof(uint32_t)) + (size_t)(2 * nkeys + 1) * sizeof(uint32_t);
    int64_t FB3 = frame_batch((int64_t)per_frame, t->n_frames);
    if (c.sw.batch) FB3 = std::min<int64_t>(FB3, c.sw.batch);   // (tests cross a frame-batch boundary without gigabytes of frames)
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)FB3 * t->n_atoms * sizeof(QAtom), &d_Q3));
    AMOF_TRY(ensure(ctx, SLOT_AUX7, (size_t)FB3 * (nkeys + 1) * sizeof(uint32_t), &d_start3));
    AMOF_TRY(ensure(ctx, SLOT_AUX6, (size_t)FB3 * t->n_atoms * sizeof(uint32_t), &d_keys));
    AMOF_TRY(ensure(ctx, SLOT_AUX9, (size_t)FB3 * nkeys * sizeof(uint32_t), &d_cursor));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag3));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag3, 0, sizeof(int32_t), ctx->stream));
    RdfCellArgs ca;
    ca.f = c.fa;
    ca.f.fs = (const FrameScale *)d_fs3;
    ca.f.Q = (const QAtom *)d_Q3;
    ca.start3 = (const uint32_t *)d_start3;
    ca.keyoff = (const uint32_t *)d_ktab;
    ca.keyU = (const uint32_t *)d_ktab + (size_t)S * S;
    ca.nx = nk[0]; ca.ny = nk[1]; ca.nz = nk[2];
    ca.npk = npk;
    ca.trim = c.sw.notrim ? 0 : 1;
    // round 5: one wave per cell (rdf_cellwave_kernel) unless AMOF_RDF_CELL_GATHER=1 asks for the per-lane gather form
    const bool wavecell = !c.sw.cell_gather;
    const int64_t groups = ((int64_t)nk[0] * nk[1] * nk[2] + CW_WAVES - 1) / CW_WAVES;
    const size_t lds3w = lds3 + ((size_t)CW_WAVES * CW_WAVE_WORDS + 1) * sizeof(unsigned);
    // (the x extent a batch's frame rule starts from is the one its predecessor launched with)
    unsigned gx = wavecell ? (unsigned)groups : (unsigned)((t->n_atoms + (int64_t)CELL_THREADS - 1) / (int64_t)CELL_THREADS);
    int64_t launches = 0;
    for (int64_t fb = 0; fb < t->n_frames; fb += FB3) {
        const int64_t nf = std::min<int64_t>(FB3, t->n_frames - fb);
        AMOF_TRY(launch_cell_sort(ctx, c.stage.dev, (const double *)c.d_geom, (int)t->n_cells, (const int32_t *)d_spec, S,
                                  t->n_atoms, (int)fb, (int)nf, nk[0], nk[1], nk[2], (QAtom *)d_Q3,
                                  (uint32_t *)d_start3, (uint32_t *)d_keys, (uint32_t *)d_cursor, (int32_t *)d_flag3));
        const CellChunks ch = cell_chunks(nf, gx, wavecell ? groups : 0, c.sw);
        gx = ch.gx;
        ca.f.f_base = (int32_t)fb;
        ca.f.nf = (int32_t)nf;
        ca.f.xcd_map = ch.xcd_map;
        ca.frames_grid = ch.frames_grid;
        ca.fpc = ch.fpc;
        ca.cpt = ch.cpw;
        dim3 grid(gx, (unsigned)ca.frames_grid);
        if (launches == 0) timing_dom_begin(ctx, "rdf_cell");
        AMOF_HIP_TRY(ctx, with_flag(ortho, [&](auto O) {
            return wavecell ? launch_lds(rdf_cellwave_kernel<O()>, grid, dim3(CW_THREADS), lds3w, ctx->stream, ca)
                            : launch_lds(rdf_cell_kernel<O()>, grid, dim3(CELL_THREADS), lds3, ctx->stream, ca);
        }));
        launches++;
    }
    timing_dom_end(ctx, launches);
    return rdf_take_flag(c, d_flag3);     // (either done, or the exact kernels take over)
}

// ---- two-level cell list for small cutoffs (range kernel) ----
static int rdf_range_tier(RdfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    const RdfSelect &sel = c.sel;
    const HostTiles &ftiles = c.ftiles;
    const int S = t->n_species, nbins = c.nbins, nz2 = sel.nz2;
    AMOF_TRY(stager_need(c.stage, t->n_frames));
    // scale records: stored component order is (remaining axis, axis_y, axis)
    const int ord2[3] = {3 - sel.axis - sel.axis_y, sel.axis_y, sel.axis};
    fill_frame_scales(t->cell, t->n_cells, c.geom.all_ortho, ord2, c.dr, nullptr, nullptr, c.fsv.data());
    AMOF_TRY(upload(ctx, SLOT_AUX5, c.fsv.data(), c.fsv.size() * sizeof(FrameScale), &c.d_fs));
    std::vector<int4> rwork;
    for (int sa2 = 0; sa2 < S; sa2++)
        for (int64_t c0 = 0; c0 < ftiles.nsp[sa2]; c0 += FAST_SUB)
            for (int sb2 = sa2; sb2 < S; sb2++)
                if (ftiles.nsp[sb2] > 0) rwork.push_back(make_int4(sa2, (int)c0, sb2, 0));
    void *d_rwork, *d_start2, *d_Q2, *d_flag2;
    AMOF_TRY(upload(ctx, SLOT_AUX6, rwork.data(), rwork.size() * sizeof(int4), &d_rwork));
    const size_t per_frame = (size_t)t->n_atoms * sizeof(QAtom) + (size_t)S * (nz2 * 256 + 1) * sizeof(uint32_t);
    const int64_t FB2 = frame_batch((int64_t)per_frame, t->n_frames);
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)FB2 * t->n_atoms * sizeof(QAtom), &d_Q2));
    AMOF_TRY(ensure(ctx, SLOT_AUX7, (size_t)FB2 * S * (nz2 * 256 + 1) * sizeof(uint32_t), &d_start2));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag2));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag2, 0, sizeof(int32_t), ctx->stream));
    RdfRangeArgs ra;
    ra.f = c.fa;
    ra.f.fs = (const FrameScale *)c.d_fs;
    ra.f.Q = (const QAtom *)d_Q2;
    ra.f.xcd_map = 0;
    ra.start2 = (const uint32_t *)d_start2;
    ra.sp_first = (const int64_t *)c.d_spfirst;
    ra.work = (const int4 *)d_rwork;
    ra.nz = nz2;
    ra.gy_bins = sel.gy;
    const size_t lds2 = FAST_TILE * sizeof(uint4) + (size_t)nbins * sizeof(unsigned);
    int64_t launches = 0;
    for (int64_t fb = 0; fb < t->n_frames && !rwork.empty(); fb += FB2) {
        const int64_t nf = std::min<int64_t>(FB2, t->n_frames - fb);
        AMOF_TRY(launch_quantize2(ctx, c.stage.dev, (const double *)c.d_geom, (int)t->n_cells, (const int32_t *)c.d_perm,
                                  (const int64_t *)c.d_spfirst, S, t->n_atoms, (int)fb, (int)nf, sel.axis, sel.axis_y, nz2,
                                  (QAtom *)d_Q2, (uint32_t *)d_start2, (int32_t *)d_flag2));
        ra.f.f_base = (int32_t)fb;
        ra.f.nf = (int32_t)nf;
        unsigned chunks;
        pick_chunks(nf, (int64_t)rwork.size(), 16, ra.f.a.frames_per_chunk, chunks);
        dim3 grid((unsigned)rwork.size(), chunks);
        if (launches == 0) timing_dom_begin(ctx, "rdf_range");
        AMOF_HIP_TRY(ctx, with_flag(c.geom.all_ortho, [&](auto O) {
            return launch_lds(rdf_range_kernel_fast<O()>, grid, dim3(FAST_THREADS), lds2, ctx->stream, ra);
        }));
        launches++;
    }
    timing_dom_end(ctx, launches);
    return rdf_take_flag(c, d_flag2);
}

// TRI: the variant's own per-cell records, fold table, guards and queue into k; *d_fold: the fold table for the quantiser
static int rdf_tri_args(RdfCall &c, RdfFastArgs &k, const double **d_fold)
{
    amof_ctx *ctx = c.ctx;
    const RdfSelect &sel = c.sel;
    const TriSelect &tri = sel.tri;
    const int64_t nc = c.t->n_cells;
    const int nbins = c.nbins;
    const double dr = c.dr;
    std::vector<FrameScale> fst((size_t)nc);
    fill_frame_scales_tri(tri.rec.data(), nc, sel.cull_gap.data(), fst.data());      // (same slab axis, same height)
    double hb = 0.0, gfrac = 0.0;
    for (int64_t q = 0; q < nc; q++) {
        hb = std::max(hb, c.geom.rec[(size_t)q * GEOM_STRIDE + 18 + sel.axis] / dr);
        gfrac = std::max(gfrac, sel.cull ? (double)sel.cull_gap[(size_t)q] / 4294967296.0 : 0.5);
    }
    void *d_fst, *d_foldv;
    AMOF_TRY(upload(ctx, SLOT_AUX5, fst.data(), fst.size() * sizeof(FrameScale), &d_fst));
    AMOF_TRY(upload(ctx, SLOT_AUX6, tri.fold.data(), tri.fold.size() * sizeof(double), &d_foldv));
    *d_fold = (const double *)d_foldv;
    k.fs = (const FrameScale *)d_fst;
    // folded coordinates: two fold roundings and the wrap constant on top of the truncation (2.5 grid units per
    // axis instead of 1): twice the grid term; XW: the truncated f32 product c10 iy moves the x wrap and the
    // candidate by < 1 + 256 |c10| units more (quant = 2 units of csum)
    // (in units of the x axis: |A| <= csum; 1.5 for margin)
    const double guard_m_tri = 2.0 * sel.quant / dr +
                               (tri.code >= 5 || tri.code % 5 == 4 ? (1.0 + 256.0 * tri.c10) * 1.5 * sel.csum * (1.0 / 4294967296.0) / dr : 0.0) +
                               (double)nbins * 1e-12;
    // (the twin image of near mode 4 has |iy| up to 2^31 (1 + 2 tau): its candidate's error bound grows with it)
    const double guard_tri = fast_guard_tri(nbins, hb, gfrac, tri.l10_bins) * (1.0 + 4.0 * tri.tau) + guard_m_tri;
    if (!(guard_tri < 0.25)) return fail(ctx, AMOF_ECAPACITY, "TRI guard out of range");      // (checked at selection)
    k.half_m_guard = guard_thresholds(nbins, guard_tri).half_m_guard;
    k.guard64 = guard_m_tri;
    k.guard64_2 = 2.0 * guard_m_tri * (1.0 + 1e-9);
    k.guard64_sq = guard_m_tri * guard_m_tri * (1.0 + 1e-9);
    // queue: the near pairs (share of all pairs) and the level-3 pairs of a step
    const ParkedQueue pq = parked_queue(tri.share);
    k.img_queue = pq.img_queue;
    k.img_defer = pq.img_defer;
    return AMOF_OK;
}

// one launch of the tile kernel's selected variant.  TRI: one instantiation per code (near tests x x wrap); ZF: a list of
// four (planned with / without the records read a quad ahead, culled, unculled)
static hipError_t rdf_tile_launch(RdfCall &c, const RdfFastArgs &k, dim3 grid, size_t lds, bool plan, bool sat)
{
    const RdfSelect &sel = c.sel;
    const bool ortho = c.geom.all_ortho, cull = sel.cull;
    auto launch = [&](auto kern) {
        const hipError_t e = launch_lds<true>(kern, grid, dim3(FAST_THREADS), lds, c.ctx->stream, k);
        if (e != hipSuccess) return e;
        // what the hardware grants: workgroups per CU of this variant at this LDS size, asked once per (variant, size,
        // device); the planned kernels are built for six at the headline, and nothing depends on the answer
        static std::mutex mu;
        static std::map<std::tuple<const void *, size_t, int>, int> granted;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) return hipGetLastError();
        std::lock_guard<std::mutex> lock(mu);
        const auto key = std::make_tuple((const void *)kern, lds, dev);
        if (!granted.count(key)) {
            int n = 0;
            const hipError_t eo = hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, kern, FAST_THREADS, lds);
            if (eo != hipSuccess) return eo;
            granted[key] = n;
            if (c.sw.debug)
                fprintf(stderr, "rdf_tile: %s%s%s%d bins, %zu bytes of LDS: %d workgroups per CU\n", plan ? "plan, " : "",
                        plan && !c.sw.noahead ? "read-ahead, " : "", sat ? "saturating tail, " : "", c.nbins, lds, n);
        }
        return hipSuccess;
    };
    if (sel.tri.ok)
        return with_flag(cull, [&](auto C) {
            return with_count<12>(sel.tri.code, [&](auto K) { return launch(rdf_tile_kernel_fast<false, C(), false, true, K()>); });
        });
    if (sel.img) return with_flags(ortho, cull, [&](auto O, auto C) { return launch(rdf_tile_kernel_fast<O(), C(), true>); });
    if (sel.zf)
        return sat && !c.sw.noahead  ? launch(rdf_tile_kernel_fast<true, true, false, true, -1, true, 1, true>)
               : sat                 ? launch(rdf_tile_kernel_fast<true, true, false, true, -1, true, 0, true>)
               : plan && !c.sw.noahead ? launch(rdf_tile_kernel_fast<true, true, false, true, -1, true, 1>)
               : plan                ? launch(rdf_tile_kernel_fast<true, true, false, true, -1, true>)
               : cull                ? launch(rdf_tile_kernel_fast<true, true, false, true>)
                                     : launch(rdf_tile_kernel_fast<true, false, false, true>);
    return with_flags(ortho, cull, [&](auto O, auto C) { return launch(rdf_tile_kernel_fast<O(), C()>); });
}

// ---- slab list (tile kernel): rdf_tile, rdf_tile_zf, rdf_tile_img, rdf_tile_tri ----
static int rdf_tile_tier(RdfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    const RdfSelect &sel = c.sel;
    const int S = t->n_species, nbins = c.nbins;
    const bool tri = sel.tri.ok;
    const int64_t FB = frame_batch(t->n_atoms * 16, t->n_frames);
    // host-resident input: batches of 512, 1024, 2048 ... frames (each >= 32 chunks of 16 frames); the copy
    // of batch k+1 overlaps the kernels of batch k, and only the first, small copy is exposed
    int64_t cur = c.stage.lazy ? std::min<int64_t>(FB, 512) : FB;
    if (c.sw.batch) cur = std::min<int64_t>(FB, c.sw.batch);   // experiments
    void *d_Q, *d_flag;
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)FB * t->n_atoms * sizeof(QAtom), &d_Q));
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
    RdfFastArgs k = c.fa;       // the selected variant's arguments
    k.Q = (const QAtom *)d_Q;
    k.img_queue = 0;
    k.img_defer = 0;
    const double *d_fold = nullptr;
    if (tri) {
        AMOF_TRY(rdf_tri_args(c, k, &d_fold));
    } else if (sel.img) {
        const ParkedQueue pq = parked_queue(sel.img_share);
        k.img_queue = pq.img_queue;
        k.img_defer = pq.img_defer;
    } else if (sel.zf) {
        k.nb_hi = sel.zf_thr.nb_hi;
        k.half_m_guard = sel.zf_thr.half_m_guard;
        k.sat_one_p_guard = sel.sat_thr.one_p_guard;
        k.sat_two_guard = sel.sat_thr.two_guard;
    }
    // rdf_tile_zf with slab culling runs from a plan of its steps (rdf_tile_kernel_fast, PLAN): the quantiser writes
    // its slab table, rdf_tile_plan_kernel the records.  Not for tables beyond the plan kernel's LDS or plans beyond
    // 256 MiB (systems far larger than a tile kernel's share).
    const size_t plan_lds = (size_t)S * (QSLABS + 1) * sizeof(uint32_t) + c.ftiles.tiles.size() * TILE_PLAN_MAX_SUBS * sizeof(uint32_t);
    const size_t plan_bytes = c.fpairs.size() * (size_t)FB * TILE_PLAN_MAX_SUBS * sizeof(uint4);
    const bool plan_ok = sel.zf && sel.cull && !tri && !sel.img && !c.sw.noplan && plan_lds <= 64 * 1024 &&
                         plan_bytes <= ((size_t)256 << 20);
    void *d_slab = nullptr, *d_plan = nullptr;
    if (plan_ok) {
        AMOF_TRY(ensure(ctx, SLOT_AUX7, (size_t)FB * S * (QSLABS + 1) * sizeof(uint32_t), &d_slab));
        AMOF_TRY(ensure(ctx, SLOT_AUX9, plan_bytes, &d_plan));
    }
    int64_t launches = 0;
    for (int64_t fb = 0; fb < t->n_frames; fb += cur, cur = std::min<int64_t>(2 * cur, FB)) {
        const int64_t nf = std::min<int64_t>(cur, t->n_frames - fb);
        AMOF_TRY(stager_need(c.stage, fb + nf));
        AMOF_TRY(launch_quantize(ctx, c.stage.dev, (const double *)c.d_geom, (int)t->n_cells, (const int32_t *)c.d_perm,
                                 (const int64_t *)c.d_spfirst, S, t->n_atoms, (int)fb, (int)nf, sel.axis, (QAtom *)d_Q,
                                 (uint32_t *)d_slab, (int32_t *)d_flag, tri ? sel.tri.ax0 : -1, tri ? sel.tri.ax1 : -1, d_fold));
        const TileChunks ch = tile_chunks(nf, (int64_t)c.fpairs.size(), c.sw);
        k.f_base = (int32_t)fb;
        k.nf = (int32_t)nf;
        k.xcd_map = ch.xcd_map;
        k.a.frames_per_chunk = ch.fpc;
        k.n_chunks = ch.chunks;
        k.nf_main = ch.nf_main;
        dim3 grid((unsigned)c.fpairs.size(), (unsigned)(ch.chunks + ch.nf_tail));
        const bool plan = plan_ok && ch.plan_fits;
        k.plan = nullptr;
        if (plan) {
            TilePlanArgs pa;
            pa.slab_start = (const uint32_t *)d_slab;
            pa.tiles = (const Tile *)c.d_ftiles;
            pa.pairs = (const int2 *)c.d_fpairs;
            pa.sp_first = (const int64_t *)c.d_spfirst;
            pa.fs = (const FrameScale *)c.d_fs;
            pa.plan = (uint4 *)d_plan;
            pa.S = S; pa.ntiles = (int32_t)c.ftiles.tiles.size(); pa.npairs = (int32_t)c.fpairs.size();
            pa.nf = (int32_t)nf; pa.f_base = (int32_t)fb; pa.n_cells = (int32_t)t->n_cells;
            AMOF_HIP_TRY(ctx, launch_lds(rdf_tile_plan_kernel, dim3((unsigned)nf), dim3(PLAN_THREADS), plan_lds, ctx->stream, pa));
            k.plan = (const uint4 *)d_plan;
        }
        if (launches == 0) timing_dom_begin(ctx, tri ? "rdf_tile_tri" : sel.img ? "rdf_tile_img" : sel.zf ? "rdf_tile_zf" : "rdf_tile");
        // (a batch without a plan runs the kernel with centre buffers, at their size; a planned one has two z slices: the
        //  steps in integer form and the steps on f32 slab coordinates, rdf_tile_kernel_fast)
        // (the saturating tail of the f32-slab slice: planned launches only, AMOF_RDF_NOSAT=1 keeps the clamped one)
        const bool sat = plan && sel.sat;
        if (plan) grid.z = 2;
        AMOF_HIP_TRY(ctx, rdf_tile_launch(c, k, grid, tile_lds(nbins, k.img_queue, k.img_defer, plan, sat), plan, sat));
        launches++;
    }
    timing_dom_end(ctx, launches);
    return rdf_take_flag(c, d_flag);
}

// ---- exact kernels: canonical f64 arithmetic, every image ----
static int rdf_exact_tier(RdfCall &c)
{
    amof_ctx *ctx = c.ctx;
    RdfArgs &a = c.a;
    AMOF_TRY(stager_need(c.stage, c.t->n_frames));
    unsigned chunks;
    pick_chunks(c.t->n_frames, (int64_t)c.pairs.size(), 64, a.frames_per_chunk, chunks);
    dim3 grid((unsigned)c.pairs.size(), chunks);
    timing_dom_begin(ctx, "rdf_exact");
    const hipError_t e = with_flags(c.geom.all_ortho, c.max_img > 0, [&](auto O, auto EXTRA) {
        if (c.nbins <= AMOF_MAX_LDS_BINS)
            return launch_lds(rdf_tile_kernel<O(), EXTRA()>, grid, dim3(RDF_TILE),
                              3 * RDF_TILE * sizeof(double) + (size_t)c.nbins * sizeof(unsigned), ctx->stream, a);
        hipLaunchKernelGGL((rdf_tile_kernel_global<O(), EXTRA()>), grid, dim3(RDF_TILE), 0, ctx->stream, a);
        return hipGetLastError();
    });
    AMOF_HIP_TRY(ctx, e);
    timing_dom_end(ctx, 1);
    return AMOF_OK;
}

static int rdf_run(amof_ctx *ctx, const amof_traj *t, double rmax, int32_t nbins,
                   unsigned long long *hist_dev, double *volume_sum)
{
    RdfCall c;
    c.ctx = ctx;
    c.t = t;
    c.rmax = rmax;
    c.nbins = nbins;
    c.dr = rmax / nbins;
    c.sw = RdfSwitches::from_env();
    AMOF_TRY(rdf_prepare(c));
    if (!c.pairs.empty() && t->n_frames > 0) {
        std::vector<double> heights((size_t)t->n_cells * 3);
        for (int64_t k = 0; k < t->n_cells; k++)
            for (int x = 0; x < 3; x++) heights[(size_t)k * 3 + x] = c.geom.rec[(size_t)k * GEOM_STRIDE + 18 + x];
        c.sel = rdf_select(t->cell, heights.data(), t->n_cells, t->pbc, t->n_species, t->n_atoms, c.tiles.nsp.data(), nbins, rmax,
                           c.max_img, c.geom.all_ortho, c.sw);
        const TriSelect &tri = c.sel.tri;
        if (tri.ok && c.sw.debug)
            fprintf(stderr, "rdf_tile_tri: code %d (near mode %d, x wrap %d) axes (%d, %d | %d) parked share %.4f tau %.5f c10 %.5f\n", tri.code,
                    tri.code >= 10 ? 4 : tri.code % 5, tri.code >= 10 ? 2 : tri.code / 5, tri.ax0, tri.ax1, tri.axis, tri.share, tri.tau, tri.c10);
        // a taken cell tier excludes range and tile; a tier that met far-away atoms hands over to the exact kernels
        if (c.sel.tile()) {
            AMOF_TRY(rdf_fast_prepare(c));
            if (c.sel.cell) AMOF_TRY(rdf_cell_tier(c));
            else if (c.sel.range) AMOF_TRY(rdf_range_tier(c));
            else AMOF_TRY(rdf_tile_tier(c));
        }
        if (!c.done) AMOF_TRY(rdf_exact_tier(c));
    }
    {
        size_t total = (size_t)t->n_species * t->n_species * nbins;
        int blocks = (int)std::min<size_t>((total + 255) / 256, 4096);
        hipLaunchKernelGGL(rdf_finalize_kernel, dim3(blocks), dim3(256), 0, ctx->stream,
                           (const unsigned long long *)c.d_U, (const unsigned long long *)c.d_self,
                           (const long long *)c.d_nsp, hist_dev, t->n_species, nbins);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    timing_end(ctx);
    // host metadata above lives on this stack frame: finish before returning
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    if (volume_sum) *volume_sum += c.geom.volume_sum;
    return AMOF_OK;
}

static int rdf_check(amof_ctx *ctx, const amof_traj *t, double rmax, int32_t nbins, const void *hist)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    if (!(rmax > 0.0) || !isfinite(rmax)) return fail(ctx, AMOF_EINVAL, "rmax must be positive and finite");
    if (nbins <= 0) return fail(ctx, AMOF_EINVAL, "nbins must be positive");
    if (!hist) return fail(ctx, AMOF_EINVAL, "hist is NULL");
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

extern "C" int amof_rdf_accumulate_dev(amof_ctx *ctx, const amof_traj *traj, double rmax, int32_t nbins,
                                       uint64_t *hist_dev, double *volume_sum)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(rdf_check(ctx, traj, rmax, nbins, hist_dev));
    return rdf_run(ctx, traj, rmax, nbins, (unsigned long long *)hist_dev, volume_sum);
}

extern "C" int amof_rdf_accumulate(amof_ctx *ctx, const amof_traj *traj, double rmax, int32_t nbins,
                                   uint64_t *hist, double *volume_sum)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(rdf_check(ctx, traj, rmax, nbins, hist));
    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t bytes = (size_t)traj->n_species * traj->n_species * nbins * sizeof(uint64_t);
    void *d_hist = nullptr;
    AMOF_TRY(upload(ctx, SLOT_OUT0, hist, bytes, &d_hist));
    AMOF_TRY(rdf_run(ctx, traj, rmax, nbins, (unsigned long long *)d_hist, volume_sum));
    AMOF_TRY(fetch(ctx, hist, d_hist, bytes));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}
