// Distinct Van Hove function: pair-distance histograms between frame k and frame k + m (gfx950).
//
// For every lag m = windows[w] and origin k = 1, 1 + s, ... <= F - m - 1 (s = origin_stride), every ordered pair (i, j),
// i != j, with i at frame k and j at frame k + m is binned by the RDF's rule: d0 = r_j(k+m) - r_i(k) on the raw float64
// positions, the canonical minimum image of DESIGN §2 in frame k's cell (plus every further image in reach), counted iff
// d2 < rmax^2 and b = (int)(sqrt(d2) / (rmax / nbins)) < nbins.  At m = 0 this is, pair for pair, what the RDF counts.
// The work is the flattened list of (lag, origin) pairs in lag-major order; a call takes [work_begin, work_end) of it, so
// ranks and halves add up bit for bit (integer counters only).  Kernel families (amof_last_path):
//   rdf_distinct_exact         rdf_distinct_exact_kernel<ORTHO,EXTRA,false>: every ordered pair through pair_base with
//                              frame k's geometry and image list; u32 counters [S][nbins] in LDS (the centre species is
//                              fixed per workgroup), flushed with u64 atomics once per chunk of origins of one lag
//   rdf_distinct_exact_global  the same kernel with u64 atomics into the global counters (S nbins beyond the LDS budget,
//                              more pairs per chunk than a u32 holds, or AMOF_VANHOVE_DISTINCT_GLOBAL=1)
//   rdf_distinct_tile          rdf_distinct_tile_kernel: constant diagonal cell, all axes periodic, one image in reach.
//                              Frames quantised by quantize_frame_kernel, centre records from Q[k], partner
//                              records from Q[k+m] through LDS, an f32 candidate from the u32 differences with the guard
//                              band of the RDF tile kernels (fast_guard_rel_rdf), every pair inside the band re-decided
//                              with the canonical arithmetic on the raw positions
// AMOF_VANHOVE_DISTINCT_EXACT=1 forces the exact kernel.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <vector>

#include "amof_internal.h"
#include "rdf_select.h"

namespace amof {
namespace {

constexpr int VHD_THREADS = 256;    // one centre atom per thread, partner tiles of 256 atoms
constexpr int VHD_OPC = 64;         // at most this many origins per workgroup (one lag)

struct VhdItem {
    int32_t k, km;      // origin frame, partner frame k + m
    int32_t sk, skm;    // their slots in the quantised batch (tile path)
};
struct VhdChunk {
    int32_t w;          // lag index
    int32_t i0, i1;     // items [i0, i1), all of lag w
    int32_t _pad;
};

struct VhdArgs {
    const double *pos;          // [F][N][3]
    const double *geom;         // [n_cells][GEOM_STRIDE]
    const double *img;          // [n_cells][max_img][3]
    const int32_t *nimg;        // [n_cells]
    const int32_t *perm;        // [N] species-sorted atom ids
    const Tile *tiles;          // species-pure tiles of <= 256 atoms
    const VhdChunk *chunks;
    const VhdItem *items;
    const QAtom *Q;             // tile path: [slots][N]
    unsigned long long *hist;   // [S][S][W][nbins]
    int64_t N;
    int32_t n_cells, S, W, nbins, max_img, n_tiles;
    double rmax2, dr;
    float sc2[3];               // tile path: (L_c 2^-32 / dr)^2
    float half_m_guard;         // 1/2 - g_f rounded down
    float nb_hi;                // nbins + g_f rounded up
};

// the RDF rule on a squared distance (exact IEEE sqrt and divide: the bin is an integer result)
template <bool GLOBAL>
__device__ __forceinline__ void vhd_count(unsigned *h, unsigned long long *hg, double d2, double rmax2, double dr, int nbins)
{
    if (d2 < rmax2) {
        const int b = (int)(sqrt(d2) / dr);
        if (b < nbins) {
            if (GLOBAL) atomicAdd(&hg[b], 1ull);
            else atomicAdd(&h[b], 1u);
        }
    }
}

template <bool ORTHO, bool EXTRA, bool GLOBAL>
__global__ __launch_bounds__(VHD_THREADS) void rdf_distinct_exact_kernel(VhdArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double *tjx = reinterpret_cast<double *>(lds_raw);
    double *tjy = tjx + VHD_THREADS;
    double *tjz = tjy + VHD_THREADS;
    int32_t *tja = reinterpret_cast<int32_t *>(tjz + VHD_THREADS);
    unsigned *hist = reinterpret_cast<unsigned *>(tja + VHD_THREADS);     // [S][nbins] (!GLOBAL)

    const int tid = threadIdx.x;
    const VhdChunk c = a.chunks[blockIdx.x];
    const Tile ti = a.tiles[blockIdx.y];
    const int nbins = a.nbins, S = a.S;
    const int64_t N = a.N;
    if (!GLOBAL)
        for (int k = tid; k < S * nbins; k += VHD_THREADS) hist[k] = 0u;
    const int32_t ai = tid < ti.count ? a.perm[ti.start + tid] : -1;
    const double rmax2 = a.rmax2, dr = a.dr;
    unsigned long long *hrow = a.hist + ((size_t)ti.species * S * a.W + c.w) * (size_t)nbins;   // + sj W nbins

    for (int it = c.i0; it < c.i1; it++) {
        const VhdItem item = a.items[it];
        const int gi = a.n_cells == 1 ? 0 : item.k;
        const double *__restrict__ g = a.geom + (size_t)gi * GEOM_STRIDE;
        const double *__restrict__ pi = a.pos + (size_t)item.k * (size_t)N * 3;
        const double *__restrict__ pj = a.pos + (size_t)item.km * (size_t)N * 3;
        double xi = 0.0, yi = 0.0, zi = 0.0;
        if (ai >= 0) {
            xi = pi[(size_t)ai * 3 + 0];
            yi = pi[(size_t)ai * 3 + 1];
            zi = pi[(size_t)ai * 3 + 2];
        }
        const int ne = EXTRA ? a.nimg[gi] : 0;
        const double *__restrict__ E = EXTRA ? a.img + (size_t)gi * a.max_img * 3 : nullptr;
        for (int t = 0; t < a.n_tiles; t++) {
            const Tile tj = a.tiles[t];
            __syncthreads();    // the previous tile is consumed (and the histogram zeroed)
            if (tid < tj.count) {
                const int32_t aj = a.perm[tj.start + tid];
                tjx[tid] = pj[(size_t)aj * 3 + 0];
                tjy[tid] = pj[(size_t)aj * 3 + 1];
                tjz[tid] = pj[(size_t)aj * 3 + 2];
                tja[tid] = aj;
            }
            __syncthreads();
            if (ai >= 0) {
                unsigned *h = GLOBAL ? nullptr : hist + (size_t)tj.species * nbins;
                unsigned long long *hg = GLOBAL ? hrow + (size_t)tj.species * a.W * nbins : nullptr;
                for (int j = 0; j < tj.count; j++) {
                    if (tja[j] == ai) continue;         // the atom itself at frame k + m: not a distinct pair
                    double dx, dy, dz;
                    pair_base<ORTHO>(g, tjx[j] - xi, tjy[j] - yi, tjz[j] - zi, dx, dy, dz);
                    vhd_count<GLOBAL>(h, hg, norm2(dx, dy, dz), rmax2, dr, nbins);
                    if (EXTRA)
                        for (int m = 0; m < ne; m++)
                            vhd_count<GLOBAL>(h, hg, norm2(dx + E[3 * m], dy + E[3 * m + 1], dz + E[3 * m + 2]), rmax2, dr, nbins);
                }
            }
        }
    }
    if (!GLOBAL) {
        __syncthreads();
        for (int k = tid; k < S * nbins; k += VHD_THREADS) {
            const unsigned v = hist[k];
            if (v) atomicAdd(&hrow[(size_t)(k / nbins) * a.W * nbins + (k % nbins)], (unsigned long long)v);
        }
    }
}

// f32 candidate bin coordinate q~ = |d| / dr of a diagonal cell from the u32 differences: the chain of the RDF tile
// kernels' diagonal form (squares first, then the squared scales), whose error fast_guard_rel_rdf bounds
__device__ __forceinline__ float vhd_q(const float *sc2, int ix, int iy, int iz)
{
    const float fx = (float)ix, fy = (float)iy, fz = (float)iz;
    const float x2 = fx * fx, y2 = fy * fy, z2 = fz * fz;
    return __builtin_amdgcn_sqrtf(fmaf(z2, sc2[2], fmaf(y2, sc2[1], x2 * sc2[0])));
}

__global__ __launch_bounds__(VHD_THREADS) void rdf_distinct_tile_kernel(VhdArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint4 *tq = reinterpret_cast<uint4 *>(lds_raw);                       // partner records [256]
    unsigned *hist = reinterpret_cast<unsigned *>(tq + VHD_THREADS);      // [S][nbins]

    const int tid = threadIdx.x;
    const VhdChunk c = a.chunks[blockIdx.x];
    const Tile ti = a.tiles[blockIdx.y];
    const int nbins = a.nbins, S = a.S;
    const int64_t N = a.N;
    for (int k = tid; k < S * nbins; k += VHD_THREADS) hist[k] = 0u;
    const float sc2[3] = {a.sc2[0], a.sc2[1], a.sc2[2]};
    const float hmg = a.half_m_guard, nb_hi = a.nb_hi;
    const double rmax2 = a.rmax2, dr = a.dr;
    const double *__restrict__ g = a.geom;
    const bool live = tid < ti.count;

    for (int it = c.i0; it < c.i1; it++) {
        const VhdItem item = a.items[it];
        const uint4 *__restrict__ Qi = reinterpret_cast<const uint4 *>(a.Q + (size_t)item.sk * N);
        const uint4 *__restrict__ Qj = reinterpret_cast<const uint4 *>(a.Q + (size_t)item.skm * N);
        const uint4 qi = live ? Qi[ti.start + tid] : make_uint4(0u, 0u, 0u, 0u);
        for (int t = 0; t < a.n_tiles; t++) {
            const Tile tj = a.tiles[t];
            __syncthreads();
            if (tid < tj.count) tq[tid] = Qj[tj.start + tid];
            __syncthreads();
            if (live) {
                unsigned *h = hist + (size_t)tj.species * nbins;
                for (int j = 0; j < tj.count; j++) {
                    const uint4 qj = tq[j];
                    const float q = vhd_q(sc2, (int)(qj.x - qi.x), (int)(qj.y - qi.y), (int)(qj.z - qi.z));
                    if (!(q < nb_hi) || qj.w == qi.w) continue;     // beyond rmax (by more than the band), or the atom itself
                    const float fr = q - floorf(q);
                    if (fabsf(fr - 0.5f) < hmg) {
                        const int b = (int)q;
                        if (b < nbins) atomicAdd(&h[b], 1u);
                    } else {
                        // inside the band of a bin edge: the canonical arithmetic on the raw positions decides
                        const double *__restrict__ ri = a.pos + ((size_t)item.k * N + qi.w) * 3;
                        const double *__restrict__ rj = a.pos + ((size_t)item.km * N + qj.w) * 3;
                        double dx, dy, dz;
                        pair_base<true>(g, rj[0] - ri[0], rj[1] - ri[1], rj[2] - ri[2], dx, dy, dz);
                        vhd_count<false>(h, nullptr, norm2(dx, dy, dz), rmax2, dr, nbins);
                    }
                }
            }
        }
    }
    __syncthreads();
    unsigned long long *hrow = a.hist + ((size_t)ti.species * S * a.W + c.w) * (size_t)nbins;
    for (int k = tid; k < S * nbins; k += VHD_THREADS) {
        const unsigned v = hist[k];
        if (v) atomicAdd(&hrow[(size_t)(k / nbins) * a.W * nbins + (k % nbins)], (unsigned long long)v);
    }
}

// items of [wb, we) of the lag-major work list, with their lag index
void vhd_items(const int32_t *windows, int W, int64_t F, int64_t stride, int64_t wb, int64_t we, std::vector<VhdItem> &items,
               std::vector<int32_t> &lag_of)
{
    std::vector<LagRange> iv((size_t)W);
    lag_work_ranges(windows, W, F, stride, wb, we, iv.data());
    for (int w = 0; w < W; w++)
        for (int64_t o = iv[w].o0; o < iv[w].o1; o++) {
            const int64_t k = lag_origin_frame(o, stride);
            items.push_back(VhdItem{(int32_t)k, (int32_t)(k + windows[w]), 0, 0});
            lag_of.push_back(w);
        }
}

// consecutive items of one lag, at most opc per chunk
void vhd_chunks(const std::vector<int32_t> &lag_of, size_t i0, size_t i1, int opc, std::vector<VhdChunk> &chunks)
{
    size_t i = i0;
    while (i < i1) {
        size_t e = i + 1;
        while (e < i1 && lag_of[e] == lag_of[i] && e - i < (size_t)opc) e++;
        chunks.push_back(VhdChunk{lag_of[i], (int32_t)i, (int32_t)e, 0});
        i = e;
    }
}

// hist (host, overwritten) or hist_dev (device, added into)
int vhd_run(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int64_t stride, int64_t wb, int64_t we,
            double rmax, int32_t nbins, uint64_t *hist, uint64_t *hist_dev)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    const int S = t->n_species;
    const int64_t N = t->n_atoms, F = t->n_frames;
    AMOF_TRY(check_lag_args(ctx, windows, W, F, stride));
    if (!(rmax > 0.0) || !isfinite(rmax)) return fail(ctx, AMOF_EINVAL, "rmax must be positive and finite");
    if (nbins <= 0) return fail(ctx, AMOF_EINVAL, "nbins must be positive");
    if (F > 0x7fffffffLL || N > 0x7fffffffLL) return fail(ctx, AMOF_EINVAL, "too many frames or atoms");
    const int64_t total = lag_work_total(windows, W, F, stride);
    if (wb < 0 || we > total || wb > we) return fail(ctx, AMOF_EINVAL, "work range [%lld, %lld) outside [0, %lld)", (long long)wb,
                                                     (long long)we, (long long)total);
    const size_t hsize = (size_t)S * S * W * nbins;
    if (hsize > ((size_t)1 << 36)) return fail(ctx, AMOF_EINVAL, "histogram too large");
    if (hist) std::fill(hist, hist + hsize, (uint64_t)0);
    if (wb == we || N < 2 || hsize == 0) return AMOF_OK;

    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    std::vector<double> img;
    std::vector<int32_t> nimg;
    int max_img = 0;
    AMOF_TRY(build_images(ctx, t, geom, rmax, img, nimg, max_img));
    if (img.empty()) img.push_back(0.0);
    const double dr = rmax / nbins;
    HostTiles tiles;
    build_tiles(t, VHD_THREADS, tiles);
    const int n_tiles = (int)tiles.tiles.size();

    std::vector<VhdItem> items;
    std::vector<int32_t> lag_of;
    vhd_items(windows, W, F, stride, wb, we, items, lag_of);

    // ---- path selection ----
    const bool lds_fits = (size_t)S * nbins <= (size_t)AMOF_MAX_LDS_BINS;
    // pairs one workgroup adds to a counter per origin: 256 centres x N partners x (1 + images); u32 counters in LDS
    const double per_origin = (double)VHD_THREADS * (double)N * (double)(1 + max_img);
    const bool force_global = getenv("AMOF_VANHOVE_DISTINCT_GLOBAL") != nullptr;
    const bool global = force_global || !lds_fits || per_origin > 4294967295.0;
    const int opc_max = (int)std::max<double>(1.0, std::min<double>(VHD_OPC, floor(4294967295.0 / per_origin)));
    // the fast path's error bound: f32 chain (guard_math.h, as the RDF tile kernels) + the 2^-32 grid
    const double *c0 = t->cell;
    const double csum = sqrt(c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2]) + sqrt(c0[3] * c0[3] + c0[4] * c0[4] + c0[5] * c0[5]) +
                        sqrt(c0[6] * c0[6] + c0[7] * c0[7] + c0[8] * c0[8]);
    const double guard_m = csum * (1.0 / 2147483648.0) / dr + (double)nbins * 1e-12;
    const double guard_f = (double)nbins * fast_guard_rel_rdf(geom.all_ortho, t->cell, t->n_cells) + guard_m;
    bool tile = !global && !getenv("AMOF_VANHOVE_DISTINCT_EXACT") && t->n_cells == 1 && geom.all_ortho && max_img == 0 &&
                t->pbc[0] && t->pbc[1] && t->pbc[2] && guard_f < 0.25;
    // origins per workgroup: enough workgroups to fill the GPU several times over
    const int opc = (int)std::max<int64_t>(1, std::min<int64_t>(opc_max, (int64_t)items.size() * n_tiles / 2048));

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    void *d_H = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_OUT1, hsize * sizeof(uint64_t), &d_H));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_H, 0, hsize * sizeof(uint64_t), ctx->stream));

    VhdArgs a;
    memset(&a, 0, sizeof a);
    a.pos = pos_dev;
    a.hist = (unsigned long long *)d_H;
    a.N = N;
    a.n_cells = (int32_t)t->n_cells;
    a.S = S;
    a.W = W;
    a.nbins = nbins;
    a.max_img = max_img;
    a.n_tiles = n_tiles;
    a.rmax2 = rmax * rmax;
    a.dr = dr;

    bool done = false;
    if (tile) {
        // frames quantised in batches of at most FB slots (bounded scratch): items in work order, a batch closes when its
        // frames would need more slots; inside a batch the frames are quantised in ascending order, runs of consecutive
        // frames by one launch
        const int64_t FB = std::max<int64_t>(2, std::min<int64_t>(32768, ((int64_t)1 << 30) / (N * (int64_t)sizeof(QAtom))));
        std::vector<std::pair<size_t, size_t>> batches;                 // item ranges
        std::vector<std::vector<int32_t>> bframes;                     // their frames, ascending
        {
            std::map<int32_t, int32_t> slot;
            size_t b0 = 0;
            auto close = [&](size_t b1) {
                std::vector<int32_t> fr;
                int32_t s = 0;
                for (auto &kv : slot) { kv.second = s++; fr.push_back(kv.first); }
                for (size_t i = b0; i < b1; i++) { items[i].sk = slot[items[i].k]; items[i].skm = slot[items[i].km]; }
                batches.push_back(std::make_pair(b0, b1));
                bframes.push_back(fr);
                slot.clear();
                b0 = b1;
            };
            for (size_t i = 0; i < items.size(); i++) {
                const int64_t extra = (slot.count(items[i].k) ? 0 : 1) + (items[i].km != items[i].k && !slot.count(items[i].km) ? 1 : 0);
                if ((int64_t)slot.size() + extra > FB) close(i);
                slot[items[i].k] = 0;
                slot[items[i].km] = 0;
            }
            close(items.size());
        }
        std::vector<VhdChunk> chunks;
        std::vector<size_t> bchunk(batches.size() + 1, 0);
        for (size_t b = 0; b < batches.size(); b++) {
            vhd_chunks(lag_of, batches[b].first, batches[b].second, opc, chunks);
            bchunk[b + 1] = chunks.size();
        }
        int64_t slots = 0;
        for (auto &fr : bframes) slots = std::max<int64_t>(slots, (int64_t)fr.size());

        UploadPack pk;
        const int i_geom = pk.add(geom.rec.data(), geom.rec.size() * sizeof(double));
        const int i_perm = pk.add(tiles.perm.data(), tiles.perm.size() * sizeof(int32_t));
        const int i_tiles = pk.add(tiles.tiles.data(), tiles.tiles.size() * sizeof(Tile));
        const int i_spf = pk.add(tiles.sp_first.data(), tiles.sp_first.size() * sizeof(int64_t));
        const int i_items = pk.add(items.data(), items.size() * sizeof(VhdItem));
        const int i_chunks = pk.add(chunks.data(), chunks.size() * sizeof(VhdChunk));
        AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
        void *d_Q, *d_flag;
        AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)slots * N * sizeof(QAtom), &d_Q));
        AMOF_TRY(ensure(ctx, SLOT_FLAGS, sizeof(int32_t), &d_flag));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flag, 0, sizeof(int32_t), ctx->stream));
        a.geom = pk.ptr<double>(i_geom);
        a.perm = pk.ptr<int32_t>(i_perm);
        a.tiles = pk.ptr<Tile>(i_tiles);
        a.items = pk.ptr<VhdItem>(i_items);
        a.Q = (const QAtom *)d_Q;
        for (int c = 0; c < 3; c++) {
            const double sc = geom.rec[4 * c] * (1.0 / 4294967296.0) / dr;
            a.sc2[c] = (float)(sc * sc);
        }
        const GuardThresholds thr = guard_thresholds(nbins, guard_f);
        a.half_m_guard = thr.half_m_guard;
        a.nb_hi = thr.nb_hi;
        const size_t lds = VHD_THREADS * sizeof(uint4) + (size_t)S * nbins * sizeof(unsigned);
        AMOF_HIP_TRY(ctx, allow_max_lds((const void *)rdf_distinct_tile_kernel));
        int64_t launches = 0;
        for (size_t b = 0; b < batches.size(); b++) {
            const std::vector<int32_t> &fr = bframes[b];
            for (size_t r = 0; r < fr.size();) {
                size_t e = r + 1;
                while (e < fr.size() && fr[e] == fr[e - 1] + 1 && e - r < 65535) e++;
                AMOF_TRY(launch_quantize(ctx, pos_dev, a.geom, 1, a.perm, pk.ptr<int64_t>(i_spf), S, N, fr[r], (int)(e - r), 2,
                                         (QAtom *)d_Q + r * (size_t)N, nullptr, (int32_t *)d_flag, 0, 1));
                r = e;
            }
            const size_t nch = bchunk[b + 1] - bchunk[b];
            if (!nch) continue;
            a.chunks = pk.ptr<VhdChunk>(i_chunks) + bchunk[b];
            if (launches == 0) timing_dom_begin(ctx, "rdf_distinct_tile");
            hipLaunchKernelGGL(rdf_distinct_tile_kernel, dim3((unsigned)nch, (unsigned)n_tiles), dim3(VHD_THREADS), lds, ctx->stream, a);
            AMOF_HIP_TRY(ctx, hipGetLastError());
            launches++;
        }
        timing_dom_end(ctx, launches);
        int32_t flag = 0;
        AMOF_TRY(fetch(ctx, &flag, d_flag, sizeof flag));
        AMOF_HIP_TRY(ctx, sync_stream(ctx));
        if (flag) AMOF_HIP_TRY(ctx, hipMemsetAsync(d_H, 0, hsize * sizeof(uint64_t), ctx->stream));   // atoms > 1e4 cells out
        else done = true;
    }
    if (!done) {
        std::vector<VhdChunk> chunks;
        vhd_chunks(lag_of, 0, items.size(), global ? VHD_OPC : opc, chunks);
        UploadPack pk;
        const int i_geom = pk.add(geom.rec.data(), geom.rec.size() * sizeof(double));
        const int i_img = pk.add(img.data(), img.size() * sizeof(double));
        const int i_nimg = pk.add(nimg.data(), nimg.size() * sizeof(int32_t));
        const int i_perm = pk.add(tiles.perm.data(), tiles.perm.size() * sizeof(int32_t));
        const int i_tiles = pk.add(tiles.tiles.data(), tiles.tiles.size() * sizeof(Tile));
        const int i_items = pk.add(items.data(), items.size() * sizeof(VhdItem));
        const int i_chunks = pk.add(chunks.data(), chunks.size() * sizeof(VhdChunk));
        AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
        a.geom = pk.ptr<double>(i_geom);
        a.img = pk.ptr<double>(i_img);
        a.nimg = pk.ptr<int32_t>(i_nimg);
        a.perm = pk.ptr<int32_t>(i_perm);
        a.tiles = pk.ptr<Tile>(i_tiles);
        a.items = pk.ptr<VhdItem>(i_items);
        a.chunks = pk.ptr<VhdChunk>(i_chunks);
        const bool ortho = geom.all_ortho, extra = max_img > 0;
        const dim3 grid((unsigned)chunks.size(), (unsigned)n_tiles);
        const size_t lds = VHD_THREADS * (3 * sizeof(double) + sizeof(int32_t)) + (global ? 0 : (size_t)S * nbins * sizeof(unsigned));
        auto launch = [&](auto kern) -> hipError_t {
            hipError_t e = allow_max_lds((const void *)kern);
            if (e != hipSuccess) return e;
            hipLaunchKernelGGL(kern, grid, dim3(VHD_THREADS), lds, ctx->stream, a);
            return hipGetLastError();
        };
        timing_dom_begin(ctx, global ? "rdf_distinct_exact_global" : "rdf_distinct_exact");
        hipError_t e;
        if (global) {
            if (ortho && !extra) e = launch(rdf_distinct_exact_kernel<true, false, true>);
            else if (ortho) e = launch(rdf_distinct_exact_kernel<true, true, true>);
            else if (!extra) e = launch(rdf_distinct_exact_kernel<false, false, true>);
            else e = launch(rdf_distinct_exact_kernel<false, true, true>);
        } else {
            if (ortho && !extra) e = launch(rdf_distinct_exact_kernel<true, false, false>);
            else if (ortho) e = launch(rdf_distinct_exact_kernel<true, true, false>);
            else if (!extra) e = launch(rdf_distinct_exact_kernel<false, false, false>);
            else e = launch(rdf_distinct_exact_kernel<false, true, false>);
        }
        AMOF_HIP_TRY(ctx, e);
        timing_dom_end(ctx, 1);
    }
    if (hist_dev) AMOF_TRY(add_into(ctx, hist_dev, (const uint64_t *)d_H, hsize));
    timing_end(ctx);
    if (hist) AMOF_TRY(fetch(ctx, hist, d_H, hsize * sizeof(uint64_t)));
    // host tables above live on this stack frame: finish before returning
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_vanhove_distinct(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                                     int64_t origin_stride, int64_t work_begin, int64_t work_end, double rmax, int32_t nbins,
                                     uint64_t *hist)
{
    if (!ctx) return AMOF_EINVAL;
    if (!hist) return fail(ctx, AMOF_EINVAL, "hist is NULL");
    return vhd_run(ctx, traj, windows, n_windows, origin_stride, work_begin, work_end, rmax, nbins, hist, nullptr);
}

extern "C" int amof_vanhove_distinct_dev(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                                         int64_t origin_stride, int64_t work_begin, int64_t work_end, double rmax, int32_t nbins,
                                         uint64_t *hist_dev)
{
    if (!ctx) return AMOF_EINVAL;
    if (!hist_dev) return fail(ctx, AMOF_EINVAL, "hist is NULL");
    return vhd_run(ctx, traj, windows, n_windows, origin_stride, work_begin, work_end, rmax, nbins, nullptr, hist_dev);
}
