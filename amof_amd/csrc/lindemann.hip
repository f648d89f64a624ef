// Lindemann index: the relative root-mean-square fluctuation of the length of neighbour pairs, per block of frames (gfx950).
//
// The definition stands in include/amof_hip.h (amof_lindemann); the per-pair arithmetic -- chunk order, delta, fixed-point
// term, bin rule, scale -- in lindemann_math.h, which the host test driver compiles too.  Stages of a call, one set at a time:
//   the pair table       bond.hip's list -> row count -> compaction stage (bond_pairs.h) over the block-start frames b S
//                        (select 0) or over frame 0 alone (select 1): a superset of the pairs bonded there, sorted by centre,
//                        in groups of at most AMOF_BOND_PAIR_BUDGET pairs, so that no table grows with N^2
//   lindemann_moments_kernel   "lindemann_chunk": a lane owns a (pair, block, chunk of 64 frames); the 64 lanes of a wave hold 64
//                        consecutive pairs of the table, so within a frame a wave reads neighbouring atoms.  The lane recomputes
//                        c = d(block start), walks its frames and writes the chunk's (p1, p2) into part [block][chunk][2][P];
//                        the lane of chunk 0 also writes c and the pair's h bit of the block (strict sqrt(d2) < rc in the
//                        canonical float64 arithmetic, at the block start or at frame 0).  Pairs and blocks are chunked so that
//                        part stays within 256 MB (LIND_PART_BYTES).
//   lindemann_reduce_kernel    a lane owns a (pair, block): the partials added in chunk order, delta, the term and the bin; an
//                        integer histogram in LDS (u32, up to LIND_LDS_BINS bins; beyond: u64 atomics in device memory), the
//                        pair count and the sum of terms reduced over the wave by shuffles into u64 LDS counters, one global
//                        u64 atomic per counter and workgroup (bond_reorient_kernel's pattern).  per_atom rows by int64 global
//                        atomics: the pairs of a centre are neighbours in the table, a few per wave.
//   lindemann_simple_kernel    "lindemann_simple" (AMOF_LINDEMANN_SIMPLE=1): a lane owns a (pair, block) and walks all its frames
//                        in the same chunk order, then the reduce kernel's tail: the cross-check inside the binary, same bits.
// Stage spans: 0 the pair lists, 1 the moments (on "lindemann_simple" the whole kernel), 2 the reduction.
// LDS: the reduce and simple kernels 16 B + 4 B per bin (<= 32 KB + 16 B); the moments kernel none.  No kernel spills, none uses
// scratch memory (checked with -Rpass-analysis=kernel-resource-usage, both ORTHO instantiations).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "bond_pairs.h"
#include "lindemann_math.h"
#include "nbr_check.h"

namespace amof {
namespace {

constexpr int LM_THREADS = 256;         // moments: four waves, four chunks of one tile of 64 pairs
constexpr int LR_THREADS = 256;         // reduce and simple: a pair per lane
constexpr int LIND_LDS_BINS = 8192;     // bins of the LDS histogram
constexpr size_t LIND_PART_BYTES = (size_t)256 << 20;   // partials of a chunk of pairs and blocks

struct LindArgs {
    const double *pos;
    const double *geom;
    const int2 *pairs;                  // this chunk's pairs
    double *part;                       // [nbg][nchunk][2][P]
    double *c0;                         // [nbg][P] d(block start)
    uint8_t *hbit;                      // [nbg][P]
    unsigned long long *sums;           // [nb][n_sets][2] of the call
    unsigned long long *hist;           // [nb][n_sets][nbins] of the call
    unsigned long long *per_atom;       // [nb][N][2] of this set, or NULL
    int64_t N, B, S;
    int32_t P, nchunk, n_cells, b0, nbg, select, nbins, n_sets, set, e, lds_bins;
    double rc, ddelta;
};

// the canonical minimum-image distance of the pair in frame f's cell
template <bool ORTHO>
__device__ __forceinline__ double lind_dist(const LindArgs &a, int64_t f, int i, int j)
{
    const double *__restrict__ pi = a.pos + ((size_t)f * (size_t)a.N + (size_t)i) * 3;
    const double *__restrict__ pj = a.pos + ((size_t)f * (size_t)a.N + (size_t)j) * 3;
    const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    double dx, dy, dz;
    pair_base<ORTHO>(g, pj[0] - pi[0], pj[1] - pi[1], pj[2] - pi[2], dx, dy, dz);
    return sqrt(norm2(dx, dy, dz));
}

// a lane owns a pair of tile blockIdx.x, the wave chunk blockIdx.y * 4 + wave of block b0 + blockIdx.z
template <bool ORTHO>
__global__ __launch_bounds__(LM_THREADS) void lindemann_moments_kernel(LindArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = blockIdx.x * 64 + lane;
    const int k = blockIdx.y * (LM_THREADS / 64) + wave;
    const int bl = blockIdx.z;
    if (k >= a.nchunk || p >= a.P) return;
    const int2 ij = a.pairs[p];
    const int64_t start = (int64_t)(a.b0 + bl) * a.S;
    const double c = lind_dist<ORTHO>(a, start, ij.x, ij.y);
    double p1, p2;
    lindemann::chunk_partial([&](int64_t f) { return lind_dist<ORTHO>(a, start + f, ij.x, ij.y); }, c, k, a.B, p1, p2);
    const size_t P = (size_t)a.P;
    double *__restrict__ o = a.part + ((size_t)bl * a.nchunk + k) * 2 * P + p;
    o[0] = p1;
    o[P] = p2;
    if (k == 0) {
        const double dh = a.select ? lind_dist<ORTHO>(a, 0, ij.x, ij.y) : c;
        a.c0[(size_t)bl * P + p] = c;
        a.hbit[(size_t)bl * P + p] = dh < a.rc ? 1 : 0;
    }
}

// LDS of the reduce and simple kernels: two u64 counters, then lds_bins u32 bins
__device__ __forceinline__ void lind_lds_init(const LindArgs &a, unsigned long long *lc, unsigned *lh)
{
    const int tid = threadIdx.x;
    if (tid < 2) lc[tid] = 0ull;
    for (int k = tid; k < a.lds_bins; k += LR_THREADS) lh[k] = 0u;
    __syncthreads();
}

// what a (pair, block) adds, by every lane of the workgroup (has: the pair is bonded in block b0 + bl; dl: its delta)
__device__ __forceinline__ void lind_tail(const LindArgs &a, int bl, bool has, int centre, double dl, unsigned long long *lc, unsigned *lh)
{
    const int tid = threadIdx.x, lane = tid & 63;
    const size_t b = (size_t)(a.b0 + bl);
    unsigned long long *__restrict__ gh = a.hist + (b * a.n_sets + a.set) * (size_t)a.nbins;
    unsigned n = 0;
    long long term = 0;
    if (has) {
        n = 1;
        term = lindemann::fixed_term(dl, a.e);
        const int bin = lindemann::bin_of(dl, a.ddelta, a.nbins);
        if (a.lds_bins) atomicAdd(&lh[bin], 1u);
        else atomicAdd(&gh[bin], 1ull);
        if (a.per_atom) {
            unsigned long long *__restrict__ pa = a.per_atom + (b * (size_t)a.N + (size_t)centre) * 2;
            atomicAdd(&pa[0], 1ull);
            atomicAdd(&pa[1], (unsigned long long)term);
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_down(n, off, 64);
        term += __shfl_down(term, off, 64);
    }
    if (lane == 0 && n) {
        atomicAdd(&lc[0], (unsigned long long)n);
        atomicAdd(&lc[1], (unsigned long long)term);
    }
    __syncthreads();
    if (tid < 2 && lc[0]) atomicAdd(&a.sums[(b * a.n_sets + a.set) * 2 + tid], lc[tid]);
    for (int k = tid; k < a.lds_bins; k += LR_THREADS) {
        const unsigned v = lh[k];
        if (v) atomicAdd(&gh[k], (unsigned long long)v);
    }
}

// a lane owns pair blockIdx.x * 256 + tid of block b0 + blockIdx.y
__global__ __launch_bounds__(LR_THREADS) void lindemann_reduce_kernel(LindArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long *lc = reinterpret_cast<unsigned long long *>(lds_raw);
    unsigned *lh = reinterpret_cast<unsigned *>(lc + 2);
    lind_lds_init(a, lc, lh);
    const int p = blockIdx.x * LR_THREADS + threadIdx.x;
    const int bl = blockIdx.y;
    const size_t P = (size_t)a.P;
    const bool has = p < a.P && a.hbit[(size_t)bl * P + p] != 0;
    double dl = 0.0;
    int centre = 0;
    if (has) {
        centre = a.pairs[p].x;
        const double *__restrict__ q = a.part + (size_t)bl * a.nchunk * 2 * P + p;
        double S1 = 0.0, S2 = 0.0;
        for (int k = 0; k < a.nchunk; k++) {
            S1 += q[(size_t)k * 2 * P];
            S2 += q[((size_t)k * 2 + 1) * P];
        }
        dl = lindemann::delta(a.c0[(size_t)bl * P + p], S1, S2, a.B);
    }
    lind_tail(a, bl, has, centre, dl, lc, lh);
}

// the same result without the partials: a lane walks every frame of its (pair, block)
template <bool ORTHO>
__global__ __launch_bounds__(LR_THREADS) void lindemann_simple_kernel(LindArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long *lc = reinterpret_cast<unsigned long long *>(lds_raw);
    unsigned *lh = reinterpret_cast<unsigned *>(lc + 2);
    lind_lds_init(a, lc, lh);
    const int p = blockIdx.x * LR_THREADS + threadIdx.x;
    const int bl = blockIdx.y;
    bool has = false;
    double dl = 0.0;
    int centre = 0;
    if (p < a.P) {
        const int2 ij = a.pairs[p];
        centre = ij.x;
        const int64_t start = (int64_t)(a.b0 + bl) * a.S;
        const double c = lind_dist<ORTHO>(a, start, ij.x, ij.y);
        const double dh = a.select ? lind_dist<ORTHO>(a, 0, ij.x, ij.y) : c;
        has = dh < a.rc;
        if (has) {
            double S1, S2;
            lindemann::block_sums([&](int64_t f) { return lind_dist<ORTHO>(a, start + f, ij.x, ij.y); }, c, a.B, S1, S2);
            dl = lindemann::delta(c, S1, S2, a.B);
        }
    }
    lind_tail(a, bl, has, centre, dl, lc, lh);
}

struct LindOut {
    int64_t *sums;          // host [nb][n_sets][2], overwritten, or NULL
    uint64_t *hist;         // host [nb][n_sets][nbins], overwritten, or NULL
    int64_t *sums_dev;      // device, added into, or NULL
    uint64_t *hist_dev;
    int64_t *per_atom;      // host [nb][n_sets][N][2] or NULL
    int32_t *scale_log2;    // host [n_sets]
};

int lindemann_run(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets, int64_t block,
                  int64_t block_stride, int32_t select, int32_t nbins, double ddelta, int64_t atom_begin, int64_t atom_end,
                  const LindOut &out)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    const int S = t->n_species;
    const int64_t N = t->n_atoms, F = t->n_frames;
    if (!cutoff || n_sets < 0 || (n_sets > 0 && !sets)) return fail(ctx, AMOF_EINVAL, "NULL argument");
    if (block < 2 || block > F) return fail(ctx, AMOF_EINVAL, "block of %lld frames outside 2..%lld", (long long)block, (long long)F);
    if (block_stride < 1) return fail(ctx, AMOF_EINVAL, "block_stride must be at least 1");
    if (select != 0 && select != 1) return fail(ctx, AMOF_EINVAL, "select must be 0 (block) or 1 (first)");
    if (nbins < 1) return fail(ctx, AMOF_EINVAL, "nbins must be at least 1");
    if (!(ddelta > 0.0) || !isfinite(ddelta)) return fail(ctx, AMOF_EINVAL, "ddelta must be positive and finite");
    if (atom_begin < 0 || atom_end > N || atom_begin > atom_end)
        return fail(ctx, AMOF_EINVAL, "atom range [%lld, %lld) outside [0, %lld)", (long long)atom_begin, (long long)atom_end, (long long)N);
    const int64_t B = block, nb = lindemann::block_count(F, B, block_stride);
    const int nchunk = lindemann::chunk_count(B);
    if (nb > 0x7fffffffLL || (nchunk + 3) / 4 > 65535) return fail(ctx, AMOF_EINVAL, "too many frames");
    for (int s = 0; s < n_sets; s++) {
        AMOF_TRY(pore_refuse(ctx, nbr_check::bond_set_species(sets, s, S)));
        AMOF_TRY(pore_refuse(ctx, nbr_check::bond_set_cutoff(cutoff[sets[2 * s] * S + sets[2 * s + 1]], s)));
    }
    const size_t n_sums = (size_t)nb * n_sets * 2, n_hist = (size_t)nb * n_sets * (size_t)nbins;
    const size_t n_pa = out.per_atom ? (size_t)nb * n_sets * (size_t)N * 2 : 0;
    auto zero_host = [&]() {
        if (out.sums) std::fill(out.sums, out.sums + n_sums, (int64_t)0);
        if (out.hist) std::fill(out.hist, out.hist + n_hist, (uint64_t)0);
        if (out.per_atom) std::fill(out.per_atom, out.per_atom + n_pa, (int64_t)0);
    };
    zero_host();
    // the scale depends on the trajectory, the set and the block length alone: never on the atom range or the chunking
    std::vector<int64_t> nsp((size_t)S, 0);
    for (int64_t i = 0; i < N; i++) nsp[(size_t)t->species[i]]++;
    for (int s = 0; s < n_sets; s++) {
        const int e = lindemann::scale_log2(nsp[(size_t)sets[2 * s]], nsp[(size_t)sets[2 * s + 1]], B);
        if (e < lindemann::SCALE_MIN)
            return fail(ctx, AMOF_EINVAL, "set %d: %lld x %lld pairs in blocks of %lld frames leave a fixed-point quantum above 2^-20", s,
                        (long long)nsp[(size_t)sets[2 * s]], (long long)nsp[(size_t)sets[2 * s + 1]], (long long)B);
        out.scale_log2[s] = e;
    }
    if (n_sets == 0) return AMOF_OK;

    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    const double hmin = nbr_check::min_periodic_height(t->pbc, geom.rec.data(), t->n_cells);
    for (int s = 0; s < n_sets; s++)
        AMOF_TRY(pore_refuse(ctx, nbr_check::half_height_set(cutoff[sets[2 * s] * S + sets[2 * s + 1]], s, hmin, "a pair could be bonded twice")));
    HostTiles tiles;
    build_tiles(t, BOND_LIST_TILE, tiles);

    const char *env_simple = getenv("AMOF_LINDEMANN_SIMPLE");
    const bool simple = env_simple && env_simple[0] == '1';
    const char *path = simple ? "lindemann_simple" : "lindemann_chunk";
    const bool ortho = geom.all_ortho;
    // AMOF_LINDEMANN_SCRATCH (bytes) is for the tests alone: it shrinks the budget so that small inputs reach the chunking of pairs
    // and blocks below.  It is no part of the interface.
    size_t part_bytes = LIND_PART_BYTES;
    if (const char *e = getenv("AMOF_LINDEMANN_SCRATCH")) {
        const long long v = atoll(e);
        if (v > 0) part_bytes = (size_t)v;
    }
    // pairs and blocks of a launch: the partials [blocks][nchunk][2][pairs] within part_bytes; 64 pairs and one block at least
    const size_t per_pb = (size_t)nchunk * 2 * sizeof(double);
    int64_t nbg_max = std::min<int64_t>(nb, 65535);
    size_t pc_max = (size_t)1 << 24;
    if (!simple) {
        pc_max = std::min<size_t>(pc_max, part_bytes / (per_pb * (size_t)nbg_max) / 64 * 64);
        if (pc_max < 64) {
            pc_max = 64;
            nbg_max = std::max<int64_t>(1, std::min<int64_t>(nbg_max, (int64_t)(part_bytes / (per_pb * 64))));
        }
    }
    const int lds_bins = nbins <= LIND_LDS_BINS ? nbins : 0;
    const size_t lds = 2 * sizeof(unsigned long long) + (size_t)lds_bins * sizeof(unsigned);

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    StageSpans spans(ctx);      // lists, moments, reduction
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(geom.rec.data(), geom.rec.size() * sizeof(double));
    const int i_perm = pk.add(tiles.perm.data(), tiles.perm.size() * sizeof(int32_t));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    void *d_sums = nullptr, *d_hist = nullptr, *d_pa = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_OUT0, n_sums * sizeof(uint64_t), &d_sums));
    AMOF_TRY(ensure(ctx, SLOT_OUT1, n_hist * sizeof(uint64_t), &d_hist));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_sums, 0, n_sums * sizeof(uint64_t), ctx->stream));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(d_hist, 0, n_hist * sizeof(uint64_t), ctx->stream));
    const size_t pa_set = (size_t)nb * (size_t)N * 2;      // per_atom words of one set
    std::vector<int64_t> pa_host;
    if (out.per_atom) {
        AMOF_TRY(ensure(ctx, SLOT_AUX7, pa_set * sizeof(int64_t), &d_pa));
        pa_host.resize(pa_set);
    }
    ctx->last_path = path;

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
    pc.first_frame = 0;
    pc.stride = select ? 1 : block_stride;
    pc.n_origins = select ? 1 : nb;
    pc.pair_max = bond_pair_budget();

    LindArgs la;
    memset(&la, 0, sizeof la);
    la.pos = pos_dev;
    la.geom = pk.ptr<double>(i_geom);
    la.sums = (unsigned long long *)d_sums;
    la.hist = (unsigned long long *)d_hist;
    la.per_atom = (unsigned long long *)d_pa;
    la.N = N;
    la.B = B;
    la.S = block_stride;
    la.nchunk = nchunk;
    la.n_cells = (int32_t)t->n_cells;
    la.select = select;
    la.nbins = nbins;
    la.n_sets = n_sets;
    la.ddelta = ddelta;
    la.lds_bins = lds_bins;
    int64_t launches = 0;

    for (int s = 0; s < n_sets; s++) {
        const int A = sets[2 * s], Bs = sets[2 * s + 1];
        const double rc = cutoff[A * S + Bs];
        la.set = s;
        la.e = out.scale_log2[s];
        la.rc = rc;
        if (out.per_atom) AMOF_HIP_TRY(ctx, hipMemsetAsync(d_pa, 0, pa_set * sizeof(int64_t), ctx->stream));
        AMOF_TRY(bond_pair_groups(pc, s, A, Bs, rc, atom_begin, atom_end, [&](const int2 *d_pairs, size_t P) -> int {
            for (size_t p0 = 0; p0 < P; p0 += pc_max) {
                const int Pc = (int)std::min(pc_max, P - p0);
                la.pairs = d_pairs + p0;
                la.P = Pc;
                for (int64_t b0 = 0; b0 < nb; b0 += nbg_max) {
                    const int nbg = (int)std::min<int64_t>(nbg_max, nb - b0);
                    la.b0 = (int32_t)b0;
                    la.nbg = nbg;
                    const dim3 rgrid((unsigned)((Pc + LR_THREADS - 1) / LR_THREADS), (unsigned)nbg);
                    spans.begin(1);
                    if (launches == 0) timing_dom_begin(ctx, path);
                    if (simple) {
                        AMOF_HIP_TRY(ctx, with_flag(ortho, [&](auto O) {
                            return launch_lds(lindemann_simple_kernel<O()>, rgrid, dim3(LR_THREADS), lds, ctx->stream, la);
                        }));
                    } else {
                        void *d_part = nullptr, *d_c0 = nullptr, *d_h = nullptr;
                        AMOF_TRY(ensure(ctx, SLOT_AUX4, (size_t)nbg * per_pb * Pc, &d_part));
                        AMOF_TRY(ensure(ctx, SLOT_AUX5, (size_t)nbg * Pc * sizeof(double), &d_c0));
                        AMOF_TRY(ensure(ctx, SLOT_AUX6, (size_t)nbg * Pc, &d_h));
                        la.part = (double *)d_part;
                        la.c0 = (double *)d_c0;
                        la.hbit = (uint8_t *)d_h;
                        const dim3 mgrid((unsigned)((Pc + 63) / 64), (unsigned)((nchunk + 3) / 4), (unsigned)nbg);
                        AMOF_HIP_TRY(ctx, with_flag(ortho, [&](auto O) {
                            return launch_lds(lindemann_moments_kernel<O()>, mgrid, dim3(LM_THREADS), 0, ctx->stream, la);
                        }));
                    }
                    launches++;
                    timing_dom_end(ctx, launches);
                    spans.end();
                    if (!simple) {
                        spans.begin(2);
                        AMOF_HIP_TRY(ctx, launch_lds(lindemann_reduce_kernel, rgrid, dim3(LR_THREADS), lds, ctx->stream, la));
                        spans.end();
                    }
                }
            }
            return AMOF_OK;
        }));
        if (out.per_atom) {
            // rows of this set: [nb][N][2] on the device, [nb][n_sets][N][2] in the caller's array
            AMOF_TRY(fetch(ctx, pa_host.data(), d_pa, pa_set * sizeof(int64_t)));
            for (int64_t b = 0; b < nb; b++)
                memcpy(out.per_atom + (((size_t)b * n_sets + s) * (size_t)N) * 2, pa_host.data() + (size_t)b * (size_t)N * 2,
                       (size_t)N * 2 * sizeof(int64_t));
        }
    }
    timing_end(ctx);
    if (out.sums_dev) AMOF_TRY(add_into(ctx, (uint64_t *)out.sums_dev, (const uint64_t *)d_sums, n_sums));
    if (out.hist_dev) AMOF_TRY(add_into(ctx, out.hist_dev, (const uint64_t *)d_hist, n_hist));
    if (out.sums) AMOF_TRY(fetch(ctx, out.sums, d_sums, n_sums * sizeof(int64_t)));
    if (out.hist) AMOF_TRY(fetch(ctx, out.hist, d_hist, n_hist * sizeof(uint64_t)));
    // host tables above live on this stack frame: finish before returning
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    return AMOF_OK;
}

// the host outputs hold zeros after an error
int lindemann_call(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *sets, int32_t n_sets, int64_t block,
                   int64_t block_stride, int32_t select, int32_t nbins, double ddelta, int64_t atom_begin, int64_t atom_end,
                   const LindOut &out)
{
    const int rc = lindemann_run(ctx, t, cutoff, sets, n_sets, block, block_stride, select, nbins, ddelta, atom_begin, atom_end, out);
    if (rc != AMOF_OK && t && n_sets > 0 && nbins >= 1 && block >= 2 && block <= t->n_frames && block_stride >= 1) {
        const size_t nb = (size_t)lindemann::block_count(t->n_frames, block, block_stride);
        if (out.sums) std::fill(out.sums, out.sums + nb * n_sets * 2, (int64_t)0);
        if (out.hist) std::fill(out.hist, out.hist + nb * n_sets * (size_t)nbins, (uint64_t)0);
        if (out.per_atom && t->n_atoms > 0) std::fill(out.per_atom, out.per_atom + nb * n_sets * (size_t)t->n_atoms * 2, (int64_t)0);
    }
    return rc;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_lindemann(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                              int64_t block, int64_t block_stride, int32_t select, int32_t nbins, double ddelta, int64_t atom_begin,
                              int64_t atom_end, int64_t *sums, uint64_t *hist, int64_t *per_atom, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!sums || !hist || !scale_log2) return fail(ctx, AMOF_EINVAL, "sums, hist or scale_log2 is NULL");
    const LindOut out = {sums, hist, nullptr, nullptr, per_atom, scale_log2};
    return lindemann_call(ctx, traj, cutoff, sets, n_sets, block, block_stride, select, nbins, ddelta, atom_begin, atom_end, out);
}

extern "C" int amof_lindemann_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                  int64_t block, int64_t block_stride, int32_t select, int32_t nbins, double ddelta, int64_t atom_begin,
                                  int64_t atom_end, int64_t *sums_dev, uint64_t *hist_dev, int64_t *per_atom, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!sums_dev || !hist_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "sums, hist or scale_log2 is NULL");
    const LindOut out = {nullptr, nullptr, sums_dev, hist_dev, per_atom, scale_log2};
    return lindemann_call(ctx, traj, cutoff, sets, n_sets, block, block_stride, select, nbins, ddelta, atom_begin, atom_end, out);
}
