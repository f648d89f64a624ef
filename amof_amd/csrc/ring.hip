// Primitive ring statistics of the bond network of every frame (include/amof_hip.h, amof_ring_stats).
// Replaces amof/ring/core.py, which writes every frame to disk and runs the external program RINGS on it.
//
// Stages of a batch of frames (a batch: as many frames as AMOF_RING_TABLE_MB admits distance tables for):
//   ring_adjacency_kernel   a centre per thread against partner tiles of 256 atoms through LDS: pair_base<ORTHO>, strict
//                           sqrt(d2) < rc of the species pair (amof_cn_count's decision), the partners in atom order, so the
//                           rows [frame][N][RING_MAX_DEGREE] come out sorted; a 17th neighbour flags the frame
//                           (launch_bond_rows, amof_internal.h: fragment.hip takes its rows from the same kernel)
//   ring_bfs_kernel         a wave per (frame, source): visited bitmap and ONE queue in LDS (the two frontiers are two ranges of
//                           it), levels <= K = nmax / 2 into the source's row of the u8 table D[frame][N][N] (preset to 255).
//                           Then the wave walks the nodes it reached and counts (pass 0) or writes (pass 1) the source's
//                           candidates (ring_search.h, even_candidate / odd_candidate); between the passes the host sums the counts into the
//                           offsets of the candidate buffer, which so has no fixed capacity.  Pass 0 also sets the truncated flag.
//   ring_search_kernel      a wave per (frame, source), after all rows of the batch exist: the source's level row in LDS, a
//                           candidate per lane, the two path stacks of a lane in LDS ([level][lane] u16), the cross checks from D
//                           in device memory; c[v][n] accumulates in LDS and is written once.  "ring_wave".
//   ring_simple_kernel      the cross-check variant, "ring_simple" (AMOF_RING_SIMPLE=1): a thread per (frame, source) runs
//                           ring_search.h's search_source -- it finds its candidates itself, reads no candidate buffer, keeps its
//                           stacks in private memory and uses no LDS.  Bit-identical outputs.
//   ring_reduce_kernel      a workgroup per frame: c -> counts[4][nmax + 1] and the truncated sources
// No loop waits on another workgroup; every loop is bounded by the levels (<= K), the queue (<= N entries: a node enters it
// once), the row length (<= RING_MAX_DEGREE) and the path cap (ring_search.h).
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no kernel spills, no scratch):
//   kernel                        VGPRs  SGPRs  static LDS  dynamic LDS                        waves / SIMD by registers
//   ring_adjacency_kernel<true>      48     38      7168 B  S S doubles                        8
//   ring_adjacency_kernel<false>     70     38      7168 B  S S doubles                        7
//   ring_bfs_kernel                  31     70         0    16 + N / 8 + 2 N B (21 KB at 9792) 8
//   ring_search_kernel               48     85         0    N + 4096 + 144 B (14 KB at 9792)   8
//   ring_simple_kernel               84     74         0    0                                  5
//   ring_reduce_kernel               18     50      1064 B  0                                  8
// The wave kernels run workgroups of one wave; at 9792 atoms the LDS admits 7 (BFS) and 11 (search) of them per CU, and at the
// 65535 atoms a u16 path can name the BFS workgroup takes 139 KB of the CU's 160 KB.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "amof_internal.h"
#include "nbr_check.h"
#include "ring_search.h"

namespace amof {
namespace {

constexpr int RA_THREADS = 256;         // ring_adjacency_kernel: a centre per thread, partner tiles of 256 atoms
constexpr int RR_THREADS = 256;         // ring_reduce_kernel
constexpr size_t RING_TABLE_BYTES = (size_t)1024 << 20;     // distance tables of a batch (AMOF_RING_TABLE_MB overrides)

struct RingArgs {
    const double *pos;          // [F][N][3] of the call
    const double *geom;
    const int32_t *species;     // [N]
    const double *cutoff;       // [S][S]
    int32_t *adj;               // [nf][N][RING_MAX_DEGREE]
    int32_t *deg;               // [nf][N]
    uint8_t *D;                 // [nf][N][N]
    uint32_t *ncand;            // [nf][N]
    const unsigned long long *cand_off;     // [nf][N]
    uint32_t *cand;
    uint8_t *open;              // [nf][N]: the source's BFS stopped in front of unvisited nodes
    uint32_t *c;                // [nf][N][nmax + 1]
    long long *counts;          // [nf][4][nmax + 1]
    long long *truncated;       // [nf]
    int32_t *flags;             // [0]: 1 + the first frame with a node of more than RING_MAX_DEGREE neighbours, [1]: 1 + the first
                                // frame with more than `cap` shortest paths to an end node (0: none)
    unsigned long long *stats;  // [0] candidates searched, [1] candidates that close a ring
    int32_t N, S, n_cells, f0, nf, nmax, K, cap;
};

template <bool ORTHO>
__global__ __launch_bounds__(RA_THREADS) void ring_adjacency_kernel(BondRows a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ra_smem[];
    double *rc = reinterpret_cast<double *>(ra_smem);               // [S][S]
    __shared__ double tx[RA_THREADS], ty[RA_THREADS], tz[RA_THREADS];
    __shared__ int ts[RA_THREADS];
    const int tid = threadIdx.x, fb = blockIdx.y, f = a.f0 + fb;
    const int i = blockIdx.x * RA_THREADS + tid;
    const bool has = i < a.N;
    for (int k = tid; k < a.S * a.S; k += RA_THREADS) rc[k] = a.cutoff[k];
    const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
    const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    const size_t ii = has ? (size_t)i : 0;
    const double xi = p[ii * 3 + 0], yi = p[ii * 3 + 1], zi = p[ii * 3 + 2];
    const int si = a.species[ii];
    int32_t *__restrict__ row = a.adj + ((size_t)fb * a.N + ii) * RING_MAX_DEGREE;
    int cnt = 0;
    for (int j0 = 0; j0 < a.N; j0 += RA_THREADS) {
        const int nj = min(RA_THREADS, a.N - j0);
        __syncthreads();
        if (tid < nj) {
            const size_t aj = (size_t)(j0 + tid);
            tx[tid] = p[aj * 3 + 0];
            ty[tid] = p[aj * 3 + 1];
            tz[tid] = p[aj * 3 + 2];
            ts[tid] = a.species[aj];
        }
        __syncthreads();
        if (!has) continue;
        for (int j = 0; j < nj; j++) {
            if (j0 + j == i) continue;
            double dx, dy, dz;
            pair_base<ORTHO>(g, tx[j] - xi, ty[j] - yi, tz[j] - zi, dx, dy, dz);
            if (sqrt(norm2(dx, dy, dz)) < rc[si * a.S + ts[j]]) {
                if (cnt < RING_MAX_DEGREE) row[cnt] = j0 + j;
                cnt++;
            }
        }
    }
    if (!has) return;
    for (int q = cnt; q < RING_MAX_DEGREE; q++) row[q] = -1;
    a.deg[(size_t)fb * a.N + ii] = min(cnt, RING_MAX_DEGREE);
    if (cnt > RING_MAX_DEGREE) flag_frame(a.flag, f);
}

}  // namespace

// the rows of frames [f0, f0 + nf) of a call, for amof_ring_stats and amof_fragment_stats (fragment.hip): the SAME kernel
int launch_bond_rows(amof_ctx *ctx, const BondRows &rows, bool ortho)
{
    AMOF_HIP_TRY(ctx, with_flag(ortho, [&](auto O) {
        return launch_lds(ring_adjacency_kernel<O()>, dim3((unsigned)((rows.N + RA_THREADS - 1) / RA_THREADS), (unsigned)rows.nf), dim3(RA_THREADS),
                          (size_t)rows.S * rows.S * sizeof(double), ctx->stream, rows);
    }));
    return AMOF_OK;
}

namespace {

// LDS of ring_bfs_kernel: 4 counters, the visited bitmap, the queue
__host__ __device__ inline size_t bfs_bitmap_words(int N) { return ((size_t)N + 31) / 32; }
__host__ __device__ inline size_t bfs_queue_off(int N) { return (16 + bfs_bitmap_words(N) * 4 + 15) & ~(size_t)15; }
inline size_t bfs_lds_bytes(int N) { return bfs_queue_off(N) + (((size_t)N * 2 + 15) & ~(size_t)15); }

__global__ __launch_bounds__(64) void ring_bfs_kernel(RingArgs a, int pass)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rb_smem[];
    unsigned *ctr = reinterpret_cast<unsigned *>(rb_smem);          // [0] queue tail, [1] candidates, [2] open
    unsigned *bitmap = ctr + 4;
    uint16_t *queue = reinterpret_cast<uint16_t *>(rb_smem + bfs_queue_off(a.N));
    const int lane = threadIdx.x;
    const int fb = blockIdx.x / a.N, v = blockIdx.x - fb * a.N;
    const int32_t *__restrict__ adj = a.adj + (size_t)fb * a.N * RING_MAX_DEGREE;
    const int32_t *__restrict__ deg = a.deg + (size_t)fb * a.N;
    uint8_t *Dframe = a.D + (size_t)fb * (size_t)a.N * (size_t)a.N;
    uint8_t *L = Dframe + (size_t)v * (size_t)a.N;
    const int words = (int)bfs_bitmap_words(a.N);
    for (int k = lane; k < words; k += 64) bitmap[k] = 0u;
    if (lane < 4) ctr[lane] = 0u;
    __syncthreads();
    if (lane == 0) {
        bitmap[v >> 5] = 1u << (v & 31);
        queue[0] = (uint16_t)v;
        ctr[0] = 1u;
        L[v] = 0;
    }
    __syncthreads();
    int lo = 0, hi = 1, level = 0;
    for (; level < a.K && lo < hi; level++) {
        for (int idx = lo + lane; idx < hi; idx += 64) {
            const int x = queue[idx];
            const int dx = deg[x];
            for (int q = 0; q < dx; q++) {
                const int u = adj[(size_t)x * RING_MAX_DEGREE + q];
                const unsigned bit = 1u << (u & 31);
                if (!(atomicOr(&bitmap[u >> 5], bit) & bit)) {
                    const unsigned slot = atomicAdd(&ctr[0], 1u);      // (< N: a node enters the queue once)
                    queue[slot] = (uint16_t)u;
                    L[u] = (uint8_t)(level + 1);
                }
            }
        }
        __syncthreads();
        lo = hi;
        hi = (int)ctr[0];
        __syncthreads();
    }
    // the rows are read back below (and by no other workgroup before the kernel ends)
    __threadfence_block();
    __syncthreads();
    const ring::Graph g{adj, deg, Dframe, a.N};
    if (pass == 0 && level == a.K) {
        // [lo, hi) is level K
        bool open = false;
        for (int idx = lo + lane; idx < hi; idx += 64) {
            const int x = queue[idx];
            const int dx = deg[x];
            for (int q = 0; q < dx; q++) {
                const int u = adj[(size_t)x * RING_MAX_DEGREE + q];
                if (!(bitmap[u >> 5] & (1u << (u & 31)))) open = true;
            }
        }
        if (open) ctr[2] = 1u;
    }
    const unsigned long long base = pass ? a.cand_off[blockIdx.x] : 0ull;
    for (int idx = 1 + lane; idx < hi; idx += 64) {
        const int x = queue[idx];
        const int dx = deg[x];
        const bool even = ring::even_candidate(g, L, x, a.nmax);
        int nc = even ? 1 : 0;
        for (int q = 0; q < dx; q++) nc += ring::odd_candidate(g, L, x, a.nmax, q) >= 0 ? 1 : 0;
        if (nc == 0) continue;
        const unsigned slot = atomicAdd(&ctr[1], (unsigned)nc);
        if (!pass) continue;
        uint32_t *dst = a.cand + base + slot;
        if (even) *dst++ = ring::pack_candidate(x, x);
        for (int q = 0; q < dx; q++) {
            const int u = ring::odd_candidate(g, L, x, a.nmax, q);
            if (u >= 0) *dst++ = ring::pack_candidate(x, u);
        }
    }
    __syncthreads();
    if (lane == 0 && pass == 0) {
        a.ncand[blockIdx.x] = ctr[1];
        a.open[blockIdx.x] = (uint8_t)ctr[2];
    }
}

// LDS of ring_search_kernel: the level row, the path stacks [2][RING_MAX_K][64] u16, nmax + 1 counters
__host__ __device__ inline size_t search_stack_off(int N) { return ((size_t)N + 15) & ~(size_t)15; }
__host__ __device__ inline size_t search_count_off(int N) { return search_stack_off(N) + 2 * RING_MAX_K * 64 * sizeof(uint16_t); }
inline size_t search_lds_bytes(int N) { return search_count_off(N) + (((size_t)(RING_MAX_SIZE + 1) * 4 + 15) & ~(size_t)15); }

__global__ __launch_bounds__(64) void ring_search_kernel(RingArgs a)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rs_smem[];
    uint8_t *L = rs_smem;
    uint16_t *P1 = reinterpret_cast<uint16_t *>(rs_smem + search_stack_off(a.N));
    uint16_t *P2 = P1 + RING_MAX_K * 64;
    unsigned *cnt = reinterpret_cast<unsigned *>(rs_smem + search_count_off(a.N));
    const int lane = threadIdx.x;
    const int fb = blockIdx.x / a.N, v = blockIdx.x - fb * a.N;
    const uint8_t *Dframe = a.D + (size_t)fb * (size_t)a.N * (size_t)a.N;
    const uint8_t *row = Dframe + (size_t)v * (size_t)a.N;
    if ((a.N & 3) == 0) {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(row);
        uint32_t *dst = reinterpret_cast<uint32_t *>(L);
        for (int k = lane; k < a.N / 4; k += 64) dst[k] = src[k];
    } else {
        for (int k = lane; k < a.N; k += 64) L[k] = row[k];
    }
    if (lane <= a.nmax) cnt[lane] = 0u;
    __syncthreads();
    const ring::Graph g{a.adj + (size_t)fb * a.N * RING_MAX_DEGREE, a.deg + (size_t)fb * a.N, Dframe, a.N};
    const unsigned long long c0 = a.cand_off[blockIdx.x], c1 = c0 + a.ncand[blockIdx.x];
    unsigned searched = 0, closed = 0;
    bool over = false;
    for (unsigned long long ci = c0 + lane; ci < c1; ci += 64) {
        int n = 0;
        const int r = ring::search_candidate(g, L, a.cand[ci], a.cap, P1 + lane, P2 + lane, 64, &n);
        searched++;
        if (r < 0) over = true;
        else if (r > 0) {
            atomicAdd(&cnt[n], (unsigned)r);
            closed++;
        }
    }
    if (over) flag_frame(&a.flags[1], a.f0 + fb);
    if (searched) atomicAdd(&a.stats[0], (unsigned long long)searched);
    if (closed) atomicAdd(&a.stats[1], (unsigned long long)closed);
    __syncthreads();
    if (lane <= a.nmax) a.c[(size_t)blockIdx.x * (a.nmax + 1) + lane] = cnt[lane];
}

__global__ __launch_bounds__(64) void ring_simple_kernel(RingArgs a)
{
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s >= (long long)a.nf * a.N) return;
    const int fb = (int)(s / a.N), v = (int)(s - (long long)fb * a.N);
    const ring::Graph g{a.adj + (size_t)fb * a.N * RING_MAX_DEGREE, a.deg + (size_t)fb * a.N, a.D + (size_t)fb * (size_t)a.N * (size_t)a.N, a.N};
    uint32_t *c = a.c + (size_t)s * (a.nmax + 1);
    for (int n = 0; n <= a.nmax; n++) c[n] = 0u;
    uint16_t P1[RING_MAX_K], P2[RING_MAX_K];
    unsigned long long st[2] = {0ull, 0ull};
    if (ring::search_source(g, v, a.nmax, a.cap, P1, P2, 1, c, st) < 0) flag_frame(&a.flags[1], a.f0 + fb);
    if (st[0]) atomicAdd(&a.stats[0], st[0]);
    if (st[1]) atomicAdd(&a.stats[1], st[1]);
}

__global__ __launch_bounds__(RR_THREADS) void ring_reduce_kernel(RingArgs a)
{
    __shared__ unsigned long long acc[4 * (RING_MAX_SIZE + 1) + 1];
    const int tid = threadIdx.x, fb = blockIdx.x, W = a.nmax + 1;
    for (int k = tid; k < 4 * W + 1; k += RR_THREADS) acc[k] = 0ull;
    __syncthreads();
    for (int v = tid; v < a.N; v += RR_THREADS) {
        const uint32_t *__restrict__ c = a.c + ((size_t)fb * a.N + v) * W;
        int first = 0, last = 0;
        for (int n = RING_MIN_SIZE; n < W; n++) {
            const uint32_t x = c[n];
            if (!x) continue;
            atomicAdd(&acc[n], (unsigned long long)x);
            atomicAdd(&acc[W + n], 1ull);
            if (!first) first = n;
            last = n;
        }
        if (first) {
            atomicAdd(&acc[2 * W + first], 1ull);
            atomicAdd(&acc[3 * W + last], 1ull);
        }
        if (a.open[(size_t)fb * a.N + v]) atomicAdd(&acc[4 * W], 1ull);
    }
    __syncthreads();
    for (int k = tid; k < 4 * W; k += RR_THREADS) a.counts[(size_t)fb * 4 * W + k] = (long long)acc[k];
    if (tid == 0) a.truncated[fb] = (long long)acc[4 * W];
}

struct RingOutputs {
    int64_t *counts, *truncated;
    uint32_t *per_atom;
    int32_t *neighbours;
    int64_t F, N;
    int32_t W;
    void zero() const
    {
        if (F <= 0) return;
        std::fill(counts, counts + (size_t)F * 4 * W, (int64_t)0);
        std::fill(truncated, truncated + (size_t)F, (int64_t)0);
        if (per_atom) std::fill(per_atom, per_atom + (size_t)F * (size_t)N * W, (uint32_t)0);
        if (neighbours) std::fill(neighbours, neighbours + (size_t)F * (size_t)N * (1 + RING_MAX_DEGREE), (int32_t)0);
    }
};

int env_int(const char *name, long long fallback)
{
    const char *e = getenv(name);
    if (!e || !e[0]) return (int)fallback;
    const long long v = atoll(e);
    return (int)std::max<long long>(0, std::min<long long>(v, 0x7fffffffLL));
}

int ring_run(amof_ctx *ctx, const amof_traj *t, const double *cutoff, int32_t nmax, const RingOutputs &out)
{
    const int S = t->n_species;
    const int64_t N = t->n_atoms, F = t->n_frames;
    const int W = nmax + 1;
    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    const double hmin = nbr_check::min_periodic_height(t->pbc, geom.rec.data(), t->n_cells);
    for (int k = 0; k < S * S; k++) AMOF_TRY(pore_refuse(ctx, nbr_check::half_height(cutoff[k], hmin)));

    const bool simple = env_int("AMOF_RING_SIMPLE", 0) == 1;
    const char *path = simple ? "ring_simple" : "ring_wave";
    int cap = env_int("AMOF_RING_MAX_PATHS", RING_MAX_PATHS);
    if (cap < 1) cap = RING_MAX_PATHS;
    const size_t table_bytes = getenv("AMOF_RING_TABLE_MB") ? (size_t)env_int("AMOF_RING_TABLE_MB", 0) << 20 : RING_TABLE_BYTES;
    const size_t per_frame = (size_t)N * (size_t)N;
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(F, 0x7fffffffLL / N), (int64_t)(table_bytes / per_frame)));     // (sources of a batch: a grid)

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    ctx->last_path = path;
    for (double &x : ctx->ring_stats) x = 0.0;
    StageSpans spans(ctx);      // adjacency, BFS, search
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(geom.rec.data(), geom.rec.size() * sizeof(double));
    const int i_spec = pk.add(t->species, (size_t)N * sizeof(int32_t));
    const int i_cut = pk.add(cutoff, (size_t)S * S * sizeof(double));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));

    RingArgs a;
    memset(&a, 0, sizeof a);
    a.pos = pos_dev;
    a.geom = pk.ptr<double>(i_geom);
    a.species = pk.ptr<int32_t>(i_spec);
    a.cutoff = pk.ptr<double>(i_cut);
    a.N = (int32_t)N;
    a.S = S;
    a.n_cells = (int32_t)t->n_cells;
    a.nmax = nmax;
    a.K = nmax / 2;
    a.cap = cap;
    const size_t sources = (size_t)batch * (size_t)N;
    void *p = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, sources * RING_MAX_DEGREE * sizeof(int32_t), &p));
    a.adj = (int32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX1, sources * sizeof(int32_t), &p));
    a.deg = (int32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX2, (size_t)batch * per_frame, &p));
    a.D = (uint8_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX3, sources * sizeof(uint32_t), &p));
    a.ncand = (uint32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX4, sources * sizeof(unsigned long long), &p));
    a.cand_off = (const unsigned long long *)p;
    void *d_off = p;
    AMOF_TRY(ensure(ctx, SLOT_AUX6, sources, &p));
    a.open = (uint8_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX7, sources * W * sizeof(uint32_t), &p));
    a.c = (uint32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_OUT0, (size_t)batch * (4 * W + 1) * sizeof(long long), &p));
    a.counts = (long long *)p;
    a.truncated = a.counts + (size_t)batch * 4 * W;
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, 2 * sizeof(int32_t) + 2 * sizeof(unsigned long long), &p));
    a.stats = (unsigned long long *)p;
    a.flags = (int32_t *)(a.stats + 2);
    AMOF_HIP_TRY(ctx, hipMemsetAsync(p, 0, 2 * sizeof(int32_t) + 2 * sizeof(unsigned long long), ctx->stream));

    std::vector<uint32_t> ncand;
    std::vector<unsigned long long> offs;
    std::vector<int32_t> rows, degs;
    int64_t launches = 0;
    double sources_done = 0.0;
    for (int64_t f0 = 0; f0 < F; f0 += batch) {
        const int nf = (int)std::min<int64_t>(batch, F - f0);
        const unsigned ns = (unsigned)((size_t)nf * (size_t)N);
        a.f0 = (int32_t)f0;
        a.nf = nf;
        int32_t flags[2];
        // ---- adjacency ----
        spans.begin(0);
        AMOF_TRY(launch_bond_rows(ctx, BondRows{a.pos, a.geom, a.species, a.cutoff, a.adj, a.deg, &a.flags[0], a.N, a.S, a.n_cells, a.f0, nf},
                                  geom.all_ortho));
        spans.end();
        AMOF_TRY(fetch(ctx, flags, a.flags, sizeof flags));
        if (flags[0])
            return fail(ctx, AMOF_ECAPACITY, "frame %d: an atom has more than RING_MAX_DEGREE = %d neighbours", flags[0] - 1, RING_MAX_DEGREE);
        if (out.neighbours) {
            rows.resize((size_t)ns * RING_MAX_DEGREE);
            degs.resize(ns);
            AMOF_TRY(fetch(ctx, rows.data(), a.adj, rows.size() * sizeof(int32_t)));
            AMOF_TRY(fetch(ctx, degs.data(), a.deg, degs.size() * sizeof(int32_t)));
            int32_t *dst = out.neighbours + (size_t)f0 * (size_t)N * (1 + RING_MAX_DEGREE);
            for (size_t s = 0; s < ns; s++) {
                dst[s * (1 + RING_MAX_DEGREE)] = degs[s];
                memcpy(dst + s * (1 + RING_MAX_DEGREE) + 1, rows.data() + s * RING_MAX_DEGREE, RING_MAX_DEGREE * sizeof(int32_t));
            }
        }
        // ---- distances, candidates ----
        spans.begin(1);
        AMOF_HIP_TRY(ctx, hipMemsetAsync(a.D, RING_FAR, (size_t)nf * per_frame, ctx->stream));
        AMOF_HIP_TRY(ctx, launch_lds(ring_bfs_kernel, dim3(ns), dim3(64), bfs_lds_bytes((int)N), ctx->stream, a, 0));
        spans.end();
        if (!simple) {
            ncand.resize(ns);
            AMOF_TRY(fetch(ctx, ncand.data(), a.ncand, (size_t)ns * sizeof(uint32_t)));
            offs.resize(ns);
            unsigned long long total = 0;
            for (unsigned s = 0; s < ns; s++) {
                offs[s] = total;
                total += ncand[s];
            }
            AMOF_TRY(ensure(ctx, SLOT_AUX5, (size_t)total * sizeof(uint32_t), &p));
            a.cand = (uint32_t *)p;
            AMOF_HIP_TRY(ctx, hipMemcpyAsync(d_off, offs.data(), (size_t)ns * sizeof(unsigned long long), hipMemcpyHostToDevice, ctx->stream));
            spans.begin(1);
            AMOF_HIP_TRY(ctx, launch_lds(ring_bfs_kernel, dim3(ns), dim3(64), bfs_lds_bytes((int)N), ctx->stream, a, 1));
            spans.end();
        }
        // ---- search ----
        timing_dom_begin(ctx, path);
        spans.begin(2);
        if (simple) AMOF_HIP_TRY(ctx, launch_lds(ring_simple_kernel, dim3((ns + 63) / 64), dim3(64), 0, ctx->stream, a));
        else AMOF_HIP_TRY(ctx, launch_lds(ring_search_kernel, dim3(ns), dim3(64), search_lds_bytes((int)N), ctx->stream, a));
        spans.end();
        timing_dom_end(ctx, ++launches);
        AMOF_HIP_TRY(ctx, launch_lds(ring_reduce_kernel, dim3((unsigned)nf), dim3(RR_THREADS), 0, ctx->stream, a));
        AMOF_TRY(fetch(ctx, flags, a.flags, sizeof flags));       // (also: offs is free again)
        if (flags[1])
            return fail(ctx, AMOF_ECAPACITY, "frame %d: more than RING_MAX_PATHS = %d shortest paths from a source to the end of a candidate",
                        flags[1] - 1, cap);
        AMOF_TRY(fetch(ctx, out.counts + (size_t)f0 * 4 * W, a.counts, (size_t)nf * 4 * W * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.truncated + f0, a.truncated, (size_t)nf * sizeof(int64_t)));
        if (out.per_atom) AMOF_TRY(fetch(ctx, out.per_atom + (size_t)f0 * (size_t)N * W, a.c, (size_t)ns * W * sizeof(uint32_t)));
        sources_done += (double)ns;
    }
    timing_end(ctx);
    unsigned long long st[2];
    AMOF_TRY(fetch(ctx, st, a.stats, sizeof st));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    ctx->ring_stats[0] = sources_done;
    ctx->ring_stats[1] = (double)st[0];
    ctx->ring_stats[2] = (double)st[1];
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_ring_stats(amof_ctx *ctx, const amof_traj *t, const double *cutoff, int32_t max_size, int64_t *counts,
                               int64_t *truncated, uint32_t *per_atom, int32_t *neighbours)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(validate_traj(ctx, t, false));
    if (max_size < RING_MIN_SIZE || max_size > RING_MAX_SIZE)
        return fail(ctx, AMOF_EINVAL, "max_size must be %d..%d", RING_MIN_SIZE, RING_MAX_SIZE);
    if (!cutoff || (t->n_frames > 0 && (!counts || !truncated))) return fail(ctx, AMOF_EINVAL, "NULL argument");
    const RingOutputs out{counts, truncated, per_atom, neighbours, t->n_frames, t->n_atoms, max_size + 1};
    out.zero();     // the outputs are overwritten: zeros first, so that a failing call leaves zeros
    AMOF_TRY(pore_refuse(ctx, nbr_check::bond_matrix(cutoff, t->n_species, "cutoff")));
    if (t->n_atoms > RING_MAX_ATOMS) return fail(ctx, AMOF_ECAPACITY, "%lld atoms: more than the %d a path of u16 node ids can name", (long long)t->n_atoms, RING_MAX_ATOMS);
    if (t->n_frames == 0 || t->n_atoms == 0) return AMOF_OK;
    const int rc = ring_run(ctx, t, cutoff, max_size, out);
    if (rc != AMOF_OK) {
        (void)sync_stream(ctx);
        out.zero();
    }
    return rc;
}

extern "C" int amof_ring_search_stats(const amof_ctx *ctx, double *out)
{
    if (!ctx || !out) return AMOF_EINVAL;
    for (int k = 0; k < 3; k++) out[k] = ctx->ring_stats[k];
    return AMOF_OK;
}
