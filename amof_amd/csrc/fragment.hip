// Fragments of the bond graph of every frame: connected components under periodic boundaries, the lattice image of every atom
// that makes its fragment whole, winding, per-fragment sums (include/amof_hip.h, amof_fragment_stats).
// Replaces the search underneath amof/coordination/reduce.py and core.py (pymatgen neighbour lists, networkx components), one
// frame at a time with a 30-minute timeout per frame.
//
// Stages of a batch of frames (a batch: as many frames as AMOF_FRAGMENT_BATCH_MB admits rows, records and scratch for):
//   ring_adjacency_kernel    ring.hip's rows through launch_bond_rows, once with the cutoff matrix and, with links, once more
//                            with the link matrix
//   fragment_image_kernel    an atom per thread: per row entry the lattice vector of fragment_math.h's pair_image, three int8 in a
//                            word; a component beyond 127 flags the frame
//   fragment_frame_kernel    "fragment_frame", the default: a workgroup per frame, both generations of the 8-byte records in LDS
//                            (16 N bytes), the rows read from device memory; a round per workgroup barrier (__syncthreads_or of
//                            "changed"); the last generation and the round count go to device memory
//   fragment_round_kernel    "fragment_global" (AMOF_FRAGMENT_GLOBAL=1, or 16 N bytes beyond the LDS of a CU): the same round as
//                            one launch over the atoms of the batch, the generations in device memory, the host reading a
//                            changed word per frame between the launches; no LDS
//   fragment_reduce_kernel   a workgroup per frame on the final records, whichever kernel wrote them: the winding relation per
//                            bond, integer atomics per root (atoms, species counts, fixed-point mass-weighted coordinates), then
//                            per root the size histogram and the census against `kinds`, then the link bonds by the kinds of
//                            their two fragments and the centres
// No loop waits on another workgroup; every loop is bounded by N rounds (a label only falls), the row length and K.
// Hooking and pointer jumping were NOT built.  Measured on 50 frames of the 9792-atom headline trajectory
// (profiles/fragment/fragment_timing.md): the percolating network of the full four-cutoff dictionary takes 88 rounds per frame on
// average and at most 262, and labelling is then 0.063 ms per frame on "fragment_frame" (0.108 ms on "fragment_global") beside
// 0.236 ms for one all-pairs adjacency pass; the ligand dictionary takes 6 to 7 rounds and 0.003 ms.  Labelling never exceeds the
// adjacency stage, so shortening it is not where the time is; "fragment_frame" is the faster kernel and the default.
//
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage; no kernel spills, no scratch):
//   kernel                   VGPRs  SGPRs  static LDS  dynamic LDS                     waves / SIMD by registers
//   fragment_image_kernel       25     44         0    0                               8
//   fragment_frame_kernel       22     49       256 B  16 N B (153 KB at 9792)         8
//   fragment_init_kernel         4     14         0    0                               8
//   fragment_round_kernel       14     26         0    0                               8
//   fragment_reduce_kernel      42    102        40 B  0                               7
// fragment_frame_kernel's static 256 B are __syncthreads_or's; with them 10224 atoms fit the 160 KB of a CU.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "amof_internal.h"
#include "fragment_math.h"
#include "nbr_check.h"

static_assert(FRAG_MAX_DEGREE == 16, "the rows are ring_adjacency_kernel's: RING_MAX_DEGREE");

namespace amof {
namespace {

constexpr int FI_THREADS = 256;         // fragment_image_kernel, fragment_init_kernel, fragment_round_kernel: an atom per thread
constexpr int FF_THREADS = 1024;        // fragment_frame_kernel, fragment_reduce_kernel: a workgroup per frame
constexpr size_t FRAG_BATCH_BYTES = (size_t)256 << 20;      // rows, records and scratch of a batch (AMOF_FRAGMENT_BATCH_MB overrides)

struct FragArgs {
    const double *pos;          // [F][N][3] of the call
    const double *geom;
    const double *masses;       // [N] (with com)
    const int32_t *species;     // [N]
    const int32_t *adj, *deg;   // [nf][N][16], [nf][N]
    uint32_t *img;              // [nf][N][16]
    const int32_t *ladj, *ldeg; // the link rows, or null
    int32_t *rounds;            // [nf]
    int32_t *changed;           // [nf] ("fragment_global")
    long long *sums;            // per root slot [nf][N][3][2]: the two words of fragment_math.h's fixed-point sums
    uint32_t *size, *wind;      // [nf][N]
    int32_t *kind;              // [nf][N]: the kind of the fragment rooted here
    uint32_t *spc;              // [nf][N][S]
    const int32_t *ref_label;   // [N] or null
    const int32_t *ref_roots;   // [M]
    const double *ref_mass;     // [M]
    const int32_t *kinds;       // [K][S]
    long long *summary, *hist, *census, *links;     // [nf][5], [nf][max_size + 2], [nf][K + 1], [nf][K + 1][K + 1] or null
    double *com;                // [nf][M][3] or null
    int32_t *flags;             // 1 + the first frame with [0] a 17th neighbour (cutoff or link rows), [1] an image or a shift that
                                // does not fit its storage, [2] a coordinate beyond FRAG_COORD_MAX
    int32_t N, S, n_cells, f0, nf, K, M, max_size, ortho;
};

__global__ __launch_bounds__(FI_THREADS) void fragment_image_kernel(FragArgs a)
{
    const int i = blockIdx.x * FI_THREADS + threadIdx.x, fb = blockIdx.y, f = a.f0 + fb;
    if (i >= a.N) return;
    const double *__restrict__ p = a.pos + (size_t)f * (size_t)a.N * 3;
    const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    const size_t at = (size_t)fb * a.N + i;
    const int32_t *__restrict__ row = a.adj + at * FRAG_MAX_DEGREE;
    uint32_t *__restrict__ out = a.img + at * FRAG_MAX_DEGREE;
    const double xi = p[(size_t)i * 3 + 0], yi = p[(size_t)i * 3 + 1], zi = p[(size_t)i * 3 + 2];
    const int d = a.deg[at];
    bool bad = false;
    for (int q = 0; q < d; q++) {
        const size_t j = (size_t)row[q];
        double n[3];
        frag::pair_image(g, a.ortho != 0, p[j * 3 + 0] - xi, p[j * 3 + 1] - yi, p[j * 3 + 2] - zi, n);
        uint32_t w = 0;
        if (!frag::pack_image(n, &w)) bad = true;
        out[q] = w;
    }
    if (bad) flag_frame(&a.flags[1], f);
}

__global__ __launch_bounds__(FF_THREADS) void fragment_frame_kernel(FragArgs a, frag::Rec *out)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ff_smem[];
    frag::Rec *A = reinterpret_cast<frag::Rec *>(ff_smem), *B = A + a.N;
    const int tid = threadIdx.x, fb = blockIdx.x;
    const int32_t *__restrict__ adj = a.adj + (size_t)fb * a.N * FRAG_MAX_DEGREE;
    const uint32_t *__restrict__ img = a.img + (size_t)fb * a.N * FRAG_MAX_DEGREE;
    const int32_t *__restrict__ deg = a.deg + (size_t)fb * a.N;
    for (int i = tid; i < a.N; i += FF_THREADS) A[i] = frag::Rec{(uint16_t)i, {0, 0, 0}};
    __syncthreads();
    int rounds = 0;
    while (rounds < a.N) {          // (a label only falls: at most N - 1 rounds change a record)
        bool changed = false, overflow = false;
        for (int i = tid; i < a.N; i += FF_THREADS)
            B[i] = frag::relabel(A, adj + (size_t)i * FRAG_MAX_DEGREE, img + (size_t)i * FRAG_MAX_DEGREE, deg[i], i, &changed, &overflow);
        if (overflow) flag_frame(&a.flags[1], a.f0 + fb);
        rounds++;
        const int any = __syncthreads_or(changed ? 1 : 0);
        frag::Rec *t = A;
        A = B;
        B = t;
        if (!any) break;
    }
    frag::Rec *dst = out + (size_t)fb * a.N;
    for (int i = tid; i < a.N; i += FF_THREADS) dst[i] = A[i];
    if (tid == 0) a.rounds[fb] = rounds;
}

__global__ __launch_bounds__(FI_THREADS) void fragment_init_kernel(FragArgs a, frag::Rec *out)
{
    const int i = blockIdx.x * FI_THREADS + threadIdx.x, fb = blockIdx.y;
    if (i < a.N) out[(size_t)fb * a.N + i] = frag::Rec{(uint16_t)i, {0, 0, 0}};
}

__global__ __launch_bounds__(FI_THREADS) void fragment_round_kernel(FragArgs a, const frag::Rec *cur, frag::Rec *nxt)
{
    const int i = blockIdx.x * FI_THREADS + threadIdx.x, fb = blockIdx.y;
    if (i >= a.N) return;
    const size_t at = (size_t)fb * a.N + i;
    bool changed = false, overflow = false;
    nxt[at] = frag::relabel(cur + (size_t)fb * a.N, a.adj + at * FRAG_MAX_DEGREE, a.img + at * FRAG_MAX_DEGREE, a.deg[at], i, &changed, &overflow);
    if (changed) a.changed[fb] = 1;
    if (overflow) flag_frame(&a.flags[1], a.f0 + fb);
}

template <typename T> __device__ __forceinline__ T load_fresh(const T *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(FF_THREADS) void fragment_reduce_kernel(FragArgs a, const frag::Rec *recs)
{
    __shared__ unsigned long long acc[5];       // fragments, atoms of the largest, winding, regrouped atoms, links inside a fragment
    const int tid = threadIdx.x, fb = blockIdx.x, f = a.f0 + fb, N = a.N, S = a.S, K = a.K;
    const size_t base = (size_t)fb * N;
    const frag::Rec *__restrict__ rec = recs + base;
    const int32_t *__restrict__ deg = a.deg + base;
    long long *sums = a.sums + base * 6;
    uint32_t *size = a.size + base, *wind = a.wind + base, *spc = a.spc + base * S;
    int32_t *kind = a.kind + base;
    const double *__restrict__ p = a.pos + (size_t)f * (size_t)N * 3;
    const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : f) * GEOM_STRIDE;
    if (tid < 5) acc[tid] = 0ull;
    __syncthreads();
    // ---- per atom: its root's counters, the relation on its bonds ----
    unsigned regrouped = 0;
    for (int i = tid; i < N; i += FF_THREADS) {
        const frag::Rec r = rec[i];
        const int L = r.label;
        atomicAdd(&size[L], 1u);
        atomicAdd(&spc[(size_t)L * S + a.species[i]], 1u);
        const int32_t *__restrict__ row = a.adj + (base + i) * FRAG_MAX_DEGREE;
        const uint32_t *__restrict__ img = a.img + (base + i) * FRAG_MAX_DEGREE;
        bool holds = true;
        const int d = deg[i];
        for (int q = 0; q < d; q++)
            if (!frag::bond_holds(r, rec[row[q]], img[q])) holds = false;
        if (!holds) atomicOr(&wind[L], 1u);
        if (a.ref_label && a.ref_label[i] != L) regrouped++;
        if (a.com) {
            double x[3];
            frag::whole_coord(g, p + (size_t)i * 3, r.s, x);
            const double m = a.masses[i];
            for (int c = 0; c < 3; c++) {
                long long hi = 0, lo = 0;
                if (!frag::fixed_term(m, x[c], &hi, &lo)) flag_frame(&a.flags[2], f);
                atomicAdd(reinterpret_cast<unsigned long long *>(&sums[((size_t)L * 3 + c) * 2]), (unsigned long long)hi);
                atomicAdd(reinterpret_cast<unsigned long long *>(&sums[((size_t)L * 3 + c) * 2 + 1]), (unsigned long long)lo);
            }
        }
    }
    if (regrouped) atomicAdd(&acc[3], (unsigned long long)regrouped);
    __threadfence();
    __syncthreads();
    // ---- per root: histogram, census ----
    for (int r = tid; r < N; r += FF_THREADS) {
        if (rec[r].label != r) continue;
        const unsigned n = load_fresh(&size[r]);
        atomicAdd(&acc[0], 1ull);
        atomicMax(&acc[1], (unsigned long long)n);
        if (load_fresh(&wind[r])) atomicAdd(&acc[2], 1ull);
        atomicAdd(reinterpret_cast<unsigned long long *>(&a.hist[(size_t)fb * (a.max_size + 2) + min((int)n, a.max_size + 1)]), 1ull);
        int k = 0;
        for (; k < K; k++) {
            bool same = true;
            for (int s = 0; s < S; s++)
                if ((int32_t)load_fresh(&spc[(size_t)r * S + s]) != a.kinds[(size_t)k * S + s]) same = false;
            if (same) break;
        }
        atomicAdd(reinterpret_cast<unsigned long long *>(&a.census[(size_t)fb * (K + 1) + k]), 1ull);
        kind[r] = k;
    }
    __threadfence();
    __syncthreads();
    // ---- link bonds by the kinds of their fragments; centres ----
    if (a.ladj) {
        unsigned inside = 0;
        for (int i = tid; i < N; i += FF_THREADS) {
            const int Li = rec[i].label;
            const int32_t *__restrict__ row = a.ladj + (base + i) * FRAG_MAX_DEGREE;
            const int d = a.ldeg[base + i];
            for (int q = 0; q < d; q++) {
                const int j = row[q], Lj = rec[j].label;
                if (Li == Lj) inside += i < j ? 1u : 0u;
                else if (a.links)
                    atomicAdd(reinterpret_cast<unsigned long long *>(&a.links[((size_t)fb * (K + 1) + load_fresh(&kind[Li])) * (K + 1) + load_fresh(&kind[Lj])]), 1ull);
            }
        }
        if (inside) atomicAdd(&acc[4], (unsigned long long)inside);
    }
    if (a.com) {
        const bool same_partition = acc[3] == 0ull;
        for (int k = tid; k < a.M; k += FF_THREADS) {
            const int root = a.ref_roots[k];
            const bool whole = same_partition && !load_fresh(&wind[root]);
            for (int c = 0; c < 3; c++)
                a.com[((size_t)fb * a.M + k) * 3 + c] = whole ? frag::centre(load_fresh(&sums[((size_t)root * 3 + c) * 2]), load_fresh(&sums[((size_t)root * 3 + c) * 2 + 1]), a.ref_mass[k]) : (double)NAN;
        }
    }
    __syncthreads();
    if (tid < 5) a.summary[(size_t)fb * 5 + tid] = tid == 3 && !a.ref_label ? -1ll : (long long)acc[tid];
}

struct FragOutputs {
    int64_t *summary, *hist, *census, *links;
    int32_t *label, *shift;
    double *com, *frag_mass;
    int64_t F, N;
    int32_t K, M, max_size;
    template <typename T> static void clear(T *p, size_t n) { if (p) std::fill(p, p + n, (T)0); }
    void zero() const
    {
        if (F <= 0) return;
        const size_t f = (size_t)F, k1 = (size_t)K + 1;
        clear(summary, f * 5), clear(hist, f * ((size_t)max_size + 2)), clear(census, f * k1), clear(links, f * k1 * k1);
        clear(label, f * (size_t)N), clear(shift, f * (size_t)N * 3), clear(com, f * (size_t)M * 3), clear(frag_mass, (size_t)M);
    }
};

struct FragInputs {
    const double *cutoff, *link;
    const int32_t *ref_label, *kinds;
    std::vector<int32_t> ref_roots;
    std::vector<double> ref_mass;
};

long long env_ll(const char *name, long long fallback)
{
    const char *e = getenv(name);
    if (!e || !e[0]) return fallback;
    return std::max<long long>(0, std::min<long long>(atoll(e), 0x7fffffffLL));
}

int fragment_run(amof_ctx *ctx, const amof_traj *t, const FragInputs &in, const FragOutputs &out)
{
    const int S = t->n_species, K = out.K, M = out.M, H = out.max_size + 2;
    const int64_t N = t->n_atoms, F = t->n_frames;
    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    const double hmin = nbr_check::min_periodic_height(t->pbc, geom.rec.data(), t->n_cells);
    for (int k = 0; k < S * S; k++)
        AMOF_TRY(pore_refuse(ctx, nbr_check::half_height(std::max(in.cutoff[k], in.link ? in.link[k] : 0.0), hmin)));

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    int lds_cap = 0;
    AMOF_HIP_TRY(ctx, hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerBlock, ctx->device));
    hipFuncAttributes attr;
    AMOF_HIP_TRY(ctx, hipFuncGetAttributes(&attr, (const void *)fragment_frame_kernel));
    lds_cap -= (int)attr.sharedSizeBytes;
    if (getenv("AMOF_FRAGMENT_LDS_KB")) lds_cap = (int)std::min<long long>(lds_cap, env_ll("AMOF_FRAGMENT_LDS_KB", 0) << 10);
    const size_t lds_bytes = (size_t)N * 2 * sizeof(frag::Rec);
    const bool global = env_ll("AMOF_FRAGMENT_GLOBAL", 0) == 1 || lds_bytes > (size_t)lds_cap;
    const char *path = global ? "fragment_global" : "fragment_frame";
    // per frame: two sets of rows and degrees, the images, two generations of records, the root scratch, the outputs
    const size_t root_bytes = (size_t)N * (6 * sizeof(long long) + 3 * sizeof(uint32_t) + (size_t)S * sizeof(uint32_t));
    const size_t out_bytes = ((size_t)5 + H + (K + 1) + (size_t)(K + 1) * (K + 1)) * sizeof(long long) + (size_t)M * 3 * sizeof(double);
    const size_t per_frame = (size_t)N * (3 * FRAG_MAX_DEGREE * 4 + 2 * 4 + 2 * sizeof(frag::Rec)) + root_bytes + out_bytes;
    const size_t cap_bytes = getenv("AMOF_FRAGMENT_BATCH_MB") ? (size_t)env_ll("AMOF_FRAGMENT_BATCH_MB", 0) << 20 : FRAG_BATCH_BYTES;
    const int64_t batch = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(F, 65535), (int64_t)(cap_bytes / per_frame)));   // (frames of a batch: grid.y)

    timing_begin(ctx);
    ctx->last_path = path;
    for (double &x : ctx->fragment_stats) x = 0.0;
    StageSpans spans(ctx);      // adjacency, labelling, reduction with the census
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    UploadPack pk;
    const int i_geom = pk.add(geom.rec.data(), geom.rec.size() * sizeof(double));
    const int i_spec = pk.add(t->species, (size_t)N * sizeof(int32_t));
    const int i_cut = pk.add(in.cutoff, (size_t)S * S * sizeof(double));
    const int i_link = pk.add(in.link, in.link ? (size_t)S * S * sizeof(double) : 0);
    const int i_mass = pk.add(t->masses, out.com ? (size_t)N * sizeof(double) : 0);
    const int i_ref = pk.add(in.ref_label, in.ref_label ? (size_t)N * sizeof(int32_t) : 0);
    const int i_roots = pk.add(in.ref_roots.data(), in.ref_roots.size() * sizeof(int32_t));
    const int i_rmass = pk.add(in.ref_mass.data(), in.ref_mass.size() * sizeof(double));
    const int i_kinds = pk.add(in.kinds, (size_t)K * S * sizeof(int32_t));
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));

    FragArgs a;
    memset(&a, 0, sizeof a);
    a.pos = pos_dev;
    a.geom = pk.ptr<double>(i_geom);
    a.species = pk.ptr<int32_t>(i_spec);
    a.masses = pk.ptr<double>(i_mass);
    a.ref_label = in.ref_label ? pk.ptr<int32_t>(i_ref) : nullptr;
    a.ref_roots = pk.ptr<int32_t>(i_roots);
    a.ref_mass = pk.ptr<double>(i_rmass);
    a.kinds = pk.ptr<int32_t>(i_kinds);
    a.N = (int32_t)N;
    a.S = S;
    a.n_cells = (int32_t)t->n_cells;
    a.K = K;
    a.M = M;
    a.max_size = out.max_size;
    a.ortho = geom.all_ortho ? 1 : 0;
    const size_t atoms = (size_t)batch * (size_t)N;
    void *p = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, atoms * FRAG_MAX_DEGREE * sizeof(int32_t), &p));
    int32_t *adj = (int32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX1, atoms * sizeof(int32_t), &p));
    int32_t *deg = (int32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX2, atoms * FRAG_MAX_DEGREE * sizeof(uint32_t), &p));
    a.img = (uint32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX3, 2 * atoms * sizeof(frag::Rec), &p));
    frag::Rec *rec0 = (frag::Rec *)p, *rec1 = rec0 + atoms;
    int32_t *ladj = nullptr, *ldeg = nullptr;
    if (in.link) {
        AMOF_TRY(ensure(ctx, SLOT_AUX4, atoms * FRAG_MAX_DEGREE * sizeof(int32_t), &p));
        ladj = (int32_t *)p;
        AMOF_TRY(ensure(ctx, SLOT_AUX5, atoms * sizeof(int32_t), &p));
        ldeg = (int32_t *)p;
    }
    void *root_dev = nullptr, *out_dev = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX6, (size_t)batch * root_bytes, &root_dev));
    a.sums = (long long *)root_dev;
    a.size = (uint32_t *)(a.sums + atoms * 6);
    a.wind = a.size + atoms;
    a.kind = (int32_t *)(a.wind + atoms);
    a.spc = (uint32_t *)(a.kind + atoms);
    AMOF_TRY(ensure(ctx, SLOT_AUX7, 2 * (size_t)batch * sizeof(int32_t), &p));
    a.rounds = (int32_t *)p;
    a.changed = a.rounds + batch;
    AMOF_TRY(ensure(ctx, SLOT_OUT0, (size_t)batch * out_bytes, &out_dev));
    a.summary = (long long *)out_dev;
    a.hist = a.summary + (size_t)batch * 5;
    a.census = a.hist + (size_t)batch * H;
    long long *links_dev = a.census + (size_t)batch * (K + 1);
    a.links = in.link && out.links ? links_dev : nullptr;
    a.com = out.com ? (double *)(links_dev + (size_t)batch * (K + 1) * (K + 1)) : nullptr;
    AMOF_TRY(ensure(ctx, SLOT_FLAGS, 4 * sizeof(int32_t), &p));
    a.flags = (int32_t *)p;
    AMOF_HIP_TRY(ctx, hipMemsetAsync(a.flags, 0, 4 * sizeof(int32_t), ctx->stream));

    std::vector<frag::Rec> recs;
    std::vector<int32_t> rounds, changed;
    int64_t launches = 0;
    double rounds_sum = 0.0, rounds_max = 0.0;
    const unsigned gx = (unsigned)((N + FI_THREADS - 1) / FI_THREADS);
    for (int64_t f0 = 0; f0 < F; f0 += batch) {
        const int nf = (int)std::min<int64_t>(batch, F - f0);
        const size_t na = (size_t)nf * (size_t)N;
        a.f0 = (int32_t)f0;
        a.nf = nf;
        int32_t flags[4];
        // ---- bond rows, link rows ----
        spans.begin(0);
        AMOF_TRY(launch_bond_rows(ctx, BondRows{a.pos, a.geom, a.species, pk.ptr<double>(i_cut), adj, deg, &a.flags[0], a.N, S, a.n_cells, a.f0, nf},
                                  geom.all_ortho));
        if (in.link)
            AMOF_TRY(launch_bond_rows(ctx, BondRows{a.pos, a.geom, a.species, pk.ptr<double>(i_link), ladj, ldeg, &a.flags[0], a.N, S, a.n_cells, a.f0, nf},
                                      geom.all_ortho));
        spans.end();
        a.adj = adj;
        a.deg = deg;
        a.ladj = ladj;
        a.ldeg = ldeg;
        AMOF_TRY(fetch(ctx, flags, a.flags, sizeof flags));
        if (flags[0])
            return fail(ctx, AMOF_ECAPACITY, "frame %d: an atom has more than FRAG_MAX_DEGREE = %d neighbours", flags[0] - 1, FRAG_MAX_DEGREE);
        // ---- labelling ----
        timing_dom_begin(ctx, path);
        spans.begin(1);
        AMOF_HIP_TRY(ctx, launch_lds(fragment_image_kernel, dim3(gx, (unsigned)nf), dim3(FI_THREADS), 0, ctx->stream, a));
        const frag::Rec *final_rec = rec0;
        rounds.assign((size_t)nf, 0);
        if (!global) {
            AMOF_HIP_TRY(ctx, launch_lds(fragment_frame_kernel, dim3((unsigned)nf), dim3(FF_THREADS), lds_bytes, ctx->stream, a, rec0));
            launches++;
            spans.end();
            AMOF_TRY(fetch(ctx, rounds.data(), a.rounds, (size_t)nf * sizeof(int32_t)));
        } else {
            AMOF_HIP_TRY(ctx, launch_lds(fragment_init_kernel, dim3(gx, (unsigned)nf), dim3(FI_THREADS), 0, ctx->stream, a, rec0));
            spans.end();
            frag::Rec *cur = rec0, *nxt = rec1;
            changed.assign((size_t)nf, 0);
            for (int64_t round = 0; round < N; round++) {       // (a label only falls)
                spans.begin(1);
                AMOF_HIP_TRY(ctx, hipMemsetAsync(a.changed, 0, (size_t)nf * sizeof(int32_t), ctx->stream));
                AMOF_HIP_TRY(ctx, launch_lds(fragment_round_kernel, dim3(gx, (unsigned)nf), dim3(FI_THREADS), 0, ctx->stream, a, (const frag::Rec *)cur, nxt));
                spans.end();
                launches++;
                AMOF_TRY(fetch(ctx, changed.data(), a.changed, (size_t)nf * sizeof(int32_t)));
                std::swap(cur, nxt);
                bool any = false;
                for (int k = 0; k < nf; k++) {
                    // a frame's rounds: those that changed a record of it and the one that found nothing to change
                    if (changed[(size_t)k]) rounds[(size_t)k] = (int32_t)round + 2;
                    else if (round == 0) rounds[(size_t)k] = 1;
                    any = any || changed[(size_t)k];
                }
                if (!any) break;
            }
            for (int k = 0; k < nf; k++) rounds[(size_t)k] = (int32_t)std::min<int64_t>(rounds[(size_t)k], N);
            final_rec = cur;
        }
        timing_dom_end(ctx, launches);
        for (int k = 0; k < nf; k++) {
            rounds_sum += rounds[(size_t)k];
            rounds_max = std::max(rounds_max, (double)rounds[(size_t)k]);
        }
        // ---- reduction, census ----
        spans.begin(2);
        AMOF_HIP_TRY(ctx, hipMemsetAsync(root_dev, 0, (size_t)batch * root_bytes, ctx->stream));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(out_dev, 0, (size_t)batch * out_bytes, ctx->stream));
        AMOF_HIP_TRY(ctx, launch_lds(fragment_reduce_kernel, dim3((unsigned)nf), dim3(FF_THREADS), 0, ctx->stream, a, final_rec));
        spans.end();
        AMOF_TRY(fetch(ctx, flags, a.flags, sizeof flags));
        if (flags[1])
            return fail(ctx, AMOF_ECAPACITY, "frame %d: a shift does not fit its storage (a bond's image beyond %d cells or an atom's shift beyond %d)",
                        flags[1] - 1, FRAG_IMAGE_MAX, FRAG_SHIFT_MAX);
        if (flags[2])
            return fail(ctx, AMOF_ECAPACITY, "frame %d: an atom of a whole fragment lies %g A or more from the origin", flags[2] - 1, FRAG_COORD_MAX);
        AMOF_TRY(fetch(ctx, out.summary + (size_t)f0 * 5, a.summary, (size_t)nf * 5 * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.hist + (size_t)f0 * H, a.hist, (size_t)nf * H * sizeof(int64_t)));
        AMOF_TRY(fetch(ctx, out.census + (size_t)f0 * (K + 1), a.census, (size_t)nf * (K + 1) * sizeof(int64_t)));
        if (a.links) AMOF_TRY(fetch(ctx, out.links + (size_t)f0 * (K + 1) * (K + 1), a.links, (size_t)nf * (K + 1) * (K + 1) * sizeof(int64_t)));
        if (a.com) AMOF_TRY(fetch(ctx, out.com + (size_t)f0 * M * 3, a.com, (size_t)nf * M * 3 * sizeof(double)));
        if (out.label || out.shift) {
            recs.resize(na);
            AMOF_TRY(fetch(ctx, recs.data(), final_rec, na * sizeof(frag::Rec)));
            for (size_t s = 0; s < na; s++) {
                if (out.label) out.label[(size_t)f0 * N + s] = recs[s].label;
                for (int c = 0; out.shift && c < 3; c++) out.shift[((size_t)f0 * N + s) * 3 + c] = recs[s].s[c];
            }
        }
    }
    timing_end(ctx);
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    ctx->fragment_stats[0] = (double)F;
    ctx->fragment_stats[1] = rounds_sum;
    ctx->fragment_stats[2] = rounds_max;
    if (out.frag_mass) std::copy(in.ref_mass.begin(), in.ref_mass.end(), out.frag_mass);
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_fragment_stats(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const double *link, const int32_t *ref_label,
                                   const int32_t *kinds, int32_t K, int32_t max_size, int64_t *summary, int64_t *size_hist, int64_t *census,
                                   int64_t *links, int32_t *label, int32_t *shift, double *com, double *frag_mass, int32_t M)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(validate_traj(ctx, t, com != nullptr || frag_mass != nullptr));
    if (max_size < 1 || max_size > FRAG_MAX_ATOMS) return fail(ctx, AMOF_EINVAL, "max_size must be 1..%d", FRAG_MAX_ATOMS);
    if (K < 0 || K > FRAG_MAX_ATOMS || M < 0) return fail(ctx, AMOF_EINVAL, "K must be 0..%d and M >= 0", FRAG_MAX_ATOMS);
    if (!cutoff || (K > 0 && !kinds) || (t->n_frames > 0 && (!summary || !size_hist || !census))) return fail(ctx, AMOF_EINVAL, "NULL argument");
    if (!ref_label) M = 0;
    const FragOutputs out{summary, size_hist, census, links, label, shift, ref_label ? com : nullptr, ref_label ? frag_mass : nullptr,
                          t->n_frames, t->n_atoms, K, M, max_size};
    if ((com || frag_mass) && !ref_label) return fail(ctx, AMOF_EINVAL, "com and frag_mass need ref_label");
    if (links && !link) return fail(ctx, AMOF_EINVAL, "links needs the link matrix");
    out.zero();     // the outputs are overwritten: zeros first, so that a failing call leaves zeros
    const int S = t->n_species;
    const int64_t N = t->n_atoms;
    AMOF_TRY(pore_refuse(ctx, nbr_check::bond_matrix(cutoff, S, "cutoff")));
    if (link) {
        AMOF_TRY(pore_refuse(ctx, nbr_check::bond_matrix(link, S, "link")));
        for (int k = 0; k < S * S; k++)
            if (link[k] > 0.0 && cutoff[k] > 0.0) return fail(ctx, AMOF_EINVAL, "a species pair is named by the cutoff and by the link matrix");
    }
    for (int64_t k = 0; k < (int64_t)K * S; k++)
        if (kinds[k] < 0) return fail(ctx, AMOF_EINVAL, "kinds must be >= 0");
    if (N > FRAG_MAX_ATOMS) return fail(ctx, AMOF_ECAPACITY, "%lld atoms: more than the %d a u16 label can name", (long long)N, FRAG_MAX_ATOMS);
    FragInputs in{cutoff, link, ref_label, kinds, {}, {}};
    if (ref_label) {
        // a partition by roots: every label is the smallest atom of its class
        for (int64_t i = 0; i < N; i++) {
            const int32_t r = ref_label[i];
            if (r < 0 || r > i || ref_label[r] != r) return fail(ctx, AMOF_EINVAL, "ref_label[%lld] = %d is not the smallest atom of a class", (long long)i, r);
            if (r == i) in.ref_roots.push_back((int32_t)i);
        }
        if ((com || frag_mass) && (int64_t)in.ref_roots.size() != M) return fail(ctx, AMOF_EINVAL, "ref_label has %zu roots, M = %d", in.ref_roots.size(), M);
        if (com || frag_mass) {
            // the masses of the reference fragments, atoms in ascending order
            std::vector<int32_t> slot((size_t)N, 0);
            for (size_t k = 0; k < in.ref_roots.size(); k++) slot[(size_t)in.ref_roots[k]] = (int32_t)k;
            in.ref_mass.assign(in.ref_roots.size(), 0.0);
            for (int64_t i = 0; i < N; i++) {
                const double m = t->masses[i];
                if (!(m > 0.0) || !(m < FRAG_MASS_MAX)) return fail(ctx, AMOF_EINVAL, "masses[%lld] = %g: outside (0, %g)", (long long)i, m, FRAG_MASS_MAX);
                in.ref_mass[(size_t)slot[(size_t)ref_label[i]]] += m;
            }
        } else {
            in.ref_roots.clear();
        }
    }
    if (t->n_frames == 0 || N == 0) {
        if (out.frag_mass) std::copy(in.ref_mass.begin(), in.ref_mass.end(), out.frag_mass);
        for (int64_t f = 0; f < t->n_frames; f++) summary[f * 5 + 3] = ref_label ? 0 : -1;
        return AMOF_OK;
    }
    const int rc = fragment_run(ctx, t, in, out);
    if (rc != AMOF_OK) {
        (void)sync_stream(ctx);
        out.zero();
    }
    return rc;
}

extern "C" int amof_fragment_round_stats(const amof_ctx *ctx, double *out)
{
    if (!ctx || !out) return AMOF_EINVAL;
    for (int k = 0; k < 3; k++) out[k] = ctx->fragment_stats[k];
    return AMOF_OK;
}
