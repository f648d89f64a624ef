// Surface area of the pore space (gfx950): deterministic Shrake-Rupley sampling.  Every atom j carries M samples
//     s = r_j + rho_j u_m,   rho_j = R_j + rp        (include/amof_hip.h amof_pore_surface; u_m: the caller's directions)
// and a sample is EXPOSED when no other atom's sphere of radius R_k + rp holds it -- when the pore field of all other atoms,
// evaluated at the sample, is >= rp: the canonical minimum image and the float64 compare of pore.hip.  The kernels count the
// exposed samples per species; with the labelling stage's channel marks an exposed sample is ACCESSIBLE when one of the 8 grid
// points around it lies in a channel of V(rp).  The reference reads ASA / NASA from Zeo++ -sa (Monte-Carlo samples on the same
// spheres); nothing of that is reproduced.
//
//   pore_surface_exact   a lane per sample, every atom of the frame through LDS tiles, canonical float64 arithmetic
//   pore_surface_list    a wave per atom of the cell-sorted order (launch_cell_sort), four per workgroup.  The wave gathers the
//                        images k with |r_k - r_j| < rho_j + rho_k, every periodic image on its own, as float32 records
//                        (image - r_j, rho_k) in its own region of LDS, those that bury a quarter of the atom's sphere or more
//                        in front (the early exit comes sooner).  Every lane then takes samples m = lane, lane + 64, ...
//                        and sweeps the records with a root-free float32 compare (pore_surface_math.h): buried ends the sample,
//                        clear goes on, and inside the guard band the canonical float64 arithmetic decides from the raw
//                        positions.  The same integers as pore_surface_exact.
// The accessible test is fused into both kernels: it is eight loads behind the few samples that come out exposed.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "pore_surface_math.h"

namespace amof {

constexpr int SURF_THREADS = 256;
constexpr int SURF_WAVES = SURF_THREADS / 64;       // atoms per workgroup of pore_surface_list
constexpr int SURF_MAX_SPECIES = 64;                // validate_traj's limit
constexpr int SURF_STATS = 5;                       // atoms, records, samples, float64 re-decisions, early exits
constexpr int SURF_CELL_EDGE_MAX = 32;
constexpr uint32_t SURF_ATOM_MASK = (1u << CELL_SPECIES_SHIFT) - 1u;

struct SurfArgs {
    const double *pos;          // the frame's [N][3]
    const double *g;            // the frame's geometry record
    const double *radii;        // [S]
    const int32_t *species;     // [N]
    const double *dirs;         // [M][3]
    const QAtom *Q;             // the frame's cell-sorted records (pore_surface_list)
    const uint32_t *start3;     // [nkeys + 1]
    const int32_t *parent, *mark;       // the periodic labels and channel marks of V(rp), or null: no accessible test
    unsigned long long *out;    // [S] exposed, [S] accessible, [1] a wave's list was full, [SURF_STATS] statistics
    uint8_t *samples;           // [N][M] or null
    double inv[9];              // cell^-1, all columns (the corner rule also reads open axes)
    double rp, rho_max;         // rho_max = max_s radii[s] + rp
    int64_t N;
    int32_t S, M;
    int32_t nc[3];              // cell list
    int32_t n[3], pbc[3];       // the field's grid
    int32_t cap;
    int32_t order;              // 1: records that bury a quarter of the sphere or more come first (0: AMOF_PORE_SURFACE_UNSORTED=1)
    float eps;
};

// the 8 grid points around the sample: f = s C^-1 (wrapped into [0, 1) on periodic axes), t_k = f_k n_k - 0.5, i_k = floor(t_k),
// corners i_k + {0, 1} -- modulo n_k on a periodic axis, dropped outside the grid on an open one
__device__ __forceinline__ bool surf_accessible(const SurfArgs &a, double sx, double sy, double sz)
{
    int i[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double f = (sx * a.inv[k] + sy * a.inv[3 + k]) + sz * a.inv[6 + k];
        if (a.pbc[k]) f = f - floor(f);
        const double t = f * (double)a.n[k] - 0.5;
        const double fl = floor(t);
        i[k] = fl < -2.0 ? -2 : fl > (double)a.n[k] ? a.n[k] : (int)fl;        // (an open axis: anywhere; NaN lands outside)
        if (!(fl == fl)) i[k] = -2;
    }
    for (int c = 0; c < 8; c++) {
        int x[3] = {i[0] + (c >> 2), i[1] + ((c >> 1) & 1), i[2] + (c & 1)};
        bool in = true;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            if (a.pbc[k]) x[k] = x[k] < 0 ? x[k] + a.n[k] : x[k] >= a.n[k] ? x[k] - a.n[k] : x[k];
            in = in && x[k] >= 0 && x[k] < a.n[k];
        }
        if (!in) continue;
        const int r = a.parent[((int64_t)x[0] * a.n[1] + x[1]) * a.n[2] + x[2]];
        if (r >= 0 && a.mark[r] < 0) return true;
    }
    return false;
}

// end of a workgroup: one 64-bit atomic per non-empty counter
__device__ __forceinline__ void surf_flush(const SurfArgs &a, const unsigned *cnt, int words)
{
    for (int w = threadIdx.x; w < words; w += SURF_THREADS)
        if (cnt[w]) atomicAdd(&a.out[w < 2 * a.S ? w : w + 1], (unsigned long long)cnt[w]);        // (the flag sits behind the 2 S counters)
}

// ---------------------------------------------------------------- exact ----
template <bool ORTHO>
__global__ __launch_bounds__(SURF_THREADS) void pore_surface_exact_kernel(SurfArgs a)
{
    __shared__ double tx[SURF_THREADS], ty[SURF_THREADS], tz[SURF_THREADS], tr[SURF_THREADS];
    __shared__ unsigned cnt[2 * SURF_MAX_SPECIES];
    const int tid = threadIdx.x;
    for (int w = tid; w < 2 * a.S; w += SURF_THREADS) cnt[w] = 0u;
    const int64_t id = (int64_t)blockIdx.x * SURF_THREADS + tid;
    const bool valid = id < a.N * (int64_t)a.M;
    int64_t j = -1;
    int sp = 0;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (valid) {
        j = id / a.M;
        const int m = (int)(id % a.M);
        sp = a.species[j];
        const double rho = a.radii[sp] + a.rp;
        sx = a.pos[j * 3 + 0] + rho * a.dirs[m * 3 + 0];
        sy = a.pos[j * 3 + 1] + rho * a.dirs[m * 3 + 1];
        sz = a.pos[j * 3 + 2] + rho * a.dirs[m * 3 + 2];
    }
    bool buried = false;
    for (int64_t k0 = 0; k0 < a.N; k0 += SURF_THREADS) {
        const int n = (int)min((int64_t)SURF_THREADS, a.N - k0);
        __syncthreads();
        if (tid < n) {
            tx[tid] = a.pos[(k0 + tid) * 3 + 0];
            ty[tid] = a.pos[(k0 + tid) * 3 + 1];
            tz[tid] = a.pos[(k0 + tid) * 3 + 2];
            tr[tid] = a.radii[a.species[k0 + tid]];
        }
        __syncthreads();
        if (valid) {
            for (int k = 0; k < n && !buried; k++) {
                if (k0 + k == j) continue;
                double dx, dy, dz;
                pair_base<ORTHO>(a.g, tx[k] - sx, ty[k] - sy, tz[k] - sz, dx, dy, dz);
                buried = !(sqrt(norm2(dx, dy, dz)) - tr[k] >= a.rp);
            }
        }
    }
    if (valid) {
        uint8_t code = 0;
        if (!buried) {
            code = 1;
            atomicAdd(&cnt[sp], 1u);
            if (a.parent && surf_accessible(a, sx, sy, sz)) {
                code = 2;
                atomicAdd(&cnt[a.S + sp], 1u);
            }
        }
        if (a.samples) a.samples[id] = code;
    }
    __syncthreads();
    surf_flush(a, cnt, 2 * a.S);
}

// ----------------------------------------------------------------- list ----
__device__ __forceinline__ int surf_floor_div(int x, int n)
{
    const int q = x / n;
    return (x % n != 0 && x < 0) ? q - 1 : q;
}

template <bool ORTHO>
__global__ __launch_bounds__(SURF_THREADS) void pore_surface_list_kernel(SurfArgs a)
{
    __shared__ float4 rec[SURF_WAVES][SURF_LIST_CAP];       // image - r_j (x, y, z) and rho_k, float32
    __shared__ uint32_t ridx[SURF_WAVES][SURF_LIST_CAP];    // species << CELL_SPECIES_SHIFT | atom
    __shared__ unsigned n_list[SURF_WAVES], n_far[SURF_WAVES];
    __shared__ unsigned cnt[2 * SURF_MAX_SPECIES + SURF_STATS];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int words = 2 * a.S + SURF_STATS;
    for (int w = tid; w < words; w += SURF_THREADS) cnt[w] = 0u;
    if (tid < SURF_WAVES) n_list[tid] = n_far[tid] = 0u;
    const int64_t w = (int64_t)blockIdx.x * SURF_WAVES + wave;      // this wave's atom, in the cell-sorted order
    const bool have = w < a.N;                                      // (wave-uniform)
    const double *__restrict__ g = a.g;
    int64_t at = 0;
    int sp = 0;
    double rho_j = 0.0, rj[3] = {0.0, 0.0, 0.0};
    __syncthreads();

    // ---- gather: the cells within reach of the atom, every periodic image by itself; the atom's own images are no neighbours
    if (have) {
        const QAtom qj = a.Q[w];
        at = min((int64_t)(qj.idx & SURF_ATOM_MASK), a.N - 1);
        sp = min((int)(qj.idx >> CELL_SPECIES_SHIFT), a.S - 1);
        rho_j = a.radii[sp] + a.rp;
        for (int c = 0; c < 3; c++) rj[c] = a.pos[at * 3 + c];
        const double fc[3] = {(double)qj.ux * (1.0 / 4294967296.0), (double)qj.uy * (1.0 / 4294967296.0), (double)qj.uz * (1.0 / 4294967296.0)};
        const double reach = (rho_j + a.rho_max) * (1.0 + 1e-6) + 2e-6;
        int lo[3], cn[3];
        for (int k = 0; k < 3; k++) {
            const double rho = reach / g[18 + k];
            lo[k] = (int)floor((fc[k] - rho) * (double)a.nc[k]);
            cn[k] = (int)floor((fc[k] + rho) * (double)a.nc[k]) - lo[k] + 1;
        }
        const int total = cn[0] * cn[1] * cn[2];
        for (int e = lane; e < total; e += 64) {
            const int ex = lo[0] + e % cn[0], ey = lo[1] + (e / cn[0]) % cn[1], ez = lo[2] + e / (cn[0] * cn[1]);
            const int sx = surf_floor_div(ex, a.nc[0]), sy = surf_floor_div(ey, a.nc[1]), sz = surf_floor_div(ez, a.nc[2]);
            const int cell = ((ez - sz * a.nc[2]) * a.nc[1] + (ey - sy * a.nc[1])) * a.nc[0] + (ex - sx * a.nc[0]);
            const uint32_t k0 = a.start3[(size_t)cell * a.S];
            const uint32_t k1 = min(a.start3[(size_t)(cell + 1) * a.S], (uint32_t)a.N);
            for (uint32_t k = k0; k < k1; k++) {
                const QAtom q = a.Q[k];
                if ((int64_t)(q.idx & SURF_ATOM_MASK) == at) continue;
                const int spk = min((int)(q.idx >> CELL_SPECIES_SHIFT), a.S - 1);
                const double d0 = ((double)q.ux * (1.0 / 4294967296.0) + (double)sx) - fc[0];
                const double d1 = ((double)q.uy * (1.0 / 4294967296.0) + (double)sy) - fc[1];
                const double d2 = ((double)q.uz * (1.0 / 4294967296.0) + (double)sz) - fc[2];
                const double Ax = (d0 * g[0] + d1 * g[3]) + d2 * g[6];
                const double Ay = (d0 * g[1] + d1 * g[4]) + d2 * g[7];
                const double Az = (d0 * g[2] + d1 * g[5]) + d2 * g[8];
                const double rho_k = a.radii[spk] + a.rp;
                const double D = sqrt(Ax * Ax + Ay * Ay + Az * Az);
                if (D < (rho_j + rho_k) * (1.0 + 1e-6) + 2e-6) {
                    // the sphere of k holds the cap of j's sphere with cos(angle to A) > c: near records (a quarter of the sphere
                    // or more) fill the list from the front, the others from the back
                    const bool far = a.order && (rho_j * rho_j + D * D - rho_k * rho_k) > rho_j * D;
                    unsigned slot = far ? atomicAdd(&n_far[wave], 1u) : atomicAdd(&n_list[wave], 1u);
                    if (far) slot = slot < (unsigned)a.cap ? (unsigned)a.cap - 1u - slot : 0xffffffffu;
                    if (slot < (unsigned)a.cap) {
                        rec[wave][slot] = make_float4((float)Ax, (float)Ay, (float)Az, (float)rho_k);
                        ridx[wave][slot] = q.idx;
                    }
                }
            }
        }
    }
    __syncthreads();
    const int n_near = (int)n_list[wave];
    int n = n_near + (int)n_far[wave];
    const bool full = n > a.cap;
    if (have && full && lane == 0) a.out[2 * a.S] = 1ull;       // (the host discards the launch's results and runs pore_surface_exact)

    // ---- sweep: a lane goes on to its next sample as soon as one is decided, whatever the other lanes are at
    unsigned n_exp = 0, n_acc = 0, n_redo = 0, n_early = 0;
    if (have && !full) {
        int m = lane, jr = 0;
        bool buried = false;
        double s[3] = {0.0, 0.0, 0.0};
        float pf[3] = {0.f, 0.f, 0.f};
        auto start = [&]() {
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const double P = rho_j * a.dirs[m * 3 + c];
                s[c] = rj[c] + P;
                pf[c] = (float)P;
            }
            buried = false;
            jr = 0;
        };
        if (m < a.M) start();
        while (m < a.M) {
            if (jr < n) {
                const int slot = jr < n_near ? jr : a.cap - 1 - (jr - n_near);
                const float4 r = rec[wave][slot];
                int dec = surf_decide(surf_d2(r.x, r.y, r.z, pf[0], pf[1], pf[2]), r.w, a.eps);
                if (dec == 0) {
                    const uint32_t id = ridx[wave][slot];
                    const int64_t k = min((int64_t)(id & SURF_ATOM_MASK), a.N - 1);
                    const int spk = min((int)(id >> CELL_SPECIES_SHIFT), a.S - 1);
                    double dx, dy, dz;
                    pair_base<ORTHO>(g, a.pos[k * 3] - s[0], a.pos[k * 3 + 1] - s[1], a.pos[k * 3 + 2] - s[2], dx, dy, dz);
                    dec = sqrt(norm2(dx, dy, dz)) - a.radii[spk] >= a.rp ? 1 : -1;
                    n_redo++;
                }
                jr++;
                if (dec < 0) {
                    buried = true;
                    n_early += jr < n;
                }
            }
            if (buried || jr >= n) {
                uint8_t code = 0;
                if (!buried) {
                    code = 1;
                    n_exp++;
                    if (a.parent && surf_accessible(a, s[0], s[1], s[2])) {
                        code = 2;
                        n_acc++;
                    }
                }
                if (a.samples) a.samples[at * a.M + m] = code;
                m += 64;
                if (m < a.M) start();
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        n_exp += __shfl_down(n_exp, off, 64);
        n_acc += __shfl_down(n_acc, off, 64);
        n_redo += __shfl_down(n_redo, off, 64);
        n_early += __shfl_down(n_early, off, 64);
    }
    if (have && !full && lane == 0) {
        if (n_exp) atomicAdd(&cnt[sp], n_exp);
        if (n_acc) atomicAdd(&cnt[a.S + sp], n_acc);
        atomicAdd(&cnt[2 * a.S + 0], 1u);
        atomicAdd(&cnt[2 * a.S + 1], (unsigned)n);
        atomicAdd(&cnt[2 * a.S + 2], (unsigned)a.M);
        atomicAdd(&cnt[2 * a.S + 3], n_redo);
        atomicAdd(&cnt[2 * a.S + 4], n_early);
    }
    __syncthreads();
    surf_flush(a, cnt, words);
}

// ------------------------------------------------------------ host side ----
struct SurfaceCall {
    amof_ctx *ctx = nullptr;
    const PoreInputs *in = nullptr;
    const PoreOutputs *out = nullptr;       // exposed, exposed_access, samples
    const double *dirs = nullptr;           // host [M][3]
    int32_t M = 0;
    bool want_access = false, force_exact = false;
    bool order = true;                      // AMOF_PORE_SURFACE_UNSORTED=1: the records in the order of the gather (for measurements)
    int32_t cap = SURF_LIST_CAP;            // AMOF_PORE_SURFACE_LIST_CAP=n (1 .. SURF_LIST_CAP) shortens a wave's list: the tests' way to the retry
    PoreAtoms atoms{};
    int64_t N = 0;
    int32_t S = 0;
    bool list_ok = false;                   // pore_surface_list applies to the call
    int32_t nc[3] = {1, 1, 1};
    int64_t nkeys = 0;
    // device
    double *d_dirs = nullptr;
    unsigned long long *d_out = nullptr;    // [2 S + 1 + SURF_STATS], then the cell sort's flags (int32 [2])
    int words = 0;
    QAtom *d_Q = nullptr;
    uint32_t *d_start = nullptr, *d_keys = nullptr, *d_cursor = nullptr;
    uint8_t *d_samples = nullptr;
    std::vector<unsigned long long> h_table, h_out;
    // the frame at hand
    int64_t sorted_frame = -1;
    bool frame_list = false;                // the sorted frame may use the list (no atom absurdly far from the cell)
    // the call
    int64_t launches = 0;
    bool used_exact = false;
    double stats[SURF_STATS] = {0.0, 0.0, 0.0, 0.0, 0.0};
};

// what the call samples and where its answers go; no device work
static void surf_plan(SurfaceCall &s, amof_ctx *ctx, const PoreInputs &in, const PoreOutputs &out, const double *dirs, int32_t n_dirs)
{
    s.ctx = ctx;
    s.in = &in;
    s.out = &out;
    s.dirs = dirs;
    s.M = n_dirs;
    s.want_access = in.want_access != 0;
    s.N = in.t->n_atoms;
    s.S = in.t->n_species;
    const char *ex = getenv("AMOF_PORE_SURFACE_EXACT");
    s.force_exact = ex && ex[0] == '1';
    if (const char *cap = getenv("AMOF_PORE_SURFACE_LIST_CAP")) s.cap = std::min(SURF_LIST_CAP, std::max(1, atoi(cap)));
    const char *od = getenv("AMOF_PORE_SURFACE_UNSORTED");
    s.order = !(od && od[0] == '1');
    s.words = 2 * s.S + 1 + SURF_STATS;
}

size_t pore_surface_fixed_bytes(const SurfaceCall &s)
{
    return (size_t)s.N * 24 + (size_t)s.M * 24 + (s.out->samples ? (size_t)s.N * (size_t)s.M : 0) + ((size_t)1 << 20);
}

void pore_surface_restart(SurfaceCall &s)
{
    s.launches = 0;
    s.used_exact = false;
    s.sorted_frame = -1;
    for (double &x : s.stats) x = 0.0;
}

void pore_surface_report(const SurfaceCall &s)
{
    s.ctx->last_path = s.used_exact ? "pore_surface_exact" : "pore_surface_list";
    s.ctx->dom_launches = s.launches;
    for (int k = 0; k < SURF_STATS; k++) s.ctx->surface_stats[k] = s.stats[k];
}

int pore_surface_setup(SurfaceCall &s, const PoreAtoms &atoms)
{
    amof_ctx *ctx = s.ctx;
    const amof_traj *t = s.in->t;
    s.atoms = atoms;
    pore_surface_restart(s);
    double tmax = 0.0;
    for (int k = 0; k < s.in->n_t; k++) tmax = std::max(tmax, s.in->thresholds[k]);
    AMOF_TRY(pore_refuse(ctx, pore_check::half_height_surface(atoms.rmax, tmax, atoms.hmin)));
    if ((s.N * (int64_t)s.M + SURF_THREADS - 1) / SURF_THREADS > 0x7fffffffLL)
        return fail(ctx, AMOF_ECAPACITY, "pore surface: %lld atoms x %d directions are more samples than one launch takes", (long long)s.N, s.M);
    // the cell list of pore_surface_list: periodic on every axis (an open axis has no fractional coordinate to sort by), within the
    // cell sort's limits; cells of 3 A or more, as pore_brick's
    s.list_ok = t->pbc[0] && t->pbc[1] && t->pbc[2] && s.N >= 1 && s.N < (1ll << CELL_SPECIES_SHIFT) && s.S <= SURF_MAX_SPECIES;
    double hmin[3] = {INFINITY, INFINITY, INFINITY};
    for (int64_t k = 0; k < t->n_cells; k++)
        for (int x = 0; x < 3; x++) hmin[x] = std::min(hmin[x], atoms.host->rec[(size_t)k * GEOM_STRIDE + 18 + x]);
    for (int x = 0; x < 3; x++) s.nc[x] = (int)std::max(1.0, std::min((double)SURF_CELL_EDGE_MAX, floor(hmin[x] / 3.0)));
    s.nkeys = (int64_t)s.nc[0] * s.nc[1] * s.nc[2] * s.S;
    // directions, then the counters of a launch and the cell sort's flags
    s.h_table.assign((size_t)3 * s.M + s.words + 1, 0ull);
    memcpy(s.h_table.data(), s.dirs, (size_t)3 * s.M * sizeof(double));
    void *p;
    AMOF_TRY(upload(ctx, SLOT_SURF4, s.h_table.data(), s.h_table.size() * sizeof(unsigned long long), &p));
    s.d_dirs = (double *)p;
    s.d_out = (unsigned long long *)p + 3 * (size_t)s.M;
    if (s.list_ok && !s.force_exact) {
        AMOF_TRY(ensure(ctx, SLOT_SURF0, (size_t)s.N * sizeof(QAtom), &p));
        s.d_Q = (QAtom *)p;
        AMOF_TRY(ensure(ctx, SLOT_SURF1, (size_t)(s.nkeys + 1) * sizeof(uint32_t), &p));
        s.d_start = (uint32_t *)p;
        AMOF_TRY(ensure(ctx, SLOT_SURF2, (size_t)s.N * sizeof(uint32_t), &p));
        s.d_keys = (uint32_t *)p;
        AMOF_TRY(ensure(ctx, SLOT_SURF3, (size_t)s.nkeys * sizeof(uint32_t), &p));
        s.d_cursor = (uint32_t *)p;
    }
    if (s.out->samples && s.N > 0) {
        AMOF_TRY(ensure(ctx, SLOT_SURF5, (size_t)s.N * (size_t)s.M, &p));
        s.d_samples = (uint8_t *)p;
    }
    return AMOF_OK;
}

// the exposed (and accessible) samples of threshold k of frame f, whose positions lie on the device
int pore_surface_threshold(SurfaceCall &s, int64_t f, int32_t k, const int32_t *parent, const int32_t *mark, bool channels, StageSpans &spans)
{
    amof_ctx *ctx = s.ctx;
    const amof_traj *t = s.in->t;
    const size_t row = ((size_t)f * (size_t)s.in->n_t + (size_t)k) * (size_t)s.S;
    int64_t *exposed = s.out->exposed + row, *access = s.out->exposed_access ? s.out->exposed_access + row : nullptr;
    for (int x = 0; x < s.S; x++) {
        exposed[x] = 0;
        if (access) access[x] = 0;
    }
    if (s.N == 0) return AMOF_OK;
    const int64_t gi = t->n_cells == 1 ? 0 : f;
    const double *rec = s.atoms.host->rec.data() + (size_t)gi * GEOM_STRIDE;
    const bool ortho = rec[22] != 0.0;
    int32_t *d_flags = (int32_t *)(s.d_out + s.words);
    spans.begin(4);
    if (s.list_ok && !s.force_exact && s.sorted_frame != f) {
        // the stage's own cell sort, one per frame: it also runs behind pore_exact, which sorts nothing
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, 2 * sizeof(int32_t), ctx->stream));
        AMOF_TRY(launch_cell_sort(ctx, s.atoms.pos, s.atoms.geom, (int)t->n_cells, s.atoms.species, s.S, s.N, (int)f, 1, s.nc[0], s.nc[1],
                                  s.nc[2], s.d_Q, s.d_start, s.d_keys, s.d_cursor, d_flags));
        s.sorted_frame = f;
        s.frame_list = true;
    }
    SurfArgs a;
    memset(&a, 0, sizeof a);
    a.pos = s.atoms.pos + (size_t)f * (size_t)s.N * 3;
    a.g = s.atoms.geom + (size_t)gi * GEOM_STRIDE;
    a.radii = s.atoms.radii;
    a.species = s.atoms.species;
    a.dirs = s.d_dirs;
    a.Q = s.d_Q;
    a.start3 = s.d_start;
    if (s.want_access && channels) {
        a.parent = parent;
        a.mark = mark;
    }
    a.out = s.d_out;
    a.samples = s.d_samples;
    for (int q = 0; q < 9; q++) a.inv[q] = s.atoms.host->invfull[(size_t)gi * 9 + q];
    a.rp = s.in->thresholds[k];
    a.rho_max = s.atoms.rmax + a.rp;
    a.N = s.N;
    a.S = s.S;
    a.M = s.M;
    for (int x = 0; x < 3; x++) {
        a.nc[x] = s.nc[x];
        a.n[x] = s.in->grid[x];
        a.pbc[x] = t->pbc[x] ? 1 : 0;
    }
    a.cap = s.cap;
    a.order = s.order ? 1 : 0;
    double tmax = 0.0;
    for (int q = 0; q < s.in->n_t; q++) tmax = std::max(tmax, s.in->thresholds[q]);
    a.eps = surf_eps32(pore_surface_bound(rec, s.atoms.rmax + tmax));
    bool list = s.list_ok && !s.force_exact && s.frame_list;
    s.h_out.resize((size_t)s.words + 1);
    for (int attempt = 0; attempt < 2; attempt++) {
        AMOF_HIP_TRY(ctx, hipMemsetAsync(s.d_out, 0, (size_t)s.words * sizeof(unsigned long long), ctx->stream));
        if (list) {
            const dim3 grid((unsigned)((s.N + SURF_WAVES - 1) / SURF_WAVES));
            AMOF_HIP_TRY(ctx, ortho ? launch_lds(pore_surface_list_kernel<true>, grid, dim3(SURF_THREADS), 0, ctx->stream, a)
                                    : launch_lds(pore_surface_list_kernel<false>, grid, dim3(SURF_THREADS), 0, ctx->stream, a));
        } else {
            const dim3 grid((unsigned)((s.N * (int64_t)s.M + SURF_THREADS - 1) / SURF_THREADS));
            AMOF_HIP_TRY(ctx, ortho ? launch_lds(pore_surface_exact_kernel<true>, grid, dim3(SURF_THREADS), 0, ctx->stream, a)
                                    : launch_lds(pore_surface_exact_kernel<false>, grid, dim3(SURF_THREADS), 0, ctx->stream, a));
        }
        s.launches++;
        AMOF_TRY(fetch(ctx, s.h_out.data(), s.d_out, s.h_out.size() * sizeof(unsigned long long)));
        if (!list) break;
        int32_t flags[2];
        memcpy(flags, &s.h_out[(size_t)s.words], sizeof flags);
        if (flags[0]) s.frame_list = false;     // an atom absurdly far from the cell: no thresholds of this frame on the list
        if (!flags[0] && !s.h_out[(size_t)2 * s.S]) break;
        list = false;                           // a wave's list was too short: the launch once more, on the exact path
    }
    spans.end();
    if (!list) s.used_exact = true;
    else
        for (int q = 0; q < SURF_STATS; q++) s.stats[q] += (double)s.h_out[(size_t)2 * s.S + 1 + q];
    for (int x = 0; x < s.S; x++) {
        exposed[x] = (int64_t)s.h_out[(size_t)x];
        if (access) access[x] = (int64_t)s.h_out[(size_t)s.S + x];
    }
    if (s.out->samples)
        AMOF_TRY(fetch(ctx, s.out->samples + ((size_t)f * (size_t)s.in->n_t + (size_t)k) * (size_t)s.N * (size_t)s.M, s.d_samples,
                       (size_t)s.N * (size_t)s.M));
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

extern "C" double amof_pore_surface_bound(const double *cell, double reach)
{
    return cell ? pore_surface_bound(cell, reach) : -1.0;
}

extern "C" int amof_pore_surface_stats(const amof_ctx *ctx, double *out5)
{
    if (!ctx || !out5) return AMOF_EINVAL;
    for (int k = 0; k < SURF_STATS; k++) out5[k] = ctx->surface_stats[k];
    return AMOF_OK;
}

extern "C" int amof_pore_surface(amof_ctx *ctx, const amof_traj *t, const double *radii, const int32_t *grid, double dr, double dmax,
                                 const double *thresholds, int32_t n_t, int32_t want_access, int32_t want_free, uint64_t *hist,
                                 int64_t *counts, double *vmax, int64_t *argmax, int64_t *access, double *free_sphere, double *field,
                                 int32_t *labels, uint64_t *psd_hist, int64_t *po_counts, int64_t *po_access, double *cover, int32_t want_psd,
                                 const double *dirs, int32_t n_dirs, int64_t *exposed, int64_t *exposed_access, uint8_t *samples)
{
    if (!ctx) return AMOF_EINVAL;
    const bool labelled = want_access || want_free;
    PoreOutputs out{hist, counts, vmax, argmax, field, labelled ? access : nullptr, labelled ? free_sphere : nullptr,
                    labelled ? labels : nullptr, want_psd ? psd_hist : nullptr, want_psd ? po_counts : nullptr,
                    want_psd && want_access ? po_access : nullptr, want_psd ? cover : nullptr, exposed,
                    want_access ? exposed_access : nullptr, samples};       // (what the call does not ask for is not the record's)
    AMOF_TRY(pore_refuse(ctx, pore_check::both_given(t, grid)));
    AMOF_TRY(validate_traj(ctx, t, false));
    AMOF_TRY(pore_refuse(ctx, pore_check::direction_count(n_dirs)));
    AMOF_TRY(pore_refuse(ctx, pore_check::both_given(dirs, dirs)));
    AMOF_TRY(pore_refuse(ctx, pore_check::directions(dirs, n_dirs)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_given(thresholds, n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_finite(thresholds, n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::probes_not_negative(thresholds, n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::surface_outputs(t->n_frames, n_t, want_access, exposed, exposed_access)));
    if (samples) AMOF_TRY(pore_refuse(ctx, pore_check::samples_cap(n_t, t->n_atoms, n_dirs)));
    out.S = t->n_species;
    out.NM = t->n_atoms * (int64_t)n_dirs;
    const int32_t pbc[3] = {t->pbc[0], t->pbc[1], t->pbc[2]};
    const PoreInputs in{t, radii, nullptr, nullptr, t->n_frames, grid, pbc, dr, dmax, thresholds, n_t, want_access, want_free};
    SurfaceCall s;
    surf_plan(s, ctx, in, out, dirs, n_dirs);
    return out.keep(pore_psd_surface_run(ctx, in, out, want_psd != 0, s));
}
