// Accessibility of the pore field (gfx950): periodic connected components of the thresholded field V(t) = {p : v(p) >= t},
// whether a component wraps around the cell (its winding lattice, include/amof_hip.h amof_pore_access) and the largest
// threshold at which one still does (the free sphere).  The field kernels are pore.hip's, unchanged; this file labels.
//
// One labelling = a union-find over the grid points whose parent array is int32 [G] in device memory, -1 outside the void:
//   pa_tile_kernel     ("pore_label_tile") a workgroup labels a tile of 8 x 8 x 32 grid points in LDS -- mask from the field on
//                      the fly, unions of the links inside the tile, roots as global indices written in whole lines
//   pa_init_kernel     ("pore_label_global", AMOF_PORE_LABEL_GLOBAL=1) parent = own index; every link is merged in HBM
//   pa_merge_kernel    the links that cross tile faces (tile 1 x 1 x 1 on the global path), not those through the cell's faces
//   pa_flatten_kernel  parent = root: the OPEN labels (label = smallest linear index of the component)
//   pa_links_kernel    the links through the periodic faces between void points, as (open label below, open label above) in
//                      the slot of their face point
//   pa_wrap_kernel     the same links merged into the parent array; flattened again: the PERIODIC labels
//   pa_count_kernel    points per root: one atomic per wave and run of one root; pa_compact_kernel: the (root, size) list
// Unions always point to the smaller index, so parent[i] <= i at every instant: a find walks a strictly descending chain and
// a union retries on a strictly smaller value -- no loop waits for another workgroup.  Inside the merging kernels every access
// to parent[] is a relaxed agent-scope atomic (the L2s of the eight XCDs are not coherent for plain accesses within a kernel),
// and a union is complete only on the value its atomic min returns.  Plain loads read what an earlier kernel wrote.
// The host (pore_access_math.h) resolves the windings from the wrap links: O(links + components) per labelling.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "amof_internal.h"
#include "pore_access_math.h"

namespace amof {

constexpr int PA_THREADS = 256;
constexpr int PA_TX = 8, PA_TY = 8, PA_TZ = 32;         // tile of the LDS phase (z is the contiguous axis: 256-byte field rows)
constexpr int PA_TILE = PA_TX * PA_TY * PA_TZ;
constexpr int PA_PPL = PA_TILE / PA_THREADS;            // grid points per lane
static_assert(PA_TY * PA_TZ == PA_THREADS && PA_PPL == PA_TX, "a lane's points are one (j, k) column of the tile: l = tid + q * PA_THREADS");

struct PaGrid {
    int32_t n[3];
    int32_t pbc[3];
    int32_t t[3];           // tile of the phase before the merge ((1, 1, 1): every link is merged)
    int64_t G;
    int64_t nl[3];          // merge kernel: links per axis; links kernel: face points per axis
};

template <int SCOPE> __device__ __forceinline__ int pa_load(const int32_t *p)
{
    return __hip_atomic_load(p, __ATOMIC_RELAXED, SCOPE);
}

// root of x: the chain descends strictly (a value that does not is a root -- or, were the array ever corrupt, the end)
template <int SCOPE> __device__ __forceinline__ int pa_find(const int32_t *parent, int x)
{
    for (;;) {
        const int p = pa_load<SCOPE>(parent + x);
        if ((unsigned)p >= (unsigned)x) return x;
        x = p;
    }
}

// a and b into one tree, the larger root under the smaller.  The atomic min may hit an `a` that lost its root status since the
// find: it returns that newer parent (< a), a then points to min(old, b), and the loop goes on to unite old with b -- every
// retry starts from a strictly smaller a.
template <int SCOPE> __device__ __forceinline__ void pa_union(int32_t *parent, int a, int b)
{
    for (;;) {
        a = pa_find<SCOPE>(parent, a);
        b = pa_find<SCOPE>(parent, b);
        if (a == b) return;
        if (a < b) {
            const int s = a;
            a = b;
            b = s;
        }
        const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, SCOPE);
        if (old == a) return;
        a = old;
    }
}

constexpr int PA_AGENT = __HIP_MEMORY_SCOPE_AGENT;
constexpr int PA_WG = __HIP_MEMORY_SCOPE_WORKGROUP;

__global__ __launch_bounds__(PA_THREADS) void pa_init_kernel(const double *__restrict__ field, double thr, int32_t *__restrict__ parent,
                                                             int64_t G)
{
    const int64_t i = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    if (i < G) parent[i] = field[i] >= thr ? (int32_t)i : -1;
}

__global__ __launch_bounds__(PA_THREADS) void pa_tile_kernel(const double *__restrict__ field, double thr, int32_t *__restrict__ parent,
                                                             PaGrid g, int ntz, int nty)
{
    __shared__ int32_t lab[PA_TILE];
    const int tid = threadIdx.x;
    const int bz = blockIdx.x % ntz, by = (blockIdx.x / ntz) % nty, bx = blockIdx.x / (ntz * nty);
    const int lk = tid % PA_TZ, lj = tid / PA_TZ;
    const int j = by * PA_TY + lj, k = bz * PA_TZ + lk, i0 = bx * PA_TX;
    const bool col = j < g.n[1] && k < g.n[2];
    const int64_t plane = (int64_t)g.n[1] * g.n[2];
    const int64_t base = (int64_t)i0 * plane + (int64_t)j * g.n[2] + k;         // (< 2^31 wherever col && i < n[0])
#pragma unroll
    for (int q = 0; q < PA_PPL; q++) {
        const int l = tid + q * PA_THREADS;
        const bool in = col && i0 + q < g.n[0];
        lab[l] = (in && field[base + q * plane] >= thr) ? l : -1;
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PA_PPL; q++) {
        const int l = tid + q * PA_THREADS;
        if (pa_load<PA_WG>(lab + l) < 0) continue;
        if (lk + 1 < PA_TZ && pa_load<PA_WG>(lab + l + 1) >= 0) pa_union<PA_WG>(lab, l, l + 1);
        if (lj + 1 < PA_TY && pa_load<PA_WG>(lab + l + PA_TZ) >= 0) pa_union<PA_WG>(lab, l, l + PA_TZ);
        if (q + 1 < PA_PPL && pa_load<PA_WG>(lab + l + PA_THREADS) >= 0) pa_union<PA_WG>(lab, l, l + PA_THREADS);
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PA_PPL; q++) {
        const int l = tid + q * PA_THREADS;
        if (!(col && i0 + q < g.n[0])) continue;
        int32_t out = -1;
        if (lab[l] >= 0) {
            const int r = pa_find<PA_WG>(lab, l);        // (nothing is written to lab any more)
            const int ri = r / PA_THREADS, rj = (r / PA_TZ) % PA_TY, rk = r % PA_TZ;
            out = (int32_t)((int64_t)(i0 + ri) * plane + (int64_t)(by * PA_TY + rj) * g.n[2] + (bz * PA_TZ + rk));
        }
        parent[base + q * plane] = out;
    }
}

// one thread per link across a tile face (not a cell face): axis 0, then 1, then 2
__global__ __launch_bounds__(PA_THREADS) void pa_merge_kernel(int32_t *parent, PaGrid g)
{
    int64_t id = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    const int64_t ny = g.n[1], nz = g.n[2];
    int64_t a, b;
    if (id < g.nl[0]) {
        const int64_t m = id / (ny * nz) + 1, rest = id % (ny * nz);
        a = (m * g.t[0] - 1) * ny * nz + rest;
        b = a + ny * nz;
    } else if ((id -= g.nl[0]) < g.nl[1]) {
        const int64_t B = (g.n[1] - 1) / g.t[1];
        const int64_t k = id % nz, m = (id / nz) % B + 1, i = id / (nz * B);
        a = (i * ny + (m * g.t[1] - 1)) * nz + k;
        b = a + nz;
    } else if ((id -= g.nl[1]) < g.nl[2]) {
        const int64_t B = (g.n[2] - 1) / g.t[2];
        const int64_t m = id % B + 1, ij = id / B;
        a = ij * nz + (m * g.t[2] - 1);
        b = a + 1;
    } else
        return;
    if (pa_load<PA_AGENT>(parent + a) >= 0 && pa_load<PA_AGENT>(parent + b) >= 0) pa_union<PA_AGENT>(parent, (int)a, (int)b);
}

__global__ __launch_bounds__(PA_THREADS) void pa_flatten_kernel(int32_t *parent, int64_t G)
{
    const int64_t i = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    if (i >= G) return;
    const int p = pa_load<PA_AGENT>(parent + i);
    if (p < 0 || p == (int)i) return;
    const int r = pa_find<PA_AGENT>(parent, p);
    // (others flatten their own entries meanwhile: whatever a find reads lies on the same descending chain to the same root)
    if (r != p) __hip_atomic_store(parent + i, r, __ATOMIC_RELAXED, PA_AGENT);
}

// slot s of the link table: the face point s of axis 0 (ny nz of them), then axis 1 (nx nz), then axis 2 (nx ny)
__device__ __forceinline__ bool pa_face_pair(const PaGrid &g, int64_t id, int64_t &a, int64_t &b, int &axis)
{
    const int64_t nx = g.n[0], ny = g.n[1], nz = g.n[2];
    if (id < g.nl[0]) {
        axis = 0;
        a = (nx - 1) * ny * nz + id;
        b = id;
    } else if ((id -= g.nl[0]) < g.nl[1]) {
        axis = 1;
        const int64_t i = id / nz, k = id % nz;
        a = (i * ny + ny - 1) * nz + k;
        b = i * ny * nz + k;
    } else if ((id -= g.nl[1]) < g.nl[2]) {
        axis = 2;
        a = id * nz + nz - 1;
        b = id * nz;
    } else
        return false;
    return true;
}

__global__ __launch_bounds__(PA_THREADS) void pa_links_kernel(const int32_t *__restrict__ parent, PaGrid g, int2 *__restrict__ links)
{
    const int64_t id = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    int64_t a, b;
    int axis;
    if (!pa_face_pair(g, id, a, b, axis)) return;
    int2 out = make_int2(-1, -1);
    if (g.pbc[axis]) {
        const int la = parent[a], lb = parent[b];
        if (la >= 0 && lb >= 0) out = make_int2(la, lb);
    }
    links[id] = out;
}

__global__ __launch_bounds__(PA_THREADS) void pa_wrap_kernel(int32_t *parent, const int2 *__restrict__ links, int64_t L)
{
    const int64_t id = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    if (id >= L) return;
    const int2 l = links[id];
    if (l.x >= 0 && l.y >= 0) pa_union<PA_AGENT>(parent, l.x, l.y);
}

// size[root] += points.  A wave walks PA_COUNT_ROUNDS x 64 consecutive points; the lanes that hold the same root count once
// (ballot), and the wave keeps the root it met last with its count in (wave-uniform) registers, so that a run of points of one
// component -- the void is mostly one -- costs one atomic per wave, not one per round: 10^7 points of one component would
// otherwise be 10^5 atomics on one word.
constexpr int PA_COUNT_ROUNDS = 16;
__global__ __launch_bounds__(PA_THREADS) void pa_count_kernel(const int32_t *__restrict__ parent, int32_t *__restrict__ size, int64_t G)
{
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = ((int64_t)blockIdx.x * (PA_THREADS / 64) + (threadIdx.x >> 6)) * (64 * PA_COUNT_ROUNDS);
    int run_label = -1, run_count = 0;
    for (int r = 0; r < PA_COUNT_ROUNDS; r++) {
        const int64_t i = wave0 + r * 64 + lane;
        const int lbl = i < G ? parent[i] : -1;
        bool active = lbl >= 0;
        unsigned long long todo = __ballot(active);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int lead = __shfl(lbl, leader, 64);
            const bool mine = active && lbl == lead;
            const unsigned long long same = __ballot(mine);
            if (lead == run_label)
                run_count += (int)__popcll(same);
            else {
                if (run_count > 0 && lane == 0) atomicAdd(size + run_label, run_count);
                run_label = lead;
                run_count = (int)__popcll(same);
            }
            if (mine) active = false;
            todo &= ~same;
        }
    }
    if (run_count > 0 && lane == 0) atomicAdd(size + run_label, run_count);
}

// (root, size) of every component, in no particular order: out[0] counts them
__global__ __launch_bounds__(PA_THREADS) void pa_compact_kernel(const int32_t *__restrict__ parent, const int32_t *__restrict__ size,
                                                                int2 *__restrict__ list, int32_t *__restrict__ out, int64_t G, int64_t cap)
{
    const int64_t i = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    const bool root = i < G && parent[i] == (int32_t)i;
    const unsigned long long roots = __ballot(root);
    if (!roots) return;
    const int lane = threadIdx.x & 63;
    int basis = 0;
    if (lane == __ffsll((long long)roots) - 1) basis = atomicAdd(out, (int)__popcll(roots));
    basis = __shfl(basis, __ffsll((long long)roots) - 1, 64);
    if (root) {
        const int64_t slot = (int64_t)basis + __popcll(roots & ((1ull << lane) - 1ull));
        if (slot < cap) list[slot] = make_int2((int)i, size[i]);
    }
}

__global__ __launch_bounds__(PA_THREADS) void pa_mark_kernel(int32_t *__restrict__ size, const int32_t *__restrict__ roots, int K)
{
    const int k = blockIdx.x * PA_THREADS + threadIdx.x;
    if (k < K) size[roots[k]] = -1;
}

// order-preserving map of a double to u64
__host__ __device__ inline unsigned long long pa_key(double v)
{
    unsigned long long u;
    memcpy(&u, &v, sizeof u);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
inline double pa_unkey(unsigned long long k)
{
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double v;
    memcpy(&v, &u, sizeof v);
    return v;
}

// the largest field value over the points whose root is marked (size < 0): one atomic per wave
__global__ __launch_bounds__(PA_THREADS) void pa_chmax_kernel(const double *__restrict__ field, const int32_t *__restrict__ parent,
                                                              const int32_t *__restrict__ size, int64_t G, unsigned long long *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * PA_THREADS + threadIdx.x;
    unsigned long long key = 0ull;
    if (i < G) {
        const int r = parent[i];
        if (r >= 0 && size[r] < 0) key = pa_key(field[i]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_down(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0 && key) atomicMax(out, key);
}

// ------------------------------------------------------------ host side ----
struct Labeller {
    amof_ctx *ctx = nullptr;
    PaGrid g;               // n, pbc, G
    bool global = false;
    const PoreInputs *in = nullptr;         // the call: thresholds [n_t], want_free
    const PoreOutputs *arrays = nullptr;    // access, free_sphere, labels (access null: the rows are nobody's, amof_pore_psd_field)
    int64_t L = 0;          // slots of the link table
    int64_t cap = 0;        // entries of the component list
    int32_t *parent = nullptr, *size = nullptr, *out = nullptr;        // out: [0] components, [2..3] the u64 of pa_chmax_kernel
    int2 *links = nullptr, *list = nullptr;
    double *sorted = nullptr;
    void *cub_tmp = nullptr;
    size_t cub_bytes = 0;
    int64_t labellings = 0;
    std::vector<int2> h_links, h_list;
    std::vector<int32_t> roots;                 // pa_mark_channels: lives until the copy queued from it has run
    std::vector<WrapLink> wrap;
    std::vector<PeriodicComponent> comps;       // of the last labelling: the periodic components with a wrap link
    WindingResolver resolver;
};

static unsigned pa_blocks(int64_t n) { return (unsigned)std::max<int64_t>(1, (n + PA_THREADS - 1) / PA_THREADS); }

static const char *pa_path(const Labeller &lb) { return lb.global ? "pore_label_global" : "pore_label_tile"; }

// what the call labels and where its answers go; no device work
static void pa_plan(Labeller &lb, amof_ctx *ctx, const PoreInputs &in, const PoreOutputs &out)
{
    const int32_t *grid = in.grid, *pbc = in.pbc;
    lb.ctx = ctx;
    memset(&lb.g, 0, sizeof lb.g);
    for (int k = 0; k < 3; k++) {
        lb.g.n[k] = grid[k];
        lb.g.pbc[k] = pbc[k] ? 1 : 0;
    }
    const int64_t nx = grid[0], ny = grid[1], nz = grid[2];
    lb.g.G = nx * ny * nz;
    lb.L = ny * nz + nx * nz + nx * ny;
    lb.cap = lb.g.G / 2 + 2;        // (no two adjacent points are both roots of one-point components: at most ceil(G / 2) components)
    const char *gl = getenv("AMOF_PORE_LABEL_GLOBAL");
    lb.global = gl && gl[0] == '1';
    lb.in = &in;
    lb.arrays = &out;
}

size_t pore_label_fixed_bytes(const Labeller &lb)
{
    const int64_t G = lb.g.G;
    return (size_t)G * 8 + (size_t)(G / 2 + 2) * 8 + (size_t)lb.L * 8 + (lb.in->want_free ? (size_t)G * 20 : 0);
}

void pore_label_report(const Labeller &lb)
{
    lb.ctx->last_path = pa_path(lb);
    lb.ctx->dom_launches = lb.labellings;
}

int pore_label_setup(Labeller &lb)
{
    amof_ctx *ctx = lb.ctx;
    void *p;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, (size_t)lb.g.G * sizeof(int32_t), &p));
    lb.parent = (int32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX4, (size_t)lb.g.G * sizeof(int32_t), &p));
    lb.size = (int32_t *)p;
    AMOF_TRY(ensure(ctx, SLOT_AUX8, (size_t)lb.cap * sizeof(int2), &p));
    lb.list = (int2 *)p;
    AMOF_TRY(ensure(ctx, SLOT_TILES, (size_t)lb.L * sizeof(int2), &p));
    lb.links = (int2 *)p;
    AMOF_TRY(ensure(ctx, SLOT_SELF, 4 * sizeof(int32_t), &p));
    lb.out = (int32_t *)p;
    if (lb.in->want_free) {
        AMOF_TRY(ensure(ctx, SLOT_PAIRS, (size_t)lb.g.G * sizeof(double), &p));
        lb.sorted = (double *)p;
        lb.cub_bytes = 0;
        AMOF_HIP_TRY(ctx, hipcub::DeviceRadixSort::SortKeys(nullptr, lb.cub_bytes, (const double *)nullptr, lb.sorted, (int)lb.g.G, 0, 64,
                                                            ctx->stream));
        AMOF_TRY(ensure(ctx, SLOT_HISTU, lb.cub_bytes, &lb.cub_tmp));
    }
    return AMOF_OK;
}

// the open labels of V(thr) into parent[], the wrap links to the host, the periodic components that have one resolved
static int pa_open(Labeller &lb, const double *d_field, double thr)
{
    amof_ctx *ctx = lb.ctx;
    PaGrid g = lb.g;
    const int64_t nx = g.n[0], ny = g.n[1], nz = g.n[2];
    if (lb.global) {
        g.t[0] = g.t[1] = g.t[2] = 1;
        hipLaunchKernelGGL(pa_init_kernel, dim3(pa_blocks(g.G)), dim3(PA_THREADS), 0, ctx->stream, d_field, thr, lb.parent, g.G);
    } else {
        g.t[0] = PA_TX;
        g.t[1] = PA_TY;
        g.t[2] = PA_TZ;
        const int64_t ntx = (nx + PA_TX - 1) / PA_TX, nty = (ny + PA_TY - 1) / PA_TY, ntz = (nz + PA_TZ - 1) / PA_TZ;
        hipLaunchKernelGGL(pa_tile_kernel, dim3((unsigned)(ntx * nty * ntz)), dim3(PA_THREADS), 0, ctx->stream, d_field, thr, lb.parent, g,
                           (int)ntz, (int)nty);
    }
    AMOF_HIP_TRY(ctx, hipGetLastError());
    g.nl[0] = (nx - 1) / g.t[0] * ny * nz;
    g.nl[1] = nx * ((ny - 1) / g.t[1]) * nz;
    g.nl[2] = nx * ny * ((nz - 1) / g.t[2]);
    const int64_t n_merge = g.nl[0] + g.nl[1] + g.nl[2];
    if (n_merge > 0) {
        hipLaunchKernelGGL(pa_merge_kernel, dim3(pa_blocks(n_merge)), dim3(PA_THREADS), 0, ctx->stream, lb.parent, g);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(pa_flatten_kernel, dim3(pa_blocks(g.G)), dim3(PA_THREADS), 0, ctx->stream, lb.parent, g.G);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    g.nl[0] = ny * nz;
    g.nl[1] = nx * nz;
    g.nl[2] = nx * ny;
    hipLaunchKernelGGL(pa_links_kernel, dim3(pa_blocks(lb.L)), dim3(PA_THREADS), 0, ctx->stream, (const int32_t *)lb.parent, g, lb.links);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    lb.h_links.resize((size_t)lb.L);
    AMOF_TRY(fetch(ctx, lb.h_links.data(), lb.links, (size_t)lb.L * sizeof(int2)));
    lb.wrap.clear();
    for (int64_t s = 0; s < lb.L; s++) {
        const int2 l = lb.h_links[(size_t)s];
        if (l.x < 0) continue;
        if ((int64_t)l.x >= g.G || l.y < 0 || (int64_t)l.y >= g.G) return fail(ctx, AMOF_EHIP, "pore labelling: a wrap link names no grid point");
        const WrapLink w{l.x, l.y, s < g.nl[0] ? 0 : s < g.nl[0] + g.nl[1] ? 1 : 2};
        // (neighbouring face points mostly join the same two components: a repeated link closes the same cycle again)
        if (!lb.wrap.empty() && lb.wrap.back().lo == w.lo && lb.wrap.back().hi == w.hi && lb.wrap.back().axis == w.axis) continue;
        lb.wrap.push_back(w);
    }
    lb.comps = lb.resolver.resolve(lb.wrap);
    lb.labellings++;
    return AMOF_OK;
}

static bool pa_has_channel(const Labeller &lb)
{
    for (const PeriodicComponent &c : lb.comps)
        if (c.dimension > 0) return true;
    return false;
}

// after pa_periodic: size[root] = -1 for the root of every channel (any: whether there is one)
static int pa_mark_channels(Labeller &lb, bool &any)
{
    amof_ctx *ctx = lb.ctx;
    lb.roots.clear();
    for (const PeriodicComponent &c : lb.comps)
        if (c.dimension > 0) lb.roots.push_back(c.label);
    any = !lb.roots.empty();
    if (!any) return AMOF_OK;
    void *d_roots;
    AMOF_TRY(upload(ctx, SLOT_PERM, lb.roots.data(), lb.roots.size() * sizeof(int32_t), &d_roots));
    hipLaunchKernelGGL(pa_mark_kernel, dim3(pa_blocks((int64_t)lb.roots.size())), dim3(PA_THREADS), 0, ctx->stream, lb.size,
                       (const int32_t *)d_roots, (int)lb.roots.size());
    AMOF_HIP_TRY(ctx, hipGetLastError());
    return AMOF_OK;
}

// after pa_open: the wrap links merged, the periodic labels in parent[], access[4] = accessible points, channels, pockets,
// largest dimension; labels (host [G] or null); chmax (or null): the largest field value over the channels (-inf without one)
static int pa_periodic(Labeller &lb, const double *d_field, int64_t *access, int32_t *labels, double *chmax)
{
    amof_ctx *ctx = lb.ctx;
    const int64_t G = lb.g.G;
    if (!lb.wrap.empty()) {
        hipLaunchKernelGGL(pa_wrap_kernel, dim3(pa_blocks(lb.L)), dim3(PA_THREADS), 0, ctx->stream, lb.parent, (const int2 *)lb.links, lb.L);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        hipLaunchKernelGGL(pa_flatten_kernel, dim3(pa_blocks(G)), dim3(PA_THREADS), 0, ctx->stream, lb.parent, G);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    AMOF_HIP_TRY(ctx, hipMemsetAsync(lb.size, 0, (size_t)G * sizeof(int32_t), ctx->stream));
    AMOF_HIP_TRY(ctx, hipMemsetAsync(lb.out, 0, 4 * sizeof(int32_t), ctx->stream));
    hipLaunchKernelGGL(pa_count_kernel, dim3(pa_blocks((G + PA_COUNT_ROUNDS - 1) / PA_COUNT_ROUNDS)), dim3(PA_THREADS), 0, ctx->stream, (const int32_t *)lb.parent, lb.size, G);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    hipLaunchKernelGGL(pa_compact_kernel, dim3(pa_blocks(G)), dim3(PA_THREADS), 0, ctx->stream, (const int32_t *)lb.parent,
                       (const int32_t *)lb.size, lb.list, lb.out, G, lb.cap);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    int32_t n_comp = 0;
    AMOF_TRY(fetch(ctx, &n_comp, lb.out, sizeof n_comp));
    if (n_comp < 0 || n_comp > lb.cap) return fail(ctx, AMOF_EHIP, "pore labelling: %d components exceed the list", n_comp);
    lb.h_list.resize((size_t)n_comp);
    AMOF_TRY(fetch(ctx, lb.h_list.data(), lb.list, (size_t)n_comp * sizeof(int2)));
    int64_t acc[4] = {0, 0, 0, 0};
    size_t found = 0;
    for (const int2 &c : lb.h_list) {
        auto it = std::lower_bound(lb.comps.begin(), lb.comps.end(), c.x,
                                   [](const PeriodicComponent &pc, int32_t label) { return pc.label < label; });
        const bool known = it != lb.comps.end() && it->label == c.x;
        found += known;
        const int dim = known ? it->dimension : 0;
        if (dim > 0) {
            acc[0] += c.y;
            acc[1]++;
            acc[3] = std::max<int64_t>(acc[3], dim);
        } else
            acc[2]++;
    }
    // the device's periodic roots are the host's: the smallest open label of every tree of wrap links
    if (found != lb.comps.size()) return fail(ctx, AMOF_EHIP, "pore labelling: the periodic labels of device and host disagree");
    for (int k = 0; k < 4; k++) access[k] = acc[k];
    if (labels) AMOF_TRY(fetch(ctx, labels, lb.parent, (size_t)G * sizeof(int32_t)));
    if (chmax) {
        *chmax = -INFINITY;
        bool any = false;
        AMOF_TRY(pa_mark_channels(lb, any));
        if (any) {
            hipLaunchKernelGGL(pa_chmax_kernel, dim3(pa_blocks(G)), dim3(PA_THREADS), 0, ctx->stream, d_field, (const int32_t *)lb.parent,
                               (const int32_t *)lb.size, G, (unsigned long long *)(lb.out + 2));
            AMOF_HIP_TRY(ctx, hipGetLastError());
            unsigned long long key = 0;
            AMOF_TRY(fetch(ctx, &key, lb.out + 2, sizeof key));
            if (key) *chmax = pa_unkey(key);
        }
    }
    return AMOF_OK;
}

// t* of one frame: the largest field value whose void has a channel, by bisection over the sorted field -- channels persist
// when the threshold falls, so "V(sorted[k]) has a channel" is true up to some k and false beyond; ceil(log2(G + 1)) labellings
// without the periodic pass, then one full labelling at t* for the largest value over its channels.
// dmax > 0 (amof_pore_access): t* >= 0 only, (0, 0) without one, +inf where V(dmax) has a channel / where the largest value
// is the cap; dmax <= 0 (amof_pore_access_field): any sign, (-inf, -inf) without a channel.
static int pa_free_sphere(Labeller &lb, const double *d_field, double dmax, double *out2)
{
    amof_ctx *ctx = lb.ctx;
    const int64_t G = lb.g.G;
    AMOF_HIP_TRY(ctx, hipcub::DeviceRadixSort::SortKeys(lb.cub_tmp, lb.cub_bytes, d_field, lb.sorted, (int)G, 0, 64, ctx->stream));
    int64_t lo = -1, hi = G;
    double t_lo = -INFINITY;
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        double t;
        AMOF_TRY(fetch(ctx, &t, lb.sorted + mid, sizeof t));
        if (t == t_lo) {        // (a run of equal values: the answer is known)
            lo = mid;
            continue;
        }
        AMOF_TRY(pa_open(lb, d_field, t));
        if (pa_has_channel(lb)) {
            lo = mid;
            t_lo = t;
        } else
            hi = mid;
    }
    const bool capped = dmax > 0.0;
    if (lo < 0 || (capped && t_lo < 0.0)) {
        out2[0] = out2[1] = capped ? 0.0 : -INFINITY;
        return AMOF_OK;
    }
    if (capped && t_lo >= dmax) {
        out2[0] = out2[1] = INFINITY;
        return AMOF_OK;
    }
    int64_t access[4];
    double chmax;
    AMOF_TRY(pa_open(lb, d_field, t_lo));
    AMOF_TRY(pa_periodic(lb, d_field, access, nullptr, &chmax));
    out2[0] = t_lo + 0.0;
    out2[1] = (capped && chmax >= dmax) ? INFINITY : chmax;
    return AMOF_OK;
}

// every threshold of frame f, whose field lies on the device, then its free sphere.  With a covering stage (want_access) every
// threshold's channels are marked for its accessible pass: that is no labelling, the span of stage 2 is closed around it.
// The surface stage (or null) runs at the same place, on the same marks.
int pore_label_frame(Labeller &lb, int64_t f, const double *d_field, CoverCall *cover, SurfaceCall *surface, StageSpans &spans)
{
    const size_t G = (size_t)lb.g.G;
    int64_t own[4];
    spans.begin(2);
    for (int32_t k = 0; k < lb.in->n_t; k++) {
        const size_t row = (size_t)f * (size_t)lb.in->n_t + (size_t)k;
        AMOF_TRY(pa_open(lb, d_field, lb.in->thresholds[k]));
        AMOF_TRY(pa_periodic(lb, d_field, lb.arrays->access ? lb.arrays->access + row * 4 : own,
                             lb.arrays->labels ? lb.arrays->labels + row * G : nullptr, nullptr));
        if (cover || surface) {
            bool any = false;
            AMOF_TRY(pa_mark_channels(lb, any));
            spans.end();
            if (cover) AMOF_TRY(pore_cover_threshold(*cover, f, k, d_field, lb.parent, lb.size, any, spans));
            if (surface) AMOF_TRY(pore_surface_threshold(*surface, f, k, lb.parent, lb.size, any, spans));
            spans.begin(2);
        }
    }
    const double cap = lb.in->t ? lb.in->dmax : 0.0;        // (of the field from atoms; a supplied field has none)
    if (lb.in->want_free) AMOF_TRY(pa_free_sphere(lb, d_field, cap, lb.arrays->free_sphere + (size_t)f * 2));
    spans.end();
    return AMOF_OK;
}

// the labelling's checks, the same for both entry points (pore_check.h has the order); the record's sizes
static int pa_check(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out)
{
    AMOF_TRY(pore_refuse(ctx, pore_check::grid(in.grid, in.pbc)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_given(in.thresholds, in.n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::thresholds_finite(in.thresholds, in.n_t)));
    AMOF_TRY(pore_refuse(ctx, pore_check::access_outputs(in.n_frames, in.n_t, in.want_free, out.access, out.free_sphere)));
    if (out.labels) AMOF_TRY(pore_refuse(ctx, pore_check::labels_cap(in.n_t, (int64_t)in.grid[0] * in.grid[1] * in.grid[2])));
    out.sized(in.n_frames, in.grid, in.n_t);
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

int amof::pore_access_run(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out, CoverCall *cover, SurfaceCall *surface)
{
    if (in.t) AMOF_TRY(pa_check(ctx, in, out));     // (the entry point of a supplied field has checked already)
    Labeller lb;
    pa_plan(lb, ctx, in, out);
    PoreStages stages{&lb, cover, cover && in.want_access, surface, in.n_t};
    return in.t ? pore_field_run(ctx, in, out, &stages) : pore_given_field_run(ctx, in, out, stages, pa_path(lb));
}

extern "C" int amof_pore_access(amof_ctx *ctx, const amof_traj *t, const double *radii, const int32_t *grid, double dr, double dmax,
                                const double *thresholds, int32_t n_t, int32_t want_free, uint64_t *hist, int64_t *counts, double *vmax,
                                int64_t *argmax, int64_t *access, double *free_sphere, double *field, int32_t *labels)
{
    if (!ctx) return AMOF_EINVAL;
    PoreOutputs out{hist, counts, vmax, argmax, field, access, free_sphere, labels};
    AMOF_TRY(pore_refuse(ctx, pore_check::both_given(t, grid)));
    const int32_t pbc[3] = {t->pbc[0], t->pbc[1], t->pbc[2]};
    return out.keep(pore_access_run(ctx, PoreInputs{t, radii, nullptr, nullptr, t->n_frames, grid, pbc, dr, dmax, thresholds, n_t, 0, want_free}, out, nullptr));
}

extern "C" int amof_pore_access_field(amof_ctx *ctx, const double *field, int64_t n_frames, const int32_t *grid, const int32_t *pbc,
                                      const double *thresholds, int32_t n_t, int32_t want_free, int64_t *access, double *free_sphere,
                                      int32_t *labels)
{
    if (!ctx) return AMOF_EINVAL;
    PoreOutputs out{nullptr, nullptr, nullptr, nullptr, nullptr, access, free_sphere, labels};
    const PoreInputs in{nullptr, nullptr, field, nullptr, n_frames, grid, pbc, 0.0, 0.0, thresholds, n_t, 0, want_free};
    AMOF_TRY(pore_refuse(ctx, pore_check::given_field_inputs(grid, pbc, n_frames, field, false, nullptr)));
    AMOF_TRY(pa_check(ctx, in, out));
    if (n_frames == 0) return AMOF_OK;
    double top;
    AMOF_TRY(pore_refuse(ctx, pore_check::field_finite(field, (size_t)out.F * (size_t)out.G, top)));
    out.zero(false);
    return out.keep(pore_access_run(ctx, in, out, nullptr));
}
