// Internal declarations shared by the translation units of libamofhip.so.
// gfx950 only; compiled with -ffp-contract=off: every fused multiply-add in the
// pair arithmetic is an explicit fma() so that integer results are reproducible
// bit for bit on any conforming IEEE-754 implementation (the CPU oracle).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/amof_hip.h"
#include "guard_math.h"
#include "lag_work.h"
#include "pore_check.h"

namespace amof {

// ---------------------------------------------------------------- context --
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

enum Slot {
    SLOT_POS = 0,   // staged positions (host input)
    SLOT_GEOM,      // per-frame geometry records
    SLOT_IMG,       // per-frame extra image vectors
    SLOT_NIMG,      // per-frame extra image counts
    SLOT_PERM,      // species-sorted atom permutation
    SLOT_TILES,     // tile descriptors
    SLOT_PAIRS,     // tile-pair work list
    SLOT_HISTU,     // unordered-key histograms (u64)
    SLOT_SELF,      // self-image histogram (u64)
    SLOT_SPEC,      // species index per atom
    SLOT_QSPEC,     // species of every atom as a byte (quantize_frame_kernel)
    SLOT_AUX0,
    SLOT_AUX1,
    SLOT_AUX2,
    SLOT_AUX3,
    SLOT_AUX4,
    SLOT_AUX5,
    SLOT_AUX6,
    SLOT_AUX7,
    SLOT_AUX8,
    SLOT_AUX9,
    SLOT_OUT0,
    SLOT_OUT1,
    SLOT_FLAGS,
    SLOT_SURF0,     // the surface stage (pore_surface.hip): cell-sorted records
    SLOT_SURF1,     // its cell offsets
    SLOT_SURF2,     // its keys
    SLOT_SURF3,     // its cursors
    SLOT_SURF4,     // directions, counters, flags
    SLOT_SURF5,     // per-sample bytes of one (frame, threshold)
    SLOT_COUNT
};

}  // namespace amof

struct amof_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipStream_t copy_stream = nullptr;   // host -> device staging that overlaps the kernels of the previous batch
    hipEvent_t ev_copy = nullptr;
    hipEvent_t ev_order = nullptr;       // amof_ctx_wait_stream
    hipEvent_t ev_all0 = nullptr, ev_all1 = nullptr, ev_dom0 = nullptr, ev_dom1 = nullptr;
    bool ev_valid = false;
    int64_t dom_launches = 0;
    std::string err;
    const char *last_path = "";   // kernel family of the last dominant launch (static strings)
    amof::DevBuf buf[amof::SLOT_COUNT];
    // pinned staging ring for the small per-call tables (tile lists, geometry records, work lists ...): a pageable
    // hipMemcpyAsync blocks the host ~40 us per table; from pinned memory it is queued in ~5 us.  The ring is reused
    // from the start after every synchronisation of the context's stream (sync_stream): nothing queued before a
    // synchronisation still reads it.
    unsigned char *pin = nullptr;
    size_t pin_cap = 0, pin_off = 0;
    // page-locked landing area for what the library reads back (flags, result tables): see fetch()
    unsigned char *rb = nullptr;
    size_t rb_cap = 0;
    // amof_msd_shard_begin leaves scratch for amof_msd_shard_finish: valid while no other call ran on the context
    int64_t calls = 0;            // entry points that started device work (timing_begin)
    int64_t progress = 0;         // 2 calls + (the call's dominant kernel is queued): read by OTHER threads (amof_ctx_follow), atomically
    int64_t shard_ticket = 0;     // `calls` right after a begin; 0 = none pending
    int64_t shard_key[7] = {0, 0, 0, 0, 0, 0, 0};
    // kernel seconds of the stages of the last amof_isf_accumulate[_dev]: rho table (with the quantisation), correlation, self;
    // of the last amof_current_accumulate[_dev]: records, table, correlation;
    // of the last amof_bond_survival[_dev]: lists, series, correlations (StageSpans); the fourth: amof_pore_psd's covering stage;
    // the fifth: amof_pore_surface's surface stage
    double stage_seconds[5] = {-1.0, -1.0, -1.0, -1.0, -1.0};
    // of the last amof_pore_psd[_field], over the full passes on "pore_cover_brick": destination bricks, the source bricks they
    // kept, the centre records they swept (amof_pore_cover_stats)
    double cover_stats[3] = {0.0, 0.0, 0.0};
    // of the last amof_pore_surface, over its launches on "pore_surface_list": atoms swept, neighbour records kept, samples,
    // float64 re-decisions, samples ended by the early exit (amof_pore_surface_stats)
    double surface_stats[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    // of the last amof_ring_stats: sources, candidates searched, candidates that closed a ring (amof_ring_search_stats)
    double ring_stats[3] = {0.0, 0.0, 0.0};
    // of the last amof_fragment_stats: frames labelled, labelling rounds summed over them, the most rounds of one frame
    // (amof_fragment_round_stats)
    double fragment_stats[3] = {0.0, 0.0, 0.0};
};

namespace amof {

int fail(amof_ctx *ctx, int code, const char *fmt, ...);
// hipStreamSynchronize(ctx->stream) + reuse of the pinned staging ring
hipError_t sync_stream(amof_ctx *ctx);
int ensure(amof_ctx *ctx, Slot s, size_t bytes, void **out);
// the arguments every entry point of the lag/origin family takes (lag_work.h): windows[W], each in [0, max(F, 1)), stride >= 1
int check_lag_args(amof_ctx *ctx, const int32_t *windows, int32_t W, int64_t F, int64_t stride);
// dst[i] += src[i] on the context's stream: a call's own counters into the caller's device buffer ("_dev" entry points)
int add_into(amof_ctx *ctx, uint64_t *dst, const uint64_t *src, size_t n);
int add_into(amof_ctx *ctx, double *dst, const double *src, size_t n);

#define AMOF_HIP_TRY(ctx, expr)                                                              \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return amof::fail((ctx), AMOF_EHIP, "%s failed: %s (%s:%d)", #expr,              \
                              hipGetErrorString(_e), __FILE__, __LINE__);                    \
    } while (0)

#define AMOF_TRY(expr)            \
    do {                          \
        int _rc = (expr);         \
        if (_rc != AMOF_OK) return _rc; \
    } while (0)

// Raise a kernel's dynamic-LDS cap to everything a workgroup may have besides the kernel's static
// LDS.  The value depends on the kernel (and the device) only, not on the launch, so contexts used from different
// threads cannot undercut each other by setting it for the same kernel -- and it is set once per kernel and device:
// the three runtime calls cost ~10 us, per launch, in front of kernels that one rank of eight runs for 9 ms.
// *static_bytes (optional): the kernel's static LDS.
inline hipError_t allow_max_lds(const void *kern, size_t *static_bytes = nullptr)
{
    static std::mutex mu;
    static std::map<std::pair<const void *, int>, size_t> done;
    int dev = 0, per_block = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> lock(mu);
        auto it = done.find(std::make_pair(kern, dev));
        if (it != done.end()) {
            if (static_bytes) *static_bytes = it->second;
            return hipSuccess;
        }
    }
    e = hipDeviceGetAttribute(&per_block, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e != hipSuccess) return e;
    hipFuncAttributes attr;
    e = hipFuncGetAttributes(&attr, kern);
    if (e != hipSuccess) return e;
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, per_block - (int)attr.sharedSizeBytes);
    if (e != hipSuccess) return e;
    if (static_bytes) *static_bytes = attr.sharedSizeBytes;
    std::lock_guard<std::mutex> lock(mu);
    done[std::make_pair(kern, dev)] = attr.sharedSizeBytes;
    return hipSuccess;
}

// the same for a kernel that takes its dynamic LDS to start at LDS address 0 (rdf_tile_kernel_fast forms histogram addresses
// from integers: bin_count): refused -- loudly, hipErrorInvalidValue -- if the kernel has static LDS in front of it
inline hipError_t allow_max_lds_from_zero(const void *kern)
{
    size_t static_bytes = 0;
    hipError_t e = allow_max_lds(kern, &static_bytes);
    if (e != hipSuccess) return e;
    return static_bytes == 0 ? hipSuccess : hipErrorInvalidValue;
}

// ---- run-time switches to template arguments ----
// Every kernel family is instantiated over a few switches.  The helpers below call f once with the run-time
// switches as std::integral_constant tags, so a family's ladder is one call: with_flags(ortho, cell, [&](auto O, auto C)
// { return launch_lds(kernel<O(), C()>, ...); }).
template <bool V> using Flag = std::integral_constant<bool, V>;
template <int V> using Count = std::integral_constant<int, V>;
template <typename F>
static hipError_t with_flag(bool a, F &&f)
{
    return a ? f(Flag<true>{}) : f(Flag<false>{});
}
template <typename F>
static hipError_t with_flags(bool a, bool b, F &&f)
{
    return with_flag(a, [&](auto A) { return with_flag(b, [&](auto B) { return f(A, B); }); });
}
// v in [0, N) as a Count tag (values beyond N - 1 take the last)
template <int N, typename F>
static hipError_t with_count(int v, F &&f)
{
    if constexpr (N == 1) return f(Count<0>{});
    else return v >= N - 1 ? f(Count<N - 1>{}) : with_count<N - 1>(v, f);
}
// v out of a list of values as a Count tag (a value that is not in the list takes the last)
template <int V0, int... Vs, typename F>
static hipError_t with_value(int v, F &&f)
{
    if constexpr (sizeof...(Vs) == 0) return f(Count<V0>{});
    else return v == V0 ? f(Count<V0>{}) : with_value<Vs...>(v, f);
}
// allow_max_lds + launch + the launch's own error (kernels without dynamic LDS take lds = 0: the cap is then a no-op)
// FROM_ZERO: allow_max_lds_from_zero
template <bool FROM_ZERO = false, typename Kernel, typename... Args>
static hipError_t launch_lds(Kernel kern, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args)
{
    const hipError_t e = FROM_ZERO ? allow_max_lds_from_zero((const void *)kern) : allow_max_lds((const void *)kern);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kern, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// --------------------------------------------------------------- geometry --
// One record per distinct cell: 24 doubles.
//   [0..8]  cell rows          [9..17] cell^-1 with non-periodic columns zeroed
//   [18..20] perpendicular heights   [21] volume   [22] ortho flag   [23] pad
constexpr int GEOM_STRIDE = 24;

struct HostGeom {
    std::vector<double> rec;      // [n_cells][GEOM_STRIDE]
    std::vector<double> invfull;  // [n_cells][9] (host-side use)
    bool all_ortho = true;
    double volume_sum = 0.0;      // over FRAMES (constant cell counted F times)
};

int validate_traj(amof_ctx *ctx, const amof_traj *t, bool need_masses);
int build_geometry(amof_ctx *ctx, const amof_traj *t, HostGeom &g);
// extra periodic images for cutoff R: per cell record a list of lattice vectors
int build_images(amof_ctx *ctx, const amof_traj *t, const HostGeom &g, double R,
                 std::vector<double> &img /* [n_cells][max_img][3] */, std::vector<int32_t> &nimg,
                 int &max_img);

// Error model of the f32 candidate distance of the fast paths (rdf.hip, nbr.hip):
//   q~ = v_sqrt_f32( sum_c d_c^2 ),  d_c = sum_k float(i_k) * s_kc   (s = cell rows * 2^-32 [/ dr])
// With u = 2^-24:  |q~ - q| <= (5 kappa + 3.06) u q, where kappa bounds how much larger than the
// pair vector the summands of d_c can be (cancellation in sheared cells):
//   sum_k |f_k| |C_kc| <= (|d| P)_c,  P = |C^-1| |C|,  kappa = sqrt(||P||_1 ||P||_inf) >= ||P||_2
// (kappa = 1 for a diagonal cell, whose kernels multiply instead of summing: 4.5u + root).
// v_sqrt_f32 on gfx950: <= 1 ulp from correctly rounded, relative error <= 1.56 u, measured
// exhaustively (profiles/tools/sqrt_ulp.hip).  Both bounds carry a further 10 % margin.
// sq_scaled: the diagonal-cell kernel squares the converted differences first and multiplies by the
// squared scales (cvt 1u, square 3u, scale^2 1u, product/fma 5-6-7u on t): 3.5u + root.
inline double fast_guard_rel(const HostGeom &g, int64_t n_cells, bool sq_scaled = false)
{
    const double u = 1.0 / 16777216.0;
    if (g.all_ortho) return 1.1 * ((sq_scaled ? 3.5 : 4.5) + 1.56) * u;
    double kappa = 1.0;
    for (int64_t k = 0; k < n_cells; k++) {
        const double *c = g.rec.data() + (size_t)k * GEOM_STRIDE, *inv = c + 9;
        kappa = std::max(kappa, kappa_cell(c, inv));
    }
    return 1.1 * (5.0 * kappa + 3.06) * u;
}

// species-sorted tiling of the atoms
struct Tile {
    int32_t start;    // offset into perm
    int32_t count;
    int32_t species;
    int32_t _pad;
};
struct HostTiles {
    std::vector<int32_t> perm;     // atoms sorted by species (stable)
    std::vector<Tile> tiles;
    std::vector<int64_t> nsp;      // atoms per species
    std::vector<int64_t> sp_first; // [S + 1] species s owns perm[sp_first[s] .. sp_first[s + 1])
    std::vector<int32_t> sp_first_tile, sp_ntiles;
};
void build_tiles(const amof_traj *t, int tile, HostTiles &out, int granule = 0);

// staging of the position array (host -> device) or pass-through
int stage_positions(amof_ctx *ctx, const amof_traj *t, const double **pos_dev);
// Pipelined variant for kernels that walk the trajectory in frame batches: the device array is
// allocated at once, frames are copied on the context's copy stream only when a batch needs them
// (stager_need), and the compute stream waits on an event -- so the PCIe copy of batch k+1 runs
// while batch k is being computed.  Device-resident and short trajectories degenerate to
// stage_positions.
struct Stager {
    amof_ctx *ctx = nullptr;
    const amof_traj *t = nullptr;
    double *dev = nullptr;
    int64_t upto = 0;       // frames [0, upto) are on the device (or queued ahead of the compute stream)
    bool lazy = false;
};
int stager_begin(amof_ctx *ctx, const amof_traj *t, bool allow_lazy, Stager &st);
int stager_need(Stager &st, int64_t f1);
int upload(amof_ctx *ctx, Slot s, const void *src, size_t bytes, void **out);
// Device -> host of a flag word or a result table, complete on return (the stream is synchronised).  Through page-locked
// memory: with a pageable destination -- a stack variable, the caller's numpy array -- the runtime pins or stages on the
// fly, and the 4-byte flag read after the RDF launch showed as a 0.36 ms copy in the round-5 trace of bench.py.
int fetch(amof_ctx *ctx, void *dst, const void *src_dev, size_t bytes);

// Several small tables in ONE device buffer with ONE host-to-device copy: however small, a copy costs ~5 us of queue time and
// a dozen of them in front of a 0.25 ms kernel were a third of a call.  add() the pieces, upload_pack(), then ptr<T>(i).
struct UploadPack {
    struct Piece {
        const void *src;
        size_t bytes, off;
    };
    std::vector<Piece> pieces;
    size_t total = 0;
    void *base = nullptr;
    int add(const void *src, size_t bytes)
    {
        pieces.push_back(Piece{src, bytes, total});
        total += (bytes + 255) & ~(size_t)255;
        return (int)pieces.size() - 1;
    }
    template <typename T> const T *ptr(int i) const
    {
        return reinterpret_cast<const T *>(static_cast<const unsigned char *>(base) + pieces[(size_t)i].off);
    }
};
int upload_pack(amof_ctx *ctx, Slot s, UploadPack &pk);

// fixed-point atom record of the fast paths: fractional coordinates * 2^32 in the stored
// axis order (slab axis last), original atom index
struct QAtom {
    uint32_t ux, uy, uz, idx;
};
constexpr int QSLABS = 256;

// fold an atom into the cell and quantise its fractional coordinates to 2^-32 (shared by every fast path)
__device__ __forceinline__ QAtom quantize_atom(const double *__restrict__ pos, const double *__restrict__ g,
                                                int64_t N, int f, int64_t a, int ax0, int ax1, int ax2,
                                                int32_t *flag)
{
    const double *__restrict__ p = pos + ((size_t)f * N + a) * 3;
    const double x = p[0], y = p[1], z = p[2];
    uint32_t u[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
        double s = fma(z, g[15 + c], fma(y, g[12 + c], x * g[9 + c]));
        if (!(fabs(s) < 1.0e4)) *flag = 1;   // absurdly far from the cell (or NaN): caller falls back
        s = s - floor(s);
        double t = s * 4294967296.0;
        u[c] = t >= 4294967295.0 ? 0xffffffffu : (uint32_t)t;
    }
    // components are stored in the order (ax0, ax1, ax2): the host puts the slab axis last
    QAtom q;
    q.ux = u[ax0]; q.uy = u[ax1]; q.uz = u[ax2]; q.idx = (uint32_t)a;
    return q;
}

// "Triangular" tile kernel (rdf.hip, TRI): the first two stored coordinates carry the slab coordinate's share of the
// shear, x'' = x + kx z, y' = y + ky z (mod 1; fold = {kx, ky} of the frame's cell), so that the u32 differences of a pair
// are the components of its vector along the orthogonalised lattice directions (see RdfTri in rdf.hip).
__device__ __forceinline__ void fold_atom(QAtom &q, const double *__restrict__ fold)
{
    const double z = (double)q.uz;
    q.ux += (uint32_t)(long long)rint(z * fold[0]);
    q.uy += (uint32_t)(long long)rint(z * fold[1]);
}

// ax0, ax1: the stored order of the two axes that are not the slab axis; d_fold (optional, device [n_cells][2]): fold_atom;
// used_mask: bit s clear = species s (< 64) is neither sorted nor written
int launch_quantize(amof_ctx *ctx, const double *pos_dev, const double *d_geom, int n_cells, const int32_t *d_perm,
                    const int64_t *d_spfirst, int S, int64_t N, int f0, int nf, int axis, QAtom *d_Q,
                    uint32_t *d_slab_start, int32_t *d_flag, int ax0 = -1, int ax1 = -1, const double *d_fold = nullptr,
                    unsigned long long used_mask = ~0ull);

int launch_quantize2(amof_ctx *ctx, const double *pos_dev, const double *d_geom, int n_cells, const int32_t *d_perm,
                     const int64_t *d_spfirst, int S, int64_t N, int f0, int nf, int axis_z, int axis_y, int nz,
                     QAtom *d_Q, uint32_t *d_start2, int32_t *d_flag);

// 3-D cell sort for the cell-list RDF kernel: all atoms of a frame sorted by
// key = ((cz * ny + cy) * nx + cx) * S + species (x fastest),
// d_start3[nf][nkeys + 1] = offsets.
// Q3[.].idx = species << CELL_SPECIES_SHIFT | atom index.  Scratch: d_keys u32 [nf][N],
// d_cursor u32 [nf][nkeys].
constexpr int CELL_SPECIES_SHIFT = 26;
int launch_cell_sort(amof_ctx *ctx, const double *pos_dev, const double *d_geom, int n_cells, const int32_t *d_species,
                     int S, int64_t N, int f0, int nf, int nx, int ny, int nz, QAtom *d_Q3, uint32_t *d_start3,
                     uint32_t *d_keys, uint32_t *d_cursor, int32_t *d_flag);

// 3-D cell sort per species segment for the neighbour kernels (cell counters in LDS: at most CELL_LDS_MAX cells):
// d_Q[nf][N] sorted by (species, cell), d_start3[nf][S * ncell + 1]
constexpr int CELL_LDS_MAX = 16384;
int launch_quantize_cells(amof_ctx *ctx, const double *pos_dev, const double *d_geom, int n_cells, const int32_t *d_perm,
                          const int64_t *d_spfirst, int S, int64_t N, int f0, int nf, int nx, int ny, int nz, QAtom *d_Q,
                          uint32_t *d_start3, int32_t *d_flag, int64_t max_species_atoms, unsigned long long used_mask);

void timing_begin(amof_ctx *ctx);
void timing_end(amof_ctx *ctx);
void timing_dom_begin(amof_ctx *ctx, const char *path);
void timing_dom_end(amof_ctx *ctx, int64_t launches);

// Event pairs around the stages of a call, for amof_last_kernel_seconds 2 .. 6 (ctx->stage_seconds).  A stage may be
// begun many times; end() closes the span begun last.  An event that cannot be created leaves its span out, silently.
struct StageSpans {
    struct Span {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        int stage = 0;
    };
    amof_ctx *ctx;
    std::vector<Span> spans;
    explicit StageSpans(amof_ctx *c) : ctx(c) {}
    StageSpans(const StageSpans &) = delete;
    StageSpans &operator=(const StageSpans &) = delete;
    ~StageSpans()
    {
        for (Span &s : spans) {
            if (s.e0) (void)hipEventDestroy(s.e0);
            if (s.e1) (void)hipEventDestroy(s.e1);
        }
    }
    void begin(int stage)
    {
        Span s;
        s.stage = stage;
        if (hipEventCreate(&s.e0) == hipSuccess && hipEventCreate(&s.e1) == hipSuccess) (void)hipEventRecord(s.e0, ctx->stream);
        spans.push_back(s);
    }
    void end()
    {
        if (!spans.empty() && spans.back().e1) (void)hipEventRecord(spans.back().e1, ctx->stream);
    }
    void collect()      // (the stream has been synchronised)
    {
        for (double &x : ctx->stage_seconds) x = 0.0;
        for (Span &s : spans) {
            float ms = 0.f;
            if (s.e0 && s.e1 && hipEventElapsedTime(&ms, s.e0, s.e1) == hipSuccess) ctx->stage_seconds[s.stage] += (double)ms * 1e-3;
        }
    }
};

// ------------------------------------------------------------------ Pore --
// The host scaffolding of amof_pore_field, amof_pore_access[_field], amof_pore_psd[_field] and amof_pore_surface (pore.hip,
// pore_access.hip, pore_cover.hip, pore_surface.hip).  Every entry point reads: check (pore_check.h), fill PoreOutputs, pick stages, run one field source, finish.
inline int pore_refuse(amof_ctx *ctx, const pore_check::Verdict &v) { return v.code == AMOF_OK ? AMOF_OK : fail(ctx, v.code, "%s", v.text); }

// The caller's arrays as the entry point got them; one it did not ask for is nulled.  F, G, n_t and nbins stay 0 until the checks of
// the arguments that size the arrays have passed.  zero() is the documented "zeros after an error": an entry point calls it once the
// record is complete (without the per-point arrays: success overwrites them in full), the destructor again unless keep(AMOF_OK) ran.
struct PoreOutputs {
    uint64_t *hist = nullptr;           // [F][nbins + 2]
    int64_t *counts = nullptr;          // [F][n_t]
    double *vmax = nullptr;             // [F]
    int64_t *argmax = nullptr;          // [F]
    double *field = nullptr;            // [F][G]
    int64_t *access = nullptr;          // [F][n_t][4]
    double *free_sphere = nullptr;      // [F][2]
    int32_t *labels = nullptr;          // [F][n_t][G]
    uint64_t *psd_hist = nullptr;       // [F][nbins + 2]
    int64_t *po_counts = nullptr, *po_access = nullptr;     // [F][n_t]
    double *cover = nullptr;            // [F][G]
    int64_t *exposed = nullptr, *exposed_access = nullptr;  // [F][n_t][S]
    uint8_t *samples = nullptr;         // [F][n_t][N][M]
    int64_t F = 0, G = 0;
    int64_t S = 0, NM = 0;              // species, atoms x directions (amof_pore_surface alone sets them)
    int32_t nbins = 0, n_t = 0;
    bool kept = false;
    void sized(int64_t frames, const int32_t *grid, int32_t thresholds) { F = frames; G = (int64_t)grid[0] * grid[1] * grid[2]; n_t = thresholds; }
    template <typename T> static void clear(T *p, size_t n) { if (p) std::fill(p, p + n, (T)0); }
    void zero(bool per_point) const
    {
        if (F <= 0) return;
        const size_t f = (size_t)F, g = per_point ? (size_t)G : 0, t = (size_t)n_t, row = nbins > 0 ? (size_t)nbins + 2 : 0;
        clear(hist, f * row), clear(counts, f * t), clear(vmax, f), clear(argmax, f), clear(field, f * g);
        clear(access, f * t * 4), clear(free_sphere, f * 2), clear(labels, f * t * g);
        clear(psd_hist, f * row), clear(po_counts, f * t), clear(po_access, f * t), clear(cover, f * g);
        clear(exposed, f * t * (size_t)S), clear(exposed_access, f * t * (size_t)S), clear(samples, per_point ? f * t * (size_t)NM : 0);
    }
    int keep(int rc) { kept = rc == AMOF_OK; return rc; }
    ~PoreOutputs() { if (!kept) zero(true); }       // (a return without keep() while F == 0 zeroes nothing)
    PoreOutputs(const PoreOutputs &) = delete;      // (a copy would zero the caller's arrays when it dies)
    PoreOutputs &operator=(const PoreOutputs &) = delete;
};

// The arguments of an entry point: atoms (t, radii) or a field of the caller (field [n_frames][G]; cells [n_frames][9]: amof_pore_psd_field)
struct PoreInputs {
    const amof_traj *t;
    const double *radii, *field, *cells;
    int64_t n_frames;
    const int32_t *grid, *pbc;      // pbc [3]: nonzero = periodic
    double dr, dmax;
    const double *thresholds;
    int32_t n_t, want_access, want_free;
};

// What runs on every frame's field while it lies in device memory: the labelling (pore_access.hip) and the covering radius
// (pore_cover.hip), each optional; both states belong to their files.  The surface stage (pore_surface.hip,
// DESIGN.md 4.3e.3) reads no field: it runs where the frame's channel marks are at hand, per (frame, threshold).
struct Labeller;
struct CoverCall;
struct SurfaceCall;
// the device arrays of the call that the stages do not see otherwise: positions [F][N][3], geometry records, radii [S], species [N]
struct PoreAtoms {
    const double *pos, *geom, *radii;
    const int32_t *species;
    const HostGeom *host;
    double rmax, hmin;
};
size_t pore_surface_fixed_bytes(const SurfaceCall &s);
int pore_surface_setup(SurfaceCall &s, const PoreAtoms &atoms);
void pore_surface_restart(SurfaceCall &s);
// threshold k of frame f; parent / mark (or null): the periodic labels and the channel marks of V(thresholds[k]), channels:
// whether there is one
int pore_surface_threshold(SurfaceCall &s, int64_t f, int32_t k, const int32_t *parent, const int32_t *mark, bool channels, StageSpans &spans);
void pore_surface_report(const SurfaceCall &s);
size_t pore_label_fixed_bytes(const Labeller &lb);
int pore_label_setup(Labeller &lb);
int pore_label_frame(Labeller &lb, int64_t f, const double *d_field, CoverCall *cover, SurfaceCall *surface, StageSpans &spans);
void pore_label_report(const Labeller &lb);
size_t pore_cover_fixed_bytes(const CoverCall &c);
int pore_cover_setup(CoverCall &c);
void pore_cover_restart(CoverCall &c);
int pore_cover_frame(CoverCall &c, int64_t f, const double *d_field, StageSpans &spans);
int pore_cover_threshold(CoverCall &c, int64_t f, int32_t k, const double *d_field, const int32_t *parent, const int32_t *mark, bool channels,
                         StageSpans &spans);
void pore_cover_report(const CoverCall &c);
struct PoreStages {
    Labeller *label = nullptr;
    CoverCall *cover = nullptr;
    bool cover_access = false;      // after every labelled threshold: the covering pass from that threshold's channels
    SurfaceCall *surface = nullptr;
    int32_t n_t = 0;                // thresholds of the call (the surface stage without a labeller walks them itself)
    size_t fixed_bytes() const
    {
        return (label ? pore_label_fixed_bytes(*label) : 0) + (cover ? pore_cover_fixed_bytes(*cover) : 0) + (surface ? pore_surface_fixed_bytes(*surface) : 0);
    }
    int setup(const PoreAtoms *atoms = nullptr)
    {
        if (label) AMOF_TRY(pore_label_setup(*label));
        if (cover) AMOF_TRY(pore_cover_setup(*cover));
        return surface && atoms ? pore_surface_setup(*surface, *atoms) : AMOF_OK;
    }
    // pore_brick gave up after its batches ran and pore_exact hands every frame over again: the covering stage's counters
    // (launches, reported path, amof_pore_cover_stats) start over, the labeller's count of labellings goes on
    void restart() { if (cover) pore_cover_restart(*cover); if (surface) pore_surface_restart(*surface); }
    int frame(int64_t f, const double *d_field, StageSpans &spans)
    {
        if (cover) AMOF_TRY(pore_cover_frame(*cover, f, d_field, spans));
        if (label) return pore_label_frame(*label, f, d_field, cover_access ? cover : nullptr, surface, spans);
        for (int32_t k = 0; surface && k < n_t; k++) AMOF_TRY(pore_surface_threshold(*surface, f, k, nullptr, nullptr, false, spans));
        return AMOF_OK;
    }
    void report() const { if (label) pore_label_report(*label); if (cover) pore_cover_report(*cover); if (surface) pore_surface_report(*surface); }
};

// the field from atoms: amof_pore_field's tiers and batches, the stages behind every batch (pore.hip)
int pore_field_run(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out, PoreStages *stages);
// the field the caller supplies: frame by frame into device memory and through the stages; path: what the call reports meanwhile
int pore_given_field_run(amof_ctx *ctx, const PoreInputs &in, const PoreOutputs &out, PoreStages &stages, const char *path);
// the labelling stage on either source, beside a covering stage (amof_pore_psd[_field]) or without (cover null)
int pore_access_run(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out, CoverCall *cover, SurfaceCall *surface = nullptr);
// amof_pore_psd's stages behind the atoms' field -- the covering stage only with want_psd -- and the surface stage (pore_cover.hip)
int pore_psd_surface_run(amof_ctx *ctx, const PoreInputs &in, PoreOutputs &out, bool want_psd, SurfaceCall &surface);

// ---------------------------------------------------------------- LDS-DMA --
typedef __attribute__((address_space(1))) const void *gptr_t;
typedef __attribute__((address_space(3))) void *lptr_t;

// One wave copies 16 B per ACTIVE lane from per-lane global addresses to LDS at dst_wave + 16 * lane
// (dst_wave wave-uniform), without passing through registers (global_load_lds_dwordx4).  Completion is
// tracked by vmcnt: s_waitcnt vmcnt(0) + a barrier before anyone reads the data.
__device__ __forceinline__ void dma16(const void *src_lane, void *dst_wave)
{
    __builtin_amdgcn_global_load_lds((gptr_t)src_lane, (lptr_t)dst_wave, 16, 0, 0);
}

// ------------------------------------------------------- device arithmetic --
// Canonical minimum-image pair vector (see oracle/amof_oracle.c header and
// DESIGN.md "canonical arithmetic").  g points at a geometry record.
template <bool ORTHO>
__device__ __forceinline__ void pair_base(const double *__restrict__ g, double d0x, double d0y,
                                          double d0z, double &dx, double &dy, double &dz)
{
    if (ORTHO) {
        // off-diagonal terms are exact zeros: identical bits to the general form
        double n0 = rint(d0x * g[9]);
        double n1 = rint(d0y * g[13]);
        double n2 = rint(d0z * g[17]);
        dx = fma(-n0, g[0], d0x);
        dy = fma(-n1, g[4], d0y);
        dz = fma(-n2, g[8], d0z);
    } else {
        double s0 = fma(d0z, g[15], fma(d0y, g[12], d0x * g[9]));
        double s1 = fma(d0z, g[16], fma(d0y, g[13], d0x * g[10]));
        double s2 = fma(d0z, g[17], fma(d0y, g[14], d0x * g[11]));
        double n0 = rint(s0), n1 = rint(s1), n2 = rint(s2);
        dx = fma(-n2, g[6], fma(-n1, g[3], fma(-n0, g[0], d0x)));
        dy = fma(-n2, g[7], fma(-n1, g[4], fma(-n0, g[1], d0y)));
        dz = fma(-n2, g[8], fma(-n1, g[5], fma(-n0, g[2], d0z)));
    }
}

__device__ __forceinline__ double norm2(double dx, double dy, double dz)
{
    return fma(dz, dz, fma(dy, dy, dx * dx));
}

// first frame that met a refusal: *flag = 1 + frame unless a smaller one stands there (bounded: the value only falls)
__device__ __forceinline__ void flag_frame(int32_t *flag, int f)
{
    int old = *flag;
    while (old == 0 || old > f + 1) {
        const int seen = atomicCAS(flag, old, f + 1);
        if (seen == old) break;
        old = seen;
    }
}

// ------------------------------------------------------------- bond rows --
// The sorted neighbour rows of the bond graph of frames [f0, f0 + nf) (ring.hip, ring_adjacency_kernel): adj [nf][N][16]
// (-1 behind the neighbours), deg [nf][N]; *flag: flag_frame of the first frame with a 17th neighbour.  amof_ring_stats and
// amof_fragment_stats take their rows from this one launch.
struct BondRows {
    const double *pos;          // [F][N][3] of the call
    const double *geom;
    const int32_t *species;     // [N]
    const double *cutoff;       // [S][S]
    int32_t *adj, *deg, *flag;
    int32_t N, S, n_cells, f0, nf;
};
int launch_bond_rows(amof_ctx *ctx, const BondRows &rows, bool ortho);

}  // namespace amof
