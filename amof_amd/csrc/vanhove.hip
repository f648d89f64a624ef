// Self Van Hove function and the moments of the non-Gaussian parameter (gfx950).
//
// Data path (all float64), the window MSD's transposed one (msd_columns.h: build_step_columns):
//   pos --com_kernel--> com[F][3];  pos, com --delta_transpose_kernel--> D_T[3N][Fp] (wrapped steps, atom-major)
//   D_T --scan_column_kernel (in place)--> U_T: the running positions u_i(k) of amof_msd_window
//   (unwrap: every column transposed and scanned from frame 0's positions, centre of mass from the unwrapped columns,
//    delta_T_kernel re-forms the wrapped steps of the call's atoms, scanned once more)
// then
//   U_T --vanhove_hist_kernel--> counts[S][W][nbins] (u64 atomics), overflow[S][W], part[z][group][W][2] (f64)
//   part --vanhove_reduce_kernel--> moments[S][W][2]   (fixed order: two identical calls give identical bits)
//
// A workgroup owns a group of <= VH_GROUP atoms of one species, a tile of <= VH_LAGS windows and a chunk of time origins.
// Per atom, a thread keeps u(k) of its origins k in registers and walks the tile's lags: u(k + m) streams from the
// column (every load predicated by k + m < F), the bin takes an LDS u32 counter ([tile lags][nbins]); the non-zero
// counters go out with one u64 atomic each at the end.  Histograms that do not fit the LDS budget even for one lag:
// the same kernel with u64 atomics straight into the global counters (msd_vanhove_global).
#include <math.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "msd_columns.h"
#include "msd_select.h"

namespace amof {
namespace {

constexpr int VH_THREADS = 256;         // (block_sum of msd_columns.h: MSD_THREADS)
constexpr int VH_GROUP = 8;             // atoms per workgroup
constexpr int VH_LAGS = 8;              // windows per workgroup (registers: two f64 partials and a counter per window)
constexpr size_t VH_LDS_BUDGET = 64 * 1024;     // u32 counters of a multi-lag tile: two workgroups per CU
// a workgroup adds at most VH_GROUP * VH_ORIGINS samples to one u32 counter: 2^31, no wrap
constexpr int64_t VH_ORIGINS = (int64_t)1 << 28;
static_assert(VH_THREADS == MSD_THREADS, "block_sum reduces MSD_THREADS lanes");

// grid (group, lag tile, origin chunk).  Samples: origins k in [k_begin, k_end) of the chunk with k + m < F, m the
// tile's windows.  r2 = (dx dx + dy dy) + dz dz (no fma: -ffp-contract=off), bin b = (int)(sqrt(r2) / dr) -- the
// comparison q < nbins on the double quotient is the same test as b < nbins without converting a huge q.
template <bool GLOBAL>
__global__ __launch_bounds__(VH_THREADS) void vanhove_hist_kernel(const double *__restrict__ UT, int64_t Fp, int F,
                                                                  const int32_t *__restrict__ perm,
                                                                  const MsdGroup *__restrict__ groups, int n_groups,
                                                                  const int32_t *__restrict__ windows, int W, int lags_per_tile,
                                                                  int64_t k_chunk, double dr, int nbins,
                                                                  unsigned long long *__restrict__ counts,
                                                                  unsigned long long *__restrict__ overflow,
                                                                  double *__restrict__ part)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(lds_raw);     // [nl][nbins] (LDS variant)
    __shared__ double red[2 * (MSD_THREADS / 64)];
    const MsdGroup gr = groups[blockIdx.x];
    const int w0 = blockIdx.y * lags_per_tile;
    const int nl = min(lags_per_tile, W - w0);
    const int64_t k_begin = 1 + (int64_t)blockIdx.z * k_chunk;
    int m[VH_LAGS];
    int mmin = F;
#pragma unroll
    for (int l = 0; l < VH_LAGS; l++) {
        m[l] = l < nl ? windows[w0 + l] : F;        // (F: no origin satisfies k + m < F)
        mmin = min(mmin, m[l]);
    }
    const int64_t k_end = min(k_begin + k_chunk, (int64_t)F - mmin);   // origins with at least one sample
    if (!GLOBAL) {
        for (int i = threadIdx.x; i < nl * nbins; i += VH_THREADS) hist[i] = 0u;
        __syncthreads();
    }
    unsigned long long *__restrict__ gcount = counts + ((size_t)gr.species * W + w0) * (size_t)nbins;
    double s2[VH_LAGS], s4[VH_LAGS];
    uint32_t ov[VH_LAGS];
#pragma unroll
    for (int l = 0; l < VH_LAGS; l++) { s2[l] = 0.0; s4[l] = 0.0; ov[l] = 0u; }
    const double fnb = (double)nbins;
    for (int c = 0; c < gr.count; c++) {
        const int64_t atom = perm[gr.start + c];
        const double *__restrict__ ux = UT + (size_t)(3 * atom) * Fp;
        const double *__restrict__ uy = ux + Fp;
        const double *__restrict__ uz = uy + Fp;
        for (int64_t k = k_begin + threadIdx.x; k < k_end; k += VH_THREADS) {
            const double x0 = ux[k], y0 = uy[k], z0 = uz[k];            // k < F - mmin <= F
#pragma unroll
            for (int l = 0; l < VH_LAGS; l++) {
                const int64_t k1 = k + m[l];
                if (k1 < F) {
                    const double dx = ux[k1] - x0, dy = uy[k1] - y0, dz = uz[k1] - z0;
                    const double r2 = (dx * dx + dy * dy) + dz * dz;
                    s2[l] += r2;
                    s4[l] += r2 * r2;
                    const double q = sqrt(r2) / dr;
                    if (q < fnb) {
                        const int b = (int)q;
                        if (GLOBAL) atomicAdd(&gcount[(size_t)l * nbins + b], 1ull);
                        else atomicAdd(&hist[l * nbins + b], 1u);
                    } else {
                        ov[l]++;
                    }
                }
            }
        }
    }
    if (!GLOBAL) {
        __syncthreads();
        for (int i = threadIdx.x; i < nl * nbins; i += VH_THREADS) {
            const uint32_t v = hist[i];
            if (v) atomicAdd(&gcount[i], (unsigned long long)v);
        }
    }
    // per-workgroup moment slots (one writer each) and the overflow counts (integers below 2^53: exact as doubles)
#pragma unroll
    for (int l = 0; l < VH_LAGS; l++) {
        if (l < nl) {
            const double t2 = block_sum(s2[l], red);
            const double t4 = block_sum(s4[l], red);
            const double to = block_sum((double)ov[l], red);
            if (threadIdx.x == 0) {
                double *o = part + (((size_t)blockIdx.z * n_groups + blockIdx.x) * W + (w0 + l)) * 2;
                o[0] = t2;
                o[1] = t4;
                if (to > 0.0) atomicAdd(&overflow[(size_t)gr.species * W + w0 + l], (unsigned long long)to);
            }
        }
    }
}

// moments[s][w][.] = sum over the origin chunks and the groups of species s of the slots: one workgroup per (s, w)
__global__ __launch_bounds__(MSD_THREADS) void vanhove_reduce_kernel(const double *__restrict__ part, int n_chunks, int n_groups,
                                                                     const int32_t *__restrict__ sp_group_first, int W,
                                                                     double *__restrict__ moments)
{
    __shared__ double red[2 * (MSD_THREADS / 64)];
    const int s = blockIdx.x / W, w = blockIdx.x % W;
    const int g0 = sp_group_first[s], ng = sp_group_first[s + 1] - g0;
    double a2 = 0.0, a4 = 0.0;
    for (int q = threadIdx.x; q < n_chunks * ng; q += MSD_THREADS) {
        const int z = q / ng, g = g0 + q % ng;
        const double *p = part + (((size_t)z * n_groups + g) * W + w) * 2;
        a2 += p[0];
        a4 += p[1];
    }
    a2 = block_sum(a2, red);
    a4 = block_sum(a4, red);
    if (threadIdx.x == 0) {
        moments[2 * (size_t)blockIdx.x] = a2;
        moments[2 * (size_t)blockIdx.x + 1] = a4;
    }
}

// host outputs (counts, overflow, moments: overwritten) or device outputs (counts_dev, overflow_dev, moments_dev: added into)
int vanhove_run(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int32_t unwrap, int32_t remove_com,
                int64_t atom_begin, int64_t atom_end, double dr, int32_t nbins, const double *com_ext, uint64_t *counts,
                uint64_t *overflow, double *moments, uint64_t *counts_dev, uint64_t *overflow_dev, double *moments_dev)
{
    AMOF_TRY(validate_traj(ctx, t, remove_com != 0));
    const int S = t->n_species;
    const int64_t N = t->n_atoms, F = t->n_frames;
    if (W < 0 || (W > 0 && !windows)) return fail(ctx, AMOF_EINVAL, "NULL argument");
    if (atom_begin < 0 || atom_end > N || atom_begin > atom_end) return fail(ctx, AMOF_EINVAL, "bad atom range");
    if (!(dr > 0.0) || !isfinite(dr)) return fail(ctx, AMOF_EINVAL, "dr must be positive and finite");
    if (nbins < 0) return fail(ctx, AMOF_EINVAL, "nbins must be >= 0");
    if (com_ext && unwrap) return fail(ctx, AMOF_EINVAL, "a precomputed centre of mass cannot be combined with unwrap");
    for (int w = 0; w < W; w++)
        if (windows[w] < 0 || (F > 0 && windows[w] >= F)) return fail(ctx, AMOF_EINVAL, "window %d out of range", windows[w]);
    if ((size_t)S * (size_t)W * (size_t)nbins > ((size_t)1 << 40)) return fail(ctx, AMOF_EINVAL, "histogram too large");
    if (counts) {
        std::fill(counts, counts + (size_t)S * W * nbins, (uint64_t)0);
        std::fill(overflow, overflow + (size_t)S * W, (uint64_t)0);
        std::fill(moments, moments + (size_t)S * W * 2, 0.0);
    }
    if (F == 0 || N == 0 || W == 0 || atom_begin == atom_end) return AMOF_OK;
    if (F > 0x7fffffffLL) return fail(ctx, AMOF_EINVAL, "too many frames");

    HostGeom hg;
    AMOF_TRY(build_geometry(ctx, t, hg));
    std::vector<double> grec;
    msd_geom_records(t, hg, grec);
    // species-sorted groups of the selected atoms
    SpeciesGroups sg;
    species_groups(t->species, atom_begin, atom_end, S, VH_GROUP, sg);
    const int n_groups = (int)sg.groups.size();
    double total_mass = 0.0;
    if (remove_com)
        for (int64_t i = 0; i < N; i++) total_mass += t->masses[i];

    // lag tiles: as many windows as fit the LDS budget (at most VH_LAGS), spread evenly over the tiles; one lag per tile up to
    // AMOF_MAX_LDS_BINS counters (one workgroup per CU); beyond that, or on request (AMOF_VANHOVE_GLOBAL=1), global counters
    const size_t hist_bytes = (size_t)std::max(nbins, 1) * sizeof(uint32_t);
    const bool global = nbins > AMOF_MAX_LDS_BINS || getenv("AMOF_VANHOVE_GLOBAL");
    int per_tile = global ? VH_LAGS : (int)std::max<size_t>(1, std::min<size_t>(VH_LAGS, VH_LDS_BUDGET / hist_bytes));
    per_tile = std::min<int>(per_tile, W);
    const int n_tiles = (W + per_tile - 1) / per_tile;
    per_tile = (W + n_tiles - 1) / n_tiles;
    const int64_t k_chunk = std::min<int64_t>(std::max<int64_t>(F - 1, 1), VH_ORIGINS);
    const int n_chunks = (int)((std::max<int64_t>(F - 1, 1) + k_chunk - 1) / k_chunk);
    if (n_tiles > 65535 || n_chunks > 65535) return fail(ctx, AMOF_EINVAL, "too many windows or frames");

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
    const int64_t Fp = (F + 31) / 32 * 32;
    UploadPack pk;
    const int i_geom = pk.add(grec.data(), grec.size() * sizeof(double));
    const int i_perm = pk.add(sg.perm.data(), sg.perm.size() * sizeof(int32_t));
    const int i_groups = pk.add(sg.groups.data(), sg.groups.size() * sizeof(MsdGroup));
    const int i_win = pk.add(windows, (size_t)W * sizeof(int32_t));
    const int i_sgf = pk.add(sg.group_first.data(), sg.group_first.size() * sizeof(int32_t));
    const int i_mass = remove_com ? pk.add(t->masses, (size_t)N * sizeof(double)) : -1;
    AMOF_TRY(upload_pack(ctx, SLOT_GEOM, pk));
    const double *d_geom = pk.ptr<double>(i_geom), *d_mass = remove_com ? pk.ptr<double>(i_mass) : nullptr;
    const int32_t *d_perm = pk.ptr<int32_t>(i_perm), *d_win = pk.ptr<int32_t>(i_win), *d_sgf = pk.ptr<int32_t>(i_sgf);
    const MsdGroup *d_groups = pk.ptr<MsdGroup>(i_groups);
    void *d_part = nullptr, *d_mom = nullptr, *d_cnt = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX5, (size_t)n_chunks * n_groups * W * 2 * sizeof(double), &d_part));
    AMOF_TRY(ensure(ctx, SLOT_OUT0, (size_t)S * W * 2 * sizeof(double), &d_mom));
    unsigned long long *cnt = reinterpret_cast<unsigned long long *>(counts_dev), *ovf = reinterpret_cast<unsigned long long *>(overflow_dev);
    if (counts) {       // host call: the counters start from zero in scratch
        const size_t cbytes = ((size_t)S * W * nbins + (size_t)S * W) * sizeof(uint64_t);
        AMOF_TRY(ensure(ctx, SLOT_OUT1, cbytes, &d_cnt));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_cnt, 0, cbytes, ctx->stream));
        cnt = (unsigned long long *)d_cnt;
        ovf = cnt + (size_t)S * W * nbins;
    }

    // ---- the running positions u_i(k) of the call's atoms, as amof_msd_window forms them: its step columns, scanned ----
    const ColumnsIn cols = {pos_dev, d_geom, hg.all_ortho, d_mass, total_mass, unwrap != 0, remove_com != 0, com_ext};
    double *d_DT = nullptr;
    AMOF_TRY(build_step_columns(ctx, t, cols, atom_begin, atom_end, &d_DT));
    double *range_cols = d_DT + (size_t)3 * atom_begin * Fp;
    const unsigned n_cols = (unsigned)(3 * (atom_end - atom_begin));
    hipLaunchKernelGGL(scan_column_kernel, dim3(n_cols), dim3(MSD_THREADS), 0, ctx->stream, (const double *)range_cols,
                       (const double *)nullptr, Fp, (int)F, range_cols);
    AMOF_HIP_TRY(ctx, hipGetLastError());

    // ---- histograms and moment slots ----
    const dim3 grid((unsigned)n_groups, (unsigned)n_tiles, (unsigned)n_chunks);
    if (global) {
        timing_dom_begin(ctx, "msd_vanhove_global");
        hipLaunchKernelGGL(vanhove_hist_kernel<true>, grid, dim3(VH_THREADS), 0, ctx->stream, (const double *)d_DT, Fp, (int)F, d_perm,
                           d_groups, n_groups, d_win, (int)W, per_tile, k_chunk, dr, (int)nbins, cnt, ovf, (double *)d_part);
    } else {
        AMOF_HIP_TRY(ctx, allow_max_lds((const void *)vanhove_hist_kernel<false>));
        timing_dom_begin(ctx, "msd_vanhove");
        hipLaunchKernelGGL(vanhove_hist_kernel<false>, grid, dim3(VH_THREADS), (size_t)per_tile * hist_bytes, ctx->stream,
                           (const double *)d_DT, Fp, (int)F, d_perm, d_groups, n_groups, d_win, (int)W, per_tile, k_chunk, dr,
                           (int)nbins, cnt, ovf, (double *)d_part);
    }
    AMOF_HIP_TRY(ctx, hipGetLastError());
    timing_dom_end(ctx, 1);
    hipLaunchKernelGGL(vanhove_reduce_kernel, dim3((unsigned)(S * W)), dim3(MSD_THREADS), 0, ctx->stream, (const double *)d_part,
                       n_chunks, n_groups, d_sgf, (int)W, (double *)d_mom);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    if (moments_dev) AMOF_TRY(add_into(ctx, moments_dev, (const double *)d_mom, (size_t)2 * S * W));
    timing_end(ctx);
    if (counts) {
        AMOF_TRY(fetch(ctx, counts, cnt, (size_t)S * W * nbins * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, overflow, ovf, (size_t)S * W * sizeof(uint64_t)));
        AMOF_TRY(fetch(ctx, moments, d_mom, (size_t)S * W * 2 * sizeof(double)));
    }
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_vanhove_window(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int32_t unwrap,
                                   int32_t remove_com, int64_t atom_begin, int64_t atom_end, double dr, int32_t nbins,
                                   uint64_t *counts, uint64_t *overflow, double *moments)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !overflow || !moments) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return vanhove_run(ctx, t, windows, W, unwrap, remove_com, atom_begin, atom_end, dr, nbins, nullptr, counts, overflow, moments,
                       nullptr, nullptr, nullptr);
}

extern "C" int amof_vanhove_window_dev(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int32_t unwrap,
                                       int32_t remove_com, int64_t atom_begin, int64_t atom_end, double dr, int32_t nbins,
                                       const double *com_dev, uint64_t *counts_dev, uint64_t *overflow_dev, double *moments_dev)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !overflow_dev || !moments_dev) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return vanhove_run(ctx, t, windows, W, unwrap, remove_com, atom_begin, atom_end, dr, nbins, com_dev, nullptr, nullptr, nullptr,
                       counts_dev, overflow_dev, moments_dev);
}
