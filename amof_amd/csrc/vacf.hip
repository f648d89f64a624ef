// Velocity autocorrelation: sums of x(k) x(k + m) over atoms, coordinates and time origins (gfx950).
//
// Data path (all float64):
//   positions mode   pos --build_step_columns (msd_columns.h)--> D_T[3N][Fp]: wrapped steps, centre of mass removed, atom-major
//   velocity mode    vel --com_kernel--> mean[F][3];  vel, mean --velocity_transpose_kernel--> D_T[3N][Fp] (no wrap, no cell)
// then
//   D_T --vacf_lds_kernel | vacf_general_kernel--> part[n_blocks][W]   (a block: <= VACF_GROUP atoms of one species)
//   part --vacf_reduce_kernel--> sums[S][W]                            (blocks of a species in order)
//
// The order of summation is fixed and the same in both kernels: one accumulator per (block, lag), updated with __fma_rn over
// the block's columns in column order and, within a column, over the origins k ascending.  vacf_lds adds products beyond the
// end of a series too: they are +-0 (zeros stand behind the column in LDS) and leave the accumulator's bits as they are (it
// starts at +0 and a sum in round-to-nearest never gives -0 from there).  No float atomics: identical calls, identical bits.
// Which kernel, the lag tiles, one column buffer or two: vacf_select.h.  AMOF_VACF_GENERAL=1: never vacf_lds; AMOF_VACF_NODB=1 /
// AMOF_VACF_DB=1: vacf_lds with one / with two column buffers where the rule says otherwise (tests, measurements).
#include <math.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "msd_columns.h"
#include "vacf_select.h"

namespace amof {
namespace {

constexpr int VT_TF = 32, VT_TA = 32, VT_THREADS = 256;     // velocity transposition: tile of frames x atoms
constexpr int VACF_PF = 4;          // vacf_lds: entries of the next column a thread holds in flight
constexpr int VACF_PQ = 48;         // ... across this many unrolled passes (48 x 11 x 11 fmas: beyond a memory latency)

// D_T[3a + c][k] = vel[k][a][c] - mean[k][c] (mean == nullptr: as given), k < F; zeros up to Fp.  Atoms [a_begin, a_end).
__global__ __launch_bounds__(VT_THREADS) void velocity_transpose_kernel(const double *__restrict__ vel, const double *__restrict__ mean,
                                                                        int64_t N, int F, int64_t Fp, int64_t a_begin, int64_t a_end,
                                                                        double *__restrict__ DT)
{
    __shared__ double tile[VT_TF][3 * VT_TA + 1];
    const int k0 = blockIdx.y * VT_TF;
    const int64_t a0 = a_begin + (int64_t)blockIdx.x * VT_TA;
    for (int idx = threadIdx.x; idx < VT_TF * 3 * VT_TA; idx += VT_THREADS) {
        const int kl = idx / (3 * VT_TA), e = idx % (3 * VT_TA);
        const int k = k0 + kl;
        double v = 0.0;
        if (k < F && a0 + e / 3 < a_end) {
            v = vel[((size_t)k * (size_t)N + (size_t)a0) * 3 + e];
            if (mean) v -= mean[3 * (size_t)k + e % 3];
        }
        tile[kl][e] = v;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < VT_TF * 3 * VT_TA; idx += VT_THREADS) {
        const int cl = idx / VT_TF, kl = idx % VT_TF;
        // (k0 + kl < Fp: the grid covers Fp / VT_TF tiles of frames exactly)
        if (a0 + cl / 3 < a_end) DT[(size_t)(3 * a0 + cl) * Fp + k0 + kl] = tile[kl][cl];
    }
}

__device__ __forceinline__ const double *block_column(const double *__restrict__ DT, int64_t Fp, const int32_t *__restrict__ perm,
                                                      const MsdGroup &gr, int c)
{
    return DT + (size_t)(3 * (int64_t)perm[gr.start + c / 3] + c % 3) * Fp;
}

// grid (block of atoms, lag tile), blockDim.x = lanes of the plan; lags m = w (consecutive from 0), origin stride 1.
// LDS: [DB ? 2 : 1][L] doubles, L = F + tail: a column and the zeros behind it.  A lane owns the R lags from
// m0 = tile_lags blockIdx.y + R lane and keeps p[q] = v(k + m0 + q) in registers; the pass over R origins is unrolled so that
// the window rotates by renaming.  A wave stops at the last origin of its smallest lag.
// Reads of a column's buffer: v(k + s), k + s <= F - 1 + R - 1, and v(k + s + R + m0), at most F + 65 R - 2 < L (vacf_select).
// DB: the entries j < F of the NEXT column (none behind the block's last) are loaded VACF_PF per thread ahead of VACF_PQ passes
// and parked in the other buffer behind them; what the passes did not cover is copied behind the loop.  Every such load is
// predicated by j < F <= Fp: nothing is read past a column's own entries, nor behind the block's last column.
// !DB: the next column is loaded between two barriers; the CU's other workgroup computes meanwhile.
template <bool DB>
__global__ __launch_bounds__(VACF_MAX_LANES) void vacf_lds_kernel(const double *__restrict__ DT, int64_t Fp, int F,
                                                                  const int32_t *__restrict__ perm,
                                                                  const MsdGroup *__restrict__ groups, int W, int tile_lags, int L,
                                                                  double *__restrict__ part)
{
    constexpr int R = VACF_R;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double *buf = reinterpret_cast<double *>(lds_raw);
    const MsdGroup gr = groups[blockIdx.x];
    const int T = blockDim.x, tid = threadIdx.x;
    const int m0 = blockIdx.y * tile_lags + tid * R;
    const int wave_m0 = blockIdx.y * tile_lags + (tid & ~63) * R;
    const int kend = wave_m0 < W ? F - wave_m0 : 0;     // origins 1 .. kend - 1 (wave-uniform; a wave of padding lanes has none)
    const int ncols = 3 * gr.count;
    for (int b = 0; b < (DB ? 2 : 1); b++)
        for (int i = F + tid; i < L; i += T) buf[(size_t)b * L + i] = 0.0;
    {
        const double *__restrict__ g0 = block_column(DT, Fp, perm, gr, 0);
        for (int j = tid; j < F; j += T) buf[j] = g0[j];
    }
    __syncthreads();
    double acc[R];
#pragma unroll
    for (int r = 0; r < R; r++) acc[r] = 0.0;
    for (int c = 0; c < ncols; c++) {
        const double *cur = buf + (DB ? (size_t)(c & 1) * L : 0);
        double *nxt = buf + (DB ? (size_t)((c + 1) & 1) * L : 0);
        const bool more = c + 1 < ncols;
        const double *__restrict__ gnext = more ? block_column(DT, Fp, perm, gr, c + 1) : DT;
        int j = DB && more ? tid : F;                   // next entry of the next column this thread fetches
        if (kend > 1) {
            double p[R];
#pragma unroll
            for (int r = 0; r < R; r++) p[r] = cur[1 + m0 + r];
            int k = 1;
            while (k < kend) {
                double nx[VACF_PF];
                if (DB) {
#pragma unroll
                    for (int q = 0; q < VACF_PF; q++) nx[q] = j + q * T < F ? gnext[j + q * T] : 0.0;
                }
                for (int it = 0; it < VACF_PQ && k < kend; it++, k += R) {
#pragma unroll
                    for (int s = 0; s < R; s++) {
                        const double a = cur[k + s];
#pragma unroll
                        for (int r = 0; r < R; r++) acc[r] = __fma_rn(a, p[(s + r) % R], acc[r]);
                        p[s] = cur[k + s + R + m0];
                    }
                }
                if (DB) {
#pragma unroll
                    for (int q = 0; q < VACF_PF; q++)
                        if (j + q * T < F) nxt[j + q * T] = nx[q];
                    j = min(j + VACF_PF * T, F);
                }
            }
        }
        if (DB)
            for (; j < F; j += T) nxt[j] = gnext[j];
        __syncthreads();
        if (!DB && more) {
            for (int i = tid; i < F; i += T) buf[i] = gnext[i];
            __syncthreads();
        }
    }
#pragma unroll
    for (int r = 0; r < R; r++)
        if (m0 + r < W) part[(size_t)blockIdx.x * W + m0 + r] = acc[r];
}

// grid (block of atoms, chunk of lags): one thread per (block, lag), the columns read from device memory; any window list, any
// origin stride, any series length.  Origins k = 1 + stride o, o < n(m): k + m <= F - 1.
__global__ __launch_bounds__(VACF_GEN_THREADS) void vacf_general_kernel(const double *__restrict__ DT, int64_t Fp, int F,
                                                                        const int32_t *__restrict__ perm,
                                                                        const MsdGroup *__restrict__ groups,
                                                                        const int32_t *__restrict__ windows, int W, int64_t stride,
                                                                        double *__restrict__ part)
{
    const int w = blockIdx.y * VACF_GEN_THREADS + threadIdx.x;
    if (w >= W) return;
    const MsdGroup gr = groups[blockIdx.x];
    const int64_t m = windows[w];
    const int64_t n = (int64_t)F - m - 2 >= 0 ? ((int64_t)F - m - 2) / stride + 1 : 0;
    double acc = 0.0;
    for (int c = 0; c < 3 * gr.count; c++) {
        const double *__restrict__ x = block_column(DT, Fp, perm, gr, c);
        for (int64_t o = 0; o < n; o++) {
            const int64_t k = 1 + stride * o;
            acc = __fma_rn(x[k], x[k + m], acc);
        }
    }
    part[(size_t)blockIdx.x * W + w] = acc;
}

// sums[s][w] = the partials of species s's blocks, added in block order: one thread per (s, w)
__global__ __launch_bounds__(MSD_THREADS) void vacf_reduce_kernel(const double *__restrict__ part, const int32_t *__restrict__ sp_group_first,
                                                                  int S, int W, double *__restrict__ sums)
{
    const int64_t idx = (int64_t)blockIdx.x * MSD_THREADS + threadIdx.x;
    if (idx >= (int64_t)S * W) return;
    const int s = (int)(idx / W), w = (int)(idx % W);
    double a = 0.0;
    for (int g = sp_group_first[s]; g < sp_group_first[s + 1]; g++) a += part[(size_t)g * W + w];
    sums[idx] = a;
}

// host output (sums: overwritten) or device output (sums_dev: added into)
int vacf_run(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int64_t origin_stride, int32_t velocity_mode,
             int32_t remove_com, int64_t atom_begin, int64_t atom_end, const double *com_ext, double *sums, double *sums_dev)
{
    AMOF_TRY(validate_traj(ctx, t, remove_com != 0));
    const int S = t->n_species;
    const int64_t N = t->n_atoms, F = t->n_frames;
    AMOF_TRY(check_lag_args(ctx, windows, W, F, origin_stride));
    if (atom_begin < 0 || atom_end > N || atom_begin > atom_end) return fail(ctx, AMOF_EINVAL, "bad atom range");
    if (sums) std::fill(sums, sums + (size_t)S * W, 0.0);
    if (F < 2 || N == 0 || W == 0 || atom_begin == atom_end) return AMOF_OK;
    if (F > 0x7fffffffLL - 4096) return fail(ctx, AMOF_EINVAL, "too many frames");

    const VacfPlan plan = vacf_select(F, W, windows, origin_stride, VacfSwitches::from_env());
    SpeciesGroups sg;
    species_groups(t->species, atom_begin, atom_end, S, VACF_GROUP, sg);
    const int n_blocks = (int)sg.groups.size();
    const int64_t Fp = (F + 31) / 32 * 32;
    const unsigned lag_chunks = (unsigned)((W + VACF_GEN_THREADS - 1) / VACF_GEN_THREADS);
    if (lag_chunks > 65535 || Fp / VT_TF > 65535) return fail(ctx, AMOF_EINVAL, "too many windows or frames");
    double total_mass = 0.0;
    if (remove_com)
        for (int64_t i = 0; i < N; i++) total_mass += t->masses[i];
    HostGeom hg;
    std::vector<double> grec;
    if (!velocity_mode) {
        AMOF_TRY(build_geometry(ctx, t, hg));
        msd_geom_records(t, hg, grec);
    }

    AMOF_HIP_TRY(ctx, hipSetDevice(ctx->device));
    timing_begin(ctx);
    StageSpans spans(ctx);      // columns, correlation
    const double *pos_dev = nullptr;
    AMOF_TRY(stage_positions(ctx, t, &pos_dev));
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
    void *d_part = nullptr, *d_sums = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX5, (size_t)n_blocks * W * sizeof(double), &d_part));
    AMOF_TRY(ensure(ctx, SLOT_OUT0, (size_t)S * W * sizeof(double), &d_sums));

    // ---- the columns of the call's atoms ----
    spans.begin(0);
    double *d_DT = nullptr;
    if (!velocity_mode) {
        const ColumnsIn cols = {pos_dev, d_geom, hg.all_ortho, d_mass, total_mass, false, remove_com != 0, com_ext};
        AMOF_TRY(build_step_columns(ctx, t, cols, atom_begin, atom_end, &d_DT));
    } else {
        void *d_cols = nullptr, *d_mean = nullptr;
        AMOF_TRY(ensure(ctx, SLOT_AUX3, (size_t)3 * N * Fp * sizeof(double), &d_cols));
        const double *mean = nullptr;
        if (remove_com && com_ext) {
            mean = com_ext;
        } else if (remove_com) {
            AMOF_TRY(ensure(ctx, SLOT_AUX2, (size_t)F * 3 * sizeof(double), &d_mean));
            hipLaunchKernelGGL(com_kernel, dim3((unsigned)F), dim3(MSD_THREADS), 0, ctx->stream, pos_dev, d_mass, N, total_mass,
                               (double *)d_mean);
            mean = (const double *)d_mean;
        }
        const dim3 grid((unsigned)((atom_end - atom_begin + VT_TA - 1) / VT_TA), (unsigned)(Fp / VT_TF));
        hipLaunchKernelGGL(velocity_transpose_kernel, grid, dim3(VT_THREADS), 0, ctx->stream, pos_dev, mean, N, (int)F, Fp, atom_begin,
                           atom_end, (double *)d_cols);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        d_DT = (double *)d_cols;
    }
    spans.end();

    // ---- block partials, then the sums ----
    spans.begin(1);
    timing_dom_begin(ctx, plan.path);
    if (plan.kernel == VACF_LDS) {
        const dim3 grid((unsigned)n_blocks, (unsigned)plan.n_tiles);
        AMOF_HIP_TRY(ctx, with_flag(plan.db, [&](auto DB) {
            return launch_lds(vacf_lds_kernel<DB()>, grid, dim3((unsigned)plan.lanes), plan.lds, ctx->stream, (const double *)d_DT, Fp,
                              (int)F, d_perm, d_groups, (int)W, plan.tile_lags, (int)plan.series, (double *)d_part);
        }));
    } else {
        hipLaunchKernelGGL(vacf_general_kernel, dim3((unsigned)n_blocks, lag_chunks), dim3(VACF_GEN_THREADS), 0, ctx->stream,
                           (const double *)d_DT, Fp, (int)F, d_perm, d_groups, d_win, (int)W, origin_stride, (double *)d_part);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    timing_dom_end(ctx, 1);
    hipLaunchKernelGGL(vacf_reduce_kernel, dim3((unsigned)(((size_t)S * W + MSD_THREADS - 1) / MSD_THREADS)), dim3(MSD_THREADS), 0,
                       ctx->stream, (const double *)d_part, d_sgf, S, (int)W, (double *)d_sums);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    spans.end();
    if (sums_dev) AMOF_TRY(add_into(ctx, sums_dev, (const double *)d_sums, (size_t)S * W));
    timing_end(ctx);
    if (sums) AMOF_TRY(fetch(ctx, sums, d_sums, (size_t)S * W * sizeof(double)));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    return AMOF_OK;
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_vacf_window(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int64_t origin_stride,
                                int32_t velocity_mode, int32_t remove_com, int64_t atom_begin, int64_t atom_end, double *sums)
{
    if (!ctx) return AMOF_EINVAL;
    if (!sums) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return vacf_run(ctx, t, windows, W, origin_stride, velocity_mode, remove_com, atom_begin, atom_end, nullptr, sums, nullptr);
}

extern "C" int amof_vacf_window_dev(amof_ctx *ctx, const amof_traj *t, const int32_t *windows, int32_t W, int64_t origin_stride,
                                    int32_t velocity_mode, int32_t remove_com, int64_t atom_begin, int64_t atom_end,
                                    const double *com_dev, double *sums_dev)
{
    if (!ctx) return AMOF_EINVAL;
    if (!sums_dev) return fail(ctx, AMOF_EINVAL, "NULL argument");
    return vacf_run(ctx, t, windows, W, origin_stride, velocity_mode, remove_com, atom_begin, atom_end, com_dev, nullptr, sums_dev);
}
