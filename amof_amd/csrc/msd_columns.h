// The MSD's atom-major data path, shared by the window MSD (msd.hip) and the self Van Hove function (vanhove.hip):
// wrap of the frame-to-frame steps (ase wrap_positions), centre of mass, transposition to atom-major columns
// D_T[3N][Fp] and their prefix sums (the running positions u of amof_msd_window), with and without unwrap -- the kernels
// and, behind them, the one host function that launches them for a call (build_step_columns).
// Everything here has internal linkage: each translation unit that includes it gets its own copy of the kernels.
#pragma once

#include <math.h>

#include <vector>

#include "amof_internal.h"

namespace amof {
namespace {

constexpr int MSD_THREADS = 256;
constexpr int MSD_GEOM = 24;  // cell[9], full inverse[9], pbc[3], pad

// ase.geometry.wrap_positions(d, cell, center=(0,0,0), eps=1e-7) ([3P-memory],
// call site amof/trajectory.py:302): fractional = d.cell^-1 - shift with
// shift = -0.5 - eps; periodic axes: fractional %= 1; fractional += shift;
// result = fractional . cell
__device__ __forceinline__ void wrap_delta(const double *__restrict__ g, double dx, double dy, double dz,
                                           double &ox, double &oy, double &oz)
{
    const double shift = 0.0 - 0.5 - 1e-7;
    double fr[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        double s = dx * g[9 + k] + dy * g[12 + k] + dz * g[15 + k];
        if (g[18 + k] != 0.0) {
            double t = s - shift;
            t = t - floor(t);
            s = t + shift;
        }
        fr[k] = s;
    }
    ox = fr[0] * g[0] + fr[1] * g[3] + fr[2] * g[6];
    oy = fr[0] * g[1] + fr[1] * g[4] + fr[2] * g[7];
    oz = fr[0] * g[2] + fr[1] * g[5] + fr[2] * g[8];
}

__device__ __forceinline__ double block_sum(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double s = 0.0;
    for (int k = 0; k < MSD_THREADS / 64; k++) s += red[k];
    return s;  // every thread holds the total
}

// mass-weighted centre of mass of every frame (ase get_center_of_mass:
// masses @ positions / masses.sum(); amof/msd.py:236)
__global__ __launch_bounds__(MSD_THREADS) void com_kernel(const double *__restrict__ pos,
                                                          const double *__restrict__ masses, int64_t N,
                                                          double total_mass, double *__restrict__ com)
{
    __shared__ double red[2 * (MSD_THREADS / 64)];     // (wave totals | event flags of the scan)
    const int f = blockIdx.x;
    const double *__restrict__ p = pos + (size_t)f * (size_t)N * 3;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t i = threadIdx.x; i < N; i += MSD_THREADS) {
        double m = masses[i];
        sx += m * p[3 * i];
        sy += m * p[3 * i + 1];
        sz += m * p[3 * i + 2];
    }
    sx = block_sum(sx, red);
    sy = block_sum(sy, red);
    sz = block_sum(sz, red);
    if (threadIdx.x == 0) {
        com[3 * f] = sx / total_mass;
        com[3 * f + 1] = sy / total_mass;
        com[3 * f + 2] = sz / total_mass;
    }
}

// D_T[3a+c][k] = wrap((pos[k][a]-com[k]) - (pos[k-1][a]-com[k-1]); cell[k-1]),  D_T[.][0] = 0
// for the atoms a in [a_begin, a_end) only (atom-sharded calls transpose just their share).
// Tile = TF frames x TA atoms.  A thread owns one atom and FPT = TF TA / THREADS CONSECUTIVE frames: it loads
// the FPT + 1 rows it needs once (every load in flight before the first use), removes the centre of mass once per
// row, wraps the FPT differences and parks them in the LDS tile; the tile leaves transposed, two frames (16 B) per
// lane, TF frames of a column as one contiguous run.  ORTHO: every cell is diagonal -- the zero terms of the
// general formula are dropped, which leaves the bits unchanged (x + (+-0) = x).
template <bool ORTHO>
__device__ __forceinline__ void wrap_delta_t(const double *__restrict__ g, double dx, double dy, double dz,
                                             double &ox, double &oy, double &oz)
{
    if (!ORTHO) {
        wrap_delta(g, dx, dy, dz, ox, oy, oz);
        return;
    }
    const double shift = 0.0 - 0.5 - 1e-7;
    double fr[3] = {dx * g[9], dy * g[13], dz * g[17]};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (g[18 + k] != 0.0) {
            double t = fr[k] - shift;
            t = t - floor(t);
            fr[k] = t + shift;
        }
    }
    ox = fr[0] * g[0];
    oy = fr[1] * g[4];
    oz = fr[2] * g[8];
}

// Sum of a double over the 64 lanes of a wave, valid in lane 63; fixed order.  Rows of 16 lanes by DPP moves (row_shr
// 1, 2, 4, 8 with zero fill: vector-ALU instructions -- __shfl_down goes through the LDS crossbar twice per double and
// cost the transposition 0.12 ms), the four row totals by readlane.
__device__ __forceinline__ double wave_sum_dpp(double x)
{
#define AMOF_DPP_STEP(CTRL)                                                                                     \
    {                                                                                                           \
        const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xf, 0xf, true);                  \
        const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xf, 0xf, true);                  \
        x += __hiloint2double(hi, lo);                                                                           \
    }
    AMOF_DPP_STEP(0x111)    // row_shr:1
    AMOF_DPP_STEP(0x112)    // row_shr:2
    AMOF_DPP_STEP(0x114)    // row_shr:4
    AMOF_DPP_STEP(0x118)    // row_shr:8
#undef AMOF_DPP_STEP
    auto lane = [&](int l) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
    };
    return ((lane(15) + lane(31)) + lane(47)) + x;      // (lane 63 holds the last row's total)
}

template <int TF, int TA, int THREADS, bool ORTHO>
__global__ __launch_bounds__(THREADS) void delta_transpose_kernel(const double *__restrict__ pos,
                                                                  const double *__restrict__ com,
                                                                  const double *__restrict__ geom,
                                                                  int n_cells, int64_t N, int F, int64_t Fp,
                                                                  int64_t a_begin, int64_t a_end,
                                                                  double *__restrict__ DT,
                                                                  const double *__restrict__ masses, double *__restrict__ cpart)
{
    constexpr int KG = THREADS / TA;      // frame groups of the workgroup
    constexpr int FPT = TF / KG;          // consecutive frames per thread
    static_assert(THREADS % TA == 0 && TF % KG == 0 && TF % 2 == 0, "tile shape");
    extern __shared__ __align__(16) unsigned char lds_raw[];
    double (*tile)[3 * TA + 1] = reinterpret_cast<double (*)[3 * TA + 1]>(lds_raw);   // [TF][3 TA + 1]
    const int k0 = blockIdx.y * TF;
    const int64_t a0 = a_begin + (int64_t)blockIdx.x * TA;
    const int al = threadIdx.x % TA, kg = threadIdx.x / TA;
    const int64_t a = a0 + al;
    const int kb = k0 + kg * FPT;         // this thread's frames: kb .. kb + FPT - 1 (row kb - 1 is needed too)
    const bool atom_ok = a < a_end;
    double px[FPT + 1], py[FPT + 1], pz[FPT + 1];
#pragma unroll
    for (int j = 0; j <= FPT; j++) {
        const int k = kb - 1 + j;
        px[j] = py[j] = pz[j] = 0.0;
        if (atom_ok && k >= 0 && k < F) {
            const double *p = pos + ((size_t)k * N + a) * 3;
            px[j] = p[0]; py[j] = p[1]; pz[j] = p[2];
        }
    }
    if (com) {
#pragma unroll
        for (int j = 0; j <= FPT; j++) {
            const int k = kb - 1 + j;
            if (k >= 0 && k < F) {
                px[j] -= com[3 * k]; py[j] -= com[3 * k + 1]; pz[j] -= com[3 * k + 2];
            }
        }
    }
    if (cpart) {
        // 2-pass form: the tile's share of sum_a m_a p_a for this thread's own frames (a wave = the TA = 64 atoms of one
        // frame group): lanes by shuffles in fixed order, one row of cpart[tile][F][3] per frame
        static_assert(TA == 64, "one wave per frame group");
        const double m = atom_ok ? masses[a] : 0.0;
#pragma unroll
        for (int j = 1; j <= FPT; j++) {
            const int k = kb - 1 + j;
            const double sx = wave_sum_dpp(m * px[j]), sy = wave_sum_dpp(m * py[j]), sz = wave_sum_dpp(m * pz[j]);
            if (al == 63 && k < F) {
                double *o = cpart + ((size_t)blockIdx.x * (size_t)F + (size_t)k) * 3;
                o[0] = sx; o[1] = sy; o[2] = sz;
            }
        }
    }
#pragma unroll
    for (int j = 1; j <= FPT; j++) {
        const int k = kb - 1 + j;
        double dx = 0.0, dy = 0.0, dz = 0.0;
        if (atom_ok && k >= 1 && k < F) {
            const double *g = geom + (size_t)(n_cells == 1 ? 0 : k - 1) * MSD_GEOM;
            wrap_delta_t<ORTHO>(g, px[j] - px[j - 1], py[j] - py[j - 1], pz[j] - pz[j - 1], dx, dy, dz);
        }
        const int kl = kg * FPT + j - 1;
        tile[kl][3 * al] = dx;
        tile[kl][3 * al + 1] = dy;
        tile[kl][3 * al + 2] = dz;
    }
    __syncthreads();
#pragma unroll 3
    for (int idx = threadIdx.x; idx < (TF / 2) * 3 * TA; idx += THREADS) {
        const int cl = idx / (TF / 2), kl = 2 * (idx % (TF / 2));
        const int64_t col = 3 * a0 + cl;
        // (k0 + kl is even and Fp a multiple of 32: the pair is inside the column or wholly outside)
        if (col < 3 * a_end && k0 + kl < Fp)
            *reinterpret_cast<double2 *>(DT + (size_t)col * Fp + k0 + kl) = make_double2(tile[kl][cl], tile[kl + 1][cl]);
    }
}

// in-place inclusive prefix sum of u[0..F) held in LDS by the whole workgroup: every thread
// owns one contiguous chunk (serial sum, then serial rewrite), the 256 chunk totals are scanned
// with wave shuffles -- two barriers per column instead of two per 256 elements.
// thr / evt (2-pass form): evt is set for the whole workgroup when some entry of the column exceeds thr in magnitude
__device__ __forceinline__ void lds_scan(double *u, int F, double *wtot, double carry_init, double thr = __builtin_inf(),
                                         bool *evt = nullptr)
{
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    // odd chunk length: lanes then start an odd number of doubles apart, so the strided LDS accesses of a
    // wave spread over all banks (an even stride such as 20 doubles is an 8-way conflict)
    const int chunk = ((F + MSD_THREADS - 1) / MSD_THREADS) | 1;
    const int k0 = min(tid * chunk, F), k1 = min(k0 + chunk, F);
    double s = 0.0;
    bool big = false;
    for (int k = k0; k < k1; k++) {
        const double x = u[k];
        big |= fabs(x) > thr;
        s += x;
    }
    const bool wbig = evt ? __any(big) != 0 : false;
    double v = s;                                   // inclusive scan of the chunk totals
    for (int off = 1; off < 64; off <<= 1) {
        double n = __shfl_up(v, off, 64);
        if (lane >= off) v += n;
    }
    __syncthreads();
    if (lane == 63) {
        wtot[wv] = v;
        if (evt) wtot[MSD_THREADS / 64 + wv] = wbig ? 1.0 : 0.0;       // (the flags ride behind the totals: no barrier of their own)
    }
    __syncthreads();
    if (evt) {
        double any = 0.0;
        for (int q = 0; q < MSD_THREADS / 64; q++) any += wtot[MSD_THREADS / 64 + q];
        *evt = any > 0.0;
    }
    double run = carry_init + (v - s);              // exclusive prefix of this thread's chunk
    for (int q = 0; q < wv; q++) run += wtot[q];
    for (int k = k0; k < k1; k++) {
        run += u[k];
        u[k] = run;
    }
    __syncthreads();
}

// ---- unwrap path (amof/msd.py:222-230) in atom-major layout ----
// OUT[col][k] = x0[col] + sum_{j<=k} IN[col][j]   (x0 == nullptr: plain prefix sum; IN may alias OUT).
// Any F: the column is scanned in LDS segments with a running carry.
constexpr int SCAN_SEG = 8192;
__global__ __launch_bounds__(MSD_THREADS) void scan_column_kernel(const double *IN, const double *__restrict__ x0,
                                                                  int64_t Fp, int F, double *OUT)
{
    __shared__ double u[SCAN_SEG];
    __shared__ double red[2 * (MSD_THREADS / 64)];     // (wave totals | event flags of the scan)
    __shared__ double carry_s;
    const size_t col = blockIdx.x;
    double carry = x0 ? x0[col] : 0.0;
    for (int base = 0; base < F; base += SCAN_SEG) {
        const int n = min(SCAN_SEG, F - base);
        __syncthreads();
        for (int k = threadIdx.x; k < n; k += MSD_THREADS) u[k] = IN[col * Fp + base + k];
        __syncthreads();
        lds_scan(u, n, red, carry);
        for (int k = threadIdx.x; k < n; k += MSD_THREADS) OUT[col * Fp + base + k] = u[k];
        if (threadIdx.x == 0) carry_s = u[n - 1];
        __syncthreads();
        carry = carry_s;
    }
}

// centre of mass from the atom-major layout, in two deterministic stages: partial sums over
// blocks of COMT_BLK atoms (thread = frame k, coalesced along k), then the blocks in order
constexpr int COMT_BLK = 128;
__global__ __launch_bounds__(MSD_THREADS) void com_T_partial_kernel(const double *__restrict__ UT,
                                                                    const double *__restrict__ masses, int64_t N,
                                                                    int64_t Fp, int F, double *__restrict__ part)
{
    const int k = blockIdx.x * MSD_THREADS + threadIdx.x;
    const int c = blockIdx.y;
    const int64_t i0 = (int64_t)blockIdx.z * COMT_BLK, i1 = min(i0 + COMT_BLK, N);
    if (k >= F) return;
    double s = 0.0;
    for (int64_t i = i0; i < i1; i++) s += masses[i] * UT[(size_t)(3 * i + c) * Fp + k];
    part[((size_t)blockIdx.z * 3 + c) * Fp + k] = s;
}

__global__ __launch_bounds__(MSD_THREADS) void com_T_final_kernel(const double *__restrict__ part, int nblk,
                                                                  int64_t Fp, int F, double total_mass,
                                                                  double *__restrict__ com)
{
    const int k = blockIdx.x * MSD_THREADS + threadIdx.x;
    const int c = blockIdx.y;
    if (k >= F) return;
    double s = 0.0;
    for (int b = 0; b < nblk; b++) s += part[((size_t)b * 3 + c) * Fp + k];
    com[3 * k + c] = s / total_mass;
}

__global__ __launch_bounds__(MSD_THREADS) void delta_T_kernel(const double *__restrict__ UT,
                                                              const double *__restrict__ com,
                                                              const double *__restrict__ geom, int n_cells,
                                                              int64_t N, int64_t Fp, int F, int64_t a_begin,
                                                              double *__restrict__ DT)
{
    const int k = blockIdx.y * MSD_THREADS + threadIdx.x;
    const size_t a = (size_t)a_begin + blockIdx.x;
    if (k >= F) return;
    double dx = 0.0, dy = 0.0, dz = 0.0;
    if (k >= 1) {
        double x1 = UT[(3 * a) * Fp + k], y1 = UT[(3 * a + 1) * Fp + k], z1 = UT[(3 * a + 2) * Fp + k];
        double x0 = UT[(3 * a) * Fp + k - 1], y0 = UT[(3 * a + 1) * Fp + k - 1], z0 = UT[(3 * a + 2) * Fp + k - 1];
        if (com) {
            x1 -= com[3 * k]; y1 -= com[3 * k + 1]; z1 -= com[3 * k + 2];
            x0 -= com[3 * (k - 1)]; y0 -= com[3 * (k - 1) + 1]; z0 -= com[3 * (k - 1) + 2];
        }
        const double *g = geom + (size_t)(n_cells == 1 ? 0 : k - 1) * MSD_GEOM;
        wrap_delta(g, x1 - x0, y1 - y0, z1 - z0, dx, dy, dz);
    }
    DT[(3 * a) * Fp + k] = dx;
    DT[(3 * a + 1) * Fp + k] = dy;
    DT[(3 * a + 2) * Fp + k] = dz;
}

// geometry records of the wrap kernels: cell rows, FULL inverse (wrap_positions semantics), periodic flags
inline void msd_geom_records(const amof_traj *t, const HostGeom &hg, std::vector<double> &grec)
{
    grec.assign((size_t)t->n_cells * MSD_GEOM, 0.0);
    for (int64_t k = 0; k < t->n_cells; k++) {
        for (int q = 0; q < 9; q++) grec[(size_t)k * MSD_GEOM + q] = t->cell[9 * k + q];
        for (int q = 0; q < 9; q++) grec[(size_t)k * MSD_GEOM + 9 + q] = hg.invfull[(size_t)k * 9 + q];
        for (int q = 0; q < 3; q++) grec[(size_t)k * MSD_GEOM + 18 + q] = t->pbc[q] ? 1.0 : 0.0;
    }
}

// ---- the wrapped step columns of a call, as amof_msd_window forms them ----
// Transposition tile: 32 frames x 64 atoms, 1024 threads (two consecutive frames per thread).  Measured on the MI355X for
// the headline shape (profiles/r02/msd_transpose_shapes.txt): 0.52 ms = 4.5 TB/s of read + write; a flat copy of the same
// bytes (torch) takes 0.46 ms.  Four or eight frames per thread: 0.57 / 1.18 ms.
constexpr int TR_TF = 32, TR_TA = 64, TR_TH = 1024;

struct ColumnsIn {
    const double *pos_dev;      // [F][N][3]
    const double *d_geom;       // msd_geom_records on the device
    bool all_ortho;
    const double *d_mass;       // [N] (remove_com)
    double total_mass;
    bool unwrap, remove_com;
    const double *com_ext;      // optional precomputed centre of mass, device [F][3] (not with unwrap)
};

// Leaves D_T[3a + c][Fp], the wrapped steps of the atoms [a0, a1), in SLOT_AUX3 (*d_DT_out: the slot, columns indexed by
// the atom's own number).  Slots: AUX2 centre of mass, AUX4 the unwrapped columns U_T, AUX6 its partial sums.
// cpart (2-pass fold): RAW wrapped steps -- no centre of mass is removed -- and the mass-weighted coordinate sums of every
// tile of TR_TA atoms and frame go to cpart[tile][F][3].
int build_step_columns(amof_ctx *ctx, const amof_traj *t, const ColumnsIn &in, int64_t a0, int64_t a1, double **d_DT_out,
                       double *cpart = nullptr)
{
    const int64_t N = t->n_atoms, F = t->n_frames, Fp = (F + 31) / 32 * 32;
    const size_t dt_bytes = (size_t)3 * N * Fp * sizeof(double);
    const dim3 frames((unsigned)((F + MSD_THREADS - 1) / MSD_THREADS));
    void *d_DT, *d_com = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX3, dt_bytes, &d_DT));
    if (in.remove_com && !cpart) AMOF_TRY(ensure(ctx, SLOT_AUX2, (size_t)F * 3 * sizeof(double), &d_com));
    // only the atoms [b0, b1) are transposed (atom-sharded ranks each do their share)
    auto transpose = [&](const double *com_dev, int64_t b0, int64_t b1) -> hipError_t {
        const dim3 grid((unsigned)((b1 - b0 + TR_TA - 1) / TR_TA), (unsigned)((F + TR_TF - 1) / TR_TF));
        return with_flag(in.all_ortho, [&](auto O) {
            return launch_lds(delta_transpose_kernel<TR_TF, TR_TA, TR_TH, O()>, grid, dim3(TR_TH),
                              (size_t)TR_TF * (3 * TR_TA + 1) * sizeof(double), ctx->stream, in.pos_dev, com_dev, in.d_geom,
                              (int)t->n_cells, N, (int)F, Fp, b0, b1, (double *)d_DT, in.d_mass, cpart);
        });
    };
    if (cpart) {
        AMOF_HIP_TRY(ctx, transpose(nullptr, a0, a1));
    } else if (!in.unwrap) {
        if (in.remove_com && !in.com_ext)
            hipLaunchKernelGGL(com_kernel, dim3((unsigned)F), dim3(MSD_THREADS), 0, ctx->stream, in.pos_dev, in.d_mass, N,
                               in.total_mass, (double *)d_com);
        AMOF_HIP_TRY(ctx, transpose(in.remove_com ? (in.com_ext ? in.com_ext : (const double *)d_com) : nullptr, a0, a1));
    } else {
        // the unwrapped centre of mass needs every atom: all columns are transposed and scanned from frame 0's positions
        void *d_UT;
        AMOF_TRY(ensure(ctx, SLOT_AUX4, dt_bytes, &d_UT));
        AMOF_HIP_TRY(ctx, transpose(nullptr, 0, N));
        hipLaunchKernelGGL(scan_column_kernel, dim3((unsigned)(3 * N)), dim3(MSD_THREADS), 0, ctx->stream, (const double *)d_DT,
                           in.pos_dev, Fp, (int)F, (double *)d_UT);
        if (in.remove_com) {
            const int nblk = (int)((N + COMT_BLK - 1) / COMT_BLK);
            void *d_part;
            AMOF_TRY(ensure(ctx, SLOT_AUX6, (size_t)nblk * 3 * Fp * sizeof(double), &d_part));
            hipLaunchKernelGGL(com_T_partial_kernel, dim3(frames.x, 3, (unsigned)nblk), dim3(MSD_THREADS), 0, ctx->stream,
                               (const double *)d_UT, in.d_mass, N, Fp, (int)F, (double *)d_part);
            hipLaunchKernelGGL(com_T_final_kernel, dim3(frames.x, 3), dim3(MSD_THREADS), 0, ctx->stream, (const double *)d_part,
                               nblk, Fp, (int)F, in.total_mass, (double *)d_com);
        }
        hipLaunchKernelGGL(delta_T_kernel, dim3((unsigned)(a1 - a0), frames.x), dim3(MSD_THREADS), 0, ctx->stream,
                           (const double *)d_UT, (const double *)d_com, in.d_geom, (int)t->n_cells, N, Fp, (int)F, a0, (double *)d_DT);
    }
    AMOF_HIP_TRY(ctx, hipGetLastError());
    *d_DT_out = (double *)d_DT;
    return AMOF_OK;
}

}  // namespace
}  // namespace amof
