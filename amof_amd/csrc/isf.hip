// Intermediate scattering function F(q, t), coherent and self: the time correlation of S(q)'s rho table (gfx950;
// amof_isf_accumulate[_dev]).
//
// Data path, per call:
//   pos --sq_quantize_kernel--> Q[slots][N]: every frame the work range touches, quantised ONCE
//   per chunk of K_c vectors (whole runs of the sorted list; the table [slots][K_c][S][2] f64 stays inside the budget):
//     Q --sq_rho_kernel--> rho[slot][v][s][2]                    (the kernel and atom order of amof_sq_modes: same bits)
//     rho --isf_corr_kernel--> counts[W][nbins], coh[S][S][W][nbins] (int64 fixed point, S(q)'s scales), beyond[W]
//   self part, per batch of (lag, origin) entries:
//     Q --isf_diff_kernel--> D[e][N] = Q[k + m] - Q[k] (u32 wrap-around: the exact phase of the displacement)
//     D --sq_rho_kernel--> rho_d[e][K][S][2];  Re rho_d --isf_self_bin_kernel--> self[S][W][nbins]
// The quantiser and sq_rho_kernel are sq.hip's, launched there (sq_launch_quantize, sq_launch_rho).
//
// isf_corr_kernel: a lane owns a vector of the chunk (consecutive lanes: consecutive 16 S-byte records of one frame's row),
// a workgroup a range of origin indices.  Origins are taken ISF_TILE at a time: their rows rho(k) and their bins are loaded
// into registers once and serve every lag of the pass; per lag the S^2 products of the tile's origins are rounded to int64
// and summed in registers while the bin stays the same (always, for a constant cell), then added with one atomic per
// (lane, lag, pair) and tile -- into per-lag LDS counter tiles ((1 + S^2) nbins u64 each; as many lags per pass as fit
// LAG_LDS_BUDGET, flushed to global memory after each pass) or straight into global memory ("isf_global").  S > ISF_SMAX
// takes a generic form of the same kernel (one atomic per sample, rows re-read through the caches).
//
// The host code is the lag scaffold of sq_call.h (shared with current.hip) around F(q, t)'s own stages: the scales, the
// quantiser, the self part and the quantiser's flag at the end.  Rules: sq_plan.h.
#include <algorithm>
#include <vector>

#include "sq_call.h"

namespace amof {
namespace {

// the bin of amof_sq_accumulate (f64, no fma), -1 = beyond
__device__ __forceinline__ int isf_bin(const double *__restrict__ R, const int32_t *__restrict__ v, double dq, int nbins)
{
    const double h = (double)v[0], k = (double)v[1], l = (double)v[2];
    const double qx = (h * R[0] + k * R[3]) + l * R[6];
    const double qy = (h * R[1] + k * R[4]) + l * R[7];
    const double qz = (h * R[2] + k * R[5]) + l * R[8];
    const double qq = sqrt((qx * qx + qy * qy) + qz * qz) / dq;
    if (!(qq < (double)nbins)) return -1;
    return (int)qq;
}

template <int ST, bool GLOBAL>
__global__ __launch_bounds__(ISF_THREADS) void isf_corr_kernel(LagArgs a)
{
    extern __shared__ __align__(16) unsigned char lds_raw[];
    unsigned long long *lc = reinterpret_cast<unsigned long long *>(lds_raw);
    const int tid = threadIdx.x;
    const int S = ST ? ST : a.S;
    constexpr int SR = ST ? ST : 1;
    const int W = a.W, nbins = a.nbins, Kc = a.Kc;
    const int v = blockIdx.x * ISF_THREADS + tid;
    const bool live = v < Kc;
    const int ob = a.omin + (int)blockIdx.y * a.opw, oe = min(ob + a.opw, a.omax);
    const int tile = (1 + S * S) * nbins;
    const int L = GLOBAL ? W : a.lags_per_pass;
    const size_t row = (size_t)S * 2;
    const int32_t *hv = a.hkl + 3 * (size_t)a.vec[live ? v : 0];

    for (int w0 = 0; w0 < W; w0 += L) {
        const int w1 = min(w0 + L, W);
        if (!GLOBAL) {
            for (int i = tid; i < (w1 - w0) * tile; i += ISF_THREADS) lc[i] = 0ull;
            __syncthreads();
        }
        if (live) {
            for (int os = ob; os < oe; os += ISF_TILE) {
                // the tile's origin rows and bins: loaded once, used by every lag of the pass
                int bins[ISF_TILE];
                const double *orow[ISF_TILE];
                double ore[ISF_TILE][SR], oim[ISF_TILE][SR];
#pragma unroll
                for (int t = 0; t < ISF_TILE; t++) {
                    bins[t] = -1;
                    orow[t] = a.tab;
                    if (os + t < oe) {
                        const int64_t k = 1 + a.stride * (int64_t)(os + t);
                        bins[t] = isf_bin(a.recip + (a.n_cells == 1 ? 0 : (size_t)k * 9), hv, a.dq, nbins);
                        orow[t] = a.tab + ((size_t)a.slot_of[k] * Kc + v) * row;
                        if (ST) {
#pragma unroll
                            for (int s = 0; s < SR; s++) { ore[t][s] = orow[t][2 * s]; oim[t][s] = orow[t][2 * s + 1]; }
                        }
                    }
                }
                for (int w = w0; w < w1; w++) {
                    const int2 iv = a.lagiv[w];
                    const int lo = max(os, iv.x), hi = min(min(os + ISF_TILE, oe), iv.y);
                    if (lo >= hi) continue;
                    const int64_t m = a.windows[w];
                    unsigned long long *cw = GLOBAL ? a.counts + (size_t)w * nbins : lc + (size_t)(w - w0) * tile;
                    // coh of (a, c): cg + (a S + c) cstep
                    unsigned long long *cg = GLOBAL ? a.sum0 + (size_t)w * nbins : cw + nbins;
                    const size_t cstep = GLOBAL ? (size_t)W * nbins : (size_t)nbins;
                    unsigned long long nbey = 0;
                    if (ST) {
                        unsigned long long acc[SR * SR], cnt = 0;
                        int cur = -1;
#pragma unroll
                        for (int i = 0; i < SR * SR; i++) acc[i] = 0ull;
                        auto flush = [&]() {
                            if (!cnt) return;
                            atomicAdd(&cw[cur], cnt);
#pragma unroll
                            for (int i = 0; i < SR * SR; i++) {
                                if (acc[i]) atomicAdd(&cg[(size_t)i * cstep + cur], acc[i]);
                                acc[i] = 0ull;
                            }
                            cnt = 0;
                        };
#pragma unroll
                        for (int t = 0; t < ISF_TILE; t++) {
                            const int o = os + t;
                            if (o < lo || o >= hi) continue;
                            if (bins[t] < 0) { nbey++; continue; }
                            if (bins[t] != cur) { flush(); cur = bins[t]; }
                            const int64_t km = 1 + a.stride * (int64_t)o + m;
                            const double *__restrict__ pr = a.tab + ((size_t)a.slot_of[km] * Kc + v) * row;
                            double pre[SR], pim[SR];
#pragma unroll
                            for (int s = 0; s < SR; s++) { pre[s] = pr[2 * s]; pim[s] = pr[2 * s + 1]; }
                            cnt++;
#pragma unroll
                            for (int x = 0; x < SR; x++)
#pragma unroll
                                for (int c = 0; c < SR; c++) {
                                    const double tt = ore[t][x] * pre[c] + oim[t][x] * pim[c];
                                    acc[x * SR + c] += (unsigned long long)(long long)rint(tt * a.scale2[x * SR + c]);
                                }
                        }
                        flush();
                    } else {
#pragma unroll
                        for (int t = 0; t < ISF_TILE; t++) {
                            const int o = os + t;
                            if (o < lo || o >= hi) continue;
                            const int bin = bins[t];
                            if (bin < 0) { nbey++; continue; }
                            const int64_t km = 1 + a.stride * (int64_t)o + m;
                            const double *__restrict__ po = orow[t];
                            const double *__restrict__ pr = a.tab + ((size_t)a.slot_of[km] * Kc + v) * row;
                            atomicAdd(&cw[bin], 1ull);
                            for (int x = 0; x < S; x++) {
                                const double ra = po[2 * x], ia = po[2 * x + 1];
                                for (int c = 0; c < S; c++) {
                                    const double tt = ra * pr[2 * c] + ia * pr[2 * c + 1];
                                    atomicAdd(&cg[(size_t)(x * S + c) * cstep + bin],
                                              (unsigned long long)(long long)rint(tt * a.scale2[x * S + c]));
                                }
                            }
                        }
                    }
                    if (nbey) atomicAdd(&a.beyond[w], nbey);
                }
            }
        }
        if (!GLOBAL) {
            __syncthreads();
            for (int i = tid; i < (w1 - w0) * tile; i += ISF_THREADS) {
                const unsigned long long val = lc[i];
                if (!val) continue;
                const int w = w0 + i / tile, r = i % tile, j = r / nbins, b = r % nbins;
                atomicAdd(j == 0 ? &a.counts[(size_t)w * nbins + b] : &a.sum0[((size_t)(j - 1) * W + w) * nbins + b], val);
            }
            __syncthreads();
        }
    }
}

// D[e][i] = Q[slot of k + m][i] - Q[slot of k][i], component by component in u32 wrap-around arithmetic
__global__ __launch_bounds__(256) void isf_diff_kernel(const uint4 *__restrict__ Q, int64_t N, const IsfEntry *__restrict__ ent,
                                                       uint4 *__restrict__ D)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const IsfEntry e = ent[blockIdx.y];
    const uint4 q0 = Q[(size_t)e.sk * N + i], q1 = Q[(size_t)e.skm * N + i];
    D[(size_t)blockIdx.y * N + i] = make_uint4(q1.x - q0.x, q1.y - q0.y, q1.z - q0.z, 0u);
}

// self[a][w][bin] += rint(Re rho_d_a 2^s_aa): one (entry, vector) sample per thread, bin from the origin frame
__global__ __launch_bounds__(SQ_THREADS) void isf_self_bin_kernel(const double *__restrict__ rho, int nb, int K, int S, int W,
                                                                  const IsfEntry *__restrict__ ent, const int32_t *__restrict__ hkl,
                                                                  const double *__restrict__ recip, int64_t n_cells, double dq,
                                                                  int nbins, const double *__restrict__ scale2,
                                                                  unsigned long long *__restrict__ selfs)
{
    const int64_t total = (int64_t)nb * K;
    for (int64_t it = (int64_t)blockIdx.x * SQ_THREADS + threadIdx.x; it < total; it += (int64_t)gridDim.x * SQ_THREADS) {
        const int b = (int)(it / K), m = (int)(it % K);
        const IsfEntry e = ent[b];
        const int bin = isf_bin(recip + (n_cells == 1 ? 0 : (size_t)e.k * 9), hkl + 3 * (size_t)m, dq, nbins);
        if (bin < 0) continue;      // (counted in beyond by the coherent part)
        const double *r = rho + (size_t)it * S * 2;
        for (int s = 0; s < S; s++)
            atomicAdd(&selfs[((size_t)s * W + e.w) * nbins + bin],
                      (unsigned long long)(long long)rint(r[2 * s] * scale2[s * S + s]));
    }
}

struct IsfCorr {
    template <int ST, bool GLOBAL> static auto kernel() { return isf_corr_kernel<ST, GLOBAL>; }
};

// --------------------------------------------------------------------------------------------- host code --
// counters: [counts | coh | self | beyond]; spans: rho table (with the quantisation), correlation, self
struct IsfCall : LagCall {
    using LagCall::LagCall;
    bool want_self = false;     // the self part is computed (selfs / self_dev given)
    size_t n_coh = 0, n_self = 0;
    std::vector<IsfEntry> entries;
    int i_scale2 = -1, i_ent = -1;
};

// per batch of (lag, origin) entries: the displacements D, their rho, the bins of the origin frames
int isf_self(IsfCall &c)
{
    amof_ctx *ctx = c.ctx;
    const UploadPack &pk = c.pk;
    const size_t nb_max = isf_self_batch(c.sw.isf_rho_budget, c.N, c.K, c.S, c.entries.size());
    void *d_D = nullptr, *d_rd = nullptr;
    AMOF_TRY(ensure(ctx, SLOT_AUX2, nb_max * (size_t)std::max<int64_t>(c.N, 1) * sizeof(uint4), &d_D));
    AMOF_TRY(ensure(ctx, SLOT_AUX3, nb_max * (size_t)c.K * c.S * 2 * sizeof(double), &d_rd));
    c.spans.begin(2);
    for (size_t e0 = 0; e0 < c.entries.size(); e0 += nb_max) {
        const int nb = (int)std::min<size_t>(nb_max, c.entries.size() - e0);
        const IsfEntry *d_ent = pk.ptr<IsfEntry>(c.i_ent) + e0;
        if (c.N > 0)
            hipLaunchKernelGGL(isf_diff_kernel, dim3((unsigned)((c.N + 255) / 256), (unsigned)nb), dim3(256), 0, ctx->stream,
                               (const uint4 *)c.d_Q, c.N, d_ent, (uint4 *)d_D);
        AMOF_HIP_TRY(ctx, hipGetLastError());
        AMOF_TRY(sq_launch_rho(c, (const uint4 *)d_D, (size_t)nb, 0, (int)c.pl.runs.size(), pk.ptr<int32_t>(c.i_order), c.K, (double *)d_rd));
        hipLaunchKernelGGL(isf_self_bin_kernel, dim3(sq_sample_blocks(nb, c.K)), dim3(SQ_THREADS), 0, ctx->stream, (const double *)d_rd,
                           nb, c.K, c.S, c.W, d_ent, pk.ptr<int32_t>(c.i_hkl), pk.ptr<double>(c.i_recip), c.t->n_cells, c.dq,
                           (int)c.nbins, pk.ptr<double>(c.i_scale2), c.sums + c.n_coh);
        AMOF_HIP_TRY(ctx, hipGetLastError());
    }
    c.spans.end();
    return AMOF_OK;
}

int isf_run(IsfCall &c, int64_t wb, int64_t we, const LagOutputs &out)
{
    amof_ctx *ctx = c.ctx;
    AMOF_TRY(lag_check(c));
    AMOF_TRY(lag_work(c, wb, we));
    c.n_coh = (size_t)c.S * c.S * c.n_cnt;
    c.n_self = c.want_self ? (size_t)c.S * c.n_cnt : 0;
    AMOF_TRY(sq_check_histogram(c, c.n_coh));
    AMOF_TRY(sq_call_scales(c, out.scale_log2));
    sq_expand_pairs(c.S, c.sc, c.scale2, c.sexp2);
    lag_zero_host(c, out);
    if (c.n_entries == 0 || c.K == 0) return AMOF_OK;

    AMOF_TRY(build_geometry(ctx, c.t, c.hg));
    AMOF_TRY(sq_call_plan(c));
    isf_touched_frames(c.lagiv.data(), c.windows, c.W, c.F, c.stride, c.fr);
    isf_cut_chunks(c.pl.runs, c.K, c.fr.fsel.size(), c.S, c.sw.isf_rho_budget, c.ch);
    c.pass = isf_pass_plan(c.S, c.nbins, c.W, c.sw);
    if (c.want_self) isf_self_entries(c.lagiv.data(), c.windows, c.W, c.stride, c.fr, c.entries);
    c.i_scale2 = c.pk.add(c.scale2.data(), c.scale2.size() * sizeof(double));
    c.i_ent = c.pk.add(c.entries.data(), c.entries.size() * sizeof(IsfEntry));
    AMOF_TRY(lag_stage(c, (size_t)c.ch.kc_top * c.ch.vec_bytes, &out));
    // every touched frame is quantised once
    c.spans.begin(0);
    AMOF_TRY(sq_launch_quantize(c, 0, c.fr.fsel.size(), c.d_Q));
    c.spans.end();
    AMOF_TRY(lag_chunk_loop(
        c, lag_kernel_args(c, c.pk.ptr<double>(c.i_scale2), c.sums, nullptr), ISF_TILE, 0, 1,
        [&](const IsfChunk &k, int64_t *launches) {
            return sq_launch_rho(c, c.d_Q, c.fr.fsel.size(), k.r0, k.r1 - k.r0, c.pk.ptr<int32_t>(c.i_olocal), k.nv, c.d_rho, launches);
        },
        [&](const LagArgs &a, dim3 grid) { return lag_launch_corr<IsfCorr>(ctx, a, grid, c.pass); }));
    if (c.want_self) AMOF_TRY(isf_self(c));
    AMOF_TRY(sq_fetch_flag(c, true));
    return lag_finish(c, out);
}

// one of the two forms: host (f64, overwritten) or device (int64 fixed point / u64, added into; scale_log2 given)
int isf_entry(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K, const int32_t *windows,
              int32_t n_windows, int64_t origin_stride, int64_t work_begin, int64_t work_end, double dq, int32_t nbins,
              LagOutputs &out, const LagSums &coh, const LagSums &selfs)
{
    IsfCall c(ctx, t, recip, hkl, K, dq, nbins);
    c.windows = windows;
    c.W = n_windows;
    c.stride = origin_stride;
    c.want_self = selfs.out_host || selfs.out_dev;
    out.blocks.push_back(coh);
    if (c.want_self) out.blocks.push_back(selfs);
    return isf_run(c, work_begin, work_end, out);
}

}  // namespace
}  // namespace amof

using namespace amof;

extern "C" int amof_isf_accumulate(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                   const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                                   int64_t work_end, double dq, int32_t nbins, uint64_t *counts, double *coh, double *self_sums,
                                   uint64_t *beyond)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts || !coh || !beyond) return fail(ctx, AMOF_EINVAL, "NULL argument");
    LagOutputs out;
    out.counts = counts;
    out.beyond = beyond;
    return isf_entry(ctx, t, recip, hkl, K, windows, n_windows, origin_stride, work_begin, work_end, dq, nbins, out,
                     LagSums{nullptr, coh, false}, LagSums{nullptr, self_sums, true});
}

extern "C" int amof_isf_accumulate_dev(amof_ctx *ctx, const amof_traj *t, const double *recip, const int32_t *hkl, int32_t K,
                                       const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                                       int64_t work_end, double dq, int32_t nbins, uint64_t *counts_dev, int64_t *coh_dev,
                                       int64_t *self_dev, uint64_t *beyond_dev, int32_t *scale_log2)
{
    if (!ctx) return AMOF_EINVAL;
    if (!counts_dev || !coh_dev || !beyond_dev || !scale_log2) return fail(ctx, AMOF_EINVAL, "NULL argument");
    LagOutputs out;
    out.counts_dev = counts_dev;
    out.beyond_dev = beyond_dev;
    out.scale_log2 = scale_log2;
    return isf_entry(ctx, t, recip, hkl, K, windows, n_windows, origin_stride, work_begin, work_end, dq, nbins, out,
                     LagSums{coh_dev, nullptr, false}, LagSums{self_dev, nullptr, true});
}
