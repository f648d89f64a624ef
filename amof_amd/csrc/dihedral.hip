// Dihedral (torsion) angle distributions of bonded chains (gfx950): amof_dihedral_hist and amof_dihedral_hist_dev.  The
// "dihedral_frame" tier reads the neighbour rows of nbr.hip's list stage (frame_lists_tier, nbr_rows.h).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "amof_internal.h"
#include "angle_math.h"
#include "dihedral_math.h"
#include "nbr_rows.h"
#include "ring_search.h"

namespace amof {

// ------------------------------------------------------------------ dihedral ----
// Torsion angle of every chain a-b-c-d of bonded atoms (include/amof_hip.h, amof_dihedral_hist; dihedral_math.h states the
// arithmetic and the pattern match once, for both kernels and the CPU driver).  A lane owns a (frame, atom b), walks the
// central bonds to partners c > b and forms every (a, d); which patterns count a species 4-tuple comes from a host-built table
// of masks (S^4 <= DIHEDRAL_TABLE_MAX words) or from the loop over the patterns.  Every output is an integer.
//   dihedral_rows_kernel   "dihedral_frame": the unit vectors and partner indices from the neighbour rows of the list stage
//                          (lists_frame_kernel<.., IDS = true>); c's rows through region_of and inv_rank
//   dihedral_exact_kernel  "dihedral_exact": index rows from launch_bond_rows, the unit vectors recomputed from the positions
//                          (pair_base<ORTHO>, unit_vec: the bits the rows hold)
// Histogram: one per workgroup in LDS ([T][nb] u32; global u64 atomics when it does not fit).  Frame sums: the lanes of a wave
// whose frame is the wave's first lane's add into the wave's own 3 T LDS words, which the wave then sends with one global
// atomic per nonzero word (a tile of 256 (frame, atom) pairs spans two frames at most unless N < 256); a lane of another
// frame adds to global memory itself.
static_assert(NBRL_CAP == RING_MAX_DEGREE, "both paths refuse the same atoms");
constexpr int DIH_WAVES = NBRF_TILE / 64;

struct DihedralArgs {
    const int32_t *chains;          // [T][4] species indices, -1: any
    const uint32_t *table;          // [S^4] pattern masks of the species 4-tuples, or null (chain_mask per chain)
    const int32_t *species;         // [N]
    const double *edges;            // [nb + 1]
    double edge_step;               // as NbrArgs::edge_step
    int32_t T, nb, global_hist;
    unsigned long long *hist;       // [T][nb]
    unsigned long long *frame_sums; // [F][T][3] (int64, two's complement): defined, undefined, sum of llrint(c 2^40)
    const int32_t *adj, *deg;       // exact kernel: the batch's index rows [nf][N][16], [nf][N]
};

struct DihedralLane {
    unsigned *lh;                   // the workgroup's histogram, or null
    unsigned long long *ws;         // the wave's frame sums [T][3]
    double e0, en, inv_w;
    int f;
    bool in_wave;                   // the lane's frame is the wave's: sums into ws
};

__device__ __forceinline__ uint32_t dihedral_mask(const DihedralArgs &d, int S, int sa, int sb, int sc, int sd)
{
    return d.table ? d.table[((sa * S + sb) * S + sc) * S + sd] : dihedral::chain_mask(d.chains, d.T, sa, sb, sc, sd);
}

// one chain for the patterns of `mask` (not 0)
__device__ __forceinline__ void dihedral_count(const DihedralArgs &d, const DihedralLane &ln, uint32_t mask, double u1x, double u1y,
                                               double u1z, double u2x, double u2y, double u2z, double u3x, double u3y, double u3z)
{
    double c;
    const bool defined = dihedral::chain_cos(u1x, u1y, u1z, u2x, u2y, u2z, u3x, u3y, u3z, c);
    int k = -1;
    long long term = 0;
    if (defined) {
        k = hist_bin(d.edges, d.nb, dihedral::angle_deg(c), ln.e0, ln.en, ln.inv_w, d.edge_step);
        term = dihedral::cos_term(c);
    }
    while (mask) {
        const int t = __ffs((int)mask) - 1;
        mask &= mask - 1u;
        if (k >= 0) {
            if (ln.lh) atomicAdd(&ln.lh[t * d.nb + k], 1u);
            else atomicAdd(&d.hist[(size_t)t * d.nb + k], 1ull);
        }
        if (ln.in_wave) {
            atomicAdd(&ln.ws[3 * t + (defined ? 0 : 1)], 1ull);
            if (term) atomicAdd(&ln.ws[3 * t + 2], (unsigned long long)term);
        } else {
            unsigned long long *fs = d.frame_sums + ((size_t)ln.f * d.T + t) * 3;
            atomicAdd(&fs[defined ? 0 : 1], 1ull);
            if (term) atomicAdd(&fs[2], (unsigned long long)term);
        }
    }
}

// the wave's LDS sums into frame f0's row (called by all 64 lanes after their chains; f0 < 0: the wave had no atom)
__device__ __forceinline__ void dihedral_wave_flush(const DihedralArgs &d, unsigned long long *ws, int f0)
{
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");      // (a wave's LDS operations execute in order: its sums are in place)
    if (f0 < 0) return;
    for (int e = (int)(threadIdx.x & 63); e < 3 * d.T; e += 64) {
        const unsigned long long v = ws[e];
        if (!v) continue;
        atomicAdd(&d.frame_sums[(size_t)f0 * d.T * 3 + e], v);
        ws[e] = 0ull;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// LDS of both kernels: [DIH_WAVES][T][3] u64, then the histogram; the lane's record
__device__ __forceinline__ DihedralLane dihedral_begin(const DihedralArgs &d, unsigned long long *lds)
{
    const int tid = threadIdx.x;
    DihedralLane ln;
    ln.ws = lds + (tid >> 6) * 3 * d.T;
    ln.lh = d.global_hist ? nullptr : reinterpret_cast<unsigned *>(lds + DIH_WAVES * 3 * d.T);
    for (int k = tid; k < DIH_WAVES * 3 * d.T; k += NBRF_TILE) lds[k] = 0ull;
    if (ln.lh)
        for (int k = tid; k < d.T * d.nb; k += NBRF_TILE) ln.lh[k] = 0u;
    ln.e0 = d.edges[0];
    ln.en = d.edges[d.nb];
    ln.inv_w = (double)d.nb / (ln.en - ln.e0);
    ln.f = -1;
    ln.in_wave = false;
    __syncthreads();
    return ln;
}

__device__ __forceinline__ void dihedral_end(const DihedralArgs &d, const DihedralLane &ln)
{
    __syncthreads();
    if (!ln.lh) return;
    for (int k = threadIdx.x; k < d.T * d.nb; k += NBRF_TILE) {
        const unsigned v = ln.lh[k];
        if (v) atomicAdd(&d.hist[k], (unsigned long long)v);
    }
}

// blockIdx.x strides over the tiles of 256 (frame, atom) pairs of the batch, the atoms in species order (perm): the lanes of
// a wave mostly share a species, and with it their rows' regions and their trip counts
__global__ __launch_bounds__(NBRF_TILE) void dihedral_rows_kernel(NbrArgs a, NbrListArgs la, DihedralArgs d, const int64_t *__restrict__ sp_first,
                                                                  int f_base, int nf)
{
    extern __shared__ unsigned long long dihedral_lds[];
    DihedralLane ln = dihedral_begin(d, dihedral_lds);
    const int S = a.S;
    const uint32_t N = (uint32_t)a.N;
    const uint32_t total = (uint32_t)nf * N;                              // (< 2^31: the host sizes the frame batch)
    const uint32_t tiles = (total + NBRF_TILE - 1) / NBRF_TILE;
    // slot k of row r of the batch's frame fl: (ux, uy, uz, partner); a row's count (the list stage's global counters of
    // shared partners run past the capacity: flags[1] is set then)
    auto entry = [&](size_t row, int k) { return reinterpret_cast<const double2 *>(la.rows + ((size_t)k * la.plane + row) * NBRL_EW); };
    auto count = [&](size_t row) { return (int)min(la.count[row], (uint32_t)NBRL_CAP); };
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t flat = tile * (uint32_t)NBRF_TILE + threadIdx.x;
        const bool has = flat < total;
        const uint32_t fl = has ? flat / N : 0u, x = has ? flat - fl * N : 0u;
        ln.f = has ? f_base + (int)fl : -1;
        const int f0 = __shfl(ln.f, 0, 64);
        ln.in_wave = ln.f == f0;
        if (has) {
            const int b = a.perm[x], sb = d.species[b];
            const size_t fbase = (size_t)fl * la.R;
            const size_t brow = fbase + (size_t)(x - (uint32_t)sp_first[sb]);       // + region: b's row for a partner species
            int degree = 0;
            for (int s = 0; s < S; s++) {
                const int reg = la.region_of[sb * S + s];
                if (reg >= 0) degree += count(brow + reg);
            }
            if (degree > NBRL_CAP) a.flags[1] = 1;          // (the exact tier names the frame)
            for (int sc = 0; sc < S && degree >= 2 && degree <= NBRL_CAP; sc++) {
                const int reg_bc = la.region_of[sb * S + sc];
                if (reg_bc < 0) continue;
                const int n_bc = count(brow + reg_bc);
                for (int kc = 0; kc < n_bc; kc++) {
                    const double2 *ec = entry(brow + reg_bc, kc);
                    const double2 c01 = ec[0], c23 = ec[1];
                    const int c = (int)__double_as_longlong(c23.y);
                    if (c <= b) continue;                   // (the chain is visited from its other end)
                    const size_t crow = fbase + (size_t)la.inv_rank[c];
                    for (int sa = 0; sa < S; sa++) {
                        const int reg_ba = la.region_of[sb * S + sa];
                        if (reg_ba < 0) continue;
                        const int n_ba = count(brow + reg_ba);
                        for (int sd = 0; sd < S && n_ba > 0; sd++) {
                            const int reg_cd = la.region_of[sc * S + sd];
                            if (reg_cd < 0) continue;
                            const uint32_t mask = dihedral_mask(d, S, sa, sb, sc, sd);
                            if (!mask) continue;
                            const int n_cd = count(crow + reg_cd);
                            for (int ka = 0; ka < n_ba; ka++) {
                                const double2 *ea = entry(brow + reg_ba, ka);
                                const double2 a01 = ea[0], a23 = ea[1];
                                const int at = (int)__double_as_longlong(a23.y);
                                if (at == c) continue;
                                for (int kd = 0; kd < n_cd; kd++) {
                                    const double2 *ed = entry(crow + reg_cd, kd);
                                    const double2 d01 = ed[0], d23 = ed[1];
                                    const int dt = (int)__double_as_longlong(d23.y);
                                    if (dt == b || dt == at) continue;
                                    dihedral_count(d, ln, mask, a01.x, a01.y, a23.x, c01.x, c01.y, c23.x, d01.x, d01.y, d23.x);
                                }
                            }
                        }
                    }
                }
            }
        }
        dihedral_wave_flush(d, ln.ws, f0);
    }
    dihedral_end(d, ln);
}

// the same chains from the index rows of launch_bond_rows (ascending, any cell); a lane owns (frame, atom b), b in atom order
template <bool ORTHO>
__global__ __launch_bounds__(NBRF_TILE) void dihedral_exact_kernel(NbrArgs a, DihedralArgs d, int f_base, int nf)
{
    extern __shared__ unsigned long long dihedral_lds[];
    DihedralLane ln = dihedral_begin(d, dihedral_lds);
    const int S = a.S;
    const uint32_t N = (uint32_t)a.N;
    const uint32_t total = (uint32_t)nf * N;                              // (< 2^31: the host sizes the frame batch)
    const uint32_t tiles = (total + NBRF_TILE - 1) / NBRF_TILE;
    for (uint32_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const uint32_t flat = tile * (uint32_t)NBRF_TILE + threadIdx.x;
        const bool has = flat < total;
        const uint32_t fl = has ? flat / N : 0u;
        const int b = has ? (int)(flat - fl * N) : 0;
        ln.f = has ? f_base + (int)fl : -1;
        const int f0 = __shfl(ln.f, 0, 64);
        ln.in_wave = ln.f == f0;
        if (has) {
            const double *__restrict__ p = a.pos + (size_t)ln.f * (size_t)a.N * 3;
            const double *__restrict__ g = a.geom + (size_t)(a.n_cells == 1 ? 0 : ln.f) * GEOM_STRIDE;
            // the canonical unit vector from atom i to its neighbour j: what the list stage writes into i's row
            auto unit = [&](int i, int j, double &ux, double &uy, double &uz) {
                double vx, vy, vz;
                pair_base<ORTHO>(g, p[(size_t)j * 3] - p[(size_t)i * 3], p[(size_t)j * 3 + 1] - p[(size_t)i * 3 + 1],
                                 p[(size_t)j * 3 + 2] - p[(size_t)i * 3 + 2], vx, vy, vz);
                ux = uy = uz = 0.0;
                if (!unit_vec(vx, vy, vz, ux, uy, uz)) a.flags[0] = 1;     // (the call fails: results are discarded)
            };
            const int32_t *__restrict__ brow = d.adj + ((size_t)fl * N + (size_t)b) * RING_MAX_DEGREE;
            const int n_b = d.deg[(size_t)fl * N + (size_t)b], sb = d.species[b];
            for (int j = 0; j < n_b; j++) {         // (every bond of the frame is seen here, whether a chain runs through it or not)
                double ux, uy, uz;
                unit(b, brow[j], ux, uy, uz);
            }
            for (int jc = 0; jc < n_b && n_b >= 2; jc++) {
                const int c = brow[jc];
                if (c <= b) continue;               // (the chain is visited from its other end)
                const int32_t *__restrict__ crow = d.adj + ((size_t)fl * N + (size_t)c) * RING_MAX_DEGREE;
                const int n_c = d.deg[(size_t)fl * N + (size_t)c], sc = d.species[c];
                double u2x, u2y, u2z;
                unit(b, c, u2x, u2y, u2z);
                for (int ja = 0; ja < n_b; ja++) {
                    const int at = brow[ja];
                    if (at == c) continue;
                    const int sa = d.species[at];
                    double u1x, u1y, u1z;
                    unit(b, at, u1x, u1y, u1z);
                    for (int jd = 0; jd < n_c; jd++) {
                        const int dt = crow[jd];
                        if (dt == b || dt == at) continue;
                        const uint32_t mask = dihedral_mask(d, S, sa, sb, sc, d.species[dt]);
                        if (!mask) continue;
                        double u3x, u3y, u3z;
                        unit(c, dt, u3x, u3y, u3z);
                        dihedral_count(d, ln, mask, u1x, u1y, u1z, u2x, u2y, u2z, u3x, u3y, u3z);
                    }
                }
            }
        }
        dihedral_wave_flush(d, ln.ws, f0);
    }
    dihedral_end(d, ln);
}

// n_dihedrals[t], n_undefined[t] = the frame sums' first two columns over the frames of the call: totals [2][T]
__global__ __launch_bounds__(256) void dihedral_totals_kernel(const unsigned long long *__restrict__ fs, unsigned long long *__restrict__ totals,
                                                              int64_t F, int T)
{
    __shared__ unsigned long long part[2][256];
    const int t = blockIdx.x, tid = threadIdx.x;
    unsigned long long n0 = 0ull, n1 = 0ull;
    for (int64_t f = tid; f < F; f += 256) {
        n0 += fs[((size_t)f * T + t) * 3];
        n1 += fs[((size_t)f * T + t) * 3 + 1];
    }
    part[0][tid] = n0;
    part[1][tid] = n1;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (tid < off) {
            part[0][tid] += part[0][tid + off];
            part[1][tid] += part[1][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        totals[t] = part[0][0];
        totals[T + t] = part[1][0];
    }
}

// ------------------------------------------------------------ dihedral: host side ----
// the extents of a call's arrays, once for the run and for the zeros the entry points leave (none: no array is touched)
struct DihedralShape {
    size_t T = 0, hist_words = 0, fs_words = 0;     // hist [T][nb]; n_dihedrals, n_undefined [T]; frame_sums [F][T][3]
    DihedralShape() {}
    DihedralShape(const amof_traj *t, int32_t n_chains, int32_t nb)
        : T((size_t)n_chains), hist_words((size_t)n_chains * nb), fs_words(t->n_frames > 0 ? (size_t)t->n_frames * n_chains * 3 : 0)
    {
    }
    // host arrays; a null one is skipped
    void zero_host(uint64_t *hist, uint64_t *n_dihedrals, uint64_t *n_undefined, int64_t *frame_sums) const
    {
        if (hist) std::fill(hist, hist + hist_words, (uint64_t)0);
        if (n_dihedrals) std::fill(n_dihedrals, n_dihedrals + T, (uint64_t)0);
        if (n_undefined) std::fill(n_undefined, n_undefined + T, (uint64_t)0);
        if (frame_sums) std::fill(frame_sums, frame_sums + fs_words, (int64_t)0);
    }
};

struct DihedralCall : HistCall {
    DihedralArgs d;
    size_t hist_words = 0;
    // dynamic LDS of either kernel (the wave sums, then the histogram unless it goes to global memory) and its grid
    size_t lds_bytes() const { return (size_t)DIH_WAVES * 3 * d.T * sizeof(unsigned long long) + (d.global_hist ? 0 : hist_words * sizeof(unsigned)); }
    dim3 grid(int64_t nfr) const
    {
        const int64_t tiles = (nfr * t->n_atoms + NBRF_TILE - 1) / NBRF_TILE;
        return dim3((unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, 2048)));
    }
};

// whole-frame-in-LDS tier: BAD's list stage with the partner's index in every row entry, every chain from the rows
static int dihedral_frame_tier(DihedralCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    NbrSetup &st = c.st;
    const int S = t->n_species;
    std::vector<char> needed((size_t)S * S, 0);     // (every bonded pair; none: no bond, no chain)
    for (int x = 0; x < S; x++)
        for (int y = 0; y < S; y++)
            if (c.cutoff[x * S + y] > 0.0 && st.tiles.nsp[x] > 0 && st.tiles.nsp[y] > 0) needed[(size_t)x * S + y] = 1;
    auto chains = [&](const RowsBatch &b) -> int {
        AMOF_HIP_TRY(ctx, launch_lds(dihedral_rows_kernel, c.grid(b.nfr), dim3(NBRF_TILE), c.lds_bytes(), ctx->stream, st.a, b.la, c.d,
                                     b.sp_first, b.f_base, b.nfr));
        return AMOF_OK;
    };
    const ListsRequest rq{needed, nullptr, 0, "AMOF_DIHEDRAL_ROWS_MB", true, FRAME_DIHEDRAL};
    ListsOutcome outcome;
    int32_t qflag;
    AMOF_TRY(frame_lists_tier(c, rq, chains, outcome, qflag));
    return frame_lists_finish(c, outcome, qflag);     // (after a reset the exact kernel answers, which names the frame)
}

// index rows of every frame from the adjacency kernel, the unit vectors recomputed per chain: any cell
static int dihedral_exact_tier(DihedralCall &c)
{
    amof_ctx *ctx = c.ctx;
    const amof_traj *t = c.t;
    NbrSetup &st = c.st;
    const int64_t N = t->n_atoms, F = t->n_frames;
    if (N <= 0 || F <= 0) return AMOF_OK;
    // rows of a batch: at most 256 MB, and a flat (frame, atom) index below 2^31
    int64_t batch = std::max<int64_t>(1, ((int64_t)256 << 20) / (N * (RING_MAX_DEGREE + 1) * (int64_t)sizeof(int32_t)));
    batch = std::min<int64_t>(std::min<int64_t>(batch, F), std::max<int64_t>(1, 0x7fffff00ll / N));
    if (const char *mb = getenv("AMOF_DIHEDRAL_ROWS_MB"))
        if (atoi(mb) <= 0) batch = 1;
    void *d_adj, *d_deg;
    AMOF_TRY(ensure(ctx, SLOT_AUX0, (size_t)batch * (size_t)N * RING_MAX_DEGREE * sizeof(int32_t), &d_adj));
    AMOF_TRY(ensure(ctx, SLOT_AUX1, (size_t)batch * (size_t)N * sizeof(int32_t), &d_deg));
    c.d.adj = (const int32_t *)d_adj;
    c.d.deg = (const int32_t *)d_deg;
    int32_t *flags = (int32_t *)c.d_flags;
    timing_dom_begin(ctx, "dihedral_exact");
    int64_t launches = 0;
    for (int64_t f0 = 0; f0 < F; f0 += batch) {
        const int nf = (int)std::min<int64_t>(batch, F - f0);
        if (c.spans) c.spans->begin(0);
        AMOF_TRY(launch_bond_rows(ctx, BondRows{st.a.pos, st.a.geom, c.d.species, st.a.cutoff, (int32_t *)d_adj, (int32_t *)d_deg, &flags[2],
                                                (int32_t)N, t->n_species, (int32_t)t->n_cells, (int32_t)f0, nf}, st.geom.all_ortho));
        if (c.spans) { c.spans->end(); c.spans->begin(1); }
        const hipError_t e = with_flag(st.geom.all_ortho, [&](auto O) {
            return launch_lds(dihedral_exact_kernel<O()>, c.grid(nf), dim3(NBRF_TILE), c.lds_bytes(), ctx->stream, st.a, c.d, (int)f0, nf);
        });
        AMOF_HIP_TRY(ctx, e);
        if (c.spans) c.spans->end();
        launches++;
    }
    timing_dom_end(ctx, launches);
    int32_t fl[4];
    AMOF_TRY(c.read_flags(fl));
    if (fl[2]) return fail(ctx, AMOF_ECAPACITY, "frame %d: an atom has more than %d neighbours", fl[2] - 1, NBRL_CAP);
    if (fl[0]) return fail(ctx, AMOF_EANGLE, "Undefined angle");
    c.done = true;
    return AMOF_OK;
}

static int dihedral_check(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *chains, int32_t T, const double *edges,
                          int32_t nb, const void *hist, const void *n_dihedrals, const void *n_undefined, const void *frame_sums)
{
    AMOF_TRY(validate_traj(ctx, t, false));
    if (!cutoff || !chains || !edges || !hist || !n_dihedrals || !n_undefined || (t->n_frames > 0 && !frame_sums))
        return fail(ctx, AMOF_EINVAL, "NULL argument");
    AMOF_TRY(pore_refuse(ctx, nbr_check::chain_count(T, DIHEDRAL_MAX_CHAINS)));
    AMOF_TRY(pore_refuse(ctx, nbr_check::hist_bins(nb)));
    AMOF_TRY(pore_refuse(ctx, nbr_check::edges_increase(edges, nb)));
    const int S = t->n_species;
    AMOF_TRY(pore_refuse(ctx, nbr_check::chains_in_range(chains, T, S)));
    AMOF_TRY(pore_refuse(ctx, nbr_check::bond_matrix(cutoff, S, "cutoff")));
    if (t->n_frames == 0 || t->n_atoms == 0) return AMOF_OK;
    HostGeom geom;
    AMOF_TRY(build_geometry(ctx, t, geom));
    const double hmin = nbr_check::min_periodic_height(t->pbc, geom.rec.data(), t->n_cells);
    for (int k = 0; k < S * S; k++) AMOF_TRY(pore_refuse(ctx, nbr_check::half_height(cutoff[k], hmin)));
    return AMOF_OK;
}

// dev[3]: device buffers (hist, n_dihedrals, n_undefined) to add into, or null (the call's own are then read back into host[3])
static int dihedral_run(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *chains, int32_t T, const double *edges,
                        int32_t nb, const DihedralShape &sh, uint64_t *const dev[3], uint64_t *const host[3], int64_t *frame_sums)
{
    if (t->n_frames == 0 || t->n_atoms == 0) return AMOF_OK;
    const int S = t->n_species;
    DihedralCall c{{{ctx, t, cutoff}}};
    AMOF_TRY(nbr_setup(ctx, t, c.cutoff, BAD_TILE, c.st));
    StageSpans spans(ctx);      // list stage (or adjacency), dihedral kernels
    c.spans = &spans;
    DihedralArgs &d = c.d;
    memset(&d, 0, sizeof d);
    d.T = T;
    d.nb = nb;
    // one table: chains | masks of the species 4-tuples | species | edges
    const size_t tuples = (size_t)S * S * S * S;
    std::vector<uint32_t> table;
    if (tuples <= DIHEDRAL_TABLE_MAX && !getenv("AMOF_DIHEDRAL_NO_TABLE")) {
        table.resize(tuples);
        for (size_t k = 0; k < tuples; k++)
            table[k] = dihedral::chain_mask(chains, T, (int)(k / ((size_t)S * S * S)), (int)(k / ((size_t)S * S) % S), (int)(k / S % S), (int)(k % S));
    }
    UploadPack pk;
    const int i_edges = pk.add(edges, (size_t)(nb + 1) * sizeof(double));
    const int i_chains = pk.add(chains, (size_t)4 * T * sizeof(int32_t));
    const int i_species = pk.add(t->species, (size_t)t->n_atoms * sizeof(int32_t));
    const int i_table = table.empty() ? -1 : pk.add(table.data(), table.size() * sizeof(uint32_t));
    AMOF_TRY(upload_pack(ctx, SLOT_AUX3, pk));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));        // (an early return below must not free `table` under the copy)
    d.edges = pk.ptr<double>(i_edges);
    d.chains = pk.ptr<int32_t>(i_chains);
    d.species = pk.ptr<int32_t>(i_species);
    d.table = i_table >= 0 ? pk.ptr<uint32_t>(i_table) : nullptr;
    d.edge_step = getenv("AMOF_BAD_EDGE_TABLE") ? 0.0 : nbr_check::uniform_edge_step(edges, nb);
    c.hist_words = sh.hist_words;
    c.hs_words = c.hist_words + 2 * sh.T;
    c.fs_bytes = sh.fs_words * sizeof(int64_t);
    d.global_hist = c.hist_words + (size_t)DIH_WAVES * 3 * T * 2 > (size_t)AMOF_MAX_LDS_BINS ? 1 : 0;
    AMOF_TRY(c.alloc_outputs());
    d.hist = (unsigned long long *)c.d_hs;
    d.frame_sums = (unsigned long long *)c.d_fs;
    unsigned long long *totals = d.hist + c.hist_words;
    AMOF_TRY(c.reset_outputs());
    const char *ex = getenv("AMOF_DIHEDRAL_EXACT");
    if (!(ex && ex[0] == '1')) AMOF_TRY(dihedral_frame_tier(c));
    AMOF_TRY(stager_need(c.st.stage, t->n_frames));   // (no-op unless the frame tier was skipped)
    if (!c.done) AMOF_TRY(dihedral_exact_tier(c));
    hipLaunchKernelGGL(dihedral_totals_kernel, dim3((unsigned)T), dim3(256), 0, ctx->stream, (const unsigned long long *)d.frame_sums, totals,
                       (int64_t)t->n_frames, (int)T);
    AMOF_HIP_TRY(ctx, hipGetLastError());
    // complete and valid: to the caller
    const uint64_t *own[3] = {(const uint64_t *)d.hist, (const uint64_t *)totals, (const uint64_t *)totals + T};
    const size_t words[3] = {c.hist_words, (size_t)T, (size_t)T};
    if (dev)
        for (int k = 0; k < 3; k++) AMOF_TRY(add_into(ctx, dev[k], own[k], words[k]));
    timing_end(ctx);
    if (!dev)
        for (int k = 0; k < 3; k++) AMOF_TRY(fetch(ctx, host[k], own[k], words[k] * sizeof(uint64_t)));
    AMOF_TRY(fetch(ctx, frame_sums, c.d_fs, c.fs_bytes));
    AMOF_HIP_TRY(ctx, sync_stream(ctx));
    spans.collect();
    return AMOF_OK;
}

}  // namespace amof

using namespace amof;

extern "C" int amof_dihedral_hist(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *chains, int32_t n_chains,
                                  const double *edges, int32_t nb, uint64_t *hist, uint64_t *n_dihedrals, uint64_t *n_undefined,
                                  int64_t *frame_sums)
{
    if (!ctx) return AMOF_EINVAL;
    // the host form overwrites: zeros first, so that a failing call leaves zeros
    const bool sized = t && n_chains >= 1 && n_chains <= DIHEDRAL_MAX_CHAINS && nb > 0 && nb <= (1 << 24);
    const DihedralShape sh = sized ? DihedralShape(t, n_chains, nb) : DihedralShape();
    sh.zero_host(hist, n_dihedrals, n_undefined, frame_sums);
    AMOF_TRY(dihedral_check(ctx, t, cutoff, chains, n_chains, edges, nb, hist, n_dihedrals, n_undefined, frame_sums));
    uint64_t *const host[3] = {hist, n_dihedrals, n_undefined};
    const int rc = dihedral_run(ctx, t, cutoff, chains, n_chains, edges, nb, sh, nullptr, host, frame_sums);
    if (rc != AMOF_OK) {
        (void)sync_stream(ctx);
        sh.zero_host(hist, n_dihedrals, n_undefined, frame_sums);
    }
    return rc;
}

extern "C" int amof_dihedral_hist_dev(amof_ctx *ctx, const amof_traj *t, const double *cutoff, const int32_t *chains, int32_t n_chains,
                                      const double *edges, int32_t nb, uint64_t *hist_dev, uint64_t *n_dihedrals_dev,
                                      uint64_t *n_undefined_dev, int64_t *frame_sums)
{
    if (!ctx) return AMOF_EINVAL;
    AMOF_TRY(dihedral_check(ctx, t, cutoff, chains, n_chains, edges, nb, hist_dev, n_dihedrals_dev, n_undefined_dev, frame_sums));
    const DihedralShape sh(t, n_chains, nb);
    sh.zero_host(nullptr, nullptr, nullptr, frame_sums);
    uint64_t *const dev[3] = {hist_dev, n_dihedrals_dev, n_undefined_dev};
    const int rc = dihedral_run(ctx, t, cutoff, chains, n_chains, edges, nb, sh, dev, nullptr, frame_sums);
    if (rc != AMOF_OK && t->n_frames > 0) {
        (void)sync_stream(ctx);
        sh.zero_host(nullptr, nullptr, nullptr, frame_sums);
    }
    return rc;
}
