// Which kernel family answers an RDF call (rdf.hip: rdf_cell, rdf_range, rdf_tile / _zf / _img / _tri, rdf_exact), the
// guards, per-cell records and chunk sizes it runs from.  Host only (no HIP dependency: the CPU test suite compiles it with
// g++, tests/test_rdf_select_cpu.py through tests/native/rdf_select_driver.cpp).
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/amof_hip.h"
#include "guard_math.h"
#include "tile_plan.h"
#include "tri_select.h"

namespace amof {

constexpr int IMG_QUEUE_MAX = 1024; // IMG variant: parked near-face pairs per step and buffer (capacity chosen by the host)
constexpr int FAST_TILE = 512;      // two centre atoms per thread
constexpr int FAST_SUB = 128;
constexpr int FAST_TRASH = 32;      // tile kernel: words behind the LDS histogram that take the out-of-range pairs (fast_bin<AA>)
constexpr int RDF_CELL_ATOM_BITS = 26;      // = CELL_SPECIES_SHIFT: the cell kernel keeps the species above the atom index
static_assert(FAST_SUB == TILE_PLAN_SUB && FAST_TILE == TILE_PLAN_MAX_SUBS * TILE_PLAN_SUB, "tile_plan.h");

// ---- the AMOF_RDF_* switches (tests / measurements), read once per call ----
struct RdfSwitches {
    bool v1 = false;            // AMOF_RDF_KERNEL=v1: the exact kernels only
    bool noimg = false;         // AMOF_RDF_NOIMG (set): never the image-aware tile variant
    bool force_img = false;     // AMOF_RDF_FORCE_IMG (set): the image-aware variant on a plain case, never TRI
    bool notri = false;         // AMOF_RDF_NOTRI (set): never the general-cell variant in the orthogonalised frame
    bool nohalf = false;        // AMOF_RDF_NOHALF (set): TRI never with the exact-half x wrap (codes 10 / 11)
    bool debug = false;         // AMOF_RDF_DEBUG (set): the TRI selection and the tile kernel's granted workgroups per CU on stderr
    bool nocull = false;        // AMOF_RDF_NOCULL=1: tile kernels without slab culling
    bool nozf = false;          // AMOF_RDF_NOZF=1: diagonal cells without the f32 slab coordinates
    bool noreach = false;       // AMOF_RDF_NOREACH=1: every quad of a diagonal tile pair masked (rdf_tile_kernel_fast, REACH)
    bool plan_noskip = false;   // AMOF_RDF_PLAN_NOSKIP=1: planned steps without a quad to visit are run all the same
    bool noplan = false;        // AMOF_RDF_NOPLAN=1: rdf_tile_zf searches the sampled quads in every step, no plan
    bool noahead = false;       // AMOF_RDF_NOAHEAD=1: planned kernel without the partner records read a quad ahead
    bool nosat = false;         // AMOF_RDF_NOSAT=1: planned kernel's f32-slab slice with the clamped tail, not the saturating one
    bool notail = false;        // AMOF_RDF_NOTAIL (set): XCD mapping without the one-frame rows behind the chunks
    bool nocell = false;        // AMOF_RDF_NOCELL (set): never the 3-D cell-list kernel
    bool force_cell = false;    // AMOF_RDF_FORCE_CELL (set): the cell-list kernel wherever it is correct
    bool notrim = false;        // AMOF_RDF_NOTRIM (set): cell kernel without the trimmed partner ranges
    bool cell_gather = false;   // AMOF_RDF_CELL_GATHER (set): one lane per centre instead of one wave per cell
    bool norange = false;       // AMOF_RDF_NORANGE (set): never the two-level range kernel
    bool force_range = false;   // AMOF_RDF_FORCE_RANGE (set): the range kernel wherever it is correct
    int batch = 0;              // AMOF_RDF_BATCH: frames per batch at most (0: unset)
    int fpc = 0;                // AMOF_RDF_FPC: tile kernel, frames per workgroup chunk (0: unset)
    int cell_fpc = 0;           // AMOF_RDF_CELL_FPC: cell kernel, frames per workgroup (0: unset)
    int cell_cpw = 0;           // AMOF_RDF_CELL_CPW: cell kernel, cell groups per workgroup (0: unset)

    static RdfSwitches from_env()
    {
        auto set = [](const char *n) { return getenv(n) != nullptr; };
        auto one = [](const char *n) { const char *v = getenv(n); return v && v[0] == '1'; };
        auto num = [](const char *n) { const char *v = getenv(n); return v ? std::max(1, atoi(v)) : 0; };
        RdfSwitches s;
        const char *k = getenv("AMOF_RDF_KERNEL");
        s.v1 = k && strcmp(k, "v1") == 0;
        s.noimg = set("AMOF_RDF_NOIMG"); s.force_img = set("AMOF_RDF_FORCE_IMG"); s.notri = set("AMOF_RDF_NOTRI");
        s.nohalf = set("AMOF_RDF_NOHALF"); s.debug = set("AMOF_RDF_DEBUG"); s.notail = set("AMOF_RDF_NOTAIL");
        s.nocell = set("AMOF_RDF_NOCELL"); s.force_cell = set("AMOF_RDF_FORCE_CELL"); s.notrim = set("AMOF_RDF_NOTRIM");
        s.cell_gather = set("AMOF_RDF_CELL_GATHER"); s.norange = set("AMOF_RDF_NORANGE"); s.force_range = set("AMOF_RDF_FORCE_RANGE");
        s.nocull = one("AMOF_RDF_NOCULL"); s.nozf = one("AMOF_RDF_NOZF"); s.noreach = one("AMOF_RDF_NOREACH");
        s.plan_noskip = one("AMOF_RDF_PLAN_NOSKIP"); s.noplan = one("AMOF_RDF_NOPLAN"); s.noahead = one("AMOF_RDF_NOAHEAD");
        s.nosat = one("AMOF_RDF_NOSAT");
        s.batch = num("AMOF_RDF_BATCH"); s.fpc = num("AMOF_RDF_FPC"); s.cell_fpc = num("AMOF_RDF_CELL_FPC");
        s.cell_cpw = num("AMOF_RDF_CELL_CPW");
        return s;
    }
};

// ---- per-cell record of the fast paths (one per frame when the cell changes) ----
struct FrameScale {
    float sc[9];        // ORTHO: sc[0..2] = L_k * 2^-32 / dr, sc[3..5] their squares ; else the lower-triangular factor of the
                        // metric of cell * 2^-32 / dr (rows in stored order): sc[0], sc[3], sc[4], sc[6..8]; the others 0
    uint32_t cull_gap;  // slab-gap threshold of this cell (0 = culling off)
    uint32_t near_t[3]; // IMG variant: a pair with |i_k| > near_t[k] (stored axis order) is evaluated canonically
    uint32_t _pad;
    double sc64[9];     // the same factors in f64 (level-2 refinement)
    // TRI variant (see RdfTri in rdf.hip): sc[3..5] = L00^2, L11^2, L22^2, sc[8] = L22 (units: bins per 2^-32 of the axis)
    uint32_t tri_kx, tri_ky;    // round(kx 2^32), round(ky 2^32) mod 2^32: what one cell of slab wrap adds to the folded x'', y'
    float tri_c10;              // L10 / L00
    float tri_near_y;           // a pair with |fl(iy)| > tri_near_y may have a second image in range (+inf: never)
    float tri_near_z;           // likewise |dz| (bins) > tri_near_z
    float tri_near_x;           // likewise |fl(ix + c10 iy)| (slow path only: the variant is refused when the fast path would need it)
};

// cells: [nc][9]; ord: the stored component order; cull_gap (optional): [nc]; near_thr (optional): [nc][3] in the cell's
// own axis order (stored permuted).  The TRI fields are left alone.
inline void fill_frame_scales(const double *cells, int64_t nc, bool ortho, const int ord[3], double dr, const uint32_t *cull_gap,
                              const uint32_t *near_thr, FrameScale *out)
{
    const double two32 = 1.0 / 4294967296.0;
    for (int64_t k = 0; k < nc; k++) {
        const double *c = cells + 9 * k;
        FrameScale &r = out[k];
        for (int q = 0; q < 9; q++) r.sc64[q] = 0.0;
        if (ortho) {
            for (int q = 0; q < 3; q++) r.sc64[q] = c[4 * ord[q]] * two32 / dr;
        } else {
            double rows[9];
            for (int q = 0; q < 3; q++)
                for (int x = 0; x < 3; x++) rows[3 * q + x] = c[3 * ord[q] + x] * two32 / dr;
            lower_factor(rows, r.sc64);
        }
        for (int q = 0; q < 9; q++) r.sc[q] = (float)r.sc64[q];
        if (ortho)
            for (int q = 0; q < 3; q++) r.sc[3 + q] = (float)(r.sc64[q] * r.sc64[q]);
        r.cull_gap = cull_gap ? cull_gap[k] : 0u;
        for (int q = 0; q < 3; q++) r.near_t[q] = near_thr ? near_thr[(size_t)k * 3 + ord[q]] : 0x7fffffffu;
        r._pad = 0u;
    }
}

// TRI: records from the selection's rec [nc][9] (tri_select.h); cull_gap: [nc], as the plain records of the same slab axis
inline void fill_frame_scales_tri(const double *tri_rec, int64_t nc, const uint32_t *cull_gap, FrameScale *out)
{
    auto down = [](double v) {      // largest float <= v
        if (!(v < INFINITY)) return (float)INFINITY;
        float f = (float)v;
        if ((double)f > v) f = nextafterf(f, -INFINITY);
        return f;
    };
    for (int64_t k = 0; k < nc; k++) {
        FrameScale &r = out[k];
        memset(&r, 0, sizeof r);
        const double *tr = &tri_rec[(size_t)k * 9];
        r.sc64[0] = tr[0]; r.sc64[3] = tr[1]; r.sc64[4] = tr[2]; r.sc64[8] = tr[3];
        r.sc[3] = (float)(tr[0] * tr[0]); r.sc[4] = (float)(tr[2] * tr[2]); r.sc[5] = (float)(tr[3] * tr[3]);
        r.sc[8] = (float)tr[3];
        r.tri_c10 = (float)(tr[1] / tr[0]);
        r.tri_near_y = down(tr[4]);
        r.tri_near_z = down(tr[5]);
        r.tri_near_x = down(tr[8]);
        r.tri_kx = (uint32_t)(long long)rint(tr[6] * 4294967296.0);
        r.tri_ky = (uint32_t)(long long)rint(tr[7] * 4294967296.0);
        r.cull_gap = cull_gap[k];
        for (int q = 0; q < 3; q++) r.near_t[q] = 0x7fffffffu;
    }
}

// thresholds in f32 with directed rounding, so that the f64 bound `guard` is never undercut
struct GuardThresholds {
    float nb_hi;            // nbins + guard rounded UP
    float half_m_guard;     // 1/2 - guard rounded DOWN
};
inline GuardThresholds guard_thresholds(int nbins, double guard)
{
    const double hi = (double)nbins + guard, half = 0.5 - guard;
    GuardThresholds g = {(float)hi, (float)half};
    if ((double)g.nb_hi < hi) g.nb_hi = nextafterf(g.nb_hi, INFINITY);
    if ((double)g.half_m_guard > half) g.half_m_guard = nextafterf(g.half_m_guard, -INFINITY);
    return g;
}

// the saturating tail (rdf_sat_math.h): q' = q~ + g + 1 is flagged when fract(q') < 2 g
struct SatThresholds {
    float one_p_guard;      // 1 + guard rounded to nearest (its rounding error is a term of the bound: fast_guard_zf_sat)
    float two_guard;        // 2 guard rounded UP
};
inline SatThresholds sat_thresholds(double guard)
{
    SatThresholds g = {(float)(1.0 + guard), (float)(2.0 * guard)};
    if ((double)g.two_guard < 2.0 * guard) g.two_guard = nextafterf(g.two_guard, INFINITY);
    return g;
}

// Parked pairs of the IMG / TRI variants; share: expected share of a step's 128 x 512 pairs that is parked.  Small shares:
// two buffers of >= 96 entries, evaluated a step later -- small enough for five workgroups per CU and no extra barrier;
// larger shares: one buffer of 1024, evaluated at the end of the step.
struct ParkedQueue {
    int32_t img_queue, img_defer;
};
inline ParkedQueue parked_queue(double share)
{
    const double expect = share * (double)FAST_SUB * FAST_TILE;
    const double want = std::max(96.0, ceil(4.0 * expect / 32.0) * 32.0);
    ParkedQueue q;
    q.img_defer = want <= 256.0 ? 1 : 0;
    q.img_queue = q.img_defer ? (int32_t)want : IMG_QUEUE_MAX;
    return q;
}
// dynamic LDS of the tile kernel: two partner tiles and centre sub-tiles, the histogram with its trash words, the queues
// plan: a planned launch (rdf_tile_kernel_fast, PLAN) has no centre buffers -- 25 760 bytes at the headline's 2310 bins, six
// workgroups in a CU's 160 KiB where 29 856 allow five
// sat: the saturating tail's histogram sits one word up (word 0 is a pad) -- 25 776 bytes at 2310 bins, still six workgroups
inline size_t tile_lds(int nbins, int32_t queue, int32_t defer, bool plan = false, bool sat = false)
{
    const size_t base = 2 * (FAST_TILE + (plan ? 0 : FAST_SUB)) * 16 +
                        (size_t)((nbins + FAST_TRASH + 2 + (sat ? 1 : 0) + 3) & ~3) * sizeof(unsigned);
    return queue ? base + (defer ? 2 : 1) * (size_t)queue * 8 + 16 : base;
}

// ---- the selection ----
struct RdfSelect {
    double csum = 0.0;          // largest sum of cell-vector lengths: bounds the fixed-point grid error
    double quant = 0.0, guard_m = 0.0, guard_f = 0.0;
    bool plain = false;         // cutoff clear of every half height: base image only (tile, cell-list and range kernels)
    bool img = false;           // image-aware tile variant
    double img_share = 0.0;
    std::vector<uint32_t> near_thr;     // IMG: [nc][3] fixed-point threshold on |i_k|, the cell's own axis order
    TriSelect tri;              // tri.ok: the general-cell variant in the orthogonalised lattice frame (excludes img)
    bool tile() const { return plain || img || tri.ok; }
    int axis = 0;               // slab axis
    double hmin[3] = {1e300, 1e300, 1e300};
    bool cull = false;
    std::vector<uint32_t> cull_gap;     // [nc] (0: culling off)
    GuardThresholds thr = {0.f, 0.f};
    bool zf = false;            // diagonal cells: slab-axis difference from f32 coordinates
    GuardThresholds zf_thr = {0.f, 0.f};
    bool sat = false;           // the planned f32-slab slice runs the saturating tail (needs zf and cull; the plan is the tier's choice)
    double guard_zf_sat = 0.0;  // its candidate's error bound g (bins), grid term included
    SatThresholds sat_thr = {0.f, 0.f};
    bool cell = false;          // 3-D cell list
    int nk[3] = {0, 0, 0};
    bool range = false;         // two-level cell list
    int nz2 = 0, axis_y = 0, gy = 0;
};

// cells: [nc][9]; heights: [nc][3] perpendicular heights (geometry records); nsp: [S] atoms per species
inline RdfSelect rdf_select(const double *cells, const double *heights, int64_t nc, const uint8_t *pbc, int S, int64_t N,
                            const int64_t *nsp, int nbins, double rmax, int max_img, bool all_ortho, const RdfSwitches &sw)
{
    RdfSelect s;
    const double dr = rmax / nbins;
    auto height = [&](int64_t k, int x) { return heights[(size_t)k * 3 + x]; };
    for (int64_t k = 0; k < nc; k++) {
        const double *c = cells + 9 * k;
        s.csum = std::max(s.csum, sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]) + sqrt(c[3] * c[3] + c[4] * c[4] + c[5] * c[5]) +
                                      sqrt(c[6] * c[6] + c[7] * c[7] + c[8] * c[8]));
    }
    // fractional coordinates are truncated to 2^-32: a pair vector moves by < csum * 2^-32;
    // quant carries a factor 2 of margin (it also covers the f64 rounding of the fold, |s| < 1e4)
    s.quant = s.csum * (1.0 / 2147483648.0);
    s.guard_m = s.quant / dr + (double)nbins * 1e-12;
    // f32 candidate: relative error bound of the chain, see fast_guard_rel_rdf (guard_math.h)
    s.guard_f = (double)nbins * fast_guard_rel_rdf(all_ortho, cells, nc) + s.guard_m;
    s.thr = s.zf_thr = guard_thresholds(nbins, s.guard_f);
    const double R = rmax * (1.0 + 4.0 * s.guard_f / (double)nbins + 1e-6);     // the cutoff with its guards
    // what every fast tier needs: all periodic, the histogram in LDS beside the tiles, a guard that leaves room in a bin
    const bool feasible = pbc[0] && pbc[1] && pbc[2] && nbins <= AMOF_MAX_LDS_BINS - 5120 && s.guard_f < 0.25 && !sw.v1;
    bool fast = feasible && max_img == 0;
    if (fast && !all_ortho) {
        // At |s_k| = 1/2 the wrapped fixed-point image and the canonical rint() image can be different
        // lattice images of unequal length in a sheared cell (equal in a diagonal one): keep both
        // decisively out of range, i.e. the cutoff clear of every half height by more than the guards.
        for (int64_t k = 0; k < nc && fast; k++)
            for (int x = 0; x < 3; x++)
                if (R >= 0.5 * height(k, x)) fast = false;
    }
    // Image-aware variant of the tile kernel: the cutoff reaches beyond half a cell height (further periodic
    // images count) or comes too close to it.  Pairs whose fractional difference lies within reach of a cell
    // face are evaluated canonically (base + every listed image); all others can only have their base image
    // in range, and that base is unambiguous.  near_thr[cell][axis]: fixed-point threshold on |i_k|.
    if (!fast && feasible && max_img <= 124 && !sw.noimg) {
        s.img = true;
        s.near_thr.assign((size_t)nc * 3, 0x7fffffffu);
        for (int64_t k = 0; k < nc && s.img; k++) {
            double share = 0.0;      // expected share of the pairs that go the canonical way
            for (int x = 0; x < 3; x++) share += 2.0 * std::max(0.0, rmax / height(k, x) - 0.5);
            // the parking queue holds 1024 of a step's 65 536 pairs; beyond that the exact kernels are the better choice
            if (share > 0.03) s.img = false;
            s.img_share = std::max(s.img_share, share);
        }
        for (int64_t k = 0; k < nc && s.img; k++)
            for (int x = 0; x < 3; x++) {
                // beyond |s| = 1/2 - tau an image shifted along this axis could come within the cutoff
                const double tau = R / height(k, x) - 0.5 + 1e-9;
                const double thr = 0.5 - std::max(tau, 0.0) - 1e-9;
                if (tau <= 0.0) {
                    // clear of this half height by more than the guards: only an exact tie is ambiguous
                    s.near_thr[(size_t)k * 3 + x] = 0x7fffffffu;
                } else if (thr < 0.3) {
                    s.img = false;      // two fifths of the pairs or more would go the canonical way
                } else {
                    s.near_thr[(size_t)k * 3 + x] = (uint32_t)floor(thr * 4294967296.0) - 2u;
                }
            }
    }
    if (fast && sw.force_img) {   // tests / measurements: the image-aware variant on a plain case
        fast = false;
        s.img = true;
        s.near_thr.assign((size_t)nc * 3, 0x7fffffffu);
    }
    s.plain = fast;
    // ---- TRI: general cells in the orthogonalised lattice frame (see fast_quad_tri; the selection: tri_select.h) ----
    if (!all_ortho && max_img <= 124 && feasible && !sw.notri && !sw.force_img) {
        s.tri = tri_select(cells, heights, nc, rmax, nbins, s.guard_f, s.quant, dr, sw.nohalf);
        if (s.tri.ok) {      // (the guard of its candidate at the widest reach must leave room between the bin edges)
            double hb = 0.0;
            for (int64_t k = 0; k < nc; k++) hb = std::max(hb, height(k, s.tri.axis) / dr);
            if (!(fast_guard_tri(nbins, hb, 0.5, s.tri.l10_bins) * (1.0 + 4.0 * s.tri.tau) + 2.0 * s.quant / dr +
                  (1.0 + 256.0 * s.tri.c10) * 1.5 * s.csum * (1.0 / 4294967296.0) / dr + (double)nbins * 1e-12 < 0.25)) s.tri.ok = false;
        }
    }
    if (s.tri.ok) s.img = false;
    if (!s.tile()) return s;
    // slab axis = the axis whose smallest perpendicular height over the trajectory is largest;
    // culling only pays when 2 rmax < h
    for (int64_t k = 0; k < nc; k++)
        for (int x = 0; x < 3; x++) s.hmin[x] = std::min(s.hmin[x], height(k, x));
    for (int x = 1; x < 3; x++)
        if (s.hmin[x] > s.hmin[s.axis]) s.axis = x;
    const int axis = s.axis;
    s.cull = !sw.nocull && 2.0 * rmax * 1.05 < s.hmin[axis];
    // a block is skipped when the slab gap alone exceeds rmax (1e-6 relative and 4 grid units of slack)
    s.cull_gap.assign((size_t)nc, 0u);
    for (int64_t k = 0; k < nc && s.cull; k++)
        s.cull_gap[(size_t)k] = (uint32_t)std::min(4294967295.0, ceil(rmax / height(k, axis) * 4294967296.0 * (1.0 + 1e-6)) + 4.0);
    // Diagonal cells: the tile kernel takes the slab-axis difference from f32 coordinates (ZF, see fast_q_zf) --
    // with slab culling for every visited partner, without it for all but a band around the sub-tile's antipode;
    // its candidate carries one more absolute term, hence its own (slightly wider) guard.
    s.zf = (s.plain || s.tri.ok) && !s.img && all_ortho && !sw.nozf;
    if (s.zf) {
        double hb = 0.0, gfrac = 0.0;
        for (int64_t k = 0; k < nc; k++) {
            hb = std::max(hb, height(k, axis) / dr);
            gfrac = std::max(gfrac, s.cull ? (double)s.cull_gap[(size_t)k] / 4294967296.0 : 0.5);   // (no culling: reach 2^31)
        }
        const double guard_zf = fast_guard_zf(nbins, hb, gfrac) + s.guard_m;
        if (!(guard_zf < 0.25)) s.zf = false;
        s.zf_thr = guard_thresholds(nbins, guard_zf);
        // the planned slice's saturating tail: its chain has its own roundings, hence its own guard
        s.guard_zf_sat = fast_guard_zf_sat(nbins, hb, gfrac) + s.guard_m;
        s.sat = s.zf && s.cull && !sw.nosat && s.guard_zf_sat < 0.25;
        s.sat_thr = sat_thresholds(s.guard_zf_sat);
    }
    // ---- 3-D cell list for cutoffs far below the cell size (cell kernel) ----
    s.cell = s.plain && S <= 16 && N < (1ll << RDF_CELL_ATOM_BITS) && N >= 64 && !sw.nocell;
    for (int x = 0; x < 3; x++) {
        s.nk[x] = (int)std::min(1024.0, floor(s.hmin[x] / (0.5 * rmax * (1.0 + 1e-5))));
        if (s.nk[x] < 5) s.cell = false;
    }
    if (((size_t)(S * (S + 1) / 2) * nbins + (size_t)S * S) * sizeof(unsigned) > 96 * 1024) s.cell = false;
    if (s.cell) {
        // no point in cells emptier than ~2 atoms: thicker cells are still correct (reach stays 2)
        while ((int64_t)s.nk[0] * s.nk[1] * s.nk[2] > std::max<int64_t>(125, N / 2)) {
            int big = 0;
            for (int x = 1; x < 3; x++)
                if (s.nk[x] > s.nk[big]) big = x;
            if (s.nk[big] <= 5) break;
            s.nk[big]--;
        }
        // visited share of all pairs: half shell of 5x5x5 cells (lane utilisation ~0.8) vs the slab list's
        // f1c / 2; a gathered pair costs ~1.8x a broadcast one and the sort is a fixed cost per frame
        // (crossovers measured with profiles/tools/sweep_cell.py)
        const double f3 = 62.5 / ((double)s.nk[0] * s.nk[1] * s.nk[2]) / 0.8;
        const double f1c = std::min(1.0, 2.0 * rmax / s.hmin[axis] + 2.0 / 256 + 0.02);
        if (!(f3 < 0.32 * f1c && N >= 4000) && !sw.force_cell) s.cell = false;
    }
    // ---- two-level cell list for small cutoffs (range kernel) ----
    s.axis_y = (axis + 1) % 3;
    if (s.hmin[(axis + 2) % 3] > s.hmin[s.axis_y]) s.axis_y = (axis + 2) % 3;
    s.nz2 = (int)std::min(64.0, floor(s.hmin[axis] / (rmax * (1.0 + 1e-5))));
    if (s.plain && s.nz2 >= 3 && nc == 1 && !s.cell && !sw.norange) {
        // visited share of the partners: 1-D slab list vs (3 slabs) x (y strip + 2 rmax)
        int64_t nmax = 0;
        for (int x = 0; x < S; x++) nmax = std::max<int64_t>(nmax, nsp[x]);
        const double strip = std::min(1.0, (double)FAST_SUB * s.nz2 / std::max<double>(1.0, (double)nmax));
        const double f1 = std::min(1.0, 2.0 * rmax / s.hmin[axis] + 2.0 / 256 + 0.02);
        const double f2 = std::min(1.0, 3.0 / s.nz2) * std::min(1.0, 2.0 * rmax / s.hmin[s.axis_y] + strip + 2.0 / 256);
        s.range = f2 < 0.6 * f1 || sw.force_range;   // (forced: tests)
    }
    if (s.range) s.gy = (int)ceil(rmax * (1.0 + 1e-5) / s.hmin[s.axis_y] * 256.0) + 1;
    return s;
}

// ---- chunk rules ----
// frames of a batch held at once: 2^30 bytes of scratch, at most 32768 frames, at most F
inline int64_t frame_batch(int64_t bytes_per_frame, int64_t F)
{
    const int64_t fb = std::max<int64_t>(1, (int64_t)(1ll << 30) / std::max<int64_t>(1, bytes_per_frame));
    return std::min<int64_t>(std::min<int64_t>(fb, 32768), F);
}

// Tile kernel, frames per workgroup chunk: ~80k workgroups per launch (1280 run at a time: > 60 rounds, so that
// ramp-up and drain stay around 1-2 %), between 2 and 16 frames -- fewer frames flush the LDS histogram
// more often (u64 global atomics: HBM-side write traffic), more do not fit the 4 MiB L2 of an XCD.
// Measured on cfg3 (profiles/r02/rdf_fpc_sweep.txt): a 625-frame shard 11.33 (10 frames) -> 11.08 ms (2);
// 5000 frames stay at 16 (8 would be 0.5 % faster for 38 % more traffic).
struct TileChunks {
    int32_t fpc, chunks, xcd_map, nf_tail, nf_main;
    bool plan_fits;     // a work item keeps the live steps of its chunk in 64 bits: four per frame
};
inline TileChunks tile_chunks(int64_t nf, int64_t npairs, const RdfSwitches &sw)
{
    int64_t fpc = (nf * npairs + 40000) / 80000;
    fpc = std::max<int64_t>(2, std::min<int64_t>(fpc, 16));
    if (sw.fpc) fpc = sw.fpc;     // experiments
    fpc = std::min<int64_t>(fpc, std::max<int64_t>(1, nf));
    if (nf >= 64) fpc = std::min<int64_t>(fpc, nf / 32);   // >= 32 chunks: every XCD gets >= 4
    int64_t chunks = (nf + fpc - 1) / fpc;
    TileChunks c;
    c.xcd_map = chunks >= 32 ? 1 : 0;
    // the XCD mapping deals chunks in groups of 8, over a number of frames that divides by 8; the rest: one grid
    // row per frame behind the chunks (rdf_tile_kernel_fast)
    c.nf_tail = (int32_t)(c.xcd_map && !sw.notail ? nf % 8 : 0);
    if (c.xcd_map) chunks = ((nf - c.nf_tail + fpc - 1) / fpc + 7) / 8 * 8;
    c.fpc = (int32_t)fpc;
    c.chunks = (int32_t)chunks;
    c.nf_main = (int32_t)(nf - c.nf_tail);
    c.plan_fits = (c.nf_main + chunks - 1) / chunks <= 64 / TILE_PLAN_MAX_SUBS;
    return c;
}

// Cell kernel: frames per workgroup (>= ~8k workgroups per launch, 32 per CU; at most 8 frames: the u32 counters of a chunk,
// 8 frames x 512 atoms x ~300 partners, stay far below 2^32) and, one wave per cell, cell groups per workgroup (the
// histogram flush is paid per workgroup and chunk, a cell and frame bring ~1e3 pairs: at most 8 groups).
// gx: workgroups along x of one frame; groups: cell groups (0: the per-lane gather form)
struct CellChunks {
    int32_t xcd_map, fpc, frames_grid, cpw;
    unsigned gx;
};
inline CellChunks cell_chunks(int64_t nf, unsigned gx, int64_t groups, const RdfSwitches &sw)
{
    CellChunks c;
    c.xcd_map = nf >= 16 ? 1 : 0;
    const int64_t frames = c.xcd_map ? (nf + 7) / 8 * 8 : nf;
    const int64_t slots = c.xcd_map ? frames / 8 : frames;       // per XCD
    int64_t fpc = std::max<int64_t>(1, std::min<int64_t>(8, (int64_t)gx * frames / 8192));
    if (sw.cell_fpc) fpc = sw.cell_fpc;      // experiments / tests
    fpc = std::min<int64_t>(fpc, slots);
    c.fpc = (int32_t)fpc;
    const int64_t chunks = (slots + fpc - 1) / fpc;
    c.frames_grid = (int32_t)(c.xcd_map ? chunks * 8 : chunks);
    c.cpw = 1;
    c.gx = gx;
    if (groups > 0) {
        int64_t cpw = std::max<int64_t>(1, std::min<int64_t>(8, groups * c.frames_grid / 8192));
        if (sw.cell_cpw) cpw = sw.cell_cpw;            // experiments / tests
        cpw = std::min<int64_t>(cpw, groups);
        c.cpw = (int32_t)cpw;
        c.gx = (unsigned)((groups + cpw - 1) / cpw);
    }
    return c;
}

// Exact kernels: enough workgroups to fill 256 CUs several times over, few enough flushes that the u64 global atomics stay
// negligible; at most fpc_max frames per chunk (the range kernel takes the same rule with 16)
inline void pick_chunks(int64_t nframes, int64_t work, int64_t fpc_max, int32_t &fpc_out, unsigned &chunks_out)
{
    int64_t want_chunks = (8 * 2048 + work - 1) / work;
    int64_t fpc = std::max<int64_t>(1, nframes / std::max<int64_t>(1, want_chunks));
    fpc = std::min<int64_t>(fpc, fpc_max);
    int64_t chunks = (nframes + fpc - 1) / fpc;
    if (chunks > 65535) {
        fpc = (nframes + 65534) / 65535;
        chunks = (nframes + fpc - 1) / fpc;
    }
    fpc_out = (int32_t)fpc;
    chunks_out = (unsigned)chunks;
}

}  // namespace amof
