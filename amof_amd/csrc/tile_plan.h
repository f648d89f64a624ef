// The partner window of one step of the slab-culled tile kernel (rdf.hip: rdf_tile_kernel_fast, REACH with a plan), from the
// quantiser's slab table instead of ballots over sampled quads.  Host and device (no HIP dependency on the host side: the
// CPU test suite compiles it with g++, tests/test_tile_plan_cpu.py).
//
// A step = (frame, centre sub-tile of tile I, tile J).  Tile J is a contiguous piece [toff, toff + cntj) of its species
// segment, which the quantiser sorted into 256 slabs along the slab axis; start[s] (s = 0 .. 256, relative to the segment)
// is the first atom of slab s.  The centres' slabs are [s_first, s_last]; their keys (32-bit fixed point along the slab
// axis) lie in [wlo, whi] = [s_first << 24, (s_last << 24) | 0xffffff], and a partner farther than G = cull_gap from all
// of them (circular) is out of range.  The rules are the kernel's own:
//   * the reach [wlo - G, whi + G] (mod 2^32) is widened to whole slabs [slo, shi];
//   * a span W + 2 G + 2 slabs >= 2^32 (or G = 0) means no culling for the step;
//   * of a diagonal tile pair, sub-tile `sub` starts at its own block, 128 sub;
//   * a wrapped reach gives two pieces, [0, first of slab > shi) and [first of slab >= slo, cntj); where their quads touch,
//     the whole tile is visited;
//   * quads (4 partners) are visited whole, and never twice.
// Every index is clamped into [0, cntj]: no table content can yield a range outside the tile.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define AMOF_TILE_PLAN_HD __host__ __device__
#else
#define AMOF_TILE_PLAN_HD
#endif

namespace amof {

constexpr int TILE_PLAN_SLABS = 256;    // = QSLABS
constexpr int TILE_PLAN_SUB = 128;      // = FAST_SUB: centre atoms per sub-tile
constexpr int TILE_PLAN_MAX_SUBS = 4;   // = FAST_TILE / FAST_SUB: records per (tile pair, frame)

struct TileWindow {
    int32_t qb[2], qe[2];   // the step's quad ranges [qb, qe): multiples of 4; empty when qe <= qb
    int32_t mz[2];          // cells of slab wrap between the centres and the partners of piece 0 / 1 (-1, 0, + 1)
    int32_t zf;             // 1: the slab differences of the step cannot wrap, f32 slab coordinates are valid
};

// first atom of the tile whose slab is >= s (s = 0 .. 256), as an index into the tile
AMOF_TILE_PLAN_HD inline int tile_plan_first(const uint32_t *start, uint32_t s, int toff, int cntj)
{
    const int64_t v = (int64_t)start[s] - (int64_t)toff;
    return (int)(v < 0 ? 0 : (v > (int64_t)cntj ? (int64_t)cntj : v));
}

// slab of atom k of the species segment (the largest s < 256 with start[s] <= k; a k outside the segment: 0 or 255)
AMOF_TILE_PLAN_HD inline uint32_t tile_plan_slab_of(const uint32_t *start, uint32_t k)
{
    uint32_t lo = 0u, hi = TILE_PLAN_SLABS;      // start[lo] <= k < start[hi], as far as the table is monotone
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (start[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

AMOF_TILE_PLAN_HD inline TileWindow tile_plan_window(const uint32_t *start, int toff, int cntj, uint32_t s_first, uint32_t s_last,
                                                     uint32_t G, bool diag, int sub)
{
    TileWindow w = {{0, 0}, {0, 0}, {0, 0}, 0};
    if (cntj <= 0) return w;
    s_first &= 255u;
    s_last &= 255u;
    const uint32_t wlo = s_first << 24, whi = (s_last << 24) | 0xffffffu;
    const uint32_t W = whi - wlo;
    const int own = diag ? sub * TILE_PLAN_SUB : 0;
    int rb0 = own < cntj ? own : cntj, re0 = cntj, rb1 = 0, re1 = 0;
    const uint64_t span = (uint64_t)W + 2ull * G + (2ull << 24);
    if (G != 0u && span < (1ull << 32)) {
        const uint32_t klo = wlo - G, khi = whi + G;
        const uint32_t slo = klo >> 24, shi = khi >> 24;
        // a_: start of the quad that holds the first partner of slab >= slo;  b_: start of the first quad behind every
        // partner of slab <= shi
        const int A = tile_plan_first(start, slo, toff, cntj), B = tile_plan_first(start, shi + 1u, toff, cntj);
        const int a_ = A >= cntj ? cntj : (A & ~3);
        const int b4 = (B + 3) & ~3, b_ = b4 < cntj ? b4 : cntj;
        if (klo <= khi) {
            rb0 = rb0 > a_ ? rb0 : a_;
            re0 = b_;
        } else if (b_ < a_) {       // wrapped reach: keys <= khi or >= klo
            re0 = b_;
            rb1 = rb0 > a_ ? rb0 : a_;
            re1 = cntj;
            if (khi < whi) w.mz[0] = -1;
            if (wlo < G) w.mz[1] = 1;
        }                           // else the two pieces touch: whole tile
        w.zf = (W < (1u << 28) && (uint64_t)G + W + (2ull << 24) < (1ull << 31)) ? 1 : 0;
    }
    w.qb[0] = rb0 & ~3;
    w.qe[0] = re0 <= rb0 ? 0 : (re0 + 3) & ~3;
    w.qb[1] = rb1 & ~3;
    w.qe[1] = re1 <= rb1 ? 0 : (re1 + 3) & ~3;
    const int m = re0 > rb0 ? re0 : rb0, behind0 = (m + 3) & ~3;     // never visit a quad twice
    if (w.qb[1] < behind0) w.qb[1] = behind0;
    return w;
}

// One step's record, 16 bytes: x = qb0 | qe0 << 16, y = qb1 | qe1 << 16, z = s_first | s_last << 8 | flags << 16,
// w = 0 (pads the record to one 16-byte scalar load).  A dead step (both ranges empty) is all zero.
constexpr uint32_t TILE_PLAN_ZF = 1u, TILE_PLAN_MZ0 = 2u, TILE_PLAN_MZ1 = 4u, TILE_PLAN_LIVE = 8u;

struct TilePlanRecord {
    uint32_t x, y, z, w;
};

AMOF_TILE_PLAN_HD inline bool tile_plan_live(const TileWindow &w) { return w.qe[0] > w.qb[0] || w.qe[1] > w.qb[1]; }

AMOF_TILE_PLAN_HD inline TilePlanRecord tile_plan_pack(const TileWindow &w, uint32_t s_first, uint32_t s_last)
{
    TilePlanRecord r = {0u, 0u, 0u, 0u};
    if (!tile_plan_live(w)) return r;
    const bool p0 = w.qe[0] > w.qb[0], p1 = w.qe[1] > w.qb[1];
    r.x = p0 ? (uint32_t)w.qb[0] | (uint32_t)w.qe[0] << 16 : 0u;
    r.y = p1 ? (uint32_t)w.qb[1] | (uint32_t)w.qe[1] << 16 : 0u;
    r.z = (s_first & 255u) | (s_last & 255u) << 8 |
          ((w.zf ? TILE_PLAN_ZF : 0u) | (w.mz[0] ? TILE_PLAN_MZ0 : 0u) | (w.mz[1] ? TILE_PLAN_MZ1 : 0u) | TILE_PLAN_LIVE) << 16;
    return r;
}

}  // namespace amof
