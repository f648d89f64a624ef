// The saturating tail of the planned f32-slab slice (amof_amd/csrc/rdf_sat_math.h, the functions the kernel itself runs) against
// the exact f64 distance of the same fixed-point differences, for tests/test_tile_sat_cpu.py.
// One request per line on stdin:  nbins sx sy sz gfrac guard_m samples seed
//   sx, sy, sz  bins per 2^-32 of the in-plane axes and of the slab axis (FrameScale::sc64[0..2]); gfrac: the culling reach as
//   a share of the slab axis; guard_m: the grid term of the guard (bins)
// One line on stdout per request:
//   pairs  in_range  flagged  saturated  bad_bound  bad_word  bad_trash  bad_lds  max_ratio  bound  guard
// bad_bound: |q' - (q + 1 + g)| > fast_guard_zf_sat for a pair with q <= nbins + 1 that did not saturate
// bad_word:  an unflagged pair whose counter is not word floor(q) + 1 (q < nbins), or that is out of range and counted below
//            word nbins + 1, or in range and counted at or above it
// bad_trash: a saturated pair not in its lane's trash word nbins + 1 + lane mod 32, or flagged, or with q < nbins + 1/4
// bad_lds:   a counter outside words [1, nbins + 32]
// Every pair is evaluated three times: with sqrtf and with its two neighbours (v_sqrt_f32 is good to one ulp).
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <random>

#include "../../amof_amd/csrc/rdf_select.h"
#include "../../amof_amd/csrc/rdf_sat_math.h"

using namespace amof;

struct Tally {
    long long pairs = 0, in_range = 0, flagged = 0, saturated = 0, bad_bound = 0, bad_word = 0, bad_trash = 0, bad_lds = 0;
    double max_ratio = 0.0;
};

struct Setup {
    int nbins;
    double sx, sy, sz, bound, guard;
    SatThresholds thr;
};

// one pair of one lane: fixed-point differences ix, iy in the plane, slab coordinates zi, zj relative to the sub-tile's z0
static void pair(const Setup &s, int lane, int ix, int iy, long long zi, long long zj, Tally &t)
{
    const SatLane L = sat_lane(s.nbins, lane, s.sx, s.sy);
    // as the kernel converts them: one rounding each (f64 product -> f32)
    const float zif = (float)((double)zi * s.sz), zjf = (float)((double)zj * s.sz);
    const float dzs = sat_dz(zjf, L.invC, sat_centre(zif, L.invC));
    const float tt = sat_t(ix, iy, dzs, L.c3, L.c4);
    const double X = (double)ix * s.sx, Y = (double)iy * s.sy, Z = (double)(zj - zi) * s.sz;
    const double q = sqrt(X * X + Y * Y + Z * Z);
    const float Q0 = sqrtf(tt);
    for (int v = 0; v < 3; v++) {
        float Q = v == 0 ? Q0 : nextafterf(Q0, v == 1 ? 2.0f : -1.0f);
        if (Q > 1.0f) Q = 1.0f;
        if (Q < 0.0f) Q = 0.0f;
        const float qp = sat_candidate(Q, L.C, s.thr.one_p_guard);
        const long long word = sat_offset(qp) >> 2;
        const bool flag = sat_unsafe(qp, s.thr.two_guard);
        t.pairs++;
        if (word < 1 || word > s.nbins + 32) t.bad_lds++;
        if (tt >= 1.0f && v == 0) {
            t.saturated++;
            if (word != s.nbins + 1 + (lane & 31) || flag || q < s.nbins + 0.25) t.bad_trash++;
            continue;
        }
        if (q <= s.nbins + 1.0 && tt < 1.0f) {
            const double ratio = fabs((double)qp - (q + 1.0 + s.guard)) / s.bound;
            if (ratio > t.max_ratio) t.max_ratio = ratio;
            if (ratio > 1.0) t.bad_bound++;
        }
        if (q < s.nbins) t.in_range++;
        if (flag) { t.flagged++; continue; }
        if (q < s.nbins ? word != (long long)floor(q) + 1 : word < s.nbins + 1) t.bad_word++;
    }
}

int main()
{
    Setup s;
    double gfrac, guard_m;
    long long samples;
    unsigned long long seed;
    while (scanf("%d %lf %lf %lf %lf %lf %lld %llu", &s.nbins, &s.sx, &s.sy, &s.sz, &gfrac, &guard_m, &samples, &seed) == 8) {
        const double hb = s.sz * 4294967296.0;
        s.bound = fast_guard_zf_sat(s.nbins, hb, gfrac);
        s.guard = s.bound + guard_m;
        s.thr = sat_thresholds(s.guard);
        Tally t;
        std::mt19937_64 rng(seed);
        std::uniform_real_distribution<double> U(0.0, 1.0);
        // the ZF window: centres within half a sub-tile span (< 2^28) of z0, partners within the reach of that span
        const long long zc = (1ll << 27) + 1, G = (long long)(gfrac * 4294967296.0), zp = G + zc + (1ll << 24);
        auto clip = [](double v) { return (int)std::max(-2147483647.0, std::min(2147483647.0, rint(v))); };
        // ---- random differences: a target q in [0, nbins + 40), a random direction, centres anywhere in their range ----
        for (long long k = 0; k < samples; k++) {
            const double qt = U(rng) < 0.1 ? U(rng) * 2.0 : U(rng) * (s.nbins + 40.0);
            const double cz = 2.0 * U(rng) - 1.0, ph = 6.283185307179586 * U(rng), st = sqrt(1.0 - cz * cz);
            const long long zi = (long long)rint((2.0 * U(rng) - 1.0) * (double)zc);
            long long zj = zi + (long long)rint(qt * cz / s.sz);
            zj = std::max(-zp, std::min(zp, zj));
            pair(s, (int)(rng() & 63), clip(qt * st * cos(ph) / s.sx), clip(qt * st * sin(ph) / s.sy), zi, zj, t);
        }
        // ---- adversarial differences, every lane ----
        for (int lane = 0; lane < 64; lane++) {
            const long long ends[4] = {-zc, zc, 0, zc / 3};
            for (int e = 0; e < 4; e++) {
                const long long zi = ends[e];
                pair(s, lane, 0, 0, zi, zi, t);                                    // coincident atoms
                pair(s, lane, 1, 0, zi, zi, t);                                    // one grid unit apart
                pair(s, lane, 0, 0, zi, zp, t);                                    // the ends of the window, slab axis only
                pair(s, lane, 0, 0, zi, -zp, t);
                pair(s, lane, 2147483647, -2147483647, zi, zp, t);                 // the largest differences
                for (int k = -40; k <= 40; k++) {
                    // q around nbins, around 1 and around the lane's clamp value, along x, y, the slab axis and a diagonal
                    const double around[4] = {(double)s.nbins, 1.0, (double)s.nbins + 0.5 + (lane & 31), 0.0};
                    for (int a = 0; a < 4; a++) {
                        const double qt = fabs(around[a] + k * s.guard * 0.26);
                        pair(s, lane, clip(qt / s.sx), 0, zi, zi, t);
                        pair(s, lane, 0, clip(qt / s.sy), zi, zi, t);
                        pair(s, lane, 0, 0, zi, std::max(-zp, std::min(zp, zi + (long long)rint(qt / s.sz))), t);
                        pair(s, lane, 0, 0, zi, std::max(-zp, std::min(zp, zi - (long long)rint(qt / s.sz))), t);
                        pair(s, lane, clip(qt * 0.6 / s.sx), clip(-qt * 0.48 / s.sy), zi,
                             std::max(-zp, std::min(zp, zi + (long long)rint(qt * 0.64 / s.sz))), t);
                    }
                }
            }
        }
        printf("%lld %lld %lld %lld %lld %lld %lld %lld %.6f %.9g %.9g\n", t.pairs, t.in_range, t.flagged, t.saturated, t.bad_bound,
               t.bad_word, t.bad_trash, t.bad_lds, t.max_ratio, s.bound, s.guard);
    }
    return 0;
}
