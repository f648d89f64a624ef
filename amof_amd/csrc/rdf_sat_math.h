// The saturating tail of the planned f32-slab slice of the RDF tile kernel (rdf.hip: fast_bin<SAT>, rdf_tile_slice<AHEAD, 1, true>),
// as functions the kernel and the CPU test suite share (tests/native/tile_sat_driver.cpp compiles this file with g++).
//
// The tail without it clamps every candidate q~ to [1/4, clampv] with one v_med3_f32 (clampv = nbins + 1/2 + lane mod 32: a
// lane's own trash word behind the histogram) and centres the edge test with a v_add_f32.  Here the squared sum is formed in
// units of C^2, C = the lane's clampv, so that the VOP3 clamp bit of the last fma -- free -- IS the upper clamp:
//     t  = sat(dz'^2 + y2 c4 + x2 c3)          c3 = sx^2 / C^2, c4 = sy^2 / C^2, dz' = (z_j - z_i) / C,  sat = clamp to [0, 1]
//     Q  = v_sqrt_f32(t)                        in [0, 1]
//     q' = Q C + (1 + g)                        = q~ + g + 1, g = the candidate's error bound g_f (fast_guard_zf_sat + g_m)
// q' >= 1, so the address conversion of bin_count never sees a sum below 2^23 and needs no lower clamp: the counter of a pair
// is word floor(q') = floor(q~ + g) + 1 -- the histogram sits one word up, LDS word 0 is a pad -- and the pair is certainly in
// bin floor(q~ + g) unless fract(q') < 2 g (the edge test of the tail without SAT, moved by g).  A saturated pair (out of range,
// or dead: an infinite term) has q' = C + 1 + g: its lane's trash word, fractional part 1/2 + g, never flagged.
// No NaN reaches the clamp (where DX10_CLAMP would turn it into 0, a count in bin 0): the only infinities are the slab
// coordinates of centres that do not exist, -inf after the scaling by 1 / C > 0 (no 0 * inf: the scale is finite and positive),
// added to a finite product (no inf - inf: partners' coordinates are finite), squared to +inf and added to a finite, non-negative
// sum; every other operand is a converted integer or a finite positive constant.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AMOF_SAT_FN __host__ __device__ __forceinline__
#else
#define AMOF_SAT_FN inline
#endif

namespace amof {

// per-lane constants: made once per work item, and again wherever the cell's constants are re-read
struct SatLane {
    float C;            // nbins + 1/2 + (lane mod 32): exact in f32
    float invC;         // fl(1 / C), the f64 quotient rounded once
    float c3, c4;       // fl(sx^2 / C^2), fl(sy^2 / C^2) from the f64 scales: one rounding each, like sc[3], sc[4]
};

AMOF_SAT_FN SatLane sat_lane(int nbins, int lane, double sx, double sy)
{
    SatLane s;
    s.C = (float)nbins + 0.5f + (float)(lane & 31);
    const double ic = 1.0 / (double)s.C, ic2 = ic * ic;
    s.invC = (float)ic;
    s.c3 = (float)(sx * sx * ic2);
    s.c4 = (float)(sy * sy * ic2);
    return s;
}

AMOF_SAT_FN uint32_t sat_bits(float v)
{
    uint32_t b;
    __builtin_memcpy(&b, &v, sizeof b);
    return b;
}

// a centre's slab coordinate (bins, f32) as the addend of sat_dz: -z_i / C, one rounding (+inf, no such centre, becomes -inf)
AMOF_SAT_FN float sat_centre(float zi, float invC) { return -(zi * invC); }

// dz' = (z_j - z_i) / C: one fma, one rounding
AMOF_SAT_FN float sat_dz(float zj, float invC, float nzi) { return fmaf(zj, invC, nzi); }

// the saturated squared sum in units of C^2
AMOF_SAT_FN float sat_t(int ix, int iy, float dzs, float c3, float c4)
{
    const float fx = (float)ix, fy = (float)iy;
    const float x2 = fx * fx, y2 = fy * fy;
    const float t = fmaf(dzs, dzs, fmaf(y2, c4, x2 * c3));
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fmed3f(t, 0.0f, 1.0f);     // (the compiler folds this into the fma's clamp bit)
#else
    return t > 1.0f ? 1.0f : t;                        // (t >= 0, never NaN: see the top of this file)
#endif
}

// q' from the root Q of sat_t
AMOF_SAT_FN float sat_candidate(float Q, float C, float one_p_guard) { return fmaf(Q, C, one_p_guard); }

// byte offset of the counter of q' (bin_count's conversion, rdf.hip): 4 floor(q') for 1 <= q' < 2^20
AMOF_SAT_FN uint32_t sat_offset(float qp) { return sat_bits(fmaf(qp, 4.0f, 8388607.5f)) & 0x007ffffcu; }

// needs refinement: within the guard of a bin edge
AMOF_SAT_FN bool sat_unsafe(float qp, float two_guard)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_fractf(qp) < two_guard;
#else
    return qp - floorf(qp) < two_guard;                // (exact: the fraction's bits are bits of q')
#endif
}

}  // namespace amof
