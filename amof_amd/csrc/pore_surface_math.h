// The float32 decision of the surface kernels' fast path (pore_surface.hip, pore_surface_list) and its error bound.  No HIP
// dependency: the CPU test suite compiles it with g++ (tests/native/pore_surface_driver.cpp) -- with -ffp-contract=off, as
// the library.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define AMOF_SURF_HD __host__ __device__
#else
#define AMOF_SURF_HD
#endif

namespace amof {

constexpr int SURF_MAX_DIRS = 4096;         // directions a call may pass (AMOF_EINVAL beyond)
constexpr int SURF_LIST_CAP = 512;          // neighbour records a wave keeps (a fuller list sends the launch to pore_surface_exact)

// A wave owns atom j with sphere radius rho_j = R_j + rp.  A neighbour image is stored once per wave as a = fl32(A),
// A = image - r_j in float64, with rho~ = fl32(rho_k), rho_k = R_k + rp; a sample as p = fl32(P), P = fl(rho_j u_m) in float64.
// Then, in float32,
//     d = a - p (per component),  d2 = fma(dz, dz, fma(dy, dy, dx dx))
// and no root is taken: d2 is compared with the squares of rho~ -+ eps.
AMOF_SURF_HD inline float surf_d2(float ax, float ay, float az, float px, float py, float pz)
{
    const float dx = ax - px, dy = ay - py, dz = az - pz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
// -1: the image buries the sample (|d| < rho_k for certain), +1: it does not (|d| >= rho_k for certain), 0: inside the guard
// band -- the canonical float64 arithmetic decides, from the raw positions
AMOF_SURF_HD inline int surf_decide(float d2, float rho32, float eps32)
{
    const float lo = rho32 - eps32, hi = rho32 + eps32;
    if (lo > 0.0f && d2 < lo * lo) return -1;
    if (d2 > hi * hi) return 1;
    return 0;
}

// Bound eps on | sqrt(d2) - rho~  -  (|D| - rho_k) | in Angstrom, D = the canonical float64 vector image - sample, u = 2^-24,
// reach = max_s radii[s] + max_t thresholds[t] >= every rho.  A wave keeps an image only if |A| < rho_j + rho_k (with a margin
// far below 1 %), so |A| < 2.02 reach, |P| = rho_j <= reach and |A - P| < 3.02 reach <= Q := 3.1 reach.
//   components  |a - A| <= u |A|, |p - P| <= u |P|, the subtraction u |d|: as vectors <= u (|A| + |P| + |d|) <= 2 u Q
//   d2          three roundings of a sum of non-negative terms: relative 3u, 1.5 u Q on the root
//   radius      |rho~ - rho_k| <= u reach <= u Q / 3; the sum rho~ -+ eps another u Q / 3
//   square      of that sum, one rounding: relative u, 0.5 u on the root, <= u Q / 6
// together (2 + 1.5 + 5/6) u Q = 4.34 u Q; 6 u Q is taken, and 10 % margin on top.  eps32 is this bound as a float rounded
// up (surf_eps32): the band only widens.
// The positions behind A are the fixed-point records of the cell sort, of both atoms: fractional coordinates floored to 2^-32
// after a float64 fold (see pore_math.h); 2^-31 sum_k |a_k| covers the two.  The canonical sample fl(r_j + P) is within
// 2^-53 (|r_j| + reach) of r_j + P, the canonical value within a few 2^-53 of its own exact value: the quantiser refuses atoms
// more than 1e4 cells out, so both stay below 1e-10 sum_k |a_k|, which is added.
inline double pore_surface_bound(const double cell[9], double reach)
{
    const double u = 1.0 / 16777216.0;
    double asum = 0.0;
    for (int k = 0; k < 3; k++) asum += sqrt(cell[3 * k] * cell[3 * k] + cell[3 * k + 1] * cell[3 * k + 1] + cell[3 * k + 2] * cell[3 * k + 2]);
    const double Q = 3.1 * reach;
    return 1.1 * 6.0 * u * Q + asum / 2147483648.0 + 1e-10 * asum;
}
inline float surf_eps32(double bound)
{
    return (float)bound * (1.0f + 2.4e-7f);
}

}  // namespace amof
