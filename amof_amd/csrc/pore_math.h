// Candidate arithmetic and error bound of the pore kernels' fast path (pore.hip, pore_brick).  No HIP dependency: the CPU
// test suite compiles it with g++ (tests/native/pore_candidate_driver.cpp) -- with -ffp-contract=off, as the library.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define AMOF_PORE_HD __host__ __device__
#else
#define AMOF_PORE_HD
#endif

namespace amof {

constexpr int PORE_BRICK = 8;                   // grid points per brick edge
constexpr double PORE_HALF_DIAG_MAX = 1.5;      // the fast path applies while the brick's half-diagonal <= 1.5 rcut

// The candidate of one (grid point, atom image) pair.  A workgroup owns a brick of grid points with centre c.  An atom image
// is stored once per brick as a = fl32(A), A = image - c in float64, with R~ = fl32(R); a grid point as p = fl32(P),
// P = point - c.  Then, in float32,
//     d  = a - p (per component),  d2 = fma(dz, dz, fma(dy, dy, dx dx)),  cand = sqrt(d2) - R~
// The sweep needs no root per atom: it compares d2 with the square of (running minimum + R~) and takes the root only where
// the minimum moves (pore_cand_d2 / pore_cand).
AMOF_PORE_HD inline float pore_cand_d2(float ax, float ay, float az, float px, float py, float pz)
{
    const float dx = ax - px, dy = ay - py, dz = az - pz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
AMOF_PORE_HD inline float pore_cand(float d2, float r32)
{
    return sqrtf(d2) - r32;
}

// first sweep: could this atom lower the running candidate minimum m?  (m + R~ < 0 passes spuriously: a root for nothing)
AMOF_PORE_HD inline bool pore_could_lower(float d2, float m, float r32)
{
    const float t = m + r32;
    return d2 < t * t;
}
// second sweep: is the atom's candidate within 2 eps_c' of the candidate minimum m?  me = fl(m + 2 eps_c), eps_c' = 7.06 u Q
// and eps_c = pore_candidate_bound below.  cand <= m + 2 eps_c' implies sqrt(d2) <= m + 2 eps_c' + R~ + 2.6 u Q (the
// candidate's last subtraction and its root undone), and T with its two roundings (<= 2 u Q) is at least that because
// 2 eps_c >= 2 eps_c' + 5.8 u Q; the factor covers the rounding of the square.  A superset is harmless: what is selected
// is re-evaluated in float64.
AMOF_PORE_HD inline bool pore_selected(float d2, float me, float r32)
{
    const float T = me + r32;
    return T >= 0.0f && d2 <= T * T * (1.0f + 9.6e-7f);
}

// Bound eps_c on |cand - v| in Angstrom, v = sqrt(d2) - R of the canonical float64 arithmetic, u = 2^-24.
// A brick keeps an image only if |A| - R < dmax + hd (hd = the brick's half-diagonal >= |P|), so |A| < rcut + hd and
// |A - P| < rcut + 2 hd <= Q := (1 + 2 PORE_HALF_DIAG_MAX) rcut = 4 rcut.
//   components  |a - A| <= u |A|, |p - P| <= u |P|, the subtraction u |d|: as vectors <= u (|A| + |P| + |d|) <= 2 u Q
//   d2          three roundings of a sum of non-negative terms: relative 3u, 1.5u on the root
//   root        v_sqrt_f32 on gfx950 is within 1.56u relative (profiles/tools/sqrt_ulp.hip); correctly rounded elsewhere
//   radius      |R~ - R| <= u R <= u Q; the final subtraction u |cand| <= u Q
// together (2 + 3.06 + 1 + 1) u Q = 7.06 u Q.  The second sweep selects by comparing d2 with a rounded square of a rounded
// sum (2.6 u Q more: see pore_brick_kernel); 10 u Q is taken, and 10 % margin on top.
// The positions behind A are the fixed-point records: fractional coordinates floored to 2^-32 (<= 2^-32 sum_k |a_k| in
// Cartesian terms) after a float64 fold of coordinates up to 1e4 cells away (the quantiser refuses more: <= 1e4 2^-50 of
// a cell), against the canonical vector's own rounding at that distance; 2^-31 sum_k |a_k| covers the three.
inline double pore_candidate_bound(const double cell[9], double rcut)
{
    const double u = 1.0 / 16777216.0;
    double asum = 0.0;
    for (int k = 0; k < 3; k++) asum += sqrt(cell[3 * k] * cell[3 * k] + cell[3 * k + 1] * cell[3 * k + 1] + cell[3 * k + 2] * cell[3 * k + 2]);
    const double Q = (1.0 + 2.0 * PORE_HALF_DIAG_MAX) * rcut;
    return 1.1 * 10.0 * u * Q + asum / 2147483648.0;
}

// half-diagonal of a full brick of a grid n over the cell: the largest |+-e_x a +- e_y b +- e_z c|, e_k = (PORE_BRICK - 1) / (2 n_k)
inline double pore_brick_half_diag(const double cell[9], const int n[3])
{
    double best = 0.0;
    for (int s = 0; s < 4; s++) {
        const double e[3] = {0.5 * (PORE_BRICK - 1) / n[0], (s & 1 ? -0.5 : 0.5) * (PORE_BRICK - 1) / n[1],
                             (s & 2 ? -0.5 : 0.5) * (PORE_BRICK - 1) / n[2]};
        double q = 0.0;
        for (int c = 0; c < 3; c++) {
            const double x = e[0] * cell[c] + e[1] * cell[3 + c] + e[2] * cell[6 + c];
            q += x * x;
        }
        best = q > best ? q : best;
    }
    return sqrt(best) * (1.0 + 1e-12);
}

}  // namespace amof
