// Dihedral (torsion) angle of a chain a-b-c-d of bonded atoms: the arithmetic and the pattern match that both GPU kernels
// (dihedral.hip: "dihedral_frame", "dihedral_exact") and the CPU driver (tests/native/dihedral_driver.cpp) compile.  Plain scalars
// and pointers, no HIP types; -ffp-contract=off everywhere.  Definition: include/amof_hip.h (amof_dihedral_hist), DESIGN.md 4.3.
//
// Chain.  An unordered central bond {b, c}, a neighbour a of b and a neighbour d of c with a != c, d != b and a != d by atom
// index; visited once, from the end with b < c.  The unit vectors are the canonical ones of the neighbour rows:
// u1 = u(b -> a), u2 = u(b -> c), u3 = u(c -> d).
// Angle, in float64, every product and sum rounded on its own, in this order:
//   n1 = u2 x u1,  n2 = u2 x u3          component x = (u2y * wz) - (u2z * wy), y = (u2z * wx) - (u2x * wz), z = (u2x * wy) - (u2y * wx)
//   s1 = (n1x n1x + n1y n1y) + n1z n1z,  s2 likewise
//   undefined iff s1 < 2^-40 or s2 < 2^-40 (a bond angle within about 1e-6 rad of straight)
//   c = clip(((n1x n2x + n1y n2y) + n1z n2z) / sqrt(s1 * s2), -1, 1),  phi = (180 / pi) * acos_fd(c) in [0, 180]
// n1 and n2 are both normal to u2, so their angle is the angle between the planes (a, b, c) and (b, c, d): 0 = cis, 180 = trans.
// Negating u2 (the chain read from d) negates both normals and changes nothing.
// Pattern.  chains[t] = (A, B, C, D) species indices, -1 = any.  A chain of species (sa, sb, sc, sd) counts ONCE for pattern t
// iff the pattern matches it read as a-b-c-d or as d-c-b-a (chain_mask: bit t).
#pragma once

#include <math.h>
#include <stdint.h>

#include "angle_math.h"

#define DIHEDRAL_MAX_CHAINS 32
#define DIHEDRAL_E 40                       // the cosine of a chain is rounded to 2^-E
#define DIHEDRAL_TABLE_MAX 4096             // S^4 up to here: the masks of every species 4-tuple in a table

namespace amof {
namespace dihedral {

constexpr double UNDEFINED_BELOW = 0x1p-40;

// the clipped cosine of the chain's torsion angle; false: undefined
ANGLE_HD bool chain_cos(double u1x, double u1y, double u1z, double u2x, double u2y, double u2z, double u3x, double u3y, double u3z,
                        double &c)
{
    const double n1x = u2y * u1z - u2z * u1y, n1y = u2z * u1x - u2x * u1z, n1z = u2x * u1y - u2y * u1x;
    const double n2x = u2y * u3z - u2z * u3y, n2y = u2z * u3x - u2x * u3z, n2z = u2x * u3y - u2y * u3x;
    const double s1 = n1x * n1x + n1y * n1y + n1z * n1z;
    const double s2 = n2x * n2x + n2y * n2y + n2z * n2z;
    c = 0.0;
    if (s1 < UNDEFINED_BELOW || s2 < UNDEFINED_BELOW) return false;
    double v = (n1x * n2x + n1y * n2y + n1z * n2z) / sqrt(s1 * s2);
    if (v > 1.0) v = 1.0;
    if (v < -1.0) v = -1.0;
    c = v;
    return true;
}

ANGLE_HD double angle_deg(double c) { return (180.0 / M_PI) * acos_fd(c); }

// what a defined chain adds to the cosine sum of its frame
ANGLE_HD long long cos_term(double c) { return llrint(c * 0x1p40); }

ANGLE_HD bool species_fits(int want, int s) { return want < 0 || want == s; }

// bit t: pattern t counts a chain of species (sa, sb, sc, sd) -- in either reading direction, once
ANGLE_HD uint32_t chain_mask(const int32_t *__restrict__ chains, int n_chains, int sa, int sb, int sc, int sd)
{
    uint32_t m = 0u;
    for (int t = 0; t < n_chains; t++) {
        const int32_t *p = chains + 4 * t;
        const bool fwd = species_fits(p[0], sa) && species_fits(p[1], sb) && species_fits(p[2], sc) && species_fits(p[3], sd);
        const bool rev = species_fits(p[0], sd) && species_fits(p[1], sc) && species_fits(p[2], sb) && species_fits(p[3], sa);
        if (fwd || rev) m |= 1u << t;
    }
    return m;
}

}  // namespace dihedral
}  // namespace amof
