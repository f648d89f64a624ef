// Fragments of one frame's bond graph under periodic boundaries: the per-bond image, the relabelling step, the winding relation
// and the centre-of-mass arithmetic that both GPU kernels (fragment.hip: "fragment_frame", "fragment_global") and the CPU driver
// (tests/native/fragment_driver.cpp) compile.  Plain pointers, no HIP types.  Definition: DESIGN.md 4.3g, include/amof_hip.h
// (amof_fragment_stats).
//
//   g [24] f64                     a geometry record (amof_internal.h): cell rows [0..8], inverse with the columns of open axes
//                                  zeroed [9..17]
//   adj [N][FRAG_MAX_DEGREE] int32 neighbour rows (ring.hip, ring_adjacency_kernel), deg [N]
//   img [N][FRAG_MAX_DEGREE] u32   per row entry the lattice vector n_ij that pair_base subtracts for r_j - r_i, three int8
//   Rec                            the state of an atom: label (u16: N <= 65535) and shift (3 x i16), 8 bytes
//
// Image.  pair_image evaluates the rint() of pair_base<ORTHO> (amof_internal.h) on the same operands in the same order: n_ij.
// The image of j bonded to i is r_j - n_ij C, so with shifts  shift[j] = shift[i] - n_ij,  and, read from i's row,
//   shift[i] = shift[j] + n_ij            (n_ji == -n_ij exactly: negation commutes with *, fma and rint).
// Relabelling (Jacobi: every atom reads the records of the previous round).  An atom adopts (label, shift + n_ij) from the
// neighbour with the smallest label of its row -- the first such entry where several carry it -- iff that label is below its own.
// A label only falls, so N rounds bound the loop; the labels of a fragment become its smallest atom index in as many rounds as
// that atom's eccentricity, and the shifts then are those along a shortest path from it.
// Winding.  Bond (i, j) HOLDS iff shift[i] == shift[j] + n_ij; a fragment winds iff one of its bonds does not.
//
// Centre of mass, order-independent: every atom adds two int64 words per component.  With x_i = r_i + shift[i] C (whole_coord:
// three fma) and t = m_i x_ic 2^8 (the scaling is exact):  hi = rint(t),  lo = llrint((t - hi) 2^32)  (t - hi is exact), i.e. the
// product at scale 2^FRAG_SCALE_BITS = 2^40 per u A split at bit 32.  Accepted inputs: 0 < m_i < FRAG_MASS_MAX = 2^9 u, |x_ic| <
// FRAG_COORD_MAX = 2^16 A (refused otherwise, naming the frame), N <= 65535 < 2^16.  Range: |hi| <= 2^33 and |lo| <= 2^31 per
// atom, the sums of a fragment below 2^49 and 2^47: no overflow for any accepted input, and both convert to f64 exactly.
// Error of a centre component of a fragment of n atoms and mass M, with mmax its largest mass and X the largest
// |r_ic| + sum_k |shift[i]_k C_kc| of its atoms (the magnitudes whole_coord passes through):
//   rounding lo                 n 2^-41            u A     (half a unit of 2^-40 per atom)
//   the product m x in f64      n mmax X 2^-53     u A     (one rounding each)
//   x_i itself                  3 X 2^-53            A     (three fma)
//   hi + lo 2^-32, / M          2 X 2^-53            A     (one rounding each; / 2^8 is exact)
// so  |centre - exact| <= n (2^-41 + mmax X 2^-53) / M + 5 X 2^-53 A  (frag::centre_bound); with X < 2^16 and mmax < 2^9 at most
// n 3.8e-9 / M + 3.7e-11 A, and 1.1e-13 A for an imidazolate within 64 A of the origin.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define FRAG_HD __host__ __device__ __forceinline__
#else
#define FRAG_HD inline
#endif

#define FRAG_MAX_DEGREE 16
#define FRAG_MAX_ATOMS 65535
#define FRAG_SCALE_BITS 40
#define FRAG_COORD_MAX 65536.0
#define FRAG_MASS_MAX 512.0
#define FRAG_IMAGE_MAX 127
#define FRAG_SHIFT_MAX 32767

namespace frag {

struct alignas(8) Rec {
    uint16_t label;
    int16_t s[3];
};

// the lattice vector pair_base subtracts for the raw difference d0 = r_j - r_i (the same products, fma order and rint)
FRAG_HD void pair_image(const double *g, bool ortho, double d0x, double d0y, double d0z, double n[3])
{
    if (ortho) {
        n[0] = rint(d0x * g[9]);
        n[1] = rint(d0y * g[13]);
        n[2] = rint(d0z * g[17]);
    } else {
        const double s0 = fma(d0z, g[15], fma(d0y, g[12], d0x * g[9]));
        const double s1 = fma(d0z, g[16], fma(d0y, g[13], d0x * g[10]));
        const double s2 = fma(d0z, g[17], fma(d0y, g[14], d0x * g[11]));
        n[0] = rint(s0);
        n[1] = rint(s1);
        n[2] = rint(s2);
    }
}

// three int8 in a word; false: a component beyond FRAG_IMAGE_MAX (or not a number)
FRAG_HD bool pack_image(const double n[3], uint32_t *out)
{
    uint32_t w = 0;
    for (int c = 0; c < 3; c++) {
        if (!(fabs(n[c]) <= (double)FRAG_IMAGE_MAX)) return false;
        w |= ((uint32_t)(int32_t)n[c] & 0xffu) << (8 * c);
    }
    *out = w;
    return true;
}
FRAG_HD int image_component(uint32_t w, int c) { return (int)(int8_t)((w >> (8 * c)) & 0xffu); }

// One round for atom i.  cur: the records of the previous round.  Returns the record of this round; *changed is set when it
// differs, *overflow when an adopted shift does not fit an i16 (the record then keeps the old shift: the call is refused).
FRAG_HD Rec relabel(const Rec *cur, const int32_t *row, const uint32_t *img, int deg, int i, bool *changed, bool *overflow)
{
    Rec r = cur[i];
    int best = r.label, bq = -1;
    for (int q = 0; q < deg; q++) {
        const int l = cur[row[q]].label;
        if (l < best) {
            best = l;
            bq = q;
        }
    }
    if (bq < 0) return r;
    const Rec from = cur[row[bq]];
    int s[3];
    bool fits = true;
    for (int c = 0; c < 3; c++) {
        s[c] = (int)from.s[c] + image_component(img[bq], c);
        if (s[c] > FRAG_SHIFT_MAX || s[c] < -FRAG_SHIFT_MAX) fits = false;
    }
    *changed = true;
    r.label = (uint16_t)best;
    if (!fits) {
        *overflow = true;
        return r;
    }
    for (int c = 0; c < 3; c++) r.s[c] = (int16_t)s[c];
    return r;
}

// the relation of a bond read from i's row: shift[i] == shift[j] + n_ij
FRAG_HD bool bond_holds(const Rec &ri, const Rec &rj, uint32_t img)
{
    for (int c = 0; c < 3; c++)
        if ((int)ri.s[c] != (int)rj.s[c] + image_component(img, c)) return false;
    return true;
}

// r + shift C
FRAG_HD void whole_coord(const double *g, const double *p, const int16_t s[3], double x[3])
{
    for (int c = 0; c < 3; c++) x[c] = fma((double)s[2], g[6 + c], fma((double)s[1], g[3 + c], fma((double)s[0], g[c], p[c])));
}

// an atom's term of the fixed-point sums, two words; false: outside the accepted range
FRAG_HD bool fixed_term(double m, double x, long long *hi, long long *lo)
{
    if (!(fabs(x) < FRAG_COORD_MAX)) return false;
    const double t = m * x * 256.0;
    const double h = rint(t);
    *hi = (long long)h;
    *lo = llrint((t - h) * 4294967296.0);
    return true;
}

FRAG_HD double centre(long long hi, long long lo, double M) { return (((double)hi + (double)lo * (1.0 / 4294967296.0)) * (1.0 / 256.0)) / M; }

// the error bound above, in A
FRAG_HD double centre_bound(int n, double M, double mmax, double X)
{
    const double u = 1.0 / 9007199254740992.0;      // 2^-53
    return (double)n * (4096.0 * u + mmax * X * u) / M + 5.0 * X * u;
}

}  // namespace frag
