// The per-pair arithmetic of amof_lindemann (include/amof_hip.h), for host and device: the chunk order of the moments, the
// index delta, its fixed-point term, the bin rule and the scale.  lindemann.hip's kernels and the stand-alone driver of
// tests/native/lindemann_driver.cpp compile this one text (-ffp-contract=off: the only fused operation is the explicit fma).
//
// A block of B frames, d(f) the pair's distance in block-relative frame f, c = d(0), e(f) = d(f) - c:
//   chunk k covers the frames [64 k, min(64 k + 64, B)); inside it, frames ascending: p1 += e, p2 = fma(e, e, p2), both from 0;
//   S1, S2: the chunk partials added in ascending k, from 0;
//   m1 = S1 / B, mean = c + m1, var = max(0, S2 / B - m1 m1), delta = var == 0 ? 0 : sqrt(var) / mean.
// The order is part of the ABI: whoever walks the frames -- a lane per chunk, a lane per block, the host -- gets the same bits.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define AMOF_LIND_HD __host__ __device__ inline
#else
#define AMOF_LIND_HD inline
#endif

namespace amof {
namespace lindemann {

constexpr int CHUNK = 64;          // frames per chunk
constexpr int SCALE_MAX = 40;      // e_s never exceeds it
constexpr int SCALE_MIN = 20;      // below it the call is refused

AMOF_LIND_HD int chunk_count(int64_t B) { return (int)((B + CHUNK - 1) / CHUNK); }

// the partial (p1, p2) of chunk k of a block of B frames; dist(f): the distance in block-relative frame f
template <typename Dist>
AMOF_LIND_HD void chunk_partial(Dist &&dist, double c, int k, int64_t B, double &p1, double &p2)
{
    const int64_t f0 = (int64_t)k * CHUNK, f1 = f0 + CHUNK < B ? f0 + CHUNK : B;
    double a1 = 0.0, a2 = 0.0;
    for (int64_t f = f0; f < f1; f++) {
        const double e = dist(f) - c;
        a1 += e;
        a2 = fma(e, e, a2);
    }
    p1 = a1;
    p2 = a2;
}

// (S1, S2) of a whole block by the same traversal: the chunks in ascending order, each from zero
template <typename Dist>
AMOF_LIND_HD void block_sums(Dist &&dist, double c, int64_t B, double &S1, double &S2)
{
    const int nk = chunk_count(B);
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < nk; k++) {
        double p1, p2;
        chunk_partial(dist, c, k, B, p1, p2);
        s1 += p1;
        s2 += p2;
    }
    S1 = s1;
    S2 = s2;
}

AMOF_LIND_HD double delta(double c, double S1, double S2, int64_t B)
{
    const double m1 = S1 / (double)B;
    const double mean = c + m1;
    const double q = S2 / (double)B;
    const double mm = m1 * m1;
    const double var = fmax(0.0, q - mm);
    return var == 0.0 ? 0.0 : sqrt(var) / mean;
}

// llrint(delta 2^e): delta <= sqrt(B - 1) and e <= scale_log2(.., B) keep it far inside int64
AMOF_LIND_HD long long fixed_term(double delta, int e) { return llrint(ldexp(delta, e)); }

// min((int)(delta / ddelta), nbins - 1), the quotient compared before the conversion: the last bin takes everything above
AMOF_LIND_HD int bin_of(double delta, double ddelta, int nbins)
{
    const double x = delta / ddelta;
    return x < (double)(nbins - 1) ? (int)x : nbins - 1;
}

// e_s = min(40, 62 - bit_length(n_a n_b ceil(sqrt(B)))): a coefficient of variation of B non-negative numbers is at most
// sqrt(B - 1), so no sum of terms over the n_a n_b pairs leaves int64.  -1: the product itself leaves u64.
inline int scale_log2(int64_t n_a, int64_t n_b, int64_t B)
{
    unsigned long long r = (unsigned long long)sqrt((double)B);
    while (r * r < (unsigned long long)B) r++;
    while (r > 0 && (r - 1) * (r - 1) >= (unsigned long long)B) r--;
    unsigned long long ab = 0, abr = 0;
    if (__builtin_mul_overflow((unsigned long long)n_a, (unsigned long long)n_b, &ab) || __builtin_mul_overflow(ab, r, &abr)) return -1;
    const int bits = abr ? 64 - __builtin_clzll(abr) : 0;
    const int e = 62 - bits;
    return e < SCALE_MAX ? e : SCALE_MAX;
}

// blocks of B frames at stride S in F frames; block b covers [b S, b S + B)
inline int64_t block_count(int64_t F, int64_t B, int64_t S) { return (F - B) / S + 1; }

}  // namespace lindemann
}  // namespace amof
