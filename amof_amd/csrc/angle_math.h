// arccos of the angle kernels (nbr.hip: BAD; dihedral.hip) and of the CPU driver tests/native/dihedral_driver.cpp.
// numpy.arccos (what ase.geometry.get_angles calls) is a different routine on different CPUs and the device library's acos a
// third one; they differ in the last place for a few percent of the arguments, which bins an angle that sits on a histogram
// edge (exact lattices) differently.  Every angle here goes through ONE published algorithm instead -- fdlibm's acos:
// (asin(t) - t) / t ~ z P(z) / Q(z), z = t^2, error < 1 ulp -- in operations that are correctly rounded on the device
// (+ - * / sqrt, no contraction: -ffp-contract=off), the same algorithm the CPU oracle evaluates.
#pragma once

#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>

#if defined(__HIPCC__)
#define ANGLE_HD __host__ __device__ __forceinline__
#else
#define ANGLE_HD inline
#endif

namespace amof {

ANGLE_HD double acos_pq(double z)
{
    double p = 3.47933107596021167570e-05;
    p = 7.91534994289814532176e-04 + z * p;
    p = -4.00555345006794114027e-02 + z * p;
    p = 2.01212532134862925881e-01 + z * p;
    p = -3.25565818622400915405e-01 + z * p;
    p = 1.66666666666666657415e-01 + z * p;
    p = z * p;
    double q = 7.70381505559019352791e-02;
    q = -6.88283971605453293030e-01 + z * q;
    q = 2.02094576023350569471e+00 + z * q;
    q = -2.40339491173441421878e+00 + z * q;
    q = 1.0 + z * q;
    return p / q;
}

// x with the low 32 bits of its significand cleared
ANGLE_HD double acos_high_word(double x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __longlong_as_double(__double_as_longlong(x) & (long long)0xffffffff00000000ull);
#else
    uint64_t w;
    memcpy(&w, &x, sizeof w);
    w &= 0xffffffff00000000ull;
    memcpy(&x, &w, sizeof w);
    return x;
#endif
}

ANGLE_HD double acos_fd(double x)
{
    constexpr double HALF_PI_HEAD = 1.57079632679489655800e+00, HALF_PI_TAIL = 6.12323399573676603587e-17;
    constexpr double PI_HEAD = 3.14159265358979311600e+00;
    const double mag = fabs(x);
    if (mag >= 1.0) return x > 0.0 ? 0.0 : PI_HEAD + 2.0 * HALF_PI_TAIL;      // (the callers clip to [-1, 1])
    if (mag < 0.5) {
        if (mag < 0x1p-57) return HALF_PI_HEAD + HALF_PI_TAIL;
        const double t = x * acos_pq(x * x);
        return HALF_PI_HEAD - (x - (HALF_PI_TAIL - t));
    }
    if (x < 0.0) {
        const double z = (1.0 + x) * 0.5, root = sqrt(z);
        const double corr = acos_pq(z) * root - HALF_PI_TAIL;
        return PI_HEAD - 2.0 * (root + corr);
    }
    const double z = (1.0 - x) * 0.5, root = sqrt(z);
    const double head = acos_high_word(root);
    const double tail = (z - head * head) / (root + head);
    const double corr = acos_pq(z) * root + tail;
    return 2.0 * (head + corr);
}

// numpy.histogram with explicit edges: bin k holds edges[k] <= x < edges[k+1], the last bin is right-closed; outside -> -1.
// (e0, en = first / last edge, inv_w = nb / (en - e0): the first guess only -- the comparisons with the edges decide)
// step > 0: the host has verified edges[k] == (double)k * step bit for bit (numpy.arange(n) * dtheta, amof/bad.py:143):
// the edges are then recomputed instead of loaded -- two dependent global loads per angle otherwise
ANGLE_HD int hist_bin(const double *__restrict__ edges, int nb, double x, double e0, double en, double inv_w, double step = 0.0)
{
#if !defined(__HIPCC__)
    using std::max;
    using std::min;
#endif
    if (!(x >= e0) || !(x <= en)) return -1;
    int k = (int)((x - e0) * inv_w);
    k = max(0, min(k, nb - 1));
    if (step > 0.0) {
        while (k > 0 && x < (double)k * step) k--;
        while (k < nb - 1 && x >= (double)(k + 1) * step) k++;
        return k;
    }
    while (k > 0 && x < edges[k]) k--;
    while (k < nb - 1 && x >= edges[k + 1]) k++;
    return k;
}

}  // namespace amof
