// The argument rules of the Pore family (amof_pore_field, amof_pore_access[_field], amof_pore_psd[_field], amof_pore_surface), each
// once, host-only C++17 without HIP or amof_ctx (tests/native/pore_check_driver.cpp and pore_surface_driver.cpp ask them directly).  A rule returns the AMOF_E* code and
// the message; the .hip files pass both on to fail() (pore_refuse, amof_internal.h) and decide none of this themselves.
// The order of the checks per entry point (the first refusal wins; F = n_frames):
//   amof_pore_field         validate_traj . both_given(radii, grid) . thresholds_given . field_outputs . grid . bin_width . radii . thresholds_finite .
//                           counter_words . [F == 0: done] . build_geometry . half_height_atoms . per_point_cap(field)
//   amof_pore_access        both_given(traj, grid) . LABELLING = grid(with pbc) . thresholds_given . thresholds_finite . access_outputs . labels_cap .
//                           then amof_pore_field's
//   amof_pore_access_field  given_field_inputs . LABELLING . [F == 0: done] . field_finite
//   amof_pore_psd           both_given(traj, grid) . COVERING = thresholds_given . bin_width . thresholds_finite . counter_words . grid .
//                           psd_outputs . per_point_cap(cover) . po_access_given . then LABELLING (want_access or want_free) . amof_pore_field's
//   amof_pore_psd_field     given_field_inputs(with cells) . COVERING . po_access_given . [F == 0: done] . per frame: singular
//                           cell (pore_cover.hip has the step geometry), field_finite, half_height_field . want_access: grid(with pbc)
//   amof_pore_surface       both_given(traj, grid) . SURFACE = direction_count . both_given(dirs, dirs) . directions . thresholds_given .
//                           thresholds_finite . probes_not_negative . surface_outputs . samples_cap . then COVERING (want_psd) .
//                           LABELLING (want_access or want_free) . amof_pore_field's . half_height_surface
#pragma once
#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/amof_hip.h"

namespace amof {
namespace pore_check {
struct Verdict {
    int code = AMOF_OK;
    char text[320] = "";
};
__attribute__((format(printf, 3, 4))) inline Verdict refuse_if(bool bad, int code, const char *fmt, ...)
{
    Verdict v;
    if (!bad) return v;
    v.code = code;
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(v.text, sizeof v.text, fmt, ap);
    va_end(ap);
    return v;
}
inline Verdict null_if(bool missing) { return refuse_if(missing, AMOF_EINVAL, "NULL argument"); }
// ---- NULL arguments (P: a pointer as the caller gave it) ---------------------------------------------------------------
typedef const void *P;
inline Verdict both_given(P a, P b) { return null_if(!a || !b); }
inline Verdict thresholds_given(P thresholds, int32_t n_t) { return null_if(n_t < 0 || (n_t > 0 && !thresholds)); }
inline Verdict field_outputs(int64_t F, int32_t n_t, P hist, P counts, P vmax, P argmax) { return null_if(F > 0 && (!hist || !vmax || !argmax || (n_t > 0 && !counts))); }
inline Verdict given_field_inputs(P grid, P pbc, int64_t F, P field, bool needs_cells, P cells) { return null_if(!grid || !pbc || F < 0 || (F > 0 && (!field || (needs_cells && !cells)))); }
inline Verdict access_outputs(int64_t F, int32_t n_t, int32_t want_free, P access, P free_sphere)
{
    if (F > 0 && n_t > 0 && !access) return null_if(true);
    return refuse_if(F > 0 && want_free && !free_sphere, AMOF_EINVAL, "want_free without a free_sphere array");
}
inline Verdict psd_outputs(int64_t F, int32_t n_t, P psd_hist, P po_counts) { return null_if(F > 0 && (!psd_hist || (n_t > 0 && !po_counts))); }
inline Verdict po_access_given(int64_t F, int32_t n_t, int32_t want_access, P po_access)
{
    return refuse_if(F > 0 && n_t > 0 && want_access && !po_access, AMOF_EINVAL, "want_access without a po_access array");
}
// ---- the grid: 1 x 1 x 1 to 2^31 - 1 points (nx ny alone within that, too); label_pbc (labelling only, or null): a periodic
// axis needs 3 points
inline Verdict grid(const int32_t *grid, const int32_t *label_pbc)
{
    for (int k = 0; k < 3; k++) {
        if (grid[k] < 1) return refuse_if(true, AMOF_EINVAL, "grid must be at least 1 x 1 x 1");
        if (label_pbc && label_pbc[k] && grid[k] < 3)
            return refuse_if(true, AMOF_EINVAL, "periodic axis %d has %d grid points: a point would meet itself or one neighbour through both "
                                                "faces, labelling needs 3", k, grid[k]);
    }
    return refuse_if((int64_t)grid[0] * grid[1] > 0x7fffffffLL || (int64_t)grid[0] * grid[1] * (int64_t)grid[2] > 0x7fffffffLL, AMOF_EINVAL,
                     "the grid has more than 2^31 - 1 points");
}
// ---- histogram and counters: nb = rint(dmax / dr), at least one bin; nbins + 2 + n_t counters per frame
inline Verdict bin_width(double dr, double dmax, double &nb)
{
    if (!(dr > 0.0) || !isfinite(dr) || !(dmax > 0.0) || !isfinite(dmax)) return refuse_if(true, AMOF_EINVAL, "dr and dmax must be finite and > 0");
    nb = rint(dmax / dr);
    return refuse_if(!(nb >= 1.0), AMOF_EINVAL, "dmax / dr rounds to no bin");
}
inline Verdict counter_words(double nb, int32_t n_t, int32_t &nbins)
{
    const bool over = nb + 2.0 + (double)n_t > (double)AMOF_PORE_MAX_WORDS;
    if (!over) nbins = (int32_t)nb;
    return refuse_if(over, AMOF_ECAPACITY, "nbins + 2 + n_thresholds exceeds %d", AMOF_PORE_MAX_WORDS);
}
// ---- values: rmax = the largest radius; top = the largest value of a supplied field (-inf of none)
inline Verdict radii(const double *radii, int n_species, double &rmax)
{
    rmax = 0.0;
    for (int s = 0; s < n_species; s++) {
        if (!(radii[s] >= 0.0) || !isfinite(radii[s])) return refuse_if(true, AMOF_EINVAL, "radii must be finite and >= 0");
        rmax = radii[s] > rmax ? radii[s] : rmax;
    }
    return Verdict();
}
inline Verdict thresholds_finite(const double *thresholds, int32_t n_t)
{
    bool finite = true;
    for (int k = 0; k < n_t; k++) finite = finite && isfinite(thresholds[k]);
    return refuse_if(!finite, AMOF_EINVAL, "thresholds must be finite");
}
inline Verdict field_finite(const double *field, size_t n, double &top)
{
    top = -INFINITY;
    for (size_t x = 0; x < n; x++) {
        if (!isfinite(field[x])) return refuse_if(true, AMOF_EINVAL, "the field must be finite");
        top = field[x] > top ? field[x] : top;
    }
    return Verdict();
}
// ---- one image at most.  hmin: the smallest perpendicular height over the periodic axes (+inf without one).  1e-12: the
// heights come out of an inverse; a cutoff of exactly half a height, as Pore's default dmax can be, passes.
inline bool above_half_height(double reach, double hmin) { return reach > 0.5 * hmin * (1.0 + 1e-12); }
inline Verdict half_height_atoms(double dmax, double rmax, double hmin)
{
    return refuse_if(above_half_height(dmax + rmax, hmin), AMOF_EINVAL, "dmax + the largest radius = %g exceeds half the smallest cell height "
                                                                        "%g: one minimum image would not do", dmax + rmax, hmin);
}
inline Verdict half_height_field(double top, int64_t frame, double hmin)
{
    return refuse_if(above_half_height(top, hmin), AMOF_EINVAL, "the largest field value %g of frame %lld exceeds half the smallest periodic "
                                                                "cell height %g: a sphere would reach a point through two images", top,
                     (long long)frame, hmin);
}
// ---- what one frame may take: 4 GiB.  what: "field" (amof_pore_field's) or "array" (the covering radius)
inline Verdict per_point_cap(int64_t G, const char *what)
{
    return refuse_if((size_t)G * sizeof(double) > ((size_t)1 << 32), AMOF_ECAPACITY, "a per-point %s of %lld points per frame exceeds the 4 GiB a "
                                                                                     "frame may take", what, (long long)G);
}
inline Verdict labels_cap(int32_t n_t, int64_t G)
{
    return refuse_if((size_t)n_t * (size_t)G * sizeof(int32_t) > ((size_t)1 << 32), AMOF_ECAPACITY,
                     "labels of %d thresholds x %lld points exceed the 4 GiB a frame may take", n_t, (long long)G);
}
// ---- the surface stage (amof_pore_surface): directions [M][3], 1 <= M <= 4096, unit vectors to 1e-12 in |u|^2; probe radii >= 0
inline Verdict direction_count(int32_t n_dirs) { return refuse_if(n_dirs < 1 || n_dirs > 4096, AMOF_EINVAL, "n_dirs = %d: 1 .. 4096 directions", n_dirs); }
inline Verdict directions(const double *dirs, int32_t n_dirs)
{
    for (int m = 0; m < n_dirs; m++) {
        const double *u = dirs + 3 * (size_t)m;
        const double q = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
        if (!(fabs(q - 1.0) <= 1e-12)) return refuse_if(true, AMOF_EINVAL, "direction %d is no unit vector: |u|^2 - 1 = %g", m, q - 1.0);
    }
    return Verdict();
}
inline Verdict probes_not_negative(const double *thresholds, int32_t n_t)
{
    for (int k = 0; k < n_t; k++)
        if (!(thresholds[k] >= 0.0)) return refuse_if(true, AMOF_EINVAL, "threshold %d = %g: the surface stage takes probe radii >= 0", k, thresholds[k]);
    return Verdict();
}
inline Verdict surface_outputs(int64_t F, int32_t n_t, int32_t want_access, P exposed, P exposed_access)
{
    if (F > 0 && n_t > 0 && !exposed) return null_if(true);
    return refuse_if(F > 0 && n_t > 0 && want_access && !exposed_access, AMOF_EINVAL, "want_access without an exposed_access array");
}
// the largest sample sphere: no other image of an atom may come closer to its own samples than the sphere's radius
inline Verdict half_height_surface(double rmax, double tmax, double hmin)
{
    return refuse_if(above_half_height(rmax + tmax, hmin), AMOF_EINVAL, "the largest radius + the largest probe radius = %g exceeds half the "
                                                                        "smallest cell height %g: a sample sphere would meet its own image",
                     rmax + tmax, hmin);
}
inline Verdict samples_cap(int32_t n_t, int64_t n_atoms, int32_t n_dirs)
{
    return refuse_if((double)n_t * (double)n_atoms * (double)n_dirs > 4294967296.0, AMOF_ECAPACITY,
                     "samples of %d thresholds x %lld atoms x %d directions exceed the 4 GiB a frame may take", n_t, (long long)n_atoms, n_dirs);
}
}  // namespace pore_check
}  // namespace amof
