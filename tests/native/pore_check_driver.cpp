// Answers questions about amof_amd/csrc/pore_check.h on stdin (tests/test_pore_check_cpu.py), one line each; every answer is
// "code <tab> value <tab> message" (value: what the rule computes besides its verdict, 0 where nothing).  Doubles are read with
// %lf: decimal, hexadecimal ("0x1.8p+1"), "nan", "inf".  A pointer argument is a 0 / 1: given or NULL.
//   "grid nx ny nz label p0 p1 p2"      label = 1: the labelling's rule for the periodic axes p
//   "bins dr dmax n_t"                  bin_width, then counter_words -> nbins
//   "radii n r0 .. r(n-1)"              -> the largest radius
//   "thr n t0 .. t(n-1)"
//   "finite n v0 .. v(n-1)"             -> the largest value
//   "hha dmax rmax hmin"                half_height_atoms
//   "hhf top frame hmin"                half_height_field
//   "cap G field|array"                 per_point_cap
//   "labels n_t G"                      labels_cap
//   "null both_given a b" | "null thresholds_given thr n_t" |
//   "null field_outputs F n_t hist counts vmax argmax" | "null given_field_inputs grid pbc F field needs_cells cells" |
//   "null access_outputs F n_t want_free access free" | "null psd_outputs F n_t psd_hist po_counts" |
//   "null po_access_given F n_t want_access po_access"
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../amof_amd/csrc/pore_check.h"

using namespace amof;
using pore_check::Verdict;

static int dummy;
static const void *ptr(long long given) { return given ? &dummy : nullptr; }

static void answer(const Verdict &v, double value) { printf("%d\t%.17g\t%s\n", v.code, value, v.text); }

static bool doubles(std::vector<double> &v)
{
    long long n;
    if (scanf("%lld", &n) != 1 || n < 0 || n > 100000) return false;
    v.resize((size_t)n);
    for (double &x : v)
        if (scanf("%lf", &x) != 1) return false;
    return true;
}

static bool ints(long long *a, int n)
{
    for (int k = 0; k < n; k++)
        if (scanf("%lld", a + k) != 1) return false;
    return true;
}

static int null_line()
{
    char rule[64];
    long long a[6];
    if (scanf(" %63s", rule) != 1) return 1;
    const std::string r(rule);
    if (r == "both_given" && ints(a, 2)) answer(pore_check::both_given(ptr(a[0]), ptr(a[1])), 0.0);
    else if (r == "thresholds_given" && ints(a, 2)) answer(pore_check::thresholds_given(ptr(a[0]), (int32_t)a[1]), 0.0);
    else if (r == "field_outputs" && ints(a, 6))
        answer(pore_check::field_outputs(a[0], (int32_t)a[1], ptr(a[2]), ptr(a[3]), ptr(a[4]), ptr(a[5])), 0.0);
    else if (r == "given_field_inputs" && ints(a, 6))
        answer(pore_check::given_field_inputs(ptr(a[0]), ptr(a[1]), a[2], ptr(a[3]), a[4] != 0, ptr(a[5])), 0.0);
    else if (r == "access_outputs" && ints(a, 5)) answer(pore_check::access_outputs(a[0], (int32_t)a[1], (int32_t)a[2], ptr(a[3]), ptr(a[4])), 0.0);
    else if (r == "psd_outputs" && ints(a, 4)) answer(pore_check::psd_outputs(a[0], (int32_t)a[1], ptr(a[2]), ptr(a[3])), 0.0);
    else if (r == "po_access_given" && ints(a, 4)) answer(pore_check::po_access_given(a[0], (int32_t)a[1], (int32_t)a[2], ptr(a[3])), 0.0);
    else return 1;
    return 0;
}

int main()
{
    char word[64];
    while (scanf(" %63s", word) == 1) {
        const std::string w(word);
        long long a[8];
        double x, y, z;
        std::vector<double> v;
        if (w == "grid" && ints(a, 7)) {
            const int32_t g[3] = {(int32_t)a[0], (int32_t)a[1], (int32_t)a[2]}, p[3] = {(int32_t)a[4], (int32_t)a[5], (int32_t)a[6]};
            answer(pore_check::grid(g, a[3] ? p : nullptr), 0.0);
        } else if (w == "bins" && scanf("%lf %lf %lld", &x, &y, a) == 3) {
            double nb = 0.0;
            int32_t nbins = 0;
            Verdict r = pore_check::bin_width(x, y, nb);
            if (r.code == AMOF_OK) r = pore_check::counter_words(nb, (int32_t)a[0], nbins);
            answer(r, (double)nbins);
        } else if (w == "radii" && doubles(v)) {
            double rmax = 0.0;
            const Verdict r = pore_check::radii(v.data(), (int)v.size(), rmax);
            answer(r, r.code == AMOF_OK ? rmax : 0.0);
        } else if (w == "thr" && doubles(v)) {
            answer(pore_check::thresholds_finite(v.data(), (int32_t)v.size()), 0.0);
        } else if (w == "finite" && doubles(v)) {
            double top = 0.0;
            const Verdict r = pore_check::field_finite(v.data(), v.size(), top);
            answer(r, r.code == AMOF_OK ? top : 0.0);
        } else if (w == "hha" && scanf("%lf %lf %lf", &x, &y, &z) == 3) {
            answer(pore_check::half_height_atoms(x, y, z), 0.0);
        } else if (w == "hhf" && scanf("%lf %lld %lf", &x, a, &z) == 3) {
            answer(pore_check::half_height_field(x, a[0], z), 0.0);
        } else if (w == "cap" && scanf("%lld %63s", a, word) == 2) {
            answer(pore_check::per_point_cap(a[0], strcmp(word, "field") == 0 ? "field" : "array"), 0.0);
        } else if (w == "labels" && ints(a, 2)) {
            answer(pore_check::labels_cap((int32_t)a[0], a[1]), 0.0);
        } else if (w == "null") {
            if (null_line()) return 2;
        } else {
            fprintf(stderr, "bad question: %s\n", word);
            return 2;
        }
    }
    return 0;
}
