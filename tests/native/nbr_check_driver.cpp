// Answers questions about amof_amd/csrc/nbr_check.h on stdin (tests/test_nbr_check_cpu.py), one line each; every answer is
// "code <tab> value <tab> message" (value: what the rule computes besides its verdict, 0 where nothing).  Doubles are read with
// %lf: decimal, hexadecimal ("0x1.8p+1"), "nan", "inf".
//   "sets S n a0 b0 .."  |  "triples S T .."  |  "chains S T .."      species named by a call
//   "bondset S a b rc"                    bond_set_species, then bond_set_cutoff
//   "values cutoff|link n v0 .."          values_not_negative
//   "sym S m00 .."                        symmetric
//   "matrix cutoff|link S m00 .."         bond_matrix
//   "badbins nb" | "histbins nb" | "orderbins nbins nbins_tet" | "edges nb e0 .. e(nb)"
//   "nl n_l max" | "l top n l0 .." | "nchains T max" | "cnmax v"
//   "hh rc hmin" | "hhs rc set hmin order|bond"                       half_height, half_height_set with either tail
//   "hmin p0 p1 p2 n_cells rec[24 n_cells]"                           -> min_periodic_height
//   "step nb e0 .. e(nb)"                                             -> uniform_edge_step
//   "bins nb e0 .. e(nb) n x0 .."         hist_bin (angle_math.h) of every x through the table -> message "k0,k1,.."; value: how
//                                         many differ through uniform_edge_step (0 where the edges are not uniform: nothing to compare)
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../amof_amd/csrc/angle_math.h"
#include "../../amof_amd/csrc/nbr_check.h"

using namespace amof;
using nbr_check::Verdict;

static void answer(const Verdict &v, double value) { printf("%d\t%.17g\t%s\n", v.code, value, v.text); }

static bool doubles(std::vector<double> &v, long long n)
{
    if (n < 0 || n > 1000000) return false;
    v.resize((size_t)n);
    for (double &x : v)
        if (scanf("%lf", &x) != 1) return false;
    return true;
}

static bool ints(std::vector<int32_t> &v, long long n)
{
    if (n < 0 || n > 1000000) return false;
    v.resize((size_t)n);
    for (int32_t &x : v)
        if (scanf("%d", &x) != 1) return false;
    return true;
}

int main()
{
    char word[64], what[64];
    while (scanf(" %63s", word) == 1) {
        const std::string w(word);
        long long a[4];
        double x, y;
        std::vector<double> v, xs;
        std::vector<int32_t> s;
        if ((w == "sets" || w == "triples" || w == "chains") && scanf("%lld %lld", a, a + 1) == 2 &&
            ints(s, a[1] * (w == "chains" ? 4 : 2))) {
            if (w == "sets") answer(nbr_check::sets_in_range(s.data(), (int32_t)a[1], (int)a[0]), 0.0);
            else if (w == "triples") answer(nbr_check::triples_in_range(s.data(), (int32_t)a[1], (int)a[0]), 0.0);
            else answer(nbr_check::chains_in_range(s.data(), (int32_t)a[1], (int)a[0]), 0.0);
        } else if (w == "bondset" && scanf("%lld %lld %lld %lf", a, a + 1, a + 2, &x) == 4) {
            const int32_t set[6] = {0, 0, 0, 0, (int32_t)a[1], (int32_t)a[2]};     // (asked as set 2)
            Verdict r = nbr_check::bond_set_species(set, 2, (int)a[0]);
            if (r.code == AMOF_OK) r = nbr_check::bond_set_cutoff(x, 2);
            answer(r, 0.0);
        } else if (w == "values" && scanf(" %63s %lld", what, a) == 2 && doubles(v, a[0])) {
            answer(nbr_check::values_not_negative(v.data(), (int)v.size(), strcmp(what, "link") == 0 ? "link" : "cutoff"), 0.0);
        } else if (w == "sym" && scanf("%lld", a) == 1 && doubles(v, a[0] * a[0])) {
            answer(nbr_check::symmetric(v.data(), (int)a[0]), 0.0);
        } else if (w == "matrix" && scanf(" %63s %lld", what, a) == 2 && doubles(v, a[0] * a[0])) {
            answer(nbr_check::bond_matrix(v.data(), (int)a[0], strcmp(what, "link") == 0 ? "link" : "cutoff"), 0.0);
        } else if (w == "badbins" && scanf("%lld", a) == 1) {
            answer(nbr_check::bad_bins((int32_t)a[0]), 0.0);
        } else if (w == "histbins" && scanf("%lld", a) == 1) {
            answer(nbr_check::hist_bins((int32_t)a[0]), 0.0);
        } else if (w == "orderbins" && scanf("%lld %lld", a, a + 1) == 2) {
            answer(nbr_check::order_bins((int32_t)a[0], (int32_t)a[1]), 0.0);
        } else if (w == "edges" && scanf("%lld", a) == 1 && doubles(v, a[0] + 1)) {
            answer(nbr_check::edges_increase(v.data(), (int32_t)a[0]), 0.0);
        } else if (w == "nl" && scanf("%lld %lld", a, a + 1) == 2) {
            answer(nbr_check::order_l_count((int32_t)a[0], (int)a[1]), 0.0);
        } else if (w == "l" && scanf("%lld %lld", a, a + 1) == 2 && ints(s, a[1])) {
            answer(nbr_check::order_l(s.data(), (int32_t)s.size(), (int)a[0]), 0.0);
        } else if (w == "nchains" && scanf("%lld %lld", a, a + 1) == 2) {
            answer(nbr_check::chain_count((int32_t)a[0], (int)a[1]), 0.0);
        } else if (w == "cnmax" && scanf("%lld", a) == 1) {
            answer(nbr_check::cn_max_range((int32_t)a[0]), 0.0);
        } else if (w == "hh" && scanf("%lf %lf", &x, &y) == 2) {
            answer(nbr_check::half_height(x, y), 0.0);
        } else if (w == "hhs" && scanf("%lf %lld %lf %63s", &x, a, &y, what) == 4) {
            answer(nbr_check::half_height_set(x, (int)a[0], y, strcmp(what, "order") == 0 ? "a neighbour could be counted twice"
                                                                                          : "a pair could be bonded twice"), 0.0);
        } else if (w == "hmin" && scanf("%lld %lld %lld %lld", a, a + 1, a + 2, a + 3) == 4 && doubles(v, a[3] * nbr_check::GEOM_REC)) {
            const uint8_t pbc[3] = {(uint8_t)a[0], (uint8_t)a[1], (uint8_t)a[2]};
            answer(Verdict(), nbr_check::min_periodic_height(pbc, v.data(), a[3]));
        } else if (w == "step" && scanf("%lld", a) == 1 && doubles(v, a[0] + 1)) {
            answer(Verdict(), nbr_check::uniform_edge_step(v.data(), (int32_t)a[0]));
        } else if (w == "bins" && scanf("%lld", a) == 1 && doubles(v, a[0] + 1) && scanf("%lld", a + 1) == 1 && doubles(xs, a[1])) {
            const int nb = (int)a[0];
            const double e0 = v[0], en = v[(size_t)nb], inv_w = (double)nb / (en - e0);     // (hist_bin's first guess, as the kernels form it)
            const double step = nbr_check::uniform_edge_step(v.data(), nb);
            Verdict r;
            std::string text;
            long long differ = 0;
            for (double ang : xs) {
                const int k = hist_bin(v.data(), nb, ang, e0, en, inv_w, 0.0);
                if (step > 0.0 && hist_bin(v.data(), nb, ang, e0, en, inv_w, step) != k) differ++;
                text += (text.empty() ? "" : ",") + std::to_string(k);
            }
            printf("%d\t%.17g\t%s\n", r.code, (double)differ, text.c_str());
        } else {
            fprintf(stderr, "bad question: %s\n", word);
            return 2;
        }
    }
    return 0;
}
