// amof_amd/csrc/dihedral_math.h on the CPU: the chain enumeration of include/amof_hip.h (amof_dihedral_hist) around the header's
// angle / undefined decision, fixed-point cosine term and pattern match, on unit vectors and index rows read from stdin.
//   N T nb
//   edges[nb + 1]
//   chains[T][4]                     species indices, -1 = any
//   species[N]
//   N rows:  deg  (j ux uy uz) x deg   the neighbours of atom i and the unit vectors i -> j
// Prints T lines "n undefined cos_sum hist[0] ... hist[nb - 1]" (integers).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../amof_amd/csrc/dihedral_math.h"

using namespace amof;

struct Entry {
    int j;
    double u[3];
};

int main()
{
    int N, T, nb;
    if (scanf("%d %d %d", &N, &T, &nb) != 3 || N < 0 || T < 1 || T > DIHEDRAL_MAX_CHAINS || nb < 1) return 2;
    std::vector<double> edges((size_t)nb + 1);
    for (double &e : edges)
        if (scanf("%lf", &e) != 1) return 2;
    std::vector<int32_t> chains((size_t)4 * T), species((size_t)N);
    for (int32_t &c : chains)
        if (scanf("%d", &c) != 1) return 2;
    for (int32_t &s : species)
        if (scanf("%d", &s) != 1) return 2;
    std::vector<std::vector<Entry>> rows((size_t)N);
    for (int i = 0; i < N; i++) {
        int deg;
        if (scanf("%d", &deg) != 1 || deg < 0) return 2;
        rows[(size_t)i].resize((size_t)deg);
        for (Entry &e : rows[(size_t)i])
            if (scanf("%d %lf %lf %lf", &e.j, &e.u[0], &e.u[1], &e.u[2]) != 4 || e.j < 0 || e.j >= N) return 2;
    }
    std::vector<long long> hist((size_t)T * nb, 0), n((size_t)T, 0), undefined((size_t)T, 0), cos_sum((size_t)T, 0);
    const double e0 = edges[0], en = edges[(size_t)nb], inv_w = (double)nb / (en - e0);
    for (int b = 0; b < N; b++)
        for (const Entry &bc : rows[(size_t)b]) {
            const int c = bc.j;
            if (c <= b) continue;
            for (const Entry &ba : rows[(size_t)b]) {
                if (ba.j == c) continue;
                for (const Entry &cd : rows[(size_t)c]) {
                    if (cd.j == b || cd.j == ba.j) continue;
                    uint32_t mask = dihedral::chain_mask(chains.data(), T, species[(size_t)ba.j], species[(size_t)b], species[(size_t)c],
                                                         species[(size_t)cd.j]);
                    if (!mask) continue;
                    double cosine;
                    const bool defined = dihedral::chain_cos(ba.u[0], ba.u[1], ba.u[2], bc.u[0], bc.u[1], bc.u[2], cd.u[0], cd.u[1], cd.u[2], cosine);
                    const int k = defined ? hist_bin(edges.data(), nb, dihedral::angle_deg(cosine), e0, en, inv_w) : -1;
                    for (int t = 0; t < T; t++) {
                        if (!(mask >> t & 1u)) continue;
                        if (!defined) {
                            undefined[(size_t)t]++;
                            continue;
                        }
                        n[(size_t)t]++;
                        cos_sum[(size_t)t] += dihedral::cos_term(cosine);
                        if (k >= 0) hist[(size_t)t * nb + k]++;
                    }
                }
            }
        }
    for (int t = 0; t < T; t++) {
        printf("%lld %lld %lld", n[(size_t)t], undefined[(size_t)t], cos_sum[(size_t)t]);
        for (int k = 0; k < nb; k++) printf(" %lld", hist[(size_t)t * nb + k]);
        printf("\n");
    }
    return 0;
}
