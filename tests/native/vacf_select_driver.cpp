// Answers questions about amof_amd/csrc/vacf_select.h on stdin (tests/test_vacf_select_cpu.py), one line each:
//   "P F stride switches W d"  windows w d, w < W; switches: 1 general + 2 nodb + 4 db
//        -> kernel n_tiles lanes tile_lags tail series db lds path, then (first lag, lags) of every tile
//   "K"  -> VACF_GROUP VACF_R VACF_MAX_LANES VACF_LDS_BUDGET
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/vacf_select.h"

using namespace amof;

int main()
{
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'K') {
            printf("%d %d %d %zu\n", VACF_GROUP, VACF_R, VACF_MAX_LANES, VACF_LDS_BUDGET);
        } else if (tag == 'P') {
            long long F, stride;
            int general, W, d;
            if (scanf("%lld %lld %d %d %d", &F, &stride, &general, &W, &d) != 5 || F < 1 || W < 0 || W > 10000000 || d < 1) return 1;
            std::vector<int32_t> win((size_t)W);
            for (int w = 0; w < W; w++) win[(size_t)w] = w * d;
            VacfSwitches sw;
            sw.general = (general & 1) != 0;
            sw.nodb = (general & 2) != 0;
            sw.db = (general & 4) != 0;
            const VacfPlan p = vacf_select(F, W, win.data(), stride, sw);
            printf("%d %d %d %d %d %lld %d %zu %s", (int)p.kernel, p.n_tiles, p.lanes, p.tile_lags, p.tail, (long long)p.series, (int)p.db,
                   p.lds, p.path);
            for (int t = 0; t < p.n_tiles; t++) {
                const int first = t * p.tile_lags;
                printf(" %d %d", first, std::min(W, first + p.tile_lags) - first);
            }
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
