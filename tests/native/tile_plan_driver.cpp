// Prints what amof_amd/csrc/tile_plan.h computes for the inputs on stdin (tests/test_tile_plan_cpu.py compares with a
// brute-force count over the atoms' slabs).  The table lives in a heap block of exactly 257 words, so that a sanitizer
// build sees any read outside it.
//   line "T v0 .. v256"                             -> sets the slab table (no output)
//   line "W toff cntj s_first s_last G diag sub"    -> "qb0 qe0 qb1 qe1 mz0 mz1 zf x y z w" (tile_plan_window, tile_plan_pack)
//   line "S k"                                      -> slab of segment atom k (tile_plan_slab_of)
#include <stdio.h>

#include <vector>

#include "../../amof_amd/csrc/tile_plan.h"

int main()
{
    std::vector<uint32_t> table((size_t)amof::TILE_PLAN_SLABS + 1, 0u);
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'T') {
            for (auto &v : table)
                if (scanf("%u", &v) != 1) return 1;
        } else if (op == 'W') {
            int toff, cntj, diag, sub;
            unsigned s_first, s_last, G;
            if (scanf("%d %d %u %u %u %d %d", &toff, &cntj, &s_first, &s_last, &G, &diag, &sub) != 7) return 1;
            const amof::TileWindow w = amof::tile_plan_window(table.data(), toff, cntj, s_first, s_last, G, diag != 0, sub);
            const amof::TilePlanRecord r = amof::tile_plan_pack(w, s_first, s_last);
            printf("%d %d %d %d %d %d %d %u %u %u %u\n", w.qb[0], w.qe[0], w.qb[1], w.qe[1], w.mz[0], w.mz[1], w.zf, r.x, r.y, r.z, r.w);
        } else if (op == 'S') {
            unsigned k;
            if (scanf("%u", &k) != 1) return 1;
            printf("%u\n", amof::tile_plan_slab_of(table.data(), k));
        } else {
            return 2;
        }
    }
    return 0;
}
