// Answers questions about amof_amd/csrc/msd_select.h on stdin (tests/test_msd_select_cpu.py), one line each:
//   "P F N unwrap remove_com com_ext all_ortho a0 a1 n_groups W d [w0 .. wW-1] | switch names .. ;"
//        windows w d for d > 0, the listed ones for d = 0
//        -> resident comb_d fused fused_general fd.d fd.nq fd.TPC fd.L fd.threads fd.lds columns family stream_L stream_T
//           regscan comb_WT db WREG Rres nq wchunks lds path n_hi then (w0 wn WT) of every further comb pass
//   "C W w0 .. wW-1"          -> comb_spacing
//   "Q atoms nq"              -> tpl U ntiles of seg_shape
//   "G S group_size a0 a1 N s0 .. sN-1"
//        -> n_perm perm.. n_groups (start count species).. group_first[0..S] atom_first[0..S]
//   "H n_cells pbc0 pbc1 pbc2 c0 .. c(9 n_cells - 1)" -> lhalf[0..2] of wrap_half_lengths
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../amof_amd/csrc/msd_select.h"

using namespace amof;

static bool set_switch(MsdSwitches &sw, const std::string &name)
{
    struct { const char *n; bool MsdSwitches::*m; } tab[] = {
        {"nocomb", &MsdSwitches::nocomb}, {"nofused", &MsdSwitches::nofused}, {"nostream", &MsdSwitches::nostream},
        {"nofold", &MsdSwitches::nofold}, {"nodb", &MsdSwitches::nodb}, {"fused_general", &MsdSwitches::fused_general}};
    for (auto &e : tab)
        if (name == e.n) { sw.*(e.m) = true; return true; }
    return false;
}

static bool read_ints(std::vector<int32_t> &v)
{
    for (auto &x : v)
        if (scanf("%d", &x) != 1) return false;
    return true;
}

static int plan_line()
{
    long long F, N, a0, a1, n_groups;
    int unwrap, remove_com, com_ext, all_ortho, W, d;
    if (scanf("%lld %lld %d %d %d %d %lld %lld %lld %d %d", &F, &N, &unwrap, &remove_com, &com_ext, &all_ortho, &a0, &a1, &n_groups, &W,
              &d) != 11 || F < 1 || W < 1 || W > 100000 || d < 0 || a0 < 0 || a1 > N || a0 >= a1) return 1;
    std::vector<int32_t> win((size_t)W);
    if (d > 0) {
        for (int w = 0; w < W; w++) win[(size_t)w] = w * d;
    } else if (!read_ints(win)) {
        return 1;
    }
    MsdSwitches sw;
    char word[64];
    if (scanf(" %63s", word) != 1 || strcmp(word, "|") != 0) return 1;
    while (scanf(" %63s", word) == 1 && strcmp(word, ";") != 0)
        if (!set_switch(sw, word)) return 3;
    const MsdPlan p = msd_select(F, N, W, win.data(), unwrap != 0, remove_com != 0, com_ext != 0, all_ortho != 0, a0, a1, n_groups, sw);
    const FusedDims fd = p.fused ? p.fd : FusedDims();
    printf("%d %d %d %d %d %d %d %d %u %zu %d %d %d %d %d %d %d %d %d %lld %u %zu %s %zu", p.resident, p.comb_d, p.fused, p.fused_general,
           fd.d, fd.nq, fd.TPC, fd.L, fd.threads, fd.lds, (int)p.columns, (int)p.family, p.stream_L, p.stream_T, p.regscan, p.comb_WT,
           p.db, p.WREG, p.Rres, (long long)p.nq, p.wchunks, p.lds, p.path, p.comb_hi.size());
    for (const CombPass &h : p.comb_hi) printf(" %d %d %d", h.w0, h.wn, h.WT);
    printf("\n");
    return 0;
}

static int groups_line()
{
    int S, gs;
    long long a0, a1, N;
    if (scanf("%d %d %lld %lld %lld", &S, &gs, &a0, &a1, &N) != 5 || S < 0 || gs < 1 || N < 0 || N > 10000000 || a0 < 0 || a1 > N ||
        a0 > a1) return 1;
    std::vector<int32_t> species((size_t)N);
    if (!read_ints(species)) return 1;
    SpeciesGroups sg;
    species_groups(species.data(), a0, a1, S, gs, sg);
    printf("%zu", sg.perm.size());
    for (int32_t v : sg.perm) printf(" %d", v);
    printf(" %zu", sg.groups.size());
    for (const MsdGroup &g : sg.groups) printf(" %d %d %d", g.start, g.count, g.species);
    for (int32_t v : sg.group_first) printf(" %d", v);
    for (int32_t v : sg.atom_first) printf(" %d", v);
    printf("\n");
    return 0;
}

int main()
{
    char tag;
    while (scanf(" %c", &tag) == 1) {
        if (tag == 'P') {
            const int rc = plan_line();
            if (rc) return rc;
        } else if (tag == 'C') {
            int W;
            if (scanf("%d", &W) != 1 || W < 0 || W > 100000) return 1;
            std::vector<int32_t> win((size_t)W);
            if (!read_ints(win)) return 1;
            printf("%d\n", comb_spacing(win.data(), W));
        } else if (tag == 'Q') {
            long long atoms;
            int nq;
            if (scanf("%lld %d", &atoms, &nq) != 2 || atoms < 1 || nq < 1) return 1;
            const SegShape s = seg_shape(atoms, nq);
            printf("%d %d %d\n", s.tpl, s.U, s.ntiles);
        } else if (tag == 'G') {
            const int rc = groups_line();
            if (rc) return rc;
        } else if (tag == 'H') {
            int n, pbc[3];
            if (scanf("%d %d %d %d", &n, &pbc[0], &pbc[1], &pbc[2]) != 4 || n < 1 || n > 100000) return 1;
            std::vector<double> cell((size_t)n * 9);
            for (double &v : cell)
                if (scanf("%lf", &v) != 1) return 1;
            amof_traj t;
            memset(&t, 0, sizeof t);
            t.cell = cell.data();
            t.n_cells = n;
            for (int q = 0; q < 3; q++) t.pbc[q] = (uint8_t)pbc[q];
            double lhalf[3];
            wrap_half_lengths(&t, lhalf);
            printf("%.17g %.17g %.17g\n", lhalf[0], lhalf[1], lhalf[2]);
        } else {
            return 2;
        }
    }
    return 0;
}
