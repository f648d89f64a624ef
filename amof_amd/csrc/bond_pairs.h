// The pair-table stage of bond.hip, callable from the other files that walk pairs through frames (lindemann.hip):
// bond_list_kernel over the frames first_frame + stride o (o < n_origins) -> bond_rowcount_kernel -> host prefix sum ->
// bond_compact_kernel, a piece of centres (bitmap <= 256 MB) and inside it a group of whole rows (at most pair_max pairs)
// at a time.  The table of a group is sorted by centre, then by partner, and free of duplicates; it holds every ordered pair
// (i of A, j of B, i != j, i a centre of the atom range) with d2 < rc^2 (1 + 1e-9) in at least one of the frames: a superset of
// the pairs bonded there, so the caller decides h itself.
#pragma once

#include <functional>

#include "amof_internal.h"

namespace amof {

struct BondPairCall {
    amof_ctx *ctx;
    StageSpans *spans;          // stage 0 spans the launches and the read-back of the row counts
    const double *pos_dev;      // [F][N][3]
    const double *d_geom;       // device geometry records
    const int32_t *d_perm;      // device copy of tiles->perm
    const HostTiles *tiles;     // build_tiles(t, BOND_LIST_TILE, ..)
    int64_t N;
    int32_t n_cells;
    bool ortho;
    int64_t first_frame, stride, n_origins;     // the frames of the list
    size_t pair_max;            // bond_pair_budget()
};

constexpr int BOND_LIST_TILE = 256;     // bond_list_kernel: a centre per thread, partner tiles of 256 atoms

// pairs of a group's table: 2^25 (256 MB), or AMOF_BOND_PAIR_BUDGET
size_t bond_pair_budget();

// every group of set s = (A, B): each(d_pairs, P) with the group's table in SLOT_AUX3 (P > 0); SLOT_AUX0 .. AUX3 are taken
int bond_pair_groups(const BondPairCall &c, int s, int A, int B, double rc, int64_t atom_begin, int64_t atom_end,
                     const std::function<int(const int2 *, size_t)> &each);

}  // namespace amof
