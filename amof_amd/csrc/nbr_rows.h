// What the analyses that read neighbour rows share (nbr.hip: CN and BAD; order.hip: the bond order parameters; dihedral.hip):
// the kernels' argument records, the call records of the host side and the list stage of the frame tier as one function,
// frame_lists_tier.  lists_frame_kernel and all that plans and launches it stay in nbr.hip (the build has no relocatable device
// code); another analysis that reads the rows brings its `needed` matrix and a consumer, as order.hip and dihedral.hip do.
#pragma once
#include <functional>
#include <vector>

#include "amof_internal.h"
#include "nbr_check.h"

namespace amof {

constexpr int BAD_TILE = 64;
constexpr int NBRF_TILE = 256;
constexpr int NBRF_NLIST = 16;     // neighbours per centre bad_fast_kernel keeps in LDS (more: big-list pass of the exact kernel)
constexpr int NBRL_CAP = NBRF_NLIST;      // a fuller centre sends the call to the exact kernels, as in bad_fast_kernel
constexpr int NBRL_EW = 4;                // doubles per row entry: (ux, uy, uz, partner or 0.0) -- one aligned 32-byte sector per unit vector

struct NbrArgs {
    const double *pos;
    const double *geom;
    const double *img;
    const int32_t *nimg;
    const int32_t *perm;
    const Tile *tiles;
    const int32_t *sp_first_tile;  // [S]
    const int32_t *sp_ntiles;      // [S]
    const double *cutoff;          // [S][S]
    const int4 *work;              // (set/triple index, centre tile, A, B)
    int64_t N;
    int32_t F;
    int32_t n_cells;
    int32_t frames_per_chunk;
    int32_t S;
    int32_t max_img;
    int32_t n_sets;
    // CN outputs
    unsigned long long *sums;  // [F][n_sets]
    int32_t *per_atom;         // [F][n_sets][N] or null
    // BAD
    const double *edges;       // [nb+1]
    int32_t nb;
    unsigned long long *hist;  // [T][nb]
    unsigned long long *n_angles;
    int32_t *flags;            // [0] zero-length vector, [1] neighbour overflow, [2] largest neighbour count (count pass)
    int32_t cn_max;            // > 0: histograms keyed by the centre's neighbour count (BadByCn)
    // big-list pass of bad_kernel (centres with more than AMOF_MAX_NEIGHBOURS neighbours): the unit vectors live in
    // global scratch, [workgroup][3][ncap][BAD_TILE] doubles, instead of LDS
    double *nbuf;
    int32_t ncap;
    int32_t count_only;        // 1: only find the largest neighbour count (flags[2])
    int32_t global_hist;       // 1: more angle bins than LDS holds -- count with global atomics
    double edge_step;          // > 0: edges[k] == (double)k * edge_step exactly (hist_bin recomputes them); 0: read the table
    // Transposed neighbour lists (fast BAD kernels).  When both triples B-A-B and A-B-A of a species pair are asked
    // for, only the side with FEWER centres is searched; every pair it finds is also appended to the list of its
    // partner, and the angles around the other species' centres are formed from those lists (bad_transposed_kernel)
    // instead of a second search -- in ZIF-4 every N has one Zn neighbour and no angle at all, yet searching from the
    // 2304 N cost as much as the whole Zn-centred triple.  The neighbour test is symmetric (same fixed-point
    // differences negated, same canonical arithmetic), so the lists are the ones the search would have found.
    const int32_t *tr_off;     // [T] first slot of the derived triple's centres, for a searched triple; -1: none (or null)
    const int32_t *inv_rank;   // [N] position of an atom inside its species segment
    uint32_t *tcount;          // [frames of the batch][tr_total]
    uint32_t *tlist;           // [frames of the batch][tr_total][TR_CAP] partner atom indices
    int32_t tr_total;
};

// the neighbour rows of a batch of frames (lists_frame_kernel writes them, the consumers' kernels read them)
struct NbrListArgs {
    const int32_t *region_of;  // [S][S] first row of the ordered pair (centre species, partner species); -1: not kept
    const int32_t *inv_rank;   // [N] rank of an atom inside its species
    uint32_t *count;           // [frames of the batch][R]
    double *rows;              // [NBRL_CAP][frames of the batch * R][NBRL_EW] unit vectors centre -> neighbour, slot-major: the
                               // k-th neighbours of consecutive centres are neighbours in memory (dense writes, coalesced reads)
    size_t plane;              // frames of the batch * R
    int32_t R;
};

// ase.geometry.get_angles on two canonical minimum-image vectors (normalise, dot, clip, acos)
__device__ __forceinline__ bool unit_vec(double x, double y, double z, double &ux, double &uy, double &uz)
{
    const double nv = sqrt(x * x + y * y + z * z);
    if (!(nv > 0.0)) return false;
    ux = x / nv; uy = y / nv; uz = z / nv;
    return true;
}

// ------------------------------------------------------------ host side ----
struct NbrSetup {
    HostGeom geom;
    std::vector<double> img;
    std::vector<int32_t> nimg;
    int max_img = 0;
    HostTiles tiles;
    NbrArgs a;
    Stager stage;
};
int nbr_setup(amof_ctx *ctx, const amof_traj *t, const double *cutoff, int tile, NbrSetup &s);
void pick_chunks(int64_t F, size_t nwork, int32_t &fpc, unsigned &chunks);

// ---- what the tiers of one call share: first tier to last, each runs unless one before it is done ----
struct NbrCall {
    amof_ctx *ctx;
    const amof_traj *t;
    const double *cutoff;
    NbrSetup st;
    bool done = false;
};

// ---- the call of a histogram user (BAD, bond order, dihedral).  Every tier accumulates into the call's own buffers; the
// caller's only ever receive a complete, valid result.
struct HistCall : NbrCall {
    void *d_flags = nullptr;    // int32 [4]: NbrArgs::flags
    void *d_hs = nullptr;       // the scratch histogram (and whatever totals follow it)
    size_t hs_words = 0;
    void *d_fs = nullptr;       // per-frame sums, or null
    size_t fs_bytes = 0;
    StageSpans *spans = nullptr;
    // the three buffers (fs_bytes = 0: no frame sums); st.a.flags is set, nothing is cleared
    int alloc_outputs()
    {
        AMOF_TRY(ensure(ctx, SLOT_FLAGS, 4 * sizeof(int32_t), &d_flags));
        AMOF_TRY(ensure(ctx, SLOT_AUX7, hs_words * sizeof(unsigned long long), &d_hs));
        if (fs_bytes) AMOF_TRY(ensure(ctx, SLOT_OUT0, fs_bytes, &d_fs));
        st.a.flags = (int32_t *)d_flags;
        return AMOF_OK;
    }
    int read_flags(int32_t (&fl)[4])
    {
        AMOF_TRY(fetch(ctx, fl, d_flags, sizeof fl));
        AMOF_HIP_TRY(ctx, sync_stream(ctx));
        return AMOF_OK;
    }
    int reset_outputs()         // the outputs as before the first tier
    {
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_hs, 0, hs_words * sizeof(unsigned long long), ctx->stream));
        if (d_fs) AMOF_HIP_TRY(ctx, hipMemsetAsync(d_fs, 0, fs_bytes, ctx->stream));
        AMOF_HIP_TRY(ctx, hipMemsetAsync(d_flags, 0, 4 * sizeof(int32_t), ctx->stream));
        return AMOF_OK;
    }
};

// ---- the list stage of the frame tier: one sort + LDS search per species pair into neighbour rows, a consumer per batch ----
enum FrameUser { FRAME_CN, FRAME_BAD, FRAME_ORDER, FRAME_DIHEDRAL };      // (whose path name amof_last_path reports)
enum ListsOutcome {
    LISTS_NOT_APPLICABLE,       // the tier cannot take the call: the next tier answers
    LISTS_NOTHING,              // no ordered pair is needed: the outputs stay as they are and the call is done
    LISTS_RAN                   // every batch ran; qflag: an atom lay absurdly far from the cell
};
struct ListsRequest {
    const std::vector<char> &needed;    // [S][S] ordered pairs (centre species, partner species) whose rows the consumer reads
    const int32_t *head;                // the consumer's words at the head of the device table (RowsBatch::head), or null
    size_t head_words;
    const char *rows_env;               // megabytes of rows per batch (tests: many batches)
    bool zero_is_one_frame;             // a value of 0 there means one frame per batch
    FrameUser user;
};
struct RowsBatch {              // what a consumer's kernels get for one batch of frames
    NbrListArgs la;
    const int32_t *head;
    const int64_t *sp_first;    // [S + 1] first sorted position of every species
    const UploadPack *pk;       // the tier's tables, with whatever `tables` added to them
    int f_base, nfr;
    bool ortho;
};
// consume: queues the kernels that read the rows of one batch (once per batch, not per frame).  tables (BAD's merged items, or
// null): called once the tier takes the call, with region_of, to add tables to the pack that goes to the device with the tier's.
typedef std::function<int(const RowsBatch &)> RowsConsumer;
typedef std::function<void(const std::vector<int32_t> &region_of, UploadPack &pk)> RowsTables;
int frame_lists_tier(HistCall &c, const ListsRequest &rq, const RowsConsumer &consume, ListsOutcome &outcome, int32_t &qflag,
                     const RowsTables &tables = nullptr);

// what follows the tier for every user: nothing to do is done; after a run an undefined angle fails the call, and atoms absurdly
// far from the cell or a centre with more than NBRL_CAP neighbours hand the call, outputs reset, to the next tier
template <typename Call>
int frame_lists_finish(Call &c, ListsOutcome outcome, int32_t qflag)
{
    if (outcome == LISTS_NOT_APPLICABLE) return AMOF_OK;
    if (outcome == LISTS_RAN) {
        int32_t flags[4];
        AMOF_TRY(c.read_flags(flags));
        if (flags[0]) return fail(c.ctx, AMOF_EANGLE, "Undefined angle");
        if (qflag || flags[1]) return c.reset_outputs();
    }
    c.done = true;
    return AMOF_OK;
}

}  // namespace amof
