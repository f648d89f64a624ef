// Which form answers a window-MSD call (msd.hip: fused, 2-pass fold, 3-pass, unwrap; msd_stream / msd_comb / msd_group on
// LDS-resident series, msd_comb_global / msd_global on long ones), the constants those decisions share with the kernels,
// and the species-sorted atom groups of the MSD and the Van Hove calls.  Host only (no HIP dependency: the CPU test suite
// compiles it with g++, tests/test_msd_select_cpu.py through tests/native/msd_select_driver.cpp).
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../include/amof_hip.h"

namespace amof {

constexpr int MSD_GROUP = 4;        // atoms per msd workgroup
constexpr int STREAM_CH = 42;       // msd_stream register scan: chunks of up to 42 entries per thread (F <= 41 T: 5248 frames at 128 threads)
constexpr int FU_EB = 5;            // fused form: comb entries (segments) per thread
#ifndef AMOF_FU_CPW
#define AMOF_FU_CPW 24
#endif
// fused form: columns (= 8 atoms) per workgroup; whole 128-byte lines measured slower: 32 (5-wave workgroups) 0.64, 16
// (2.5-wave workgroups) 0.57 against 0.47 ms (-DAMOF_FU_CPW=..: experiments)
constexpr int FU_CPW = AMOF_FU_CPW;
constexpr int FU_MAX_TPC = 21;      // fused form, threads per column: nq <= 105 (workgroups of <= 512 threads: 168 registers per lane)
constexpr size_t MSD_LDS_SERIES = 150 * 1024;   // a whole time series (+ window sums) of a column held in LDS
constexpr size_t MSD_LDS_DB = 80 * 1024;        // two column buffers of the comb kernel, twice per CU

// ---- the AMOF_MSD_* switches (tests / measurements), read once per call; every one means "set" ----
struct MsdSwitches {
    bool nocomb = false;            // AMOF_MSD_NOCOMB: evenly spaced windows are treated like any others (one-call path)
    bool nofused = false;           // AMOF_MSD_NOFUSED: never the fused form
    bool nostream = false;          // AMOF_MSD_NOSTREAM: never the streaming comb kernel
    bool nofold = false;            // AMOF_MSD_NOFOLD: the 3-pass form where the 2-pass fold would run
    bool nodb = false;              // AMOF_MSD_NODB: comb kernel with one column buffer
    bool fused_general = false;     // AMOF_MSD_FUSED_GENERAL: the general fused kernel where the lean one would run

    static MsdSwitches from_env()
    {
        MsdSwitches s;
        s.nocomb = getenv("AMOF_MSD_NOCOMB") != nullptr;
        s.nofused = getenv("AMOF_MSD_NOFUSED") != nullptr;
        s.nostream = getenv("AMOF_MSD_NOSTREAM") != nullptr;
        s.nofold = getenv("AMOF_MSD_NOFOLD") != nullptr;
        s.nodb = getenv("AMOF_MSD_NODB") != nullptr;
        s.fused_general = getenv("AMOF_MSD_FUSED_GENERAL") != nullptr;
        return s;
    }
};

// windows in arithmetic progression from 0 (the only thing WindowMsd produces), windows[w] = w d: d, else 0
inline int comb_spacing(const int32_t *windows, int W)
{
    if (W < 2 || windows[0] != 0 || windows[1] <= 0) return 0;
    const int d = windows[1];
    for (int w = 0; w < W; w++)
        if ((int64_t)windows[w] != (int64_t)w * d) return 0;
    return d;
}

// ---- the fused form ----
struct FusedDims {
    int d = 0, nq = 0, TPC = 0, L = 0;
    int64_t ncols = 0, stride = 0;      // columns of the atom range; row stride of RS / colpart (columns padded to 32)
    size_t lds = 0;
    unsigned threads = 0;
};

// does the fused form take windows m_w = w * comb_d, w = 0 .. W-1, over F frames?
inline bool fused_dims(int64_t F, int W, int comb_d, int64_t a0, int64_t a1, FusedDims &fd)
{
    if (comb_d < 16 || W < 2 || W > 32 || F < 64 || a1 <= a0) return false;
    fd.d = comb_d;
    fd.nq = (int)((F + comb_d - 1) / comb_d);
    fd.TPC = (fd.nq + FU_EB - 1) / FU_EB;
    if (fd.TPC > FU_MAX_TPC) return false;
    fd.L = W <= 8 ? 7 : W <= 16 ? 15 : W <= 25 ? 24 : 31;
    fd.ncols = 3 * (a1 - a0);
    fd.stride = (fd.ncols + 31) / 32 * 32;
    fd.threads = (unsigned)((fd.TPC * FU_CPW + 63) / 64 * 64);
    fd.lds = (size_t)2 * (fd.L + fd.TPC * FU_EB) * FU_CPW * sizeof(double);
    return true;
}

// the lean pass-2 kernel needs every thread to own FU_EB whole segments
inline bool fused_general(const FusedDims &fd, int64_t F, const MsdSwitches &sw)
{
    return fd.nq % FU_EB != 0 || F % fd.d != 0 || sw.fused_general;
}

// Pass 1: four atoms per lane where that still gives every SIMD a wave, two down to a quarter of that, else one (measured on
// the headline shape and its eighth, profiles/r05/msd_fused_experiments.txt: 4 x 2 0.248 / 0.092, 2 x 4 0.256 / 0.067,
// 1 x 4 0.273 / 0.073 ms).  tpl: atoms per lane, U: frames in flight, ntiles: tiles of 64 tpl atoms
struct SegShape {
    int tpl, U, ntiles;
};
inline SegShape seg_shape(int64_t atoms, int nq)
{
    const int64_t work = atoms * (int64_t)nq;
    SegShape s;
    s.tpl = work >= (int64_t)4 * 64 * 1024 ? 4 : work >= (int64_t)2 * 64 * 256 ? 2 : 1;
    s.U = s.tpl == 4 ? 2 : 4;
    s.ntiles = (int)((atoms + 64 * s.tpl - 1) / (64 * s.tpl));
    return s;
}

// ---- species-sorted groups of the atoms [a0, a1) ----
// (the MSD and the Van Hove kernels read the same record)
struct MsdGroup {
    int32_t start;    // into perm
    int32_t count;    // atoms
    int32_t species;
    int32_t _pad;
};
struct SpeciesGroups {
    std::vector<int32_t> perm;          // the atoms of the range sorted by species (stable)
    std::vector<MsdGroup> groups;       // at most group_size atoms of one species each
    std::vector<int32_t> group_first;   // [S + 1] species s owns groups[group_first[s] .. group_first[s + 1])
    std::vector<int32_t> atom_first;    // [S + 1] species s owns perm[atom_first[s] .. atom_first[s + 1])
};
inline void species_groups(const int32_t *species, int64_t a0, int64_t a1, int S, int group_size, SpeciesGroups &out)
{
    out.perm.clear();
    out.groups.clear();
    out.group_first.assign((size_t)S + 1, 0);
    out.atom_first.assign((size_t)S + 1, 0);
    for (int s = 0; s < S; s++) {
        out.group_first[s] = (int32_t)out.groups.size();
        const size_t first = out.perm.size();
        out.atom_first[s] = (int32_t)first;
        for (int64_t i = a0; i < a1; i++)
            if (species[i] == s) out.perm.push_back((int32_t)i);
        for (size_t off = first; off < out.perm.size(); off += (size_t)group_size)
            out.groups.push_back(MsdGroup{(int32_t)off, (int32_t)std::min<size_t>((size_t)group_size, out.perm.size() - off), s, 0});
    }
    out.group_first[S] = (int32_t)out.groups.size();
    out.atom_first[S] = (int32_t)out.perm.size();
}

// 2-pass and fused forms: lhalf[c] = smallest L_c (0.5 - 1e-6) over the cells -- a raw entry beyond lhalf - max|dc| may wrap
// again under the centre-of-mass step (a non-periodic axis never wraps)
inline void wrap_half_lengths(const amof_traj *t, double lhalf[3])
{
    for (int c = 0; c < 3; c++) {
        double lmin = 1e300;
        for (int64_t k = 0; k < t->n_cells; k++) lmin = std::min(lmin, fabs(t->cell[9 * k + 4 * c]));
        lhalf[c] = t->pbc[c] ? lmin * (0.5 - 1e-6) : 1e300;
    }
}

// ---- the selection ----
enum MsdColumns { MSD_COL_FOLD, MSD_COL_3PASS, MSD_COL_UNWRAP };
enum MsdFamily { MSD_STREAM, MSD_COMB, MSD_GROUP_LDS, MSD_COMB_GLOBAL, MSD_GLOBAL };
struct CombPass {
    int w0, wn, WT;     // windows w0 .. w0 + wn - 1 with the template bucket WT
};
struct MsdPlan {
    bool resident = false;      // the whole time series of a column and the window sums fit in LDS
    int comb_d = 0;             // window spacing the one-call path works with (0: no comb)
    // fused form, tried first (an answer of its flag hands the call to the forms below)
    bool fused = false, fused_general = false;
    FusedDims fd;
    // how the wrapped step columns are formed
    MsdColumns columns = MSD_COL_3PASS;
    // the window kernels and their template buckets
    MsdFamily family = MSD_GROUP_LDS;
    int stream_L = 0, stream_T = 0;     // stream
    bool regscan = false;
    int comb_WT = 0;                    // comb: the first 32 windows, then passes of up to 32
    bool db = false;
    std::vector<CombPass> comb_hi;
    int WREG = 0;                       // group
    int Rres = 0;                       // comb_global: residues held per workgroup; nq segments
    int64_t nq = 0;
    unsigned wchunks = 0;               // global
    size_t lds = 0;                     // dynamic LDS of the window launch (further comb passes: F doubles)
    const char *path = "";              // amof_last_path of the window family ("msd_fused" when the fused form answers)
};

inline MsdPlan msd_select(int64_t F, int64_t N, int W, const int32_t *windows, bool unwrap, bool remove_com, bool com_ext,
                          bool all_ortho, int64_t a0, int64_t a1, int64_t n_groups, const MsdSwitches &sw)
{
    MsdPlan p;
    const int64_t Fp = (F + 31) / 32 * 32;
    const size_t col_bytes = (size_t)Fp * sizeof(double);
    p.resident = ((size_t)F + (size_t)W) * sizeof(double) <= MSD_LDS_SERIES;
    p.comb_d = W <= (p.resident ? 128 : 256) && !sw.nocomb ? comb_spacing(windows, W) : 0;
    // The centre of mass as a correction of raw differences (fused and 2-pass forms): diagonal cells, the whole system in one
    // call (the centre of mass needs every atom; atom-sharded ranks go through amof_msd_shard_begin / _finish), no unwrap
    const bool raw_com = !unwrap && remove_com && !com_ext && all_ortho && a0 == 0 && a1 == N;
    p.fused = raw_com && !sw.nofused && fused_dims(F, W, p.comb_d, a0, a1, p.fd);
    p.fused_general = p.fused && fused_general(p.fd, F, sw);
    // streaming comb kernel: one thread per residue class (window spacing 64 .. 256 frames, <= 32 windows); it subtracts C in
    // its register scan, chunks of at most STREAM_CH entries per thread
    const bool stream = p.resident && p.comb_d >= 64 && p.comb_d <= 256 && W <= 32 && col_bytes <= MSD_LDS_SERIES && !sw.nostream;
    p.stream_T = p.comb_d <= 128 ? 128 : 256;
    p.regscan = (((F + p.stream_T - 1) / p.stream_T) | 1) <= STREAM_CH;
    const bool fold = raw_com && p.resident && !(stream && !p.regscan) && !sw.nofold;
    p.columns = fold ? MSD_COL_FOLD : unwrap ? MSD_COL_UNWRAP : MSD_COL_3PASS;
    if (stream) {
        p.family = MSD_STREAM;
        p.stream_L = W <= 8 ? 7 : W <= 16 ? 15 : W <= 24 ? 23 : W <= 25 ? 24 : 31;
        p.lds = col_bytes;
        p.path = "msd_stream";
    } else if (p.resident && p.comb_d > 0) {
        p.family = MSD_COMB;
        p.comb_WT = std::min((W + 3) / 4 * 4, 32);
        // two column buffers (the next column streams in behind the arithmetic) when they fit twice per CU
        p.db = 2 * col_bytes <= MSD_LDS_DB && !sw.nodb;
        p.lds = p.db ? 2 * col_bytes : (size_t)F * sizeof(double);
        // windows 32 .. W-1 in further passes of up to 32 (each re-reads the columns)
        for (int w0 = 32; w0 < W; w0 += 32) {
            const int wn = std::min(32, W - w0);
            p.comb_hi.push_back(CombPass{w0, wn, wn <= 8 ? 8 : wn <= 16 ? 16 : 32});
        }
        p.path = "msd_comb";
    } else if (p.resident) {
        p.family = MSD_GROUP_LDS;
        p.WREG = W <= 8 ? 8 : W <= 32 ? 32 : 0;
        p.lds = ((size_t)F + (size_t)W) * sizeof(double);
        p.path = "msd_group";
    } else {
        // long trajectory: every column prefix-summed in global memory, the windows reduced from there
        p.nq = p.comb_d > 0 ? (F + p.comb_d - 1) / p.comb_d : 0;
        p.Rres = p.nq > 0 ? (int)std::min<int64_t>(std::min<int64_t>(p.comb_d, 32), 16384 / p.nq) : 0;
        if (p.Rres >= 1) {
            p.family = MSD_COMB_GLOBAL;     // comb kernel on the scanned columns, 32 windows per launch
            p.lds = (size_t)p.nq * (size_t)p.Rres * sizeof(double);
            p.path = "msd_comb_global";
        } else {
            p.family = MSD_GLOBAL;
            const int64_t g = std::max<int64_t>(1, n_groups);
            p.wchunks = (unsigned)std::min<int64_t>(65535, std::max<int64_t>(1, std::min<int64_t>(W, (4096 + g - 1) / g)));
            p.path = "msd_global";
        }
    }
    return p;
}

}  // namespace amof
