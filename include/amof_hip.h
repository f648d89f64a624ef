/*
 * amof_hip.h -- C ABI of libamofhip.so: MI355X (gfx950) kernels for aMOF's
 * per-frame pair-distance hot path (RDF / CN / BAD / window MSD).
 *
 * The reference (coudertlab/amof v1.1.0) is pure Python and has no FFI of its
 * own; the seam this library fills is the set of third-party / numpy call
 * sites underneath its analysis classes.  Each entry point names the reference
 * interface it replaces (paths relative to the reference root).  Host Python
 * (the amof_amd Python package) keeps everything that is O(bins): bin-count arithmetic,
 * normalisation, column naming, DataFrames.
 *
 * Conventions
 *   - plain C types only; no C++ exceptions cross the boundary; never aborts.
 *   - return value: 0 = AMOF_OK, negative = error; amof_last_error(ctx) gives
 *     a human-readable message for the last failing call on that context.
 *   - buffers are caller-owned; the library keeps no caller pointer after a call
 *     returns.  Every entry point is synchronous: it returns after its work on the
 *     context's stream has completed.  "_dev" entry points take caller-owned DEVICE
 *     output buffers (e.g. a torch tensor that an RCCL all-reduce consumes next) and
 *     run on the stream set with amof_ctx_set_stream.
 *   - a context is bound to one device and is not thread-safe; distinct
 *     contexts may be used concurrently.  ctypes releases the GIL during calls.
 *   - all integer results are exact and independent of launch geometry.
 */
#ifndef AMOF_HIP_H
#define AMOF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMOF_OK 0
#define AMOF_EINVAL (-1)     /* bad argument */
#define AMOF_ESINGULAR (-2)  /* singular cell */
#define AMOF_EANGLE (-3)     /* undefined angle (zero-length bond vector): ASE raises ZeroDivisionError */
#define AMOF_ENOMEM (-4)     /* host or device allocation failed */
#define AMOF_EHIP (-5)       /* HIP runtime error (message in amof_last_error) */
#define AMOF_ECAPACITY (-6)  /* a documented kernel capacity was exceeded */
#define AMOF_ENODEVICE (-7)  /* no usable GPU */
#define AMOF_EUNSUPPORTED (-8) /* a specialised entry point does not take these arguments: use the general one */

#define AMOF_ABI_VERSION 4

/* capacities */
#define AMOF_MAX_LDS_BINS 36864     /* histogram bins held in LDS per workgroup (u32); more bins: global-memory kernels */
#define AMOF_MAX_NEIGHBOURS 32      /* neighbours per centre atom the exact BAD kernel keeps in LDS (the fast kernels keep
                                       16 and hand a call with a fuller centre to the exact kernel); a centre with more
                                       sends the call through a further pass with lists in global memory (no error) */
#define AMOF_MAX_IMAGES 4096        /* extra periodic images per frame (AMOF_ECAPACITY when exceeded) */
#define AMOF_PORE_MAX_WORDS 2048    /* amof_pore_field: nbins + 2 + n_thresholds counters per frame (AMOF_ECAPACITY beyond) */

typedef struct amof_ctx amof_ctx;

/*
 * A trajectory as the reference sees it: a list of F frames of the same N atoms
 * (amof/trajectory.py:27-35; species read from frame 0 only, amof/rdf.py:71).
 */
typedef struct amof_traj {
    const double *pos;      /* [F][N][3] xyz, float64, C-contiguous                  */
    int32_t pos_on_device;  /* 0: pos is a host pointer; 1: device pointer (resident) */
    int32_t n_species;      /* S                                                     */
    const double *cell;     /* HOST [n_cells][3][3], rows = cell vectors (ASE)       */
    int64_t n_cells;        /* 1 (constant cell) or F                                */
    int64_t n_frames;       /* F                                                     */
    int64_t n_atoms;        /* N                                                     */
    const int32_t *species; /* HOST [N], species index 0..S-1                        */
    const double *masses;   /* HOST [N]; MSD only (centre of mass), else may be NULL */
    uint8_t pbc[3];         /* periodic flags per cell vector (ase.Atoms.pbc)        */
    uint8_t _pad[5];
} amof_traj;

int amof_abi_version(void);

/* number of visible GPUs (hipGetDeviceCount); 0 when none */
int amof_device_count(void);

int amof_ctx_create(int device, amof_ctx **out);
/* The same with flags.  AMOF_CTX_HIGH_PRIORITY: the context's stream is created at the device's highest stream
 * priority -- the second context of a device, on which the memory-bound analyses (MSD, BAD, CN) run beside the
 * pair-evaluation-bound RDF launch of the first (the reference runs its analyses as independent calls,
 * examples/Compute structural properties.py:58-118, and parallelises inside them with joblib, amof/msd.py:252-256);
 * their workgroups are dispatched ahead of the RDF kernel's whenever a CU has room. */
#define AMOF_CTX_HIGH_PRIORITY 1
/* AMOF_CTX_LOW_PRIORITY: the lowest stream priority -- its workgroups are dispatched where the other context's kernel
 * leaves compute units free: before that kernel starts and in its tail, instead of delaying it. */
#define AMOF_CTX_LOW_PRIORITY 2
int amof_ctx_create2(int device, int flags, amof_ctx **out);
void amof_ctx_destroy(amof_ctx *ctx);
const char *amof_last_error(const amof_ctx *ctx);

/* Run subsequent work on the caller's hipStream_t (e.g. torch's current
 * stream).  NULL restores the context's own stream. */
int amof_ctx_set_stream(amof_ctx *ctx, void *hip_stream);
int amof_ctx_synchronize(amof_ctx *ctx);
/* Order the context's stream after everything queued so far on another stream of the same device
 * (hipEventRecord + hipStreamWaitEvent; NULL = the legacy default stream).  A caller that hands over
 * a device-resident `pos` produced by work still pending on its own stream (a torch tensor, say)
 * calls this first: the library's kernels otherwise run on the context's non-blocking stream with
 * no ordering against the producer. */
int amof_ctx_wait_stream(amof_ctx *ctx, void *hip_stream);
/* Two contexts of one device, driven by two host threads (amof_amd/_lazy.py: the RDF on one, the memory-bound analyses on
 * the other).  Their kernels do not run well side by side -- the RDF tile kernel fills the LDS and the register file of every
 * CU, a second stream's workgroups trickle in between and both lose (profiles/r05/stops.txt A) -- so the second context
 * FOLLOWS the first: amof_ctx_follow waits on the HOST (at most timeout_s) until `other` has begun its call number
 * min_calls (amof_ctx_calls counts them; 0: no host wait) and queued that call's dominant kernel, then orders ctx's stream
 * after everything `other` has queued so far (amof_ctx_wait_stream).  The follower's host work (tables, uploads) then runs
 * beside the leader's kernel, its kernels right behind it, beside the leader's read-back and result assembly.
 * Returns 1 when ordered, 0 on timeout (nothing ordered: the caller decides), < 0 on error.  Safe to call while `other` is
 * inside a call on another thread.  The classes use it only on request (AMOF_LANE_ORDER=1): on the headline workload the
 * ordered lanes measure the same as the unordered ones at N = 1 and 0.1 - 0.2 ms slower for one rank of eight
 * (profiles/r05/lane_order.txt).  Replaces nothing in the reference (its analyses run one after the other:
 * examples/Compute structural properties.py:58-118). */
int amof_ctx_follow(amof_ctx *ctx, amof_ctx *other, int64_t min_calls, double timeout_s);
/* calls of this context that have started device work so far (any thread may ask) */
int64_t amof_ctx_calls(const amof_ctx *ctx);
/* Diagnostics for the test-suite: fill every scratch buffer the context currently owns with `byte`
 * (after a synchronisation).  No call may depend on what a previous call left in scratch; a test
 * that poisons between calls turns such a dependence into a wrong answer instead of a lucky one. */
int amof_ctx_debug_poison(amof_ctx *ctx, int byte);

/* Seconds spent inside kernels of the last call, measured with HIP events on
 * the context's stream around the dominant kernel's launches:
 * which = 0 total, 1 dominant kernel only.  After amof_isf_accumulate[_dev] also the sums over the call's launches of
 * which = 2 the rho table (quantisation included), 3 the correlation kernel, 4 the self part (0 if not asked for);
 * after amof_bond_survival[_dev]: 2 the bond lists, 3 the bit series, 4 the correlations;
 * after amof_bond_reorientation[_dev]: 2 the bond lists, 3 the bit series, 4 the vector table and the reorientation sums.
 * after amof_lindemann[_dev]: 2 the pair lists, 3 the moments, 4 the reduction (0 on "lindemann_simple").
 * after amof_bond_order[_dev]: 2 the list stage, 3 the order kernels.
 * after amof_vacf_window[_dev]: 2 the columns, 3 the correlation kernel with its reduction.
 * after amof_current_accumulate[_dev]: 2 the records (means and vmax included), 3 the table, 4 the correlation kernel.
 * after amof_dihedral_hist[_dev]: 2 the list stage (the adjacency rows on "dihedral_exact"), 3 the dihedral kernels.
 * after amof_ring_stats: 2 the adjacency rows, 3 the breadth-first searches (distance table, candidates), 4 the ring search.
 * after amof_fragment_stats: 2 the adjacency rows (the link rows included), 3 the labelling (bond images and rounds), 4 the
 *   reduction with the census.
 * after amof_pore_field: 2 the cell sort (0 on "pore_exact"), 3 the field kernels.
 * after amof_pore_access / amof_pore_access_field: 4 the labelling (amof_pore_access: 2 and 3 as amof_pore_field).
 * after amof_pore_psd / amof_pore_psd_field: 5 the covering stage (2 .. 4 as amof_pore_access where those stages ran).
 * after amof_pore_surface: 6 the surface stage, its cell sorts included (2 .. 5 as amof_pore_psd where those stages ran).
 * Returns < 0 if unavailable. */
double amof_last_kernel_seconds(const amof_ctx *ctx, int which);
/* number of launches of the dominant kernel in the last call */
int64_t amof_last_kernel_launches(const amof_ctx *ctx);
/* kernel family that produced the result of the last call (diagnostics and tests; "" before the first call):
 *   RDF  "rdf_tile_zf" (diagonal cells, f32 slab coordinates), "rdf_tile_tri" (general cells in the orthogonalised
 *        lattice frame, f32 slab coordinates), "rdf_tile" (plain general tile kernel), "rdf_tile_img" (cutoffs beyond
 *        half a cell height where "rdf_tile_tri" does not apply), "rdf_cell" (3-D cell list), "rdf_range" (2-level list),
 *        "rdf_exact" (canonical float64 arithmetic per pair)
 *   CN   "cn_frame" (whole frame in LDS), "cn_frame_slabs" (z-slabs of a frame in LDS: pairs of more than 8192 atoms),
 *        "cn_cell", "cn_fast", "cn_exact"
 *   BAD  "bad_frame" (whole frame in LDS), "bad_frame_slabs" (z-slabs of a frame in LDS), "bad_cell", "bad_fast",
 *        "bad_exact", "bad_exact_biglist"
 *   MSD  "msd_fused" (no transposed copy: diagonal cells, evenly spaced windows), "msd_stream" (register-ring comb, window
 *        spacing 64..256), "msd_comb" (block comb kernels incl. the
 *        double-buffered and > 32-window passes), "msd_group" (arbitrary window lists), "msd_comb_global" /
 *        "msd_global" (series too long for LDS), "msd_direct", "msd_com" (amof_msd_com_dev alone)
 *   Van Hove "msd_vanhove" (u32 counters in LDS, lag tiles), "msd_vanhove_global" (u64 counters in global memory: more than
 *        AMOF_MAX_LDS_BINS bins, or AMOF_VANHOVE_GLOBAL=1)
 *   VACF "vacf_lds" (every lag from 0, origin stride 1: a column and a zero tail in LDS, consecutive lags per lane),
 *        "vacf_general" (a thread per block of atoms and lag on the columns in device memory: any window list, any origin
 *        stride, series beyond the LDS; also AMOF_VACF_GENERAL=1)
 *   S(q) "sq" (counters in LDS), "sq_bin_global" (counters in global memory: (P + 1) nbins beyond the LDS budget, or
 *        AMOF_SQ_GLOBAL=1), "sq_modes" (amof_sq_modes)
 *   distinct Van Hove "rdf_distinct_tile" (constant diagonal cell, all axes periodic, one image in reach: quantised frames,
 *        guarded f32 candidates), "rdf_distinct_exact" (canonical float64 arithmetic per pair, any cell; also
 *        AMOF_VANHOVE_DISTINCT_EXACT=1), "rdf_distinct_exact_global" (the same with u64 counters in global memory: S nbins
 *        beyond AMOF_MAX_LDS_BINS, or AMOF_VANHOVE_DISTINCT_GLOBAL=1)
 *   F(q, t) "isf" (per-lag counter tiles in LDS), "isf_global" (u64 counters in global memory: (1 + S^2) nbins counters
 *        beyond the LDS budget, or AMOF_ISF_GLOBAL=1)
 *   bond survival "bond_series" (constant diagonal cell, all axes periodic: f32 distance of the fixed-point differences,
 *        the guard band re-decided exactly), "bond_series_exact" (canonical float64 arithmetic per pair and frame: general
 *        and per-frame cells, open axes; also AMOF_BOND_EXACT=1)
 *   bond reorientation "bond_reorient" (the bond indicator decided as "bond_series"), "bond_reorient_exact" (as
 *        "bond_series_exact"); the bond vectors are the canonical float64 ones on both
 *   Lindemann index "lindemann_chunk" (a lane per pair, block and chunk of 64 frames, the partial sums added in chunk order by
 *        a second kernel), "lindemann_simple" (a lane per pair and block walks every frame; AMOF_LINDEMANN_SIMPLE=1)
 *   bond order "order_frame" (the neighbour rows of BAD's frame tier: whole frames or z-slabs in LDS), "order_exact"
 *        (canonical float64 arithmetic per pair: general and per-frame cells, open axes, centres with 17 .. 64
 *        neighbours; also AMOF_ORDER_EXACT=1)
 *   ring statistics "ring_wave" (a wave per source: level row and path stacks in LDS, a candidate per lane), "ring_simple" (a
 *        thread per source, private stacks, no LDS, no candidate buffer; AMOF_RING_SIMPLE=1)
 *   fragments "fragment_frame" (a workgroup per frame, both generations of the label / shift records in LDS, a round per
 *        barrier), "fragment_global" (a launch per round over the atoms of the batch, the records in device memory:
 *        AMOF_FRAGMENT_GLOBAL=1, or 16 N bytes of records beyond the LDS of a CU)
 *   pore field "pore_brick" (bricks of grid points against a cell list, float32 candidates, the near-minimal atoms
 *        re-evaluated in canonical float64), "pore_exact" (every atom per grid point in canonical float64: open axes,
 *        bricks too coarse for the cutoff or too full; also AMOF_PORE_EXACT=1)
 *   pore labelling (amof_pore_access, amof_pore_access_field) "pore_label_tile" (tiles labelled in LDS, tile faces merged in
 *        device memory), "pore_label_global" (every link merged in device memory; AMOF_PORE_LABEL_GLOBAL=1)
 *   pore covering (amof_pore_psd, amof_pore_psd_field) "pore_cover_brick" (bricks of grid points gather the centres whose
 *        sphere reaches them from the source bricks within reach), "pore_cover_exact" (every offset within reach per grid
 *        point: a brick's list too short, a reach of too many bricks; also AMOF_PORE_COVER_EXACT=1)
 *   pore surface (amof_pore_surface) "pore_surface_list" (a wave per atom against its neighbour list, float32 compares, the
 *        guard band re-decided in canonical float64), "pore_surface_exact" (every atom per sample in canonical float64: open
 *        axes, a list too short; also AMOF_PORE_SURFACE_EXACT=1) */
const char *amof_last_path(const amof_ctx *ctx);

/*
 * RDF histogram accumulation.
 * Replaces asap3.analysis.rdf.RadialDistributionFunction(atoms, rMax, nBins)
 * + .update() per frame, as driven by amof/rdf.py:88-93 (and :181-185).
 *   hist[(a*S + b)*nbins + k] += number of ORDERED pairs (i of species a,
 *       j of species b, any periodic image, zero-shift self pair excluded)
 *       with bin k = (int)(r / (rmax/nbins)), r < rmax
 *   *volume_sum += sum over frames of the cell volume (asap3 keeps it for
 *       the normalisation done by get_rdf, amof/rdf.py:96,109)
 * The total histogram is the sum over (a,b).  hist is accumulated into
 * (+=), so the caller zeroes it first.
 */
int amof_rdf_accumulate(amof_ctx *ctx, const amof_traj *traj, double rmax, int32_t nbins,
                        uint64_t *hist /* host [S*S][nbins] */, double *volume_sum);
int amof_rdf_accumulate_dev(amof_ctx *ctx, const amof_traj *traj, double rmax, int32_t nbins,
                            uint64_t *hist_dev /* device [S*S][nbins] */, double *volume_sum);

/*
 * Coordination-number counts.
 * Replaces amof.atom.get_neighborlist (amof/atom.py:72-87, i.e.
 * ase.neighborlist.neighbor_list('ij', atoms, {(Z1,Z2): rc})) + the counting
 * loop of amof/cn.py:67-73.
 *   cutoff[a*S + b]: per-species-pair cutoff (symmetric); 0 = never neighbours.
 *       Neighbour test is strict: sqrt(d2) < rc, every periodic image counts.
 *   sets[s] = (A, B): sums[f*n_sets + s] = sum over atoms i of species A of
 *       the number of neighbours of species B (the mean is sums / N_A).
 *   per_atom (optional, may be NULL) [F][n_sets][N]: that count per atom,
 *       -1 where the atom is not of species A.
 */
int amof_cn_count(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S] */,
                  const int32_t *sets /* [n_sets][2] */, int32_t n_sets,
                  int64_t *sums /* host [F][n_sets] */, int32_t *per_atom /* host or NULL */);

/*
 * Bond-angle histograms.
 * Replaces amof.atom.get_neighborlist + ase.Atoms.get_angles(idx, mic=True) +
 * numpy.histogram(bins=edges) as driven by amof/bad.py:70-114,154-160.
 *   triples[t] = (A, B): centre species A, neighbour species B; -1 = "X" (any).
 *   edges[nb+1]: histogram edges in degrees (host builds arange(bins+2)*dtheta,
 *       amof/bad.py:143); bin k holds edges[k] <= x < edges[k+1], last bin
 *       right-closed, values outside are dropped (numpy.histogram).
 *   hist[t*nb + k] += counts;  n_angles[t] += number of angles found
 * Returns AMOF_EANGLE for a zero-length bond vector (ASE: ZeroDivisionError).
 */
int amof_bad_hist(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S] */,
                  const int32_t *triples /* [T][2] */, int32_t n_triples,
                  const double *edges /* [nb+1] */, int32_t nb,
                  uint64_t *hist /* host [T][nb] */, uint64_t *n_angles /* host [T] */);
int amof_bad_hist_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff,
                      const int32_t *triples, int32_t n_triples, const double *edges, int32_t nb,
                      uint64_t *hist_dev /* device [T][nb] */, uint64_t *n_angles_dev /* device [T] */);

/*
 * Bond-angle histograms split by the centre atom's number of B-neighbours.
 * Replaces BadByCn.bad_BAB (amof/bad.py:190-224): slot c (0..cn_max) of triple t holds the
 * angles of centres with exactly c B-neighbours (c = cn_max also collects any larger count;
 * 1 <= cn_max <= 65535).  hist[(t*(cn_max+1) + c)*nb + k], n_angles[t*(cn_max+1) + c].
 */
int amof_bad_hist_by_cn(amof_ctx *ctx, const amof_traj *traj, const double *cutoff,
                        const int32_t *triples, int32_t n_triples, const double *edges, int32_t nb,
                        int32_t cn_max, uint64_t *hist, uint64_t *n_angles);

/*
 * Window-averaged MSD partial sums.
 * Replaces amof.trajectory.get_delta_pos (amof/trajectory.py:285-303, i.e.
 * ase.geometry.wrap_positions(d, cell[k], center=0)) + the per-window loop
 * WindowMsd.compute_msd_of_m (amof/msd.py:185-205) + the centre-of-mass
 * removal and optional unwrap of amof/msd.py:222-237.
 *   windows[w] = m (frames); 0 <= m < F
 *   sumsq[s*W + w] = sum over atoms i of species s in [atom_begin, atom_end)
 *                    of sum_{k=1}^{F-m-1} |u_i(k+m) - u_i(k)|^2
 *       where u_i is the running sum of wrapped frame-to-frame displacements.
 *       (The reference never evaluates time origin k=0 and divides by F-m:
 *        MSD_s(m) = sumsq / N_s / (F-m); the host applies it.)
 *   unwrap != 0: rebuild unwrapped positions first (amof/msd.py:222-230).
 *   remove_com != 0: subtract the mass-weighted centre of mass of ALL atoms
 *       per frame (amof/msd.py:235-237; always on in the reference).
 * [atom_begin, atom_end) lets several devices split the atoms; partial sums
 * add up exactly like the full call up to float64 summation order.
 */
int amof_msd_window(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                    int32_t unwrap, int32_t remove_com, int64_t atom_begin, int64_t atom_end,
                    double *sumsq /* host [S][W] */);
/*
 * The same with the sums ADDED into a device buffer (it stays in HBM for the ranks' all-reduce) and, optionally, the
 * per-frame centre of mass handed in (com_dev: device [F][3], NULL = computed here from all atoms; not with unwrap).
 * amof_msd_com_dev writes rows [frame_begin, frame_end) of that table -- masses @ positions / masses.sum() per frame
 * (ase get_center_of_mass, amof/msd.py:235-237) -- and leaves the others alone: the ranks of an atom-sharded run
 * each compute the centre of mass of their FRAME share into a zeroed table and sum the tables (x + 0 = x: exact),
 * instead of every rank reading every frame.  The element-parallel split this stands in for: amof/msd.py:252-256.
 */
int amof_msd_window_dev(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                        int32_t unwrap, int32_t remove_com, int64_t atom_begin, int64_t atom_end,
                        const double *com_dev /* device [F][3] or NULL */, double *sumsq_dev /* device [S][W], += */);
int amof_msd_com_dev(amof_ctx *ctx, const amof_traj *traj, int64_t frame_begin, int64_t frame_end,
                     double *com_dev /* device [F][3] */);

/*
 * Atom-sharded window MSD around ONE all-reduce (one process per GPU; the element-parallel split this stands in for:
 * amof/msd.py:252-256).  Every rank holds the whole device-resident trajectory and owns the atoms [atom_begin, atom_end):
 *   amof_msd_shard_begin  reads ITS atoms once: csum_dev[F][3] (device, overwritten) = sum over its atoms of m_a p_a(k),
 *                         its share of the centre of mass of every frame (amof/msd.py:235-237), and keeps the segment
 *                         sums of its atoms' wrapped displacements in the context's scratch;
 *   the caller sums csum_dev over the ranks (one all-reduce of 24 F bytes);
 *   amof_msd_shard_finish reads its atoms a second time and ADDS their sums of squared displacements (amof_msd_window's
 *                         definition) into sumsq_dev[S][W] (device), which the caller all-reduces next.
 * finish must be the next call on the context after its begin, with the same arguments.  begin returns AMOF_EUNSUPPORTED
 * (nothing done) where this form does not apply -- general (non-diagonal) cells, host positions, windows that are not
 * w * d (16 <= d, W <= 32) -- and the caller then uses amof_msd_com_dev + amof_msd_window_dev.
 */
int amof_msd_shard_begin(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                         int64_t atom_begin, int64_t atom_end, double *csum_dev /* device [F][3] */);
int amof_msd_shard_finish(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                          int64_t atom_begin, int64_t atom_end, const double *csum_dev /* device [F][3], summed over the ranks */,
                          double *sumsq_dev /* device [S][W], += */);

/*
 * Self Van Hove function and the moments of the non-Gaussian parameter (window form).
 * Replaces nothing the reference computes: the same displacements as amof_msd_window (amof.trajectory.get_delta_pos,
 * amof/trajectory.py:285-303; the centre-of-mass removal and optional unwrap of amof/msd.py:222-237; the time origins
 * k = 1 .. F-m-1 that WindowMsd.compute_msd_of_m visits, amof/msd.py:185-205), binned instead of summed.
 *   u_i(k): the running sum of wrapped frame-to-frame displacements, as amof_msd_window defines it.
 *   one sample per atom i of [atom_begin, atom_end), window m = windows[w] and origin k = 1 .. F-m-1:
 *       D = u_i(k+m) - u_i(k),  r2 = (Dx*Dx + Dy*Dy) + Dz*Dz (float64, no fma),  r = sqrt(r2) (correctly rounded)
 *       bin b = (int)(r / dr); b >= nbins goes to overflow.  n_s(m) = N_s (F-m-1) samples per species and window.
 *   counts[(s*W + w)*nbins + b]   samples of species s (library order) at window w in bin b
 *   overflow[s*W + w]             samples with b >= nbins
 *   moments[(s*W + w)*2 + 0] = sum of r2,  [.. + 1] = sum of r2*r2 -- over every sample, overflow included
 *       (sum of r2 is amof_msd_window's sumsq up to float64 rounding; the alpha_2 of the host is
 *        3 n sum4 / (5 sum2^2) - 1).  Two identical calls give identical bits: fixed-order reductions, integer atomics.
 *   unwrap, remove_com, atom_begin, atom_end: as amof_msd_window.  dr > 0, nbins >= 0 (no capacity limit on nbins, W,
 *   F or N: histograms beyond the LDS take the global-counter kernel).
 * The host form overwrites its outputs.  Errors: AMOF_EINVAL (bad window, range, dr, nbins, NULL argument),
 * AMOF_ENOMEM, AMOF_EHIP, AMOF_ENODEVICE.
 */
int amof_vanhove_window(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows, int32_t unwrap,
                        int32_t remove_com, int64_t atom_begin, int64_t atom_end, double dr, int32_t nbins,
                        uint64_t *counts /* host [S][W][nbins] */, uint64_t *overflow /* host [S][W] */,
                        double *moments /* host [S][W][2] */);
/* The same with the results ADDED into device buffers (atom-sharded ranks all-reduce them next) and, optionally, the
 * per-frame centre of mass handed in (com_dev: device [F][3] from amof_msd_com_dev, NULL = computed here; not with unwrap). */
int amof_vanhove_window_dev(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows, int32_t unwrap,
                            int32_t remove_com, int64_t atom_begin, int64_t atom_end, double dr, int32_t nbins,
                            const double *com_dev /* device [F][3] or NULL */, uint64_t *counts_dev /* device [S][W][nbins], += */,
                            uint64_t *overflow_dev /* device [S][W], += */, double *moments_dev /* device [S][W][2], += */);

/*
 * Velocity autocorrelation sums (window form).
 * Replaces nothing the reference computes (the reference has no velocity analysis).
 *   Samples x_ic(k), coordinate c of atom i:
 *     velocity_mode == 0: the wrapped step of atom i from frame k - 1 to frame k, k = 1 .. F - 1, exactly as amof_msd_window
 *       forms it without unwrap (the earlier frame's cell; remove_com as there).  The caller divides by the timestep.
 *     velocity_mode != 0: traj's "positions" are velocities; x(k) = frame k's value minus, with remove_com, the mass-weighted
 *       mean of the frame over ALL atoms.  No wrap; the cell is ignored.
 *   Lags m = windows[w] and their origins k = 1, 1 + s, ... <= F - m - 1 (s = origin_stride >= 1): amof_vanhove_distinct's rule
 *   (stated there); sample 0 is never used.
 *     sums[s*W + w] = sum over atoms i of species s in [atom_begin, atom_end), c and the origins k of lag w of
 *                     x_ic(k) * x_ic(k + m)
 *   Order of summation: the atoms of a species in blocks of 8 (in atom order), one accumulator per block and lag updated with
 *   fma over the block's columns (atom, then c) and k ascending; the blocks of a species added in order.  No float atomics: two
 *   identical calls give identical bits, and so do the two kernels ("vacf_lds", "vacf_general": amof_last_path).
 *   amof_last_kernel_seconds: which = 2 the columns, 3 the correlation with its reduction.
 * The host form overwrites sums.  Errors: AMOF_EINVAL (bad window, stride, range, NULL argument), AMOF_ENOMEM, AMOF_EHIP,
 * AMOF_ENODEVICE.
 */
int amof_vacf_window(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows /* host [W] */, int32_t n_windows,
                     int64_t origin_stride, int32_t velocity_mode, int32_t remove_com, int64_t atom_begin, int64_t atom_end,
                     double *sums /* host [S][W] */);
/* The same with the sums ADDED into a device buffer (atom-sharded ranks all-reduce it next) and, optionally, the per-frame
 * centre of mass -- in velocity mode the per-frame mean velocity -- handed in (com_dev: device [F][3] from amof_msd_com_dev,
 * NULL = computed here from all atoms). */
int amof_vacf_window_dev(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                         int64_t origin_stride, int32_t velocity_mode, int32_t remove_com, int64_t atom_begin, int64_t atom_end,
                         const double *com_dev /* device [F][3] or NULL */, double *sums_dev /* device [S][W], += */);

/*
 * Distinct Van Hove function: pair-distance histograms between two frames of a trajectory.
 * Replaces nothing the reference computes (the reference has no dynamic pair analysis).
 *   Lags m = windows[w] (0 <= m < F), origins k = 1, 1 + s, 1 + 2s, ... <= F - m - 1 (s = origin_stride >= 1); the work
 *   list is every (w, k) in lag-major order (w, then k), n_w = floor((F - m - 2) / s) + 1 entries for lag w (0 if m > F - 2).
 *   A call handles the entries [work_begin, work_end) of that list: ranges add up bit for bit.
 *   For every entry and every ordered pair (i, j), i != j: d0 = r_j(k + m) - r_i(k) on the raw float64 positions, the
 *   canonical minimum image with frame k's cell and pbc (pair_base, plus every further image in reach of
 *   rmax), counted iff d2 < rmax^2 and b = (int)(sqrt(d2) / (rmax / nbins)) < nbins:
 *     hist[((a*S + c)*W + w)*nbins + b] += 1,  a = species of i (the centre, at the origin), c = species of j (at k + m),
 *     library species order.  At m = 0 the counts are the RDF's (amof_rdf_accumulate) over the same frames.
 *   No centre-of-mass removal, no unwrap: pair distances are periodic.  rmax > 0, nbins >= 1.
 * The host form overwrites hist.  Errors: AMOF_EINVAL (bad window, stride, work range, rmax, nbins, NULL argument),
 * AMOF_ENOMEM, AMOF_EHIP, AMOF_ENODEVICE.
 */
int amof_vanhove_distinct(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows /* host [W] */, int32_t n_windows,
                          int64_t origin_stride, int64_t work_begin, int64_t work_end, double rmax, int32_t nbins,
                          uint64_t *hist /* host [S][S][W][nbins] */);
/* The same with the counts ADDED into a device buffer (ranks that share the work list all-reduce it next). */
int amof_vanhove_distinct_dev(amof_ctx *ctx, const amof_traj *traj, const int32_t *windows, int32_t n_windows,
                              int64_t origin_stride, int64_t work_begin, int64_t work_end, double rmax, int32_t nbins,
                              uint64_t *hist_dev /* device [S][S][W][nbins], += */);

/*
 * Bond survival correlations: does the SAME pair stay bonded?
 * Replaces the per-frame neighbour-list loop a user writes around amof.atom.get_neighborlist (amof/atom.py:72-87; the
 * search amof/cn.py:65 profiles at "92 % of computation time") to follow individual bonds through a trajectory; the
 * reference itself has no dynamic neighbour analysis.
 *   cutoff, sets: as amof_cn_count.  h_ij(f) = 1 iff atom j (species B) is a neighbour of atom i (species A), i != j, in
 *   frame f -- amof_cn_count's decision for that frame, pair and cutoff: strict sqrt(d2) < rc on the canonical minimum
 *   image in frame f's cell and pbc.  For h to be 0 or 1, a cutoff of a set above half the smallest
 *   perpendicular cell height over all frames on a periodic axis is refused (AMOF_EINVAL).
 *   Lags m = windows[w] and their origins (s = origin_stride >= 1): amof_vanhove_distinct's (stated there).
 *   Per set s and lag w, summed over the lag's origins k and the ordered pairs (i, j) with atom_begin <= i < atom_end:
 *     counts[(s*W + w)*3 + 0] = sum h_ij(k)                              bonds present at the origins
 *     counts[(s*W + w)*3 + 1] = sum h_ij(k) h_ij(k + m)                  intermittent: bonded at both ends
 *     counts[(s*W + w)*3 + 2] = sum prod_{f = k .. k + m} h_ij(f)        continuous: bonded at EVERY frame from k to k + m
 *   The host forms C(t) = [1] / [0] and S(t) = [2] / [0].  counts[(s*W + w)*3] of a lag m = 0 is amof_cn_count's sums[f][s]
 *   added over the frames f = 1, 1 + s, ... <= F - 1.  Integer counters: ranges of centres add up bit for bit, and the
 *   result does not depend on launch order or on how the library chunks pairs, centres and lags.
 *   No capacity limit on the number of pairs, F, W or N: scratch is bounded -- a piece of centres (bitmap <= 256 MB), inside
 *   it groups of centres of at most 2^25 pairs (pair table <= 256 MB; AMOF_BOND_PAIR_BUDGET, in pairs, overrides), a chunk of
 *   pairs (series words <= 256 MB) and 2048 lags at a time.  amof_last_kernel_seconds: which = 2 the bond lists of the origin frames, 3 the bit series, 4 the
 *   correlations; 1 spans the series launches.
 * The host form overwrites counts.  Errors: AMOF_EINVAL (bad window, stride, atom range, set, cutoff, NULL argument),
 * AMOF_ESINGULAR, AMOF_ENOMEM, AMOF_EHIP, AMOF_ENODEVICE.
 */
int amof_bond_survival(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], as amof_cn_count */,
                       const int32_t *sets /* [n_sets][2] */, int32_t n_sets, const int32_t *windows /* host [W] */,
                       int32_t n_windows, int64_t origin_stride, int64_t atom_begin, int64_t atom_end,
                       uint64_t *counts /* host [n_sets][W][3] */);
/* The same with the counters ADDED into a device buffer (ranks that share the centres all-reduce it next). */
int amof_bond_survival_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                           const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t atom_begin,
                           int64_t atom_end, uint64_t *counts_dev /* device [n_sets][W][3], += */);

/*
 * Bond reorientation: first- and second-rank correlations C_l(t) = <P_l(u(0) . u(t))> of the bond vectors.
 * Replaces the same per-frame neighbour-list loop (amof/cn.py:65) with a minimum-image call per pair.
 *   Arguments, bond indicator h_ij(f), lags, origins, the refusal of a cutoff above half the smallest height: as
 *   amof_bond_survival.  d_ij(f): the canonical float64 minimum-image vector r_j - r_i in frame f's cell, on every
 *   path.  With dot(a, b) = fma(az, bz, fma(ay, by, ax bx)):
 *     cos = dot(d(k), d(k + m)) / sqrt(dot(d(k), d(k)) * dot(d(k + m), d(k + m))), clamped to [-1, 1]
 *     P1 = cos,  P2 = fma(1.5 cos, cos, -0.5)              (a lag of 0 gives cos = P1 = P2 = 1 exactly)
 *   Per set s and lag w, summed over the lag's origins k and the ordered pairs (i, j) with atom_begin <= i < atom_end:
 *     out[(s*W + w)*3 + 0] = sum h(k) h(k + m)                             (amof_bond_survival's counts[..][1], bit for bit)
 *     out[(s*W + w)*3 + 1] = sum h(k) h(k + m) rint(P1 2^e_s)              int64, two's complement
 *     out[(s*W + w)*3 + 2] = sum h(k) h(k + m) rint(P2 2^e_s)
 *   scale_log2[s] = e_s = min(40, 62 - bit_length(n_A n_B n_0)), n_A and n_B the atoms of the set's species in the whole
 *   trajectory, n_0 the origins of lag 0: it depends on the trajectory, the set and the stride only.  e_s < 20 is refused
 *   (AMOF_EINVAL).  The host forms C_l(t) = out[l] 2^-e_s / out[0].  Integer sums: ranges of centres add up bit for bit, and
 *   the result does not depend on launch order, chunking or the path.
 *   A contributing term with a zero-length vector returns AMOF_EANGLE; the host form's out holds zeros then, the _dev form's
 *   buffer is untouched.
 *   Scratch as amof_bond_survival, plus the vector table of a chunk of pairs (<= 256 MB, 64 pairs at least).
 *   amof_last_kernel_seconds: which = 2 the bond lists, 3 the bit series, 4 the vector table and the sums.
 * The host form overwrites out.  Errors: amof_bond_survival's, and AMOF_EANGLE.
 */
int amof_bond_reorientation(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], as amof_cn_count */,
                            const int32_t *sets /* [n_sets][2] */, int32_t n_sets, const int32_t *windows /* host [W] */,
                            int32_t n_windows, int64_t origin_stride, int64_t atom_begin, int64_t atom_end,
                            int64_t *out /* host [n_sets][W][3] */, int32_t *scale_log2 /* host [n_sets] */);
/* The same with the sums ADDED into a device buffer (ranks that share the centres all-reduce it next). */
int amof_bond_reorientation_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                                const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t atom_begin,
                                int64_t atom_end, int64_t *out_dev /* device [n_sets][W][3], += */,
                                int32_t *scale_log2 /* host [n_sets] */);

/*
 * Lindemann index: how much does the LENGTH of a neighbour pair fluctuate?  delta = sqrt(<d^2> - <d>^2) / <d> per pair, over
 * blocks of frames: the melting criterion (a glass stays below about 0.1, a liquid does not).  Replaces nothing in the
 * reference, whose neighbour analyses (amof/cn.py) count bonds per frame and follow no pair through time.
 *   Blocks.  F frames, a block length B = block (2 <= B <= F) and a block stride S = block_stride >= 1 give
 *     nb = (F - B) / S + 1 blocks (integer division); block b covers the frames [b S, b S + B).  Frame 0 is used: this is no
 *     lag analysis, and the origin rule of the lag family (origins from frame 1) does not apply.  Frames behind the last block
 *     are not used.
 *   cutoff, sets, h_ij(f): amof_cn_count's and amof_bond_survival's -- strict sqrt(d2) < rc on the canonical minimum image
 *      in frame f's cell and pbc, decided by the canonical float64 arithmetic (one decision per pair and block: there
 *     is no f32 form).  A cutoff of a set above half the smallest perpendicular cell height on a periodic axis is refused
 *     (AMOF_EINVAL), as for amof_bond_survival; a zero cutoff gives an empty set.
 *   Pairs of a block: the ordered pairs (i of species A, j of species B, i != j, atom_begin <= i < atom_end) with
 *     select = 0 ("block")  h_ij(b S) = 1: the bonds that exist at the block's first frame;
 *     select = 1 ("first")  h_ij(0) = 1, in every block: a fixed population, whose delta keeps growing as the initial network
 *                           dissolves.
 *   Distance.  d_ij(f) = sqrt(norm2(pair_base(r_j - r_i))): the canonical minimum-image distance in frame f's own cell and pbc.
 *     A pair that drifts beyond half the cell is measured to its nearest image: delta of such a pair only means "large".
 *   Moments, in a fixed order.  With c = d(first frame of the block) and e_f = d_f - c:
 *     chunks of 64 block-relative frames [64 k, 64 k + 64); inside a chunk, frames ascending from p1 = p2 = 0:
 *       p1 += e,  p2 = fma(e, e, p2);
 *     S1, S2 = the chunk partials added in ascending k, from 0;
 *     m1 = S1 / B,  mean = c + m1,  var = max(0, S2 / B - m1 * m1),  delta = var == 0 ? 0 : sqrt(var) / mean.
 *     This order is part of the ABI: every kernel and every launch geometry gives the same bits.
 *   Outputs, all integers:
 *     sums[(b*n_sets + s)*2 + 0] = number of pairs of block b and set s
 *     sums[(b*n_sets + s)*2 + 1] = sum over them of llrint(delta_ij 2^e_s)                      int64
 *     scale_log2[s] = e_s = min(40, 62 - bit_length(n_A n_B ceil(sqrt(B)))), n_A and n_B the atoms of the set's species in the
 *       whole trajectory (the coefficient of variation of B non-negative numbers is at most sqrt(B - 1)): it depends on the
 *       trajectory, the set and B only.  e_s < 20 is refused (AMOF_EINVAL).
 *     hist[(b*n_sets + s)*nbins + k]: pairs with k = min((int)(delta / ddelta), nbins - 1); the last bin takes everything above
 *     per_atom (optional, may be NULL) int64 [nb][n_sets][N][2]: the pairs of centre i and their sum of llrint(delta_ij 2^e_s);
 *       zero rows where the atom has no pair
 *     Ranges of centres add up bit for bit, and nothing depends on launch order, on how the library chunks pairs, centres,
 *     blocks and frames, or on the path.
 *   Paths (amof_last_path): "lindemann_chunk" -- a lane per (pair, block, chunk of 64 frames) writes the chunk's partial sums,
 *     a second kernel adds them in chunk order; "lindemann_simple" (AMOF_LINDEMANN_SIMPLE=1) -- a lane per (pair, block) walks
 *     every frame in the same order: the cross-check inside the binary.  Scratch is bounded: the pair table as
 *     amof_bond_survival's (AMOF_BOND_PAIR_BUDGET), the partial sums of a chunk of pairs and blocks <= 256 MB
 *     (64 pairs and one block at least).
 *   amof_last_kernel_seconds: which = 2 the pair lists, 3 the moments, 4 the reduction; 1 spans the moments launches.
 * The host form overwrites sums, hist and per_atom (zeros after an error).  The _dev form ADDS sums and hist into device
 * buffers (ranks that share the centres all-reduce them next; untouched after an error); per_atom and scale_log2 stay host
 * arrays.  Errors: AMOF_EINVAL (block, block_stride, select, nbins, ddelta, atom range, set, cutoff, NULL argument),
 * AMOF_ESINGULAR, AMOF_ENOMEM, AMOF_EHIP, AMOF_ENODEVICE.
 */
int amof_lindemann(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], as amof_cn_count */,
                   const int32_t *sets /* [n_sets][2] */, int32_t n_sets, int64_t block, int64_t block_stride, int32_t select,
                   int32_t nbins, double ddelta, int64_t atom_begin, int64_t atom_end, int64_t *sums /* host [nb][n_sets][2] */,
                   uint64_t *hist /* host [nb][n_sets][nbins] */, int64_t *per_atom /* host [nb][n_sets][N][2] or NULL */,
                   int32_t *scale_log2 /* host [n_sets] */);
int amof_lindemann_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets, int64_t block,
                       int64_t block_stride, int32_t select, int32_t nbins, double ddelta, int64_t atom_begin, int64_t atom_end,
                       int64_t *sums_dev /* device [nb][n_sets][2], += */, uint64_t *hist_dev /* device [nb][n_sets][nbins], += */,
                       int64_t *per_atom /* host or NULL */, int32_t *scale_log2 /* host [n_sets] */);

/*
 * Bond order parameters of neighbour shells: Steinhardt q_l and the tetrahedral order parameter q_tet per centre atom.
 * Replaces nothing in the reference (it stops at bond counts and angle histograms, amof/cn.py, amof/bad.py); both are
 * non-linear functions of ALL the angles of one centre, which a histogram of angles cannot give.
 *   cutoff, sets: as amof_cn_count, and so is the neighbour decision: strict sqrt(d2) < rc on the canonical minimum image.
 *   As amof_bond_survival, a cutoff of a set above half the smallest perpendicular cell height on a periodic axis is
 *   refused (AMOF_EINVAL): a neighbour is then one image, and n is amof_cn_count's per-atom count.
 *   Centre i (species A) with n neighbours of species B: u_1 .. u_n = v / sqrt(vx vx + vy vy + vz vz) of the canonical
 *   minimum-image vectors (as BAD; a zero-length vector returns AMOF_EANGLE).  For every unordered pair j < k:
 *     c = ux*vx + uy*vy + uz*vz, clipped to [-1, 1]                   (BAD's expression and operation order, no fma)
 *     P_m(c) by the Bonnet recurrence in float64: p0 = 1, p1 = c,
 *         p_{m+1} = (((double)(2m+1) * c) * p_m - (double)m * p_{m-1}) / (double)(m+1)
 *     with E = 40:  T_l(i) = sum_{j<k} llrint(P_l(c) * 2^E)                                  (int64)
 *                   U(i)   = sum_{j<k} llrint((c + 1.0/3.0) * (c + 1.0/3.0) * 2^E)           (used when n == 4)
 *   By the addition theorem of the spherical harmonics q_l^2 = (n + 2 sum_{j<k} P_l(cos theta_jk)) / n^2, so
 *     Q_l = max(0, n*2^E + 2*T_l),  q_l = sqrt(ldexp((double)Q_l, -E)) / (double)n          n >= 1 (n = 1: exactly 1)
 *     q_tet = 1.0 - 0.375 * ldexp((double)U, -E)                                             n == 4 only; in [-3, 1]
 *   A centre with more than 64 neighbours returns AMOF_ECAPACITY; up to 64, Q_l < 2^53 converts exactly.
 *   l[n_l]: 1 <= n_l <= 4 values, each in 1 .. 12.
 *   Bins: q_l:   b = min((int)(q_l * (double)nbins), nbins - 1)
 *         q_tet: b = min((int)((q_tet + 3.0) * 0.25 * (double)nbins_tet), nbins_tet - 1)     (last bin right-closed: q = 1 counts)
 *   Outputs, over the frames of the call:
 *     hist [n_sets][n_l][nbins]: centres with n >= 1;  hist_tet [n_sets][nbins_tet]: centres with n == 4
 *     frame_sums int64 [F][n_sets][4 + n_l + 1]: sum of n (amof_cn_count's sums[f][s], bit for bit), centres with n >= 1,
 *       centres with n == 4, sum of n (n - 1) / 2 (amof_bad_hist's n_angles of the triple B-A-B over the same frames),
 *       sum of llrint(q_l * 2^30) per l, sum of llrint(q_tet * 2^30)
 *     per_atom (optional, may be NULL) int64 [F][n_sets][N][2 + n_l]: (n, T_l ..., U); n = -1 where the atom is not of species A
 *   All outputs are integers: frame ranges concatenate / add up bit for bit, and nothing depends on launch geometry,
 *   batching or the path ("order_frame": the neighbour rows of BAD's frame tier; "order_exact": canonical float64
 *   arithmetic per pair, any cell, up to 64 neighbours; AMOF_ORDER_EXACT=1 forces it; AMOF_ORDER_ROWS_MB=n caps
 *   the scratch of the neighbour rows -- more, smaller frame batches; 0: one frame per batch).
 *   amof_last_kernel_seconds: which = 2 the list stage, 3 the order kernels.
 * The host form overwrites hist, hist_tet, frame_sums and per_atom (zeros after an error).  The _dev form ADDS hist and
 * hist_tet into device buffers (frame-sharded ranks all-reduce them next); frame_sums and per_atom stay host buffers, as
 * amof_cn_count's sums.  Errors: AMOF_EINVAL, AMOF_EANGLE, AMOF_ECAPACITY, AMOF_ESINGULAR, AMOF_ENOMEM, AMOF_EHIP.
 */
int amof_bond_order(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], as amof_cn_count */,
                    const int32_t *sets /* [n_sets][2] */, int32_t n_sets, const int32_t *l /* host [n_l] */, int32_t n_l,
                    int32_t nbins, int32_t nbins_tet, uint64_t *hist /* host [n_sets][n_l][nbins] */,
                    uint64_t *hist_tet /* host [n_sets][nbins_tet] */, int64_t *frame_sums /* host [F][n_sets][4 + n_l + 1] */,
                    int64_t *per_atom /* host [F][n_sets][N][2 + n_l] or NULL */);
int amof_bond_order_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *sets, int32_t n_sets,
                        const int32_t *l, int32_t n_l, int32_t nbins, int32_t nbins_tet,
                        uint64_t *hist_dev /* device [n_sets][n_l][nbins], += */,
                        uint64_t *hist_tet_dev /* device [n_sets][nbins_tet], += */, int64_t *frame_sums /* host */,
                        int64_t *per_atom /* host or NULL */);

/*
 * Dihedral (torsion) angle distributions of chains a-b-c-d of bonded atoms.
 * Replaces nothing in the reference (its static analyses stop at three bodies: amof/rdf.py, amof/bad.py); the angle AROUND a
 * bond is what the rotation of a linker about its Zn-N bond, the planarity of a ring and the conformation of a chain are.
 *   Bond graph: i != j are bonded iff j is a neighbour of i by amof_cn_count's decision -- the canonical minimum image, strict
 *   sqrt(d2) < rc with rc = cutoff[species i][species j] (symmetric; 0 = never bonded): the graph of amof_ring_stats, whatever
 *   the patterns name.  As amof_bond_order, a cutoff above half the smallest perpendicular cell height on a periodic axis is
 *   refused (AMOF_EINVAL): a neighbour is one image.  An atom with more than 16 neighbours returns AMOF_ECAPACITY (the message
 *   names the frame), a bonded pair of coincident atoms AMOF_EANGLE (as amof_bad_hist).
 *   Chains: an unordered central bond {b, c}, a neighbour a of b and a neighbour d of c, with a != c, d != b and a != d BY ATOM
 *   INDEX (the quotient-graph convention of amof_ring_stats: three-membered rings are dropped, and so is a chain that returns
 *   to an image of its first atom around a small cell).  Every chain is visited once, from the end with b < c.
 *   chains[t] = (A, B, C, D), species indices, -1 = any.  A chain counts ONCE for pattern t iff the pattern matches its species
 *   read as a-b-c-d or as d-c-b-a: A-B-C-D and D-C-B-A give the same column, palindromes and wildcards never count twice.
 *   1 <= n_chains <= 32.
 *   Angle: with the canonical unit vectors u1 = u(b -> a), u2 = u(b -> c), u3 = u(c -> d) -- v / sqrt(vx vx + vy vy + vz vz) of
 *   the canonical minimum-image vectors, as BAD; u(c -> b) == -u(b -> c) exactly -- in float64, no fma, in this order:
 *     n1 = u2 x u1,  n2 = u2 x u3        x = (u2y * wz) - (u2z * wy),  y = (u2z * wx) - (u2x * wz),  z = (u2x * wy) - (u2y * wx)
 *     s1 = (n1x*n1x + n1y*n1y) + n1z*n1z,  s2 = (n2x*n2x + n2y*n2y) + n2z*n2z
 *     s1 < 2^-40 or s2 < 2^-40: the chain is UNDEFINED (a bond angle within about 1e-6 rad of straight): counted, not binned
 *     c = ((n1x*n2x + n1y*n2y) + n1z*n2z) / sqrt(s1 * s2), clipped to [-1, 1]
 *     phi = (180 / pi) * acos(c) in [0, 180], acos being the fixed algorithm of amof_bad_hist (fdlibm's)
 *   The sign of the torsion is folded away (0: cis, 180: trans).
 *   Bins: edges[nb + 1], strictly increasing, used as amof_bad_hist's: bin k holds edges[k] <= phi < edges[k + 1], the last
 *   bin is right-closed.
 *   Outputs, over the frames of the call, all integers:
 *     hist [n_chains][nb]; n_dihedrals [n_chains]: the defined chains; n_undefined [n_chains]
 *     frame_sums int64 [F][n_chains][3]: the defined chains, the undefined chains, sum of llrint(c * 2^40) over the defined ones
 *       (<cos phi> of a frame and pattern = [2] / 2^40 / [0])
 *   Frame ranges concatenate / add up bit for bit, and nothing depends on launch geometry, batching or the path
 *   ("dihedral_frame": the neighbour rows of BAD's frame tier with the partner's index in every entry; "dihedral_exact": index
 *   rows of amof_ring_stats' adjacency kernel, the unit vectors recomputed, any cell; AMOF_DIHEDRAL_EXACT=1 forces it;
 *   AMOF_DIHEDRAL_ROWS_MB=n caps the scratch of the neighbour rows -- more, smaller frame batches; 0: one frame per batch).
 *   amof_last_kernel_seconds: which = 2 the list stage (the adjacency rows on "dihedral_exact"), 3 the dihedral kernels.
 * The host form overwrites hist, n_dihedrals, n_undefined and frame_sums (zeros after an error).  The _dev form ADDS hist,
 * n_dihedrals and n_undefined into device buffers (frame-sharded ranks all-reduce them next); frame_sums stays a host buffer.
 * Errors: AMOF_EINVAL, AMOF_EANGLE, AMOF_ECAPACITY, AMOF_ESINGULAR, AMOF_ENOMEM, AMOF_EHIP.
 */
int amof_dihedral_hist(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], symmetric */,
                       const int32_t *chains /* [n_chains][4] */, int32_t n_chains, const double *edges /* host [nb + 1] */,
                       int32_t nb, uint64_t *hist /* host [n_chains][nb] */, uint64_t *n_dihedrals /* host [n_chains] */,
                       uint64_t *n_undefined /* host [n_chains] */, int64_t *frame_sums /* host [F][n_chains][3] */);
int amof_dihedral_hist_dev(amof_ctx *ctx, const amof_traj *traj, const double *cutoff, const int32_t *chains, int32_t n_chains,
                           const double *edges, int32_t nb, uint64_t *hist_dev /* device [n_chains][nb], += */,
                           uint64_t *n_dihedrals_dev /* device [n_chains], += */,
                           uint64_t *n_undefined_dev /* device [n_chains], += */, int64_t *frame_sums /* host */);

/*
 * Primitive ring statistics of the bond network, per frame.
 * Replaces amof.ring.Ring (amof/ring/core.py), which writes every frame to a temporary directory and runs the external
 * program RINGS on it with growing search depth; the counts are those of its primitive rings (RINGS-res-5.dat).
 *   Graph of a frame: the N atoms; i != j are bonded iff j is a neighbour of i by amof_cn_count's decision -- the canonical
 *   minimum image, strict sqrt(d2) < rc with rc = cutoff[species i][species j] (symmetric; 0 = never bonded).  A cutoff
 *   above half the smallest perpendicular cell height on a periodic axis is refused (AMOF_EINVAL), as amof_bond_survival's:
 *   a pair then has at most one bond and the graph is simple.  It is the QUOTIENT graph of the cell: a closed path that
 *   winds around a small cell is a ring of it (RINGS does the same on a periodic box).
 *   Primitive ring (Franzblau's shortest-path ring): a simple cycle R of n >= 3 nodes with dist_G(y, z) == dist_R(y, z)
 *   for every pair of its nodes.  With K = max_size / 2, D[v][.] = the breadth-first levels from v truncated at K (u8):
 *     size 2k:      an unordered pair of shortest paths v -> w, D[v][w] = k >= 2, that share v and w only
 *     size 2k + 1:  shortest paths v -> w1 and v -> w2 of a bonded pair w1 < w2 at level k >= 1, that share v only
 *   and in both every cross pair y = P1[a], z = P2[b] has D[y][z] == min(a + b, n - a - b).  Every primitive n-ring is found
 *   once from each of its n nodes: c[v][n] = primitive n-rings through v, rings[n] = sum_v c[v][n] / n exactly.
 *   max_size: 3 .. 32.  The counts at sizes <= n1 do not depend on max_size >= n1.
 *   Outputs, over the frames of the call (the caller passes the frames of its range: a trajectory handle of them):
 *     counts int64 [F][4][max_size + 1]: [0] sum_v c[v][n], [1] nodes with c[v][n] > 0, [2] nodes whose smallest ring size
 *       is n, [3] nodes whose largest ring size is n
 *     truncated int64 [F]: sources whose search still had unvisited neighbours at level K.  0: the frame has no primitive
 *       ring of more than 2K + 1 nodes; otherwise larger rings cannot be excluded (RINGS: "potentially undiscovered")
 *     per_atom (optional, may be NULL) u32 [F][N][max_size + 1]: c[v][n]
 *     neighbours (optional, may be NULL) int32 [F][N][1 + 16]: the degree and the neighbours in ascending order, -1 behind
 *   Capacities (AMOF_ECAPACITY, the message names the limit and the frame; nothing is truncated silently): N <= 65535,
 *   at most 16 neighbours per atom, at most 1024 shortest paths from a source to an end node of a candidate
 *   (AMOF_RING_MAX_PATHS=n overrides the last, for tests).
 *   All outputs are integers and independent per frame: frame ranges concatenate bit for bit, and nothing depends on the
 *   batching (AMOF_RING_TABLE_MB=n caps the distance tables D of a batch of frames, N^2 bytes each, default 1024; 0: one
 *   frame per batch) or the path ("ring_wave"; AMOF_RING_SIMPLE=1: "ring_simple").
 *   amof_last_kernel_seconds: which = 2 the adjacency rows, 3 the breadth-first searches, 4 the ring search.
 *   amof_ring_search_stats: out[3] = sources, candidates searched, candidates that closed at least one ring, of the last call.
 * The outputs are overwritten (zeros after an error).  Errors: AMOF_EINVAL (max_size, an asymmetric, negative or oversized
 * cutoff, NULL argument), AMOF_ESINGULAR, AMOF_ECAPACITY, AMOF_ENOMEM, AMOF_EHIP.
 */
int amof_ring_stats(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], symmetric */, int32_t max_size,
                    int64_t *counts /* host [F][4][max_size + 1] */, int64_t *truncated /* host [F] */,
                    uint32_t *per_atom /* host [F][N][max_size + 1] or NULL */,
                    int32_t *neighbours /* host [F][N][1 + 16] or NULL */);
int amof_ring_search_stats(const amof_ctx *ctx, double *out /* [3] */);

/*
 * Fragments: the connected components of a bond graph under periodic boundaries, per frame, and what makes them whole.
 * Replaces the search underneath the reference's building-unit reduction (amof/coordination/reduce.py, core.py and
 * ReducedTrajectory in amof/trajectory.py: pymatgen neighbour lists and networkx components, one frame at a time); its
 * MOF-specific chemistry (zif.py) is not restated.
 *   Bond graph G: amof_ring_stats' -- i != j bonded iff sqrt(d2) < cutoff[species i][species j] on the canonical minimum
 *   image (strict; symmetric matrix; 0 = never bonded), cutoffs above half the smallest perpendicular cell height refused.
 *   Fragment: a connected component of G.  Its ROOT is its smallest atom index; label[i] = the root of i's fragment.
 *   Shift: shift[i] in Z^3 with shift[root] = 0 and, along a bond i-j, shift[j] = shift[i] + s_ij, where s_ij = -n_ij and
 *   n_ij = rint((r_j - r_i) C^-1) is the lattice vector the canonical minimum image subtracts (the same products, fma order
 *   and rint: amof_amd/csrc/fragment_math.h), so that r_j + shift[j] C is the image bonded to r_i + shift[i] C.
 *   Winding: a fragment WINDS iff a bond of it violates that relation for the shifts found; it is then periodic and has no
 *   centre.  The shifts of a fragment that does not wind do not depend on the path; those of a winding one are whatever the
 *   relabelling rounds left (the same on both kernels) and mean nothing.
 *   Centre of mass: sum m_i (r_i + shift[i] C) / sum m_i, not wrapped into the cell; int64 fixed-point sums at scale 2^40
 *   per u A (two words per component), so the summation order does not matter.  Accepted: 0 < m_i < 512 u (AMOF_EINVAL
 *   otherwise), |coordinate of a whole fragment's atom| < 65536 A (AMOF_ECAPACITY naming the frame).  For a fragment of n
 *   atoms, mass M and largest atomic mass mmax whose atoms pass through magnitudes of at most X A:
 *   |centre - exact| <= n (2^-41 + mmax X 2^-53) / M + 5 X 2^-53 A (derivation: fragment_math.h).
 *   Link bonds (optional): a second matrix `link`, the same decision; it must not name a species pair `cutoff` names
 *   (AMOF_EINVAL).  Link bonds never join fragments; they are counted between them.
 *   ref_label (optional) [N]: a partition by roots (ref_label[i] = the smallest atom of i's class; AMOF_EINVAL otherwise),
 *   e.g. the labels of a reference frame.  kinds (optional) [K][S]: species-count vectors; a fragment is OF KIND k iff its
 *   species counts equal kinds[k] (the first such k), of kind K otherwise.
 *   Outputs, over the frames of the call:
 *     summary int64 [F][5]: fragments, atoms of the largest, winding fragments, atoms with label != ref_label (-1 without
 *       ref_label), link bonds (unordered) whose two ends lie in one fragment (0 without link)
 *     size_hist int64 [F][max_size + 2]: fragments by atom count 0 .. max_size; the last bin: larger ones
 *     census int64 [F][K + 1]: fragments per kind; the last column: all others
 *     links (optional) int64 [F][K + 1][K + 1]: ORDERED link bonds i -> j with label[i] != label[j], by the kind of i's
 *       fragment and the kind of j's (every bond is counted once from each end; bonds, not distinct partner fragments)
 *     label (optional) int32 [F][N], shift (optional) int32 [F][N][3]
 *     com (optional, needs ref_label) f64 [F][M][3], frag_mass (optional, needs ref_label) f64 [M]: M = the number of
 *       distinct roots of ref_label (the caller passes it; checked), row k = the k-th smallest root; frag_mass in ascending
 *       atom order.  A frame whose partition differs from ref_label (summary column 3 != 0) has NaN rows, and so has a
 *       fragment that winds.
 *   Capacities (AMOF_ECAPACITY, the message names the limit and the first frame; nothing is truncated silently): N <= 65535,
 *   at most 16 neighbours per atom (cutoff and link rows alike), a bond's image within 127 cells, a shift within 32767.
 *   Every output is independent per frame: frame ranges concatenate bit for bit, and nothing depends on the batching
 *   (AMOF_FRAGMENT_BATCH_MB=n caps the rows, records and scratch of a batch of frames, default 256; 0: one frame per batch) or
 *   the path ("fragment_frame"; AMOF_FRAGMENT_GLOBAL=1, or 16 N bytes beyond the LDS of a workgroup -- AMOF_FRAGMENT_LDS_KB=n
 *   lowers that limit, for tests: "fragment_global").
 *   amof_last_kernel_seconds: which = 2 the adjacency rows, 3 the labelling, 4 the reduction with the census.
 *   amof_fragment_round_stats: out[3] = frames, labelling rounds summed over them (a frame's rounds: one more than the
 *   eccentricity of the root that takes longest), the most rounds of a frame, of the last call.
 * The outputs are overwritten (zeros after an error).  Errors: AMOF_EINVAL, AMOF_ESINGULAR, AMOF_ECAPACITY, AMOF_ENOMEM,
 * AMOF_EHIP.
 */
int amof_fragment_stats(amof_ctx *ctx, const amof_traj *traj, const double *cutoff /* [S][S], symmetric */,
                        const double *link /* [S][S] or NULL */, const int32_t *ref_label /* [N] or NULL */,
                        const int32_t *kinds /* [K][S] or NULL */, int32_t K, int32_t max_size,
                        int64_t *summary /* host [F][5] */, int64_t *size_hist /* host [F][max_size + 2] */,
                        int64_t *census /* host [F][K + 1] */, int64_t *links /* host [F][K + 1][K + 1] or NULL */,
                        int32_t *label /* host [F][N] or NULL */, int32_t *shift /* host [F][N][3] or NULL */,
                        double *com /* host [F][M][3] or NULL */, double *frag_mass /* host [M] or NULL */, int32_t M);
int amof_fragment_round_stats(const amof_ctx *ctx, double *out /* [3] */);

/*
 * Pore geometry on a grid: the distance of every grid point to the nearest atomic surface, and from it the void
 * fraction for a set of probe radii, the cavity-size histogram and the largest included sphere, per frame.
 * The reference's Pore (amof/pore.py) writes one CIF per frame and runs the external Zeo++ binary on it (Voronoi network,
 * Monte-Carlo sampling, accessibility test); this is the deterministic grid version of the same geometric quantities and
 * does not reproduce Zeo++'s numbers.  The counts are of probe CENTRES that fit, accessible or not: amof_pore_access below
 * splits them.
 *   grid n = (nx, ny, nz), G = nx ny nz <= 2^31 - 1.  Point (i, j, k), linear index (i ny + j) nz + k:
 *     f = (((double)i + 0.5) / (double)nx, ...),  p_c = (f_x C[0][c] + f_y C[1][c]) + f_z C[2][c]   (no fma; the grid spans
 *     the cell parallelepiped, also along non-periodic axes)
 *   atom j of species s: d0 = r_j - p from the raw positions, the canonical minimum image of it and d2 exactly as
 *     amof_cn_count forms them, v_j = sqrt(d2) - radii[s]
 *   field v(p) = min_j v_j if that is < dmax, else dmax (the point then counts as overflow).  The minimum of IEEE numbers
 *     does not depend on the order: v is bit-identical whatever the path, the batching or the frame range.
 *   dmax + max_s radii[s] must not exceed half the smallest perpendicular height of any frame's cell on a periodic axis
 *     (AMOF_EINVAL; the heights are compared with a relative slack of 1e-12): one minimum image then suffices.
 *   nbins = (int)rint(dmax / dr);  nbins + 2 + n_t <= AMOF_PORE_MAX_WORDS (AMOF_ECAPACITY)
 *   hist [F][nbins + 2]: [0] points with v < 0 (inside an atom: v < 0 <=> sqrt(d2) < R, amof_cn_count's decision);
 *     [1 + b] points with b = (int)(v / dr), 0 <= v < dmax, b < nbins;  [nbins + 1] the rest (overflow).  A row sums to G.
 *   counts [F][n_t]: points with v >= thresholds[t] (float64 compare of the field value)
 *   vmax [F], argmax [F]: the largest field value and the smallest linear index that has it
 *   field (optional, may be NULL) host [F][G]: the field itself; at most 4 GiB per frame (AMOF_ECAPACITY)
 * Paths (amof_last_path): "pore_brick", "pore_exact"; AMOF_PORE_EXACT=1 forces the latter, AMOF_PORE_BATCH=n caps the frames
 * per launch.  amof_last_kernel_seconds: which = 2 the cell sort, 3 the field kernels.
 * All outputs are overwritten (zeros after an error).  Errors: AMOF_EINVAL, AMOF_ECAPACITY, AMOF_ESINGULAR, AMOF_ENOMEM, AMOF_EHIP.
 */
int amof_pore_field(amof_ctx *ctx, const amof_traj *traj, const double *radii /* host [S], Angstrom */,
                    const int32_t *grid /* host [3] */, double dr, double dmax, const double *thresholds /* host [n_t] */,
                    int32_t n_t, uint64_t *hist /* host [F][nbins + 2] */, int64_t *counts /* host [F][n_t] */,
                    double *vmax /* host [F] */, int64_t *argmax /* host [F] */, double *field /* host [F][G] or NULL */);
/* the bound eps_c (Angstrom) on |candidate - v| that "pore_brick" uses for a cell (rows = cell vectors) and
 * rcut = dmax + max_s radii[s] (amof_amd/csrc/pore_math.h): atoms whose float32 candidate is within 2 eps_c of the
 * candidate minimum are re-evaluated in float64.  Tests plant decisions inside it. */
double amof_pore_candidate_bound(const double *cell /* host [9] */, double rcut);

/*
 * Accessibility of the void: which part of V(t) percolates through the periodic cell, and the free sphere.
 * (The reference's Pore.compute_surface_volume reads AV_* / NAV_* from Zeo++ -vol; this is the grid version on the field
 * above and does not reproduce Zeo++'s numbers.)  Definitions:
 *   void       V(t) = { p : v(p) >= t }, the float64 compare of the (dmax-capped) field that `counts` uses
 *   adjacency  two grid points whose indices differ by +-1 along exactly one grid axis (6-neighbourhood in index space; the
 *              grid axes are the lattice vectors).  On a periodic axis index n_k - 1 is adjacent to index 0 of the next
 *              image, on an open axis it is not.  A periodic axis needs n_k >= 3 (AMOF_EINVAL): with 1 or 2 points a point
 *              meets itself or the same neighbour through both faces.
 *   component  a connected component of V(t) in this periodic graph; its label is the smallest linear index
 *              (i ny + j) nz + k among its points -- independent of launch order, batching, path and frame range
 *   winding    of a closed path inside a component: + e_k for every time it leaves through the upper face of periodic axis
 *              k, - e_k through the lower.  The winding vectors of a component form a lattice in Z^3; its rank (0 .. 3) is
 *              the component's DIMENSION.  Dimension >= 1: a CHANNEL, its points are ACCESSIBLE; dimension 0: a POCKET (also
 *              a component that crosses a face and comes back through the same face).
 *   free sphere  t* = the largest field value t >= 0 for which V(t) has a channel: V(t*) has one, V(nextafter(t*, +inf))
 *              has none.  Df = 2 t* (0 if V(0) has no channel, +inf if V(dmax) has one: not resolved, as for Di);
 *              Dif = 2 max v over the channels of V(t*), +inf where that is the cap dmax, 0 where Df = 0.
 * amof_pore_access: amof_pore_field (same tiers, same switches, same first outputs and field, bit for bit) with every batch's
 * field kept in device memory and labelled there.
 *   access [F][n_t][4]: accessible points, channels, pockets, largest channel dimension of V(thresholds[t])
 *   free_sphere [F][2] (may be NULL when want_free == 0; AMOF_EINVAL otherwise): t* and Dif / 2
 *   labels (optional) host int32 [F][n_t][G]: the component label of every point, -1 outside the void; at most 4 GiB per
 *     frame (AMOF_ECAPACITY)
 * amof_pore_access_field: the same labelling of a field the caller supplies (host [n_frames][G], finite), e.g. one kept from
 * amof_pore_field or one that is no distance at all; pbc[3]: which grid axes are periodic.  Here t* is the largest field
 * value of any sign with a channel and free_sphere is (-inf, -inf) where V(t) has no channel for any t.
 * One labelling is a union-find over the grid points (amof_amd/csrc/pore_access.hip); the windings are resolved on the host
 * from the links through the cell's faces (amof_amd/csrc/pore_access_math.h).  The free sphere takes ceil(log2(G + 1))
 * labellings per frame at most (bisection over the sorted field) and one more.
 * Paths (amof_last_path names the labelling): "pore_label_tile" (tiles of 8 x 8 x 32 points labelled in LDS, the links across
 * tile faces merged in device memory), "pore_label_global" (every link merged in device memory; AMOF_PORE_LABEL_GLOBAL=1).
 * Both give the same bits.  amof_last_kernel_seconds: which = 4 the labelling (device work and the host's share between
 * its kernels); amof_last_kernel_launches: the labellings of the call.
 * All outputs are overwritten (zeros after an error).  Errors: as amof_pore_field.
 */
int amof_pore_access(amof_ctx *ctx, const amof_traj *traj, const double *radii /* host [S] */, const int32_t *grid /* host [3] */,
                     double dr, double dmax, const double *thresholds /* host [n_t] */, int32_t n_t, int32_t want_free,
                     uint64_t *hist /* host [F][nbins + 2] */, int64_t *counts /* host [F][n_t] */, double *vmax /* host [F] */,
                     int64_t *argmax /* host [F] */, int64_t *access /* host [F][n_t][4] */,
                     double *free_sphere /* host [F][2] or NULL */, double *field /* host [F][G] or NULL */,
                     int32_t *labels /* host [F][n_t][G] or NULL */);
int amof_pore_access_field(amof_ctx *ctx, const double *field /* host [n_frames][G] */, int64_t n_frames,
                           const int32_t *grid /* host [3] */, const int32_t *pbc /* host [3] */,
                           const double *thresholds /* host [n_t] */, int32_t n_t, int32_t want_free,
                           int64_t *access /* host [n_frames][n_t][4] */, double *free_sphere /* host [n_frames][2] or NULL */,
                           int32_t *labels /* host [n_frames][n_t][G] or NULL */);

/*
 * Covering radius of the pore field: the Gelb-Gubbins pore size distribution and the probe-occupiable volume.
 * (The reference reads POAV / PONAV from Zeo++ -volpo and the distribution from -psd, amof/pore/pysimmzeopp.py; this is the
 * grid version on the field above and does not reproduce Zeo++'s numbers.)  The cumulative pore volume V(r) is the volume of
 * the points that a sphere of radius r, overlapping no atom, can cover; - dV/dr is the pore size distribution, and V(rp) the
 * volume a probe of radius rp occupies -- the whole probe sphere, not only its centre.  Both are read off one field over the
 * grid, the covering radius w.  Let v be the (dmax-capped) field of amof_pore_field on the grid n of a frame with cell C:
 *   step vectors   A_k[c] = C[k][c] / (double)n_k
 *   offset distance  of an integer offset D = (Di, Dj, Dk): s_c = ((double)Di A_0[c] + (double)Dj A_1[c]) + (double)Dk A_2[c],
 *                  d2(D) = (s_x s_x + s_y s_y) + s_z s_z -- float64 in this order, no fma.  It depends on the offset and the
 *                  frame's cell only, not on the point.
 *   target point   p + D: the grid point whose indices are those of p plus D, modulo n_k on a periodic axis; on an open axis an
 *                  offset that leaves the grid does not exist
 *   covering       a centre c = p + D COVERS p iff v(c) >= 0 and d2(D) <= v(c) v(c) (float64 product and compare)
 *   covering radius  w(p) = max { v(c) : c covers p }; w(p) = v(p) if no centre covers p.  A point with v(p) >= 0 covers
 *                  itself through D = 0, so an uncovered point has w = v < 0.  The maximum of IEEE numbers does not depend on
 *                  the order: w is bit-identical on every path, batching, frame range and rank.
 *   one image at most  every value of v is at most dmax, which is at most half the smallest periodic perpendicular height: no
 *                  sphere reaches p through more than one image of its centre.  amof_pore_psd_field enforces the same on the
 *                  field it is given: max(field) > half the smallest periodic perpendicular height (1 + 1e-12) of the frame's
 *                  cell is AMOF_EINVAL.
 *   overflow       where v is capped at dmax, w is a lower bound; such frames are flagged as for the largest included sphere
 *                  (hist[f][nbins + 1] > 0).
 * Per frame:
 *   psd_hist [F][nbins + 2]: [0] points with w < 0 (covered by no sphere); [1 + b] points with b = (int)(w / dr) for
 *     0 <= w < dmax, b < nbins; [nbins + 1] the rest (w >= dmax).  A row sums to G; nbins and dr are the field histogram's.
 *   po_counts [F][n_t]: points with w >= thresholds[t] -- the probe-occupiable volume in points, at least counts[f][t]
 *   po_access [F][n_t] (want_access; AMOF_EINVAL if NULL then): points covered by at least one centre that lies in a CHANNEL
 *     of V(thresholds[t]) -- the components and channels of amof_pore_access; every such centre has v >= thresholds[t].  At
 *     most po_counts; po_counts - po_access, the points a probe reaches only from pockets, is the non-accessible occupiable
 *     count, so that POAV + PONAV = POV holds in integers.
 *   cover (optional, may be NULL) host [F][G]: w itself; at most 4 GiB per frame (AMOF_ECAPACITY)
 * amof_pore_psd: amof_pore_field -- or, with want_access or want_free, amof_pore_access, whose `access` array is then
 * required -- with the same tiers, switches and outputs, bit for bit, and every batch's field covered where it lies.
 * amof_pore_psd_field: the same analysis of a field the caller supplies (host [n_frames][G], finite) with the cell of every
 * frame (host [n_frames][9], rows = cell vectors); pbc[3]: which grid axes are periodic (want_access: at least 3 points each).
 * Paths (amof_last_path): "pore_cover_brick" -- a workgroup owns a brick of 8 x 8 x 8 points, keeps the source bricks and of
 * those the centres whose sphere reaches the brick's bounding sphere, and every lane sweeps these records for its points --
 * and "pore_cover_exact" -- a lane per point walks every offset with d2 <= (the frame's largest v)^2; also
 * AMOF_PORE_COVER_EXACT=1, a brick that keeps more than 2048 source bricks (the frame is then run again on the exact path;
 * AMOF_PORE_COVER_SRC_CAP=n lowers that limit, for tests), a reach of more than 32768 source bricks.  Both
 * decide with the canonical compare above and give the same bits.  amof_last_kernel_seconds: which = 5 the covering stage
 * (2 .. 4 as amof_pore_access); amof_last_kernel_launches: its passes.  amof_pore_cover_stats: out3 = destination bricks,
 * source bricks kept, centre records swept, summed over the full passes of the last call on "pore_cover_brick".
 * All outputs are overwritten (zeros after an error).  Errors: as amof_pore_field.
 */
int amof_pore_psd(amof_ctx *ctx, const amof_traj *traj, const double *radii /* host [S] */, const int32_t *grid /* host [3] */,
                  double dr, double dmax, const double *thresholds /* host [n_t] */, int32_t n_t, int32_t want_access,
                  int32_t want_free, uint64_t *hist /* host [F][nbins + 2] */, int64_t *counts /* host [F][n_t] */,
                  double *vmax /* host [F] */, int64_t *argmax /* host [F] */,
                  int64_t *access /* host [F][n_t][4]; may be NULL without want_access and want_free */,
                  double *free_sphere /* host [F][2] or NULL */, double *field /* host [F][G] or NULL */,
                  int32_t *labels /* host [F][n_t][G] or NULL */, uint64_t *psd_hist /* host [F][nbins + 2] */,
                  int64_t *po_counts /* host [F][n_t] */, int64_t *po_access /* host [F][n_t]; NULL unless want_access */,
                  double *cover /* host [F][G] or NULL */);
int amof_pore_psd_field(amof_ctx *ctx, const double *field /* host [n_frames][G] */, const double *cells /* host [n_frames][9] */,
                        int64_t n_frames, const int32_t *grid /* host [3] */, const int32_t *pbc /* host [3] */, double dr,
                        double dmax, const double *thresholds /* host [n_t] */, int32_t n_t, int32_t want_access,
                        uint64_t *psd_hist /* host [n_frames][nbins + 2] */, int64_t *po_counts /* host [n_frames][n_t] */,
                        int64_t *po_access /* host [n_frames][n_t]; NULL unless want_access */,
                        double *cover /* host [n_frames][G] or NULL */);
int amof_pore_cover_stats(const amof_ctx *ctx, double *out3 /* host [3] */);

/*
 * Surface area of the pore space: deterministic Shrake-Rupley sampling of the atoms' spheres.
 * (The reference reads ASA / NASA from Zeo++ -sa, amof/pore/core.py get_surface_volume: Monte-Carlo samples on the same
 * spheres, accessibility from a Voronoi network.  This is the deterministic version on a fixed table of directions, with
 * accessibility from the grid's channels; it does not reproduce Zeo++'s numbers.)  Definitions:
 *   directions  dirs, host float64 [M][3], 1 <= M <= 4096 (AMOF_EINVAL), every row a unit vector: | |u|^2 - 1 | <= 1e-12 with
 *               |u|^2 = (u_x u_x + u_y u_y) + u_z u_z (AMOF_EINVAL).  The library computes no sine or cosine: the caller builds
 *               the table (amof_amd.pore.sphere_points: the Fibonacci lattice).
 *   samples     probe radius rp = thresholds[t] >= 0 (AMOF_EINVAL), atom j of species s: rho_j = radii[s] + rp in float64 and
 *               s_c = r_jc + rho_j u_mc -- the product first, then the sum, no fma
 *   exposed     sample (j, m) is exposed iff for every atom k != j (by atom index): d0 = r_k - s from the raw positions, the
 *               canonical minimum image of it and d2 exactly as amof_cn_count and the field form them, and
 *               sqrt(d2) - radii[s_k] >= rp -- the field's float64 compare.  A sample is exposed exactly when the field of all
 *               OTHER atoms, evaluated at the sample, is >= rp.
 *   one image   max_s radii[s] + max_t thresholds[t] must not exceed half the smallest perpendicular cell height on a periodic
 *               axis (AMOF_EINVAL; relative slack 1e-12 as for the field): one minimum image per pair then suffices, and no
 *               other image of j comes closer to its own sample than rho_j.
 *   exposed [F][n_t][S]: exposed samples per species of the sampled atom.  Integers: paths, batches, frame ranges and ranks agree
 *               bit for bit.  The host forms SA = sum_s 4 pi (radii[s] + rp)^2 exposed_s / M (Angstrom^2); rp = 0 is the van
 *               der Waals surface.
 *   accessible  (want_access) f = s C^-1, wrapped into [0, 1) on periodic axes; t_k = f_k n_k - 0.5, i_k = floor(t_k).  The 8
 *               grid points (i_x + a, i_y + b, i_z + c), a, b, c in {0, 1}, are the sample's corners: indices modulo n_k on a
 *               periodic axis, a corner outside the grid on an open axis is dropped.  An exposed sample is accessible iff at
 *               least one corner belongs to a channel of V(rp) (amof_pore_access).  An exposed sample with no corner in a
 *               channel -- also one in a crevice narrower than the grid -- counts as non-accessible: a grid estimate that
 *               converges with the spacing.
 *   exposed_access [F][n_t][S] (want_access; AMOF_EINVAL if NULL then): accessible samples; NASA = exposed - exposed_access
 *   samples (optional, may be NULL) host uint8 [F][n_t][N][M], atoms in input order: 0 buried, 1 exposed, 2 exposed and
 *               accessible; at most 4 GiB per frame (AMOF_ECAPACITY)
 * amof_pore_surface: amof_pore_psd's arguments, stages, switches and outputs, bit for bit -- the covering stage only with
 * want_psd (psd_hist, po_counts, po_access and cover may be NULL without it) -- and the surface stage per (frame, threshold):
 * behind the labelling of that threshold where the call labels (want_access or want_free), on its own otherwise.
 * Paths (amof_last_path): "pore_surface_list" -- a wave per atom of a cell-sorted frame gathers the atom's neighbour images as
 * float32 records, its lanes sweep them per sample with a root-free float32 compare and re-decide in canonical float64 inside
 * the guard band amof_pore_surface_bound -- and "pore_surface_exact" -- a lane per sample, every atom in canonical float64: open
 * axes, AMOF_PORE_SURFACE_EXACT=1, a wave with more than 512 neighbour records (the launch is then run again on the exact
 * path; AMOF_PORE_SURFACE_LIST_CAP=n lowers that limit, for tests).  Both give the same integers.  The list holds the records
 * that bury a quarter of the atom's sphere or more in front, so that a buried sample ends sooner; AMOF_PORE_SURFACE_UNSORTED=1
 * keeps the order of the gather (for measurements; the same integers).
 * amof_last_kernel_seconds: which = 6 the surface stage; amof_last_kernel_launches: its launches.  amof_pore_surface_stats:
 * out5 = atoms swept, neighbour records kept, samples, float64 re-decisions, samples ended before the end of their list, summed
 * over the launches of the last call that stayed on "pore_surface_list".
 * All outputs are overwritten (zeros after an error).  Errors: as amof_pore_field.
 */
int amof_pore_surface(amof_ctx *ctx, const amof_traj *traj, const double *radii /* host [S] */, const int32_t *grid /* host [3] */,
                      double dr, double dmax, const double *thresholds /* host [n_t], >= 0 */, int32_t n_t, int32_t want_access,
                      int32_t want_free, uint64_t *hist /* host [F][nbins + 2] */, int64_t *counts /* host [F][n_t] */,
                      double *vmax /* host [F] */, int64_t *argmax /* host [F] */,
                      int64_t *access /* host [F][n_t][4]; may be NULL without want_access and want_free */,
                      double *free_sphere /* host [F][2] or NULL */, double *field /* host [F][G] or NULL */,
                      int32_t *labels /* host [F][n_t][G] or NULL */, uint64_t *psd_hist /* host [F][nbins + 2]; NULL without want_psd */,
                      int64_t *po_counts /* host [F][n_t]; NULL without want_psd */,
                      int64_t *po_access /* host [F][n_t]; NULL unless want_psd and want_access */,
                      double *cover /* host [F][G] or NULL */, int32_t want_psd, const double *dirs /* host [n_dirs][3] */,
                      int32_t n_dirs, int64_t *exposed /* host [F][n_t][S] */,
                      int64_t *exposed_access /* host [F][n_t][S]; NULL unless want_access */,
                      uint8_t *samples /* host [F][n_t][N][n_dirs] or NULL */);
/* the bound eps (Angstrom) of the float32 compare of "pore_surface_list" for a cell (rows = cell vectors) and
 * reach = max_s radii[s] + max_t thresholds[t] (amof_amd/csrc/pore_surface_math.h): a sample closer than eps to a neighbour's
 * sphere is re-decided in float64.  Tests plant decisions inside it. */
double amof_pore_surface_bound(const double *cell /* host [9] */, double reach);
int amof_pore_surface_stats(const amof_ctx *ctx, double *out5 /* host [5] */);

/*
 * Static structure factor by direct summation over reciprocal-lattice vectors.
 * Replaces nothing the reference computes (the structure of an amorphous MOF is compared with total-scattering data; the
 * reference stops at g(r), amof/rdf.py).  Cells must be periodic on all three axes.
 *   For every selected frame f = frame_begin, frame_begin + frame_stride, ... < frame_end and every vector m of hkl
 *   (integer triples, not (0, 0, 0); the caller passes half a space: rho(-k) = conj rho(k)):
 *     R = recip[cell of f] ([3][3], 2 pi inv(cell).T, computed by the caller),
 *     qx = (h*R[0][0] + k*R[1][0]) + l*R[2][0] (likewise y, z; float64, no fma), q2 = (qx*qx + qy*qy) + qz*qz,
 *     q = sqrt(q2) (correctly rounded), bin b = (int)(q / dq); b >= nbins: one more in *beyond, nothing else.
 *     rho_a = sum over the atoms j of species a of exp(2 pi i phi_j / 2^32), phi_j = h ux_j + k uy_j + l uz_j (mod 2^32)
 *       with u = the atom's fractional coordinates * 2^32, folded into the cell (the fast paths' quantisation): the
 *       phase is exact for any cell and for unwrapped input; one f32 v_sin / v_cos per term, f32 partials over <= 64
 *       atoms folded into f64 (the tests hold every S column within 1e-5 max(1, |S|) of a float64 restatement).
 *       Measured on the MI355X against the exact phase (tests/test_gpu_sq_accuracy.py: test_single_terms), the error of
 *       one term, int-to-float conversion included, is at most 2.980 x 2^-24 for cos and 2.931 x 2^-24 for sin over
 *       2 x 262 144 swept phases, and 1.017 / 0.814 x 2^-24 over 2 x 128 planted ones (powers of two and their
 *       neighbours, eighths of a revolution, +-1/2); the tests' constant is TERM_ERR = 2^-21, the smallest power of
 *       two at least twice the largest.  rho_a then lies within n TERM_ERR + acc(n) of the exact sum per component, n
 *       the atoms of the species and acc(n) = 2^-24 sum over the partials of (m (m + 1) / 2 - 1), m <= 64 their
 *       lengths: 1.94e-6 per atom at worst, which keeps a fully coherent (Bragg) peak of S within 5e-6 |S|.
 *     counts[b] += 1;  for every unordered pair p = (a, c), a <= c, in the order (0,0), (0,1) .. (0,S-1), (1,1) ..:
 *     sums[p][b] += t_ac = Re rho_a Re rho_c + Im rho_a Im rho_c.
 *   Each t is rounded to an integer multiple of 2^-s_p and added as int64 (integer atomics: the result is independent of
 *   the launch and of how frames are split); s_p is the largest exponent with F * C * (N_a N_c + 1/2) * 2^s_p < 2^62.
 *   F = traj->n_frames; C = the largest number of vectors of hkl that can fall into one bin in one frame of any of the
 *   trajectory's cells (|q| within delta |hkl| of its value on the mean reciprocal matrix, delta the largest Frobenius
 *   norm of a cell's deviation from that mean): every frame range of one trajectory has the same scale, and ranges add
 *   up bit for bit.  When 2^-s_p / sqrt(N_a N_c) would exceed 2^-20: AMOF_ECAPACITY (the caller passes shorter
 *   trajectories: StructureFactor then accumulates chunks of frames).  Two identical calls give identical bits (the
 *   atoms are summed in species order, in a fixed order).
 *   Errors: AMOF_EINVAL (pbc not all set, hkl (0, 0, 0), bad frame range, dq, nbins < 1, positions beyond 10^4 cells,
 *   NULL argument), AMOF_ECAPACITY, AMOF_ESINGULAR, AMOF_ENOMEM, AMOF_EHIP, AMOF_ENODEVICE.
 * The host form overwrites counts, sums (float64: int64 * 2^-s_p) and *beyond.
 */
int amof_sq_accumulate(amof_ctx *ctx, const amof_traj *traj, const double *recip /* host [n_cells][3][3] */,
                       const int32_t *hkl /* host [K][3] */, int32_t K, int64_t frame_begin, int64_t frame_end,
                       int64_t frame_stride, double dq, int32_t nbins, uint64_t *counts /* host [nbins] */,
                       double *sums /* host [P][nbins], P = S(S+1)/2 */, uint64_t *beyond /* host [1] */);
/* The same with the results ADDED into device buffers (frame-sharded ranks all-reduce them next): sums_dev holds the
 * int64 fixed-point sums (sums = sums_dev * 2^-scale_log2[p]); scale_log2 (host [P]) receives the exponents. */
int amof_sq_accumulate_dev(amof_ctx *ctx, const amof_traj *traj, const double *recip, const int32_t *hkl, int32_t K,
                           int64_t frame_begin, int64_t frame_end, int64_t frame_stride, double dq, int32_t nbins,
                           uint64_t *counts_dev /* device [nbins], += */, int64_t *sums_dev /* device [P][nbins], += */,
                           uint64_t *beyond_dev /* device [1], += */, int32_t *scale_log2 /* host [P] */);
/* rho_a(k) of one frame: rho[(m*S + a)*2 + 0 / 1] = Re / Im rho_a of vector m of hkl (the kernel of amof_sq_accumulate,
 * written out instead of binned; any hkl but (0, 0, 0), no half-space rule).  Errors as amof_sq_accumulate. */
int amof_sq_modes(amof_ctx *ctx, const amof_traj *traj, int64_t frame, const int32_t *hkl /* host [K][3] */, int32_t K,
                  double *rho /* host [K][S][2] */);

/*
 * Intermediate scattering function F(q, t): the time correlation of rho_a(k) on reciprocal-lattice vectors, coherent and self.
 * Replaces nothing the reference computes (the reference has no dynamic analysis in reciprocal space).  Cells must be
 * periodic on all three axes.  recip, hkl (half a space, no (0, 0, 0)), dq, nbins: as amof_sq_accumulate.
 *   Lags, origins and work list: amof_vanhove_distinct's (stated there).  A call handles the entries
 *   [work_begin, work_end): ranges of one trajectory add up bit for bit.
 *   rho_a(f; hkl) is what amof_sq_modes returns for frame f and that vector, bit for bit (the same kernel and atom order;
 *   it does not depend on how the vectors are grouped into runs or chunks).
 *   For every entry (w, k) and every vector: the bin b from frame k's (the ORIGIN's) reciprocal matrix in
 *   amof_sq_accumulate's operation order (float64, no fma, b = (int)(q / dq)); !(q / dq < nbins): beyond[w] += 1 and
 *   nothing else.  Otherwise counts[w][b] += 1 and
 *     coherent, every ORDERED species pair (a at the origin, c at the origin + lag -- amof_vanhove_distinct's order):
 *       t_ac = Re rho_a(k) * Re rho_c(k + m) + Im rho_a(k) * Im rho_c(k + m)   (float64, two products and one add, no fma)
 *       coh[a][c][w][b] += rint(t_ac * 2^s_p) as int64 (integer atomics), p the unordered pair {a, c};
 *     self, every species a (only when the self output is given):
 *       u_a = sum over the atoms j of a of cos(2 pi phi_j / 2^32), phi_j = h dx + k dy + l dz (mod 2^32),
 *       d = Q_j(k + m) - Q_j(k) in u32 wrap-around arithmetic on the quantised fractional coordinates: on reciprocal-LATTICE
 *       vectors the phase of a displacement is periodic in the cell, so no unwrapping and no centre-of-mass convention
 *       enters.  This is rho's real part on a "difference frame" (the same kernel: f32 partials over <= 64 atoms folded
 *       into f64 in a fixed order);  self[a][w][b] += rint(u_a * 2^s_(a,a)).
 *   s_p is amof_sq_accumulate's scale for the same trajectory, vectors, dq and nbins (a counter receives at most n_w C <=
 *   F C samples, so that bound holds unchanged; it does not depend on windows, stride or work range), with the same
 *   AMOF_ECAPACITY rule.  At lag 0, coh[a][c] == coh[c][a] == amof_sq_accumulate's sums[p] over the origin frames, and
 *   self[a] = N_a counts up to the fixed-point quantum.  Integer sums: the result is independent of tiling, vector
 *   chunking, launch order and rank split; two identical calls give identical bits.
 *   The rho table of a chunk of vectors ([frames touched][K_c][S][2] float64) is kept within 1 GiB (AMOF_ISF_RHO_BUDGET,
 *   bytes, overrides); every touched frame is quantised once per call (16 N bytes per frame of scratch).
 *   No capacity limit on W, nbins, K, F or N other than the fixed-point rule.
 * The host form overwrites counts, coh, self_sums (float64: int64 * 2^-s; self_sums == NULL: no self part) and beyond.
 * Errors: as amof_sq_accumulate, plus AMOF_EINVAL for a bad window, origin_stride or work range.
 */
int amof_isf_accumulate(amof_ctx *ctx, const amof_traj *traj, const double *recip /* host [n_cells][3][3] */,
                        const int32_t *hkl /* host [K][3] */, int32_t K, const int32_t *windows /* host [W] */,
                        int32_t n_windows, int64_t origin_stride, int64_t work_begin, int64_t work_end, double dq, int32_t nbins,
                        uint64_t *counts /* host [W][nbins] */, double *coh /* host [S][S][W][nbins] */,
                        double *self_sums /* host [S][W][nbins] or NULL */, uint64_t *beyond /* host [W] */);
/* The same with the results ADDED into device buffers (ranks that share the work list all-reduce them next): coh_dev and
 * self_dev (NULL: no self part) hold the int64 fixed-point sums (value = sum * 2^-scale_log2[p], p = the unordered pair
 * of amof_sq_accumulate's order; self of species a uses the pair (a, a)); scale_log2 (host [P]) receives the exponents. */
int amof_isf_accumulate_dev(amof_ctx *ctx, const amof_traj *traj, const double *recip, const int32_t *hkl, int32_t K,
                            const int32_t *windows, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                            int64_t work_end, double dq, int32_t nbins, uint64_t *counts_dev /* device [W][nbins], += */,
                            int64_t *coh_dev /* device [S][S][W][nbins], += */,
                            int64_t *self_dev /* device [S][W][nbins] or NULL, += */, uint64_t *beyond_dev /* device [W], += */,
                            int32_t *scale_log2 /* host [P] */);

/*
 * Current correlation functions C_L(q, t) and C_T(q, t): the time correlation of the particle current
 *   j_a(k, t) = sum over the atoms j of species a of v_j(t) exp(i k . r_j(t))
 * on reciprocal-lattice vectors, projected along (longitudinal) and across (transverse) k.  The collective counterpart of
 * amof_vacf_window; replaces nothing the reference computes.  Cells must be periodic on all three axes.  recip, hkl, dq,
 * nbins, the lags, origins and the work list: as amof_isf_accumulate.  The library works in Angstrom per frame (velocity
 * mode: the input's units); the caller divides by the timestep.
 *   Sample of atom j on frame f >= 1 (a sample of the positions mode lives on the half step f - 1/2):
 *     positions mode (vel == NULL): d = the signed int32 reading of Q_j(f) - Q_j(f - 1) per fractional component (u32
 *       wrap-around arithmetic on quantize_atom's coordinates, each frame in its own cell: the device of the self part of
 *       F(q, t)); s = (double)d * 2^-32; v_c = fma(s_z, C[2][c], fma(s_y, C[1][c], s_x * C[0][c])) with C the cell of frame
 *       f.  Phase position: p = Q_j(f - 1) + (uint32)(d >> 1) per component (arithmetic shift), the midpoint.
 *     velocity mode (vel: a second amof_traj whose pos holds velocities [F][N][3] of the same frames and atoms; nothing else
 *       of it is read): v = vel[f][j], p = Q_j(f).
 *     remove_com != 0: the mass-weighted mean sample of the frame, sum_j m_j v_j / sum_j m_j (float64, a fixed order, no
 *       float atomics: identical calls, identical bits), is subtracted.  Then w = (float)v per component.
 *   Modes: j_a(f; hkl)[c] = sum_j w_j[c] exp(2 pi i phi_j / 2^32), phi_j = h p_x + k p_y + l p_z (mod 2^32: the exact
 *     phase).  Per (atom, vector): x = (float)(int32)phi * 2^-32, v_cos_f32 / v_sin_f32 of x once, six fmaf with w into f32
 *     partials over at most 64 atoms of the species (stable species order), the partials folded into float64 in a fixed
 *     order.  Identical calls give identical bits; the result does not depend on how the vectors are cut into runs or chunks.
 *   Projection (float64, no fma), per frame with ITS reciprocal matrix R: q = (h R0 + k R1) + l R2 per component,
 *     n = sqrt((qx qx + qy qy) + qz qz), k^ = q / n;  L_a = (k^x j_x + k^y j_y) + k^z j_z for the real and for the imaginary
 *     parts;  T_a[c] = j_a[c] - k^[c] L_a likewise.
 *   Sums, per work entry (w, k), vector and ORDERED species pair (a at the origin k, c at k + m): the bin b and beyond[w]
 *     from frame k as in amof_isf_accumulate; counts[w][b] += 1;
 *       t_L = Re L_a(k) Re L_c(k + m) + Im L_a(k) Im L_c(k + m)
 *       t_T = ((Tx.Tx') + (Ty.Ty')) + (Tz.Tz'),  each (T.T') = Re T Re T' + Im T Im T'   (no factor 1/2)
 *       long[a][c][w][b] += rint(t_L * 2^s_p),  trans[a][c][w][b] += rint(t_T * 2^s_p)  as int64 (integer atomics).
 *   Scale: vmax = the largest |w| component over ALL frames 1 .. F - 1 of the trajectory (an exact maximum, whatever the
 *     work range: ranks and work ranges arrive at the same exponents); per unordered pair p = {a, c}, 2^s_p is the largest
 *     power of two with F C (N_a N_c + 1/2) 3 vmax^2 2^s_p < 2^62 (amof_sq_accumulate's bound times 3 vmax^2), C its bin
 *     capacity: the sums stay below 2^62 + F C / 2 < 2^63.  vmax == 0:
 *     zero sums, scale_log2 == 0.  AMOF_ECAPACITY when 2^-s_p > 2^-20 * 3 vmax^2 sqrt(N_a N_c).
 *   The table of a chunk of vectors ([frames touched][K_c][S][3][2] float64) is kept within 1 GiB
 *   (AMOF_CURRENT_RHO_BUDGET, bytes, overrides).  AMOF_CURRENT_GLOBAL=1: counters in global memory ("current_global").
 * amof_current_modes: j of one frame >= 1, written out: j[((m*S + a)*3 + c)*2 + 0 / 1].
 * The host form overwrites counts, long_sums, trans_sums (float64: int64 * 2^-s) and beyond; both forms write scale_log2
 * (host [P], amof_sq_accumulate's pair order) and *vmax.  amof_last_kernel_seconds: 2 the records (means and vmax included),
 * 3 the table, 4 the correlation.
 * Errors: as amof_isf_accumulate, plus AMOF_EINVAL for velocities of another shape, not finite or beyond float32, missing
 * masses with remove_com, and a frame < 1 in amof_current_modes.
 */
int amof_current_modes(amof_ctx *ctx, const amof_traj *traj, const amof_traj *vel_or_NULL, int64_t frame, int32_t remove_com,
                       const int32_t *hkl /* host [K][3] */, int32_t K, double *j /* host [K][S][3][2] */);
int amof_current_accumulate(amof_ctx *ctx, const amof_traj *traj, const amof_traj *vel_or_NULL, int32_t remove_com,
                            const double *recip /* host [n_cells][3][3] */, const int32_t *hkl /* host [K][3] */, int32_t K,
                            const int32_t *windows /* host [W] */, int32_t n_windows, int64_t origin_stride, int64_t work_begin,
                            int64_t work_end, double dq, int32_t nbins, uint64_t *counts /* host [W][nbins] */,
                            double *long_sums /* host [S][S][W][nbins] */, double *trans_sums /* host [S][S][W][nbins] */,
                            uint64_t *beyond /* host [W] */, int32_t *scale_log2 /* host [P] */, double *vmax /* host [1] */);
/* The same with the results ADDED into device buffers (int64 fixed point: value = sum * 2^-scale_log2[p]): ranks that share
 * the work list all-reduce them next. */
int amof_current_accumulate_dev(amof_ctx *ctx, const amof_traj *traj, const amof_traj *vel_or_NULL, int32_t remove_com,
                                const double *recip, const int32_t *hkl, int32_t K, const int32_t *windows, int32_t n_windows,
                                int64_t origin_stride, int64_t work_begin, int64_t work_end, double dq, int32_t nbins,
                                uint64_t *counts_dev /* device [W][nbins], += */, int64_t *long_dev /* device [S][S][W][nbins], += */,
                                int64_t *trans_dev /* device [S][S][W][nbins], += */, uint64_t *beyond_dev /* device [W], += */,
                                int32_t *scale_log2 /* host [P] */, double *vmax /* host [1] */);

/*
 * Direct MSD with running unwrap, orthogonal cells only (deprecated in the reference).
 * Replaces DirectMsd.compute_species_msd (amof/msd.py:83-107) for every species at once:
 *   msd[t*(S+1) + 0]     = sum over all atoms  |r_i(t) - r_i(0)|^2 / N     (column 'X')
 *   msd[t*(S+1) + 1 + s] = the same over the atoms of species s / N_s
 * with r_i(t) = r_i(t-1) + fold(pos_i(t) - (r_i(t-1) % a_t)) per axis, a_t = cell_t[j][j].
 */
int amof_msd_direct(amof_ctx *ctx, const amof_traj *traj, double *msd /* host [F][S+1] */);

/*
 * Trajectory ingest (host only).
 * Replaces, for the packed path, ase.io.read(filename, index, format='xyz') as driven by
 * Trajectory.from_traj / read_lammps_traj / read_cp2k_traj (amof/trajectory.py:37-60,193-228)
 * and np.genfromtxt on the CP2K cell log (amof/trajectory.py:217).
 *   amof_xyz_scan: number of frames and atoms per frame (all frames must agree).
 *   amof_xyz_read: frames first, first+step, ... (count of them) into pos[count][N][3], N = n_atoms as
 *       amof_xyz_scan reported it (AMOF_EINVAL if the file no longer agrees: nothing is written then);
 *       symbols[N][4] (NUL padded) from the first frame read; lattice[count][9] (may be NULL)
 *       receives extended-XYZ Lattice="..." when every frame carries one (*has_lattice = 1).
 *       n_threads <= 0: all hardware threads.  Numbers are parsed correctly rounded.
 *   amof_cp2k_cell_read: columns [2:-1] (Ax..Cz) of every data row into cell[rows][9];
 *       cell == NULL only counts rows.
 *   amof_xyz_open / amof_xyz_read_frames / amof_xyz_close: the same reader on an OPEN file -- mapping and frame index
 *       are built once and serve any number of batch reads (streamed analyses: amof_amd/stream.py); a handle may be
 *       read from several threads at once.  pos == NULL with lattice != NULL reads the Lattice of the frames only.
 * Errors: negative code, message via amof_ingest_last_error() (thread local).
 */
typedef struct amof_xyz_file amof_xyz_file;
int amof_xyz_open(const char *path, amof_xyz_file **out, int64_t *n_frames, int64_t *n_atoms);
int amof_xyz_read_frames(amof_xyz_file *file, int64_t first, int64_t count, int64_t step, int64_t n_atoms, double *pos,
                         char *symbols, double *lattice, int32_t *has_lattice, int32_t n_threads);
void amof_xyz_close(amof_xyz_file *file);
int amof_xyz_scan(const char *path, int64_t *n_frames, int64_t *n_atoms);
int amof_xyz_read(const char *path, int64_t first, int64_t count, int64_t step, int64_t n_atoms, double *pos,
                  char *symbols, double *lattice, int32_t *has_lattice, int32_t n_threads);
int amof_cp2k_cell_read(const char *path, int64_t max_rows, double *cell, int64_t *n_rows);
const char *amof_ingest_last_error(void);

/*
 * Packing a list of frames (host only).
 * Replaces the per-frame Python walk over a list of ase.Atoms (amof/trajectory.py:27-35,56-59; amof/rdf.py:88-93,
 * amof/msd.py:218-242) for the packed path: frame_pos[k] points at frame k's positions ([N][3] float64, C-contiguous --
 * ase.Atoms.positions); amof_pack_frames copies them into dst[F][N][3] on n_threads threads (<= 0: all hardware threads)
 * and, when checksums != NULL, fingerprints each frame's bytes; amof_frames_checksum fingerprints without copying (is a
 * list that was packed before still the same?).  Equal bytes give equal checksums; the hash is not cryptographic.
 */
int amof_pack_frames(const double *const *frame_pos, int64_t n_frames, int64_t n_atoms, double *dst, uint64_t *checksums,
                     int32_t n_threads);
int amof_frames_checksum(const double *const *frame_pos, int64_t n_frames, int64_t n_atoms, uint64_t *checksums,
                         int32_t n_threads);

#ifdef __cplusplus
}
#endif
#endif /* AMOF_HIP_H */
