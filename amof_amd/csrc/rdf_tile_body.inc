// The body of the tile kernel (rdf.hip: rdf_tile_kernel_fast), included there twice: as the kernel itself for the variants
// without a plan, and as the device function of one grid slice of the planned variants (rdf_tile_slice).  One text, because
// the planned slices are the same kernel with parts compiled out; two places, because a device function that takes the
// arguments by reference is not compiled like the kernel that owns them, and the variants without a plan stay as they are.
// In scope: the template parameters ORTHO, CULL, IMG, ZFK, TRI, PLAN, AHEAD, KIND, SAT and the arguments `fa`.
    // TRI >= 0: general cells in the orthogonalised lattice frame (fast_quad_tri; TRI % 5: near tests, TRI / 5: x wrap with the y term)
    static_assert(!ZFK || (ORTHO && !IMG) || TRI >= 0, "f32 slab coordinates: diagonal cells (no image queue) or TRI");
    static_assert(TRI < 0 || (!ORTHO && !IMG && ZFK), "TRI: general cells, f32 slab coordinates, its own queue");
    // always-add histogram scheme (fast_bin<AA>): measured per variant (profiles/r02/tile_variants.txt) -- the plain
    // general-cell variant spills under it (nine scales, 96 VGPRs) and keeps the masked form
    constexpr bool AA = ORTHO || IMG;
    constexpr bool QUEUE = IMG || TRI >= 0;     // parked pairs, drained densely by the canonical arithmetic
    // flagged pairs wait in per-lane register queues for the end of the step (fast_quad): the diagonal-cell kernels.  68.6 ->
    // 67.0 ms per headline launch -- the first parking scheme that pays (seven with LDS queues lost: profiles/r04/rdf_tile_stop.txt)
    constexpr bool PARK = ORTHO && ZFK && !IMG && TRI < 0 && AA;
    // REACH (rdf_tile_zf with slab culling): of a diagonal tile pair only the sub-tile's own 128-partner block runs the masked
    // body -- partners behind it satisfy j > ia and j > ib always and go through the unmasked loop and the ragged tail quad,
    // like an off-diagonal pair (fa.noreach: every quad masked, as before).  Its quad loops use the SLIM form of fast_quad.
    constexpr bool REACH = ORTHO && CULL && ZFK && !IMG && TRI < 0;
    // PLAN (REACH only): a step's partner window comes from its record of fa.plan (rdf_tile_plan_kernel: the window arithmetic
    // of tile_plan.h over the quantiser's slab table, once per step instead of ballots over sampled quads in every wave), and a
    // step without a quad to visit is not run at all: no centres loaded, no barrier; a frame without a live step stages no
    // tile J, a work item without one returns at once.  Chunks of at most 16 frames (the host launches the kernel without
    // a plan otherwise): the live steps of the chunk are one 64-bit mask.
    static_assert(!PLAN || REACH, "PLAN: the slab-culled diagonal-cell kernel on f32 slab coordinates");
    // AHEAD (PLAN only) bit 0: a wave reads the partner records of its next quad of a piece before the arithmetic of the
    // quad in hand (fast_quad<PRE>); AMOF_RDF_NOAHEAD=1 launches the kernel without it
    static_assert(AHEAD == 0 || PLAN, "AHEAD: the plan variant");
    // KIND (PLAN only): 1 = this workgroup runs the steps its records flag ZF (f32 slab coordinates) and no others, 2 = the steps
    // in integer form and no others; every step of the plan belongs to exactly one of the two, and integer histograms add
    // (rdf_tile_kernel_fast: the grid's two z slices)
    static_assert((KIND != 0) == PLAN, "KIND: the plan variant");
    // SAT (PLAN only): the histogram sits one word up in LDS (both slices: one launch, one LDS size), and the slice on f32 slab
    // coordinates runs the saturating tail (SATS; rdf_sat_math.h, fast_bin<SAT>): no per-pair clamp, no centring of the edge test
    static_assert(!SAT || PLAN, "SAT: the plan variant");
    constexpr bool SATS = SAT && KIND == 1;
    // TRI = 10 / 11: near mode 4 with the exact-half x wrap, c10 = + 1/2 / - 1/2 (tri_q_twin)
    constexpr int NEAR = TRI >= 10 ? 4 : (TRI >= 0 ? TRI % 5 : 0);
    constexpr bool XW = TRI >= 5;
    constexpr int HALF = TRI == 10 ? 1 : (TRI == 11 ? -1 : 0);
    const RdfArgs &a = fa.a;
    extern __shared__ __align__(16) unsigned char lds_raw[];
    // double-buffered tiles: J (512 entries) and the centre sub-tile (128 entries; none with a plan: load_c)
    // (the histogram first: bin_count forms LDS byte addresses from the candidate's bits)
    // (SATS: word 0 is a pad, bin b is word b + 1 -- the address of a candidate q' >= 1 is 4 floor(q') -- and every pointer to
    //  the histogram but bin_count's own arithmetic is `hist`: the zeroing loop, the refinements and the flush follow by themselves)
    unsigned *hist0 = reinterpret_cast<unsigned *>(lds_raw);                 // [nbins + trash (+ pad)], padded to 16 bytes
    unsigned *hist = hist0 + (SATS ? 1 : 0);
    uint4 *tqb = reinterpret_cast<uint4 *>(hist0 + ((fa.a.nbins + FAST_TRASH + 2 + (SAT ? 1 : 0) + 3) & ~3));      // [2][FAST_TILE]
    uint4 *tcb = tqb + 2 * FAST_TILE;                                        // [2][FAST_SUB]; PLAN: [0]
    // IMG: queue of the pairs that need the canonical evaluation (drained densely once per step), two counters
    // (two buffers: a step parks into one while the previous step's is drained; three counters so that one can be
    // reset a whole step away from its last reader and its next writer)
    uint2 *nq_base = reinterpret_cast<uint2 *>(tcb + (PLAN ? 0 : 2 * FAST_SUB));                // [2][img_queue]
    const unsigned nq_cap = (unsigned)fa.img_queue;
    // (the three counters behind the queue, in the dynamic LDS like everything else: the kernel has NO static LDS, so that
    //  the dynamic part starts at LDS address 0 -- bin_count)
    unsigned *nq_count = reinterpret_cast<unsigned *>(nq_base + (size_t)(fa.img_defer ? 2 : 1) * nq_cap);        // [3]

    const int tid = threadIdx.x, lane = tid & 63;
    int wave = __builtin_amdgcn_readfirstlane(tid >> 6);            // (scalar: the quad loops below count in SGPRs)
    // XCD-aware work mapping: workgroups are dealt round-robin over the 8 XCDs (id % 8), each
    // with its own 4 MiB L2.  All work items of one frame chunk go to the same XCD so that the
    // chunk's quantised frames (16 frames x 16 B x N) are re-read from that L2, not from the
    // fabric.  Pure bijection of the grid: correctness does not depend on the placement.
    // The frames that do not divide by 8 (nf % 8 of them) come last, one frame per grid row, their work items on all XCDs:
    // kept in the XCDs' ranges they made one XCD's share a whole frame longer (625 frames: 79 against 78 1/8, 1.1 % of a
    // rank's launch in an 8-GPU run).
    unsigned chunk = blockIdx.y, bx = blockIdx.x;
    const bool tail = (int)blockIdx.y >= fa.n_chunks;
    if (fa.xcd_map && !tail) {      // (off when there are too few chunks to give every XCD its share)
        const unsigned long long lin = (unsigned long long)blockIdx.y * gridDim.x + blockIdx.x;
        // (PLAN: workgroups are dealt to the XCDs by their index in the whole grid, the z slice in front of this one included)
        const unsigned xcd = (unsigned)((lin + (PLAN ? (unsigned long long)blockIdx.z * gridDim.x * gridDim.y : 0ull)) & 7ull);
        const unsigned long long kk = lin >> 3;
        chunk = (unsigned)(kk / gridDim.x) * 8u + xcd;
        bx = (unsigned)(kk % gridDim.x);
    }
    const int2 pr = a.pairs[bx];
    Tile ti = a.tiles[pr.x];
    Tile tj = a.tiles[pr.y];
    const bool diag = pr.x == pr.y;
    const int nbins = a.nbins;
    if constexpr (!PLAN)
        for (int k = tid; k < nbins; k += FAST_THREADS) hist[k] = 0u;

    // equal shares (+-1 frame): with the XCD mapping n_chunks is a multiple of 8, so every XCD gets the same work
    // (with the XCD mapping, XCD x owns the contiguous frame range [x nf/8, (x+1) nf/8), cut into n_chunks/8 shares)
    const unsigned cs = fa.xcd_map ? (chunk & 7u) * ((unsigned)fa.n_chunks >> 3) + (chunk >> 3) : chunk;
    int f0 = tail ? fa.nf_main + ((int)blockIdx.y - fa.n_chunks) : (int)((long long)cs * fa.nf_main / fa.n_chunks);
    const int f1 = tail ? f0 + 1 : (int)((long long)(cs + 1) * fa.nf_main / fa.n_chunks);
    // The (up to four) 128-atom centre sub-tiles of tile I are handled by the same workgroup, frame by
    // frame: a step is (frame, sub-tile); tile J of a frame is staged once and serves all its sub-tiles,
    // and the LDS histogram is flushed once for everything.
    const int nsub = (ti.count + FAST_SUB - 1) / FAST_SUB;
    const int la = 2 * lane, lb = la + 1;                          // local indices in the sub-tile
    // (SATS: the two words of the pair loops are the edge test's 2 g and the candidate's addend 1 + g -- in the scalar
    //  registers and the parameters of fast_quad / fast_bin that the clamped tail uses for 1/2 - g and nbins + g, named there;
    //  clampv is dead in that slice: its place is taken by sat.C)
    const float half_m_guard = SATS ? fa.sat_two_guard : fa.half_m_guard;
    const float nb_hi = SATS ? fa.sat_one_p_guard : fa.nb_hi;
    SatLane sat = {0.0f, 0.0f, 0.0f, 0.0f};      // SATS: the lane's clamp value C, 1 / C and the in-plane scales over C^2
    const float clampv = (float)nbins + 0.5f + (float)(lane & (FAST_TRASH - 1));   // see fast_bin<AA>
    int cntj = tj.count;
    int cntj4 = (cntj + 3) & ~3;
    int full = cntj & ~3;

    // LDS-DMA (1 KiB per wave instruction), indices clamped (slots beyond the counts are never used unmasked):
    // tile J of frame fl into J buffer jb -- wave w moves entries [64w, 64w+64) and [256+64w, ...)
    auto stage_j = [&](int fl, int jb) {
        const QAtom *__restrict__ Qf = fa.Q + (size_t)fl * (size_t)a.N;
        uint4 *tq = tqb + jb * FAST_TILE;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int k = r * 256 + wave * 64 + lane;
            if (r * 256 + wave * 64 < cntj4) dma_1k(Qf + tj.start + min(k, cntj - 1), tq + r * 256 + wave * 64);
        }
    };
    // centre sub-tile `sub` of frame fl into centre buffer cb -- waves 0/1
    auto stage_c = [&](int fl, int sub, int cb) {
        const QAtom *__restrict__ Qf = fa.Q + (size_t)fl * (size_t)a.N;
        const int cnt = min(FAST_SUB, ti.count - sub * FAST_SUB);
        if (wave < 2 && wave * 64 < cnt)
            dma_1k(Qf + ti.start + sub * FAST_SUB + min(wave * 64 + lane, cnt - 1), tcb + cb * FAST_SUB + wave * 64);
    };

    // PLAN: a lane's two centres of sub-tile `sub` of frame fl from the quantised frame (resident in the XCD's L2 by the chunk
    // mapping) straight into registers, two 16-byte loads with the indices stage_c clamps: a record is read once per step and
    // kept for the whole step, so a copy in LDS buys nothing, and without the centre buffers a sixth workgroup fits the CU
    auto load_c = [&](int fl, int sub, uint4 &ra, uint4 &rb) {
        const uint4 *__restrict__ Qc = reinterpret_cast<const uint4 *>(fa.Q + (size_t)fl * (size_t)a.N + ti.start + sub * FAST_SUB);
        const int cnt = min(FAST_SUB, ti.count - sub * FAST_SUB);
        ra = Qc[min(la, cnt - 1)];
        rb = Qc[min(lb, cnt - 1)];
    };

    // PLAN: bit 4 (fl - f0) + sub of `live` = that step is still to run; the records of this work item's chunk
    // (read through the constant address space, so that a step's record arrives by one scalar load that the step before
    //  issued: as an ordinary load it is a vector load, a wait and three v_readfirstlane behind every barrier)
    typedef uint32_t plan_rec_t __attribute__((ext_vector_type(4)));
    typedef const plan_rec_t __attribute__((address_space(4))) *plan_ptr_t;
    unsigned long long live = 0ull;
    const uint4 *__restrict__ plan_wg = nullptr;
    plan_ptr_t plan_c = nullptr;
    if constexpr (PLAN) {
        plan_wg = fa.plan + ((size_t)bx * (size_t)fa.nf + (size_t)f0) * TILE_PLAN_MAX_SUBS;
        plan_c = (plan_ptr_t)(uintptr_t)plan_wg;
        bool lv = false;
        if (f0 + (lane >> 2) < f1 && (lane & 3) < nsub)
        {
            const uint32_t flags = plan_wg[lane].z >> 16;
            lv = (fa.plan_noskip || (flags & TILE_PLAN_LIVE) != 0u) && (KIND == 0 || ((flags & TILE_PLAN_ZF) != 0u) == (KIND == 1));
        }
        live = __ballot(lv);
        if (live == 0ull) return;       // (nothing to zero, nothing to flush)
        for (int k = tid; k < nbins; k += FAST_THREADS) hist[k] = 0u;
    }
    const int nsteps = PLAN ? 1 : (f1 - f0) * nsub;      // (PLAN: the step loop runs until `live` is empty)
    if (QUEUE && tid < 3) nq_count[tid] = 0u;
    const double *p_prev = nullptr, *g_prev = nullptr;
    int gi_prev = 0;
    int fl = f0, sub = 0;
    int jbp = 0, fl_j = -1;         // PLAN: the J buffer in use and the frame it holds
    plan_rec_t rec_next = {0u, 0u, 0u, 0u};
    if constexpr (PLAN) {
        const int bit = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
        fl = f0 + (bit >> 2); sub = bit & 3;
        rec_next = plan_c[bit];
    }
    if (nsteps > 0) {
        stage_j(fl, 0);
        if constexpr (!PLAN) stage_c(fl, sub, 0);
    }
    float sc[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    double sc64r[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    TriConst trc = {0.0f, 0.0f, 0.0f, 0.0f, 0u, 0u};
    float near_f[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    uint32_t cull_gap = 0u;
    // PLAN: "one cell per frame" as a word (0 / 1) the compiler cannot turn back into a lane mask: two scalar registers less
    // across the quad loops, and they were spilled ones
    int cell_step = PLAN ? __builtin_amdgcn_readfirstlane(a.n_cells == 1 ? 0 : 1) : 0;
    int nb_lds = nbins;
    // PLAN: the end of the own block, min(qe, own_add + (sub + 1) own_mul), from two words instead of two lane masks (diagonal
    // tile pair? AMOF_RDF_NOREACH?): 0 + 0 off the diagonal, 0 + 128 (sub + 1) on it, 2^20 + 0 when every quad is masked
    int own_mul = PLAN ? __builtin_amdgcn_readfirstlane(diag && !fa.noreach ? FAST_SUB : 0) : 0;
    int own_add = PLAN ? __builtin_amdgcn_readfirstlane(diag && fa.noreach ? 1 << 20 : 0) : 0;
    for (int step = 0; PLAN ? live != 0ull : step < nsteps; step++) {
        // PLAN: steps count the live ones; the first live step of a frame turns to the other J buffer
        if constexpr (PLAN) {       // (the step in hand is the lowest bit of `live`: nothing but the mask is carried from step to step)
            const int bit = __builtin_amdgcn_readfirstlane(__ffsll((long long)live) - 1);
            fl = f0 + (bit >> 2); sub = bit & 3;
        }
        const bool new_frame = PLAN && fl != fl_j;
        const bool first = PLAN ? fl_j < 0 : step == 0;
        if constexpr (PLAN) {
            // The work item's own constants pass through an empty statement once per step.  What the compiler derives from them
            // -- lane masks of scalar conditions, 64-bit byte offsets, the staging indices -- is then made where a step uses it,
            // by a few scalar instructions, instead of once in front of the loop: carried across the quad loops it sat in
            // spilled scalar registers, a v_readlane_b32 per word and step (profiles/r14/tile_step_state.txt)
            asm volatile("" : "+s"(wave), "+s"(cntj), "+s"(ti.start), "+s"(ti.count), "+s"(tj.start), "+s"(cell_step), "+s"(nb_lds),
                         "+s"(own_mul), "+s"(own_add), "+s"(f0));
            cntj4 = (cntj + 3) & ~3;
            full = cntj & ~3;
            tqb = reinterpret_cast<uint4 *>(hist0 + ((nb_lds + FAST_TRASH + 2 + (SAT ? 1 : 0) + 3) & ~3));      // (the LDS layout at the top of the kernel)
        }
        if (PLAN && new_frame) { if (fl_j >= 0) jbp = __builtin_amdgcn_readfirstlane(jbp ^ 1); fl_j = fl; }
        const unsigned long long rest = live & (live - 1ull);          // PLAN: the live steps behind this one
        const plan_rec_t rec = rec_next;
        const int jb = PLAN ? jbp : (fl - f0) & 1, cbuf = step & 1;
        const int cnti = min(FAST_SUB, ti.count - sub * FAST_SUB);     // centre atoms of this sub-tile
        const int ia = sub * FAST_SUB + la, ib = ia + 1;               // indices in tile I
        const bool has_a = la < cnti, has_b = lb < cnti;
        const int f = fa.f_base + fl;
        // (PLAN: the positions, the cell record and the partner segment are addressed where a level-3 refinement reads them: `late`)
        const double *__restrict__ p = PLAN ? nullptr : a.pos + (size_t)f * (size_t)a.N * 3;
        const uint4 *tq = tqb + jb * FAST_TILE, *tc = tcb + (PLAN ? 0 : cbuf * FAST_SUB);
        const int gi = PLAN ? 0 : (a.n_cells == 1 ? 0 : f);     // (PLAN: used by the cell's constants only, below)
        const FrameScale *__restrict__ fs = PLAN ? nullptr : fa.fs + gi;
        const double *__restrict__ g = PLAN ? nullptr : a.geom + (size_t)gi * GEOM_STRIDE;
        const LateRefs late = {fl, tj.start};
        // wave-uniform per-cell constants: kept in scalar registers; a constant cell's are read once, at the first step
        // (per step they cost ~20 v_readfirstlane and a global-memory latency at the head of every step)
        if (first || (PLAN ? cell_step != 0 : a.n_cells != 1)) {
            if constexpr (PLAN) {
                // (the table's address and the batch's first frame from the kernel's arguments, read again here: neither is
                //  held in a scalar register across the steps of a constant cell)
                rdf_kernarg_t ka = (rdf_kernarg_t)__builtin_amdgcn_kernarg_segment_ptr();
                asm volatile("" : "+s"(ka));
                fs = ka->fs + (cell_step != 0 ? ka->f_base + fl : 0);
            }
            cull_gap = __builtin_amdgcn_readfirstlane(fs->cull_gap);
#pragma unroll
            for (int k = 0; k < 9; k++)
                sc[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->sc[k])));
            // the f64 scales of the level-2 refinement: diagonal cells keep their three in scalar registers (a vector load
            // at the head of every refinement visit costs a memory latency each time)
            if (ORTHO) {
#pragma unroll
                for (int k = 0; k < 3; k++) sc64r[k] = uniform_f64(fs->sc64[k]);
            }
            if constexpr (SATS) sat = sat_lane(nb_lds, lane, sc64r[0], sc64r[1]);
            if (TRI >= 0) {     // L00, L10, L11, L22 of the level-2 form (rdf_pair_refine_tri): a load at the head of every visit would cost its latency
                sc64r[0] = uniform_f64(fs->sc64[0]); sc64r[3] = uniform_f64(fs->sc64[3]);
                sc64r[4] = uniform_f64(fs->sc64[4]); sc64r[8] = uniform_f64(fs->sc64[8]);
                trc.c10 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->tri_c10)));
                trc.near_y = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->tri_near_y)));
                trc.near_z = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->tri_near_z)));
                trc.near_x = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fs->tri_near_x)));
                trc.kx = __builtin_amdgcn_readfirstlane(fs->tri_kx);
                trc.ky = __builtin_amdgcn_readfirstlane(fs->tri_ky);
            }
            if (IMG) {
#pragma unroll
                for (int k = 0; k < 3; k++) {
                    const uint32_t tk = __builtin_amdgcn_readfirstlane(fs->near_t[k]);
                    near_f[k] = tk != 0x7fffffffu ? __uint_as_float(__float_as_uint(__uint2float_rd(tk)) - 1u) : __builtin_inff();
                }
            }
        }
        const double *sc64 = (ORTHO || TRI >= 0) ? sc64r : fs->sc64;
        uint4 ca, cb;
        if constexpr (PLAN) {
            // this step's centres: no register is held across the quad loops for them (issued behind the last quad loop
            // of the step before, they were 0.25 ms slower: profiles/r13/tile_six.txt)
            load_c(fl, sub, ca, cb);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's DMA for this step has landed
        __syncthreads();                                    // everyone's has; the previous step is fully consumed
        if (QUEUE) {
            // what the previous step parked is complete (barrier above): dense canonical pass, one pair per lane,
            // while this step parks into the other buffer; the counter of step + 1 was last read a step ago
            if (tid == 0) nq_count[(step + 1) % 3] = 0u;
            if (fa.img_defer && step > 0) {
                const uint2 *nqp = nq_base + (size_t)((step - 1) & 1) * nq_cap;
                const int npark = (int)min(nq_count[(step - 1) % 3], nq_cap);
                for (int e = tid; e < npark; e += FAST_THREADS) {
                    const uint2 pr2 = nqp[e];
                    rdf_pair_images<ORTHO>(hist, fa, g_prev, p_prev, pr2.x, pr2.y, gi_prev);
                }
            }
            p_prev = p; g_prev = g; gi_prev = gi;
        }
        uint2 *nq = nq_base + (fa.img_defer ? (size_t)(step & 1) * nq_cap : 0);
        // what the next step needs streams in behind the arithmetic
        if constexpr (PLAN) {
            // the next frame with a live step (buffer jb^1: the frame before this one, consumed before this barrier)
            const unsigned long long later = rest & ~(0xfull << (4 * (fl - f0)));
            if (new_frame && later) stage_j(f0 + ((__ffsll((long long)later) - 1) >> 2), jb ^ 1);
        } else {
            const int nsub_next = sub + 1 < nsub ? sub + 1 : 0;
            const int fl_next = sub + 1 < nsub ? fl : fl + 1;
            if (step + 1 < nsteps) stage_c(fl_next, nsub_next, cbuf ^ 1);
            if (sub == 0 && fl + 1 < f1) stage_j(fl + 1, jb ^ 1);   // (buffer jb^1: frame fl-1, consumed before this barrier)
        }
        if constexpr (!PLAN) { ca = tc[min(la, cnti - 1)]; cb = tc[min(lb, cnti - 1)]; }
        const uint32_t uax = ca.x, uay = ca.y, uaz = ca.z, ida = ca.w;
        const uint32_t ubx = cb.x, uby = cb.y, ubz = cb.z, idb = cb.w;
        // Partner index range(s) to visit.  Tile J is slab-sorted along the stored .z axis, so
        // the partners within reach of the centre atoms (slab distance <= cull_gap, circular)
        // form at most two contiguous index ranges, found once per frame.
        int rb0 = diag ? (sub * FAST_SUB) : 0, re0 = cntj, rb1 = 0, re1 = 0;
        bool zf = false;          // this step has quads that run on f32 slab coordinates (ZF kernels)
        uint32_t z0 = 0u;         // their origin: the middle of the centre sub-tile's slab range
        int mz[2] = {0, 0};       // TRI: cells of slab wrap between the centres and the ZF partners of piece 0 / 1
        bool touch = false;       // TRI: the two pieces of a wrapped reach touch; [sa, sb) = the quads that straddle them
        int sa = 0, sb = 0;
        // quad ranges [b, e) of this step, quads dealt round-robin to the four waves: zq on f32 slab coordinates,
        // iq on the integer slab differences
        int zqb[2] = {0, 0}, zqe[2] = {0, 0}, iqb[2] = {0, 0}, iqe[2] = {0, 0};
        if constexpr (PLAN) {
            // the step's record: quad ranges as tile_plan_window made them, the centres' slab range, the ZF flag
            const uint32_t s_first = rec.z & 255u, s_last = (rec.z >> 8) & 255u;
            const uint32_t wlo = s_first << 24, whi = (s_last << 24) | 0xffffffu;
            zf = KIND == 0 ? ((rec.z >> 16) & TILE_PLAN_ZF) != 0u : KIND == 1;      // (KIND: `live` holds steps of one form only)
            z0 = wlo + ((whi - wlo) >> 1);
            (zf ? zqb : iqb)[0] = (int)(rec.x & 0xffffu); (zf ? zqe : iqe)[0] = (int)(rec.x >> 16);
            (zf ? zqb : iqb)[1] = (int)(rec.y & 0xffffu); (zf ? zqe : iqe)[1] = (int)(rec.y >> 16);
        } else if (CULL || ZFK) {
            // the sub-tile is slab-sorted: its first / last atoms give its slab range
            const uint32_t s_first = tc[0].z >> 24, s_last = tc[cnti - 1].z >> 24;
            const uint32_t wlo = s_first << 24, whi = (s_last << 24) | 0xffffffu;
            const uint32_t W = whi - wlo;
            // every lane samples two quads of tile J; ballots give the boundary quads
            const int q0 = lane, q1 = lane + 64;     // FAST_TILE / 4 = 128 quads
            const uint32_t l0 = tq[min(4 * q0 + 3, cntj - 1)].z >> 24, l1 = tq[min(4 * q1 + 3, cntj - 1)].z >> 24;
            const uint32_t h0 = tq[min(4 * q0, cntj - 1)].z >> 24, h1 = tq[min(4 * q1, cntj - 1)].z >> 24;
            auto first_set = [&](bool g0, bool g1) {
                const unsigned long long m0 = __ballot(g0), m1 = __ballot(g1);
                const int fq = m0 ? __ffsll((long long)m0) - 1 : (m1 ? 64 + __ffsll((long long)m1) - 1 : 128);
                return min(4 * fq, cntj);
            };
            if (CULL) {
                const uint32_t G = cull_gap;
                // reachable keys: [wlo - G, whi + G] (mod 2^32), widened to whole slabs (2^24 each)
                const unsigned long long span = (unsigned long long)W + 2ull * G + (2ull << 24);
                if (G != 0u && span < (1ull << 32)) {
                    const uint32_t klo = wlo - G, khi = whi + G;
                    const uint32_t slo = klo >> 24, shi = khi >> 24;
                    // a_: start of the first quad whose LAST partner has slab >= slo
                    // b_: start of the first quad whose FIRST partner has slab > shi
                    const int a_ = first_set(4 * q0 >= cntj || l0 >= slo, 4 * q1 >= cntj || l1 >= slo);
                    const int b_ = first_set(4 * q0 >= cntj || h0 > shi, 4 * q1 >= cntj || h1 > shi);
                    if (klo <= khi) {
                        rb0 = max(rb0, a_); re0 = b_;
                    } else if (b_ < a_) {      // wrapped reach: keys <= khi or >= klo
                        re0 = b_;
                        rb1 = max(rb0, a_); re1 = cntj;
                        // (piece 0 = the keys <= khi: a cell below the centres when whi + G ran over; piece 1 = the keys
                        //  >= klo: a cell above them when wlo - G ran under)
                        if (khi < whi) mz[0] = -1;
                        if (wlo < G) mz[1] = 1;
                    } else if (TRI >= 0) {
                        // the two pieces touch (no partner in the gap, or the tile lies inside one of them).  TRI needs the
                        // slab wrap of a piece: quads before a_ hold keys <= khi only (or the gap), quads from b_ on keys >=
                        // klo only; the quads in between (b_ >= a_) straddle both and take the integer path
                        touch = true;
                        re0 = a_;
                        rb1 = max(rb0, b_); re1 = cntj;
                        sa = max(rb0, a_); sb = b_;
                        if (khi < whi) mz[0] = -1;
                        if (wlo < G) mz[1] = 1;
                    }                          // else the two pieces touch: whole tile
                    if (ZFK) {
                        // f32 slab coordinates are valid when no slab difference of a partner inside the reach window and
                        // a centre can wrap: |z_j - z0| <= G + W/2 + 2^24 + 1, |z_i - z0| <= W/2 + 1, their difference
                        // below 2^31 in magnitude -- then it IS the minimum image.  A partner outside the window (quads are
                        // visited whole) comes out beyond G either way round, i.e. out of range.  W < 2^28 is the span
                        // the host's error bound (fast_guard_zf) assumes.
                        zf = W < (1u << 28) && (unsigned long long)G + W + (2ull << 24) < (1ull << 31);
                        z0 = wlo + (W >> 1);
                    }
                }
                int qbr[2], qer[2];
#pragma unroll
                for (int r = 0; r < 2; r++) {
                    const int rb = r == 0 ? rb0 : rb1, re = r == 0 ? re0 : re1;
                    qbr[r] = rb & ~3;
                    qer[r] = re <= rb ? 0 : (re + 3) & ~3;
                    if (r == 1) qbr[r] = max(qbr[r], (max(re0, rb0) + 3) & ~3);   // never visit a quad twice
                    (zf ? zqb : iqb)[r] = qbr[r];
                    (zf ? zqe : iqe)[r] = qer[r];
                }
                if (TRI >= 0 && touch) {
                    if (zf) {               // (the integer ranges are free in a ZF step)
                        iqb[0] = sa & ~3; iqe[0] = sb <= sa ? 0 : (sb + 3) & ~3;
                    } else {                // everything on the integer path: one range
                        iqb[0] = rb0 & ~3; iqe[0] = (cntj + 3) & ~3;
                        iqb[1] = 0; iqe[1] = 0;
                    }
                }
            } else {
                // No culling (the cutoff reaches across the slab axis: cubic cells at the default cutoff): every quad is
                // visited, and the f32 slab coordinates still hold for all partners but a band around the antipode of
                // the sub-tile, where the wrap depends on the centre.  G2 = the largest reach they allow; a ZF quad may
                // only hold partners inside the window (here a partner outside is NOT out of range), so the window is
                // cut at whole quads from the inside: a2 = first quad whose FIRST partner has slab >= slo, b2 = first
                // quad whose LAST partner has slab > shi.  The band (>= 4 slabs wide) and the straddling quads take the
                // integer path.
                const int start = rb0, endq = (cntj + 3) & ~3;          // (start is a multiple of 4)
                iqb[0] = start; iqe[0] = endq;
                if (W < (1u << 28)) {
                    const uint32_t G2 = 0x7fffffffu - W - (2u << 24) - 2u;
                    const uint32_t klo = wlo - G2, khi = whi + G2;
                    const uint32_t slo = klo >> 24, shi = khi >> 24;
                    const int a2 = first_set(4 * q0 >= cntj || h0 >= slo, 4 * q1 >= cntj || h1 >= slo);
                    const int b2 = first_set(4 * q0 >= cntj || l0 > shi, 4 * q1 >= cntj || l1 > shi);
                    auto up4 = [](int x) { return (x + 3) & ~3; };
                    zf = true;
                    z0 = wlo + (W >> 1);
                    if (klo <= khi) {              // window = slabs [slo, shi]: ZF quads [a2, b2)
                        zqb[0] = max(start, a2); zqe[0] = up4(b2);
                        iqb[0] = start; iqe[0] = min(max(start, a2), endq);
                        iqb[1] = max(start, up4(b2)); iqe[1] = endq;
                    } else {                       // window = slabs [0, shi] and [slo, 255]: ZF quads [0, b2) and [a2, end)
                        zqb[0] = start; zqe[0] = up4(b2);
                        zqb[1] = max(start, a2); zqe[1] = endq;
                        iqb[0] = max(start, up4(b2)); iqe[0] = min(max(start, a2), endq);
                        if (khi < whi) mz[0] = -1;
                        if (wlo < G2) mz[1] = 1;
                    }
                }
            }
        } else {
            iqb[0] = rb0 & ~3;
            iqe[0] = (re0 + 3) & ~3;
        }
        float zaf = 0.0f, zbf = 0.0f;
        if (ZFK && zf) {
            // each wave converts the slab coordinate of the partners it is about to meet on the ZF path (its own quads
            // of both pieces) into bins relative to z0, one rounding (f64 product -> f32), and parks it in the LDS
            // copy's .w; centre atoms likewise, in registers.  Wave-local: LDS operations of a wave execute in order.
            const double cz = TRI >= 0 ? sc64[8] : sc64[2];
            uint4 *tqw = tqb + jb * FAST_TILE;
#pragma unroll 1
            for (int r = 0; r < 2; r++) {
                for (int j = zqb[r] + 4 * wave + 16 * (lane >> 2) + (lane & 3); j < zqe[r]; j += 256)
                    tqw[j].w = __float_as_uint((float)((double)(int)(tqw[j].z - z0) * cz));
            }
            zaf = has_a ? (float)((double)(int)(uaz - z0) * cz) : __builtin_inff();
            zbf = has_b ? (float)((double)(int)(ubz - z0) * cz) : __builtin_inff();
            if constexpr (SATS) { zaf = sat_centre(zaf, sat.invC); zbf = sat_centre(zbf, sat.invC); }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        const QAtom *__restrict__ qseg = PLAN ? nullptr : fa.Q + (size_t)fl * (size_t)a.N + tj.start;
        LaneQueue lq = {QUEUE_EMPTY, QUEUE_EMPTY, 0.0f, 0.0f};
        auto run = [&](auto zf_tag, const int *qbr, const int *qer) {
            constexpr bool ZF = decltype(zf_tag)::value;
#pragma unroll 1
            for (int r = 0; r < 2; r++) {
                const int qb = qbr[r], qe = qer[r];
                if (qe <= qb) continue;
                const int qe_full = min(qe, full);
                if (TRI >= 0) {
                    // ZF quads: the piece's slab wrap goes onto the centres' folded coordinates; integer quads correct per pair
                    const uint32_t kxm = ZF ? (uint32_t)mz[r] * trc.kx : 0u, kym = ZF ? (uint32_t)mz[r] * trc.ky : 0u;
                    const uint32_t cax = uax + kxm, cay = uay + kym, cbx = ubx + kxm, cby = uby + kym;
                    unsigned *nqc = &nq_count[step % 3];
                    if (diag) {
                        for (int j0 = qb + 4 * wave; j0 < qe; j0 += 16)
                            fast_quad_tri<true, true, ZF, NEAR, XW, HALF>(hist, fa, sc64, sc, trc, tq, j0, cntj, has_a, has_b, ia, ib, half_m_guard,
                                                                cax, cay, uaz, ida, cbx, cby, ubz, idb,
                                                                nq, nqc, nq_cap, g, p, gi, zaf, zbf, qseg, clampv);
                    } else {
                        int j0 = qb + 4 * wave;
                        for (; j0 < qe_full; j0 += 16)
                            fast_quad_tri<false, false, ZF, NEAR, XW, HALF>(hist, fa, sc64, sc, trc, tq, j0, cntj, has_a, has_b, ia, ib, half_m_guard,
                                                                  cax, cay, uaz, ida, cbx, cby, ubz, idb,
                                                                  nq, nqc, nq_cap, g, p, gi, zaf, zbf, qseg, clampv);
                        if (j0 == full && j0 < qe && full < cntj)
                            fast_quad_tri<false, true, ZF, NEAR, XW, HALF>(hist, fa, sc64, sc, trc, tq, full, cntj, has_a, has_b, ia, ib, half_m_guard,
                                                                 cax, cay, uaz, ida, cbx, cby, ubz, idb,
                                                                 nq, nqc, nq_cap, g, p, gi, zaf, zbf, qseg, clampv);
                    }
                    continue;
                }
                if constexpr (REACH) {
                    // (PLAN, ZF quads: a centre that does not exist carries an infinite slab coordinate -- zaf, zbf -- so its candidate
                    //  is infinite with or without the lane's mask, and the masked and the ragged quad need no has_a / has_b)
                    const bool ha = (PLAN && ZF) || has_a, hb = (PLAN && ZF) || has_b;
                    // (a piece starts at or behind the own block's first quad, and a wave keeps its residue across the cut:
                    //  the quads whose slab coordinates it converted)
                    const int own_end = PLAN ? min(qe, own_add + (sub + 1) * own_mul)
                                             : (!diag ? 0 : (fa.noreach ? qe : min(qe, (sub + 1) * FAST_SUB)));
                    const int qe_plain = min(qe, full);
                    int j0 = qb + 4 * wave;
                    if constexpr ((AHEAD & 1) != 0) {
                        // the wave's quads of the piece are j0 = qb + 4 wave + 16 k < qe, whichever of the three loops takes
                        // them: each reads the records of the next one, the last reads its own again (never past the piece),
                        // a wave without a quad reads none
                        // (the kernel has no static LDS: a byte offset into the dynamic part is the LDS address, see bin_count)
                        const unsigned tq_addr = (unsigned)((const unsigned char *)tq - lds_raw);
                        PreRec pre[4];
                        if (j0 >= qe) continue;
                        pre_prime<ZF>(pre, tq_addr + 16u * (unsigned)j0, uax, uay, uaz, ubx, uby, ubz);
                        for (; j0 < own_end; j0 += 16)
                            fast_quad<ORTHO, true, true, IMG, ZF, ZFK, AA, PARK, true, 1, PLAN, SATS && ZF>(hist, fa, sc64, g, sc, tq, j0, cntj, ha, hb, ia, ib,
                                                                                half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                                idb, p, near_f, gi, nq, nullptr, nq_cap, zaf,
                                                                                zbf, qseg, clampv, &lq, pre,
                                                                                tq_addr + 16u * (unsigned)(j0 + 16 < qe ? j0 + 16 : j0), &late, &sat);
                        for (; j0 < qe_plain; j0 += 16)
                            fast_quad<ORTHO, false, false, IMG, ZF, ZFK, AA, PARK, true, 1, PLAN, SATS && ZF>(hist, fa, sc64, g, sc, tq, j0, cntj, ha, hb, ia, ib,
                                                                                  half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                                  idb, p, near_f, gi, nq, nullptr, nq_cap,
                                                                                  zaf, zbf, qseg, clampv, &lq, pre,
                                                                                  tq_addr + 16u * (unsigned)(j0 + 16 < qe ? j0 + 16 : j0), &late, &sat);
                        if (j0 == full && j0 < qe && full < cntj)
                            fast_quad<ORTHO, false, true, IMG, ZF, ZFK, AA, PARK, true, 2, PLAN, SATS && ZF>(hist, fa, sc64, g, sc, tq, full, cntj, ha, hb, ia, ib,
                                                                                 half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                                 idb, p, near_f, gi, nq, nullptr, nq_cap, zaf,
                                                                                 zbf, qseg, clampv, &lq, pre, 0u, &late, &sat);
                        else
                            pre_drain(pre);
                        continue;
                    }
                    for (; j0 < own_end; j0 += 16)
                        fast_quad<ORTHO, true, true, IMG, ZF, ZFK, AA, PARK, true, 0, PLAN, SATS && ZF>(hist, fa, sc64, g, sc, tq, j0, cntj, ha, hb, ia, ib,
                                                                         half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                         idb, p, near_f, gi, nq, nullptr, nq_cap, zaf,
                                                                         zbf, qseg, clampv, &lq, nullptr, 0u, &late, &sat);
                    for (; j0 < qe_plain; j0 += 16)
                        fast_quad<ORTHO, false, false, IMG, ZF, ZFK, AA, PARK, true, 0, PLAN, SATS && ZF>(hist, fa, sc64, g, sc, tq, j0, cntj, ha, hb, ia, ib,
                                                                           half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                           idb, p, near_f, gi, nq, nullptr, nq_cap,
                                                                           zaf, zbf, qseg, clampv, &lq, nullptr, 0u, &late, &sat);
                    if (j0 == full && j0 < qe && full < cntj)
                        fast_quad<ORTHO, false, true, IMG, ZF, ZFK, AA, PARK, true, 0, PLAN, SATS && ZF>(hist, fa, sc64, g, sc, tq, full, cntj, ha, hb, ia, ib,
                                                                          half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                          idb, p, near_f, gi, nq, nullptr, nq_cap, zaf,
                                                                          zbf, qseg, clampv, &lq, nullptr, 0u, &late, &sat);
                    continue;
                }
                if (diag) {
                    for (int j0 = qb + 4 * wave; j0 < qe; j0 += 16)
                        fast_quad<ORTHO, true, true, IMG, ZF, ZFK, AA, PARK>(hist, fa, sc64, g, sc, tq, j0, cntj, has_a, has_b, ia, ib,
                                                                   half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                   idb, p, near_f, gi, nq, &nq_count[step % 3], nq_cap, zaf,
                                                                   zbf, qseg, clampv, &lq);
                } else {
                    int j0 = qb + 4 * wave;
                    for (; j0 < qe_full; j0 += 16)
                        fast_quad<ORTHO, false, false, IMG, ZF, ZFK, AA, PARK>(hist, fa, sc64, g, sc, tq, j0, cntj, has_a, has_b, ia, ib,
                                                                     half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                     idb, p, near_f, gi, nq, &nq_count[step % 3], nq_cap,
                                                                     zaf, zbf, qseg, clampv, &lq);
                    if (j0 == full && j0 < qe && full < cntj)
                        fast_quad<ORTHO, false, true, IMG, ZF, ZFK, AA, PARK>(hist, fa, sc64, g, sc, tq, full, cntj, has_a, has_b, ia, ib,
                                                                    half_m_guard, nb_hi, uax, uay, uaz, ida, ubx, uby, ubz,
                                                                    idb, p, near_f, gi, nq, &nq_count[step % 3], nq_cap, zaf,
                                                                    zbf, qseg, clampv, &lq);
                }
            }
        };
        if constexpr (KIND != 2) {
            if (ZFK && zf) run(std::true_type{}, zqb, zqe);
        }
        if constexpr (KIND != 1) run(std::false_type{}, iqb, iqe);
        if constexpr (PLAN) {
            // the next live step and its record, one scalar load whose latency passes in the queue bodies below: the record is not
            // held across the quad loops (fetched at the head of the step it sat there in four spilled scalar registers)
            live = rest;
            if (rest) rec_next = plan_c[__builtin_amdgcn_readfirstlane(__ffsll((long long)rest) - 1)];
        }
        if (PARK) {
            // the step's parked pairs: one refinement body per queue level, for every lane that has an entry there (the
            // partner's record from the tile's LDS copy again, the centre by the entry's low bit)
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const unsigned code = k == 0 ? lq.pk0 : lq.pk1;
                const float qk = k == 0 ? lq.pq0 : lq.pq1;
                if (code != QUEUE_EMPTY) {
                    const int j = (int)(code >> 1);
                    const bool isb = (code & 1u) != 0u;
                    const uint4 qr = tq[j];
                    rdf_pair_refine<ORTHO, ZFK, AA, PLAN, SATS>(hist, fa, sc64, g, qk, isb ? ubx : uax, isb ? uby : uay, isb ? ubz : uaz, qr, p,
                                                          isb ? idb : ida, qseg, j, &late);
                }
            }
        }
        if (QUEUE && !fa.img_defer) {
            // large shares: dense canonical pass over this step's parked pairs right away (one more barrier per step)
            __syncthreads();
            const int npark = (int)min(nq_count[step % 3], nq_cap);
            for (int e = tid; e < npark; e += FAST_THREADS) {
                const uint2 pr2 = nq[e];
                rdf_pair_images<ORTHO>(hist, fa, g, p, pr2.x, pr2.y, gi);
            }
        }
        if constexpr (!PLAN) {
            if (++sub == nsub) { sub = 0; fl++; }
        }
    }
    if (QUEUE && fa.img_defer && nsteps > 0) {   // the last step's parked pairs
        __syncthreads();
        const uint2 *nqp = nq_base + (size_t)((nsteps - 1) & 1) * nq_cap;
        const int npark = (int)min(nq_count[(nsteps - 1) % 3], nq_cap);
        for (int e = tid; e < npark; e += FAST_THREADS) {
            const uint2 pr2 = nqp[e];
            rdf_pair_images<ORTHO>(hist, fa, g_prev, p_prev, pr2.x, pr2.y, gi_prev);
        }
    }
    __syncthreads();
    unsigned long long *U = a.U + ((size_t)ti.species * a.S + tj.species) * (size_t)nbins;
    for (int k = tid; k < nbins; k += FAST_THREADS) {
        unsigned v = hist[k];
        if (v) atomicAdd(&U[k], (unsigned long long)v);
    }
