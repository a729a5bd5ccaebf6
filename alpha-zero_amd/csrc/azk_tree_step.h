// azk_tree_step.h - the body of k_tree (azk_tree.hip), which includes it once per kernel definition: the kernels without FORCED and the ones
// with it are two overloads (the second takes one more argument block), and the first must keep the device code it had before the option
// existed - a body shared through a __forceinline__ function does not (the inliner hands the scheduler another instruction order;
// tools/compare_kernel_isa.py), the same text compiled in place does.  In scope here: the template parameters EXPAND, SELECT, DBG, MULTI,
// KSL, a constant FORCED, the kernel arguments dd, logits, values, and AZK_TREE_FORCED_ARG = the ForcedDev block (read under FORCED only);
// a constant GUMBEL and AZK_TREE_GUMBEL_ARG = the GumbelDev block (read under GUMBEL only), the third overload's;
// a constant PUCT and AZK_TREE_PUCT_ARG = the PuctDev block (read under PUCT only), the fourth overload's;
// a constant SOLVER and AZK_TREE_SOLVER_ARG = the SolverDev block (read under SOLVER only), the fifth overload's.
    const Dev &d = dd;
    const int ablate = DBG ? dd.ablate : 0;
    const int g = blockIdx.x;
    const int lane0 = azk_lane();
    const GameDesc &gd = d.g;
    const int A = gd.action_dim, rc = gd.rc;
    const size_t base = (size_t)g * (size_t)d.cap;
    LdsView L = carve_at(d.lds_off, d.table_size, d.g.rc);
    const bool wrec = DBG && (ablate & 8192) != 0;      // debug only: ONE record per game and launch (overwritten), for the distribution of wave times
    const bool stamp = (ablate & 16) != 0 || wrec;
    long long t0 = stamp ? clock64() : 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
    constexpr bool TWO = !MULTI;
    if constexpr (TWO) {
        if (uniform_i32((int)(threadIdx.x >> 6)) != 0) {             // wave-uniform: the role split is a scalar branch
            if constexpr (EXPAND) {
                if constexpr (GUMBEL) tree_expand_wave<DBG, KSL, TreeGumbelHook>(d, L, logits, values, ablate, AZK_TREE_GUMBEL_ARG);
                else if constexpr (FORCED) tree_expand_wave<DBG, KSL, TreeForcedHook>(d, L, logits, values, ablate);
                else if constexpr (PUCT) tree_expand_wave<DBG, KSL, TreePuctHook>(d, L, logits, values, ablate);
                else if constexpr (SOLVER) tree_expand_wave<DBG, KSL, TreeSolverHook>(d, L, logits, values, ablate, GumbelDev{}, AZK_TREE_SOLVER_ARG);
                else tree_expand_wave<DBG, KSL>(d, L, logits, values, ablate);
            }
            // every store above has been acknowledged and the hand-off words are in LDS before the barrier (the workgroup-scope
            // release alone leaves vmcnt open on this target: one CU's vector memory operations are performed in issue order)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
            __builtin_amdgcn_s_barrier();
            return;
        }
    }
    bool joined = false;                                             // wave 0 has executed its barrier
    int prev_leaf_done = -1;                                         // >= 0: leaf_node still names the leaf wave 1 expands (cleared at the end unless a new leaf was written)
    int bar_phase = 0, prev_leaf_rec = -1;                           // wrec: where wave 0 met the barrier (1 walk, 2 before the leaf writes, 3 at its end)
    long long bar_wait = 0, w1_end = 0;                              // wrec: cycles wave 0 spent at the barrier; wave 1's clock at its own
    auto join = [&](int phase) {                                     // wave 0's one barrier; behind it the hand-off words are wave 1's
        const long long ta = wrec ? clock64() : 0;
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
        if (wrec) { bar_wait += clock64() - ta; bar_phase = phase; }
        joined = true;
    };
    int rec_type = -1, rec_depth = 0, rec_env = 0;   // wrec: -1 idle game, 0 terminal leaf, 1 eval-cache hit, 2 leaf for the evaluator
    int done_sims = MULTI ? d.sims_done[g] : 0;
    const int sim_target = MULTI ? d.budget[0] : 0, max_iter = MULTI ? d.budget[1] : 1;
    // a launch lasts as long as its slowest wave: a game whose simulation needed no evaluator starts another one only while the launch is
    // YOUNG (budget[2] ticks of the constant-rate clock; scalar, so the decision is wave-uniform) - a cheap simulation (terminal leaf) then
    // makes room for a second one, an expensive one does not push the wave past the launch's slowest.  Scheduling only: a game's
    // simulations stay in order, the trees do not change.
    const int young = MULTI ? d.budget[2] : 0;
    const long long t_launch = MULTI && young > 0 ? (long long)wall_clock64() : 0;
    double fk = 0.0;                                                 // FORCED: k of this game's search (0: a fast search - no child is ever forced)
    if constexpr (FORCED) {
        int full = 1;
        const ForcedDev &fd = AZK_TREE_FORCED_ARG;
        if (fd.search_full != nullptr) full = uniform_i32((int)fd.search_full[g]);
        fk = full ? fd.k : 0.0;
    }
    auto still_young = [&]() { return young <= 0 || (long long)wall_clock64() - t_launch < (long long)young; };
    for (int it = 0; it < max_iter; it++) {
    // MULTI: the lane index is made opaque per iteration - left alone, the compiler hoists every lane-dependent address of the loop
    // body (the ~40 per-lane loads of a simulation) out of the loop and keeps them live across it: 294 VGPRs, one wave per SIMD,
    // the 2 048 waves of a launch in TWO rounds (measured 63 us for one simulation per launch against 36 us for the plain kernel)
    int lane = lane0;
    if (MULTI) asm volatile("" : "+v"(lane));
    if (MULTI && it > 0) __syncthreads();       // the previous simulation's LDS scratch is free and its tree / leaf writes are done
    // virtual-loss mode (K > 1, opt-in, changes search results): iteration k serves slot k - it expands the slot's pending leaf,
    // then selects a new one with a virtual loss left on its path so that the other slots' selections move elsewhere
    const bool vl = MULTI && d.K > 1;
    const int vi = g * d.K + (vl ? it : 0);

    // ---- every load whose address depends only on the game index is issued here, together: ONE memory round trip for
    //      the pending leaf's record, its path and move list, the game's state and board, and the root header ----
    const bool shared = d.cache_entries && d.cache_shared;
    int e_node, e_slot, e_depth, e_nv, e_top, e_centry, s_done, s_player, s_mc, s_rootf64, r_fc, r_N;
    uint32_t r_meta;
    unsigned cstamp;
    constexpr bool ONE_LOAD = EXPAND && SELECT && !MULTI;
    int uw = 0;
    if (ONE_LOAD) {
        // The fourteen per-game words below are uniform, and left to the compiler they become scalar loads issued in four
        // dependent groups (SGPR pressure) - four round trips before the first branch.  Here lane k fetches word k: ONE vector
        // load, first in the queue, and the words come back through v_readlane.
        const int *up = d.leaf_node + vi;                                 // lane 0 (and every lane without a word of its own)
        up = lane == 1 ? d.leaf_slot + vi : up;
        up = lane == 2 ? d.leaf_depth + vi : up;
        up = lane == 3 ? d.leaf_nmoves + vi : up;
        up = lane == 4 ? d.arena_top + g : up;
        up = (lane == 5 && d.cache_entries) ? d.leaf_cache + vi : up;
        up = (lane == 6 && shared) ? (const int *)d.cache_stamp : up;
        up = lane == 7 ? d.done + g : up;
        up = lane == 8 ? d.to_move + g : up;
        up = lane == 9 ? d.move_count + g : up;
        up = lane == 10 ? d.root_f64 + g : up;
        up = lane == 11 ? &d.H[base].fc : up;
        up = lane == 12 ? &d.H[base].N : up;
        up = lane == 13 ? (const int *)&d.H[base].meta : up;
        uw = *up;
    } else {
        e_node = EXPAND ? d.leaf_node[vi] : -1; e_slot = EXPAND ? d.leaf_slot[vi] : 0; e_depth = EXPAND ? d.leaf_depth[vi] : 0;
        e_nv = EXPAND ? d.leaf_nmoves[vi] : 0; e_top = EXPAND ? d.arena_top[g] : 0;
        e_centry = (EXPAND && d.cache_entries) ? d.leaf_cache[vi] : -1;
        cstamp = shared ? d.cache_stamp[0] : 0u;
        s_done = SELECT ? d.done[g] : 1; s_player = SELECT ? d.to_move[g] : 0; s_mc = SELECT ? d.move_count[g] : 0;
        s_rootf64 = SELECT ? d.root_f64[g] : 0;
        r_fc = SELECT ? d.H[base].fc : -1; r_N = SELECT ? d.H[base].N : 0;
        r_meta = SELECT ? d.H[base].meta : 0u;
    }
    double r_W = 0.0;                                        // PUCT: the root's value sum, beside its N (mode 2's qn at the root)
    bool r_W_stale = false;                                  // ... a long path's backup went through memory: read it again behind it
    if constexpr (PUCT) r_W = d.W[base];
    unsigned long long e_key = 0ull;
    if (EXPAND && MULTI && shared) e_key = d.leaf_key[(size_t)vi * d.key_words + min(lane, d.key_words - 1)];
    // (every per-lane load below is UNCONDITIONAL with a clamped index: a load under a lane predicate - `lane < n ? p[lane] : 0` -
    //  is compiled as a branch around the load plus a wait for its result right behind it, and the eighteen loads of this entry
    //  sequence then cost one memory round trip EACH instead of one together)
    const int e_path = EXPAND ? d.path[(size_t)vi * d.path_cap + min(lane, d.path_cap - 1)] : 0;     // trace nodes 0..63 (deeper ones: below)
    int e_mv[KSL] = {};
    if (EXPAND && MULTI) {                                   // (two-wave kernels: the list belongs to wave 1)
#pragma unroll
        for (int k4 = 0; k4 < KSL; k4++) e_mv[k4] = d.leaf_moves[(size_t)vi * rc + min(lane + AZK_WAVE * k4, rc - 1)];
    }
    // the game's cell codes, four to a register: a row of `cells` is rc_pad bytes (a multiple of 16, zeros past rc), so the board comes in as
    // NCW dword loads per lane instead of KSL byte loads, and goes to LDS - and later out to leaf_cells - the same way
    constexpr int NCW = (KSL * AZK_WAVE / 4 + AZK_WAVE - 1) / AZK_WAVE;
    const int ncw = d.rc_pad >> 2;
    uint32_t s_cw[NCW] = {};
    if (SELECT) {
        const uint32_t *cw = (const uint32_t *)(d.cells + (size_t)g * d.rc_pad);
#pragma unroll
        for (int q = 0; q < NCW; q++) s_cw[q] = cw[min(lane + AZK_WAVE * q, ncw - 1)];
    }
    if (ONE_LOAD) {                                          // (behind the loads that do not depend on them)
        e_node = __builtin_amdgcn_readlane(uw, 0); e_slot = __builtin_amdgcn_readlane(uw, 1); e_depth = __builtin_amdgcn_readlane(uw, 2);
        e_nv = __builtin_amdgcn_readlane(uw, 3); e_top = __builtin_amdgcn_readlane(uw, 4);
        e_centry = d.cache_entries ? __builtin_amdgcn_readlane(uw, 5) : -1;
        cstamp = shared ? (unsigned)__builtin_amdgcn_readlane(uw, 6) : 0u;
        s_done = __builtin_amdgcn_readlane(uw, 7); s_player = __builtin_amdgcn_readlane(uw, 8); s_mc = __builtin_amdgcn_readlane(uw, 9);
        s_rootf64 = __builtin_amdgcn_readlane(uw, 10); r_fc = __builtin_amdgcn_readlane(uw, 11); r_N = __builtin_amdgcn_readlane(uw, 12);
        r_meta = (uint32_t)__builtin_amdgcn_readlane(uw, 13);
    }

    const int prev_leaf = (EXPAND && TWO) ? uniform_i32(e_node) : -1;   // the node wave 1 is expanding (-1: none)
    prev_leaf_done = prev_leaf;
    if (wrec) prev_leaf_rec = prev_leaf;
    int prev_crow = -1;                                      // shared eval cache: the entry wave 1 may be rewriting in this launch
    if constexpr (EXPAND && TWO) {
        // wave 0's share of mcts.py:46-60: Node.backup of the previous leaf - the path, the depth and the value, nothing else
        const int node = prev_leaf;
        if (node >= 0) {
            const int slot = uniform_i32(e_slot);
            const int depth = uniform_i32(e_depth);
            const int centry = d.cache_entries ? uniform_i32(e_centry) : -1;
            const bool hit = d.cache_entries && centry >= 0;
            const size_t crow = shared ? (size_t)(hit ? centry : -(centry + 1)) : ((size_t)g * d.cache_entries + (hit ? centry : -(centry + 1)));
            if (shared && !hit) prev_crow = -(centry + 1);
            const bool shortpath = depth < AZK_WAVE;
            // (unconditional, the lanes beyond the path read the root: a load under a lane predicate is followed by a wait for it)
            const int bnode = (shortpath && lane <= depth) ? e_path : 0;
            const int bN = d.H[base + bnode].N;
            const double bW = d.W[base + bnode];
            const float vraw = hit ? (shared ? d.hit_value[vi] : d.cache_value[crow]) : values[slot];
            const double v = -(double)vraw;                          // mcts.py:56
            if (shortpath) {                                          // Node.backup (node.py:62-74) on the operands fetched above
                const int nN = bN + 1;
                const double nW = bW + (((depth - lane) & 1) ? -v : v);
                if (lane <= depth) node_store(d, base + e_path, nN, nW);
                if constexpr (PUCT) r_W = tree_readlane_f64(nW, 0);   // (trace node 0 is the root: lane 0 holds its new sum)
            } else {
                backup_path(d, base, d.path + (size_t)vi * d.path_cap, depth, v, false);
                if constexpr (PUCT) r_W_stale = true;
            }
            r_N += 1;                                                 // the root is trace node 0 of every simulation
            if (lane == 0) count_add(d, CNT_TRACE, g, depth + 1);
            // (leaf_node = -1 waits until the barrier is behind this wave: wave 1 reads the word at ITS entry)
        }
        azk_wave_sync();   // this wave's tree writes are visible to its own SELECT reads below
        if constexpr (PUCT) { if (r_W_stale) r_W = d.W[base]; }
    }
    if constexpr (EXPAND && MULTI) {
        const int node = uniform_i32(e_node);
        if (MULTI && node >= 0 && (uniform_i32(e_nv) < 0 ||          // a leaf of the two-wave kernels: its move list was never built
                                   (!(d.cache_entries && uniform_i32(e_centry) >= 0) && ((!vl && it > 0) || logits == nullptr)))) {
            if (lane == 0) atomicExch(d.err, AZK_ERR_STATE);          // ... or a pending evaluation without its logits: caller error
            break;
        }
        if (node >= 0) {
            const bool xst = (ablate & 1024) != 0;              // debug only: cycle stamps of the expansion's sub-phases
            long long x0 = 0, x1 = 0, x2 = 0, x3 = 0, x4 = 0;
            if (xst) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); x0 = clock64(); }
            const int slot = uniform_i32(e_slot);
            const int depth = uniform_i32(e_depth);
            const int nv = uniform_i32(e_nv);
            if (wrec) rec_env = nv;
            const int centry = d.cache_entries ? uniform_i32(e_centry) : -1;
            const bool hit = d.cache_entries && centry >= 0;
            const size_t crow = shared ? (size_t)(hit ? centry : -(centry + 1)) : ((size_t)g * d.cache_entries + (hit ? centry : -(centry + 1)));
            const float *lg = hit ? (shared ? d.hit_logits + (size_t)vi * A : d.cache_logits + crow * A) : logits + (size_t)slot * A;
            unsigned claim_now = 0u;
            if (shared && !hit) claim_now = __hip_atomic_load(d.cache_claim + crow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            // Node.backup operands (trace nodes 0..depth, one per lane) are fetched now, next to the logits: second round trip
            const bool shortpath = depth < AZK_WAVE;
            // (unconditional, the lanes beyond the path read the root: a load under a lane predicate is followed by a wait for it,
            //  which put a whole round trip between these two loads and the logits below)
            const int bnode = (shortpath && lane <= depth) ? e_path : 0;
            const int bN = d.H[base + bnode].N;
            const double bW = d.W[base + bnode];
            // second (and last) round trip of the expansion, all straight-line: logits, value, the node's header, root noise
            // a lane takes FOUR consecutive logits per load (actions 4 lane .. 4 lane + 3 of each block of 256; the lane at the row's end
            // takes the row's last four, overlapping its neighbour - the same values twice): one 16-byte load instead of four 4-byte ones,
            // here and for the eval-cache row's stores and loads below (row_first / row_load4 / row_store4: a row of fewer than four floats
            // goes component by component, as on the expanding wave)
            constexpr int NV4 = (KSL * AZK_WAVE + 255) / 256;
            int la[NV4];                                              // first action of the lane's group
            bool lact[NV4];
            f32x4_a4 lgv[NV4];
#pragma unroll
            for (int q = 0; q < NV4; q++) {
                lact[q] = 256 * q + 4 * lane < A;
                la[q] = row_first(256 * q + 4 * lane, A);
                lgv[q] = row_load4(lg, la[q], A);
            }
            const float vraw = hit ? (shared ? d.hit_value[vi] : d.cache_value[crow]) : values[slot];
            const uint32_t node_meta = d.H[base + node].meta;
            const bool mix = depth == 0 && d.noise != nullptr;        // mcts.py:42-43,52-53
            double nzv[KSL] = {};
            if (mix) {
                // asynchronous moves keep two rows per game - the current search's and the next one's, generated a whole search ahead
                // (k_noise_ahead) - and the slot's move counter says which is which
                const size_t nrow = (MULTI && d.noise_sel != nullptr) ? (size_t)g * 2 + (size_t)(uniform_i32((int)d.noise_sel[g]) & 1) : (size_t)g;
#pragma unroll
                for (int k4 = 0; k4 < KSL; k4++) {
                    const int i = lane + AZK_WAVE * k4;
                    nzv[k4] = d.noise[nrow * A + azk_action_idx(gd, i < nv ? e_mv[k4] : 0)];   // (a lane's e_mv beyond nv is stale memory)
                }
            }
            bool cache_write = d.cache_entries && !hit;               // MCTS.cache[board_key] = (...)  (mcts.py:51)
            if (shared && !hit) {
                // one writer per entry and launch: the claim word moves to this launch's stamp by compare-and-swap; an entry
                // already claimed in this launch (by any game) is left alone.  The round trip hides under the softmax below.
                const unsigned cur = (unsigned)uniform_i32((int)claim_now);
                unsigned got = cur;
                if (cur != cstamp && lane == 0) got = atomicCAS(d.cache_claim + crow, cur, cstamp);
                cache_write = cur != cstamp && (unsigned)uniform_i32((int)got) == cur;
                if (cache_write && lane < d.key_words) d.cache_key[crow * d.key_words + lane] = e_key;
            }
            if (xst) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); x1 = clock64(); }
            // float32 softmax, no max subtraction (mcts.py:48-49)
#pragma unroll
            for (int q = 0; q < NV4; q++) {
                if (256 * q >= A) break;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const float ev = (ablate & 1) ? 1.0f : azk_exp_det(lgv[q][c]);
                    if (lact[q] && la[q] + c < A) L.e[la[q] + c] = ev;
                }
            }
            azk_wave_sync();
            if (cache_write) {
                // (behind the exponentials: by now every logit is in its register, and the stores go out back to back - placed
                //  right behind the loads, each store waited for the one before it, one write round trip per 64 actions)
#pragma unroll
                for (int q = 0; q < NV4; q++) if (lact[q]) row_store4(d.cache_logits + crow * A, la[q], A, lgv[q]);
                if (lane == 0) d.cache_value[crow] = vraw;
            }
            if (xst) x2 = clock64();
            const float s = azk_pairwise_sum(L.e, A);
            if (xst) x3 = clock64();
            const int fc = uniform_i32(e_top);
            const bool fits = fc + nv <= d.cap;
            if (fits) {
#pragma unroll
                for (int k4 = 0; k4 < KSL; k4++) {                    // Node.expand (node.py:50-59)
                    const int i = lane + AZK_WAVE * k4;
                    if (i >= nv) break;
                    const int cell = e_mv[k4];
                    const int a = azk_action_idx(gd, cell);
                    const float p = L.e[a] / s;
                    const size_t idx = base + fc + i;
                    d.H[idx] = NodeH{0, p, meta_pack(cell, 0), -1}; d.W[idx] = 0.0;   // (N = 0: Q[idx] stays unwritten - unspecified until the first backup)
                    if constexpr (SOLVER) AZK_TREE_SOLVER_ARG.status[idx] = (uint8_t)SOLVER_UNKNOWN;   // a new node is UNKNOWN whatever the slot held (idx < base + cap: `fits`)
                    if constexpr (GUMBEL) {                           // the child's base score: its raw logit + the game's Gumbel draw for its action
                        if (mix) { const float lga = lg[a]; d.rootP[(size_t)g * rc + i] = (double)lga + nzv[k4]; AZK_TREE_GUMBEL_ARG.logit[(size_t)g * rc + i] = lga; }
                    } else
                    if (mix) d.rootP[(size_t)g * rc + i] = (double)(0.75f * p) + 0.25 * nzv[k4];   // utils.py:24-25
                }
                if constexpr (GUMBEL) { if (mix && lane == 0) AZK_TREE_GUMBEL_ARG.v0[g] = vraw; }
                if constexpr (SOLVER) { if (depth == 0 && lane == 0) AZK_TREE_SOLVER_ARG.status[base + node] = (uint8_t)SOLVER_UNKNOWN; }   // the root becomes UNKNOWN when it is expanded
                if (lane == 0) {
                    d.H[base + node].fc = fc;
                    d.H[base + node].meta = (node_meta & 0xffff0000u) | (uint32_t)nv;
                    d.arena_top[g] = fc + nv;
                    if (depth == 0) d.root_f64[g] = mix ? 1 : 0;
                    count_add(d, CNT_CREATED, g, nv);
                }
                if (node == 0) { r_fc = fc; r_meta = (r_meta & 0xffff0000u) | (uint32_t)nv; s_rootf64 = mix ? 1 : 0; }   // the root header loaded above is stale now
            } else if (lane == 0) {
                atomicExch(d.err, AZK_ERR_ARENA_FULL);
            }
            const double v = -(double)vraw;                          // mcts.py:56
            if (shortpath) {                                          // Node.backup (node.py:62-74) on the operands fetched above
                // virtual-loss mode: the visit was already counted at selection and the value carries the loss (-1) left there
                const int nN = vl ? bN : bN + 1;
                const double nW = bW + (((depth - lane) & 1) ? -v : v) + (vl ? 1.0 : 0.0);
                if (lane <= depth) node_store(d, base + e_path, nN, nW);
                if constexpr (PUCT) r_W = tree_readlane_f64(nW, 0);   // (trace node 0 is the root: lane 0 holds its new sum)
            } else {
                backup_path(d, base, d.path + (size_t)vi * d.path_cap, depth, v, vl);
                if constexpr (PUCT) r_W_stale = true;
            }
            if (!vl) r_N += 1;                                        // the root is trace node 0 of every simulation
            if (xst && lane == 0) {
                x4 = clock64();
                long long *qq = d.dbg + (size_t)g * 8;
                qq[0] += x0 - t0; qq[1] += x1 - x0; qq[2] += x2 - x1; qq[3] += x3 - x2; qq[4] += x4 - x3; qq[6] += 1;
            }
            if (lane == 0) {
                d.leaf_node[vi] = -1;
                count_add(d, CNT_TRACE, g, depth + 1);
            }
        }
        azk_wave_sync();   // this wave's tree writes are visible to its own SELECT reads below
        if constexpr (PUCT) { if (r_W_stale) r_W = d.W[base]; }
    }

    if (SELECT) {
        const bool active = uniform_i32(s_done) == 0;
        if (!active || (MULTI && done_sims >= sim_target)) {          // finished game / simulation budget of this search used up
            if (lane == 0 && (!MULTI || it == 0 || vl)) d.leaf_flag[vi] = 0;
            if (vl) continue;                                         // the other slots may still hold leaves to expand
            break;
        }
        done_sims++;
        if (stamp) t1 = clock64();
#pragma unroll
        for (int q = 0; q < NCW; q++) { const int i = lane + AZK_WAVE * q; if (i < ncw) ((uint32_t *)L.board)[i] = s_cw[q]; }
        const int root_player = uniform_i32(s_player);
        const int root_mc = uniform_i32(s_mc);
        if (lane == 0) L.path[0] = 0;
        azk_wave_sync();
        int node = 0, depth = 0, scanned = 0;
        bool forced_root = false;                                     // FORCED: this simulation's root selection took a forced child (counted below, nothing else)
        // header of the current node, carried in registers: one dependent round trip per level (the child scan itself
        // brings every candidate's header along, and the winner's is taken from the winning lane)
        int fc = uniform_i32(r_fc);
        int Np = uniform_i32(r_N);
        uint32_t nmeta = (uint32_t)uniform_i32((int)r_meta);
        int node_cell = -1;
        bool root_f64 = uniform_i32(s_rootf64) != 0;
        double Wn = r_W;                                              // PUCT: the current node's value sum, carried like Np
        long long seg_a = 0, seg_b = 0, seg_c = 0, seg_d = 0, seg_t = 0;      // debug only (ablate & 64)
        int nst = 0;                                                  // SOLVER: the current node's status, carried like Np (the root's is never looked at)
        int shut_sels = 0;                                            // SOLVER: selections of this simulation that shut a child out (counted below)
        int bst = 0;                                                  // SOLVER, per level: the winner's status, beside bN
        bool open_any = true;                                         // SOLVER, general form of the scan: some child of this node is not LOST
        bool shut_any = false;                                        // ... and this lane shut one of its candidates out
        int stc[4];                                                   // ... and the statuses of the lane's four candidates of a chunk
        for (;;) {                                                    // mcts.py:20-23
            if (TWO && EXPAND && node == prev_leaf && !joined) {
                // the walk stands on the node wave 1 is expanding (the root: at once): the one barrier, then the node's children from
                // the hand-off words - the header in registers was loaded while wave 1 may have been writing it.  A full arena leaves
                // the node a leaf (HO_OK = 0: nothing was written, the header stands).
                join(1);
                if (uniform_i32(L.ho[HO_OK])) {
                    fc = uniform_i32(L.ho[HO_FC]); nmeta = (nmeta & 0xffff0000u) | (uint32_t)uniform_i32(L.ho[HO_NV]);
                    if (node == 0) root_f64 = uniform_i32(L.ho[HO_ROOTF64]) != 0;
                }
            }
            if constexpr (SOLVER) { if (depth > 0 && nst != SOLVER_UNKNOWN) break; }   // a proven node below the root: the simulation ends here
            const int nch = meta_nch(nmeta);
            if (nch <= 0 || (ablate & 2)) break;
            if (ablate & 64) seg_t = clock64();
            const bool f64 = node == 0 && root_f64;
            int gcv = 0;                                              // GUMBEL: the visit count a root child must have to be eligible now
            double gsig = 0.0;                                        // ... and sigma's factor at that count
            if constexpr (GUMBEL) {
                if (f64) {                                            // (a uniform word of (nch, Np): its load goes out with the children's)
                    const GumbelDev &gb = AZK_TREE_GUMBEL_ARG;
                    gcv = gb.table[(size_t)min(gb.m, nch) * gb.n + max(0, min(Np - 1, gb.n - 1))];
                    gsig = (gb.c_visit + (double)gcv) * gb.c_scale;
                }
            }
            double pc = 1.0, qf = 0.0;                                // PUCT: c at this node's Np; an unvisited child's value (until mode 2 has it: the level's FPU parameter)
            int pmode = 0;
            if constexpr (PUCT) {                                     // (a uniform word of Np: its load goes out with the children's)
                const PuctDev &pu = AZK_TREE_PUCT_ARG;
                pc = pu.c_table[min(Np, pu.n_table - 1)];
                qf = node == 0 ? pu.fpu_root : pu.fpu_tree;           // mode 1 as it stands; mode 2 needs the children first (each scan form below); mode 0 never reads it
                pmode = pu.fpu_mode;
            }
            double bW = 0.0;                                          // PUCT: the winner's value sum, beside bN
            double bu64 = 0.0;
            float bu32 = 0.f;
            int best = 0x7fffffff, bN = 0, bfc = -1;
            uint32_t bmeta = 0;
            bool forced_sel = false;                                  // FORCED: the child taken at the root was a forced one (counted, nothing else)
            if constexpr (SOLVER) { bst = 0; open_any = true; shut_any = false; }
            // SOLVER: a child's status byte is loaded beside its header and quotient (unconditional, clamped index: the same round trip).  After
            // the scores: WON -> +inf, LOST -> -inf provided some child is not LOST (one ballot per level), then the argmax as it stands.
            // a child's q = W / (double)N comes from the Q column, where the backup that last changed W left it (node_store_wq: the same division
            // on the same operands, once per backup instead of once per scanned child and level).  Where N = 0 the word is unspecified, and every
            // use of q there is discarded: by the `Nc != 0 ? .. : un` select below, which is all tree_forced_score sees of it, and by
            // tree_gumbel_score's own `N != 0` select.  The PUCT kernels need the winner's W beside its N (bW): they load W and divide, as before.
            const double *const qcol = PUCT ? d.W : d.Q;
            if (nch <= AZK_WAVE && !(ablate & 2048)) {
                // the common case (a Gomoku position has ~50 candidate moves): one candidate per lane, one load per column, the
                // argmax as a DPP maximum + ballot - "first maximum wins" (node.py:47) is the lowest lane holding the maximum
                const bool valid = lane < nch;
                const size_t ci = base + fc + (valid ? lane : 0);
                const NodeH hc = d.H[ci];                             // one 16-byte load: N, P, meta, first_child
                const double Vc = qcol[ci];                           // the child's quotient (PUCT: its value sum)
                int st1 = 0;
                bool s_shut = false;
                if constexpr (SOLVER) {
                    st1 = AZK_TREE_SOLVER_ARG.status[ci];
                    const bool open1 = __ballot(valid & (st1 != SOLVER_LOST)) != 0ull;
                    s_shut = valid & (st1 == SOLVER_LOST) & open1;
                    shut_sels += __ballot(s_shut) != 0ull ? 1 : 0;
                }
                const int Nc = hc.N, fcc = hc.fc;
                const uint32_t mc = hc.meta;
                const float P32 = hc.P;
                unsigned long long winners;
                if (f64) {                                            // root after Dirichlet mixing: float64 priors => float64 UCB
                    const double P64 = d.rootP[(size_t)g * rc + (valid ? lane : 0)];
                    if constexpr (PUCT) { if (pmode == 2) qf = tree_puct_qf2(qf, Wn, Np, tree_puct_mass((valid & (Nc > 0)) ? P64 : 0.0)); }
                    double s = sqrt((double)Np);
                    if constexpr (PUCT) s = pc * s;
                    const double u0 = P64 * s / (double)(Nc + 1);
                    const double q = PUCT ? Vc / (double)Nc : Vc;     // N = 0: unspecified (PUCT: inf/nan), discarded by the select
                    double un = u0;                                   // an unvisited child's score (plain text, no helper call: see the head of this file)
                    if constexpr (PUCT) un = pmode != 0 ? qf + u0 : u0;
                    double u = valid ? tree_gumbel_score<GUMBEL>(tree_forced_score<FORCED>(Nc != 0 ? q + u0 : un, Nc, P64, fk, Np), Nc, q, P64, gcv, gsig) : -__builtin_huge_val();
                    if constexpr (SOLVER) u = (valid & (st1 == SOLVER_WON)) ? __builtin_huge_val() : (s_shut ? -__builtin_huge_val() : u);
                    const double um = wave_max_f64(u);               // (all lanes take part: never under the short-circuit below)
                    winners = __ballot(valid & (u == um));
                    if constexpr (FORCED) forced_sel = um == __builtin_huge_val();
                } else {                                              // float32 priors => float32 UCB (numpy >= 2)
                    if constexpr (PUCT) { if (pmode == 2) qf = tree_puct_qf2(qf, Wn, Np, (double)tree_puct_mass((valid & (Nc > 0)) ? P32 : 0.f)); }
                    float s = (float)sqrt((double)Np);
                    if constexpr (PUCT) s = (float)(pc * sqrt((double)Np));
                    const float u0 = (P32 * s) / (float)(Nc + 1);
                    const float q = (float)(PUCT ? Vc / (double)Nc : Vc);
                    float un = u0;
                    if constexpr (PUCT) un = pmode != 0 ? (float)qf + u0 : u0;
                    float u = valid ? (Nc != 0 ? q + u0 : un) : -__builtin_huge_valf();
                    if constexpr (SOLVER) u = (valid & (st1 == SOLVER_WON)) ? __builtin_huge_valf() : (s_shut ? -__builtin_huge_valf() : u);
                    const float um = wave_max_f32(u);
                    winners = __ballot(valid & (u == um));
                }
                best = __ffsll((long long)winners) - 1;
                bN = Nc; bmeta = mc; bfc = fcc;
                if constexpr (PUCT) bW = Vc;
                if constexpr (SOLVER) bst = st1;
            } else if (nch <= 2 * AZK_WAVE && !(ablate & 2048)) {
                // 65 .. 128 candidates (late plies: every node of the tree): two per lane, the same straight-line shape - ten loads,
                // one round trip.  (The general loop below sinks its prior loads into per-slot branches: one more round trip per
                // 64 candidates, on every level of a late-game walk.)  First maximum wins: indices below 64 before the others.
                const bool va = true, vb = lane + AZK_WAVE < nch;
                const size_t ca = base + fc + lane, cb = base + fc + (vb ? lane + AZK_WAVE : 0);
                const NodeH ha = d.H[ca], hb = d.H[cb];
                const double Va = qcol[ca], Vb = qcol[cb];            // quotients (PUCT: value sums)
                int sta = 0, stb = 0;
                bool shut_a = false, shut_b = false;
                if constexpr (SOLVER) {
                    sta = AZK_TREE_SOLVER_ARG.status[ca]; stb = AZK_TREE_SOLVER_ARG.status[cb];
                    const bool open2 = __ballot((sta != SOLVER_LOST) | (vb & (stb != SOLVER_LOST))) != 0ull;
                    shut_a = (sta == SOLVER_LOST) & open2; shut_b = vb & (stb == SOLVER_LOST) & open2;
                    shut_sels += __ballot(shut_a | shut_b) != 0ull ? 1 : 0;
                }
                const int Na = ha.N, Nb = hb.N, fa = ha.fc, fb = hb.fc;
                const uint32_t ma = ha.meta, mb = hb.meta;
                const float Pa = ha.P, Pb = hb.P;
                unsigned long long wa, wb;
                if (f64) {
                    const double Qa = d.rootP[(size_t)g * rc + lane], Qb = d.rootP[(size_t)g * rc + (vb ? lane + AZK_WAVE : 0)];
                    if constexpr (PUCT) {
                        if (pmode == 2) {                             // (list order inside the lane: child `lane`, then child `lane + 64`)
                            double part = Na > 0 ? Qa : 0.0;
                            part = (vb & (Nb > 0)) ? part + Qb : part;
                            qf = tree_puct_qf2(qf, Wn, Np, tree_puct_mass(part));
                        }
                    }
                    double s = sqrt((double)Np);
                    if constexpr (PUCT) s = pc * s;
                    const double u0a = Qa * s / (double)(Na + 1), u0b = Qb * s / (double)(Nb + 1);
                    const double qa = PUCT ? Va / (double)Na : Va, qb = PUCT ? Vb / (double)Nb : Vb;
                    double una = u0a, unb = u0b;
                    if constexpr (PUCT) { una = pmode != 0 ? qf + u0a : u0a; unb = pmode != 0 ? qf + u0b : u0b; }
                    double ua = tree_gumbel_score<GUMBEL>(tree_forced_score<FORCED>(Na != 0 ? qa + u0a : una, Na, Qa, fk, Np), Na, qa, Qa, gcv, gsig);
                    double ub = vb ? tree_gumbel_score<GUMBEL>(tree_forced_score<FORCED>(Nb != 0 ? qb + u0b : unb, Nb, Qb, fk, Np), Nb, qb, Qb, gcv, gsig) : -__builtin_huge_val();
                    if constexpr (SOLVER) {
                        ua = sta == SOLVER_WON ? __builtin_huge_val() : (shut_a ? -__builtin_huge_val() : ua);
                        ub = (vb & (stb == SOLVER_WON)) ? __builtin_huge_val() : (shut_b ? -__builtin_huge_val() : ub);
                    }
                    const double um = wave_max_f64(fmax(ua, ub));
                    wa = __ballot(va & (ua == um)); wb = __ballot(vb & (ub == um));
                    if constexpr (FORCED) forced_sel = um == __builtin_huge_val();
                } else {
                    if constexpr (PUCT) {
                        if (pmode == 2) {
                            float part = Na > 0 ? Pa : 0.f;
                            part = (vb & (Nb > 0)) ? part + Pb : part;
                            qf = tree_puct_qf2(qf, Wn, Np, (double)tree_puct_mass(part));
                        }
                    }
                    float s = (float)sqrt((double)Np);
                    if constexpr (PUCT) s = (float)(pc * sqrt((double)Np));
                    const float u0a = (Pa * s) / (float)(Na + 1), u0b = (Pb * s) / (float)(Nb + 1);
                    const float qa = (float)(PUCT ? Va / (double)Na : Va), qb = (float)(PUCT ? Vb / (double)Nb : Vb);
                    float una = u0a, unb = u0b;
                    if constexpr (PUCT) { una = pmode != 0 ? (float)qf + u0a : u0a; unb = pmode != 0 ? (float)qf + u0b : u0b; }
                    float ua = Na != 0 ? qa + u0a : una;
                    float ub = vb ? (Nb != 0 ? qb + u0b : unb) : -__builtin_huge_valf();
                    if constexpr (SOLVER) {
                        ua = sta == SOLVER_WON ? __builtin_huge_valf() : (shut_a ? -__builtin_huge_valf() : ua);
                        ub = (vb & (stb == SOLVER_WON)) ? __builtin_huge_valf() : (shut_b ? -__builtin_huge_valf() : ub);
                    }
                    const float um = wave_max_f32(fmaxf(ua, ub));
                    wa = __ballot(va & (ua == um)); wb = __ballot(vb & (ub == um));
                }
                const bool first = wa != 0ull;
                best = first ? __ffsll((long long)wa) - 1 : AZK_WAVE + __ffsll((long long)wb) - 1;
                bN = first ? Na : Nb; bmeta = first ? ma : mb; bfc = first ? fa : fb;
                if constexpr (PUCT) bW = first ? Va : Vb;
                if constexpr (SOLVER) bst = first ? sta : stb;
            } else {
            if constexpr (PUCT) {
                // mode 2 over more than one chunk (a board beyond 256 cells): the mass is needed before the first child is scored, so it takes
                // a pass of its own over (N, P) - one more round trip on such a level; a single chunk sums the registers it has loaded anyway
                if (pmode == 2 && nch > 4 * AZK_WAVE) {
                    double p64 = 0.0;
                    float p32 = 0.f;
                    for (int i = lane; i < nch; i += AZK_WAVE) {
                        const NodeH hk = d.H[base + fc + i];
                        if (f64) { const double P = d.rootP[(size_t)g * rc + i]; p64 = hk.N > 0 ? p64 + P : p64; }
                        else p32 = hk.N > 0 ? p32 + hk.P : p32;
                    }
                    qf = tree_puct_qf2(qf, Wn, Np, f64 ? tree_puct_mass(p64) : (double)tree_puct_mass(p32));
                }
            }
            if constexpr (SOLVER) {
                // more than one chunk (a board beyond 256 cells): "some child is not LOST" is needed before the first child is scored, so it takes a
                // pass of its own over the status bytes; a single chunk asks the registers it has loaded anyway
                if (nch > 4 * AZK_WAVE) {
                    bool mine = false;
                    for (int i = lane; i < nch; i += AZK_WAVE) mine = mine | (AZK_TREE_SOLVER_ARG.status[base + fc + i] != SOLVER_LOST);
                    open_any = __ballot(mine) != 0ull;
                }
            }
            // all of this level's loads are issued before any arithmetic: 4 candidates per lane per 256-child chunk
            for (int c0 = 0; c0 < nch; c0 += 4 * AZK_WAVE) {
                int Nc[4], fcc[4];
                double Vc[4], P64[4] = {0.0, 0.0, 0.0, 0.0};                  // Vc: quotients (PUCT: value sums)
                float P32[4];
                uint32_t mc[4];
                // straight-line loads, no per-slot control flow: a branch inside this loop makes the compiler wait for each
                // slot's prior before issuing the next slot (four serial round trips per level instead of one)
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int i = c0 + lane + AZK_WAVE * k;
                    const size_t ci = base + fc + (i < nch ? i : 0);
                    const NodeH hk = d.H[ci];
                    Nc[k] = hk.N; Vc[k] = qcol[ci]; mc[k] = hk.meta; fcc[k] = hk.fc; P32[k] = hk.P;
                    if constexpr (SOLVER) stc[k] = AZK_TREE_SOLVER_ARG.status[ci];
                }
                if constexpr (SOLVER) {
                    if (nch <= 4 * AZK_WAVE) {                        // the one chunk
                        bool mine = false;
#pragma unroll
                        for (int k = 0; k < 4; k++) mine = mine | ((lane + AZK_WAVE * k < nch) & (stc[k] != SOLVER_LOST));
                        open_any = __ballot(mine) != 0ull;
                    }
                }
                if (f64) {                                            // root after Dirichlet mixing: float64 priors by child position
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int i = c0 + lane + AZK_WAVE * k;
                        P64[k] = d.rootP[(size_t)g * rc + (i < nch ? i : 0)];
                    }
                }
                if (ablate & 64) {   // debug only: time the level's memory round trip separately from its arithmetic
                    const long long ta = clock64();
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    seg_a += clock64() - ta;
                    seg_d += ta - seg_t;                              // (reusing seg_d: issue of the level's loads)
                }
                // branch-free on purpose: every `if` around a division or a compare chain becomes a saveexec/branch pair on
                // this target, and a level of the walk is a few hundred cycles of arithmetic buried under thousands of those
                if constexpr (PUCT) {
                    if (pmode == 2 && nch <= 4 * AZK_WAVE) {          // the one chunk: list order inside the lane is k = 0, 1, 2, 3
                        double p64 = 0.0;
                        float p32 = 0.f;
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const bool in = (lane + AZK_WAVE * k < nch) & (Nc[k] > 0);
                            p64 = in ? p64 + P64[k] : p64; p32 = in ? p32 + P32[k] : p32;
                        }
                        qf = tree_puct_qf2(qf, Wn, Np, f64 ? tree_puct_mass(p64) : (double)tree_puct_mass(p32));
                    }
                }
                if (f64) {                                            // float64 priors => float64 UCB
                    double s = sqrt((double)Np);
                    if constexpr (PUCT) s = pc * s;
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (c0 + AZK_WAVE * k >= nch) break;             // wave-uniform: no candidate in this slot at all
                        const int i = c0 + lane + AZK_WAVE * k;
                        const double u0 = P64[k] * s / (double)(Nc[k] + 1);
                        const double q = PUCT ? Vc[k] / (double)Nc[k] : Vc[k];   // N = 0: unspecified (PUCT: inf/nan), discarded by the select below
                        double un = u0;
                        if constexpr (PUCT) un = pmode != 0 ? qf + u0 : u0;
                        double u = tree_gumbel_score<GUMBEL>(tree_forced_score<FORCED>(Nc[k] != 0 ? q + u0 : un, Nc[k], P64[k], fk, Np), Nc[k], q, P64[k], gcv, gsig);
                        if constexpr (SOLVER) {
                            const bool sh = (i < nch) & (stc[k] == SOLVER_LOST) & open_any;
                            shut_any = shut_any | sh;
                            u = stc[k] == SOLVER_WON ? __builtin_huge_val() : (sh ? -__builtin_huge_val() : u);
                        }
                        const bool take = (i < nch) & ((best == 0x7fffffff) | (u > bu64));
                        bu64 = take ? u : bu64; best = take ? i : best; bN = take ? Nc[k] : bN;
                        bmeta = take ? mc[k] : bmeta; bfc = take ? fcc[k] : bfc;
                        if constexpr (PUCT) bW = take ? Vc[k] : bW;
                        if constexpr (SOLVER) bst = take ? stc[k] : bst;
                    }
                } else {                                              // float32 priors => float32 UCB (numpy>=2)
                    float s = (float)sqrt((double)Np);
                    if constexpr (PUCT) s = (float)(pc * sqrt((double)Np));
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (c0 + AZK_WAVE * k >= nch) break;             // wave-uniform: no candidate in this slot at all
                        const int i = c0 + lane + AZK_WAVE * k;
                        const float u0 = (P32[k] * s) / (float)(Nc[k] + 1);
                        const float q = (float)(PUCT ? Vc[k] / (double)Nc[k] : Vc[k]);   // N = 0: unspecified (PUCT: inf/nan), discarded by the select below
                        float un = u0;
                        if constexpr (PUCT) un = pmode != 0 ? (float)qf + u0 : u0;
                        float u = Nc[k] != 0 ? q + u0 : un;
                        if constexpr (SOLVER) {
                            const bool sh = (i < nch) & (stc[k] == SOLVER_LOST) & open_any;
                            shut_any = shut_any | sh;
                            u = stc[k] == SOLVER_WON ? __builtin_huge_valf() : (sh ? -__builtin_huge_valf() : u);
                        }
                        const bool take = (i < nch) & ((best == 0x7fffffff) | (u > bu32));
                        bu32 = take ? u : bu32; best = take ? i : best; bN = take ? Nc[k] : bN;
                        bmeta = take ? mc[k] : bmeta; bfc = take ? fcc[k] : bfc;
                        if constexpr (PUCT) bW = take ? Vc[k] : bW;
                        if constexpr (SOLVER) bst = take ? stc[k] : bst;
                    }
                }
            }
            if (ablate & 64) { const long long tn = clock64(); seg_b += tn - seg_t; seg_t = tn; }
            if constexpr (FORCED) forced_sel = f64 && __ballot(bu64 == __builtin_huge_val()) != 0ull;   // (+inf is the maximum: the winner is one of them)
            if constexpr (SOLVER) shut_sels += __ballot(shut_any) != 0ull ? 1 : 0;
            if (f64) wave_argmax_first_lane63<double>(bu64, best);
            else wave_argmax_first_lane63<float>(bu32, best);
            best = __builtin_amdgcn_readlane(best, 63);               // DPP reduction: the wave's result lives in lane 63
            }
            const int wl = best & 63;                                 // the lane whose own best candidate won
            scanned += nch;
            if constexpr (FORCED) forced_root = forced_root | forced_sel;
            const int child = fc + best;
            Np = __builtin_amdgcn_readlane(bN, wl);
            nmeta = (uint32_t)__builtin_amdgcn_readlane((int)bmeta, wl);
            fc = __builtin_amdgcn_readlane(bfc, wl);
            if constexpr (PUCT) Wn = tree_readlane_f64(bW, wl);
            if constexpr (SOLVER) nst = __builtin_amdgcn_readlane(bst, wl);
            if (ablate & 64) { const long long tn = clock64(); seg_c += tn - seg_t; seg_t = tn; }
            const int cellc = meta_cell(nmeta);
            const int mover = (root_player + depth) & 1;
            depth++;
            node = child;
            node_cell = cellc;
            if (lane == 0) {
                L.path[depth] = node;
                // make_move (gomoku.py:51-58 / tictactoe.py:37-45 test emptiness; connect4.py:56-63 does not)
                if (gd.kind == AZK_KIND_C4) L.board[cellc] |= (uint8_t)(1 << mover);
                else if (L.board[cellc] == 0) L.board[cellc] = (uint8_t)(1 << mover);
            }
            if (depth + 1 >= d.path_cap) break;
        }
        if ((ablate & 64) && lane == 0) {
            long long *qq = d.dbg + (size_t)g * 8;
            qq[0] += seg_a; qq[1] += seg_b; qq[2] += seg_c; qq[3] += seg_d; qq[5] += depth; qq[6] += 1;
        }
        azk_wave_sync();
        if (stamp) t2 = clock64();
        if (vl && fc == -2) {                                         // the walk ended on a node another slot is already evaluating: no simulation
            done_sims--;
            if (lane == 0) d.leaf_flag[vi] = 0;
            continue;
        }
        const int node_player = (root_player + depth) & 1;
        const int node_mc = root_mc + depth;
        // ---- eval-cache probe (mcts.py:37-44: key = canonical board bytes), issued early and looked at late: the table sits in HBM, and
        //      its round trips (claim word + key + row, then the claim word again for a hit) pass under other work instead of behind
        //      it.  MULTI: issued behind the terminal test, passes under the move generation.  Two-wave kernels: no move generation
        //      follows, so the loads go out in FRONT of the terminal test, which covers their first round trip (a terminal leaf then
        //      fetches a cache row for nothing).  key = ballots of "own stone" / "opponent stone" over the cells (own = the side to
        //      move at the leaf)
        bool cached = false;
        int entry = 0;
        unsigned long long mykey = 0ull, kw = 0ull;
        unsigned c1v = 0u, c2v = 0u;
        constexpr int NV4P = (KSL * AZK_WAVE + 255) / 256;           // the cached row, four consecutive logits per lane and load (as at the expansion)
        f32x4_a4 row[NV4P] = {};
        float vv = 0.f;
        bool maybe_hit = false;                                       // shared table: key and claim word say "hit" - the second claim read decides
        const int KW = d.key_words;
        auto probe_issue = [&]() {
            if (!d.cache_entries) return;
            const int half = KW >> 1;
            unsigned long long h = 0x9E3779B97F4A7C15ull;
            for (int q = 0; q < half; q++) {
                const int c = q * AZK_WAVE + lane;
                const uint8_t code = c < rc ? L.board[c] : (uint8_t)0;
                unsigned long long own = __ballot((code >> node_player) & 1);
                const unsigned long long opp = __ballot((code >> (node_player ^ 1)) & 1);
                if (q == half - 1) own |= (unsigned long long)node_player << 63;   // side to move (3-plane games; cell 63 of the last word is never a cell)
                if (lane == q) mykey = own;
                if (lane == half + q) mykey = opp;
                h = (h ^ own) * 0xFF51AFD7ED558CCDull; h ^= h >> 29;
                h = (h ^ opp) * 0xC4CEB9FE1A85EC53ull; h ^= h >> 32;
            }
            if (shared) {
                entry = (int)(h & d.cache_mask);
                // the claim word, the key and the entry's row (fetched on speculation: most probes miss, a row is 900 bytes) together
                c1v = __hip_atomic_load(d.cache_claim + entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                kw = d.cache_key[(size_t)entry * KW + min(lane, KW - 1)];
#pragma unroll
                for (int q = 0; q < NV4P; q++) row[q] = row_load4(d.cache_logits + (size_t)entry * A, row_first(256 * q + 4 * lane, A), A);
                vv = d.cache_value[entry];
            } else {
                entry = (int)(h & (unsigned long long)(d.cache_entries - 1));
                kw = d.cache_key[((size_t)g * d.cache_entries + entry) * KW + min(lane, KW - 1)];
            }
        };
        // SOLVER: a walk that stopped on a proven node (depth > 0 && nst != SOLVER_UNKNOWN) looks at nothing below - no probe, no terminal test.
        // (Its two conditions are spelled out under `if constexpr`, and the terminal test stands twice: a flag declared here for every kernel,
        // even one that folds away, gave the fused PUCT kernels another instruction order - tools/compare_kernel_isa.py.)
        if constexpr (SOLVER) { if (TWO && !(depth > 0 && nst != SOLVER_UNKNOWN)) probe_issue(); }
        else if (TWO) probe_issue();
        int term = -1;
        if constexpr (SOLVER) {
            if (depth > 0 && nst == SOLVER_UNKNOWN) {                 // mcts.py:25-32 (root is never tested)
                const int w = azk_check_winner(L.board, gd, 1 - node_player, node_cell);
                if (w != -1) term = 1;
                else if (node_mc == gd.state_dim) term = 0;
            }
        } else
        if (depth > 0) {                                              // mcts.py:25-32 (root is never tested)
            const int w = azk_check_winner(L.board, gd, 1 - node_player, node_cell);
            if (w != -1) term = 1;
            else if (node_mc == gd.state_dim) term = 0;
        }
        if (lane == 0) {
            count_add(d, CNT_SIMS, g, 1);
            count_add(d, CNT_SCANNED, g, scanned);
            if constexpr (FORCED) { if (forced_root) count_add(d, CNT_FORCED, g, 1); }   // (with the simulation's other counters, off the walk)
        }
        if (wrec) rec_depth = depth;
        if constexpr (SOLVER) {
            if (lane == 0 && shut_sels) atomicAdd((unsigned long long *)&AZK_TREE_SOLVER_ARG.stats[SST_EXCLUDING], (unsigned long long)shut_sels);
            const bool sstop = depth > 0 && nst != SOLVER_UNKNOWN;   // the walk stopped on a proven node
            if (sstop || term >= 0) {
                const SolverDev &sv = AZK_TREE_SOLVER_ARG;
                const bool has_children = meta_nch(nmeta) > 0;
                double bv = (double)term;
                int n_by_won = 0, n_by_all = 0, root_proven = 0;
                if (sstop) {
                    bv = nst == SOLVER_WON ? 1.0 : (nst == SOLVER_LOST ? -1.0 : 0.0);
                } else {
                    // the first arrival at this terminal leaf marks it, and the proof runs from it up the path: cs = the status the node at
                    // trace index ci has just taken.  Wave 0 reads the children of PATH nodes only; the one path node whose children wave 1 may be
                    // writing is prev_leaf, and the walk stands on it only behind join(1) - every byte read here was stored before the barrier or
                    // by this wave.  The child that has just been proven is taken from the register, not from the byte stored a moment ago.
                    int cs = term == 1 ? SOLVER_WON : SOLVER_DRAW, cnode = node;
                    if (lane == 0) sv.status[base + node] = (uint8_t)cs;
                    for (int ci = depth; ci > 0; ci--) {
                        const int p = uniform_i32(L.path[ci - 1]);
                        if (uniform_i32((int)sv.status[base + p]) != SOLVER_UNKNOWN) break;       // already proven (only the root can be): stop
                        int ns = SOLVER_LOST;                                                     // c WON: p is LOST
                        if (cs == SOLVER_WON) n_by_won++;
                        else {                                                                    // one wave-wide pass over all of p's children
                            const NodeH hp = d.H[base + p];
                            const int pfc = uniform_i32(hp.fc), pn = meta_nch((uint32_t)uniform_i32((int)hp.meta));
                            bool unk = false, open = false;
                            for (int i = lane; i < pn; i += AZK_WAVE) {
                                const int ch = pfc + i;
                                const int st = ch == cnode ? cs : (int)sv.status[base + ch];
                                unk = unk | (st == SOLVER_UNKNOWN); open = open | (st != SOLVER_LOST);
                            }
                            if (__ballot(unk) != 0ull) break;
                            ns = __ballot(open) != 0ull ? SOLVER_DRAW : SOLVER_WON;              // all LOST: WON; LOST and DRAW: DRAW
                            n_by_all++;
                        }
                        if (lane == 0) sv.status[base + p] = (uint8_t)ns;
                        if (ci == 1) root_proven = 1;
                        cs = ns; cnode = p;
                    }
                }
                backup_path(d, base, L.path, depth, bv);
                if (lane == 0) {
                    d.leaf_flag[vi] = 0;
                    if (!has_children) count_add(d, CNT_TERMINAL, g, 1);
                    count_add(d, CNT_TRACE, g, depth + 1);
                    unsigned long long *ss = (unsigned long long *)sv.stats;
                    if (sstop) { if (has_children) atomicAdd(ss + SST_STOPPED, 1ull); }
                    else {
                        atomicAdd(ss + SST_TERMINAL, 1ull);
                        if (n_by_won) atomicAdd(ss + SST_BY_WON_CHILD, (unsigned long long)n_by_won);
                        if (n_by_all) atomicAdd(ss + SST_BY_ALL_CHILDREN, (unsigned long long)n_by_all);
                        if (root_proven) atomicAdd(ss + SST_ROOTS, 1ull);
                    }
                }
                if (MULTI && (vl || still_young())) continue;
                break;
            }
        } else
        if (term >= 0) {
            if (wrec) { rec_type = 0; t3 = t4 = clock64(); }
            backup_path(d, base, L.path, depth, (double)term);
            if (lane == 0) {
                d.leaf_flag[vi] = 0;
                count_add(d, CNT_TERMINAL, g, 1);
                count_add(d, CNT_TRACE, g, depth + 1);
            }
            if (MULTI && (vl || still_young())) continue;             // no evaluation needed: the next simulation starts at once
            break;
        }
        if (stamp) t3 = clock64();
        if (MULTI) probe_issue();
        // called by the move generator once its first phase is behind it (a few thousand cycles after the loads above went out):
        // the copy of the row is in registers before the claim word is read again
        auto probe_mid = [&]() {
            if (!(d.cache_entries && shared)) return;
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned c1 = (unsigned)uniform_i32((int)c1v);
            const bool same = lane < KW ? kw == mykey : true;
            maybe_hit = c1 != 0u && c1 < cstamp && __ballot(!same) == 0ull;   // written in an earlier launch (complete and visible), same position
            // the entry wave 1 claims in this launch for the previous leaf: in one wave the claim came first and the probe saw this
            // launch's stamp there - never a hit, whichever wave gets to the claim word first
            if (TWO && entry == prev_crow) maybe_hit = false;
            if (maybe_hit) c2v = __hip_atomic_load(d.cache_claim + entry, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        // (the second claim read is consumed inside each branch: a load still in flight where the branches meet makes the compiler
        //  wait for it wherever its register is reused - here that was the head of the Gomoku move generation, in front of
        //  everything the probe is meant to pass under)
        int nv = -1;                                                  // two-wave kernels: "list not built" (mcts.py:34 runs at expansion, on wave 1)
        unsigned c2 = 0u;
        if constexpr (TWO) { probe_mid(); c2 = (unsigned)uniform_i32((int)c2v); }
        else if (gd.kind == AZK_KIND_GOMOKU) {                         // mcts.py:34
            nv = azk_valid_moves_gomoku<KSL>(L.board, gd, L.moves, L.ms, false, nullptr, probe_mid);
            c2 = (unsigned)uniform_i32((int)c2v);
        } else { probe_mid(); c2 = (unsigned)uniform_i32((int)c2v); nv = azk_valid_moves_small(L.board, gd, L.moves); }
        if (stamp) t4 = clock64();
        // everything below rewrites the pending-leaf record that wave 1 reads for the previous leaf: behind the barrier
        if (TWO && !joined) join(2);
        prev_leaf_done = -1;                                          // (leaf_node gets the new leaf below)
        if (d.cache_entries) {
            if (shared) {
                if (maybe_hit && c2 == (unsigned)uniform_i32((int)c1v)) {   // nobody started rewriting the entry meanwhile: the copy is whole
                    cached = true;
#pragma unroll
                    for (int q = 0; q < NV4P; q++)
                        if (256 * q + 4 * lane < A) row_store4(d.hit_logits + (size_t)vi * A, row_first(256 * q + 4 * lane, A), A, row[q]);
                    if (lane == 0) d.hit_value[vi] = vv;
                }
                if (!cached && lane < KW) d.leaf_key[(size_t)vi * KW + lane] = mykey;      // written into the table at expansion
            } else {
                unsigned long long *kp = d.cache_key + ((size_t)g * d.cache_entries + entry) * KW;
                const bool same = lane < KW ? kw == mykey : true;
                cached = __ballot(!same) == 0ull;
                if (!cached && lane < KW) kp[lane] = mykey;            // claim the slot now; logits/value land at expansion
            }
            if (lane == 0) d.leaf_cache[vi] = cached ? entry : -(entry + 1);
        }
        if (MULTI) for (int i = lane; i < nv; i += AZK_WAVE) d.leaf_moves[(size_t)vi * rc + i] = L.moves[i];
        {
            uint32_t *lw = (uint32_t *)(d.leaf_cells + (size_t)vi * d.rc_pad);
#pragma unroll
            for (int q = 0; q < NCW; q++) { const int i = lane + AZK_WAVE * q; if (i < ncw) lw[i] = ((const uint32_t *)L.board)[i]; }
        }
        for (int i = lane; i <= depth; i += AZK_WAVE) d.path[(size_t)vi * d.path_cap + i] = L.path[i];
        if (vl) {                                                     // virtual loss: the path counts a visit now and a lost game until its value arrives
            for (int i = lane; i <= depth; i += AZK_WAVE) { const int nd = L.path[i]; node_store(d, base + nd, d.H[base + nd].N + 1, d.W[base + nd] - 1.0); }
            if (lane == 0) d.H[base + node].fc = -2;           // "expansion pending": a second slot arriving here gives up
        }
        if (lane == 0) {
            d.leaf_node[vi] = node; d.leaf_depth[vi] = depth; d.leaf_nmoves[vi] = nv;
            // 1 + cost class: the evaluator's embedding kernel works through the boards of a launch from the stone-heavy ones down
            // (a board's cost is the number of tokens a stone can reach: 0.93 correlated with its stone count)
            d.leaf_flag[vi] = cached ? 0 : (uint8_t)(1 + min(7, node_mc / 6));
            if (cached) count_add(d, CNT_CACHE_HITS, g, 1);
            count_add(d, CNT_LEAVES, g, cached ? 0 : 1);
            if (wrec) rec_type = cached ? 1 : 2;
            if (stamp && !wrec) {
                long long *q = d.dbg + (size_t)g * 8;
                const long long tend = clock64();
                q[0] += t1 - t0; q[1] += t2 - t1; q[2] += t3 - t2; q[3] += t4 - t3; q[4] += tend - t4; q[5] += depth; q[6] += 1;
                if (!(ablate & 64) && tend - t0 > q[7]) q[7] = tend - t0;   // slowest simulation of this game
            }
        }
        if (MULTI && (vl || (cached && still_young()))) continue;     // served by the cache: expand it and go on, in this launch (vl: next slot)
    }
    if (vl) continue;
    break;
    }
    if (MULTI && lane0 == 0) d.sims_done[g] = done_sims;
    if (TWO && !joined) join(3);                                  // (idle or finished game, terminal leaf, expand-only launch: the walk never got there)
    if (TWO && EXPAND && prev_leaf_done >= 0 && lane0 == 0) d.leaf_node[g * d.K] = -1;   // the previous leaf is expanded and no new one took its place
    if (wrec) {
        // the game's record: wave 0's phases, the cycles it spent at the barrier (in whichever phase it met it; q[7] includes them) and
        // wave 1's clock at its barrier relative to wave 0's start (0: wave 1 had nothing to expand)
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // the wave's own stores are out: the record covers its whole life
        if (lane0 == 0) {
            long long *q = d.dbg + (size_t)g * 8;
            const long long tend = clock64();
            if (rec_type < 0) { t1 = t2 = t3 = t4 = tend; }
            if (EXPAND && prev_leaf_rec >= 0) {
                rec_env = L.ho[HO_OK] ? L.ho[HO_NV] : 0;
                w1_end = (long long)(((unsigned long long)(unsigned)L.ho[HO_END_HI] << 32) | (unsigned)L.ho[HO_END_LO]);
            }
            const long long w1 = (prev_leaf_rec >= 0 && w1_end > t0) ? w1_end - t0 : 0;
            q[0] = t1 - t0; q[1] = t2 - t1; q[2] = t3 - t2; q[3] = t4 - t3; q[4] = tend - t4;
            q[5] = (long long)rec_depth | (bar_wait << 16) | ((long long)bar_phase << 56);
            q[6] = (long long)(rec_type + 1) | ((long long)rec_env << 20) | (w1 << 32); q[7] = tend - t0;
        }
    }
