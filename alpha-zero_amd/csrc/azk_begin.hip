// azk_begin.hip - a game or a search starts: a fresh root for every game, or on a tree-reuse engine the re-rooted subtree of the played
// child (k_begin_search, k_reroot), games reset and recycled, random openings, and the asynchronous drain's restart of finished games and
// re-root of parked ones; the kernels and the C ABI calls that launch them (include/azk.h).  Built with -ffp-contract=off like every
// engine file.
#include "azk_opt_pack.h"
#include "azk_rng.h"

namespace {

// Game() for game g less its board (gomoku.py: player 0 to move, no ply played, no winner); the caller clears the cells
__device__ __forceinline__ void new_game_one(const Dev &d, int g) { d.to_move[g] = 0; d.move_count[g] = 0; d.done[g] = 0; d.winner[g] = -2; }

// CAP, here and in every kernel that has the flag (playout-cap randomisation, azk_set_playout_cap): a fast search is the same search
// with fewer simulations - sims_done starts at budget - n_fast and budget stepping (k_tree<MULTI>, k_unfinished, the movers' "search complete"
// test) ends it after n_fast.  The root's Dirichlet mix lives in k_tree and stays on for fast searches too.
template <bool CAP>
__global__ void k_begin_search(CapKeyPack<Dev, CAP> a) {
    const Dev d = a;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    if (g == 0 && d.cache_entries && d.cache_shared) d.cache_stamp[0] += 1u;
    fresh_root_one(d, g);
    if constexpr (CAP) { const Keyed<CapDev> c = opt<Keyed<CapDev>>(a); cap_begin_fresh(d, c, g, c.key, false); }
}

// ================================================================================================
// Tree reuse across moves (azk_config.tree_reuse, opt-in): the search of the next move starts on the subtree under the child
// that was played - the reference's MCTS.mcts(model, board, root, ...) (ai/mcts.py:11) handed `root = chosen_child;
// root.parent = None` instead of a new Node (games/gomoku.py:134).  reroot_one moves that subtree to the front of the game's
// arena IN PLACE (the arena pointers are baked into captured step graphs) and repairs the links.  One wave per game:
//   mark   a child block is allocated after its parent exists, so first_child(node) > node: ONE ascending sweep over a bitmap
//          of the arena finds the subtree - a marked, expanded node marks its child block, always at higher indices.  The sweep
//          holds 64 bitmap words (4 096 nodes) in registers, skips empty words without touching memory, reads the 16-byte
//          headers of a word's marked nodes in one load, and fetches the window again only after a mark that fell inside it.
//   rank   new index of a kept node = number of kept nodes below it: a running popcount per bitmap word (rr_pre) + the bits
//          below the node in its own word.  Order-preserving, so blocks stay contiguous, in list order, behind their parents.
//   slide  kept records (NodeH + W) move to their rank in ascending order, four bitmap words per round trip; destination <=
//          source for every node and a round's records are all in registers before its first store, so no record is overwritten
//          before it was read.  first_child goes through the same rank computation.
// Every loop is bounded by the game's arena_top; a link that does not point forward inside the arena ends in the sticky
// error word and a fresh root.  n_sims: the simulations this search may still run (the arena rule's worst case, and the
// top-up target).  The kept subtree is dropped for a fresh root when  kept + n_new * widest > cap  (include/azk.h).
// noise: the game's Dirichlet row of this search, float64 [A], or null (the asynchronous engine keeps two rows per game).
// ================================================================================================
__device__ __forceinline__ unsigned long long rr_load64(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);          // past the vector L1: the words are updated by atomics
}
__device__ __forceinline__ unsigned long long rr_below(int bit) { return (1ull << bit) - 1ull; }
// rank of node i among the kept nodes
__device__ __forceinline__ int rr_rank(const unsigned long long *bm, const unsigned *pre, int i) {
    const unsigned long long w = rr_load64(bm + (i >> 6));
    const unsigned p = __hip_atomic_load(pre + (i >> 6), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return (int)p + __popcll(w & rr_below(i & 63));
}

// sims_base: what sims_done starts from before the top-up preset - 0, or budget - target under a playout cap (n_sims is then the game's
// own target and the budget stops the game after n_new simulations).
__device__ void reroot_one(const Dev &d, const ReuseDev &r, int g, int c, int n_sims, const double *noise, int sims_base = 0) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * (size_t)d.cap;
    const int T = uniform_i32(d.arena_top[g]);
    unsigned long long *bm = r.bits + (size_t)g * r.words;
    unsigned *pre = r.pre + (size_t)g * r.words;
    bool keep = c > 0 && c < T && T <= d.cap && uniform_i32(d.done[g]) == 0;
    bool bad = false;
    NodeH hroot = NodeH{0, 0.f, 0u, -1};
    if (keep) hroot = d.H[base + c];
    const int root_fc = uniform_i32(hroot.fc), root_nch = uniform_i32(meta_nch(hroot.meta)), root_N = uniform_i32(hroot.N);
    if (keep && root_fc < 0) keep = false;                        // the chosen child was never expanded (n_sims = 1)
    const int n_new = r.mode == 2 ? max(1, n_sims - root_N) : n_sims;
    const int w0 = c >> 6, w1 = (T - 1) >> 6;                     // bitmap words the subtree can touch
    int kept = 0;
    if (keep) {
        for (int w = w0 + lane; w <= w1; w += AZK_WAVE) bm[w] = w == w0 ? 1ull << (c & 63) : 0ull;
        __threadfence();
        for (int wb = w0; wb <= w1 && !bad; wb += AZK_WAVE) {
            unsigned long long wreg = wb + lane <= w1 ? rr_load64(bm + wb + lane) : 0ull;
            for (int k = 0; k < AZK_WAVE && wb + k <= w1 && !bad; k++) {
                unsigned long long seen = 0ull;
                for (int round = 0; round <= AZK_WAVE; round++) {            // a round handles at least one new node of the word
                    const unsigned long long word = azk_readlane_u64(wreg, k) & ~seen;
                    if (word == 0ull) break;
                    seen |= word;
                    kept += __popcll(word);
                    const int node = (wb + k) * AZK_WAVE + lane;
                    const bool has = (word >> lane) & 1ull;
                    const NodeH h = d.H[base + (has ? node : c)];
                    const int hn = meta_nch(h.meta);
                    const bool ex = has && h.fc >= 0;
                    if (__ballot(ex && !(h.fc > node && hn >= 1 && hn <= T - h.fc)) != 0ull) { bad = true; break; }
                    unsigned long long m = __ballot(ex);
                    bool near = false;
                    while (m != 0ull) {                                       // the child block of each expanded node, as whole-word masks
                        const int l = __ffsll((long long)m) - 1;
                        m &= m - 1ull;
                        const int f = __builtin_amdgcn_readlane(h.fc, l), n = __builtin_amdgcn_readlane(hn, l);
                        const int fw = f >> 6, lw = (f + n - 1) >> 6;
                        for (int w = fw + lane; w <= lw; w += AZK_WAVE) {
                            const int lo = max(f, w * 64) - w * 64, hi = min(f + n, w * 64 + 64) - w * 64;
                            const unsigned long long mask = hi - lo == 64 ? ~0ull : rr_below(hi - lo) << lo;
                            atomicOr(bm + w, mask);
                        }
                        near = near || fw < wb + AZK_WAVE;
                    }
                    if (!near) break;                                         // every new mark lies beyond this window
                    __threadfence();
                    wreg = wb + lane <= w1 ? rr_load64(bm + wb + lane) : 0ull;
                }
            }
        }
        __threadfence();
    }
    // the arena rule: the kept subtree plus the most this search can still allocate - one expansion per simulation, and no position
    // below the root has more legal moves than min(max children, empty cells of the root position).  (The root's own child count is
    // NOT such a bound: Gomoku's legal moves are the cells next to a stone, and their number grows along a line of play.)
    const int widest = min(gd.kind == AZK_KIND_C4 ? gd.cols : gd.rc, gd.state_dim - uniform_i32(d.move_count[g]));
    if (bad || !keep || (long long)kept + (long long)n_new * widest > (long long)d.cap) {
        if (lane == 0) {
            if (bad) atomicExch(d.err, AZK_ERR_STATE);
            fresh_root_one(d, g);
            if (sims_base != 0) d.sims_done[g] = sims_base;
        }
        return;
    }
    // rank: kept nodes below each word
    int run = 0;
    for (int wb = w0; wb <= w1; wb += AZK_WAVE) {
        const unsigned long long word = wb + lane <= w1 ? rr_load64(bm + wb + lane) : 0ull;
        int incl = __popcll(word);
        const int own = incl;
#pragma unroll
        for (int off = 1; off < AZK_WAVE; off <<= 1) { const int o = __shfl_up(incl, off); if (lane >= off) incl += o; }
        if (wb + lane <= w1) pre[wb + lane] = (unsigned)(run + incl - own);
        run += __shfl(incl, AZK_WAVE - 1);
    }
    __threadfence();
    // slide
    for (int wb = w0; wb <= w1; wb += AZK_WAVE) {
        const unsigned long long wreg = wb + lane <= w1 ? rr_load64(bm + wb + lane) : 0ull;
        const int preg = wb + lane <= w1 ? (int)__hip_atomic_load(pre + wb + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
        for (int k0 = 0; k0 < AZK_WAVE && wb + k0 <= w1; k0 += 4) {
            unsigned long long wd[4];
            int pk[4];
#pragma unroll
            for (int j = 0; j < 4; j++) { wd[j] = azk_readlane_u64(wreg, k0 + j); pk[j] = __builtin_amdgcn_readlane(preg, k0 + j); }
            if ((wd[0] | wd[1] | wd[2] | wd[3]) == 0ull) continue;
            NodeH h[4];
            double wv[4], qv[4];                                              // (Q travels with W: a kept node's N and W do not change, so neither does their quotient)
            bool has[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {                                     // every record of the round, before any store
                has[j] = (wd[j] >> lane) & 1ull;
                const size_t src = base + (has[j] ? (wb + k0 + j) * AZK_WAVE + lane : c);
                h[j] = d.H[src]; wv[j] = d.W[src]; qv[j] = d.Q[src];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) if (has[j] && h[j].fc >= 0) h[j].fc = rr_rank(bm, pre, h[j].fc);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (!has[j]) continue;
                const int dst = pk[j] + __popcll(wd[j] & rr_below(lane));
                if ((wb + k0 + j) * AZK_WAVE + lane == c) { h[j].P = 0.f; h[j].meta = meta_pack(0xffff, root_nch); }   // the root: no prevAction
                d.H[base + dst] = h[j]; d.W[base + dst] = wv[j]; d.Q[base + dst] = qv[j];
            }
        }
    }
    __threadfence();
    azk_wave_sync();
    // the root's children: float64 priors with this move's Dirichlet row (utils.py:24-25 on the stored float32 prior), else as they are
    const int new_fc = rr_rank(bm, pre, root_fc);
    if (noise != nullptr) {
        for (int i = lane; i < root_nch; i += AZK_WAVE) {
            const NodeH ch = d.H[base + new_fc + i];
            d.rootP[(size_t)g * gd.rc + i] = (double)(0.75f * ch.P) + 0.25 * noise[azk_action_idx(gd, meta_cell(ch.meta))];
        }
    }
    if (lane == 0) {
        drop_pending_cache_claim(d, g);
        d.arena_top[g] = kept; d.root_f64[g] = noise != nullptr ? 1 : 0;
        clear_leaf_slots(d, g);
        d.sims_done[g] = sims_base + (r.mode == 2 ? n_sims - n_new : 0);
        count_add(d, CNT_REUSED, g, 1);
        count_add(d, CNT_CARRIED, g, kept);
    }
}

// azk_begin_search on a reuse engine: re-root on the child k_advance recorded, or a fresh root where there is none.  CAP
// (azk_begin_search_capped): n_sims is the budget, and the per-game target by the coin of the launch's move key replaces it in reroot_one
template <bool CAP>
__global__ __launch_bounds__(AZK_WAVE) void k_reroot(Dev d, CapKeyPack<ReuseDev, CAP> r, int n_sims) {
    const int g = blockIdx.x;
    if (g == 0 && azk_lane() == 0 && d.cache_entries && d.cache_shared) d.cache_stamp[0] += 1u;
    const int c = uniform_i32(r.chosen_node[g]);
    const double *noise = d.noise != nullptr ? d.noise + (size_t)g * d.g.action_dim : nullptr;
    if constexpr (CAP) {
        const Keyed<CapDev> cp = opt<Keyed<CapDev>>(r);
        const bool full = uniform_i32((int)cap_coin(cp, g, cp.key)) != 0;
        const int target = cap_target(cp, full, n_sims);
        reroot_one(d, r, g, c, target, noise, n_sims - target);
        if (azk_lane() == 0) cp.search_full[g] = full ? 1 : 0;
    } else reroot_one(d, r, g, c, n_sims, noise);
    if (azk_lane() == 0) r.chosen_node[g] = -1;                   // one search per recorded move
}

// a game has just started in slot g (one lane; engines with random openings): k_open_pending, which follows, decides whether it is opened
__device__ __forceinline__ void open_mark_one(const OpenDev &od, int g) { od.pending[g] = 1; od.open_plies[g] = 0; }

// OPEN, here and in k_recycle (engines with random openings, azk_set_openings): the new games are flagged for k_open_pending
template <bool OPEN>
__global__ void k_reset_games(OpenPack<OPEN> a, int first, int count, int *chosen_node) {
    const Dev d = a;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= count * d.rc_pad) return;
    const int g = first + t / d.rc_pad, i = t % d.rc_pad;
    d.cells[(size_t)g * d.rc_pad + i] = 0;
    if (i == 0) drop_pending_cache_claim(d, g);
    if (i == 0) { new_game_one(d, g); clear_leaf_slots(d, g); if (chosen_node) chosen_node[g] = -1; }
    if constexpr (OPEN) { if (i == 0) open_mark_one(opt<OpenDev>(a), g); }
}

// Continuous self-play: every finished game's slot restarts from Game() (empty board, player 0).
// stats[0] += games recycled, stats[1] += plies those games lasted (opening plies included), stats[2..4] += wins of player 0 / player 1 / draws.
template <bool OPEN>
__global__ void k_recycle(OpenPack<OPEN> a, long long *stats, int *chosen_node) {
    const Dev d = a;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G || !d.done[g]) return;
    atomicAdd((unsigned long long *)&stats[0], 1ull);
    atomicAdd((unsigned long long *)&stats[1], (unsigned long long)d.move_count[g]);
    const int w = d.winner[g];
    atomicAdd((unsigned long long *)&stats[w == 0 ? 2 : (w == 1 ? 3 : 4)], 1ull);
    drop_pending_cache_claim(d, g);
    for (int i = 0; i < d.rc_pad; i++) d.cells[(size_t)g * d.rc_pad + i] = 0;
    new_game_one(d, g);
    clear_leaf_slots(d, g);
    if (chosen_node) chosen_node[g] = -1;
    if constexpr (OPEN) open_mark_one(opt<OpenDev>(a), g);
}

// ================================================================================================
// Random openings (azk_set_openings, opt-in): a game that has just started in slot g - empty board, player 0 - is played
// forward a few uniformly drawn plies before its first search, so that the batch's games do not all grow from one position.  One wave per
// game, nothing waits on another wave.  key = the move key of the game's first search (the lock-step move index, the asynchronous slot's
// move counter): the key of its noise row and of its resignation coin.  With gg = first_game + g, every draw one Philox4x32-10 block under
// key (seed lo, seed hi) and word 3 = 0xFFFFFFFA (no other stream's), a uniform = ((hi << 32 | lo) >> 11) * 2^-53 (u53_incl0, azk_rng.h):
//   game draw   counter {gg lo, gg hi, key, tag}: c0 from words (0, 1), c1 from (2, 3); opened iff c0 < p_open,
//               n = min(1 + floor(c1 * max_plies), max_plies) plies
//   ply j       counter {gg lo, gg hi ^ ((j + 1) << 8), key, tag}: u from words (0, 1); with m candidates - the legal actions inside the window,
//               ascending - the side to move plays candidate min(floor(u * m), m - 1).  m == 0 ends the opening; a ply that decides the game or
//               fills the board is taken back and ends it (cut short): an opened position always has a legal move.
// The window: cell (r, c) iff spread < 0 or |2r - (rows - 1)| <= 2 spread and |2c - (cols - 1)| <= 2 spread; Connect4's candidates are its
// columns that are not full (the column condition alone) and the stone lands where the engine's rule puts it.
// The wave holds the board in registers, four cells of a dword per lane and two dwords (512 cells >= make_game's 400): the window is a
// 4-bit mask per dword, computed once; per ply the candidates are (window & empty), ranked by a DPP prefix sum of the lanes' popcounts, and
// the lane whose range holds the drawn index names the cell.  The draws are wave-uniform (scalar inputs, readfirstlane on the results).  The
// plies are ordinary plies without a search: cells, to_move, move_count and traj_action are written; no pi, no q, no record.
// ================================================================================================
__device__ __forceinline__ int wave_scan_incl_i32(int v) {               // inclusive prefix sum over the wave's lanes, on DPP (as azk_valid_moves_gomoku's)
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
    return v;
}
// bits 0..3: which of the dword's four cells are empty
__device__ __forceinline__ unsigned open_empty4(uint32_t w) {
    return ((w & 0xffu) == 0u ? 1u : 0u) | ((w & 0xff00u) == 0u ? 2u : 0u) | ((w & 0xff0000u) == 0u ? 4u : 0u) | ((w & 0xff000000u) == 0u ? 8u : 0u);
}
// position of the r-th set bit of a 4-bit mask (r < popcount)
__device__ __forceinline__ int open_nth_bit4(unsigned m, int r) {
    int pos = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
        const bool set = (m >> b) & 1u;
        if (set && r == 0) pos = b;
        r -= set ? 1 : 0;
    }
    return pos;
}

// board: the wave's LDS board (up16(rc) bytes).  All lanes of the wave call; g and key are made wave-uniform here
__device__ __forceinline__ void open_game_one(const Dev &d, const OpenDev &od, uint8_t *board, int g_in, uint32_t key_in) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const int g = uniform_i32(g_in);
    const uint32_t key = (uint32_t)uniform_i32((int)key_in);
    const unsigned long long gg = (unsigned long long)(od.first_game + g);
    const uint32_t k0 = (uint32_t)od.seed, k1 = (uint32_t)(od.seed >> 32), tag = 0xFFFFFFFAu;
    int n = 0;
    {
        uint32_t w[4] = {(uint32_t)gg, (uint32_t)(gg >> 32), key, tag};
        philox4x32_10(w, k0, k1);
        const double c0 = u53_incl0(w[0], w[1]), c1 = u53_incl0(w[2], w[3]);
        if (c0 < od.p_open) n = min(1 + (int)floor(c1 * (double)od.max_plies), od.max_plies);
    }
    n = uniform_i32(n);
    if (n == 0) {                                                   // not opened: the game starts from the empty board, as ever
        if (lane == 0) od.open_plies[g] = 0;
        return;
    }
    // the board by dword, and the window's cells of each dword
    const bool c4 = gd.kind == AZK_KIND_C4;
    uint32_t *cw = (uint32_t *)(d.cells + (size_t)g * d.rc_pad);
    uint32_t cell4[2];
    unsigned win4[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int idx = p * AZK_WAVE + lane;
        const bool in = 4 * idx < d.rc_pad;                           // (rc_pad is a multiple of 16: a dword is inside or outside as a whole)
        cell4[p] = in ? cw[idx] : 0u;
        win4[p] = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int e = 4 * idx + b;
            const int r = (int)(((unsigned)(e < gd.rc ? e : 0) * gd.inv_cols) >> 16), c = (e < gd.rc ? e : 0) - r * gd.cols;
            const bool col_ok = od.spread < 0 || abs(2 * c - (gd.cols - 1)) <= 2 * od.spread;
            const bool row_ok = c4 ? r == 0 : (od.spread < 0 || abs(2 * r - (gd.rows - 1)) <= 2 * od.spread);   // Connect4: a column stands for its top cell
            if (e < gd.rc && col_ok && row_ok) win4[p] |= 1u << b;
        }
        if (in) ((uint32_t *)board)[idx] = cell4[p];
    }
    __syncthreads();
    int mc = uniform_i32(d.move_count[g]), mover = uniform_i32(d.to_move[g]);
    int played = 0, cut = 0;
    for (int j = 0; j < n; j++) {
        const unsigned cm0 = win4[0] & open_empty4(cell4[0]), cm1 = win4[1] & open_empty4(cell4[1]);
        const int n0 = __popc(cm0), n1 = __popc(cm1);
        const int incl0 = wave_scan_incl_i32(n0), incl1 = wave_scan_incl_i32(n1);
        const int tot0 = __builtin_amdgcn_readlane(incl0, AZK_WAVE - 1), m = tot0 + __builtin_amdgcn_readlane(incl1, AZK_WAVE - 1);
        if (m == 0) break;                                            // no legal action inside the window
        uint32_t w[4] = {(uint32_t)gg, (uint32_t)(gg >> 32) ^ ((uint32_t)(j + 1) << 8), key, tag};
        philox4x32_10(w, k0, k1);
        const int k = uniform_i32(min((int)floor(u53_incl0(w[0], w[1]) * (double)m), m - 1));
        int cell = -1;                                                // the lane whose range of candidates holds index k names the cell
        if (k >= incl0 - n0 && k < incl0) cell = 4 * lane + open_nth_bit4(cm0, k - (incl0 - n0));
        if (k - tot0 >= incl1 - n1 && k - tot0 < incl1) cell = 4 * (AZK_WAVE + lane) + open_nth_bit4(cm1, k - tot0 - (incl1 - n1));
        const unsigned long long owner = __ballot(cell >= 0);
        if (owner == 0ull) break;                                     // (cannot happen: k < m)
        int cellc = __builtin_amdgcn_readlane(cell, __ffsll((long long)owner) - 1);
        if (c4) {                                                     // connect4.py:44-53: the lowest empty row of the column
            const int col = cellc;
            const unsigned long long emp = __ballot(lane < gd.rows && board[(lane < gd.rows ? lane : 0) * gd.cols + col] == 0);
            if (emp == 0ull) break;                                   // (cannot happen: a candidate column's top cell is empty)
            cellc = (63 - __clzll((long long)emp)) * gd.cols + col;
        }
        AZK_PLACE_STONE(board, gd, lane, mover, cellc);
        const int won = azk_check_winner(board, gd, mover, cellc);
        if (won != -1 || mc + 1 == gd.state_dim) {                                                     // decided or full: the ply is taken back, the opening ends here
            __syncthreads();
            if (lane == 0) board[cellc] = 0;
            __syncthreads();
            cut = 1;
            break;
        }
        const int idx = cellc >> 2;
        const uint32_t stone = (1u << mover) << (8 * (cellc & 3));
        if (lane == (idx & (AZK_WAVE - 1))) { if (idx < AZK_WAVE) cell4[0] |= stone; else cell4[1] |= stone; }
        if (lane == 0 && d.traj_action != nullptr && mc < gd.state_dim) d.traj_action[(size_t)g * gd.state_dim + mc] = (int16_t)cellc;
        if (lane == 0 && played < gd.state_dim) od.actions[(size_t)g * gd.state_dim + played] = (int16_t)cellc;
        mc += 1; mover = 1 - mover; played += 1;
    }
    if (played > 0) {
#pragma unroll
        for (int p = 0; p < 2; p++) { const int idx = p * AZK_WAVE + lane; if (4 * idx < d.rc_pad) cw[idx] = cell4[p]; }
    }
    if (lane == 0) {
        d.to_move[g] = mover; d.move_count[g] = mc;
        od.open_plies[g] = played;
        atomicAdd((unsigned long long *)&od.stats[0], 1ull);
        if (played) atomicAdd((unsigned long long *)&od.stats[1], (unsigned long long)played);
        if (cut) atomicAdd((unsigned long long *)&od.stats[2], 1ull);
    }
}

// The lock-step entry (azk_open_pending): one wave per slot; a slot without a pending flag ends after one load.  k_reset_games / k_recycle
// set the flag where a game starts; key = the move index of the search that follows
__global__ __launch_bounds__(AZK_WAVE) void k_open_pending(Dev d, OpenDev od, int key) {
    const int g = blockIdx.x;
    if (uniform_i32((int)od.pending[g]) == 0) return;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const bool fresh = uniform_i32(d.move_count[g]) == 0 && uniform_i32(d.done[g]) == 0;   // (a position set by hand is no new game)
    if (fresh) open_game_one(d, od, L.board, g, (uint32_t)key);
    if (azk_lane() == 0) { od.pending[g] = 0; if (!fresh) od.open_plies[g] = 0; }     // (not a new game: whatever plies it has were not drawn here)
}

// drain, step 4 (re-rooting engines): the next search of every game parked since the last drain - its subtree under the played child
// moved to the front of the arena, or a fresh root where reroot_one refuses; one wave per game.  The Dirichlet row is the one of the
// game's new key slot_moves[g] (the move kernel moved only once that row existed); k_noise_ahead, behind this kernel, writes the other.
// CAP: the coin of that key decides the search's target
template <bool CAP>
__global__ __launch_bounds__(AZK_WAVE) void k_reroot_list(Dev d, AsyncDev p, CapPack<ReuseDev, CAP> r) {
    const CapDev cp = opt<CapDev>(r);
    const int n = uniform_i32(*p.reroot_count), n_sims = uniform_i32(d.budget[0]), A = d.g.action_dim;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        const int g = uniform_i32(p.reroot_list[f]);
        const int c = uniform_i32(r.chosen_node[g]);
        const double *row = p.dirichlet ? p.noise + ((size_t)g * 2 + (size_t)(uniform_i32((int)p.slot_moves[g]) & 1)) * A : nullptr;
        bool full = true;
        if constexpr (CAP) {
            full = uniform_i32((int)cap_coin(cp, g, uniform_i32((int)p.slot_moves[g]))) != 0;
            const int target = cap_target(cp, full, n_sims);
            reroot_one(d, r, g, c, target, row, n_sims - target);
        } else reroot_one(d, r, g, c, n_sims, row);
        if (azk_lane() == 0) {
            r.chosen_node[g] = -1;                                 // one search per recorded move
            p.parked[g] = 0;
            atomicAdd((unsigned long long *)&p.stats[7], 1ull);
            if (CAP) {
                cp.search_full[g] = full ? 1 : 0;
                if (cp.stats != nullptr) atomicAdd((unsigned long long *)&cp.stats[full ? 8 : 9], 1ull);
            }
        }
    }
}

// drain, step 3: statistics + Game() + the next search for every listed game
// OPEN (engines with random openings): the new game is opened here, where it is born - nothing on the host runs between two
// games of a slot -, under the key of its first search (the slot's move counter), before that search begins
template <bool CAP, bool OPEN>
__device__ __forceinline__ void async_restart_body(Dev d, AsyncDev p, int recycle, CapDev cp, const OpenDev &od) {
    const int lane = azk_lane();
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int n = *p.fin_count;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        const int g = p.fin_list[f];
        if (uniform_i32(d.done[g]) == 3) continue;                 // already counted by an earlier drain (recycle off: the slot stays finished)
        if (lane == 0) {
            atomicAdd((unsigned long long *)&p.stats[0], 1ull);
            atomicAdd((unsigned long long *)&p.stats[1], (unsigned long long)d.move_count[g]);
            const int w = d.winner[g];
            atomicAdd((unsigned long long *)&p.stats[w == 0 ? 2 : (w == 1 ? 3 : 4)], 1ull);
        }
        if (!recycle) { if (lane == 0) d.done[g] = 3; continue; }
        for (int i = lane; i < d.rc_pad; i += AZK_WAVE) d.cells[(size_t)g * d.rc_pad + i] = 0;
        if (lane == 0) new_game_one(d, g);
        __syncthreads();
        if constexpr (OPEN) {
            open_game_one(d, od, L.board, g, (uint32_t)p.slot_moves[g]);
            __syncthreads();
        }
        begin_search_one(d, p, g);
        if (CAP && lane == 0) cap_begin_fresh(d, cp, g, (int)p.slot_moves[g], true);
        __syncthreads();
    }
}

template <bool CAP, bool OPEN>
__global__ __launch_bounds__(AZK_WAVE) void k_async_restart(RestartPack<CAP, OPEN> d, AsyncDev p, int recycle) {
    async_restart_body<CAP, OPEN>(d, p, recycle, opt<CapDev>(d), opt<OpenDev>(d));
}

// Adaptive search budgets (azk_set_kld_stop, azk_set_lead_stop; DESIGN sections 31 and 32): the searches that have just begun are armed (kld_arm_one), one thread per game -
// every game (list == nullptr: the lock-step begin, azk_async_begin) or the listed ones (the drain: the games k_async_restart restarted, the
// games k_reroot_list re-rooted).  It follows the kernel that began the searches on the same stream: sims_done is what that kernel left.
__global__ void k_kld_arm(Dev d, KldDev kd, const int *list, const int *n_list) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = list != nullptr ? min(*n_list, d.G) : d.G;
    if (t >= n) return;
    const int g = list != nullptr ? list[t] : t;
    if ((unsigned)g >= (unsigned)d.G) return;
    kld_arm_one(d, kd, g);
}

}  // namespace

void azk_launch_kld_arm(azk_engine *e, const int *list, const int *n_list, hipStream_t st) {
    if (!adaptive_on(e)) return;
    k_kld_arm<<<(unsigned)((e->d.G + 255) / 256), 256, 0, st>>>(e->d, e->kd, list, n_list);
}

int32_t azk_init_games(azk_engine *e) {
    const Dev &d = e->d;
    k_reset_games<false><<<(unsigned)(((size_t)d.G * d.rc_pad + 255) / 256), 256>>>(OpenPack<false>{d}, 0, d.G, e->ru.chosen_node);
    k_begin_search<false><<<(unsigned)((d.G + 255) / 256), 256>>>(cap_key_pack<false>(d, e, 0));
    HIPCHK(e, hipDeviceSynchronize());
    return AZK_OK;
}

// the start of a search for every game, on the stream: a fresh root, or on a tree-reuse engine the subtree under the played child (n_sims:
// the simulations the search may run).  On a capped engine the coin of (seed, global game, move_index) sets each game's target
static void launch_begin_search(azk_engine *e, int n_sims, int move_index, hipStream_t st) {
    const Dev &d = e->d;
    with_flags([&](auto cap) {
        if (e->ru.mode) k_reroot<cap.value><<<d.G, AZK_WAVE, 0, st>>>(d, cap_key_pack<cap.value>(e->ru, e, move_index), n_sims);
        else k_begin_search<cap.value><<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(cap_key_pack<cap.value>(d, e, move_index));
    }, e->cp.n_fast != 0);
    azk_launch_kld_arm(e, nullptr, nullptr, st);                   // adaptive search budgets: every game's first segment
}

void azk_launch_first_searches(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    if (e->op_on) k_open_pending<<<d.G, AZK_WAVE, d.lds_bytes, st>>>(d, e->op, 0);      // random openings: the first games, under move key 0
    with_flags([&](auto cap) { k_begin_search<cap.value><<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(cap_key_pack<cap.value>(d, e, 0)); }, e->cp.n_fast != 0);
    azk_launch_kld_arm(e, nullptr, nullptr, st);                   // adaptive search budgets: every game's first segment
}

// the drain's steps 3 and 4: every listed game counted and, with recycling on, restarted; re-rooting engines: the next search of every game
// that moved since the last drain
int32_t azk_launch_next_searches(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    with_flags([&](auto cap, auto open) {
        k_async_restart<cap.value, open.value><<<(unsigned)(d.G < 256 ? d.G : 256), AZK_WAVE, d.lds_bytes, st>>>(
            RestartPack<cap.value, open.value>{d, on<cap.value>(e->cp), on<open.value>(e->op)}, e->ad, e->async_recycle);
    }, e->cp.n_fast != 0, e->op_on);
    azk_launch_kld_arm(e, e->ad.fin_list, e->ad.fin_count, st);    // adaptive search budgets: the restarted games (a slot that stays finished is not armed)
    // root noise on the legal moves: the rows of the restarted games (opened or empty boards) and of the parked ones, whose positions stand
    // since their move - in front of k_reroot_list, which mixes a parked game's row into its carried root
    if (e->rn.mode && e->ad.dirichlet) azk_launch_root_noise_due(e, st);
    if (!e->ru.mode) return AZK_OK;
    with_flags([&](auto cap) {
        k_reroot_list<cap.value><<<(unsigned)d.G, AZK_WAVE, 0, st>>>(d, e->ad, CapPack<ReuseDev, cap.value>{e->ru, on<cap.value>(e->cp)});
    }, e->cp.n_fast != 0);
    azk_launch_kld_arm(e, e->ad.reroot_list, e->ad.reroot_count, st);   // adaptive search budgets: the re-rooted games, behind reroot_one's sims_done
    HIPCHK(e, hipMemsetAsync(e->ad.reroot_count, 0, sizeof(int), st));
    return AZK_OK;
}

extern "C" {

int32_t azk_reset_games(azk_engine *e, int32_t first, int32_t count, void *stream) {
    if (!e || first < 0 || count < 0 || first + count > e->d.G) { if (e) e->err = "azk_reset_games: bad range"; return AZK_ERR_ARG; }
    if (count == 0) return AZK_OK;
    e->in_search = false;                  // new games: whatever search was under way is over
    with_flags([&](auto open) {
        k_reset_games<open.value><<<(unsigned)(((size_t)count * e->d.rc_pad + 255) / 256), 256, 0, (hipStream_t)stream>>>(
            OpenPack<open.value>{e->d, on<open.value>(e->op)}, first, count, e->ru.chosen_node);
    }, e->op_on);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

// forced playouts act on the root's float64 (noise-mixed) priors: a search without a noise row is refused while the option is set
static bool forced_needs_noise(azk_engine *e, const double *noise_dev, const char *who) {
    if (e->forced_k == 0.0 || noise_dev != nullptr) return false;
    e->err = std::string(who) + ": forced playouts are set - a search needs its Dirichlet row (noise_dev = NULL is the noise-free search)";
    return true;
}

// a Gumbel root's searches read their Gumbel rows through noise_dev and run the option's own budget
static bool gumbel_refuses(azk_engine *e, const double *noise_dev, int n_sims, const char *who) {
    if (e->gb.m == 0) return false;
    if (noise_dev == nullptr) { e->err = std::string(who) + ": a Gumbel root is set - noise_dev carries the games' Gumbel rows (a row of zeros is the noise-free search, NULL is not)"; return true; }
    if (n_sims > 0 && n_sims != e->gumbel_sims) { e->err = std::string(who) + ": a Gumbel root is set - n_sims differs from the n_sims its halving table was built for (azk_set_gumbel_root)"; return true; }
    return false;
}

int32_t azk_begin_search(azk_engine *e, const double *noise_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (gumbel_refuses(e, noise_dev, 0, "azk_begin_search")) return AZK_ERR_STATE;
    if (forced_needs_noise(e, noise_dev, "azk_begin_search")) return AZK_ERR_STATE;
    if (adaptive_on(e)) { e->err = "azk_begin_search: adaptive search budgets are set (azk_set_kld_stop / azk_set_lead_stop) - their searches run under budget stepping (azk_begin_search_budget / _capped)"; return AZK_ERR_STATE; }
    if (e->cp.n_fast) { e->err = "azk_begin_search: a playout cap is set - its searches begin with azk_begin_search_capped (budget + move index)"; return AZK_ERR_STATE; }
    e->d.noise = noise_dev; e->d.noise_sel = nullptr;
    if (e->ru.mode == 2) { e->err = "azk_begin_search: top-up tree reuse needs the budget (azk_begin_search_budget)"; return AZK_ERR_STATE; }
    e->multi = false;
    e->in_search = true;
    launch_begin_search(e, e->cfg.max_sims, -1, (hipStream_t)stream);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

// azk_begin_search_budget (move_index < 0) and azk_begin_search_capped
static int32_t begin_budget(azk_engine *e, const double *noise_dev, int32_t n_sims, int32_t max_sims_per_launch, int32_t move_index, void *stream) {
    e->d.noise = noise_dev; e->d.noise_sel = nullptr;
    e->multi = true;
    e->in_search = true;
    if (e->budget_host[0] != n_sims || e->budget_host[1] != (e->d.K > 1 ? e->d.K : max_sims_per_launch)) {
        e->budget_host[0] = n_sims; e->budget_host[1] = max_sims_per_launch; e->budget_host[2] = 0;
        if (e->d.K > 1) e->budget_host[1] = e->d.K;               // virtual-loss mode: one iteration per slot
        const int32_t rc = upload_budget(e, (hipStream_t)stream);
        if (rc != AZK_OK) return rc;
    }
    launch_begin_search(e, n_sims, move_index, (hipStream_t)stream);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_begin_search_budget(azk_engine *e, const double *noise_dev, int32_t n_sims, int32_t max_sims_per_launch, void *stream) {
    if (!e || n_sims < 1 || n_sims > e->cfg.max_sims || max_sims_per_launch < 1) { if (e) e->err = "azk_begin_search_budget: bad argument"; return AZK_ERR_ARG; }
    if (e->cp.n_fast) { e->err = "azk_begin_search_budget: a playout cap is set - its searches begin with azk_begin_search_capped (the coin needs the move index)"; return AZK_ERR_STATE; }
    if (forced_needs_noise(e, noise_dev, "azk_begin_search_budget")) return AZK_ERR_STATE;
    if (gumbel_refuses(e, noise_dev, n_sims, "azk_begin_search_budget")) return AZK_ERR_STATE;
    return begin_budget(e, noise_dev, n_sims, max_sims_per_launch, -1, stream);
}

int32_t azk_begin_search_capped(azk_engine *e, const double *noise_dev, int32_t n_sims, int32_t max_sims_per_launch, int32_t move_index, void *stream) {
    if (!e || n_sims < 1 || n_sims > e->cfg.max_sims || max_sims_per_launch < 1 || move_index < 0) { if (e) e->err = "azk_begin_search_capped: bad argument"; return AZK_ERR_ARG; }
    if (!e->cp.n_fast) { e->err = "azk_begin_search_capped: no playout cap is set (azk_set_playout_cap)"; return AZK_ERR_STATE; }
    if (e->cp.n_fast > n_sims) { e->err = "azk_begin_search_capped: n_fast exceeds n_sims"; return AZK_ERR_ARG; }
    if (forced_needs_noise(e, noise_dev, "azk_begin_search_capped")) return AZK_ERR_STATE;
    return begin_budget(e, noise_dev, n_sims, max_sims_per_launch, move_index, stream);
}

int32_t azk_recycle_finished(azk_engine *e, int64_t *stats_dev, void *stream) {
    if (!e || !stats_dev) return AZK_ERR_ARG;
    with_flags([&](auto open) {
        k_recycle<open.value><<<(unsigned)((e->d.G + 255) / 256), 256, 0, (hipStream_t)stream>>>(OpenPack<open.value>{e->d, on<open.value>(e->op)},
                                                                                              (long long *)stats_dev, e->ru.chosen_node);
    }, e->op_on);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_open_pending(azk_engine *e, int32_t key, void *stream) {
    if (!e || key < 0) { if (e) e->err = "azk_open_pending: bad argument"; return AZK_ERR_ARG; }
    if (!e->op_on) { e->err = "azk_open_pending: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_open_pending: the asynchronous movers open their games themselves"; return AZK_ERR_STATE; }
    k_open_pending<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, e->op, key);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

}  // extern "C"
