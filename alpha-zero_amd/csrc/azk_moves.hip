// azk_moves.hip - everything of the batched self-play engine that happens between searches: a search begins (fresh root, or the
// re-rooted subtree of the played child), root statistics, the move, games reset and recycled, (state, pi, z) emission, the Philox
// noise rows, counters, and the asynchronous movers that do all of it per game inside the step; the kernels and the C ABI calls
// that launch them (include/azk.h).  Built with -ffp-contract=off like every engine file.
#include "azk_engine_int.h"
#include "azk_sym_map.h"      // sym_source: emission under a mask of elements
#include <type_traits>
#include <algorithm>

namespace {

// ------------------------------------------------------------------------------------------------
// The opt-ins (playout cap, resignation, forced playouts, emission under a mask of elements, surprise weighting, random openings; DESIGN sections
// 18 to 20, 22, 23 and 25).  A kernel an option touches is ONE __global__ template with a bool per option, and the options' argument blocks (CapDev, ResignDev, ForcedDev, EmitSym, SurpriseDev, OpenDev)
// ride on the block in front of them as a Pack: that block plus exactly the blocks whose flag is set.  A block that is off is an empty
// base, which takes no room, so with every flag off the Pack IS its first block: the kernel an engine without options launches has the
// argument layout and the instruction stream it always had, and an option costs the others nothing.  The kernels are one line each: the
// *_body functions behind them take the blocks by value, all zero where an option is off (opt), and fold on their flags.  The host turns the engine's state
// into the template arguments in one place per kernel (with_flags, in front of the launchers).
// A new option is a flag on each template it touches, an Opt<> in their Packs and a bool at their dispatch.  (An option that combines with few
// of the others can keep the existing kernels' names instead: the Gumbel root's movers are overloads on a pack of their own, GumbelPack.)
// ------------------------------------------------------------------------------------------------
template <class Block, bool ON> struct Opt {};
template <class Block> struct Opt<Block, true> { Block v; };
template <class First, class... Opts> struct Pack : First, Opts... {};
// the option's block out of a pack, or the block of "off" (all zero) where the pack has none
template <class Block, class P> __device__ __forceinline__ Block opt(const P &p) {
    if constexpr (std::is_base_of_v<Opt<Block, true>, P>) return static_cast<const Opt<Block, true> &>(p).v;
    else return Block{};
}
template <class Block> struct Keyed : Block { int key; };        // a block and the move key whose coin this launch flips
template <class First, bool CAP> using CapPack = Pack<First, Opt<CapDev, CAP>>;
template <class First, bool CAP> using CapKeyPack = Pack<First, Opt<Keyed<CapDev>, CAP>>;
template <class First, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE>
using MovePack = Pack<First, Opt<CapDev, CAP>, Opt<ResignDev, RESIGN>, Opt<ForcedDev, FORCED>, Opt<SurpriseDev, SURPRISE>>;
template <bool CAP, bool SYM, bool SURPRISE, bool OPEN>
using EmitPack = Pack<Dev, Opt<CapDev, CAP>, Opt<EmitSym, SYM>, Opt<SurpriseDev, SURPRISE>, Opt<OpenEmit, OPEN>>;
// random openings: the kernels that start games take the option's block behind Dev
template <bool OPEN> using OpenPack = Pack<Dev, Opt<OpenDev, OPEN>>;
template <bool CAP, bool OPEN> using RestartPack = Pack<Dev, Opt<CapDev, CAP>, Opt<OpenDev, OPEN>>;
// Gumbel root search combines with resignation only, and the kernels of the other options keep their names: the movers'
// GUMBEL forms are overloads that take this pack
template <class First, bool RESIGN> using GumbelPack = Pack<First, Opt<ResignDev, RESIGN>, Opt<GumbelDev, true>>;
static_assert(sizeof(MovePack<Dev, false, false, false, false>) == sizeof(Dev) && sizeof(EmitPack<false, false, false, false>) == sizeof(Dev) &&
              sizeof(OpenPack<false>) == sizeof(Dev) && sizeof(RestartPack<false, false>) == sizeof(Dev) && sizeof(RestartPack<true, false>) == sizeof(CapPack<Dev, true>) &&
              sizeof(MovePack<ReuseDev, false, false, false, false>) == sizeof(ReuseDev) &&
              sizeof(MovePack<Dev, true, true, true, false>) == sizeof(Pack<Dev, Opt<CapDev, true>, Opt<ResignDev, true>, Opt<ForcedDev, true>>) &&
              sizeof(EmitPack<true, true, false, false>) == sizeof(Pack<Dev, Opt<CapDev, true>, Opt<EmitSym, true>>) &&
              sizeof(CapPack<ReuseDev, false>) == sizeof(ReuseDev) && sizeof(CapKeyPack<ReuseDev, false>) == sizeof(ReuseDev), "a pack without options is its first block");

// A leaf that missed the eval cache claims its entry's key at selection and fills logits/value at expansion; if the search
// is abandoned in between (new search, reset, recycle) the half-written entry must not survive.
__device__ __forceinline__ void drop_pending_cache_claim(const Dev &d, int g) {
    for (int k = 0; k < d.K; k++) {
        const int v = g * d.K + k;
        if (d.cache_entries && !d.cache_shared && d.leaf_node[v] >= 0 && d.leaf_cache[v] < 0) {      // (shared mode claims nothing at selection)
            unsigned long long *kp = d.cache_key + ((size_t)g * d.cache_entries + (size_t)(-(d.leaf_cache[v] + 1))) * d.key_words;
            for (int w = 0; w < d.key_words; w++) kp[w] = ~0ull;
        }
    }
}

// every pending-leaf slot of game g back to "nothing pending"
__device__ __forceinline__ void clear_leaf_slots(const Dev &d, int g) {
    for (int k = 0; k < d.K; k++) { d.leaf_node[g * d.K + k] = -1; d.leaf_flag[g * d.K + k] = 0; d.to_move_v[g * d.K + k] = d.to_move[g]; }
}

// Game() for game g less its board (gomoku.py: player 0 to move, no ply played, no winner); the caller clears the cells
__device__ __forceinline__ void new_game_one(const Dev &d, int g) { d.to_move[g] = 0; d.move_count[g] = 0; d.done[g] = 0; d.winner[g] = -2; }

// Node(None, None, current_player, move_count) for every game (gomoku.py:134)
__device__ __forceinline__ void fresh_root_one(const Dev &d, int g) {
    drop_pending_cache_claim(d, g);
    const size_t base = (size_t)g * d.cap;
    d.H[base] = NodeH{0, 0.f, meta_pack(0xffff, 0), -1}; d.W[base] = 0.0;
    d.arena_top[g] = 1; d.root_f64[g] = 0;
    clear_leaf_slots(d, g);
    d.sims_done[g] = 0;
}

// Philox4x32-10, the counter-based generator of every random number the product path draws (the noise rows and move uniforms further down)
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// the options' coins: the uniform in [0, 1) of (seed, global game, word 2) under the Philox word 3 `tag`, made as noise_uniform makes its own.
// A tag is no other draw's (noise_uniform: 0xFFFFFFFF; noise_row: it < 64 and it | 0x40000000), so every other stream is what it was.
__device__ __forceinline__ double keyed_coin(unsigned long long seed, unsigned long long gg, uint32_t word2, uint32_t tag) {
    uint32_t w[4] = {(uint32_t)gg, (uint32_t)(gg >> 32), word2, tag};
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (double)((((unsigned long long)w[0] << 32) | w[1]) >> 11) * (1.0 / 9007199254740992.0);
}
// the coin of playout-cap randomisation (tag 0xFFFFFFFE): is the search of (seed, global game, move key) a FULL one?
__device__ __forceinline__ bool cap_coin(const CapDev &c, int g, int move) {
    return keyed_coin(c.seed, (unsigned long long)(c.first_game + g), (uint32_t)move, 0xFFFFFFFEu) < c.p_full;
}
// the game coin of resignation (tag 0xFFFFFFFD): is the game of (seed, global game, move key of its first search) a NEVER-RESIGN control
// game?  Stateless: the mover recomputes it at every move from start = (the slot's move counter) - (the game's plies), so no restart,
// recycle or reset kernel knows of it.
__device__ __forceinline__ bool resign_never(const ResignDev &rs, int g, uint32_t start) {
    return keyed_coin(rs.seed, (unsigned long long)(rs.first_game + g), start, 0xFFFFFFFDu) < rs.p_never;
}
// the ply coin of policy surprise weighting (tag 0xFFFFFFFC): the uniform that rounds the ply's weight to a whole number of copies
__device__ __forceinline__ double surprise_coin(const SurpriseDev &sp, int g, int move) {
    return keyed_coin(sp.seed, (unsigned long long)(sp.first_game + g), (uint32_t)move, 0xFFFFFFFCu);
}
// simulations of a search of that kind under the budget as it stands (a fast search never exceeds the budget)
__device__ __forceinline__ int cap_target(const CapDev &c, bool full, int budget) { return full ? budget : min(c.n_fast, budget); }

// a fresh-root search has just begun for game g (one lane): flip its coin and preset sims_done so that budget stepping stops a fast
// search after n_fast simulations - what top-up does with the carried visits
__device__ __forceinline__ void cap_begin_fresh(const Dev &d, const CapDev &c, int g, int move, bool count) {
    const int n = d.budget[0];
    const bool full = cap_coin(c, g, move);
    c.search_full[g] = full ? 1 : 0;
    d.sims_done[g] = n - cap_target(c, full, n);
    if (count && c.stats != nullptr) atomicAdd((unsigned long long *)&c.stats[full ? 8 : 9], 1ull);
}

// CAP, here and in every kernel below (playout-cap randomisation, azk_set_playout_cap): a fast search is the same search
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
            double wv[4];
            bool has[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {                                     // every record of the round, before any store
                has[j] = (wd[j] >> lane) & 1ull;
                const size_t src = base + (has[j] ? (wb + k0 + j) * AZK_WAVE + lane : c);
                h[j] = d.H[src]; wv[j] = d.W[src];
            }
#pragma unroll
            for (int j = 0; j < 4; j++) if (has[j] && h[j].fc >= 0) h[j].fc = rr_rank(bm, pre, h[j].fc);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                if (!has[j]) continue;
                const int dst = pk[j] + __popcll(wd[j] & rr_below(lane));
                if ((wb + k0 + j) * AZK_WAVE + lane == c) { h[j].P = 0.f; h[j].meta = meta_pack(0xffff, root_nch); }   // the root: no prevAction
                d.H[base + dst] = h[j]; d.W[base + dst] = wv[j];
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

// utils.get_probablity_distribution_of_children (utils.py:46-55), root.value / root.visit (gomoku.py:140)
__global__ __launch_bounds__(AZK_WAVE) void k_root_stats(Dev d, double *pi, double *q, int *root_visit) {
    const int g = blockIdx.x, lane = azk_lane();
    const size_t base = (size_t)g * d.cap;
    const int A = d.g.action_dim;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int fc = d.H[base].fc, nch = meta_nch(d.H[base].meta);
    for (int a = lane; a < A; a += AZK_WAVE) L.cnt[a] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        L.cnt[azk_action_idx(d.g, meta_cell(d.H[base + fc + i].meta))] = n;
        sum += n;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    if (pi) for (int a = lane; a < A; a += AZK_WAVE) pi[(size_t)g * A + a] = (double)L.cnt[a] / (double)sum;
    if (lane == 0) {
        if (q) q[g] = d.W[base] / (double)d.H[base].N;
        if (root_visit) root_visit[g] = d.H[base].N;
    }
}

// Policy target pruning (forced playouts; Wu 2019, section 3.2) for one game (one wave).  L.cnt holds the root children's
// RAW visit counts by action; on return it holds the counts the recorded pi is made of, and the function returns their sum.  With
// Np = root visits, s = sqrt(Np) and c* = the first child with the most visits (Node.max_visit_child):
//     pstar = W* / N* + (P* * s) / (N* + 1)
// and every other child with N >= 1 loses up to nf = floor(sqrt((k * P) * (Np - 1))) visits - the floor forced playouts gave it - one at a
// time, while its PUCT score with that visit removed (q held at W / N) would still lose to c*:
//     m = N;  while (m > N - nf && m > 0 && q + (P * s) / m < pstar) m -= 1;   if (m == 1 && nf >= 1) m = 0
// All float64, P = the root's mixed priors (rootP); c* and unvisited children keep their counts.  At most nf <= sqrt(k * max_sims) rounds per
// lane.  The tree is not touched: the move, q, resignation and tree reuse see raw visits.
__device__ __forceinline__ int prune_counts(const Dev &d, const LdsView &L, int g, double k) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta)), Np = uniform_i32(d.H[base].N);
    const double *P = d.rootP + (size_t)g * gd.rc;
    const double s = sqrt((double)Np);
    int best = 0x7fffffff, bn = 0;                                  // Node.max_visit_child (node.py:76-81)
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        if (best == 0x7fffffff || n > bn) { bn = n; best = i; }
    }
    wave_argmax_first<int>(bn, best);
    best = uniform_i32(best); bn = uniform_i32(bn);
    const double pstar = d.W[base + fc + best] / (double)bn + (P[best] * s) / (double)(bn + 1);
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const NodeH h = d.H[base + fc + i];
        int m = h.N;
        if (i != best && h.N >= 1) {
            const double Pi = P[i];
            const int nf = (int)floor(sqrt((k * Pi) * (double)(Np - 1)));
            const double q = d.W[base + fc + i] / (double)h.N;
            while (m > h.N - nf && m > 0 && q + (Pi * s) / (double)m < pstar) m -= 1;
            if (m == 1 && nf >= 1) m = 0;
            L.cnt[azk_action_idx(gd, meta_cell(h.meta))] = m;
        }
        sum += m;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    return sum;
}
// is the search game g has just completed a forced one?  (the option set - the caller's template parameter - the search full, the root mixed)
__device__ __forceinline__ bool forced_search(const Dev &d, const ForcedDev &fp, int g) {
    const int full = fp.search_full != nullptr ? uniform_i32((int)fp.search_full[g]) : 1;
    return full != 0 && uniform_i32(d.root_f64[g]) != 0;
}

// Policy surprise (surprise weighting) of one game's move (one wave): KL(recorded pi || the network's prior) over the root's
// children, all float64:  kl = max(0, sum over children with m > 0 of  p * log(p / P)),  p = m / sum  the recorded pi's entry (L.cnt: the
// counts after pruning), P = the child's RAW float32 prior as k_tree stored it in the header (not rootP, the Dirichlet mix), floored at the
// smallest normal float.  Lanes sum their children in list order, then the wave's butterfly: the same order in both movers.
__device__ __forceinline__ double surprise_kl(const Dev &d, const LdsView &L, int g, int sum) {
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    double part = 0.0;
    for (int i = azk_lane(); i < nch; i += AZK_WAVE) {
        const NodeH h = d.H[base + fc + i];
        const int m = L.cnt[azk_action_idx(d.g, meta_cell(h.meta))];
        if (m > 0) {
            const double p = (double)m / (double)sum, P = (double)fmaxf(h.P, 0x1p-126f);
            part += p * log(p / P);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    return part > 0.0 ? part : 0.0;
}

// Gumbel root search (azk_set_gumbel_root): the move and the recorded pi of one game's search (one wave), all float64,
// children in list order.  With N_i, W_i, P_i (the header's float32 prior), gl_i = rootP, logit_i and v0 as the root's expansion kept them:
//     S = sum N;  q_i = W_i / N_i (N_i > 0);  pv = sum over visited of P_i;  pq = sum over visited of P_i * q_i   (both sequential, list order)
//     vmix = S > 0 ? (v0 + S * (pq / pv)) / (1 + S) : v0;  qh_i = N_i > 0 ? q_i : vmix;  sigf = (c_visit + max N) * c_scale
//     move    among the children with N_i == max N, the first maximum of gl_i + sigf * qh_i
//     pi      y_i = logit_i + sigf * qh_i;  pi[a_i] = exp(y_i - max y) / sum_j exp(y_j - max y), 0 on every other action
// Returns the played child's list index (wave-uniform) and leaves pi, by action, in L.cdf.  The tree is not touched.
__device__ __forceinline__ int gumbel_target(const Dev &d, const LdsView &L, int g, const GumbelDev &gb) {
    constexpr int KMAX = 7;                                           // children per lane: make_game allows 400 cells
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int A = gd.action_dim, rc = gd.rc;
    const int fc = uniform_i32(d.H[base].fc), nch = min(uniform_i32(meta_nch(d.H[base].meta)), KMAX * AZK_WAVE);
    int *Nl = (int *)L.ms.claim;                                      // visits by child position (table_size words: more than any board has cells)
    int nv[KMAX], cellv[KMAX];
    double qv[KMAX], yv[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int i = lane + AZK_WAVE * k;
        nv[k] = 0; cellv[k] = 0; qv[k] = 0.0; yv[k] = 0.0;
        if (i < nch) {
            const NodeH h = d.H[base + fc + i];
            nv[k] = h.N; cellv[k] = meta_cell(h.meta);
            qv[k] = h.N > 0 ? d.W[base + fc + i] / (double)h.N : 0.0;
            Nl[i] = h.N; L.e[i] = h.P; L.cdf[i] = qv[k];
        }
    }
    __syncthreads();
    double vmix = 0.0;
    int maxn = 0;
    if (lane == 0) {
        int S = 0;
        double pv = 0.0, pq = 0.0;
        for (int i = 0; i < nch; i++) {
            const int n = Nl[i];
            S += n; maxn = max(maxn, n);
            if (n > 0) { const double P = (double)L.e[i]; pv += P; pq += P * L.cdf[i]; }
        }
        const double v0 = (double)gb.v0[g];
        vmix = S > 0 ? (v0 + (double)S * (pq / pv)) / (1.0 + (double)S) : v0;
    }
    vmix = __shfl(vmix, 0); maxn = __shfl(maxn, 0);
    const double sigf = (gb.c_visit + (double)maxn) * gb.c_scale;
    int best = 0x7fffffff;
    double bs = -__builtin_huge_val(), ym = -__builtin_huge_val();
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int i = lane + AZK_WAVE * k;
        if (i < nch) {
            const double qh = nv[k] > 0 ? qv[k] : vmix;
            const double sc = d.rootP[(size_t)g * rc + i] + sigf * qh;
            yv[k] = (double)gb.logit[(size_t)g * rc + i] + sigf * qh;
            if (nv[k] == maxn && (best == 0x7fffffff || sc > bs)) { bs = sc; best = i; }
            ym = fmax(ym, yv[k]);
        }
    }
    wave_argmax_first<double>(bs, best);
    best = uniform_i32(best);
    ym = wave_max_f64(ym);
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        if (lane + AZK_WAVE * k < nch) { yv[k] = exp(yv[k] - ym); part += yv[k]; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    __syncthreads();
    for (int a = lane; a < A; a += AZK_WAVE) L.cdf[a] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        if (lane + AZK_WAVE * k < nch) L.cdf[azk_action_idx(gd, cellv[k])] = yv[k] / part;
    }
    __syncthreads();
    return best;
}

// make_move (gomoku.py:148) on the wave's LDS board: the mover's stone goes onto cellc, placed by lane 0; azk_check_winner follows it.  The
// ONE copy of the placing rule, which the movers (advance_one) and the openings (open_game_one) both play their plies through.  It is text,
// not a function: behind a call the compiler schedules the movers differently, and an engine without openings launches the device code it
// always launched (profiles/openings_isa_vs_parent.txt).  Two statements without a wrapper, for the same reason: use it only as a full statement
// at block scope, never as the body of an unbraced if / else / loop.
#define AZK_PLACE_STONE(board, gd, lane, mover, cellc)                                         \
    if ((lane) == 0) {                                                                         \
        if ((gd).kind == AZK_KIND_C4) (board)[cellc] |= (uint8_t)(1 << (mover));               \
        else if ((board)[cellc] == 0) (board)[cellc] = (uint8_t)(1 << (mover));                \
    }                                                                                          \
    __syncthreads()

// ================================================================================================
// Random openings (azk_set_openings, opt-in): a game that has just started in slot g - empty board, player 0 - is played
// forward a few uniformly drawn plies before its first search, so that the batch's games do not all grow from one position.  One wave per
// game, nothing waits on another wave.  key = the move key of the game's first search (the lock-step move index, the asynchronous slot's
// move counter): the key of its noise row and of its resignation coin.  With gg = first_game + g, every draw one Philox4x32-10 block under
// key (seed lo, seed hi) and word 3 = 0xFFFFFFFA (no other stream's), a uniform = ((hi << 32 | lo) >> 11) * 2^-53 as keyed_coin makes it:
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
__device__ __forceinline__ double open_uniform(uint32_t hi, uint32_t lo) {
    return (double)((((unsigned long long)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
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
        const double c0 = open_uniform(w[0], w[1]), c1 = open_uniform(w[2], w[3]);
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
        const int k = uniform_i32(min((int)floor(open_uniform(w[0], w[1]) * (double)m), m - 1));
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

// gomoku.py:143-162 for one game (one wave): choose (sample ~ visits | first max-visit child), record pi / the action in the
// trajectory, make_move, check_winner, draw.  Returns the chosen cell (-1: state error, already reported); *win_out / *done_out as
// k_advance's outputs; pi of the move is left in L.cnt / sum_out (visit counts per action and their sum).
// RESIGN (resigning engines, azk_set_resign): after a move that does not end the game the mover concedes when the
// root's q reached v_resign - or, in a never-resign game, is noted as the game's mark.  key = the slot's move counter at this move,
// *rsg_out = 1 when the move ended the game by resignation.  A resignation happens where a natural end happens (winner and done are set
// here), so emission, recycling, the drain and the re-root see an ordinary finished game.
// FORCED (engines with forced playouts, azk_set_forced_playouts): once the cell is chosen - from raw visits - the counts
// of a forced search are pruned in place (prune_counts), so that traj_pi and the caller's record hold the pruned pi.  The selection half of
// the option lives in k_tree<.., FORCED> (azk_tree.hip).
// SURPRISE (engines with surprise weighting, azk_set_surprise_weighting): the kl of the pi that is recorded - after the
// pruning - and the ply's coin of the move key go into traj_kl / traj_coin beside traj_pi and into the game's last-move pair (lane 0 writes
// them: the asynchronous mover's lane 0 copies the pair into its record).
// GUMBEL (engines with a Gumbel root, azk_set_gumbel_root): the move is gumbel_target's - the uniform and sample_until are
// not looked at, the Gumbel arg-max is the sample - and the recorded pi is its float64 row in L.cdf (the caller's record reads it there too);
// L.cnt / sum_out still hold the raw visits.
template <bool RESIGN, bool FORCED, bool SURPRISE, bool GUMBEL = false>
__device__ __forceinline__ int advance_one(const Dev &d, LdsView &L, int g, bool have_u, double u, int sample_until, int *win_out, int *done_out,
                                           int *sum_out, const ResignDev &rs, int key, int *rsg_out, const ForcedDev &fp, const SurpriseDev &sp,
                                           const GumbelDev &gb = GumbelDev{}) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int A = gd.action_dim, rc = gd.rc;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    const int mc = uniform_i32(d.move_count[g]), mover = uniform_i32(d.to_move[g]);
    for (int i = lane; i < rc; i += AZK_WAVE) L.board[i] = d.cells[(size_t)g * d.rc_pad + i];
    for (int a = lane; a < A; a += AZK_WAVE) L.cnt[a] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        L.cnt[azk_action_idx(gd, meta_cell(d.H[base + fc + i].meta))] = n;
        sum += n;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    *sum_out = sum;
    int cellc = -1;
    if (nch <= 0 || sum <= 0) {
        if (lane == 0) atomicExch(d.err, AZK_ERR_STATE);
        return -1;
    }
    if constexpr (GUMBEL) {
        cellc = meta_cell(d.H[base + fc + gumbel_target(d, L, g, gb)].meta);
    } else
    if (have_u && mc < sample_until) {
        // Node.sample_child (node.py:83-93) -> legacy np.random.choice(p=pi): cdf = cumsum(pi); cdf /= cdf[-1];
        // index = searchsorted(cdf, u, side='right').  cumsum is sequential in float64.
        if (lane == 0) {
            double acc = 0.0;
            for (int a = 0; a < A; a++) { acc += (double)L.cnt[a] / (double)sum; L.cdf[a] = acc; }
            const double lastv = L.cdf[A - 1];
            int lo = 0, hi = A;
            while (lo < hi) { int mid = (lo + hi) >> 1; if (u < L.cdf[mid] / lastv) hi = mid; else lo = mid + 1; }
            L.path[0] = lo < A ? lo : A - 1;                         // action drawn (path scratch: cnt[] is still needed)
        }
        __syncthreads();
        const int act = L.path[0];
        int found = 0x7fffffff;
        for (int i = lane; i < nch; i += AZK_WAVE)
            if (azk_action_idx(gd, meta_cell(d.H[base + fc + i].meta)) == act && i < found) found = i;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { int o = __shfl_xor(found, off); found = o < found ? o : found; }
        cellc = found != 0x7fffffff ? meta_cell(d.H[base + fc + found].meta) : -1;
    } else {
        // Node.max_visit_child (node.py:76-81): first child with the most visits
        int best = 0x7fffffff, bn = 0;
        for (int i = lane; i < nch; i += AZK_WAVE) {
            const int n = d.H[base + fc + i].N;
            if (best == 0x7fffffff || n > bn) { bn = n; best = i; }
        }
        wave_argmax_first<int>(bn, best);
        cellc = meta_cell(d.H[base + fc + uniform_i32(best)].meta);
    }
    cellc = uniform_i32(cellc);
    if (cellc < 0) {
        if (lane == 0) atomicExch(d.err, AZK_ERR_STATE);
        return -1;
    }
    if constexpr (FORCED) {
        if (forced_search(d, fp, g)) {
            const int raw = sum;
            sum = prune_counts(d, L, g, fp.k);
            *sum_out = sum;
            if (lane == 0) { count_add(d, CNT_PRUNED, g, raw - sum); count_add(d, CNT_PRUNE_OF, g, raw); }
        }
    }
    if (d.traj_pi != nullptr && mc < gd.state_dim) {               // gomoku.py:138-146: pi and the action of this ply
        double *tp = d.traj_pi + ((size_t)g * gd.state_dim + mc) * A;
        if constexpr (GUMBEL) { for (int a = lane; a < A; a += AZK_WAVE) tp[a] = L.cdf[a]; }
        else
        for (int a = lane; a < A; a += AZK_WAVE) tp[a] = (double)L.cnt[a] / (double)sum;
        if (lane == 0) d.traj_action[(size_t)g * gd.state_dim + mc] = (int16_t)cellc;
    }
    if constexpr (SURPRISE) {
        const double kl = surprise_kl(d, L, g, sum), coin = surprise_coin(sp, g, key);
        if (lane == 0) {
            if (d.traj_pi != nullptr && mc < gd.state_dim) { sp.traj_kl[(size_t)g * gd.state_dim + mc] = kl; sp.traj_coin[(size_t)g * gd.state_dim + mc] = coin; }
            sp.last_kl[g] = kl; sp.last_coin[g] = coin;
        }
    }
    AZK_PLACE_STONE(L.board, gd, lane, mover, cellc);
    const int w = azk_check_winner(L.board, gd, mover, cellc);      // gomoku.py:150
    int win = -2, dn = 0;
    if (w != -1) { win = w; dn = 1; }
    else if (mc + 1 == gd.state_dim) { win = -1; dn = 1; }
    if (RESIGN) {
        // the game's first search had move key key - mc; q is the recorded q (k_root_stats, the movers' rec_q): the same float64 expression
        const uint32_t start = (uint32_t)key - (uint32_t)mc;
        const bool never = resign_never(rs, g, start);
        const int side = uniform_i32(rs.mark_side[g]);
        const bool marked = side >= 0 && (uint32_t)uniform_i32((int)rs.mark_start[g]) == start;
        int rsg = 0;
        if (dn == 0 && mc + 1 >= rs.min_ply && d.W[base] / (double)d.H[base].N >= rs.v_resign) {
            if (!never) { win = 1 - mover; dn = 1; rsg = 1; }                                  // the mover concedes
            else if (!marked && lane == 0) { rs.mark_start[g] = start; rs.mark_side[g] = mover; }   // ... would have: the game plays on
        }
        if (lane == 0) {
            rs.resigned[g] = (uint8_t)rsg;
            if (rsg) atomicAdd((unsigned long long *)&rs.stats[0], 1ull);
            else if (dn && never) {
                atomicAdd((unsigned long long *)&rs.stats[1], 1ull);
                if (marked) atomicAdd((unsigned long long *)&rs.stats[2], 1ull);
                if (marked && win != 1 - side) atomicAdd((unsigned long long *)&rs.stats[3], 1ull);     // a false positive: it won or drew
            }
        }
        *rsg_out = rsg;
    }
    if (lane == 0) {
        d.cells[(size_t)g * d.rc_pad + cellc] = L.board[cellc];
        d.to_move[g] = 1 - mover;
        d.move_count[g] = mc + 1;
        d.winner[g] = win; d.done[g] = dn;
        d.counters[(size_t)CNT_MOVES * d.G + g] += 1;
    }
    *win_out = win; *done_out = dn;
    return cellc;
}

// tree reuse: the arena index of the root's child that holds cell `cellc` (a cell occurs once among a node's children), -1 = none.
// One wave; the result is wave-uniform.  The move itself (advance_one) does not touch the tree, so this may follow it.
__device__ __forceinline__ int played_child(const Dev &d, int g, int cellc) {
    const int lane = azk_lane();
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    int found = 0x7fffffff;
    for (int i = lane; i < nch; i += AZK_WAVE) if (meta_cell(d.H[base + fc + i].meta) == cellc && i < found) found = i;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(found, off); found = o < found ? o : found; }
    return (cellc >= 0 && found != 0x7fffffff) ? fc + found : -1;
}

// The lock-step mover (azk_advance, azk_advance_resign): every game's move, one wave per game.  CAP: the ply's kind goes into traj_full beside its
// pi; RESIGN, SURPRISE (move_index = the slot's move counter), FORCED: as advance_one has them
template <bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool GUMBEL = false>
__device__ __forceinline__ void advance_body(Dev d, CapDev cp, ResignDev rs, int move_index, const double *uniforms, int sample_until,
                                             int *chosen, int *winner_out, int *done_out, int *chosen_node, const ForcedDev &fp, const SurpriseDev &sp,
                                             const GumbelDev &gb = GumbelDev{}) {
    const int g = blockIdx.x, lane = azk_lane();
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    if (uniform_i32(d.done[g]) != 0) {
        if (lane == 0) {
            if (chosen) chosen[g] = -1;
            if (winner_out) winner_out[g] = d.winner[g];
            if (done_out) done_out[g] = 1;
            if (chosen_node) chosen_node[g] = -1;
        }
        return;
    }
    int win = -2, dn = 0, sum = 0, rsg = 0;
    const int mc = CAP ? uniform_i32(d.move_count[g]) : 0;
    int cellc;
    if constexpr (GUMBEL) cellc = advance_one<RESIGN, false, false, true>(d, L, g, false, 0.0, 0, &win, &dn, &sum, rs, move_index, &rsg, fp, sp, gb);
    else cellc = advance_one<RESIGN, FORCED, SURPRISE>(d, L, g, uniforms != nullptr, uniforms != nullptr ? uniforms[g] : 0.0, sample_until, &win, &dn, &sum,
                                                            rs, move_index, &rsg, fp, sp);
    if (CAP && cellc >= 0 && lane == 0 && cp.traj_full != nullptr && mc < d.g.state_dim) cp.traj_full[(size_t)g * d.g.state_dim + mc] = cp.search_full[g];
    if (chosen_node) {
        const int child = played_child(d, g, cellc);               // tree reuse: the next search's root
        if (lane == 0) chosen_node[g] = dn == 0 ? child : -1;
    }
    if (cellc < 0) return;
    if (lane == 0) {
        if (chosen) chosen[g] = cellc;
        if (winner_out) winner_out[g] = win;
        if (done_out) done_out[g] = dn;
    }
}

// the lock-step mover's scalars: move_index is an argument only of the kernels of engines with a keyed option (resignation, surprise weighting)
template <bool KEYED> struct Ply { int sample_until; };
template <> struct Ply<true> { int sample_until, move_index; };

template <bool CAP, bool RESIGN, bool FORCED, bool SURPRISE>
__global__ __launch_bounds__(AZK_WAVE) void k_advance(MovePack<Dev, CAP, RESIGN, FORCED, SURPRISE> a, const double *uniforms, Ply<RESIGN || SURPRISE> ply,
                                                       int *chosen, int *winner_out, int *done_out, int *chosen_node) {
    int move_index = 0;
    if constexpr (RESIGN || SURPRISE) move_index = ply.move_index;
    advance_body<CAP, RESIGN, FORCED, SURPRISE>(a, opt<CapDev>(a), opt<ResignDev>(a), move_index, uniforms, ply.sample_until, chosen, winner_out, done_out,
                                                chosen_node, opt<ForcedDev>(a), opt<SurpriseDev>(a));
}

// the lock-step mover of an engine with a Gumbel root (with or without resignation)
template <bool RESIGN>
__global__ __launch_bounds__(AZK_WAVE) void k_advance(GumbelPack<Dev, RESIGN> a, Ply<RESIGN> ply, int *chosen, int *winner_out, int *done_out) {
    int move_index = 0;
    if constexpr (RESIGN) move_index = ply.move_index;
    advance_body<false, RESIGN, false, false, true>(a, CapDev{}, opt<ResignDev>(a), move_index, nullptr, 0, chosen, winner_out, done_out, nullptr, ForcedDev{},
                                                    SurpriseDev{}, opt<GumbelDev>(a));
}

// ------------------------------------------------------------------------------------------------
// (state, pi, z) emission: train.save_data_to_buffer (train.py:30-49) with rotate_data / flip_data (train.py:8-27).
// Position i of a finished game (side to move = i & 1): z = +-1 by winner (0 for a draw), state = canonical board;
// positions 0 and 1 once, the others 8 times in the order rot0, lr(rot0), tb(rot0), rot90, lr(rot90), tb(rot90),
// rot180, rot270 (np.rot90 is counter-clockwise).  Tuple t of the stream lands in slot t % capacity (deque(maxlen)).
// ------------------------------------------------------------------------------------------------
// CAP (playout-cap engines): only the plies of FULL searches are emitted - ply i's group (1 tuple for i < 2, else 8) sits at
// the sum of the groups of the full plies before it; the board before ply i is rebuilt from every earlier ply, fast ones included.
// SYM (engines created with emit_elements): the group of a ply from the third on is one tuple per
// element of the mask (es.n of them, es.els in ascending order) instead of the reference's eight, on any R x C board and action kind.
// SURPRISE (engines with surprise weighting): ply i of the recorded plies F (all, or with CAP the full ones; n_F of them, S = the
// sequential sum of their kl in ply order) is written c_i = floor(w_i) + (coin_i < w_i - floor(w_i)) times,
//     w_i = S > 0 ? (1 - lambda) + ((lambda * n_F) * kl_i) / S : 1      (float64)
// copy-major at base + sum_{j<i} c_j * grp_j.  k_emit_alloc writes c into traj_copies (0 outside F) and reserves the sum; k_emit_tuples reads it.
// OPEN (engines with random openings): the opening's plies i < open_plies[g] had no search and are left out exactly as a
// capped engine's fast plies are - no tuples, not in n_F or S, 0 copies, not in the sums of the tuples before a ply; `i < 2 ? 1 : grp`
// stays keyed on the absolute ply index, and boards are rebuilt from ply 0.
template <bool CAP, bool SYM, bool SURPRISE, bool OPEN>
__device__ __forceinline__ void emit_alloc_body(Dev d, const uint8_t *traj_full, unsigned long long *cursor, long long *game_base_out, const EmitSym &es,
                                                const SurpriseDev &sp, const OpenEmit &oe) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    long long base = -1;                                          // the stream index stays 64-bit end to end (2^31 tuples = hours of self-play)
    if (d.done[g] == 1) {
        const int n = d.move_count[g];
        const int grp = SYM ? es.n : 8;
        int o = 0;                                                // the first ply that had a search
        if constexpr (OPEN) o = min(oe.open_plies[g], n);
        int tuples = n <= 2 ? n : 2 + grp * (n - 2);
        if (OPEN) tuples -= o <= 2 ? o : 2 + grp * (o - 2);
        if (CAP) {
            tuples = 0;
            for (int i = o; i < n; i++) if (traj_full[(size_t)g * d.g.state_dim + i]) tuples += i < 2 ? 1 : grp;
        }
        if constexpr (SURPRISE) {
            const size_t row = (size_t)g * d.g.state_dim;
            int n_F = 0;
            double S = 0.0;
            for (int i = o; i < n; i++) if (!CAP || traj_full[row + i]) { n_F += 1; S += sp.traj_kl[row + i]; }
            tuples = 0;
            for (int i = 0; i < n; i++) {
                int c = 0;
                if ((!OPEN || i >= o) && (!CAP || traj_full[row + i])) {
                    const double w = S > 0.0 ? (1.0 - sp.lambda) + ((sp.lambda * (double)n_F) * sp.traj_kl[row + i]) / S : 1.0;
                    const double f = floor(w);
                    c = (int)f + (sp.traj_coin[row + i] < w - f ? 1 : 0);
                }
                sp.traj_copies[row + i] = (uint16_t)c;
                tuples += c * (i < 2 ? 1 : grp);
            }
        }
        base = (long long)atomicAdd(cursor, (unsigned long long)tuples);
    }
    d.emit_base[g] = base;
    if (game_base_out) game_base_out[g] = base;
}

template <bool CAP, bool SYM, bool SURPRISE, bool OPEN>
__global__ void k_emit_alloc(EmitPack<CAP, SYM, SURPRISE, OPEN> a, unsigned long long *cursor, long long *game_base_out) {
    emit_alloc_body<CAP, SYM, SURPRISE, OPEN>(a, opt<CapDev>(a).traj_full, cursor, game_base_out, opt<EmitSym>(a), opt<SurpriseDev>(a), opt<OpenEmit>(a));
}

__device__ __forceinline__ int d4_source(int t, int i, int j, int N) {
    // source cell (row-major) of output cell (i, j) under transform t of the reference's emission order
    int si, sj;
    switch (t) {
        case 0: si = i; sj = j; break;                          // rot0
        case 1: si = i; sj = N - 1 - j; break;                  // lr(rot0)
        case 2: si = N - 1 - i; sj = j; break;                  // tb(rot0)
        case 3: si = j; sj = N - 1 - i; break;                  // rot90 (ccw): out[i][j] = in[j][N-1-i]
        case 4: si = N - 1 - j; sj = N - 1 - i; break;          // lr(rot90)
        case 5: si = j; sj = i; break;                          // tb(rot90)
        case 6: si = N - 1 - i; sj = N - 1 - j; break;          // rot180
        default: si = N - 1 - j; sj = i; break;                 // rot270: out[i][j] = in[N-1-j][i]
    }
    return si * N + sj;
}

// LIST: the grid walks a list of finished games (asynchronous drain) instead of covering all G.  SURPRISE: the ply's group is written
// traj_copies[i] times, copy-major, behind the copies of the plies before it (a capped engine's fast plies have 0 copies: traj_full is not read)
// OPEN: the opening's plies are not written and do not count among the tuples before a ply (their copies are 0 under SURPRISE)
template <bool LIST, bool CAP, bool SYM, bool SURPRISE, bool OPEN>
__device__ __forceinline__ void emit_tuples_body(Dev d, const uint8_t *traj_full, float *states, double *pis, float *zs, long long capacity,
                                                 const unsigned long long *cursor, const int *list, const int *n_list, const EmitSym &es,
                                                 const uint16_t *traj_copies, const OpenEmit &oe) {
    const int S = d.g.state_dim, A = d.g.action_dim, rc = d.g.rc, F = d.g.planes, N = d.g.rows;
    const int lane = azk_lane();
    const int nb = LIST ? *n_list * S : (int)gridDim.x;
    for (int blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    if (LIST && blk != (int)blockIdx.x) __syncthreads();
    const int gi = blk / S, i = blk - gi * S;
    const int g = LIST ? list[gi] : gi;
    const long long base = d.emit_base[g];
    if (base < 0 || i >= d.move_count[g]) continue;
    int o = 0;                                                    // the first ply that had a search
    if constexpr (OPEN) { o = uniform_i32(oe.open_plies[g]); if (i < o) continue; }   // an opening ply: it was drawn, not searched
    if (CAP && !SURPRISE && traj_full[(size_t)g * S + i] == 0) continue;      // a fast ply: it chose the move, it is not trained on
    const int copies = SURPRISE ? (int)traj_copies[(size_t)g * S + i] : 1;
    if (SURPRISE && copies == 0) continue;                        // no copy of this ply: the coin rounded its weight down to none (or a fast ply)
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    uint8_t *cells = sm;                                          // board before ply i
    for (int c = lane; c < rc; c += AZK_WAVE) cells[c] = 0;
    __syncthreads();
    const int16_t *acts = d.traj_action + (size_t)g * S;
    for (int j = lane; j < i; j += AZK_WAVE) cells[acts[j]] = (uint8_t)(1 << (j & 1));
    __syncthreads();
    const int side = i & 1, winner = d.winner[g];
    const float z = winner == -1 ? 0.0f : (side == winner ? 1.0f : -1.0f);
    const double *pi = d.traj_pi + ((size_t)g * S + i) * A;
    const int grp = SYM ? es.n : 8;
    const int ntr = i < 2 ? 1 : grp;
    long long first = base + (i < 2 ? i : 2 + grp * (i - 2));
    if (OPEN) first -= o < 2 ? o : 2 + grp * (o - 2);
    if (CAP && !SURPRISE) {                                       // tuples of the full plies before this one
        int before = 0;
        for (int j = o + lane; j < i; j += AZK_WAVE) if (traj_full[(size_t)g * S + j]) before += j < 2 ? 1 : grp;
        first = base + wave_sum_i32(before);
    }
    if (SURPRISE) {                                               // tuples of every copy of the plies before this one
        int before = 0;
        for (int j = lane; j < i; j += AZK_WAVE) before += (int)traj_copies[(size_t)g * S + j] * (j < 2 ? 1 : grp);
        first = base + wave_sum_i32(before);
    }
    const long long stream_end = (long long)*cursor;              // after k_emit_alloc: one past the newest tuple of this call
    for (int tt = 0; tt < ntr * copies; tt++) {
        const int t = SURPRISE ? tt % ntr : tt;                   // copy-major: copy tt / ntr of the group's tuple t
        if (first + tt < stream_end - capacity) continue;         // already pushed out of the ring by newer tuples (deque(maxlen))
        const long long slot = (first + tt) % capacity;
        float *so = states + (size_t)slot * F * rc;
        double *po = pis + (size_t)slot * A;
        const int el = SYM ? (int)((es.els >> (4 * t)) & 15u) : t;   // (plies 0 and 1: t = 0 and the mask's first element is the identity)
        for (int e = lane; e < rc; e += AZK_WAVE) {
            const int src = SYM ? sym_source(el, e, d.g.rows, d.g.cols, d.g.inv_cols) : d4_source(t, e / N, e % N, N);
            const uint8_t code = cells[src];
            so[e] = (float)((code >> side) & 1);                    // canonical: own stones first (gomoku.py:34-40)
            so[rc + e] = (float)((code >> (side ^ 1)) & 1);
            if (F == 3) so[2 * rc + e] = (float)side;
            if (!SYM || A == rc) po[e] = pi[src];                   // one action per cell: action index == cell index
        }
        if (SYM && A != rc)                                         // Connect4's columns, a -> cols - 1 - a under lr: the cells' map on a board of one row
            for (int a = lane; a < A; a += AZK_WAVE) po[a] = pi[sym_source(el, a, 1, A, 0u)];
        if (lane == 0) zs[slot] = z;
    }
    }
}

template <bool LIST, bool CAP, bool SYM, bool SURPRISE, bool OPEN>
__global__ __launch_bounds__(AZK_WAVE) void k_emit_tuples(EmitPack<CAP, SYM, SURPRISE, OPEN> a, float *states, double *pis, float *zs, long long capacity,
                                                            const unsigned long long *cursor, const int *list, const int *n_list) {
    emit_tuples_body<LIST, CAP, SYM, SURPRISE, OPEN>(a, opt<CapDev>(a).traj_full, states, pis, zs, capacity, cursor, list, n_list, opt<EmitSym>(a),
                                                     opt<SurpriseDev>(a).traj_copies, opt<OpenEmit>(a));
}

__global__ void k_emit_mark(Dev d) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < d.G && d.done[g] == 1 && d.emit_base[g] >= 0) d.done[g] = 2;      // emitted; recycle / later calls skip it
}

__global__ void k_sum_counters(const long long *counters, int G, long long *out) {
    // one block per counter
    __shared__ long long sm[256];
    long long s = 0;
    for (int i = threadIdx.x; i < G; i += blockDim.x) s += counters[(size_t)blockIdx.x * G + i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

// ------------------------------------------------------------------------------------------------
// Counter-based RNG for the product path: Philox4x32-10 (philox4x32_10, above) keyed by (seed), counter = (game, move, lane idx, draw).
// Dirichlet(alpha) via Gamma(alpha) = Gamma(alpha + 1) * U^(1/alpha) (Marsaglia-Tsang for the shape > 1 part).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {     // uniform in (0, 1)
    const unsigned long long x = (((unsigned long long)hi << 32) | lo) >> 11;
    return ((double)x + 0.5) * (1.0 / 9007199254740992.0);
}

// the uniform of (seed, global game, move): np.random.choice's draw of that move
__device__ __forceinline__ double noise_uniform(unsigned long long seed, unsigned long long gg, int move) {
    uint32_t c[4] = {(uint32_t)gg, (uint32_t)(gg >> 32), (uint32_t)move, 0xFFFFFFFFu};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (double)((((unsigned long long)c[0] << 32) | c[1]) >> 11) * (1.0 / 9007199254740992.0);   // [0,1)
}

// the Dirichlet(alpha) row of (seed, global game, move), by one wave; red: 64 doubles of LDS scratch
__device__ __forceinline__ void noise_row(int A, unsigned long long seed, unsigned long long gg, int move, double alpha, double *row, double *red) {
    const int lane = azk_lane();
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double part = 0.0;
    for (int a = lane; a < A; a += AZK_WAVE) {
        const double d = alpha + 1.0 - 1.0 / 3.0, cc = 1.0 / sqrt(9.0 * d);
        double gam = 0.0;
        for (uint32_t it = 0; it < 64; it++) {
            uint32_t c[4] = {(uint32_t)gg, (uint32_t)(gg >> 32) ^ ((uint32_t)a << 8), (uint32_t)move, it};
            philox4x32_10(c, k0, k1);
            uint32_t c2[4] = {(uint32_t)gg, (uint32_t)(gg >> 32) ^ ((uint32_t)a << 8), (uint32_t)move, it | 0x40000000u};
            philox4x32_10(c2, k0, k1);
            const double u1 = u53(c[0], c[1]), u2 = u53(c[2], c[3]), u3 = u53(c2[0], c2[1]), u4 = u53(c2[2], c2[3]);
            const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
            const double t = 1.0 + cc * x;
            if (t <= 0.0) continue;
            const double v = t * t * t;
            if (log(u3) < 0.5 * x * x + d - d * v + d * log(v)) { gam = d * v * pow(u4, 1.0 / alpha); break; }
        }
        row[a] = gam;
        part += gam;
    }
    red[lane] = part;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) { if (lane < o) red[lane] += red[lane + o]; __syncthreads(); }
    const double tot = red[0];
    for (int a = lane; a < A; a += AZK_WAVE) row[a] = tot > 0.0 ? row[a] / tot : 1.0 / (double)A;
    __syncthreads();
}

__global__ __launch_bounds__(AZK_WAVE) void k_gen_noise(int A, unsigned long long seed, long long first_game, int move,
                                                         double alpha, double *noise, double *uniforms, long long row_stride) {
    const int g = blockIdx.x, lane = azk_lane();
    const unsigned long long gg = (unsigned long long)(first_game + g);
    __shared__ double red[AZK_WAVE];
    if (uniforms && lane == 0) uniforms[g] = noise_uniform(seed, gg, move);
    if (!noise) return;
    noise_row(A, seed, gg, move, alpha, noise + (size_t)g * (size_t)row_stride, red);
}

// The Gumbel(0, 1) row of (seed, global game, move), by one wave (Gumbel root search): entry a draws ONE Philox block at
// counter {gg lo, gg hi ^ (a << 8), move, 0xFFFFFFFB} - a word 3 that is no other stream's -, u = (((c0 << 32 | c1) >> 12) + 0.5) * 2^-52
// (exact, strictly inside (0, 1)) and g = -log(-log(u)).
__device__ __forceinline__ void gumbel_row(int A, unsigned long long seed, unsigned long long gg, int move, double *row, double *urow = nullptr) {
    for (int a = azk_lane(); a < A; a += AZK_WAVE) {
        uint32_t c[4] = {(uint32_t)gg, (uint32_t)(gg >> 32) ^ ((uint32_t)a << 8), (uint32_t)move, 0xFFFFFFFBu};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        const double u = ((double)((((unsigned long long)c[0] << 32) | c[1]) >> 12) + 0.5) * (1.0 / 4503599627370496.0);
        if (row != nullptr) row[a] = -log(-log(u));
        if (urow != nullptr) urow[a] = u;
    }
}

__global__ __launch_bounds__(AZK_WAVE) void k_gen_gumbel(int A, unsigned long long seed, long long first_game, int move, double *rows, double *uniforms,
                                                          long long row_stride) {
    const int g = blockIdx.x;
    const size_t o = (size_t)g * (size_t)row_stride;
    gumbel_row(A, seed, (unsigned long long)(first_game + g), move, rows != nullptr ? rows + o : nullptr, uniforms != nullptr ? uniforms + o : nullptr);
}

// ------------------------------------------------------------------------------------------------
// Asynchronous self-play (games/gomoku.py:132-162: a game moves as soon as ITS search is done).  After every tree launch
// k_move_async looks at every game: one whose search is complete (its simulation budget used up, nothing pending) gets its move
// - root statistics, pi into the trajectory, sampled / most-visited child, make_move, check_winner, a record into the device
// ring - and, unless the game ended, its next search at once: fresh root, Dirichlet row of (seed, global game, the slot's move
// counter).  Finished games wait for azk_async_drain ((state, pi, z) emission, statistics, restart), which the host runs every
// few launches.  Random numbers are keyed by (seed, global game index, per-slot move counter): exactly the keys of the lock-step
// driver, so a slot plays the same sequence of games move for move, whatever the timing.
// A re-rooting engine (azk_async_begin_reuse) does not begin the next search in the move kernel: re-rooting a large subtree is a
// dependent chain of some hundred memory round trips for ONE wave, and every launch of the step chain would last that long.  The
// move kernel notes the played child and PARKS the game - its parked word set, sims_done at the largest int so that k_tree idles it
// whatever the budget becomes - on a list; the drain re-roots the listed games (k_reroot_list) and un-parks them.  The kernel
// boundary is the only ordering relied on.
// ------------------------------------------------------------------------------------------------
// Node(None, None, player, move_count) for one game (one wave).  The search's Dirichlet row is NOT made here: a row's key (seed, global
// game, slot move counter) is known a whole search before its use, so the rows are generated one search ahead, off the step's chain
// (k_noise_ahead in the drain) - in this function the Marsaglia-Tsang chain (float64 log / cos / pow, two Philox blocks per try) cost a
// moving game's wave ~30 us inside a launch every other wave had left after 1 us.
__device__ __forceinline__ void begin_search_one(const Dev &d, const AsyncDev &p, int g) {
    if (azk_lane() == 0) {
        fresh_root_one(d, g);
        atomicAdd((unsigned long long *)&p.stats[7], 1ull);
    }
}

// drain: the Dirichlet rows that fell due since the last drain - for every game that moved, the row of the search AFTER the one it has
// just begun (key slot_moves[g] + 1, into the buffer the finished search read from)
__global__ __launch_bounds__(AZK_WAVE) void k_noise_ahead(Dev d, AsyncDev p) {
    __shared__ double red[AZK_WAVE];
    const int n = *p.todo_count, A = d.g.action_dim;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        const int g = p.todo_list[f];
        const int key = (int)p.slot_moves[g] + 1;
        if (uniform_i32(p.noise_key[g]) >= key) continue;
        noise_row(A, p.seed, (unsigned long long)(p.first_game + g), key, p.alpha, p.noise + ((size_t)g * 2 + (size_t)(key & 1)) * A, red);
        if (azk_lane() == 0) p.noise_key[g] = key;
        __syncthreads();
    }
}

// ... and its Gumbel form (an engine with a Gumbel root keeps Gumbel rows where the others keep Dirichlet rows)
__global__ __launch_bounds__(AZK_WAVE) void k_gumbel_ahead(Dev d, AsyncDev p) {
    const int n = *p.todo_count, A = d.g.action_dim;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        const int g = p.todo_list[f];
        const int key = (int)p.slot_moves[g] + 1;
        if (uniform_i32(p.noise_key[g]) >= key) continue;
        gumbel_row(A, p.seed, (unsigned long long)(p.first_game + g), key, p.noise + ((size_t)g * 2 + (size_t)(key & 1)) * A);
        __syncthreads();
        if (azk_lane() == 0) p.noise_key[g] = key;
    }
}

__global__ void k_fill_i32(int *p, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// The asynchronous mover.  REROOT: a re-rooting engine - the moved game is parked for the drain's k_reroot_list instead of beginning its search
// here; CAP: the kind of the completed search goes into the record and traj_full, and the next fresh-root search flips its coin; RESIGN, FORCED:
// SURPRISE: as advance_one has them (the move key is the slot's move counter; kl and coin go into the record's columns too)
template <bool REROOT, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool GUMBEL = false>
__device__ __forceinline__ void move_async_body(Dev d, AsyncDev p, ReuseDev r, CapDev cp, ResignDev rs, const ForcedDev &fp, const SurpriseDev &sp,
                                                const GumbelDev &gb = GumbelDev{}) {
    const int g = blockIdx.x, lane = azk_lane();
    // one vector load for the three words that decide whether this game moves now (almost never: the wave then ends at once)
    const int *up = d.done + g;
    up = lane == 1 ? d.sims_done + g : up;
    up = lane == 2 ? d.leaf_node + g : up;
    up = lane == 3 ? d.budget : up;                                // (the simulation budget lives in device memory: azk_async_set_budget)
    up = (lane == 4 && p.dirichlet) ? p.noise_key + g : up;
    up = lane == 5 ? (const int *)(p.slot_moves + g) : up;         // (low word: a slot plays far fewer than 2^31 moves)
    if (REROOT) up = lane == 6 ? p.parked + g : up;                // a parked game has moved already: its sims_done passes any budget
    const int uw = *up;
    if (REROOT && __builtin_amdgcn_readlane(uw, 6) != 0) return;
    if (__builtin_amdgcn_readlane(uw, 0) != 0 || __builtin_amdgcn_readlane(uw, 1) < __builtin_amdgcn_readlane(uw, 3) || __builtin_amdgcn_readlane(uw, 2) >= 0) return;
    // the next search's Dirichlet row is made a search ahead (k_noise_ahead, every drain); a game whose whole search fitted between two
    // drains (tiny budgets only) waits for it - a scheduling delay, the game's moves do not change
    if (p.dirichlet && __builtin_amdgcn_readlane(uw, 4) < __builtin_amdgcn_readlane(uw, 5) + 1) return;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int A = d.g.action_dim;
    const size_t base = (size_t)g * d.cap;
    const long long mv = p.slot_moves[g];
    const double q = d.W[base] / (double)d.H[base].N;                 // root.value / root.visit (gomoku.py:140), before the tree is reset
    int win = -2, dn = 0, sum = 0, rsg = 0;
    const double u = noise_uniform(p.seed, (unsigned long long)(p.first_game + g), (int)mv);
    const int mc = CAP ? uniform_i32(d.move_count[g]) : 0;
    const int kind = CAP ? uniform_i32((int)cp.search_full[g]) : 1;     // of the search that is complete
    int cellc;
    if constexpr (GUMBEL) cellc = advance_one<RESIGN, false, false, true>(d, L, g, false, 0.0, 0, &win, &dn, &sum, rs, (int)mv, &rsg, fp, sp, gb);
    else cellc = advance_one<RESIGN, FORCED, SURPRISE>(d, L, g, true, u, p.sample_until, &win, &dn, &sum, rs, (int)mv, &rsg, fp, sp);
    if (cellc < 0) return;
    if (CAP && lane == 0 && cp.traj_full != nullptr && mc < d.g.state_dim) cp.traj_full[(size_t)g * d.g.state_dim + mc] = (uint8_t)kind;
    if (p.rec_cap > 0) {                                           // the move's record: what the reference's self_play keeps per ply
        long long slot = 0;
        if (lane == 0) slot = (long long)(atomicAdd((unsigned long long *)&p.stats[6], 1ull) % (unsigned long long)p.rec_cap);
        slot = ((long long)__builtin_amdgcn_readfirstlane((int)(slot >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)slot);
        if constexpr (GUMBEL) { for (int a = lane; a < A; a += AZK_WAVE) p.rec_pi[(size_t)slot * A + a] = L.cdf[a]; }
        else
        for (int a = lane; a < A; a += AZK_WAVE) p.rec_pi[(size_t)slot * A + a] = (double)L.cnt[a] / (double)sum;
        if (lane == 0) {
            p.rec_q[slot] = q;
            int *m = p.rec_meta + (size_t)slot * 4;
            m[0] = g; m[1] = (int)mv; m[2] = cellc; m[3] = win;
            if (CAP && cp.rec_full != nullptr) cp.rec_full[slot] = (uint8_t)kind;
            if (RESIGN && rs.rec_resigned != nullptr) rs.rec_resigned[slot] = (uint8_t)rsg;
            if (SURPRISE && sp.rec_kl != nullptr) sp.rec_kl[slot] = sp.last_kl[g];        // (this lane wrote the pair in advance_one)
            if (SURPRISE && sp.rec_coin != nullptr) sp.rec_coin[slot] = sp.last_coin[g];
        }
    }
    __syncthreads();
    if (lane == 0) {
        p.slot_moves[g] = mv + 1;                                  // the NEW search's key: its row (mv + 1) & 1 has been waiting since the last move
        atomicAdd((unsigned long long *)&p.stats[5], 1ull);
        if (p.dirichlet) p.todo_list[atomicAdd(p.todo_count, 1)] = g;          // row mv + 2 is due
    }
    __syncthreads();
    if (REROOT) {
        if (uniform_i32(dn)) return;                               // an ended game restarts from a fresh root in the drain, as ever
        const int child = played_child(d, g, cellc);
        if (lane == 0) {
            r.chosen_node[g] = child;
            d.sims_done[g] = 0x7fffffff;                           // no budget reaches this: k_tree and k_unfinished see a finished search
            p.parked[g] = 1;
            p.reroot_list[atomicAdd(p.reroot_count, 1)] = g;
        }
    } else if (!dn) {
        begin_search_one(d, p, g);
        if (CAP && lane == 0) cap_begin_fresh(d, cp, g, (int)mv + 1, true);
    }
}

template <bool REROOT, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE>
__global__ __launch_bounds__(AZK_WAVE) void k_move_async(Dev d, AsyncDev p, MovePack<ReuseDev, CAP, RESIGN, FORCED, SURPRISE> r) {
    move_async_body<REROOT, CAP, RESIGN, FORCED, SURPRISE>(d, p, r, opt<CapDev>(r), opt<ResignDev>(r), opt<ForcedDev>(r), opt<SurpriseDev>(r));
}

// the asynchronous mover of an engine with a Gumbel root (no re-rooting, no cap; with or without resignation)
template <bool RESIGN>
__global__ __launch_bounds__(AZK_WAVE) void k_move_async(Dev d, AsyncDev p, GumbelPack<ReuseDev, RESIGN> r) {
    move_async_body<false, false, RESIGN, false, false, true>(d, p, r, CapDev{}, opt<ResignDev>(r), ForcedDev{}, SurpriseDev{}, opt<GumbelDev>(r));
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

// drain, step 1: list the finished games (done == 1) - the emission and restart kernels work through the list only
__global__ void k_async_list(Dev d, AsyncDev p) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < d.G && d.done[g] != 0) p.fin_list[atomicAdd(p.fin_count, 1)] = g;
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

// azk_root_policy_target: the pi the next move would record - k_root_stats' counts, pruned where the game's search is a forced one
__global__ __launch_bounds__(AZK_WAVE) void k_root_policy_target(Dev d, ForcedDev fp, double *pi) {
    const int g = blockIdx.x, lane = azk_lane();
    const size_t base = (size_t)g * d.cap;
    const int A = d.g.action_dim;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    for (int a = lane; a < A; a += AZK_WAVE) L.cnt[a] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        L.cnt[azk_action_idx(d.g, meta_cell(d.H[base + fc + i].meta))] = n;
        sum += n;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    if (nch > 0 && sum > 0 && forced_search(d, fp, g)) sum = prune_counts(d, L, g, fp.k);
    for (int a = lane; a < A; a += AZK_WAVE) pi[(size_t)g * A + a] = (double)L.cnt[a] / (double)sum;
}

// ... and of an engine with a Gumbel root: gumbel_target's row
__global__ __launch_bounds__(AZK_WAVE) void k_root_policy_target_gumbel(Dev d, GumbelDev gb, double *pi) {
    const int g = blockIdx.x, lane = azk_lane();
    const int A = d.g.action_dim;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const bool searched = uniform_i32(meta_nch(d.H[(size_t)g * d.cap].meta)) > 0 && uniform_i32(d.root_f64[g]) != 0;
    if (searched) gumbel_target(d, L, g, gb);
    for (int a = lane; a < A; a += AZK_WAVE) pi[(size_t)g * A + a] = searched ? L.cdf[a] : 0.0;
}

// ---- the host side of the options: runtime flags -> template arguments, engine state -> argument packs ----------------------------------
// f(std::bool_constant per flag), called once: the one place where a kernel's instantiation is chosen
template <class F> void with_flags(F &&f) { f(); }
template <class F, class... Rest> void with_flags(F &&f, bool flag, Rest... rest) {
    if (flag) with_flags([&](auto... more) { f(std::true_type{}, more...); }, rest...);
    else with_flags([&](auto... more) { f(std::false_type{}, more...); }, rest...);
}
// the option's block as a pack takes it: the block where the flag is set, nothing where it is not
template <bool ON, class Block> Opt<Block, ON> on(const Block &b) {
    if constexpr (ON) return {b};
    else return {};
}
template <bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, class First>
MovePack<First, CAP, RESIGN, FORCED, SURPRISE> move_pack(const First &first, const azk_engine *e) {
    return {first, on<CAP>(e->cp), on<RESIGN>(e->rs), on<FORCED>(e->forced()), on<SURPRISE>(e->sp)};
}
template <bool CAP, class First> CapKeyPack<First, CAP> cap_key_pack(const First &first, const azk_engine *e, int key) {
    return {first, on<CAP>(Keyed<CapDev>{e->cp, key})};
}

}  // namespace

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
}

// (state, pi, z) emission on the stream: each finished game's tuple range, the tuples, done = 2.  list == nullptr: one block per (game, ply)
// of all G games; else the blocks walk the *n_list listed games (asynchronous drain).  A capped engine emits the plies of full searches only
static void launch_emit(azk_engine *e, float *states, double *pis, float *zs, long long capacity, unsigned long long *cursor, long long *game_base,
                        const int *list, const int *n_list, hipStream_t st) {
    const Dev &d = e->d;
    const unsigned per_game = (unsigned)((d.G + 255) / 256), lds = (unsigned)up16(d.g.rc);
    const int plies = d.G * d.g.state_dim;
    const unsigned blocks = (unsigned)(list && plies > 16384 ? 16384 : plies);
    with_flags([&](auto by_list, auto cap, auto sym, auto surprise, auto open) {   // sym: emit_elements, the mask's elements on any geometry
        const EmitPack<cap.value, sym.value, surprise.value, open.value> a{d, on<cap.value>(e->cp), on<sym.value>(e->emit), on<surprise.value>(e->sp),
                                                                           on<open.value>(OpenEmit{e->op.open_plies})};
        k_emit_alloc<cap.value, sym.value, surprise.value, open.value><<<per_game, 256, 0, st>>>(a, cursor, game_base);
        k_emit_tuples<by_list.value, cap.value, sym.value, surprise.value, open.value><<<blocks, AZK_WAVE, lds, st>>>(a, states, pis, zs, capacity, cursor, list,
                                                                                                                     n_list);
    }, list != nullptr, e->cp.n_fast != 0, e->emit.n != 0, e->sp_on, e->op_on);
    k_emit_mark<<<per_game, 256, 0, st>>>(d);
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
        // the budget lives in device memory so that a captured step graph keeps working when it changes
        e->budget_host[0] = n_sims; e->budget_host[1] = max_sims_per_launch; e->budget_host[2] = 0;
        if (e->d.K > 1) e->budget_host[1] = e->d.K;               // virtual-loss mode: one iteration per slot
        HIPCHK(e, hipMemcpyAsync(e->d.budget, e->budget_host, sizeof e->budget_host, hipMemcpyHostToDevice, (hipStream_t)stream));
        HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
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

// ---- playout-cap randomisation ---------------------------------------------------------------------------------------------
int32_t azk_set_playout_cap(azk_engine *e, double p_full, int32_t n_fast, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_playout_cap: set the cap before azk_async_begin"; return AZK_ERR_STATE; }
    if (n_fast == 0) { e->cp.n_fast = 0; return AZK_OK; }         // off: the engine launches what it launched before
    if (e->gb.m) { e->err = "azk_set_playout_cap: a Gumbel root is set - its halving table is built for one budget"; return AZK_ERR_STATE; }
    if (!(p_full >= 0.0 && p_full <= 1.0)) { e->err = "azk_set_playout_cap: p_full must lie in [0, 1]"; return AZK_ERR_ARG; }
    if (n_fast < 1 || n_fast > e->cfg.max_sims) { e->err = "azk_set_playout_cap: n_fast must lie in [1, max_sims]"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_playout_cap: a playout cap does not combine with leaves_per_step > 1 (virtual loss counts completed simulations differently)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    CapDev &c = e->cp;
    if (!c.search_full) {
        HIPCHK(e, dalloc(e, &c.search_full, (size_t)d.G));
        if (d.traj_pi) HIPCHK(e, dalloc(e, &c.traj_full, (size_t)d.G * d.g.state_dim));
    }
    HIPCHK(e, hipMemsetAsync(c.search_full, 1, (size_t)d.G, (hipStream_t)stream));
    if (c.traj_full) HIPCHK(e, hipMemsetAsync(c.traj_full, 1, (size_t)d.G * d.g.state_dim, (hipStream_t)stream));
    c.p_full = p_full; c.seed = seed; c.first_game = first_global_game; c.stats = nullptr; c.rec_full = nullptr;
    c.n_fast = n_fast;
    return AZK_OK;
}

int32_t azk_begin_search_capped(azk_engine *e, const double *noise_dev, int32_t n_sims, int32_t max_sims_per_launch, int32_t move_index, void *stream) {
    if (!e || n_sims < 1 || n_sims > e->cfg.max_sims || max_sims_per_launch < 1 || move_index < 0) { if (e) e->err = "azk_begin_search_capped: bad argument"; return AZK_ERR_ARG; }
    if (!e->cp.n_fast) { e->err = "azk_begin_search_capped: no playout cap is set (azk_set_playout_cap)"; return AZK_ERR_STATE; }
    if (e->cp.n_fast > n_sims) { e->err = "azk_begin_search_capped: n_fast exceeds n_sims"; return AZK_ERR_ARG; }
    if (forced_needs_noise(e, noise_dev, "azk_begin_search_capped")) return AZK_ERR_STATE;
    return begin_budget(e, noise_dev, n_sims, max_sims_per_launch, move_index, stream);
}

int32_t azk_get_search_full(azk_engine *e, uint8_t *full_dev, void *stream) {
    if (!e || !full_dev) return AZK_ERR_ARG;
    if (!e->cp.n_fast) { e->err = "azk_get_search_full: no playout cap is set (azk_set_playout_cap)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(full_dev, e->cp.search_full, (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_record_flags(azk_engine *e, uint8_t *rec_full_dev) {
    if (!e) return AZK_ERR_ARG;
    if (!e->cp.n_fast) { e->err = "azk_async_record_flags: no playout cap is set (azk_set_playout_cap)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_record_flags: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->cp.rec_full = rec_full_dev;
    return AZK_OK;
}

// ---- forced playouts and policy target pruning ------------------------------------------------------------------------------
int32_t azk_set_forced_playouts(azk_engine *e, double k, void *stream) {
    (void)stream;
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_forced_playouts: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!(k >= 0.0) || k - k != 0.0) { e->err = "azk_set_forced_playouts: k must be finite and not negative (0 = off)"; return AZK_ERR_ARG; }
    if (k == 0.0) { e->forced_k = 0.0; return AZK_OK; }              // off: the engine launches what it launched before
    if (e->gb.m) { e->err = "azk_set_forced_playouts: a Gumbel root is set - its eligibility rule needs raw root selection"; return AZK_ERR_STATE; }
    if (e->d.K > 1) { e->err = "azk_set_forced_playouts: forced playouts do not combine with leaves_per_step > 1 (a virtual-loss search counts a visit before its value exists: the floor would be met by visits that carry nothing)"; return AZK_ERR_ARG; }
    e->forced_k = k;
    return AZK_OK;
}

// ---- Gumbel root search -----------------------------------------------------------------------------------------------------
// schedule(m, n): the visit count a root child must have at each of the n root selections of a search that halves m sampled children
static void gumbel_schedule(int m, int n, int *out) {
    if (m <= 1) { for (int t = 0; t < n; t++) out[t] = t; return; }
    int L = 0;
    while ((1 << L) < m) L++;
    std::vector<int> v((size_t)m, 0);
    int c = m, len = 0;
    while (len < n) {
        const int extra = std::max(1, n / (L * c));
        for (int x = 0; x < extra && len < n; x++)
            for (int i = 0; i < c; i++) { if (len < n) out[len++] = v[i]; v[i] += 1; }
        c = std::max(2, c / 2);
    }
}

int32_t azk_set_gumbel_root(azk_engine *e, int32_t m, int32_t n_sims, double c_visit, double c_scale, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_gumbel_root: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (m < 1 || m > 64) { e->err = "azk_set_gumbel_root: m must lie in [1, 64]"; return AZK_ERR_ARG; }
    if (n_sims < 2 || n_sims > e->cfg.max_sims) { e->err = "azk_set_gumbel_root: n_sims must lie in [2, max_sims]"; return AZK_ERR_ARG; }
    if (!(c_visit >= 0.0) || c_visit - c_visit != 0.0) { e->err = "azk_set_gumbel_root: c_visit must be finite and not negative"; return AZK_ERR_ARG; }
    if (!(c_scale > 0.0) || c_scale - c_scale != 0.0) { e->err = "azk_set_gumbel_root: c_scale must be finite and positive"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with leaves_per_step > 1 (a virtual-loss search counts a visit before its value exists: eligibility by visit count would pass over it)"; return AZK_ERR_ARG; }
    if (e->ru.mode) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with tree reuse (the eligibility rule needs a fresh root: every child at 0 visits)"; return AZK_ERR_STATE; }
    if (e->cp.n_fast) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with a playout cap (the halving table is built for one budget)"; return AZK_ERR_STATE; }
    if (e->forced_k != 0.0) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with forced playouts (the eligibility rule needs raw root selection)"; return AZK_ERR_STATE; }
    if (e->sp_on) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with surprise weighting (its recorded pi is not a visit distribution)"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    GumbelDev &gb = e->gb;
    hipStream_t st = (hipStream_t)stream;
    const int n = n_sims - 1;
    std::vector<int> table((size_t)(m + 1) * n);
    for (int mm = 0; mm <= m; mm++) gumbel_schedule(mm, n, table.data() + (size_t)mm * n);
    int *tab = nullptr;                                              // (a table of its own per call: a captured step graph may still hold the last one)
    HIPCHK(e, dalloc(e, &tab, table.size()));
    if (!gb.logit) {
        HIPCHK(e, dalloc(e, &gb.logit, (size_t)d.G * d.g.rc));
        HIPCHK(e, dalloc(e, &gb.v0, (size_t)d.G));
        HIPCHK(e, hipMemsetAsync(gb.logit, 0, sizeof(float) * (size_t)d.G * d.g.rc, st));
        HIPCHK(e, hipMemsetAsync(gb.v0, 0, sizeof(float) * (size_t)d.G, st));
    }
    HIPCHK(e, hipMemcpyAsync(tab, table.data(), sizeof(int) * table.size(), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipStreamSynchronize(st));
    gb.table = tab; gb.n = n; gb.c_visit = c_visit; gb.c_scale = c_scale;
    gb.m = m;
    e->gumbel_sims = n_sims;
    return AZK_OK;
}

int32_t azk_clear_gumbel_root(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_gumbel_root: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->gb.m = 0;                                                   // off: the engine launches what it launched before
    return AZK_OK;
}

static int32_t gen_gumbel(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *gumbel_dev, double *uniforms_dev, void *stream) {
    k_gen_gumbel<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(e->d.g.action_dim, seed, first_global_game, move_index, gumbel_dev, uniforms_dev,
                                                             (long long)e->d.g.action_dim);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_gen_gumbel(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *gumbel_dev, void *stream) {
    if (!e || !gumbel_dev) return AZK_ERR_ARG;
    return gen_gumbel(e, seed, first_global_game, move_index, gumbel_dev, nullptr, stream);
}

int32_t azk_gen_gumbel_uniforms(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *uniforms_dev, void *stream) {
    if (!e || !uniforms_dev) return AZK_ERR_ARG;
    return gen_gumbel(e, seed, first_global_game, move_index, nullptr, uniforms_dev, stream);
}

int32_t azk_root_policy_target(azk_engine *e, double *pi_dev, void *stream) {
    if (!e || !pi_dev) return AZK_ERR_ARG;
    if (e->gb.m) k_root_policy_target_gumbel<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, e->gb, pi_dev);
    else if (e->forced_k == 0.0) k_root_stats<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, pi_dev, nullptr, nullptr);
    else k_root_policy_target<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, e->forced(), pi_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

// ---- resignation ------------------------------------------------------------------------------------------------------
// no game resigned, no mark, zero statistics (azk_set_resign, and azk_async_begin where the slots' move counters start again at 0)
static int32_t resign_clear(azk_engine *e, hipStream_t st) {
    const ResignDev &r = e->rs;
    HIPCHK(e, hipMemsetAsync(r.resigned, 0, (size_t)e->d.G, st));
    HIPCHK(e, hipMemsetAsync(r.mark_start, 0, sizeof(uint32_t) * (size_t)e->d.G, st));
    HIPCHK(e, hipMemsetAsync(r.mark_side, 0xff, sizeof(int) * (size_t)e->d.G, st));
    HIPCHK(e, hipMemsetAsync(r.stats, 0, sizeof(long long) * 4, st));
    return AZK_OK;
}

int32_t azk_set_resign(azk_engine *e, double v_resign, int32_t min_ply, double p_never, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_resign: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!(v_resign >= 0.0 && v_resign <= 1.0)) { e->err = "azk_set_resign: v_resign must lie in [0, 1] (0 = off)"; return AZK_ERR_ARG; }
    if (!(p_never >= 0.0 && p_never <= 1.0)) { e->err = "azk_set_resign: p_never must lie in [0, 1]"; return AZK_ERR_ARG; }
    if (min_ply < 0) { e->err = "azk_set_resign: min_ply must not be negative"; return AZK_ERR_ARG; }
    if (v_resign == 0.0) { e->rs.v_resign = 0.0; return AZK_OK; }  // off: the engine launches what it launched before
    if (e->d.K > 1) { e->err = "azk_set_resign: resignation does not combine with leaves_per_step > 1 (a virtual-loss search is another search: its q is not the one a threshold was set on)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    ResignDev &r = e->rs;
    if (!r.resigned) {
        HIPCHK(e, dalloc(e, &r.resigned, (size_t)d.G));
        HIPCHK(e, dalloc(e, &r.mark_start, (size_t)d.G));
        HIPCHK(e, dalloc(e, &r.mark_side, (size_t)d.G));
        HIPCHK(e, dalloc(e, &r.stats, 4));
    }
    const int32_t rc = resign_clear(e, (hipStream_t)stream);
    if (rc != AZK_OK) return rc;
    r.min_ply = min_ply; r.p_never = p_never; r.seed = seed; r.first_game = first_global_game; r.rec_resigned = nullptr;
    r.v_resign = v_resign;
    return AZK_OK;
}

int32_t azk_get_resigned(azk_engine *e, uint8_t *resigned_dev, void *stream) {
    if (!e || !resigned_dev) return AZK_ERR_ARG;
    if (e->rs.v_resign == 0.0) { e->err = "azk_get_resigned: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(resigned_dev, e->rs.resigned, (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_resign_stats(azk_engine *e, int64_t *out4_host, void *stream) {
    if (!e || !out4_host) return AZK_ERR_ARG;
    if (e->rs.v_resign == 0.0) { e->err = "azk_get_resign_stats: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out4_host, e->rs.stats, sizeof(long long) * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_resign_flags(azk_engine *e, uint8_t *rec_resigned_dev) {
    if (!e) return AZK_ERR_ARG;
    if (e->rs.v_resign == 0.0) { e->err = "azk_async_resign_flags: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_resign_flags: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->rs.rec_resigned = rec_resigned_dev;
    return AZK_OK;
}

// ---- policy surprise weighting ------------------------------------------------------------------------------------------
int32_t azk_set_surprise_weighting(azk_engine *e, double lambda, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_surprise_weighting: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->gb.m) { e->err = "azk_set_surprise_weighting: a Gumbel root is set - its recorded pi is not a visit distribution, which the weight is defined on"; return AZK_ERR_STATE; }
    if (!(lambda >= 0.0 && lambda <= 1.0)) { e->err = "azk_set_surprise_weighting: lambda must lie in [0, 1] (azk_clear_surprise_weighting switches the option off)"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_surprise_weighting: surprise weighting does not combine with leaves_per_step > 1 (a virtual-loss search's visit counts are not the ones the weight was defined on)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    if (!d.traj_pi) { e->err = "azk_set_surprise_weighting: the engine records no trajectories (a square board with one action per cell, or an engine created with emit_elements)"; return AZK_ERR_ARG; }
    SurpriseDev &s = e->sp;
    const size_t plies = (size_t)d.G * d.g.state_dim;
    if (!s.traj_kl) {
        HIPCHK(e, dalloc(e, &s.traj_kl, plies));
        HIPCHK(e, dalloc(e, &s.traj_coin, plies));
        HIPCHK(e, dalloc(e, &s.traj_copies, plies));
        HIPCHK(e, dalloc(e, &s.last_kl, (size_t)d.G));
        HIPCHK(e, dalloc(e, &s.last_coin, (size_t)d.G));
    }
    HIPCHK(e, hipMemsetAsync(s.traj_kl, 0, sizeof(double) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.traj_coin, 0, sizeof(double) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.traj_copies, 0, sizeof(uint16_t) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.last_kl, 0, sizeof(double) * (size_t)d.G, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.last_coin, 0, sizeof(double) * (size_t)d.G, (hipStream_t)stream));
    s.lambda = lambda; s.seed = seed; s.first_game = first_global_game; s.rec_kl = nullptr; s.rec_coin = nullptr;
    e->sp_on = true;
    return AZK_OK;
}

int32_t azk_clear_surprise_weighting(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_surprise_weighting: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->sp_on = false;                                             // off: the engine launches what it launched before
    return AZK_OK;
}

int32_t azk_get_surprise(azk_engine *e, double *kl_dev, double *coin_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (!e->sp_on) { e->err = "azk_get_surprise: no surprise weighting is set (azk_set_surprise_weighting)"; return AZK_ERR_STATE; }
    if (kl_dev) HIPCHK(e, hipMemcpyAsync(kl_dev, e->sp.last_kl, sizeof(double) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (coin_dev) HIPCHK(e, hipMemcpyAsync(coin_dev, e->sp.last_coin, sizeof(double) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_surprise_columns(azk_engine *e, double *rec_kl_dev, double *rec_coin_dev) {
    if (!e) return AZK_ERR_ARG;
    if (!e->sp_on) { e->err = "azk_async_surprise_columns: no surprise weighting is set (azk_set_surprise_weighting)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_surprise_columns: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->sp.rec_kl = rec_kl_dev; e->sp.rec_coin = rec_coin_dev;
    return AZK_OK;
}

// ---- random openings -------------------------------------------------------------------------------------------------------
int32_t azk_set_openings(azk_engine *e, double p_open, int32_t max_plies, int32_t spread, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_openings: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!(p_open >= 0.0 && p_open <= 1.0)) { e->err = "azk_set_openings: p_open must lie in [0, 1] (azk_clear_openings switches the option off)"; return AZK_ERR_ARG; }
    if (max_plies < 1 || max_plies > e->d.g.state_dim - 1) { e->err = "azk_set_openings: max_plies must lie in [1, state_dim - 1]"; return AZK_ERR_ARG; }
    if (spread < -1) { e->err = "azk_set_openings: spread must be -1 (the whole board) or >= 0"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    OpenDev &o = e->op;
    hipStream_t st = (hipStream_t)stream;
    if (!o.pending) {
        HIPCHK(e, dalloc(e, &o.pending, (size_t)d.G));
        HIPCHK(e, dalloc(e, &o.open_plies, (size_t)d.G));
        HIPCHK(e, dalloc(e, &o.stats, 3));
        HIPCHK(e, dalloc(e, &o.actions, (size_t)d.G * d.g.state_dim));
    }
    // every slot is looked at by the next azk_open_pending (or azk_async_begin), which opens the games that have not started yet
    HIPCHK(e, hipMemsetAsync(o.pending, 1, (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(o.open_plies, 0, sizeof(int) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(o.stats, 0, sizeof(long long) * 3, st));
    o.p_open = p_open; o.max_plies = max_plies; o.spread = spread; o.seed = seed; o.first_game = first_global_game;
    e->op_on = true;
    return AZK_OK;
}

int32_t azk_clear_openings(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_openings: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->op_on = false;                                             // off: the engine launches what it launched before
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

int32_t azk_get_open_plies(azk_engine *e, int32_t *open_plies_dev, void *stream) {
    if (!e || !open_plies_dev) return AZK_ERR_ARG;
    if (!e->op_on) { e->err = "azk_get_open_plies: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(open_plies_dev, e->op.open_plies, sizeof(int) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_opening_actions(azk_engine *e, int16_t *actions_dev, void *stream) {
    if (!e || !actions_dev) return AZK_ERR_ARG;
    if (!e->op_on) { e->err = "azk_get_opening_actions: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(actions_dev, e->op.actions, sizeof(int16_t) * (size_t)e->d.G * e->d.g.state_dim, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_leaf_flags(azk_engine *e, uint8_t *flags_dev, void *stream) {
    if (!e || !flags_dev) return AZK_ERR_ARG;
    HIPCHK(e, hipMemcpyAsync(flags_dev, e->d.leaf_flag, (size_t)e->d.G * e->d.K, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_opening_stats(azk_engine *e, int64_t *out3_host, void *stream) {
    if (!e || !out3_host) return AZK_ERR_ARG;
    if (!e->op_on) { e->err = "azk_get_opening_stats: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out3_host, e->op.stats, sizeof(long long) * 3, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

// ---- asynchronous self-play ---------------------------------------------------------------------------------------------
static int32_t async_begin(azk_engine *e, const azk_async_config *c, void *stream, bool reuse) {
    if (!e || !c || !c->stats_dev || c->n_sims < 1 || c->n_sims > e->cfg.max_sims || c->max_sims_per_launch < 1 || !(c->alpha > 0.0)) {
        if (e) e->err = "azk_async_begin: bad argument";
        return AZK_ERR_ARG;
    }
    if (e->ru.mode && !reuse) { e->err = "azk_async_begin: a tree_reuse engine begins with azk_async_begin_reuse (games are parked and re-rooted in the drain)"; return AZK_ERR_STATE; }
    if (!e->ru.mode && reuse) { e->err = "azk_async_begin_reuse: the engine was created with tree_reuse = 0 (use azk_async_begin)"; return AZK_ERR_STATE; }
    if (c->record_capacity < 0 || (c->record_capacity > 0 && (!c->rec_meta_dev || !c->rec_q_dev || !c->rec_pi_dev))) { e->err = "azk_async_begin: record ring pointers missing"; return AZK_ERR_ARG; }
    if (e->cp.n_fast > c->n_sims) { e->err = "azk_async_begin: the playout cap's n_fast exceeds n_sims"; return AZK_ERR_ARG; }
    if (e->forced_k != 0.0 && !c->dirichlet) { e->err = "azk_async_begin: forced playouts are set - the searches need root noise (dirichlet = 1)"; return AZK_ERR_STATE; }
    if (e->gb.m && !c->dirichlet) { e->err = "azk_async_begin: a Gumbel root is set - the searches need their Gumbel rows (dirichlet = 1 makes the movers generate them)"; return AZK_ERR_STATE; }
    if (e->gb.m && reuse) { e->err = "azk_async_begin_reuse: a Gumbel root is set - it does not combine with re-rooting (the eligibility rule needs a fresh root)"; return AZK_ERR_STATE; }
    if (e->gb.m && c->n_sims != e->gumbel_sims) { e->err = "azk_async_begin: a Gumbel root is set - n_sims differs from the n_sims its halving table was built for (azk_set_gumbel_root)"; return AZK_ERR_STATE; }
    Dev &d = e->d;
    if (d.K > 1) { e->err = "azk_async_begin: asynchronous moves run the sequential search (leaves_per_step = 1)"; return AZK_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    AsyncDev &a = e->ad;
    if (!a.slot_moves) {
        HIPCHK(e, dalloc(e, &a.slot_moves, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.noise, (size_t)d.G * 2 * d.g.action_dim));
        HIPCHK(e, dalloc(e, &a.noise_key, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.todo_list, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.todo_count, 1));
        HIPCHK(e, dalloc(e, &a.fin_list, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.fin_count, 1));
    }
    if (reuse && !a.parked) {
        HIPCHK(e, dalloc(e, &a.parked, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.reroot_list, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.reroot_count, 1));
    }
    a.n_sims = c->n_sims; a.sample_until = c->sample_until_move; a.dirichlet = c->dirichlet ? 1 : 0;
    a.seed = c->seed; a.first_game = c->first_global_game; a.alpha = c->alpha;
    a.stats = (long long *)c->stats_dev; a.rec_cap = c->record_capacity; a.rec_meta = c->rec_meta_dev; a.rec_q = c->rec_q_dev; a.rec_pi = c->rec_pi_dev;
    e->async_recycle = c->recycle ? 1 : 0;
    HIPCHK(e, hipMemsetAsync(a.slot_moves, 0, sizeof(long long) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(a.stats, 0, sizeof(long long) * 16, st));
    if (reuse) {                                                  // nothing parked, no child noted: every game's first search starts from a fresh root
        HIPCHK(e, hipMemsetAsync(a.parked, 0, sizeof(int) * (size_t)d.G, st));
        HIPCHK(e, hipMemsetAsync(a.reroot_count, 0, sizeof(int), st));
        HIPCHK(e, hipMemsetAsync(e->ru.chosen_node, 0xff, sizeof(int) * (size_t)d.G, st));
    }
    // the simulation budget lives in device memory (a captured step graph keeps working when it changes)
    e->budget_host[0] = c->n_sims; e->budget_host[1] = c->max_sims_per_launch;
    e->budget_host[2] = c->young_launch_us > 0 ? c->young_launch_us * e->ticks_per_us : 0;
    HIPCHK(e, hipMemcpyAsync(d.budget, e->budget_host, sizeof e->budget_host, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipStreamSynchronize(st));
    d.noise = a.dirichlet ? a.noise : nullptr;
    d.noise_sel = a.dirichlet ? a.slot_moves : nullptr;
    e->multi = true;
    e->async_on = true;
    if (e->rs.v_resign != 0.0) {                                  // the game coins share the noise rows' key too
        e->rs.seed = a.seed; e->rs.first_game = a.first_game;
        const int32_t rc = resign_clear(e, st);
        if (rc != AZK_OK) return rc;
    }
    if (e->sp_on) { e->sp.seed = a.seed; e->sp.first_game = a.first_game; }      // ... and the ply coins of surprise weighting
    // first search of every game: fresh roots + the Dirichlet rows of move keys 0 (this search) and 1 (the next one)
    if (e->cp.n_fast) { e->cp.seed = a.seed; e->cp.first_game = a.first_game; e->cp.stats = a.stats; }   // the coins share the noise rows' key: this run's seed and first game
    if (e->op_on) k_open_pending<<<d.G, AZK_WAVE, d.lds_bytes, st>>>(d, e->op, 0);      // random openings: the first games, under move key 0
    with_flags([&](auto cap) { k_begin_search<cap.value><<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(cap_key_pack<cap.value>(d, e, 0)); }, e->cp.n_fast != 0);
    HIPCHK(e, hipMemsetAsync(a.todo_count, 0, sizeof(int), st));
    if (a.dirichlet) {
        const int A = d.g.action_dim;
        if (e->gb.m) {                                            // a Gumbel root: Gumbel rows where the others keep Dirichlet rows
            k_gen_gumbel<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 0, a.noise, nullptr, 2LL * A);
            k_gen_gumbel<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 1, a.noise + A, nullptr, 2LL * A);
        } else {
        k_gen_noise<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 0, a.alpha, a.noise, nullptr, 2LL * A);
        k_gen_noise<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 1, a.alpha, a.noise + A, nullptr, 2LL * A);
        }
        k_fill_i32<<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(a.noise_key, d.G, 1);
    }
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_async_begin(azk_engine *e, const azk_async_config *c, void *stream) { return async_begin(e, c, stream, false); }

int32_t azk_async_begin_reuse(azk_engine *e, const azk_async_config *c, void *stream) { return async_begin(e, c, stream, true); }

int32_t azk_async_step(azk_engine *e, const float *logits_dev, const float *values_dev, int32_t phases, void *stream) {
    if (!e || !e->async_on) { if (e) e->err = "azk_async_step: call azk_async_begin first"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    if (phases & 1) { const int32_t rc = azk_launch_tree(e, true, true, true, logits_dev, values_dev, st); if (rc != AZK_OK) return rc; }
    if ((phases & 2) && e->gb.m)
        with_flags([&](auto resign) {
            k_move_async<resign.value><<<d.G, AZK_WAVE, d.lds_bytes, st>>>(d, e->ad, GumbelPack<ReuseDev, resign.value>{e->ru, on<resign.value>(e->rs), on<true>(e->gb)});
        }, e->rs.v_resign != 0.0);
    else if (phases & 2)
        with_flags([&](auto reroot, auto cap, auto resign, auto forced, auto surprise) {
            k_move_async<reroot.value, cap.value, resign.value, forced.value, surprise.value><<<d.G, AZK_WAVE, d.lds_bytes, st>>>(
                d, e->ad, move_pack<cap.value, resign.value, forced.value, surprise.value>(e->ru, e));
        }, e->ru.mode != 0, e->cp.n_fast != 0, e->rs.v_resign != 0.0, e->forced_k != 0.0, e->sp_on);
    HIPCHK(e, hipGetLastError());
    return azk_sym_leaves(e, st);                                 // (eval symmetry: the leaves the tree launch selected, behind the movers)
}

int32_t azk_async_set_budget(azk_engine *e, int32_t n_sims, int32_t max_sims_per_launch, void *stream) {
    if (!e || !e->async_on || n_sims < 1 || n_sims > e->cfg.max_sims || max_sims_per_launch < 1) { if (e) e->err = "azk_async_set_budget: bad argument"; return AZK_ERR_ARG; }
    if (e->gb.m && n_sims != e->gumbel_sims) { e->err = "azk_async_set_budget: a Gumbel root is set - n_sims differs from the n_sims its halving table was built for"; return AZK_ERR_STATE; }
    e->budget_host[0] = n_sims; e->budget_host[1] = max_sims_per_launch;
    HIPCHK(e, hipMemcpyAsync(e->d.budget, e->budget_host, sizeof e->budget_host, hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_drain(azk_engine *e, float *states_dev, double *pis_dev, float *zs_dev, int64_t capacity, int64_t *cursor_dev, void *stream) {
    if (!e || !e->async_on) { if (e) e->err = "azk_async_drain: call azk_async_begin first"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(e, hipMemsetAsync(e->ad.fin_count, 0, sizeof(int), st));
    k_async_list<<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(d, e->ad);
    if (states_dev) {
        if (!pis_dev || !zs_dev || !cursor_dev || capacity < 1 || !d.traj_pi) { e->err = "azk_async_drain: bad replay arguments"; return AZK_ERR_ARG; }
        launch_emit(e, states_dev, pis_dev, zs_dev, (long long)capacity, (unsigned long long *)cursor_dev, nullptr, e->ad.fin_list, e->ad.fin_count, st);
    }
    with_flags([&](auto cap, auto open) {
        k_async_restart<cap.value, open.value><<<(unsigned)(d.G < 256 ? d.G : 256), AZK_WAVE, d.lds_bytes, st>>>(
            RestartPack<cap.value, open.value>{d, on<cap.value>(e->cp), on<open.value>(e->op)}, e->ad, e->async_recycle);
    }, e->cp.n_fast != 0, e->op_on);
    with_flags([&](auto cap) {
        // re-rooting engines: the next search of every game that moved since the last drain
        if (e->ru.mode) k_reroot_list<cap.value><<<(unsigned)d.G, AZK_WAVE, 0, st>>>(d, e->ad, CapPack<ReuseDev, cap.value>{e->ru, on<cap.value>(e->cp)});
    }, e->cp.n_fast != 0);
    if (e->ru.mode) HIPCHK(e, hipMemsetAsync(e->ad.reroot_count, 0, sizeof(int), st));
    if (e->ad.dirichlet) {                                        // the rows of the searches AFTER the ones begun since the last drain
        if (e->gb.m) k_gumbel_ahead<<<(unsigned)(d.G < 512 ? d.G : 512), AZK_WAVE, 0, st>>>(d, e->ad);
        else k_noise_ahead<<<(unsigned)(d.G < 512 ? d.G : 512), AZK_WAVE, 0, st>>>(d, e->ad);
        HIPCHK(e, hipMemsetAsync(e->ad.todo_count, 0, sizeof(int), st));
    }
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_emit_finished(azk_engine *e, float *states_dev, double *pis_dev, float *zs_dev, int64_t capacity,
                          int64_t *cursor_dev, int64_t *game_base_dev, void *stream) {
    if (!e || !states_dev || !pis_dev || !zs_dev || !cursor_dev || capacity < 1) return AZK_ERR_ARG;
    const Dev &d = e->d;
    if (!d.traj_pi) { e->err = "azk_emit_finished: (state, pi, z) emission needs a square board with one action per cell (or an engine created with emit_elements)"; return AZK_ERR_ARG; }
    launch_emit(e, states_dev, pis_dev, zs_dev, (long long)capacity, (unsigned long long *)cursor_dev, (long long *)game_base_dev, nullptr, nullptr, (hipStream_t)stream);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_emit_elements(const azk_engine *e, int32_t *mask_out, int32_t *group_out) {
    if (!e) return AZK_ERR_ARG;
    if (mask_out) *mask_out = e->cfg.emit_elements;
    if (group_out) *group_out = e->emit.n ? e->emit.n : (e->d.traj_pi ? 8 : 0);
    return AZK_OK;
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

int32_t azk_root_stats(azk_engine *e, double *pi_dev, double *q_dev, int32_t *root_visit_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    k_root_stats<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, pi_dev, q_dev, root_visit_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

// azk_advance and azk_advance_resign (move_index: the game coin's key, read on a resigning engine only)
static int32_t advance(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index, int32_t *chosen_cell_dev,
                       int32_t *winner_dev, int32_t *done_dev, void *stream) {
    const Dev &d = e->d;
    e->in_search = false;
    if (e->gb.m) {                                                // a Gumbel root: the Gumbel arg-max is the sample - no uniforms, no sample_until
        with_flags([&](auto resign) {
            Ply<resign.value> ply{0};
            if constexpr (resign.value) ply.move_index = move_index;
            k_advance<resign.value><<<d.G, AZK_WAVE, d.lds_bytes, (hipStream_t)stream>>>(
                GumbelPack<Dev, resign.value>{d, on<resign.value>(e->rs), on<true>(e->gb)}, ply, chosen_cell_dev, winner_dev, done_dev);
        }, e->rs.v_resign != 0.0);
        HIPCHK(e, hipGetLastError());
        return AZK_OK;
    }
    with_flags([&](auto cap, auto resign, auto forced, auto surprise) {
        Ply<resign.value || surprise.value> ply{sample_until_move};
        if constexpr (resign.value || surprise.value) ply.move_index = move_index;
        k_advance<cap.value, resign.value, forced.value, surprise.value><<<d.G, AZK_WAVE, d.lds_bytes, (hipStream_t)stream>>>(
            move_pack<cap.value, resign.value, forced.value, surprise.value>(d, e), uniforms_dev, ply, chosen_cell_dev, winner_dev, done_dev, e->ru.chosen_node);
    }, e->cp.n_fast != 0, e->rs.v_resign != 0.0, e->forced_k != 0.0, e->sp_on);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_advance(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t *chosen_cell_dev,
                    int32_t *winner_dev, int32_t *done_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->sp_on) { e->err = "azk_advance: surprise weighting is set - its moves are made by azk_advance_keyed (the ply coin needs the move index)"; return AZK_ERR_STATE; }
    if (e->rs.v_resign != 0.0) { e->err = "azk_advance: resignation is set - its moves are made by azk_advance_resign (the game coin needs the move index)"; return AZK_ERR_STATE; }
    return advance(e, uniforms_dev, sample_until_move, 0, chosen_cell_dev, winner_dev, done_dev, stream);
}

int32_t azk_advance_resign(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index, int32_t *chosen_cell_dev,
                           int32_t *winner_dev, int32_t *done_dev, void *stream) {
    if (!e || move_index < 0) { if (e) e->err = "azk_advance_resign: bad argument"; return AZK_ERR_ARG; }
    if (e->sp_on) { e->err = "azk_advance_resign: surprise weighting is set - its moves are made by azk_advance_keyed"; return AZK_ERR_STATE; }
    if (e->rs.v_resign == 0.0) { e->err = "azk_advance_resign: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    return advance(e, uniforms_dev, sample_until_move, move_index, chosen_cell_dev, winner_dev, done_dev, stream);
}

int32_t azk_advance_keyed(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index, int32_t *chosen_cell_dev,
                          int32_t *winner_dev, int32_t *done_dev, void *stream) {
    if (!e || move_index < 0) { if (e) e->err = "azk_advance_keyed: bad argument"; return AZK_ERR_ARG; }
    if (!e->sp_on) { e->err = "azk_advance_keyed: no surprise weighting is set (azk_set_surprise_weighting)"; return AZK_ERR_STATE; }
    return advance(e, uniforms_dev, sample_until_move, move_index, chosen_cell_dev, winner_dev, done_dev, stream);
}

int32_t azk_get_counters(azk_engine *e, azk_counters *out, void *stream) {
    if (!e || !out) return AZK_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    k_sum_counters<<<CNT_N, 256, 0, st>>>(e->d.counters, e->d.G, e->counter_sums);
    HIPCHK(e, hipGetLastError());
    long long h[CNT_N];
    HIPCHK(e, hipMemcpyAsync(h, e->counter_sums, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    memset(out, 0, sizeof *out);
    out->sims = h[CNT_SIMS]; out->edges_scanned = h[CNT_SCANNED]; out->trace_nodes = h[CNT_TRACE];
    out->edges_created = h[CNT_CREATED]; out->leaves_evaluated = h[CNT_LEAVES]; out->terminal_sims = h[CNT_TERMINAL];
    out->moves_played = h[CNT_MOVES]; out->cache_hits = h[CNT_CACHE_HITS];
    out->roots_reused = h[CNT_REUSED]; out->nodes_carried = h[CNT_CARRIED];
    out->forced_selections = h[CNT_FORCED]; out->visits_pruned = h[CNT_PRUNED]; out->visits_before_pruning = h[CNT_PRUNE_OF];
    return AZK_OK;
}

int32_t azk_gen_noise(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double alpha,
                      double *noise_dev, double *uniforms_dev, void *stream) {
    if (!e || alpha <= 0.0) return AZK_ERR_ARG;
    k_gen_noise<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(e->d.g.action_dim, seed, first_global_game, move_index, alpha,
                                                            noise_dev, uniforms_dev, (long long)e->d.g.action_dim);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

}  // extern "C"
