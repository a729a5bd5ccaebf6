// azk_tree.hip - the AlphaZero search step of the batched self-play engine for MI355X (gfx950): k_tree (all forty-two instantiations
// live in this one translation unit), its expanding wave, the leaf gather, and the C ABI calls that launch them (include/azk.h).
// One 64-lane wavefront owns one game (the plain k_tree gives it a helper wave); the tree is
// a structure-of-arrays arena in HBM whose child blocks are contiguous, so a PUCT scan is a coalesced read
// of the header records and the Q column (W / N, kept at backup: the walk divides nothing); per-wave scratch (board, path, move list, emulated CPython set) lives in LDS.
// Built with -ffp-contract=off: every float result is the same sequence of IEEE operations the oracle runs.
// Reference lines cited as file:line relative to the reference root.
#include "azk_engine_int.h"
#include <type_traits>

namespace {

typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // four consecutive floats of a row that is only 4-byte aligned (A = 225: 900-byte rows)

// Four consecutive floats of a row of A floats, one 16-byte access.  first = row_first(wanted, A): the lane at the row's end takes the
// row's last four (overlapping its neighbour).  Rows of fewer than four floats (boards of 1-3 cells) go component by component.
__device__ __forceinline__ int row_first(int wanted, int A) { return max(min(wanted, A - 4), 0); }
__device__ __forceinline__ f32x4_a4 row_load4(const float *row, int first, int A) {
    if (A >= 4) return *(const f32x4_a4 *)(row + first);
    f32x4_a4 v;
#pragma unroll
    for (int c = 0; c < 4; c++) v[c] = row[min(first + c, A - 1)];
    return v;
}
__device__ __forceinline__ void row_store4(float *row, int first, int A, f32x4_a4 v) {
    if (A >= 4) { *(f32x4_a4 *)(row + first) = v; return; }
#pragma unroll
    for (int c = 0; c < 4; c++) if (first + c < A) row[first + c] = v[c];
}

enum { HO_OK = 0, HO_FC, HO_NV, HO_ROOTF64, HO_END_LO, HO_END_HI };   // hand-off words (wave 1 -> wave 0); END: wave 1's clock at the barrier (DBG records)

// Wave 1 of a two-wave k_tree: mcts.py:46-60 for the leaf the previous launch selected, without Node.backup (wave 0's).  It reads the
// pending-leaf record (wave 0 rewrites it only behind the barrier), builds the leaf's move list from leaf_cells when the selection
// left none (leaf_nmoves = -1; a list left by a MULTI launch, >= 0, is taken from leaf_moves), and creates the children.  The
// arithmetic and its order are those of the one-wave expansion.  Always posts the hand-off words; the caller executes the barrier.
// Hook: the move generator's (empty) mid-way hook type.  The FORCED kernels pass one of their own, so that their wave 1 calls an instantiation of
// azk_valid_moves_gomoku of its own and the other kernels' copy keeps the callers - and with them the inlining order and the device code - it had.
struct TreeForcedHook { __device__ __forceinline__ void operator()() const {} };
// The GUMBEL kernels' hook type says more: their wave 1 writes a root's children as a Gumbel search wants them (gb, read under that type only) -
// rootP = the child's raw logit + the game's Gumbel draw for its action, the logit and the root's value kept in the GumbelDev block.
struct TreeGumbelHook { __device__ __forceinline__ void operator()() const {} };
// The SOLVER kernels' hook type: their wave 1 writes the status byte of every child it creates - and the root's, when it expands the root -
// as UNKNOWN (sv, read under that type only), whatever the arena slot held before.
struct TreeSolverHook { __device__ __forceinline__ void operator()() const {} };
template <bool DBG, int KSL, typename Hook = AzkNoHook>
__device__ __forceinline__ void tree_expand_wave(const Dev &d, const LdsView &L, const float *__restrict__ logits, const float *__restrict__ values, int ablate,
                                                 const GumbelDev &gb = GumbelDev{}, const SolverDev &sv = SolverDev{}) {
    constexpr bool GUMBEL = std::is_same_v<Hook, TreeGumbelHook>;
    constexpr bool SOLVER = std::is_same_v<Hook, TreeSolverHook>;
    const int g = blockIdx.x, vi = g * d.K, lane = azk_lane();        // (slot 0 of the game, as in wave 0)
    const GameDesc &gd = d.g;
    const int A = gd.action_dim, rc = gd.rc;
    const size_t base = (size_t)g * (size_t)d.cap;
    const bool shared = d.cache_entries && d.cache_shared;
    const bool wrec = DBG && (ablate & 8192) != 0;
    // first round trip: the record's words (lane k fetches word k), the leaf's key and its cells
    const int *up = d.leaf_node + vi;
    up = lane == 1 ? d.leaf_slot + vi : up;
    up = lane == 2 ? d.leaf_depth + vi : up;
    up = lane == 3 ? d.leaf_nmoves + vi : up;
    up = lane == 4 ? d.arena_top + g : up;
    up = (lane == 5 && d.cache_entries) ? d.leaf_cache + vi : up;
    up = (lane == 6 && shared) ? (const int *)d.cache_stamp : up;
    const int uw = *up;
    unsigned long long e_key = 0ull;
    if (shared) e_key = d.leaf_key[(size_t)vi * d.key_words + min(lane, d.key_words - 1)];
    constexpr int NCW = (KSL * AZK_WAVE / 4 + AZK_WAVE - 1) / AZK_WAVE;
    const int ncw = d.rc_pad >> 2;
    uint32_t cw[NCW];
    {
        const uint32_t *lw = (const uint32_t *)(d.leaf_cells + (size_t)vi * d.rc_pad);
#pragma unroll
        for (int q = 0; q < NCW; q++) cw[q] = lw[min(lane + AZK_WAVE * q, ncw - 1)];
    }
    const int node = __builtin_amdgcn_readlane(uw, 0);
    int ok = 0, fc = -1, nv = 0, rootf64 = 0;
    if (node >= 0) {
        const bool xst = (ablate & 1024) != 0;                  // debug only: cycle stamps of the expansion's sub-phases
        long long x0 = 0, x1 = 0, x2 = 0, x3 = 0, x4 = 0;
        if (xst) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); x0 = clock64(); }
        const int slot = __builtin_amdgcn_readlane(uw, 1);
        const int depth = __builtin_amdgcn_readlane(uw, 2);
        nv = __builtin_amdgcn_readlane(uw, 3);
        const int centry = d.cache_entries ? __builtin_amdgcn_readlane(uw, 5) : -1;
        const unsigned cstamp = shared ? (unsigned)__builtin_amdgcn_readlane(uw, 6) : 0u;
        const bool hit = d.cache_entries && centry >= 0;
        const size_t crow = shared ? (size_t)(hit ? centry : -(centry + 1)) : ((size_t)g * d.cache_entries + (hit ? centry : -(centry + 1)));
        const float *lg = hit ? (shared ? d.hit_logits + (size_t)vi * A : d.cache_logits + crow * A) : logits + (size_t)slot * A;
        unsigned claim_now = 0u;
        if (shared && !hit) claim_now = __hip_atomic_load(d.cache_claim + crow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        // second round trip, issued before the move list is built and landing under it: logits (a lane takes FOUR consecutive ones per
        // load: actions 4 lane .. 4 lane + 3 of each block of 256), value, the node's header; a list left in leaf_moves comes along
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
#pragma unroll
        for (int q = 0; q < NCW; q++) { const int i = lane + AZK_WAVE * q; if (i < ncw) ((uint32_t *)L.board1)[i] = cw[q]; }
        if (nv >= 0) {
            for (int i = lane; i < nv; i += AZK_WAVE) L.moves[i] = d.leaf_moves[(size_t)vi * rc + i];
        }
        azk_wave_sync();
        if (nv < 0) {                                                 // mcts.py:34, moved from the selection to the expansion
            if (ablate & 4) { nv = 1; if (lane == 0) L.moves[0] = (int16_t)(gd.rc / 2); azk_wave_sync(); }
            else if (gd.kind == AZK_KIND_GOMOKU)
                nv = azk_valid_moves_gomoku<KSL, Hook>(L.board1, gd, L.moves, L.ms, (ablate & 8) != 0, (ablate & 32) ? d.dbg + (size_t)g * 8 : nullptr);
            else nv = azk_valid_moves_small(L.board1, gd, L.moves);
        }
        nv = uniform_i32(nv);
        int e_mv[KSL];
#pragma unroll
        for (int k4 = 0; k4 < KSL; k4++) { const int i = lane + AZK_WAVE * k4; e_mv[k4] = L.moves[i < nv ? i : 0]; }
        const bool mix = depth == 0 && d.noise != nullptr;        // mcts.py:42-43,52-53
        double nzv[KSL] = {};
        if (mix) {
#pragma unroll
            for (int k4 = 0; k4 < KSL; k4++) nzv[k4] = d.noise[(size_t)g * A + azk_action_idx(gd, e_mv[k4])];
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
            // (behind the exponentials: by now every logit is in its register, and the stores go out back to back)
#pragma unroll
            for (int q = 0; q < NV4; q++) if (lact[q]) row_store4(d.cache_logits + crow * A, la[q], A, lgv[q]);
            if (lane == 0) d.cache_value[crow] = vraw;
        }
        if (xst) x2 = clock64();
        const float s = azk_pairwise_sum(L.e, A);
        if (xst) x3 = clock64();
        fc = __builtin_amdgcn_readlane(uw, 4);
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
                d.H[idx] = NodeH{0, p, meta_pack(cell, 0), -1}; d.W[idx] = 0.0;       // (N = 0: Q[idx] stays unwritten - unspecified until the first backup)
                if constexpr (SOLVER) sv.status[idx] = (uint8_t)SOLVER_UNKNOWN;       // a new node is UNKNOWN whatever the slot held (idx < base + cap: `fits`)
                if constexpr (GUMBEL) {                               // the child's base score: its raw logit + the game's Gumbel draw for its action
                    if (mix) { const float lga = lg[a]; d.rootP[(size_t)g * rc + i] = (double)lga + nzv[k4]; gb.logit[(size_t)g * rc + i] = lga; }
                } else
                if (mix) d.rootP[(size_t)g * rc + i] = (double)(0.75f * p) + 0.25 * nzv[k4];   // utils.py:24-25
            }
            if constexpr (GUMBEL) { if (mix && lane == 0) gb.v0[g] = vraw; }
            if constexpr (SOLVER) { if (depth == 0 && lane == 0) sv.status[base + node] = (uint8_t)SOLVER_UNKNOWN; }   // the root becomes UNKNOWN when it is expanded
            if (lane == 0) {
                d.H[base + node].fc = fc;
                d.H[base + node].meta = (node_meta & 0xffff0000u) | (uint32_t)nv;
                d.arena_top[g] = fc + nv;
                if (depth == 0) d.root_f64[g] = mix ? 1 : 0;
                count_add(d, CNT_CREATED, g, nv);
            }
            ok = 1; rootf64 = mix ? 1 : 0;
        } else if (lane == 0) {
            atomicExch(d.err, AZK_ERR_ARENA_FULL);
        }
        if (xst && lane == 0) {
            x4 = clock64();
            long long *qq = d.dbg + (size_t)g * 8;
            qq[1] += x1 - x0; qq[2] += x2 - x1; qq[3] += x3 - x2; qq[4] += x4 - x3; qq[6] += 1;
        }
    }
    if (wrec) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the record's clock: behind the last store, like the barrier)
    if (lane == 0) {
        L.ho[HO_OK] = ok; L.ho[HO_FC] = fc; L.ho[HO_NV] = nv; L.ho[HO_ROOTF64] = rootf64;
        if (wrec) { const unsigned long long te = (unsigned long long)clock64(); L.ho[HO_END_LO] = (int)(unsigned)te; L.ho[HO_END_HI] = (int)(unsigned)(te >> 32); }
    }
}

// ================================================================================================
// k_tree<EXPAND, SELECT>: one simulation step for every game.
//   EXPAND: mcts.py:46-60 for the leaf selected by the previous step (softmax, noise, expand, backup)
//   SELECT: mcts.py:18-37 (PUCT walk, terminal test + backup, valid moves, leaf hand-off)
// ================================================================================================
// DBG: the AZK_TREE_ABLATE experiments and cycle stamps exist only in the <.., true> instantiation; the product kernel
// (DBG = false) carries none of their branches.
// MULTI: a game keeps simulating inside the launch for as long as its simulations need no evaluator - a terminal leaf is backed
// up at once (mcts.py:25-32) and a leaf served by the eval cache is expanded from the cached row (mcts.py:38-44) - and stops at
// the first leaf that misses the cache (one pending evaluation per game, as before), at its simulation budget, or after
// budget[1] simulations.  The order of a game's simulations is untouched (they are sequential inside one wave), so every tree
// is bit-identical to one-simulation-per-launch stepping; what changes is that ~55 % of the simulations no longer wait for a
// kernel boundary and every launch hands the evaluator a (nearly) full batch.
// KSL: cells (and actions) per lane the kernel is compiled for - 4 covers boards of up to 256 cells (every shipped game), 7 the rest
// (make_game allows 400).  A compile-time bound: the per-lane load sequences, their registers and the move generator's cell groups are
// unrolled to it, and a 15 x 15 board does not pay for three empty groups in each of them.
//
// TWO WAVES PER GAME (every instantiation with MULTI = false; the MULTI ones stay one wave and build the move list at the leaf):
//   wave 0  the game's critical chain: entry loads, Node.backup of the previous leaf along its path (path, depth and value only), the
//           walk, the terminal test, the eval-cache probe and the leaf's record.  It builds no move list: leaf_nmoves = -1 means
//           "build it from leaf_cells at expansion".
//   wave 1  everything else about the previous leaf, beside wave 0's memory round trips: its move list (from leaf_cells, on a board and
//           scratch of its own), softmax, eval-cache write, root noise, the children, the node's fc / child count, arena_top, root_f64.
// The hand-off is ONE s_barrier, executed exactly once by each wave on every path (idle or finished game, no pending leaf, terminal
// leaf, full arena): wave 1 behind its last store (vmcnt(0)) and the hand-off words in LDS; wave 0 when its walk arrives at the
// previous leaf's node - whose fc and child count it then takes from the hand-off words, never from the header its parent's scan brought
// along - or, if the walk goes elsewhere, before the first store to the pending-leaf record that wave 1 reads (leaf_cells, leaf_cache,
// leaf_key, hit_logits ...), at the latest before it ends.  Both waves share a CU and its L1: workgroup scope is enough.  Nothing
// waits on memory.

//
// FORCED (forced playouts, azk_set_forced_playouts): the float64 root scan - and only it, in all three of its forms - sets a
// child's score to +inf while  N >= 1  and  (double)N * (double)N < (k * P) * (double)(Np - 1):  a compare and a select on u, nothing else
// of the scan moves, "first maximum wins" picks the first forced child in list order.  fd.k is folded to 0 for a fast search of a capped
// engine (search_full, read once per wave), which makes the comparison false for every child.  Wave 1 never sees any of it.
// the rule, in one place: the score of a root child with N visits and mixed prior P under a root of Np visits (u: its PUCT score)
template <bool FORCED>
__device__ __forceinline__ double tree_forced_score(double u, int N, double P, double fk, int Np) {
    if constexpr (FORCED) return ((N != 0) & ((double)N * (double)N < (fk * P) * (double)(Np - 1))) ? __builtin_huge_val() : u;
    else return u;
}

// GUMBEL (Gumbel root search, azk_set_gumbel_root): the float64 root scan - and only it, in all three of its forms - scores
// a child  gl + sig * (W / N)  (gl alone while N = 0) if its visit count N equals cv, the sequential-halving table's word for this root
// selection, and -inf otherwise; gl = rootP (raw logit + Gumbel draw, written at the root's expansion), sig = (c_visit + cv) * c_scale.  "First
// maximum wins" stays.  The table guarantees an eligible child at every selection; were there none, the first child would be taken.
template <bool GUMBEL>
__device__ __forceinline__ double tree_gumbel_score(double u, int N, double q, double gl, int cv, double sig) {
    if constexpr (GUMBEL) return N == cv ? (N != 0 ? gl + sig * q : gl) : -__builtin_huge_val();
    else return u;
}

// PUCT (configurable PUCT, azk_set_puct): every scan of the walk - all three forms, both precision paths - multiplies the
// exploration term's sqrt(Np) by c = c_table[min(Np, n_table - 1)] and scores an unvisited child  qf + u0  instead of u0 (fpu_mode 1: qf = f;
// mode 2: qf = -(Wn / Np) - f * sqrt(vm), Wn the selecting node's value sum, vm the prior mass of its visited children; f = fpu_root at the
// root, fpu_tree below it).  The table word goes out with the children's loads; the chosen child's W comes down beside its N, meta and fc;
// the mass is summed in mode 2 only.  Wave 1 never sees any of it.  The factor c and the unvisited child's score are plain statements under
// `if constexpr (PUCT)` in the body, not helper templates like the two above: a call inside the scan's arithmetic, even one that folds to
// its argument, reaches the optimiser as other IR and the 28 kernels without the option came out different (tools/compare_kernel_isa.py).
// What only the PUCT kernels call is below.
struct TreePuctHook { __device__ __forceinline__ void operator()() const {} };     // (wave 1's move generator: a copy of the PUCT kernels' own)
// the wave's sum of the lanes' partial masses by the xor butterfly 32, 16, 8, 4, 2, 1 (x = x + partner; every lane ends with the sum).  Behind
// the steps 32 and 16 the lanes of one index modulo 16 hold the same bits, behind step 8 those of one index modulo 8, so the partner of the last
// four steps is reached inside the lane's row of 16: row_ror:8 is lane ^ 8, row_ror:4 brings a lane of the class (lane ^ 4) mod 8, and the
// quad permutes are lane ^ 2 and lane ^ 1 - four DPP adds instead of four more trips through the LDS crossbar.
template <typename T>
__device__ __forceinline__ T tree_puct_mass(T part) {
    part = part + __shfl_xor(part, 32);
    part = part + __shfl_xor(part, 16);
    part = part + dpp_val<0x128>(part);                           // row_ror:8
    part = part + dpp_val<0x124>(part);                           // row_ror:4
    part = part + dpp_val<0x4E>(part);                            // quad_perm [2,3,0,1]
    part = part + dpp_val<0xB1>(part);                            // quad_perm [1,0,3,2]
    return part;
}
// mode 2: the selecting node's value for the side that chooses (Node.backup keeps it as the player who moved INTO the node sees it), less the reduction
__device__ __forceinline__ double tree_puct_qf2(double f, double Wn, int Np, double vm) {
    const double qn = -(Wn / (double)Np);
    return qn - f * sqrt(vm);
}
__device__ __forceinline__ double tree_readlane_f64(double v, int lane) {
    return __builtin_bit_cast(double, azk_readlane_u64(__builtin_bit_cast(unsigned long long, v), lane));
}

// The kernels.  The fourteen instantiations without FORCED keep the name, the arguments and the device code they had before the option
// existed (tools/compare_kernel_isa.py); the six with it - fused, select-only and MULTI, each at KSL 4 and 7 - take the extra argument block,
// and so do the eight with GUMBEL (theirs is the GumbelDev block).
template <bool EXPAND, bool SELECT, bool DBG, bool MULTI = false, int KSL = 7>
__global__ __launch_bounds__(MULTI ? AZK_WAVE : 2 * AZK_WAVE) void k_tree(Dev dd, const float *__restrict__ logits, const float *__restrict__ values) {
    constexpr bool FORCED = false;
    constexpr bool GUMBEL = false;
    constexpr bool PUCT = false;
#define AZK_TREE_FORCED_ARG ForcedDev{}
#define AZK_TREE_GUMBEL_ARG GumbelDev{}
#define AZK_TREE_PUCT_ARG PuctDev{}
    constexpr bool SOLVER = false;
#define AZK_TREE_SOLVER_ARG SolverDev{}
#include "azk_tree_step.h"
#undef AZK_TREE_SOLVER_ARG
#undef AZK_TREE_PUCT_ARG
#undef AZK_TREE_GUMBEL_ARG
#undef AZK_TREE_FORCED_ARG
}

template <bool EXPAND, bool SELECT, bool DBG, bool MULTI, int KSL, bool FORCED>
__global__ __launch_bounds__(MULTI ? AZK_WAVE : 2 * AZK_WAVE) void k_tree(Dev dd, const float *__restrict__ logits, const float *__restrict__ values, ForcedDev fd_arg) {
    static_assert(FORCED && SELECT && !DBG, "FORCED exists for the product kernels that select");
    constexpr bool GUMBEL = false;
    constexpr bool PUCT = false;
#define AZK_TREE_FORCED_ARG fd_arg
#define AZK_TREE_GUMBEL_ARG GumbelDev{}
#define AZK_TREE_PUCT_ARG PuctDev{}
    constexpr bool SOLVER = false;
#define AZK_TREE_SOLVER_ARG SolverDev{}
#include "azk_tree_step.h"
#undef AZK_TREE_SOLVER_ARG
#undef AZK_TREE_PUCT_ARG
#undef AZK_TREE_GUMBEL_ARG
#undef AZK_TREE_FORCED_ARG
}

// the eight GUMBEL kernels: fused, select-only, expand-only (the root's expansion writes rootP its own way) and MULTI, each at KSL 4 and 7
template <bool EXPAND, bool SELECT, bool DBG, bool MULTI, int KSL, bool FORCED, bool GUMBEL>
__global__ __launch_bounds__(MULTI ? AZK_WAVE : 2 * AZK_WAVE) void k_tree(Dev dd, const float *__restrict__ logits, const float *__restrict__ values, GumbelDev gb_arg) {
    static_assert(GUMBEL && !FORCED && !DBG, "GUMBEL exists for the product kernels, without forced playouts");
    constexpr bool PUCT = false;
#define AZK_TREE_FORCED_ARG ForcedDev{}
#define AZK_TREE_GUMBEL_ARG gb_arg
#define AZK_TREE_PUCT_ARG PuctDev{}
    constexpr bool SOLVER = false;
#define AZK_TREE_SOLVER_ARG SolverDev{}
#include "azk_tree_step.h"
#undef AZK_TREE_SOLVER_ARG
#undef AZK_TREE_PUCT_ARG
#undef AZK_TREE_GUMBEL_ARG
#undef AZK_TREE_FORCED_ARG
}

// the six PUCT kernels: fused, select-only and MULTI, each at KSL 4 and 7 (an expand-only launch selects nothing: the plain kernel)
template <bool EXPAND, bool SELECT, bool DBG, bool MULTI, int KSL, bool FORCED, bool GUMBEL, bool PUCT>
__global__ __launch_bounds__(MULTI ? AZK_WAVE : 2 * AZK_WAVE) void k_tree(Dev dd, const float *__restrict__ logits, const float *__restrict__ values, PuctDev pu_arg) {
    static_assert(PUCT && !FORCED && !GUMBEL && SELECT && !DBG, "PUCT exists for the product kernels that select, without forced playouts or a Gumbel root");
#define AZK_TREE_FORCED_ARG ForcedDev{}
#define AZK_TREE_GUMBEL_ARG GumbelDev{}
#define AZK_TREE_PUCT_ARG pu_arg
    constexpr bool SOLVER = false;
#define AZK_TREE_SOLVER_ARG SolverDev{}
#include "azk_tree_step.h"
#undef AZK_TREE_SOLVER_ARG
#undef AZK_TREE_PUCT_ARG
#undef AZK_TREE_GUMBEL_ARG
#undef AZK_TREE_FORCED_ARG
}

// the eight SOLVER kernels: fused, select-only, expand-only (expansion writes the new nodes' UNKNOWN bytes) and MULTI, each at KSL 4 and 7
template <bool EXPAND, bool SELECT, bool DBG, bool MULTI, int KSL, bool FORCED, bool GUMBEL, bool PUCT, bool SOLVER>
__global__ __launch_bounds__(MULTI ? AZK_WAVE : 2 * AZK_WAVE) void k_tree(Dev dd, const float *__restrict__ logits, const float *__restrict__ values, SolverDev sv_arg) {
    static_assert(SOLVER && !FORCED && !GUMBEL && !PUCT && !DBG, "SOLVER exists for the product kernels, without forced playouts, a Gumbel root or configurable PUCT");
#define AZK_TREE_FORCED_ARG ForcedDev{}
#define AZK_TREE_GUMBEL_ARG GumbelDev{}
#define AZK_TREE_PUCT_ARG PuctDev{}
#define AZK_TREE_SOLVER_ARG sv_arg
#include "azk_tree_step.h"
#undef AZK_TREE_SOLVER_ARG
#undef AZK_TREE_PUCT_ARG
#undef AZK_TREE_GUMBEL_ARG
#undef AZK_TREE_FORCED_ARG
}

// Leaf compaction: slot = number of leaf games with a lower index (deterministic order); writes the
// canonical board (gomoku.py:34-40; 3-plane: mcts.py:126-137) of each leaf into the evaluator batch.
__global__ __launch_bounds__(AZK_WAVE) void k_gather(Dev d, void *__restrict__ leaf_boards, int *__restrict__ n_leaf_out) {
    const int g = blockIdx.x, lane = azk_lane();          // g = slot index over the G * K pending-leaf slots
    const int NV = d.G * d.K;
    // prefix over byte flags, 8 flags per lane per load (leaf_flag is padded to a multiple of 512 bytes)
    int before = 0, total = 0;
    const unsigned long long *fw = (const unsigned long long *)d.leaf_flag;
    const int nw = (NV + 7) >> 3;
    const bool last = g == NV - 1;
    const int limit_words = last ? nw : ((g + 8) >> 3);
    for (int w0 = 0; w0 < limit_words; w0 += AZK_WAVE) {
        int w = w0 + lane;
        unsigned long long x = w < nw ? fw[w] : 0ull;
        x = (((x & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | x) & 0x8080808080808080ull;   // one bit per non-zero flag byte (a flag carries its leaf's cost class)
        total += __popcll(x);
        // flags strictly before game g
        int lo = w * 8;
        if (lo + 8 <= g) before += __popcll(x);
        else if (lo < g) before += __popcll(x & ((1ull << ((g - lo) * 8)) - 1ull));
    }
    before = wave_sum_i32(before);
    if (last) {
        total = wave_sum_i32(total);
        if (lane == 0) {
            *n_leaf_out = total;
            if (d.cache_entries && d.cache_shared) d.cache_stamp[0] += 1u;   // the next tree launch may read what the last one cached
        }
    }
    if (!d.leaf_flag[g]) return;
    const int slot = before;
    if (lane == 0) d.leaf_slot[g] = slot;
    const int rc = d.g.rc, F = d.g.planes;
    const int player = (d.to_move[g / d.K] + d.leaf_depth[g]) & 1;     // node.currentPlayer
    const uint8_t *b = d.leaf_cells + (size_t)g * d.rc_pad;
    const size_t o = (size_t)slot * F * rc;
    for (int i = lane; i < F * rc; i += AZK_WAVE) {
        const int plane = i / rc, c = i - plane * rc;
        float v;
        if (plane == 2) v = (float)player;                            // side-to-move plane (tictactoe.py:41)
        else v = (float)((b[c] >> (plane ^ player)) & 1);             // own stones first for player 1
        if (d.leaf_dtype == AZK_LEAF_BF16) ((__hip_bfloat16 *)leaf_boards)[o + i] = __float2bfloat16(v);
        else ((float *)leaf_boards)[o + i] = v;
    }
}

}  // namespace

// launch: the instantiation compiled for this engine's cells-per-lane bound
template <bool E, bool S, bool D, bool M>
static void launch_k_tree(const Dev &d, const float *logits, const float *values, hipStream_t st) {
    const int nthr = M ? AZK_WAVE : 2 * AZK_WAVE;                     // plain kernels: two waves per game
    if (d.g.rc <= 4 * AZK_WAVE && d.g.action_dim <= 4 * AZK_WAVE) k_tree<E, S, D, M, 4><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values);
    else k_tree<E, S, D, M, 7><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values);
}
template <bool E, bool M>                                             // forced playouts: the selecting product kernels
static void launch_k_tree_forced(const Dev &d, const float *logits, const float *values, const ForcedDev &fd, hipStream_t st) {
    const int nthr = M ? AZK_WAVE : 2 * AZK_WAVE;
    if (d.g.rc <= 4 * AZK_WAVE && d.g.action_dim <= 4 * AZK_WAVE) k_tree<E, true, false, M, 4, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, fd);
    else k_tree<E, true, false, M, 7, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, fd);
}

template <bool E, bool S, bool M>                                     // Gumbel root search: the product kernels
static void launch_k_tree_gumbel(const Dev &d, const float *logits, const float *values, const GumbelDev &gb, hipStream_t st) {
    const int nthr = M ? AZK_WAVE : 2 * AZK_WAVE;
    if (d.g.rc <= 4 * AZK_WAVE && d.g.action_dim <= 4 * AZK_WAVE) k_tree<E, S, false, M, 4, false, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, gb);
    else k_tree<E, S, false, M, 7, false, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, gb);
}

template <bool E, bool M>                                             // configurable PUCT: the selecting product kernels
static void launch_k_tree_puct(const Dev &d, const float *logits, const float *values, const PuctDev &pu, hipStream_t st) {
    const int nthr = M ? AZK_WAVE : 2 * AZK_WAVE;
    if (d.g.rc <= 4 * AZK_WAVE && d.g.action_dim <= 4 * AZK_WAVE) k_tree<E, true, false, M, 4, false, false, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, pu);
    else k_tree<E, true, false, M, 7, false, false, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, pu);
}

template <bool E, bool S, bool M>                                     // exact game-end proofs: the product kernels
static void launch_k_tree_solver(const Dev &d, const float *logits, const float *values, const SolverDev &sv, hipStream_t st) {
    const int nthr = M ? AZK_WAVE : 2 * AZK_WAVE;
    if (d.g.rc <= 4 * AZK_WAVE && d.g.action_dim <= 4 * AZK_WAVE) k_tree<E, S, false, M, 4, false, false, false, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, sv);
    else k_tree<E, S, false, M, 7, false, false, false, true><<<d.G, nthr, d.lds_bytes, st>>>(d, logits, values, sv);
}

// The one place that picks a k_tree instantiation: seven (EXPAND, SELECT, DBG, MULTI) forms, three FORCED ones, four GUMBEL ones, three PUCT ones and four
// SOLVER ones, each at KSL 4 and 7.
//   multi   the caller wants budget stepping.  The lock-step entry points pass `e->multi && !d.ablate` - an ablation build
//           (AZK_TREE_ABLATE) never runs MULTI from them; azk_async_step passes true and has never looked at the ablation word.
//           MULTI exists only with SELECT: budget stepping with `select` always launches <true, true, false, true>, whatever
//           `expand` says - a leaf served by the cache is expanded inside the launch (logits may be null when no game has a pending
//           evaluation, e.g. in a search's first launch) - and an expand-only launch is the plain kernel.
//   DBG     chosen from d.ablate.
//   FORCED  an engine with forced playouts set (e->forced_k != 0) launches the FORCED sibling of whichever product kernel selects; its
//           expand-only launches and an ablation build's DBG kernels are the plain ones (no selection / debug only).
//   GUMBEL  an engine with a Gumbel root set (e->gb.m != 0; never together with FORCED) launches the GUMBEL sibling of every product kernel,
//           the expand-only one included; an ablation build's DBG kernels are the plain ones.
//   PUCT    an engine with configurable PUCT set (e->puct_on; never together with FORCED or GUMBEL) launches the PUCT sibling of whichever
//           product kernel selects; its expand-only launches and an ablation build's DBG kernels are the plain ones.
//   SOLVER  an engine with the solver set (e->sv_on; never together with FORCED, GUMBEL or PUCT) launches the SOLVER sibling of every product
//           kernel, the expand-only one included (expansion writes the new nodes' status bytes); an ablation build's DBG kernels are the plain ones.
//   symmetry an engine with azk_set_eval_symmetry on expands from ITS copy of the rows, turned back into each position's frame by
//           k_sym_logits in front of the launch (the kernel is the same, it is handed another pointer); the callers run azk_sym_leaves
//           behind a launch that selects.
int32_t azk_launch_tree(azk_engine *e, bool expand, bool select, bool multi, const float *logits, const float *values, hipStream_t st) {
    const Dev &d = e->d;
    if (expand || (multi && select)) logits = azk_sym_restore(e, logits, st);
    const bool forced = e->forced_k != 0.0 && select && (multi || !d.ablate);
    const bool gumbel = e->gb.m != 0 && (multi || !d.ablate);
    const bool puct = e->puct_on && select && (multi || !d.ablate);
    const bool solver = e->sv_on && (multi || !d.ablate);
    if (gumbel && multi && select) launch_k_tree_gumbel<true, true, true>(d, logits, values, e->gb, st);
    else if (gumbel && expand && select) launch_k_tree_gumbel<true, true, false>(d, logits, values, e->gb, st);
    else if (gumbel && expand) launch_k_tree_gumbel<true, false, false>(d, logits, values, e->gb, st);
    else if (gumbel) launch_k_tree_gumbel<false, true, false>(d, logits, values, e->gb, st);
    else if (forced && multi) launch_k_tree_forced<true, true>(d, logits, values, e->forced(), st);
    else if (forced && expand) launch_k_tree_forced<true, false>(d, logits, values, e->forced(), st);
    else if (forced) launch_k_tree_forced<false, false>(d, logits, values, e->forced(), st);
    else if (puct && multi) launch_k_tree_puct<true, true>(d, logits, values, e->pu, st);
    else if (puct && expand) launch_k_tree_puct<true, false>(d, logits, values, e->pu, st);
    else if (puct) launch_k_tree_puct<false, false>(d, logits, values, e->pu, st);
    else if (solver && multi && select) launch_k_tree_solver<true, true, true>(d, logits, values, e->sv, st);
    else if (solver && expand && select) launch_k_tree_solver<true, true, false>(d, logits, values, e->sv, st);
    else if (solver && expand) launch_k_tree_solver<true, false, false>(d, logits, values, e->sv, st);
    else if (solver) launch_k_tree_solver<false, true, false>(d, logits, values, e->sv, st);
    else if (multi && select) launch_k_tree<true, true, false, true>(d, logits, values, st);
    else if (d.ablate) {
        if (expand && select) launch_k_tree<true, true, true, false>(d, logits, values, st);
        else if (expand) launch_k_tree<true, false, true, false>(d, logits, values, st);
        else launch_k_tree<false, true, true, false>(d, logits, values, st);
    } else if (expand && select) launch_k_tree<true, true, false, false>(d, logits, values, st);
    else if (expand) launch_k_tree<true, false, false, false>(d, logits, values, st);
    else launch_k_tree<false, true, false, false>(d, logits, values, st);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

extern "C" {

namespace {      // (inside extern "C": the kernel's symbol is the plain `k_unfinished`, as it has always been)
__global__ void k_unfinished(Dev d, int *out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    bool open = g < d.G && d.done[g] == 0 && d.sims_done[g] < d.budget[0];
    if (g < d.G && d.done[g] == 0)
        for (int k = 0; k < d.K; k++)        // a leaf awaiting the evaluator; with K > 1 also one served by the cache (only a tree launch expands it)
            open = open || (d.leaf_node[g * d.K + k] >= 0 && (d.leaf_flag[g * d.K + k] || d.K > 1));
    const unsigned long long m = __ballot(open);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(out, __popcll(m));
}
}  // namespace

int32_t azk_search_unfinished(azk_engine *e, int32_t *count_host, void *stream) {
    if (!e || !count_host) return AZK_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(e, hipMemsetAsync(e->n_leaf_scratch, 0, sizeof(int), st));
    k_unfinished<<<(unsigned)((e->d.G + 255) / 256), 256, 0, st>>>(e->d, e->n_leaf_scratch);
    HIPCHK(e, hipMemcpyAsync(count_host, e->n_leaf_scratch, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return AZK_OK;
}

// what k_gather is handed: the engine's view - under azk_set_eval_symmetry a host-side copy of it whose leaf_cells are the turned ones
static Dev gather_view(const azk_engine *e) {
    Dev d = e->d;
    if (e->sym.mode) d.leaf_cells = e->sym.sym_cells;
    return d;
}

static int32_t launch_tree(azk_engine *e, bool expand, bool select, const float *logits, const float *values,
                           void *leaf_boards, int32_t *n_leaf, hipStream_t st) {
    const Dev &d = e->d;
    if (expand && (!logits || !values)) { e->err = "expand needs logits_dev and values_dev"; return AZK_ERR_ARG; }
    if (select && (!leaf_boards || !n_leaf)) { e->err = "select needs leaf_boards_dev and n_leaf_dev"; return AZK_ERR_ARG; }
    const int32_t rc = azk_launch_tree(e, expand, select, e->multi && !d.ablate, logits, values, st);
    if (rc != AZK_OK) return rc;
    if (select) {
        const int32_t rs = azk_sym_leaves(e, st);
        if (rs != AZK_OK) return rs;
        k_gather<<<d.G * d.K, AZK_WAVE, 0, st>>>(gather_view(e), leaf_boards, n_leaf);
        HIPCHK(e, hipGetLastError());
    }
    return AZK_OK;
}

int32_t azk_step_select(azk_engine *e, void *leaf_boards_dev, int32_t *n_leaf_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    return launch_tree(e, false, true, nullptr, nullptr, leaf_boards_dev, n_leaf_dev, (hipStream_t)stream);
}

int32_t azk_step_expand_backup(azk_engine *e, const float *logits_dev, const float *values_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    return launch_tree(e, true, false, logits_dev, values_dev, nullptr, nullptr, (hipStream_t)stream);
}

int32_t azk_step(azk_engine *e, const float *logits_dev, const float *values_dev, void *leaf_boards_dev,
                 int32_t *n_leaf_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    return launch_tree(e, logits_dev != nullptr, true, logits_dev, values_dev, leaf_boards_dev, n_leaf_dev, (hipStream_t)stream);
}

int32_t azk_step_tree(azk_engine *e, const float *logits_dev, const float *values_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (logits_dev && !values_dev) { e->err = "values_dev missing"; return AZK_ERR_ARG; }
    // null logits: a select-only launch (no gather, no evaluator outputs)
    const int32_t rc = azk_launch_tree(e, logits_dev != nullptr, true, e->multi && !e->d.ablate, logits_dev, logits_dev ? values_dev : nullptr, (hipStream_t)stream);
    return rc != AZK_OK ? rc : azk_sym_leaves(e, (hipStream_t)stream);
}

int32_t azk_step_gather(azk_engine *e, void *leaf_boards_dev, int32_t *n_leaf_dev, void *stream) {
    if (!e || !leaf_boards_dev || !n_leaf_dev) return AZK_ERR_ARG;
    k_gather<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(gather_view(e), leaf_boards_dev, n_leaf_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_leaf_source_of(azk_engine *e, int32_t *n_leaf_dev, azk_leaf_source *out) {
    if (!e || !n_leaf_dev || !out) return AZK_ERR_ARG;
    const Dev &d = e->d;
    out->leaf_flag = d.leaf_flag; out->leaf_cells = e->sym.mode ? e->sym.sym_cells : d.leaf_cells; out->to_move = d.K > 1 ? d.to_move_v : d.to_move; out->leaf_depth = d.leaf_depth;
    out->leaf_slot = d.leaf_slot; out->n_leaf = n_leaf_dev;
    out->n_games = d.G * d.K; out->rows = d.g.rows; out->cols = d.g.cols; out->rc = d.g.rc; out->rc_pad = d.rc_pad; out->planes = d.g.planes;
    out->flag_bytes = ((d.G * d.K + 511) / 512) * 512 + 512;
    out->cache_stamp = (d.cache_entries && d.cache_shared) ? d.cache_stamp : nullptr;
    return AZK_OK;
}

}  // extern "C"
