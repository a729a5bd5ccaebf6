// azk_engine_int.h - what more than one engine file needs (azk_tree.hip, azk_vanilla.hip, azk_rules.hip, azk_begin.hip, azk_moves.hip,
// azk_emit.hip, azk_noise.hip and the kernel-free azk_engine.hip and azk_options.hip): the device view of the engine
// and its LDS layout, the node-record helpers, the host struct behind the opaque azk_engine, and the few host symbols that cross files.
// Not part of the ABI (include/azk.h).  A __device__ function is here only if kernels of two files call it.
// The shared types and helpers live in namespace azk_eng, which every file that includes this header uses: struct azk_engine, a global
// type whose members are of those types and whose pointers cross files (azk_launch_tree, azk_init_games), is then ONE type in every
// translation unit.  The kernels themselves stay in each .hip file's unnamed namespace.  tools/compare_kernel_isa.py --strip-namespace
// azk_eng compares such a build with one from before the namespace had a name (Dev is a parameter of nearly every engine kernel, so
// naming it changed their mangled symbols and nothing else).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "azk.h"
#include "azk_device.h"

namespace azk_eng {

enum { CNT_SIMS = 0, CNT_SCANNED, CNT_TRACE, CNT_CREATED, CNT_LEAVES, CNT_TERMINAL, CNT_MOVES, CNT_CACHE_HITS, CNT_REUSED, CNT_CARRIED,
       CNT_FORCED, CNT_PRUNED, CNT_PRUNE_OF,   // forced playouts: root selections that took a forced child; visits pruning removed from recorded pi, of how many
       CNT_N };

struct __attribute__((aligned(16))) NodeH { int N; float P; uint32_t meta; int fc; };

enum { LDS_REGIONS = 14,      // regions of an engine block's LDS: what lds_layout() fills in
       LDS_REGIONS_DEV = 12 };  // the first of them, whose offsets travel in Dev; carve_at() derives the last two

struct Dev {               // device view of the engine, passed to kernels by value
    GameDesc g;
    int G, cap, path_cap, rc_pad, leaf_dtype, table_size, lds_bytes;
    int lds_off[LDS_REGIONS_DEV];   // lds_layout()'s offsets, computed once on the host (k_tree reads them instead of redoing the arithmetic in every wave)
    int K;                 // leaves in flight per game (virtual-loss mode, opt-in; 1 = the reference's sequential search).  Every
                           // pending-leaf array below is [G * K], slot v = g * K + k
    // game state
    uint8_t *cells;        // [G][rc_pad]  cell codes (1 = player 0, 2 = player 1)
    int *to_move, *move_count, *done, *winner;   // [G]
    // tree arena, [G][cap] each (ai/node.py:21-40 as columns)
    NodeH *H;              // per node, ONE 16-byte record: Node.visit N, Node.prior P (float32 softmax entry), meta = (Node.prevAction as
                           // r*cols+c) << 16 | len(Node.children) (cell 0xFFFF = root), fc = index of children[0] in this game's arena
                           // (-1 = not expanded): a PUCT candidate costs one 16-byte load + W instead of five column loads
    double *W;             // Node.value (running sum)
    double *Q;             // W / (double)N of every node with N > 0, bit for bit the quotient the walk used to compute per child and level: kept by
                           // node_store_wq(), the one writer of a visited node's W.  UNSPECIFIED where N = 0 (never written there: fresh roots,
                           // new children), and every reader discards it there
    double *rootP;         // [G][rc] float64 root priors after Dirichlet mixing (utils.py:24-25), by child position
    int *root_f64;         // [G] root children use rootP (float64 UCB) instead of P (float32 UCB)
    int *arena_top;        // [G] bump allocator
    // pending leaf of the current simulation
    int *leaf_node, *leaf_depth, *leaf_nmoves, *leaf_slot;   // [G]
    int *path;             // [G][path_cap]
    uint8_t *leaf_cells;   // [G][rc_pad] board at the leaf
    int16_t *leaf_moves;   // [G][rc] valid moves at the leaf, reference list order
    uint8_t *leaf_flag;    // [G * K] 1 = this slot contributes a leaf to the evaluator batch this step
    int *to_move_v;        // [G * K] to_move of the slot's game (K > 1: what the leaf hand-off kernels index by slot)
    const double *noise;   // [G][A] or nullptr (asynchronous moves: [G][2][A], see noise_sel)
    const long long *noise_sel;   // asynchronous moves: [G] the slot's move counter - its low bit selects the row of the game's CURRENT search; else nullptr
    // eval cache (MCTS.cache, ai/mcts.py:7,38-51): per-game direct-mapped table keyed by the exact canonical position
    int cache_entries, key_words;          // entries per game (power of two, 0 = off); 64-bit words per key
    unsigned long long *cache_key;         // [G][E][key_words] own-stone bit plane, opponent bit plane (+ side bit)
    float *cache_logits;                   // [G][E][A] the evaluator's logits row
    float *cache_value;                    // [G][E]
    int *leaf_cache;                       // [G] >= 0: pending leaf was a cache hit (entry index); < 0: miss, insert at -(x)-1
    // shared mode (one table for every game of the engine, like the reference's process-global MCTS.cache): entries are written
    // at EXPANSION by whichever game wins the entry's claim word for the current launch stamp, and read at selection only when
    // their claim stamp is older than the current launch (the kernel boundary is the only cross-CU ordering relied on); a hit is
    // copied into the game's own buffers at once, because another game may overwrite the entry before this game expands
    int cache_shared;
    unsigned long long cache_mask;         // shared: entries - 1 (entries = the largest power of two <= G * cache_entries)
    unsigned *cache_claim;                 // shared: [entries] launch stamp of the entry's last write, 0 = never written
    unsigned *cache_stamp;                 // shared: [1] stamp of the current launch (bumped by the leaf hand-off kernels)
    unsigned long long *leaf_key;          // shared: [G][key_words] key of the pending (missed) leaf
    float *hit_logits, *hit_value;         // shared: [G][A], [G] private copy of a hit
    int16_t *traj_action;  // [G][state_dim] cell played at each ply of the current game (square boards with one action per cell and emit_elements engines, else null)
    double *traj_pi;       // [G][state_dim][A] visit distribution recorded at each ply
    long long *emit_base;  // [G] first tuple index (64-bit: the stream never wraps) of a game being emitted, -1 = not emitting
    int *sims_done;        // [G] simulations of the current search already run (budget stepping, azk_begin_search_budget)
    int *budget;           // [4] simulations per search, most simulations per game and launch, launch age (wall-clock ticks) up to which a
                           //     game may start another simulation (0: no limit), reserved
    long long *counters;   // [CNT_N][G]
    int *err;              // sticky error word
    int ablate;            // debug only (AZK_TREE_ABLATE): timing experiments that break parity on purpose
    long long *dbg;        // debug only: [G][8] cycle stamps per phase when ablate & 16
};

// tree reuse across moves (azk_config.tree_reuse, opt-in; all null / 0 otherwise).  Its own argument of the few kernels that need it:
// Dev - and with it the kernel-argument offsets and instruction stream of k_tree - is that of an engine without the feature
struct ReuseDev {
    int mode;              // 0 off, 1 carry, 2 top-up
    int words;             // 64-bit words of one game's mark bitmap: ceil(cap / 64)
    int *chosen_node;      // [G] arena index of the child k_advance played (the next search's root), -1 = start from a fresh root
    unsigned long long *bits;   // [G][words] k_reroot scratch: bit i = node i belongs to the kept subtree
    unsigned *pre;         // [G][words] k_reroot scratch: kept nodes below the word = new index of the word's first kept node
};

// playout-cap randomisation (azk_set_playout_cap, opt-in; n_fast == 0 otherwise): a search is FULL (the budget's simulations) with probability
// p_full and FAST (n_fast simulations) otherwise, by a coin keyed like the search's noise row.  Its own argument block, passed only to the CAP
// instantiations of the kernels it touches (azk_opt_pack.h, "the opt-ins"): Dev, AsyncDev and ReuseDev - and every kernel an engine without the
// option launches - stay as they were
struct CapDev {
    int n_fast;                // simulations of a fast search; 0 = off
    double p_full;
    unsigned long long seed;   // the coin's key: (seed, first_game + g, move key), azk_async_begin puts its own seed / first game here
    long long first_game;
    uint8_t *search_full;      // [G] kind of the game's current search: 1 full, 0 fast
    uint8_t *traj_full;        // [G][state_dim] kind of the search behind each ply of the current game (null where traj_pi is)
    uint8_t *rec_full;         // asynchronous record ring: [record_capacity] kind per record, or null
    long long *stats;          // asynchronous movers: the caller's stats_dev ([8] full, [9] fast searches begun), else null
};

// resignation (azk_set_resign, opt-in; v_resign == 0 otherwise): after a move that does not end the game, the side that
// has just moved concedes when the root's q (root.value / root.visit: the outcome as the mover's OPPONENT sees it) reached v_resign.  A coin
// per game makes it a never-resign control game, which is only marked with the side that would have conceded first and played on.  Its own
// argument block, passed only to the RESIGN instantiations of the two movers (azk_moves.hip; azk_opt_pack.h, "the opt-ins"): every other argument block - and
// every kernel an engine without the option launches - stays as it was
struct ResignDev {
    double v_resign;           // threshold on q, in (0, 1]; 0 = off
    double p_never;            // share of never-resign games
    int min_ply;               // no concession before the game has this many plies
    unsigned long long seed;   // the game coin's key: (seed, first_game + g, move key of the game's first search), azk_async_begin puts its own here
    long long first_game;
    uint8_t *resigned;         // [G] 1 = the game's last move ended it by resignation (written by every move of a live game)
    uint32_t *mark_start;      // [G] never-resign mark: the game (by its first search's move key) that mark_side belongs to
    int *mark_side;            // [G] the side that would have conceded first, -1 = none; valid only while mark_start is the current game's
    long long *stats;          // [4] games resigned, never-resign games ended, of those marked, of those whose marked side did not lose
    uint8_t *rec_resigned;     // asynchronous record ring: [record_capacity] 1 = the record's move was a resignation, or null
};

// forced playouts and policy target pruning at the root (azk_set_forced_playouts, opt-in; k == 0 otherwise): in a FORCED
// search - the option set and, on a capped engine, the search a full one - a root child with N >= 1 visits and mixed prior P is selected
// before any PUCT comparison while  N * N < (k * P) * (Np - 1)  (float64), and the pi that is RECORDED for the move loses the visits that
// only this floor explains.  Its own argument block, passed only to the FORCED instantiations (k_tree<.., FORCED> in azk_tree.hip, the two
// movers in azk_moves.hip): every other argument block - and every kernel an engine without the option launches - stays as it was
struct ForcedDev {
    double k;                      // KataGo's 2; 0 = off
    const uint8_t *search_full;    // [G] CapDev's kind of the game's current search (1 full: forced, 0 fast: not), or null without a cap
};

// Gumbel root search (azk_set_gumbel_root, opt-in; m == 0 otherwise): the root's children are scored gl = logit + Gumbel
// draw (rootP holds gl), a child is eligible for a simulation iff its visit count equals the word of the sequential-halving table at the
// simulation's index, and the move and the recorded pi come from completed Q values.  Its own argument block, passed only to the GUMBEL
// instantiations (k_tree<.., GUMBEL> in azk_tree.hip, the movers and the target kernel in azk_moves.hip): every other argument block - and
// every kernel an engine without the option launches - stays as it was
struct GumbelDev {
    int m;                     // actions sampled at the root, 1..64; 0 = off
    int n;                     // words per table row: n_sims - 1 (simulation 0 expands the root and selects nothing)
    double c_visit, c_scale;   // sigma(q) = (c_visit + max visits) * c_scale * q
    const int *table;          // [m + 1][n] row m' = schedule(m', n): the visit count a child must have to be eligible at root selection t
    float *logit;              // [G][rc] the root children's raw float32 logits, by child position
    float *v0;                 // [G] the root's value as its evaluation (or the eval cache) gave it, for the side to move
};

// configurable PUCT (azk_set_puct, opt-in): the exploration rate is a table word of the selecting node's visit count, and an
// unvisited child is worth a first-play urgency instead of the reference's 0.  Its own argument block, passed only to the PUCT instantiations
// (k_tree<.., PUCT> in azk_tree.hip): every other argument block - and every kernel an engine without the option launches - stays as it was
struct PuctDev {
    const double *c_table;     // [n_table] c at a node of Np visits: c_table[min(Np, n_table - 1)], built by the host (no device log)
    int n_table;               // 1..65536
    int fpu_mode;              // 0 as the reference (an unvisited child scores u0), 1 absolute, 2 the node's value minus a reduction
    double fpu_tree, fpu_root; // the value (mode 1) or the reduction r >= 0 (mode 2), below the root and at it
};

// exact game-end proofs (azk_set_solver, opt-in): a status byte per node, seen by the player who moved INTO the node - proofs
// start at terminal leaves and move up the path of the simulation that found them, the walk stops on proven nodes below the root, and selection
// shuts out children proven LOST.  Its own argument block, passed only to the SOLVER instantiations (k_tree<.., SOLVER> in azk_tree.hip): every
// other argument block - and every kernel an engine without the option launches - stays as it was
enum { SOLVER_UNKNOWN = 0, SOLVER_WON = 1, SOLVER_LOST = 2, SOLVER_DRAW = 3 };
enum { SST_TERMINAL = 0, SST_BY_WON_CHILD, SST_BY_ALL_CHILDREN, SST_STOPPED, SST_EXCLUDING, SST_ROOTS, SST_N };
struct SolverDev {
    uint8_t *status;           // [G][cap] beside the tree arena's columns; written UNKNOWN wherever a node is created and when the root is expanded
    long long *stats;          // [SST_N] the counters of azk_get_solver_stats
};

// move temperature (azk_set_move_temperature, opt-in): the played child is drawn with a weight per visit count, read from a
// host-built table whose row is the ply's (no device pow), after a visit offset and a value cutoff; a ply whose row is -1 plays the first
// most-visited child.  Its own argument block, passed only to the TEMP instantiations of the two movers (azk_moves.hip): every other argument
// block - and every kernel an engine without the option launches - stays as it was
struct TempDev {
    const int *row_of_ply;     // [n_plies] row of `weights` for a move at that ply, -1 = greedy; the last entry holds for every later ply
    const double *weights;     // [n_rows][n_cols] weight of a child by its visit count (less the offset); column 0 is 0
    int n_plies, n_cols;       // n_cols = max_sims + 1
    int visit_offset;          // >= 0: a child of N visits weighs weights[row][max(0, N - visit_offset)]
    double value_cutoff;       // >= 0: a child whose W / N is more than this below the most-visited child's weighs 0; < 0: no cutoff
    long long *stats;          // [4] plies drawn by weight, of those not the most-visited child, children cut, plies that fell back (all weights 0)
};

// value targets (azk_set_value_target, opt-in): every move keeps the root's q = W / N beside traj_pi, and emission writes
// t_i = (1 - r) * z_i + r * G_i in place of z_i, G the lam-horizon return over the game's own search values (v_i = -q_i), ending in z.  Its own
// argument block, passed only to the VALUE instantiations of the two movers (azk_moves.hip) and the two emitters (azk_emit.hip): every other
// argument block - and every kernel an engine without the option launches - stays as it was
struct ValueDev {
    double r;                  // weight of the search-based part G in the target, in [0, 1] (0: today's z, q still recorded)
    double lam;                // horizon of G in [0, 1]: 0 = the ply's own search value (Leela's q-ratio), 1 = z
    double *traj_q;            // [G][state_dim] q of each ply of the current game, beside traj_pi (the value for the mover's OPPONENT)
    double *traj_vt;           // [G][state_dim] the plies' targets: written by k_emit_alloc, read by k_emit_tuples
};

// evaluation under a board symmetry (azk_set_eval_symmetry, opt-in; mode == 0 otherwise): the evaluator is shown each pending
// leaf in orientation s = the fixed element, or a hash of (seed, the leaf's position), and its logits row is turned back before k_tree expands
// from it.  Its own argument of the two kernels that exist only for it (azk_sym.hip): every other argument block - and every kernel an engine
// without the option launches - stays as it was
struct SymDev {
    int mode;                  // 0 off, 1 position-keyed, 2 one fixed element
    int fixed;                 // mode 2: the element
    uint32_t seed_lo, seed_hi; // mode 1: the key's seed
    uint32_t valid;            // the elements the geometry admits, four bits each, lowest first
    int n_valid;
    uint8_t *leaf_sym;         // [G] element of the slot's pending leaf (written for flagged slots by k_sym_leaves)
    uint8_t *sym_cells;        // [G][rc_pad] the pending leaf's cells in that orientation: what k_gather and the fused evaluators read
    float *sym_logits;         // [G][A] the evaluator's rows turned back into the position's frame: what k_tree expands from
};

// (state, pi, z) emission under a mask of D4 elements (azk_config.emit_elements, opt-in; n == 0 otherwise): ply i >= 2 of
// a finished game is emitted once per element of the mask instead of under the reference's eight.  Its own argument block, passed only to the SYM
// instantiations of k_emit_alloc and k_emit_tuples (azk_emit.hip): every other argument block - and every kernel an engine without the option launches - stays as
// it was
struct EmitSym {
    uint32_t els;              // the mask's elements, four bits each, ascending, lowest first
    int n;                     // how many; 0 = off
};

// policy surprise weighting (azk_set_surprise_weighting, opt-in): every move records kl = KL(recorded pi || the root
// children's raw float32 priors) and a coin keyed like the playout coin (Philox word 3 = 0xFFFFFFFC); at emission a recorded ply is written
// c = floor(w) + (coin < frac(w)) times, w = (1 - lambda) + lambda * n_F * kl / (sum of kl over the game's recorded plies).  Its own
// argument block, passed only to the SURPRISE instantiations of the two movers (azk_moves.hip) and the two emitters (azk_emit.hip): every other argument
// block - and every kernel an engine without the option launches - stays as it was
struct SurpriseDev {
    double lambda;             // share of a game's weight that follows kl, in [0, 1] (0: one copy each, kl and coin still recorded)
    unsigned long long seed;   // the ply coin's key: (seed, first_game + g, move key), azk_async_begin puts its own seed / first game here
    long long first_game;
    double *traj_kl;           // [G][state_dim] kl of each ply of the current game, beside traj_pi
    double *traj_coin;         // [G][state_dim] the ply's coin
    uint16_t *traj_copies;     // [G][state_dim] copies of each ply's tuple group: written by k_emit_alloc, read by k_emit_tuples
    double *last_kl, *last_coin;   // [G] what the game's last move recorded (azk_get_surprise)
    double *rec_kl, *rec_coin; // asynchronous record ring: [record_capacity] columns, or null
};

// random openings (azk_set_openings, opt-in): a game that starts in slot g is, with probability p_open, played forward
// 1..max_plies uniformly drawn legal moves inside a centred window before its first search, by draws keyed like the search's noise row
// (Philox word 3 = 0xFFFFFFFA).  Those plies are ordinary plies without a search: emission leaves them out.  Its own argument block, passed
// only to k_open_pending and to the OPEN instantiations of the kernels that start games (azk_begin.hip) or emit them (azk_emit.hip): every other argument
// block - and every kernel an engine without the option launches - stays as it was
struct OpenDev {
    double p_open;             // share of the games that are opened
    int max_plies;             // an opening has 1..max_plies plies (less where it is cut short)
    int spread;                // window half-width about the board's centre, per axis; -1 = the whole board
    unsigned long long seed;   // the draws' key: (seed, first_game + g, move key of the game's first search); the option's own, in both drivers
    long long first_game;
    uint8_t *pending;          // [G] 1 = the slot's game has just started and has not been through open_game_one
    int *open_plies;           // [G] opening plies of the slot's current game (0: not opened)
    int16_t *actions;          // [G][state_dim] the cells those plies were played on, in order (an engine without trajectories has them too)
    long long *stats;          // [3] games opened, opening plies played, openings cut short
};
// ... and what emission needs of it
struct OpenEmit { const int *open_plies; };

// root noise on the legal moves (azk_set_root_noise, opt-in; mode == 0 otherwise): a search's Dirichlet row is drawn over the
// actions that are legal in the position it starts from - the root's children - and is +0.0 elsewhere; k_tree and reroot_one read it as they read
// any row.  Its own argument of the two kernels that exist only for it (azk_noise.hip: k_root_noise, k_root_noise_due): every other argument
// block - and every kernel an engine without the option launches - stays as it was
struct RootNoiseDev {
    int mode;                  // 0 off, 1 "legal": Gamma(alpha) per legal action, 2 "total": Gamma(alpha / n) for n legal actions
    double alpha;              // replaces azk_async_config.alpha while the option is set
    int *row_key;              // asynchronous engines: [G] the move key the game's row pair last got a row for, -1 = none; null otherwise
};

// adaptive search budgets (azk_set_kld_stop and azk_set_lead_stop, opt-in; DESIGN sections 31 and 32): a search runs in segments of `interval`
// simulations - sims_done is preset so that budget stepping stops the game after the segment - and at each checkpoint between two segments the
// game is either released for the next one or moved on the tree as it stands: once the KL divergence its root's visit distribution gained per
// simulation fell below min_gain (the KLD rule; min_gain == 0: off), or once the most-visited root child leads the second by more than the
// simulations left can make up (the lead rule; lead_factor == 0: off).  Either rule or both.
// Its own argument block, passed only to the kernels that exist for it (k_kld_arm in azk_begin.hip; k_kld_checkpoint and the movers
// k_move_async_kld in azk_moves_kld.hip): every other argument block - and every kernel an engine without the option launches - stays as it was
enum { KST_JUDGED = 0, KST_EARLY, KST_UNRUN, KST_ALLOWANCE, KST_N };
enum { LST_JUDGED = 0, LST_EARLY, LST_UNRUN, LST_FORCED, LST_ALLOWANCE, LST_N };
struct KldDev {
    int interval;              // simulations per segment, 1..max_sims (one value for both rules)
    int min_sims;              // KLD rule: no search ends early before it has run this many new simulations
    double min_gain;           // KLD rule: the threshold on KL gained per simulation, finite and > 0; 0 = the rule is off
    int max_children;          // row length of snap: the board's cells
    int *left;                 // [G] simulations of the search's allowance behind the current segment
    int *run;                  // [G] new simulations the search has run once the current segment is complete (azk_get_search_sims)
    int *ckpt;                 // [G] checkpoints the search has passed; negative once the search is over: ~(that count)
    int *snap_sum;             // KLD rule: [G] So: sum of the snapshot, 0 = none; null while the rule was never set
    int *snap;                 // KLD rule: [G][max_children] the root children's N at the last checkpoint, list order; null likewise
    double *rate;              // KLD rule: [G] the rate of the game's last judged checkpoint (azk_get_kld_rate); null likewise
    long long *stats;          // [KST_N] KLD rule: checkpoints judged, searches ended early, simulations those left unrun, searches that ran their allowance
    int *rec_sims;             // asynchronous record ring: [record_capacity] new simulations of the record's search, or null
    double lead_factor;        // lead rule: f, finite and > 0; 0 = the rule is off
    int lead_min_sims;         // lead rule: its own min_sims
    int *lead_rec;             // lead rule: [G][3] N1, N2 and left at the game's last judged lead checkpoint (azk_get_lead)
    long long *lead_stats;     // [LST_N] lead rule: checkpoints judged, searches ended early, simulations those left unrun, forced-move ends, searches that ran their allowance
};

// Arming (one lane; wherever a search begins, behind the begin code's own write of sims_done): the search's allowance T = budget - sims_done
// is cut into segments; the first one is what budget stepping sees.  A game that is done is not armed.  (The snapshot sum is the KLD rule's:
// it exists only while that rule is set.)
__device__ __forceinline__ void kld_arm_one(const Dev &d, const KldDev &kd, int g) {
    if (d.done[g] != 0) return;
    const int budget = d.budget[0];
    const int T = max(0, budget - d.sims_done[g]);
    const int seg = min(kd.interval, T);
    if (T > 0) d.sims_done[g] = budget - seg;
    kd.left[g] = T - seg;
    kd.run[g] = seg;
    kd.ckpt[g] = 0;
    if (kd.min_gain > 0.0) kd.snap_sum[g] = 0;
}

struct LdsView {
    uint8_t *board;
    int *path;
    int16_t *moves;
    float *e;
    int *cnt;
    double *cdf;
    MoveScratch ms;
    uint8_t *board1;       // two-wave k_tree: the expanding wave's board (the pending leaf's cells)
    int *ho;               // two-wave k_tree: hand-off words, see HO_*
};

__host__ __device__ inline int up16(int x) { return (x + 15) & ~15; }

__host__ __device__ inline int lds_layout(const GameDesc &g, int path_cap, int table_size, int *off) {
    // off[LDS_REGIONS]: offsets (bytes) of board, path, moves, e, cnt, cdf, bits, pref, ord, tabA, tabB, claim, board1, hand-off words
    int o = 0;
    off[0] = o; o += up16(g.rc);
    off[1] = o; o += up16(path_cap * 4);
    off[2] = o; o += up16(g.rc * 2);
    int ea = g.action_dim > g.rc ? g.action_dim : g.rc;
    off[3] = o; o += up16(ea * 4);
    off[4] = o; o += up16(ea * 4);
    off[5] = o; o += up16(ea * 8);
    int nwords = (g.rc * 8 + 31) >> 5;
    off[6] = o; o += up16((nwords > (table_size >> 5) + 2 ? nwords : (table_size >> 5) + 2) * 4);   // key bitmap, later the set table's occupancy bitmap
    off[7] = o; o += up16(nwords * 2);
    off[8] = o; o += up16(g.rc * 2);
    off[9] = o; o += up16(table_size * 2);
    off[10] = o; o += up16(table_size * 2);
    off[11] = o; o += up16(table_size * 4);
    off[12] = o; o += up16(g.rc);
    off[13] = o; o += 32;
    return o;
}

extern __shared__ __attribute__((aligned(16))) unsigned char azk_smem[];

__device__ __forceinline__ LdsView carve_at(const int *off, int table_size, int rc) {
    LdsView L;
    L.board = azk_smem + off[0];
    L.path = (int *)(azk_smem + off[1]);
    L.moves = (int16_t *)(azk_smem + off[2]);
    L.e = (float *)(azk_smem + off[3]);
    L.cnt = (int *)(azk_smem + off[4]);
    L.cdf = (double *)(azk_smem + off[5]);
    L.ms.bits = (uint32_t *)(azk_smem + off[6]);
    L.ms.pref = (uint16_t *)(azk_smem + off[7]);
    L.ms.ord = (int16_t *)(azk_smem + off[8]);
    L.ms.tabA = (uint16_t *)(azk_smem + off[9]);
    L.ms.tabB = (uint16_t *)(azk_smem + off[10]);
    L.ms.claim = (uint32_t *)(azk_smem + off[11]);
    L.ms.table_size = table_size;
    // (the last two regions follow `claim`; Dev carries the twelve offsets it always did, so no kernel's argument layout moves)
    const int o12 = off[11] + up16(table_size * 4);
    L.board1 = azk_smem + o12;
    L.ho = (int *)(azk_smem + o12 + up16(rc));
    return L;
}

// the same view for a kernel that has no Dev (or no reason to read its offsets): lds_layout() puts board1 and the hand-off words exactly
// where carve_at() looks for them
__device__ __forceinline__ LdsView carve(const GameDesc &g, int path_cap, int table_size) {
    int off[LDS_REGIONS];
    lds_layout(g, path_cap, table_size, off);
    return carve_at(off, table_size, g.rc);
}

__device__ __forceinline__ uint32_t meta_pack(int cell, int nch) { return ((uint32_t)(cell & 0xffff) << 16) | (uint32_t)nch; }
__device__ __forceinline__ int meta_cell(uint32_t m) { return (int)(m >> 16); }
__device__ __forceinline__ int meta_nch(uint32_t m) { return (int)(m & 0xffffu); }

// device counters: fire-and-forget atomics (no load -> add -> store round trip on the simulation's critical path)
__device__ __forceinline__ void count_add(const Dev &d, int which, int g, long long v) {
    atomicAdd((unsigned long long *)&d.counters[(size_t)which * d.G + g], (unsigned long long)v);
}

// The ONE copy of "a visited node's statistics change": every store of a node's N or W after its creation goes through these two, so that
// Q[node] == W[node] / (double)H[node].N holds bit for bit wherever N > 0 (the walk reads Q and divides nothing; the division is the one the
// walk's scan made, on the same operands).  N: the node's visit count as it stands behind the change, >= 1.
__device__ __forceinline__ void node_store_wq(const Dev &d, size_t idx, int N, double W) {       // the count itself stays as it is in memory
    d.W[idx] = W;
    d.Q[idx] = W / (double)N;
}
__device__ __forceinline__ void node_store(const Dev &d, size_t idx, int N, double W) {
    d.H[idx].N = N;
    node_store_wq(d, idx, N, W);
}

// Node.backup (node.py:62-74): the node at trace index i gets value * (-1)^(depth - i); lanes take one node each.
__device__ __forceinline__ void backup_path(const Dev &d, size_t base, const int *path, int depth, double value, bool undo_virtual_loss = false) {
    for (int i = azk_lane(); i <= depth; i += AZK_WAVE) {
        int nd = path[i];
        double sv = ((depth - i) & 1) ? -value : value;
        const int N = d.H[base + nd].N;
        const double W = d.W[base + nd];
        if (undo_virtual_loss) { node_store_wq(d, base + nd, N, (W + sv) + 1.0); continue; }     // the visit was counted at selection (same association as the short-path form)
        node_store(d, base + nd, N + 1, W + sv);
    }
}

// asynchronous self-play (azk_async_begin): the movers' own kernel argument, see azk_moves.hip
struct AsyncDev {
    int n_sims, sample_until, dirichlet;
    unsigned long long seed;
    long long first_game;
    double alpha;
    long long *slot_moves;     // [G] moves this slot has played since azk_async_begin (all its games): the RNG's move key
    double *noise;             // [G][2][A] engine-owned: row (k & 1) of game g is the Dirichlet row of its search with move key k, for the
                               //   current key (slot_moves[g]) and the next one - generated a whole search ahead of its use
    int *noise_key;            // [G] the highest move key whose row exists
    int *todo_list, *todo_count;   // games that moved since the last drain: their row for key slot_moves[g] + 1 is due (k_noise_ahead)
    long long *stats;          // caller's int64 [16]: games, plies, wins 0 / 1, draws, moves, record cursor, searches begun
    long long rec_cap;
    int *rec_meta; double *rec_q; double *rec_pi;
    int *fin_list, *fin_count; // games found finished by the drain
    // re-rooting engines only (azk_async_begin_reuse; null otherwise)
    int *parked;               // [G] 1 = the game has moved and waits for the drain to re-root it: the movers pass it by (its sims_done is the
                               //   largest int, so k_tree idles it whatever the budget becomes); the played child is in ReuseDev.chosen_node
    int *reroot_list, *reroot_count;   // the games parked since the last drain (k_reroot_list)
};

// ---- a search starts from a fresh root: the kernels that begin searches (azk_begin.hip) and the asynchronous mover (azk_moves.hip) ----
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

// Node(None, None, current_player, move_count) for every game (gomoku.py:134)
__device__ __forceinline__ void fresh_root_one(const Dev &d, int g) {
    drop_pending_cache_claim(d, g);
    const size_t base = (size_t)g * d.cap;
    d.H[base] = NodeH{0, 0.f, meta_pack(0xffff, 0), -1}; d.W[base] = 0.0;   // (N = 0: Q[base] is unspecified until the first backup)
    d.arena_top[g] = 1; d.root_f64[g] = 0;
    clear_leaf_slots(d, g);
    d.sims_done[g] = 0;
}

// Node(None, None, player, move_count) for one game of the asynchronous engine (one wave).  The search's Dirichlet row is NOT made here: a
// row's key (seed, global game, slot move counter) is known a whole search before its use, so the rows are generated one search ahead, off
// the step's chain (k_noise_ahead in the drain) - in this function the Marsaglia-Tsang chain (float64 log / cos / pow, two Philox blocks per
// try) cost a moving game's wave ~30 us inside a launch every other wave had left after 1 us.
__device__ __forceinline__ void begin_search_one(const Dev &d, const AsyncDev &p, int g) {
    if (azk_lane() == 0) {
        fresh_root_one(d, g);
        atomicAdd((unsigned long long *)&p.stats[7], 1ull);
    }
}

// make_move (gomoku.py:148) on the wave's LDS board: the mover's stone goes onto cellc, placed by lane 0; azk_check_winner follows it.  The
// ONE copy of the placing rule, which the movers (advance_one, azk_moves.hip) and the openings (open_game_one, azk_begin.hip) both play
// their plies through.  It is text, not a function: behind a call the compiler schedules the movers differently, and an engine without
// openings launches the device code it always launched (profiles/openings_isa_vs_parent.txt).  Two statements without a wrapper, for the
// same reason: use it only as a full statement at block scope, never as the body of an unbraced if / else / loop.
#define AZK_PLACE_STONE(board, gd, lane, mover, cellc)                                         \
    if ((lane) == 0) {                                                                         \
        if ((gd).kind == AZK_KIND_C4) (board)[cellc] |= (uint8_t)(1 << (mover));               \
        else if ((board)[cellc] == 0) (board)[cellc] = (uint8_t)(1 << (mover));                \
    }                                                                                          \
    __syncthreads()

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
inline bool make_game(int kind, int rows, int cols, GameDesc *g, std::string *err) {
    memset(g, 0, sizeof *g);
    g->kind = kind;
    if (kind == AZK_TICTACTOE) { rows = 3; cols = 3; g->planes = 3; g->win_len = 3; g->action_dim = 9; }
    else if (kind == AZK_CONNECT4) { rows = 6; cols = 7; g->planes = 3; g->win_len = 4; g->action_dim = 7; }
    else if (kind == AZK_GOMOKU) {
        // (<= 30 columns: azk_valid_moves_gomoku shifts the board's bit string by up to cols + 1 inside 64-bit words)
        if (rows < 1 || cols < 1 || rows * cols > 400 || cols > 30) { *err = "gomoku board must have 1..400 cells and at most 30 columns"; return false; }
        g->planes = 2; g->win_len = 5; g->action_dim = rows * cols;
    } else { *err = "unknown game id"; return false; }
    g->rows = rows; g->cols = cols; g->rc = rows * cols; g->state_dim = rows * cols;
    g->inv_cols = (65536u + (unsigned)cols - 1u) / (unsigned)cols;
    return true;
}

inline int table_size_for(const GameDesc &g) { return g.rc < 307 ? 512 : 2048; }   // CPython set growth: 8 -> 32 -> 128 -> 512 -> 2048

}  // namespace azk_eng
using namespace azk_eng;

struct azk_engine {
    Dev d;
    azk_config cfg;
    std::string err;
    std::vector<void *> allocs;
    long long *counter_sums = nullptr;   // device [CNT_N]
    int *n_leaf_scratch = nullptr;
    void *leaf_scratch = nullptr;        // used when the caller passes no leaf buffer
    uint32_t *vanilla_rng = nullptr;     // [G][625] MT19937 key + position (vanilla mode), allocated on first use
    double *lntab = nullptr;             // [lntab_n] math.log(N), from the host libm (the reference's math.log)
    int lntab_n = 0;
    bool multi = false;                  // budget stepping (azk_begin_search_budget): the MULTI instantiation of k_tree
    int budget_host[4] = {0, 1, 0, 0};
    int ticks_per_us = 100;              // constant-rate clock of wall_clock64()
    ReuseDev ru;                         // tree reuse (cfg.tree_reuse); ru.mode == 0: off, every pointer null
    AsyncDev ad;                         // asynchronous self-play (azk_async_begin); ad.slot_moves == nullptr: not set up
    CapDev cp = {};                      // playout-cap randomisation (azk_set_playout_cap); cp.n_fast == 0: off
    ResignDev rs = {};                   // resignation (azk_set_resign); rs.v_resign == 0: off
    double forced_k = 0.0;               // forced playouts + policy target pruning (azk_set_forced_playouts); 0: off
    ForcedDev forced() const { return ForcedDev{forced_k, cp.n_fast ? cp.search_full : nullptr}; }   // the argument block as the options stand now
    GumbelDev gb = {};                   // Gumbel root search (azk_set_gumbel_root); gb.m == 0: off
    int gumbel_sims = 0;                 // ... the n_sims its table was built for
    PuctDev pu = {};                     // configurable PUCT (azk_set_puct); puct_on == false: off, nothing allocated
    bool puct_on = false;                // (c_table = [1.0] with mode 0 is a live setting, so the switch is its own word)
    TempDev tp = {};                     // move temperature (azk_set_move_temperature); tp_on == false: off, nothing allocated
    bool tp_on = false;
    ValueDev vt = {};                    // value targets (azk_set_value_target); vt_on == false: off, nothing allocated
    bool vt_on = false;                  // (r = 0 is a live setting, so the switch is its own word)
    bool async_on = false;
    int async_recycle = 1;
    SymDev sym = {};                     // evaluation under a board symmetry (azk_set_eval_symmetry); sym.mode == 0: off, nothing allocated
    SurpriseDev sp = {};                 // policy surprise weighting (azk_set_surprise_weighting); sp_on == false: off, nothing allocated
    bool sp_on = false;                  // (lambda = 0 is a live setting, so the switch is its own word)
    EmitSym emit = {};                   // emission under a mask of elements (cfg.emit_elements); emit.n == 0: off, the reference's rule
    OpenDev op = {};                     // random openings (azk_set_openings); op_on == false: off, nothing allocated
    bool op_on = false;                  // (p_open = 0 is a live setting, so the switch is its own word)
    SolverDev sv = {};                   // exact game-end proofs (azk_set_solver); sv_on == false: off, nothing allocated
    bool sv_on = false;
    RootNoiseDev rn = {};                // root noise on the legal moves (azk_set_root_noise); rn.mode == 0: off, nothing allocated
    KldDev kd = {};                      // adaptive search budgets: kld_on - the KLD rule is set (azk_set_kld_stop), lead_on - the lead rule is
    bool kld_on = false;                 // (azk_set_lead_stop); neither: off, nothing allocated.  adaptive_on(e): either
    bool lead_on = false;
    bool in_search = false;             // between a search's begin and the move (or new position) that ends it: azk_set_eval_symmetry refuses
};

#define HIPCHK(e, call)                                                                 \
    do {                                                                                \
        hipError_t _s = (call);                                                         \
        if (_s != hipSuccess) {                                                         \
            (e)->err = std::string(#call) + ": " + hipGetErrorString(_s);              \
            return AZK_ERR_HIP;                                                         \
        }                                                                               \
    } while (0)

template <typename T>
static hipError_t dalloc(azk_engine *e, T **p, size_t count) {
    void *q = nullptr;
    hipError_t s = hipMalloc(&q, count * sizeof(T) + 64);
    if (s != hipSuccess) return s;
    e->allocs.push_back(q);
    *p = (T *)q;
    return hipSuccess;
}

// the simulation budget lives in device memory, so that a captured step graph keeps working when it changes: budget_host as it stands goes
// up, and the call waits for it
static inline int32_t upload_budget(azk_engine *e, hipStream_t st) {
    HIPCHK(e, hipMemcpyAsync(e->d.budget, e->budget_host, sizeof e->budget_host, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipStreamSynchronize(st));
    return AZK_OK;
}

// host symbols that cross engine files: hidden, not in include/azk.h
#define AZK_INTERNAL __attribute__((visibility("hidden")))
extern AZK_INTERNAL thread_local std::string azk_create_error;   // azk_last_error(nullptr): written by azk_create and the stateless rule calls (azk_engine.hip)
// the k_tree instantiation for this engine and step (azk_tree.hip)
AZK_INTERNAL int32_t azk_launch_tree(azk_engine *e, bool expand, bool select, bool multi, const float *logits, const float *values, hipStream_t st);
// azk_create's last step: every game empty, every tree a fresh root (azk_begin.hip)
AZK_INTERNAL int32_t azk_init_games(azk_engine *e);
// what the asynchronous engine (azk_moves.hip) launches out of the other families' files; all on the stream, none waits.
// azk_launch_first_searches: azk_async_begin - the first games opened (engines with random openings) and a fresh root for every game, under
// move key 0 (azk_begin.hip).  azk_launch_next_searches: the drain - finished games counted and restarted, parked games re-rooted (azk_begin.hip)
AZK_INTERNAL void azk_launch_first_searches(azk_engine *e, hipStream_t st);
AZK_INTERNAL int32_t azk_launch_next_searches(azk_engine *e, hipStream_t st);
// azk_launch_first_rows: azk_async_begin - every game's Dirichlet (Gumbel root: Gumbel) rows of move keys 0 and 1.  azk_launch_rows_ahead:
// the drain - the next row of every game that moved since the last one (azk_noise.hip)
AZK_INTERNAL void azk_launch_first_rows(azk_engine *e, hipStream_t st);
AZK_INTERNAL void azk_launch_rows_ahead(azk_engine *e, hipStream_t st);
// root noise on the legal moves (azk_set_root_noise), asynchronous engines: the rows are made where the position is known, not a search ahead.
// azk_root_noise_begin: azk_async_begin, behind the first searches - row_key allocated and cleared, noise_key at the largest int (the movers'
// "row exists" test holds), every game's first row.  azk_launch_root_noise_due: the row of every game whose key moved (azk_noise.hip)
AZK_INTERNAL int32_t azk_root_noise_begin(azk_engine *e, hipStream_t st);
AZK_INTERNAL void azk_launch_root_noise_due(azk_engine *e, hipStream_t st);
// adaptive search budgets under either rule?
static inline bool adaptive_on(const azk_engine *e) { return e->kld_on || e->lead_on; }
// adaptive search budgets (azk_set_kld_stop, azk_set_lead_stop): the searches that have just begun are armed - every game's (list == nullptr) or the *n_list listed
// ones'; returns at once while the option is off (azk_begin.hip)
AZK_INTERNAL void azk_launch_kld_arm(azk_engine *e, const int *list, const int *n_list, hipStream_t st);
// ... and the asynchronous movers of such an engine, in the place of k_move_async (azk_moves_kld.hip); on the stream, does not wait
AZK_INTERNAL void azk_launch_move_async_kld(azk_engine *e, hipStream_t st);
// azk_launch_emit: (state, pi, z) emission of the finished games, all G or the *n_list listed ones (azk_emit.hip)
AZK_INTERNAL void azk_launch_emit(azk_engine *e, float *states, double *pis, float *zs, long long capacity, unsigned long long *cursor, long long *game_base,
                                  const int *list, const int *n_list, hipStream_t st);
// azk_resign_clear: no game resigned, no mark, zero statistics (azk_options.hip)
AZK_INTERNAL int32_t azk_resign_clear(azk_engine *e, hipStream_t st);
// evaluation under a board symmetry (azk_sym.hip); both return at once while the option is off.  azk_sym_leaves: behind a selecting tree
// launch - element and turned cells of every flagged slot.  azk_sym_restore: in front of an expanding one - the rows it is to expand from
// (the engine's turned-back copy of `logits`, or `logits` itself)
AZK_INTERNAL int32_t azk_sym_leaves(azk_engine *e, hipStream_t st);
AZK_INTERNAL const float *azk_sym_restore(azk_engine *e, const float *logits, hipStream_t st);
