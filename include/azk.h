/*
 * azk.h - C ABI of libazk.so: the MI355X-native batched self-play engine (HIP, gfx950).
 *
 * This is the drop-in boundary for the reference's self-play hot path
 *     train.collect_data -> <Game>.self_play -> ai.mcts.MCTS.mcts -> Game statics + model
 * (reference files cited per entry point as file:line, relative to the reference root).
 * The reference has no native layer: everything below replaces interpreted Python.  The ABI is
 * plain C: no C++ / torch types, raw pointers + sizes, int32 status returns (0 = OK, <0 = error,
 * text via azk_last_error).  Pointers named *_dev are device (HBM) pointers - e.g. a torch
 * tensor's data_ptr() - valid until the stream reaches the call; *_host are host pointers.
 * `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream); every
 * kernel is enqueued on it and nothing here synchronises unless stated, so calls are capturable
 * in a hipGraph.  One host thread drives one engine; one engine per GPU / process.
 *
 * Data model (DESIGN.md "HBM layout"): G concurrent games; per game a structure-of-arrays tree
 * arena (the reference's Node fields, ai/node.py:21-40, one row per child edge): N int32, W float64,
 * P float32 (+ a float64 root-prior row after Dirichlet mixing), cell int16, first_child int32,
 * n_children int16.  One 64-lane wavefront owns one game; child blocks are contiguous, so a PUCT
 * scan is a coalesced read of the N/W/P columns.
 */
#ifndef AZK_H
#define AZK_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 2: azk_emit_finished's game_base_dev became int64*, azk_leaf_source gained cache_stamp, azk_config gained cache_shared /
 * leaves_per_step (round 2); 5: the split-K row GEMM with its two summing kernels and the float32-input MFMA tail
 * link were retired, azk_nn_ln_heads lost its unfolded-affine operands; callers compare azk_abi_version() with the header they were
 * built against */
#define AZK_ABI_VERSION 5

/* games (games/tictactoe.py, games/connect4.py, games/gomoku.py) */
#define AZK_TICTACTOE 0
#define AZK_CONNECT4 1
#define AZK_GOMOKU 2

/* leaf batch element type handed to the evaluator */
#define AZK_LEAF_F32 0
#define AZK_LEAF_BF16 1

/* status codes */
#define AZK_OK 0
#define AZK_ERR_ARG (-1)
#define AZK_ERR_HIP (-2)
#define AZK_ERR_ARENA_FULL (-3)
#define AZK_ERR_STATE (-4)

typedef struct azk_engine azk_engine;

typedef struct {
    int32_t game;          /* AZK_* */
    int32_t rows, cols;    /* Gomoku only (reference ships 7x7, gomoku.py:10; 15x15 by attribute override); 1..400 cells, at most 30 columns,
                            * rows and cols independent (cells and actions are row-major, r * cols + c) */
    int32_t n_games;       /* G: games resident on this GPU */
    int32_t max_sims;      /* largest mcts_iterations a search will run (arena sizing) */
    int32_t leaf_dtype;    /* AZK_LEAF_F32 | AZK_LEAF_BF16 */
    int32_t device;        /* HIP device ordinal */
    int32_t arena_nodes;   /* nodes per game; 0 = worst case 1 + max_sims * max_children */
    int32_t cache_entries; /* eval cache (MCTS.cache, ai/mcts.py:7,38-51): entries per game, power of two, 0 = off.  Exact keys
                            * (the whole canonical position), so a hit returns precisely what the evaluator returned. */
    int32_t cache_shared;  /* 0: one table per game (single writer; exact MCTS.matched bookkeeping of a one-game run).
                            * 1: ONE table of n_games * cache_entries entries shared by every game of the engine - the reference's
                            * MCTS.cache is process-global (mcts.py:7): positions reached by several games (openings) are evaluated
                            * once.  Entries are written at expansion under a per-entry claim word and become readable at the next
                            * tree launch; a hit is copied into the game's own buffers at once.  Results are identical in both
                            * modes (the cache is transparent); only the hit COUNT of the shared mode depends on timing. */
    int32_t leaves_per_step; /* 0 / 1: the reference's sequential search, one leaf in flight per game (parity mode, the default).
                              * K > 1 (OPT-IN, changes search results): virtual-loss expansion - K leaves in flight per game; a
                              * selection leaves a visit and a lost game on its path until the leaf's value is backed up, so the
                              * next selections of the same game go elsewhere; the evaluator batch holds up to n_games * K boards.
                              * Drive it with azk_begin_search_budget (n_sims completed simulations per game). */
    int32_t tree_reuse;    /* 0: every search starts from a fresh root (games/gomoku.py:134; parity mode, the default).
                            * 1 / 2 (OPT-IN, changes search results): tree reuse across moves - the search that follows azk_advance starts
                            * on the subtree under the child that was played, i.e. the reference's own MCTS.mcts (ai/mcts.py:11-60) handed
                            * `root = chosen_child; root.parent = None` with its visits, values and priors; with Dirichlet noise the new
                            * root's children get (double)(0.75f * prior) + 0.25 * noise of this move's row, exactly as a freshly expanded
                            * noisy root does.  azk_begin_search(_budget) moves the subtree to the front of the game's arena (k_reroot).
                            *   1 carry : the full n_sims new simulations on top of the carried statistics (a deeper search per move);
                            *   2 top-up: only max(1, n_sims - root.visit) new simulations, so the root ends at n_sims visits again;
                            *             needs azk_begin_search_budget.
                            * A game starts from a fresh root instead - today's behaviour, bit for bit - when the played child was never
                            * expanded, when the game was reset, recycled or given a position since its last search, or when the ARENA RULE
                            * refuses:  kept_nodes + n_new * widest <= nodes per game  must hold, with n_new the most simulations the search may
                            * still run (the budget's; max_sims for azk_begin_search) and widest = min(max_children, empty cells of the root
                            * position), a bound on the legal moves of every position below the root - the most a search can allocate, so
                            * AZK_ERR_ARENA_FULL cannot come from a re-rooted search.  (The new root's own child count is no such bound:
                            * Gomoku's legal moves are the cells next to a stone and grow along a line of play.)  With arena_nodes = 0 a carry engine allocates
                            * 1 + 2 * max_sims * max_children nodes per game (TWICE the default: about 17 GB instead of 9 GB at 2 048 games
                            * x 800 simulations of 15x15 Gomoku) and drops a subtree of more than about max_sims expansions; top-up fits
                            * the default arena.  Not with leaves_per_step > 1 (AZK_ERR_ARG).  The asynchronous movers take such an engine through
                            * azk_async_begin_reuse; azk_async_begin answers AZK_ERR_STATE. */
    int32_t emit_elements; /* 0: (state, pi, z) emission as the reference does it (train.py:30-49; parity mode, the default) - eight images per
                            * position from the third on, square boards with one action per cell only.
                            * m != 0 (OPT-IN): emission under the D4 elements of the bit mask m, bit s = element s of the emission's numbering
                            * (azk_set_eval_symmetry: 0 rot0, 1 lr, 2 tb, 3 rot90, 4 lr(rot90), 5 tb(rot90), 6 rot180, 7 rot270), on EVERY
                            * geometry; azk_emit_finished below has the semantics.  azk_create answers AZK_ERR_ARG for bits above 7, a mask
                            * without bit 0 and an element the geometry does not admit (azk_set_eval_symmetry's rule: all eight on square
                            * boards with one action per cell, {0, 1, 2, 6} on Gomoku with rows != cols, {0, 1} on Connect4).  A create-time
                            * field: the trajectory buffers such an engine always has exist before the first move, and no captured graph
                            * ever sees another device view.  They cost n_games * state_dim * action_dim * 8 bytes (+ 2 per ply), the same
                            * as a square board of equal cell count: 1.2 MB per game on a 13 x 30 Gomoku board, 2.4 kB on Connect4. */
    int32_t reserved[3];
} azk_config;

/* device-side work counters; sums over all games since the last azk_reset_counters */
typedef struct {
    int64_t sims;             /* iterations of ai/mcts.py:16 */
    int64_t edges_scanned;    /* children read by PUCT scans (utils.py:29-44) */
    int64_t trace_nodes;      /* nodes updated by backups (node.py:62-74) */
    int64_t edges_created;    /* children appended by expansions (node.py:50-59) */
    int64_t leaves_evaluated; /* leaf boards handed to the evaluator (mcts.py:46) */
    int64_t terminal_sims;    /* simulations that ended in mcts.py:25-32 */
    int64_t moves_played;
    int64_t cache_hits;       /* MCTS.matched (mcts.py:9,44): leaves served by the eval cache; leaves_evaluated counts the misses */
    int64_t roots_reused;     /* tree reuse: searches that began on a carried subtree (the others began on a fresh root) */
    int64_t nodes_carried;    /* tree reuse: nodes of those subtrees */
    int64_t forced_selections;      /* forced playouts: root selections that took a forced child (of `sims` root selections in all) */
    int64_t visits_pruned;          /* policy target pruning: visits removed from the recorded pi ... */
    int64_t visits_before_pruning;  /* ... of this many raw root-child visits (the moves of forced searches only) */
    int64_t reserved[3];
} azk_counters;

int32_t azk_abi_version(void);
/* e may be NULL: returns the message of the last failed azk_create on this thread */
const char *azk_last_error(const azk_engine *e);

/* ---- engine life cycle ---------------------------------------------------------------------- */
int32_t azk_create(const azk_config *cfg, azk_engine **out);
void azk_destroy(azk_engine *e);
/* geometry the caller needs to size buffers: planes F, rows, cols, action_dim A, state_dim */
int32_t azk_geometry(const azk_engine *e, int32_t *planes, int32_t *rows, int32_t *cols,
                     int32_t *action_dim, int32_t *state_dim);

/* Game(): empty boards, player 0 to move, move_count 0 (gomoku.py:16-17,125-126) for games [first, first+count) */
int32_t azk_reset_games(azk_engine *e, int32_t first, int32_t count, void *stream);
/* load caller positions: cells int8 [count][rows*cols] (0 empty, 1 player-0, 2 player-1), side to move, plies played.
 * This is how MCTS.mcts(model, board, root, ...) (ai/mcts.py:11) receives the caller's board and root. */
int32_t azk_set_positions(azk_engine *e, int32_t first, int32_t count, const int8_t *cells_host,
                          const int32_t *to_move_host, const int32_t *move_count_host, void *stream);

/* ---- one search = Node(None, None, player, move_count) + MCTS.mcts(...) (gomoku.py:134-136) ---- */
/* Fresh root for every game (a tree_reuse engine: the carried subtree of every game that has one, see azk_config).  noise_dev: float64 [G][A] Dirichlet draws (utils.py:24) or NULL for
 * dirichlet=False.  The pointer is read by later steps: keep it alive until the search ends. */
int32_t azk_begin_search(azk_engine *e, const double *noise_dev, void *stream);

/* Budget stepping: like azk_begin_search, plus a simulation budget per game.  After it, every azk_step / azk_step_tree lets a game
 * run on inside the launch while its simulations need no evaluator (terminal leaves, leaves served by the eval cache) and stop at
 * the first leaf that does, at n_sims simulations in all, or after max_sims_per_launch in one launch.  A game's simulations stay
 * strictly sequential, so trees and games are bit-identical to one-simulation-per-call stepping; the caller steps until
 * azk_search_unfinished reports 0 (games still owing simulations or an evaluation), then calls azk_step_expand_backup once. */
int32_t azk_begin_search_budget(azk_engine *e, const double *noise_dev, int32_t n_sims, int32_t max_sims_per_launch, void *stream);
int32_t azk_search_unfinished(azk_engine *e, int32_t *count_host, void *stream);

/* ---- asynchronous self-play: a game moves as soon as ITS search is done (games/gomoku.py:132-162 runs one game at a time; in
 * the batched engine that means no game waits for the slowest search of its batch).  Drive it as
 *     azk_async_begin;  loop { azk_async_step(logits, values);  evaluator over the pending leaves;  every few steps: azk_async_drain }
 * azk_async_step = one budget-stepped tree launch (as azk_step_tree after azk_begin_search_budget: a game's simulations stay strictly
 * sequential, so every tree is bit-identical to one-simulation-per-call stepping) followed by the per-game move kernel: a game whose
 * n_sims simulations are complete gets root statistics, pi recorded, the move chosen (sampled while move_count < sample_until_move with
 * the uniform of (seed, global game, slot move counter), else the first most-visited child), make_move / check_winner / draw, a record
 * into the caller's ring, and - unless it ended - its next search at once (fresh root, the Dirichlet row of its next move key).
 * azk_async_drain handles the games that ended: (state, pi, z) emission into the caller's replay ring (as azk_emit_finished; pass
 * states_dev = NULL to skip), statistics, and - with recycle - Game() + first search of the next game in the slot.
 * The random keys are those of the lock-step drivers (azk_gen_noise with move_index = the slot's move counter), so a slot plays the
 * same games move for move.  Both calls only enqueue kernels (capturable).
 * An engine created with tree_reuse = 1 | 2 begins with azk_async_begin_reuse and plays the games of the lock-step reuse drivers.  Its
 * move kernel does not begin the moved game's next search: it notes the played child and PARKS the game - the tree launches and the
 * movers pass a parked game by, whatever azk_async_set_budget does meanwhile - and the next search of a moved game begins at the
 * FOLLOWING azk_async_drain, which re-roots every parked game on its noted child (carry / top-up and the fresh-root fallbacks exactly
 * as azk_config.tree_reuse describes, with n_sims = the budget as it stands at that drain, and the Dirichlet row of the game's new
 * move key mixed into the new root's children) and un-parks it.  A game idles from its move to that drain, so such an engine wants
 * the drain often (a few steps apart); azk_counters.roots_reused / nodes_carried count as in the lock-step drivers.
 *   stats_dev  int64 [16], zeroed by azk_async_begin(_reuse): [0] games finished, [1] their plies (opening plies included), [2] wins of player 0, [3] of player 1,
 *              [4] draws, [5] moves played, [6] records written (ring cursor), [7] searches begun - by azk_async_begin's move kernel,
 *              by the drain's restart of a finished game, and by the drain's re-root of a parked game (carried subtree or fallback)
 *              [8] / [9] with a playout cap (azk_set_playout_cap): full / fast searches among those of [7]
 *   record ring (optional, record_capacity entries; entry r % capacity): rec_meta int32 [cap][4] = slot, the slot's move counter,
 *              chosen cell, winner (-2 running, -1 draw, 0 / 1); rec_q float64 [cap] = root.value / root.visit; rec_pi float64 [cap][A] */
typedef struct azk_async_config {
    int32_t n_sims, max_sims_per_launch, sample_until_move, dirichlet, recycle;
    int32_t young_launch_us;   /* > 0: a game starts another simulation inside a launch only while the launch is younger than this
                                * (a launch lasts as long as its slowest wave); 0: up to max_sims_per_launch whatever the time */
    uint64_t seed;
    int64_t first_global_game;
    double alpha;
    int64_t *stats_dev;
    int64_t record_capacity;
    int32_t *rec_meta_dev;
    double *rec_q_dev, *rec_pi_dev;
} azk_async_config;
int32_t azk_async_begin(azk_engine *e, const azk_async_config *cfg, void *stream);
/* azk_async_begin for an engine created with tree_reuse = 1 | 2 (AZK_ERR_STATE on any other; azk_async_begin answers the same on such an
 * engine).  azk_async_step, azk_async_drain and azk_async_set_budget serve both kinds. */
int32_t azk_async_begin_reuse(azk_engine *e, const azk_async_config *cfg, void *stream);
/* phases: bit 0 = the tree launch, bit 1 = the move kernel (3 = both; separately for per-kernel timing) */
int32_t azk_async_step(azk_engine *e, const float *logits_dev, const float *values_dev, int32_t phases, void *stream);
/* change the simulation budget of every later launch (it lives in device memory, so captured step graphs pick it up); synchronises */
int32_t azk_async_set_budget(azk_engine *e, int32_t n_sims, int32_t max_sims_per_launch, void *stream);
int32_t azk_async_drain(azk_engine *e, float *states_dev, double *pis_dev, float *zs_dev, int64_t capacity, int64_t *cursor_dev, void *stream);

/* ---- playout-cap randomisation (OPT-IN; off, the engine is what it was bit for bit).  The data-generation scheme of KataGo (Wu 2019,
 * section 3.1): each search is FULL - the budget's n_sims simulations, exactly the search the engine runs without the option - with
 * probability p_full, and FAST - n_fast simulations - otherwise.  A fast search only chooses the move: its ply is left out of the
 * (state, pi, z) emission (azk_emit_finished, azk_async_drain), so every pi that is trained on comes from a full search, while games
 * finish several times sooner.
 *   the coin   one per search, drawn where the search begins, keyed like the search's Dirichlet row: Philox4x32-10, counter
 *              {global game lo, global game hi, move key, 0xFFFFFFFE}, key (seed lo, seed hi), u = ((c0 << 32 | c1) >> 11) * 2^-53, full iff
 *              u < p_full.  Word 3 = 0xFFFFFFFE belongs to no other draw (azk_gen_noise's uniform has 0xFFFFFFFF, its rows it < 64 and
 *              it | 0x40000000): every noise row and move uniform is unchanged, and the coins do not depend on how games are sharded.
 *              p_full = 1: every search full; p_full = 0: every search fast.
 *   fast       the same search with fewer simulations: the game's completed-simulation count starts at budget - n_fast (the budget as it
 *              stands when the search begins; a budget below n_fast runs the budget), and budget stepping ends the search after n_fast.
 *              Dirichlet noise, eval cache, move selection, q and the records are those of any search.  DEVIATION from KataGo: fast
 *              searches keep the configured root noise (the mix is part of the tree kernel, which this option leaves untouched).
 *   tree_reuse the per-game target (n_sims full, n_fast fast) takes n_sims' place: carry runs target more simulations, top-up
 *              max(1, target - carried root visits); the arena rule uses the same count.
 *   emission   a game reserves the sum over its full plies of (ply < 2 ? 1 : 8) tuples; ply i's group lands at the sum over the full
 *              plies before it, each group as azk_emit_finished describes (boards rebuilt from ALL earlier plies).  A game without a
 *              full ply emits nothing and is marked and recycled as usual.
 * azk_set_playout_cap: 0 <= p_full <= 1, 1 <= n_fast <= max_sims, not with leaves_per_step > 1, else AZK_ERR_ARG; n_fast = 0 switches the
 * option off.  Call it before azk_async_begin(_reuse) (which then uses ITS seed and first_global_game for the coins, move key = the
 * slot's move counter, and counts stats_dev[8] full / [9] fast searches begun, where it counts [7]); AZK_ERR_ARG there when n_fast > n_sims.
 * Lock-step drivers begin every search with azk_begin_search_capped (azk_begin_search_budget + the move key; azk_begin_search and
 * azk_begin_search_budget answer AZK_ERR_STATE while a cap is set) and step as after azk_begin_search_budget.
 * azk_get_search_full: uint8 [G] into device memory, 1 = the game's current search is full (asynchronous copy on the stream).
 * azk_async_record_flags (optional, before azk_async_begin): a uint8 [record_capacity] column of the record ring, entry r % capacity = 1
 * when record r's search was full. */
int32_t azk_set_playout_cap(azk_engine *e, double p_full, int32_t n_fast, uint64_t seed, int64_t first_global_game, void *stream);
int32_t azk_begin_search_capped(azk_engine *e, const double *noise_dev, int32_t n_sims, int32_t max_sims_per_launch, int32_t move_index, void *stream);
int32_t azk_get_search_full(azk_engine *e, uint8_t *full_dev, void *stream);
int32_t azk_async_record_flags(azk_engine *e, uint8_t *rec_full_dev);

/* ---- resignation (OPT-IN; off, the engine is what it was bit for bit).  AlphaGo Zero's rule: a game whose outcome is decided stops
 * paying searches for it.  After a move that does not end the game, the side that has just moved concedes when the root value of the
 * search behind that move reached a threshold; a share of the games never resigns, so that the threshold's false positives can be counted.
 *   q          root.value / root.visit as azk_root_stats and the record ring give it, with NO sign change.  Node.backup stores in a node
 *              the value as seen by the player who moved INTO it, so the root's q is the expected outcome for the OPPONENT of the side to
 *              move: near +1 when the side to move - the mover of the ply - is lost.
 *   the rule   for the ply with move_count = mc before the move: the move the search chose is always played and recorded.  If it neither
 *              wins nor fills the board, and mc + 1 >= min_ply, and q >= v_resign (float64, the recorded q): in a game that may resign
 *              done = 1, winner = 1 - mover, the game's resigned flag = 1; in a never-resign game the game is marked with the mover -
 *              once, the first time - and plays on.  Everything downstream (emission and its z, recycling, the drain, restart, tree
 *              reuse, the statistics of azk_recycle_finished / stats_dev) sees an ordinary finished game whose winner is set.
 *   the coin   one per game, stateless: Philox4x32-10, counter {global game lo, global game hi, start, 0xFFFFFFFD}, key (seed lo, seed hi),
 *              u = ((c0 << 32 | c1) >> 11) * 2^-53, never-resign iff u < p_never.  start = low 32 bits of (the slot's move counter at the
 *              move - mc): the move key of the game's first search (a game that azk_set_positions started with move_count > 0 gets
 *              whatever the subtraction gives - still a pure function of the key).  Word 3 = 0xFFFFFFFD belongs to no other draw, so
 *              every noise row, move uniform and playout-cap coin is unchanged and the coins do not depend on the sharding.
 *   statistics int64 [4], counted by the mover at the move that ends a game, whatever the drain / recycle timing: [0] games ended by
 *              resignation, [1] never-resign games ended, [2] of those the marked ones, [3] of those the ones whose marked side did not
 *              lose (a win or a draw): the false positives.
 * azk_set_resign: v_resign in [0, 1] (0 switches the option off), p_never in [0, 1], min_ply >= 0, not with leaves_per_step > 1, else
 * AZK_ERR_ARG; clears flags, marks and statistics.  Call it before azk_async_begin(_reuse), which then keys the coin by ITS seed and
 * first_global_game, clears the same, and makes the movers apply the rule.  Lock-step drivers move with azk_advance_resign = azk_advance +
 * move_index, the slot's move counter (the move_index of the search's noise row); azk_advance answers AZK_ERR_STATE while the option is
 * set, azk_advance_resign while it is not.  Combines with tree_reuse and with a playout cap (a fast search resigns like a full one).
 * azk_get_resigned: uint8 [G] into device memory, 1 = the game's last move was a resignation (asynchronous copy on the stream).
 * azk_get_resign_stats: the four counts into host memory; synchronises.
 * azk_async_resign_flags (optional, before azk_async_begin): a uint8 [record_capacity] column of the record ring, entry r % capacity = 1
 * when record r's move was a resignation (its rec_meta winner is then the conceded one). */
int32_t azk_set_resign(azk_engine *e, double v_resign, int32_t min_ply, double p_never, uint64_t seed, int64_t first_global_game, void *stream);
int32_t azk_advance_resign(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index,
                           int32_t *chosen_cell_dev, int32_t *winner_dev, int32_t *done_dev, void *stream);
int32_t azk_get_resigned(azk_engine *e, uint8_t *resigned_dev, void *stream);
int32_t azk_get_resign_stats(azk_engine *e, int64_t *out4_host, void *stream);
int32_t azk_async_resign_flags(azk_engine *e, uint8_t *rec_resigned_dev);

/* ---- forced playouts and policy target pruning at the root (OPT-IN; off, the engine is what it was bit for bit).  KataGo's third
 * self-play economy (Wu 2019, section 3.2): every root child the search has tried gets a floor of visits proportional to the square root
 * of its noised prior, so that a move the Dirichlet noise points at is followed up; and the pi that is RECORDED loses exactly the visits
 * that only that floor explains, so that they do not pass for the search's liking.  All arithmetic float64; k > 0 (KataGo: 2).
 *   forced     a search is FORCED when the option is set and - on an engine with a playout cap - the search is a full one (fast searches
 *              run unforced; their pi is not recorded).  A forced search needs root noise: its priors are the root's float64 mixed
 *              priors P (utils.py:24-25).  A search begun with noise_dev = NULL while the option is set: AZK_ERR_STATE (azk_async_begin
 *              with dirichlet = 0 likewise).
 *   selection  the root only, every simulation of a forced search.  Np = the root's visit count as the scan has it (Np - 1 = the sum of
 *              its children's visits, for a fresh root and a re-rooted one alike).  A root child with N >= 1 visits is forced iff
 *                  (double)N * (double)N  <  (k * P) * (double)(Np - 1)
 *              and a forced child's score is +inf; everything else of the scan stays, "first maximum wins" (node.py:47) included: among
 *              several forced children the first in list order is taken.  Children with N = 0 are never forced.  No square root is
 *              taken.  Levels below the root are untouched.  The rule is stateless in (N, P, Np): it combines with tree_reuse 1 | 2.
 *   pruning    once per move, after the move is chosen.  Np = root visits, s = sqrt((double)Np), c* = the first child with the most
 *              visits (Node.max_visit_child):  pstar = W* / N* + (P* * s) / (double)(N* + 1).  For every other child with N >= 1:
 *                  nf = (int)floor(sqrt((k * P) * (double)(Np - 1)));   q = W / (double)N;   m = N
 *                  while (m > N - nf  &&  m > 0  &&  q + (P * s) / (double)m < pstar)  m -= 1
 *                  if (m == 1 && nf >= 1)  m = 0
 *              c* and children with N = 0 keep their counts; pi[action] = m / sum(m).
 *   who sees   RAW visits: the move (sampled or arg-max), azk_root_stats, q, resignation, tree reuse - a search with the option on plays
 *   what       exactly the move the same tree would play without it.  PRUNED counts: the recorded pi only - the trajectory behind
 *              azk_emit_finished / azk_async_drain's (state, pi, z) tuples and the asynchronous record ring's rec_pi.  The record of a
 *              fast search keeps raw counts.
 * azk_set_forced_playouts: k = 0 switches the option off; k < 0, NaN or infinite: AZK_ERR_ARG; not with leaves_per_step > 1 (AZK_ERR_ARG).
 * Call it before azk_async_begin(_reuse).  Combines with the playout cap, resignation, tree_reuse, plain and budget stepping and the
 * asynchronous movers.  azk_counters.forced_selections / visits_pruned / visits_before_pruning count what it did.
 * azk_root_policy_target: float64 [G][A] into device memory, what the next azk_advance would record for each game.  With the option off, or
 * for a game whose search is a fast one, this is azk_root_stats' pi bit for bit - a root without a visited child (no search yet, a finished
 * game) included: both divide by a zero sum and write NaN. */
int32_t azk_set_forced_playouts(azk_engine *e, double k, void *stream);
int32_t azk_root_policy_target(azk_engine *e, double *pi_dev, void *stream);

/* ---- evaluation under a board symmetry (OPT-IN; off, the engine is what it was bit for bit).  The self-play ingredient of AlphaGo Zero, Leela and
 * KataGo: the network sees each leaf in one of the board's orientations and its policy row is turned back, so that whatever orientation
 * bias the network has is mixed over instead of going straight into pi.  The element is a pure function of (seed, the leaf's POSITION) - not
 * a draw per evaluation - so the evaluator the search sees stays a function of the position,
 *     f'(pos) = restore_s(f(transform_s(pos))),   s = h(seed, pos),
 * and everything the engine holds bit for bit survives: the eval cache stays transparent (off, per game, shared), budget stepping, tree
 * reuse and the asynchronous movers play the trees and games of lock-step stepping with the same option.
 *   elements   the emission's numbering (azk_emit_finished; np.rot90 is counter-clockwise):
 *                  0 rot0   1 lr(rot0)   2 tb(rot0)   3 rot90   4 lr(rot90)   5 tb(rot90)   6 rot180   7 rot270
 *              src_s(j) = the source cell of output cell j = (i, c), row-major on an R x C board (N = R = C where the element transposes):
 *                  0 (i, c)   1 (i, C-1-c)   2 (R-1-i, c)   3 (c, N-1-i)   4 (N-1-c, N-1-i)   5 (c, i)   6 (R-1-i, C-1-c)   7 (N-1-c, i)
 *              dst_s = src_s^-1 = src_t with t = s except 3 <-> 7.
 *   valid      square boards with one action per cell (TicTacToe, square Gomoku): all eight;  Gomoku with rows != cols: {0, 1, 2, 6};
 *              Connect4: {0, 1} (gravity keeps the rows), with the action map column a -> cols - 1 - a under element 1.
 *   transform  the board the evaluator is shown: b'[j] = b[src_s(j)] over the cells (cell codes; padding bytes as the leaf's row has them);
 *              azk_step_gather's planes and the rows azk_leaf_source_of hands the fused evaluators are built from b'.  The side to move
 *              (plane 2, the plane order) is that of the leaf.
 *   restore    the evaluator's row l' is in the transformed frame; the tree expands from out[src_s(j)] = l'[j], i.e. out[a] = l'[dst_s(a)]
 *              (Connect4, element 1: out[a] = l'[cols - 1 - a]).  Values pass through.  The caller's logits buffer is read only: the engine
 *              expands from a float32 copy of its own.
 *   modes      0 off;  1 position-keyed, seed_or_element = the 64-bit seed;  2 one fixed element for every leaf, seed_or_element = the
 *              element (for tests, and to look at a network's orientation bias).
 *   the key    mode 1.  fmix = murmur3's 32-bit finaliser (h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16),
 *              seed_lo / seed_hi the halves of the seed, side = (to_move + leaf depth) & 1 the side to move at the leaf, code_i = cell i's
 *              code (1 = player 0's stone, 2 = player 1's), all arithmetic modulo 2^32:
 *                  h = fmix(seed_hi ^ side ^ 0x9E3779B9) + sum over occupied cells i of fmix(((i << 2) | code_i) ^ seed_lo)
 *                  r = fmix(h);   element = valid[((r >> 16) * n_valid) >> 16]          (valid in ascending order)
 *              (tests/eval_symmetry_restated.py restates it; over the 6 046 count-balanced 3 x 3 boards every element's share is within
 *              2.62 sigma of 1 / n_valid for seeds 0, 1, 12345, 2^40 + 7 and n_valid 8, 4, 2.)
 * azk_set_eval_symmetry: AZK_ERR_ARG for a mode outside 0..2, an element the geometry does not admit, leaves_per_step > 1 (the virtual-loss
 * schedule is not pinned under it), and for a call between the begin of a search and the azk_advance(_resign), azk_reset_games or
 * azk_set_positions that ends it (after azk_async_begin: always) - the engine stays usable.  Allocates its buffers at first use; with the
 * option off no kernel of it is launched and nothing is allocated.  Two small kernels beside the step (k_sym_leaves behind every tree
 * launch that selects, k_sym_logits in front of every one that expands); k_tree, k_gather and the evaluator kernels are unchanged.
 * Combines with tree_reuse, playout cap, resignation, forced playouts, plain and budget stepping, the eval cache and the asynchronous movers.
 * azk_get_leaf_symmetry: uint8 [G] into device memory, the element of each game's pending leaf (valid where the game has one that needs
 * the evaluator; asynchronous copy on the stream).  azk_eval_symmetry_restore: the restore alone, into a caller buffer - for every game with
 * such a pending leaf, row r = its evaluator row: out_dev[r][a] = logits_dev[r][dst_s(a)]; other rows of out_dev are not written.  Both
 * answer AZK_ERR_STATE while the option is off. */
int32_t azk_set_eval_symmetry(azk_engine *e, int32_t mode, uint64_t seed_or_element, void *stream);
int32_t azk_get_leaf_symmetry(azk_engine *e, uint8_t *out_dev, void *stream);
int32_t azk_eval_symmetry_restore(azk_engine *e, const float *logits_dev, float *out_dev, void *stream);

/* ---- policy surprise weighting (OPT-IN; off, the engine is what it was bit for bit).  KataGo's data-weighting rule ("KataGoMethods"): a
 * recorded ply is written into the replay ring with a frequency proportional to how much the search disagreed with the network's own
 * prior, so that the positions the network is most wrong about are seen most often - while a game still writes, in expectation, as many
 * tuples as it has recorded plies.  Games, searches, moves and q are untouched.  All arithmetic float64.
 *   kl         at each move, after the forced-playout pruning, on the counts m_a and their sum the recorded pi is made of: over the root's
 *              children with m > 0,  p = (double)m / (double)sum,  P = (double)max(prior, 0x1p-126f),  t = p * log(p / P);
 *              kl = max(0.0, sum of t).  prior is the child's RAW float32 softmax entry as the tree stores it (the softmax over all A
 *              actions, turned back where evaluation symmetry is on) - not the root's Dirichlet mix.  Each lane of the mover's wave sums
 *              its children (i, i + 64, ...) in list order and the wave adds the 64 partial sums pairwise (xor butterfly 32, 16, .. 1); log
 *              is the device library's float64 log.
 *   the coin   one per ply: Philox4x32-10, counter {global game lo, global game hi, move key, 0xFFFFFFFC}, key (seed lo, seed hi),
 *              u = ((c0 << 32 | c1) >> 11) * 2^-53.  The move key is the slot's move counter (the move_index of the search's noise row).
 *              Word 3 = 0xFFFFFFFC belongs to no other draw, so every noise row, move uniform, playout-cap coin and resignation coin is
 *              unchanged and the coins do not depend on the sharding.
 *   record     kl and coin go into two float64 trajectory columns [G][state_dim] beside the ply's pi, and into a per-game pair that holds
 *              what the game's last move recorded (azk_get_surprise).  On a capped engine fast plies record both too; they carry no weight.
 *   emission   for a finished game with recorded plies F (all plies; on a capped engine the full ones), n_F = |F|, S = the sequential
 *              sum of kl_i over F in ply order:
 *                  w_i = S > 0 ? (1.0 - lambda) + ((lambda * (double)n_F) * kl_i) / S : 1.0
 *                  c_i = (int)floor(w_i) + (coin_i < w_i - floor(w_i) ? 1 : 0)                 (0 for plies outside F)
 *              The game reserves sum c_i * grp_i tuples (grp_i = 1 for plies 0 and 1, else the ply's group: 8, or the mask's elements with
 *              emit_elements); ply i's tuples start at base + sum_{j<i} c_j * grp_j and lie copy-major - copy 0's whole group, then copy
 *              1's - each group byte for byte the one the ply gets without the option.  Ring slot t % capacity, the 64-bit cursor,
 *              game_base_dev, the pushed-out skip, z and the asynchronous drain are as ever.  sum w_i = n_F, so the ring fills at the rate
 *              it fills without the option; lambda = 0 gives c_i = 1: the option-off ring, byte for byte, with kl and coin still recorded.
 * azk_set_surprise_weighting: lambda in [0, 1] (lambda = 0 is a live setting), else - NaN included - AZK_ERR_ARG; not with leaves_per_step
 * > 1 and not on an engine without trajectory buffers (where azk_emit_finished answers AZK_ERR_ARG): AZK_ERR_ARG.  Allocates the three
 * columns at first use.  Call it before azk_async_begin(_reuse), which then keys the coin by ITS seed and first_global_game.
 * azk_clear_surprise_weighting switches the option off: the engine launches what it launched before.  Lock-step drivers move with
 * azk_advance_keyed = azk_advance + move_index (it applies resignation too where that is set); azk_advance and azk_advance_resign answer
 * AZK_ERR_STATE while the option is set, azk_advance_keyed while it is not.  Combines with tree_reuse, the playout cap, resignation, forced
 * playouts (kl of the pruned pi), evaluation symmetry, emit_elements and the asynchronous movers.
 * azk_get_surprise: float64 [G] each into device memory, the kl and the coin each game's last move recorded (either pointer may be NULL;
 * asynchronous copies on the stream).  azk_async_surprise_columns (optional, before azk_async_begin): float64 [record_capacity] columns of
 * the record ring, entry r % capacity = record r's kl and coin (either may be NULL). */
int32_t azk_set_surprise_weighting(azk_engine *e, double lambda, uint64_t seed, int64_t first_global_game, void *stream);
int32_t azk_clear_surprise_weighting(azk_engine *e);
int32_t azk_advance_keyed(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index,
                          int32_t *chosen_cell_dev, int32_t *winner_dev, int32_t *done_dev, void *stream);
int32_t azk_get_surprise(azk_engine *e, double *kl_dev, double *coin_dev, void *stream);
int32_t azk_async_surprise_columns(azk_engine *e, double *rec_kl_dev, double *rec_coin_dev);

/* ---- Gumbel root search (OPT-IN; off, the engine is what it was bit for bit).  "Policy improvement by planning with Gumbel" (Danihelka et
 * al., ICLR 2022): m root actions are sampled without replacement by the Gumbel-top-k trick, the search's simulations are spread over them by
 * sequential halving, the survivor is played, and the recorded pi is softmax(logits + sigma(completed Q)) - a policy improvement at any
 * budget, 16 or 32 simulations included.  Levels below the root keep the reference's PUCT.  All arithmetic float64.
 *   rows       while the option is set, noise_dev of azk_begin_search / azk_begin_search_budget carries the games' GUMBEL rows g[G][A] instead
 *              of Dirichlet rows: no Dirichlet mixing takes place, a row of zeros is the noise-free (arena) search, NULL: AZK_ERR_STATE.
 *   schedule   schedule(m, n) is a list of n visit counts.  m <= 1: 0, 1, .., n - 1.  Else L = ceil(log2 m), v[0..m-1] = 0, c = m, and while
 *              the list is shorter than n:  extra = max(1, n / (L * c)) (integer division);  extra times: append v[0..c-1], then add 1 to each
 *              of v[0..c-1];  then c = max(2, c / 2).  Cut to n.  The engine keeps the rows m' = 0..m for n = n_sims - 1 (simulation 0 expands
 *              the root and selects nothing).  schedule(4, 15) = 0,0,0,0,1,1,2,2,3,3,4,4,5,5,6.
 *   expansion  of the root: children, float32 priors and the eval-cache write as ever; child i with action a also gets its base score
 *              gl_i = (double)logit_a + g[a]  (the raw float32 logit), which azk_root_children / azk_export_tree report as its prior; its
 *              logit and the root's float32 value v0 (the evaluator's or the cache's, for the side to move) are kept.
 *   selection  the root only, in every simulation.  Np = the root's visit count, t = Np - 1, m' = min(m, children),
 *              cv = schedule(m', n)[min(t, n - 1)],  sig = (c_visit + (double)cv) * c_scale.  A child with N visits and value sum W scores
 *                  N == cv ? (N != 0 ? gl + sig * (W / (double)N) : gl) : -inf
 *              and the first maximum wins.  Every simulation finds an eligible child and exactly min(m, children) children are ever visited.
 *   move and   once per move, children in list order.  S = sum N;  q_i = W_i / N_i for N_i > 0;  P_i = the child's float32 prior;
 *   target     pv = sum over visited of P_i,  pq = sum over visited of P_i * q_i  (both sequential in list order);
 *                  vmix = S > 0 ? (v0 + S * (pq / pv)) / (1 + S) : v0;   qh_i = N_i > 0 ? q_i : vmix;   sigf = (c_visit + max N) * c_scale
 *              The move: among the children with N_i == max N, the first maximum of gl_i + sigf * qh_i.  The recorded pi:
 *                  y_i = logit_i + sigf * qh_i;   pi[a_i] = exp(y_i - max y) / sum_j exp(y_j - max y);   0 on every other action
 *              (each lane of the mover's wave sums its children's exponentials in list order, the wave adds the 64 partial sums pairwise).
 *              azk_advance(_resign) ignores uniforms_dev and sample_until_move (the Gumbel arg-max is the sample), and so do the asynchronous
 *              movers with azk_async_config.sample_until_move.
 *   who sees   the recorded pi goes where pi goes: the trajectory behind azk_emit_finished / azk_async_drain's tuples, the asynchronous
 *   what       record ring's rec_pi, and azk_root_policy_target.  azk_root_stats, q, resignation and the counters keep raw visits.
 *   gen        azk_gen_gumbel: float64 [G][A] into device memory.  Entry a of game g draws one Philox4x32-10 block at counter
 *              {gg lo, gg hi ^ (a << 8), move_index, 0xFFFFFFFB}, gg = first_global_game + g, key (seed lo, seed hi);
 *              u = (((c0 << 32 | c1) >> 12) + 0.5) * 2^-52 (exact, strictly inside (0, 1));  g = -log(-log(u)).  Word 3 = 0xFFFFFFFB is no
 *              other stream's.  The asynchronous movers (dirichlet = 1) make these rows a search ahead where they make Dirichlet rows now.
 *              azk_gen_gumbel_uniforms: the same call's uniforms u, float64 [G][A] (what a restatement compares bit for bit).
 * azk_set_gumbel_root: 1 <= m <= 64, 2 <= n_sims <= max_sims, c_visit >= 0 and c_scale > 0, both finite, else AZK_ERR_ARG; not with
 * leaves_per_step > 1 (AZK_ERR_ARG).  AZK_ERR_STATE in combination with tree reuse, a playout cap, forced playouts or surprise weighting (the
 * eligibility rule needs a fresh root, one budget and raw root selection; those options' setters refuse likewise while a Gumbel root is
 * set), for a budget search or azk_async_begin whose n_sims differs from the option's, for azk_async_begin with dirichlet = 0 and for
 * azk_async_begin_reuse, and after azk_async_begin.  azk_clear_gumbel_root switches the option off.  Combines with resignation,
 * evaluation symmetry, emit_elements, the eval cache, plain and budget stepping and the asynchronous movers. */
int32_t azk_set_gumbel_root(azk_engine *e, int32_t m, int32_t n_sims, double c_visit, double c_scale, void *stream);
int32_t azk_clear_gumbel_root(azk_engine *e);
int32_t azk_gen_gumbel(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *gumbel_dev, void *stream);
int32_t azk_gen_gumbel_uniforms(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *uniforms_dev, void *stream);

/* ---- configurable PUCT: exploration-rate schedule and first-play urgency (OPT-IN; off, the engine launches exactly the kernels it launched
 * before).  The reference scores a child  Q + P * sqrt(Np) / (N + 1)  with no constant, and an unvisited child as if its Q were 0
 * (utils.calcUcbOfChildrenFromParent).  With the option the selecting product kernels have PUCT siblings that follow this rule (DESIGN
 * section 26):
 *   state      c_table    float64 [n_table], 1 <= n_table <= 65536, built by the host (AlphaZero's log((1 + N + c_base) / c_base) + c_init is a
 *                         table the caller fills; no device log).
 *              fpu_mode   0 as the reference, 1 absolute, 2 the selecting node's value minus a reduction.
 *              fpu_tree, fpu_root   the value (mode 1) or the reduction r >= 0 (mode 2); fpu_root at the root, fpu_tree below it.
 *   per level  selection at a node of Np visits (>= 1 whenever it has children) and value sum Wn:
 *                  c = c_table[min(Np, n_table - 1)];   f = the node is the root ? fpu_root : fpu_tree
 *                  mode 1: qf = f.   mode 2: qn = -(Wn / (double)Np)  (the node's value for the side that chooses here: Node.backup keeps the
 *                  sum as the player who moved INTO the node sees it);  qf = qn - f * sqrt((double)vm).
 *              vm = the prior mass of the node's visited children, the sum of P over the children with N > 0, in a fixed order: lane l of the
 *              wave adds its children l, l + 64, .. in list order starting from 0, then the 64 partial sums are combined by the xor butterfly
 *              32, 16, 8, 4, 2, 1 as x = x + partner.  On the float64 root path P is the root's mixed float64 prior and the sum is float64;
 *              elsewhere P is the float32 prior and the sum is float32, widened afterwards.
 *   score      of a child (N, W, P).  Float64 root path (a root that got noise rows):
 *                  s = c * sqrt((double)Np);   u0 = P * s / (double)(N + 1);   visited: W / (double)N + u0;   unvisited: mode 0 ? u0 : qf + u0
 *              Float32 path (everything else):
 *                  s = (float)(c * sqrt((double)Np));   u0 = (P * s) / (float)(N + 1);   visited: (float)(W / (double)N) + u0;
 *                  unvisited: mode 0 ? u0 : (float)qf + u0
 *              The first maximum wins, in all three forms of the scan.  c_table = {1.0} with mode 0 is the reference's formula bit for bit.
 *   stateless  the rule reads nothing the tree does not store already: it holds on a re-rooted tree, under budget stepping and in the
 *              asynchronous movers as it stands.  Expansion, backup, the root's noise weight (0.25), the movers and the evaluator are untouched.
 * azk_set_puct copies the table to device memory (a table of its own per call; nothing is allocated while the option was never set).
 * AZK_ERR_ARG: a null table, n_table outside [1, 65536], a table entry that is negative, NaN or infinite, a mode outside 0..2, a non-finite
 * FPU parameter, a negative reduction in mode 2, an engine with leaves_per_step > 1.  AZK_ERR_STATE: with forced playouts (the pruning bound
 * restates the selection formula) or a Gumbel root set - azk_set_forced_playouts and azk_set_gumbel_root refuse likewise while the option is
 * set; between the begin of a search and the call that ends it (a move, new positions or a reset); after azk_async_begin; and
 * azk_vanilla_search while the option is set (vanilla UCB1 is not covered).  azk_clear_puct switches the option off, under the same two state
 * rules.  Combines with tree reuse, a playout cap, resignation, evaluation symmetry, emit_elements, surprise weighting, random openings, the
 * eval cache in every mode, plain and budget stepping and the asynchronous movers with and without re-rooting. */
int32_t azk_set_puct(azk_engine *e, const double *c_table_host, int32_t n_table, int32_t fpu_mode, double fpu_tree, double fpu_root, void *stream);
int32_t azk_clear_puct(azk_engine *e);

/* ---- exact game-end proofs in the search: a solver for k_tree (OPT-IN; off, the engine launches exactly the kernels it launched before).
 * A simulation that walks into a decided position learns nothing new, and the reference's search never writes a decided result down.  With
 * the option every node keeps a STATUS byte, seen by the player who moved INTO the node - the view Node.value has (node.py:34) - as in
 * Winands' MCTS-Solver and Leela's certainty propagation:
 *   status     0 UNKNOWN;  1 WON, backed up as +1;  2 LOST, backed up as -1;  3 DRAW, backed up as 0.  A new node is UNKNOWN whatever the
 *              arena slot held before (recycled, restarted and re-positioned games); the root becomes UNKNOWN when it is expanded.
 *   walk       descends while the node has children and is either the root or UNKNOWN.  If it stops on a proven node other than the root
 *              the simulation ends there: check_winner, the eval-cache probe, the move list and the evaluator are skipped and the status's
 *              value is backed up along the path exactly as a terminal value is.  The root is never stopped on: it keeps selecting, so
 *              N[root] = 1 + sum N[child] still holds and the movers, pi, q and resignation read what they read without the option.
 *   terminal   the first arrival at a terminal leaf (mcts.py:25-32) marks it - WON for a win, DRAW for a full board - and the proof runs
 *              from it; later arrivals find it proven.
 *   proof      after a node c on the path has just become proven, its parent p on the path is examined, from the leaf upwards: p already
 *              proven: stop.  c WON: p becomes LOST.  Otherwise the statuses of ALL of p's children are read in list order: any UNKNOWN:
 *              stop; all LOST: p becomes WON; otherwise (LOST and DRAW) p becomes DRAW.  If p was newly proven the proof goes on to its
 *              parent; the root takes a status like any node.  The backup of the simulation's value does not change.
 *   selection  at the root or an UNKNOWN node the scores are computed as without the option, on both precision paths and in all three forms
 *              of the scan; then a WON child scores +infinity (possible only at a proven root) and a LOST child -infinity provided at least
 *              one child of the node is not LOST (if every child is LOST the scores stay as they were).  The first maximum wins; a DRAW
 *              child is an ordinary candidate.
 *   hence      an UNKNOWN node never has a WON child and has at least one UNKNOWN child.  At a root proven for its mover every further
 *              simulation goes to the first WON child, whose visits then dominate pi and the move without the movers knowing the option.
 *              Every W is still a sum of float32 network values and of +1, -1 and 0.  With the option on and no terminal reached, the tree
 *              is the option-off tree bit for bit.
 * azk_set_solver allocates the status column (uint8 [G][cap]) and six counters on first use and zeroes both (nothing is allocated while the
 * option was never set); azk_clear_solver makes the engine launch what it launched before.  AZK_ERR_ARG: an engine with leaves_per_step > 1.
 * AZK_ERR_STATE: with forced playouts, a Gumbel root or configurable PUCT set - azk_set_forced_playouts, azk_set_gumbel_root and
 * azk_set_puct refuse likewise while the solver is set; on an engine created with tree_reuse != 0 (the status column is not carried through
 * a re-rooting; azk_async_begin_reuse refuses likewise); between the begin of a search and the call that ends it; after azk_async_begin;
 * and azk_vanilla_search while the option is set.  Combines with a playout cap, resignation, evaluation symmetry, emit_elements, surprise
 * weighting, random openings, a move temperature, value targets, the eval cache in both modes, plain and budget stepping and the
 * asynchronous movers without re-rooting.
 * azk_get_solver_status: root_status_host int8 [G], each root's status as the side TO MOVE at the root sees it - 0 unknown, 1 wins, 2 loses,
 * 3 draw: the flip of the stored WON and LOST.  Meaningful from the root's expansion (a search's first simulation) on.  Waits.
 * azk_export_tree_status: status_host uint8 [cap], the stored statuses of one game's nodes in azk_export_tree's row order; returns the node
 * count.  azk_get_solver_stats: out6_host int64 [6] since azk_set_solver - terminal leaves marked; nodes proven by one WON child; nodes proven
 * by all their children; simulations ended on a proven node that has children; selections that shut at least one child out; roots that took
 * a status.  All three: AZK_ERR_STATE while the option is off.
 * azk_debug_fill_solver_status (debug / tests only): every byte of the status column becomes `byte`; for engines whose trees are fresh
 * roots - a search that follows must come out the same whatever was filled in. */
int32_t azk_set_solver(azk_engine *e, void *stream);
int32_t azk_clear_solver(azk_engine *e);
int32_t azk_get_solver_status(azk_engine *e, int8_t *root_status_host, void *stream);
int32_t azk_export_tree_status(azk_engine *e, int32_t game, int32_t cap, uint8_t *status_host, void *stream);
int32_t azk_get_solver_stats(azk_engine *e, int64_t *out6_host, void *stream);
int32_t azk_debug_fill_solver_status(azk_engine *e, int32_t byte, void *stream);

/* ---- move temperature: per-ply schedule, visit offset, value cutoff (OPT-IN; off, the engine launches exactly the kernels it launched
 * before).  The reference picks a move in one way: in proportion to the visits while move_count < sample_until, the first most-visited child
 * afterwards.  With the option the movers (azk_advance*, the asynchronous movers) ignore sample_until_move - the argument and
 * azk_async_config.sample_until_move alike - and follow this rule, all float64.  The engine knows no temperature, only a
 * weight per visit count that the host puts into a table (no device pow):
 *   state      row_of_ply   int32 [n_plies]: entry p is a row of `weights` or -1 (greedy); the last entry holds for every later ply.
 *              weights      float64 [n_rows][n_cols], n_cols = max_sims + 1.  A temperature tau is the row pow(n, 1 / tau).
 *              visit_offset >= 0 (Leela's temp-visit-offset).   value_cutoff: >= 0 (Leela's temp-value-cutoff), negative = none.
 *   per move   of a game with mc plies played:  r = row_of_ply[min(mc, n_plies - 1)].
 *              b = the first root child with the most visits (Node.max_visit_child), qb = W_b / N_b.
 *              No uniforms (uniforms_dev == NULL) or r < 0: b is played.  Otherwise, for every root child i in list order,
 *                  w_i = weights[r][max(0, N_i - visit_offset)];
 *                  if value_cutoff >= 0 and w_i > 0 and W_i / N_i < qb - value_cutoff:  w_i = 0, the child is cut
 *              (W / N of a child: the outcome as the side choosing at the root sees it).  w[a] = w_i of the child with action a, 0 where there
 *              is none;  S = w[0] + w[1] + .. + w[A - 1], added in that order.  S == 0: b is played (a fallback).  Otherwise what the sampler
 *              does with the counts:  acc += w[a] / S, cdf[a] = acc in that order;  index = the first a with u < cdf[a] / cdf[A - 1]
 *              (searchsorted side='right'), A - 1 if there is none;  the first child with that action is played.
 *   identity   a row w[n] = n with offset 0 and no cutoff makes every intermediate the sampler's own (integer sums are exact in float64): the
 *              table {0, .., 0 (sample_until entries), -1} plays the games of an engine without the option.
 *   unchanged  what is recorded as pi (traj_pi, the asynchronous record ring, azk_root_stats, azk_root_policy_target): raw visits, pruned
 *              where a forced search prunes them - KataGo's and Leela's convention, not AlphaGo Zero's tempered target.  Surprise kl, q,
 *              resignation, pruning and the played-child note of tree reuse work on whatever cell was chosen.
 *   stats      four counters since azk_set_move_temperature: plies chosen by the weighted path, those among them whose played child is
 *              not b, children cut by the value cutoff, plies that fell back because S == 0.
 * azk_set_move_temperature takes HOST pointers, copies both tables to device memory (tables of their own per call; nothing is allocated
 * while the option was never set) and zeroes the stats.  AZK_ERR_ARG: a null table, n_plies < 1 or n_rows < 1, n_cols != max_sims + 1, a row
 * index outside [-1, n_rows), a weight that is negative, NaN or infinite, weights[r][0] != 0 (an unvisited child is never played), a row
 * without a positive weight, a weight above DBL_MAX / (n_rows * n_cols) (S must stay finite), visit_offset < 0, a NaN cutoff.
 * AZK_ERR_STATE: between the begin of a search and the call that ends it (a move, new positions or a reset); after azk_async_begin; with a
 * Gumbel root set (its arg-max is the sample) - azk_set_gumbel_root refuses likewise while the option is set; on an engine created with
 * tree_reuse = 1 (a carried root child's visits are not bounded by max_sims, so the table has no column for them; top-up, tree_reuse = 2, is
 * bounded and allowed).  azk_clear_move_temperature makes the engine launch what it launched before (AZK_ERR_STATE after azk_async_begin).
 * azk_get_move_temperature_stats copies the four counters to out4_host and waits (AZK_ERR_STATE while the option is off).  Combines with a
 * playout cap, resignation, forced playouts, surprise weighting, configurable PUCT, evaluation symmetry, emit_elements, random openings,
 * top-up tree reuse and the asynchronous movers with and without top-up re-rooting. */
int32_t azk_set_move_temperature(azk_engine *e, const int32_t *row_of_ply_host, int32_t n_plies, const double *weights_host, int32_t n_rows,
                                 int32_t n_cols, int32_t visit_offset, double value_cutoff, void *stream);
int32_t azk_clear_move_temperature(azk_engine *e);
int32_t azk_get_move_temperature_stats(azk_engine *e, int64_t *out4_host, void *stream);

/* ---- value targets: the outcome blended with the game's own search values at emission (OPT-IN; off, the engine launches exactly the
 * kernels it launched before).  azk_emit_finished and azk_async_drain otherwise write z = +1 / -1 / 0 by the final winner into every tuple
 * of a game.  With the option the movers (azk_advance*, the asynchronous movers) keep q = W[root] / (double)N[root] of every move beside
 * its pi - the expression of azk_root_stats, the asynchronous record's q and resignation: the value for the OPPONENT of the side to move -
 * and emission writes a target t in place of z, all float64.  For a finished game of n plies whose first searched ply
 * is o (its opening plies with random openings, else 0), and i = o .. n - 1:
 *   v_i = -q_i                                     the mover's own search value
 *   z_i = +1 / -1 / 0                              what emission writes without the option: the final winner from ply i's mover's view
 *   G_{n-1} = (1 - lam) * v_{n-1} + lam * z_{n-1}
 *   G_i     = (1 - lam) * v_i + lam * (-G_{i+1})   from the last ply down; the side to move alternates, hence the sign
 *   t_i     = (1 - r) * z_i + r * G_i              written to zs as (float)t_i
 * r in [0, 1] is the weight of the search-based part, lam in [0, 1] its horizon: (r, 0) is Leela's q-ratio, (1, lam) a TD(lambda) return
 * over search values that ends in z, and (0, any lam) and (1, 1) write today's ring byte for byte (a draw keeps +0.0).  Every searched ply
 * takes part in the recurrence, a capped engine's fast plies too; opening plies had no search and are never reached.  Every tuple of a ply -
 * each element of its group, each copy under surprise weighting - carries the same target; states and pis do not change.  With tree reuse
 * and re-rooting q is the carried root's W / N as it stands; a resigned game is an ordinary finished game.
 * azk_set_value_target allocates the two [n_games][state_dim] float64 arrays on first use and zero-fills them.  AZK_ERR_ARG: r or lam NaN or
 * outside [0, 1]; an engine that records no trajectories; leaves_per_step > 1 (a virtual-loss search is another search).  AZK_ERR_STATE:
 * after azk_async_begin; with a Gumbel root set (its movers do not keep q) - azk_set_gumbel_root refuses likewise while the option is set.
 * azk_clear_value_target makes the engine launch what it launched before (AZK_ERR_STATE after azk_async_begin).  azk_get_value_record
 * copies the q of the current games' plies, float64 [n_games][state_dim], to q_out_dev on the stream: row g holds game g's plies up to its
 * move count, older entries are what earlier games in the slot left (AZK_ERR_STATE while the option is off). */
int32_t azk_set_value_target(azk_engine *e, double r, double lam, void *stream);
int32_t azk_clear_value_target(azk_engine *e);
int32_t azk_get_value_record(azk_engine *e, double *q_out_dev, void *stream);

/* ---- random openings (OPT-IN; off, the engine launches exactly the kernels it launched before).  Every game otherwise starts from the
 * empty board and differs from its neighbours only through root noise and move sampling; with the option a game that starts in slot g is,
 * with probability p_open, played forward 1..max_plies uniformly drawn legal plies inside a centred window before its first search (KataGo's
 * and Leela's game initialisation).  The plies are drawn on the device, where the game is born - a recycled slot and an asynchronous restart
 * never pass through the host - from a stateless key.  DESIGN section 25.
 *   the key     gg = first_global_game + g and key = the move key of the game's first search: the lock-step move index (azk_open_pending's
 *               argument), the slot's move counter in the asynchronous movers - the key of its noise row and of its resignation coin.
 *   game draw   Philox4x32-10, key (seed lo, seed hi), counter {gg lo, gg hi, key, 0xFFFFFFFA}: c0 from words (0, 1), c1 from (2, 3), each
 *               ((hi << 32 | lo) >> 11) * 2^-53.  The game is opened iff c0 < p_open, with n = min(1 + floor(c1 * max_plies), max_plies) plies.
 *               Word 3 = 0xFFFFFFFA belongs to no other draw (0xFFFFFFFF..FC: move uniform and the option coins, ..FB: Gumbel rows; noise rows:
 *               it < 64 and it | 0x40000000), so every other stream is what it was.
 *   ply j < n   counter {gg lo, gg hi ^ ((j + 1) << 8), key, 0xFFFFFFFA}, u from words (0, 1) (j + 1 <= 400, global game index below 2^40: the
 *               noise rows' bound).  Candidates: the legal actions inside the window, ascending by action index - cell (r, c) is inside iff
 *               spread < 0, or |2r - (rows - 1)| <= 2 spread and |2c - (cols - 1)| <= 2 spread; Connect4's candidates are the columns that are
 *               not full and meet the column condition, and the stone lands where the engine's rule puts it.  With m candidates the side to
 *               move plays candidate min(floor(u * m), m - 1) (float64).  m == 0 ends the opening.  A ply after which the engine's winner rule
 *               decides the game, or the board is full, is taken back and ends the opening ("cut short"): an opened position is never
 *               terminal and always has a legal move.
 *   the plies   are ordinary plies - cells, side to move, ply count and the trajectory's actions are written - without a search: no pi, no q,
 *               no record, and azk_emit_finished / azk_async_drain leave them out exactly as a playout cap leaves out fast plies (no tuples,
 *               not in the surprise weights' n and S, 0 copies; the group size stays keyed on the absolute ply index; boards are rebuilt from
 *               ply 0).  The plies of finished games that azk_recycle_finished and stats_dev [1] count include them; moves played do not.
 *               Resignation needs nothing: its game coin is keyed by (move counter - plies), constant over the game, and min_ply counts all plies.
 *   statistics  int64 [3]: [0] games opened, [1] opening plies played, [2] openings cut short.
 * azk_set_openings: 0 <= p_open <= 1 (0 is a live setting: every game is looked at and none is opened), 1 <= max_plies <= state_dim - 1,
 * spread = -1 or >= 0, else AZK_ERR_ARG; allocates on first use, zeroes the statistics and flags every slot, so that the next
 * azk_open_pending (or azk_async_begin) opens the games that have not started yet (ply count 0, not finished).  Call it before
 * azk_async_begin(_reuse); seed and first_global_game are the option's own in both drivers.  azk_clear_openings switches the option off.
 * azk_open_pending(key): lock-step drivers call it after the games were created or reset (key 0) and after azk_recycle_finished (key = the
 * move index of the search that follows), outside any captured graph; one wave per slot, a slot whose game did not just start ends after
 * one load.  azk_reset_games and azk_recycle_finished flag the slots they restart.  The asynchronous movers open a restarted game inside
 * the drain's restart kernel and the first games inside azk_async_begin; azk_open_pending answers AZK_ERR_STATE there.
 * azk_get_open_plies: int32 [G] into device memory, the opening plies of each slot's current game (0: not opened).
 * azk_get_opening_actions: int16 [G][state_dim] into device memory, row g = the cells the opening of slot g's current game was played on, in
 * order; entries from azk_get_open_plies' count on are not defined.
 * azk_get_opening_stats: the three counts into host memory; synchronises.
 * azk_get_leaf_flags (any engine): uint8 [G * leaves_per_step] into device memory, non-zero = the slot contributes a row to the evaluator batch
 * of the step that has just selected; the rows are in ascending slot order.  It is how a host loop whose games are not all at the same ply
 * (an arena between two models on opened games) tells which game a row belongs to. */
int32_t azk_set_openings(azk_engine *e, double p_open, int32_t max_plies, int32_t spread, uint64_t seed, int64_t first_global_game, void *stream);
int32_t azk_clear_openings(azk_engine *e);
int32_t azk_open_pending(azk_engine *e, int32_t key, void *stream);
int32_t azk_get_open_plies(azk_engine *e, int32_t *open_plies_dev, void *stream);
int32_t azk_get_opening_actions(azk_engine *e, int16_t *actions_dev, void *stream);
int32_t azk_get_opening_stats(azk_engine *e, int64_t *out3_host, void *stream);
int32_t azk_get_leaf_flags(azk_engine *e, uint8_t *flags_dev, void *stream);

/* One simulation per active game (ai/mcts.py:16-60), split around the evaluator:
 *   azk_step_select   - mcts.py:18-37: PUCT walk (node.py:42-47, utils.py:29-44), make_move along the
 *                       path, terminal test + immediate backup, get_valid_moves, canonical board.
 *                       Non-terminal leaves are compacted (ascending game index) into
 *                       leaf_boards_dev [n_leaf][F][R][C]; *n_leaf_dev (int32) gets the count.
 *   azk_step_expand_backup - mcts.py:46-60: float32 softmax without max subtraction, root noise
 *                       mixing (utils.py:12-27), Node.expand (node.py:50-59), Node.backup (node.py:62-74)
 *                       with value = -v.  logits_dev float32 [n_leaf][A], values_dev float32 [n_leaf],
 *                       rows in the slot order azk_step_select produced.
 * azk_step fuses "expand+backup of the previous step's leaves" with "select of the next" in one launch
 * (pass logits_dev = NULL on the first step of a search). */
int32_t azk_step_select(azk_engine *e, void *leaf_boards_dev, int32_t *n_leaf_dev, void *stream);
int32_t azk_step_expand_backup(azk_engine *e, const float *logits_dev, const float *values_dev, void *stream);
int32_t azk_step(azk_engine *e, const float *logits_dev, const float *values_dev,
                 void *leaf_boards_dev, int32_t *n_leaf_dev, void *stream);

/* The two launches azk_step is made of, separately (per-kernel timing; also lets the caller overlap):
 *   azk_step_tree   - k_tree: expand+backup of the pending leaves (logits_dev != NULL) then PUCT select
 *   azk_step_gather - k_gather: leaf compaction + canonical boards into the evaluator batch */
int32_t azk_step_tree(azk_engine *e, const float *logits_dev, const float *values_dev, void *stream);
int32_t azk_step_gather(azk_engine *e, void *leaf_boards_dev, int32_t *n_leaf_dev, void *stream);

/* Continuous self-play (the batched form of train.collect_data's `for iter in range(iterations): game = Game()`,
 * train.py:63-65): every finished game's slot restarts from an empty board.  stats_dev int64[8] accumulates
 * [0] games finished, [1] their total plies (the plies of a random opening included, azk_set_openings), [2] wins of player 0,
 * [3] wins of player 1, [4] draws. */
int32_t azk_recycle_finished(azk_engine *e, int64_t *stats_dev, void *stream);

/* (state, pi, z) emission for every game that has just finished (train.save_data_to_buffer, train.py:30-49, with the D4
 * augmentation of rotate_data / flip_data, train.py:8-27).  Call after azk_advance and before azk_recycle_finished.
 * Position i of the game (side to move i & 1): state = canonical board float32 [F][R][C], pi float64 [A] as recorded by
 * azk_advance, z = +1 / -1 / 0; positions 0 and 1 once, the rest 8 times in the reference's order (rot0, lr, tb, rot90,
 * lr, tb, rot180, rot270).  The engine appends at *cursor_dev (uint64, monotonically increasing) and writes tuple t to
 * slot t % capacity of the caller's ring buffers - the device-resident form of ReplayBuffer's deque(maxlen)
 * (replay_buffer.py:7-13).  game_base_dev (optional, int64 [G]) receives each emitted game's first tuple index, -1 for
 * the others.  Square boards with one action per cell only (Gomoku, TicTacToe); others return AZK_ERR_ARG - unless the engine was
 * created with azk_config.emit_elements = m != 0 (OPT-IN; 0: everything above, bit for bit).  Then, on every geometry, with
 * n = popcount(m):
 *   - a finished game of p plies reserves  p <= 2 ? p : 2 + n * (p - 2)  tuples; plies 0 and 1 once, under element 0, as ever;
 *   - ply i >= 2 gets one tuple per element of m, in ascending element order, at base + 2 + n * (i - 2);
 *   - the tuple for element s: every plane of the canonical board turned, out[j] = in[src_s(j)] on the R x C board (src_s as
 *     azk_set_eval_symmetry defines it); the side plane (F == 3) is the constant it was; with one action per cell
 *     pi'[j] = pi[src_s(j)], with Connect4's column actions pi'[a] = pi[cols - 1 - a] under element 1; z is unchanged;
 *   - on a playout-cap engine the group of a full ply is  i < 2 ? 1 : n; fast plies are left out, offsets are the sum over the full
 *     plies before;
 *   - the ring slot t % capacity, the 64-bit cursor, game_base_dev, the asynchronous drain, resignation's winner and the pruned pi of
 *     forced playouts are what they are without the option.
 * On a square board m = 0xFF fills the ring of an engine with the option off, byte for byte; m = 0x01 stores one image per position
 * (for a caller that turns the batch when it is drawn: azk_replay_gather).
 * azk_emit_elements: *mask_out = the engine's azk_config.emit_elements, *group_out = the tuples per ply from the third on - popcount of
 * the mask; with the option off 8 on a board the reference's rule emits, 0 where emission answers AZK_ERR_ARG - to size a ring by. */
int32_t azk_emit_finished(azk_engine *e, float *states_dev, double *pis_dev, float *zs_dev, int64_t capacity,
                          int64_t *cursor_dev, int64_t *game_base_dev, void *stream);
int32_t azk_emit_elements(const azk_engine *e, int32_t *mask_out, int32_t *group_out);

/* A training batch gathered from a replay ring, each row turned by a D4 element drawn for it (stateless; no engine).  The ring is the
 * caller's: states_ring float32 [rows_ring][planes][rows][cols], pis_ring float64 [rows_ring][action_dim], zs_ring float32 [rows_ring]
 * (azk_emit_finished's layout).  Row b of the output (b < n) comes from ring row r = idx_dev[b] (int64; the caller guarantees
 * 0 <= r < rows_ring) under element
 *     draws_dev == NULL ? 0 : valid[(((uint32_t)draws_dev[b] >> 16) * n_valid) >> 16]
 * with valid = the elements of element_mask in ascending order (the pick of azk_set_eval_symmetry's mode 1):
 *     states_out[b] = every plane turned, out[j] = in[src_s(j)];   zs_out[b] = zs_ring[r];
 *     pis_out[b]    = the float64 row turned as azk_emit_finished turns it, rounded to float32 (round to nearest even).
 * With draws_dev == NULL that is  states[idx], pis[idx].float(), zs[idx]  exactly.  The action kind follows from action_dim:
 * rows * cols = one action per cell (all eight elements where rows == cols, else {0, 1, 2, 6}); cols = column actions, {0, 1} with pi
 * mirrored; anything else: element 0 only.  AZK_ERR_ARG (message: azk_last_error(NULL)) for a mask without bit 0 or with bits above 7,
 * an element the geometry and action kind do not admit (a transposing one with rows != cols), rows * cols > 400 or a dimension < 1
 * (any rows x cols inside that: the engine's limit of 30 columns does not apply here, 1 x 400 is a board),
 * n < 0, a null pointer; n == 0 does nothing.  One wave per output row; asynchronous on the stream. */
int32_t azk_replay_gather(int32_t rows, int32_t cols, int32_t planes, int32_t action_dim, uint32_t element_mask,
                          const float *states_ring, const double *pis_ring, const float *zs_ring,
                          const int64_t *idx_dev, const int32_t *draws_dev, int32_t n,
                          float *states_out, float *pis_out, float *zs_out, void *stream);

/* MCTS.cache.clear() (main.py:55-57): must be called whenever the evaluator's weights change. */
int32_t azk_clear_cache(azk_engine *e, void *stream);

/* Root statistics after a search, for all G games (device outputs, any may be NULL):
 *   pi_dev float64 [G][A]   utils.get_probablity_distribution_of_children (utils.py:46-55)
 *   q_dev  float64 [G]      root.value / root.visit (gomoku.py:140)
 *   root_visit_dev int32 [G] */
int32_t azk_root_stats(azk_engine *e, double *pi_dev, double *q_dev, int32_t *root_visit_dev, void *stream);

/* Root children of ONE game, in the reference's list order (what callers read from root.children:
 * child.prevAction / visit / value / prior, test.py:46-47, node.py:76-97).  Host outputs of
 * capacity `cap` each; returns the child count (>= 0) or an error.  Synchronises the stream. */
int32_t azk_root_children(azk_engine *e, int32_t game, int32_t cap, int32_t *cells_host,
                          int32_t *visits_host, double *values_host, double *priors_host, void *stream);
/* Whole tree of one game, DFS pre-order with children in list order (for digests / Node views).
 * Returns the node count (may exceed cap: only the first cap rows are written).  Synchronises. */
int32_t azk_export_tree(azk_engine *e, int32_t game, int32_t cap, int32_t *depth_host, int32_t *cell_host,
                        int32_t *visit_host, double *value_host, double *prior_host, void *stream);
/* The same rows with one more column (any output may be NULL): quotient_host[m] = the node's word of the engine's quotient column, which
 * holds value / visit (IEEE float64 division of the two numbers azk_export_tree reports) bit for bit for every node with visit > 0 - the
 * search keeps it at backup and the walk reads it instead of dividing.  For a node with visit == 0 the word is unspecified (whatever the
 * memory held) and nothing reads it. */
int32_t azk_export_tree_quotients(azk_engine *e, int32_t game, int32_t cap, int32_t *depth_host, int32_t *cell_host,
                                  int32_t *visit_host, double *value_host, double *prior_host, double *quotient_host, void *stream);
/* Debug / tests only: every byte of the quotient column of every game becomes `byte` (0: +0.0 everywhere, 255: a NaN everywhere).  It
 * breaks the column for visited nodes, so it is for engines whose trees are fresh roots (after azk_create / azk_reset_games, before the
 * first search, no tree reuse pending): a search that follows must come out the same whatever was filled in.  Asynchronous on the stream. */
int32_t azk_debug_fill_quotients(azk_engine *e, int32_t byte, void *stream);

/* Move selection + state advance for all active games (gomoku.py:143-162; a tree_reuse engine also notes the played child as the
 * next search's root - forgotten again by azk_reset_games, azk_set_positions, azk_recycle_finished and for finished games):
 *   game g samples ~ visits when move_count[g] < sample_until_move (Node.sample_child, node.py:83-93:
 *   legacy np.random.choice == searchsorted(cumsum(pi)/sum, u, 'right') with u = uniforms_dev[g]),
 *   else takes the first child with the most visits (Node.max_visit_child, node.py:76-81);
 *   then make_move, check_winner for the mover, draw when move_count == state_dim.
 * Outputs (device, may be NULL): chosen_cell_dev int32 [G] (r*cols+c, -1 for finished games),
 * winner_dev int32 [G] (-2 still running, -1 draw, 0/1 winner), done_dev int32 [G]. */
int32_t azk_advance(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move,
                    int32_t *chosen_cell_dev, int32_t *winner_dev, int32_t *done_dev, void *stream);

/* current boards as int8 cells [G][rows*cols], side to move [G], plies [G] (host outputs; synchronises) */
int32_t azk_get_positions(azk_engine *e, int8_t *cells_host, int32_t *to_move_host, int32_t *move_count_host, void *stream);

int32_t azk_get_counters(azk_engine *e, azk_counters *out, void *stream);   /* synchronises */
int32_t azk_reset_counters(azk_engine *e, void *stream);
/* debug only: per-phase shader-clock sums of k_tree (collected when AZK_TREE_ABLATE has bit 16): expand, board+root
 * load, walk, terminal test, valid moves, writes (cycles), then summed depth and sample count.  Synchronises. */
int32_t azk_debug_stamps(azk_engine *e, int64_t *out8_host);
/* debug only: the raw [n_games][8] stamp records (AZK_TREE_ABLATE bit 8192: one record per wave of the LAST k_tree launch - cycles of
 * expansion, walk, terminal test, legal moves, leaf writes + cache probe; depth; kind + 1 | legal moves << 8 | children created << 20;
 * the wave's whole life).  Synchronises. */
int32_t azk_debug_stamps_raw(azk_engine *e, int64_t *out_host, int32_t n_games);
/* sticky device-side error word (arena overflow etc.); synchronises; returns AZK_OK or the error */
int32_t azk_check_device_error(azk_engine *e, void *stream);

/* Dirichlet(alpha) rows and uniforms from a counter-based generator keyed by
 * (seed, global game index, move index) - results do not depend on how games are sharded over GPUs.
 * noise_dev float64 [count][A]; uniforms_dev float64 [count] (either may be NULL).
 * Philox4x32-10, key (seed lo, seed hi); the uniform's counter is {game lo, game hi, move, 0xFFFFFFFF}, entry a's tries it = 0..63 draw
 * from {game lo, game hi ^ (a << 8), move, it} and it | 0x40000000.  A <= 400 keeps the action index in bits 8..16 of word 1, so the
 * streams of distinct (game, action) pairs are distinct for global game indices below 2^40, and word 3 keeps the uniform and the
 * playout-cap coin out of every row's draws (tests/rng_restated.py restates the whole chain in float64). */
int32_t azk_gen_noise(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double alpha,
                      double *noise_dev, double *uniforms_dev, void *stream);

/* ---- OPT-IN root noise on the legal moves ----
 * azk_gen_noise keeps the reference's law: utils.add_dirichlet_noise is handed the whole softmax vector (mcts.py:43,53), so a row is
 * Dirichlet(alpha) over all A = action_dim entries and only the part that falls on the root's children acts.  With this option a search's row
 * is drawn over the actions that are legal in the position the search starts from - exactly the children its root gets:
 *   L           TicTacToe: the empty cells; Connect4: the columns that are not full; Gomoku: the empty cells next to a stone, the centre cell
 *               (rows / 2, cols / 2) where there is none (get_valid_moves as a set).  n = |L|.
 *   alpha_eff   alpha (mode 1, "legal") or alpha / n (mode 2, "total": the row's total concentration stays alpha whatever n is)
 *   a in L      gam[a] = the Gamma(alpha_eff) draw of azk_gen_noise's recipe at azk_gen_noise's counters for entry a - Philox4x32-10, key
 *               (seed lo, seed hi), tries it = 0..63 from {game lo, game hi ^ (a << 8), move key, it} and it | 0x40000000 -, and
 *               row[a] = gam[a] / sum over L of gam, or 1 / n where that sum is 0.  n == 1 gives exactly 1.0.
 *   a not in L  row[a] = +0.0.  (A full TicTacToe or Connect4 board - a finished game that waits in the batch - has n == 0: a row of zeros.)
 * In mode 1 the row is azk_gen_noise's row of the same (seed, game, move key, alpha) restricted to L and renormalised, from the same Philox
 * blocks; no new word-3 tag exists and the move uniform (word 3 = 0xFFFFFFFF) is what it was.  A row depends on (seed, global game, move key,
 * position) only - not on the engine's game count or on sharding.  The root mix (0.75 prior + 0.25 row, k_tree and the re-rooting kernels) is
 * not part of the option: it reads a row that was made differently.
 * azk_set_root_noise: mode 1 | 2 and a finite alpha > 0, else AZK_ERR_ARG; AZK_ERR_STATE with a Gumbel root set (and azk_set_gumbel_root
 * with this option set), after azk_async_begin(_reuse), and between a search's begin and its move.  azk_clear_root_noise switches it off.
 * azk_gen_root_noise (lock-step): azk_gen_noise's buffers and NULL conventions, its uniforms bit for bit, the rows from the engine's cells as
 * they stand: call it after azk_open_pending / azk_advance and before azk_begin_search*; one wave per game.  AZK_ERR_STATE without the option.
 * The asynchronous movers: while the option is set its alpha replaces azk_async_config.alpha, no row is made a search ahead (the position is
 * not known then), and the row of a game whose move key has moved is made from its position - behind the movers in every azk_async_step
 * (engines that do not re-root), and in azk_async_drain behind the restart of finished games and in front of the re-rooting of parked ones.
 * azk_get_root_noise: float64 [G][A] into device memory, the row each game's current search reads (an asynchronous engine: row
 * (move counter & 1) of the game's pair); AZK_ERR_STATE before the first search with rows. */
int32_t azk_set_root_noise(azk_engine *e, int32_t mode, double alpha, void *stream);
int32_t azk_clear_root_noise(azk_engine *e);
int32_t azk_gen_root_noise(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *noise_dev, double *uniforms_dev,
                           void *stream);
int32_t azk_get_root_noise(azk_engine *e, double *rows_dev, void *stream);

/* ---- adaptive search budgets: a search ends when its root stops changing (OPT-IN; off, the engine launches exactly the kernels it launched
 * before).  The reference runs a fixed number of simulations whether the position is a forced recapture or a real decision.  With the option a
 * search runs in SEGMENTS of `interval` simulations and, between two segments, compares the root's visit distribution with the one a segment
 * earlier: once the KL divergence gained per simulation falls below min_gain the game moves (Lc0's KLD-gain stopper, minimum-kldgain-per-node
 * and kldgain-average-interval).  k_tree does not change: a segment is a preset of sims_done, the word budget stepping
 * already counts a game's simulations in, so a checkpoint is a point where the game looks complete to the mover.  All arithmetic is float64.
 *   state      interval I, 1 <= I <= max_sims;  min_gain, finite and > 0;  min_sims >= 0.  Per game: left, run, the snapshot o (int32 per root
 *              child, list order) and its sum So.
 *   arming     wherever a search begins - azk_begin_search_budget / _capped on a fresh root or a re-rooted one, azk_async_begin, the
 *              asynchronous mover's own next search, the drain's restarted, opened and re-rooted games - behind the begin code's own write of
 *              sims_done, for every game that is not done:  T = budget - sims_done  is the search's own allowance of new simulations (n_sims,
 *              or the playout cap's target, or top-up's n_new);  seg = min(I, T);  sims_done = budget - seg;  left = T - seg;  run = seg;
 *              So = 0 (no snapshot).
 *   checkpoint a game that is not done, with sims_done >= budget and no pending leaf (the asynchronous movers' test).  n_i = the root
 *              children's N in list order, S = their sum.
 *                1  left == 0: the search is over, it ran its allowance.
 *                2  otherwise, if So > 0 and run >= min_sims:  gain = sum over i with o_i > 0 of  po_i * log(po_i / pn_i),
 *                   po_i = (double)o_i / (double)So,  pn_i = (double)n_i / (double)S - each lane sums its children i, i + 64, ... in list
 *                   order, then the xor butterfly 32 ... 1 combines the lanes (surprise weighting's convention);
 *                   rate = gain / (double)(S - So);  rate < min_gain: the search is over, it ended early with `left` simulations unrun.
 *                3  otherwise the game is RELEASED:  o = n, So = S;  seg = min(I, left);  sims_done = budget - seg;  left -= seg;  run += seg;
 *                   nothing else about the game changes.
 *   hence      a search that is over is moved exactly as without the option, on the tree as it stands: pi, q, resignation, policy target
 *              pruning, surprise kl, the temperature table, the value record and re-rooting read the root as it is.  The tree at every
 *              checkpoint is the tree a plain search of `run` simulations holds, and with a min_gain so small that it never fires the games
 *              are the option-off games bit for bit.
 *   zero       a rate of exactly 0 - a root with one child (Gomoku's empty board), or visits that grew in exact proportion - is below every
 *              positive min_gain: such a search ends at its first judged checkpoint, a forced move moving early; min_sims holds it back.
 * azk_set_kld_stop allocates left, run, the checkpoint count, So (int32 [G] each), the snapshot (int32 [G][cells]), the last rate (float64 [G])
 * and four counters on first use and clears them (nothing is allocated, and no new kernel is launched, while the option was never set);
 * azk_clear_kld_stop makes the engine launch what it launched before.  AZK_ERR_ARG: a parameter out of range, or an engine with
 * leaves_per_step > 1.  AZK_ERR_STATE: with a Gumbel root set (its halving table needs a fixed n; azk_set_gumbel_root refuses likewise while
 * this option is set); between the begin of a search and the call that ends it; after azk_async_begin; and, while the option is set,
 * azk_begin_search (plain stepping), azk_vanilla_search and azk_async_set_budget (the running searches' segments are cut against the budget
 * as it stood).  Combines with everything else: playout cap, resignation, forced playouts, surprise weighting, configurable PUCT, the solver,
 * a move temperature, value targets, openings, both kinds of root noise, evaluation symmetry, the eval cache and both tree-reuse modes.
 * Lock-step drivers: begin with azk_begin_search_budget / _capped, step until azk_search_unfinished reports 0, run the closing
 * azk_step_expand_backup where the eval cache needs one, then azk_kld_checkpoint - one wave per game judges every game at a checkpoint and
 * *released_host is the number of games released - and step on while it released a game; then move.  Waits, like azk_search_unfinished.
 * AZK_ERR_STATE while the option is off or after azk_async_begin.  The asynchronous movers judge a game themselves, behind their "search
 * complete" test and in front of the move; nothing is launched that an azk_async_step did not launch before, the drain arms the searches it
 * begins with one small launch per list.
 * azk_get_search_sims: int32 [G] into device memory, the new simulations each game's current or last-judged search has run once its current
 * segment is complete (`run`).  azk_get_kld_rate: float64 [G] into device memory, the rate of each game's last judged checkpoint (0 before
 * the first).  azk_get_kld_stats: out4_host int64 [4] since azk_set_kld_stop - checkpoints judged (step 2 reached), searches ended early,
 * simulations those searches left unrun, searches that ran their allowance; waits.  azk_async_sims_column (optional, before azk_async_begin):
 * an int32 [record_capacity] column of the record ring, entry r % capacity = `run` of the record's search.  All AZK_ERR_STATE while the option
 * is off. */
int32_t azk_set_kld_stop(azk_engine *e, int32_t interval, double min_gain, int32_t min_sims, void *stream);
int32_t azk_clear_kld_stop(azk_engine *e);
int32_t azk_kld_checkpoint(azk_engine *e, int32_t *released_host, void *stream);
int32_t azk_get_search_sims(azk_engine *e, int32_t *sims_dev, void *stream);
int32_t azk_get_kld_rate(azk_engine *e, double *rate_dev, void *stream);
int32_t azk_get_kld_stats(azk_engine *e, int64_t *out4_host, void *stream);
int32_t azk_async_sims_column(azk_engine *e, int32_t *rec_sims_dev);

/* ---- adaptive search budgets, the second rule: a search ends once the runner-up cannot catch up (OPT-IN; off, the engine launches exactly the
 * kernels it launched before).  Smart pruning's stop as Lc0 ships it beside the KLD stopper: the search is over once the most-visited root child
 * leads the second by more than the simulations that are left.  Segments, arming and the checkpoint's place are the KLD
 * rule's above, unchanged; the two rules are set apart or together and share the kernels (k_kld_arm, k_kld_checkpoint, k_move_async_kld).
 *   state      interval I, 1 <= I <= max_sims;  factor f, finite and > 0;  min_sims >= 0.  Per game: left, run (as above) and three int32
 *              words, N1, N2 and left at the last judged lead checkpoint.
 *   arming     as above:  T = budget - sims_done;  seg = min(I, T);  sims_done = budget - seg;  left = T - seg;  run = seg.
 *   checkpoint a game that is not done, with sims_done >= budget and no pending leaf.  n_i = the root children's N, nch their number.
 *                1  left == 0: the search is over, it ran its allowance.
 *                2  otherwise, if run >= min_sims (the checkpoint is JUDGED):
 *                     nch == 1: the search is over - a forced move, counted as such (not as ended early);
 *                     otherwise N1 = max n_i and N2 = the second largest COUNTING MULTIPLICITY (a tie for the maximum gives N2 = N1; each lane
 *                     keeps a (max, second) pair over its children i, i + 64, ..., the xor butterfly 32 ... 1 merges two pairs into the larger
 *                     max and the largest of the smaller max and both seconds; no child index is kept);  lead = N1 - N2;  the search is over,
 *                     ended early with `left` simulations unrun, iff  (double)left < f * (double)lead  - one float64 multiply and one
 *                     compare of exactly converted integers, so host and device agree bit for bit and no margin is needed.
 *                     The three words are written: N1, N2 (0 for a single child), left.
 *                3  otherwise the game is RELEASED:  seg = min(I, left);  sims_done = budget - seg;  left -= seg;  run += seg.
 *   hence      a search that is over is moved on the tree as it stands, as under the KLD rule: pi, q, resignation, pruning, surprise kl, the
 *              temperature table, value records and re-rooting read the root as it is; the tree at every checkpoint is the tree a plain
 *              search of `run` simulations holds.
 *   exactness  every simulation adds one visit to exactly one root child.  At f = 1, left < N1 - N2 means that no child can reach N1 in the
 *              simulations left: the holder of N1 is unique and stays the strict maximum, so the FIRST MOST-VISITED child of the stopped
 *              search is that of the full search, and greedy play is move for move what it was.  This holds on carried roots: `left` counts
 *              new simulations, n_i includes carried visits.  (pi, q and a sampled move are those of the shorter search.)
 *   both rules they share the one interval: azk_set_lead_stop and azk_set_kld_stop refuse (AZK_ERR_STATE) an interval that differs from the
 *              other rule's.  At a checkpoint the lead rule is judged first, each rule under its own min_sims; the search ends if either
 *              fires; if neither does the KLD snapshot is taken as above.  With the KLD rule off the judge touches neither the snapshot, its
 *              sum nor the rate - they are not allocated - and executes no log.
 * azk_set_lead_stop allocates on first use and clears the three words and the five counters (and left / run / the checkpoint count: no search
 * is armed); azk_clear_lead_stop switches the rule off.  The refusals are azk_set_kld_stop's: AZK_ERR_ARG for a parameter out of range or an
 * engine with leaves_per_step > 1; AZK_ERR_STATE with a Gumbel root set (azk_set_gumbel_root refuses in turn), inside a search, after
 * azk_async_begin, for the interval mismatch, and - while the rule is set - from azk_begin_search, azk_vanilla_search and azk_async_set_budget.
 * While either rule is set azk_kld_checkpoint, azk_get_search_sims and azk_async_sims_column work as described above; azk_get_kld_rate and
 * azk_get_kld_stats need the KLD rule.
 * azk_get_lead: int32 [G][3] into device memory, the three words.  azk_get_lead_stats: out5_host int64 [5] since azk_set_lead_stop -
 * checkpoints judged, searches ended early, simulations those left unrun, forced-move ends, searches that ran their allowance; waits.  Both
 * AZK_ERR_STATE while the lead rule is off. */
int32_t azk_set_lead_stop(azk_engine *e, int32_t interval, double factor, int32_t min_sims, void *stream);
int32_t azk_clear_lead_stop(azk_engine *e);
int32_t azk_get_lead(azk_engine *e, int32_t *lead_dev, void *stream);
int32_t azk_get_lead_stats(azk_engine *e, int64_t *out5_host, void *stream);

/* ---- stateless board-rule kernels over caller boards (float32 [n][F][R][C], the reference's layout) ----
 * game/rows/cols as in azk_config.  These replace the Game statics (games/game.py:4-38):
 *   azk_rules_legal_moves : get_valid_moves - cells in the reference's LIST ORDER (tictactoe.py:82-83,
 *                           connect4.py:44-53, gomoku.py:93-106 incl. CPython set order), moves_dev int16 [n][R*C],
 *                           counts_dev int32 [n]
 *   azk_rules_legal_mask  : same set as a uint8 mask over ACTIONS [n][A]
 *   azk_rules_apply_move  : make_move (returns next player; occupied cell => unchanged player, tictactoe.py:37-45,
 *                           gomoku.py:51-58; connect4.py:56-63 never checks)
 *   azk_rules_undo_move   : undo_move (tictactoe.py:48-51, connect4.py:67-70, gomoku.py:61-63)
 *   azk_rules_check_winner: check_winner (k-in-a-row through the cell; player or -1)
 *   azk_rules_canonical   : get_canonical_board (gomoku.py:34-40; 3-plane: mcts.py:126-137) */
int32_t azk_rules_legal_moves(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                              int16_t *moves_dev, int32_t *counts_dev, void *stream);
int32_t azk_rules_legal_mask(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                             uint8_t *mask_dev, void *stream);
int32_t azk_rules_apply_move(int32_t game, int32_t rows, int32_t cols, float *boards_dev, int32_t n,
                             const int32_t *players_dev, const int32_t *cells_dev, int32_t *next_player_dev, void *stream);
int32_t azk_rules_undo_move(int32_t game, int32_t rows, int32_t cols, float *boards_dev, int32_t n,
                            const int32_t *current_players_dev, const int32_t *cells_dev, void *stream);
int32_t azk_rules_check_winner(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                               const int32_t *players_dev, const int32_t *cells_dev, int32_t *winners_dev, void *stream);
int32_t azk_rules_canonical(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                            const int32_t *players_dev, float *out_dev, void *stream);

/* ---- policy-value network: token embedding on the matrix cores (ai/nn.py:5-36) ------------------------------
 * tokens[b,0,:] = cls + pos[0];  tokens[b,1+j,:] = Conv2d(C->D, k x k, stride 1, pad k/2)(board)[:, j] + pos[1+j]
 * as an im2col GEMM on the matrix cores (fp32 accumulate), epilogue fused: + bias + positional embedding,
 * and optionally the first block's LayerNorm (nn.py:53, eps 1e-5) so the block's Q/K/V GEMM reads xhat directly.
 *   boards_dev        [n][C][R][Cc] bf16 (boards_are_f32 = 0) or float32 (1), values 0/1 (the engine's leaf batch)
 *   wt_bf16_dev       [D][kp] bf16: conv weight reshaped [D][C*k*k], zero padded to kp (multiple of 32)
 *   cpos_dev          [T][D] float32: row 0 = cls + pos[0], row 1+j = conv bias + pos[1+j]   (T = R*Cc + 1)
 *   ln_w_dev/ln_b_dev [D] float32 (required when xhat_out is given)
 *   x_out / xhat_out  [n][T][D] bf16, either may be NULL
 * Supported: embed_dim in {128, 256, 512}, kp in {32, 64, 96}, C*R*Cc <= 1984; anything else returns AZK_ERR_ARG
 * (the caller keeps a generic path).  v_mfma_f32_16x16x32_bf16; one wavefront per 16-token x D tile. */
int32_t azk_nn_patch_embed(const void *boards_dev, int32_t boards_are_f32, const void *wt_bf16_dev,
                           const float *cpos_dev, const float *ln_w_dev, const float *ln_b_dev,
                           void *x_out_bf16_dev, void *xhat_out_bf16_dev, int32_t n, int32_t channels,
                           int32_t rows, int32_t cols, int32_t ksize, int32_t kp, int32_t embed_dim,
                           float ln_eps, void *stream);

/* cls-row attention of the last block, folded (ai/nn.py:52-56 restricted to the row nn.py:80 reads): streams
 * xhat = LayerNorm1(tokens) [n][T][D] bf16 once and writes z[b][h][:] = sum_t softmax_t(xhat_t . m[b][h] + c[b][h])[t] * xhat_t
 * ([n][H][D] bf16) with an online softmax, so K and V are never materialised.  m_dev float32 [n or 1][H][D] =
 * scale * Wk_h^T q_h, c_dev float32 [n or 1][H] = scale * q_h . bk_h (per_board_m = 0: one shared row set, the depth-1
 * case where q is input independent).  Supported (embed_dim, heads): (512,8) (512,4) (256,8) (256,4) (128,4) (128,8). */
int32_t azk_nn_cls_attention(const void *xhat_bf16_dev, const float *m_dev, const float *c_dev, int32_t per_board_m,
                             void *z_out_bf16_dev, int32_t n, int32_t tokens, int32_t embed_dim, int32_t num_heads,
                             void *stream);

/* Depth-1 fast path of the folded cls attention (the cls query is a constant of the weights, so m is shared):
 *   azk_nn_patch_embed_scores - writes xn = (tokens - mean) * rstd (LayerNorm WITHOUT the affine; the caller folds gamma/beta
 *       into m', c and the value projection; ln_w/ln_b are ignored) and scores_out[b][h][t] = xn[b][t][:] . m'[h][:]
 *       (float32 [n][H][Tp], Tp = 16*ceil(T/16)).  The scores ride on the matrix cores: wt_bf16_dev has 16 extra rows
 *       [D .. D+16) holding m'_h^T Wconv (heads >= H zero), so x . m' comes out of the same MFMA chain as 16 extra output
 *       columns; score_cpos_dev float32 [T][16] = m'_h . cpos[t] is their additive term, score_msum_dev float32 [16] =
 *       sum_d m'_h[d], and xn . m' = rstd * (x . m' - mean * sum(m')).
 *   azk_nn_cls_pool - a = softmax_t(scores + c[h]);  z[b][h][:] = sum_t a[h][t] * xhat[b][t][:]  ([n][H][D] bf16):
 *       one streaming pass over xhat with no cross-lane reductions (HBM-read-bound).
 * n_valid_dev (optional, device int32): only the first min(n, *n_valid_dev) boards are processed - lets a captured
 * hipGraph with fixed launch sizes do work proportional to the live leaf count (azk_step_select's n_leaf_dev).
 * Heads: 8 or 4 (and 2*H <= 16). */
int32_t azk_nn_patch_embed_scores(const void *boards_dev, int32_t boards_are_f32, const void *wt_bf16_dev,
                                  const float *cpos_dev, const float *ln_w_dev, const float *ln_b_dev,
                                  void *xhat_out_bf16_dev, const float *score_cpos_dev, const float *score_msum_dev,
                                  float *scores_out_dev, int32_t num_heads, int32_t n, int32_t channels, int32_t rows, int32_t cols,
                                  int32_t ksize, int32_t kp, int32_t embed_dim, float ln_eps,
                                  const int32_t *n_valid_dev, void *stream);
int32_t azk_nn_cls_pool(const void *xhat_bf16_dev, const float *scores_dev, const float *c_dev, void *z_out_bf16_dev,
                        int32_t n, int32_t tokens, int32_t embed_dim, int32_t num_heads, const int32_t *n_valid_dev,
                        void *stream);

/* azk_nn_embed_pool - the two calls above fused: the normalised tokens stay on the CU (one workgroup per board, the
 * LayerNorm statistics cross its four waves through LDS, softmax over the tokens, the weighted token sum as a second
 * MFMA on the tile while it is still in registers).  Operands as azk_nn_patch_embed_scores, with the per-token constants
 * padded to whole 16-token tiles (Tp = 16 ceil(T/16) rows; cpos padding rows 0, score-constant padding rows -1e30 in the
 * head columns and 0 elsewhere) and stored in the kernel's accumulator order:
 *   cpos_frag_dev  [Tp/16][4][8][64][4]: [tile][w][q][lane][r] = cpos[16 tile + 4 (lane>>4) + r][128 w + 8 (lane&15) + q]
 *   score_frag_dev [Tp/16][64][4]:       [tile][lane][r]       = score_cpos[16 tile + 4 (lane>>4) + r][lane&15]
 * Column 15 of the extra weight rows / score constants is the row mean ((1/D) sum_d W[d][k], (1/D) sum_d cpos[t][d]).  score_ref_dev [16] (optional): per-head upper bound of
 * the scores (sqrt(D) |m'_h|) used as the softmax reference when 2*bound cannot underflow exp(); NULL = running maximum.
 * The constant c[h] of azk_nn_cls_pool drops out of a softmax over tokens.  embed_dim 512, heads 8 or 4.
 * z_out [n][H][512] bf16. */
int32_t azk_nn_embed_pool(const void *boards_dev, int32_t boards_are_f32, const void *wt_ext_bf16_dev,
                          const float *cpos_frag_dev, const float *score_frag_dev, const float *score_msum_dev,
                          const float *score_ref_dev, void *z_out_bf16_dev, int32_t num_heads, int32_t n, int32_t channels,
                          int32_t rows, int32_t cols, int32_t ksize, int32_t kp, int32_t embed_dim, float ln_eps,
                          const int32_t *n_valid_dev, void *stream);

/* Board source for the fused step: azk_nn_embed_pool_leaves takes the pending leaves of the last azk_step_tree straight from
 * the engine - it builds the prefix over the leaf flags itself (board j = the j-th flagged game in ascending game order,
 * exactly azk_step_gather's order), reads that game's cell codes, stores the slot j the next expansion will read its
 * logits row from, and writes the leaf count to n_leaf - so a simulation step is azk_step_tree -> azk_nn_embed_pool_leaves
 * -> tail, without azk_step_gather and without an evaluator batch.  Pointers are device pointers owned by the engine
 * (valid until azk_destroy) except n_leaf, which is the caller's. */
typedef struct azk_leaf_source {
    const uint8_t *leaf_flag;     /* [flag_bytes] 1 = the game has a pending leaf that needs the evaluator */
    const uint8_t *leaf_cells;    /* [n_games][rc_pad] cell codes at the leaf (bit 0 / 1 = player 0 / 1 stone) */
    const int32_t *to_move;       /* [n_games] side to move at the root */
    const int32_t *leaf_depth;    /* [n_games] */
    int32_t *leaf_slot;           /* [n_games] out: row of the evaluator outputs */
    int32_t *n_leaf;              /* [1] out */
    int32_t n_games, rows, cols, rc, rc_pad, planes, flag_bytes;
    uint32_t *cache_stamp;        /* shared eval cache: launch stamp the hand-off kernel bumps (NULL otherwise) */
} azk_leaf_source;
int32_t azk_leaf_source_of(azk_engine *e, int32_t *n_leaf_dev, azk_leaf_source *out);
int32_t azk_nn_embed_pool_leaves(const azk_leaf_source *src, const void *wt_ext_bf16_dev, const float *cpos_frag_dev,
                                 const float *score_frag_dev, const float *score_msum_dev, const float *score_ref_dev,
                                 void *z_out_bf16_dev, int32_t num_heads, int32_t ksize, int32_t kp, int32_t embed_dim,
                                 float ln_eps, void *stream);

/* azk_nn_embed_pool_compact(_leaves) - azk_nn_embed_pool restricted to the tokens a stone can reach (static softmax
 * reference only).  A token whose k x k patch is empty is a constant of the weights, so its contribution to the weighted
 * token sum and to the softmax denominator is precomputed over ALL tokens (z_all, l_all) and the kernel only evaluates the
 * "dirty" tokens - adding their real contribution and subtracting their constant one in the same MFMA.  The per-token
 * tables are indexed by token (T = rows*cols + 1 tokens; row T is the null token that pads the last tile):
 *   cpos_tok    f32  [T+1][512]  bias + positional term (row 0: cls + pos[0]); row T = 0
 *   score_tok   f32  [T+1][16]   score constants (column 15: row mean of cpos); row T = -1e30 in the head columns, 0 elsewhere
 *   wconst_tok  f32  [T+1][16]   exp(score - ref) of the token taken as an empty-patch token; 0 beyond num_heads and in row T
 *   xnconst_tok bf16 [T+1][512]  LayerNorm (no affine) of cpos_tok; row T = 0
 *   z_all       f32  [4][8][64][4] sum_t bf16(wconst)[t][h] * xnconst[t][col] at [w][q][lane][j]: h = 4 (lane>>4) + j, col = 128 w + 8 (lane&15) + q
 *   l_all       f32  [16]        sum_t wconst[t][h]
 *   wt_frag     bf16 the conv weight with its 16 extra rows (azk_nn_embed_pool's wt_ext [512+16][kp]) in MFMA fragment order:
 *               [33 column tiles][kp/32][64 lanes][8]: element [ct][s][l][i] = wt_ext[col(ct, l)][32 s + 8 (l>>4) + i],
 *               col(ct, l) = 128 (ct>>3) + 8 (l&15) + (ct&7) for ct < 32, 512 + (l&15) for ct = 32
 * sched_dev: int32 [2] work-queue words, zero before the first launch (each launch leaves them zero); one buffer per
 * stream that may run the kernel concurrently.  Boards differ in cost, so workgroups pull them from that queue.
 * Channels x ksize in {2, 3} x {3, 5}; kp = 32 ceil(channels ksize^2 / 32). */
typedef struct azk_embed_pool_consts {
    const void *wt_frag;
    const float *cpos_tok, *score_tok, *wconst_tok;
    const void *xnconst_tok;
    const float *z_all, *l_all, *score_msum, *score_ref;
    int32_t num_heads, ksize, kp, embed_dim;
    float ln_eps;
    uint64_t *work_stats;   /* optional device uint64 [2]: += boards evaluated, += 16-token tiles evaluated (bench accounting) */
} azk_embed_pool_consts;
int32_t azk_nn_embed_pool_compact(const void *boards_dev, int32_t boards_are_f32, const azk_embed_pool_consts *consts,
                                  void *z_out_bf16_dev, int32_t n, int32_t channels, int32_t rows, int32_t cols,
                                  const int32_t *n_valid_dev, int32_t *sched_dev, void *stream);
/* azk_nn_embed_pool_compact_leaves ranks the pending leaves with 16-bit counters: engines with more pending-leaf slots
 * (n_games * leaves_per_step) than this get AZK_ERR_ARG and keep azk_nn_embed_pool_leaves */
#define AZK_EMBED_POOL_COMPACT_MAX_SLOTS 65279
int32_t azk_nn_embed_pool_compact_leaves(const azk_leaf_source *src, const azk_embed_pool_consts *consts, void *z_out_bf16_dev,
                                         int32_t *sched_dev, void *stream);

/* ---- cls-row tail (nn.py:54-60, 78-83 for the row the heads read): small-M GEMMs with a device-side row count.
 * Packed weights (azk.pack_linear_weight): an nn.Linear weight [n_out][k] as bf16 in MFMA B-fragment order
 *   Wp[n_out/64][k/32][4][64][8] with element [g][s][c][lane][i] = W[64 g + 4 (lane&15) + c][32 s + 8 (lane>>4) + i]
 *   (n_out a multiple of 64 - pad with zero rows -, k of 32): one 16-byte load per fragment, and a lane's four accumulators
 *   of a row are four consecutive output columns. */
/* azk_nn_tail_gemm - one link of the cls-row tail as a latency-shaped small GEMM (every load of a K chunk in flight before
 * the first MFMA, no LDS):  C[m][nbatch * n_out] = op(A) W^T (+ bias) through one of four epilogues.
 *   a_bf16 [m][lda] row-major; batch b reads A columns [b * a_batch_stride, b * a_batch_stride + k), multiplies them with
 *   weight block b and writes output columns [b * n_out, (b + 1) * n_out) - nbatch = 1 is a plain GEMM, nbatch = heads is the
 *   block-diagonal per-head value projection.  w_packed: nbatch consecutive nn.Linear weights [n_out][k] in
 *   azk.pack_linear_weight's fragment packing (above).  k = 512 or 2048 (or 384 = AZK_EMBED_FOLD_ROW, plain bf16 epilogue only); n_out a multiple of 64.
 *   layernorm_a (k = 512): A = LayerNorm(rows) without affine (fold it into weight / bias: W diag(gamma), W beta + b); the row
 *            statistics are read from a_stats [m][a_stats_groups][2] = per 64-column group (sum, sum of squares) of the row, as
 *            left by the GEMM that produced A (its stats_out); a_stats_groups must be 8 (= k / 64; 64-byte rows, 16-byte aligned).
 *   stats_out (optional, epilogues 0-2): float32 [m][nbatch * n_out / 64][2], the same partials of the rows written here.
 *   epilogue 0: out_bf16 = acc + bias;  1: GELU(acc + bias) (exact erf);  2: acc + bias + resid_bf16;
 *            3: merged heads - logits_out float32 [m][action_dim], values_out[m] = tanh(column action_dim)   (nn.py:82-83).
 *   n_valid (optional, device): rows at or beyond it are neither read nor written. */
typedef struct azk_tail_gemm {
    const void *a_bf16; int32_t lda, a_batch_stride;
    const void *w_packed;
    int32_t m, n_out, k, nbatch;
    const int32_t *n_valid;
    const float *bias;
    int32_t layernorm_a, epilogue;
    float ln_eps;
    const float *a_stats; int32_t a_stats_groups;
    float *stats_out;
    void *out_bf16; int32_t ldo;
    const void *resid_bf16; int32_t ldr;
    float *logits_out, *values_out; int32_t action_dim;
    const float *a_col_sums;          /* azk_nn_tail_gemm_lds with layernorm_a: float32 [n_out] column sums of the bf16 weight (ABI 4) */
} azk_tail_gemm;
int32_t azk_nn_tail_gemm(const azk_tail_gemm *desc, void *stream);
/* azk_nn_tail_gemm_lds - the same descriptor, the two WIDE links of the tail (nn.py:58-60) as LDS-staged GEMMs (csrc/azk_tail.hip:
 * activation and weight tiles to LDS by LDS-DMA in full 128-byte lines, a ring of K stages retired by counted waits, eight waves per
 * workgroup at two waves per SIMD):
 *   k = 512,  epilogue 1 (GELU), layernorm_a = 1, n_out a multiple of 128: LayerNorm applied in the epilogue,
 *             out = GELU(rstd (A W^T - mean a_col_sums) + bias) - A enters the matrix pipe as stored (no re-rounded normalised copy);
 *             a_stats as for azk_nn_tail_gemm, a_col_sums required, no stats_out;
 *   k = 2048, epilogue 2 (residual), layernorm_a = 0, n_out a multiple of 64: K split over four wave groups whose chains are added in
 *             the fixed order 0..3 - bit for bit azk_nn_tail_gemm's result on the same inputs; optional stats_out.
 * Anything else: AZK_ERR_ARG (use azk_nn_tail_gemm). */
int32_t azk_nn_tail_gemm_lds(const azk_tail_gemm *desc, void *stream);
/* process-wide launch-shape knobs for callers that step several game groups on separate streams (selfplay.SelfPlayRunner n_split > 1):
 * azk_nn_tail_lds_footprint(1): the K = 2048 link keeps two LDS ring buffers (96 KB) instead of three (144 KB);
 * azk_nn_embed_fold_grid(n): azk_nn_embed_fold(_leaves) launches at most n workgroups (0 = default, two per CU).  Results do not change. */
int32_t azk_nn_tail_lds_footprint(int32_t small);
int32_t azk_nn_embed_fold_grid(int32_t max_workgroups);

/* azk_nn_ln_heads: final LayerNorm + merged policy/value head + finalize in one launch (nn.py:78-83 for the cls row):
 *   logits[n][A] = LN(x) Wh^T + bh (float32), values[n] = tanh(column A).  LayerNorm's affine is folded into the operands by the
 *   caller: w_packed_dev = the merged head weight times diag(gamma), [n_out_padded][embed_dim] in azk.pack_linear_weight's packing,
 *   bias_dev = Wh beta + bh.  Each wave fetches its 16-row slab once, takes the row statistics from those registers and normalises
 *   on the way into the MFMAs (embed_dim 256 or 512). */
int32_t azk_nn_ln_heads(const void *x_bf16_dev, float eps, const void *w_packed_dev, const float *bias_dev, int32_t n,
                        int32_t embed_dim, int32_t n_out_padded, int32_t action_dim, float *logits_out_dev, float *values_out_dev,
                        const int32_t *n_valid_dev, void *stream);

/* azk_nn_embed_fold(_leaves) - the embedding + cls pooling WITHOUT forming the token rows (round 3; ai/nn.py:7-27, 36-56 for the
 * cls row, as azk_nn_embed_pool_compact + the first azk_nn_tail_gemm link).  With x_t = Wc p_t + cpos_t (p_t: the 0/1 patch of token
 * t, <= 64 bits) LayerNorm1's statistics and the cls scores of a token are functions of its patch bits alone:
 *     x_t - mean(x_t) = Wt p_t + ct_t        D var_t = p_t' G p_t + u2_t . p_t + n_t        s_t[h] = rstd_t (S_h . p_t + sc_t[h])
 * (Wt = Wc minus its column means, ct_t = cpos_t minus its mean, G = Wt' Wt, u2_t = 2 Wt' ct_t, n_t = |ct_t|^2, S_h = Wt' m'_h,
 * sc_t[h] = m'_h . ct_t), and the value-projected pooled row is linear in x_t:
 *     u_h = Wv'_h z_h = (1 / L_h) sum_t a_t[h] (M_h p_t + D_t[h]),   a = w rstd,   M_h = Wv'_h Wt,   D_t[h] = Wv'_h ct_t.
 * The kernel evaluates the tokens a stone can reach (the rest are constants of the weights, summed ahead: U_all, l_all) and writes,
 * per board and head, one bf16 row of AZK_EMBED_FOLD_ROW entries:
 *     [0, T)       (a_t - aconst_t) / L      (0 for tokens no stone reaches)
 *     [T, T+3)     1 / L as bf16 hi, lo, hi  (against U_all hi, U_all hi, U_all lo in the weight)
 *     [256, 320)   sum_t a_t p_t / L         (the pooled patch; entries >= channels ksize^2 are 0)
 *     elsewhere 0
 * so that ONE batched azk_nn_tail_gemm (nbatch = heads, k = AZK_EMBED_FOLD_ROW, weight rows [D_t[h]; U_all; ...; M_h]) yields u, the
 * input of the output projection.  Tables (T = rows cols + 1 tokens, row T = the null token that pads the last tile):
 *   g_frag      f16 [2 (hi, lo)][4 column tiles][2 k-steps][64 lanes][8]: G x g_scale as two terms, MFMA B-fragment order
 *               (element [t][q][s][l][i] = term t of G[16 q + (l & 15)][32 s + 8 (l >> 4) + i])
 *   e_frag      f16 [2][2][64][8]: the score columns S (column h < heads; others 0) x e_scale, same order
 *   u2_tok      f32 [T+1][64];   score_tok f32 [T+1][16]: sc_t[h], column 15 = n_t (row T: -1e30 in the head columns, column 15 = 512)
 *   wconst_tok  f32 [T+1][16]: exp(rstdc_t sc_t[h] - ref[h]), column 15 = rstdc_t = rsqrt(n_t / 512 + eps)
 *   l_all, score_ref f32 [16] (score_ref >= 1e30 beyond the heads)
 * Covered: embed_dim 512, head dim 64, 4 / 8 heads, channels ksize^2 <= 64, T + 3 <= 256. */
#define AZK_EMBED_FOLD_ROW 384
/* azk_nn_embed_fold_leaves keeps the rank -> game table of the launch in LDS: engines with more pending-leaf slots than this get
 * AZK_ERR_ARG and keep azk_nn_embed_pool_compact_leaves */
#define AZK_EMBED_FOLD_MAX_SLOTS 8192
typedef struct azk_embed_fold_consts {
    const void *g_frag, *e_frag;
    const float *u2_tok, *score_tok, *wconst_tok, *l_all, *score_ref;
    const float *inv_scales;    /* device [2]: 1 / g_scale, 1 / e_scale (device data, so that new weights can be copied in under a captured graph) */
    int32_t num_heads, ksize, embed_dim;
    float ln_eps;
    uint64_t *work_stats;   /* optional device uint64 [2]: += boards evaluated, += 16-token tiles evaluated */
} azk_embed_fold_consts;
int32_t azk_nn_embed_fold(const void *boards_dev, int32_t boards_are_f32, const azk_embed_fold_consts *consts, void *rows_out_bf16_dev,
                          int32_t n, int32_t channels, int32_t rows, int32_t cols, const int32_t *n_valid_dev, int32_t *sched_dev,
                          void *stream);
int32_t azk_nn_embed_fold_leaves(const azk_leaf_source *src, const azk_embed_fold_consts *consts, void *rows_out_bf16_dev,
                                 int32_t *sched_dev, void *stream);
/* azk_nnx_embed_fold(_leaves): the same function in float32-accurate arithmetic for the fp32 line (ai/nn.py:74-84 at ai/mcts.py:46 in the
 * reference's own precision): correctly rounded rsqrt, exp with an extended-precision argument, the pooled patch on v_mfma_f32_16x16x4_f32,
 * float32 rows out ([T] = 1 / L, [T+1], [T+2] = 0) for azk_nnx_gemm_h's float32-A link (k = AZK_EMBED_FOLD_ROW). */
int32_t azk_nnx_embed_fold(const void *boards_dev, int32_t boards_are_f32, const azk_embed_fold_consts *consts, float *rows_out_f32_dev,
                           int32_t n, int32_t channels, int32_t rows, int32_t cols, const int32_t *n_valid_dev, int32_t *sched_dev,
                           void *stream);
int32_t azk_nnx_embed_fold_leaves(const azk_leaf_source *src, const azk_embed_fold_consts *consts, float *rows_out_f32_dev,
                                  int32_t *sched_dev, void *stream);

/* ---- fp32-accurate network path (csrc/azk_nnx.hip): the reference evaluates its network in float32 (ai/nn.py:74-84 called at
 * ai/mcts.py:46), and north_star asks for visit-count policies within 1e-5 of it.  The same two stages as above - boards -> pooled
 * tokens (azk_nn_embed_pool_compact's function) -> cls-row tail (azk_nn_tail_gemm's function) - in arithmetic that keeps float32
 * accuracy end to end: the 0/1 board against the conv weight (and the folded score / mean columns) split into two fp16 terms
 * (exact products, float32 accumulation on v_mfma_f32_16x16x32_f16), everything with two run-time operands on v_mfma_f32_16x16x4_f32,
 * statistics / softmax / GELU(erf) / tanh in float32.  Tables as azk_embed_pool_consts, all float32, with
 *   wt_frag     fp16 [33 column tiles][kp/32][2: hi, lo][64 lanes][8]: element [ct][s][p][l][i] = the p-th fp16 term of
 *               wt_scale * wt_ext[col(ct, l)][32 s + 8 (l>>4) + i], col(ct, l) = 64 (ct>>2) + 4 (l&15) + (ct&3) for ct < 32, 512 + (l&15) for ct = 32
 *   xnconst_tok fp16 [T+1][128][8]: the constant tokens' normalised rows x 16 as two fp16 terms, per 4 columns (hi0..hi3, lo0..lo3)
 *   score_ref   per head the largest score of a constant token (their weights wconst are in (0, 1]); score bound <= 40 required
 *   z_all       f32 [8][4][64][4]: pool_scale * sum_t wconst[t][h] * xnconst[t][col] (from the fp16 terms) at [g][q][lane][j]: h = 4 (lane>>4) + j, col = 64 g + 4 (lane&15) + q
 * kp <= 64 (the hi / lo image must fit one CU's LDS), tokens <= 256.  z_out float32 [n][H][512]. */
typedef struct azk_embed_pool_x_consts {
    const void *wt_frag;
    const float *cpos_tok, *score_tok, *wconst_tok;
    const void *xnconst_tok;
    const float *z_all, *l_all, *score_msum, *score_ref;
    int32_t num_heads, ksize, kp, embed_dim;
    float ln_eps, wt_scale;
    uint64_t *work_stats;   /* optional device uint64 [2]: += boards evaluated, += 16-token tiles evaluated */
    const uint32_t *wconst_h16_tok;   /* [T+1][16]: -wconst * 64 as two fp16 terms, hi | lo << 16 */
    float pool_scale;                 /* 64 * 16: the unit of z_all and of the kernel's accumulators */
} azk_embed_pool_x_consts;
int32_t azk_nnx_embed_pool(const void *boards_dev, int32_t boards_are_f32, const azk_embed_pool_x_consts *consts,
                           float *z_out_f32_dev, int32_t n, int32_t channels, int32_t rows, int32_t cols,
                           const int32_t *n_valid_dev, int32_t *sched_dev, void *stream);
int32_t azk_nnx_embed_pool_leaves(const azk_leaf_source *src, const azk_embed_pool_x_consts *consts, float *z_out_f32_dev,
                                  int32_t *sched_dev, void *stream);
/* azk_nnx_gemm_h - one link of the cls-row tail (azk_nn_tail_gemm's function: C[m][nbatch * n_out] = op(A) W^T (+ bias) through
 * epilogues 0-3, batches and n_valid as there) in float32 accuracy: every operand as TWO fp16 terms (x scale = hi + lo, 22
 * significant bits; products hi*hi + hi*lo + lo*hi exact in the float32 accumulator) on v_mfma_f32_16x16x32_f16, a fifth of the
 * matrix-pipe time of the float32-input MFMA.  k = 512 or 2048 (or AZK_EMBED_FOLD_ROW with a_f32).
 *   A: either (a_hi, a_lo) fp16 planes [m][lda] holding a * a_scale (written by the producing call's out_hi / out_lo), or a_f32
 *      float32 [m][lda] split on the fly (first link only: epilogue 0);
 *   w_packed: nbatch weights [n_out][k] x w_scale as fp16 (hi, lo) in fragment order Wp[n_out/64][k/32][4][2][64 lanes][8]:
 *      element [g][s][c][p][lane][i] = term p of W[64 g + 4 (lane&15) + c][32 s + 8 (lane>>4) + i];
 *   layernorm_a (k = 512): LayerNorm moves into the epilogue - out = rstd (acc - mean col_sums[n]) + bias, col_sums[n] = sum_k W[n][k]
 *      (of the reconstructed terms), mean / rstd from a_stats [m][8][2] = per 64-column group (sum, sum of squares) of the row, as
 *      left by the producing call's stats_out;
 *   outputs: out_f32 and / or (out_hi, out_lo) planes (x a_scale) [m][ldo]; stats_out (optional, epilogues 0-2): float32
 *      [m][nbatch * n_out / 64][2], the same partials of the rows written here;
 *   epilogue 0: acc + bias;  1: GELU(acc + bias) (exact erf form via erff);  2: acc + bias + resid_f32;
 *            3: merged heads - logits_out float32 [m][action_dim], values_out[m] = tanh(column action_dim). */
typedef struct azk_gemm_h {
    const void *a_hi, *a_lo; const float *a_f32; int32_t lda, a_batch_stride;
    const void *w_packed;
    int32_t m, n_out, k, nbatch;
    const int32_t *n_valid;
    const float *bias, *col_sums;
    int32_t layernorm_a, epilogue;
    float ln_eps, a_scale, w_scale;
    const float *a_stats;
    float *stats_out;
    void *out_hi, *out_lo; float *out_f32; int32_t ldo;
    const float *resid_f32; int32_t ldr;
    float *logits_out, *values_out; int32_t action_dim;
    int32_t *overflow_flag;       /* optional, device (ABI 4): set to 1 when a value written to (or split into) the fp16 planes leaves fp16's range
                                   * (|x a_scale| >= 65504): the planes then hold inf and the caller must not trust the outputs */
} azk_gemm_h;
int32_t azk_nnx_gemm_h(const azk_gemm_h *desc, void *stream);
/* azk_nnx_gemm_h_lds - the same descriptor, the two WIDE links (k = 512 -> n_out, LayerNorm + GELU; k = 2048, residual) with both
 * operand planes staged through LDS by LDS-DMA (csrc/azk_tail.hip, as azk_nn_tail_gemm_lds): the same accumulation chains in the same
 * order and the same epilogue arithmetic as azk_nnx_gemm_h.  (a_hi, a_lo) planes only, nbatch = 1; anything else: AZK_ERR_ARG. */
int32_t azk_nnx_gemm_h_lds(const azk_gemm_h *desc, void *stream);

/* ---- vanilla mode: MCTS.mcts(model=None, ...) (mcts.py:57-59), MCTS.simulate (mcts.py:62-79), UCB1 of
 * utils.py:29-44 mode 'normal'.  A search is azk_begin_search(e, NULL) followed by azk_vanilla_search calls summing to
 * n simulations (each launch runs its simulations - select, expand, random rollout, backup - entirely on the device);
 * results are read with azk_root_stats / azk_root_children / azk_export_tree / azk_advance as in network mode.
 * Random numbers: np.random.randint of the legacy global RandomState, i.e. MT19937 + numpy's masked rejection, on one
 * MT19937 state per game: 625 uint32 = the 624 key words and the position, the layout of np.random.get_state()[1:3].
 * Seeding a game with the caller's np.random state makes the search consume exactly the reference's stream; the state
 * read back is what np.random.set_state() needs afterwards.  Default states: init_genrand(5489 + game). */
int32_t azk_vanilla_set_rng(azk_engine *e, int32_t first, int32_t count, const uint32_t *mt_states_host, void *stream);
int32_t azk_vanilla_get_rng(azk_engine *e, int32_t first, int32_t count, uint32_t *mt_states_host, void *stream);  /* synchronises */
int32_t azk_vanilla_search(azk_engine *e, int32_t n_sims, void *stream);

/* ---- the full-token transformer block (ai/nn.py:38-61) for networks with depth > 1 (csrc/azk_block.hip) ----
 * azk_nn_gemm_tok: out[m][n_out] = A[m][k] W^T (+ bias) through an epilogue, LDS-staged (LDS-DMA in full lines, counted-wait ring):
 *   a_bf16 [m][lda] row-major; w_packed = an nn.Linear weight [n_out][k] in azk.pack_linear_weight's fragment packing (n_out a multiple of
 *   128 - pad with zero rows -, k a multiple of 64, k >= 128); epilogue 0: bf16 out; 1: bf16 GELU(.) (erf form); 2: bf16 out = . +
 *   resid_bf16[m][ldr]; 4: float32 out.  n_valid (optional, device): rows at or beyond it are neither read nor written. */
typedef struct azk_gemm_tok {
    const void *a_bf16; int32_t lda;
    const void *w_packed;
    int32_t m, n_out, k;
    const int32_t *n_valid;
    const float *bias;
    int32_t epilogue;
    void *out; int32_t ldo;
    const void *resid_bf16; int32_t ldr;
} azk_gemm_tok;
int32_t azk_nn_gemm_tok(const azk_gemm_tok *desc, void *stream);
/* azk_nn_attention_tok: nn.MultiheadAttention (eval mode) over ALL tokens of every board: out[b][t][h dh ..] = softmax_t'(q k^T /
 * sqrt(dh)) v per board b and head h.  qkv_bf16 [n_boards][tokens][3 embed_dim] = the in-projection's output (q | k | v);
 * tokens <= 256; head dimension 32 or 64.  n_valid (optional, device): boards at or beyond it are skipped. */
int32_t azk_nn_attention_tok(const void *qkv_bf16_dev, void *out_bf16_dev, int32_t n_boards, int32_t tokens, int32_t embed_dim,
                             int32_t num_heads, const int32_t *n_valid_dev, void *stream);

/* nn.LayerNorm over the rows of a bf16 matrix [n][embed_dim] (norm2 / norm of nn.py:41-42,78; fp32 statistics) -> y;
 * with add_bias_dev != NULL the rows of x are also replaced by x + add_bias (the residual the next GEMM accumulates
 * onto, nn.py:59-60).  embed_dim in {128, 256, 512}. */
int32_t azk_nn_layernorm_rows(void *x_bf16_dev, const float *w_dev, const float *b_dev, float eps, void *y_bf16_dev,
                              const float *add_bias_dev, int32_t n, int32_t embed_dim, const int32_t *n_valid_dev,
                              void *stream);

/* Merged policy/value head output (bf16 [n][ld]: columns [0, A) logits, column A the raw value) -> float32 logits [n][A]
 * and values [n] = tanh(raw) (nn.py:82-83) in one launch; n_valid_dev as above. */
int32_t azk_nn_heads_finalize(const void *heads_bf16_dev, int32_t ld, int32_t action_dim, int32_t n, float *logits_out_dev,
                              float *values_out_dev, const int32_t *n_valid_dev, void *stream);

/* float32 softmax exactly as the engine applies it to logits (test hook; [n][A] -> [n][A]) */
int32_t azk_softmax_rows(const float *logits_dev, int32_t n, int32_t action_dim, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* AZK_H */
