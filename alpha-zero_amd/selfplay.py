"""Batched self-play on the azk engine: thousands of <Game>.self_play loops as one lock-step batch.

Mirrors the per-move loop of games/gomoku.py:123-164 (and tictactoe.py:99-133, connect4.py:117-151):
fresh root -> n_sims simulations -> pi, q, raw board recorded -> sample (early moves) or most-visited
child -> make_move -> check_winner / draw.  Every game does that in the same step of the same kernels.

self_play_batch returns, per game, the tuple the reference's Gomoku.self_play returns
(boards, actions, policy_distributions, qs, winner) so train.collect_data's consumer
(train.save_data_to_buffer, train.py:30-49) can take it unchanged.
"""
import contextlib
import gc
import math

import numpy as np

from azk import Engine, board_elements, emit_mask, puct_setting, puct_table  # noqa: F401  (puct_table: the public helper behind puct=((c_init, c_base), ...))
from azk import move_temperature_setting

# gomoku.py:144 samples while move_count < 8; tictactoe.py:117 / connect4.py:135 sample every move
SAMPLE_UNTIL = {"gomoku": 8, "tictactoe": 1 << 30, "connect4": 1 << 30}


@contextlib.contextmanager
def capture_without_finalisers():
    """Around a hipGraph capture: no finaliser may run inside it.  An Engine that a dead reference cycle keeps alive (a runner and the
    closure it reports to) is destroyed whenever Python's cyclic collector next runs, and azk_destroy's hipFree inside a capture invalidates
    the capture (torch.cuda.graph no longer collects before it begins).  So: collect now, and keep the collector off until the capture ends."""
    gc.collect()
    was_on = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was_on:
            gc.enable()


def cells_to_board(cells, planes, rows, cols, side_to_move):
    """int8 cell codes -> the reference's float32 board [F,R,C] (plane 2 = side to move, tictactoe.py:17,41)."""
    b = np.zeros((planes, rows, cols), np.float32)
    c = np.asarray(cells).reshape(rows, cols)
    b[0] = c == 1
    b[1] = c == 2
    if planes == 3:
        b[2] = side_to_move
    return b


def check_playout_cap(playout_cap, n_sims, leaves_per_step=1):
    """playout_cap = (p_full, n_fast) -> (float, int), or None for off.  OPT-IN playout-cap randomisation (include/azk.h azk_set_playout_cap;
    DESIGN section 18): a search is FULL (n_sims simulations) with probability p_full, else FAST (n_fast simulations); only full plies are
    trained on.  Raises ValueError for what the engine refuses too: p_full outside [0, 1], n_fast outside [1, n_sims], virtual loss."""
    if playout_cap is None:
        return None
    try:
        p_full, n_fast = playout_cap
        p_full, n_fast = float(p_full), int(n_fast)
    except (TypeError, ValueError):
        raise ValueError(f"playout_cap must be (p_full, n_fast), not {playout_cap!r}")
    if not 0.0 <= p_full <= 1.0:                                  # (NaN fails both comparisons)
        raise ValueError(f"playout_cap: p_full must lie in [0, 1], not {p_full!r}")
    low = min(n_sims) if isinstance(n_sims, (tuple, list)) else n_sims
    if not 1 <= n_fast <= low:
        raise ValueError(f"playout_cap: n_fast must lie in [1, n_sims = {low}], not {n_fast!r}")
    if int(leaves_per_step) > 1:
        raise ValueError("playout_cap does not combine with leaves_per_step > 1 (virtual loss counts completed simulations differently)")
    return p_full, n_fast


def check_resign(resign, leaves_per_step=1):
    """resign = (v_resign, p_never[, min_ply]) -> (float, float, int), or None for off.  OPT-IN resignation (include/azk.h azk_set_resign;
    DESIGN section 19): after a move that does not end the game the side that has just moved concedes when the recorded root q - the
    outcome for the OPPONENT of the side to move, as it is, no sign change - is >= v_resign and the game has at least min_ply plies; a share
    p_never of the games never resigns and is only marked.  Raises ValueError for what the engine refuses too: v_resign outside (0, 1]
    (None is "off"), p_never outside [0, 1], a negative min_ply, virtual loss."""
    if resign is None:
        return None
    try:
        v, p_never, min_ply = resign if len(resign) == 3 else (resign[0], resign[1], 0) if len(resign) == 2 else (None, None, None)
        if int(min_ply) != min_ply:
            raise ValueError
        v, p_never, min_ply = float(v), float(p_never), int(min_ply)
    except (TypeError, ValueError):
        raise ValueError(f"resign must be (v_resign, p_never) or (v_resign, p_never, min_ply), not {resign!r}")
    if not 0.0 < v <= 1.0:                                        # (NaN fails both comparisons)
        raise ValueError(f"resign: v_resign must lie in (0, 1] (None switches resignation off), not {v!r}")
    if not 0.0 <= p_never <= 1.0:
        raise ValueError(f"resign: p_never must lie in [0, 1], not {p_never!r}")
    if min_ply < 0:
        raise ValueError(f"resign: min_ply must not be negative, not {min_ply!r}")
    if int(leaves_per_step) > 1:
        raise ValueError("resign does not combine with leaves_per_step > 1 (a virtual-loss search is another search: its q is not the one a threshold was set on)")
    return v, p_never, min_ply


def check_forced_playouts(forced_playouts, evaluator=True, dirichlet=True, leaves_per_step=1):
    """forced_playouts = k -> float, or None for off (None or 0).  OPT-IN forced playouts and policy target pruning at the root (include/azk.h
    azk_set_forced_playouts): a root child with N >= 1 visits and mixed prior P is selected first while
    N * N < (k * P) * (root visits - 1), and the recorded pi loses the visits only that floor explains.  Raises ValueError, before any engine
    exists, for what the engine refuses too - a negative, NaN or infinite k, virtual loss - and for searches without the root's mixed priors:
    vanilla MCTS (evaluator None) and dirichlet=False."""
    if forced_playouts is None:
        return None
    try:
        k = float(forced_playouts)
    except (TypeError, ValueError):
        raise ValueError(f"forced_playouts must be a number k >= 0 (KataGo: 2), not {forced_playouts!r}")
    if not 0.0 <= k < float("inf"):                               # (NaN fails both comparisons)
        raise ValueError(f"forced_playouts: k must be finite and not negative, not {forced_playouts!r}")
    if k == 0.0:
        return None
    if evaluator is None or (isinstance(evaluator, (tuple, list)) and any(e is None for e in evaluator)):
        raise ValueError("forced_playouts: vanilla MCTS (evaluator None) is refused - it has no priors for the floor to be proportional to")
    if not dirichlet:
        raise ValueError("forced_playouts needs root noise (dirichlet=True): the rule acts on the root's noise-mixed float64 priors")
    if int(leaves_per_step) > 1:
        raise ValueError("forced_playouts does not combine with leaves_per_step > 1 (a virtual-loss search counts a visit before its value exists)")
    return k


def check_gumbel_root(gumbel_root, n_sims=None, evaluator=True, dirichlet=True, leaves_per_step=1, tree_reuse=0, playout_cap=None,
                      forced_playouts=None, surprise_weight=None):
    """gumbel_root = (m, c_visit, c_scale) -> (int, float, float), or None for off.  OPT-IN Gumbel root search (include/azk.h azk_set_gumbel_root;
    DESIGN section 24): m root actions sampled by Gumbel-top-k, the search's simulations spread over them by sequential halving, the survivor
    played and softmax(logits + sigma(completed Q)) recorded.  Raises ValueError, before any engine exists, for what the engine refuses too - m
    outside 1..64, a negative or non-finite c_visit, a c_scale that is not positive and finite, fewer than 2 simulations, virtual loss, tree
    reuse, a playout cap, forced playouts, surprise weighting - and for searches without a network or without the Gumbel rows: vanilla MCTS
    (evaluator None) and dirichlet=False."""
    if gumbel_root is None:
        return None
    try:
        m, c_visit, c_scale = gumbel_root
        m, c_visit, c_scale = int(m), float(c_visit), float(c_scale)
    except (TypeError, ValueError):
        raise ValueError(f"gumbel_root must be (m, c_visit, c_scale), not {gumbel_root!r}")
    if not 1 <= m <= 64:
        raise ValueError(f"gumbel_root: m must lie in [1, 64], not {m!r}")
    if not 0.0 <= c_visit < float("inf"):
        raise ValueError(f"gumbel_root: c_visit must be finite and not negative, not {c_visit!r}")
    if not 0.0 < c_scale < float("inf"):
        raise ValueError(f"gumbel_root: c_scale must be finite and positive, not {c_scale!r}")
    if n_sims is not None and (isinstance(n_sims, (tuple, list)) or int(n_sims) < 2):
        raise ValueError(f"gumbel_root: n_sims must be one number >= 2 (the halving table is built for one budget), not {n_sims!r}")
    if evaluator is None or (isinstance(evaluator, (tuple, list)) and any(e is None for e in evaluator)):
        raise ValueError("gumbel_root: vanilla MCTS (evaluator None) is refused - it has no logits for the Gumbel draws to be added to")
    if not dirichlet:
        raise ValueError("gumbel_root takes the place of root noise (dirichlet=True): the runners pass Gumbel rows where they pass Dirichlet rows")
    if int(leaves_per_step) > 1:
        raise ValueError("gumbel_root does not combine with leaves_per_step > 1 (a virtual-loss search counts a visit before its value exists)")
    if tree_reuse:
        raise ValueError("gumbel_root does not combine with tree reuse (the eligibility rule needs a fresh root)")
    if playout_cap is not None:
        raise ValueError("gumbel_root does not combine with playout_cap (the halving table is built for one budget)")
    if forced_playouts:
        raise ValueError("gumbel_root does not combine with forced_playouts (the eligibility rule needs raw root selection)")
    if surprise_weight is not None:
        raise ValueError("gumbel_root does not combine with surprise_weight (its recorded pi is not a visit distribution)")
    return m, c_visit, c_scale


def check_puct(puct, evaluator=True, leaves_per_step=1, forced_playouts=None, gumbel_root=None):
    """puct = (c, fpu) -> the (c_table, fpu_mode, fpu_tree, fpu_root) of azk_set_puct, or None for off.  OPT-IN configurable PUCT (include/azk.h
    azk_set_puct): c is a number, a tuple (c_init, c_base) (puct_table) or a list of table entries indexed by the selecting
    node's visit count; fpu is None, ("absolute", v_tree[, v_root]) or ("reduction", r_tree[, r_root]).  Raises ValueError, before any engine
    exists, for what the engine refuses too - a table that is empty, too long or holds a negative or non-finite entry, an unknown FPU kind, a
    non-finite FPU parameter, a negative reduction, virtual loss, forced playouts, a Gumbel root - and for vanilla MCTS (evaluator None), whose
    UCB1 the option does not cover."""
    if puct is None:
        return None
    try:
        c, fpu = puct
    except (TypeError, ValueError):
        raise ValueError(f"puct must be (c, fpu), not {puct!r}")
    setting = puct_setting(c, fpu)
    if _is_vanilla(evaluator):
        raise ValueError("puct: vanilla MCTS (evaluator None) is refused - it selects by UCB1, which the option does not cover")
    if int(leaves_per_step) > 1:
        raise ValueError("puct does not combine with leaves_per_step > 1 (a virtual-loss search leaves losses in the value sums the FPU rule reads)")
    if forced_playouts:
        raise ValueError("puct does not combine with forced_playouts (the pruning bound restates the reference's selection formula)")
    if gumbel_root is not None:
        raise ValueError("puct does not combine with gumbel_root (its root selection is not PUCT)")
    return setting


def check_solver(solver, evaluator=True, leaves_per_step=1, forced_playouts=None, gumbel_root=None, puct=None, tree_reuse=0):
    """solver = True -> True, or None for off (None or False).  OPT-IN exact game-end proofs in the search (include/azk.h azk_set_solver; DESIGN
    section 29): every node keeps a status proven from terminal leaves up the simulation's path, the walk stops on proven nodes below the
    root and selection shuts out children proven lost.  Raises ValueError, before any engine exists, for what the engine refuses too - virtual
    loss, forced playouts, a Gumbel root, configurable PUCT, tree reuse - and for vanilla MCTS (evaluator None), which keeps no status."""
    if solver is None or solver is False:
        return None
    if solver is not True:
        raise ValueError(f"solver must be True, False or None, not {solver!r}")
    if _is_vanilla(evaluator):
        raise ValueError("solver: vanilla MCTS (evaluator None) is refused - its search keeps no status column")
    if int(leaves_per_step) > 1:
        raise ValueError("solver does not combine with leaves_per_step > 1 (a virtual-loss search leaves losses on paths a proof would end)")
    if forced_playouts:
        raise ValueError("solver does not combine with forced_playouts (a forced child and a child shut out would claim the same selection)")
    if gumbel_root is not None:
        raise ValueError("solver does not combine with gumbel_root (the eligibility rule needs raw root selection)")
    if puct is not None:
        raise ValueError("solver does not combine with puct (the two options' kernels are not combined)")
    if int(tree_reuse) != 0:
        raise ValueError("solver does not combine with tree_reuse (the status column is not carried through a re-rooting)")
    return True


def eval_symmetry_elements(game, size=None):
    """The D4 elements (the emission's numbering: rot0, lr, tb, rot90, lr(rot90), tb(rot90), rot180, rot270) a game's geometry admits
    (include/azk.h azk_set_eval_symmetry): all eight on a square board with one action per cell, {0, 1, 2, 6} on a Gomoku board with
    rows != cols, {0, 1} for Connect4 (gravity)."""
    return board_elements(game, size)


def check_eval_symmetry(eval_symmetry, game, size=None, evaluator=True, leaves_per_step=1, seed=0):
    """eval_symmetry = True | ("fixed", s) -> the (mode, value) of Engine.set_eval_symmetry, or None for off (None or False).  OPT-IN evaluation
    under a board symmetry (include/azk.h azk_set_eval_symmetry): the evaluator sees every leaf turned by a D4 element and
    its logits are turned back.  True: the element is a hash of (seed, the leaf's position) - mode 1 with `seed`; ("fixed", s): element s for
    every leaf.  Raises ValueError, before any engine exists, for what the engine refuses too - an element the geometry does not admit, virtual
    loss - and for vanilla MCTS (evaluator None), which evaluates nothing."""
    if eval_symmetry is None or eval_symmetry is False:
        return None
    if eval_symmetry is True:
        mode, value = 1, int(seed) & ((1 << 64) - 1)
    else:
        try:
            kind, value = eval_symmetry
            if kind != "fixed" or int(value) != value:
                raise ValueError
            mode, value = 2, int(value)
        except (TypeError, ValueError):
            raise ValueError(f"eval_symmetry must be True (keyed by the position) or ('fixed', element), not {eval_symmetry!r}")
        if value not in eval_symmetry_elements(game, size):
            raise ValueError(f"eval_symmetry: element {value!r} is not one of {eval_symmetry_elements(game, size)}, the elements this board's geometry admits")
    if evaluator is None or (isinstance(evaluator, (tuple, list)) and any(e is None for e in evaluator)):
        raise ValueError("eval_symmetry: vanilla MCTS (evaluator None) is refused - it evaluates no leaf")
    if int(leaves_per_step) > 1:
        raise ValueError("eval_symmetry does not combine with leaves_per_step > 1 (the virtual-loss schedule is not pinned under it)")
    return mode, value


def check_emit_symmetry(emit_symmetry, game, size=None):
    """emit_symmetry = None | "board" | "none" | an iterable of elements -> the engine's azk_config.emit_elements mask (0 for None: off).  OPT-IN
    (state, pi, z) emission under a mask of D4 elements, on every geometry (include/azk.h azk_config.emit_elements): plies 0
    and 1 of a finished game are stored once, every later ply once per element of the mask - "board": every element the geometry admits, on a
    square board the reference's eight; "none": the identity alone.  Raises ValueError, before any engine exists, for what azk_create refuses
    too: an element above 7, a mask without element 0, an element the geometry does not admit (eval_symmetry_elements)."""
    mask = emit_mask(emit_symmetry, game, size)
    if mask == 0:
        return 0
    if mask & ~0xFF:
        raise ValueError(f"emit_symmetry: elements are 0..7, not {emit_symmetry!r}")
    if not mask & 1:
        raise ValueError(f"emit_symmetry: the mask needs element 0 (the identity), not {emit_symmetry!r}")
    admitted = eval_symmetry_elements(game, size)
    if any((mask >> s) & 1 and s not in admitted for s in range(8)):
        raise ValueError(f"emit_symmetry: {emit_symmetry!r} holds an element outside {admitted}, the elements this board's geometry admits")
    return mask


def _is_vanilla(evaluator):
    return evaluator is None or (isinstance(evaluator, (tuple, list)) and any(e is None for e in evaluator))


def check_surprise_weight(surprise_weight, evaluator=True, leaves_per_step=1):
    """surprise_weight = lambda -> float in [0, 1], or None for off.  OPT-IN policy surprise weighting (include/azk.h azk_set_surprise_weighting;
    DESIGN section 23): every move records kl = KL(recorded pi || the network's raw prior) and a keyed coin, and a finished game's recorded
    ply i is stored floor(w_i) + (coin_i < frac(w_i)) times, w_i = (1 - lambda) + lambda * n * kl_i / sum(kl).  lambda = 0 is a live setting
    (one copy each; kl and coin are still recorded).  Raises ValueError, before any engine exists, for what the engine refuses too - lambda
    outside [0, 1] or NaN, virtual loss - and for vanilla MCTS (evaluator None), which has no priors to be surprised about."""
    if surprise_weight is None:
        return None
    try:
        if isinstance(surprise_weight, bool):
            raise TypeError
        lam = float(surprise_weight)
    except (TypeError, ValueError):
        raise ValueError(f"surprise_weight must be a number lambda in [0, 1], not {surprise_weight!r}")
    if not 0.0 <= lam <= 1.0:                                     # (NaN fails both comparisons)
        raise ValueError(f"surprise_weight: lambda must lie in [0, 1] (None switches the option off), not {surprise_weight!r}")
    if _is_vanilla(evaluator):
        raise ValueError("surprise_weight: vanilla MCTS (evaluator None) is refused - it has no priors for the search to disagree with")
    if int(leaves_per_step) > 1:
        raise ValueError("surprise_weight does not combine with leaves_per_step > 1 (a virtual-loss search's visit counts are not the ones the weight was defined on)")
    return lam


def surprise_copies(kl, coin, lam, full=None):
    """The emission rule of surprise weighting for one finished game, for host buffers (train.save_data_to_buffer(copies=...)): kl, coin = the
    game's per-ply records (SelfPlayResult.kl / .coin), full = the playout cap's per-ply flags (None: every ply is recorded).  -> int array,
    copies per ply: with F the recorded plies, n = |F| and S = the sum of kl over F in ply order,
        w_i = S > 0 ? (1 - lam) + ((lam * n) * kl_i) / S : 1,    c_i = floor(w_i) + (coin_i < w_i - floor(w_i)),    0 outside F
    in float64, operation for operation what k_emit_alloc computes."""
    kl, coin = np.asarray(kl, np.float64), np.asarray(coin, np.float64)
    rec = np.ones(len(kl), bool) if full is None else np.asarray(full, bool)
    lam = np.float64(lam)
    n = np.float64(int(rec.sum()))
    S = np.float64(0.0)
    for i in np.nonzero(rec)[0]:
        S = S + kl[i]
    out = np.zeros(len(kl), np.int64)
    for i in np.nonzero(rec)[0]:
        w = (np.float64(1.0) - lam) + ((lam * n) * kl[i]) / S if S > 0.0 else np.float64(1.0)
        f = np.floor(w)
        out[i] = int(f) + (1 if coin[i] < w - f else 0)
    return out


def check_value_target(value_target, evaluator=True, leaves_per_step=1, gumbel_root=None):
    """value_target = r | (r, lam) -> (r, lam), floats in [0, 1], or None for off.  OPT-IN value targets (include/azk.h azk_set_value_target;
    DESIGN section 28): the z of every emitted tuple becomes (1 - r) * z + r * G, G the horizon-lam return over the game's own search values
    that ends in z (value_targets).  A number r means (r, 0.0), Leela's q-ratio; (1, lam) is a TD(lambda) return; r = 0 is a live setting
    (today's ring; q is still recorded).  Raises ValueError, before any engine exists, for what the engine refuses too - r or lam outside
    [0, 1] or NaN, virtual loss, a Gumbel root (its movers do not keep q) - and for vanilla MCTS (evaluator None), whose q is a rollout mean."""
    if value_target is None:
        return None
    try:
        if isinstance(value_target, bool):
            raise TypeError
        if isinstance(value_target, (tuple, list)):
            r, lam = value_target
            if isinstance(r, bool) or isinstance(lam, bool):
                raise TypeError
            r, lam = float(r), float(lam)
        else:
            r, lam = float(value_target), 0.0
    except (TypeError, ValueError):
        raise ValueError(f"value_target must be a number r or a pair (r, lam), both in [0, 1], not {value_target!r}")
    if not (0.0 <= r <= 1.0 and 0.0 <= lam <= 1.0):             # (NaN fails every comparison)
        raise ValueError(f"value_target: r and lam must lie in [0, 1] (None switches the option off), not {value_target!r}")
    if _is_vanilla(evaluator):
        raise ValueError("value_target: vanilla MCTS (evaluator None) is refused - its q is a rollout mean, not a search value to train on")
    if int(leaves_per_step) > 1:
        raise ValueError("value_target does not combine with leaves_per_step > 1 (a virtual-loss search is another search: its q is not the one the target was defined on)")
    if gumbel_root is not None:
        raise ValueError("value_target does not combine with gumbel_root (the Gumbel movers do not keep the per-ply q)")
    return r, lam


def value_targets(qs, winner, first_ply, r, lam):
    """The emission rule of value targets for one finished game, for host buffers (train.save_data_to_buffer(values=...)): qs = the game's
    per-ply q (SelfPlayResult.qs: root W / N at each move, the value for the mover's OPPONENT), the game's first searched ply first_ply
    (SelfPlayResult.open_plies), winner 0 / 1 / -1.  -> float64 array, one target per ply of qs: with v_i = -q_i and z_i the outcome from the
    mover's view (ply first_ply + i is moved by side (first_ply + i) & 1),
        G_last = (1 - lam) * v_last + lam * z_last,    G_i = (1 - lam) * v_i + lam * (-G_{i+1}),    t_i = (1 - r) * z_i + r * G_i
    in float64, operation for operation what k_emit_alloc computes (the ring stores np.float32(t_i))."""
    qs = np.asarray(qs, np.float64)
    r, lam = np.float64(r), np.float64(lam)
    one = np.float64(1.0)
    out = np.zeros(len(qs), np.float64)
    G = np.float64(0.0)
    for i in range(len(qs) - 1, -1, -1):
        side = (int(first_ply) + i) & 1
        z = np.float64(0.0 if winner == -1 else (1.0 if side == winner else -1.0))
        v = -qs[i]
        G = (one - lam) * v + lam * (z if i == len(qs) - 1 else -G)
        out[i] = (one - r) * z + r * G
    return out


def board_cells(game, size=None):
    """rows * cols of a game's board (its state_dim)."""
    if game == "tictactoe":
        return 9
    if game == "connect4":
        return 42
    rows, cols = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size or 0), int(size or 0))
    return rows * cols


def check_openings(openings, game, size=None, evaluator=True):
    """openings = (p_open, max_plies, spread) -> (float, int, int), or None for off.  OPT-IN random openings (include/azk.h azk_set_openings;
    DESIGN section 25): a game that starts in a slot is, with probability p_open, played forward 1..max_plies uniformly drawn legal plies inside
    the centred window of half-width spread (-1: the whole board) before its first search; those plies are not trained on.  Raises ValueError,
    before any engine exists, for what the engine refuses too - p_open outside [0, 1] or NaN, max_plies outside [1, state_dim - 1], a spread
    below -1 - and for vanilla MCTS on either side (evaluator None): its oracle is not driven from set-up positions."""
    if openings is None:
        return None
    try:
        p_open, max_plies, spread = openings
        if isinstance(p_open, bool) or int(max_plies) != max_plies or int(spread) != spread:
            raise ValueError
        p_open, max_plies, spread = float(p_open), int(max_plies), int(spread)
    except (TypeError, ValueError):
        raise ValueError(f"openings must be (p_open, max_plies, spread), not {openings!r}")
    if not 0.0 <= p_open <= 1.0:                                  # (NaN fails both comparisons)
        raise ValueError(f"openings: p_open must lie in [0, 1] (None switches the option off), not {p_open!r}")
    cells = board_cells(game, size)
    if not 1 <= max_plies <= cells - 1:
        raise ValueError(f"openings: max_plies must lie in [1, state_dim - 1 = {cells - 1}], not {max_plies!r}")
    if spread < -1:
        raise ValueError(f"openings: spread must be -1 (the whole board) or >= 0, not {spread!r}")
    if _is_vanilla(evaluator):
        raise ValueError("openings: vanilla MCTS (evaluator None) is refused - its rollouts are not driven from set-up positions")
    return p_open, max_plies, spread


def check_root_noise(root_noise, dirichlet=True, evaluator=True, gumbel_root=None, noise_fn=None):
    """root_noise = ("legal", alpha) | ("total", alpha_total) -> (str, float), or None for off.  OPT-IN root noise on the legal moves
    (include/azk.h azk_set_root_noise): a search's Dirichlet row is drawn over the actions that are legal in the position it
    starts from - "legal": Gamma(alpha) each, "total": Gamma(alpha_total / n) for n legal actions - instead of over the whole action vector.
    Raises ValueError, before any engine exists, for what the engine refuses too - an unknown mode, an alpha that is not finite and positive, a
    Gumbel root (its rows are Gumbel rows) - and for dirichlet=False (there is no row), vanilla MCTS on either side (evaluator None: it mixes no
    row in) and a caller-supplied noise_fn (its rows are the caller's)."""
    if root_noise is None:
        return None
    try:
        mode, alpha = root_noise
        if isinstance(alpha, bool) or not isinstance(mode, str):
            raise ValueError
        alpha = float(alpha)
    except (TypeError, ValueError):
        raise ValueError(f"root_noise must be ('legal', alpha) or ('total', alpha_total), not {root_noise!r}")
    if mode not in ("legal", "total"):
        raise ValueError(f"root_noise: the mode must be 'legal' or 'total', not {mode!r}")
    if not (alpha > 0.0 and math.isfinite(alpha)):                # (NaN fails the comparison)
        raise ValueError(f"root_noise: alpha must be finite and positive, not {alpha!r}")
    if not dirichlet:
        raise ValueError("root_noise shapes the root's Dirichlet row: dirichlet=False has none")
    if _is_vanilla(evaluator):
        raise ValueError("root_noise: vanilla MCTS (evaluator None) is refused - its searches mix no noise row in")
    if gumbel_root is not None:
        raise ValueError("root_noise does not combine with gumbel_root (its rows are Gumbel rows, not Dirichlet rows)")
    if noise_fn is not None:
        raise ValueError("root_noise does not combine with a caller-supplied noise_fn (the rows are then the caller's)")
    return mode, alpha


def check_move_temperature(move_temperature, n_sims, game, size=None, gumbel_root=None, tree_reuse=0):
    """move_temperature -> the (row_of_ply, weights, visit_offset, value_cutoff) of azk_set_move_temperature, or None for off.  OPT-IN move
    temperature (include/azk.h azk_set_move_temperature): how the played child is picked from a finished search.
    move_temperature is a schedule tau in one of move_temperature_setting's forms - a positive number, ("until", t, n_plies), ("halflife", t0,
    halflife[, t_final]), ("linear", t0, decay_plies[, t_final]) or a list of per-ply values - or a dict(tau=..., visit_offset=0,
    value_cutoff=None) that adds Leela's two guards.  n_sims is the engine's max_sims (the largest of a pair).  Raises ValueError, before any
    engine exists, for what the engine refuses too: a bad schedule, a row that overflows, a Gumbel root (its arg-max is the sample) and
    tree_reuse = 1 (a carried root child's visits are not bounded by max_sims; top-up, 2, is)."""
    if move_temperature is None:
        return None
    if isinstance(move_temperature, dict):
        extra = set(move_temperature) - {"tau", "visit_offset", "value_cutoff"}
        if extra or "tau" not in move_temperature:
            raise ValueError(f"move_temperature: a dict must have tau and may have visit_offset and value_cutoff, not {move_temperature!r}")
        tau, offset, cutoff = move_temperature["tau"], move_temperature.get("visit_offset", 0), move_temperature.get("value_cutoff")
    else:
        tau, offset, cutoff = move_temperature, 0, None
    max_sims = max(n_sims) if isinstance(n_sims, (tuple, list)) else n_sims
    setting = move_temperature_setting(tau, max_sims, board_cells(game, size), offset, cutoff)
    if gumbel_root is not None:
        raise ValueError("move_temperature does not combine with gumbel_root (the Gumbel arg-max is the sample)")
    if int(tree_reuse) == 1:
        raise ValueError("move_temperature does not combine with tree_reuse = 1 (a carried root child's visits are not bounded by max_sims, so the "
                         "table has no column for them; top-up, tree_reuse = 2, is bounded)")
    return setting


def check_kld_stop(kld_stop, n_sims, evaluator=True, leaves_per_step=1, gumbel_root=None):
    """kld_stop = (interval, min_gain[, min_sims]) -> (int, float, int), or None for off.  OPT-IN adaptive search budgets (include/azk.h
    azk_set_kld_stop): a search runs in segments of `interval` simulations and ends at the first checkpoint between two
    segments at which the KL divergence its root's visit distribution gained per simulation since the last checkpoint is below min_gain, not
    before it has run min_sims new simulations.  n_sims is the engine's max_sims (the largest of a pair).  Raises ValueError, before any engine
    exists, for what the engine refuses too - an interval outside [1, n_sims], a min_gain that is not finite and positive, a negative min_sims,
    virtual loss, a Gumbel root (its halving table needs a fixed number of simulations) - and for vanilla MCTS on either side (evaluator None:
    it runs whole searches inside one launch, without checkpoints)."""
    if kld_stop is None:
        return None
    try:
        interval, min_gain, min_sims = kld_stop if len(kld_stop) == 3 else (kld_stop[0], kld_stop[1], 0) if len(kld_stop) == 2 else (None, None, None)
        if isinstance(interval, bool) or isinstance(min_sims, bool) or int(interval) != interval or int(min_sims) != min_sims:
            raise ValueError
        interval, min_gain, min_sims = int(interval), float(min_gain), int(min_sims)
    except (TypeError, ValueError):
        raise ValueError(f"kld_stop must be (interval, min_gain) or (interval, min_gain, min_sims), not {kld_stop!r}")
    max_sims = max(n_sims) if isinstance(n_sims, (tuple, list)) else n_sims
    if not 1 <= interval <= max_sims:
        raise ValueError(f"kld_stop: interval must lie in [1, n_sims = {max_sims}], not {interval!r}")
    if not (min_gain > 0.0 and math.isfinite(min_gain)):          # (NaN fails the comparison)
        raise ValueError(f"kld_stop: min_gain must be finite and positive, not {min_gain!r}")
    if min_sims < 0:
        raise ValueError(f"kld_stop: min_sims must not be negative, not {min_sims!r}")
    if _is_vanilla(evaluator):
        raise ValueError("kld_stop: vanilla MCTS (evaluator None) is refused - it runs whole searches inside one launch, without checkpoints")
    if int(leaves_per_step) > 1:
        raise ValueError("kld_stop does not combine with leaves_per_step > 1 (a virtual-loss search has several leaves in flight: no checkpoint finds its tree complete)")
    if gumbel_root is not None:
        raise ValueError("kld_stop does not combine with gumbel_root (the halving table needs a fixed number of simulations)")
    return interval, min_gain, min_sims


def check_lead_stop(lead_stop, n_sims, evaluator=True, leaves_per_step=1, gumbel_root=None, kld_stop=None):
    """lead_stop = (interval, factor[, min_sims]) -> (int, float, int), or None for off.  OPT-IN adaptive search budgets, the lead rule
    (include/azk.h azk_set_lead_stop): a search runs in segments of `interval` simulations and ends at the first checkpoint
    between two segments at which the simulations left are fewer than factor * (the most-visited root child's lead over the second), not before
    it has run min_sims new simulations; at factor 1 the first most-visited child is the full search's.  n_sims is the engine's max_sims (the
    largest of a pair); kld_stop is the KLD rule's checked setting where both are given - the two share one interval.  Raises ValueError,
    before any engine exists, for what the engine refuses too - an interval outside [1, n_sims] or unlike kld_stop's, a factor that is not
    finite and positive, a negative min_sims, virtual loss, a Gumbel root - and for vanilla MCTS on either side (evaluator None)."""
    if lead_stop is None:
        return None
    try:
        interval, factor, min_sims = lead_stop if len(lead_stop) == 3 else (lead_stop[0], lead_stop[1], 0) if len(lead_stop) == 2 else (None, None, None)
        if isinstance(interval, bool) or isinstance(min_sims, bool) or int(interval) != interval or int(min_sims) != min_sims:
            raise ValueError
        interval, factor, min_sims = int(interval), float(factor), int(min_sims)
    except (TypeError, ValueError):
        raise ValueError(f"lead_stop must be (interval, factor) or (interval, factor, min_sims), not {lead_stop!r}")
    max_sims = max(n_sims) if isinstance(n_sims, (tuple, list)) else n_sims
    if not 1 <= interval <= max_sims:
        raise ValueError(f"lead_stop: interval must lie in [1, n_sims = {max_sims}], not {interval!r}")
    if not (factor > 0.0 and math.isfinite(factor)):              # (NaN fails the comparison)
        raise ValueError(f"lead_stop: factor must be finite and positive, not {factor!r}")
    if min_sims < 0:
        raise ValueError(f"lead_stop: min_sims must not be negative, not {min_sims!r}")
    if _is_vanilla(evaluator):
        raise ValueError("lead_stop: vanilla MCTS (evaluator None) is refused - it runs whole searches inside one launch, without checkpoints")
    if int(leaves_per_step) > 1:
        raise ValueError("lead_stop does not combine with leaves_per_step > 1 (a virtual-loss search has several leaves in flight: no checkpoint finds its tree complete)")
    if gumbel_root is not None:
        raise ValueError("lead_stop does not combine with gumbel_root (the halving table needs a fixed number of simulations)")
    if kld_stop is not None and int(kld_stop[0]) != interval:
        raise ValueError(f"lead_stop and kld_stop share one interval, not {interval!r} and {kld_stop[0]!r}")
    return interval, factor, min_sims


def mask_elements(mask):
    """The elements of an emission mask, ascending."""
    return tuple(s for s in range(8) if (mask >> s) & 1)


def _refuse_vanilla_resign(resign, evaluator):
    if resign is not None and (evaluator is None or (isinstance(evaluator, (tuple, list)) and any(e is None for e in evaluator))):
        raise ValueError("resign: vanilla MCTS (evaluator None) is refused - its q is a rollout mean and no threshold is defined for it")


class SelfPlayResult:
    __slots__ = ("boards", "actions", "pis", "qs", "winner", "cells", "replay_base", "full", "resigned", "kl", "coin", "open_plies", "opening", "root_status", "sims")

    def __init__(self):
        self.boards, self.actions, self.pis, self.qs, self.winner, self.cells = [], [(-1, -1)], [], [], None, []
        self.full = []               # per ply: was its search a full one (always True without playout_cap); only those plies are trained on
        self.replay_base = None      # first tuple index in the DeviceReplay stream (when a replay ring is attached)
        self.resigned = False        # the game ended by resignation (resign=...): winner is then the side that did not concede
        self.open_plies = 0          # plies of the game's random opening (openings=...): boards[0] is the position after them, ply open_plies
        self.opening = []            # ... and the cells they were played on, in order (the players alternate from player 0)
        self.root_status = []        # per ply with solver=True: the root's proven status as the mover sees it (0 unknown, 1 wins, 2 loses, 3 draw)
        self.kl, self.coin = [], []  # per ply with surprise_weight=...: KL(recorded pi || raw prior) and the ply's coin (empty without)
        self.sims = []               # per ply with kld_stop=... or lead_stop=...: the new simulations the ply's search ran (empty without)

    def as_reference_tuple(self):
        """(boards, actions, policy_distributions, qs, winner) - gomoku.py:164"""
        return self.boards, self.actions, self.pis, self.qs, self.winner


def self_play_batch(game, evaluator, n_games, n_sims, size=None, seed=0, first_global_game=0, dirichlet=True,
                    alpha=0.03, noise_fn=None, uniform_fn=None, device=0, leaf_dtype="float32", engine=None,
                    max_moves=None, sample_until=None, stats=None, replay=None, cache_entries=0, vanilla_rng=None, cache_shared=False,
                    budget_stepping=False, leaves_per_step=1, tree_reuse=0, playout_cap=None, resign=None, forced_playouts=None,
                    eval_symmetry=None, emit_symmetry=None, surprise_weight=None, gumbel_root=None, openings=None, openings_seed=None,
                    openings_first_game=None, puct=None, move_temperature=None, value_target=None, solver=None, root_noise=None, kld_stop=None,
                    lead_stop=None):
    """Play n_games games to the end in one batch.

    evaluator(boards[n,F,R,C] CUDA) -> (logits [n,A], values [n] | [n,1]).
    RNG: by default Dirichlet noise and sampling uniforms come from the engine's counter-based generator
    keyed by (seed, first_global_game + g, move) - independent of how games are sharded over GPUs.
    noise_fn(move_idx) -> float64 [G, A] and uniform_fn(move_idx) -> float64 [G] (numpy) override it
    (that is how parity tests inject the reference's recorded np.random draws).
    An evaluator of None plays vanilla MCTS (random rollouts on the device, mcts.py:57-79) - for a whole game
    (self_play(None, n): greedy moves, tictactoe.py:117 / gomoku.py:146) or for one side of an (ev0, ev1) pair
    (test.compare(Game, None, model, ...), main.py:76).  tree_reuse (OPT-IN, changes search results; azk.h azk_config.tree_reuse): 1 = every
    search after a game's first starts on the subtree under the move that was played and runs n_sims more simulations, 2 = only as
    many as bring the root back to n_sims visits (driven by the simulation budget).  vanilla_rng: uint32 [G, 625] MT19937 states (default: one
    np.random.RandomState per global game index derived from `seed`).  playout_cap = (p_full, n_fast) (OPT-IN, check_playout_cap): per ply a
    coin keyed (seed, global game, move) makes the search full or fast; SelfPlayResult.full records it and a replay ring gets the full plies only.
    resign = (v_resign, p_never[, min_ply]) (OPT-IN, check_resign): a game may end by resignation - SelfPlayResult.resigned, winner = the
    other side, z and the replay tuples as for any finished game.  forced_playouts = k (OPT-IN, check_forced_playouts): forced playouts at the
    root; SelfPlayResult.pis and the replay tuples carry the PRUNED pi of every full search, the moves are those of the raw visits.
    eval_symmetry = True | ("fixed", s) (OPT-IN, check_eval_symmetry): every leaf is evaluated in an orientation keyed by (seed, its position),
    or in the one given.  emit_symmetry = "board" | "none" | elements (OPT-IN, check_emit_symmetry): the replay ring gets every ply from the
    third on once per element of the mask, on every geometry (Connect4 and non-square Gomoku included); an engine handed in must have
    been created with the same mask (ValueError).  surprise_weight = lambda (OPT-IN, check_surprise_weight): every ply records its policy surprise
    and coin (SelfPlayResult.kl / .coin) and the replay ring gets each recorded ply as often as its weight says (surprise_copies).
    gumbel_root = (m, c_visit, c_scale) (OPT-IN, check_gumbel_root): a Gumbel root search of n_sims simulations per move - the engine's Gumbel
    rows (or noise_fn's) where the Dirichlet rows go, SelfPlayResult.pis and the replay tuples carry softmax(logits + sigma(completed Q)).
    openings = (p_open, max_plies, spread) (OPT-IN, check_openings): every game starts from a drawn position with that probability, keyed
    (openings_seed or seed, (openings_first_game or first_global_game) + g, move 0); SelfPlayResult.open_plies counts the opening's plies,
    SelfPlayResult.opening holds their cells in order, boards[0] is the position after them, and a replay ring does not get them.  With an
    (evaluator0, evaluator1) pair the games of the batch are no longer at one ply, so the pair is told apart per game: every leaf of a game
    whose root has player p to move is evaluated by evaluator p (both run over the step's batch, Engine.leaf_flags says which game a row
    belongs to); the two sides then search the same number of simulations (ValueError otherwise).  puct = (c, fpu) (OPT-IN, check_puct):
    every selection of every network search scores a child with the exploration rate c - a number, a tuple (c_init, c_base) or a table over
    the selecting node's visit count - and an unvisited child by the first-play urgency fpu (None, ("absolute", v_tree[, v_root]) or
    ("reduction", r_tree[, r_root])); with an (evaluator0, evaluator1) pair both sides search under it.  move_temperature (OPT-IN,
    check_move_temperature): a schedule tau, or dict(tau=, visit_offset=, value_cutoff=) - every move is picked by the engine's weight table
    instead of "sample in proportion to the visits while move_count < sample_until", which is then not looked at; the recorded pis stay the raw
    visit distributions.  ("until", 1.0, sample_until) plays the games of a call without the option.  value_target = r | (r, lam) (OPT-IN,
    check_value_target): the replay ring gets (1 - r) * z + r * G as the z of every tuple, G the horizon-lam return over the game's own search
    values (value_targets(SelfPlayResult.qs, ...) is the same rule on the host); the games, states and pis do not change.  solver = True
    (OPT-IN, check_solver): every search keeps exact game-end proofs (Engine.set_solver); SelfPlayResult.root_status gets each move's root
    status as the mover sees it (0 unknown, 1 wins, 2 loses, 3 draw).  root_noise = ("legal", alpha) | ("total", alpha_total) (OPT-IN,
    check_root_noise): every search's Dirichlet row is drawn over the legal moves of the position it starts from (Engine.gen_root_noise where
    gen_noise is called); `alpha` is then not looked at.  kld_stop = (interval, min_gain[, min_sims]) (OPT-IN, check_kld_stop): every search runs in
    segments and ends when its root's visit distribution stops changing (Engine.search_budget's checkpoints; budget stepping is switched on);
    SelfPlayResult.sims gets the new simulations each ply's search ran.  lead_stop = (interval, factor[, min_sims]) (OPT-IN, check_lead_stop;
    alone or beside kld_stop, one interval): a search ends once the simulations left are fewer than factor * (the most-visited root child's
    lead over the second) - at factor 1 and sample_until = 0 the games are the option-off games move for move, for fewer simulations.
    """
    import torch
    rnz = check_root_noise(root_noise, dirichlet, evaluator, gumbel_root, noise_fn)
    opn = check_openings(openings, game, size, evaluator)
    by_game = opn is not None and isinstance(evaluator, (tuple, list))       # the pair is told apart per game, not by the batch's ply
    if by_game and isinstance(n_sims, (tuple, list)) and len(set(n_sims)) != 1:
        raise ValueError(f"openings: with an (evaluator0, evaluator1) pair both sides search the same number of simulations, not {n_sims!r} - "
                         "opened games are not all at the same ply, so one search serves movers of both sides")
    emit = check_emit_symmetry(emit_symmetry, game, size)
    if engine is not None and engine.emit_elements != emit:
        raise ValueError(f"self_play_batch: emit_symmetry={emit_symmetry!r} is mask {emit:#x}, the engine handed in was created with {engine.emit_elements:#x}")
    cap = check_playout_cap(playout_cap, n_sims, leaves_per_step)
    rsg = check_resign(resign, leaves_per_step)
    fpk = check_forced_playouts(forced_playouts, evaluator, dirichlet, leaves_per_step)
    sym = check_eval_symmetry(eval_symmetry, game, size, evaluator, leaves_per_step, seed)
    lam = check_surprise_weight(surprise_weight, evaluator, leaves_per_step)
    gum = check_gumbel_root(gumbel_root, n_sims, evaluator, dirichlet, leaves_per_step, tree_reuse, cap, fpk, lam)
    pct = puct if check_puct(puct, evaluator, leaves_per_step, fpk, gum) is not None else None
    tmp = check_move_temperature(move_temperature, engine.max_sims if engine is not None else n_sims, game, size, gum,
                                 engine.tree_reuse if engine is not None else tree_reuse)
    vtg = check_value_target(value_target, evaluator, leaves_per_step, gum)
    slv = check_solver(solver, evaluator, leaves_per_step, fpk, gum, pct, engine.tree_reuse if engine is not None else tree_reuse)
    kls = check_kld_stop(kld_stop, engine.max_sims if engine is not None else n_sims, evaluator, leaves_per_step, gum)
    lds = check_lead_stop(lead_stop, engine.max_sims if engine is not None else n_sims, evaluator, leaves_per_step, gum, kls)
    _refuse_vanilla_resign(rsg, evaluator)
    if cap is not None and (evaluator is None or (isinstance(evaluator, (tuple, list)) and any(e is None for e in evaluator))):
        raise ValueError("playout_cap caps network searches; vanilla MCTS (evaluator None) has no budget stepping")
    max_sims = max(n_sims) if isinstance(n_sims, (tuple, list)) else n_sims
    eng = engine or Engine(game, n_games, max_sims, size=size, device=device, leaf_dtype=leaf_dtype, cache_entries=cache_entries,
                           cache_shared=cache_shared, leaves_per_step=leaves_per_step, tree_reuse=tree_reuse,
                           emit_symmetry=mask_elements(emit) if emit else None)
    if cap is not None:
        eng.set_playout_cap(cap[0], cap[1], seed, first_global_game)
    if rsg is not None:
        eng.set_resign(rsg[0], rsg[1], rsg[2], seed, first_global_game)
    if fpk is not None:
        eng.set_forced_playouts(fpk)
    if sym is not None:
        eng.set_eval_symmetry(*sym)
    if lam is not None:
        eng.set_surprise_weighting(lam, seed, first_global_game)
    if gum is not None:
        eng.set_gumbel_root(gum[0], n_sims, gum[1], gum[2])
    if pct is not None:
        eng.set_puct(*pct)
    if tmp is not None:
        eng.set_move_temperature(*tmp)
    if vtg is not None:
        eng.set_value_target(*vtg)
    if slv is not None:
        eng.set_solver(True)
    elif eng.solver:                                              # an engine handed in with the option still on
        eng.set_solver(False)
    if rnz is not None:
        eng.set_root_noise(*rnz)
    elif eng.root_noise is not None:
        eng.clear_root_noise()
    if eng.kld_stop is not None:                                  # an engine handed in with the option still on (and before the other rule
        eng.clear_kld_stop()                                      # is set: the two must agree on the interval)
    if eng.lead_stop is not None:
        eng.clear_lead_stop()
    if kls is not None:
        eng.set_kld_stop(*kls)
    if lds is not None:
        eng.set_lead_stop(*lds)
    # virtual-loss, top-up and capped engines, and engines with adaptive search budgets, are driven by the simulation budget
    budget_stepping = budget_stepping or eng.K > 1 or eng.tree_reuse == 2 or eng.playout_cap is not None or eng.adaptive
    assert eng.G == n_games
    G, A = eng.G, eng.action_dim
    eng.reset_games()
    results = [SelfPlayResult() for _ in range(G)]
    if opn is not None:
        eng.set_openings(opn[0], opn[1], opn[2], seed if openings_seed is None else openings_seed,
                         first_global_game if openings_first_game is None else openings_first_game)
        eng.open_pending(0)
        for r, n, cells in zip(results, eng.open_plies().cpu().numpy(), eng.opening_actions()):
            r.open_plies, r.opening = int(n), cells
    elif eng.openings is not None:                                # an engine handed in with the option still on: this batch starts from empty boards
        eng.clear_openings()
    active = np.ones(G, bool)
    su = SAMPLE_UNTIL[game] if sample_until is None else sample_until
    evs = list(evaluator) if isinstance(evaluator, (tuple, list)) else [evaluator]
    if any(e is None for e in evs):
        if vanilla_rng is None:
            from azk import mt_state_from_numpy
            vanilla_rng = np.stack([mt_state_from_numpy(np.random.RandomState(
                (int(seed) * 2654435761 + first_global_game + g) % (1 << 32)).get_state()) for g in range(G)])
        eng.vanilla_set_rng(vanilla_rng)
        if evaluator is None and sample_until is None:
            su = 0                                                # model=None: max_visit_child every move
    vanilla_chunk = 64 if eng.rows * eng.cols > 64 else None     # bounds one launch's run time on the big boards
    move = 0
    while active.any():
        if noise_fn is not None:
            nz = noise_fn(move)
            noise = torch.from_numpy(np.ascontiguousarray(nz, np.float64)).to(eng.device) if nz is not None else None
            uni = None
        elif gum is not None:
            noise, uni = eng.gen_gumbel(seed, first_global_game, move), None
        elif rnz is not None:                                     # rows over the legal moves of the positions as they stand
            noise, uni = eng.gen_root_noise(seed, first_global_game, move)
        else:
            noise, uni = eng.gen_noise(seed, first_global_game, move, alpha, want_noise=dirichlet)
        if uniform_fn is not None:
            uni = torch.from_numpy(np.ascontiguousarray(uniform_fn(move), np.float64)).to(eng.device)
        # an (evaluator0, evaluator1) pair plays the two sides (test.compete, test.py:79-84); all games are at the same ply
        ev = evaluator[move & 1] if isinstance(evaluator, (tuple, list)) else evaluator
        ns = n_sims[move & 1] if isinstance(n_sims, (tuple, list)) else n_sims
        cells_before, to_move, _ = eng.get_positions()
        if by_game:
            side = torch.from_numpy(np.ascontiguousarray(to_move, np.int64)).to(eng.device)

            def ev(x, side=side):
                rows = torch.nonzero(eng.leaf_flags()).reshape(-1)[: x.shape[0]] // eng.K     # the game of each row: rows are in ascending slot order
                first = side[rows] == 0
                (l0, v0), (l1, v1) = evaluator[0](x), evaluator[1](x)
                return torch.where(first[:, None], l0, l1), torch.where(first, v0.reshape(-1), v1.reshape(-1))
        if ev is None:
            eng.vanilla_search(ns, chunk=vanilla_chunk)
        elif budget_stepping:
            eng.search_budget(ev, ns, noise if dirichlet else None, move_index=move)
        else:
            eng.search(ev, ns, noise if dirichlet else None)
        full_h = eng.search_full().cpu().numpy() if eng.playout_cap is not None else None
        status_h = eng.solver_status() if eng.solver else None
        sims_h = eng.search_sims().cpu().numpy() if eng.adaptive else None
        pi, q, _ = eng.root_stats()
        if eng.forced_playouts is not None or eng.gumbel_root is not None:
            pi = eng.root_policy_target()                         # what advance records: pruned where the search was a forced one; a Gumbel root's target
        chosen, winner, done = eng.advance(uni, su, move_index=move)
        resigned_h = eng.resigned().cpu().numpy() if eng.resign is not None else None
        kl_h, coin_h = [t.cpu().numpy() for t in eng.surprise()] if eng.surprise_weight is not None else (None, None)
        bases = eng.emit_finished(replay).cpu().numpy() if replay is not None else None     # train.save_data_to_buffer on device
        pi_h, q_h = pi.cpu().numpy(), q.cpu().numpy()
        chosen_h, winner_h, done_h = chosen.cpu().numpy(), winner.cpu().numpy(), done.cpu().numpy()
        for g in np.nonzero(active)[0]:
            r = results[g]
            r.boards.append(cells_to_board(cells_before[g], eng.planes, eng.rows, eng.cols, to_move[g]))
            r.pis.append(pi_h[g].copy())
            r.qs.append(float(q_h[g]))
            r.full.append(True if full_h is None else bool(full_h[g]))
            if status_h is not None:
                r.root_status.append(int(status_h[g]))
            if kl_h is not None:
                r.kl.append(float(kl_h[g]))
                r.coin.append(float(coin_h[g]))
            if sims_h is not None:
                r.sims.append(int(sims_h[g]))
            c = int(chosen_h[g])
            r.cells.append(c)
            r.actions.append((c // eng.cols, c % eng.cols))
            if done_h[g]:
                r.winner = int(winner_h[g])
                r.resigned = bool(resigned_h[g]) if resigned_h is not None else False
                active[g] = False
                if bases is not None:
                    r.replay_base = int(bases[g])
        move += 1
        if max_moves is not None and move >= max_moves:
            break
    eng.check_error()
    if stats is not None:
        stats.update(eng.counters())
        stats["moves"] = move
    return results


class _Half:
    """State of one independently stepped group of games (an engine + its static step buffers + pinned records)."""

    def __init__(self, torch, eng, dirichlet):
        self.eng = eng
        e = eng
        self.stats = torch.zeros(8, dtype=torch.int64, device=e.device)
        pin = dict(pin_memory=True)
        self.h_pi = torch.zeros((e.G, e.action_dim), dtype=torch.float64, **pin)
        self.h_q = torch.zeros(e.G, dtype=torch.float64, **pin)
        self.h_chosen = torch.zeros(e.G, dtype=torch.int32, **pin)
        self.h_winner = torch.zeros(e.G, dtype=torch.int32, **pin)
        self.h_done = torch.zeros(e.G, dtype=torch.int32, **pin)
        self.h_stats = torch.zeros(8, dtype=torch.int64, **pin)
        self.h_full = torch.ones(e.G, dtype=torch.uint8, **pin)      # playout cap: kind of each slot's search (1 = full); all ones without
        self.h_resigned = torch.zeros(e.G, dtype=torch.uint8, **pin)  # resignation: 1 = the slot's move conceded the game; all zeros without
        self.h_kl = torch.zeros(e.G, dtype=torch.float64, **pin)      # surprise weighting: kl and coin of each slot's move; zeros without
        self.h_coin = torch.zeros(e.G, dtype=torch.float64, **pin)
        self.h_sims = torch.zeros(e.G, dtype=torch.int32, **pin)      # adaptive search budgets: new simulations of each slot's search; zeros without
        # static buffers so a captured step graph always sees the same addresses
        self.noise_buf = torch.zeros((e.G, e.action_dim), dtype=torch.float64, device=e.device) if dirichlet else None
        self.logits_buf = torch.zeros((e.slots, e.action_dim), dtype=torch.float32, device=e.device)
        self.values_buf = torch.zeros(e.slots, dtype=torch.float32, device=e.device)
        self.uni = None


def concurrent_streams(torch, device, n, spin_cycles=600_000):
    """n HIP streams whose kernels really run side by side.  HIP hands its streams out over a few hardware queues (four per priority by
    default) and two streams on one queue serialize - measured on this pool: of six fresh streams three pairs shared a queue, and the
    two streams the game groups used to get were such a pair (rocprofv3 kernel trace: same Queue_Id, 0.1 % of the time with two kernels
    in flight).  So candidates are probed pairwise with a one-thread spin kernel: two spins that take the time of one overlap."""
    import time
    cand = [torch.cuda.Stream(device=device) for _ in range(8)] + [torch.cuda.Stream(device=device, priority=-1) for _ in range(2)]
    for st in cand:                                  # queues are created at first use
        with torch.cuda.stream(st):
            torch.cuda._sleep(1000)
    torch.cuda.synchronize(device)

    def spins(a, b):
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        for st in (a, b):
            with torch.cuda.stream(st):
                torch.cuda._sleep(spin_cycles)
        torch.cuda.synchronize(device)
        return time.perf_counter() - t0
    serial = min(spins(cand[0], cand[0]) for _ in range(2))
    chosen = [cand[0]]
    for st in cand[1:]:
        if len(chosen) == n:
            break
        if all(min(spins(st, c) for _ in range(2)) < 0.75 * serial for c in chosen):
            chosen.append(st)
    if len(chosen) < n:
        if n == 2:
            # a noisy probe (another tenant on the box): a normal- and a high-priority stream never share a queue
            return [cand[0], cand[-1]]
        raise RuntimeError(f"only {len(chosen)} of {n} streams found that run concurrently on this device")
    return chosen


def _evaluate_step(ev, e, h, from_leaves, timer=None):
    """The evaluator hand-off of one step of either runner: the evaluator runs over engine e's (fixed-size) leaf buffer - or reads
    e's pending leaves itself (from_leaves) - honours the device-side leaf count and writes the step buffers of h.  Everything lent
    to the evaluator is taken back afterwards: the step's row count belongs to THIS engine, and an evaluator shared with another
    runner (or called directly afterwards) must not keep honouring it."""
    if hasattr(ev, "leaf_source"):
        ev.leaf_source = e.leaf_source() if from_leaves else None
    had_fast = getattr(ev, "fast_outputs", False)
    if hasattr(ev, "live_count"):
        ev.live_count, ev.fast_outputs = e.n_leaf, True
    if hasattr(ev, "kernel_timers"):
        if timer is None:
            ev.kernel_timers = None
        elif getattr(ev, "fused_embed_pool", False):
            ev.kernel_timers = (timer.child("k_embed_pool"), timer.child("k_tail"))
        else:
            ev.kernel_timers = (timer.child("k_embed"), timer.child("k_cls_pool"), timer.child("k_tail"))
    if hasattr(ev, "out_buffers"):
        ev.out_buffers = (h.logits_buf, h.values_buf)
    logits, values = ev(e.leaf_boards)
    if logits.data_ptr() != h.logits_buf.data_ptr():        # evaluators that do not write the step buffers themselves
        h.logits_buf.copy_(logits)
        h.values_buf.copy_(values.reshape(-1))
    if hasattr(ev, "out_buffers"):
        ev.out_buffers = None
    if hasattr(ev, "leaf_source"):
        ev.leaf_source = None
    if hasattr(ev, "live_count"):
        ev.live_count, ev.fast_outputs = None, had_fast


class SelfPlayRunner:
    """Continuous self-play: G slots advance one move per `play_move()`; a slot whose game ends restarts
    from an empty board in the same call (azk_recycle_finished), so every move does G searches.
    Per move the records the reference's self_play keeps (pi, q, action, winner; gomoku.py:138-146)
    are copied to pinned host buffers; `on_records` (optional) receives them.

    `n_split` groups of G/n_split games are stepped on separate HIP streams inside ONE captured graph: the
    latency-bound kernels of one group (tree walk, the cls-row tail) run under the bandwidth/VALU-bound kernels
    of the other.  Groups are independent games, so this changes no result.

    RNG key = (seed, first_global_game + slot, move counter): results do not depend on the sharding.

    playout_cap = (p_full, n_fast) (OPT-IN, check_playout_cap): every search is full or fast by a coin of the same key; the searches run under
    the simulation budget (as tree_reuse=2), `record_full` (uint8 [group size], valid inside on_records) tells the kind of each record, and
    the replay ring gets the plies of full searches only.

    resign = (v_resign, p_never[, min_ply]) (OPT-IN, check_resign; with any tree_reuse and with playout_cap): after a move the mover concedes
    when the recorded q >= v_resign; the slot's record then carries the conceded winner and done, `record_resigned` (uint8 [group size], valid
    inside on_records) is 1 for it, and the game is emitted and recycled like any finished game.  resign_stats() counts the outcomes.

    forced_playouts = k (OPT-IN, check_forced_playouts; with any tree_reuse, playout_cap and resign): forced playouts at the root of every
    (full) search; the records' pi and the replay ring carry the pruned pi, the moves are those of the raw visits.

    eval_symmetry = True | ("fixed", s) (OPT-IN, check_eval_symmetry; with everything above): every leaf is evaluated in an orientation keyed by
    (seed, its position) - or in the one given - and its logits are turned back; set at construction, before any graph is captured.

    emit_symmetry = "board" | "none" | elements (OPT-IN, check_emit_symmetry; with everything above): the replay ring gets every ply from the
    third on once per element of the mask, on every geometry; the engines are created with it.

    surprise_weight = lambda (OPT-IN, check_surprise_weight; with everything above): every move records its policy surprise and coin -
    `record_surprise` ((kl, coin), float64 [group size] each, valid inside on_records) - and the replay ring gets each recorded ply as often as
    its weight says.

    gumbel_root = (m, c_visit, c_scale) (OPT-IN, check_gumbel_root; with resign, eval_symmetry, emit_symmetry, the eval cache, plain and budget
    stepping): every search is a Gumbel root search of n_sims simulations; the groups get Gumbel rows of the same key where they get Dirichlet
    rows, the records' pi and the replay ring carry softmax(logits + sigma(completed Q)).

    openings = (p_open, max_plies, spread) (OPT-IN, check_openings; with everything above): a game that starts in a slot - the first games and
    every recycled one - is, with that probability, played forward a few drawn plies before its first search (Engine.open_pending, outside the
    captured graphs), keyed (openings_seed or seed, (openings_first_game or first_global_game) + slot, the move counter of that search).  Records
    start at the first searched ply; the replay ring does not get the opening's plies; finished_plies counts them, plies_played does not.

    puct = (c, fpu) (OPT-IN, check_puct; with everything above except forced_playouts and gumbel_root): every selection of every search uses
    the exploration rate c (a number, a tuple (c_init, c_base), or a table over the selecting node's visit count) and the first-play urgency
    fpu (None, ("absolute", v_tree[, v_root]) or ("reduction", r_tree[, r_root])); set at construction, before any graph is captured.

    move_temperature (OPT-IN, check_move_temperature; with everything above except gumbel_root and tree_reuse = 1): a schedule tau or
    dict(tau=, visit_offset=, value_cutoff=) - every move is picked by the engine's weight table instead of the reference's "sample while
    move_count < sample_until"; the records' pis stay raw visit distributions.  move_temperature_stats() sums the groups' four counters.

    value_target = r | (r, lam) (OPT-IN, check_value_target; with everything above except gumbel_root and leaves_per_step > 1): the replay ring
    gets (1 - r) * z + r * G as the z of every tuple, G the horizon-lam return over the game's own search values (value_targets); the games,
    the records, states and pis do not change.

    solver = True (OPT-IN, check_solver; with everything above except forced_playouts, gumbel_root, puct, tree_reuse and leaves_per_step > 1):
    every search keeps exact game-end proofs (Engine.set_solver); solver_stats() sums the groups' six counters.

    root_noise = ("legal", alpha) | ("total", alpha_total) (OPT-IN, check_root_noise; with everything above except gumbel_root): every search's
    Dirichlet row is drawn over the legal moves of the position it starts from - gen_root_noise where gen_noise is called, behind the recycle and
    the openings of the move before; `alpha` is then not looked at.

    kld_stop = (interval, min_gain[, min_sims]) (OPT-IN, check_kld_stop; with everything above except gumbel_root and leaves_per_step > 1): every
    search runs in segments of `interval` simulations and ends at the first checkpoint at which its root's visit distribution gained less than
    min_gain of KL divergence per simulation (Engine.kld_checkpoint between the segments, outside the captured graphs).  It turns budget stepping
    on, like top-up.  `record_sims` (int32 [group size], valid inside on_records) holds the new simulations each record's search ran;
    kld_stats() sums the groups' four counters.

    lead_stop = (interval, factor[, min_sims]) (OPT-IN, check_lead_stop; alone or beside kld_stop, which it is driven like): every search ends
    once the simulations left are fewer than factor * (the most-visited root child's lead over the second).  `record_sims` is filled under
    either rule; lead_stats() sums the groups' five counters.
    """

    def __init__(self, game, evaluator, n_games, n_sims, size=None, seed=0, first_global_game=0, dirichlet=True,
                 alpha=0.03, device=0, leaf_dtype="float32", recycle=True, on_records=None, kernel_timer=None,
                 use_graph=False, n_split=1, replay=None, cache_entries=0, cache_shared=False, budget_stepping=False, per_launch=8,
                 steps_per_graph=32,
                 leaves_per_step=1, tree_reuse=0, playout_cap=None, resign=None, forced_playouts=None, eval_symmetry=None, emit_symmetry=None,
                 surprise_weight=None, gumbel_root=None, openings=None, openings_seed=None, openings_first_game=None, puct=None,
                 move_temperature=None, value_target=None, solver=None, root_noise=None, kld_stop=None, lead_stop=None):
        import torch
        self.root_noise = check_root_noise(root_noise, dirichlet, evaluator, gumbel_root)
        self.openings = check_openings(openings, game, size, evaluator)
        self.gumbel_root = check_gumbel_root(gumbel_root, n_sims, evaluator, dirichlet, leaves_per_step, tree_reuse, playout_cap, forced_playouts,
                                             surprise_weight)
        self.kld_stop = check_kld_stop(kld_stop, n_sims, evaluator, leaves_per_step, self.gumbel_root)
        self.lead_stop = check_lead_stop(lead_stop, n_sims, evaluator, leaves_per_step, self.gumbel_root, self.kld_stop)
        self.adaptive = self.kld_stop is not None or self.lead_stop is not None      # searches run in segments: either rule
        self.record_sims = None
        self.solver = check_solver(solver, evaluator, leaves_per_step, forced_playouts, gumbel_root, puct, tree_reuse)
        self.value_target = check_value_target(value_target, evaluator, leaves_per_step, self.gumbel_root)
        self.move_temperature = check_move_temperature(move_temperature, n_sims, game, size, self.gumbel_root, tree_reuse)
        self.puct = puct if check_puct(puct, evaluator, leaves_per_step, forced_playouts, gumbel_root) is not None else None
        self.emit_elements = check_emit_symmetry(emit_symmetry, game, size)
        self.surprise_weight = check_surprise_weight(surprise_weight, evaluator, leaves_per_step)
        self.record_surprise = None
        self.eval_symmetry = check_eval_symmetry(eval_symmetry, game, size, evaluator, leaves_per_step, seed)
        self.playout_cap = check_playout_cap(playout_cap, n_sims, leaves_per_step)
        self.resign = check_resign(resign, leaves_per_step)
        _refuse_vanilla_resign(self.resign, evaluator)
        self.forced_playouts = check_forced_playouts(forced_playouts, evaluator, dirichlet, leaves_per_step)
        self.record_full = self.record_resigned = None
        self.replay = replay
        self.torch = torch
        # leaves_per_step > 1: OPT-IN virtual-loss expansion (K leaves in flight per game; changes search results); it is driven
        # by the simulation budget, like budget stepping
        self.leaves_per_step = max(1, int(leaves_per_step))
        # tree_reuse: OPT-IN tree reuse across moves (azk.h azk_config.tree_reuse; changes search results): 1 = carry, 2 = top-up.  Top-up
        # stops a game at n_sims root visits through the simulation budget, so it turns budget stepping on (eager runner: Engine.search_budget)
        self.tree_reuse = int(tree_reuse)
        self.budget_stepping = (budget_stepping or self.leaves_per_step > 1 or self.tree_reuse == 2 or self.playout_cap is not None
                                or self.adaptive) and use_graph
        self.per_launch = per_launch
        assert self.leaves_per_step == 1 or use_graph, "virtual-loss mode runs on the graph runner"
        self.launches = 0               # simulation-step launches issued (per game group) since construction
        self.use_graph = use_graph
        self._graph = None
        self.steps_per_graph = max(1, int(steps_per_graph))
        assert n_games % n_split == 0
        self.n_split = n_split if use_graph else 1
        per = n_games // self.n_split
        self.halves = [_Half(torch, Engine(game, per, n_sims, size=size, device=device, leaf_dtype=leaf_dtype,
                                           cache_entries=cache_entries, cache_shared=cache_shared, leaves_per_step=self.leaves_per_step,
                                           tree_reuse=self.tree_reuse, emit_symmetry=mask_elements(self.emit_elements) if self.emit_elements else None),
                             dirichlet)
                       for _ in range(self.n_split)]
        self.eng = self.halves[0].eng
        self.G = n_games
        self.evaluator, self.n_sims, self.seed, self.first = evaluator, n_sims, seed, first_global_game
        self.dirichlet, self.alpha, self.recycle, self.on_records = dirichlet, alpha, recycle, on_records
        self.sample_until = SAMPLE_UNTIL[game]
        self.kernel_timer = kernel_timer
        self.leaf_source_ok = True              # let a fused evaluator read the pending leaves straight from the engine (no azk_step_gather)
        self.streams = concurrent_streams(torch, self.eng.device, self.n_split) if self.n_split > 1 else []
        self.move_idx = 0
        self.plies_played = 0
        for i, h in enumerate(self.halves):
            h.eng.reset_games()
            if self.playout_cap is not None:
                h.eng.set_playout_cap(self.playout_cap[0], self.playout_cap[1], seed, first_global_game + i * per)
            if self.resign is not None:
                h.eng.set_resign(self.resign[0], self.resign[1], self.resign[2], seed, first_global_game + i * per)
            if self.forced_playouts is not None:
                h.eng.set_forced_playouts(self.forced_playouts)
            if self.eval_symmetry is not None:
                h.eng.set_eval_symmetry(*self.eval_symmetry)      # (the key is the position: the same for every group)
            if self.surprise_weight is not None:
                h.eng.set_surprise_weighting(self.surprise_weight, seed, first_global_game + i * per)
            if self.gumbel_root is not None:
                h.eng.set_gumbel_root(self.gumbel_root[0], n_sims, self.gumbel_root[1], self.gumbel_root[2])
            if self.puct is not None:
                h.eng.set_puct(*self.puct)
            if self.move_temperature is not None:
                h.eng.set_move_temperature(*self.move_temperature)
            if self.value_target is not None:
                h.eng.set_value_target(*self.value_target)
            if self.solver is not None:
                h.eng.set_solver(True)
            if self.root_noise is not None:
                h.eng.set_root_noise(*self.root_noise)
            if self.kld_stop is not None:
                h.eng.set_kld_stop(*self.kld_stop)
            if self.lead_stop is not None:
                h.eng.set_lead_stop(*self.lead_stop)
            if self.openings is not None:                         # the first games, under the key of their first search (move 0)
                h.eng.set_openings(self.openings[0], self.openings[1], self.openings[2], seed if openings_seed is None else openings_seed,
                                   (first_global_game if openings_first_game is None else openings_first_game) + i * per)
                h.eng.open_pending(0)

    # ---- one move for every slot -------------------------------------------------------------------------
    def play_move(self):
        torch = self.torch
        per = self.halves[0].eng.G
        for i, h in enumerate(self.halves):
            if self.gumbel_root is not None:                  # Gumbel rows where the Dirichlet rows go; the move needs no uniform
                noise, h.uni = h.eng.gen_gumbel(self.seed, self.first + i * per, self.move_idx), None
            elif self.root_noise is not None:                 # rows over the legal moves of the positions as they stand
                noise, h.uni = h.eng.gen_root_noise(self.seed, self.first + i * per, self.move_idx)
            else:
                noise, h.uni = h.eng.gen_noise(self.seed, self.first + i * per, self.move_idx, self.alpha, want_noise=self.dirichlet)
            if self.dirichlet:
                h.noise_buf.copy_(noise)
        if self.use_graph:
            self.search_graph()
        else:
            self.search(self.halves[0].noise_buf)
        for h in self.halves:
            e = h.eng
            if self.playout_cap is not None:
                h.h_full.copy_(e.search_full(), non_blocking=True)
            if self.adaptive:
                h.h_sims.copy_(e.search_sims(), non_blocking=True)
            pi, q, _ = e.root_stats()
            if self.forced_playouts is not None or self.gumbel_root is not None:
                pi = e.root_policy_target()                   # what advance records: pruned where the search was a forced one; a Gumbel root's target
            h.h_pi.copy_(pi, non_blocking=True)
            h.h_q.copy_(q, non_blocking=True)
            chosen, winner, done = e.advance(h.uni, self.sample_until, move_index=self.move_idx)
            if self.resign is not None:
                h.h_resigned.copy_(e.resigned(), non_blocking=True)
            if self.surprise_weight is not None:
                kl, coin = e.surprise()
                h.h_kl.copy_(kl, non_blocking=True)
                h.h_coin.copy_(coin, non_blocking=True)
            h.h_chosen.copy_(chosen, non_blocking=True)
            h.h_winner.copy_(winner, non_blocking=True)
            h.h_done.copy_(done, non_blocking=True)
            if self.replay is not None:
                e.emit_finished(self.replay)              # (state, pi, z) tuples with D4 augmentation, on device
            if self.recycle:
                e.recycle_finished(h.stats)
                if self.openings is not None:                     # the games that have just started, under the key of the next move's search
                    e.open_pending(self.move_idx + 1)
            h.h_stats.copy_(h.stats, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        for i, h in enumerate(self.halves):
            self.plies_played += int((h.h_chosen >= 0).sum())
            if self.on_records is not None:
                self.record_full, self.record_resigned = h.h_full, h.h_resigned
                self.record_surprise = (h.h_kl, h.h_coin) if self.surprise_weight is not None else None
                self.record_sims = h.h_sims if self.adaptive else None
                self.on_records(self.move_idx, i * per, h.h_pi, h.h_q, h.h_chosen, h.h_winner, h.h_done)
        self.move_idx += 1

    def search(self, noise):
        """Eager stepping (host sync per simulation, n_leaf-sized evaluator batches); optional k_tree event timing."""
        e, kt = self.eng, self.kernel_timer
        if self.tree_reuse == 2 or self.playout_cap is not None or self.adaptive:
            e.search_budget(self.evaluator, self.n_sims, noise if self.dirichlet else None, self.per_launch, move_index=self.move_idx)
            return
        e.begin_search(noise)
        logits = values = None
        for s in range(self.n_sims):
            if kt is not None and kt.want(s):
                kt.start()
                e.step_tree(logits, values)
                kt.stop()
                e.step_gather()
            else:
                e.step(logits, values)
            n = int(e.n_leaf.item())
            if n > 0:
                logits, values = e.evaluate_leaves(self.evaluator, n)
            elif e.cache_entries:
                logits, values = e.placeholder_rows()
            else:
                logits = values = None
        if logits is not None:
            e.step_expand_backup(logits, values)

    def _step_body(self, h, timer=None):
        """One simulation for every game of one group, with no host round trip: expand+backup of the previous leaves,
        PUCT select, leaf compaction, then the evaluator over the (fixed-size) leaf buffer.  Rows past n_leaf hold
        older boards; kernels that honour `live_count` skip them and nothing ever reads their outputs."""
        e = h.eng
        from_leaves = getattr(self.evaluator, "fused_embed_pool", False) and self.leaf_source_ok
        if timer is not None:
            timer.start()
            e.step_tree(h.logits_buf, h.values_buf)
            timer.stop()
            if not from_leaves:
                e.step_gather()
        elif from_leaves:
            e.step_tree(h.logits_buf, h.values_buf)          # the network kernel compacts the leaves itself
        else:
            e.step(h.logits_buf, h.values_buf)
        _evaluate_step(self.evaluator, e, h, from_leaves, timer)

    def _all_bodies(self):
        torch = self.torch
        if self.n_split == 1:
            self._step_body(self.halves[0])
            return
        cur = torch.cuda.current_stream()
        for st in self.streams:
            st.wait_stream(cur)
        for h, st in zip(self.halves, self.streams):
            with torch.cuda.stream(st):
                self._step_body(h)
        for st in self.streams:
            cur.wait_stream(st)

    def search_graph(self):
        """Replays of captured hipGraphs (per group: k_tree -> evaluator kernels).  Each group has its own graph, replayed on its
        own stream.  One-simulation stepping replays n_sims times; budget stepping (games run on inside a launch while their
        simulations need no evaluator) replays until no game owes simulations - about 45 % of n_sims at the benchmark config."""
        torch = self.torch
        for h in self.halves:
            if self.budget_stepping:
                h.eng.begin_search_budget(h.noise_buf, self.n_sims, self.per_launch, move_index=self.move_idx)
            else:
                h.eng.begin_search(h.noise_buf)
        cur = torch.cuda.current_stream()
        if self._graph is None:
            # the first simulations run eagerly on a side stream (allocator warm-up), the capture records one more
            side = torch.cuda.Stream()
            side.wait_stream(cur)
            with torch.cuda.stream(side):
                for _ in range(3):
                    for h in self.halves:
                        self._step_body(h)
            cur.wait_stream(side)
            torch.cuda.synchronize()
            self._graph, self._graph_many = [], []
            for h in self.halves:
                g = torch.cuda.CUDAGraph()
                with capture_without_finalisers(), torch.cuda.graph(g):
                    self._step_body(h)
                self._graph.append(g)
                if self.steps_per_graph > 1:
                    # the same step `steps_per_graph` times in one graph: consecutive graph launches leave the GPU idle for ~8 us
                    # (rocprofv3 kernel trace: gap before k_tree), consecutive kernels of one graph do not
                    gm = torch.cuda.CUDAGraph()
                    with capture_without_finalisers(), torch.cuda.graph(gm):
                        for _ in range(self.steps_per_graph):
                            self._step_body(h)
                    self._graph_many.append(gm)
            done = 3                     # the three eager steps ran; the captured ones were only recorded
        else:
            done = 0
        kt = self.kernel_timer
        streams = self.streams if self.n_split > 1 else [cur]
        for st in self.streams:
            st.wait_stream(cur)

        def replay(s, timed=None, many=False):
            timed = (kt is not None and kt.want(s)) if timed is None else timed
            for i, (h, g, st) in enumerate(zip(self.halves, self._graph, streams)):
                with torch.cuda.stream(st):
                    if timed:
                        # sampled steps run the same kernels eagerly so HIP events can bracket k_tree on its stream
                        self._step_body(h, timer=kt)
                    elif many:
                        self._graph_many[i].replay()
                    else:
                        g.replay()
        if not self.budget_stepping:
            # (the sampling phase carries over from move to move: with a stride that does not divide n_sims the sampled simulations
            #  drift through the search - leaf counts differ between its early and late simulations - instead of hitting the same few)
            s, U, next_sample = done, self.steps_per_graph, max(done, getattr(self, "_sample_phase", 0))
            while s < self.n_sims:
                if kt is not None and kt.enabled and s >= next_sample and len(kt.pairs) < kt.max:
                    replay(s, timed=True)
                    next_sample = s + kt.stride
                    s += 1
                elif U > 1 and s + U <= self.n_sims:
                    replay(s, timed=False, many=True)
                    s += U
                else:
                    replay(s, timed=False)
                    s += 1
            self.launches += self.n_sims
            if kt is not None:
                self._sample_phase = max(0, next_sample - self.n_sims)
        else:
            # no game can finish before its budget's worth of cache misses: a first stretch without looking, then a look (one
            # 4-byte read-back) every few launches
            longest = self.playout_cap[1] if self.playout_cap is not None and self.playout_cap[0] == 0.0 else self.n_sims   # (all searches fast)
            # adaptive search budgets (kld_stop, lead_stop): the same loop once per segment - when every game's segment is complete and its last leaf
            # expanded, the groups' checkpoints judge the games (outside the graphs), and the stepping goes on while one was released
            if self.adaptive:
                longest = min(longest, (self.kld_stop or self.lead_stop)[0])
            s, first, segments = done, max(done, int(0.36 * longest / self.leaves_per_step)), 1
            while True:
                while True:
                    stop = first if s < first else s + 8
                    while s < stop:
                        replay(s)
                        s += 1
                    for st in self.streams:
                        cur.wait_stream(st)
                    if all(h.eng.unfinished() == 0 for h in self.halves):
                        break
                    if s > 2 * self.n_sims + 16 * segments:
                        raise RuntimeError("budget stepping does not terminate")
                if not self.adaptive:
                    break
                self._expand_last_leaves(streams)
                if sum(h.eng.kld_checkpoint() for h in self.halves) == 0:
                    break
                if segments > self.n_sims:
                    raise RuntimeError("the checkpoints do not terminate")
                segments += 1
                first = s + int(0.36 * longest)
                for st in self.streams:
                    st.wait_stream(cur)
            self.launches += s
        if not self.adaptive:
            self._expand_last_leaves(streams)

    def _expand_last_leaves(self, streams):
        """The closing expand + backup of a search (or of one of its segments): the leaves the last launch selected."""
        torch = self.torch
        cur = torch.cuda.current_stream()
        if self.leaves_per_step == 1:            # (K > 1: the stepping loop only ends once nothing is pending)
            for h, st in zip(self.halves, streams):
                with torch.cuda.stream(st):
                    h.eng.step_expand_backup(h.logits_buf, h.values_buf)
        for st in self.streams:
            cur.wait_stream(st)

    def move_temperature_stats(self):
        """[plies drawn by weight, of those not the most-visited child, children cut, plies that fell back] over the groups (host sync)."""
        if self.move_temperature is None:
            raise ValueError("move_temperature_stats: the runner was built without move_temperature")
        return [sum(x) for x in zip(*[h.eng.move_temperature_stats() for h in self.halves])]

    def solver_stats(self):
        """The six counters of Engine.solver_stats summed over the groups (host sync)."""
        if self.solver is None:
            raise ValueError("solver_stats: the runner was built without solver=True")
        out = {}
        for h in self.halves:
            for k, v in h.eng.solver_stats().items():
                out[k] = out.get(k, 0) + v
        return out

    def kld_stats(self):
        """The four counters of Engine.kld_stats summed over the groups (host sync)."""
        if self.kld_stop is None:
            raise ValueError("kld_stats: the runner was built without kld_stop=...")
        out = {}
        for h in self.halves:
            for k, v in h.eng.kld_stats().items():
                out[k] = out.get(k, 0) + v
        return out

    def lead_stats(self):
        """The five counters of Engine.lead_stats summed over the groups (host sync)."""
        if self.lead_stop is None:
            raise ValueError("lead_stats: the runner was built without lead_stop=...")
        out = {}
        for h in self.halves:
            for k, v in h.eng.lead_stats().items():
                out[k] = out.get(k, 0) + v
        return out

    def resign_stats(self):
        """[games ended by resignation, never-resign games ended, of those marked, of those whose marked side did not lose], all groups."""
        if self.resign is None:
            raise ValueError("resign_stats: the runner was built without resign=...")
        return [sum(x) for x in zip(*(h.eng.resign_stats() for h in self.halves))]

    @property
    def games_finished(self):
        return sum(int(h.h_stats[0]) for h in self.halves)

    @property
    def finished_plies(self):
        return sum(int(h.h_stats[1]) for h in self.halves)

    def counters(self):
        tot = {}
        for h in self.halves:
            for k, v in h.eng.counters().items():
                tot[k] = tot.get(k, 0) + v
        return tot

    def reset_counters(self):
        for h in self.halves:
            h.eng.reset_counters()

    def check_error(self):
        for h in self.halves:
            h.eng.check_error()


class AsyncSelfPlayRunner:
    """Continuous self-play with ASYNCHRONOUS moves (games/gomoku.py:132-162: a game moves as soon as ITS search is done - in the
    batched engine: no game waits for the slowest search of the batch) and budget stepping (a game keeps simulating inside a tree
    launch while its simulations need no evaluator - terminal leaves, eval-cache hits -, at most `per_launch` simulations per
    launch).  Trees, moves and games are those of the lock-step runner, slot for slot and move for move: a game's simulations stay
    sequential, the random keys are (seed, global game, the slot's move counter) (tests/test_gpu_async.py).

    One step = k_tree (budget-stepped) -> k_move_async (moves every game whose search is complete, starts its next search) ->
    evaluator over the pending leaves; `steps_per_graph` steps are captured in one hipGraph.  After every graph replay the host
    enqueues the drain (finished games: (state, pi, z) emission into `replay`, statistics, restart) and an asynchronous copy of
    the statistics; it looks at them one replay late, so the GPU never waits for the host.

    play_move() keeps the lock-step runner's contract for its callers (bench.py): it returns once the batch has played G more
    moves in total (one move per resident game on average) - G x n_sims simulations, the same work as one lock-step move.

    reroot = 1 | 2 (OPT-IN tree reuse across moves, azk.h azk_config.tree_reuse: 1 carry, 2 top-up; arena_nodes as Engine's): the games
    of SelfPlayRunner(tree_reuse=reroot).  The move kernel parks a moved game and the drain re-roots it on the played child, so a game
    idles from its move to the next drain - about half of `steps_per_graph` steps.

    playout_cap = (p_full, n_fast) (OPT-IN, check_playout_cap; with any reroot): the games of SelfPlayRunner(playout_cap=...), slot for slot.
    `record_full` (uint8 numpy, one per record, valid inside on_records) tells each record's kind; searches_full / searches_fast count them.

    resign = (v_resign, p_never[, min_ply]) (OPT-IN, check_resign; with any reroot and with playout_cap): the games of SelfPlayRunner(resign=...),
    slot for slot - the move kernel applies the rule, the drain sees an ordinary finished game.  `record_resigned` (uint8 numpy, one per record,
    valid inside on_records) is 1 where the record's move conceded; resign_stats() counts the outcomes.

    forced_playouts = k (OPT-IN, check_forced_playouts; with any reroot, playout_cap and resign): the games of SelfPlayRunner(forced_playouts=k),
    slot for slot; the record ring's pi and the replay ring carry the pruned pi.

    eval_symmetry = True | ("fixed", s) (OPT-IN, check_eval_symmetry; with everything above): the games of SelfPlayRunner(eval_symmetry=...), slot
    for slot - the element is a function of the position, so it does not matter which step evaluates a leaf.

    emit_symmetry = "board" | "none" | elements (OPT-IN, check_emit_symmetry; with everything above): the drain emits every ply from the third
    on once per element of the mask, on every geometry - the tuples of SelfPlayRunner(emit_symmetry=...).

    surprise_weight = lambda (OPT-IN, check_surprise_weight; with everything above): the games and records of SelfPlayRunner(surprise_weight=...),
    slot for slot - the move kernel records kl and coin, the drain writes each recorded ply as often as its weight says.  `record_surprise`
    ((kl, coin), float64 numpy, one per record, valid inside on_records) carries them.

    gumbel_root = (m, c_visit, c_scale) (OPT-IN, check_gumbel_root; with resign, eval_symmetry, emit_symmetry and the eval cache; not with
    reroot): the games and records of SelfPlayRunner(gumbel_root=...), slot for slot - the movers make the Gumbel rows a search ahead where they
    make Dirichlet rows, play the survivor and record the Gumbel target.  n_sims is fixed for the run.

    openings = (p_open, max_plies, spread) (OPT-IN, check_openings; with everything above): the games of SelfPlayRunner(openings=...), slot for
    slot - the first games are opened inside async_begin, a restarted game inside the drain's restart kernel, under the slot's move counter.

    puct = (c, fpu) (OPT-IN, check_puct; with everything above except forced_playouts and gumbel_root): the games of SelfPlayRunner(puct=...),
    slot for slot - the rule reads only what the tree stores, so the movers and the re-root need nothing of it.

    move_temperature (OPT-IN, check_move_temperature; with everything above except gumbel_root and reroot = 1): the games of
    SelfPlayRunner(move_temperature=...), slot for slot - the movers draw from the same table with the same uniforms.

    value_target = r | (r, lam) (OPT-IN, check_value_target; with everything above except gumbel_root): the games of SelfPlayRunner, slot for
    slot, and the drain writes (1 - r) * z + r * G as the z of every tuple - the mover keeps each ply's q beside its pi, with re-rooting the
    carried root's W / N as it stands; the record ring's q column holds the same numbers.

    solver = True (OPT-IN, check_solver; with everything above except forced_playouts, gumbel_root, puct and reroot): the games of
    SelfPlayRunner(solver=True), slot for slot - the option lives in k_tree alone, the movers do not know it.

    root_noise = ("legal", alpha) | ("total", alpha_total) (OPT-IN, check_root_noise; with everything above except gumbel_root): the games of
    SelfPlayRunner(root_noise=...), slot for slot - a row cannot be made a search ahead (the position is not known then), so the row of a game
    that has just moved is made behind the movers, inside the step chain, and a parked or restarted game's in the drain; `alpha` is then not
    looked at.

    kld_stop = (interval, min_gain[, min_sims]) (OPT-IN, check_kld_stop; with everything above except gumbel_root): the games of
    SelfPlayRunner(kld_stop=...), slot for slot - the move kernel judges a game whose segment is complete and either releases it for the next
    segment or moves it, so a game whose root has settled moves without waiting for its allowance.  `record_sims` (int32 numpy, one per record,
    valid inside on_records) holds the new simulations each record's search ran; kld_stats() reads the four counters.  n_sims is fixed for
    the run (the segments are cut against the budget).

    lead_stop = (interval, factor[, min_sims]) (OPT-IN, check_lead_stop; alone or beside kld_stop): the games of SelfPlayRunner(lead_stop=...),
    slot for slot - the same movers judge the lead rule with integer arithmetic only.  `record_sims` is filled under either rule;
    lead_stats() reads the five counters."""

    def __init__(self, game, evaluator, n_games, n_sims, size=None, seed=0, first_global_game=0, dirichlet=True, alpha=0.03, device=0,
                 leaf_dtype="float32", recycle=True, on_records=None, kernel_timer=None, replay=None, cache_entries=0, cache_shared=False,
                 per_launch=2, steps_per_graph=32, record_capacity=None, use_graph=True, young_launch_us=0, tree_reuse=0, reroot=0, arena_nodes=0,
                 playout_cap=None, resign=None, forced_playouts=None, eval_symmetry=None, emit_symmetry=None, surprise_weight=None, gumbel_root=None,
                 openings=None, openings_seed=None, openings_first_game=None, puct=None, move_temperature=None, value_target=None, solver=None,
                 root_noise=None, kld_stop=None, lead_stop=None):
        import torch
        self.root_noise = check_root_noise(root_noise, dirichlet, evaluator, gumbel_root)
        self.openings = check_openings(openings, game, size, evaluator)
        self.gumbel_root = check_gumbel_root(gumbel_root, n_sims, evaluator, dirichlet, 1, tree_reuse or reroot, playout_cap, forced_playouts, surprise_weight)
        self.kld_stop = check_kld_stop(kld_stop, n_sims, evaluator, 1, self.gumbel_root)
        self.lead_stop = check_lead_stop(lead_stop, n_sims, evaluator, 1, self.gumbel_root, self.kld_stop)
        self.record_sims = None
        self.solver = check_solver(solver, evaluator, 1, forced_playouts, gumbel_root, puct, tree_reuse or reroot)
        self.value_target = check_value_target(value_target, evaluator, 1, self.gumbel_root)
        self.move_temperature = check_move_temperature(move_temperature, n_sims, game, size, self.gumbel_root, tree_reuse or reroot)
        self.puct = puct if check_puct(puct, evaluator, 1, forced_playouts, gumbel_root) is not None else None
        self.emit_elements = check_emit_symmetry(emit_symmetry, game, size)
        self.surprise_weight = check_surprise_weight(surprise_weight, evaluator)
        self.record_surprise = None
        self.eval_symmetry = check_eval_symmetry(eval_symmetry, game, size, evaluator, 1, seed)
        self.playout_cap = check_playout_cap(playout_cap, n_sims)
        self.resign = check_resign(resign)
        _refuse_vanilla_resign(self.resign, evaluator)
        self.forced_playouts = check_forced_playouts(forced_playouts, evaluator, dirichlet)
        self.record_full = self.record_resigned = None
        if tree_reuse:
            raise ValueError("AsyncSelfPlayRunner takes tree reuse as reroot=1 (carry) or reroot=2 (top-up): the re-root runs in the drain "
                             "(azk_async_begin_reuse), not where SelfPlayRunner(tree_reuse=...) has it")
        if reroot not in (0, 1, 2):
            raise ValueError(f"AsyncSelfPlayRunner: reroot must be 0 (off), 1 (carry) or 2 (top-up), not {reroot!r}")
        self.reroot = int(reroot)
        self.torch, self.replay, self.evaluator = torch, replay, evaluator
        self.eng = Engine(game, n_games, n_sims, size=size, device=device, leaf_dtype=leaf_dtype, cache_entries=cache_entries, cache_shared=cache_shared,
                          tree_reuse=self.reroot, arena_nodes=arena_nodes, emit_symmetry=mask_elements(self.emit_elements) if self.emit_elements else None)
        e = self.eng
        self.G, self._n_sims, self.n_split, self.leaves_per_step = n_games, n_sims, 1, 1
        self.per_launch, self.steps_per_graph, self.use_graph = int(per_launch), max(1, int(steps_per_graph)), use_graph
        self.kernel_timer, self.on_records = kernel_timer, on_records
        self.halves = [_Half(torch, e, False)]              # (logits / values step buffers; .eng for callers that walk the groups)
        self.h = self.halves[0]
        self.leaf_source_ok = True
        e.reset_games()
        if self.playout_cap is not None:
            e.set_playout_cap(self.playout_cap[0], self.playout_cap[1], seed, first_global_game)
        if self.resign is not None:
            e.set_resign(self.resign[0], self.resign[1], self.resign[2], seed, first_global_game)
        if self.forced_playouts is not None:
            e.set_forced_playouts(self.forced_playouts)
        if self.eval_symmetry is not None:
            e.set_eval_symmetry(*self.eval_symmetry)
        if self.surprise_weight is not None:
            e.set_surprise_weighting(self.surprise_weight, seed, first_global_game)
        if self.gumbel_root is not None:
            e.set_gumbel_root(self.gumbel_root[0], n_sims, self.gumbel_root[1], self.gumbel_root[2])
        if self.puct is not None:
            e.set_puct(*self.puct)
        if self.move_temperature is not None:
            e.set_move_temperature(*self.move_temperature)
        if self.value_target is not None:
            e.set_value_target(*self.value_target)
        if self.solver is not None:
            e.set_solver(True)
        if self.root_noise is not None:                           # the movers make the rows themselves, from each game's position
            e.set_root_noise(*self.root_noise)
        if self.kld_stop is not None:                             # async_begin arms the first searches, the movers and the drain every later one
            e.set_kld_stop(*self.kld_stop)
        if self.lead_stop is not None:
            e.set_lead_stop(*self.lead_stop)
        if self.openings is not None:                             # async_begin opens the first games, the drain's restart every later one
            e.set_openings(self.openings[0], self.openings[1], self.openings[2], seed if openings_seed is None else openings_seed,
                           first_global_game if openings_first_game is None else openings_first_game)
        cap = (4 * n_games if record_capacity is None else record_capacity) if (on_records is not None or record_capacity) else 0
        self.stats, self.records = e.async_begin(n_sims, self.per_launch, SAMPLE_UNTIL[game], seed, first_global_game, alpha, dirichlet, recycle, cap,
                                                 young_launch_us=young_launch_us, reroot=bool(self.reroot))
        self.rec_cap, self.rec_read, self.copy_stream = cap, 0, None
        self.h_stats = [torch.zeros(16, dtype=torch.int64, pin_memory=True) for _ in range(2)]
        self.events = [None, None]
        self.launches = 0               # simulation-step launches issued
        self.chunks = 0
        self.move_target = 0
        self._graph = None
        self._seen = torch.zeros(16, dtype=torch.int64)
        self.move_idx = 0

    @property
    def n_sims(self):
        return self._n_sims

    @n_sims.setter
    def n_sims(self, v):
        """Simulations per search from now on (bench.py's cheap pre-roll); read from device memory by the captured graphs."""
        if int(v) != self._n_sims:
            self._n_sims = int(v)
            self.eng.async_set_budget(self._n_sims, self.per_launch)

    # the lock-step runner's step body, with the asynchronous tree step in front
    def _step_body(self, timer=None):
        h, e = self.h, self.eng
        from_leaves = getattr(self.evaluator, "fused_embed_pool", False) and self.leaf_source_ok
        if timer is not None:
            timer.start()
            e.async_step(h.logits_buf, h.values_buf, 1)     # k_tree alone between the events
            timer.stop()
            e.async_step(h.logits_buf, h.values_buf, 2)
        else:
            e.async_step(h.logits_buf, h.values_buf, 3)
        if not from_leaves:
            e.step_gather()
        _evaluate_step(self.evaluator, e, h, from_leaves, timer)

    def _capture(self):
        torch = self.torch
        cur = torch.cuda.current_stream()
        side = torch.cuda.Stream()
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            for _ in range(3):                              # allocator warm-up; these steps count
                self._step_body()
        cur.wait_stream(side)
        torch.cuda.synchronize()
        self.launches += 3
        self._graph = torch.cuda.CUDAGraph()
        with capture_without_finalisers(), torch.cuda.graph(self._graph):
            for _ in range(self.steps_per_graph):
                self._step_body()

    def run_chunk(self):
        """`steps_per_graph` steps, the drain, and an asynchronous copy of the statistics (read one chunk late)."""
        torch = self.torch
        if not self.use_graph:
            for _ in range(self.steps_per_graph):
                self._step_body()
        else:
            if self._graph is None:
                self._capture()
            kt = self.kernel_timer
            if kt is not None and kt.enabled and len(kt.pairs) < kt.max and self.chunks % max(1, kt.stride // self.steps_per_graph) == 0:
                self._step_body(timer=kt)                   # a sampled step runs eagerly so HIP events can bracket its kernels
                self.launches += 1
            self._graph.replay()
        self.launches += self.steps_per_graph
        self.eng.async_drain(self.replay)
        i = self.chunks & 1
        self.h_stats[i].copy_(self.stats, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self.events[i] = ev
        self.chunks += 1

    def _look(self, i):
        """Statistics of the chunk before last (its copy has certainly landed once its event is done)."""
        if self.events[i] is not None:
            self.events[i].synchronize()
            self._seen = self.h_stats[i].clone()
            self._deliver_records()

    def _deliver_records(self):
        if self.on_records is None or self.records is None:
            return
        cursor = int(self._seen[6])
        if cursor - self.rec_read > self.rec_cap:
            raise RuntimeError("move-record ring overrun: raise record_capacity or drain more often")
        if cursor == self.rec_read:
            return
        # on a stream of their own: the entries are complete (their chunk's event is done) and the copies must not queue behind the
        # chunk that is running now
        if self.copy_stream is None:
            self.copy_stream = self.torch.cuda.Stream(device=self.eng.device)
        with self.torch.cuda.stream(self.copy_stream):
            idx = self.torch.arange(self.rec_read, cursor, device=self.eng.device) % self.rec_cap
            meta, q, pi = self.records["meta"][idx].cpu().numpy(), self.records["q"][idx].cpu().numpy(), self.records["pi"][idx].cpu().numpy()
            if "full" in self.records:
                self.record_full = self.records["full"][idx].cpu().numpy()
            if "resigned" in self.records:
                self.record_resigned = self.records["resigned"][idx].cpu().numpy()
            if "kl" in self.records:
                self.record_surprise = (self.records["kl"][idx].cpu().numpy(), self.records["coin"][idx].cpu().numpy())
            if "sims" in self.records:
                self.record_sims = self.records["sims"][idx].cpu().numpy()
        self.rec_read = cursor
        self.on_records(meta, q, pi)

    def run_until_moves(self, total_moves):
        """Run until the batch has played `total_moves` moves since construction (all slots together)."""
        while int(self._seen[5]) < total_moves:
            self.run_chunk()
            self._look((self.chunks & 1))                   # the OTHER buffer: the chunk before the one just enqueued
        return int(self._seen[5])

    def play_move(self):
        self.move_target += self.G
        self.run_until_moves(self.move_target)
        self.move_idx += 1

    def finish(self):
        """Wait for everything enqueued and read the final statistics."""
        self.torch.cuda.synchronize()
        self._seen = self.stats.cpu()
        self._deliver_records()
        return self._seen

    @property
    def plies_played(self):
        return int(self._seen[5])

    @property
    def games_finished(self):
        return int(self._seen[0])

    @property
    def finished_plies(self):
        return int(self._seen[1])

    def move_temperature_stats(self):
        """[plies drawn by weight, of those not the most-visited child, children cut, plies that fell back] over the groups (host sync)."""
        if self.move_temperature is None:
            raise ValueError("move_temperature_stats: the runner was built without move_temperature")
        return [sum(x) for x in zip(*[h.eng.move_temperature_stats() for h in self.halves])]

    def solver_stats(self):
        """The six counters of Engine.solver_stats summed over the groups (host sync)."""
        if self.solver is None:
            raise ValueError("solver_stats: the runner was built without solver=True")
        out = {}
        for h in self.halves:
            for k, v in h.eng.solver_stats().items():
                out[k] = out.get(k, 0) + v
        return out

    def kld_stats(self):
        """The four counters of Engine.kld_stats (host sync)."""
        if self.kld_stop is None:
            raise ValueError("kld_stats: the runner was built without kld_stop=...")
        return self.eng.kld_stats()

    def lead_stats(self):
        """The five counters of Engine.lead_stats (host sync)."""
        if self.lead_stop is None:
            raise ValueError("lead_stats: the runner was built without lead_stop=...")
        return self.eng.lead_stats()

    def resign_stats(self):
        """[games ended by resignation, never-resign games ended, of those marked, of those whose marked side did not lose] (host sync)."""
        if self.resign is None:
            raise ValueError("resign_stats: the runner was built without resign=...")
        return self.eng.resign_stats()

    @property
    def searches_full(self):
        """Full / fast searches among the searches begun (stats [8] / [9]; both 0 without playout_cap)."""
        return int(self._seen[8])

    @property
    def searches_fast(self):
        return int(self._seen[9])

    def counters(self):
        return self.eng.counters()

    def reset_counters(self):
        self.eng.reset_counters()

    def check_error(self):
        self.eng.check_error()


class KernelTimer:
    """HIP-event timing of one kernel on the stream it is launched on (torch's current stream)."""

    def __init__(self, stride=16, max_samples=4096):
        import torch
        self.torch, self.stride, self.max = torch, stride, max_samples
        self.pairs = []
        self.enabled = False
        self.children = {}                       # named sub-timers sharing this timer's sampling decisions

    def child(self, name):
        if name not in self.children:
            self.children[name] = KernelTimer(self.stride, self.max)
        return self.children[name]

    def want(self, step):
        return self.enabled and step % self.stride == 0 and len(self.pairs) < self.max

    def start(self):
        self._a = self.torch.cuda.Event(enable_timing=True)
        self._a.record()

    def stop(self):
        b = self.torch.cuda.Event(enable_timing=True)
        b.record()
        self.pairs.append((self._a, b))

    def mean_ms(self):
        self.torch.cuda.synchronize()
        if not self.pairs:
            return None
        return sum(a.elapsed_time(b) for a, b in self.pairs) / len(self.pairs)

    def robust_mean_ms(self):
        """Mean of the samples that are not host stalls: a pair brackets an EAGER launch, and a host hiccup between its two event records
        (garbage collection, another process tearing down) adds milliseconds to a ~10 us sample - a handful of those moves the mean of a
        few hundred samples by tens of percent.  Samples above three times the median are dropped; returns (mean_ms, dropped, total)."""
        self.torch.cuda.synchronize()
        if not self.pairs:
            return None, 0, 0
        t = sorted(a.elapsed_time(b) for a, b in self.pairs)
        med = t[len(t) // 2]
        kept = [x for x in t if x <= 3.0 * med]
        return sum(kept) / len(kept), len(t) - len(kept), len(t)

    def spread_us(self):
        """(median, max) of the samples in microseconds: a mean that sits far above the median is a few stalled samples, not the kernel."""
        self.torch.cuda.synchronize()
        t = sorted(a.elapsed_time(b) * 1e3 for a, b in self.pairs)
        return (t[len(t) // 2], t[-1]) if t else (None, None)
