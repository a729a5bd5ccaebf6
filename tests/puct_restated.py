"""Configurable PUCT - exploration-rate table and first-play urgency - restated in plain Python (TEST INFRASTRUCTURE, not product code).

The oracle's search is C and frozen, so the rule of include/azk.h (azk_set_puct) is restated here on the plain-Python copy
of the reference's search that tests/forced_playouts_restated.py keeps (its RNode, evaluator, export and positions are used as they are), with
numpy >= 2 scalar arithmetic: float32 priors below the root and at a root without noise (float32 scores), float64 mixed priors at a root that
got a noise row (float64 scores).  With c_table = [1.0] and mode 0 it is the reference's search and reproduces oracle.mcts trees bit for bit
(tests/test_puct_restated.py), which is what makes it a yardstick for every other setting.

Also here: the positions, noise rows and reference results the CPU and GPU tests share (computed once per process).
"""
import functools
import math

import numpy as np

import forced_playouts_restated as fr
from azk import puct_setting
from forced_playouts_restated import RNode, export, hash_evaluator, oracle_game, position, same_tree  # noqa: F401  (the tests' one import)

assert int(np.__version__.split(".")[0]) >= 2, "the restatement relies on numpy >= 2 scalar promotion (NEP 50)"

PLAIN = (1.0, None)                                               # the reference's formula, as a setting


def butterfly(parts):
    """The wave's sum of 64 partial sums by the xor butterfly 32, 16, 8, 4, 2, 1 (x = x + partner); every lane ends with the same bits."""
    x = list(parts)
    for off in (32, 16, 8, 4, 2, 1):
        x = [x[lane] + x[lane ^ off] for lane in range(64)]
    return x[0]


def visited_mass(node, f64):
    """vm: lane l adds the priors of its visited children l, l + 64, .. in list order, starting from 0; then the butterfly.  float64 on
    the float64 root path, float32 elsewhere."""
    parts = [np.float64(0.0) if f64 else np.float32(0.0)] * 64
    for i, c in enumerate(node.children):
        if c.visit > 0:
            parts[i & 63] = parts[i & 63] + (np.float64(c.prior) if f64 else np.float32(c.prior))
    return butterfly(parts)


def scores(node, setting, is_root, f64):
    """The score of every child of `node` under setting = (c_table, fpu_mode, fpu_tree, fpu_root), in list order."""
    table, mode, f_tree, f_root = setting
    c = float(table[min(node.visit, len(table) - 1)])
    f = f_root if is_root else f_tree
    qf = 0.0
    if mode == 1:
        qf = f
    elif mode == 2:
        qn = -(node.value / float(node.visit))
        qf = qn - f * math.sqrt(float(visited_mass(node, f64)))
    root = math.sqrt(float(node.visit))
    out = []
    if f64:
        s = c * root
        for ch in node.children:
            u0 = np.float64(ch.prior) * s / float(ch.visit + 1)
            out.append(ch.value / float(ch.visit) + u0 if ch.visit > 0 else (u0 if mode == 0 else qf + u0))
    else:
        s = np.float32(c * root)
        for ch in node.children:
            u0 = (np.float32(ch.prior) * s) / np.float32(ch.visit + 1)
            assert u0.dtype == np.float32
            out.append(np.float32(ch.value / float(ch.visit)) + u0 if ch.visit > 0 else (u0 if mode == 0 else np.float32(qf) + u0))
    return out


def first_max(us):
    best = 0
    for i, u in enumerate(us):
        if u > us[best]:
            best = i
    return best


def mcts(og, root, board, n_iter, evaluator, noise, setting, log=None):
    """fr.mcts with the selection rule of azk_set_puct.  log (a list) receives one record per selection:
    (simulation, depth, children, visited children, decided) - decided: the winner and the child the same scores with fpu_mode 0 would
    have taken are one visited and one unvisited child, i.e. an unvisited child's qf + u0 against a visited child's score settled it."""
    table, mode, f_tree, f_root = setting
    for it in range(n_iter):
        node, trace = root, [root]
        while node.children:
            is_root = node is root
            f64 = is_root and noise is not None
            i = first_max(scores(node, setting, is_root, f64))
            if log is not None:
                decided = False
                if mode != 0:
                    j = first_max(scores(node, (table, 0, 0.0, 0.0), is_root, f64))
                    decided = (node.children[i].visit > 0) != (node.children[j].visit > 0)
                log.append((it, len(trace) - 1, len(node.children), sum(1 for c in node.children if c.visit > 0), decided))
            node = node.children[i]
            trace.append(node)
            og.make_move(board, 1 - node.player, og.rc(node.cell))
        done = None
        if node.parent is not None:
            if og.check_winner(board, 1 - node.player, og.rc(node.cell)) != -1:
                done = 1
            elif node.move_count == og.state_dim:
                done = 0
        if done is None:
            cells = og.valid_cells(board)
            pri, value = evaluator(og.get_canonical_board(board, node.player))
            pri = np.asarray(pri, np.float32)
            if node.parent is None and noise is not None:
                pri = np.float32(0.75) * pri + 0.25 * np.asarray(noise, np.float64)      # utils.py:24-25: float32 product, float64 sum
            for c in cells:                                                                  # Node.expand (node.py:50-59)
                node.children.append(RNode(node, int(c), 1 - node.player, node.move_count + 1, pri[og.get_action_idx(og.rc(c))]))
            result = -value
        else:
            result = done
        for nd in trace[::-1]:                                                               # Node.backup (node.py:62-74)
            nd.visit += 1
            nd.value += result
            result *= -1
            if nd.parent is not None:
                og.undo_move(board, nd.player, og.rc(nd.cell))


def carry(og, root, cell, noise):
    """Tree reuse (carry) after the move `cell`: the played child becomes the root of the next search - prior 0, no parent - and with a
    noise row its children get the mixed float64 priors of a root (tests/tree_reuse_common.reroot).  None where the root has no such child
    or the child was never expanded: the next search starts from a fresh root."""
    for ch in root.children:
        if ch.cell == cell:
            if not ch.children:
                return None
            ch.parent, ch.prior = None, 0.0
            if noise is not None:
                for gc in ch.children:
                    gc.prior = np.float64(np.float32(0.75) * np.float32(gc.prior)) + 0.25 * np.float64(noise[og.get_action_idx(og.rc(gc.cell))])
            return ch
    return None


# ---- the positions the CPU and GPU tests share ------------------------------------------------------------------------------------------
G = fr.G
GAMES, SIMS, PLIES, NOISE_ALPHA = fr.GAMES, fr.SIMS, fr.PLIES, fr.NOISE_ALPHA
SETTINGS = {"c2.5": (2.5, None),
            "az_reduction": ((1.25, 19652), ("reduction", 0.3, 0.0)),
            "c1.5_absolute": (1.5, ("absolute", -1.0))}
WIDE_SETTING = "az_reduction"
WIDE_STONES, WIDE_SIMS = fr.WIDE_STONES, fr.WIDE_SIMS


@functools.lru_cache(maxsize=None)
def setting_of(name):
    """The normalised (c_table, fpu_mode, fpu_tree, fpu_root) of a named setting: exactly what Engine.set_puct hands to azk_set_puct."""
    return puct_setting(*(PLAIN if name == "plain" else SETTINGS[name]))


# slots whose first seed gives a search on which a setting shows nothing (tests/test_puct_restated.py asserts the preconditions): they take a later seed
SEED_BUMP = {("gomoku5x3", 5): 100, ("gomoku7", 1): 100}


def slot_seed(name, g):
    return 5000 + 1000 * sorted(GAMES).index(name) + g + SEED_BUMP.get((name, g), 0)


def searched(og, ev, cells, to_move, mc, noise, n_sims, names):
    out = dict(cells=cells, to_move=to_move, move_count=mc, noise=noise)
    for key in ("plain",) + tuple(names):
        root, log = RNode(None, None, to_move, mc), []
        mcts(og, root, og.board_from_cells(cells, to_move), n_sims, ev, noise, setting_of(key), log)
        out[key] = dict(tree=export(root), log=log)
    return out


@functools.lru_cache(maxsize=None)
def small_case(name, n_sims):
    """G slots of one small game: positions, noise rows and the restated searches under every setting and under the plain rule."""
    og = oracle_game(name)
    ev = hash_evaluator(og)
    slots = []
    for g in range(G):
        cells, to_move, mc = position(og, slot_seed(name, g), PLIES[g])
        noise = np.random.RandomState(slot_seed(name, g) + 500).dirichlet([NOISE_ALPHA] * og.action_dim)
        slots.append(searched(og, ev, cells, to_move, mc, noise, n_sims, tuple(SETTINGS)))
    return og, slots


HUGE_SIZE, HUGE_STONES, HUGE_SIMS = 20, 36, 48     # 20 x 20 (the engine's kernels for boards beyond 256 cells): 36 stones -> 273 root children


def huge_cells():
    """20 x 20: stones alternating 1, 2 on the cells (r, c), r and c in 1, 4, .., 19, row-major - each brings its free neighbours (eight, fewer at the right edge)."""
    cells = np.zeros(HUGE_SIZE * HUGE_SIZE, np.int8)
    spots = [(r, c) for r in range(1, HUGE_SIZE, 3) for c in range(1, HUGE_SIZE, 3)]
    for i, (r, c) in enumerate(spots[:HUGE_STONES]):
        cells[r * HUGE_SIZE + c] = 1 + (i & 1)
    return cells


@functools.lru_cache(maxsize=None)
def huge_case(noisy):
    """More children than one pass of the general loop holds (256): mode 2 sums the visited mass in a pass of its own."""
    from oracle import az_oracle as ao
    og = ao.OracleGame("gomoku", HUGE_SIZE)
    noise = np.random.RandomState(7).dirichlet([0.03] * HUGE_SIZE * HUGE_SIZE) if noisy else None
    return og, searched(og, hash_evaluator(og), huge_cells(), HUGE_STONES & 1, HUGE_STONES, noise, HUGE_SIMS, (WIDE_SETTING,))


WIDE_NOISE_SEED = (1, 2, 3)


@functools.lru_cache(maxsize=None)
def wide_case(i, noisy):
    """15 x 15 with 6 / 12 / 24 stones (48 / 96 / 192 root children: the three forms of the scan) under the second setting, with a noise
    row (the float64 root path) or without one (the float32 path at the root too)."""
    og = oracle_game("gomoku15")
    n = WIDE_STONES[i]
    noise = np.random.RandomState(WIDE_NOISE_SEED[i]).dirichlet([0.03] * 225) if noisy else None
    return og, searched(og, hash_evaluator(og), fr.wide_cells(n), n & 1, n, noise, WIDE_SIMS, (WIDE_SETTING,))
