"""Forced playouts and policy target pruning, restated in plain Python (TEST INFRASTRUCTURE, not product code).

The oracle's search is C and frozen, so the rule of include/azk.h (azk_set_forced_playouts) is restated here on a plain-Python
copy of the reference's search - MCTS.mcts (ai/mcts.py:11-60), Node.select / expand / backup (ai/node.py:42-74) and the 'network' UCB
(utils.py:29-44) - with numpy >= 2 scalar arithmetic: float32 priors below the root (float32 UCB), and at a root that got Dirichlet noise the
float64 priors  np.float32(0.75) * p + 0.25 * noise  (float64 UCB).  With k = 0 it is the reference's search and reproduces oracle.mcts
trees bit for bit (tests/test_forced_playouts_restated.py), which is what makes it a yardstick for k > 0.

Also here: the positions, noise rows and reference results the CPU and GPU tests share (computed once per process).
"""
import functools
import math

import numpy as np
import torch

from fixture_eval import fixture_logits_value
from oracle import az_oracle as ao

assert int(np.__version__.split(".")[0]) >= 2, "the restatement relies on numpy >= 2 scalar promotion (NEP 50)"

INF = float("inf")


class RNode:
    """ai/node.py:21-40, the fields the network search uses."""
    __slots__ = ("parent", "visit", "value", "prior", "move_count", "cell", "player", "children")

    def __init__(self, parent, cell, player, move_count, prior=0.0):
        self.parent, self.cell, self.player, self.move_count, self.prior = parent, cell, player, move_count, prior
        self.visit, self.value, self.children = 0, 0, []


def hash_evaluator(og):
    """evaluator(canonical board) -> (float32 priors [A] by the engine's deterministic softmax, value) on the fixture's "hash" logits."""
    A = og.action_dim

    def ev(canon):
        logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], A, "hash")
        return ao.softmax_det(logits[0].numpy()), float(v[0])
    return ev


def forced(n, p, n_parent, k):
    """The selection rule: a root child with n >= 1 visits and mixed prior p under a root of n_parent visits."""
    return n >= 1 and float(n) * float(n) < (k * p) * float(n_parent - 1)


def select(node, k, is_root):
    """Node.select (node.py:42-47) with utils.calcUcbOfChildrenFromParent(node, 'network') (utils.py:29-44); first maximum wins.
    Returns (child index, was the child a forced one)."""
    s = math.sqrt(node.visit)
    best, best_u, best_forced = -1, None, False
    for i, c in enumerate(node.children):
        if c.visit == 0:
            u = c.prior * s / (c.visit + 1)
        else:
            u = (c.value / c.visit) + c.prior * s / (c.visit + 1)
        f = is_root and k > 0.0 and forced(c.visit, c.prior, node.visit, k)
        if f:
            u = INF
        if best < 0 or u > best_u:
            best, best_u, best_forced = i, u, f
    return best, best_forced


def mcts(og, root, board, n_iter, evaluator, noise, k=0.0, log=None):
    """MCTS.mcts(model, board, root, Game, n_iter, dirichlet = noise is not None) without the eval cache (a deterministic evaluator makes it
    invisible).  k > 0: forced playouts at the root - which then needs its mixed priors, i.e. noise.  log (a list) receives
    (simulation, root child index) of every forced selection."""
    assert k == 0.0 or noise is not None
    for it in range(n_iter):
        node, trace = root, [root]
        while node.children:
            i, f = select(node, k, node is root)
            if f and log is not None:
                log.append((it, i))
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


def export(root):
    """The tree as azk_export_tree / OracleTree.export give it: DFS pre-order, children in list order."""
    rows, stack = [], [(root, 0)]
    while stack:
        nd, d = stack.pop()
        rows.append((d, -1 if nd.parent is None else nd.cell, nd.visit, float(nd.value), float(nd.prior)))
        for c in reversed(nd.children):
            stack.append((c, d + 1))
    a = list(zip(*rows))
    return dict(depth=np.array(a[0], np.int32), cell=np.array(a[1], np.int32), visit=np.array(a[2], np.int64),
                value=np.array(a[3], np.float64), prior=np.array(a[4], np.float64))


def same_tree(a, b):
    """Bit for bit: depth, cell, visit, value and prior of every node."""
    if len(a["depth"]) != len(b["depth"]):
        return False
    ok = all(np.array_equal(np.asarray(a[f]).astype(np.int64), np.asarray(b[f]).astype(np.int64)) for f in ("depth", "cell", "visit"))
    return ok and all(np.asarray(a[f], np.float64).tobytes() == np.asarray(b[f], np.float64).tobytes() for f in ("value", "prior"))


def prune(visits, values, priors, n_parent, k):
    """Policy target pruning over the root's children (list order): the integer counts the recorded pi is made of."""
    visits = [int(v) for v in visits]
    s = math.sqrt(float(n_parent))
    star = max(range(len(visits)), key=lambda i: visits[i])                                  # first child with the most visits
    pstar = float(values[star]) / float(visits[star]) + (float(priors[star]) * s) / float(visits[star] + 1)
    out = []
    for i, n in enumerate(visits):
        m = n
        if i != star and n >= 1:
            p = float(priors[i])
            nf = int(math.floor(math.sqrt((k * p) * float(n_parent - 1))))
            q = float(values[i]) / float(n)
            while m > n - nf and m > 0 and q + (p * s) / float(m) < pstar:
                m -= 1
            if m == 1 and nf >= 1:
                m = 0
        out.append(m)
    return out


def pi_of(og, cells, counts):
    """utils.get_probablity_distribution_of_children (utils.py:46-55) on the given counts."""
    v = np.zeros(og.action_dim)
    for c, m in zip(cells, counts):
        v[og.get_action_idx(og.rc(c))] = m
    return v / np.sum(v)


def root_target(og, ch, n_parent, k):
    """The recorded pi from azk_root_children-shaped data (cell / visit / value / prior arrays): pruned for k > 0, raw for k = 0."""
    counts = prune(ch["visit"], ch["value"], ch["prior"], n_parent, k) if k > 0.0 else [int(v) for v in ch["visit"]]
    return pi_of(og, ch["cell"], counts)


# ---- the positions the CPU and GPU tests share ------------------------------------------------------------------------------------------
K = 2.0
G = 8
GAMES = {"gomoku7": ("gomoku", 7), "gomoku5x3": ("gomoku", (5, 3)), "tictactoe": ("tictactoe", None), "connect4": ("connect4", None)}
SIMS = (24, 64)
PLIES = (1, 2, 2, 3, 3, 4, 4, 4)           # plies played before the search, per slot (<= 4: no game here can have ended; Gomoku's empty board has ONE legal move)
NOISE_ALPHA = 0.3


def oracle_game(name):
    kind, size = GAMES[name] if name in GAMES else ("gomoku", 15)
    return ao.OracleGame(kind, size)


def position(og, seed, plies):
    """cells int8 [rc] (0 empty, 1 player 0, 2 player 1), side to move, plies: `plies` legal moves drawn by RandomState(seed)."""
    rng = np.random.RandomState(seed)
    board = og.new_board()
    cells = np.zeros(og.rows * og.cols, np.int8)
    for ply in range(plies):
        valid = og.valid_cells(board)
        c = int(valid[rng.randint(len(valid))])
        og.make_move(board, ply & 1, og.rc(c))
        cells[c] = 1 + (ply & 1)
    return cells, plies & 1, plies


# slots whose first seed gives a search on which the option shows nothing (tests/test_forced_playouts_restated.py asserts that every slot's
# k = 2 search has a forced selection, a pruned count and another tree than k = 0): they take a later seed
SEED_BUMP = {("gomoku7", 0): 900, ("gomoku5x3", 4): 100}


def slot_seed(name, g):
    return 1000 * (1 + sorted(GAMES).index(name)) + g + SEED_BUMP.get((name, g), 0)


@functools.lru_cache(maxsize=None)
def small_case(name, n_sims):
    """G slots of one small game: positions, noise rows and the restated k = 2 / k = 0 searches."""
    og = oracle_game(name)
    ev = hash_evaluator(og)
    slots = []
    for g in range(G):
        cells, to_move, mc = position(og, slot_seed(name, g), PLIES[g])
        noise = np.random.RandomState(slot_seed(name, g) + 500).dirichlet([NOISE_ALPHA] * og.action_dim)
        slots.append(searched(og, ev, cells, to_move, mc, noise, n_sims))
    return og, slots


def searched(og, ev, cells, to_move, mc, noise, n_sims, k=K):
    out = dict(cells=cells, to_move=to_move, move_count=mc, noise=noise)
    for key, kk in (("forced", k), ("plain", 0.0)):
        root, log = RNode(None, None, to_move, mc), []
        mcts(og, root, og.board_from_cells(cells, to_move), n_sims, ev, noise, kk, log)
        ch = dict(cell=[c.cell for c in root.children], visit=[c.visit for c in root.children], value=[c.value for c in root.children],
                  prior=[c.prior for c in root.children])
        out[key] = dict(tree=export(root), log=log, children=ch, root_visit=root.visit)
    f = out["forced"]
    f["pruned"] = prune(f["children"]["visit"], f["children"]["value"], f["children"]["prior"], f["root_visit"], k)
    f["target"] = pi_of(og, f["children"]["cell"], f["pruned"])
    return out


WIDE_STONES = (6, 12, 24)                  # stones on the 15 x 15 board -> 48, 96, 192 root children: the three forms of the root scan
WIDE_SIMS = 96


def wide_cells(n_stones):
    """15 x 15: stones alternating 1, 2 on the cells (r, c), r and c in 1, 4, 7, 10, 13, row-major."""
    cells = np.zeros(225, np.int8)
    spots = [(r, c) for r in (1, 4, 7, 10, 13) for c in (1, 4, 7, 10, 13)]
    for i, (r, c) in enumerate(spots[:n_stones]):
        cells[r * 15 + c] = 1 + (i & 1)
    return cells


@functools.lru_cache(maxsize=None)
def wide_case(i):
    og = ao.OracleGame("gomoku", 15)
    n = WIDE_STONES[i]
    noise = np.random.RandomState(i + 1).dirichlet([0.03] * 225)
    return og, searched(og, hash_evaluator(og), wide_cells(n), n & 1, n, noise, WIDE_SIMS)
