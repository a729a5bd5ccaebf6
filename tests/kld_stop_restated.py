"""Adaptive search budgets - the KLD-gain stopper - restated in plain Python (TEST INFRASTRUCTURE, not product code).

The rule of include/azk.h (azk_set_kld_stop) on top of forced_playouts_restated.mcts at k = 0, which is pinned to oracle.mcts
(tests/test_forced_playouts_restated.py): the search is run on ONE root in segments, by calling mcts again on the same root, and judged between
them.  All arithmetic is Python float (IEEE float64); the lanes' partial sums and the xor butterfly are restated as the device has them, so the
only difference between this gain and the device's is the `log` of the two libraries.

Also here: the positions, thresholds and reference results the CPU and GPU tests share (computed once per process).
"""
import functools
import math

import numpy as np

import forced_playouts_restated as fr

WAVE = 64


def arm(T, interval):
    """Arming: the allowance T cut into its first segment -> (seg, left, run)."""
    seg = min(interval, T)
    return seg, T - seg, seg


def gain(old, new):
    """sum over i with o_i > 0 of po_i * log(po_i / pn_i): lane l sums its children l, l + 64, ... in list order, then the xor butterfly
    32 ... 1 combines the lanes.  Returns (gain, sum of |terms|)."""
    So, S = sum(old), sum(new)
    part, mag = [0.0] * WAVE, 0.0
    for i, (o, n) in enumerate(zip(old, new)):
        if o > 0:
            po, pn = float(o) / float(So), float(n) / float(S)
            t = po * math.log(po / pn)
            part[i % WAVE] += t
            mag += abs(t)
    off = 32
    while off > 0:
        part = [part[l] + part[l ^ off] for l in range(WAVE)]
        off >>= 1
    return part[0], mag


def rate(old, new):
    return gain(old, new)[0] / float(sum(new) - sum(old))


def search(og, root, board, T, evaluator, noise, interval, min_gain, min_sims=0):
    """The search of allowance T on `root` (a fresh RNode) under the rule.  Returns dict(run, ckpt, ended, left, rates, visits): the new
    simulations run, the checkpoint (1-based) at which the search ended, "early" | "allowance", the simulations left unrun, every judged
    rate in order, and the root children's visits at every checkpoint."""
    seg, left, run = arm(T, interval)
    fr.mcts(og, root, board, seg, evaluator, noise)
    snap, rates, visits, ckpt = None, [], [], 0
    while True:
        ckpt += 1
        n = [c.visit for c in root.children]
        visits.append(n)
        if left == 0:
            return dict(run=run, ckpt=ckpt, ended="allowance", left=0, rates=rates, visits=visits)
        if snap is not None and sum(snap) > 0 and run >= min_sims:
            r = rate(snap, n)
            rates.append(r)
            if r < min_gain:
                return dict(run=run, ckpt=ckpt, ended="early", left=left, rates=rates, visits=visits)
        snap = n
        seg = min(interval, left)
        left -= seg
        run += seg
        fr.mcts(og, root, board, seg, evaluator, noise)


# ---- the cases the CPU and GPU tests share ---------------------------------------------------------------------------------------------
G = fr.G
SMALL = ("tictactoe", "connect4", "gomoku7")
SMALL_T, SMALL_I = 64, 8
WIDE_T, WIDE_I = 96, 16
THRESHOLDS = (1e-3, 4e-3, 1e-2)
NEVER = 1e-300                             # a threshold only a rate of exactly 0 is below (see never_games): the smallest positive rates seen here are 1e-4


def searched(og, s, T, interval, min_gain, min_sims=0):
    """One slot (a dict of forced_playouts_restated's: cells, to_move, move_count, noise) searched under the rule: search()'s dict plus the
    tree, the root children and the raw pi."""
    root = fr.RNode(None, None, s["to_move"], s["move_count"])
    out = search(og, root, og.board_from_cells(s["cells"], s["to_move"]), T, fr.hash_evaluator(og), s["noise"], interval, min_gain, min_sims)
    out["tree"] = fr.export(root)
    out["cells"] = [c.cell for c in root.children]
    out["pi"] = fr.pi_of(og, out["cells"], [c.visit for c in root.children])
    return out


@functools.lru_cache(maxsize=None)
def small_results(name, min_gain):
    """forced_playouts_restated.small_case's G positions of one small game, each searched with T = 64, I = 8."""
    og, slots = fr.small_case(name, SMALL_T)
    return og, slots, [searched(og, s, SMALL_T, SMALL_I, min_gain) for s in slots]


@functools.lru_cache(maxsize=None)
def wide_results(i, min_gain):
    """forced_playouts_restated.wide_case(i) - 48 / 96 / 192 root children - searched with T = 96, I = 16."""
    og, s = fr.wide_case(i)
    return og, s, searched(og, s, WIDE_T, WIDE_I, min_gain)


# games for "a threshold that never fires": a rate of exactly 0 - a root with one child, or visits that grew in exact proportion - is below every
# positive threshold, so the games are played here first and tests/test_kld_stop_restated.py asserts that no search of theirs ends early
NEVER_GAME, NEVER_MOVES, NEVER_T, NEVER_I = "connect4", 6, 32, 8


def never_noise(move):
    """The G noise rows of move `move` (what the GPU test hands to self_play_batch as noise_fn)."""
    return np.random.RandomState(7000 + move).dirichlet([fr.NOISE_ALPHA] * 7, size=G)


@functools.lru_cache(maxsize=None)
def never_games():
    """G Connect4 games from the empty board, NEVER_MOVES greedy moves each (the first most-visited child), every search under the rule with
    min_gain = NEVER: per game the cells played and (ended, smallest judged rate) of every search."""
    og = fr.oracle_game(NEVER_GAME)
    ev = fr.hash_evaluator(og)
    games = []
    for g in range(G):
        board, player, cells, outcomes = og.new_board(), 0, [], []
        for mv in range(NEVER_MOVES):
            root = fr.RNode(None, None, player, mv)
            r = search(og, root, board, NEVER_T, ev, never_noise(mv)[g], NEVER_I, NEVER)
            outcomes.append((r["ended"], min(r["rates"])))
            c = max(root.children, key=lambda ch: ch.visit).cell                 # (max returns the first of equals: Node.max_visit_child)
            cells.append(c)
            og.make_move(board, player, og.rc(c))
            if og.check_winner(board, player, og.rc(c)) != -1:
                break
            player = 1 - player
        games.append(dict(cells=cells, outcomes=outcomes))
    return games


def stats_of(results):
    """azk_get_kld_stats over a list of search() results."""
    early = [r for r in results if r["ended"] == "early"]
    return dict(judged=sum(len(r["rates"]) for r in results), ended_early=len(early), sims_unrun=sum(r["left"] for r in early),
                ran_allowance=len(results) - len(early))
