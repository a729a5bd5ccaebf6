#!/usr/bin/env python3
"""Generate tests/golden/tree_reuse.npz by RUNNING THE REFERENCE's own Node / MCTS with the search of every move after the
first started on the subtree under the child that was played (tree reuse across moves, include/azk.h azk_config.tree_reuse).

TEST INFRASTRUCTURE.  Run on the development machine's CPU only (the reference never travels to the GPU box):
    python3 -B tests/golden/generate_tree_reuse.py
Only data goes into the .npz: inputs (noise rows, uniforms) and what the reference's code computed from them.

The reference never re-roots (games/gomoku.py:134 builds Node(None, None, ...) every move), but its MCTS.mcts (ai/mcts.py:11-60)
works on whatever root it is handed, so "reuse" is defined as the reference's search driven like this after the move was made:

    root = chosen_child; root.parent = None
    if dirichlet:                      # utils.add_dirichlet_noise's arithmetic on the children's stored float32 priors
        for c in root.children: c.prior = (1 - 0.25) * c.prior + 0.25 * noise[Game.get_action_idx(c.prevAction)]
    MCTS.mcts(model, board, root, Game, n_new, dirichlet)

with n_new = n_sims (mode 1, carry) or max(1, n_sims - root.visit) (mode 2, top-up).  A chosen child that was never expanded
gets a fresh root.  The arena rule (kept_nodes + n_new * widest <= nodes per game, widest = min(max children, empty cells of the
root position): what every position below the root is bounded by) is evaluated for every re-rooted search against the engine's
default arena of the mode and must never refuse: the golden games contain no arena fallback.

Exported trees / digests follow azk_export_tree: DFS pre-order, children in list order, depth from the CURRENT root, the root's
cell -1 and the root's prior 0.0 (a root's own prior is never read by the search; the engine does not keep it).
"""
import sys
sys.dont_write_bytecode = True
import os
import json
import hashlib
import struct
import logging

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))           # tests/ -> fixture_eval
from fixture_eval import FixtureModel                 # noqa: E402

# neutralise the reference's import-time file side effects (as generate_golden.py does)
_real_makedirs = os.makedirs


def _makedirs(path, *a, **k):
    if os.path.abspath(str(path)).startswith(REF):
        return None
    return _real_makedirs(path, *a, **k)


os.makedirs = _makedirs
logging.FileHandler = lambda *a, **k: logging.NullHandler()
sys.path.insert(0, REF)
import games as ref_games          # noqa: E402
import ai as ref_ai                # noqa: E402
import utils as ref_utils          # noqa: E402

Node, MCTS = ref_ai.Node, ref_ai.MCTS
TTT, C4, GMK = ref_games.TicTacToe, ref_games.Connect4, ref_games.Gomoku


def _canon3(board, player):
    if player == 0:
        return board
    out = np.empty_like(board)
    out[0], out[1], out[2] = board[1], board[0], board[2]
    return out


for _G in (TTT, C4):
    _G.feature_dim = 3
    _G.get_canonical_board = staticmethod(_canon3)


def set_gomoku(n):
    GMK.rows = GMK.cols = n
    GMK.action_dim = GMK.state_dim = n * n


def cell_idx(Game, mv):
    return mv[0] * Game.cols + mv[1]


def export_tree(root, Game):
    """azk_export_tree's rows for the tree under `root`."""
    rows = []
    stack = [(root, 0)]
    while stack:
        node, depth = stack.pop()
        is_root = node is root
        rows.append((depth, -1 if is_root else cell_idx(Game, node.prevAction), int(node.visit), float(node.value),
                     0.0 if is_root else float(node.prior)))
        for ch in reversed(node.children):
            stack.append((ch, depth + 1))
    return rows


def digest_rows(rows):
    h = hashlib.sha256()
    for d, c, n, w, p in rows:
        h.update(struct.pack("<iiqdd", d, c, n, w, p))
    return h.hexdigest()


def sdigest_rows(rows):
    """The same without the priors: the engine's softmax differs from numpy's in the last bits of a prior (tests/test_gpu_engine.py
    compares trees with the oracle's deterministic softmax for that reason), visits and values do not depend on those bits here."""
    h = hashlib.sha256()
    for d, c, n, w, p in rows:
        h.update(struct.pack("<iiqd", d, c, n, w))
    return h.hexdigest()


def rows_arrays(rows):
    return dict(depth=np.array([r[0] for r in rows], np.int32), cell=np.array([r[1] for r in rows], np.int32),
                visit=np.array([r[2] for r in rows], np.int64), value=np.array([r[3] for r in rows], np.float64),
                prior=np.array([r[4] for r in rows], np.float64))


def max_depth(rows):
    return max(r[0] for r in rows)


# (game, size, n_sims, mode, dirichlet, variant, seed, sample_until, max_plies, moves whose trees are stored in full[, start_plies])
# start_plies: the game starts from a position of that many stones dropped on uniformly random empty cells, colours alternating
# (stored as cells; what azk_set_positions loads) - scattered stones give Gomoku roots with more than 128 legal moves, which self-play
# from the empty board with a fixture evaluator never reaches (the reference's legal moves are the cells next to a stone)
CASES = [
    ("gomoku", 7, 64, 1, True, "hash", 11, 8, 0, (1, 2)),
    ("gomoku", 7, 64, 2, True, "hash", 12, 8, 0, (1,)),
    ("gomoku", 7, 48, 1, False, "uniform", 13, 8, 0, ()),
    ("gomoku", 7, 48, 2, False, "hash", 14, 8, 0, ()),
    ("gomoku", 15, 200, 1, True, "hash", 15, 8, 0, ()),
    ("gomoku", 15, 200, 2, True, "hash", 16, 8, 0, ()),
    ("gomoku", 15, 150, 1, False, "uniform", 17, 4, 8, ()),
    ("gomoku", 15, 160, 1, True, "hash", 24, 50, 6, (), 42),
    ("gomoku", 15, 160, 2, True, "hash", 25, 50, 6, (), 30),
    # carry on a narrow game: every node has about max_children children, so the arena rule drops the subtree as soon as it holds more
    # than about n_sims expansions - a few moves into a game whose visits concentrate.  The case stops before that (the fallback
    # is the GPU test's own case); the condition "no golden search is refused" is asserted in play()
    ("connect4", 0, 100, 1, True, "hash", 26, 8, 6, (3,)),
    ("connect4", 0, 100, 2, True, "hash", 19, 8, 0, ()),
    ("connect4", 0, 60, 2, False, "uniform", 20, 8, 0, ()),
    ("tictactoe", 3, 50, 1, True, "hash", 21, 8, 0, (1,)),
    ("tictactoe", 3, 50, 2, True, "hash", 22, 8, 0, ()),
    ("tictactoe", 3, 30, 1, False, "uniform", 23, 2, 0, ()),
]


def play(case_index, gname, size, n_sims, mode, dirichlet, variant, seed, sample_until, max_plies, full_moves, start_plies=0):
    Game = {"gomoku": GMK, "tictactoe": TTT, "connect4": C4}[gname]
    if gname == "gomoku":
        set_gomoku(size)
    A = Game.action_dim
    maxch = Game.cols if gname == "connect4" else Game.rows * Game.cols
    arena = 1 + (2 if mode == 1 else 1) * n_sims * maxch          # azk_create's default for the mode
    rng = np.random.RandomState(seed)
    # Dirichlet rows and move uniforms come from a legacy RandomState of their own (its stream is frozen by numpy's compatibility
    # policy): the fixture stores the uniforms and a sha256 of the rows, and the tests draw the rows again the same way - 225 random
    # float64 per move do not compress
    nrng = np.random.RandomState(seed + 1000)
    model = FixtureModel(A, variant)
    MCTS.cache.clear()
    while True:                                                       # (retry when the random opening already ends the game)
        game = Game()
        board, player, mc = game.board, 0, 0
        ok = True
        for _ in range(start_plies):
            empty = [(r, c) for r in range(Game.rows) for c in range(Game.cols) if board[0, r, c] == 0 and board[1, r, c] == 0]
            mv = empty[rng.randint(len(empty))]
            mover = player
            player = Game.make_move(board, player, mv)
            mc += 1
            if Game.check_winner(board, mover, mv) != -1:
                ok = False
                break
        if ok:
            break
    start_cells = (board[0] + 2 * board[1]).astype(np.int8).reshape(-1)
    first_mc = mc
    rec = dict(pi=[], q=[], chosen=[], root_visit=[], start_visit=[], n_new=[], reused=[], kept=[], noise=[], u=[],
               start_digest=[], end_digest=[], start_sdigest=[], end_sdigest=[], start_depth=[], start_width=[])
    full = {}
    chosen_child = None
    winner = -2
    orig_dirichlet = np.random.dirichlet
    while True:
        noise = nrng.dirichlet([0.03] * A)
        u = nrng.random_sample()
        reused = chosen_child is not None and len(chosen_child.children) > 0
        if reused:
            root = chosen_child
            root.parent = None
            if dirichlet:
                for c in root.children:
                    c.prior = (1 - 0.25) * c.prior + 0.25 * noise[Game.get_action_idx(c.prevAction)]
                    assert isinstance(c.prior, np.float64)
            n_new = n_sims if mode == 1 else max(1, n_sims - root.visit)
            start_rows = export_tree(root, Game)
            # the arena rule must hold for every re-rooted search of the golden games
            widest = min(maxch, Game.state_dim - mc)
            assert len(root.children) <= widest
            assert len(start_rows) + n_new * widest <= arena, (gname, size, mc, len(start_rows), n_new, widest, arena)
        else:
            root = Node(None, None, player, mc)
            n_new = n_sims
            start_rows = export_tree(root, Game)
        np.random.dirichlet = lambda alpha, size=None: noise          # the move's recorded row, wherever the root is expanded
        before = board.copy()
        with torch.no_grad():
            MCTS.mcts(model, board, root, Game, n_new, dirichlet)
        np.random.dirichlet = orig_dirichlet
        assert np.array_equal(before, board)
        end_rows = export_tree(root, Game)
        assert len(end_rows) <= arena
        pi = ref_utils.get_probablity_distribution_of_children(root, Game).astype(np.float64)
        if mc < sample_until:                                         # Node.sample_child: legacy np.random.choice(p=pi) on the uniform u
            cdf = np.cumsum(pi)
            cdf /= cdf[-1]
            act = int(np.searchsorted(cdf, u, side="right"))
            chosen_child = [c for c in root.children if Game.get_action_idx(c.prevAction) == act][0]
        else:
            chosen_child = root.max_visit_child()
        rec["pi"].append(pi); rec["q"].append(root.value / root.visit); rec["chosen"].append(cell_idx(Game, chosen_child.prevAction))
        rec["root_visit"].append(root.visit); rec["start_visit"].append(start_rows[0][2]); rec["n_new"].append(n_new)
        rec["reused"].append(int(reused)); rec["kept"].append(len(start_rows)); rec["noise"].append(noise); rec["u"].append(u)
        rec["start_digest"].append(digest_rows(start_rows)); rec["end_digest"].append(digest_rows(end_rows))
        rec["start_sdigest"].append(sdigest_rows(start_rows)); rec["end_sdigest"].append(sdigest_rows(end_rows))
        rec["start_depth"].append(max_depth(start_rows)); rec["start_width"].append(len(root.children) if reused else 0)
        if mc in full_moves or mc + 1 in full_moves:            # (move numbers of games that start from the empty board)
            if mc in full_moves:
                full[f"m{mc}_start"] = rows_arrays(start_rows)
            full[f"m{mc}_end"] = rows_arrays(end_rows)
        mover = player
        player = Game.make_move(board, player, chosen_child.prevAction)
        mc += 1
        w = Game.check_winner(board, mover, chosen_child.prevAction)
        if w != -1:
            winner = w
            break
        if mc == Game.state_dim:
            winner = -1
            break
        if max_plies and mc - first_mc >= max_plies:
            break                                                     # truncated (winner stays -2): the long 15x15 games
    out = {}
    k = f"g{case_index}_"
    out[k + "start_cells"] = start_cells
    out[k + "pi"] = np.stack(rec["pi"])
    for name, dt in (("q", np.float64), ("u", np.float64), ("chosen", np.int32), ("root_visit", np.int32), ("start_visit", np.int32),
                     ("n_new", np.int32), ("reused", np.int8), ("kept", np.int32), ("start_depth", np.int32), ("start_width", np.int32)):
        out[k + name] = np.array(rec[name], dt)
    out[k + "start_digest"] = np.array(rec["start_digest"])
    out[k + "end_digest"] = np.array(rec["end_digest"])
    out[k + "start_sdigest"] = np.array(rec["start_sdigest"])
    out[k + "end_sdigest"] = np.array(rec["end_sdigest"])
    for name, arrs in full.items():
        for col, a in arrs.items():
            out[k + name + "_" + col] = a
    meta = dict(case=case_index, game=gname, size=size, n_sims=n_sims, mode=mode, dirichlet=bool(dirichlet), variant=variant,
                seed=seed, sample_until=sample_until, max_plies=max_plies, start_plies=start_plies, plies=mc - first_mc, noise_sha256=hashlib.sha256(np.stack(rec["noise"]).tobytes()).hexdigest(), winner=int(winner), arena=arena,
                full=sorted(full.keys()), reused=int(sum(rec["reused"])), max_start_depth=int(max(rec["start_depth"])),
                max_start_width=int(max(rec["start_width"])),
                mean_share=float(np.mean([s / e for s, e, r in zip(rec["start_visit"][1:], rec["root_visit"][:-1], rec["reused"][1:]) if r] or [0.0])))
    print(meta)
    return out, meta


def main():
    out, metas = {}, []
    for i, c in enumerate(CASES):
        o, m = play(i, *c)
        out.update(o)
        metas.append(m)
    assert any(m["max_start_width"] > 128 for m in metas) and any(m["max_start_depth"] > 8 for m in metas)
    out["meta_json"] = np.frombuffer(json.dumps(metas).encode(), np.uint8)
    path = os.path.join(HERE, "tree_reuse.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
