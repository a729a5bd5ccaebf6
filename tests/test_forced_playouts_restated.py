"""CPU: the plain-Python restatement of forced playouts and policy target pruning (tests/forced_playouts_restated.py) is the reference's search
at k = 0 - bit for bit the oracle's trees - and the positions the GPU tests (tests/test_gpu_forced_playouts.py) use do exercise the option;
the refusals that happen before any engine exists."""
import numpy as np
import pytest

import forced_playouts_restated as fr
from oracle import az_oracle as ao

IDENTITY = [("gomoku", 7), ("gomoku", (5, 3)), ("gomoku", 15), ("tictactoe", None), ("connect4", None)]


@pytest.mark.parametrize("n_sims", (24, 64, 200))
@pytest.mark.parametrize("kind,size", IDENTITY)
def test_k0_is_the_oracles_search(kind, size, n_sims):
    """Guards the yardstick: at k = 0 the restatement's trees are oracle.mcts' - depth, cell, visit, value and prior of every node - from an
    empty board and from a position a few plies in, with a Dirichlet row."""
    og = ao.OracleGame(kind, size)
    ev = fr.hash_evaluator(og)
    for seed, plies in ((11, 0), (12, 3)):
        cells, to_move, mc = fr.position(og, seed, plies)
        noise = np.random.RandomState(seed).dirichlet([0.3] * og.action_dim)
        tree = ao.OracleTree(og, cap=1 << 16)
        tree.reset(to_move, mc)
        ao.mcts(og, tree, og.board_from_cells(cells, to_move), n_sims, ev, noise)
        root = fr.RNode(None, None, to_move, mc)
        fr.mcts(og, root, og.board_from_cells(cells, to_move), n_sims, ev, noise, 0.0)
        assert fr.same_tree(fr.export(root), tree.export()), (kind, size, n_sims, seed)
        ch = tree.root_children()
        assert fr.root_target(og, ch, tree.root_visit, 0.0).tobytes() == tree.pi().tobytes()


@pytest.mark.parametrize("n_sims", fr.SIMS)
@pytest.mark.parametrize("name", sorted(fr.GAMES))
def test_preconditions_of_the_small_cases(name, n_sims):
    """Every (game, seed, position) of the GPU tests: at k = 2 a forced selection happens, pruning changes the counts, and the tree is
    not the k = 0 tree."""
    og, slots = fr.small_case(name, n_sims)
    for g, s in enumerate(slots):
        f = s["forced"]
        assert len(f["log"]) > 0, (name, n_sims, g)
        assert f["pruned"] != [int(v) for v in f["children"]["visit"]], (name, n_sims, g)
        assert sum(f["pruned"]) >= 1 and all(0 <= m <= n for m, n in zip(f["pruned"], f["children"]["visit"]))
        assert not fr.same_tree(f["tree"], s["plain"]["tree"]), (name, n_sims, g)
        assert s["plain"]["log"] == []
    assert any(s["move_count"] >= 3 for s in slots)                # positions several plies into a game


@pytest.mark.parametrize("i", range(3))
def test_preconditions_of_the_wide_positions(i):
    """15 x 15 with 6 / 12 / 24 stones: 48 / 96 / 192 root children - one position per form of the root scan - and in the two wider ones a
    forced selection takes a child beyond the first 64 / 128 of the list."""
    og, s = fr.wide_case(i)
    board = og.board_from_cells(s["cells"], s["to_move"])
    assert len(og.valid_cells(board)) == (48, 96, 192)[i]
    f = s["forced"]
    assert len(f["children"]["cell"]) == (48, 96, 192)[i]
    assert len(f["log"]) > 0 and max(j for _, j in f["log"]) >= (0, 64, 128)[i]
    assert f["pruned"] != [int(v) for v in f["children"]["visit"]]
    assert not fr.same_tree(f["tree"], s["plain"]["tree"])


def test_prune_keeps_the_most_visited_child_and_unvisited_children():
    visits, values, priors = [0, 5, 9, 1, 9], [0.0, 1.0, 3.0, -1.0, 2.0], [0.1, 0.2, 0.3, 0.3, 0.1]
    m = fr.prune(visits, values, priors, 25, 2.0)
    assert m[0] == 0 and m[2] == 9                                 # N = 0 stays; c* = the FIRST child with the most visits
    assert m[3] == 0                                               # a lone forced visit is dropped altogether
    assert all(0 <= a <= b for a, b in zip(m, visits))
    assert fr.prune(visits, values, priors, 25, 0.0) == visits     # nf = 0: nothing can be removed


def test_refusals_before_any_engine_exists():
    from fixture_eval import FixtureModel
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_forced_playouts, self_play_batch
    import train as az_train
    from games import Gomoku
    assert check_forced_playouts(None) is None and check_forced_playouts(0) is None and check_forced_playouts(2) == 2.0
    for bad in (-1, float("nan"), float("inf"), "two"):
        with pytest.raises(ValueError, match="forced_playouts"):
            check_forced_playouts(bad)
    with pytest.raises(ValueError, match="vanilla"):
        check_forced_playouts(2, evaluator=None)
    with pytest.raises(ValueError, match="dirichlet"):
        check_forced_playouts(2, dirichlet=False)
    with pytest.raises(ValueError, match="leaves_per_step"):
        check_forced_playouts(2, leaves_per_step=2)
    ev = FixtureModel(49)
    # (no GPU is needed: each constructor validates first)
    with pytest.raises(ValueError, match="vanilla"):
        SelfPlayRunner("gomoku", None, 4, 8, size=7, forced_playouts=2)
    with pytest.raises(ValueError, match="dirichlet"):
        SelfPlayRunner("gomoku", ev, 4, 8, size=7, dirichlet=False, forced_playouts=2)
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 4, 8, size=7, leaves_per_step=2, use_graph=True, forced_playouts=2)
    with pytest.raises(ValueError, match="dirichlet"):
        AsyncSelfPlayRunner("gomoku", ev, 4, 8, size=7, dirichlet=False, forced_playouts=2)
    with pytest.raises(ValueError, match="vanilla"):
        AsyncSelfPlayRunner("gomoku", None, 4, 8, size=7, forced_playouts=2)
    with pytest.raises(ValueError, match="vanilla"):
        self_play_batch("gomoku", None, 4, 8, size=7, forced_playouts=2)
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(Gomoku, ev, [], 1, 8, batched=False, forced_playouts=2)
