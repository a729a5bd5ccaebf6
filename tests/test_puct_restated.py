"""CPU: the plain-Python restatement of configurable PUCT (tests/puct_restated.py) is the reference's search at c_table = [1.0], mode 0 - bit
for bit the oracle's trees - and the positions the GPU tests (tests/test_gpu_puct.py) use do exercise the option; the table helper, the
butterfly's order, and the refusals that happen before any engine exists."""
import math

import numpy as np
import pytest

import puct_restated as pr
from oracle import az_oracle as ao

IDENTITY = [("gomoku", 7), ("gomoku", (5, 3)), ("tictactoe", None), ("connect4", None)]


@pytest.mark.parametrize("n_sims", (24, 64, 200))
@pytest.mark.parametrize("kind,size", IDENTITY)
def test_plain_setting_is_the_oracles_search(kind, size, n_sims):
    """Guards the yardstick: with c_table = [1.0] and mode 0 the restatement's trees are oracle.mcts' - depth, cell, visit, value and prior of
    every node - from an empty board and from a position a few plies in, with a Dirichlet row (the float64 root path) and without one."""
    og = ao.OracleGame(kind, size)
    ev = pr.hash_evaluator(og)
    for seed, plies, noisy in ((11, 0, True), (12, 3, True), (13, 2, False)):
        cells, to_move, mc = pr.position(og, seed, plies)
        noise = np.random.RandomState(seed).dirichlet([0.3] * og.action_dim) if noisy else None
        tree = ao.OracleTree(og, cap=1 << 16)
        tree.reset(to_move, mc)
        ao.mcts(og, tree, og.board_from_cells(cells, to_move), n_sims, ev, noise)
        root = pr.RNode(None, None, to_move, mc)
        pr.mcts(og, root, og.board_from_cells(cells, to_move), n_sims, ev, noise, pr.setting_of("plain"))
        assert pr.same_tree(pr.export(root), tree.export()), (kind, size, n_sims, seed)


def test_plain_setting_is_the_oracles_search_on_the_wide_board():
    og = ao.OracleGame("gomoku", 15)
    ev = pr.hash_evaluator(og)
    cells, noise = pr.fr.wide_cells(24), np.random.RandomState(5).dirichlet([0.03] * 225)
    tree = ao.OracleTree(og, cap=1 << 16)
    tree.reset(0, 24)
    ao.mcts(og, tree, og.board_from_cells(cells, 0), 64, ev, noise)
    root = pr.RNode(None, None, 0, 24)
    pr.mcts(og, root, og.board_from_cells(cells, 0), 64, ev, noise, pr.setting_of("plain"))
    assert pr.same_tree(pr.export(root), tree.export())


@pytest.mark.parametrize("n_sims", pr.SIMS)
@pytest.mark.parametrize("name", sorted(pr.GAMES))
def test_preconditions_of_the_small_cases(name, n_sims):
    """Every (game, seed, position) of the GPU tests, under each of the three settings: the tree is not the plain tree, and under the two FPU
    settings at least one selection of the slot was settled by an unvisited child's qf + u0 against a visited child."""
    og, slots = pr.small_case(name, n_sims)
    for g, s in enumerate(slots):
        for key, (c, fpu) in pr.SETTINGS.items():
            assert not pr.same_tree(s[key]["tree"], s["plain"]["tree"]), (name, n_sims, key, g)
            decided = sum(1 for r in s[key]["log"] if r[4])
            assert (decided > 0) == (fpu is not None), (name, n_sims, key, g)
    assert any(s["move_count"] >= 3 for s in slots)                # positions several plies into a game


@pytest.mark.parametrize("noisy", (True, False))
@pytest.mark.parametrize("i", range(3))
def test_preconditions_of_the_wide_positions(i, noisy):
    """15 x 15 with 6 / 12 / 24 stones: 48 / 96 / 192 root children - one position per form of the scan, on either precision path at the
    root - and in the 192-child case a node below the root with more than 128 children selected among visited children."""
    og, s = pr.wide_case(i, noisy)
    log = s[pr.WIDE_SETTING]["log"]
    assert max(r[2] for r in log if r[1] == 0) == (48, 96, 192)[i]
    assert any(r[4] for r in log)
    assert not pr.same_tree(s[pr.WIDE_SETTING]["tree"], s["plain"]["tree"])
    assert any(r[1] == 0 and r[3] > 0 for r in log)                # the root itself summed a visited mass
    if i == 2:
        assert any(r[1] >= 1 and r[2] > 128 and r[3] > 0 for r in log)


@pytest.mark.parametrize("noisy", (True, False))
def test_preconditions_of_the_20x20_position(noisy):
    """273 root children, and below the root a node with more than 256 children selected among visited ones: the mass's own pass, on both
    precision paths.  The plain setting is the oracle's search here too."""
    og, s = pr.huge_case(noisy)
    log = s[pr.WIDE_SETTING]["log"]
    assert max(r[2] for r in log if r[1] == 0) == 273
    assert any(r[1] == 0 and r[3] > 0 for r in log) and any(r[1] >= 1 and r[2] > 256 and r[3] > 0 for r in log)
    assert any(r[4] for r in log) and not pr.same_tree(s[pr.WIDE_SETTING]["tree"], s["plain"]["tree"])
    tree = ao.OracleTree(og, cap=1 << 16)
    tree.reset(s["to_move"], s["move_count"])
    ao.mcts(og, tree, og.board_from_cells(s["cells"], s["to_move"]), pr.HUGE_SIMS, pr.hash_evaluator(og), s["noise"])
    assert pr.same_tree(s["plain"]["tree"], tree.export())


def test_puct_table_and_settings():
    from selfplay import puct_table
    t = puct_table(1.25, 19652, 300)
    assert t.dtype == np.float64 and len(t) == 300
    assert all(t[n] == math.log((1 + n + 19652) / 19652) + 1.25 for n in (0, 1, 17, 299))
    table, mode, f_tree, f_root = pr.setting_of("az_reduction")
    assert len(table) == 65536 and table[:300].tobytes() == t.tobytes() and (mode, f_tree, f_root) == (2, 0.3, 0.0)
    assert [list(pr.setting_of("plain")[0])] + list(pr.setting_of("plain")[1:]) == [[1.0], 0, 0.0, 0.0]
    table, mode, f_tree, f_root = pr.setting_of("c1.5_absolute")
    assert list(table) == [1.5] and (mode, f_tree, f_root) == (1, -1.0, -1.0)          # the root's parameter defaults to the tree's
    assert list(pr.puct_setting([1.0, 2.0, 3.0])[0]) == [1.0, 2.0, 3.0]


def test_the_butterfly_is_not_a_sequential_sum():
    """The order is part of the rule: on float32 parts of mixed magnitude the butterfly and a left-to-right sum give different bits."""
    rng = np.random.RandomState(0)
    parts = [np.float32(x) for x in rng.uniform(0, 1, 64) ** 8]
    seq = np.float32(0.0)
    for p in parts:
        seq = seq + p
    b = pr.butterfly(parts)
    assert b.dtype == np.float32 and abs(float(b) - float(seq)) < 1e-5 and b.tobytes() != seq.tobytes()


def test_refusals_before_any_engine_exists():
    from fixture_eval import FixtureModel
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_puct, self_play_batch
    import arena
    import train as az_train
    from games import Gomoku
    assert check_puct(None) is None
    assert check_puct((2.5, None))[1:] == (0, 0.0, 0.0)
    assert check_puct(((1.25, 19652), ("reduction", 0.3, 0.0)))[1:] == (2, 0.3, 0.0)
    for bad in (2.5, (2.5,), (-1.0, None), (float("nan"), None), (float("inf"), None), ([], None), ([1.0] * 65537, None), ([1.0, -2.0], None),
                (1.0, ("reduction", -0.1)), (1.0, ("reduction", 0.1, -0.1)), (1.0, ("absolute", float("nan"))), (1.0, ("absolute", 0.0, float("inf"))),
                (1.0, ("relative", 0.1)), (1.0, ("absolute",)), (1.0, "absolute"), (None, None)):
        with pytest.raises(ValueError, match="puct"):
            check_puct(bad)
    with pytest.raises(ValueError, match="vanilla"):
        check_puct((2.0, None), evaluator=None)
    with pytest.raises(ValueError, match="leaves_per_step"):
        check_puct((2.0, None), leaves_per_step=2)
    with pytest.raises(ValueError, match="forced_playouts"):
        check_puct((2.0, None), forced_playouts=2.0)
    with pytest.raises(ValueError, match="gumbel_root"):
        check_puct((2.0, None), gumbel_root=(4, 50.0, 1.0))
    ev = FixtureModel(49)
    # (no GPU is needed: each constructor validates first)
    with pytest.raises(ValueError, match="vanilla"):
        SelfPlayRunner("gomoku", None, 4, 8, size=7, puct=(2.0, None))
    with pytest.raises(ValueError, match="forced_playouts"):
        SelfPlayRunner("gomoku", ev, 4, 8, size=7, forced_playouts=2, puct=(2.0, None))
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 4, 8, size=7, leaves_per_step=2, use_graph=True, puct=(2.0, None))
    with pytest.raises(ValueError, match="gumbel_root"):
        AsyncSelfPlayRunner("gomoku", ev, 4, 8, size=7, gumbel_root=(4, 50.0, 1.0), puct=(2.0, None))
    with pytest.raises(ValueError, match="vanilla"):
        AsyncSelfPlayRunner("gomoku", None, 4, 8, size=7, puct=(2.0, None))
    with pytest.raises(ValueError, match="vanilla"):
        self_play_batch("gomoku", None, 4, 8, size=7, puct=(2.0, None))
    with pytest.raises(ValueError, match="reduction"):
        self_play_batch("gomoku", ev, 4, 8, size=7, puct=(2.0, ("reduction", -1.0)))
    with pytest.raises(ValueError, match="vanilla"):
        arena.compare("gomoku", ev, None, 8, 8, 4, False, False, size=7, puct=(2.0, None))
    with pytest.raises(ValueError, match="vanilla"):
        arena.compete_batch("gomoku", None, ev, 4, 8, 8, size=7, puct=(2.0, None))
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(Gomoku, ev, [], 1, 8, batched=False, puct=(2.0, None))
