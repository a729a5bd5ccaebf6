"""CPU: the plain-Python restatement of exact game-end proofs in the search (tests/solver_restated.py; include/azk.h azk_set_solver, DESIGN
section 29) is the reference's search with the option off - bit for bit fr.mcts at k = 0 and hence the oracle's trees -, keeps the header's
invariants after every simulation and proves only what an exhaustive minimax confirms; the refusals that happen before any engine exists;
and the preconditions of the GPU tests (tests/test_gpu_solver.py), so that none of them can pass by showing nothing."""
import numpy as np
import pytest

import forced_playouts_restated as fr
import solver_restated as sr
from oracle import az_oracle as ao

IDENTITY = [("gomoku", 7), ("gomoku", (5, 3)), ("gomoku", 15), ("tictactoe", None), ("connect4", None)]


@pytest.mark.parametrize("n_sims", (24, 64, 200))
@pytest.mark.parametrize("kind,size", IDENTITY)
def test_solver_off_is_the_reference_search(kind, size, n_sims):
    """Guards the yardstick: with solver=False the restatement's trees are fr.mcts' at k = 0 and oracle.mcts' - every node - from an empty
    board and from a position a few plies in, with a Dirichlet row; no status is written and nothing is counted."""
    og = ao.OracleGame(kind, size)
    ev = fr.hash_evaluator(og)
    for seed, plies in ((11, 0), (12, 3)):
        cells, to_move, mc = fr.position(og, seed, plies)
        noise = np.random.RandomState(seed).dirichlet([0.3] * og.action_dim)
        tree = ao.OracleTree(og, cap=1 << 16)
        tree.reset(to_move, mc)
        ao.mcts(og, tree, og.board_from_cells(cells, to_move), n_sims, ev, noise)
        plain = fr.RNode(None, None, to_move, mc)
        fr.mcts(og, plain, og.board_from_cells(cells, to_move), n_sims, ev, noise, 0.0)
        root = sr.SNode(None, None, to_move, mc)
        stats = sr.mcts(og, root, og.board_from_cells(cells, to_move), n_sims, ev, noise, solver=False)
        assert fr.same_tree(fr.export(root), fr.export(plain)), (kind, size, n_sims, seed)
        assert fr.same_tree(fr.export(root), tree.export()), (kind, size, n_sims, seed)
        assert not sr.export_status(root).any() and not any(stats.values())


def test_no_terminal_reached_means_the_plain_tree():
    """With the option on and no terminal reached the tree is the option-off tree bit for bit (Gomoku 7 x 7 from shallow positions)."""
    og = fr.oracle_game("gomoku7")
    ev = fr.hash_evaluator(og)
    for g in range(4):
        cells, to_move, mc = fr.position(og, 300 + g, g)
        noise = np.random.RandomState(g).dirichlet([0.3] * og.action_dim)
        s = sr.searched(og, ev, cells, to_move, mc, noise, 32)
        assert s["solver"]["stats"]["terminal_marked"] == 0
        assert fr.same_tree(s["solver"]["tree"], s["plain"]["tree"]) and not s["solver"]["status"].any()


@pytest.mark.parametrize("name", ("tictactoe", "connect4", "gomoku7"))
def test_invariants_hold_after_every_simulation(name):
    """What the header lists as consequences: an UNKNOWN node never has a WON child and has an UNKNOWN child; N[root] = 1 + sum N[child];
    at a root proven for its mover every further simulation goes to the first WON child."""
    og, slots = sr.tictactoe_case() if name == "tictactoe" else sr.constructed_case(name)
    ev = fr.hash_evaluator(og)
    for s in slots:
        root = sr.SNode(None, None, s["to_move"], s["move_count"])
        seen = {}

        def after(it, r, seen=seen):
            sr.check_invariants(r)
            if r.status == sr.LOST:                                   # lost for the player who moved into the root: its mover wins
                first = next(i for i, c in enumerate(r.children) if c.status == sr.WON)
                visits = [c.visit for c in r.children]
                if "visits" in seen:
                    grown = [i for i, (a, b) in enumerate(zip(seen["visits"], visits)) if a != b]
                    assert grown == [first]
                seen["visits"] = visits
        sr.mcts(og, root, og.board_from_cells(s["cells"], s["to_move"]), s["n_sims"], ev, s["noise"], True, after_sim=after)
        assert fr.same_tree(fr.export(root), s["solver"]["tree"])       # (the shared case is this very search)


def test_every_proven_status_is_the_minimax_value_on_tictactoe():
    """Every proven status of the eight TicTacToe searches equals an exhaustive minimax of that node's position."""
    og, slots = sr.tictactoe_case()
    ev = fr.hash_evaluator(og)
    proven = 0
    for s in slots:
        root = sr.SNode(None, None, s["to_move"], s["move_count"])
        board = og.board_from_cells(s["cells"], s["to_move"])
        sr.mcts(og, root, board, s["n_sims"], ev, s["noise"], True)

        def walk(nd):
            nonlocal proven
            if nd.parent is not None:
                og.make_move(board, 1 - nd.player, og.rc(nd.cell))
            if nd.status != sr.UNKNOWN and nd.parent is not None:
                assert nd.status == sr.minimax_status(og, board, nd), (nd.cell, nd.status)
                proven += 1
            for c in nd.children:
                walk(c)
            if nd.parent is not None:
                og.undo_move(board, nd.player, og.rc(nd.cell))
        walk(root)
        if root.status != sr.UNKNOWN:                                  # the root: minimax over its children, as the player who moved into it
            values = [sr.VALUE[sr.minimax_status(og, _after(og, board, c), c)] for c in root.children]
            assert sr.VALUE[root.status] == -max(values)
    assert proven >= 50


def _after(og, board, child):
    b = board.copy()
    og.make_move(b, 1 - child.player, og.rc(child.cell))
    return b


def test_check_solver_refusals():
    from selfplay import check_solver
    assert check_solver(None) is None and check_solver(False) is None and check_solver(True) is True
    for kw in (dict(evaluator=None), dict(evaluator=(object(), None)), dict(leaves_per_step=2), dict(forced_playouts=2.0),
               dict(gumbel_root=(16, 50.0, 1.0)), dict(puct=(1.5, None)), dict(tree_reuse=1), dict(tree_reuse=2)):
        with pytest.raises(ValueError):
            check_solver(True, **kw)
    with pytest.raises(ValueError):
        check_solver(1)


# ---- the preconditions of tests/test_gpu_solver.py --------------------------------------------------------------------------------------
def test_preconditions_tictactoe():
    """Over the TicTacToe slots at 64 simulations: at least five of the eight trees differ from the plain search; a node proven by one child,
    one proven by all-LOST and one proven DRAW occur; a simulation ends on a proven interior node; a root takes a status before the last
    simulation."""
    og, slots = sr.tictactoe_case()
    assert slots[0]["n_sims"] == 64 and len(slots) == 8
    assert sum(not fr.same_tree(s["solver"]["tree"], s["plain"]["tree"]) for s in slots) >= 5
    kinds = {e[1] for s in slots for e in s["solver"]["events"]}
    assert {"won_child", "all_lost", "all_draw", "stop"} <= kinds
    assert any(s["solver"]["decided_at"] is not None and s["solver"]["decided_at"] < 63 for s in slots)
    assert all(not any(s["plain"]["stats"].values()) and not s["plain"]["status"].any() for s in slots)


@pytest.mark.parametrize("name", ("connect4", "gomoku7"))
def test_preconditions_constructed(name):
    """Connect4 and Gomoku 7 x 7: a slot with a proven node and an exclusion (positions a few plies from a full board or from a four)."""
    og, slots = sr.constructed_case(name)
    assert any(s["solver"]["stats"]["proven_by_won_child"] + s["solver"]["stats"]["proven_by_all_children"] > 0
               and s["solver"]["stats"]["selections_excluding"] > 0 for s in slots)
    assert any(not fr.same_tree(s["solver"]["tree"], s["plain"]["tree"]) for s in slots)
    assert any(s["solver"]["stats"]["stopped_on_proven"] > 0 for s in slots)


@pytest.mark.parametrize("group", sorted(sr.WIDE_SLOTS))
def test_preconditions_wide(group):
    """The three root widths (56 / 60, 92 and 176 / 184 children: the three forms of the scan): every slot shows the selection outcome it is
    there for - a WON child taken (+infinity) or a LOST child shut out (-infinity) - on its precision path and in its scan form; at the
    root for every outcome the root can reach within the budget, below it otherwise."""
    og, slots, n_sims = sr.wide_group(group)
    assert len(slots) == 8
    at_root = set()
    for g, s in enumerate(slots):
        path, outcome, form = s["shows"]
        oc = sr.selection_outcomes(s["solver"]["events"])
        n_root = int((s["solver"]["tree"]["depth"] == 1).sum())
        assert sr.scan_form(n_root) == form or (path, outcome) == ("f32", "shut") and group == "noise", (group, g, n_root)
        assert (path, outcome, form, True) in oc or (path, outcome, form, False) in oc, (group, g, s["shows"], sorted(oc))
        at_root |= {o[:3] for o in oc if o[3]}
    path = "f64" if group == "noise" else "f32"
    for form in (1, 2, 3):                                              # at the ROOT: both outcomes in every form, on the group's path
        assert (path, "won", form) in at_root and (path, "shut", form) in at_root, (group, form, sorted(at_root))
