"""CPU: the restatement of evaluation under a board symmetry (tests/eval_symmetry_restated.py; include/azk.h azk_set_eval_symmetry) against
numpy's own rot90 / fliplr / flipud in the emission's order, the hash condition the header states, the wrapper's algebra on the oracle's
search with an evaluator that is equivariant, and the refusals selfplay.check_eval_symmetry makes before any engine exists."""
import itertools
import math

import numpy as np
import pytest
import torch

import eval_symmetry_restated as es

SEEDS = (0, 1, 12345, 2 ** 40 + 7)


def numpy_element(b, s):
    """Element s of the emission's order (train.py:8-27: rot0, lr, tb, rot90, lr, tb, rot180, rot270) by numpy."""
    r = np.rot90(b, {0: 0, 1: 0, 2: 0, 3: 1, 4: 1, 5: 1, 6: 2, 7: 3}[s])
    return np.fliplr(r) if s in (1, 4) else np.flipud(r) if s in (2, 5) else r


# ---- 1. the maps --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 7, 15])
def test_maps_are_numpys_compositions_on_square_boards(n):
    b = np.arange(n * n).reshape(n, n)
    for s in range(8):
        src = es.src_map(s, n, n)
        assert np.array_equal(b.reshape(-1)[src].reshape(n, n), numpy_element(b, s)), s
        assert np.array_equal(es.dst_map(s, n, n)[src], np.arange(n * n)), s
        assert np.array_equal(es.dst_map(s, n, n), es.src_map(es.INVERSE[s], n, n)), s
        x = np.random.RandomState(s).rand(3, 2, n, n).astype(np.float32)
        assert np.array_equal(es.transform_planes(x, s), np.stack([[numpy_element(p, s) for p in bb] for bb in x])), s
        assert torch.equal(es.transform_planes(torch.from_numpy(x), s), torch.from_numpy(es.transform_planes(x, s)))
        row = np.random.RandomState(s).rand(n * n).astype(np.float32)
        # a policy row that was turned like the board comes back
        assert np.array_equal(es.restore_rows(row[src], s, "gomoku", n, n), row), s


@pytest.mark.parametrize("rows,cols", [(1, 3), (4, 6), (6, 4), (17, 18), (6, 7)])
def test_maps_and_valid_sets_on_rectangular_boards(rows, cols):
    assert es.valid_elements("gomoku", rows, cols) == (0, 1, 2, 6)
    b = np.arange(rows * cols).reshape(rows, cols)
    for s in (0, 1, 2, 6):
        src = es.src_map(s, rows, cols)
        assert np.array_equal(b.reshape(-1)[src].reshape(rows, cols), numpy_element(b, s)), s
        assert np.array_equal(es.dst_map(s, rows, cols)[src], np.arange(rows * cols)), s
    for s in (3, 4, 5, 7):
        with pytest.raises(AssertionError):
            es.src_map(s, rows, cols)


def test_valid_sets_and_connect4_action_map():
    assert es.valid_elements("tictactoe", 3, 3) == es.valid_elements("gomoku", 15, 15) == tuple(range(8))
    assert es.valid_elements("connect4", 6, 7) == (0, 1)
    assert es.action_dst_map(0, "connect4", 6, 7).tolist() == list(range(7))
    assert es.action_dst_map(1, "connect4", 6, 7).tolist() == [6, 5, 4, 3, 2, 1, 0]
    # a stone dropped in column a of the mirrored board is a stone in column cols - 1 - a of the board
    b = np.zeros((6, 7), np.int8)
    b[5, 2] = 1
    assert es.transform_cells(b, 1, 6, 7).reshape(6, 7)[5, 4] == 1


# ---- 2. the hash ------------------------------------------------------------------------------------------------------------------------
def balanced_boards():
    """The 3 x 3 boards alternating play can reach by stone counts: equal, or the first player one ahead; with the side to move."""
    out = []
    for cells in itertools.product((0, 1, 2), repeat=9):
        a, b = cells.count(1), cells.count(2)
        if a == b or a == b + 1:
            out.append((cells, a - b))
    return out


def test_hash_spreads_the_balanced_3x3_boards_evenly():
    boards = balanced_boards()
    n = len(boards)
    assert n == 6046
    picks = {}
    for seed in SEEDS:
        for valid in (tuple(range(8)), (0, 1, 2, 6), (0, 1)):
            els = [es.position_element(seed, c, side, valid) for c, side in boards]
            picks[(seed, len(valid))] = els
            p = 1.0 / len(valid)
            sigma = math.sqrt(p * (1 - p) / n)
            for e in valid:
                share = els.count(e) / n
                print(seed, len(valid), e, "share", share, "sigmas", abs(share - p) / sigma)
                assert abs(share - p) <= 4 * sigma, (seed, valid, e, share)
            assert set(els) == set(valid)
    # two seeds are two keys: they agree on about 1 / n_valid of the boards
    for nv in (8, 4, 2):
        p = 1.0 / nv
        sigma = math.sqrt(p * (1 - p) / n)
        for a, b in itertools.combinations(SEEDS, 2):
            agree = sum(x == y for x, y in zip(picks[(a, nv)], picks[(b, nv)])) / n
            print(a, b, nv, "agree", agree, "sigmas", abs(agree - p) / sigma)
            assert abs(agree - p) <= 4 * sigma, (a, b, nv, agree)


def test_hash_sees_the_side_to_move_and_the_stone_colours():
    cells = [0, 1, 2, 0, 0, 0, 0, 0, 0]
    swapped = [0, 2, 1, 0, 0, 0, 0, 0, 0]
    v8 = tuple(range(8))
    a = [es.position_element(s, cells, 0, v8) for s in range(64)]
    assert a != [es.position_element(s, cells, 1, v8) for s in range(64)]
    assert a != [es.position_element(s, swapped, 0, v8) for s in range(64)]
    assert es.cells_and_side(es.canonical_planes(cells, 0, 2, 3, 3))[0].tolist() == cells
    assert es.cells_and_side(es.canonical_planes([1, 1, 2, 0, 0, 0, 0, 0, 0], 1, 2, 3, 3)) [1] == 1
    assert es.cells_and_side(es.canonical_planes(cells, 1, 3, 3, 3))[1] == 1


# ---- 3. the wrapper's algebra, on the oracle's search ---------------------------------------------------------------------------------------
ALGEBRA = [("tictactoe", None, []), ("connect4", None, [38, 39, 31]), ("gomoku", 5, [12, 13]), ("gomoku", (4, 6), [8, 9, 14])]


def oracle_search(ao, game, board, player, plies, n_sims, batch_evaluator, noise=None):
    tree = ao.OracleTree(game)
    tree.reset(player, plies)

    def ev(canon):
        logits, v = batch_evaluator(torch.from_numpy(np.ascontiguousarray(canon))[None])
        return ao.softmax_det(logits[0].numpy()), float(v[0])
    ao.mcts(game, tree, board, n_sims, ev, noise)
    return tree.export()


def same_tree(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in ("depth", "cell", "visit", "value", "prior"))


@pytest.mark.parametrize("name,size,moves", ALGEBRA, ids=[f"{a[0]}{a[1]}" for a in ALGEBRA])
def test_an_equivariant_evaluator_wrapped_in_any_element_searches_the_same_tree(name, size, moves):
    from oracle import az_oracle as ao
    from selfplay import eval_symmetry_elements
    game = ao.OracleGame(name, size)
    valid = eval_symmetry_elements(name, size)
    assert valid == es.valid_elements(name, game.rows, game.cols)
    board, player = game.new_board(), 0
    for cell in moves:
        player = game.make_move(board, player, game.rc(cell))
    noise = np.random.RandomState(7).dirichlet([0.3] * game.action_dim)
    f = lambda x: es.equivariant_logits_value(x, game.action_dim)
    want = oracle_search(ao, game, board, player, len(moves), 40, f, noise)
    assert len(want["depth"]) > 20
    for mode, value in [(2, s) for s in valid] + [(1, 5), (1, 2 ** 40 + 7)]:
        got = oracle_search(ao, game, board, player, len(moves), 40, es.wrap(f, name, game.rows, game.cols, mode, value), noise)
        assert same_tree(got, want), (mode, value)
    # and the fixture the other tests wrap is NOT equivariant: some element gives another tree
    from fixture_eval import fixture_logits_value
    h = lambda x: fixture_logits_value(x, game.action_dim, "hash")
    plain = oracle_search(ao, game, board, player, len(moves), 40, h, noise)
    assert any(not same_tree(oracle_search(ao, game, board, player, len(moves), 40, es.wrap(h, name, game.rows, game.cols, 2, s), noise), plain)
               for s in valid[1:])


# ---- 4. refusals before any engine exists ---------------------------------------------------------------------------------------------------
def test_check_eval_symmetry_refuses_what_the_engine_refuses():
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_eval_symmetry, eval_symmetry_elements, self_play_batch
    ev = lambda x: None
    assert check_eval_symmetry(None, "gomoku", 7) is None and check_eval_symmetry(False, "gomoku", 7) is None
    assert check_eval_symmetry(True, "gomoku", 7, seed=11) == (1, 11)
    assert check_eval_symmetry(("fixed", 3), "gomoku", 7) == (2, 3) and check_eval_symmetry(("fixed", 1), "connect4") == (2, 1)
    assert check_eval_symmetry(("fixed", 6), "gomoku", (4, 6)) == (2, 6) and check_eval_symmetry(("fixed", 7), "tictactoe") == (2, 7)
    for game, size in (("gomoku", 15), ("gomoku", (4, 6)), ("gomoku", (6, 4)), ("connect4", None), ("tictactoe", None)):
        rows, cols = {"connect4": (6, 7), "tictactoe": (3, 3)}.get(game, size if isinstance(size, tuple) else (size, size))
        assert eval_symmetry_elements(game, size) == es.valid_elements(game, rows, cols)
    for bad, game, size in ((("fixed", 3), "gomoku", (4, 6)), (("fixed", 2), "connect4", None), (("fixed", 8), "gomoku", 7), (("fixed", -1), "gomoku", 7),
                            (("fixed", 1.5), "gomoku", 7), (("turn", 1), "gomoku", 7), ("x", "gomoku", 7), (3, "gomoku", 7)):
        with pytest.raises(ValueError, match="eval_symmetry"):
            check_eval_symmetry(bad, game, size)
    with pytest.raises(ValueError, match="vanilla"):
        check_eval_symmetry(True, "gomoku", 7, evaluator=None)
    with pytest.raises(ValueError, match="leaves_per_step"):
        check_eval_symmetry(True, "gomoku", 7, leaves_per_step=2)
    # the entry points validate before they create an engine (no GPU here, none needed)
    with pytest.raises(ValueError, match="eval_symmetry"):
        SelfPlayRunner("gomoku", ev, 4, 8, size=(4, 6), eval_symmetry=("fixed", 3))
    with pytest.raises(ValueError, match="vanilla"):
        SelfPlayRunner("gomoku", None, 4, 8, size=7, eval_symmetry=True)
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 4, 8, size=7, leaves_per_step=2, use_graph=True, eval_symmetry=True)
    with pytest.raises(ValueError, match="eval_symmetry"):
        AsyncSelfPlayRunner("connect4", ev, 4, 8, eval_symmetry=("fixed", 2))
    with pytest.raises(ValueError, match="vanilla"):
        AsyncSelfPlayRunner("gomoku", None, 4, 8, size=7, eval_symmetry=True)
    with pytest.raises(ValueError, match="vanilla"):
        self_play_batch("gomoku", None, 2, 8, size=7, eval_symmetry=True)
    with pytest.raises(ValueError, match="eval_symmetry"):
        self_play_batch("gomoku", ev, 2, 8, size=(6, 4), eval_symmetry=("fixed", 5))
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 8, batched=False, eval_symmetry=True)
