"""CPU: the restatement of (state, pi, z) emission under a mask of D4 elements (tests/emission_restated.py; include/azk.h
azk_config.emit_elements) against numpy's own flips, against the reference-pinned oracle on a square board, and against the host route
train.save_data_to_buffer(elements=...); the mask rules of selfplay.check_emit_symmetry; the config structure's layout."""
import ctypes

import numpy as np
import pytest

import emission_restated as er
from oracle import replay_oracle as ro


class _HostGame:
    """get_canonical_board without the device: the rule of games/game.py (the facade's runs a kernel)."""
    get_canonical_board = staticmethod(er.canonical)


class _ListBuffer(list):
    def add(self, state, pi, target):
        self.append((np.array(state, np.float32), np.array(pi, np.float64), float(target[0])))


def record(rows, cols, planes, action_dim, plies, winner, seed):
    """A game record as SelfPlayResult holds it: raw boards before each ply (player 0 = plane 0; plane 2 = the side to move), one pi per ply."""
    rng = np.random.RandomState(seed)
    order = rng.permutation(rows * cols)[:plies]
    board = np.zeros((planes, rows, cols), np.float32)
    boards, pis = [], []
    for i, c in enumerate(order):
        b = board.copy()
        if planes == 3:
            b[2] = i & 1
        boards.append(b)
        pis.append(rng.dirichlet(np.ones(action_dim)))
        board[i & 1, c // cols, c % cols] = 1.0
    return boards, pis, winner


def same(a, b):
    return len(a) == len(b) and all(x[0].dtype == np.float32 and np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]) and x[2] == y[2]
                                    for x, y in zip(a, b))


@pytest.mark.parametrize("winner", [0, 1, -1])
def test_all_eight_elements_on_a_square_board_are_the_reference_emission(winner):
    import train
    boards, pis, _ = record(5, 5, 2, 25, 11, winner, seed=3 + winner)
    got = er.emit_tuples("gomoku", boards, pis, winner, range(8))
    want = ro.emit_tuples(boards, pis, winner)
    assert len(got) == er.count_tuples(11, 8) == 74 and ro.digest(got) == ro.digest(want)
    buf = _ListBuffer()
    train.save_data_to_buffer(_HostGame, buf, (boards, None, pis, None, winner, 0 if winner == -1 else 1))      # elements=None: the reference's path
    assert same(got, buf)


@pytest.mark.parametrize("rows,cols", [(3, 5), (5, 3)])
def test_shape_keeping_elements_are_numpys_flips(rows, cols):
    rng = np.random.RandomState(rows)
    state = (rng.rand(2, rows, cols) < 0.4).astype(np.float32)
    pi = rng.dirichlet(np.ones(rows * cols))
    p2 = pi.reshape(rows, cols)
    want = {0: (state, p2), 1: (np.flip(state, 2), np.fliplr(p2)), 2: (np.flip(state, 1), np.flipud(p2)),
            6: (np.rot90(state, k=2, axes=(1, 2)), np.rot90(p2, k=2))}
    for s, (ws, wp) in want.items():
        ts, tp = er.turn(state, pi, s, "gomoku")
        assert np.array_equal(ts, ws) and np.array_equal(tp, wp.reshape(-1)), s
    tuples = er.emit_tuples("gomoku", [state] * 3, [pi] * 3, 0, (0, 1, 2, 6))
    assert len(tuples) == 2 + 4 and [t[2] for t in tuples] == [1.0, -1.0, 1.0, 1.0, 1.0, 1.0]
    for (ts, tp, _), s in zip(tuples[2:], (0, 1, 2, 6)):
        assert np.array_equal(ts, want[s][0]) and np.array_equal(tp, want[s][1].reshape(-1))


def test_connect4_policy_is_mirrored_with_the_board():
    rng = np.random.RandomState(4)
    state = (rng.rand(3, 6, 7) < 0.3).astype(np.float32)
    state[2] = 1.0
    pi = rng.dirichlet(np.ones(7))
    ts, tp = er.turn(state, pi, 1, "connect4")
    assert np.array_equal(ts, np.flip(state, 2)) and np.array_equal(tp, pi[::-1]) and np.all(ts[2] == 1.0)


CASES = [("connect4", 6, 7, 3, 7, (0, 1)), ("connect4", 6, 7, 3, 7, (0,)), ("gomoku", 5, 7, 2, 35, (0, 1, 2, 6)), ("gomoku", 5, 7, 2, 35, (0, 6))]


@pytest.mark.parametrize("game,rows,cols,planes,A,elements", CASES)
@pytest.mark.parametrize("capped", [False, True])
def test_host_route_equals_the_restatement(game, rows, cols, planes, A, elements, capped):
    import train
    for winner in (0, 1, -1):
        boards, pis, _ = record(rows, cols, planes, A, 13, winner, seed=7 + winner)
        full = [bool(x) for x in np.random.RandomState(winner + 5).rand(13) < 0.6] if capped else None
        if capped:
            full[0], full[1], full[2] = True, False, True              # both group sizes among the kept plies, a dropped early ply
        buf = _ListBuffer()
        train.save_data_to_buffer(_HostGame, buf, (boards, None, pis, None, winner, 0 if winner == -1 else 1), full=full, elements=elements)
        want = er.emit_tuples(game, boards, pis, winner, elements, full=full)
        assert same(want, buf)
        kept = [i for i in range(13) if full is None or full[i]]
        assert len(buf) == sum(1 if i < 2 else len(elements) for i in kept)


def test_host_route_refuses_a_transposing_element_on_a_rectangle():
    import train
    boards, pis, winner = record(5, 7, 2, 35, 4, 0, seed=1)
    with pytest.raises(ValueError):
        train.save_data_to_buffer(_HostGame, _ListBuffer(), (boards, None, pis, None, winner, 1), elements=(0, 3))
    with pytest.raises(ValueError):
        train.element_image(np.zeros((3, 6, 7), np.float32), np.full(7, 1 / 7), 2)


def test_check_emit_symmetry_masks():
    from selfplay import check_emit_symmetry, mask_elements
    assert check_emit_symmetry(None, "gomoku", 7) == 0
    assert check_emit_symmetry("board", "gomoku", 7) == 0xFF and check_emit_symmetry("board", "tictactoe") == 0xFF
    assert check_emit_symmetry("board", "gomoku", (5, 7)) == 0x47 and check_emit_symmetry("board", "connect4") == 0x03
    assert check_emit_symmetry("none", "connect4") == 1 and check_emit_symmetry([0, 6], "gomoku", (5, 7)) == 0x41
    assert check_emit_symmetry((0, 3, 7), "gomoku", 7) == 0x89 and mask_elements(0x47) == (0, 1, 2, 6)
    for bad, game, size in (((0, 3), "gomoku", (5, 7)), ((0, 2), "connect4", None), ((1, 2), "gomoku", 7), ((0, 8), "gomoku", 7), ((), "gomoku", 7),
                            ("all", "gomoku", 7), ((0, 1.5), "gomoku", 7), (5, "gomoku", 7)):
        with pytest.raises(ValueError):
            check_emit_symmetry(bad, game, size)


def test_config_has_the_field_and_keeps_its_size():
    import azk
    names = [n for n, _ in azk.structs.Config._fields_]
    assert names[-2:] == ["emit_elements", "reserved"] and names.index("emit_elements") == 12
    assert ctypes.sizeof(azk.structs.Config) == 16 * 4 and azk.structs.Config.emit_elements.offset == 12 * 4
    assert azk.ABI_VERSION == 5


def test_game_size_reaches_the_engine_as_rows_and_cols():
    """Game._size(): what Engine, rules_* and self_play_batch are handed - one side for a square Gomoku board, (rows, cols) for a subclass with
    rows != cols (it used to be `rows`, a square board of the wrong shape), None for the fixed-size games."""
    from games import Connect4, Gomoku, TicTacToe

    class Gomoku5x7(Gomoku):
        rows, cols = 5, 7
        action_dim = state_dim = 35

    class Gomoku9(Gomoku):
        rows = cols = 9
        action_dim = state_dim = 81
    assert Gomoku._size() == Gomoku.rows == Gomoku.cols and Gomoku9._size() == 9 and Gomoku5x7._size() == (5, 7)
    assert Connect4._size() is None and TicTacToe._size() is None


def test_gather_pick_is_the_evaluation_symmetrys_pick():
    els = (0, 1, 2, 6)
    assert [er.pick_element(h << 16, els) for h in (0, 1, 0x3FFF, 0x4000, 0x7FFF, 0x8000, 0xBFFF, 0xC000, 0xFFFF)] == [0, 0, 0, 1, 1, 2, 2, 6, 6]
    assert er.pick_element(-1, els) == 6 and er.pick_element(-(1 << 31), (0, 1)) == 1 and er.pick_element(0x7FFFFFFF, (0, 1)) == 0
