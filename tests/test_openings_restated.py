"""Random openings (azk_set_openings), CPU only: the restated draws (tests/openings_restated.py) behave as the rule says,
the shapes tests/test_gpu_openings.py runs meet their preconditions on the restatement alone, and the runners refuse bad settings before
any engine exists."""
import pytest

import openings_restated as R

SEED = 11                      # the openings' own seed in the GPU tests
KEYS = (0, 7)                  # the two move keys the kernel test opens every slot under
SLOTS = 64
EDGE_SEED, EDGE_FIRST = (1 << 64) - 1, (1 << 32) - 2      # the first game straddles the word boundary of the global game index
TTT = (1.0, 8, -1)             # TicTacToe: whole board, up to state_dim - 1 plies
C4_MID = (1.0, 10, 0)          # Connect4: the middle column alone


def test_p_open_zero_opens_nothing_and_one_opens_everything():
    for g in range(SLOTS):
        for key in range(40):
            assert R.game_draw(SEED, g, key, 0.0, 8) == (False, 0)
            opened, n = R.game_draw(SEED, g, key, 1.0, 8)
            assert opened and 1 <= n <= 8


def test_lengths_cover_one_to_max_plies_and_the_share_follows_p_open():
    draws = [R.game_draw(SEED, g, key, 0.5, 6) for g in range(SLOTS) for key in range(40)]
    assert {n for opened, n in draws if opened} == set(range(1, 7))
    share = sum(1 for opened, _ in draws if opened) / len(draws)
    assert 0.45 < share < 0.55, share                                # 2560 coins: three standard deviations are 0.03
    assert all(n == 0 for opened, n in draws if not opened)


def test_every_word_of_the_key_is_live_at_the_edges():
    """The edge seed (2^64 - 1) and first game (2^32 - 2: slots 0..3 straddle the word boundary) change the draws word by word."""
    base = [R.philox4x32_10([(EDGE_FIRST + g) & R.M32, (EDGE_FIRST + g) >> 32, 5, R.TAG], EDGE_SEED & R.M32, EDGE_SEED >> 32) for g in range(4)]
    assert len({tuple(w) for w in base}) == 4
    assert [(EDGE_FIRST + g) >> 32 for g in range(4)] == [0, 0, 1, 1]
    u = R.ply_uniform(EDGE_SEED, EDGE_FIRST + 2, 5, 0)
    assert u != R.ply_uniform(EDGE_SEED, EDGE_FIRST + 2 - (1 << 32), 5, 0)          # the high word of the game index
    assert u != R.ply_uniform(EDGE_SEED ^ (1 << 63), EDGE_FIRST + 2, 5, 0)          # the high word of the seed
    assert u != R.ply_uniform(EDGE_SEED ^ 1, EDGE_FIRST + 2, 5, 0)                  # the low word of the seed
    assert u != R.ply_uniform(EDGE_SEED, EDGE_FIRST + 2, 6, 0) and u != R.ply_uniform(EDGE_SEED, EDGE_FIRST + 2, 5, 1)
    # a ply draw is never the game draw: j + 1 >= 1 sits in bits 8.. of word 1
    w_game = R.philox4x32_10([7, 0, 5, R.TAG], SEED, 0)
    assert R.ply_uniform(SEED, 7, 5, 0) != R._u(w_game[0], w_game[1])
    # a negative key (none occurs) would be its low 32 bits, as for the resignation coin
    assert R.game_draw(SEED, 3, -1, 0.5, 8) == R.game_draw(SEED, 3, 0xFFFFFFFF, 0.5, 8)


def test_precondition_tictactoe_has_cut_short_and_full_length_openings():
    from oracle import az_oracle as ao
    og = ao.OracleGame("tictactoe")
    opens = [R.open_game(og, SEED, g, key, TTT) for key in KEYS for g in range(SLOTS)]
    assert any(o.cut for o in opens) and any(o.plies == o.n == 8 for o in opens), R.stats_of(opens)
    for o in opens:                                                 # never terminal, always a legal move
        assert o.plies < 9 and (o.codes() == 0).any()
        assert o.plies == len(o.cells) and o.player == o.plies & 1


def test_precondition_connect4_middle_column_fills_up():
    from oracle import az_oracle as ao
    og = ao.OracleGame("connect4")
    opens = [R.open_game(og, SEED, g, key, C4_MID) for key in KEYS for g in range(SLOTS)]
    full = [o for o in opens if o.ended_empty]
    assert full and all(o.plies == 6 and [c % 7 for c in o.cells] == [3] * 6 for o in full)
    assert all(not o.cut for o in opens)                            # alternating stones in one column never make four


def test_window_per_axis_on_even_and_odd_extents():
    inside = lambda rows, cols, s: [(r, c) for r in range(rows) for c in range(cols) if R.in_window(rows, cols, r, c, s)]
    assert inside(5, 9, 1) == [(r, c) for r in (1, 2, 3) for c in (3, 4, 5)]
    assert inside(4, 4, 0) == []                                    # an even extent has no centre line: spread 0 holds no cell
    assert inside(4, 4, 1) == [(r, c) for r in (1, 2) for c in (1, 2)]
    assert len(inside(20, 20, -1)) == 400
    assert [c for c in range(7) if R.in_window(6, 7, 0, c, 1, True)] == [2, 3, 4]


def test_refusals_before_any_engine_exists():
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_openings, self_play_batch
    ev = lambda x: None
    assert check_openings(None, "gomoku", 7) is None and check_openings((0.5, 8, 2), "gomoku", 7) == (0.5, 8, 2)
    assert check_openings((1, 48, -1), "gomoku", 7) == (1.0, 48, -1) and check_openings((0, 41, 0), "connect4") == (0.0, 41, 0)
    assert check_openings((0.5, 39, 0), "gomoku", (5, 8)) == (0.5, 39, 0)
    for bad in ((-0.1, 4, 0), (1.5, 4, 0), (float("nan"), 4, 0), (0.5, 0, 0), (0.5, 49, 0), (0.5, 4, -2), (0.5, 4.5, 0), (0.5, 4), (0.5, 4, 0, 0), "x", 0.5):
        with pytest.raises(ValueError):
            check_openings(bad, "gomoku", 7)
        with pytest.raises(ValueError):
            SelfPlayRunner("gomoku", ev, 2, 24, size=7, openings=bad)
        with pytest.raises(ValueError):
            AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, openings=bad)
        with pytest.raises(ValueError):
            self_play_batch("gomoku", ev, 2, 24, size=7, openings=bad)
    for game, size, cells in (("tictactoe", None, 9), ("connect4", None, 42), ("gomoku", (1, 3), 3), ("gomoku", 2, 4)):
        assert check_openings((0.5, cells - 1, -1), game, size)[1] == cells - 1
        with pytest.raises(ValueError, match="max_plies"):
            check_openings((0.5, cells, -1), game, size)            # max_plies >= state_dim
    for make in (lambda: SelfPlayRunner("gomoku", None, 2, 24, size=7, openings=(0.5, 4, 1)),
                 lambda: AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, openings=(0.5, 4, 1)),
                 lambda: self_play_batch("gomoku", None, 2, 24, size=7, openings=(0.5, 4, 1)),
                 lambda: self_play_batch("gomoku", (ev, None), 2, 24, size=7, openings=(0.5, 4, 1))):
        with pytest.raises(ValueError, match="vanilla"):
            make()
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 24, batched=False, openings=(0.5, 4, 1))
    # the arena: an odd number of games has no pairs; a vanilla side, a bad range and unequal iteration counts are refused too
    import arena
    with pytest.raises(ValueError, match="even"):
        arena.compare("gomoku", ev, ev, 24, 24, 7, False, False, size=7, openings=(4, 1))
    with pytest.raises(ValueError, match="vanilla"):
        arena.compare("gomoku", None, ev, 24, 24, 8, False, False, size=7, openings=(4, 1))
    for bad in ((0, 1), (49, 1), (4, -2), (4,), 4):
        with pytest.raises(ValueError):
            arena.compare("gomoku", ev, ev, 24, 24, 8, False, False, size=7, openings=bad)
    with pytest.raises(ValueError, match="same number"):
        arena.compete_batch("gomoku", ev, ev, 4, 24, 32, size=7, openings=(4, 1))
