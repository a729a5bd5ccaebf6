"""CPU: policy surprise weighting (include/azk.h azk_set_surprise_weighting) - the restated rule
(tests/surprise_restated.py) against hand-worked cases, the product's numpy rule (selfplay.surprise_copies) and host route
(train.save_data_to_buffer(copies=...)) against the restatement, the coin's stream, and the refusals that come before any engine."""
import math

import numpy as np
import pytest

import emission_restated as er
import rng_restated as rr
import surprise_restated as sr
from test_emission_restated import _HostGame, _ListBuffer, record, same


# ---- the copy rule, by hand --------------------------------------------------------------------------------------------------------
def test_lambda_zero_is_one_copy_each_and_lambda_one_follows_kl_alone():
    kls, coins = [0.5, 0.0, 1.5, 2.0], [0.0, 0.999, 0.5, 0.25]
    assert sr.weights(kls, 0.0) == [1.0] * 4 and sr.copies(kls, coins, 0.0) == [1] * 4
    # lambda = 1: w = 4 * kl / 4 = kl
    assert sr.weights(kls, 1.0) == [0.5, 0.0, 1.5, 2.0]
    assert sr.copies(kls, coins, 1.0) == [1, 0, 1, 2]             # 0.5: coin 0 < 0.5; 0: none; 1.5: coin 0.5 is not < 0.5; 2: exactly two
    # lambda = 0.5: w = 0.5 + 0.5 * kl
    assert sr.weights(kls, 0.5) == [0.75, 0.5, 1.25, 1.5]
    assert sr.copies(kls, coins, 0.5) == [1, 0, 1, 2]             # coin 0.999 >= 0.5 drops the second ply; 0.25 < 0.5 doubles the last


def test_a_game_without_surprise_and_one_ply_games():
    assert sr.weights([0.0, 0.0, 0.0], 0.7) == [1.0] * 3 and sr.copies([0.0, 0.0, 0.0], [0.0, 0.5, 0.99], 0.7) == [1, 1, 1]      # S = 0
    for lam in (0.0, 0.3, 1.0):
        assert sr.weights([0.25], lam) == [1.0] and sr.copies([0.25], [0.0], lam) == [1]      # one ply: w = (1 - lam) + lam * 1 * kl / kl
        assert sr.copies([0.0], [0.5], lam) == [1]
    assert sr.copies([], [], 0.5) == []


@pytest.mark.parametrize("lam", [0.0, 0.25, 0.5, 1.0])
def test_weights_sum_to_the_number_of_recorded_plies(lam):
    rng = np.random.RandomState(5)
    for n in (1, 2, 7, 49, 400):
        kls = rng.gamma(0.5, 0.8, n)
        assert abs(math.fsum(sr.weights(kls, lam)) - n) <= 1e-12 * n
        full = rng.rand(n) < 0.5
        full[rng.randint(n)] = True
        w = sr.weights(kls, lam, full)
        assert abs(math.fsum(w) - int(full.sum())) <= 1e-12 * n and all(w[i] == 0.0 for i in range(n) if not full[i])
        assert max(w) <= int(full.sum()) + 1e-9


def test_a_coin_at_exactly_the_fraction_gives_no_extra_copy():
    # w = 0.5 + 0.5 * 2 * kl / 2 = 0.5 + 0.5 * kl -> 1.25 and 0.75
    kls = [1.5, 0.5]
    assert sr.weights(kls, 0.5) == [1.25, 0.75]
    assert sr.copies(kls, [0.25, 0.75], 0.5) == [1, 0]            # coin == frac(w): strict comparison, no extra copy
    below = [math.nextafter(0.25, 0.0), math.nextafter(0.75, 0.0)]
    assert sr.copies(kls, below, 0.5) == [2, 1]


def test_capped_games_whose_first_full_ply_is_not_ply_zero():
    kls, coins = [9.0, 9.0, 1.0, 9.0, 3.0], [0.0] * 5
    full = [False, False, True, False, True]
    # F = {2, 4}: n_F = 2, S = 4; lambda = 1: w = 2 * kl / 4
    assert sr.weights(kls, 1.0, full) == [0.0, 0.0, 0.5, 0.0, 1.5]
    assert sr.copies(kls, coins, 1.0, full) == [0, 0, 1, 0, 2]
    assert sr.copies(kls, [0.9] * 5, 1.0, full) == [0, 0, 0, 0, 1]
    boards, pis, _ = record(5, 5, 2, 25, 5, 0, seed=2)
    tuples, c = sr.game_tuples("gomoku", boards, pis, 0, range(8), kls, coins, 1.0, full)
    assert c == [0, 0, 1, 0, 2] and len(tuples) == 8 + 16
    group2, group4 = er.emit_tuples("gomoku", boards, pis, 0, range(8), full=[i == 2 for i in range(5)]), er.emit_tuples(
        "gomoku", boards, pis, 0, range(8), full=[i == 4 for i in range(5)])
    assert same(tuples, group2 + group4 + group4)                  # copy-major: the whole group, then the whole group again


def test_kl_by_hand():
    k, sa, n = sr.kl([0.5, 0.0, 0.5], np.asarray([0.25, 0.5, 0.25], np.float32))
    assert n == 2 and k == sa == math.log(2.0)
    k, sa, n = sr.kl([1.0, 0.0], np.asarray([0.0, 1.0], np.float32))      # a prior that underflowed: floored at 2^-126
    assert n == 1 and abs(k - 126 * math.log(2.0)) < 1e-12 and sa == k
    assert sr.kl([0.25, 0.75], np.asarray([0.25, 0.75], np.float32))[0] == 0.0


# ---- the product's numpy rule and host route -------------------------------------------------------------------------------------
def test_surprise_copies_equals_the_restatement_bit_for_bit():
    from selfplay import surprise_copies
    rng = np.random.RandomState(11)
    for trial in range(300):
        n = int(rng.randint(1, 60))
        kls = rng.gamma(0.4, 1.0, n) * (rng.rand(n) < 0.9)
        if trial % 10 == 0:
            kls[:] = 0.0
        coins = rng.rand(n)
        lam = float(rng.choice([0.0, 0.25, 0.5, 1.0, rng.rand()]))
        full = None if trial % 2 else list(rng.rand(n) < 0.5)
        got = surprise_copies(kls, coins, lam, full)
        assert got.tolist() == sr.copies(kls, coins, lam, full), (trial, lam)
        assert got.dtype == np.int64 and (full is None or all(got[i] == 0 for i in range(n) if not full[i]))


CASES = [("gomoku", 5, 5, 2, 25, None), ("connect4", 6, 7, 3, 7, (0, 1)), ("gomoku", 5, 7, 2, 35, (0, 1, 2, 6)), ("gomoku", 5, 7, 2, 35, (0,))]


@pytest.mark.parametrize("game,rows,cols,planes,A,elements", CASES)
@pytest.mark.parametrize("capped", [False, True])
def test_host_route_with_copies_equals_the_restated_tuple_list(game, rows, cols, planes, A, elements, capped):
    import train
    from selfplay import surprise_copies
    for winner in (0, 1, -1):
        boards, pis, _ = record(rows, cols, planes, A, 13, winner, seed=17 + winner)
        rng = np.random.RandomState(winner + 9)
        kls, coins = rng.gamma(0.4, 1.0, 13), rng.rand(13)
        full = [bool(x) for x in rng.rand(13) < 0.6] if capped else None
        if capped:
            full[0], full[1], full[2] = False, True, True
        c = surprise_copies(kls, coins, 0.5, full)
        buf = _ListBuffer()
        train.save_data_to_buffer(_HostGame, buf, (boards, None, pis, None, winner, 0 if winner == -1 else 1), full=full, elements=elements, copies=c)
        want, cr = sr.game_tuples(game, boards, pis, winner, elements if elements is not None else range(8), kls, coins, 0.5, full)
        assert cr == c.tolist() and same(want, buf)
        assert min(cr) == 0 and max(cr) >= 2                      # both kinds of ply occur in every case


# ---- the coin ----------------------------------------------------------------------------------------------------------------
def test_the_coin_is_a_stream_of_its_own():
    for seed in (0, 3, 2 ** 40 + 7):
        for gg in (0, 5, 2 ** 33 + 1):
            for move in (0, 1, 29):
                u = sr.coin(seed, gg, move)
                assert u == float(rr._keyed_u(seed, gg, move, 0xFFFFFFFC)) and 0.0 <= u < 1.0
                assert u != float(rr.move_uniform(seed, gg, move)) and u != float(rr.coin(seed, gg, move))
                assert u != float(rr._keyed_u(seed, gg, move, 0xFFFFFFFD))     # resignation's game coin
    us = [sr.coin(3, g, m) for g in range(8) for m in range(30)]
    assert len(set(us)) == len(us) and 0.35 < sum(us) / len(us) < 0.65


# ---- the refusals, before any engine exists ----------------------------------------------------------------------------------------
def test_refusals_before_any_engine_exists():
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_surprise_weight, self_play_batch
    assert check_surprise_weight(None) is None and check_surprise_weight(0) == 0.0 and check_surprise_weight(0.5) == 0.5 and check_surprise_weight(1) == 1.0
    ev = lambda x: None
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "x", (0.5,), True):
        with pytest.raises(ValueError):
            check_surprise_weight(bad)
        with pytest.raises(ValueError):
            SelfPlayRunner("gomoku", ev, 2, 24, size=7, surprise_weight=bad)
        with pytest.raises(ValueError):
            AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, surprise_weight=bad)
        with pytest.raises(ValueError):
            self_play_batch("gomoku", ev, 2, 24, size=7, surprise_weight=bad)
        with pytest.raises(ValueError):
            az_train.collect_data(None, ev, None, 1, 24, surprise_weight=bad)
    for make in (lambda: SelfPlayRunner("gomoku", None, 2, 24, size=7, surprise_weight=0.5),
                 lambda: AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, surprise_weight=0.5),
                 lambda: self_play_batch("gomoku", None, 2, 24, size=7, surprise_weight=0.5),
                 lambda: self_play_batch("gomoku", (ev, None), 2, 24, size=7, surprise_weight=0.5),
                 lambda: az_train.collect_data(None, None, None, 1, 24, surprise_weight=0.5)):
        with pytest.raises(ValueError, match="vanilla"):
            make()
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, use_graph=True, leaves_per_step=2, surprise_weight=0.5)
    with pytest.raises(ValueError, match="leaves_per_step"):
        self_play_batch("gomoku", ev, 2, 24, size=7, leaves_per_step=2, surprise_weight=0.5)
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, ev, None, 1, 24, batched=False, surprise_weight=0.5)
