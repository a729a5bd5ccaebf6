"""CPU: value targets (include/azk.h azk_set_value_target) - the restated rule (tests/value_target_restated.py) against
its closed form and its identity cases, the product's numpy rule (selfplay.value_targets) and host route
(train.save_data_to_buffer(values=...)) against the restatement, and the refusals that come before any engine."""
import math
import struct

import numpy as np
import pytest

import emission_restated as er
import surprise_restated as sr
import value_target_restated as vr
from test_emission_restated import _HostGame, _ListBuffer, record, same


def bits(x):
    return struct.pack("<d", float(x))


# ---- the rule ---------------------------------------------------------------------------------------------------------------------
def test_by_hand():
    # three plies, player 0 wins: z = +1, -1, +1; q = value for the mover's opponent, v = -q
    qs = [-0.5, 0.25, -1.0]
    assert vr.targets(qs, 0, 0, 1.0, 0.0) == [0.5, -0.25, 1.0]                     # r = 1, lam = 0: the ply's own search value
    assert vr.targets(qs, 0, 0, 0.5, 0.0) == [0.75, -0.625, 1.0]                   # Leela's q-ratio at 0.5
    # lam = 0.5: G2 = 0.5 * 1 + 0.5 * 1 = 1; G1 = 0.5 * -0.25 + 0.5 * -1 = -0.625; G0 = 0.5 * 0.5 + 0.5 * 0.625 = 0.5625
    assert vr.targets(qs, 0, 0, 1.0, 0.5) == [0.5625, -0.625, 1.0]
    assert vr.targets(qs, 0, 1, 1.0, 0.0) == [0.5, -0.25, 1.0] and vr.targets(qs, 0, 1, 0.0, 0.0) == [-1.0, 1.0, -1.0]      # first_ply 1: sides swap
    assert vr.targets([], 0, 0, 0.5, 0.5) == []


@pytest.mark.parametrize("lam", [0.0, 0.3, 0.7, 0.9, 1.0])
def test_the_loop_equals_the_closed_form(lam):
    """Within 1e-12: at most 225 terms of magnitude <= 1, each with a few roundings of 2^-53 (225 * 4 * 2^-53 = 1e-13)."""
    rng = np.random.RandomState(int(lam * 10) + 1)
    worst = 0.0
    for n in (1, 2, 3, 9, 42, 49, 224, 225):
        for winner in (0, 1, -1):
            for first in (0, 3):
                qs = rng.uniform(-1.0, 1.0, n)
                got, want = vr.targets(qs, winner, first, 1.0, lam), vr.horizon_closed_form(qs, winner, first, lam)
                worst = max(worst, max(abs(a - b) for a, b in zip(got, want)))
                assert all(abs(t) <= 1.0 + 1e-12 for t in got)
    print("lam", lam, "worst |loop - closed form|", worst)
    assert worst <= 1e-12


def test_identity_settings_give_z_bit_for_bit():
    rng = np.random.RandomState(2)
    for trial in range(200):
        n = int(rng.randint(1, 60))
        qs = rng.uniform(-1.0, 1.0, n)
        if trial % 7 == 0:
            qs[rng.randint(n)] = 0.0
        winner, first = int(rng.choice([0, 1, -1])), int(rng.randint(0, 5))
        z = [vr.outcome(winner, first + k) for k in range(n)]
        for r, lam in ((0.0, 0.0), (0.0, 0.5), (0.0, float(rng.rand())), (0.0, 1.0), (1.0, 1.0)):
            got = vr.targets(qs, winner, first, r, lam)
            assert [bits(a) for a in got] == [bits(b) for b in z], (trial, r, lam)
            if winner == -1:
                assert all(math.copysign(1.0, a) == 1.0 and bits(np.float32(a)) == bits(0.0) for a in got)      # a draw keeps +0.0


def test_a_live_setting_differs_from_z():
    qs = [0.2, -0.4, 0.1, 0.3]
    for r, lam in ((0.5, 0.0), (1.0, 0.7), (0.5, 0.9)):
        t = vr.targets(qs, 1, 0, r, lam)
        assert max(abs(a - vr.outcome(1, i)) for i, a in enumerate(t)) > 1e-3


# ---- the product's numpy rule and host route -------------------------------------------------------------------------------------
def test_value_targets_equals_the_restatement_bit_for_bit():
    from selfplay import value_targets
    rng = np.random.RandomState(11)
    for trial in range(300):
        n = int(rng.randint(1, 80))
        qs = rng.uniform(-1.0, 1.0, n)
        winner = int(rng.choice([0, 1, -1]))
        first = 0 if trial % 3 else int(rng.randint(1, 7))
        r, lam = [float(rng.choice([0.0, 0.5, 0.7, 0.9, 1.0, rng.rand()])) for _ in range(2)]
        got = value_targets(list(qs) if trial % 2 else qs, winner, first, r, lam)
        assert got.dtype == np.float64 and got.shape == (n,)
        assert [bits(a) for a in got] == [bits(b) for b in vr.targets(qs, winner, first, r, lam)], (trial, r, lam, first)
    assert value_targets([], 0, 0, 0.5, 0.5).shape == (0,)


CASES = [("gomoku", 5, 5, 2, 25, None), ("connect4", 6, 7, 3, 7, (0, 1)), ("gomoku", 5, 7, 2, 35, (0, 1, 2, 6))]


@pytest.mark.parametrize("game,rows,cols,planes,A,elements", CASES)
@pytest.mark.parametrize("variant", ["plain", "full", "copies", "first_ply"])
def test_host_route_with_values_replaces_only_the_z_column(game, rows, cols, planes, A, elements, variant):
    import train
    from selfplay import surprise_copies, value_targets
    els = elements if elements is not None else tuple(range(8))
    for winner in (0, 1, -1):
        boards, pis, _ = record(rows, cols, planes, A, 13, winner, seed=23 + winner)
        rng = np.random.RandomState(winner + 4)
        qs = rng.uniform(-1.0, 1.0, 13)
        full = copies = None
        first = 0
        if variant == "full":
            full = [bool(x) for x in rng.rand(13) < 0.6]
            full[0], full[1], full[2] = False, True, True
        if variant == "copies":
            kls, coins = rng.gamma(0.4, 1.0, 13), rng.rand(13)
            copies = surprise_copies(kls, coins, 0.5)
            assert min(copies) == 0 and max(copies) >= 2
        if variant == "first_ply":
            first = 3                                              # boards[0] is ply 3: its mover is side 1, and every ply has its group
        values = value_targets(qs, winner, first, 0.5, 0.9)
        data = (boards, None, pis, list(qs), winner, 0 if winner == -1 else 1)
        buf, plain = _ListBuffer(), _ListBuffer()
        train.save_data_to_buffer(_HostGame, buf, data, full=full, elements=elements, copies=copies, first_ply=first, values=values)
        train.save_data_to_buffer(_HostGame, plain, data, full=full, elements=elements, copies=copies, first_ply=first)
        # the tuple list without the option, from the restatements that pin it ...
        if variant == "copies":
            base, cr = sr.game_tuples(game, boards, pis, winner, els, kls, coins, 0.5, None)
            assert cr == copies.tolist()
        elif variant == "first_ply":
            base = vr.game_tuples(game, boards, pis, winner, els, None, first_ply=first)
        else:
            base = er.emit_tuples(game, boards, pis, winner, els, full=full)
        assert same(base, plain)
        # ... and with it: the same states and pis, the z column the ply's target in every tuple of the ply
        t = vr.targets(qs, winner, first, 0.5, 0.9)
        want = vr.game_tuples(game, boards, pis, winner, els, t, first_ply=first, full=full, copies=copies)
        assert same(want, buf) and len(buf) == len(plain)
        assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(buf, plain))
        assert max(abs(a[2] - b[2]) for a, b in zip(buf, plain)) > 1e-3
        # values = the outcome itself is the call without the argument
        zbuf = _ListBuffer()
        train.save_data_to_buffer(_HostGame, zbuf, data, full=full, elements=elements, copies=copies, first_ply=first,
                                  values=value_targets(qs, winner, first, 0.0, 0.5))
        assert same(zbuf, plain)


# ---- the refusals, before any engine exists ----------------------------------------------------------------------------------------
def test_refusals_before_any_engine_exists():
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_value_target, self_play_batch
    assert check_value_target(None) is None
    assert check_value_target(0) == (0.0, 0.0) and check_value_target(0.5) == (0.5, 0.0) and check_value_target(1) == (1.0, 0.0)
    assert check_value_target((0.5, 0.9)) == (0.5, 0.9) and check_value_target([1, 1]) == (1.0, 1.0)
    ev = lambda x: None
    for bad in (-0.1, 1.5, float("nan"), float("inf"), "x", (0.5,), (0.5, 0.5, 0.5), True, (0.5, -0.1), (0.5, 1.5), (0.5, float("nan")), (1.5, 0.5),
                (0.5, True), (None, 0.5)):
        with pytest.raises(ValueError):
            check_value_target(bad)
        with pytest.raises(ValueError):
            SelfPlayRunner("gomoku", ev, 2, 24, size=7, value_target=bad)
        with pytest.raises(ValueError):
            AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, value_target=bad)
        with pytest.raises(ValueError):
            self_play_batch("gomoku", ev, 2, 24, size=7, value_target=bad)
        with pytest.raises(ValueError):
            az_train.collect_data(None, ev, None, 1, 24, value_target=bad)
    for make in (lambda: SelfPlayRunner("gomoku", None, 2, 24, size=7, value_target=0.5),
                 lambda: AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, value_target=0.5),
                 lambda: self_play_batch("gomoku", None, 2, 24, size=7, value_target=0.5),
                 lambda: self_play_batch("gomoku", (ev, None), 2, 24, size=7, value_target=0.5),
                 lambda: az_train.collect_data(None, None, None, 1, 24, value_target=0.5)):
        with pytest.raises(ValueError, match="vanilla"):
            make()
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, use_graph=True, leaves_per_step=2, value_target=0.5)
    with pytest.raises(ValueError, match="leaves_per_step"):
        self_play_batch("gomoku", ev, 2, 24, size=7, leaves_per_step=2, value_target=0.5)
    for make in (lambda: SelfPlayRunner("gomoku", ev, 2, 24, size=7, gumbel_root=(4, 50.0, 1.0), value_target=0.5),
                 lambda: AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, gumbel_root=(4, 50.0, 1.0), value_target=0.5),
                 lambda: self_play_batch("gomoku", ev, 2, 24, size=7, gumbel_root=(4, 50.0, 1.0), value_target=0.5)):
        with pytest.raises(ValueError, match="gumbel_root"):
            make()
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, ev, None, 1, 24, batched=False, value_target=0.5)


def test_the_symbols_are_declared():
    """The three calls are in the public header and in the package's symbol list (the library side is tests/test_abi.py's comparison)."""
    import os
    import azk
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "azk.h")).read()
    for name in ("azk_set_value_target", "azk_clear_value_target", "azk_get_value_record"):
        assert name in azk.SYMBOLS and ("int32_t " + name + "(") in header
