"""Move temperature (azk_set_move_temperature), the CPU half: the plain-Python restatement of tests/move_temperature_restated.py
against the oracle's restatement of Node.sample_child, the preconditions that make a pass of tests/test_gpu_move_temperature.py mean something,
the table builder (selfplay.move_temperature_setting) and the refusals of selfplay.check_move_temperature.  No GPU."""
import math
import sys

import numpy as np
import pytest

import move_temperature_restated as mt
from forced_playouts_restated import pi_of
from oracle import az_oracle as ao

N_ROW = (1.0, 0, None)                                             # tau 1: the row w[n] = n, no offset, no cutoff


# ---- 1. the restatement is the reference's sampler where the weights are the visits ----------------------------------------------------------
@pytest.mark.parametrize("name", mt.CASES)
def test_the_visits_row_is_the_oracles_sample_child(name):
    og, slots = mt.case(name)
    a_of = mt.action_of_game(og)
    row = mt.expected_row(1.0, mt.N_SIMS)
    assert row == [float(n) for n in range(mt.N_SIMS + 1)]
    us, cells, stats = mt.expected(name, N_ROW)
    for g, s in enumerate(slots):
        ch = s["children"]
        pi = pi_of(og, ch["cell"], [int(n) for n in ch["visit"]])
        for u, cell in zip(us[g], cells[g]):
            act = ao.sample_action(pi, u)                          # Node.sample_child: legacy np.random.choice(p=pi) on the uniform u
            want = next(int(c) for c in ch["cell"] if a_of(int(c)) == act)
            assert cell == want, (name, g, u)
    assert stats[0] == 6 * mt.G and stats[2] == 0 and stats[3] == 0


def test_greedy_is_the_first_most_visited_child():
    og, slots = mt.case("gomoku7")
    a_of = mt.action_of_game(og)
    for s in slots:
        ch = s["children"]
        visits = [int(n) for n in ch["visit"]]
        b = visits.index(max(visits))
        for row, u in ((None, 0.3), (mt.expected_row(4.0, mt.N_SIMS), None)):
            assert mt.choose(ch, a_of, row, 0, None, u, og.action_dim) == (int(ch["cell"][b]), [0, 0, 0, 0])


# ---- 2. the preconditions of the GPU cases -------------------------------------------------------------------------------------------------
def test_a_sharp_row_plays_other_cells_than_the_visits_row():
    """Some (slot, u) of every case but the short one: tau 0.25 and tau 1 play different cells on the SAME uniform - an engine that kept sampling
    in proportion to the visits fails the GPU test's tau 0.25 cases."""
    for name in mt.SMALL + mt.WIDE:
        og, slots = mt.case(name)
        a_of = mt.action_of_game(og)
        us = mt.expected(name, N_ROW)[0]
        differ = 0
        for g, s in enumerate(slots):
            for u in us[g]:
                sharp = mt.choose(s["children"], a_of, mt.expected_row(0.25, mt.N_SIMS), 0, None, u, og.action_dim)[0]
                differ += sharp != mt.choose(s["children"], a_of, mt.expected_row(1.0, mt.N_SIMS), 0, None, u, og.action_dim)[0]
        assert differ >= 1, name


def test_the_cutoff_cuts_a_child_and_keeps_another_beside_the_most_visited():
    for name in mt.SMALL + mt.WIDE:
        og, slots = mt.case(name)
        hits = 0
        for s in slots:
            b = mt.first_most_visited([int(n) for n in s["children"]["visit"]])
            for cutoff in (0.1, 0.0):
                w, cut = mt.weights_of(s["children"], mt.expected_row(1.0, mt.N_SIMS), 0, cutoff)
                hits += cut >= 1 and any(x > 0.0 for i, x in enumerate(w) if i != b)
        assert hits >= 1, name


def test_the_offset_makes_a_fallback_in_one_case_and_none_in_the_others():
    for name in mt.CASES:
        for tau in mt.TAUS:
            fallbacks = mt.expected(name, (tau, 2, None))[2][3]
            assert fallbacks == (6 * mt.G if name in mt.SHORT else 0), (name, tau)
            assert mt.expected(name, (tau, 0, None))[2][3] == 0, (name, tau)
    og, slots = mt.case(mt.SHORT[0])
    assert all(max(s["children"]["visit"]) <= 2 for s in slots)


def test_interior_uniforms_sit_on_a_step_of_the_cdf():
    """Every case has slots whose fifth and sixth uniforms equal a cdf[k] / cdf[-1]: side='right' sends them to the next weighted action."""
    for name in mt.SMALL + mt.WIDE:
        og, slots = mt.case(name)
        a_of = mt.action_of_game(og)
        on_step = 0
        for setting in mt.SETTINGS:
            tau, offset, cutoff = setting
            us = mt.expected(name, setting)[0]
            for g, s in enumerate(slots):
                w, _ = mt.weights_of(s["children"], mt.expected_row(tau, mt.N_SIMS), offset, cutoff)
                S, cdf = mt.cdf_of(s["children"], a_of, w, og.action_dim)
                steps = {x / cdf[-1] for x in cdf}
                on_step += us[g][4] in steps and us[g][5] in steps
        assert on_step >= len(mt.SETTINGS), name


# ---- 3. the table builder ------------------------------------------------------------------------------------------------------------------
def test_rows_are_pow_of_the_visit_count():
    from selfplay import move_temperature_setting
    for tau in (0.25, 0.5, 1.0, 4.0, 0.75):
        rows, w, offset, cutoff = move_temperature_setting(tau, 24, 49)
        assert rows.dtype == np.int32 and rows.tolist() == [0] and w.dtype == np.float64 and w.shape == (1, 25)
        assert w[0].tolist() == mt.expected_row(tau, 24) and w[0, 0] == 0.0
        assert (offset, cutoff) == (0, -1.0)
        if tau in mt.EXACT_ROWS:
            assert w[0].tolist() == [mt.EXACT_ROWS[tau](n) for n in range(25)]
    assert move_temperature_setting(1.0, 24, 49, visit_offset=3, value_cutoff=0.25)[2:] == (3, 0.25)


def test_schedules_equal_their_formulas():
    from selfplay import move_temperature_setting
    rows, w, _, _ = move_temperature_setting(("halflife", 1.0, 10, 0.1), 16, 49)
    assert rows.tolist() == list(range(49)) and w.shape == (49, 17)
    for p in (0, 1, 10, 48):
        tau = mt.halflife(p, 1.0, 10, 0.1)
        assert tau == 0.1 + (1.0 - 0.1) * 0.5 ** (p / 10) and w[p].tolist() == mt.expected_row(tau, 16)
    assert mt.halflife(10, 1.0, 10, 0.1) == 0.55
    rows, w, _, _ = move_temperature_setting(("linear", 1.0, 4, 0.5), 16, 9)
    assert [mt.linear(p, 1.0, 4, 0.5) for p in range(9)] == [1.0, 0.875, 0.75, 0.625, 0.5, 0.5, 0.5, 0.5, 0.5]
    assert rows.tolist() == [0, 1, 2, 3, 4, 4, 4, 4, 4] and w.shape == (5, 17)             # equal values share one row
    assert w[3].tolist() == mt.expected_row(0.625, 16)
    rows, w, _, _ = move_temperature_setting(("linear", 1.0, 4), 16, 9)                      # t_final left out: 0, greedy from decay_plies on
    assert rows.tolist() == [0, 1, 2, 3, -1, -1, -1, -1, -1]
    rows, w, _, _ = move_temperature_setting(("until", 0.5, 3), 16, 9)
    assert rows.tolist() == [0, 0, 0, -1] and w[0].tolist() == mt.expected_row(0.5, 16)
    rows, w, _, _ = move_temperature_setting(("until", 1.0, 1 << 30), 16, 42)                # "every ply": no table of 2^30 entries
    assert rows.tolist() == [0] * 42 + [-1]


def test_lists_share_rows_and_zero_is_greedy():
    from selfplay import move_temperature_setting
    rows, w, _, _ = move_temperature_setting([4.0, 0.25, 0.0, 4.0, 0.25], 8, 49)
    assert rows.tolist() == [0, 1, -1, 0, 1] and w.shape == (2, 9)
    assert w[0].tolist() == mt.expected_row(4.0, 8) and w[1].tolist() == mt.expected_row(0.25, 8)


def test_bad_schedules_and_overflow_are_refused():
    from selfplay import move_temperature_setting
    for bad in (-1.0, float("nan"), float("inf"), True, "warm", ("until", 1.0), ("halflife", 1.0, 0.0), ("linear", 1.0, -2), ("cosine", 1.0, 3), [],
                [1.0, -0.5], 0.0, [0.0, 0.0], None):
        with pytest.raises(ValueError, match="move_temperature"):
            move_temperature_setting(bad, 24, 49)
    for kw in (dict(visit_offset=-1), dict(visit_offset=1.5), dict(value_cutoff=float("nan"))):
        with pytest.raises(ValueError, match="move_temperature"):
            move_temperature_setting(1.0, 24, 49, **kw)
    # 800 ** (1 / tau) against DBL_MAX / (1 * 801): the message names the smallest admissible tau, which passes, and a smaller one does not
    with pytest.raises(ValueError, match="smallest admissible tau") as info:
        move_temperature_setting(0.005, 800, 225)
    tau_min = math.log(800) / math.log(sys.float_info.max / 801)
    assert "%.6g" % tau_min in str(info.value)
    assert math.isfinite(move_temperature_setting(tau_min * 1.0001, 800, 225)[1].max())
    with pytest.raises(ValueError, match="smallest admissible tau"):
        move_temperature_setting(tau_min * 0.999, 800, 225)
    with pytest.raises(ValueError, match="smallest admissible tau"):
        move_temperature_setting(("halflife", 1.0, 10), 800, 225)                         # t_final 0: tau(224) = 2 ** -22.4


# ---- 4. check_move_temperature -------------------------------------------------------------------------------------------------------------
def test_check_move_temperature():
    from selfplay import check_move_temperature
    assert check_move_temperature(None, 24, "gomoku", 7) is None
    rows, w, offset, cutoff = check_move_temperature(0.5, 24, "gomoku", 7)
    assert rows.tolist() == [0] and w.shape == (1, 25) and (offset, cutoff) == (0, -1.0)
    rows, w, offset, cutoff = check_move_temperature(dict(tau=("halflife", 1.0, 10, 0.1), visit_offset=1, value_cutoff=0.2), (16, 24), "connect4")
    assert rows.tolist() == list(range(42)) and w.shape == (42, 25) and (offset, cutoff) == (1, 0.2)      # a pair: the larger budget's columns
    assert check_move_temperature(1.0, 24, "gomoku", (5, 3), tree_reuse=2) is not None                  # top-up is bounded
    with pytest.raises(ValueError, match="gumbel_root"):
        check_move_temperature(1.0, 24, "gomoku", 7, gumbel_root=(4, 50.0, 1.0))
    with pytest.raises(ValueError, match="tree_reuse = 1"):
        check_move_temperature(1.0, 24, "gomoku", 7, tree_reuse=1)
    for bad in (dict(visit_offset=1), dict(tau=1.0, offset=1), dict(tau=-1.0), "warm"):
        with pytest.raises(ValueError, match="move_temperature"):
            check_move_temperature(bad, 24, "gomoku", 7)


def test_runners_refuse_before_an_engine_exists():
    """The refusals fire in the constructors' checks, which need no GPU."""
    import arena
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, self_play_batch
    ev = lambda x: None                                            # noqa: E731  (never called)
    with pytest.raises(ValueError, match="tree_reuse = 1"):
        SelfPlayRunner("gomoku", ev, 8, 16, size=7, tree_reuse=1, move_temperature=1.0)
    with pytest.raises(ValueError, match="tree_reuse = 1"):
        AsyncSelfPlayRunner("gomoku", ev, 8, 16, size=7, reroot=1, move_temperature=1.0)
    with pytest.raises(ValueError, match="gumbel_root"):
        self_play_batch("gomoku", ev, 8, 16, size=7, gumbel_root=(4, 50.0, 1.0), move_temperature=1.0)
    with pytest.raises(ValueError, match="move_temperature"):
        arena.compare("gomoku", ev, ev, 16, 16, 4, False, False, size=7, move_temperature=-1.0)
