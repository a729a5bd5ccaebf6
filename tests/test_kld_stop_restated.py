"""The restatement of adaptive search budgets (tests/kld_stop_restated.py) checked on the CPU: a threshold that never fires leaves the pinned
search of forced_playouts_restated (k = 0) bit for bit, the arming arithmetic, what selfplay.check_kld_stop refuses before any engine exists,
and the preconditions of the GPU cases (tests/test_gpu_kld_stop.py)."""
import math

import pytest

import forced_playouts_restated as fr
import kld_stop_restated as kr


@pytest.mark.parametrize("name", kr.SMALL)
def test_a_threshold_that_never_fires_is_the_plain_search(name):
    og, slots, res = kr.small_results(name, kr.NEVER)
    for g, (s, r) in enumerate(zip(slots, res)):
        root = fr.RNode(None, None, s["to_move"], s["move_count"])
        fr.mcts(og, root, og.board_from_cells(s["cells"], s["to_move"]), kr.SMALL_T, fr.hash_evaluator(og), s["noise"])
        assert fr.same_tree(r["tree"], fr.export(root)), (name, g)
        assert fr.same_tree(r["tree"], s["plain"]["tree"]), (name, g)            # ... which is forced_playouts_restated's own k = 0 search
        assert (r["ended"], r["run"], r["left"], r["ckpt"]) == ("allowance", kr.SMALL_T, 0, kr.SMALL_T // kr.SMALL_I)
        assert len(r["rates"]) == r["ckpt"] - 2                                  # the first checkpoint has no snapshot, the last is not judged


def test_the_tree_at_a_checkpoint_is_the_plain_search_of_run_simulations():
    og, slots, res = kr.small_results("gomoku7", 1e-2)
    for g, (s, r) in enumerate(zip(slots, res)):
        assert r["ended"] == "early" and r["run"] == r["ckpt"] * kr.SMALL_I and r["left"] == kr.SMALL_T - r["run"]
        root = fr.RNode(None, None, s["to_move"], s["move_count"])
        fr.mcts(og, root, og.board_from_cells(s["cells"], s["to_move"]), r["run"], fr.hash_evaluator(og), s["noise"])
        assert fr.same_tree(r["tree"], fr.export(root)), g


@pytest.mark.parametrize("T,interval,want", [(5, 8, [5]), (8, 8, [8]), (9, 8, [8, 1]), (64, 8, [8] * 8), (20, 8, [8, 8, 4]), (1, 1, [1]), (3, 1, [1, 1, 1])])
def test_arming_arithmetic(T, interval, want):
    seg, left, run = kr.arm(T, interval)
    segs = [seg]
    assert seg == min(interval, T) and left == T - seg and run == seg
    while left:
        seg = min(interval, left)
        left -= seg
        run += seg
        segs.append(seg)
    assert segs == want and run == T


def test_min_sims_holds_a_search_back():
    og, slots = fr.small_case("gomoku7", kr.SMALL_T)
    a = kr.searched(og, slots[1], kr.SMALL_T, kr.SMALL_I, 1e-2)
    b = kr.searched(og, slots[1], kr.SMALL_T, kr.SMALL_I, 1e-2, min_sims=24)
    assert (a["ckpt"], a["run"]) == (2, 16) and b["run"] >= 24 and b["ckpt"] > a["ckpt"]
    assert len(b["rates"]) == b["ckpt"] - 2                                      # checkpoint 2 (run = 16 < 24) was not judged


def test_gain_is_zero_on_equal_distributions_and_positive_otherwise():
    assert kr.gain([1, 2, 3], [2, 4, 6])[0] == 0.0
    g, mag = kr.gain([4, 0, 4], [5, 6, 5])
    assert g > 0.0 and mag >= g and math.isclose(g, math.log(1.6), rel_tol=1e-15)   # two terms of 1/2 * log((1/2) / (5/16))
    # 130 children: lanes 0 and 1 hold three terms each, the butterfly adds all of them
    old, new = [1] * 130, [1 + (i % 3) for i in range(130)]
    want = sum((1 / 130) * math.log((1 / 130) / (n / sum(new))) for n in new)
    assert math.isclose(kr.gain(old, new)[0], want, rel_tol=1e-12)


def test_check_kld_stop():
    from selfplay import SelfPlayRunner, AsyncSelfPlayRunner, check_kld_stop, self_play_batch
    import train as az_train
    ev = lambda x: None  # noqa: E731
    assert check_kld_stop(None, 64) is None
    assert check_kld_stop((8, 1e-3), 64) == (8, 1e-3, 0) and check_kld_stop((64, 1e-3, 16), (32, 64)) == (64, 1e-3, 16)
    for bad in (5, (8,), (8, 1e-3, 0, 0), (0, 1e-3), (65, 1e-3), (8.5, 1e-3), (True, 1e-3), (8, 0.0), (8, -1e-3), (8, float("nan")), (8, float("inf")),
                (8, 1e-3, -1), (8, 1e-3, 1.5), ("8", "x")):
        with pytest.raises(ValueError, match="kld_stop"):
            check_kld_stop(bad, 64)
    with pytest.raises(ValueError, match="vanilla"):
        check_kld_stop((8, 1e-3), 64, evaluator=None)
    with pytest.raises(ValueError, match="vanilla"):
        check_kld_stop((8, 1e-3), 64, evaluator=(ev, None))
    with pytest.raises(ValueError, match="leaves_per_step"):
        check_kld_stop((8, 1e-3), 64, leaves_per_step=2)
    with pytest.raises(ValueError, match="gumbel_root"):
        check_kld_stop((8, 1e-3), 64, gumbel_root=(4, 50.0, 1.0))
    # ... and every entry point raises before an engine exists (no GPU here)
    with pytest.raises(ValueError, match="kld_stop"):
        self_play_batch("gomoku", ev, 2, 24, size=7, kld_stop=(25, 1e-3))
    with pytest.raises(ValueError, match="gumbel_root"):
        self_play_batch("gomoku", ev, 2, 24, size=7, kld_stop=(8, 1e-3), gumbel_root=(4, 50.0, 1.0))
    with pytest.raises(ValueError, match="kld_stop"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, kld_stop=(8, 0.0))
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, use_graph=True, leaves_per_step=2, kld_stop=(8, 1e-3))
    with pytest.raises(ValueError, match="kld_stop"):
        AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, kld_stop=(0, 1e-3))
    with pytest.raises(ValueError, match="vanilla"):
        AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, kld_stop=(8, 1e-3))
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 24, batched=False, kld_stop=(8, 1e-3))


def every_result():
    for name in kr.SMALL:
        for thr in kr.THRESHOLDS:
            for g, r in enumerate(kr.small_results(name, thr)[2]):
                yield (name, thr, g), thr, r, kr.SMALL_T // kr.SMALL_I
    for i in range(3):
        for thr in kr.THRESHOLDS:
            yield (fr.WIDE_STONES[i], thr), thr, kr.wide_results(i, thr)[2], kr.WIDE_T // kr.WIDE_I


def test_preconditions_of_the_gpu_cases():
    """Every outcome occurs - a search that ends at the first judged checkpoint, at every later one, and one that runs its allowance - and no
    judged rate lies within 1e-6 (relative) of its threshold: the device's log differs from this one by a few ulp, which cannot flip a decision."""
    ended = {}
    for tag, thr, r, n_ckpt in every_result():
        for x in r["rates"]:
            assert abs(x - thr) > 1e-6 * thr, (tag, x)
            assert 1e-5 < x < 1e-1, (tag, x)                                       # from a few 1e-2 down to a few 1e-4
        ended.setdefault((n_ckpt, r["ended"]), set()).add(r["ckpt"])
        assert r["ckpt"] == n_ckpt if r["ended"] == "allowance" else 2 <= r["ckpt"] < n_ckpt, tag
    # small cases: 8 checkpoints, judged at 2 .. 7; wide roots: 6 checkpoints, judged at 2 .. 5
    assert ended[(8, "early")] == set(range(2, 8)) and ended[(8, "allowance")] == {8}
    assert ended[(6, "early")] >= {2, 3, 5} and ended[(6, "allowance")] == {6}
    # the searches the issue names
    assert kr.small_results("gomoku7", 1e-2)[2][1]["ckpt"] == 2 and kr.wide_results(2, 1e-2)[2]["ckpt"] == 2
    assert kr.small_results("tictactoe", 1e-3)[2][0]["ended"] == "allowance" and kr.wide_results(1, 4e-3)[2]["ended"] == "allowance"
    # the wide roots have the child counts that cover one, two and three strides of the 64 lanes
    assert [len(kr.wide_results(i, 1e-2)[2]["cells"]) for i in range(3)] == [48, 96, 192]


def test_precondition_no_search_of_the_never_games_has_a_zero_rate():
    """A rate of exactly 0 is below every positive threshold: "a threshold that never fires" needs games without one."""
    games = kr.never_games()
    assert len(games) == kr.G and len({tuple(g["cells"]) for g in games}) > 1
    for g in games:
        assert len(g["cells"]) == kr.NEVER_MOVES                                 # no game ended: every slot plays every move
        for ended, smallest in g["outcomes"]:
            assert ended == "allowance" and smallest > 1e-6


def test_stats_of():
    res = kr.small_results("gomoku7", 1e-2)[2]
    st = kr.stats_of(res)
    assert st["ended_early"] + st["ran_allowance"] == len(res) and st["judged"] == sum(r["ckpt"] - 1 for r in res)
    assert st["sims_unrun"] == sum(kr.SMALL_T - r["run"] for r in res)
