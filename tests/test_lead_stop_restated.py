"""The restatement of the lead rule (tests/lead_stop_restated.py) checked on the CPU: a factor that cannot fire leaves the
pinned plain search bit for bit, the tree where a search ends is the plain search of `run` simulations, the theorem at factor 1 (the first
most-visited child is the full search's), the (max, second) pair, both rules together, what selfplay.check_lead_stop refuses before any engine
exists, and the preconditions of the GPU cases (tests/test_gpu_lead_stop.py)."""
import pytest

import forced_playouts_restated as fr
import kld_stop_restated as kr
import lead_stop_restated as lr


def every_result(factors=lr.FACTORS):
    """(tag, factor, result, plain key, plain index) over section 31's case set plus the empty board."""
    for name in lr.SMALL + ("gomoku7+empty",):
        for f in factors:
            for g, r in enumerate(lr.small_results(name, f)[2]):
                yield (name, f, g), f, r, name, g
    for i in range(3):
        for f in factors:
            yield ("wide", fr.WIDE_STONES[i], f), f, lr.wide_results(i, f)[2], "wide", i


def allowance(key):
    return lr.WIDE_T if key == "wide" else lr.SMALL_T


@pytest.mark.parametrize("name", lr.SMALL)
def test_a_factor_that_cannot_fire_is_the_plain_search(name):
    og, slots, res = lr.small_results(name, lr.NEVER)
    for g, (s, r) in enumerate(zip(slots, res)):
        for n1, n2, left in r["leads"]:
            assert lr.NEVER * float(n1 - n2) <= float(left), (name, g)            # "cannot fire", at every judged checkpoint
        assert fr.same_tree(r["tree"], lr.plain_visits(name, g, lr.SMALL_T)[1]), (name, g)
        assert fr.same_tree(r["tree"], s["plain"]["tree"]), (name, g)            # ... which is forced_playouts_restated's own k = 0 search
        assert (r["ended"], r["run"], r["left"], r["ckpt"]) == ("allowance", lr.SMALL_T, 0, lr.SMALL_T // lr.SMALL_I)
        assert len(r["leads"]) == r["ckpt"] - 1                                  # every checkpoint but the last is judged: the rule needs no snapshot


def test_the_tree_where_a_search_ends_is_the_plain_search_of_run_simulations():
    seen = 0
    for tag, f, r, key, i in every_result():
        if r["ended"] in ("early", "forced"):
            interval = lr.WIDE_I if key == "wide" else lr.SMALL_I
            assert r["run"] == r["ckpt"] * interval and r["left"] == allowance(key) - r["run"], tag
            assert fr.same_tree(r["tree"], lr.plain_visits(key, i, r["run"])[1]), tag
            seen += 1
    assert seen > 40


def test_the_theorem_at_factor_one():
    """Every pinned search that ends early at f = 1: the plain search run to T has the same first most-visited root child, and holds it
    as a strict maximum (each simulation adds one visit to one child, so no child can make up a lead larger than the simulations left)."""
    seen = 0
    for tag, f, r, key, i in every_result((1.0,)):
        if r["ended"] != "early":
            continue
        seen += 1
        n1, n2, left = r["lead"]
        assert left < n1 - n2, tag
        stopped = r["visits"][-1]
        assert stopped.count(max(stopped)) == 1, tag                             # the holder of N1 is unique
        full = lr.plain_visits(key, i, allowance(key))[0]
        assert lr.first_max(full) == lr.first_max(stopped), tag
        assert full.count(max(full)) == 1, tag                                   # ... and stays the strict maximum
    assert seen >= 20


def test_the_pair_counts_multiplicity_and_crosses_the_64_child_trips():
    assert lr.lead_pair([5]) == (5, 0) and lr.lead_pair([3, 3]) == (3, 3) and lr.lead_pair([0, 0, 0]) == (0, 0)
    assert lr.lead_pair([1, 7, 2, 7, 3]) == (7, 7) and lr.lead_pair([4, 9, 2]) == (9, 4)
    for hi, lo in ((0, 64), (64, 0), (130, 5), (5, 130), (70, 134), (191, 127), (3, 67)):      # same lane / different lanes, across trips
        n = [1] * 192
        n[hi], n[lo] = 50, 20
        assert lr.lead_pair(n) == (50, 20), (hi, lo)
    n = [0] * 130
    n[129] = n[1] = 6                                                            # lane 1 holds both: the tie survives the lane's own fold
    assert lr.lead_pair(n) == (6, 6)
    assert lr.fires(7, 1.0, 10, 2) and not lr.fires(8, 1.0, 10, 2) and lr.fires(8, 1.33, 10, 2) and not lr.fires(0, 1.0, 3, 3)


def test_min_sims_holds_a_search_back():
    """Held back ONLY by min_sims: without it the search ends earlier; with it every earlier checkpoint is passed unjudged and the search ends
    at its first judged one."""
    og, slots, free = lr.small_results("gomoku7", 4.0)
    _, _, held = lr.small_results("gomoku7", 4.0, lr.HELD_MIN_SIMS)
    first = lr.HELD_MIN_SIMS // lr.SMALL_I
    only = [g for g in range(lr.G) if free[g]["run"] < lr.HELD_MIN_SIMS]
    assert len(only) >= 4
    for g in range(lr.G):
        assert held[g]["run"] >= lr.HELD_MIN_SIMS and len(held[g]["leads"]) == held[g]["ckpt"] - (first - 1) - (held[g]["ended"] == "allowance"), g
    at_first = [g for g in only if held[g]["ended"] == "early" and held[g]["ckpt"] == first and len(held[g]["leads"]) == 1]
    assert len(at_first) >= 3, at_first                                          # (a lead can shrink again: not every one of `only` still fires there)
    assert any(len(held[g]["leads"]) > 1 for g in range(lr.G))                   # ... and one that goes on past its first judged checkpoint


def test_preconditions_of_the_gpu_cases():
    """Every kind of search occurs among the cases, so the GPU tests cannot pass vacuously."""
    kinds = set()
    for tag, f, r, key, i in every_result():
        if r["ended"] == "early":
            kinds.add("first judged" if len(r["leads"]) == 1 else "later")
        kinds.add(r["ended"])
        if any(n1 == n2 for n1, n2, _ in r["leads"]) and len(r["visits"][0]) > 1:
            kinds.add("tie")
    for g, r in enumerate(lr.small_results("gomoku7", 4.0, lr.HELD_MIN_SIMS)[2]):
        if r["ended"] == "early" and len(r["leads"]) == 1:
            kinds.add("first judged")
    assert kinds >= {"first judged", "later", "early", "allowance", "forced", "tie"}, kinds
    # the single-child root: Gomoku's empty board, over at its first checkpoint whatever the factor
    for f in lr.FACTORS:
        r = lr.small_results("gomoku7+empty", f)[2][0]
        assert (r["ended"], r["ckpt"], r["run"], r["lead"]) == ("forced", 1, lr.SMALL_I, (lr.SMALL_I - 1, 0, lr.SMALL_T - lr.SMALL_I))
    # the wide roots have the child counts that cover one, two and three trips of the 64 lanes, and at 96 and 192 the maximum and the
    # second maximum sit in different trips at a judged checkpoint
    assert [len(lr.wide_results(i, 1.0)[2]["cells"]) for i in range(3)] == [48, 96, 192]
    for i in (1, 2):
        r = lr.wide_results(i, 1.0)[2]
        apart = 0
        for v in r["visits"][:len(r["leads"])]:
            top = sorted(range(len(v)), key=lambda j: (-v[j], j))
            if v[top[1]] > v[top[2]]:                                            # (the second is one child, not a tie of several)
                apart += top[0] // 64 != top[1] // 64
        assert apart >= 1, i
        assert r["ended"] == "early"


def same_search(a, b):
    return fr.same_tree(a["tree"], b["tree"]) and (a["run"], a["ckpt"], a["left"]) == (b["run"], b["ckpt"], b["left"])


@pytest.mark.parametrize("name", lr.SMALL)
def test_both_rules_together(name):
    # a min_gain that never fires: the lead-only searches
    for f in lr.FACTORS:
        for g, (a, b) in enumerate(zip(lr.small_results(name, f, 0, kr.NEVER)[2], lr.small_results(name, f)[2])):
            assert same_search(a, b) and a["ended"] == b["ended"] and a["leads"] == b["leads"], (name, f, g)
    # a factor that never fires: the KLD-only searches of tests/kld_stop_restated.py
    for thr in kr.THRESHOLDS:
        for g, (a, b) in enumerate(zip(lr.small_results(name, lr.NEVER, 0, thr)[2], kr.small_results(name, thr)[2])):
            assert same_search(a, b) and a["rates"] == b["rates"] and a["ended"] == {"early": "kld", "allowance": "allowance"}[b["ended"]], (name, thr, g)
    # ... and where both can fire each ends some searches: the lead rule is judged first
    res = lr.small_results(name, lr.BOTH_FACTOR, 0, lr.BOTH_GAIN)[2]
    assert {"early", "kld"} <= {r["ended"] for r in res}, [r["ended"] for r in res]


def test_stats_of():
    res = lr.small_results("gomoku7+empty", 1.0)[2]
    st = lr.stats_of(res)
    assert st["ended_early"] + st["forced"] + st["ran_allowance"] == len(res) and st["forced"] == 1
    assert st["judged"] == sum(r["ckpt"] - (r["ended"] == "allowance") for r in res)
    assert st["sims_unrun"] == sum(lr.SMALL_T - r["run"] for r in res if r["ended"] == "early")


def test_check_lead_stop():
    from selfplay import SelfPlayRunner, AsyncSelfPlayRunner, check_lead_stop, self_play_batch
    import arena
    import train as az_train
    ev = lambda x: None  # noqa: E731
    assert check_lead_stop(None, 64) is None
    assert check_lead_stop((8, 1.0), 64) == (8, 1.0, 0) and check_lead_stop((64, 1.33, 16), (32, 64)) == (64, 1.33, 16)
    assert check_lead_stop((8, 2), 64, kld_stop=(8, 1e-3, 0)) == (8, 2.0, 0)
    for bad in (5, (8,), (8, 1.0, 0, 0), (0, 1.0), (65, 1.0), (8.5, 1.0), (True, 1.0), (8, 0.0), (8, -1.0), (8, float("nan")), (8, float("inf")),
                (8, 1.0, -1), (8, 1.0, 1.5), ("8", "x")):
        with pytest.raises(ValueError, match="lead_stop"):
            check_lead_stop(bad, 64)
    with pytest.raises(ValueError, match="vanilla"):
        check_lead_stop((8, 1.0), 64, evaluator=None)
    with pytest.raises(ValueError, match="vanilla"):
        check_lead_stop((8, 1.0), 64, evaluator=(ev, None))
    with pytest.raises(ValueError, match="leaves_per_step"):
        check_lead_stop((8, 1.0), 64, leaves_per_step=2)
    with pytest.raises(ValueError, match="gumbel_root"):
        check_lead_stop((8, 1.0), 64, gumbel_root=(4, 50.0, 1.0))
    with pytest.raises(ValueError, match="share one interval"):
        check_lead_stop((8, 1.0), 64, kld_stop=(16, 1e-3, 0))
    # ... and every entry point raises before an engine exists (no GPU here)
    with pytest.raises(ValueError, match="lead_stop"):
        self_play_batch("gomoku", ev, 2, 24, size=7, lead_stop=(25, 1.0))
    with pytest.raises(ValueError, match="gumbel_root"):
        self_play_batch("gomoku", ev, 2, 24, size=7, lead_stop=(8, 1.0), gumbel_root=(4, 50.0, 1.0))
    with pytest.raises(ValueError, match="share one interval"):
        self_play_batch("gomoku", ev, 2, 24, size=7, lead_stop=(8, 1.0), kld_stop=(12, 1e-3))
    with pytest.raises(ValueError, match="lead_stop"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, lead_stop=(8, 0.0))
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, use_graph=True, leaves_per_step=2, lead_stop=(8, 1.0))
    with pytest.raises(ValueError, match="share one interval"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, lead_stop=(8, 1.0), kld_stop=(4, 1e-3))
    with pytest.raises(ValueError, match="lead_stop"):
        AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, lead_stop=(0, 1.0))
    with pytest.raises(ValueError, match="vanilla"):
        AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, lead_stop=(8, 1.0))
    with pytest.raises(ValueError, match="share one interval"):
        AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, lead_stop=(8, 1.0), kld_stop=(4, 1e-3))
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 24, batched=False, lead_stop=(8, 1.0))
    with pytest.raises(ValueError, match="vanilla"):
        arena.compete_batch("gomoku", ev, None, 2, 24, 24, size=7, lead_stop=(8, 1.0))
    with pytest.raises(ValueError, match="lead_stop"):
        arena.compete_batch("gomoku", ev, ev, 2, 16, 24, size=7, lead_stop=(25, 1.0))
    with pytest.raises(ValueError, match="vanilla"):
        arena.compare("gomoku", ev, None, 24, 24, 4, False, False, size=7, lead_stop=(8, 1.0))
    with pytest.raises(ValueError, match="lead_stop"):
        arena.compare("gomoku", ev, ev, 24, 24, 4, False, False, size=7, lead_stop=(8, -1.0))
