"""Adaptive search budgets (azk_set_kld_stop) against the plain-Python restatement of tests/kld_stop_restated.py: whole trees
at the end of the search bit for bit through eager lock-step stepping, the simulations run, pi and the counters; the device's rate at a
checkpoint against float64 under a derived bound; a threshold that never fires and clear_kld_stop against an engine without the option; the
asynchronous movers against the lock-step runner slot for slot; stale columns; the refusals.  The positions and thresholds are those whose
preconditions tests/test_kld_stop_restated.py asserts on the CPU."""
import numpy as np
import pytest

import forced_playouts_restated as fr
import kld_stop_restated as kr
from fixture_eval import fixture_logits_value

gpu = pytest.mark.gpu
G = kr.G
SEED, MOVES, N_SIMS, INTERVAL, GAIN = 3, 10, 32, 8, 4e-3


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_for(name, n_sims, **kw):
    import azk
    kind, size = fr.GAMES[name] if name in fr.GAMES else ("gomoku", 15)
    return azk.Engine(kind, G, n_sims, size=size, **kw)


def load(eng, slots):
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
    return torch.from_numpy(np.stack([s["noise"] for s in slots])).to(eng.device)


def assert_is_the_restatement(eng, results, tag):
    sims = eng.search_sims().cpu().numpy()
    pi = eng.root_stats()[0].cpu().numpy()
    for g, r in enumerate(results):
        assert fr.same_tree(eng.export_tree(g), r["tree"]), tag + (g,)
        assert int(sims[g]) == r["run"], tag + (g, int(sims[g]), r["run"])
        assert pi[g].tobytes() == r["pi"].tobytes(), tag + (g,)


# ---- 1. whole trees, search_sims, pi and the counters -----------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("thr", kr.THRESHOLDS)
@pytest.mark.parametrize("name", kr.SMALL)
def test_small_games_are_the_restatement(name, thr):
    og, slots, results = kr.small_results(name, thr)
    eng = engine_for(name, kr.SMALL_T)
    eng.set_kld_stop(kr.SMALL_I, thr)
    noise = load(eng, slots)
    eng.search_budget(evaluator(eng.action_dim), kr.SMALL_T, noise, per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, results, (name, thr))
    assert eng.kld_stats() == kr.stats_of(results)
    assert eng.kld_checkpoint() == 0 and eng.kld_stats() == kr.stats_of(results)       # a search that is over is neither judged nor counted again


@gpu
@pytest.mark.parametrize("thr", kr.THRESHOLDS)
@pytest.mark.parametrize("i", range(3))
def test_wide_roots_are_the_restatement(i, thr):
    """15 x 15 with 48 / 96 / 192 root children: one, two and three strides of the wave's 64 lanes."""
    og, s, r = kr.wide_results(i, thr)
    eng = engine_for("gomoku15", kr.WIDE_T)
    eng.set_kld_stop(kr.WIDE_I, thr)
    noise = load(eng, [s] * G)
    eng.search_budget(evaluator(eng.action_dim), kr.WIDE_T, noise, per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, [r] * G, (i, thr))
    assert eng.kld_stats() == kr.stats_of([r] * G)


@gpu
def test_the_eval_cache_changes_nothing():
    """With an eval cache a segment's last leaves may be served by the cache: the closing expand + backup runs in front of every checkpoint."""
    og, slots, results = kr.small_results("tictactoe", 4e-3)
    eng = engine_for("tictactoe", kr.SMALL_T, cache_entries=64)
    eng.set_kld_stop(kr.SMALL_I, 4e-3)
    noise = load(eng, slots)
    eng.search_budget(evaluator(eng.action_dim), kr.SMALL_T, noise, per_launch=3)
    eng.check_error()
    assert eng.counters()["cache_hits"] > 0
    assert_is_the_restatement(eng, results, ("cache",))
    assert eng.kld_stats() == kr.stats_of(results)


# ---- 2. the rate at one checkpoint ------------------------------------------------------------------------------------------------------
def run_segment(eng, ev):
    logits = values = None
    for _ in range(4 * kr.WIDE_I + 8):
        eng.step(logits, values)
        n = int(eng.n_leaf.item())
        if n > 0:
            logits, values = eng.evaluate_leaves(ev, n)
        else:
            logits = values = None
            if eng.unfinished() == 0:
                return
    raise AssertionError("the segment does not end")


@gpu
@pytest.mark.parametrize("i", range(3))
def test_checkpoint_rate_against_float64(i):
    """The device's rate at the second checkpoint, recomputed from the root children's visits exported at the first and at the second.
    The bound.  po_i, pn_i and po_i / pn_i are single correctly rounded divisions of the same operands on both sides: identical.  The two
    logs differ: each library's is within 1 ulp of the true value (OCML's documented bound for the float64 log; glibc's is below 1 ulp), so
    with e = 2^-52 they differ by at most 2 e |log|, taken as 4 e |log| - "a few ulp".  A term t_i = po_i * log(..) then differs by at most
    4 e |t_i| from the log and e |t_i| from its own rounding.  The terms are added in the same order on both sides (kr.gain restates the lanes
    and the butterfly); each of the fewer than `children` additions a term takes part in rounds a partial sum of at most sum |t_j| and may
    round it differently: at most e * sum |t_j| each.  Together  |gain - gain'| <= (5 + children) e sum |t_j|,  bounded here by
    8 * children * e * sum |t_j|;  the division by (S - So) adds e |rate|."""
    og, s, _ = kr.wide_results(i, kr.NEVER)
    eng = engine_for("gomoku15", kr.WIDE_T)
    eng.set_kld_stop(kr.WIDE_I, kr.NEVER)
    noise = load(eng, [s] * G)
    ev = evaluator(eng.action_dim)
    eng.begin_search_budget(noise, kr.WIDE_T, 3)
    run_segment(eng, ev)
    assert eng.kld_checkpoint() == G                                 # no snapshot yet: released unjudged
    old = [eng.root_children(g)["visit"].tolist() for g in range(G)]
    run_segment(eng, ev)
    new = [eng.root_children(g)["visit"].tolist() for g in range(G)]
    assert eng.kld_checkpoint() == G and eng.kld_stats()["judged"] == G
    got = eng.kld_rate().cpu().numpy()
    eng.check_error()
    e = 2.0 ** -52
    for g in range(G):
        assert sum(old[g]) == kr.WIDE_I - 1 and sum(new[g]) == 2 * kr.WIDE_I - 1 and len(new[g]) == (48, 96, 192)[i]
        gain, mag = kr.gain(old[g], new[g])
        want = gain / float(sum(new[g]) - sum(old[g]))
        bound = 8 * len(new[g]) * e * mag / float(sum(new[g]) - sum(old[g])) + e * abs(want)
        print(f"wide root {i} game {g}: device rate {got[g]!r} float64 {want!r} |diff| {abs(got[g] - want):.3e} bound {bound:.3e}")
        assert abs(got[g] - want) <= bound, (i, g, got[g], want, bound)
        assert want == kr.wide_results(i, kr.NEVER)[2]["rates"][0]   # ... and it is the restated search's first judged rate


# ---- 3. option off ----------------------------------------------------------------------------------------------------------------------
def batch(**kw):
    """kr.never_games on the engine: Connect4 from the empty board, greedy moves, the restatement's noise rows."""
    from selfplay import self_play_batch
    res = self_play_batch(kr.NEVER_GAME, evaluator(7), G, kr.NEVER_T, seed=SEED, max_moves=kr.NEVER_MOVES, budget_stepping=True, sample_until=0,
                          noise_fn=kr.never_noise, **kw)
    return [(r.cells, [p.tobytes() for p in r.pis], r.qs, r.winner) for r in res], res


@gpu
def test_a_threshold_that_never_fires_and_clear_give_the_games_without_the_option():
    """(No search of these games has a rate of exactly 0, which is below every threshold: tests/test_kld_stop_restated.py.)"""
    import azk
    want, res = batch()
    assert [r.cells for r in res] == [g["cells"] for g in kr.never_games()]
    got, res = batch(kld_stop=(kr.NEVER_I, kr.NEVER))
    assert got == want
    assert all(r.sims == [kr.NEVER_T] * kr.NEVER_MOVES for r in res)
    eng = azk.Engine(kr.NEVER_GAME, G, kr.NEVER_T)
    eng.set_kld_stop(kr.NEVER_I, 1e-2)
    eng.clear_kld_stop()
    assert eng.kld_stop is None
    got, res = batch(engine=eng)
    assert got == want and all(r.sims == [] for r in res)
    # ... and a threshold that fires plays other games, with shorter searches
    got, res = batch(kld_stop=(kr.NEVER_I, 1e-2))
    assert got != want and any(x < kr.NEVER_T for r in res for x in r.sims)


# ---- 4. the asynchronous movers ---------------------------------------------------------------------------------------------------------
GAME_ARGS = {"gomoku": (7, 49), "tictactoe": (None, 9)}


def lockstep_records(game, moves, use_graph=False, **kw):
    """{(slot, move): (pi bytes, q, cell, winner, sims)} of SelfPlayRunner(recycle=True), and the runner."""
    from selfplay import SelfPlayRunner
    size, A = GAME_ARGS[game]
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]), int(r.record_sims[g]))
    r = SelfPlayRunner(game, evaluator(A), G, N_SIMS, size=size, seed=SEED, on_records=on, recycle=True, use_graph=use_graph, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_records(game, moves, **kw):
    from selfplay import AsyncSelfPlayRunner
    size, A = GAME_ARGS[game]
    rec = {}

    def on(meta, q, pi):
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]), int(r.record_sims[i]))
    r = AsyncSelfPlayRunner(game, evaluator(A), G, N_SIMS, size=size, seed=SEED, on_records=on, recycle=True, use_graph=False, per_launch=2,
                            steps_per_graph=4, **kw)
    for _ in range(4000):                                       # until EVERY slot has played `moves` moves (slots run at their own pace)
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(G)):
            break
    r.check_error()
    return rec, r


def assert_same_records(got, want, moves, tag):
    for g in range(G):
        for mv in range(moves):
            assert got[(g, mv)] == want[(g, mv)], tag + (g, mv)


def assert_both_outcomes(r, records):
    st = r.kld_stats()
    assert st["ended_early"] > 0 and st["ran_allowance"] > 0 and st["sims_unrun"] > 0 and st["judged"] > 0
    sims = [v[4] for v in records.values()]
    assert min(sims) < N_SIMS and all(1 <= x <= N_SIMS for x in sims)


@gpu
@pytest.mark.parametrize("game", ["gomoku", "tictactoe"])
def test_async_equals_lockstep_slot_for_slot(game):
    """tictactoe: ten moves are two or three games per slot - the recycled games start from an armed first segment, not from the columns
    the last game left."""
    want, lr = lockstep_records(game, MOVES, kld_stop=(INTERVAL, GAIN))
    got, r = async_records(game, MOVES, kld_stop=(INTERVAL, GAIN))
    assert_same_records(got, want, MOVES, (game,))
    assert_both_outcomes(lr, want)
    assert_both_outcomes(r, got)
    if game == "tictactoe":
        assert lr.games_finished >= G and int(r.finish()[0]) >= G


@gpu
def test_async_reroot_equals_lockstep_top_up():
    want, lr = lockstep_records("gomoku", MOVES, kld_stop=(INTERVAL, GAIN), tree_reuse=2)
    got, r = async_records("gomoku", MOVES, kld_stop=(INTERVAL, GAIN), reroot=2)
    assert_same_records(got, want, MOVES, ("reroot",))
    assert lr.counters()["roots_reused"] > 0 and r.counters()["roots_reused"] > 0
    assert_both_outcomes(lr, want)
    # top-up: a carried root's allowance is what brings it back to N_SIMS visits - fewer than N_SIMS new simulations even where it ran out
    assert all(v[4] <= N_SIMS for v in want.values())


@gpu
def test_async_equals_lockstep_with_a_cap_resignation_and_a_temperature():
    kw = dict(kld_stop=(INTERVAL, GAIN), playout_cap=(0.5, 8), resign=(0.6, 0.25, 2), move_temperature=1.0)
    want, lr = lockstep_records("gomoku", MOVES, **kw)
    got, r = async_records("gomoku", MOVES, **kw)
    assert_same_records(got, want, MOVES, ("combined",))
    sims = [v[4] for v in want.values()]
    assert 8 in sims and max(sims) == N_SIMS and any(8 < x < N_SIMS for x in sims)      # fast searches, full ones, and full ones ended early


@gpu
def test_graph_runner_equals_eager():
    want, _ = lockstep_records("gomoku", 6, kld_stop=(INTERVAL, GAIN))
    got, r = lockstep_records("gomoku", 6, use_graph=True, steps_per_graph=4, per_launch=2, kld_stop=(INTERVAL, GAIN))
    assert_same_records(got, want, 6, ("graph",))
    assert r.kld_stats()["ended_early"] > 0


# ---- 5. stale columns -------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_game_given_a_position_mid_run_starts_from_an_armed_first_segment():
    og, slots, results = kr.small_results("gomoku7", 1e-2)
    eng = engine_for("gomoku7", kr.SMALL_T)
    eng.set_kld_stop(kr.SMALL_I, 1e-2)
    ev = evaluator(eng.action_dim)
    eng.search_budget(ev, kr.SMALL_T, load(eng, slots), per_launch=3)
    assert_is_the_restatement(eng, results, ("first",))
    # the same positions in other slots, with the snapshots, sums, counts and `over` marks of the searches above still in the columns
    order = [(g + 3) % G for g in range(G)]
    eng.search_budget(ev, kr.SMALL_T, load(eng, [slots[g] for g in order]), per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, [results[g] for g in order], ("second",))
    both = kr.stats_of(results)
    assert eng.kld_stats() == {k: 2 * v for k, v in both.items()}


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    import azk
    e = azk.Engine("gomoku", 2, N_SIMS, size=7)
    for bad in ((0, 1e-3, 0), (N_SIMS + 1, 1e-3, 0), (8, 0.0, 0), (8, -1.0, 0), (8, float("nan"), 0), (8, float("inf"), 0), (8, 1e-3, -1)):
        with pytest.raises(azk.AzkError, match="-1"):
            e.set_kld_stop(*bad)
        assert e.kld_stop is None
    for call in (e.search_sims, e.kld_stats, e.kld_rate):
        with pytest.raises(azk.AzkError):
            call()                                                   # no option set
    with pytest.raises(azk.AzkError, match="-4"):
        e.kld_checkpoint()
    vl = azk.Engine("gomoku", 2, N_SIMS, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="-1"):
        vl.set_kld_stop(8, 1e-3)
    assert "leaves_per_step" in vl.L.azk_last_error(vl.h).decode()
    # a Gumbel root, either way round
    gm = azk.Engine("gomoku", 2, N_SIMS, size=7)
    gm.set_gumbel_root(4, N_SIMS)
    with pytest.raises(azk.AzkError, match="-4"):
        gm.set_kld_stop(8, 1e-3)
    gm.clear_gumbel_root()
    gm.set_kld_stop(8, 1e-3)
    with pytest.raises(azk.AzkError, match="-4"):
        gm.set_gumbel_root(4, N_SIMS)
    # inside a search
    e.begin_search_budget(None, N_SIMS, 8)
    with pytest.raises(azk.AzkError, match="-4"):
        e.set_kld_stop(8, 1e-3)
    e.reset_games()                                                  # new games: the search is over
    e.set_kld_stop(8, 1e-3, 16)
    assert e.kld_stop == (8, 1e-3, 16)
    # plain stepping and vanilla MCTS while set
    with pytest.raises(azk.AzkError, match="-4"):
        e.begin_search(None)
    assert e.L.azk_vanilla_search(e.h, 4, None) == -4 and "azk_set_kld_stop" in e.L.azk_last_error(e.h).decode()
    e.begin_search_budget(None, N_SIMS, 8)
    with pytest.raises(azk.AzkError, match="-4"):
        e.clear_kld_stop()                                           # inside a search
    e.reset_games()
    e.clear_kld_stop()
    e.begin_search(None)                                             # off again: the plain entry point is back
    # the asynchronous movers: fixed at async_begin, and the budget with it
    a = azk.Engine("gomoku", 2, N_SIMS, size=7)
    a.set_kld_stop(8, 1e-3)
    a.async_begin(N_SIMS, 2, 8, SEED, 0)
    for call in (lambda: a.set_kld_stop(8, 1e-3), a.clear_kld_stop, lambda: a.async_set_budget(16, 2), a.kld_checkpoint):
        with pytest.raises(azk.AzkError, match="-4"):
            call()
    a.check_error()
    b = azk.Engine("gomoku", 2, N_SIMS, size=7)
    b.async_begin(N_SIMS, 2, 8, SEED, 0)
    with pytest.raises(azk.AzkError, match="-4"):
        b.set_kld_stop(8, 1e-3)
