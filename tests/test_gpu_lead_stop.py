"""Adaptive search budgets, the lead rule (azk_set_lead_stop) against the plain-Python restatement of
tests/lead_stop_restated.py: whole trees at the end of the search bit for bit through eager lock-step stepping, the simulations run, the three
words of lead(), pi and the five counters; the headline property - greedy games under factor 1 are the option-off games move for move, for
fewer simulations - in self-play and in the arena; a factor that never fires and clear_lead_stop against an engine without the option; the
asynchronous movers against the lock-step runner slot for slot; both rules set; stale columns; the refusals.  The positions and factors are
those whose preconditions tests/test_lead_stop_restated.py asserts on the CPU."""
import numpy as np
import pytest

import forced_playouts_restated as fr
import kld_stop_restated as kr
import lead_stop_restated as lr
from fixture_eval import fixture_logits_value

gpu = pytest.mark.gpu
G = lr.G
SEED, MOVES, N_SIMS, INTERVAL, FACTOR = 3, 10, 32, 8, 1.33


def evaluator(A, variant="hash"):
    return lambda x: fixture_logits_value(x, A, variant)


def engine_for(name, n_sims, **kw):
    import azk
    kind, size = fr.GAMES[name.split("+")[0]] if name.split("+")[0] in fr.GAMES else ("gomoku", 15)
    return azk.Engine(kind, G, n_sims, size=size, **kw)


def load(eng, slots):
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
    return torch.from_numpy(np.stack([s["noise"] for s in slots])).to(eng.device)


def assert_is_the_restatement(eng, results, tag):
    sims = eng.search_sims().cpu().numpy()
    words = eng.lead().cpu().numpy()
    pi = eng.root_stats()[0].cpu().numpy()
    for g, r in enumerate(results):
        assert fr.same_tree(eng.export_tree(g), r["tree"]), tag + (g,)
        assert int(sims[g]) == r["run"], tag + (g, int(sims[g]), r["run"])
        assert tuple(int(x) for x in words[g]) == tuple(r["lead"]), tag + (g, words[g].tolist(), r["lead"])
        assert pi[g].tobytes() == r["pi"].tobytes(), tag + (g,)


# ---- 1. whole trees, search_sims, lead(), pi and the counters ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("f", lr.FACTORS)
@pytest.mark.parametrize("name", lr.SMALL + ("gomoku7+empty",))
def test_small_games_are_the_restatement(name, f):
    og, slots, results = lr.small_results(name, f)
    eng = engine_for(name, lr.SMALL_T)
    eng.set_lead_stop(lr.SMALL_I, f)
    noise = load(eng, slots)
    eng.search_budget(evaluator(eng.action_dim), lr.SMALL_T, noise, per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, results, (name, f))
    assert eng.lead_stats() == lr.stats_of(results)
    assert eng.kld_checkpoint() == 0 and eng.lead_stats() == lr.stats_of(results)     # a search that is over is neither judged nor counted again


@gpu
@pytest.mark.parametrize("f", lr.FACTORS)
@pytest.mark.parametrize("i", range(3))
def test_wide_roots_are_the_restatement(i, f):
    """15 x 15 with 48 / 96 / 192 root children: one, two and three trips of the wave's 64 lanes; at 96 and 192 the maximum and the second
    maximum come from different trips."""
    og, s, r = lr.wide_results(i, f)
    eng = engine_for("gomoku15", lr.WIDE_T)
    eng.set_lead_stop(lr.WIDE_I, f)
    noise = load(eng, [s] * G)
    eng.search_budget(evaluator(eng.action_dim), lr.WIDE_T, noise, per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, [r] * G, (i, f))
    assert eng.lead_stats() == lr.stats_of([r] * G)


@gpu
def test_min_sims_holds_searches_back():
    og, slots, results = lr.small_results("gomoku7", 4.0, lr.HELD_MIN_SIMS)
    eng = engine_for("gomoku7", lr.SMALL_T)
    eng.set_lead_stop(lr.SMALL_I, 4.0, lr.HELD_MIN_SIMS)
    noise = load(eng, slots)
    eng.search_budget(evaluator(eng.action_dim), lr.SMALL_T, noise, per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, results, ("held",))
    assert eng.lead_stats() == lr.stats_of(results)


@gpu
@pytest.mark.parametrize("name", ["tictactoe", "gomoku7+empty"])
def test_the_eval_cache_changes_nothing(name):
    """With an eval cache a segment's last leaves may be served by the cache: the closing expand + backup runs in front of every checkpoint."""
    og, slots, results = lr.small_results(name, 1.0)
    eng = engine_for(name, lr.SMALL_T, cache_entries=64)
    eng.set_lead_stop(lr.SMALL_I, 1.0)
    noise = load(eng, slots)
    eng.search_budget(evaluator(eng.action_dim), lr.SMALL_T, noise, per_launch=3)
    eng.check_error()
    assert eng.counters()["cache_hits"] > 0 or name != "tictactoe"                # (TicTacToe transposes within 64 simulations; the others need not)
    assert_is_the_restatement(eng, results, ("cache", name))
    assert eng.lead_stats() == lr.stats_of(results)


# ---- 2. the headline property: greedy play is move for move what it was, for fewer simulations ------------------------------------------
HEAD_SIMS, HEAD_MOVES = 64, 14


@gpu
@pytest.mark.parametrize("game,size,A", [("connect4", None, 7), ("gomoku", 7, 49)])
def test_greedy_self_play_is_move_for_move_the_game_without_the_option(game, size, A):
    """factor 1, sample_until = 0, Dirichlet noise on (the engine's own keyed rows): the first most-visited child of a stopped search is that
    of the full search, so every ply is the same - and the searches are shorter."""
    from selfplay import self_play_batch
    kw = dict(size=size, seed=SEED, max_moves=HEAD_MOVES, sample_until=0, dirichlet=True, alpha=0.3)
    want = self_play_batch(game, evaluator(A), G, HEAD_SIMS, **kw)
    got = self_play_batch(game, evaluator(A), G, HEAD_SIMS, lead_stop=(8, 1.0), **kw)
    for g in range(G):
        assert got[g].cells == want[g].cells and got[g].winner == want[g].winner, g
        assert len(got[g].sims) == len(got[g].cells) and all(1 <= x <= HEAD_SIMS for x in got[g].sims), g
    plies = sum(len(r.cells) for r in want)
    total = sum(sum(r.sims) for r in got)
    print(f"{game}: {plies} plies, {total} simulations under lead_stop=(8, 1.0) against {plies * HEAD_SIMS} without")
    assert total < plies * HEAD_SIMS


@gpu
def test_greedy_arena_games_are_move_for_move_the_games_without_the_option():
    import arena
    evs = (evaluator(49, "hash"), evaluator(49, "uniform"))
    kw = dict(model1_mcts_iter=32, model2_mcts_iter=48, sampling=False, size=7, seed=SEED)
    w0, want = arena.compete_batch("gomoku", evs[0], evs[1], G, **kw)
    w1, got = arena.compete_batch("gomoku", evs[0], evs[1], G, lead_stop=(8, 1.0), **kw)
    assert w0.tolist() == w1.tolist()
    full = total = 0
    for g in range(G):
        assert got[g].cells == want[g].cells, g
        assert len(got[g].sims) == len(got[g].cells)
        assert all(x <= (32, 48)[ply & 1] for ply, x in enumerate(got[g].sims)), g
        full += sum((32, 48)[ply & 1] for ply in range(len(got[g].cells)))
        total += sum(got[g].sims)
    print(f"arena: {total} simulations under lead_stop=(8, 1.0) against {full} without")
    assert total < full


# ---- 3. option off ----------------------------------------------------------------------------------------------------------------------
def batch(**kw):
    """kr.never_games on the engine: Connect4 from the empty board, greedy moves, the restatement's noise rows."""
    from selfplay import self_play_batch
    res = self_play_batch(kr.NEVER_GAME, evaluator(7), G, kr.NEVER_T, seed=SEED, max_moves=kr.NEVER_MOVES, budget_stepping=True, sample_until=0,
                          noise_fn=kr.never_noise, **kw)
    return [(r.cells, [p.tobytes() for p in r.pis], r.qs, r.winner) for r in res], res


@gpu
def test_a_factor_that_never_fires_and_clear_give_the_games_without_the_option():
    """(Connect4 has no single-child root in its first six plies, and lr.NEVER * lead < 1 <= left.)"""
    import azk
    want, res = batch()
    assert [r.cells for r in res] == [g["cells"] for g in kr.never_games()]
    got, res = batch(lead_stop=(kr.NEVER_I, lr.NEVER))
    assert got == want
    assert all(r.sims == [kr.NEVER_T] * kr.NEVER_MOVES for r in res)
    eng = azk.Engine(kr.NEVER_GAME, G, kr.NEVER_T)
    eng.set_lead_stop(kr.NEVER_I, 4.0)
    eng.clear_lead_stop()
    assert eng.lead_stop is None and not eng.adaptive
    got, res = batch(engine=eng)
    assert got == want and all(r.sims == [] for r in res)
    # ... and a factor that fires plays shorter searches (pi and q are those of the shorter search)
    got, res = batch(lead_stop=(kr.NEVER_I, 4.0))
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
    st = r.lead_stats()
    assert st["ended_early"] > 0 and st["sims_unrun"] > 0 and st["judged"] > 0
    sims = [v[4] for v in records.values()]
    assert min(sims) < N_SIMS and all(1 <= x <= N_SIMS for x in sims)


@gpu
@pytest.mark.parametrize("game", ["gomoku", "tictactoe"])
def test_async_equals_lockstep_slot_for_slot(game):
    """gomoku: every slot's first search is the empty board's forced move.  tictactoe: ten moves are two or three games per slot - the
    recycled games start from an armed first segment, not from the columns the last game left."""
    want, lr_ = lockstep_records(game, MOVES, lead_stop=(INTERVAL, FACTOR))
    got, r = async_records(game, MOVES, lead_stop=(INTERVAL, FACTOR))
    assert_same_records(got, want, MOVES, (game,))
    assert_both_outcomes(lr_, want)
    assert_both_outcomes(r, got)
    if game == "gomoku":
        assert lr_.lead_stats()["forced"] >= G and all(want[(g, 0)][4] == INTERVAL for g in range(G))
    if game == "tictactoe":
        assert lr_.games_finished >= G and int(r.finish()[0]) >= G


@gpu
def test_async_reroot_equals_lockstep_top_up():
    want, lr_ = lockstep_records("gomoku", MOVES, lead_stop=(INTERVAL, FACTOR), tree_reuse=2)
    got, r = async_records("gomoku", MOVES, lead_stop=(INTERVAL, FACTOR), reroot=2)
    assert_same_records(got, want, MOVES, ("reroot",))
    assert lr_.counters()["roots_reused"] > 0 and r.counters()["roots_reused"] > 0
    st = lr_.lead_stats()
    assert st["ended_early"] > 0 and st["judged"] > 0
    # top-up: a carried root's allowance is what brings it back to N_SIMS visits - fewer than N_SIMS new simulations even where it ran out
    assert all(v[4] <= N_SIMS for v in want.values())


@gpu
def test_async_equals_lockstep_with_a_cap_resignation_a_temperature_and_the_solver():
    kw = dict(lead_stop=(INTERVAL, FACTOR), playout_cap=(0.5, 8), resign=(0.6, 0.25, 2), move_temperature=1.0, solver=True)
    want, lr_ = lockstep_records("gomoku", MOVES, **kw)
    got, r = async_records("gomoku", MOVES, **kw)
    assert_same_records(got, want, MOVES, ("combined",))
    sims = [v[4] for v in want.values()]
    assert 8 in sims and any(8 < x <= N_SIMS for x in sims)                              # fast searches (and forced moves), and full ones


@gpu
def test_graph_runner_equals_eager():
    want, _ = lockstep_records("gomoku", 6, lead_stop=(INTERVAL, FACTOR))
    got, r = lockstep_records("gomoku", 6, use_graph=True, steps_per_graph=4, per_launch=2, lead_stop=(INTERVAL, FACTOR))
    assert_same_records(got, want, 6, ("graph",))
    assert r.lead_stats()["ended_early"] > 0


# ---- 5. both rules ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", lr.SMALL)
def test_both_rules_are_the_restatement(name):
    og, slots, results = lr.small_results(name, lr.BOTH_FACTOR, 0, lr.BOTH_GAIN)
    eng = engine_for(name, lr.SMALL_T)
    eng.set_kld_stop(lr.SMALL_I, lr.BOTH_GAIN)
    eng.set_lead_stop(lr.SMALL_I, lr.BOTH_FACTOR)
    noise = load(eng, slots)
    eng.search_budget(evaluator(eng.action_dim), lr.SMALL_T, noise, per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, results, ("both", name))
    assert eng.lead_stats() == lr.stats_of(results) and eng.kld_stats() == lr.kld_stats_of(results)
    assert eng.lead_stats()["ended_early"] > 0 and eng.kld_stats()["ended_early"] > 0


@gpu
def test_both_rules_share_one_interval():
    import azk
    e = azk.Engine("gomoku", 2, N_SIMS, size=7)
    e.set_kld_stop(8, 1e-3)
    with pytest.raises(azk.AzkError, match="-4"):
        e.set_lead_stop(4, 1.0)
    assert e.lead_stop is None and "interval" in e.L.azk_last_error(e.h).decode()
    e.set_lead_stop(8, 1.0)
    with pytest.raises(azk.AzkError, match="-4"):
        e.set_kld_stop(16, 1e-3)
    assert e.kld_stop == (8, 1e-3, 0)
    e.clear_kld_stop()
    e.set_lead_stop(4, 1.0)                                          # alone again: any interval
    e.set_kld_stop(4, 1e-3)
    assert e.kld_stop == (4, 1e-3, 0) and e.lead_stop == (4, 1.0, 0)
    # KLD rule off: its reads are refused while the shared ones work
    e.clear_kld_stop()
    for call in (e.kld_stats, e.kld_rate):
        with pytest.raises(azk.AzkError):
            call()
    assert e.search_sims().shape == (2,) and e.kld_checkpoint() == 0
    # lead rule off, KLD rule on: the same the other way round
    e.set_kld_stop(4, 1e-3)
    e.clear_lead_stop()
    for call in (e.lead_stats, e.lead):
        with pytest.raises(azk.AzkError):
            call()
    assert e.L.azk_get_lead_stats(e.h, np.zeros(5, np.int64).ctypes.data, None) == -4
    assert e.search_sims().shape == (2,)
    e.check_error()


# ---- 6. stale columns -------------------------------------------------------------------------------------------------------------------
@gpu
def test_a_game_given_a_position_mid_run_starts_from_an_armed_first_segment():
    og, slots, results = lr.small_results("gomoku7+empty", 1.33)
    eng = engine_for("gomoku7", lr.SMALL_T)
    eng.set_lead_stop(lr.SMALL_I, 1.33)
    ev = evaluator(eng.action_dim)
    eng.search_budget(ev, lr.SMALL_T, load(eng, slots), per_launch=3)
    assert_is_the_restatement(eng, results, ("first",))
    # the same positions in other slots, with the words, counts and `over` marks of the searches above still in the columns
    order = [(g + 3) % G for g in range(G)]
    eng.search_budget(ev, lr.SMALL_T, load(eng, [slots[g] for g in order]), per_launch=3)
    eng.check_error()
    assert_is_the_restatement(eng, [results[g] for g in order], ("second",))
    both = lr.stats_of(results)
    assert eng.lead_stats() == {k: 2 * v for k, v in both.items()}


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    import azk
    e = azk.Engine("gomoku", 2, N_SIMS, size=7)
    for bad in ((0, 1.0, 0), (N_SIMS + 1, 1.0, 0), (8, 0.0, 0), (8, -1.0, 0), (8, float("nan"), 0), (8, float("inf"), 0), (8, 1.0, -1)):
        with pytest.raises(azk.AzkError, match="-1"):
            e.set_lead_stop(*bad)
        assert e.lead_stop is None
    for call in (e.search_sims, e.lead_stats, e.lead):
        with pytest.raises(azk.AzkError):
            call()                                                   # no option set
    with pytest.raises(azk.AzkError, match="-4"):
        e.kld_checkpoint()
    vl = azk.Engine("gomoku", 2, N_SIMS, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="-1"):
        vl.set_lead_stop(8, 1.0)
    assert "leaves_per_step" in vl.L.azk_last_error(vl.h).decode()
    # a Gumbel root, either way round
    gm = azk.Engine("gomoku", 2, N_SIMS, size=7)
    gm.set_gumbel_root(4, N_SIMS)
    with pytest.raises(azk.AzkError, match="-4"):
        gm.set_lead_stop(8, 1.0)
    gm.clear_gumbel_root()
    gm.set_lead_stop(8, 1.0)
    with pytest.raises(azk.AzkError, match="-4"):
        gm.set_gumbel_root(4, N_SIMS)
    # inside a search
    e.begin_search_budget(None, N_SIMS, 8)
    with pytest.raises(azk.AzkError, match="-4"):
        e.set_lead_stop(8, 1.0)
    e.reset_games()                                                  # new games: the search is over
    e.set_lead_stop(8, 1.0, 16)
    assert e.lead_stop == (8, 1.0, 16)
    # plain stepping and vanilla MCTS while set
    with pytest.raises(azk.AzkError, match="-4"):
        e.begin_search(None)
    assert e.L.azk_vanilla_search(e.h, 4, None) == -4 and "azk_set_lead_stop" in e.L.azk_last_error(e.h).decode()
    e.begin_search_budget(None, N_SIMS, 8)
    with pytest.raises(azk.AzkError, match="-4"):
        e.clear_lead_stop()                                          # inside a search
    e.reset_games()
    e.clear_lead_stop()
    e.begin_search(None)                                             # off again: the plain entry point is back
    # ... and the engine is usable after all that: a search under the rule is the restatement's
    og, slots, results = lr.small_results("gomoku7", 1.0)
    u = engine_for("gomoku7", lr.SMALL_T)
    with pytest.raises(azk.AzkError, match="-1"):
        u.set_lead_stop(0, 1.0)
    u.set_lead_stop(lr.SMALL_I, 1.0)
    u.search_budget(evaluator(u.action_dim), lr.SMALL_T, load(u, slots), per_launch=3)
    u.check_error()
    assert_is_the_restatement(u, results, ("usable",))
    # the asynchronous movers: fixed at async_begin, and the budget with it
    a = azk.Engine("gomoku", 2, N_SIMS, size=7)
    a.set_lead_stop(8, 1.0)
    a.async_begin(N_SIMS, 2, 8, SEED, 0)
    for call in (lambda: a.set_lead_stop(8, 1.0), a.clear_lead_stop, lambda: a.async_set_budget(16, 2), a.kld_checkpoint):
        with pytest.raises(azk.AzkError, match="-4"):
            call()
    a.check_error()
    b = azk.Engine("gomoku", 2, N_SIMS, size=7)
    b.async_begin(N_SIMS, 2, 8, SEED, 0)
    with pytest.raises(azk.AzkError, match="-4"):
        b.set_lead_stop(8, 1.0)
