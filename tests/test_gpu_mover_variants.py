"""Every instantiation of the two movers (k_advance, k_move_async; azk_moves.hip) and the emitter instantiations (azk_emit.hip) no other file reaches.
The option files test each opt-in with the combinations it was written for; this file launches ALL sixteen (re-root, playout cap,
resignation, forced playouts) combinations on their board - Gomoku 7 x 7, test_gpu_forced_playouts' MOVES, cap, resignation and k with
test_gpu_playout_cap's G and helpers - and asserts per case that the asynchronous movers play the lock-step runner's games slot for slot,
bit for bit, and that every option of the case was live in both runs (a case must not pass with its option idle).  The lock-step side of
a case runs k_advance<cap, resign, forced>, the asynchronous side k_move_async<re-root, cap, resign, forced>.

Seeds: every case runs with the option files' SEED except those listed in SEEDS, for which the lock-step run alone showed an option idle
at SEED (see there)."""
import itertools

import numpy as np
import pytest

import emission_restated as er
from fixture_eval import fixture_logits_value
from test_gpu_forced_playouts import CAP, K, MOVES
from test_gpu_playout_cap import G, N_SIMS, SEED, assert_same_records, async_records, lockstep_records, ring_rows

gpu = pytest.mark.gpu
RESIGN = (0.25, 0.5)                                              # test_gpu_forced_playouts' "cap_resign" case
REROOT = 2                                                        # ... and its "reroot2" case (the movers' template knows only on / off)
CASES = list(itertools.product((0, REROOT), (False, True), (False, True), (False, True)))
# (reroot, cap, resign, forced) -> seed, where SEED leaves an option of the case idle.  Re-root + resignation + forced playouts without a cap: no
# game of the lock-step run resigns within MOVES moves at SEED = 3 (nor at seeds 1, 2, 4 to 9); 10 is the first seed at which one does.
SEEDS = {(REROOT, False, True, True): 10}


def case_id(c):
    return "-".join(n for n, on in zip(("reroot", "cap", "resign", "forced"), c) if on) or "plain"


@gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_async_movers_play_the_lockstep_games(case):
    reroot, cap, resign, forced = case
    lock_kw, async_kw = dict(cache_entries=64), dict(cache_entries=64, per_launch=2, steps_per_graph=4)
    if reroot:
        lock_kw["tree_reuse"] = async_kw["reroot"] = reroot
    if resign:
        lock_kw["resign"] = async_kw["resign"] = RESIGN
    opts = dict(seed=SEEDS.get(case, SEED), cap=CAP if cap else None, forced_playouts=K if forced else None)
    want, lr = lockstep_records("gomoku", MOVES, **opts, **lock_kw)
    got, ar = async_records("gomoku", MOVES, **opts, **async_kw)
    kinds = [v[4] for v in want.values()]
    lc, ac = lr.counters(), ar.counters()
    print(case_id(case), "seed", opts["seed"], "full plies", sum(kinds), "of", len(kinds), "resigned", lr.resign_stats()[0] if resign else None,
          "pruned", lc["visits_pruned"], ac["visits_pruned"], "reused", lc["roots_reused"], ac["roots_reused"])
    assert_same_records(got, want, MOVES, (case_id(case),))
    # every option of the case was live, in both runs; an option that is off left no trace
    assert 0 < sum(kinds) < len(kinds) if cap else all(kinds)
    if resign:
        assert lr.resign_stats()[0] > 0 and ar.resign_stats()[0] > 0
    for c in (lc, ac):
        assert (c["visits_pruned"] > 0) == forced and (c["roots_reused"] > 0) == bool(reroot)


def drain_until_every_game_ended(a, n_games):
    for _ in range(3000):
        a.run_chunk()
        if int(a.finish()[0]) == n_games:
            break
    a.check_error()
    assert int(a.finish()[0]) == n_games


@gpu
def test_async_drain_with_cap_and_element_mask_emits_the_lockstep_tuples():
    """k_emit_tuples<LIST, CAP, SYM>: the drain of a capped engine created with emit_elements, against the lock-step emission as a multiset
    (test_gpu_emit_symmetry's capped Connect4 batch, whose plies are of both kinds)."""
    import test_gpu_emit_symmetry as es
    from selfplay import AsyncSelfPlayRunner
    res, ring, cursor = es.play("connect4", None, "board", 8, playout_cap=(0.5, 4))
    flags = [f for r in res for f in r.full]
    assert any(flags) and not all(flags) and cursor > 0
    want = sorted(er.tuple_sha(ring[0][i], ring[1][i], ring[2][i]) for i in range(cursor))
    rb = es.new_ring("connect4", None, len(ring[2]))
    a = AsyncSelfPlayRunner("connect4", lambda x: fixture_logits_value(x, 7, "hash"), es.G, es.SIMS, seed=8, recycle=False, replay=rb, per_launch=2,
                            steps_per_graph=4, use_graph=False, emit_symmetry="board", playout_cap=(0.5, 4))
    drain_until_every_game_ended(a, es.G)
    s, p, z = es.ring_numpy(rb)
    assert int(rb.cursor.item()) == cursor
    assert sorted(er.tuple_sha(s[i], p[i], z[i]) for i in range(cursor)) == want
    assert np.all(z[cursor:] == 7.0) and np.all(s[cursor:] == -5.0)


@gpu
def test_async_drain_with_cap_on_a_rerooting_engine_emits_the_lockstep_tuples():
    """k_emit_tuples<LIST, CAP> behind k_reroot_list<CAP>: games played to the end without restarts on a re-rooting capped engine, against
    SelfPlayRunner(tree_reuse=...)'s emission as a multiset (the stream order follows the finishing order)."""
    import azk
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner
    ev = lambda x: fixture_logits_value(x, 49, "hash")
    ra, rb = azk.DeviceReplay(4096, 2, 7, 7, 49), azk.DeviceReplay(4096, 2, 7, 7, 49)
    r = SelfPlayRunner("gomoku", ev, G, N_SIMS, size=7, seed=SEED, recycle=False, replay=ra, playout_cap=CAP, tree_reuse=REROOT)
    for _ in range(49):
        r.play_move()
    r.check_error()
    a = AsyncSelfPlayRunner("gomoku", ev, G, N_SIMS, size=7, seed=SEED, recycle=False, replay=rb, per_launch=2, steps_per_graph=4,
                            use_graph=False, playout_cap=CAP, reroot=REROOT)
    drain_until_every_game_ended(a, G)
    assert r.counters()["roots_reused"] > 0 and a.counters()["roots_reused"] > 0
    assert 0 < ra.size() == rb.size() == int(rb.cursor.item()) and sorted(ring_rows(ra)) == sorted(ring_rows(rb))
