"""Tree reuse inside the asynchronous movers (azk_async_begin_reuse): the move kernel parks a moved game, the
drain re-roots it on the played child.  One sentence is the specification: such an engine plays, slot for slot and move for move,
the games of the lock-step reuse runner - SelfPlayRunner(tree_reuse=mode, recycle=True) with the same seed, first global game,
budget and arena.  Records are (pi bytes, q, chosen cell, winner) per (slot, move) and are compared for equality."""
import hashlib

import pytest
import torch

from fixture_eval import fixture_logits_value

pytestmark = pytest.mark.gpu


def lockstep_records(game, ev, G, sims, moves, size, seed, leaf_dtype="float32", **kw):
    from selfplay import SelfPlayRunner
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        for g in range(G):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]))
    r = SelfPlayRunner(game, ev, G, sims, size=size, seed=seed, leaf_dtype=leaf_dtype, recycle=True, on_records=on, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_records(game, ev, G, sims, moves, size, seed, leaf_dtype="float32", **kw):
    from selfplay import AsyncSelfPlayRunner
    rec = {}

    def on(meta, q, pi):
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]))
    r = AsyncSelfPlayRunner(game, ev, G, sims, size=size, seed=seed, leaf_dtype=leaf_dtype, recycle=True, on_records=on, **kw)
    # until EVERY slot has played `moves` moves (slots run at their own pace)
    for _ in range(8000):
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(G)):
            break
    r.check_error()
    return rec, r


def assert_same_records(got, want, G, moves, tag=()):
    for g in range(G):
        for mv in range(moves):
            assert got[(g, mv)] == want[(g, mv)], tag + (g, mv)


_shared = {}


def shared(key, make):
    """A reference computed once for the cases that need it; never modified afterwards."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


# ---------------------------------------------------------------------------------------------------
# 1. fixture evaluator, eager stepping, across game ends and restarts
# ---------------------------------------------------------------------------------------------------
FIXTURE_CASES = [("gomoku", 7, 49, 40, 40), ("connect4", None, 7, 40, 20), ("tictactoe", None, 9, 30, 14)]


@pytest.mark.parametrize("game,size,A,sims,moves", FIXTURE_CASES)
@pytest.mark.parametrize("per_launch", [1, 3])
@pytest.mark.parametrize("mode", [1, 2])
def test_async_reroot_plays_the_lockstep_reuse_games(game, size, A, sims, moves, per_launch, mode):
    G = 24
    ev = lambda x: fixture_logits_value(x, A, "hash")
    want = shared(("fixture", game, mode), lambda: lockstep_records(game, ev, G, sims, moves, size, 5, cache_entries=64, tree_reuse=mode)[0])
    got, r = async_records(game, ev, G, sims, moves, size, 5, cache_entries=64, per_launch=per_launch, steps_per_graph=4, use_graph=False, reroot=mode)
    assert_same_records(got, want, G, moves, (mode, per_launch))
    st = r.finish()
    assert int(st[5]) == len(got) and int(st[0]) > 0 and int(st[2] + st[3] + st[4]) == int(st[0])
    c = r.counters()
    assert c["roots_reused"] > G
    if mode == 2:
        assert c["sims"] < int(st[5]) * sims                   # top-up searches really are shorter


# ---------------------------------------------------------------------------------------------------
# 2. a subtree that crosses the mark sweep's 4 096-node window, a root with more than 64 children
# ---------------------------------------------------------------------------------------------------
def test_async_reroot_large_subtrees():
    G, sims, moves, A = 6, 140, 5, 225
    ev = lambda x: fixture_logits_value(x, A, "hash")
    want, lr = lockstep_records("gomoku", ev, G, sims, moves, 15, 7, tree_reuse=1)
    got, r = async_records("gomoku", ev, G, sims, moves, 15, 7, per_launch=2, steps_per_graph=4, use_graph=False, reroot=1)
    assert_same_records(got, want, G, moves)
    want_reused = lr.counters()["roots_reused"]
    assert want_reused > 0 and r.counters()["roots_reused"] >= want_reused       # (the asynchronous slots have played on past `moves`)


# ---------------------------------------------------------------------------------------------------
# 3. captured graphs with the real bf16 network
# ---------------------------------------------------------------------------------------------------
def real_net():
    from pvnet import NetConfig, PolicyValueNet
    return PolicyValueNet(NetConfig(15, 15, 2, 225, 5, 512, 8, 1), seed=6, device="cuda", dtype=torch.bfloat16, path="clsfold")


@pytest.mark.parametrize("per_launch", [1, 2, 4])
@pytest.mark.parametrize("mode", [1, 2])
def test_async_reroot_graph_runner_real_network(mode, per_launch):
    net = shared("net", real_net)
    G, sims, moves = 96, 64, 5
    want = shared(("net", mode), lambda: lockstep_records("gomoku", net, G, sims, moves, 15, 9, "bfloat16", use_graph=True, cache_entries=256,
                                                          cache_shared=True, steps_per_graph=8, tree_reuse=mode)[0])
    got, r = async_records("gomoku", net, G, sims, moves, 15, 9, "bfloat16", cache_entries=256, cache_shared=True, per_launch=per_launch,
                           steps_per_graph=8, reroot=mode)
    assert_same_records(got, want, G, moves, (mode, per_launch))
    assert r.counters()["roots_reused"] > G


# ---------------------------------------------------------------------------------------------------
# 4. replay emission
# ---------------------------------------------------------------------------------------------------
def test_async_reroot_replay_emission_equals_lockstep():
    import azk
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner
    A, G, sims = 49, 16, 40
    ev = lambda x: fixture_logits_value(x, A, "hash")

    def digest(rp):
        n = rp.size()
        rows = [hashlib.sha256(rp.states[i].cpu().numpy().tobytes() + rp.pis[i].cpu().numpy().tobytes() + rp.zs[i:i + 1].cpu().numpy().tobytes()).hexdigest()
                for i in range(n)]
        return sorted(rows)
    ra = azk.DeviceReplay(20000, 2, 7, 7, A)
    r = SelfPlayRunner("gomoku", ev, G, sims, size=7, seed=2, recycle=False, replay=ra, tree_reuse=2)
    for _ in range(49):
        r.play_move()
    r.check_error()
    rb = azk.DeviceReplay(20000, 2, 7, 7, A)
    a = AsyncSelfPlayRunner("gomoku", ev, G, sims, size=7, seed=2, recycle=False, replay=rb, per_launch=2, steps_per_graph=4, use_graph=False, reroot=2)
    for _ in range(3000):
        a.run_chunk()
        if int(a.finish()[0]) == G:
            break
    a.check_error()
    assert int(a.finish()[0]) == G
    assert ra.size() == rb.size() > 100 and digest(ra) == digest(rb)


# ---------------------------------------------------------------------------------------------------
# 5. the budget is raised while games are parked
# ---------------------------------------------------------------------------------------------------
def test_budget_raised_while_games_are_parked():
    """Tiny searches (12 simulations, 8 steps between drains) keep many games parked at every drain; then the budget goes to 40, as
    bench.py's pre-roll does.  A parked game holds an advanced board over a stale tree: it must neither simulate nor move again before
    its re-root, whatever the budget says."""
    from selfplay import AsyncSelfPlayRunner
    A, G = 49, 32
    ev = lambda x: fixture_logits_value(x, A, "hash")
    rec = {}

    def on(meta, q, pi):
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key                          # a game moves once
            rec[key] = pi[i].copy()
    r = AsyncSelfPlayRunner("gomoku", ev, G, 40, size=7, seed=11, recycle=True, on_records=on, cache_entries=64, per_launch=2, steps_per_graph=8,
                            use_graph=False, reroot=2)
    r.n_sims = 12
    for _ in range(6):
        r.run_chunk()
        r.finish()
    # half a chunk more without its drain: the games that move in these steps are parked when the budget changes
    before = int(r.stats[5].item())
    for _ in range(4):
        r._step_body()
    r.launches += 4
    assert int(r.stats[5].item()) > before
    r.n_sims = 40
    for _ in range(4):
        r._step_body()
    r.launches += 4
    r.eng.async_drain(None)
    r.finish()
    assert len(rec) > 0
    at_change = [max([mv for (g, mv) in rec if g == s], default=-1) for s in range(G)]
    for _ in range(4000):
        r.run_chunk()
        r.finish()
        if all((s, at_change[s] + 12) in rec for s in range(G)):
            break
    r.check_error()
    for s in range(G):
        mine = sorted(mv for (g, mv) in rec if g == s)
        assert mine == list(range(len(mine))) and len(mine) > at_change[s] + 12, s      # the move counter keeps advancing, no gap
    assert int(r.finish()[5]) == len(rec)
    for key, pi in rec.items():
        assert abs(float(pi.sum()) - 1.0) <= 1e-12, key


# ---------------------------------------------------------------------------------------------------
# 6. the arena rule refuses: a fresh root
# ---------------------------------------------------------------------------------------------------
def test_arena_rule_refusal_falls_back_to_a_fresh_root():
    """Connect4, arena_nodes = 226, 32 simulations (test_fallback_after_state_changes_and_arena_rule[small_arena]): a fresh search needs at
    most 1 + 32 * 7 = 225 nodes, a carried subtree holds at least the new root and its 7 children, 8 + 32 * 7 = 232 > 226 - every
    carry re-root is refused and the games are those of an engine without reuse.  Top-up is never refused by that arena."""
    G, sims, moves = 8, 32, 6
    ev = lambda x: fixture_logits_value(x, 7, "hash")
    kw = dict(per_launch=2, steps_per_graph=4, use_graph=False, arena_nodes=226)
    plain, _ = async_records("connect4", ev, G, sims, moves, None, 4, **kw)
    got, r = async_records("connect4", ev, G, sims, moves, None, 4, reroot=1, **kw)
    assert r.counters()["roots_reused"] == 0
    assert_same_records(got, plain, G, moves)
    st = r.finish()
    assert int(st[7]) >= int(st[5])                             # the fallback counts as a search begun
    _, r2 = async_records("connect4", ev, G, sims, moves, None, 4, reroot=2, **kw)      # (check_error inside: no AZK_ERR_ARENA_FULL)
    assert r2.counters()["roots_reused"] > 0


# ---------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    import azk
    from selfplay import AsyncSelfPlayRunner
    off = azk.Engine("gomoku", 2, 8, size=7)
    with pytest.raises(azk.AzkError, match="-4"):
        off.async_begin(8, 2, 8, 0, 0, reroot=True)
    with pytest.raises(ValueError):
        AsyncSelfPlayRunner("gomoku", None, 2, 8, size=7, reroot=3)
    for mode in (1, 2):
        e = azk.Engine("gomoku", 2, 8, size=7, tree_reuse=mode)
        with pytest.raises(azk.AzkError, match="-4"):
            e.async_begin(8, 2, 8, 0, 0)
        e.async_begin(8, 2, 8, 0, 0, reroot=True)               # ... and the new entry point takes it
        e.check_error()
