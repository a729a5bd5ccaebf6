"""Playout-cap randomisation (azk_set_playout_cap): per search a coin keyed like the search's noise row - (seed,
global game, the slot's move counter) - makes it FULL (n_sims simulations, the reference's search) or FAST (n_fast simulations); only
the plies of full searches are emitted as (state, pi, z).  Checked here: the coin stream against a restatement of Philox4x32-10, the
lock-step runner against the oracle's primitives ply by ply, the degenerate probabilities, emission, the asynchronous movers against
the lock-step runner (with and without tree reuse), and the refusals.  The two tests without the gpu mark run on the CPU."""
import hashlib

import numpy as np
import pytest

from fixture_eval import fixture_logits_value

gpu = pytest.mark.gpu

G, N_SIMS, N_FAST, P_FULL, MOVES, SEED = 8, 24, 6, 0.5, 30, 3
COIN_SEEDS, COIN_MOVES = (1, 3), 6
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------
# the coin, restated: Philox4x32-10, counter {gg lo, gg hi, move, 0xFFFFFFFE}, key (seed lo, seed hi)
# ---------------------------------------------------------------------------------------------------
def philox4x32_10(c, k0, k1):
    c = list(c)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def coin_full(seed, gg, move, p_full):
    c = philox4x32_10([gg & M32, gg >> 32, move, 0xFFFFFFFE], seed & M32, seed >> 32)
    return float(((c[0] << 32) | c[1]) >> 11) * 2.0 ** -53 < p_full


def test_precondition_the_chosen_seeds_mix_full_and_fast_plies():
    """CPU: with the seeds this file uses at least a quarter of the plies are full and at least a quarter fast - the runner tests (SEED,
    G slots x MOVES moves, p_full 0.5) and the coin-stream test (COIN_SEEDS, G x COIN_MOVES, p_full 0.25 and 0.5) exercise both kinds."""
    grids = [(SEED, MOVES, P_FULL)] + [(s, COIN_MOVES, p) for s in COIN_SEEDS for p in (0.25, 0.5)]
    for seed, moves, p in grids:
        flags = [coin_full(seed, g, m, p) for g in range(G) for m in range(moves)]
        assert 4 * sum(flags) >= len(flags) and 4 * (len(flags) - sum(flags)) >= len(flags), (seed, moves, p, sum(flags))
    assert not any(coin_full(SEED, g, m, 0.0) for g in range(G) for m in range(MOVES))
    assert all(coin_full(SEED, g, m, 1.0) for g in range(G) for m in range(MOVES))


def test_refusals_before_any_engine_exists():
    """CPU: the runners and self_play_batch validate playout_cap before they create an engine (no GPU here, none needed)."""
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_playout_cap, self_play_batch
    assert check_playout_cap(None, 24) is None and check_playout_cap((0.25, 6), 24) == (0.25, 6) and check_playout_cap((1, 24), 24) == (1.0, 24)
    for bad in ((-0.1, 6), (1.5, 6), (float("nan"), 6), (0.5, 0), (0.5, 25), (0.5,), "x"):
        with pytest.raises(ValueError):
            check_playout_cap(bad, 24)
        with pytest.raises(ValueError):
            SelfPlayRunner("gomoku", None, 2, 24, size=7, playout_cap=bad)
        with pytest.raises(ValueError):
            AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, playout_cap=bad)
        with pytest.raises(ValueError):
            self_play_batch("gomoku", lambda x: None, 2, 24, size=7, playout_cap=bad)
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", None, 2, 24, size=7, use_graph=True, leaves_per_step=2, playout_cap=(0.5, 6))
    with pytest.raises(ValueError, match="vanilla"):
        self_play_batch("gomoku", None, 2, 24, size=7, playout_cap=(0.5, 6))
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 24, batched=False, playout_cap=(0.5, 6))


# ---------------------------------------------------------------------------------------------------
# helpers
# ---------------------------------------------------------------------------------------------------
GAMES = {"gomoku": (7, 49), "connect4": (None, 7), "tictactoe": (None, 9)}
_shared = {}


def shared(key, make):
    """A reference computed once for the cases that need it; never modified afterwards."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def lockstep_records(game, moves, seed=SEED, n_sims=N_SIMS, cap=(P_FULL, N_FAST), n_games=G, **kw):
    """{(slot, move): (pi bytes, q, cell, winner, full)} of SelfPlayRunner(recycle=True), and the runner."""
    from selfplay import SelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        full = r.record_full
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]), int(full[g]))
    kw.setdefault("recycle", True)
    r = SelfPlayRunner(game, evaluator(A), n_games, n_sims, size=size, seed=seed, on_records=on, playout_cap=cap, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_records(game, moves, seed=SEED, n_sims=N_SIMS, cap=(P_FULL, N_FAST), n_games=G, **kw):
    from selfplay import AsyncSelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(meta, q, pi):
        full = r.record_full if r.record_full is not None else np.ones(len(meta), np.uint8)
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]), int(full[i]))
    kw.setdefault("recycle", True)
    r = AsyncSelfPlayRunner(game, evaluator(A), n_games, n_sims, size=size, seed=seed, on_records=on, playout_cap=cap, use_graph=False, **kw)
    for _ in range(8000):                                       # until EVERY slot has played `moves` moves (slots run at their own pace)
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(n_games)):
            break
    r.check_error()
    return rec, r


def assert_same_records(got, want, moves, tag=(), n_games=G):
    for g in range(n_games):
        for mv in range(moves):
            assert got[(g, mv)] == want[(g, mv)], tag + (g, mv)


def ring_rows(rp):
    """sha256 of every tuple in the ring, by slot."""
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    return [hashlib.sha256(s[i].tobytes() + p[i].tobytes() + z[i:i + 1].tobytes()).hexdigest() for i in range(rp.size())]


# ---------------------------------------------------------------------------------------------------
# 1. the coin stream
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("p_full", [0.25, 0.5])
@pytest.mark.parametrize("seed", COIN_SEEDS)
def test_coin_stream_is_the_restated_philox(seed, p_full):
    import azk
    whole, part = azk.Engine("gomoku", G, N_SIMS, size=7), azk.Engine("gomoku", 3, N_SIMS, size=7)
    whole.set_playout_cap(p_full, N_FAST, seed, 0)
    part.set_playout_cap(p_full, N_FAST, seed, 5)
    for move in range(COIN_MOVES):
        whole.begin_search_budget(None, N_SIMS, 8, move_index=move)
        part.begin_search_budget(None, N_SIMS, 8, move_index=move)
        got, sub = whole.search_full().cpu().numpy().tolist(), part.search_full().cpu().numpy().tolist()
        assert got == [int(coin_full(seed, g, move, p_full)) for g in range(G)], (seed, p_full, move)
        assert sub == got[5:8], (seed, p_full, move)             # the coins do not depend on the sharding
    whole.check_error()
    part.check_error()


# ---------------------------------------------------------------------------------------------------
# 2. lock-step, eager, against the oracle's primitives
# ---------------------------------------------------------------------------------------------------
def oracle_records(game, moves, seed=SEED, n_sims=N_SIMS, cap=(P_FULL, N_FAST)):
    """Every slot's games through oracle.az_oracle primitives in a loop shaped like <Game>.self_play, the search size by the coin; noise
    rows and move uniforms are the engine's own (Engine.gen_noise)."""
    import torch
    import azk
    from oracle import az_oracle as ao
    from selfplay import SAMPLE_UNTIL
    size, A = GAMES[game]
    og = ao.OracleGame(game, size)
    eng = azk.Engine(game, G, n_sims, size=size)
    draws = [eng.gen_noise(seed, 0, mv) for mv in range(moves)]
    draws = [(nz.cpu().numpy(), u.cpu().numpy()) for nz, u in draws]

    def ev(canon):
        logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], A, "hash")
        return ao.softmax_det(logits[0].numpy()), float(v[0])
    rec = {}
    for g in range(G):
        tree = ao.OracleTree(og)
        board, player, mc = og.new_board(), 0, 0
        for mv in range(moves):
            full = coin_full(seed, g, mv, cap[0])
            tree.reset(player, mc)
            ao.mcts(og, tree, board, n_sims if full else cap[1], ev, draws[mv][0][g])
            pi = tree.pi()
            q = tree.root_value / tree.root_visit
            if mc < SAMPLE_UNTIL[game]:
                cell = tree.cell_for_action(ao.sample_action(pi, draws[mv][1][g]))
            else:
                cell = tree.max_visit_cell()
            mover = player
            player = og.make_move(board, player, og.rc(cell))
            mc += 1
            w = og.check_winner(board, mover, og.rc(cell))
            winner = w if w != -1 else (-1 if mc == og.state_dim else -2)
            rec[(g, mv)] = (pi.tobytes(), float(q), int(cell), int(winner), int(full))
            if winner != -2:
                board, player, mc = og.new_board(), 0, 0
    return rec


@gpu
@pytest.mark.parametrize("game,moves,cache", [("gomoku", MOVES, "off"), ("gomoku", MOVES, "per_game"), ("gomoku", MOVES, "shared"),
                                              ("connect4", 20, "off"), ("tictactoe", 14, "off")])
def test_lockstep_eager_equals_the_oracle(game, moves, cache):
    want = shared(("oracle", game), lambda: oracle_records(game, moves))
    kw = dict(off={}, per_game=dict(cache_entries=64), shared=dict(cache_entries=64, cache_shared=True))[cache]
    got, r = lockstep_records(game, moves, **kw)
    kinds = [v[4] for v in got.values()]
    assert 0 < sum(kinds) < len(kinds)
    assert_same_records(got, want, moves, (game, cache))
    assert r.games_finished > 0                                  # game ends and restarts were part of it


@gpu
def test_graph_runner_equals_eager():
    """SelfPlayRunner(use_graph=True, playout_cap=...): budget stepping inside the captured step graph plays the eager runner's games."""
    want = shared(("lockstep", "gomoku", 64), lambda: lockstep_records("gomoku", MOVES, cache_entries=64)[0])
    got, _ = lockstep_records("gomoku", MOVES, cache_entries=64, use_graph=True, steps_per_graph=4, per_launch=2)
    assert_same_records(got, want, MOVES)


# ---------------------------------------------------------------------------------------------------
# 3. degenerate probabilities
# ---------------------------------------------------------------------------------------------------
@gpu
def test_p_full_one_is_the_runner_without_the_option():
    import azk
    ra, rb = azk.DeviceReplay(3000, 2, 7, 7, 49), azk.DeviceReplay(3000, 2, 7, 7, 49)
    plain, _ = lockstep_records("gomoku", MOVES, cap=None, replay=ra)
    capped, _ = lockstep_records("gomoku", MOVES, cap=(1.0, N_FAST), replay=rb)
    assert plain == capped and all(v[4] == 1 for v in capped.values())
    assert int(ra.cursor.item()) == int(rb.cursor.item()) > 0
    for a, b in ((ra.states, rb.states), (ra.pis, rb.pis), (ra.zs, rb.zs)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


@gpu
def test_p_full_zero_is_the_runner_with_n_fast_simulations_and_an_empty_ring():
    import azk
    rb = azk.DeviceReplay(3000, 2, 7, 7, 49)
    small, _ = lockstep_records("gomoku", MOVES, n_sims=N_FAST, cap=None)
    capped, r = lockstep_records("gomoku", MOVES, cap=(0.0, N_FAST), replay=rb)
    assert capped.keys() == small.keys() and r.games_finished > 0
    for k in small:
        assert capped[k][:4] == small[k][:4] and capped[k][4] == 0, k
    assert int(rb.cursor.item()) == 0 and rb.size() == 0


# ---------------------------------------------------------------------------------------------------
# 4. emission
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("capacity", [4096, 97])
def test_emission_is_the_oracle_emission_without_the_fast_plies(capacity):
    """Every finished game's tuples are oracle.replay_oracle.emit_tuples(boards, pis, winner) with the groups of fast plies dropped, in
    order within the game, from the game's first stream index on; the cursor is the total; slot t % capacity holds tuple t (97: the
    ring wraps)."""
    import azk
    from oracle import replay_oracle as ro
    from selfplay import self_play_batch
    rp = azk.DeviceReplay(capacity, 2, 7, 7, 49)
    res = self_play_batch("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, replay=rp, playout_cap=(P_FULL, N_FAST))
    stream, total = {}, 0
    for g, r in enumerate(res):
        assert r.winner is not None and len(r.full) == len(r.boards) == len(r.pis)
        assert r.full == [coin_full(SEED, g, i, P_FULL) for i in range(len(r.full))]
        tuples, at = ro.emit_tuples(r.boards, r.pis, r.winner), 0
        kept = []
        for i, full in enumerate(r.full):
            n = 1 if i < 2 else 8
            if full:
                kept += tuples[at:at + n]
            at += n
        assert at == len(tuples)
        for k, t in enumerate(kept):
            assert r.replay_base + k not in stream
            stream[r.replay_base + k] = t
        total += len(kept)
    assert int(rp.cursor.item()) == total == len(stream) and sorted(stream) == list(range(total)) and total > capacity // 40
    assert any(not all(r.full) for r in res) and rp.size() == min(total, capacity)
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    for t in range(max(0, total - capacity), total):
        st, pi, zz = stream[t]
        slot = t % capacity
        assert s[slot].tobytes() == np.ascontiguousarray(st, np.float32).tobytes() and p[slot].tobytes() == np.ascontiguousarray(pi, np.float64).tobytes(), t
        assert float(z[slot]) == zz, t


@gpu
def test_collect_data_host_buffer_skips_the_fast_plies_too():
    """train.collect_data(..., playout_cap=...): a host buffer (save_data_to_buffer by the flags) and a DeviceReplay (the engine's emission)
    receive the same tuples."""
    import azk
    import train as az_train
    from fixture_eval import FixtureModel
    from games import Gomoku
    Gomoku.rows = Gomoku.cols = 7
    Gomoku.action_dim = Gomoku.state_dim = 49

    class HostBuffer:
        def __init__(self):
            self.buffer = []

        def add(self, s, p, r):
            self.buffer.append((np.array(s, np.float32), np.array(p, np.float64), list(r)))
    dev_buf, host_buf = azk.DeviceReplay(4096, 2, 7, 7, 49), HostBuffer()
    r1 = az_train.collect_data(Gomoku, FixtureModel(49), dev_buf, 4, N_SIMS, seed=SEED, playout_cap=(P_FULL, N_FAST))
    r2 = az_train.collect_data(Gomoku, FixtureModel(49), host_buf, 4, N_SIMS, seed=SEED, playout_cap=(P_FULL, N_FAST))
    plain = HostBuffer()
    az_train.collect_data(Gomoku, FixtureModel(49), plain, 4, N_SIMS, seed=SEED, playout_cap=(1.0, N_FAST))
    keyed = lambda items: sorted((s.tobytes(), p.tobytes(), float(z[0])) for s, p, z in items)
    assert r1 == r2 and sum(r1) == 4
    assert 0 < dev_buf.size() == len(host_buf.buffer) and keyed(dev_buf.to_reference_deque()) == keyed(host_buf.buffer)
    assert len(plain.buffer) > 0


# ---------------------------------------------------------------------------------------------------
# 5. the asynchronous movers play the lock-step games
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("per_launch", [1, 2, 3])
def test_async_equals_lockstep_slot_for_slot(per_launch):
    want = shared(("lockstep", "gomoku", 64), lambda: lockstep_records("gomoku", MOVES, cache_entries=64)[0])
    got, r = async_records("gomoku", MOVES, cache_entries=64, per_launch=per_launch, steps_per_graph=4)
    assert_same_records(got, want, MOVES, (per_launch,))
    st = r.finish()
    assert int(st[0]) > 0 and int(st[5]) == len(got)
    assert int(st[8]) > 0 and int(st[9]) > 0 and int(st[8] + st[9]) == int(st[7])      # full + fast = searches begun
    # every search begun after the first of a slot is the search behind one of its records, or still running
    begun = {1: 0, 0: 0}
    for (g, mv), v in got.items():
        if mv > 0:
            begun[v[4]] += 1
    assert begun[1] <= int(st[8]) <= begun[1] + G and begun[0] <= int(st[9]) <= begun[0] + G


@gpu
def test_async_replay_equals_lockstep_as_a_multiset():
    """Games played to the end without restarts: the drain's emission holds the tuples of the lock-step runner's (the stream order follows
    the finishing order)."""
    import azk
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner
    ra, rb = azk.DeviceReplay(4096, 2, 7, 7, 49), azk.DeviceReplay(4096, 2, 7, 7, 49)
    r = SelfPlayRunner("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, recycle=False, replay=ra, playout_cap=(P_FULL, N_FAST))
    for _ in range(49):
        r.play_move()
    r.check_error()
    a = AsyncSelfPlayRunner("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, recycle=False, replay=rb, per_launch=2, steps_per_graph=4,
                            use_graph=False, playout_cap=(P_FULL, N_FAST))
    for _ in range(3000):
        a.run_chunk()
        if int(a.finish()[0]) == G:
            break
    a.check_error()
    assert int(a.finish()[0]) == G
    assert 0 < ra.size() == rb.size() == int(rb.cursor.item()) and sorted(ring_rows(ra)) == sorted(ring_rows(rb))


# ---------------------------------------------------------------------------------------------------
# 6. with tree reuse
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_async_reroot_equals_lockstep_tree_reuse(mode):
    want, lr = lockstep_records("gomoku", MOVES, cache_entries=64, tree_reuse=mode)
    got, r = async_records("gomoku", MOVES, cache_entries=64, per_launch=2, steps_per_graph=4, reroot=mode)
    kinds = [v[4] for v in want.values()]
    assert 0 < sum(kinds) < len(kinds)
    assert_same_records(got, want, MOVES, (mode,))
    assert lr.counters()["roots_reused"] > 0 and r.counters()["roots_reused"] > 0
    st = r.finish()
    assert int(st[8]) > 0 and int(st[9]) > 0 and int(st[8] + st[9]) == int(st[7])


@gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_root_visits_follow_the_per_game_target(mode):
    """The per-game target replaces n_sims in the re-root: with `carried` the root's visits when the search begins (0: fresh root), the
    search ends at carried + target visits in carry mode and at max(target, carried + 1) in top-up."""
    import torch
    import azk
    e = azk.Engine("gomoku", G, N_SIMS, size=7, tree_reuse=mode)
    e.reset_games()
    e.set_playout_cap(P_FULL, N_FAST, SEED, 0)
    ev = evaluator(49)
    stats = torch.zeros(8, dtype=torch.int64, device=e.device)
    reused_searches = 0
    for mv in range(12):
        noise, uni = e.gen_noise(SEED, 0, mv)
        e.begin_search_budget(noise, N_SIMS, 2, move_index=mv)
        carried = e.root_stats()[2].cpu().numpy().copy()
        full = e.search_full().cpu().numpy().copy()
        assert full.tolist() == [int(coin_full(SEED, g, mv, P_FULL)) for g in range(G)]
        logits = values = None
        for _ in range(2 * N_SIMS + 8):
            e.step(logits, values)
            n = int(e.n_leaf.item())
            if n > 0:
                logits, values = ev(e.leaf_boards[:n])
                logits, values = logits.contiguous(), values.reshape(-1).contiguous()
            else:
                logits = values = None
                if e.unfinished() == 0:
                    break
        assert e.unfinished() == 0
        visits = e.root_stats()[2].cpu().numpy()
        for g in range(G):
            target = N_SIMS if full[g] else N_FAST
            want = carried[g] + target if mode == 1 else max(target, carried[g] + 1)
            assert visits[g] == want, (mode, mv, g, int(carried[g]), target)
        reused_searches += int((carried > 0).sum())
        e.advance(uni, 8)
        e.recycle_finished(stats)
    e.check_error()
    assert reused_searches > 0 and e.counters()["roots_reused"] == reused_searches


# ---------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    import azk
    e = azk.Engine("gomoku", 2, N_SIMS, size=7)
    for p, n in ((-0.1, 6), (1.5, 6), (float("nan"), 6), (0.5, -1), (0.5, N_SIMS + 1)):
        with pytest.raises(azk.AzkError, match="-1"):
            e.set_playout_cap(p, n)
        assert e.playout_cap is None
    with pytest.raises(azk.AzkError):
        e.search_full()                                          # no cap set
    vl = azk.Engine("gomoku", 2, N_SIMS, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="-1"):
        vl.set_playout_cap(0.5, 6)
    assert "leaves_per_step" in vl.L.azk_last_error(vl.h).decode()
    e.set_playout_cap(0.5, 6, SEED, 0)
    with pytest.raises(azk.AzkError, match="-4"):
        e.begin_search(None)                                     # a capped search needs the budget and the move key
    with pytest.raises(azk.AzkError):
        e.begin_search_budget(None, N_SIMS, 8)                   # ... the binding asks for the move key
    with pytest.raises(azk.AzkError, match="-1"):
        e.begin_search_budget(None, 4, 8, move_index=0)          # n_fast > n_sims
    with pytest.raises(azk.AzkError, match="-1"):
        e.async_begin(4, 2, 8, 0, 0)                             # n_fast > n_sims
    e.begin_search_budget(None, N_SIMS, 8, move_index=0)
    e.set_playout_cap(0.0, 0)                                    # off again: the plain entry points are back
    assert e.playout_cap is None
    e.begin_search(None)
    e.check_error()
