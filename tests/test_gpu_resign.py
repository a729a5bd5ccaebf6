"""Resignation (azk_set_resign): after a move that does not end the game, the side that has just moved concedes when
the recorded root q - root.value / root.visit, the outcome for the OPPONENT of the side to move, no sign change - is >= v_resign and the
game has at least min_ply plies; a game coin keyed (seed, global game, move key of the game's first search) makes a share p_never of the
games never-resign control games, which are only marked.  Checked here: the lock-step runner against a restatement of the rule around the
oracle's primitives (the coin restated in Python, the engine's flags never the checker), the four statistics, the graph runner, sharding,
the degenerate settings, emission, the asynchronous movers against the lock-step runner (with and without tree reuse and a playout
cap), self_play_batch / collect_data, and the refusals.  The two tests without the gpu mark run on the CPU.

SEED, G and MOVES were chosen on a GPU run for the precondition of test_lockstep_eager_equals_the_restatement: with the engine's own noise
rows the restatement alone (Gomoku 7x7, v_resign 0.25, p_never 0.5) gives, within MOVES moves of G slots, at least two games ended by
resignation, two ended naturally, one never-resign game with a false-positive mark and one whose marked side did lose."""
import hashlib

import numpy as np
import pytest

from fixture_eval import fixture_logits_value

gpu = pytest.mark.gpu

G, N_SIMS, MOVES, SEED = 8, 24, 40, 6
V, P_NEVER = 0.25, 0.5
TTT_V, TTT_MIN_PLY, TTT_MOVES = 0.15, 4, 20
CAP = (0.5, 6)
M32 = 0xFFFFFFFF


# ---------------------------------------------------------------------------------------------------
# the coins, restated: Philox4x32-10, key (seed lo, seed hi); the game coin's counter is {gg lo, gg hi, start, 0xFFFFFFFD}, the playout
# cap's {gg lo, gg hi, move, 0xFFFFFFFE}
# ---------------------------------------------------------------------------------------------------
def philox4x32_10(c, k0, k1):
    c = list(c)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def keyed_u(seed, gg, word2, word3):
    c = philox4x32_10([gg & M32, gg >> 32, word2 & M32, word3], seed & M32, seed >> 32)
    return float(((c[0] << 32) | c[1]) >> 11) * 2.0 ** -53


def never_resigns(seed, gg, start, p_never):
    return keyed_u(seed, gg, start, 0xFFFFFFFD) < p_never


def coin_full(seed, gg, move, p_full):
    return keyed_u(seed, gg, move, 0xFFFFFFFE) < p_full


def test_precondition_the_game_coin_mixes_both_kinds():
    """CPU: over the seeds this file uses (SEED; game starts 0 .. MOVES - 1 of G slots: every key a game of the runner tests can have) the
    restated coin makes at least a quarter of the games never-resign games and at least a quarter not at p_never 0.5, none at 0, all at 1."""
    flags = [never_resigns(SEED, g, s, 0.5) for g in range(G) for s in range(MOVES)]
    assert 4 * sum(flags) >= len(flags) and 4 * (len(flags) - sum(flags)) >= len(flags), sum(flags)
    first = [never_resigns(SEED, g, 0, 0.5) for g in range(G)]                    # the first game of each slot alone
    assert 4 * sum(first) >= G and 4 * (G - sum(first)) >= G, first
    assert not any(never_resigns(SEED, g, s, 0.0) for g in range(G) for s in range(MOVES))
    assert all(never_resigns(SEED, g, s, 1.0) for g in range(G) for s in range(MOVES))
    # a start below 0 (a game set up with move_count > 0) is its low 32 bits
    assert never_resigns(SEED, 1, -3, 0.5) == never_resigns(SEED, 1, 0xFFFFFFFD, 0.5)


def test_refusals_before_any_engine_exists():
    """CPU: the runners, self_play_batch and collect_data validate resign before they create an engine (no GPU here, none needed)."""
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_resign, self_play_batch
    ev = lambda x: None
    assert check_resign(None) is None and check_resign((0.25, 0.5)) == (0.25, 0.5, 0) and check_resign((1, 0, 4)) == (1.0, 0.0, 4)
    for bad in ((0.0, 0.5), (-0.1, 0.5), (1.5, 0.5), (float("nan"), 0.5), (0.25, -0.1), (0.25, 1.5), (0.25, float("nan")), (0.25, 0.5, -1),
                (0.25, 0.5, 1.5), (0.25,), (0.25, 0.5, 0, 0), "x", 0.25):
        with pytest.raises(ValueError):
            check_resign(bad)
        with pytest.raises(ValueError):
            SelfPlayRunner("gomoku", ev, 2, 24, size=7, resign=bad)
        with pytest.raises(ValueError):
            AsyncSelfPlayRunner("gomoku", ev, 2, 24, size=7, resign=bad)
        with pytest.raises(ValueError):
            self_play_batch("gomoku", ev, 2, 24, size=7, resign=bad)
    with pytest.raises(ValueError, match="leaves_per_step"):
        SelfPlayRunner("gomoku", ev, 2, 24, size=7, use_graph=True, leaves_per_step=2, resign=(V, P_NEVER))
    with pytest.raises(ValueError, match="leaves_per_step"):
        self_play_batch("gomoku", ev, 2, 24, size=7, leaves_per_step=2, resign=(V, P_NEVER))
    for make in (lambda: SelfPlayRunner("gomoku", None, 2, 24, size=7, resign=(V, P_NEVER)),
                 lambda: AsyncSelfPlayRunner("gomoku", None, 2, 24, size=7, resign=(V, P_NEVER)),
                 lambda: self_play_batch("gomoku", None, 2, 24, size=7, resign=(V, P_NEVER)),
                 lambda: self_play_batch("gomoku", (ev, None), 2, 24, size=7, resign=(V, P_NEVER))):
        with pytest.raises(ValueError, match="vanilla"):
            make()
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 24, batched=False, resign=(V, P_NEVER))


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


def engine_draws(game, moves, seed=SEED):
    """[(noise rows float64 [G, A], move uniforms float64 [G])] per move key: the engine's own (Engine.gen_noise)."""
    def make():
        import azk
        size, _ = GAMES[game]
        eng = azk.Engine(game, G, N_SIMS, size=size)
        return [(nz.cpu().numpy(), u.cpu().numpy()) for nz, u in (eng.gen_noise(seed, 0, mv) for mv in range(moves))]
    return shared(("draws", game, moves, seed), make)


class Restated:
    """What restate() returns: rec {(slot, move): (pi bytes, q, cell, winner, resigned)}, stats (the four counts of azk_get_resign_stats over
    the games that ended), games [slot] -> [(plies, winner, resigned, never, marked side or None)] of the games that ended."""

    def __init__(self):
        self.rec, self.stats, self.games = {}, [0, 0, 0, 0], {}

    def kinds(self):
        """(ended by resignation, ended naturally, never-resign with a false-positive mark, never-resign whose marked side lost)"""
        allg = [x for gs in self.games.values() for x in gs]
        nat = sum(1 for x in allg if not x[2])
        fp = sum(1 for x in allg if x[3] and x[4] is not None and x[1] != 1 - x[4])
        tp = sum(1 for x in allg if x[3] and x[4] is not None and x[1] == 1 - x[4])
        return self.stats[0], nat, fp, tp


def restate(game, moves, draws, resign, seed=SEED, n_sims=N_SIMS, cap=None, slots=range(G)):
    """Every slot's games through oracle.az_oracle primitives in a loop shaped like <Game>.self_play, with the rule restated: the move the
    search chose is played; if it does not end the game, mc + 1 >= min_ply and q >= v_resign, the mover concedes - or, in a never-resign
    game (the restated coin), is noted as the game's mark if it has none.  resign None: no rule.  cap: the search size by the coin of the
    playout cap.  Noise rows and move uniforms come from `draws` (by move key)."""
    import torch
    from oracle import az_oracle as ao
    from selfplay import SAMPLE_UNTIL
    size, A = GAMES[game]
    og = ao.OracleGame(game, size)
    v, p_never, min_ply = (resign + (0,))[:3] if resign is not None else (None, 0.0, 0)

    def ev(canon):
        logits, val = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], A, "hash")
        return ao.softmax_det(logits[0].numpy()), float(val[0])
    out = Restated()
    for g in slots:
        out.games[g] = []
        tree = ao.OracleTree(og)
        board, player, mc, start, mark = og.new_board(), 0, 0, 0, None
        for mv in range(moves):
            n = n_sims if cap is None or coin_full(seed, g, mv, cap[0]) else cap[1]
            tree.reset(player, mc)
            ao.mcts(og, tree, board, n, ev, draws[mv][0][g])
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
            never = resign is not None and never_resigns(seed, g, start, p_never)
            resigned = 0
            if resign is not None and winner == -2 and mc >= min_ply and q >= v:
                if not never:
                    winner, resigned = 1 - mover, 1
                elif mark is None:
                    mark = mover
            out.rec[(g, mv)] = (pi.tobytes(), float(q), int(cell), int(winner), resigned)
            if winner != -2:
                out.games[g].append((mc, int(winner), resigned, never, mark))
                if resign is not None:
                    out.stats[0] += resigned
                    out.stats[1] += int(never)
                    out.stats[2] += int(never and mark is not None)
                    out.stats[3] += int(never and mark is not None and winner != 1 - mark)
                board, player, mc, start, mark = og.new_board(), 0, 0, mv + 1, None
    return out


def lockstep_records(game, moves, seed=SEED, n_sims=N_SIMS, resign=(V, P_NEVER), n_games=G, **kw):
    """{(slot, move): (pi bytes, q, cell, winner, resigned)} of SelfPlayRunner(recycle=True), and the runner."""
    from selfplay import SelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        flags = r.record_resigned
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                assert int(d[g]) == int(int(w[g]) != -2)
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]), int(flags[g]))
    kw.setdefault("recycle", True)
    r = SelfPlayRunner(game, evaluator(A), n_games, n_sims, size=size, seed=seed, on_records=on, resign=resign, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_records(game, moves, seed=SEED, n_sims=N_SIMS, resign=(V, P_NEVER), n_games=G, **kw):
    from selfplay import AsyncSelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(meta, q, pi):
        flags = r.record_resigned if r.record_resigned is not None else np.zeros(len(meta), np.uint8)
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]), int(flags[i]))
    kw.setdefault("recycle", True)
    r = AsyncSelfPlayRunner(game, evaluator(A), n_games, n_sims, size=size, seed=seed, on_records=on, resign=resign, use_graph=False, **kw)
    for _ in range(8000):                                       # until EVERY slot has played `moves` moves (slots run at their own pace)
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(n_games)):
            break
    r.check_error()
    return rec, r


def assert_same_records(got, want, moves, tag=(), n_games=G, offset=0):
    for g in range(n_games):
        for mv in range(moves):
            assert got[(g, mv)] == want[(g + offset, mv)], tag + (g, mv)


def ring_rows(rp):
    """sha256 of every tuple in the ring, by slot."""
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    return [hashlib.sha256(s[i].tobytes() + p[i].tobytes() + z[i:i + 1].tobytes()).hexdigest() for i in range(rp.size())]


def gomoku_restated():
    return shared(("restated", "gomoku"), lambda: restate("gomoku", MOVES, engine_draws("gomoku", MOVES), (V, P_NEVER)))


def gomoku_lockstep():
    return shared(("lockstep", "gomoku", 64), lambda: lockstep_records("gomoku", MOVES, cache_entries=64)[0])


# ---------------------------------------------------------------------------------------------------
# 1. + 2. lock-step, eager, against the restatement; the statistics
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("game,moves,cache,resign", [("gomoku", MOVES, "off", (V, P_NEVER)), ("gomoku", MOVES, "per_game", (V, P_NEVER)),
                                                     ("gomoku", MOVES, "shared", (V, P_NEVER)), ("connect4", 30, "off", (V, P_NEVER)),
                                                     ("tictactoe", TTT_MOVES, "off", (TTT_V, P_NEVER, TTT_MIN_PLY))])
def test_lockstep_eager_equals_the_restatement(game, moves, cache, resign):
    draws = engine_draws(game, moves)
    want = gomoku_restated() if game == "gomoku" else shared(("restated", game), lambda: restate(game, moves, draws, resign))
    print(game, "restated kinds (resigned, natural, false-positive marks, true marks):", want.kinds(), "stats:", want.stats)
    # the preconditions, on the restatement alone
    if game == "gomoku":
        res, nat, fp, tp = want.kinds()
        assert res >= 2 and nat >= 2 and fp >= 1 and tp >= 1, want.kinds()
    elif game == "tictactoe":                                     # min_ply changes at least one game
        free = shared(("restated", game, "min_ply 0"), lambda: restate(game, moves, draws, resign[:2]))
        print("tictactoe resigned with min_ply 4 / 0:", want.stats[0], free.stats[0])
        assert want.stats[0] > 0 and want.rec != free.rec
        assert all(x[0] >= TTT_MIN_PLY for gs in want.games.values() for x in gs if x[2])
        assert any(x[0] < TTT_MIN_PLY for gs in free.games.values() for x in gs if x[2])
    else:
        assert want.stats[0] > 0
    kw = dict(off={}, per_game=dict(cache_entries=64), shared=dict(cache_entries=64, cache_shared=True))[cache]
    got, r = lockstep_records(game, moves, resign=resign, **kw)
    assert_same_records(got, want.rec, moves, (game, cache))
    assert r.resign_stats() == want.stats                         # 2. the four counts
    assert r.games_finished == sum(len(gs) for gs in want.games.values()) > 0
    assert r.finished_plies == sum(x[0] for gs in want.games.values() for x in gs)      # plies emitted per game stay move_count


# ---------------------------------------------------------------------------------------------------
# 3. the graph runner, 4. sharding
# ---------------------------------------------------------------------------------------------------
@gpu
def test_graph_runner_equals_eager():
    want = gomoku_lockstep()
    got, r = lockstep_records("gomoku", MOVES, cache_entries=64, use_graph=True, steps_per_graph=4)
    assert_same_records(got, want, MOVES)
    assert r.resign_stats() == gomoku_restated().stats


@gpu
def test_a_shard_plays_its_slots_of_the_whole_run():
    """An engine of 3 slots with first_global_game = 5 plays slots 5..7 of the 8-slot run: the game coins do not depend on the sharding."""
    whole = gomoku_restated()
    got, r = lockstep_records("gomoku", MOVES, n_games=3, first_global_game=5)
    assert_same_records(got, whole.rec, MOVES, n_games=3, offset=5)
    part = restate("gomoku", MOVES, engine_draws("gomoku", MOVES), (V, P_NEVER), slots=range(5, 8))
    assert r.resign_stats() == part.stats and sum(part.stats) > 0


# ---------------------------------------------------------------------------------------------------
# 5. degenerate settings
# ---------------------------------------------------------------------------------------------------
@gpu
def test_off_never_and_unreachable_threshold_are_the_runner_without_the_option():
    import azk
    rings = [azk.DeviceReplay(3000, 2, 7, 7, 49) for _ in range(3)]
    plain, _ = lockstep_records("gomoku", MOVES, resign=None, replay=rings[0])
    never, rn = lockstep_records("gomoku", MOVES, resign=(V, 1.0), replay=rings[1])
    high, rh = lockstep_records("gomoku", MOVES, resign=(1.0, 0.0), replay=rings[2])
    draws = engine_draws("gomoku", MOVES)
    off = restate("gomoku", MOVES, draws, None)
    assert_same_records(plain, off.rec, MOVES)                    # option off: the games of the restatement without the rule
    assert plain == never == high and not any(v[4] for v in plain.values())
    assert int(rings[0].cursor.item()) > 0
    for rp in rings[1:]:
        assert int(rp.cursor.item()) == int(rings[0].cursor.item())
        for a, b in ((rings[0].states, rp.states), (rings[0].pis, rp.pis), (rings[0].zs, rp.zs)):
            assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    want = restate("gomoku", MOVES, draws, (V, 1.0))
    assert want.stats[0] == 0 and want.stats[1] == sum(len(gs) for gs in want.games.values()) and want.stats[2] > 0
    assert rn.resign_stats() == want.stats
    # v_resign = 1.0: the q of these searches stays below 1, so nothing resigns and nothing is marked
    assert max(v[1] for v in plain.values()) < 1.0
    assert rh.resign_stats() == [0, 0, 0, 0]


# ---------------------------------------------------------------------------------------------------
# 6. emission, 10. self_play_batch and collect_data
# ---------------------------------------------------------------------------------------------------
def batch_restated():
    return shared(("restated", "gomoku", 49), lambda: restate("gomoku", 49, engine_draws("gomoku", 49), (V, P_NEVER)))


@gpu
@pytest.mark.parametrize("capacity", [4096, 97])
def test_emission_is_the_oracle_emission_fed_the_resigned_winners(capacity):
    """self_play_batch(resign=...): every game is the restatement's first game of its slot - plies, pi, winner, resigned - and its tuples are
    oracle.replay_oracle.emit_tuples(boards, pis, the restated winner), from the game's first stream index on; slot t % capacity holds tuple t
    (97: the ring wraps)."""
    import azk
    from oracle import replay_oracle as ro
    from selfplay import self_play_batch
    want = batch_restated()
    rp = azk.DeviceReplay(capacity, 2, 7, 7, 49)
    res = self_play_batch("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, replay=rp, resign=(V, P_NEVER))
    stream, total = {}, 0
    for g, r in enumerate(res):
        plies, winner, resigned, _, _ = want.games[g][0]
        assert (len(r.pis), r.winner, r.resigned) == (plies, winner, bool(resigned)), g
        for i in range(plies):
            assert (r.pis[i].tobytes(), r.qs[i], r.cells[i]) == want.rec[(g, i)][:3], (g, i)
        if resigned:                                              # z of a resigned game: by the side that did not concede
            assert winner == 1 - ((plies - 1) & 1)
        tuples = ro.emit_tuples(r.boards, r.pis, winner)
        assert len(tuples) == (plies if plies <= 2 else 2 + 8 * (plies - 2))
        for k, t in enumerate(tuples):
            assert r.replay_base + k not in stream
            stream[r.replay_base + k] = t
        total += len(tuples)
    assert any(r.resigned for r in res) and not all(r.resigned for r in res)
    assert int(rp.cursor.item()) == total == len(stream) and sorted(stream) == list(range(total)) and rp.size() == min(total, capacity)
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    for t in range(max(0, total - capacity), total):
        st, pi, zz = stream[t]
        slot = t % capacity
        assert s[slot].tobytes() == np.ascontiguousarray(st, np.float32).tobytes() and p[slot].tobytes() == np.ascontiguousarray(pi, np.float64).tobytes(), t
        assert float(z[slot]) == zz, t


@gpu
def test_collect_data_fills_both_buffer_kinds_alike():
    """train.collect_data(..., resign=...): a host buffer (save_data_to_buffer with the resigned winners) and a DeviceReplay (the engine's
    emission) receive the same tuples, and fewer of them than without the option."""
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
    want = batch_restated()
    dev_buf, host_buf, plain = azk.DeviceReplay(8192, 2, 7, 7, 49), HostBuffer(), HostBuffer()
    r1 = az_train.collect_data(Gomoku, FixtureModel(49), dev_buf, G, N_SIMS, seed=SEED, resign=(V, P_NEVER))
    r2 = az_train.collect_data(Gomoku, FixtureModel(49), host_buf, G, N_SIMS, seed=SEED, resign=(V, P_NEVER))
    az_train.collect_data(Gomoku, FixtureModel(49), plain, G, N_SIMS, seed=SEED)
    winners = [want.games[g][0][1] for g in range(G)]
    assert r1 == r2 == [winners.count(0), winners.count(1), winners.count(-1)]
    keyed = lambda items: sorted((s.tobytes(), p.tobytes(), float(z[0])) for s, p, z in items)
    assert 0 < dev_buf.size() == len(host_buf.buffer) < len(plain.buffer) and keyed(dev_buf.to_reference_deque()) == keyed(host_buf.buffer)


# ---------------------------------------------------------------------------------------------------
# 7. the asynchronous movers play the lock-step games, 8. with tree reuse
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("per_launch", [1, 2, 3])
def test_async_equals_lockstep_slot_for_slot(per_launch):
    want = gomoku_lockstep()
    got, r = async_records("gomoku", MOVES, cache_entries=64, per_launch=per_launch, steps_per_graph=4)
    assert_same_records(got, want, MOVES, (per_launch,))
    st, rs = r.finish(), r.resign_stats()
    assert int(st[0]) > 0 and int(st[5]) == len(got)
    # the statistics are the movers' own: every resignation among the records, at least the lock-step run's counts (slots may be further on)
    assert rs[0] == sum(v[4] for v in got.values()) > 0
    assert all(a >= b for a, b in zip(rs, gomoku_restated().stats)) and rs[1] >= rs[2] >= rs[3]


@gpu
def test_async_replay_equals_lockstep_as_a_multiset():
    """Games played to the end without restarts: the drain's emission holds the tuples of the lock-step runner's (the stream order follows
    the finishing order), and the statistics agree."""
    import azk
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner
    ra, rb = azk.DeviceReplay(4096, 2, 7, 7, 49), azk.DeviceReplay(4096, 2, 7, 7, 49)
    r = SelfPlayRunner("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, recycle=False, replay=ra, resign=(V, P_NEVER))
    for _ in range(49):
        r.play_move()
    r.check_error()
    a = AsyncSelfPlayRunner("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, recycle=False, replay=rb, per_launch=2, steps_per_graph=4,
                            use_graph=False, resign=(V, P_NEVER))
    for _ in range(3000):
        a.run_chunk()
        if int(a.finish()[0]) == G:
            break
    a.check_error()
    assert int(a.finish()[0]) == G
    assert 0 < ra.size() == rb.size() == int(rb.cursor.item()) and sorted(ring_rows(ra)) == sorted(ring_rows(rb))
    want = batch_restated()
    first = [want.games[g][0] for g in range(G)]
    stats = [sum(x[2] for x in first), sum(x[3] for x in first), sum(x[3] and x[4] is not None for x in first),
             sum(x[3] and x[4] is not None and x[1] != 1 - x[4] for x in first)]
    assert r.resign_stats() == a.resign_stats() == stats and stats[0] > 0


@gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_async_reroot_equals_lockstep_tree_reuse(mode):
    want, lr = lockstep_records("gomoku", MOVES, cache_entries=64, tree_reuse=mode)
    got, r = async_records("gomoku", MOVES, cache_entries=64, per_launch=2, steps_per_graph=4, reroot=mode)
    flags = [v[4] for v in want.values()]
    assert 0 < sum(flags) and lr.games_finished > sum(flags)      # resignations and natural ends
    assert_same_records(got, want, MOVES, (mode,))
    assert lr.counters()["roots_reused"] > 0 and r.counters()["roots_reused"] > 0
    assert r.resign_stats()[0] == sum(v[4] for v in got.values()) >= lr.resign_stats()[0] == sum(flags)


# ---------------------------------------------------------------------------------------------------
# 9. with a playout cap
# ---------------------------------------------------------------------------------------------------
@gpu
def test_with_a_playout_cap_lockstep_equals_the_restatement_and_async_equals_lockstep():
    want = restate("gomoku", MOVES, engine_draws("gomoku", MOVES), (V, P_NEVER), cap=CAP)
    print("capped restated kinds:", want.kinds(), "stats:", want.stats)
    assert want.stats[0] > 0 and want.kinds()[1] > 0
    got, r = lockstep_records("gomoku", MOVES, playout_cap=CAP)
    assert_same_records(got, want.rec, MOVES, ("cap",))
    assert r.resign_stats() == want.stats
    agot, ar = async_records("gomoku", MOVES, playout_cap=CAP, per_launch=2, steps_per_graph=4)
    assert_same_records(agot, got, MOVES, ("cap", "async"))
    assert ar.resign_stats()[0] == sum(v[4] for v in agot.values())


# ---------------------------------------------------------------------------------------------------
# 11. refusals
# ---------------------------------------------------------------------------------------------------
@gpu
def test_refusals():
    import azk
    e = azk.Engine("gomoku", 2, N_SIMS, size=7)
    for v, p, m in ((-0.1, 0.5, 0), (1.5, 0.5, 0), (float("nan"), 0.5, 0), (0.25, -0.1, 0), (0.25, 1.5, 0), (0.25, float("nan"), 0), (0.25, 0.5, -1)):
        with pytest.raises(azk.AzkError, match="-1"):
            e.set_resign(v, p, m)
        assert e.resign is None
    for call in (e.resigned, e.resign_stats):
        with pytest.raises(azk.AzkError):
            call()                                               # no resignation set
    vl = azk.Engine("gomoku", 2, N_SIMS, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="-1"):
        vl.set_resign(V, P_NEVER)
    assert "leaves_per_step" in vl.L.azk_last_error(vl.h).decode()
    e.reset_games()
    e.search(evaluator(49), N_SIMS)
    with pytest.raises(azk.AzkError, match="-4"):
        e._chk(e.L.azk_advance_resign(e.h, None, 0, 0, None, None, None, None))      # azk_advance_resign while the option is not set
    e.set_resign(V, P_NEVER, 0, SEED, 0)
    with pytest.raises(azk.AzkError, match="-4"):
        e.advance(None, 0)                                       # plain azk_advance while the option is set
    with pytest.raises(azk.AzkError, match="-1"):
        e._chk(e.L.azk_advance_resign(e.h, None, 0, -1, None, None, None, None))
    e.advance(None, 0, move_index=0)
    assert e.resigned().cpu().numpy().tolist() == [0, 0] and e.resign_stats() == [0, 0, 0, 0]
    e.set_resign(0.0)                                            # off again: the plain entry point is back
    assert e.resign is None
    e.search(evaluator(49), N_SIMS)
    e.advance(None, 0)
    e.check_error()
