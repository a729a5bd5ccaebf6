"""Random openings (azk_set_openings) on the GPU, against the plain-Python restatement (tests/openings_restated.py: its own
Philox, the oracle's rule primitives; the engine's flags are never the checker): the kernel alone on every board shape, p_open = 0 against the
option off, the lock-step runner with recycling against the oracle's searches from the restated positions, emission, the asynchronous movers
against the lock-step runner, resignation with openings, the arena's paired openings."""
import hashlib

import numpy as np
import pytest

import openings_restated as R
from fixture_eval import fixture_logits_value
from test_openings_restated import C4_MID, EDGE_FIRST, EDGE_SEED, KEYS, SEED as OSEED, SLOTS, TTT

gpu = pytest.mark.gpu

G, N_SIMS, SEED = 8, 24, 6
OPEN = (0.75, 6, 1)                                              # the runners' openings: three games in four, up to six plies, the 3 x 3 centre
GAMES = {"gomoku": (7, 49), "connect4": (None, 7), "tictactoe": (None, 9)}
MOVES = {"gomoku": 50, "tictactoe": 20}                          # a game has at most state_dim plies: every slot restarts at least once
_shared = {}


def shared(key, make):
    """A reference computed once for the tests that need it; never modified afterwards."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_draws(game, moves, seed=SEED):
    def make():
        import azk
        eng = azk.Engine(game, G, N_SIMS, size=GAMES[game][0])
        return [(nz.cpu().numpy(), u.cpu().numpy()) for nz, u in (eng.gen_noise(seed, 0, mv) for mv in range(moves))]
    return shared(("draws", game, moves, seed), make)


# ---------------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------------
KERNEL_CASES = [
    ("tictactoe", None, TTT, OSEED, 0),
    ("connect4", None, C4_MID, OSEED, 0),
    ("connect4", None, (0.75, 12, 1), OSEED, 0),
    ("gomoku", 7, (0.75, 9, 1), OSEED, 0),
    ("gomoku", 7, (0.75, 9, 1), EDGE_SEED, EDGE_FIRST),           # the edge seed and a first game that straddles the word boundary
    ("gomoku", 15, (0.75, 24, 2), OSEED, 0),                      # 225 cells: more than one 64-lane group of cells
    ("gomoku", 20, (0.75, 40, -1), OSEED, 0),                     # two dword passes, 400 candidates
    ("gomoku", (5, 9), (0.75, 8, 1), OSEED, 0),                   # the window per axis: odd x odd, 3 x 3 of 5 x 9
    ("gomoku", (9, 5), (0.75, 8, 1), OSEED, 0),
    ("gomoku", (4, 6), (0.75, 8, 1), OSEED, 0),                   # even extents: 2 x 2
    ("gomoku", (4, 4), (1.0, 3, 0), OSEED, 0),                    # an empty window: opened, no ply
    ("gomoku", (1, 3), (1.0, 2, -1), OSEED, 0),
    ("gomoku", (2, 2), (1.0, 3, -1), OSEED, 0),
]


@gpu
@pytest.mark.parametrize("game,size,openings,seed,first", KERNEL_CASES)
def test_kernel_alone_equals_the_restatement(game, size, openings, seed, first):
    import azk
    from oracle import az_oracle as ao
    og = ao.OracleGame(game, size)
    eng = azk.Engine(game, SLOTS, 8, size=size)
    eng.set_openings(*openings, seed=seed, first_global_game=first)
    assert eng.opening_stats() == [0, 0, 0]
    opens = []
    for key in KEYS:
        eng.reset_games()
        eng.open_pending(key)
        cells, to_move, mc = eng.get_positions()
        plies = eng.open_plies().cpu().numpy()
        want = [R.open_game(og, seed, first + g, key, openings) for g in range(SLOTS)]
        for g, o in enumerate(want):
            assert cells[g].tobytes() == o.codes().tobytes(), (key, g, o.cells)
            assert (int(to_move[g]), int(mc[g]), int(plies[g])) == (o.player, o.plies, o.plies), (key, g)
        opens += want
        eng.open_pending(key + 1)                                 # nothing is pending any more: a second call opens nothing
        assert eng.get_positions()[0].tobytes() == cells.tobytes()
    print(game, size, openings, "restated [opened, plies, cut short]:", R.stats_of(opens), "ended without a candidate:",
          sum(o.ended_empty for o in opens))
    assert eng.opening_stats() == R.stats_of(opens)
    eng.check_error()
    if openings[0] < 1.0:
        assert any(o.opened for o in opens) and not all(o.opened for o in opens)
    if openings == (1.0, 3, 0):
        assert all(o.opened and o.plies == 0 for o in opens)


# ---------------------------------------------------------------------------------------------------
# the runners: records, the restatement around the oracle's searches
# ---------------------------------------------------------------------------------------------------
def lockstep_records(game, moves, openings=OPEN, n_games=G, replay=None, **kw):
    """{(slot, move): (pi bytes, q, cell, winner)} of SelfPlayRunner(recycle=True), the runner, and the first games' positions."""
    from selfplay import SelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]))
    kw.setdefault("recycle", True)
    r = SelfPlayRunner(game, evaluator(A), n_games, N_SIMS, size=size, seed=SEED, on_records=on, replay=replay, openings=openings,
                       openings_seed=OSEED if openings is not None else None, **kw)
    start = r.eng.get_positions()
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r, start


def ring_rows(rp):
    """sha256 of every tuple in a ring that has not wrapped, in stream order."""
    n = int(rp.cursor.item())
    assert 0 < n <= rp.size()
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    return [hashlib.sha256(s[i].tobytes() + p[i].tobytes() + z[i:i + 1].tobytes()).hexdigest() for i in range(n)]


def async_records(game, moves, openings=OPEN, n_games=G, **kw):
    from selfplay import AsyncSelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(meta, q, pi):
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]))
    r = AsyncSelfPlayRunner(game, evaluator(A), n_games, N_SIMS, size=size, seed=SEED, on_records=on, use_graph=False, openings=openings,
                            openings_seed=OSEED, **kw)
    for _ in range(8000):                                         # until EVERY slot has played `moves` moves (slots run at their own pace)
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(n_games)):
            break
    r.check_error()
    return rec, r


class Restated:
    def __init__(self):
        self.rec, self.games, self.opens, self.resign_stats = {}, {}, [], [0, 0, 0, 0]


def restate(game, moves, openings=OPEN, resign=None):
    """Every slot's games through the oracle's primitives in a loop shaped like <Game>.self_play: a game that starts under move key k starts
    from open_game(..., k, ...); every searched move is the oracle's search from there.  resign = (v, p_never): the rule of DESIGN section 19
    with the game coin at start = (key of the game's first search) - (its opening's plies)."""
    import torch
    from oracle import az_oracle as ao
    from selfplay import SAMPLE_UNTIL
    from test_gpu_resign import never_resigns
    size, A = GAMES[game]
    og = ao.OracleGame(game, size)
    draws = engine_draws(game, moves)

    def ev(canon):
        logits, val = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], A, "hash")
        return ao.softmax_det(logits[0].numpy()), float(val[0])
    out = Restated()
    for g in range(G):
        out.games[g] = []
        tree = ao.OracleTree(og)

        def begin(key):
            o = R.open_game(og, OSEED, g, key, openings) if openings is not None else R.open_game(og, OSEED, g, key, (0.0, 1, -1))
            out.opens.append(o)
            return o.board.copy(), o.player, o.plies, o, (key - o.plies) & R.M32      # (the game plays on a copy: o stays the start)
        board, player, mc, o, start = begin(0)
        mark = None
        for mv in range(moves):
            tree.reset(player, mc)
            ao.mcts(og, tree, board, N_SIMS, ev, draws[mv][0][g])
            pi = tree.pi()
            q = tree.root_value / tree.root_visit
            cell = tree.cell_for_action(ao.sample_action(pi, draws[mv][1][g])) if mc < SAMPLE_UNTIL[game] else tree.max_visit_cell()
            mover = player
            player = og.make_move(board, player, og.rc(cell))
            mc += 1
            w = og.check_winner(board, mover, og.rc(cell))
            winner = w if w != -1 else (-1 if mc == og.state_dim else -2)
            never = resign is not None and never_resigns(SEED, g, start, resign[1])
            resigned = 0
            if resign is not None and winner == -2 and q >= resign[0]:
                if not never:
                    winner, resigned = 1 - mover, 1
                elif mark is None:
                    mark = mover
            out.rec[(g, mv)] = (pi.tobytes(), float(q), int(cell), int(winner))
            if winner != -2:
                out.games[g].append((mc, int(winner), o.plies))
                if resign is not None:
                    for i, hit in enumerate((resigned, never, never and mark is not None, never and mark is not None and winner != 1 - mark)):
                        out.resign_stats[i] += int(bool(hit))
                board, player, mc, o, start = begin(mv + 1)
                mark = None
    return out


def assert_same_records(got, want, moves, tag=()):
    for g in range(G):
        for mv in range(moves):
            assert got[(g, mv)] == want[(g, mv)], tag + (g, mv)


# ---------------------------------------------------------------------------------------------------
# 2. p_open = 0 is the option off
# ---------------------------------------------------------------------------------------------------
@gpu
def test_p_open_zero_is_the_runner_without_the_option():
    import azk
    rings = [azk.DeviceReplay(3000, 2, 7, 7, 49) for _ in range(2)]
    off, r0, _ = lockstep_records("gomoku", 12, openings=None, replay=rings[0])
    zero, r1, _ = lockstep_records("gomoku", 12, openings=(0.0, 6, 1), replay=rings[1])
    assert off == zero and len(off) == 12 * G
    assert r1.eng.opening_stats() == [0, 0, 0]
    assert int(rings[0].cursor.item()) == int(rings[1].cursor.item())
    for a, b in ((rings[0].states, rings[1].states), (rings[0].pis, rings[1].pis), (rings[0].zs, rings[1].zs)):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------
# 3. the lock-step runner with recycling
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("game", ["gomoku", "tictactoe"])
def test_lockstep_with_recycling_equals_the_restatement(game):
    moves = MOVES[game]
    openings = OPEN if game == "gomoku" else (0.75, 5, -1)
    want = shared(("restated", game), lambda: restate(game, moves, openings))
    print(game, "games per slot:", [len(want.games[g]) for g in range(G)], "openings [opened, plies, cut short]:", R.stats_of(want.opens))
    assert all(len(want.games[g]) >= 1 for g in range(G))         # the precondition: every slot restarts at least once
    assert sum(1 for o in want.opens[G:] if o.plies) >= 2         # ... and restarted games are opened too
    got, r, start = shared(("lockstep", game), lambda: lockstep_records(game, moves, openings))
    for g in range(G):                                            # the first games' positions
        o = want.opens[sum(len(want.games[k]) + 1 for k in range(g))]       # (a slot's openings: one per game that ended, and the one running)
        assert start[0][g].tobytes() == o.codes().tobytes() and (int(start[1][g]), int(start[2][g])) == (o.player, o.plies), g
    assert_same_records(got, want.rec, moves, (game,))
    assert r.eng.opening_stats() == R.stats_of(want.opens)
    assert r.games_finished == sum(len(gs) for gs in want.games.values())
    assert r.finished_plies == sum(x[0] for gs in want.games.values() for x in gs)     # stats[1] counts the opening's plies too
    assert r.plies_played == moves * G                            # searched moves only


@gpu
def test_graph_runner_equals_eager():
    want = shared(("lockstep", "gomoku"), lambda: lockstep_records("gomoku", MOVES["gomoku"], OPEN))[0]
    got, r, _ = lockstep_records("gomoku", MOVES["gomoku"], OPEN, use_graph=True, steps_per_graph=4)
    assert_same_records(got, want, MOVES["gomoku"])


# ---------------------------------------------------------------------------------------------------
# 4. emission
# ---------------------------------------------------------------------------------------------------
def expected_tuples(game, og, r, o, elements, full=None, copies=None):
    """One finished game's tuples in ring order: the full trajectory's groups with the opening's plies left out and ply indices kept -
    emission_restated's canonical / turn; plies 0 and 1 once, later ones once per element; a ply's group `copies` times, copy-major."""
    import emission_restated as E
    reward = 0 if r.winner == -1 else 1
    out = []
    for k, (b, p) in enumerate(zip(r.boards, r.pis)):
        i = o.plies + k                                           # the absolute ply
        if full is not None and not full[k]:
            continue
        side = i & 1
        z = float(reward if side == r.winner else -reward)
        group = [E.turn(E.canonical(b, side), p, s, game) + (z,) for s in ((0,) if i < 2 else elements)]
        out += group * (1 if copies is None else int(copies[k]))
    return out


@gpu
@pytest.mark.parametrize("variant", ["plain", "connect4_board", "playout_cap", "surprise"])
def test_emission_leaves_the_opening_out_and_keeps_ply_indices(variant):
    import azk
    from oracle import az_oracle as ao
    from selfplay import self_play_batch, surprise_copies
    game = "connect4" if variant == "connect4_board" else "gomoku"
    size, A = GAMES[game]
    og = ao.OracleGame(game, size)
    openings = (0.75, 6, 1)
    kw = dict(connect4_board=dict(emit_symmetry="board"), playout_cap=dict(playout_cap=(0.5, 6)), surprise=dict(surprise_weight=0.5), plain={})[variant]
    elements = (0, 1) if game == "connect4" else tuple(range(8))
    rp = azk.DeviceReplay(8192, og.planes, og.rows, og.cols, A)
    res = self_play_batch(game, evaluator(A), G, N_SIMS, size=size, seed=SEED, replay=rp, openings=openings, openings_seed=OSEED, **kw)
    stream, total = {}, 0
    opens = [R.open_game(og, OSEED, g, 0, openings) for g in range(G)]
    assert any(o.plies >= 3 for o in opens) and any(o.plies == 1 for o in opens) and any(o.plies == 0 for o in opens), [o.plies for o in opens]
    for g, (r, o) in enumerate(zip(res, opens)):
        assert r.open_plies == o.plies and r.boards[0].tobytes() == o.board.tobytes(), g      # the game starts from the restated position
        assert r.opening == o.cells, g                                                          # ... reached by the restated plies, in order
        assert len(r.pis) + o.plies <= og.state_dim
        full = r.full if variant == "playout_cap" else None
        copies = surprise_copies(r.kl, r.coin, 0.5) if variant == "surprise" else None          # n_F and S over the searched plies alone
        tuples = expected_tuples(game, og, r, o, elements, full, copies)
        for k, t in enumerate(tuples):
            assert r.replay_base + k not in stream
            stream[r.replay_base + k] = t
        total += len(tuples)
    if variant == "surprise":
        assert any(int(c) != 1 for r in res for c in surprise_copies(r.kl, r.coin, 0.5))
    if variant == "playout_cap":
        assert any(not f for r in res for f in r.full) and any(f for r in res for f in r.full)
    assert int(rp.cursor.item()) == total == len(stream) and sorted(stream) == list(range(total)) and total <= 8192
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    for t in range(total):
        st, pi, zz = stream[t]
        assert s[t].tobytes() == np.ascontiguousarray(st, np.float32).tobytes(), (variant, t)
        assert p[t].tobytes() == np.ascontiguousarray(pi, np.float64).tobytes() and float(z[t]) == zz, (variant, t)


@gpu
def test_host_buffer_gets_the_tuples_of_the_device_ring():
    """train.collect_data(openings=...): save_data_to_buffer(first_ply=open_plies) puts into a host buffer what the engine emits."""
    import azk
    import train as az_train
    from fixture_eval import FixtureModel
    from games import Gomoku
    Gomoku.rows = Gomoku.cols = 7
    Gomoku.action_dim = Gomoku.state_dim = 49

    class HostBuffer:
        def __init__(self):
            self.rows = []

        def add(self, s, p, r):
            self.rows.append(hashlib.sha256(np.ascontiguousarray(s, np.float32).tobytes() + np.ascontiguousarray(p, np.float64).tobytes()
                                            + np.float32(r[0]).tobytes()).hexdigest())
    model = FixtureModel(49, "hash")
    host, ring = HostBuffer(), azk.DeviceReplay(8192, 2, 7, 7, 49)
    a = az_train.collect_data(Gomoku, model, host, G, N_SIMS, seed=SEED, openings=(1.0, 6, 1))
    b = az_train.collect_data(Gomoku, model, ring, G, N_SIMS, seed=SEED, openings=(1.0, 6, 1))
    assert a == b
    n = int(ring.cursor.item())
    s, p, z = ring.states.cpu().numpy(), ring.pis.cpu().numpy(), ring.zs.cpu().numpy()
    dev = [hashlib.sha256(s[i].tobytes() + p[i].tobytes() + z[i:i + 1].tobytes()).hexdigest() for i in range(n)]
    assert n == len(host.rows) > 0 and sorted(dev) == sorted(host.rows)


# ---------------------------------------------------------------------------------------------------
# 5. the asynchronous movers
# ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("reroot", [0, 2])
def test_async_movers_play_the_lockstep_games(reroot):
    moves = 30
    import azk
    from collections import Counter
    rings = [azk.DeviceReplay(16384, 2, 7, 7, 49) for _ in range(2)]
    want, rl, _ = lockstep_records("gomoku", moves, OPEN, tree_reuse=reroot, cache_entries=64, replay=rings[0])
    got, ra = async_records("gomoku", moves, OPEN, reroot=reroot, cache_entries=64, per_launch=2, steps_per_graph=4, replay=rings[1])
    assert_same_records(got, want, moves, (reroot,))
    # the drained ring: the slots run at their own pace, so the asynchronous ring holds the lock-step run's games and those the faster slots
    # went on to finish - every tuple of the lock-step ring is in it, as often
    lock_rows, async_rows = ring_rows(rings[0]), ring_rows(rings[1])
    missing = Counter(lock_rows) - Counter(async_rows)
    assert not missing, sum(missing.values())
    # ... and each ring holds exactly the tuples of the games its records show as ended: per game 8 per ply from the third on, one for plies
    # 0 and 1, less the groups of the restated opening's plies.  So the asynchronous ring is the lock-step ring plus the tuples of the
    # games that ended after the window, no more and no fewer
    from oracle import az_oracle as ao
    og = ao.OracleGame("gomoku", 7)
    count = lambda x: x if x <= 2 else 2 + 8 * (x - 2)

    def ended_games(rec):
        """(slot, move of the last ply, tuples) of every game the records show as ended."""
        out = []
        for g in range(G):
            start, mv = 0, 0
            while (g, mv) in rec:
                if rec[(g, mv)][3] != -2:
                    o = R.open_game(og, OSEED, g, start, OPEN).plies
                    out.append((g, mv, count(o + mv - start + 1) - count(o)))
                    start = mv + 1
                mv += 1
        return out
    in_window = [x for x in ended_games(got) if x[1] < moves]
    assert in_window == ended_games(want)
    assert len(lock_rows) == sum(x[2] for x in in_window) and len(async_rows) == sum(x[2] for x in ended_games(got))
    assert any(v[3] != -2 for (g, mv), v in want.items() if mv < moves - 1)     # games ended and restarted inside the window
    stats = ra.eng.opening_stats()
    assert stats[0] > G // 2 and stats[1] >= stats[0] - stats[2]


# ---------------------------------------------------------------------------------------------------
# 6. resignation with openings
# ---------------------------------------------------------------------------------------------------
@gpu
def test_resignation_with_openings():
    moves, resign = 40, (0.25, 0.5)
    want = restate("gomoku", moves, OPEN, resign)
    print("restated resign stats:", want.resign_stats, "games:", sum(len(gs) for gs in want.games.values()))
    assert want.resign_stats[0] >= 1 and want.resign_stats[1] >= 1
    got, r, _ = lockstep_records("gomoku", moves, OPEN, resign=resign)
    assert_same_records(got, want.rec, moves)
    assert r.resign_stats() == want.resign_stats


# ---------------------------------------------------------------------------------------------------
# 7. the arena
# ---------------------------------------------------------------------------------------------------
@gpu
def test_arena_pairs_share_an_opening_and_equal_the_oracle():
    """compare(openings=...): game i of the second half starts from the position game i of the first half started from - the restatement's, at
    the openings' own first game index - with the models swapped, and every game is the oracle's alternating-model game from there."""
    import arena
    import azk
    import torch
    from oracle import az_oracle as ao
    N, iters, aseed, opn = 16, N_SIMS, 9, (6, 1)
    half, A = N // 2, 49
    og = ao.OracleGame("gomoku", 7)
    models = {v: (lambda x, v=v: fixture_logits_value(x, A, v)) for v in ("hash", "uniform")}

    def oracle_ev(variant):
        def ev(canon):
            logits, val = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], A, variant)
            return ao.softmax_det(logits[0].numpy()), float(val[0])
        return ev

    def oracle_half(pair, first):
        """winners of `half` games: player p is model pair[p]; noise rows and uniforms keyed (aseed, first + g, searched move)."""
        eng = azk.Engine("gomoku", half, iters, size=7)
        draws = [(nz.cpu().numpy(), u.cpu().numpy()) for nz, u in (eng.gen_noise(aseed, first, mv) for mv in range(49))]
        evs, winners = [oracle_ev(v) for v in pair], []
        for g in range(half):
            o = R.open_game(og, aseed, g, 0, (1.0,) + opn)           # the openings' first game index is 0 in both halves
            board, player, mc, tree = o.board.copy(), o.player, o.plies, ao.OracleTree(og)
            for mv in range(49):
                tree.reset(player, mc)
                ao.mcts(og, tree, board, iters, evs[player], draws[mv][0][g])
                cell = tree.cell_for_action(ao.sample_action(tree.pi(), draws[mv][1][g])) if mc < 20 else tree.max_visit_cell()
                mover = player
                player = og.make_move(board, player, og.rc(cell))
                mc += 1
                w = og.check_winner(board, mover, og.rc(cell))
                if w != -1 or mc == og.state_dim:
                    winners.append(int(w))
                    break
        return winners
    opens = [R.open_game(og, aseed, g, 0, (1.0,) + opn) for g in range(half)]
    assert len({o.plies & 1 for o in opens}) == 2                   # the precondition: games of one batch start with either side to move
    w1, r1 = arena.compete_batch("gomoku", models["hash"], models["uniform"], half, iters, iters, True, 7, aseed, 0, openings=opn, openings_first_game=0)
    w2, r2 = arena.compete_batch("gomoku", models["uniform"], models["hash"], half, iters, iters, True, 7, aseed, half, openings=opn, openings_first_game=0)
    for g, o in enumerate(opens):                                   # every pair: one opening, the restatement's
        assert r1[g].opening == o.cells == r2[g].opening and r1[g].open_plies == o.plies == r2[g].open_plies, g
        assert r1[g].boards[0].tobytes() == o.board.tobytes() == r2[g].boards[0].tobytes(), g
    want1, want2 = oracle_half(("hash", "uniform"), 0), oracle_half(("uniform", "hash"), half)
    print("arena winners, first half:", want1, "second half:", want2)
    assert [int(w) for w in w1] == want1 and [int(w) for w in w2] == want2
    score = arena.compare("gomoku", models["hash"], models["uniform"], iters, iters, N, True, False, size=7, seed=aseed, openings=opn)
    assert score == arena.score_like_reference(want1, want2, N, False)
