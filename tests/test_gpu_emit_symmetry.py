"""(state, pi, z) emission under a mask of D4 elements on the GPU (azk_config.emit_elements): the option against an engine
without it on square boards, and on the geometries the reference's rule refuses - Connect4, non-square and tiny Gomoku - against the numpy
restatement (tests/emission_restated.py) applied to the engine's own game record.  Every comparison is exact."""
import functools

import numpy as np
import pytest
import torch

import emission_restated as er
from fixture_eval import fixture_logits_value

pytestmark = pytest.mark.gpu

G, SIMS = 4, 16
GEOM = {"connect4": (3, 6, 7, 7), "tictactoe": (3, 3, 3, 9)}


def geometry(game, size):
    if game != "gomoku":
        return GEOM[game]
    rows, cols = size if isinstance(size, tuple) else (size, size)
    return 2, rows, cols, rows * cols


def elements_of(game, size, emit):
    from selfplay import check_emit_symmetry, mask_elements
    return mask_elements(check_emit_symmetry(emit, game, size))


def new_ring(game, size, capacity, start=0):
    import azk
    planes, rows, cols, A = geometry(game, size)
    rp = azk.DeviceReplay(capacity, planes, rows, cols, A)
    rp.states.fill_(-5.0); rp.pis.fill_(-3.0); rp.zs.fill_(7.0)      # sentinels: no tuple holds them
    rp.cursor.fill_(start)
    return rp


def ring_numpy(rp):
    return rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()


@functools.lru_cache(maxsize=None)
def play(game, size, emit, seed, capacity=None, start=0, playout_cap=None, forced_playouts=None):
    """One batch of G games to the end with the ring attached -> (results, ring as numpy, cursor)."""
    from selfplay import self_play_batch
    planes, rows, cols, A = geometry(game, size)
    n = max(1, len(elements_of(game, size, emit)) if emit is not None else 8)
    capacity = capacity or G * er.count_tuples(rows * cols, n) + 16
    rp = new_ring(game, size, capacity, start)
    res = self_play_batch(game, lambda x: fixture_logits_value(x, A, "hash"), G, SIMS, size=size, seed=seed, replay=rp, emit_symmetry=emit,
                          playout_cap=playout_cap, forced_playouts=forced_playouts)
    return res, ring_numpy(rp), int(rp.cursor.item())


def expected_stream(game, size, emit, res, start=0, capped=False):
    """{stream index: tuple} over every game's block, from the engine's own records; and the stream's end."""
    els = elements_of(game, size, emit)
    stream, total = {}, 0
    for r in res:
        want = er.emit_tuples("connect4" if game == "connect4" else "gomoku", r.boards, r.pis, r.winner, els, full=r.full if capped else None)
        if not capped:
            assert len(want) == er.count_tuples(len(r.boards), len(els))
        for t, tup in enumerate(want):
            assert r.replay_base + t not in stream
            stream[r.replay_base + t] = tup
        total += len(want)
    assert sorted(stream) == list(range(start, start + total))       # the blocks tile the stream
    return stream, start + total


def assert_ring(ring, cursor, stream, end, capacity, start=0):
    states, pis, zs = ring
    assert cursor == end
    live = {t % capacity: t for t in range(max(start, end - capacity), end)}       # deque(maxlen): the newest `capacity` tuples
    for slot in range(capacity):
        if slot in live:
            st, pi, z = stream[live[slot]]
            assert states[slot].dtype == np.float32 and np.array_equal(states[slot], st) and np.array_equal(pis[slot], pi) and float(zs[slot]) == z, live[slot]
        else:
            assert np.all(states[slot] == -5.0) and np.all(pis[slot] == -3.0) and zs[slot] == 7.0, slot


# ---- 1. the option with every element equals the engine without it, on the boards the reference's rule emits ----------------------
@pytest.mark.parametrize("game,size", [("gomoku", 7), ("tictactoe", None)])
def test_board_mask_on_square_boards_is_the_reference_emission(game, size):
    res_on, ring_on, cur_on = play(game, size, "board", 11)
    res_off, ring_off, cur_off = play(game, size, None, 11)
    assert cur_on == cur_off > 0
    for a, b in zip(ring_on, ring_off):
        assert a.tobytes() == b.tobytes()
    assert [r.replay_base for r in res_on] == [r.replay_base for r in res_off] and all(r.replay_base is not None for r in res_on)
    stream, end = expected_stream(game, size, "board", res_on)         # ... which is the restatement's, too
    assert_ring(ring_on, cur_on, stream, end, len(ring_on[2]))


# ---- 2. / 3. the geometries the reference's rule refuses, and subset masks ----------------------------------------------------------------
NEW = [("connect4", None, "board", 0x03), ("gomoku", (5, 7), "board", 0x47), ("gomoku", (7, 5), "board", 0x47), ("gomoku", (3, 4), "board", 0x47),
       ("gomoku", 7, "none", 0x01), ("gomoku", (5, 7), (0, 6), 0x41)]


@pytest.mark.parametrize("game,size,emit,mask", NEW, ids=[f"{g}-{s}-{e}" for g, s, e, _ in NEW])
def test_emission_equals_the_restatement_on_the_engines_own_record(game, size, emit, mask):
    import azk
    res, ring, cursor = play(game, size, emit, 5)
    els = elements_of(game, size, emit)
    assert sum(1 << s for s in els) == mask
    stream, end = expected_stream(game, size, emit, res)
    assert end == sum(er.count_tuples(len(r.boards), len(els)) for r in res) < len(ring[2])
    assert_ring(ring, cursor, stream, end, len(ring[2]))
    if size == (3, 4):                                                  # no five in a row exists: twelve plies, a draw
        assert all(len(r.boards) == 12 and r.winner == -1 for r in res) and all(z == 0.0 for _, _, z in stream.values())
    eng = azk.Engine(game, 2, 8, size=size, emit_symmetry=emit)
    assert (eng.emit_elements, eng.emit_group) == (mask, len(els))


def test_getter_without_the_option():
    import azk
    assert (azk.Engine("gomoku", 2, 8, size=7).emit_elements, azk.Engine("gomoku", 2, 8, size=7).emit_group) == (0, 8)
    assert (azk.Engine("connect4", 2, 8).emit_elements, azk.Engine("connect4", 2, 8).emit_group) == (0, 0)


# ---- 4. the ring wraps; the stream index is 64-bit ----------------------------------------------------------------------------------------
def test_ring_smaller_than_the_output_keeps_the_newest_tuples():
    res, ring, cursor = play("connect4", None, "board", 6, capacity=40)
    stream, end = expected_stream("connect4", None, "board", res)
    assert end > 40                                                    # (a game has at least seven plies: four games fill 4 * 12 slots or more)
    assert_ring(ring, cursor, stream, end, 40)


def test_stream_index_past_2_to_31():
    start = (1 << 31) - 5
    res, ring, cursor = play("connect4", None, "board", 6, capacity=1000, start=start)
    stream, end = expected_stream("connect4", None, "board", res, start=start)
    bases = sorted(r.replay_base for r in res)
    assert bases[0] == start and bases[-1] > (1 << 31) and end - start < 1000
    assert_ring(ring, cursor, stream, end, 1000, start=start)


# ---- 5. with the other opt-ins ---------------------------------------------------------------------------------------------------------------
def test_playout_cap_emits_the_full_plies_in_groups_of_one_and_n():
    res, ring, cursor = play("connect4", None, "board", 8, playout_cap=(0.5, 4))
    flags = [f for r in res for f in r.full]
    assert any(flags) and not all(flags)
    stream, end = expected_stream("connect4", None, "board", res, capped=True)
    assert end == sum(sum((1 if i < 2 else 2) for i, f in enumerate(r.full) if f) for r in res)
    assert_ring(ring, cursor, stream, end, len(ring[2]))


def test_forced_playouts_emit_the_pruned_policy_target(monkeypatch):
    import azk
    raw, pruned = [], []                                               # per move: root_stats' pi (raw visits) and root_policy_target's, [G, A] each
    target = azk.Engine.root_policy_target

    def recording(self):
        raw.append(self.pi.cpu().numpy().copy())                       # (self_play_batch has just called root_stats: its pi is in Engine.pi)
        out = target(self)
        pruned.append(out.cpu().numpy().copy())
        return out
    monkeypatch.setattr(azk.Engine, "root_policy_target", recording)
    res, ring, cursor = play("gomoku", (5, 7), "board", 9, forced_playouts=2.0)       # SelfPlayResult.pis: root_policy_target's rows
    monkeypatch.undo()
    stream, end = expected_stream("gomoku", (5, 7), "board", res)
    assert_ring(ring, cursor, stream, end, len(ring[2]))
    # ... and those rows ARE pruned ones: some ply from the third on lost a visited child altogether, and the ring holds that row, not the raw one
    # (a child that is not the most visited, has ONE visit and a mixed prior >= 1 / (k * 16) = 1 / 32 is pruned to zero - prune_counts' last rule;
    #  16 simulations over a Gomoku root's handful of legal moves leave such children at most plies)
    hits = 0
    for g, r in enumerate(res):
        for i in range(2, len(r.pis)):
            assert np.array_equal(r.pis[i], pruned[i][g])
            if np.any((raw[i][g] > 0) & (pruned[i][g] == 0)):
                hits += 1
                stored = [stream[r.replay_base + er.count_tuples(i, 4) + k][1] for k in range(4)]      # the ply's group, element 0 first
                assert np.array_equal(stored[0], pruned[i][g]) and not np.array_equal(stored[0], raw[i][g])
                slot = (r.replay_base + er.count_tuples(i, 4)) % len(ring[2])
                assert np.array_equal(ring[1][slot], pruned[i][g])
    print("plies whose recorded pi lost a visited child:", hits)
    assert hits > 0


# ---- 6. the asynchronous drain ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,size", [("gomoku", (5, 7)), ("connect4", None)])
def test_async_drain_emits_the_lockstep_tuples(game, size):
    from selfplay import AsyncSelfPlayRunner
    planes, rows, cols, A = geometry(game, size)
    res, ring, cursor = play(game, size, "board", 5)
    want = sorted(er.tuple_sha(ring[0][i], ring[1][i], ring[2][i]) for i in range(cursor))
    rb = new_ring(game, size, len(ring[2]))
    a = AsyncSelfPlayRunner(game, lambda x: fixture_logits_value(x, A, "hash"), G, SIMS, size=size, seed=5, recycle=False, replay=rb, per_launch=2,
                            steps_per_graph=4, use_graph=False, emit_symmetry="board")
    for _ in range(2000):
        a.run_chunk()
        if int(a.finish()[0]) == G:
            break
    assert int(a.finish()[0]) == G
    s, p, z = ring_numpy(rb)
    assert int(rb.cursor.item()) == cursor
    assert sorted(er.tuple_sha(s[i], p[i], z[i]) for i in range(cursor)) == want
    assert np.all(z[cursor:] == 7.0) and np.all(s[cursor:] == -5.0)


# ---- 7. what azk_create refuses ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,size,emit", [("gomoku", (5, 7), (0, 3)), ("connect4", None, (0, 2)), ("gomoku", 7, (1, 2)), ("gomoku", 7, (0, 8))])
def test_create_refuses(game, size, emit):
    import azk
    with pytest.raises(azk.AzkError, match="emit_elements"):
        azk.Engine(game, 2, 8, size=size, emit_symmetry=emit)


def test_an_engine_handed_in_must_agree():
    import azk
    from selfplay import self_play_batch
    eng = azk.Engine("connect4", G, SIMS, emit_symmetry="board")
    with pytest.raises(ValueError):
        self_play_batch("connect4", lambda x: fixture_logits_value(x, 7, "hash"), G, SIMS, engine=eng, emit_symmetry="none")
    with pytest.raises(ValueError):
        self_play_batch("connect4", lambda x: fixture_logits_value(x, 7, "hash"), G, SIMS, engine=eng)


# ---- train.collect_data: the device ring and a host buffer get the same tuples ------------------------------------------------------------------
@pytest.mark.parametrize("game", ["connect4", "gomoku5x7"])
def test_collect_data_fills_both_buffer_kinds_alike(game):
    import azk
    import train
    from fixture_eval import FixtureModel
    from games import Connect4, Gomoku

    class Gomoku5x7(Gomoku):
        rows, cols = 5, 7
        action_dim = state_dim = 35
    Game = Connect4 if game == "connect4" else Gomoku5x7
    n = len(elements_of(Game.engine_name, Game._size(), "board"))
    ring = azk.DeviceReplay(G * er.count_tuples(Game.state_dim, n), Game.feature_dim, Game.rows, Game.cols, Game.action_dim)
    host = []

    class Host:
        add = staticmethod(lambda s, p, t: host.append((np.array(s, np.float32), np.array(p, np.float64), float(t[0]))))
    r1 = train.collect_data(Game, FixtureModel(Game.action_dim), ring, G, SIMS, seed=3, emit_symmetry="board")
    r2 = train.collect_data(Game, FixtureModel(Game.action_dim), Host, G, SIMS, seed=3, emit_symmetry="board")
    assert r1 == r2 and sum(r1) == G and ring.size() == len(host) > 0
    assert sorted(er.tuple_sha(s, p, z[0]) for s, p, z in ring.to_reference_deque()) == sorted(er.tuple_sha(*t) for t in host)
    with pytest.raises(ValueError):
        train.collect_data(Game, FixtureModel(Game.action_dim), Host, 1, SIMS, batched=False, emit_symmetry="board")
