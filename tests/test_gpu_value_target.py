"""Value targets on the GPU (azk_set_value_target): the per-ply q the movers keep against SelfPlayResult.qs bit for bit, the
ring's z column against the plain-Python restatement (tests/value_target_restated.py) on the engine's own record with states and pis equal to
the option-off ring byte for byte, the two identity settings against the engine without the option, the asynchronous movers against the
lock-step runner, sharding, and the ABI's refusals.  G = 8 games, 24 simulations, the "hash" fixture evaluator.

Liveness is asserted, not assumed: every emission batch must hold a decisive game and a tuple whose target differs from its z by more than
1e-3, and the batches together a drawn game and a resigned one.  Seeds: every batch runs at SEED = 3; SEEDS lists the batches that need
another seed for that, and why."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest

import emission_restated as er
import test_gpu_emit_symmetry as es
import value_target_restated as vr
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import GAMES, ring_rows

pytestmark = pytest.mark.gpu

G, SIMS, SEED, MOVES = 8, 24, 3, 12
CAP, RESIGN, OPEN, REROOT = (0.5, 6), (0.25, 0.5), (1.0, 4, 2), 2
SETTINGS = [(0.5, 0.0), (1.0, 0.7), (0.5, 0.9)]
# batch name -> seed, where SEED = 3 leaves a batch without a decisive game (none needed one so far: the drawn games are tictactoe's, the
# resigned ones the resign batch's at p_never = 0.5)
SEEDS = {}


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


@functools.lru_cache(maxsize=None)
def play(name, game, size, emit, vt, n_games=G, first=0, **opts):
    """One lock-step batch to the end on an engine of its own, the ring attached -> (results, ring as numpy, cursor, the engine's q record
    or None without the option); computed once per case and left unchanged."""
    import azk
    from selfplay import self_play_batch
    planes, rows, cols, A = es.geometry(game, size)
    rp = es.new_ring(game, size, n_games * er.count_tuples(rows * cols, 8) * 2)
    eng = azk.Engine(game, n_games, SIMS, size=size, tree_reuse=opts.get("tree_reuse", 0),
                     emit_symmetry=es.elements_of(game, size, emit) if emit is not None else None)
    res = self_play_batch(game, evaluator(A), n_games, SIMS, size=size, seed=SEEDS.get(name, SEED), first_global_game=first, replay=rp,
                          emit_symmetry=emit, engine=eng, value_target=vt, **opts)
    rec = eng.value_record().cpu().numpy() if vt is not None else None
    assert eng.value_target == vt
    return res, es.ring_numpy(rp), int(rp.cursor.item()), rec


def group_elements(game, size, emit):
    return es.elements_of(game, size, emit) if emit is not None else tuple(range(8))


def kind_of(game):
    return "connect4" if game == "connect4" else "gomoku"


def copies_of(r, opts):
    from selfplay import surprise_copies
    if "surprise_weight" not in opts:
        return None
    return surprise_copies(r.kl, r.coin, opts["surprise_weight"], r.full if "playout_cap" in opts else None)


# ---- 1. the record -------------------------------------------------------------------------------------------------------------------
RECORD = [("rec-gomoku7", "gomoku", 7, None, {}), ("rec-connect4", "connect4", None, "board", {}), ("rec-tictactoe", "tictactoe", None, None, {}),
          ("rec-gomoku5x3-forced-cap", "gomoku", (5, 3), "board", dict(playout_cap=CAP, forced_playouts=2.0))]


@pytest.mark.parametrize("name,game,size,emit,opts", RECORD, ids=[c[0] for c in RECORD])
def test_the_movers_keep_the_q_of_every_played_ply(name, game, size, emit, opts):
    res, _, _, rec = play(name, game, size, emit, (0.5, 0.9), **opts)
    n_plies = 0
    for g, r in enumerate(res):
        assert r.winner is not None and len(r.qs) == len(r.boards) > 0
        got = rec[g, :len(r.qs)]
        assert got.tobytes() == np.asarray(r.qs, np.float64).tobytes(), (name, g)
        n_plies += len(r.qs)
    assert any(q != 0.0 for r in res for q in r.qs)
    if "playout_cap" in opts:
        flags = [f for r in res for f in r.full]
        assert any(flags) and not all(flags)
    print(name, "plies", n_plies)


# ---- 2. emission, bit for bit given the recorded q ------------------------------------------------------------------------------------
EMIT = [("emit-gomoku7", "gomoku", 7, None, {}),
        ("emit-tictactoe", "tictactoe", None, None, {}),                                    # the drawn games
        ("emit-connect4-board", "connect4", None, "board", {}),
        ("emit-gomoku7-cap", "gomoku", 7, None, dict(playout_cap=CAP)),                      # fast plies: not written, read by the recurrence
        ("emit-gomoku7-openings", "gomoku", 7, None, dict(openings=OPEN)),                   # the recurrence stops at the first searched ply
        ("emit-gomoku7-surprise", "gomoku", 7, None, dict(surprise_weight=0.5)),             # every copy carries the target
        ("emit-gomoku7-resign", "gomoku", 7, None, dict(resign=RESIGN)),                     # an ordinary finished game
        ("emit-gomoku7-topup", "gomoku", 7, None, dict(tree_reuse=2))]                       # q is the carried root's W / N


def expected_stream(game, size, emit, res, vt, opts):
    """{stream index: tuple}, the stream's end, and per tuple (target as the ring keeps it, outcome) from the engine's own records."""
    els = group_elements(game, size, emit)
    capped = "playout_cap" in opts
    stream, total, pairs = {}, 0, []
    for r in res:
        assert r.winner is not None and r.replay_base is not None
        full, copies = (r.full if capped else None), copies_of(r, opts)
        t = None if vt is None else [vr.ring_z(x) for x in vr.targets(r.qs, r.winner, r.open_plies, *vt)]
        want = vr.game_tuples(kind_of(game), r.boards, r.pis, r.winner, els, t, first_ply=r.open_plies, full=full, copies=copies)
        outc = vr.game_tuples(kind_of(game), r.boards, r.pis, r.winner, els, None, first_ply=r.open_plies, full=full, copies=copies)
        for k, tup in enumerate(want):
            assert r.replay_base + k not in stream
            stream[r.replay_base + k] = tup
        pairs += [(a[2], b[2]) for a, b in zip(want, outc)]
        total += len(want)
    assert sorted(stream) == list(range(total))                   # the games' ranges tile the stream
    return stream, total, pairs


@pytest.mark.parametrize("vt", SETTINGS, ids=lambda v: "r%g-lam%g" % v)
@pytest.mark.parametrize("name,game,size,emit,opts", EMIT, ids=[c[0] for c in EMIT])
def test_emission_writes_the_restated_targets_and_nothing_else(name, game, size, emit, opts, vt):
    res, ring, cursor, rec = play(name, game, size, emit, vt, **opts)
    res_off, ring_off, cursor_off, _ = play(name, game, size, emit, None, **opts)
    # the games are the games of the engine without the option, and so are states and pis, byte for byte
    assert cursor == cursor_off > 0 and [r.replay_base for r in res] == [r.replay_base for r in res_off]
    assert all(a.cells == b.cells and a.winner == b.winner and a.qs == b.qs and a.open_plies == b.open_plies for a, b in zip(res, res_off))
    assert ring[0].tobytes() == ring_off[0].tobytes() and ring[1].tobytes() == ring_off[1].tobytes()
    # the z column: np.float32 of the restated target at every tuple (and the option-off ring is the restated emission too)
    stream, end, pairs = expected_stream(game, size, emit, res, vt, opts)
    es.assert_ring(ring, cursor, stream, end, len(ring[2]))
    stream_off, end_off, _ = expected_stream(game, size, emit, res_off, None, opts)
    es.assert_ring(ring_off, cursor_off, stream_off, end_off, len(ring_off[2]))
    # liveness
    far = sum(abs(t - z) > 1e-3 for t, z in pairs)
    print(name, vt, "tuples", end, "targets off z by > 1e-3", far, "winners", [r.winner for r in res], "resigned", sum(r.resigned for r in res))
    assert any(r.winner in (0, 1) for r in res) and far >= 1
    assert ring[2].tobytes() != ring_off[2].tobytes()
    if "playout_cap" in opts:
        flags = [f for r in res for f in r.full]
        assert any(flags) and not all(flags)
        assert any(not f and any(r.full[:i]) for r in res for i, f in enumerate(r.full))      # a fast ply above a written one: its q is read
    if "openings" in opts:
        assert any(r.open_plies >= 2 for r in res) and all(r.open_plies >= 1 for r in res)
    if "surprise_weight" in opts:
        c = [int(x) for r in res for x in copies_of(r, opts)]
        assert c.count(0) >= 1 and sum(x >= 2 for x in c) >= 1
    if "resign" in opts:
        assert any(r.resigned for r in res)


def test_the_batches_together_hold_a_drawn_and_a_resigned_game():
    drawn = resigned = 0
    for name, game, size, emit, opts in EMIT:
        res = play(name, game, size, emit, SETTINGS[0], **opts)[0]
        drawn += sum(r.winner == -1 for r in res)
        resigned += sum(bool(r.resigned) for r in res)
    print("drawn", drawn, "resigned", resigned)
    assert drawn >= 1 and resigned >= 1


# ---- 3. the identity settings are the engine without the option ----------------------------------------------------------------------
@pytest.mark.parametrize("vt", [(0.0, 0.5), (1.0, 1.0)], ids=lambda v: "r%g-lam%g" % v)
@pytest.mark.parametrize("name,game,size,emit", [("emit-gomoku7", "gomoku", 7, None), ("emit-tictactoe", "tictactoe", None, None)])
def test_identity_settings_write_the_option_off_ring_and_still_record(name, game, size, emit, vt):
    res, ring, cursor, rec = play(name, game, size, emit, vt)
    res_off, ring_off, cursor_off, _ = play(name, game, size, emit, None)
    assert cursor == cursor_off > 0
    for a, b in zip(ring, ring_off):
        assert a.tobytes() == b.tobytes()                          # (a draw's z keeps +0.0: the bytes are compared, not the values)
    assert [r.replay_base for r in res] == [r.replay_base for r in res_off]
    for g, r in enumerate(res):
        assert rec[g, :len(r.qs)].tobytes() == np.asarray(r.qs, np.float64).tobytes() and any(q != 0.0 for q in r.qs)
    if game == "tictactoe":
        assert any(r.winner == -1 for r in res)


# ---- 4. the asynchronous movers ------------------------------------------------------------------------------------------------------
CASES = list(itertools.product((0, REROOT), (False, True)))
VT = (0.5, 0.9)


def case_id(c):
    return "-".join(n for n, on in zip(("reroot", "cap"), c) if on) or "plain"


def case_kw(case):
    reroot, cap = case
    lock_kw, async_kw = dict(cache_entries=64), dict(cache_entries=64, per_launch=2, steps_per_graph=4)
    if reroot:
        lock_kw["tree_reuse"] = async_kw["reroot"] = reroot
    if cap:
        lock_kw["playout_cap"] = async_kw["playout_cap"] = CAP
    return lock_kw, async_kw


def lockstep_run(moves, recycle, replay=None, **kw):
    """{(slot, move): (pi bytes, q, cell, winner, kind)} of SelfPlayRunner(value_target=VT), and the runner."""
    from selfplay import SelfPlayRunner
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        full = r.record_full if r.record_full is not None else np.ones(len(ch), np.uint8)
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]), int(full[g]))
    r = SelfPlayRunner("gomoku", evaluator(49), G, SIMS, size=7, seed=SEED, on_records=on, recycle=recycle, replay=replay, value_target=VT, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_run(done, recycle, replay=None, **kw):
    from selfplay import AsyncSelfPlayRunner
    rec = {}

    def on(meta, q, pi):
        full = r.record_full if r.record_full is not None else np.ones(len(meta), np.uint8)
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]), int(full[i]))
    r = AsyncSelfPlayRunner("gomoku", evaluator(49), G, SIMS, size=7, seed=SEED, on_records=on, recycle=recycle, replay=replay, use_graph=False,
                            value_target=VT, **kw)
    for _ in range(8000):
        r.run_chunk()
        fin = r.finish()
        if done(rec, fin):
            break
    r.check_error()
    return rec, r


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_async_movers_play_the_lockstep_games(case):
    lock_kw, async_kw = case_kw(case)
    want, lr = lockstep_run(MOVES, True, **lock_kw)
    got, ar = async_run(lambda rec, fin: all((g, MOVES - 1) in rec for g in range(G)), True, **async_kw)
    for g in range(G):
        for mv in range(MOVES):
            assert got[(g, mv)] == want[(g, mv)], (case_id(case), g, mv)
    assert lr.eng.value_target == ar.eng.value_target == VT
    kinds = [v[4] for v in want.values()]
    assert 0 < sum(kinds) < len(kinds) if case[1] else all(kinds)
    for c in (lr.counters(), ar.counters()):
        assert (c["roots_reused"] > 0) == bool(case[0])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_drained_rings_equal_the_lockstep_rings_and_the_restated_targets(case):
    """Games played to their end without restarts: the drain's k_emit_tuples<LIST, .., VALUE> against the lock-step emission (the stream's
    order follows the finishing order, so the rings are compared as multisets of rows), and the drained z values against the restatement
    applied to the q column of the asynchronous record ring."""
    import azk
    lock_kw, async_kw = case_kw(case)
    ra, rb = azk.DeviceReplay(8192, 2, 7, 7, 49), azk.DeviceReplay(8192, 2, 7, 7, 49)
    _, lr = lockstep_run(49, False, replay=ra, **lock_kw)
    rec, ar = async_run(lambda rec, fin: int(fin[0]) == G, False, replay=rb, **async_kw)
    assert int(ar.finish()[0]) == G
    assert 0 < int(ra.cursor.item()) == int(rb.cursor.item()) <= 8192 and sorted(ring_rows(ra)) == sorted(ring_rows(rb))
    want_z, decisive, far = [], 0, 0
    for g in range(G):
        plies = sorted(mv for (slot, mv) in rec if slot == g)
        assert plies == list(range(len(plies))) and rec[(g, plies[-1])][3] != -2       # the whole game, its last record the one that ended it
        qs, winner = [rec[(g, mv)][1] for mv in plies], rec[(g, plies[-1])][3]
        decisive += winner in (0, 1)
        for i, t in enumerate(vr.targets(qs, winner, 0, *VT)):
            if rec[(g, i)][4]:                                     # fast plies take part in the recurrence and are not written
                want_z += [vr.ring_z(t)] * (1 if i < 2 else 8)
                far += abs(t - vr.outcome(winner, i)) > 1e-3
    got_z = rb.zs.cpu().numpy()[:int(rb.cursor.item())]
    assert np.sort(got_z).tobytes() == np.sort(np.asarray(want_z, np.float32)).tobytes()
    assert decisive >= 1 and far >= 1
    if case[1]:
        assert any(v[4] == 0 for v in rec.values()) and any(v[4] == 1 for v in rec.values())


# ---- 5. sharding -------------------------------------------------------------------------------------------------------------------
def test_two_engines_of_four_games_write_what_one_of_eight_writes():
    import hashlib
    whole = play("emit-gomoku7", "gomoku", 7, None, (0.5, 0.9))

    def rows(ring, cursor):
        s, p, z = ring
        return [hashlib.sha256(s[i].tobytes() + p[i].tobytes() + z[i:i + 1].tobytes()).hexdigest() for i in range(cursor)]
    parts = []
    for first in (0, 4):
        res, ring, cursor, rec = play("shard-4", "gomoku", 7, None, (0.5, 0.9), n_games=4, first=first)
        parts += rows(ring, cursor)
        for g in range(4):
            a, b = res[g], whole[0][first + g]
            assert a.cells == b.cells and a.qs == b.qs and a.winner == b.winner
            assert rec[g, :len(a.qs)].tobytes() == whole[3][first + g, :len(a.qs)].tobytes()
    assert sorted(parts) == sorted(rows(whole[1], whole[2])) and len(parts) > 0


# ---- 6. the ABI's refusals ---------------------------------------------------------------------------------------------------------
def test_abi_refusals_and_clear():
    import azk
    L = azk.lib()
    ERR_ARG, ERR_STATE = -1, -4
    e = azk.Engine("gomoku", 2, 8, size=7)
    st = azk._stream()
    q = e.torch.zeros((2, 49), dtype=e.torch.float64, device=e.device)
    assert L.azk_get_value_record(e.h, azk._p(q), st) == ERR_STATE                # the option is not set
    for r, lam in ((-0.25, 0.5), (1.5, 0.5), (float("nan"), 0.5), (math.inf, 0.5), (0.5, -0.25), (0.5, 1.5), (0.5, float("nan")), (0.5, -math.inf)):
        assert L.azk_set_value_target(e.h, C.c_double(r), C.c_double(lam), st) == ERR_ARG, (r, lam)
        assert L.azk_get_value_record(e.h, azk._p(q), st) == ERR_STATE
    assert L.azk_set_value_target(e.h, C.c_double(0.0), C.c_double(0.0), st) == 0     # r = 0 is a live setting
    assert L.azk_get_value_record(e.h, azk._p(q), st) == 0 and L.azk_get_value_record(e.h, None, st) == ERR_ARG
    assert L.azk_set_gumbel_root(e.h, 4, 8, C.c_double(50.0), C.c_double(1.0), st) == ERR_STATE and b"value target" in L.azk_last_error(e.h)
    assert L.azk_clear_value_target(e.h) == 0
    assert L.azk_get_value_record(e.h, azk._p(q), st) == ERR_STATE
    assert L.azk_set_gumbel_root(e.h, 4, 8, C.c_double(50.0), C.c_double(1.0), st) == 0       # ... and the other order
    assert L.azk_set_value_target(e.h, C.c_double(0.5), C.c_double(0.5), st) == ERR_STATE and b"Gumbel" in L.azk_last_error(e.h)
    e.check_error()
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    assert L.azk_set_value_target(vl.h, C.c_double(0.5), C.c_double(0.5), st) == ERR_ARG and b"leaves_per_step" in L.azk_last_error(vl.h)
    c4 = azk.Engine("connect4", 2, 8)                              # created without emit_elements: no trajectories
    assert L.azk_set_value_target(c4.h, C.c_double(0.5), C.c_double(0.5), st) == ERR_ARG and b"trajectories" in L.azk_last_error(c4.h)
    with pytest.raises(azk.AzkError):
        c4.set_value_target(0.5)
    with pytest.raises(azk.AzkError):
        c4.value_record()
    assert azk.Engine("connect4", 2, 8, emit_symmetry="none").set_value_target(0.5, 0.9) is None


def test_clear_returns_the_engine_to_option_off_emission():
    """One engine: a batch with the option, clear, a batch without - the second ring is the ring of an engine that never had the option."""
    import azk
    from selfplay import self_play_batch
    eng = azk.Engine("tictactoe", G, SIMS)
    rings = []
    for vt in ((0.5, 0.9), None):
        rp = es.new_ring("tictactoe", None, G * er.count_tuples(9, 8) * 2)       # the capacity of play's rings: the arrays are compared whole
        if vt is None:
            eng.set_value_target(None)
            assert eng.value_target is None
        self_play_batch("tictactoe", evaluator(9), G, SIMS, seed=SEED, replay=rp, engine=eng, value_target=vt)
        rings.append(es.ring_numpy(rp))
    off = play("emit-tictactoe", "tictactoe", None, None, None)[1]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(rings[1], off))
    assert rings[0][2].tobytes() != off[2].tobytes() and rings[0][0].tobytes() == off[0].tobytes()
