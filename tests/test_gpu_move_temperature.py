"""Move temperature - per-ply schedule, visit offset, value cutoff (azk_set_move_temperature) - against the plain-Python
restatement of tests/move_temperature_restated.py: the mover's cell and the four counters on every case and setting, the ply schedule, the
table that plays the games of an engine without the option, the recorded pi, the asynchronous movers against the lock-step runner, the arena,
and the refusals.  The positions are those whose preconditions tests/test_move_temperature_restated.py asserts on the CPU."""
import hashlib

import numpy as np
import pytest

import move_temperature_restated as mt
from fixture_eval import FixtureModel, fixture_logits_value
from test_gpu_playout_cap import assert_same_records, async_records, lockstep_records, shared

gpu = pytest.mark.gpu
G = mt.G
SEED, MOVES, N_SIMS = 5, 10, 16
SCHEDULE = dict(tau=[4.0, 4.0, 0.25, 0.25, 1.0, 0.0], visit_offset=1, value_cutoff=0.3)     # the runners' setting: three rows, then greedy


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_for(name, **kw):
    import azk
    kind, size = mt.engine_game(name)
    return azk.Engine(kind, G, mt.N_SIMS, size=size, **kw)


def load(eng, slots, move_count=None):
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots],
                      [s["move_count"] for s in slots] if move_count is None else move_count)
    return torch.from_numpy(np.stack([s["noise"] for s in slots])).to(eng.device)


def searched(name):
    """An engine holding the case's positions and the trees of their searches; the root children are the restatement's (the CPU test's
    preconditions are then the engine's)."""
    og, slots = mt.case(name)
    eng = engine_for(name)
    eng.search(evaluator(eng.action_dim), mt.sims_of(name), load(eng, slots))
    eng.check_error()
    for g, s in enumerate(slots):
        ch = eng.root_children(g)
        assert ch["cell"].tolist() == [int(c) for c in s["children"]["cell"]] and ch["visit"].tolist() == [int(n) for n in s["children"]["visit"]], (name, g)
        assert ch["value"].tobytes() == np.array(s["children"]["value"], np.float64).tobytes(), (name, g)
    return og, slots, eng


def move(eng, slots, us, move_count=None):
    """One advance of the loaded positions on the uniforms us ([G] or None); the move does not touch the tree, so loading the positions again
    puts the engine back in front of the same move of the same search."""
    import torch
    load(eng, slots, move_count)
    uni = torch.tensor(us, dtype=torch.float64, device=eng.device) if us is not None else None
    chosen, _, _ = eng.advance(uni, 0)
    eng.check_error()
    return chosen.cpu().numpy().tolist()


# ---- 1. the mover is the restatement -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("name", mt.CASES)
def test_the_mover_is_the_restatement(name):
    """Every setting (tau x visit offset x value cutoff) on every slot and each of its six uniforms: the cell is `choose`'s, exactly, and the
    four counters are the restatement's sums.  One search per case: the settings and uniforms all move from its trees."""
    from selfplay import move_temperature_setting
    og, slots, eng = searched(name)
    a_of = mt.action_of_game(og)
    children = [eng.root_children(g) for g in range(G)]            # the engine's own children through the restatement: the same cell again
    for setting in mt.SETTINGS:
        tau, offset, cutoff = setting
        us, cells, stats = mt.expected(name, setting)
        load(eng, slots)                                           # (new positions end the search: the option is set between searches)
        eng.set_move_temperature(*move_temperature_setting(tau, mt.N_SIMS, eng.state_dim, offset, cutoff))
        for k in range(6):
            got = move(eng, slots, [us[g][k] for g in range(G)])
            for g, s in enumerate(slots):
                again = mt.choose(children[g], a_of, mt.expected_row(tau, mt.N_SIMS), offset, cutoff, us[g][k], og.action_dim)[0]
                assert got[g] == cells[g][k] == again, (name, setting, g, k, us[g][k])
        assert eng.move_temperature_stats() == stats, (name, setting)


# ---- 2. the ply schedule -------------------------------------------------------------------------------------------------------------------
@gpu
def test_each_ply_uses_its_own_row():
    from selfplay import move_temperature_setting
    og, slots, eng = searched("gomoku7")
    a_of = mt.action_of_game(og)
    taus = [4.0, 0.25, 0.0]
    plies = [0, 1, 2, 5, 0, 1, 2, 5]
    load(eng, slots, plies)                                        # (new positions end the search: the option is set between searches)
    eng.set_move_temperature(*move_temperature_setting(taus, mt.N_SIMS, eng.state_dim))
    assert eng.move_temperature[0].tolist() == [0, 1, -1]
    rng = np.random.RandomState(11)
    differ = 0
    for _ in range(4):
        us = [float(u) for u in rng.random_sample(G)]
        got = move(eng, slots, us, plies)
        for g, s in enumerate(slots):
            tau = taus[min(plies[g], 2)]
            row = mt.expected_row(tau, mt.N_SIMS) if tau > 0.0 else None
            assert got[g] == mt.choose(s["children"], a_of, row, 0, None, us[g], og.action_dim)[0], (g, us[g])
            if tau > 0.0:
                other = mt.expected_row(taus[1 - min(plies[g], 2)], mt.N_SIMS)
                differ += got[g] != mt.choose(s["children"], a_of, other, 0, None, us[g], og.action_dim)[0]
            else:                                                  # plies 2 and 5: the first most-visited child whatever u is
                visits = [int(n) for n in s["children"]["visit"]]
                assert got[g] == int(s["children"]["cell"][visits.index(max(visits))])
    assert differ >= 1                                             # the rows are told apart: some slot's cell is not the other row's
    assert eng.move_temperature_stats()[0] == 4 * 4                # plies 0 and 1 only
    assert move(eng, slots, None, [0] * G) == [mt.choose(s["children"], a_of, None, 0, None, None)[0] for s in slots]     # no uniforms: greedy
    assert eng.move_temperature_stats()[0] == 4 * 4


# ---- 3. the identity -----------------------------------------------------------------------------------------------------------------------
def ring_rows(rp):
    s, p, z = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    return [hashlib.sha256(s[i].tobytes() + p[i].tobytes() + z[i:i + 1].tobytes()).hexdigest() for i in range(rp.size())]


def games(res):
    return [(r.cells, [p.tobytes() for p in r.pis], r.qs, r.winner) for r in res]


@gpu
@pytest.mark.parametrize("game,size,shape", [("gomoku", 7, (2, 7, 7, 49)), ("connect4", None, (3, 6, 7, 7))])
def test_the_visits_row_until_sample_until_plays_the_games_of_an_engine_without_the_option(game, size, shape):
    import azk
    from selfplay import SAMPLE_UNTIL, self_play_batch
    ev = evaluator(shape[3])
    emit = None if game == "gomoku" else "board"                   # (a rectangular board emits under a mask of elements only)

    def play(**kw):
        rp = azk.DeviceReplay(8192, *shape)
        res = self_play_batch(game, ev, G, N_SIMS, size=size, seed=SEED, replay=rp, emit_symmetry=emit, **kw)
        assert all(r.winner is not None for r in res)
        return games(res), ring_rows(rp)
    want = play()
    assert play(move_temperature=("until", 1.0, SAMPLE_UNTIL[game])) == want
    # ... and an engine that had another table set, cleared, is an engine without the option
    eng = azk.Engine(game, G, N_SIMS, size=size, emit_symmetry=emit)
    sharp = self_play_batch(game, ev, G, N_SIMS, size=size, seed=SEED, emit_symmetry=emit, engine=eng, move_temperature=dict(tau=0.25, visit_offset=1))
    assert [r.cells for r in sharp] != [g[0] for g in want[0]] and eng.move_temperature_stats()[0] > 0
    eng.clear_move_temperature()
    assert eng.move_temperature is None
    assert play(engine=eng) == want


# ---- 4. the recorded pi --------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_recorded_pi_is_the_raw_visit_distribution():
    import azk
    from selfplay import move_temperature_setting, self_play_batch
    og, slots, eng = searched("gomoku7")
    load(eng, slots)
    eng.set_move_temperature(*move_temperature_setting(0.25, mt.N_SIMS, eng.state_dim))
    want = eng.root_stats()[0].cpu().numpy().copy()
    assert eng.root_policy_target().cpu().numpy().tobytes() == want.tobytes()
    for g, s in enumerate(slots):
        visits = np.zeros(49)
        visits[[int(c) for c in s["children"]["cell"]]] = s["children"]["visit"]
        assert want[g].tobytes() == (visits / np.sum(visits)).tobytes(), g
    # whole games at tau 0.25: what the batch records (root_stats before each move) and what the movers record (traj_pi, which emission reads)
    rp = azk.DeviceReplay(8192, 2, 7, 7, 49)
    res = self_play_batch("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, move_temperature=0.25, replay=rp)
    plain = self_play_batch("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, max_moves=1)
    # ply 0 is the same search in both calls (same seed, same noise row): the same recorded bytes, however the move is made afterwards
    assert all(a.pis[0].tobytes() == b.pis[0].tobytes() for a, b in zip(res, plain))
    recorded = set()
    for r in res:
        for pi in r.pis:                                           # a visit distribution: counts over their sum, which no tempered target is
            counts = np.rint(pi * (N_SIMS - 1))
            assert counts.sum() == N_SIMS - 1 and np.array_equal(pi, counts / float(N_SIMS - 1))
            recorded.add(np.sort(pi).tobytes())
    ring = rp.pis.cpu().numpy()[: rp.size()]
    assert len(ring) > 0 and all(np.sort(row).tobytes() in recorded for row in ring)     # (emission turns the board: the entries are permuted)


# ---- 5. the asynchronous movers ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("extras", ["none", "reroot2", "resign_cap"])
def test_async_equals_lockstep_slot_for_slot(extras):
    lock_kw, async_kw, cap = dict(cache_entries=64), dict(cache_entries=64, per_launch=2, steps_per_graph=4), None
    if extras == "reroot2":
        lock_kw["tree_reuse"], async_kw["reroot"] = 2, 2
    if extras == "resign_cap":
        cap = (0.5, 6)
        lock_kw["resign"] = async_kw["resign"] = (0.25, 0.5)
    want, lr = lockstep_records("gomoku", MOVES, seed=SEED, n_sims=N_SIMS, cap=cap, move_temperature=SCHEDULE, **lock_kw)
    got, ar = async_records("gomoku", MOVES, seed=SEED, n_sims=N_SIMS, cap=cap, move_temperature=SCHEDULE, **async_kw)
    assert_same_records(got, want, MOVES, (extras,))
    off = shared(("move temperature off", extras), lambda: lockstep_records("gomoku", MOVES, seed=SEED, n_sims=N_SIMS, cap=cap, **lock_kw)[0])
    assert any(want[k][2] != off[k][2] for k in want if k in off)                  # the option was on: other cells
    ls, as_ = lr.move_temperature_stats(), ar.move_temperature_stats()
    assert ls[0] > 0 and as_[0] >= ls[0] > ls[1] > 0                               # (the asynchronous slots may have moved on past MOVES)


# ---- 6. the arena --------------------------------------------------------------------------------------------------------------------------
@gpu
def test_the_arena_plays_self_play_batchs_games():
    import arena
    from selfplay import self_play_batch
    m1, m2 = FixtureModel(49), FixtureModel(49, "uniform")
    setting = dict(tau=("until", 0.5, 6), value_cutoff=0.5)
    rng = np.random.RandomState(3)
    us = rng.random_sample((49, G))

    def uniform_fn(mv):
        return us[mv]
    winners, res = arena.compete_batch("gomoku", m1, m2, G, 16, 12, size=7, seed=SEED, uniform_fn=uniform_fn, move_temperature=setting)
    want = self_play_batch("gomoku", (m1, m2), G, (16, 12), size=7, seed=SEED, uniform_fn=uniform_fn, sample_until=0, move_temperature=setting)
    assert [r.cells for r in res] == [r.cells for r in want] and winners.tolist() == [r.winner for r in want]
    # `sampling` is not looked at under the option, and without the option the games differ
    w2, res2 = arena.compete_batch("gomoku", m1, m2, G, 16, 12, sampling=True, size=7, seed=SEED, uniform_fn=uniform_fn, move_temperature=setting)
    assert [r.cells for r in res2] == [r.cells for r in want]
    _, greedy = arena.compete_batch("gomoku", m1, m2, G, 16, 12, size=7, seed=SEED, uniform_fn=uniform_fn)
    assert [r.cells for r in greedy] != [r.cells for r in want]


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_engine_usable():
    import ctypes
    import azk
    ARG, STATE = -1, -4
    og, slots, eng = searched("gomoku7")
    L, h = eng.L, eng.h
    n = mt.N_SIMS + 1
    rows = np.array([0, 1, -1], np.int32)
    w = np.array([mt.expected_row(1.0, mt.N_SIMS), mt.expected_row(0.5, mt.N_SIMS)], np.float64)

    def call(rows=rows, n_plies=3, w=w, n_rows=2, n_cols=n, offset=0, cutoff=-1.0):
        rc = L.azk_set_move_temperature(h, rows.ctypes.data, n_plies, np.ascontiguousarray(w, np.float64).ctypes.data, n_rows, n_cols, offset,
                                        ctypes.c_double(cutoff), None)
        if rc != 0:
            assert len(L.azk_last_error(h).decode()) > 20 and "azk_set_move_temperature" in L.azk_last_error(h).decode()
        return rc

    def changed(r, c, v):
        x = w.copy()
        x[r, c] = v
        return x
    load(eng, slots)                                               # (the search is over)
    assert call(n_plies=0) == ARG and call(n_rows=0) == ARG
    assert call(n_cols=n - 1) == ARG and call(w=np.zeros((2, n + 1)), n_cols=n + 1) == ARG
    assert call(rows=np.array([0, 2, -1], np.int32)) == ARG and call(rows=np.array([0, -2, -1], np.int32)) == ARG
    for bad in (-1.0, float("nan"), float("inf")):
        assert call(w=changed(1, 3, bad)) == ARG, bad
    assert call(w=changed(0, 0, 0.5)) == ARG                       # an unvisited child is never played
    assert call(w=np.array([w[0], np.zeros(n)])) == ARG           # a row without a positive weight
    big = np.finfo(np.float64).max / (2 * n)
    assert call(w=changed(1, n - 1, big * 1.001)) == ARG and call(w=changed(1, n - 1, big * 0.999)) == 0
    assert call(offset=-1) == ARG and call(cutoff=float("nan")) == ARG
    assert call(cutoff=float("inf")) == 0 and call(cutoff=-5.0) == 0 and call() == 0
    assert L.azk_clear_move_temperature(h) == 0
    out = np.zeros(4, np.int64)
    assert L.azk_get_move_temperature_stats(h, out.ctypes.data, None) == STATE      # off: nothing to read
    with pytest.raises(azk.AzkError):
        eng.move_temperature_stats()
    # during a search
    eng.begin_search(load(eng, slots))
    assert call() == STATE
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
    # a Gumbel root, in both directions
    eng.set_gumbel_root(4, mt.N_SIMS)
    assert call() == STATE
    eng.clear_gumbel_root()
    assert call() == 0
    with pytest.raises(azk.AzkError, match="error -4"):
        eng.set_gumbel_root(4, mt.N_SIMS)
    assert eng.gumbel_root is None
    assert L.azk_clear_move_temperature(h) == 0
    # carry tree reuse is refused, top-up is not
    carry = azk.Engine("gomoku", 2, 8, size=7, tree_reuse=1)
    with pytest.raises(azk.AzkError, match="error -4"):
        carry.set_move_temperature([0], [mt.expected_row(1.0, 8)])
    assert carry.move_temperature is None and "tree_reuse = 1" in carry.L.azk_last_error(carry.h).decode()
    azk.Engine("gomoku", 2, 8, size=7, tree_reuse=2).set_move_temperature([0], [mt.expected_row(1.0, 8)])
    # after azk_async_begin
    from selfplay import AsyncSelfPlayRunner
    r = AsyncSelfPlayRunner("gomoku", evaluator(49), 4, 8, size=7, use_graph=False, move_temperature=1.0)
    with pytest.raises(azk.AzkError, match="error -4"):
        r.eng.set_move_temperature([0], [mt.expected_row(1.0, 8)])
    with pytest.raises(azk.AzkError, match="error -4"):
        r.eng.clear_move_temperature()
    r.run_chunk()
    r.finish()
    r.check_error()
    # ... and the engine searches and moves as if nothing had been asked: the trees and the greedy moves of an engine without the option
    eng.search(evaluator(49), mt.N_SIMS, load(eng, slots))
    eng.check_error()
    for g, s in enumerate(slots):
        assert eng.root_children(g)["visit"].tolist() == [int(x) for x in s["children"]["visit"]], g
    a_of = mt.action_of_game(og)
    assert move(eng, slots, [0.5] * G) == [mt.choose(s["children"], a_of, None, 0, None, None)[0] for s in slots]
