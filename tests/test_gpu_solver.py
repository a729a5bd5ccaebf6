"""Exact game-end proofs in the search (azk_set_solver) against the plain-Python restatement of tests/solver_restated.py:
whole trees and status columns bit for bit in every stepping mode, in every form of the scan and on both precision paths, the outputs, nothing
stale from an earlier search, nothing changed where nothing is proven, the eval caches, the asynchronous movers against the lock-step runner,
one combination run, the arena, and the refusals.  The positions are those whose preconditions tests/test_solver_restated.py asserts on the CPU."""
import numpy as np
import pytest

import forced_playouts_restated as fr
import solver_restated as sr
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import assert_same_records, async_records, lockstep_records, ring_rows

gpu = pytest.mark.gpu
G = sr.G
SEED, MOVES, N_SIMS = 3, 12, 24


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_for(name, n_sims, **kw):
    import azk
    kind, size = fr.GAMES[name] if name in fr.GAMES else ("gomoku", 15)
    return azk.Engine(kind, G, n_sims, size=size, **kw)


def case(name):
    return sr.tictactoe_case() if name == "tictactoe" else sr.constructed_case(name)


def load(eng, slots):
    """The slots' positions into the engine; returns their noise rows as a CUDA tensor (None where the slots have none)."""
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
    if slots[0]["noise"] is None:
        return None
    return torch.from_numpy(np.stack([s["noise"] for s in slots])).to(eng.device)


def run_search(eng, mode, n_sims, noise):
    ev = evaluator(eng.action_dim)
    if mode == "fused":                                            # select-only first launch, fused launches, expand-only last launch
        eng.search(ev, n_sims, noise)
    elif mode == "split":                                          # select-only and expand-only launches alone
        eng.begin_search(noise)
        for _ in range(n_sims):
            eng.step_select()
            n = int(eng.n_leaf.item())
            if n > 0:
                eng.step_expand_backup(*eng.evaluate_leaves(ev, n))
    else:                                                          # budget stepping: the MULTI kernel
        eng.search_budget(ev, n_sims, noise, per_launch=3)
    eng.check_error()


def total(slots, key="solver"):
    return {k: sum(s[key]["stats"][k] for s in slots) for k in sr.STATS}


def assert_search(eng, slots, tag, key="solver"):
    """Trees, status columns, root statuses and (where the counters were zeroed before the search) the six counters."""
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s[key]["tree"]), tag + (g, "tree")
        assert eng.export_tree_status(g).tobytes() == s[key]["status"].tobytes(), tag + (g, "status")
    assert list(eng.solver_status()) == [s[key]["root_status"] for s in slots], tag


# ---- 1. whole trees and status columns ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("name", ["tictactoe", "connect4", "gomoku7"])
def test_trees_and_status_columns_are_the_restatements(name, mode):
    og, slots = case(name)
    eng = engine_for(name, sr.SIMS)
    noise = load(eng, slots)
    eng.set_solver()
    run_search(eng, mode, sr.SIMS, noise)
    assert_search(eng, slots, (name, mode))
    assert eng.solver_stats() == total(slots), (name, mode)


@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
@pytest.mark.parametrize("group", sorted(sr.WIDE_SLOTS))
def test_wide_roots(group, mode):
    """15 x 15, roots of 56 / 60, 92 and 176 / 184 children - one candidate per lane, two per lane, the general loop - with noise rows (float64
    scores at the root) and without (float32 everywhere): a WON child taken and a LOST child shut out in every form on either path."""
    og, slots, n_sims = sr.wide_group(group)
    eng = engine_for("gomoku15", n_sims)
    noise = load(eng, slots)
    eng.set_solver()
    run_search(eng, mode, n_sims, noise)
    assert_search(eng, slots, (group, mode))
    assert eng.solver_stats() == total(slots), (group, mode)


# ---- 2. nothing stale --------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
def test_nothing_stale(mode):
    """The status column of an arena that has held other trees: a second search after set_positions, a column pre-filled with 0xFF, and
    games recycled in their slots all give the restatement's trees."""
    import torch
    og, slots = case("tictactoe")
    eng = engine_for("tictactoe", sr.SIMS)
    eng.set_solver()
    run_search(eng, mode, sr.SIMS, load(eng, slots))
    assert_search(eng, slots, (mode, "first"))
    other = slots[4:] + slots[:4]                                   # the same arenas, other positions
    run_search(eng, mode, sr.SIMS, load(eng, other))
    assert_search(eng, other, (mode, "second"))
    noise = load(eng, slots)
    eng.fill_solver_status(0xFF)
    run_search(eng, mode, sr.SIMS, noise)
    assert_search(eng, slots, (mode, "prefilled"))
    # play every game to its end, recycle the slots, search the new games' empty boards
    ev, stats = evaluator(9), torch.zeros(8, dtype=torch.int64, device=eng.device)
    done = None
    for _ in range(9):
        done = eng.advance(None, 0)[2]
        if bool(done.bool().all()):
            break
        eng.search(ev, 16, None)
    assert bool(done.bool().all())
    eng.recycle_finished(stats)
    cells, to_move, mc = eng.get_positions()
    assert not cells.any() and not mc.any()
    noise = torch.from_numpy(np.stack([s["noise"] for s in slots])).to(eng.device)
    if mode == "fused":
        eng.search(ev, sr.SIMS, noise)
    else:
        eng.search_budget(ev, sr.SIMS, noise, per_launch=3)
    eng.check_error()
    hev = fr.hash_evaluator(og)
    fresh = [sr.searched(og, hev, np.zeros(9, np.int8), 0, 0, s["noise"], sr.SIMS, want_plain=False) for s in slots]
    assert_search(eng, fresh, (mode, "recycled"))


# ---- 3. nothing changes where nothing is proven ------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
def test_no_terminal_no_change_and_clear_gives_the_plain_engine(mode):
    og, slots = fr.small_case("gomoku7", 24)                        # shallow positions: 24 simulations reach no terminal
    plain = engine_for("gomoku7", 24)
    run_search(plain, mode, 24, load(plain, slots))
    eng = engine_for("gomoku7", 24)
    noise = load(eng, slots)
    eng.set_solver()
    run_search(eng, mode, 24, noise)
    for g, s in enumerate(slots):
        assert fr.same_tree(plain.export_tree(g), s["plain"]["tree"]) and fr.same_tree(eng.export_tree(g), s["plain"]["tree"]), (mode, g)
        assert not eng.export_tree_status(g).any()
    assert not any(eng.solver_stats().values()) and not eng.solver_status().any()
    # clear_solver: the plain engine's trees everywhere, also where the solver changes them
    og, slots = case("tictactoe")
    eng = engine_for("tictactoe", sr.SIMS)
    noise = load(eng, slots)
    eng.set_solver()
    run_search(eng, mode, sr.SIMS, noise)
    assert_search(eng, slots, (mode, "on"))
    noise = load(eng, slots)
    eng.set_solver(False)
    assert eng.solver is False
    run_search(eng, mode, sr.SIMS, noise)
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s["plain"]["tree"]), (mode, g)


# ---- 4. the eval caches ------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
@pytest.mark.parametrize("cache", ["per_game", "shared"])
def test_eval_caches_leave_the_trees_unchanged(cache, mode):
    og, slots = case("tictactoe")
    eng = engine_for("tictactoe", sr.SIMS, cache_entries=64, cache_shared=cache == "shared")
    eng.reset_counters()
    for again in (False, True):                                    # the second search of the same positions finds its leaves in the table
        noise = load(eng, slots)
        eng.set_solver()
        run_search(eng, mode, sr.SIMS, noise)
        assert_search(eng, slots, (cache, mode, again))
        assert eng.solver_stats() == total(slots), (cache, mode, again)
    assert eng.counters()["cache_hits"] > 0


# ---- 5. the runners ----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("game", ["gomoku", "tictactoe"])
def test_async_equals_lockstep_slot_for_slot(game):
    want, lr = lockstep_records(game, MOVES, cap=None, solver=True, cache_entries=64)
    got, ar = async_records(game, MOVES, cap=None, solver=True, cache_entries=64, per_launch=2, steps_per_graph=4)
    assert_same_records(got, want, MOVES, (game,))
    assert lr.eng.solver and ar.eng.solver
    if game == "tictactoe":                                        # the option was on and had something to do
        st = lr.solver_stats()
        assert st["terminal_marked"] > 0 and st["proven_by_won_child"] > 0 and ar.solver_stats()["terminal_marked"] > 0


@gpu
def test_combination_with_cap_resign_value_targets_and_temperature():
    """Playout cap + resignation + value targets + move temperature with the solver on: the asynchronous movers' records, per-ply q record
    and replay ring are the lock-step runner's (games played to their end without restarts; the ring as a multiset of rows)."""
    import azk
    kw = dict(solver=True, resign=(0.9, 0.5), value_target=(0.5, 0.5), move_temperature=("until", 1.0, 6), recycle=False)
    ra, rb = azk.DeviceReplay(8192, 2, 7, 7, 49), azk.DeviceReplay(8192, 2, 7, 7, 49)
    want, lr = lockstep_records("gomoku", 49, cap=(0.5, 6), replay=ra, **kw)
    got, ar = async_records("gomoku", 1, cap=(0.5, 6), replay=rb, per_launch=2, steps_per_graph=4, **kw)
    for _ in range(8000):
        ar.run_chunk()
        if int(ar.finish()[0]) == G:
            break
    ar.check_error()
    assert int(ar.finish()[0]) == G
    assert set(got) == set(want) and all(got[k] == want[k] for k in want)
    assert lr.eng.value_record().cpu().numpy().tobytes() == ar.eng.value_record().cpu().numpy().tobytes()
    assert 0 < int(ra.cursor.item()) == int(rb.cursor.item()) <= 8192 and sorted(ring_rows(ra)) == sorted(ring_rows(rb))
    assert lr.solver_stats()["terminal_marked"] > 0


@gpu
def test_arena_plays_the_wins_it_has_proven():
    """arena.compete_batch(..., solver=True) on TicTacToe: every move made at a root with status "wins" leads to a position that ends the
    game or has status "loses" for the opponent at its next search."""
    import arena
    from fixture_eval import FixtureModel
    ev = FixtureModel(9)
    winners, res = arena.compete_batch("tictactoe", ev, ev, G, 64, 64, seed=SEED, solver=True)
    proven_moves = 0
    for g, r in enumerate(res):
        assert len(r.root_status) == len(r.cells)
        for i, st in enumerate(r.root_status):
            if st == 1:
                proven_moves += 1
                last = i == len(r.cells) - 1
                assert (last and r.winner == i & 1) or (not last and r.root_status[i + 1] == 2), (g, i, r.root_status, r.winner)
    assert proven_moves > 0
    off = arena.compete_batch("tictactoe", ev, ev, G, 64, 64, seed=SEED)[1]
    assert all(r.root_status == [] for r in off)


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_engine_usable():
    import azk
    ARG, STATE = "error -1", "error -4"
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match=ARG):
        vl.set_solver()
    for mode in (1, 2):
        ru = azk.Engine("gomoku", 2, 8, size=7, tree_reuse=mode)
        with pytest.raises(azk.AzkError, match=STATE):
            ru.set_solver()
    og, slots = case("tictactoe")
    eng = engine_for("tictactoe", sr.SIMS)
    L, h = eng.L, eng.h
    out8, out6 = np.zeros(G, np.int8), np.zeros(6, np.int64)
    col = np.zeros(16, np.uint8)
    # the readers while the option is off, and their null pointers
    assert L.azk_get_solver_status(h, out8.ctypes.data, None) == -4 and L.azk_get_solver_stats(h, out6.ctypes.data, None) == -4
    assert L.azk_export_tree_status(h, 0, 16, col.ctypes.data, None) == -4 and L.azk_debug_fill_solver_status(h, 0, None) == -4
    assert L.azk_get_solver_status(h, None, None) == -1 and L.azk_get_solver_stats(h, None, None) == -1
    assert L.azk_export_tree_status(h, 0, 16, None, None) == -1 and L.azk_debug_fill_solver_status(h, 256, None) == -1
    # forced playouts, a Gumbel root and configurable PUCT, in both directions
    eng.set_forced_playouts(2.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_solver()
    eng.set_forced_playouts(0)
    eng.set_gumbel_root(4, 24)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_solver()
    eng.clear_gumbel_root()
    eng.set_puct(2.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_solver()
    eng.clear_puct()
    assert eng.solver is False
    eng.set_solver()
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_forced_playouts(2.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_gumbel_root(4, 24)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_puct(2.0)
    assert eng.forced_playouts is None and eng.gumbel_root is None and eng.puct is None
    assert L.azk_export_tree_status(h, G, 16, col.ctypes.data, None) == -1           # a game index outside the engine
    # vanilla search while the option is set
    assert L.azk_vanilla_search(h, 8, None) == -4
    # between the begin of a search and the call that ends it
    noise = load(eng, slots)
    eng.set_solver()
    eng.begin_search(noise)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_solver()
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_solver(False)
    assert eng.solver is True
    # ... and the engine goes on as if nothing had been asked: the search it had begun, under the option it had
    ev = evaluator(9)
    logits = values = None
    for _ in range(sr.SIMS):
        eng.step(logits, values)
        n = int(eng.n_leaf.item())
        logits, values = eng.evaluate_leaves(ev, n) if n > 0 else (None, None)
    if logits is not None:
        eng.step_expand_backup(logits, values)
    eng.check_error()
    assert_search(eng, slots, ("after refusals",))
    # after azk_async_begin, and re-rooting movers
    from selfplay import AsyncSelfPlayRunner
    r = AsyncSelfPlayRunner("gomoku", evaluator(49), 4, 8, size=7, use_graph=False, solver=True)
    with pytest.raises(azk.AzkError, match=STATE):
        r.eng.set_solver()
    with pytest.raises(azk.AzkError, match=STATE):
        r.eng.set_solver(False)
    r.run_chunk()
    r.finish()
    r.check_error()
    with pytest.raises(ValueError, match="solver"):
        AsyncSelfPlayRunner("gomoku", evaluator(49), 4, 8, size=7, use_graph=False, solver=True, reroot=1)
