"""Configurable PUCT - exploration-rate table and first-play urgency (azk_set_puct) - against the plain-Python restatement
of tests/puct_restated.py: whole trees bit for bit in every stepping mode, in every form of the scan and on both precision paths, the
settings that must change nothing, tree reuse, the eval caches, the asynchronous movers against the lock-step runner, and the refusals.
The positions are those whose preconditions tests/test_puct_restated.py asserts on the CPU."""
import numpy as np
import pytest

import puct_restated as pr
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import assert_same_records, async_records, lockstep_records, shared

gpu = pytest.mark.gpu
G = pr.G
SEED, MOVES, N_SIMS = 3, 12, 24
CAP = (0.5, 6)


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_for(name, n_sims, **kw):
    import azk
    kind, size = pr.GAMES[name] if name in pr.GAMES else ("gomoku", 15)
    return azk.Engine(kind, G, n_sims, size=size, **kw)


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


def assert_trees(eng, slots, key, tag):
    for g, s in enumerate(slots):
        assert pr.same_tree(eng.export_tree(g), s[key]["tree"]), tag + (g,)


# ---- 1. whole trees ------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("n_sims", pr.SIMS)
@pytest.mark.parametrize("name", sorted(pr.GAMES))
def test_trees_are_the_restatements(name, n_sims, mode):
    """The three settings one after the other on one engine: a constant, AlphaZero's schedule with a reduction, a constant with an absolute value."""
    og, slots = pr.small_case(name, n_sims)
    eng = engine_for(name, n_sims)
    for key, (c, fpu) in pr.SETTINGS.items():
        noise = load(eng, slots)                                   # (new positions end the last search: the option is set between searches)
        eng.set_puct(c, fpu)
        run_search(eng, mode, n_sims, noise)
        assert_trees(eng, slots, key, (name, n_sims, mode, key))


@gpu
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("noisy", [True, False])
@pytest.mark.parametrize("i", range(3))
def test_wide_roots(i, noisy, mode):
    """15 x 15 with 48 / 96 / 192 root children: one candidate per lane, two per lane, the general loop - with a noise row (float64 scores at
    the root) and without one (float32 scores everywhere)."""
    og, s = pr.wide_case(i, noisy)
    eng = engine_for("gomoku15", pr.WIDE_SIMS)
    eng.set_puct(*pr.SETTINGS[pr.WIDE_SETTING])
    noise = load(eng, [s] * G)
    run_search(eng, mode, pr.WIDE_SIMS, noise)
    for g in (0, G - 1):
        assert pr.same_tree(eng.export_tree(g), s[pr.WIDE_SETTING]["tree"]), (i, noisy, mode, g)


@gpu
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("noisy", [True, False])
def test_more_children_than_one_pass_holds(noisy, mode):
    """20 x 20 with 273 root children: the kernels for boards beyond 256 cells, and the visited mass summed in a pass of its own."""
    import azk
    og, s = pr.huge_case(noisy)
    eng = azk.Engine("gomoku", G, pr.HUGE_SIMS, size=pr.HUGE_SIZE)
    eng.set_puct(*pr.SETTINGS[pr.WIDE_SETTING])
    noise = load(eng, [s] * G)
    run_search(eng, mode, pr.HUGE_SIMS, noise)
    for g in (0, G - 1):
        assert pr.same_tree(eng.export_tree(g), s[pr.WIDE_SETTING]["tree"]), (noisy, mode, g)


# ---- 2. the settings that change nothing ------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
def test_c_one_and_clear_give_the_trees_of_an_engine_without_the_option(mode):
    og, slots = pr.small_case("gomoku7", 24)
    plain = engine_for("gomoku7", 24)
    run_search(plain, mode, 24, load(plain, slots))
    want = [plain.export_tree(g) for g in range(G)]
    for g, s in enumerate(slots):
        assert pr.same_tree(want[g], s["plain"]["tree"]), g
    eng = engine_for("gomoku7", 24)
    eng.set_puct(1.0)
    assert eng.puct is not None
    run_search(eng, mode, 24, load(eng, slots))
    for g in range(G):
        assert pr.same_tree(eng.export_tree(g), want[g]), (mode, g)
    noise = load(eng, slots)
    eng.set_puct(*pr.SETTINGS["c1.5_absolute"])
    run_search(eng, mode, 24, noise)
    assert_trees(eng, slots, "c1.5_absolute", (mode,))
    noise = load(eng, slots)
    eng.clear_puct()
    assert eng.puct is None
    run_search(eng, mode, 24, noise)
    for g in range(G):
        assert pr.same_tree(eng.export_tree(g), want[g]), (mode, g)


# ---- 3. tree reuse ----------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("key", ["az_reduction", "c1.5_absolute"])
def test_tree_reuse_carries_the_subtree_into_the_next_search(key):
    """Carry, two moves into a Gomoku 7x7 game: each search's tree is the restatement's search started from the carried subtree - the rule
    reads only what the tree stores, so a re-rooted tree needs nothing more."""
    import azk
    og = pr.oracle_game("gomoku7")
    ev = pr.hash_evaluator(og)
    setting = pr.setting_of(key)
    eng = azk.Engine("gomoku", G, N_SIMS, size=7, tree_reuse=1)
    eng.set_puct(*pr.SETTINGS[key])
    eng.reset_games()
    roots, chosen = [None] * G, None
    for mv in range(3):
        noise, uni = eng.gen_noise(SEED, 0, mv, 0.3)
        nz = noise.cpu().numpy()
        cells, to_move, mc = eng.get_positions()
        eng.search(evaluator(49), N_SIMS, noise)
        for g in range(G):
            root = pr.carry(og, roots[g], int(chosen[g]), nz[g]) if roots[g] is not None else None
            if mv > 0:
                assert root is not None, (g, mv)                   # (24 simulations over one or a few moves: the played child was expanded)
            if root is None:
                root = pr.RNode(None, None, int(to_move[g]), int(mc[g]))
            pr.mcts(og, root, og.board_from_cells(cells[g], to_move[g]), N_SIMS, ev, nz[g], setting)
            assert pr.same_tree(eng.export_tree(g), pr.export(root)), (key, g, mv)
            roots[g] = root
        chosen = eng.advance(uni, 8)[0].cpu().numpy()
    eng.check_error()
    assert eng.counters()["roots_reused"] > 0


# ---- 4. the eval caches -----------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
@pytest.mark.parametrize("cache", ["per_game", "shared"])
def test_eval_caches_leave_the_trees_unchanged(cache, mode):
    og, slots = pr.small_case("gomoku7", 64)
    eng = engine_for("gomoku7", 64, cache_entries=64, cache_shared=cache == "shared")
    eng.set_puct(*pr.SETTINGS["az_reduction"])
    eng.reset_counters()
    for again in (False, True):                                    # the second search of the same positions finds its leaves in the table
        run_search(eng, mode, 64, load(eng, slots))
        assert_trees(eng, slots, "az_reduction", (cache, mode, again))
    assert eng.counters()["cache_hits"] > 0


# ---- 5. the runners ---------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("extras", ["none", "reroot2", "cap_resign_symmetry"])
def test_async_equals_lockstep_slot_for_slot(extras):
    puct = pr.SETTINGS["az_reduction"]
    lock_kw, async_kw, cap = dict(cache_entries=64), dict(cache_entries=64, per_launch=2, steps_per_graph=4), None
    if extras == "reroot2":
        lock_kw["tree_reuse"], async_kw["reroot"] = 2, 2
    if extras == "cap_resign_symmetry":
        cap = CAP
        lock_kw["resign"] = async_kw["resign"] = (0.25, 0.5)
        lock_kw["eval_symmetry"] = async_kw["eval_symmetry"] = True
    want, _ = lockstep_records("gomoku", MOVES, cap=cap, puct=puct, **lock_kw)
    got, _ = async_records("gomoku", MOVES, cap=cap, puct=puct, **async_kw)
    assert_same_records(got, want, MOVES, (extras,))
    off = shared(("puct off", extras), lambda: lockstep_records("gomoku", MOVES, cap=cap, **lock_kw)[0])
    assert any(want[k][0] != off[k][0] for k in want if k in off)                  # the option was on: recorded pi differ


@gpu
def test_self_play_batch_and_the_arena_take_the_option():
    import arena
    from fixture_eval import FixtureModel
    from selfplay import self_play_batch
    ev = FixtureModel(49)
    on = self_play_batch("gomoku", ev, 4, 16, size=7, seed=SEED, puct=pr.SETTINGS["c1.5_absolute"], max_moves=4)
    off = self_play_batch("gomoku", ev, 4, 16, size=7, seed=SEED, max_moves=4)
    one = self_play_batch("gomoku", ev, 4, 16, size=7, seed=SEED, puct=(1.0, None), max_moves=4)
    assert all(a.pis[i].tobytes() == b.pis[i].tobytes() for a, b in zip(off, one) for i in range(len(a.pis)))
    assert any(a.pis[i].tobytes() != b.pis[i].tobytes() for a, b in zip(off, on) for i in range(min(len(a.pis), len(b.pis))))
    w_on, _ = arena.compete_batch("gomoku", ev, ev, 4, 16, 16, size=7, seed=SEED, puct=pr.SETTINGS["az_reduction"])
    assert len(w_on) == 4 and set(int(w) for w in w_on) <= {0, 1, -1}


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_leave_the_engine_usable():
    import azk
    ARG, STATE = "error -1", "error -4"
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match=ARG):
        vl.set_puct(2.0)
    og, slots = pr.small_case("gomoku7", 24)
    eng = engine_for("gomoku7", 24)
    L, h = eng.L, eng.h
    good = np.array([1.0, 2.0], np.float64)
    p = good.ctypes.data
    for args in ((None, 2, 0, 0.0, 0.0), (p, 0, 0, 0.0, 0.0), (p, 65537, 0, 0.0, 0.0), (p, 2, -1, 0.0, 0.0), (p, 2, 3, 0.0, 0.0),
                 (p, 2, 1, float("nan"), 0.0), (p, 2, 1, 0.0, float("inf")), (p, 2, 2, -0.5, 0.0), (p, 2, 2, 0.5, -0.5)):
        assert L.azk_set_puct(h, *args, None) == -1, args
    for bad in (-1.0, float("nan"), float("inf")):
        tab = np.array([1.0, bad], np.float64)
        assert L.azk_set_puct(h, tab.ctypes.data, 2, 0, 0.0, 0.0, None) == -1, bad
    assert L.azk_set_puct(h, p, 2, 1, -1.0, 0.5, None) == 0           # (a negative ABSOLUTE value is a value like any other)
    assert L.azk_clear_puct(h) == 0
    with pytest.raises(ValueError, match="puct"):
        eng.set_puct(-1.0)
    assert eng.puct is None
    # forced playouts and a Gumbel root, in both directions
    eng.set_forced_playouts(2.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_puct(2.0)
    eng.set_forced_playouts(0)
    eng.set_gumbel_root(4, 24)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_puct(2.0)
    eng.clear_gumbel_root()
    eng.set_puct(2.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_forced_playouts(2.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_gumbel_root(4, 24)
    assert eng.forced_playouts is None and eng.gumbel_root is None
    # vanilla search while the option is set
    assert L.azk_vanilla_search(h, 8, None) == -4
    # between the begin of a search and the call that ends it
    eng.set_puct(*pr.SETTINGS["c2.5"])
    noise = load(eng, slots)
    eng.begin_search(noise)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.set_puct(1.0)
    with pytest.raises(azk.AzkError, match=STATE):
        eng.clear_puct()
    assert eng.puct is not None
    # ... and the engine goes on as if nothing had been asked: the search it had begun, under the setting it had
    ev = evaluator(49)
    logits = values = None
    for _ in range(24):
        eng.step(logits, values)
        n = int(eng.n_leaf.item())
        logits, values = eng.evaluate_leaves(ev, n) if n > 0 else (None, None)
    if logits is not None:
        eng.step_expand_backup(logits, values)
    eng.check_error()
    assert_trees(eng, slots, "c2.5", ("after refusals",))
    # after azk_async_begin
    from selfplay import AsyncSelfPlayRunner
    r = AsyncSelfPlayRunner("gomoku", ev, 4, 8, size=7, use_graph=False, puct=(2.0, None))
    with pytest.raises(azk.AzkError, match=STATE):
        r.eng.set_puct(1.0)
    with pytest.raises(azk.AzkError, match=STATE):
        r.eng.clear_puct()
    r.run_chunk()
    r.finish()
    r.check_error()
