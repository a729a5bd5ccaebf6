"""Forced playouts and policy target pruning at the root (azk_set_forced_playouts) against the plain-Python restatement of
tests/forced_playouts_restated.py: whole trees bit for bit in every stepping mode and in every form of the root scan, the pruned pi, what
the movers record and emit, the combination with the playout cap, the asynchronous movers against the lock-step runner, and the refusals.
The positions are those whose preconditions tests/test_forced_playouts_restated.py asserts on the CPU."""
import numpy as np
import pytest

import forced_playouts_restated as fr
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import assert_same_records, async_records, coin_full, lockstep_records, ring_rows, shared

gpu = pytest.mark.gpu
K, G = fr.K, fr.G
SEED, MOVES, N_SIMS = 3, 12, 24
CAP = (0.5, 6)
CAP_PLIES = 4


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_for(name, n_sims, **kw):
    import azk
    kind, size = fr.GAMES[name] if name in fr.GAMES else ("gomoku", 15)
    return azk.Engine(kind, G, n_sims, size=size, **kw)


def load(eng, slots):
    """The slots' positions into the engine; returns their noise rows as a CUDA tensor."""
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
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


def check_targets(eng, og, k):
    """root_policy_target() against prune() on what azk_root_children and the root visit count say, bit for bit."""
    tgt = eng.root_policy_target().cpu().numpy()
    visits = eng.root_stats()[2].cpu().numpy()
    for g in range(eng.G):
        want = fr.root_target(og, eng.root_children(g), int(visits[g]), k)
        assert tgt[g].tobytes() == want.tobytes(), g
    return tgt


# ---- 1. selection: whole trees; 3. pruning on the same searches ----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("n_sims", fr.SIMS)
@pytest.mark.parametrize("name", sorted(fr.GAMES))
def test_trees_and_targets_are_the_restatements(name, n_sims, mode):
    og, slots = fr.small_case(name, n_sims)
    eng = engine_for(name, n_sims)
    eng.set_forced_playouts(K)
    noise = load(eng, slots)
    eng.reset_counters()
    run_search(eng, mode, n_sims, noise)
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s["forced"]["tree"]), (name, n_sims, mode, g)
    tgt = check_targets(eng, og, K)
    raw = eng.root_stats()[0].cpu().numpy()
    for g, s in enumerate(slots):
        assert tgt[g].tobytes() == s["forced"]["target"].tobytes() and tgt[g].tobytes() != raw[g].tobytes(), g
    c = eng.counters()
    assert c["forced_selections"] == sum(len(s["forced"]["log"]) for s in slots) and c["visits_pruned"] == 0      # (nothing has moved yet)


# ---- 2. the three forms of the root scan -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "budget"])
@pytest.mark.parametrize("i", range(3))
def test_wide_roots(i, mode):
    """15 x 15 with 48 / 96 / 192 root children: one candidate per lane, two per lane, the general loop."""
    og, s = fr.wide_case(i)
    eng = engine_for("gomoku15", fr.WIDE_SIMS)
    eng.set_forced_playouts(K)
    noise = load(eng, [s] * G)
    run_search(eng, mode, fr.WIDE_SIMS, noise)
    for g in (0, G - 1):
        assert fr.same_tree(eng.export_tree(g), s["forced"]["tree"]), (i, mode, g)
    tgt = check_targets(eng, og, K)
    assert tgt[0].tobytes() == s["forced"]["target"].tobytes()


# ---- 3. pruning, on any engine state ------------------------------------------------------------------------------------------------------
@gpu
def test_targets_on_a_reused_tree_two_moves_into_a_game():
    import azk
    og = fr.oracle_game("gomoku7")
    eng = azk.Engine("gomoku", G, N_SIMS, size=7, tree_reuse=1)
    eng.set_forced_playouts(K)
    eng.reset_games()
    for mv in range(3):
        noise, uni = eng.gen_noise(SEED, 0, mv, 0.3)
        eng.search(evaluator(49), N_SIMS, noise)
        tgt = check_targets(eng, og, K)
        if mv == 2:
            assert eng.counters()["roots_reused"] > 0
            assert tgt.tobytes() != eng.root_stats()[0].cpu().numpy().tobytes()
        eng.advance(uni, 8)
    eng.check_error()


@gpu
def test_k0_target_is_root_stats_pi():
    og, slots = fr.small_case("gomoku7", 24)
    eng = engine_for("gomoku7", 24)
    noise = load(eng, slots)
    run_search(eng, "fused", 24, noise)
    assert eng.root_policy_target().cpu().numpy().tobytes() == eng.root_stats()[0].cpu().numpy().tobytes()
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s["plain"]["tree"]), g


# ---- 4. records ---------------------------------------------------------------------------------------------------------------------------
def manual_records(moves, replay):
    """An engine driven as SelfPlayRunner(recycle=True) drives its own, with a look at the raw counts and the target before every move:
    {(slot, move): (target bytes, q, cell, winner)}; and per finished game (first stream index, boards, targets, winner)."""
    import azk
    import torch
    from oracle import az_oracle as ao
    from selfplay import SAMPLE_UNTIL, cells_to_board
    eng = azk.Engine("gomoku", G, N_SIMS, size=7)
    eng.set_forced_playouts(K)
    eng.reset_games()
    stats = torch.zeros(8, dtype=torch.int64, device=eng.device)
    rec, games, open_games = {}, [], [([], []) for _ in range(G)]
    for mv in range(moves):
        noise, uni = eng.gen_noise(SEED, 0, mv)
        eng.search(evaluator(49), N_SIMS, noise)
        raw, q, _ = eng.root_stats()
        raw, q, uni_h = raw.cpu().numpy(), q.cpu().numpy(), uni.cpu().numpy()
        tgt = eng.root_policy_target().cpu().numpy().copy()
        cells, to_move, mc = eng.get_positions()
        children = [eng.root_children(g) for g in range(G)]
        chosen, winner, done = [t.cpu().numpy().copy() for t in eng.advance(uni, SAMPLE_UNTIL["gomoku"])]
        bases = eng.emit_finished(replay).cpu().numpy()
        eng.recycle_finished(stats)
        for g in range(G):
            # the move: from RAW visits and the same uniform
            if mc[g] < SAMPLE_UNTIL["gomoku"]:
                want = ao.sample_action(raw[g], uni_h[g])
            else:
                want = int(children[g]["cell"][int(np.argmax(children[g]["visit"]))])
            assert int(chosen[g]) == want, (g, mv)
            rec[(g, mv)] = (tgt[g].tobytes(), float(q[g]), int(chosen[g]), int(winner[g]))
            open_games[g][0].append(cells_to_board(cells[g], 2, 7, 7, to_move[g]))
            open_games[g][1].append(tgt[g])
        for g in range(G):
            if done[g]:
                games.append((int(bases[g]), open_games[g][0], open_games[g][1], int(winner[g])))
                open_games[g] = ([], [])
    eng.check_error()
    return rec, games


@gpu
def test_runner_records_and_emission_carry_the_pruned_pi():
    import azk
    from oracle import replay_oracle as ro
    from selfplay import SelfPlayRunner
    moves = 40
    ra, rb = azk.DeviceReplay(1 << 14, 2, 7, 7, 49), azk.DeviceReplay(1 << 14, 2, 7, 7, 49)
    want, games = manual_records(moves, ra)
    assert len(games) > 0
    # what advance recorded and emitted: the D4 images of the targets read before each move
    tuples = {}
    for base, boards, pis, w in games:
        for i, t in enumerate(ro.emit_tuples(boards, pis, w)):
            assert base + i not in tuples
            tuples[base + i] = t
    assert int(ra.cursor.item()) == len(tuples) <= ra.capacity and sorted(tuples) == list(range(len(tuples)))
    s, p, z = ra.states.cpu().numpy(), ra.pis.cpu().numpy(), ra.zs.cpu().numpy()
    for t, (st, pi, zz) in tuples.items():
        assert s[t].tobytes() == np.ascontiguousarray(st, np.float32).tobytes() and p[t].tobytes() == np.ascontiguousarray(pi, np.float64).tobytes(), t
        assert float(z[t]) == zz, t
    # the runner plays and records the same
    got = {}

    def on(mv, base, pi, q, ch, w, d):
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                got[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]))
    r = SelfPlayRunner("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, on_records=on, recycle=True, replay=rb, forced_playouts=K)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    assert got == want
    assert sorted(ring_rows(ra)) == sorted(ring_rows(rb))
    c = r.counters()
    assert c["forced_selections"] > 0 and 0 < c["visits_pruned"] < c["visits_before_pruning"]


# ---- 5. with the playout cap ------------------------------------------------------------------------------------------------------------------
def test_precondition_the_cap_plies_are_of_both_kinds():
    """CPU: among the G x CAP_PLIES searches of the capped test both kinds occur."""
    flags = [coin_full(SEED, g, mv, CAP[0]) for g in range(G) for mv in range(CAP_PLIES)]
    assert 0 < sum(flags) < len(flags)


@gpu
def test_with_the_cap_full_plies_are_forced_and_fast_plies_are_not():
    import azk
    from oracle import az_oracle as ao
    og = fr.oracle_game("gomoku7")
    ev = fr.hash_evaluator(og)
    eng = azk.Engine("gomoku", G, N_SIMS, size=7)
    eng.set_playout_cap(CAP[0], CAP[1], SEED, 0)
    eng.set_forced_playouts(K)
    eng.reset_games()
    kinds, pruned_full, lock = [], 0, {}
    for mv in range(CAP_PLIES):
        noise, uni = eng.gen_noise(SEED, 0, mv)
        noise_h = noise.cpu().numpy()
        eng.search_budget(evaluator(49), N_SIMS, noise, move_index=mv)
        full = eng.search_full().cpu().numpy().copy()
        cells, to_move, mc = eng.get_positions()
        raw = eng.root_stats()[0].cpu().numpy()
        visits = eng.root_stats()[2].cpu().numpy()
        tgt = eng.root_policy_target().cpu().numpy()
        for g in range(G):
            assert bool(full[g]) == coin_full(SEED, g, mv, CAP[0])
            board = og.board_from_cells(cells[g], to_move[g])
            if full[g]:
                root = fr.RNode(None, None, int(to_move[g]), int(mc[g]))
                fr.mcts(og, root, board, N_SIMS, ev, noise_h[g], K)
                want = fr.export(root)
                assert tgt[g].tobytes() == fr.root_target(og, eng.root_children(g), int(visits[g]), K).tobytes(), (g, mv)
                pruned_full += tgt[g].tobytes() != raw[g].tobytes()
            else:
                tree = ao.OracleTree(og)
                tree.reset(int(to_move[g]), int(mc[g]))
                ao.mcts(og, tree, board, CAP[1], ev, noise_h[g])
                want = tree.export()
                assert tgt[g].tobytes() == raw[g].tobytes(), (g, mv)      # a fast search's record keeps raw counts
            assert fr.same_tree(eng.export_tree(g), want), (g, mv, int(full[g]))
            kinds.append(int(full[g]))
            lock[(g, mv)] = (raw[g].tobytes(), tgt[g].tobytes(), int(full[g]))
        chosen = eng.advance(uni, 8)[0].cpu().numpy()
        for g in range(G):
            lock[(g, mv)] += (int(chosen[g]),)
    eng.check_error()
    assert 0 < sum(kinds) < len(kinds)
    assert pruned_full > 0                                         # the full plies were positions on which the option shows
    # (the lock-step traj_pi of a fast ply is never emitted, so nothing reads it back; k_advance and k_move_async record through the
    #  one advance_one, and the ring below is that function's output)
    # the record itself, as the capped mover writes it (the asynchronous ring's rec_pi; same keys, so the same games): a fast ply's
    # holds the RAW counts, a full ply's the pruned ones
    got, _ = async_records("gomoku", CAP_PLIES, cap=CAP, forced_playouts=K, per_launch=2, steps_per_graph=4)
    for (g, mv), (raw_b, tgt_b, full_flag, cell) in lock.items():
        pi_b, _, cell_a, _, full_a = got[(g, mv)]
        assert (cell_a, full_a) == (cell, full_flag), (g, mv)
        assert pi_b == (tgt_b if full_flag else raw_b), (g, mv, full_flag)


# ---- 6. the asynchronous movers ------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("extras", ["none", "reroot2", "cap_resign"])
def test_async_equals_lockstep_slot_for_slot(extras):
    lock_kw, async_kw, cap = dict(cache_entries=64), dict(cache_entries=64, per_launch=2, steps_per_graph=4), None
    if extras == "reroot2":
        lock_kw["tree_reuse"], async_kw["reroot"] = 2, 2
    if extras == "cap_resign":
        cap = CAP
        lock_kw["resign"] = async_kw["resign"] = (0.25, 0.5)
    want, _ = lockstep_records("gomoku", MOVES, cap=cap, forced_playouts=K, **lock_kw)
    got, r = async_records("gomoku", MOVES, cap=cap, forced_playouts=K, **async_kw)
    assert_same_records(got, want, MOVES, (extras,))
    off = shared(("fp off", extras), lambda: lockstep_records("gomoku", MOVES, cap=cap, **lock_kw)[0])
    assert any(want[key][0] != off[key][0] for key in want if key in off)          # the option was on: recorded pi differ
    assert r.counters()["visits_pruned"] > 0


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_refusals_and_switching_off():
    import azk
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="error -1"):
        vl.set_forced_playouts(K)
    og, slots = fr.small_case("gomoku7", 24)
    eng = engine_for("gomoku7", 24)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(azk.AzkError, match="error -1"):
            eng.set_forced_playouts(bad)
    assert eng.forced_playouts is None
    eng.set_forced_playouts(K)
    with pytest.raises(azk.AzkError, match="error -4"):
        eng.begin_search(None)
    with pytest.raises(azk.AzkError, match="error -4"):
        eng.begin_search_budget(None, 24)
    eng.set_forced_playouts(0)
    noise = load(eng, slots)
    run_search(eng, "fused", 24, noise)
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s["plain"]["tree"]), g
    run_search(eng, "budget", 24, noise)
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s["plain"]["tree"]), g
    eng.begin_search(None)                                         # and the noise-free search is accepted again
    eng.check_error()
