"""Gumbel root search (azk_set_gumbel_root) against the plain-Python restatement of tests/gumbel_restated.py: whole trees bit for
bit in every stepping mode, cache mode and form of the root scan, the move and the float64 target, the Gumbel rows, what the movers record
and emit, the runners (lock-step against an engine-level loop, asynchronous against lock-step), and the refusals.  The positions are those
whose preconditions tests/test_gumbel_restated.py asserts on the CPU.

Target bound (gr.target_bound; derived, not taken from the kernel): |dy| <= sigf * (n + 8) * 2^-53, an entry's relative error
<= 2 |dy| + 4 (n + 4) * 2^-52.  Largest error / bound seen on an MI355X: see DESIGN section 24."""
import numpy as np
import pytest

import forced_playouts_restated as fr
import gumbel_restated as gr
import rng_restated as rr
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import assert_same_records, async_records, lockstep_records, ring_rows, shared

gpu = pytest.mark.gpu
G, CV, CS = gr.G, gr.C_VISIT, gr.C_SCALE
SEED, MOVES, N_SIMS, M = 3, 12, 17, 4
GUM = (M, CV, CS)
CACHES = {"off": {}, "per_game": dict(cache_entries=64), "shared": dict(cache_entries=64, cache_shared=True)}
seen = {"target": 0.0, "rows": 0.0}            # largest error / bound (target) and largest scaled row error met in this process


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine_for(name, n_sims, m, **kw):
    import azk
    kind, size = gr.GAMES[name] if name in gr.GAMES else ("gomoku", 15)
    eng = azk.Engine(kind, G, n_sims, size=size, **kw)
    eng.set_gumbel_root(m, n_sims, CV, CS)
    return eng


def load(eng, slots):
    """The slots' positions into the engine; returns their Gumbel rows as a CUDA tensor."""
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
    return torch.from_numpy(np.stack([s["row"] for s in slots])).to(eng.device)


def run_search(eng, mode, n_sims, rows, ev=None):
    ev = ev or evaluator(eng.action_dim)
    if mode == "fused":                                            # select-only first launch, fused launches, expand-only last launch
        eng.search(ev, n_sims, rows)
    elif mode == "split":                                          # select-only and expand-only launches alone
        eng.begin_search(rows)
        for _ in range(n_sims):
            eng.step_select()
            n = int(eng.n_leaf.item())
            if n > 0:
                eng.step_expand_backup(*eng.evaluate_leaves(ev, n))
            elif eng.cache_entries:
                eng.step_expand_backup(*eng.placeholder_rows())
    else:                                                          # budget stepping: the MULTI kernel
        eng.search_budget(ev, n_sims, rows, per_launch=3)
    eng.check_error()


def assert_target(got, s, tag):
    """One game's root_policy_target() row against the restated target: zero where the restatement is zero, within the derived bound elsewhere."""
    want = s["target"]
    bound = gr.target_bound(s["sigf"], len(s["children"]["cell"]))
    assert np.array_equal(got == 0.0, want == 0.0), tag
    nz = want != 0.0
    err = float(np.max(np.abs(got[nz] - want[nz]) / want[nz]))
    seen["target"] = max(seen["target"], err / bound)
    print(f"target {tag}: rel err {err:.3e} bound {bound:.3e} ratio {err / bound:.4f}")
    assert err <= bound, (tag, err, bound)


def check_moves_and_targets(eng, og, slots, tag):
    raw = eng.root_stats()[0].cpu().numpy()
    tgt = eng.root_policy_target().cpu().numpy().copy()
    for g, s in enumerate(slots):
        assert raw[g].tobytes() == fr.pi_of(og, s["children"]["cell"], s["children"]["visit"]).tobytes(), tag + (g,)     # root_stats: raw visits
        assert_target(tgt[g], s, tag + (g,))
    chosen = eng.advance(None, 8)[0].cpu().numpy()
    assert [int(c) for c in chosen] == [s["move"] for s in slots], tag
    eng.check_error()


# ---- 1. whole trees, the move and the target ---------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("cache", sorted(CACHES))
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("n_sims,m", gr.CASES)
@pytest.mark.parametrize("name", sorted(gr.GAMES))
def test_trees_moves_and_targets_are_the_restatements(name, n_sims, m, mode, cache):
    og, slots = gr.small_case(name, n_sims, m)
    eng = engine_for(name, n_sims, m, **CACHES[cache])
    rows = load(eng, slots)
    run_search(eng, mode, n_sims, rows)
    for g, s in enumerate(slots):
        assert fr.same_tree(eng.export_tree(g), s["tree"]), (name, n_sims, mode, cache, g)
    check_moves_and_targets(eng, og, slots, (name, n_sims, mode, cache))


# ---- 2. the three forms of the root scan -----------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("mode", ["fused", "split", "budget"])
@pytest.mark.parametrize("i", range(3))
def test_wide_roots(i, mode):
    """15 x 15 with 48 / 96 / 192 root children: one candidate per lane, two per lane, the general loop; the Gumbel rows put the top m on high
    list indices."""
    og, s = gr.wide_case(i)
    eng = engine_for("gomoku15", gr.WIDE_SIMS, gr.WIDE_M)
    rows = load(eng, [s] * G)
    run_search(eng, mode, gr.WIDE_SIMS, rows)
    for g in (0, G - 1):
        assert fr.same_tree(eng.export_tree(g), s["tree"]), (i, mode, g)
    check_moves_and_targets(eng, og, [s] * G, ("wide", i, mode))


# ---- 3. the Gumbel rows ------------------------------------------------------------------------------------------------------------------------
ROW_SETS = [("gomoku", 7, 49, 0x0123456789ABCDEF, 100, 1), ("gomoku", 15, 225, 7, 2 ** 32 - 2, 511), ("connect4", None, 7, 2 ** 64 - 1, 0, 0),
            ("gomoku", 20, 400, 0, 100, 3)]


@gpu
@pytest.mark.parametrize("game,size,A,seed,first,move", ROW_SETS, ids=[f"{g}-{s}-{mv}" for g, s, _, _, _, mv in ROW_SETS])
def test_gumbel_rows_are_the_restated_chain(game, size, A, seed, first, move):
    import azk
    eng = azk.Engine(game, G, 8, size=size)
    noise0, uni0 = [t.cpu().numpy().copy() for t in eng.gen_noise(seed, first, move, 0.3)]
    u = eng.gen_gumbel(seed, first, move, uniforms=True).cpu().numpy()
    assert u.tobytes() == gr.gumbel_uniforms(A, seed, first, G, move).tobytes()          # the uniforms underneath: bit for bit
    got, want = eng.gen_gumbel(seed, first, move).cpu().numpy(), gr.gumbel_rows(A, seed, first, G, move)
    err = float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want))))
    seen["rows"] = max(seen["rows"], err)
    print(f"gumbel rows {game} {size}: largest scaled error {err:.3e}")
    assert err <= 1e-12
    # the other streams of the same keys are what they were: word 3 = 0xFFFFFFFB is no other draw's
    noise1, uni1 = [t.cpu().numpy() for t in eng.gen_noise(seed, first, move, 0.3)]
    assert noise1.tobytes() == noise0.tobytes() and uni1.tobytes() == uni0.tobytes()
    assert uni1.tobytes() == rr.move_uniform(seed, np.arange(G, dtype=np.uint64) + np.uint64(first), move).tobytes()
    assert not np.array_equal(u[:, 0], uni1) and not np.array_equal(u[:, 0], rr.coin(seed, np.arange(G, dtype=np.uint64) + np.uint64(first), move))
    eng.check_error()


# ---- 4. records, emission and the lock-step runner -------------------------------------------------------------------------------------------
def manual_records(moves, replay):
    """An engine driven as SelfPlayRunner(recycle=True) drives its own, with the restated search of every position before every move:
    {(slot, move): (target bytes, q, cell, winner)}; and per finished game (first stream index, boards, targets, winner)."""
    import azk
    import torch
    from selfplay import cells_to_board
    og = fr.oracle_game("gomoku7")
    ev = gr.logits_evaluator(og)
    eng = azk.Engine("gomoku", G, N_SIMS, size=7)
    eng.set_gumbel_root(M, N_SIMS, CV, CS)
    eng.reset_games()
    stats = torch.zeros(8, dtype=torch.int64, device=eng.device)
    rec, games, open_games = {}, [], [([], []) for _ in range(G)]
    for mv in range(moves):
        rows = eng.gen_gumbel(SEED, 0, mv)
        rows_h = rows.cpu().numpy()
        assert rows_h.tobytes() != np.zeros_like(rows_h).tobytes()
        eng.search(evaluator(49), N_SIMS, rows)
        raw, q, _ = eng.root_stats()
        raw, q = raw.cpu().numpy(), q.cpu().numpy()
        tgt = eng.root_policy_target().cpu().numpy().copy()
        cells, to_move, mc = eng.get_positions()
        chosen, winner, done = [t.cpu().numpy().copy() for t in eng.advance(None, 8)]
        bases = eng.emit_finished(replay).cpu().numpy()
        eng.recycle_finished(stats)
        for g in range(G):
            s = gr.searched(og, ev, cells[g], int(to_move[g]), int(mc[g]), rows_h[g], N_SIMS, M)
            assert int(chosen[g]) == s["move"], (g, mv)
            assert_target(tgt[g], s, ("loop", g, mv))
            assert raw[g].tobytes() == fr.pi_of(og, s["children"]["cell"], s["children"]["visit"]).tobytes()
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
def test_runner_records_and_emission_carry_the_gumbel_target():
    import azk
    from oracle import replay_oracle as ro
    from selfplay import SelfPlayRunner
    moves = 36
    ra, rb = azk.DeviceReplay(1 << 14, 2, 7, 7, 49), azk.DeviceReplay(1 << 14, 2, 7, 7, 49)
    want, games = manual_records(moves, ra)
    assert len(games) > 0
    # what advance recorded and emitted: the D4 images of root_policy_target()'s rows read before each move, bit for bit
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
    r = SelfPlayRunner("gomoku", evaluator(49), G, N_SIMS, size=7, seed=SEED, on_records=on, recycle=True, replay=rb, gumbel_root=GUM)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    assert got == want
    assert sorted(ring_rows(ra)) == sorted(ring_rows(rb))


@gpu
def test_graph_runner_with_budget_stepping_equals_the_eager_runner():
    want, _ = lockstep_records("gomoku", 6, n_sims=N_SIMS, cap=None, gumbel_root=GUM)
    got, _ = lockstep_records("gomoku", 6, n_sims=N_SIMS, cap=None, gumbel_root=GUM, use_graph=True, budget_stepping=True, per_launch=2, steps_per_graph=4,
                              cache_entries=64)
    assert got == want


# ---- 5. the asynchronous movers --------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("extras", ["plain", "resign"])
def test_async_equals_lockstep_slot_for_slot(extras):
    kw = dict(resign=(0.25, 0.5)) if extras == "resign" else {}
    want, _ = lockstep_records("gomoku", MOVES, n_sims=N_SIMS, cap=None, gumbel_root=GUM, **kw)
    got, r = async_records("gomoku", MOVES, n_sims=N_SIMS, cap=None, gumbel_root=GUM, per_launch=2, steps_per_graph=4, **kw)
    assert_same_records(got, want, MOVES, (extras,))
    off = shared(("gumbel off", extras), lambda: lockstep_records("gomoku", MOVES, n_sims=N_SIMS, cap=None, **kw)[0])
    assert any(want[key][0] != off[key][0] for key in want if key in off)          # the option was on: recorded pi differ


# ---- 6. with evaluation symmetry and with emission under a mask ---------------------------------------------------------------------------------
@gpu
def test_fixed_eval_symmetry_is_the_restatement_on_the_wrapped_evaluator():
    import azk
    import eval_symmetry_restated as es
    og, slots = gr.small_case("gomoku7", 17, 4)
    wrapped = es.wrap(evaluator(49), "gomoku", 7, 7, 2, 3)
    ev = gr.logits_evaluator(og, wrapped)
    eng = azk.Engine("gomoku", G, 17, size=7, eval_symmetry=("fixed", 3))
    eng.set_gumbel_root(4, 17, CV, CS)
    rows = load(eng, slots)
    run_search(eng, "fused", 17, rows)
    want = [gr.searched(og, ev, s["cells"], s["to_move"], s["move_count"], s["row"], 17, 4) for s in slots]
    assert any(not fr.same_tree(w["tree"], s["tree"]) for w, s in zip(want, slots))      # the orientation shows
    for g, w in enumerate(want):
        assert fr.same_tree(eng.export_tree(g), w["tree"]), g
    check_moves_and_targets(eng, og, want, ("sym",))


@gpu
def test_non_square_board_emission_carries_the_gumbel_target():
    from selfplay import self_play_batch
    from test_gpu_emit_symmetry import assert_ring, expected_stream, new_ring, ring_numpy
    size, A = (5, 7), 35
    rp = new_ring("gomoku", size, 4096)
    res = self_play_batch("gomoku", evaluator(A), 4, N_SIMS, size=size, seed=5, replay=rp, emit_symmetry="board", gumbel_root=GUM)
    stream, end = expected_stream("gomoku", size, "board", res)
    assert_ring(ring_numpy(rp), int(rp.cursor.item()), stream, end, 4096)
    for r in res:
        for pi in r.pis:
            assert abs(float(np.sum(pi)) - 1.0) < 1e-12 and (np.asarray(pi) >= 0).all()
    assert any(int((np.asarray(pi) > 0).sum()) > M for r in res for pi in r.pis)       # mass on more actions than a search visits: not a visit distribution


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------------
@gpu
def test_abi_refusals_and_switching_off():
    import azk
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="error -1.*leaves_per_step"):
        vl.set_gumbel_root(4, 8)
    og, slots = gr.small_case("gomoku7", 17, 4)
    eng = azk.Engine("gomoku", G, 24, size=7)
    for bad in ((0, 17, 50.0, 1.0), (65, 17, 50.0, 1.0), (4, 1, 50.0, 1.0), (4, 25, 50.0, 1.0), (4, 17, -1.0, 1.0), (4, 17, float("nan"), 1.0),
                (4, 17, float("inf"), 1.0), (4, 17, 50.0, 0.0), (4, 17, 50.0, float("nan")), (4, 17, 50.0, float("inf"))):
        with pytest.raises(azk.AzkError, match="error -1"):
            eng.set_gumbel_root(*bad)
    assert eng.gumbel_root is None
    # the combinations: either order
    reuse = azk.Engine("gomoku", 2, 24, size=7, tree_reuse=1)
    with pytest.raises(azk.AzkError, match="error -4.*tree reuse"):
        reuse.set_gumbel_root(4, 17)
    for setter, word in ((lambda e: e.set_playout_cap(0.5, 6), "playout cap"), (lambda e: e.set_forced_playouts(2.0), "forced playouts"),
                         (lambda e: e.set_surprise_weighting(0.5), "surprise weighting")):
        a, b = azk.Engine("gomoku", 2, 24, size=7), azk.Engine("gomoku", 2, 24, size=7)
        setter(a)
        with pytest.raises(azk.AzkError, match="error -4.*" + word):
            a.set_gumbel_root(4, 17)
        b.set_gumbel_root(4, 17)
        with pytest.raises(azk.AzkError, match="error -4.*Gumbel root"):
            setter(b)
    eng.set_gumbel_root(4, 17)
    with pytest.raises(azk.AzkError, match="error -4.*Gumbel rows"):
        eng.begin_search(None)
    with pytest.raises(azk.AzkError, match="error -4.*Gumbel rows"):
        eng.begin_search_budget(None, 17)
    rows = load(eng, slots)
    with pytest.raises(azk.AzkError, match="error -4.*n_sims differs"):
        eng.begin_search_budget(rows, 24)
    with pytest.raises(azk.AzkError, match="error -4.*dirichlet = 1"):
        eng.async_begin(17, 2, 8, SEED, 0, dirichlet=False)
    with pytest.raises(azk.AzkError, match="error -4.*n_sims differs"):
        eng.async_begin(24, 2, 8, SEED, 0)
    # a zero row is the noise-free search; switched off, the engine is the reference's search again
    eng.clear_gumbel_root()
    assert eng.gumbel_root is None
    import torch
    eng.set_positions(np.stack([s["cells"] for s in slots]), [s["to_move"] for s in slots], [s["move_count"] for s in slots])
    eng.search(evaluator(49), 17, None)
    from oracle import az_oracle as ao
    s = slots[0]
    tree = ao.OracleTree(og)
    tree.reset(int(s["to_move"]), int(s["move_count"]))
    ao.mcts(og, tree, og.board_from_cells(s["cells"], s["to_move"]), 17, fr.hash_evaluator(og), None)
    assert fr.same_tree(eng.export_tree(0), tree.export())
    eng.set_gumbel_root(4, 17)
    run_search(eng, "fused", 17, torch.zeros_like(rows))
    z = gr.searched(og, gr.logits_evaluator(og), s["cells"], s["to_move"], s["move_count"], np.zeros(49), 17, 4)
    assert fr.same_tree(eng.export_tree(0), z["tree"])
    # after azk_async_begin the option is fixed
    eng.async_begin(17, 2, 8, SEED, 0)
    with pytest.raises(azk.AzkError, match="error -4.*azk_async_begin"):
        eng.set_gumbel_root(4, 17)
    with pytest.raises(azk.AzkError, match="error -4"):
        eng.clear_gumbel_root()
    with pytest.raises(azk.AzkError, match="error -4.*n_sims differs"):
        eng.async_set_budget(12, 2)


def test_python_refusals_before_any_engine_exists():
    """CPU: check_gumbel_root and the runners' constructors refuse with a ValueError that names the reason."""
    import train as az_train
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, check_gumbel_root, self_play_batch
    assert check_gumbel_root(None) is None and check_gumbel_root((16, 50, 1), 64) == (16, 50.0, 1.0)
    for bad, word in (((0, 50, 1), "m must"), ((65, 50, 1), "m must"), ((4, -1, 1), "c_visit"), ((4, float("nan"), 1), "c_visit"), ((4, 50, 0), "c_scale"),
                      ((4, 50, float("inf")), "c_scale"), ((4, 50), "must be"), ("x", "must be")):
        with pytest.raises(ValueError, match=word):
            check_gumbel_root(bad, 17)
    with pytest.raises(ValueError, match="n_sims"):
        check_gumbel_root(GUM, 1)
    with pytest.raises(ValueError, match="n_sims"):
        check_gumbel_root(GUM, (17, 24))
    with pytest.raises(ValueError, match="vanilla"):
        self_play_batch("gomoku", None, 2, 17, size=7, gumbel_root=GUM)
    with pytest.raises(ValueError, match="dirichlet"):
        self_play_batch("gomoku", lambda x: None, 2, 17, size=7, dirichlet=False, gumbel_root=GUM)
    for kw, word in ((dict(leaves_per_step=2, use_graph=True), "leaves_per_step"), (dict(tree_reuse=1), "tree reuse"), (dict(playout_cap=(0.5, 6)), "playout_cap"),
                     (dict(forced_playouts=2.0), "forced_playouts"), (dict(surprise_weight=0.5), "surprise_weight")):
        with pytest.raises(ValueError, match=word):
            SelfPlayRunner("gomoku", lambda x: None, 2, 17, size=7, gumbel_root=GUM, **kw)
    for kw, word in ((dict(reroot=1), "tree reuse"), (dict(playout_cap=(0.5, 6)), "playout_cap"), (dict(forced_playouts=2.0), "forced_playouts"),
                     (dict(surprise_weight=0.5), "surprise_weight"), (dict(dirichlet=False), "dirichlet")):
        with pytest.raises(ValueError, match=word):
            AsyncSelfPlayRunner("gomoku", lambda x: None, 2, 17, size=7, gumbel_root=GUM, **kw)
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(None, None, None, 1, 17, batched=False, gumbel_root=GUM)
