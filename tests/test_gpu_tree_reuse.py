"""GPU tests of tree reuse across moves (azk_config.tree_reuse, include/azk.h) through the C ABI (the azk ctypes binding):
 1. the re-root is exact: the tree after azk_begin_search is the played child's subtree of the tree before azk_advance;
 2. whole games equal tests/golden/tree_reuse.npz - the reference's own Node / MCTS driven with `root = chosen_child`
    (tests/golden/generate_tree_reuse.py) - in both modes, with eager, budget and captured-graph stepping;
 3. the fallbacks start from a fresh root; 4. the eval cache stays transparent; 5. off is off; 6. sharding invariance.
The reference's softmax is numpy's, the engine's is the oracle's deterministic one: the two differ in the last bits of a prior
(tests/test_gpu_engine.py compares whole trees with the oracle for that reason).  Against the golden, visits, values, pi, q and
moves are compared bit for bit; priors within 1e-6 - a float32 probability is <= 1 and its spacing <= 6e-8, and the two
softmaxes are a few roundings of exp and of the sum apart."""
import numpy as np
import pytest
import torch

from conftest import golden_meta, load_golden
from fixture_eval import fixture_logits_value
from tree_reuse_common import COLS, IDS, META, Z, action_of, digest, geometry, noise_rows, reroot, same_tree, subtree_of

pytestmark = pytest.mark.gpu
PRIOR_TOL = 1e-6


@pytest.fixture(scope="module")
def azk():
    import azk as m
    m.lib()
    return m


@pytest.fixture(scope="module")
def ao():
    from oracle import az_oracle
    return az_oracle


def dev():
    return torch.device("cuda", 0)


def evaluator(A, variant):
    return lambda x: fixture_logits_value(x, A, variant)


def t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev())


def run_steps(eng, ev, n_sims, budget):
    """Engine.search / Engine.search_budget without their begin call (the tests look at the tree between the two)."""
    logits = values = None
    if not budget:
        for _ in range(n_sims):
            eng.step(logits, values)
            n = int(eng.n_leaf.item())
            if n > 0:
                logits, values = ev(eng.leaf_boards[:n])
                logits, values = logits.float().contiguous(), values.float().reshape(-1).contiguous()
            elif eng.cache_entries:
                logits, values = eng._no_logits, eng._no_values
            else:
                logits = values = None
        if logits is not None:
            eng.step_expand_backup(logits, values)
        return
    launches = 0
    while True:
        eng.step(logits, values)
        launches += 1
        n = int(eng.n_leaf.item())
        if n > 0:
            logits, values = ev(eng.leaf_boards[:n])
            logits, values = logits.float().contiguous(), values.float().reshape(-1).contiguous()
        else:
            logits, values = (eng._no_logits, eng._no_values) if eng._no_logits is not None else (None, None)
            if eng.unfinished() == 0:
                break
        assert launches <= 2 * n_sims + 8
    if eng.cache_entries:
        eng.step_expand_backup(eng._no_logits, eng._no_values)


def start_position(eng, m, G):
    cells = Z[f"g{m['case']}_start_cells"]
    stones = int((cells != 0).sum())
    eng.set_positions(np.tile(cells, (G, 1)), [stones & 1] * G, [stones] * G)


def play_golden_case(azk, m, G=2, budget=False, trees=True, **engine_kw):
    """Play the golden case's game in G slots with its recorded inputs; returns per move what the golden records."""
    k = f"g{m['case']}_"
    A = geometry(m)[2]
    eng = azk.Engine(m["game"], G, m["n_sims"], size=m["size"] or None, tree_reuse=m["mode"], **engine_kw)
    start_position(eng, m, G)
    noise, us = noise_rows(m), Z[k + "u"]
    ev = evaluator(A, m["variant"])
    budget = budget or m["mode"] == 2
    out = []
    for mv in range(len(us)):
        nz = t64(np.tile(noise[mv], (G, 1))) if m["dirichlet"] else None
        if budget:
            eng.begin_search_budget(nz, m["n_sims"])
        else:
            eng.begin_search(nz)
        start = [eng.export_tree(g) for g in range(G)] if trees else None
        run_steps(eng, ev, m["n_sims"], budget)
        end = [eng.export_tree(g) for g in range(G)] if trees else None
        pi, q, rv = eng.root_stats()
        pi, q, rv = pi.cpu().numpy().copy(), q.cpu().numpy().copy(), rv.cpu().numpy().copy()
        chosen, winner, done = eng.advance(t64(np.full(G, us[mv])), m["sample_until"])
        out.append(dict(start=start, end=end, pi=pi, q=q, root_visit=rv, chosen=chosen.cpu().numpy().copy(),
                        winner=winner.cpu().numpy().copy(), done=done.cpu().numpy().copy()))
    eng.check_error()
    return eng, out


def assert_equals_golden(m, out, G):
    k = f"g{m['case']}_"
    for mv, r in enumerate(out):
        for g in range(G):
            where = (m["case"], mv, g)
            assert r["pi"][g].tobytes() == Z[k + "pi"][mv].tobytes(), where
            assert r["q"][g].tobytes() == Z[k + "q"][mv].tobytes(), where
            assert r["root_visit"][g] == Z[k + "root_visit"][mv], where
            assert r["chosen"][g] == Z[k + "chosen"][mv], where
            if r["start"] is not None:
                assert len(r["start"][g]["depth"]) == Z[k + "kept"][mv], where
                assert int(r["start"][g]["visit"][0]) == Z[k + "start_visit"][mv], where
                assert digest(r["start"][g], priors=False) == str(Z[k + "start_sdigest"][mv]), where
                assert digest(r["end"][g], priors=False) == str(Z[k + "end_sdigest"][mv]), where
    last = out[-1]
    if m["winner"] != -2:
        assert (last["winner"] == m["winner"]).all() and last["done"].all()
    for name in (m["full"] if out[0]["start"] is not None else ()):      # whole exports: priors too
        mv, which = int(name[1:].split("_")[0]), name.split("_")[1]
        idx = mv - int((Z[k + "start_cells"] != 0).sum())
        want = {c: Z[f"{k}{name}_{c}"] for c in COLS}
        for g in range(G):
            got = out[idx][which][g]
            for c in ("depth", "cell", "visit", "value"):
                assert np.array_equal(np.asarray(got[c]), want[c]), (name, c)
            assert np.abs(got["prior"] - want["prior"]).max() <= PRIOR_TOL, name


def assert_reroot_exact(m_like, before, chosen, after, noise_row):
    """after == the played child's subtree of before, as include/azk.h defines the re-root (bit for bit, priors included)."""
    want = reroot(before, int(chosen), lambda c: action_of(m_like, c), noise_row)
    assert len(after["depth"]) == len(want["depth"])
    assert same_tree(want, after)
    return int(want["depth"].max()), int((want["depth"] == 1).sum())


# ---------------------------------------------------------------------------------------------------
# 1. the re-root is exact
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("game,size,n_sims,dirichlet,mode", [("gomoku", 7, 64, True, 1), ("gomoku", 7, 40, False, 2), ("connect4", None, 60, True, 2),
                                                             ("connect4", None, 40, False, 1), ("tictactoe", 3, 40, True, 1),
                                                             ("gomoku", 15, 140, True, 1), ("gomoku", 15, 140, False, 2)])
def test_reroot_is_exact_on_a_batch(azk, game, size, n_sims, dirichlet, mode):
    """A batch of different games (the engine's own noise rows and uniforms per game): search, export every game, advance, begin
    the next search, export again before any step."""
    G, moves = 6, 5
    m_like = dict(game=game, size=size)
    A = geometry(m_like)[2]
    eng = azk.Engine(game, G, n_sims, size=size, tree_reuse=mode)
    eng.reset_games()
    ev = evaluator(A, "hash")
    budget = mode == 2
    before = chosen = None
    reused = 0
    for mv in range(moves):
        noise, uni = eng.gen_noise(3, 0, mv, 0.3, want_noise=dirichlet)
        if budget:
            eng.begin_search_budget(noise, n_sims)
        else:
            eng.begin_search(noise)
        after = [eng.export_tree(g) for g in range(G)]
        if before is not None:
            nz = noise.cpu().numpy() if dirichlet else None
            for g in range(G):
                if done[g]:
                    continue
                expanded = subtree_of(before[g], int(chosen[g]))
                if len(expanded["depth"]) == 1:                   # never expanded: a fresh root
                    assert len(after[g]["depth"]) == 1 and after[g]["visit"][0] == 0
                    continue
                assert_reroot_exact(m_like, before[g], chosen[g], after[g], nz[g] if dirichlet else None)
                reused += 1
        run_steps(eng, ev, n_sims, budget)
        before = [eng.export_tree(g) for g in range(G)]
        c, _, d = eng.advance(uni, 1 << 30)
        chosen, done = c.cpu().numpy().copy(), d.cpu().numpy().copy()
    eng.check_error()
    assert reused >= G * (moves - 1) - 4
    assert eng.counters()["roots_reused"] == reused


@pytest.mark.parametrize("case,want_depth,want_width", [(4, 9, 0), (7, 0, 129)])
def test_reroot_is_exact_deep_and_wide(azk, case, want_depth, want_width):
    """The golden 15x15 carry games: a carried subtree deeper than 8, and a root with more than 128 children (scattered stones)."""
    m = META[case]
    assert m["game"] == "gomoku" and m["size"] == 15 and m["mode"] == 1
    G = 2
    eng, out = play_golden_case(azk, m, G)
    noise = noise_rows(m)
    k = f"g{m['case']}_"
    deepest = widest = 0
    for mv in range(1, len(out)):
        for g in range(G):
            d, w = assert_reroot_exact(m, out[mv - 1]["end"][g], Z[k + "chosen"][mv - 1], out[mv]["start"][g], noise[mv])
            deepest, widest = max(deepest, d), max(widest, w)
    assert deepest >= want_depth and widest >= want_width
    assert_equals_golden(m, out, G)


# ---------------------------------------------------------------------------------------------------
# 2. whole games equal the reference-driven golden
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", META, ids=IDS)
def test_whole_games_equal_the_golden(azk, m):
    G = 2
    eng, out = play_golden_case(azk, m, G)
    assert_equals_golden(m, out, G)
    c = eng.counters()
    assert c["roots_reused"] == G * m["reused"]                  # every re-root the reference-driven game made, none refused
    assert c["nodes_carried"] == G * int(Z[f"g{m['case']}_kept"][Z[f"g{m['case']}_reused"] == 1].sum())


@pytest.mark.parametrize("m", [x for x in META if x["mode"] == 1], ids=[i for i, x in zip(IDS, META) if x["mode"] == 1])
def test_carry_with_budget_stepping_equals_the_golden(azk, m):
    G = 2
    eng, out = play_golden_case(azk, m, G, budget=True, trees=False)
    assert_equals_golden(m, out, G)


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("game,size,n_sims", [("gomoku", 7, 48), ("connect4", None, 40)])
def test_runners_play_the_same_games(azk, game, size, n_sims, mode):
    """self_play_batch, the eager SelfPlayRunner and the captured-graph runner (one-simulation and budget stepping) on the engine's
    own random keys: the same records move for move."""
    from selfplay import SelfPlayRunner, self_play_batch
    G, moves = 8, 7
    A = geometry(dict(game=game, size=size))[2]
    ev = evaluator(A, "hash")
    res = self_play_batch(game, ev, G, n_sims, size=size, seed=5, max_moves=moves, tree_reuse=mode)

    def run(**kw):
        rec = []
        r = SelfPlayRunner(game, ev, G, n_sims, size=size, seed=5, recycle=False, tree_reuse=mode,
                           on_records=lambda mv, base, pi, q, ch, w, d: rec.append((pi.numpy().copy(), q.numpy().copy(), ch.numpy().copy())), **kw)
        for _ in range(moves):
            r.play_move()
        r.check_error()
        return rec, r.counters()
    eager, c0 = run()
    graph, c1 = run(use_graph=True, steps_per_graph=4)
    budget, c2 = run(use_graph=True, budget_stepping=True)
    assert c0["roots_reused"] > G and c0["roots_reused"] == c1["roots_reused"] == c2["roots_reused"]
    for mv in range(moves):
        for other in (graph, budget):
            for a, b in zip(eager[mv], other[mv]):
                assert a.tobytes() == b.tobytes(), mv
        for g in range(G):
            if mv < len(res[g].cells):
                assert res[g].cells[mv] == eager[mv][2][g] and res[g].pis[mv].tobytes() == eager[mv][0][g].tobytes()


# ---------------------------------------------------------------------------------------------------
# 3. fallbacks: a fresh root, today's search bit for bit
# ---------------------------------------------------------------------------------------------------
def oracle_search(ao, game, size, cells, n_sims, variant, noise):
    og = ao.OracleGame(game, size)
    stones = int((np.asarray(cells) != 0).sum())
    board = og.board_from_cells(cells, stones & 1)
    tree = ao.OracleTree(og, cap=1 + n_sims * og.rows * og.cols)
    tree.reset(stones & 1, stones)

    def ev(canon):
        logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], og.action_dim, variant)
        return ao.softmax_det(logits[0].numpy()), float(v[0])
    ao.mcts(og, tree, board, n_sims, ev, noise)
    return tree.export()


def fresh_search_check(azk, ao, eng, game, size, n_sims, budget, mv):
    """One more search on the engine's current positions: every game must hold the oracle's fresh-root tree."""
    A = eng.action_dim
    noise, _ = eng.gen_noise(9, 0, mv, 0.3)
    cells, _, _ = eng.get_positions()
    if budget:
        eng.begin_search_budget(noise, n_sims)
    else:
        eng.begin_search(noise)
    for g in range(eng.G):
        e = eng.export_tree(g)
        assert len(e["depth"]) == 1 and e["visit"][0] == 0 and e["cell"][0] == -1
    run_steps(eng, evaluator(A, "hash"), n_sims, budget)
    nz = noise.cpu().numpy()
    for g in range(eng.G):
        assert digest(eng.export_tree(g)) == digest(oracle_search(ao, game, size, cells[g], n_sims, "hash", nz[g])), g


@pytest.mark.parametrize("mode", [1, 2])
def test_fallback_single_simulation(azk, ao, mode):
    """n_sims = 1: the only simulation expands the root, so no child is ever expanded - or even visited: azk_advance has no visit
    counts to choose from and reports the state error it always did (the reference divides by zero there).  Search after search
    starts from a fresh root; then the same on 2-simulation searches whose second simulation is never run."""
    G = 3
    eng = azk.Engine("gomoku", G, 1, size=7, tree_reuse=mode)
    eng.reset_games()
    for mv in range(3):
        fresh_search_check(azk, ao, eng, "gomoku", 7, 1, mode == 2, mv)
    eng.check_error()
    assert eng.counters()["roots_reused"] == 0
    _, uni = eng.gen_noise(9, 0, 0, 0.3, want_noise=False)
    eng.advance(uni, 1 << 30)
    with pytest.raises(azk.AzkError):
        eng.check_error()
    fresh_search_check(azk, ao, eng, "gomoku", 7, 1, mode == 2, 3)
    assert eng.counters()["roots_reused"] == 0


@pytest.mark.parametrize("how,mode", [(h, m) for h in ("set_positions", "reset", "recycle") for m in (1, 2)] + [("small_arena", 1)])
def test_fallback_after_state_changes_and_arena_rule(azk, ao, mode, how):
    """small_arena: Connect4 with arena_nodes = 226 and 32 simulations.  Early in a game every node has 7 children, so a fresh
    search needs at most 1 + 32 * 7 = 225 nodes and fits, while a carried subtree holds at least the new root and its 7 children:
    kept + 32 * 7 >= 232 > 226, the rule refuses every carry re-root.  (Top-up cannot be refused by an arena that holds a fresh
    search of the same budget - kept + n_new * 7 = 1 + 7 * 32 - which is the sizing argument of include/azk.h; see the next test.)"""
    G, n_sims = 4, 32
    budget = mode == 2
    kw = dict(arena_nodes=226) if how == "small_arena" else {}
    game, size = {"recycle": ("tictactoe", 3), "small_arena": ("connect4", None)}.get(how, ("gomoku", 7))
    eng = azk.Engine(game, G, n_sims, size=size, tree_reuse=mode, **kw)
    eng.reset_games()
    stats = torch.zeros(8, dtype=torch.int64, device=dev())
    expect_reused = 0
    for mv in range(4 if how != "recycle" else 12):
        if how == "recycle":
            # games that ended are recycled and must start fresh; the others are re-rooted: checked through the counter and
            # through the fresh-root trees of the recycled slots
            noise, uni = eng.gen_noise(9, 0, mv, 0.3)
            before_done = eng.done.cpu().numpy().copy() if mv else np.zeros(G, np.int32)
            if budget:
                eng.begin_search_budget(noise, n_sims)
            else:
                eng.begin_search(noise)
            sizes = [len(eng.export_tree(g)["depth"]) for g in range(G)]
            for g in range(G):
                if mv == 0 or before_done[g]:
                    assert sizes[g] == 1
                else:
                    assert sizes[g] > 1
                    expect_reused += 1
            run_steps(eng, evaluator(eng.action_dim, "hash"), n_sims, budget)
            eng.advance(uni, 1 << 30)
            eng.recycle_finished(stats)
            continue
        fresh_search_check(azk, ao, eng, game, size, n_sims, budget, mv)
        _, uni = eng.gen_noise(9, 0, mv, 0.3, want_noise=False)
        eng.advance(uni, 1 << 30)
        cells, tm, mc = eng.get_positions()
        if how == "set_positions":
            eng.set_positions(cells, tm, mc)
        elif how == "reset":
            eng.reset_games()
    eng.check_error()
    assert eng.counters()["roots_reused"] == expect_reused
    if how == "recycle":
        assert int(stats[0].item()) > 0 and expect_reused > 0


def test_top_up_fits_the_arena_of_a_fresh_search(azk):
    """Connect4, arena_nodes = 226 = what a fresh 32-simulation search can need: top-up re-roots every move and never overflows."""
    G, n_sims = 4, 32
    eng = azk.Engine("connect4", G, n_sims, tree_reuse=2, arena_nodes=226)
    eng.reset_games()
    for mv in range(6):
        noise, uni = eng.gen_noise(9, 0, mv, 0.3)
        eng.begin_search_budget(noise, n_sims)
        run_steps(eng, evaluator(7, "hash"), n_sims, True)
        _, _, rv = eng.root_stats()
        assert (rv.cpu().numpy() == n_sims).all()
        eng.advance(uni, 1 << 30)
    eng.check_error()
    assert eng.counters()["roots_reused"] == G * 5


# ---------------------------------------------------------------------------------------------------
# 4. the eval cache is transparent
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cache", ["per_game", "shared"])
@pytest.mark.parametrize("case", [0, 1, 10, 12])
def test_eval_cache_is_transparent(azk, case, cache):
    m = META[case]
    G = 2
    for budget in (False, True):
        eng, out = play_golden_case(azk, m, G, budget=budget, cache_entries=256, cache_shared=cache == "shared")
        assert_equals_golden(m, out, G)
        assert eng.counters()["cache_hits"] > 0


# ---------------------------------------------------------------------------------------------------
# 5. off is off; refused combinations
# ---------------------------------------------------------------------------------------------------
def test_off_reproduces_the_golden_games(azk):
    """tree_reuse = 0 passed explicitly: tests/golden/games.npz as today (pi, moves, winner; the loader of test_gpu_engine.py)."""
    from selfplay import self_play_batch
    gz = load_golden("games.npz")
    for m in [x for x in golden_meta(gz) if x["variant"]]:
        k = f"g{m['game']}_"
        noise, uniforms = gz[k + "noise"], gz[k + "uniforms"]
        G = 2
        A = geometry(dict(game=m["name"], size=m["size"]))[2]
        res = self_play_batch(m["name"], evaluator(A, m["variant"]), G, m["n_sims"], size=m["size"] or None, tree_reuse=0,
                              noise_fn=lambda mv: np.tile(noise[min(mv, len(noise) - 1)], (G, 1)),
                              uniform_fn=lambda mv: np.full(G, uniforms[mv] if mv < len(uniforms) else 0.5))
        for r in res:
            assert r.winner == m["winner"] and len(r.boards) == m["n_moves"]
            assert np.stack(r.pis).tobytes() == gz[k + "pis"].tobytes()
            assert r.cells[:len(gz[k + "actions"])] == gz[k + "actions"].tolist()


def test_off_engine_never_reuses_and_refused_combinations(azk):
    import ctypes as C
    eng = azk.Engine("gomoku", 2, 16, size=7)
    eng.reset_games()
    ev = evaluator(49, "hash")
    for mv in range(2):
        eng.begin_search(None)
        assert all(len(eng.export_tree(g)["depth"]) == 1 for g in range(2))
        run_steps(eng, ev, 16, False)
        eng.advance(None, 0)
    c = eng.counters()
    assert c["roots_reused"] == 0 and c["nodes_carried"] == 0
    L = azk.lib()

    def create(**kw):
        cfg = azk.Config()
        cfg.game, cfg.rows, cfg.cols, cfg.n_games, cfg.max_sims = azk.GAME_ID["gomoku"], 7, 7, 2, 8
        for k, v in kw.items():
            setattr(cfg, k, v)
        h = C.c_void_p()
        rc = L.azk_create(C.byref(cfg), C.byref(h))
        if rc == 0:
            L.azk_destroy(h)
        return rc
    assert create() == 0 and create(tree_reuse=1) == 0 and create(tree_reuse=2) == 0
    assert create(tree_reuse=3) == -1 and create(tree_reuse=-1) == -1                     # AZK_ERR_ARG
    assert create(tree_reuse=1, leaves_per_step=2) == -1 and create(tree_reuse=2, leaves_per_step=4) == -1
    with pytest.raises(azk.AzkError):
        azk.Engine("gomoku", 2, 8, size=7, tree_reuse=1, leaves_per_step=2)
    top = azk.Engine("gomoku", 2, 8, size=7, tree_reuse=2)
    assert L.azk_begin_search(top.h, None, None) == -4                                    # AZK_ERR_STATE: top-up needs the budget
    for mode in (1, 2):
        e = azk.Engine("gomoku", 2, 8, size=7, tree_reuse=mode)
        with pytest.raises(azk.AzkError, match="-4"):
            e.async_begin(8, 2, 8, 0, 0)
    from selfplay import AsyncSelfPlayRunner
    with pytest.raises(ValueError):
        AsyncSelfPlayRunner("gomoku", ev, 2, 8, size=7, tree_reuse=1)


# ---------------------------------------------------------------------------------------------------
# 6. sharding invariance
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2])
def test_two_half_engines_play_the_games_of_one(azk, mode):
    from selfplay import self_play_batch
    G, n_sims = 8, 40
    ev = evaluator(49, "hash")
    whole = self_play_batch("gomoku", ev, G, n_sims, size=7, seed=11, first_global_game=100, tree_reuse=mode)
    halves = [self_play_batch("gomoku", ev, G // 2, n_sims, size=7, seed=11, first_global_game=100 + i * (G // 2), tree_reuse=mode) for i in range(2)]
    parts = halves[0] + halves[1]
    for g in range(G):
        assert whole[g].cells == parts[g].cells and whole[g].winner == parts[g].winner
        assert np.stack(whole[g].pis).tobytes() == np.stack(parts[g].pis).tobytes()
        assert np.array(whole[g].qs).tobytes() == np.array(parts[g].qs).tobytes()
