"""Gomoku boards the rest of the suite never builds: rows != cols, one row or one column, fewer than four cells, 30 columns, and cell
counts on both sides of every switch in the kernels (four or seven cells per lane at 256 cells, the 512- or 2048-slot set table at
307).  On a square board an expression with rows and cols swapped gives the right answer; here it does not.

Rules are pinned to the reference through tests/golden/rules_gomoku_rect.npz (its statics with rows / cols overridden).  Trees and
games are pinned to the C oracle only: the reference's own get_action_idx is r * rows + c (gomoku.py:48), which is no cell index
when rows != cols, so its searches on such boards cannot be recorded.  Every comparison is exact."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from fixture_eval import fixture_logits_value
from test_gpu_engine import boards_from_cells, digest, gpu_evaluator

pytestmark = pytest.mark.gpu

_RECT = load_golden("rules_gomoku_rect.npz")
GEOMETRIES = [(int(r), int(c)) for r, c in _RECT["geometries"]]
COUNTERS = ("edges_scanned", "trace_nodes", "edges_created", "terminal_sims")


def gid(g):
    return f"{g[0]}x{g[1]}"


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


def rect_fixture(rows, cols):
    p = f"g{rows}x{cols}_"
    return {k[len(p):]: _RECT[k] for k in _RECT.files if k.startswith(p)}


def cpu_evaluator(ao, A):
    def ev(canon):
        logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], A, "hash")
        return ao.softmax_det(logits[0].numpy()), float(v[0])
    return ev


def cells_of(b):
    return (b[0] + 2 * b[1]).astype(np.int8).reshape(-1)


def random_prefix(game, plies, seed):
    """(board, side to move, plies) after `plies` uniformly random legal moves none of which wins."""
    rng = np.random.RandomState(seed)
    b, player, mc = game.new_board(), 0, 0
    while mc < plies:
        vm = game.valid_cells(b)
        cell = int(vm[rng.randint(len(vm))])
        b2 = b.copy()
        nxt = game.make_move(b2, player, game.rc(cell))
        if game.check_winner(b2, player, game.rc(cell)) == -1:
            b, player, mc = b2, nxt, mc + 1
    return b, player, mc


def sims_for(rc):
    """6 to 12 simulations below five cells (the whole game tree has fewer nodes than that), 120 / 100 up to 64 / 256 cells, 60 above."""
    if rc < 5:
        return 4 + 2 * rc
    return 120 if rc <= 64 else (100 if rc <= 256 else 60)


# ---------------------------------------------------------------------------------------------------
# rules, every geometry of the fixture
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", GEOMETRIES, ids=[gid(g) for g in GEOMETRIES])
def test_rules_vs_reference_fixture(azk, ao, rows, cols):
    z = rect_fixture(rows, cols)
    size, A = (rows, cols), rows * cols
    cells = z["rb_cells"]
    boards = torch.from_numpy(boards_from_cells(cells, 2, rows, cols)).to(dev())
    moves, counts = azk.rules_legal_moves("gomoku", boards, size)
    moves, counts = moves.cpu().numpy(), counts.cpu().numpy()
    mask = azk.rules_legal_mask("gomoku", boards, A, size).cpu().numpy()
    for bi in range(len(cells)):
        want = z["rb_valid_flat"][z["rb_valid_off"][bi]:z["rb_valid_off"][bi + 1]].tolist()
        assert int(counts[bi]) == len(want), bi
        assert moves[bi, :counts[bi]].tolist() == want, bi
        wm = np.zeros(A, np.uint8)
        wm[want] = 1
        assert np.array_equal(mask[bi], wm), bi
    q = z["rb_queries"]
    qb = boards[torch.from_numpy(q[:, 0].astype(np.int64)).to(dev())].contiguous()
    players = torch.from_numpy(q[:, 1].astype(np.int32)).to(dev())
    cellq = torch.from_numpy(q[:, 2].astype(np.int32) * cols + q[:, 3].astype(np.int32)).to(dev())
    w = azk.rules_check_winner("gomoku", qb, players, cellq, size).cpu().numpy()
    assert w.tolist() == q[:, 4].astype(np.int32).tolist()

    # the fixture's first playout, all plies in one batch: legal lists and winners against the fixture, the boards after
    # make_move / undo_move and the canonical boards against the oracle's
    game = ao.OracleGame("gomoku", size)
    t0, t1 = int(z["game_off"][0]), int(z["game_off"][1])
    acts = z["actions"][t0:t1].astype(np.int32)
    before, after, canon, nxt_want = [], [], [], []
    b, player = game.new_board(), 0
    for cell in acts:
        before.append(b.copy())
        canon.append(game.get_canonical_board(b, player))
        nxt = game.make_move(b, player, game.rc(int(cell)))
        after.append(b.copy())
        nxt_want.append(nxt)
        player = nxt
    assert np.array_equal(cells_of(b), z["final_cells"][0])
    T = len(acts)
    pl = torch.from_numpy((np.arange(T) & 1).astype(np.int32)).to(dev())
    ct = torch.from_numpy(acts).to(dev())
    bt = torch.from_numpy(np.stack(before)).to(dev())
    moves, counts = azk.rules_legal_moves("gomoku", bt, size)
    moves, counts = moves.cpu().numpy(), counts.cpu().numpy()
    for t in range(T):
        want = z["valid_flat"][z["valid_off"][t0 + t]:z["valid_off"][t0 + t + 1]].tolist()
        assert moves[t, :counts[t]].tolist() == want, t
    can = azk.rules_canonical("gomoku", bt, pl, size)
    assert np.array_equal(can.cpu().numpy(), np.stack(canon))
    work = bt.clone()
    nxt = azk.rules_apply_move("gomoku", work, pl, ct, size)
    assert nxt.tolist() == nxt_want
    assert np.array_equal(work.cpu().numpy(), np.stack(after))
    w = azk.rules_check_winner("gomoku", work, pl, ct, size).cpu().numpy()
    assert w.tolist() == z["winners"][t0:t1].astype(np.int32).tolist()
    again = azk.rules_apply_move("gomoku", work, nxt, ct, size)          # occupied now: the same player, the board untouched
    assert torch.equal(again, nxt) and np.array_equal(work.cpu().numpy(), np.stack(after))
    azk.rules_undo_move("gomoku", work, nxt, ct, size)
    assert np.array_equal(work.cpu().numpy(), np.stack(before))


# ---------------------------------------------------------------------------------------------------
# search trees
# ---------------------------------------------------------------------------------------------------
_memo = {}


def search_case(ao, rows, cols, plies, n_sims, G, K=1):
    """The position, one Dirichlet row per slot (K > 1: one row for all) and the oracle's trees (digest and counters per slot), computed once per case."""
    key = (rows, cols, plies, n_sims, G, K)
    if key not in _memo:
        game = ao.OracleGame("gomoku", (rows, cols))
        A = rows * cols
        b, player, mc = random_prefix(game, plies, 31 * rows + cols)
        noise = np.random.RandomState(1000 * rows + cols).dirichlet([0.3] * A, size=G)
        if K > 1:
            noise[1:] = noise[0]                 # (the same game in every slot: the engine's launch count is that game's)
        want, cnts, launches = [], [], []
        for g in range(G):
            tree = ao.OracleTree(game, cap=1 + n_sims * A)
            tree.reset(player, mc)
            cnt = ao.Counters()
            if K == 1:
                ao.mcts(game, tree, b.copy(), n_sims, cpu_evaluator(ao, A), noise[g], ao.OracleCache(game), None, cnt)
            else:
                launches.append(ao.mcts_vl(game, tree, b.copy(), n_sims, K, cpu_evaluator(ao, A), noise[g], None, cnt))
            want.append(digest(tree.export()))
            cnts.append(cnt.as_dict())
        _memo[key] = dict(cells=cells_of(b), player=player, mc=mc, noise=noise, want=want, cnts=cnts, launches=launches)
    return _memo[key]


def check_trees(eng, case, G, n_sims, cached):
    eng.check_error()
    for g in range(G):
        assert digest(eng.export_tree(g)) == case["want"][g], g
    c = eng.counters()
    assert c["sims"] == G * n_sims
    for name in COUNTERS:
        assert c[name] == sum(cn[name] for cn in case["cnts"]), name
    expansions = sum(cn["expansions"] for cn in case["cnts"])
    if cached:
        assert c["leaves_evaluated"] + c["cache_hits"] == expansions
    else:
        assert c["leaves_evaluated"] == expansions and c["cache_hits"] == 0
    return c


def prefix_plies(rc):
    return max(rc // 4, 1)


TWO_WAVE = [(1, 1), (1, 3), (3, 1), (2, 2), (5, 5), (4, 6), (6, 4), (1, 30), (30, 1), (16, 16), (8, 30), (17, 18), (11, 28), (13, 30), (30, 13)]
# (a one-cell board has no position but the empty one to search from)
TWO_WAVE_CASES = [(r, c, 0) for r, c in TWO_WAVE] + [(r, c, prefix_plies(r * c)) for r, c in TWO_WAVE if r * c > 1]


@pytest.mark.parametrize("rows,cols,plies", TWO_WAVE_CASES, ids=[f"{r}x{c}-p{p}" for r, c, p in TWO_WAVE_CASES])
def test_two_wave_trees_vs_oracle(azk, ao, rows, cols, plies):
    """Plain stepping (the two-wave k_tree): hashed logits, a Dirichlet row of its own per slot, whole trees and counters."""
    G, A = 2, rows * cols
    n_sims = sims_for(A)
    case = search_case(ao, rows, cols, plies, n_sims, G)
    eng = azk.Engine("gomoku", G, n_sims, size=(rows, cols))
    assert (eng.rows, eng.cols, eng.action_dim, eng.state_dim) == (rows, cols, A, A)
    eng.set_positions(np.tile(case["cells"], (G, 1)), [case["player"]] * G, [case["mc"]] * G)
    eng.search(gpu_evaluator(A, "hash"), n_sims, torch.from_numpy(case["noise"]).to(dev()))
    check_trees(eng, case, G, n_sims, cached=False)
    cells_after, tm, mc = eng.get_positions()
    assert np.array_equal(cells_after[1], case["cells"]) and tm[1] == case["player"] and mc[1] == case["mc"]
    eng.close()


ONE_WAVE = [(1, 1), (1, 2), (1, 3), (3, 1), (2, 2), (5, 5), (4, 6), (8, 30), (13, 30)]


@pytest.mark.parametrize("cache", ["off", "per-game", "shared"])
@pytest.mark.parametrize("rows,cols", ONE_WAVE, ids=[gid(g) for g in ONE_WAVE])
def test_one_wave_trees_vs_oracle(azk, ao, rows, cols, cache):
    """Budget stepping (the one-wave k_tree, which expands, writes and reads eval-cache rows itself), twice in a row on one engine.
    The second search repeats the first's leaves: a leaf whose table slot no other leaf of the search shares is served from the
    table, so with at most 60 leaves per game in 64 slots some are."""
    G, A = 2, rows * cols
    n_sims = sims_for(A)
    plies = 0 if A < 25 else A // 4
    case = search_case(ao, rows, cols, plies, n_sims, G)
    eng = azk.Engine("gomoku", G, n_sims, size=(rows, cols), cache_entries=0 if cache == "off" else 64, cache_shared=cache == "shared")
    eng.set_positions(np.tile(case["cells"], (G, 1)), [case["player"]] * G, [case["mc"]] * G)
    noise = torch.from_numpy(case["noise"]).to(dev())
    for rep in range(2):
        eng.reset_counters()
        launches = eng.search_budget(gpu_evaluator(A, "hash"), n_sims, noise, per_launch=4)
        c = check_trees(eng, case, G, n_sims, cached=cache != "off")
        assert launches <= n_sims + 2
        if rep == 1 and cache != "off":
            assert c["cache_hits"] > 0
    eng.close()


@pytest.mark.parametrize("rows,cols", [(1, 3), (6, 9)], ids=["1x3", "6x9"])
def test_virtual_loss_trees_vs_oracle(azk, ao, rows, cols):
    """Two leaves in flight per game (the one-wave k_tree's K-slot schedule) against its sequential statement in the oracle."""
    G, A, K = 2, rows * cols, 2
    n_sims = 10 if A < 5 else 80
    plies = 0 if A < 25 else A // 4
    case = search_case(ao, rows, cols, plies, n_sims, G, K)
    noise = torch.from_numpy(case["noise"]).to(dev())
    for entries in (0, 64):
        eng = azk.Engine("gomoku", G, n_sims, size=(rows, cols), leaves_per_step=K, cache_entries=entries)
        eng.set_positions(np.tile(case["cells"], (G, 1)), [case["player"]] * G, [case["mc"]] * G)
        launches = eng.search_budget(gpu_evaluator(A, "hash"), n_sims, noise)
        eng.check_error()
        for g in range(G):
            assert digest(eng.export_tree(g)) == case["want"][g], (entries, g)
        assert eng.counters()["sims"] == G * n_sims
        if entries == 0:
            assert launches == case["launches"][0]
        eng.close()


# ---------------------------------------------------------------------------------------------------
# whole games
# ---------------------------------------------------------------------------------------------------
def oracle_games(ao, rows, cols, G, n_sims, seed):
    """G oracle games with injected Dirichlet rows and sampling uniforms (computed once and shared by the stepping modes)."""
    key = ("games", rows, cols, G, n_sims, seed)
    if key not in _memo:
        game = ao.OracleGame("gomoku", (rows, cols))
        A = rows * cols
        rng = np.random.RandomState(seed)
        noise = rng.dirichlet([0.3] * A, size=(A, G))            # [ply, game, action]: a game has at most A plies
        uniforms = rng.random_sample((A, G))
        outs = [ao.self_play(game, cpu_evaluator(ao, A), n_sims, noise_fn=lambda mv, g=g: noise[mv, g],
                             uniform_fn=lambda mv, g=g: uniforms[mv, g]) for g in range(G)]
        _memo[key] = (noise, uniforms, outs)
    return _memo[key]


def play_and_compare(ao, rows, cols, G, n_sims, seed, budget):
    from selfplay import self_play_batch
    noise, uniforms, outs = oracle_games(ao, rows, cols, G, n_sims, seed)
    res = self_play_batch("gomoku", gpu_evaluator(rows * cols, "hash"), G, n_sims, size=(rows, cols), noise_fn=lambda mv: noise[mv],
                          uniform_fn=lambda mv: uniforms[mv], budget_stepping=budget, cache_entries=64 if budget else 0)
    for g in range(G):
        r, out = res[g], outs[g]
        assert r.cells == out["cells"].tolist(), g
        assert r.winner == out["winner"], g
        assert np.stack(r.pis).tobytes() == out["pis"].tobytes(), g
        assert np.array(r.qs).tobytes() == out["qs"].tobytes(), g
        assert all(np.array_equal(a, b) for a, b in zip(r.boards, out["boards"])), g
    return outs


@pytest.mark.parametrize("budget", [False, True], ids=["plain", "budget"])
@pytest.mark.parametrize("rows,cols", [(1, 1), (1, 2), (2, 2), (3, 1)], ids=["1x1", "1x2", "2x2", "3x1"])
def test_games_that_can_only_be_drawn(ao, azk, rows, cols, budget):
    """Fewer than five cells: every game fills the board and is a draw at ply rows * cols; the last searches start one move from
    the full board."""
    outs = play_and_compare(ao, rows, cols, 4, 8, 11, budget)
    for out in outs:
        assert out["winner"] == -1 and len(out["cells"]) == rows * cols
        assert sorted(out["cells"].tolist()) == list(range(rows * cols))


# (seeds picked on the oracle alone so that its sixteen games end at more than one length)
@pytest.mark.parametrize("budget", [False, True], ids=["plain", "budget"])
@pytest.mark.parametrize("rows,cols,seed", [(5, 6, 1), (4, 9, 1)], ids=["5x6", "4x9"])
def test_ragged_batches_of_games(ao, azk, rows, cols, seed, budget):
    """Sixteen games with noise and uniforms of their own on boards where five in a row fits along some directions only (5 x 6: not
    on every diagonal; 4 x 9: horizontally only); they end at different plies, and each equals the oracle's game."""
    outs = play_and_compare(ao, rows, cols, 16, 32, seed, budget)
    assert len({len(out["cells"]) for out in outs}) >= 2
