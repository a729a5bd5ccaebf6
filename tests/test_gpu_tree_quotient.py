"""The quotient column of the tree arena: beside every node's W the engine keeps Q = W / (double)N, written by the one
helper through which a backup, a virtual loss and its undo change a visited node (node_store_wq, csrc/azk_engine_int.h); the walk of
k_tree reads Q where it used to divide W by N for every scanned child on every level.

 1. the invariant: after a search, the bits of Q equal the bits of np.float64(W) / np.float64(N) for every node with N > 0 - under plain
    stepping, budget stepping and the asynchronous movers with two simulations per launch, virtual loss (K = 2) once every loss is undone,
    and tree reuse in both modes on the move after a re-root (the copy), each with root noise (float64 scan at the root) and without;
 2. trees, bit for bit against the C oracle, and the move played, on every form of the child scan;
 3. a node with N = 0 has no quotient, and nothing reads the word: a search over a column pre-filled with zeros and one over a column
    pre-filled with NaNs leave identical trees - also under forced playouts and a Gumbel root, whose scans see q as well.

The child counts of 2, checked with the oracle alone on the CPU (64 simulations, fixture evaluator; "scanned" = the child count of a node
that was visited again after its expansion, i.e. whose children a walk has scored):
    gomoku 6 x 6, 10 x 10 and 12 x 12 from the EMPTY board: the root has ONE child (an empty Gomoku board's only legal move is its centre;
        a position's legal moves are the empty cells next to a stone) and the scanned nodes have 1 .. 21, 1 .. 22 and 1 .. 20 children:
        one child per lane, on every level.  An empty board cannot reach the wider forms, and a 12 x 12 board cannot at all: more than
        128 children need more than 128 empty cells next to a stone, each stone has at most 8 neighbours, and 144 - s > 128 with
        8 s >= 144 - s has no solution;
    gomoku 10 x 10 with nine stones on the lattice {1, 4, 7}^2: root 72 children, scanned nodes 69 .. 74: two children per lane, at the
        root and below it;
    gomoku 14 x 14 with 25 stones on the lattice {1, 4, 7, 10, 12}^2: root 171 children, scanned nodes 167 .. 171: the general loop, at the
        root and below it;
    tic-tac-toe after two plies 2 .. 7, Connect 4 after three plies 7: one child per lane, the other two make_move kinds.
test_oracle_child_counts asserts these figures, so the cases keep exercising the form they are named for."""
import numpy as np
import pytest
import torch

from fixture_eval import fixture_logits_value
from test_gpu_tree_two_wave import G7, digest, dirichlet, position

pytestmark = pytest.mark.gpu


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


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def lattice(size, marks):
    return [r * size + c for r in marks for c in marks]


# name -> (game, size, cells played from the empty board, (fewest, most) children of a scanned node, children of the root)
N_SIMS = 64
CASES = {
    "gomoku6_empty": ("gomoku", 6, [], (1, 21), 1),
    "gomoku10_empty": ("gomoku", 10, [], (1, 22), 1),
    "gomoku12_empty": ("gomoku", 12, [], (1, 20), 1),
    "gomoku10_two_per_lane": ("gomoku", 10, lattice(10, (1, 4, 7)), (69, 74), 72),
    "gomoku14_general_loop": ("gomoku", 14, lattice(14, (1, 4, 7, 10, 12)), (167, 171), 171),
    "tictactoe": ("tictactoe", None, [4, 0], (2, 7), 7),
    "connect4": ("connect4", None, [38, 37, 31], (7, 7), 7),
}

_memo = {}


def oracle_search(ao, case, with_noise):
    """The oracle's search of a case, once: (exported tree, the first most-visited root child's cell, the noise row or None)."""
    key = (case, with_noise)
    if key not in _memo:
        name, size, played, _, _ = CASES[case]
        game, b, _, player, mc = position(ao, name, size, played)
        nz = dirichlet(game.action_dim, 5) if with_noise else None
        tree = ao.OracleTree(game, cap=1 + N_SIMS * game.rows * game.cols)
        tree.reset(player, mc)

        def ev(canon):
            logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], game.action_dim, "hash")
            return ao.softmax_det(logits[0].numpy()), float(v[0])
        ao.mcts(game, tree, b.copy(), N_SIMS, ev, nz)
        ch = tree.root_children()
        _memo[key] = (tree.export(), int(ch["cell"][int(np.argmax(ch["visit"]))]), nz)     # (argmax: the first maximum, node.py:76-81)
    return _memo[key]


def child_counts(t):
    depth = np.asarray(t["depth"])
    nch, stack = np.zeros(len(depth), np.int64), []
    for i, d in enumerate(depth):
        while stack and depth[stack[-1]] >= d:
            stack.pop()
        if stack:
            nch[stack[-1]] += 1
        stack.append(i)
    return nch


@pytest.mark.parametrize("with_noise", [False, True], ids=["plain", "dirichlet"])
@pytest.mark.parametrize("case", list(CASES))
def test_oracle_child_counts(ao, case, with_noise):
    """The cases reach the child counts they are named for (no GPU code runs here; it shares the oracle's searches with the tests below)."""
    t, _, _ = oracle_search(ao, case, with_noise)
    nch, visit = child_counts(t), np.asarray(t["visit"])
    scanned = nch[(visit >= 2) & (nch > 0)]
    lo, hi = CASES[case][3]
    assert int(nch[0]) == CASES[case][4] and len(scanned) >= 10
    if case in ("tictactoe", "connect4"):
        assert lo <= scanned.min() and scanned.max() == hi
    else:
        assert (int(scanned.min()), int(scanned.max())) == (lo, hi)
    if case == "gomoku10_two_per_lane":
        assert ((scanned > 64) & (scanned <= 128)).all() and (visit[np.asarray(t["depth"]) >= 1] >= 2).any()   # ... below the root too
    if case == "gomoku14_general_loop":
        assert (scanned > 128).all() and (visit[np.asarray(t["depth"]) >= 1] >= 2).any()


def assert_quotients(t, where, at_least=2):
    """Q == W / N, bit for bit, wherever N > 0."""
    visit, value, quot = np.asarray(t["visit"]), np.asarray(t["value"], np.float64), np.asarray(t["quotient"], np.float64)
    m = visit > 0
    assert int(m.sum()) >= at_least, where
    want = value[m] / visit[m].astype(np.float64)
    assert want.tobytes() == np.ascontiguousarray(quot[m]).tobytes(), where
    return int(m.sum())


def start(azk, ao, case, G, with_noise, **kw):
    name, size, played, _, _ = CASES[case]
    game, _, cells, player, mc = position(ao, name, size, played)
    nz = dirichlet(game.action_dim, 5) if with_noise else None
    noise = torch.from_numpy(np.tile(nz, (G, 1))).to(dev()) if with_noise else None
    eng = azk.Engine(name, G, N_SIMS, size=size, **kw)
    eng.set_positions(np.tile(cells, (G, 1)), [player] * G, [mc] * G)
    return eng, evaluator(game.action_dim), noise


# ---------------------------------------------------------------------------------------------------
# 1. the invariant
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True], ids=["plain", "dirichlet"])
@pytest.mark.parametrize("stepping", ["plain", "budget2", "virtual_loss2"])
@pytest.mark.parametrize("case", ["gomoku6_empty", "gomoku10_two_per_lane"])
def test_invariant_after_a_search(azk, ao, case, stepping, with_noise):
    """plain: the two-wave kernels (wave 0's short-path backup, backup_path at terminal leaves).  budget2: the one-wave MULTI kernel, two
    simulations per launch, eval cache on so that a game does run on inside a launch.  virtual_loss2: K = 2 - every selection leaves a
    visit and a loss on its path and the backup takes the loss back; after the search none is left, and Q says so."""
    G = 3
    kw = dict(plain={}, budget2=dict(cache_entries=256), virtual_loss2=dict(leaves_per_step=2))[stepping]
    eng, ev, noise = start(azk, ao, case, G, with_noise, **kw)
    if stepping == "plain":
        eng.search(ev, N_SIMS, noise)
    else:
        eng.search_budget(ev, N_SIMS, noise, per_launch=2)
    eng.check_error()
    for g in range(G):
        t = eng.export_tree(g, quotient=True)
        assert int(t["visit"][0]) == N_SIMS
        assert_quotients(t, (case, stepping, with_noise, g), at_least=10)
        if stepping != "virtual_loss2":                               # (K = 2 is another search: pinned by tests/test_gpu_virtual_loss.py)
            assert digest(t) == digest(oracle_search(ao, case, with_noise)[0]), g
        else:
            assert (np.abs(t["value"]) <= t["visit"] + 1e-9).all()    # no virtual loss left behind
    eng.close()


@pytest.mark.parametrize("with_noise", [False, True], ids=["plain", "dirichlet"])
@pytest.mark.parametrize("mode", [1, 2], ids=["carry", "top_up"])
def test_invariant_across_a_reroot(azk, ao, mode, with_noise):
    """Tree reuse: the move after a re-root starts from the played child's subtree, slid to the front of the arena - H, W and Q together.
    Checked on the tree as the re-root leaves it (nothing but the copy has written those words) and after the search that follows."""
    from test_gpu_tree_reuse import run_steps
    G, case = 3, "gomoku6_empty"
    eng, ev, noise = start(azk, ao, case, G, with_noise, tree_reuse=mode)
    kept = 0
    for mv in range(3):
        eng.begin_search_budget(noise, N_SIMS, 2)
        for g in range(G):
            t = eng.export_tree(g, quotient=True)
            if mv > 0:
                kept += assert_quotients(t, ("start", mode, with_noise, mv, g), at_least=1)
        run_steps(eng, ev, N_SIMS, True)
        eng.check_error()
        for g in range(G):
            assert_quotients(eng.export_tree(g, quotient=True), ("end", mode, with_noise, mv, g), at_least=10)
        eng.advance()
    assert eng.counters()["roots_reused"] == 2 * G and kept > 2 * G    # the re-roots happened and carried visited nodes over
    eng.close()


@pytest.mark.parametrize("reroot", [0, 1], ids=["fresh_roots", "reroot"])
def test_invariant_under_the_asynchronous_movers(azk, reroot):
    """The asynchronous movers, two simulations per launch, root noise on: games move at their own pace (with reroot=1 the drain re-roots
    them), and at every launch boundary we look at, every tree of the engine satisfies the invariant."""
    from selfplay import AsyncSelfPlayRunner
    G, sims = 4, 48
    r = AsyncSelfPlayRunner("gomoku", evaluator(36), G, sims, size=6, seed=5, recycle=True, cache_entries=64, per_launch=2, steps_per_graph=8,
                            use_graph=False, reroot=reroot)
    visited = 0
    for _ in range(12):
        r.run_chunk()
        r.finish()
        for g in range(G):
            visited += assert_quotients(r.eng.export_tree(g, quotient=True), (reroot, g), at_least=0)
    r.check_error()
    assert int(r.finish()[5]) >= G and visited > 12 * G                # every slot's worth of moves was played, the trees were not empty
    if reroot:
        assert r.counters()["roots_reused"] > 0


# ---------------------------------------------------------------------------------------------------
# 2. trees against the oracle on every scan form
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_noise", [False, True], ids=["plain", "dirichlet"])
@pytest.mark.parametrize("case", list(CASES))
def test_trees_and_moves_equal_the_oracle(azk, ao, case, with_noise):
    """N, W, P and the children of every node (the digest of the whole export) and the move played, per scan form and prior width."""
    G = 2
    want, want_cell, _ = oracle_search(ao, case, with_noise)
    eng, ev, noise = start(azk, ao, case, G, with_noise)
    eng.search(ev, N_SIMS, noise)
    eng.check_error()
    for g in range(G):
        t = eng.export_tree(g, quotient=True)
        assert digest(t) == digest(want), (case, with_noise, g)
        assert_quotients(t, (case, with_noise, g), at_least=10)
    chosen, _, _ = eng.advance()
    assert chosen.tolist() == [want_cell] * G
    eng.close()


# ---------------------------------------------------------------------------------------------------
# 3. N = 0 is inert
# ---------------------------------------------------------------------------------------------------
def searched_with_fill(azk, ao, case, byte, option, stepping):
    G = 2
    kw = dict(cache_entries=256) if stepping == "budget2" else {}
    eng, ev, noise = start(azk, ao, case, G, True, **kw)
    if option == "forced":
        eng.set_forced_playouts(2.0)
    elif option == "gumbel":
        eng.set_gumbel_root(8, N_SIMS)
    eng.fill_quotients(byte)
    if stepping == "plain":
        eng.search(ev, N_SIMS, noise)
    else:
        eng.search_budget(ev, N_SIMS, noise, per_launch=2)
    eng.check_error()
    trees = [eng.export_tree(g, quotient=True) for g in range(G)]
    for g, t in enumerate(trees):
        assert_quotients(t, (case, byte, option, stepping, g), at_least=5)
        fresh = np.asarray(t["quotient"])[np.asarray(t["visit"]) == 0]
        assert len(fresh) > 0                                          # unvisited children exist and kept what was filled in: nobody writes them
        assert np.isnan(fresh).all() if byte == 255 else (fresh == 0.0).all()
    chosen = eng.advance()[0].tolist()
    eng.close()
    return [digest(t) for t in trees], chosen


@pytest.mark.parametrize("stepping", ["plain", "budget2"])
@pytest.mark.parametrize("option", ["none", "forced", "gumbel"])
@pytest.mark.parametrize("case", ["gomoku6_empty", "gomoku10_two_per_lane", "gomoku14_general_loop"])
def test_unvisited_quotients_reach_no_result(azk, ao, case, option, stepping):
    """The same search over a quotient column of zeros and over one of NaNs (root noise on: the float64 scan at the root, the float32 scan
    below it): identical trees, identical moves - without options also the oracle's tree.  Were an N = 0 quotient to reach a score, the
    NaN run would lose every comparison it took part in and the zero run would not."""
    zeros = searched_with_fill(azk, ao, case, 0, option, stepping)
    nans = searched_with_fill(azk, ao, case, 255, option, stepping)
    assert zeros == nans
    if option == "none":
        assert zeros[0] == [digest(oracle_search(ao, case, True)[0])] * 2
