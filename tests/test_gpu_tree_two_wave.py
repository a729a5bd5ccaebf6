"""k_tree with two waves per game (plain lock-step stepping): wave 0 backs the previous leaf up and walks, wave 1 builds that leaf's
move list and its children beside it, and one barrier hands the new children over.  Everything here is bit for bit against the C
oracle: the first simulations of a search one by one (the root hand-off, then previous leaves one or two levels down, where the
walk arrives while the expansion is still running), every board family, engines with idle slots, the move-list contract between
the plain and the budget kernels, and boards with fewer than four actions."""
import hashlib
import struct

import numpy as np
import pytest
import torch

from fixture_eval import fixture_logits_value

pytestmark = pytest.mark.gpu

AZK_ERR_STATE = -4


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


def digest(e):
    h = hashlib.sha256()
    for d, c, n, w, p in zip(e["depth"], e["cell"], e["visit"], e["value"], e["prior"]):
        h.update(struct.pack("<iiqdd", int(d), int(c), int(n), float(w), float(p)))
    return h.hexdigest(), len(e["depth"])


def position(ao, name, size, cells_played):
    """(game, board planes, cell codes, side to move, move count) after playing `cells_played` from the empty board."""
    game = ao.OracleGame(name, size)
    b = game.new_board()
    player = 0
    for c in cells_played:
        player = game.make_move(b, player, game.rc(int(c)))
    return game, b, (b[0] + 2 * b[1]).astype(np.int8).reshape(-1), player, len(cells_played)


_oracle_memo = {}


def oracle_digest(ao, name, size, played, n_sims, noise):
    """The oracle's tree after n_sims simulations (computed once per case and shared)."""
    key = (name, size, tuple(played), n_sims, None if noise is None else noise.tobytes())
    if key not in _oracle_memo:
        game, b, _, player, mc = position(ao, name, size, played)
        tree = ao.OracleTree(game, cap=1 + n_sims * game.rows * game.cols)
        tree.reset(player, mc)

        def ev(canon):
            logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], game.action_dim, "hash")
            return ao.softmax_det(logits[0].numpy()), float(v[0])
        ao.mcts(game, tree, b.copy(), n_sims, ev, noise)
        _oracle_memo[key] = digest(tree.export())
    return _oracle_memo[key]


def dirichlet(A, seed):
    return np.random.RandomState(seed).dirichlet([0.3] * A)


# a few stones around the centre: the first leaves have 15-30 legal moves and the walk is one or two levels deep
G7 = [24, 17, 25, 31, 18]
G15 = [112, 113, 97, 127, 98, 128]


@pytest.mark.parametrize("with_noise", [False, True], ids=["plain", "dirichlet"])
@pytest.mark.parametrize("size,played", [(7, G7), (15, G15)], ids=["gomoku7", "gomoku15"])
def test_stepwise_trees(azk, ao, size, played, with_noise):
    """export_tree after exactly 1, 2, 3, 5 and 8 simulations: simulation 1 expands nothing, 2 hands the root's children over at once,
    the next ones walk straight into the node the other wave is still expanding."""
    G, A = 3, size * size
    _, _, cells, player, mc = position(ao, "gomoku", size, played)
    nz = dirichlet(A, 5) if with_noise else None
    noise = torch.from_numpy(np.tile(nz, (G, 1))).to(dev()) if with_noise else None
    eng = azk.Engine("gomoku", G, 8, size=size)
    eng.set_positions(np.tile(cells, (G, 1)), [player] * G, [mc] * G)
    for n in (1, 2, 3, 5, 8):
        eng.search(evaluator(A), n, noise)
        eng.check_error()
        want = oracle_digest(ao, "gomoku", size, played, n, nz)
        for g in range(G):
            assert digest(eng.export_tree(g)) == want, (n, g)
    eng.close()


def test_stepwise_trees_from_the_shared_cache(azk, ao):
    """The same position searched twice with the shared eval cache: the second time the expansions read hit_logits."""
    G, size, A = 3, 7, 49
    _, _, cells, player, mc = position(ao, "gomoku", size, G7)
    eng = azk.Engine("gomoku", G, 8, size=size, cache_entries=1024, cache_shared=True)
    eng.set_positions(np.tile(cells, (G, 1)), [player] * G, [mc] * G)
    eng.search(evaluator(A), 8, None)
    for n in (1, 2, 3, 5, 8):
        eng.reset_counters()
        eng.search(evaluator(A), n, None)
        eng.check_error()
        want = oracle_digest(ao, "gomoku", size, G7, n, None)
        for g in range(G):
            assert digest(eng.export_tree(g)) == want, (n, g)
        if n >= 3:
            assert eng.counters()["cache_hits"] > 0
    eng.close()


@pytest.mark.parametrize("name,size,played,n_sims", [("tictactoe", None, [4, 0], 64), ("connect4", None, [38, 37, 31], 64),
                                                      ("gomoku", 19, [180, 181, 161, 199, 162], 32)],
                         ids=["tictactoe", "connect4", "gomoku19"])
def test_other_boards(azk, ao, name, size, played, n_sims):
    """The small games' move generators and the 7-cells-per-lane instantiation (19 x 19) on the second wave."""
    G = 3 if size is None else 1
    game, _, cells, player, mc = position(ao, name, size, played)
    eng = azk.Engine(name, G, n_sims, size=size)
    eng.set_positions(np.tile(cells, (G, 1)), [player] * G, [mc] * G)
    eng.search(evaluator(game.action_dim), n_sims, None)
    eng.check_error()
    want = oracle_digest(ao, name, size, played, n_sims, None)
    for g in range(G):
        assert digest(eng.export_tree(g)) == want, g
    eng.close()


def _full_but_one(ao):
    """A 7 x 7 Gomoku board with one empty cell and no five in a row anywhere: the next move ends the game in a draw."""
    game = ao.OracleGame("gomoku", 7)
    codes = np.array([[1 + ((c // 2 + r) & 1) for c in range(7)] for r in range(7)], np.int8)
    codes[6, 5] = 0                                        # (a stone of the colour that had 25)
    b = game.board_from_cells(codes)
    for r in range(7):
        for c in range(7):
            if codes[r, c]:
                assert game.check_winner(b, int(codes[r, c]) - 1, (r, c)) == -1
    n1, n2 = int((codes == 1).sum()), int((codes == 2).sum())
    assert n1 == n2 and n1 + n2 == 48                      # player 0 to move, move 48 of 49
    return codes.reshape(-1)


def _mixed_engine_run(azk, ao):
    G, size, A, n_sims = 4, 7, 49, 24
    last = _full_but_one(ao)
    _, _, live_cells, live_player, live_mc = position(ao, "gomoku", size, G7)
    eng = azk.Engine("gomoku", G, n_sims, size=size)
    eng.set_positions(np.stack([last, live_cells, last, live_cells]), [0, live_player, 0, live_player], [48, live_mc, 48, live_mc])
    eng.search(evaluator(A), n_sims, None)
    chosen, _, done = eng.advance()
    assert done.tolist() == [1, 0, 1, 0]
    played = G7 + [int(chosen[1].item())]
    assert int(chosen[3].item()) == played[-1]
    eng.search(evaluator(A), n_sims, None)                  # slots 0 and 2 are finished games now
    eng.check_error()
    _, _, rv = eng.root_stats()
    assert rv.tolist()[1::2] == [n_sims, n_sims]
    out = [digest(eng.export_tree(g)) for g in range(G)]
    want = oracle_digest(ao, "gomoku", size, played, n_sims, None)
    assert out[1] == want and out[3] == want
    eng.close()
    return out


def test_mixed_engine_finished_and_live_slots(azk, ao):
    """Two finished games and two live ones in one engine: every wave of every workgroup meets its barrier, the search completes, the
    live trees are the oracle's, and a second run leaves the same digests in all four slots."""
    assert _mixed_engine_run(azk, ao) == _mixed_engine_run(azk, ao)


def test_budget_step_refuses_a_leaf_without_move_list(azk, ao):
    """A plain step leaves leaf_nmoves = -1 (the list is built at expansion).  The budget kernels expand from the list: meeting such a
    leaf is a caller error, AZK_ERR_STATE in the sticky error word - and the engine closes cleanly afterwards."""
    G, size, A = 2, 7, 49
    eng = azk.Engine("gomoku", G, 8, size=size)
    eng.async_begin(8, 4, 0, 1, 0, dirichlet=False, recycle=False)     # (the asynchronous mover steps with the budget kernel)
    eng.begin_search(None)
    eng.step()
    n = int(eng.n_leaf.item())
    assert n == G
    logits, values = evaluator(A)(eng.leaf_boards[:n])
    eng.async_step(logits.contiguous(), values.contiguous(), phases=1)
    assert eng.L.azk_check_device_error(eng.h, None) == AZK_ERR_STATE
    with pytest.raises(azk.AzkError):
        eng.check_error()
    eng.close()


def test_plain_expansion_accepts_a_list_left_by_the_budget_kernel(azk, ao):
    """The other direction of the contract: budget stepping ends with a plain expand-only launch over leaves whose list the budget
    kernel built (leaf_nmoves >= 0)."""
    G, size, A, n_sims = 3, 7, 49, 16
    _, _, cells, player, mc = position(ao, "gomoku", size, G7)
    eng = azk.Engine("gomoku", G, n_sims, size=size, cache_entries=256)
    eng.set_positions(np.tile(cells, (G, 1)), [player] * G, [mc] * G)
    for _ in range(2):                                      # second search: leaves served by the cache, expanded by the final plain launch
        eng.search_budget(evaluator(A), n_sims, None, per_launch=4)
        eng.check_error()
        want = oracle_digest(ao, "gomoku", size, G7, n_sims, None)
        for g in range(G):
            assert digest(eng.export_tree(g)) == want, g
    eng.close()


@pytest.mark.parametrize("rows,cols", [(1, 3), (2, 2)], ids=["1x3", "2x2"])
def test_boards_with_fewer_than_four_actions(azk, rows, cols):
    """Rows of fewer than four logits: the four-floats-per-lane accesses of the expansion and the cache probe stay inside the row."""
    n_sims, G = 6, 2
    for cache in (0, 64):
        eng = azk.Engine("gomoku", G, n_sims, size=(rows, cols), cache_entries=cache, cache_shared=bool(cache))
        eng.reset_games()
        eng.search(evaluator(rows * cols), n_sims, None)
        eng.check_error()
        _, _, rv = eng.root_stats()
        assert rv.tolist() == [n_sims] * G
        eng.close()
