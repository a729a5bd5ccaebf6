"""tests/golden/tree_reuse.npz (the reference's Node / MCTS driven with `root = chosen_child`, see generate_tree_reuse.py) is
self-consistent, and its first moves - always a fresh root - are the searches the pinned oracle runs.  CPU only."""
import numpy as np
import pytest
import torch

from fixture_eval import fixture_logits_value, numpy_softmax_like_reference
from oracle import az_oracle as ao
from tree_reuse_common import COLS, IDS, META, Z, action_of, digest, geometry, noise_rows, reroot, same_tree


def stored(m, name):
    k = f"g{m['case']}_{name}_"
    return {c: Z[k + c] for c in COLS}


@pytest.mark.parametrize("m", META, ids=IDS)
def test_budget_and_visit_bookkeeping(m):
    """n_new follows the mode's rule; the root ends at start + n_new visits; a re-rooted root starts with the visits the played
    child had; a fresh root starts empty; no golden search was refused by the arena rule of its mode's default arena."""
    k = f"g{m['case']}_"
    n = m["n_sims"]
    maxch = geometry(m)[3]
    assert m["arena"] == 1 + (2 if m["mode"] == 1 else 1) * n * maxch
    stones = int((Z[k + "start_cells"] != 0).sum())
    reused, n_new, start, end = Z[k + "reused"], Z[k + "n_new"], Z[k + "start_visit"], Z[k + "root_visit"]
    assert reused[0] == 0 and m["reused"] == int(reused.sum()) and m["reused"] > 0
    for i in range(len(reused)):
        if reused[i]:
            assert n_new[i] == (n if m["mode"] == 1 else max(1, n - start[i]))
            assert start[i] >= 1 and Z[k + "kept"][i] > 1
            state_dim = 42 if m["game"] == "connect4" else geometry(m)[2]
            widest = min(maxch, state_dim - (stones + i))         # bounds the legal moves of every position below the root
            assert Z[k + "start_width"][i] <= widest
            assert Z[k + "kept"][i] + n_new[i] * widest <= m["arena"]                           # the arena rule
            pi_prev = Z[k + "pi"][i - 1]
            # the played child's share of the previous root's child visits is its visit count
            total = end[i - 1] - (0 if reused[i - 1] else 1)      # a fresh root's first simulation expands it: no child visit
            if not reused[i - 1]:
                assert round(pi_prev[action_of(m, int(Z[k + "chosen"][i - 1]))] * total) == start[i]
        else:
            assert n_new[i] == n and start[i] == 0 and Z[k + "kept"][i] == 1
        assert end[i] == start[i] + n_new[i]
        if m["mode"] == 2:
            assert end[i] == n or n_new[i] == 1
    noise_rows(m)                                                 # the rows can be drawn again (sha256 inside)


_FULL = [(m, name) for m in META for name in m["full"] if name.endswith("_start")]


@pytest.mark.parametrize("m,name", _FULL, ids=[f"{m['case']}-{name}" for m, name in _FULL])
def test_start_tree_is_the_chosen_childs_subtree(m, name):
    """Every stored start-of-search tree equals the chosen child's subtree of the previous move's end-of-search tree: visits and
    values bit for bit, priors as include/azk.h states them (root children mixed with the move's row under Dirichlet)."""
    mv = int(name[1:].split("_")[0])
    k = f"g{m['case']}_"
    prev = stored(m, f"m{mv - 1}_end")
    start = stored(m, name)
    noise = noise_rows(m)[mv] if m["dirichlet"] else None
    want = reroot(prev, int(Z[k + "chosen"][mv - 1]), lambda c: action_of(m, c), noise)
    assert same_tree(want, start)
    assert digest(start) == str(Z[k + "start_digest"][mv]) and digest(start, priors=False) == str(Z[k + "start_sdigest"][mv])
    end = stored(m, f"m{mv}_end")
    assert digest(end) == str(Z[k + "end_digest"][mv]) and digest(end, priors=False) == str(Z[k + "end_sdigest"][mv])
    assert len(start["depth"]) == Z[k + "kept"][mv] and int(start["visit"][0]) == Z[k + "start_visit"][mv]


@pytest.mark.parametrize("m", META, ids=IDS)
def test_first_move_equals_the_oracle(m):
    """Move 0 of every golden game is a fresh-root search: oracle.mcts on the same inputs, bit for bit (whole tree, pi, q)."""
    k = f"g{m['case']}_"
    game = ao.OracleGame(m["game"], m["size"] or None)
    cells = Z[k + "start_cells"]
    stones = int((cells != 0).sum())
    player = stones & 1
    board = game.board_from_cells(cells, player)
    tree = ao.OracleTree(game, cap=m["arena"])
    tree.reset(player, stones)

    def ev(canon):
        logits, v = fixture_logits_value(torch.from_numpy(np.ascontiguousarray(canon))[None], game.action_dim, m["variant"])
        return numpy_softmax_like_reference(logits[0].numpy()), float(v[0])
    noise = noise_rows(m)[0] if m["dirichlet"] else None
    ao.mcts(game, tree, board, m["n_sims"], ev, noise)
    e = tree.export()
    assert digest(e) == str(Z[k + "end_digest"][0])
    assert tree.pi().tobytes() == Z[k + "pi"][0].tobytes()
    assert tree.root_visit == Z[k + "root_visit"][0] == m["n_sims"]
    assert np.float64(tree.root_value / tree.root_visit).tobytes() == Z[k + "q"][0].tobytes()
