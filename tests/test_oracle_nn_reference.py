"""The reference's own runs of the seed-0 network (tests/golden/nn_search15.npz: 800-simulation searches from the 92 positions of the
recorded 15x15 games; tests/golden/nn_edges.npz: outputs on boards where the fold kernels can go wrong) against the oracle and the
host-side network code.  CPU only: a GPU failure in tests/test_gpu_reference_nn.py can then be traced to the fixture, the fold
arithmetic or the kernels."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_meta, load_golden
from oracle import az_oracle as ao
from pvnet import NetConfig, PolicyValueNet

CFG = NetConfig(15, 15, 2, 225, 5, 512, 8, 1)
S = load_golden("nn_search15.npz")
E = load_golden("nn_edges.npz")
EDGE_NAMES = json.loads(bytes(E["names_json"]).decode())


def positions():
    """golden positions of the 15x15 games in games.npz (tools/measure_nn_parity.golden_positions' order)."""
    z = load_golden("games.npz")
    out = []
    for m in golden_meta(z):
        if m["size"] == 15:
            cells = z[f"g{m['game']}_board_cells"]
            out += [(cells[ply].astype(np.int8).reshape(-1), ply & 1, ply) for ply in range(len(cells))]
    return out


def root_boards():
    """The canonical root board of each position (plane 0 = side to move), as the search evaluated it."""
    x = np.zeros((len(S["cells"]), 2, 225), np.float32)
    for i, (c, t) in enumerate(zip(S["cells"], S["to_move"])):
        x[i, t] = c == 1
        x[i, 1 - t] = c == 2
    return x.reshape(-1, 2, 15, 15)


NOISE = np.random.RandomState(7).dirichlet([0.03] * 225, size=92)     # position i's Dirichlet draw: row i


def children(i):
    a, b = S["child_off"][i], S["child_off"][i + 1]
    return S["child_cell"][a:b].astype(np.int64), S["child_visit"][a:b].astype(np.int64), S["child_value"][a:b], S["child_prior"][a:b]


def test_search_fixture_positions_and_noise():
    pos = positions()
    assert len(pos) == len(S["cells"]) == 92
    for (c, t, m), c2, t2, m2 in zip(pos, S["cells"], S["to_move"], S["move_count"]):
        assert np.array_equal(c, c2) and t == t2 and m == m2
    for i in range(92):                                 # the draw the reference's search consumed, at its root children's cells
        a, b = S["child_off"][i], S["child_off"][i + 1]
        assert S["child_noise"][a:b].tobytes() == NOISE[i, S["child_cell"][a:b]].tobytes(), i


def test_search_fixture_visits_and_child_order():
    """Sum of child visits = root visits - 1 (the root's own expansion), and the children in the reference's CPython-set order of
    get_valid_moves, which the oracle reproduces."""
    meta = golden_meta(S)
    game = ao.OracleGame("gomoku", 15)
    for i, m in enumerate(meta):
        cell, visit, value, prior = children(i)
        assert m["root_visit"] == 800 and m["mcts_count"] == 800
        assert visit.sum() == m["root_visit"] - 1 and len(cell) == m["n_children"]
        assert np.array_equal(cell, game.valid_cells(game.board_from_cells(S["cells"][i])))
        assert (value[visit == 0] == 0).all() and (np.abs(value) <= visit).all()


def test_search_fixture_priors_are_the_recorded_root_forward_bit_for_bit():
    """Every root child's prior = 0.75 * softmax(root logits)[cell] + 0.25 * noise[cell] in the reference's arithmetic, bit for bit
    (mcts.py:47's numpy softmax; utils.py:24-25: the float32 product, then a float64 sum): the recorded batch-1 root forward is the one
    the search used.  oracle.softmax_det (the engine's softmax) is within 4 ulp of that numpy expression (test_oracle_numerics)."""
    for i in range(92):
        cell, _, _, prior = children(i)
        lg = S["root_logits"][i]
        p = np.exp(lg) / np.sum(np.exp(lg))
        want = (0.75 * p).astype(np.float64) + 0.25 * NOISE[i]
        assert p.dtype == np.float32 and want[cell].tobytes() == prior.tobytes(), i
        np.testing.assert_allclose(ao.softmax_det(lg), p, rtol=5e-7, atol=0)


def fold_u_forward(net, x):
    """logits, value by pvnet.fold_u's formulas (what k_embed_fold<EX> + the tail compute), float64 end to end."""
    r = net.exact_fold("cpu")
    u, _, _, _ = net.forward_fold_u_emulated(x)
    f8 = lambda t: t.double()
    ln = lambda t: (t - t.mean(1, keepdim=True)) / torch.sqrt(t.var(1, unbiased=False, keepdim=True) + 1e-5)
    x1 = u @ f8(r["Wo"]).t() + f8(r["bias1"])
    x2 = x1 + F.gelu(ln(x1) @ f8(r["W0G"]).t() + f8(r["b0G"])) @ f8(r["W3"]).t() + f8(r["b3"])
    out = ln(x2) @ f8(r["WhG"]).t() + f8(r["bhG"])
    return out[:, :225].float(), torch.tanh(out[:, 225:226]).float()


def kat_boards():
    names = EDGE_NAMES + [f"root_{i}" for i in range(92)]
    return (torch.from_numpy(np.concatenate([E["x"], root_boards()])), np.concatenate([E["d1_logits"], S["root_logits"]]),
            np.concatenate([E["d1_value"], S["root_value"]]), names)


def test_edge_fixture_boards():
    """The edge boards are legal canonical inputs and cover what they are meant to: the empty board, single stones at the corners and
    edge midpoints, dense and near-full boards."""
    x = E["x"]
    assert x.shape == (len(EDGE_NAMES), 2, 15, 15) and not (x[:, 0] * x[:, 1]).any()
    n = x.sum((1, 2, 3))
    assert n.min() == 0 and n.max() >= 224
    for name in ("empty", "own_14_14", "opp_0_0", "row14", "col14", "patch_10_10", "own_only_120", "opp_only_40", "checker",
                 "random_224_0", "position_91"):
        assert name in EDGE_NAMES
    assert x[EDGE_NAMES.index("row14")][:, :14].sum() == 0 and x[EDGE_NAMES.index("col14")][:, :, :14].sum() == 0


@pytest.mark.parametrize("path", ["full", "cls"])
def test_torch_forward_against_the_reference(path):
    """The float32 torch paths on the 47 edge boards + 92 root boards: test_pvnet.py's budget, logits 5e-5 / value 2e-5 (measured
    5e-7 / 6e-8)."""
    x, rl, rv, names = kat_boards()
    logits, v = PolicyValueNet(CFG, seed=0, path=path)(x)
    dl = np.abs(logits.numpy() - rl).max(1)
    dv = np.abs(v.numpy().reshape(-1) - rv)
    assert dl.max() < 5e-5 and dv.max() < 2e-5, (names[int(dl.argmax())], dl.max(), dv.max())


@pytest.mark.parametrize("form", ["exact_fold", "fold_u"])
def test_fold_emulations_against_the_reference(form):
    """The float64 emulations of the fp32-accurate kernels' folds - exact_fold (k_embed_pool_x) and fold_u (k_embed_fold<EX>) - on the
    same boards: the exact path's bar, logits 1e-5 / value 1e-6 (measured 1.4e-6 / 6e-8, the worst on a single stone at the border)."""
    x, rl, rv, names = kat_boards()
    net = PolicyValueNet(CFG, seed=0, path="full")
    if form == "exact_fold":
        logits, v, _ = net.forward_exact_emulated(x)
    else:
        logits, v = fold_u_forward(net, x)
    dl = np.abs(logits.numpy() - rl).max(1)
    dv = np.abs(v.numpy().reshape(-1) - rv)
    assert dl.max() < 1e-5 and dv.max() < 1e-6, (names[int(dl.argmax())], dl.max(), names[int(dv.argmax())], dv.max())


def test_depth2_network_against_the_reference_on_edge_boards():
    """main.py:186-188's depth-2 D = 256 network on the edge boards, float32 CPU, both paths: within 2e-5 (measured 8e-7 / 2.4e-7),
    far inside test_gpu_block.py's bf16 budget of 2e-2."""
    net = PolicyValueNet(NetConfig(15, 15, 2, 225, 5, 256, 8, 2), seed=0, path="full")
    x = torch.from_numpy(E["x"])
    for path in ("full", "cls"):
        logits, v = net(x, path=path)
        assert np.abs(logits.numpy() - E["d2_logits"]).max() < 2e-5, path
        assert np.abs(v.numpy().reshape(-1) - E["d2_value"]).max() < 2e-6, path
