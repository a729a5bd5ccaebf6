"""Every evaluator path and the searches it drives, pinned to the reference's own run of the seed-0 network (ai/nn.py Net under
torch.manual_seed(0), ai/mcts.py MCTS.mcts), not to another GPU path:
  * tests/golden/nn_edges.npz: the reference's logits / value of the depth-1 D = 512 network (main.py:134) and of the depth-2 D = 256
    network (main.py:186-188) on 47 boards where the compacted fold kernels do their least common work - stones on the conv padding
    and border tokens, one-colour, checkerboard, near-full and random dense boards - plus the reference's root forwards of the 92
    positions of tests/golden/nn_search15.npz;
  * tests/golden/nn_search15.npz: the reference's 800-simulation searches from the 92 positions of its recorded 15x15 games, fixture
    Dirichlet noise: child order, visits, value sums and priors of every root child.
The fixtures' own consistency (noise rows, child order, priors from the recorded logits bit for bit) is checked on the CPU in
tests/test_oracle_nn_reference.py."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import load_golden
from pvnet import NetConfig, PolicyValueNet

pytestmark = pytest.mark.gpu

CFG = NetConfig(15, 15, 2, 225, 5, 512, 8, 1)
CFG2 = NetConfig(15, 15, 2, 225, 5, 256, 8, 2)
EXACT_TAILS = ("h16", "h16-conv")            # h16: k_embed_fold<EX>; h16-conv: k_embed_pool_x (both in front of the fp16-pipe tail)


def canonical(cells, to_move):
    b = np.zeros((2, 225), np.float32)
    b[to_move] = cells == 1
    b[1 - to_move] = cells == 2
    return b.reshape(2, 15, 15)


def reference_searches():
    """(positions [(cells, to_move, move_count)], noise [92, 225] f64 (RandomState(7)'s rows, the draws the reference's searches
    consumed), per-position dicts of the reference's root children, root logits [92, 225] f32, root values [92] f32)."""
    z = load_golden("nn_search15.npz")
    off = z["child_off"]
    kids = [dict(cell=z["child_cell"][a:b].astype(np.int64), visit=z["child_visit"][a:b].astype(np.int64), value=z["child_value"][a:b],
                 prior=z["child_prior"][a:b]) for a, b in zip(off[:-1], off[1:])]
    pos = [(z["cells"][i], int(z["to_move"][i]), int(z["move_count"][i])) for i in range(len(kids))]
    noise = np.random.RandomState(7).dirichlet([0.03] * 225, size=len(pos))
    assert np.array_equal(z["child_noise"], np.concatenate([noise[i, k["cell"]] for i, k in enumerate(kids)]))
    return pos, noise, kids, z["root_logits"], z["root_value"]


def kat_boards():
    """nn_edges.npz's boards + the 92 root boards: x [n, 2, 15, 15], depth-1 logits / value, depth-2 logits / value (edge boards only:
    the first n_edges rows), names."""
    e = load_golden("nn_edges.npz")
    names = json.loads(bytes(e["names_json"]).decode())
    pos, _, _, rl, rv = reference_searches()
    x = np.concatenate([e["x"], np.stack([canonical(c, t) for c, t, _ in pos])])
    names = names + [f"root_{i}" for i in range(len(pos))]
    return (x, np.concatenate([e["d1_logits"], rl]), np.concatenate([e["d1_value"], rv]), e["d2_logits"], e["d2_value"],
            len(e["x"]), names)


def filler(n, seed):
    rng = np.random.RandomState(seed)
    x = np.zeros((n, 2, 15, 15), np.float32)
    for b in range(n):
        k = rng.randint(0, 60)
        cells = rng.choice(225, size=2 * k, replace=False)
        x[b, 0].reshape(-1)[cells[:k]] = 1
        x[b, 1].reshape(-1)[cells[k:]] = 1
    return x


# two placements of the KAT boards inside a 400-row batch whose device live count is 360: rows 5 .. 5 + n in order, and rows
# 211 + n - 1 .. 211 in reverse (neither start a multiple of 16; every KAT row below the live count)
BATCH, LIVE, OFF_A, OFF_B = 400, 360, 5, 211


def run_placed(net, x, dtype):
    """net's outputs for x's boards from both placements: (logits_a, value_a, logits_b, value_b) as float32 numpy, rows in x's order, and
    whether the path's value has bf16 precision (every value exactly representable in bf16)."""
    n = len(x)
    assert OFF_B + n <= LIVE and OFF_A + n <= OFF_B
    outs = []
    for off, order, seed in ((OFF_A, np.arange(n), 1), (OFF_B, np.arange(n)[::-1], 2)):
        xb = filler(BATCH, seed)
        xb[off:off + n] = x[order]
        net.live_count = torch.tensor([LIVE], dtype=torch.int32, device="cuda")
        lg, v = net(torch.from_numpy(xb).cuda().to(dtype))
        torch.cuda.synchronize()
        net.live_count = None
        v_bf16 = bool(torch.equal(v.float(), v.float().to(torch.bfloat16).float()))      # heads run in bf16 ('full', 'cls')
        lg, v = lg.float().cpu().numpy(), v.float().cpu().numpy().reshape(-1)
        inv = np.empty(n, np.int64)
        inv[order] = np.arange(n)
        outs += [lg[off:off + n][inv], v[off:off + n][inv]]
    return outs, v_bf16


def check_kat(tag, placed, ref_l, ref_v, tol_l, tol_v, names, value_rounding=True):
    """Prints the measured errors; returns the failures (empty list: within budget, and a board's row does not depend on where it
    sits in the batch).  value_rounding: a value computed in bf16 to the end also carries its final rounding, half a bf16 ulp
    (1.95e-3 for |v| in [0.5, 1)), on top of tol_v."""
    (la, va, lb, vb), v_bf16 = placed
    dl, dv = np.abs(la - ref_l).max(1), np.abs(va - ref_v)
    tv = tol_v + (np.exp2(np.floor(np.log2(np.abs(ref_v))) - 8) if v_bf16 and value_rounding else 0.0)       # bf16: 8 significant bits
    same = np.array_equal(la, lb) and np.array_equal(va, vb)
    print(f"{tag}: max |dlogit| {dl.max():.2e} ({names[int(dl.argmax())]}), max |dvalue| {dv.max():.2e} ({names[int(dv.argmax())]}), "
          f"placements identical {same}")
    bad = [names[i] for i in np.nonzero((dl > tol_l) | (dv > tv))[0]]
    return ([(tag, bad[:12], float(dl.max()), float(dv.max()))] if bad else []) + ([] if same else [(tag, "rows depend on the placement")])


def test_every_evaluator_path_on_edge_boards_against_the_reference():
    """The reference's seed-0 logits / value on 139 boards (47 edge boards + the 92 search roots), each board placed twice inside a
    400-row batch with a device live count of 360.  Budgets: float32 paths logits 1e-5 / value 1e-6 (north_star's bar; the torch
    'full' forward and the two fp32-accurate forms), bf16 paths logits 2e-2 / value 2e-3, plus the final rounding
    where the value is computed in bf16 to the end ('full', 'cls': tanh in bf16, whose half ulp at |v| in [0.5, 1) is 1.95e-3 - on the
    near-full board the torch bf16 forward lands 2.05e-3 from the reference, on the CPU as on the GPU).  A board's outputs are bit for
    bit the same in both placements.  Measured (logits / value): fp32 'full' 2.4e-6 / 1.2e-7, the fp32-accurate forms 1.2e-6 /
    6e-8 - 1.2e-7; bf16 'full' 1.0e-2 / 2.1e-3, 'cls' 9.9e-3 / 2.3e-3, 'clsfold' (float32 value) 8.7e-3 / 4.6e-4."""
    x, rl, rv, _, _, _, names = kat_boards()
    failures = []
    for path, dtype, tail, tol_l, tol_v in (("full", torch.float32, None, 1e-5, 1e-6),
                                            *(("clsfold", torch.float32, t, 1e-5, 1e-6) for t in EXACT_TAILS),
                                            ("full", torch.bfloat16, None, 2e-2, 2e-3), ("cls", torch.bfloat16, None, 2e-2, 2e-3),
                                            ("clsfold", torch.bfloat16, None, 2e-2, 2e-3)):
        net = PolicyValueNet(CFG, seed=0, device="cuda", dtype=dtype, path=path)
        if tail is not None:
            assert net._exact is not None
            net.use_fold_u = tail == "h16"
        failures += check_kat(f"{path} {str(dtype)[6:]}{' ' + tail if tail else ''}", run_placed(net, x, dtype), rl, rv, tol_l, tol_v, names)
    assert not failures, failures


def test_depth2_hand_written_path_on_edge_boards_against_the_reference(monkeypatch):
    """main.py:186-188's depth-2 D = 256 network on the 47 edge boards, bf16, hand-written kernels only (test_gpu_block.py's set-up:
    F.linear, bmm, matmul, addmm, einsum and scaled_dot_product_attention raise while it runs): logits within 2e-2 and value within
    1e-2 of the reference (the budgets of test_depth2_evaluator_on_hand_written_kernels_only)."""
    x, _, _, l2, v2, n_edges, names = kat_boards()
    x, names = x[:n_edges], names[:n_edges]
    net = PolicyValueNet(CFG2, seed=0, device="cuda", dtype=torch.bfloat16, path="clsfold")
    assert net._blocks is not None

    def banned(*a, **k):
        raise AssertionError("a library GEMM / attention entry point was called inside the hand-written forward")
    with monkeypatch.context() as mp:
        for mod, name in ((F, "linear"), (torch, "bmm"), (torch, "matmul"), (F, "scaled_dot_product_attention"), (torch, "addmm"), (torch, "einsum")):
            mp.setattr(mod, name, banned)
        net.last_forward_kernels = None
        outs = run_placed(net, x, torch.bfloat16)
    assert net.last_forward_kernels == "hand-written"
    failures = check_kat("depth-2 bf16 hand-written", outs, l2, v2, 2e-2, 1e-2, names, value_rounding=False)
    assert not failures, failures


# ---- searches ---------------------------------------------------------------------------------------------------------------------
def search_children(net, leaf_dtype, positions, noise, n_sims=800):
    import azk
    G = len(positions)
    eng = azk.Engine("gomoku", G, n_sims, size=15, leaf_dtype=leaf_dtype)
    try:
        eng.reset_games()
        eng.set_positions(np.stack([p[0] for p in positions]), [p[1] for p in positions], [p[2] for p in positions])
        eng.search(net, n_sims, torch.from_numpy(noise).cuda())
        eng.check_error()
        return [eng.root_children(g) for g in range(G)]
    finally:
        eng.close()


def compare_searches(got, ref, tag):
    """Per position: the child order must equal the reference's; returns (positions whose visits differ, max relative prior error,
    max child-Q error over the positions whose visits agree)."""
    diff, dp, dq = [], 0.0, 0.0
    for i, (g, r) in enumerate(zip(got, ref)):
        assert np.array_equal(g["cell"], r["cell"]), (tag, i)
        dp = max(dp, float((np.abs(g["prior"] - r["prior"]) / r["prior"]).max()))
        if not np.array_equal(g["visit"], r["visit"]):
            diff.append(i)
            continue
        seen = r["visit"] > 0
        assert (g["value"][~seen] == 0).all(), (tag, i)
        dq = max(dq, float(np.abs(g["value"][seen] / g["visit"][seen] - r["value"][seen] / r["visit"][seen]).max()))
    return diff, dp, dq


# Positions where a float32 evaluator on the GPU and the reference's CPU float32 forward lead the search to different visit counts
# (measured: none, for all four evaluators).
EXPECTED_DIFFERING = []


def test_exact_evaluator_searches_reproduce_the_reference():
    """800-simulation searches from the 92 positions of the reference's recorded 15x15 games with the fixture noise, under the
    fp32-accurate evaluator (both embedding forms) and, as a control, the torch float32 'full' forward: every root child's cell order and
    visit count equal the reference's own search (north_star's 1e-5 on visit-count policies: not one visit moves), child Q within 1e-5
    (measured <= 1.8e-7), priors within 1e-6 relative for the hand-written kernels (measured 7.2e-7 - 7.9e-7) and 2e-6 for the torch
    control (measured 1.44e-6: its logits are up to 2.4e-6 from the reference's, against the kernels' 1.4e-6; a prior also carries
    the engine's deterministic softmax, within 4 ulp of numpy's).  Measured: 92 / 92 positions identical under every one."""
    positions, noise, ref, _, _ = reference_searches()
    assert len(positions) == 92
    found = {}
    nets = [("full", None)] + [("clsfold", t) for t in EXACT_TAILS]
    for path, tail in nets:
        net = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path=path)
        if tail is not None:
            assert net._exact is not None
            net.use_fold_u = tail == "h16"
        tag = f"fp32 {path}{' ' + tail if tail else ''}"
        got = search_children(net, "float32", positions, noise)
        found[tag] = compare_searches(got, ref, tag)
        d, dp, dq = found[tag]
        print(f"{tag} vs reference search: {92 - len(d)}/92 positions with identical visits (differing: {d}), "
              f"max relative prior error {dp:.2e}, max |dQ| {dq:.2e}")
    for tag, (d, dp, dq) in found.items():
        assert d == EXPECTED_DIFFERING, (tag, d)
        assert dp <= (2e-6 if tag == "fp32 full" else 1e-6) and dq <= 1e-5, (tag, dp, dq)


def test_benched_bf16_searches_against_the_reference():
    """The benched evaluator (bf16, path 'clsfold') in the same 92 searches, against the reference's own pi (= child visits / 799).
    Measured: 87 / 92 positions identical, max |delta pi| 2.5e-3 (2 visits of 799), mean total variation 9.5e-5, no position changes
    its most-visited move.  Asserted: >= 85 identical (measured - 2), max |delta pi| <= 5e-3 (4 visits), mean TV <= 2e-4, the
    most-visited move changed in at most 1 position; and the rerun is identical."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from measure_nn_parity import reference_pi, search_pis
    positions, noise, _, _, _ = reference_searches()
    ref_pi = reference_pi()
    net16 = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.bfloat16, path="clsfold")
    pi16, _ = search_pis(net16, "bfloat16", positions, 800, torch.from_numpy(noise).cuda())
    d = np.abs(pi16 - ref_pi)
    identical = int((d.max(1) == 0).sum())
    tv = 0.5 * d.sum(1)
    changed = float((pi16.argmax(1) != ref_pi.argmax(1)).mean())          # share of positions
    print(f"bf16 clsfold vs reference search: {identical}/92 identical, max |dpi| {d.max():.2e}, mean TV {tv.mean():.2e}, "
          f"argmax changed {changed:.3f}")
    assert identical >= 85
    assert d.max() <= 5e-3 and tv.mean() <= 2e-4
    assert changed <= 1 / 92
    again, _ = search_pis(net16, "bfloat16", positions, 800, torch.from_numpy(noise).cuda())
    assert np.array_equal(again, pi16)
