"""Evaluation under a board symmetry (azk_set_eval_symmetry) on the GPU, through the C ABI: the two kernels alone on every
geometry class, whole trees against the oracle driven by the restated wrapper (tests/eval_symmetry_restated.py) in every stepping and cache
mode, the option against itself on an equivariant evaluator, the runners against each other, the fused evaluator's leaf path, the refusals."""
import ctypes as C
import hashlib
import struct

import numpy as np
import pytest
import torch

import eval_symmetry_restated as es
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import assert_same_records, async_records, lockstep_records, ring_rows, shared

pytestmark = pytest.mark.gpu

G, N_SIMS = 6, 48
KEYED = ((1, 5), (1, 2 ** 40 + 7))
#        id          game         size      rows cols planes
GEOMS = {"ttt": ("tictactoe", None, 3, 3, 3), "g1x3": ("gomoku", (1, 3), 1, 3, 2), "g4x6": ("gomoku", (4, 6), 4, 6, 2),
         "g6x4": ("gomoku", (6, 4), 6, 4, 2), "g5": ("gomoku", 5, 5, 5, 2), "g7": ("gomoku", 7, 7, 7, 2), "g15": ("gomoku", 15, 15, 15, 2),
         "g17x18": ("gomoku", (17, 18), 17, 18, 2), "c4": ("connect4", None, 6, 7, 3)}
KERNEL_GEOMS = ["ttt", "g1x3", "g4x6", "g6x4", "g5", "g15", "g17x18", "c4"]


def ao():
    from oracle import az_oracle
    return az_oracle


def hash_eval(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def positions(gid, n=G, seed=0):
    """n positions of the geometry reached by alternating legal play without a winner, slot g after about g plies (so both sides are to
    move and one board is empty): [(cells int8, side to move, plies)], computed once per geometry."""
    def make():
        name, size, rows, cols, _ = GEOMS[gid]
        og = ao().OracleGame(name, size)
        rng = np.random.RandomState(1000 + seed)
        out = []
        for g in range(n):
            want = min(g, 2 if rows * cols == 3 else 5 if rows * cols < 12 else g)
            for _ in range(200):
                board, player, ok = og.new_board(), 0, True
                for _ply in range(want):
                    legal = og.valid_cells(board)
                    cell = int(legal[rng.randint(len(legal))])
                    mover = player
                    player = og.make_move(board, player, og.rc(cell))
                    if og.check_winner(board, mover, og.rc(cell)) != -1:
                        ok = False
                        break
                if ok:
                    break
            assert ok
            out.append(((board[0] + 2 * board[1]).astype(np.int8).reshape(-1), player, want))
        return out
    return shared(("sym positions", gid, n, seed), make)


def engine(gid, n_sims=N_SIMS, n=G, **kw):
    import azk
    name, size = GEOMS[gid][:2]
    return azk.Engine(name, n, n_sims, size=size, **kw)


def load(eng, pos):
    eng.set_positions(np.stack([p[0] for p in pos]), [p[1] for p in pos], [p[2] for p in pos])


def digest(e):
    h = hashlib.sha256()
    for d, c, n, w, p in zip(e["depth"], e["cell"], e["visit"], e["value"], e["prior"]):
        h.update(struct.pack("<iiqdd", int(d), int(c), int(n), float(w), float(p)))
    return h.hexdigest(), len(e["depth"])


# ---- 1. the kernels alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gid", KERNEL_GEOMS)
def test_kernels_alone(gid):
    """One select step from set positions (the pending leaf of a fresh root is the root's own position), then what the evaluator is handed
    and what comes back: the gathered planes, the element bytes, the restore."""
    name, size, rows, cols, planes = GEOMS[gid]
    valid = es.valid_elements(name, rows, cols)
    pos = positions(gid)
    canon = [es.canonical_planes(c, side, planes, rows, cols) for c, side, _ in pos]
    eng = engine(gid, 8)
    A = eng.action_dim
    assert eng.eval_symmetry is None
    rng = np.random.RandomState(3)
    for mode, value in [(2, s) for s in valid] + list(KEYED):
        load(eng, pos)
        eng.set_eval_symmetry(mode, value)
        eng.begin_search(None)
        eng.step_select()
        assert int(eng.n_leaf.item()) == G
        want = [value if mode == 2 else es.position_element(value, c, side, valid) for c, side, _ in pos]
        assert eng.leaf_symmetry().cpu().tolist() == want, (mode, value)
        got = eng.leaf_boards.cpu().numpy()
        for g in range(G):
            assert np.array_equal(got[g], es.transform_planes(canon[g], want[g])), (mode, value, g)
        rows_in = torch.from_numpy(rng.uniform(-3, 3, (G + 2, A)).astype(np.float32)).to(eng.device)
        out = eng.restore_logits(rows_in, out=torch.full_like(rows_in, 7.0))
        keep = rows_in.clone()
        for g in range(G):                                                    # row g belongs to game g: every game has a leaf
            assert torch.equal(out[g], es.restore_rows(rows_in[g], want[g], name, rows, cols)), (mode, value, g)
        assert bool((out[G:] == 7.0).all()) and torch.equal(rows_in, keep)    # rows of no leaf and the caller's buffer: untouched
    if len(valid) == 8:
        assert len(set(es.position_element(KEYED[1][1], c, side, valid) for c, side, _ in pos)) > 1     # the keyed case mixed elements
    # off again: the plain planes, and the getters refuse
    import azk
    load(eng, pos)
    eng.set_eval_symmetry(0)
    eng.begin_search(None)
    eng.step_select()
    assert np.array_equal(eng.leaf_boards.cpu().numpy(), np.stack(canon))
    with pytest.raises(azk.AzkError):
        eng.leaf_symmetry()
    eng.check_error()
    eng.close()


# ---- 2. whole trees against the oracle driven by the wrapped fixture -----------------------------------------------------------------------
def oracle_trees(gid, mode, value):
    """Per slot the oracle's tree under restore . hash fixture . transform, and the slots' noise rows: computed once per (geometry, mode)."""
    def make():
        name, size, rows, cols, _ = GEOMS[gid]
        og = ao().OracleGame(name, size)
        f = es.wrap(hash_eval(og.action_dim), name, rows, cols, mode, value)
        noise = np.random.RandomState(11).dirichlet([0.3] * og.action_dim, G)
        trees = []
        for g, (cells, side, plies) in enumerate(positions(gid)):
            tree = ao().OracleTree(og)
            tree.reset(side, plies)

            def ev(canon):
                logits, v = f(torch.from_numpy(np.ascontiguousarray(canon))[None])
                return ao().softmax_det(logits[0].numpy()), float(v[0])
            ao().mcts(og, tree, og.board_from_cells(cells, side), N_SIMS, ev, noise[g])
            trees.append(digest(tree.export()))
        return trees, noise
    return shared(("sym oracle", gid, mode, value), make)


def run_search(eng, stepping, noise):
    ev = hash_eval(eng.action_dim)
    if stepping == "fused":
        eng.search(ev, N_SIMS, noise)
    elif stepping == "split":
        eng.begin_search(noise)
        for _ in range(N_SIMS):
            eng.step_select()
            n = int(eng.n_leaf.item())
            if n > 0:
                eng.step_expand_backup(*eng.evaluate_leaves(ev, n))
            elif eng.cache_entries:
                eng.step_expand_backup(*eng.placeholder_rows())
    else:
        eng.search_budget(ev, N_SIMS, noise, per_launch=3)
    eng.check_error()


CACHES = {"off": {}, "game": dict(cache_entries=64), "shared": dict(cache_entries=64, cache_shared=True)}
TREE_CASES = [("g7", m, st, "off") for m in [(2, s) for s in range(8)] + list(KEYED) for st in ("fused", "budget")]
TREE_CASES += [("g7", (1, 5), "split", "off")]
for _gid in ("ttt", "c4", "g4x6", "g6x4", "g15", "g7"):
    _valid = es.valid_elements(GEOMS[_gid][0], GEOMS[_gid][2], GEOMS[_gid][3])
    for _m in ((1, 5), (2, _valid[-1])):
        TREE_CASES += [(_gid, _m, st, c) for st, c in (("fused", "game"), ("budget", "game"), ("fused", "shared"), ("budget", "shared"))]
        if _gid != "g7":
            TREE_CASES += [(_gid, _m, "fused", "off"), (_gid, _m, "budget", "off")]


@pytest.mark.parametrize("gid,mode,stepping,cache", TREE_CASES, ids=[f"{g}-m{m[0]}v{m[1]}-{s}-{c}" for g, m, s, c in TREE_CASES])
def test_whole_trees_are_the_oracles_under_the_wrapped_evaluator(gid, mode, stepping, cache):
    want, noise = oracle_trees(gid, *mode)
    eng = engine(gid, **CACHES[cache])
    eng.set_eval_symmetry(*mode)
    load(eng, positions(gid))
    run_search(eng, stepping, torch.from_numpy(noise).to(eng.device))
    for g in range(G):
        assert digest(eng.export_tree(g)) == want[g], (gid, mode, stepping, cache, g)
    if mode != (2, 0) and gid != "g1x3":
        plain, _ = oracle_trees(gid, 0, 0)
        assert plain != want                                       # the option shows on these searches: the fixture is not equivariant
    eng.close()


# ---- 3. an equivariant evaluator: option on == option off, independent of the restatement's maps ---------------------------------------------
@pytest.mark.parametrize("gid", ["g7", "c4", "g4x6", "ttt"])
def test_equivariant_evaluator_option_on_equals_option_off(gid):
    name, size, rows, cols, _ = GEOMS[gid]
    pos = positions(gid)
    noise = torch.from_numpy(np.random.RandomState(12).dirichlet([0.3] * (cols if name == "connect4" else rows * cols), G))
    trees = {}
    for mode in [(0, 0)] + [(2, s) for s in es.valid_elements(name, rows, cols)[1:]] + list(KEYED):
        eng = engine(gid, cache_entries=64 if mode[0] == 1 else 0)
        eng.set_eval_symmetry(*mode)
        load(eng, pos)
        ev = lambda x: es.equivariant_logits_value(x, eng.action_dim)
        if mode[0] == 1:
            eng.search_budget(ev, N_SIMS, noise.to(eng.device), per_launch=3)
        else:
            eng.search(ev, N_SIMS, noise.to(eng.device))
        eng.check_error()
        trees[mode] = [digest(eng.export_tree(g)) for g in range(G)]
        eng.close()
    assert trees[(0, 0)][0][1] > 20                                # (slot 0: the search from the empty board)
    for mode, t in trees.items():
        assert t == trees[(0, 0)], mode


# ---- 4. the runners -------------------------------------------------------------------------------------------------------------------------
MOVES, R_SIMS, R_G = 10, 24, 8


def test_graph_runner_equals_eager_stepping_with_the_option_on():
    kw = dict(cap=None, n_sims=R_SIMS, n_games=R_G, eval_symmetry=True, cache_entries=64)
    want = shared(("sym lock", "plain"), lambda: lockstep_records("gomoku", MOVES, **kw)[0])
    got, r = lockstep_records("gomoku", MOVES, use_graph=True, n_split=1, steps_per_graph=4, **kw)
    assert_same_records(got, want, MOVES, ("graph",), R_G)
    off = shared(("sym lock", "off"), lambda: lockstep_records("gomoku", MOVES, cap=None, n_sims=R_SIMS, n_games=R_G, cache_entries=64)[0])
    assert any(want[k][0] != off[k][0] for k in want if k in off)      # the option was on: recorded pi differ
    assert r.eng.eval_symmetry == (1, 3)                              # keyed by the runner's seed (test_gpu_playout_cap.SEED)


@pytest.mark.parametrize("reroot", [0, 2])
def test_async_equals_lockstep_slot_for_slot(reroot):
    lock_kw = dict(cap=None, n_sims=R_SIMS, n_games=R_G, eval_symmetry=True, cache_entries=64)
    async_kw = dict(lock_kw, per_launch=2, steps_per_graph=4)
    if reroot:
        lock_kw["tree_reuse"], async_kw["reroot"] = reroot, reroot
    want = shared(("sym lock", "plain" if not reroot else "reuse2"), lambda: lockstep_records("gomoku", MOVES, **lock_kw)[0])
    got, r = async_records("gomoku", MOVES, **async_kw)
    assert_same_records(got, want, MOVES, ("async", reroot), R_G)
    fixed = lockstep_records("gomoku", 3, cap=None, n_sims=R_SIMS, n_games=R_G, eval_symmetry=("fixed", 3), cache_entries=64)[0]
    assert any(fixed[k][0] != want[k][0] for k in fixed)


def test_replay_multiset_equals_lockstep():
    """Games played to the end without restarts on 5 x 5: the asynchronous drain emits the tuples the lock-step runner emits."""
    import azk
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner
    A, n, sims = 25, 8, 16
    ra, rb = azk.DeviceReplay(4096, 2, 5, 5, A), azk.DeviceReplay(4096, 2, 5, 5, A)
    r = SelfPlayRunner("gomoku", hash_eval(A), n, sims, size=5, seed=2, recycle=False, replay=ra, eval_symmetry=True)
    for _ in range(25):
        r.play_move()
    r.check_error()
    a = AsyncSelfPlayRunner("gomoku", hash_eval(A), n, sims, size=5, seed=2, recycle=False, replay=rb, per_launch=2, steps_per_graph=4,
                            use_graph=False, eval_symmetry=True)
    for _ in range(1000):
        a.run_chunk()
        if int(a.finish()[0]) == n:
            break
    assert int(a.finish()[0]) == n
    a.check_error()
    assert ra.size() == rb.size() > 50 and sorted(ring_rows(ra)) == sorted(ring_rows(rb))


# ---- 5. the fused path: the evaluator reads the engine's leaves ------------------------------------------------------------------------------
@pytest.mark.parametrize("element", [3, 4])
def test_fused_evaluator_reads_the_turned_leaves(element):
    """PolicyValueNet bf16 clsfold at 15 x 15: k_embed_fold over the engine's leaf source (the turned cells) against the same kernel - and the
    whole evaluator against the same network - on the restated-transformed board batch: bit for bit, as tests/test_gpu_fold.py and
    tests/test_gpu_nn.py assert leaves against a gathered batch."""
    import azk
    from pvnet import NetConfig, PolicyValueNet
    from selfplay import _evaluate_step, _Half
    n = 8
    cfg = NetConfig(15, 15, 2, 225, 5, 512, 8, 1)
    net = PolicyValueNet(cfg, seed=6, device="cuda", dtype=torch.bfloat16, path="clsfold")
    assert net._foldu is not None
    pos = positions("g15", n)
    eng = engine("g15", 8, n, leaf_dtype="bfloat16")
    load(eng, pos)
    plain_src = eng.leaf_source()
    eng.set_eval_symmetry(2, element)
    src = eng.leaf_source()
    assert src is not plain_src and src.leaf_cells != plain_src.leaf_cells       # the cached struct was dropped with the mode
    eng.begin_search(None)
    eng.step_tree(None, None)
    batch = torch.from_numpy(np.stack([es.transform_planes(es.canonical_planes(c, side, 2, 15, 15), element) for c, side, _ in pos]))
    batch = batch.to(eng.device).to(torch.bfloat16).contiguous()
    sched = azk.new_sched("cuda")
    ref = azk.nn_embed_fold(batch, net._foldu, 15, 15, sched)
    new = azk.nn_embed_fold_leaves(src, net._foldu, sched)
    torch.cuda.synchronize()
    assert int(eng.n_leaf.item()) == n
    slot = np.empty(n, np.int32)
    assert C.CDLL("libamdhip64.so").hipMemcpy(slot.ctypes.data_as(C.c_void_p), C.c_void_p(src.leaf_slot), C.c_size_t(slot.nbytes), 2) == 0
    assert sorted(slot.tolist()) == list(range(n))
    for g in range(n):
        assert torch.equal(new[int(slot[g])], ref[g]), g
    # the whole evaluator, as a runner's step hands the leaves to it
    h = _Half(torch, eng, False)
    _evaluate_step(net, eng, h, True)
    l_ref, v_ref = net(batch)
    torch.cuda.synchronize()
    assert C.CDLL("libamdhip64.so").hipMemcpy(slot.ctypes.data_as(C.c_void_p), C.c_void_p(src.leaf_slot), C.c_size_t(slot.nbytes), 2) == 0
    for g in range(n):
        assert torch.equal(h.logits_buf[int(slot[g])], l_ref[g].float()), g
        assert torch.equal(h.values_buf[int(slot[g])], v_ref.reshape(-1)[g].float()), g
    eng.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_engine_usable():
    import azk
    e46, c4 = engine("g4x6"), engine("c4", 8)
    with pytest.raises(azk.AzkError, match="error -1"):
        e46.set_eval_symmetry(2, 3)
    with pytest.raises(azk.AzkError, match="error -1"):
        c4.set_eval_symmetry(2, 2)
    with pytest.raises(azk.AzkError, match="error -1"):
        c4.set_eval_symmetry(3, 0)
    assert e46.eval_symmetry is None and c4.eval_symmetry is None
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    with pytest.raises(azk.AzkError, match="error -1"):
        vl.set_eval_symmetry(1, 5)
    with pytest.raises(azk.AzkError, match="error -1"):
        azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2, eval_symmetry=(1, 5))
    # in mid-search
    want, noise = oracle_trees("g4x6", 2, 6)
    noise = torch.from_numpy(noise).to(e46.device)
    load(e46, positions("g4x6"))
    e46.set_eval_symmetry(2, 6)
    e46.begin_search(noise)
    e46.step()
    with pytest.raises(azk.AzkError, match="error -1"):
        e46.set_eval_symmetry(1, 5)
    with pytest.raises(azk.AzkError, match="error -1"):
        e46.set_eval_symmetry(0)
    assert e46.eval_symmetry == (2, 6)
    # ... and the engine is as usable as before: the refused calls changed nothing
    load(e46, positions("g4x6"))
    run_search(e46, "fused", noise)
    assert [digest(e46.export_tree(g)) for g in range(G)] == want
    e46.advance(None, 0)
    e46.set_eval_symmetry(1, 5)                                     # between searches: accepted
    e46.set_eval_symmetry(0)
    load(e46, positions("g4x6"))
    run_search(e46, "budget", noise)
    assert [digest(e46.export_tree(g)) for g in range(G)] == oracle_trees("g4x6", 0, 0)[0]
    for e in (e46, c4, vl):
        e.close()
