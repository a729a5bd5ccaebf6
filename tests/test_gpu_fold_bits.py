"""k_embed_fold (csrc/azk_nn.hip) held to its rows bit for bit: tests/golden/fold_rows_digest.npz carries one sha256 per board of
the rows the kernel gave before its instruction stream outside the tile loop was cut (tools/record_fold_rows.py, recorded from the
parent build), for the bf16 kernel and its float32 EX form, over board sets that reach every clipping of the patch, the tile
boundary, the board queue's series path (two workgroups for every board) and the three patch shapes.  The engine-leaf entry point
(the launch prologue: rank scan and rank -> game table) is held to the batch entry point on the gathered boards.

The issue asked for boards of exactly 16 and 17 dirty tokens.  No 15 x 15 position reaches exactly 17 tokens with 5 x 5 patches
(the reached set is a union of clipped rectangles: 9, 12, 15, 16, 18, 19, 20, ... - checked below), so the boundary is taken at
16, 18, 32 and 33: one full tile, the nearest count above it, two full tiles, and two full tiles plus one token."""
import ctypes as C

import numpy as np
import pytest
import torch

import fold_bits_common as fb
from conftest import load_golden
from fixture_eval import fixture_logits_value


def test_board_sets_cover_the_cases():
    boards, labels = fb.board_set("g15k5")
    assert boards.shape[1:] == (2, 15, 15) and len(labels) == boards.shape[0] >= 44
    for x, (label, nd) in zip(boards, labels):
        if nd is not None:
            assert fb.dirty_tokens(x, 5) == nd, label
    nds = sorted({fb.dirty_tokens(x, 5) for x in boards})
    assert {0, 9, 15, 16, 18, 32, 33, 225} <= set(nds)
    assert sum(1 for l, _ in labels if l.startswith("random")) == 20
    for name in ("g7k3", "t3k3"):
        b, l = fb.board_set(name)
        assert b.shape[1:] == (fb.CONFIGS[name][2],) + fb.CONFIGS[name][:2] and len(l) == b.shape[0]


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("name", list(fb.CONFIGS))
def test_fold_rows_equal_the_recorded_digests(name, exact):
    """Every board's rows equal the recording, with the default grid and with two workgroups taking every board in series (ticket,
    prefetch of the next board's cells, reuse of the LDS lists); the board queue is left zero."""
    want = load_golden("fold_rows_digest.npz")[fb.key(name, exact)]
    boards, labels = fb.board_set(name)
    assert len(want) == len(labels)                            # no board may be left out
    tables = fb.fold_tables(name, exact)
    for grid in (0, 2):
        rows, sched = fb.run_rows(name, boards, tables, exact, grid=grid)
        got = fb.digests(rows)
        bad = [labels[i][0] for i in range(len(labels)) if got[i] != want[i]]
        assert not bad, (grid, bad)
        assert sched == [0, 0], (grid, sched)


def _peek(ptr, count, dtype):
    hip = C.CDLL("libamdhip64.so")
    buf = np.empty(count, dtype)
    assert hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(buf.nbytes), 2) == 0
    return buf


@pytest.mark.gpu
@pytest.mark.parametrize("G,exact", [(5, False), (300, False), (2048, False), (300, True)], ids=["g5", "g300", "g2048", "g300-f32"])
def test_leaf_rows_equal_batch_rows_in_rank_order(G, exact):
    """azk_nn_embed_fold_leaves (SRC = true: rank scan, rank -> game table, cell codes) against azk_step_gather + the batch entry
    point on the same engine state: every row bit for bit in rank order (cost class descending, game ascending), n_leaf and
    leaf_slot as the ranks say.  The games start from random positions of 0 - 60 stones so that every cost class is present (the
    cells with (r + 2 c) % 5 == 0 stay empty: no line of five in any direction, so no game starts finished)."""
    import azk
    A = 225
    tables = fb.fold_tables("g15k5", exact)
    eng = azk.Engine("gomoku", G, 64, size=15, leaf_dtype="bfloat16", cache_entries=64)
    rng = np.random.RandomState(G)
    cells = np.zeros((G, A), np.int8)
    mc = rng.randint(0, 61, size=G)
    free = np.array([r * 15 + c for r in range(15) for c in range(15) if (r + 2 * c) % 5 != 0])
    for g in range(G):
        pick = rng.choice(free, size=mc[g], replace=False)
        cells[g, pick[0::2]] = 1
        cells[g, pick[1::2]] = 2
    eng.set_positions(cells, (mc & 1).tolist(), mc.tolist())
    noise, _ = eng.gen_noise(3, 0, 0)
    eng.begin_search(noise)
    logits = values = None
    for _ in range(6):
        eng.step_tree(logits, values)
        eng.step_gather()
        logits, values = fixture_logits_value(eng.leaf_boards.float(), A, "hash")
        logits, values = logits.contiguous(), values.contiguous()
    n = int(eng.n_leaf.item())
    assert 0 < n <= G
    sched = azk.new_sched("cuda")
    batch, leaves = (azk.nnx_embed_fold, azk.nnx_embed_fold_leaves) if exact else (azk.nn_embed_fold, azk.nn_embed_fold_leaves)
    ref = batch(eng.leaf_boards[:n].contiguous(), tables, 15, 15, sched)
    src = eng.leaf_source()
    torch.cuda.synchronize()
    gather_slot = _peek(src.leaf_slot, G, np.int32)
    fl = _peek(src.leaf_flag, G, np.uint8)
    eng.n_leaf.zero_()
    new = leaves(src, tables, sched)
    torch.cuda.synchronize()
    assert int(eng.n_leaf.item()) == n and sched.tolist() == [0, 0]
    new_slot = _peek(src.leaf_slot, G, np.int32)
    games = np.nonzero(fl)[0]
    assert len(games) == n
    if G >= 300:
        assert len(set(fl[games].tolist())) >= 4               # several cost classes: the rank order is not the game order
    order = sorted(games.tolist(), key=lambda g: (-int(fl[g]), g))
    assert [int(new_slot[g]) for g in order] == list(range(n))
    idle = np.setdiff1d(np.arange(G), games)
    assert np.array_equal(new_slot[idle], gather_slot[idle])   # games without a leaf keep their slot word
    want = ref[torch.from_numpy(gather_slot[order].astype(np.int64)).cuda()]
    assert torch.equal(new[:n], want)
    # twice more: the ranks, the rows and the queue do not depend on the schedule
    again = leaves(src, tables, sched)
    torch.cuda.synchronize()
    assert torch.equal(again[:n], want) and sched.tolist() == [0, 0]
    eng.close()
