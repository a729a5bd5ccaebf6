"""k_embed_fold's board hand-out (csrc/azk_nn.hip): workgroup b of a grid of Gd takes boards b, 2 Gd - 1 - b, 2 Gd + b, 4 Gd - 1 - b, ...
below the live count - a fixed schedule, no shared ticket.  With the grid capped at 4 workgroups, 3 / 4 / 5 / 8 / 9 / 12 / 13 boards
end a workgroup's list in every position of the forward and the backward sweep (one board short of a sweep, a full sweep, one board
into the next), so a board handed out twice, left out, or written to another board's slot shows in the rows or in the work counters.
The rows are held bit for bit to the same boards at the default grid (one workgroup per board: no hand-out at all), which
tests/test_gpu_fold_bits.py in turn holds to the recorded digests."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fold_bits_common as fb
from fixture_eval import fixture_logits_value

NAME = "g15k5"
COUNTS = (3, 4, 5, 8, 9, 12, 13)
# mixed cost classes, heavy and light in no order: 15 tiles, none, one, three, a few each
PICK = ("nearly-full", "empty", "dirty16", "random3", "corner00-p0", "dirty33", "random7", "side0", "edge-left-p1", "random12", "dirty18",
        "side1", "random19")


@functools.lru_cache(maxsize=None)
def _tables(exact):
    return fb.fold_tables(NAME, exact)


@functools.lru_cache(maxsize=None)
def _boards():
    boards, labels = fb.board_set(NAME)
    index = {label: i for i, (label, _) in enumerate(labels)}
    x = np.ascontiguousarray(boards[[index[p] for p in PICK]])
    tiles = [(fb.dirty_tokens(b, 5) + 15) // 16 for b in x]
    assert len(set(tiles)) >= 4 and max(tiles) == 15 and min(tiles) == 0
    return x, tiles


@functools.lru_cache(maxsize=None)
def _reference(exact):
    """The 13 boards at the default grid, once per number format (never written to)."""
    rows, sched = fb.run_rows(NAME, _boards()[0], _tables(exact), exact, grid=0)
    assert sched == [0, 0]
    rows.setflags(write=False)
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("exact", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("n", COUNTS)
def test_four_workgroups_give_the_default_grids_rows(n, exact):
    boards, tiles = _boards()
    tables = _tables(exact)
    want = _reference(exact)[:n]
    stats = tables.enable_work_stats()
    stats.zero_()
    rows, sched = fb.run_rows(NAME, boards[:n], tables, exact, grid=4)
    bad = [PICK[i] for i in range(n) if not np.array_equal(rows[i], want[i])]
    assert not bad, bad
    assert stats.tolist() == [n, sum(tiles[:n])]                # every board once, with its own tiles
    assert sched == [0, 0]


def _peek(ptr, count, dtype):
    hip = C.CDLL("libamdhip64.so")
    buf = np.empty(count, dtype)
    assert hip.hipMemcpy(buf.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(buf.nbytes), 2) == 0
    return buf


@pytest.mark.gpu
def test_leaf_rows_in_rank_order_with_four_workgroups():
    """The engine-leaf entry point at 300 games (tests/test_gpu_fold_bits.py test_leaf_rows_equal_batch_rows_in_rank_order) with four
    workgroups sweeping the ranks forth and back dozens of times each: rows, leaf slots and the live count as the ranks say."""
    import azk
    G, A = 300, 225
    tables = _tables(False)
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
    assert 4 < n <= G
    sched = azk.new_sched("cuda")
    ref = azk.nn_embed_fold(eng.leaf_boards[:n].contiguous(), tables, 15, 15, sched)     # default grid
    src = eng.leaf_source()
    torch.cuda.synchronize()
    gather_slot = _peek(src.leaf_slot, G, np.int32)
    fl = _peek(src.leaf_flag, G, np.uint8)
    games = np.nonzero(fl)[0]
    assert len(games) == n and len(set(fl[games].tolist())) >= 4
    order = sorted(games.tolist(), key=lambda g: (-int(fl[g]), g))
    want = ref[torch.from_numpy(gather_slot[order].astype(np.int64)).cuda()]
    stats = tables.enable_work_stats()
    stats.zero_()
    eng.n_leaf.zero_()
    assert azk.lib().azk_nn_embed_fold_grid(4) == 0
    try:
        new = azk.nn_embed_fold_leaves(src, tables, sched)
        torch.cuda.synchronize()
    finally:
        assert azk.lib().azk_nn_embed_fold_grid(0) == 0
    assert int(eng.n_leaf.item()) == n and sched.tolist() == [0, 0]
    assert int(stats[0].item()) == n
    new_slot = _peek(src.leaf_slot, G, np.int32)
    assert [int(new_slot[g]) for g in order] == list(range(n))
    assert torch.equal(new[:n], want)
    eng.close()
