"""k_embed_fold (csrc/azk_nn.hip) through its batch entry points - azk.nn_embed_fold (bf16 rows) and azk.nnx_embed_fold (the float32-accurate
EX form) - at the sixteen shapes of fold_restated.SHAPES, pinned two ways.  Exact probes: synthetic tables (eps = 0) under which the
kernel's float32 arithmetic is exact in any order, so that every output entry is known from the plain-loop patch layout alone - which
tokens see a stone, at which patch bit, the compaction into tiles, the head lanes, the 1 / L slots, the zero columns.  Float64: the real
seed-6 tables of each shape against fold_restated.fold_f64, entry by entry, within a bound derived from the number formats and the
operation counts of the kernel's source (fold_restated.bound); no block-maximum tolerance.  tests/test_fold_restated.py proves every
probe's expected value on the CPU and shows which probe notices which mistake; DESIGN.md, "What pins k_embed_fold", lists what the
kernel's own deliberate mistakes turn red.

Each float64 test prints `RATIO <name> <largest error / bound>` before it asserts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fold_restated as fr

pytestmark = pytest.mark.gpu

SHAPE_IDS = ["x".join(map(str, s)) for s in fr.SHAPES]
shapes = pytest.mark.parametrize("shape", list(fr.SHAPES), ids=SHAPE_IDS)
forms = pytest.mark.parametrize("form", fr.FORMS)
S = fr.SENTINEL


@functools.lru_cache(maxsize=None)
def _tables(shape, form, kind=None):
    """azk.EmbedFoldTables of a probe (eps = 0) or, kind None, of the seed-6 network of the shape (fold_u() on the CPU in float64: the
    reference evaluates the very operands the kernel's tables were packed from)."""
    import azk
    if kind is None:
        return azk.EmbedFoldTables(fr.real_tables(shape)[1], 8, shape[3], 512, "cuda", exact=form == "f32")
    return azk.EmbedFoldTables(fr.probe_tables(kind, shape), 8, shape[3], 512, "cuda", eps=0.0, exact=form == "f32")


@functools.lru_cache(maxsize=2)
def _probe(kind, shape):
    boards = fr.probe_boards(kind, shape)
    return boards, fr.probe_expected(kind, shape, boards)


@functools.lru_cache(maxsize=1)
def _reference(shape):
    boards = fr.bound_boards(shape)
    return boards, fr.fold_f64(fr.real_tables(shape)[1], fr.patch_bits(boards, shape[3]), 1e-5)


@pytest.fixture(autouse=True, scope="module")
def release_tables():
    """Tables, boards and references are shared by the tests of this file and dropped with the last of them."""
    yield
    for f in (_tables, _probe, _reference, fr.real_tables):
        f.cache_clear()
    torch.cuda.empty_cache()


def _run(form, x, tables, shape, count=None, rows_behind=0):
    """One launch on boards x [n, C, R, Cc] (bf16 or float32, on the card) -> (rows [n + rows_behind, 8, 384] pre-filled with the
    sentinel, the schedule words after it)."""
    import azk
    R, Cc, planes, k = shape
    n = x.shape[0]
    out = torch.full((n + rows_behind, 8, azk.EMBED_FOLD_ROW), S, dtype=torch.float32 if form == "f32" else torch.bfloat16, device="cuda")
    sched = azk.new_sched("cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    fn = getattr(azk.lib(), "azk_nnx_embed_fold" if form == "f32" else "azk_nn_embed_fold")
    rc = fn(x.data_ptr(), 1 if x.dtype == torch.float32 else 0, C.byref(tables.c), out.data_ptr(), n, planes, R, Cc,
            None if cnt is None else cnt.data_ptr(), sched.data_ptr(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out, sched.tolist()


def _both_board_types(form, boards, tables, shape):
    """The rows from bf16 boards, after checking that float32 boards give the same rows, that the default grid leaves the schedule words
    zero and that the rows behind the batch keep the sentinel."""
    x = torch.from_numpy(boards).cuda().contiguous()
    r16, s16 = _run(form, x.to(torch.bfloat16).contiguous(), tables, shape, rows_behind=2)
    r32, s32 = _run(form, x, tables, shape, rows_behind=2)
    assert s16 == [0, 0] and s32 == [0, 0]
    assert torch.equal(r16, r32)
    assert bool((r16[len(boards):].float() == S).all())
    return fr.decode(r16[:len(boards)], form)


@pytest.mark.parametrize("kind", fr.KINDS)
@forms
@shapes
def test_exact_probes_bit_for_bit(shape, form, kind):
    """fold_restated.probe_tables / probe_boards / probe_expected.  selection: a stone at every cell of every stone plane (three planes:
    under either side plane) and the empty board; a token's entry is 2^(t mod 4 - h) where a stone reaches it and 0 elsewhere, the pooled
    patch holds the same power of two at the one bit the stone has in that token's patch.  count: many-stone boards with a = 1: the
    pooled patch is (tokens holding bit k) / 2^h, an integer of at most 252; count2: L = (reached tokens + 1) / 2.  diagonal: G diagonal,
    one set cell anywhere in any plane: rstd = 2^(k mod 4) through the fp16 fragments, the accumulator layout and the bit pairing.
    float32 rows are held to their bits everywhere (count2: to the numpy float32 quotient).  bf16 rows are held to their bits wherever
    the expected value is a bf16 number, which is everywhere but count2's quotients and the selection probe's sums over a set side
    plane: there, and in the 1 / L remainder slot, to the window fold_restated.probe_window derives (the value itself unless it lies
    within 2^-20 of a rounding tie).  The zero columns are part of the window."""
    T = fr.tokens(shape)
    boards, e = _probe(kind, shape)
    got = _both_board_types(form, boards, _tables(shape, form, kind), shape)
    lo, hi = fr.probe_window(kind, shape, e, form)
    bad = fr.in_window(got, lo, hi)
    assert len(bad) == 0, (len(bad), [(tuple(i), got[tuple(i)], lo[tuple(i)], hi[tuple(i)]) for i in bad[:8]])
    if form == "bf16":
        assert np.array_equal(got[:, :, T], got[:, :, T + 2])
        worst = float(np.max(np.abs(got[:, :, T] + got[:, :, T + 1] - e["inv"]) / fr.inv_sum_bound(e["inv"])))
        print(f"RATIO inv_sum_{kind}_{'x'.join(map(str, shape))} {worst:.4f}")
        assert worst <= 1.0, worst


@forms
@shapes
def test_within_the_float64_bound(shape, form):
    """The seed-6 tables of the shape; empty, full, checkerboard, the one-stone sweep thinned to every third cell, 40 random boards of
    every density and, at its three shapes, fold_bits_common's recorded set (so the boards behind tests/golden/fold_rows_digest.npz are
    shown to lie within the bound of float64).  Every entry of the token weights, the pooled patch and the 1 / L slots against
    fold_restated.bound: half an ulp of the output format plus the propagated float32 terms; the zero columns are asserted zero.
    Largest error / bound on an MI355X: see DESIGN.md, "What pins k_embed_fold"."""
    r = fr.real_tables(shape)[1]
    boards, o = _reference(shape)
    got = _both_board_types(form, boards, _tables(shape, form), shape)
    worst = fr.check_rows(got, o, fr.bound(r, o, 1e-5, form), fr.tokens(shape), form)
    print(f"RATIO f64_{'x'.join(map(str, shape))}_{form} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("grid", [1, 2, 3, 5])
def test_every_board_is_taken_once(grid):
    """azk_nn_embed_fold_grid(g): g workgroups sweep the boards forth and back.  At 15 x 15 and 6 x 7, both forms, n in 1, g, g + 1, 2 g,
    2 g + 1, 4 g + 3 (both directions of the sweep, a partial last sweep): the rows are those of the default grid bit for bit, as a batch
    of n and as 4 g + 3 boards under a device-side count of n, where the rows from the count on keep the sentinel."""
    import azk
    for shape in ((15, 15, 2, 5), (6, 7, 3, 3)):
        boards = np.stack(fr.stone_boards(shape, 31, 4 * grid + 3, 0.02, 0.6))
        x = torch.from_numpy(boards).cuda().to(torch.bfloat16).contiguous()
        for form in fr.FORMS:
            tables = _tables(shape, form)
            want, sched = _run(form, x, tables, shape)
            assert sched == [0, 0]
            assert azk.lib().azk_nn_embed_fold_grid(grid) == 0
            try:
                for n in sorted({1, grid, grid + 1, 2 * grid, 2 * grid + 1, 4 * grid + 3}):
                    got, sched = _run(form, x[:n].contiguous(), tables, shape, rows_behind=1)
                    assert sched == [0, 0] and torch.equal(got[:n], want[:n]) and bool((got[n:].float() == S).all()), (shape, form, n)
                    got, sched = _run(form, x, tables, shape, count=n)
                    assert sched == [0, 0] and torch.equal(got[:n], want[:n]) and bool((got[n:].float() == S).all()), (shape, form, n, "count")
            finally:
                assert azk.lib().azk_nn_embed_fold_grid(0) == 0


def _connect4_positions():
    """[18, 42] cell codes of legal Connect4 positions without a line of four: one disc at the bottom of each column in either colour,
    and four stacked positions of at most three discs a column, coloured 1 + ((col / 2 + row) & 1): no run longer than two in a row,
    three in a column or on a diagonal."""
    cells = []
    for colour in (1, 2):
        for col in range(7):
            x = np.zeros((6, 7), np.int8)
            x[5, col] = colour
            cells.append(x)
    for heights in ((3, 3, 3, 3, 3, 3, 3), (1, 2, 3, 0, 1, 2, 3), (0, 0, 3, 3, 0, 1, 0), (2, 0, 0, 0, 0, 0, 2)):
        x = np.zeros((6, 7), np.int8)
        for col, h in enumerate(heights):
            for i in range(h):
                x[5 - i, col] = 1 + (((col >> 1) + i) & 1)
        cells.append(x)
    return np.stack(cells).reshape(len(cells), 42)


@forms
def test_leaf_entry_point_on_connect4(form):
    """A 6 x 7 three-plane engine one step into a search (test_gpu_fold_cells._Leaves): the gathered leaf boards are the canonical planes
    of the positions as fold_restated.canonical_planes states them (the third plane the side to move), and the leaf entry point's rows
    equal the batch rows of those boards bit for bit, with either side to move.  The batch rows themselves are held by the tests above."""
    from test_gpu_fold_cells import _Leaves
    one = _connect4_positions()
    cells = np.concatenate([one, one])
    side = np.repeat([0, 1], len(one))
    shape = (6, 7, 3, 3)
    lv = _Leaves("connect4", None, cells, side, _tables(shape, form), form == "f32")
    try:
        assert lv.src.planes == 3 and lv.src.rc == 42 and lv.eng.rows == 6 and lv.eng.cols == 7
        seen = lv.boards[lv.gather_slot].float().reshape(len(cells), 3, 42).cpu().numpy()
        want_boards = np.stack([fr.canonical_planes(cells[g], int(side[g]), 3) for g in range(len(cells))])
        assert np.array_equal(seen, want_boards)
        got, want = lv.rows(), lv.want()
        bad = [g for g in range(lv.G) if not torch.equal(got[g], want[g])]
        assert not bad, bad
    finally:
        lv.eng.close()
