"""k_embed_fold's leaf front by dword (azk_nn.hip, CW): a two-plane engine's leaf comes in as one cell dword per lane and the board bit
string is built from nibbles and DPP steps instead of byte loads and ballots.  Every check here is exact and follows
test_gpu_fold_bits.test_leaf_rows_equal_batch_rows_in_rank_order: azk_step_gather + the batch entry point (whose code takes boards, not
cell codes) is the reference, the leaf entry point on the same engine state is the code under test, rows meet through leaf_slot.

The start positions hold one to five stones and no line, so no game is finished and the first step_tree leaves every game with its
root as the pending leaf (depth 0: the side to move of the leaf is the side set)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import fold_bits_common as fb

pytestmark = pytest.mark.gpu


def _hip():
    return C.CDLL("libamdhip64.so")


def _peek(ptr, count, dtype):
    buf = np.empty(count, dtype)
    assert _hip().hipMemcpy(buf.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), C.c_size_t(buf.nbytes), 2) == 0
    return buf


def _poke(ptr, buf):
    buf = np.ascontiguousarray(buf)
    assert _hip().hipMemcpy(C.c_void_p(ptr), buf.ctypes.data_as(C.c_void_p), C.c_size_t(buf.nbytes), 1) == 0


@functools.lru_cache(maxsize=None)
def _tables(R, Cc, planes, k, exact):
    """As fold_bits_common.fold_tables, for any board shape."""
    import azk
    from pvnet import NetConfig, PolicyValueNet
    net = PolicyValueNet(NetConfig(R, Cc, planes, R * Cc, k, 512, 8, 1), seed=fb.SEED, device="cuda", dtype=torch.float32, path="full")
    r = net.fold_u()
    assert r is not None, (R, Cc, planes, k)                    # the shape must reach k_embed_fold
    return azk.EmbedFoldTables(r, 8, k, 512, "cuda", exact=exact)


def _sweep(rc):
    """2 rc positions [2 rc, rc] of one stone: cell g % rc in colour 1 + g // rc."""
    cells = np.zeros((2 * rc, rc), np.int8)
    g = np.arange(2 * rc)
    cells[g, g % rc] = 1 + g // rc
    return cells


def _extras_15():
    """Stones at the string's ends and at the seam between the planes (bit 225: plane 1 begins one bit into a dword; cells 224 and 0 are
    neighbours there), in both colours; 220-224 is the last, partial dword and the one before it.  Mixed colours: no line of five."""
    rows = []
    for a, b in ((1, 2), (2, 1)):
        x = np.zeros(225, np.int8)
        x[[0, 2]], x[[1, 3]] = a, b
        rows.append(x)
        x = np.zeros(225, np.int8)
        x[[220, 222, 224]], x[[221, 223]] = a, b
        rows.append(x)
        x = np.zeros(225, np.int8)
        x[224], x[0] = a, b
        rows.append(x)
        x = np.zeros(225, np.int8)
        x[[0, 1, 2, 3]], x[[221, 222, 223, 224]] = a, b
        rows.append(x)
    return np.stack(rows)


class _Leaves:
    """An engine one step_tree + step_gather into its first search, the batch rows of its leaf boards, and the leaf entry point."""

    def __init__(self, game, size, cells, side, tables, exact):
        import azk
        self.azk, self.tables, self.exact = azk, tables, exact
        G = len(cells)
        self.G = G
        self.eng = eng = azk.Engine(game, G, 8, size=size, leaf_dtype="bfloat16")
        side = np.broadcast_to(np.asarray(side, np.int32), (G,))
        eng.set_positions(cells, side.tolist(), (cells != 0).sum(1).tolist())
        eng.begin_search(None)
        eng.step_tree(None, None)
        eng.step_gather()
        n = int(eng.n_leaf.item())
        assert n == G                                           # every game has a leaf: nothing is finished
        self.sched = azk.new_sched("cuda")
        batch = azk.nnx_embed_fold if exact else azk.nn_embed_fold
        self.boards = eng.leaf_boards[:n].contiguous()
        self.ref = batch(self.boards, tables, eng.rows, eng.cols, self.sched)
        self.src = eng.leaf_source()
        torch.cuda.synchronize()
        self.gather_slot = torch.from_numpy(_peek(self.src.leaf_slot, G, np.int32).astype(np.int64)).cuda()

    def rows(self):
        """The leaf entry point's rows, game by game (through the slots it wrote), after checking n_leaf and the queue words."""
        self.eng.n_leaf.zero_()
        new = (self.azk.nnx_embed_fold_leaves if self.exact else self.azk.nn_embed_fold_leaves)(self.src, self.tables, self.sched)
        torch.cuda.synchronize()
        assert int(self.eng.n_leaf.item()) == self.G and self.sched.tolist() == [0, 0]
        slot = _peek(self.src.leaf_slot, self.G, np.int32)
        assert sorted(slot.tolist()) == list(range(self.G))     # every game a slot of its own
        return new[torch.from_numpy(slot.astype(np.int64)).cuda()]

    def want(self):
        return self.ref[self.gather_slot]

    def check_sweep_boards(self, rc, side):
        """The reference's own input: game g of the sweep shows one stone, at cell g % rc of plane (g // rc) ^ side."""
        b = self.boards[self.gather_slot[:2 * rc]].float().reshape(2 * rc, 2, rc).cpu().numpy()
        want = np.zeros_like(b)
        g = np.arange(2 * rc)
        want[g, (g // rc) ^ side, g % rc] = 1.0
        assert np.array_equal(b, want)


def _run_sweep(R, Cc, k, side, exact=False, extras=None):
    rc = R * Cc
    cells = _sweep(rc) if extras is None else np.concatenate([_sweep(rc), extras])
    lv = _Leaves("gomoku", (R, Cc), cells, side, _tables(R, Cc, 2, k, exact), exact)
    try:
        assert lv.src.planes == 2 and lv.src.rc == rc and lv.src.rc_pad == (rc + 15) // 16 * 16
        lv.check_sweep_boards(rc, side)
        got, want = lv.rows(), lv.want()
        bad = [g for g in range(lv.G) if not torch.equal(got[g], want[g])]
        assert not bad, bad[:20]
    finally:
        lv.eng.close()


@pytest.mark.parametrize("side", [0, 1])
def test_every_bit_position_15x15(side):
    """15 x 15, 5 x 5 patches (the benched shape): a stone at every cell in either colour - 450 games - and the ends-and-seam games, with
    every game's side to move `side`: the canonical swap sends every cell through both planes."""
    _run_sweep(15, 15, 5, side, extras=_extras_15())


@pytest.mark.parametrize("side", [0, 1])
@pytest.mark.parametrize("shape", [(7, 7, 3), (14, 18, 5), (15, 16, 5)], ids=["7x7k3", "14x18k5", "15x16k5"])
def test_every_bit_position_other_seams(shape, side):
    """The same sweep where rc falls differently in a dword and a row: 7 x 7 k3 (rc 49, rc_pad 64: the plane seam at bit 17 of word 1,
    eleven lanes past the row), 14 x 18 k5 (rc 252, rc_pad 256: all 64 lanes load, no partial dword, the largest board the fold covers),
    15 x 16 k5 (rc = rc_pad = 240: no padding).  All three reach k_embed_fold (fold_u() gives tables for them)."""
    _run_sweep(*shape, side)


def test_every_bit_position_15x15_exact():
    """The float32-accurate instantiation (azk_nnx_embed_fold_leaves) takes the same front."""
    _run_sweep(15, 15, 5, 1, exact=True, extras=_extras_15())


def test_padding_of_a_cell_row_is_not_trusted():
    """Bytes [225, 240) of every leaf_cells row set to 0xFF: the rows do not change.  (The engine is closed without another step.)"""
    cells = np.concatenate([_sweep(225)[::7], _extras_15()])
    lv = _Leaves("gomoku", (15, 15), cells, np.arange(len(cells)) & 1, _tables(15, 15, 2, 5, False), False)
    try:
        want = lv.want()
        assert torch.equal(lv.rows(), want)
        pad = lv.src.rc_pad
        assert pad == 240
        raw = _peek(lv.src.leaf_cells, lv.G * pad, np.uint8).reshape(lv.G, pad)
        assert not raw[:, 225:].any() and np.array_equal(raw[:, :225].astype(np.int8), cells)
        raw[:, 225:] = 0xFF
        _poke(lv.src.leaf_cells, raw)
        assert (_peek(lv.src.leaf_cells, lv.G * pad, np.uint8).reshape(lv.G, pad)[:, 225:] == 0xFF).all()
        assert torch.equal(lv.rows(), want)
    finally:
        lv.eng.close()


def test_three_planes_still_take_the_byte_form():
    """3 x 3 with three planes (t3k3): not a two-plane source, so the cell codes come in by byte and the rows equal the batch rows.  One
    stone at every cell in either colour and three two-stone positions, each with either side to move."""
    one = _sweep(9)
    two = np.zeros((3, 9), np.int8)
    two[0, [0, 8]], two[1, [4, 5]], two[2, [2, 6]] = (1, 2), (2, 1), (1, 2)
    cells = np.concatenate([one, two, one, two])
    side = np.repeat([0, 1], len(one) + len(two))
    lv = _Leaves("tictactoe", None, cells, side, _tables(3, 3, 3, 3, False), False)
    try:
        assert lv.src.planes == 3
        got, want = lv.rows(), lv.want()
        bad = [g for g in range(lv.G) if not torch.equal(got[g], want[g])]
        assert not bad, bad
    finally:
        lv.eng.close()
