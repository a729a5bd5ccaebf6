"""Evaluation under a board symmetry (include/azk.h azk_set_eval_symmetry), restated in plain Python and numpy
(TEST INFRASTRUCTURE, not product code): the maps src_s / dst_s, the elements a geometry admits, the position hash, and a wrapper that
turns any evaluator f into restore_s . f . transform_s - the evaluator an engine with the option on is equivalent to, which the oracle's
search can be driven by.  Nothing here reads the engine; tests/test_eval_symmetry_restated.py holds it to numpy's own rot90 / fliplr /
flipud and to the hash condition of the header."""
import numpy as np

M32 = 0xFFFFFFFF
INVERSE = (0, 1, 2, 7, 4, 5, 6, 3)            # rot90 <-> rot270; every other element is its own inverse


def valid_elements(game, rows, cols):
    if game == "connect4":
        return (0, 1)                          # gravity keeps the rows
    return tuple(range(8)) if rows == cols else (0, 1, 2, 6)


def src_cell(s, i, c, rows, cols):
    """Source (row, column) of output cell (i, c) under element s of the emission's order (np.rot90 is counter-clockwise)."""
    n = cols                                   # the elements that transpose exist on square boards only
    return [(i, c), (i, cols - 1 - c), (rows - 1 - i, c), (c, n - 1 - i), (n - 1 - c, n - 1 - i), (c, i), (rows - 1 - i, cols - 1 - c),
            (n - 1 - c, i)][s]


def src_map(s, rows, cols):
    """int array [rows * cols]: transformed[j] = board[src_map[j]]."""
    assert s in (0, 1, 2, 6) or rows == cols
    out = np.empty(rows * cols, np.int64)
    for i in range(rows):
        for c in range(cols):
            si, sc = src_cell(s, i, c, rows, cols)
            out[i * cols + c] = si * cols + sc
    return out


def dst_map(s, rows, cols):
    """The inverse permutation: dst_map[src_map[j]] = j."""
    src = src_map(s, rows, cols)
    out = np.empty_like(src)
    out[src] = np.arange(len(src))
    return out


def action_dst_map(s, game, rows, cols):
    """restored[a] = row[action_dst_map[a]]: the cells' dst_s, or Connect4's column map a -> cols - 1 - a."""
    if game == "connect4":
        assert s in (0, 1)
        return np.arange(cols)[::-1].copy() if s == 1 else np.arange(cols)
    return dst_map(s, rows, cols)


def transform_cells(cells, s, rows, cols):
    return np.asarray(cells).reshape(-1)[src_map(s, rows, cols)]


def transform_planes(x, s):
    """x [..., F, R, C] (numpy or torch): every plane turned by element s."""
    rows, cols = x.shape[-2], x.shape[-1]
    flat = x.reshape(*x.shape[:-2], rows * cols)
    idx = src_map(s, rows, cols)
    if not isinstance(x, np.ndarray):
        import torch
        idx = torch.from_numpy(idx).to(x.device)
    return flat[..., idx].reshape(x.shape)


def restore_rows(rows_, s, game, rows, cols):
    """rows_ [..., A]: the evaluator's rows (in the transformed frame) turned back into the position's frame."""
    idx = action_dst_map(s, game, rows, cols)
    if not isinstance(rows_, np.ndarray):
        import torch
        idx = torch.from_numpy(idx).to(rows_.device)
    return rows_[..., idx]


def fmix(h):
    """murmur3's 32-bit finaliser."""
    h &= M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def position_element(seed, cells, side, valid):
    """The element of mode 1: cells = the position's cell codes (0 empty, 1 player 0's stone, 2 player 1's), side = the side to move."""
    seed_lo, seed_hi = seed & M32, (seed >> 32) & M32
    h = fmix(seed_hi ^ side ^ 0x9E3779B9)
    for i, code in enumerate(np.asarray(cells).reshape(-1).tolist()):
        if code:
            h = (h + fmix(((i << 2) | int(code)) ^ seed_lo)) & M32
    r = fmix(h)
    return valid[((r >> 16) * len(valid)) >> 16]


def canonical_planes(cells, side, planes, rows, cols):
    """The evaluator's input for a position: own stones first, then the opponent's (gomoku.py:34-40), plane 2 = the side to move."""
    c = np.asarray(cells).reshape(rows, cols)
    x = np.zeros((planes, rows, cols), np.float32)
    x[0], x[1] = c == 1 + side, c == 2 - side
    if planes == 3:
        x[2] = side
    return x


def cells_and_side(canon):
    """(cell codes, side to move) of one canonical board [F, R, C] of a game played by alternating moves, player 0 first: plane 2 says
    the side where there is one, else the stone counts do (equal: player 0 to move)."""
    own, opp = np.asarray(canon[0]) != 0, np.asarray(canon[1]) != 0
    side = int(np.asarray(canon[2]).flat[0]) if canon.shape[0] == 3 else int(own.sum() != opp.sum())
    return (own * (1 + side) + opp * (2 - side)).astype(np.int8).reshape(-1), side


def wrap(evaluator, game, rows, cols, mode, value):
    """f -> restore_s . f . transform_s over board batches: evaluator(x [n, F, R, C] torch) -> (logits [n, A], values [n]); mode 1: s is
    the position's element under seed `value`, mode 2: s = value; mode 0: f itself."""
    import torch
    valid = valid_elements(game, rows, cols)

    def wrapped(x):
        if mode == 0:
            return evaluator(x)
        xs = x.detach().cpu().numpy()
        els = [value if mode == 2 else position_element(value, *cells_and_side(b), valid) for b in xs]
        turned = torch.stack([transform_planes(x[i], s) for i, s in enumerate(els)])
        logits, values = evaluator(turned)
        return torch.stack([restore_rows(logits[i], s, game, rows, cols) for i, s in enumerate(els)]), values
    return wrapped


def equivariant_logits_value(x, action_dim):
    """A fixture evaluator that IS equivariant under every element its board admits: integer logits from the stone counts in each cell's
    8-neighbourhood (Connect4: summed down the column), the value from the stone counts; every float32 operation exact.
    x [n, F, R, C] torch holding 0 / 1 -> (logits [n, A] float32, values [n] float32)."""
    import torch
    n, rows, cols = x.shape[0], x.shape[2], x.shape[3]
    p = x[:, :2].to(torch.int64)
    pad = torch.zeros((n, 2, rows + 2, cols + 2), dtype=torch.int64, device=x.device)
    pad[:, :, 1:-1, 1:-1] = p
    nb = sum(pad[:, :, 1 + di:1 + di + rows, 1 + dc:1 + dc + cols] for di in (-1, 0, 1) for dc in (-1, 0, 1) if (di, dc) != (0, 0))
    t = 2 * nb[:, 0] + 3 * nb[:, 1] - 5 * (p[:, 0] + p[:, 1])
    t = t.sum(dim=1) if action_dim == cols and action_dim != rows * cols else t.reshape(n, rows * cols)
    own, opp = p[:, 0].sum(dim=(1, 2)), p[:, 1].sum(dim=(1, 2))
    v = (((own * 7 + opp * 13 + 3) % 64) - 32).to(torch.float32) * (1.0 / 32.0)
    return t.to(torch.float32) * 0.25, v
