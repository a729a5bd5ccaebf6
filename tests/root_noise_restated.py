"""Root noise on the legal moves (azk_set_root_noise), restated in plain Python over rng_restated.gamma_rows: the legal set
from the cell codes by the rules as include/azk.h states them, the row from the float64 Gamma draws of the product RNG's restatement.  Test
infrastructure: no GPU, no libazk.  The engine's rows are never the checker.

For game gg at move key k, in a position whose legal actions are L (n = |L|):
    alpha_eff = alpha ("legal") or alpha / n ("total")
    a in L:      gam[a] = gamma_rows(...).gam[a] at alpha_eff - entry a's stream {gg lo, gg hi ^ (a << 8), k, it} and it | 0x40000000 -,
                 row[a] = gam[a] / sum_L gam, or 1 / n where that sum is 0
    a not in L:  row[a] = +0.0
An entry's stream does not depend on the row's length (test_rng_restated.py shows it), so "legal" is gen_noise's row restricted and renormalised."""
from collections import namedtuple

import numpy as np

import rng_restated as R

MODES = ("legal", "total")
NoiseRows = namedtuple("NoiseRows", "rows gam margin tries legal")


def geometry(game, size=None):
    """(rows, cols, A) of a game."""
    if game == "tictactoe":
        return 3, 3, 9
    if game == "connect4":
        return 6, 7, 7
    rows, cols = (int(size[0]), int(size[1])) if isinstance(size, (tuple, list)) else (int(size), int(size))
    return rows, cols, rows * cols


def legal_actions(game, size, cells):
    """The action indices that are legal in a position given as cell codes (0 empty), ascending: TicTacToe the empty cells, Connect4 the
    columns whose top cell is empty, Gomoku the empty cells with a stone among their eight neighbours - the centre cell where there is none."""
    rows, cols, _ = geometry(game, size)
    c = [int(x) for x in np.asarray(cells).reshape(-1)]
    assert len(c) == rows * cols
    if game == "tictactoe":
        return [i for i in range(9) if c[i] == 0]
    if game == "connect4":
        return [col for col in range(cols) if c[col] == 0]
    out = set()
    for r in range(rows):
        for q in range(cols):
            if c[r * cols + q] == 0:
                continue
            for dr in (-1, 0, 1):
                for dq in (-1, 0, 1):
                    rr, qq = r + dr, q + dq
                    if (dr or dq) and 0 <= rr < rows and 0 <= qq < cols and c[rr * cols + qq] == 0:
                        out.add(rr * cols + qq)
    if not out:
        out.add((rows // 2) * cols + cols // 2)
    return sorted(out)


def noise_rows(game, size, cells, seed, first_game, key, mode, alpha, *, _plant=None):
    """The rows of games first_game .. first_game + G - 1 at move key `key`, game g in the position cells[g].  Returns NoiseRows: rows [G][A],
    and over the legal entries only (elsewhere 0 / inf / 0) the Gamma draws, the decision margins and the tries of gamma_rows; legal[g] the
    legal actions.  _plant is for the tests of this module alone: "all" normalises over all A entries, the recipe the option replaces."""
    assert mode in MODES and _plant in (None, "all")
    _, _, A = geometry(game, size)
    cells = np.asarray(cells)
    G = len(cells)
    legal = [legal_actions(game, size, cells[g]) for g in range(G)]
    rows, gam = np.zeros((G, A)), np.zeros((G, A))
    margin, tries = np.full((G, A), np.inf), np.zeros((G, A), np.int64)
    drawn = {}
    for g in range(G):
        n = len(legal[g])
        if n == 0:                                                # a full TicTacToe or Connect4 board: a row of zeros
            continue
        a_eff = float(alpha) if mode == "legal" else float(alpha) / n
        if a_eff not in drawn:
            drawn[a_eff] = R.gamma_rows(A, seed, first_game, G, key, a_eff)
        d, L = drawn[a_eff], legal[g]
        gam[g, L], margin[g, L], tries[g, L] = d.gam[g, L], d.margin[g, L], d.tries[g, L]
        if _plant == "all":
            rows[g, L] = d.rows[g, L]
            continue
        tot = float(np.sum(d.gam[g, L]))
        rows[g, L] = d.gam[g, L] / tot if tot > 0.0 else 1.0 / n
    return NoiseRows(rows, gam, margin, tries, legal)


# ---------------------------------------------------------------------------------------------------------------------------------
# the positions and settings of tests/test_gpu_root_noise.py (test_root_noise_restated.py shows on the CPU that their legal sets are the
# rules' and that none of their draws has a borderline accept / reject)
# ---------------------------------------------------------------------------------------------------------------------------------
def _board(rows, cols, stones):
    """cell codes with stones [(r, c), ...] alternating 1, 2."""
    cells = np.zeros(rows * cols, np.int8)
    for i, (r, c) in enumerate(stones):
        cells[r * cols + c] = 1 + (i & 1)
    return cells


def _filled(rows, cols, empty):
    """a board with every cell taken but the cells `empty` (rows are made from the cells alone: no search starts here)."""
    cells = np.array([1 + (((c >> 1) + (r >> 1)) & 1) for r in range(rows) for c in range(cols)], np.int8)
    for r, c in empty:
        cells[r * cols + c] = 0
    return cells


def _connect4(heights):
    """cell codes of a Connect4 board (row 0 is the top) whose column c holds heights[c] stones, alternating from the bottom."""
    cells = np.zeros(42, np.int8)
    for c, h in enumerate(heights):
        for k in range(h):
            cells[(5 - k) * 7 + c] = 1 + ((k + c) & 1)
    return cells


def _wide(n):
    import forced_playouts_restated as fr                          # (solver_restated.fr: the same function)
    return fr.wide_cells(n)


# (name, cells, legal actions expected); to_move and move_count follow from the stone count (rows are made from the cells alone)
POSITIONS = {
    ("tictactoe", None): [("empty", np.zeros(9, np.int8), 9), ("one left", np.array([1, 2, 1, 1, 2, 2, 2, 1, 0], np.int8), 1)],
    ("connect4", None): [("empty", _connect4([0] * 7), 7), ("one full column", _connect4([0, 2, 0, 6, 1, 0, 3]), 6),
                         ("one column left", _connect4([6, 6, 6, 6, 6, 6, 2]), 1)],
    ("gomoku", 7): [("empty", np.zeros(49, np.int8), 1), ("corner stone", _board(7, 7, [(0, 0)]), 3), ("centre stone", _board(7, 7, [(3, 3)]), 8),
                    ("one empty", _filled(7, 7, [(6, 6)]), 1), ("two empty", _filled(7, 7, [(0, 3), (4, 0)]), 2)],
    ("gomoku", (5, 9)): [("three stones", _board(5, 9, [(0, 8), (2, 4), (4, 0)]), 14), ("empty", np.zeros(45, np.int8), 1)],
    ("gomoku", 15): [("wide 6", _wide(6), 48), ("wide 12", _wide(12), 96), ("wide 24", _wide(24), 192)],
    # cell 256 = (12, 16) is the first of the second dword half; (19, *) and (*, 19) are the last row and column
    ("gomoku", 20): [("both halves", _board(20, 20, [(0, 0), (5, 19), (12, 15), (12, 16), (13, 5), (19, 0), (19, 10), (19, 19), (10, 19), (18, 18)]), 46),
                     ("last cell", _board(20, 20, [(19, 19)]), 3)],
}
GEOMETRIES = tuple(POSITIONS)
SEED = R.LAW_SEED
ALPHAS = (0.03, 0.3, 10.83)
FIRST_GAMES = (0, 2 ** 32 - 2)
KEYS = (0, 1, 511)
ROW_G = 8                                                          # games per engine: the positions of its geometry, cycled
SETTINGS = [(mode, alpha, first, key) for mode in MODES for alpha in ALPHAS for first in FIRST_GAMES for key in KEYS]


def cells_of(geom, G=ROW_G):
    """[G][rc] cell codes: game g stands in position g % (positions of the geometry)."""
    pos = POSITIONS[geom]
    return np.stack([pos[g % len(pos)][1] for g in range(G)])


def to_move_and_count(cells):
    """(to_move, move_count) per game from the stone counts (player 0 moves first)."""
    mc = (np.asarray(cells) != 0).sum(axis=1).astype(np.int32)
    return (mc & 1).astype(np.int32), mc
