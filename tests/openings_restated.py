"""Random openings (azk_set_openings), restated in plain Python: the draws through a Philox4x32-10 of its own, the plies
through the oracle's rule primitives (oracle.az_oracle: make_move, check_winner, Connect4's landing cell).  The engine's flags are never the
checker.  openings = (p_open, max_plies, spread).

A game that starts in slot g under move key `key` (the key of its first search), gg = first_game + g:
    game draw   counter {gg lo, gg hi, key, 0xFFFFFFFA}: c0 from words (0, 1), c1 from (2, 3); opened iff c0 < p_open,
                n = min(1 + floor(c1 * max_plies), max_plies)
    ply j < n   counter {gg lo, gg hi ^ ((j + 1) << 8), key, 0xFFFFFFFA}: u from words (0, 1); with m candidates (legal actions inside the
                window, ascending action index) the side to move plays candidate min(floor(u * m), m - 1); m == 0 ends the opening; a ply
                that decides the game or fills the board is taken back and ends it (cut short)."""
import math

import numpy as np

M32 = 0xFFFFFFFF
TAG = 0xFFFFFFFA


def philox4x32_10(c, k0, k1):
    c = list(c)
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & M32, p1 & M32, ((p0 >> 32) ^ c[3] ^ k1) & M32, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def _u(hi, lo):
    return float(((hi << 32) | lo) >> 11) * 2.0 ** -53


def game_draw(seed, gg, key, p_open, max_plies):
    """(opened, n plies) of the game (seed, gg, key)."""
    w = philox4x32_10([gg & M32, (gg >> 32) & M32, key & M32, TAG], seed & M32, (seed >> 32) & M32)
    c0, c1 = _u(w[0], w[1]), _u(w[2], w[3])
    if not c0 < p_open:
        return False, 0
    return True, min(1 + int(math.floor(c1 * max_plies)), max_plies)


def ply_uniform(seed, gg, key, j):
    w = philox4x32_10([gg & M32, ((gg >> 32) ^ ((j + 1) << 8)) & M32, key & M32, TAG], seed & M32, (seed >> 32) & M32)
    return _u(w[0], w[1])


def in_window(rows, cols, r, c, spread, columns_only=False):
    if spread < 0:
        return True
    col_ok = abs(2 * c - (cols - 1)) <= 2 * spread
    return col_ok if columns_only else (col_ok and abs(2 * r - (rows - 1)) <= 2 * spread)


def candidates(og, board, spread):
    """The cells the side to move may be given, ascending by action index (Connect4: the landing cell of each open column in the window)."""
    occupied = (board[0] != 0) | (board[1] != 0)
    if og.name == "connect4":
        landing = {int(c) % og.cols: int(c) for c in og.valid_cells(board)}          # the oracle's rule: (lowest empty row, col) per open column
        return [landing[c] for c in range(og.cols) if c in landing and in_window(og.rows, og.cols, 0, c, spread, True)]
    return [r * og.cols + c for r in range(og.rows) for c in range(og.cols)
            if not occupied[r, c] and in_window(og.rows, og.cols, r, c, spread)]


class Opening:
    """One game's start: board (the oracle's float32 planes), player to move, plies (== len(cells)), the cells played, and how it went."""
    __slots__ = ("board", "player", "plies", "cells", "opened", "cut", "n", "ended_empty")

    def codes(self):
        """int8 cell codes as Engine.get_positions returns them."""
        return (self.board[0] != 0).astype(np.int8).reshape(-1) + 2 * (self.board[1] != 0).astype(np.int8).reshape(-1)


def open_game(og, seed, gg, key, openings):
    """The position game (seed, gg, key) starts from under openings = (p_open, max_plies, spread)."""
    p_open, max_plies, spread = openings
    o = Opening()
    o.board, o.player, o.plies, o.cells, o.cut, o.ended_empty = og.new_board(), 0, 0, [], False, False
    o.opened, o.n = game_draw(seed, gg, key, p_open, max_plies)
    for j in range(o.n):
        cand = candidates(og, o.board, spread)
        m = len(cand)
        if m == 0:
            o.ended_empty = True
            break
        cell = cand[min(int(math.floor(ply_uniform(seed, gg, key, j) * m)), m - 1)]
        mover = o.player
        nxt = og.make_move(o.board, mover, og.rc(cell))
        if og.check_winner(o.board, mover, og.rc(cell)) != -1 or o.plies + 1 == og.state_dim:
            og.undo_move(o.board, nxt, og.rc(cell))               # decided or full: the ply is taken back
            o.cut = True
            break
        o.player = nxt
        o.plies += 1
        o.cells.append(int(cell))
    return o


def stats_of(opens):
    """[games opened, opening plies, openings cut short] over a list of Opening."""
    return [sum(1 for o in opens if o.opened), sum(o.plies for o in opens), sum(1 for o in opens if o.cut)]
