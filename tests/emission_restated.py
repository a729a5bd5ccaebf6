"""(state, pi, z) emission under a mask of D4 elements (include/azk.h azk_config.emit_elements), restated in plain numpy
(TEST INFRASTRUCTURE, not product code): the expected tuple list of one finished game from its record, and the pick and turn of
azk_replay_gather.  Nothing here reads the engine; tests/test_emission_restated.py holds it to numpy's own flips and, on square boards, to
the reference-pinned oracle (oracle/replay_oracle.py)."""
import hashlib

import numpy as np

from eval_symmetry_restated import src_map


def canonical(board, side):
    """The facade's canonical-board rule (games/game.py get_canonical_board; gomoku.py:34-40): own stones first; plane 2, where there is
    one, stays the side to move."""
    board = np.asarray(board, np.float32)
    if side == 0:
        return board
    out = board.copy()
    out[0], out[1] = board[1], board[0]
    return out


def turn(state, pi, s, game):
    """(state [F, R, C], pi [A]) under element s: planes out[j] = in[src_s(j)]; pi with the cells, or - Connect4's column actions -
    mirrored under element 1."""
    planes, rows, cols = state.shape
    src = src_map(s, rows, cols)
    st = np.ascontiguousarray(state.reshape(planes, rows * cols)[:, src].reshape(planes, rows, cols))
    pi = np.asarray(pi, np.float64)
    if game == "connect4":
        assert s in (0, 1) and len(pi) == cols
        return st, (pi[::-1].copy() if s == 1 else pi.copy())
    assert len(pi) == rows * cols
    return st, pi[src].copy()


def emit_tuples(game, boards, pis, winner, elements, full=None):
    """-> list of (state float32 [F, R, C], pi float64 [A], z float), in ring order, for one finished game: boards / pis / winner as
    SelfPlayResult holds them, elements ascending with 0 among them, full = the playout cap's per-ply flags (None: every ply)."""
    elements = tuple(elements)
    assert elements and elements[0] == 0 and list(elements) == sorted(set(elements))
    reward = 0 if winner == -1 else 1
    out = []
    for i, (b, p) in enumerate(zip(boards, pis)):
        side = i & 1
        if full is not None and not full[i]:
            continue
        z = float(reward if side == winner else -reward)
        st = canonical(b, side)
        for s in ((0,) if i < 2 else elements):
            ts, tp = turn(st, p, s, game)
            out.append((ts, tp, z))
    return out


def count_tuples(plies, n):
    return plies if plies <= 2 else 2 + n * (plies - 2)


def tuple_sha(state, pi, z):
    return hashlib.sha256(np.ascontiguousarray(state, np.float32).tobytes() + np.ascontiguousarray(pi, np.float64).tobytes()
                          + np.float32(z).tobytes()).hexdigest()


def pick_element(draw, elements):
    """azk_replay_gather's pick: valid[((uint32(draw) >> 16) * n_valid) >> 16]."""
    u = int(draw) & 0xFFFFFFFF
    return elements[((u >> 16) * len(elements)) >> 16]


def gather_rows(states, pis, zs, idx, draws, elements, game):
    """The expected outputs of azk_replay_gather (numpy in, numpy out): float32 states, float32 pis (float64 rounded to nearest even,
    numpy's astype), float32 zs; and the element of each row."""
    els = [0 if draws is None else pick_element(draws[b], elements) for b in range(len(idx))]
    so, po = [], []
    for b, r in enumerate(idx):
        st, pi = turn(states[r], pis[r], els[b], game)
        so.append(st)
        po.append(pi.astype(np.float32))
    return np.stack(so), np.stack(po), np.asarray([zs[r] for r in idx], np.float32), els
