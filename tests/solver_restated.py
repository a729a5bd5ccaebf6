"""Exact game-end proofs in the search, restated in plain Python (TEST INFRASTRUCTURE, not product code).

The rule of include/azk.h (azk_set_solver) on forced_playouts_restated's copy of the reference's search (RNode, export,
hash_evaluator, position): every node keeps a status as the player who moved INTO it sees the game - 0 UNKNOWN, 1 WON, 2 LOST, 3 DRAW -
proofs start at terminal leaves and move up the path of the simulation that found them, the walk stops on proven nodes below the root, and
selection shuts out children proven LOST.  With solver=False this is fr.mcts with k = 0 and hence oracle.mcts, bit for bit
(tests/test_solver_restated.py), which is what makes it a yardstick for solver=True.

Also here: the positions, noise rows and restated searches the CPU and GPU tests share (computed once per process).
"""
import functools
import math

import numpy as np

import forced_playouts_restated as fr
from oracle import az_oracle as ao

UNKNOWN, WON, LOST, DRAW = 0, 1, 2, 3
VALUE = {WON: 1, LOST: -1, DRAW: 0}
INF = float("inf")

# the six counters of azk_get_solver_stats, in its order
STATS = ("terminal_marked", "proven_by_won_child", "proven_by_all_children", "stopped_on_proven", "selections_excluding", "roots_proven")


class SNode(fr.RNode):
    """RNode with the status byte (a new node is UNKNOWN)."""
    __slots__ = ("status",)

    def __init__(self, parent, cell, player, move_count, prior=0.0):
        super().__init__(parent, cell, player, move_count, prior)
        self.status = UNKNOWN


def select(node, solver, stats=None):
    """Node.select with the reference's 'network' UCB (fr.select with k = 0), then the solver's rule: a WON child scores +inf, a LOST child
    -inf provided at least one child of the node is not LOST; first maximum wins.  Returns (child index, what the rule did to the winner's
    score: 0 nothing, 1 +inf; and whether any child was shut out)."""
    s = math.sqrt(node.visit)
    some_open = solver and any(c.status != LOST for c in node.children)
    best, best_u, took_won, shut = -1, None, False, False
    for i, c in enumerate(node.children):
        if c.visit == 0:
            u = c.prior * s / (c.visit + 1)
        else:
            u = (c.value / c.visit) + c.prior * s / (c.visit + 1)
        won = solver and c.status == WON
        if won:
            u = INF
        elif solver and c.status == LOST and some_open:
            u, shut = -INF, True
        if best < 0 or u > best_u:
            best, best_u, took_won = i, u, won
    if shut and stats is not None:
        stats["selections_excluding"] += 1
    return best, took_won, shut


def prove_up(trace, stats, events=None, it=None):
    """The proof: trace[-1] has just become proven; examine its parents on the path, from the leaf upwards."""
    for i in range(len(trace) - 2, -1, -1):
        c, p = trace[i + 1], trace[i]
        if p.status != UNKNOWN:
            return
        if c.status == WON:
            p.status = LOST
            stats["proven_by_won_child"] += 1
            kind = "won_child"
        else:
            sts = [ch.status for ch in p.children]                 # list order
            if any(st == UNKNOWN for st in sts):
                return
            assert WON not in sts
            p.status = WON if all(st == LOST for st in sts) else DRAW
            stats["proven_by_all_children"] += 1
            kind = "all_lost" if p.status == WON else "all_draw"
        if p.parent is None:
            stats["roots_proven"] += 1
        if events is not None:
            events.append((it, kind, i, p.status))


def new_stats():
    return {k: 0 for k in STATS}


def mcts(og, root, board, n_iter, evaluator, noise, solver=False, stats=None, events=None, after_sim=None):
    """fr.mcts with k = 0 under the solver's rule.  stats: a new_stats() dict, counted into.  events (a list) receives
    (simulation, kind, trace index, status) of every proof above a leaf, ("stop", depth) of every stop on a proven interior node, and
    ("select", depth, f64 path, took a WON child, shut a child out) of every selection the rule touched.  after_sim(it, root) runs behind
    every simulation."""
    stats = new_stats() if stats is None else stats
    for it in range(n_iter):
        node, trace = root, [root]
        while node.children and (node is root or not solver or node.status == UNKNOWN):
            i, took_won, shut = select(node, solver, stats)
            if events is not None and (took_won or shut):
                events.append((it, "select", len(trace) - 1, node is root and noise is not None, took_won, shut, len(node.children)))
            node = node.children[i]
            trace.append(node)
            og.make_move(board, 1 - node.player, og.rc(node.cell))
        done = None
        if solver and node.parent is not None and node.status != UNKNOWN:
            done = VALUE[node.status]                                 # proven: no check_winner, no move list, no evaluation
            if node.children:
                stats["stopped_on_proven"] += 1
                if events is not None:
                    events.append((it, "stop", len(trace) - 1, node.status))
        elif node.parent is not None:
            if og.check_winner(board, 1 - node.player, og.rc(node.cell)) != -1:
                done = 1
            elif node.move_count == og.state_dim:
                done = 0
            if solver and done is not None:
                node.status = WON if done == 1 else DRAW
                stats["terminal_marked"] += 1
                prove_up(trace, stats, events, it)
        if done is None:
            cells = og.valid_cells(board)
            pri, value = evaluator(og.get_canonical_board(board, node.player))
            pri = np.asarray(pri, np.float32)
            if node.parent is None and noise is not None:
                pri = np.float32(0.75) * pri + 0.25 * np.asarray(noise, np.float64)      # utils.py:24-25: float32 product, float64 sum
            for c in cells:                                                                  # Node.expand (node.py:50-59)
                node.children.append(SNode(node, int(c), 1 - node.player, node.move_count + 1, pri[og.get_action_idx(og.rc(c))]))
            if node.parent is None:
                node.status = UNKNOWN                                                        # the root becomes UNKNOWN when it is expanded
            result = -value
        else:
            result = done
        for nd in trace[::-1]:                                                               # Node.backup (node.py:62-74)
            nd.visit += 1
            nd.value += result
            result *= -1
            if nd.parent is not None:
                og.undo_move(board, nd.player, og.rc(nd.cell))
        if after_sim is not None:
            after_sim(it, root)
    return stats


def export_status(root):
    """The status column in fr.export's row order (DFS pre-order, children in list order), stored view."""
    out, stack = [], [root]
    while stack:
        nd = stack.pop()
        out.append(nd.status)
        stack.extend(reversed(nd.children))
    return np.array(out, np.uint8)


def root_view(status):
    """azk_get_solver_status: the stored root status as the side to move at the root sees it (0 unknown, 1 wins, 2 loses, 3 draw)."""
    return {UNKNOWN: 0, WON: 2, LOST: 1, DRAW: 3}[int(status)]


def check_invariants(root):
    """What include/azk.h states as consequences, on the whole tree."""
    stack = [root]
    while stack:
        nd = stack.pop()
        if nd.children and nd.status == UNKNOWN:
            sts = [c.status for c in nd.children]
            assert WON not in sts, "an UNKNOWN node has a WON child"
            assert UNKNOWN in sts, "an UNKNOWN node has no UNKNOWN child"
        if nd.parent is None and nd.children:
            assert nd.visit == 1 + sum(c.visit for c in nd.children), "N[root] != 1 + sum N[child]"
        stack.extend(nd.children)


# ---- the positions the CPU and GPU tests share ------------------------------------------------------------------------------------------
G = fr.G
SIMS = 64


def searched(og, ev, cells, to_move, mc, noise, n_sims, want_plain=True):
    """One slot: the position, the noise row and the restated searches with and without the solver."""
    out = dict(cells=np.asarray(cells, np.int8), to_move=int(to_move), move_count=int(mc), noise=noise, n_sims=n_sims)
    for key, on in (("solver", True), ("plain", False)):
        if not on and not want_plain:
            continue
        root, events, stats = SNode(None, None, to_move, mc), [], new_stats()
        decided = []

        def after(it, r, decided=decided):
            if r.status != UNKNOWN and not decided:
                decided.append(it)
        mcts(og, root, og.board_from_cells(out["cells"], to_move), n_sims, ev, noise, on, stats, events, after)
        out[key] = dict(tree=fr.export(root), status=export_status(root), stats=stats, events=events, root_status=root_view(root.status),
                        decided_at=decided[0] if decided else None)
    return out


@functools.lru_cache(maxsize=None)
def tictactoe_case(n_sims=SIMS):
    """The eight TicTacToe slots of forced_playouts_restated (its seeds, plies and noise rows)."""
    og = fr.oracle_game("tictactoe")
    ev = fr.hash_evaluator(og)
    slots = []
    for g in range(G):
        seed = fr.slot_seed("tictactoe", g)
        cells, to_move, mc = fr.position(og, seed, fr.PLIES[g])
        noise = np.random.RandomState(seed + 500).dirichlet([fr.NOISE_ALPHA] * og.action_dim)
        slots.append(searched(og, ev, cells, to_move, mc, noise, n_sims))
    return og, slots


def cells_from(rc, first, second):
    """cells int8 [rc]: 1 on the cells of `first` (player 0), 2 on those of `second` (player 1)."""
    cells = np.zeros(rc, np.int8)
    for c in first:
        cells[c] = 1
    for c in second:
        cells[c] = 2
    return cells


def fill_position(og, seed, n_empty):
    """A legal position without a winner that leaves n_empty cells: legal moves drawn by RandomState(seed), a draw that would end the game
    redrawn (at most 64 times a ply, then the whole position again from the next state of the stream)."""
    rng = np.random.RandomState(seed)
    total = og.rows * og.cols
    while True:
        board = og.new_board()
        cells = np.zeros(total, np.int8)
        ok = True
        for ply in range(total - n_empty):
            for _ in range(64):
                valid = og.valid_cells(board)
                c = int(valid[rng.randint(len(valid))])
                og.make_move(board, ply & 1, og.rc(c))
                if og.check_winner(board, ply & 1, og.rc(c)) == -1:
                    break
                og.undo_move(board, 1 - (ply & 1), og.rc(c))
            else:
                ok = False
                break
            cells[c] = 1 + (ply & 1)
        if ok:
            return cells, (total - n_empty) & 1, total - n_empty


# constructed positions for the games on which random shallow positions prove next to nothing: boards a few plies from full, and (Gomoku)
# a four on the board.  name -> (game key of fr.GAMES, slots as (kind, argument))
@functools.lru_cache(maxsize=None)
def constructed_case(name, n_sims=SIMS):
    og = fr.oracle_game(name)
    ev = fr.hash_evaluator(og)
    rc = og.rows * og.cols
    slots = []
    for g in range(G):
        if name == "gomoku7" and g < 4:
            # a four of the side to move (g even) or of the other side (g odd) on row 2 + g // 2, one end blocked
            r = 2 + g // 2
            four = [r * 7 + c for c in (1, 2, 3, 4)]
            other = [r * 7 + 0, 0 * 7 + 6, 5 * 7 + 1, 6 * 7 + 4]
            cells, to_move, mc = (cells_from(rc, four, other), 0, 8) if g % 2 == 0 else (cells_from(rc, other, four), 0, 8)
        else:
            cells, to_move, mc = fill_position(og, 7000 + 10 * sorted(fr.GAMES).index(name) + g, 3 + g % 4)
        noise = np.random.RandomState(8000 + g).dirichlet([fr.NOISE_ALPHA] * og.action_dim)
        slots.append(searched(og, ev, cells, to_move, mc, noise, n_sims))
    return og, slots


WIDE_STONES = fr.WIDE_STONES               # 6, 12, 24 stones -> roots of 56, 92 and 184 children under the added stones: the three forms of the scan
WIDE_FOUR = [(2, 2), (2, 3), (2, 4), (2, 5)]
WIDE_OTHER = [(2, 1), (0, 9), (3, 12), (6, 14)]
WIDE_SIMS = {"noise": 480, "plain": 416}


def wide_position(i, mover_owns, variant=None):
    """fr.wide_cells(6 | 12 | 24) on 15 x 15 plus four stones of one colour on (2,2)..(2,5) and the other colour on (2,1), (0,9), (3,12), (6,14);
    the side to move owns the four (mover_owns) or faces it.  (At 24 stones the other colour holds (0,9), (1,10), (3,12), (4,13) as well: a
    second four, so that both sides have a winning cell there.)  variant "open": the blocking stone on (2,1) stands on (14,0) instead - two
    winning cells.  variant "second": a second four of the same colour on (5,2)..(5,5), the other colour on (14,0), (14,2), (14,4), (14,6)."""
    n = WIDE_STONES[i]
    cells = fr.wide_cells(n)
    to_move = n & 1                                                   # wide_cells alternates 1, 2: an even count leaves player 0 to move
    own, opp = (1 + to_move, 2 - to_move)
    a, b = (own, opp) if mover_owns else (opp, own)
    four, other = list(WIDE_FOUR), list(WIDE_OTHER)
    if variant == "open":
        other[0] = (14, 0)
    elif variant == "second":
        four += [(5, 2), (5, 3), (5, 4), (5, 5)]
        other += [(14, 0), (14, 2), (14, 4), (14, 6)]
    for r, c in four:
        assert cells[r * 15 + c] == 0
        cells[r * 15 + c] = a
    for r, c in other:
        assert cells[r * 15 + c] == 0
        cells[r * 15 + c] = b
    return cells, to_move, n + len(four) + len(other)


# The wide slots, in two groups that each run on one engine: "noise" (a Dirichlet-mixed root: the float64 path at the root) and "plain" (no
# noise: float32 everywhere).  A slot is (width index, the mover owns the four, variant, noise kind) -> what it is there to show:
# (precision path, outcome, scan form); noise kind "win" puts 0.8 of the row on the winning cell (2,6), "dir" is a Dirichlet(0.03) draw.
WIDE_SLOTS = {
    "noise": [((0, True, None, "win"), ("f64", "won", 1)), ((1, True, None, "win"), ("f64", "won", 2)), ((2, True, None, "win"), ("f64", "won", 3)),
              ((0, False, None, "dir"), ("f64", "shut", 1)), ((1, False, None, "dir"), ("f64", "shut", 2)), ((2, True, None, "dir"), ("f64", "shut", 3)),
              ((1, True, None, "dir"), ("f64", "won", 2)), ((0, True, None, "dir"), ("f32", "shut", 1))],
    "plain": [((0, True, "open", None), ("f32", "won", 1)), ((1, True, None, None), ("f32", "won", 2)), ((2, True, "second", None), ("f32", "won", 3)),
              ((0, False, None, None), ("f32", "shut", 1)), ((1, False, None, None), ("f32", "shut", 2)), ((2, True, None, None), ("f32", "shut", 3)),
              ((0, True, None, None), ("f32", "shut", 1)), ((2, False, None, None), ("f32", "shut", 3))],
}


def scan_form(n_children):
    return 1 if n_children <= 64 else 2 if n_children <= 128 else 3


@functools.lru_cache(maxsize=None)
def wide_group(group):
    """(og, slots, n_sims) of one group of WIDE_SLOTS; slot["shows"] = what the slot is there to show."""
    og = ao.OracleGame("gomoku", 15)
    ev = fr.hash_evaluator(og)
    slots = []
    for g, ((i, owns, variant, kind), shows) in enumerate(WIDE_SLOTS[group]):
        cells, to_move, mc = wide_position(i, owns, variant)
        if kind == "win":
            noise = np.full(225, 0.2 / 224)
            noise[2 * 15 + 6] = 0.8
        elif kind == "dir":
            noise = np.random.RandomState(i + 1).dirichlet([0.03] * 225)
        else:
            noise = None
        s = searched(og, ev, cells, to_move, mc, noise, WIDE_SIMS[group], want_plain=False)
        s["shows"] = shows
        slots.append(s)
    return og, slots, WIDE_SIMS[group]


def selection_outcomes(events):
    """{(precision path, "won" | "shut", scan form, at the root)} over a search's selection events."""
    out = set()
    for e in events:
        if e[1] == "select":
            _, _, depth, f64, took_won, shut, nch = e
            if took_won:
                out.add(("f64" if f64 else "f32", "won", scan_form(nch), depth == 0))
            if shut:
                out.add(("f64" if f64 else "f32", "shut", scan_form(nch), depth == 0))
    return out


def minimax_status(og, board, node):
    """Exhaustive minimax of the position behind `node` (the board stands there), as the player who moved INTO the node sees it."""
    def solve(player_to_move, last_player, last_cell, move_count):
        # value for the player who has just moved (last_player)
        if last_cell is not None:
            if og.check_winner(board, last_player, og.rc(last_cell)) != -1:
                return 1
            if move_count == og.state_dim:
                return 0
        best = -2
        for c in og.valid_cells(board):
            c = int(c)
            og.make_move(board, player_to_move, og.rc(c))
            v = solve(1 - player_to_move, player_to_move, c, move_count + 1)
            og.undo_move(board, 1 - player_to_move, og.rc(c))
            best = max(best, v)
            if best == 1:
                break
        return -best
    v = solve(node.player, 1 - node.player, node.cell, node.move_count)
    return {1: WON, -1: LOST, 0: DRAW}[v]
