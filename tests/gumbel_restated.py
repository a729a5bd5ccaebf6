"""Gumbel root search, restated in plain Python (TEST INFRASTRUCTURE, not product code).

The rule of include/azk.h (azk_set_gumbel_root) on the plain-Python copy of the reference's search that
tests/forced_playouts_restated.py keeps (its node, export, position and interior-PUCT helpers are imported, not edited): the evaluator returns the
fixture's "hash" LOGITS and value, the root's children are scored gl = logit + Gumbel draw and are eligible by the sequential-halving table,
interior nodes keep the reference's PUCT.  With the root rule switched to the reference's (gumbel=None) it is the reference's search and reproduces
oracle.mcts trees bit for bit (tests/test_gumbel_restated.py), which is what makes it a yardstick.

Also here: schedule(), the move rule and the float64 target, the Gumbel-row chain in numpy float64, and the positions, rows and reference
results the CPU and GPU tests share (computed once per process).
"""
import functools
import math

import numpy as np
import torch

import forced_playouts_restated as fr
from fixture_eval import fixture_logits_value
from oracle import az_oracle as ao
from rng_restated import M32, _split, _u64, philox4x32_10

INF = float("inf")


class GNode(fr.RNode):
    """fr.RNode + what a Gumbel root keeps: the child's raw float32 logit and float32 prior (`prior` holds gl for a root child), the root's v0."""
    __slots__ = ("logit", "p32", "v0")

    def __init__(self, parent, cell, player, move_count, prior=0.0, logit=None, p32=None):
        super().__init__(parent, cell, player, move_count, prior)
        self.logit, self.p32, self.v0 = logit, p32, None


def logits_evaluator(og, fn=None):
    """evaluator(canonical board) -> (float32 logits [A], float32 value) of the fixture's "hash" network, or of fn (boards [n, F, R, C] torch ->
    (logits [n, A], values [n]))."""
    A = og.action_dim
    fn = fn or (lambda x: fixture_logits_value(x, A, "hash"))

    def ev(canon):
        logits, v = fn(torch.from_numpy(np.ascontiguousarray(canon))[None])
        return logits[0].numpy().astype(np.float32), np.float32(v.reshape(-1)[0].item())
    return ev


def schedule(m, n):
    """The visit count a root child must have to be eligible at each of n root selections, m sampled children."""
    if m <= 1:
        return list(range(n))
    L = int(math.ceil(math.log2(m)))
    v, c, out = [0] * m, m, []
    while len(out) < n:
        extra = max(1, n // (L * c))
        for _ in range(extra):
            out.extend(v[:c])
            for i in range(c):
                v[i] += 1
        c = max(2, c // 2)
    return out[:n]


def phases(m, n):
    """[(first selection, count of selections, width c)] of schedule(m, n)'s halving phases that begin before n (m >= 2)."""
    L = int(math.ceil(math.log2(m)))
    c, t, out = m, 0, []
    while t < n:
        extra = max(1, n // (L * c))
        out.append((t, min(extra * c, n - t), c))
        t += extra * c
        c = max(2, c // 2)
    return out


def root_select(root, m, n, c_visit, c_scale):
    """The root rule: index of the first maximum among the eligible children (index 0 if none were eligible - the table never lets that happen)."""
    t = root.visit - 1
    cv = schedule(min(m, len(root.children)), n)[min(t, n - 1)]
    sig = (c_visit + float(cv)) * c_scale
    best, best_u = -1, None
    for i, c in enumerate(root.children):
        if c.visit == cv:
            u = c.prior + sig * (c.value / float(c.visit)) if c.visit != 0 else c.prior
        else:
            u = -INF
        if best < 0 or u > best_u:
            best, best_u = i, u
    return best, best_u


def mcts(og, root, board, n_iter, evaluator, row, gumbel=None, log=None):
    """MCTS.mcts(model, board, root, Game, n_iter) without the eval cache.  gumbel = (m, c_visit, c_scale): `row` is the game's Gumbel row and
    the root rule is the option's, for a search of n_iter simulations; gumbel = None: `row` is a Dirichlet row (or None) and the root rule is
    the reference's.  log (a list) receives (simulation, root child index, eligible count) of every Gumbel root selection."""
    n = n_iter - 1
    for it in range(n_iter):
        node, trace = root, [root]
        while node.children:
            if node is root and gumbel is not None:
                i, u = root_select(root, gumbel[0], n, gumbel[1], gumbel[2])
                if log is not None:
                    cv = schedule(min(gumbel[0], len(root.children)), n)[min(root.visit - 1, n - 1)]
                    log.append((it, i, sum(1 for c in root.children if c.visit == cv)))
            else:
                i, _ = fr.select(node, 0.0, False)
            node = node.children[i]
            trace.append(node)
            og.make_move(board, 1 - node.player, og.rc(node.cell))
        done = None
        if node.parent is not None:
            if og.check_winner(board, 1 - node.player, og.rc(node.cell)) != -1:
                done = 1
            elif node.move_count == og.state_dim:
                done = 0
        if done is None:
            cells = og.valid_cells(board)
            logits, value = evaluator(og.get_canonical_board(board, node.player))
            pri = np.asarray(ao.softmax_det(logits), np.float32)
            at_root = node.parent is None
            if at_root and gumbel is None and row is not None:
                mixed = np.float32(0.75) * pri + 0.25 * np.asarray(row, np.float64)         # utils.py:24-25: float32 product, float64 sum
            for c in cells:                                                                  # Node.expand (node.py:50-59)
                a = og.get_action_idx(og.rc(c))
                if at_root and gumbel is not None:
                    gl = float(np.float64(logits[a])) + float(row[a])
                    node.children.append(GNode(node, int(c), 1 - node.player, node.move_count + 1, gl, logits[a], pri[a]))
                elif at_root and row is not None:
                    node.children.append(GNode(node, int(c), 1 - node.player, node.move_count + 1, mixed[a], logits[a], pri[a]))
                else:
                    node.children.append(GNode(node, int(c), 1 - node.player, node.move_count + 1, pri[a], logits[a], pri[a]))
            if at_root:
                node.v0 = float(value)
            result = -float(value)
        else:
            result = done
        for nd in trace[::-1]:                                                               # Node.backup (node.py:62-74)
            nd.visit += 1
            nd.value += result
            result *= -1
            if nd.parent is not None:
                og.undo_move(board, nd.player, og.rc(nd.cell))


def move_and_target(og, cells, visits, values, gl, logit, p32, v0, c_visit, c_scale):
    """The move (child index) and the recorded pi [A] from the root's children in list order; float64 throughout.
    Also returns (sigf, n children) for the tests' bound."""
    n = len(cells)
    S = sum(int(v) for v in visits)
    q = [float(values[i]) / float(visits[i]) if visits[i] > 0 else None for i in range(n)]
    pv = pq = 0.0
    for i in range(n):
        if visits[i] > 0:
            P = float(np.float64(np.float32(p32[i])))
            pv += P
            pq += P * q[i]
    v0 = float(v0)
    vmix = (v0 + float(S) * (pq / pv)) / (1.0 + float(S)) if S > 0 else v0
    qh = [q[i] if visits[i] > 0 else vmix for i in range(n)]
    maxn = max(int(v) for v in visits)
    sigf = (c_visit + float(maxn)) * c_scale
    best, best_s = -1, None
    for i in range(n):
        if visits[i] == maxn:
            s = float(gl[i]) + sigf * qh[i]
            if best < 0 or s > best_s:
                best, best_s = i, s
    y = [float(np.float64(np.float32(logit[i]))) + sigf * qh[i] for i in range(n)]
    ymax = max(y)
    ex = [math.exp(v - ymax) for v in y]
    tot = math.fsum(ex)
    pi = np.zeros(og.action_dim)
    for i in range(n):
        pi[og.get_action_idx(og.rc(int(cells[i])))] = ex[i] / tot
    return best, pi, sigf


def target_bound(sigf, n):
    """Relative error allowed on an entry of the recorded pi (derived, not taken from the kernel): |dy| <= sigf * (n + 8) * 2^-53 from the
    float64 sums behind qh, an entry's relative error <= 2 |dy| + 4 (n + 4) * 2^-52 (exp within 2 ulp on either side, the n-term sum)."""
    dy = abs(sigf) * (n + 8) * 2.0 ** -53
    return 2.0 * dy + 4.0 * (n + 4) * 2.0 ** -52


# ---- the Gumbel rows ---------------------------------------------------------------------------------------------------------------------
def gumbel_uniforms(A, seed, first_game, G, move):
    """[G][A] float64: u = (((c0 << 32 | c1) >> 12) + 0.5) * 2^-52 of the Philox block at {gg lo, gg hi ^ (a << 8), move, 0xFFFFFFFB}."""
    k0, k1, g0, g1 = _split(seed, np.arange(G, dtype=np.uint64) + np.uint64(int(first_game)))
    g0, g1 = np.repeat(g0, A), np.repeat(g1, A) ^ np.tile(np.arange(A, dtype=np.uint64) << np.uint64(8), G)
    w = philox4x32_10(g0, g1, _u64(move), np.uint64(0xFFFFFFFB), k0, k1)
    x = (((w[0] & M32) << np.uint64(32)) | (w[1] & M32)) >> np.uint64(12)
    return ((x.astype(np.float64) + 0.5) * 2.0 ** -52).reshape(G, A)


def gumbel_rows(A, seed, first_game, G, move):
    return -np.log(-np.log(gumbel_uniforms(A, seed, first_game, G, move)))


# ---- the positions the CPU and GPU tests share ------------------------------------------------------------------------------------------
G = fr.G
GAMES = fr.GAMES
PLIES = fr.PLIES
CASES = ((17, 4), (64, 16))                # (n_sims, m); TicTacToe (at most 8 children here) and Connect4 (7) make m > nch at m = 16
C_VISIT, C_SCALE = 50.0, 1.0
ROW_SEED = 77

# slots whose first seed gives a search on which the option shows too little (tests/test_gumbel_restated.py asserts the preconditions): a later seed
SEED_BUMP = {}


def slot_seed(name, g):
    return 3000 * (1 + sorted(GAMES).index(name)) + g + SEED_BUMP.get((name, g), 0)


def children_of(root):
    ch = root.children
    return dict(cell=[c.cell for c in ch], visit=[c.visit for c in ch], value=[c.value for c in ch], prior=[c.prior for c in ch],
                logit=[c.logit for c in ch], p32=[c.p32 for c in ch])


def searched(og, ev, cells, to_move, mc, row, n_sims, m, c_visit=C_VISIT, c_scale=C_SCALE):
    root, log = GNode(None, None, to_move, mc), []
    mcts(og, root, og.board_from_cells(cells, to_move), n_sims, ev, row, (m, c_visit, c_scale), log)
    ch = children_of(root)
    best, pi, sigf = move_and_target(og, ch["cell"], ch["visit"], ch["value"], ch["prior"], ch["logit"], ch["p32"], root.v0, c_visit, c_scale)
    return dict(cells=cells, to_move=to_move, move_count=mc, row=np.asarray(row, np.float64), tree=fr.export(root), log=log, children=ch,
                root_visit=root.visit, v0=root.v0, move=int(ch["cell"][best]), move_index=best, target=pi, sigf=sigf)


@functools.lru_cache(maxsize=None)
def small_case(name, n_sims, m):
    """G slots of one small game: positions (those of the forced-playouts tests' geometry, other seeds), Gumbel rows and the restated searches."""
    og = fr.oracle_game(name)
    ev = logits_evaluator(og)
    slots = []
    for g in range(G):
        cells, to_move, mc = fr.position(og, slot_seed(name, g), PLIES[g])
        row = gumbel_rows(og.action_dim, ROW_SEED, slot_seed(name, g), 1, mc)[0]
        slots.append(searched(og, ev, cells, to_move, mc, row, n_sims, m))
    return og, slots


WIDE_STONES = fr.WIDE_STONES               # 48, 96, 192 root children: the three forms of the root scan
WIDE_SIMS, WIDE_M = 96, 16


def wide_row(i, nch_cells):
    """A Gumbel row that puts the top m on HIGH list indices: the row's own draws, plus 40 on the last WIDE_M / 2 children and on WIDE_M / 2
    children just below the list's middle (so that the wider roots select at indices >= 64 and >= 128 as well as below)."""
    row = gumbel_rows(225, ROW_SEED, 9000 + i, 1, 0)[0].copy()
    n = len(nch_cells)
    for j in list(range(n - WIDE_M // 2, n)) + list(range(n // 2 - WIDE_M // 2, n // 2)):
        row[int(nch_cells[j])] += 40.0
    return row


@functools.lru_cache(maxsize=None)
def wide_case(i):
    og = ao.OracleGame("gomoku", 15)
    n = WIDE_STONES[i]
    cells = fr.wide_cells(n)
    valid = og.valid_cells(og.board_from_cells(cells, n & 1))
    return og, searched(og, logits_evaluator(og), cells, n & 1, n, wide_row(i, valid), WIDE_SIMS, WIDE_M)
