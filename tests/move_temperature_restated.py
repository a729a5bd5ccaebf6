"""Move temperature - per-ply schedule, visit offset, value cutoff - restated in plain Python (TEST INFRASTRUCTURE, not product code).

The rule of include/azk.h (azk_set_move_temperature) on azk_root_children-shaped data, in Python floats (IEEE float64, one
rounding per operation, as the engine files are built with contraction off): `choose` is steps 1-6 of the rule.  With the row w[n] = n it is
the oracle's restatement of Node.sample_child (tests/test_move_temperature_restated.py), which is what makes it a yardstick for every other row.

Also here: the table builder's expected values, and the positions, settings and uniforms the CPU and GPU tests share (computed once per process).
"""
import functools
import itertools
import math

import numpy as np

import forced_playouts_restated as fr
from forced_playouts_restated import oracle_game  # noqa: F401  (the tests' one import)


def first_most_visited(visits):
    """Node.max_visit_child (node.py:76-81): the first child with the most visits."""
    best = 0
    for i, n in enumerate(visits):
        if n > visits[best]:
            best = i
    return best


def weights_of(children, row, visit_offset, value_cutoff):
    """Step 3: the weight of every root child in list order, and how many the cutoff cut.  value_cutoff None or negative: no cutoff."""
    visits, values = [int(n) for n in children["visit"]], [float(v) for v in children["value"]]
    b = first_most_visited(visits)
    qb = values[b] / float(visits[b])
    cutoff = -1.0 if value_cutoff is None else float(value_cutoff)
    w, cut = [], 0
    for n, v in zip(visits, values):
        wi = float(row[max(0, n - visit_offset)])
        if cutoff >= 0.0 and wi > 0.0 and v / float(n) < qb - cutoff:
            wi, cut = 0.0, cut + 1
        w.append(wi)
    return w, cut


def cdf_of(children, action_of, w, action_dim):
    """Steps 4 and 6a: the weights by action, their sequential sum S, and (S != 0) the sampler's running sums."""
    by_action = [0.0] * action_dim
    for c, wi in zip(children["cell"], w):
        by_action[action_of(int(c))] = wi
    S = 0.0
    for x in by_action:
        S += x
    if S == 0.0:
        return S, None
    acc, cdf = 0.0, []
    for x in by_action:
        acc += x / S
        cdf.append(acc)
    return S, cdf


def choose(children, action_of, row, visit_offset, value_cutoff, u, action_dim=None):
    """The played cell of one root under one row of the weight table, and the four stats increments [weighted plies, of those not b,
    children cut, fallbacks].  children: dict(cell, visit, value) in list order; action_of(cell) -> action index; row None (the ply's table
    entry is -1) or u None (no uniforms) is the greedy path, which counts nothing."""
    cells, visits = [int(c) for c in children["cell"]], [int(n) for n in children["visit"]]
    b = first_most_visited(visits)
    if row is None or u is None:
        return cells[b], [0, 0, 0, 0]
    A = action_dim if action_dim is not None else 1 + max(action_of(c) for c in cells)
    w, cut = weights_of(children, row, visit_offset, value_cutoff)
    S, cdf = cdf_of(children, action_of, w, A)
    if cdf is None:
        return cells[b], [0, 0, cut, 1]
    last = cdf[-1]
    index = min(int(np.searchsorted(np.array([x / last for x in cdf], np.float64), np.float64(u), side="right")), A - 1)
    i = next(i for i, c in enumerate(cells) if action_of(c) == index)          # the first child with that action
    return cells[i], [1, int(i != b), cut, 0]


# ---- the table builder's expected values ---------------------------------------------------------------------------------------------------
def expected_row(tau, max_sims):
    return [math.pow(float(n), 1.0 / tau) for n in range(max_sims + 1)]


EXACT_ROWS = {0.25: lambda n: float(n ** 4), 0.5: lambda n: float(n * n), 1.0: lambda n: float(n)}     # rows that are integers, exactly


def halflife(p, t0, half, t_final=0.0):
    return t_final + (t0 - t_final) * 0.5 ** (p / half)


def linear(p, t0, decay, t_final=0.0):
    return t0 + (t_final - t0) * (min(float(p), float(decay)) / float(decay))


# ---- the positions, settings and uniforms the CPU and GPU tests share -----------------------------------------------------------------------
G = fr.G
N_SIMS = 24
SMALL = ("tictactoe", "connect4", "gomoku7", "gomoku5x3")
WIDE = ("wide48", "wide96", "wide192")                             # 15 x 15 roots: one, two and three trips of the movers' lane loops
SHORT = ("gomoku7_sims3",)                                        # a search so short that no child has more than 2 visits: visit_offset 2 leaves no weight
CASES = SMALL + WIDE + SHORT
TAUS, OFFSETS, CUTOFFS = (0.25, 1.0, 4.0), (0, 2), (None, 0.1, 0.0)
SETTINGS = tuple(itertools.product(TAUS, OFFSETS, CUTOFFS))


def engine_game(name):
    """(engine game name, size) of a case."""
    return fr.GAMES["gomoku7"] if name in SHORT else fr.GAMES[name] if name in fr.GAMES else ("gomoku", 15)


def sims_of(name):
    """Simulations of a case's search (the engines are all created for N_SIMS: the table has N_SIMS + 1 columns)."""
    return 3 if name in SHORT else N_SIMS


def action_of_game(og):
    return lambda cell: og.get_action_idx(og.rc(cell))


@functools.lru_cache(maxsize=None)
def case(name):
    """(oracle game, G slots) of a case: each slot is dict(cells, to_move, move_count, noise, children) - the position, its noise row and the
    root children (cell / visit / value / prior, list order) of the reference's search of sims_of(name) simulations from it (the restated plain search
    of tests/forced_playouts_restated.py, which test_forced_playouts_restated.py pins to oracle.mcts)."""
    if name in SMALL + SHORT:
        og, slots = fr.small_case("gomoku7" if name in SHORT else name, sims_of(name))
        return og, [dict(cells=s["cells"], to_move=s["to_move"], move_count=s["move_count"], noise=s["noise"], children=s["plain"]["children"])
                    for s in slots]
    og = fr.oracle_game("gomoku15")
    n = fr.WIDE_STONES[WIDE.index(name)]
    ev = fr.hash_evaluator(og)
    slots = []
    for g in range(G):                                             # one position, G noise rows: G different searches
        noise = np.random.RandomState(100 * n + g).dirichlet([0.03] * 225)
        s = fr.searched(og, ev, fr.wide_cells(n), n & 1, n, noise, N_SIMS, k=0.0)
        slots.append(dict(cells=s["cells"], to_move=s["to_move"], move_count=s["move_count"], noise=noise, children=s["plain"]["children"]))
    return og, slots


def uniforms_for(name, g, children, action_of, row, visit_offset, value_cutoff, action_dim):
    """The six uniforms of a slot under a setting: 0, the largest double below 1, two drawn values, and two values equal to an interior
    cdf[k] / cdf[-1] of the slot (side='right': the draw goes to the NEXT action with weight); where the slot has fewer than two interior
    steps - one or two weighted children, or none: the fallback - further drawn values take their place."""
    rng = np.random.RandomState(7000 + 97 * CASES.index(name) + g)
    drawn = [float(x) for x in rng.random_sample(4)]
    out = [0.0, float(np.nextafter(1.0, 0.0)), drawn[0], drawn[1]]
    w, _ = weights_of(children, row, visit_offset, value_cutoff)
    S, cdf = cdf_of(children, action_of, w, action_dim)
    interior = []
    if cdf is not None:
        steps = sorted({x / cdf[-1] for x in cdf if 0.0 < x / cdf[-1] < 1.0})
        interior = [steps[0], steps[len(steps) // 2]] if len(steps) >= 2 else steps
    return out + (interior + drawn[2:])[:2]


@functools.lru_cache(maxsize=None)
def expected(name, setting):
    """Per slot of a case under setting = (tau, visit_offset, value_cutoff): the six uniforms, the cell `choose` plays for each, and the
    stats increments summed over the slots and uniforms."""
    tau, offset, cutoff = setting
    og, slots = case(name)
    a_of, row = action_of_game(og), expected_row(tau, N_SIMS)
    us, cells, stats = [], [], [0, 0, 0, 0]
    for g, s in enumerate(slots):
        u6 = uniforms_for(name, g, s["children"], a_of, row, offset, cutoff, og.action_dim)
        picks = [choose(s["children"], a_of, row, offset, cutoff, u, og.action_dim) for u in u6]
        us.append(u6)
        cells.append([p[0] for p in picks])
        stats = [a + sum(p[1][k] for p in picks) for k, a in enumerate(stats)]
    return us, cells, stats
