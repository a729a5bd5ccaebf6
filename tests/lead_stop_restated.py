"""Adaptive search budgets - the lead rule, smart pruning's stop - restated in plain Python (TEST INFRASTRUCTURE, not product code).

The rule of include/azk.h (azk_set_lead_stop) on the arming and the segments of tests/kld_stop_restated.py (imported, not
copied: arm, rate and the case constants are that file's): the search is run on ONE root in segments, by calling forced_playouts_restated.mcts
again on the same root, and judged between them - the lead rule first, then, where a KLD threshold is given as well, the KLD rule.  The lead
rule is integer arithmetic but for one float64 multiply and one compare; the lanes' (max, second) pairs and the xor butterfly are restated as
the device has them.

Also here: the positions, factors and reference results the CPU and GPU tests share (computed once per process).
"""
import functools

import numpy as np

import forced_playouts_restated as fr
import kld_stop_restated as kr

WAVE = kr.WAVE


def merge(a, b):
    """Two (max, second) pairs -> the larger max, and the largest of the smaller max and both seconds."""
    return max(a[0], b[0]), max(min(a[0], b[0]), a[1], b[1])


def lead_pair(n):
    """(N1, N2) of the visits n: lane l folds its children l, l + 64, ... into a pair starting from (0, 0), then the xor butterfly 32 ... 1
    merges the lanes' pairs.  N2 counts multiplicity: a tie for the maximum gives N2 = N1; a single child gives N2 = 0."""
    pair = [(0, 0)] * WAVE
    for i, x in enumerate(n):
        pair[i % WAVE] = merge(pair[i % WAVE], (int(x), 0))
    off = 32
    while off > 0:
        pair = [merge(pair[l], pair[l ^ off]) for l in range(WAVE)]
        off >>= 1
    assert all(p == pair[0] for p in pair)
    return pair[0]


def fires(left, factor, n1, n2):
    return float(left) < factor * float(n1 - n2)


def search(og, root, board, T, evaluator, noise, interval, factor=None, lead_min_sims=0, min_gain=None, min_sims=0):
    """The search of allowance T on `root` (a fresh RNode) under the lead rule (factor), the KLD rule (min_gain) or both.  Returns
    dict(run, ckpt, ended, left, leads, rates, visits): the new simulations run, the checkpoint (1-based) at which the search ended,
    "early" (the lead rule) | "forced" | "kld" | "allowance", the simulations left unrun, (N1, N2, left) of every judged lead checkpoint and
    every judged rate in order, and the root children's visits at every checkpoint."""
    seg, left, run = kr.arm(T, interval)
    fr.mcts(og, root, board, seg, evaluator, noise)
    snap, leads, rates, visits, ckpt = None, [], [], [], 0

    def over(ended):
        return dict(run=run, ckpt=ckpt, ended=ended, left=left, leads=leads, rates=rates, visits=visits)
    while True:
        ckpt += 1
        n = [c.visit for c in root.children]
        visits.append(n)
        if left == 0:
            return over("allowance")
        if factor is not None and run >= lead_min_sims:
            n1, n2 = lead_pair(n)
            leads.append((n1, n2, left))
            if len(n) == 1:
                return over("forced")
            if fires(left, factor, n1, n2):
                return over("early")
        if min_gain is not None:
            if snap is not None and sum(snap) > 0 and run >= min_sims:
                r = kr.rate(snap, n)
                rates.append(r)
                if r < min_gain:
                    return over("kld")
            snap = n
        seg = min(interval, left)
        left -= seg
        run += seg
        fr.mcts(og, root, board, seg, evaluator, noise)


# ---- the cases the CPU and GPU tests share: section 31's ---------------------------------------------------------------------------------
G = kr.G
SMALL, SMALL_T, SMALL_I = kr.SMALL, kr.SMALL_T, kr.SMALL_I
WIDE_T, WIDE_I = kr.WIDE_T, kr.WIDE_I
FACTORS = (1.0, 1.33, 4.0)
NEVER = 1e-9                               # a factor that cannot fire here: f * lead <= 1e-9 * 2^31 < 1 <= left at every judged checkpoint (asserted by the CPU test)
BOTH_FACTOR, BOTH_GAIN = 4.0, 1e-2           # both rules set: each ends searches of every small game (asserted by the CPU test)
HELD_MIN_SIMS = 40                         # the min_sims of the "held back" cases


def searched(og, s, T, interval, factor=None, lead_min_sims=0, min_gain=None, min_sims=0):
    """One slot (a dict of forced_playouts_restated's: cells, to_move, move_count, noise) searched under the rules: search()'s dict plus the
    tree, the root children, the raw pi and the three words of azk_get_lead."""
    root = fr.RNode(None, None, s["to_move"], s["move_count"])
    out = search(og, root, og.board_from_cells(s["cells"], s["to_move"]), T, fr.hash_evaluator(og), s["noise"], interval, factor, lead_min_sims,
                 min_gain, min_sims)
    out["tree"] = fr.export(root)
    out["cells"] = [c.cell for c in root.children]
    out["pi"] = fr.pi_of(og, out["cells"], [c.visit for c in root.children])
    out["lead"] = out["leads"][-1] if out["leads"] else (0, 0, 0)
    return out


@functools.lru_cache(maxsize=None)
def empty_slot():
    """Gomoku 7x7's empty board: ONE legal move (the centre) - the single-child root."""
    og = fr.oracle_game("gomoku7")
    cells, to_move, mc = fr.position(og, 0, 0)
    return dict(cells=cells, to_move=to_move, move_count=mc, noise=np.random.RandomState(77).dirichlet([fr.NOISE_ALPHA] * og.action_dim))


@functools.lru_cache(maxsize=None)
def small_slots(name):
    """forced_playouts_restated.small_case's G positions; "gomoku7+empty": Gomoku 7x7's with slot 0 replaced by the empty board."""
    if name == "gomoku7+empty":
        og, slots = fr.small_case("gomoku7", SMALL_T)
        return og, [empty_slot()] + list(slots[1:])
    return fr.small_case(name, SMALL_T)


@functools.lru_cache(maxsize=None)
def small_results(name, factor, lead_min_sims=0, min_gain=None):
    """G positions of one small game, each searched with T = 64, I = 8."""
    og, slots = small_slots(name)
    return og, slots, [searched(og, s, SMALL_T, SMALL_I, factor, lead_min_sims, min_gain) for s in slots]


# section 31's 192-child root keeps its two most-visited children inside the first 64 under this rule's searches; the same stones under another
# noise row put them into different 64-child trips of the scan (tests/test_lead_stop_restated.py asserts it)
WIDE_NOISE_SEED = {2: 35}


@functools.lru_cache(maxsize=None)
def wide_slot(i):
    """forced_playouts_restated.wide_case(i)'s position - 48 / 96 / 192 root children - and noise row (i = 2: the row of WIDE_NOISE_SEED)."""
    og, s = fr.wide_case(i)
    if i in WIDE_NOISE_SEED:
        s = dict(cells=s["cells"], to_move=s["to_move"], move_count=s["move_count"], noise=np.random.RandomState(WIDE_NOISE_SEED[i]).dirichlet([0.03] * 225))
    return og, s


@functools.lru_cache(maxsize=None)
def wide_results(i, factor, lead_min_sims=0, min_gain=None):
    """wide_slot(i) searched with T = 96, I = 16."""
    og, s = wide_slot(i)
    return og, s, searched(og, s, WIDE_T, WIDE_I, factor, lead_min_sims, min_gain)


@functools.lru_cache(maxsize=None)
def plain_visits(key, i, T):
    """The root children's visits of the plain search of T simulations on small_slots(key)[i] (key a game name) or wide_slot(i) (key "wide")."""
    og, s = wide_slot(i) if key == "wide" else (small_slots(key)[0], small_slots(key)[1][i])
    root = fr.RNode(None, None, s["to_move"], s["move_count"])
    fr.mcts(og, root, og.board_from_cells(s["cells"], s["to_move"]), T, fr.hash_evaluator(og), s["noise"])
    return [c.visit for c in root.children], fr.export(root)


def first_max(visits):
    """The list index of the first most-visited child (Node.max_visit_child)."""
    return max(range(len(visits)), key=lambda i: (visits[i], -i))


def stats_of(results):
    """azk_get_lead_stats over a list of search() results."""
    early = [r for r in results if r["ended"] == "early"]
    return dict(judged=sum(len(r["leads"]) for r in results), ended_early=len(early), sims_unrun=sum(r["left"] for r in early),
                forced=sum(r["ended"] == "forced" for r in results), ran_allowance=sum(r["ended"] == "allowance" for r in results))


def kld_stats_of(results):
    """azk_get_kld_stats over a list of search() results with both rules set."""
    early = [r for r in results if r["ended"] == "kld"]
    return dict(judged=sum(len(r["rates"]) for r in results), ended_early=len(early), sims_unrun=sum(r["left"] for r in early),
                ran_allowance=sum(r["ended"] == "allowance" for r in results))
