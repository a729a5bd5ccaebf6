"""Policy surprise weighting (include/azk.h azk_set_surprise_weighting), restated in plain Python / numpy (TEST
INFRASTRUCTURE, not product code; written independently of selfplay.surprise_copies): the ply coin, the KL of a recorded pi against the
network's raw prior, the copy rule, and the expected tuple list of one finished game - each recorded ply's group, as
emission_restated.emit_tuples gives it, c_i times.  Nothing here reads the engine."""
import math

import emission_restated as er
import rng_restated as rr

COIN_TAG = 0xFFFFFFFC
MIN_PRIOR = 2.0 ** -126                                           # the smallest normal float32: the prior's floor


def coin(seed, gg, move):
    """The ply coin: the uniform of (seed, global game, move key) under Philox word 3 = 0xFFFFFFFC."""
    return float(rr._keyed_u(seed, gg, move, COIN_TAG))


def kl_terms(pi, prior):
    """The terms t_a = p_a * log(p_a / P_a) over the actions with p_a > 0, as Python floats (math.log): pi = the recorded float64 row
    (m_a / sum, the engine's own quotient), prior = the float32 softmax row of the position, floored at the smallest normal float."""
    out = []
    for p, P in zip(pi, prior):
        p = float(p)
        if p > 0.0:
            out.append(p * math.log(p / max(float(P), MIN_PRIOR)))
    return out


def kl(pi, prior):
    """(kl, sum |t_a|, number of terms): kl = max(0, the exactly rounded sum of the terms) - the float64 reference the engine's own sum, in
    whatever order, is held to within (children + 8) * 2^-53 * sum |t_a|."""
    t = kl_terms(pi, prior)
    return max(0.0, math.fsum(t)), math.fsum(abs(x) for x in t), len(t)


def weights(kls, lam, full=None):
    """w_i per ply (0.0 outside the recorded plies F): S = the sequential sum of kl over F in ply order, n_F = |F|,
    w_i = S > 0 ? (1 - lam) + ((lam * n_F) * kl_i) / S : 1."""
    rec = [i for i in range(len(kls)) if full is None or full[i]]
    s = 0.0
    for i in rec:
        s += float(kls[i])
    n = float(len(rec))
    w = [0.0] * len(kls)
    for i in rec:
        w[i] = (1.0 - lam) + ((lam * n) * float(kls[i])) / s if s > 0.0 else 1.0
    return w


def copies(kls, coins, lam, full=None):
    """c_i per ply: floor(w_i) + (coin_i < w_i - floor(w_i)) for the recorded plies, 0 for the others."""
    w = weights(kls, lam, full)
    out = []
    for i, wi in enumerate(w):
        if full is not None and not full[i]:
            out.append(0)
            continue
        f = math.floor(wi)
        out.append(int(f) + (1 if float(coins[i]) < wi - f else 0))
    return out


def game_tuples(game, boards, pis, winner, elements, kls, coins, lam, full=None):
    """-> (tuples in ring order, copies per ply) for one finished game: ply i's group (emission_restated.emit_tuples of that ply alone),
    c_i times, copy after copy."""
    c = copies(kls, coins, lam, full)
    out = []
    for i in range(len(boards)):
        if c[i] == 0:
            continue
        only = [j == i for j in range(len(boards))]
        group = er.emit_tuples(game, boards, pis, winner, elements, full=only)
        assert len(group) == (1 if i < 2 else len(tuple(elements)))
        for _ in range(c[i]):
            out.extend(group)
    return out, c
