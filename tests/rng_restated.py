"""The product RNG (noise_uniform / cap_coin / noise_row in csrc/azk_rng.h, k_gen_noise in csrc/azk_noise.hip), restated in float64 numpy from the
counter layouts include/azk.h documents (azk_gen_noise, azk_set_playout_cap) and the kernel's comments.  Test infrastructure: no GPU,
no libazk; everything is vectorised over games (and actions).

The chain: Philox4x32-10 -> 53-bit uniforms -> Box-Muller normal -> Marsaglia-Tsang Gamma(alpha + 1) -> times U^(1/alpha), which is
Gamma(alpha) -> row / row sum, which is Dirichlet(alpha).  Key = (seed lo, seed hi) for every draw; the counters are

    move uniform    {gg lo, gg hi,            move, 0xFFFFFFFF}            u = ((w0 << 32 | w1) >> 11) * 2^-53         in [0, 1)
    playout coin    {gg lo, gg hi,            move, 0xFFFFFFFE}            the same
    row entry a     {gg lo, gg hi ^ (a << 8), move, it} and it | 0x40000000, it = 0..63 the try
                                                                           u = (((hi << 32 | lo) >> 11) + 0.5) * 2^-53 in (0, 1)

What the layout implies: an engine has at most 400 actions, so the action index sits in bits 8..16 of word 1 and the global game
index's high word in bits 0..7 as long as the index is below 2^40 - below that bound the streams of distinct (game, action) pairs are
distinct (they differ in word 0 or word 1), and word 3 keeps the move uniform and the coin apart from every row's draws (a row has
it < 64 and it | 0x40000000).  From 2^40 on, game g and action a can meet game g ^ (a' << 40), action a ^ a'.
"""
from collections import namedtuple

import numpy as np

M32 = np.uint64(0xFFFFFFFF)
_S32, _S11 = np.uint64(32), np.uint64(11)
TWO_M53 = 2.0 ** -53
MAX_TRIES = 64

GammaRows = namedtuple("GammaRows", "rows gam tries margin")


def _u64(x):
    """Python ints (any size below 2^64) or arrays -> uint64 array."""
    if isinstance(x, np.ndarray):
        return x.astype(np.uint64)
    return np.asarray(x, dtype=np.uint64)


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (Salmon et al., SC'11; Random123).  Words are uint64 arrays (or ints) holding 32-bit values; broadcast together."""
    c0, c1, c2, c3, k0, k1 = (_u64(w) & M32 for w in (c0, c1, c2, c3, k0, k1))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                                       # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & M32, (p0 >> _S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return c0, c1, c2, c3


def _split(seed, gg):
    """(seed lo, seed hi, gg lo, gg hi); seed and gg are Python ints below 2^64 or uint64 arrays."""
    seed, gg = _u64(seed), _u64(gg)
    return seed & M32, seed >> _S32, gg & M32, gg >> _S32


def _keyed_u(seed, gg, move, word3):
    k0, k1, g0, g1 = _split(seed, gg)
    w0, w1, _, _ = philox4x32_10(g0, g1, _u64(move), np.uint64(word3), k0, k1)
    return (((w0 << _S32) | w1) >> _S11).astype(np.float64) * TWO_M53


def move_uniform(seed, gg, move):
    """The uniform np.random.choice would consume for (seed, global game, move); in [0, 1)."""
    return _keyed_u(seed, gg, move, 0xFFFFFFFF)


def coin(seed, gg, move):
    """The playout-cap coin's uniform for (seed, global game, move key): the search is full iff coin < p_full."""
    return _keyed_u(seed, gg, move, 0xFFFFFFFE)


def _u53(hi, lo):
    return ((((hi << _S32) | lo) >> _S11).astype(np.float64) + 0.5) * TWO_M53


def gamma_rows(A, seed, first_game, G, move, alpha, *, _plant=None):
    """Dirichlet(alpha) rows of games first_game .. first_game + G - 1 at one move.  Returns GammaRows:
        rows   [G][A] the normalised rows (1 / A everywhere where a row's gammas sum to 0)
        gam    [G][A] the Gamma(alpha) draws before normalisation (0: never accepted in 64 tries)
        tries  [G][A] tries used (65: never accepted)
        margin [G][A] the smallest of |t| and |log(u3) - rhs| over the entry's tries: how far its accept / reject decisions were from
                      going the other way
    _plant is for the tests of this module alone: a deliberately wrong recipe ("exponent": 1 / (1.05 alpha); "d": d = alpha + 1)."""
    assert 1 <= A <= 400 and _plant in (None, "exponent", "d")
    alpha = float(alpha)
    k0, k1, g0, g1 = _split(seed, np.arange(G, dtype=np.uint64) + np.uint64(int(first_game)))
    n = G * A
    g0, g1 = np.repeat(g0, A), np.repeat(g1, A) ^ np.tile(np.arange(A, dtype=np.uint64) << np.uint64(8), G)
    mv = _u64(move)
    d = alpha + 1.0 if _plant == "d" else alpha + 1.0 - 1.0 / 3.0
    cc = 1.0 / np.sqrt(9.0 * d)
    inv_alpha = 1.0 / (1.05 * alpha) if _plant == "exponent" else 1.0 / alpha
    gam, tries, margin = np.zeros(n), np.full(n, MAX_TRIES + 1, np.int64), np.full(n, np.inf)
    live = np.arange(n)
    for it in range(MAX_TRIES):
        if live.size == 0:
            break
        a0, a1 = g0[live], g1[live]
        w = philox4x32_10(a0, a1, mv, np.uint64(it), k0, k1)
        w2 = philox4x32_10(a0, a1, mv, np.uint64(it | 0x40000000), k0, k1)
        u1, u2, u3, u4 = _u53(w[0], w[1]), _u53(w[2], w[3]), _u53(w2[0], w2[1]), _u53(w2[2], w2[3])
        x = np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)
        t = 1.0 + cc * x
        pos = t > 0.0
        v = np.where(pos, t * t * t, 1.0)
        lhs, rhs = np.log(u3), 0.5 * x * x + d - d * v + d * np.log(v)
        acc = pos & (lhs < rhs)
        margin[live] = np.minimum(margin[live], np.where(pos, np.minimum(np.abs(t), np.abs(lhs - rhs)), np.abs(t)))
        hit = live[acc]
        gam[hit] = d * v[acc] * np.power(u4[acc], inv_alpha)
        tries[hit] = it + 1
        live = live[~acc]
    gam, tries, margin = gam.reshape(G, A), tries.reshape(G, A), margin.reshape(G, A)
    tot = gam.sum(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        rows = np.where(tot > 0.0, gam / tot, 1.0 / A)
    return GammaRows(rows, gam, tries, margin)


# ---------------------------------------------------------------------------------------------------------------------------------
# the input sets of tests/test_gpu_rng.py (test_rng_restated.py shows on the CPU that none of them has a borderline accept / reject)
# ---------------------------------------------------------------------------------------------------------------------------------
SEEDS = (0, 7, 0x0123456789ABCDEF, 2 ** 64 - 1)                # the high key word is live in the last two
FIRST_GAMES = (0, 100, 2 ** 32 - 2)                            # the last: consecutive games straddle the 32-bit boundary (counter word 1 live)
MOVES = (0, 1, 511)
ALPHAS = (0.03, 0.3, 1.0)
GAMES = (("tictactoe", None, 9), ("connect4", None, 7), ("gomoku", 7, 49), ("gomoku", 8, 64), ("gomoku", 15, 225), ("gomoku", 20, 400))
LAW_SEED, LAW_FIRST, LAW_MOVE, LAW_G = 0x0123456789ABCDEF, 0, 3, 4096      # the inputs of the Kolmogorov-Smirnov tests
ROW_G = 64

# (game, size, A, G, seed, first game, move, alpha)
SHAPE_SETS = [(g, s, A, ROW_G, LAW_SEED, 100, 1, al) for g, s, A in GAMES for al in ALPHAS]
EDGE_SETS = [("gomoku", 7, 49, ROW_G, seed, first, mv, 0.3) for seed in SEEDS for first in FIRST_GAMES for mv in MOVES]
LAW_SET = ("gomoku", 15, 225, LAW_G, LAW_SEED, LAW_FIRST, LAW_MOVE, 0.03)
