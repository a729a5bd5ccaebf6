"""CPU: the float64 restatement of the product RNG (tests/rng_restated.py) is what it claims to be, before test_gpu_rng.py holds the
device generator to it.  Its Philox is the published Philox4x32-10 (Random123's known answers) and the stream the playout-cap coin's
own restatement draws from; its gammas follow Gamma(alpha) by a Kolmogorov-Smirnov statistic against torch.special.gammainc in
float64, a statistic that two planted errors fail; its rows are Dirichlet rows with numpy's E[max]; and no input set of the GPU module
has an accept / reject decision close enough to the line for a last-bit libm difference to flip it."""
import math

import numpy as np
import pytest
import torch

import rng_restated as R
from test_gpu_playout_cap import coin_full
from test_gpu_playout_cap import philox4x32_10 as coin_philox

_shared = {}


def drawn(A, seed, first, G, move, alpha, **plant):
    """gamma_rows computed once per input set for the tests that need it; never modified afterwards."""
    key = (A, seed, first, G, move, alpha, tuple(plant.items()))
    if key not in _shared:
        _shared[key] = R.gamma_rows(A, seed, first, G, move, alpha, **plant)
    return _shared[key]


# ---------------------------------------------------------------------------------------------------
# Philox and the uniforms
# ---------------------------------------------------------------------------------------------------
KNOWN_ANSWERS = [      # Random123 (kat_vectors), philox4x32 with 10 rounds: counter, key, output
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


def test_philox_is_the_published_philox4x32_10():
    for ctr, key, out in KNOWN_ANSWERS:
        assert tuple(int(w) for w in R.philox4x32_10(*ctr, *key)) == out, (ctr, key)
    # vectorised: the three at once, word by word
    cols = [np.array([k[0][i] for k in KNOWN_ANSWERS], np.uint64) for i in range(4)] + [np.array([k[1][i] for k in KNOWN_ANSWERS], np.uint64) for i in range(2)]
    got = R.philox4x32_10(*cols)
    assert [tuple(int(w[j]) for w in got) for j in range(3)] == [k[2] for k in KNOWN_ANSWERS]


def test_coin_and_uniform_are_the_stream_of_the_playout_cap_restatement():
    """A few hundred keys, the seed's and the game index's high words live: coin() is the uniform test_gpu_playout_cap.py's scalar Philox
    gives for word 3 = 0xFFFFFFFE, and its coin_full flips exactly at that uniform; move_uniform() is the same with 0xFFFFFFFF."""
    keys = [(seed, gg, mv) for seed in R.SEEDS + (1, 3) for gg in (0, 1, 5, 100, 2 ** 32 - 1, 2 ** 32, 2 ** 40 - 1) for mv in (0, 1, 2, 7, 29, 511, 2 ** 31 - 1)]
    assert len(keys) >= 250
    for seed, gg, mv in keys:
        u, um = float(R.coin(seed, gg, mv)), float(R.move_uniform(seed, gg, mv))
        for word3, got in ((0xFFFFFFFE, u), (0xFFFFFFFF, um)):
            c = coin_philox([gg & 0xFFFFFFFF, gg >> 32, mv, word3], seed & 0xFFFFFFFF, seed >> 32)
            assert got == float(((c[0] << 32) | c[1]) >> 11) * 2.0 ** -53 and 0.0 <= got < 1.0, (seed, gg, mv, word3)
        assert u != um
        assert not coin_full(seed, gg, mv, u) and coin_full(seed, gg, mv, math.nextafter(u, 1.0)), (seed, gg, mv)
        for p in (0.0, 0.25, 0.5, 1.0):
            assert coin_full(seed, gg, mv, p) == (u < p), (seed, gg, mv, p)
    # vectorised over games = one game at a time
    ggs = np.array([0, 100, 2 ** 32 - 2, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1], np.uint64)
    for fn in (R.coin, R.move_uniform):
        assert fn(R.LAW_SEED, ggs, 3).tolist() == [float(fn(R.LAW_SEED, int(g), 3)) for g in ggs]


# ---------------------------------------------------------------------------------------------------
# the law of the gammas
# ---------------------------------------------------------------------------------------------------
LAW_CASES = [(0.03, 225), (0.3, 49), (1.0, 7)]
KS_COLUMNS = 7
KS_N = R.LAW_G * KS_COLUMNS
KS_BAR = 1.628 / math.sqrt(KS_N)                     # the 1 % critical value of the Kolmogorov-Smirnov statistic: 0.00961


def ks_against_gamma(x, alpha):
    """sup |empirical CDF - P(alpha, x)| of the sample x, P the regularised lower incomplete gamma function in float64."""
    x = np.sort(np.asarray(x, np.float64).ravel())
    n = x.size
    F = torch.special.gammainc(torch.full((n,), float(alpha), dtype=torch.float64), torch.from_numpy(x)).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - F).max(), (F - (i - 1.0) / n).max()))


def law_draw(alpha, A, **plant):
    return drawn(A, R.LAW_SEED, R.LAW_FIRST, R.LAW_G, R.LAW_MOVE, alpha, **plant)


def test_an_entry_does_not_depend_on_the_row_length():
    """Entry a's stream is keyed by (game, a) alone, so the first columns of a long row are a short row's: the planted-error runs below
    may draw 7 columns instead of 225."""
    for alpha, A in LAW_CASES:
        assert np.array_equal(law_draw(alpha, A).gam[:, :KS_COLUMNS], law_draw(alpha, KS_COLUMNS).gam)


@pytest.mark.parametrize("alpha,A", LAW_CASES)
def test_the_restatement_draws_gamma_alpha(alpha, A):
    """Columns 0..6 of 4096 rows pooled (independent before normalisation), N = 28 672, against the 1 % critical value.  The inputs are
    fixed: D = 0.00597, 0.00614, 0.00430 for alpha = 0.03, 0.3, 1.0."""
    r = law_draw(alpha, A)
    assert r.gam.shape == (R.LAW_G, A) and (r.gam > 0).all()
    d = ks_against_gamma(r.gam[:, :KS_COLUMNS], alpha)
    print(f"alpha {alpha} A {A}: D = {d:.5f} (bar {KS_BAR:.5f})")
    assert d < KS_BAR, (alpha, A, d)


@pytest.mark.parametrize("alpha,A", LAW_CASES)
@pytest.mark.parametrize("plant", ["exponent", "d"])
def test_the_statistic_notices_a_planted_error(plant, alpha, A):
    """The same statistic on a deliberately wrong recipe - U^(1 / (1.05 alpha)), or d = alpha + 1 - exceeds the bar (D = 0.0203, 0.0181,
    0.0151 and 0.0167, 0.0556, 0.0686): the bar above is not one that anything passes."""
    d = ks_against_gamma(law_draw(alpha, KS_COLUMNS, _plant=plant).gam, alpha)
    print(f"{plant}, alpha {alpha}: D = {d:.5f} (bar {KS_BAR:.5f})")
    assert d > KS_BAR, (plant, alpha, d)


# ---------------------------------------------------------------------------------------------------
# normalised rows
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alpha,A", LAW_CASES)
def test_rows_are_normalised_and_accepted_early(alpha, A):
    r = law_draw(alpha, A)
    assert np.abs(r.rows.sum(axis=1) - 1.0).max() <= 1e-12
    assert (r.rows >= 0).all() and np.array_equal(r.rows, r.gam / r.gam.sum(axis=1, keepdims=True))
    assert r.tries.min() >= 1 and r.tries.max() <= 8, int(r.tries.max())         # (Marsaglia-Tsang accepts ~ 95 % of the tries)


def test_expected_maximum_is_numpys_dirichlet_figure():
    """numpy's Dirichlet([0.03] * 225) has E[max] = 0.255 (tests/test_gpu_engine.py quotes it); 4096 rows: 0.2547."""
    e_max = float(law_draw(0.03, 225).rows.max(axis=1).mean())
    print(f"E[max] = {e_max:.4f}")
    assert abs(e_max - 0.255) <= 0.01, e_max


def test_a_row_that_sums_to_zero_is_uniform():
    """The restatement's fallback, reached only when every gamma of a row underflows: alpha = 1e-4 gives U^10000, 0 in float64 for
    almost every draw."""
    r = R.gamma_rows(9, 1, 0, 64, 0, 1e-4)
    dead = r.gam.sum(axis=1) == 0.0
    assert dead.any() and (r.rows[dead] == 1.0 / 9).all() and np.abs(r.rows.sum(axis=1) - 1.0).max() <= 1e-12


# ---------------------------------------------------------------------------------------------------
# the GPU module's inputs are unambiguous
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sets", ["shapes", "edges", "law"])
def test_no_gpu_input_set_has_a_borderline_decision(sets):
    """Over every try of every entry of every input set of test_gpu_rng.py the accept / reject decisions keep |t| and |log(u3) - rhs| above
    1e-9 (seen: 2.3e-6 and more) - eight orders above what a last-bit difference of log / cos / sqrt can move them by - so host and
    device take the same tries and the entry-by-entry bound of the GPU module may be tight."""
    cases = dict(shapes=R.SHAPE_SETS, edges=R.EDGE_SETS, law=[R.LAW_SET])[sets]
    worst = math.inf
    for game, size, A, G, seed, first, move, alpha in cases:
        r = drawn(A, seed, first, G, move, alpha)
        worst = min(worst, float(r.margin.min()))
        assert r.margin.min() > 1e-9, (game, size, seed, first, move, alpha, float(r.margin.min()))
        assert r.tries.max() <= 8 and (r.gam > 1e-290).all()          # ... and the bound's absolute term is never what passes an entry
    print(f"{sets}: smallest margin {worst:.2e}")
