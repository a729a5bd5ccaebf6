"""CPU: the restatement of root noise on the legal moves (tests/root_noise_restated.py) is what it claims to be, before test_gpu_root_noise.py
holds the device rows to it.  Its legal sets are the rules' get_valid_moves as sets (the oracle's primitives); mode "legal" is today's restated
row restricted and renormalised; one legal move gives exactly 1.0, illegal entries are +0.0, a row whose gammas all underflow is uniform over
the legal moves; the rows follow the Dirichlet law over n entries by their first two moments, which the recipe the option replaces fails; no
input set of the GPU module has an accept / reject decision near the line; and selfplay.check_root_noise refuses what it must."""
import math

import numpy as np
import pytest

import rng_restated as R
import root_noise_restated as N


# ---------------------------------------------------------------------------------------------------
# legal sets
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", N.GEOMETRIES, ids=str)
def test_legal_sets_are_the_rules_valid_moves(geom):
    from oracle import az_oracle as ao
    og = ao.OracleGame(*geom)
    for name, cells, n in N.POSITIONS[geom]:
        got = N.legal_actions(geom[0], geom[1], cells)
        board = og.board_from_cells(cells, int((cells != 0).sum()) & 1)
        want = {og.get_action_idx(og.rc(c)) for c in og.valid_cells(board)}
        assert set(got) == want and got == sorted(want) and len(got) == n >= 1, (geom, name, len(got))


def test_positions_cover_the_shapes_the_kernel_branches_on():
    """One legal move, fewer than 64, more than 64 and more than 128 (a second and a third pass of the lanes), stones in both dword halves of
    the 20 x 20 board and on its last row and column."""
    counts = {n for pos in N.POSITIONS.values() for _, _, n in pos}
    assert 1 in counts and any(64 < n <= 128 for n in counts) and any(n > 128 for n in counts)
    both = N.POSITIONS[("gomoku", 20)][0][1]
    assert both[:256].any() and both[256:].any() and both.reshape(20, 20)[19].any() and both.reshape(20, 20)[:, 19].any()


# ---------------------------------------------------------------------------------------------------
# the row's definition
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", N.GEOMETRIES, ids=str)
def test_mode_legal_is_todays_row_restricted_and_renormalised(geom):
    game, size = geom
    cells = N.cells_of(geom)
    A = N.geometry(game, size)[2]
    for alpha, first, key in ((0.03, 0, 0), (0.3, 2 ** 32 - 2, 511)):
        today = R.gamma_rows(A, N.SEED, first, N.ROW_G, key, alpha)
        got = N.noise_rows(game, size, cells, N.SEED, first, key, "legal", alpha)
        for g in range(N.ROW_G):
            L = got.legal[g]
            want = np.zeros(A)
            want[L] = today.rows[g, L] / today.rows[g, L].sum()
            assert np.allclose(got.rows[g], want, rtol=1e-14, atol=0.0), (geom, g)
            assert np.array_equal(got.gam[g, L], today.gam[g, L])             # ... from the same Philox blocks
            assert abs(got.rows[g].sum() - 1.0) <= 1e-12


@pytest.mark.parametrize("mode,alpha", [(m, a) for m in N.MODES for a in N.ALPHAS])
def test_one_legal_move_is_exactly_one_and_illegal_entries_are_plus_zero(mode, alpha):
    for geom in N.GEOMETRIES:
        game, size = geom
        got = N.noise_rows(game, size, N.cells_of(geom), N.SEED, 0, 1, mode, alpha)
        for g in range(N.ROW_G):
            L = got.legal[g]
            off = np.setdiff1d(np.arange(got.rows.shape[1]), L)
            assert (got.rows[g, off] == 0.0).all() and not np.signbit(got.rows[g, off]).any()
            if len(L) == 1:
                assert got.rows[g, L[0]] == 1.0, (geom, g)


def test_total_mode_divides_alpha_by_the_legal_count():
    geom = ("gomoku", 7)
    cells = N.cells_of(geom)
    got = N.noise_rows(*geom, cells, N.SEED, 0, 1, "total", 10.83)
    for g in range(N.ROW_G):
        n = len(got.legal[g])
        same = N.noise_rows(*geom, cells, N.SEED, 0, 1, "legal", 10.83 / n)
        assert np.array_equal(got.rows[g], same.rows[g]), g


FALLBACK = ("legal", 1e-5, 0, 0)                                  # (mode, alpha, first game, key): U^(100 000) is 0 in float64 for almost every draw


def test_a_row_whose_gammas_all_underflow_is_uniform_over_the_legal_moves():
    geom = ("gomoku", 7)
    mode, alpha, first, key = FALLBACK
    got = N.noise_rows(*geom, N.cells_of(geom), N.SEED, first, key, mode, alpha)
    dead = [g for g in range(N.ROW_G) if got.gam[g].sum() == 0.0]
    assert N.ROW_G // 2 <= len(dead) < N.ROW_G                     # the GPU module's fallback case: most games take the fallback, not all
    assert any(len(got.legal[g]) > 1 for g in dead)
    for g in dead:
        L = got.legal[g]
        assert (got.rows[g, L] == 1.0 / len(L)).all() and got.rows[g].sum() == pytest.approx(1.0, abs=1e-15)


# ---------------------------------------------------------------------------------------------------
# the Dirichlet law over the legal moves, on one fixed seed
# ---------------------------------------------------------------------------------------------------
LAW_GEOM, LAW_POS, LAW_N, LAW_G = ("gomoku", 7), 2, 8, 4096       # the centre stone: eight legal moves
LAW_CASES = [("legal", 0.3), ("total", 10.83), ("legal", 0.03)]


def beta_moments(a, a0):
    """(mean, variance, fourth central moment) of one entry of a Dirichlet with that entry's concentration a and total a0: Beta(a, a0 - a),
    whose raw moments are E[x^k] = prod_{j < k} (a + j) / (a0 + j)."""
    m = [1.0]
    for j in range(4):
        m.append(m[-1] * (a + j) / (a0 + j))
    mu = m[1]
    var = m[2] - mu * mu
    m4 = m[4] - 4 * mu * m[3] + 6 * mu * mu * m[2] - 3 * mu ** 4
    return mu, var, m4


def law_rows(mode, alpha, **plant):
    cells = np.tile(N.POSITIONS[LAW_GEOM][LAW_POS][1], (LAW_G, 1))
    return N.noise_rows(*LAW_GEOM, cells, N.SEED, R.LAW_FIRST, R.LAW_MOVE, mode, alpha, **plant)


def law_deviations(rows, L, a_eff):
    """Per legal entry: |sample mean - 1 / n| and |sample variance - V| in units of their standard errors over LAW_G independent rows.
    The mean's is sqrt(V / G); the variance's is sqrt((m4 - V^2) / G), the large-sample standard error of a sample variance."""
    n = len(L)
    mu, var, m4 = beta_moments(a_eff, n * a_eff)
    assert mu == pytest.approx(1.0 / n) and var == pytest.approx((1.0 / n) * (1.0 - 1.0 / n) / (n * a_eff + 1.0))
    x = rows[:, L]
    dm = np.abs(x.mean(axis=0) - mu) / math.sqrt(var / LAW_G)
    dv = np.abs(x.var(axis=0) - var) / math.sqrt((m4 - var * var) / LAW_G)
    return dm, dv


@pytest.mark.parametrize("mode,alpha", LAW_CASES)
def test_rows_follow_the_dirichlet_law_over_the_legal_moves(mode, alpha):
    """4 096 rows of one position with n = 8: every entry's mean within 5 standard errors of 1 / n, every entry's variance within 5 standard
    errors of (1 / n)(1 - 1 / n) / (n alpha_eff + 1)."""
    got = law_rows(mode, alpha)
    L = got.legal[0]
    assert len(L) == LAW_N and all(l == L for l in got.legal)
    a_eff = alpha if mode == "legal" else alpha / LAW_N
    dm, dv = law_deviations(got.rows, L, a_eff)
    print(f"{mode} {alpha}: largest deviation of a mean {dm.max():.2f}, of a variance {dv.max():.2f} standard errors")
    assert dm.max() < 5.0 and dv.max() < 5.0
    assert np.abs(got.rows.sum(axis=1) - 1.0).max() <= 1e-12


@pytest.mark.parametrize("mode,alpha", LAW_CASES)
def test_the_law_test_notices_normalisation_over_the_whole_action_vector(mode, alpha):
    """The recipe the option replaces - the row normalised over all 49 entries, read at the legal ones - is tens of standard errors off."""
    got = law_rows(mode, alpha, _plant="all")
    a_eff = alpha if mode == "legal" else alpha / LAW_N
    dm, dv = law_deviations(got.rows, got.legal[0], a_eff)
    print(f"planted, {mode} {alpha}: means {dm.min():.1f} .. {dm.max():.1f} standard errors off")
    assert dm.min() > 5.0


# ---------------------------------------------------------------------------------------------------
# the GPU module's inputs are unambiguous
# ---------------------------------------------------------------------------------------------------
SUBNORMAL = 2.2250738585072014e-308


@pytest.mark.parametrize("geom", N.GEOMETRIES, ids=str)
def test_no_gpu_input_set_has_a_borderline_decision(geom):
    """Over every try of every legal entry of every setting of test_gpu_root_noise.py the accept / reject decisions keep the 1e-9 floor
    test_rng_restated.py asserts for its sets, so host and device take the same tries.  With alpha_eff down to 0.03 / 192 most draws of a row
    underflow (U^6400): the count of gammas that come out subnormal is printed.  Such a gamma keeps fewer bits than a double, so a last-bit
    difference between two pow implementations moves it only where the exact value sits on a rounding boundary of the coarser grid."""
    game, size = geom
    cells = N.cells_of(geom)
    worst, under, zero = math.inf, 0, 0
    for mode, alpha, first, key in N.SETTINGS + [FALLBACK]:
        got = N.noise_rows(game, size, cells, N.SEED, first, key, mode, alpha)
        for g in range(N.ROW_G):
            L = got.legal[g]
            worst = min(worst, float(got.margin[g, L].min()))
            assert got.tries[g, L].min() >= 1 and got.tries[g, L].max() <= 8
            under += int(((got.gam[g, L] > 0.0) & (got.gam[g, L] < SUBNORMAL)).sum())
            zero += int((got.gam[g, L] == 0.0).sum())
    print(f"{geom}: smallest margin {worst:.2e}, gammas that underflow to 0: {zero}, to a subnormal: {under}")
    assert worst > 1e-9, (geom, worst)


def test_the_count_independence_set_is_unambiguous_too():
    geom = ("gomoku", 7)
    got = N.noise_rows(*geom, N.cells_of(geom, 64), N.SEED, 2 ** 32 - 2, 1, "total", 10.83)
    assert min(float(got.margin[g, got.legal[g]].min()) for g in range(64)) > 1e-9


# ---------------------------------------------------------------------------------------------------
# the refusals of selfplay.check_root_noise
# ---------------------------------------------------------------------------------------------------
def test_check_root_noise():
    from selfplay import check_root_noise
    assert check_root_noise(None) is None and check_root_noise(None, dirichlet=False, evaluator=None) is None
    assert check_root_noise(("legal", 0.03)) == ("legal", 0.03) and check_root_noise(["total", 10]) == ("total", 10.0)
    for bad in (("legal",), ("legal", 0.03, 1), "legal", 0.03, ("both", 0.03), (1, 0.03), ("legal", None), ("legal", True),
                ("legal", 0.0), ("legal", -1.0), ("total", float("nan")), ("total", float("inf"))):
        with pytest.raises(ValueError, match="root_noise"):
            check_root_noise(bad)
    with pytest.raises(ValueError, match="dirichlet=False"):
        check_root_noise(("legal", 0.03), dirichlet=False)
    for ev in (None, (None, lambda x: x), (lambda x: x, None)):
        with pytest.raises(ValueError, match="vanilla"):
            check_root_noise(("legal", 0.03), evaluator=ev)
    with pytest.raises(ValueError, match="gumbel_root"):
        check_root_noise(("legal", 0.03), gumbel_root=(16, 50.0, 1.0))
    with pytest.raises(ValueError, match="noise_fn"):
        check_root_noise(("legal", 0.03), noise_fn=lambda mv: None)


def test_the_drivers_refuse_before_any_engine_exists():
    """No GPU here: a refusal that came after Engine() would be an AzkError about the missing device, not a ValueError."""
    import train as az_train
    from games import Gomoku
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner, self_play_batch
    ev = lambda x: None                                            # noqa: E731  (never called)
    for make in (lambda **kw: self_play_batch("gomoku", kw.pop("evaluator", ev), 2, 8, size=7, **kw),
                 lambda **kw: SelfPlayRunner("gomoku", kw.pop("evaluator", ev), 2, 8, size=7, **kw),
                 lambda **kw: AsyncSelfPlayRunner("gomoku", kw.pop("evaluator", ev), 2, 8, size=7, **kw)):
        with pytest.raises(ValueError, match="root_noise"):
            make(root_noise=("legal", 0.0))
        with pytest.raises(ValueError, match="dirichlet=False"):
            make(root_noise=("legal", 0.03), dirichlet=False)
        with pytest.raises(ValueError, match="vanilla"):
            make(root_noise=("legal", 0.03), evaluator=None)
        with pytest.raises(ValueError, match="gumbel_root"):
            make(root_noise=("legal", 0.03), gumbel_root=(4, 50.0, 1.0))
    with pytest.raises(ValueError, match="noise_fn"):
        self_play_batch("gomoku", ev, 2, 8, size=7, root_noise=("total", 10.83), noise_fn=lambda mv: None)
    with pytest.raises(ValueError, match="batched"):
        az_train.collect_data(Gomoku, ev, None, 2, 8, batched=False, root_noise=("legal", 0.03))
