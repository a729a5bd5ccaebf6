"""The product RNG on the device - Engine.gen_noise through the C ABI as shipped (azk_gen_noise: k_gen_noise in
csrc/azk_noise.hip over noise_uniform and noise_row in csrc/azk_rng.h) and the playout-cap coin - against the float64 restatement of tests/rng_restated.py, which test_rng_restated.py
pins on the CPU to the published Philox vectors and to the Gamma(alpha) law.  Uniforms and coins are integer arithmetic and one exact
conversion: bit for bit.  Rows go through log / cos / sqrt / pow of two different libms: entry by entry within ROW_RTOL, no row and
no entry left out; the CPU module shows that no accept / reject decision of these inputs is close enough to flip."""
import numpy as np
import pytest
import torch

import rng_restated as R

pytestmark = pytest.mark.gpu

# |got - want| <= ROW_RTOL * want + ROW_ATOL, derived and not measured: host and device log, cos, sqrt and pow are each good to a few ulp
# (2^-53 = 1.1e-16) and an entry is at most eight dependent operations deep, then divided by a sum of at most 400 positive terms taken
# in another order (lane partials and a tree on the device, pairwise on the host): about 3e-15 for a typical entry.  One step magnifies:
# t = 1 + x / sqrt(9 d) cancels when x is near -sqrt(9 d), a last-bit difference in x grows by 1 / t and v = t^3 triples it - moving
# EVERY cos of the restatement by one ulp moves the 921 600 entries of the largest case by at most 6.1e-14.  1e-12 stays an order above
# that and four below the 1e-8 relative step of a float32 anywhere in the chain.  The engine files are compiled without FMA contraction,
# so the arithmetic between the libm calls is the restatement's own.  ROW_ATOL only covers subnormal entries; the smallest gamma of
# these inputs is 3.4e-191 (test_rng_restated.py asserts > 1e-290), so it passes nothing.
# Seen on an MI355X: 1.4e-14 at the largest (the 4096 x 225 case, a small-t entry), at most 3.6e-15 in the 64-game cases.
ROW_RTOL, ROW_ATOL = 1e-12, 1e-300

_engines = {}


def engine(game, size, G):
    """One tiny engine (max_sims = 1) per geometry and game count, shared by the cases."""
    import azk
    key = (game, size, G)
    if key not in _engines:
        _engines[key] = azk.Engine(game, G, 1, size=size)
    return _engines[key]


def games(first, G):
    return np.arange(G, dtype=np.uint64) + np.uint64(first)


def assert_rows(got, want, tag):
    """Every entry within the bound; prints the largest relative difference before asserting."""
    got = got.cpu().numpy()
    assert got.shape == want.shape and np.isfinite(got).all() and (want > 0).all(), tag
    rel = np.abs(got - want) / want
    print(f"{tag}: largest relative difference {rel.max():.3e}")
    bad = np.abs(got - want) > ROW_RTOL * want + ROW_ATOL
    assert not bad.any(), (tag, int(bad.sum()), float(rel.max()), np.argwhere(bad)[:4].tolist())
    return float(rel.max())


# ---------------------------------------------------------------------------------------------------
# uniforms and coins, bit for bit
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.SEEDS)
def test_move_uniforms_bit_for_bit(seed):
    """Four games per call; first game 2^32 - 2 puts two of them on either side of the 32-bit boundary (counter word 1 live), the seeds
    above 2^32 make the key's high word live."""
    e = engine("gomoku", 7, 4)
    for first in R.FIRST_GAMES:
        for move in R.MOVES:
            _, u = e.gen_noise(seed, first, move, want_noise=False)
            want = torch.from_numpy(R.move_uniform(seed, games(first, 4), move))
            assert u.dtype == torch.float64 and torch.equal(u.cpu(), want), (seed, first, move, u.cpu().tolist(), want.tolist())
    e.check_error()


def test_coins_across_the_32_bit_game_boundary():
    """azk_get_search_full at first_global_game = 2^32 - 2 (tests/test_gpu_playout_cap.py stays below 2^32)."""
    import azk
    first, seed = 2 ** 32 - 2, R.LAW_SEED
    e = azk.Engine("gomoku", 4, 1, size=7)
    kinds = set()
    for p_full in (0.25, 0.5):
        e.set_playout_cap(p_full, 1, seed, first)
        for move in range(8):
            e.begin_search_budget(None, 1, 8, move_index=move)
            want = (R.coin(seed, games(first, 4), move) < p_full).astype(np.uint8)
            assert e.search_full().cpu().numpy().tolist() == want.tolist(), (p_full, move)
            kinds.update(want.tolist())
    assert kinds == {0, 1}
    e.check_error()


# ---------------------------------------------------------------------------------------------------
# rows, entry by entry
# ---------------------------------------------------------------------------------------------------
def check_set(game, size, A, G, seed, first, move, alpha):
    e = engine(game, size, G)
    assert e.action_dim == A
    noise, u = e.gen_noise(seed, first, move, alpha=alpha)
    e.check_error()
    want = R.gamma_rows(A, seed, first, G, move, alpha)
    assert torch.equal(u.cpu(), torch.from_numpy(R.move_uniform(seed, games(first, G), move)))
    return assert_rows(noise, want.rows, (game, size, hex(seed), first, move, alpha))


@pytest.mark.parametrize("alpha", R.ALPHAS)
@pytest.mark.parametrize("game,size,A", R.GAMES)
def test_rows_at_every_lane_occupancy(game, size, A, alpha):
    """A = 9 and 7: 55 / 57 lanes idle in the loop, all 64 in the reduction; 49; 64: exactly one pass; 225: three passes and 33 lanes of
    a fourth; 400: the largest a << 8.  64 games each.  Largest relative difference seen on an MI355X over the 18 cases: 3.6e-15."""
    check_set(game, size, A, R.ROW_G, R.LAW_SEED, 100, 1, alpha)


@pytest.mark.parametrize("seed", R.SEEDS)
def test_rows_at_the_seed_game_and_move_edges(seed):
    """The key's high word, counter word 1 across the 32-bit boundary and the move word, on A = 49."""
    for s in R.EDGE_SETS:
        if s[4] == seed:
            check_set(*s)


def test_rows_of_the_law_test():
    """All 4096 x 225 entries of the rows whose gammas test_rng_restated.py holds to Gamma(0.03) (same seed, first game and move): with
    the entry bound the law shown on the CPU is the device rows' law, and so are E[max] = 0.255 +- 0.01 and the row sums.
    Largest relative difference seen on an MI355X: 1.389e-14, the largest of the module - below the 1e-13 that would ask for a culprit;
    it is the cancellation in t = 1 + x / sqrt(9 d) described at ROW_RTOL, not one function's error."""
    game, size, A, G, seed, first, move, alpha = R.LAW_SET
    e = engine(game, size, G)
    noise, _ = e.gen_noise(seed, first, move, alpha=alpha)
    e.check_error()
    want = R.gamma_rows(A, seed, first, G, move, alpha).rows
    assert_rows(noise, want, "law")
    assert abs(noise.max(1).values.mean().item() - 0.255) <= 0.01
    assert (noise.sum(1) - 1.0).abs().max().item() <= 1e-12


# ---------------------------------------------------------------------------------------------------
# bookkeeping
# ---------------------------------------------------------------------------------------------------
def test_either_output_alone():
    """noise_dev = NULL: the uniforms are still written; uniforms_dev = NULL: the rows are.  Through the raw ABI a buffer that is not passed
    keeps its contents (the sentinel) while the other one gets exactly what a call with both writes."""
    import ctypes as C
    e = engine("gomoku", 7, R.ROW_G)
    seed, first, move, alpha = 7, 100, 3, 0.3
    both_n, both_u = e.gen_noise(seed, first, move, alpha=alpha)
    n_only, none_u = e.gen_noise(seed, first, move, alpha=alpha, want_uniforms=False)
    none_n, u_only = e.gen_noise(seed, first, move, alpha=alpha, want_noise=False)
    assert none_u is None and none_n is None and torch.equal(n_only, both_n) and torch.equal(u_only, both_u)
    rows = torch.full_like(both_n, -7.0)
    uni = torch.full_like(both_u, -7.0)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    e._chk(e.L.azk_gen_noise(e.h, seed, first, move, alpha, None, C.c_void_p(uni.data_ptr()), stream))
    torch.cuda.synchronize()
    assert (rows == -7.0).all() and torch.equal(uni, both_u)
    uni.fill_(-7.0)
    e._chk(e.L.azk_gen_noise(e.h, seed, first, move, alpha, C.c_void_p(rows.data_ptr()), None, stream))
    torch.cuda.synchronize()
    assert (uni == -7.0).all() and torch.equal(rows, both_n)
    e.check_error()


def test_rows_do_not_depend_on_the_engines_game_count_across_the_boundary():
    """Games 2^32 - 2 .. 2^32 + 1 from a 64-game engine, a 4-game engine and a 2-game engine that starts at 2^32: the same bits."""
    first = 2 ** 32 - 2
    n64, u64 = engine("gomoku", 7, R.ROW_G).gen_noise(R.LAW_SEED, first, 1, alpha=0.3)
    n4, u4 = engine("gomoku", 7, 4).gen_noise(R.LAW_SEED, first, 1, alpha=0.3)
    n2, u2 = engine("gomoku", 7, 2).gen_noise(R.LAW_SEED, first + 2, 1, alpha=0.3)
    assert torch.equal(n64[:4], n4) and torch.equal(u64[:4], u4) and torch.equal(n4[2:], n2) and torch.equal(u4[2:], u2)
    low, _ = engine("gomoku", 7, 2).gen_noise(R.LAW_SEED, 0, 1, alpha=0.3)
    assert not torch.equal(low[0], n2[0]) and not torch.equal(low[1], n2[1])       # ... and 2^32 + k is not k's row under another name
