"""Root noise on the legal moves (azk_set_root_noise) on the GPU.  The rows of k_root_noise through the C ABI as shipped,
entry by entry against the plain-Python restatement (tests/root_noise_restated.py, which test_root_noise_restated.py pins on the CPU), under
test_gpu_rng.py's bound; zeros and one-hot rows exactly.  Then what reads the rows: the root's mixed priors on a fresh and on a re-rooted
root, from the device's own row; the asynchronous movers (k_root_noise_due) against the lock-step runner, slot for slot; the option beside the
other options; set-then-cleared against an engine that never had it; every refusal."""
import numpy as np
import pytest
import torch

import root_noise_restated as N
from fixture_eval import fixture_logits_value
from test_gpu_rng import ROW_ATOL, ROW_RTOL
from test_root_noise_restated import FALLBACK

pytestmark = pytest.mark.gpu

_engines = {}
_shared = {}


def shared(key, make):
    """A reference computed once for the tests that need it; never modified afterwards."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


def engine(geom, G=N.ROW_G):
    """One tiny engine (max_sims = 1) per geometry and game count, its games standing in the geometry's positions."""
    import azk
    key = (geom, G)
    if key not in _engines:
        e = azk.Engine(geom[0], G, 1, size=geom[1])
        cells = N.cells_of(geom, G)
        e.set_positions(cells, *N.to_move_and_count(cells))
        _engines[key] = e
    return _engines[key]


def assert_rows(got, want, tag):
    """Legal entries within the bound, every other entry exactly +0.0, one-hot rows exactly 1.0; returns the largest relative difference."""
    got = got.cpu().numpy()
    assert got.shape == want.rows.shape and np.isfinite(got).all(), tag
    worst = 0.0
    for g, L in enumerate(want.legal):
        off = np.setdiff1d(np.arange(got.shape[1]), L)
        assert (got[g, off] == 0.0).all() and not np.signbit(got[g, off]).any(), (tag, g)
        w, x = want.rows[g, L], got[g, L]
        if len(L) == 1:
            assert x[0] == 1.0, (tag, g)
        bad = np.abs(x - w) > ROW_RTOL * w + ROW_ATOL
        pos = w > 0.0
        if pos.any():
            worst = max(worst, float((np.abs(x - w)[pos] / w[pos]).max()))
        assert not bad.any(), (tag, g, int(bad.sum()), x[bad][:4].tolist(), w[bad][:4].tolist())
    return worst


# ---------------------------------------------------------------------------------------------------
# 1. rows, entry by entry
# ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", N.MODES)
@pytest.mark.parametrize("geom", N.GEOMETRIES, ids=str)
def test_rows_entry_by_entry(geom, mode):
    """Every position of the geometry, alphas 0.03 / 0.3 / 10.83, first games 0 and 2^32 - 2, keys 0 / 1 / 511: 18 settings of 8 games.  The
    uniforms are gen_noise's bit for bit.  ROW_RTOL's derivation (tests/test_gpu_rng.py) covers the rows: the same chain per entry, then a
    sum of at most 400 terms.  Largest relative difference seen on an MI355X over the 12 cases: 9.93e-14 (Gomoku 5x9, "total"), 5.3e-14 (15x15,
    "total"), at most 1.8e-15 in every "legal" case: with alpha_eff down to 0.03 / 192 the draw ends in U^(1 / alpha_eff), a power of some
    thousands, where two libms' pow differ by more last bits than at the exponents of test_gpu_rng.py - an order inside the bound."""
    e = engine(geom)
    game, size = geom
    cells = N.cells_of(geom)
    worst = 0.0
    for m, alpha, first, key in N.SETTINGS:
        if m != mode:
            continue
        e.set_root_noise(mode, alpha)
        rows, u = e.gen_root_noise(N.SEED, first, key)
        _, u_plain = e.gen_noise(N.SEED, first, key, want_noise=False)
        assert torch.equal(u, u_plain), (geom, mode, alpha, first, key)
        want = N.noise_rows(game, size, cells, N.SEED, first, key, mode, alpha)
        worst = max(worst, assert_rows(rows, want, (geom, mode, alpha, first, key)))
    e.check_error()
    e.clear_root_noise()
    print(f"{geom} {mode}: largest relative difference {worst:.3e}")


def test_fallback_rows_are_uniform_over_the_legal_moves():
    """alpha = 1e-5: most rows' gammas all underflow (shown on the CPU) and come out 1 / n exactly; the others stay within the bound."""
    geom = ("gomoku", 7)
    e = engine(geom)
    mode, alpha, first, key = FALLBACK
    e.set_root_noise(mode, alpha)
    rows, _ = e.gen_root_noise(N.SEED, first, key)
    want = N.noise_rows(*geom, N.cells_of(geom), N.SEED, first, key, mode, alpha)
    assert_rows(rows, want, "fallback")
    got = rows.cpu().numpy()
    dead = [g for g in range(N.ROW_G) if want.gam[g].sum() == 0.0]
    assert len(dead) >= N.ROW_G // 2
    for g in dead:
        assert (got[g, want.legal[g]] == 1.0 / len(want.legal[g])).all(), g
    e.clear_root_noise()


def test_either_output_alone_and_finished_boards():
    """NULL conventions of azk_gen_noise; a full TicTacToe board (a finished game that waits in the batch) gets a row of zeros."""
    import azk
    e = azk.Engine("tictactoe", 4, 1)
    full = np.array([1, 2, 1, 1, 2, 2, 2, 1, 1], np.int8)
    cells = np.stack([full, np.zeros(9, np.int8), full, np.zeros(9, np.int8)])
    e.set_positions(cells, *N.to_move_and_count(cells))
    e.set_root_noise("total", 10.83)
    both_n, both_u = e.gen_root_noise(7, 100, 3)
    n_only, none_u = e.gen_root_noise(7, 100, 3, want_uniforms=False)
    none_n, u_only = e.gen_root_noise(7, 100, 3, want_noise=False)
    assert none_u is None and none_n is None and torch.equal(n_only, both_n) and torch.equal(u_only, both_u)
    rows = both_n.cpu().numpy()
    assert (rows[[0, 2]] == 0.0).all() and np.abs(rows[[1, 3]].sum(axis=1) - 1.0).max() <= 1e-12 and (rows[[1, 3]] > 0.0).all()
    e.check_error()


def test_rows_do_not_depend_on_the_engines_game_count():
    """Global games 2^32 - 2 .. from a 64-game, a 4-game and a 2-game engine (which starts at 2^32), each game in the same position: the same
    bits.  The positions cycle with period 5, so the 2-game engine's games get the positions of games 2 and 3."""
    import azk
    geom, first = ("gomoku", 7), 2 ** 32 - 2
    cells = N.cells_of(geom, 64)
    out = []
    for G, lo in ((64, 0), (4, 0), (2, 2)):
        e = azk.Engine("gomoku", G, 1, size=7)
        e.set_positions(cells[lo:lo + G], *N.to_move_and_count(cells[lo:lo + G]))
        e.set_root_noise("total", 10.83)
        out.append(e.gen_root_noise(N.SEED, first + lo, 1))
        e.check_error()
    (n64, u64), (n4, u4), (n2, u2) = out
    assert torch.equal(n64[:4], n4) and torch.equal(u64[:4], u4) and torch.equal(n4[2:], n2) and torch.equal(u4[2:], u2)
    want = N.noise_rows(*geom, cells, N.SEED, first, 1, "total", 10.83)
    assert_rows(n64, want, "64 games")


# ---------------------------------------------------------------------------------------------------
# 2. the root's mixed priors, from the device's own row
# ---------------------------------------------------------------------------------------------------
MIX_SIMS, MIX_G = 16, 6
MIX_CELLS = {
    ("gomoku", 7): [N._board(7, 7, s) for s in ([], [(0, 0)], [(3, 3)], [(3, 3), (3, 4)], [(6, 0), (0, 6), (3, 3)], [(2, 2), (4, 4), (2, 4), (4, 2)])],
    ("connect4", None): [N._connect4(h) for h in ([0] * 7, [1, 0, 0, 0, 0, 0, 0], [0, 2, 0, 6, 1, 0, 3], [2, 2, 0, 0, 0, 2, 2], [0, 0, 0, 1, 0, 0, 0],
                                                  [6, 1, 6, 0, 0, 0, 1])],
}


def raw_priors(geom, positions):
    """{cell: float32 prior} of every game's root children for the positions as they stand: a noise-free search of one simulation on an engine
    of its own, whose root children keep the evaluator's softmax entries as they are."""
    import azk
    ref = azk.Engine(geom[0], MIX_G, 1, size=geom[1])
    ref.set_positions(*positions)
    ref.search(evaluator(ref.action_dim), 1, None)
    out = []
    for g in range(MIX_G):
        ch = ref.root_children(g)
        out.append({int(c): np.float32(p) for c, p in zip(ch["cell"], ch["prior"])})
        assert all(float(np.float32(p)) == float(p) for p in ch["prior"])         # (noise-free: the float32 prior itself)
    ref.check_error()
    return out


def assert_mixed(e, geom, row, tag):
    """Every root's child actions are its row's support, and rootP[i] == (double)(0.75f * P_i) + 0.25 * row[action_i], bit for bit."""
    positions = e.get_positions()
    raw = raw_priors(geom, positions)
    row = row.cpu().numpy()
    cols = e.cols
    for g in range(MIX_G):
        ch = e.root_children(g)
        act = [int(c) % cols if geom[0] == "connect4" else int(c) for c in ch["cell"]]
        assert sorted(act) == np.nonzero(row[g])[0].tolist() == N.legal_actions(geom[0], geom[1], positions[0][g]), (tag, g)
        for c, a, p in zip(ch["cell"], act, ch["prior"]):
            want = np.float64(np.float32(0.75) * raw[g][int(c)]) + 0.25 * row[g, a]
            assert float(p) == float(want), (tag, g, int(c), float(p), float(want))


@pytest.mark.parametrize("tree_reuse", [0, 1, 2])
@pytest.mark.parametrize("geom", list(MIX_CELLS), ids=str)
def test_root_priors_mix_the_devices_own_row(geom, tree_reuse):
    """Move 0 searches from fresh roots (k_tree's mix), move 1 - on a tree_reuse engine - from the re-rooted subtree (reroot_one's mix, on the
    stored float32 prior).  root_noise_rows() is the row the search read."""
    import azk
    e = azk.Engine(geom[0], MIX_G, MIX_SIMS, size=geom[1], tree_reuse=tree_reuse)
    cells = np.stack(MIX_CELLS[geom])
    e.set_positions(cells, *N.to_move_and_count(cells))
    e.set_root_noise("total", 10.83)
    ev = evaluator(e.action_dim)
    for move in range(2):
        noise, uni = e.gen_root_noise(N.SEED, 0, move)
        if tree_reuse == 2:
            e.search_budget(ev, MIX_SIMS, noise)
        else:
            e.search(ev, MIX_SIMS, noise)
        rows = e.root_noise_rows()
        assert torch.equal(rows, noise)
        assert_mixed(e, geom, rows, (geom, tree_reuse, move))
        e.advance(uni, 0)
    reused = e.counters()["roots_reused"]
    assert (reused > 0) == (tree_reuse != 0), reused
    e.check_error()


# ---------------------------------------------------------------------------------------------------
# 3. the runners
# ---------------------------------------------------------------------------------------------------
RG, RSIMS, RSEED = 8, 16, 6
RN = ("total", 10.83)
GAMES = {"gomoku": (7, 49), "connect4": (None, 7)}
OPEN = (0.75, 6, 1)


def lockstep_records(game, moves, n_sims=RSIMS, root_noise=RN, **kw):
    """{(slot, move): (pi bytes, q, cell, winner)} of SelfPlayRunner(recycle=True, root_noise=...), and the runner."""
    from selfplay import SelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]))
    r = SelfPlayRunner(game, evaluator(A), RG, n_sims, size=size, seed=RSEED, on_records=on, recycle=True, root_noise=root_noise, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_records(game, moves, n_sims=RSIMS, root_noise=RN, **kw):
    from selfplay import AsyncSelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(meta, q, pi):
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]))
    r = AsyncSelfPlayRunner(game, evaluator(A), RG, n_sims, size=size, seed=RSEED, on_records=on, use_graph=False, root_noise=root_noise, **kw)
    for _ in range(8000):                                         # until EVERY slot has played `moves` moves (slots run at their own pace)
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(RG)):
            break
    r.check_error()
    return rec, r


def assert_same_records(got, want, moves, tag=()):
    for g in range(RG):
        for mv in range(moves):
            assert got[(g, mv)] == want[(g, mv)], tag + (g, mv)


def assert_async_rows_are_the_lockstep_rows(game, got, ra, root_noise):
    """After finish() every slot's game is live and searching under key = the moves its slot has played: root_noise_rows() of the asynchronous
    engine equals, bit for bit, gen_root_noise of a lock-step engine standing in the same positions at that key."""
    import azk
    rows = ra.eng.root_noise_rows().cpu()
    positions = ra.eng.get_positions()
    keys = [1 + max(mv for (g, mv) in got if g == slot) for slot in range(RG)]
    lock = azk.Engine(game, RG, 1, size=GAMES[game][0])
    lock.set_positions(*positions)
    lock.set_root_noise(*root_noise)
    for key in sorted(set(keys)):
        want, _ = lock.gen_root_noise(RSEED, 0, key)
        for g in range(RG):
            if keys[g] == key:
                assert torch.equal(rows[g], want[g].cpu()), (game, g, key)
    lock.check_error()


ASYNC_CASES = {
    # name: (moves, n_sims, lock-step keywords, asynchronous keywords)
    "plain": (16, RSIMS, {}, dict(per_launch=2, steps_per_graph=4)),
    "reroot": (16, RSIMS, dict(tree_reuse=2, cache_entries=64), dict(reroot=2, cache_entries=64, per_launch=2, steps_per_graph=4)),
    "openings": (46, RSIMS, dict(openings=OPEN, openings_seed=11), dict(openings=OPEN, openings_seed=11, per_launch=2, steps_per_graph=4)),
    # a whole search fits between two drains, many times over: without rows made ahead nothing holds a game back to one move per drain, so
    # the record ring is sized for a move per step
    "tiny budget": (20, 2, {}, dict(per_launch=2, steps_per_graph=32, record_capacity=64 * RG)),
    "tiny budget reroot": (20, 2, dict(tree_reuse=1), dict(reroot=1, per_launch=2, steps_per_graph=32, record_capacity=64 * RG)),
}


@pytest.mark.parametrize("case", list(ASYNC_CASES))
@pytest.mark.parametrize("game", list(GAMES))
def test_async_movers_play_the_lockstep_games(game, case):
    moves, n_sims, lock_kw, async_kw = ASYNC_CASES[case]
    mode = ("legal", 0.3) if case == "plain" else RN
    want, rl = lockstep_records(game, moves, n_sims, mode, **lock_kw)
    got, ra = async_records(game, moves, n_sims, mode, **async_kw)
    assert_same_records(got, want, moves, (game, case))
    if case == "openings":                                        # games ended and restarted inside the window, and restarted games were opened
        assert any(v[3] != -2 for (g, mv), v in want.items() if mv < moves - 1)
        assert ra.eng.opening_stats()[0] > RG // 2
    assert_async_rows_are_the_lockstep_rows(game, got, ra, mode)


def test_the_option_changes_the_games_and_cleared_it_does_not():
    """Set and cleared before the first search: the games, byte for byte, of an engine that never had the option; set: other games."""
    from selfplay import self_play_batch
    import azk
    kw = dict(size=7, seed=RSEED, max_moves=12)
    plain = self_play_batch("gomoku", evaluator(49), RG, RSIMS, **kw)
    eng = azk.Engine("gomoku", RG, RSIMS, size=7)
    eng.set_root_noise(*RN)
    eng.clear_root_noise()
    cleared = self_play_batch("gomoku", evaluator(49), RG, RSIMS, engine=eng, **kw)
    left_on = azk.Engine("gomoku", RG, RSIMS, size=7)
    left_on.set_root_noise(*RN)                                   # an engine handed in with the option still on: the batch switches it off
    handed = self_play_batch("gomoku", evaluator(49), RG, RSIMS, engine=left_on, **kw)
    assert left_on.root_noise is None
    with_it = self_play_batch("gomoku", evaluator(49), RG, RSIMS, root_noise=RN, **kw)
    key = lambda res: [(r.cells, [p.tobytes() for p in r.pis], r.qs) for r in res]      # noqa: E731
    assert key(plain) == key(cleared) == key(handed)
    assert key(plain) != key(with_it)


def test_beside_the_other_options():
    """Playout cap, resignation, forced playouts, evaluation symmetry and value targets together with the option: the asynchronous movers play
    the lock-step runner's games, and the drained ring holds the lock-step ring's tuples."""
    import azk
    from collections import Counter
    from test_gpu_openings import ring_rows
    moves = 40
    opts = dict(playout_cap=(0.5, 6), resign=(0.9, 0.25), forced_playouts=2.0, eval_symmetry=True, value_target=(0.5, 0.5), cache_entries=64)
    rings = [azk.DeviceReplay(16384, 2, 7, 7, 49) for _ in range(2)]
    want, rl = lockstep_records("gomoku", moves, RSIMS, RN, replay=rings[0], **opts)
    got, ra = async_records("gomoku", moves, RSIMS, RN, replay=rings[1], per_launch=2, steps_per_graph=4, **opts)
    assert_same_records(got, want, moves)
    assert any(v[3] != -2 for v in want.values())                  # games ended inside the window
    missing = Counter(ring_rows(rings[0])) - Counter(ring_rows(rings[1]))
    assert not missing, sum(missing.values())


def test_graph_runners_equal_eager():
    """The captured step graphs - the lock-step runner's, and the asynchronous one's with k_root_noise_due as one more node of its chain - play
    the eager runners' games."""
    moves = 12
    want, _ = lockstep_records("gomoku", moves)
    got, _ = lockstep_records("gomoku", moves, use_graph=True, steps_per_graph=4)
    assert_same_records(got, want, moves, ("lock-step graph",))
    from selfplay import AsyncSelfPlayRunner
    rec = {}

    def on(meta, q, pi):
        for i in range(len(meta)):
            rec[(int(meta[i, 0]), int(meta[i, 1]))] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]))
    r = AsyncSelfPlayRunner("gomoku", evaluator(49), RG, RSIMS, size=7, seed=RSEED, on_records=on, use_graph=True, steps_per_graph=4, root_noise=RN)
    for _ in range(2000):
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(RG)):
            break
    r.check_error()
    assert_same_records(rec, want, moves, ("asynchronous graph",))


# ---------------------------------------------------------------------------------------------------
# 4. refusals
# ---------------------------------------------------------------------------------------------------
def test_refusals():
    import azk
    e = azk.Engine("gomoku", 2, 8, size=7)
    with pytest.raises(azk.AzkError, match="no root noise is set"):
        e.gen_root_noise(0, 0, 0)
    with pytest.raises(azk.AzkError, match="no root noise is set"):
        e.root_noise_rows()
    with pytest.raises(azk.AzkError, match="mode"):
        e.set_root_noise("both", 0.3)
    for rc_mode in (0, 3, -1):
        assert e.L.azk_set_root_noise(e.h, rc_mode, 0.3, None) == -1 and b"mode must be" in e.L.azk_last_error(e.h)
    assert e.L.azk_gen_root_noise(e.h, 0, 0, 0, None, None, None) == -4 and b"azk_gen_root_noise" in e.L.azk_last_error(e.h)
    for alpha in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(azk.AzkError, match="finite and positive"):
            e.set_root_noise("legal", alpha)
    assert e.root_noise is None
    e.set_root_noise("legal", 0.3)
    with pytest.raises(azk.AzkError, match="no search with a noise row"):
        e.root_noise_rows()
    with pytest.raises(azk.AzkError, match="root noise on the legal moves"):
        e.set_gumbel_root(4, 8)
    e.clear_root_noise()
    e.set_gumbel_root(4, 8)
    with pytest.raises(azk.AzkError, match="Gumbel root is set"):
        e.set_root_noise("legal", 0.3)
    e.clear_gumbel_root()
    # inside a search
    e.set_root_noise("total", 10.83)
    noise, uni = e.gen_root_noise(1, 0, 0)
    e.begin_search(noise)
    with pytest.raises(azk.AzkError, match="search is under way"):
        e.set_root_noise("legal", 0.3)
    with pytest.raises(azk.AzkError, match="search is under way"):
        e.clear_root_noise()
    e.search(evaluator(49), 8, noise)
    e.advance(uni, 0)
    e.set_root_noise("legal", 0.3)                                # between two moves it may change
    # after azk_async_begin
    e.async_begin(8, 2, 0, 1, 0)
    for call in (lambda: e.set_root_noise("legal", 0.3), e.clear_root_noise, lambda: e.gen_root_noise(1, 0, 0)):
        with pytest.raises(azk.AzkError, match="async"):
            call()
    assert e.root_noise_rows().shape == (2, 49)
    e.check_error()
