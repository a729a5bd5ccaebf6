"""Policy surprise weighting on the GPU (azk_set_surprise_weighting): what a move records (the coin bit for bit, the kl
within a float64 bound), the emission pinned bit for bit given the recorded values (tests/surprise_restated.py on the engine's own record),
lambda = 0 against the engine without the option, the asynchronous movers against the lock-step runner in all sixteen (re-root, cap,
resign, forced) combinations, sharding, and the ABI's refusals.  G = 8 games, 24 simulations, the "hash" fixture evaluator.

Liveness is asserted, not measured: every emission batch must hold a recorded ply with no copy and one with two or more.  Seeds: every
batch runs at SEED = 3; SEEDS lists the batches that need another seed for that, and why."""
import ctypes as C
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import emission_restated as er
import surprise_restated as sr
import test_gpu_emit_symmetry as es
from fixture_eval import fixture_logits_value
from test_gpu_playout_cap import GAMES, ring_rows

pytestmark = pytest.mark.gpu

G, SIMS, SEED, LAM, MOVES = 8, 24, 3, 0.5, 12
CAP, K, RESIGN, REROOT = (0.5, 6), 2.0, (0.25, 0.5), 2
# batch name -> seed, where SEED = 3 leaves a batch without a ply of no copy or without one of two or more copies (none needed one so far)
SEEDS = {}


def evaluator(A):
    return lambda x: fixture_logits_value(x, A, "hash")


@functools.lru_cache(maxsize=None)
def play(name, game, size, emit, lam=LAM, capacity=None, playout_cap=None, forced_playouts=None, resign=None, n_games=G, first=0, max_moves=None,
         with_ring=True):
    """One lock-step batch, to the end unless max_moves, the ring attached -> (results, ring as numpy, cursor); computed once per case."""
    from selfplay import self_play_batch
    planes, rows, cols, A = es.geometry(game, size)
    rp = es.new_ring(game, size, capacity or n_games * er.count_tuples(rows * cols, 8) * 2) if with_ring else None
    res = self_play_batch(game, evaluator(A), n_games, SIMS, size=size, seed=SEEDS.get(name, SEED), first_global_game=first, replay=rp,
                          emit_symmetry=emit, playout_cap=playout_cap, forced_playouts=forced_playouts, resign=resign, surprise_weight=lam,
                          max_moves=max_moves)
    return res, (es.ring_numpy(rp) if rp is not None else None), (int(rp.cursor.item()) if rp is not None else None)


def group_elements(game, size, emit):
    """The elements of a ply's group: the mask's, or - option off, square boards - the reference's eight."""
    return es.elements_of(game, size, emit) if emit is not None else tuple(range(8))


def kind_of(game):
    return "connect4" if game == "connect4" else "gomoku"


# ---- 1. the move's record ------------------------------------------------------------------------------------------------------------
RECORD = [("rec-gomoku7", "gomoku", 7, None, {}), ("rec-connect4", "connect4", None, "board", {}), ("rec-tictactoe", "tictactoe", None, None, {}),
          ("rec-gomoku5x3-forced-cap", "gomoku", (5, 3), "board", dict(playout_cap=CAP, forced_playouts=K))]


@pytest.mark.parametrize("name,game,size,emit,opts", RECORD, ids=[c[0] for c in RECORD])
def test_every_move_records_the_restated_coin_and_a_kl_within_the_bound(name, game, size, emit, opts):
    """coin: the restated Philox value, bit for bit.  kl: within (nch + 8) * 2^-53 * sum |t_a| of the float64 restatement from the recorded pi and
    azk.softmax_rows of the fixture's logits on the ply's canonical board - nch covers any summation order of the nch children's terms, the 8
    the quotient, the product, the two int-to-double conversions and a log within 2 ulp."""
    import azk
    res, _, _ = play(name, game, size, emit, **opts)
    seed = SEEDS.get(name, SEED)
    planes, rows, cols, A = es.geometry(game, size)
    worst, n_plies = 0.0, 0
    for g, r in enumerate(res):
        assert len(r.kl) == len(r.coin) == len(r.boards) > 0
        canon = torch.from_numpy(np.stack([er.canonical(b, i & 1) for i, b in enumerate(r.boards)])).cuda()
        priors = azk.softmax_rows(fixture_logits_value(canon, A, "hash")[0]).cpu().numpy()
        nch = azk.rules_legal_mask(game, torch.from_numpy(np.stack(r.boards)).cuda().contiguous(), A, size=size).cpu().numpy().sum(axis=1)
        for i in range(len(r.boards)):
            assert r.coin[i] == sr.coin(seed, g, i), (g, i)
            want, sum_abs, terms = sr.kl(r.pis[i], priors[i])
            assert terms <= int(nch[i])
            bound = (int(nch[i]) + 8) * 2.0 ** -53 * sum_abs
            err = abs(r.kl[i] - want)
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else math.inf))
            assert err <= bound, (g, i, r.kl[i], want, err, bound)
            assert r.kl[i] >= 0.0
            n_plies += 1
    print(name, "plies", n_plies, "worst error / bound", worst)
    assert any(k > 0.0 for r in res for k in r.kl)


# ---- 2. emission, bit for bit given the recorded values -----------------------------------------------------------------------------
EMIT = [("emit-gomoku7", "gomoku", 7, None, {}),                                        # option-off grouping: the reference's eight
        ("emit-connect4-board", "connect4", None, "board", {}),
        ("emit-connect4-none", "connect4", None, "none", {}),
        ("emit-tictactoe", "tictactoe", None, None, {}),
        ("emit-gomoku7-cap", "gomoku", 7, None, dict(playout_cap=CAP)),
        ("emit-gomoku5x3-forced", "gomoku", (5, 3), "board", dict(forced_playouts=K)),
        ("emit-gomoku7-resign", "gomoku", 7, None, dict(resign=RESIGN)),
        ("emit-tictactoe-wrap", "tictactoe", None, None, dict(capacity=12))]             # a ring smaller than any one game's tuples


def expected_stream(game, size, emit, res, lam, capped):
    els = group_elements(game, size, emit)
    stream, total, all_copies, per_game = {}, 0, [], []
    for r in res:
        assert r.winner is not None and r.replay_base is not None
        want, c = sr.game_tuples(kind_of(game), r.boards, r.pis, r.winner, els, r.kl, r.coin, lam, full=r.full if capped else None)
        assert len(want) == sum(ci * (1 if i < 2 else len(els)) for i, ci in enumerate(c))
        for t, tup in enumerate(want):
            assert r.replay_base + t not in stream
            stream[r.replay_base + t] = tup
        total += len(want)
        per_game.append(len(want))
        all_copies += [ci for i, ci in enumerate(c) if not capped or r.full[i]]
    assert sorted(stream) == list(range(total))                   # the games' ranges tile the stream
    return stream, total, all_copies, per_game


@pytest.mark.parametrize("name,game,size,emit,opts", EMIT, ids=[c[0] for c in EMIT])
def test_emission_equals_the_restated_tuple_list_of_the_engines_own_record(name, game, size, emit, opts):
    res, ring, cursor = play(name, game, size, emit, **opts)
    capped = "playout_cap" in opts
    stream, end, copies, per_game = expected_stream(game, size, emit, res, LAM, capped)
    capacity = len(ring[2])
    print(name, "tuples", end, "plies", len(copies), "no copy", copies.count(0), "two or more", sum(c >= 2 for c in copies), "capacity", capacity)
    es.assert_ring(ring, cursor, stream, end, capacity)
    assert copies.count(0) >= 1 and sum(c >= 2 for c in copies) >= 1          # liveness: the copy path ran with both kinds of ply
    if capped:
        flags = [f for r in res for f in r.full]
        assert any(flags) and not all(flags)
    if "resign" in opts:
        assert any(r.resigned for r in res)
    if "capacity" in opts:
        assert capacity == opts["capacity"] < min(per_game)       # every game alone overflows the ring: wrap and the pushed-out skip


# ---- 3. lambda = 0 is the engine without the option ----------------------------------------------------------------------------------
@pytest.mark.parametrize("game,size,emit", [("gomoku", 7, None), ("connect4", None, "board")])
def test_lambda_zero_writes_the_option_off_ring_and_still_records(game, size, emit):
    res0, ring0, cur0 = play("zero-" + game, game, size, emit, lam=0.0)
    res_off, ring_off, cur_off = play("off-" + game, game, size, emit, lam=None)
    assert cur0 == cur_off > 0
    for a, b in zip(ring0, ring_off):
        assert a.tobytes() == b.tobytes()
    assert [r.replay_base for r in res0] == [r.replay_base for r in res_off]
    assert all(len(r.kl) == len(r.coin) == len(r.boards) for r in res0) and any(k > 0.0 for r in res0 for k in r.kl)
    assert all(r.kl == [] and r.coin == [] for r in res_off)
    assert all(np.array_equal(np.stack(a.pis), np.stack(b.pis)) and a.cells == b.cells and a.winner == b.winner for a, b in zip(res0, res_off))


# ---- 4. the asynchronous movers ------------------------------------------------------------------------------------------------------
CASES = list(itertools.product((0, REROOT), (False, True), (False, True), (False, True)))
# (reroot, cap, resign, forced) -> seed, as test_gpu_mover_variants.SEEDS: re-root + resignation + forced playouts without a cap has no resignation
# within MOVES moves at seed 3; 10 is the first seed with one
CASE_SEEDS = {(REROOT, False, True, True): 10}


def case_id(c):
    return "-".join(n for n, on in zip(("reroot", "cap", "resign", "forced"), c) if on) or "plain"


def lockstep_records(game, moves, seed, **kw):
    """{(slot, move): (pi bytes, q, cell, winner, kind, kl, coin)} of SelfPlayRunner(recycle=True, surprise_weight=LAM), and the runner."""
    from selfplay import SelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(mv, base, pi, q, ch, w, d):
        kl, coin = r.record_surprise
        for g in range(len(ch)):
            if int(ch[g]) >= 0:
                rec[(base + g, mv)] = (pi[g].numpy().tobytes(), float(q[g]), int(ch[g]), int(w[g]), int(r.record_full[g]), float(kl[g]), float(coin[g]))
    r = SelfPlayRunner(game, evaluator(A), G, SIMS, size=size, seed=seed, on_records=on, recycle=True, surprise_weight=LAM, **kw)
    for _ in range(moves):
        r.play_move()
    r.check_error()
    return rec, r


def async_records(game, moves, seed, **kw):
    from selfplay import AsyncSelfPlayRunner
    size, A = GAMES[game]
    rec = {}

    def on(meta, q, pi):
        full = r.record_full if r.record_full is not None else np.ones(len(meta), np.uint8)
        kl, coin = r.record_surprise
        for i in range(len(meta)):
            key = (int(meta[i, 0]), int(meta[i, 1]))
            assert key not in rec, key
            rec[key] = (pi[i].tobytes(), float(q[i]), int(meta[i, 2]), int(meta[i, 3]), int(full[i]), float(kl[i]), float(coin[i]))
    r = AsyncSelfPlayRunner(game, evaluator(A), G, SIMS, size=size, seed=seed, on_records=on, recycle=True, use_graph=False, surprise_weight=LAM, **kw)
    for _ in range(8000):                                         # until EVERY slot has played `moves` moves
        r.run_chunk()
        r.finish()
        if all((g, moves - 1) in rec for g in range(G)):
            break
    r.check_error()
    return rec, r


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_async_movers_play_the_lockstep_games_and_records(case):
    reroot, cap, resign, forced = case
    lock_kw, async_kw = dict(cache_entries=64), dict(cache_entries=64, per_launch=2, steps_per_graph=4)
    if reroot:
        lock_kw["tree_reuse"] = async_kw["reroot"] = reroot
    for name, on, value in (("playout_cap", cap, CAP), ("resign", resign, RESIGN), ("forced_playouts", forced, K)):
        if on:
            lock_kw[name] = async_kw[name] = value
    seed = CASE_SEEDS.get(case, SEED)
    want, lr = lockstep_records("gomoku", MOVES, seed, **lock_kw)
    got, ar = async_records("gomoku", MOVES, seed, **async_kw)
    for g in range(G):
        for mv in range(MOVES):
            assert got[(g, mv)] == want[(g, mv)], (case_id(case), g, mv)
            assert want[(g, mv)][6] == sr.coin(seed, g, mv)
    kinds = [v[4] for v in want.values()]
    lc, ac = lr.counters(), ar.counters()
    # every option of the case was live in both runs, the surprise records included
    assert any(v[5] > 0.0 for v in want.values()) and any(v[5] > 0.0 for v in got.values())
    assert lr.eng.surprise_weight == ar.eng.surprise_weight == LAM
    assert 0 < sum(kinds) < len(kinds) if cap else all(kinds)
    if resign:
        assert lr.resign_stats()[0] > 0 and ar.resign_stats()[0] > 0
    for c in (lc, ac):
        assert (c["visits_pruned"] > 0) == forced and (c["roots_reused"] > 0) == bool(reroot)


@pytest.mark.parametrize("opts", [{}, dict(playout_cap=CAP), dict(reroot=REROOT)], ids=["plain", "cap", "reroot"])
def test_drained_rings_equal_the_lockstep_rings_as_multisets(opts):
    """Games played to their end without restarts: the drain's k_emit_tuples<LIST, .., SURPRISE> against the lock-step emission (the stream's
    order follows the finishing order, so the rings are compared as multisets)."""
    import azk
    from selfplay import AsyncSelfPlayRunner, SelfPlayRunner
    ev = evaluator(49)
    ra, rb = azk.DeviceReplay(8192, 2, 7, 7, 49), azk.DeviceReplay(8192, 2, 7, 7, 49)
    lock = {("tree_reuse" if k == "reroot" else k): v for k, v in opts.items()}
    r = SelfPlayRunner("gomoku", ev, G, SIMS, size=7, seed=SEED, recycle=False, replay=ra, surprise_weight=LAM, **lock)
    for _ in range(49):
        r.play_move()
    r.check_error()
    a = AsyncSelfPlayRunner("gomoku", ev, G, SIMS, size=7, seed=SEED, recycle=False, replay=rb, per_launch=2, steps_per_graph=4, use_graph=False,
                            surprise_weight=LAM, **opts)
    for _ in range(3000):
        a.run_chunk()
        if int(a.finish()[0]) == G:
            break
    a.check_error()
    assert int(a.finish()[0]) == G
    assert 0 < int(ra.cursor.item()) == int(rb.cursor.item()) <= 8192 and sorted(ring_rows(ra)) == sorted(ring_rows(rb))


# ---- 5. sharding -------------------------------------------------------------------------------------------------------------------
def test_two_engines_of_four_games_record_what_one_of_eight_records():
    whole, _, _ = play("shard-8", "gomoku", 7, None, max_moves=MOVES, with_ring=False)
    for first in (0, 4):
        part, _, _ = play("shard-4", "gomoku", 7, None, n_games=4, first=first, max_moves=MOVES, with_ring=False)
        for g in range(4):
            a, b = part[g], whole[first + g]
            assert a.kl == b.kl and a.coin == b.coin and a.cells == b.cells and len(a.kl) > 0
            assert np.array_equal(np.stack(a.pis), np.stack(b.pis)) and a.qs == b.qs


# ---- 6. the ABI's refusals ---------------------------------------------------------------------------------------------------------
def test_abi_refusals():
    import azk
    L = azk.lib()
    ERR_ARG, ERR_STATE = -1, -4
    e = azk.Engine("gomoku", 2, 8, size=7)
    st = azk._stream()
    adv = (None, 0, azk._p(e.chosen), azk._p(e.winner), azk._p(e.done), st)
    assert L.azk_advance_keyed(e.h, None, 0, 0, *adv[2:]) == ERR_STATE            # the option is not set
    assert L.azk_get_surprise(e.h, None, None, st) == ERR_STATE
    assert L.azk_async_surprise_columns(e.h, None, None) == ERR_STATE
    for bad in (-0.25, 1.5, float("nan"), float("inf"), -math.inf):
        assert L.azk_set_surprise_weighting(e.h, C.c_double(bad), 1, 0, st) == ERR_ARG
        assert e.surprise_weight is None
    assert L.azk_set_surprise_weighting(e.h, C.c_double(0.0), 1, 0, st) == 0          # lambda = 0 is a live setting
    assert L.azk_advance(e.h, *adv) == ERR_STATE and b"azk_advance_keyed" in L.azk_last_error(e.h)
    assert L.azk_advance_resign(e.h, None, 0, 0, *adv[2:]) == ERR_STATE
    assert L.azk_advance_keyed(e.h, None, 0, -1, *adv[2:]) == ERR_ARG
    assert L.azk_get_surprise(e.h, None, None, st) == 0
    assert L.azk_clear_surprise_weighting(e.h) == 0
    assert L.azk_advance_keyed(e.h, None, 0, 0, *adv[2:]) == ERR_STATE
    assert L.azk_advance_resign(e.h, None, 0, 0, *adv[2:]) == ERR_STATE           # (no resignation is set either: its own answer, unchanged)
    e.check_error()
    vl = azk.Engine("gomoku", 2, 8, size=7, leaves_per_step=2)
    assert L.azk_set_surprise_weighting(vl.h, C.c_double(0.5), 1, 0, st) == ERR_ARG and b"leaves_per_step" in L.azk_last_error(vl.h)
    c4 = azk.Engine("connect4", 2, 8)                              # created without emit_elements: no trajectories
    assert L.azk_set_surprise_weighting(c4.h, C.c_double(0.5), 1, 0, st) == ERR_ARG and b"trajectories" in L.azk_last_error(c4.h)
    with pytest.raises(azk.AzkError):
        c4.set_surprise_weighting(0.5)
    assert azk.Engine("connect4", 2, 8, emit_symmetry="none").set_surprise_weighting(0.5) is None
