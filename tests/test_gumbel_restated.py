"""CPU checks of tests/gumbel_restated.py, the yardstick of tests/test_gpu_gumbel.py: the schedule's literal rows and its two properties, the
restatement with the reference's root rule against oracle.mcts, and the preconditions of the positions the GPU tests use."""
import numpy as np
import pytest

import forced_playouts_restated as fr
import gumbel_restated as gr
from oracle import az_oracle as ao


def test_schedule_rows():
    assert gr.schedule(4, 15) == [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6]
    assert gr.schedule(3, 7) == [0, 0, 0, 1, 1, 2, 2]
    assert gr.schedule(2, 5) == [0, 0, 1, 1, 2]
    assert gr.schedule(16, 63)[:40] == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4 + [4] * 4 + [5, 5, 6, 6]
    assert gr.schedule(1, 4) == [0, 1, 2, 3] and gr.schedule(0, 3) == [0, 1, 2]
    for m in range(2, 17):
        for n in (1, 15, 63):
            ph = gr.phases(m, n)
            assert ph[0][0] == 0 and sum(p[1] for p in ph) == n and all(a[0] + a[1] == b[0] for a, b in zip(ph, ph[1:]))


def test_every_simulation_finds_an_eligible_child_and_m_children_are_visited():
    """m in 1..16, n in 1..64, nch in {m, m + 3, 60}, arbitrary scores: a child is eligible at every selection, exactly min(m, nch) children get
    visits (min(m, nch, n) where the search is shorter than that), and the played child is one the last phase selected."""
    rng = np.random.RandomState(5)
    for m in range(1, 17):
        for n in range(1, 65):
            for nch in (m, m + 3, 60):
                mp = min(m, nch)
                sched = gr.schedule(mp, n)
                gl, q = rng.gumbel(size=nch), rng.uniform(-1, 1, nch)
                N = np.zeros(nch, np.int64)
                picked = []
                for t in range(n):
                    cv = sched[t]
                    el = N == cv
                    assert el.any(), (m, n, nch, t)
                    score = np.where(el, gl + (50.0 + cv) * q * (N > 0), -np.inf)
                    i = int(np.argmax(score))
                    N[i] += 1
                    picked.append(i)
                assert int((N > 0).sum()) == min(mp, n), (m, n, nch)
                top = np.flatnonzero(N == N.max())
                played = int(top[np.argmax((gl + (50.0 + N.max()) * q)[top])])
                last = picked if mp == 1 else picked[gr.phases(mp, n)[-1][0]:]
                assert played in last, (m, n, nch)


@pytest.mark.parametrize("name", sorted(gr.GAMES))
def test_with_the_reference_root_rule_it_is_the_oracle_search(name):
    og = fr.oracle_game(name)
    ev_l, ev_p = gr.logits_evaluator(og), fr.hash_evaluator(og)
    for g in (0, 3, 7):
        cells, to_move, mc = fr.position(og, gr.slot_seed(name, g), gr.PLIES[g])
        for noise in (None, np.random.RandomState(g).dirichlet([0.3] * og.action_dim)):
            root = gr.GNode(None, None, to_move, mc)
            gr.mcts(og, root, og.board_from_cells(cells, to_move), 40, ev_l, noise, None)
            tree = ao.OracleTree(og)
            tree.reset(int(to_move), int(mc))
            ao.mcts(og, tree, og.board_from_cells(cells, to_move), 40, ev_p, noise)
            assert fr.same_tree(fr.export(root), tree.export()), (name, g, noise is None)


@pytest.mark.parametrize("name", sorted(gr.GAMES))
def test_the_gpu_positions_show_the_option(name):
    off_first_max = 0
    for n_sims, m, og, g, s in [(n_sims, m, og, g, s) for n_sims, m in gr.CASES for og, slots in [gr.small_case(name, n_sims, m)] for g, s in enumerate(slots)]:
        ch = s["children"]
        visits = np.asarray(ch["visit"])
        mp = min(m, len(visits))
        assert len(gr.phases(mp, n_sims - 1)) >= 2, (name, g)                       # at least two halving phases
        assert all(e >= 1 for _, _, e in s["log"]) and len(s["log"]) == n_sims - 1
        assert int((visits > 0).sum()) == mp
        assert ((visits > 0) & (visits < visits.max())).any(), (name, g)            # a child was dropped
        raw = fr.pi_of(og, ch["cell"], visits)
        assert s["target"].tobytes() != raw.tobytes() and abs(s["target"].sum() - 1.0) < 1e-12
        assert (s["target"] > 0).sum() == len(visits)                               # every legal move has mass, visited or not
        assert visits[s["move_index"]] == visits.max()
        off_first_max += s["move_index"] != int(np.argmax(visits))
    # in at least one slot of the game, a played move that is not the first most-visited child (Connect4 at 64 simulations cannot show it: seven
    # children leave the 63rd selection alone in its round, so one child has the most visits; its 17-simulation searches do)
    assert off_first_max >= 1, name


def test_wide_roots_select_at_high_list_indices():
    for i, want_nch in enumerate((48, 96, 192)):
        og, s = gr.wide_case(i)
        assert len(s["children"]["cell"]) == want_nch
        idx = [j for _, j, _ in s["log"]]
        if want_nch > 64:
            assert max(idx) >= 64
        if want_nch > 128:
            assert max(idx) >= 128 and any(64 <= j < 128 for j in idx)
        assert int((np.asarray(s["children"]["visit"]) > 0).sum()) == gr.WIDE_M


def test_gumbel_uniforms_are_strictly_inside_the_unit_interval_and_keyed():
    u = gr.gumbel_uniforms(49, 0x0123456789ABCDEF, 2 ** 32 - 2, 4, 3)
    assert u.shape == (4, 49) and (u > 0).all() and (u < 1).all() and len(np.unique(u)) == u.size
    assert (u * 2.0 ** 52 - 0.5 == np.floor(u * 2.0 ** 52)).all()                   # (x + 0.5) * 2^-52 with x a 52-bit integer: exact
    assert not np.array_equal(u, gr.gumbel_uniforms(49, 0x0123456789ABCDEF, 2 ** 32 - 2, 4, 4))
    assert np.isfinite(gr.gumbel_rows(49, 7, 0, 4, 0)).all()
