"""Value targets (include/azk.h azk_set_value_target), restated in plain Python float64 (TEST INFRASTRUCTURE, not product
code): the target of every ply of one finished game from its record, one loop from the last ply down, no numpy reductions; its closed form;
and the expected tuple list of the game.  Nothing here reads the engine; tests/test_value_target_restated.py holds the loop to the closed form.

q_i is the root's W / N at the move of ply i - the value for the mover's OPPONENT - so v_i = -q_i is the mover's own search value, and z_i is
the outcome from the mover's view.  The side to move alternates, hence the sign in the recurrence."""
import numpy as np

import emission_restated as er


def outcome(winner, ply):
    """z of a ply: +1 where its mover (side ply & 1) is the winner, -1 where the other side is, +0.0 for a draw (winner -1)."""
    if winner == -1:
        return 0.0
    return 1.0 if (ply & 1) == winner else -1.0


def targets(qs, winner, first_ply, r, lam):
    """-> list of Python floats, t_i for the plies first_ply .. first_ply + len(qs) - 1 (qs[k] is the q of ply first_ply + k):
        G_last = (1 - lam) * v_last + lam * z_last;    G_i = (1 - lam) * v_i + lam * (-G_{i+1});    t_i = (1 - r) * z_i + r * G_i"""
    r, lam = float(r), float(lam)
    n = len(qs)
    out = [0.0] * n
    G = 0.0
    for k in range(n - 1, -1, -1):
        z = outcome(winner, first_ply + k)
        v = -float(qs[k])
        G = (1.0 - lam) * v + lam * (z if k == n - 1 else -G)
        out[k] = (1.0 - r) * z + r * G
    return out


def horizon_closed_form(qs, winner, first_ply, lam):
    """G_i = (1 - lam) * sum_k (-lam)^k v_{i+k} + (-lam)^(n-1-i) * lam * z_{n-1}, by powers (another route to the same numbers).  The
    outcome in the last term is the LAST ply's: unrolling the recurrence carries z_{n-1} down with one sign change per ply, and since
    z_{n-1} = (-1)^(n-1-i) * z_i the term is lam^(n-i) * z_i - at lam = 1 every G_i is z_i, as the rule's identity case demands."""
    n = len(qs)
    out = []
    for i in range(n):
        s = 0.0
        for k in range(n - i):
            s += (-lam) ** k * -float(qs[i + k])
        out.append((1.0 - lam) * s + (-lam) ** (n - 1 - i) * lam * outcome(winner, first_ply + n - 1))
    return out


def ring_z(t):
    """What the ring keeps of a target: (float)t."""
    return float(np.float32(t))


def game_tuples(game, boards, pis, winner, elements, values, first_ply=0, full=None, copies=None):
    """-> list of (state float32 [F, R, C], pi float64 [A], z) in ring order for one finished game whose record starts at ply first_ply:
    emission_restated's canonical / turn, plies 0 and 1 (absolute) once and later ones once per element, a fast ply (full) left out, a ply's
    group `copies` times copy-major - with values[k] as the z of every tuple of ply first_ply + k (None: the outcome)."""
    out = []
    for k, (b, p) in enumerate(zip(boards, pis)):
        i = first_ply + k
        if full is not None and not full[k]:
            continue
        z = outcome(winner, i) if values is None else values[k]
        st = er.canonical(b, i & 1)
        group = [er.turn(st, p, s, game) + (z,) for s in ((0,) if i < 2 else tuple(elements))]
        out += group * (1 if copies is None else int(copies[k]))
    return out
