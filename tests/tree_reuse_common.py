"""Helpers shared by the tree-reuse tests (TEST INFRASTRUCTURE): the golden fixture's loader, the move's Dirichlet rows, and the
re-root of an exported tree (azk_export_tree's rows) as include/azk.h defines it."""
import hashlib
import struct

import numpy as np

from conftest import golden_meta, load_golden

Z = load_golden("tree_reuse.npz")
META = golden_meta(Z)
IDS = [f"{m['case']}-{m['game']}{m['size']}-n{m['n_sims']}-mode{m['mode']}-{'dir' if m['dirichlet'] else 'nodir'}-{m['variant']}" for m in META]
COLS = ("depth", "cell", "visit", "value", "prior")


def geometry(m):
    """rows, cols, action_dim, max children of the case's game"""
    if m["game"] == "connect4":
        return 6, 7, 7, 7
    n = m["size"]
    return n, n, n * n, n * n


def action_of(m, cell):
    return cell % 7 if m["game"] == "connect4" else cell


def noise_rows(m):
    """The rows and uniforms the generator drew: legacy RandomState(seed + 1000), dirichlet then random_sample per move."""
    A = geometry(m)[2]
    rng = np.random.RandomState(m["seed"] + 1000)
    n_moves = len(Z[f"g{m['case']}_chosen"])
    rows, us = [], []
    for _ in range(n_moves):
        rows.append(rng.dirichlet([0.03] * A))
        us.append(rng.random_sample())
    rows = np.stack(rows)
    assert hashlib.sha256(rows.tobytes()).hexdigest() == m["noise_sha256"], "numpy's legacy Dirichlet stream moved"
    assert np.array(us).tobytes() == Z[f"g{m['case']}_u"].tobytes()
    return rows


def digest(e, priors=True):
    h = hashlib.sha256()
    for d, c, n, w, p in zip(*(e[k] for k in COLS)):
        if priors:
            h.update(struct.pack("<iiqdd", int(d), int(c), int(n), float(w), float(p)))
        else:
            h.update(struct.pack("<iiqd", int(d), int(c), int(n), float(w)))
    return h.hexdigest()


def subtree_of(e, cell):
    """Rows of the subtree under the root's child that plays `cell`, or None if the root has no such child."""
    depth = np.asarray(e["depth"])
    idx = [i for i in range(len(depth)) if depth[i] == 1 and int(e["cell"][i]) == cell]
    if not idx:
        return None
    i = idx[0]
    j = i + 1
    while j < len(depth) and depth[j] > 1:
        j += 1
    return {k: np.array(e[k][i:j]) for k in COLS}


def reroot(e, cell, action_idx, noise=None):
    """The tree a reuse engine must hold after azk_advance played `cell` and the next search began: the chosen child's subtree
    with depths from the new root, the root's cell -1 and prior 0.0, and - with a Dirichlet row - the new root's children on
    (double)(0.75f * prior) + 0.25 * noise[action] (utils.add_dirichlet_noise on a float32 prior row)."""
    s = subtree_of(e, cell)
    s["depth"] = s["depth"] - 1
    s["cell"][0] = -1
    s["prior"][0] = 0.0
    if noise is not None:
        for i in np.nonzero(s["depth"] == 1)[0]:
            p32 = np.float32(s["prior"][i])
            assert float(p32) == s["prior"][i]                       # an inner node's prior is a float32 softmax entry
            s["prior"][i] = np.float64(np.float32(0.75) * p32) + 0.25 * noise[action_idx(int(s["cell"][i]))]
    return s


def same_tree(a, b):
    return all(np.asarray(a[k]).astype(np.float64).tobytes() == np.asarray(b[k]).astype(np.float64).tobytes() for k in COLS)
