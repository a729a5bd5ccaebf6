"""What tests/test_gpu_fold_bits.py and tools/record_fold_rows.py share (TEST INFRASTRUCTURE, not product code): the board sets of
the k_embed_fold bit-for-bit check, built from fixed lists and numpy.random.RandomState(0), the tables they run against, and the
digest of a board's rows.  tests/golden/fold_rows_digest.npz holds one sha256 per board, recorded once by the tool from the build
the kernel's later forms are held to."""
import hashlib

import numpy as np

SEED = 6                                    # of the network whose tables the kernel runs with
# name -> (rows, cols, planes, ksize): the benched shape, and the two other patch shapes at their smallest board (Gomoku ships
# 7 x 7 with two planes; tic-tac-toe is 3 x 3 with three)
CONFIGS = {"g15k5": (15, 15, 2, 5), "g7k3": (7, 7, 2, 3), "t3k3": (3, 3, 3, 3)}


def dirty_tokens(board, ksize):
    """Number of tokens some stone of the board [C, R, Cc] reaches (what k_embed_fold compacts into 16-token tiles)."""
    occ = board[:2].sum(0) > 0
    R, Cc = occ.shape
    p = ksize // 2
    hit = np.zeros_like(occ)
    for r, c in zip(*np.nonzero(occ)):
        hit[max(0, r - p):r + p + 1, max(0, c - p):c + p + 1] = True
    return int(hit.sum())


def _put(x, stones):
    for i, (r, c) in enumerate(stones):
        x[i & 1, r, c] = 1.0


def _random(rng, R, Cc, planes, lo, hi):
    x = np.zeros((planes, R, Cc), np.float32)
    m = int(rng.randint(lo, hi + 1))
    cells = rng.choice(R * Cc, size=m, replace=False)
    for i, cell in enumerate(cells):
        x[i & 1, cell // Cc, cell % Cc] = 1.0
    if planes == 3:
        x[2] = float(rng.randint(2))
    return x


def board_set(name):
    """float32 [n, C, R, Cc] of 0 / 1, and what is known of each board: a list of (label, dirty token count or None)."""
    R, Cc, planes, k = CONFIGS[name]
    rng = np.random.RandomState(0)
    boards, labels = [], []

    def add(label, x, nd=None):
        boards.append(x)
        labels.append((label, nd))
    zero = lambda: np.zeros((planes, R, Cc), np.float32)
    add("empty", zero(), 0)
    if name == "g15k5":
        m, e = R // 2, R - 1
        for label, rc in (("corner00", (0, 0)), ("corner0e", (0, e)), ("cornere0", (e, 0)), ("corneree", (e, e)),
                          ("edge-top", (0, m)), ("edge-bottom", (e, m)), ("edge-left", (m, 0)), ("edge-right", (m, e))):
            for plane in (0, 1):
                x = zero()
                x[plane, rc[0], rc[1]] = 1.0
                add(f"{label}-p{plane}", x)
        # the tile boundary.  A 5 x 5 patch clipped by a 15 x 15 board reaches 9, 12, 15, 16, 18, 19, 20, ... tokens: no set of
        # stones reaches exactly 17 (the reached set is a union of rectangles of at least 3 x 3), so the boundary is taken at 16
        # (one full tile), at 18 (the nearest count above it), and at 32 / 33 (two full tiles, and one token more)
        for nd, stones in ((16, [(1, 1)]), (18, [(0, 0), (0, 3)]), (32, [(0, 0), (3, 4)]), (33, [(0, 0), (4, 4)])):
            x = zero()
            _put(x, stones)
            add(f"dirty{nd}", x, nd)
        # nearly full: every token reached, 15 tiles
        x = zero()
        u = rng.rand(R, Cc)
        x[0], x[1] = u < 0.48, (u >= 0.48) & (u < 0.96)
        add("nearly-full", x.astype(np.float32), R * Cc)
        # both sides to move: the same position seen by either player (the canonical planes swap)
        x = _random(rng, R, Cc, planes, 30, 30)
        add("side0", x)
        add("side1", np.ascontiguousarray(x[::-1]))
        for i in range(20):
            add(f"random{i}", _random(rng, R, Cc, planes, 5, 60))
    else:
        hi = R * Cc
        corners = [(0, 0), (0, Cc - 1), (R - 1, 0), (R - 1, Cc - 1), (0, Cc // 2), (R // 2, 0), (R - 1, Cc // 2), (R // 2, Cc - 1)]
        for r, c in corners:
            x = zero()
            x[0, r, c] = 1.0
            add(f"stone{r}{c}", x)
        if planes == 3:
            x = zero()
            x[2] = 1.0
            add("empty-side1", x)
        x = _random(rng, R, Cc, planes, hi - 1, hi - 1)
        add("nearly-full", x)
        x = _random(rng, R, Cc, planes, hi // 2, hi // 2)
        add("side0", x)
        y = x.copy()
        y[0], y[1] = x[1], x[0]
        if planes == 3:
            y[2] = 1.0 - x[2]
        add("side1", y)
        for i in range(8):
            add(f"random{i}", _random(rng, R, Cc, planes, 1, hi - 2))
    return np.stack(boards), labels


def fold_tables(name, exact):
    """(azk.EmbedFoldTables, heads) of the seed-SEED network of this shape, from its float64 fold (PolicyValueNet.fold_u)."""
    import torch
    import azk
    from pvnet import NetConfig, PolicyValueNet
    R, Cc, planes, k = CONFIGS[name]
    cfg = NetConfig(R, Cc, planes, R * Cc, k, 512, 8, 1)
    net = PolicyValueNet(cfg, seed=SEED, device="cuda", dtype=torch.float32, path="full")
    r = net.fold_u()
    assert r is not None, name
    return azk.EmbedFoldTables(r, 8, k, 512, "cuda", exact=exact)


def run_rows(name, boards, tables, exact, grid=0):
    """The kernel's rows of the set [n, 8, EMBED_FOLD_ROW] as a host array (bf16 rows as their uint16 words), with the grid capped
    at `grid` workgroups (0: the default); the cap is reset afterwards.  Also the board queue's words after the launch."""
    import torch
    import azk
    R, Cc, planes, k = CONFIGS[name]
    x = torch.from_numpy(boards).cuda().to(torch.bfloat16).contiguous()
    sched = azk.new_sched("cuda")
    assert azk.lib().azk_nn_embed_fold_grid(grid) == 0
    try:
        rows = (azk.nnx_embed_fold if exact else azk.nn_embed_fold)(x, tables, R, Cc, sched)
        torch.cuda.synchronize()
    finally:
        assert azk.lib().azk_nn_embed_fold_grid(0) == 0
    host = rows.cpu().numpy() if exact else rows.view(torch.int16).cpu().numpy().view(np.uint16)
    return np.ascontiguousarray(host), sched.tolist()


def digests(host_rows):
    """One sha256 per board over the bytes of its [8][EMBED_FOLD_ROW] row."""
    return np.array([hashlib.sha256(host_rows[b].tobytes()).hexdigest() for b in range(host_rows.shape[0])])


def key(name, exact):
    return f"{name}_{'f32' if exact else 'bf16'}"
