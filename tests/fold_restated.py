"""k_embed_fold (csrc/azk_nn.hip, through azk.nn_embed_fold and its float32-accurate EX form azk.nnx_embed_fold) restated on the CPU.
Test infrastructure: no GPU, no libazk.

  * SHAPES: the sixteen (rows, cols, planes, ksize) the pinned tests run at, each with what it is the edge of.
  * `patch_bits`: the patch layout in plain loops; `front_emulate`: the kernel's own route to the same bits (row words with two margin
    bits, one shift per token, a row mask), taking one deliberate mistake; `canonical_planes`: an engine leaf's cell codes as planes.
  * `fold_f64`: the fold's formulas in float64 from any table dict, with eps as an argument -> what the kernel emits before rounding.
  * probes (`probe_tables`, `probe_boards`, `probe_expected`, `probe_window`): tables under which the kernel's float32 arithmetic is exact
    in any order, the boards they run on, the closed-form expected values from the plain-loop layout, and the window of output values a
    correct kernel may store (a single value wherever the expected value is one the output format holds).
  * `bound`: the entrywise error a correct kernel meets on real tables, each term derived where it is computed.
  * `fold_f32`: a numpy float32 evaluation from tables split into fp16 hi + lo as azk.EmbedFoldTables splits them, output rounded once,
    taking one deliberate mistake.

Unit roundoffs: float32 U32 = 2^-24, bf16 U16 = 2^-8 (eight significant bits); v_rsq_f32 / v_rcp_f32 / v_exp_f32 one ulp = 2 U32."""
import functools

import numpy as np
import torch

U32, U16 = 2.0 ** -24, 2.0 ** -8
D, H, KP, ROW = 512, 8, 64, 384
SENTINEL = 3.0
FORMS = ("bf16", "f32")
KINDS = ("selection", "count", "count2", "diagonal")
FRONT_MUTATIONS = ("swap_rc", "shift1", "rowmask_cols")
F32_MUTATIONS = ("drop_lo", "drop_wave_L")

# (rows, cols, planes, ksize): what it is the edge of.  PolicyValueNet.fold_u() gives tables for every one of them at seed 6.
SHAPES = {
    (15, 15, 2, 5): "the benched shape: 15 tiles, the plane seam one bit into a dword",
    (7, 7, 2, 3): "Gomoku's smallest shipped board, 3 x 3 patches: patch bits 0..17, three full tiles and one token",
    (3, 3, 3, 3): "tic-tac-toe: three planes, T = 10 inside one tile",
    (6, 7, 3, 3): "Connect4's own shape: three planes, rows != cols, 42 + 1 tokens",
    (14, 18, 2, 5): "rows < cols at the largest token count, T + 3 = 256: every thread has a role, the 1 / L threads are the last three",
    (15, 16, 2, 5): "rows != cols by one: rdivR / rdivC differ in the last place only",
    (9, 28, 2, 5): "cols = 28: the row word with its margins fills all 32 bits; T + 3 = 256; 504 cells, the fast loads' last board size",
    (28, 9, 2, 5): "rows = 28 > cols: channels * rows = 56 row-word lanes, the transposed partner of 9 x 28",
    (1, 1, 2, 3): "one cell: a board smaller than its patch, T = 2, one token in the one tile",
    (1, 2, 2, 5): "one row of two: every patch clipped on all four sides",
    (2, 2, 2, 5): "2 x 2 under a 5 x 5 patch: the board lies inside every token's patch",
    (1, 28, 2, 5): "a single row at cols = 28: rdivR = 65537, one row-word lane per plane",
    (5, 5, 2, 5): "the board is exactly one patch: T = 26, two tiles with six null tokens",
    (21, 3, 3, 3): "channels * rows = 63: one lane short of a full wave of row words; T = 64",
    (21, 12, 3, 3): "756 cells > 512: the general board loop; channels * rows = 63; T + 3 = 256",
    (9, 28, 3, 3): "756 cells > 512 at cols = 28: the general board loop with full row words; T + 3 = 256",
}


def tokens(shape):
    return shape[0] * shape[1] + 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the patch layout
# ---------------------------------------------------------------------------------------------------------------------------------
def patch_bits(boards, k):
    """boards [n, C, R, Cc] of 0 / 1 -> P float64 [n, T, 64].  Token t = 1 + r Cc + c; patch bit p = ch k k + ky k + kx is cell
    (r + ky - k // 2, c + kx - k // 2) of plane ch, zero off the board; token 0 has an empty patch.  Plain loops over everything but n."""
    b = np.asarray(boards, np.float64)
    n, C, R, Cc = b.shape
    pad = k // 2
    P = np.zeros((n, R * Cc + 1, KP))
    for r in range(R):
        for c in range(Cc):
            t = 1 + r * Cc + c
            for ch in range(C):
                for ky in range(k):
                    for kx in range(k):
                        rr, cc = r + ky - pad, c + kx - pad
                        if 0 <= rr < R and 0 <= cc < Cc:
                            P[:, t, ch * k * k + ky * k + kx] = b[:, ch, rr, cc]
    return P


def front_emulate(board, k, mutate=None):
    """One board [C, R, Cc] -> P [T, 64] the way the kernel gets there: plane ch's row r as a word with the cells at bits 2 .. Cc + 1,
    thread tv's token coordinate from tj = tv - 1 by tr = tj / Cc, tc = tj - tr Cc, its k bits of row tr + ky - pad by one shift
    (tc + 2 - pad, a 5-bit shift amount as the hardware takes it) under a row mask (0 <= row < R; the row read is clamped).
    mutate: 'swap_rc' (tr = tj / R), 'shift1' (the shift one more), 'rowmask_cols' (the row tested against Cc)."""
    assert mutate is None or mutate in FRONT_MUTATIONS
    C, R, Cc = board.shape
    pad, T = k // 2, R * Cc + 1
    assert Cc <= 28 and k <= 5 and C * R <= 64
    roww = [[sum(int(board[ch, r, c] != 0) << (c + 2) for c in range(Cc)) for r in range(R)] for ch in range(C)]
    P = np.zeros((T, KP))
    for tv in range(1, T):
        tj = tv - 1
        tr = tj // (R if mutate == "swap_rc" else Cc)
        tc = tj - tr * Cc
        sh = (tc + 2 - pad + (1 if mutate == "shift1" else 0)) & 31
        for ch in range(C):
            for ky in range(k):
                rr = tr + ky - pad
                if not 0 <= rr < (Cc if mutate == "rowmask_cols" else R):
                    continue
                bits = (roww[ch][min(max(rr, 0), R - 1)] >> sh) & ((1 << k) - 1)
                for kx in range(k):
                    P[tv, ch * k * k + ky * k + kx] = (bits >> kx) & 1
    return P


def canonical_planes(cells, player, planes, mutate=None):
    """An engine leaf as the evaluator sees it: cells [rc] of codes (bit 0: a stone of side 0, bit 1: of side 1), `player` the side to
    move at the leaf -> [planes, rc] of 0 / 1.  Plane ch < 2 is bit ch ^ player of the code (the mover's stones first); the third plane
    is the side to move everywhere.  mutate 'plane_pick': element e >= 2 rc taken for plane 1 (the general loop's pick without its
    second term)."""
    cells = np.asarray(cells).astype(np.int64)
    out = np.zeros((planes, cells.shape[-1]))
    for ch in range(planes):
        if ch == 2 and mutate != "plane_pick":
            out[ch] = float(player != 0)
        else:
            out[ch] = (cells >> (min(ch, 1) ^ player)) & 1
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# the formulas in float64
# ---------------------------------------------------------------------------------------------------------------------------------
def _f8(r, key):
    return torch.as_tensor(r[key]).detach().cpu().double()


def fold_f64(r, P, eps):
    """r: a table dict as PolicyValueNet.fold_u returns it (G [64, 64], ext [64, 16], U2 [T, 64], nt [T], sct [T, H], rstdc [T], ref [H],
    wc [T, H], lall [H]); P [n, T, 64] patch bits.  What the kernel emits before rounding - bw [n, H, T] token weights (a - ac) / L on
    the tokens some stone reaches and 0 elsewhere (the kernel never evaluates the others; in exact arithmetic their a equals ac),
    inv [n, H] = 1 / L with L = l_all + sum over the reached tokens of (w - wc), pw [n, H, 64] pooled patch / L - and the
    intermediates `bound` needs."""
    P = torch.as_tensor(P).double()
    G, ext, U2, nt, sct = _f8(r, "G"), _f8(r, "ext")[:, :H], _f8(r, "U2"), _f8(r, "nt"), _f8(r, "sct")
    rstdc, ref, wc, lall = _f8(r, "rstdc"), _f8(r, "ref"), _f8(r, "wc"), _f8(r, "lall")
    dirty = P.sum(2) > 0                                                                 # [n, T]
    dm = dirty.double()[..., None]
    quad = torch.einsum("ntk,kl,ntl->nt", P, G, P)
    cross = (P * U2[None]).sum(2)
    var = ((quad + cross + nt[None]) / D).clamp_min(0.0) + eps
    var = torch.where(dirty, var, torch.ones_like(var))                                 # (the kernel never evaluates an unreached token)
    rstd = 1.0 / torch.sqrt(var)
    e = P @ ext + sct[None]                                                              # [n, T, H]
    x = rstd[..., None] * e - ref[None, None]
    w = torch.exp(x)
    a = w * rstd[..., None]
    ac = wc * rstdc[:, None]
    L = lall[None] + ((w - wc[None]) * dm).sum(1)                                        # [n, H]
    bw = ((a - ac[None]) * dm / L[:, None, :]).transpose(1, 2)
    pw = torch.einsum("nth,ntk->nhk", a * dm, P) / L[..., None]
    return dict(bw=bw, inv=1.0 / L, pw=pw, P=P, dirty=dirty, var=var, rstd=rstd, e=e, x=x, w=w, a=a, ac=ac, L=L)


def row_image(o, T, form):
    """The [n, H, 384] output row as float64: token weights at [0, T), 1 / L at T (bf16 rows: its bf16 value at T and T + 2, the
    remainder at T + 1 - here the unrounded 1 / L at T and T + 2 and 0 at T + 1: `check_rows` treats the three slots by name), pooled
    patch at [256, 320), zero elsewhere."""
    n = o["bw"].shape[0]
    img = torch.zeros(n, H, ROW, dtype=torch.float64)
    img[:, :, :T] = o["bw"]
    img[:, :, T] = o["inv"]
    if form == "bf16":
        img[:, :, T + 2] = o["inv"]
    img[:, :, 256:320] = o["pw"]
    return img


# ---------------------------------------------------------------------------------------------------------------------------------
# rounding helpers
# ---------------------------------------------------------------------------------------------------------------------------------
def bf16_rne(x):
    """float array -> the float64 value of its bf16 rounding, by the integer arithmetic of the kernel's bf16_rne on the float32 bits."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = ((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def half_ulp(x, form):
    """Half an ulp of the output format at |x| (float64 array): 2^(floor(log2 |x|) - p) with p = 8 significant bits (bf16) or 24."""
    x = np.abs(np.asarray(x, np.float64))
    ex = np.floor(np.log2(np.maximum(x, 2.0 ** -126)))
    return np.where(x > 0, 2.0 ** (ex - (8 if form == "bf16" else 24)), 0.0)


def decode(rows, form):
    """The kernel's rows (a torch tensor, bf16 or float32, any device) -> float64 numpy [n, H, 384]."""
    return rows.detach().cpu().double().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------
# exact probes
# ---------------------------------------------------------------------------------------------------------------------------------
def probe_tables(kind, shape):
    """Synthetic table dict for azk.EmbedFoldTables(r, 8, k, 512, dev, eps=0.0).  In every kind G' = U2 = ext = sct = ref = 0 except as
    stated, rstdc = 0 (so ac = 0 and the weight entry is a / L itself), the score is 0 and w = exp(0) = 1.
      selection: wc = 1, lall[h] = 2^h, nt[t] = 512 * 4^-(t mod 4): var = 4^-j, rstd = a = 2^j with j = t mod 4, L = 2^h.
      count:     the same with nt = 512: a = 1.
      count2:    count with wc = lall = 1 / 2: L = (nd + 1) / 2 counts the reached tokens.
      diagonal:  selection's wc and lall, nt = 0, G[k][k] = 512 * 4^-(k mod 4): a token whose patch is the single bit k has rstd = 2^(k mod 4).
    Every table entry is a power of two (or 0): exact in float32 and in the fp16 hi term at any power-of-two scale, lo = 0."""
    assert kind in KINDS
    T = tokens(shape)
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    t = torch.arange(T, dtype=torch.float64)
    r = dict(G=z(KP, KP), ext=z(KP, 16), U2=z(T, KP), nt=z(T), sct=z(T, H), Dtab=z(T, D), M=z(D, KP), rstdc=z(T), ref=z(H),
             wc=torch.ones(T, H, dtype=torch.float64), uall=z(D), lall=2.0 ** torch.arange(H, dtype=torch.float64), kreal=shape[2] * shape[3] ** 2)
    if kind == "selection":
        r["nt"] = 512.0 * 4.0 ** -(t % 4)
    elif kind in ("count", "count2"):
        r["nt"] = torch.full((T,), 512.0, dtype=torch.float64)
        if kind == "count2":
            r["wc"], r["lall"] = r["wc"] * 0.5, torch.full((H,), 0.5, dtype=torch.float64)
    else:
        kk = torch.arange(KP, dtype=torch.float64)
        r["G"] = torch.diag(512.0 * 4.0 ** -(kk % 4))
    return r


def _one_stone(shape, plane_list):
    R, Cc, C, k = shape
    out = []
    for ch in plane_list:
        for cell in range(R * Cc):
            x = np.zeros((C, R, Cc), np.float32)
            x[ch, cell // Cc, cell % Cc] = 1.0
            out.append(x)
    return out


def stone_boards(shape, seed, count, lo=0.0, hi=1.0):
    """`count` random boards, each with its own stone density in [lo, hi] of the cells, stones alternating between the two stone planes,
    the side plane (three planes) drawn 0 or 1."""
    R, Cc, C, k = shape
    rng = np.random.RandomState(seed)
    out = []
    for i in range(count):
        x = np.zeros((C, R, Cc), np.float32)
        m = int(round((lo + (hi - lo) * rng.rand()) * R * Cc))
        for j, cell in enumerate(rng.choice(R * Cc, size=m, replace=False)):
            x[j & 1, cell // Cc, cell % Cc] = 1.0
        if C == 3:
            x[2] = float(rng.randint(2))
        out.append(x)
    return out


def fixed_boards(shape):
    """empty, full (plane 0 everywhere; side plane 1), checkerboard over the two stone planes (side plane 0)."""
    R, Cc, C, k = shape
    empty, full, chk = (np.zeros((C, R, Cc), np.float32) for _ in range(3))
    full[0] = 1.0
    if C == 3:
        full[2] = 1.0
    par = (np.arange(R)[:, None] + np.arange(Cc)[None, :]) & 1
    chk[0], chk[1] = par == 0, par == 1
    return [empty, full, chk]


def probe_boards(kind, shape):
    """float32 [n, C, R, Cc].  selection: a stone at every cell of every stone plane - for three planes once with the side plane 0 and
    once with it 1 - and the empty board.  diagonal: one set cell at every cell of EVERY plane (the third included: the batch entry
    point takes any 0 / 1 planes), so every token's patch is a single bit and every bit position occurs.  count, count2: empty, full,
    checkerboard, the one-stone boards thinned to every fifth, two- to four-stone boards and 24 random boards of every density."""
    R, Cc, C, k = shape
    if kind == "selection":
        b = _one_stone(shape, (0, 1))
        if C == 3:
            b = b + [np.concatenate([x[:2], np.ones((1, R, Cc), np.float32)]) for x in b]
        b.append(np.zeros((C, R, Cc), np.float32))
    elif kind == "diagonal":
        b = _one_stone(shape, range(C))
    else:
        b = fixed_boards(shape) + _one_stone(shape, (0, 1))[::5] + stone_boards(shape, 11, 24)
        rng = np.random.RandomState(12)
        for m in (2, 3, 4, 2, 3, 4):
            x = np.zeros((C, R, Cc), np.float32)
            for j, cell in enumerate(rng.choice(R * Cc, size=min(m, R * Cc), replace=False)):
                x[j & 1, cell // Cc, cell % Cc] = 1.0
            b.append(x)
    return np.stack(b)


def probe_expected(kind, shape, boards):
    """The closed form, from the plain-loop layout alone: dict(bw [n, H, T], inv [n, H], pw [n, H, 64]) float64 numpy.
    With a_t the token's a (selection: 2^(t mod 4); count: 1; diagonal: 2^(k mod 4) for its single bit k) and reached_t = the patch is
    not empty: bw = reached_t a_t / L, pw[k] = sum_t a_t P[t][k] / L, L = 2^h (count2: (number reached + 1) / 2 for every head)."""
    P = patch_bits(boards, shape[3])
    n, T, _ = P.shape
    reached = P.sum(2) > 0
    if kind == "selection":
        a = np.broadcast_to(2.0 ** (np.arange(T) % 4), (n, T))
    elif kind == "diagonal":
        assert (P.sum(2) <= 1).all()                              # one bit per patch
        a = (P * 2.0 ** (np.arange(KP) % 4)).sum(2)
    else:
        a = np.ones((n, T))
    a = a * reached
    if kind == "count2":
        L = np.repeat(((reached.sum(1) + 1) / 2.0)[:, None], H, 1)
    else:
        L = np.broadcast_to(2.0 ** np.arange(H), (n, H))
    bw = a[:, None, :] / L[:, :, None]
    pw = np.einsum("nt,ntk->nk", a, P)[:, None, :] / L[:, :, None]
    return dict(bw=bw, inv=1.0 / L, pw=pw, a=a, L=np.ascontiguousarray(L), count=np.einsum("nt,ntk->nk", a, P))


# What a correct kernel may store for an exact-probe value x.  Every operand and every sum of the probes is exact in float32 (shown by
# test_fold_restated: all are dyadic with few bits), so the float32 value in front of the output rounding is x (1 + d) where d collects
# only the hardware approximations: v_rsq_f32 on var (<= 1 ulp = 2^-23), v_rcp_f32 on L (2^-23), the product a * (1 / L) and the
# bf16 remainder of a (2^-24, 2^-16 * 2^-23): |d| < 2^-21.  Windows are taken at 2^-20.
#   EX rows: sqrtf, the two divisions and exp_acc(0) = 1 are exact at these arguments (d = 0), and x is a float32 number: one value -
#   except count2, where 1 / L is one IEEE division and every entry is that quotient times an exact integer: restated in numpy float32.
#   bf16 rows: the stored value lies between the bf16 roundings of x (1 - 2^-20) and x (1 + 2^-20).  Where x is a bf16 number (every
#   power of two, every integer up to 256 over a power of two) both are x: one value.  Elsewhere - sums over the side plane in the
#   selection probe, quotients in count2 - the window is one value unless x lies within 2^-20 of a bf16 tie, then the two neighbours.
#   The 1 / L remainder slot holds bf16(inv - bf16(inv)): 0 when v_rcp is exact, at most 2^-23 / L in size otherwise; count2's is held to
#   the derived sum bound instead (`inv_sum_bound`).
WINDOW = 2.0 ** -20


def probe_window(kind, shape, e, form):
    """(lo, hi): float64 [n, H, 384] bounds of every output entry, lo == hi wherever the bits are known."""
    T = tokens(shape)
    n = e["bw"].shape[0]
    lo, hi = np.zeros((n, H, ROW)), np.zeros((n, H, ROW))
    if form == "f32":
        if kind == "count2":
            inv = (np.float32(1.0) / e["L"].astype(np.float32))
            bw = (e["a"].astype(np.float32)[:, None, :] * inv[:, :, None]).astype(np.float64)
            pw = (e["count"].astype(np.float32)[:, None, :] * inv[:, :, None]).astype(np.float64)
            inv = inv.astype(np.float64)
        else:
            bw, pw, inv = e["bw"], e["pw"], e["inv"]
        for img in (lo, hi):
            img[:, :, :T], img[:, :, T], img[:, :, 256:320] = bw, inv, pw
        return lo, hi
    for img, f in ((lo, 1.0 - WINDOW), (hi, 1.0 + WINDOW)):
        img[:, :, :T], img[:, :, 256:320] = bf16_rne(e["bw"] * f), bf16_rne(e["pw"] * f)
        img[:, :, T] = img[:, :, T + 2] = bf16_rne(e["inv"] * f)
    rem = 2.0 ** -23 * e["inv"]
    if kind == "count2":                                       # any remainder a bf16 split can leave; the sum is checked on its own
        rem = U16 * e["inv"] * (1 + WINDOW)
    lo[:, :, T + 1], hi[:, :, T + 1] = -rem, rem
    return lo, hi


def inv_sum_bound(inv):
    """bf16 rows: |(slot T + slot T + 1) - 1 / L| <=.  v_rcp_f32 is within one ulp, 2^-23 relative; inv - bf16(inv) is exact in float32 (both
    lie on inv's grid and differ by at most half a bf16 ulp, 2^-8 |inv|); rounding that remainder to bf16 costs at most 2^-8 of it:
    (2^-23 + 2^-16 (1 + 2^-23)) / L."""
    return (2.0 ** -23 + 2.0 ** -16 * (1 + 2.0 ** -23)) * np.abs(inv)


def in_window(got, lo, hi):
    """-> indices of the entries outside [lo, hi] (empty when the rows pass)."""
    return np.argwhere(~((got >= lo) & (got <= hi)))


# ---------------------------------------------------------------------------------------------------------------------------------
# the float64 bound for real tables
# ---------------------------------------------------------------------------------------------------------------------------------
def table_scale(t):
    """azk.EmbedFoldTables' power-of-two scale: the largest entry's hi term near 2^10."""
    import math
    return 2.0 ** (10 - math.ceil(math.log2(max(float(torch.as_tensor(t).abs().max()), 1e-30))))


def split_fp16(x64, scale):
    """As azk.split_fp16: two round-to-nearest steps."""
    xs = torch.as_tensor(x64).double() * float(scale)
    hi = xs.to(torch.float16)
    lo = (xs - hi.double()).to(torch.float16)
    return hi, lo


def bound(r, o, eps, form):
    """The entrywise error bound of a correct kernel against fold_f64's `o` on tables `r`: dict(bw, inv_hi, inv_sum, pw), float64 numpy.
    u = U32.  Every count below is of the kernel's source (k_embed_fold); zero products add exactly, so chains count set bits only.
    With nb = the set bits of the token's patch:

    D var.  The table split: (hi + lo) / scale is the entry to 2^-22 relative, or to half an fp16 subnormal step 2^-25 / scale where
      lo is subnormal: per product 2^-22 |G_kl| + 2^-25 / gs, over the nb^2 products.  The products themselves are exact (0 / 1 against
      fp16).  Sums: a column of Y chains 2 nb non-zero products (hi and lo) through its four MFMAs; the four fma over q, one fma that
      joins the cross term (itself four fma on float32-rounded U2: 1 + 4), four DPP additions: (2 nb + 14) u (S_G + S_U) with S_G, S_U
      the sums of the terms' magnitudes.  n_t is rounded to float32 (u |n_t|), added (u), scaled by 1 / D (exact), eps added (u):
      dvar = [2^-22 S_G + nb^2 2^-25 / gs + (2 nb + 14) u (S_G + S_U) + u |n_t|] / D + 2 u var.
    rstd.  d rstd / rstd = dvar / (2 var) (1 + dvar / var) + 2 u: v_rsq_f32 within one ulp = 2 u; EX: sqrtf and the division, u each.
    e.  As Y with one column: 2^-22 S_E + nb 2^-25 / es + (2 nb + 2) u (S_E + |sct|), sct rounded to float32 included.
    x = rstd e - ref.  |rstd e| (d rstd / rstd + u) + rstd de + u |ref| (the table) + u |x|.
    w = exp(x).  dw / w = expm1(dx) + rho; rho = (2.5 |x| + 2) u for __expf - DESIGN.md, "What pins the fp16-plane tail links": the product
      with log2(e) rounded twice and carried through the exponential, plus v_exp_f32's ulp; EX (exp_acc): the argument's rounding is
      carried as lo and corrected to first order, leaving v_exp_f32's ulp (2 u), the final fma (u) and the rounding of lo ln 2 (below
      u): 4 u.  Results below 2^-126 are flushed: an absolute 2^-126.
    a = w rstd: da / a = dw / w + d rstd / rstd + u.
    b = a - wc rstdc: da + 3 u |ac| (two float32 tables, one product) + u |b|.
    L = l_all + sum (w - wc): every term dw + u |wc| + u |w - wc|; a lane adds at most 64 of them in turn, two shuffles, four waves,
      l_all (float32: u |l_all|): 72 u (sum |w - wc| + |l_all|).
    1 / L: d inv / inv = dL / L (1 + dL / L) + 2 u (v_rcp_f32 one ulp; EX: one division).
    bw = b inv: db / L + |bw| (d inv / inv + u), then the output rounding: half an ulp of the format at |ref| + that error.
    pw = (sum_t a_t p_tk) inv: sum da_t; bf16 rows carry a as bf16 hi + bf16 remainder: 2^-16 a_t; the MFMA chain over the cnt_k
      tokens that hold bit k (two k-slots each), four waves: (2 cnt_k + 4) u sum a_t p_tk; then d inv / inv + u, then the output rounding.
    1 / L slots: float32 rows and the bf16 hi slot: d inv + half an ulp; bf16 hi + remainder: d inv + 2^-16 |inv| (inv_sum_bound's rounding)."""
    u = U32
    P, dirty = o["P"], o["dirty"]
    dm = dirty.double()
    Ga, exta, U2a = _f8(r, "G").abs(), _f8(r, "ext")[:, :H].abs(), _f8(r, "U2").abs()
    nt, sct, ref, wc, lall = _f8(r, "nt"), _f8(r, "sct"), _f8(r, "ref"), _f8(r, "wc"), _f8(r, "lall")
    gs, es = table_scale(r["G"]), table_scale(r["ext"])
    nb = P.sum(2)                                                                       # [n, T]
    SG = torch.einsum("ntk,kl,ntl->nt", P, Ga, P)
    SU = (P * U2a[None]).sum(2)
    var, rstd, e, x, w, a, L = o["var"], o["rstd"], o["e"], o["x"], o["w"], o["a"], o["L"]
    dvar = (2.0 ** -22 * SG + nb * nb * 2.0 ** -25 / gs + (2 * nb + 14) * u * (SG + SU) + u * nt.abs()[None]) / D + 2 * u * var
    rr = dvar / (2 * var) * (1 + dvar / var) + 2 * u                                    # d rstd / rstd [n, T]
    SE = P @ exta
    de = 2.0 ** -22 * SE + (nb * 2.0 ** -25 / es)[..., None] + (2 * nb + 2)[..., None] * u * (SE + sct.abs()[None])
    dx = (rstd[..., None] * e).abs() * (rr[..., None] + u) + rstd[..., None] * de + u * ref.abs()[None, None] + u * x.abs()
    rho = 4 * u if form == "f32" else (2.5 * x.abs() + 2) * u
    dw = w * (torch.expm1(dx) + rho) + 2.0 ** -126
    da = a * (dw / w + rr[..., None] + u)
    ac = o["ac"]
    b = a - ac[None]
    db = da + 3 * u * ac.abs()[None] + u * b.abs()
    wd = (w - wc[None]).abs()
    dL = ((dw + u * wc.abs()[None] + u * wd) * dm[..., None]).sum(1) + 72 * u * ((wd * dm[..., None]).sum(1) + lall.abs()[None]) + u * lall.abs()[None]
    ri = dL / L.abs() * (1 + dL / L.abs()) + 2 * u                                      # d inv / inv [n, H]
    inv = o["inv"].abs()
    f_bw = ((db * dm[..., None]) / L.abs()[:, None, :]).transpose(1, 2) + o["bw"].abs() * (ri[..., None] + u)
    apk = torch.einsum("nth,ntk->nhk", a * dm[..., None], P)
    cnt = torch.einsum("nt,ntk->nk", dm, P)[:, None, :]
    f_pw = (torch.einsum("nth,ntk->nhk", (da + (2.0 ** -16 * a if form == "bf16" else 0.0)) * dm[..., None], P) + (2 * cnt + 4) * u * apk) / L.abs()[..., None]
    f_pw = f_pw + o["pw"].abs() * (ri[..., None] + u)
    f_inv = inv * ri
    rnd = lambda ref_, f: f.numpy() + half_ulp(ref_.abs().numpy() + f.numpy(), form)
    return dict(bw=rnd(o["bw"], f_bw), pw=rnd(o["pw"], f_pw), inv_hi=rnd(o["inv"], f_inv),
                inv_sum=(f_inv + 2.0 ** -16 * (1 + 2.0 ** -23) * inv).numpy())


def check_rows(got, o, bd, T, form):
    """got: float64 [n, H, 384] decoded rows.  -> largest error / bound over EVERY entry of the three blocks and the 1 / L slots; the zero
    columns ([T + 3, 256) and [320, 384); float32 rows also T + 1 and T + 2) are asserted zero here."""
    worst = 0.0
    ratio = lambda err, b_: float(np.max(np.where(err == 0, 0.0, err / np.maximum(b_, 1e-300)))) if err.size else 0.0
    worst = max(worst, ratio(np.abs(got[:, :, :T] - o["bw"].numpy()), bd["bw"]))
    worst = max(worst, ratio(np.abs(got[:, :, 256:320] - o["pw"].numpy()), bd["pw"]))
    inv = o["inv"].numpy()
    worst = max(worst, ratio(np.abs(got[:, :, T] - inv), bd["inv_hi"]))
    if form == "bf16":
        assert np.array_equal(got[:, :, T], got[:, :, T + 2])
        worst = max(worst, ratio(np.abs(got[:, :, T] + got[:, :, T + 1] - inv), bd["inv_sum"]))
        assert not got[:, :, T + 3:256].any() and not got[:, :, 320:].any()
    else:
        assert not got[:, :, T + 1:256].any() and not got[:, :, 320:].any()
    return worst


# ---------------------------------------------------------------------------------------------------------------------------------
# the float32 restatement
# ---------------------------------------------------------------------------------------------------------------------------------
def fold_f32(r, P, eps, form, mutate=None):
    """The formulas in numpy float32 from the tables as the kernel holds them - G and ext as fp16 hi + lo at EmbedFoldTables' scales, the
    rest rounded to float32 - with the reached tokens compacted into 16-token tiles, tile i summed by wave i mod 4, and the output
    rounded once (bf16 rows: a as bf16 hi + remainder in the pooled patch, 1 / L as hi, remainder, hi).  -> float64 [n, H, 384].
    mutate: 'drop_lo' (the lo fragments never join), 'drop_wave_L' (wave 3's share of L never joins)."""
    assert mutate is None or mutate in F32_MUTATIONS
    f = np.float32
    P64 = np.asarray(torch.as_tensor(P).double().numpy())
    n, T, _ = P64.shape
    Pf = P64.astype(f)
    gs, es = table_scale(r["G"]), table_scale(r["ext"])
    ghi, glo = split_fp16(r["G"], gs)
    ehi, elo = split_fp16(_f8(r, "ext"), es)
    if mutate == "drop_lo":
        glo, elo = torch.zeros_like(glo), torch.zeros_like(elo)
    g32 = lambda t: t.float().numpy()
    tab = lambda key: _f8(r, key).numpy().astype(f)
    U2, nt, sct, rstdc, ref, wc, lall = (tab(k_) for k_ in ("U2", "nt", "sct", "rstdc", "ref", "wc", "lall"))
    Y = (Pf @ g32(ghi) + Pf @ g32(glo)).astype(f)                                       # exact products, float32 sums
    qd = ((Pf * Y).sum(2, dtype=f) * f(1.0 / gs) + (Pf * U2[None]).sum(2, dtype=f)).astype(f)
    dirty = P64.sum(2) > 0
    var = np.where(dirty, np.maximum((qd + nt[None]) * f(1.0 / D), f(0)) + f(eps), f(1)).astype(f)   # (unreached tokens are never evaluated)
    rstd = (f(1.0) / np.sqrt(var)).astype(f)
    e = ((Pf @ g32(ehi)[:, :H] + Pf @ g32(elo)[:, :H]) * f(1.0 / es) + sct[None]).astype(f)
    w = np.exp((rstd[..., None] * e - ref[None, None]).astype(f)).astype(f)
    a = (w * rstd[..., None]).astype(f)
    b = (a - wc[None] * rstdc[None, :, None]).astype(f)
    out = np.zeros((n, H, ROW))
    rnd = bf16_rne if form == "bf16" else (lambda v: np.asarray(v, f).astype(np.float64))
    for i in range(n):
        idx = np.nonzero(dirty[i])[0]
        wave = (np.arange(len(idx)) // 16) % 4
        Lw = [(w[i, idx[wave == v]] - wc[idx[wave == v]]).sum(0, dtype=f) for v in range(4)]
        if mutate == "drop_wave_L":
            Lw[3] = np.zeros(H, f)
        L = (((Lw[0] + Lw[1]) + (Lw[2] + Lw[3])) + lall).astype(f)
        inv = (f(1.0) / L).astype(f)
        ai = a[i, idx]
        if form == "bf16":
            hi = bf16_rne(ai).astype(f)
            ai = (hi + bf16_rne(ai - hi).astype(f)).astype(f)
        pw = np.stack([(ai[wave == v].T @ Pf[i, idx[wave == v]]).astype(f) for v in range(4)])
        pw = ((pw[0] + pw[1]) + (pw[2] + pw[3])).astype(f)
        out[i, :, idx] = rnd(b[i, idx] * inv[None])
        out[i, :, 256:320] = rnd(pw * inv[:, None])
        if form == "bf16":
            hi = bf16_rne(inv)
            out[i, :, T], out[i, :, T + 1], out[i, :, T + 2] = hi, bf16_rne(inv - hi.astype(f)), hi
        else:
            out[i, :, T] = inv
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# real tables, real boards
# ---------------------------------------------------------------------------------------------------------------------------------
SEED = 6


@functools.lru_cache(maxsize=None)
def real_tables(shape):
    """fold_u() of the seed-6 network of this shape, on the CPU in float64."""
    from pvnet import NetConfig, PolicyValueNet
    R, Cc, C, k = shape
    net = PolicyValueNet(NetConfig(R, Cc, C, R * Cc, k, 512, 8, 1), seed=SEED, device="cpu", dtype=torch.float32, path="full")
    r = net.fold_u()
    assert r is not None, shape                                   # the shape must reach k_embed_fold
    return net, r


def bound_boards(shape, random=40):
    """empty, full, checkerboard; the one-stone sweep thinned to every third cell; `random` random boards of every density; and, where the
    shape is one of fold_bits_common's three, that module's recorded set."""
    import fold_bits_common as fb
    b = fixed_boards(shape) + _one_stone(shape, (0, 1))[::3] + stone_boards(shape, 21, random)
    for name, cfg in fb.CONFIGS.items():
        if cfg == shape:
            b = b + list(fb.board_set(name)[0])
    return np.stack(b)
