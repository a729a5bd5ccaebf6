"""k_embed (token embedding, LayerNorm1, optional score columns) and k_cls_pool (softmax over tokens, weighted token sum), the two kernels
of csrc/azk_embed_tok.hip that open the "two-kernel" depth-1 path, called through azk.nn_patch_embed, azk.nn_patch_embed_scores and
azk.nn_cls_pool at small shapes and pinned two ways: probes whose float32 arithmetic is exact, so the output is known bit for bit (a
patch read back through an identity weight, an integer GEMM over every column, a selected row, a mean over 2^j rows), and float64
references with bounds derived from the number formats.  tests/embed_tok_restated.py states every probe and derivation;
tests/test_embed_tok_restated.py shows on the CPU which probe notices which deliberate mistake.  DESIGN.md, "What pins k_embed and
k_cls_pool", has the measured ratios.

Every output buffer carries 16 sentinel rows past its end, which must survive.  Each float64 test prints
`RATIO <name> <largest error / bound>` before it asserts."""
import math

import pytest
import torch

import embed_tok_restated as er

pytestmark = pytest.mark.gpu

SENTINEL = 7.0
PAD = 16
ERR_ARG = -1                      # include/azk.h AZK_ERR_ARG
HEADS = {128: 4, 256: 8, 512: 8}
EMBED_CASES = [(g, 128) for g in er.GEOMS] + [(g, D) for D in (256, 512) for g in er.WIDE_GEOMS]
GID = lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v)      # noqa: E731


def same(a, b):
    return torch.equal(er.bits(a.cpu()), er.bits(b.cpu()))


def first_diff(a, b):
    d = (er.bits(a.cpu()) != er.bits(b.cpu())).nonzero()
    return f"{d.shape[0]} elements differ, first at {d[0].tolist()}" if d.shape[0] else "equal"


def worst_ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 (an exact result where the bound is 0) and x / 0 = inf."""
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


def padded(n, T, D):
    buf = torch.full((n * T + PAD, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    return buf, buf[: n * T].view(n, T, D)


def pad_kept(buf, rows):
    return bool((buf[rows:].float() == SENTINEL).all())


def embed(boards, wt, cpos, ln_w, ln_b, geom, D, want_x, want_xhat):
    """azk.nn_patch_embed into padded buffers -> (x, xhat) on the CPU (None where not requested)."""
    import azk
    C, R, Cc, k = geom
    n, T = boards.shape[0], R * Cc + 1
    bx, vx = padded(n, T, D) if want_x else (None, None)
    bh, vh = padded(n, T, D) if want_xhat else (None, None)
    azk.nn_patch_embed(boards.cuda().contiguous(), wt.cuda().contiguous(), cpos.cuda(), ln_w.cuda(), ln_b.cuda(), R, Cc, k, D,
                       want_x=want_x, want_xhat=want_xhat, x_out=vx, xhat_out=vh)
    torch.cuda.synchronize()
    assert (bx is None or pad_kept(bx, n * T)) and (bh is None or pad_kept(bh, n * T)), "wrote past n T rows"
    return (None if vx is None else vx.cpu()), (None if vh is None else vh.cpu())


def embed_scores(boards, pr, geom, D, count=None):
    """azk.nn_patch_embed_scores into padded buffers -> (xhat [n, T, D], scores [n, H, Tp]) on the CPU."""
    import azk
    C, R, Cc, k = geom
    n, T, H = boards.shape[0], R * Cc + 1, pr["H"]
    bh, vh = padded(n, T, D)
    sc = torch.full((n * H * er.tp_of(T) + PAD,), SENTINEL, device="cuda")
    vs = sc[: n * H * er.tp_of(T)].view(n, H, er.tp_of(T))
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    azk.nn_patch_embed_scores(boards.cuda().contiguous(), pr["wt_ext"].cuda().contiguous(), pr["cpos"].cuda(), pr["mtab"].cuda(),
                              pr["msum"].cuda(), R, Cc, k, D, H, count=cnt, xhat=vh, scores=vs)
    torch.cuda.synchronize()
    assert pad_kept(bh, n * T) and bool((sc[n * H * er.tp_of(T):] == SENTINEL).all()), "wrote past its rows"
    return vh.cpu(), vs.cpu()


def boards_of(geom, seed=None):
    C, R, Cc, k = geom
    return er.probe_boards(C, R, Cc, seed=R * 31 + Cc if seed is None else seed)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_embed: exact probes
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,D", EMBED_CASES, ids=GID)
def test_embed_returns_the_patch_through_an_identity_weight(geom, D):
    """wt[p][p] = 1, cpos = 0: x[b, 1 + j, p] is bit p of token j's patch, so x[:, 1:, :C k^2] == F.unfold(board) exactly, the other
    columns and row 0 are 0.  Seven boards (empty, full, one colour, corners + last cell, three random), float32 and bf16."""
    C, R, Cc, k = geom
    boards = boards_of(geom)
    wt, cpos = er.identity_probe(C, R, Cc, k, D)
    want = er.identity_expected(boards, k, D)
    one = torch.ones(D)
    for b in (boards, boards.to(torch.bfloat16)):
        x, _ = embed(b, wt, cpos, one, one, geom, D, True, False)
        assert same(x, want), (b.dtype, first_diff(x, want))


@pytest.mark.parametrize("geom,D", EMBED_CASES, ids=GID)
def test_embed_integer_gemm_over_every_column(geom, D):
    """Weights in {-1, 0, 1} on all D rows, integer cpos in [-100, 100] on every row: x == unfold @ wt^T + cpos bit for bit (entries
    are integers <= 175), with x alone and with x + xhat requested.  This pins the permuted column map."""
    C, R, Cc, k = geom
    boards = boards_of(geom)
    pr = er.int_probe(C, R, Cc, k, D, HEADS[D], seed=R + Cc + D)
    want = er.int_expected_x(boards, pr).to(torch.bfloat16)
    wt = pr["wt_ext"][:D]
    for b in (boards, boards.to(torch.bfloat16)):
        x, _ = embed(b, wt, pr["cpos"], pr["ln_w"], pr["ln_b"], geom, D, True, False)
        assert same(x, want), (b.dtype, "x", first_diff(x, want))
        x, xh = embed(b, wt, pr["cpos"], pr["ln_w"], pr["ln_b"], geom, D, True, True)
        assert same(x, want), (b.dtype, "x + xhat", first_diff(x, want))


def test_embed_grid_stride_second_trip():
    """n = 16 388 one-cell boards (T = 2, D = 128): more than 4 096 workgroups x 4 waves of items, so four waves take a second item.
    The integer probe, bit for bit on every board; board b holds pattern b mod 4."""
    geom, D, n = (2, 1, 1, 3), 128, 16388
    boards = torch.zeros(n, 2, 1, 1)
    boards[:, 0, 0, 0] = (torch.arange(n) & 1).float()
    boards[:, 1, 0, 0] = ((torch.arange(n) >> 1) & 1).float()
    pr = er.int_probe(2, 1, 1, 3, D, 4, seed=11)
    want = er.int_expected_x(boards, pr).to(torch.bfloat16)
    for b in (boards, boards.to(torch.bfloat16)):
        x, _ = embed(b, pr["wt_ext"][:D], pr["cpos"], pr["ln_w"], pr["ln_b"], geom, D, True, False)
        assert same(x, want), (b.dtype, first_diff(x, want))


REFUSED = {
    "1985_cells": dict(C=2, R=31, Cc=33, k=3, kp=32, D=128),
    "kp_128": dict(C=2, R=7, Cc=7, k=7, kp=128, D=128),
    "even_k": dict(C=2, R=7, Cc=7, k=4, kp=32, D=128),
    "k_9": dict(C=1, R=7, Cc=7, k=9, kp=96, D=128),
    "D_384": dict(C=2, R=7, Cc=7, k=5, kp=64, D=384),
}


@pytest.mark.parametrize("case", sorted(REFUSED))
def test_embed_refuses_what_it_does_not_cover(case):
    """AZK_ERR_ARG and nothing launched (the output keeps its sentinel): a board of 1 985 cells or more, kp = 128, an even k, k = 9,
    D = 384.  Both entry points."""
    import azk
    a = REFUSED[case]
    n, T, D, H = 2, a["R"] * a["Cc"] + 1, a["D"], 4
    boards = torch.zeros(n, a["C"], a["R"], a["Cc"], device="cuda")
    wt = torch.zeros(D + 16, a["kp"], dtype=torch.bfloat16, device="cuda")
    cpos = torch.zeros(T, D, device="cuda")
    one = torch.ones(D, device="cuda")
    mtab, msum = torch.zeros(T, 16, device="cuda"), torch.zeros(16, device="cuda")
    x = torch.full((n, T, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    sc = torch.full((n, H, er.tp_of(T)), SENTINEL, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    L = azk.lib()
    rc = L.azk_nn_patch_embed(boards.data_ptr(), 1, wt.data_ptr(), cpos.data_ptr(), one.data_ptr(), one.data_ptr(), x.data_ptr(), None,
                              n, a["C"], a["R"], a["Cc"], a["k"], a["kp"], D, 1e-5, st)
    assert rc == ERR_ARG
    rc = L.azk_nn_patch_embed_scores(boards.data_ptr(), 1, wt.data_ptr(), cpos.data_ptr(), None, None, x.data_ptr(), mtab.data_ptr(),
                                     msum.data_ptr(), sc.data_ptr(), H, n, a["C"], a["R"], a["Cc"], a["k"], a["kp"], D, 1e-5, None, st)
    assert rc == ERR_ARG
    torch.cuda.synchronize()
    assert bool((x.float() == SENTINEL).all()) and bool((sc == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# k_embed: LayerNorm and score columns against float64
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom,D", EMBED_CASES + [((2, 15, 15, 5), "512h4"), ((3, 6, 7, 5), "128h8")], ids=GID)
def test_embed_layernorm_and_scores_on_the_integer_probe(geom, D):
    """On the integer probe the float32 tokens are known exactly, so LayerNorm and the scores are compared with float64 of those
    integers: xhat (affine form, and the score entry's plain normalised form) within half a bf16 ulp + the float32 term of
    embed_tok_restated.ln_bound; scores = rstd (x . m' - mean msum) within score_c(D) u32 |s| (everything before the product with rstd
    is exact).  Row D + 15 of the weight and column 15 of the score constants (the fused kernel's row-mean column) are set and must be
    unused: zeroing them changes no bit.
    Largest error / bound on an MI355X over all cases: xhat 0.9997 and the plain form 0.9996 (a float64 result next to a rounding
    boundary: half an ulp is the whole of it), scores 0.280."""
    H = HEADS[D] if isinstance(D, int) else int(D[-1])
    D = D if isinstance(D, int) else int(D[:3])
    C, R, Cc, k = geom
    boards = boards_of(geom)
    pr = er.int_probe(C, R, Cc, k, D, H, seed=R + Cc + D)
    xi = er.int_expected_x(boards, pr)
    _, xh = embed(boards, pr["wt_ext"][:D], pr["cpos"], pr["ln_w"], pr["ln_b"], geom, D, False, True)
    y, xw, kappa, _, _ = er.ln_rows_f64(xi, pr["ln_w"], pr["ln_b"])
    r_aff = worst_ratio((xh.double() - y).abs(), er.ln_bound(D, y, xw, kappa, pr["ln_w"], pr["ln_b"]))
    xn, sc = embed_scores(boards.to(torch.bfloat16), pr, geom, D)
    one, zero = torch.ones(D), torch.zeros(D)
    y, xw, kappa, _, _ = er.ln_rows_f64(xi, one, zero)
    r_xn = worst_ratio((xn.double() - y).abs(), er.ln_bound(D, y, xw, kappa, one, zero))
    s, _ = er.int_scores_f64(boards, pr, xi)
    T = R * Cc + 1
    r_s = worst_ratio((sc[:, :, :T].double() - s).abs(), er.score_c(D) * er.U32 * s.abs())
    print(f"RATIO embed_int_{GID(geom)}_D{D}_H{H} xhat {r_aff:.4f} xn {r_xn:.4f} scores {r_s:.4f}")
    assert r_aff <= 1.0 and r_xn <= 1.0 and r_s <= 1.0, (r_aff, r_xn, r_s)
    pr0 = dict(pr, wt_ext=pr["wt_ext"].clone(), mtab=pr["mtab"].clone())
    pr0["wt_ext"][D + 15] = 0
    pr0["mtab"][:, 15] = 0
    xn0, sc0 = embed_scores(boards.to(torch.bfloat16), pr0, geom, D)
    assert same(xn0, xn) and torch.equal(sc0, sc)


@pytest.mark.parametrize("D", (128, 256, 512))
def test_embed_constant_and_mean_100_rows(D):
    """Zero weights, so x = cpos exactly; rows t = 0 (mod 3) constant (variance 0: xhat = bf16(ln_b) exactly, the plain form 0, every
    score 0), t = 1 (mod 3) 100 + {-1, 0, 1}, the others random integers; all within the bounds of the integer probe.
    Largest error / bound on an MI355X: xhat 0.9987, the plain form 0.9981, scores 0.133."""
    geom = (2, 4, 5, 3)
    C, R, Cc, k = geom
    H, T = HEADS[D], R * Cc + 1
    boards = boards_of(geom)
    pr = er.int_probe(C, R, Cc, k, D, H, seed=D)
    pr["cpos"] = er.ln_case_probe(R, Cc, D)
    pr["wt_ext"] = torch.zeros_like(pr["wt_ext"])
    pr["mtab"] = torch.zeros_like(pr["mtab"])
    pr["mtab"][:, :H] = pr["cpos"] @ pr["mprime"].t()
    xi = pr["cpos"].expand(7, -1, -1).contiguous()
    x, xh = embed(boards, pr["wt_ext"][:D], pr["cpos"], pr["ln_w"], pr["ln_b"], geom, D, True, True)
    assert same(x, xi.to(torch.bfloat16))
    nconst = len(range(0, T, 3))
    assert same(xh[:, 0::3], pr["ln_b"].to(torch.bfloat16).expand(7, nconst, D).contiguous())
    y, xw, kappa, _, _ = er.ln_rows_f64(xi, pr["ln_w"], pr["ln_b"])
    r_aff = worst_ratio((xh.double() - y).abs(), er.ln_bound(D, y, xw, kappa, pr["ln_w"], pr["ln_b"]))
    xn, sc = embed_scores(boards, pr, geom, D)
    assert bool((xn[:, 0::3].float() == 0).all()) and bool((sc[:, :, 0:T:3] == 0).all())
    one, zero = torch.ones(D), torch.zeros(D)
    y, xw, kappa, mean, rstd = er.ln_rows_f64(xi, one, zero)
    r_xn = worst_ratio((xn.double() - y).abs(), er.ln_bound(D, y, xw, kappa, one, zero))
    s = er.scores_f64(xi, mean, rstd, pr["mtab"][:, :H].double().expand(7, -1, -1), pr["msum"][:H])
    r_s = worst_ratio((sc[:, :, :T].double() - s).abs(), er.score_c(D) * er.U32 * s.abs())
    print(f"RATIO embed_rows_D{D} xhat {r_aff:.4f} xn {r_xn:.4f} scores {r_s:.4f}")
    assert r_aff <= 1.0 and r_xn <= 1.0 and r_s <= 1.0, (r_aff, r_xn, r_s)


RAND_CASES = (((2, 7, 7, 5), 128, 4), ((3, 6, 7, 5), 256, 8), ((2, 16, 16, 5), 512, 8), ((2, 20, 20, 5), 128, 8), ((1, 8, 8, 7), 256, 4))


def check_against(ref, x, xh, xn, sc, T, tag):
    r = dict(x=worst_ratio((x.double() - ref["x"]).abs(), ref["x_bound"]),
             xn=worst_ratio((xn.double() - ref["xn"]).abs(), ref["xn_bound"]),
             scores=worst_ratio((sc[:, :, :T].double() - ref["s"]).abs(), ref["s_bound"]))
    if xh is not None:
        r["xhat"] = worst_ratio((xh.double() - ref["xhat"]).abs(), ref["xhat_bound"])
    print(f"RATIO {tag} " + " ".join(f"{k} {v:.4f}" for k, v in r.items()))
    assert max(r.values()) <= 1.0, r


@pytest.mark.parametrize("geom,D,H", RAND_CASES, ids=GID)
def test_embed_random_operands_within_the_float64_bounds(geom, D, H):
    """bf16-representable randn weights, cpos and score constants: x within 2^-8 |ref| + (C k^2 + 2) 2^-24 (|patch| |w| + |cpos|);
    xhat, the plain normalised tokens and the scores within the forms embed_tok_restated.embed_f64 derives from that.
    Largest error / bound on an MI355X: x 0.9953, xhat 0.9994, the plain form 0.9949 (each the final bf16 rounding), scores 0.011."""
    C, R, Cc, k = geom
    boards = boards_of(geom)
    pr = er.rand_probe(C, R, Cc, k, D, H, seed=D + R)
    ref = er.embed_f64(boards, pr["wt_ext"].float(), pr["cpos"], pr["mtab"], pr["msum"], k, D, H, pr["ln_w"], pr["ln_b"])
    x, xh = embed(boards, pr["wt_ext"][:D], pr["cpos"], pr["ln_w"], pr["ln_b"], geom, D, True, True)
    xn, sc = embed_scores(boards, pr, geom, D)
    check_against(ref, x, xh, xn, sc, R * Cc + 1, f"embed_rand_{GID(geom)}_D{D}_H{H}")


@pytest.mark.parametrize("R,D,H", ((7, 128, 4), (16, 256, 8)))
def test_embed_on_the_products_own_operands(R, D, H):
    """A depth-1 clsfold network's own _hip / _fold operands (7 x 7, D = 128, 4 heads; 16 x 16, D = 256, 8 heads; k = 5) against float64
    from the MASTER weights: tokens from the float32 conv weight and position table, the folded score vector m' = scale Wk_h^T q_h gamma
    recomputed in float64.  On top of the random case's bounds, the operands' own distance from the master:
      x       |patch| hulp(W) (the conv weight's rounding to bf16: half a bf16 ulp of each weight, between 2^-9 and 2^-8 of it - a
              patch with a single stone meets one weight's full half ulp, so the average figure 2^-9 |W| that serves for a sum over D
              terms is not a bound here) + u32 |cpos| (cpos is one float32 addition)
      scores  dm = (2 D + 16) u32 scale |Wk_h|^T (|Wq| |h0| + |bq|) |gamma| for m' evaluated in float32 (two dot products of length
              <= D and LayerNorm of the cls row); E = x . m' then carries |patch| hulp(m' W) (bf16 rounding of the score rows) +
              |patch| (dm |W| + (D + 2) u32 |m'| |W|) + |cpos| dm + (D + 2) u32 |cpos| |m'|, and mean msum carries
              |mean| (sum dm + (D + 2) u32 sum |m'|).
    Largest error / bound on an MI355X: x 0.9932, the normalised tokens 0.9950, scores 0.084 (7 x 7) and 0.036 (16 x 16)."""
    from pvnet import NetConfig, PolicyValueNet
    k, C = 5, 2
    geom = (C, R, R, k)
    net = PolicyValueNet(NetConfig(R, R, C, R * R, k, D, H, 1), seed=8, device="cuda", dtype=torch.bfloat16, path="clsfold")
    hp, f, m = net._hip, net._fold, net.master
    assert f is not None and "wt_ext" in f
    kreal, dh = C * k * k, D // H
    dd = lambda name: m[name].detach().cpu().double()      # noqa: E731
    W = dd("embedding.patch_embed.patch_embed.weight").reshape(D, kreal)
    cpos = dd("embedding.pos_embedding")[0].clone()
    cpos[0] += dd("embedding.cls_token")[0, 0]
    cpos[1:] += dd("embedding.patch_embed.patch_embed.bias")
    g, beta = dd("blocks.0.norm1.weight"), dd("blocks.0.norm1.bias")
    Wi, bi = dd("blocks.0.attn.in_proj_weight"), dd("blocks.0.attn.in_proj_bias")
    h0 = torch.nn.functional.layer_norm(cpos[0], (D,), g, beta, 1e-5)
    q = (Wi[:D] @ h0 + bi[:D]).view(H, dh)
    Wk = Wi[D:2 * D].view(H, dh, D)
    scale = 1.0 / math.sqrt(dh)
    mn = torch.einsum("he,hed->hd", q, Wk) * scale * g                                              # [H, D]
    qa = (Wi[:D].abs() @ h0.abs() + bi[:D].abs()).view(H, dh)
    dm = (2 * D + 16) * er.U32 * scale * torch.einsum("he,hed->hd", qa, Wk.abs()) * g.abs()
    boards = boards_of(geom)
    n = boards.shape[0]
    pz = torch.cat([torch.zeros(n, 1, kreal, dtype=torch.float64), er.unfold(boards, k).double()], 1)
    wt_ext = torch.zeros(D + 16, kreal, dtype=torch.float64)
    wt_ext[:D], wt_ext[D:D + H] = W, mn @ W
    mtab = torch.zeros(cpos.shape[0], 16, dtype=torch.float64)
    mtab[:, :H] = cpos @ mn.t()
    msum = torch.zeros(16, dtype=torch.float64)
    msum[:H] = mn.sum(1)
    extra_x = pz @ er.half_ulp_bf16(W).t() + er.U32 * cpos.abs()
    mean = (pz @ W.t() + cpos).mean(2, keepdim=True).abs()
    extra_E = (pz @ er.half_ulp_bf16(mn @ W).t() + pz @ (dm @ W.abs() + (D + 2) * er.U32 * (mn.abs() @ W.abs())).t()
               + cpos.abs() @ dm.t() + (D + 2) * er.U32 * (cpos.abs() @ mn.abs().t())
               + mean * (dm.sum(1) + (D + 2) * er.U32 * mn.abs().sum(1)))
    ref = er.embed_f64(boards, wt_ext, cpos, mtab, msum, k, D, H, extra_x=extra_x, extra_E=extra_E)
    ref["x_bound"] = ref["x_bound"] + extra_x
    x, _ = embed(boards, hp["wt"], hp["cpos"], hp["ln_w"], hp["ln_b"], geom, D, True, False)
    pr = dict(wt_ext=f["wt_ext"], cpos=hp["cpos"], mtab=f["score_cpos"], msum=f["score_msum"], H=H)
    xn, sc = embed_scores(boards.to(torch.bfloat16), pr, geom, D)
    check_against(ref, x, None, xn, sc, R * R + 1, f"embed_product_{R}x{R}_D{D}_H{H}")


@pytest.mark.parametrize("geom,D", (((2, 8, 10, 3), 128), ((2, 15, 15, 5), 256), ((2, 16, 16, 5), 512)), ids=GID)
def test_embed_scores_entry_honours_the_live_count(geom, D):
    """The live count is reachable through the score entry only.  With a count of 3 of 7 boards, and of 0: the live rows of xhat and
    scores are the uncounted run's bit for bit, the rows past the count keep their sentinel."""
    C, R, Cc, k = geom
    boards = boards_of(geom)
    pr = er.rand_probe(C, R, Cc, k, D, HEADS[D], seed=D)
    xn, sc = embed_scores(boards, pr, geom, D)
    for live in (3, 0):
        xc, scc = embed_scores(boards, pr, geom, D, count=live)
        assert same(xc[:live], xn[:live]) and torch.equal(scc[:live], sc[:live]), live
        assert bool((xc[live:].float() == SENTINEL).all()) and bool((scc[live:] == SENTINEL).all()), live


# ---------------------------------------------------------------------------------------------------------------------------------
# k_cls_pool
# ---------------------------------------------------------------------------------------------------------------------------------
def pool(xhat, scores, c, H, count=None):
    import azk
    n, T, D = xhat.shape
    buf = torch.full((n * H + PAD, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    cnt = None if count is None else torch.tensor([count], dtype=torch.int32, device="cuda")
    z = azk.nn_cls_pool(xhat.cuda(), scores.cuda(), c.cuda(), H, count=cnt, z=buf[: n * H].view(n, H, D))
    torch.cuda.synchronize()
    assert pad_kept(buf, n * H), "wrote past n H rows"
    return z.cpu()


def test_pool_admits_every_listed_token_count():
    assert all(er.pool_lds_bytes(T, D, H) <= 64 * 1024 for T in er.POOL_T for D, H in er.POOL_DH)


@pytest.mark.parametrize("T", er.POOL_T)
@pytest.mark.parametrize("D,H", er.POOL_DH)
def test_pool_selects_and_averages_bit_for_bit(D, H, T):
    """Select (embed_tok_restated.pool_select_probe): score 0 at a target token, -200 elsewhere, c non-zero: z[b][h] is the target's
    xhat row bit for bit; the targets visit token 0, T - 1, every (wave, register set) pair's last chunk and, above 256 tokens, the
    tokens from 256 on.  Mean (pool_mean_probe): 2^j tokens score 0: z = bf16(mean over the set) bit for bit.  Both again with the
    score padding [T, Tp) set to NaN: the same bits."""
    n = 5
    for probe in (er.pool_select_probe, er.pool_mean_probe):
        for poison in (False, True):
            xhat, s, c, want = probe(n, T, D, H, seed=T, poison=poison)
            z = pool(xhat, s, c, H)
            assert same(z, want), (probe.__name__, poison, first_diff(z, want))


@pytest.mark.parametrize("T", er.POOL_T)
@pytest.mark.parametrize("D,H", er.POOL_DH)
def test_pool_within_the_float64_bound(D, H, T):
    """randn xhat, randn scores at a flat (0.5) and a peaked (8) scale: |z - ref| <= 2^-8 |ref| + K u32 A, A = sum p |x| and
    K = 10 Smax + ceil(Tp / 64) + 8 ceil(T / 32) + 15 (embed_tok_restated.pool_k has the derivation).
    Largest error / bound on an MI355X over all cases: 0.9938 (D = 512, T = 31), above 256 tokens 0.9899 (T = 257): the final bf16
    rounding.  Before the softmax phase covered every token, all 36 cases above 256 tokens left the bound."""
    n, worst = 5, 0.0
    g = torch.Generator().manual_seed(1000 * T + D + H)
    for scale in (0.5, 8.0):
        xhat = torch.randn(n, T, D, generator=g).to(torch.bfloat16)
        s = torch.zeros(n, H, er.tp_of(T))
        s[:, :, :T] = torch.randn(n, H, T, generator=g) * scale
        c = torch.randn(H, generator=g)
        ref, A, Smax = er.pool_f64(xhat, s, c, T)
        err = (pool(xhat, s, c, H).double() - ref).abs()
        worst = max(worst, worst_ratio(err, er.pool_bound(ref, A, T, Smax, float(xhat.float().abs().max()))))
    print(f"RATIO pool_D{D}_H{H}_T{T} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("T", (50, 401))
@pytest.mark.parametrize("D,H", er.POOL_DH)
def test_pool_honours_the_live_count(D, H, T):
    """2 of 5 boards, then 0 of 5: the live boards' rows are the uncounted run's bit for bit, the dead boards keep the sentinel."""
    n = 5
    xhat, s, c, want = er.pool_mean_probe(n, T, D, H, seed=T)
    full = pool(xhat, s, c, H)
    for live in (2, 0):
        z = pool(xhat, s, c, H, count=live)
        assert same(z[:live], full[:live]) and bool((z[live:].float() == SENTINEL).all()), live


@pytest.mark.parametrize("D,H,T", ((384, 8, 50), (256, 16, 50), (128, 2, 50), (512, 8, 1025), (512, 4, 3073)))
def test_pool_refuses_what_it_does_not_cover(D, H, T):
    """AZK_ERR_ARG and nothing launched: an unsupported (D, H), and a token count whose weights and partial sums need more than 64 KB
    of LDS ((512, 8): Tp > 1 024; (512, 4): Tp > 3 072)."""
    import azk
    n = 2
    assert (D, H) not in er.POOL_DH or er.pool_lds_bytes(T, D, H) > 64 * 1024
    xhat = torch.zeros(n, T, D, dtype=torch.bfloat16, device="cuda")
    s = torch.zeros(n, H, er.tp_of(T), device="cuda")
    c = torch.zeros(H, device="cuda")
    z = torch.full((n, H, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    rc = azk.lib().azk_nn_cls_pool(xhat.data_ptr(), s.data_ptr(), c.data_ptr(), z.data_ptr(), n, T, D, H, None,
                                   torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == ERR_ARG and bool((z.float() == SENTINEL).all())
