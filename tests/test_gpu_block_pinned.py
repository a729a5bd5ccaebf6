"""The four kernels of the general hand-written forward (PolicyValueNet.forward_blocks_hip: k_ln_rows, k_gemm_tok, k_attn_tok,
k_cls_attn), each called through its azk.nn_* wrapper at small shapes and pinned two ways: probes whose float32 arithmetic is exact,
so the output is known bit for bit (a selected row, a column mean, an integer matmul), and float64 references with bounds derived
from the number formats (tests/block_restated.py states each derivation; tests/test_block_restated.py shows on the CPU that every
probe notices the mistakes it is there for).  DESIGN.md, "What pins the full-token block kernels", lists which of these tests turn
red under five deliberate mistakes in the kernels.

Each float64 test prints `RATIO <name> <largest error / bound>` before it asserts."""
import pytest
import torch

import block_restated as br

pytestmark = pytest.mark.gpu

ATTN_T = (1, 2, 15, 16, 17, 31, 32, 33, 43, 50, 63, 64, 65, 226, 255, 256)
ATTN_CASES = [(T, 256, H) for T in ATTN_T for H in (4, 8)] + [(33, 128, 4), (226, 128, 2), (65, 512, 8), (255, 512, 16)]
CLS_DH = ((512, 8), (256, 8), (256, 4), (128, 4), (128, 8), (512, 4))
CLS_T = (1, 2, 3, 4, 5, 16, 50, 226, 256)
SENTINEL = 7.0


def same(a, b):
    return torch.equal(br.bits(a.cpu()), br.bits(b.cpu()))


def worst_ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 (an exact result where the bound is 0) and x / 0 = inf."""
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


def first_diff(a, b):
    d = (br.bits(a.cpu()) != br.bits(b.cpu())).nonzero()
    return f"{d.shape[0]} elements differ, first at {d[0].tolist()}" if d.shape[0] else "equal"


def attn(qkv, n, T, D, H, **kw):
    import azk
    out = azk.nn_attention_tok(qkv.cuda(), n, T, D, H, **kw)
    torch.cuda.synchronize()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# k_attn_tok
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,D,H", ATTN_CASES)
def test_attention_selects_the_permuted_value_row_bit_for_bit(T, D, H):
    """One-hot softmax by construction (block_restated.attn_select_probe): output row i of head h of board b is V row perm[b][h][i],
    a different permutation per (board, head).  Wrong K chunk, wrong V^T slot, wrong head or board offset: some row is another row."""
    qkv, want = br.attn_select_probe(3, T, D, H, seed=T)
    out = attn(qkv, 3, T, D, H)
    assert same(out, want), first_diff(out, want)


@pytest.mark.parametrize("T,D,H", ATTN_CASES)
def test_attention_counts_exactly_the_live_keys(T, D, H):
    """Q = 0 (block_restated.attn_count_probe): every output is its column's mean over exactly T keys, a bf16 number with a full
    significand.  One pad key in the denominator, or one key dropped, moves it by an ulp.  (T = 256 has no pad key to count.)"""
    qkv, want = br.attn_count_probe(3, T, D, H, seed=T)
    out = attn(qkv, 3, T, D, H)
    assert same(out, want), first_diff(out, want)


@pytest.mark.parametrize("T,D,H", ATTN_CASES)
def test_attention_within_the_float64_bound(T, D, H):
    """randn inputs at scales 0.3, 1.2, 3.0 against float64 softmax attention: |out - o| <= 2^-8 (A + |o|) + 2^-14 A
    (block_restated.attn_bound).  Largest error / bound on an MI355X over all cases and scales: 0.865 (T = 256, head dimension 32); the CPU emulation reaches 0.87."""
    worst = 0.0
    for scale in (0.3, 1.2, 3.0):
        qkv = br.attn_randn(3, T, D, scale, seed=1000 * T + int(10 * scale))
        o, A = br.attn_f64(qkv, 3, T, D, H)
        err = (attn(qkv, 3, T, D, H).cpu().double() - o).abs()
        worst = max(worst, worst_ratio(err, br.attn_bound(o, A)))
    print(f"RATIO attn_T{T}_D{D}_H{H} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("T,D,H", ATTN_CASES)
def test_attention_writes_its_rows_and_nothing_else(T, D, H):
    """`out` is a prefix of a buffer with 16 more rows: those keep their sentinel.  Under a live count of 2 (and of 1) the live boards'
    rows are the uncounted run's bit for bit and the dead boards' rows keep the sentinel."""
    n = 3
    qkv = br.attn_randn(n, T, D, 1.2, seed=T).cuda()
    buf = torch.full((n * T + 16, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
    full = attn(qkv, n, T, D, H, out=buf[: n * T])
    assert full.data_ptr() == buf.data_ptr() and bool((buf[n * T:].float() == SENTINEL).all())
    assert same(full, attn(qkv, n, T, D, H))
    for live in (2, 1):
        buf2 = torch.full((n * T + 16, D), SENTINEL, dtype=torch.bfloat16, device="cuda")
        attn(qkv, n, T, D, H, out=buf2[: n * T], count=torch.tensor([live], dtype=torch.int32, device="cuda"))
        assert same(buf2[: live * T], full[: live * T]) and bool((buf2[live * T:].float() == SENTINEL).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# k_cls_attn
# ---------------------------------------------------------------------------------------------------------------------------------
def cls(xhat, m, c, H):
    import azk
    z = azk.nn_cls_attention(xhat.cuda(), m.cuda(), c.cuda(), H)
    torch.cuda.synchronize()
    return z.cpu()


@pytest.mark.parametrize("per_board", (False, True), ids=("shared", "per_board"))
@pytest.mark.parametrize("D,H", CLS_DH)
def test_cls_attention_selects_and_counts_bit_for_bit(D, H, per_board):
    """Every (D, H) the entry point accepts, T from 1 (three waves without a token: their running max stays -3e38) to 256.
    Selection (block_restated.cls_select_probe): z[b][h] is the target token's xhat row, the targets visiting every residue mod 4 (a
    wave takes the tokens of one residue).  Count (cls_count_probe): m = 0, z is the column mean over exactly T tokens."""
    n = 5
    for T in CLS_T:
        xhat, m, c, want = br.cls_select_probe(n, T, D, H, per_board, seed=T)
        z = cls(xhat, m, c, H)
        assert same(z, want), (T, "select", first_diff(z, want))
        xhat, m, c, want = br.cls_count_probe(n, T, D, H, per_board, seed=T)
        z = cls(xhat, m, c, H)
        assert same(z, want), (T, "count", first_diff(z, want))


@pytest.mark.parametrize("per_board", (False, True), ids=("shared", "per_board"))
@pytest.mark.parametrize("D,H", CLS_DH)
def test_cls_attention_within_the_float64_bound(D, H, per_board):
    """randn xhat, m at two scales (flat and peaked softmax): |z - ref| <= 2^-8 |ref| + 2^-14 A (block_restated.cls_bound).
    Largest error / bound on an MI355X over all cases: 0.981 (a result just above a power of two, where half a bf16 ulp is 2^-8 of it)."""
    n, worst = 5, 0.0
    g = torch.Generator().manual_seed(D + H)
    for T in CLS_T:
        for ms in (0.02, 0.3):
            xhat = torch.randn(n, T, D, generator=g).to(torch.bfloat16)
            m = torch.randn((n, H, D) if per_board else (H, D), generator=g) * ms
            c = torch.randn((n, H) if per_board else (H,), generator=g)
            ref, A = br.cls_f64(xhat, m, c)
            err = (cls(xhat, m, c, H).double() - ref).abs()
            ratio = worst_ratio(err, br.cls_bound(ref, A))
            worst = max(worst, ratio)
            assert ratio <= 1.0, (T, ms, ratio)
    print(f"RATIO cls_D{D}_H{H}_{'pb' if per_board else 'sh'} {worst:.4f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# k_ln_rows
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 301))
@pytest.mark.parametrize("D", (128, 256, 512))
def test_layernorm_rows_within_half_an_ulp_of_float64(D, n):
    """Float64 LayerNorm of the bf16 input; bound = half a bf16 ulp of the float64 result + the float32 term of
    block_restated.ln_bound (constant derived there from the kernel's operation count).  Rows: random, constant (variance 0: eps
    alone sets the scale, y = bf16(b) exactly), mean 100 (at 0.01 deviation, which bf16 rounds away, and at bf16's own resolution
    there), one-hot.  With add_bias the rewritten x is bf16(float32(x) + add) bit for bit and y does not change.
    Largest error / bound on an MI355X: 0.9997 (n = 301, D = 512: a float64 result next to a rounding boundary; half an ulp is the
    whole of it)."""
    import azk
    g = torch.Generator().manual_seed(D + n)
    w = torch.randn(D, generator=g) * 0.5 + 1.0
    b = torch.randn(D, generator=g) * 0.2
    add = torch.randn(D, generator=g) * 0.3
    wc, bc, addc = w.cuda(), b.cuda(), add.cuda()
    worst = 0.0
    for kind in br.LN_KINDS:
        x = br.ln_rows(kind, n, D, seed=D + n)
        ref, xw, kappa = br.ln_f64(x, w, b)
        xin = x.cuda()
        y = azk.nn_layernorm_rows(xin, wc, bc, 1e-5)
        assert same(xin, x)                                                    # no add_bias: the input is left alone
        err = (y.cpu().double() - ref).abs()
        ratio = worst_ratio(err, br.ln_bound(ref, xw, kappa, w, b))
        worst = max(worst, ratio)
        assert ratio <= 1.0, (kind, ratio)
        if kind in ("constant", "mean100_0.01"):
            assert same(y, b.to(torch.bfloat16).expand(n, D).contiguous()), kind
        y2 = azk.nn_layernorm_rows(xin, wc, bc, 1e-5, add_bias=addc)
        assert same(y2, y) and same(xin, (x.float() + add).to(torch.bfloat16)), kind
    print(f"RATIO ln_D{D}_n{n} {worst:.6f}")


# ---------------------------------------------------------------------------------------------------------------------------------
# k_gemm_tok
# ---------------------------------------------------------------------------------------------------------------------------------
def gemm(a, wp, n_out, epi, bias, out, resid=None, count=None):
    import azk
    azk.nn_gemm_tok(a, wp, n_out, br.EPI[epi], bias=bias, out=out, resid=resid if epi == "resid" else None, count=count)
    torch.cuda.synchronize()
    return out


def out_dtype(epi):
    return torch.float32 if epi == "f32" else torch.bfloat16


def check_int(out, pre, resid, epi, live, tag):
    want = br.gemm_int_expected(pre, resid, epi, live)
    got = out[:live].cpu()
    assert torch.equal(got, want) if epi == "f32" else same(got, want), tag
    assert bool((out[live:].float() == SENTINEL).all()), tag


@pytest.mark.parametrize("n_out", (128, 256))
@pytest.mark.parametrize("k", (128, 192, 256, 320, 384, 2048))
def test_gemm_tok_integer_matmul_bit_for_bit(k, n_out):
    """Small integers (block_restated.gemm_int_probe): the F32, BF16 and RESID epilogues equal the integer matmul, bf16-rounded where
    the epilogue rounds.  K / 64 stages in every residue mod 3 of the three-buffer ring (K = 192, 384: 0); M on both sides of the 64-row
    tile; each M with and without a live count that ends inside a tile; rows beyond the count keep their sentinel."""
    import azk
    a, w, bias, resid, pre = br.gemm_int_probe(129, k, n_out, seed=k + n_out)
    wp = azk.pack_linear_weight128(w.cuda())
    ac, bc, rc = a.cuda(), bias.cuda(), resid.cuda()
    for m in (1, 63, 64, 65, 127, 128, 129):
        for live in (None, 0 if m == 1 else m - 7):
            cnt = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
            for epi in ("f32", "bf16", "resid"):
                out = torch.full((m, n_out), SENTINEL, dtype=out_dtype(epi), device="cuda")
                gemm(ac[:m], wp, n_out, epi, bc, out, resid=rc[:m], count=cnt)
                check_int(out, pre, resid, epi, m if live is None else live, (m, live, epi))


@pytest.mark.parametrize("n_out", (128, 256))
def test_gemm_tok_integer_matmul_on_128_row_tiles(n_out):
    """M = 8192 + 65 takes the 128-row-tile variant (K = 128), with and without a live count that ends inside a tile."""
    import azk
    m, k = 8192 + 65, 128
    a, w, bias, resid, pre = br.gemm_int_probe(m, k, n_out, seed=n_out)
    wp = azk.pack_linear_weight128(w.cuda())
    ac, bc, rc = a.cuda(), bias.cuda(), resid.cuda()
    for live in (None, 8192 + 3):
        cnt = None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")
        for epi in ("f32", "bf16", "resid"):
            out = torch.full((m, n_out), SENTINEL, dtype=out_dtype(epi), device="cuda")
            gemm(ac, wp, n_out, epi, bc, out, resid=rc, count=cnt)
            check_int(out, pre, resid, epi, m if live is None else live, (live, epi))


@pytest.mark.parametrize("k,n_out", ((192, 128), (384, 256)))
def test_gemm_tok_leading_dimensions(k, n_out):
    """lda = 3 K, ldr = 5 N, ldo = n_out + 128, passed as strided views (forward_blocks_hip's cls rows are such views): the integer
    probe stays bit for bit, a randn case stays within the float64 bound, and the output columns the view skips keep their sentinel.
    Largest error / bound of the randn case on an MI355X: 0.973 for the bf16 epilogues (the final rounding), 0.005 for float32."""
    import azk
    m = 129
    a, w, bias, resid, pre = br.gemm_int_probe(m, k, n_out, seed=k)
    wp = azk.pack_linear_weight128(w.cuda())
    av, _ = br.strided(a.cuda(), 3 * k, -3.0)
    rv, _ = br.strided(resid.cuda(), 5 * n_out, -3.0)
    assert av.stride(0) == 3 * k and rv.stride(0) == 5 * n_out
    for epi in ("f32", "bf16", "resid"):
        buf = torch.full((m, n_out + 128), SENTINEL, dtype=out_dtype(epi), device="cuda")
        gemm(av, wp, n_out, epi, bias.cuda(), buf[:, :n_out], resid=rv)
        check_int(buf[:, :n_out], pre, resid, epi, m, epi)
        assert bool((buf[:, n_out:].float() == SENTINEL).all()), epi
    g = torch.Generator().manual_seed(k)
    a = (torch.randn(m, k, generator=g) * 0.7).to(torch.bfloat16)
    w = (torch.randn(n_out, k, generator=g) / k ** 0.5).to(torch.bfloat16).float()
    bias = torch.randn(n_out, generator=g) * 0.2
    resid = torch.randn(m, n_out, generator=g).to(torch.bfloat16)
    wp = azk.pack_linear_weight128(w.cuda())
    av, _ = br.strided(a.cuda(), 3 * k, -3.0)
    rv, _ = br.strided(resid.cuda(), 5 * n_out, -3.0)
    for epi in ("f32", "bf16", "gelu", "resid"):
        buf = torch.full((m, n_out + 128), SENTINEL, dtype=out_dtype(epi), device="cuda")
        gemm(av, wp, n_out, epi, bias.cuda(), buf[:, :n_out], resid=rv)
        ref, p, S = br.gemm_f64(a, w, bias, epi, resid=resid)
        ratio = worst_ratio((buf[:, :n_out].cpu().double() - ref).abs(), br.gemm_bound(ref, p, S, k, epi))
        print(f"RATIO gemm_ld_K{k}_{epi} {ratio:.4f}")
        assert ratio <= 1.0, (epi, ratio)
        assert bool((buf[:, n_out:].float() == SENTINEL).all()), epi


def test_gemm_tok_gelu_epilogue_against_float64():
    """Exact pre-activations sweeping [-6, 6] in steps of 2^-12 (block_restated.gemm_gelu_probe) against float64 F.gelu: relative
    2^-8 for the bf16 store plus gelu_erf's stated erf error (1.5e-7, and its float32 evaluation) times |x| / 2; no absolute slack.
    Largest error / bound on an MI355X: 0.989."""
    import azk
    a, w, bias, pre = br.gemm_gelu_probe()
    wp = azk.pack_linear_weight128(w.cuda())
    out = torch.full((a.shape[0], 128), SENTINEL, dtype=torch.bfloat16, device="cuda")
    gemm(a.cuda(), wp, 128, "gelu", bias.cuda(), out)
    ref, p, S = br.gemm_f64(a, w, bias, "gelu")
    assert torch.equal(p, pre)
    ratio = worst_ratio((out.cpu().double() - ref).abs(), br.gemm_bound(ref, p, S, 128, "gelu"))
    print(f"RATIO gemm_gelu {ratio:.4f}")
    assert ratio <= 1.0, ratio
