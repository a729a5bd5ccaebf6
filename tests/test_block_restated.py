"""The probes of tests/test_gpu_block_pinned.py do their job, shown without a GPU: the float32 emulation of each kernel
(tests/block_restated.py) gives a probe's expected output bit for bit, and the emulation with one deliberate mistake gives something
else (or leaves the float64 bound)."""
import numpy as np
import pytest
import torch

import block_restated as br

ATTN_T = (1, 2, 15, 16, 17, 31, 32, 33, 43, 50, 63, 64, 65, 226, 255, 256)
ATTN_DH = ((256, 4), (256, 8))               # head dimension 64 and 32
CLS_DH = ((512, 8), (256, 8), (256, 4), (128, 4), (128, 8), (512, 4))
CLS_T = (1, 2, 3, 4, 5, 16, 50, 226, 256)


def same(a, b):
    return torch.equal(br.bits(a), br.bits(b))


@pytest.mark.parametrize("D,H", ATTN_DH)
@pytest.mark.parametrize("T", ATTN_T)
def test_attention_probes_are_exact_and_see_the_mutations(T, D, H):
    n = 3
    qkv, want = br.attn_select_probe(n, T, D, H, seed=T)
    # the float32 softmax is exactly one-hot: best minus second-best scaled score (pad keys included) is at least 256
    q, k, _ = br.attn_split(qkv, n, T, D, H)
    s = torch.zeros(n, H, T, br.TP, dtype=torch.float64)
    s[..., :T] = q @ k.transpose(-1, -2) / np.sqrt(D // H)
    top = s.topk(2, dim=-1).values
    assert float((top[..., 0] - top[..., 1]).min()) >= 256.0
    assert same(br.attn_emulate(qkv, n, T, D, H), want)
    assert same(br.attn_emulate(qkv, n, T, D, H, "mask_le"), want)             # a pad key weighs exp(-gap) = 0 here: the count probe's job
    if T >= 15:                                                                # (keys 0..3 keep their slot; row 0 has no swizzle)
        assert not same(br.attn_emulate(qkv, n, T, D, H, "vt_natural"), want)
        assert not same(br.attn_emulate(qkv, n, T, D, H, "kswz_read0"), want)
    qkv, want = br.attn_count_probe(n, T, D, H, seed=T)
    assert same(br.attn_emulate(qkv, n, T, D, H), want)
    assert same(br.attn_emulate(qkv, n, T, D, H, "kswz_read0"), want)          # Q = 0: K does not matter
    if T < br.TP:
        assert not same(br.attn_emulate(qkv, n, T, D, H, "mask_le"), want)


@pytest.mark.parametrize("D,H", ATTN_DH)
@pytest.mark.parametrize("T", (17, 50, 226, 256))
def test_attention_emulation_meets_the_float64_bound(T, D, H):
    worst = 0.0
    for scale in (0.3, 1.2, 3.0):
        qkv = br.attn_randn(3, T, D, scale, seed=T + int(10 * scale))
        o, A = br.attn_f64(qkv, 3, T, D, H)
        bound = br.attn_bound(o, A)
        err = (br.attn_emulate(qkv, 3, T, D, H).double() - o).abs()
        worst = max(worst, float((err / bound).max()))
        assert bool((err <= bound).all())
        bad = (br.attn_emulate(qkv, 3, T, D, H, "vt_natural").double() - o).abs()
        assert not bool((bad <= bound).all())
    assert worst < 1.0


@pytest.mark.parametrize("per_board", (False, True))
@pytest.mark.parametrize("D,H", CLS_DH)
def test_cls_attention_probes_are_exact_and_see_the_mutation(D, H, per_board):
    n = 5
    for T in CLS_T:
        xhat, m, c, want = br.cls_select_probe(n, T, D, H, per_board, seed=T)
        assert same(br.cls_emulate(xhat, m, c), want)
        z, A = br.cls_f64(xhat, m, c)
        assert bool(((want.double() - z).abs() <= br.cls_bound(z, A)).all())
        if T >= 4:                                                             # some head's target token is 3 mod 4
            assert not same(br.cls_emulate(xhat, m, c, "combine3"), want)
        xhat, m, c, want = br.cls_count_probe(n, T, D, H, per_board, seed=T)
        assert same(br.cls_emulate(xhat, m, c), want)       # (a dropped wave drops its tokens from both sums: the selection probe's job)


def test_cls_attention_emulation_meets_the_float64_bound():
    g = torch.Generator().manual_seed(0)
    for (n, T, D, H) in ((3, 5, 128, 4), (3, 226, 256, 8), (2, 256, 512, 8)):
        xhat = torch.randn(n, T, D, generator=g).to(torch.bfloat16)
        m = torch.randn(n, H, D, generator=g) * 0.1
        c = torch.randn(n, H, generator=g)
        z, A = br.cls_f64(xhat, m, c)
        assert bool(((br.cls_emulate(xhat, m, c).double() - z).abs() <= br.cls_bound(z, A)).all())


@pytest.mark.parametrize("D", (128, 256, 512))
def test_layernorm_emulation_meets_the_bound_on_every_row_kind(D):
    g = torch.Generator().manual_seed(D)
    w = torch.randn(D, generator=g) * 0.5 + 1.0
    b = torch.randn(D, generator=g) * 0.2
    add = torch.randn(D, generator=g) * 0.3
    for kind in br.LN_KINDS:
        x = br.ln_rows(kind, 5, D, seed=D)
        y, xw, kappa = br.ln_f64(x, w, b)
        got, xr = br.ln_emulate(x, w, b, add_bias=add)
        assert bool(((got.double() - y).abs() <= br.ln_bound(y, xw, kappa, w, b)).all()), kind
        assert same(xr, (x.float() + add).to(torch.bfloat16))
        if kind in ("constant", "mean100_0.01"):                               # variance exactly 0: y = bf16(b) and nothing else
            assert bool((x.float().var(1, unbiased=False) == 0).all()) and same(got, b.to(torch.bfloat16).expand(5, D).contiguous())
    # the bound is tight enough to see a variance taken with D - 1, or an eps outside the root's scale
    x = br.ln_rows("random", 5, D, seed=1)
    y, xw, kappa = br.ln_f64(x, w, b)
    wrong = ((x.float() - x.float().mean(1, keepdim=True)) / x.float().std(1, keepdim=True) * w + b).to(torch.bfloat16)
    assert not bool(((wrong.double() - y).abs() <= br.ln_bound(y, xw, kappa, w, b)).all())


@pytest.mark.parametrize("k", (128, 192, 256, 320, 384, 2048))
def test_gemm_integer_probe_is_exact_and_sees_the_mutation(k):
    m, n_out = 65, 128
    a, w, bias, resid, pre = br.gemm_int_probe(m, k, n_out, seed=k)
    assert float(pre.abs().max()) + 16 < 2 ** 14
    for epi in ("f32", "bf16", "resid"):
        want = br.gemm_int_expected(pre, resid, epi, m)
        got = br.gemm_emulate(a, w, bias, epi, resid=resid)
        assert torch.equal(got, want) if epi == "f32" else same(got, want)
    # strided residual: the mistake reads inside the same buffer, elsewhere
    rv, rbuf = br.strided(resid, 5 * n_out, -3.0)
    want = br.gemm_int_expected(pre, resid, "resid", m)
    assert same(br.gemm_emulate(a, w, bias, "resid", resid=rv, ldo=n_out + 128), want)
    assert (m - 1) * (n_out + 128) + n_out <= rbuf.numel()
    assert not same(br.gemm_emulate(a, w, bias, "resid", resid=rv, ldo=n_out + 128, mutate="resid_ldo"), want)
    # contiguous operands (ldr = ldo) cannot see it
    assert same(br.gemm_emulate(a, w, bias, "resid", resid=resid, ldo=n_out, mutate="resid_ldo"), want)


def test_gemm_gelu_probe_and_float64_bounds():
    a, w, bias, pre = br.gemm_gelu_probe()
    ref, pre2, S = br.gemm_f64(a, w, bias, "gelu")
    assert torch.equal(pre, pre2) and float(pre.min()) == -6.0 and float(pre.max()) > 6.0
    assert torch.equal((a.float() @ w.t() + bias).double(), pre)              # exact in float32
    bound = br.gemm_bound(ref, pre, S, 128, "gelu")
    assert bool(((br.gemm_emulate(a, w, bias, "gelu").double() - ref).abs() <= bound).all())
    tanh_form = torch.nn.functional.gelu(pre.float(), approximate="tanh").to(torch.bfloat16)
    assert not bool(((tanh_form.double() - ref).abs() <= bound).all())        # the other GELU leaves the bound
    g = torch.Generator().manual_seed(3)
    a = (torch.randn(70, 384, generator=g) * 0.7).to(torch.bfloat16)
    w = (torch.randn(128, 384, generator=g) / 384 ** 0.5).to(torch.bfloat16).float()
    bias = torch.randn(128, generator=g) * 0.2
    resid = torch.randn(70, 128, generator=g).to(torch.bfloat16)
    for epi in ("f32", "bf16", "gelu", "resid"):
        ref, pre, S = br.gemm_f64(a, w, bias, epi, resid=resid)
        err = (br.gemm_emulate(a, w, bias, epi, resid=resid).double() - ref).abs()
        assert bool((err <= br.gemm_bound(ref, pre, S, 384, epi)).all()), epi
