"""One link of the fp32-accurate tail (csrc/azk_nnx.hip k_gemm_h through azk_nnx_gemm_h, csrc/azk_tail.hip k_gemm_h_lds through
azk_nnx_gemm_h_lds), restated on the CPU.  Test infrastructure: no GPU, no libazk (azk.pack_linear_weight_h and azk.split_fp16 are
plain tensor code).

The scheme: every operand travels as two fp16 planes of its SCALED value (activations x 16, weights x 256; hi = fp16(x),
lo = fp16(x - hi): 22 significant bits), a k-step adds hi hi + hi lo + lo hi into a float32 accumulator that therefore holds 4096 times
the product, and the epilogue multiplies by 1 / 4096.  The lo lo term is dropped by design.

  * LINKS: every dispatch row of the two entry points; `chains` gives the K split its instantiation uses.
  * exact probes (`probe`): inputs whose planes are exact and whose three-term arithmetic is exact in float32 in any summation order,
    so both output planes, out_f32 and stats_out are known bit for bit - `exactness` returns what a test must assert about them.
  * float64 cases: dense and sparse rows of random 22-bit operands, rows with exact LayerNorm statistics; `_gemm_err`, `_ln_rand` and
    `expected` derive each term of the bound from the formats, with the operation count beside it.
  * `emulate`: the link's float32 arithmetic as the kernels' sources state it, from the PACKED weight, taking one deliberate mistake
    (`mutate=`): tests/test_gemm_h_restated.py shows that each probe notices the mistake it is there for.

Unit roundoffs: float32 u = 2^-24; an fp16 plane pair is within 2^-23 of its (normal) value, and fp16's subnormal step is 2^-24."""
import functools

import numpy as np
import torch

import block_restated as br
import tail_restated as tr
from block_restated import U32
from tail_restated import ACTION_DIMS, SENTINEL, TANHF_MARGIN, heads_n_out, worst_ratio  # noqa: F401

A_SCALE, W_SCALE = 16.0, 256.0                                # azk.GEMM_H_A_SCALE, azk.GEMM_H_W_SCALE
ACC = A_SCALE * W_SCALE                                        # what one unit of the product is in the accumulator: 4096
EPI = {"plain": 0, "gelu": 1, "resid": 2, "heads": 3}         # azk.TAIL_*
LN_EPS = 1e-5
F16_MAX, F16_BELOW_MAX = 65504.0, 65472.0                     # the overflow flag's threshold and the next fp16 number below it
MUTATIONS = ("lo_lo", "reduce3", "a_first_range", "resid_ldo", "col0_no_batch", "stats_01", "ln_lane_j", "split_lo0", "lds_chain")

# name -> k, float32 A (split on the fly), LayerNorm in the epilogue, epilogue, batches, output widths, LDS form.
# Widths: 64 / 128 are one and two wave columns of the split-K instantiations; the GELU links switch to the "wide" 2 x 2-wave block
# (one chain over K) at N >= 1024, N % 128 == 0.
LINKS = {
    "k384_f32_b8":      dict(k=384, af32=True, ln=False, epi="plain", nbatch=8, n_outs=(64,), lds=False),
    "k512_f32":         dict(k=512, af32=True, ln=False, epi="plain", nbatch=1, n_outs=(64, 128), lds=False),
    "k512_f32_b8":      dict(k=512, af32=True, ln=False, epi="plain", nbatch=8, n_outs=(64,), lds=False),
    "k512_plain":       dict(k=512, af32=False, ln=False, epi="plain", nbatch=1, n_outs=(64, 128), lds=False),
    "k512_gelu":        dict(k=512, af32=False, ln=False, epi="gelu", nbatch=1, n_outs=(64, 128, 1024, 2048), lds=False),
    "k512_resid":       dict(k=512, af32=False, ln=False, epi="resid", nbatch=1, n_outs=(64, 128), lds=False),
    "k512_heads":       dict(k=512, af32=False, ln=False, epi="heads", nbatch=1, n_outs=(256,), lds=False),
    "k512_ln_gelu":     dict(k=512, af32=False, ln=True, epi="gelu", nbatch=1, n_outs=(64, 128, 2048), lds=False),
    "k512_ln_heads":    dict(k=512, af32=False, ln=True, epi="heads", nbatch=1, n_outs=(256,), lds=False),
    "k2048_resid":      dict(k=2048, af32=False, ln=False, epi="resid", nbatch=1, n_outs=(64, 128), lds=False),
    "k2048_plain":      dict(k=2048, af32=False, ln=False, epi="plain", nbatch=1, n_outs=(64, 128), lds=False),
    "lds_k512_ln_gelu": dict(k=512, af32=False, ln=True, epi="gelu", nbatch=1, n_outs=(128, 2048), lds=True),
    "lds_k2048_resid":  dict(k=2048, af32=False, ln=False, epi="resid", nbatch=1, n_outs=(64, 128, 512), lds=True),
}
CASES = [(link, n_out) for link, L in LINKS.items() for n_out in L["n_outs"]]


def is_wide(n_out):
    return n_out % 128 == 0 and n_out >= 1024


def chains(L, n_out):
    """Accumulation chains the K range is cut into; their sums are added in the order 0, 1, 2, 3.  Register form: the four waves of a
    split-K workgroup (NWK = 4), one chain in the wide GELU instantiations.  LDS form: link 3 runs one chain, link 4 two wave groups
    of two chains (512 columns each, as the register form's four waves)."""
    if L["lds"]:
        return 4 if L["k"] == 2048 else 1
    return 1 if L["epi"] == "gelu" and is_wide(n_out) else 4


def on_cpu(fn, *args):
    """An azk packing helper on CPU tensors (the binding's helpers ask for a GPU; the packers themselves are tensor arithmetic)."""
    import azk
    saved = azk._torch
    azk._torch = lambda: torch
    try:
        return fn(*args)
    finally:
        azk._torch = saved


def pack(w64):
    """-> (packed planes, col_sums) of azk.pack_linear_weight_h for the float64 [rows, k] weight."""
    import azk
    return on_cpu(azk.pack_linear_weight_h, w64)


def split(x64, scale):
    import azk
    return on_cpu(azk.split_fp16, x64, scale)


def unpack(wp, rows, k):
    """The packed weight's planes as float64 [rows, k] each, read the way a wave reads them: tile (group g, k-step s, column c), plane
    p holds, in lane (l4, l15), the eight k values 32 s + 8 l4 .. + 7 of output column 64 g + 4 l15 + c."""
    t = wp.cpu().view(rows // 64, k // 32, 4, 2, 4, 16, 8).permute(3, 0, 5, 2, 1, 4, 6).reshape(2, rows, k).double()
    return t[0], t[1]


def split_f32(x):
    """The kernels' split of a float32 value that is already scaled: hi = fp16(x), lo = fp16(x - hi) (the difference is exact)."""
    hi = x.to(torch.float16)
    return hi, (x - hi.float()).to(torch.float16)


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def gelu_erff_f32(x):
    """azk_nn_common.h gelu_erff in float32: 0.5 x (1 + erff(x / sqrt 2)).  (block_restated.gelu_erf_f32 is the Abramowitz & Stegun
    form with a true division that stood in its place before: see GELU_ERF_ERR below.)  torch.erf on the CPU stands in for the device's
    erff: the two need not agree to the bit, which does no harm, since GELU links are held to their bound and never to bits."""
    x = x.float()
    return (np.float32(0.5) * x) * (1.0 + torch.erf(x * np.float32(0.70710678118654752)))


def emulate(a, wp, n_out, k, epi, nchains, nbatch=1, a_batch_stride=0, bias=None, col_sums=None, resid=None, a_stats=None,
            eps=LN_EPS, action_dim=0, ldo=None, mutate=None):
    """-> {'f32', 'hi', 'lo', 'stats' [m, N / 64, 2], 'oflow'} or {'logits', 'values'} for HEADS.
    a: float32 [m, >= width] (split here as the kernel splits it) or an fp16 (hi, lo) pair; strided views are fine.
    One MFMA (32 products of one term) is summed exactly and rounded into the float32 accumulator once; the terms of a k-step follow
    each other as hi hi, hi lo, lo hi; the chains are added in the order 0..nchains-1; then x 1 / 4096, LayerNorm from the eight
    (sum, sum of squares) groups as ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)), bias, epilogue, output split, statistics.
    mutate: 'lo_lo' (the third term multiplies lo by the weight's lo plane), 'reduce3' / 'lds_chain' (the last chain never joins the
    sum), 'a_first_range' (every chain reads A's first K range), 'resid_ldo' (the residual row found with the output's `ldo`),
    'col0_no_batch' (bias and col_sums read without b N), 'stats_01' (groups 0 and 1 only), 'ln_lane_j' (mean and rstd of fragment
    row j in place of row 4 l4 + j), 'split_lo0' (the float32 A's lo plane is 0)."""
    assert mutate is None or mutate in MUTATIONS
    f32 = torch.float32
    whi, wlo = unpack(wp, nbatch * n_out, k)
    if isinstance(a, (tuple, list)):
        ahi, alo = a[0].detach().cpu().double(), a[1].detach().cpu().double()
        oflow = False
    else:
        x = a.detach().cpu().float() * np.float32(A_SCALE)
        oflow = bool((~(x.abs() < F16_MAX)).any())
        h, l = split_f32(x)
        ahi, alo = h.double(), (torch.zeros_like(l) if mutate == "split_lo0" else l).double()
    m, kw = ahi.shape[0], k // nchains
    acc = torch.zeros(m, nbatch * n_out, dtype=f32)
    for b in range(nbatch):
        ws = slice(b * n_out, (b + 1) * n_out)
        tot = None
        for c in range(nchains):
            if mutate in ("reduce3", "lds_chain") and nchains > 1 and c == nchains - 1:
                continue
            part = torch.zeros(m, n_out, dtype=f32)
            for s in range(kw // 32):
                ka = b * a_batch_stride + (0 if mutate == "a_first_range" else c * kw) + 32 * s
                kb = c * kw + 32 * s
                xh, xl = ahi[:, ka: ka + 32], alo[:, ka: ka + 32]
                yh, yl = whi[ws, kb: kb + 32].t(), wlo[ws, kb: kb + 32].t()
                for p, q in ((xh, yh), (xh, yl), (xl, yl if mutate == "lo_lo" else yh)):
                    part = (part.double() + p @ q).float()
            tot = part if tot is None else tot + part
        acc[:, ws] = tot
    v = acc * np.float32(1.0 / ACC)
    nb_cols = nbatch * n_out
    pick = (lambda t: t[:n_out].repeat(nbatch)) if mutate == "col0_no_batch" else (lambda t: t[:nb_cols])
    if a_stats is not None:
        st = a_stats.detach().cpu().float().view(m, 8, 2)
        g = [st[:, i, :] for i in range(8)]
        s = g[0] + g[1] if mutate == "stats_01" else ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]))
        mean = s[:, 0:1] * np.float32(1.0 / 512.0)
        var = (s[:, 1:2].double() / 512.0 - mean.double() * mean.double()).float()          # one fma: rounded once
        rstd = 1.0 / torch.sqrt(torch.clamp(var, min=0.0) + np.float32(eps))
        if mutate == "ln_lane_j":
            r = torch.arange(m)
            src = torch.clamp(r // 16 * 16 + r % 4, max=m - 1)
            mean, rstd = mean[src], rstd[src]
        v = (v - pick(col_sums.detach().cpu().float())[None, :] * mean) * rstd
    if bias is not None:
        v = v + pick(bias.detach().cpu().float())[None, :]
    if epi == "heads":
        return {"logits": v[:, :action_dim].contiguous(), "values": torch.tanh(v[:, action_dim]).contiguous()}
    if epi == "gelu":
        v = gelu_erff_f32(v)
    if epi == "resid":
        r = resid.detach().cpu()
        if mutate == "resid_ldo":
            r = torch.as_strided(r, (m, nb_cols), (ldo, 1))
        v = v + r.float()
    x = v * np.float32(A_SCALE)
    hi, lo = split_f32(x)
    g = v.double().view(m, nb_cols // 64, 64)
    return {"f32": v, "hi": hi, "lo": lo, "oflow": oflow or bool((~(x.abs() < F16_MAX)).any()),
            "stats": torch.stack([g.sum(2), (g * g).sum(2)], dim=2).float().contiguous()}


# ---------------------------------------------------------------------------------------------------------------------------------
# probes.  A builder returns a64 / w64 (the TRUE values the planes reconstruct to), bias, resid, a_stats, eps and `pre`, the float64
# value in front of GELU / the residual / tanh.
# ---------------------------------------------------------------------------------------------------------------------------------
def full22(shape, rng, lo_e=7, hi_e=13):
    """Random scaled values with full 22-bit significands: +-n 2^-e, n in [2^21, 2^22), e in lo_e .. hi_e - 1: magnitudes in
    [2^(21 - e), 2^(22 - e)), inside fp16's range, the lo plane a multiple of 2^-e (far above fp16's subnormal step 2^-24)."""
    n = rng.randint(2 ** 21, 2 ** 22, size=shape).astype(np.float64)
    return torch.from_numpy(n * np.exp2(-rng.randint(lo_e, hi_e, size=shape).astype(np.float64)) * rng.choice([-1.0, 1.0], size=shape))


def select_k(r, b, k):
    """37 is prime to 384, 512 and 2048: k consecutive rows hit every slot, 65 rows already land in every chain's K range."""
    return (37 * r + 101 * b) % k


def identity_stats(m):
    """Eight equal groups with sum 0 and sum of squares 64: mean 0 and, with eps = 0, rstd 1 - the LayerNorm links then pass the
    accumulator through unchanged, so the selection, the terms and the count are exact on them too."""
    st = torch.zeros(m, 8, 2)
    st[:, :, 1] = 64.0
    return st


def _finish(L, n_out, m, a64, w64, bias=None, resid=None, a_stats=None, eps=LN_EPS, exact=True, pre=None, **more):
    nb, k = L["nbatch"], L["k"]
    if L["ln"] and a_stats is None:
        a_stats, eps = identity_stats(m), 0.0
    if pre is None:
        pre = torch.zeros(m, nb * n_out, dtype=torch.float64)
        for b in range(nb):
            sl = slice(b * n_out, (b + 1) * n_out)
            pre[:, sl] = a64[:, b * k: (b + 1) * k] @ w64[sl].t()
        if bias is not None:
            pre += bias.double()
    if resid is None and L["epi"] == "resid":
        resid = torch.zeros(m, nb * n_out)
    return dict(a64=a64, w64=w64, bias=bias, resid=resid, a_stats=a_stats, eps=eps, exact=exact, pre=pre, **more)


def _heads_blank(L, w64, action_dim):
    """The probes that are not about the value column zero its weights (and carry no bias): its tanh argument is exactly 0."""
    if L["epi"] == "heads":
        w64[action_dim] = 0.0


def _select(L, n_out, m, rng, action_dim=None):
    """Row r of batch b holds 1 or 2 at slot select_k(r, b): the output row is that (reconstructed) column of W, or twice it.  W carries
    full 22-bit scaled significands, so its lo plane is live almost everywhere; a scaled integer below fp16's 65504 has 16 bits at
    most, which is why these scaled weights are dyadic fractions (multiples of 2^-12) and not integers - `exactness` measures
    every output on its own grid."""
    k, nb = L["k"], L["nbatch"]
    w64 = full22((nb * n_out, k), rng) / W_SCALE
    _heads_blank(L, w64, action_dim)
    a64 = torch.zeros(m, nb * k, dtype=torch.float64)
    r = np.arange(m)
    for b in range(nb):
        a64[r, b * k + select_k(r, b, k)] = torch.from_numpy(1.0 + ((r // 3 + b) & 1))
    return _finish(L, n_out, m, a64, w64)


def _mirror(L, n_out, m, rng, action_dim=None):
    """The selection's mirror image for the float32-A links: W holds +-1, 2 (the output keeps 22 bits and so has exact planes), the
    one-hot A a value whose scaled form has a full 22-bit significand - the row is that value times a column of W only if the
    on-the-fly split keeps its lo plane."""
    k, nb = L["k"], L["nbatch"]
    w64 = torch.from_numpy(np.exp2(rng.randint(0, 2, size=(nb * n_out, k))) * rng.choice([-1.0, 1.0], size=(nb * n_out, k)))
    a64 = torch.zeros(m, nb * k, dtype=torch.float64)
    r = np.arange(m)
    val = full22((m, nb), rng, 9, 13) / A_SCALE
    for b in range(nb):
        a64[r, b * k + select_k(r, b, k)] = val[:, b]
    return _finish(L, n_out, m, a64, w64)


def _terms(L, n_out, m, rng, action_dim=None):
    """Both planes live on both sides, all three terms integers.  Scaled W = 2048 mw + lw, scaled A = (2048 ma + la) / 2048 with
    |m| in {2, 3}, l = +-1 (hi = 2048 mw and ma, lo = lw and la / 2048: the splits of these values); W holds two non-zeros in every
    32-wide k-step of every column, A is dense.  Per product: hi hi = 2048 ma mw, hi lo = ma lw, lo hi = la mw - and the dropped
    lo lo = la lw / 2048.  Expected: the integer sum of the three over 4096, NOT the product of the values."""
    k, nb = L["k"], L["nbatch"]
    ml = lambda shape: (rng.randint(2, 4, size=shape) * rng.choice([-1, 1], size=shape), rng.choice([-1, 1], size=shape))
    ma, la = ml((m, nb * k))
    mw, lw = ml((nb * n_out, k))
    keep = np.argsort(np.argsort(rng.random_sample((nb * n_out, k // 32, 32)), axis=2), axis=2) < 2
    keep = keep.reshape(nb * n_out, k)
    a64 = torch.from_numpy((2048.0 * ma + la) / 2048.0) / A_SCALE
    w64 = torch.from_numpy((2048.0 * mw + lw) * keep) / W_SCALE
    _heads_blank(L, w64, action_dim)
    ahi, alo, whi, wlo = (torch.from_numpy(t.astype(np.float64)) for t in (ma, la / 2048.0, 2048.0 * mw * keep, lw * keep))
    if L["epi"] == "heads":
        whi[action_dim], wlo[action_dim] = 0.0, 0.0
    pre = torch.zeros(m, nb * n_out, dtype=torch.float64)
    for b in range(nb):
        sl, ks = slice(b * n_out, (b + 1) * n_out), slice(b * k, (b + 1) * k)
        pre[:, sl] = (ahi[:, ks] @ whi[sl].t() + ahi[:, ks] @ wlo[sl].t() + alo[:, ks] @ whi[sl].t()) / ACC
    return _finish(L, n_out, m, a64, w64, pre=pre, planes=(ahi, alo, whi, wlo))


def _count(L, n_out, m, rng, action_dim=None):
    """A all ones; W: 255 ones in every output column's K range, floor(255 / steps) or one more in every 32-wide k-step."""
    p = tr._count(L, n_out, m, rng)
    w64 = p["w"].double()
    _heads_blank(L, w64, action_dim)
    return _finish(L, n_out, m, torch.ones(m, L["nbatch"] * L["k"], dtype=torch.float64), w64)


def _int(L, n_out, m, rng, action_dim=None):
    """tail_restated's integer matmul: a in -2 .. 2, w in {-1, 0, 1}, integer bias (|.| <= 8) and residual (|.| <= 16); HEADS: the value
    column's weights are scaled by 2^-6 and every fourth row's argument is exactly 0."""
    p = tr._int(L, n_out, m, rng, action_dim)
    return _finish(L, n_out, m, p["a"].double(), p["w"].double(), bias=p["bias"], resid=p["resid"].float(), pre=p["pre"])


def _value(L, n_out, m, rng, action_dim=None):
    """tail_restated's value-column probe itself (the same rows, weights and bias, so the same tanh arguments as the recorded tanhf
    measurement behind TANHF_MARGIN): multiples of 2^-6 in (-4, 4), exactly 0 in every fourth row."""
    p = tr.probe("int", "k512_heads", n_out, m, action_dim)
    return _finish(L, n_out, m, p["a"].double(), p["w"].double(), bias=p["bias"], pre=p["pre"])


def exact_ln_stats(m):
    """[m, 8, 2] groups with mean +-2^(r mod 3) (the sign flips every four rows) and variance 4^(r mod 4), in unequal shares
    (1, 2, 3, 4, 5, 6, 7, 36) / 64 of the row's sum and sum of squares: all integers, and any group dropped or taken twice moves both."""
    r = torch.arange(m)
    mean = torch.exp2((r % 3).double()) * (1.0 - 2.0 * ((r // 4) % 2).double())
    var = torch.pow(4.0, (r % 4).double())
    share = torch.tensor([1, 2, 3, 4, 5, 6, 7, 36], dtype=torch.float64) / 64.0
    st = torch.stack([512.0 * mean[:, None] * share, 512.0 * (var + mean * mean)[:, None] * share], dim=2)
    return st.float().contiguous(), mean, var


def _ln_exact(L, n_out, m, rng, action_dim=None):
    """LayerNorm with exact statistics, eps = 0: with `exact_ln_stats` the float32 mean is +-2^i, fma(-mean, mean, E2) is 4^j, and
    1 / sqrtf(4^j) = 2^-j - this relies on correctly rounded float32 sqrtf and division, which is hipcc's default (csrc/Makefile sets
    no fast-math flag; an approximate square root or reciprocal would be off by an ulp here and nowhere else).  A and W are the integer
    matmul's, so acc / 4096, col_sums and the bias are integers and rstd (acc / 4096 - mean csum) + bias is a dyadic number of a few
    bits: exact under any FMA contraction of the epilogue.  The statistics say nothing about A's rows: the kernel takes them as given."""
    p = tr._int(L, n_out, m, rng, None)
    a64, w64, bias = p["a"].double(), p["w"].double(), p["bias"]
    _heads_blank(L, w64, action_dim)
    if L["epi"] == "heads":
        bias[action_dim] = 0.0
    st, mean, var = exact_ln_stats(m)
    pre = (a64 @ w64.t() - mean[:, None] * w64.sum(1)[None, :]) / torch.sqrt(var)[:, None] + bias.double()
    return _finish(L, n_out, m, a64, w64, bias=bias, a_stats=st, eps=0.0, pre=pre)


def _gemm_err(L, n_out, planes, S, nonzeros):
    """Bound on the error of acc / 4096 against the float64 product of the reconstructed operands, u = 2^-24.
      the dropped lo lo      |lo| <= 2^-11 |x| on both sides: 2^-22 S, S = sum |a| |w|
      the float32-A split    the kernel's own planes are within 2^-23 of A (two roundings to 11 bits): 2^-23 S
      accumulation           3 `nonzeros` additions of (sums of) term products and the `chains` merges, each within u of the running
                             sum, which stays below S3 = sum |a_hi w_hi| + |a_hi w_lo| + |a_lo w_hi| (taken from the planes):
                             (3 nonzeros + chains) u S3.  A zero product adds exactly, so sparse rows count their non-zeros only.
    x 1 / 4096 is exact (a power of two)."""
    ahi, alo, whi, wlo = planes
    nb, k = L["nbatch"], L["k"]
    S3 = torch.zeros_like(S)
    for b in range(nb):
        sl, ks = slice(b * n_out, (b + 1) * n_out), slice(b * k, (b + 1) * k)
        S3[:, sl] = (ahi[:, ks].abs() @ (whi[sl].abs() + wlo[sl].abs()).t() + alo[:, ks].abs() @ whi[sl].abs().t()) / ACC
    return 2.0 ** -22 * S + (2.0 ** -23 * S if L["af32"] else 0.0) + (3 * nonzeros + chains(L, n_out)) * U32 * S3


def _random(L, n_out, m, rng, action_dim=None, sparse=False):
    """Dense: randn rows (x 0.7) against randn weights / sqrt(K); the operands are what the kernel is given - the planes'
    reconstruction of the draws, or the float32 draws themselves on the float32-A links, whose split happens in the kernel.
    Sparse: 8 non-zeros per row of A with full 22-bit scaled significands (|a| in [1/32, 2)), two in every quarter of the K range
    (every chain of every instantiation), against weights with 22-bit significands.  Reference: the float64 product of these operands."""
    k, nb = L["k"], L["nbatch"]
    if sparse:
        keep = np.argsort(np.argsort(rng.random_sample((m, nb, 4, k // 4)), axis=3), axis=3) < 2
        a64 = full22((m, nb * k), rng, 17, 23) / A_SCALE * torch.from_numpy(keep.reshape(m, nb * k).astype(np.float64))   # scaled in [1/2, 32)
        # scaled in [1, 64) x 16 / sqrt(K) (not a power of two): split again, and the weight is what its planes reconstruct to
        w64 = full22((nb * n_out, k), rng, 16, 22) / W_SCALE * (16.0 / k ** 0.5)
    else:
        a64 = torch.from_numpy((rng.standard_normal((m, nb * k)) * 0.7).astype(np.float32)).double()
        if not L["af32"]:
            ah, al = split(a64, A_SCALE)
            a64 = (ah.double() + al.double()) / A_SCALE
        w64 = torch.from_numpy(rng.standard_normal((nb * n_out, k)) / k ** 0.5)
    hi, lo = split(w64, W_SCALE)
    w64 = (hi.double() + lo.double()) / W_SCALE
    bias = torch.from_numpy(rng.standard_normal(nb * n_out).astype(np.float32)) * 0.2
    resid = torch.from_numpy(rng.standard_normal((m, nb * n_out)).astype(np.float32))
    p = _finish(L, n_out, m, a64, w64, bias=bias, resid=resid if L["epi"] == "resid" else None, exact=False)
    S = torch.zeros_like(p["pre"])
    for b in range(nb):
        sl = slice(b * n_out, (b + 1) * n_out)
        S[:, sl] = a64[:, b * k: (b + 1) * k].abs() @ w64[sl].abs().t()
    p["S"], p["nonzeros"] = S, (8 if sparse else k)
    return p


def _ln_rand(L, n_out, m, rng, action_dim=None):
    """LayerNorm links on real statistics.  Row r is one pattern x0 (integers -100 .. 155 over 16) times 2^(r mod 5), so the groups'
    sums and sums of squares are exact in float32; W random with 22-bit significands; reference: float64 LayerNorm (eps 1e-5) of the
    rows times W^T plus bias.  Float32 operations of k_gemm_h's statistics (the LDS form's are the same), u = 2^-24:
      s1, s2     three additions each on the exact groups: |ds1| <= 3 u G1 (G1 = sum of the groups' |sums|), |ds2| <= 3 u s2;
                 x 1 / 512 is exact: dmean = 3 u G1 / 512, dE2 = 3 u E2
      var + eps  fma(-mean, mean, E2): one rounding, u |var|; + eps: u (var + eps)
                 -> d(var + eps) <= 2 |mean| dmean + 3 u E2 + u |var| + u (var + eps) =: V
      rstd       sqrtf and the division, correctly rounded, u each: rho = V / (2 (var + eps)) + 2 u   (relative)
    and of the epilogue, with P = |x W^T| (float64), C = |csum|, Eg = _gemm_err of the product:
      csum       a float64 sum rounded once: u C;  csum mean: u C |mean| + C dmean;  the difference: u (P + C |mean|)
      x rstd     (rho + u) on at most (P + C |mean|);  + bias: u |pre|
      err = rstd (Eg + C dmean + 3 u (P + C |mean|)) + (rho + u) rstd (P + C |mean|) + u |pre|"""
    k = L["k"]
    x0 = torch.from_numpy(rng.randint(-100, 156, size=k).astype(np.float64)) / 16.0
    x = x0[None, :] * torch.from_numpy(np.exp2(np.arange(m) % 5))[:, None]
    g = x.view(m, 8, 64)
    st64 = torch.stack([g.sum(2), (g * g).sum(2)], dim=2)
    a_stats = st64.float().contiguous()
    assert torch.equal(a_stats.double(), st64)
    w64 = full22((n_out, k), rng, 16, 22) / W_SCALE * (16.0 / k ** 0.5)
    hi, lo = split(w64, W_SCALE)
    w64 = (hi.double() + lo.double()) / W_SCALE
    bias = torch.from_numpy(rng.standard_normal(n_out).astype(np.float32)) * 0.2
    mean = x.mean(1, keepdim=True)
    E2 = (x * x).mean(1, keepdim=True)
    var = E2 - mean * mean
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    pre = ((x - mean) * rstd) @ w64.t() + bias.double()
    dmean = 3 * U32 * st64[:, :, 0].abs().sum(1, keepdim=True) / 512.0
    V = 2 * mean.abs() * dmean + 3 * U32 * E2 + U32 * var.abs() + U32 * (var + LN_EPS)
    rho = V / (2 * (var + LN_EPS)) + 2 * U32
    P, C = (x @ w64.t()).abs(), w64.sum(1).abs()[None, :]
    ahi, alo = split(x, A_SCALE)
    assert torch.equal((ahi.double() + alo.double()) / A_SCALE, x)
    Eg = _gemm_err(L, n_out, (ahi.double(), alo.double(), hi.double(), lo.double()), x.abs() @ w64.abs().t(), k)
    PC = P + C * mean.abs()
    err = rstd * (Eg + C * dmean + 3 * U32 * PC) + (rho + U32) * rstd * PC + U32 * pre.abs()
    return _finish(L, n_out, m, x, w64, bias=bias, a_stats=a_stats, eps=LN_EPS, exact=False, pre=pre, err=err)


_KINDS = {"select": _select, "mirror": _mirror, "terms": _terms, "count": _count, "int": _int, "value": _value, "ln_exact": _ln_exact,
          "dense": _random, "sparse": functools.partial(_random, sparse=True), "ln_rand": _ln_rand}
EXACT_KINDS = ("select", "terms", "count", "int")


@functools.lru_cache(maxsize=None)
def probe(kind, link, n_out, m, action_dim=None):
    """The probe of one kind for one link at m rows (rows are independent: a test may use any prefix).  Cached and never changed.
    Besides the builders' fields: a (what the link is given: the float32 tensor, or the fp16 planes of a64 x 16), wp and csum
    (azk.pack_linear_weight_h of w64), planes (ahi, alo, whi, wlo as float64, in scaled units), err (bound on `pre`)."""
    L = LINKS[link]
    assert kind not in ("ln_exact", "ln_rand") or L["ln"]
    assert kind != "mirror" or L["af32"]
    rng = np.random.RandomState(sorted(_KINDS).index(kind) * 1000003 + sorted(LINKS).index(link) * 10007 + n_out * 13 + (action_dim or 0))
    p = _KINDS[kind](L, n_out, m, rng, action_dim)
    p["wp"], p["csum"] = pack(p["w64"])
    whi, wlo = unpack(p["wp"], L["nbatch"] * n_out, L["k"])
    assert torch.equal((whi + wlo) / W_SCALE, p["w64"]), "the weight's planes reconstruct it exactly"
    if L["af32"]:
        p["a"] = p["a64"].float()
        assert torch.equal(p["a"].double(), p["a64"])
        ahi, alo = split_f32(p["a"] * np.float32(A_SCALE))
    else:
        ahi, alo = split(p["a64"], A_SCALE)
        p["a"] = (ahi, alo)
    if p["exact"] or not L["af32"] or kind == "sparse":       # (the dense float32 A has 24 bits: its split is the kernel's business)
        assert torch.equal((ahi.double() + alo.double()) / A_SCALE, p["a64"]), "A's planes reconstruct it exactly"
    if "planes" in p:
        assert all(torch.equal(x, y) for x, y in zip(p["planes"], (ahi.double(), alo.double(), whi, wlo))), "the planes the builder meant"
    p["planes"] = (ahi.double(), alo.double(), whi, wlo)
    if "err" not in p:
        if p["exact"]:
            p["err"] = torch.zeros_like(p["pre"])
        else:
            # the product's bound, the LayerNorm-free epilogue's bias addition (one rounding of a value within |pre| + bound)
            p["err"] = _gemm_err(L, n_out, p["planes"], p["S"], p["nonzeros"]) + U32 * p["pre"].abs()
    return p


def partial_all_rows(p, L, n_out):
    """The largest sum of |term products| of any output of any row, in the accumulator's units: where every term product is an
    integer there (`exactness`'s `literal`), every partial sum in any order is an integer of at most this magnitude."""
    ahi, alo, whi, wlo = p["planes"]
    nb, k = L["nbatch"], L["k"]
    worst = 0.0
    for b in range(nb):
        sl, ks = slice(b * n_out, (b + 1) * n_out), slice(b * k, (b + 1) * k)
        worst = max(worst, float((ahi[:, ks].abs() @ (whi[sl].abs() + wlo[sl].abs()).t() + alo[:, ks].abs() @ whi[sl].abs().t()).max()))
    return worst


def log2_lowbit(x):
    """log2 of the largest power of two that divides each (dyadic) float64 value; +inf at 0."""
    mant, ex = torch.frexp(x)
    mi = (mant.abs() * 2.0 ** 53).to(torch.int64)
    low = (mi & -mi).double()
    return torch.where(x != 0, ex.double() - 53.0 + torch.log2(torch.clamp(low, min=1.0)), torch.full_like(x, float("inf")))


def exactness(p, L, n_out, rows):
    """What an exact probe rests on, for the test that asserts it (first `rows` rows) -> dict:
      integer_a, integer_w   every scaled operand is an integer
      partial                over all outputs, the sum of |term products| in units of the OUTPUT'S grid - the largest power of two that
                             divides every non-zero term product hi hi, hi lo, lo hi of that output (the low bit of a product of dyadic
                             numbers is the product of their low bits).  Every partial sum, in any order, is an integer multiple of the
                             grid of at most this many units: below 2^24 it is a float32 number
      literal                every output's grid is at least 1, i.e. the partial sums are integers in units of 1 / 4096
    That each plane value is an fp16 number holds by type; that hi + lo is the scaled operand exactly is asserted by `probe`."""
    ahi, alo, whi, wlo = p["planes"]
    nb, k = L["nbatch"], L["k"]
    lah, lal, lwh, lwl = (log2_lowbit(t) for t in p["planes"])
    partial, grid_min = 0.0, float("inf")
    for b in range(nb):
        sl, ks = slice(b * n_out, (b + 1) * n_out), slice(b * k, (b + 1) * k)
        S3 = ahi[:rows, ks].abs() @ (whi[sl].abs() + wlo[sl].abs()).t() + alo[:rows, ks].abs() @ whi[sl].abs().t()
        for r in range(rows):
            g = torch.full((n_out,), float("inf"), dtype=torch.float64)
            for x, y in ((lah, lwh), (lah, lwl), (lal, lwh)):
                g = torch.minimum(g, (x[r, ks][None, :] + y[sl]).min(1).values)
            live = torch.isfinite(g)
            if bool(live.any()):
                partial = max(partial, float((S3[r][live] / torch.exp2(g[live])).max()))
                grid_min = min(grid_min, float(g[live].min()))
    whole = lambda t: bool(torch.equal(t, t.round()))
    return dict(integer_a=whole((ahi + alo)[:rows]), integer_w=whole(whi + wlo), partial=partial, literal=grid_min >= 0.0)


# ---------------------------------------------------------------------------------------------------------------------------------
# expected outputs and bounds
# ---------------------------------------------------------------------------------------------------------------------------------
def _expf_term():
    """The `__expf` share of the issue's erf bound.  __expf(-z^2) inside the Abramowitz & Stegun form is exp2(log2(e) x) on the
    hardware's v_exp_f32 (documented at 1 ulp = 2 u): the argument x = -z z is rounded once (u z^2 absolute), its product with the
    rounded constant log2(e) (half an ulp: u / 2) is rounded again, together at most 2.5 u z^2 absolute on the exponent in natural
    units, i.e. 2.5 u z^2 relative on the result; with the instruction's 2 u: (2.5 z^2 + 2) u relative.  erf takes
    poly exp(-z^2) = erfc(z) of it: erfc(z) (2.5 z^2 + 2) u, largest at z = 0 -> 2 u."""
    z = torch.linspace(0.0, 6.0, 6001, dtype=torch.float64)
    return float((torch.erfc(z) * (2.5 * z * z + 2.0)).max()) * U32


# What a GELU link's erf may be off by: Abramowitz & Stegun 7.1.26's 1.5e-7 plus the __expf share, 2.7e-7 together - the figure the
# former gelu_as documented, now the budget of whatever evaluates erf.  The float32 evaluation of that form did NOT meet it: its erf
# is off by up to 6.1e-7 (2.28 times the budget, at x = 0.035; tests/test_gemm_h_restated.py shows it), which is why the kernels
# call erff now.  Besides erf, the result 0.5 x (1 + erf) takes two roundings: 1 + erf (u (1 + erf) <= 2 u, times |x| / 2) and the
# product (u |gelu| <= u |x|): GELU_RESULT_ROUNDINGS u |x|.  0.5 x is exact.
GELU_ERF_ERR = 1.5e-7 + _expf_term()
GELU_RESULT_ROUNDINGS = 2.0


def gelu_bound(pre, err):
    """|x| / 2 GELU_ERF_ERR + 2 u |x| + 1.13 err (GELU's slope is at most 1.13, which carries the pre-activation's error through)."""
    return 0.5 * pre.abs() * GELU_ERF_ERR + GELU_RESULT_ROUNDINGS * U32 * pre.abs() + 1.13 * err


PLANE_REL, PLANE_ABS = 2.0 ** -23, 2.0 ** -24 / A_SCALE       # an output plane pair: two roundings to 11 bits; fp16's subnormal step over the scale


def expected(p, L, rows=None, action_dim=None):
    """-> dict for the first `rows` rows.  ref (float64) and bound for out_f32, plane_bound for (hi + lo) / 16; exact probes through PLAIN /
    RESID (and the LayerNorm probe): f32, hi, lo (the bits) and stats.  HEADS: logits_ref / logits_bound / logits (bits), values_ref,
    values_bound, values_arg.
      PLAIN, RESID   err (+ u |ref| for the residual's addition)
      GELU           gelu_bound: |x| / 2 GELU_ERF_ERR + 2 u |x| + 1.13 err
      planes         the float32 bound + 2^-23 |ref| + 2^-24 / 16
      logits         err;  value: err + TANHF_MARGIN (|tanh'| <= 1)"""
    epi = L["epi"]
    rows = p["pre"].shape[0] if rows is None else rows
    pre, err = p["pre"][:rows], p["err"][:rows]
    if epi == "heads":
        e = dict(logits_ref=pre[:, :action_dim], logits_bound=err[:, :action_dim], values_arg=pre[:, action_dim],
                 values_ref=torch.tanh(pre[:, action_dim]), values_bound=err[:, action_dim] + TANHF_MARGIN)
        if p["exact"]:
            e["logits"] = pre[:, :action_dim].float().contiguous()
        e["values_zero"] = bool((pre[:, action_dim] == 0).all()) and p["exact"]     # a blanked value column: tanhf(0) is 0, bit for bit
        return e
    if epi == "gelu":
        ref = torch.nn.functional.gelu(pre)
        bound = gelu_bound(pre, err)
        return dict(ref=ref, bound=bound, plane_bound=bound + PLANE_REL * ref.abs() + PLANE_ABS)
    ref, bound = pre, err
    if epi == "resid":
        ref = pre + p["resid"][:rows].double()
        bound = err + U32 * ref.abs()
    e = dict(ref=ref, bound=bound, plane_bound=bound + PLANE_REL * ref.abs() + PLANE_ABS)
    if p["exact"]:
        v = ref.float()
        assert torch.equal(v.double(), ref)
        e["f32"] = v
        e["hi"], e["lo"] = split_f32(v * np.float32(A_SCALE))
        assert torch.equal((e["hi"].double() + e["lo"].double()) / A_SCALE, ref), "the output's planes hold it exactly"
        g = ref.view(rows, -1, 64)
        e["stats"] = torch.stack([g.sum(2), (g * g).sum(2)], dim=2).float().contiguous()
        e["stats_exact"] = bool(float((g * g).sum(2).max()) < 2 ** 24 and torch.equal(g * 1.0, g.round()))
    return e


def call_kwargs(p, L, n_out, rows, action_dim=None):
    """What both azk.nnx_gemm_h and `emulate` take besides (a, wp, n_out, k, epilogue) and the output buffers."""
    kw = dict(nbatch=L["nbatch"], a_batch_stride=L["k"] if L["nbatch"] > 1 else 0, bias=p["bias"], eps=p["eps"])
    if L["epi"] == "resid":
        kw["resid"] = p["resid"][:rows]
    if L["ln"]:
        kw.update(a_stats=p["a_stats"][:rows], col_sums=p["csum"])
    if L["epi"] == "heads":
        kw["action_dim"] = action_dim
    return kw


def emulate_probe(p, L, n_out, rows, action_dim=None, mutate=None, **over):
    kw = call_kwargs(p, L, n_out, rows, action_dim)
    kw.update(over)
    a = p["a"][:rows] if L["af32"] else (p["a"][0][:rows], p["a"][1][:rows])
    return emulate(a, p["wp"], n_out, L["k"], L["epi"], chains(L, n_out), mutate=mutate, **kw)


# ---------------------------------------------------------------------------------------------------------------------------------
# the overflow flag
# ---------------------------------------------------------------------------------------------------------------------------------
def overflow_probe(link, at, sign=1.0, m=33, row=17, col=5):
    """One link whose scaled output (on the float32-A links: whose scaled INPUT) is 65472, the fp16 number below the threshold, in every
    element, and sign x `at` in some: the flag must be set exactly when `at` reaches 65504.  All values are exact, so the outputs are
    held bit for bit as well.
      plane links   A is 8 in column 3 of every row, W[j][3] = 200 (128 x 51200 = 6 553 600 in the accumulator: 1600).  PLAIN: bias
                    2492 brings every element to 4092 = 65472 / 16, column `col`'s bias brings that column to sign x at / 16.  RESID:
                    bias 1000, residual 1492, and the one element (row, col) of the residual makes sign x at / 16.
      float32 A     A[r][r] = 4092, A[row][row] = sign x at / 16, W[0][r] = 1: out[r][0] = A[r][r] (65504 x 256 < 2^24); called with
                    out_f32 only, so that the output's own split stays out of it.
    -> dict(a, wp, bias, resid, n_out, want [m, n_out] float64, expect_flag)."""
    L = LINKS[link]
    k, n_out = L["k"], L["n_outs"][0]
    assert L["nbatch"] == 1 and L["epi"] in ("plain", "resid") and not L["ln"]
    w64 = torch.zeros(n_out, k, dtype=torch.float64)
    a64 = torch.zeros(m, k, dtype=torch.float64)
    below, hit = F16_BELOW_MAX / A_SCALE, sign * at / A_SCALE
    bias = resid = None
    if L["af32"]:
        a64[torch.arange(m), torch.arange(m)] = below
        a64[row, row] = hit
        w64[0, :m] = 1.0
        want = torch.zeros(m, n_out, dtype=torch.float64)
        want[:, 0] = a64[torch.arange(m), torch.arange(m)]
    else:
        a64[:, 3], w64[:, 3] = 8.0, 200.0
        want = torch.full((m, n_out), below, dtype=torch.float64)
        if L["epi"] == "resid":
            want[row, col] = hit
            bias, resid = torch.full((n_out,), 1000.0), (want - 2600.0).float()
        else:
            want[:, col] = hit
            bias = (want[0] - 1600.0).float()
    wp, _ = pack(w64)
    a = a64.float() if L["af32"] else split(a64, A_SCALE)
    return dict(a=a, wp=wp, bias=bias, resid=resid, n_out=n_out, want=want, expect_flag=at >= F16_MAX)


def stats_ratio(stats, e):
    """stats_out [rows, N / 64, 2] where its bits are not known, against the float64 sums of the reference: a value v within `bound`
    of ref, 64 of them added in float32 in some order (at most 64 roundings of partial sums below sum |v|):
      sum      sum bound + 64 u sum (|ref| + bound)
      squares  v^2 within 2 |ref| bound + bound^2 and one rounding of the square (u v^2): sum of those + 64 u sum v^2"""
    rows = stats.shape[0]
    ref, b = e["ref"].view(rows, -1, 64), e["bound"].view(rows, -1, 64)
    mag = ref.abs() + b
    d1 = (stats[:, :, 0].double() - ref.sum(2)).abs()
    d2 = (stats[:, :, 1].double() - (ref * ref).sum(2)).abs()
    b1 = b.sum(2) + 64 * U32 * mag.sum(2)
    b2 = (2 * ref.abs() * b + b * b).sum(2) + 65 * U32 * (mag * mag).sum(2)
    return max(worst_ratio(d1, b1), worst_ratio(d2, b2))


def verdict(got, e, L):
    """A result (the emulation's, a mutant's or the card's: any of f32 / hi + lo / stats, or logits + values, as CPU tensors of the
    same rows as `e`) against `expected` -> largest error / bound; bits where the probe gives bits: 0 if they all agree, inf if not."""
    bad = float("inf")
    if L["epi"] == "heads":
        if "logits" in e:
            worst = 0.0 if torch.equal(got["logits"], e["logits"]) else bad
        else:
            worst = worst_ratio((got["logits"].double() - e["logits_ref"]).abs(), e["logits_bound"])
        if e["values_zero"] and not bool((got["values"] == 0).all()):
            return bad
        return max(worst, worst_ratio((got["values"].double() - e["values_ref"]).abs(), e["values_bound"]))
    worst = 0.0
    if "stats" in got and not e.get("stats_exact", False):
        worst = stats_ratio(got["stats"], e)
    if "f32" in e:
        if "f32" in got and not torch.equal(got["f32"], e["f32"]):
            worst = bad
        if "hi" in got and not (torch.equal(got["hi"].view(torch.int16), e["hi"].view(torch.int16))
                                and torch.equal(got["lo"].view(torch.int16), e["lo"].view(torch.int16))):
            worst = bad
        if "stats" in got and e["stats_exact"] and not torch.equal(got["stats"], e["stats"]):
            worst = bad
        return worst
    if "f32" in got:
        worst = max(worst, worst_ratio((got["f32"].double() - e["ref"]).abs(), e["bound"]))
    if "hi" in got:
        worst = max(worst, worst_ratio(((got["hi"].double() + got["lo"].double()) / A_SCALE - e["ref"]).abs(), e["plane_bound"]))
    return worst
