"""The four kernels of the general hand-written forward (PolicyValueNet.forward_blocks_hip): k_ln_rows (csrc/azk_rows.hip), k_gemm_tok and
k_attn_tok (csrc/azk_block.hip) and k_cls_attn (csrc/azk_embed_tok.hip), restated on the CPU.  Test infrastructure: no GPU, no libazk.

For each operation there is
  * a float64 reference (`*_f64`) with the error bound a correct kernel must meet (`*_bound`),
  * a float32 emulation of the kernel's arithmetic as its source states it (`*_emulate`), which also takes the name of one deliberate
    mistake (`mutate=`), so that a probe can be shown to notice that mistake without a GPU,
  * probe builders: inputs whose float32 arithmetic is exact in any summation order, so that the kernel's output is known bit for bit.

Unit roundoffs: bf16 keeps 8 significand bits, u16 = 2^-8 (a rounded value is within 2^-8 of itself, relative); float32 u32 = 2^-24.
"""
import math

import numpy as np
import torch

U16 = 2.0 ** -8
U32 = 2.0 ** -24
TP = 256                                      # k_attn_tok pads the keys of a board to 256
NEG = -3.0e38                                 # the kernels' "no key yet" running max


def bf16(x):
    """Round to bf16 (nearest even) and come back as float32: the value a kernel's bf16 store keeps."""
    return x.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def bits(x):
    """bf16 tensor -> its int16 bit patterns (bit-for-bit comparison that tells -0 from +0 and is defined for NaN)."""
    assert x.dtype == torch.bfloat16
    return x.contiguous().view(torch.int16)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_attn_tok
# ---------------------------------------------------------------------------------------------------------------------------------
def attn_vt_slot(k):
    """The V^T slot of key k: within a 32-key group, the order in which a lane group holds the rows of two stacked accumulator tiles."""
    k = np.asarray(k)
    return 32 * (k >> 5) + 8 * ((k >> 2) & 3) + 4 * ((k >> 4) & 1) + (k & 3)


def attn_kswz(r, dh):
    r = np.asarray(r)
    return (r & 7) if dh == 64 else ((r >> 2) & 3)


def attn_split(qkv, n, T, D, H):
    """bf16 [n T, 3 D] -> q, k, v as float64 [n, H, T, dh]."""
    dh = D // H
    x = qkv.detach().cpu().to(torch.float64).view(n, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    return x[0], x[1], x[2]


def attn_f64(qkv, n, T, D, H):
    """softmax(q k^T / sqrt(dh)) v in float64 -> (o, A) as [n T, D]: o the output, A = sum_k p_k |v_k| the bound's scale."""
    q, k, v = attn_split(qkv, n, T, D, H)
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D // H), dim=-1)
    back = lambda t: t.permute(0, 2, 1, 3).reshape(n * T, D)
    return back(p @ v), back(p @ v.abs())


def attn_bound(o, A):
    """|out - o| <= 2^-8 (A + |o|) + 2^-14 A.  The probabilities enter the second product rounded to bf16: each p_k moves by at most
    2^-8 p_k, the numerator by at most 2^-8 A; the output is rounded once more, 2^-8 |o|.  The denominator is summed unrounded.  The last
    term allows for float32 accumulation: at most 2 x 256 additions of u32 = 2^-24 each relative to A is 2^-15, doubled."""
    return U16 * (A + o.abs()) + 2.0 ** -14 * A


def attn_emulate(qkv, n, T, D, H, mutate=None):
    """k_attn_tok's arithmetic in float32: scores of the query against 256 key slots (pad keys are zero rows), times 1/sqrt(dh), pad
    keys set to -3e38; p = exp(s - max); the sum over the UNROUNDED p; the numerator over the bf16-ROUNDED p; times 1/sum; one rounding
    to bf16.  mutate: None | 'mask_le' (key <= T is live) | 'vt_natural' (V^T slots in natural key order) | 'kswz_read0' (the K chunk
    swizzle left out on the read side)."""
    assert mutate in (None, "mask_le", "vt_natural", "kswz_read0")
    dh = D // H
    x = qkv.detach().cpu().to(torch.float32).view(n, T, 3, H, dh).permute(2, 0, 3, 1, 4)
    q = x[0]
    kp = torch.zeros(n, H, TP, dh)
    vp = torch.zeros(n, H, TP, dh)
    kp[:, :, :T] = x[1]
    vp[:, :, :T] = x[2]
    if mutate == "kswz_read0":                # the read of logical chunk c lands on physical chunk c, which holds logical chunk c ^ swz(row)
        r = np.arange(TP)[:, None]
        d = np.arange(dh)[None, :]
        src = 8 * ((d >> 3) ^ attn_kswz(r, dh)) + (d & 7)
        kp = torch.gather(kp, 3, torch.from_numpy(src).expand(n, H, TP, dh))
    if mutate == "vt_natural":                # slot s holds key s, but the probability that meets slot s is that of the key whose slot is s
        vp = vp[:, :, torch.from_numpy(attn_vt_slot(np.arange(TP)))]
    scale = torch.tensor(1.0 / np.sqrt(np.float32(dh)), dtype=torch.float32)
    s = (q @ kp.transpose(-1, -2)) * scale
    live = T + 1 if (mutate == "mask_le" and T < TP) else T
    s[..., live:] = NEG
    p = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    inv = 1.0 / p.sum(dim=-1, keepdim=True)
    o = (bf16(p) @ vp) * inv
    return o.permute(0, 2, 1, 3).reshape(n * T, D).to(torch.bfloat16)


def code_rows(codes, dh, mag):
    """Integer codes (0..255) -> float rows [..., dh] of +-mag: element d carries bit (d + d // 8) mod 8 of the code, so every 16-byte
    chunk (8 elements) holds all eight bits, each chunk in its own rotation - a chunk read from the wrong place scores differently."""
    d = np.arange(dh)
    bit = (d + (d >> 3)) & 7
    b = (np.asarray(codes)[..., None] >> bit) & 1
    return (2.0 * b - 1.0) * mag


def distinct_bf16(count, rng):
    """`count` distinct finite, normal, non-zero bf16 bit patterns of moderate size (|x| in 2^-60 .. 2^61, either sign)."""
    e = np.arange(67, 188)
    pats = ((e[:, None] << 7) | np.arange(128)[None, :]).reshape(-1)
    pats = np.concatenate([pats, pats | 0x8000]).astype(np.uint16)
    assert count <= pats.size
    return rng.permutation(pats)[:count]


def attn_select_probe(n, T, D, H, seed):
    """-> (qkv bf16 [n T, 3 D], expected bf16 [n T, D]).  Key k of a head is the code of k as +-32 and query i the code of perm[b][h][i]:
    the matching key scores 1024 dh, any other at most 1024 (dh - dh/4), so after the scale the gap is at least 1024 dh / (4 sqrt(dh))
    >= 1448, exp underflows to 0 and the float32 softmax is exactly one-hot (pad keys score 0, far below too).  V holds distinct bf16
    patterns per (board, head): the output row must be V[perm[b][h][i]] bit for bit."""
    dh = D // H
    rng = np.random.RandomState(seed)
    x = np.zeros((n, T, 3, H, dh), np.float32)
    vb = np.zeros((n, T, H, dh), np.uint16)
    want = np.zeros((n, T, H, dh), np.uint16)
    for b in range(n):
        for h in range(H):
            perm = rng.permutation(T)
            x[b, :, 0, h] = code_rows(perm, dh, 32.0)
            x[b, :, 1, h] = code_rows(np.arange(T), dh, 32.0)
            pat = distinct_bf16(T * dh, rng).reshape(T, dh)
            vb[b, :, h] = pat
            want[b, :, h] = pat[perm]
    qkv = torch.from_numpy(x).to(torch.bfloat16)
    qkv[:, :, 2] = torch.from_numpy(vb.view(np.int16)).view(torch.bfloat16)
    return qkv.reshape(n * T, 3 * D), torch.from_numpy(want.view(np.int16)).view(torch.bfloat16).reshape(n * T, D)


COUNT_MEANS = (255.0, -127.5, -255.0, 127.5)  # bf16 numbers with all eight significand bits set


def mean_columns(T, cols, rng):
    """float32 [T, cols]: column c holds COUNT_MEANS[c % 4] plus one ulp-sized step up on some rows and down on as many others, so its
    mean over exactly the T rows is COUNT_MEANS[c % 4] (255 +- 1 and 127.5 +- 0.5 are bf16 numbers; every partial sum is an integer
    multiple of 0.5 below 2^17, exact in float32 in any order).  One row more or fewer in the denominator moves the mean by at least
    |mean| / 256, which is an ulp of these numbers: twice the half ulp that bf16 rounding forgives."""
    out = np.zeros((T, cols), np.float32)
    for c in range(cols):
        mean = COUNT_MEANS[c % 4]
        step = np.zeros(T, np.float32)
        half = rng.randint(0, T // 2 + 1)
        idx = rng.permutation(T)
        step[idx[:half]] = 1.0
        step[idx[half: 2 * half]] = -1.0
        out[:, c] = mean + step * (abs(mean) / 255.0)
    return out


def attn_count_probe(n, T, D, H, seed):
    """-> (qkv, expected).  Q = 0: every live key weighs 1, the sum is T; V's columns come from mean_columns per board: the expected
    output is the column mean in every row.  K is random (it must not matter)."""
    rng = np.random.RandomState(seed)
    x = np.zeros((n, T, 3, D), np.float32)
    x[:, :, 1] = rng.standard_normal((n, T, D))
    want = np.zeros((n, T, D), np.float32)
    for b in range(n):
        x[b, :, 2] = mean_columns(T, D, rng)
    want[:] = np.asarray(COUNT_MEANS, np.float32)[np.arange(D) % 4]
    return torch.from_numpy(x).to(torch.bfloat16).reshape(n * T, 3 * D), torch.from_numpy(want).to(torch.bfloat16).reshape(n * T, D)


def attn_randn(n, T, D, scale, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n * T, 3 * D, generator=g) * scale).to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_cls_attn
# ---------------------------------------------------------------------------------------------------------------------------------
def _cls_mc(m, c, n):
    m = m.detach().cpu()
    c = c.detach().cpu()
    if m.dim() == 2:
        m = m.expand(n, *m.shape)
        c = c.expand(n, *c.shape)
    return m, c


def cls_f64(xhat, m, c):
    """z[b,h,:] = sum_t softmax_t(xhat[b,t,:] . m[.,h,:] + c[.,h]) xhat[b,t,:] in float64 -> (z, A), A = sum_t p_t |xhat_t|."""
    x = xhat.detach().cpu().double()
    m, c = _cls_mc(m, c, x.shape[0])
    p = torch.softmax(torch.einsum("ntd,nhd->nht", x, m.double()) + c.double()[:, :, None], dim=2)
    return torch.einsum("nht,ntd->nhd", p, x), torch.einsum("nht,ntd->nhd", p, x.abs())


def cls_bound(z, A):
    """|out - z| <= 2^-8 |z| + 2^-14 A: float32 probabilities and sums, one rounding to bf16 at the end; the float32 allowance is
    the same as attn_bound's (at most 256 tokens)."""
    return U16 * z.abs() + 2.0 ** -14 * A


def cls_emulate(xhat, m, c, mutate=None):
    """k_cls_attn in float32: wave w streams the tokens t = w (mod 4) with a running max (-3e38 before the first token), a running
    sum and a running weighted row; the four waves are combined as sum_w exp(max_w - M) (.) and divided once; one rounding to bf16.
    mutate: None | 'combine3' (the combine loop runs over three waves)."""
    assert mutate in (None, "combine3")
    x = xhat.detach().cpu().float()
    n, T, D = x.shape
    m, c = _cls_mc(m, c, n)
    m = m.float()
    c = c.float()
    H = m.shape[1]
    s = torch.einsum("ntd,nhd->nht", x, m) + c[:, :, None]
    run_m = torch.full((4, n, H), NEG)
    run_l = torch.zeros(4, n, H)
    zacc = torch.zeros(4, n, H, D)
    for t in range(T):
        w = t & 3
        nm = torch.maximum(run_m[w], s[:, :, t])
        alpha = torch.exp(run_m[w] - nm)
        p = torch.exp(s[:, :, t] - nm)
        run_m[w] = nm
        run_l[w] = run_l[w] * alpha + p
        zacc[w] = zacc[w] * alpha[:, :, None] + p[:, :, None] * x[:, None, t, :]
    M = run_m.max(dim=0).values
    L = torch.zeros(n, H)
    Z = torch.zeros(n, H, D)
    for w in range(3 if mutate == "combine3" else 4):
        e = torch.exp(run_m[w] - M)
        L = L + run_l[w] * e
        Z = Z + zacc[w] * e[:, :, None]
    return (Z / L[:, :, None]).to(torch.bfloat16)


def cls_select_probe(n, T, D, H, per_board, seed):
    """-> (xhat bf16 [n,T,D], m, c, expected bf16 [n,H,D]).  The eight code dimensions j D / 8 (one in every
    eighth of the row, so in eight different lanes) hold bit j of the token index as +-8 in xhat and bit j of the head's target token
    as +-8 in m; m is 0 elsewhere.  The target scores 512, any other token at most 384: the gap of 128 underflows exp, the softmax is
    one-hot and z[b][h] is the target's xhat row bit for bit.  The other dimensions hold arbitrary moderate bf16 patterns.  With
    per-board m the target of (b, h) is (b + h) mod T, so it visits every residue mod 4; with shared m it is h mod T."""
    rng = np.random.RandomState(seed)
    cd = np.arange(8) * (D // 8)
    pat = rng.permutation(np.tile(distinct_bf16(30000, rng), (n * T * D + 29999) // 30000))[: n * T * D]
    xb = torch.from_numpy(pat.view(np.int16).reshape(n, T, D).copy()).view(torch.bfloat16)
    tok = np.arange(T)
    xb[:, :, cd] = torch.from_numpy(((((tok[:, None] >> np.arange(8)) & 1) * 2.0 - 1.0) * 8.0).astype(np.float32)).to(torch.bfloat16)
    tgt = (np.arange(n)[:, None] * (1 if per_board else 0) + np.arange(H)[None, :]) % T          # [n, H]
    m = torch.zeros(n, H, D)
    m[:, :, cd] = torch.from_numpy((((tgt[:, :, None] >> np.arange(8)) & 1) * 2.0 - 1.0) * 8.0).float()
    c = torch.from_numpy(rng.standard_normal((n, H))).float()
    want = torch.stack([torch.stack([xb[b, tgt[b, h]] for h in range(H)]) for b in range(n)])
    if not per_board:
        m, c = m[0].contiguous(), c[0].contiguous()
    return xb, m, c, want


def cls_count_probe(n, T, D, H, per_board, seed):
    """-> (xhat, m, c, expected).  m = 0, so every token weighs exp(c - c) = 1; xhat's columns come from mean_columns: z must be the
    column mean bit for bit, for every head."""
    rng = np.random.RandomState(seed)
    xb = torch.from_numpy(np.stack([mean_columns(T, D, rng) for _ in range(n)])).to(torch.bfloat16)
    m = torch.zeros((n, H, D) if per_board else (H, D))
    c = torch.from_numpy(rng.standard_normal((n, H) if per_board else (H,))).float()
    want = torch.from_numpy(np.asarray(COUNT_MEANS, np.float32)[np.arange(D) % 4]).to(torch.bfloat16).expand(n, H, D).contiguous()
    return xb, m, c, want


# ---------------------------------------------------------------------------------------------------------------------------------
# k_ln_rows
# ---------------------------------------------------------------------------------------------------------------------------------
LN_C = 16.0          # see ln_bound
LN_SUM_DEPTH = 13.0  # additions on the longest path of a row sum at D = 512: 7 in the lane, 4 in row16_sum, 2 across lane groups


def ln_f64(x, w, b, eps=1e-5):
    """nn.LayerNorm (biased variance, eps inside the root) in float64 on the bf16 input -> (y, xw, kappa): xw = xhat w, and
    kappa[row] = mean|x| / sqrt(var + eps), the row's sensitivity to an error in the mean."""
    x = x.detach().cpu().double()
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + eps)
    xw = (x - mean) * rstd * w.detach().cpu().double()
    return xw + b.detach().cpu().double(), xw, x.abs().mean(1, keepdim=True) * rstd


def ln_bound(y, xw, kappa, w, b):
    """|out - y| <= half a bf16 ulp of y + u32 (LN_C (|xhat w| + |b|) + LN_SUM_DEPTH kappa |w|).
    The float32 operations between the bf16 input and the bf16 store, by k_ln_rows' source:
      mean     a tree sum of depth <= 13 (then x 1/D, exact): absolute error <= 13 u32 mean|x|.  It shifts every x - mean by the same
               amount, which after x rstd x w is 13 u32 kappa |w| - the only term that is not relative to the result.  (It vanishes
               when the row sum is exact, as for a constant row: D c has at most 8 + 9 significant bits.)
      x - mean 1 rounding;  squares 2 x 1 + 1;  their tree sum 13;  + eps 1  -> the variance carries 17 u32, its inverse root half
               of that plus 2 for v_rsq_f32 (1 ulp): 10.5
      x rstd, x w, + b   one rounding each (fewer where the compiler contracts to an fma)
    so |xhat w| carries at most 1 + 10.5 + 2 = 13.5 u32 and the sum with b one more, relative to at most |xhat w| + |b|: LN_C = 16
    covers 14.5 with the second-order terms."""
    y = y.double()
    mant, expo = torch.frexp(y)                                   # |y| in [2^(e-1), 2^e): a bf16 ulp there is 2^(e-8), half of it 2^(e-9)
    half_ulp = torch.where(y == 0, torch.zeros_like(y), torch.ldexp(torch.ones_like(y), expo - 9))
    wd, bd = w.detach().cpu().double(), b.detach().cpu().double()
    return half_ulp + U32 * (LN_C * (xw.abs() + bd.abs()) + LN_SUM_DEPTH * kappa * wd.abs())


def ln_emulate(x, w, b, eps=1e-5, add_bias=None):
    """k_ln_rows in float32 -> (y bf16, x rewritten bf16 or None)."""
    v = x.detach().cpu().float()
    D = v.shape[1]
    mean = v.sum(1, keepdim=True) * np.float32(1.0 / D)
    d = v - mean
    rstd = torch.rsqrt((d * d).sum(1, keepdim=True) * np.float32(1.0 / D) + np.float32(eps))
    y = (d * rstd * w.detach().cpu().float() + b.detach().cpu().float()).to(torch.bfloat16)
    return y, (None if add_bias is None else (v + add_bias.detach().cpu().float()).to(torch.bfloat16))


LN_KINDS = ("random", "constant", "mean100_0.01", "mean100_ulp", "onehot")


def ln_rows(kind, n, D, seed):
    """bf16 [n, D] rows of one kind.  'constant': variance 0, eps alone sets the scale.  'mean100_0.01': 100 + 0.01 randn - bf16 has
    an ulp of 0.5 at 100, so these rows round to the constant 100 (kept as stated; the variance is exactly 0 again).  'mean100_ulp':
    the same idea at the resolution bf16 has there, 100 + 0.5 k with k in {-1, 0, 1}: a large mean over a small deviation."""
    g = torch.Generator().manual_seed(seed)
    if kind == "random":
        x = torch.randn(n, D, generator=g) * 1.7 + 0.3
    elif kind == "constant":
        x = (torch.randn(n, 1, generator=g) * 3.0).expand(n, D)
    elif kind == "mean100_0.01":
        x = 100.0 + 0.01 * torch.randn(n, D, generator=g)
    elif kind == "mean100_ulp":
        x = 100.0 + 0.5 * torch.randint(-1, 2, (n, D), generator=g).float()
    elif kind == "onehot":
        x = torch.zeros(n, D)
        x[torch.arange(n), torch.randint(0, D, (n,), generator=g)] = torch.randn(n, generator=g) * 4.0 + 5.0
    else:
        raise ValueError(kind)
    return x.contiguous().to(torch.bfloat16)


# ---------------------------------------------------------------------------------------------------------------------------------
# k_gemm_tok
# ---------------------------------------------------------------------------------------------------------------------------------
EPI = {"bf16": 0, "gelu": 1, "resid": 2, "f32": 4}          # azk.TOK_*
GELU_ERF_ERR = 1.5e-7 + 16.0 * U32   # Abramowitz & Stegun 7.1.26 as azk_nn_common.h states it, plus its float32 evaluation: the reciprocal
                                     # (1 ulp = 2 u32), 1 + p z (2), Horner (5 x 2 on values below 1.5), __expf (2), 1 - . and 1 + . (2)


def gemm_f64(a, w, bias, epi, resid=None):
    """a [m, k] bf16, w [n_out, k] (the bf16 values the packed weight holds), bias float32 -> (ref, pre, S): the epilogue's float64
    result, the pre-activation a w^T + bias, and S = |a| |w|^T + |bias| (the dot product's scale)."""
    ad, wd, bd = a.detach().cpu().double(), w.detach().cpu().double(), bias.detach().cpu().double()
    pre = ad @ wd.t() + bd
    S = ad.abs() @ wd.abs().t() + bd.abs()
    ref = pre
    if epi == "gelu":
        ref = torch.nn.functional.gelu(pre)
    if epi == "resid":
        ref = pre + resid.detach().cpu().double()
        S = S + resid.detach().cpu().double().abs()
    return ref, pre, S


def gemm_bound(ref, pre, S, k, epi):
    """float32 accumulation of k products and the bias (and the residual) in any order: (k + 2) u32 S.  The bf16 epilogues round once
    more: 2^-8 |ref|.  GELU: gelu_erf's erf is off by at most GELU_ERF_ERR, the result by half of |x| times that; GELU has slope at
    most 1.13, which carries the accumulation error through.  No absolute slack."""
    acc = (k + 2) * U32 * S
    if epi == "f32":
        return acc + U32 * ref.abs()
    if epi == "gelu":
        return U16 * ref.abs() + 0.5 * pre.abs() * GELU_ERF_ERR + 1.13 * acc
    return U16 * ref.abs() + acc


def gelu_erf_f32(x):
    """azk_nn_common.h gelu_erf in float32 (a true reciprocal in place of v_rcp_f32)."""
    x = x.float()
    z = x.abs() * np.float32(0.70710678118654752)
    t = 1.0 / (1.0 + np.float32(0.3275911) * z)
    poly = t * (np.float32(0.254829592) + t * (np.float32(-0.284496736) + t * (np.float32(1.421413741) + t * (np.float32(-1.453152027) + t * np.float32(1.061405429)))))
    erf_abs = 1.0 - poly * torch.exp(-z * z)
    return 0.5 * x * (1.0 + torch.copysign(erf_abs, x))


def gemm_emulate(a, w, bias, epi, resid=None, ldo=None, mutate=None):
    """k_gemm_tok in float32 -> [m, n_out] (float32 for 'f32', else bf16).  resid may be a strided view; mutate: None | 'resid_ldo'
    (the residual row is found with the OUTPUT's leading dimension `ldo` in resid's storage)."""
    assert mutate in (None, "resid_ldo")
    v = a.detach().cpu().float() @ w.detach().cpu().float().t() + bias.detach().cpu().float()
    m, n_out = v.shape
    if epi == "gelu":
        v = gelu_erf_f32(v)
    if epi == "resid":
        r = resid.detach().cpu()
        if mutate == "resid_ldo":
            r = torch.as_strided(r, (m, n_out), (ldo, 1))
        v = v + r.float()
    return v if epi == "f32" else v.to(torch.bfloat16)


def gemm_int_probe(m, k, n_out, seed):
    """-> (a bf16 [m,k], w float32 [n_out,k], bias float32, resid bf16 [m,n_out], pre float64).  Integers in [-2, 2] in a and w, integer
    bias (|.| <= 8) and residual (|.| <= 16): every partial sum is an integer below 2^14, so the float32 result is the integer matmul
    in any order and each epilogue's output is known bit for bit (bf16-rounded where it rounds: sums can pass 256)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-2, 3, (m, k), generator=g).to(torch.bfloat16)
    w = torch.randint(-2, 3, (n_out, k), generator=g).float()
    bias = torch.randint(-8, 9, (n_out,), generator=g).float()
    resid = torch.randint(-16, 17, (m, n_out), generator=g).to(torch.bfloat16)
    pre = a.double() @ w.double().t() + bias.double()
    return a, w, bias, resid, pre


def gemm_int_expected(pre, resid, epi, rows):
    v = pre[:rows]
    if epi == "resid":
        v = v + resid[:rows].double()
    return v.float() if epi == "f32" else v.float().to(torch.bfloat16)


def gemm_gelu_probe():
    """-> (a bf16 [385, 128], w float32 [128, 128], bias float32 [128], pre float64 [385, 128]).  Row i carries x_i = -6 + i / 32 in
    column 0 (8 significant bits at most) and w[j][0] = 1, bias[j] = j 2^-12: the pre-activation x_i + j 2^-12 has 15 significant
    bits, exact in float32, and sweeps [-6, 6 + 1/32) in steps of 2^-12."""
    a = torch.zeros(385, 128)
    a[:, 0] = -6.0 + torch.arange(385) / 32.0
    w = torch.zeros(128, 128)
    w[:, 0] = 1.0
    bias = torch.arange(128).float() * 2.0 ** -12
    ab = a.to(torch.bfloat16)
    assert torch.equal(ab.float(), a)
    return ab, w, bias, a[:, :1].double() + bias.double()[None, :]


def strided(t, ld, fill):
    """A copy of the 2-d tensor t as the leading columns of a fresh [rows, ld] buffer filled with `fill` -> (view, buffer)."""
    buf = torch.full((t.shape[0], ld), fill, dtype=t.dtype, device=t.device)
    buf[:, : t.shape[1]] = t
    return buf[:, : t.shape[1]], buf
