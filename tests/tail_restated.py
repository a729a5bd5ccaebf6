"""One link of the bf16 cls-row tail (csrc/azk_nn.hip k_tail_gemm through azk_nn_tail_gemm, csrc/azk_tail.hip k_tail_lds through
azk_nn_tail_gemm_lds), restated on the CPU.  Test infrastructure: no GPU, no libazk (azk.pack_linear_weight is plain tensor code).

  * LINKS: every dispatch row of the two entry points, with the K split (NWK waves) its instantiation uses.
  * probes (`probe`): inputs whose float32 arithmetic is exact in any summation order - a one-hot selection, a count of 255 ones, an
    integer matmul (with its row statistics and a value column whose tanh argument is exactly 0 in every fourth row) - and inputs held
    to a float64 reference: randn operands for the plain links, scaled copies of one row with exact statistics for the LayerNorm links.
  * `expected`: the float64 reference, the error bound a correct kernel meets (each term derived where it is computed) and, for the
    exact probes, the bits.
  * `tail_emulate`: the link's float32 arithmetic as the kernels' sources state it, from the PACKED weight, taking one deliberate
    mistake (`mutate=`): tests/test_tail_restated.py shows that each probe notices the mistake it is there for.  (`unpack` is the
    packer's inverse, so the emulation on the packed weight equals the emulation on the plain one and says nothing about the packer:
    what checks the packer against the kernels' fragment reads is the GPU file, whose expected values come from the plain weight.)

Unit roundoffs: bf16 round-to-nearest is within 2^-9 relative (block_restated's U16 = 2^-8 is kept for the output store, as there);
float32 u = 2^-24."""
import functools

import numpy as np
import torch

import block_restated as br
from block_restated import U16, U32, bf16, bits  # noqa: F401

EPI = {"bf16": 0, "gelu": 1, "resid": 2, "heads": 3}          # azk.TAIL_*
LN_EPS = 1e-5
SENTINEL = 7.0
MUTATIONS = ("reduce3", "a_first_range", "stats_half", "resid_ldo", "bias_no_batch", "lds_chain")

# Largest |tanhf(x) - tanh(x)| of the HEADS epilogue on an MI355X over the value-column probe's arguments (multiples of 2^-6 in
# (-4, 4), exact in float32, so the error is tanhf's alone): 0.929 x 2^-24, the same at every action_dim of ACTION_DIMS;
# test_gpu_tail_pinned.py's test_heads_value_column prints it (TANHF <largest error / 2^-24>).  The value head is allowed four times
# that.  This is the one number here that the formats do not give.
TANHF_ERR_MEASURED = 0.929 * U32
TANHF_MARGIN = 4.0 * TANHF_ERR_MEASURED

# name -> k, layernorm of A, epilogue, NWK (waves the K range is split over; their partial sums are added in the order 0..NWK-1),
# batches, the output widths the tests use (64 / 128: one wave column, two; 2048: the "wide" 2 x 2-wave instantiations; 512 for the
# LDS link 4: eight column tiles, the XCD-row block mapping), LDS form.
# Four register instantiations choose their wave tile (32, 48 or 64 rows: RT = 2, 3, 4) in the kernel: RT goes up while
# ceil(live / (16 RT NWR)) NWR (N / 64) nbatch NWK exceeds the waves the chip holds at once (one per SIMD for these: 1024 on a
# 256-CU part).  The wide GELU links (N = 2048, NWR = 2) and the K = 2048 links at N = 512 (NWK = 4) put 32 waves on a strip, so RT = 3
# starts above 1024 live rows and RT = 4 above 1536; at N = 64 / 128 the K = 2048 links never leave RT = 2, which is why they also
# run at 512.
LINKS = {
    "k384_bf16_b8":     dict(k=384, ln=False, epi="bf16", nwk=4, nbatch=8, n_outs=(64, 128), lds=False),
    "k512_bf16":        dict(k=512, ln=False, epi="bf16", nwk=4, nbatch=1, n_outs=(64, 128), lds=False),
    "k512_bf16_b8":     dict(k=512, ln=False, epi="bf16", nwk=4, nbatch=8, n_outs=(64, 128), lds=False),
    "k512_gelu":        dict(k=512, ln=False, epi="gelu", nwk=1, nbatch=1, n_outs=(64, 128, 2048), lds=False),
    "k512_resid":       dict(k=512, ln=False, epi="resid", nwk=1, nbatch=1, n_outs=(64, 128), lds=False),
    "k512_heads":       dict(k=512, ln=False, epi="heads", nwk=1, nbatch=1, n_outs=(256,), lds=False),
    "k512_ln_gelu":     dict(k=512, ln=True, epi="gelu", nwk=1, nbatch=1, n_outs=(64, 128, 2048), lds=False),
    "k512_ln_bf16":     dict(k=512, ln=True, epi="bf16", nwk=1, nbatch=1, n_outs=(64, 128), lds=False),
    "k512_ln_heads":    dict(k=512, ln=True, epi="heads", nwk=4, nbatch=1, n_outs=(256,), lds=False),
    "k2048_resid":      dict(k=2048, ln=False, epi="resid", nwk=4, nbatch=1, n_outs=(64, 128, 512), lds=False),
    "k2048_bf16":       dict(k=2048, ln=False, epi="bf16", nwk=4, nbatch=1, n_outs=(64, 128, 512), lds=False),
    "lds_k512_ln_gelu": dict(k=512, ln=True, epi="gelu", nwk=1, nbatch=1, n_outs=(128, 2048), lds=True),
    "lds_k2048_resid":  dict(k=2048, ln=False, epi="resid", nwk=4, nbatch=1, n_outs=(64, 128, 512), lds=True),
}
PLAIN = tuple(n for n, L in LINKS.items() if not L["ln"])
LNA = tuple(n for n, L in LINKS.items() if L["ln"])
ACTION_DIMS = (63, 64, 225, 226, 227, 228, 255)     # all four lane residues (a lane holds four columns), both sides of a 64-column group, action_dim + 1 == n_out


def heads_n_out(action_dim):
    return (action_dim + 1 + 63) // 64 * 64


def pack(w):
    """azk.pack_linear_weight on a CPU tensor (the binding's helpers ask for a GPU; the packer itself is tensor arithmetic)."""
    import azk
    saved = azk._torch
    azk._torch = lambda: torch
    try:
        return azk.pack_linear_weight(w.cpu())
    finally:
        azk._torch = saved


def unpack(wp, rows, k):
    """The packed weight as float32 [rows, k], read the way a wave reads it: fragment tile (group g, k-step s, tile c) holds, in lane
    (l4, l15), the eight k values 32 s + 8 l4 .. + 7 of output column 64 g + 4 l15 + c."""
    return wp.cpu().view(rows // 64, k // 32, 4, 4, 16, 8).permute(0, 4, 2, 1, 3, 5).reshape(rows, k).float()


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_stats_f32(a_stats, k, eps, half=False):
    """(mean, rstd) in float32 from [m, 8, 2] (sum, sum of squares) groups, added as both kernels add them:
    ((g0 + g1) + (g2 + g3)) + ((g4 + g5) + (g6 + g7)).  half: the lane's first group only, i.e. groups 0, 2, 4, 6."""
    st = a_stats.cpu().float()
    g = [st[:, i, :] for i in range(8)]
    if half:
        s = (g[0] + g[2]) + (g[4] + g[6])
    else:
        s = ((g[0] + g[1]) + (g[2] + g[3])) + ((g[4] + g[5]) + (g[6] + g[7]))
    inv = np.float32(1.0 / k)
    mean = s[:, 0:1] * inv
    rstd = torch.rsqrt(torch.clamp(s[:, 1:2] * inv - mean * mean, min=0.0) + np.float32(eps))
    return mean, rstd


def tail_emulate(a, wp, n_out, k, epi, nwk=1, nbatch=1, a_batch_stride=0, bias=None, resid=None, a_stats=None, eps=LN_EPS,
                 action_dim=0, col_sums=None, ldo=None, mutate=None):
    """-> {'out': bf16 [m, nbatch n_out], 'stats': float32 [m, nbatch n_out / 64, 2]} or {'logits', 'values'} for HEADS.
    a: bf16 [m, >= k] (a strided view is fine); wp: pack() of the [nbatch n_out, k] weight; col_sums given: the LDS link 3, LayerNorm
    applied in the epilogue as rstd (x W^T - mean csum) on the un-normalised rows; otherwise a_stats normalises A on the fly and the
    normalised fragment is rounded to bf16.  resid may be a strided view.
    mutate: 'reduce3' / 'lds_chain' (the last K range's partial never joins the sum: the register form's reduction loop, the LDS
    form's fixed-order chain sum), 'a_first_range' (every wave reads A's first K range against its own weight range), 'stats_half'
    (half the statistics' groups), 'resid_ldo' (the residual row found with the OUTPUT's leading dimension `ldo`), 'bias_no_batch'
    (every batch reads batch 0's bias)."""
    assert mutate is None or mutate in MUTATIONS
    assert k % (32 * nwk) == 0
    m = a.shape[0]
    af = a.detach().cpu().float()
    W = unpack(wp, nbatch * n_out, k)
    kq = k // nwk
    lds3 = col_sums is not None
    if a_stats is not None:
        mean, rstd = ln_stats_f32(a_stats, k, eps, half=(mutate == "stats_half"))
    acc = torch.zeros(m, nbatch * n_out)
    for b in range(nbatch):
        x = af[:, b * a_batch_stride: b * a_batch_stride + k]
        if a_stats is not None and not lds3:
            x = bf16(x * rstd + (-mean * rstd))
        tot = None
        for w in range(nwk):
            if mutate in ("reduce3", "lds_chain") and nwk > 1 and w == nwk - 1:
                continue
            ka = 0 if mutate == "a_first_range" else w * kq
            part = x[:, ka: ka + kq] @ W[b * n_out: (b + 1) * n_out, w * kq: (w + 1) * kq].t()
            tot = part if tot is None else tot + part
        acc[:, b * n_out: (b + 1) * n_out] = tot
    bv = torch.zeros(nbatch * n_out) if bias is None else bias.detach().cpu().float()[: nbatch * n_out]
    if mutate == "bias_no_batch":
        bv = bv[:n_out].repeat(nbatch)
    if lds3:
        v = acc * rstd - (mean * rstd) * col_sums.detach().cpu().float()[None, : n_out] + bv
    else:
        v = acc + bv
    if epi == "heads":
        return {"logits": v[:, :action_dim].contiguous(), "values": torch.tanh(v[:, action_dim]).contiguous()}
    if epi == "gelu":
        v = br.gelu_erf_f32(v)
    if epi == "resid":
        r = resid.detach().cpu()
        if mutate == "resid_ldo":
            r = torch.as_strided(r, (m, nbatch * n_out), (ldo, 1))
        v = v + r.float()
    out = v.to(torch.bfloat16)
    r = out.float().view(m, nbatch * n_out // 64, 64)
    return {"out": out, "stats": torch.stack([r.sum(2), (r * r).sum(2)], dim=2).contiguous()}


# ---------------------------------------------------------------------------------------------------------------------------------
# probes
# ---------------------------------------------------------------------------------------------------------------------------------
def full_bf16(shape, rng):
    """Random bf16 numbers with full significands: +-(128 .. 255) 2^e, e in -13 .. -7, so |x| in [2^-6, 4) on the grid 2^-13."""
    v = (128 + rng.randint(0, 128, size=shape)) * np.exp2(rng.randint(-13, -6, size=shape)) * rng.choice([-1.0, 1.0], size=shape)
    return torch.from_numpy(v.astype(np.float32))


def select_k(r, b, k):
    """The k slot row r of batch b selects: 37 is prime to 384, 512 and 2048, so k consecutive rows hit every slot, and 65 rows
    already land in every wave's K range."""
    return (37 * r + 101 * b) % k


def _select(L, n_out, m, rng):
    k, nb = L["k"], L["nbatch"]
    w = full_bf16((nb * n_out, k), rng)
    a = torch.zeros(m, nb * k)
    r = np.arange(m)
    pre = torch.zeros(m, nb * n_out, dtype=torch.float64)
    for b in range(nb):
        p = select_k(r, b, k)
        val = 1.0 + ((r // 3 + b) & 1)
        a[r, b * k + p] = torch.from_numpy(val).float()
        pre[:, b * n_out: (b + 1) * n_out] = w[b * n_out: (b + 1) * n_out][:, p].t().double() * torch.from_numpy(val)[:, None]
    return dict(a=a.to(torch.bfloat16), w=w, bias=None, resid=torch.zeros(m, nb * n_out, dtype=torch.bfloat16), pre=pre, S=pre.abs(), exact=True)


def _count(L, n_out, m, rng):
    """W: 255 ones in every output column's K range, floor(255 / steps) or one more in every 32-wide k-step."""
    k, nb = L["k"], L["nbatch"]
    rows, steps = nb * n_out, k // 32
    cnt = np.full((rows, steps), 255 // steps)
    cnt += np.argsort(np.argsort(rng.random_sample((rows, steps)), axis=1), axis=1) < 255 % steps
    w = (np.argsort(np.argsort(rng.random_sample((rows, steps, 32)), axis=2), axis=2) < cnt[:, :, None]).reshape(rows, k)
    assert (w.sum(1) == 255).all() and (w.reshape(rows, steps, 32).sum(2) >= 1).all()
    pre = torch.full((m, rows), 255.0, dtype=torch.float64)
    return dict(a=torch.ones(m, nb * k, dtype=torch.bfloat16), w=torch.from_numpy(w.astype(np.float32)), bias=None,
                resid=torch.zeros(m, rows, dtype=torch.bfloat16), pre=pre, S=pre.clone(), exact=True)


def _int(L, n_out, m, rng, action_dim=None):
    """a in -2 .. 2, w in {-1, 0, 1} (half of it 0), integer bias (|.| <= 8) and residual (|.| <= 16): every partial sum is an integer
    below 2^13.  HEADS: the value column's weights are scaled by 2^-6, its bias is 0, and in every fourth row one element of a is
    moved so that the column's pre-activation is exactly 0 there (tanh 0 = 0); the other rows hold multiples of 2^-6."""
    k, nb = L["k"], L["nbatch"]
    a = torch.from_numpy(rng.randint(-2, 3, size=(m, nb * k)).astype(np.float32))
    w = torch.from_numpy((rng.randint(-1, 2, size=(nb * n_out, k)) * rng.randint(0, 2, size=(nb * n_out, k))).astype(np.float32))
    bias = torch.from_numpy(rng.randint(-8, 9, size=(nb * n_out,)).astype(np.float32))
    resid = torch.from_numpy(rng.randint(-16, 17, size=(m, nb * n_out)).astype(np.float32)).to(torch.bfloat16)
    if action_dim is not None:
        j = int(w[action_dim].abs().argmax())
        assert abs(float(w[action_dim, j])) == 1.0
        rows = torch.arange(0, m, 4)
        a[rows, j] -= (a[rows] @ w[action_dim]) * w[action_dim, j]
        assert float(a.abs().max()) <= 256.0
        w[action_dim] *= 2.0 ** -6
        bias[action_dim] = 0.0
    pre = torch.zeros(m, nb * n_out, dtype=torch.float64)
    S = torch.zeros_like(pre)
    for b in range(nb):
        sl = slice(b * n_out, (b + 1) * n_out)
        ab, wb = a[:, b * k: (b + 1) * k].double(), w[sl].double()
        pre[:, sl] = ab @ wb.t() + bias[sl].double()
        S[:, sl] = ab.abs() @ wb.abs().t() + bias[sl].double().abs()
    return dict(a=a.to(torch.bfloat16), w=w, bias=bias, resid=resid, pre=pre, S=S, exact=True)


def _randn(L, n_out, m, rng):
    k, nb = L["k"], L["nbatch"]
    a = bf16(torch.from_numpy(rng.standard_normal((m, nb * k)).astype(np.float32)) * 0.7)
    w = bf16(torch.from_numpy(rng.standard_normal((nb * n_out, k)).astype(np.float32)) / k ** 0.5)
    bias = torch.from_numpy(rng.standard_normal(nb * n_out).astype(np.float32)) * 0.2
    resid = torch.from_numpy(rng.standard_normal((m, nb * n_out)).astype(np.float32)).to(torch.bfloat16)
    pre = torch.zeros(m, nb * n_out, dtype=torch.float64)
    S = torch.zeros_like(pre)
    for b in range(nb):
        sl = slice(b * n_out, (b + 1) * n_out)
        ab, wb = a[:, b * k: (b + 1) * k].double(), w[sl].double()
        pre[:, sl] = ab @ wb.t() + bias[sl].double()
        S[:, sl] = ab.abs() @ wb.abs().t() + bias[sl].double().abs()
    return dict(a=a.to(torch.bfloat16), w=w, bias=bias, resid=resid, pre=pre, S=S, exact=False)


def _ln(L, n_out, m, rng):
    """LayerNorm links.  Row r is one pattern x0 (integers -100 .. 155 over 16) times 2^(r mod 5): the groups' sums and sums of
    squares are exact in float32 (multiples of 2^-4 and 2^-8 below 2^24 of them), and the normalised row is the same for every r up
    to what eps does.  Statistics of another row are off by a power of two, half the groups by about two - not by a rounding.
    -> pre (float64), err: the bound on the pre-activation's error, derived here.

    float32 operations behind rstd and shift, u = 2^-24 (both kernels; s1, s2 the row's sum and sum of squares, E2 = s2 / K):
      s1, s2     three additions each on the exact groups: relative 3 u.  x 1/K is exact (a power of two).
      var + eps  mean^2: 2 x 3 u + 1 for the product = 7 u mean^2;  E2: 3 u E2;  the difference: u |var| <= u E2;  + eps: u (var + eps)
                 -> |d(var + eps)| <= u (4 E2 + 7 mean^2 + var + eps) =: u V
      rstd       rho = u (V / (2 (var + eps)) + 2)   (the inverse root halves the relative error; rsqrtf within 2 u)
      shift      -mean rstd: rho + 3 u (the mean) + u (the product)
    Register form (A normalised on the fly, v = x rstd + shift, then rounded to bf16):
      |dv|  <= (rho + 4 u) rstd (|x| + |mean|) + 2 u (|x| rstd + |mean| rstd)         (one or two roundings for the multiply-add)
            <= (rho + 6 u) rstd (|x| + |mean|)
      the bf16 rounding of v: 2^-9 (|xhat| + |dv|)
      the product over K: (K + 2) u S with S = |xhat| |w| + |b|
      err = sum_k (|dv| + 2^-9 (|xhat| + |dv|)) |w| + (K + 2) u S
    LDS link 3 (rstd (x W^T) - (mean rstd) csum + b on the stored rows, no re-rounding of A):
      x W^T        K u |x| |w|, then x rstd: (rho + u) on at most rstd |x| |w|
      mean rstd    rho + 4 u; csum is a float64 sum rounded once (u); their product u: (rho + 6 u) |mean| rstd |csum|
      two additions: 2 u (rstd |x| |w| + |mean| rstd |csum| + |b|)
      err = rstd |x| |w| ((K + 3) u + rho) + |mean| rstd |csum| (rho + 8 u) + 2 u |b|"""
    k = L["k"]
    x0 = torch.from_numpy(rng.randint(-100, 156, size=k).astype(np.float64)) / 16.0
    scale = torch.from_numpy(np.exp2(np.arange(m) % 5))[:, None]
    x = x0[None, :] * scale
    a = x.float().to(torch.bfloat16)
    assert torch.equal(a.double(), x)
    g = x.view(m, 8, 64)
    st64 = torch.stack([g.sum(2), (g * g).sum(2)], dim=2)
    a_stats = st64.float().contiguous()
    assert torch.equal(a_stats.double(), st64)
    w = bf16(torch.from_numpy(rng.standard_normal((n_out, k)).astype(np.float32)) / k ** 0.5)
    bias = torch.from_numpy(rng.standard_normal(n_out).astype(np.float32)) * 0.2
    wd, bd = w.double(), bias.double()
    mean = x.mean(1, keepdim=True)
    E2 = (x * x).mean(1, keepdim=True)
    var = E2 - mean * mean
    rstd = 1.0 / torch.sqrt(var + LN_EPS)
    xhat = (x - mean) * rstd
    pre = xhat @ wd.t() + bd
    V = 4 * E2 + 7 * mean * mean + var + LN_EPS
    rho = U32 * (V / (2 * (var + LN_EPS)) + 2)
    if L["lds"]:
        csum = wd.sum(1)
        err = rstd * (x.abs() @ wd.abs().t()) * ((k + 3) * U32 + rho) + mean.abs() * rstd * csum.abs()[None, :] * (rho + 8 * U32) + 2 * U32 * bd.abs()
    else:
        dv = (rho + 6 * U32) * rstd * (x.abs() + mean.abs())
        S = xhat.abs() @ wd.abs().t() + bd.abs()
        err = (dv + 2.0 ** -9 * (xhat.abs() + dv)) @ wd.abs().t() + (k + 2) * U32 * S
    return dict(a=a, w=w, bias=bias, resid=None, a_stats=a_stats, pre=pre, err=err, exact=False)


_KINDS = {"select": _select, "count": _count, "int": _int, "randn": _randn, "ln": _ln}


@functools.lru_cache(maxsize=None)
def probe(kind, link, n_out, m, action_dim=None):
    """The probe of one kind for one link at m rows (rows are independent: a test may use any prefix).  Cached and never changed.
    Besides the builders' fields: wp (the packed weight), err (bound on the pre-activation's error; plain links: block_restated's
    (K + 2) u S), col_sums for the LDS link 3."""
    L = LINKS[link]
    assert (kind == "ln") == L["ln"]
    rng = np.random.RandomState(sorted(_KINDS).index(kind) * 1000003 + sorted(LINKS).index(link) * 10007 + n_out * 13 + (action_dim or 0))
    p = _KINDS[kind](L, n_out, m, rng, action_dim) if kind == "int" else _KINDS[kind](L, n_out, m, rng)
    p["wp"] = pack(p["w"])
    if "err" not in p:
        p["err"] = (L["k"] + 2) * U32 * p["S"]
    if L["lds"] and L["ln"]:
        p["col_sums"] = unpack(p["wp"], n_out, L["k"]).double().sum(1).float().contiguous()
    return p


def exactness(p, L, epi):
    """The conditions an exact probe rests on, for the test that asserts them: (largest sum of |a| |w| + |bias| + |resid|, whether
    every value a bf16 epilogue stores has at most 8 significant bits, largest 64-column sum of squares of the stored values)."""
    S = p["S"] + (p["resid"].double().abs() if epi == "resid" else 0)
    stored = p["pre"] + (p["resid"].double() if epi == "resid" else 0)
    fits = bool(torch.equal(bf16(stored.float()).double(), stored))
    sq = (stored * stored).view(stored.shape[0], -1, 64).sum(2)
    return float(S.max()), fits, float(sq.max())


def expected(p, L, rows=None, action_dim=None):
    """-> dict for the first `rows` rows.  bf16 epilogues: ref, bound (float64 [rows, N]) and, for exact probes through BF16 / RESID, out
    (the bits) and stats (float32 [rows, N / 64, 2]: sums and sums of squares of the stored values).  HEADS: logits_ref, logits_bound,
    logits (exact probes), values_ref, values_bound, values_arg (the tanh argument).
      BF16, RESID  2^-8 |ref| + err                 (block_restated.gemm_bound; the residual joins S)
      GELU         2^-8 |ref| + |x| / 2 GELU_ERF_ERR + 1.13 err
      logits       2^-24 |ref| + err                (float32 store)
      value        err + TANHF_MARGIN               (|tanh'| <= 1 carries err through; the margin is tanhf's own, see above)"""
    epi = L["epi"]
    rows = p["pre"].shape[0] if rows is None else rows
    pre, err = p["pre"][:rows], p["err"][:rows]
    if epi == "heads":
        e = dict(logits_ref=pre[:, :action_dim], logits_bound=U32 * pre[:, :action_dim].abs() + err[:, :action_dim],
                 values_arg=pre[:, action_dim], values_ref=torch.tanh(pre[:, action_dim]), values_bound=err[:, action_dim] + TANHF_MARGIN)
        if p["exact"]:
            e["logits"] = pre[:, :action_dim].float().contiguous()
        return e
    if epi == "gelu":
        ref = torch.nn.functional.gelu(pre)
        return dict(ref=ref, bound=U16 * ref.abs() + 0.5 * pre.abs() * br.GELU_ERF_ERR + 1.13 * err)
    if epi == "resid":
        r = p["resid"][:rows].double()
        ref = pre + r
        err = err + (L["k"] + 2) * U32 * r.abs()
    else:
        ref = pre
    e = dict(ref=ref, bound=U16 * ref.abs() + err)
    if p["exact"]:
        out = ref.float().to(torch.bfloat16)
        g = out.double().view(rows, -1, 64)
        e["out"] = out
        e["stats"] = torch.stack([g.sum(2), (g * g).sum(2)], dim=2).float().contiguous()
    return e


def call_kwargs(p, L, n_out, rows, action_dim=None):
    """What both azk.nn_tail_gemm and tail_emulate take besides (a, wp, n_out, k, epilogue) and the output buffers."""
    kw = dict(nbatch=L["nbatch"], a_batch_stride=L["k"] if L["nbatch"] > 1 else 0, bias=p["bias"])
    if L["epi"] == "resid":
        kw["resid"] = p["resid"][:rows]
    if L["ln"]:
        kw["a_stats"] = p["a_stats"][:rows]
        if L["lds"]:
            kw["col_sums"] = p["col_sums"]
    if L["epi"] == "heads":
        kw["action_dim"] = action_dim
    return kw


def emulate(p, L, n_out, rows, action_dim=None, mutate=None, **over):
    kw = call_kwargs(p, L, n_out, rows, action_dim)
    kw.update(over)
    return tail_emulate(p["a"][:rows], p["wp"], n_out, L["k"], L["epi"], nwk=L["nwk"], mutate=mutate, **kw)


def worst_ratio(err, bound):
    """max err / bound, with 0 / 0 = 0 (an exact result where the bound is 0) and x / 0 = inf."""
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max()) if r.numel() else 0.0
