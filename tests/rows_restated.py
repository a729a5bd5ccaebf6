"""The library tail's last launch (csrc/azk_rows.hip): k_ln_heads through azk_nn_ln_heads - final LayerNorm, merged policy / value head
and tanh in one launch - and its unfused read-out k_heads_finalize through azk_nn_heads_finalize, restated on the CPU.  Test
infrastructure: no GPU, no libazk (azk.pack_linear_weight is plain tensor code).  It reuses tests/tail_restated.py (pack, unpack,
ACTION_DIMS, heads_n_out, TANHF_MARGIN, worst_ratio, SENTINEL) and tests/block_restated.py (ln_rows).

  * `ln_heads_emulate`: the kernel's float32 arithmetic as the source states it, from the PACKED weight, taking one deliberate mistake
    (`mutate=`); tests/test_rows_restated.py shows which probe notices which mistake.
  * `balanced`: the exact probe.  Its float32 arithmetic is exact in any order up to rsqrtf, and what rsqrtf's last bits do is removed
    by the bf16 rounding of the normalised fragment: the logits are integers, known bit for bit.
  * `probe`: rows of five kinds against a float64 reference, with a bound derived term by term in `ln_heads_f64`.
  * `finalize_probe`: k_heads_finalize's input and expected output.

Unit roundoffs: float32 u = 2^-24; bf16 round-to-nearest moves a number by at most half an ulp of its binade (`bf16_half_ulp`: between
2^-9 and 2^-8 relative)."""
import functools

import numpy as np
import torch

import block_restated as br
from block_restated import U32, bf16
from tail_restated import ACTION_DIMS, SENTINEL, TANHF_MARGIN, heads_n_out, pack, unpack, worst_ratio  # noqa: F401

LN_EPS = 1e-5                                                 # the ABI's default eps (azk.nn_ln_heads)
WIDTHS = (256, 512)                                           # k_ln_heads<8>, k_ln_heads<16>
ONE_GROUP = (7, 9, 49)                                        # action_dim + 1 <= 64: one 64-column group
SEVEN_GROUPS = (399, 400)                                     # n_out = 448: an odd group count against the four waves of a block
EXACT_ACTION_DIMS = ONE_GROUP + ACTION_DIMS + SEVEN_GROUPS
F64_ACTION_DIMS = (49, 225, 400)
MUTATIONS = ("stats_half", "stale_fragment", "bias_group0", "no_mean_sq", "shift_sign", "value_lane", "no_tanh", "live_guard")
KINDS = ("pattern", "random", "onehot", "constant", "mean100_ulp")
BALANCED_M0 = (0.0, 3.0, -12.0)
BALANCED_S = (0.5, 1.0, 4.0)
POISON = -1536.0                                              # finalize_probe: what the columns behind the value column hold


# ---------------------------------------------------------------------------------------------------------------------------------
# the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
def ln_heads_stats_f32(xv, eps, mutate=None):
    """k_ln_heads' statistics -> (mean, rstd, shift), float32 [rows, 4]: one column per lane group l4 (all four are equal unless a
    mutation separates them).  Lane (l15, l4) of a wave holds, for row l15 of the tile, k = 32 ks + 8 l4 + 0 .. 7 of every k-step ks as
    four (lo, hi) pairs; s1 += lo + hi and s2 += lo lo + hi hi run over ks (outer) and the pair q (inner); the xor-16 shuffle adds lane
    groups 0 + 1 and 2 + 3, the xor-32 shuffle the two halves."""
    rows, K = xv.shape
    KT = K // 32
    lanes = xv.view(rows, KT, 4, 4, 2)                        # ks, l4, q, (lo, hi)
    s1 = torch.zeros(rows, 4)
    s2 = torch.zeros(rows, 4)
    for ks in range(KT):
        for q in range(4):
            lo, hi = lanes[:, ks, :, q, 0], lanes[:, ks, :, q, 1]
            s1 = s1 + (lo + hi)
            s2 = s2 + (lo * lo + hi * hi)
    s1 = s1 + s1[:, [1, 0, 3, 2]]
    s2 = s2 + s2[:, [1, 0, 3, 2]]
    if mutate != "stats_half":
        s1 = s1 + s1[:, [2, 3, 0, 1]]
        s2 = s2 + s2[:, [2, 3, 0, 1]]
    inv = np.float32(1.0 / K)
    mean = s1 * inv
    var = s2 * inv if mutate == "no_mean_sq" else s2 * inv - mean * mean
    rstd = torch.rsqrt(torch.clamp(var, min=0.0) + np.float32(eps))
    shift = mean * rstd if mutate == "shift_sign" else -mean * rstd
    return mean, rstd, shift


def ln_heads_emulate(x, wp, bias, n_out, action_dim, eps=LN_EPS, count=None, mutate=None):
    """-> (logits float32 [n, action_dim], values float32 [n]) with SENTINEL in the rows at or beyond the live count min(n, count).
    x: bf16 [n, K], K = 256 or 512; wp: pack() of the [n_out, K] weight; bias: float32 [n_out].
    v = x rstd + shift is rounded to bf16, multiplied with the weight in float32, the bias added, tanh taken on column action_dim.
    mutate:
      stats_half      no xor-32 add: lane groups 0, 1 normalise with the sums over their own half of the row, groups 2, 3 with theirs
      stale_fragment  the `bf = nb` rotation skipped: k-steps >= 4 multiply with the weight fragments of k-steps 0 .. 3 again
      bias_group0     bias read at 4 l15 + c rather than 64 ng + 4 l15 + c
      no_mean_sq      var = E2
      shift_sign      shift = +mean rstd
      value_lane      tanh / value taken at column action_dim + 1 (never written when that is n_out)
      no_tanh         the value stored raw
      live_guard      the rows of the last 16-row tile at or beyond the count are written (they hold the last live row's result: the
                      kernel clamps the row it reads), as far as the buffer reaches"""
    assert mutate is None or mutate in MUTATIONS
    xf = x.detach().cpu().float()
    n, K = xf.shape
    assert K in WIDTHS and n_out % 64 == 0 and action_dim + 1 <= n_out
    KT = K // 32
    nvalid = n if count is None else min(n, int(count))
    logits = torch.full((n, action_dim), SENTINEL)
    values = torch.full((n,), SENTINEL)
    if nvalid <= 0:
        return logits, values
    xv = xf[:nvalid].contiguous()
    mean, rstd, shift = ln_heads_stats_f32(xv, eps, mutate)
    v = bf16(xv.view(nvalid, KT, 4, 8) * rstd[:, None, :, None] + shift[:, None, :, None]).view(nvalid, K)
    W = unpack(wp, n_out, K)
    if mutate == "stale_fragment":
        W = W.view(n_out, KT, 32)[:, torch.arange(KT) % 4].reshape(n_out, K)
    b = bias.detach().cpu().float()[:n_out]
    if mutate == "bias_group0":
        b = b[:64].repeat(n_out // 64)
    out = v @ W.t() + b
    vcol = action_dim + 1 if mutate == "value_lane" else action_dim
    val = out[:, vcol] if vcol < n_out else None
    if val is not None and mutate != "no_tanh":
        val = torch.tanh(val.double()).float()
    logits[:nvalid] = out[:, :action_dim]
    if val is not None:
        values[:nvalid] = val
    if mutate == "live_guard":
        end = min((nvalid + 15) // 16 * 16, n)
        logits[nvalid:end] = out[nvalid - 1, :action_dim]
        if val is not None:
            values[nvalid:end] = val[nvalid - 1]
    return logits, values


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact probe
# ---------------------------------------------------------------------------------------------------------------------------------
def _ulps(r, k):
    """float32 tensor r moved by k units in the last place."""
    return (r.view(torch.int32) + k).view(torch.float32)


@functools.lru_cache(maxsize=None)
def balanced_margin(eps):
    """The condition the exact probe rests on, for all nine (m0, s): with mean = m0 and var = s^2 exact, v = x rstd + shift for
    x = m0 +- s is rounded to exactly +-1 by the bf16 conversion - for every rstd within 8 float32 ulp of 1 / sqrt(s^2 + eps), with the
    multiply-add fused (one rounding) or not (two).  bf16 rounds everything in (1 - 2^-9, 1 + 2^-8) to 1.
    -> the largest |v -+ 1| seen.  It is eps / (2 s^2) (2e-5 at s = 0.5, eps = 1e-5; nothing at eps = 0) plus the roundings of
    x rstd and mean rstd, two float32 ulps at 25 = 2^-18 at most (m0 = -12, s = 0.5: rstd = 2, the products are near 25 and 24):
    far inside 2^-9 either way, which is asserted."""
    worst = 0.0
    for m0 in BALANCED_M0:
        for s in BALANCED_S:
            r0 = torch.tensor([1.0 / np.sqrt(np.float64(s) ** 2 + eps)], dtype=torch.float64).float()
            for k in range(-8, 9):
                rstd = _ulps(r0, k)
                shift = -torch.tensor([m0]) * rstd
                for sign in (-1.0, 1.0):
                    x = torch.tensor([m0 + sign * s])
                    assert torch.equal(bf16(x), x)
                    unfused = x * rstd + shift
                    fused = (x.double() * rstd.double() + shift.double()).float()
                    for v in (unfused, fused):
                        assert float(bf16(v)) == sign, (m0, s, k, float(v))
                        worst = max(worst, abs(float(v) - sign))
    assert worst < 2.0 ** -10
    return worst


@functools.lru_cache(maxsize=None)
def balanced(D, action_dim, m=256):
    """The exact probe at width D for one action_dim: m rows (rows are independent: a test may use any prefix, or tile the first 64).
    Row r is m0 + s sigma[r, :] with sigma balanced +-1 (D / 2 of each sign, drawn per row), m0 = (0, 3, -12)[r mod 3],
    s = (0.5, 1, 4)[(r div 3) mod 3]: all nine pairs in nine rows.  W in {-1, 0, 1} (half of it 0) over all n_out columns, the
    padding behind the value column included; integer bias, |.| <= 8.  The value column (row action_dim of W) has D / 2 entries
    +-2^-6 and bias 0; in every fourth row sigma agrees with its sign on half of them and disagrees on the other half, so the tanh
    argument is exactly 0 there; elsewhere it is a multiple of 2^-6 in (-4, 4).
    Why the logits are known bit for bit (asserted here):
      x is a multiple of 1/2 with |x| <= 16, x^2 a multiple of 1/4 up to 256: every partial sum of either, in any order, is a multiple
      of the quantum below 2^24 quanta - exact in float32.  sum x = D m0 and sum x^2 = D (m0^2 + s^2) (the cross term cancels over a
      balanced row), so mean = m0, E2 - mean^2 = s^2, both exact; rsqrtf's result is the first inexact number, and `balanced_margin`
      shows that v rounds to sigma exactly whatever its last bits are.  The product sigma W^T + b is an integer below 2^10.
    -> x (bf16), w, wp, bias, pre (float64 [m, n_out]: the integers, the value column scaled), sigma."""
    assert D in WIDTHS and m % 4 == 0
    n_out = heads_n_out(action_dim)
    rng = np.random.RandomState(D * 1009 + action_dim)
    w = (rng.randint(-1, 2, size=(n_out, D)) * rng.randint(0, 2, size=(n_out, D))).astype(np.float64)
    bias = rng.randint(-8, 9, size=n_out).astype(np.float64)
    wa = np.zeros(D)
    nz = rng.permutation(D)[: D // 2]
    wa[nz] = rng.choice([-1.0, 1.0], size=D // 2)
    zero_pos = np.setdiff1d(np.arange(D), nz)
    sigma = np.zeros((m, D))
    for r in range(m):
        if r % 4 == 0:
            agree = rng.permutation(nz)
            sigma[r, agree[: D // 4]] = wa[agree[: D // 4]]
            sigma[r, agree[D // 4:]] = -wa[agree[D // 4:]]
            plus = D // 2 - int((sigma[r] > 0).sum())
            fill = rng.permutation(zero_pos)
            sigma[r, fill[:plus]] = 1.0
            sigma[r, fill[plus:]] = -1.0
        else:
            sigma[r] = rng.permutation(np.repeat([-1.0, 1.0], D // 2))
    assert (np.abs(sigma) == 1).all() and (sigma.sum(1) == 0).all()
    assert len({sigma[r].tobytes() for r in range(m)}) == m   # the signs differ between rows
    t = sigma @ wa
    assert (t[0::4] == 0).all() and (t != 0).any() and np.abs(t).max() < 256
    w[action_dim] = wa * 2.0 ** -6
    bias[action_dim] = 0.0
    r = np.arange(m)
    m0 = np.asarray(BALANCED_M0)[r % 3]
    s = np.asarray(BALANCED_S)[(r // 3) % 3]
    xd = torch.from_numpy(m0[:, None] + s[:, None] * sigma)
    x = xd.float().to(torch.bfloat16)
    assert torch.equal(x.double(), xd)
    # every partial sum exact in any order: multiples of 1/2 (1/4 for the squares), fewer than 2^24 of them
    assert float(xd.abs().sum(1).max()) / 0.5 < 2 ** 24 and float((xd * xd).sum(1).max()) / 0.25 < 2 ** 24
    mean, rstd, _ = ln_heads_stats_f32(x.float(), 0.0)
    assert torch.equal(mean.double(), torch.from_numpy(m0)[:, None].expand(m, 4))
    assert torch.equal(rstd.double(), torch.from_numpy(1.0 / s)[:, None].expand(m, 4))        # var = s^2, a power of four
    for eps in (0.0, LN_EPS):
        balanced_margin(eps)
    wt, bt = torch.from_numpy(w).float(), torch.from_numpy(bias).float()
    pre = torch.from_numpy(sigma @ w.T + bias)
    assert float((torch.from_numpy(np.abs(sigma) @ np.abs(w).T) + bt.abs().double()).max()) < 2 ** 24
    arg = pre[:, action_dim]
    assert torch.equal(arg * 64, (arg * 64).round()) and float(arg.abs().max()) < 4.0
    return dict(x=x, w=wt, wp=pack(wt), bias=bt.contiguous(), pre=pre, sigma=torch.from_numpy(sigma), exact=True, err=torch.zeros_like(pre))


# ---------------------------------------------------------------------------------------------------------------------------------
# float64 reference and bound
# ---------------------------------------------------------------------------------------------------------------------------------
def _quantum(xd):
    """[m, K] float64 holding bf16 numbers -> [m]: the largest power of two that divides every non-zero element of the row."""
    mant, expo = torch.frexp(xd)
    mi = (mant.abs() * 256).round().to(torch.int64)           # 8 significant bits: an integer in 128 .. 255 (0 for 0)
    low = (mi & -mi).double()
    q = torch.ldexp(low, expo - 8)
    q = torch.where(xd == 0, torch.full_like(q, float("inf")), q)
    return q.min(1).values


def sum_roundings(big, q, KT):
    """How many of the additions on an element's way into the kernel's row sum can round.  The terms of a row are multiples of the
    quantum q, at most `big` in size ([m] each).  A partial sum over j terms is a multiple of q of at most j big: exact when
    j big <= 2^24 q.  A lane adds 8 KT terms (one addition for the pair, 4 KT in sequence), the xor-16 shuffle makes it 16 KT, the
    xor-32 shuffle 32 KT = K.  -> [m], between 0 and 4 KT + 3."""
    lim = 2.0 ** 24 * q
    lane = torch.where(8 * KT * big <= lim, 0.0, 4.0 * KT + 1)
    x16 = torch.where(16 * KT * big <= lim, 0.0, 1.0)
    x32 = torch.where(32 * KT * big <= lim, 0.0, 1.0)
    return (lane + x16 + x32).double()


def bf16_half_ulp(a):
    """Half a bf16 ulp at |a| (float64, a >= 0): 2^(e - 8) for a in [2^e, 2^(e + 1)), 0 at 0 - what round-to-nearest can move a by."""
    _, expo = torch.frexp(a)                                  # a = mant 2^expo, mant in [0.5, 1): the binade is [2^(expo - 1), 2^expo)
    return torch.where(a == 0, torch.zeros_like(a), torch.ldexp(torch.ones_like(a), expo - 9))


def ln_heads_f64(x, w, bias, eps=LN_EPS):
    """Float64 LayerNorm (no affine) of the bf16 rows x [m, K] times w^T ([n_out, K]: the values the kernel multiplies with) plus bias
    -> pre, and err: the bound on |kernel's pre-activation - pre|, derived here.  Also xhat, dv and rho (the relative error allowed
    to rstd: where the one-pass statistics' accuracy ends).

    This is tail_restated._ln's register form with the kernel's own summation in place of "three additions on exact groups", and with
    the cancellation term kept in full.  u = 2^-24; A1 = mean |x|, E2 = mean x^2, var = E2 - mean^2, w = var + eps.
      s1        d1 roundings of at most u sum|x| each on an element's path: |d mean| <= dm = d1 u A1 (x 1/K is exact).  d1 counts only
                additions that can round (`sum_roundings`): 0 where the row's partial sums are exact (constant, one-hot, pattern and
                mean-100 rows), 4 KT + 3 for arbitrary rows (pair, 4 KT in sequence, two shuffles).
      s2        the squares of bf16 numbers are exact in float32; all terms are positive: |d E2| <= dE = d2 u E2.
      var + eps mean'^2: 2 |mean| dm + dm^2, its rounding u mean'^2;  the difference: u max(E2', mean'^2) <= u E2';  the clamp at 0
                moves var' towards var >= 0;  + eps: u (var' + eps)
                -> |d(var + eps)| <= D = dE + 2 |mean| dm + dm^2 + u (mean'^2 + E2' + w + ...)
      rstd      the kernel's argument lies in [max(w - D, eps (1 - u)), w + D] (the clamp keeps it at eps or more), rsqrtf is within
                2 u: rstd' in [(1 - 2 u) / sqrt(w + D), (1 + 2 u) / sqrt(max(w - D, eps (1 - u)))] =: [lo, hi], drstd the farther
                end's distance from rstd.  To first order drstd / rstd = D / (2 (var + eps)) + 2 u - _ln's rho with the
                cancellation term V / (2 (var + eps)) - but the interval also holds where D is no longer small against w (constant
                rows: var = 0 and D >> eps).
      v         v' = fl(x rstd' + shift'), shift' = fl(-mean' rstd'):
                |dv| <= |x - mean| drstd + hi dm + 2 u hi (|x| + |mean| + dm)     (the products' roundings and the sum's)
      bf16      h = half a bf16 ulp of |xhat| + |dv|: 2^(e - 8) in the binade [2^e, 2^(e + 1)).  (_ln writes 2^-9 |xhat| here, which is
                half an ulp at the top of a binade only.  Summed over random elements the difference drowns; a one-hot row has one
                xhat of sqrt(D) = 22.6 in [16, 32), half an ulp 2^-4 = 1.42 x 2^-9 x 22.6, and the correct emulation leaves the
                2^-9 form there.)
      product   (K + 2) u S over the rounded fragment, S = (|xhat| + |dv| + h) |w| + |b|
      err = sum_k (|dv| + h) |w| + (K + 2) u S"""
    xd = x.detach().cpu().double()
    wd, bd = w.detach().cpu().double(), bias.detach().cpu().double()[: w.shape[0]]
    K = xd.shape[1]
    KT = K // 32
    mean = xd.mean(1, keepdim=True)
    var = ((xd - mean) ** 2).mean(1, keepdim=True)
    E2 = (xd * xd).mean(1, keepdim=True)
    A1 = xd.abs().mean(1, keepdim=True)
    wv = var + eps
    rstd = 1.0 / torch.sqrt(wv)
    xhat = (xd - mean) * rstd
    pre = xhat @ wd.t() + bd
    q = _quantum(xd)
    d1 = sum_roundings(xd.abs().max(1).values, q, KT)[:, None]
    d2 = sum_roundings((xd * xd).max(1).values, q * q, KT)[:, None]
    dm = d1 * U32 * A1 / (1 - d1 * U32)
    dE = d2 * U32 * E2 / (1 - d2 * U32)
    D0 = dE + 2 * mean.abs() * dm + dm * dm
    Dv = (D0 + U32 * ((mean.abs() + dm) ** 2 + E2 + dE + wv + D0)) * (1 + 2.0 ** -20)
    hi = (1 + 2 * U32) / torch.sqrt(torch.clamp(wv - Dv, min=eps * (1 - U32)))
    lo = (1 - 2 * U32) / torch.sqrt(wv + Dv)
    drstd = torch.maximum(hi - rstd, rstd - lo)
    dv = (xd - mean).abs() * drstd + hi * dm + 2 * U32 * hi * (xd.abs() + mean.abs() + dm)
    h = bf16_half_ulp(xhat.abs() + dv)
    S = (xhat.abs() + dv + h) @ wd.abs().t() + bd.abs()
    err = (dv + h) @ wd.abs().t() + (K + 2) * U32 * S
    return dict(pre=pre, err=err, xhat=xhat, dv=dv, rho=drstd / rstd, rstd=rstd)


def rows_of(kind, m, D, seed):
    """bf16 [m, D] rows of one kind.  'pattern': tail_restated._ln's rows, one pattern of integers -100 .. 155 over 16 times
    2^(r mod 5) - every partial sum of x and x^2 exact.  The other four: block_restated.ln_rows."""
    if kind == "pattern":
        rng = np.random.RandomState(seed)
        x0 = torch.from_numpy(rng.randint(-100, 156, size=D).astype(np.float64)) / 16.0
        x = x0[None, :] * torch.from_numpy(np.exp2(np.arange(m) % 5))[:, None]
        xb = x.float().to(torch.bfloat16)
        assert torch.equal(xb.double(), x)
        return xb
    return br.ln_rows(kind, m, D, seed)


@functools.lru_cache(maxsize=None)
def probe(kind, D, action_dim, m=256):
    """A float64-bounded probe: rows of `kind`, W = bf16(randn / sqrt(D)) over all n_out columns, bias 0.2 randn.  Cached, never changed.
      pattern      exact sums: the bound is the bf16 re-rounding and the product's alone
      random       arbitrary rows, mean 0.3, sigma 1.7: the full summation depth
      onehot       one element of 5 +- 4: exact sums; xhat is sqrt(D) in one place
      constant     var = 0: eps alone sets the scale and rstd' may lie anywhere in [1 / sqrt(D + eps), 1 / sqrt(eps)]; x = mean
                   exactly (the row sum of a constant is exact), so v' is a rounding residual of c rstd' and the bias is all that is
                   left of the logits
      mean100_ulp  100 + k / 2, k in {-1, 0, 1}: var = 1 / 6 under mean^2 = 10^4.  The sums are exact (one rounding in s2 at
                   D = 512) and the one-pass formula loses what u mean^2 and u E2 are against var: rho = 4.1e-3 at D = 256, 6.1e-3 at
                   D = 512 - the widest bound here, and still three hundred times under what half the statistics do"""
    assert kind in KINDS and D in WIDTHS
    n_out = heads_n_out(action_dim)
    seed = KINDS.index(kind) * 100003 + D * 101 + action_dim
    x = rows_of(kind, m, D, seed)
    g = torch.Generator().manual_seed(seed + 1)
    w = bf16(torch.randn(n_out, D, generator=g) / D ** 0.5)
    bias = (torch.randn(n_out, generator=g) * 0.2).contiguous()
    p = ln_heads_f64(x, w, bias)
    p.update(x=x, w=w, wp=pack(w), bias=bias, exact=False)
    return p


def expected(p, action_dim, rows=None):
    """-> logits_ref, logits_bound (2^-24 |ref| + err: the float32 store), values_arg, values_ref, values_bound (err + TANHF_MARGIN:
    |tanh'| <= 1 carries err through, the margin is tanhf's own) and, for the exact probe, logits (the bits) for the first `rows` rows."""
    rows = p["pre"].shape[0] if rows is None else rows
    pre, err = p["pre"][:rows], p["err"][:rows]
    e = dict(logits_ref=pre[:, :action_dim], logits_bound=U32 * pre[:, :action_dim].abs() + err[:, :action_dim],
             values_arg=pre[:, action_dim], values_ref=torch.tanh(pre[:, action_dim]), values_bound=err[:, action_dim] + TANHF_MARGIN)
    if p["exact"]:
        e["logits"] = pre[:, :action_dim].float().contiguous()
        e["logits_bound"] = torch.zeros_like(e["logits_ref"])
    return e


def agrees(logits, values, e, live):
    """(logits, values) of a kernel or an emulation against `expected` on the first `live` rows -> (ok, largest error / bound): bits
    for the exact probe's logits, the bound otherwise; exact zeros where the value's argument is 0; SENTINEL in every other row."""
    lg, v = logits.detach().cpu(), values.detach().cpu()
    ok = bool((lg[live:] == SENTINEL).all()) and bool((v[live:] == SENTINEL).all())
    worst = 0.0
    if "logits" in e:
        ok = ok and torch.equal(lg[:live], e["logits"][:live])
        zero = e["values_arg"][:live] == 0
        ok = ok and bool((v[:live][zero] == 0).all())
    else:
        worst = worst_ratio((lg[:live].double() - e["logits_ref"][:live]).abs(), e["logits_bound"][:live])
    worst = max(worst, worst_ratio((v[:live].double() - e["values_ref"][:live]).abs(), e["values_bound"][:live]))
    return ok and worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------------------
# k_heads_finalize
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def finalize_probe(n, action_dim, ld):
    """-> heads bf16 [n, ld], logits float32 [n, action_dim] (the bf16 values widened: bit for bit), values_arg, values_ref (float64).
    Logit columns: arbitrary finite bf16 patterns, none equal to SENTINEL or POISON; the value column: multiples of 2^-6 in (-4, 4)
    (8 significant bits at most), 0 in every fourth row; columns action_dim + 1 .. ld - 1: POISON, which must appear nowhere in the
    outputs.  The value is held to TANHF_MARGIN of float64 tanh."""
    assert ld >= action_dim + 1
    rng = np.random.RandomState(n * 7 + action_dim * 3 + ld)
    pats = br.distinct_bf16(30000, rng)
    vals = torch.from_numpy(pats.view(np.int16).copy()).view(torch.bfloat16).float()
    pats = pats[((vals != SENTINEL) & (vals != POISON)).numpy()]
    heads = torch.full((n, ld), POISON, dtype=torch.bfloat16)
    body = pats[rng.randint(0, pats.size, size=(n, action_dim))]
    heads[:, :action_dim] = torch.from_numpy(body.view(np.int16).copy()).view(torch.bfloat16)
    k = rng.randint(-255, 256, size=n)
    k[0::4] = 0
    arg = torch.from_numpy(k / 64.0)
    heads[:, action_dim] = arg.float().to(torch.bfloat16)
    assert torch.equal(heads[:, action_dim].double(), arg)
    return dict(heads=heads, logits=heads[:, :action_dim].float().contiguous(), values_arg=arg, values_ref=torch.tanh(arg))


def finalize_emulate(heads, action_dim, count=None):
    """k_heads_finalize on the CPU: the widening is exact, the value is float64 tanh rounded once."""
    n = heads.shape[0]
    live = n if count is None else max(0, min(n, int(count)))
    logits = torch.full((n, action_dim), SENTINEL)
    values = torch.full((n,), SENTINEL)
    logits[:live] = heads[:live, :action_dim].float()
    values[:live] = torch.tanh(heads[:live, action_dim].double()).float()
    return logits, values
