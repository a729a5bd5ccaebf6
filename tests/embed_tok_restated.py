"""The two kernels that open the "two-kernel" depth-1 path, k_embed (token embedding, LayerNorm1, optional score columns) and
k_cls_pool (softmax over tokens, weighted token sum), both in csrc/azk_embed_tok.hip, restated on the CPU.  Test infrastructure: no
GPU, no libazk.  The layout follows block_restated.py:
  * probe builders: inputs whose float32 arithmetic is exact in any summation order, so the kernel's output is known bit for bit,
  * float64 references with the error bound a correct kernel must meet, each derived from the kernel's source and the number formats,
  * a float32 emulation of the kernel's data movement as its source states it (`embed_emulate`, `pool_emulate`), which takes the name
    of one deliberate mistake (`mutate=`), so a probe can be shown to notice that mistake without a GPU.

Unit roundoffs: bf16 u16 = 2^-8, float32 u32 = 2^-24 (block_restated's conventions)."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from block_restated import U16, U32, bf16, bits, distinct_bf16, ln_f64  # noqa: F401  (re-exported for the tests)

# (C, R, Cc, k): each the smallest geometry that reaches its case
GEOMS = (
    (2, 15, 15, 5),   # baseline
    (3, 6, 7, 5),     # 75 patch bits: the phi branch (a row straddles patch bit 64), KS = 3
    (3, 3, 3, 3),     # KS = 1
    (1, 8, 8, 7),     # k = 7, KS = 2
    (2, 1, 1, 3),     # T = 2
    (2, 1, 30, 5),    # one row
    (2, 30, 1, 5),    # one column
    (2, 8, 10, 3),    # 6 tiles: the first shape with 3 tile groups
    (2, 10, 10, 5),   # 7 tiles, split 3 + 3 + 1
    (2, 16, 16, 5),   # T = 257
    (2, 20, 20, 5),   # 800 board bits, T = 401
    (2, 17, 18, 3),   # non-square, just past 15 x 15
    (2, 13, 30, 5),   # non-square, at the 30-column limit
    (2, 31, 32, 3),   # 1 984 bits: the entry point's limit, lanes 1..62 all used
)
WIDE_GEOMS = ((2, 15, 15, 5), (3, 6, 7, 5), (2, 20, 20, 5))      # also run at D = 256 and 512
EPS = 1e-5


def kp_of(C, k):
    return (C * k * k + 31) // 32 * 32


def tokens_of(R, Cc):
    return R * Cc + 1


def probe_boards(C, R, Cc, seed):
    """float32 [7, C, R, Cc] of 0 / 1, every board another stone pattern: empty, full, one colour (channel 0 alone), stones in the four
    corners of channel 0 and on the last cell of the last channel (the last bit of the board's bit string), three random boards of
    different densities."""
    rng = np.random.RandomState(seed)
    b = np.zeros((7, C, R, Cc), np.float32)
    b[1] = 1
    b[2, 0] = rng.rand(R, Cc) < 0.5
    b[2, 0, R - 1, Cc - 1] = 1
    for r in (0, R - 1):
        for c in (0, Cc - 1):
            b[3, 0, r, c] = 1
    b[3, C - 1, R - 1, Cc - 1] = 1
    for i, dens in enumerate((0.15, 0.5, 0.85)):
        b[4 + i] = rng.rand(C, R, Cc) < dens
    return torch.from_numpy(b)


def unfold(boards, k):
    """[n, C, R, Cc] -> the patches [n, R Cc, C k^2] of the stride-1 'same' convolution, k index = ch k^2 + ky k + kx."""
    return F.unfold(boards.float(), kernel_size=k, padding=k // 2).transpose(1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_embed: exact probes
# ---------------------------------------------------------------------------------------------------------------------------------
def identity_probe(C, R, Cc, k, D):
    """-> (wt bf16 [D, KP], cpos f32 [T, D]): wt[p][p] = 1 for p < C k^2, cpos = 0, so x[b, 1 + j, p] is bit p of token j's patch."""
    wt = torch.zeros(D, kp_of(C, k))
    p = torch.arange(C * k * k)
    wt[p, p] = 1
    return wt.to(torch.bfloat16), torch.zeros(tokens_of(R, Cc), D)


def identity_expected(boards, k, D):
    n, C, R, Cc = boards.shape
    want = torch.zeros(n, R * Cc + 1, D)
    want[:, 1:, :C * k * k] = unfold(boards, k)
    return want.to(torch.bfloat16)


def int_probe(C, R, Cc, k, D, H, seed):
    """Integer GEMM over every column.  wt in {-1, 0, 1} on every one of the D rows, cpos integers in [-100, 100] on every row (row 0 is
    the cls row): every token entry is an integer of magnitude <= C k^2 + 100 <= 175, exact in float32 and in bf16.
    Score columns: m' [H, D] in {-1, 0, 1} on 32 columns per head, so wt_ext[D + h] = m'_h W (|.| <= 32), mtab = cpos m'^T
    (|.| <= 3 200) and msum = sum m' are integers and x . m' - mean msum is exact in float32 (a multiple of 1 / D below 2^14).
    Row D + 15 and mtab[:, 15] (the row-mean column of the fused kernel's operands) hold arbitrary integers: k_embed must not use them.
    LayerNorm affine: random float32 ln_w, ln_b."""
    g = torch.Generator().manual_seed(seed)
    kreal, KP, T = C * k * k, kp_of(C, k), tokens_of(R, Cc)
    W = torch.randint(-1, 2, (D, kreal), generator=g).float()
    cpos = torch.randint(-100, 101, (T, D), generator=g).float()
    mp = torch.zeros(H, D)
    for h in range(H):
        cols = torch.randperm(D, generator=g)[:32]
        mp[h, cols] = (torch.randint(0, 2, (32,), generator=g) * 2 - 1).float()
    wt_ext = torch.zeros(D + 16, KP)
    wt_ext[:D, :kreal] = W
    wt_ext[D:D + H, :kreal] = mp @ W
    wt_ext[D + 15, :kreal] = torch.randint(-3, 4, (kreal,), generator=g).float()
    mtab = torch.zeros(T, 16)
    mtab[:, :H] = cpos @ mp.t()
    mtab[:, 15] = torch.randint(-50, 51, (T,), generator=g).float()
    msum = torch.zeros(16)
    msum[:H] = mp.sum(1)
    assert float(wt_ext.abs().max()) <= 256
    return dict(wt_ext=wt_ext.to(torch.bfloat16), cpos=cpos, mprime=mp, mtab=mtab, msum=msum, H=H, D=D, k=k,
                ln_w=torch.randn(D, generator=g) * 0.5 + 1.0, ln_b=torch.randn(D, generator=g) * 0.2)


def embed_x_f64(boards, wt, cpos, k):
    """tokens in float64 from the operands as given: [n, T, D] = [0 ; unfold] wt[:, :C k^2]^T + cpos."""
    n, C = boards.shape[0], boards.shape[1]
    kreal = C * k * k
    p = unfold(boards, k).double()
    x = torch.cat([torch.zeros(n, 1, wt.shape[0], dtype=torch.float64), p @ wt[:, :kreal].double().t()], 1)
    return x + cpos.double()


def int_expected_x(boards, pr):
    """The integer probe's tokens, exact: float32 integers [n, T, D]."""
    x = embed_x_f64(boards, pr["wt_ext"][:pr["D"]].float(), pr["cpos"], pr["k"])
    assert float(x.abs().max()) <= 175 and bool((x == x.round()).all())
    return x.float()


# ---------------------------------------------------------------------------------------------------------------------------------
# k_embed: LayerNorm and score columns against float64
# ---------------------------------------------------------------------------------------------------------------------------------
def sum_depth(D):
    """Additions on the longest path of k_embed's row sums: a lane adds its 8 D / 128 accumulators one after the other
    (8 D / 128 - 1 additions), then row16_sum's 4 butterfly steps.  11 at D = 128, 19 at 256, 35 at 512."""
    return 8 * (D // 128) - 1 + 4


def ln_c(D):
    """Relative float32 error of k_embed's xhat w + b, in units of u32, by its source:
      x - mean  1 rounding;  squares 1 x 2 + 1 = 3;  their sum sum_depth(D);  x 1 / D exact;  + eps 1: the variance carries
      sum_depth + 4, rsqrtf half of that plus 2 (stated error 1 ulp);  x rstd, x w, + b one rounding each.
    |xhat w| carries 1 + (sum_depth + 4) / 2 + 2 + 2 and the sum with b one more: sum_depth / 2 + 8; + 2 for the second-order terms."""
    return 0.5 * sum_depth(D) + 10.0


def half_ulp_bf16(y):
    mant, expo = torch.frexp(y)                                   # |y| in [2^(e-1), 2^e): a bf16 ulp there is 2^(e-8)
    return torch.where(y == 0, torch.zeros_like(y), torch.ldexp(torch.ones_like(y), expo - 9))


def ln_bound(D, y, xw, kappa, w, b):
    """|xhat - y| <= half a bf16 ulp of y + u32 (ln_c(D) (|xhat w| + |b|) + sum_depth(D) kappa |w|): block_restated.ln_bound's form
    with k_embed's own constants.  The kappa term is the error of the mean (absolute sum_depth u32 mean|x|), which shifts every
    x - mean alike; it vanishes where the row sum is exact, as on the integer probe, and is kept because the bound does not
    assume that."""
    y = y.double()
    return half_ulp_bf16(y) + U32 * (ln_c(D) * (xw.abs() + b.double().abs()) + sum_depth(D) * kappa * w.double().abs())


def ln_rows_f64(x, w, b):
    """float64 LayerNorm of [n, T, D] tokens -> (y, xw, kappa, mean, rstd) with ln_f64's meanings, shaped like x ([n, T, 1] for the
    per-row ones)."""
    n, T, D = x.shape
    y, xw, kappa = ln_f64(x.reshape(n * T, D), w, b, EPS)
    xd = x.double()
    mean = xd.mean(2, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(2, keepdim=True) + EPS)
    return y.view(n, T, D), xw.view(n, T, D), kappa.view(n, T, 1), mean, rstd


def score_c(D):
    """rstd carries (sum_depth + 4) / 2 + 2 u32 (ln_c), the product with the exact x . m' - mean msum one more; + 1 second order."""
    return 0.5 * sum_depth(D) + 6.0


def scores_f64(x, mean, rstd, E, msum):
    """The kernel's formula in float64: s[b, h, t] = rstd (E - mean msum[h]), E[b, t, h] = x_t . m'_h as the extra MFMA columns give it."""
    return (rstd * (E - mean * msum.double()[None, None, :])).transpose(1, 2)


def int_scores_f64(boards, pr, x):
    """-> (s [n, H, T], E) of the integer probe; E = x m'^T exactly."""
    H = pr["H"]
    _, _, _, mean, rstd = ln_rows_f64(x, torch.ones(pr["D"]), torch.zeros(pr["D"]))
    E = x.double() @ pr["mprime"].double().t()
    n, C = boards.shape[0], boards.shape[1]
    kreal = C * pr["k"] ** 2
    E2 = torch.cat([torch.zeros(n, 1, H, dtype=torch.float64),
                    unfold(boards, pr["k"]).double() @ pr["wt_ext"][pr["D"]:pr["D"] + H, :kreal].double().t()], 1) + pr["mtab"][:, :H].double()
    assert torch.equal(E, E2)                                    # the folded columns state the same integers
    return scores_f64(x, mean, rstd, E, pr["msum"][:H]), E


def rand_probe(C, R, Cc, k, D, H, seed):
    """bf16-representable randn weights (conv scale 1 / sqrt(C k^2)), cpos, score rows, mtab and msum: nothing but the kernel rounds."""
    g = torch.Generator().manual_seed(seed)
    kreal, KP, T = C * k * k, kp_of(C, k), tokens_of(R, Cc)
    wt_ext = torch.zeros(D + 16, KP)
    wt_ext[:D + H, :kreal] = torch.randn(D + H, kreal, generator=g) / math.sqrt(kreal)
    mtab = torch.zeros(T, 16)
    mtab[:, :H] = torch.randn(T, H, generator=g)
    msum = torch.zeros(16)
    msum[:H] = torch.randn(H, generator=g) * 0.5
    return dict(wt_ext=wt_ext.to(torch.bfloat16), cpos=bf16(torch.randn(T, D, generator=g) * 0.5), mtab=bf16(mtab), msum=bf16(msum),
                H=H, D=D, k=k, ln_w=torch.randn(D, generator=g) * 0.5 + 1.0, ln_b=torch.randn(D, generator=g) * 0.2)


def embed_f64(boards, wt_ext, cpos, mtab, msum, k, D, H, ln_w=None, ln_b=None, extra_x=None, extra_E=None):
    """Float64 reference of everything k_embed emits, from operands given as tensors, with the bounds a correct kernel meets.
    -> dict(x, x_bound, xhat, xhat_bound [affine, when ln_w is given], xn, xn_bound [the score variant's plain normalised tokens],
            s, s_bound [n, H, T]).
    x:     2^-8 |x| + (C k^2 + 2) u32 S, S = |patch| |w| + |cpos|: the bf16 store, and C k^2 float32 accumulations onto cpos with
           exact products (a patch entry is 0 or 1).  dx = the float32 part is what LayerNorm sees; extra_x (the caller's bound on the
           operands' own distance from the reference's, [n, T, D]) is added to it.
    xhat:  ln_bound on top of the propagated dx.  With dmax = max_d dx over the row: the mean moves by <= dmax, x - mean by <= 2 dmax;
           d var = (2 / D) sum (x - mean) dx (the mean's shift cancels, sum (x - mean) = 0), so rstd moves by at most
           rstd^2 mean|x - mean| dmax <= rstd dmax, relative.  |d xn| <= rstd dmax (2 + |xn|), times |w| with the affine.
    s:     rstd (E - mean msum).  E carries dE = (C k^2 + 2) u32 (|patch| |w_ext| + |mtab|) + extra_E; the mean dmax plus its own
           float32 sum, sum_depth u32 mean|x|; product and difference 2 u32 (|E| + |mean msum|); rstd relative rstd dmax + score_c u32."""
    n, C = boards.shape[0], boards.shape[1]
    kreal = C * k * k
    p = unfold(boards, k).double()
    pz = torch.cat([torch.zeros(n, 1, kreal, dtype=torch.float64), p], 1)                       # the cls row has no patch
    W = wt_ext[:D, :kreal].double()
    x = pz @ W.t() + cpos.double()
    dx = (kreal + 2) * U32 * (pz @ W.abs().t() + cpos.double().abs())
    out = dict(x=x, x_bound=U16 * x.abs() + dx)
    if extra_x is not None:
        dx = dx + extra_x
    dmax = dx.max(2, keepdim=True).values
    one, zero = torch.ones(D), torch.zeros(D)
    xn, _, kappa, mean, rstd = ln_rows_f64(x, one, zero)
    prop = rstd * dmax * (2.0 + xn.abs())
    out.update(xn=xn, xn_bound=ln_bound(D, xn, xn, kappa, one, zero) + prop)
    if ln_w is not None:
        y, xw, kappa, _, _ = ln_rows_f64(x, ln_w, ln_b)
        out.update(xhat=y, xhat_bound=ln_bound(D, y, xw, kappa, ln_w, ln_b) + prop * ln_w.double().abs())
    We = wt_ext[D:D + H, :kreal].double()
    E = pz @ We.t() + mtab[:, :H].double()
    dE = (kreal + 2) * U32 * (pz @ We.abs().t() + mtab[:, :H].double().abs())
    if extra_E is not None:
        dE = dE + extra_E
    ms = msum[:H].double()[None, None, :]
    s = rstd * (E - mean * ms)
    ds = s.abs() * (rstd * dmax + score_c(D) * U32) + rstd * (
        dE + ms.abs() * (dmax + sum_depth(D) * U32 * x.abs().mean(2, keepdim=True)) + 2 * U32 * (E.abs() + (mean * ms).abs()))
    out.update(s=s.transpose(1, 2), s_bound=ds.transpose(1, 2))
    return out


def ln_case_probe(R, Cc, D):
    """Zero weights, so x = cpos exactly, with rows of three kinds by t mod 3: a constant row (variance 0: xhat = bf16(ln_b) exactly
    with the affine, 0 without; every score 0), a mean-100 row 100 + {-1, 0, 1}, and a row of random integers."""
    g = torch.Generator().manual_seed(R * Cc + D)
    T = tokens_of(R, Cc)
    cpos = torch.randint(-100, 101, (T, D), generator=g).float()
    cpos[0::3] = torch.randint(-100, 101, (len(range(0, T, 3)), 1), generator=g).float().expand(-1, D)
    cpos[1::3] = 100.0 + torch.randint(-1, 2, (len(range(1, T, 3)), D), generator=g).float()
    return cpos


# ---------------------------------------------------------------------------------------------------------------------------------
# k_embed: the emulation
# ---------------------------------------------------------------------------------------------------------------------------------
EMBED_MISTAKES = ("word_off_by_one", "phi_carry_dropped", "dead_row_kept", "stride_RR", "cols_swapped")


def column_map(D, mutate=None):
    """load[c] = the weight row whose products land in output column c.  Accumulator a = 8 g + q of lane l15 is fed from weight row
    128 (a >> 3) + 8 l15 + (a & 7) and stored to column 128 g + 8 l15 + q: the identity when both sides agree.
    'cols_swapped': the staging takes rows D - 3 and D - 12 for one another."""
    load = np.zeros(D, np.int64)
    for a in range(8 * (D // 128)):
        for l15 in range(16):
            src = 128 * (a >> 3) + 8 * l15 + (a & 7)
            if mutate == "cols_swapped":
                src = {D - 3: D - 12, D - 12: D - 3}.get(src, src)
            load[128 * (a // 8) + 8 * l15 + (a % 8)] = src
    return load


def patch_words(board, k, T, mutate=None):
    """One board [C, R, Cc] -> (plo, phi) uint64 [16 ceil(T / 16)]: each token's patch bits as k_embed assembles them.
    The board is a bit string (cell e = bit e) in 32-bit words, word i - 1 in lane i (lanes 0 and 63: zeros; a lane index wraps
    mod 64).  Per (channel, patch row): off = 32 + ch R Cc + clamp(row) Cc + (c - pad), the two words around it funnel-shifted
    right by off & 31, masked to the columns on the board, zeroed for a dead token or a row off the board, and placed at patch bit
    p0 = ch k^2 + ky k: into plo, into phi (p0 >= 64), or split over both (p0 < 64 < p0 + k).
    mutate: 'word_off_by_one'   the word index is (off + 1) >> 5: wrong only where off & 31 == 31
            'phi_carry_dropped' the bits of a straddling row that belong to phi are lost
            'dead_row_kept'     a row off the board is not zeroed (the clamped row's bits stay)
            'stride_RR'         the channel stride R Cc taken as R R"""
    C, R, Cc = board.shape
    cells = (board.reshape(-1).numpy() != 0).astype(np.uint64)
    ncell = C * R * Cc
    assert ncell <= 62 * 32
    words = np.zeros(64, np.uint64)
    for e in np.nonzero(cells)[0]:
        words[1 + (e >> 5)] |= np.uint64(1) << np.uint64(e & 31)
    RC = R * R if mutate == "stride_RR" else R * Cc
    pad, kk = k // 2, k * k
    Tp = (T + 15) // 16 * 16
    t = np.arange(Tp, dtype=np.int64)
    j = t - 1
    r = np.where(j >= 0, j // Cc, 0)                      # C division truncates: j = -1 gives r = 0, c = -1
    c = j - r * Cc
    live = (t >= 1) & (t < T)
    colmask = np.zeros(Tp, np.uint64)
    for kx in range(k):
        cc = c + kx - pad
        colmask |= np.where((cc >= 0) & (cc < Cc), np.uint64(1) << np.uint64(kx), np.uint64(0)).astype(np.uint64)
    plo = np.zeros(Tp, np.uint64)
    phi = np.zeros(Tp, np.uint64)
    M32 = np.uint64(0xffffffff)
    for ch in range(C):
        for ky in range(k):
            rr = r + ky - pad
            off = 32 + ch * RC + np.clip(rr, 0, R - 1) * Cc + (c - pad)
            wi = ((off + 1) >> 5) if mutate == "word_off_by_one" else (off >> 5)
            sh = (off & 31).astype(np.uint64)
            lo, hi = words[wi & 63], words[(wi + 1) & 63]
            b = (((lo | (hi << np.uint64(32))) >> sh) & M32) & colmask
            dead = ~live if mutate == "dead_row_kept" else (~live | (rr < 0) | (rr >= R))
            b = np.where(dead, np.uint64(0), b).astype(np.uint64)
            p0 = ch * kk + ky * k
            if p0 < 64:
                plo |= b << np.uint64(p0)
                if p0 + k > 64 and mutate != "phi_carry_dropped":
                    phi |= b >> np.uint64(64 - p0)
            else:
                phi |= b << np.uint64(p0 - 64)
    return plo, phi


def embed_emulate(boards, wt_ext, cpos, k, D, H=0, mtab=None, msum=None, ln_w=None, ln_b=None, mutate=None):
    """k_embed in float32 -> dict(x bf16 [n, T, D], xhat bf16 (affine when ln_w is given, else the plain normalised tokens),
    scores f32 [n, H, T] when H > 0).  The A operand is the byte 32 s + 8 (lane >> 4) of plo / phi expanded to 0 / 1."""
    assert mutate is None or mutate in EMBED_MISTAKES
    n, C, R, Cc = boards.shape
    T, KP = R * Cc + 1, wt_ext.shape[1]
    A = torch.zeros(n, T, KP)
    for b in range(n):
        plo, phi = patch_words(boards[b], k, T, mutate)
        for p in range(KP):
            src, sh = (plo, p) if p < 64 else (phi, p - 64)
            A[b, :, p] = torch.from_numpy(((src[:T] >> np.uint64(sh)) & np.uint64(1)).astype(np.float32))
    w = wt_ext.float()
    acc = cpos.float() + A @ w[:D][torch.from_numpy(column_map(D, mutate))].t()
    out = dict(x=acc.to(torch.bfloat16))
    mean = acc.sum(2, keepdim=True) * np.float32(1.0 / D)
    d = acc - mean
    rstd = torch.rsqrt((d * d).sum(2, keepdim=True) * np.float32(1.0 / D) + np.float32(EPS))
    xn = d * rstd
    out["xhat"] = (xn * ln_w.float() + ln_b.float() if ln_w is not None else xn).to(torch.bfloat16)
    if H:
        E = mtab[:, :H].float() + A @ w[D:D + H].t()
        out["scores"] = (rstd * (E - mean * msum[:H].float())).transpose(1, 2).contiguous()
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# k_cls_pool
# ---------------------------------------------------------------------------------------------------------------------------------
POOL_DH = ((512, 8), (256, 8), (256, 4), (128, 4), (128, 8), (512, 4))
POOL_T = (1, 2, 8, 9, 31, 32, 33, 50, 64, 65, 226, 255, 256, 257, 272, 273, 320, 401, 993)
POOL_MISTAKES = ("cut256", "pad_counted", "last_chunk_skipped")
OFF = -200.0          # a score that weighs exactly 0 beside a 0: exp(-200) underflows float32


def pool_lds_bytes(T, D, H):
    """launch_cls_pool's dynamic LDS: the weights [Tp][H] and two partial z [H][D], float32.  The entry point refuses above 64 KB."""
    return (tp_of(T) * H + 2 * H * D) * 4


def tp_of(T):
    return (T + 15) // 16 * 16


def pool_scores(n, H, T, poison):
    """[n, H, Tp] filled with OFF on the tokens; the padding [T, Tp) holds 0 (a pad that is counted weighs as much as a selected
    token) or, poisoned, NaN.  k_cls_pool does not read the padding, so both give the same bits."""
    s = torch.full((n, H, tp_of(T)), OFF)
    s[:, :, T:] = float("nan") if poison else 0.0
    return s


def pool_targets(n, H, T):
    """[n, H] target tokens, a different one per (board, head) while T allows.  Wave w streams the 8-token chunks q = t // 8 with
    q mod 4 = w, alternating between two register sets ((q // 4) mod 2).  The targets visit token 0, token T - 1, where T > 256 the
    tokens 256 and 257 (the first ones the softmax phase used to leave out), and for each of the eight (wave, register set) pairs the
    last chunk of that pair at a different place inside the chunk; the rest are spread evenly."""
    must = [0, T - 1] + ([256, min(257, T - 1)] if T > 256 else [])
    nq = (T + 7) // 8
    for pair in range(8):
        q = pair + 8 * ((nq - 1 - pair) // 8) if nq > pair else None
        if q is not None:
            must.append(min(8 * q + (3 * pair + 1) % 8, T - 1))
    rest = [int(i * (T - 1) / max(1, n * H - 1)) for i in range(n * H)]
    seen, tg = set(), []
    for t in must + rest:
        if t not in seen:
            seen.add(t)
            tg.append(t)
    tg = (tg * (n * H // len(tg) + 1))[:n * H]
    return np.asarray(tg).reshape(H, n).T.copy()                  # heads vary slowest: each board sees several kinds


def pool_select_probe(n, T, D, H, seed, poison=False):
    """-> (xhat bf16 [n, T, D] of distinct bit patterns, scores, c, expected bf16 [n, H, D]).  Score 0 at the target and OFF elsewhere,
    with a non-zero c[h]: the weights are exactly 1 and 0 and z[b][h] is the target's xhat row bit for bit."""
    rng = np.random.RandomState(seed)
    pat = rng.permutation(np.tile(distinct_bf16(30000, rng), (n * T * D + 29999) // 30000))[: n * T * D]
    xb = torch.from_numpy(pat.view(np.int16).reshape(n, T, D).copy()).view(torch.bfloat16)
    tgt = pool_targets(n, H, T)
    s = pool_scores(n, H, T, poison)
    for b in range(n):
        for h in range(H):
            s[b, h, tgt[b, h]] = 0.0
    c = torch.from_numpy(rng.standard_normal(H) * 2.0 + 0.5).float()
    want = torch.stack([torch.stack([xb[b, tgt[b, h]] for h in range(H)]) for b in range(n)])
    return xb, s, c, want


def pool_mean_sets(n, H, T):
    """Per (board, head) a set of 2^j tokens holding 0, T - 1 and, where they exist, 256 and a token beyond it; j cycles with b + h
    through 1 .. 6 (from 2 where the set has those four to hold; 0 for T = 1)."""
    jmax = min(6, int(math.floor(math.log2(T))))
    sets = {}
    for b in range(n):
        for h in range(H):
            j = 0 if jmax == 0 else (2 + (b + h) % 5 if T > 258 else 1 + (b + h) % jmax)
            size = 2 ** j
            must = [T - 1, 0] + ([256, (256 + T - 1) // 2] if T > 258 else [])
            rng = np.random.RandomState(1000 * b + h)
            S = []
            for t in must + list(rng.permutation(T)):
                if int(t) not in S and len(S) < size:
                    S.append(int(t))
            sets[b, h] = S
    return sets


def pool_mean_probe(n, T, D, H, seed, poison=False):
    """-> (xhat of integers |.| <= 127, scores, c, expected).  The 2^j tokens of the set score 0, the rest OFF: the weights are 2^-j
    and 0 exactly, every partial sum is a multiple of 2^-j below 2^7 (exact in any order), and z = bf16(mean over the set)."""
    rng = np.random.RandomState(seed)
    xi = torch.from_numpy(rng.randint(-127, 128, size=(n, T, D)).astype(np.float32))
    s = pool_scores(n, H, T, poison)
    want = torch.zeros(n, H, D)
    for (b, h), S in pool_mean_sets(n, H, T).items():
        s[b, h, S] = 0.0
        want[b, h] = xi[b, S].double().mean(0).float()
    c = torch.from_numpy(rng.standard_normal(H) * 2.0 + 0.5).float()
    return xi.to(torch.bfloat16), s, c, want.to(torch.bfloat16)


def pool_f64(xhat, scores, c, T):
    """-> (z, A, Smax): z = sum_t softmax_t(scores[..., :T] + c) xhat_t in float64, A = sum_t p_t |xhat_t|, Smax [n, H, 1] = the
    largest |score + c| of the row."""
    x = xhat.detach().cpu().double()
    e = scores[:, :, :T].double() + c.double()[None, :, None]
    p = torch.softmax(e, dim=2)
    return torch.einsum("nht,ntd->nhd", p, x), torch.einsum("nht,ntd->nhd", p, x.abs()), e.abs().max(2, keepdim=True).values


def pool_k(T, Smax):
    """The float32 allowance of k_cls_pool in units of u32 A, re-derived from block_restated.cls_bound's 2^-14 A for this kernel, which
    normalises the weights before the sum and evaluates exp as __expf (v_exp_f32 of x log2 e):
      e = s + c and e - max: one rounding each, <= 3 u32 Smax absolute on the exponent; x log2 e: another 2 u32 Smax;
      v_exp_f32: 1 ulp = 2 u32   -> an unnormalised weight carries 5 Smax + 2, relative;
      their sum: the same again from its terms, ceil(Tp / 64) - 1 additions in the lane and 6 butterfly steps;
      1 / sum: 2 (1 ulp allowed);  x inv: 1   -> a weight carries 10 Smax + ceil(Tp / 64) + 12;
      the token sum: a wave adds its 8 ceil(T / 32) products one after the other (each product 1, each addition 1), and the
      four waves are combined in 2 more additions: 8 ceil(T / 32) + 3.
    K = 10 Smax + ceil(Tp / 64) + 8 ceil(T / 32) + 15, times 1 + 2^-6 for the second-order terms."""
    return (10.0 * Smax + (tp_of(T) + 63) // 64 + 8 * ((T + 31) // 32) + 15) * (1.0 + 2.0 ** -6)


def pool_bound(z, A, T, Smax, xmax):
    """|out - z| <= 2^-8 |z| + pool_k u32 A + T 2^-126 max|x|: the bf16 store, the float32 allowance, and the weights that __expf
    flushes to 0 where float64 keeps a denormal-sized one."""
    return U16 * z.abs() + pool_k(T, Smax) * U32 * A + T * 2.0 ** -126 * xmax


def pool_emulate(xhat, scores, c, T, mutate=None):
    """k_cls_pool in float32.  Softmax: lane l of the head's wave takes tokens l + 64 k, k < ceil(Tp / 64): maximum, sum (in the lane
    in rising k, then a 6-step butterfly) and weights e inv; the weights of [T, Tp) are 0.  Token sum: wave w streams the chunks
    8 (w + 4 i) .. + 8 in rising i, rows past T - 1 clamped to T - 1; the waves combine as (0 + 2) + (1 + 3); one rounding to bf16.
    mutate: 'cut256'             the softmax phase stops after four chunks: tokens from 256 on take no part and their weights are
                                 whatever the LDS held (1.0 here)
            'pad_counted'        the tokens [T, Tp) take part in the softmax with the scores found there
            'last_chunk_skipped' the wave that owns the last 8-token chunk leaves it out"""
    assert mutate is None or mutate in POOL_MISTAKES
    x = xhat.detach().cpu().float()
    n, _, D = x.shape
    H = scores.shape[1]
    Tp = tp_of(T)
    nchunk = (Tp + 63) // 64
    lim = Tp if mutate == "pad_counted" else T
    seen = min(lim, 256) if mutate == "cut256" else lim
    e = torch.full((n, H, nchunk * 64), -3.0e38)
    e[:, :, :seen] = scores[:, :, :seen].float() + c.float()[None, :, None]
    mx = e.view(n, H, nchunk, 64).max(2).values.max(2, keepdim=True).values
    ex = torch.zeros(n, H, nchunk * 64)
    ex[:, :, :seen] = torch.exp(e[:, :, :seen] - mx)
    lane = torch.zeros(n, H, 64)
    for k in range(nchunk):
        lane = lane + ex[:, :, 64 * k:64 * k + 64]
    for off in (32, 16, 8, 4, 2, 1):
        lane = lane + lane[:, :, torch.arange(64) ^ off]
    aw = ex[:, :, :Tp] * (1.0 / lane[:, :, :1])
    aw[:, :, lim:] = 0.0
    if mutate == "cut256":
        aw[:, :, 256:] = 1.0
    zw = torch.zeros(4, n, H, D)
    last_chunk = (T - 1) // 8
    for q in range((T + 7) // 8):
        if mutate == "last_chunk_skipped" and q == last_chunk:
            continue
        for kk in range(8):
            t = 8 * q + kk
            zw[q & 3] = zw[q & 3] + aw[:, :, t, None] * x[:, None, min(t, T - 1), :]
    return ((zw[0] + zw[2]) + (zw[1] + zw[3])).to(torch.bfloat16)
