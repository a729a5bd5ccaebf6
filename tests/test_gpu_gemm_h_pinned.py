"""Every link of the fp32-accurate tail on its own, through azk.nnx_gemm_h: all twelve instantiations azk_nnx_gemm_h dispatches
(k_gemm_h, csrc/azk_nnx.hip) and both rows of azk_nnx_gemm_h_lds (k_gemm_h_lds, csrc/azk_tail.hip), never chained, every input built
here.  Pinned two ways.  Exact probes, whose planes are exact and whose hi hi + hi lo + lo hi arithmetic is exact in float32 in any order,
so out_f32, both output planes and stats_out are known bit for bit: a one-hot selection of a 22-bit weight column (and its mirror image
for the float32-A split), a terms probe with both planes live on both sides, a count of 255 ones, an integer matmul with its row
statistics, a LayerNorm with exact statistics, a value column whose tanh argument is exactly 0 in every fourth row, the overflow flag at
its threshold.  Float64 references with bounds derived from the number formats: dense and sparse random 22-bit rows, rows with exact
LayerNorm partial sums.  tests/gemm_h_restated.py holds the probes and states each derivation; tests/test_gemm_h_restated.py shows on
the CPU that every probe notices the mistakes it is there for.  DESIGN.md, "What pins the fp16-plane tail links", lists which of these
tests turn red under nine deliberate mistakes in the kernels.

Rows: M in 1 .. 65 with no count (both sides of the 16-row fragment, of the split-K instantiations' 32-row tile and of the 2 x 2 wave
block's 32 / 64 rows), and a 2048-row buffer under device-side live counts 1, 33, 1024, 1025, 2048 (both sides of both LDS tilings'
switch; the register form runs the same counts).  The launches of a sweep take turns at planes only / out_f32 only / both, with and
without stats_out.

Each float64 test prints `RATIO <name> <largest error / bound>` before it asserts."""
import functools

import pytest
import torch

import gemm_h_restated as gh

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65)
LIVE = (1, 33, 1024, 1025, 2048)
MBUF = 2048
PAD = 4                                                       # rows behind every output buffer that must keep the sentinel
S = gh.SENTINEL
MODES = ("planes", "f32", "both")
SWEEP = [(m, None) for m in MS] + [(MBUF, c) for c in LIVE]


@functools.lru_cache(maxsize=None)
def on_card(kind, link, n_out, action_dim=None):
    """(probe, its tensors on the card, expected for all MBUF rows): built once, shared, never changed."""
    L = gh.LINKS[link]
    _held.add((kind, link, n_out, action_dim))
    p = gh.probe(kind, link, n_out, MBUF, action_dim)
    if p["exact"]:                                            # the conditions the bits rest on, on the rows that run here
        x = gh.exactness(p, L, n_out, 16)
        assert x["partial"] < 2 ** 24 and (not x["literal"] or gh.partial_all_rows(p, L, n_out) < 2 ** 24), (kind, link, n_out, x)
    d = {key: p[key].cuda() for key in ("wp", "csum", "bias", "resid", "a_stats") if p.get(key) is not None}
    d["a"] = p["a"].cuda() if L["af32"] else (p["a"][0].cuda(), p["a"][1].cuda())
    return p, d, gh.expected(p, L, action_dim=action_dim if L["epi"] == "heads" else None)


def release_probes():
    _held.clear()
    on_card.cache_clear()
    gh.probe.cache_clear()
    gh.tr.probe.cache_clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def release_wide_probes():
    """A probe at N >= 1024 keeps several float64 [2048, N] tensors: dropped after the test that used it."""
    yield
    if any(key[2] >= 1024 for key in _held):
        release_probes()


@pytest.fixture(autouse=True, scope="module")
def release_shared_probes():
    """The narrower probes are shared by the tests of this file and dropped with the last of them."""
    yield
    release_probes()


_held = set()


def sentinel_kept(t):
    return bool((t.float() == S).all())


def launch(link, n_out, d, rows, live=None, action_dim=None, mode="both", want_stats=False, ld=False, eps=gh.LN_EPS, overflow=None):
    """One link on the first `rows` rows of the probe -> the buffers it may write, each PAD rows (and, with ld, 128 columns) larger
    than what it should write, pre-filled with the sentinel."""
    import azk
    L = gh.LINKS[link]
    N = L["nbatch"] * n_out
    cut = lambda t: gh.br.strided(t[:rows], t.shape[1] + 64, -3.0)[0] if ld else t[:rows]      # lda = width + 64: 16-byte aligned rows
    a = cut(d["a"]) if L["af32"] else (cut(d["a"][0]), cut(d["a"][1]))
    kw = dict(nbatch=L["nbatch"], a_batch_stride=L["k"] if L["nbatch"] > 1 else 0, bias=d.get("bias"), lds=L["lds"], eps=eps,
              count=None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda"), overflow=overflow)
    if L["ln"]:
        kw.update(a_stats=d["a_stats"][:rows], col_sums=d["csum"])
    res = {}
    if L["epi"] == "heads":
        res["logits"] = torch.full((rows + PAD, action_dim), S, device="cuda")
        res["values"] = torch.full((rows + PAD,), S, device="cuda")
        kw.update(logits=res["logits"][:rows], values=res["values"][:rows], action_dim=action_dim)
    else:
        shape = (rows + PAD, N + (128 if ld else 0))          # ldo = N + 128, shared by the planes and out_f32
        if mode in ("planes", "both"):
            res["hi"], res["lo"] = (torch.full(shape, S, dtype=torch.float16, device="cuda") for _ in range(2))
            kw["out"] = (res["hi"][:rows, :N], res["lo"][:rows, :N])
        if mode in ("f32", "both"):
            res["f32"] = torch.full(shape, S, device="cuda")
            kw["out_f32"] = res["f32"][:rows, :N]
        if L["epi"] == "resid":
            kw["resid"] = gh.br.strided(d["resid"][:rows], 5 * N, -3.0)[0] if ld else d["resid"][:rows]
        if want_stats and not (L["lds"] and L["ln"]):         # (the LDS link 3 takes no stats_out)
            res["stats"] = torch.full((rows + PAD, N // 64, 2), S, device="cuda")
            kw["stats_out"] = res["stats"][:rows]
    azk.nnx_gemm_h(a, d["wp"], n_out, L["k"], gh.EPI[L["epi"]], **kw)
    torch.cuda.synchronize()
    return res


def check(res, e, L, n_out, live, tag):
    """The first `live` rows against `expected` (bits where the probe gives bits, else the bound); every other row, and every column
    past the link's own, keeps the sentinel.  -> largest error / bound (0 for a bit-for-bit case)."""
    N = L["nbatch"] * n_out
    got = {}
    for key, t in res.items():
        t = t.cpu()
        assert sentinel_kept(t[live:]), (tag, key)
        if key in ("hi", "lo", "f32"):
            assert sentinel_kept(t[:, N:]), (tag, key)
            t = t[:, :N]
        got[key] = t[:live].contiguous()
    want = {key: (v[:live] if torch.is_tensor(v) else v) for key, v in e.items()}
    worst = gh.verdict(got, want, L)
    assert worst != float("inf"), (tag, "bits differ")
    return worst


def sweep(link, n_out, kind, action_dim=None, cases=SWEEP, ld=False):
    """The probe at every M of MS with no count and on the MBUF-row buffer under every live count of LIVE."""
    L = gh.LINKS[link]
    p, d, e = on_card(kind, link, n_out, action_dim)
    ad = action_dim if L["epi"] == "heads" else None
    worst = 0.0
    for i, (rows, live) in enumerate(cases):
        mode, stats = ("both", True) if ld else (MODES[i % 3], i % 2 == 0)
        res = launch(link, n_out, d, rows, live, ad, mode, stats, ld, eps=p["eps"])
        worst = max(worst, check(res, e, L, n_out, rows if live is None else live, (kind, rows, live, mode)))
    return worst


def exact_kinds(L):
    return ("select", "terms", "count") + (("ln_exact",) if L["ln"] else ("int",)) + (("mirror",) if L["af32"] else ())


@pytest.mark.parametrize("link,n_out", gh.CASES)
def test_exact_probes_bit_for_bit(link, n_out):
    """Selection: row r of A is one-hot (1 or 2) at slot 37 r (+ 101 per batch) mod K, W random with full 22-bit scaled significands,
    another block per batch; the output row is that reconstructed column of W.  Its mirror on the float32-A links: W in +-1, 2, the
    one-hot value 22 bits wide - the on-the-fly split.  Terms: scaled operands 2048 m + l on both sides, expected the integer
    hi hi + hi lo + lo hi over 4096 (not the product: lo lo is dropped by design) - any term on the wrong plane gives other bits.
    Count: A all ones, 255 ones per column of W with some in every 32-wide k-step: 255 everywhere.  Integer matmul with integer bias
    (b N + col on the batched links) and residual, stats_out bit for bit.  LayerNorm links: exact statistics (mean +-2^(r mod 3),
    variance 4^(r mod 4), eps 0, eight unequal groups), the other probes under identity statistics.  out_f32 and both planes bit for bit;
    rows at or beyond the live count keep the sentinel.  Through GELU the same exact pre-activations are held to float64 GELU within
    the erf budget of gemm_h_restated.gelu_bound; through HEADS the logits are bit for bit and the (blanked) value column gives exactly 0."""
    L = gh.LINKS[link]
    ad = 225 if L["epi"] == "heads" else None
    worst = 0.0
    for kind in exact_kinds(L):
        w = sweep(link, n_out, kind, ad)
        # every bit as expected (check() has asserted it); a ratio is left by GELU, by the integer probe's value column (tanhf) and by
        # the statistics of the selection and the terms, whose sums of squares are no float32 numbers
        assert w == 0.0 or L["epi"] in ("gelu", "heads") or kind in ("select", "terms", "mirror"), (kind, w)
        worst = max(worst, w)
    print(f"RATIO exact_{link}_N{n_out} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("link,n_out", gh.CASES)
def test_within_the_float64_bound(link, n_out):
    """Against the float64 product of the operands the kernel was given (the reconstructed planes, or the float32 A itself).  Dense
    random rows: 2^-22 sum |a| |w| for the dropped term, (3 K + chains) 2^-24 for the accumulation, the epilogue's roundings, the
    output split - a worst-case bound that a float32 dot product of this length stays far below (the ratio is small by nature; what
    pins the arithmetic is the exact probes and the sparse rows).  Sparse rows: 8 non-zeros per row over all chains, the bound counts
    3 x 8 + chains additions - a missing cross term (2^-11 of a product) breaks it by orders of magnitude.  LayerNorm links: rows that
    are one pattern times 2^(r mod 5) with their exact partial sums; gemm_h_restated._ln_rand counts the operations of rstd and mean.
    Largest error / bound on an MI355X: see DESIGN.md, "What pins the fp16-plane tail links"."""
    L = gh.LINKS[link]
    ad = 225 if L["epi"] == "heads" else None
    for kind in (("ln_rand",) if L["ln"] else ("dense", "sparse")):
        worst = sweep(link, n_out, kind, ad)
        print(f"RATIO {kind}_{link}_N{n_out} {worst:.4f}")
        assert worst <= 1.0, (kind, worst)


@pytest.mark.parametrize("action_dim", gh.ACTION_DIMS)
def test_heads_value_column(action_dim):
    """The heads at action_dim in every lane residue, on both sides of a 64-column group and with action_dim + 1 == n_out, on
    tail_restated's value-column probe itself: the logits [m, action_dim] are the integers bit for bit, the value is exactly 0 where its
    argument is and within TANHF_MARGIN of float64 tanh elsewhere (the same tanhf on the same arguments as the recorded measurement;
    printed again as TANHF, in units of 2^-24); logits and values beyond the live rows keep the sentinel.  The LayerNorm heads run at
    the same action_dim on the exact statistics (bit for bit) and on real ones (float64 bound)."""
    L = gh.LINKS["k512_heads"]
    n_out = gh.heads_n_out(action_dim)
    p, d, e = on_card("value", "k512_heads", n_out, action_dim)
    worst, terr = 0.0, 0.0
    for rows, live in SWEEP:
        res = launch("k512_heads", n_out, d, rows, live, action_dim)
        n = rows if live is None else live
        worst = max(worst, check(res, e, L, n_out, n, (rows, live)))
        v = res["values"][:n].cpu()
        assert bool((v[0::4] == 0).all()), (rows, live)
        terr = max(terr, float((v.double() - e["values_ref"][:n]).abs().max()))
    print(f"TANHF ad{action_dim} {terr / gh.U32:.3f}")
    print(f"RATIO heads_value_ad{action_dim} {worst:.4f}")
    assert worst <= 1.0, worst
    assert sweep("k512_ln_heads", n_out, "ln_exact", action_dim) == 0.0
    worst = sweep("k512_ln_heads", n_out, "ln_rand", action_dim)
    print(f"RATIO ln_rand_k512_ln_heads_ad{action_dim} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("link", list(gh.LINKS))
def test_leading_dimensions(link):
    """Every link once with lda = its A width + 64, ldo = N + 128 (shared by the planes and out_f32) and (RESID) ldr = 5 N, as strided
    views: the integer probe (LayerNorm links: the exact-statistics probe) and the selection stay bit for bit with their statistics, and
    every output column past nbatch N keeps the sentinel.  A residual row found with ldo lands elsewhere in the residual's buffer."""
    L = gh.LINKS[link]
    n_out = L["n_outs"][1] if len(L["n_outs"]) > 1 else L["n_outs"][0]
    ad = 225 if L["epi"] == "heads" else None
    worst = 0.0
    for kind in ("ln_exact" if L["ln"] else "int", "select"):
        worst = max(worst, sweep(link, n_out, kind, ad, cases=((33, None), (65, None), (MBUF, 1025)), ld=True))
    print(f"RATIO ld_{link}_N{n_out} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("link", ("k512_plain", "k512_resid", "k512_f32", "k2048_plain", "lds_k2048_resid"))
def test_overflow_flag_at_its_threshold(link):
    """The sticky flag (atomic OR of 1) where a scaled plane value reaches fp16's 65504, clear at 65472, the fp16 number below: the
    output planes of PLAIN and RESID (register and LDS form), and the on-the-fly split of a float32 A (out_f32 only, so that only the
    input's split can raise it).  Other bits of the flag word survive; the values themselves are exact either way."""
    import azk
    L = gh.LINKS[link]
    for at, sign in ((gh.F16_BELOW_MAX, 1.0), (gh.F16_MAX, 1.0), (gh.F16_MAX, -1.0)):
        o = gh.overflow_probe(link, at, sign)
        m, n_out = o["want"].shape
        flag = torch.tensor([2], dtype=torch.int32, device="cuda")
        a = o["a"].cuda() if L["af32"] else (o["a"][0].cuda(), o["a"][1].cuda())
        kw = dict(bias=None if o["bias"] is None else o["bias"].cuda(), lds=L["lds"], overflow=flag)
        if o["resid"] is not None:
            kw["resid"] = o["resid"].cuda()
        f32 = torch.full((m + PAD, n_out), S, device="cuda")
        kw["out_f32"] = f32[:m]
        if not L["af32"]:
            hi, lo = (torch.full((m + PAD, n_out), S, dtype=torch.float16, device="cuda") for _ in range(2))
            kw["out"] = (hi[:m], lo[:m])
        azk.nnx_gemm_h(a, o["wp"].cuda(), n_out, L["k"], gh.EPI[L["epi"]], **kw)
        torch.cuda.synchronize()
        assert int(flag.item()) == (3 if o["expect_flag"] else 2), (at, sign, int(flag.item()))
        assert torch.equal(f32[:m].cpu().double(), o["want"]) and sentinel_kept(f32[m:]), (at, sign)
        if not L["af32"]:
            assert torch.equal(hi[:m].cpu().double(), o["want"] * gh.A_SCALE) and bool((lo[:m] == 0).all()) and sentinel_kept(hi[m:]), (at, sign)
