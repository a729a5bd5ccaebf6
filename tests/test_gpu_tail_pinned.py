"""Every link of the bf16 cls-row tail on its own, through azk.nn_tail_gemm: all twelve instantiations azk_nn_tail_gemm dispatches
(k_tail_gemm, csrc/azk_nn.hip) and both rows of azk_nn_tail_gemm_lds (k_tail_lds, csrc/azk_tail.hip), pinned two ways.  Exact probes,
whose float32 arithmetic is exact in any order, so the output is known bit for bit: a one-hot selection of a weight column, a count
of 255 ones, an integer matmul with its row statistics, a value column whose tanh argument is exactly 0 in every fourth row.  Float64
references with bounds derived from the number formats.  tests/tail_restated.py holds the probes and states each derivation;
tests/test_tail_restated.py shows on the CPU that every probe notices the mistakes it is there for.  DESIGN.md, "What pins the
cls-row tail links", lists which of these tests turn red under six deliberate mistakes in the kernels.

Rows: M in 1 .. 65 with no count (both sides of the 16-row fragment and of the 32- and 64-row tiles), and a 2048-row buffer under
device-side live counts 1, 33, 1024, 1025, 1536, 1537, 2048.  On a 256-CU part those sit on both sides of the LDS form's switch of
tilings at 1024 live rows and of the register form's choice between 32-, 48- and 64-row wave tiles - for the four instantiations that
have the choice, at the widths that put 32 waves on a strip: the wide GELU links at N = 2048 and the K = 2048 links at N = 512
(tail_restated.LINKS states the rule; at N = 64 / 128 the K = 2048 links stay on 32-row tiles at every count).  On a part with another
CU count the register form's thresholds move and the probes stay valid (a row's result does not depend on the tile that computes it).

Each float64 test prints `RATIO <name> <largest error / bound>` before it asserts."""
import functools

import pytest
import torch

import tail_restated as tr

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 31, 32, 33, 64, 65)
LIVE = (1, 33, 1024, 1025, 1536, 1537, 2048)
MBUF = 2048
PAD = 4                                                       # rows behind every output buffer that must keep the sentinel
S = tr.SENTINEL
CASES = [(link, n_out) for link, L in tr.LINKS.items() for n_out in L["n_outs"]]
PLAIN_CASES = [(link, n_out) for link, n_out in CASES if not tr.LINKS[link]["ln"]]


@functools.lru_cache(maxsize=None)
def on_card(kind, link, n_out, action_dim=None):
    """(probe, its tensors on the card, expected for all MBUF rows): built once, shared, never changed."""
    L = tr.LINKS[link]
    _held.add((kind, link, n_out, action_dim))
    p = tr.probe(kind, link, n_out, MBUF, action_dim)
    d = {key: p[key].cuda() for key in ("a", "wp", "bias", "resid", "a_stats", "col_sums") if p.get(key) is not None}
    return p, d, tr.expected(p, L, action_dim=action_dim if L["epi"] == "heads" else None)


def release_probes():
    _held.clear()
    on_card.cache_clear()
    tr.probe.cache_clear()
    torch.cuda.empty_cache()


@pytest.fixture(autouse=True)
def release_wide_probes():
    """A probe at N = 2048 keeps several float64 [2048, 2048] tensors: dropped after the test that used it."""
    yield
    if any(key[2] >= 2048 for key in _held):
        release_probes()


@pytest.fixture(autouse=True, scope="module")
def release_shared_probes():
    """The narrower probes are shared by the tests of this file and dropped with the last of them."""
    yield
    release_probes()


_held = set()


def sentinel_kept(t):
    return bool((t.float() == S).all())


def launch(link, n_out, d, rows, live=None, action_dim=None, want_stats=False, ld=False):
    """One link on the first `rows` rows of the probe -> the buffers it may write, each PAD rows (and, with ld, 128 columns) larger
    than what it should write, pre-filled with the sentinel."""
    import azk
    L = tr.LINKS[link]
    N = L["nbatch"] * n_out
    a = d["a"][:rows]
    if ld:                                                    # lda = width + 64, ldo = N + 128, ldr = 5 N, as strided views
        a, _ = tr.br.strided(a, a.shape[1] + 64, -3.0)
    kw = dict(nbatch=L["nbatch"], a_batch_stride=L["k"] if L["nbatch"] > 1 else 0, bias=d.get("bias"), lds=L["lds"],
              count=None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda"))
    if L["ln"]:
        kw["a_stats"] = d["a_stats"][:rows]
        if L["lds"]:
            kw["col_sums"] = d["col_sums"]
    res = {}
    if L["epi"] == "heads":
        res["logits"] = torch.full((rows + PAD, action_dim), S, device="cuda")
        res["values"] = torch.full((rows + PAD,), S, device="cuda")
        kw.update(logits=res["logits"][:rows], values=res["values"][:rows], action_dim=action_dim)
    else:
        res["out"] = torch.full((rows + PAD, N + (128 if ld else 0)), S, dtype=torch.bfloat16, device="cuda")
        kw["out"] = res["out"][:rows, :N]
        if L["epi"] == "resid":
            kw["resid"] = tr.br.strided(d["resid"][:rows], 5 * N, -3.0)[0] if ld else d["resid"][:rows]
        if want_stats:
            res["stats"] = torch.full((rows + PAD, N // 64, 2), S, device="cuda")
            kw["stats_out"] = res["stats"][:rows]
    azk.nn_tail_gemm(a, d["wp"], n_out, L["k"], tr.EPI[L["epi"]], **kw)
    torch.cuda.synchronize()
    return res


def check(res, e, L, n_out, live, tag, action_dim=None):
    """The first `live` rows against `expected` (bits where the probe gives bits, else the bound); every other row, and every column
    past the link's own, keeps the sentinel.  -> largest error / bound (0 for a bit-for-bit case)."""
    worst = 0.0
    if L["epi"] == "heads":
        lg, v = res["logits"].cpu(), res["values"].cpu()
        assert sentinel_kept(lg[live:]) and sentinel_kept(v[live:]), tag
        if "logits" in e:
            assert torch.equal(lg[:live], e["logits"][:live]), tag
        else:
            worst = tr.worst_ratio((lg[:live].double() - e["logits_ref"][:live]).abs(), e["logits_bound"][:live])
        worst = max(worst, tr.worst_ratio((v[:live].double() - e["values_ref"][:live]).abs(), e["values_bound"][:live]))
        return worst
    N = L["nbatch"] * n_out
    out = res["out"].cpu()
    assert sentinel_kept(out[live:]) and sentinel_kept(out[:, N:]), tag
    got = out[:live, :N].contiguous()
    if "out" in e:
        want = e["out"][:live]
        assert torch.equal(tr.bits(got), tr.bits(want)), (tag, f"{int((tr.bits(got) != tr.bits(want)).sum())} elements differ")
    else:
        worst = tr.worst_ratio((got.double() - e["ref"][:live]).abs(), e["bound"][:live])
    if "stats" in res:
        st = res["stats"].cpu()
        assert sentinel_kept(st[live:]), tag
        assert torch.equal(st[:live], e["stats"][:live]), tag
    return worst


def sweep(link, n_out, kind, action_dim=None, want_stats=False):
    """The probe at every M of MS with no count and on the MBUF-row buffer under every live count of LIVE."""
    L = tr.LINKS[link]
    p, d, e = on_card(kind, link, n_out, action_dim)
    ad = action_dim if L["epi"] == "heads" else None
    worst = 0.0
    for rows, live in [(m, None) for m in MS] + [(MBUF, c) for c in LIVE]:
        res = launch(link, n_out, d, rows, live, ad, want_stats)
        worst = max(worst, check(res, e, L, n_out, rows if live is None else live, (kind, rows, live), ad))
    return worst


@pytest.mark.parametrize("link,n_out", PLAIN_CASES)
def test_exact_probes_bit_for_bit(link, n_out):
    """Selection: row r of A is one-hot (1 or 2) at slot 37 r (+ 101 per batch) mod K, W random bf16 with full significands, another
    block per batch; the output row is that column of W, doubled where A held 2.  A wrong k slot, a wrong wave's K range, a wrong batch
    offset of A, W or the output, a dropped partial: another column, or 0.  Count: A all ones, 255 ones in every column of W with some
    in every 32-wide k-step of every wave's range: 255 everywhere; a k-step dropped or taken twice gives another number.  Integer
    matmul with integer bias and residual rows: the result bit for bit, and with it stats_out - the integer sums and sums of squares of
    the stored values per 64 columns.  Rows at or beyond the live count keep the sentinel in out and in stats_out.
    Through the GELU epilogue the same exact pre-activations are held to float64 GELU within the bf16 store and gelu_erf's stated error;
    through HEADS the logits are float32 bit for bit and the value is held to float64 tanh."""
    L = tr.LINKS[link]
    ad = 225 if L["epi"] == "heads" else None
    worst = 0.0
    for kind in ("select", "count", "int"):
        worst = max(worst, sweep(link, n_out, kind, ad, want_stats=L["epi"] in ("bf16", "resid") and kind != "select"))
    print(f"RATIO exact_{link}_N{n_out} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("link,n_out", CASES)
def test_within_the_float64_bound(link, n_out):
    """Plain links: randn operands against the float64 product through the epilogue, 2^-8 |ref| + (K + 2) 2^-24 (|a| |w| + |b|), GELU
    with |x| / 2 times gelu_erf's erf error; no absolute slack.  LayerNorm links: rows that are one pattern times 2^(r mod 5) with their
    exact statistics - the register form adds the re-rounding of the normalised fragment (2^-9 sum |xhat| |w|) and the float32 error of
    rstd and shift, the LDS link 3 (LayerNorm in the epilogue, no re-rounding) its own derivation; tail_restated._ln counts the
    operations.  Statistics of the wrong row or of half the groups are off by a factor.
    Largest error / bound on an MI355X: see DESIGN.md, "What pins the cls-row tail links"."""
    L = tr.LINKS[link]
    worst = sweep(link, n_out, "ln" if L["ln"] else "randn", 225 if L["epi"] == "heads" else None)
    print(f"RATIO f64_{link}_N{n_out} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("action_dim", tr.ACTION_DIMS)
def test_heads_value_column(action_dim):
    """The merged heads at action_dim in every lane residue, on both sides of a 64-column group and with action_dim + 1 == n_out.
    Integer probe whose value column holds multiples of 2^-6 in (-4, 4), exactly 0 in every fourth row: the logits [m, action_dim]
    are the integers bit for bit, the value is exactly 0 where its argument is and within TANHF_MARGIN of float64 tanh elsewhere (the
    argument is exact, so the error is tanhf's own: printed as TANHF, in units of 2^-24); logits and values beyond the live rows keep
    the sentinel, and the padding columns beyond action_dim (which hold other integers) reach neither.  The LayerNorm + split-K heads
    run at the same action_dim against their float64 bound."""
    L = tr.LINKS["k512_heads"]
    n_out = tr.heads_n_out(action_dim)
    p, d, e = on_card("int", "k512_heads", n_out, action_dim)
    worst, terr = 0.0, 0.0
    for rows, live in [(m, None) for m in MS] + [(MBUF, c) for c in LIVE]:
        res = launch("k512_heads", n_out, d, rows, live, action_dim)
        n = rows if live is None else live
        worst = max(worst, check(res, e, L, n_out, n, (rows, live), action_dim))
        v = res["values"][:n].cpu()
        assert bool((v[0::4] == 0).all()), (rows, live)
        terr = max(terr, float((v.double() - e["values_ref"][:n]).abs().max()))
    print(f"TANHF ad{action_dim} {terr / tr.U32:.3f}")
    print(f"RATIO heads_value_ad{action_dim} {worst:.4f}")
    assert worst <= 1.0, worst
    worst = sweep("k512_ln_heads", n_out, "ln", action_dim)
    print(f"RATIO f64_k512_ln_heads_ad{action_dim} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("link", list(tr.LINKS))
def test_leading_dimensions(link):
    """Every link once with lda = its A width + 64, ldo = N + 128 and (RESID) ldr = 5 N, as strided views whose A pointer stays 16-byte
    aligned: the integer probe stays bit for bit with its statistics (GELU and LayerNorm links: their float64 bound), and every output
    column past N keeps the sentinel.  A residual row found with ldo lands elsewhere in the residual's buffer."""
    L = tr.LINKS[link]
    n_out = L["n_outs"][1] if len(L["n_outs"]) > 1 else L["n_outs"][0]
    ad = 225 if L["epi"] == "heads" else None
    p, d, e = on_card("ln" if L["ln"] else "int", link, n_out, ad)
    worst = 0.0
    for rows, live in ((33, None), (65, None), (MBUF, 1025)):
        res = launch(link, n_out, d, rows, live, ad, want_stats=L["epi"] in ("bf16", "resid") and not L["ln"], ld=True)
        worst = max(worst, check(res, e, L, n_out, rows if live is None else live, (rows, live), ad))
    print(f"RATIO ld_{link}_N{n_out} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("n_out", tr.LINKS["lds_k2048_resid"]["n_outs"])
def test_lds_link_4_with_two_ring_buffers(n_out):
    """azk_nn_tail_lds_footprint(1): the K = 2048 LDS link on two ring buffers instead of three - the same exact probes, bit for bit."""
    import azk
    lib = azk.lib()
    try:
        assert lib.azk_nn_tail_lds_footprint(1) == 0
        for kind in ("select", "count", "int"):
            assert sweep("lds_k2048_resid", n_out, kind, want_stats=kind != "select") == 0.0
    finally:
        lib.azk_nn_tail_lds_footprint(0)
