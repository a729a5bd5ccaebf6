"""The probes of tests/test_gpu_gemm_h_pinned.py do their job, shown without a GPU: the float32 emulation of an fp16-plane tail link
(tests/gemm_h_restated.py) gives every probe's expected bits (or stays inside its float64 bound), the probes' inputs meet the exactness
conditions they rest on, and the emulation with one deliberate mistake gives other bits (or leaves the bound).  The mistakes are
lettered as in DESIGN.md, "What pins the fp16-plane tail links"."""
import pytest
import torch

import gemm_h_restated as gh

M = 70                                                        # more than one 64-row tile; 70 rows of the selection land in every chain's K range
AD = 225
FIRST = [(link, L["n_outs"][0]) for link, L in gh.LINKS.items()]
SPLIT = [(link, n) for link, n in FIRST if not gh.LINKS[link]["lds"] and gh.chains(gh.LINKS[link], n) > 1]
AF32 = [link for link, L in gh.LINKS.items() if L["af32"]]
LN = [(link, n) for link, n in gh.CASES if gh.LINKS[link]["ln"]]


def ad_of(L):
    return AD if L["epi"] == "heads" else None


def exact_kinds(L):
    return ("select", "terms", "count") + (("ln_exact",) if L["ln"] else ("int",)) + (("mirror",) if L["af32"] else ())


def ratio(kind, link, n_out, mutate=None, action_dim=None, **over):
    """Largest error / bound (0: every bit as expected, inf: some bit differs) of the emulation, or of one mistake, on a probe."""
    L = gh.LINKS[link]
    ad = action_dim if action_dim is not None else ad_of(L)
    p = gh.probe(kind, link, n_out, M, ad)
    return gh.verdict(gh.emulate_probe(p, L, n_out, M, ad, mutate=mutate, **over), gh.expected(p, L, action_dim=ad), L)


@pytest.mark.parametrize("link,n_out", gh.CASES)
def test_exact_probes_meet_their_conditions_and_the_emulation_gives_their_bits(link, n_out):
    """Every scaled operand an integer (the selection's W and the mirror's A carry 22-bit significands, and the terms probe's A is
    (2048 m + l) / 2048: dyadic fractions, measured on each output's own grid), every plane pair exact (asserted where the probe is
    built), every partial sum an integer below 2^24 - in units of 1 / 4096 for the terms, the count, the integer matmul and the
    LayerNorm probe - and non-zeros in every 32-wide k-step of the count's and the terms' weights."""
    L = gh.LINKS[link]
    for kind in exact_kinds(L):
        p = gh.probe(kind, link, n_out, M, ad_of(L))
        x = gh.exactness(p, L, n_out, 8)
        assert x["partial"] < 2 ** 24, (kind, x)
        assert x["literal"] == (kind not in ("select", "mirror")), (kind, x)
        assert x["integer_w"] == (kind != "select") and x["integer_a"] == (kind not in ("terms", "mirror")), (kind, x)
        assert torch.equal(p["pre"].float().double(), p["pre"]), kind
        assert ratio(kind, link, n_out) <= 1.0, kind
        if L["epi"] in ("plain", "resid"):
            # every bit as expected (a differing bit is inf); the selection's and the terms' statistics are held to their bound
            assert ratio(kind, link, n_out) == 0.0 or kind in ("select", "terms", "mirror"), kind
            assert gh.expected(p, L)["stats_exact"] == (kind in ("count", "int")), kind
    steps = lambda t: t.abs().reshape(t.shape[0], -1, 32).sum(2)
    ahi, alo, whi, wlo = gh.probe("terms", link, n_out, M, ad_of(L))["planes"]
    live = whi.abs().sum(1) > 0                                           # (HEADS blanks the value column)
    assert bool((steps(whi)[live] > 0).all()) and bool((steps(wlo)[live] > 0).all()) and bool((ahi != 0).all()) and bool((alo != 0).all())
    whi = gh.probe("count", link, n_out, M, ad_of(L))["planes"][2]
    live = whi.sum(1) > 0
    assert bool((steps(whi)[live] >= 256.0).all()) and bool((whi[live].sum(1) == 255 * 256.0).all())
    w = gh.probe("select", link, n_out, M, ad_of(L))["planes"][3]
    assert float((w != 0).double().mean()) > 0.95                         # the selection's W: lo != 0 almost everywhere


@pytest.mark.parametrize("link,n_out", gh.CASES)
def test_emulation_meets_the_float64_bounds(link, n_out):
    L = gh.LINKS[link]
    for kind in (("ln_rand",) if L["ln"] else ("dense", "sparse")):
        assert ratio(kind, link, n_out) <= 1.0, kind


@pytest.mark.parametrize("link,n_out", FIRST)
def test_a_third_term_on_the_wrong_plane_changes_the_terms_probe(link, n_out):
    """(a) lo x the weight's lo plane: the terms probe gives other bits on every link, and the sparse rows leave their bound by orders
    of magnitude.  The selection (A's lo plane is 0) and the count cannot tell; the dense rows' worst-case bound can hide it."""
    L = gh.LINKS[link]
    assert ratio("terms", link, n_out, "lo_lo") > 1.0
    assert ratio("select", link, n_out, "lo_lo") <= 1.0 and ratio("count", link, n_out, "lo_lo") <= 1.0
    if not L["ln"]:
        assert ratio("sparse", link, n_out, "lo_lo") > 30.0


@pytest.mark.parametrize("link,n_out", SPLIT)
def test_split_k_mistakes_change_the_exact_probes(link, n_out):
    """(b) the reduction stops one wave early: selection, terms, count (255 -> 191 or 192), integer matmul.  (c) every wave reads A's
    first K range: all but the count, whose A is all ones."""
    L = gh.LINKS[link]
    for kind in exact_kinds(L):
        if kind == "mirror":
            continue
        assert ratio(kind, link, n_out, "reduce3") > 1.0, kind
        assert (ratio(kind, link, n_out, "a_first_range") > 1.0) == (kind != "count"), kind


@pytest.mark.parametrize("n_out", gh.LINKS["lds_k2048_resid"]["n_outs"])
def test_a_chain_left_out_of_the_lds_sum_changes_the_exact_probes(n_out):
    """(i) the last of link 4's four chains never joins the fixed-order sum."""
    for kind in ("select", "terms", "count", "int"):
        assert ratio(kind, "lds_k2048_resid", n_out, "lds_chain") > 1.0, kind


@pytest.mark.parametrize("link", ("k512_resid", "k2048_resid", "lds_k2048_resid"))
def test_residual_found_with_the_output_stride_changes_the_integer_probe(link):
    """(d), with ldr = 5 n_out against ldo = n_out + 128: the mistaken read stays inside the residual's buffer.  Contiguous operands
    (ldr = ldo) cannot see it."""
    L = gh.LINKS[link]
    n_out = L["n_outs"][0]
    p = gh.probe("int", link, n_out, M)
    rv, rbuf = gh.br.strided(p["resid"], 5 * n_out, -3.0)
    ldo = n_out + 128
    assert (M - 1) * ldo + n_out <= rbuf.numel()
    assert ratio("int", link, n_out, resid=rv, ldo=ldo) == 0.0
    assert ratio("int", link, n_out, "resid_ldo", resid=rv, ldo=ldo) > 1.0
    assert ratio("int", link, n_out, "resid_ldo", ldo=n_out) == 0.0


@pytest.mark.parametrize("link", ("k384_f32_b8", "k512_f32_b8"))
def test_bias_without_the_batch_offset_changes_the_integer_probe(link):
    """(e): every batch but the first gets batch 0's bias.  The selection, the terms and the count carry no bias and cannot tell."""
    assert ratio("int", link, 64, "col0_no_batch") > 1.0
    L = gh.LINKS[link]
    p = gh.probe("int", link, 64, M)
    bad = gh.emulate_probe(p, L, 64, M, mutate="col0_no_batch")
    assert torch.equal(bad["f32"][:, :64], gh.expected(p, L)["f32"][:, :64])
    assert ratio("select", link, 64, "col0_no_batch") <= 1.0


@pytest.mark.parametrize("link,n_out", LN)
def test_statistics_mistakes_change_the_layernorm_probe(link, n_out):
    """(f) groups 0 and 1 only: with the shares 1 .. 7, 36 of 64 the mean and the variance shrink 21-fold - other bits on the exact
    probe, out of the bound on the real statistics.  (g) mean and rstd of fragment row j in place of row 4 l4 + j: twelve of every
    sixteen rows get another row's mean (the exact probe's means differ between them; so do the scaled rows' statistics)."""
    for mut in ("stats_01", "ln_lane_j"):
        assert ratio("ln_exact", link, n_out, mut) > 1.0, mut
        assert ratio("ln_rand", link, n_out, mut) > 1.0, mut
    L = gh.LINKS[link]
    p = gh.probe("ln_exact", link, n_out, M, ad_of(L))
    st = p["a_stats"].double()
    mean, e2 = st[:, :, 0].sum(1) / 512, st[:, :, 1].sum(1) / 512
    r = torch.arange(M)
    assert torch.equal(mean.abs(), torch.exp2((r % 3).double())) and torch.equal(e2 - mean * mean, torch.pow(4.0, (r % 4).double()))
    assert torch.equal(p["csum"].double(), p["w64"].sum(1))                # integer W: col_sums is exact


@pytest.mark.parametrize("link", AF32)
def test_a_float32_split_without_its_lo_plane_changes_the_mirror_probe(link):
    """(h): the one-hot A's 22-bit value loses its low eleven bits.  The selection's A (1 or 2) cannot tell; the sparse rows leave
    their bound by orders of magnitude."""
    n_out = gh.LINKS[link]["n_outs"][0]
    assert ratio("mirror", link, n_out, "split_lo0") > 1.0
    assert ratio("select", link, n_out, "split_lo0") <= 1.0
    assert ratio("sparse", link, n_out, "split_lo0") > 30.0


@pytest.mark.parametrize("action_dim", gh.ACTION_DIMS)
def test_value_column_probe_holds_exact_zeros_and_bounded_arguments(action_dim):
    L = gh.LINKS["k512_heads"]
    n_out = gh.heads_n_out(action_dim)
    p = gh.probe("value", "k512_heads", n_out, M, action_dim)
    e = gh.expected(p, L, action_dim=action_dim)
    arg = e["values_arg"]
    assert bool((arg[0::4] == 0).all()) and bool((arg != 0).any()) and float(arg.abs().max()) < 4.0
    assert torch.equal(arg * 64, (arg * 64).round())
    assert gh.exactness(p, L, n_out, 8)["partial"] < 2 ** 24
    got = gh.emulate_probe(p, L, n_out, M, action_dim)
    assert bool((got["values"][0::4] == 0).all()) and gh.verdict(got, e, L) <= 1.0
    off = gh.emulate_probe(p, L, n_out, M, action_dim - 1)
    assert not bool((off["values"][0::4] == 0).all())


@pytest.mark.parametrize("link", ("k512_plain", "k512_resid", "k512_f32", "k2048_plain", "lds_k2048_resid"))
def test_overflow_probe_sits_on_the_threshold(link):
    """65472 everywhere: clear; 65504 (either sign) in one place: set - and the values themselves stay exact."""
    L = gh.LINKS[link]
    for at, sign in ((gh.F16_BELOW_MAX, 1.0), (gh.F16_MAX, 1.0), (gh.F16_MAX, -1.0)):
        o = gh.overflow_probe(link, at, sign)
        got = gh.emulate(o["a"], o["wp"], o["n_out"], L["k"], L["epi"], gh.chains(L, o["n_out"]), bias=o["bias"], resid=o["resid"])
        assert torch.equal(got["f32"].double(), o["want"]) and got["oflow"] == o["expect_flag"], (at, sign)
        assert float(o["want"].abs().max()) * gh.A_SCALE == (at if o["expect_flag"] else gh.F16_BELOW_MAX)


def as_7_1_26_f32(x):
    """The Abramowitz & Stegun 7.1.26 form with a true division, in float32, as gelu_as stated it (kept here, with the test that needs it,
    so that nothing else's helper decides this test)."""
    f = torch.float32
    c = lambda v: torch.tensor(v, dtype=f)
    x = x.float()
    z = x.abs() * c(0.70710678118654752)
    t = 1.0 / (1.0 + c(0.3275911) * z)
    poly = t * (c(0.254829592) + t * (c(-0.284496736) + t * (c(1.421413741) + t * (c(-1.453152027) + t * c(1.061405429)))))
    return c(0.5) * x * (1.0 + torch.copysign(1.0 - poly * torch.exp(-z * z), x))


def test_the_float32_gelu_meets_its_bound_and_the_former_form_did_not():
    """Over [-8, 8] in 2 000 001 steps: 0.5 x (1 + erff) stays inside |x| / 2 (1.5e-7 + the __expf share) + 2 u |x|; the Abramowitz &
    Stegun form evaluated in float32 leaves it (DESIGN.md records by how much: 2.28 times the erf budget alone, 1.21 times with the
    result's two roundings, largest near x = 0.035 where 1 - poly exp cancels)."""
    x = torch.linspace(-8.0, 8.0, 2_000_001, dtype=torch.float64).float()
    ref = torch.nn.functional.gelu(x.double())
    bound = gh.gelu_bound(x.double(), torch.zeros_like(ref))
    worst = lambda f: gh.worst_ratio((f(x).double() - ref).abs(), bound)
    assert worst(gh.gelu_erff_f32) <= 1.0
    assert worst(as_7_1_26_f32) > 1.0


def test_sixteen_rows_say_what_the_exactness_conditions_need():
    """`exactness` is asserted on a prefix because its per-output grid is a min-plus product over K.  What it rests on does not depend
    on the row: the selection and its mirror have ONE non-zero product per output (a 22-bit number times 1, 2 or a power of two); in
    the other exact probes every term product is an integer in the accumulator's units by construction (asserted on the prefix as
    `literal`), so the partial sums of ALL rows are bounded by the largest sum of |term products|, which `partial_all_rows` takes
    over every row - tests/test_gpu_gemm_h_pinned.py asserts both on the 2048-row probes it runs."""
    for link, n_out in (("k2048_plain", 128), ("k384_f32_b8", 64), ("k512_ln_heads", 256)):
        L = gh.LINKS[link]
        for kind in exact_kinds(L):
            p = gh.probe(kind, link, n_out, M, ad_of(L))
            x = gh.exactness(p, L, n_out, 16)
            assert x["partial"] < 2 ** 24, (kind, x)
            if x["literal"]:
                assert x["partial"] <= gh.partial_all_rows(p, L, n_out) < 2 ** 24, kind
