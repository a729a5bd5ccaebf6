"""The probes of tests/test_gpu_tail_pinned.py do their job, shown without a GPU: the float32 emulation of a cls-row tail link
(tests/tail_restated.py) gives every probe's expected bits (or stays inside its float64 bound), the probes' inputs meet the
exactness conditions they rest on, and the emulation with one deliberate mistake gives other bits (or leaves the bound)."""
import pytest
import torch

import tail_restated as tr

M = 70                                                        # more than one 64-row tile; 70 rows of the selection land in every wave's K range
CASES = [(link, n_out) for link, L in tr.LINKS.items() for n_out in L["n_outs"]]
PLAIN_CASES = [(link, n_out) for link, n_out in CASES if not tr.LINKS[link]["ln"]]
LN_CASES = [(link, n_out) for link, n_out in CASES if tr.LINKS[link]["ln"]]
SPLIT = [n for n, L in tr.LINKS.items() if L["nwk"] > 1 and not L["lds"] and not L["ln"]]
AD = 225


def same(a, b):
    return torch.equal(tr.bits(a), tr.bits(b))


def ratio(got, ref, bound):
    return tr.worst_ratio((got.double() - ref).abs(), bound)


def agrees(got, e, L, stats=True):
    """The emulation's (or a mutant's) result against `expected`: bits where the probe gives bits, else the bound."""
    if L["epi"] == "heads":
        lg = torch.equal(got["logits"], e["logits"]) if "logits" in e else ratio(got["logits"], e["logits_ref"], e["logits_bound"]) <= 1.0
        return lg and ratio(got["values"], e["values_ref"], e["values_bound"]) <= 1.0
    if "out" in e:
        return same(got["out"], e["out"]) and (not stats or torch.equal(got["stats"], e["stats"]))
    return ratio(got["out"], e["ref"], e["bound"]) <= 1.0


def ad_of(L):
    return AD if L["epi"] == "heads" else None


@pytest.mark.parametrize("link,n_out", PLAIN_CASES)
def test_exact_probes_meet_their_conditions_and_the_emulation_gives_their_bits(link, n_out):
    L = tr.LINKS[link]
    for kind in ("select", "count", "int"):
        p = tr.probe(kind, link, n_out, M, ad_of(L) if kind == "int" else None)
        S, fits, sq = tr.exactness(p, L, L["epi"])
        assert S < 2 ** 24, (kind, S)                         # every partial sum is exact in float32, in any order
        if L["epi"] in ("bf16", "resid"):
            assert fits, kind                                 # what the epilogue stores has at most 8 significant bits
            if kind != "select":
                assert sq < 2 ** 24, (kind, sq)               # the row statistics are integers below 2^24
        e = tr.expected(p, L, action_dim=ad_of(L))
        assert agrees(tr.emulate(p, L, n_out, M, ad_of(L)), e, L, stats=kind != "select"), kind
    p = tr.probe("count", link, n_out, M)
    w = tr.unpack(p["wp"], L["nbatch"] * n_out, L["k"]).view(-1, L["nwk"], L["k"] // L["nwk"] // 32, 32)
    assert bool((w.sum(3) >= 1).all()) and bool((w.sum((1, 2, 3)) == 255).all())     # ones in every k-step of every wave's range


@pytest.mark.parametrize("link,n_out", CASES)
def test_emulation_meets_the_float64_bounds(link, n_out):
    L = tr.LINKS[link]
    p = tr.probe("ln" if L["ln"] else "randn", link, n_out, M)
    e = tr.expected(p, L, action_dim=ad_of(L))
    assert agrees(tr.emulate(p, L, n_out, M, ad_of(L)), e, L)
    if L["ln"]:
        # the scaled rows carry one normalised pattern: the float64 result of row r is that of row r - 5 to eps / var
        assert float((p["pre"][5:] - p["pre"][:-5]).abs().max()) < 1e-4


@pytest.mark.parametrize("link", SPLIT)
def test_split_k_mistakes_change_the_exact_probes(link):
    """(a) the reduction stops one wave early: selection (rows whose slot lies in the last range), count (255 -> 191 or 192), integer
    matmul.  (b) every wave reads A's first K range: selection and integer matmul (the count's A is all ones and cannot tell)."""
    L = tr.LINKS[link]
    n_out = L["n_outs"][0]
    for kind in ("select", "count", "int"):
        p = tr.probe(kind, link, n_out, M)
        e = tr.expected(p, L)
        assert not agrees(tr.emulate(p, L, n_out, M, mutate="reduce3"), e, L, stats=False), kind
        assert agrees(tr.emulate(p, L, n_out, M, mutate="a_first_range"), e, L, stats=False) == (kind == "count"), kind


def test_split_k_mistakes_leave_the_bound_on_the_layernorm_heads():
    L = tr.LINKS["k512_ln_heads"]
    p = tr.probe("ln", "k512_ln_heads", 256, M)
    e = tr.expected(p, L, action_dim=AD)
    for mut in ("reduce3", "a_first_range"):
        assert not agrees(tr.emulate(p, L, 256, M, AD, mutate=mut), e, L), mut


@pytest.mark.parametrize("n_out", tr.LINKS["lds_k2048_resid"]["n_outs"])
def test_a_chain_left_out_of_the_lds_sum_changes_the_exact_probes(n_out):
    """(f) one of link 4's four chain groups never joins the fixed-order sum."""
    L = tr.LINKS["lds_k2048_resid"]
    for kind in ("select", "count", "int"):
        p = tr.probe(kind, "lds_k2048_resid", n_out, M)
        assert not agrees(tr.emulate(p, L, n_out, M, mutate="lds_chain"), tr.expected(p, L), L, stats=False), kind


@pytest.mark.parametrize("link,n_out", LN_CASES)
def test_half_the_statistics_groups_leave_the_bound(link, n_out):
    """(c): mean and variance are off by about two, not by a rounding.  So are statistics taken from the neighbouring row."""
    L = tr.LINKS[link]
    p = tr.probe("ln", link, n_out, M)
    e = tr.expected(p, L, action_dim=ad_of(L))
    assert not agrees(tr.emulate(p, L, n_out, M, ad_of(L), mutate="stats_half"), e, L)
    assert not agrees(tr.emulate(p, L, n_out, M, ad_of(L), a_stats=torch.roll(p["a_stats"], 1, 0)), e, L)


@pytest.mark.parametrize("link", ("k512_resid", "k2048_resid", "lds_k2048_resid"))
def test_residual_found_with_the_output_stride_changes_the_integer_probe(link):
    """(d), with ldr = 5 n_out against ldo = n_out + 128: the mistaken read stays inside the residual's buffer.  Contiguous operands
    (ldr = ldo) cannot see it."""
    L = tr.LINKS[link]
    n_out = L["n_outs"][0]
    p = tr.probe("int", link, n_out, M)
    e = tr.expected(p, L)
    rv, rbuf = tr.br.strided(p["resid"], 5 * n_out, -3.0)
    ldo = n_out + 128
    assert (M - 1) * ldo + n_out <= rbuf.numel()
    assert agrees(tr.emulate(p, L, n_out, M, resid=rv, ldo=ldo), e, L)
    assert not agrees(tr.emulate(p, L, n_out, M, resid=rv, ldo=ldo, mutate="resid_ldo"), e, L)
    assert agrees(tr.emulate(p, L, n_out, M, ldo=n_out, mutate="resid_ldo"), e, L)


@pytest.mark.parametrize("link", ("k384_bf16_b8", "k512_bf16_b8"))
def test_bias_without_the_batch_offset_changes_the_integer_probe(link):
    """(e): every batch but the first gets batch 0's bias.  The selection and the count carry no bias and cannot tell."""
    L = tr.LINKS[link]
    n_out = L["n_outs"][0]
    p = tr.probe("int", link, n_out, M)
    e = tr.expected(p, L)
    bad = tr.emulate(p, L, n_out, M, mutate="bias_no_batch")
    assert not agrees(bad, e, L)
    assert same(bad["out"][:, :n_out].contiguous(), e["out"][:, :n_out].contiguous())


@pytest.mark.parametrize("action_dim", tr.ACTION_DIMS)
def test_value_column_probe_holds_exact_zeros_and_bounded_arguments(action_dim):
    L = tr.LINKS["k512_heads"]
    n_out = tr.heads_n_out(action_dim)
    assert action_dim + 1 <= n_out and (action_dim != 255 or n_out == 256)
    p = tr.probe("int", "k512_heads", n_out, M, action_dim)
    e = tr.expected(p, L, action_dim=action_dim)
    arg = e["values_arg"]
    assert bool((arg[0::4] == 0).all()) and bool((arg != 0).any()) and float(arg.abs().max()) < 4.0
    assert torch.equal(arg, arg.float().double()) and torch.equal(arg * 64, (arg * 64).round())
    got = tr.emulate(p, L, n_out, M, action_dim)
    assert bool((got["values"][0::4] == 0).all()) and agrees(got, e, L)
    assert got["logits"].shape == (M, action_dim)
    # a value column taken one lane residue off reads another column's integers: outside (-1, 1) or not 0 where 0 is due
    off = tr.emulate(p, L, n_out, M, action_dim - 1)
    assert not bool((off["values"][0::4] == 0).all())
