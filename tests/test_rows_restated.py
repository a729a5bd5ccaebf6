"""The probes of tests/test_gpu_rows_pinned.py do their job, shown without a GPU: the float32 emulation of k_ln_heads
(tests/rows_restated.py) gives the exact probe's bits and stays inside every float64 bound, the exact probe meets the conditions it
rests on at both widths, and the emulation with one deliberate mistake gives other bits or leaves a bound.

Which probe catches which mistake (CAUGHT_BY below is asserted, entry by entry, at D = 256 and 512):

  mistake          exact probe `balanced`                                    float64 probes that leave their bound
  stats_half       bits (mean and var of half a row)                         all five
  stale_fragment   bits (other weights in k-steps >= 4)                      pattern, random, onehot, mean100_ulp
  bias_group0      bits, from two groups on (one group has no other bias)    all five, from two groups on
  no_mean_sq       bits (rows with m0 != 0)                                  pattern, random, onehot, mean100_ulp
  shift_sign       bits (rows with m0 != 0)                                  all five
  value_lane       zeros missing in every fourth row, values beyond tanh     all five
  no_tanh          values beyond TANHF_MARGIN (arguments up to 4)            random, onehot, mean100_ulp
  live_guard       sentinel gone behind a count that ends inside a tile      all five (the same sentinel check)

A constant row normalises to 0 whatever the weights and the variance are, so `constant` cannot see stale_fragment or no_mean_sq; it
stays because it is the one kind that drives rstd to 1 / sqrt(eps) and it does see the other six.  `pattern`'s value arguments are
small enough at some action_dim that raw and tanh agree within its bound.  No kind is blind to every mistake, so none is dropped."""
import pytest
import torch

import rows_restated as rr

M = 70                                                        # more than four 16-row tiles, not a multiple of 16
LIVE = 37                                                     # a count that ends inside a tile: live_guard writes rows 37 .. 47
ADS = (49, 225, 400)                                          # one group, four, seven

# mutation -> the float64 kinds that must leave their bound under it (at action_dim 225 and 400; 49 has one group: no bias_group0)
CAUGHT_BY = {
    "stats_half": ("pattern", "random", "onehot", "constant", "mean100_ulp"),
    "stale_fragment": ("pattern", "random", "onehot", "mean100_ulp"),
    "bias_group0": ("pattern", "random", "onehot", "constant", "mean100_ulp"),
    "no_mean_sq": ("pattern", "random", "onehot", "mean100_ulp"),
    "shift_sign": ("pattern", "random", "onehot", "constant", "mean100_ulp"),
    "value_lane": ("pattern", "random", "onehot", "constant", "mean100_ulp"),
    "no_tanh": ("random", "onehot", "mean100_ulp"),
    "live_guard": ("pattern", "random", "onehot", "constant", "mean100_ulp"),
}


def run(p, D, ad, mutate=None, rows=M, count=None):
    lg, v = rr.ln_heads_emulate(p["x"][:rows], p["wp"], p["bias"], rr.heads_n_out(ad), ad, count=count, mutate=mutate)
    live = rows if count is None else max(0, min(rows, count))
    return rr.agrees(lg, v, rr.expected(p, ad, rows), live)


@pytest.mark.parametrize("D", rr.WIDTHS)
def test_exact_probe_meets_its_conditions(D):
    """rows_restated.balanced asserts them while it builds the probe (exact partial sums, mean = m0, rstd = 1 / s at eps = 0, the bf16
    rounding to +-1 for every rstd within 8 ulp at eps 0 and 1e-5, integer logits, value arguments on the 2^-6 grid with exact zeros);
    here: at every action_dim the GPU file uses, and the margin itself."""
    for ad in rr.EXACT_ACTION_DIMS:
        p = rr.balanced(D, ad)
        arg = p["pre"][:, ad]
        assert bool((arg[0::4] == 0).all()) and bool((arg != 0).any()) and float(arg.abs().max()) < 4.0
        lg = p["pre"][:, :ad]
        assert torch.equal(lg, lg.round()) and float(lg.abs().max()) < 2 ** 10
        # all nine (m0, s) pairs within any nine consecutive rows
        x = p["x"].double()
        pairs = {(float(x[r].mean()), float(x[r].var(unbiased=False))) for r in range(9)}
        assert pairs == {(m0, s * s) for m0 in rr.BALANCED_M0 for s in rr.BALANCED_S}
    assert rr.balanced_margin(0.0) <= 2.0 ** -18                # two float32 roundings near 25
    assert rr.balanced_margin(rr.LN_EPS) <= rr.LN_EPS / (2 * 0.25) + 2.0 ** -18


@pytest.mark.parametrize("D", rr.WIDTHS)
def test_emulation_gives_the_exact_probes_bits(D):
    for ad in rr.EXACT_ACTION_DIMS:
        p = rr.balanced(D, ad)
        for rows, count in ((M, None), (256, None), (256, 0), (256, 1), (256, LIVE), (256, 300)):
            ok, worst = run(p, D, ad, rows=rows, count=count)
            assert ok, (ad, rows, count, worst)
        # and at eps = 0, where rstd is exact
        lg, v = rr.ln_heads_emulate(p["x"][:M], p["wp"], p["bias"], rr.heads_n_out(ad), ad, eps=0.0)
        assert rr.agrees(lg, v, rr.expected(p, ad, M), M)[0], ad


@pytest.mark.parametrize("D", rr.WIDTHS)
@pytest.mark.parametrize("kind", rr.KINDS)
def test_emulation_stays_inside_every_float64_bound(kind, D):
    for ad in rr.F64_ACTION_DIMS:
        p = rr.probe(kind, D, ad)
        ok, worst = run(p, D, ad, rows=256)
        assert ok, (ad, worst)
        assert worst > 1e-6                                   # the bound is of the error's own order somewhere, not vacuous


@pytest.mark.parametrize("D", rr.WIDTHS)
@pytest.mark.parametrize("mutate", rr.MUTATIONS)
def test_every_mistake_changes_the_exact_probe(mutate, D):
    count = LIVE if mutate == "live_guard" else None
    for ad in rr.EXACT_ACTION_DIMS:
        ok, _ = run(rr.balanced(D, ad), D, ad, mutate=mutate, count=count)
        one_group = rr.heads_n_out(ad) == 64
        assert ok == (mutate == "bias_group0" and one_group), ad
    if mutate == "live_guard":                                # a count on a tile's edge, or no count, leaves nothing to write
        assert run(rr.balanced(D, 225), D, 225, mutate=mutate, count=32)[0]
        assert run(rr.balanced(D, 225), D, 225, mutate=mutate, rows=64)[0]


@pytest.mark.parametrize("D", rr.WIDTHS)
@pytest.mark.parametrize("mutate", rr.MUTATIONS)
def test_every_mistake_leaves_the_float64_bounds_it_is_listed_for(mutate, D):
    count = LIVE if mutate == "live_guard" else None
    for ad in (225, 400):
        for kind in rr.KINDS:
            ok, worst = run(rr.probe(kind, D, ad), D, ad, mutate=mutate, count=count)
            if kind in CAUGHT_BY[mutate]:
                assert not ok, (kind, ad, worst)


@pytest.mark.parametrize("D", rr.WIDTHS)
def test_no_float64_probe_is_blind_and_the_wide_one_still_sees_the_statistics(D):
    """A probe on which no mistake leaves the bound would be dropped.  mean100_ulp has the widest bound (rho: what rstd may be off
    by, relative) and must still see half the statistics and a stale weight fragment."""
    for kind in rr.KINDS:
        assert any(kind in kinds for kinds in CAUGHT_BY.values())
    for ad in rr.F64_ACTION_DIMS:
        p = rr.probe("mean100_ulp", D, ad)
        rho = float(p["rho"].max())
        assert 1e-3 < rho < 1e-2, rho                         # 4.1e-3 at D = 256, 6.1e-3 at D = 512
        for mutate in ("stats_half", "stale_fragment"):
            ok, worst = run(p, D, ad, mutate=mutate)
            assert not ok and worst > 10.0, (mutate, worst)
        for kind in ("pattern", "random", "onehot"):
            assert float(rr.probe(kind, D, ad)["rho"].max()) < 1e-5


@pytest.mark.parametrize("D", rr.WIDTHS)
def test_one_pass_statistics_on_a_large_mean(D):
    """Where k_ln_heads' accuracy ends: on 100 + k / 2 rows the kernel's one-pass variance, in the kernel's own summation order, puts
    rstd off by 1.4e-3 (D = 256) or 3.0e-3 (D = 512) relative, a two-pass variance over the same sums by 7e-8.  The bound's rho
    covers the former with a factor of two to three."""
    x = rr.rows_of("mean100_ulp", 256, D, 11)
    xd = x.double()
    rstd64 = 1.0 / torch.sqrt(xd.var(1, unbiased=False) + rr.LN_EPS)
    mean, rstd, _ = rr.ln_heads_stats_f32(x.float(), rr.LN_EPS)
    one = float(((rstd[:, 0].double() - rstd64).abs() / rstd64).max())
    d = x.float() - mean[:, :1]
    two = torch.rsqrt((d * d).sum(1) * (1.0 / D) + rr.LN_EPS)
    two = float(((two.double() - rstd64).abs() / rstd64).max())
    w = torch.zeros(64, D)
    rho = float(rr.ln_heads_f64(x, w, torch.zeros(64))["rho"].max())
    print(f"ONEPASS D{D} one-pass {one:.3g} two-pass {two:.3g} rho {rho:.3g}")
    assert 3e-4 < one < rho and two < 2e-7


def test_pack_and_unpack_are_inverse_on_the_head_shapes():
    g = torch.Generator().manual_seed(5)
    for D in rr.WIDTHS:
        for ad in rr.EXACT_ACTION_DIMS:
            n_out = rr.heads_n_out(ad)
            w = torch.randn(n_out, D, generator=g)
            assert torch.equal(rr.unpack(rr.pack(w), n_out, D), rr.bf16(w))
            rows = torch.randn(ad + 1, D, generator=g)          # the product packs action_dim + 1 rows: zero rows fill the last group
            back = rr.unpack(rr.pack(rows), n_out, D)
            assert torch.equal(back[: ad + 1], rr.bf16(rows)) and bool((back[ad + 1:] == 0).all())


def test_heads_finalize_probe_and_its_emulation():
    for n, ad, ld in ((70, 225, 232), (70, 225, 226), (33, 7, 8)):
        p = rr.finalize_probe(n, ad, ld)
        arg = p["values_arg"]
        assert bool((arg[0::4] == 0).all()) and float(arg.abs().max()) < 4.0 and torch.equal(arg * 64, (arg * 64).round())
        assert not bool((p["logits"] == rr.POISON).any()) and not bool((p["logits"] == rr.SENTINEL).any())
        assert bool(torch.isfinite(p["logits"]).all())
        assert ld == ad + 1 or bool((p["heads"][:, ad + 1:].float() == rr.POISON).all())
        for count in (None, 0, 1, n - 1, n + 5):
            lg, v = rr.finalize_emulate(p["heads"], ad, count)
            live = n if count is None else min(n, count)
            assert torch.equal(lg[:live], p["logits"][:live]) and bool((lg[live:] == rr.SENTINEL).all())
            assert float((v[:live].double() - p["values_ref"][:live]).abs().max() if live else 0.0) <= rr.TANHF_MARGIN
            assert bool((v[live:] == rr.SENTINEL).all())
