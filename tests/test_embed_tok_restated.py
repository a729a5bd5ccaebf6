"""The probes of tests/test_gpu_embed_tok_pinned.py do their job, shown without a GPU: the float32 emulation of k_embed and k_cls_pool
(tests/embed_tok_restated.py) gives every probe's expected output bit for bit, and the emulation with one deliberate mistake gives
something else on the geometries and token counts the probe is there for.  The emulation also meets the float64 bounds."""
import pytest
import torch

import embed_tok_restated as er


def same(a, b):
    return torch.equal(er.bits(a), er.bits(b))


def ratio(err, bound):
    r = torch.where(bound > 0, err / bound, torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
    return float(r.max())


def embed_probes(geom, D, H=4):
    C, R, Cc, k = geom
    boards = er.probe_boards(C, R, Cc, seed=R * 31 + Cc)
    wt, cpos = er.identity_probe(C, R, Cc, k, D)
    pr = er.int_probe(C, R, Cc, k, D, H, seed=R + Cc + D)
    return boards, (wt, cpos, er.identity_expected(boards, k, D)), (pr, er.int_expected_x(boards, pr))


def notices(geom, D, mistake):
    """-> (identity probe differs, integer probe differs) under one mistake."""
    boards, (wt, cpos, want_id), (pr, want_x) = embed_probes(geom, D)
    k = geom[3]
    a = er.embed_emulate(boards, wt, cpos, k, D, mutate=mistake)["x"]
    b = er.embed_emulate(boards, pr["wt_ext"], pr["cpos"], k, D, mutate=mistake)["x"]
    return not same(a, want_id), not same(b, want_x.to(torch.bfloat16))


@pytest.mark.parametrize("geom", er.GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_embed_probes_equal_the_emulation(geom):
    """Patch identity = F.unfold, the integer GEMM = unfold @ wt^T + cpos, both bit for bit from the emulated bit string, funnel shifts
    and plo / phi packing; on the integer probe xhat (both forms) and the scores of the emulation sit inside their float64 bounds."""
    D, H, k = 128, 4, geom[3]
    boards, (wt, cpos, want_id), (pr, want_x) = embed_probes(geom, D, H)
    assert same(er.embed_emulate(boards, wt, cpos, k, D)["x"], want_id)
    em = er.embed_emulate(boards, pr["wt_ext"], pr["cpos"], k, D, H, pr["mtab"], pr["msum"], pr["ln_w"], pr["ln_b"])
    assert same(em["x"], want_x.to(torch.bfloat16)) and torch.equal(em["x"].float(), want_x)
    y, xw, kappa, _, _ = er.ln_rows_f64(want_x, pr["ln_w"], pr["ln_b"])
    assert ratio((em["xhat"].double() - y).abs(), er.ln_bound(D, y, xw, kappa, pr["ln_w"], pr["ln_b"])) <= 1.0
    s, _ = er.int_scores_f64(boards, pr, want_x)
    assert ratio((em["scores"].double() - s).abs(), er.score_c(D) * er.U32 * s.abs()) <= 1.0


@pytest.mark.parametrize("D", (256, 512))
@pytest.mark.parametrize("geom", er.WIDE_GEOMS, ids=lambda g: "x".join(map(str, g)))
def test_embed_probes_equal_the_emulation_on_wide_rows(geom, D):
    boards, (wt, cpos, want_id), (pr, want_x) = embed_probes(geom, D, 8)
    assert same(er.embed_emulate(boards, wt, cpos, geom[3], D)["x"], want_id)
    assert same(er.embed_emulate(boards, pr["wt_ext"], pr["cpos"], geom[3], D)["x"], want_x.to(torch.bfloat16))


# which probe on which geometry notices which mistake (identity, integer): True = must differ, False = must not (the case is not there)
SEES = {
    "word_off_by_one": {(2, 15, 15, 5): (True, True), (2, 1, 1, 3): (True, True), (2, 20, 20, 5): (True, True),
                        (2, 31, 32, 3): (True, True), (3, 3, 3, 3): (True, True)},
    # a patch row straddles bit 64 only with 75 patch bits (p0 = 60, k = 5)
    "phi_carry_dropped": {(3, 6, 7, 5): (True, True), (2, 15, 15, 5): (False, False), (1, 8, 8, 7): (False, False)},
    "dead_row_kept": {(2, 15, 15, 5): (True, True), (2, 1, 30, 5): (True, True), (3, 3, 3, 3): (True, True),
                      (2, 31, 32, 3): (True, True)},
    # only a non-square board tells R Cc from R R
    "stride_RR": {(3, 6, 7, 5): (True, True), (2, 1, 30, 5): (True, True), (2, 30, 1, 5): (True, True), (2, 17, 18, 3): (True, True),
                  (2, 13, 30, 5): (True, True), (2, 15, 15, 5): (False, False), (2, 20, 20, 5): (False, False)},
    # columns D - 3 and D - 12 lie beyond the C k^2 <= 75 columns the identity weight fills: the integer GEMM over every column sees them
    "cols_swapped": {(2, 15, 15, 5): (False, True), (3, 6, 7, 5): (False, True)},
}


@pytest.mark.parametrize("mistake", er.EMBED_MISTAKES)
def test_each_embed_mistake_is_noticed_where_its_case_is(mistake):
    assert set(SEES) == set(er.EMBED_MISTAKES)
    for geom, want in SEES[mistake].items():
        assert notices(geom, 128, mistake) == want, (mistake, geom)


@pytest.mark.parametrize("D", (256, 512))
def test_swapped_columns_are_noticed_at_every_width(D):
    assert notices((3, 6, 7, 5), D, "cols_swapped") == (False, True)


def test_every_geometry_notices_a_patch_mistake():
    """Each geometry of the list sees at least the dead-row and the word-index mistake with both probes (a one-row board has dead rows
    in every patch, a one-cell board reads the word boundary at bit 31)."""
    for geom in er.GEOMS:
        for mistake in ("word_off_by_one", "dead_row_kept"):
            assert notices(geom, 128, mistake) == (True, True), (geom, mistake)


@pytest.mark.parametrize("geom,D,H", (((2, 7, 7, 5), 128, 4), ((3, 6, 7, 5), 256, 8), ((2, 16, 16, 5), 512, 8)))
def test_embed_emulation_meets_the_float64_bounds_on_random_operands(geom, D, H):
    C, R, Cc, k = geom
    boards = er.probe_boards(C, R, Cc, seed=5)
    pr = er.rand_probe(C, R, Cc, k, D, H, seed=D + R)
    ref = er.embed_f64(boards, pr["wt_ext"].float(), pr["cpos"], pr["mtab"], pr["msum"], k, D, H, pr["ln_w"], pr["ln_b"])
    em = er.embed_emulate(boards, pr["wt_ext"], pr["cpos"], k, D, H, pr["mtab"], pr["msum"], pr["ln_w"], pr["ln_b"])
    en = er.embed_emulate(boards, pr["wt_ext"], pr["cpos"], k, D, H, pr["mtab"], pr["msum"])
    assert ratio((em["x"].double() - ref["x"]).abs(), ref["x_bound"]) <= 1.0
    assert ratio((em["xhat"].double() - ref["xhat"]).abs(), ref["xhat_bound"]) <= 1.0
    assert ratio((en["xhat"].double() - ref["xn"]).abs(), ref["xn_bound"]) <= 1.0
    assert ratio((en["scores"].double() - ref["s"]).abs(), ref["s_bound"]) <= 1.0
    # and the bounds are not slack enough to hide a wrong patch bit
    bad = er.embed_emulate(boards, pr["wt_ext"], pr["cpos"], k, D, H, pr["mtab"], pr["msum"], mutate="dead_row_kept")
    assert ratio((bad["x"].double() - ref["x"]).abs(), ref["x_bound"]) > 1.0


def test_constant_rows_normalise_to_the_bias_exactly():
    """Zero weights and a constant cpos row: variance 0, xhat = bf16(ln_b) with the affine, 0 without, and every score 0."""
    R, Cc, k, D, H = 4, 5, 3, 128, 4
    boards = er.probe_boards(2, R, Cc, seed=1)
    pr = er.int_probe(2, R, Cc, k, D, H, seed=2)
    cpos = er.ln_case_probe(R, Cc, D)
    wt0 = torch.zeros_like(pr["wt_ext"])
    mtab = torch.zeros_like(pr["mtab"])
    mtab[:, :H] = cpos @ pr["mprime"].t()
    em = er.embed_emulate(boards, wt0, cpos, k, D, H, mtab, pr["msum"], pr["ln_w"], pr["ln_b"])
    assert torch.equal(em["x"].float(), cpos.expand(7, -1, -1))
    assert same(em["xhat"][:, 0::3], pr["ln_b"].to(torch.bfloat16).expand(7, len(range(0, R * Cc + 1, 3)), D).contiguous())
    assert bool((em["scores"][:, :, 0::3] == 0).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# k_cls_pool
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,H", ((128, 4), (256, 8)))
@pytest.mark.parametrize("T", er.POOL_T)
def test_pool_probes_are_exact_and_see_the_mistakes(T, D, H):
    """Select and mean probe = the emulation bit for bit, with plain and with NaN padding.  The softmax cut at 256 tokens is noticed by
    both probes for every T > 256 and for no other; a counted pad wherever there is one (T not a multiple of 16); a skipped last chunk
    at every T."""
    n = 5
    for probe in (er.pool_select_probe, er.pool_mean_probe):
        for poison in (False, True):
            xhat, s, c, want = probe(n, T, D, H, seed=T, poison=poison)
            assert same(er.pool_emulate(xhat, s, c, T), want), (probe.__name__, poison)
            assert same(er.pool_emulate(xhat, s, c, T, "cut256"), want) == (T <= 256), probe.__name__
            assert same(er.pool_emulate(xhat, s, c, T, "pad_counted"), want) == (T % 16 == 0), (probe.__name__, poison)
            assert not same(er.pool_emulate(xhat, s, c, T, "last_chunk_skipped"), want), probe.__name__


def test_pool_targets_visit_what_they_are_there_for():
    for T in er.POOL_T:
        for H in (4, 8):
            tg = er.pool_targets(5, H, T)
            seen = set(tg.reshape(-1).tolist())
            assert 0 in seen and T - 1 in seen and max(seen) < T
            assert len(seen) == min(5 * H, len(seen)) and (T < 5 * H or len(seen) == 5 * H)          # all different while T allows
            if T > 256:
                assert 256 in seen and (T == 257 or any(t > 256 for t in seen))
            pairs = {(t // 8) % 8 for t in seen}                                                  # (wave, register set) of the chunk
            assert pairs == set(range(min(8, (T + 7) // 8)))
            sets = er.pool_mean_sets(5, H, T)
            for S in sets.values():
                assert len(S) & (len(S) - 1) == 0 and len(set(S)) == len(S) and (T == 1 or {0, T - 1} <= set(S))
                assert T <= 258 or (256 in S and max(x for x in S if x != T - 1) > 256)


@pytest.mark.parametrize("T", (9, 226, 257, 401, 993))
def test_pool_emulation_meets_the_float64_bound(T):
    n, D, H = 5, 128, 4
    g = torch.Generator().manual_seed(T)
    for scale in (0.5, 8.0):
        xhat = torch.randn(n, T, D, generator=g).to(torch.bfloat16)
        s = torch.zeros(n, H, er.tp_of(T))
        s[:, :, :T] = torch.randn(n, H, T, generator=g) * scale
        c = torch.randn(H, generator=g)
        z, A, Smax = er.pool_f64(xhat, s, c, T)
        bound = er.pool_bound(z, A, T, Smax, float(xhat.float().abs().max()))
        assert ratio((er.pool_emulate(xhat, s, c, T).double() - z).abs(), bound) <= 1.0
        if T > 256:
            assert ratio((er.pool_emulate(xhat, s, c, T, "cut256").double() - z).abs(), bound) > 1.0


def test_pool_lds_limit():
    """Every (D, H) admits T = 993 (31 x 32); (512, 8) is the tightest and stops at Tp = 1 024."""
    for D, H in er.POOL_DH:
        assert er.pool_lds_bytes(993, D, H) <= 64 * 1024
    assert er.pool_lds_bytes(1024, 512, 8) <= 64 * 1024 < er.pool_lds_bytes(1025, 512, 8)
