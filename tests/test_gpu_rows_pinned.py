"""The launch that writes what the tree reads on every network but the benchmark's - k_ln_heads<8> / <16> through azk.nn_ln_heads
(csrc/azk_rows.hip: final LayerNorm, merged policy / value head and tanh) - and its unfused read-out k_heads_finalize through
azk.nn_heads_finalize, pinned two ways.  The exact probe `balanced` (tests/rows_restated.py): rows m0 + s sigma with balanced signs, whose
statistics are exact in float32 in any order and whose normalised fragment the bf16 rounding returns to +-1 whatever rsqrtf's last bits
are; integer weights and bias; a value column whose tanh argument is a multiple of 2^-6, exactly 0 in every fourth row - logits bit for
bit at the ABI's default eps.  Float64 references on five kinds of rows with the bound rows_restated.ln_heads_f64 derives term by term;
each such test prints `RATIO <name> <largest error / bound>` before it asserts.  tests/test_rows_restated.py shows on the CPU which
probe notices which of eight deliberate mistakes; DESIGN.md, "What pins the library tail's row kernels", lists the tests here that
turn red when six of them are made in the kernel.

Every output buffer is pre-filled with a sentinel and four rows longer than the launch may write."""
import functools

import pytest
import torch
import torch.nn.functional as F

import rows_restated as rr

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 31, 32, 33, 64, 65)                      # no count: n < 16, both sides of the 16-row tile, the row clamp
LIVE = (0, 1, 16, 17, 33, 200, 256, 300)                      # device-side live counts on the MBUF-row buffer; 300 > n
MBUF = 256
PAD = 4
S = rr.SENTINEL
AZK_OK, AZK_ERR_ARG = 0, -1                                   # include/azk.h


@functools.lru_cache(maxsize=None)
def on_card(kind, D, action_dim):
    """(probe, x / wp / bias on the card, expected for all MBUF rows): built once, shared, never changed."""
    p = rr.balanced(D, action_dim, MBUF) if kind == "balanced" else rr.probe(kind, D, action_dim, MBUF)
    return p, {key: p[key].cuda() for key in ("x", "wp", "bias")}, rr.expected(p, action_dim)


@pytest.fixture(autouse=True, scope="module")
def release_shared_probes():
    yield
    on_card.cache_clear()
    rr.balanced.cache_clear()
    rr.probe.cache_clear()
    torch.cuda.empty_cache()


def count_on_card(live):
    return None if live is None else torch.tensor([live], dtype=torch.int32, device="cuda")


def launch(d, action_dim, rows, live=None):
    """azk.nn_ln_heads on the first `rows` rows -> (logits, values), each PAD rows longer than the launch may write."""
    import azk
    lg = torch.full((rows + PAD, action_dim), S, device="cuda")
    v = torch.full((rows + PAD,), S, device="cuda")
    azk.nn_ln_heads(d["x"][:rows], d["wp"], d["bias"], action_dim, lg, v, count=count_on_card(live))
    torch.cuda.synchronize()
    return lg.cpu(), v.cpu()


def sweep(kind, D, action_dim):
    """The probe at every M of MS with no count and on the MBUF-row buffer under every live count of LIVE: bits or bound on the live
    rows, the sentinel everywhere else, and every live row's bits the same as without a count.  -> largest error / bound."""
    p, d, e = on_card(kind, D, action_dim)
    full = launch(d, action_dim, MBUF)
    worst = 0.0
    for rows, live in [(m, None) for m in MS] + [(MBUF, c) for c in LIVE]:
        lg, v = launch(d, action_dim, rows, live)
        n = rows if live is None else min(rows, live)
        ok, w = rr.agrees(lg, v, e, n)
        assert ok, (kind, D, action_dim, rows, live, w)
        assert torch.equal(lg[:n], full[0][:n]) and torch.equal(v[:n], full[1][:n]), (kind, D, action_dim, rows, live)
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("action_dim", rr.EXACT_ACTION_DIMS)
@pytest.mark.parametrize("D", rr.WIDTHS)
def test_exact_probe_bit_for_bit(D, action_dim):
    """k_ln_heads<8> and <16> at action_dim in one group (7, 9, 49), in every lane residue and on both sides of a 64-column group
    (63, 64, 225 .. 228, 255: 64 and 255 have action_dim + 1 == n_out) and with seven groups (399, 400: `item % ngroups` moves
    against the four waves of a block).  Logits are the integers sigma W^T + b bit for bit; the value is exactly 0 in every fourth
    row and within TANHF_MARGIN of float64 tanh elsewhere; rows at or beyond the live count keep the sentinel (counts 0, 1 and 300
    > n included); a row's bits do not depend on the count or on M.
    What it is there for: a dropped cross-lane add or a wrong variance (v is no longer +-1), a stale weight fragment in k-steps >= 4
    (other integers; <8> takes the prefetch-and-rotate branch once, <16> three times), a bias read from the wrong group, a value
    column one lane off (no zeros in every fourth row), a missing tanh, a row written behind the count."""
    worst = sweep("balanced", D, action_dim)
    print(f"RATIO exact_D{D}_ad{action_dim} {worst:.4f}")       # the value column against TANHF_MARGIN; the logits are bits
    assert worst <= 1.0, worst


@pytest.mark.parametrize("kind", rr.KINDS)
@pytest.mark.parametrize("D", rr.WIDTHS)
def test_within_the_float64_bound(D, kind):
    """Rows of one kind (pattern: exact sums; random; one-hot; constant: var = 0; mean100_ulp: var = 1 / 6 under mean^2 = 10^4, where
    the one-pass statistics lose 1.4e-3 .. 3.0e-3 of rstd) against float64 LayerNorm x W^T + b at action_dim 49, 225, 400.  The bound
    (rows_restated.ln_heads_f64) counts the kernel's own summation depth and keeps the cancellation term of E2 - mean^2.
    Largest error / bound on an MI355X: see DESIGN.md, "What pins the library tail's row kernels"."""
    worst = 0.0
    for action_dim in rr.F64_ACTION_DIMS:
        worst = max(worst, sweep(kind, D, action_dim))
    print(f"RATIO f64_{kind}_D{D} {worst:.4f}")
    assert worst <= 1.0, worst


def test_ln_heads_grid_stride_second_trip():
    """azk_nn_ln_heads launches at most 4096 blocks of four waves.  D = 256, action_dim = 400 (seven groups), n = 37 441: 2 341 row
    tiles x 7 = 16 387 wave tiles, three more than 16 384, so waves 0 .. 2 of block 0 make a second trip - to groups 4, 5, 6 (the
    value column's) of the last tile, which has one live row.  The exact probe's first 64 rows, tiled: the expectation is 64 rows."""
    D, ad, n = 256, 400, 37441
    assert ((n + 15) // 16) * (rr.heads_n_out(ad) // 64) == 16387 and n % 16 == 1
    p, d, e = on_card("balanced", D, ad)
    x = d["x"][:64].repeat((n + 63) // 64, 1)[:n].contiguous()
    import azk
    lg = torch.full((n + PAD, ad), S, device="cuda")
    v = torch.full((n + PAD,), S, device="cuda")
    azk.nn_ln_heads(x, d["wp"], d["bias"], ad, lg, v)
    torch.cuda.synchronize()
    want = e["logits"][:64].cuda()
    whole = n // 64 * 64
    assert bool((lg[:whole].view(-1, 64, ad) == want[None]).all())
    assert torch.equal(lg[whole:n], want[: n - whole])
    assert bool((lg[n:] == S).all()) and bool((v[n:] == S).all())
    vref = e["values_ref"][:64].repeat((n + 63) // 64)[:n]
    vc = v[:n].cpu()
    assert bool((vc[0::4] == 0).all())
    worst = float((vc.double() - vref).abs().max()) / rr.TANHF_MARGIN
    print(f"RATIO grid_stride_ln_heads {worst:.4f}")
    assert worst <= 1.0, worst


def finalize(heads, action_dim, live=None):
    import azk
    n = heads.shape[0]
    lg = torch.full((n + PAD, action_dim), S, device="cuda")
    v = torch.full((n + PAD,), S, device="cuda")
    azk.nn_heads_finalize(heads, action_dim, lg, v, count=count_on_card(live))
    torch.cuda.synchronize()
    return lg.cpu(), v.cpu()


@pytest.mark.parametrize("n,action_dim,ld", [(1200, 225, 232), (1200, 225, 226), (33, 7, 8), (1, 49, 56)])
def test_heads_finalize_bits_and_second_trip(n, action_dim, ld):
    """k_heads_finalize runs 1024 blocks of 256 threads over n (A + 1) elements: 1200 x 226 = 271 200 is more than 262 144, so the
    grid-stride loop makes a second trip.  Logits are the bf16 inputs widened, bit for bit; the value is exactly 0 where its
    argument is and within TANHF_MARGIN of float64 tanh elsewhere (arguments: multiples of 2^-6 in (-4, 4)); ld = A + 1 and
    ld = A + 7; counts 0, 1, n - 1, n, n + 5; what the columns behind the value column hold appears nowhere in the outputs."""
    assert n < 1200 or n * (action_dim + 1) > 1024 * 256
    p = rr.finalize_probe(n, action_dim, ld)
    heads = p["heads"].cuda()
    worst = 0.0
    for live in (None, 0, 1, n - 1, n, n + 5):
        lg, v = finalize(heads, action_dim, live)
        m = n if live is None else min(n, live)
        assert torch.equal(lg[:m], p["logits"][:m]), live
        assert bool((lg[m:] == S).all()) and bool((v[m:] == S).all()), live
        assert not bool((lg == rr.POISON).any()) and not bool((v == rr.POISON).any()), live
        assert bool((v[:m][0::4] == 0).all()), live
        if m:
            worst = max(worst, float((v[:m].double() - p["values_ref"][:m]).abs().max()) / rr.TANHF_MARGIN)
    print(f"RATIO heads_finalize_n{n}_ad{action_dim}_ld{ld} {worst:.4f}")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("R,D,heads", [(7, 256, 8), (15, 512, 4)])
def test_the_products_own_operands(R, D, heads):
    """A clsfold network whose tail is the library form (7 x 7, D = 256, A = 49; 15 x 15, D = 512 with 4 heads, whose head width 128
    keeps it off the chain): azk.nn_ln_heads on the network's own packed weight WhGP (LayerNorm's affine folded in) and bias bhG_f,
    against float64 LayerNorm + heads from the MASTER weights with the affine unfolded.  On top of the probe bound: the rounding of
    W gamma to bf16, 2^-9 |xhat| |W gamma|, and the float32 evaluation of W beta + b, (D + 2) 2^-24 (|W| |beta| + |b|).
    Then the unfused branch of the same tail (fuse_ln_heads = False: k_ln_rows, the library GEMM on bf16 Wh / bh, k_heads_finalize)
    against the same reference: k_ln_rows' bound (block_restated.ln_bound) through |Wh|, the weights' and the bias' own bf16
    rounding, the float32 accumulation, and the bf16 store of the GEMM's output."""
    import azk
    import block_restated as br
    from pvnet import NetConfig, PolicyValueNet
    A = R * R
    net = PolicyValueNet(NetConfig(R, R, 2, A, 5, D, heads, 1), seed=8, device="cuda", dtype=torch.bfloat16, path="clsfold")
    assert net.hip_tail and net.fuse_ln_heads and not net.chain_tail
    assert net.tail_choice(torch.empty(0, dtype=torch.bfloat16)) == "library"
    f, m = net._fold, net.master
    n, live = 70, 37
    x = torch.cat([rr.rows_of("random", n - 10, D, 21), rr.rows_of("mean100_ulp", 4, D, 22), rr.rows_of("onehot", 4, D, 23),
                   rr.rows_of("constant", 2, D, 24)])
    xc = x.cuda()
    g, beta = m["norm.weight"].cpu().double(), m["norm.bias"].cpu().double()
    Ap = f["Wh"].shape[0]
    Wh = torch.zeros(Ap, D, dtype=torch.float64)
    bh = torch.zeros(Ap, dtype=torch.float64)
    Wh[:A], bh[:A] = m["policy_head.weight"].cpu().double(), m["policy_head.bias"].cpu().double()
    Wh[A], bh[A] = m["value_head.weight"].cpu().double()[0], m["value_head.bias"].cpu().double()[0]
    n_out = f["bhG_f"].numel()
    assert n_out == rr.heads_n_out(A) and f["WhGP"].numel() == n_out * D
    k = rr.ln_heads_f64(x, rr.unpack(f["WhGP"], n_out, D), f["bhG_f"].cpu())
    xhat = k["xhat"]
    Wg = Wh * g[None, :]
    pre = xhat @ Wg.t() + Wh @ beta + bh                                        # the reference: master weights, affine unfolded
    fold = 2.0 ** -9 * (xhat.abs() @ Wg.abs().t()) + (D + 2) * rr.U32 * (Wh.abs() @ beta.abs() + bh.abs())
    err = k["err"][:, :Ap] + fold
    e = dict(logits_ref=pre[:, :A], logits_bound=rr.U32 * pre[:, :A].abs() + err[:, :A], values_arg=pre[:, A],
             values_ref=torch.tanh(pre[:, A]), values_bound=err[:, A] + rr.TANHF_MARGIN)
    for cnt in (None, live):
        lg = torch.full((n + PAD, A), S, device="cuda")
        v = torch.full((n + PAD,), S, device="cuda")
        azk.nn_ln_heads(xc, f["WhGP"], f["bhG_f"], A, lg, v, count=count_on_card(cnt))
        torch.cuda.synchronize()
        ok, worst = rr.agrees(lg, v, e, n if cnt is None else cnt)
        print(f"RATIO product_fused_D{D}_count{cnt} {worst:.4f}")
        assert ok, worst
    # the unfused branch, as PolicyValueNet._tail_fast runs it with fuse_ln_heads = False and out_buffers set
    y64, xw, kappa = br.ln_f64(x, g, beta)
    lnb = br.ln_bound(y64, xw, kappa, g, beta)
    Whb, bhb = f["Wh"].cpu().double(), f["bh"].cpu().double()
    assert torch.equal(Whb, Wh.float().to(torch.bfloat16).double())
    yabs = y64.abs() + lnb
    acc = lnb @ Whb.abs().t() + y64.abs() @ (Whb - Wh).abs().t() + (bhb - bh).abs() + (D + 2) * rr.U32 * (yabs @ Whb.abs().t() + bhb.abs())
    ref = y64 @ Wh.t() + bh
    assert float((ref - pre).abs().max()) < 1e-9                                # the same reference, written the other way round
    err2 = acc + rr.bf16_half_ulp(ref.abs() + acc)
    e2 = dict(logits_ref=ref[:, :A], logits_bound=err2[:, :A], values_arg=ref[:, A], values_ref=torch.tanh(ref[:, A]),
              values_bound=err2[:, A] + rr.TANHF_MARGIN)
    for cnt in (None, live):
        c = count_on_card(cnt)
        lg = torch.full((n + PAD, A), S, device="cuda")
        v = torch.full((n + PAD,), S, device="cuda")
        out = F.linear(azk.nn_layernorm_rows(xc, f["lnf_w"], f["lnf_b"], 1e-5, count=c), f["Wh"], f["bh"])
        azk.nn_heads_finalize(out, A, lg, v, count=c)
        torch.cuda.synchronize()
        ok, worst = rr.agrees(lg, v, e2, n if cnt is None else cnt)
        print(f"RATIO product_unfused_D{D}_count{cnt} {worst:.4f}")
        assert ok, worst


def test_refusals_leave_the_outputs_alone():
    """The ABI's argument error for embed_dim = 128, n_out_padded of 32 or 96, action_dim + 1 > n_out_padded and (finalize)
    ld < A + 1, with both outputs left at the sentinel; n = 0 is OK and writes nothing."""
    import azk
    lib = azk.lib()
    st = torch.cuda.current_stream().cuda_stream
    n = 16
    x = torch.zeros(n, 512, dtype=torch.bfloat16, device="cuda")
    wp = torch.zeros(128 * 512, dtype=torch.bfloat16, device="cuda")
    bias = torch.zeros(128, device="cuda")
    heads = torch.zeros(n, 64, dtype=torch.bfloat16, device="cuda")
    lg = torch.full((n, 128), S, device="cuda")
    v = torch.full((n,), S, device="cuda")

    def ln_heads(rows, D, n_out, ad):
        return lib.azk_nn_ln_heads(x.data_ptr(), 1e-5, wp.data_ptr(), bias.data_ptr(), rows, D, n_out, ad, lg.data_ptr(), v.data_ptr(), None, st)

    def fin(rows, ld, ad):
        return lib.azk_nn_heads_finalize(heads.data_ptr(), ld, ad, rows, lg.data_ptr(), v.data_ptr(), None, st)

    for D, n_out, ad in ((128, 64, 49), (512, 32, 7), (256, 96, 49), (512, 64, 64), (256, 128, 128)):
        assert ln_heads(n, D, n_out, ad) == AZK_ERR_ARG, (D, n_out, ad)
    assert fin(n, 49, 49) == AZK_ERR_ARG and fin(n, 7, 49) == AZK_ERR_ARG
    assert ln_heads(0, 512, 64, 49) == AZK_OK and ln_heads(0, 256, 128, 100) == AZK_OK and fin(0, 64, 49) == AZK_OK
    torch.cuda.synchronize()
    assert bool((lg == S).all()) and bool((v == S).all())
    # and the same shapes accepted: the sentinel goes
    assert ln_heads(n, 512, 64, 63) == AZK_OK
    torch.cuda.synchronize()
    assert not bool((lg.view(-1)[: n * 63] == S).any()) and bool((lg.view(-1)[n * 63:] == S).all()) and not bool((v == S).any())
    lg.fill_(S)
    v.fill_(S)
    assert fin(n, 64, 63) == AZK_OK
    torch.cuda.synchronize()
    assert not bool((lg.view(-1)[: n * 63] == S).any()) and bool((lg.view(-1)[n * 63:] == S).all()) and not bool((v == S).any())
