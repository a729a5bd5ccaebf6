"""The fp32-accurate network path (csrc/azk_nnx.hip: k_embed_pool_x, k_embed_fold<EX>, k_gemm_h; VERDICT r02 'missing #1'): the reference evaluates
its network in float32 (ai/nn.py:74-84 at ai/mcts.py:46) and north_star asks for visit-count policies within 1e-5.  Checked here,
through the C ABI:
  * every kernel against the float64 evaluation of the same folded operands (pvnet.forward_exact_emulated) and against a plain
    torch float64 GEMM chain - tolerances are float32 rounding (1e-6 relative on O(1) values), written at each assert;
  * the whole evaluator against the reference's own seed-0 outputs (tests/golden/nn_small.npz full_*) at 1e-5;
  * 800-simulation searches from all 92 recorded positions of the reference's 15x15 games: pi IDENTICAL (<= 1e-5, i.e. not one
    visit moved) to the searches under the torch float32 'full' forward."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from pvnet import NetConfig, PolicyValueNet

pytestmark = pytest.mark.gpu

CFG = NetConfig(15, 15, 2, 225, 5, 512, 8, 1)


def random_boards(n, seed, max_stones=60):
    rng = np.random.RandomState(seed)
    x = np.zeros((n, 2, 15, 15), np.float32)
    for b in range(n):
        k = rng.randint(0, max_stones + 1)
        cells = rng.choice(225, size=2 * k, replace=False)
        x[b, 0].reshape(-1)[cells[:k]] = 1
        x[b, 1].reshape(-1)[cells[k:]] = 1
    return torch.from_numpy(x)


def test_gemm_h_against_float64():
    """azk_nnx_gemm_h (every operand as two fp16 terms on v_mfma_f32_16x16x32_f16): the chain of links of the tail - float32 A split
    on the fly, (hi, lo) planes from link to link, LayerNorm in the consuming epilogue (rstd (acc - mean col_sums) + bias), K = 2048
    with residual, heads - against float64.  Budget: operands carried to 22 bits (2.4e-7 relative per term), float32 accumulation:
    measured ~2e-6 on outputs of magnitude ~1, asserted at 3e-5; rows past the device-side count untouched.
    What this test still adds is the CHAIN: each link fed the planes and the statistics the previous one wrote.  As a check of any one
    link its 3e-5 / 5e-5 are redundant since tests/test_gpu_gemm_h_pinned.py, which holds every link on its own to exact bits and to
    bounds derived from the formats ("What pins the fp16-plane tail links"); they are kept as they were."""
    import azk
    g = torch.Generator("cuda").manual_seed(4)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)
    m = 300
    cnt = torch.tensor([257], dtype=torch.int32, device="cuda")
    planes = lambda c: (torch.full((m, c), 7.0, device="cuda", dtype=torch.float16), torch.full((m, c), 7.0, device="cuda", dtype=torch.float16))
    val = lambda p: (p[0].double() + p[1].double()) / azk.GEMM_H_A_SCALE
    # first link: float32 A, batched block-diagonal form
    z, wv = rn(m, 8 * 512), rn(8, 64, 512) * 0.05
    u = planes(512)
    azk.nnx_gemm_h(z, torch.cat([azk.pack_linear_weight_h(wv[h])[0].reshape(-1) for h in range(8)]), 64, 512, azk.TAIL_BF16, nbatch=8, a_batch_stride=512, out=u, count=cnt)
    ru = torch.einsum("nhd,hed->nhe", z.view(m, 8, 512).double(), wv.double()).reshape(m, 512)
    assert (val(u)[:257] - ru[:257]).abs().max().item() < 3e-5 and bool((u[0][257:] == 7.0).all())
    # planes in, planes + float32 + statistics out
    w, b = rn(512, 512) * 0.05, rn(512)
    wp, _ = azk.pack_linear_weight_h(w)
    x1, x1f, st = planes(512), torch.full((m, 512), 7.0, device="cuda"), torch.zeros(m, 8, 2, device="cuda")
    azk.nnx_gemm_h(u, wp, 512, 512, azk.TAIL_BF16, bias=b, out=x1, out_f32=x1f, stats_out=st, count=cnt)
    r1 = ru[:257] @ w.double().t() + b.double()
    assert (x1f[:257].double() - r1).abs().max().item() < 3e-5 and (val(x1)[:257] - r1).abs().max().item() < 3e-5 and bool((x1f[257:] == 7.0).all())
    # LayerNorm in the epilogue + GELU, wide N
    w0, b0 = rn(2048, 512) * 0.05, rn(2048)
    w0p, cs0 = azk.pack_linear_weight_h(w0)
    hh = planes(2048)
    azk.nnx_gemm_h(x1, w0p, 2048, 512, azk.TAIL_GELU, bias=b0, col_sums=cs0, out=hh, a_stats=st, count=cnt)
    ln = (r1 - r1.mean(1, keepdim=True)) / torch.sqrt(r1.var(1, unbiased=False, keepdim=True) + 1e-5)
    rh = torch.nn.functional.gelu(ln @ w0.double().t() + b0.double())
    assert (val(hh)[:257] - rh).abs().max().item() < 3e-5
    # K = 2048 + residual + statistics
    w3, b3 = rn(512, 2048) * 0.02, rn(512)
    x2, st2 = planes(512), torch.zeros(m, 8, 2, device="cuda")
    azk.nnx_gemm_h(hh, azk.pack_linear_weight_h(w3)[0], 512, 2048, azk.TAIL_RESID, bias=b3, resid=x1f, out=x2, stats_out=st2, count=cnt)
    r2 = r1 + rh @ w3.double().t() + b3.double()
    assert (val(x2)[:257] - r2).abs().max().item() < 5e-5
    # heads
    wh, bh = rn(256, 512) * 0.05, rn(256)
    whp, csh = azk.pack_linear_weight_h(wh)
    lg, vl = torch.full((m, 225), 7.0, device="cuda"), torch.full((m,), 7.0, device="cuda")
    azk.nnx_gemm_h(x2, whp, 256, 512, azk.TAIL_HEADS, bias=bh, col_sums=csh, a_stats=st2, logits=lg, values=vl, action_dim=225, count=cnt)
    ln2 = (r2 - r2.mean(1, keepdim=True)) / torch.sqrt(r2.var(1, unbiased=False, keepdim=True) + 1e-5)
    ro = ln2 @ wh.double().t() + bh.double()
    assert (lg[:257].double() - ro[:, :225]).abs().max().item() < 5e-5 and (vl[:257].double() - torch.tanh(ro[:, 225])).abs().max().item() < 1e-5
    assert bool((lg[257:] == 7.0).all()) and bool((vl[257:] == 7.0).all())


def test_embed_pool_x_against_float64():
    """k_embed_pool_x: z [n, H, 512] against the float64 evaluation of the same tables.  Budget: conv weights carried as two fp16
    terms (2.4e-7 relative), float32 statistics / exp / pooling: measured ~3e-7; asserted at 3e-6 on |z| <= ~1.  Empty boards
    (every token constant: z = ZALL / LALL), full-ish boards (every token dirty), a device-side count, and the result of a board
    independent of what else is in the batch (bit for bit)."""
    import azk
    net = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path="clsfold")
    assert net._exact is not None
    x = random_boards(70, 5, max_stones=100)
    x[0] = 0
    x = x.cuda()
    _, _, z_ref = net.forward_exact_emulated(x)
    z = azk.nnx_embed_pool(x, net._exact["tables"], 15, 15, net._sched_for(None))
    torch.cuda.synchronize()
    assert (z - z_ref).abs().max().item() < 3e-6, (z - z_ref).abs().max().item()
    zb = azk.nnx_embed_pool(x.to(torch.bfloat16), net._exact["tables"], 15, 15, net._sched_for(None))
    assert torch.equal(z, zb)
    cnt = torch.tensor([33], dtype=torch.int32, device="cuda")
    z2 = azk.nnx_embed_pool(x.flip(0).contiguous(), net._exact["tables"], 15, 15, net._sched_for(None), count=cnt)
    assert torch.equal(z2[:33], z.flip(0)[:33])
    assert int(net._sched_for(None)[0]) == 0              # the board queue is left zero


def test_embed_fold_exact_rows_against_float64():
    """k_embed_fold<EX> (azk_nnx_embed_fold: embedding + pooling from the patch bits, float32 rows) against the float64 evaluation of
    its formulas, entry by entry, and through the batched (hi, lo)-plane link against the float64 value-projected row.  Budget: the
    quadratic form and the score columns on two fp16 terms (2.4e-7 relative), float32 statistics / exp / sums: asserted at 3e-6 of
    the largest entry.  Engine-leaf variant: the same rows, bit for bit, handed out from the stone-heavy classes down.
    (tests/test_gpu_fold_pinned.py holds every entry to a derived bound of its own, on every board shape.)"""
    import azk
    net = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path="clsfold")
    ft = net._exact["foldu"]
    assert ft is not None and ft.exact
    T, H, ROW = CFG.tokens, CFG.num_heads, azk.EMBED_FOLD_ROW
    x = random_boards(600, 5, max_stones=100)
    x[0] = 0
    x = x.cuda()
    sched = net._sched_for(None)
    rows = azk.nnx_embed_fold(x, ft, 15, 15, sched)
    torch.cuda.synchronize()
    assert rows.dtype == torch.float32 and rows.shape == (600, H, ROW) and int(sched[0]) == 0
    u64, bw, inv_l, pw = net.forward_fold_u_emulated(x)
    got = rows.double()
    for a_, b_ in ((got[:, :, :T], bw), (got[:, :, T], inv_l), (got[:, :, 256:320], pw)):
        assert (a_ - b_).abs().max().item() < 3e-6 * b_.abs().max().item(), ((a_ - b_).abs().max().item(), b_.abs().max().item())
    assert bool((rows[:, :, T + 1:256] == 0).all()) and bool((rows[:, :, 320:] == 0).all()) and bool((rows[0, :, :T] == 0).all())
    u = (torch.empty(600, 512, dtype=torch.float16, device="cuda"), torch.empty(600, 512, dtype=torch.float16, device="cuda"))
    uf = torch.empty(600, 512, dtype=torch.float32, device="cuda")
    azk.nnx_gemm_h(rows.view(600, H * ROW), ft.weight, 64, ROW, azk.TAIL_BF16, nbatch=H, a_batch_stride=ROW, out=u, out_f32=uf)
    assert (uf.double() - u64).abs().max().item() < 3e-6 * u64.abs().max().item(), (uf.double() - u64).abs().max().item()
    assert torch.equal(azk.nnx_embed_fold(x.to(torch.bfloat16), ft, 15, 15, sched), rows)
    cnt = torch.tensor([33], dtype=torch.int32, device="cuda")
    r2 = azk.nnx_embed_fold(x.flip(0).contiguous(), ft, 15, 15, sched, count=cnt)
    assert torch.equal(r2[:33], rows.flip(0)[:33])


@pytest.mark.parametrize("tail", ["h16", "h16-conv"])
def test_exact_evaluator_against_reference_known_answers(tail):
    """The whole fp32-accurate evaluator against the reference's seed-0 outputs (nn_small.npz full_*): north_star's float32 bar,
    logits 1e-5 / value 1e-6 (measured ~1e-6 / 1e-7) - the tolerance the torch float32 paths are held to.  Both embedding forms
    in front of the fp16 (hi, lo)-plane tail."""
    z = load_golden("nn_small.npz")
    net = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path="clsfold")
    net.use_fold_u = tail == "h16"      # h16: k_embed_fold<EX>; h16-conv: k_embed_pool_x
    logits, v = net(torch.from_numpy(z["full_x"]).cuda())
    np.testing.assert_allclose(logits.cpu().numpy(), z["full_logits"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(v.cpu().numpy().reshape(-1), z["full_value"].reshape(-1), rtol=0, atol=1e-6)
    # and on 512 benchmark-like boards against the torch float32 full forward
    xb = random_boards(512, 9, max_stones=40).cuda()
    lf, vf = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path="full")(xb)
    le, ve = net(xb)
    assert (le - lf).abs().max().item() < 1e-5 and (ve.reshape(-1) - vf.reshape(-1)).abs().max().item() < 2e-6


def test_search_policies_identical_under_the_exact_evaluator():
    """800-simulation searches from all 92 recorded positions of the reference's 15x15 games, same Dirichlet noise: the
    hand-written fp32-accurate evaluator against the torch float32 'full' forward (the reference's own arithmetic):
    max |delta pi| <= 1e-5 on every position (north_star's bar; with 799 child visits that means not one visit moved)."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    from measure_nn_parity import golden_positions, search_pis
    positions = golden_positions()
    assert len(positions) == 92
    noise = torch.from_numpy(np.random.RandomState(7).dirichlet([0.03] * 225, size=len(positions))).cuda()
    ref_pi, ref_q = search_pis(PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path="full"), "float32", positions, 800, noise)
    for tail in ("h16", "h16-conv"):
        net = PolicyValueNet(CFG, seed=0, device="cuda", dtype=torch.float32, path="clsfold")
        net.use_fold_u = tail == "h16"  # h16: k_embed_fold<EX>; h16-conv: k_embed_pool_x
        pi, q = search_pis(net, "float32", positions, 800, noise)
        d = np.abs(pi - ref_pi)
        print(f"exact clsfold ({tail} tail) vs fp32 full: {(d.max(1) == 0).sum()}/{len(positions)} identical, max |dpi| {d.max():.2e}, max |dq| {np.abs(q - ref_q).max():.2e}")
        assert d.max() <= 1e-5, tail
        assert np.abs(q - ref_q).max() < 1e-5, tail


def test_runner_exact_evaluator_graph_stepping():
    """The exact evaluator inside the step graph (pending leaves straight from the engine, live count on the device) plays the same
    moves as eager stepping with n_leaf-sized batches; continuous self-play with recycling and the shared eval cache."""
    from selfplay import SelfPlayRunner
    net = PolicyValueNet(CFG, seed=6, device="cuda", dtype=torch.float32, path="clsfold")

    def play(graph):
        rec = []
        r = SelfPlayRunner("gomoku", net, 96, 64, size=15, seed=9, leaf_dtype="float32", recycle=True, use_graph=graph, cache_entries=256,
                           cache_shared=True, steps_per_graph=8,
                           on_records=lambda mv, base, pi, q, ch, w, d: rec.append((pi.numpy().copy(), ch.numpy().copy())))
        for _ in range(4):
            r.play_move()
        r.check_error()
        return rec
    a, b = play(True), play(False)
    for (pa, ca), (pb, cb) in zip(a, b):
        assert np.array_equal(ca, cb) and pa.tobytes() == pb.tobytes()


def test_weights_outside_the_fp16_plane_scales_fall_back_to_the_torch_forward():
    """The fp32-accurate tables carry weights as fp16 (hi, lo) terms at fixed scales (x 256 for the tail, x 4096 for the conv weight):
    trained weights beyond those ranges must not raise in the middle of a promotion (PolicyValueNet.load_state_dict -> to()) - the
    hand-written path steps aside (as for an uncovered configuration), the torch float32 forward answers, and the in-place
    promotion reports False so that the owner of a captured graph re-captures."""
    from pvnet import NetConfig, PolicyValueNet
    cfg = NetConfig(15, 15, 2, 225, 5, 512, 8, 1)
    net = PolicyValueNet(cfg, seed=0, device="cuda", dtype=torch.float32, path="clsfold")
    assert net._exact is not None
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    sd["blocks.0.mlp.3.weight"] *= 1.0e5                       # |w| x 256 no longer fits fp16
    big = PolicyValueNet(cfg, weights=sd, device="cuda", dtype=torch.float32, path="clsfold")
    assert big._exact is None
    x = (torch.rand(4, 2, 15, 15, device="cuda") < 0.1).float()
    ref = PolicyValueNet(cfg, weights=sd, device="cuda", dtype=torch.float32, path="full")
    lb, vb = big(x)
    lr, vr = ref(x)
    assert torch.isfinite(lb).all() and (lb - lr).abs().max().item() <= 1e-3 * max(1.0, lr.abs().max().item())
    assert net.load_state_dict(sd) is False and net._exact is None
    l2, _ = net(x)
    assert torch.equal(l2, lb)


def test_activation_beyond_the_fp16_planes_is_flagged():
    """The tail's links hand activations on as fp16 (hi, lo) planes of x * 16: an activation of magnitude >= 4094 becomes inf in the planes.
    Every link that writes or splits planes raises a sticky device flag, and PolicyValueNet.check_exact_range() turns it into an error."""
    import azk
    from pvnet import NetConfig, PolicyValueNet
    D, m = 512, 64
    hh = torch.randn(m, 4 * D, device="cuda") * 0.4
    w3 = torch.randn(D, 4 * D, device="cuda") * 0.03
    wp3, _ = azk.pack_linear_weight_h(w3)
    xr = torch.randn(m, D, device="cuda")
    hi, lo = azk.split_fp16(hh.double(), azk.GEMM_H_A_SCALE)
    for lds in (False, True):
        for big in (False, True):
            flag = torch.zeros(1, dtype=torch.int32, device="cuda")
            r = xr.clone()
            if big:
                r[3, 7] = 5000.0                                   # the residual pushes one output past 4094
            oh, ol = torch.empty(m, D, device="cuda", dtype=torch.float16), torch.empty(m, D, device="cuda", dtype=torch.float16)
            azk.nnx_gemm_h((hi.contiguous(), lo.contiguous()), wp3, D, 4 * D, azk.TAIL_RESID, bias=torch.zeros(D, device="cuda"), resid=r, out=(oh, ol), lds=lds, overflow=flag)
            torch.cuda.synchronize()
            assert int(flag.item()) == (1 if big else 0), (lds, big)
    cfg = NetConfig(15, 15, 2, 225, 5, 512, 8, 1)
    net = PolicyValueNet(cfg, seed=0, device="cuda", dtype=torch.float32, path="clsfold")
    x = (torch.rand(4, 2, 15, 15, device="cuda") < 0.1).float()
    net(x)
    net.check_exact_range()                                        # a sane network: nothing flagged
    net._exact_overflow.fill_(1)
    with pytest.raises(FloatingPointError):
        net.check_exact_range()
