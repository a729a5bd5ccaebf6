"""tests/fold_restated.py checked on the CPU: the plain-loop patch layout against F.unfold and against the kernel's own route to the
bits, the float64 evaluation against pvnet's (at every shape of SHAPES, where tests/test_pvnet.py has 15 x 15 only), every exact probe's
closed form against the float64 evaluation of its tables, a numpy float32 restatement against `bound`, and six deliberate mistakes,
each of which some probe or the bound must notice.  tests/test_gpu_fold_pinned.py holds the kernel to the same probes and bound."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fold_restated as fr

SHAPE_IDS = ["x".join(map(str, s)) for s in fr.SHAPES]
shapes = pytest.mark.parametrize("shape", list(fr.SHAPES), ids=SHAPE_IDS)


@pytest.fixture(autouse=True, scope="module")
def release_networks():
    """The sixteen seed-6 networks are shared by the tests of this file and dropped with the last of them."""
    yield
    fr.real_tables.cache_clear()


def _few(shape, n=5):
    return np.stack(fr.fixed_boards(shape) + fr.stone_boards(shape, 3, n))


def _thin(boards, most=120):
    """Every board of a small set, an even pick (with the last board) of a large one: the closed form is one function of the board."""
    step = -(-len(boards) // most)
    return boards if step == 1 else np.concatenate([boards[::step], boards[-1:]])


@shapes
def test_patch_layout(shape):
    """The plain loops give F.unfold's patches, token 0 empty; the kernel's route (row words, one shift, the row mask) gives the same."""
    R, Cc, C, k = shape
    b = _few(shape)
    P = fr.patch_bits(b, k)
    cols = F.unfold(torch.from_numpy(b).double(), kernel_size=k, padding=k // 2).transpose(1, 2).numpy()
    assert P.shape == (len(b), R * Cc + 1, 64) and not P[:, 0].any() and not P[:, :, C * k * k:].any()
    assert np.array_equal(P[:, 1:, :C * k * k], cols)
    for i in (1, 2, 3, 4):
        assert np.array_equal(fr.front_emulate(b[i], k), P[i]), i


@shapes
def test_float64_evaluation(shape):
    """fold_f64 at eps = 1e-5 is forward_fold_u_emulated (which evaluates the unreached tokens too: their weight is zero to rounding), and
    its row against [D_t; U_all; M_h] is the plain pooled forward's value-projected row within the 2e-7 of test_pvnet.py."""
    R, Cc, C, k = shape
    net, r = fr.real_tables(shape)
    x = torch.from_numpy(_few(shape))
    o = fr.fold_f64(r, fr.patch_bits(x.numpy(), k), 1e-5)
    u, bw, inv, pw = net.forward_fold_u_emulated(x, r)
    for name, mine, theirs in (("bw", o["bw"], bw), ("inv", o["inv"], inv), ("pw", o["pw"], pw)):
        assert (mine - theirs).abs().max().item() <= 1e-12 * theirs.abs().max().item(), name
    T, dh = R * Cc + 1, 64
    mine = (torch.einsum("nht,thj->nhj", o["bw"], r["Dtab"].view(T, fr.H, dh)) + r["uall"].view(1, fr.H, dh) * o["inv"][..., None]
            + torch.einsum("nhk,hjk->nhj", o["pw"], r["M"].view(fr.H, dh, 64))).reshape(len(x), 512)
    rx = net.exact_fold("cpu")
    _, _, z = net.forward_exact_emulated(x, rx)
    u_ref = torch.einsum("nhd,hed->nhe", z.double(), rx["Wvn"].double()).reshape(len(x), 512)
    assert (mine - u_ref).abs().max().item() < 2e-7 * u_ref.abs().max().item() + 1e-7


@shapes
@pytest.mark.parametrize("kind", fr.KINDS)
def test_probe_expectations(kind, shape):
    """The float64 evaluation of the probe tables at eps = 0 gives the closed form exactly (count2: a quotient, to 2^-50), every value is a
    float32 number with at most 12 significant bits times a power of two, and the window of allowed outputs is a single value wherever
    the closed form is a bf16 number: everywhere but the 1 / L remainder slot, count2's quotients and the selection probe's sums over
    a set side plane.  The float32 restatement of the kernel lands inside every window."""
    R, Cc, C, k = shape
    T = fr.tokens(shape)
    b = _thin(fr.probe_boards(kind, shape))
    e = fr.probe_expected(kind, shape, b)
    r = fr.probe_tables(kind, shape)
    P = fr.patch_bits(b, k)
    o = fr.fold_f64(r, P, 0.0)
    for key in ("bw", "inv", "pw"):
        got, want = o[key].numpy(), e[key]
        if kind == "count2":
            assert np.abs(got - want).max() <= 2.0 ** -50 * np.abs(want).max(), key
            continue
        assert np.array_equal(got, want), key
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want), key
        m, _ = np.frexp(want)
        assert np.array_equal(m * 4096, np.round(m * 4096)), key                # (sums of 2^j over at most 252 tokens: < 2^11 units)
        if kind != "selection" or C == 2:
            if key != "pw" or kind != "count":
                assert np.isin(m, (0.0, 0.5)).all(), key                         # a power of two, or zero
            else:
                assert (want * 2.0 ** np.arange(fr.H)[None, :, None] <= 252).all()   # an integer of at most 252 over 2^h
    for form in fr.FORMS:
        lo, hi = fr.probe_window(kind, shape, e, form)
        one = lo == hi
        if form == "f32":
            assert one.all()
        elif kind != "count2":
            one[:, :, T + 1] = True
            if kind == "selection" and C == 3:
                one[:, :, 256 + 2 * k * k:256 + 3 * k * k] = True               # the side plane's bits: sums over many tokens
            assert one.all(), (kind, form)
        rows = fr.fold_f32(r, P, 0.0, form)
        assert len(fr.in_window(rows, lo, hi)) == 0, (kind, form)
        if form == "bf16":
            assert (np.abs(rows[:, :, T] + rows[:, :, T + 1] - e["inv"]) <= fr.inv_sum_bound(e["inv"])).all()


@shapes
@pytest.mark.parametrize("form", fr.FORMS)
def test_float32_restatement_within_the_bound(shape, form):
    """A numpy float32 evaluation from the fp16 hi + lo tables, rounded once, stays within `bound` of float64 at every entry."""
    R, Cc, C, k = shape
    _, r = fr.real_tables(shape)
    b = _thin(fr.bound_boards(shape, random=6), most=16)
    o = fr.fold_f64(r, fr.patch_bits(b, k), 1e-5)
    bd = fr.bound(r, o, 1e-5, form)
    worst = fr.check_rows(fr.fold_f32(r, o["P"], 1e-5, form), o, bd, fr.tokens(shape), form)
    print(f"RATIO f32_restated_{'x'.join(map(str, shape))}_{form} {worst:.4f}")
    assert worst <= 1.0, worst


def _probe_rows(kind, shape, form, boards, front=None, f32=None):
    """The float32 restatement's rows of a probe, with the front end's or the arithmetic's mistake, and the probe's window."""
    k = shape[3]
    e = fr.probe_expected(kind, shape, boards)
    P = fr.patch_bits(boards, k) if front is None else np.stack([fr.front_emulate(x, k, front) for x in boards])
    rows = fr.fold_f32(fr.probe_tables(kind, shape), P, 0.0, form, mutate=f32)
    return len(fr.in_window(rows, *fr.probe_window(kind, shape, e, form)))


@pytest.mark.parametrize("form", fr.FORMS)
def test_front_end_mistakes_are_noticed_by_the_selection_probe(form):
    """rows / cols swapped in the token coordinate and the row mask tested against cols: the selection probe at 6 x 7 notices both, and at
    7 x 7 neither can be seen (why the shapes with rows != cols are there).  The column shift off by one: noticed at any shape."""
    sq, c4 = (7, 7, 2, 3), (6, 7, 3, 3)
    bsq, bc4 = fr.probe_boards("selection", sq)[::3], fr.probe_boards("selection", c4)[::3]
    assert _probe_rows("selection", c4, form, bc4) == 0 and _probe_rows("selection", sq, form, bsq) == 0
    for m in ("swap_rc", "rowmask_cols"):
        assert _probe_rows("selection", c4, form, bc4, front=m) > 0, m
        assert _probe_rows("selection", sq, form, bsq, front=m) == 0, m
    assert _probe_rows("selection", c4, form, bc4, front="shift1") > 0 and _probe_rows("selection", sq, form, bsq, front="shift1") > 0
    for shape in ((1, 2, 2, 5), (2, 2, 2, 5)):
        b = fr.probe_boards("selection", shape)
        assert _probe_rows("selection", shape, form, b, front="shift1") > 0, shape


@pytest.mark.parametrize("form", fr.FORMS)
def test_a_dropped_wave_is_noticed_by_the_count_probes(form):
    """Wave 3's share of L left out: count2 (L counts the reached tokens) notices on every board with a fourth tile, and the full 7 x 7
    board's 49 reached tokens leave one in the fourth tile: 1 / L is 2 / 49 in place of 2 / 50."""
    shape = (7, 7, 2, 3)
    b = fr.probe_boards("count2", shape)
    assert _probe_rows("count2", shape, form, b) == 0
    assert _probe_rows("count2", shape, form, b, f32="drop_wave_L") > 0
    full = b[1:2]
    rows = fr.fold_f32(fr.probe_tables("count2", shape), fr.patch_bits(full, 3), 0.0, form, mutate="drop_wave_L")
    assert abs(rows[0, 0, 50] - 2.0 / 49) < 1e-4


def test_a_dropped_lo_term_is_noticed_by_the_float32_rows_bound():
    """G and ext as their fp16 hi terms alone (2^-11 of every entry): the float32 rows leave the bound on the one-stone boards, where the
    sums are short and the bound sharp.  The bf16 rows' own rounding (2^-8) hides it: the EX form is what pins the lo fragments."""
    shape = (6, 7, 3, 3)
    _, r = fr.real_tables(shape)
    b = np.stack(fr._one_stone(shape, (0, 1))[::3])
    o = fr.fold_f64(r, fr.patch_bits(b, 3), 1e-5)
    bd = fr.bound(r, o, 1e-5, "f32")
    good = fr.check_rows(fr.fold_f32(r, o["P"], 1e-5, "f32"), o, bd, 43, "f32")
    bad = fr.check_rows(fr.fold_f32(r, o["P"], 1e-5, "f32", mutate="drop_lo"), o, bd, 43, "f32")
    print(f"RATIO drop_lo good {good:.4f} bad {bad:.4f}")
    assert good <= 1.0 < bad


def test_a_wrong_plane_pick_is_noticed_by_the_leaf_boards_check():
    """The third plane taken from the cell codes: differs from the side to move on every position with a stone, for either mover (what
    test_leaf_entry_point_on_connect4 compares the gathered boards with)."""
    cells = np.array([0, 1, 2, 0, 1, 2, 0])
    for player in (0, 1):
        good, bad = fr.canonical_planes(cells, player, 3), fr.canonical_planes(cells, player, 3, mutate="plane_pick")
        assert np.array_equal(good[2], np.full(7, float(player))) and np.array_equal(good[:2], bad[:2]) and not np.array_equal(good[2], bad[2])
        assert np.array_equal(good[0], (cells == 1 + player).astype(float)) and np.array_equal(good[1], (cells == 2 - player).astype(float))
