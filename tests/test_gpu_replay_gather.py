"""azk_replay_gather on the GPU (include/azk.h): a batch gathered from a replay ring, each row turned by the element drawn
for it - against torch's own gathers without draws, against the numpy restatement (tests/emission_restated.py) with them; then
DeviceReplay.sample(augment=...) and train.train(augment=...) end to end.  Needs no engine; every comparison is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

import emission_restated as er

pytestmark = pytest.mark.gpu

# (planes, rows, cols, action_dim, the elements "board" means, the restatement's action kind)
GEOMS = {"7x7": (2, 7, 7, 49, tuple(range(8)), "gomoku"), "5x7": (2, 5, 7, 35, (0, 1, 2, 6), "gomoku"), "connect4": (3, 6, 7, 7, (0, 1), "connect4"),
         "20x20": (2, 20, 20, 400, tuple(range(8)), "gomoku"), "1x3": (2, 1, 3, 3, (0, 1, 2, 6), "gomoku"),
         # wider than the engine's 30 columns, where a 16-bit reciprocal of cols no longer splits a cell into row and column: 256 * ceil(65536 / 257)
         # = 65536 puts cell 256 of 1x257 into row 1, cell 389 of 2x195 into row 2 - the gather divides
         "1x257": (2, 1, 257, 257, (0, 1, 2, 6), "gomoku"), "2x195": (2, 2, 195, 390, (0, 1, 2, 6), "gomoku"), "1x400": (2, 1, 400, 400, (0, 1, 2, 6), "gomoku")}
N, RING = 37, 23


def filled_ring(name, capacity=RING):
    import azk
    planes, rows, cols, A, _, _ = GEOMS[name]
    gen = torch.Generator().manual_seed(1234 + rows * 31 + cols)
    rp = azk.DeviceReplay(capacity, planes, rows, cols, A)
    states = (torch.rand((capacity, planes, rows, cols), generator=gen) < 0.4).to(torch.float32)
    rp.states.copy_(states)
    rp.pis.copy_(torch.rand((capacity, A), generator=gen, dtype=torch.float64))
    rp.zs.copy_(torch.randint(-1, 2, (capacity,), generator=gen).to(torch.float32))
    rp.cursor.fill_(capacity)
    return rp


def batch_index(dev):
    idx = torch.arange(N, dtype=torch.int64) * 7 % RING               # repeats (37 > 23) ...
    idx[5], idx[N - 1] = RING - 1, RING - 1                            # ... and the last ring row, twice
    return idx.to(dev)


def mask_of(elements):
    return sum(1 << s for s in elements)


@pytest.mark.parametrize("name", list(GEOMS))
def test_without_draws_it_is_torchs_gather(name):
    rp = filled_ring(name)
    idx = batch_index(rp.states.device)
    for mask in (1, mask_of(GEOMS[name][4])):
        s, p, z = rp.gather(idx, None, mask)
        assert s.dtype == p.dtype == z.dtype == torch.float32
        assert torch.equal(s, rp.states[idx]) and torch.equal(p, rp.pis[idx].float()) and torch.equal(z, rp.zs[idx])


@pytest.mark.parametrize("name", list(GEOMS))
def test_with_draws_it_is_the_restated_pick_and_turn(name):
    planes, rows, cols, A, elements, kind = GEOMS[name]
    rp = filled_ring(name)
    idx = batch_index(rp.states.device)
    highs = [0, 1, 0x7FFF, 0x8000, 0xFFFF, 0x1FFF, 0x2000, 0x3FFF, 0x4000, 0x5FFF, 0x6000, 0x9FFF, 0xA000, 0xBFFF, 0xC000, 0xDFFF, 0xE000]
    rng = np.random.RandomState(7)
    u = [(h << 16) | int(rng.randint(0, 1 << 16)) for h in highs] + [int(x) for x in rng.randint(0, 1 << 32, size=N - len(highs), dtype=np.uint64)]
    draws_h = np.array(u, np.uint32).view(np.int32)                    # the full int32 range, negative values among them
    assert len(draws_h) == N and (draws_h < 0).any()
    draws = torch.from_numpy(draws_h.copy()).to(rp.states.device)
    states, pis, zs = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    if name in ("1x257", "2x195"):
        idx[:] = RING - 1                                               # every row from the LAST ring row: a source index past the row leaves the ring
    for els in {elements, (0,), elements[:2]}:
        s, p, z = rp.gather(idx, draws, mask_of(els))
        ws, wp, wz, picked = er.gather_rows(states, pis, zs, idx.cpu().numpy(), draws_h, els, kind)
        assert np.array_equal(s.cpu().numpy(), ws) and np.array_equal(p.cpu().numpy(), wp) and np.array_equal(z.cpu().numpy(), wz)
        assert set(picked) == set(els)                                  # every element of the mask was drawn (the fixed high halves see to it)


def test_zero_rows_touch_nothing_and_bad_arguments_are_refused():
    import azk
    from azk import _p
    rp = filled_ring("5x7")
    L, dev = azk.lib(), rp.states.device
    idx = batch_index(dev)
    s = torch.full((N, 2, 5, 7), -5.0, device=dev)
    p = torch.full((N, 35), -3.0, device=dev)
    z = torch.full((N,), 7.0, device=dev)

    def call(rows, cols, A, mask, n):
        return L.azk_replay_gather(rows, cols, 2, A, mask, _p(rp.states), _p(rp.pis), _p(rp.zs), _p(idx), None, n, _p(s), _p(p), _p(z),
                                   C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert call(5, 7, 35, 0x47, 0) == 0
    torch.cuda.synchronize()
    assert torch.all(s == -5.0) and torch.all(p == -3.0) and torch.all(z == 7.0)
    ARG = -1                                                            # AZK_ERR_ARG
    assert call(5, 7, 35, 0x46, N) == ARG and b"bit 0" in L.azk_last_error(None)                  # no identity
    assert call(5, 7, 35, 0x09, N) == ARG and b"does not admit" in L.azk_last_error(None)         # rot90 on a rectangle
    assert call(5, 7, 35, 0x101, N) == ARG                                                        # a bit above 7
    assert call(21, 20, 420, 0x01, N) == ARG and b"400" in L.azk_last_error(None)
    assert call(5, 7, 35, 0x47, -1) == ARG
    assert call(5, 7, 7, 0x05, N) == ARG and call(5, 7, 11, 0x03, N) == ARG                      # column actions: {0, 1}; any other kind: {0}
    torch.cuda.synchronize()
    assert torch.all(s == -5.0) and torch.all(p == -3.0) and torch.all(z == 7.0)
    with pytest.raises(azk.AzkError):
        rp.gather(idx, None, 0x09)
    assert call(5, 7, 35, 0x47, N) == 0                                 # ... and the same buffers do get written by a good call
    torch.cuda.synchronize()
    assert torch.equal(s, rp.states[idx]) and torch.equal(z, rp.zs[idx])


@pytest.mark.parametrize("name", ["7x7", "5x7", "connect4"])
def test_sample_augment_returns_images_of_ring_rows(name):
    planes, rows, cols, A, elements, kind = GEOMS[name]
    rp = filled_ring(name, capacity=64)
    states, pis, zs = rp.states.cpu().numpy(), rp.pis.cpu().numpy(), rp.zs.cpu().numpy()
    assert len({states[r].tobytes() for r in range(64)}) == 64          # pairwise distinct rows
    images = {}                                                        # state bytes -> [(pi float32 bytes, z)] over every row and admitted element
    for r in range(64):
        for e in elements:
            st, pi = er.turn(states[r], pis[r], e, kind)
            images.setdefault(st.tobytes(), []).append((pi.astype(np.float32).tobytes(), float(zs[r])))
    torch.manual_seed(3)
    seen = set()
    for augment in ("board", elements):
        s, p, z = rp.sample(16, augment=augment)
        assert s.shape == (16, planes, rows, cols) and p.shape == (16, A) and z.shape == (16, 1) and p.dtype == torch.float32
        for b in range(16):
            key = s[b].cpu().numpy().tobytes()
            assert key in images                                       # the image of one ring row under one admitted element ...
            assert (p[b].cpu().numpy().tobytes(), float(z[b])) in images[key]      # ... with pi under the same element, and the row's z
            seen.add(key)
    assert len(seen) > 16                                              # not the same sixteen rows twice over
    s0, p0, z0 = rp.sample(16)                                          # augment=None: today's result types
    assert z0.shape == (16, 1) and p0.dtype == torch.float32
    with pytest.raises(ValueError):
        rp.sample(16, augment="all")


def test_connect4_collect_then_train_with_sample_time_augmentation():
    import azk
    import train
    from fixture_eval import FixtureModel
    from games import Connect4
    from pvnet import NetConfig, PolicyValueNet
    buffer = azk.DeviceReplay(8 * 42, 3, 6, 7, 7)
    results = train.collect_data(Connect4, FixtureModel(7), buffer, 8, 16, seed=4, emit_symmetry="none")
    assert sum(results) == 8 and 8 * 7 <= buffer.size() == int(buffer.cursor.item()) <= 8 * 42      # one tuple per ply
    host = []

    class Host:
        add = staticmethod(lambda s, p, t: host.append((np.array(s, np.float32), np.array(p, np.float64), float(t[0]))))
    train.collect_data(Connect4, FixtureModel(7), Host, 8, 16, seed=4, emit_symmetry="none")       # the host route: the same tuples
    dq = buffer.to_reference_deque()
    assert sorted(er.tuple_sha(s, p, z[0]) for s, p, z in dq) == sorted(er.tuple_sha(*t) for t in host)
    cfg = NetConfig(6, 7, 3, 7, patch_size=5, embed_dim=128, num_heads=4, depth=1)
    model = PolicyValueNet(cfg, seed=0, device="cuda")
    before = model.state_dict()
    losses = train.train(model, 32, buffer, 2, 1e-3, "cuda", augment="board")
    assert len(losses) == 4 and all(np.isfinite(float(x)) for x in losses)
    after = model.state_dict()
    assert any(not torch.equal(before[k], after[k]) for k in before)
