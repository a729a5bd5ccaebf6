"""Weight packers: nn.Linear weights in the MFMA fragment orders the GEMM kernels read, and the fp16 (hi, lo) split of the
fp32-accurate path."""
from ._rt import _torch


def pack_linear_weight(w):
    """nn.Linear weight [n_out, k] (any float dtype, any device) -> bf16 tensor in the MFMA B-fragment order of include/azk.h's cls-row tail section
    (n_out padded with zero rows to a multiple of 64; k must be a multiple of 32)."""
    torch = _torch()
    n_out, k = w.shape
    assert k % 32 == 0
    npad = (n_out + 63) // 64 * 64
    wp = torch.zeros(npad, k, dtype=torch.float32, device=w.device)
    wp[:n_out] = w.float()
    # [g, l15, c, s, l4, i] -> [g, s, c, l4, l15, i]
    return wp.view(npad // 64, 16, 4, k // 32, 4, 8).permute(0, 3, 2, 4, 1, 5).contiguous().to(torch.bfloat16)


def pack_linear_weight128(w):
    """pack_linear_weight with the output dimension padded (zero rows) to a multiple of 128: the operand of nn_gemm_tok."""
    torch = _torch()
    n_out, k = w.shape
    npad = (n_out + 127) // 128 * 128
    wp = torch.zeros(npad, k, dtype=torch.float32, device=w.device)
    wp[:n_out] = w.float()
    return pack_linear_weight(wp)


def packed_weight_col_sums(w_packed, n_out, k):
    """Column sums sum_k W[j][k] of a pack_linear_weight() tensor's bf16 values (float64 sum, rounded once): the
    a_col_sums operand of azk_nn_tail_gemm_lds (LayerNorm applied in the epilogue)."""
    torch = _torch()
    npad = (n_out + 63) // 64 * 64
    # [g, s, c, l4, l15, i] -> [g, l15, c, s, l4, i]: column 64 g + 4 l15 + c, k = 32 s + 8 l4 + i
    w = w_packed.view(npad // 64, k // 32, 4, 4, 16, 8).permute(0, 4, 2, 1, 3, 5).reshape(npad, k)
    return w.double().sum(1).float().contiguous()


def split_fp16(x64, scale):
    """float64 tensor -> (hi, lo) fp16 tensors with (hi + lo) / scale = x to 22 significant bits (two round-to-nearest steps)."""
    torch = _torch()
    xs = x64.double() * float(scale)
    hi = xs.to(torch.float16)
    lo = (xs - hi.double()).to(torch.float16)
    return hi, lo


GEMM_H_A_SCALE, GEMM_H_W_SCALE = 16.0, 256.0      # activations x 16, weights x 256 before the fp16 (hi, lo) split (azk_nnx_gemm_h)


def pack_linear_weight_h(w):
    """nn.Linear weight [n_out, k] (float64 / float32) -> (fp16 planes in azk_nnx_gemm_h's fragment order
    [n_out/64][k/32][4][2][64][8], float32 col_sums [n_out padded] = sum_k of the RECONSTRUCTED weights)."""
    torch = _torch()
    n_out, k = w.shape
    assert k % 32 == 0
    npad = (n_out + 63) // 64 * 64
    wp = torch.zeros(npad, k, dtype=torch.float64, device=w.device)
    wp[:n_out] = w.double()
    assert float(wp.abs().max()) * GEMM_H_W_SCALE < 60000.0
    hi, lo = split_fp16(wp, GEMM_H_W_SCALE)
    # [g, l15, c, s, l4, i] -> [g, s, c, plane, l4, l15, i]
    f = lambda t: t.view(npad // 64, 16, 4, k // 32, 4, 8).permute(0, 3, 2, 4, 1, 5)
    packed = torch.stack([f(hi), f(lo)], dim=3).contiguous()
    csum = ((hi.double() + lo.double()) / GEMM_H_W_SCALE).sum(1).float().contiguous()
    return packed, csum
