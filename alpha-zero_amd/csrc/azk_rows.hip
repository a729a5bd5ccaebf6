// azk_rows.hip - the row kernels of the cls-row tail in its library form (`--tail library`) and of the full-token blocks: LayerNorm
// over bf16 rows (k_ln_rows), the fused final LayerNorm + heads (k_ln_heads) and the heads' float32 read-out (k_heads_finalize).
// The chain form of the tail is azk_nn.hip k_tail_gemm / azk_tail.hip k_tail_lds.
#include <hip/hip_runtime.h>
#include <hip/hip_bf16.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <type_traits>

#include "azk.h"
#include "azk_launch.h"
#include "azk_nn_common.h"

// =====================================================================================================
// k_heads_finalize: the merged policy/value head GEMM output [n][ld] (bf16; columns [0, A) logits, column A the raw
// value) -> logits float32 [n][A] and values float32 [n] = tanh(raw) (nn.py:82-83), one launch instead of three.
// =====================================================================================================
namespace {
using namespace azk_nn;
__global__ void k_heads_finalize(const unsigned short *__restrict__ out, int ld, int A, int n, float *__restrict__ logits,
                                 float *__restrict__ values, const int *count) {
    const int nvalid = count ? min(n, *count) : n;
    const long long total = (long long)nvalid * (A + 1);
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int row = (int)(i / (A + 1)), col = (int)(i - (long long)row * (A + 1));
        const float v = __uint_as_float((unsigned)out[(size_t)row * ld + col] << 16);
        if (col < A) logits[(size_t)row * A + col] = v;
        else values[row] = tanhf(v);
    }
}
}  // namespace

extern "C" int32_t azk_nn_heads_finalize(const void *heads_bf16_dev, int32_t ld, int32_t action_dim, int32_t n,
                                         float *logits_out_dev, float *values_out_dev, const int32_t *n_valid_dev,
                                         void *stream) {
    if (!heads_bf16_dev || !logits_out_dev || !values_out_dev || ld < action_dim + 1 || n < 0) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    k_heads_finalize<<<1024, 256, 0, (hipStream_t)stream>>>((const unsigned short *)heads_bf16_dev, ld, action_dim, n, logits_out_dev,
                                                           values_out_dev, n_valid_dev);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

// =====================================================================================================
// k_ln_rows: LayerNorm over the rows of a bf16 matrix [n][D] (nn.LayerNorm: biased variance, eps inside the sqrt,
// fp32 statistics), one wave per row, 16-byte loads/stores; optionally also writes x + add_bias back in place (the
// residual operand of the following GEMM, nn.py:59-60: the mlp.3 bias joins the residual before the product is added).
// =====================================================================================================
namespace {
__device__ __forceinline__ float wave64_sum(float v) {
    v = row16_sum(v);
    v += __shfl_xor(v, 16);
    v += __shfl_xor(v, 32);
    return v;
}

template <int VPL>   // values per lane: D = 64 * VPL
__global__ __launch_bounds__(256) void k_ln_rows(unsigned short *__restrict__ x, const float *__restrict__ w, const float *__restrict__ b,
                                                 float eps, unsigned short *__restrict__ y, const float *__restrict__ add_bias, int n,
                                                 const int *count) {
    constexpr int D = 64 * VPL;
    const int nvalid = count ? min(n, *count) : n;
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= nvalid) return;
    unsigned short *xr = x + (size_t)row * D + lane * VPL;
    float v[VPL];
    if constexpr (VPL == 8) {
        const uint4 raw = *(const uint4 *)xr;
        const unsigned u[4] = {raw.x, raw.y, raw.z, raw.w};
#pragma unroll
        for (int q = 0; q < 4; q++) { v[2 * q] = __uint_as_float(u[q] << 16); v[2 * q + 1] = __uint_as_float(u[q] & 0xffff0000u); }
    } else {
#pragma unroll
        for (int q = 0; q < VPL; q++) v[q] = __uint_as_float((unsigned)xr[q] << 16);
    }
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < VPL; q++) s += v[q];
    const float mean = wave64_sum(s) * (1.0f / D);
    float ss = 0.f;
#pragma unroll
    for (int q = 0; q < VPL; q++) { const float d = v[q] - mean; ss += d * d; }
    const float rstd = rsqrtf(wave64_sum(ss) * (1.0f / D) + eps);
    float o[VPL], r[VPL];
#pragma unroll
    for (int q = 0; q < VPL; q++) {
        o[q] = (v[q] - mean) * rstd * w[lane * VPL + q] + b[lane * VPL + q];
        if (add_bias) r[q] = v[q] + add_bias[lane * VPL + q];
    }
    unsigned short *yr = y + (size_t)row * D + lane * VPL;
    if constexpr (VPL == 8) {
        *(uint4 *)yr = pack8(o);
        if (add_bias) *(uint4 *)xr = pack8(r);
    } else {
#pragma unroll
        for (int q = 0; q < VPL; q++) {
            yr[q] = __builtin_bit_cast(unsigned short, (__bf16)o[q]);
            if (add_bias) xr[q] = __builtin_bit_cast(unsigned short, (__bf16)r[q]);
        }
    }
}
}  // namespace

extern "C" int32_t azk_nn_layernorm_rows(void *x_bf16_dev, const float *w_dev, const float *b_dev, float eps, void *y_bf16_dev,
                                         const float *add_bias_dev, int32_t n, int32_t embed_dim, const int32_t *n_valid_dev,
                                         void *stream) {
    if (!x_bf16_dev || !w_dev || !b_dev || !y_bf16_dev || n < 0) return AZK_ERR_ARG;
    if (embed_dim != 128 && embed_dim != 256 && embed_dim != 512) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((n + 3) / 4), block(256);
    unsigned short *x = (unsigned short *)x_bf16_dev, *y = (unsigned short *)y_bf16_dev;
    if (embed_dim == 512) k_ln_rows<8><<<grid, block, 0, st>>>(x, w_dev, b_dev, eps, y, add_bias_dev, n, n_valid_dev);
    else if (embed_dim == 256) k_ln_rows<4><<<grid, block, 0, st>>>(x, w_dev, b_dev, eps, y, add_bias_dev, n, n_valid_dev);
    else k_ln_rows<2><<<grid, block, 0, st>>>(x, w_dev, b_dev, eps, y, add_bias_dev, n, n_valid_dev);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

// =====================================================================================================
// k_ln_heads: final LayerNorm + merged heads of the cls row (nn.py:78-83), logits float32 and tanh(value) in one launch.  The weight
// comes packed in MFMA B-fragment order (azk.pack_linear_weight: Wp[N/64][K/32][4][64 lanes][8] with element =
// W[64 g + 4 (lane&15) + c][32 s + 8 (lane>>4) + i], one 16-byte load per fragment; a lane's four accumulators of a row are four
// consecutive output columns).  Rows at or beyond *n_valid are never touched.
// =====================================================================================================
namespace {

// The argument block keeps the byte layout it had when the split-K row GEMM shared it: k_ln_heads' kernel-argument offsets, and with
// them its instruction stream, stay exactly what tools/compare_kernel_isa.py has on record.  The pad fields are never read.
struct GemmArgs {
    const unsigned short *A;   // [M][lda] bf16
    int lda;
    const uint4 *Wp;           // packed weight
    int M, N, pad0[2];
    const int *count;
    const void *pad1;
    const float *bias;         // [N]
    const void *pad2[3];
    float ln_eps;
    float *logits, *values;    // float32 [M][action_dim], [M] = tanh(column action_dim)
    int action_dim;
};

// Final LayerNorm + merged heads for embed_dim = 32 KT, LayerNorm's affine folded into the weight (W diag(gamma)) and the bias
// (W beta + b) by the caller: one wave = 16 rows x 64 output columns; the wave's 16 x K slab of x is fetched ONCE (KT loads in
// flight together with the first weight fragments), the row statistics come from those registers, the normalised fragments
// feed the MFMAs - three to four dependent memory round trips per wave instead of eight.
template <int KT>
__global__ __launch_bounds__(256) void k_ln_heads(GemmArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int nvalid = a.count ? min(a.M, *a.count) : a.M;
    const int rtiles = (nvalid + 15) >> 4, ngroups = a.N >> 6;
    const int nitems = rtiles * ngroups;
    constexpr int K = 32 * KT;
    for (int item = blockIdx.x * 4 + wave; item < nitems; item += gridDim.x * 4) {
        const int ng = item % ngroups, rt = item / ngroups;
        const int row = min(16 * rt + l15, nvalid - 1);
        const unsigned short *ap = a.A + (size_t)row * a.lda + 8 * l4;
        const uint4 *bp = a.Wp + (size_t)ng * KT * 4 * 64 + lane;
        uint4 raw[KT];
#pragma unroll
        for (int ks = 0; ks < KT; ks++) raw[ks] = *(const uint4 *)(ap + 32 * ks);
        union BF { uint4 u; bf16x8 v; };
        BF bf[4][4];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int c = 0; c < 4; c++) bf[u][c].u = bp[(u * 4 + c) * 64];
        __builtin_amdgcn_sched_barrier(0);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int ks = 0; ks < KT; ks++) {
            const unsigned w4[4] = {raw[ks].x, raw[ks].y, raw[ks].z, raw[ks].w};
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const float lo = __uint_as_float(w4[q] << 16), hi = __uint_as_float(w4[q] & 0xffff0000u);
                s1 += lo + hi; s2 += lo * lo + hi * hi;
            }
        }
        s1 += __shfl_xor(s1, 16); s1 += __shfl_xor(s1, 32);
        s2 += __shfl_xor(s2, 16); s2 += __shfl_xor(s2, 32);
        const float mean = s1 * (1.0f / K);
        const float rstd = rsqrtf(fmaxf(s2 * (1.0f / K) - mean * mean, 0.f) + a.ln_eps);
        const float shift = -mean * rstd;
        f32x4 acc[4];
#pragma unroll
        for (int c = 0; c < 4; c++) acc[c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kb = 0; kb < KT; kb += 4) {
            BF nb[4][4];
            if (kb + 4 < KT) {
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int c = 0; c < 4; c++) nb[u][c].u = bp[((kb + 4 + u) * 4 + c) * 64];
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint4 r = raw[kb + u];
                const unsigned w4[4] = {r.x, r.y, r.z, r.w};
                float v[8];
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    v[2 * q] = __uint_as_float(w4[q] << 16) * rstd + shift;
                    v[2 * q + 1] = __uint_as_float(w4[q] & 0xffff0000u) * rstd + shift;
                }
                BF af;
                af.u = pack8(v);
#pragma unroll
                for (int c = 0; c < 4; c++) acc[c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af.v, bf[u][c].v, acc[c], 0, 0, 0);
            }
            if (kb + 4 < KT) {
#pragma unroll
                for (int u = 0; u < 4; u++)
#pragma unroll
                    for (int c = 0; c < 4; c++) bf[u][c] = nb[u][c];
            }
        }
        const int col0 = 64 * ng + 4 * l15;
        const f32x4 bv = *(const f32x4 *)(a.bias + col0);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int orow = 16 * rt + 4 * l4 + j;
            if (orow >= nvalid) continue;
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const int col = col0 + c;
                const float x = acc[c][j] + bv[c];
                if (col < a.action_dim) a.logits[(size_t)orow * a.action_dim + col] = x;
                else if (col == a.action_dim) a.values[orow] = tanhf(x);
            }
        }
    }
}
}  // namespace

extern "C" int32_t azk_nn_ln_heads(const void *x_bf16_dev, float eps, const void *w_packed_dev, const float *bias_dev, int32_t n,
                                   int32_t embed_dim, int32_t n_out_padded, int32_t action_dim, float *logits_out_dev,
                                   float *values_out_dev, const int32_t *n_valid_dev, void *stream) {
    if (!x_bf16_dev || !w_packed_dev || !bias_dev || !logits_out_dev || !values_out_dev) return AZK_ERR_ARG;
    if (n < 0 || (embed_dim != 256 && embed_dim != 512) || n_out_padded < 64 || (n_out_padded & 63) || action_dim + 1 > n_out_padded) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    GemmArgs a = {};
    a.A = (const unsigned short *)x_bf16_dev; a.lda = embed_dim; a.Wp = (const uint4 *)w_packed_dev; a.M = n; a.N = n_out_padded;
    a.count = n_valid_dev; a.bias = bias_dev; a.ln_eps = eps; a.logits = logits_out_dev; a.values = values_out_dev; a.action_dim = action_dim;
    const long long items = (long long)((n + 15) / 16) * (n_out_padded / 64);       // 16-row x 64-column wave tiles
    const unsigned blocks = (unsigned)((items + 3) / 4 < 4096 ? (items + 3) / 4 : 4096);
    if (embed_dim == 512) k_ln_heads<16><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
    else k_ln_heads<8><<<blocks, 256, 0, (hipStream_t)stream>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}
