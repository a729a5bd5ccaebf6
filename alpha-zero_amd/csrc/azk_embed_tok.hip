// azk_embed_tok.hip - hand-written CDNA4 kernels for the policy-value network's token embedding (ai/nn.py:5-36):
//   tokens[n, 0, :]   = cls_token + pos_embedding[0]
//   tokens[n, 1+j, :] = Conv2d(C -> D, k x k, stride 1, 'same')(board)[:, r, c] + pos_embedding[1+j]      j = r*cols + c
// lowered to an im2col GEMM on the matrix cores (v_mfma_f32_16x16x32_bf16, fp32 accumulate).
//
// Structure (one wavefront = one 16-token x D output tile, no workgroup barriers in the main loop):
//   * the conv weight [D][KP] is staged ONCE per workgroup into LDS in MFMA-fragment order, so every B-fragment
//     read is a conflict-free, lane-linear ds_read_b128;
//   * the board is a bit string held across the wave's lanes (one ballot per 64 cells); each lane assembles the
//     k*k*C-bit patch of its token with funnel shifts and expands its 8 k-values to a bf16 A fragment - the
//     im2col matrix never exists in memory;
//   * bias + positional embedding enter as the accumulator's initial value (coalesced fp32 loads);
//   * the column -> accumulator map is permuted so each lane ends up with 8 consecutive columns per group:
//     LayerNorm statistics need only a 16-lane butterfly, and stores are 16 B per lane, 256 B contiguous.
// The kernel is bound by its HBM writes (T*D*2 bytes per board per output), not by MFMA.
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

namespace {
using namespace azk_nn;

struct EmbedArgs {
    const void *boards;        // [n][C][R][Cc] bf16 or f32, values 0/1
    int boards_f32;
    const __hip_bfloat16 *wt;  // [D][KP] conv weight, k index = ch*k*k + ky*k + kx, zero padded
    const float *cpos;         // [T][D]: row 0 = cls + pos[0]; row 1+j = conv bias + pos[1+j]
    const float *ln_w, *ln_b;  // [D] LayerNorm affine (used when xhat != nullptr)
    __hip_bfloat16 *x;         // [n][T][D] tokens (may be null)
    __hip_bfloat16 *xhat;      // [n][T][D] LayerNorm(tokens) (may be null)
    const float *mtab;         // scores variant: [T][16] per-token additive term of the 16 folded score columns (m'_h . cpos[t]), or null
    const float *msum;         // scores variant: [16] sum_d m'_h[d]
    float *scores;             // [n][NH][Tp] (Tp = 16*ceil(T/16)) xn_t . m'_h, written when mtab != null
    int nh;
    const int *count;          // optional device-side number of valid boards (<= n): rows beyond it are skipped
    int n, C, R, Cc, ksz, T;
    float eps;
    int ablate;                // debug only (AZK_EMBED_ABLATE): 1 no cpos loads, 2 no stores, 4 no MFMA, 8 no patch build
};

// NG = D / 128 column groups (each lane owns 8 consecutive columns per group); KS = KP / 32 k-steps.
template <int NG, int KS, bool WANT_X, bool WANT_XHAT, int NH>
__global__ __launch_bounds__(256, 2) void k_embed(EmbedArgs a) {
    constexpr int D = 128 * NG, KP = 32 * KS, NACC = 8 * NG;
    constexpr int NTILE = NACC + (NH > 0 ? 1 : 0);     // NH > 0: one extra 16-column tile = the folded head-score columns
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4 *bimg = (uint4 *)smem;                       // [NTILE][KS][64 lanes] 16-byte B fragments
    float *lnw = (float *)(smem + NTILE * KS * 64 * 16);  // [D] LayerNorm weight, then [D] bias (affine variant only)
    float *lnb = lnw + D;
    constexpr bool AFFINE = WANT_XHAT && NH == 0;      // NH > 0 emits the plain normalised tokens (affine folded by the caller)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // work item = (board, group of consecutive 16-token tiles): a board's tiles are spread over `groups` wavefronts so
    // the chip stays busy when only part of the batch is live
    const int tiles_per_leaf_ = (a.T + 15) >> 4;
    const int groups = tiles_per_leaf_ >= 6 ? 3 : 1, tiles_per_group = (tiles_per_leaf_ + groups - 1) / groups;
    const int nvalid = a.count ? min(a.n, *a.count) : a.n;
    const int nitems = nvalid * groups;
    if ((int)blockIdx.x * 4 >= nitems) return;                  // nothing for this workgroup: skip the weight staging too

    // ---- stage the weight in fragment order: fragment (acc, s) of lane l = wt[col(acc, l)][32 s + 8 (l>>4) .. +8] ----
    for (int f = tid; f < NTILE * KS * 64; f += 256) {
        const int l = f & 63, s = (f >> 6) % KS, acc = (f >> 6) / KS;
        const int col = acc < NACC ? 128 * (acc >> 3) + 8 * (l & 15) + (acc & 7) : D + (l & 15);   // weight rows D..D+15: score columns
        bimg[f] = *(const uint4 *)(a.wt + (size_t)col * KP + 32 * s + 8 * (l >> 4));
    }
    if (AFFINE)
        for (int i = tid; i < D; i += 256) { lnw[i] = a.ln_w[i]; lnb[i] = a.ln_b[i]; }
    __syncthreads();

    const int RC = a.R * a.Cc, T = a.T, ksz = a.ksz, kk = ksz * ksz, pad = ksz / 2, ncell = a.C * RC;
    const int tiles_per_leaf = (T + 15) >> 4;
    const int nwaves = gridDim.x * 4;

    // the board's bit string is built once per item, then the wave walks its group of 16-token tiles
    for (int item = blockIdx.x * 4 + wave; item < nitems; item += nwaves) {
        const int leaf = item / groups, grp = item - leaf * groups;
        const int tile_lo = grp * tiles_per_group;
        const int tile_hi = min(tiles_per_leaf, tile_lo + tiles_per_group);
        unsigned wbits = 0;                             // lane i holds bits [32 (i-1), 32 i) of the board bit string (lane 0: zeros)
        if (!(a.ablate & 8)) {
            for (int q = 0; q * 64 < ncell; q++) {
                const int e = q * 64 + lane;
                bool on = false;
                if (e < ncell)
                    on = a.boards_f32 ? ((const float *)a.boards)[(size_t)leaf * ncell + e] != 0.0f
                                      : (((const unsigned short *)a.boards)[(size_t)leaf * ncell + e] & 0x7fff) != 0;
                const unsigned long long m = __ballot(on);
                if ((lane - 1) >> 1 == q && lane >= 1) wbits = ((lane - 1) & 1) ? (unsigned)(m >> 32) : (unsigned)m;
            }
        }
      for (int tile = tile_lo; tile < tile_hi; tile++) {
        // ---- this lane's token (A-fragment row l&15) and its patch bits ----
        const int t = tile * 16 + l15;
        unsigned long long plo = 0, phi = 0;
        {
            const int j = t - 1, r = j / a.Cc, c = j - r * a.Cc;
            const bool live = t >= 1 && t < T;
            unsigned colmask = 0;
            for (int kx = 0; kx < ksz; kx++) { const int cc = c + kx - pad; if (cc >= 0 && cc < a.Cc) colmask |= 1u << kx; }
            for (int ch = 0; ch < ((a.ablate & 8) ? 0 : a.C); ch++)
                for (int ky = 0; ky < ksz; ky++) {
                    const int rr = r + ky - pad;
                    // every lane takes part in the shuffles; dead rows contribute zero bits
                    const int off = 32 + ch * RC + (rr < 0 ? 0 : (rr >= a.R ? a.R - 1 : rr)) * a.Cc + (c - pad);
                    const int wi = off >> 5, sh = off & 31;
                    const unsigned lo = __shfl(wbits, wi), hi = __shfl(wbits, wi + 1);
                    unsigned bits = __funnelshift_r(lo, hi, sh) & colmask;
                    if (!live || rr < 0 || rr >= a.R) bits = 0;
                    const int p0 = ch * kk + ky * ksz;
                    if (p0 < 64) { plo |= (unsigned long long)bits << p0; if (p0 + ksz > 64) phi |= (unsigned long long)bits >> (64 - p0); }
                    else phi |= (unsigned long long)bits << (p0 - 64);
                }
        }
        bf16x8 afrag[KS];
#pragma unroll
        for (int s = 0; s < KS; s++) {
            const int b0 = 32 * s + 8 * l4;
            const unsigned byte = (unsigned)((b0 < 64 ? (plo >> b0) : (phi >> (b0 - 64))) & 0xff);
            union { bf16x8 v; unsigned short h[8]; } u;
#pragma unroll
            for (int q = 0; q < 8; q++) u.h[q] = ((byte >> q) & 1) ? 0x3F80 : 0;
            afrag[s] = u.v;
        }
        // ---- accumulators start at bias + positional embedding (C/D map: col = lane&15 -> permuted column,
        //      row = 4 (lane>>4) + reg) ----
        f32x4 acc[NACC];
        int trow[4];
#pragma unroll
        for (int r4 = 0; r4 < 4; r4++) { const int tt = tile * 16 + 4 * l4 + r4; trow[r4] = tt < T ? tt : T - 1; }
#pragma unroll
        for (int g = 0; g < NG; g++)
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) {
                const float *src = a.cpos + ((a.ablate & 1) ? 0 : (size_t)trow[r4] * D) + 128 * g + 8 * l15;
                const f32x4 c0 = *(const f32x4 *)src, c1 = *(const f32x4 *)(src + 4);
                acc[g * 8 + 0][r4] = c0[0]; acc[g * 8 + 1][r4] = c0[1]; acc[g * 8 + 2][r4] = c0[2]; acc[g * 8 + 3][r4] = c0[3];
                acc[g * 8 + 4][r4] = c1[0]; acc[g * 8 + 5][r4] = c1[1]; acc[g * 8 + 6][r4] = c1[2]; acc[g * 8 + 7][r4] = c1[3];
            }
        f32x4 acce;                                                   // NH > 0: raw scores x_t . m'_h for head = lane&15, tokens 4 (lane>>4) + r
        if (NH > 0) {
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) acce[r4] = a.mtab[(size_t)trow[r4] * 16 + l15];
#pragma unroll
            for (int s = 0; s < KS; s++) {
                union { uint4 u; bf16x8 v; } bf;
                bf.u = bimg[(NACC * KS + s) * 64 + lane];
                acce = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[s], bf.v, acce, 0, 0, 0);
            }
        }
        // ---- MFMA: acc[n] (16 x 16) += A (16 x KP) * B (KP x 16) ----
        if (!(a.ablate & 4))
#pragma unroll
        for (int n = 0; n < NACC; n++) {
#pragma unroll
            for (int s = 0; s < KS; s++) {
                union { uint4 u; bf16x8 v; } bf;
                bf.u = bimg[(n * KS + s) * 64 + lane];
                acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[s], bf.v, acc[n], 0, 0, 0);
            }
            if ((n & 3) == 3) __builtin_amdgcn_sched_barrier(0);   // keep B-fragment prefetch to 4 accumulators (VGPR budget)
        }
        // ---- epilogue: rows 4 (lane>>4) + r4, this lane's columns 128 g + 8 (lane&15) + q ----
        float mean[4], rstd[4];
        if (WANT_XHAT) {
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) {
                float s = 0.f;
#pragma unroll
                for (int n = 0; n < NACC; n++) s += acc[n][r4];
                s = row16_sum(s);
                mean[r4] = s * (1.0f / (float)D);
                float ss = 0.f;
#pragma unroll
                for (int n = 0; n < NACC; n++) { const float dl = acc[n][r4] - mean[r4]; ss += dl * dl; }
                ss = row16_sum(ss);
                rstd[r4] = rsqrtf(ss * (1.0f / (float)D) + a.eps);
            }
        }
#pragma unroll
        for (int g = 0; g < NG; g++) {
            f32x4 w0, w1, b0, b1;
            if (AFFINE) {
                w0 = *(const f32x4 *)(lnw + 128 * g + 8 * l15); w1 = *(const f32x4 *)(lnw + 128 * g + 8 * l15 + 4);
                b0 = *(const f32x4 *)(lnb + 128 * g + 8 * l15); b1 = *(const f32x4 *)(lnb + 128 * g + 8 * l15 + 4);
            }
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) {
                const int tt = tile * 16 + 4 * l4 + r4;
                const bool ok = tt < T && !((a.ablate & 2) && tt != 7777);
                const size_t orow = ((size_t)leaf * T + (tt < T ? tt : 0)) * D;
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; q++) v[q] = acc[g * 8 + q][r4];
                if (WANT_X && ok) *(uint4 *)(a.x + orow + 128 * g + 8 * l15) = pack8(v);
                if (WANT_XHAT) {
                    if (AFFINE) {
#pragma unroll
                        for (int q = 0; q < 4; q++) {
                            v[q] = (v[q] - mean[r4]) * rstd[r4] * w0[q] + b0[q];
                            v[q + 4] = (v[q + 4] - mean[r4]) * rstd[r4] * w1[q] + b1[q];
                        }
                    } else {
#pragma unroll
                        for (int q = 0; q < 8; q++) v[q] = (v[q] - mean[r4]) * rstd[r4];
                    }
                    if (ok) *(uint4 *)(a.xhat + orow + 128 * g + 8 * l15) = pack8(v);
                }
            }
        }
        if (NH > 0 && l15 < NH) {
            // xn = (x - mean) * rstd  =>  xn . m' = rstd * (x . m' - mean * sum(m'))
            const int Tp = tiles_per_leaf * 16;
            const float ms = a.msum[l15];
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++)
                a.scores[((size_t)leaf * NH + l15) * Tp + tile * 16 + 4 * l4 + r4] = rstd[r4] * (acce[r4] - mean[r4] * ms);
        }
      }
    }
}

template <int NG, int KS, bool WX, bool WH, int NH>
int launch_embed2(const EmbedArgs &a, hipStream_t st) {
    constexpr int NACC = 8 * NG;
    const int lds = (NACC + (NH > 0 ? 1 : 0)) * KS * 64 * 16 + (NH > 0 ? 0 : 2 * 128 * NG * 4);
    const int tiles = (a.T + 15) >> 4, groups = tiles >= 6 ? 3 : 1;
    long long blocks = ((long long)a.n * groups + 3) / 4;       // one wavefront per (board, tile group); idle workgroups exit at once
    if (blocks > 4096) blocks = 4096;
    if (azk_set_max_lds((const void *)k_embed<NG, KS, WX, WH, NH>, lds) != hipSuccess) return AZK_ERR_HIP;
    k_embed<NG, KS, WX, WH, NH><<<(unsigned)blocks, 256, lds, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

template <int NG, int KS>
int launch_embed(const EmbedArgs &a, hipStream_t st) {
    if (a.mtab) {                                     // scores ride along with xhat (folded cls attention, shared query)
        if (!a.xhat || a.x) return AZK_ERR_ARG;
        if (a.nh == 8) return launch_embed2<NG, KS, false, true, 8>(a, st);
        if (a.nh == 4) return launch_embed2<NG, KS, false, true, 4>(a, st);
        return AZK_ERR_ARG;
    }
    if (a.x && a.xhat) return launch_embed2<NG, KS, true, true, 0>(a, st);
    if (a.xhat) return launch_embed2<NG, KS, false, true, 0>(a, st);
    return launch_embed2<NG, KS, true, false, 0>(a, st);
}

}  // namespace

static int32_t patch_embed_impl(const void *boards_dev, int32_t boards_are_f32, const void *wt_bf16_dev,
                                const float *cpos_dev, const float *ln_w_dev, const float *ln_b_dev,
                                void *x_out_bf16_dev, void *xhat_out_bf16_dev, int32_t n, int32_t channels,
                                int32_t rows, int32_t cols, int32_t ksize, int32_t kp, int32_t embed_dim,
                                float ln_eps, const float *mtab_dev, const float *msum_dev, float *scores_dev, int32_t num_heads,
                                const int32_t *n_valid_dev, void *stream) {
    if (!boards_dev || !wt_bf16_dev || !cpos_dev || (!x_out_bf16_dev && !xhat_out_bf16_dev)) return AZK_ERR_ARG;
    if (xhat_out_bf16_dev && !mtab_dev && (!ln_w_dev || !ln_b_dev)) return AZK_ERR_ARG;   // the scores variant has no affine
    if (n < 0 || channels < 1 || rows < 1 || cols < 1 || ksize < 1 || (ksize & 1) == 0 || ksize > 7) return AZK_ERR_ARG;
    if (kp < channels * ksize * ksize || kp % 32 != 0 || kp > 128) return AZK_ERR_ARG;
    if (channels * rows * cols > 62 * 32) return AZK_ERR_ARG;         // the board bit string lives in one wave's lanes
    if (n == 0) return AZK_OK;
    EmbedArgs a;
    a.boards = boards_dev; a.boards_f32 = boards_are_f32; a.wt = (const __hip_bfloat16 *)wt_bf16_dev; a.cpos = cpos_dev;
    a.ln_w = ln_w_dev; a.ln_b = ln_b_dev; a.x = (__hip_bfloat16 *)x_out_bf16_dev; a.xhat = (__hip_bfloat16 *)xhat_out_bf16_dev;
    a.mtab = mtab_dev; a.msum = msum_dev; a.scores = scores_dev; a.nh = num_heads; a.count = n_valid_dev;
    if ((mtab_dev != nullptr) != (scores_dev != nullptr)) return AZK_ERR_ARG;
    { const char *ab = getenv("AZK_EMBED_ABLATE"); a.ablate = ab ? atoi(ab) : 0; }
    a.n = n; a.C = channels; a.R = rows; a.Cc = cols; a.ksz = ksize; a.T = rows * cols + 1; a.eps = ln_eps;
    hipStream_t st = (hipStream_t)stream;
    const int ks = kp / 32;
#define CASE(NG_, KS_) if (embed_dim == 128 * NG_ && ks == KS_) return launch_embed<NG_, KS_>(a, st)
    CASE(4, 2); CASE(4, 1); CASE(4, 3);
    CASE(2, 2); CASE(2, 1); CASE(2, 3);
    CASE(1, 2); CASE(1, 1); CASE(1, 3);
#undef CASE
    return AZK_ERR_ARG;   // unsupported (embed_dim, kp): the caller keeps its generic path
}

extern "C" int32_t azk_nn_patch_embed(const void *boards_dev, int32_t boards_are_f32, const void *wt_bf16_dev,
                                      const float *cpos_dev, const float *ln_w_dev, const float *ln_b_dev,
                                      void *x_out_bf16_dev, void *xhat_out_bf16_dev, int32_t n, int32_t channels,
                                      int32_t rows, int32_t cols, int32_t ksize, int32_t kp, int32_t embed_dim,
                                      float ln_eps, void *stream) {
    return patch_embed_impl(boards_dev, boards_are_f32, wt_bf16_dev, cpos_dev, ln_w_dev, ln_b_dev, x_out_bf16_dev,
                            xhat_out_bf16_dev, n, channels, rows, cols, ksize, kp, embed_dim, ln_eps, nullptr, nullptr, nullptr, 0, nullptr, stream);
}

extern "C" int32_t azk_nn_patch_embed_scores(const void *boards_dev, int32_t boards_are_f32, const void *wt_bf16_dev,
                                             const float *cpos_dev, const float *ln_w_dev, const float *ln_b_dev,
                                             void *xhat_out_bf16_dev, const float *score_cpos_dev, const float *score_msum_dev,
                                             float *scores_out_dev, int32_t num_heads, int32_t n, int32_t channels, int32_t rows, int32_t cols,
                                             int32_t ksize, int32_t kp, int32_t embed_dim, float ln_eps,
                                             const int32_t *n_valid_dev, void *stream) {
    if (!score_cpos_dev || !score_msum_dev || !scores_out_dev) return AZK_ERR_ARG;
    return patch_embed_impl(boards_dev, boards_are_f32, wt_bf16_dev, cpos_dev, ln_w_dev, ln_b_dev, nullptr,
                            xhat_out_bf16_dev, n, channels, rows, cols, ksize, kp, embed_dim, ln_eps, score_cpos_dev, score_msum_dev,
                            scores_out_dev, num_heads, n_valid_dev, stream);
}

// =====================================================================================================
// cls-row attention of the LAST block, folded (ai/nn.py:52-56 restricted to the row nn.py:80 reads).
// With q = Wq LN1(x)[cls] + bq fixed per board, the scores against every token are
//     s[h][t] = scale * q_h . (Wk_h xhat_t + bk_h) = xhat_t . m_h + c_h,   m_h = scale * Wk_h^T q_h,  c_h = scale * q_h . bk_h
// and the head outputs are Wv_h (sum_t softmax_t(s[h])[t] xhat_t) + bv_h, so K and V are never formed:
// this kernel streams xhat once (online softmax, flash-style running max / sum per wave) and emits
//     z[b][h][:] = sum_t softmax_t(s[b][h][:])[t] * xhat[b][t][:]            ([n][H][D])
// The tiny per-board GEMMs around it (m_h, Wv_h z_h, out-proj, MLP, heads) stay in the caller.
// One workgroup (4 waves) per board; wave w takes tokens t = w (mod 4); lane l owns CPL = D/64 columns.
// HBM-bound: reads T*D*2 bytes per board once.
// =====================================================================================================
namespace {

struct ClsAttnArgs {
    const __hip_bfloat16 *xhat;   // [n][T][D]
    const float *m;               // [n or 1][H][D]  (already multiplied by the softmax scale)
    const float *c;               // [n or 1][H]
    long long m_stride, c_stride; // elements between boards (0 = shared by every board)
    __hip_bfloat16 *z;            // [n][H][D]
    int n, T;
};

template <int CPL, int NH>
__global__ __launch_bounds__(256) void k_cls_attn(ClsAttnArgs a) {
    constexpr int D = 64 * CPL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *zpart = (float *)smem;                    // [4 waves][NH][D]
    float *mlpart = (float *)(smem + 4 * NH * D * 4); // [4][NH] running max, then [4][NH] running sum
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const float *mp = a.m + (size_t)b * a.m_stride, *cp = a.c + (size_t)b * a.c_stride;
    float mh[NH][CPL], ch[NH];
#pragma unroll
    for (int h = 0; h < NH; h++) {
        ch[h] = cp[h];
#pragma unroll
        for (int q = 0; q < CPL; q++) mh[h][q] = mp[h * D + lane * CPL + q];
    }
    float run_m[NH], run_l[NH], zacc[NH][CPL];
#pragma unroll
    for (int h = 0; h < NH; h++) {
        run_m[h] = -3.0e38f; run_l[h] = 0.f;
#pragma unroll
        for (int q = 0; q < CPL; q++) zacc[h][q] = 0.f;
    }
    const unsigned short *base = (const unsigned short *)a.xhat + (size_t)b * a.T * D + lane * CPL;
    for (int t = wave; t < a.T; t += 4) {
        float xv[CPL];
        if (CPL == 8) {
            const uint4 raw = *(const uint4 *)(base + (size_t)t * D);
            xv[0] = __uint_as_float(raw.x << 16); xv[1] = __uint_as_float(raw.x & 0xffff0000u);
            xv[2] = __uint_as_float(raw.y << 16); xv[3] = __uint_as_float(raw.y & 0xffff0000u);
            xv[4] = __uint_as_float(raw.z << 16); xv[5] = __uint_as_float(raw.z & 0xffff0000u);
            xv[6] = __uint_as_float(raw.w << 16); xv[7] = __uint_as_float(raw.w & 0xffff0000u);
        } else {
#pragma unroll
            for (int q = 0; q < CPL; q++) xv[q] = __uint_as_float((unsigned)base[(size_t)t * D + q] << 16);
        }
        float s[NH];
#pragma unroll
        for (int h = 0; h < NH; h++) {
            float p = 0.f;
#pragma unroll
            for (int q = 0; q < CPL; q++) p += xv[q] * mh[h][q];
            s[h] = p;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1)
#pragma unroll
            for (int h = 0; h < NH; h++) s[h] += __shfl_xor(s[h], off);
#pragma unroll
        for (int h = 0; h < NH; h++) {
            const float sc = s[h] + ch[h];
            const float nm = fmaxf(run_m[h], sc);
            const float alpha = __expf(run_m[h] - nm), p = __expf(sc - nm);
            run_m[h] = nm;
            run_l[h] = run_l[h] * alpha + p;
#pragma unroll
            for (int q = 0; q < CPL; q++) zacc[h][q] = zacc[h][q] * alpha + p * xv[q];
        }
    }
    // ---- combine the four waves' partial (max, sum, z) ----
#pragma unroll
    for (int h = 0; h < NH; h++) {
        if (lane == 0) { mlpart[wave * NH + h] = run_m[h]; mlpart[4 * NH + wave * NH + h] = run_l[h]; }
#pragma unroll
        for (int q = 0; q < CPL; q++) zpart[(wave * NH + h) * D + lane * CPL + q] = zacc[h][q];
    }
    __syncthreads();
    for (int i = tid; i < NH * D; i += 256) {
        const int h = i / D, col = i - h * D;
        float M = mlpart[h];
#pragma unroll
        for (int w = 1; w < 4; w++) M = fmaxf(M, mlpart[w * NH + h]);
        float L = 0.f, Z = 0.f;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const float e = __expf(mlpart[w * NH + h] - M);
            L += mlpart[4 * NH + w * NH + h] * e;
            Z += zpart[(w * NH + h) * D + col] * e;
        }
        a.z[((size_t)b * NH + h) * D + col] = __float2bfloat16(Z / L);
    }
}

template <int CPL, int NH>
int launch_cls_attn(const ClsAttnArgs &a, hipStream_t st) {
    constexpr int D = 64 * CPL;
    const int lds = 4 * NH * D * 4 + 8 * NH * 4;
    if (azk_set_max_lds((const void *)k_cls_attn<CPL, NH>, lds) != hipSuccess) return AZK_ERR_HIP;
    k_cls_attn<CPL, NH><<<a.n, 256, lds, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

}  // namespace

extern "C" int32_t azk_nn_cls_attention(const void *xhat_bf16_dev, const float *m_dev, const float *c_dev,
                                        int32_t per_board_m, void *z_out_bf16_dev, int32_t n, int32_t tokens,
                                        int32_t embed_dim, int32_t num_heads, void *stream) {
    if (!xhat_bf16_dev || !m_dev || !c_dev || !z_out_bf16_dev || n < 0 || tokens < 1) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    ClsAttnArgs a;
    a.xhat = (const __hip_bfloat16 *)xhat_bf16_dev; a.m = m_dev; a.c = c_dev; a.z = (__hip_bfloat16 *)z_out_bf16_dev;
    a.m_stride = per_board_m ? (long long)num_heads * embed_dim : 0; a.c_stride = per_board_m ? num_heads : 0;
    a.n = n; a.T = tokens;
    hipStream_t st = (hipStream_t)stream;
#define CASE(CPL_, NH_) if (embed_dim == 64 * CPL_ && num_heads == NH_) return launch_cls_attn<CPL_, NH_>(a, st)
    CASE(8, 8); CASE(4, 8); CASE(4, 4); CASE(2, 4); CASE(2, 8); CASE(8, 4);
#undef CASE
    return AZK_ERR_ARG;
}

// =====================================================================================================
// k_cls_pool: the streaming half of the folded cls attention when the scores already exist (emitted by k_embed for the
// depth-1 case, where the cls query is a constant of the weights):  a = softmax_t(scores[b][h][:] + c[h]),
// z[b][h][:] = sum_t a[h][t] * xhat[b][t][:].  No cross-lane reduction in the token loop: each lane owns 8 (CPL)
// columns, reads its 16 bytes of every token row and the token's NH weights (one broadcast LDS read).
// One workgroup per board, 4 waves interleave tokens, 4 tokens in flight per wave.  HBM-read-bound.
// Any token count whose weights [Tp][NH] and two partial rows [NH][D] fit 64 KB of LDS (the entry point refuses the others).
// =====================================================================================================
namespace {

struct ClsPoolArgs {
    const __hip_bfloat16 *xhat;   // [n][T][D]
    const float *scores;          // [n][NH][Tp]
    const float *c;               // [NH]
    __hip_bfloat16 *z;            // [n][NH][D]
    int n, T, Tp;
    const int *count;             // optional device-side number of valid boards
    int ablate;                   // debug only (AZK_POOL_ABLATE): 1 no softmax phase, 2 no token loop, 4 no combine
};

template <int CPL>
__device__ __forceinline__ void load_row(const unsigned short *p, float *xv) {
    if (CPL == 8) {
        const uint4 raw = *(const uint4 *)p;
        xv[0] = __uint_as_float(raw.x << 16); xv[1] = __uint_as_float(raw.x & 0xffff0000u);
        xv[2] = __uint_as_float(raw.y << 16); xv[3] = __uint_as_float(raw.y & 0xffff0000u);
        xv[4] = __uint_as_float(raw.z << 16); xv[5] = __uint_as_float(raw.z & 0xffff0000u);
        xv[6] = __uint_as_float(raw.w << 16); xv[7] = __uint_as_float(raw.w & 0xffff0000u);
    } else if (CPL == 4) {
        const uint2 raw = *(const uint2 *)p;
        xv[0] = __uint_as_float(raw.x << 16); xv[1] = __uint_as_float(raw.x & 0xffff0000u);
        xv[2] = __uint_as_float(raw.y << 16); xv[3] = __uint_as_float(raw.y & 0xffff0000u);
    } else {
        const unsigned raw = *(const unsigned *)p;
        xv[0] = __uint_as_float(raw << 16); xv[1] = __uint_as_float(raw & 0xffff0000u);
    }
}

template <int CPL, int NH>
__global__ __launch_bounds__(256) void k_cls_pool(ClsPoolArgs a) {
    constexpr int D = 64 * CPL;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;                                // one workgroup (4 waves) per board: wave w takes tokens 8 (4 i + w) .. +8
    if (b >= (a.count ? min(a.n, *a.count) : a.n)) return;
    float *aw = (float *)smem;                               // [Tp][NH] softmax weights
    float *zpart = aw + (size_t)a.Tp * NH;                   // [2][NH][D] partial sums handed between waves
    const float *sp = a.scores + (size_t)b * NH * a.Tp;
    // ---- softmax over tokens: wave w handles heads w, w + 4 (scores are tiny: NH * T floats) ----
    // Lane l takes the tokens l + 64 k for every k < ceil(Tp / 64), in rising k: maximum, sum and weights each walk the same
    // chunks, so a lane's order of operations does not depend on how many chunks there are.  Between the passes a token's value
    // waits in its own aw slot, which only this lane touches before the barrier.
    if (!(a.ablate & 1)) {
        const int nchunk = (a.Tp + 63) >> 6;
        for (int h = wave; h < NH; h += 4) {
            const float ch = a.c[h];
            float mx = -3.0e38f;
            for (int k = 0; k < nchunk; k++) {
                const int t = lane + 64 * k;
                if (t < a.T) { const float e = sp[h * a.Tp + t] + ch; aw[t * NH + h] = e; mx = fmaxf(mx, e); }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
            float sum = 0.f;
            for (int k = 0; k < nchunk; k++) {
                const int t = lane + 64 * k;
                if (t < a.T) { const float e = __expf(aw[t * NH + h] - mx); aw[t * NH + h] = e; sum += e; }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off);
            const float inv = 1.0f / sum;
            for (int k = 0; k < nchunk; k++) {
                const int t = lane + 64 * k;
                if (t < a.Tp) aw[t * NH + h] = t < a.T ? aw[t * NH + h] * inv : 0.f;      // the Tp padding weighs exactly 0
            }
        }
    }
    __syncthreads();
    // ---- weighted token sum: each lane owns CPL columns; 8-row register sets, two in flight per wave ----
    float zacc[NH][CPL];
#pragma unroll
    for (int h = 0; h < NH; h++)
#pragma unroll
        for (int q = 0; q < CPL; q++) zacc[h][q] = 0.f;
    const unsigned short *base = (const unsigned short *)a.xhat + (size_t)b * a.T * D + lane * CPL;
    const int T = (a.ablate & 2) ? 0 : a.T;
    // raw rows stay in registers exactly as loaded (no conversion at fetch time, so nothing waits on a load until its row
    // is consumed and a whole 8-row set stays in flight behind the one being used)
    typedef typename std::conditional<CPL == 8, uint4, typename std::conditional<CPL == 4, uint2, unsigned>::type>::type raw_t;
    auto consume = [&](const raw_t (&x)[8], int t0) {
#pragma unroll
        for (int k = 0; k < 8; k++) {
            float xv[CPL];
            if constexpr (CPL == 8) {
                xv[0] = __uint_as_float(x[k].x << 16); xv[1] = __uint_as_float(x[k].x & 0xffff0000u);
                xv[2] = __uint_as_float(x[k].y << 16); xv[3] = __uint_as_float(x[k].y & 0xffff0000u);
                xv[4] = __uint_as_float(x[k].z << 16); xv[5] = __uint_as_float(x[k].z & 0xffff0000u);
                xv[6] = __uint_as_float(x[k].w << 16); xv[7] = __uint_as_float(x[k].w & 0xffff0000u);
            } else if constexpr (CPL == 4) {
                xv[0] = __uint_as_float(x[k].x << 16); xv[1] = __uint_as_float(x[k].x & 0xffff0000u);
                xv[2] = __uint_as_float(x[k].y << 16); xv[3] = __uint_as_float(x[k].y & 0xffff0000u);
            } else {
                xv[0] = __uint_as_float(x[k] << 16); xv[1] = __uint_as_float(x[k] & 0xffff0000u);
            }
            float w[NH];
#pragma unroll
            for (int h = 0; h < NH; h += 4) {
                const f32x4 w4 = *(const f32x4 *)(aw + (t0 + k) * NH + h);
                w[h] = w4[0]; w[h + 1] = w4[1]; w[h + 2] = w4[2]; w[h + 3] = w4[3];
            }
#pragma unroll
            for (int h = 0; h < NH; h++)
#pragma unroll
                for (int q = 0; q < CPL; q++) zacc[h][q] += w[h] * xv[q];
        }
    };
    // rows past T are clamped to the last row; their weights aw[t >= T] are exactly 0 (Tp padding), so they add nothing
    auto fetch = [&](raw_t (&x)[8], int t0) {
#pragma unroll
        for (int k = 0; k < 8; k++) { const int t = t0 + k < a.T ? t0 + k : a.T - 1; x[k] = *(const raw_t *)(base + (size_t)t * D); }
    };
    raw_t xa[8], xb[8];
    const int t_first = 8 * wave;                             // this wave's 8-token chunks: t_first, t_first + 32, ...
    if (t_first < T) fetch(xa, t_first);
    for (int t = t_first; t < T; t += 64) {
        if (t + 32 < T) fetch(xb, t + 32);
        consume(xa, t);
        if (t + 64 < T) fetch(xa, t + 64);
        if (t + 32 < T) consume(xb, t + 32);
    }
    // ---- combine the four waves: 3,2 -> LDS ; 1,0 add theirs and 1 -> LDS ; 0 adds, packs, stores ----
    if (!(a.ablate & 4)) {
        if (wave >= 2) {
#pragma unroll
            for (int h = 0; h < NH; h++)
#pragma unroll
                for (int q = 0; q < CPL; q++) zpart[((wave - 2) * NH + h) * D + q * 64 + lane] = zacc[h][q];
        }
        __syncthreads();
        if (wave < 2) {
#pragma unroll
            for (int h = 0; h < NH; h++)
#pragma unroll
                for (int q = 0; q < CPL; q++) zacc[h][q] += zpart[(wave * NH + h) * D + q * 64 + lane];
        }
        __syncthreads();
        if (wave == 1) {
#pragma unroll
            for (int h = 0; h < NH; h++)
#pragma unroll
                for (int q = 0; q < CPL; q++) zpart[h * D + q * 64 + lane] = zacc[h][q];
        }
        __syncthreads();
        if (wave == 0) {
#pragma unroll
            for (int h = 0; h < NH; h++) {
#pragma unroll
                for (int q = 0; q < CPL; q++) zacc[h][q] += zpart[h * D + q * 64 + lane];
                unsigned short *dst = (unsigned short *)a.z + ((size_t)b * NH + h) * D + lane * CPL;
                if (CPL == 8) {
                    *(uint4 *)dst = pack8(zacc[h]);
                } else {
#pragma unroll
                    for (int q = 0; q < CPL; q++) dst[q] = __bfloat16_as_ushort(__float2bfloat16(zacc[h][q]));
                }
            }
        }
    }
}

template <int CPL, int NH>
int launch_cls_pool(const ClsPoolArgs &a, hipStream_t st) {
    const int lds = (a.Tp * NH + 2 * NH * 64 * CPL) * 4;
    if (azk_set_max_lds((const void *)k_cls_pool<CPL, NH>, 64 * 1024) != hipSuccess) return AZK_ERR_HIP;
    if (lds > 64 * 1024) return AZK_ERR_ARG;
    k_cls_pool<CPL, NH><<<a.n, 256, lds, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

}  // namespace

extern "C" int32_t azk_nn_cls_pool(const void *xhat_bf16_dev, const float *scores_dev, const float *c_dev,
                                   void *z_out_bf16_dev, int32_t n, int32_t tokens, int32_t embed_dim,
                                   int32_t num_heads, const int32_t *n_valid_dev, void *stream) {
    if (!xhat_bf16_dev || !scores_dev || !c_dev || !z_out_bf16_dev || n < 0 || tokens < 1) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    ClsPoolArgs a;
    a.xhat = (const __hip_bfloat16 *)xhat_bf16_dev; a.scores = scores_dev; a.c = c_dev; a.z = (__hip_bfloat16 *)z_out_bf16_dev;
    a.n = n; a.T = tokens; a.Tp = (tokens + 15) / 16 * 16; a.count = n_valid_dev;
    { const char *ab = getenv("AZK_POOL_ABLATE"); a.ablate = ab ? atoi(ab) : 0; }
    hipStream_t st = (hipStream_t)stream;
#define CASE(CPL_, NH_) if (embed_dim == 64 * CPL_ && num_heads == NH_) return launch_cls_pool<CPL_, NH_>(a, st)
    CASE(8, 8); CASE(4, 8); CASE(4, 4); CASE(2, 4); CASE(2, 8); CASE(8, 4);
#undef CASE
    return AZK_ERR_ARG;
}
