// azk_embed_conv.hip - the token-forming evaluators that keep the whole cls path of a depth-1 network on the CU: the conv of every
// (k_embed_pool) or of every stone-touched (k_embed_pool_c, `--embed conv`) token, LayerNorm1, the folded cls scores, the softmax
// over the tokens and the weighted token sum in ONE kernel; pooled rows z[n][H][D] out.  The token rows never reach memory
// (azk_embed_tok.hip holds the generation that writes them; azk_nn.hip the one that forms no token at all).
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
// k_embed_pool: patch embedding + LayerNorm1 + folded cls attention (scores, softmax over tokens, weighted token sum)
// in ONE kernel - the normalised tokens never leave the CU (nn.py:13-36, 52-56 restricted to the cls query).
//   One workgroup (4 waves) per board; wave w owns the 128 output columns [128 w, 128 w + 128) of every 16-token tile
//   (8 MFMA accumulators) and recomputes the 16 extra columns (heads' raw scores, and column 15 = the row mean).  Per tile:
//     x tile (MFMA 16x16x32; accumulators start at bias + positional embedding; A fragments = a 256-entry LDS table
//     indexed by 8 patch bits)
//     -> per-row sum of squares over the wave's columns -> LDS -> one barrier -> LayerNorm statistics of the full row
//     -> scores s[t][h] = rstd_t (x_t . m'_h - mean_t sum(m'_h)); weights w = exp(s - ref_h): ref_h is either a static
//        upper bound (|s| <= sqrt(D) |m'_h|, used when it cannot underflow) or the running maximum (online softmax)
//     -> Z[h][cols] += sum_t w[t][h] xn[t][cols] as MFMA 16x16x16: the A operand (weights: head = lane&15, tokens
//        4 (lane>>4) + r) and the B operand (normalised tile: column = lane&15, same tokens) are exactly the C/D layout
//        the score and x accumulators already have, so nothing moves between lanes.
//   Output z[b][h][:] = Z[h][:] / L[h]  ([n][H][D] bf16).  No HBM traffic besides the board, the (L2-resident) constants
//   and 8 KB of output per board.  The per-token constants are padded to whole tiles by the caller: padding rows of
//   cpos are 0 and padding rows of the score columns are -1e30, which makes their softmax weight exactly 0.
// =====================================================================================================
namespace {
using namespace azk_nn;

struct EmbedPoolArgs {
    const void *boards;
    int boards_f32;
    const __hip_bfloat16 *wt;   // [D + 16][KP]: conv weight rows, then the 16 extra rows (head scores; row 15 = column mean)
    const float *cpos;          // accumulator order [tiles][4 waves][8][64 lanes][4 rows]: cpos[16 tile + 4 (lane>>4) + r][128 wave + 8 (lane&15) + q], rows >= T zero
    const float *mtab;          // accumulator order [tiles][64 lanes][4 rows]: score constants [16 tile + 4 (lane>>4) + r][lane&15]; rows >= T: -1e30 in the head columns
    const float *msum;          // [16]
    const float *sref;          // [16] static per-head reference (upper bound of the scores) or null = running maximum
    __hip_bfloat16 *z;          // [n][NH][D]
    const int *count;
    int n, C, R, Cc, ksz, T;
    float eps;
    azk_leaf_source src;        // SRC variant only
};

// SRC: the boards are the engine's pending leaves (azk_leaf_source): the kernel builds the prefix over the leaf flags itself
// (board j = the j-th flagged game, ascending game order = azk_step_gather's order), reads the cell codes of that game,
// records the slot for the next expansion and publishes the leaf count - no compaction launch, no evaluator batch.
template <int KS, int NH, bool STATIC_REF, bool SRC>
__global__ __launch_bounds__(256, 2) void k_embed_pool(EmbedPoolArgs a) {
    constexpr int D = 512, KP = 32 * KS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4 *alut = (uint4 *)smem;                                  // [256] A fragment of 8 patch bits (bit q -> bf16 1.0 in slot q)
    const int Tp16 = ((a.T + 15) >> 4) * 16;
    float *part = (float *)(alut + 256);                          // [2 parities][16 rows][4 waves] partial sums of squares
    uint4 *pbits = (uint4 *)(part + 128);                         // [Tp] patch bits per token (<= 128 bits)
    int *scan = (int *)(pbits + Tp16);                            // SRC: [4] wave totals, [16] games of this workgroup's next leaves

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    int nvalid, my_first = 0, my_count = 0, my_lo = 0, my_per = 0;
    if (SRC) {
        // exclusive prefix of the leaf flags over the workgroup's 256 threads (thread t owns games [t per, (t+1) per))
        my_per = ((((a.src.n_games + 255) >> 8) + 7) >> 3) << 3;
        my_lo = tid * my_per;
        for (int w = 0; w < my_per; w += 8)
            if (my_lo + w < a.src.flag_bytes) {
                const unsigned long long f = *(const unsigned long long *)(a.src.leaf_flag + my_lo + w);
                my_count += __popcll((((f & 0x7f7f7f7f7f7f7f7full) + 0x7f7f7f7f7f7f7f7full) | f) & 0x8080808080808080ull);   // non-zero flag bytes
            }
        int incl = my_count;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) { const int v = __shfl_up(incl, off); if (lane >= off) incl += v; }
        if (lane == 63) scan[wave] = incl;
        __syncthreads();
        int before = 0;
        for (int w = 0; w < wave; w++) before += scan[w];
        my_first = before + incl - my_count;
        nvalid = scan[0] + scan[1] + scan[2] + scan[3];
        if (blockIdx.x == 0 && tid == 0) { *a.src.n_leaf = nvalid; if (a.src.cache_stamp) *a.src.cache_stamp += 1u; }
        __syncthreads();
    } else {
        nvalid = a.count ? min(a.n, *a.count) : a.n;
    }
    if ((int)blockIdx.x >= nvalid) return;

    // this wave's weight fragments (its 8 column tiles + the extra tile) live in registers for the whole kernel: 9 * KS * 4
    // VGPRs instead of 9 * KS LDS reads per token tile.  Fragment (tile, s) of lane l = wt[col(tile, l)][32 s + 8 (l>>4) .. +8]
    union BF { uint4 u; bf16x8 v; };
    BF bw[8][KS], be[KS];
#pragma unroll
    for (int q = 0; q < 8; q++)
#pragma unroll
        for (int s = 0; s < KS; s++) bw[q][s].u = *(const uint4 *)(a.wt + (size_t)(128 * wave + 8 * l15 + q) * KP + 32 * s + 8 * l4);
#pragma unroll
    for (int s = 0; s < KS; s++) be[s].u = *(const uint4 *)(a.wt + (size_t)(D + l15) * KP + 32 * s + 8 * l4);
    {
        unsigned r[4];
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = (((tid >> (2 * i)) & 1) ? 0x3F80u : 0u) | (((tid >> (2 * i + 1)) & 1) ? 0x3F800000u : 0u);
        alut[tid] = make_uint4(r[0], r[1], r[2], r[3]);
    }
    __syncthreads();

    const int RC = a.R * a.Cc, T = a.T, ksz = a.ksz, kk = ksz * ksz, pad = ksz / 2, ncell = a.C * RC;
    const int tiles = (T + 15) >> 4;
    const float msum = a.msum[l15];
    const float sref = STATIC_REF ? a.sref[l15] : 0.f;
    const bool headlane = l15 < NH;
    const f32x4 *cbase = (const f32x4 *)a.cpos + (size_t)wave * 8 * 64 + lane;
    const f32x4 *mbase = (const f32x4 *)a.mtab + lane;
    int par = 0;

    for (int leaf0 = blockIdx.x; leaf0 < nvalid; leaf0 += 16 * gridDim.x) {
      if (SRC) {
          // the games behind this workgroup's next (up to 16) leaves, resolved in one pass: the thread whose flag range holds
          // the leaf-th flagged game finds it, records its slot for the next expansion and posts the game index
          __syncthreads();
          for (int k = 0; k < 16; k++) {
              const int lf = leaf0 + k * (int)gridDim.x;
              if (lf >= nvalid) break;
              if (lf >= my_first && lf < my_first + my_count) {
                  int kk = lf - my_first, g = my_lo;
                  for (int w = 0; w < my_per; w++) {
                      const int f = a.src.leaf_flag[my_lo + w];
                      if (f && kk-- == 0) { g = my_lo + w; break; }
                  }
                  scan[4 + k] = g;
                  a.src.leaf_slot[g] = lf;
              }
          }
          __syncthreads();
      }
      for (int k16 = 0; k16 < 16; k16++) {
        const int leaf = leaf0 + k16 * (int)gridDim.x;
        if (leaf >= nvalid) break;
        int game = 0, player = 0;
        if (SRC) {
            game = scan[4 + k16];
            player = (a.src.to_move[game] + a.src.leaf_depth[game]) & 1;     // node.currentPlayer at the leaf
        }
        unsigned wbits = 0;                             // lane i holds bits [32 (i-1), 32 i) of the board bit string (lane 0: zeros)
        for (int q = 0; q * 64 < ncell; q++) {
            const int e = q * 64 + lane;
            bool on = false;
            if (SRC) {
                if (e < ncell) {                                     // canonical planes from the cell codes (gomoku.py:34-40; 3-plane: mcts.py:126-137)
                    const int ch = (e >= RC) + (e >= 2 * RC), cell = e - ch * RC;
                    const int code = a.src.leaf_cells[(size_t)game * a.src.rc_pad + cell];
                    on = ch == 2 ? player != 0 : ((code >> (ch ^ player)) & 1) != 0;
                }
            } else if (e < ncell)
                on = a.boards_f32 ? ((const float *)a.boards)[(size_t)leaf * ncell + e] != 0.0f
                                  : (((const unsigned short *)a.boards)[(size_t)leaf * ncell + e] & 0x7fff) != 0;
            const unsigned long long m = __ballot(on);
            if ((lane - 1) >> 1 == q && lane >= 1) wbits = ((lane - 1) & 1) ? (unsigned)(m >> 32) : (unsigned)m;
        }
        // ---- patch bits of every token, once per board: token = wave * 64 + lane (+ 256 per round) ----
        for (int t0 = 0; t0 < tiles * 16; t0 += 256) {
            const int t = t0 + wave * 64 + lane;
            unsigned long long plo = 0, phi = 0;
            const int j = t - 1, r = j / a.Cc, c = j - r * a.Cc;
            const bool live = t >= 1 && t < T;
            unsigned colmask = 0;
            for (int kx = 0; kx < ksz; kx++) { const int cc = c + kx - pad; if (cc >= 0 && cc < a.Cc) colmask |= 1u << kx; }
            for (int ch = 0; ch < a.C; ch++)
                for (int ky = 0; ky < ksz; ky++) {
                    const int rr = r + ky - pad;
                    // every lane takes part in the shuffles; dead rows contribute zero bits
                    int off = 32 + ch * RC + (rr < 0 ? 0 : (rr >= a.R ? a.R - 1 : rr)) * a.Cc + (c - pad);
                    if (!live) off = 32;
                    const int wi = off >> 5, sh = off & 31;
                    const unsigned lo = __shfl(wbits, wi), hi = __shfl(wbits, wi + 1);
                    unsigned bits = __funnelshift_r(lo, hi, sh) & colmask;
                    if (!live || rr < 0 || rr >= a.R) bits = 0;
                    const int p0 = ch * kk + ky * ksz;
                    if (p0 < 64) { plo |= (unsigned long long)bits << p0; if (p0 + ksz > 64) phi |= (unsigned long long)bits >> (64 - p0); }
                    else phi |= (unsigned long long)bits << (p0 - 64);
                }
            if (t < tiles * 16) pbits[t] = make_uint4((unsigned)plo, (unsigned)(plo >> 32), (unsigned)phi, (unsigned)(phi >> 32));
        }
        __syncthreads();
        f32x4 Z[8];
#pragma unroll
        for (int q = 0; q < 8; q++) Z[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        float M = -INFINITY, L = 0.f;                   // per head (lane&15 < NH); L is this lane>>4 group's share

        const f32x4 *cp = cbase;
        const f32x4 *mp = mbase;
        for (int tile = 0; tile < tiles; tile++, cp += 4 * 8 * 64, mp += 64) {
            // ---- accumulators: rows 4 (lane>>4) + r4, columns 128 wave + 8 (lane&15) + q; the constants are stored in
            //      this very order, so each accumulator is one 16-byte load, 1 KB contiguous per wave ----
            f32x4 acc[8], acce = *mp;
#pragma unroll
            for (int q = 0; q < 8; q++) acc[q] = cp[q * 64];
            // ---- A fragments: 8 patch bits of this lane's token (row lane&15) per k-step -> table ----
            const uint4 pb = pbits[tile * 16 + l15];
            const unsigned pw[4] = {pb.x, pb.y, pb.z, pb.w};
            bf16x8 afrag[KS];
#pragma unroll
            for (int s = 0; s < KS; s++) {
                union { uint4 u; bf16x8 v; } af;
                af.u = alut[(pw[s] >> (8 * l4)) & 0xffu];
                afrag[s] = af.v;
            }
#pragma unroll
            for (int s = 0; s < KS; s++) acce = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[s], be[s].v, acce, 0, 0, 0);
#pragma unroll
            for (int s = 0; s < KS; s++)
#pragma unroll
                for (int q = 0; q < 8; q++) acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[s], bw[q][s].v, acc[q], 0, 0, 0);
            // ---- LayerNorm statistics of the full rows.  The mean is GEMM column 15 of the extra tile; only the sum of
            //      squares needs this wave's 128 columns -> LDS -> all four waves ----
            float mean[4];
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) mean[r4] = __shfl(acce[r4], (lane & 48) | 15);
            f32x2 q01 = {0.f, 0.f}, q23 = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x2 lo = {acc[q][0], acc[q][1]}, hi = {acc[q][2], acc[q][3]};
                q01 = __builtin_elementwise_fma(lo, lo, q01);
                q23 = __builtin_elementwise_fma(hi, hi, q23);
            }
            // the row pairs (0,1) and (2,3) travel as float2 from here on: every step below works on adjacent register pairs
            // (packed-math operands), nothing has to be shuffled into place
            const f32x2 pq01 = {row16_sum(q01[0]), row16_sum(q01[1])}, pq23 = {row16_sum(q23[0]), row16_sum(q23[1])};
            f32x2 *part2 = (f32x2 *)part;                             // [parity][8 row pairs][4 waves]
            if (l15 == 0) {
                part2[(par * 8 + 2 * l4) * 4 + wave] = pq01;
                part2[(par * 8 + 2 * l4 + 1) * 4 + wave] = pq23;
            }
            __syncthreads();
            const f32x4 *pp = (const f32x4 *)(part2 + (par * 8 + 2 * l4) * 4);
            const f32x4 a0 = pp[0], a1 = pp[1], b0 = pp[2], b1 = pp[3];   // pair (0,1): waves 0,1 | 2,3; pair (2,3): likewise
            const f32x2 s01 = (f32x2{a0[0], a0[1]} + f32x2{a0[2], a0[3]}) + (f32x2{a1[0], a1[1]} + f32x2{a1[2], a1[3]});
            const f32x2 s23 = (f32x2{b0[0], b0[1]} + f32x2{b0[2], b0[3]}) + (f32x2{b1[0], b1[1]} + f32x2{b1[2], b1[3]});
            const f32x2 mean01 = {mean[0], mean[1]}, mean23 = {mean[2], mean[3]};
            const f32x2 invD = {1.0f / (float)D, 1.0f / (float)D};
            const f32x2 v01 = __builtin_elementwise_fma(-mean01, mean01, s01 * invD), v23 = __builtin_elementwise_fma(-mean23, mean23, s23 * invD);
            const f32x2 r01 = {__builtin_amdgcn_rsqf(fmaxf(v01[0], 0.f) + a.eps), __builtin_amdgcn_rsqf(fmaxf(v01[1], 0.f) + a.eps)};
            const f32x2 r23 = {__builtin_amdgcn_rsqf(fmaxf(v23[0], 0.f) + a.eps), __builtin_amdgcn_rsqf(fmaxf(v23[1], 0.f) + a.eps)};
            const f32x2 h01 = -mean01 * r01, h23 = -mean23 * r23;    // xn = x * rstd + shift
            par ^= 1;
            // ---- scores (head = lane&15, tokens 4 (lane>>4) + r4) and softmax weights; lanes >= NH carry harmless finite
            //      values into rows of Z that are never stored ----
            const f32x2 ms2 = {msum, msum};
            const f32x2 sc01 = r01 * __builtin_elementwise_fma(-mean01, ms2, f32x2{acce[0], acce[1]});
            const f32x2 sc23 = r23 * __builtin_elementwise_fma(-mean23, ms2, f32x2{acce[2], acce[3]});
            const float sc[4] = {sc01[0], sc01[1], sc23[0], sc23[1]};
            float w[4];
            if (STATIC_REF) {
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) w[r4] = __expf(sc[r4] - sref);
            } else {
                float tmax = fmaxf(fmaxf(sc[0], sc[1]), fmaxf(sc[2], sc[3]));
                tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
                tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
                const float Mn = fmaxf(M, tmax);
                const float f = __expf(M - Mn);                       // M = -inf on the first tile: f = 0 (Z and L are 0)
#pragma unroll
                for (int r4 = 0; r4 < 4; r4++) w[r4] = __expf(sc[r4] - Mn);
                L *= f;
                M = Mn;
                if (__ballot(headlane && f != 1.0f) != 0ull) {        // some head's running maximum moved: rescale its Z rows
                    float fr[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) fr[j] = l4 < 2 ? __shfl(f, 4 * l4 + j) : 1.0f;   // rows of Z = heads 4 (lane>>4) + j
#pragma unroll
                    for (int q = 0; q < 8; q++)
#pragma unroll
                        for (int j = 0; j < 4; j++) Z[q][j] *= fr[j];
                }
            }
            L += (w[0] + w[1]) + (w[2] + w[3]);
            // ---- Z += W^T Xn : A = weights (bf16), B = normalised tile (bf16), both already in operand layout ----
            const s16x4 wa = pack4_bf16(f32x2{w[0], w[1]}, f32x2{w[2], w[3]});
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x2 lo = {acc[q][0], acc[q][1]}, hi = {acc[q][2], acc[q][3]};
                const f32x2 vlo = __builtin_elementwise_fma(lo, r01, h01), vhi = __builtin_elementwise_fma(hi, r23, h23);   // (x - mean) * rstd
                Z[q] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(wa, pack4_bf16(vlo, vhi), Z[q], 0, 0, 0);
            }
        }
        // ---- z[b][h][:] = Z[h][:] / L[h] ----
        float Lt = L + __shfl_xor(L, 16);
        Lt += __shfl_xor(Lt, 32);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int head = 4 * l4 + j;
            const float Lh = __shfl(Lt, head & 15);
            if (head < NH) {
                const float inv = 1.0f / Lh;
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; q++) v[q] = Z[q][j] * inv;
                *(uint4 *)(a.z + ((size_t)leaf * NH + head) * D + 128 * wave + 8 * l15) = pack8(v);
            }
        }
      }
    }
}

template <int KS, int NH, bool SR, bool SRC>
int launch_embed_pool2(const EmbedPoolArgs &a, hipStream_t st) {
    const int lds = 256 * 16 + 512 + ((a.T + 15) / 16) * 16 * 16 + 96;
    if (azk_set_max_lds((const void *)k_embed_pool<KS, NH, SR, SRC>, lds) != hipSuccess) return AZK_ERR_HIP;
    const int blocks = a.n < 512 ? a.n : 512;                      // two resident workgroups per CU, each walks its boards
    k_embed_pool<KS, NH, SR, SRC><<<blocks, 256, lds, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

template <int KS, int NH>
int launch_embed_pool(const EmbedPoolArgs &a, hipStream_t st) {
    if (a.src.leaf_flag) return a.sref ? launch_embed_pool2<KS, NH, true, true>(a, st) : launch_embed_pool2<KS, NH, false, true>(a, st);
    return a.sref ? launch_embed_pool2<KS, NH, true, false>(a, st) : launch_embed_pool2<KS, NH, false, false>(a, st);
}
}  // namespace

static int32_t embed_pool_impl(const void *boards_dev, int32_t boards_are_f32, const azk_leaf_source *src, const void *wt_ext_bf16_dev,
                               const float *cpos_frag_dev, const float *score_frag_dev, const float *score_msum_dev,
                               const float *score_ref_dev, void *z_out_bf16_dev, int32_t num_heads, int32_t n, int32_t channels,
                               int32_t rows, int32_t cols, int32_t ksize, int32_t kp, int32_t embed_dim, float ln_eps,
                               const int32_t *n_valid_dev, void *stream) {
    if ((!boards_dev && !src) || !wt_ext_bf16_dev || !cpos_frag_dev || !score_frag_dev || !score_msum_dev || !z_out_bf16_dev) return AZK_ERR_ARG;
    if (n < 0 || channels < 1 || rows < 1 || cols < 1 || ksize < 1 || (ksize & 1) == 0 || ksize > 7) return AZK_ERR_ARG;
    if (kp < channels * ksize * ksize || kp % 32 != 0 || kp > 96) return AZK_ERR_ARG;
    if (channels * rows * cols > 62 * 32 || embed_dim != 512) return AZK_ERR_ARG;      // one column group per wave, four waves
    if (num_heads != 8 && num_heads != 4) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    EmbedPoolArgs a;
    memset(&a, 0, sizeof a);
    a.boards = boards_dev; a.boards_f32 = boards_are_f32; a.wt = (const __hip_bfloat16 *)wt_ext_bf16_dev; a.cpos = cpos_frag_dev;
    a.mtab = score_frag_dev; a.msum = score_msum_dev; a.sref = score_ref_dev; a.z = (__hip_bfloat16 *)z_out_bf16_dev;
    a.count = n_valid_dev;
    a.n = n; a.C = channels; a.R = rows; a.Cc = cols; a.ksz = ksize; a.T = rows * cols + 1; a.eps = ln_eps;
    if (src) a.src = *src;
    hipStream_t st = (hipStream_t)stream;
    const int ks = kp / 32;
#define CASE(KS_, NH_) if (ks == KS_ && num_heads == NH_) return launch_embed_pool<KS_, NH_>(a, st)
    CASE(2, 8); CASE(1, 8); CASE(3, 8); CASE(2, 4); CASE(1, 4); CASE(3, 4);
#undef CASE
    return AZK_ERR_ARG;
}

extern "C" int32_t azk_nn_embed_pool(const void *boards_dev, int32_t boards_are_f32, const void *wt_ext_bf16_dev,
                                     const float *cpos_frag_dev, const float *score_frag_dev, const float *score_msum_dev,
                                     const float *score_ref_dev, void *z_out_bf16_dev, int32_t num_heads, int32_t n,
                                     int32_t channels, int32_t rows, int32_t cols, int32_t ksize, int32_t kp, int32_t embed_dim,
                                     float ln_eps, const int32_t *n_valid_dev, void *stream) {
    if (!boards_dev) return AZK_ERR_ARG;
    return embed_pool_impl(boards_dev, boards_are_f32, nullptr, wt_ext_bf16_dev, cpos_frag_dev, score_frag_dev, score_msum_dev,
                           score_ref_dev, z_out_bf16_dev, num_heads, n, channels, rows, cols, ksize, kp, embed_dim, ln_eps, n_valid_dev, stream);
}

extern "C" int32_t azk_nn_embed_pool_leaves(const azk_leaf_source *src, const void *wt_ext_bf16_dev, const float *cpos_frag_dev,
                                            const float *score_frag_dev, const float *score_msum_dev, const float *score_ref_dev,
                                            void *z_out_bf16_dev, int32_t num_heads, int32_t ksize, int32_t kp, int32_t embed_dim,
                                            float ln_eps, void *stream) {
    if (!src || !src->leaf_flag || !src->leaf_cells || !src->to_move || !src->leaf_depth || !src->leaf_slot || !src->n_leaf) return AZK_ERR_ARG;
    if (src->n_games < 1 || src->rows * src->cols != src->rc || src->flag_bytes < src->n_games) return AZK_ERR_ARG;
    return embed_pool_impl(nullptr, 0, src, wt_ext_bf16_dev, cpos_frag_dev, score_frag_dev, score_msum_dev, score_ref_dev,
                           z_out_bf16_dev, num_heads, src->n_games, src->planes, src->rows, src->cols, ksize, kp, embed_dim, ln_eps, nullptr, stream);
}

// =====================================================================================================
// k_embed_pool_c: k_embed_pool that only computes the tokens a stone can reach.
//   A token whose k x k patch holds no stone is a constant of the weights: x_t = cpos[t], so its normalised row xn_t, its
//   head scores and - with the static softmax reference - its weights w_t[h] = exp(s_t[h] - ref[h]) do not depend on the
//   board.  With  ZALL[h] = sum_t wc_t[h] xnc_t  and  LALL[h] = sum_t wc_t[h]  over ALL tokens taken as empty-patch tokens,
//       Z[h] = ZALL[h] + sum_{t dirty} (w_t[h] xn_t - wc_t[h] xnc_t),     L[h] = LALL[h] + sum_{t dirty} (w_t[h] - wc_t[h])
//   exactly (the softmax reference is the same constant on both sides).  On a 15x15 board with ~20 stones ~100 of the 226
//   tokens are dirty: 7 sixteen-token tiles instead of 15.  Per board: patch bits of all tokens (one per thread), the
//   dirty ones compacted through LDS (ballot + prefix), then the tile loop of k_embed_pool over the compacted list with
//   the per-token constants GATHERED by token index ([token][...] tables, L2 resident); the subtraction rides on the same
//   MFMA: v_mfma_f32_16x16x32_bf16 with k-slots 0..3 of a lane group = its four tokens (A: w, B: xn) and k-slots 4..7 = the
//   same tokens as constants (A: -wc, B: xnc).
//   Scheduling: a workgroup's first board is blockIdx.x; further boards come from a device-side queue head (one atomic per
//   board, issued behind the first tile's loads so its round trip hides under the tile), because boards now differ in
//   cost.  Exactly n_valid tickets are drawn per launch (every workgroup with a board draws until one fails), so the
//   workgroup holding ticket n_valid - 1 knows the queue is finished and leaves the counter zero for the next launch.
// =====================================================================================================
namespace {

struct EmbedPoolCArgs {
    const void *boards;
    int boards_f32;
    const void *wt_frag;           // conv weight (+ the 16 extra columns) in MFMA fragment order [33][KS][64] x 16 bytes
    const float *cposT;            // [T + 1][D]   bias + positional term per token; row T (the null token) = 0
    const float *scoreT;           // [T + 1][16]  score constants per token (column 15: row mean); row T: -1e30 in the head columns
    const float *wcT;              // [T + 1][16]  softmax weight of the token taken as an empty-patch token; row T = 0
    const __hip_bfloat16 *xncT;    // [T + 1][D]   normalised empty-patch token (bf16); row T = 0
    const float *zall;             // accumulator order [4 waves][8][64 lanes][4]: ZALL[head 4 (lane>>4) + j][128 w + 8 (lane&15) + q]
    const float *lall;             // [16]
    const float *msum, *sref;      // [16]
    __hip_bfloat16 *z;             // [n][NH][D]
    const int *count;
    int *sched;                    // [1]: ticket counter of the board queue; zero between launches
    long long *dbg;                // debug only (AZK_EMBED_POOL_STAMPS): [8] cycle sums per phase, wave 0 of every workgroup
    unsigned long long *wstats;    // optional [2]: boards evaluated, 16-token tiles evaluated (fire-and-forget atomics, one pair per board)
    int n, R, Cc, T;
    float eps;
    azk_leaf_source src;
};

template <int NC, int KSZ, int NH, bool SRC>
__global__ __launch_bounds__(256, 2) void k_embed_pool_c(EmbedPoolCArgs a) {
    constexpr int KS = (NC * KSZ * KSZ + 31) / 32;
    constexpr int D = 512, KP = 32 * KS;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4 *alut = (uint4 *)smem;                                  // [256] A fragment of 8 patch bits
    float *part = (float *)(alut + 256);                          // [2 parities][16 rows][4 waves] partial sums of squares
    const int Tp16 = ((a.T + 15) >> 4) << 4;
    uint4 *pbits = (uint4 *)(part + 128);                         // [Tp16] patch bits of the compacted dirty tokens
    int *dlist = (int *)(pbits + Tp16);                           // [Tp16] their token indices (null token = T past the end)
    int *scan = dlist + Tp16;                                     // [4] SRC wave totals, [4] dirty counts per wave, [8] next board, [9] game
    uint4 *rankv = (uint4 *)(scan + 32);                          // SRC: [256 threads] ranks of the thread's first eight games, 16 bits each (scan[16..31]: class totals of the four waves)
    uint4 *bimg = rankv + (SRC ? 256 : 0);                        // [33 column tiles][KS][64 lanes] weight B fragments                           // [33 column tiles][KS][64 lanes] weight B fragments (the wave's 8 tiles + the extra one)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    // SRC: a non-zero leaf flag is 1 + the leaf's cost class (0..7, by stone count).  Board j of the launch is the j-th flagged
    // game in the order (class descending, game index ascending): the stone-heavy boards - the ones with the most tokens to
    // evaluate - are handed out first, the light ones fill the gaps at the end (longest-processing-time-first; the queue is
    // dynamic).  Every workgroup derives the same ranks: per-class counts of its threads' games (thread t owns games
    // [t per, (t+1) per)), an exclusive scan over the 256 threads with the eight 16-bit counters packed in two 64-bit words.
    int nvalid, my_lo = 0, my_per = 0;
    unsigned long long cb_lo = 0ull, cb_hi = 0ull;                // rank of this thread's first game of each class, 16 bits each (classes 0-3 / 4-7)
    // The launch's fixed cost is a chain of round trips (leaf flags -> ranks -> weights -> first board): the flag words and the
    // whole conv weight image (wt_frag, MFMA fragment order [33 column tiles][KS][64 lanes] x 16 bytes: fragment (tile, s) of lane l
    // = wt[col(tile, l)][32 s + 8 (l>>4) .. +8], column tile 32 = the extra columns) are requested together, the flags first so
    // that the rank arithmetic waits for them alone; the image goes to LDS once the ranks are done.
    constexpr int NF = 33 * KS * 64, PER = (NF + 255) / 256;
    unsigned long long myflags = 0ull;
    if (SRC) {
        my_per = ((((a.src.n_games + 255) >> 8) + 7) >> 3) << 3;
        my_lo = tid * my_per;
        if (my_lo < a.src.flag_bytes) myflags = *(const unsigned long long *)(a.src.leaf_flag + my_lo);
    }
    // (LDS-DMA: a wave instruction moves 64 x 16 contiguous bytes, no registers; NF is a multiple of 64, whole wave pieces only)
    static_assert(NF % 64 == 0, "the weight image is copied in whole 1 KiB wave pieces");
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (256 * i + 64 * wave < NF)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)((const uint4 *)a.wt_frag + tid + 256 * i),
                                             (__attribute__((address_space(3))) void *)(bimg + 256 * i + 64 * wave), 16, 0, 0);
    if (SRC) {
        unsigned long long c_lo = 0ull, c_hi = 0ull;              // classes 0-3 / 4-7, 16 bits each
        for (int w = 0; w < my_per; w += 8)
            if (my_lo + w < a.src.flag_bytes) {
                const unsigned long long f = w == 0 ? myflags : *(const unsigned long long *)(a.src.leaf_flag + my_lo + w);
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const unsigned c = (unsigned)((f >> (8 * q)) & 0xffull);
                    if (c) { if (c <= 4) c_lo += 1ull << (16 * (c - 1)); else c_hi += 1ull << (16 * (c - 5)); }
                }
            }
        unsigned long long i_lo = c_lo, i_hi = c_hi;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned long long v_lo = __shfl_up(i_lo, off), v_hi = __shfl_up(i_hi, off);
            if (lane >= off) { i_lo += v_lo; i_hi += v_hi; }
        }
        unsigned long long *wtot = (unsigned long long *)(scan + 16);           // [4 waves][2]
        if (lane == 63) { wtot[2 * wave] = i_lo; wtot[2 * wave + 1] = i_hi; }
        __syncthreads();
        unsigned long long b_lo = 0ull, b_hi = 0ull, t_lo = 0ull, t_hi = 0ull;
        for (int w = 0; w < 4; w++) {
            if (w < wave) { b_lo += wtot[2 * w]; b_hi += wtot[2 * w + 1]; }
            t_lo += wtot[2 * w]; t_hi += wtot[2 * w + 1];
        }
        const unsigned long long e_lo = b_lo + i_lo - c_lo, e_hi = b_hi + i_hi - c_hi;   // exclusive prefix over lower threads, per class
        unsigned start = 0;
#pragma unroll
        for (int c = 7; c >= 0; c--) {                            // class 7 (most stones) first
            const unsigned tot = (unsigned)(((c < 4 ? t_lo : t_hi) >> (16 * (c & 3))) & 0xffffull);
            const unsigned long long cb = (unsigned long long)(start + (unsigned)(((c < 4 ? e_lo : e_hi) >> (16 * (c & 3))) & 0xffffull)) << (16 * (c & 3));
            if (c < 4) cb_lo |= cb; else cb_hi |= cb;
            start += tot;
        }
        nvalid = (int)start;
        unsigned run = 0;                                         // games of each class seen so far in this thread: 4 bits each
        unsigned myrank[4] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};   // 0xffff: no game
#pragma unroll
        for (int q = 0; q < 8; q++) {
            const unsigned c = (unsigned)((myflags >> (8 * q)) & 0xffull);
            unsigned r = 0xffffu;
            if (c) {
                const unsigned bsel = (unsigned)(((c <= 4 ? cb_lo : cb_hi) >> (16 * ((c - 1) & 3))) & 0xffffull);
                r = bsel + ((run >> (4 * (c - 1))) & 0xfu);
                run += 1u << (4 * (c - 1));
            }
            myrank[q >> 1] = (q & 1) ? ((myrank[q >> 1] & 0x0000ffffu) | (r << 16)) : ((myrank[q >> 1] & 0xffff0000u) | r);
        }
        rankv[tid] = make_uint4(myrank[0], myrank[1], myrank[2], myrank[3]);      // read back by the same thread only
        if (blockIdx.x == 0 && tid == 0) { *a.src.n_leaf = nvalid; if (a.src.cache_stamp) *a.src.cache_stamp += 1u; }
    } else {
        nvalid = a.count ? min(a.n, *a.count) : a.n;
    }
    int board = blockIdx.x;
#ifdef AZK_EP_STAMPS          // diagnosis build only (make EXTRA=-DAZK_EP_STAMPS): the stamps cost registers, the product kernel has none
    const bool stamp = a.dbg != nullptr && tid == 0;
    long long tp = stamp ? clock64() : 0, tacc[5] = {0, 0, 0, 0, 0}, nt_acc = 0, nb_acc = 0;     // sums stay in registers until the end
#define AZK_STAMP(i) do { if (stamp) { const long long tn_ = clock64(); tacc[i] += tn_ - tp; tp = tn_; } } while (0)
#else
    constexpr bool stamp = false;
    long long nt_acc = 0, nb_acc = 0;
#define AZK_STAMP(i) do { } while (0)
#endif
    int ws_boards = 0, ws_tiles = 0;
    if (board >= nvalid) __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0): no LDS-DMA may outlive the workgroup
    if (board < nvalid) {                                         // (workgroups without a board go straight to the sign-off below)
    union BF { uint4 u; bf16x8 v; };
    const uint4 *bwv = bimg + (size_t)wave * 8 * KS * 64 + lane, *bev = bimg + (size_t)32 * KS * 64 + lane;
    {
        unsigned r[4];
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = (((tid >> (2 * i)) & 1) ? 0x3F80u : 0u) | (((tid >> (2 * i + 1)) & 1) ? 0x3F800000u : 0u);
        alut[tid] = make_uint4(r[0], r[1], r[2], r[3]);
    }
    constexpr int ksz = KSZ, kk = KSZ * KSZ, pad = KSZ / 2;
    const int RC = a.R * a.Cc, T = a.T, ncell = NC * RC;
    const float msum = a.msum[l15], sref = a.sref[l15], lall = a.lall[l15];
    const int colofs = 128 * wave + 8 * l15;
    int par = 0, nxt = 0;
    __syncthreads();
    AZK_STAMP(0);                                                 // prologue: weights staged

    while (board < nvalid) {
        // Everything below that depends only on the thread index (where the token's patch rows sit in the board bit string, the
        // cell each lane fetches, the cross-lane read addresses) is recomputed per board from an opaque copy of the index: left
        // to the compiler these ~60 values are hoisted out of the board loop, live through the tile loop, and the spills they
        // cause are reloaded between the board's loads - one memory round trip per reload.
        int tv = tid;
        asm volatile("" : "+v"(tv));
        const int lane_b = tv & 63;
        const int tj = tv - 1, tr = tj / a.Cc, tc = tj - tr * a.Cc;
        const bool tlive = tv >= 1 && tv < T;
        unsigned colmask = 0;
#pragma unroll
        for (int kx = 0; kx < ksz; kx++) { const int cc = tc + kx - pad; if (cc >= 0 && cc < a.Cc) colmask |= 1u << kx; }
        int game = 0, player = 0;
        if (SRC) {
            // the game behind board `board`: the thread that owns the game with that rank posts it and records the slot the next
            // expansion reads (its first eight games' ranks sit in registers; engines with more than 2048 slots walk the rest)
            int g = -1;
            const uint4 rk = rankv[tid];
            const unsigned myrank[4] = {rk.x, rk.y, rk.z, rk.w};
#pragma unroll
            for (int q = 0; q < 8; q++) if (((myrank[q >> 1] >> (16 * (q & 1))) & 0xffffu) == (unsigned)board) g = my_lo + q;
            if (my_per > 8) {
                unsigned long long run2 = 0ull;                    // games of each class seen so far: 8 bits each
                for (int w = 0; w < my_per; w++) {
                    const unsigned c = my_lo + w < a.src.flag_bytes ? (unsigned)a.src.leaf_flag[my_lo + w] : 0u;
                    if (!c) continue;
                    const unsigned r = (unsigned)(((c <= 4 ? cb_lo : cb_hi) >> (16 * ((c - 1) & 3))) & 0xffffull) + (unsigned)((run2 >> (8 * (c - 1))) & 0xffull);
                    run2 += 1ull << (8 * (c - 1));
                    if (w >= 8 && r == (unsigned)board) g = my_lo + w;
                }
            }
            if (g >= 0) { scan[9] = g; a.src.leaf_slot[g] = board; }
            __syncthreads();
            game = scan[9];
        }
        // the workgroup's Z starts at the constant part (fetched here, under the board's own loads)
        f32x4 Z[8];
        if (l4 < (NH + 3) / 4) {
            const f32x4 *zp = (const f32x4 *)a.zall + (size_t)wave * 8 * 64 + lane;
#pragma unroll
            for (int q = 0; q < 8; q++) Z[q] = zp[q * 64];
        } else {
#pragma unroll
            for (int q = 0; q < 8; q++) Z[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        unsigned wbits = 0;                             // lane i holds bits [32 (i-1), 32 i) of the board bit string (lane 0: zeros)
        constexpr int NQ = 8;                           // boards of up to 512 plane cells: every load of the board in ONE round trip
        if (ncell <= 64 * NQ) {
            bool on[NQ];
            if (SRC) {
                // canonical planes from the cell codes (gomoku.py:34-40; 3-plane: mcts.py:126-137); the code loads do not
                // depend on the side to move, so they travel together with the two words that give it
                int code[NQ], chq[NQ];
                const auto *cells = a.src.leaf_cells + (size_t)game * a.src.rc_pad;       // uniform base + 32-bit lane offsets
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const int e = min(q * 64 + lane_b, ncell - 1);
                    chq[q] = (e >= RC) + (e >= 2 * RC);
                    code[q] = cells[(unsigned)(e - chq[q] * RC)];
                }
                player = (a.src.to_move[game] + a.src.leaf_depth[game]) & 1;     // node.currentPlayer at the leaf
#pragma unroll
                for (int q = 0; q < NQ; q++)
                    on[q] = q * 64 + lane_b < ncell && (chq[q] == 2 ? player != 0 : ((code[q] >> (chq[q] ^ player)) & 1) != 0);
            } else if (a.boards_f32) {
                float raw[NQ];
                const float *bp32 = (const float *)a.boards + (size_t)board * ncell;
#pragma unroll
                for (int q = 0; q < NQ; q++) raw[q] = bp32[(unsigned)min(q * 64 + lane_b, ncell - 1)];
#pragma unroll
                for (int q = 0; q < NQ; q++) on[q] = q * 64 + lane_b < ncell && raw[q] != 0.0f;
            } else {
                unsigned short raw[NQ];
                const unsigned short *bp16 = (const unsigned short *)a.boards + (size_t)board * ncell;
#pragma unroll
                for (int q = 0; q < NQ; q++) raw[q] = bp16[(unsigned)min(q * 64 + lane_b, ncell - 1)];
#pragma unroll
                for (int q = 0; q < NQ; q++) on[q] = q * 64 + lane_b < ncell && (raw[q] & 0x7fff) != 0;
            }
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const unsigned long long m = __ballot(on[q]);
                if ((lane_b - 1) >> 1 == q && lane_b >= 1) wbits = ((lane_b - 1) & 1) ? (unsigned)(m >> 32) : (unsigned)m;
            }
        } else {
            if (SRC) player = (a.src.to_move[game] + a.src.leaf_depth[game]) & 1;
            for (int q = 0; q * 64 < ncell; q++) {
                const int e = q * 64 + lane;
                bool on = false;
                if (SRC) {
                    if (e < ncell) {
                        const int ch = (e >= RC) + (e >= 2 * RC), cell = e - ch * RC;
                        const int code = a.src.leaf_cells[(size_t)game * a.src.rc_pad + cell];
                        on = ch == 2 ? player != 0 : ((code >> (ch ^ player)) & 1) != 0;
                    }
                } else if (e < ncell)
                    on = a.boards_f32 ? ((const float *)a.boards)[(size_t)board * ncell + e] != 0.0f
                                      : (((const unsigned short *)a.boards)[(size_t)board * ncell + e] & 0x7fff) != 0;
                const unsigned long long m = __ballot(on);
                if ((lane - 1) >> 1 == q && lane >= 1) wbits = ((lane - 1) & 1) ? (unsigned)(m >> 32) : (unsigned)m;
            }
        }
        AZK_STAMP(1);                                             // board resolved, loaded, bit string built
        // ---- patch bits of this thread's token; dirty = some stone in the patch ----
        unsigned long long plo = 0, phi = 0;
        {
            // compile-time trip counts: all 2 NC KSZ cross-lane reads of the bit string are issued together
            unsigned lo[NC * KSZ], hi[NC * KSZ];
#pragma unroll
            for (int ch = 0; ch < NC; ch++)
#pragma unroll
                for (int ky = 0; ky < KSZ; ky++) {
                    const int rr = tr + ky - pad;
                    int off = 32 + ch * RC + (rr < 0 ? 0 : (rr >= a.R ? a.R - 1 : rr)) * a.Cc + (tc - pad);
                    if (!tlive) off = 32;
                    lo[ch * KSZ + ky] = __shfl(wbits, off >> 5); hi[ch * KSZ + ky] = __shfl(wbits, (off >> 5) + 1);
                }
#pragma unroll
            for (int ch = 0; ch < NC; ch++)
#pragma unroll
                for (int ky = 0; ky < KSZ; ky++) {
                    const int rr = tr + ky - pad;
                    int off = 32 + ch * RC + (rr < 0 ? 0 : (rr >= a.R ? a.R - 1 : rr)) * a.Cc + (tc - pad);
                    if (!tlive) off = 32;
                    unsigned bits = __funnelshift_r(lo[ch * KSZ + ky], hi[ch * KSZ + ky], off & 31) & colmask;
                    if (!tlive || rr < 0 || rr >= a.R) bits = 0;
                    constexpr int dummy = 0; (void)dummy;
                    const int p0 = ch * kk + ky * ksz;
                    if (p0 < 64) { plo |= (unsigned long long)bits << p0; if (p0 + ksz > 64) phi |= (unsigned long long)bits >> (64 - p0); }
                    else phi |= (unsigned long long)bits << (p0 - 64);
                }
        }
        const bool dirty = (plo | phi) != 0ull;
        const unsigned long long dm = __ballot(dirty);
        if (lane == 0) scan[4 + wave] = __popcll(dm);
        __syncthreads();                                  // (also: every wave is done with the previous board's lists)
        int dpos = __popcll(dm & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) dpos += scan[4 + w];
        const int nd = scan[4] + scan[5] + scan[6] + scan[7];
        const int ntile = (nd + 15) >> 4;
        if (dirty) {
            dlist[dpos] = tid;
            pbits[dpos] = make_uint4((unsigned)plo, (unsigned)(plo >> 32), (unsigned)phi, (unsigned)(phi >> 32));
        }
        if (tid < 16 && nd + tid < ntile * 16) { dlist[nd + tid] = T; pbits[nd + tid] = make_uint4(0u, 0u, 0u, 0u); }   // null tokens fill the last tile
        __syncthreads();

        AZK_STAMP(2);                                             // patch bits + compaction
        if (stamp) nt_acc += ntile;
        ws_boards += 1; ws_tiles += ntile;                  // (uniform; one pair of atomics per workgroup at the very end: an atomic here sits in
                                                            //  the vmcnt queue in front of the tile's gathers, which wait for it - measured +7 us per launch)
        float L = 0.f;                                    // per head (lane&15 < NH): this lane>>4 group's share of sum (w - wc)
        // The per-token constants are GATHERED (by token index, L2) and every tile would wait a full round trip for them, so they
        // run one phase ahead: the conv MFMAs start from zero and the constants are added behind them; the registers they leave
        // are refilled with the NEXT tile's constants before the statistics / pooling phase, and the constant rows of the pooling
        // (needed last) are refetched right behind their use.  Same registers, the round trip under the other phase's arithmetic.
        f32x4 c0[4], c1[4], scn, wcn;
        uint4 xr[4];
        auto gather_a = [&](int t) {
            const int4 tk = *(const int4 *)(dlist + 16 * t + 4 * l4);
            const int tks[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
            for (int r = 0; r < 4; r++) {
                // 32-bit BYTE offsets from the (uniform) table bases: the loads take the base from SGPRs, one VGPR per token and table
                const unsigned orow = ((unsigned)tks[r] * (unsigned)D + (unsigned)colofs) * 4u, osc = ((unsigned)tks[r] * 16u + (unsigned)l15) * 4u;
                c0[r] = *(const f32x4 *)((const char *)a.cposT + orow); c1[r] = *(const f32x4 *)((const char *)a.cposT + orow + 16);
                scn[r] = *(const float *)((const char *)a.scoreT + osc);
                wcn[r] = *(const float *)((const char *)a.wcT + osc);
            }
        };
        auto gather_x = [&](int t) {
            const int4 tk = *(const int4 *)(dlist + 16 * t + 4 * l4);
            const int tks[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
            for (int r = 0; r < 4; r++) xr[r] = *(const uint4 *)((const char *)a.xncT + ((unsigned)tks[r] * (unsigned)D + (unsigned)colofs) * 2u);
        };
        if (ntile > 0) { gather_a(0); gather_x(0); }
        for (int tile = 0; tile < ntile; tile++) {
            if (tile == 0 && tid == 0) {                  // next board: the round trip hides under this tile
                __builtin_amdgcn_sched_barrier(0);
                nxt = atomicAdd(a.sched, 1);
                __builtin_amdgcn_sched_barrier(0);
            }
            // ---- A fragments: 8 patch bits of this lane's token (row lane&15) per k-step -> table ----
            const uint4 pb = pbits[tile * 16 + l15];
            const unsigned pw[4] = {pb.x, pb.y, pb.z, pb.w};
            bf16x8 afrag[KS];
#pragma unroll
            for (int s = 0; s < KS; s++) {
                union { uint4 u; bf16x8 v; } af;
                af.u = alut[(pw[s] >> (8 * l4)) & 0xffu];
                afrag[s] = af.v;
            }
            f32x4 acc[8];
            f32x4 acce = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 8; q++) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};
            // k-step outermost: nine independent accumulator chains per step, the B fragments stream from LDS
#pragma unroll
            for (int s = 0; s < KS; s++) {
                { BF b; b.u = bev[s * 64]; acce = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[s], b.v, acce, 0, 0, 0); }
#pragma unroll
                for (int q = 0; q < 8; q++) { BF b; b.u = bwv[(q * KS + s) * 64]; acc[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afrag[s], b.v, acc[q], 0, 0, 0); }
                if (s + 1 < KS) __builtin_amdgcn_sched_barrier(0);    // one k-step's fragments in flight at a time (VGPR budget)
            }
            // ---- the gathered constants (bias + positional term, score constants), then the next tile's gathers into their registers ----
#pragma unroll
            for (int r = 0; r < 4; r++) {
                acc[0][r] += c0[r][0]; acc[1][r] += c0[r][1]; acc[2][r] += c0[r][2]; acc[3][r] += c0[r][3];
                acc[4][r] += c1[r][0]; acc[5][r] += c1[r][1]; acc[6][r] += c1[r][2]; acc[7][r] += c1[r][3];
            }
            acce += scn;
            const f32x4 wc = wcn;
            __builtin_amdgcn_sched_barrier(0);
            const int tnext = min(tile + 1, ntile - 1);          // (the last tile refetches itself: no branch around loads)
            gather_a(tnext);
            __builtin_amdgcn_sched_barrier(0);
            // ---- LayerNorm statistics of the full rows (mean = GEMM column 15 of the extra tile) ----
            float mean[4];
#pragma unroll
            for (int r4 = 0; r4 < 4; r4++) mean[r4] = __shfl(acce[r4], (lane & 48) | 15);
            f32x2 q01 = {0.f, 0.f}, q23 = {0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x2 lo = {acc[q][0], acc[q][1]}, hi = {acc[q][2], acc[q][3]};
                q01 = __builtin_elementwise_fma(lo, lo, q01);
                q23 = __builtin_elementwise_fma(hi, hi, q23);
            }
            const f32x2 pq01 = {row16_sum(q01[0]), row16_sum(q01[1])}, pq23 = {row16_sum(q23[0]), row16_sum(q23[1])};
            f32x2 *part2 = (f32x2 *)part;                             // [parity][8 row pairs][4 waves]
            if (l15 == 0) {
                part2[(par * 8 + 2 * l4) * 4 + wave] = pq01;
                part2[(par * 8 + 2 * l4 + 1) * 4 + wave] = pq23;
            }
            __syncthreads();
            const f32x4 *pp = (const f32x4 *)(part2 + (par * 8 + 2 * l4) * 4);
            const f32x4 a0 = pp[0], a1 = pp[1], b0 = pp[2], b1 = pp[3];
            const f32x2 s01 = (f32x2{a0[0], a0[1]} + f32x2{a0[2], a0[3]}) + (f32x2{a1[0], a1[1]} + f32x2{a1[2], a1[3]});
            const f32x2 s23 = (f32x2{b0[0], b0[1]} + f32x2{b0[2], b0[3]}) + (f32x2{b1[0], b1[1]} + f32x2{b1[2], b1[3]});
            const f32x2 mean01 = {mean[0], mean[1]}, mean23 = {mean[2], mean[3]};
            const f32x2 invD = {1.0f / (float)D, 1.0f / (float)D};
            const f32x2 v01 = __builtin_elementwise_fma(-mean01, mean01, s01 * invD), v23 = __builtin_elementwise_fma(-mean23, mean23, s23 * invD);
            const f32x2 r01 = {__builtin_amdgcn_rsqf(fmaxf(v01[0], 0.f) + a.eps), __builtin_amdgcn_rsqf(fmaxf(v01[1], 0.f) + a.eps)};
            const f32x2 r23 = {__builtin_amdgcn_rsqf(fmaxf(v23[0], 0.f) + a.eps), __builtin_amdgcn_rsqf(fmaxf(v23[1], 0.f) + a.eps)};
            const f32x2 h01 = -mean01 * r01, h23 = -mean23 * r23;    // xn = x * rstd + shift
            par ^= 1;
            // ---- scores (head = lane&15, tokens = rows) and softmax weights against the static reference ----
            const f32x2 ms2 = {msum, msum};
            const f32x2 sc01 = r01 * __builtin_elementwise_fma(-mean01, ms2, f32x2{acce[0], acce[1]});
            const f32x2 sc23 = r23 * __builtin_elementwise_fma(-mean23, ms2, f32x2{acce[2], acce[3]});
            float w[4];
            w[0] = __expf(sc01[0] - sref); w[1] = __expf(sc01[1] - sref); w[2] = __expf(sc23[0] - sref); w[3] = __expf(sc23[1] - sref);
            L += ((w[0] - wc[0]) + (w[1] - wc[1])) + ((w[2] - wc[2]) + (w[3] - wc[3]));
            // ---- Z += W^T Xn - Wc^T Xnc as ONE 16x16x32 MFMA per column: k-slots 0..3 actual, 4..7 constant ----
            union { bf16x8 v; s16x4 h[2]; } wa;
            wa.h[0] = pack4_bf16(f32x2{w[0], w[1]}, f32x2{w[2], w[3]});
            wa.h[1] = pack4_bf16(f32x2{-wc[0], -wc[1]}, f32x2{-wc[2], -wc[3]});
            const unsigned xw[4][4] = {{xr[0].x, xr[0].y, xr[0].z, xr[0].w}, {xr[1].x, xr[1].y, xr[1].z, xr[1].w},
                                       {xr[2].x, xr[2].y, xr[2].z, xr[2].w}, {xr[3].x, xr[3].y, xr[3].z, xr[3].w}};
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const f32x2 lo = {acc[q][0], acc[q][1]}, hi = {acc[q][2], acc[q][3]};
                const f32x2 vlo = __builtin_elementwise_fma(lo, r01, h01), vhi = __builtin_elementwise_fma(hi, r23, h23);   // (x - mean) * rstd
                union { bf16x8 v; struct { s16x4 h; unsigned c01, c23; } p; } xb;
                xb.p.h = pack4_bf16(vlo, vhi);
                const unsigned sel = (q & 1) ? 0x07060302u : 0x05040100u;                  // bf16 element q of each token's 16-byte row
                xb.p.c01 = __builtin_amdgcn_perm(xw[1][q >> 1], xw[0][q >> 1], sel);
                xb.p.c23 = __builtin_amdgcn_perm(xw[3][q >> 1], xw[2][q >> 1], sel);
                Z[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa.v, xb.v, Z[q], 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            gather_x(tnext);
        }
        AZK_STAMP(3);                                             // tile loop
        if (ntile == 0 && tid == 0) nxt = atomicAdd(a.sched, 1);
        // ---- z[b][h][:] = (ZALL + Z)[h][:] / (LALL + L)[h] ----
        float Lt = L + __shfl_xor(L, 16);
        Lt += __shfl_xor(Lt, 32);
        Lt += lall;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int head = 4 * l4 + j;
            const float Lh = __shfl(Lt, head & 15);
            if (head < NH) {
                const float inv = 1.0f / Lh;
                float v[8];
#pragma unroll
                for (int q = 0; q < 8; q++) v[q] = Z[q][j] * inv;
                *(uint4 *)(a.z + ((size_t)board * NH + head) * D + colofs) = pack8(v);
            }
        }
        if (tid == 0) {
            // every workgroup that got a board draws tickets until one fails, so exactly nvalid tickets are drawn per launch:
            // whoever holds the last one (nvalid - 1) knows the queue is finished for this launch and leaves it zero
            if (nxt == nvalid - 1) a.sched[0] = 0;
            scan[8] = (int)gridDim.x + nxt;
        }
        __syncthreads();
        board = scan[8];
        AZK_STAMP(4);                                             // epilogue + next board known
        if (stamp) nb_acc += 1;
    }
    }
    if (a.wstats != nullptr && tid == 0 && ws_boards) { atomicAdd(a.wstats, (unsigned long long)ws_boards); atomicAdd(a.wstats + 1, (unsigned long long)ws_tiles); }
#undef AZK_STAMP
#ifdef AZK_EP_STAMPS
    if (stamp) {
        const long long wg_total = tacc[0] + tacc[1] + tacc[2] + tacc[3] + tacc[4];
        atomicMax((unsigned long long *)a.dbg + 5, (unsigned long long)wg_total);       // the busiest workgroup of any launch
        for (int i = 0; i < 5; i++) atomicAdd((unsigned long long *)a.dbg + i, (unsigned long long)tacc[i]);
        atomicAdd((unsigned long long *)a.dbg + 6, (unsigned long long)nt_acc);
        atomicAdd((unsigned long long *)a.dbg + 7, (unsigned long long)nb_acc);
    }
#endif
    (void)nt_acc; (void)nb_acc;
}

template <int NC, int KSZ, int NH, bool SRC>
int launch_embed_pool_c2(const EmbedPoolCArgs &a, hipStream_t st) {
    constexpr int KS = (NC * KSZ * KSZ + 31) / 32;
    const int tp16 = ((a.T + 15) / 16) * 16;
    const int lds = 256 * 16 + 512 + tp16 * 16 + tp16 * 4 + 128 + (SRC ? 256 * 16 : 0) + 33 * KS * 64 * 16;      // 77 KB at KS = 2: two workgroups per CU
    if (azk_set_max_lds((const void *)k_embed_pool_c<NC, KSZ, NH, SRC>, lds) != hipSuccess) return AZK_ERR_HIP;
    const int blocks = a.n < 512 ? a.n : 512;                      // two resident workgroups per CU; each pulls boards until the queue is dry
    k_embed_pool_c<NC, KSZ, NH, SRC><<<blocks, 256, lds, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}
}  // namespace

static int32_t embed_pool_c_impl(const void *boards_dev, int32_t boards_are_f32, const azk_leaf_source *src, const azk_embed_pool_consts *k,
                                 void *z_out_bf16_dev, int32_t n, int32_t channels, int32_t rows, int32_t cols,
                                 const int32_t *n_valid_dev, int32_t *sched_dev, void *stream) {
    if ((!boards_dev && !src) || !k || !z_out_bf16_dev || !sched_dev) return AZK_ERR_ARG;
    if (!k->wt_frag || !k->cpos_tok || !k->score_tok || !k->wconst_tok || !k->xnconst_tok || !k->z_all || !k->l_all || !k->score_msum || !k->score_ref) return AZK_ERR_ARG;
    const int ksize = k->ksize, kp = k->kp;
    if (n < 0 || channels < 1 || rows < 1 || cols < 1 || ksize < 1 || (ksize & 1) == 0 || ksize > 7) return AZK_ERR_ARG;
    if (kp < channels * ksize * ksize || kp % 32 != 0 || kp > 96) return AZK_ERR_ARG;
    if (channels * rows * cols > 62 * 32 || k->embed_dim != 512) return AZK_ERR_ARG;
    if (rows * cols + 1 > 256) return AZK_ERR_ARG;                 // one thread per token
    if (k->num_heads != 8 && k->num_heads != 4) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    EmbedPoolCArgs a;
    memset(&a, 0, sizeof a);
    a.boards = boards_dev; a.boards_f32 = boards_are_f32; a.wt_frag = k->wt_frag; a.cposT = k->cpos_tok;
    a.scoreT = k->score_tok; a.wcT = k->wconst_tok; a.xncT = (const __hip_bfloat16 *)k->xnconst_tok; a.zall = k->z_all; a.lall = k->l_all;
    a.msum = k->score_msum; a.sref = k->score_ref; a.z = (__hip_bfloat16 *)z_out_bf16_dev; a.count = n_valid_dev; a.sched = sched_dev;
    a.wstats = (unsigned long long *)k->work_stats;
    a.n = n; a.R = rows; a.Cc = cols; a.T = rows * cols + 1; a.eps = k->ln_eps;
    if (src) a.src = *src;
    {
        static long long *dbg_buf = nullptr;
        const char *ds = getenv("AZK_EMBED_POOL_STAMPS");
        if (ds && atoi(ds)) {
            if (!dbg_buf && (hipMalloc((void **)&dbg_buf, 64) != hipSuccess || hipMemset(dbg_buf, 0, 64) != hipSuccess)) return AZK_ERR_HIP;
            a.dbg = dbg_buf;
            if (atoi(ds) == 2) {          // print-and-reset request
                long long h[8];
                if (hipMemcpy(h, dbg_buf, 64, hipMemcpyDeviceToHost) != hipSuccess) return AZK_ERR_HIP;
                fprintf(stderr, "[embed_pool_c stamps] busiest workgroup %lld cycles | ", h[5]);
                fprintf(stderr, "[embed_pool_c stamps] boards %lld tiles %lld | cycles per board: prologue(total) %lld, load %.0f, patch+compact %.0f, tiles %.0f (%.0f per tile), epilogue %.0f\n",
                        h[7], h[6], h[0], (double)h[1] / (double)(h[7] ? h[7] : 1), (double)h[2] / (double)(h[7] ? h[7] : 1), (double)h[3] / (double)(h[7] ? h[7] : 1),
                        (double)h[3] / (double)(h[6] ? h[6] : 1), (double)h[4] / (double)(h[7] ? h[7] : 1));
                if (hipMemset(dbg_buf, 0, 64) != hipSuccess) return AZK_ERR_HIP;
            }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int nh = k->num_heads;
    if (kp != (channels * ksize * ksize + 31) / 32 * 32) return AZK_ERR_ARG;
#define CASE(NC_, KSZ_, NH_) if (channels == NC_ && ksize == KSZ_ && nh == NH_) \
        return src ? launch_embed_pool_c2<NC_, KSZ_, NH_, true>(a, st) : launch_embed_pool_c2<NC_, KSZ_, NH_, false>(a, st)
    CASE(2, 5, 8); CASE(2, 5, 4); CASE(3, 5, 8); CASE(3, 5, 4); CASE(2, 3, 8); CASE(2, 3, 4); CASE(3, 3, 8); CASE(3, 3, 4);
#undef CASE
    return AZK_ERR_ARG;
}

extern "C" int32_t azk_nn_embed_pool_compact(const void *boards_dev, int32_t boards_are_f32, const azk_embed_pool_consts *consts,
                                             void *z_out_bf16_dev, int32_t n, int32_t channels, int32_t rows, int32_t cols,
                                             const int32_t *n_valid_dev, int32_t *sched_dev, void *stream) {
    if (!boards_dev) return AZK_ERR_ARG;
    return embed_pool_c_impl(boards_dev, boards_are_f32, nullptr, consts, z_out_bf16_dev, n, channels, rows, cols, n_valid_dev, sched_dev, stream);
}

extern "C" int32_t azk_nn_embed_pool_compact_leaves(const azk_leaf_source *src, const azk_embed_pool_consts *consts, void *z_out_bf16_dev,
                                                    int32_t *sched_dev, void *stream) {
    if (!src || !src->leaf_flag || !src->leaf_cells || !src->to_move || !src->leaf_depth || !src->leaf_slot || !src->n_leaf) return AZK_ERR_ARG;
    if (src->n_games < 1 || src->rows * src->cols != src->rc || src->flag_bytes < src->n_games) return AZK_ERR_ARG;
    // the leaf ranks travel as 16-bit per-class counters with 0xffff = "no game" (and 8-bit per-thread run counters): more pending-leaf
    // slots than this would wrap them silently - refuse, the caller keeps azk_nn_embed_pool_leaves / azk_step_gather for such engines
    if (src->n_games > AZK_EMBED_POOL_COMPACT_MAX_SLOTS) return AZK_ERR_ARG;
    return embed_pool_c_impl(nullptr, 0, src, consts, z_out_bf16_dev, src->n_games, src->planes, src->rows, src->cols, nullptr, sched_dev, stream);
}
