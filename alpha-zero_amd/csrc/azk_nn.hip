// azk_nn.hip - the headline bf16 evaluator of a depth-1 network, hand-written for gfx950: k_embed_fold (boards -> the folded cls rows
// [n][H][384] without forming a token; entry points azk_nn_embed_fold*, azk_nnx_embed_fold* for its float32-accurate EX form) and
// k_tail_gemm (the cls-row tail over those rows, azk_nn_tail_gemm).  Earlier generations: azk_embed_tok.hip, azk_embed_conv.hip,
// azk_rows.hip; shared device helpers: azk_nn_common.h; what k_tail_gemm shares with azk_tail.hip: azk_tail_common.h.
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
#include "azk_tail_common.h"

// =====================================================================================================
// k_embed_fold: embedding + cls pooling without the token rows (include/azk.h azk_nn_embed_fold; pvnet.PolicyValueNet.fold_u).
//   x_t = Wc p_t + cpos_t with p_t the token's 0/1 patch, so LayerNorm1's variance is a quadratic form of <= 64 bits, the cls scores
//   are linear in them, and the value-projected pooled row u_h = (1/L_h) sum_t a_t[h] (M_h p_t + D_t[h]) is linear in x_t: what a
//   board contributes is, per head, one weight per token, 1/L, and the pooled patch sum_t a_t p_t / L - 384 bf16 per head, which the
//   tail's first GEMM multiplies with [D_t; U_all; M_h].  No conv, no D-wide normalisation, no gather of D-wide rows.
//   Board hand-out, leaf ranks, board bits, patch bits and the compaction of the stone-touched ("dirty") tokens do what the front end of
//   k_embed_pool_c (azk_embed_conv.hip) and k_embed_pool_x (azk_nnx.hip) does, in a copy that is tuned apart on purpose: the rank scan
//   runs on DPP (no shuffles), the ranks are inverted once into an LDS table (gor: game of rank r) instead of searched per board, and
//   the next board - known from a fixed schedule, no queue - has its cell codes prefetched behind the last tile (load_cells).
//   Tile loop: a WAVE owns 16-token tiles (tile = wave, wave + 4, ...), nothing between the waves until the board's sums meet:
//     Y = P G (16 x 64, fp16 hi + lo terms: exact products with the 0/1 patch), E = P S (scores), both v_mfma_f32_16x16x32_f16;
//     var_t = (sum_k p_tk (Y_tk + u2_tk) + n_t) / D from the accumulator layout (DPP row sum); w = exp(rstd (E + sc) - ref);
//     a = w rstd; b = a - aconst to LDS; pooled patch: Pw[h][k] += a_t[h] p_tk on v_mfma_f32_16x16x32_bf16 with k-slots 0..3 of a
//     lane group = its four tokens' a as bf16 hi, slots 4..7 = the bf16 remainder (B: the patch bits twice).
//   Board end: L and Pw of the four waves meet in LDS, every thread scales ITS token's eight weights by 1 / L into the output image
//   (LDS, bf16), the pooled patch and the three 1/L slots follow, the image leaves with 16-byte stores.
// =====================================================================================================
namespace {
using namespace azk_nn;

struct EmbedFoldArgs {
    const void *boards;
    int boards_f32;
    const uint4 *gfrag;            // [2 (hi, lo)][4][2][64]
    const uint4 *efrag;            // [2][2][64]
    const float *u2T, *scoreT, *wcT, *lall, *sref, *inv_scales;
    void *out;                     // [n][NH][FOLD_ROW] bf16 (EX: float32)
    const int *count;
    int *sched;                    // two zero words of the caller's: the boards are handed out by a fixed schedule, the kernel touches neither
    unsigned long long *wstats;
    long long *dbg;                // debug only (AZK_EP_STAMPS build + AZK_EMBED_POOL_STAMPS): [8] cycle sums per phase, wave 0 of every workgroup
    int n, R, Cc, T;
    int rdivR, rdivC;              // 65536 / R + 1, 65536 / Cc + 1: x / d = (x m) >> 16 for x < 256, d <= 64
    float eps;
    azk_leaf_source src;
    int cwmax;                     // leaf boards by dword (embed_fold_impl decides): index of a row's last cell dword, -1 = the source does not qualify
};

constexpr int FOLD_ROW = AZK_EMBED_FOLD_ROW;
constexpr int FOLD_MAX_SLOTS = AZK_EMBED_FOLD_MAX_SLOTS;

// EX: the float32-accurate form (azk_nnx_embed_fold, the fp32 line): correctly rounded rsqrt, exp with an extended-precision argument, the
// pooled patch on v_mfma_f32_16x16x4_f32 (float32 weights against the 0 / 1 patch: exact products), float32 rows out (1 / L in one slot).
template <int NC, int KSZ, int NH, bool SRC, bool EX>
__global__ __launch_bounds__(256, 2) void k_embed_fold(EmbedFoldArgs a) {
    static_assert(NC * KSZ * KSZ <= 64, "the patch is one 64-bit word");
    constexpr int D = 512;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint4 *alut = (uint4 *)smem;                                  // [256] A fragment (fp16 0 / 1) of 8 patch bits
    const int Tp16 = ((a.T + 15) >> 4) << 4;
    uint2 *pbits = (uint2 *)(alut + 256);                         // [Tp16] patch bits of the compacted dirty tokens
    int *dlist = (int *)(pbits + Tp16);                           // [Tp16] their token indices (null token = T past the end)
    int *scan = dlist + Tp16;                                     // [4 dirty counts per wave at 4..7], [16..31] class totals of the rank scan
    float *lred = (float *)(scan + 32);                           // [4 waves][8 heads]
    float *lall_s = lred + 32;                                    // [8] l_all
    float *bw = lall_s + 8;                                       // [Tp16][8]  a - aconst per dirty token and head
    float *pwred = bw + Tp16 * 8;                                 // [4 waves][8 heads][64]
    unsigned short *gor = (unsigned short *)(pwred + 4 * 8 * 64); // SRC: [n_games] game of rank r (= of the launch's r-th board)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l15 = lane & 15, l4 = lane >> 4;
    int nvalid;
    // the quadratic form's and the score columns' B fragments live in registers for the whole launch (80 VGPRs, 20 KB per wave once).
    // Measured against keeping them in LDS (154 VGPRs: three workgroups per CU, or two tiles per wave at a time): 86.5 vs 92.4 / 90.1 ms
    // per move - every MFMA then waits for its ds_read.
    uint4 gfr[16], efr[4];
#pragma unroll
    for (int i = 0; i < 16; i++) gfr[i] = a.gfrag[i * 64 + lane];
#pragma unroll
    for (int i = 0; i < 4; i++) efr[i] = a.efrag[i * 64 + lane];
    if (SRC) {
        // A non-zero leaf flag is 1 + the leaf's cost class (0..7, by stone count).  Board r of the launch is the r-th flagged game in
        // the order (class descending, game ascending): the stone-heavy boards are handed out first, the light ones fill the gaps at
        // the end.  Every workgroup derives the same ranks - per-class counts of its threads' games (thread t owns games [t per, (t+1)
        // per)), an exclusive scan over the 256 threads - and keeps the inverse (game of rank r) in LDS: a board's game is then one LDS
        // read, whoever asks.  All of it in 32-bit arithmetic without a branch per flag: the eight counts of one 8-byte flag word are at
        // most 8 and sit in the 4-bit fields of one dword; they are widened to 16-bit fields (two classes a dword) only where counts of
        // many games meet - the thread's total, the wave scan, the class bases.  A thread's first flag word (all of its flags up to
        // 2 048 games) is read once and kept for the second pass; the further words of larger engines are read again there.
        const int my_per = ((((a.src.n_games + 255) >> 8) + 7) >> 3) << 3, my_lo = tid * my_per;
        auto flag_word = [&](const int w) {                       // flags [my_lo + w, my_lo + w + 8), zero past the end
            const bool in = my_lo + w < a.src.flag_bytes;
            const uint2 f = *(const uint2 *)(a.src.leaf_flag + (in ? my_lo + w : 0));
            return make_uint2(in ? f.x : 0u, in ? f.y : 0u);
        };
        const uint2 fw0 = flag_word(0);
        auto flag_of = [](const uint2 f, const int q) { return ((q < 4 ? f.x : f.y) >> (8 * (q & 3))) & 0xffu; };
        auto widen = [](const unsigned c4, const int q) { return ((c4 >> (8 * q)) & 0xfu) | (((c4 >> (8 * q + 4)) & 0xfu) << 16); };   // classes 2q, 2q + 1
        unsigned cw[4] = {0u, 0u, 0u, 0u};                        // this thread's games per class, 16 bits each
#pragma unroll 1
        for (int w = 0; w < my_per; w += 8) {
            const uint2 f = w ? flag_word(w) : fw0;
            unsigned c4 = 0u;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const unsigned c = flag_of(f, q);
                c4 += min(c, 1u) << ((4u * c - 4u) & 31u);
            }
#pragma unroll
            for (int q = 0; q < 4; q++) cw[q] += widen(c4, q);
        }
        // inclusive wave scan of the packed 16-bit counters on DPP (row_shr 1, 2, 4, 8, then row_bcast 15 / 31: six dependent v_add per
        // dword instead of six ds_bpermute round trips).  The fields never carry into each other (a count is at most the slot count,
        // < 65536), so the four dwords scan - and add, and subtract - independently.
        unsigned iw[4];
#pragma unroll
        for (int q = 0; q < 4; q++) {
            int v = (int)cw[q];
            v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, true);
            v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, true);
            v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, true);
            v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, true);
            v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);
            v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);
            iw[q] = (unsigned)v;
        }
        unsigned *wtot = (unsigned *)(scan + 16);                 // [4 waves][4]
        if (lane == 63) *(uint4 *)(wtot + 4 * wave) = make_uint4(iw[0], iw[1], iw[2], iw[3]);
        __syncthreads();
        unsigned ew[4], tw[4];                                    // exclusive prefix over lower threads / total, per class
#pragma unroll
        for (int q = 0; q < 4; q++) { ew[q] = iw[q] - cw[q]; tw[q] = 0u; }
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint4 t = *(const uint4 *)(wtot + 4 * w);
            const unsigned tq[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
            for (int q = 0; q < 4; q++) { ew[q] += w < wave ? tq[q] : 0u; tw[q] += tq[q]; }
        }
        unsigned cb[4] = {0u, 0u, 0u, 0u};                        // rank of this thread's next game of each class, 16 bits each
        unsigned start = 0;
#pragma unroll
        for (int c = 7; c >= 0; c--) {                            // class 7 (most stones) first
            cb[c >> 1] |= (start + ((ew[c >> 1] >> (16 * (c & 1))) & 0xffffu)) << (16 * (c & 1));
            start += (tw[c >> 1] >> (16 * (c & 1))) & 0xffffu;
        }
        nvalid = (int)start;
        // second pass: a game's rank is its class's base + the games of that class the thread has met in this flag word (4-bit running
        // counts); the bases move on by the word's counts.  The thread's nine bases - entry 0 for "no leaf": 16 spare entries past the
        // table that nobody reads - lie in an LDS row of its own (pwred is idle until the first board's sums), so a flag costs one
        // LDS read and one LDS write and neither a select between the packed words nor a branch.
        typedef unsigned __attribute__((may_alias)) u32a;
        unsigned short *brow = (unsigned short *)pwred + 10 * tid;
        const unsigned spare = (unsigned)(((a.src.n_games + 7) >> 3) << 3);
#pragma unroll 1
        for (int w = 0; w < my_per; w += 8) {
            const uint2 f = w ? flag_word(w) : fw0;
            u32a *br = (u32a *)brow;
            br[0] = spare | (cb[0] << 16); br[1] = (cb[0] >> 16) | (cb[1] << 16); br[2] = (cb[1] >> 16) | (cb[2] << 16);
            br[3] = (cb[2] >> 16) | (cb[3] << 16); br[4] = cb[3] >> 16;
            unsigned base[8], run4 = 0u;
#pragma unroll
            for (int q = 0; q < 8; q++) base[q] = brow[flag_of(f, q)];   // (all eight reads in flight before the first write)
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const unsigned c = flag_of(f, q), sh4 = (4u * c - 4u) & 31u;
                gor[base[q] + ((run4 >> sh4) & 0xfu)] = (unsigned short)(my_lo + w + q);
                run4 += min(c, 1u) << sh4;
            }
#pragma unroll
            for (int q = 0; q < 4; q++) cb[q] += widen(run4, q);
        }
        if (blockIdx.x == 0 && tid == 0) { *a.src.n_leaf = nvalid; if (a.src.cache_stamp) *a.src.cache_stamp += 1u; }
    } else {
        nvalid = a.count ? min(a.n, *a.count) : a.n;
    }
    int board = blockIdx.x;
    int ws_boards = 0, ws_tiles = 0;
#ifdef AZK_EP_STAMPS
    const bool stamp = a.dbg != nullptr && tid == 0;
    long long tp = stamp ? clock64() : 0, tacc[5] = {0, 0, 0, 0, 0};
#define AZK_FSTAMP(i) do { if (stamp) { const long long tn_ = clock64(); tacc[i] += tn_ - tp; tp = tn_; } } while (0)
#else
#define AZK_FSTAMP(i) do { } while (0)
#endif
    if (board < nvalid) {
    {
        unsigned r[4];
#pragma unroll
        for (int i = 0; i < 4; i++) r[i] = (((tid >> (2 * i)) & 1) ? 0x3C00u : 0u) | (((tid >> (2 * i + 1)) & 1) ? 0x3C000000u : 0u);
        alut[tid] = make_uint4(r[0], r[1], r[2], r[3]);
    }
    constexpr int ksz = KSZ, kk = KSZ * KSZ, pad = KSZ / 2;
    const int RC = a.R * a.Cc, T = a.T, ncell = NC * RC;
    const float sref = a.sref[l15];
    if (tid < 8) lall_s[tid] = a.lall[tid];
    const float invD = 1.0f / (float)D, ginv = a.inv_scales[0], einv = a.inv_scales[1];
    __syncthreads();
    AZK_FSTAMP(0);                                                // launch prologue: ranks, fragments staged

    // Boards of up to 512 plane cells: every load of a board is issued at once (one round trip), and the NEXT board's loads are issued
    // behind the wave's last tile - in front of the sums' barrier and the output phase - so a board starts with its cells on hand.
    constexpr int NQ = 8;
    // Leaf boards of two planes (CW) take their fast path by dword: rows of leaf_cells are whole dwords, four cells each (the engine writes
    // them so, azk_tree_step.h), and a board of the fold is at most 252 cells, so the board is ONE load per lane - lane l takes cells
    // 4 l .. 4 l + 3, the lanes past the row its last dword - held in codeN[0] across the previous board's output phase, and the bit string
    // is built from it without a ballot (below).  Whether a source qualifies is decided on the host (a.cwmax); one that does not - rows
    // that are no multiple of four bytes, a misaligned base - takes the general loop of the boards past the fast path.
    constexpr bool CW = SRC && NC == 2;
    const bool fast = CW ? a.cwmax >= 0 : ncell <= 64 * NQ;
    int codeN[NQ], tmN = 0, ldN = 0, game = 0;
    auto load_cells = [&](int g) {                                // SRC: cell codes (one byte per cell) + the two words that give the side to move
        const auto *cells = a.src.leaf_cells + (size_t)g * a.src.rc_pad;           // uniform base + 32-bit lane offsets
        int lv = tid;                                             // (opaque: the eight offsets are recomputed per call, not kept across the board loop)
        asm volatile("" : "+v"(lv));
        lv &= 63;
        if (CW) {
            codeN[0] = (int)((const unsigned *)cells)[(unsigned)min(lv, a.cwmax)];
        } else {
#pragma unroll
            for (int q = 0; q < NQ; q++) {
                const int e = min(q * 64 + lv, ncell - 1);
                codeN[q] = cells[(unsigned)(e - ((e >= RC) + (NC > 2 && e >= 2 * RC)) * RC)];
            }
        }
        tmN = a.src.to_move[g]; ldN = a.src.leaf_depth[g];
    };
    // (a board's rank is uniform and its game an LDS word every thread reads alike: taken to scalar registers, the row and cell
    //  addresses below are a scalar base + 32-bit lane offsets)
    if (SRC) { game = __builtin_amdgcn_readfirstlane((int)gor[board]); if (fast) load_cells(game); }

    while (board < nvalid) {
        // Everything below that depends only on the thread index is recomputed per board from an opaque copy of the index: hoisted out of
        // the board loop these values live through the tile loop and spill.
        int tv = tid;
        asm volatile("" : "+v"(tv));
        const int lane_b = tv & 63;
        const int tj = max(tv - 1, 0), tr = (tj * a.rdivC) >> 16, tc = tj - tr * a.Cc;   // (tj < 256, Cc <= 28: the product form of the division is exact)
        const bool tlive = tv >= 1 && tv < T;
        int player = 0;
        if (SRC && tid == 0) a.src.leaf_slot[game] = board;       // the slot the next expansion reads this game's outputs from
        unsigned wbits = 0;                             // lane i holds bits [32 (i-1), 32 i) of the board bit string (lane 0: zeros)
                                                        // (CW: lane 8 i + 4 ch + (0..3) holds bits [32 i, 32 i + 32) of plane ch's own bit string)
        if (CW && fast) {
            // canonical plane ch = bit ch ^ player of every code byte.  A lane's four bits of a plane meet in a nibble by one multiply
            // (bits 0, 8, 16, 24 times 2^24 + 2^17 + 2^10 + 2^3 land on bits 24..27, every cross term below bit 20 or past bit 31);
            // the eight nibbles of a lane group meet by three DPP steps.  Lanes 0..3 of a group keep plane 0 and hand plane 1 to lanes
            // 4..7 in the half-mirror step, and the other way round, so ONE register ends up holding both planes' strings.
            player = (tmN + ldN) & 1;
            const unsigned cw = (unsigned)codeN[0];
            const unsigned sk = ((unsigned)(lane_b >> 2) ^ (unsigned)player) & 1u, j4 = 4u * (unsigned)(lane_b & 7);
            const unsigned keep = ((((cw >> sk) & 0x01010101u) * 0x01020408u) >> 24) << j4;
            const unsigned send = ((((cw >> (sk ^ 1u)) & 0x01010101u) * 0x01020408u) >> 24) << j4;
            int v = (int)keep | __builtin_amdgcn_update_dpp(0, (int)send, 0x141, 0xF, 0xF, false);     // row_half_mirror: lane j of eight <-> 7 - j
            v |= __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false);                              // quad_perm [1, 0, 3, 2]
            v |= __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false);                              // quad_perm [2, 3, 0, 1]
            wbits = (unsigned)v;
        } else if (fast) {
            bool on[NQ];
            if (SRC) {
                // canonical planes from the cell codes (gomoku.py:34-40; 3-plane: mcts.py:126-137)
                player = (tmN + ldN) & 1;                         // node.currentPlayer at the leaf
#pragma unroll
                for (int q = 0; q < NQ; q++) {
                    const int e = min(q * 64 + lane_b, ncell - 1), chq = (e >= RC) + (NC > 2 && e >= 2 * RC);
                    on[q] = q * 64 + lane_b < ncell && (chq == 2 ? player != 0 : ((codeN[q] >> (chq ^ player)) & 1) != 0);
                }
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
        AZK_FSTAMP(1);                                            // board loaded, bit string built
        // ---- patch bits of this thread's token; dirty = some stone in the patch ----
        // Row words first: lane L < NC R holds plane L / R, row L % R of the board with two zero bits on either side (two cross-lane reads
        // of the bit string + a funnel shift, once); a token then takes its KSZ bits of each of its NC KSZ rows with ONE cross-lane read
        // and a shift - no column mask, the margins are zero.
        // Straight-line: every cross-lane read is issued before the first is used, the rows off the board and the threads without a token
        // take a zero mask (no branch between the reads), and the 64 patch bits are built as two 32-bit halves.
        unsigned plx = 0u, ply = 0u;
        {
            const int chL = (lane_b * a.rdivR) >> 16, rL = lane_b - chL * a.R;
            int offL = 32 + chL * RC + rL * a.Cc - 2, loA = (offL >> 5) << 2, hiA = loA + 4;
            if (CW && fast) {
                // the row's words straight from its plane's own string (word i of plane ch: lane 8 i + 4 ch).  Row 0 starts two bits in
                // front of the string and the last row may end in its last word: the words that do not exist come from whichever lane
                // the address wraps to, and the row mask below drops their bits - as it drops every cell at or past rc, so the
                // padding of a leaf_cells row never reaches a patch.
                offL = rL * a.Cc - 2;
                loA = ((offL >> 5) << 5) + (chL << 4); hiA = loA + 32;
            }
            const unsigned loL = (unsigned)__builtin_amdgcn_ds_bpermute(loA, (int)wbits);
            const unsigned hiL = (unsigned)__builtin_amdgcn_ds_bpermute(hiA, (int)wbits);
            const unsigned roww = lane_b < NC * a.R ? (__funnelshift_r(loL, hiL, offL & 31) & (((1u << a.Cc) - 1u) << 2)) : 0u;
            unsigned vm[KSZ];
            int src4[KSZ];
#pragma unroll
            for (int ky = 0; ky < KSZ; ky++) {
                const int rr = tr + ky - pad;
                vm[ky] = (tlive & ((unsigned)rr < (unsigned)a.R)) ? (1u << KSZ) - 1u : 0u;
                src4[ky] = min(max(rr, 0), a.R - 1) << 2;
            }
            unsigned rw[NC * KSZ];
#pragma unroll
            for (int ch = 0; ch < NC; ch++)
#pragma unroll
                for (int ky = 0; ky < KSZ; ky++) rw[ch * KSZ + ky] = (unsigned)__builtin_amdgcn_ds_bpermute(src4[ky] + 4 * ch * a.R, (int)roww);
            const unsigned sh = (unsigned)(tc + 2 - pad);
#pragma unroll
            for (int ch = 0; ch < NC; ch++)
#pragma unroll
                for (int ky = 0; ky < KSZ; ky++) {
                    const unsigned bits = (rw[ch * KSZ + ky] >> sh) & vm[ky];
                    const int p = ch * kk + ky * ksz;
                    if (p < 32) plx |= bits << p;
                    if (p >= 32) ply |= bits << (p & 31);
                    else if (p + KSZ > 32) ply |= bits >> (32 - p);
                }
        }
        const bool dirty = (plx | ply) != 0u;
        const unsigned long long dm = __ballot(dirty);
        if (lane == 0) scan[4 + wave] = __popcll(dm);
        __syncthreads();                                  // (also: every wave is done with the previous board's lists and sums)
        int dpos = __popcll(dm & ((1ull << lane) - 1ull));
        for (int w = 0; w < wave; w++) dpos += scan[4 + w];
        const int nd = scan[4] + scan[5] + scan[6] + scan[7];
        const int ntile = (nd + 15) >> 4;
        if (dirty) {
            dlist[dpos] = tid;
            pbits[dpos] = make_uint2(plx, ply);
        }
        if (tid < 16 && nd + tid < ntile * 16) { dlist[nd + tid] = T; pbits[nd + tid] = make_uint2(0u, 0u); }   // null tokens fill the last tile
        __syncthreads();
        ws_boards += 1; ws_tiles += ntile;
        AZK_FSTAMP(2);                                            // patch bits + compaction

        // ---- the wave's tiles: wave, wave + 4, ... ----
        float L = 0.f;                                    // per head (lane&15 < NH): this lane group's share of sum (w - wconst)
        f32x4 Pw[4];
#pragma unroll
        for (int q = 0; q < 4; q++) Pw[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        // the per-token constants are gathered (L2) one tile ahead: the round trip runs under the previous tile's arithmetic
        f32x4 utn[4];
        float scnn[4], wcnn[4], ntn[4], rcn[4];
        auto gather = [&](int t) {
            const int4 tk = *(const int4 *)(dlist + 16 * t + 4 * l4);
            const int tks[4] = {tk.x, tk.y, tk.z, tk.w};
#pragma unroll
            for (int r = 0; r < 4; r++) {
                // (the cross term u2_t . p_t is summed over the lane group like the quadratic form, but with ITS OWN column split: lane
                //  l15 takes columns 4 l15 .. 4 l15 + 3 - one 16-byte load per token instead of four 4-byte ones)
                const unsigned ou = ((unsigned)tks[r] * 64u + 4u * (unsigned)l15) * 4u, os = ((unsigned)tks[r] * 16u + (unsigned)l15) * 4u;
                utn[r] = *(const f32x4 *)((const char *)a.u2T + ou);
                scnn[r] = *(const float *)((const char *)a.scoreT + os);
                wcnn[r] = *(const float *)((const char *)a.wcT + os);
                // the token's n_t and constant rstd sit in column 15 of the same rows: loaded by every lane of the group (one line, a
                // tile ahead) instead of being broadcast from lane 15 through two ds_bpermute round trips on the tile's critical path
                ntn[r] = *(const float *)((const char *)a.scoreT + (unsigned)tks[r] * 64u + 60u);
                rcn[r] = *(const float *)((const char *)a.wcT + (unsigned)tks[r] * 64u + 60u);
            }
        };
        if (wave < ntile) gather(wave);
        for (int tile = wave; tile < ntile; tile += 4) {
            const int base = 16 * tile;
            // patch bits of this lane group's four tokens (rows 4 l4 + r)
            const int4 pq0 = *(const int4 *)(pbits + base + 4 * l4), pq1 = *(const int4 *)(pbits + base + 4 * l4 + 2);
            const unsigned prx[4] = {(unsigned)pq0.x, (unsigned)pq0.z, (unsigned)pq1.x, (unsigned)pq1.z};
            const unsigned pry[4] = {(unsigned)pq0.y, (unsigned)pq0.w, (unsigned)pq1.y, (unsigned)pq1.w};
            // the gathered rows are consumed at once (their registers take the next tile's): this lane's share of u2_t . p_t
            float cross[4], scn[4], wcn[4], ntv[4], rcv[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned nib = (l15 < 8 ? prx[r] : pry[r]) >> (4 * (l15 & 7));                   // patch bits 4 l15 .. 4 l15 + 3
                float c = 0.f;
#pragma unroll
                for (int cidx = 0; cidx < 4; cidx++) c = fmaf((float)((nib >> cidx) & 1u), utn[r][cidx], c);
                cross[r] = c; scn[r] = scnn[r]; wcn[r] = wcnn[r]; ntv[r] = ntn[r]; rcv[r] = rcn[r];
            }
            __builtin_amdgcn_sched_barrier(0);
            gather(tile + 4 < ntile ? tile + 4 : tile);          // (the last tile refetches itself: no branch around loads)
            __builtin_amdgcn_sched_barrier(0);
            const uint2 pa = pbits[base + l15];
            union { uint4 u; f16x8 v; } af[2];
            af[0].u = alut[(pa.x >> (8 * l4)) & 0xffu];
            af[1].u = alut[(pa.y >> (8 * l4)) & 0xffu];
            f32x4 Y[4], E = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < 4; q++) Y[q] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s2 = 0; s2 < 2; s2++) {
#pragma unroll
                for (int hl = 0; hl < 2; hl++) {
                    union { uint4 u; f16x8 v; } b;
                    b.u = efr[hl * 2 + s2];
                    E = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s2].v, b.v, E, 0, 0, 0);
                }
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int hl = 0; hl < 2; hl++) {
                        union { uint4 u; f16x8 v; } b;
                        b.u = gfr[(hl * 4 + q) * 2 + s2];
                        Y[q] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[s2].v, b.v, Y[q], 0, 0, 0);
                    }
            }
            // ---- per token (row 4 l4 + r): variance from the quadratic form, scores, weights ----
            // patch bit of token r at column 16 q + l15 as a float (0 / 1): multiplies the quadratic form's column and, as its upper half, IS the
            // bf16 B operand of the pooled patch (one v_perm per pair of tokens instead of compare / select chains)
            float bitf[4][4];
#pragma unroll
            for (int r = 0; r < 4; r++)
#pragma unroll
                for (int q = 0; q < 4; q++) bitf[r][q] = (float)(((q < 2 ? prx[r] : pry[r]) >> (16 * (q & 1) + l15)) & 1u);
            float av[4];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float qd = 0.f;
#pragma unroll
                for (int q = 0; q < 4; q++) qd = fmaf(bitf[r][q], Y[q][r], qd);
                qd = fmaf(qd, ginv, cross[r]);
                qd = row16_sum(qd);
                const float e = fmaf(E[r], einv, scn[r]);                        // head lanes: the raw score
                const float var = fmaxf((qd + ntv[r]) * invD, 0.f) + a.eps;
                const float rstd = EX ? 1.0f / sqrtf(var) : __builtin_amdgcn_rsqf(var);
                const float w = EX ? exp_acc(rstd * e - sref) : __expf(rstd * e - sref);   // (0 beyond the heads: their reference is +1e30)
                av[r] = w * rstd;
                L += w - wcn[r];
                if (l15 < NH) bw[(base + 4 * l4 + r) * 8 + l15] = av[r] - wcn[r] * rcv[r];
            }
            // ---- pooled patch: Pw[h][k] += a_t[h] p_tk ----
            if (EX) {
                // float32: one v_mfma_f32_16x16x4_f32 per token of the lane group and column tile (A: a of token 4 l4 + r for head l15,
                // B: that token's patch bit at column 16 q + l15; the k index of both is the lane group)
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        Pw[q] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bitf[r][q], Pw[q], 0, 0, 0);
                    }
            } else {
                // bf16: a as hi + remainder in the eight k-slots of the lane group (B: the patch bits twice)
                union { bf16x8 v; s16x4 h[2]; } wa;
                wa.h[0] = pack4_bf16(f32x2{av[0], av[1]}, f32x2{av[2], av[3]});
                {
                    const u32x2 hh = __builtin_bit_cast(u32x2, wa.h[0]);
                    const float r0 = av[0] - __uint_as_float(hh[0] << 16), r1 = av[1] - __uint_as_float(hh[0] & 0xffff0000u);
                    const float r2 = av[2] - __uint_as_float(hh[1] << 16), r3 = av[3] - __uint_as_float(hh[1] & 0xffff0000u);
                    wa.h[1] = pack4_bf16(f32x2{r0, r1}, f32x2{r2, r3});
                }
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    // (bf16 of a float is its upper half: 1.0f -> 0x3F80)
                    const unsigned b01 = __builtin_amdgcn_perm(__float_as_uint(bitf[1][q]), __float_as_uint(bitf[0][q]), 0x07060302u);
                    const unsigned b23 = __builtin_amdgcn_perm(__float_as_uint(bitf[3][q]), __float_as_uint(bitf[2][q]), 0x07060302u);
                    union { uint4 u; bf16x8 v; } pb;
                    pb.u = make_uint4(b01, b23, b01, b23);
                    Pw[q] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa.v, pb.v, Pw[q], 0, 0, 0);
                }
            }
        }
        // next board, by a fixed schedule: workgroup b of Gd sweeps the ranks forth and back - b, 2 Gd - 1 - b, 2 Gd + b, 4 Gd - 1 - b, ... -
        // so the heavy head of the rank order is paired with the light end of the next sweep, every rank below nvalid is taken exactly
        // once, and nobody waits for anybody: the board's game and cell codes are asked for behind the wave's last tile, in front of the
        // sums' barrier.  (Before: one ticket per board from a shared word - the ~400 workgroups that end their first, equally heavy
        // board together queued up on it, and the ticket's return was waited for at the barrier.)
        const int nboard = (ws_boards & 1) ? (ws_boards + 1) * (int)gridDim.x - 1 - (int)blockIdx.x : ws_boards * (int)gridDim.x + (int)blockIdx.x;
        int ngame = 0;
        if (SRC && nboard < nvalid) { ngame = __builtin_amdgcn_readfirstlane((int)gor[nboard]); if (fast) load_cells(ngame); }
        AZK_FSTAMP(3);                                            // wave 0's tiles
        // ---- the waves' sums meet ----
        {
            float Lw = L + __shfl_xor(L, 16);
            Lw += __shfl_xor(Lw, 32);
            if (lane < 8) lred[wave * 8 + lane] = lane < NH ? Lw : 0.f;
            if (l4 < 2) {
#pragma unroll
                for (int q = 0; q < 4; q++)
#pragma unroll
                    for (int j = 0; j < 4; j++) pwred[(wave * 8 + 4 * l4 + j) * 64 + 16 * q + l15] = Pw[q][j];
            }
        }
        __syncthreads();
        // ---- output rows, straight to memory: [head][0, T) token weights / L, [T, T+3) 1 / L (hi, lo, hi), [256, 320) pooled patch / L ----
        {
            // 1 / L once per wave: lane l sums head l & 7 (the four waves' shares in the order every thread used to add them, + l_all),
            // one reciprocal, and the eight values go to scalar registers
            float inv[NH], ivl;
            {
                const int hl = lane & 7;
                const float sl = ((lred[hl] + lred[8 + hl]) + (lred[16 + hl] + lred[24 + hl])) + lall_s[hl];
                ivl = EX ? 1.0f / sl : __builtin_amdgcn_rcpf(sl);   // (bf16 rows: 1 ulp is below their rounding)
#pragma unroll
                for (int h = 0; h < NH; h++) inv[h] = __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(ivl), h));
            }
            const bool isL = tid >= T && tid < T + 3;
            f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = {0.f, 0.f, 0.f, 0.f};
            if (dirty) { b0 = *(const f32x4 *)(bw + dpos * 8); b1 = *(const f32x4 *)(bw + dpos * 8 + 4); }
            float tinv[NH];                                        // the scale of this thread's token entries
#pragma unroll
            for (int h = 0; h < NH; h++) tinv[h] = inv[h];
            if (isL) {                                             // three threads: 1 / L (bf16 rows: as hi, remainder, hi; float32 rows: value, 0, 0)
#pragma unroll
                for (int h = 0; h < NH; h++) {
                    const unsigned hi = bf16_rne(inv[h]);
                    float v = tid == T + 1 ? inv[h] - __uint_as_float(hi << 16) : __uint_as_float(hi << 16);
                    if (EX) v = tid == T ? inv[h] : 0.f;
                    if (h < 4) b0[h & 3] = v; else b1[h & 3] = v;
                    tinv[h] = 1.0f;
                }
            }
            if (EX) {
                float *of = (float *)a.out + (size_t)board * NH * FOLD_ROW;
#pragma unroll
                for (int h = 0; h < NH; h++) of[h * FOLD_ROW + tid] = (h < 4 ? b0[h & 3] : b1[h & 3]) * tinv[h];
                {
                    const int h = tid >> 5, k = 2 * (tid & 31);           // two columns a thread: one 8-byte store each for the patch and its zero half
                    const float ih = __shfl(ivl, h);
                    if (h < NH) {
                        const f32x2 *pr = (const f32x2 *)(pwred + h * 64 + k);
                        const f32x2 p0 = pr[0], p1 = pr[256], p2 = pr[512], p3 = pr[768];
                        const f32x2 v = {((p0[0] + p1[0]) + (p2[0] + p3[0])) * ih, ((p0[1] + p1[1]) + (p2[1] + p3[1])) * ih};
                        *(f32x2 *)(of + h * FOLD_ROW + 256 + k) = v;
                        *(f32x2 *)(of + h * FOLD_ROW + 320 + k) = f32x2{0.f, 0.f};
                    }
                }
            } else {
                unsigned short *ob = (unsigned short *)a.out + (size_t)board * NH * FOLD_ROW;
                const u32x2 p0 = __builtin_bit_cast(u32x2, pack4_bf16(f32x2{b0[0] * tinv[0], b0[1] * tinv[1]}, f32x2{b0[2] * tinv[2], b0[3] * tinv[3]}));
                ob[0 * FOLD_ROW + tid] = (unsigned short)p0[0]; ob[1 * FOLD_ROW + tid] = (unsigned short)(p0[0] >> 16);
                ob[2 * FOLD_ROW + tid] = (unsigned short)p0[1]; ob[3 * FOLD_ROW + tid] = (unsigned short)(p0[1] >> 16);
                if (NH > 4) {
                    const u32x2 p1 = __builtin_bit_cast(u32x2, pack4_bf16(f32x2{b1[0] * tinv[4 % NH], b1[1] * tinv[5 % NH]}, f32x2{b1[2] * tinv[6 % NH], b1[3] * tinv[7 % NH]}));
                    ob[4 * FOLD_ROW + tid] = (unsigned short)p1[0]; ob[5 * FOLD_ROW + tid] = (unsigned short)(p1[0] >> 16);
                    ob[6 * FOLD_ROW + tid] = (unsigned short)p1[1]; ob[7 * FOLD_ROW + tid] = (unsigned short)(p1[1] >> 16);
                }
                {
                    const int h = tid >> 5, k = 2 * (tid & 31);           // two columns a thread: one packed word each for the patch and its zero half
                    const float ih = __shfl(ivl, h);
                    if (h < NH) {
                        const f32x2 *pr = (const f32x2 *)(pwred + h * 64 + k);
                        const f32x2 p0 = pr[0], p1 = pr[256], p2 = pr[512], p3 = pr[768];
                        const float v0 = ((p0[0] + p1[0]) + (p2[0] + p3[0])) * ih, v1 = ((p0[1] + p1[1]) + (p2[1] + p3[1])) * ih;
                        *(unsigned *)(ob + h * FOLD_ROW + 256 + k) = bf16_rne(v0) | (bf16_rne(v1) << 16);
                        *(unsigned *)(ob + h * FOLD_ROW + 320 + k) = 0u;
                    }
                }
            }
        }
        board = nboard; game = ngame;
        AZK_FSTAMP(4);                                            // sums, output rows, next board's loads issued
    }
    }
    if (a.wstats != nullptr && tid == 0 && ws_boards) { atomicAdd(a.wstats, (unsigned long long)ws_boards); atomicAdd(a.wstats + 1, (unsigned long long)ws_tiles); }
#undef AZK_FSTAMP
#ifdef AZK_EP_STAMPS
    if (stamp) {
        atomicMax((unsigned long long *)a.dbg + 5, (unsigned long long)(tacc[0] + tacc[1] + tacc[2] + tacc[3] + tacc[4]));   // the busiest workgroup of any launch
        for (int i = 0; i < 5; i++) atomicAdd((unsigned long long *)a.dbg + i, (unsigned long long)tacc[i]);
        atomicAdd((unsigned long long *)a.dbg + 6, (unsigned long long)ws_tiles);
        atomicAdd((unsigned long long *)a.dbg + 7, (unsigned long long)ws_boards);
    }
#endif
}

int g_fold_grid = 0;

template <int NC, int KSZ, int NH, bool SRC, bool EX>
int launch_embed_fold(const EmbedFoldArgs &a, hipStream_t st) {
    const int tp16 = ((a.T + 15) / 16) * 16;
    const int lds = 256 * 16 + tp16 * 8 + tp16 * 4 + 128 + 128 + 32 + tp16 * 32 + 4 * 8 * 64 * 4 + (SRC ? ((a.src.n_games + 7) / 8) * 16 + 32 : 0);   // 29 KB at 2 048 games (the rank -> game table + 16 spare entries)
    if (azk_set_max_lds((const void *)k_embed_fold<NC, KSZ, NH, SRC, EX>, lds + 2 * FOLD_MAX_SLOTS) != hipSuccess) return AZK_ERR_HIP;
    // two resident workgroups per CU by default; each sweeps the ranks forth and back (k_embed_fold, "next board").  azk_nn_embed_fold_grid(n): a caller that steps
    // several game groups on separate streams caps the grid (one workgroup per CU leaves the register file room for another group's
    // tree waves)
    const int cap = g_fold_grid > 0 ? g_fold_grid : 512;
    const int blocks = a.n < cap ? a.n : cap;
    k_embed_fold<NC, KSZ, NH, SRC, EX><<<blocks, 256, lds, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}
}  // namespace

extern "C" int32_t azk_nn_embed_fold_grid(int32_t max_workgroups) {
    if (max_workgroups < 0) return AZK_ERR_ARG;
    g_fold_grid = max_workgroups;                                   // 0: the default (512)
    return AZK_OK;
}

static int32_t embed_fold_impl(const void *boards_dev, int32_t boards_are_f32, const azk_leaf_source *src, const azk_embed_fold_consts *k,
                               void *rows_out, int32_t n, int32_t channels, int32_t rows, int32_t cols, const int32_t *n_valid_dev,
                               int32_t *sched_dev, void *stream, bool exact = false) {
    if ((!boards_dev && !src) || !k || !rows_out || !sched_dev) return AZK_ERR_ARG;
    if (!k->g_frag || !k->e_frag || !k->u2_tok || !k->score_tok || !k->wconst_tok || !k->l_all || !k->score_ref || !k->inv_scales) return AZK_ERR_ARG;
    const int ksize = k->ksize;
    if (n < 0 || channels < 1 || rows < 1 || cols < 1 || ksize < 1 || (ksize & 1) == 0 || channels * ksize * ksize > 64) return AZK_ERR_ARG;
    if (channels * rows * cols > 62 * 32 || k->embed_dim != 512) return AZK_ERR_ARG;
    if (rows * cols + 1 + 3 > 256) return AZK_ERR_ARG;             // one thread per token, three more for 1 / L
    if (channels * rows > 64 || cols > 28 || ksize > 5) return AZK_ERR_ARG;   // one lane per (plane, row) word: the row + two margin bits a side in 32 bits
    if (k->num_heads != 8 && k->num_heads != 4) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    EmbedFoldArgs a;
    memset(&a, 0, sizeof a);
    a.boards = boards_dev; a.boards_f32 = boards_are_f32; a.gfrag = (const uint4 *)k->g_frag; a.efrag = (const uint4 *)k->e_frag;
    a.u2T = k->u2_tok; a.scoreT = k->score_tok; a.wcT = k->wconst_tok; a.lall = k->l_all; a.sref = k->score_ref; a.inv_scales = k->inv_scales;
    a.out = rows_out; a.count = n_valid_dev; a.sched = sched_dev; a.wstats = (unsigned long long *)k->work_stats;
    a.n = n; a.R = rows; a.Cc = cols; a.T = rows * cols + 1; a.eps = k->ln_eps;
    a.rdivR = 65536 / rows + 1; a.rdivC = 65536 / cols + 1;
    if (src) a.src = *src;
    // leaf boards by dword: two planes, at most 64 dwords of cells, rows that start and end on a dword (k_embed_fold, load_cells)
    a.cwmax = src && channels == 2 && src->rc <= 256 && src->rc_pad >= src->rc && src->rc_pad % 4 == 0 && ((uintptr_t)src->leaf_cells & 3) == 0
                  ? src->rc_pad / 4 - 1 : -1;
    {
        static long long *dbg_buf = nullptr;
        const char *ds = getenv("AZK_EMBED_POOL_STAMPS");
        if (ds && atoi(ds)) {
            if (!dbg_buf && (hipMalloc((void **)&dbg_buf, 64) != hipSuccess || hipMemset(dbg_buf, 0, 64) != hipSuccess)) return AZK_ERR_HIP;
            a.dbg = dbg_buf;
            if (atoi(ds) == 2) {          // print-and-reset request
                long long h[8];
                if (hipMemcpy(h, dbg_buf, 64, hipMemcpyDeviceToHost) != hipSuccess) return AZK_ERR_HIP;
                const double nb = (double)(h[7] ? h[7] : 1);
                fprintf(stderr, "[embed_fold stamps] busiest workgroup %lld cycles | boards %lld tiles %lld | launch prologue (total) %lld | cycles per board: "
                        "load %.0f, patch+compact %.0f, wave 0 tiles %.0f, sums+output %.0f\n", h[5], h[7], h[6], h[0], h[1] / nb, h[2] / nb, h[3] / nb, h[4] / nb);
                if (hipMemset(dbg_buf, 0, 64) != hipSuccess) return AZK_ERR_HIP;
            }
        }
    }
    hipStream_t st = (hipStream_t)stream;
    const int nh = k->num_heads;
#define CASE(NC_, KSZ_, NH_) if (channels == NC_ && ksize == KSZ_ && nh == NH_) \
        return exact ? (src ? launch_embed_fold<NC_, KSZ_, NH_, true, true>(a, st) : launch_embed_fold<NC_, KSZ_, NH_, false, true>(a, st)) \
                     : (src ? launch_embed_fold<NC_, KSZ_, NH_, true, false>(a, st) : launch_embed_fold<NC_, KSZ_, NH_, false, false>(a, st))
    CASE(2, 5, 8); CASE(2, 5, 4); CASE(2, 3, 8); CASE(2, 3, 4); CASE(3, 3, 8); CASE(3, 3, 4);
#undef CASE
    return AZK_ERR_ARG;
}

extern "C" int32_t azk_nn_embed_fold(const void *boards_dev, int32_t boards_are_f32, const azk_embed_fold_consts *consts, void *rows_out_bf16_dev,
                                     int32_t n, int32_t channels, int32_t rows, int32_t cols, const int32_t *n_valid_dev, int32_t *sched_dev,
                                     void *stream) {
    if (!boards_dev) return AZK_ERR_ARG;
    return embed_fold_impl(boards_dev, boards_are_f32, nullptr, consts, rows_out_bf16_dev, n, channels, rows, cols, n_valid_dev, sched_dev, stream);
}

static int32_t embed_fold_leaves_impl(const azk_leaf_source *src, const azk_embed_fold_consts *consts, void *rows_out, int32_t *sched_dev,
                                      void *stream, bool exact) {
    if (!src || !src->leaf_flag || !src->leaf_cells || !src->to_move || !src->leaf_depth || !src->leaf_slot || !src->n_leaf) return AZK_ERR_ARG;
    if (src->n_games < 1 || src->rows * src->cols != src->rc || src->flag_bytes < src->n_games) return AZK_ERR_ARG;
    if (src->n_games > AZK_EMBED_FOLD_MAX_SLOTS) return AZK_ERR_ARG;        // the rank -> game table lives in LDS (2 bytes per slot)
    return embed_fold_impl(nullptr, 0, src, consts, rows_out, src->n_games, src->planes, src->rows, src->cols, nullptr, sched_dev, stream, exact);
}

extern "C" int32_t azk_nn_embed_fold_leaves(const azk_leaf_source *src, const azk_embed_fold_consts *consts, void *rows_out_bf16_dev,
                                            int32_t *sched_dev, void *stream) {
    return embed_fold_leaves_impl(src, consts, rows_out_bf16_dev, sched_dev, stream, false);
}

// the float32-accurate form (the fp32 line, include/azk.h): float32 rows for azk_nnx_gemm_h's float32-A first link
extern "C" int32_t azk_nnx_embed_fold(const void *boards_dev, int32_t boards_are_f32, const azk_embed_fold_consts *consts, float *rows_out_f32_dev,
                                      int32_t n, int32_t channels, int32_t rows, int32_t cols, const int32_t *n_valid_dev, int32_t *sched_dev,
                                      void *stream) {
    if (!boards_dev) return AZK_ERR_ARG;
    return embed_fold_impl(boards_dev, boards_are_f32, nullptr, consts, rows_out_f32_dev, n, channels, rows, cols, n_valid_dev, sched_dev, stream, true);
}

extern "C" int32_t azk_nnx_embed_fold_leaves(const azk_leaf_source *src, const azk_embed_fold_consts *consts, float *rows_out_f32_dev,
                                             int32_t *sched_dev, void *stream) {
    return embed_fold_leaves_impl(src, consts, rows_out_f32_dev, sched_dev, stream, true);
}

// =====================================================================================================
// k_tail_gemm: the cls-row tail (nn.py:54-60, 78-83 for the one row the heads read) as a chain of latency-shaped small
// GEMMs.  At ~1000 live rows every GEMM of the tail is a few MFLOP per CU: what costs time is the number of dependent
// memory round trips, so a wave issues EVERY load of its K range (A rows and weight fragments) before its first MFMA: one
// round trip.  NWK > 1 splits K over the waves of a workgroup (partials meet in LDS): a quarter of the loads and MFMAs on
// each wave's chain - what the three small GEMMs of the tail use.
//   wave tile 16 RT rows x 64 columns (RT picked in the kernel from the live row count, see k_tail_gemm below), no LDS staging;
//   A fragments straight from the row-major activations, B fragments from weights packed in fragment order
//   (pack_linear_weight: one 16-byte load per fragment);
//   AMODE 1: A = LayerNorm(rows) with the affine folded into weight and bias by the caller.  The row statistics come from the
//            PRODUCING GEMM: its epilogue leaves, per row and 64-column group, the (sum, sum of squares) of the bf16 values it
//            stored; the consumer adds the groups in a fixed order (deterministic, no atomics) and normalises its fragments on
//            the fly - LayerNorm costs no pass over the rows at all;
//   batched (block-diagonal) form: batch b reads A columns [b a_batch, b a_batch + K), its own weight block, and writes output
//            columns [b N, (b+1) N) - the per-head value projection (8 heads x [64 x 512]) in one launch;
//   epilogues: bf16 (+ bias), bf16 GELU(+ bias), bf16 (+ bias + residual), merged policy / value heads (float32 logits, tanh).
// Rows at or beyond *count are neither read nor written; the grid is sized for the full buffer and idle workgroups exit.
// =====================================================================================================
namespace {

using azk_tail::TailArgs;                         // the argument block and the epilogue selectors are shared with the LDS-staged form
                                                  // of the wide links (azk_tail.hip); so is the GELU arithmetic (azk_nn_common.h gelu_erf)
using azk_tail::TAIL_EPI_BF16;
using azk_tail::TAIL_EPI_GELU;
using azk_tail::TAIL_EPI_RESID;
using azk_tail::TAIL_EPI_HEADS;

// NWK > 1: the K range is split over NWK waves of the workgroup (every load of the whole K in flight at once, one round trip),
// their partial accumulators meet in LDS and wave 0 runs the epilogue.
// A wave keeps every A fragment of its K range in flight at once; the weight fragments are all in flight too when RT <= 2, and
// for the taller tiles the second half of them is fetched into the registers the matrix pipe has just consumed.
template <int RT, int KCH, int AMODE, int EPI, int NWR, int NWC, int NWK>
__device__ __forceinline__ void tail_items(const TailArgs &a, const int nvalid, f32x4 *kred) {
    constexpr int K = 32 * KCH * NWK, KS = KCH * NWK;
    constexpr int BH = RT > 3 ? KCH / 4 : RT > 2 ? KCH / 2 : KCH;  // weight k-steps in flight before the first MFMA
    static_assert(NWK == 1 || (NWR == 1 && NWC == 1), "split-K workgroups hold one wave tile");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, l15 = lane & 15, l4 = lane >> 4;
    const int wk = NWK > 1 ? wave : 0, wrc = NWK > 1 ? 0 : wave;
    const int wr = wrc / NWC, wc = wrc - wr * NWC;
    constexpr int WROWS = 16 * RT * NWR;
    const int rtiles = (nvalid + WROWS - 1) / WROWS, ctiles = a.N / (64 * NWC);
    const int nitems = rtiles * ctiles * a.nbatch;
    union BF { uint4 u; bf16x8 v; };
    for (int item = blockIdx.x; item < nitems; item += gridDim.x) {
        if (NWK > 1 && item != (int)blockIdx.x) __syncthreads();      // wave 0 is done with the previous item's partial sums
        const int ct = item % ctiles, r2 = item / ctiles, rt = r2 % rtiles, b = r2 / rtiles;
        const int row0 = rt * WROWS + wr * 16 * RT, g = ct * NWC + wc;
        const unsigned short *ap[RT];
#pragma unroll
        for (int i = 0; i < RT; i++) ap[i] = a.A + (size_t)min(row0 + 16 * i + l15, a.M - 1) * a.lda + (size_t)b * a.a_batch + 8 * l4 + 32 * KCH * wk;
        const uint4 *bp = a.Wp + (size_t)b * a.w_batch + ((size_t)g * KS + (size_t)KCH * wk) * 4 * 64 + lane;
        f32x4 acc[RT][4];
#pragma unroll
        for (int i = 0; i < RT; i++)
#pragma unroll
            for (int c = 0; c < 4; c++) acc[i][c] = f32x4{0.f, 0.f, 0.f, 0.f};
        // AMODE 1: the row statistics were left by the producing GEMM as per-column-group partial sums (of the bf16 values this
        // wave now reads), eight (sum, sum of squares) pairs per row: fetched FIRST, as four 16-byte loads per row, so that they
        // are back before the fragments they normalise (a scalar loop over the groups here cost one round trip per group)
        f32x4 st[AMODE == 1 ? RT : 1];                        // a lane fetches the quarter l4 of its row's 64 bytes
        if (AMODE == 1) {
#pragma unroll
            for (int i = 0; i < RT; i++) st[i] = *((const f32x4 *)(a.stats_in + (size_t)min(row0 + 16 * i + l15, a.M - 1) * 16) + l4);
        }
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        const int col0 = b * a.N + 64 * g + 4 * l15;          // a lane's four accumulators of a row are four consecutive output columns
        if (a.bias) bv = *(const f32x4 *)(a.bias + col0);
        BF af[RT][KCH], bf[KCH][4];
#pragma unroll
        for (int s = 0; s < KCH; s++) {
#pragma unroll
            for (int i = 0; i < RT; i++) af[i][s].u = *(const uint4 *)(ap[i] + 32 * s);
            if (s < BH) {
#pragma unroll
                for (int c = 0; c < 4; c++) bf[s][c].u = bp[(s * 4 + c) * 64];
            }
        }
        float rstd[RT], shift[RT];
        if (AMODE == 1) {                                     // the groups are added in a fixed order: deterministic, no atomics
#pragma unroll
            for (int i = 0; i < RT; i++) {
                float s1 = st[i][0] + st[i][2], s2 = st[i][1] + st[i][3];
                s1 += __shfl_xor(s1, 16); s2 += __shfl_xor(s2, 16);
                s1 += __shfl_xor(s1, 32); s2 += __shfl_xor(s2, 32);
                const float mean = s1 * (1.0f / K);
                rstd[i] = rsqrtf(fmaxf(s2 * (1.0f / K) - mean * mean, 0.f) + a.ln_eps);
                shift[i] = -mean * rstd[i];
            }
        }
        __builtin_amdgcn_sched_barrier(0);                    // every load above is issued before the first MFMA
#pragma unroll
        for (int s = 0; s < KCH; s++) {
            if (AMODE == 1) {
#pragma unroll
                for (int i = 0; i < RT; i++) {
                    const unsigned w4[4] = {af[i][s].u.x, af[i][s].u.y, af[i][s].u.z, af[i][s].u.w};
                    float v[8];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        v[2 * q] = __uint_as_float(w4[q] << 16) * rstd[i] + shift[i];
                        v[2 * q + 1] = __uint_as_float(w4[q] & 0xffff0000u) * rstd[i] + shift[i];
                    }
                    af[i][s].u = pack8(v);
                }
            }
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int c = 0; c < 4; c++) acc[i][c] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][s].v, bf[s][c].v, acc[i][c], 0, 0, 0);
            if (BH < KCH && s + BH < KCH) {
#pragma unroll
                for (int c = 0; c < 4; c++) bf[s + BH][c].u = bp[((s + BH) * 4 + c) * 64];
                __builtin_amdgcn_sched_barrier(0);            // (the refill stays behind the MFMAs that free its registers)
            }
        }
        if (row0 >= nvalid) continue;                          // (uniform per wave tile; with NWK > 1 per workgroup)
        if (NWK > 1) {
            if (wave > 0) {
#pragma unroll
                for (int i = 0; i < RT; i++)
#pragma unroll
                    for (int c = 0; c < 4; c++) kred[((wave - 1) * RT * 4 + i * 4 + c) * 64 + lane] = acc[i][c];
            }
            __syncthreads();
            if (wave > 0) continue;
#pragma unroll
            for (int w = 1; w < NWK; w++)
#pragma unroll
                for (int i = 0; i < RT; i++)
#pragma unroll
                    for (int c = 0; c < 4; c++) acc[i][c] += kred[((w - 1) * RT * 4 + i * 4 + c) * 64 + lane];
        }
        // epilogue: every load (residual rows) first, then straight-line arithmetic, then the stores under their row predicate with
        // nothing to wait for in between (a load or a branch between two stores makes every store wait for the one before it)
        uint2 rr[EPI == TAIL_EPI_RESID ? RT : 1][4];
        if (EPI == TAIL_EPI_RESID) {
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) rr[i][j] = *(const uint2 *)(a.resid + (size_t)min(row0 + 16 * i + 4 * l4 + j, a.M - 1) * a.ldr + col0);
        }
        if (EPI == TAIL_EPI_HEADS) {                          // nn.py:82-83
            f32x4 hv[RT][4];
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    hv[i][j] = f32x4{acc[i][0][j] + bv[0], acc[i][1][j] + bv[1], acc[i][2][j] + bv[2], acc[i][3][j] + bv[3]};
#pragma unroll
                    for (int c = 0; c < 4; c++)
                        if (col0 + c == a.action_dim) hv[i][j][c] = tanhf(hv[i][j][c]);
                }
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int row = row0 + 16 * i + 4 * l4 + j;
#pragma unroll
                    for (int c = 0; c < 4; c++) {
                        const int col = col0 + c;
                        if (row < nvalid && col < a.action_dim) a.logits[(size_t)row * a.action_dim + col] = hv[i][j][c];
                        if (row < nvalid && col == a.action_dim) a.values[row] = hv[i][j][c];
                    }
                }
        } else {
            uint2 o[RT][4];
            f32x2 ps[RT][4];
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    f32x4 v = {acc[i][0][j] + bv[0], acc[i][1][j] + bv[1], acc[i][2][j] + bv[2], acc[i][3][j] + bv[3]};
                    if (EPI == TAIL_EPI_GELU) {
#pragma unroll
                        for (int c = 0; c < 4; c++) v[c] = gelu_erf(v[c]);                                      // nn.GELU (erf form)
                    }
                    if (EPI == TAIL_EPI_RESID) {
                        v[0] += __uint_as_float(rr[i][j].x << 16); v[1] += __uint_as_float(rr[i][j].x & 0xffff0000u);
                        v[2] += __uint_as_float(rr[i][j].y << 16); v[3] += __uint_as_float(rr[i][j].y & 0xffff0000u);
                    }
                    union { bf16x4 b4; uint2 u; } ob;
                    ob.b4 = __builtin_convertvector(v, bf16x4);
                    o[i][j] = ob.u;
                    if (a.stats_out) {
                        // partial LayerNorm statistics of the row, over this wave's 64 columns, from the ROUNDED values
                        const f32x4 vr = __builtin_convertvector(ob.b4, f32x4);
                        ps[i][j] = f32x2{row16_sum((vr[0] + vr[1]) + (vr[2] + vr[3])),
                                         row16_sum((vr[0] * vr[0] + vr[1] * vr[1]) + (vr[2] * vr[2] + vr[3] * vr[3]))};
                    }
                }
            const int ngr = a.nbatch * (a.N >> 6), gr = b * (a.N >> 6) + g;
#pragma unroll
            for (int i = 0; i < RT; i++)
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int row = row0 + 16 * i + 4 * l4 + j;
                    if (row < nvalid) *(uint2 *)(a.out + (size_t)row * a.ldo + col0) = o[i][j];
                    if (a.stats_out && l15 == 0 && row < nvalid) *(f32x2 *)(a.stats_out + ((size_t)row * ngr + gr) * 2) = ps[i][j];
                }
        }
    }
}

// The wave tile is 16 RT rows tall, RT chosen per launch from the LIVE row count (RTLO..RTHI): the smallest tile that still puts
// every wave of the launch on the chip at once.  These kernels hold their whole K range in registers (one wave per SIMD), so a
// launch with more waves than SIMDs runs as two rounds of the same latency chain - measured: the five-launch tail took 54 us at
// 1024 live rows and 79 us at 1056 with a fixed 32-row tile.
template <int RTLO, int RTHI, int KCH, int AMODE, int EPI, int NWR, int NWC, int NWK>
__global__ __launch_bounds__(64 * NWR * NWC * NWK, 1) void k_tail_gemm(TailArgs a) {
    __shared__ f32x4 kred[NWK > 1 ? (NWK - 1) * RTHI * 4 * 64 : 1];
    // the items cover the live rows only (measured: letting the dead half of the buffer issue its loads too costs 40-60 % - these
    // GEMMs move ~100 KB per wave through L2 and are bound by that traffic, not by the count's extra round trip)
    // (every kernel argument is wanted in SGPRs HERE: left alone, the compiler fetches the count pointer first, waits for the count,
    //  and only then goes back to the argument segment for the rest - a third dependent scalar round trip before the first load)
    asm volatile("" :: "s"(a.A), "s"(a.Wp), "s"(a.out), "s"(a.bias), "s"(a.resid), "s"(a.stats_in), "s"(a.stats_out), "s"(a.logits), "s"(a.values),
                 "s"(a.lda), "s"(a.ldo), "s"(a.N), "s"(a.nbatch), "s"(a.wave_slots), "s"(a.M), "s"(a.a_batch), "s"(a.w_batch), "s"(a.ldr),
                 "s"(a.ln_eps), "s"(a.action_dim));
    const int nvalid = a.count ? min(a.M, *a.count) : a.M;
    const int strip_waves = (a.N >> 6) * a.nbatch * NWK;          // waves per strip of 16 RT rows
    int rt = RTLO;
    while (rt < RTHI && ((nvalid + 16 * rt * NWR - 1) / (16 * rt * NWR)) * NWR * strip_waves > a.wave_slots) rt++;
    if (RTHI >= RTLO + 2 && rt == RTLO + 2) tail_items<(RTHI >= RTLO + 2 ? RTLO + 2 : RTLO), KCH, AMODE, EPI, NWR, NWC, NWK>(a, nvalid, kred);
    else if (RTHI >= RTLO + 1 && rt == RTLO + 1) tail_items<(RTHI >= RTLO + 1 ? RTLO + 1 : RTLO), KCH, AMODE, EPI, NWR, NWC, NWK>(a, nvalid, kred);
    else tail_items<RTLO, KCH, AMODE, EPI, NWR, NWC, NWK>(a, nvalid, kred);
}

int tail_cu_count() {
    static int cus = 0;
    if (!cus) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    }
    return cus;
}

template <int RTLO, int RTHI, int KCH, int AMODE, int EPI, int NWR, int NWC, int NWK = 1>
int launch_tail(TailArgs &a, hipStream_t st) {
    static_assert(RTHI <= RTLO + 2, "three tile heights per kernel");
    // waves of this instantiation the chip holds at once (its register footprint decides: 1 per SIMD for the whole-K variants,
    // 2-3 for the split-K ones)
    static int slots = 0;
    if (!slots) {
        int nb = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_tail_gemm<RTLO, RTHI, KCH, AMODE, EPI, NWR, NWC, NWK>, 64 * NWR * NWC * NWK, 0) != hipSuccess || nb < 1) nb = 1;
        slots = nb * NWR * NWC * NWK * tail_cu_count();
    }
    a.wave_slots = slots;
    const long long items = (long long)((a.M + 16 * RTLO * NWR - 1) / (16 * RTLO * NWR)) * (a.N / (64 * NWC)) * a.nbatch;
    const unsigned blocks = (unsigned)(items < 8192 ? items : 8192);
    k_tail_gemm<RTLO, RTHI, KCH, AMODE, EPI, NWR, NWC, NWK><<<blocks, 64 * NWR * NWC * NWK, 0, st>>>(a);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}
}  // namespace

extern "C" int32_t azk_nn_tail_gemm(const azk_tail_gemm *t, void *stream) {
    if (!t || !t->a_bf16 || !t->w_packed || t->m < 0 || t->n_out < 64 || (t->n_out & 63) || t->nbatch < 1) return AZK_ERR_ARG;
    if ((t->k != 512 && t->k != 2048 && t->k != 384) || t->lda < t->k || (t->lda & 7) || (t->a_batch_stride & 7)) return AZK_ERR_ARG;
    if (t->epilogue < 0 || t->epilogue > 3 || (t->layernorm_a && (t->k != 512 || !t->a_stats || t->a_stats_groups != 8))) return AZK_ERR_ARG;
    if (t->epilogue == TAIL_EPI_HEADS ? (!t->logits_out || !t->values_out || t->action_dim + 1 > t->n_out * t->nbatch) : (!t->out_bf16 || t->ldo < t->n_out * t->nbatch || (t->ldo & 3)))
        return AZK_ERR_ARG;
    if (t->epilogue == TAIL_EPI_RESID && (!t->resid_bf16 || (t->ldr & 3))) return AZK_ERR_ARG;
    if (t->m == 0) return AZK_OK;
    TailArgs a = {};
    a.A = (const unsigned short *)t->a_bf16; a.lda = t->lda; a.a_batch = t->a_batch_stride; a.Wp = (const uint4 *)t->w_packed;
    a.w_batch = (long long)(t->n_out / 64) * (t->k / 32) * 4 * 64;
    a.M = t->m; a.N = t->n_out; a.nbatch = t->nbatch; a.count = t->n_valid; a.bias = t->bias; a.out = (unsigned short *)t->out_bf16; a.ldo = t->ldo;
    a.resid = (const unsigned short *)t->resid_bf16; a.ldr = t->ldr; a.ln_eps = t->ln_eps; a.logits = t->logits_out; a.values = t->values_out;
    a.action_dim = t->action_dim; a.stats_in = t->a_stats; a.stats_groups = t->a_stats_groups; a.stats_out = t->stats_out;
    hipStream_t st = (hipStream_t)stream;
    const bool wide = t->n_out % 128 == 0 && t->n_out >= 1024;          // many column groups: 2 x 2 waves share A rows and weight fragments in L1
    if (t->k == 384)                                                    // the embed-fold rows (AZK_EMBED_FOLD_ROW) against [D_t; U_all; M_h]: K split over four waves
        return !t->layernorm_a && t->epilogue == TAIL_EPI_BF16 ? launch_tail<2, 2, 3, 0, TAIL_EPI_BF16, 1, 1, 4>(a, st) : AZK_ERR_ARG;
    if (t->k == 512) {
        if (t->layernorm_a) {
            if (t->epilogue == TAIL_EPI_GELU) return wide ? launch_tail<2, 4, 16, 1, TAIL_EPI_GELU, 2, 2>(a, st) : launch_tail<2, 2, 16, 1, TAIL_EPI_GELU, 1, 1>(a, st);
            if (t->epilogue == TAIL_EPI_HEADS) return launch_tail<1, 1, 4, 1, TAIL_EPI_HEADS, 1, 1, 4>(a, st);
            if (t->epilogue == TAIL_EPI_BF16) return launch_tail<2, 2, 16, 1, TAIL_EPI_BF16, 1, 1>(a, st);
            return AZK_ERR_ARG;
        }
        if (t->epilogue == TAIL_EPI_BF16) return launch_tail<2, 2, 4, 0, TAIL_EPI_BF16, 1, 1, 4>(a, st);       // (K split over four waves: a quarter of the loads and MFMAs on each wave's chain)
        if (t->epilogue == TAIL_EPI_GELU) return wide ? launch_tail<2, 4, 16, 0, TAIL_EPI_GELU, 2, 2>(a, st) : launch_tail<2, 2, 16, 0, TAIL_EPI_GELU, 1, 1>(a, st);
        if (t->epilogue == TAIL_EPI_RESID) return launch_tail<2, 2, 16, 0, TAIL_EPI_RESID, 1, 1>(a, st);
        return launch_tail<2, 2, 16, 0, TAIL_EPI_HEADS, 1, 1>(a, st);
    }
    // k = 2048: four waves of a workgroup take 512 columns of K each
    if (t->epilogue == TAIL_EPI_RESID) return launch_tail<2, 4, 16, 0, TAIL_EPI_RESID, 1, 1, 4>(a, st);
    if (t->epilogue == TAIL_EPI_BF16) return launch_tail<2, 4, 16, 0, TAIL_EPI_BF16, 1, 1, 4>(a, st);
    return AZK_ERR_ARG;
}
