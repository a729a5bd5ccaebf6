// azk_noise.hip - the rows of random numbers a search reads, made ahead of it: Dirichlet rows and move uniforms (k_gen_noise), Gumbel rows
// (k_gen_gumbel), both from azk_rng.h's generators; the Dirichlet rows over the legal moves, made from the position itself (k_root_noise,
// k_root_noise_due; azk_set_root_noise); and the counters' sums.  The kernels and the C ABI calls that launch them (include/azk.h).
// Built with -ffp-contract=off like every engine file.
#include "azk_rng.h"

namespace {

__global__ void k_sum_counters(const long long *counters, int G, long long *out) {
    // one block per counter
    __shared__ long long sm[256];
    long long s = 0;
    for (int i = threadIdx.x; i < G; i += blockDim.x) s += counters[(size_t)blockIdx.x * G + i];
    sm[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) sm[threadIdx.x] += sm[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) out[blockIdx.x] = sm[0];
}

__global__ __launch_bounds__(AZK_WAVE) void k_gen_noise(int A, unsigned long long seed, long long first_game, int move,
                                                         double alpha, double *noise, double *uniforms, long long row_stride) {
    const int g = blockIdx.x, lane = azk_lane();
    const unsigned long long gg = (unsigned long long)(first_game + g);
    __shared__ double red[AZK_WAVE];
    if (uniforms && lane == 0) uniforms[g] = noise_uniform(seed, gg, move);
    if (!noise) return;
    noise_row(A, seed, gg, move, alpha, noise + (size_t)g * (size_t)row_stride, red);
}

__global__ __launch_bounds__(AZK_WAVE) void k_gen_gumbel(int A, unsigned long long seed, long long first_game, int move, double *rows, double *uniforms,
                                                          long long row_stride) {
    const int g = blockIdx.x;
    const size_t o = (size_t)g * (size_t)row_stride;
    gumbel_row(A, seed, (unsigned long long)(first_game + g), move, rows != nullptr ? rows + o : nullptr, uniforms != nullptr ? uniforms + o : nullptr);
}

// The asynchronous engine (azk_moves.hip) keeps two rows per game and makes them a search ahead, off the step's chain.
// drain: the Dirichlet rows that fell due since the last drain - for every game that moved, the row of the search AFTER the one it has
// just begun (key slot_moves[g] + 1, into the buffer the finished search read from)
__global__ __launch_bounds__(AZK_WAVE) void k_noise_ahead(Dev d, AsyncDev p) {
    __shared__ double red[AZK_WAVE];
    const int n = *p.todo_count, A = d.g.action_dim;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        const int g = p.todo_list[f];
        const int key = (int)p.slot_moves[g] + 1;
        if (uniform_i32(p.noise_key[g]) >= key) continue;
        noise_row(A, p.seed, (unsigned long long)(p.first_game + g), key, p.alpha, p.noise + ((size_t)g * 2 + (size_t)(key & 1)) * A, red);
        if (azk_lane() == 0) p.noise_key[g] = key;
        __syncthreads();
    }
}

// ... and its Gumbel form (an engine with a Gumbel root keeps Gumbel rows where the others keep Dirichlet rows)
__global__ __launch_bounds__(AZK_WAVE) void k_gumbel_ahead(Dev d, AsyncDev p) {
    const int n = *p.todo_count, A = d.g.action_dim;
    for (int f = blockIdx.x; f < n; f += gridDim.x) {
        const int g = p.todo_list[f];
        const int key = (int)p.slot_moves[g] + 1;
        if (uniform_i32(p.noise_key[g]) >= key) continue;
        gumbel_row(A, p.seed, (unsigned long long)(p.first_game + g), key, p.noise + ((size_t)g * 2 + (size_t)(key & 1)) * A);
        __syncthreads();
        if (azk_lane() == 0) p.noise_key[g] = key;
    }
}

__global__ void k_fill_i32(int *p, int n, int v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

// ================================================================================================
// Root noise on the legal moves (azk_set_root_noise, opt-in): the Dirichlet row of a search is drawn over L, the actions
// that are legal in the position the search starts from - exactly the children its root gets -, and is +0.0 everywhere else.  With n = |L|:
//   alpha_eff   alpha (mode 1, "legal") or alpha / n (mode 2, "total": the row's total concentration n * alpha_eff stays alpha)
//   a in L      gam[a] = noise_row's Gamma(alpha_eff) draw of entry a at the same counters (AZK_GAMMA_ENTRY, azk_rng.h), row[a] = gam[a] / sum_L gam,
//               or 1 / n where that sum is 0; n == 1 gives exactly 1.0
//   L           TicTacToe: the empty cells; Connect4: the columns whose top cell is empty; Gomoku: the empty cells with a stone among their
//               eight neighbours, or the centre cell (rows / 2, cols / 2) where there is none (gomoku.py:94-106, as a set).  A full TicTacToe or
//               Connect4 board (a finished game that waits in the batch) has n == 0: its row is all zeros
// One wave per game.  The cells arrive as dwords, four cells per lane and two dwords (512 cells >= make_game's 400), as in open_game_one; each
// lane keeps a 4-bit legality mask per dword (Gomoku's neighbour test reads the wave's LDS copy of the board), the masks' popcounts are ranked
// by a prefix sum over the lanes, and the legal actions go into an LDS list in ascending order.  The Gamma chain then runs over that list, lanes
// over the legal actions - ceil(n / 64) entries per lane instead of ceil(A / 64) -, the sum is the lane partials in list order and noise_row's
// LDS tree, and every lane stores the entries of its own cells: value or zero, one plain vector store each, no atomics.
// ================================================================================================
enum { RN_MAX_CELLS = 400 };                                         // make_game's bound on rc (and so on A)
struct RootNoiseLds {
    double red[AZK_WAVE];                                            // noise_row's reduction tree
    double gam[RN_MAX_CELLS];                                        // the legal actions' draws, by rank
    int16_t act[RN_MAX_CELLS];                                       // the legal actions, ascending
    uint8_t board[8 * AZK_WAVE];                                     // the cells, for Gomoku's neighbour test
};

__device__ __forceinline__ int rn_scan_incl(int v) {                 // inclusive prefix sum over the wave's lanes
    const int lane = azk_lane();
#pragma unroll
    for (int off = 1; off < AZK_WAVE; off <<= 1) { const int o = __shfl_up(v, off); if (lane >= off) v += o; }
    return v;
}

// All lanes of the wave call; g, key, mode and alpha are wave-uniform.  row: the game's float64 [A]
__device__ __forceinline__ void root_noise_row(const Dev &d, int g, unsigned long long seed, unsigned long long gg, int key, int mode, double alpha,
                                               double *row, RootNoiseLds &s) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const int A = gd.action_dim, R = gd.rows, C = gd.cols;
    const uint32_t *cw = (const uint32_t *)(d.cells + (size_t)g * d.rc_pad);
    uint32_t cell4[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        const int idx = p * AZK_WAVE + lane;
        cell4[p] = 4 * idx < d.rc_pad ? cw[idx] : 0u;                 // (rc_pad is a multiple of 16: a dword is inside or outside as a whole)
        ((uint32_t *)s.board)[idx] = cell4[p];
    }
    __syncthreads();
    // a legality bit per cell
    unsigned leg4[2];
#pragma unroll
    for (int p = 0; p < 2; p++) {
        leg4[p] = 0u;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int e = 4 * (p * AZK_WAVE + lane) + b;
            if (e >= gd.rc || ((cell4[p] >> (8 * b)) & 0xffu) != 0u) continue;
            bool ok = gd.kind == AZK_KIND_TTT || (gd.kind == AZK_KIND_C4 && e < C);      // Connect4: a column stands for its top cell
            if (gd.kind == AZK_KIND_GOMOKU) {
                const int r = (int)(((unsigned)e * gd.inv_cols) >> 16), c = e - r * C;
#pragma unroll
                for (int dr = -1; dr <= 1; dr++)
#pragma unroll
                    for (int dc = -1; dc <= 1; dc++) {
                        const int rr = r + dr, cc = c + dc;
                        if ((dr != 0 || dc != 0) && rr >= 0 && rr < R && cc >= 0 && cc < C && (s.board[rr * C + cc] & 3) != 0) ok = true;
                    }
            }
            if (ok) leg4[p] |= 1u << b;
        }
    }
    if (gd.kind == AZK_KIND_GOMOKU && __ballot((leg4[0] | leg4[1]) != 0u) == 0ull) {      // no candidate: the centre cell (gomoku.py:104-105)
        const int centre = (R / 2) * C + C / 2, idx = centre >> 2;
        if (lane == (idx & (AZK_WAVE - 1))) leg4[idx >> 6] |= 1u << (centre & 3);
    }
    // n, and the legal actions in ascending order
    const int n0 = __popc(leg4[0]), n1 = __popc(leg4[1]);
    const int incl0 = rn_scan_incl(n0), incl1 = rn_scan_incl(n1);
    const int tot0 = __builtin_amdgcn_readlane(incl0, AZK_WAVE - 1), n = tot0 + __builtin_amdgcn_readlane(incl1, AZK_WAVE - 1);
    const int first[2] = {incl0 - n0, tot0 + incl1 - n1};            // rank of the lane's first legal cell of each dword
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int b = 0; b < 4; b++)
            if ((leg4[p] >> b) & 1u) s.act[first[p] + __popc(leg4[p] & ((1u << b) - 1u))] = (int16_t)(4 * (p * AZK_WAVE + lane) + b);   // (Connect4: e < cols is the column)
    __syncthreads();
    // the Gamma chain, lanes over the legal actions
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const double alpha_eff = mode == 2 ? alpha / (double)n : alpha;
    double part = 0.0;
    for (int r = lane; r < n; r += AZK_WAVE) {
        const int a = (int)s.act[r];
        AZK_GAMMA_ENTRY(gam, k0, k1, gg, a, key, alpha_eff)
        s.gam[r] = gam;
        part += gam;
    }
    s.red[lane] = part;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) { if (lane < o) s.red[lane] += s.red[lane + o]; __syncthreads(); }
    const double tot = s.red[0];
    // every lane stores the entries of its own cells
#pragma unroll
    for (int p = 0; p < 2; p++)
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const int e = 4 * (p * AZK_WAVE + lane) + b;
            if (e >= A) continue;
            const bool legal = (leg4[p] >> b) & 1u;
            const int r = legal ? first[p] + __popc(leg4[p] & ((1u << b) - 1u)) : 0;
            row[e] = legal ? (tot > 0.0 ? s.gam[r] / tot : 1.0 / (double)n) : 0.0;
        }
    __syncthreads();
}

// The lock-step entry (azk_gen_root_noise): one wave per game, the uniforms of k_gen_noise bit for bit, the rows from d.cells as they stand
__global__ __launch_bounds__(AZK_WAVE) void k_root_noise(Dev d, RootNoiseDev rn, unsigned long long seed, long long first_game, int move, double *noise,
                                                          double *uniforms) {
    const int g = blockIdx.x;
    const unsigned long long gg = (unsigned long long)(first_game + g);
    __shared__ RootNoiseLds s;
    if (uniforms && azk_lane() == 0) uniforms[g] = noise_uniform(seed, gg, move);
    if (!noise) return;
    root_noise_row(d, g, seed, gg, move, rn.mode, rn.alpha, noise + (size_t)g * (size_t)d.g.action_dim, s);
}

// The asynchronous entry: one wave per game; a game is DUE iff it is not finished and its row pair has no row for its move key yet (the
// mover has moved it, or the drain has restarted it, since).  A due game gets row slot_moves[g] & 1 of its pair - the row k_tree and
// reroot_one take for that key - and row_key[g] = the key.  The test describes itself and is idempotent: the kernel may be launched wherever a
// key may have moved, and a wave that is not due ends after one vector load, as k_move_async's does.  (On a re-rooting engine the due games
// are the parked and the restarted ones: no other game's key moves.)  It also empties the movers' list of rows that fell due, which nothing
// reads while the option is set: behind every mover launch, so that the list never holds more than G games.
__global__ __launch_bounds__(AZK_WAVE) void k_root_noise_due(Dev d, AsyncDev p, RootNoiseDev rn) {
    const int g = blockIdx.x, lane = azk_lane();
    __shared__ RootNoiseLds s;
    const int *up = d.done + g;
    up = lane == 1 ? (const int *)(p.slot_moves + g) : up;         // (low word: a slot plays far fewer than 2^31 moves)
    up = lane == 2 ? rn.row_key + g : up;
    const int uw = *up;
    if (g == 0 && lane == 0) *p.todo_count = 0;
    const int key = __builtin_amdgcn_readlane(uw, 1);
    if (__builtin_amdgcn_readlane(uw, 0) != 0 || __builtin_amdgcn_readlane(uw, 2) == key) return;
    const int A = d.g.action_dim;
    root_noise_row(d, g, p.seed, (unsigned long long)(p.first_game + g), key, rn.mode, rn.alpha, p.noise + ((size_t)g * 2 + (size_t)(key & 1)) * A, s);
    if (lane == 0) rn.row_key[g] = key;
}

// azk_get_root_noise: the row each game's current search reads, out of [G][A] rows or the asynchronous engine's [G][2][A] pairs (sel: the
// slots' move counters, whose low bit names the row)
__global__ void k_copy_rows(const double *noise, const long long *sel, int G, int A, double *out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)G * A) return;
    const size_t g = i / (size_t)A, a = i - g * (size_t)A;
    out[i] = sel != nullptr ? noise[(g * 2 + (size_t)(sel[g] & 1)) * A + a] : noise[i];
}

}  // namespace

int32_t azk_root_noise_begin(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    if (!e->rn.row_key) HIPCHK(e, dalloc(e, &e->rn.row_key, (size_t)d.G));
    HIPCHK(e, hipMemsetAsync(e->rn.row_key, 0xff, sizeof(int) * (size_t)d.G, st));
    k_fill_i32<<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(e->ad.noise_key, d.G, 0x7fffffff);   // the movers' "row exists" test holds for every key
    azk_launch_root_noise_due(e, st);
    return AZK_OK;
}

void azk_launch_root_noise_due(azk_engine *e, hipStream_t st) {
    k_root_noise_due<<<e->d.G, AZK_WAVE, 0, st>>>(e->d, e->ad, e->rn);
}

void azk_launch_rows_ahead(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    if (e->gb.m) k_gumbel_ahead<<<(unsigned)(d.G < 512 ? d.G : 512), AZK_WAVE, 0, st>>>(d, e->ad);
    else k_noise_ahead<<<(unsigned)(d.G < 512 ? d.G : 512), AZK_WAVE, 0, st>>>(d, e->ad);
}

void azk_launch_first_rows(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    const AsyncDev &a = e->ad;
    const int A = d.g.action_dim;
    if (e->gb.m) {                                                // a Gumbel root: Gumbel rows where the others keep Dirichlet rows
        k_gen_gumbel<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 0, a.noise, nullptr, 2LL * A);
        k_gen_gumbel<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 1, a.noise + A, nullptr, 2LL * A);
    } else {
        k_gen_noise<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 0, a.alpha, a.noise, nullptr, 2LL * A);
        k_gen_noise<<<d.G, AZK_WAVE, 0, st>>>(A, a.seed, a.first_game, 1, a.alpha, a.noise + A, nullptr, 2LL * A);
    }
    k_fill_i32<<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(a.noise_key, d.G, 1);       // every game's rows exist up to key 1
}

extern "C" {

int32_t azk_gen_noise(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double alpha,
                      double *noise_dev, double *uniforms_dev, void *stream) {
    if (!e || alpha <= 0.0) return AZK_ERR_ARG;
    k_gen_noise<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(e->d.g.action_dim, seed, first_global_game, move_index, alpha,
                                                            noise_dev, uniforms_dev, (long long)e->d.g.action_dim);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_gen_root_noise(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *noise_dev, double *uniforms_dev,
                           void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (!e->rn.mode) { e->err = "azk_gen_root_noise: no root noise is set (azk_set_root_noise; azk_gen_noise draws the rows over the whole action vector)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_gen_root_noise: the asynchronous movers make their rows themselves"; return AZK_ERR_STATE; }
    k_root_noise<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(e->d, e->rn, seed, first_global_game, move_index, noise_dev, uniforms_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_get_root_noise(azk_engine *e, double *rows_dev, void *stream) {
    if (!e || !rows_dev) return AZK_ERR_ARG;
    if (!e->rn.mode) { e->err = "azk_get_root_noise: no root noise is set (azk_set_root_noise)"; return AZK_ERR_STATE; }
    if (e->d.noise == nullptr) { e->err = "azk_get_root_noise: no search with a noise row has begun"; return AZK_ERR_STATE; }
    const int G = e->d.G, A = e->d.g.action_dim;
    k_copy_rows<<<(unsigned)(((size_t)G * A + 255) / 256), 256, 0, (hipStream_t)stream>>>(e->d.noise, e->d.noise_sel, G, A, rows_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

static int32_t gen_gumbel(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *gumbel_dev, double *uniforms_dev, void *stream) {
    k_gen_gumbel<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(e->d.g.action_dim, seed, first_global_game, move_index, gumbel_dev, uniforms_dev,
                                                             (long long)e->d.g.action_dim);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_gen_gumbel(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *gumbel_dev, void *stream) {
    if (!e || !gumbel_dev) return AZK_ERR_ARG;
    return gen_gumbel(e, seed, first_global_game, move_index, gumbel_dev, nullptr, stream);
}

int32_t azk_gen_gumbel_uniforms(azk_engine *e, uint64_t seed, int64_t first_global_game, int32_t move_index, double *uniforms_dev, void *stream) {
    if (!e || !uniforms_dev) return AZK_ERR_ARG;
    return gen_gumbel(e, seed, first_global_game, move_index, nullptr, uniforms_dev, stream);
}

int32_t azk_get_counters(azk_engine *e, azk_counters *out, void *stream) {
    if (!e || !out) return AZK_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    k_sum_counters<<<CNT_N, 256, 0, st>>>(e->d.counters, e->d.G, e->counter_sums);
    HIPCHK(e, hipGetLastError());
    long long h[CNT_N];
    HIPCHK(e, hipMemcpyAsync(h, e->counter_sums, sizeof h, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    memset(out, 0, sizeof *out);
    out->sims = h[CNT_SIMS]; out->edges_scanned = h[CNT_SCANNED]; out->trace_nodes = h[CNT_TRACE];
    out->edges_created = h[CNT_CREATED]; out->leaves_evaluated = h[CNT_LEAVES]; out->terminal_sims = h[CNT_TERMINAL];
    out->moves_played = h[CNT_MOVES]; out->cache_hits = h[CNT_CACHE_HITS];
    out->roots_reused = h[CNT_REUSED]; out->nodes_carried = h[CNT_CARRIED];
    out->forced_selections = h[CNT_FORCED]; out->visits_pruned = h[CNT_PRUNED]; out->visits_before_pruning = h[CNT_PRUNE_OF];
    return AZK_OK;
}

}  // extern "C"
