// azk_emit.hip - (state, pi, z) emission of finished games into the caller's replay ring: each game's tuple range (k_emit_alloc), the tuples
// under the reference's eight transforms or a mask of D4 elements (k_emit_tuples), the mark that ends it; the kernels and the C ABI calls
// that launch them (include/azk.h).  Built with -ffp-contract=off like every engine file.
#include "azk_opt_pack.h"
#include "azk_sym_map.h"      // sym_source: emission under a mask of elements

namespace {

// ------------------------------------------------------------------------------------------------
// (state, pi, z) emission: train.save_data_to_buffer (train.py:30-49) with rotate_data / flip_data (train.py:8-27).
// Position i of a finished game (side to move = i & 1): z = +-1 by winner (0 for a draw), state = canonical board;
// positions 0 and 1 once, the others 8 times in the order rot0, lr(rot0), tb(rot0), rot90, lr(rot90), tb(rot90),
// rot180, rot270 (np.rot90 is counter-clockwise).  Tuple t of the stream lands in slot t % capacity (deque(maxlen)).
// ------------------------------------------------------------------------------------------------
// CAP (playout-cap engines): only the plies of FULL searches are emitted - ply i's group (1 tuple for i < 2, else 8) sits at
// the sum of the groups of the full plies before it; the board before ply i is rebuilt from every earlier ply, fast ones included.
// SYM (engines created with emit_elements): the group of a ply from the third on is one tuple per
// element of the mask (es.n of them, es.els in ascending order) instead of the reference's eight, on any R x C board and action kind.
// SURPRISE (engines with surprise weighting): ply i of the recorded plies F (all, or with CAP the full ones; n_F of them, S = the
// sequential sum of their kl in ply order) is written c_i = floor(w_i) + (coin_i < w_i - floor(w_i)) times,
//     w_i = S > 0 ? (1 - lambda) + ((lambda * n_F) * kl_i) / S : 1      (float64)
// copy-major at base + sum_{j<i} c_j * grp_j.  k_emit_alloc writes c into traj_copies (0 outside F) and reserves the sum; k_emit_tuples reads it.
// OPEN (engines with random openings): the opening's plies i < open_plies[g] had no search and are left out exactly as a
// capped engine's fast plies are - no tuples, not in n_F or S, 0 copies, not in the sums of the tuples before a ply; `i < 2 ? 1 : grp`
// stays keyed on the absolute ply index, and boards are rebuilt from ply 0.
// VALUE (engines with value targets): the tuples of ply i carry t_i instead of z_i.  With o the first searched ply, q_i =
// traj_q (the root's W / N at the move of ply i: the value for the mover's opponent), v_i = -q_i, z_i the outcome from ply i's mover's view:
//     G_{n-1} = (1 - lam) * v_{n-1} + lam * z_{n-1};    G_i = (1 - lam) * v_i + lam * (-G_{i+1})  for i = n-2 .. o;    t_i = (1 - r) * z_i + r * G_i
// in float64, one ply after the other from the last one down (the side to move alternates, hence the sign).  Every searched ply takes part,
// a capped engine's fast plies too; k_emit_alloc's thread of the game writes t into traj_vt, k_emit_tuples writes (float)t_i into every tuple
// of ply i - every element of the group, every copy.  r = 0, and r = lam = 1, write z bit for bit (a draw keeps +0.0: the last sum has a +0.0 term).
template <bool CAP, bool SYM, bool SURPRISE, bool OPEN, bool VALUE>
__device__ __forceinline__ void emit_alloc_body(Dev d, const uint8_t *traj_full, unsigned long long *cursor, long long *game_base_out, const EmitSym &es,
                                                const SurpriseDev &sp, const OpenEmit &oe, const ValueDev &vt) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= d.G) return;
    long long base = -1;                                          // the stream index stays 64-bit end to end (2^31 tuples = hours of self-play)
    if (d.done[g] == 1) {
        const int n = d.move_count[g];
        const int grp = SYM ? es.n : 8;
        int o = 0;                                                // the first ply that had a search
        if constexpr (OPEN) o = min(oe.open_plies[g], n);
        int tuples = n <= 2 ? n : 2 + grp * (n - 2);
        if (OPEN) tuples -= o <= 2 ? o : 2 + grp * (o - 2);
        if (CAP) {
            tuples = 0;
            for (int i = o; i < n; i++) if (traj_full[(size_t)g * d.g.state_dim + i]) tuples += i < 2 ? 1 : grp;
        }
        if constexpr (SURPRISE) {
            const size_t row = (size_t)g * d.g.state_dim;
            int n_F = 0;
            double S = 0.0;
            for (int i = o; i < n; i++) if (!CAP || traj_full[row + i]) { n_F += 1; S += sp.traj_kl[row + i]; }
            tuples = 0;
            for (int i = 0; i < n; i++) {
                int c = 0;
                if ((!OPEN || i >= o) && (!CAP || traj_full[row + i])) {
                    const double w = S > 0.0 ? (1.0 - sp.lambda) + ((sp.lambda * (double)n_F) * sp.traj_kl[row + i]) / S : 1.0;
                    const double f = floor(w);
                    c = (int)f + (sp.traj_coin[row + i] < w - f ? 1 : 0);
                }
                sp.traj_copies[row + i] = (uint16_t)c;
                tuples += c * (i < 2 ? 1 : grp);
            }
        }
        if constexpr (VALUE) {
            const size_t row = (size_t)g * d.g.state_dim;
            const int winner = d.winner[g];
            double G = 0.0;
            for (int i = n - 1; i >= o; i--) {
                const double z = winner == -1 ? 0.0 : ((i & 1) == winner ? 1.0 : -1.0);
                const double v = -vt.traj_q[row + i];
                G = (1.0 - vt.lam) * v + vt.lam * (i == n - 1 ? z : -G);
                vt.traj_vt[row + i] = (1.0 - vt.r) * z + vt.r * G;
            }
        }
        base = (long long)atomicAdd(cursor, (unsigned long long)tuples);
    }
    d.emit_base[g] = base;
    if (game_base_out) game_base_out[g] = base;
}

template <bool CAP, bool SYM, bool SURPRISE, bool OPEN, bool VALUE>
__global__ void k_emit_alloc(EmitPack<CAP, SYM, SURPRISE, OPEN, VALUE> a, unsigned long long *cursor, long long *game_base_out) {
    emit_alloc_body<CAP, SYM, SURPRISE, OPEN, VALUE>(a, opt<CapDev>(a).traj_full, cursor, game_base_out, opt<EmitSym>(a), opt<SurpriseDev>(a), opt<OpenEmit>(a),
                                                     opt<ValueDev>(a));
}

__device__ __forceinline__ int d4_source(int t, int i, int j, int N) {
    // source cell (row-major) of output cell (i, j) under transform t of the reference's emission order
    int si, sj;
    switch (t) {
        case 0: si = i; sj = j; break;                          // rot0
        case 1: si = i; sj = N - 1 - j; break;                  // lr(rot0)
        case 2: si = N - 1 - i; sj = j; break;                  // tb(rot0)
        case 3: si = j; sj = N - 1 - i; break;                  // rot90 (ccw): out[i][j] = in[j][N-1-i]
        case 4: si = N - 1 - j; sj = N - 1 - i; break;          // lr(rot90)
        case 5: si = j; sj = i; break;                          // tb(rot90)
        case 6: si = N - 1 - i; sj = N - 1 - j; break;          // rot180
        default: si = N - 1 - j; sj = i; break;                 // rot270: out[i][j] = in[N-1-j][i]
    }
    return si * N + sj;
}

// LIST: the grid walks a list of finished games (asynchronous drain) instead of covering all G.  SURPRISE: the ply's group is written
// traj_copies[i] times, copy-major, behind the copies of the plies before it (a capped engine's fast plies have 0 copies: traj_full is not read)
// OPEN: the opening's plies are not written and do not count among the tuples before a ply (their copies are 0 under SURPRISE)
// VALUE: the z of a tuple is the ply's target out of traj_vt, rounded to float32, instead of the outcome
template <bool LIST, bool CAP, bool SYM, bool SURPRISE, bool OPEN, bool VALUE>
__device__ __forceinline__ void emit_tuples_body(Dev d, const uint8_t *traj_full, float *states, double *pis, float *zs, long long capacity,
                                                 const unsigned long long *cursor, const int *list, const int *n_list, const EmitSym &es,
                                                 const uint16_t *traj_copies, const OpenEmit &oe, const double *traj_vt) {
    const int S = d.g.state_dim, A = d.g.action_dim, rc = d.g.rc, F = d.g.planes, N = d.g.rows;
    const int lane = azk_lane();
    const int nb = LIST ? *n_list * S : (int)gridDim.x;
    for (int blk = blockIdx.x; blk < nb; blk += gridDim.x) {
    if (LIST && blk != (int)blockIdx.x) __syncthreads();
    const int gi = blk / S, i = blk - gi * S;
    const int g = LIST ? list[gi] : gi;
    const long long base = d.emit_base[g];
    if (base < 0 || i >= d.move_count[g]) continue;
    int o = 0;                                                    // the first ply that had a search
    if constexpr (OPEN) { o = uniform_i32(oe.open_plies[g]); if (i < o) continue; }   // an opening ply: it was drawn, not searched
    if (CAP && !SURPRISE && traj_full[(size_t)g * S + i] == 0) continue;      // a fast ply: it chose the move, it is not trained on
    const int copies = SURPRISE ? (int)traj_copies[(size_t)g * S + i] : 1;
    if (SURPRISE && copies == 0) continue;                        // no copy of this ply: the coin rounded its weight down to none (or a fast ply)
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    uint8_t *cells = sm;                                          // board before ply i
    for (int c = lane; c < rc; c += AZK_WAVE) cells[c] = 0;
    __syncthreads();
    const int16_t *acts = d.traj_action + (size_t)g * S;
    for (int j = lane; j < i; j += AZK_WAVE) cells[acts[j]] = (uint8_t)(1 << (j & 1));
    __syncthreads();
    const int side = i & 1, winner = d.winner[g];
    float z = winner == -1 ? 0.0f : (side == winner ? 1.0f : -1.0f);
    if constexpr (VALUE) z = (float)traj_vt[(size_t)g * S + i];
    const double *pi = d.traj_pi + ((size_t)g * S + i) * A;
    const int grp = SYM ? es.n : 8;
    const int ntr = i < 2 ? 1 : grp;
    long long first = base + (i < 2 ? i : 2 + grp * (i - 2));
    if (OPEN) first -= o < 2 ? o : 2 + grp * (o - 2);
    if (CAP && !SURPRISE) {                                       // tuples of the full plies before this one
        int before = 0;
        for (int j = o + lane; j < i; j += AZK_WAVE) if (traj_full[(size_t)g * S + j]) before += j < 2 ? 1 : grp;
        first = base + wave_sum_i32(before);
    }
    if (SURPRISE) {                                               // tuples of every copy of the plies before this one
        int before = 0;
        for (int j = lane; j < i; j += AZK_WAVE) before += (int)traj_copies[(size_t)g * S + j] * (j < 2 ? 1 : grp);
        first = base + wave_sum_i32(before);
    }
    const long long stream_end = (long long)*cursor;              // after k_emit_alloc: one past the newest tuple of this call
    for (int tt = 0; tt < ntr * copies; tt++) {
        const int t = SURPRISE ? tt % ntr : tt;                   // copy-major: copy tt / ntr of the group's tuple t
        if (first + tt < stream_end - capacity) continue;         // already pushed out of the ring by newer tuples (deque(maxlen))
        const long long slot = (first + tt) % capacity;
        float *so = states + (size_t)slot * F * rc;
        double *po = pis + (size_t)slot * A;
        const int el = SYM ? (int)((es.els >> (4 * t)) & 15u) : t;   // (plies 0 and 1: t = 0 and the mask's first element is the identity)
        for (int e = lane; e < rc; e += AZK_WAVE) {
            const int src = SYM ? sym_source(el, e, d.g.rows, d.g.cols, d.g.inv_cols) : d4_source(t, e / N, e % N, N);
            const uint8_t code = cells[src];
            so[e] = (float)((code >> side) & 1);                    // canonical: own stones first (gomoku.py:34-40)
            so[rc + e] = (float)((code >> (side ^ 1)) & 1);
            if (F == 3) so[2 * rc + e] = (float)side;
            if (!SYM || A == rc) po[e] = pi[src];                   // one action per cell: action index == cell index
        }
        if (SYM && A != rc)                                         // Connect4's columns, a -> cols - 1 - a under lr: the cells' map on a board of one row
            for (int a = lane; a < A; a += AZK_WAVE) po[a] = pi[sym_source(el, a, 1, A, 0u)];
        if (lane == 0) zs[slot] = z;
    }
    }
}

template <bool LIST, bool CAP, bool SYM, bool SURPRISE, bool OPEN, bool VALUE>
__global__ __launch_bounds__(AZK_WAVE) void k_emit_tuples(EmitPack<CAP, SYM, SURPRISE, OPEN, VALUE> a, float *states, double *pis, float *zs, long long capacity,
                                                            const unsigned long long *cursor, const int *list, const int *n_list) {
    emit_tuples_body<LIST, CAP, SYM, SURPRISE, OPEN, VALUE>(a, opt<CapDev>(a).traj_full, states, pis, zs, capacity, cursor, list, n_list, opt<EmitSym>(a),
                                                            opt<SurpriseDev>(a).traj_copies, opt<OpenEmit>(a), opt<ValueDev>(a).traj_vt);
}

__global__ void k_emit_mark(Dev d) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < d.G && d.done[g] == 1 && d.emit_base[g] >= 0) d.done[g] = 2;      // emitted; recycle / later calls skip it
}

}  // namespace

// (state, pi, z) emission on the stream: each finished game's tuple range, the tuples, done = 2.  list == nullptr: one block per (game, ply)
// of all G games; else the blocks walk the *n_list listed games (asynchronous drain).  A capped engine emits the plies of full searches only
void azk_launch_emit(azk_engine *e, float *states, double *pis, float *zs, long long capacity, unsigned long long *cursor, long long *game_base,
                        const int *list, const int *n_list, hipStream_t st) {
    const Dev &d = e->d;
    const unsigned per_game = (unsigned)((d.G + 255) / 256), lds = (unsigned)up16(d.g.rc);
    const int plies = d.G * d.g.state_dim;
    const unsigned blocks = (unsigned)(list && plies > 16384 ? 16384 : plies);
    with_flags([&](auto by_list, auto cap, auto sym, auto surprise, auto open, auto value) {   // sym: emit_elements, the mask's elements on any geometry
        const EmitPack<cap.value, sym.value, surprise.value, open.value, value.value> a{d, on<cap.value>(e->cp), on<sym.value>(e->emit), on<surprise.value>(e->sp),
                                                                                        on<open.value>(OpenEmit{e->op.open_plies}), on<value.value>(e->vt)};
        k_emit_alloc<cap.value, sym.value, surprise.value, open.value, value.value><<<per_game, 256, 0, st>>>(a, cursor, game_base);
        k_emit_tuples<by_list.value, cap.value, sym.value, surprise.value, open.value, value.value><<<blocks, AZK_WAVE, lds, st>>>(a, states, pis, zs, capacity,
                                                                                                                                  cursor, list, n_list);
    }, list != nullptr, e->cp.n_fast != 0, e->emit.n != 0, e->sp_on, e->op_on, e->vt_on);
    k_emit_mark<<<per_game, 256, 0, st>>>(d);
}

extern "C" {

int32_t azk_emit_finished(azk_engine *e, float *states_dev, double *pis_dev, float *zs_dev, int64_t capacity,
                          int64_t *cursor_dev, int64_t *game_base_dev, void *stream) {
    if (!e || !states_dev || !pis_dev || !zs_dev || !cursor_dev || capacity < 1) return AZK_ERR_ARG;
    const Dev &d = e->d;
    if (!d.traj_pi) { e->err = "azk_emit_finished: (state, pi, z) emission needs a square board with one action per cell (or an engine created with emit_elements)"; return AZK_ERR_ARG; }
    azk_launch_emit(e, states_dev, pis_dev, zs_dev, (long long)capacity, (unsigned long long *)cursor_dev, (long long *)game_base_dev, nullptr, nullptr, (hipStream_t)stream);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_emit_elements(const azk_engine *e, int32_t *mask_out, int32_t *group_out) {
    if (!e) return AZK_ERR_ARG;
    if (mask_out) *mask_out = e->cfg.emit_elements;
    if (group_out) *group_out = e->emit.n ? e->emit.n : (e->d.traj_pi ? 8 : 0);
    return AZK_OK;
}

}  // extern "C"
