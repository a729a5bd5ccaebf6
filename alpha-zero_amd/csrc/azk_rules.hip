// azk_rules.hip - the stateless board-rule kernels (no azk_engine: the rule set of games/*.py over float32 boards) and the
// deterministic row softmax; k_rules, k_softmax_rows and the azk_rules_* / azk_softmax_rows calls.  Built with -ffp-contract=off.
#include "azk_engine_int.h"

namespace {

// ------------------------------------------------------------------------------------------------
// stateless rule kernels over float32 boards [n][F][R][C] (the reference's own board layout)
// ------------------------------------------------------------------------------------------------
enum { RULE_MOVES = 0, RULE_MASK, RULE_APPLY, RULE_UNDO, RULE_WINNER, RULE_CANON };

struct RuleArgs {
    GameDesc g;
    int mode, n, table_size;
    const float *boards_in; float *boards;
    const int *players; const int *cells;
    int16_t *moves; int *counts; uint8_t *mask; int *out_i; float *out_f;
};

__device__ __forceinline__ uint8_t code_of(float p0, float p1) {
    uint8_t c = (p0 == 1.0f ? 1 : 0) | (p1 == 1.0f ? 2 : 0);
    if ((p0 != 0.0f && p0 != 1.0f) || (p1 != 0.0f && p1 != 1.0f)) c |= 4;
    return c;
}

__global__ __launch_bounds__(AZK_WAVE) void k_rules(RuleArgs a) {
    const int b = blockIdx.x, lane = azk_lane();
    const GameDesc &g = a.g;
    const int rc = g.rc, F = g.planes;
    LdsView L = carve(g, 4, a.table_size);
    const float *src = (a.boards_in ? a.boards_in : a.boards) + (size_t)b * F * rc;
    for (int i = lane; i < rc; i += AZK_WAVE) L.board[i] = code_of(src[i], src[rc + i]);
    __syncthreads();
    if (a.mode == RULE_MOVES || a.mode == RULE_MASK) {
        const int n = azk_valid_moves(L.board, g, L.moves, L.ms);
        if (a.mode == RULE_MOVES) {
            for (int i = lane; i < n; i += AZK_WAVE) a.moves[(size_t)b * rc + i] = L.moves[i];
            if (lane == 0) a.counts[b] = n;
        } else {
            for (int i = lane; i < g.action_dim; i += AZK_WAVE) a.mask[(size_t)b * g.action_dim + i] = 0;
            __syncthreads();
            for (int i = lane; i < n; i += AZK_WAVE) a.mask[(size_t)b * g.action_dim + azk_action_idx(g, L.moves[i])] = 1;
        }
    } else if (a.mode == RULE_APPLY) {
        const int player = a.players[b], cell = a.cells[b];
        float *dst = a.boards + (size_t)b * F * rc;
        int next = player;
        if (g.kind == AZK_KIND_C4 || L.board[cell] == 0) {
            next = 1 - player;
            if (lane == 0) dst[(size_t)player * rc + cell] = 1.0f;
            if (F == 3) for (int i = lane; i < rc; i += AZK_WAVE) dst[2 * rc + i] = (float)(1 - player);
        }
        if (lane == 0) a.out_i[b] = next;
    } else if (a.mode == RULE_UNDO) {
        const int cur = a.players[b], cell = a.cells[b];
        float *dst = a.boards + (size_t)b * F * rc;
        if (lane == 0) dst[(size_t)(1 - cur) * rc + cell] = 0.0f;
        if (F == 3) for (int i = lane; i < rc; i += AZK_WAVE) dst[2 * rc + i] = (float)(1 - cur);
    } else if (a.mode == RULE_WINNER) {
        const int w = azk_check_winner(L.board, g, a.players[b], a.cells[b]);
        if (lane == 0) a.out_i[b] = w;
    } else if (a.mode == RULE_CANON) {
        const int player = a.players[b];
        float *dst = a.out_f + (size_t)b * F * rc;
        for (int i = lane; i < F * rc; i += AZK_WAVE) {
            const int plane = i / rc, c = i - plane * rc;
            const int sp = plane < 2 ? (plane ^ player) : plane;
            dst[i] = src[(size_t)sp * rc + c];
        }
    }
}

__global__ __launch_bounds__(AZK_WAVE) void k_softmax_rows(const float *logits, int A, float *out) {
    const int b = blockIdx.x, lane = azk_lane();
    float *e = (float *)azk_smem;
    for (int i = lane; i < A; i += AZK_WAVE) e[i] = azk_exp_det(logits[(size_t)b * A + i]);
    __syncthreads();
    const float s = azk_pairwise_sum(e, A);
    for (int i = lane; i < A; i += AZK_WAVE) out[(size_t)b * A + i] = e[i] / s;
}

}  // namespace

extern "C" {

// ---- stateless rule kernels ---------------------------------------------------------------------
static int32_t run_rules(int mode, int32_t game, int32_t rows, int32_t cols, const float *in, float *inout, int32_t n,
                         const int32_t *players, const int32_t *cells, int16_t *moves, int32_t *counts, uint8_t *mask,
                         int32_t *out_i, float *out_f, void *stream) {
    RuleArgs a;
    memset(&a, 0, sizeof a);
    std::string err;
    if (!make_game(game, rows, cols, &a.g, &err)) { azk_create_error = err; return AZK_ERR_ARG; }
    if (n < 0) { azk_create_error = "negative batch"; return AZK_ERR_ARG; }
    if (n == 0) return AZK_OK;
    a.mode = mode; a.n = n; a.table_size = table_size_for(a.g);
    a.boards_in = in; a.boards = inout; a.players = players; a.cells = cells;
    a.moves = moves; a.counts = counts; a.mask = mask; a.out_i = out_i; a.out_f = out_f;
    int off[LDS_REGIONS];
    const int lds = lds_layout(a.g, 4, a.table_size, off);
    k_rules<<<n, AZK_WAVE, lds, (hipStream_t)stream>>>(a);
    hipError_t s = hipGetLastError();
    if (s != hipSuccess) { azk_create_error = std::string("k_rules: ") + hipGetErrorString(s); return AZK_ERR_HIP; }
    return AZK_OK;
}

int32_t azk_rules_legal_moves(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                              int16_t *moves_dev, int32_t *counts_dev, void *stream) {
    if (!boards_dev || !moves_dev || !counts_dev) return AZK_ERR_ARG;
    return run_rules(RULE_MOVES, game, rows, cols, boards_dev, nullptr, n, nullptr, nullptr, moves_dev, counts_dev, nullptr, nullptr, nullptr, stream);
}
int32_t azk_rules_legal_mask(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                             uint8_t *mask_dev, void *stream) {
    if (!boards_dev || !mask_dev) return AZK_ERR_ARG;
    return run_rules(RULE_MASK, game, rows, cols, boards_dev, nullptr, n, nullptr, nullptr, nullptr, nullptr, mask_dev, nullptr, nullptr, stream);
}
int32_t azk_rules_apply_move(int32_t game, int32_t rows, int32_t cols, float *boards_dev, int32_t n,
                             const int32_t *players_dev, const int32_t *cells_dev, int32_t *next_player_dev, void *stream) {
    if (!boards_dev || !players_dev || !cells_dev || !next_player_dev) return AZK_ERR_ARG;
    return run_rules(RULE_APPLY, game, rows, cols, nullptr, boards_dev, n, players_dev, cells_dev, nullptr, nullptr, nullptr, next_player_dev, nullptr, stream);
}
int32_t azk_rules_undo_move(int32_t game, int32_t rows, int32_t cols, float *boards_dev, int32_t n,
                            const int32_t *current_players_dev, const int32_t *cells_dev, void *stream) {
    if (!boards_dev || !current_players_dev || !cells_dev) return AZK_ERR_ARG;
    return run_rules(RULE_UNDO, game, rows, cols, nullptr, boards_dev, n, current_players_dev, cells_dev, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}
int32_t azk_rules_check_winner(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                               const int32_t *players_dev, const int32_t *cells_dev, int32_t *winners_dev, void *stream) {
    if (!boards_dev || !players_dev || !cells_dev || !winners_dev) return AZK_ERR_ARG;
    return run_rules(RULE_WINNER, game, rows, cols, boards_dev, nullptr, n, players_dev, cells_dev, nullptr, nullptr, nullptr, winners_dev, nullptr, stream);
}
int32_t azk_rules_canonical(int32_t game, int32_t rows, int32_t cols, const float *boards_dev, int32_t n,
                            const int32_t *players_dev, float *out_dev, void *stream) {
    if (!boards_dev || !players_dev || !out_dev) return AZK_ERR_ARG;
    return run_rules(RULE_CANON, game, rows, cols, boards_dev, nullptr, n, players_dev, nullptr, nullptr, nullptr, nullptr, nullptr, out_dev, stream);
}

int32_t azk_softmax_rows(const float *logits_dev, int32_t n, int32_t action_dim, float *out_dev, void *stream) {
    if (!logits_dev || !out_dev || n < 0 || action_dim < 1 || action_dim > 512) return AZK_ERR_ARG;
    if (n == 0) return AZK_OK;
    const int lds = (((action_dim + 31) & ~31) + 32) * 4;
    k_softmax_rows<<<n, AZK_WAVE, lds, (hipStream_t)stream>>>(logits_dev, action_dim, out_dev);
    return hipGetLastError() == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

}  // extern "C"
