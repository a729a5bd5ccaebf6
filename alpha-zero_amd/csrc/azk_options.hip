// azk_options.hip - the opt-ins' state calls (include/azk.h): set, clear and read playout cap, forced playouts, Gumbel root, resignation,
// surprise weighting, random openings, root noise on the legal moves, the move temperature, value targets, the solver and adaptive search budgets (both rules).  No kernel: they check arguments, allocate the option's arrays on first use and fill the argument
// block (azk_engine_int.h) that azk_opt_pack.h hands to the kernels of azk_begin.hip, azk_moves.hip and azk_emit.hip.
#include "azk_engine_int.h"
#include <algorithm>
#include <float.h>

// resignation: no game resigned, no mark, zero statistics (azk_set_resign, and azk_async_begin where the slots' move counters start again at 0)
int32_t azk_resign_clear(azk_engine *e, hipStream_t st) {
    const ResignDev &r = e->rs;
    HIPCHK(e, hipMemsetAsync(r.resigned, 0, (size_t)e->d.G, st));
    HIPCHK(e, hipMemsetAsync(r.mark_start, 0, sizeof(uint32_t) * (size_t)e->d.G, st));
    HIPCHK(e, hipMemsetAsync(r.mark_side, 0xff, sizeof(int) * (size_t)e->d.G, st));
    HIPCHK(e, hipMemsetAsync(r.stats, 0, sizeof(long long) * 4, st));
    return AZK_OK;
}

extern "C" {

// ---- playout-cap randomisation ---------------------------------------------------------------------------------------------
int32_t azk_set_playout_cap(azk_engine *e, double p_full, int32_t n_fast, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_playout_cap: set the cap before azk_async_begin"; return AZK_ERR_STATE; }
    if (n_fast == 0) { e->cp.n_fast = 0; return AZK_OK; }         // off: the engine launches what it launched before
    if (e->gb.m) { e->err = "azk_set_playout_cap: a Gumbel root is set - its halving table is built for one budget"; return AZK_ERR_STATE; }
    if (!(p_full >= 0.0 && p_full <= 1.0)) { e->err = "azk_set_playout_cap: p_full must lie in [0, 1]"; return AZK_ERR_ARG; }
    if (n_fast < 1 || n_fast > e->cfg.max_sims) { e->err = "azk_set_playout_cap: n_fast must lie in [1, max_sims]"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_playout_cap: a playout cap does not combine with leaves_per_step > 1 (virtual loss counts completed simulations differently)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    CapDev &c = e->cp;
    if (!c.search_full) {
        HIPCHK(e, dalloc(e, &c.search_full, (size_t)d.G));
        if (d.traj_pi) HIPCHK(e, dalloc(e, &c.traj_full, (size_t)d.G * d.g.state_dim));
    }
    HIPCHK(e, hipMemsetAsync(c.search_full, 1, (size_t)d.G, (hipStream_t)stream));
    if (c.traj_full) HIPCHK(e, hipMemsetAsync(c.traj_full, 1, (size_t)d.G * d.g.state_dim, (hipStream_t)stream));
    c.p_full = p_full; c.seed = seed; c.first_game = first_global_game; c.stats = nullptr; c.rec_full = nullptr;
    c.n_fast = n_fast;
    return AZK_OK;
}

int32_t azk_get_search_full(azk_engine *e, uint8_t *full_dev, void *stream) {
    if (!e || !full_dev) return AZK_ERR_ARG;
    if (!e->cp.n_fast) { e->err = "azk_get_search_full: no playout cap is set (azk_set_playout_cap)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(full_dev, e->cp.search_full, (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_record_flags(azk_engine *e, uint8_t *rec_full_dev) {
    if (!e) return AZK_ERR_ARG;
    if (!e->cp.n_fast) { e->err = "azk_async_record_flags: no playout cap is set (azk_set_playout_cap)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_record_flags: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->cp.rec_full = rec_full_dev;
    return AZK_OK;
}

// ---- forced playouts and policy target pruning ------------------------------------------------------------------------------
int32_t azk_set_forced_playouts(azk_engine *e, double k, void *stream) {
    (void)stream;
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_forced_playouts: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!(k >= 0.0) || k - k != 0.0) { e->err = "azk_set_forced_playouts: k must be finite and not negative (0 = off)"; return AZK_ERR_ARG; }
    if (k == 0.0) { e->forced_k = 0.0; return AZK_OK; }              // off: the engine launches what it launched before
    if (e->gb.m) { e->err = "azk_set_forced_playouts: a Gumbel root is set - its eligibility rule needs raw root selection"; return AZK_ERR_STATE; }
    if (e->sv_on) { e->err = "azk_set_forced_playouts: the solver is set (azk_set_solver) - a forced child and a child shut out would claim the same selection"; return AZK_ERR_STATE; }
    if (e->puct_on) { e->err = "azk_set_forced_playouts: configurable PUCT is set (azk_set_puct) - the pruning bound restates the reference's selection formula"; return AZK_ERR_STATE; }
    if (e->d.K > 1) { e->err = "azk_set_forced_playouts: forced playouts do not combine with leaves_per_step > 1 (a virtual-loss search counts a visit before its value exists: the floor would be met by visits that carry nothing)"; return AZK_ERR_ARG; }
    e->forced_k = k;
    return AZK_OK;
}

// ---- Gumbel root search -----------------------------------------------------------------------------------------------------
// schedule(m, n): the visit count a root child must have at each of the n root selections of a search that halves m sampled children
static void gumbel_schedule(int m, int n, int *out) {
    if (m <= 1) { for (int t = 0; t < n; t++) out[t] = t; return; }
    int L = 0;
    while ((1 << L) < m) L++;
    std::vector<int> v((size_t)m, 0);
    int c = m, len = 0;
    while (len < n) {
        const int extra = std::max(1, n / (L * c));
        for (int x = 0; x < extra && len < n; x++)
            for (int i = 0; i < c; i++) { if (len < n) out[len++] = v[i]; v[i] += 1; }
        c = std::max(2, c / 2);
    }
}

int32_t azk_set_gumbel_root(azk_engine *e, int32_t m, int32_t n_sims, double c_visit, double c_scale, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_gumbel_root: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (m < 1 || m > 64) { e->err = "azk_set_gumbel_root: m must lie in [1, 64]"; return AZK_ERR_ARG; }
    if (n_sims < 2 || n_sims > e->cfg.max_sims) { e->err = "azk_set_gumbel_root: n_sims must lie in [2, max_sims]"; return AZK_ERR_ARG; }
    if (!(c_visit >= 0.0) || c_visit - c_visit != 0.0) { e->err = "azk_set_gumbel_root: c_visit must be finite and not negative"; return AZK_ERR_ARG; }
    if (!(c_scale > 0.0) || c_scale - c_scale != 0.0) { e->err = "azk_set_gumbel_root: c_scale must be finite and positive"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with leaves_per_step > 1 (a virtual-loss search counts a visit before its value exists: eligibility by visit count would pass over it)"; return AZK_ERR_ARG; }
    if (e->ru.mode) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with tree reuse (the eligibility rule needs a fresh root: every child at 0 visits)"; return AZK_ERR_STATE; }
    if (e->cp.n_fast) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with a playout cap (the halving table is built for one budget)"; return AZK_ERR_STATE; }
    if (e->forced_k != 0.0) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with forced playouts (the eligibility rule needs raw root selection)"; return AZK_ERR_STATE; }
    if (e->sp_on) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with surprise weighting (its recorded pi is not a visit distribution)"; return AZK_ERR_STATE; }
    if (e->sv_on) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with the solver (azk_set_solver: the eligibility rule needs raw root selection)"; return AZK_ERR_STATE; }
    if (e->puct_on) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with configurable PUCT (azk_set_puct: its root selection is not PUCT)"; return AZK_ERR_STATE; }
    if (e->tp_on) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with a move temperature (azk_set_move_temperature: the Gumbel arg-max is the sample)"; return AZK_ERR_STATE; }
    if (e->vt_on) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with value targets (azk_set_value_target: the Gumbel movers do not keep the per-ply q)"; return AZK_ERR_STATE; }
    if (e->rn.mode) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with root noise on the legal moves (azk_set_root_noise: its rows are Dirichlet rows)"; return AZK_ERR_STATE; }
    if (adaptive_on(e)) { e->err = "azk_set_gumbel_root: a Gumbel root does not combine with adaptive search budgets (azk_set_kld_stop, azk_set_lead_stop: the halving table needs a fixed number of simulations)"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    GumbelDev &gb = e->gb;
    hipStream_t st = (hipStream_t)stream;
    const int n = n_sims - 1;
    std::vector<int> table((size_t)(m + 1) * n);
    for (int mm = 0; mm <= m; mm++) gumbel_schedule(mm, n, table.data() + (size_t)mm * n);
    int *tab = nullptr;                                              // (a table of its own per call: a captured step graph may still hold the last one)
    HIPCHK(e, dalloc(e, &tab, table.size()));
    if (!gb.logit) {
        HIPCHK(e, dalloc(e, &gb.logit, (size_t)d.G * d.g.rc));
        HIPCHK(e, dalloc(e, &gb.v0, (size_t)d.G));
        HIPCHK(e, hipMemsetAsync(gb.logit, 0, sizeof(float) * (size_t)d.G * d.g.rc, st));
        HIPCHK(e, hipMemsetAsync(gb.v0, 0, sizeof(float) * (size_t)d.G, st));
    }
    HIPCHK(e, hipMemcpyAsync(tab, table.data(), sizeof(int) * table.size(), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipStreamSynchronize(st));
    gb.table = tab; gb.n = n; gb.c_visit = c_visit; gb.c_scale = c_scale;
    gb.m = m;
    e->gumbel_sims = n_sims;
    return AZK_OK;
}

int32_t azk_clear_gumbel_root(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_gumbel_root: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->gb.m = 0;                                                   // off: the engine launches what it launched before
    return AZK_OK;
}

// ---- configurable PUCT ----------------------------------------------------------------------------------------------------
int32_t azk_set_puct(azk_engine *e, const double *c_table_host, int32_t n_table, int32_t fpu_mode, double fpu_tree, double fpu_root, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_puct: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!c_table_host) { e->err = "azk_set_puct: c_table_host is null"; return AZK_ERR_ARG; }
    if (n_table < 1 || n_table > 65536) { e->err = "azk_set_puct: n_table must lie in [1, 65536]"; return AZK_ERR_ARG; }
    for (int i = 0; i < n_table; i++)
        if (!(c_table_host[i] >= 0.0) || c_table_host[i] - c_table_host[i] != 0.0) { e->err = "azk_set_puct: every table entry must be finite and not negative"; return AZK_ERR_ARG; }
    if (fpu_mode < 0 || fpu_mode > 2) { e->err = "azk_set_puct: fpu_mode must be 0 (as the reference), 1 (absolute) or 2 (parent value minus reduction)"; return AZK_ERR_ARG; }
    if (fpu_tree - fpu_tree != 0.0 || fpu_root - fpu_root != 0.0) { e->err = "azk_set_puct: the FPU parameters must be finite"; return AZK_ERR_ARG; }
    if (fpu_mode == 2 && (fpu_tree < 0.0 || fpu_root < 0.0)) { e->err = "azk_set_puct: a reduction (fpu_mode 2) must not be negative"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_puct: configurable PUCT does not combine with leaves_per_step > 1 (a virtual-loss search leaves losses in the value sums the FPU rule reads)"; return AZK_ERR_ARG; }
    if (e->forced_k != 0.0) { e->err = "azk_set_puct: forced playouts are set - their pruning bound restates the reference's selection formula"; return AZK_ERR_STATE; }
    if (e->gb.m) { e->err = "azk_set_puct: a Gumbel root is set - its root selection is not PUCT"; return AZK_ERR_STATE; }
    if (e->sv_on) { e->err = "azk_set_puct: the solver is set (azk_set_solver) - the two options' kernels are not combined (a follow-up, DESIGN section 29)"; return AZK_ERR_STATE; }
    if (e->in_search) { e->err = "azk_set_puct: a search is under way - set the option between searches"; return AZK_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    double *tab = nullptr;                                           // (a table of its own per call: a captured step graph may still hold the last one)
    HIPCHK(e, dalloc(e, &tab, (size_t)n_table));
    HIPCHK(e, hipMemcpyAsync(tab, c_table_host, sizeof(double) * (size_t)n_table, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipStreamSynchronize(st));
    e->pu = PuctDev{tab, n_table, fpu_mode, fpu_tree, fpu_root};
    e->puct_on = true;
    return AZK_OK;
}

int32_t azk_clear_puct(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_puct: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    if (e->in_search && e->puct_on) { e->err = "azk_clear_puct: a search is under way - clear the option between searches"; return AZK_ERR_STATE; }
    e->puct_on = false;                                            // off: the engine launches what it launched before
    return AZK_OK;
}

// ---- exact game-end proofs ------------------------------------------------------------------------------------------------
int32_t azk_set_solver(azk_engine *e, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_solver: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->d.K > 1) { e->err = "azk_set_solver: the solver does not combine with leaves_per_step > 1 (a virtual-loss search leaves losses on paths a proof would end)"; return AZK_ERR_ARG; }
    if (e->forced_k != 0.0) { e->err = "azk_set_solver: forced playouts are set - a forced child and a child shut out would claim the same selection"; return AZK_ERR_STATE; }
    if (e->gb.m) { e->err = "azk_set_solver: a Gumbel root is set - its eligibility rule needs raw root selection"; return AZK_ERR_STATE; }
    if (e->puct_on) { e->err = "azk_set_solver: configurable PUCT is set (azk_set_puct) - the two options' kernels are not combined (a follow-up, DESIGN section 29)"; return AZK_ERR_STATE; }
    if (e->ru.mode) { e->err = "azk_set_solver: the engine was created with tree_reuse != 0 - the status column is not carried through a re-rooting (a follow-up, DESIGN section 29)"; return AZK_ERR_STATE; }
    if (e->in_search) { e->err = "azk_set_solver: a search is under way - set the option between searches"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    SolverDev &s = e->sv;
    hipStream_t st = (hipStream_t)stream;
    if (!s.status) {
        HIPCHK(e, dalloc(e, &s.status, (size_t)d.G * (size_t)d.cap));
        HIPCHK(e, dalloc(e, &s.stats, (size_t)SST_N));
    }
    HIPCHK(e, hipMemsetAsync(s.status, 0, (size_t)d.G * (size_t)d.cap, st));
    HIPCHK(e, hipMemsetAsync(s.stats, 0, sizeof(long long) * SST_N, st));
    e->sv_on = true;
    return AZK_OK;
}

int32_t azk_clear_solver(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_solver: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    if (e->in_search && e->sv_on) { e->err = "azk_clear_solver: a search is under way - clear the option between searches"; return AZK_ERR_STATE; }
    e->sv_on = false;                                             // off: the engine launches what it launched before
    return AZK_OK;
}

int32_t azk_get_solver_status(azk_engine *e, int8_t *root_status_host, void *stream) {
    if (!e || !root_status_host) return AZK_ERR_ARG;
    if (!e->sv_on) { e->err = "azk_get_solver_status: no solver is set (azk_set_solver)"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    // one byte per game, a row of the column apart: the roots are node 0 of every arena
    HIPCHK(e, hipMemcpy2DAsync(root_status_host, 1, e->sv.status, (size_t)d.cap, 1, (size_t)d.G, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    for (int g = 0; g < d.G; g++) {                                // stored: as the player who moved INTO the root sees it; reported: as the side to move does
        const int s = (uint8_t)root_status_host[g];
        root_status_host[g] = (int8_t)(s == SOLVER_WON ? 2 : s == SOLVER_LOST ? 1 : s == SOLVER_DRAW ? 3 : 0);
    }
    return AZK_OK;
}

int32_t azk_get_solver_stats(azk_engine *e, int64_t *out6_host, void *stream) {
    if (!e || !out6_host) return AZK_ERR_ARG;
    if (!e->sv_on) { e->err = "azk_get_solver_stats: no solver is set (azk_set_solver)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out6_host, e->sv.stats, sizeof(long long) * SST_N, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_debug_fill_solver_status(azk_engine *e, int32_t byte, void *stream) {
    if (!e || byte < 0 || byte > 255) { if (e) e->err = "azk_debug_fill_solver_status: bad argument"; return AZK_ERR_ARG; }
    if (!e->sv_on) { e->err = "azk_debug_fill_solver_status: no solver is set (azk_set_solver)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemsetAsync(e->sv.status, byte, (size_t)e->d.G * (size_t)e->d.cap, (hipStream_t)stream));
    return AZK_OK;
}

// ---- move temperature -----------------------------------------------------------------------------------------------------
int32_t azk_set_move_temperature(azk_engine *e, const int32_t *row_of_ply_host, int32_t n_plies, const double *weights_host, int32_t n_rows, int32_t n_cols,
                                 int32_t visit_offset, double value_cutoff, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_move_temperature: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!row_of_ply_host || !weights_host) { e->err = "azk_set_move_temperature: a table pointer is null"; return AZK_ERR_ARG; }
    if (n_plies < 1 || n_rows < 1) { e->err = "azk_set_move_temperature: n_plies and n_rows must be at least 1"; return AZK_ERR_ARG; }
    if (n_cols != e->cfg.max_sims + 1) { e->err = "azk_set_move_temperature: n_cols must be max_sims + 1 (a weight for every visit count a root child can have)"; return AZK_ERR_ARG; }
    for (int p = 0; p < n_plies; p++)
        if (row_of_ply_host[p] < -1 || row_of_ply_host[p] >= n_rows) { e->err = "azk_set_move_temperature: a row index lies outside [-1, n_rows)"; return AZK_ERR_ARG; }
    const double wmax = DBL_MAX / ((double)n_rows * (double)n_cols);
    for (int r = 0; r < n_rows; r++) {
        const double *w = weights_host + (size_t)r * n_cols;
        bool positive = false;
        for (int c = 0; c < n_cols; c++) {
            if (!(w[c] >= 0.0) || w[c] - w[c] != 0.0) { e->err = "azk_set_move_temperature: every weight must be finite and not negative"; return AZK_ERR_ARG; }
            if (w[c] > wmax) { e->err = "azk_set_move_temperature: a weight exceeds DBL_MAX / (n_rows * n_cols) (the sum over a root's children must stay finite)"; return AZK_ERR_ARG; }
            positive = positive || w[c] > 0.0;
        }
        if (w[0] != 0.0) { e->err = "azk_set_move_temperature: column 0 of every row must be 0 (an unvisited child is never played)"; return AZK_ERR_ARG; }
        if (!positive) { e->err = "azk_set_move_temperature: a row has no positive weight"; return AZK_ERR_ARG; }
    }
    if (visit_offset < 0) { e->err = "azk_set_move_temperature: visit_offset must not be negative"; return AZK_ERR_ARG; }
    if (value_cutoff != value_cutoff) { e->err = "azk_set_move_temperature: value_cutoff is NaN (a negative value means no cutoff)"; return AZK_ERR_ARG; }
    if (e->in_search) { e->err = "azk_set_move_temperature: a search is under way - set the option between searches"; return AZK_ERR_STATE; }
    if (e->gb.m) { e->err = "azk_set_move_temperature: a Gumbel root is set - the Gumbel arg-max is the sample"; return AZK_ERR_STATE; }
    if (e->ru.mode == 1) { e->err = "azk_set_move_temperature: the engine was created with tree_reuse = 1 - a carried root child's visits are not bounded by max_sims, so the table has no column for them (top-up, tree_reuse = 2, is bounded)"; return AZK_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    int *rows = nullptr;                                             // (tables of their own per call: a captured step graph may still hold the last ones)
    double *wts = nullptr;
    HIPCHK(e, dalloc(e, &rows, (size_t)n_plies));
    HIPCHK(e, dalloc(e, &wts, (size_t)n_rows * n_cols));
    if (!e->tp.stats) HIPCHK(e, dalloc(e, &e->tp.stats, 4));
    HIPCHK(e, hipMemcpyAsync(rows, row_of_ply_host, sizeof(int) * (size_t)n_plies, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(wts, weights_host, sizeof(double) * (size_t)n_rows * n_cols, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemsetAsync(e->tp.stats, 0, sizeof(long long) * 4, st));
    HIPCHK(e, hipStreamSynchronize(st));
    e->tp = TempDev{rows, wts, n_plies, n_cols, visit_offset, value_cutoff, e->tp.stats};
    e->tp_on = true;
    return AZK_OK;
}

int32_t azk_clear_move_temperature(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_move_temperature: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->tp_on = false;                                             // off: the engine launches what it launched before
    return AZK_OK;
}

int32_t azk_get_move_temperature_stats(azk_engine *e, int64_t *out4_host, void *stream) {
    if (!e || !out4_host) return AZK_ERR_ARG;
    if (!e->tp_on) { e->err = "azk_get_move_temperature_stats: no move temperature is set (azk_set_move_temperature)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out4_host, e->tp.stats, sizeof(long long) * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

// ---- resignation ------------------------------------------------------------------------------------------------------
int32_t azk_set_resign(azk_engine *e, double v_resign, int32_t min_ply, double p_never, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_resign: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!(v_resign >= 0.0 && v_resign <= 1.0)) { e->err = "azk_set_resign: v_resign must lie in [0, 1] (0 = off)"; return AZK_ERR_ARG; }
    if (!(p_never >= 0.0 && p_never <= 1.0)) { e->err = "azk_set_resign: p_never must lie in [0, 1]"; return AZK_ERR_ARG; }
    if (min_ply < 0) { e->err = "azk_set_resign: min_ply must not be negative"; return AZK_ERR_ARG; }
    if (v_resign == 0.0) { e->rs.v_resign = 0.0; return AZK_OK; }  // off: the engine launches what it launched before
    if (e->d.K > 1) { e->err = "azk_set_resign: resignation does not combine with leaves_per_step > 1 (a virtual-loss search is another search: its q is not the one a threshold was set on)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    ResignDev &r = e->rs;
    if (!r.resigned) {
        HIPCHK(e, dalloc(e, &r.resigned, (size_t)d.G));
        HIPCHK(e, dalloc(e, &r.mark_start, (size_t)d.G));
        HIPCHK(e, dalloc(e, &r.mark_side, (size_t)d.G));
        HIPCHK(e, dalloc(e, &r.stats, 4));
    }
    const int32_t rc = azk_resign_clear(e, (hipStream_t)stream);
    if (rc != AZK_OK) return rc;
    r.min_ply = min_ply; r.p_never = p_never; r.seed = seed; r.first_game = first_global_game; r.rec_resigned = nullptr;
    r.v_resign = v_resign;
    return AZK_OK;
}

int32_t azk_get_resigned(azk_engine *e, uint8_t *resigned_dev, void *stream) {
    if (!e || !resigned_dev) return AZK_ERR_ARG;
    if (e->rs.v_resign == 0.0) { e->err = "azk_get_resigned: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(resigned_dev, e->rs.resigned, (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_resign_stats(azk_engine *e, int64_t *out4_host, void *stream) {
    if (!e || !out4_host) return AZK_ERR_ARG;
    if (e->rs.v_resign == 0.0) { e->err = "azk_get_resign_stats: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out4_host, e->rs.stats, sizeof(long long) * 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_resign_flags(azk_engine *e, uint8_t *rec_resigned_dev) {
    if (!e) return AZK_ERR_ARG;
    if (e->rs.v_resign == 0.0) { e->err = "azk_async_resign_flags: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_resign_flags: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->rs.rec_resigned = rec_resigned_dev;
    return AZK_OK;
}

// ---- policy surprise weighting ------------------------------------------------------------------------------------------
int32_t azk_set_surprise_weighting(azk_engine *e, double lambda, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_surprise_weighting: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->gb.m) { e->err = "azk_set_surprise_weighting: a Gumbel root is set - its recorded pi is not a visit distribution, which the weight is defined on"; return AZK_ERR_STATE; }
    if (!(lambda >= 0.0 && lambda <= 1.0)) { e->err = "azk_set_surprise_weighting: lambda must lie in [0, 1] (azk_clear_surprise_weighting switches the option off)"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_surprise_weighting: surprise weighting does not combine with leaves_per_step > 1 (a virtual-loss search's visit counts are not the ones the weight was defined on)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    if (!d.traj_pi) { e->err = "azk_set_surprise_weighting: the engine records no trajectories (a square board with one action per cell, or an engine created with emit_elements)"; return AZK_ERR_ARG; }
    SurpriseDev &s = e->sp;
    const size_t plies = (size_t)d.G * d.g.state_dim;
    if (!s.traj_kl) {
        HIPCHK(e, dalloc(e, &s.traj_kl, plies));
        HIPCHK(e, dalloc(e, &s.traj_coin, plies));
        HIPCHK(e, dalloc(e, &s.traj_copies, plies));
        HIPCHK(e, dalloc(e, &s.last_kl, (size_t)d.G));
        HIPCHK(e, dalloc(e, &s.last_coin, (size_t)d.G));
    }
    HIPCHK(e, hipMemsetAsync(s.traj_kl, 0, sizeof(double) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.traj_coin, 0, sizeof(double) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.traj_copies, 0, sizeof(uint16_t) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.last_kl, 0, sizeof(double) * (size_t)d.G, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(s.last_coin, 0, sizeof(double) * (size_t)d.G, (hipStream_t)stream));
    s.lambda = lambda; s.seed = seed; s.first_game = first_global_game; s.rec_kl = nullptr; s.rec_coin = nullptr;
    e->sp_on = true;
    return AZK_OK;
}

int32_t azk_clear_surprise_weighting(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_surprise_weighting: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->sp_on = false;                                             // off: the engine launches what it launched before
    return AZK_OK;
}

int32_t azk_get_surprise(azk_engine *e, double *kl_dev, double *coin_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (!e->sp_on) { e->err = "azk_get_surprise: no surprise weighting is set (azk_set_surprise_weighting)"; return AZK_ERR_STATE; }
    if (kl_dev) HIPCHK(e, hipMemcpyAsync(kl_dev, e->sp.last_kl, sizeof(double) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    if (coin_dev) HIPCHK(e, hipMemcpyAsync(coin_dev, e->sp.last_coin, sizeof(double) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_surprise_columns(azk_engine *e, double *rec_kl_dev, double *rec_coin_dev) {
    if (!e) return AZK_ERR_ARG;
    if (!e->sp_on) { e->err = "azk_async_surprise_columns: no surprise weighting is set (azk_set_surprise_weighting)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_surprise_columns: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->sp.rec_kl = rec_kl_dev; e->sp.rec_coin = rec_coin_dev;
    return AZK_OK;
}

// ---- value targets ---------------------------------------------------------------------------------------------------------
int32_t azk_set_value_target(azk_engine *e, double r, double lam, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_value_target: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->gb.m) { e->err = "azk_set_value_target: a Gumbel root is set - its movers do not keep the per-ply q (a follow-up, DESIGN section 28)"; return AZK_ERR_STATE; }
    if (!(r >= 0.0 && r <= 1.0)) { e->err = "azk_set_value_target: r must lie in [0, 1] (azk_clear_value_target switches the option off)"; return AZK_ERR_ARG; }
    if (!(lam >= 0.0 && lam <= 1.0)) { e->err = "azk_set_value_target: lam must lie in [0, 1]"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_value_target: value targets do not combine with leaves_per_step > 1 (a virtual-loss search is another search: its q is not the one the target was defined on)"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    if (!d.traj_pi) { e->err = "azk_set_value_target: the engine records no trajectories (a square board with one action per cell, or an engine created with emit_elements)"; return AZK_ERR_ARG; }
    ValueDev &v = e->vt;
    const size_t plies = (size_t)d.G * d.g.state_dim;
    if (!v.traj_q) {
        HIPCHK(e, dalloc(e, &v.traj_q, plies));
        HIPCHK(e, dalloc(e, &v.traj_vt, plies));
    }
    HIPCHK(e, hipMemsetAsync(v.traj_q, 0, sizeof(double) * plies, (hipStream_t)stream));
    HIPCHK(e, hipMemsetAsync(v.traj_vt, 0, sizeof(double) * plies, (hipStream_t)stream));
    v.r = r; v.lam = lam;
    e->vt_on = true;
    return AZK_OK;
}

int32_t azk_clear_value_target(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_value_target: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->vt_on = false;                                             // off: the engine launches what it launched before
    return AZK_OK;
}

int32_t azk_get_value_record(azk_engine *e, double *q_out_dev, void *stream) {
    if (!e || !q_out_dev) return AZK_ERR_ARG;
    if (!e->vt_on) { e->err = "azk_get_value_record: no value target is set (azk_set_value_target)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(q_out_dev, e->vt.traj_q, sizeof(double) * (size_t)e->d.G * e->d.g.state_dim, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

// ---- random openings -------------------------------------------------------------------------------------------------------
int32_t azk_set_openings(azk_engine *e, double p_open, int32_t max_plies, int32_t spread, uint64_t seed, int64_t first_global_game, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_openings: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (!(p_open >= 0.0 && p_open <= 1.0)) { e->err = "azk_set_openings: p_open must lie in [0, 1] (azk_clear_openings switches the option off)"; return AZK_ERR_ARG; }
    if (max_plies < 1 || max_plies > e->d.g.state_dim - 1) { e->err = "azk_set_openings: max_plies must lie in [1, state_dim - 1]"; return AZK_ERR_ARG; }
    if (spread < -1) { e->err = "azk_set_openings: spread must be -1 (the whole board) or >= 0"; return AZK_ERR_ARG; }
    const Dev &d = e->d;
    OpenDev &o = e->op;
    hipStream_t st = (hipStream_t)stream;
    if (!o.pending) {
        HIPCHK(e, dalloc(e, &o.pending, (size_t)d.G));
        HIPCHK(e, dalloc(e, &o.open_plies, (size_t)d.G));
        HIPCHK(e, dalloc(e, &o.stats, 3));
        HIPCHK(e, dalloc(e, &o.actions, (size_t)d.G * d.g.state_dim));
    }
    // every slot is looked at by the next azk_open_pending (or azk_async_begin), which opens the games that have not started yet
    HIPCHK(e, hipMemsetAsync(o.pending, 1, (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(o.open_plies, 0, sizeof(int) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(o.stats, 0, sizeof(long long) * 3, st));
    o.p_open = p_open; o.max_plies = max_plies; o.spread = spread; o.seed = seed; o.first_game = first_global_game;
    e->op_on = true;
    return AZK_OK;
}

int32_t azk_clear_openings(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_openings: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    e->op_on = false;                                             // off: the engine launches what it launched before
    return AZK_OK;
}

// ---- root noise on the legal moves ------------------------------------------------------------------------------------------
int32_t azk_set_root_noise(azk_engine *e, int32_t mode, double alpha, void *stream) {
    (void)stream;                                                 // (nothing is allocated or written here: an asynchronous engine's row_key at azk_async_begin)
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_root_noise: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->in_search) { e->err = "azk_set_root_noise: a search is under way - its row was made under the setting as it stood"; return AZK_ERR_STATE; }
    if (mode != 1 && mode != 2) { e->err = "azk_set_root_noise: mode must be 1 (legal: alpha per legal move) or 2 (total: alpha / legal moves)"; return AZK_ERR_ARG; }
    if (!(alpha > 0.0) || alpha - alpha != 0.0) { e->err = "azk_set_root_noise: alpha must be finite and positive"; return AZK_ERR_ARG; }
    if (e->gb.m) { e->err = "azk_set_root_noise: a Gumbel root is set - its rows are Gumbel rows, not Dirichlet rows"; return AZK_ERR_STATE; }
    e->rn.mode = mode; e->rn.alpha = alpha;
    return AZK_OK;
}

int32_t azk_clear_root_noise(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_root_noise: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    if (e->in_search) { e->err = "azk_clear_root_noise: a search is under way"; return AZK_ERR_STATE; }
    e->rn.mode = 0;                                               // off: the engine launches what it launched before
    return AZK_OK;
}

// ---- adaptive search budgets: the KLD rule and the lead rule ------------------------------------------------------------------
// what both rules keep per game (left, run, the checkpoint count), allocated by whichever is set first and cleared by either setter: no search
// is armed, a game counts as over (ckpt < 0) until its next search begins.  Both rules' counters are allocated here so that the judge's
// argument block never holds a null counter pointer; each setter clears its own.
static int32_t adaptive_common(azk_engine *e, hipStream_t st) {
    const Dev &d = e->d;
    KldDev &k = e->kd;
    if (!k.left) {
        HIPCHK(e, dalloc(e, &k.left, (size_t)d.G));
        HIPCHK(e, dalloc(e, &k.run, (size_t)d.G));
        HIPCHK(e, dalloc(e, &k.ckpt, (size_t)d.G));
        HIPCHK(e, dalloc(e, &k.stats, (size_t)KST_N));
        HIPCHK(e, dalloc(e, &k.lead_stats, (size_t)LST_N));
        HIPCHK(e, hipMemsetAsync(k.stats, 0, sizeof(long long) * KST_N, st));
        HIPCHK(e, hipMemsetAsync(k.lead_stats, 0, sizeof(long long) * LST_N, st));
    }
    HIPCHK(e, hipMemsetAsync(k.left, 0, sizeof(int) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(k.run, 0, sizeof(int) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(k.ckpt, 0xff, sizeof(int) * (size_t)d.G, st));
    k.max_children = d.g.rc; k.rec_sims = nullptr;
    return AZK_OK;
}

int32_t azk_set_kld_stop(azk_engine *e, int32_t interval, double min_gain, int32_t min_sims, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_kld_stop: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->in_search) { e->err = "azk_set_kld_stop: a search is under way - set the option between searches"; return AZK_ERR_STATE; }
    if (interval < 1 || interval > e->cfg.max_sims) { e->err = "azk_set_kld_stop: interval must lie in [1, max_sims]"; return AZK_ERR_ARG; }
    if (!(min_gain > 0.0) || min_gain - min_gain != 0.0) { e->err = "azk_set_kld_stop: min_gain must be finite and positive"; return AZK_ERR_ARG; }
    if (min_sims < 0) { e->err = "azk_set_kld_stop: min_sims must not be negative"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_kld_stop: adaptive search budgets do not combine with leaves_per_step > 1 (a virtual-loss search has several leaves in flight: no checkpoint finds its tree complete)"; return AZK_ERR_ARG; }
    if (e->gb.m) { e->err = "azk_set_kld_stop: a Gumbel root is set - its halving table needs a fixed number of simulations"; return AZK_ERR_STATE; }
    if (e->lead_on && interval != e->kd.interval) { e->err = "azk_set_kld_stop: the lead rule is set with another interval (azk_set_lead_stop) - the two rules share one"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    KldDev &k = e->kd;
    hipStream_t st = (hipStream_t)stream;
    int32_t rc = adaptive_common(e, st);
    if (rc != AZK_OK) return rc;
    if (!k.snap) {
        HIPCHK(e, dalloc(e, &k.snap_sum, (size_t)d.G));
        HIPCHK(e, dalloc(e, &k.snap, (size_t)d.G * d.g.rc));
        HIPCHK(e, dalloc(e, &k.rate, (size_t)d.G));
    }
    HIPCHK(e, hipMemsetAsync(k.snap_sum, 0, sizeof(int) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(k.snap, 0, sizeof(int) * (size_t)d.G * d.g.rc, st));
    HIPCHK(e, hipMemsetAsync(k.rate, 0, sizeof(double) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(k.stats, 0, sizeof(long long) * KST_N, st));
    k.interval = interval; k.min_gain = min_gain; k.min_sims = min_sims;
    e->kld_on = true;
    return AZK_OK;
}

int32_t azk_clear_kld_stop(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_kld_stop: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    if (e->in_search && e->kld_on) { e->err = "azk_clear_kld_stop: a search is under way - clear the option between searches"; return AZK_ERR_STATE; }
    e->kld_on = false;                                            // off: the engine launches what it launched before (or, with the lead rule
    e->kd.min_gain = 0.0;                                         // still set, the judge without its KLD part)
    return AZK_OK;
}

// the lead rule: set, clear, read.  The refusals are azk_set_kld_stop's.
int32_t azk_set_lead_stop(azk_engine *e, int32_t interval, double factor, int32_t min_sims, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_set_lead_stop: set it before azk_async_begin"; return AZK_ERR_STATE; }
    if (e->in_search) { e->err = "azk_set_lead_stop: a search is under way - set the option between searches"; return AZK_ERR_STATE; }
    if (interval < 1 || interval > e->cfg.max_sims) { e->err = "azk_set_lead_stop: interval must lie in [1, max_sims]"; return AZK_ERR_ARG; }
    if (!(factor > 0.0) || factor - factor != 0.0) { e->err = "azk_set_lead_stop: factor must be finite and positive"; return AZK_ERR_ARG; }
    if (min_sims < 0) { e->err = "azk_set_lead_stop: min_sims must not be negative"; return AZK_ERR_ARG; }
    if (e->d.K > 1) { e->err = "azk_set_lead_stop: adaptive search budgets do not combine with leaves_per_step > 1 (a virtual-loss search has several leaves in flight: no checkpoint finds its tree complete)"; return AZK_ERR_ARG; }
    if (e->gb.m) { e->err = "azk_set_lead_stop: a Gumbel root is set - its halving table needs a fixed number of simulations"; return AZK_ERR_STATE; }
    if (e->kld_on && interval != e->kd.interval) { e->err = "azk_set_lead_stop: the KLD rule is set with another interval (azk_set_kld_stop) - the two rules share one"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    KldDev &k = e->kd;
    hipStream_t st = (hipStream_t)stream;
    int32_t rc = adaptive_common(e, st);
    if (rc != AZK_OK) return rc;
    if (!k.lead_rec) HIPCHK(e, dalloc(e, &k.lead_rec, (size_t)d.G * 3));
    HIPCHK(e, hipMemsetAsync(k.lead_rec, 0, sizeof(int) * (size_t)d.G * 3, st));
    HIPCHK(e, hipMemsetAsync(k.lead_stats, 0, sizeof(long long) * LST_N, st));
    k.interval = interval; k.lead_factor = factor; k.lead_min_sims = min_sims;
    e->lead_on = true;
    return AZK_OK;
}

int32_t azk_clear_lead_stop(azk_engine *e) {
    if (!e) return AZK_ERR_ARG;
    if (e->async_on) { e->err = "azk_clear_lead_stop: the asynchronous movers are running (the option is fixed at azk_async_begin)"; return AZK_ERR_STATE; }
    if (e->in_search && e->lead_on) { e->err = "azk_clear_lead_stop: a search is under way - clear the option between searches"; return AZK_ERR_STATE; }
    e->lead_on = false;
    e->kd.lead_factor = 0.0;
    return AZK_OK;
}

int32_t azk_get_lead(azk_engine *e, int32_t *lead_dev, void *stream) {
    if (!e || !lead_dev) return AZK_ERR_ARG;
    if (!e->lead_on) { e->err = "azk_get_lead: no lead rule is set (azk_set_lead_stop)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(lead_dev, e->kd.lead_rec, sizeof(int) * (size_t)e->d.G * 3, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_lead_stats(azk_engine *e, int64_t *out5_host, void *stream) {
    if (!e || !out5_host) return AZK_ERR_ARG;
    if (!e->lead_on) { e->err = "azk_get_lead_stats: no lead rule is set (azk_set_lead_stop)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out5_host, e->kd.lead_stats, sizeof(long long) * LST_N, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_search_sims(azk_engine *e, int32_t *sims_dev, void *stream) {
    if (!e || !sims_dev) return AZK_ERR_ARG;
    if (!adaptive_on(e)) { e->err = "azk_get_search_sims: no adaptive search budget is set (azk_set_kld_stop / azk_set_lead_stop)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(sims_dev, e->kd.run, sizeof(int) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_kld_rate(azk_engine *e, double *rate_dev, void *stream) {
    if (!e || !rate_dev) return AZK_ERR_ARG;
    if (!e->kld_on) { e->err = "azk_get_kld_rate: no adaptive search budget is set (azk_set_kld_stop)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(rate_dev, e->kd.rate, sizeof(double) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_kld_stats(azk_engine *e, int64_t *out4_host, void *stream) {
    if (!e || !out4_host) return AZK_ERR_ARG;
    if (!e->kld_on) { e->err = "azk_get_kld_stats: no adaptive search budget is set (azk_set_kld_stop)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out4_host, e->kd.stats, sizeof(long long) * KST_N, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_async_sims_column(azk_engine *e, int32_t *rec_sims_dev) {
    if (!e) return AZK_ERR_ARG;
    if (!adaptive_on(e)) { e->err = "azk_async_sims_column: no adaptive search budget is set (azk_set_kld_stop / azk_set_lead_stop)"; return AZK_ERR_STATE; }
    if (e->async_on) { e->err = "azk_async_sims_column: call it before azk_async_begin"; return AZK_ERR_STATE; }
    e->kd.rec_sims = rec_sims_dev;
    return AZK_OK;
}

int32_t azk_get_open_plies(azk_engine *e, int32_t *open_plies_dev, void *stream) {
    if (!e || !open_plies_dev) return AZK_ERR_ARG;
    if (!e->op_on) { e->err = "azk_get_open_plies: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(open_plies_dev, e->op.open_plies, sizeof(int) * (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_opening_actions(azk_engine *e, int16_t *actions_dev, void *stream) {
    if (!e || !actions_dev) return AZK_ERR_ARG;
    if (!e->op_on) { e->err = "azk_get_opening_actions: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(actions_dev, e->op.actions, sizeof(int16_t) * (size_t)e->d.G * e->d.g.state_dim, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_leaf_flags(azk_engine *e, uint8_t *flags_dev, void *stream) {
    if (!e || !flags_dev) return AZK_ERR_ARG;
    HIPCHK(e, hipMemcpyAsync(flags_dev, e->d.leaf_flag, (size_t)e->d.G * e->d.K, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_opening_stats(azk_engine *e, int64_t *out3_host, void *stream) {
    if (!e || !out3_host) return AZK_ERR_ARG;
    if (!e->op_on) { e->err = "azk_get_opening_stats: no openings are set (azk_set_openings)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out3_host, e->op.stats, sizeof(long long) * 3, hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    return AZK_OK;
}

}  // extern "C"
