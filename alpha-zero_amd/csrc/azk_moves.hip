// azk_moves.hip - a search ends and the game moves: root statistics, the recorded pi (pruned, or the Gumbel root's), the move of the
// lock-step driver (k_advance) and the asynchronous movers that make it per game inside the step (k_move_async), with the drain around
// them; the kernels and the C ABI calls that launch them (include/azk.h).  What starts the next search or game is azk_begin.hip, emission
// azk_emit.hip, the noise rows azk_noise.hip, the options' state azk_options.hip.  Built with -ffp-contract=off like every engine file.
#include "azk_moves_dev.h"

namespace {

// utils.get_probablity_distribution_of_children (utils.py:46-55), root.value / root.visit (gomoku.py:140)
__global__ __launch_bounds__(AZK_WAVE) void k_root_stats(Dev d, double *pi, double *q, int *root_visit) {
    const int g = blockIdx.x, lane = azk_lane();
    const size_t base = (size_t)g * d.cap;
    const int A = d.g.action_dim;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int fc = d.H[base].fc, nch = meta_nch(d.H[base].meta);
    for (int a = lane; a < A; a += AZK_WAVE) L.cnt[a] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        L.cnt[azk_action_idx(d.g, meta_cell(d.H[base + fc + i].meta))] = n;
        sum += n;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    if (pi) for (int a = lane; a < A; a += AZK_WAVE) pi[(size_t)g * A + a] = (double)L.cnt[a] / (double)sum;
    if (lane == 0) {
        if (q) q[g] = d.W[base] / (double)d.H[base].N;
        if (root_visit) root_visit[g] = d.H[base].N;
    }
}

// the lock-step mover's scalars: move_index is an argument only of the kernels of engines with a keyed option (resignation, surprise weighting)
template <bool KEYED> struct Ply { int sample_until; };
template <> struct Ply<true> { int sample_until, move_index; };

template <bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool TEMP, bool VALUE>
__global__ __launch_bounds__(AZK_WAVE) void k_advance(MovePack<Dev, CAP, RESIGN, FORCED, SURPRISE, TEMP, VALUE> a, const double *uniforms, Ply<RESIGN || SURPRISE> ply,
                                                       int *chosen, int *winner_out, int *done_out, int *chosen_node) {
    int move_index = 0;
    if constexpr (RESIGN || SURPRISE) move_index = ply.move_index;
    advance_body<CAP, RESIGN, FORCED, SURPRISE, false, TEMP, VALUE>(a, opt<CapDev>(a), opt<ResignDev>(a), move_index, uniforms, ply.sample_until, chosen, winner_out,
                                                                    done_out, chosen_node, opt<ForcedDev>(a), opt<SurpriseDev>(a), GumbelDev{}, opt<TempDev>(a),
                                                                    opt<ValueDev>(a));
}

// the lock-step mover of an engine with a Gumbel root (with or without resignation)
template <bool RESIGN>
__global__ __launch_bounds__(AZK_WAVE) void k_advance(GumbelPack<Dev, RESIGN> a, Ply<RESIGN> ply, int *chosen, int *winner_out, int *done_out) {
    int move_index = 0;
    if constexpr (RESIGN) move_index = ply.move_index;
    advance_body<false, RESIGN, false, false, true>(a, CapDev{}, opt<ResignDev>(a), move_index, nullptr, 0, chosen, winner_out, done_out, nullptr, ForcedDev{},
                                                    SurpriseDev{}, opt<GumbelDev>(a));
}

template <bool REROOT, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool TEMP, bool VALUE>
__global__ __launch_bounds__(AZK_WAVE) void k_move_async(Dev d, AsyncDev p, MovePack<ReuseDev, CAP, RESIGN, FORCED, SURPRISE, TEMP, VALUE> r) {
    move_async_body<REROOT, CAP, RESIGN, FORCED, SURPRISE, false, TEMP, VALUE>(d, p, r, opt<CapDev>(r), opt<ResignDev>(r), opt<ForcedDev>(r), opt<SurpriseDev>(r),
                                                                               GumbelDev{}, opt<TempDev>(r), opt<ValueDev>(r));
}

// the asynchronous mover of an engine with a Gumbel root (no re-rooting, no cap; with or without resignation)
template <bool RESIGN>
__global__ __launch_bounds__(AZK_WAVE) void k_move_async(Dev d, AsyncDev p, GumbelPack<ReuseDev, RESIGN> r) {
    move_async_body<false, false, RESIGN, false, false, true>(d, p, r, CapDev{}, opt<ResignDev>(r), ForcedDev{}, SurpriseDev{}, opt<GumbelDev>(r));
}

// drain, step 1: list the finished games (done == 1) - the emission and restart kernels work through the list only
__global__ void k_async_list(Dev d, AsyncDev p) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g < d.G && d.done[g] != 0) p.fin_list[atomicAdd(p.fin_count, 1)] = g;
}

// azk_root_policy_target: the pi the next move would record - k_root_stats' counts, pruned where the game's search is a forced one
__global__ __launch_bounds__(AZK_WAVE) void k_root_policy_target(Dev d, ForcedDev fp, double *pi) {
    const int g = blockIdx.x, lane = azk_lane();
    const size_t base = (size_t)g * d.cap;
    const int A = d.g.action_dim;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    for (int a = lane; a < A; a += AZK_WAVE) L.cnt[a] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        L.cnt[azk_action_idx(d.g, meta_cell(d.H[base + fc + i].meta))] = n;
        sum += n;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    if (nch > 0 && sum > 0 && forced_search(d, fp, g)) sum = prune_counts(d, L, g, fp.k);
    for (int a = lane; a < A; a += AZK_WAVE) pi[(size_t)g * A + a] = (double)L.cnt[a] / (double)sum;
}

// ... and of an engine with a Gumbel root: gumbel_target's row
__global__ __launch_bounds__(AZK_WAVE) void k_root_policy_target_gumbel(Dev d, GumbelDev gb, double *pi) {
    const int g = blockIdx.x, lane = azk_lane();
    const int A = d.g.action_dim;
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const bool searched = uniform_i32(meta_nch(d.H[(size_t)g * d.cap].meta)) > 0 && uniform_i32(d.root_f64[g]) != 0;
    if (searched) gumbel_target(d, L, g, gb);
    for (int a = lane; a < A; a += AZK_WAVE) pi[(size_t)g * A + a] = searched ? L.cdf[a] : 0.0;
}

}  // namespace

extern "C" {

int32_t azk_root_stats(azk_engine *e, double *pi_dev, double *q_dev, int32_t *root_visit_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    k_root_stats<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, pi_dev, q_dev, root_visit_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

// azk_advance and azk_advance_resign (move_index: the game coin's key, read on a resigning engine only)
static int32_t advance(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index, int32_t *chosen_cell_dev,
                       int32_t *winner_dev, int32_t *done_dev, void *stream) {
    const Dev &d = e->d;
    e->in_search = false;
    if (e->gb.m) {                                                // a Gumbel root: the Gumbel arg-max is the sample - no uniforms, no sample_until
        with_flags([&](auto resign) {
            Ply<resign.value> ply{0};
            if constexpr (resign.value) ply.move_index = move_index;
            k_advance<resign.value><<<d.G, AZK_WAVE, d.lds_bytes, (hipStream_t)stream>>>(
                GumbelPack<Dev, resign.value>{d, on<resign.value>(e->rs), on<true>(e->gb)}, ply, chosen_cell_dev, winner_dev, done_dev);
        }, e->rs.v_resign != 0.0);
        HIPCHK(e, hipGetLastError());
        return AZK_OK;
    }
    with_flags([&](auto cap, auto resign, auto forced, auto surprise, auto temp, auto value) {
        Ply<resign.value || surprise.value> ply{sample_until_move};
        if constexpr (resign.value || surprise.value) ply.move_index = move_index;
        k_advance<cap.value, resign.value, forced.value, surprise.value, temp.value, value.value><<<d.G, AZK_WAVE, d.lds_bytes, (hipStream_t)stream>>>(
            move_pack<cap.value, resign.value, forced.value, surprise.value, temp.value, value.value>(d, e), uniforms_dev, ply, chosen_cell_dev, winner_dev,
            done_dev, e->ru.chosen_node);
    }, e->cp.n_fast != 0, e->rs.v_resign != 0.0, e->forced_k != 0.0, e->sp_on, e->tp_on, e->vt_on);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_advance(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t *chosen_cell_dev,
                    int32_t *winner_dev, int32_t *done_dev, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->sp_on) { e->err = "azk_advance: surprise weighting is set - its moves are made by azk_advance_keyed (the ply coin needs the move index)"; return AZK_ERR_STATE; }
    if (e->rs.v_resign != 0.0) { e->err = "azk_advance: resignation is set - its moves are made by azk_advance_resign (the game coin needs the move index)"; return AZK_ERR_STATE; }
    return advance(e, uniforms_dev, sample_until_move, 0, chosen_cell_dev, winner_dev, done_dev, stream);
}

int32_t azk_advance_resign(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index, int32_t *chosen_cell_dev,
                           int32_t *winner_dev, int32_t *done_dev, void *stream) {
    if (!e || move_index < 0) { if (e) e->err = "azk_advance_resign: bad argument"; return AZK_ERR_ARG; }
    if (e->sp_on) { e->err = "azk_advance_resign: surprise weighting is set - its moves are made by azk_advance_keyed"; return AZK_ERR_STATE; }
    if (e->rs.v_resign == 0.0) { e->err = "azk_advance_resign: no resignation is set (azk_set_resign)"; return AZK_ERR_STATE; }
    return advance(e, uniforms_dev, sample_until_move, move_index, chosen_cell_dev, winner_dev, done_dev, stream);
}

int32_t azk_advance_keyed(azk_engine *e, const double *uniforms_dev, int32_t sample_until_move, int32_t move_index, int32_t *chosen_cell_dev,
                          int32_t *winner_dev, int32_t *done_dev, void *stream) {
    if (!e || move_index < 0) { if (e) e->err = "azk_advance_keyed: bad argument"; return AZK_ERR_ARG; }
    if (!e->sp_on) { e->err = "azk_advance_keyed: no surprise weighting is set (azk_set_surprise_weighting)"; return AZK_ERR_STATE; }
    return advance(e, uniforms_dev, sample_until_move, move_index, chosen_cell_dev, winner_dev, done_dev, stream);
}

int32_t azk_root_policy_target(azk_engine *e, double *pi_dev, void *stream) {
    if (!e || !pi_dev) return AZK_ERR_ARG;
    if (e->gb.m) k_root_policy_target_gumbel<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, e->gb, pi_dev);
    else if (e->forced_k == 0.0) k_root_stats<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, pi_dev, nullptr, nullptr);
    else k_root_policy_target<<<e->d.G, AZK_WAVE, e->d.lds_bytes, (hipStream_t)stream>>>(e->d, e->forced(), pi_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

// ---- asynchronous self-play ---------------------------------------------------------------------------------------------
static int32_t async_begin(azk_engine *e, const azk_async_config *c, void *stream, bool reuse) {
    if (!e || !c || !c->stats_dev || c->n_sims < 1 || c->n_sims > e->cfg.max_sims || c->max_sims_per_launch < 1 || !(c->alpha > 0.0)) {
        if (e) e->err = "azk_async_begin: bad argument";
        return AZK_ERR_ARG;
    }
    if (e->ru.mode && !reuse) { e->err = "azk_async_begin: a tree_reuse engine begins with azk_async_begin_reuse (games are parked and re-rooted in the drain)"; return AZK_ERR_STATE; }
    if (e->sv_on && reuse) { e->err = "azk_async_begin_reuse: the solver is set (azk_set_solver) - the status column is not carried through a re-rooting"; return AZK_ERR_STATE; }
    if (!e->ru.mode && reuse) { e->err = "azk_async_begin_reuse: the engine was created with tree_reuse = 0 (use azk_async_begin)"; return AZK_ERR_STATE; }
    if (c->record_capacity < 0 || (c->record_capacity > 0 && (!c->rec_meta_dev || !c->rec_q_dev || !c->rec_pi_dev))) { e->err = "azk_async_begin: record ring pointers missing"; return AZK_ERR_ARG; }
    if (e->cp.n_fast > c->n_sims) { e->err = "azk_async_begin: the playout cap's n_fast exceeds n_sims"; return AZK_ERR_ARG; }
    if (e->forced_k != 0.0 && !c->dirichlet) { e->err = "azk_async_begin: forced playouts are set - the searches need root noise (dirichlet = 1)"; return AZK_ERR_STATE; }
    if (e->gb.m && !c->dirichlet) { e->err = "azk_async_begin: a Gumbel root is set - the searches need their Gumbel rows (dirichlet = 1 makes the movers generate them)"; return AZK_ERR_STATE; }
    if (e->gb.m && reuse) { e->err = "azk_async_begin_reuse: a Gumbel root is set - it does not combine with re-rooting (the eligibility rule needs a fresh root)"; return AZK_ERR_STATE; }
    if (e->gb.m && c->n_sims != e->gumbel_sims) { e->err = "azk_async_begin: a Gumbel root is set - n_sims differs from the n_sims its halving table was built for (azk_set_gumbel_root)"; return AZK_ERR_STATE; }
    Dev &d = e->d;
    if (d.K > 1) { e->err = "azk_async_begin: asynchronous moves run the sequential search (leaves_per_step = 1)"; return AZK_ERR_ARG; }
    hipStream_t st = (hipStream_t)stream;
    AsyncDev &a = e->ad;
    if (!a.slot_moves) {
        HIPCHK(e, dalloc(e, &a.slot_moves, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.noise, (size_t)d.G * 2 * d.g.action_dim));
        HIPCHK(e, dalloc(e, &a.noise_key, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.todo_list, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.todo_count, 1));
        HIPCHK(e, dalloc(e, &a.fin_list, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.fin_count, 1));
    }
    if (reuse && !a.parked) {
        HIPCHK(e, dalloc(e, &a.parked, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.reroot_list, (size_t)d.G));
        HIPCHK(e, dalloc(e, &a.reroot_count, 1));
    }
    a.n_sims = c->n_sims; a.sample_until = c->sample_until_move; a.dirichlet = c->dirichlet ? 1 : 0;
    a.seed = c->seed; a.first_game = c->first_global_game; a.alpha = c->alpha;
    a.stats = (long long *)c->stats_dev; a.rec_cap = c->record_capacity; a.rec_meta = c->rec_meta_dev; a.rec_q = c->rec_q_dev; a.rec_pi = c->rec_pi_dev;
    e->async_recycle = c->recycle ? 1 : 0;
    HIPCHK(e, hipMemsetAsync(a.slot_moves, 0, sizeof(long long) * (size_t)d.G, st));
    HIPCHK(e, hipMemsetAsync(a.stats, 0, sizeof(long long) * 16, st));
    if (reuse) {                                                  // nothing parked, no child noted: every game's first search starts from a fresh root
        HIPCHK(e, hipMemsetAsync(a.parked, 0, sizeof(int) * (size_t)d.G, st));
        HIPCHK(e, hipMemsetAsync(a.reroot_count, 0, sizeof(int), st));
        HIPCHK(e, hipMemsetAsync(e->ru.chosen_node, 0xff, sizeof(int) * (size_t)d.G, st));
    }
    e->budget_host[0] = c->n_sims; e->budget_host[1] = c->max_sims_per_launch;
    e->budget_host[2] = c->young_launch_us > 0 ? c->young_launch_us * e->ticks_per_us : 0;
    if (const int32_t rc = upload_budget(e, st); rc != AZK_OK) return rc;
    d.noise = a.dirichlet ? a.noise : nullptr;
    d.noise_sel = a.dirichlet ? a.slot_moves : nullptr;
    e->multi = true;
    e->async_on = true;
    if (e->rs.v_resign != 0.0) {                                  // the game coins share the noise rows' key too
        e->rs.seed = a.seed; e->rs.first_game = a.first_game;
        const int32_t rc = azk_resign_clear(e, st);
        if (rc != AZK_OK) return rc;
    }
    if (e->sp_on) { e->sp.seed = a.seed; e->sp.first_game = a.first_game; }      // ... and the ply coins of surprise weighting
    // first search of every game: fresh roots + the Dirichlet rows of move keys 0 (this search) and 1 (the next one)
    if (e->cp.n_fast) { e->cp.seed = a.seed; e->cp.first_game = a.first_game; e->cp.stats = a.stats; }   // the coins share the noise rows' key: this run's seed and first game
    azk_launch_first_searches(e, st);
    HIPCHK(e, hipMemsetAsync(a.todo_count, 0, sizeof(int), st));
    if (a.dirichlet && e->rn.mode) {                              // root noise on the legal moves: the rows come from the positions, none is made ahead
        if (const int32_t rc = azk_root_noise_begin(e, st); rc != AZK_OK) return rc;
    } else if (a.dirichlet) azk_launch_first_rows(e, st);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

int32_t azk_async_begin(azk_engine *e, const azk_async_config *c, void *stream) { return async_begin(e, c, stream, false); }

int32_t azk_async_begin_reuse(azk_engine *e, const azk_async_config *c, void *stream) { return async_begin(e, c, stream, true); }

int32_t azk_async_step(azk_engine *e, const float *logits_dev, const float *values_dev, int32_t phases, void *stream) {
    if (!e || !e->async_on) { if (e) e->err = "azk_async_step: call azk_async_begin first"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    if (phases & 1) { const int32_t rc = azk_launch_tree(e, true, true, true, logits_dev, values_dev, st); if (rc != AZK_OK) return rc; }
    if ((phases & 2) && e->gb.m)
        with_flags([&](auto resign) {
            k_move_async<resign.value><<<d.G, AZK_WAVE, d.lds_bytes, st>>>(d, e->ad, GumbelPack<ReuseDev, resign.value>{e->ru, on<resign.value>(e->rs), on<true>(e->gb)});
        }, e->rs.v_resign != 0.0);
    else if ((phases & 2) && adaptive_on(e)) azk_launch_move_async_kld(e, st);     // adaptive search budgets, either rule: their movers (azk_moves_kld.hip)
    else if (phases & 2)
        with_flags([&](auto reroot, auto cap, auto resign, auto forced, auto surprise, auto temp, auto value) {
            k_move_async<reroot.value, cap.value, resign.value, forced.value, surprise.value, temp.value, value.value><<<d.G, AZK_WAVE, d.lds_bytes, st>>>(
                d, e->ad, move_pack<cap.value, resign.value, forced.value, surprise.value, temp.value, value.value>(e->ru, e));
        }, e->ru.mode != 0, e->cp.n_fast != 0, e->rs.v_resign != 0.0, e->forced_k != 0.0, e->sp_on, e->tp_on, e->vt_on);
    // root noise on the legal moves: a game that has just moved began its next search in the mover - its row, from the new position, before the
    // next tree launch; one more node of the linear chain.  (A re-rooting engine's moved games are parked: their rows are the drain's.)
    if ((phases & 2) && e->rn.mode && e->ad.dirichlet && !e->ru.mode) azk_launch_root_noise_due(e, st);
    HIPCHK(e, hipGetLastError());
    return azk_sym_leaves(e, st);                                // (eval symmetry: the leaves the tree launch selected, behind the movers)
}

int32_t azk_async_set_budget(azk_engine *e, int32_t n_sims, int32_t max_sims_per_launch, void *stream) {
    if (!e || !e->async_on || n_sims < 1 || n_sims > e->cfg.max_sims || max_sims_per_launch < 1) { if (e) e->err = "azk_async_set_budget: bad argument"; return AZK_ERR_ARG; }
    if (adaptive_on(e)) { e->err = "azk_async_set_budget: adaptive search budgets are set (azk_set_kld_stop / azk_set_lead_stop) - the running searches' segments are cut against the budget as it stood"; return AZK_ERR_STATE; }
    if (e->gb.m && n_sims != e->gumbel_sims) { e->err = "azk_async_set_budget: a Gumbel root is set - n_sims differs from the n_sims its halving table was built for"; return AZK_ERR_STATE; }
    e->budget_host[0] = n_sims; e->budget_host[1] = max_sims_per_launch;
    return upload_budget(e, (hipStream_t)stream);
}

int32_t azk_async_drain(azk_engine *e, float *states_dev, double *pis_dev, float *zs_dev, int64_t capacity, int64_t *cursor_dev, void *stream) {
    if (!e || !e->async_on) { if (e) e->err = "azk_async_drain: call azk_async_begin first"; return AZK_ERR_STATE; }
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    HIPCHK(e, hipMemsetAsync(e->ad.fin_count, 0, sizeof(int), st));
    k_async_list<<<(unsigned)((d.G + 255) / 256), 256, 0, st>>>(d, e->ad);
    if (states_dev) {
        if (!pis_dev || !zs_dev || !cursor_dev || capacity < 1 || !d.traj_pi) { e->err = "azk_async_drain: bad replay arguments"; return AZK_ERR_ARG; }
        azk_launch_emit(e, states_dev, pis_dev, zs_dev, (long long)capacity, (unsigned long long *)cursor_dev, nullptr, e->ad.fin_list, e->ad.fin_count, st);
    }
    if (const int32_t rc = azk_launch_next_searches(e, st); rc != AZK_OK) return rc;      // finished games restarted, parked games re-rooted
    if (e->ad.dirichlet) {                                        // the rows of the searches AFTER the ones begun since the last drain
        if (!e->rn.mode) azk_launch_rows_ahead(e, st);            // (root noise on the legal moves: azk_launch_next_searches has made the rows that are due)
        HIPCHK(e, hipMemsetAsync(e->ad.todo_count, 0, sizeof(int), st));
    }
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

}  // extern "C"
