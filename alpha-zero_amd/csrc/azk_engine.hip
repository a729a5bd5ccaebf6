// azk_engine.hip - the kernel-free part of the C ABI declared in include/azk.h: engine creation and teardown, geometry, positions in
// and out, the eval cache's reset, tree export, counters' reset, debug stamps and the device error word.  The kernels and the calls that
// launch them live with their families: azk_tree.hip (search step), azk_vanilla.hip, azk_rules.hip (stateless rules), azk_begin.hip (games and
// searches start), azk_moves.hip (searches end: the moves, the asynchronous movers), azk_emit.hip (replay emission), azk_noise.hip; the
// options' kernel-free state calls are azk_options.hip.  azk_engine_int.h is what they share.
#include "azk_engine_int.h"
#include "azk_sym_map.h"      // the elements a geometry admits (emit_elements)

thread_local std::string azk_create_error;

extern "C" {

int32_t azk_abi_version(void) { return AZK_ABI_VERSION; }

const char *azk_last_error(const azk_engine *e) { return e ? e->err.c_str() : azk_create_error.c_str(); }

int32_t azk_create(const azk_config *cfg, azk_engine **out) {
    if (!cfg || !out) { azk_create_error = "null argument"; return AZK_ERR_ARG; }
    *out = nullptr;
    azk_engine *e = new azk_engine();
    e->cfg = *cfg;
    Dev &d = e->d;
    memset(&d, 0, sizeof d);
    memset(&e->ad, 0, sizeof e->ad);
    memset(&e->ru, 0, sizeof e->ru);
    auto fail = [&](int code, const std::string &msg) { azk_create_error = msg; azk_destroy(e); return code; };
    std::string gerr;
    if (!make_game(cfg->game, cfg->rows, cfg->cols, &d.g, &gerr)) return fail(AZK_ERR_ARG, gerr);
    if (cfg->n_games < 1 || cfg->max_sims < 1) return fail(AZK_ERR_ARG, "n_games and max_sims must be >= 1");
    if (cfg->leaf_dtype != AZK_LEAF_F32 && cfg->leaf_dtype != AZK_LEAF_BF16) return fail(AZK_ERR_ARG, "bad leaf_dtype");
    if (cfg->leaves_per_step < 0 || cfg->leaves_per_step > 64) return fail(AZK_ERR_ARG, "leaves_per_step must be 0..64");
    const int tree_reuse = cfg->tree_reuse;
    if (tree_reuse < 0 || tree_reuse > 2) return fail(AZK_ERR_ARG, "tree_reuse must be 0 (off), 1 (carry) or 2 (top-up)");
    if (tree_reuse != 0 && cfg->leaves_per_step > 1) return fail(AZK_ERR_ARG, "tree_reuse does not combine with leaves_per_step > 1 (virtual loss)");
    if (cfg->emit_elements != 0) {
        if (const char *bad = sym_mask_error((uint32_t)cfg->emit_elements, d.g.rows, d.g.cols, d.g.action_dim)) return fail(AZK_ERR_ARG, std::string("emit_elements: ") + bad);
        e->emit.els = sym_pack((uint32_t)cfg->emit_elements, &e->emit.n);
    }
    if (cfg->cache_entries < 0 || (cfg->cache_entries & (cfg->cache_entries - 1)) != 0) return fail(AZK_ERR_ARG, "cache_entries must be 0 or a power of two");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1)
        return fail(AZK_ERR_HIP, "no HIP device visible: libazk needs an MI355X (there is no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(AZK_ERR_ARG, "bad device ordinal");
    if (hipSetDevice(cfg->device) != hipSuccess) return fail(AZK_ERR_HIP, "hipSetDevice failed");
    { int khz = 0; if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, cfg->device) == hipSuccess && khz >= 1000) e->ticks_per_us = khz / 1000; }
    const GameDesc &g = d.g;
    const int maxch = g.kind == AZK_CONNECT4 ? g.cols : g.rc;
    // carry mode: the root's visits grow beyond max_sims from move to move, so the default arena holds a kept subtree of max_sims
    // expansions plus the max_sims new ones (the arena rule of include/azk.h drops a larger subtree)
    long long cap = cfg->arena_nodes > 0 ? cfg->arena_nodes : 1 + (long long)(tree_reuse == 1 ? 2 : 1) * cfg->max_sims * maxch;
    if (cap > 0x7ffffff0LL) return fail(AZK_ERR_ARG, "arena too large");
    d.G = cfg->n_games; d.cap = (int)cap; d.path_cap = g.state_dim + 2; d.rc_pad = up16(g.rc);
    d.leaf_dtype = cfg->leaf_dtype; d.table_size = table_size_for(g);
    { const char *ab = getenv("AZK_TREE_ABLATE"); d.ablate = ab ? atoi(ab) : 0; }
    int off[LDS_REGIONS];
    d.lds_bytes = lds_layout(g, d.path_cap, d.table_size, off);
    for (int i = 0; i < LDS_REGIONS_DEV; i++) d.lds_off[i] = off[i];
    const size_t G = d.G, nodes = G * (size_t)d.cap;
    hipError_t s = hipSuccess;
#define DA(ptr, count) if (s == hipSuccess) s = dalloc(e, &ptr, (count))
    DA(d.cells, G * d.rc_pad); DA(d.to_move, G); DA(d.move_count, G); DA(d.done, G); DA(d.winner, G);
    DA(d.H, nodes); DA(d.W, nodes); DA(d.Q, nodes);
    DA(d.rootP, G * g.rc); DA(d.root_f64, G); DA(d.arena_top, G);
    e->ru.mode = tree_reuse;
    if (tree_reuse) {
        e->ru.words = (d.cap + 63) / 64;
        DA(e->ru.chosen_node, G); DA(e->ru.bits, G * (size_t)e->ru.words); DA(e->ru.pre, G * (size_t)e->ru.words);
    }
    d.K = cfg->leaves_per_step > 1 ? cfg->leaves_per_step : 1;
    const size_t GV = G * (size_t)d.K;                            // pending-leaf slots
    DA(d.leaf_node, GV); DA(d.leaf_depth, GV); DA(d.leaf_nmoves, GV); DA(d.leaf_slot, GV); DA(d.to_move_v, GV);
    DA(d.path, GV * d.path_cap); DA(d.leaf_cells, GV * d.rc_pad); DA(d.leaf_moves, GV * g.rc);
    DA(d.leaf_flag, ((GV + 511) / 512) * 512 + 512);
    DA(d.counters, (size_t)CNT_N * G); DA(d.err, 1); DA(d.dbg, G * 8); DA(d.emit_base, G); DA(d.sims_done, G); DA(d.budget, 4);
    d.cache_entries = cfg->cache_entries;
    d.key_words = 2 * ((g.rc + 64) / 64);                         // one spare bit (63 of the last own-plane word) for the side to move
    d.cache_shared = (d.cache_entries && cfg->cache_shared) ? 1 : 0;
    size_t cache_total = G * (size_t)d.cache_entries;
    if (d.cache_shared) {
        size_t p2 = 1;
        while (p2 * 2 <= cache_total && p2 * 2 <= (size_t)1 << 30) p2 *= 2;       // entry indices travel as int32
        cache_total = p2;
        d.cache_mask = (unsigned long long)cache_total - 1ull;
    }
    if (d.cache_entries) {
        DA(d.cache_key, cache_total * d.key_words); DA(d.cache_logits, cache_total * g.action_dim);
        DA(d.cache_value, cache_total); DA(d.leaf_cache, GV);
        if (d.cache_shared) {
            DA(d.cache_claim, cache_total); DA(d.cache_stamp, 1); DA(d.leaf_key, GV * d.key_words);
            DA(d.hit_logits, GV * g.action_dim); DA(d.hit_value, GV);
        }
    }
    if ((g.rows == g.cols && g.action_dim == g.rc) || e->emit.n) { DA(d.traj_action, G * g.state_dim); DA(d.traj_pi, G * g.state_dim * g.action_dim); } DA(e->counter_sums, CNT_N); DA(e->n_leaf_scratch, 1);
    if (s == hipSuccess) { uint8_t *ls = nullptr; s = dalloc(e, &ls, GV * g.planes * g.rc * 4); e->leaf_scratch = ls; }
#undef DA
    if (s != hipSuccess) return fail(AZK_ERR_HIP, std::string("hipMalloc: ") + hipGetErrorString(s));
    (void)hipMemset(d.leaf_flag, 0, ((GV + 511) / 512) * 512 + 512);
    (void)hipMemset(d.counters, 0, sizeof(long long) * CNT_N * G);
    (void)hipMemset(d.err, 0, sizeof(int));
    if (d.cache_entries) (void)hipMemset(d.cache_key, 0xff, sizeof(unsigned long long) * cache_total * d.key_words);   // all-ones = no position
    if (d.cache_shared) {
        (void)hipMemset(d.cache_claim, 0, sizeof(unsigned) * cache_total);
        const unsigned one = 1u;
        (void)hipMemcpy(d.cache_stamp, &one, sizeof one, hipMemcpyHostToDevice);
    }
    (void)hipMemset(d.dbg, 0, sizeof(long long) * G * 8);
    (void)hipMemset(d.leaf_node, 0xff, sizeof(int) * GV);
    if (azk_init_games(e) != AZK_OK) return fail(AZK_ERR_HIP, "init kernels: " + e->err);
    *out = e;
    return AZK_OK;
}

void azk_destroy(azk_engine *e) {
    if (!e) return;
    for (void *p : e->allocs) (void)hipFree(p);
    delete e;
}

int32_t azk_geometry(const azk_engine *e, int32_t *planes, int32_t *rows, int32_t *cols, int32_t *action_dim, int32_t *state_dim) {
    if (!e) return AZK_ERR_ARG;
    if (planes) *planes = e->d.g.planes;
    if (rows) *rows = e->d.g.rows;
    if (cols) *cols = e->d.g.cols;
    if (action_dim) *action_dim = e->d.g.action_dim;
    if (state_dim) *state_dim = e->d.g.state_dim;
    return AZK_OK;
}

int32_t azk_set_positions(azk_engine *e, int32_t first, int32_t count, const int8_t *cells_host,
                          const int32_t *to_move_host, const int32_t *move_count_host, void *stream) {
    if (!e || first < 0 || count < 1 || first + count > e->d.G || !cells_host || !to_move_host || !move_count_host) {
        if (e) e->err = "azk_set_positions: bad argument";
        return AZK_ERR_ARG;
    }
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    e->in_search = false;                  // a new position: whatever search was under way is over
    std::vector<uint8_t> padded((size_t)count * d.rc_pad, 0);
    std::vector<int> zeros(count, 0), win(count, -2);
    for (int i = 0; i < count; i++)
        for (int c = 0; c < d.g.rc; c++) {
            int8_t v = cells_host[(size_t)i * d.g.rc + c];
            if (v < 0 || v > 2) { e->err = "azk_set_positions: cell codes must be 0, 1 or 2"; return AZK_ERR_ARG; }
            padded[(size_t)i * d.rc_pad + c] = (uint8_t)v;
        }
    HIPCHK(e, hipMemcpyAsync(d.cells + (size_t)first * d.rc_pad, padded.data(), padded.size(), hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(d.to_move + first, to_move_host, sizeof(int) * count, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(d.move_count + first, move_count_host, sizeof(int) * count, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(d.done + first, zeros.data(), sizeof(int) * count, hipMemcpyHostToDevice, st));
    HIPCHK(e, hipMemcpyAsync(d.winner + first, win.data(), sizeof(int) * count, hipMemcpyHostToDevice, st));
    if (e->ru.chosen_node) HIPCHK(e, hipMemsetAsync(e->ru.chosen_node + first, 0xff, sizeof(int) * count, st));   // a new position: its search starts from a fresh root
    HIPCHK(e, hipStreamSynchronize(st));   // host staging buffers go out of scope
    return AZK_OK;
}

int32_t azk_clear_cache(azk_engine *e, void *stream) {
    if (!e) return AZK_ERR_ARG;
    const Dev &d = e->d;
    if (!d.cache_entries) return AZK_OK;
    if (d.cache_shared) {       // an entry whose claim word is 0 was never written: clearing the claims empties the table
        HIPCHK(e, hipMemsetAsync(d.cache_claim, 0, sizeof(unsigned) * (size_t)(d.cache_mask + 1ull), (hipStream_t)stream));
        return AZK_OK;
    }
    HIPCHK(e, hipMemsetAsync(d.cache_key, 0xff, sizeof(unsigned long long) * (size_t)d.G * d.cache_entries * d.key_words, (hipStream_t)stream));
    return AZK_OK;
}

// copy one game's used arena to the host
struct HostTree {
    std::vector<int> N, first_child;
    std::vector<double> W, Q, rootP;
    std::vector<float> P;
    std::vector<uint32_t> meta;
    std::vector<int> cell, nch;
    int top = 0, root_f64 = 0;
};

static int32_t fetch_tree(azk_engine *e, int game, HostTree *t, hipStream_t st) {
    const Dev &d = e->d;
    if (game < 0 || game >= d.G) { e->err = "bad game index"; return AZK_ERR_ARG; }
    HIPCHK(e, hipMemcpyAsync(&t->top, d.arena_top + game, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(&t->root_f64, d.root_f64 + game, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    const size_t n = (size_t)t->top, base = (size_t)game * d.cap;
    t->N.resize(n); t->first_child.resize(n); t->W.resize(n); t->Q.resize(n); t->P.resize(n); t->cell.resize(n); t->nch.resize(n); t->meta.resize(n);
    t->rootP.resize(d.g.rc);
    std::vector<NodeH> recs(n);
    HIPCHK(e, hipMemcpyAsync(recs.data(), d.H + base, n * sizeof(NodeH), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(t->W.data(), d.W + base, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(t->Q.data(), d.Q + base, n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipMemcpyAsync(t->rootP.data(), d.rootP + (size_t)game * d.g.rc, d.g.rc * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    for (size_t i = 0; i < n; i++) { t->N[i] = recs[i].N; t->first_child[i] = recs[i].fc; t->P[i] = recs[i].P; t->meta[i] = recs[i].meta; }
    for (size_t i = 0; i < n; i++) {
        const int c = (int)(t->meta[i] >> 16);
        t->cell[i] = c == 0xffff ? -1 : c;
        t->nch[i] = (int)(t->meta[i] & 0xffffu);
    }
    return AZK_OK;
}

int32_t azk_root_children(azk_engine *e, int32_t game, int32_t cap, int32_t *cells_host, int32_t *visits_host,
                          double *values_host, double *priors_host, void *stream) {
    if (!e) return AZK_ERR_ARG;
    HostTree t;
    int32_t rc = fetch_tree(e, game, &t, (hipStream_t)stream);
    if (rc != AZK_OK) return rc;
    const int fc = t.first_child[0], n = t.nch[0];
    for (int i = 0; i < n && i < cap; i++) {
        if (cells_host) cells_host[i] = t.cell[fc + i];
        if (visits_host) visits_host[i] = t.N[fc + i];
        if (values_host) values_host[i] = t.W[fc + i];
        if (priors_host) priors_host[i] = t.root_f64 ? t.rootP[i] : (double)t.P[fc + i];
    }
    return n;
}

// azk_export_tree and azk_export_tree_quotients: one walk, the second with the Q column beside the others
static int32_t export_tree_rows(azk_engine *e, int32_t game, int32_t cap, int32_t *depth_host, int32_t *cell_host,
                                int32_t *visit_host, double *value_host, double *prior_host, double *quotient_host, void *stream) {
    if (!e) return AZK_ERR_ARG;
    HostTree t;
    int32_t rc = fetch_tree(e, game, &t, (hipStream_t)stream);
    if (rc != AZK_OK) return rc;
    std::vector<std::pair<int, int>> stack;
    stack.push_back({0, 0});
    int m = 0;
    const int rfc = t.first_child[0];
    while (!stack.empty()) {
        auto [node, dep] = stack.back();
        stack.pop_back();
        if (m < cap) {
            if (depth_host) depth_host[m] = dep;
            if (cell_host) cell_host[m] = t.cell[node];
            if (visit_host) visit_host[m] = t.N[node];
            if (value_host) value_host[m] = t.W[node];
            if (quotient_host) quotient_host[m] = t.Q[node];
            if (prior_host) {
                const bool root_child = dep == 1 && t.root_f64;
                prior_host[m] = root_child ? t.rootP[node - rfc] : (double)t.P[node];
            }
        }
        m++;
        for (int i = t.nch[node] - 1; i >= 0; i--) stack.push_back({t.first_child[node] + i, dep + 1});
    }
    return m;
}

int32_t azk_export_tree(azk_engine *e, int32_t game, int32_t cap, int32_t *depth_host, int32_t *cell_host,
                        int32_t *visit_host, double *value_host, double *prior_host, void *stream) {
    return export_tree_rows(e, game, cap, depth_host, cell_host, visit_host, value_host, prior_host, nullptr, stream);
}

int32_t azk_export_tree_quotients(azk_engine *e, int32_t game, int32_t cap, int32_t *depth_host, int32_t *cell_host,
                                  int32_t *visit_host, double *value_host, double *prior_host, double *quotient_host, void *stream) {
    return export_tree_rows(e, game, cap, depth_host, cell_host, visit_host, value_host, prior_host, quotient_host, stream);
}

// the solver's status column in the same row order (azk_set_solver)
int32_t azk_export_tree_status(azk_engine *e, int32_t game, int32_t cap, uint8_t *status_host, void *stream) {
    if (!e || !status_host) return AZK_ERR_ARG;
    if (!e->sv_on) { e->err = "azk_export_tree_status: no solver is set (azk_set_solver)"; return AZK_ERR_STATE; }
    HostTree t;
    int32_t rc = fetch_tree(e, game, &t, (hipStream_t)stream);
    if (rc != AZK_OK) return rc;
    std::vector<uint8_t> col((size_t)t.top);
    HIPCHK(e, hipMemcpyAsync(col.data(), e->sv.status + (size_t)game * e->d.cap, col.size(), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    std::vector<int> stack;
    stack.push_back(0);
    int m = 0;
    while (!stack.empty()) {
        const int node = stack.back();
        stack.pop_back();
        if (m < cap) status_host[m] = col[node];
        m++;
        for (int i = t.nch[node] - 1; i >= 0; i--) stack.push_back(t.first_child[node] + i);
    }
    return m;
}

int32_t azk_debug_fill_quotients(azk_engine *e, int32_t byte, void *stream) {
    if (!e || byte < 0 || byte > 255) { if (e) e->err = "azk_debug_fill_quotients: bad argument"; return AZK_ERR_ARG; }
    HIPCHK(e, hipMemsetAsync(e->d.Q, byte, sizeof(double) * (size_t)e->d.G * (size_t)e->d.cap, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_get_positions(azk_engine *e, int8_t *cells_host, int32_t *to_move_host, int32_t *move_count_host, void *stream) {
    if (!e) return AZK_ERR_ARG;
    const Dev &d = e->d;
    hipStream_t st = (hipStream_t)stream;
    std::vector<uint8_t> padded((size_t)d.G * d.rc_pad);
    HIPCHK(e, hipMemcpyAsync(padded.data(), d.cells, padded.size(), hipMemcpyDeviceToHost, st));
    if (to_move_host) HIPCHK(e, hipMemcpyAsync(to_move_host, d.to_move, sizeof(int) * d.G, hipMemcpyDeviceToHost, st));
    if (move_count_host) HIPCHK(e, hipMemcpyAsync(move_count_host, d.move_count, sizeof(int) * d.G, hipMemcpyDeviceToHost, st));
    HIPCHK(e, hipStreamSynchronize(st));
    if (cells_host)
        for (int g = 0; g < d.G; g++) memcpy(cells_host + (size_t)g * d.g.rc, padded.data() + (size_t)g * d.rc_pad, d.g.rc);
    return AZK_OK;
}

int32_t azk_debug_stamps(azk_engine *e, int64_t *out8_host) {
    if (!e || !out8_host) return AZK_ERR_ARG;
    std::vector<long long> h((size_t)e->d.G * 8);
    if (hipMemcpy(h.data(), e->d.dbg, h.size() * sizeof(long long), hipMemcpyDeviceToHost) != hipSuccess) return AZK_ERR_HIP;
    for (int k = 0; k < 8; k++) { long long s = 0; for (int g = 0; g < e->d.G; g++) s += h[(size_t)g * 8 + k]; out8_host[k] = s; }
    { long long mx = 0; for (int g = 0; g < e->d.G; g++) if (h[(size_t)g * 8 + 7] > mx) mx = h[(size_t)g * 8 + 7]; if (getenv("AZK_STAMP_MAX")) out8_host[7] = mx; }
    return AZK_OK;
}

int32_t azk_debug_stamps_raw(azk_engine *e, int64_t *out_host, int32_t n_games) {
    if (!e || !out_host || n_games != e->d.G) return AZK_ERR_ARG;
    return hipMemcpy(out_host, e->d.dbg, (size_t)e->d.G * 8 * sizeof(long long), hipMemcpyDeviceToHost) == hipSuccess ? AZK_OK : AZK_ERR_HIP;
}

int32_t azk_reset_counters(azk_engine *e, void *stream) {
    if (!e) return AZK_ERR_ARG;
    HIPCHK(e, hipMemsetAsync(e->d.counters, 0, sizeof(long long) * CNT_N * e->d.G, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_check_device_error(azk_engine *e, void *stream) {
    if (!e) return AZK_ERR_ARG;
    int h = 0;
    HIPCHK(e, hipMemcpyAsync(&h, e->d.err, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(e, hipStreamSynchronize((hipStream_t)stream));
    if (h == AZK_ERR_ARENA_FULL) e->err = "tree arena full: raise azk_config.max_sims / arena_nodes";
    else if (h != 0) e->err = "device-side state error (search advanced without visits?)";
    return h;
}

}  // extern "C"
