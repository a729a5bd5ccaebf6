// azk_noise.hip - the rows of random numbers a search reads, made ahead of it: Dirichlet rows and move uniforms (k_gen_noise), Gumbel rows
// (k_gen_gumbel), both from azk_rng.h's generators; and the counters' sums.  The kernels and the C ABI calls that launch them (include/azk.h).
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

}  // namespace

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
