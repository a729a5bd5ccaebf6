// azk_replay.hip - azk_replay_gather (include/azk.h has the semantics, DESIGN section 22 the reasons): a training batch gathered from a
// replay ring, each row turned by the D4 element drawn for it - what DeviceReplay.sample(augment=...) launches instead of three torch
// gathers and a dtype conversion.  Stateless: no engine, the ring is the caller's.  One wave per output row, in the manner of k_sym_logits;
// any rows x cols of at most 400 cells, so a cell is split into row and column by division (the engine's reciprocal holds for <= 30 columns).
#include "azk_engine_int.h"
#include "azk_sym_map.h"      // sym_source, the elements a geometry admits

namespace {

struct GatherArgs {
    int rows, cols, rc, planes, action_dim;
    uint32_t valid;            // the mask's elements, four bits each, ascending, lowest first
    int n_valid;
    const float *states; const double *pis; const float *zs;
    const long long *idx; const int *draws;
    float *states_out, *pis_out, *zs_out;
};

// Q: cells / actions per lane and pass (a board of up to 64 * Q cells is one pass); the planes go three to a pass
template <int Q>
__global__ __launch_bounds__(AZK_WAVE) void k_replay_gather(GatherArgs p) {
    const int b = blockIdx.x, lane = azk_lane();
    const long long r = p.idx[b];
    const int draw = p.draws != nullptr ? p.draws[b] : 0;
    // the pick of k_sym_leaves; without draws ((0 >> 16) * n_valid) >> 16 = 0: the mask's first element, the identity
    const int el = (int)((p.valid >> (4 * ((((uint32_t)draw >> 16) * (uint32_t)p.n_valid) >> 16))) & 15u);
    const int rc = p.rc, F = p.planes, A = p.action_dim;
    const float *__restrict__ ss = p.states + (size_t)r * F * rc;
    float *__restrict__ so = p.states_out + (size_t)b * F * rc;
    const float z = p.zs[r];
    for (int c0 = 0; c0 < rc; c0 += AZK_WAVE * Q) {
        int src[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {                               // the row split is a division here: a caller's board may be wider than the
            const int j = min(c0 + lane + AZK_WAVE * q, rc - 1);   // engine's 30 columns (1 x 257, 2 x 195), where sym_source's reciprocal is off
            const int i = j / p.cols;
            src[q] = sym_source_rc(el, i, j - i * p.cols, p.rows, p.cols);
        }
        for (int f0 = 0; f0 < F; f0 += 3) {
            float v[3][Q];
#pragma unroll
            for (int k = 0; k < 3; k++) {                          // gather loads inside one row, all in flight together (clamped, unconditional)
                const float *pl = ss + (size_t)min(f0 + k, F - 1) * rc;
#pragma unroll
                for (int q = 0; q < Q; q++) v[k][q] = pl[src[q]];
            }
#pragma unroll
            for (int k = 0; k < 3; k++)
#pragma unroll
                for (int q = 0; q < Q; q++) {
                    const int j = c0 + lane + AZK_WAVE * q;
                    if (f0 + k < F && j < rc) so[(size_t)(f0 + k) * rc + j] = v[k][q];
                }
        }
    }
    // one action per cell: the cells' map; else Connect4's columns, a -> cols - 1 - a under lr: the same map on a board of one row (every
    // other action kind admits the identity alone)
    const bool cells = A == rc;
    const int R = cells ? p.rows : 1, C = cells ? p.cols : A;
    const double *__restrict__ ps = p.pis + (size_t)r * A;
    float *__restrict__ po = p.pis_out + (size_t)b * A;
    for (int a0 = 0; a0 < A; a0 += AZK_WAVE * Q) {
        double w[Q];
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int a = min(a0 + lane + AZK_WAVE * q, A - 1);
            const int i = cells ? a / C : 0;
            w[q] = ps[sym_source_rc(el, i, a - i * C, R, C)];
        }
#pragma unroll
        for (int q = 0; q < Q; q++) {
            const int a = a0 + lane + AZK_WAVE * q;
            if (a < A) po[a] = (float)w[q];                        // round to nearest even: torch's .float()
        }
    }
    if (lane == 0) p.zs_out[b] = z;
}

}  // namespace

extern "C" {

int32_t azk_replay_gather(int32_t rows, int32_t cols, int32_t planes, int32_t action_dim, uint32_t element_mask,
                          const float *states_ring, const double *pis_ring, const float *zs_ring,
                          const int64_t *idx_dev, const int32_t *draws_dev, int32_t n,
                          float *states_out, float *pis_out, float *zs_out, void *stream) {
    auto fail = [&](const char *msg) { azk_create_error = std::string("azk_replay_gather: ") + msg; return AZK_ERR_ARG; };
    if (rows < 1 || cols < 1 || planes < 1 || action_dim < 1) return fail("rows, cols, planes and action_dim must be >= 1");
    if ((long long)rows * cols > 400) return fail("a board has at most 400 cells");
    if (n < 0) return fail("n must not be negative");
    if (const char *bad = sym_mask_error(element_mask, rows, cols, action_dim)) return fail(bad);
    if (!states_ring || !pis_ring || !zs_ring || !idx_dev || !states_out || !pis_out || !zs_out) return fail("null pointer");
    if (n == 0) return AZK_OK;
    GatherArgs p;
    p.rows = rows; p.cols = cols; p.rc = rows * cols; p.planes = planes; p.action_dim = action_dim;
    p.valid = sym_pack(element_mask, &p.n_valid);
    p.states = states_ring; p.pis = pis_ring; p.zs = zs_ring;
    p.idx = (const long long *)idx_dev; p.draws = draws_dev;
    p.states_out = states_out; p.pis_out = pis_out; p.zs_out = zs_out;
    hipStream_t st = (hipStream_t)stream;
    const int widest = p.rc > action_dim ? p.rc : action_dim;
    if (widest <= AZK_WAVE) k_replay_gather<1><<<n, AZK_WAVE, 0, st>>>(p);
    else if (widest <= 2 * AZK_WAVE) k_replay_gather<2><<<n, AZK_WAVE, 0, st>>>(p);
    else if (widest <= 4 * AZK_WAVE) k_replay_gather<4><<<n, AZK_WAVE, 0, st>>>(p);
    else k_replay_gather<7><<<n, AZK_WAVE, 0, st>>>(p);
    if (hipGetLastError() != hipSuccess) { azk_create_error = "azk_replay_gather: launch failed"; return AZK_ERR_HIP; }
    return AZK_OK;
}

}  // extern "C"
