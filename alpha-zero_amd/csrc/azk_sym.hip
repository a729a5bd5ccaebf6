// azk_sym.hip - evaluation of the pending leaves under a board symmetry (azk_set_eval_symmetry; include/azk.h has the semantics, DESIGN
// section 21 the reasons): k_sym_leaves picks each flagged slot's element and writes its cells turned into that orientation, k_sym_logits
// turns the evaluator's rows back.  Both are one wave per pending-leaf slot and sit beside the search step: k_tree, k_gather and every
// evaluator kernel are the ones of an engine without the option - they are handed other pointers.
#include "azk_engine_int.h"
#include "azk_sym_map.h"      // sym_source, the elements a geometry admits

namespace {

enum { SYM_MAX_PER_LANE = 7 };       // make_game allows 400 cells / actions: 7 per lane

__device__ __forceinline__ uint32_t sym_fmix(uint32_t h) {    // murmur3's 32-bit finaliser
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return h;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {   // wave_sum_i32 modulo 2^32
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__device__ __forceinline__ int sym_inverse(int s) { return (int)((0x36547210u >> (4 * s)) & 7u); }   // rot90 <-> rot270, the others their own

__global__ __launch_bounds__(AZK_WAVE) void k_sym_leaves(Dev d, SymDev p) {
    const int g = blockIdx.x, lane = azk_lane();
    __shared__ uint32_t row[2 * AZK_WAVE];                        // the leaf's cells (rc_pad <= 400 bytes)
    const int rc = d.g.rc, nd = d.rc_pad >> 2;
    // everything whose address depends only on the slot, in one round trip (unconditional, clamped)
    const uint32_t *lw = (const uint32_t *)(d.leaf_cells + (size_t)g * d.rc_pad);
    const int k0 = lane, k1 = lane + AZK_WAVE;
    const uint32_t w0 = lw[min(k0, nd - 1)], w1 = lw[min(k1, nd - 1)];
    const int flag = d.leaf_flag[g], tm = d.to_move[g], dep = d.leaf_depth[g];
    asm volatile("" ::"v"(w0), "v"(w1), "v"(tm), "v"(dep));        // (keeps the loads in front of the exit: else the compiler sinks them behind the flag's round trip)
    if (!flag) return;
    int el = p.fixed;
    if (p.mode == 1) {
        uint32_t h = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t c0 = (w0 >> (8 * b)) & 0xffu, c1 = (w1 >> (8 * b)) & 0xffu;
            const int i0 = 4 * k0 + b, i1 = 4 * k1 + b;
            const uint32_t t0 = sym_fmix((((uint32_t)i0 << 2) | c0) ^ p.seed_lo), t1 = sym_fmix((((uint32_t)i1 << 2) | c1) ^ p.seed_lo);
            h += (c0 != 0 && i0 < rc) ? t0 : 0u;
            h += (c1 != 0 && i1 < rc) ? t1 : 0u;
        }
        const uint32_t side = (uint32_t)((tm + dep) & 1);
        h = wave_sum_u32(h) + sym_fmix(p.seed_hi ^ side ^ 0x9E3779B9u);
        const uint32_t r = sym_fmix(h);
        el = (int)((p.valid >> (4 * (((r >> 16) * (uint32_t)p.n_valid) >> 16))) & 15u);
    }
    if (lane == 0) p.leaf_sym[g] = (uint8_t)el;
    row[k0] = w0; row[k1] = w1;
    __syncthreads();
    const uint8_t *rb = (const uint8_t *)row;
    uint32_t *ow = (uint32_t *)(p.sym_cells + (size_t)g * d.rc_pad);
    uint32_t o0 = 0, o1 = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {                                 // padding bytes stay where they are
        const int j0 = 4 * k0 + b, j1 = 4 * k1 + b;
        const int s0 = j0 < rc ? sym_source(el, j0, d.g.rows, d.g.cols, d.g.inv_cols) : j0;
        const int s1 = j1 < rc ? sym_source(el, j1, d.g.rows, d.g.cols, d.g.inv_cols) : min(j1, 8 * AZK_WAVE - 1);
        o0 |= (uint32_t)rb[s0] << (8 * b);
        o1 |= (uint32_t)rb[s1] << (8 * b);
    }
    if (k0 < nd) ow[k0] = o0;
    if (k1 < nd) ow[k1] = o1;
}

// out[slot][a] = logits[slot][dst_s(a)] for every flagged slot; rows of no flagged slot are not touched
__global__ __launch_bounds__(AZK_WAVE) void k_sym_logits(Dev d, SymDev p, const float *__restrict__ logits, float *__restrict__ out) {
    const int g = blockIdx.x, lane = azk_lane();
    const int flag = d.leaf_flag[g], slot_raw = d.leaf_slot[g], el = p.leaf_sym[g] & 7;
    asm volatile("" ::"v"(slot_raw), "v"(el));                    // (one round trip for the three: see k_sym_leaves)
    if (!flag) return;
    const int A = d.g.action_dim;
    const int slot = min(max(slot_raw, 0), d.G * d.K - 1);
    const int inv = sym_inverse(el);
    // one action per cell; else Connect4's columns, a -> cols - 1 - a under lr: the same map on a board of one row (inv_cols 0: every a in row 0)
    const bool cells = A == d.g.rc;
    const int R = cells ? d.g.rows : 1, C = cells ? d.g.cols : A;
    const unsigned inv_cols = cells ? d.g.inv_cols : 0u;
    const float *src = logits + (size_t)slot * A;
    float v[SYM_MAX_PER_LANE];
#pragma unroll
    for (int q = 0; q < SYM_MAX_PER_LANE; q++) {                  // gather loads inside one row, all in flight together
        const int a = min(lane + AZK_WAVE * q, A - 1);
        v[q] = src[sym_source(inv, a, R, C, inv_cols)];
    }
#pragma unroll
    for (int q = 0; q < SYM_MAX_PER_LANE; q++) asm volatile("" ::"v"(v[q]));   // (every load issued before the first store's predicate)
    float *dst = out + (size_t)slot * A;
#pragma unroll
    for (int q = 0; q < SYM_MAX_PER_LANE; q++)
        if (lane + AZK_WAVE * q < A) dst[lane + AZK_WAVE * q] = v[q];
}

}  // namespace

int32_t azk_sym_leaves(azk_engine *e, hipStream_t st) {
    if (!e->sym.mode) return AZK_OK;
    k_sym_leaves<<<e->d.G, AZK_WAVE, 0, st>>>(e->d, e->sym);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

const float *azk_sym_restore(azk_engine *e, const float *logits, hipStream_t st) {
    if (!e->sym.mode || !logits) return logits;
    k_sym_logits<<<e->d.G, AZK_WAVE, 0, st>>>(e->d, e->sym, logits, e->sym.sym_logits);
    return e->sym.sym_logits;
}

extern "C" {

int32_t azk_set_eval_symmetry(azk_engine *e, int32_t mode, uint64_t seed_or_element, void *stream) {
    if (!e) return AZK_ERR_ARG;
    if (e->in_search || e->async_on) { e->err = "azk_set_eval_symmetry: a search is under way - set the option between searches (and before azk_async_begin)"; return AZK_ERR_ARG; }
    if (mode < 0 || mode > 2) { e->err = "azk_set_eval_symmetry: mode must be 0 (off), 1 (position-keyed) or 2 (one fixed element)"; return AZK_ERR_ARG; }
    if (mode == 0) { e->sym.mode = 0; return AZK_OK; }          // off: the engine launches what it launched before
    const Dev &d = e->d;
    if (d.K > 1) { e->err = "azk_set_eval_symmetry: does not combine with leaves_per_step > 1 (the virtual-loss schedule is not pinned under it)"; return AZK_ERR_ARG; }
    SymDev &s = e->sym;
    const GameDesc &g = d.g;
    int n_valid;
    const uint32_t valid = sym_pack(sym_valid_mask(g.rows, g.cols, g.action_dim), &n_valid);    // Connect4 {rot0, lr}; rows != cols: the elements that keep the shape
    if (mode == 2) {
        bool ok = false;
        for (int i = 0; i < n_valid; i++) ok = ok || seed_or_element == (uint64_t)((valid >> (4 * i)) & 15u);
        if (!ok) { e->err = "azk_set_eval_symmetry: the board's geometry does not admit this element"; return AZK_ERR_ARG; }
    }
    if (!s.leaf_sym) {
        HIPCHK(e, dalloc(e, &s.leaf_sym, (size_t)d.G));
        HIPCHK(e, dalloc(e, &s.sym_cells, (size_t)d.G * d.rc_pad));
        HIPCHK(e, dalloc(e, &s.sym_logits, (size_t)d.G * g.action_dim));
        HIPCHK(e, hipMemsetAsync(s.sym_cells, 0, (size_t)d.G * d.rc_pad, (hipStream_t)stream));
    }
    HIPCHK(e, hipMemsetAsync(s.leaf_sym, 0, (size_t)d.G, (hipStream_t)stream));
    s.valid = valid; s.n_valid = n_valid;
    s.fixed = mode == 2 ? (int)seed_or_element : 0;
    s.seed_lo = (uint32_t)seed_or_element; s.seed_hi = (uint32_t)(seed_or_element >> 32);
    s.mode = mode;
    return AZK_OK;
}

int32_t azk_get_leaf_symmetry(azk_engine *e, uint8_t *out_dev, void *stream) {
    if (!e || !out_dev) return AZK_ERR_ARG;
    if (!e->sym.mode) { e->err = "azk_get_leaf_symmetry: no evaluation symmetry is set (azk_set_eval_symmetry)"; return AZK_ERR_STATE; }
    HIPCHK(e, hipMemcpyAsync(out_dev, e->sym.leaf_sym, (size_t)e->d.G, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return AZK_OK;
}

int32_t azk_eval_symmetry_restore(azk_engine *e, const float *logits_dev, float *out_dev, void *stream) {
    if (!e || !logits_dev || !out_dev) return AZK_ERR_ARG;
    if (!e->sym.mode) { e->err = "azk_eval_symmetry_restore: no evaluation symmetry is set (azk_set_eval_symmetry)"; return AZK_ERR_STATE; }
    k_sym_logits<<<e->d.G, AZK_WAVE, 0, (hipStream_t)stream>>>(e->d, e->sym, logits_dev, out_dev);
    HIPCHK(e, hipGetLastError());
    return AZK_OK;
}

}  // extern "C"
