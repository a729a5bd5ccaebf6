// azk_rng.h - the counter-based RNG of the product path, for the engine files that draw from it (azk_begin.hip, azk_moves.hip,
// azk_noise.hip): Philox4x32-10 keyed by (seed), counter = (global game, move key, entry, draw), the options' coins, and the Dirichlet and
// Gumbel rows.  tests/rng_restated.py restates all of it in float64 numpy.  Every function is inlined into the kernels that call it; they sit
// in an unnamed namespace like those kernels.
#pragma once
#include "azk_engine_int.h"

namespace {

// Philox4x32-10, the counter-based generator of every random number the product path draws
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0];
        const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n1 = (uint32_t)p1;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1, n3 = (uint32_t)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// two Philox words as a uniform: the top 53 bits of (hi << 32 | lo).  u53_incl0 takes them as they are, [0, 1): the moves' uniforms, the
// options' coins, the openings' draws.  u53 adds a half, (0, 1): the Dirichlet sampler, which takes logarithms
__device__ __forceinline__ double u53_incl0(uint32_t hi, uint32_t lo) {
    return (double)((((unsigned long long)hi << 32) | lo) >> 11) * (1.0 / 9007199254740992.0);
}
__device__ __forceinline__ double u53(uint32_t hi, uint32_t lo) {
    const unsigned long long x = (((unsigned long long)hi << 32) | lo) >> 11;
    return ((double)x + 0.5) * (1.0 / 9007199254740992.0);
}

// the options' coins: the uniform in [0, 1) of (seed, global game, word 2) under the Philox word 3 `tag`, made as noise_uniform makes its own.
// A tag is no other draw's (noise_uniform: 0xFFFFFFFF; noise_row: it < 64 and it | 0x40000000), so every other stream is what it was.
__device__ __forceinline__ double keyed_coin(unsigned long long seed, unsigned long long gg, uint32_t word2, uint32_t tag) {
    uint32_t w[4] = {(uint32_t)gg, (uint32_t)(gg >> 32), word2, tag};
    philox4x32_10(w, (uint32_t)seed, (uint32_t)(seed >> 32));
    return u53_incl0(w[0], w[1]);
}
// the coin of playout-cap randomisation (tag 0xFFFFFFFE): is the search of (seed, global game, move key) a FULL one?
__device__ __forceinline__ bool cap_coin(const CapDev &c, int g, int move) {
    return keyed_coin(c.seed, (unsigned long long)(c.first_game + g), (uint32_t)move, 0xFFFFFFFEu) < c.p_full;
}
// the game coin of resignation (tag 0xFFFFFFFD): is the game of (seed, global game, move key of its first search) a NEVER-RESIGN control
// game?  Stateless: the mover recomputes it at every move from start = (the slot's move counter) - (the game's plies), so no restart,
// recycle or reset kernel knows of it.
__device__ __forceinline__ bool resign_never(const ResignDev &rs, int g, uint32_t start) {
    return keyed_coin(rs.seed, (unsigned long long)(rs.first_game + g), start, 0xFFFFFFFDu) < rs.p_never;
}
// the ply coin of policy surprise weighting (tag 0xFFFFFFFC): the uniform that rounds the ply's weight to a whole number of copies
__device__ __forceinline__ double surprise_coin(const SurpriseDev &sp, int g, int move) {
    return keyed_coin(sp.seed, (unsigned long long)(sp.first_game + g), (uint32_t)move, 0xFFFFFFFCu);
}
// simulations of a search of that kind under the budget as it stands (a fast search never exceeds the budget)
__device__ __forceinline__ int cap_target(const CapDev &c, bool full, int budget) { return full ? budget : min(c.n_fast, budget); }

// a fresh-root search has just begun for game g (one lane): flip its coin and preset sims_done so that budget stepping stops a fast
// search after n_fast simulations - what top-up does with the carried visits
__device__ __forceinline__ void cap_begin_fresh(const Dev &d, const CapDev &c, int g, int move, bool count) {
    const int n = d.budget[0];
    const bool full = cap_coin(c, g, move);
    c.search_full[g] = full ? 1 : 0;
    d.sims_done[g] = n - cap_target(c, full, n);
    if (count && c.stats != nullptr) atomicAdd((unsigned long long *)&c.stats[full ? 8 : 9], 1ull);
}

// the uniform of (seed, global game, move): np.random.choice's draw of that move
__device__ __forceinline__ double noise_uniform(unsigned long long seed, unsigned long long gg, int move) {
    uint32_t c[4] = {(uint32_t)gg, (uint32_t)(gg >> 32), (uint32_t)move, 0xFFFFFFFFu};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return u53_incl0(c[0], c[1]);
}

// the Gamma(alpha) draw `gam` of entry a of the row of (key k0 k1, global game, move): Gamma(alpha) = Gamma(alpha + 1) * U^(1/alpha) (Marsaglia-
// Tsang for the shape > 1 part), two Philox blocks per try - {gg lo, gg hi ^ (a << 8), move, it} and it | 0x40000000 -, at most 64 tries (0 then).
// The ONE copy of the recipe: noise_row draws every entry of the action vector with it, root_noise_row (azk_noise.hip) the legal ones.  It is
// text, not a function: behind a call the compiler schedules k_gen_noise and k_noise_ahead differently, and an engine without root noise on
// the legal moves launches the device code it always launched (profiles/root_noise_isa_vs_parent.txt).  Declarations and a loop without a
// wrapper: use it only as full statements at block scope; it declares `gam`.
#define AZK_GAMMA_ENTRY(gam, k0, k1, gg, a, move, alpha)                                                                              \
    const double gm_d = (alpha) + 1.0 - 1.0 / 3.0, gm_cc = 1.0 / sqrt(9.0 * gm_d);                                                    \
    double gam = 0.0;                                                                                                                 \
    for (uint32_t it = 0; it < 64; it++) {                                                                                            \
        uint32_t c[4] = {(uint32_t)(gg), (uint32_t)((gg) >> 32) ^ ((uint32_t)(a) << 8), (uint32_t)(move), it};                        \
        philox4x32_10(c, k0, k1);                                                                                                     \
        uint32_t c2[4] = {(uint32_t)(gg), (uint32_t)((gg) >> 32) ^ ((uint32_t)(a) << 8), (uint32_t)(move), it | 0x40000000u};         \
        philox4x32_10(c2, k0, k1);                                                                                                    \
        const double u1 = u53(c[0], c[1]), u2 = u53(c[2], c[3]), u3 = u53(c2[0], c2[1]), u4 = u53(c2[2], c2[3]);                      \
        const double x = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);                                                          \
        const double t = 1.0 + gm_cc * x;                                                                                             \
        if (t <= 0.0) continue;                                                                                                       \
        const double v = t * t * t;                                                                                                   \
        if (log(u3) < 0.5 * x * x + gm_d - gm_d * v + gm_d * log(v)) { gam = gm_d * v * pow(u4, 1.0 / (alpha)); break; }              \
    }

// the Dirichlet(alpha) row of (seed, global game, move), by one wave; red: 64 doubles of LDS scratch.
__device__ __forceinline__ void noise_row(int A, unsigned long long seed, unsigned long long gg, int move, double alpha, double *row, double *red) {
    const int lane = azk_lane();
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    double part = 0.0;
    for (int a = lane; a < A; a += AZK_WAVE) {
        AZK_GAMMA_ENTRY(gam, k0, k1, gg, a, move, alpha)
        row[a] = gam;
        part += gam;
    }
    red[lane] = part;
    __syncthreads();
    for (int o = 32; o > 0; o >>= 1) { if (lane < o) red[lane] += red[lane + o]; __syncthreads(); }
    const double tot = red[0];
    for (int a = lane; a < A; a += AZK_WAVE) row[a] = tot > 0.0 ? row[a] / tot : 1.0 / (double)A;
    __syncthreads();
}

// The Gumbel(0, 1) row of (seed, global game, move), by one wave (Gumbel root search): entry a draws ONE Philox block at
// counter {gg lo, gg hi ^ (a << 8), move, 0xFFFFFFFB} - a word 3 that is no other stream's -, u = (((c0 << 32 | c1) >> 12) + 0.5) * 2^-52
// (exact, strictly inside (0, 1)) and g = -log(-log(u)).
__device__ __forceinline__ void gumbel_row(int A, unsigned long long seed, unsigned long long gg, int move, double *row, double *urow = nullptr) {
    for (int a = azk_lane(); a < A; a += AZK_WAVE) {
        uint32_t c[4] = {(uint32_t)gg, (uint32_t)(gg >> 32) ^ ((uint32_t)a << 8), (uint32_t)move, 0xFFFFFFFBu};
        philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
        const double u = ((double)((((unsigned long long)c[0] << 32) | c[1]) >> 12) + 0.5) * (1.0 / 4503599627370496.0);
        if (row != nullptr) row[a] = -log(-log(u));
        if (urow != nullptr) urow[a] = u;
    }
}

}  // namespace
