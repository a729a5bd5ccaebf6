// azk_moves_dev.h - the movers' device functions, for the two files whose kernels call them (azk_moves.hip: k_advance, k_move_async, the root
// statistics; azk_moves_kld.hip: the movers of engines with adaptive search budgets, split off so that the two halves of the mover family
// compile side by side): the recorded pi (pruned, or the Gumbel root's), the policy surprise, the checkpoint of adaptive search budgets, the
// move itself (advance_one) and the bodies of the lock-step and the asynchronous mover.  Everything is in an unnamed namespace, as the kernels
// that call it are.  Built with -ffp-contract=off like every engine file.
#pragma once
#include "azk_opt_pack.h"
#include "azk_rng.h"

namespace {

// Policy target pruning (forced playouts; Wu 2019, section 3.2) for one game (one wave).  L.cnt holds the root children's
// RAW visit counts by action; on return it holds the counts the recorded pi is made of, and the function returns their sum.  With
// Np = root visits, s = sqrt(Np) and c* = the first child with the most visits (Node.max_visit_child):
//     pstar = W* / N* + (P* * s) / (N* + 1)
// and every other child with N >= 1 loses up to nf = floor(sqrt((k * P) * (Np - 1))) visits - the floor forced playouts gave it - one at a
// time, while its PUCT score with that visit removed (q held at W / N) would still lose to c*:
//     m = N;  while (m > N - nf && m > 0 && q + (P * s) / m < pstar) m -= 1;   if (m == 1 && nf >= 1) m = 0
// All float64, P = the root's mixed priors (rootP); c* and unvisited children keep their counts.  At most nf <= sqrt(k * max_sims) rounds per
// lane.  The tree is not touched: the move, q, resignation and tree reuse see raw visits.
__device__ __forceinline__ int prune_counts(const Dev &d, const LdsView &L, int g, double k) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta)), Np = uniform_i32(d.H[base].N);
    const double *P = d.rootP + (size_t)g * gd.rc;
    const double s = sqrt((double)Np);
    int best = 0x7fffffff, bn = 0;                                  // Node.max_visit_child (node.py:76-81)
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        if (best == 0x7fffffff || n > bn) { bn = n; best = i; }
    }
    wave_argmax_first<int>(bn, best);
    best = uniform_i32(best); bn = uniform_i32(bn);
    const double pstar = d.W[base + fc + best] / (double)bn + (P[best] * s) / (double)(bn + 1);
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const NodeH h = d.H[base + fc + i];
        int m = h.N;
        if (i != best && h.N >= 1) {
            const double Pi = P[i];
            const int nf = (int)floor(sqrt((k * Pi) * (double)(Np - 1)));
            const double q = d.W[base + fc + i] / (double)h.N;
            while (m > h.N - nf && m > 0 && q + (Pi * s) / (double)m < pstar) m -= 1;
            if (m == 1 && nf >= 1) m = 0;
            L.cnt[azk_action_idx(gd, meta_cell(h.meta))] = m;
        }
        sum += m;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    return sum;
}
// is the search game g has just completed a forced one?  (the option set - the caller's template parameter - the search full, the root mixed)
__device__ __forceinline__ bool forced_search(const Dev &d, const ForcedDev &fp, int g) {
    const int full = fp.search_full != nullptr ? uniform_i32((int)fp.search_full[g]) : 1;
    return full != 0 && uniform_i32(d.root_f64[g]) != 0;
}

// Policy surprise (surprise weighting) of one game's move (one wave): KL(recorded pi || the network's prior) over the root's
// children, all float64:  kl = max(0, sum over children with m > 0 of  p * log(p / P)),  p = m / sum  the recorded pi's entry (L.cnt: the
// counts after pruning), P = the child's RAW float32 prior as k_tree stored it in the header (not rootP, the Dirichlet mix), floored at the
// smallest normal float.  Lanes sum their children in list order, then the wave's butterfly: the same order in both movers.
__device__ __forceinline__ double surprise_kl(const Dev &d, const LdsView &L, int g, int sum) {
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    double part = 0.0;
    for (int i = azk_lane(); i < nch; i += AZK_WAVE) {
        const NodeH h = d.H[base + fc + i];
        const int m = L.cnt[azk_action_idx(d.g, meta_cell(h.meta))];
        if (m > 0) {
            const double p = (double)m / (double)sum, P = (double)fmaxf(h.P, 0x1p-126f);
            part += p * log(p / P);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    return part > 0.0 ? part : 0.0;
}

// Adaptive search budgets (azk_set_kld_stop, azk_set_lead_stop; DESIGN sections 31 and 32): the checkpoint of one game (one wave) whose segment
// is complete - not done, sims_done >= budget, nothing pending; the caller has made that test.  Returns true when the game is RELEASED for
// another segment (wave-uniform), false when its search is over and the game is to be moved on the tree as it stands.  With n_i the root
// children's N in list order, S their sum, o_i / So the KLD rule's snapshot of the last checkpoint (So = 0: none):
//   1  left == 0                          over: the search ran its allowance
//   2L else, lead rule set (lead_factor > 0) and run >= lead_min_sims:
//                                          nch == 1: over, a forced move.  Otherwise N1 = max n_i, N2 = the second largest counting
//                                          multiplicity (a tie for the maximum: N2 = N1);  (double)left < lead_factor * (double)(N1 - N2): over,
//                                          the search ended early with `left` simulations unrun.  Integers but for that one multiply and compare
//   2K else, KLD rule set (min_gain > 0), So > 0 and run >= min_sims:
//                                          gain = sum over i with o_i > 0 of  po_i * log(po_i / pn_i),  po_i = (double)o_i / (double)So,
//                                          pn_i = (double)n_i / (double)S;  rate = gain / (double)(S - So);  rate < min_gain: over, the search
//                                          ended early with `left` simulations unrun
//   3  else                               KLD rule: snapshot o = n, So = S;  seg = min(interval, left);  sims_done = budget - seg;  left -= seg;
//                                          run += seg;  released, nothing else about the game changes
// Lanes take their children i, i + 64, ... in list order, then the xor butterfly 32 ... 1: surprise_kl's convention for the sum; for the lead
// rule each lane keeps a (max, second max) pair and two pairs merge into (the larger max, the largest of the smaller max and both seconds) -
// the pair's identity is (0, 0), visits are not negative.  Plain vector loads and stores; lane 0 writes the game's words.  With the KLD rule off
// neither snap, snap_sum nor rate is touched (they do not exist) and no log is executed.  A search that is over keeps ckpt negative, so a
// lock-step checkpoint that meets it again (other games were released) neither counts nor judges it twice.
__device__ __forceinline__ bool kld_judge_one(const Dev &d, const KldDev &kd, int g) {
    const int lane = azk_lane();
    const int ck = uniform_i32(kd.ckpt[g]);
    if (ck < 0) return false;                                       // over already
    const int left = uniform_i32(kd.left[g]);
    const bool kld = kd.min_gain > 0.0, lead = kd.lead_factor > 0.0;
    unsigned long long *st = (unsigned long long *)kd.stats, *ls = (unsigned long long *)kd.lead_stats;
    if (left == 0) {
        if (lane == 0) {
            kd.ckpt[g] = ~(ck + 1);
            if (kld) atomicAdd(&st[KST_ALLOWANCE], 1ull);
            if (lead) atomicAdd(&ls[LST_ALLOWANCE], 1ull);
        }
        return false;
    }
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = min(uniform_i32(meta_nch(d.H[base].meta)), kd.max_children);
    const int run = uniform_i32(kd.run[g]);
    if (lead && run >= kd.lead_min_sims) {
        int n1 = 0, n2 = 0;
        for (int i = lane; i < nch; i += AZK_WAVE) {
            const int n = d.H[base + fc + i].N;
            n2 = max(n2, min(n1, n));
            n1 = max(n1, n);
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int o1 = __shfl_xor(n1, off), o2 = __shfl_xor(n2, off);
            n2 = max(min(n1, o1), max(n2, o2));
            n1 = max(n1, o1);
        }
        const bool forced = nch == 1;
        const bool early = !forced && (double)left < kd.lead_factor * (double)(n1 - n2);
        if (lane == 0) {
            int *rec = kd.lead_rec + (size_t)g * 3;
            rec[0] = n1; rec[1] = n2; rec[2] = left;
            atomicAdd(&ls[LST_JUDGED], 1ull);
            if (forced) atomicAdd(&ls[LST_FORCED], 1ull);
            if (early) { atomicAdd(&ls[LST_EARLY], 1ull); atomicAdd(&ls[LST_UNRUN], (unsigned long long)left); }
            if (forced || early) kd.ckpt[g] = ~(ck + 1);
        }
        if (forced || early) return false;
    }
    int S = 0;
    if (kld) {
        const int So = uniform_i32(kd.snap_sum[g]);
        int *snap = kd.snap + (size_t)g * kd.max_children;
        for (int i = lane; i < nch; i += AZK_WAVE) S += d.H[base + fc + i].N;
        S = wave_sum_i32(S);
        if (So > 0 && run >= kd.min_sims) {
            double part = 0.0;
            for (int i = lane; i < nch; i += AZK_WAVE) {
                const int o = snap[i], n = d.H[base + fc + i].N;
                if (o > 0) {
                    const double po = (double)o / (double)So, pn = (double)n / (double)S;
                    part += po * log(po / pn);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
            const double rate = part / (double)(S - So);
            const bool early = rate < kd.min_gain;
            if (lane == 0) {
                kd.rate[g] = rate;
                atomicAdd(&st[KST_JUDGED], 1ull);
                if (early) { kd.ckpt[g] = ~(ck + 1); atomicAdd(&st[KST_EARLY], 1ull); atomicAdd(&st[KST_UNRUN], (unsigned long long)left); }
            }
            if (early) return false;
        }
        for (int i = lane; i < nch; i += AZK_WAVE) snap[i] = d.H[base + fc + i].N;
    }
    if (lane == 0) {
        const int seg = min(kd.interval, left);
        if (kld) kd.snap_sum[g] = S;
        d.sims_done[g] = d.budget[0] - seg;
        kd.left[g] = left - seg;
        kd.run[g] = run + seg;
        kd.ckpt[g] = ck + 1;
    }
    return true;
}

// Gumbel root search (azk_set_gumbel_root): the move and the recorded pi of one game's search (one wave), all float64,
// children in list order.  With N_i, W_i, P_i (the header's float32 prior), gl_i = rootP, logit_i and v0 as the root's expansion kept them:
//     S = sum N;  q_i = W_i / N_i (N_i > 0);  pv = sum over visited of P_i;  pq = sum over visited of P_i * q_i   (both sequential, list order)
//     vmix = S > 0 ? (v0 + S * (pq / pv)) / (1 + S) : v0;  qh_i = N_i > 0 ? q_i : vmix;  sigf = (c_visit + max N) * c_scale
//     move    among the children with N_i == max N, the first maximum of gl_i + sigf * qh_i
//     pi      y_i = logit_i + sigf * qh_i;  pi[a_i] = exp(y_i - max y) / sum_j exp(y_j - max y), 0 on every other action
// Returns the played child's list index (wave-uniform) and leaves pi, by action, in L.cdf.  The tree is not touched.
__device__ __forceinline__ int gumbel_target(const Dev &d, const LdsView &L, int g, const GumbelDev &gb) {
    constexpr int KMAX = 7;                                           // children per lane: make_game allows 400 cells
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int A = gd.action_dim, rc = gd.rc;
    const int fc = uniform_i32(d.H[base].fc), nch = min(uniform_i32(meta_nch(d.H[base].meta)), KMAX * AZK_WAVE);
    int *Nl = (int *)L.ms.claim;                                      // visits by child position (table_size words: more than any board has cells)
    int nv[KMAX], cellv[KMAX];
    double qv[KMAX], yv[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int i = lane + AZK_WAVE * k;
        nv[k] = 0; cellv[k] = 0; qv[k] = 0.0; yv[k] = 0.0;
        if (i < nch) {
            const NodeH h = d.H[base + fc + i];
            nv[k] = h.N; cellv[k] = meta_cell(h.meta);
            qv[k] = h.N > 0 ? d.W[base + fc + i] / (double)h.N : 0.0;
            Nl[i] = h.N; L.e[i] = h.P; L.cdf[i] = qv[k];
        }
    }
    __syncthreads();
    double vmix = 0.0;
    int maxn = 0;
    if (lane == 0) {
        int S = 0;
        double pv = 0.0, pq = 0.0;
        for (int i = 0; i < nch; i++) {
            const int n = Nl[i];
            S += n; maxn = max(maxn, n);
            if (n > 0) { const double P = (double)L.e[i]; pv += P; pq += P * L.cdf[i]; }
        }
        const double v0 = (double)gb.v0[g];
        vmix = S > 0 ? (v0 + (double)S * (pq / pv)) / (1.0 + (double)S) : v0;
    }
    vmix = __shfl(vmix, 0); maxn = __shfl(maxn, 0);
    const double sigf = (gb.c_visit + (double)maxn) * gb.c_scale;
    int best = 0x7fffffff;
    double bs = -__builtin_huge_val(), ym = -__builtin_huge_val();
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int i = lane + AZK_WAVE * k;
        if (i < nch) {
            const double qh = nv[k] > 0 ? qv[k] : vmix;
            const double sc = d.rootP[(size_t)g * rc + i] + sigf * qh;
            yv[k] = (double)gb.logit[(size_t)g * rc + i] + sigf * qh;
            if (nv[k] == maxn && (best == 0x7fffffff || sc > bs)) { bs = sc; best = i; }
            ym = fmax(ym, yv[k]);
        }
    }
    wave_argmax_first<double>(bs, best);
    best = uniform_i32(best);
    ym = wave_max_f64(ym);
    double part = 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        if (lane + AZK_WAVE * k < nch) { yv[k] = exp(yv[k] - ym); part += yv[k]; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) part += __shfl_xor(part, off);
    __syncthreads();
    for (int a = lane; a < A; a += AZK_WAVE) L.cdf[a] = 0.0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        if (lane + AZK_WAVE * k < nch) L.cdf[azk_action_idx(gd, cellv[k])] = yv[k] / part;
    }
    __syncthreads();
    return best;
}

// Move temperature (azk_set_move_temperature): the played child of one game's search (one wave), all float64.  With mc the
// game's plies, r = row_of_ply[min(mc, n_plies - 1)], b = the first child with the most visits (Node.max_visit_child), qb = W_b / N_b:
//     no uniform, or r < 0     b
//     else, per child i        w_i = weights[r][max(0, N_i - visit_offset)];  with a cutoff >= 0, a child with w_i > 0 and
//                              W_i / N_i < qb - cutoff gets w_i = 0 (it is cut)
//     by action a              w[a] = its child's w_i, 0 where there is none;  S = w[0] + w[1] + ... sequentially
//     S == 0                   b (a fallback)
//     else                     Node.sample_child's arithmetic on w instead of the counts: acc += w[a] / S, cdf[a] = acc sequentially,
//                              index = searchsorted(cdf / cdf[-1], u, side='right') clamped to A - 1, the first child with that action
// The weights fill L.cdf and are accumulated in place; L.cnt keeps the raw visits, which the recorded pi is made of.  (The column is also
// held below n_cols: no engine the option admits has a root child with more than max_sims visits, and no table is read past its end.)
// Returns the played child's list index (wave-uniform), -1 if the drawn action has no child (a state error, as in the sampler below).
__device__ __forceinline__ int temp_child(const Dev &d, const LdsView &L, int g, bool have_u, double u, int mc, const TempDev &tm) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int A = gd.action_dim;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    int best = 0x7fffffff, bn = 0;                                  // Node.max_visit_child (node.py:76-81)
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        if (best == 0x7fffffff || n > bn) { bn = n; best = i; }
    }
    wave_argmax_first<int>(bn, best);
    best = uniform_i32(best); bn = uniform_i32(bn);
    const int row = have_u ? uniform_i32(tm.row_of_ply[max(0, min(mc, tm.n_plies - 1))]) : -1;
    if (row < 0) return best;
    const double qb = d.W[base + fc + best] / (double)bn;
    const double *wr = tm.weights + (size_t)row * tm.n_cols;
    for (int a = lane; a < A; a += AZK_WAVE) L.cdf[a] = 0.0;
    __syncthreads();
    int cut = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const NodeH h = d.H[base + fc + i];
        double w = wr[min(max(h.N - tm.visit_offset, 0), tm.n_cols - 1)];
        if (tm.value_cutoff >= 0.0 && w > 0.0 && d.W[base + fc + i] / (double)h.N < qb - tm.value_cutoff) { w = 0.0; cut += 1; }
        L.cdf[azk_action_idx(gd, meta_cell(h.meta))] = w;
    }
    cut = wave_sum_i32(cut);
    __syncthreads();
    double S = 0.0;
    if (lane == 0) for (int a = 0; a < A; a++) S += L.cdf[a];
    S = __shfl(S, 0);
    // (the quotients are elementwise: every lane divides its actions, and only the two running sums stay on lane 0's chain)
    if (S != 0.0) for (int a = lane; a < A; a += AZK_WAVE) L.cdf[a] = L.cdf[a] / S;
    __syncthreads();
    if (lane == 0) {
        int act = -1;
        if (S != 0.0) {
            double acc = 0.0;
            for (int a = 0; a < A; a++) { acc += L.cdf[a]; L.cdf[a] = acc; }
            const double lastv = L.cdf[A - 1];
            int lo = 0, hi = A;
            while (lo < hi) { int mid = (lo + hi) >> 1; if (u < L.cdf[mid] / lastv) hi = mid; else lo = mid + 1; }
            act = lo < A ? lo : A - 1;
        }
        L.path[0] = act;                                             // action drawn, -1 = every weight is 0 (path scratch, as the sampler's)
    }
    __syncthreads();
    const int act = uniform_i32(L.path[0]);
    int found = best;
    if (act >= 0) {
        found = 0x7fffffff;
        for (int i = lane; i < nch; i += AZK_WAVE)
            if (azk_action_idx(gd, meta_cell(d.H[base + fc + i].meta)) == act && i < found) found = i;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { int o = __shfl_xor(found, off); found = o < found ? o : found; }
    }
    if (lane == 0) {
        unsigned long long *st = (unsigned long long *)tm.stats;
        if (act >= 0) {
            atomicAdd(&st[0], 1ull);
            if (found != best) atomicAdd(&st[1], 1ull);
        } else atomicAdd(&st[3], 1ull);
        if (cut) atomicAdd(&st[2], (unsigned long long)cut);
    }
    return found != 0x7fffffff ? found : -1;
}

// gomoku.py:143-162 for one game (one wave): choose (sample ~ visits | first max-visit child), record pi / the action in the
// trajectory, make_move, check_winner, draw.  Returns the chosen cell (-1: state error, already reported); *win_out / *done_out as
// k_advance's outputs; pi of the move is left in L.cnt / sum_out (visit counts per action and their sum).
// RESIGN (resigning engines, azk_set_resign): after a move that does not end the game the mover concedes when the
// root's q reached v_resign - or, in a never-resign game, is noted as the game's mark.  key = the slot's move counter at this move,
// *rsg_out = 1 when the move ended the game by resignation.  A resignation happens where a natural end happens (winner and done are set
// here), so emission, recycling, the drain and the re-root see an ordinary finished game.
// FORCED (engines with forced playouts, azk_set_forced_playouts): once the cell is chosen - from raw visits - the counts
// of a forced search are pruned in place (prune_counts), so that traj_pi and the caller's record hold the pruned pi.  The selection half of
// the option lives in k_tree<.., FORCED> (azk_tree.hip).
// SURPRISE (engines with surprise weighting, azk_set_surprise_weighting): the kl of the pi that is recorded - after the
// pruning - and the ply's coin of the move key go into traj_kl / traj_coin beside traj_pi and into the game's last-move pair (lane 0 writes
// them: the asynchronous mover's lane 0 copies the pair into its record).
// GUMBEL (engines with a Gumbel root, azk_set_gumbel_root): the move is gumbel_target's - the uniform and sample_until are
// not looked at, the Gumbel arg-max is the sample - and the recorded pi is its float64 row in L.cdf (the caller's record reads it there too);
// L.cnt / sum_out still hold the raw visits.
// TEMP (engines with a move temperature, azk_set_move_temperature): the move is temp_child's - sample_until is not looked
// at, the ply table is - and everything after the choice works on that cell as it does on any other; the recorded pi stays the raw (or pruned)
// visit distribution in L.cnt.
// VALUE (engines with value targets, azk_set_value_target): the root's q = W / N - the expression of k_root_stats, the
// asynchronous record and resignation, the value for the mover's opponent - goes into traj_q beside traj_pi (lane 0 writes it); the move itself
// and everything else recorded are what they are without the option.
template <bool RESIGN, bool FORCED, bool SURPRISE, bool GUMBEL = false, bool TEMP = false, bool VALUE = false>
__device__ __forceinline__ int advance_one(const Dev &d, LdsView &L, int g, bool have_u, double u, int sample_until, int *win_out, int *done_out,
                                           int *sum_out, const ResignDev &rs, int key, int *rsg_out, const ForcedDev &fp, const SurpriseDev &sp,
                                           const GumbelDev &gb = GumbelDev{}, const TempDev &tm = TempDev{}, const ValueDev &vt = ValueDev{}) {
    const int lane = azk_lane();
    const GameDesc &gd = d.g;
    const size_t base = (size_t)g * d.cap;
    const int A = gd.action_dim, rc = gd.rc;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    const int mc = uniform_i32(d.move_count[g]), mover = uniform_i32(d.to_move[g]);
    for (int i = lane; i < rc; i += AZK_WAVE) L.board[i] = d.cells[(size_t)g * d.rc_pad + i];
    for (int a = lane; a < A; a += AZK_WAVE) L.cnt[a] = 0;
    __syncthreads();
    int sum = 0;
    for (int i = lane; i < nch; i += AZK_WAVE) {
        const int n = d.H[base + fc + i].N;
        L.cnt[azk_action_idx(gd, meta_cell(d.H[base + fc + i].meta))] = n;
        sum += n;
    }
    sum = wave_sum_i32(sum);
    __syncthreads();
    *sum_out = sum;
    int cellc = -1;
    if (nch <= 0 || sum <= 0) {
        if (lane == 0) atomicExch(d.err, AZK_ERR_STATE);
        return -1;
    }
    if constexpr (GUMBEL) {
        cellc = meta_cell(d.H[base + fc + gumbel_target(d, L, g, gb)].meta);
    } else
    if constexpr (TEMP) {
        const int child = temp_child(d, L, g, have_u, u, mc, tm);
        cellc = child >= 0 ? meta_cell(d.H[base + fc + child].meta) : -1;
    } else
    if (have_u && mc < sample_until) {
        // Node.sample_child (node.py:83-93) -> legacy np.random.choice(p=pi): cdf = cumsum(pi); cdf /= cdf[-1];
        // index = searchsorted(cdf, u, side='right').  cumsum is sequential in float64.
        if (lane == 0) {
            double acc = 0.0;
            for (int a = 0; a < A; a++) { acc += (double)L.cnt[a] / (double)sum; L.cdf[a] = acc; }
            const double lastv = L.cdf[A - 1];
            int lo = 0, hi = A;
            while (lo < hi) { int mid = (lo + hi) >> 1; if (u < L.cdf[mid] / lastv) hi = mid; else lo = mid + 1; }
            L.path[0] = lo < A ? lo : A - 1;                         // action drawn (path scratch: cnt[] is still needed)
        }
        __syncthreads();
        const int act = L.path[0];
        int found = 0x7fffffff;
        for (int i = lane; i < nch; i += AZK_WAVE)
            if (azk_action_idx(gd, meta_cell(d.H[base + fc + i].meta)) == act && i < found) found = i;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) { int o = __shfl_xor(found, off); found = o < found ? o : found; }
        cellc = found != 0x7fffffff ? meta_cell(d.H[base + fc + found].meta) : -1;
    } else {
        // Node.max_visit_child (node.py:76-81): first child with the most visits
        int best = 0x7fffffff, bn = 0;
        for (int i = lane; i < nch; i += AZK_WAVE) {
            const int n = d.H[base + fc + i].N;
            if (best == 0x7fffffff || n > bn) { bn = n; best = i; }
        }
        wave_argmax_first<int>(bn, best);
        cellc = meta_cell(d.H[base + fc + uniform_i32(best)].meta);
    }
    cellc = uniform_i32(cellc);
    if (cellc < 0) {
        if (lane == 0) atomicExch(d.err, AZK_ERR_STATE);
        return -1;
    }
    if constexpr (FORCED) {
        if (forced_search(d, fp, g)) {
            const int raw = sum;
            sum = prune_counts(d, L, g, fp.k);
            *sum_out = sum;
            if (lane == 0) { count_add(d, CNT_PRUNED, g, raw - sum); count_add(d, CNT_PRUNE_OF, g, raw); }
        }
    }
    if (d.traj_pi != nullptr && mc < gd.state_dim) {               // gomoku.py:138-146: pi and the action of this ply
        double *tp = d.traj_pi + ((size_t)g * gd.state_dim + mc) * A;
        if constexpr (GUMBEL) { for (int a = lane; a < A; a += AZK_WAVE) tp[a] = L.cdf[a]; }
        else
        for (int a = lane; a < A; a += AZK_WAVE) tp[a] = (double)L.cnt[a] / (double)sum;
        if (lane == 0) d.traj_action[(size_t)g * gd.state_dim + mc] = (int16_t)cellc;
        if constexpr (VALUE) { if (lane == 0) vt.traj_q[(size_t)g * gd.state_dim + mc] = d.W[base] / (double)d.H[base].N; }
    }
    if constexpr (SURPRISE) {
        const double kl = surprise_kl(d, L, g, sum), coin = surprise_coin(sp, g, key);
        if (lane == 0) {
            if (d.traj_pi != nullptr && mc < gd.state_dim) { sp.traj_kl[(size_t)g * gd.state_dim + mc] = kl; sp.traj_coin[(size_t)g * gd.state_dim + mc] = coin; }
            sp.last_kl[g] = kl; sp.last_coin[g] = coin;
        }
    }
    AZK_PLACE_STONE(L.board, gd, lane, mover, cellc);
    const int w = azk_check_winner(L.board, gd, mover, cellc);      // gomoku.py:150
    int win = -2, dn = 0;
    if (w != -1) { win = w; dn = 1; }
    else if (mc + 1 == gd.state_dim) { win = -1; dn = 1; }
    if (RESIGN) {
        // the game's first search had move key key - mc; q is the recorded q (k_root_stats, the movers' rec_q): the same float64 expression
        const uint32_t start = (uint32_t)key - (uint32_t)mc;
        const bool never = resign_never(rs, g, start);
        const int side = uniform_i32(rs.mark_side[g]);
        const bool marked = side >= 0 && (uint32_t)uniform_i32((int)rs.mark_start[g]) == start;
        int rsg = 0;
        if (dn == 0 && mc + 1 >= rs.min_ply && d.W[base] / (double)d.H[base].N >= rs.v_resign) {
            if (!never) { win = 1 - mover; dn = 1; rsg = 1; }                                  // the mover concedes
            else if (!marked && lane == 0) { rs.mark_start[g] = start; rs.mark_side[g] = mover; }   // ... would have: the game plays on
        }
        if (lane == 0) {
            rs.resigned[g] = (uint8_t)rsg;
            if (rsg) atomicAdd((unsigned long long *)&rs.stats[0], 1ull);
            else if (dn && never) {
                atomicAdd((unsigned long long *)&rs.stats[1], 1ull);
                if (marked) atomicAdd((unsigned long long *)&rs.stats[2], 1ull);
                if (marked && win != 1 - side) atomicAdd((unsigned long long *)&rs.stats[3], 1ull);     // a false positive: it won or drew
            }
        }
        *rsg_out = rsg;
    }
    if (lane == 0) {
        d.cells[(size_t)g * d.rc_pad + cellc] = L.board[cellc];
        d.to_move[g] = 1 - mover;
        d.move_count[g] = mc + 1;
        d.winner[g] = win; d.done[g] = dn;
        d.counters[(size_t)CNT_MOVES * d.G + g] += 1;
    }
    *win_out = win; *done_out = dn;
    return cellc;
}

// tree reuse: the arena index of the root's child that holds cell `cellc` (a cell occurs once among a node's children), -1 = none.
// One wave; the result is wave-uniform.  The move itself (advance_one) does not touch the tree, so this may follow it.
__device__ __forceinline__ int played_child(const Dev &d, int g, int cellc) {
    const int lane = azk_lane();
    const size_t base = (size_t)g * d.cap;
    const int fc = uniform_i32(d.H[base].fc), nch = uniform_i32(meta_nch(d.H[base].meta));
    int found = 0x7fffffff;
    for (int i = lane; i < nch; i += AZK_WAVE) if (meta_cell(d.H[base + fc + i].meta) == cellc && i < found) found = i;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const int o = __shfl_xor(found, off); found = o < found ? o : found; }
    return (cellc >= 0 && found != 0x7fffffff) ? fc + found : -1;
}

// The lock-step mover (azk_advance, azk_advance_resign): every game's move, one wave per game.  CAP: the ply's kind goes into traj_full beside its
// pi; RESIGN, SURPRISE (move_index = the slot's move counter), FORCED, TEMP, VALUE: as advance_one has them
template <bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool GUMBEL = false, bool TEMP = false, bool VALUE = false>
__device__ __forceinline__ void advance_body(Dev d, CapDev cp, ResignDev rs, int move_index, const double *uniforms, int sample_until,
                                             int *chosen, int *winner_out, int *done_out, int *chosen_node, const ForcedDev &fp, const SurpriseDev &sp,
                                             const GumbelDev &gb = GumbelDev{}, const TempDev &tm = TempDev{}, const ValueDev &vt = ValueDev{}) {
    const int g = blockIdx.x, lane = azk_lane();
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    if (uniform_i32(d.done[g]) != 0) {
        if (lane == 0) {
            if (chosen) chosen[g] = -1;
            if (winner_out) winner_out[g] = d.winner[g];
            if (done_out) done_out[g] = 1;
            if (chosen_node) chosen_node[g] = -1;
        }
        return;
    }
    int win = -2, dn = 0, sum = 0, rsg = 0;
    const int mc = CAP ? uniform_i32(d.move_count[g]) : 0;
    int cellc;
    if constexpr (GUMBEL) cellc = advance_one<RESIGN, false, false, true>(d, L, g, false, 0.0, 0, &win, &dn, &sum, rs, move_index, &rsg, fp, sp, gb);
    else cellc = advance_one<RESIGN, FORCED, SURPRISE, false, TEMP, VALUE>(d, L, g, uniforms != nullptr, uniforms != nullptr ? uniforms[g] : 0.0, sample_until, &win, &dn, &sum,
                                                            rs, move_index, &rsg, fp, sp, GumbelDev{}, tm, vt);
    if (CAP && cellc >= 0 && lane == 0 && cp.traj_full != nullptr && mc < d.g.state_dim) cp.traj_full[(size_t)g * d.g.state_dim + mc] = cp.search_full[g];
    if (chosen_node) {
        const int child = played_child(d, g, cellc);               // tree reuse: the next search's root
        if (lane == 0) chosen_node[g] = dn == 0 ? child : -1;
    }
    if (cellc < 0) return;
    if (lane == 0) {
        if (chosen) chosen[g] = cellc;
        if (winner_out) winner_out[g] = win;
        if (done_out) done_out[g] = dn;
    }
}

// ------------------------------------------------------------------------------------------------
// Asynchronous self-play (games/gomoku.py:132-162: a game moves as soon as ITS search is done).  After every tree launch
// k_move_async looks at every game: one whose search is complete (its simulation budget used up, nothing pending) gets its move
// - root statistics, pi into the trajectory, sampled / most-visited child, make_move, check_winner, a record into the device
// ring - and, unless the game ended, its next search at once: fresh root, Dirichlet row of (seed, global game, the slot's move
// counter).  Finished games wait for azk_async_drain ((state, pi, z) emission, statistics, restart), which the host runs every
// few launches.  Random numbers are keyed by (seed, global game index, per-slot move counter): exactly the keys of the lock-step
// driver, so a slot plays the same sequence of games move for move, whatever the timing.
// A re-rooting engine (azk_async_begin_reuse) does not begin the next search in the move kernel: re-rooting a large subtree is a
// dependent chain of some hundred memory round trips for ONE wave, and every launch of the step chain would last that long.  The
// move kernel notes the played child and PARKS the game - its parked word set, sims_done at the largest int so that k_tree idles it
// whatever the budget becomes - on a list; the drain re-roots the listed games (k_reroot_list) and un-parks them.  The kernel
// boundary is the only ordering relied on.  The drain's restart and re-root kernels live with the other kernels that start games and
// searches (azk_begin.hip: k_async_restart, k_reroot_list); begin_search_one, which they share with the mover, in azk_engine_int.h.
// The rows a search reads are made a search ahead by the drain (azk_noise.hip: k_noise_ahead, k_gumbel_ahead).
// ------------------------------------------------------------------------------------------------
// The asynchronous mover.  REROOT: a re-rooting engine - the moved game is parked for the drain's k_reroot_list instead of beginning its search
// here; CAP: the kind of the completed search goes into the record and traj_full, and the next fresh-root search flips its coin; RESIGN, FORCED:
// SURPRISE, TEMP, VALUE: as advance_one has them (the move key is the slot's move counter; kl and coin go into the record's columns too)
// KLD (engines with adaptive search budgets, azk_set_kld_stop): a game that passes the early-out is at a checkpoint - it is judged
// (kld_judge_one) and, where it is released for another segment, the wave ends there; a search that is over is moved as ever, the new
// simulations it ran go into the record's sims column, and the search the mover begins itself is armed
template <bool REROOT, bool CAP, bool RESIGN, bool FORCED, bool SURPRISE, bool GUMBEL = false, bool TEMP = false, bool VALUE = false, bool KLD = false>
__device__ __forceinline__ void move_async_body(Dev d, AsyncDev p, ReuseDev r, CapDev cp, ResignDev rs, const ForcedDev &fp, const SurpriseDev &sp,
                                                const GumbelDev &gb = GumbelDev{}, const TempDev &tm = TempDev{}, const ValueDev &vt = ValueDev{},
                                                const KldDev &kd = KldDev{}) {
    const int g = blockIdx.x, lane = azk_lane();
    // one vector load for the three words that decide whether this game moves now (almost never: the wave then ends at once)
    const int *up = d.done + g;
    up = lane == 1 ? d.sims_done + g : up;
    up = lane == 2 ? d.leaf_node + g : up;
    up = lane == 3 ? d.budget : up;                                // (the simulation budget lives in device memory: azk_async_set_budget)
    up = (lane == 4 && p.dirichlet) ? p.noise_key + g : up;
    up = lane == 5 ? (const int *)(p.slot_moves + g) : up;         // (low word: a slot plays far fewer than 2^31 moves)
    if (REROOT) up = lane == 6 ? p.parked + g : up;                // a parked game has moved already: its sims_done passes any budget
    const int uw = *up;
    if (REROOT && __builtin_amdgcn_readlane(uw, 6) != 0) return;
    if (__builtin_amdgcn_readlane(uw, 0) != 0 || __builtin_amdgcn_readlane(uw, 1) < __builtin_amdgcn_readlane(uw, 3) || __builtin_amdgcn_readlane(uw, 2) >= 0) return;
    // the next search's Dirichlet row is made a search ahead (k_noise_ahead, every drain); a game whose whole search fitted between two
    // drains (tiny budgets only) waits for it - a scheduling delay, the game's moves do not change
    if (p.dirichlet && __builtin_amdgcn_readlane(uw, 4) < __builtin_amdgcn_readlane(uw, 5) + 1) return;
    if constexpr (KLD) { if (kld_judge_one(d, kd, g)) return; }
    LdsView L = carve(d.g, d.path_cap, d.table_size);
    const int A = d.g.action_dim;
    const size_t base = (size_t)g * d.cap;
    const long long mv = p.slot_moves[g];
    const double q = d.W[base] / (double)d.H[base].N;                 // root.value / root.visit (gomoku.py:140), before the tree is reset
    int win = -2, dn = 0, sum = 0, rsg = 0;
    const double u = noise_uniform(p.seed, (unsigned long long)(p.first_game + g), (int)mv);
    const int mc = CAP ? uniform_i32(d.move_count[g]) : 0;
    const int kind = CAP ? uniform_i32((int)cp.search_full[g]) : 1;     // of the search that is complete
    int cellc;
    if constexpr (GUMBEL) cellc = advance_one<RESIGN, false, false, true>(d, L, g, false, 0.0, 0, &win, &dn, &sum, rs, (int)mv, &rsg, fp, sp, gb);
    else cellc = advance_one<RESIGN, FORCED, SURPRISE, false, TEMP, VALUE>(d, L, g, true, u, p.sample_until, &win, &dn, &sum, rs, (int)mv, &rsg, fp, sp, GumbelDev{}, tm, vt);
    if (cellc < 0) return;
    if (CAP && lane == 0 && cp.traj_full != nullptr && mc < d.g.state_dim) cp.traj_full[(size_t)g * d.g.state_dim + mc] = (uint8_t)kind;
    if (p.rec_cap > 0) {                                           // the move's record: what the reference's self_play keeps per ply
        long long slot = 0;
        if (lane == 0) slot = (long long)(atomicAdd((unsigned long long *)&p.stats[6], 1ull) % (unsigned long long)p.rec_cap);
        slot = ((long long)__builtin_amdgcn_readfirstlane((int)(slot >> 32)) << 32) | (unsigned)__builtin_amdgcn_readfirstlane((int)slot);
        if constexpr (GUMBEL) { for (int a = lane; a < A; a += AZK_WAVE) p.rec_pi[(size_t)slot * A + a] = L.cdf[a]; }
        else
        for (int a = lane; a < A; a += AZK_WAVE) p.rec_pi[(size_t)slot * A + a] = (double)L.cnt[a] / (double)sum;
        if (lane == 0) {
            p.rec_q[slot] = q;
            int *m = p.rec_meta + (size_t)slot * 4;
            m[0] = g; m[1] = (int)mv; m[2] = cellc; m[3] = win;
            if (CAP && cp.rec_full != nullptr) cp.rec_full[slot] = (uint8_t)kind;
            if (RESIGN && rs.rec_resigned != nullptr) rs.rec_resigned[slot] = (uint8_t)rsg;
            if (SURPRISE && sp.rec_kl != nullptr) sp.rec_kl[slot] = sp.last_kl[g];        // (this lane wrote the pair in advance_one)
            if (SURPRISE && sp.rec_coin != nullptr) sp.rec_coin[slot] = sp.last_coin[g];
            if constexpr (KLD) { if (kd.rec_sims != nullptr) kd.rec_sims[slot] = kd.run[g]; }   // (this lane wrote the word, at arming or in kld_judge_one)
        }
    }
    __syncthreads();
    if (lane == 0) {
        p.slot_moves[g] = mv + 1;                                  // the NEW search's key: its row (mv + 1) & 1 has been waiting since the last move
        atomicAdd((unsigned long long *)&p.stats[5], 1ull);
        if (p.dirichlet) p.todo_list[atomicAdd(p.todo_count, 1)] = g;          // row mv + 2 is due
    }
    __syncthreads();
    if (REROOT) {
        if (uniform_i32(dn)) return;                               // an ended game restarts from a fresh root in the drain, as ever
        const int child = played_child(d, g, cellc);
        if (lane == 0) {
            r.chosen_node[g] = child;
            d.sims_done[g] = 0x7fffffff;                           // no budget reaches this: k_tree and k_unfinished see a finished search
            p.parked[g] = 1;
            p.reroot_list[atomicAdd(p.reroot_count, 1)] = g;
        }
    } else if (!dn) {
        begin_search_one(d, p, g);
        if (CAP && lane == 0) cap_begin_fresh(d, cp, g, (int)mv + 1, true);
        if constexpr (KLD) { if (lane == 0) kld_arm_one(d, kd, g); }
    }
}

// ... and of an engine with adaptive search budgets (azk_set_kld_stop): the same family under a name of its own (azk_moves_kld.hip), KldDev
// behind the pack, so that the movers of azk_moves.hip keep their symbols and argument layouts
template <class P> struct KldPack : P { KldDev kd; };

}  // namespace
