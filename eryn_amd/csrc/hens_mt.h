// hens_mt.h - k_mt_dist<DT, LIKE, NW>: the multiple-try independence move of MTDistGenMove(independent=True) (mtdistgen.py:7-136 over
// MultipleTryMove.get_mt_proposal, multipletry.py:238-514, under MHMove.propose, mh.py:56-193) as ONE full-ensemble launch at a
// compile-time row width.  Every walker of every resident rung is offered K = num_try fresh points from a generator of per-coordinate
// terms (hens_set_mt_dist_proposal: hens_set_dist_proposal's generator), one is picked with probability proportional to its
// importance weight and the accept test compares the sum of the tries' weights with the sum in which the current point stands in the
// picked try's place:
//   w_k    = (beta ll_k + lp_k) - lq_k                                                    (multipletry.py:45,221-223)
//   lsw    = max w + log(sum exp(w - max w))                                              (multipletry.py:25-33)
//   j      = first k with cumsum(exp(w - lsw))_k > u_pick, else 0                         (multipletry.py:51-57)
//   w'_k   = w_k (k != j), w'_j = (beta L_old + P_old) - logq(x_old);  aux_lsw likewise   (multipletry.py:381-417,463)
//   factors = ((aux_logP_j - aux_lsw) - alq_j + alq_j) - ((logP_j - lsw) - lq_j + lq_j)   (multipletry.py:472-476)
// into the accept rule every stepping kernel shares (accept_test) with logl = ll_j, logp = lp_j (mh.py:150-171: not re-evaluated).
// An old point outside the generator has w'_j = +inf, aux_lsw = NaN and is never moved.  The reference evaluates the likelihood of a
// try whose prior is -inf; this kernel skips and fills it as every stepping kernel does: such a try has weight -inf either way and can
// be "picked" only through the j = 0 fallback, which gives a NaN lnpdiff and a rejection - the difference is unobservable.
//
// On k_dist's term tile (TermTile, hens_prior.h) and hens_dist.h's device functions, called, not copied.  The 64 rows of the tile are
// the tries of a few walkers: KP = the smallest power of two >= K, one workgroup = G = 64 / KP walkers of one rung, walker g of the
// tile owns rows g KP .. g KP + K - 1 (one try each); rows k >= K of a segment are dead (no draw, weight -inf, never picked, never
// written).  Grid ceil(W / G) x Tl; the last workgroup of a rung is ragged whenever G does not divide W.  LDS: prior_lds_bytes.
//   phase A  lane-per-row    : the row's walker: own row, {L, P}, log u_acc, u_pick (every lane of a segment holds its walker's)  (wave 0)
//   phase B  lanes-over-d    : as k_dist, the proposal being try k's point (the caller's q[Tl][W][K][D], or dist_draw with counter
//                              word 3 = PURPOSE_DIST | d << 8 | k << 16: try 0 is the point k_dist draws); B1 forms the generator's
//                              terms at the OLD row in the segment's first row only (one row per walker is enough), B2 at the new
//                              rows, B3 the prior's - the one term tile in turn
//   phase C  lane-per-row    : TermTile::logl on the 64 rows as they stand
//   phase D  lane-per-try    : wave 0 holds one try per lane.  Segmented over the KP lanes of a walker (butterfly shuffles; a segment
//                              is aligned and a power of two wide, so every lane ends with its segment's value, bit for bit the same):
//                              max with NumPy's NaN rule, sum of exp(w - max), lsw; p = exp(w - lsw), an inclusive scan (shuffle-up
//                              inside the segment), the pick by a ballot; the picked lane's {ll, lp, lq, logP} broadcast; aux_lsw
//                              with the picked lane's weight replaced; the factor; the segment's first lane runs accept_test and
//                              writes {L, P} = {ll_j, stored_logp(lp_j)} to the record or the by-field arrays, the MH accept
//                              counter and the outputs
//   phase E  lanes-over-d    : row j of the proposal tile over the walker's own row in place, accepted walkers only
// The sums' order is the butterfly's, not NumPy's pairwise one: lsw / aux_lsw / factors agree with the reference to rounding
// (tests/mt_move.py derives the bound), picks and keeps away from knife edges exactly.
// Plain stores; launched on the HIP stream with its release like every MH launch; not among the fence-free kernels of the store census.
#pragma once
#include "hens_dist.h"

namespace hens {

struct MtArgs : DistArgs {      // q: [Tl][W][K][D] teacher-forced tries, or nullptr: device draws
    const double* u_pick;       // [Tl][W] pick uniforms (teacher-forced), or nullptr: mt_pick_uniform(seed, iter, wid)
    int32_t* pick_out;          // [Tl][W] or nullptr
    double* lsw_out;            // [2][Tl][W] (lsw, aux_lsw) or nullptr
    int32_t K, kp_shift;        // num_try; KP = 1 << kp_shift
};

// the pick uniform of walker `wid` in iteration `it` (multipletry.py:57), by mh_uniform's construction under a purpose of its own
__device__ __forceinline__ double mt_pick_uniform(uint64_t seed, uint64_t it, uint32_t wid) {
    const u4 ctr{(uint32_t)it, (uint32_t)(it >> 32), wid, PURPOSE_MT_PICK};
    const u4 d = philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
    return u01(d.x, d.y);
}

// multipletry.py:25-33 over the KP lanes of a segment: every lane of the wavefront calls it with its weight (`live`: the lane holds a
// try; a dead lane adds nothing).  np.max hands a NaN on; max = +-inf gives w - max = NaN for that entry and a NaN sum, as there.
__device__ __forceinline__ double seg_logsumexp(double w, bool live, int KP, int lane) {
    const unsigned long long anynan = row_ballot(live && (w != w), KP, lane);
    double m = live ? w : -INFINITY;
    for (int off = 1; off < KP; off <<= 1) m = fmax(m, __shfl_xor(m, off));
    if (anynan != 0ull) m = NAN;
    double s = live ? exp(w - m) : 0.0;
    for (int off = 1; off < KP; off <<= 1) s += __shfl_xor(s, off);
    return m + log(s);
}

template <int DT, int LIKE, int NW>
__global__ __launch_bounds__(NW * 64) void k_mt_dist(const MtArgs A) {
    static_assert(DT == 8 || DT == 16 || DT == 32 || DT == 64 || DT == 128, "power-of-two row width");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Tile = TermTile<DT, NW>;
    constexpr int D = DT, RS = Tile::RS, LPR = Tile::LPR;
    constexpr int F_OLD = 16, F_NEW = 32;          // k_dist's row-flag bits: old / new row inside the generator's supports

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Tile T(smem_raw, tid);
    const int tl = blockIdx.y;
    const int W = A.W;
    const int K = A.K, sh = A.kp_shift, KP = 1 << sh;
    const int k0 = blockIdx.x * (TILE >> sh);      // the tile's first walker
    const bool forced = A.q != nullptr;

    MfRegs mfr = T.template prologue<LIKE>(A, tid, lane, wv);

    // ---- phase A: lane = tile row = (walker k0 + (lane >> sh), try lane & (KP - 1))
    const int kt = lane & (KP - 1), base = lane & ~(KP - 1);
    double lu = 0.0, up = 0.0, Lold = 0.0, Pold = 0.0;
    size_t gi = 0;
    bool wvalid = false, valid = false;
    if (wv == 0) {
        const int own = k0 + (lane >> sh);
        wvalid = own < W;
        valid = wvalid && kt < K;
        int rs = 0;
        if (wvalid) {
            gi = (size_t)tl * W + own;
            rs = A.loc[gi];
            const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)W + (uint32_t)own;
            lu = A.lu ? A.lu[gi] : mh_log_uniform(A.seed, A.iter, wid);
            up = A.u_pick ? A.u_pick[gi] : mt_pick_uniform(A.seed, A.iter, wid);
            if (A.wrec) {
                const double2 lp = *reinterpret_cast<const double2*>(&A.wrec[gi].L);
                Lold = lp.x; Pold = lp.y;
            } else {
                Lold = A.L[gi];
                Pold = A.P[gi];
            }
        }
        T.s_rs[lane] = rs;
        T.s_flag[lane] = valid ? F_VALID : 0;
    }
    __syncthreads();

    // ---- phase B1: the tries; the generator's terms at the OLD row, in the segment's first row
    const int e = T.e;
    const bool speaker = T.jl == 0;
    const double2 glov = *reinterpret_cast<const double2*>(A.glo + e);
    const double2 ghiv = *reinterpret_cast<const double2*>(A.ghi + e);
    const PriorTerm g0 = A.gterms[e], g1 = A.gterms[e + 1];
    const bool pads = g0.kind == PRIOR_NONE || g1.kind == PRIOR_NONE;
    double* __restrict__ pool = A.pool;
    auto q_at = [&](int r) { return *reinterpret_cast<const double2*>(T.qtile + r * RS + e); };
#pragma unroll
    for (int p = 0; p < Tile::NPASS; ++p) {
        const int r = p * Tile::RPP + T.rsub;
        const bool rvalid = (r < TILE) && (T.s_flag[r < TILE ? r : 0] & F_VALID) != 0;
        const bool first = (r & (KP - 1)) == 0;
        PairTerms pt = NO_PAIR;
        if (rvalid) {
            const int own = k0 + (r >> sh), rk = r & (KP - 1);
            double2 sv{0.0, 0.0};
            if (first || pads) sv = *reinterpret_cast<const double2*>(pool + (size_t)T.s_rs[r] * D + e);
            double2 qv;
            if (forced) {
                qv = *reinterpret_cast<const double2*>(A.q + (((size_t)tl * W + own) * K + rk) * D + e);
            } else {
                const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)W + (uint32_t)own;
                qv.x = dist_draw(A.seed, A.iter, wid, e, g0, glov.x, ghiv.x, (uint32_t)rk);
                qv.y = dist_draw(A.seed, A.iter, wid, e + 1, g1, glov.y, ghiv.y, (uint32_t)rk);
            }
            if (g0.kind == PRIOR_NONE) qv.x = sv.x;         // a pad: no draw, no term
            if (g1.kind == PRIOR_NONE) qv.y = sv.y;
            *reinterpret_cast<double2*>(T.qtile + r * RS + e) = qv;
            if (first) pt = T.put_terms(r, pair_terms<true>(g0, g1, glov, ghiv, sv));   // log q(old), multipletry.py:387
        }
        dist_row_all(pt.ok, LPR, lane, speaker && rvalid && first, &T.s_flag[r < TILE ? r : 0], F_OLD);
    }
    __syncthreads();
    double sum_old = 0.0;
    if (wv == 0 && valid && kt == 0) sum_old = T.term_sum(lane, A.gterms);
    __syncthreads();

    // ---- phase B2: the generator's terms at the NEW rows; under a box prior the rows' ballots
    const double2 lov = *reinterpret_cast<const double2*>(A.lo + e);
    const double2 hiv = *reinterpret_cast<const double2*>(A.hi + e);
    T.rows([&](int r, int fl) {
        const bool rvalid = (fl & F_VALID) != 0;
        PairTerms pt = NO_PAIR;
        bool inbox = true;
        if (rvalid) {
            const double2 qv = q_at(r);
            pt = T.put_terms(r, pair_terms<true>(g0, g1, glov, ghiv, qv));          // log q(y_k), mtdistgen.py:77-79
            inbox = pair_inside(qv, lov, hiv);                                      // prior.py:80-88
        }
        dist_row_all(pt.ok, LPR, lane, speaker && rvalid, &T.s_flag[r < TILE ? r : 0], F_NEW);
        if (!A.pterms) row_verdict(inbox, pt.finite, LPR, lane, speaker && rvalid, &T.s_flag[r < TILE ? r : 0], A.flags);
    });
    __syncthreads();
    double lq = -INFINITY;
    if (wv == 0 && valid && (T.s_flag[lane] & F_NEW)) lq = T.term_sum(lane, A.gterms);

    // ---- phase B3 (prior terms): the prior's supports and terms at the new rows, by k_stretch_prior's rule
    if (A.pterms) {
        __syncthreads();
        const PriorTerm t0 = A.pterms[e], t1 = A.pterms[e + 1];
        T.rows([&](int r, int fl) {
            const bool rvalid = (fl & F_VALID) != 0;
            PairTerms pt = NO_PAIR;
            if (rvalid) pt = T.put_terms(r, pair_terms<false>(t0, t1, lov, hiv, q_at(r)));
            row_verdict(pt.ok, pt.finite, LPR, lane, speaker && rvalid, &T.s_flag[r < TILE ? r : 0], A.flags);
        });
    }
    if constexpr (DT != 32) mfr = like_prefetch<DT, LIKE, NW>(lane, wv, A.prec_sym);   // (the matrix operand of phase C: in flight across the barrier)
    __syncthreads();

    // ---- phase C, phase D
    const double logl = T.template logl<LIKE>(A, lane, wv, wv == 0 && valid, mfr);
    if (wv == 0) {                                 // (all 64 lanes: the segmented steps read their neighbours)
        const double beta = A.tempered ? A.betas[A.rung_begin + tl] : 1.0;
        double ll = 0.0, lp = -INFINITY, logP = -INFINITY, w = -INFINITY;
        if (valid) {
            ll = logl;
            if (T.s_flag[lane] & F_IN) lp = A.pterms ? T.term_sum(lane, A.pterms) : A.logp_in;   // prior.py:364-383 / 80-88
            logP = beta * ll + lp;                                                  // multipletry.py:221-223
            w = logP - lq;                                                          // multipletry.py:45
        }
        const double lsw = seg_logsumexp(w, valid, KP, lane);
        double cs = valid ? exp(w - lsw) : 0.0;                                     // multipletry.py:51-57
        for (int off = 1; off < KP; off <<= 1) {
            const double below = __shfl_up(cs, off, KP);
            if (kt >= off) cs += below;
        }
        const unsigned long long above = row_ballot(valid && cs > up, KP, lane);
        const int j = above != 0ull ? (int)__builtin_ctzll(above) - base : 0;
        const double ll_j = __shfl(ll, base + j), lp_j = __shfl(lp, base + j), lq_j = __shfl(lq, base + j), logP_j = __shfl(logP, base + j);
        // the auxiliary set: the current point in the picked try's place (multipletry.py:381-417)
        const double lq_old = (T.s_flag[base] & F_OLD) ? __shfl(sum_old, base) : -INFINITY;
        const double logP_old = beta * Lold + Pold;
        const double aux_lsw = seg_logsumexp(kt == j ? logP_old - lq_old : w, valid, KP, lane);
        const double factors = ((logP_old - aux_lsw) - lq_old + lq_old) - ((logP_j - lsw) - lq_j + lq_j);   // multipletry.py:472-476
        if (wvalid && kt == 0) {
            const bool keep = accept_test(A.tempered, [&] { return beta; }, ll_j, lp_j, Lold, Pold, factors, lu);
            if (keep) {
                const double newP = stored_logp(lp_j);
                if (A.wrec) {
                    *reinterpret_cast<double2*>(&A.wrec[gi].L) = double2{ll_j, newP};
                } else {
                    A.L[gi] = ll_j;
                    A.P[gi] = newP;
                }
                atomicAdd(&A.accepted[gi], 1u);
                atomicOr(&T.s_flag[base + j], F_KEEP);
            }
            const size_t TW = (size_t)A.Tl * W;
            if (A.keep_out) A.keep_out[gi] = keep ? 1 : 0;
            if (A.factors_out) A.factors_out[gi] = factors;
            if (A.pick_out) A.pick_out[gi] = j;
            if (A.lsw_out) { A.lsw_out[gi] = lsw; A.lsw_out[TW + gi] = aux_lsw; }
        }
    }
    __syncthreads();

    // ---- phase E: the picked row of an accepted walker, in place
    T.rows([&](int r, int fl) {
        if ((fl & (F_VALID | F_KEEP)) != (F_VALID | F_KEEP)) return;
        *reinterpret_cast<double2*>(pool + (size_t)T.s_rs[r] * D + e) = q_at(r);
    });
}

}  // namespace hens
