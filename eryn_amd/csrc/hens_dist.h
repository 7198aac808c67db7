// hens_dist.h - k_dist<DT, LIKE, NW>: the independence proposal of DistributionGenerate (distgen.py:34-104 under MHMove.propose,
// mh.py:56-193) as ONE full-ensemble launch at a compile-time row width.  Every walker of every resident rung is proposed a fresh
// point from a generator of per-coordinate terms (hens_set_dist_proposal: PriorTerm records with the meaning they have as prior
// terms) and carries the Hastings factor
//   factors = (0.0 + logq(old)) + (-logq(new))                                             (distgen.py:84,94,100)
// into the accept rule every stepping kernel shares (accept_test).
//
// On k_stretch_prior's term tile (TermTile, hens_prior.h: its LDS, row passes, pair_terms, term_sum, prologue and logl): one workgroup =
// TILE (64) walkers of one rung, NW = fast_nw(D) wavefronts.  Its own argument struct: StretchArgs' offsets are part of the timed kernels.
//   phase A  lane-per-walker : own row, {L, P} (walker record by slot in record mode, else by field), log u          (wave 0)
//   phase B  lanes-over-d    : the lane reads its two coordinates of the walker's own row; q is the caller's point (teacher-forced) or
//                              the device draw (dist_draw: one Philox call per coordinate, rj_birth_value's transform, clamped into
//                              a uniform / log-uniform support); a pad coordinate (PRIOR_NONE) keeps its value and has no term.
//                              Up to three per-coordinate terms, each formed by pair_terms from the lane's registers:
//                                B1 the generator's at the OLD coordinate, B2 the generator's at the NEW one, B3 the context's prior
//                                at the new one (contexts with prior terms; a box keeps its ballot and its constant logp_in)
//                              with three support tests: old row inside the generator (else logq(old) = -inf: never accepted), new
//                              row inside the generator (true after the clamp; kept), new row inside the prior (row_verdict: the
//                              likelihood is skipped and filled as for a -inf prior).  A non-finite normal term counts as outside.
//   sums                     : ONE [TILE][DT + 1] term tile, used in turn at every width: write terms, barrier, wave 0 adds its
//                              walker's terms ascending from 0.0 (prior.py:364-383), barrier.  Three tiles side by side would not fit
//                              at D = 128 (66.6 kB + 3 x 66.0 kB > 160 kB); one tile is prior_lds_bytes' 139 kB there.
//   phase C  lane-per-walker : likelihood partial sums
//   phase D  lane-per-walker : nan_logl_rule, accept_test with the factor, stored_logp; {L, P} to the record or the by-field arrays,
//                              the MH move's accept counter, keep_out / factors_out when given
//   phase E  lanes-over-d    : always in place - an accepted q overwrites the walker's own row, a rejected proposal writes nothing (a
//                              walker reads no row but its own: safe in both state forms); the pool's parity is not flipped.
// Plain stores; launched on the HIP stream with its release like every MH launch; not among the fence-free kernels of the store census.
#pragma once
#include "hens_kernels.h"
#include "hens_prior.h"

namespace hens {

struct DistArgs {
    double* pool;
    const int32_t* loc;
    double* L;
    double* P;
    WalkerRec* wrec;            // record mode (hens_step's packed state, slot order): {L, P} live in the walker records; else nullptr
    const double* betas;        // [T] or nullptr when not tempered
    const double* lo;           // [D] the prior's inclusive supports
    const double* hi;
    const PriorTerm* pterms;    // [D] the context's prior terms, or nullptr: a box with the constant logp_in
    const double* glo;          // [D] the generator's supports
    const double* ghi;
    const PriorTerm* gterms;    // [D] the generator's terms (PRIOR_NONE: a pad)
    const double* q;            // [Tl][W][D] teacher-forced proposals, or nullptr: device draws
    const double* lu;           // [Tl][W] log accept uniforms (teacher-forced), or nullptr: mh_log_uniform(seed, iter, wid)
    uint32_t* accepted;         // [Tl][W] the MH move's accept counts
    uint8_t* keep_out;          // [Tl][W] or nullptr
    double* factors_out;        // [Tl][W] or nullptr
    const double* mu;
    const double* prec;
    const double* prec_sym;
    unsigned* flags;
    double logp_in, fill, rosen_a, rosen_b;
    uint64_t seed, iter;
    int32_t Tl, W, rung_begin, tempered;
};

// Coordinate d of the point walker `wid` (= global rung * W + walker) is proposed in iteration `it`: Philox4x32-10 on
// (iter lo, iter hi, wid, PURPOSE_DIST | d << 8) keyed by the seed, the words turned into a value by the function that draws births
// (rj_birth_value).  A uniform or log-uniform draw is clamped into its support: rounding can put exp(log a) one ulp outside [a, b],
// where logq(new) = -inf and the factor would be +inf.  (Births are not clamped: there the generator is the prior and such a
// point is rejected.)  k_dist and the export kernel k_dist_draw evaluate this one function.  `k`: the try of a multiple-try move
// (hens_mt.h: word 3 = PURPOSE_DIST | d << 8 | k << 16); try 0's word is the word of this move.
__device__ __forceinline__ double dist_draw(uint64_t seed, uint64_t it, uint32_t wid, int d, const PriorTerm& t, double lo, double hi, uint32_t k = 0) {
    const u4 e = philox4x32_10(u4{(uint32_t)it, (uint32_t)(it >> 32), wid, PURPOSE_DIST | ((uint32_t)d << 8) | (k << 16)}, (uint32_t)seed, (uint32_t)(seed >> 32));
    const double v = rj_birth_value(e, t.kind, lo, hi, t.c0, t.c1);
    return t.kind == PRIOR_NORMAL ? v : fmin(fmax(v, lo), hi);
}

// row-wide AND of a generator support test: the lane that speaks for a valid row sets `bit` of its flag word when all its LPR lanes
// are inside (row_verdict's ballot without the prior's bit and the non-finite report).  Every lane of the wavefront calls it.
__device__ __forceinline__ void dist_row_all(bool ok, int LPR, int lane, bool speaks, int32_t* row_flag, int bit) {
    const unsigned long long bad = row_ballot(!ok, LPR, lane);
    if (speaks && bad == 0ull) atomicOr(row_flag, bit);
}

template <int DT, int LIKE, int NW>
__global__ __launch_bounds__(NW * 64) void k_dist(const DistArgs A) {
    static_assert(DT == 8 || DT == 16 || DT == 32 || DT == 64 || DT == 128, "power-of-two row width");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Tile = TermTile<DT, NW>;                 // (s_zz, s_rc and s_dst stay unused: one layout, one size)
    constexpr int D = DT, RS = Tile::RS, LPR = Tile::LPR;
    constexpr int F_OLD = 16, F_NEW = 32;          // row-flag bits of this kernel: old / new row inside the generator's supports

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Tile T(smem_raw, tid);
    const int tl = blockIdx.y;
    const int W = A.W;
    const int k0 = blockIdx.x * TILE;
    const bool forced = A.q != nullptr;

    MfRegs mfr = T.template prologue<LIKE>(A, tid, lane, wv);

    // ---- phase A
    double lu = 0.0, Lold = 0.0, Pold = 0.0;
    int own = 0;
    bool valid = false;
    if (wv == 0) {
        const int k = k0 + lane;
        valid = k < W;
        int rs = 0;
        if (valid) {
            own = k;
            const size_t gi = (size_t)tl * W + own;
            rs = A.loc[gi];
            lu = A.lu ? A.lu[gi] : mh_log_uniform(A.seed, A.iter, (uint32_t)(A.rung_begin + tl) * (uint32_t)W + (uint32_t)own);
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

    // ---- phase B1: own row, proposal, the generator's terms at the OLD row
    const int e = T.e;
    const bool speaker = T.jl == 0;
    const double2 glov = *reinterpret_cast<const double2*>(A.glo + e);
    const double2 ghiv = *reinterpret_cast<const double2*>(A.ghi + e);
    const PriorTerm g0 = A.gterms[e], g1 = A.gterms[e + 1];
    double* __restrict__ pool = A.pool;
    auto q_at = [&](int r) { return *reinterpret_cast<const double2*>(T.qtile + r * RS + e); };
    // (TermTile::rows' loop written out: as a lambda the unrolled rounds each repeat the draw's row-invariant work)
#pragma unroll
    for (int p = 0; p < Tile::NPASS; ++p) {
        const int r = p * Tile::RPP + T.rsub;
        const bool rvalid = (r < TILE) && (T.s_flag[r < TILE ? r : 0] & F_VALID) != 0;
        PairTerms pt = NO_PAIR;
        if (rvalid) {
            const double2 sv = *reinterpret_cast<const double2*>(pool + (size_t)T.s_rs[r] * D + e);
            double2 qv;
            if (forced) {
                qv = *reinterpret_cast<const double2*>(A.q + ((size_t)tl * W + k0 + r) * D + e);
            } else {
                const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)W + (uint32_t)(k0 + r);
                qv.x = dist_draw(A.seed, A.iter, wid, e, g0, glov.x, ghiv.x);
                qv.y = dist_draw(A.seed, A.iter, wid, e + 1, g1, glov.y, ghiv.y);
            }
            if (g0.kind == PRIOR_NONE) qv.x = sv.x;         // a pad: no draw, no term
            if (g1.kind == PRIOR_NONE) qv.y = sv.y;
            *reinterpret_cast<double2*>(T.qtile + r * RS + e) = qv;
            pt = T.put_terms(r, pair_terms<true>(g0, g1, glov, ghiv, sv));          // + log q(old), distgen.py:94
        }
        dist_row_all(pt.ok, LPR, lane, speaker && rvalid, &T.s_flag[r], F_OLD);
    }
    __syncthreads();
    double sum_old = 0.0;
    if (wv == 0 && valid) sum_old = T.term_sum(lane, A.gterms);
    __syncthreads();

    // ---- phase B2: the generator's terms at the NEW row; under a box prior the row's ballot
    const double2 lov = *reinterpret_cast<const double2*>(A.lo + e);
    const double2 hiv = *reinterpret_cast<const double2*>(A.hi + e);
    T.rows([&](int r, int fl) {
        const bool rvalid = (fl & F_VALID) != 0;
        PairTerms pt = NO_PAIR;
        bool inbox = true;
        if (rvalid) {
            const double2 qv = q_at(r);
            pt = T.put_terms(r, pair_terms<true>(g0, g1, glov, ghiv, qv));          // - log q(new), distgen.py:100
            inbox = pair_inside(qv, lov, hiv);                                      // prior.py:80-88
        }
        dist_row_all(pt.ok, LPR, lane, speaker && rvalid, &T.s_flag[r], F_NEW);
        if (!A.pterms) row_verdict(inbox, pt.finite, LPR, lane, speaker && rvalid, &T.s_flag[r], A.flags);
    });
    __syncthreads();
    double factors = 0.0;
    if (wv == 0 && valid) {
        const int fl = T.s_flag[lane];
        const double lq_old = (fl & F_OLD) ? sum_old : -INFINITY;
        const double lq_new = (fl & F_NEW) ? T.term_sum(lane, A.gterms) : -INFINITY;
        factors = (0.0 + lq_old) + (-lq_new);                                   // distgen.py:84,94,100
    }

    // ---- phase B3 (prior terms): the prior's supports and terms at the new row, by k_stretch_prior's rule
    if (A.pterms) {
        __syncthreads();
        const PriorTerm t0 = A.pterms[e], t1 = A.pterms[e + 1];
        T.rows([&](int r, int fl) {
            const bool rvalid = (fl & F_VALID) != 0;
            PairTerms pt = NO_PAIR;
            if (rvalid) pt = T.put_terms(r, pair_terms<false>(t0, t1, lov, hiv, q_at(r)));
            row_verdict(pt.ok, pt.finite, LPR, lane, speaker && rvalid, &T.s_flag[r], A.flags);
        });
    }
    if constexpr (DT != 32) mfr = like_prefetch<DT, LIKE, NW>(lane, wv, A.prec_sym);   // (the matrix operand of phase C: in flight across the barrier)
    __syncthreads();

    // ---- phase C, phase D
    const double logl = T.template logl<LIKE>(A, lane, wv, wv == 0 && valid, mfr);
    if (wv == 0 && valid) {
        const bool inbox = (T.s_flag[lane] & F_IN) != 0;
        double logp = -INFINITY;
        if (inbox) logp = A.pterms ? T.term_sum(lane, A.pterms) : A.logp_in;       // prior.py:364-383 / 80-88
        const size_t gi = (size_t)tl * W + own;
        const bool keep = accept_test(A.tempered, [&] { return A.betas[A.rung_begin + tl]; }, logl, logp, Lold, Pold, factors, lu);
        if (keep) {
            const double newP = stored_logp(logp);
            if (A.wrec) {
                *reinterpret_cast<double2*>(&A.wrec[gi].L) = double2{logl, newP};
            } else {
                A.L[gi] = logl;
                A.P[gi] = newP;
            }
            atomicAdd(&A.accepted[gi], 1u);        // (the MH move counts in an array of its own)
            atomicOr(&T.s_flag[lane], F_KEEP);
        }
        if (A.keep_out) A.keep_out[gi] = keep ? 1 : 0;
        if (A.factors_out) A.factors_out[gi] = factors;
    }
    __syncthreads();

    // ---- phase E: accepted rows only, in place
    T.rows([&](int r, int fl) {
        if ((fl & (F_VALID | F_KEEP)) != (F_VALID | F_KEEP)) return;
        *reinterpret_cast<double2*>(pool + (size_t)T.s_rs[r] * D + e) = q_at(r);
    });
}

}  // namespace hens
