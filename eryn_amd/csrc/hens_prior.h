// hens_prior.h - the term tile (TermTile<DT, NW> and the device functions on it, shared with k_dist: hens_dist.h) and
// k_stretch_prior<DT, LIKE, MODE, NW>: the copying half-step at a compile-time row width under per-parameter prior terms
// (hens_set_prior_terms; PriorTerm: hens_prior_host.h; prior_term: hens_kernels.h).
//
// One workgroup = TILE (64) walkers of one rung, NW wavefronts, the five phases of k_stretch_fast's copying launch without what a
// single, non-pipeline context on the copying path does not need: no PIPE, no folded adaptation (k_adapt stands alone), no rows in
// place, no walker records, no column order, no periodic parameters (those contexts take the generic k_stretch), planned draws only.
// It shares hens_kernels.h's device functions (like_partials and the matrix-pipe tiles, like_prefetch, prior_term) and copies none.
//   phase A  lane-per-walker : indices, draws                                          (wave 0)
//   phase B  lanes-over-d    : 16-byte row gathers, q = c - (c - s) zz.  The lane that holds q_d in registers tests its support and
//                              forms t_d from the REGISTER (pair_terms; the tile holds q itself here, never q - mu:
//                              like_partials<.., CEN = false>, the form the MH launches of k_stretch_fast use at every width); a
//                              non-finite term (a normal coordinate whose y y overflows) counts as outside the support, so the
//                              likelihood is skipped and filled as the reference does for a -inf prior.  The verdict joins the row's
//                              ballot; q goes to the proposal tile, t to the term tile
//   phase C  lane-per-walker : likelihood partial sums, the dense kind on the matrix pipe at D = 32 / 64 / 128        (TermTile::logl)
//   phase D  lane-per-walker : wave 0 adds its walker's terms in ascending d from 0.0 (term_sum), tempered MH test, L / P / loc /
//                              accept counters
//   phase E  lanes-over-d    : the new row (q if kept, the old row otherwise) to its home in the other half of the pool
// Term tile: [TILE][DT + 1] doubles.  The accept wave reads lane l's row with ds_read_b64 at a lane stride of 2 (DT + 1) dwords, an
// odd number of bank pairs: the 32 lanes of a group land on 32 distinct bank pairs of the 64 - conflict-free - where the proposal
// tile's stride DT + 2 (chosen for its b128 reads) would put lanes l and l + 16 on one pair at DT = 32, 64, 128.  D = 128, NW = 8:
// 66.6 kB proposal tile + 66.0 kB term tile + 1 kB mu + 5.6 kB = 139 kB of the CU's 160: it fits, one workgroup per CU.
// Launched on the HIP stream with a release, like every copying launch; not among the fence-free kernels of the store census.
//
// GIBBS (hens_set_gibbs; instantiated in a unit of its own, MODE_STRETCH and MODE_MH): the half-step of ONE Gibbs block
// (move.py:113-221, red_blue.py:119-333, mh.py:79-193).  The launch's term block carries the block's coordinate mask behind the
// records (prior_on == 2, gibbs_mask_of); the lane that holds coordinates e, e + 1 reads its two mask words once and phase B forms
// q_d = m_d ? proposal : s_d - a frozen coordinate is the old row's BITS (a select, never s + 0.0: the sign of a zero survives;
// move.py:321-324 puts the old values back).  Pads are frozen by the host's mask.  Everything else is the code above, called: the
// supports and terms of the whole row, the likelihood of the whole row, the accept test, phase E.  The planned Hastings factor is
// the block's, (n_b - 1) log zz (stretch.py:55-72).
#pragma once
#include "hens_kernels.h"

namespace hens {

// what the host asks for at a launch; TermTile is what the kernels carve, and asserts that the two agree
__host__ __device__ constexpr size_t prior_lds_bytes(int D, int NW, int like) {
    return ((size_t)TILE * (D + 2) + (size_t)TILE * (D + 1) + TILE + (size_t)NW * TILE) * 8 + 4 * (size_t)TILE * 4 + 16 + mf_lds_extra(D, like);
}

// One coordinate pair against its supports, its terms formed from the registers that hold it (prior.py:364-383).  A non-finite term
// counts as outside; tx / ty are 0.0 for a pad (PRIOR_NONE: term_sum skips it) and wherever `ok` is false (never read then).
// PADS_PASS: a pad is inside without a test (the generator's rule, dist_term of old); else every coordinate is tested, a NaN pad
// is outside (the prior's rule).
struct PairTerms {
    double tx, ty;
    bool ok, finite;
};
constexpr PairTerms NO_PAIR{0.0, 0.0, true, true};      // a lane without a row in this round of a pass: nothing to object to

// The LDS of one workgroup of k_stretch_prior / k_dist, and this thread's place in a pass over the tile's rows.
template <int DT, int NW>
struct TermTile {
    static constexpr int D = DT, RS = DT + 2, TS = DT + 1;
    static constexpr int LPR = DT / 2;                // lanes per row, 16 B each
    static constexpr int RPP = NW * 64 / LPR;         // rows per pass
    static constexpr int NPASS = (TILE + RPP - 1) / RPP;
    // the carve, once: every array's offset is the end of the one before it
    static constexpr size_t O_Q = 0;                                       // double  qtile [TILE][RS] proposals
    static constexpr size_t O_T = O_Q + sizeof(double) * TILE * RS;        // double  ttile [TILE][TS] terms, one kind at a time
    static constexpr size_t O_ZZ = O_T + sizeof(double) * TILE * TS;       // double  s_zz  [TILE]
    static constexpr size_t O_PART = O_ZZ + sizeof(double) * TILE;         // double  s_part [NW][TILE]
    static constexpr size_t O_RS = O_PART + sizeof(double) * NW * TILE;    // int32_t s_rs  [TILE] own row
    static constexpr size_t O_RC = O_RS + sizeof(int32_t) * TILE;          // int32_t s_rc  [TILE] complement row
    static constexpr size_t O_DST = O_RC + sizeof(int32_t) * TILE;         // int32_t s_dst [TILE] destination row
    static constexpr size_t O_FLAG = O_DST + sizeof(int32_t) * TILE;       // int32_t s_flag [TILE] F_* per walker of the tile (+ 4: the next 16 bytes)
    static constexpr size_t O_MU = O_FLAG + sizeof(int32_t) * (TILE + 4);  // double  s_mu  [D] dense D = 32 / 64 / 128: mu for the matrix pipe
    template <int LIKE>
    static constexpr size_t END = O_MU + (like_mf<DT, LIKE, NW>() ? sizeof(double) * D : 0);
    char* const raw;
    template <class X>
    __device__ __forceinline__ X* at(size_t off) const { return reinterpret_cast<X*>(raw + off); }
    double *const qtile = at<double>(O_Q), *const ttile = at<double>(O_T), *const s_zz = at<double>(O_ZZ), *const s_part = at<double>(O_PART), *const s_mu = at<double>(O_MU);
    int32_t *const s_rs = at<int32_t>(O_RS), *const s_rc = at<int32_t>(O_RC), *const s_dst = at<int32_t>(O_DST), *const s_flag = at<int32_t>(O_FLAG);
    const int jl, rsub, e;    // this thread's lane of its row, row of a pass, first of its two coordinates

    __device__ __forceinline__ TermTile(char* smem, int tid) : raw(smem), jl(tid & (LPR - 1)), rsub(tid / LPR), e(2 * jl) {
        static_assert(END<LIKE_DENSE> == prior_lds_bytes(DT, NW, LIKE_DENSE) && END<LIKE_DIAG> == prior_lds_bytes(DT, NW, LIKE_DIAG) &&
                          END<LIKE_ROSEN> == prior_lds_bytes(DT, NW, LIKE_ROSEN) && O_MU % 16 == 0,
                      "the launch's LDS size (prior_lds_bytes) is not the tile's");
    }

    // One pass over the tile's rows: f(r, fl) with this thread's row of each round and the row's flag word, 0 where the round has no
    // row for it (RPP exceeds TILE at D = 8 with 8 waves: not built, kept safe).  Every lane reaches every call of f: the ballots in it.
    template <class F>
    __device__ __forceinline__ void rows(F&& f) const {
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int r = p * RPP + rsub;
            f(r, r < TILE ? s_flag[r] : 0);
        }
    }

    // row r's pair of terms to the term tile
    __device__ __forceinline__ const PairTerms& put_terms(int r, const PairTerms& pt) const {
        ttile[r * TS + e] = pt.tx;
        ttile[r * TS + e + 1] = pt.ty;
        return pt;
    }

    // the wave that adds: walker `lane`'s terms of the tile, ascending from 0.0, pads skipped (prior.py:364-383)
    __device__ __forceinline__ double term_sum(int lane, const PriorTerm* __restrict__ terms) const {
        double acc = 0.0;
        const double* trow = ttile + lane * TS;
        for (int d = 0; d < D; ++d)
            if (terms[d].kind != PRIOR_NONE) acc += trow[d];
        return acc;
    }

    // the head of both kernels: mu staged for the matrix pipe, its D = 32 operands requested
    template <int LIKE, class Args>
    __device__ __forceinline__ MfRegs prologue(const Args& A, int tid, int lane, int wv) const {
        if constexpr (like_mf<DT, LIKE, NW>()) {
            if (tid < DT / 2) *reinterpret_cast<double2*>(s_mu + 2 * tid) = *reinterpret_cast<const double2*>(A.mu + 2 * tid);
        }
        return like_prefetch<DT == 32 ? DT : 0, LIKE, NW>(lane, wv, A.prec_sym);
    }

    // phase C and the head of phase D: the proposal tile's log-likelihoods, in the lanes that add (`adds`: wave 0's valid walkers).
    // Every thread calls it (a barrier inside); the caller's barrier stands in front.
    template <int LIKE, class Args>
    __device__ __forceinline__ double logl(const Args& A, int lane, int wv, bool adds, const MfRegs& mfr) const {
        const bool inbox = (s_flag[lane] & F_IN) != 0;
        like_partials<DT, LIKE, NW, false>(qtile, s_part, lane, wv, inbox, like_mf<DT, LIKE, NW>() ? s_mu : A.mu, A.prec, A.prec_sym, A.rosen_a,
                                           A.rosen_b, mfr);
        __syncthreads();
        if (!adds) return 0.0;
        const bool in2 = (s_flag[lane] & F_IN) != 0;
        double acc = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < like_nparts<DT, LIKE, NW>(); ++w2) acc += s_part[w2 * TILE + lane];
        return nan_logl_rule(in2 ? -0.5 * acc : A.fill, A.flags);   // ensemble.py:1486-1513
    }
};

__device__ __forceinline__ bool pair_inside(const double2& q, const double2& lo, const double2& hi) {
    return (q.x >= lo.x) && (q.x <= hi.x) && (q.y >= lo.y) && (q.y <= hi.y);
}
__device__ __forceinline__ bool pair_finite(const double2& q) { return (fabs(q.x) < INFINITY) && (fabs(q.y) < INFINITY); }
template <bool PADS_PASS>
__device__ __forceinline__ PairTerms pair_terms(const PriorTerm& t0, const PriorTerm& t1, const double2& lo, const double2& hi, const double2& q) {
    const bool inx = (PADS_PASS && t0.kind == PRIOR_NONE) || ((q.x >= lo.x) && (q.x <= hi.x));
    const bool iny = (PADS_PASS && t1.kind == PRIOR_NONE) || ((q.y >= lo.y) && (q.y <= hi.y));
    PairTerms o{0.0, 0.0, inx && iny, pair_finite(q)};
    if (o.ok) {
        if (t0.kind != PRIOR_NONE) o.tx = prior_term(t0, q.x);
        if (t1.kind != PRIOR_NONE) o.ty = prior_term(t1, q.y);
        o.ok = (fabs(o.tx) < INFINITY) && (fabs(o.ty) < INFINITY);
    }
    return o;
}

template <int DT, int LIKE, int MODE, int NW, bool GIBBS = false>
__global__ __launch_bounds__(NW * 64) void k_stretch_prior(const StretchArgs A) {
    constexpr bool EVAL = MODE == MODE_EVAL, MH = MODE == MODE_MH;
    static_assert(DT == 8 || DT == 16 || DT == 32 || DT == 64 || DT == 128, "power-of-two row width");
    static_assert(!GIBBS || !EVAL, "an evaluation proposes nothing: no mask to apply");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    using Tile = TermTile<DT, NW>;
    constexpr int D = DT, RS = Tile::RS, LPR = Tile::LPR;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const Tile T(smem_raw, tid);
    const int tl = blockIdx.y;
    const int W = A.W;
    const int Ns = (EVAL || MH) ? W : (A.ns_x ? A.ns_x : (A.split == 0 ? A.N0 : W - A.N0));
    const int s_off = (EVAL || MH) ? 0 : (A.ns_x ? A.soff_x : (A.split == 0 ? 0 : A.N0));
    const int k0 = blockIdx.x * TILE;
    const PriorTerm* __restrict__ terms = prior_terms_of(A);

    MfRegs mfr = T.template prologue<LIKE>(A, tid, lane, wv);

    // ---- phase A
    double factors = 0.0, lu = 0.0, Lold = 0.0, Pold = 0.0;
    int own = 0;
    bool valid = false;
    if (wv == 0) {
        const int k = k0 + lane;
        valid = k < Ns;
        double zz = 1.0;
        int rs = 0, rc = 0;
        if (valid) {
            if (EVAL) {
                own = k;
                rs = A.loc[tl * W + own];
                rc = rs;
            } else if (MH) {                     // every walker proposes; no partner, no Hastings factor
                own = k;
                rs = A.loc[tl * W + own];
                rc = rs;
                lu = A.dr.lu[(size_t)tl * W + own];
                Lold = A.L[tl * W + own];
                Pold = A.P[tl * W + own];
            } else {
                const size_t di = (size_t)tl * W + s_off + k;
                own = A.dr.own[di];
                const int cw = A.dr.cw[di];
                zz = A.dr.zz[di];
                factors = A.dr.fac[di];
                lu = A.dr.lu[di];
                rs = A.loc[tl * W + own];
                rc = A.split == 1 ? A.home_off + tl * W + cw : A.loc[tl * W + cw];
                Lold = A.L[tl * W + own];
                Pold = A.P[tl * W + own];
            }
        }
        T.s_zz[lane] = zz;
        T.s_rs[lane] = rs;
        T.s_rc[lane] = rc;
        T.s_dst[lane] = A.home_off + tl * W + own;
        T.s_flag[lane] = valid ? F_VALID : 0;
    }
    __syncthreads();

    // ---- phase B: this lane's two coordinates, their supports and term records (the same for every row it meets)
    const int e = T.e;
    const double2 lov = *reinterpret_cast<const double2*>(A.lo + e);
    const double2 hiv = *reinterpret_cast<const double2*>(A.hi + e);
    const PriorTerm t0 = terms[e], t1 = terms[e + 1];
    int2 mk{1, 1};
    if constexpr (GIBBS) mk = *reinterpret_cast<const int2*>(gibbs_mask_of(A) + e);
    const double* __restrict__ pool_r = A.pool;
    T.rows([&](int r, int fl) {
        const bool rvalid = (fl & F_VALID) != 0;
        PairTerms pt = NO_PAIR;
        if (rvalid) {
            const double zz = T.s_zz[r];
            const double2 sv = *reinterpret_cast<const double2*>(pool_r + (size_t)T.s_rs[r] * D + e);
            double2 qv;
            if (EVAL) {
                qv = sv;
            } else {
                const double2 cv = MH ? *reinterpret_cast<const double2*>(A.mh_step + ((size_t)tl * W + k0 + r) * D + e)
                                      : *reinterpret_cast<const double2*>(pool_r + (size_t)T.s_rc[r] * D + e);
                if (MH) {
                    qv.x = sv.x + cv.x;               // gaussian.py:166-167
                    qv.y = sv.y + cv.y;
                } else {
                    qv.x = cv.x - (cv.x - sv.x) * zz; // stretch.py:143,145
                    qv.y = cv.y - (cv.y - sv.y) * zz;
                }
                if constexpr (GIBBS) {                // move.py:321-324: outside the block the old row, bit for bit
                    qv.x = mk.x ? qv.x : sv.x;
                    qv.y = mk.y ? qv.y : sv.y;
                }
            }
            *reinterpret_cast<double2*>(T.qtile + r * RS + e) = qv;
            pt = T.put_terms(r, pair_terms<false>(t0, t1, lov, hiv, qv));
        }
        row_verdict(pt.ok, pt.finite, LPR, lane, T.jl == 0 && rvalid, &T.s_flag[r], A.flags);   // (`ok`: inside every support, prior.py:364-383)
    });
    if constexpr (DT != 32) mfr = like_prefetch<DT, LIKE, NW>(lane, wv, A.prec_sym);   // (the matrix operand of phase C: in flight across the barrier)
    __syncthreads();

    // ---- phase C, phase D
    const double logl = T.template logl<LIKE>(A, lane, wv, wv == 0 && valid, mfr);
    if (wv == 0 && valid) {
        const bool inbox = (T.s_flag[lane] & F_IN) != 0;
        const double logp = inbox ? T.term_sum(lane, terms) : -INFINITY;
        const size_t gi = (size_t)tl * W + own;
        if (EVAL) {
            A.L[gi] = logl;
            A.P[gi] = logp;
        } else {
            const bool keep = accept_test(A.tempered, [&] { return A.betas[A.rung_begin + tl]; }, logl, logp, Lold, Pold, factors, lu);
            if (keep) {
                A.L[gi] = logl;
                A.P[gi] = stored_logp(logp);
                atomicAdd(&A.accepted[gi], 1u);
                atomicOr(&T.s_flag[lane], F_KEEP);
            }
            A.loc[gi] = T.s_dst[lane];
            if (A.keep_out) A.keep_out[(size_t)tl * Ns + k0 + lane] = keep ? 1 : 0;
        }
    }
    if (EVAL) return;
    __syncthreads();

    // ---- phase E
    double* __restrict__ pool_w = A.pool;
    T.rows([&](int r, int fl) {
        if (!(fl & F_VALID)) return;
        const double2 v = (fl & F_KEEP) ? *reinterpret_cast<const double2*>(T.qtile + r * RS + e)
                                        : *reinterpret_cast<const double2*>(pool_r + (size_t)T.s_rs[r] * D + e);
        *reinterpret_cast<double2*>(pool_w + (size_t)T.s_dst[r] * D + e) = v;
    });
}

}  // namespace hens
