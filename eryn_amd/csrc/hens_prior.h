// hens_prior.h - k_stretch_prior<DT, LIKE, MODE, NW>: the copying half-step at a compile-time row width under per-parameter prior
// terms (hens_set_prior_terms; PriorTerm: hens_prior_host.h; prior_term: hens_kernels.h).
//
// One workgroup = TILE (64) walkers of one rung, NW wavefronts, the five phases of k_stretch_fast's copying launch without what a
// single, non-pipeline context on the copying path does not need: no PIPE, no folded adaptation (k_adapt stands alone), no rows in
// place, no walker records, no column order, no periodic parameters (those contexts take the generic k_stretch), planned draws only.
// It shares hens_kernels.h's device functions (like_partials and the matrix-pipe tiles, like_prefetch, prior_term) and copies none.
//   phase A  lane-per-walker : indices, draws                                          (wave 0)
//   phase B  lanes-over-d    : 16-byte row gathers, q = c - (c - s) zz.  The lane that holds q_d in registers tests its support and
//                              forms t_d from the REGISTER (the tile holds q itself here, never q - mu: like_partials<.., CEN = false>,
//                              the form the MH launches of k_stretch_fast use at every width); a non-finite term (a normal
//                              coordinate whose y y overflows) counts as outside the support, so the likelihood is skipped and
//                              filled as the reference does for a -inf prior.  The verdict joins the row's ballot; q goes to the
//                              proposal tile, t to the term tile
//   phase C  lane-per-walker : likelihood partial sums, the dense kind on the matrix pipe at D = 32 / 64 / 128
//   phase D  lane-per-walker : wave 0 adds its walker's terms in ascending d from 0.0 (prior.py:364-383; pads skipped), tempered MH
//                              test, L / P / loc / accept counters
//   phase E  lanes-over-d    : the new row (q if kept, the old row otherwise) to its home in the other half of the pool
// Term tile: [TILE][DT + 1] doubles.  The accept wave reads lane l's row with ds_read_b64 at a lane stride of 2 (DT + 1) dwords, an
// odd number of bank pairs: the 32 lanes of a group land on 32 distinct bank pairs of the 64 - conflict-free - where the proposal
// tile's stride DT + 2 (chosen for its b128 reads) would put lanes l and l + 16 on one pair at DT = 32, 64, 128.  D = 128, NW = 8:
// 66.6 kB proposal tile + 66.0 kB term tile + 1 kB mu + 5.6 kB = 139 kB of the CU's 160: it fits, one workgroup per CU.
// Launched on the HIP stream with a release, like every copying launch; not among the fence-free kernels of the store census.
#pragma once
#include "hens_kernels.h"

namespace hens {

__host__ __device__ constexpr size_t prior_lds_bytes(int D, int NW, int like) {
    return ((size_t)TILE * (D + 2) + (size_t)TILE * (D + 1) + TILE + (size_t)NW * TILE) * 8 + 4 * (size_t)TILE * 4 + 16 + mf_lds_extra(D, like);
}

template <int DT, int LIKE, int MODE, int NW>
__global__ __launch_bounds__(NW * 64) void k_stretch_prior(const StretchArgs A) {
    constexpr bool EVAL = MODE == MODE_EVAL, MH = MODE == MODE_MH;
    static_assert(DT == 8 || DT == 16 || DT == 32 || DT == 64 || DT == 128, "power-of-two row width");
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    constexpr int D = DT, RS = DT + 2, TS = DT + 1, NT = NW * 64;
    constexpr int LPR = DT / 2;                // lanes per row, 16 B each
    constexpr int RPP = NT / LPR;              // rows per pass
    constexpr int NPASS = (TILE + RPP - 1) / RPP;
    double* qtile = reinterpret_cast<double*>(smem_raw);                 // [TILE][RS] proposals
    double* ttile = qtile + TILE * RS;                                   // [TILE][TS] prior terms
    double* s_zz = ttile + TILE * TS;                                    // [TILE]
    double* s_part = s_zz + TILE;                                        // [NW][TILE]
    int32_t* s_rs = reinterpret_cast<int32_t*>(s_part + NW * TILE);      // [TILE] own row
    int32_t* s_rc = s_rs + TILE;                                         // [TILE] complement row
    int32_t* s_dst = s_rc + TILE;                                        // [TILE] destination row
    int32_t* s_flag = s_dst + TILE;                                      // bit0 inside every support, bit1 keep, bit2 valid
    double* s_mu = reinterpret_cast<double*>(s_flag + TILE + 4);         // [D] dense D = 32 / 64 / 128: mu for the matrix pipe (16-byte aligned)

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tl = blockIdx.y;
    const int W = A.W;
    const int Ns = (EVAL || MH) ? W : (A.ns_x ? A.ns_x : (A.split == 0 ? A.N0 : W - A.N0));
    const int s_off = (EVAL || MH) ? 0 : (A.ns_x ? A.soff_x : (A.split == 0 ? 0 : A.N0));
    const int k0 = blockIdx.x * TILE;
    const PriorTerm* __restrict__ terms = prior_terms_of(A);

    if constexpr (like_mf<DT, LIKE, NW>()) {
        if (tid < DT / 2) *reinterpret_cast<double2*>(s_mu + 2 * tid) = *reinterpret_cast<const double2*>(A.mu + 2 * tid);
    }
    MfRegs mfr = like_prefetch<DT == 32 ? DT : 0, LIKE, NW>(lane, wv, A.prec_sym);

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
        s_zz[lane] = zz;
        s_rs[lane] = rs;
        s_rc[lane] = rc;
        s_dst[lane] = A.home_off + tl * W + own;
        s_flag[lane] = valid ? 4 : 0;
    }
    __syncthreads();

    // ---- phase B: this lane's two coordinates, their supports and term records (the same for every row it meets)
    const int jl = tid & (LPR - 1);
    const int rsub = tid / LPR;
    const int e = 2 * jl;
    const double2 lov = *reinterpret_cast<const double2*>(A.lo + e);
    const double2 hiv = *reinterpret_cast<const double2*>(A.hi + e);
    const PriorTerm t0 = terms[e], t1 = terms[e + 1];
    const double* __restrict__ pool_r = A.pool;
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        const int r = p * RPP + rsub;
        const bool rvalid = (r < TILE) && (s_flag[r < TILE ? r : 0] & 4) != 0;   // (RPP exceeds TILE at D = 8 with 8 waves: not built, kept safe)
        bool ok = true, finite = true;
        if (rvalid) {
            const double zz = s_zz[r];
            const double2 sv = *reinterpret_cast<const double2*>(pool_r + (size_t)s_rs[r] * D + e);
            double2 qv;
            if (EVAL) {
                qv = sv;
            } else {
                const double2 cv = MH ? *reinterpret_cast<const double2*>(A.mh_step + ((size_t)tl * W + k0 + r) * D + e)
                                      : *reinterpret_cast<const double2*>(pool_r + (size_t)s_rc[r] * D + e);
                if (MH) {
                    qv.x = sv.x + cv.x;               // gaussian.py:166-167
                    qv.y = sv.y + cv.y;
                } else {
                    qv.x = cv.x - (cv.x - sv.x) * zz; // stretch.py:143,145
                    qv.y = cv.y - (cv.y - sv.y) * zz;
                }
            }
            ok = (qv.x >= lov.x) && (qv.x <= hiv.x) && (qv.y >= lov.y) && (qv.y <= hiv.y);
            finite = (fabs(qv.x) < INFINITY) && (fabs(qv.y) < INFINITY);
            double tx = 0.0, ty = 0.0;
            if (ok) {                                 // (from the registers that hold q_d; a pad's kind is NONE: phase D skips it)
                if (t0.kind != PRIOR_NONE) tx = prior_term(t0, qv.x);
                if (t1.kind != PRIOR_NONE) ty = prior_term(t1, qv.y);
                ok = (fabs(tx) < INFINITY) && (fabs(ty) < INFINITY);
            }
            *reinterpret_cast<double2*>(qtile + r * RS + e) = qv;
            ttile[r * TS + e] = tx;
            ttile[r * TS + e + 1] = ty;
        }
        row_verdict(ok, finite, LPR, lane, jl == 0 && rvalid, &s_flag[r], A.flags);   // (`ok`: inside every support, prior.py:364-383)
    }
    if constexpr (DT != 32) mfr = like_prefetch<DT, LIKE, NW>(lane, wv, A.prec_sym);   // (the matrix operand of phase C: in flight across the barrier)
    __syncthreads();

    // ---- phase C
    {
        const bool inbox = (s_flag[lane] & 1) != 0;
        like_partials<DT, LIKE, NW, false>(qtile, s_part, lane, wv, inbox, like_mf<DT, LIKE, NW>() ? s_mu : A.mu, A.prec, A.prec_sym, A.rosen_a,
                                           A.rosen_b, mfr);
    }
    __syncthreads();

    // ---- phase D
    if (wv == 0 && valid) {
        const bool inbox = (s_flag[lane] & 1) != 0;
        double acc = 0.0;
#pragma unroll
        for (int w2 = 0; w2 < like_nparts<DT, LIKE, NW>(); ++w2) acc += s_part[w2 * TILE + lane];
        const double logl = nan_logl_rule(inbox ? -0.5 * acc : A.fill, A.flags);   // ensemble.py:1486-1513
        double logp = -INFINITY;
        if (inbox) {                                           // prior.py:364-383: prior_vals += temp, ascending, from 0.0
            logp = 0.0;
            const double* trow = ttile + lane * TS;
            for (int d = 0; d < D; ++d)
                if (terms[d].kind != PRIOR_NONE) logp += trow[d];
        }
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
                atomicOr(&s_flag[lane], 2);
            }
            A.loc[gi] = s_dst[lane];
            if (A.keep_out) A.keep_out[(size_t)tl * Ns + k0 + lane] = keep ? 1 : 0;
        }
    }
    if (EVAL) return;
    __syncthreads();

    // ---- phase E
    double* __restrict__ pool_w = A.pool;
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
        const int r = p * RPP + rsub;
        if (r >= TILE) continue;
        const int fl = s_flag[r];
        if (!(fl & 4)) continue;
        const double2 v = (fl & 2) ? *reinterpret_cast<const double2*>(qtile + r * RS + e)
                                   : *reinterpret_cast<const double2*>(pool_r + (size_t)s_rs[r] * D + e);
        *reinterpret_cast<double2*>(pool_w + (size_t)s_dst[r] * D + e) = v;
    }
}

}  // namespace hens
