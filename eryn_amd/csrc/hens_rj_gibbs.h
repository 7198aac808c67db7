// hens_rj_gibbs.h - Gibbs blocks over branches and leaf slots for the in-model Gaussian move on leaf-packing records:
// GaussianMove(cov, gibbs_sampling_setup=[...]) on a state of several branches and leaves (move.py:113-402 under mh.py:79-193,
// gaussian.py:68-115).  A block is a mask over the record's coordinates [ind_off]; per block, in table order:
//
//   member slot    a leaf slot with any true coordinate in the block's mask (`ir_keep`, move.py:278)
//   moved leaf     an ACTIVE leaf in a member slot: q = x + step on its coordinates whose mask entry is true; every other coordinate
//                  of the record keeps its bits (move.py:322-324)
//   log-prior      over every active leaf of every branch (ensemble.py:1189-1210: dead slots 0.0, NumPy's sum order per branch), then
//                  fix_logp_gibbs (move.py:368-402): a walker without a moved leaf gets -inf if a branch OUTSIDE the block holds a
//                  leaf, else 0.0 - the reference counts a block's own branches by their member slots only (move.py:378-398), so a
//                  walker whose only leaves sit in non-member slots of the block's branches gets 0.0 and is evaluated as it stands
//   likelihood     not evaluated where the log-prior is infinite or the walker has no leaf (`fill`; ensemble.py:1278-1306, 1486-1513)
//   accept         factors 0 (gaussian.py:104): beta logl + logp - (beta L + P) > log u (mh.py:155-157), Move.update (move.py:472-703)
//
// and the next block starts from the state the last one left.  An in-model proposal depends on no other walker, so ONE wavefront
// walks all blocks [b0, b1) of an iteration on one load of its record and its resident template: one launch per iteration instead
// of one per block.  The device does not skip a block that no walker has a moved leaf in (mh.py:105-107 does, before any draw): every
// walker of such a block is rejected by fix_logp_gibbs, and the draws are counter-based, so nothing else depends on it.
//
// Unit of work: k_rj's - one wavefront per walker, grid x over the walkers, y over the rungs.  Phases:
//   1  record -> LDS, L / P -> registers, the resident template row -> registers (ndata <= 512: 8 doubles per lane, k_rj's strided
//      layout); (wave 0 of the launch: the folded ladder adaptation, RjArgs::ad, as k_rj / k_rj_mt have it)
//   2  per block: member slots (a lane per slot), the steps - the caller's, or scale x unit normal from Philox with the block in the
//      key - with the mask put-back, the prior (a lane per slot, summed in k_rj's order), fix_logp_gibbs, the likelihood:
//        production (tm != nullptr): for every moved leaf in ascending (branch, slot) order, per data point
//            template = (template - leaf_old) + leaf_new
//          - 2 m leaf evaluations for m moved leaves instead of every active leaf's;
//        parity (tm == nullptr): full evaluation of the walker's active leaves in k_rj's order - per-branch sums for the pulse /
//          sine box models, one running template otherwise (RjGibbsArgs::per_branch, as RjMtArgs::per_branch)
//      - the residual sum reduced across the wave as k_rj's birth / death by difference does; the accept test; on acceptance the
//      record in LDS, L, P and the register template take the proposal
//   3  one store of the record's coordinates, L, P and the template if any block was accepted; `accepted` += accepted blocks;
//      keep_out when the range is a single block.
// Every leaf value is per point (rj_leaf_at): the uniform-grid recurrences of k_rj (pulse / sine, RjModel::t_step64) are not used
// here - a block's 2 m leaves are a fraction of k_rj's sum, and the by-difference rule needs old and new leaf at the same points.
// Log-prior, fix_logp_gibbs, accept and update are stated here again (with their citations): k_rj's text is untouched, so its
// instantiations' code cannot change.
//
// Draws (production): block k's unit normal of record coordinate i is the call keyed rj_normal_key(i) | k << 25 (rj_normal_key uses
// bits 0 - 24), its accept uniform the call keyed rj_acc_key(RJ_MODE_MH, 0) | k << 19 (rj_acc_key uses bits 0 - 18); k < 128.
// Block 0's words are those of a context without a table.
#pragma once
#include "hens_rj.h"

namespace hens {

constexpr int RJ_GIBBS_MAX_BLOCKS = 128;
__device__ __forceinline__ uint32_t rj_gibbs_normal_key(int i, int block) { return rj_normal_key(i) | ((uint32_t)block << 25); }
__device__ __forceinline__ uint32_t rj_gibbs_acc_key(int block) { return rj_acc_key(RJ_MODE_MH, 0) | ((uint32_t)block << 19); }
__device__ __forceinline__ double rj_gibbs_unit_normal(uint64_t seed, uint64_t it, uint32_t wid, int i, int block) {
    const u4 d = rj_philox(seed, it, wid, rj_gibbs_normal_key(i, block));
    return mh_normal_from32(d.x, d.y).x;
}

struct RjGibbsArgs {
    RjArgs A;                    // k_rj's arguments (mode RJ_MODE_MH): walkers, model, data, step / u_acc or Philox, templates, adaptation
    const uint8_t* btab;         // [nblocks][M.ind_off] block table in record layout, non-zero: the coordinate moves with the block
    int32_t b0, b1;              // the launch walks blocks [b0, b1)
    int32_t per_branch;          // parity: a branch's leaves are summed on their own, then added (pulse / sine box models: k_rj's order)
    int32_t chol;                // Philox steps: L z per leaf out of RjArgs::ctab's Cholesky rows (hens_rj_set_mh_chol), else scale x z
};

// waves per SIMD the allocator is held to: three (168 VGPRs), as k_rj_mt.  Held to k_rj's four (128) the production instantiation
// spilled 103 registers and the parity one 27: the block loop keeps the resident template's 8 points, L, P and beta live across a
// per-point leaf evaluation with the library's sin inlined.  At three, with the proposal's template in LDS instead of a second set
// of registers and old and new leaf evaluated in two passes, the production instantiation still spills 8 (84 B of scratch), the
// parity one none (profiles/rj_gibbs_ab.txt has the resource lines).  Not measured: four waves with the template in LDS throughout.
#ifndef HENS_RJ_GIBBS_WPE
#define HENS_RJ_GIBBS_WPE 3
#endif
template <bool HAVE_TM>
__global__ __launch_bounds__(RJ_WAVES * 64) __attribute__((amdgpu_waves_per_eu(HENS_RJ_GIBBS_WPE))) void k_rj_gibbs(const RjGibbsArgs G) {
    const RjArgs& A = G.A;
    __shared__ double s_cur[RJ_WAVES][RJ_MAX_RW];
    __shared__ double s_q[RJ_WAVES][RJ_MAX_RW];
    __shared__ double s_leafv[RJ_WAVES][64];
    __shared__ double s_tab[64];
    // production: the proposal's template at the lane's points, point (ch, k) of lane l at [(ch NPT + k) 64 + l] - in LDS, not in a
    // second set of registers beside the resident template's (see HENS_RJ_GIBBS_WPE)
    __shared__ double s_tnew[HAVE_TM ? RJ_WAVES : 1][HAVE_TM ? 512 : 1];
    s_tab[threadIdx.x & 63] = RJ_EXP_TAB[threadIdx.x & 63];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int idx = (int)blockIdx.x * RJ_WAVES + wv;
    if (idx >= A.W) return;                          // whole wavefront (nothing below synchronises across waves)
    const int tl = (int)blockIdx.y;
    const int64_t gw = (int64_t)tl * A.W + idx;
    const RjModel& M = A.M;
    const int RW = M.RW, IO = M.ind_off;
    double* tnl = s_tnew[HAVE_TM ? wv : 0];
#define RJ_G_LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
    double* cur = s_cur[wv];
    double* q = s_q[wv];
    double* leafv = s_leafv[wv];
    double* row = A.pool + (size_t)A.loc[gw] * RW;
    for (int i = lane; i < RW; i += 64) cur[i] = row[i];
    RJ_G_LDS_SYNC();
    // the leaf masks (an in-model move never changes them), wave-uniform named scalars (k_rj: an array indexed by a run-time branch
    // goes to scratch)
    uint32_t mk0 = 0u, mk1 = 0u, mk2 = 0u, mk3 = 0u;
    for (int b = 0; b < M.nb; ++b) {
        const uint32_t v = __builtin_amdgcn_readfirstlane((uint32_t)cur[IO + b]);
        mk0 = b == 0 ? v : mk0; mk1 = b == 1 ? v : mk1; mk2 = b == 2 ? v : mk2; mk3 = b == 3 ? v : mk3;
    }
    auto mask_of = [&](const int b) { return (mk0 & (0u - (uint32_t)(b == 0))) | (mk1 & (0u - (uint32_t)(b == 1))) | (mk2 & (0u - (uint32_t)(b == 2))) | (mk3 & (0u - (uint32_t)(b == 3))); };
    const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)A.W + (uint32_t)idx;
    int total_leaves = 0;
    for (int b = 0; b < M.nb; ++b) total_leaves += __builtin_popcount(mask_of(b));

    if (HAVE_TM && A.ad_fold && blockIdx.x == 0 && blockIdx.y == 0 && wv == 0) {     // (production launches of hens_rj_step: k_rj's folded adaptation)
        __shared__ double s_ad[64];
        __shared__ unsigned s_adc[64];
        rj_adapt_wave(A.ad, lane, s_ad, s_adc);
        __threadfence();
        if (lane == 0) __hip_atomic_store(A.ad_flag, A.ad_serial, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }

    // this lane's leaf slot (lanes over the slots of all branches, <= 64: hens_rj_set_gibbs): branch, slot in the branch, first coordinate
    int s_b = -1, s_n = 0, s_i0 = 0, s_nd = 0;
    for (int b = 0; b < M.nb; ++b) {
        const int n = lane - M.slot0[b];
        if (n >= 0 && n < M.nl[b]) { s_b = b; s_n = n; s_nd = M.nd[b]; s_i0 = M.off[b] + n * M.nd[b]; }
    }
    const bool s_active = s_b >= 0 && ((mask_of(s_b) >> s_n) & 1u);
    const bool pri = M.prior_on != 0;
    double Lcur = A.L[gw], Pcur = A.P[gw];
    constexpr int NPT = 4, MAXCH = 2;                        // (k_rj's strided form: template points per lane and chunk; ndata <= 512)
    double tmk[MAXCH][NPT];                                  // production: the walker's template at this lane's points
    double* tmrow = HAVE_TM ? A.tm + (size_t)A.loc[gw] * M.ndata : nullptr;
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
        for (int k = 0; k < NPT; ++k) {
            const int i = ch * 64 * NPT + k * 64 + lane;
            tmk[ch][k] = (HAVE_TM && i < M.ndata) ? tmrow[i] : 0.0;
        }
    int sig_e = 0;
    const bool sig_pow2 = frexp(M.sigma, &sig_e) == 0.5 && sig_e > -1000 && sig_e < 1000;      // (k_rj: residual / sigma as the reference divides it)
    const double sig_inv = 1.0 / M.sigma;
    double beta = 1.0;
    bool have_beta = false;
    int nacc = 0;
    bool keep_last = false;

    for (int blk = G.b0; blk < G.b1; ++blk) {
        const uint8_t* bm = G.btab + (size_t)blk * IO;
        // ---- member slots, moved leaves (wave-uniform masks per branch) ---------------------------------------------------------
        bool member = false;
        if (s_b >= 0)
            for (int d = 0; d < s_nd; ++d) member = member || bm[s_i0 + d] != 0;
        const unsigned long long mvbits = __ballot(member && s_active);      // bit s: slot s holds a leaf that moves with the block
        const int here = __builtin_popcountll(mvbits);
        // fix_logp_gibbs's two counts (move.py:378-398): `here` the moved leaves; `total` = here + every leaf of the branches that
        // are NOT in the block (a branch is in the block if it has a member slot) - the leaves a block's own branches hold in
        // non-member slots are in neither count, as in the reference
        const unsigned long long membits = __ballot(member);
        int total_blk = here;
        for (int b = 0; b < M.nb; ++b) {
            const uint32_t full = M.nl[b] >= 32 ? 0xffffffffu : ((1u << M.nl[b]) - 1u);
            if (((uint32_t)(membits >> M.slot0[b]) & full) == 0u) total_blk += __builtin_popcount(mask_of(b));
        }
        // ---- proposal: q = x + step on the moved leaves' true coordinates, the old bits everywhere else ------------------------------
        for (int i = lane; i < IO; i += 64) {
            const int bn = A.cbn[i];
            const double x = cur[i];
            double v = x;
            if (((mvbits >> RJ_CBN_SLOT8(bn)) & 1ull) && bm[i] != 0) {
                double st;
                if (A.step) {
                    st = A.step[(size_t)gw * IO + i];
                } else {
                    const u4 dr = rj_philox(A.seed, A.iter, wid, rj_gibbs_normal_key(i, blk));
                    const double z = mh_normal_from32(dr.x, dr.y).x;
                    if (!G.chol) {
                        st = A.ctab[RJ_CTAB_SCALE + i] * z;
                    } else {
                        // correlated step L z per leaf (hens_rj_set_mh_chol; k_rj<.., CHOL>'s sums): the lane forms the lower
                        // coordinates' unit normals itself - a leaf with a partial mask still draws all its normals
                        const int d = RJ_CBN_D(bn);
                        const double l0 = A.ctab[RJ_CTAB_CHOL + i], l1 = A.ctab[RJ_CTAB_CHOL + RJ_MAX_RW + i], l2 = A.ctab[RJ_CTAB_CHOL + 2 * RJ_MAX_RW + i];
                        const double z1 = d >= 1 ? rj_gibbs_unit_normal(A.seed, A.iter, wid, i - 1, blk) : 0.0;
                        const double z2 = d >= 2 ? rj_gibbs_unit_normal(A.seed, A.iter, wid, i - 2, blk) : 0.0;
                        st = d == 0 ? l0 * z : (d == 1 ? l0 * z1 + l1 * z : (l0 * z2 + l1 * z1) + l2 * z);
                    }
                }
                v = x + st;                                                  // gaussian.py:96-104
            }
            // periodic leaf parameters (hens_rj_set_periodic): get_proposal wraps the whole arrays of the block's branches (gaussian.py:
            // 110-127), cleanup_proposals_gibbs puts back the coordinates outside the block's mask (move.py:322-324) - so every TRUE
            // coordinate of the mask is wrapped, moved or not, active or not, and every other coordinate keeps its bits
            if (A.per_on && bm[i] != 0) v = periodic_wrap(v, A.ctab[RJ_CTAB_PERIOD + i]);
            q[i] = v;
        }
        RJ_G_LDS_SYNC();
        // ---- log-prior: lane s the value of leaf slot s (k_rj's log-prior phase: 0.0 dead, the branch's constant or the slot's terms
        // ascending from 0.0, -inf outside a support or on a non-finite term), summed per branch in NumPy's order ---------------------
        if (s_b >= 0) {
            double sv = 0.0;
            if (s_active) {
                bool bad = false;
                double s = 0.0;
                for (int d = 0; d < s_nd; ++d) {
                    const int i = s_i0 + d;
                    const double x = q[i];
                    if (!(fabs(x) < INFINITY)) atomicOr(A.flags, FLAG_NONFINITE_X);      // ensemble.py:1258-1262
                    if (!((x >= A.ctab[RJ_CTAB_LO + i]) && (x <= A.ctab[RJ_CTAB_HI + i]))) { bad = true; continue; }
                    if (pri) {
                        const PriorTerm t{A.ctab[RJ_CTAB_C0 + i], A.ctab[RJ_CTAB_C1 + i], A.ctab[RJ_CTAB_C2 + i], RJ_CBN_PK(A.cbn[i]), 0};
                        const double tv = prior_term(t, x);
                        if (!(fabs(tv) < INFINITY)) bad = true;
                        s = s + tv;
                    }
                }
                sv = bad ? -INFINITY : (pri ? s : A.ctab[RJ_CTAB_LOGP + s_i0]);
            }
            leafv[lane] = sv;
        }
        RJ_G_LDS_SYNC();
        double logp = 0.0;
        for (int b = 0; b < M.nb; ++b) logp = logp + numpy_sum(leafv + M.slot0[b], M.nl[b]);
        if (total_blk != 0 && here == 0) logp = -INFINITY;                   // Move.fix_logp_gibbs (move.py:400-402)
        if (total_blk == 0 && here == 0) logp = 0.0;
        const bool evaluated = total_leaves > 0 && !(fabs(logp) == INFINITY);   // ensemble.py:1278-1306, 1486-1513
        // ---- likelihood -----------------------------------------------------------------------------------------------------------
        double logl = A.fill;
        if (evaluated) {
            double acc = 0.0;
            if constexpr (HAVE_TM) {
#pragma unroll
                for (int ch = 0; ch < MAXCH; ++ch) {
                    if (ch * 64 * NPT >= M.ndata) continue;                  // (wave-uniform)
                    double ti[NPT], tnew[NPT];
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        const int i = ch * 64 * NPT + k * 64 + lane;
                        ti[k] = A.tdata[i < M.ndata ? i : M.ndata - 1];
                        tnew[k] = tmk[ch][k];
                    }
                    unsigned long long m = mvbits;
                    while (m) {                                              // ascending slots = ascending (branch, slot in the branch)
                        const int s = __builtin_ctzll(m);
                        m &= m - 1ull;
                        int b = 0;
                        while (b + 1 < M.nb && s >= M.slot0[b + 1]) ++b;
                        const int i0 = M.off[b] + (s - M.slot0[b]) * M.nd[b];
                        // (two passes, the same operations per point: old and new leaf are not live together)
#pragma unroll 1
                        for (int side = 0; side < 2; ++side) {
                            const RjLeaf f = rj_leaf_load(M.kind[b], M.nd[b], (side == 0 ? cur : q) + i0);
                            const double sg = side == 0 ? -1.0 : 1.0;
#pragma unroll
                            for (int k = 0; k < NPT; ++k) tnew[k] = tnew[k] + sg * rj_leaf_at(f, ti[k], s_tab);
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        const int i = ch * 64 * NPT + k * 64 + lane;
                        tnl[(ch * NPT + k) * 64 + lane] = tnew[k];
                        if (i < M.ndata) {
                            const double d0 = tnew[k] - A.ydata[i];
                            const double r = sig_pow2 ? d0 * sig_inv : d0 / M.sigma;
                            acc += r * r;
                        }
                    }
                }
            } else {
                // parity: the reference's order of operations - every active leaf of the walker from the proposal (k_rj's strided form)
                for (int i0 = 0; i0 < M.ndata; i0 += 64 * NPT) {
                    double ti[NPT], tm[NPT];
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        const int i = i0 + k * 64 + lane;
                        ti[k] = i < M.ndata ? A.tdata[i] : 0.0;
                        tm[k] = 0.0;
                    }
                    for (int b = 0; b < M.nb; ++b) {
                        double sub[NPT];
#pragma unroll
                        for (int k = 0; k < NPT; ++k) sub[k] = 0.0;
                        uint32_t m = mask_of(b);
                        while (m) {
                            const int n = __builtin_ctz(m);
                            m &= m - 1u;
                            const RjLeaf f = rj_leaf_load(M.kind[b], M.nd[b], q + M.off[b] + n * M.nd[b]);
                            if (G.per_branch) {
#pragma unroll
                                for (int k = 0; k < NPT; ++k) sub[k] += rj_leaf_at(f, ti[k], s_tab);
                            } else {
#pragma unroll
                                for (int k = 0; k < NPT; ++k) tm[k] += rj_leaf_at(f, ti[k], s_tab);
                            }
                        }
                        if (G.per_branch) {
#pragma unroll
                            for (int k = 0; k < NPT; ++k) tm[k] += sub[k];
                        }
                    }
#pragma unroll
                    for (int k = 0; k < NPT; ++k) {
                        const int i = i0 + k * 64 + lane;
                        if (i < M.ndata) {
                            const double d0 = tm[k] - A.ydata[i];
                            const double r = sig_pow2 ? d0 * sig_inv : d0 / M.sigma;
                            acc += r * r;
                        }
                    }
                }
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
            logl = nan_logl_rule(-0.5 * acc, A.flags);
        }
        // ---- accept test (mh.py:155-157), update (Move.update, move.py:472-703) into the wave's own copy -------------------------
        double u;
        if (A.u_acc) {
            u = A.u_acc[gw];
        } else {
            const u4 du = rj_philox(A.seed, A.iter, wid, rj_gibbs_acc_key(blk));
            u = u01(du.x, du.y);
        }
        if (A.tempered && !have_beta) {          // (the first block's test: a wave that has to wait for its beta waits here and nowhere else)
            if (HAVE_TM && A.ad_fold) {              // the ladder of this launch: published by wave 0 (k_rj: relaxed agent-scope loads)
                while (__hip_atomic_load(A.ad_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.ad_serial) __builtin_amdgcn_s_sleep(4);
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                beta = __hip_atomic_load(A.betas + (A.rung_begin + tl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            } else {
                beta = A.betas[A.rung_begin + tl];
            }
            have_beta = true;
        }
        const double beta_now = beta;
        const bool keep = accept_test(A.tempered, [beta_now] { return beta_now; }, logl, logp, Lcur, Pcur, 0.0, log(u));
        if (keep) {
            for (int i = lane; i < IO; i += 64) cur[i] = q[i];
            Lcur = logl;
            Pcur = stored_logp(logp);
            if (HAVE_TM && evaluated) {          // (not evaluated: nothing moved that a template shows)
#pragma unroll
                for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
                    for (int k = 0; k < NPT; ++k)
                        if (ch * 64 * NPT < M.ndata) tmk[ch][k] = tnl[(ch * NPT + k) * 64 + lane];
            }
            nacc += 1;
        }
        keep_last = keep;
        RJ_G_LDS_SYNC();
    }

    // ---- 3: one store --------------------------------------------------------------------------------------------------------------
    if (nacc > 0) {
        for (int i = lane; i < IO; i += 64) row[i] = cur[i];
        if (lane == 0) {
            A.L[gw] = Lcur;
            A.P[gw] = Pcur;
            if (A.accepted) A.accepted[gw] += (uint32_t)nacc;
        }
        if constexpr (HAVE_TM) {
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
                for (int k = 0; k < NPT; ++k) {
                    const int i = ch * 64 * NPT + k * 64 + lane;
                    if (i < M.ndata) tmrow[i] = total_leaves > 0 ? tmk[ch][k] : 0.0;
                }
        }
    }
    if (lane == 0 && A.keep_out && G.b1 - G.b0 == 1) A.keep_out[gw] = keep_last ? 1 : 0;
#undef RJ_G_LDS_SYNC
}

// hens_rj_gibbs_debug_draws: block `block`'s in-model draws of iteration `iter` in hens_rj_mh_step's form (one thread per walker) - the
// functions k_rj_gibbs evaluates.  Every coordinate slot gets its step, as hens_rj_debug_draws's `step` does.
struct RjGibbsDebugArgs {
    RjModel M;
    double* step;        // [Tl][W][ind_off]
    double* u_mh;        // [Tl][W]
    uint64_t iter, seed;
    int32_t Tl, W, rung_begin, block;
    int32_t use_chol;    // hens_rj_set_mh_chol: step_d = sum_{j <= d} chol[b][d][j] z_j, ascending j (k_rj_debug_draws's sum)
    double chol[RJ_MAX_BRANCH][RJ_ND][RJ_ND];
};
__global__ void k_rj_gibbs_debug_draws(const RjGibbsDebugArgs A) {
    const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= (int64_t)A.Tl * A.W) return;
    const RjModel& M = A.M;
    const int tl = (int)(gw / A.W);
    const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)A.W + (uint32_t)(gw - (int64_t)tl * A.W);
    for (int i = 0; i < M.ind_off; ++i) {
        int b = 0;
        while (b + 1 < M.nb && i >= M.off[b + 1]) ++b;
        const int d = (i - M.off[b]) % M.nd[b];
        double st = 0.0;
        if (!A.use_chol) {
            st = M.mh_scale[b][d] * rj_gibbs_unit_normal(A.seed, A.iter, wid, i, A.block);
        } else {
            for (int j = 0; j <= d; ++j) {
                const double term = A.chol[b][d][j] * rj_gibbs_unit_normal(A.seed, A.iter, wid, i - d + j, A.block);
                st = j == 0 ? term : st + term;
            }
        }
        A.step[(size_t)gw * M.ind_off + i] = st;
    }
    const u4 du = rj_philox(A.seed, A.iter, wid, rj_gibbs_acc_key(A.block));
    A.u_mh[gw] = u01(du.x, du.y);
}

}  // namespace hens
