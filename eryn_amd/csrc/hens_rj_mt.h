// hens_rj_mt.h - the multiple-try birth / death move on leaf-packing records: MTDistGenMoveRJ(generate_dist, num_try = K, rj = True)
// (mtdistgenrj.py:7-189 over multipletry.py:238-514 - the `elif self.rj` branch - and multipletry.py:597-776, inside
// ReversibleJumpMove.propose, rj.py:145-388).  One branch per proposal; coin, edge rule and leaf slot are DistributionGenerateRJ's
// (distgenrj.py:63-112) exactly as k_rj<RJ_MODE_BD> has them.  With beta the walker's rung, logq the generator's log-density of one
// leaf, lp(.) the log-prior of a whole walker and ll(.) its log-likelihood:
//
//   birth walker   base = the walker;                        ll_in = L, lp_in = P;        tries y_0 .. y_{K-1} from the generator
//   death walker   base = the walker without the dying leaf; ll_in, lp_in evaluated on it; try 0 IS the dying leaf (multipletry.py:
//                  315-317 fill_values), tries 1 .. K-1 fresh draws into the same slot
//   per try k      lp_k = lp(base + y_k in the slot);  ll_k = ll(base + y_k), `fill` where lp_k is infinite (not evaluated)
//                  lq_k = logq(y_k) + lp_in                                                               (multipletry.py:350-351)
//                  w_k  = (beta ll_k + lp_k) - lq_k                                                       (multipletry.py:45, 221-223)
//   lsw  = max w + log(sum exp(w - max w))                                                                (multipletry.py:25-33)
//   pick = first k with cumsum(exp(w - lsw))_k > u_pick, else 0; 0 on a death walker                      (multipletry.py:51-57, 365)
//   aux_logP = beta ll_in + lp_in;  aux_w = aux_logP - lp_in;  aux_lsw = logsumexp of K entries aux_w     (multipletry.py:419-431, 463)
//   factors = ((aux_logP - aux_lsw) - a + a) - ((logP_pick - lsw) - lq_pick + lq_pick), a = lp_in; negated on a death walker
//                                                                                                         (multipletry.py:472-480)
//   proposed (logl, logp) = (ll_pick, lp_pick) on a birth, (ll_in, lp_in) on a death                      (multipletry.py:373-374, 481-482)
// then ReversibleJumpMove.propose: + edge factors (rj.py:236-270), fix_logp_gibbs on logp (rj.py:303, move.py:368-402),
// factors + tempered(new) - tempered(old) > log u_acc (rj.py:330-332), Move.update (move.py:472-703).  DistributionGenerateRJ's own
// -+ logq factor is not added.  Every weight -inf, or a dying leaf outside the generator (lq_0 = -inf, w_0 = +inf), gives NaN sums
// and a rejection, as there.
//
// Unit of work: k_rj's - one wavefront per walker, grid x over the walkers, y over the rungs.  Phases:
//   1  record -> LDS; (wave 0 of the launch: the folded ladder adaptation, RjArgs::ad, as k_rj has it)
//   2  coin / leaf slot (the caller's, or the Philox call of the plain move), the K tries into LDS: the caller's, or the generator's
//      draws - lanes over (try, parameter) - by rj_birth_value on the generator's terms; a death walker's try 0 from the record
//   3  prior: lane s the value of leaf slot s of the record; lane k the try's prior value, its logq and the walker's lp_k (the
//      slots summed in NumPy's pairwise order per branch with the try in its slot); lp_in
//   4  likelihood, lanes over the data points, tries in a loop: every try is ONE leaf's values (rj_leaf_at) on the base -
//        production (tm != nullptr): base = the resident template (birth) / resident - dying leaf (death), try = base + leaf_k;
//        parity (tm == nullptr): every try a full evaluation of the walker's active leaves, the try in its slot, in k_rj's order
//      - the residual sum reduced across the wave; lane k keeps ll_k
//   5  wave-uniform: w, lsw, pick, the auxiliary sum, factors, edge factors, fix_logp_gibbs, accept test
//   6  update: the picked try into the slot or the mask bit cleared, L, P, the accepted template (production), accepted, keep_out
// The uniform-grid recurrences of k_rj (pulse / sine, RjModel::t_step64) are not used here: every leaf value is per point.
// Edge factors, fix_logp_gibbs and the update are stated here a second time (with their citations): k_rj's text is untouched, so
// its instantiations' code cannot change.
#pragma once
#include "hens_rj.h"
#include "hens_mt.h"

namespace hens {

constexpr int RJ_MT_MAX_TRY = TILE;          // one lane per try
// draw kinds of the move: coordinate d of try k >= 1 (try 0 of a birth is the plain move's rj_birth_key(branch, d)); the pick uniform
enum : uint32_t { PURPOSE_RJ_TRY = 27, PURPOSE_RJ_PICK = 28 };
// parameter d in bits 8 - 9, try k in bits 10 - 15, branch in bits 16 - 17
__device__ __forceinline__ uint32_t rj_try_key(int branch, int d, int k) {
    return PURPOSE_RJ_TRY | ((uint32_t)d << 8) | ((uint32_t)k << 10) | ((uint32_t)branch << 16);
}
__device__ __forceinline__ uint32_t rj_pick_key(int branch) { return PURPOSE_RJ_PICK | ((uint32_t)branch << 16); }

// one leaf parameter's density record in device memory: lo, hi, c0, c1, c2, kind (as a double) - the fields of hens_rj_set_prior_terms
constexpr int RJ_MT_DENS = 6;
enum { RJ_MT_OUT_PICK = 0, RJ_MT_OUT_LSW = 1, RJ_MT_OUT_AUX = 2, RJ_MT_OUT_FACTORS = 3, RJ_MT_OUT_LL = 4, RJ_MT_OUT_LP = 5, RJ_MT_NOUT = 6 };

struct RjMtArgs {
    RjArgs A;                    // k_rj's arguments (mode RJ_MODE_BD, one branch): walkers, model, data, change / leaf / u_acc or Philox, templates, adaptation
    const double* tries;         // [Tl][W][K][M.ndmax] teacher-forced tries (a death walker's try 0 is ignored), or nullptr: Philox
    const double* u_pick;        // [Tl][W] pick uniforms, or nullptr: Philox
    double* out;                 // [RJ_MT_NOUT][Tl][W] pick, lsw, aux_lsw, factors (before the edge factors), mt_ll, mt_lp; or nullptr
    const double* gen;           // [M.nd[branch]][RJ_MT_DENS] the generator's terms of the launch's branch
    const double* pri;           // ... the prior's terms of the same leaf
    double gen_logq, pri_logp;   // an all-uniform generator's / prior's constant log-density inside its box
    int32_t K, gen_box, pri_box;
    int32_t per_branch;          // parity: a branch's leaves are summed on their own, then added (pulse / sine box models: k_rj's order); else one running template
};

// log-density of one leaf with parameters v[0 .. nd) under the terms `dn`: ((0.0 + t_0) + t_1) + ... ascending (prior.py:364-383), -inf
// if a parameter is outside its support or a term not finite; an all-uniform density: the constant `cst` inside the box
__device__ __forceinline__ double rj_mt_leaf_density(const double* dn, const int nd, const bool box, const double cst, const double* v) {
    double s = 0.0;
    bool bad = false;
    for (int d = 0; d < nd; ++d) {
        const double* r = dn + d * RJ_MT_DENS;
        const double x = v[d];
        if (!((x >= r[0]) && (x <= r[1]))) { bad = true; continue; }
        if (!box) {
            const PriorTerm tr{r[2], r[3], r[4], (int32_t)r[5], 0};
            const double t = prior_term(tr, x);
            if (!(fabs(t) < INFINITY)) bad = true;
            s = s + t;
        }
    }
    return bad ? -INFINITY : (box ? cst : s);
}

// numpy_sum (hens_rj.h) over v[0 .. n) with v[at] replaced by `val`
__device__ __forceinline__ double numpy_sum_sub(const double* v, const int n, const int at, const double val) {
    auto e = [&](const int i) { return i == at ? val : v[i]; };
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r = r + e(i);
        return r;
    }
    double r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = e(j);
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] = r[j] + e(i + j);
    double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + e(i);
    return res;
}

// waves per SIMD the allocator is held to: three (168 VGPRs) - the production instantiation keeps its 8 data points' t, y and base
// template across the tries' loop beside a leaf evaluation (the library's sin / cos among them) and takes 167; held to four it
// spilled 62 registers, the parity instantiation 10
#ifndef HENS_RJ_MT_WPE
#define HENS_RJ_MT_WPE 3
#endif
template <bool HAVE_TM>
__global__ __launch_bounds__(RJ_WAVES * 64) __attribute__((amdgpu_waves_per_eu(HENS_RJ_MT_WPE))) void k_rj_mt(const RjMtArgs G) {
    const RjArgs& A = G.A;
    __shared__ double s_cur[RJ_WAVES][RJ_MAX_RW];
    __shared__ double s_try[RJ_WAVES][RJ_MT_MAX_TRY][RJ_MAX_ND];
    __shared__ double s_leafv[RJ_WAVES][64];
    __shared__ double s_tab[64];
    s_tab[threadIdx.x & 63] = RJ_EXP_TAB[threadIdx.x & 63];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int idx = (int)blockIdx.x * RJ_WAVES + wv;
    if (idx >= A.W) return;                          // whole wavefront (nothing below synchronises across waves)
    const int tl = (int)blockIdx.y;
    const int64_t gw = (int64_t)tl * A.W + idx;
    const RjModel& M = A.M;
    const int RW = M.RW, K = G.K, B = A.branch, nd = M.nd[B], offB = M.off[B];
#define RJ_MT_TRACE(i) do { if (A.trace && gw < A.trace_n && lane == 0) A.trace[gw * 8 + (i)] = trace_stamp(); } while (0)
#define RJ_MT_LDS_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")
    RJ_MT_TRACE(0);
    double* cur = s_cur[wv];
    double (*tr)[RJ_MAX_ND] = s_try[wv];
    double* leafv = s_leafv[wv];
    double* row = A.pool + (size_t)A.loc[gw] * RW;
    for (int i = lane; i < RW; i += 64) cur[i] = row[i];
    RJ_MT_LDS_SYNC();
    // the leaf masks in front of the proposal, wave-uniform named scalars (k_rj: an array indexed by a run-time branch goes to scratch)
    uint32_t mo0 = 0u, mo1 = 0u, mo2 = 0u, mo3 = 0u;
    for (int b = 0; b < M.nb; ++b) {
        const uint32_t v = __builtin_amdgcn_readfirstlane((uint32_t)cur[M.ind_off + b]);
        mo0 = b == 0 ? v : mo0; mo1 = b == 1 ? v : mo1; mo2 = b == 2 ? v : mo2; mo3 = b == 3 ? v : mo3;
    }
    auto mask_old_of = [&](const int b) { return (mo0 & (0u - (uint32_t)(b == 0))) | (mo1 & (0u - (uint32_t)(b == 1))) | (mo2 & (0u - (uint32_t)(b == 2))) | (mo3 & (0u - (uint32_t)(b == 3))); };
    const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)A.W + (uint32_t)idx;

    if (HAVE_TM && A.ad_fold && blockIdx.x == 0 && blockIdx.y == 0 && wv == 0) {     // (production launches of hens_rj_step: k_rj's folded adaptation)
        __shared__ double s_ad[64];
        __shared__ unsigned s_adc[64];
        rj_adapt_wave(A.ad, lane, s_ad, s_adc);
        __threadfence();
        if (lane == 0) __hip_atomic_store(A.ad_flag, A.ad_serial, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
    RJ_MT_TRACE(1);

    // ---- 2: coin, leaf slot, tries --------------------------------------------------------------------------------------------
    const uint32_t moB = mask_old_of(B);
    const int nold = __builtin_popcount(moB);
    int c, lf;
    double u_acc, u_pick;
    const size_t tstride = (size_t)M.ndmax;
    if (A.change) {                                   // teacher-forced: everything is the caller's
        c = A.change[gw];
        lf = A.leaf[gw];
        u_acc = A.u_acc[gw];
        u_pick = G.u_pick[gw];
        for (int e = lane; e < K * nd; e += 64) {
            const int k = e / nd, d = e - k * nd;
            tr[k][d] = G.tries[((size_t)gw * K + k) * tstride + d];
        }
    } else {
        // the plain move's call (k_rj): lane 0 the coin and the leaf selector, lanes 1 .. nd try 0's coordinates (a birth's: rj_birth_key),
        // lane nd + 1 the accept uniform; lane nd + 2 the pick uniform
        const uint32_t key = lane == 0 ? rj_bd_key(B) : (lane <= nd ? rj_birth_key(B, lane - 1) : (lane == nd + 1 ? rj_acc_key(RJ_MODE_BD, B) : rj_pick_key(B)));
        const u4 dr = rj_philox(A.seed, A.iter, wid, key);
        u_acc = __shfl(u01(dr.x, dr.y), nd + 1);
        u_pick = __shfl(u01(dr.x, dr.y), nd + 2);
        const uint32_t dx = __builtin_amdgcn_readfirstlane(dr.x), dy = __builtin_amdgcn_readfirstlane(dr.y);
        c = (dx & 1u) ? +1 : -1;                                  // distgenrj.py:63-66
        if (nold == M.nlmin[B]) c = +1;                           // :69-73 (nleaves_min != nleaves_max: hens_rj_set_mt_proposal)
        else if (nold == M.nl[B]) c = -1;
        const uint32_t full = M.nl[B] >= 32 ? 0xffffffffu : ((1u << M.nl[B]) - 1u);
        const uint32_t pool_bits = c > 0 ? (~moB & full) : moB;
        const int cnt = __builtin_popcount(pool_bits);
        lf = cnt ? nth_set_bit(pool_bits, rj_pick(dy, cnt)) : 0;   // uniform over the candidates (:97-112)
        if (lane >= 1 && lane <= nd) {
            const double* r = G.gen + (lane - 1) * RJ_MT_DENS;
            tr[0][lane - 1] = rj_birth_value(dr, (int)r[5], r[0], r[1], r[2], r[3]);
        }
        for (int e = lane; e < (K - 1) * nd; e += 64) {
            const int k = 1 + e / nd, d = e - (k - 1) * nd;
            const double* r = G.gen + d * RJ_MT_DENS;
            tr[k][d] = rj_birth_value(rj_philox(A.seed, A.iter, wid, rj_try_key(B, d, k)), (int)r[5], r[0], r[1], r[2], r[3]);
        }
    }
    const bool birth = c > 0;
    RJ_MT_LDS_SYNC();
    if (!birth && lane < nd) tr[0][lane] = cur[offB + lf * nd + lane];      // multipletry.py:315-317: try 0 is the leaf that would die
    RJ_MT_LDS_SYNC();
    const uint32_t mbase = moB & ~(1u << lf), mtry = moB | (1u << lf);      // the branch's mask of the base; of base + a try
    const uint32_t mnew = birth ? mtry : mbase;

    RJ_MT_TRACE(2);
    // ---- 3: prior ---------------------------------------------------------------------------------------------------------------
    // lane s: the value of leaf slot s of the record as it is (ensemble.py:1189-1210: dead slots 0.0) - a box model's constant or the
    // slot's prior terms out of RjArgs::ctab, as k_rj's log-prior phase forms them
    const bool pri = M.prior_on != 0;
    for (int b = 0; b < M.nb; ++b) {
        const int n = lane - M.slot0[b];
        if (n >= 0 && n < M.nl[b]) {
            double sv = 0.0;
            if ((mask_old_of(b) >> n) & 1u) {
                const int i0 = M.off[b] + n * M.nd[b];
                bool bad = false;
                double s = 0.0;
                for (int d = 0; d < M.nd[b]; ++d) {
                    const int i = i0 + d;
                    const double x = cur[i];
                    if (!((x >= A.ctab[RJ_CTAB_LO + i]) && (x <= A.ctab[RJ_CTAB_HI + i]))) { bad = true; continue; }
                    if (pri) {
                        const PriorTerm t{A.ctab[RJ_CTAB_C0 + i], A.ctab[RJ_CTAB_C1 + i], A.ctab[RJ_CTAB_C2 + i], RJ_CBN_PK(A.cbn[i]), 0};
                        const double tv = prior_term(t, x);
                        if (!(fabs(tv) < INFINITY)) bad = true;
                        s = s + tv;
                    }
                }
                sv = bad ? -INFINITY : (pri ? s : A.ctab[RJ_CTAB_LOGP + i0]);
            }
            leafv[lane] = sv;
        }
    }
    RJ_MT_LDS_SYNC();
    // the walker's log-prior with `val` in slot lf of the branch: per branch NumPy's sum over the slots, branches in order from 0.0
    auto walker_logp = [&](const double val) {
        double lp = 0.0;
        for (int b = 0; b < M.nb; ++b)
            lp = lp + (b == B ? numpy_sum_sub(leafv + M.slot0[b], M.nl[b], lf, val) : numpy_sum(leafv + M.slot0[b], M.nl[b]));
        return lp;
    };
    const bool live = lane < K;
    double lp_k = -INFINITY, lq_leaf = -INFINITY;
    if (live) {
        bool fin = true;
        for (int d = 0; d < nd; ++d) fin = fin && (fabs(tr[lane][d]) < INFINITY);
        if (!fin) atomicOr(A.flags, FLAG_NONFINITE_X);                     // ensemble.py:1258-1262
        lp_k = walker_logp(rj_mt_leaf_density(G.pri, nd, G.pri_box != 0, G.pri_logp, tr[lane]));
        lq_leaf = rj_mt_leaf_density(G.gen, nd, G.gen_box != 0, G.gen_logq, tr[lane]);
    }
    const double Lold = A.L[gw], Pold = A.P[gw];
    const double lp_in = birth ? Pold : walker_logp(0.0);                  // multipletry.py:739-741 (no fix_logp_gibbs there)
    int others = 0;                                                         // active leaves outside the branch under proposal
    for (int b = 0; b < M.nb; ++b) others += b == B ? 0 : __builtin_popcount(mask_old_of(b));
    const int base_leaves = others + __builtin_popcount(mbase);

    RJ_MT_TRACE(3);
    // ---- 4: likelihood ----------------------------------------------------------------------------------------------------------
    // (a try is not evaluated where its walker's log-prior is infinite: ensemble.py:1278-1306; base + a try always holds a leaf)
    const unsigned long long evalmask = __ballot(live && !(fabs(lp_k) == INFINITY));
    int sig_e = 0;
    const bool sig_pow2 = frexp(M.sigma, &sig_e) == 0.5 && sig_e > -1000 && sig_e < 1000;      // (k_rj: residual / sigma as the reference divides it)
    const double sig_inv = 1.0 / M.sigma;
    constexpr int NPT = 4, MAXCH = 2;
    double ll_k = A.fill, ll_in = birth ? Lold : A.fill;
    double tmk[MAXCH][NPT];                                  // production: the base template at this lane's points (k_rj's strided layout)
#pragma unroll
    for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
        for (int k = 0; k < NPT; ++k) tmk[ch][k] = 0.0;
    double* tmrow = HAVE_TM ? A.tm + (size_t)A.loc[gw] * M.ndata : nullptr;
    const int kindB = M.kind[B];
    if constexpr (HAVE_TM) {
        double ti[MAXCH][NPT], yv[MAXCH][NPT];
#pragma unroll
        for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
            for (int k = 0; k < NPT; ++k) {
                const int i = ch * 64 * NPT + k * 64 + lane;
                const bool in = i < M.ndata;
                ti[ch][k] = in ? A.tdata[i] : 0.0;
                yv[ch][k] = in ? A.ydata[i] : 0.0;
                tmk[ch][k] = in ? tmrow[i] : 0.0;
            }
        // residual sum of (base + sg * leaf f) over the wave; `keep`: the sum becomes the base
        auto resid = [&](const RjLeaf& f, const bool with_leaf, const double sg, const bool keep) {
            double acc = 0.0;
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
                for (int k = 0; k < NPT; ++k) {
                    const int i = ch * 64 * NPT + k * 64 + lane;
                    double v = tmk[ch][k];
                    if (with_leaf) v += sg * rj_leaf_at(f, ti[ch][k], s_tab);
                    if (keep) tmk[ch][k] = v;
                    if (i < M.ndata) {
                        const double d0 = v - yv[ch][k];
                        const double r = sig_pow2 ? d0 * sig_inv : d0 / M.sigma;
                        acc += r * r;
                    }
                }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
            return nan_logl_rule(-0.5 * acc, A.flags);
        };
        if (!birth) {                                        // base = resident - dying leaf (a dead leaf's coordinates stay in the record)
            const RjLeaf f = rj_leaf_load(kindB, nd, cur + offB + lf * nd);
            const double l = resid(f, true, -1.0, true);
            ll_in = base_leaves > 0 ? l : A.fill;            // ensemble.py:1486-1513: no leaf, fill_zero_leaves_val
        }
        for (int k = 0; k < K; ++k) {
            if (!((evalmask >> k) & 1ull)) continue;         // (wave-uniform)
            const RjLeaf f = rj_leaf_load(kindB, nd, tr[k]);
            const double l = resid(f, true, 1.0, false);
            if (lane == k) ll_k = l;
        }
    } else {
        // parity: the reference's order of operations - every active leaf of the walker, the try in slot lf (trc == nullptr: the base)
        auto full_ll = [&](const uint32_t maskB, const double* trc) {
            double acc = 0.0;
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
                    uint32_t m = b == B ? maskB : mask_old_of(b);
                    while (m) {
                        const int n = __builtin_ctz(m);
                        m &= m - 1u;
                        const double* p = (b == B && n == lf && trc) ? trc : cur + M.off[b] + n * M.nd[b];
                        const RjLeaf f = rj_leaf_load(M.kind[b], M.nd[b], p);
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
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off);
            return nan_logl_rule(-0.5 * acc, A.flags);
        };
        if (!birth && base_leaves > 0) ll_in = full_ll(mbase, nullptr);
        for (int k = 0; k < K; ++k) {
            if (!((evalmask >> k) & 1ull)) continue;
            const double l = full_ll(mtry, tr[k]);
            if (lane == k) ll_k = l;
        }
    }

    RJ_MT_TRACE(4);
    // ---- 5: weights, pick, auxiliary sum, factors -------------------------------------------------------------------------------
    double beta = 1.0;
    if (A.tempered) {
        if (HAVE_TM && A.ad_fold) {              // the ladder of this launch: published by wave 0 (k_rj: relaxed agent-scope loads)
            while (__hip_atomic_load(A.ad_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != A.ad_serial) __builtin_amdgcn_s_sleep(4);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            beta = __hip_atomic_load(A.betas + (A.rung_begin + tl), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            beta = A.betas[A.rung_begin + tl];
        }
    }
    const double lq_k = lq_leaf + lp_in;                                   // multipletry.py:350-351
    const double logP_k = beta * ll_k + lp_k;                              // multipletry.py:221-223
    const double w = live ? logP_k - lq_k : -INFINITY;                     // multipletry.py:45
    const double lsw = seg_logsumexp(w, live, 64, lane);
    double cs = live ? exp(w - lsw) : 0.0;                                 // multipletry.py:51-57
    for (int off = 1; off < 64; off <<= 1) {
        const double below = __shfl_up(cs, off, 64);
        if (lane >= off) cs += below;
    }
    const unsigned long long above = __ballot(live && cs > u_pick);
    const int j = (birth && above != 0ull) ? (int)__builtin_ctzll(above) : 0;    // multipletry.py:365: try 0 on a death walker
    const double ll_j = __shfl(ll_k, j), lp_j = __shfl(lp_k, j), lq_j = __shfl(lq_k, j), logP_j = __shfl(logP_k, j);
    const double aux_logP = beta * ll_in + lp_in;                          // multipletry.py:419-428
    const double aux_w = aux_logP - lp_in;                                 // :431
    const double aux_ds = aux_w - aux_w;                                   // (K equal entries: w - max = 0, or NaN where aux_w is not finite)
    const double aux_lsw = aux_w + log((double)K * exp(aux_ds));           // :463 (the sum of K ones is exact)
    double mtf = (((aux_logP - aux_lsw) - lp_in) + lp_in) - (((logP_j - lsw) - lq_j) + lq_j);      // multipletry.py:472-476
    if (!birth) mtf = -mtf;                                                // :480
    const double mt_ll = birth ? ll_j : ll_in, mt_lp = birth ? lp_j : lp_in;      // :373-374, 481-482
    if (G.out && lane == 0) {
        const size_t TW = (size_t)A.Tl * A.W;
        G.out[RJ_MT_OUT_PICK * TW + gw] = (double)j; G.out[RJ_MT_OUT_LSW * TW + gw] = lsw; G.out[RJ_MT_OUT_AUX * TW + gw] = aux_lsw;
        G.out[RJ_MT_OUT_FACTORS * TW + gw] = mtf; G.out[RJ_MT_OUT_LL * TW + gw] = mt_ll; G.out[RJ_MT_OUT_LP * TW + gw] = mt_lp;
    }
    double edge = 0.0;
    if (!(M.nlmin[B] == M.nl[B] || M.nlmin[B] + 1 == M.nl[B])) {           // edge factors (rj.py:236-270)
        const int nnew = __builtin_popcount(mnew);
        const double lh = log(1 / 2.0);
        if (nold == M.nlmin[B]) edge += lh;
        if (nold == M.nl[B]) edge += lh;
        if (nnew == M.nlmin[B]) edge -= lh;
        if (nnew == M.nl[B]) edge -= lh;
    }
    const double factors = mtf + edge;                                     // rj.py:271
    double logp = mt_lp;
    const int here = __builtin_popcount(mnew), total_leaves = others + here;
    if (total_leaves != 0 && here == 0) logp = -INFINITY;                  // Move.fix_logp_gibbs (move.py:368-402), one branch under proposal
    if (total_leaves == 0 && here == 0) logp = 0.0;
    const double logl = mt_ll;
    const bool keep = accept_test(A.tempered, [&] { return beta; }, logl, logp, Lold, Pold, factors, log(u_acc));      // rj.py:330-332

    // ---- 6: update (Move.update, move.py:472-703) -----------------------------------------------------------------------------
    if (keep) {
        if (birth && lane < nd) row[offB + lf * nd + lane] = tr[j][lane];
        if (lane == 0) {
            row[M.ind_off + B] = (double)mnew;
            A.L[gw] = logl;
            A.P[gw] = stored_logp(logp);
            if (A.accepted) A.accepted[gw] += 1u;     // ("iterate_branches": the move's mask is its LAST branch's, rj.py:385-386)
        }
        if constexpr (HAVE_TM) {
            // the accepted template: base + the picked leaf (the same operations the try's likelihood was formed from), or the base
            RjLeaf f = rj_leaf_load(kindB, nd, tr[j]);
#pragma unroll
            for (int ch = 0; ch < MAXCH; ++ch)
#pragma unroll
                for (int k = 0; k < NPT; ++k) {
                    const int i = ch * 64 * NPT + k * 64 + lane;
                    if (i < M.ndata) {
                        double v = tmk[ch][k];
                        if (birth) v += 1.0 * rj_leaf_at(f, A.tdata[i], s_tab);
                        tmrow[i] = total_leaves > 0 ? v : 0.0;
                    }
                }
        }
    }
    if (lane == 0 && A.keep_out) A.keep_out[gw] = keep ? 1 : 0;
    RJ_MT_TRACE(5);
#undef RJ_MT_TRACE
#undef RJ_MT_LDS_SYNC
}

// hens_rj_mt_debug_draws: the tries and the pick uniform hens_rj_step draws per walker for `branch` in iteration `iter` (one thread per
// walker) - the functions k_rj_mt evaluates.  Coin, selector, accept uniform and the cascades' draws: hens_rj_debug_draws.
struct RjMtDebugArgs {
    double* tries;       // [Tl][W][K][ndmax] (zeros behind the branch's width); try 0 is what a BIRTH walker gets
    double* u_pick;      // [Tl][W]
    const double* gen;   // [nd][RJ_MT_DENS]
    uint64_t iter, seed;
    int32_t Tl, W, rung_begin, branch, K, nd, ndmax;
};
__global__ void k_rj_mt_debug_draws(const RjMtDebugArgs A) {
    const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= (int64_t)A.Tl * A.W) return;
    const int tl = (int)(gw / A.W);
    const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)A.W + (uint32_t)(gw - (int64_t)tl * A.W);
    for (int k = 0; k < A.K; ++k)
        for (int d = 0; d < A.ndmax; ++d) {
            double v = 0.0;
            if (d < A.nd) {
                const double* r = A.gen + d * RJ_MT_DENS;
                const u4 e = rj_philox(A.seed, A.iter, wid, k == 0 ? rj_birth_key(A.branch, d) : rj_try_key(A.branch, d, k));
                v = rj_birth_value(e, (int)r[5], r[0], r[1], r[2], r[3]);
            }
            A.tries[((size_t)gw * A.K + k) * A.ndmax + d] = v;
        }
    const u4 p = rj_philox(A.seed, A.iter, wid, rj_pick_key(A.branch));
    A.u_pick[gw] = u01(p.x, p.y);
}

}  // namespace hens
