// hens_ladder_fold.inc - the folded ladder adaptation of one wavefront (tempering.py:563-596), T <= 128: lane l owns rungs l and l + 64.
// ONE text for k_stretch_fast (hens_kernels.h) and k_stretch2 (hens_tile2.h), included into the kernel's body section by section:
//   #define HENS_LF_SECTION n
//   #include "hens_ladder_fold.inc"
// The sections define lambdas and locals over the kernel's own names - A, lane, wv, PIPE, ADW, s_part, s_beta, the flags ad_lead /
// ad_early / ad_defer / ad_x, cnt_wait, inject_until (k_stretch_fast's latency-injection hook of dev builds; constexpr 0 elsewhere) -
// so both kernels compile the tokens they compiled when each carried a copy.  The kernels decide the flags and where the pieces run.
//   1  the state that crosses the first barrier in registers (ad_c0 ... ad_inv0); adapt_part1 (ratios, dS, exp, deltaT: ~2500 cycles
//      of dependent FP64 divides that need the counts but not the cumulative sum - a wave runs it while it would otherwise idle before
//      the first barrier); adapt_part2 (cumsum, reciprocals, update, the ring of a pipeline rank, workgroup (0,0)'s books: in the
//      shadow of the row gathers)
//   2  ad_u0 / ad_u1 / ad_bi0 / ad_bi1, ad_defer_all, ADX, the ADX wave (count rows -> exp(dS) into s_exp, its books and clears),
//      adapt_early, and the LDS aliases s_exp / s_late / s_lateb on s_part (nobody touches it before the likelihood phase; the two
//      `* const`: without it k_stretch2<PIPE> compiles to other code, profiles/ladder_fold_ab.txt)
//   3  pipe_chain: the chain of a pipeline rank's adapting wave, with its late wait
//   4  that wave's first look (loads only), the body of `if (ad_early && ad_lead && wv == ADW)`
//   5  the ADW wave where every workgroup adapts for itself: loads, wait, first part (and the second unless deferred)
// (k_stretch2 never takes the `two` branches - column-ordered records need T * label_cb == 128, a ladder of at most 64 rungs; ladders
//  of 65 to 128 rungs take them in k_stretch_fast's copying launches: tests/test_hip_ladders.py long_T65 ... T130.)
#if HENS_LF_SECTION == 1
    double ad_c0 = 0.0, ad_c1 = 0.0, ad_dT0 = 0.0, ad_dT1 = 0.0, ad_b0n = 1.0, ad_b1n = 1.0, ad_bb0 = 1.0, ad_bb1 = 1.0, ad_inv0 = 1.0;
    auto adapt_part1 = [&](const double cnt0, const double cnt1, const double ad_b, const double ad_b1, const bool exp_elsewhere = false) {
        const int T = A.ad.T;
        const int e0 = lane, e1 = lane + 64;
        ad_c0 = cnt0; ad_c1 = cnt1; ad_bb0 = ad_b; ad_bb1 = ad_b1;
        if (!A.ad.moving) return;
        if (exp_elsewhere) {                 // (T <= 64) the ratio chain - cnt / W, dS, exp - runs on wave ADX; here: 1 / beta differences
            const double inv0v = 1.0 / ad_b;
            ad_inv0 = inv0v;
            ad_b0n = __shfl_down(ad_b, 1);
            const double inv0n = __shfl_down(inv0v, 1);
            ad_dT0 = (e0 + 2 < T) ? inv0n - inv0v : 0.0;                           // :578; times exp(dS) after the barrier
            ad_dT1 = 0.0;
            return;
        }
        const bool two = T > 64;                                                   // wave-uniform: rungs 64.. exist
        const double r0 = cnt0 / (double)A.ad.W, r1 = two ? cnt1 / (double)A.ad.W : 0.0;   // :587
        const double kappa = A.ad.kappa;                                           // :571-572 (host)
        // ONE reciprocal per rung: 1 / beta of the next rung is the next lane's (round 3: the chain had 1 / b twice per lane, and
        // 1 / b[0] once more in the second part - on the path of every launch since the first barrier comes earlier)
        const double inv0v = 1.0 / ad_b, inv1v = two ? 1.0 / ad_b1 : 1.0;
        ad_inv0 = inv0v;
        // the value of the NEXT rung (e + 1): lane 63's successor is rung 64 = lane 0's second element
        // (lane exchanges are LDS crossbar trips: the second rung set's only for ladders above 64 rungs - wave-uniform)
        const double r0d = __shfl_down(r0, 1), b0d = __shfl_down(ad_b, 1), i0d = __shfl_down(inv0v, 1);
        double r0n = r0d, b0n = b0d, inv0n = i0d, r1n = 0.0, b1n = 1.0, inv1n = 1.0;
        if (two) {
            const double r1first = __shfl(r1, 0), b1first = __shfl(ad_b1, 0), i1first = __shfl(inv1v, 0);
            if (lane == 63) { r0n = r1first; b0n = b1first; inv0n = i1first; }
            r1n = __shfl_down(r1, 1); b1n = __shfl_down(ad_b1, 1); inv1n = __shfl_down(inv1v, 1);
        }
        ad_b0n = b0n; ad_b1n = b1n;
        double dT0 = 0.0, dT1 = 0.0;
        if (e0 + 2 < T) {
            const double dS = kappa * (r0 - r0n);                                  // :575
            dT0 = inv0n - inv0v;                                                   // :578  1 / b[e+1] - 1 / b[e]
            dT0 *= exp(dS);
        }
        if (two && e1 + 2 < T) {
            const double dS = kappa * (r1 - r1n);
            dT1 = inv1n - inv1v;
            dT1 *= exp(dS);
        }
        ad_dT0 = dT0; ad_dT1 = dT1;
    };
    auto adapt_part2 = [&]() {
        const int T = A.ad.T;
        const int e0 = lane, e1 = lane + 64;
        const double cnt0 = ad_c0, cnt1 = ad_c1, ad_b = ad_bb0, ad_b1 = ad_bb1;
        double bnew0 = ad_b, bnew1 = ad_b1;
        if (A.ad.moving) {
            const double dT0 = ad_dT0, dT1 = ad_dT1, b0n = ad_b0n, b1n = ad_b1n;
            double cs0 = 0.0, cs1 = 0.0;                                           // np.cumsum: left-to-right
            for (int i = 0; i + 2 < T; ++i) {
                const double v = i < 64 ? readlane_f64(dT0, i) : readlane_f64(dT1, i - 64);
                if (i == 0) { cs0 = v; cs1 = v; }
                else {
                    if (i <= e0) cs0 = cs0 + v;
                    if (i <= e1) cs1 = cs1 + v;
                }
            }
            const double inv0 = readlane_f64(ad_inv0, 0);                          // 1 / b[0]
            const double bn0 = 1.0 / (cs0 + inv0), bn1 = T > 64 ? 1.0 / (cs1 + inv0) : 0.0;   // :580, belong to rungs e + 1
            const double upd0 = b0n + (bn0 - b0n), upd1 = b1n + (bn1 - b1n);      // :583,:593
            const double up0 = __shfl_up(upd0, 1);
            if (e0 >= 1 && e0 + 1 < T) bnew0 = up0;
            if (T > 64) {                                                          // (wave-uniform: the second rung set)
                const double up1 = __shfl_up(upd1, 1), upd0last = readlane_f64(upd0, 63);
                if (e1 + 1 < T) bnew1 = lane >= 1 ? up1 : upd0last;
            }
        }
        if (e0 < T) s_beta[e0] = bnew0;
        if (e1 < T) s_beta[e1] = bnew1;
        if (ad_lead) {       // publish: agent-scope stores (other XCDs read them with agent-scope loads); retire the slot after next
            double* slot = A.ad_ring + (size_t)(A.ad_serial & 3u) * T;
            double* clear = A.ad_ring + (size_t)((A.ad_serial + 2u) & 3u) * T;
            if (e0 < T) {
                __hip_atomic_store(clear + e0, -1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(slot + e0, bnew0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            if (e1 < T) {
                __hip_atomic_store(clear + e1, -1.0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(slot + e1, bnew1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
        if (blockIdx.x == 0 && blockIdx.y == 0) {
            // (workgroup (0,0)'s books: the three pointers are read from the kernarg segment HERE on one GPU - as by-value arguments
            //  they sit in SGPRs from the entry of every workgroup's every wave, late_kernarg)
            constexpr size_t AD = offsetof(StretchArgs, ad);
            double* const betas_out_l = PIPE ? A.ad.betas_out : late_kernarg<double*>(AD + offsetof(AdaptArgs, betas_out));
            double* const swaps_last_l = PIPE ? A.ad.swaps_last : late_kernarg<double*>(AD + offsetof(AdaptArgs, swaps_last));
            double* const swaps_total_l = PIPE ? A.ad.swaps_total : late_kernarg<double*>(AD + offsetof(AdaptArgs, swaps_total));
            if (e0 < T) wt_store(&betas_out_l[e0], bnew0);
            if (e1 < T) wt_store(&betas_out_l[e1], bnew1);
            if (e0 < T - 1 && !ad_x) {             // (ad_x: wave ADX, the only reader of the counts then, keeps these books)
                wt_store(&swaps_last_l[e0], cnt0);
                // (a pipeline rank: an atomic without a return value - `+=` is a load this wave, in front of workgroup (0,0)'s first
                //  barrier there, waits a memory round trip for: the rank's first launch 9.4 -> 8.8 us at 16 x 4096 x 32; the counts are
                //  integers, the sum is the same double.  One GPU keeps `+=`: in the gathers' shadow it costs nothing, and the atomic made
                //  config 2 0.1 us SLOWER - 17.40 -> 17.50, four alternations)
                if constexpr (PIPE) atomicAdd(&swaps_total_l[e0], cnt0);
                else wt_store(&swaps_total_l[e0], swaps_total_l[e0] + cnt0);
            }
            if (e1 < T - 1) {
                wt_store(&swaps_last_l[e1], cnt1);
                if constexpr (PIPE) atomicAdd(&swaps_total_l[e1], cnt1);
                else wt_store(&swaps_total_l[e1], swaps_total_l[e1] + cnt1);
            }
        }
    };
#elif HENS_LF_SECTION == 2
    unsigned ad_u0[8], ad_u1[8];
    double ad_bi0 = 1.0, ad_bi1 = 1.0;
    // (column-ordered records, measured at config 2 in workgroup cycles up to the second barrier: both parts in front of the
    //  first barrier 13 070, both in the gathers' shadow 11 520, the split as it is 9 900)
    constexpr bool ad_defer_all = false;
    // Round 3: the first part was the last to reach the first barrier (4 460 cycles after the workgroup's start; the complement
    // rows' wave 2 830, the rest < 2 000): its two independent chains run on two waves - ratios -> dS -> exp on wave ADX,
    // reciprocals of the ladder on wave ADW - and meet through LDS after the barrier (ladders of up to 64 rungs).
    constexpr int ADX = 3;
    double* s_exp = s_part;                  // [64] exp(dS) per rung (phase C overwrites it after the second barrier)
    if (ad_x && wv == ADX) {
        const int T = A.ad.T, NR = A.ad.nblocks;
        const int G = A.ad.row_groups, P2 = 64 / G, p = lane & (P2 - 1), g = lane / P2;
        unsigned u[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) u[r] = (r * G + g < NR && p < T - 1) ? A.ad.swap_part[(size_t)(r * G + g) * (T - 1) + p] : 0u;
        __builtin_amdgcn_s_waitcnt(0x0F70);
        unsigned s0 = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) s0 += u[r];
        for (int m = P2; m < 64; m <<= 1) s0 += __shfl_xor(s0, m);
        const double r0 = (double)s0 / (double)A.ad.W;                             // :587
        const double r0n = __shfl_down(r0, 1);
        s_exp[lane] = (lane + 2 < T) ? exp(A.ad.kappa * (r0 - r0n)) : 1.0;        // :575
        // This wave is the ONLY reader of the count rows (the reciprocal chain on wave ADW needs none of them: every workgroup
        // reading the same 15 cache lines twice made those loads ~3 000 cycles long and wave ADW the last at the first
        // barrier, 4 150 cycles after the start against the complement wave's 3 000), so workgroup (0,0)'s books are kept here.
        if (blockIdx.x == 0 && blockIdx.y == 0) {
            if (g == 0 && p < T - 1) {
                constexpr size_t AD = offsetof(StretchArgs, ad);
                wt_store(&late_kernarg<double*>(AD + offsetof(AdaptArgs, swaps_last))[p], (double)s0);
                double* const tot = late_kernarg<double*>(AD + offsetof(AdaptArgs, swaps_total));
                wt_store(&tot[p], tot[p] + (double)s0);
            }
            if (A.ad.zero_after) {
#pragma unroll
                for (int r = 0; r < 8; ++r)
                    if (r * G + g < NR && p < T - 1 && u[r]) wt_store(&A.ad.swap_part[(size_t)(r * G + g) * (T - 1) + p], 0u);
            }
            if (A.ad.zero_rows)
                for (int e = lane; e < NR * (T - 1); e += 64) wt_store(&A.ad.zero_rows[e], 0u);
        }
    }
    auto adapt_early = [&]() {
        const int T = A.ad.T, NR = A.ad.nblocks;
        unsigned s0 = 0, s1 = 0;
#pragma unroll
        for (int r = 0; r < 8; ++r) { s0 += ad_u0[r]; s1 += ad_u1[r]; }
        const int G = A.ad.row_groups, P2 = 64 / G;
        for (int m = P2; m < 64; m <<= 1) s0 += __shfl_xor(s0, m);       // (the lane groups' partial sums)
        if (blockIdx.x == 0 && blockIdx.y == 0 && !ad_x) {
            if (A.ad.zero_after) {                   // sole reader (mode 2 / a pipeline rank): clear what was read
                const int p = lane & (P2 - 1), g = lane / P2;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    if (r * G + g < NR && p < T - 1 && ad_u0[r]) wt_store(&A.ad.swap_part[(size_t)(r * G + g) * (T - 1) + p], 0u);
                    if (r < NR && lane + 64 < T - 1 && ad_u1[r]) wt_store(&A.ad.swap_part[(size_t)r * (T - 1) + lane + 64], 0u);
                }
            }
            if (A.ad.zero_rows)                      // every workgroup reads the rows: clear the buffer of the NEXT sweep
                for (int e = lane; e < NR * (T - 1); e += 64) wt_store(&A.ad.zero_rows[e], 0u);
        }
        adapt_part1((double)s0, (double)s1, ad_bi0, ad_bi1, ad_x);
    };
    unsigned* const s_late = reinterpret_cast<unsigned*>(s_part);      // [l] late, [64 + l] own sums, [128 + l] / [192 + l] counts of rungs l / l + 64
    double* const s_lateb = s_part + 128;                              // [l] / [64 + l] the ladder
#elif HENS_LF_SECTION == 3
    auto pipe_chain = [&]() {
        const int T = A.ad.T, rb = A.rung_begin, np = A.cp_np;
        const bool own_acc = A.cnt_push == 2;
        unsigned m0 = s_late[128 + lane], m1 = s_late[192 + lane];
        const unsigned own = s_late[64 + lane];
        const double b0 = s_lateb[lane], b1 = s_lateb[64 + lane];
        if (s_late[lane] != 0u) {
            // a rank's counts were not there at the first look: wait for them now (the polls queue up behind this wave's own
            // gathers - loads return in order - so the chain overlaps the OTHER waves' gathers only)
            if (lane >= PF_CNT0 && lane != PF_CNT0 + A.cp_rank && ((A.wmask >> lane) & 1ull))
                pipe_spin(A.wflags + lane, A.wtarget_cnt, A.wbudget, A.flags, A.wstats ? A.wstats + 2 : nullptr, inject_until);
#ifdef HENS_DEV_BUILD
            if (inject_until)                    // (a lone rank has no flag to wait for: the injected delay alone)
                while ((long long)(__builtin_amdgcn_s_memtime() - inject_until) < 0) __builtin_amdgcn_s_sleep(2);
#endif
            if (!(own_acc && A.cp_nranks == 1)) {
                if (lane < T - 1) m0 = A.ad.swap_part[lane];
                if (lane + 64 < T - 1) m1 = A.ad.swap_part[lane + 64];
            }
        }
        if (own_acc) {                           // my pairs out of my own sums: global pair e = rung_begin + local pair
            const int j0 = lane - rb, j1 = lane + 64 - rb;
            const unsigned o0 = (unsigned)__shfl((int)own, (j0 >= 0 && j0 < np) ? j0 : 0);
            const unsigned o1 = (unsigned)__shfl((int)own, (j1 >= 0 && j1 < np) ? j1 : 0);
            if (j0 >= 0 && j0 < np) m0 = o0;
            if (j1 >= 0 && j1 < np) m1 = o1;
        }
        adapt_part1((double)m0, (double)m1, b0, b1);
        adapt_part2();
    };
#elif HENS_LF_SECTION == 4
            const int T = A.ad.T;
            // (one round trip: ladder and flags are requested first, the accumulation rows last - loads return in order, the wait for
            //  the rows' sum covers all of them)
            const double b0 = (lane < T) ? A.ad.betas_in[lane] : 1.0, b1 = (lane + 64 < T) ? A.ad.betas_in[lane + 64] : 1.0;
            uint32_t fl = 0xFFFFFFFFu;
            if (cnt_wait && lane >= PF_CNT0 && lane != PF_CNT0 + A.cp_rank && ((A.wmask >> lane) & 1ull))
                fl = __hip_atomic_load(A.wflags + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            unsigned own = 0;                        // lane p: this rank's count of local pair p (cnt_push == 2)
            if (A.cnt_push == 2) own = acc_rows_sum(A.cp_rows, A.cp_nblocks, A.cp_np, lane);
            bool late = false;
            if (cnt_wait) {
                bool here = fl >= A.wtarget_cnt;
#ifdef HENS_DEV_BUILD
                if (inject_until && (long long)(__builtin_amdgcn_s_memtime() - inject_until) < 0) here = false;
#endif
                late = __ballot(!here) != 0ull;
                if (A.inject_c64 < 0) late = true;       // (HENS_PIPE_FORCE_LATE=1, tests: every adaptation takes the late path)
                __atomic_signal_fence(__ATOMIC_SEQ_CST);          // (acquire side: see pipe_spin)
            }
            unsigned m0 = 0, m1 = 0;                 // (row_groups = 1: the mailbox's reduced counts, one row)
            if (!late && !(A.cnt_push == 2 && A.cp_nranks == 1)) {
                if (lane < T - 1) m0 = A.ad.swap_part[lane];
                if (lane + 64 < T - 1) m1 = A.ad.swap_part[lane + 64];
            }
            s_late[lane] = late ? 1u : 0u;           // (every lane its own word: a value one lane stores for the others needs a barrier -
                                                     //  without one the compiler may read before the store, and did)
            s_late[64 + lane] = own; s_late[128 + lane] = m0; s_late[192 + lane] = m1;
            s_lateb[lane] = b0; s_lateb[64 + lane] = b1;
#elif HENS_LF_SECTION == 5
    if (ad_early && wv == ADW && !(PIPE && ad_lead)) {
        const int T = A.ad.T, NR = A.ad.nblocks;
        // (row_groups G > 1 - ladders of at most 64 / G pairs: lane = (group g, pair p), group g sums rows g, g + G, ...)
        const int G = A.ad.row_groups, P2 = 64 / G, p = lane & (P2 - 1), g = lane / P2;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            ad_u0[r] = (!ad_x && r * G + g < NR && p < T - 1) ? A.ad.swap_part[(size_t)(r * G + g) * (T - 1) + p] : 0u;
            ad_u1[r] = (!ad_x && r < NR && lane + 64 < T - 1) ? A.ad.swap_part[(size_t)r * (T - 1) + lane + 64] : 0u;
        }
        if (lane < T) ad_bi0 = A.ad.betas_in[lane];
        if (lane + 64 < T) ad_bi1 = A.ad.betas_in[lane + 64];
        // Wait for these loads HERE (the wave has nothing else to do before the first barrier), with the builtin the
        // compiler's wait-count pass understands: otherwise it guards the deferred computation with a wait that also
        // covers the row gathers issued in between, and the adaptation no longer overlaps them.
        __builtin_amdgcn_s_waitcnt(0x0F70);      // vmcnt(0), expcnt / lgkmcnt untouched
        // first part now: this wave has nothing else to do before the barrier - unless the barrier comes early (column-ordered
        // records: phase A is one coalesced load), then everything waits for the shadow of the row gathers
        if (!ad_defer_all) adapt_early();
        if (!ad_defer) adapt_part2();
    }
#endif
#undef HENS_LF_SECTION
