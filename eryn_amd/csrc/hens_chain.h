// hens_chain.h - k_chain_store: one stored step of the chain store (include/hipensemble.h: hens_step_chain) appended to the chain
// buffers in device memory.  Replaces, on the device, Backend.save_step (backends/backend.py:1014-1091): the walkers of the stored
// rungs in WALKER order, their log-likelihood / log-prior, the ladder, and the accepted / swap totals the backend accumulates.
//
// A pure gather / scatter through memory, read where the state rides behind a hens_step call - nothing is unpacked, repacked or
// flipped (the three forms k_report_mask knows):
//   column-ordered records   record i of rung t belongs to walker slot rec.slot
//   slot-ordered records     ... to slot i
//   by-field arrays          L / P / loc by slot
// and the walker's row is the pool row its `loc` names NOW (k_iter's versioned rows: the accepted ones sit in the pool's other
// half until state_to_fields folds them back - the record knows).
//
// Shape: a row belongs to a group of LPR = 2^k >= D / VEC lanes (RW / 2 at the compile-time widths: 128 / RW rows per wave), lane
// j of the group moves the VEC doubles at j VEC, j VEC + LPR VEC, ...: the groups of a wave read consecutive records (one coalesced
// load, the same address within a group) and every destination row leaves as one contiguous burst of 16-byte stores.  The
// destination stride is the caller's D, not the padded row width: the inert pads are not stored, and no lane stores
// across a row's end.  VEC = 2 needs 16-byte aligned rows on both sides (row width and D even); else VEC = 1, chosen per launch.
// Nobody on the device reads the chain: its stores are nontemporal, the rung rows the XCD-affine numbering keeps in L2 between
// iterations should not make room for them.
//
// Totals (lane 0 of a group, whose slot is its alone): accepted[t][slot] += what the slot's accept counters - the stretch move's,
// riding in the record, and the Gaussian move's - gained since the mark in `prev` (hens_step_report's snapshot: k_report_mask),
// and `prev` moves up to now, so that back-to-back stored steps need no snapshot of their own.  Workgroup 0 copies the ladder and
// adds the last cascade's swap counts (settled by the host: flush_adapt in front of this launch).
#pragma once

namespace hens {

struct ChainArgs {
    const WalkerRec* wrec;                 // [Tl][W] records (state in record mode) or nullptr
    const double* L; const double* P;      // by-field state (wrec == nullptr)
    const int32_t* loc;
    const uint32_t* acc_fields;            // [Tl][W] stretch accept counters by slot (wrec == nullptr: they ride in the records else)
    const uint32_t* acc_mh;                // [Tl][W] Gaussian move's accept counters by slot, or nullptr
    uint32_t* prev; uint32_t* prev_mh;     // [Tl][W] the counters at the mark (hens_ctx_impl::report_prev)
    const double* pool;                    // [2 Tl W][RW]
    const double* betas;                   // [T] the ladder after the step's adaptation, or nullptr (not tempered)
    const double* swaps_last;              // [T-1] the last cascade's swap counts, or nullptr
    double* out_x;                         // [Ts][W][D]   this step's slice of the chain
    double* out_L; double* out_P;          // [Ts][W]
    double* out_betas;                     // [T]
    uint32_t* acc_tot;                     // [Ts][W]
    unsigned long long* swaps_tot;         // [T-1]
    int32_t colmode, T, W, Ts, RW, D, lpr_shift;
};

template <int VEC>
__global__ __launch_bounds__(256) void k_chain_store(const ChainArgs A) {
    if (blockIdx.x == 0) {
        for (int p = threadIdx.x; p < A.T; p += 256) {
            __builtin_nontemporal_store(A.betas ? A.betas[p] : 0.0, A.out_betas + p);
            if (A.swaps_last && p < A.T - 1) A.swaps_tot[p] += (unsigned long long)A.swaps_last[p];
        }
    }
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = g >> A.lpr_shift;                     // record
    const int lpr = 1 << A.lpr_shift, j = (int)(g & (lpr - 1));
    if (i >= (int64_t)A.Ts * A.W) return;
    int32_t loc;
    uint32_t a = 0;
    int64_t s = i;                                          // rung * W + slot
    if (A.wrec) {
        const int4 la = *reinterpret_cast<const int4*>(&A.wrec[i].loc);      // {loc, acc, slot, -}: the record's second 16 bytes
        loc = la.x;
        a = (uint32_t)la.y;
        if (A.colmode) s = (i / A.W) * A.W + la.z;
    } else {
        loc = A.loc[i];
        if (j == 0) a = A.acc_fields[i];
    }
    const double* src = A.pool + (int64_t)loc * A.RW;
    double* dst = A.out_x + s * A.D;
    for (int e = j * VEC; e + VEC <= A.D; e += lpr * VEC) {
        if constexpr (VEC == 2) {
            const dvec2 v = *reinterpret_cast<const dvec2*>(src + e);
            __builtin_nontemporal_store(v, reinterpret_cast<dvec2*>(dst + e));
        } else {
            __builtin_nontemporal_store(src[e], dst + e);
        }
    }
    if (j != 0) return;
    double Lv, Pv;
    if (A.wrec) {
        const dvec2 lp = *reinterpret_cast<const dvec2*>(&A.wrec[i].L);
        Lv = lp.x; Pv = lp.y;
    } else {
        Lv = A.L[i]; Pv = A.P[i];
    }
    __builtin_nontemporal_store(Lv, A.out_L + s);
    __builtin_nontemporal_store(Pv, A.out_P + s);
    uint32_t d = a - A.prev[s];
    A.prev[s] = a;
    if (A.acc_mh) {
        const uint32_t m = A.acc_mh[s];
        d += m - A.prev_mh[s];
        A.prev_mh[s] = m;
    }
    A.acc_tot[s] += d;
}

}  // namespace hens
