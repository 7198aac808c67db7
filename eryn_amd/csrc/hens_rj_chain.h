// hens_rj_chain.h - k_rj_chain_store: one stored step of a LEAF-PACKING context (include/hipensemble.h: hens_rj_step_chain) appended
// to the chain buffers in device memory - k_chain_store's twin for records of several branches and leaves.  Replaces, on the device,
// what a stored step of RJEnsembleSampler did on the host (hens_download_state + RJEngine.unpack(nan_fill=True) + a State): per branch
// the coordinates [nl][nd] of every walker of the stored rungs with the reference's NaN fill of unused leaves
// (backends/backend.py:1049-1059), the leaf masks as bytes, log-likelihood / log-prior, the ladder, and the accepted / rj_accepted /
// swap totals the reference's backend accumulates (backends/backend.py:1069-1091).
//
// The state between hens_rj_step iterations is by field: L / P / loc by slot, the walker's record the pool row its `loc` names - RW
// doubles [branch 0 coords | branch 1 coords | ... | one mask double per branch | pad], a mask an exact integer < 2^53 whose bit n says
// leaf slot n is in use.  The record is only read: a dead leaf keeps its coordinates on the device (distgenrj.py:120), the NaN is
// formed on the way out.  Neither the mask doubles nor the pad are stored.
//
// Shape (k_chain_store's): a record belongs to a group of LPR = 2^k lanes, 64 / LPR consecutive records per wave.  A branch's
// coordinates are contiguous in the record (from off[b]) and in the destination, so the group walks the branches - a uniform loop over
// the launch's own per-branch scalars (offset, leaves, width, destination: no table lookup, nothing dependent on a lane's index) - and
// lane j moves the VEC doubles at j VEC, j VEC + LPR VEC, ... of the branch's segment: every destination segment leaves as one
// contiguous burst, and no lane stores across a segment's end.  LPR covers the widest segment (at most a wave; wider: two rounds).
// VEC = 2 (16-byte lanes) where every segment is 16-byte aligned on both sides - every off[b] and every nl nd even (RW is even by
// construction) -, else VEC = 1: 3 leaves x 3 parameters = 9 is common.  The leaf of a coordinate is e / nd with nd in 1 .. 4.
// Nobody on the device reads the chain: its stores are nontemporal.
//
// Totals (lane 0 of a group, whose slot is its alone): accepted[t][slot] / rj_accepted[t][slot] += what the in-model accept counter
// and the birth / death accept counter gained since the mark in `prev` / `prev_bd`, and the marks move up to now.  Workgroup 0
// copies the ladder and adds the step's in-model swap counts (set aside by the host behind the last iteration's first cascade).
#pragma once

namespace hens {

struct RjChainArgs {
    const double* pool;                    // [2 Tl W][RW]
    const int32_t* loc;                    // [Tl][W] by slot
    const double* L; const double* P;      // [Tl][W]
    const uint32_t* acc; const uint32_t* acc_bd;       // [Tl][W] in-model / birth-death accept counters
    uint32_t* prev; uint32_t* prev_bd;     // [Tl][W] the counters at the mark
    const double* betas;                   // [T] the ladder after the step's adaptation, or nullptr (not tempered)
    const double* swaps;                   // [T-1] the in-model cascade's swap counts of the step's last iteration, or nullptr
    double* out_x[RJ_MAX_BRANCH];          // [Ts][W][nl_b][nd_b]  this step's slice of branch b's chain
    uint8_t* out_inds[RJ_MAX_BRANCH];      // [Ts][W][nl_b]
    double* out_L; double* out_P;          // [Ts][W]
    double* out_betas;                     // [T]
    uint32_t* acc_tot; uint32_t* bd_tot;   // [Ts][W]
    unsigned long long* swaps_tot;         // [T-1]
    int32_t off[RJ_MAX_BRANCH], nl[RJ_MAX_BRANCH], nd[RJ_MAX_BRANCH];
    int32_t nb, ind_off, T, W, Ts, RW, lpr_shift;
};

// leaf slot of coordinate e of a branch whose leaves have nd parameters (e < 128: 43 e >> 7 = e / 3)
__device__ __forceinline__ int rj_chain_leaf(int e, int nd) {
    return nd == 1 ? e : nd == 2 ? e >> 1 : nd == 3 ? (e * 43) >> 7 : nd == 4 ? e >> 2 : e / nd;
}

template <int VEC>
__global__ __launch_bounds__(256) void k_rj_chain_store(const RjChainArgs A) {
    if (blockIdx.x == 0) {
        for (int p = threadIdx.x; p < A.T; p += 256) {
            __builtin_nontemporal_store(A.betas ? A.betas[p] : 0.0, A.out_betas + p);
            if (A.swaps && p < A.T - 1) A.swaps_tot[p] += (unsigned long long)A.swaps[p];
        }
    }
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t s = g >> A.lpr_shift;                     // rung * W + slot
    const int lpr = 1 << A.lpr_shift, j = (int)(g & (lpr - 1));
    if (s >= (int64_t)A.Ts * A.W) return;
    const double* src = A.pool + (int64_t)A.loc[s] * A.RW;
    const double qnan = __builtin_nan("");
    for (int b = 0; b < A.nb; ++b) {
        const int nd = A.nd[b], nl = A.nl[b], seg = nl * nd;
        const unsigned long long m = (unsigned long long)src[A.ind_off + b];
        const double* sb = src + A.off[b];
        double* db = A.out_x[b] + s * seg;
        for (int e = j * VEC; e + VEC <= seg; e += lpr * VEC) {
            if constexpr (VEC == 2) {
                dvec2 v = *reinterpret_cast<const dvec2*>(sb + e);
                if (!((m >> rj_chain_leaf(e, nd)) & 1ull)) v.x = qnan;
                if (!((m >> rj_chain_leaf(e + 1, nd)) & 1ull)) v.y = qnan;
                __builtin_nontemporal_store(v, reinterpret_cast<dvec2*>(db + e));
            } else {
                const double v = ((m >> rj_chain_leaf(e, nd)) & 1ull) ? sb[e] : qnan;
                __builtin_nontemporal_store(v, db + e);
            }
        }
        uint8_t* ib = A.out_inds[b] + s * nl;
        for (int n = j; n < nl; n += lpr) __builtin_nontemporal_store((uint8_t)((m >> n) & 1ull), ib + n);
    }
    if (j != 0) return;
    __builtin_nontemporal_store(A.L[s], A.out_L + s);
    __builtin_nontemporal_store(A.P[s], A.out_P + s);
    const uint32_t a = A.acc[s], d = A.acc_bd[s];
    A.acc_tot[s] += a - A.prev[s];
    A.prev[s] = a;
    A.bd_tot[s] += d - A.prev_bd[s];
    A.prev_bd[s] = d;
}

}  // namespace hens
