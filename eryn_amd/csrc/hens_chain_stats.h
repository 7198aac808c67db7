// hens_chain_stats.h - k_chain_moments, k_chain_act: the chain diagnostics (include/hipensemble.h: hens_chain_moments,
// hens_chain_act) as streaming reductions over the step axis of the chain buffers k_chain_store fills (csrc/hens_chain.h).  On the
// device they replace the reductions under the reference's get_autocorr_time / get_gelman_rubin_convergence_diagnostic /
// get_evidence_estimate (backends/backend.py:616-817 on utils/utility.py:43-144, 279-330); the arithmetic and its ORDER are those
// of eryn_amd/chain_stats.py, bit for bit (no fused multiply-add: -ffp-contract=off; division and subtraction are IEEE).
//
// A series is one (rung, walker, coordinate) - or (rung, walker) of logl / logp - over the kept steps.  The stored rungs [0, ntemps)
// are the head of every step's slice, so series i of the selection sits at offset i of the slice and the kept steps are `stride`
// doubles apart (thin x the step's size: hens_chain_host.h: stat_plan).  Lane = series: the lanes of a wave read consecutive
// doubles of one step, one coalesced burst per step, and walk the steps in order with STAT_U loads in flight.  Plain loads: the
// chain is read twice in a row (sum, then the centred pass) and a few steps of the selection fit in L2.  Nobody reads the outputs
// on the device.
//
// k_chain_moments<VEC, MASK>: VEC = 2 where the selection's size and the step's are even - a lane owns two adjacent series and
//   loads 16 bytes -, else 1; chosen per launch as k_chain_store's.  MASK (logl / logp): non-finite entries are skipped and counted.
// k_chain_act<KMAX>: one series per lane, a workgroup is ONE wave.  Pass two keeps each lane's last K centred values in an LDS ring
//   laid out [K][64] - lag k's read is 64 consecutive doubles: conflict-free, two LDS cycles per wave (ds_read_b64) - and the K
//   accumulators in registers (KMAX = 16 / 32 / 64 of them, the lags [K, KMAX) predicated off by a wave-uniform compare).  Every
//   new sample y_j adds y_j y_{j-k} into lag k's accumulator: c_k's products in ascending j.  A lane reads only its own column, a
//   wave's LDS operations are in order: no barrier.  Two series per lane would double the ring per lane and halve the waves a
//   CU's LDS holds, and the LDS reads, not the chain's loads, bound this kernel: VEC = 1 always.  Tail lanes of the last wave walk
//   series 0 and store nothing.
#pragma once

namespace hens {

constexpr int STAT_U = 8;          // chain loads in flight per lane
constexpr int ACT_LANES = 64;      // (hens_chain_host.h: ACT_LANES)

struct ChainStatArgs {
    const double* src;             // the first kept step's slice of the field
    int64_t stride;                // doubles between kept steps
    int64_t count;                 // kept steps
    int64_t nseries;               // series selected: ntemps x W x D, or ntemps x W
    double* sum; double* m2; long long* nfin;      // k_chain_moments' outputs [nseries], any may be nullptr
    double* tau; double* mean; double* c0;         // k_chain_act's
    int32_t K;                     // lags 0 .. K-1 enter tau: min(window, count)
};

template <int VEC>
__device__ __forceinline__ void stat_load(const double* q, double (&v)[VEC]) {
    if constexpr (VEC == 2) {
        const dvec2 t = *reinterpret_cast<const dvec2*>(q);
        v[0] = t.x; v[1] = t.y;
    } else {
        v[0] = *q;
    }
}

// f(v) for every kept step in order, STAT_U loads issued before the first of them is used
template <int VEC, class F>
__device__ __forceinline__ void stat_walk(const double* p, int64_t stride, int64_t count, F&& f) {
    int64_t j = 0;
    for (; j + STAT_U <= count; j += STAT_U) {
        double v[STAT_U][VEC];
#pragma unroll
        for (int u = 0; u < STAT_U; ++u) stat_load<VEC>(p + (j + u) * stride, v[u]);
#pragma unroll
        for (int u = 0; u < STAT_U; ++u) f(v[u]);
    }
    for (; j < count; ++j) {
        double v[VEC];
        stat_load<VEC>(p + j * stride, v);
        f(v);
    }
}

__device__ __forceinline__ bool stat_finite(double v) { return __builtin_fabs(v) < __builtin_inf(); }   // (false for NaN)

template <int VEC, bool MASK>
__global__ __launch_bounds__(256) void k_chain_moments(const ChainStatArgs A) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * VEC;
    if (i >= A.nseries) return;                       // (VEC = 2: nseries is even, i + 1 is inside)
    const double* p = A.src + i;
    double s[VEC], q[VEC], mean[VEC];
    long long nf[VEC];
#pragma unroll
    for (int e = 0; e < VEC; ++e) { s[e] = 0.0; q[e] = 0.0; nf[e] = MASK ? 0 : (long long)A.count; }
    stat_walk<VEC>(p, A.stride, A.count, [&](const double (&v)[VEC]) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            if constexpr (MASK) {
                if (stat_finite(v[e])) { s[e] += v[e]; nf[e] += 1; }
            } else {
                s[e] += v[e];
            }
        }
    });
#pragma unroll
    for (int e = 0; e < VEC; ++e) mean[e] = s[e] / (double)nf[e];
    if (A.m2)
        stat_walk<VEC>(p, A.stride, A.count, [&](const double (&v)[VEC]) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const double y = v[e] - mean[e];
                if (!MASK || stat_finite(v[e])) q[e] += y * y;
            }
        });
#pragma unroll
    for (int e = 0; e < VEC; ++e) {
        if (A.sum) A.sum[i + e] = s[e];
        if (A.m2) A.m2[i + e] = q[e];
        if (A.nfin) A.nfin[i + e] = nf[e];
    }
}

template <int KMAX>
__global__ __launch_bounds__(ACT_LANES) void k_chain_act(const ChainStatArgs A) {
    extern __shared__ double act_ring[];              // [K][ACT_LANES]
    const int lane = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * ACT_LANES + lane;
    const bool live = i < A.nseries;
    const double* p = A.src + (live ? i : 0);
    const int K = A.K;
    double s = 0.0;
    stat_walk<1>(p, A.stride, A.count, [&](const double (&v)[1]) { s += v[0]; });
    const double mean = s / (double)A.count;
    double c[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) c[k] = 0.0;
    int h = 0;                                        // the ring row of the sample at hand
    int64_t j = 0;
    stat_walk<1>(p, A.stride, A.count, [&](const double (&v)[1]) {
        const double y = v[0] - mean;
        act_ring[h * ACT_LANES + lane] = y;
        const int top = (int)(j < (int64_t)(K - 1) ? j : (int64_t)(K - 1));      // lags 0 .. top have a partner
        c[0] += y * y;
#pragma unroll
        for (int k = 1; k < KMAX; ++k) {
            if (k <= top) {
                const int row = h - k < 0 ? h - k + K : h - k;
                c[k] += y * act_ring[row * ACT_LANES + lane];
            }
        }
        h = h + 1 == K ? 0 : h + 1;
        ++j;
    });
    double r = 0.0;
#pragma unroll
    for (int k = 1; k < KMAX; ++k)
        if (k < K) r += c[k] / c[0];
    if (!live) return;
    if (A.tau) A.tau[i] = 1.0 + 2.0 * r;
    if (A.mean) A.mean[i] = mean;
    if (A.c0) A.c0[i] = c[0];
}

}  // namespace hens
