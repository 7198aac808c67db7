// hens_rj_chain_stats.h - k_rj_chain_leaves, k_rj_chain_leaf_moments: the diagnostics of a LEAF-PACKING context's chain
// (include/hipensemble.h: hens_rj_chain_leaves, hens_rj_chain_leaf_moments) as streaming reductions over the step axis of the buffers
// k_rj_chain_store fills (csrc/hens_rj_chain.h): per branch x[step][Ts][W][nl][nd] with NaN on unused leaves and the leaf masks
// inds[step][Ts][W][nl] as bytes.  On the device they replace the reductions under the reference's get_nleaves and the projection
// through the leaf masks of its get_gelman_rubin_convergence_diagnostic (backends/backend.py:410-434, 786-799); the arithmetic and its
// ORDER are those of eryn_amd/chain_stats.py (leaf_counts, leaf_moments), bit for bit (-ffp-contract=off).
//
// A PLACE is one (rung, walker) of the selection.  The stored rungs [0, ntemps) are the head of a step's slice: place i's nl mask
// bytes sit at byte i nl of the step's mask slice, its coordinates at double i nl nd of the step's coordinate slice; kept steps are
// `stride` apart (hens_chain_host.h: rj_stat_plan).  Plain loads: the chain is read more than once.  No cross-workgroup atomic, and
// nobody reads the outputs on the device.
//
// k_rj_chain_leaves<VEC>: lane = place.  A wave reads 64 nl contiguous mask bytes per kept step - as bytes (VEC = 1), or as dwords
//   where nl is a multiple of 4 (VEC = 4: every place then starts on a dword) - and counts them.  The histogram is an LDS table
//   [nl + 1][256] of u32: a lane increments its own column (bank = lane: conflict-free, a plain read-modify-write, no atomic, no
//   barrier) and writes it out at the end.  The count goes out as one byte per place and kept step (coalesced) where asked for.
// k_rj_chain_leaf_moments: lane = series (place, parameter): a branch has few parameters per leaf (1 to 4), so lane-per-place would
//   leave a third of the lanes of a device-filling launch at the flagship shape; the nd lanes of a place read the same mask bytes
//   (one cache line) and adjacent doubles of a leaf.  A lane walks the kept steps in order, builds the step's mask from the place's
//   bytes - the masks of STAT_U steps before the first coordinate of the batch is asked for - and adds, for every set bit in
//   ascending slot whose ordinal among the place's leaves in use lies in [lo, hi), the leaf's coordinate: first the sum, then m2
//   about sum / n in a second walk.  Steps wholly below `lo` are skipped by their popcount, and a series stops once its ordinal
//   reaches `hi`.
#pragma once

namespace hens {

constexpr int RJ_STAT_LANES = 256;     // (hens_chain_host.h: RJ_STAT_LANES sizes the LDS table)

struct RjStatArgs {
    const uint8_t* inds;           // the first kept step's mask slice of the branch
    const double* x;               // ... and its coordinate slice (k_rj_chain_leaf_moments)
    int64_t inds_stride;           // bytes between kept steps
    int64_t x_stride;              // doubles between kept steps
    int64_t count;                 // kept steps
    int64_t nplaces;               // ntemps x W
    int64_t lo, hi;                // the ordinal window (k_rj_chain_leaf_moments)
    int32_t nl, nd;
    uint8_t* nleaves;              // [count][nplaces], or nullptr
    uint32_t* hist;                // [nplaces][nl + 1]
    double* sum; double* m2;       // [nplaces][nd]; m2 may be nullptr (one walk)
    long long* n;                  // [nplaces]
};

// the leaf mask of one place at one step: bit n = byte n (0 / 1) of its nl <= 32 bytes
template <int VEC>
__device__ __forceinline__ uint32_t rj_stat_mask(const uint8_t* p, int nl) {
    uint32_t m = 0;
    if constexpr (VEC == 4) {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
        for (int g = 0; g < nl / 4; ++g) {
            const uint32_t w = q[g] & 0x01010101u;                     // bytes b0 b1 b2 b3 -> bits 0, 8, 16, 24
            m |= (((w * 0x10204080u) >> 28) & 0xFu) << (4 * g);        // ... gathered into bits 28 .. 31 (no two products collide)
        }
    } else {
        for (int n = 0; n < nl; ++n) m |= (uint32_t)(p[n] & 1u) << n;
    }
    return m;
}

template <int VEC>
__global__ __launch_bounds__(RJ_STAT_LANES) void k_rj_chain_leaves(const RjStatArgs A) {
    extern __shared__ uint32_t leaf_tab[];            // [nl + 1][RJ_STAT_LANES]
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * RJ_STAT_LANES + tid;
    if (i >= A.nplaces) return;                       // (no barrier below: a lane touches its own column only)
    const int nl = A.nl;
    for (int k = 0; k <= nl; ++k) leaf_tab[k * RJ_STAT_LANES + tid] = 0u;
    const uint8_t* p = A.inds + i * nl;
    constexpr int U = 4;                              // kept steps whose masks are in flight together
    int64_t j = 0;
    for (; j + U <= A.count; j += U) {
        int c[U];
#pragma unroll
        for (int u = 0; u < U; ++u) c[u] = __builtin_popcount(rj_stat_mask<VEC>(p + (j + u) * A.inds_stride, nl));
#pragma unroll
        for (int u = 0; u < U; ++u) {
            leaf_tab[c[u] * RJ_STAT_LANES + tid] += 1u;
            if (A.nleaves) A.nleaves[(j + u) * A.nplaces + i] = (uint8_t)c[u];
        }
    }
    for (; j < A.count; ++j) {
        const int c = __builtin_popcount(rj_stat_mask<VEC>(p + j * A.inds_stride, nl));
        leaf_tab[c * RJ_STAT_LANES + tid] += 1u;
        if (A.nleaves) A.nleaves[j * A.nplaces + i] = (uint8_t)c;
    }
    if (A.hist)
        for (int k = 0; k <= nl; ++k) A.hist[i * (nl + 1) + k] = leaf_tab[k * RJ_STAT_LANES + tid];
}

// f(v) for every leaf of the place in use whose ordinal lies in [lo, hi), in ascending (step, slot); v its coordinate `d`.
// Returns how many entered.
template <int VEC, class F>
__device__ __forceinline__ int64_t rj_leaf_walk(const RjStatArgs& A, const uint8_t* pm, const double* px, F&& f) {
    const int nl = A.nl, nd = A.nd;
    int64_t ord = 0, n = 0;
    // one step's leaves; false: the window is behind us
    auto step = [&](uint32_t m, int64_t j) {
        const int c = __builtin_popcount(m);
        if (ord + c <= A.lo) { ord += c; return true; }                // (nothing of this step enters: no coordinate is loaded)
        const double* q = px + j * A.x_stride;
        while (m) {
            const int slot = __builtin_ctz(m);
            m &= m - 1;
            if (ord >= A.lo) { f(q[slot * nd]); ++n; }
            if (++ord >= A.hi) return false;
        }
        return true;
    };
    int64_t j = 0;
    for (; j + STAT_U <= A.count; j += STAT_U) {
        uint32_t m[STAT_U];
#pragma unroll
        for (int u = 0; u < STAT_U; ++u) m[u] = rj_stat_mask<VEC>(pm + (j + u) * A.inds_stride, nl);
#pragma unroll
        for (int u = 0; u < STAT_U; ++u)
            if (!step(m[u], j + u)) return n;
    }
    for (; j < A.count; ++j)
        if (!step(rj_stat_mask<VEC>(pm + j * A.inds_stride, nl), j)) return n;
    return n;
}

template <int VEC>
__global__ __launch_bounds__(RJ_STAT_LANES) void k_rj_chain_leaf_moments(const RjStatArgs A) {
    const int64_t i = (int64_t)blockIdx.x * RJ_STAT_LANES + threadIdx.x;       // series: place x nd + d
    const int nd = A.nd;
    if (i >= A.nplaces * nd) return;
    const int64_t place = i / nd;
    const int d = (int)(i - place * nd);
    const uint8_t* pm = A.inds + place * A.nl;
    const double* px = A.x + place * A.nl * nd + d;
    double s = 0.0, q = 0.0;
    const int64_t n = rj_leaf_walk<VEC>(A, pm, px, [&](double v) { s += v; });
    if (A.m2) {
        const double mean = s / (double)n;
        rj_leaf_walk<VEC>(A, pm, px, [&](double v) { const double y = v - mean; q += y * y; });
        A.m2[i] = q;
    }
    if (A.sum) A.sum[i] = s;
    if (A.n && d == 0) A.n[place] = (long long)n;
}

}  // namespace hens
