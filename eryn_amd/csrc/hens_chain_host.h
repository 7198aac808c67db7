// hens_chain_host.h - the capacity / range / launch arithmetic of the chain store's two families (hens_chain_*, hens_step_chain; on a
// leaf-packing context hens_rj_chain_*, hens_rj_step_chain: one host protocol in hens.hip) as plain host functions without HIP types:
// hens.hip calls them, and tools/chain_host_check.cpp, tools/chain_stats_host_check.cpp and tools/rj_chain_stats_host_check.cpp run
// them alone under -fsanitize=address,undefined (sizes come straight from the caller: every product is overflow-checked before
// anything is allocated, launched or copied).
#pragma once
#include <cstdint>

namespace hens_chain {

// what one chain holds, in doubles per stored step: x[Ts][W][D], logl / logp [Ts][W] each, betas[T]
struct Shape { int64_t T, Ts, W, D; };
struct Sizes {          // bytes of the four device arrays of a chain of `capacity` steps, and of one step
    int64_t x, lp, betas, step, total;
};

enum { OK = 0, INVALID = 1, FULL = 2 };

inline bool mul(int64_t a, int64_t b, int64_t* out) { return !__builtin_mul_overflow(a, b, out); }
inline bool add(int64_t a, int64_t b, int64_t* out) { return !__builtin_add_overflow(a, b, out); }

// false: not a shape (a dimension < 1, more stored rungs than rungs) or a size beyond int64
inline bool sizes(const Shape& s, int64_t capacity, Sizes* out) {
    if (s.T < 1 || s.W < 1 || s.D < 1 || s.Ts < 1 || s.Ts > s.T || capacity < 0) return false;
    int64_t tw, row, lp1, x1, b1, step;
    if (!mul(s.T, 8, &b1) || !mul(s.Ts, s.W, &tw) || !mul(tw, 8, &lp1) || !mul(tw, s.D, &row) || !mul(row, 8, &x1)) return false;
    if (!add(x1, lp1, &step) || !add(step, lp1, &step) || !add(step, b1, &step)) return false;
    Sizes z{};
    z.step = step;
    if (!mul(x1, capacity, &z.x) || !mul(lp1, capacity, &z.lp) || !mul(b1, capacity, &z.betas) || !mul(step, capacity, &z.total)) return false;
    *out = z;
    return true;
}

// hens_step_chain's arguments against the chain: INVALID (a count < 0, n_last < 1, iters_per_store < n_last, more iterations than
// an int64 counts), FULL (the steps do not fit behind `count`), else OK with the iterations the call runs in *iters
inline int append_check(int64_t capacity, int64_t count, int64_t n_store, int64_t iters_per_store, int64_t n_last, int64_t* iters) {
    if (n_store < 0 || n_last < 1 || iters_per_store < n_last) return INVALID;
    if (count < 0 || count > capacity) return INVALID;
    if (n_store > capacity - count) return FULL;
    if (!mul(n_store, iters_per_store, iters)) return INVALID;
    return OK;
}

// a download range [first, first + n) inside [0, count)   (n = 0: allowed anywhere in [0, count])
inline bool range_ok(int64_t count, int64_t first, int64_t n) {
    return first >= 0 && n >= 0 && first <= count && n <= count - first;
}

// ---- leaf-packing contexts (hens_rj_chain_*, hens_rj_step_chain) ----------------------------------------------------------------
// what one chain of a leaf-packing context holds per stored step: per branch b x_b[Ts][W][nl_b][nd_b] doubles and inds_b[Ts][W][nl_b]
// bytes, logl / logp [Ts][W] each, betas[T]:  step = 8 (Ts W (ncoord + 2) + T) + Ts W nslots bytes
constexpr int RJ_BRANCHES = 4;
struct RjShape {
    int64_t T, Ts, W, nb;
    int64_t nl[RJ_BRANCHES], nd[RJ_BRANCHES];
};
struct RjSizes {        // bytes of the device arrays of a chain of `capacity` steps, and of one step
    int64_t x[RJ_BRANCHES], inds[RJ_BRANCHES], lp, betas, step, total;
    int64_t ncoord, nslots;
};

// false: not a shape (a dimension < 1, more stored rungs than rungs, more branches than a record has) or a size beyond int64
inline bool rj_sizes(const RjShape& s, int64_t capacity, RjSizes* out) {
    if (s.T < 1 || s.W < 1 || s.Ts < 1 || s.Ts > s.T || s.nb < 1 || s.nb > RJ_BRANCHES || capacity < 0) return false;
    int64_t tw, lp1, b1, step;
    if (!mul(s.T, 8, &b1) || !mul(s.Ts, s.W, &tw) || !mul(tw, 8, &lp1)) return false;
    if (!add(lp1, lp1, &step) || !add(step, b1, &step)) return false;
    RjSizes z{};
    for (int b = 0; b < s.nb; ++b) {
        if (s.nl[b] < 1 || s.nd[b] < 1) return false;
        int64_t seg, row, x1, i1;
        if (!mul(s.nl[b], s.nd[b], &seg) || !mul(tw, seg, &row) || !mul(row, 8, &x1) || !mul(tw, s.nl[b], &i1)) return false;
        if (!add(step, x1, &step) || !add(step, i1, &step)) return false;
        if (!add(z.ncoord, seg, &z.ncoord) || !add(z.nslots, s.nl[b], &z.nslots)) return false;
        if (!mul(x1, capacity, &z.x[b]) || !mul(i1, capacity, &z.inds[b])) return false;
    }
    z.step = step;
    if (!mul(lp1, capacity, &z.lp) || !mul(b1, capacity, &z.betas) || !mul(step, capacity, &z.total)) return false;
    *out = z;
    return true;
}

// hens_rj_step_chain's arguments against the chain (a stored step's accept totals take its last iteration: n_last = 1)
inline int rj_append_check(int64_t capacity, int64_t count, int64_t n_store, int64_t iters_per_store, int64_t* iters) {
    return append_check(capacity, count, n_store, iters_per_store, 1, iters);
}

// hens_rj_chain_download's branch: one of the model's, or -1 (the shared fields only)
inline bool rj_branch_ok(int64_t nb, int64_t branch) { return branch >= -1 && branch < nb; }

// The append launch of BOTH families: a row is a list of segments, and a fixed-dimension chain's (k_chain_store) is the one-segment case
inline RjShape one_segment(const Shape& s) { return RjShape{s.T, s.Ts, s.W, 1, {1}, {s.D}}; }      // D doubles at offset 0
// doubles per lane of the append launch: 2 (16-byte loads and stores) where every segment starts and ends on an even double on both
// sides - the source's rows are RW doubles apart, the destination's rows nl nd -, else 1   (one segment: RW and D both even)
inline int rj_store_vec(const RjShape& s, int64_t RW) {
    int64_t off = 0;
    if (RW % 2) return 1;
    for (int b = 0; b < s.nb; ++b) {
        const int64_t seg = s.nl[b] * s.nd[b];
        if (off % 2 || seg % 2) return 1;
        off += seg;
    }
    return 2;
}

// lanes per record as a shift: the smallest power of two that covers the widest segment, at most a wave (a wider one takes rounds)
inline int rj_lane_shift(const RjShape& s, int vec) {
    int64_t widest = 1;
    for (int b = 0; b < s.nb; ++b) widest = s.nl[b] * s.nd[b] > widest ? s.nl[b] * s.nd[b] : widest;
    int sh = 0;
    while (((int64_t)1 << sh) * vec < widest && sh < 6) ++sh;
    return sh;
}

// ---- chain diagnostics (hens_chain_moments, hens_chain_act; csrc/hens_chain_stats.h) ---------------------------------------------
// The kept steps first, first + thin, ..., first + (count - 1) thin of a chain that holds `stored` steps, the rungs [0, ntemps) of
// field 0 (x: W D doubles per rung), 1 or 2 (logl, logp: W per rung).  A series is one double of the selected head of a step's slice.
struct StatPlan {
    int64_t offset;     // doubles from the field's base to the first kept step's slice
    int64_t stride;     // doubles between kept steps
    int64_t nseries;    // ntemps x W x D, or ntemps x W
    int vec;            // doubles per lane of k_chain_moments: 2 where every kept step's selection starts on 16 bytes and pairs up
};

inline bool stat_plan(const Shape& s, int64_t stored, int64_t field, int64_t first, int64_t count, int64_t thin, int64_t ntemps, StatPlan* out) {
    if (s.T < 1 || s.W < 1 || s.D < 1 || s.Ts < 1 || s.Ts > s.T || stored < 0) return false;
    if (field < 0 || field > 2 || first < 0 || count < 1 || thin < 1 || ntemps < 1 || ntemps > s.Ts) return false;
    int64_t span, last;
    if (!mul(count - 1, thin, &span) || !add(first, span, &last) || last >= stored) return false;
    int64_t width = s.W, step, total;
    if (field == 0 && !mul(s.W, s.D, &width)) return false;
    if (!mul(s.Ts, width, &step) || !mul(step, stored, &total) || !mul(total, 8, &total)) return false;    // (every offset below is inside `total`)
    StatPlan p{};
    p.offset = first * step;
    p.stride = count > 1 ? thin * step : step;          // (count > 1: thin <= last < stored; one kept step: never used)
    p.nseries = ntemps * width;
    p.vec = (p.nseries % 2 == 0 && step % 2 == 0) ? 2 : 1;
    *out = p;
    return true;
}

// k_chain_act: a workgroup is one wave of ACT_LANES series; its LDS ring holds K = min(window, count) centred values per lane, its
// registers up to ACT_WINDOW_MAX accumulators
constexpr int ACT_LANES = 64, ACT_WINDOW_MAX = 64;
inline int64_t act_lags(int64_t window, int64_t count) { return window < count ? window : count; }
inline bool act_fits(int64_t lags) { return lags >= 1 && lags <= ACT_WINDOW_MAX; }
inline int64_t act_lds_bytes(int64_t lags) { return lags * ACT_LANES * 8; }
// accumulators the instantiation carries: the smallest of 16 / 32 / 64 that covers the lags
inline int act_kmax(int64_t lags) { return lags <= 16 ? 16 : lags <= 32 ? 32 : 64; }
inline int64_t stat_blocks(int64_t lanes, int64_t per_block) { return (lanes + per_block - 1) / per_block; }

// ---- chain diagnostics of a leaf-packing context (hens_rj_chain_leaves, hens_rj_chain_leaf_moments; csrc/hens_rj_chain_stats.h) ----
// The kept steps first, first + thin, ... of branch `branch` of a chain that holds `stored` steps, the rungs [0, ntemps): a PLACE is
// one (rung, walker) of the selection, a series one (place, parameter).  Place i's nl mask bytes sit at byte i nl of a step's mask
// slice, its coordinates at double i nl nd of the step's coordinate slice.
constexpr int RJ_STAT_LANES = 256, RJ_STAT_NL_MAX = 32, RJ_STAT_ND_MAX = 4;
constexpr int64_t RJ_STAT_COUNT_MAX = (int64_t)1 << 31;      // kept steps: a u32 histogram bin cannot wrap
struct RjStatPlan {
    int64_t inds_offset, inds_stride;   // bytes from inds_b's base to the first kept step's slice / between kept steps
    int64_t x_offset, x_stride;         // doubles, of x_b
    int64_t nplaces, nseries;           // ntemps x W, ntemps x W x nd
    int64_t nl, nd;
    int64_t lds_bytes;                  // k_rj_chain_leaves' table [nl + 1][RJ_STAT_LANES] of u32
    int vec;                            // mask bytes per load: 4 where nl is a multiple of 4 (every place starts on a dword), else 1
};

inline bool rj_stat_plan(const RjShape& s, int64_t stored, int64_t branch, int64_t first, int64_t count, int64_t thin, int64_t ntemps,
                         RjStatPlan* out) {
    RjSizes sz{};
    if (stored < 0 || !rj_sizes(s, stored, &sz)) return false;                  // (the shape, and every buffer size inside int64)
    if (branch < 0 || branch >= s.nb) return false;
    const int64_t nl = s.nl[branch], nd = s.nd[branch];
    if (nl > RJ_STAT_NL_MAX || nd > RJ_STAT_ND_MAX) return false;
    if (first < 0 || count < 1 || count > RJ_STAT_COUNT_MAX || thin < 1 || ntemps < 1 || ntemps > s.Ts) return false;
    int64_t span, last;
    if (!mul(count - 1, thin, &span) || !add(first, span, &last) || last >= stored) return false;
    int64_t tw, istep, xstep;
    if (!mul(s.Ts, s.W, &tw) || !mul(tw, nl, &istep) || !mul(istep, nd, &xstep)) return false;
    RjStatPlan p{};
    p.nl = nl; p.nd = nd;
    p.inds_offset = first * istep;                       // (first <= last < stored, and stored x istep = sz.inds fits)
    p.x_offset = first * xstep;
    p.inds_stride = count > 1 ? thin * istep : istep;    // (count > 1: thin <= last < stored; one kept step: never used)
    p.x_stride = count > 1 ? thin * xstep : xstep;
    p.nplaces = ntemps * s.W;
    p.nseries = p.nplaces * nd;
    p.lds_bytes = (nl + 1) * RJ_STAT_LANES * 4;
    p.vec = nl % 4 == 0 ? 4 : 1;
    *out = p;
    return true;
}

// k_rj_chain_leaf_moments' ordinal window [lo, hi)
inline bool rj_window_ok(int64_t lo, int64_t hi) { return lo >= 0 && lo < hi; }

// hens_rj_chain_moments: the fixed-dimension plan over a leaf-packing chain's own arrays - field 0: x of `branch` as stored, a
// "coordinate" row the nl nd doubles of a walker; 1 / 2: logl / logp
inline bool rj_plain_plan(const RjShape& s, int64_t stored, int64_t field, int64_t branch, int64_t first, int64_t count, int64_t thin,
                          int64_t ntemps, StatPlan* out) {
    RjSizes sz{};
    if (stored < 0 || !rj_sizes(s, stored, &sz)) return false;
    if (field == 0 && (branch < 0 || branch >= s.nb)) return false;
    const int64_t D = field == 0 ? s.nl[branch] * s.nd[branch] : 1;             // (rj_sizes multiplied them)
    return stat_plan(Shape{s.T, s.Ts, s.W, D}, stored, field, first, count, thin, ntemps, out);
}

}  // namespace hens_chain
