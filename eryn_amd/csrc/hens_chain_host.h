// hens_chain_host.h - the capacity / range arithmetic of the chain store (hens_chain_create, hens_step_chain, hens_chain_download) as
// plain host functions without HIP types: hens.hip calls them, and tests/chain_host_check.cpp runs them alone under
// -fsanitize=address,undefined (sizes come straight from the caller: every product is overflow-checked before anything is
// allocated, launched or copied).
#pragma once
#include <cstdint>

namespace hens_chain {

// what one chain holds, in doubles per stored step: x[Ts][W][D], logl / logp [Ts][W] each, betas[T]
struct Shape {
    int64_t T, Ts, W, D;
};
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

}  // namespace hens_chain
