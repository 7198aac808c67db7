// hens_rj_group_host.h - the window of a leaf in a branch's friend table (hens_rj_group.h, rule 2), for the host and the device.
//
// keys[0 .. n) are the table's keys, ascending.  The window of a leaf whose key parameter is x holds the nf <= n table entries a
// STABLE argsort of |x - keys| puts first.  On sorted keys these are contiguous, so the window is its first index.  It is found by
// a greedy walk from pos = lower_bound(keys, x): nf times, step left when there is an entry on the left and either none on the
// right or the left one is no farther (ties go left: the lower index, as the stable argsort has it), else step right.
// tools/rj_group_host_check.cpp holds this function to the argsort under -fsanitize=address,undefined.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HENS_HD __host__ __device__
#else
#define HENS_HD
#endif

namespace hens {

constexpr int RJ_GROUP_MAX_FRIENDS = 64;

// first index i with keys[i] >= x (n if there is none)
HENS_HD inline int rj_group_lower_bound(const double* keys, int n, double x) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// the window's first index; nf = min(nfriends, n) entries belong to it (nf == 0: 0)
HENS_HD inline int rj_group_window(const double* keys, int n, int nfriends, double x) {
    const int nf = nfriends < n ? nfriends : n;
    int lo = rj_group_lower_bound(keys, n, x), hi = lo;           // the window is [lo, hi)
    for (int k = 0; k < nf; ++k) {
        const bool left = lo > 0 && (hi == n || __builtin_fabs(x - keys[lo - 1]) <= __builtin_fabs(keys[hi] - x));
        if (left) --lo;
        else ++hi;
    }
    return lo;
}

}  // namespace hens
