// rj_group_host_check.cpp - the window of a leaf in a friend table (eryn_amd/csrc/hens_rj_group_host.h: rj_group_window) on its
// own, for a sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rj_group_host_check.cpp -o rj_group_host_check && ./rj_group_host_check
// (tests/test_rj_group_move.py::test_window_walk_under_a_sanitizer_build builds and runs it so.)
// The greedy walk against the brute force it stands for - the nf entries a stable argsort of |x - keys| puts first: the same keys
// always, the same entries where the keys are all different (see check() below) -: keys with duplicates, fewer entries than
// friends, an empty table, a key below / above / equal to every entry, ties between the two sides, and random tables.  The key arrays are heap allocations of exactly n doubles, so a read past either end is the sanitizer's.
// Exit status 0 and "ok" = every expectation held.
#include "../eryn_amd/csrc/hens_rj_group_host.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

using namespace hens;

static int failures = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

// the brute force: the table indices a stable argsort of |x - keys| puts first, nf of them, ascending
static std::vector<int> brute(const std::vector<double>& keys, int nfriends, double x) {
    const int n = (int)keys.size(), nf = std::min(nfriends, n);
    std::vector<int> idx((size_t)n);
    std::iota(idx.begin(), idx.end(), 0);
    std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return std::fabs(x - keys[(size_t)a]) < std::fabs(x - keys[(size_t)b]); });
    std::vector<int> w(idx.begin(), idx.begin() + nf);
    std::sort(w.begin(), w.end());
    return w;
}

// What holds between the two (hens_rj_group.h, rule 2): the window's keys ARE the keys of the argsort's first nf entries, value for
// value; where the table's keys are all different the two are the same entries.  Among entries with the SAME key on the left of x the
// walk takes the ones next to x and the stable argsort the ones with the lowest index, so with duplicate keys the argsort's set need
// not even be contiguous ({3, 3, 3, 4}, x = 4, two friends: entries 3 and 0) - a window is contiguous by construction.
static void check(const std::vector<double>& keys, int nfriends, double x) {
    std::vector<double> exact(keys);                      // (capacity == size: the walk may read keys[0 .. n) and nothing else)
    exact.shrink_to_fit();
    const int n = (int)keys.size(), nf = std::min(nfriends, n);
    const int got = rj_group_window(exact.data(), n, nfriends, x);
    const std::vector<int> want = brute(keys, nfriends, x);
    bool ok = got >= 0 && got + nf <= n && (int)want.size() == nf;
    bool distinct = true;
    for (int i = 1; i < n; ++i) distinct = distinct && keys[(size_t)i - 1] < keys[(size_t)i];
    if (ok) {
        std::vector<double> kw, ka;
        for (int j = 0; j < nf; ++j) { kw.push_back(keys[(size_t)(got + j)]); ka.push_back(keys[(size_t)want[(size_t)j]]); }
        std::sort(ka.begin(), ka.end());
        ok = kw == ka;
        if (distinct)
            for (int j = 0; j < nf; ++j) ok = ok && want[(size_t)j] == got + j;
    }
    if (!ok) { std::printf("n = %d nfriends = %d x = %.17g: window %d is not the argsort's\n", n, nfriends, x, got); ++failures; }
}

int main() {
    // ---- an empty table, fewer entries than friends
    check({}, 3, 0.5);
    EXPECT(rj_group_window(nullptr, 0, 64, 1.0) == 0);
    check({1.0}, 3, 0.5);
    check({1.0, 2.0}, 8, 5.0);
    check({1.0, 2.0}, 2, 1.5);
    // ---- duplicates, ties between the two sides (the lower index wins), a key equal to an entry
    const std::vector<double> dup = {1.0, 1.0, 3.0, 3.0, 3.0, 4.0};
    for (int nf = 1; nf <= 7; ++nf)
        for (double x : {0.0, 1.0, 2.0, 2.5, 3.0, 3.5, 4.0, 9.0, -0.0}) check(dup, nf, x);
    EXPECT(rj_group_window(dup.data(), 6, 2, 2.0) == 0);        // |2 - 1| == |3 - 2|: both 1.0 entries come first
    EXPECT(rj_group_window(dup.data(), 6, 3, 2.0) == 0);
    EXPECT(rj_group_window(dup.data(), 6, 1, 2.0) == 1);        // ... and of the two the one next to x (the argsort: entry 0)
    EXPECT(rj_group_window(dup.data(), 6, 2, 4.0) == 4);        // contiguous where the argsort's set {5, 2} is not
    // ---- a key below / above every entry
    const std::vector<double> asc = {-2.0, -1.0, -0.0 + 0.0, 0.5, 0.75, 8.0};
    for (int nf = 1; nf <= 6; ++nf) {
        check(asc, nf, -100.0);
        check(asc, nf, 100.0);
        EXPECT(rj_group_window(asc.data(), 6, nf, -100.0) == 0);
        EXPECT(rj_group_window(asc.data(), 6, nf, 100.0) == 6 - nf);
    }
    // ---- random tables: few distinct values (many duplicates and ties) and many
    uint64_t s = 0x9e3779b97f4a7c15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    for (int trial = 0; trial < 4000; ++trial) {
        const int n = (int)(next() % 40), levels = trial % 2 ? 5 : 1000;
        std::vector<double> keys((size_t)n);
        for (double& k : keys) k = (double)(next() % (uint64_t)levels) / 4.0;
        std::sort(keys.begin(), keys.end());
        const int nf = 1 + (int)(next() % 64);
        check(keys, nf, (double)(next() % (uint64_t)(levels + 8)) / 8.0 - 0.5);
        if (n) check(keys, nf, keys[(size_t)(next() % (uint64_t)n)]);
    }
    if (failures) { std::printf("%d expectation(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
