// chain_stats_host_check.cpp - the launch arithmetic of the chain diagnostics (eryn_amd/csrc/hens_chain_host.h: stat_plan, act_*) on
// its own, for a sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/chain_stats_host_check.cpp -o chain_stats_host_check && ./chain_stats_host_check
// Walks stat_plan over the edges of its domain (zero, one, INT64_MAX, products that pass 2^63) and, for a grid of ordinary shapes
// and ranges, replays every address k_chain_moments / k_chain_act form from an accepted plan - lane by lane, step by step, with the
// kernels' own index expressions - on host arrays of exactly the chain's size and the outputs' size, so that a plan that reaches
// outside them is an AddressSanitizer report; the LDS ring's rows are replayed the same way.  Exit status 0 and "ok" = every
// expectation held.
#include "../eryn_amd/csrc/hens_chain_host.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hens_chain;

static int failures = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

int main() {
    const int64_t MAX = INT64_MAX;
    StatPlan p{};
    // config 2 (16 x 4096 x 32), 400 stored steps, by hand
    const Shape c2{16, 16, 4096, 32};
    EXPECT(stat_plan(c2, 400, 0, 0, 400, 1, 1, &p) && p.offset == 0 && p.stride == 16LL * 4096 * 32 && p.nseries == 4096 * 32 && p.vec == 2);
    EXPECT(stat_plan(c2, 400, 0, 100, 100, 3, 16, &p) && p.offset == 100LL * 16 * 4096 * 32 && p.stride == 3LL * 16 * 4096 * 32 && p.nseries == 16LL * 4096 * 32);
    EXPECT(stat_plan(c2, 400, 1, 399, 1, 1, 16, &p) && p.offset == 399LL * 16 * 4096 && p.nseries == 16 * 4096 && p.vec == 2);
    EXPECT(stat_plan(c2, 400, 2, 1, 200, 2, 3, &p) && p.nseries == 3 * 4096);                 // last kept step 399
    EXPECT(!stat_plan(c2, 400, 2, 2, 200, 2, 3, &p));                                          // ... 400
    // vector width: pairs only where the selection and the step's size are even
    EXPECT(stat_plan(Shape{3, 3, 40, 5}, 9, 0, 0, 9, 1, 3, &p) && p.vec == 2 && p.nseries == 600);      // 3 x 200: even both
    EXPECT(stat_plan(Shape{3, 3, 5, 5}, 9, 0, 0, 9, 1, 3, &p) && p.vec == 1);                  // 75 per step
    EXPECT(stat_plan(Shape{3, 3, 5, 5}, 9, 0, 0, 9, 1, 2, &p) && p.vec == 1 && p.nseries == 50);        // even selection, odd step
    EXPECT(stat_plan(Shape{2, 2, 5, 5}, 9, 0, 0, 9, 1, 1, &p) && p.vec == 1);                  // odd selection, even step
    EXPECT(stat_plan(Shape{4, 2, 7, 11}, 9, 1, 0, 9, 1, 1, &p) && p.vec == 1 && p.nseries == 7);
    EXPECT(stat_plan(Shape{4, 2, 7, 11}, 9, 1, 0, 9, 1, 2, &p) && p.vec == 2 && p.nseries == 14);
    // not plans
    const Shape s{4, 3, 5, 7};
    EXPECT(!stat_plan(s, 9, -1, 0, 1, 1, 1, &p) && !stat_plan(s, 9, 3, 0, 1, 1, 1, &p));      // field
    EXPECT(!stat_plan(s, 9, 0, -1, 1, 1, 1, &p) && !stat_plan(s, 9, 0, 9, 1, 1, 1, &p) && stat_plan(s, 9, 0, 8, 1, 1, 1, &p));
    EXPECT(!stat_plan(s, 9, 0, 0, 0, 1, 1, &p) && !stat_plan(s, 9, 0, 0, -3, 1, 1, &p) && !stat_plan(s, 9, 0, 0, 10, 1, 1, &p));
    EXPECT(!stat_plan(s, 9, 0, 0, 1, 0, 1, &p) && !stat_plan(s, 9, 0, 0, 1, -1, 1, &p));
    EXPECT(!stat_plan(s, 9, 0, 0, 1, 1, 0, &p) && !stat_plan(s, 9, 0, 0, 1, 1, 4, &p) && stat_plan(s, 9, 0, 0, 1, 1, 3, &p));
    EXPECT(!stat_plan(s, 0, 0, 0, 1, 1, 1, &p) && !stat_plan(s, -1, 0, 0, 1, 1, 1, &p));     // an empty chain keeps nothing
    EXPECT(!stat_plan(Shape{4, 5, 5, 7}, 9, 0, 0, 1, 1, 1, &p) && !stat_plan(Shape{4, 3, 0, 7}, 9, 0, 0, 1, 1, 1, &p));
    // beyond int64: refused, never wrapped
    EXPECT(!stat_plan(s, 9, 0, 1, MAX, MAX, 1, &p) && !stat_plan(s, 9, 0, MAX, 2, MAX, 1, &p) && !stat_plan(s, 9, 0, 0, 2, MAX, 1, &p));
    EXPECT(stat_plan(s, 9, 0, 8, 1, MAX, 1, &p) && p.stride == 3 * 5 * 7);                   // one kept step: thin never multiplies
    EXPECT(!stat_plan(s, MAX, 0, 0, 1, 1, 1, &p) && !stat_plan(Shape{MAX, MAX, MAX, MAX}, 9, 0, 0, 1, 1, 1, &p));
    EXPECT(!stat_plan(Shape{4, 3, MAX / 2, 7}, 9, 0, 0, 1, 1, 1, &p) && !stat_plan(s, 9, INT64_MIN, 0, 1, 1, 1, &p));
    // the autocorrelation kernel's plan
    EXPECT(act_lags(50, 400) == 50 && act_lags(50, 20) == 20 && act_lags(7, 7) == 7 && act_lags(MAX, 3) == 3);
    EXPECT(act_fits(1) && act_fits(50) && act_fits(64) && !act_fits(65) && !act_fits(0) && !act_fits(-1) && !act_fits(MAX));
    EXPECT(act_kmax(1) == 16 && act_kmax(16) == 16 && act_kmax(17) == 32 && act_kmax(32) == 32 && act_kmax(33) == 64 && act_kmax(50) == 64 && act_kmax(64) == 64);
    EXPECT(act_lds_bytes(50) == 50 * 64 * 8 && act_lds_bytes(ACT_WINDOW_MAX) <= 64 * 1024);  // (under the default dynamic-LDS limit)
    EXPECT(stat_blocks(1, 256) == 1 && stat_blocks(256, 256) == 1 && stat_blocks(257, 256) == 2 && stat_blocks(4096 * 32, 64) == 2048);
    // every address of an accepted plan: inside a chain of exactly `stored` steps, inside outputs of exactly nseries
    for (const Shape& sh : {Shape{4, 4, 64, 8}, Shape{3, 3, 40, 5}, Shape{16, 3, 40, 8}, Shape{4, 4, 33, 11}, Shape{2, 1, 3, 1}})
        for (int64_t stored : {(int64_t)1, (int64_t)7, (int64_t)20})
            for (int64_t field = 0; field <= 2; ++field) {
                const int64_t step = sh.Ts * sh.W * (field == 0 ? sh.D : 1);
                std::vector<char> chain((size_t)(stored * step), 0);
                for (int64_t first = -1; first <= stored; ++first)
                    for (int64_t count = 0; count <= stored + 1; ++count)
                        for (int64_t thin = 0; thin <= 4; ++thin)
                            for (int64_t nt = 0; nt <= sh.Ts + 1; ++nt) {
                                if (!stat_plan(sh, stored, field, first, count, thin, nt, &p)) {
                                    const bool fine = first >= 0 && count >= 1 && thin >= 1 && nt >= 1 && nt <= sh.Ts && first + (count - 1) * thin < stored;
                                    EXPECT(!fine);
                                    continue;
                                }
                                EXPECT(first + (count - 1) * thin < stored && p.nseries == nt * step / sh.Ts);
                                std::vector<char> out((size_t)p.nseries, 0);
                                const char* src = chain.data() + p.offset;
                                // k_chain_moments: lanes of whole workgroups of 256, VEC series each
                                const int64_t lanes = stat_blocks(p.nseries / p.vec, 256) * 256;
                                for (int64_t g = 0; g < lanes; ++g) {
                                    const int64_t i = g * p.vec;
                                    if (i >= p.nseries) continue;
                                    for (int64_t j = 0; j < count; j += (count > 3 ? count - 1 : 1))      // (first, last and, on short ranges, every step)
                                        for (int e = 0; e < p.vec; ++e) EXPECT(src[i + j * p.stride + e] == 0);
                                    for (int e = 0; e < p.vec; ++e) out[(size_t)(i + e)] += 1;
                                }
                                for (char c : out) EXPECT(c == 1);                                         // every series written exactly once
                                // k_chain_act: waves of ACT_LANES, tail lanes read series 0 and write nothing
                                if (field == 0) {
                                    const int64_t waves = stat_blocks(p.nseries, ACT_LANES);
                                    for (int64_t g = 0; g < waves * ACT_LANES; ++g) {
                                        const bool live = g < p.nseries;
                                        EXPECT(src[(live ? g : 0) + (count - 1) * p.stride] == 0);
                                        if (live) out[(size_t)g] += 1;
                                    }
                                    for (char c : out) EXPECT(c == 2);
                                }
                            }
            }
    // the LDS ring: every row the kernel forms lies in [0, K), and lag k of sample j reads what sample j - k wrote
    for (int64_t K = 1; K <= ACT_WINDOW_MAX; ++K) {
        std::vector<int64_t> ring((size_t)(act_lds_bytes(K) / 8 / ACT_LANES), -1);
        int h = 0;
        for (int64_t j = 0; j < 3 * K + 2; ++j) {
            ring[(size_t)h] = j;
            const int top = (int)(j < K - 1 ? j : K - 1);
            for (int k = 1; k < act_kmax(K); ++k)
                if (k <= top) {
                    const int row = h - k < 0 ? h - k + (int)K : h - k;
                    EXPECT(ring[(size_t)row] == j - k);
                }
            h = h + 1 == K ? 0 : h + 1;
        }
    }
    if (failures) return EXIT_FAILURE;
    std::puts("ok");
    return EXIT_SUCCESS;
}
