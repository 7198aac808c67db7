// chain_host_check.cpp - the chain store's capacity / range arithmetic (eryn_amd/csrc/hens_chain_host.h) on its own, for a
// sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/chain_host_check.cpp -o chain_host_check && ./chain_host_check
// Walks the functions over the edges of their domains (zero, one, INT64_MAX, products that pass 2^63) and over a grid of ordinary
// shapes, and replays what hens_chain_download does with an accepted range on host arrays of exactly `count` entries, so that an
// accepted range that reaches outside them is an AddressSanitizer report.  Exit status 0 and "ok" = every expectation held.
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
    Sizes z{};
    // sizes: config 2 (16 x 4096 x 32) by hand
    EXPECT(sizes(Shape{16, 16, 4096, 32}, 400, &z));
    EXPECT(z.step == 8 * (16 * 4096 * 34 + 16) && z.x == 400LL * 16 * 4096 * 32 * 8 && z.lp == 400LL * 16 * 4096 * 8 && z.betas == 400 * 16 * 8);
    EXPECT(z.total == 400 * z.step && z.total == z.x + 2 * z.lp + z.betas);
    EXPECT(sizes(Shape{6, 1, 33, 11}, 1, &z) && z.step == 8 * (33 * 13 + 6));
    // not shapes
    for (const Shape& s : {Shape{0, 0, 4, 4}, Shape{4, 5, 4, 4}, Shape{4, 0, 4, 4}, Shape{4, 4, 0, 4}, Shape{4, 4, 4, 0}, Shape{-1, -1, 4, 4}, Shape{4, 4, -4, 4}})
        EXPECT(!sizes(s, 1, &z));
    EXPECT(!sizes(Shape{4, 4, 4, 4}, -1, &z));
    // byte counts beyond int64: refused, never wrapped
    EXPECT(!sizes(Shape{MAX, MAX, MAX, MAX}, MAX, &z));
    EXPECT(!sizes(Shape{16, 16, 4096, 32}, MAX, &z));
    EXPECT(!sizes(Shape{16, 16, MAX / 8, 32}, 1, &z));
    EXPECT(!sizes(Shape{MAX, 1, 1, 1}, 1, &z));
    EXPECT(sizes(Shape{16, 16, 4096, 32}, 0, &z) && z.total == 0 && z.step > 0);
    const int64_t big = MAX / (8 * (16 * 4096 * 34 + 16));
    EXPECT(sizes(Shape{16, 16, 4096, 32}, big, &z) && !sizes(Shape{16, 16, 4096, 32}, big + 1, &z));
    // append_check
    int64_t it = -1;
    EXPECT(append_check(12, 0, 12, 3, 1, &it) == OK && it == 36);
    EXPECT(append_check(12, 5, 7, 1, 1, &it) == OK && it == 7);
    EXPECT(append_check(12, 5, 8, 1, 1, &it) == FULL);
    EXPECT(append_check(12, 12, 0, 1, 1, &it) == OK && it == 0);
    EXPECT(append_check(12, 12, 1, 1, 1, &it) == FULL);
    EXPECT(append_check(0, 0, 1, 1, 1, &it) == FULL);
    EXPECT(append_check(12, 0, 1, 1, 0, &it) == INVALID && append_check(12, 0, 1, 1, 2, &it) == INVALID && append_check(12, 0, 1, 0, 0, &it) == INVALID);
    EXPECT(append_check(12, 0, -1, 1, 1, &it) == INVALID && append_check(12, 0, 1, 1, -1, &it) == INVALID);
    EXPECT(append_check(12, 13, 0, 1, 1, &it) == INVALID && append_check(12, -1, 0, 1, 1, &it) == INVALID);
    EXPECT(append_check(MAX, 0, MAX, 1, 1, &it) == OK && it == MAX);
    EXPECT(append_check(MAX, 0, MAX, 2, 1, &it) == INVALID);              // n_store * iters_per_store passes 2^63
    EXPECT(append_check(MAX, 1, MAX, 1, 1, &it) == FULL);                 // capacity - count, never count + n_store
    EXPECT(append_check(MAX, MAX, MAX, MAX, MAX, &it) == FULL);
    EXPECT(append_check(4, 0, 2, MAX, MAX, &it) == INVALID && append_check(4, 0, 1, MAX, MAX, &it) == OK && it == MAX);
    // range_ok
    EXPECT(range_ok(12, 0, 12) && range_ok(12, 11, 1) && range_ok(12, 12, 0) && range_ok(0, 0, 0) && range_ok(12, 3, 0));
    EXPECT(!range_ok(12, 0, 13) && !range_ok(12, 12, 1) && !range_ok(12, 13, 0) && !range_ok(12, -1, 1) && !range_ok(12, 1, -1));
    EXPECT(!range_ok(12, MAX, MAX) && !range_ok(12, 1, MAX) && !range_ok(MAX, MAX, 1) && range_ok(MAX, MAX - 1, 1) && !range_ok(12, INT64_MIN, 1));
    // every accepted range stays inside arrays of `count` entries (what hens_chain_download copies from); the x offsets inside the buffer
    for (int64_t count = 0; count <= 9; ++count) {
        std::vector<int64_t> iteration((size_t)count);
        for (int64_t k = 0; k < count; ++k) iteration[(size_t)k] = 10 * k;
        EXPECT(sizes(Shape{3, 2, 5, 7}, count, &z));
        std::vector<char> x((size_t)z.x);
        for (int64_t first = -2; first <= 11; ++first)
            for (int64_t n = -2; n <= 11; ++n) {
                if (!range_ok(count, first, n)) continue;
                std::vector<int64_t> out((size_t)n);
                for (int64_t k = 0; k < n; ++k) out[(size_t)k] = iteration[(size_t)(first + k)];
                EXPECT(n == 0 || out[(size_t)(n - 1)] == 10 * (first + n - 1));
                const int64_t one = 2 * 5 * 7 * 8;
                for (int64_t b = first * one; b < (first + n) * one; b += one) x[(size_t)b] = 1, x[(size_t)(b + one - 1)] = 1;
            }
    }
    if (failures) return EXIT_FAILURE;
    std::puts("ok");
    return EXIT_SUCCESS;
}
