// chain_host_check.cpp - the chain store's capacity / range arithmetic (eryn_amd/csrc/hens_chain_host.h) on its own, for a
// sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/chain_host_check.cpp -o chain_host_check && ./chain_host_check
// (tests/test_chain_backend.py::test_capacity_and_launch_arithmetic_under_a_sanitizer_build builds and runs it so.)
// Covers the fixed-dimension chain (hens_chain_*) and the leaf-packing one (hens_rj_chain_*: sizes per branch, branch range), and
// the store width and lanes per record of both append kernels (k_chain_store: one segment; k_rj_chain_store).  Walks the functions over the edges of their domains (zero, one, INT64_MAX, products that pass 2^63) and over a grid of ordinary
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
    // ---- leaf-packing chains (hens_rj_chain_*) ----
    RjSizes r{};
    // config 4's shape (8 x 2048, pulses x 10 + sines x 10: 60 coordinates, 20 leaf slots) by hand
    const RjShape c4{8, 8, 2048, 2, {10, 10}, {3, 3}};
    EXPECT(rj_sizes(c4, 100, &r));
    EXPECT(r.ncoord == 60 && r.nslots == 20 && r.step == 8 * (8 * 2048 * 62 + 8) + 8 * 2048 * 20);
    EXPECT(r.x[0] == 100LL * 8 * 2048 * 30 * 8 && r.x[1] == r.x[0] && r.inds[0] == 100LL * 8 * 2048 * 10 && r.x[2] == 0 && r.inds[3] == 0);
    EXPECT(r.total == 100 * r.step && r.total == r.x[0] + r.x[1] + r.inds[0] + r.inds[1] + 2 * r.lp + r.betas);
    // odd offsets, stored rungs fewer than rungs, four branches of widths 1 .. 4
    EXPECT(rj_sizes(RjShape{4, 2, 10, 2, {3, 4}, {3, 3}}, 1, &r) && r.step == 8 * (2 * 10 * 23 + 4) + 2 * 10 * 7);
    const RjShape w4{4, 4, 33, 4, {3, 2, 2, 2}, {1, 2, 3, 4}};
    EXPECT(rj_sizes(w4, 3, &r) && r.ncoord == 21 && r.nslots == 9 && r.step == 8 * (4 * 33 * 23 + 4) + 4 * 33 * 9);
    EXPECT(r.x[3] == 3 * 4 * 33 * 8 * 8 && r.inds[1] == 3 * 4 * 33 * 2);
    // not shapes
    for (const RjShape& s : {RjShape{0, 0, 4, 1, {1}, {1}}, RjShape{4, 5, 4, 1, {1}, {1}}, RjShape{4, 0, 4, 1, {1}, {1}}, RjShape{4, 4, 0, 1, {1}, {1}},
                             RjShape{4, 4, 4, 0, {1}, {1}}, RjShape{4, 4, 4, 5, {1, 1, 1, 1}, {1, 1, 1, 1}}, RjShape{4, 4, 4, 2, {1, 0}, {1, 1}},
                             RjShape{4, 4, 4, 2, {1, 1}, {1, -3}}, RjShape{4, 4, 4, -1, {1}, {1}}})
        EXPECT(!rj_sizes(s, 1, &r));
    EXPECT(!rj_sizes(c4, -1, &r));
    // byte counts beyond int64: refused, never wrapped
    EXPECT(!rj_sizes(RjShape{MAX, MAX, MAX, 4, {MAX, MAX, MAX, MAX}, {MAX, MAX, MAX, MAX}}, MAX, &r));
    EXPECT(!rj_sizes(c4, MAX, &r));
    EXPECT(!rj_sizes(RjShape{8, 8, MAX / 8, 2, {10, 10}, {3, 3}}, 1, &r));
    EXPECT(!rj_sizes(RjShape{8, 8, 2048, 1, {MAX / 2}, {3}}, 1, &r));
    EXPECT(rj_sizes(c4, 0, &r) && r.total == 0 && r.step > 0);
    const int64_t step4 = 8 * (8 * 2048 * 62 + 8) + 8 * 2048 * 20, big4 = MAX / step4;
    EXPECT(rj_sizes(c4, big4, &r) && !rj_sizes(c4, big4 + 1, &r));
    // rj_append_check: append_check with n_last = 1
    EXPECT(rj_append_check(12, 0, 12, 3, &it) == OK && it == 36);
    EXPECT(rj_append_check(12, 5, 8, 1, &it) == FULL && rj_append_check(12, 12, 0, 1, &it) == OK && it == 0);
    EXPECT(rj_append_check(12, 0, 1, 0, &it) == INVALID && rj_append_check(12, 0, 1, -1, &it) == INVALID && rj_append_check(12, 0, -1, 1, &it) == INVALID);
    EXPECT(rj_append_check(MAX, 0, MAX, 2, &it) == INVALID && rj_append_check(MAX, 1, MAX, 1, &it) == FULL);
    // rj_branch_ok
    EXPECT(rj_branch_ok(2, -1) && rj_branch_ok(2, 0) && rj_branch_ok(2, 1) && !rj_branch_ok(2, 2) && !rj_branch_ok(2, -2) && !rj_branch_ok(4, MAX) && !rj_branch_ok(4, INT64_MIN));
    // store width: 16-byte lanes only where every segment starts and ends on an even double on both sides
    EXPECT(rj_store_vec(RjShape{4, 4, 10, 2, {3, 4}, {3, 3}}, 24) == 1);       // 9 | 12: the second offset is odd
    EXPECT(rj_store_vec(c4, 62) == 2);                                          // 30 | 30
    EXPECT(rj_store_vec(RjShape{4, 4, 10, 2, {4, 3}, {3, 3}}, 24) == 1);       // 12 | 9: the last segment's end
    EXPECT(rj_store_vec(w4, 26) == 1);                                          // 3 | 4 | 6 | 8
    EXPECT(rj_store_vec(RjShape{4, 4, 10, 2, {32, 32}, {1, 2}}, 98) == 2 && rj_store_vec(RjShape{4, 4, 10, 2, {21, 20}, {3, 3}}, 126) == 1);
    EXPECT(rj_store_vec(c4, 63) == 1);
    // lanes per record: the widest segment covered, a power of two, at most a wave; and every lane's stores stay inside its segment
    for (const RjShape& s : {c4, w4, RjShape{4, 4, 10, 2, {3, 4}, {3, 3}}, RjShape{4, 4, 10, 1, {5}, {3}}, RjShape{4, 4, 10, 2, {32, 32}, {1, 2}},
                             RjShape{4, 4, 10, 2, {21, 20}, {3, 3}}, RjShape{4, 4, 10, 1, {1}, {1}}, RjShape{2, 2, 3, 4, {32, 1, 1, 1}, {4, 1, 1, 1}}})
        for (int64_t RW : {(int64_t)130, (int64_t)131}) {
            const int vec = rj_store_vec(s, RW), sh = rj_lane_shift(s, vec), lpr = 1 << sh;
            EXPECT(sh >= 0 && sh <= 6 && (vec == 1 || vec == 2));
            for (int b = 0; b < s.nb; ++b) {
                const int64_t seg = s.nl[b] * s.nd[b];
                EXPECT(sh == 6 || (int64_t)lpr * vec >= seg);
                std::vector<char> dst((size_t)seg * 8, 0);                      // (the kernel's loop: an overrun is an ASan report)
                for (int j = 0; j < lpr; ++j)
                    for (int64_t e = (int64_t)j * vec; e + vec <= seg; e += (int64_t)lpr * vec)
                        for (int64_t k = e * 8; k < (e + vec) * 8; ++k) dst[(size_t)k] += 1;
                for (char ch : dst) EXPECT(ch == 1);                            // every byte written exactly once
            }
        }
    // the fixed-dimension chain is the one-segment case of the same two functions: the width and shift launch_chain_store had inline,
    // and k_chain_store's copy loop (csrc/hens_chain.h) on a row of exactly D doubles
    for (int64_t D : {1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 130})
        for (int64_t RW : {D, D + 1}) {
            const RjShape s = one_segment(Shape{4, 3, 10, D});
            EXPECT(s.nb == 1 && s.nl[0] * s.nd[0] == D && s.T == 4 && s.Ts == 3 && s.W == 10);
            const int vec = rj_store_vec(s, RW), sh = rj_lane_shift(s, vec), lpr = 1 << sh;
            EXPECT(vec == ((RW % 2 == 0 && D % 2 == 0) ? 2 : 1));
            int want = 0;
            while ((1 << want) * vec < D && want < 6) ++want;
            EXPECT(sh == want);
            std::vector<char> dst((size_t)D * 8, 0);                            // (an overrun is an ASan report)
            for (int j = 0; j < lpr; ++j)
                for (int64_t e = (int64_t)j * vec; e + vec <= D; e += (int64_t)lpr * vec)
                    for (int64_t k = e * 8; k < (e + vec) * 8; ++k) dst[(size_t)k] += 1;
            for (char ch : dst) EXPECT(ch == 1);                                // every byte written exactly once
        }
    // what hens_rj_chain_download copies for an accepted (range, branch): inside buffers of exactly the sizes rj_sizes gives
    for (int64_t count = 0; count <= 5; ++count) {
        const RjShape s{3, 2, 5, 2, {3, 4}, {3, 1}};
        EXPECT(rj_sizes(s, count, &r));
        for (int64_t br = -2; br <= 3; ++br) {
            if (!rj_branch_ok(s.nb, br) || br < 0) continue;
            std::vector<char> x((size_t)r.x[br]), in((size_t)r.inds[br]);
            const int64_t x1 = 2 * 5 * s.nl[br] * s.nd[br] * 8, i1 = 2 * 5 * s.nl[br];
            for (int64_t first = -1; first <= 7; ++first)
                for (int64_t n = -1; n <= 7; ++n) {
                    if (!range_ok(count, first, n)) continue;
                    for (int64_t k = first; k < first + n; ++k) { x[(size_t)(k * x1)] = 1; x[(size_t)((k + 1) * x1 - 1)] = 1; in[(size_t)(k * i1)] = 1; in[(size_t)((k + 1) * i1 - 1)] = 1; }
                }
        }
    }
    if (failures) return EXIT_FAILURE;
    std::puts("ok");
    return EXIT_SUCCESS;
}
