// rj_chain_stats_host_check.cpp - the launch arithmetic of a leaf-packing chain's diagnostics (eryn_amd/csrc/hens_chain_host.h:
// rj_stat_plan, rj_window_ok, rj_plain_plan) on its own, for a sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rj_chain_stats_host_check.cpp -o rj_chain_stats_host_check && ./rj_chain_stats_host_check
// Walks rj_stat_plan over the edges of its domain (branch, zero, one, 2^31 kept steps, products that pass 2^63) and, for a grid of
// ordinary shapes and ranges, replays every address k_rj_chain_leaves / k_rj_chain_leaf_moments form from an accepted plan - lane by
// lane, step by step, with the kernels' own index expressions - on host arrays of exactly the sizes rj_sizes gives the chain's buffers
// and of exactly the outputs' sizes, so that a plan that reaches outside them is an AddressSanitizer report; the LDS table's cells
// are replayed the same way.  Exit status 0 and "ok" = every expectation held.
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
    RjStatPlan p{};
    StatPlan q{};
    // config 4 (8 rungs x 2048 walkers, 2 branches of 10 leaves x 3 parameters), 400 stored steps, by hand
    const RjShape c4{8, 8, 2048, 2, {10, 10}, {3, 3}};
    EXPECT(rj_stat_plan(c4, 400, 1, 0, 400, 1, 8, &p) && p.inds_offset == 0 && p.inds_stride == 8LL * 2048 * 10 && p.x_stride == 8LL * 2048 * 30 &&
           p.nplaces == 8 * 2048 && p.nseries == 8 * 2048 * 3 && p.vec == 1 && p.lds_bytes == 11 * 256 * 4 && p.nl == 10 && p.nd == 3);
    EXPECT(rj_stat_plan(c4, 400, 0, 100, 100, 3, 2, &p) && p.inds_offset == 100LL * 8 * 2048 * 10 && p.x_offset == 100LL * 8 * 2048 * 30 &&
           p.inds_stride == 3LL * 8 * 2048 * 10 && p.nplaces == 2 * 2048);
    EXPECT(rj_stat_plan(c4, 400, 0, 1, 200, 2, 3, &p) && !rj_stat_plan(c4, 400, 0, 2, 200, 2, 3, &p));          // last kept step 399 / 400
    // load width: dwords only where every place starts on one
    EXPECT(rj_stat_plan(RjShape{4, 4, 10, 2, {3, 4}, {3, 3}}, 9, 0, 0, 9, 1, 4, &p) && p.vec == 1);
    EXPECT(rj_stat_plan(RjShape{4, 4, 10, 2, {3, 4}, {3, 3}}, 9, 1, 0, 9, 1, 4, &p) && p.vec == 4);
    EXPECT(rj_stat_plan(RjShape{4, 4, 10, 2, {32, 32}, {1, 2}}, 9, 1, 0, 9, 1, 4, &p) && p.vec == 4 && p.lds_bytes == 33 * 1024 && p.lds_bytes <= 64 * 1024);
    EXPECT(rj_stat_plan(RjShape{4, 4, 10, 1, {2}, {4}}, 9, 0, 0, 9, 1, 4, &p) && p.vec == 1);
    // not plans
    const RjShape s{4, 3, 5, 2, {3, 2}, {3, 1}};
    EXPECT(!rj_stat_plan(s, 9, -1, 0, 1, 1, 1, &p) && !rj_stat_plan(s, 9, 2, 0, 1, 1, 1, &p) && rj_stat_plan(s, 9, 1, 0, 1, 1, 1, &p));     // branch
    EXPECT(!rj_stat_plan(s, 9, 0, -1, 1, 1, 1, &p) && !rj_stat_plan(s, 9, 0, 9, 1, 1, 1, &p) && rj_stat_plan(s, 9, 0, 8, 1, 1, 1, &p));
    EXPECT(!rj_stat_plan(s, 9, 0, 0, 0, 1, 1, &p) && !rj_stat_plan(s, 9, 0, 0, -3, 1, 1, &p) && !rj_stat_plan(s, 9, 0, 0, 10, 1, 1, &p));
    EXPECT(!rj_stat_plan(s, 9, 0, 0, 1, 0, 1, &p) && !rj_stat_plan(s, 9, 0, 0, 1, -1, 1, &p));
    EXPECT(!rj_stat_plan(s, 9, 0, 0, 1, 1, 0, &p) && !rj_stat_plan(s, 9, 0, 0, 1, 1, 4, &p) && rj_stat_plan(s, 9, 0, 0, 1, 1, 3, &p));
    EXPECT(!rj_stat_plan(s, 0, 0, 0, 1, 1, 1, &p) && !rj_stat_plan(s, -1, 0, 0, 1, 1, 1, &p));                 // an empty chain keeps nothing
    EXPECT(!rj_stat_plan(RjShape{4, 5, 5, 1, {3}, {3}}, 9, 0, 0, 1, 1, 1, &p) && !rj_stat_plan(RjShape{4, 3, 0, 1, {3}, {3}}, 9, 0, 0, 1, 1, 1, &p));
    EXPECT(!rj_stat_plan(RjShape{4, 3, 5, 5, {3}, {3}}, 9, 0, 0, 1, 1, 1, &p) && !rj_stat_plan(RjShape{4, 3, 5, 1, {0}, {3}}, 9, 0, 0, 1, 1, 1, &p));
    EXPECT(!rj_stat_plan(RjShape{4, 3, 5, 1, {33}, {1}}, 9, 0, 0, 1, 1, 1, &p) && !rj_stat_plan(RjShape{4, 3, 5, 1, {3}, {5}}, 9, 0, 0, 1, 1, 1, &p));   // the table, the widths
    // 2^31 kept steps count, one more does not; beyond int64: refused, never wrapped
    const RjShape tiny{1, 1, 1, 1, {1}, {1}};
    EXPECT(rj_stat_plan(tiny, RJ_STAT_COUNT_MAX, 0, 0, RJ_STAT_COUNT_MAX, 1, 1, &p) && !rj_stat_plan(tiny, RJ_STAT_COUNT_MAX + 1, 0, 0, RJ_STAT_COUNT_MAX + 1, 1, 1, &p));
    EXPECT(!rj_stat_plan(s, 9, 0, 1, MAX, MAX, 1, &p) && !rj_stat_plan(s, 9, 0, MAX, 2, MAX, 1, &p) && !rj_stat_plan(s, 9, 0, 0, 2, MAX, 1, &p));
    EXPECT(rj_stat_plan(s, 9, 0, 8, 1, MAX, 1, &p) && p.inds_stride == 3 * 5 * 3 && p.x_stride == 3 * 5 * 9);   // one kept step: thin never multiplies
    EXPECT(!rj_stat_plan(s, MAX, 0, 0, 1, 1, 1, &p) && !rj_stat_plan(RjShape{MAX, MAX, MAX, 1, {3}, {3}}, 9, 0, 0, 1, 1, 1, &p));
    EXPECT(!rj_stat_plan(RjShape{4, 3, MAX / 2, 1, {3}, {3}}, 9, 0, 0, 1, 1, 1, &p) && !rj_stat_plan(s, 9, 0, INT64_MIN, 1, 1, 1, &p));
    // the ordinal window
    EXPECT(rj_window_ok(0, 1) && rj_window_ok(5, MAX) && !rj_window_ok(0, 0) && !rj_window_ok(3, 3) && !rj_window_ok(4, 3) && !rj_window_ok(-1, 3) && !rj_window_ok(INT64_MIN, MAX));
    // the chain as it lies: the fixed-dimension plan over this chain's arrays
    EXPECT(rj_plain_plan(s, 9, 0, 0, 0, 9, 1, 3, &q) && q.nseries == 3 * 5 * 9 && q.stride == 3 * 5 * 9 && q.vec == 1);
    EXPECT(rj_plain_plan(s, 9, 0, 1, 2, 3, 2, 2, &q) && q.nseries == 2 * 5 * 2 && q.offset == 2 * 3 * 5 * 2 && q.stride == 2 * 3 * 5 * 2 && q.vec == 2);
    EXPECT(rj_plain_plan(s, 9, 1, -7, 0, 9, 1, 3, &q) && q.nseries == 15 && rj_plain_plan(s, 9, 2, 0, 8, 1, 1, 1, &q) && q.offset == 8 * 15);   // (logl / logp: no branch)
    EXPECT(!rj_plain_plan(s, 9, 0, 2, 0, 9, 1, 3, &q) && !rj_plain_plan(s, 9, 0, -1, 0, 9, 1, 3, &q) && !rj_plain_plan(s, 9, 3, 0, 0, 9, 1, 3, &q) &&
           !rj_plain_plan(s, 9, -1, 0, 0, 9, 1, 3, &q) && !rj_plain_plan(s, 9, 0, 0, 0, 10, 1, 3, &q) && !rj_plain_plan(s, 9, 1, 0, 0, 9, 1, 4, &q));

    // every address of an accepted plan: inside buffers of exactly rj_sizes' bytes, inside outputs of exactly their size
    const RjShape shapes[] = {RjShape{4, 4, 10, 2, {3, 4}, {3, 3}}, RjShape{4, 2, 33, 4, {3, 2, 2, 2}, {1, 2, 3, 4}}, RjShape{3, 3, 70, 2, {32, 32}, {1, 2}},
                              RjShape{2, 1, 3, 1, {1}, {3}}, RjShape{5, 5, 130, 1, {8}, {4}}};
    for (const RjShape& sh : shapes)
        for (int64_t stored : {(int64_t)1, (int64_t)6, (int64_t)13}) {
            RjSizes sz{};
            EXPECT(rj_sizes(sh, stored, &sz));
            for (int64_t b = 0; b < sh.nb; ++b) {
                const int64_t nl = sh.nl[b], nd = sh.nd[b];
                std::vector<uint8_t> inds((size_t)sz.inds[b], 1);                  // every leaf in use: every coordinate address is formed
                std::vector<double> x((size_t)(sz.x[b] / 8), 0.0);
                EXPECT(sz.x[b] % 8 == 0);
                for (int64_t first = -1; first <= stored; ++first)
                    for (int64_t count = 0; count <= stored + 1; ++count)
                        for (int64_t thin = 0; thin <= 3; ++thin)
                            for (int64_t nt = 0; nt <= sh.Ts + 1; ++nt) {
                                if (!rj_stat_plan(sh, stored, b, first, count, thin, nt, &p)) {
                                    const bool fine = first >= 0 && count >= 1 && thin >= 1 && nt >= 1 && nt <= sh.Ts && first + (count - 1) * thin < stored;
                                    EXPECT(!fine);
                                    continue;
                                }
                                EXPECT(first + (count - 1) * thin < stored && p.nplaces == nt * sh.W && p.nseries == p.nplaces * nd && p.nl == nl && p.nd == nd);
                                EXPECT(p.vec == 1 || (p.vec == 4 && nl % 4 == 0 && p.inds_offset % 4 == 0 && p.inds_stride % 4 == 0));
                                const uint8_t* pi = inds.data() + p.inds_offset;
                                const double* px = x.data() + p.x_offset;
                                const int64_t step_a = 0, step_b = count - 1;                  // (the first and the last kept step bound the others)
                                // k_rj_chain_leaves: whole workgroups of RJ_STAT_LANES lanes, lane = place
                                std::vector<uint8_t> nleaves((size_t)(count * p.nplaces), 0);
                                std::vector<uint32_t> hist((size_t)(p.nplaces * (nl + 1)), 0);
                                std::vector<uint32_t> tab((size_t)(p.lds_bytes / 4), 0);
                                const int64_t lanes = stat_blocks(p.nplaces, RJ_STAT_LANES) * RJ_STAT_LANES;
                                for (int64_t g = 0; g < lanes; ++g) {
                                    const int64_t i = g, tid = g % RJ_STAT_LANES;
                                    if (i >= p.nplaces) continue;
                                    for (int64_t j : {step_a, step_b}) {
                                        int c = 0;
                                        const uint8_t* m = pi + i * nl + j * p.inds_stride;
                                        if (p.vec == 4) {
                                            EXPECT((p.inds_offset + i * nl + j * p.inds_stride) % 4 == 0);     // (the buffer's base is aligned on the device)
                                            for (int64_t w = 0; w < nl / 4; ++w) c += m[4 * w] + m[4 * w + 1] + m[4 * w + 2] + m[4 * w + 3];
                                        } else {
                                            for (int64_t n = 0; n < nl; ++n) c += m[n];
                                        }
                                        EXPECT(c == nl);
                                        tab[(size_t)(c * RJ_STAT_LANES + tid)] += 1;
                                        nleaves[(size_t)(j * p.nplaces + i)] += 1;
                                    }
                                    for (int64_t k = 0; k <= nl; ++k) hist[(size_t)(i * (nl + 1) + k)] += 1;
                                }
                                for (uint32_t h : hist) EXPECT(h == 1);                          // every bin written exactly once
                                for (int64_t i = 0; i < p.nplaces; ++i) EXPECT(nleaves[(size_t)i] >= 1 && nleaves[(size_t)(step_b * p.nplaces + i)] >= 1);
                                // k_rj_chain_leaf_moments: lane = series (place, parameter)
                                std::vector<char> sum((size_t)p.nseries, 0), n_out((size_t)p.nplaces, 0);
                                const int64_t lanes2 = stat_blocks(p.nseries, RJ_STAT_LANES) * RJ_STAT_LANES;
                                for (int64_t i = 0; i < lanes2; ++i) {
                                    if (i >= p.nplaces * nd) continue;
                                    const int64_t place = i / nd, d = i - place * nd;
                                    const double* q0 = px + place * nl * nd + d;
                                    for (int64_t j : {step_a, step_b})
                                        for (int64_t slot = 0; slot < nl; ++slot) EXPECT(q0[j * p.x_stride + slot * nd] == 0.0);
                                    EXPECT(pi[place * nl + step_b * p.inds_stride + nl - 1] == 1);
                                    sum[(size_t)i] += 1;
                                    if (d == 0) n_out[(size_t)place] += 1;
                                }
                                for (char c : sum) EXPECT(c == 1);
                                for (char c : n_out) EXPECT(c == 1);
                            }
            }
        }
    if (failures) return EXIT_FAILURE;
    std::puts("ok");
    return EXIT_SUCCESS;
}
