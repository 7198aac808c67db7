// gibbs_host_check.cpp - the parser of a caller's Gibbs block table and the device image of one block
// (eryn_amd/csrc/hens_gibbs_host.h: parse_gibbs, box_as_terms, gibbs_image) on their own, for a sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/gibbs_host_check.cpp -o gibbs_host_check && ./gibbs_host_check
// (tests/test_gibbs_move.py::test_mask_parser_and_block_image_under_a_sanitizer_build builds and runs it so.)
// Every refusal of the parser with its reason (the texts tests/test_hip_gibbs.py expects behind "hens_set_gibbs: "), accepted tables
// - overlapping blocks, a coordinate in no block, pads - with their counts and masks, the box as terms (its sum in term_sum's order
// is the box's constant, bit for bit) and an image compared byte for byte.  Exit status 0 and "ok" = every expectation held.
#include "../eryn_amd/csrc/hens_gibbs_host.h"

#include <cstdlib>
#include <limits>
#include <string>

using namespace hens;

static int failures = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const double INF = std::numeric_limits<double>::infinity();

static std::string why_of(int nblocks, const uint8_t* mask, int D, int Da) { return parse_gibbs(nblocks, mask, D, Da).why; }

int main() {
    // ---- refusals
    const int D = 8, Da = 5;
    std::vector<uint8_t> two = {1, 1, 0, 0, 0, 0, 0, 0, /**/ 0, 0, 1, 0, 0, 0, 0, 0};
    EXPECT(why_of(-1, two.data(), D, Da) == "nblocks must be >= 0 (-1)");
    EXPECT(why_of(129, two.data(), D, Da) == "at most 128 Gibbs blocks (129)");
    EXPECT(why_of(2, nullptr, D, Da) == "null mask");
    std::vector<uint8_t> empty1 = two;
    empty1[10] = 0;
    EXPECT(why_of(2, empty1.data(), D, Da) == "block 1 has no true coordinate");
    std::vector<uint8_t> pad = two;
    pad[8 + 5] = 1;
    EXPECT(why_of(2, pad.data(), D, Da) == "block 1 moves coordinate 5, a pad of the row");
    {
        const ParsedGibbs p = parse_gibbs(2, pad.data(), D, Da);      // a refusal leaves nothing behind
        EXPECT(p.n.empty() && p.mask.empty());
    }
    // ---- accepted: nblocks == 0, overlapping blocks, a coordinate in no block, any non-zero byte is true, 128 blocks
    {
        const ParsedGibbs p = parse_gibbs(0, nullptr, D, Da);
        EXPECT(p.why[0] == 0 && p.n.empty() && p.mask.empty());
    }
    {
        std::vector<uint8_t> m = {1, 200, 1, 0, 0, 0, 0, 0, /**/ 0, 0, 1, 1, 0, 0, 0, 0};      // coordinate 4 in no block
        const ParsedGibbs p = parse_gibbs(2, m.data(), D, Da);
        EXPECT(p.why[0] == 0 && p.n.size() == 2 && p.n[0] == 3 && p.n[1] == 2 && p.mask.size() == 16);
        const int32_t want[16] = {1, 1, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 0, 0, 0};
        EXPECT(std::memcmp(p.mask.data(), want, sizeof want) == 0);
    }
    {
        std::vector<uint8_t> m((size_t)128 * D, 0);
        for (int b = 0; b < 128; ++b) m[(size_t)b * D + b % Da] = 1;
        const ParsedGibbs p = parse_gibbs(128, m.data(), D, Da);
        EXPECT(p.why[0] == 0 && p.n.size() == 128);
        for (int b = 0; b < 128; ++b) EXPECT(p.n[(size_t)b] == 1 && p.mask[(size_t)b * D + b % Da] == 1);
    }
    {
        std::vector<uint8_t> m((size_t)D, 1);                          // no pads: every coordinate may move
        const ParsedGibbs p = parse_gibbs(1, m.data(), D, D);
        EXPECT(p.why[0] == 0 && p.n[0] == D);
    }
    // ---- the box as terms: term_sum's sum (ascending from 0.0, pads skipped) is the constant, bit for bit
    for (const double c : {-13.862943611198906, 0.0, 1e-300, -7.25e17, 3.0}) {
        PriorTerm t[8];
        box_as_terms(c, D, Da, t);
        double acc = 0.0;
        for (int d = 0; d < D; ++d)
            if (t[d].kind != PRIOR_NONE) acc += t[d].c0;
        EXPECT(std::memcmp(&acc, &c, 8) == 0);
        for (int d = 0; d < D; ++d) EXPECT(t[d].kind == (d < Da ? PRIOR_UNIFORM : PRIOR_NONE) && t[d].c1 == 0.0 && t[d].c2 == 0.0 && t[d].pad_ == 0);
    }
    // ---- one image, byte for byte: lo[D] hi[D] terms[D] mask[D]
    {
        double lo[8], hi[8];
        PriorTerm t[8];
        int32_t mask[8] = {0, 1, 0, 1, 1, 0, 0, 0};
        for (int d = 0; d < D; ++d) { lo[d] = d < Da ? -1.0 - d : -INF; hi[d] = d < Da ? 2.0 + d : INF; }
        box_as_terms(-2.5, D, Da, t);
        EXPECT(gibbs_image_doubles(D) == 52 && gibbs_image_doubles(128) == 832 && (gibbs_image_doubles(D) * 8) % 16 == 0);
        std::vector<double> img(gibbs_image_doubles(D) + 1, 777.0);
        gibbs_image(lo, hi, t, mask, D, img.data());
        EXPECT(std::memcmp(img.data(), lo, 64) == 0 && std::memcmp(img.data() + 8, hi, 64) == 0);
        EXPECT(std::memcmp(img.data() + 16, t, sizeof t) == 0 && std::memcmp(img.data() + 48, mask, sizeof mask) == 0);
        EXPECT(img[52] == 777.0);                                      // nothing behind the image is written
        const PriorTerm* back = reinterpret_cast<const PriorTerm*>(img.data() + 2 * D);      // the device's reading (prior_terms_of, gibbs_mask_of)
        const int32_t* mback = reinterpret_cast<const int32_t*>(back + D);
        EXPECT(back[0].c0 == -2.5 && back[7].kind == PRIOR_NONE && mback[1] == 1 && mback[2] == 0 && mback[4] == 1);
    }
    if (failures) { std::printf("%d expectation(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
