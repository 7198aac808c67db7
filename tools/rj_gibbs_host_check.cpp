// rj_gibbs_host_check.cpp - the parser of a caller's Gibbs block table over a leaf-packing record
// (eryn_amd/csrc/hens_rj_gibbs_host.h: parse_rj_gibbs) on its own, for a sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/rj_gibbs_host_check.cpp -o rj_gibbs_host_check && ./rj_gibbs_host_check
// (tests/test_rj_gibbs_move.py::test_table_parser_under_a_sanitizer_build builds and runs it so.)
// Every refusal of the parser with its reason (the texts tests/test_hip_rj_gibbs.py expects behind "hens_rj_set_gibbs: "), accepted
// tables - overlapping blocks, a coordinate in no block, any non-zero byte, 128 blocks, the whole-record block - byte for byte.
// Exit status 0 and "ok" = every expectation held.
#include "../eryn_amd/csrc/hens_rj_gibbs_host.h"

#include <cstring>
#include <string>

using namespace hens;

static int failures = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static std::string why_of(int nblocks, const uint8_t* mask, int io) { return parse_rj_gibbs(nblocks, mask, io).why; }

int main() {
    const int IO = 6;                                  // (two slots of three parameters)
    std::vector<uint8_t> two = {1, 1, 0, 0, 0, 0, /**/ 0, 0, 0, 1, 1, 1};
    // ---- refusals
    EXPECT(why_of(-1, two.data(), IO) == "nblocks must be >= 0 (-1)");
    EXPECT(why_of(129, two.data(), IO) == "at most 128 Gibbs blocks (129)");
    EXPECT(why_of(2, nullptr, IO) == "null mask");
    EXPECT(why_of(1, two.data(), 0) == "a record without coordinates (0)");
    std::vector<uint8_t> empty1 = two;
    empty1[9] = empty1[10] = empty1[11] = 0;
    EXPECT(why_of(2, empty1.data(), IO) == "block 1 has no true coordinate");
    {
        const ParsedRjGibbs p = parse_rj_gibbs(2, empty1.data(), IO);      // a refusal leaves nothing behind
        EXPECT(p.table.empty() && p.n.empty() && !p.whole);
    }
    // ---- accepted
    {
        const ParsedRjGibbs p = parse_rj_gibbs(0, nullptr, IO);
        EXPECT(p.why[0] == 0 && p.table.empty() && p.n.empty() && !p.whole);
    }
    {
        std::vector<uint8_t> m = {1, 200, 1, 0, 0, 0, /**/ 0, 0, 1, 1, 0, 0};      // overlap on coordinate 2, coordinates 4 and 5 in no block
        const ParsedRjGibbs p = parse_rj_gibbs(2, m.data(), IO);
        const uint8_t want[12] = {1, 1, 1, 0, 0, 0, 0, 0, 1, 1, 0, 0};
        EXPECT(p.why[0] == 0 && p.n.size() == 2 && p.n[0] == 3 && p.n[1] == 2 && p.table.size() == 12 && !p.whole);
        EXPECT(std::memcmp(p.table.data(), want, sizeof want) == 0);
    }
    {
        std::vector<uint8_t> m((size_t)128 * IO, 0);
        for (int b = 0; b < 128; ++b) m[(size_t)b * IO + b % IO] = 1;
        const ParsedRjGibbs p = parse_rj_gibbs(128, m.data(), IO);
        EXPECT(p.why[0] == 0 && p.n.size() == 128 && p.table.size() == (size_t)128 * IO && !p.whole);
        for (int b = 0; b < 128; ++b) EXPECT(p.n[(size_t)b] == 1 && p.table[(size_t)b * IO + b % IO] == 1);
        EXPECT(std::memcmp(p.table.data(), m.data(), m.size()) == 0);
    }
    {
        std::vector<uint8_t> m((size_t)IO, 7);                              // the whole record in one block
        const ParsedRjGibbs p = parse_rj_gibbs(1, m.data(), IO);
        EXPECT(p.why[0] == 0 && p.whole && p.n[0] == IO);
        std::vector<uint8_t> twice((size_t)2 * IO, 1);                      // ... twice: two moves per iteration, not the plain one
        EXPECT(!parse_rj_gibbs(2, twice.data(), IO).whole);
        m[3] = 0;
        EXPECT(!parse_rj_gibbs(1, m.data(), IO).whole);
    }
    {
        std::vector<uint8_t> m((size_t)128, 1);                             // the widest record
        const ParsedRjGibbs p = parse_rj_gibbs(1, m.data(), 126);
        EXPECT(p.why[0] == 0 && p.table.size() == 126 && p.whole);
    }
    if (failures) { std::printf("%d expectation(s) failed\n", failures); return 1; }
    std::printf("ok\n");
    return 0;
}
