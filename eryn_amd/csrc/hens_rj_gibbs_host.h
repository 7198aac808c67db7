// hens_rj_gibbs_host.h - the Gibbs block table of the in-model Gaussian move on leaf-packing records (hens_rj_set_gibbs; move.py:113-221
// over branches and leaf slots): the host's reading of a caller's mask[nblocks][ind_off], as plain host functions without HIP types,
// in the style of hens_gibbs_host.h.  hens.hip keeps the state checks, the upload and the place it appends to a refusal;
// tools/rj_gibbs_host_check.cpp runs these functions alone under -fsanitize=address,undefined.
#pragma once
#include <cstdint>
#include <cstdio>
#include <vector>

namespace hens {

constexpr int RJ_GIBBS_HOST_MAX_BLOCKS = 128;      // (= RJ_GIBBS_MAX_BLOCKS of hens_rj_gibbs.h: the block index has 7 bits in the draws' keys)

struct ParsedRjGibbs {
    std::vector<uint8_t> table;   // [nblocks][ind_off] 0 / 1, as k_rj_gibbs reads it
    std::vector<int32_t> n;       // [nblocks] true coordinates of every block
    bool whole = false;           // exactly one block with every coordinate true: the move of a context without a table
    char why[96];                 // "": accepted; else the reason, without the place
};

// mask: [nblocks][ind_off] bytes in record layout (branch after branch, slot after slot, the slot's parameters), non-zero = the
// coordinate moves with the block.  Blocks may overlap and need not cover every coordinate; a block without a true coordinate is
// refused (the reference would skip it at every iteration).  nblocks == 0: the empty table (clears).
inline ParsedRjGibbs parse_rj_gibbs(int nblocks, const uint8_t* mask, int ind_off) {
    ParsedRjGibbs p{};
    p.why[0] = 0;
    auto refuse = [&p](const char* fmt, int a) { std::snprintf(p.why, sizeof(p.why), fmt, a); p.table.clear(); p.n.clear(); p.whole = false; };
    if (nblocks < 0) { refuse("nblocks must be >= 0 (%d)", nblocks); return p; }
    if (nblocks > RJ_GIBBS_HOST_MAX_BLOCKS) { refuse("at most 128 Gibbs blocks (%d)", nblocks); return p; }
    if (nblocks > 0 && !mask) { refuse("null mask", 0); return p; }
    if (nblocks > 0 && ind_off < 1) { refuse("a record without coordinates (%d)", ind_off); return p; }
    p.table.assign((size_t)nblocks * (size_t)ind_off, 0);
    p.n.assign((size_t)nblocks, 0);
    for (int b = 0; b < nblocks; ++b) {
        for (int i = 0; i < ind_off; ++i)
            if (mask[(size_t)b * ind_off + i]) { p.table[(size_t)b * ind_off + i] = 1; p.n[(size_t)b] += 1; }
        if (p.n[(size_t)b] == 0) { refuse("block %d has no true coordinate", b); return p; }
    }
    p.whole = nblocks == 1 && p.n[0] == ind_off;
    return p;
}

}  // namespace hens
