// hens_gibbs_host.h - the Gibbs block table of one move (hens_set_gibbs; move.py:113-221 for one branch, nleaves_max == 1): the host's
// reading of a caller's mask[nblocks][D] and the device image of one block, as plain host functions without HIP types, in the
// style of hens_prior_host.h.  hens.hip keeps the state checks, the upload and the place it appends to a refusal;
// tools/gibbs_host_check.cpp runs these functions alone under -fsanitize=address,undefined.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "hens_prior_host.h"

namespace hens {

constexpr int GIBBS_MAX_BLOCKS = 128;

struct ParsedGibbs {
    std::vector<int32_t> n;       // [nblocks] true coordinates of every block (the Hastings factor's dimension, stretch.py:55-72)
    std::vector<int32_t> mask;    // [nblocks][D] 0 / 1, as the device reads it
    char why[96];                 // "": accepted; else the reason, without the place
};

// mask: [nblocks][D] bytes, non-zero = the coordinate moves with the block; D the context's row width, Da its real parameters
// (hens_config::ndim_active: coordinates from Da on are pads, always frozen - a true pad is refused).  Blocks may overlap and
// need not cover every coordinate; a block without a true coordinate is refused (the reference skips it silently).
inline ParsedGibbs parse_gibbs(int nblocks, const uint8_t* mask, int D, int Da) {
    ParsedGibbs p{};
    p.why[0] = 0;
    auto refuse = [&p](const char* fmt, int a, int b) { std::snprintf(p.why, sizeof(p.why), fmt, a, b); p.n.clear(); p.mask.clear(); };
    if (nblocks < 0) { refuse("nblocks must be >= 0 (%d)", nblocks, 0); return p; }
    if (nblocks > GIBBS_MAX_BLOCKS) { refuse("at most %d Gibbs blocks (%d)", GIBBS_MAX_BLOCKS, nblocks); return p; }
    if (nblocks > 0 && !mask) { refuse("null mask", 0, 0); return p; }
    p.n.assign((size_t)nblocks, 0);
    p.mask.assign((size_t)nblocks * D, 0);
    for (int b = 0; b < nblocks; ++b) {
        for (int d = 0; d < D; ++d) {
            if (!mask[(size_t)b * D + d]) continue;
            if (d >= Da) { refuse("block %d moves coordinate %d, a pad of the row", b, d); return p; }
            p.mask[(size_t)b * D + d] = 1;
            p.n[(size_t)b] += 1;
        }
        if (p.n[(size_t)b] == 0) { refuse("block %d has no true coordinate", b, 0); return p; }
    }
    return p;
}

// A plain box as terms the term tile can add: the box's constant on coordinate 0, 0.0 on the other real coordinates, no term on a
// pad - term_sum's ((0.0 + logp_in) + 0.0) + ... is logp_in bit for bit (x + 0.0 == x for every x but -0.0, which compares equal).
inline void box_as_terms(double logp_in, int D, int Da, PriorTerm* out) {
    for (int d = 0; d < D; ++d) {
        out[d] = PriorTerm{};
        out[d].kind = d < Da ? PRIOR_UNIFORM : PRIOR_NONE;
        if (d == 0) out[d].c0 = logp_in;
    }
}

// One block's device image: lo[D] hi[D] terms[D] mask[D], the form StretchArgs::lo / hi address with prior_on == 2
// (prior_terms_of, gibbs_mask_of).  D even: mask[D] int32 is D / 2 doubles, and every image starts 16-byte aligned.
inline size_t gibbs_image_doubles(int D) { return (size_t)6 * D + (size_t)D / 2; }
inline void gibbs_image(const double* lo, const double* hi, const PriorTerm* terms, const int32_t* mask, int D, double* out) {
    std::memcpy(out, lo, (size_t)D * 8);
    std::memcpy(out + D, hi, (size_t)D * 8);
    std::memcpy(out + 2 * (size_t)D, terms, (size_t)D * sizeof(PriorTerm));
    std::memcpy(out + 6 * (size_t)D, mask, (size_t)D * 4);
}

}  // namespace hens
