// hens_prior_host.h - one parameter's prior term: the record the kernels read (PriorTerm; prior_term / prior_sum: hens_kernels.h) and
// the host's reading of a caller's kind / lo / hi / c0 / c1 / c2 into it, as plain host functions without HIP types.  BOTH entry
// points that take prior terms (hens_set_prior_terms: the row of a stepping context; hens_rj_set_prior_terms: the leaf parameters of a
// leaf-packing model) parse every term with parse_term and fold the parsed run with fold_box; hens.hip keeps their state checks,
// uploads and the place it appends to a refusal.  tools/prior_host_check.cpp runs the two functions alone under
// -fsanitize=address,undefined.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdio>

namespace hens {

// the kinds are include/hipensemble.h's HENS_PRIOR_* (hens.hip asserts it); NONE is no caller's: the pad of a padded row
constexpr int PRIOR_UNIFORM = 0, PRIOR_LOG_UNIFORM = 1, PRIOR_NORMAL = 2, PRIOR_NONE = 3;
struct PriorTerm {
    double c0;       // UNIFORM: log(1/(hi - lo));  LOG_UNIFORM: log(log(b) - log(a));  NORMAL: loc
    double c1;       // NORMAL: scale
    double c2;       // NORMAL: log(scale)
    int32_t kind, pad_;
};
static_assert(sizeof(PriorTerm) == 32, "PriorTerm: four doubles' worth");

struct ParsedTerm {
    PriorTerm term;      // all zero on a refusal
    char why[96];        // "": accepted; else the reason, without the place (the entry point appends its own)
};

// One parameter's term.  `admit_pad`: the caller's rows may be padded (hens_config::ndim_active), and a uniform term on
// (-inf, +inf) is a pad - PRIOR_NONE, no term, its c0 not read; a caller without pads (the leaves of a record: a leaf is born from
// its prior, distgenrj.py:188-214) gets a uniform term on finite bounds or a refusal.  That is the one difference between the two
// callers that is meant.  The place of the c0 rule is the other, and is history: a pad's c0 must not be looked at, so the row's
// caller has always reported c0 behind the kind's own rule, the leaves' caller in front of it; both orders are kept, so each entry
// point names first what it named first before this header.
inline ParsedTerm parse_term(int32_t kind, double lo, double hi, double c0, double c1, double c2, bool admit_pad) {
    ParsedTerm p{};
    auto finite = [](double v) { return std::fabs(v) < INFINITY; };
    auto refuse = [&p](const char* why) { std::snprintf(p.why, sizeof(p.why), "%s", why); return p; };
    if (kind != PRIOR_UNIFORM && kind != PRIOR_LOG_UNIFORM && kind != PRIOR_NORMAL) {
        std::snprintf(p.why, sizeof(p.why), "unknown prior kind %d", (int)kind);
        return p;
    }
    if (!(lo < hi)) return refuse("prior terms need lo < hi in every dimension");
    if (admit_pad && kind == PRIOR_UNIFORM && lo == -INFINITY && hi == INFINITY) {
        p.term.kind = PRIOR_NONE;
        return p;
    }
    const char* own = nullptr;       // the kind's own rule on its bounds / scale
    if (kind == PRIOR_UNIFORM && !admit_pad && (!finite(lo) || !finite(hi))) own = "uniform prior term needs finite bounds";
    if (kind == PRIOR_LOG_UNIFORM && (!(lo > 0.0) || !(hi < INFINITY))) own = "log-uniform prior term needs 0 < lo < hi < inf";
    if (kind == PRIOR_NORMAL && (!(c1 > 0.0) || !(c1 < INFINITY))) own = "normal prior term needs a finite scale > 0";
    if (own && admit_pad) return refuse(own);
    if (!finite(c0)) return refuse(kind == PRIOR_NORMAL ? "normal prior term: loc (c0) must be finite" : "prior term: c0 must be finite");
    if (own) return refuse(own);
    if (kind == PRIOR_NORMAL && !finite(c2)) return refuse("normal prior term: log(scale) must be finite");
    p.term.kind = kind;
    p.term.c0 = c0;
    if (kind == PRIOR_NORMAL) { p.term.c1 = c1; p.term.c2 = c2; }
    return p;
}

// A run of parsed terms as a box: `box` while every term is uniform (or a pad), `logp` the constant log-density inside it -
// ((0.0 + c0_0) + c0_1) + ... over the uniform terms, ascending (prior.py:364-383: prior_vals += temp), pads skipped.  `logp` is
// that sum over the run's uniform terms whether or not the run is a box.
struct PriorBox { bool box; double logp; };
inline PriorBox fold_box(const PriorTerm* terms, int n) {
    PriorBox b{true, 0.0};
    for (int d = 0; d < n; ++d) {
        if (terms[d].kind == PRIOR_UNIFORM) b.logp += terms[d].c0;
        else if (terms[d].kind != PRIOR_NONE) b.box = false;
    }
    return b;
}

}  // namespace hens
