// prior_host_check.cpp - the one parser of a caller's prior term and the fold of a parsed run into a box
// (eryn_amd/csrc/hens_prior_host.h: parse_term, fold_box) on their own, for a sanitizer build on the host:
//     c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/prior_host_check.cpp -o prior_host_check && ./prior_host_check
// (tests/test_prior_terms.py::test_term_parser_and_box_fold_under_a_sanitizer_build builds and runs it so.)
// A table per mode - pads admitted (hens_set_prior_terms) and not (hens_rj_set_prior_terms): every refusal the GPU tests of the two
// entry points list (tests/test_hip_priors.py: the `bad` table; tests/test_hip_rj_priors.py: test_refusals_leave_the_context_as_it_was)
// with its reason, terms with two faults (which one each entry point names first), and one accepted term of each kind, whose record
// is compared byte for byte.  Then the fold: the order of the sum, pads, and a run that is no box.  Exit status 0 and "ok" = every
// expectation held.
#include "../eryn_amd/csrc/hens_prior_host.h"

#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <limits>

using namespace hens;

static int failures = 0;
#define EXPECT(cond)                                                                  \
    do {                                                                              \
        if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); ++failures; } \
    } while (0)

static const double INF = std::numeric_limits<double>::infinity(), NaN = std::numeric_limits<double>::quiet_NaN();

struct Case {
    const char* what;
    int32_t kind;
    double lo, hi, c0, c1, c2;
    const char* why[2];      // [0]: pads admitted, [1]: not; nullptr: accepted
    PriorTerm want[2];       // the record of an accepted term
};

// the tests' terms: log-uniform on [1, 6], normal(5, 2), uniform on [-1, 1]
static const double LU0 = std::log(std::log(6.0) - std::log(1.0)), LS = std::log(2.0), U0 = std::log(1 / 2.0);
static const char* const LOHI = "prior terms need lo < hi in every dimension";
static const char* const C0 = "prior term: c0 must be finite";
static const char* const LOC = "normal prior term: loc (c0) must be finite";
static const char* const SCALE = "normal prior term needs a finite scale > 0";
static const char* const LOGSCALE = "normal prior term: log(scale) must be finite";
static const char* const LUB = "log-uniform prior term needs 0 < lo < hi < inf";
static const char* const UB = "uniform prior term needs finite bounds";

static const Case CASES[] = {
    // accepted, one of each kind: the same record in both modes
    {"uniform", 0, -1.0, 1.0, U0, 7.0, 8.0, {nullptr, nullptr}, {{U0, 0.0, 0.0, PRIOR_UNIFORM, 0}, {U0, 0.0, 0.0, PRIOR_UNIFORM, 0}}},
    {"log-uniform", 1, 1.0, 6.0, LU0, 7.0, 8.0, {nullptr, nullptr}, {{LU0, 0.0, 0.0, PRIOR_LOG_UNIFORM, 0}, {LU0, 0.0, 0.0, PRIOR_LOG_UNIFORM, 0}}},
    {"normal", 2, -INF, INF, 5.0, 2.0, LS, {nullptr, nullptr}, {{5.0, 2.0, LS, PRIOR_NORMAL, 0}, {5.0, 2.0, LS, PRIOR_NORMAL, 0}}},
    {"normal on a finite support", 2, -3.0, 4.0, -0.0, 2.0, LS, {nullptr, nullptr}, {{-0.0, 2.0, LS, PRIOR_NORMAL, 0}, {-0.0, 2.0, LS, PRIOR_NORMAL, 0}}},
    // the pad: no term where pads are admitted (c0 not read), refused where not
    {"pad", 0, -INF, INF, 3.0, 0.0, 0.0, {nullptr, UB}, {{0.0, 0.0, 0.0, PRIOR_NONE, 0}, {}}},
    {"pad, c0 not read", 0, -INF, INF, NaN, NaN, NaN, {nullptr, C0}, {{0.0, 0.0, 0.0, PRIOR_NONE, 0}, {}}},
    {"half-open uniform", 0, -INF, 1.0, 0.5, 0.0, 0.0, {nullptr, UB}, {{0.5, 0.0, 0.0, PRIOR_UNIFORM, 0}, {}}},
    {"half-open uniform, its constant", 0, 0.0, INF, -INF, 0.0, 0.0, {C0, C0}, {}},
    // tests/test_hip_priors.py, `bad`
    {"lo >= hi", 1, 1.0, 1.0, LU0, 0.0, 0.0, {LOHI, LOHI}, {}},
    {"a <= 0", 1, 0.0, 6.0, LU0, 0.0, 0.0, {LUB, LUB}, {}},
    {"scale <= 0", 2, -INF, INF, 5.0, 0.0, LS, {SCALE, SCALE}, {}},
    {"non-finite constant", 1, 1.0, 6.0, INF, 0.0, 0.0, {C0, C0}, {}},
    {"non-finite log scale", 2, -INF, INF, 5.0, 2.0, NaN, {LOGSCALE, LOGSCALE}, {}},
    {"unknown kind", 7, -1.0, 1.0, U0, 0.0, 0.0, {"unknown prior kind 7", "unknown prior kind 7"}, {}},
    // tests/test_hip_rj_priors.py, `refused`
    {"NaN loc", 2, -INF, INF, NaN, 2.0, LS, {LOC, LOC}, {}},
    {"negative scale", 2, -INF, INF, 5.0, -1.0, LS, {SCALE, SCALE}, {}},
    {"log-uniform to inf", 1, 1.0, INF, LU0, 0.0, 0.0, {LUB, LUB}, {}},
    {"empty support", 0, -1.0, -1.0, U0, 0.0, 0.0, {LOHI, LOHI}, {}},
    // further edges of the same rules
    {"negative kind", -1, -1.0, 1.0, U0, 0.0, 0.0, {"unknown prior kind -1", "unknown prior kind -1"}, {}},
    {"the pad's kind is no caller's", 3, -INF, INF, 0.0, 0.0, 0.0, {"unknown prior kind 3", "unknown prior kind 3"}, {}},
    {"NaN bound", 0, NaN, 1.0, U0, 0.0, 0.0, {LOHI, LOHI}, {}},
    {"reversed bounds", 2, 1.0, -1.0, 5.0, 2.0, LS, {LOHI, LOHI}, {}},
    {"uniform, NaN constant", 0, -1.0, 1.0, NaN, 0.0, 0.0, {C0, C0}, {}},
    {"infinite scale", 2, -INF, INF, 5.0, INF, LS, {SCALE, SCALE}, {}},
    {"NaN scale", 2, -INF, INF, 5.0, NaN, LS, {SCALE, SCALE}, {}},
    {"negative a", 1, -2.0, 6.0, LU0, 0.0, 0.0, {LUB, LUB}, {}},
    // two faults: the row's entry point names the kind's own rule first, the leaves' the constant
    {"a <= 0 and a non-finite constant", 1, 0.0, 6.0, INF, 0.0, 0.0, {LUB, C0}, {}},
    {"scale 0 and a NaN loc", 2, -INF, INF, NaN, 0.0, LS, {SCALE, LOC}, {}},
    {"NaN loc and NaN log scale", 2, -INF, INF, NaN, 2.0, NaN, {LOC, LOC}, {}},
    {"scale 0 and NaN log scale", 2, -INF, INF, 5.0, 0.0, NaN, {SCALE, SCALE}, {}},
    {"unknown kind and lo >= hi", 9, 1.0, 1.0, NaN, 0.0, 0.0, {"unknown prior kind 9", "unknown prior kind 9"}, {}},
    {"lo >= hi and a non-finite constant", 0, 2.0, 1.0, NaN, 0.0, 0.0, {LOHI, LOHI}, {}},
};

int main() {
    static const PriorTerm zero{};
    int accepted[2][4] = {};
    for (const Case& k : CASES)
        for (int mode = 0; mode < 2; ++mode) {
            const ParsedTerm p = parse_term(k.kind, k.lo, k.hi, k.c0, k.c1, k.c2, mode == 0);
            bool ok;
            if (k.why[mode]) ok = std::strcmp(p.why, k.why[mode]) == 0 && std::memcmp(&p.term, &zero, sizeof(PriorTerm)) == 0;
            else ok = p.why[0] == 0 && std::memcmp(&p.term, &k.want[mode], sizeof(PriorTerm)) == 0 && ++accepted[mode][p.term.kind];
            if (!ok) { std::printf("FAILED '%s' (%s): got '%s', kind %d\n", k.what, mode == 0 ? "pads admitted" : "no pads", p.why, (int)p.term.kind); ++failures; }
            EXPECT(std::strlen(p.why) < sizeof(p.why) - 1);
        }
    for (int kind = 0; kind < 3; ++kind) EXPECT(accepted[0][kind] >= 1 && accepted[1][kind] >= 1);      // one accepted term of each kind per mode
    EXPECT(accepted[0][PRIOR_NONE] == 2 && accepted[1][PRIOR_NONE] == 0);

    // ---- fold_box ----
    auto uni = [](double c0) { return PriorTerm{c0, 0.0, 0.0, PRIOR_UNIFORM, 0}; };
    // ((0.0 + 1e16) + 1) + 1 = 1e16: ascending; any other order gives 1e16 + 2
    const PriorTerm asc[3] = {uni(1e16), uni(1.0), uni(1.0)}, desc[3] = {uni(1.0), uni(1.0), uni(1e16)};
    PriorBox b = fold_box(asc, 3);
    EXPECT(b.box && b.logp == 1e16);
    b = fold_box(desc, 3);
    EXPECT(b.box && b.logp == 1e16 + 2.0 && b.logp != 1e16);
    const PriorTerm three[3] = {uni(0.1), uni(0.2), uni(0.3)};              // (0.1 + 0.2) + 0.3 != 0.1 + (0.2 + 0.3)
    b = fold_box(three, 3);
    EXPECT(b.box && b.logp == (0.1 + 0.2) + 0.3 && b.logp != 0.1 + (0.2 + 0.3));
    // from 0.0: a single -0.0 sums to +0.0; no terms: the empty box, 0.0
    const PriorTerm mz[1] = {uni(-0.0)};
    b = fold_box(mz, 1);
    EXPECT(b.box && b.logp == 0.0 && !std::signbit(b.logp));
    b = fold_box(mz, 0);
    EXPECT(b.box && b.logp == 0.0 && !std::signbit(b.logp));
    // pads are skipped whatever their record holds
    const PriorTerm padded[4] = {uni(0.1), PriorTerm{NaN, NaN, NaN, PRIOR_NONE, 0}, uni(0.2), PriorTerm{INF, 0.0, 0.0, PRIOR_NONE, 0}};
    b = fold_box(padded, 4);
    EXPECT(b.box && b.logp == 0.1 + 0.2);
    // one term that is not uniform: no box, at any place; the sum stays that of the uniform terms
    for (int at = 0; at < 3; ++at)
        for (int kind : {PRIOR_LOG_UNIFORM, PRIOR_NORMAL}) {
            PriorTerm run[3] = {uni(0.1), uni(0.2), uni(0.3)};
            run[at] = PriorTerm{5.0, 2.0, LS, kind, 0};
            b = fold_box(run, 3);
            double want = 0.0;
            for (int d = 0; d < 3; ++d) want += d == at ? 0.0 : run[d].c0;
            EXPECT(!b.box && b.logp == want);
            EXPECT(fold_box(run, at).box && !fold_box(run, at + 1).box);             // false as soon as the term is in the run
        }
    // parse, then fold: an all-uniform padded row is the box of its real dimensions
    PriorTerm row[4];
    const double lo[4] = {-1.0, 0.0, -INF, -INF}, hi[4] = {1.0, 4.0, INF, INF}, c0[4] = {U0, 2 * U0, NaN, NaN};
    for (int d = 0; d < 4; ++d) {
        const ParsedTerm p = parse_term(PRIOR_UNIFORM, lo[d], hi[d], c0[d], 0.0, 0.0, true);
        EXPECT(p.why[0] == 0);
        row[d] = p.term;
    }
    b = fold_box(row, 4);
    EXPECT(b.box && b.logp == (0.0 + U0) + 2 * U0);
    if (failures) return EXIT_FAILURE;
    std::puts("ok");
    return EXIT_SUCCESS;
}
