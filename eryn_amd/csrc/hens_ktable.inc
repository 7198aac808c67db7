// hens_ktable.inc - body of a per-likelihood kernel translation unit: define HENS_KT_LIKE (LIKE_DENSE ...) and HENS_KT_NAME
// (dense ...) and include.  See hens_ktable.h.  HENS_KT_PART (from the build) halves a unit once more: 0 = the half-step kernels
// (k_stretch_fast, k_stretch), 1 = the fused ones (k_split1_pt, k_iter), 2 = k_stretch_prior (hens_prior.h: a unit of its own, so that
// the units of the kernels that were there before compile to the code they compiled to), 3 = k_dist (hens_dist.h: likewise),
// 4 = k_stretch_prior<GIBBS> (hens_prior.h: the half-step of a Gibbs block, likewise), 5 = k_mt_dist (hens_mt.h: likewise);
// undefined = all.
#include "hens_kernels.h"
#include "hens_iter.h"
#include "hens_tile2.h"
#include "hens_ktable.h"
namespace hens {
#define HENS_KT_CAT2(a, b) a##b
#define HENS_KT_CAT(a, b) HENS_KT_CAT2(a, b)
#define KT(fn) HENS_KT_CAT(fn, HENS_KT_NAME)
#define KPTR(...) reinterpret_cast<const void*>(&__VA_ARGS__)
#ifndef HENS_DEV_D         // dev builds: the one row width they carry (NW = 8: 32, 64 or 128)
#define HENS_DEV_D 32
#endif

#if !defined(HENS_KT_PART) || HENS_KT_PART == 0
template <int MODE>
static const void* kt_fast_mode(int D, bool pipe, bool per) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD      // (tools/devbuild.sh: the dense D = 32 kernels of one GPU only - seconds instead of minutes)
    if (D == HENS_DEV_D && !per) return pipe ? KPTR(k_stretch_fast<HENS_DEV_D, L, MODE, 8, true, false>) : KPTR(k_stretch_fast<HENS_DEV_D, L, MODE, 8, false, false>);
    return nullptr;
#else
#define KT_FAST(DT, NW)                                                                            \
    if (D == DT) {                                                                                 \
        if (pipe) { if (!per) return KPTR(k_stretch_fast<DT, L, MODE, NW, true, false>);        \
                    if constexpr (MODE != MODE_EVAL) return KPTR(k_stretch_fast<DT, L, MODE, NW, true, true>); else return nullptr; } \
        if (per) { if constexpr (MODE != MODE_EVAL) return KPTR(k_stretch_fast<DT, L, MODE, NW, false, true>); else return nullptr; } \
        return KPTR(k_stretch_fast<DT, L, MODE, NW, false, false>);                                \
    }
    KT_FAST(32, 8) KT_FAST(64, 8) KT_FAST(16, 4) KT_FAST(8, 4) KT_FAST(128, 8)
#undef KT_FAST
    return nullptr;
#endif
}
const void* KT(ktab_stretch_fast_)(int mode, int D, bool pipe, bool per) {
    switch (mode) {
        case MODE_STRETCH: return kt_fast_mode<MODE_STRETCH>(D, pipe, per);
        case MODE_EVAL: return kt_fast_mode<MODE_EVAL>(D, pipe, per);
        case MODE_MH: return kt_fast_mode<MODE_MH>(D, pipe, per);
    }
    return nullptr;
}
const void* KT(ktab_stretch2_)(int D, bool pipe) {   // the persistent, software-pipelined first launch (hens_tile2.h)
#ifdef HENS_DEV_BUILD
    return nullptr;
#else
    if (D != 64) return nullptr;
    return pipe ? KPTR(k_stretch2<64, HENS_KT_LIKE, true>) : KPTR(k_stretch2<64, HENS_KT_LIKE, false>);
#endif
}
#endif
#if !defined(HENS_KT_PART) || HENS_KT_PART == 2
}  // namespace hens
#include "hens_prior.h"
namespace hens {
template <int MODE>
static const void* kt_prior_mode(int D) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD
    return nullptr;            // (the generic k_stretch serves prior terms in a dev build)
#else
#define KT_PRIOR(DT, NW) if (D == DT) return KPTR(k_stretch_prior<DT, L, MODE, NW>);
    KT_PRIOR(32, 8) KT_PRIOR(64, 8) KT_PRIOR(16, 4) KT_PRIOR(8, 4) KT_PRIOR(128, 8)
#undef KT_PRIOR
    return nullptr;
#endif
}
const void* KT(ktab_stretch_prior_)(int mode, int D) {
    switch (mode) {
        case MODE_STRETCH: return kt_prior_mode<MODE_STRETCH>(D);
        case MODE_EVAL: return kt_prior_mode<MODE_EVAL>(D);
        case MODE_MH: return kt_prior_mode<MODE_MH>(D);
    }
    return nullptr;
}
#endif
#if !defined(HENS_KT_PART) || HENS_KT_PART == 4
}  // namespace hens
#include "hens_prior.h"
namespace hens {
template <int MODE>
static const void* kt_gibbs_mode(int D) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD
    (void)D;
    return nullptr;            // (a dev build carries no Gibbs launch)
#else
#define KT_GIBBS(DT, NW) if (D == DT) return KPTR(k_stretch_prior<DT, L, MODE, NW, true>);
    KT_GIBBS(32, 8) KT_GIBBS(64, 8) KT_GIBBS(16, 4) KT_GIBBS(8, 4) KT_GIBBS(128, 8)
#undef KT_GIBBS
    return nullptr;
#endif
}
const void* KT(ktab_stretch_gibbs_)(int mode, int D) {
    switch (mode) {
        case MODE_STRETCH: return kt_gibbs_mode<MODE_STRETCH>(D);
        case MODE_MH: return kt_gibbs_mode<MODE_MH>(D);
    }
    return nullptr;
}
#endif
#if !defined(HENS_KT_PART) || HENS_KT_PART == 3
}  // namespace hens
#include "hens_dist.h"
namespace hens {
const void* KT(ktab_dist_)(int D) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD
    (void)D;
    return nullptr;            // (a dev build carries no DistributionGenerate launch)
#else
#define KT_DIST(DT, NW) if (D == DT) return KPTR(k_dist<DT, L, NW>);
    KT_DIST(32, 8) KT_DIST(64, 8) KT_DIST(16, 4) KT_DIST(8, 4) KT_DIST(128, 8)
#undef KT_DIST
    return nullptr;
#endif
}
#endif
#if !defined(HENS_KT_PART) || HENS_KT_PART == 5
}  // namespace hens
#include "hens_mt.h"
namespace hens {
const void* KT(ktab_mt_dist_)(int D) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD
    (void)D;
    return nullptr;            // (a dev build carries no multiple-try launch)
#else
#define KT_MT(DT, NW) if (D == DT) return KPTR(k_mt_dist<DT, L, NW>);
    KT_MT(32, 8) KT_MT(64, 8) KT_MT(16, 4) KT_MT(8, 4) KT_MT(128, 8)
#undef KT_MT
    return nullptr;
#endif
}
#endif
#if !defined(HENS_KT_PART) || HENS_KT_PART == 0
const void* KT(ktab_stretch_)(int mode) {
    constexpr int L = HENS_KT_LIKE;
    switch (mode) {
        case MODE_STRETCH: return KPTR(k_stretch<L, MODE_STRETCH>);
        case MODE_EVAL: return KPTR(k_stretch<L, MODE_EVAL>);
        case MODE_MH: return KPTR(k_stretch<L, MODE_MH>);
    }
    return nullptr;
}
#endif
#if !defined(HENS_KT_PART) || HENS_KT_PART == 1
const void* KT(ktab_split1_pt_)(int D, bool per, bool shrt, bool pipe, bool col) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD
    if (D != HENS_DEV_D || per || shrt) return nullptr;
    if (pipe) return col ? KPTR(k_split1_pt<HENS_DEV_D, L, 8, false, false, true, true>) : KPTR(k_split1_pt<HENS_DEV_D, L, 8, false, false, true, false>);
    return col ? KPTR(k_split1_pt<HENS_DEV_D, L, 8, false, false, false, true>) : KPTR(k_split1_pt<HENS_DEV_D, L, 8, false, false, false, false>);
#else
#define KT_FUSED(DT, NW)                                                                           \
    if (D == DT) {                                                                                 \
        if (pipe) return (shrt || (per && col)) ? nullptr : (per ? KPTR(k_split1_pt<DT, L, NW, true, false, true, false>) : (col ? KPTR(k_split1_pt<DT, L, NW, false, false, true, true>) : KPTR(k_split1_pt<DT, L, NW, false, false, true, false>))); \
        if (col) return (per || shrt) ? nullptr : KPTR(k_split1_pt<DT, L, NW, false, false, false, true>); \
        if (per) return shrt ? KPTR(k_split1_pt<DT, L, NW, true, true, false, false>) : KPTR(k_split1_pt<DT, L, NW, true, false, false, false>); \
        return shrt ? KPTR(k_split1_pt<DT, L, NW, false, true, false, false>) : KPTR(k_split1_pt<DT, L, NW, false, false, false, false>); \
    }
    KT_FUSED(32, 8) KT_FUSED(8, 4) KT_FUSED(16, 4) KT_FUSED(64, 8) KT_FUSED(128, 8)
#undef KT_FUSED
    return nullptr;
#endif
}
const void* KT(ktab_iter_)(int D, bool per) {
    constexpr int L = HENS_KT_LIKE;
#ifdef HENS_DEV_BUILD
    return (D == 32 && HENS_DEV_D == 32 && !per) ? KPTR(k_iter<32, L, 8, false>) : nullptr;
#else
    if (D == 32) return per ? KPTR(k_iter<32, L, 8, true>) : KPTR(k_iter<32, L, 8, false>);
    if (D == 16) return per ? KPTR(k_iter<16, L, 8, true>) : KPTR(k_iter<16, L, 8, false>);
    return nullptr;
#endif
}
#endif
}  // namespace hens
