// hens_rj_group.h - the group stretch move with a stationary friend table on leaf-packing records: k_rj<RJ_MODE_GROUP>'s proposal
// phase and the kernels that rebuild the table.  Included by hens_rj.h in front of k_rj (it needs RjArgs and the draw functions, and
// k_rj needs rj_group_propose); citations are relative to the same tree as hens_rj.h's.
//
// The reference's GroupStretchMove (moves/group.py:122-281, moves/groupstretch.py:34-120 over stretch.py:103-158) with
// gibbs_sampling_setup = None stretches every leaf toward a FRIEND, a leaf near it out of a stationary snapshot of the cold chain that
// is rebuilt every n_iter_update iterations.  The reference leaves setup_friends / fix_friends / find_friends to the user; this
// project fixes one scheme - nearest friends by one key parameter per branch, as the reference's own test does (tests/test_eryn.py:
// 809-1010) - and this comment is its specification (tests/rj_group_move.py states it in NumPy).
//
// Parameters: nfriends 1 .. 64; n_iter_update >= 2 (>= 1 with live_dangerously: group.py:45-46); a, the stretch scale; key[b], the
// parameter index of branch b that measures nearness.
//
//  1 Friend table (rebuild).  Per branch b the active leaves of the cold rung (global rung 0) in ascending (walker, slot) order, sorted
//    STABLY by x[key[b]] ascending with -0.0 keyed as +0.0: keys_b[n_b], tab_b[n_b][ndim_b] (the rows keep their bits).  No uniqueness
//    filter (the reference's test has one); n_b may be 0.
//  2 Window of a leaf.  nf = min(nfriends, n_b) contiguous table entries, given by their first index `start`: the greedy walk of
//    hens_rj_group_host.h from lower_bound(keys_b, x[key]) - nf times: step left when there is an entry on the left and (none on the
//    right or fabs(x - keys[lo - 1]) <= fabs(keys[hi] - x)), else step right.  Friend j of the leaf is tab_b[start + j], in key order.
//    The window's keys are the keys of the nf entries a stable argsort of |x[key] - keys_b| puts first, value for value, and where the
//    table's keys are all different they are the same entries.  Among entries with the SAME key left of x the walk takes the ones
//    next to x, the argsort the ones of lowest index - with duplicate keys the argsort's set need not be contiguous, a window is.
//    (tools/rj_group_host_check.cpp and tests/test_rj_group_move.py hold the walk to exactly this.)
//  3 Which windows are computed when.  At a rebuild every active leaf of every rung gets its window from its position then.  A leaf
//    born since the last group move gets its window at the head of the next group move, from its position then (fix_friends).
//    Otherwise a window stays with its leaf while the leaf moves, travels with the walker through the PT cascade and is dropped when
//    the leaf dies.  Births are detected by keeping, beside the windows, the leaf masks as they stood at the last group move; both
//    arrays are indexed by POOL ROW (RjGroup::start / snap), so a swap - a permutation of `loc` - carries them and no other kernel
//    knows of them.
//  4 Rebuild schedule.  At the move's call number m with m % n_iter_update == 0, from the state in front of the move.  (The reference
//    calls setup_friends a second time behind the move, on a copy of the state in front of it, group.py:275-278: the same table from
//    the same state, and the windows it computes go to the copy.  Built once here.)  m restarts at 0 when a state is uploaded or the
//    group is set.  The table is state that a State does not carry: a chain resumed in a new context is the uninterrupted chain only
//    if the resume falls on a rebuild.
//  5 Proposal.  One zz = ((a - 1) u + 1)^2 / a per walker; per active leaf a pick j uniform on [0, nf), c = tab_b[start + j],
//    q = c - (c - x) zz on all its parameters.  Dead slots, and leaves of a branch with n_b == 0, keep their bits.
//    Under hens_rj_set_periodic: q = wrap(c - distance(x, c) zz) (stretch.py:136-154), and the slots that keep their bits are wrapped
//    too (x % period on their periodic coordinates: the reference wraps the whole array).  The friend RULE (2) stays linear in the key.
//    factors = (sum_b nleaves_max_b ndim_b - 1) log zz: the reference's count (groupstretch.py:112, group.py:195-201: every slot,
//    active or not), as k_rj<RJ_MODE_STRETCH> has it.
//  6 Evaluation and acceptance: k_rj's - the log-prior over the active leaves, fix_logp_gibbs with every branch under proposal, the
//    likelihood not evaluated where the log-prior is -inf or the walker has no leaf (fill), accept when factors + beta logl + logp -
//    (beta L + P) > log u (group.py:240-254), Move.update.  All (rung, walker) move in ONE proposal - a proposal reads no other
//    walker's current state, so there is no red / blue split: one launch.  Behind it accepted += mask, num_proposals += 1 and one
//    swap cascade with adaptation.
//
// Draws (production): one Philox call per (iteration, walker), a lane per key - lane s < nslots: PURPOSE_RJ_GROUP | s << 8, word x is
// slot s's pick rj_pick(x, nf); lane nslots: PURPOSE_RJ_GROUP | 64 << 8, zz's uniform u01(x, y); lane nslots + 1: rj_acc_key(
// RJ_MODE_GROUP, 0), the accept uniform.  (A record of 63 or 64 slots has no lanes left for the last two: a second call on lanes 0 / 1.)
#pragma once
#include "hens_rj_group_host.h"

namespace hens {

constexpr int RJ_GROUP_SLOTS = 64;                      // leaf slots of a record under a group (a lane each), stride of RjGroup::start
constexpr uint32_t RJ_GROUP_ZZ = 64;                    // the "slot" of zz's key
__host__ __device__ __forceinline__ uint32_t rj_group_key(uint32_t s) { return PURPOSE_RJ_GROUP | (s << 8); }

// the key of logical lane l of a walker's call: picks, zz, accept
__device__ __forceinline__ uint32_t rj_group_lane_key(int l, int nslots) {
    return l < nslots ? rj_group_key((uint32_t)l) : (l == nslots ? rj_group_key(RJ_GROUP_ZZ) : rj_acc_key(RJ_MODE_GROUP, 0));
}

// k_rj<RJ_MODE_GROUP>'s proposal phase (rules 2, 3, 5): fixes the newborn leaves' windows, stores windows and mask snapshot, writes the
// proposal into q (= cur on entry) and returns the factors.  One wavefront per walker, a lane per leaf slot.  GEN: leaf widths are
// the model's run-time values (k_rj's GEN), else RJ_ND.
template <bool GEN>
__device__ __forceinline__ double rj_group_propose(const RjArgs& A, const int lane, const int64_t gw, const uint32_t wid, const double* cur,
                                                   double* q, const uint32_t mk0, const uint32_t mk1, const uint32_t mk2, const uint32_t mk3,
                                                   double& u_drawn, bool& u_have) {
    const RjModel& M = A.M;
    const RjGroup& G = A.G;
    const size_t prow = (size_t)A.loc[gw];
    // this lane's slot: branch, slot in the branch and what the branch says about it (a wave-uniform loop, per-lane selects)
    bool is_slot = false, active = false, had = false;
    int n_of = 0, nd_l = 1, off_l = 0, koff_l = 0, key_l = 0, cnt_l = 0, s0 = 0;
    for (int b = 0; b < M.nb; ++b) {
        const uint32_t mk = b == 0 ? mk0 : (b == 1 ? mk1 : (b == 2 ? mk2 : mk3));
        const uint32_t sn = G.snap[prow * RJ_MAX_BRANCH + b];
        const int cnt = G.cnt[b];
        if (lane >= s0 && lane < s0 + M.nl[b]) {
            is_slot = true; n_of = lane - s0;
            nd_l = GEN ? M.nd[b] : RJ_ND; off_l = M.off[b]; koff_l = G.koff[b]; key_l = G.key[b]; cnt_l = cnt;
            active = (mk >> n_of) & 1u; had = (sn >> n_of) & 1u;
        }
        s0 += M.nl[b];
    }
    const int nslots = s0;                                // (<= RJ_GROUP_SLOTS: hens_rj_set_group)
    const int nf = G.nfriends < cnt_l ? G.nfriends : cnt_l;
    int st = -1;
    if (is_slot) {
        st = G.start[prow * RJ_GROUP_SLOTS + lane];
        if (!active) st = -1;                             // (the leaf died, or was never there)
        else if (!had || st < 0) st = rj_group_window(G.keys + koff_l, cnt_l, G.nfriends, cur[off_l + n_of * nd_l + key_l]);     // newborn
        G.start[prow * RJ_GROUP_SLOTS + lane] = st;
    }
    if (lane < RJ_MAX_BRANCH)
        G.snap[prow * RJ_MAX_BRANCH + lane] = lane == 0 ? mk0 : (lane == 1 ? mk1 : (lane == 2 ? mk2 : mk3));
    // draws
    double uzz;
    int pick = 0;
    if (G.pick) {
        if (is_slot) pick = G.pick[(size_t)gw * nslots + lane];
        uzz = A.st_uzz[gw];
    } else {
        const u4 dr = rj_philox(A.seed, A.iter, wid, rj_group_lane_key(lane, nslots));
        const double u1 = u01(dr.x, dr.y);
        double u2 = 0.0;
        if (nslots + 1 >= 64) {                           // (logical lanes 64 / 65)
            const u4 d2 = rj_philox(A.seed, A.iter, wid, rj_group_lane_key(64 + (lane & 1), nslots));
            u2 = u01(d2.x, d2.y);
        }
        uzz = nslots < 64 ? __shfl(u1, nslots) : __shfl(u2, nslots - 64);
        u_drawn = nslots + 1 < 64 ? __shfl(u1, nslots + 1) : __shfl(u2, nslots + 1 - 64);
        u_have = true;
        pick = nf > 0 ? rj_pick(dr.x, nf) : 0;
    }
    pick = pick < 0 ? 0 : (pick >= nf ? nf - 1 : pick);   // (a caller's pick outside [0, nf) reads no other memory)
    const double zz = draw_zz(uzz, A.st_a);                                          // stretch.py:129-132
    if (is_slot && active && nf > 0 && st >= 0 && st + pick < cnt_l) {
        const double* c_row = G.tab + (size_t)(koff_l + st + pick) * RJ_MAX_ND;
        for (int d = 0; d < nd_l; ++d) {
            const int i = off_l + n_of * nd_l + d;
            const double c = c_row[d];
            if (A.per_on) {                                                          // stretch.py:136-154 (period 0: c - s, no wrap)
                const double pr = A.ctab[RJ_CTAB_PERIOD + i];
                q[i] = periodic_wrap(c - periodic_diff(cur[i], c, pr) * zz, pr);
            } else {
                q[i] = c - (c - cur[i]) * zz;                                        // stretch.py:141-145
            }
        }
    } else if (A.per_on && is_slot) {
        // a dead slot, a leaf of a branch without a table: its own friend - c - (c - x) zz = x - 0 zz keeps x's bits, and the reference
        // wraps the whole array (stretch.py:149-153): x % period on the slot's periodic coordinates
        for (int d = 0; d < nd_l; ++d) {
            const int i = off_l + n_of * nd_l + d;
            const double pr = A.ctab[RJ_CTAB_PERIOD + i];
            if (pr > 0.0) q[i] = periodic_wrap(cur[i], pr);
        }
    }
    return ((double)M.ind_off - 1.0) * log(zz);                                      // groupstretch.py:112
}

// ---- rebuild (rule 1, and rule 3's "at a rebuild"): three launches on the context's stream, once per n_iter_update iterations ------
struct RjGroupBuildArgs {
    const double* pool; const int32_t* loc;
    RjModel M;
    double* gkey; int32_t* gsrc;        // gather scratch [W nslots]: key and source (pool row << 6 | slot in the branch), cold-rung order
    double* keys; double* tab; int32_t* cnt;
    int32_t* start; uint32_t* snap;
    int32_t koff[RJ_MAX_BRANCH], key[RJ_MAX_BRANCH];
    int32_t Tl, W, nfriends;
};

// one workgroup per branch: the cold rung's active leaves in ascending (walker, slot) order - count, scan, gather
__global__ __launch_bounds__(256) void k_rj_group_gather(const RjGroupBuildArgs A) {
    __shared__ int s_scan[256];
    const RjModel& M = A.M;
    const int b = (int)blockIdx.x, tid = (int)threadIdx.x;
    const int nd = M.nd[b], koff = A.koff[b];
    int base = 0;
    for (int w0 = 0; w0 < A.W; w0 += 256) {
        const int w = w0 + tid;
        uint32_t m = 0u;
        size_t row = 0;
        if (w < A.W) {                                    // (the cold rung: rows loc[0 .. W))
            row = (size_t)A.loc[w];
            m = (uint32_t)A.pool[row * M.RW + M.ind_off + b];
        }
        const int c = __builtin_popcount(m);
        s_scan[tid] = c;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {
            const int v = tid >= off ? s_scan[tid - off] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        int pos = base + s_scan[tid] - c;
        base += s_scan[255];
        while (m) {
            const int n = __builtin_ctz(m);
            m &= m - 1u;
            A.gkey[koff + pos] = A.pool[row * M.RW + M.off[b] + n * nd + A.key[b]] + 0.0;       // (-0.0 -> +0.0)
            A.gsrc[koff + pos] = (int32_t)(row << 6) | n;
            ++pos;
        }
        __syncthreads();
    }
    if (tid == 0) A.cnt[b] = base;
}

// stable sort by rank: entry e goes to the number of entries that come before it - a smaller key, or the same key and a lower index
__global__ __launch_bounds__(256) void k_rj_group_rank(const RjGroupBuildArgs A) {
    __shared__ double s_k[256];
    const RjModel& M = A.M;
    const int b = (int)blockIdx.y, tid = (int)threadIdx.x;
    const int n = A.cnt[b], koff = A.koff[b];
    const int e = (int)blockIdx.x * 256 + tid;
    if ((int)blockIdx.x * 256 >= n) return;               // (the whole workgroup)
    const double ke = e < n ? A.gkey[koff + e] : 0.0;
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 256) {
        s_k[tid] = j0 + tid < n ? A.gkey[koff + j0 + tid] : 0.0;
        __syncthreads();
        const int jn = n - j0 < 256 ? n - j0 : 256;
        for (int j = 0; j < jn; ++j) {
            const double kj = s_k[j];
            rank += (kj < ke || (kj == ke && j0 + j < e)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (e >= n || rank >= n) return;
    const int src = A.gsrc[koff + e], nd = M.nd[b];
    const double* leaf = A.pool + (size_t)(src >> 6) * M.RW + M.off[b] + (src & 63) * nd;
    A.keys[koff + rank] = ke;
    for (int d = 0; d < RJ_MAX_ND; ++d) A.tab[(size_t)(koff + rank) * RJ_MAX_ND + d] = d < nd ? leaf[d] : 0.0;
}

// every rung's windows from the leaves' positions now, and the mask snapshot: one thread per (rung, walker, slot of RJ_GROUP_SLOTS)
__global__ __launch_bounds__(256) void k_rj_group_windows(const RjGroupBuildArgs A) {
    const RjModel& M = A.M;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t gw = e >> 6;
    const int s = (int)(e & 63);
    if (gw >= (int64_t)A.Tl * A.W) return;
    const size_t prow = (size_t)A.loc[gw];
    const double* row = A.pool + prow * M.RW;
    int st = -1, s0 = 0;
    for (int b = 0; b < M.nb; ++b) {
        if (s >= s0 && s < s0 + M.nl[b]) {
            const int n = s - s0;
            if (((uint32_t)row[M.ind_off + b] >> n) & 1u)
                st = rj_group_window(A.keys + A.koff[b], A.cnt[b], A.nfriends, row[M.off[b] + n * M.nd[b] + A.key[b]]);
        }
        s0 += M.nl[b];
    }
    A.start[prow * RJ_GROUP_SLOTS + s] = st;
    if (s < RJ_MAX_BRANCH) A.snap[prow * RJ_MAX_BRANCH + s] = s < M.nb ? (uint32_t)row[M.ind_off + s] : 0u;
}

// hens_rj_group_debug: every slot's window by (rung, walker) - through `loc` - as it stands
__global__ void k_rj_group_export(const int32_t* start, const int32_t* loc, int32_t* out, int64_t TW, int nslots) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= TW * nslots) return;
    const int64_t gw = e / nslots;
    out[e] = start[(size_t)loc[gw] * RJ_GROUP_SLOTS + (e - gw * nslots)];
}

// hens_rj_group_debug_draws: what k_rj<RJ_MODE_GROUP> draws in iteration `iter`, in hens_rj_group_step's form (one thread per walker);
// a pick is taken against the table as it stands (nf = min(nfriends, n_b); 0 where nf == 0)
struct RjGroupDebugArgs {
    RjModel M;
    const int32_t* cnt;
    int32_t* pick; double* u_zz; double* u_acc;
    uint64_t iter, seed;
    int32_t Tl, W, rung_begin, nfriends;
};
__global__ void k_rj_group_debug_draws(const RjGroupDebugArgs A) {
    const int64_t gw = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (gw >= (int64_t)A.Tl * A.W) return;
    const RjModel& M = A.M;
    const int tl = (int)(gw / A.W);
    const uint32_t wid = (uint32_t)(A.rung_begin + tl) * (uint32_t)A.W + (uint32_t)(gw - (int64_t)tl * A.W);
    int nslots = 0;
    for (int b = 0; b < M.nb; ++b) nslots += M.nl[b];
    int s = 0;
    for (int b = 0; b < M.nb; ++b) {
        const int nf = A.nfriends < A.cnt[b] ? A.nfriends : A.cnt[b];
        for (int n = 0; n < M.nl[b]; ++n, ++s)
            A.pick[(size_t)gw * nslots + s] = nf > 0 ? rj_pick(rj_philox(A.seed, A.iter, wid, rj_group_key((uint32_t)s)).x, nf) : 0;
    }
    const u4 z = rj_philox(A.seed, A.iter, wid, rj_group_key(RJ_GROUP_ZZ));
    A.u_zz[gw] = u01(z.x, z.y);
    A.u_acc[gw] = rj_accept_uniform(A.seed, A.iter, wid, RJ_MODE_GROUP, 0);
}

}  // namespace hens
