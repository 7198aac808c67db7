// hens.hip - host side of libhipensemble.so: context, memory, launches, C ABI.
// Built for gfx950 only:  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
#include "../../include/hipensemble.h"
#include "hens_kernels.h"
#include "hens_rj.h"
#include "hens_iter.h"
#include "hens_tile2.h"
#include "hens_aql.h"
#include "hens_ktable.h"
#include "hens_prior.h"
#include "hens_dist.h"
#include "hens_mt.h"
#include "hens_rj_mt.h"
#include "hens_rj_gibbs.h"
#include "hens_gibbs_host.h"
#include "hens_rj_gibbs_host.h"
#include "hens_chain.h"
#include "hens_chain_stats.h"
#include "hens_rj_chain.h"
#include "hens_rj_chain_stats.h"
#include "hens_chain_host.h"
#include <unordered_map>
#include <hip/hip_ext.h>
// RCCL: types only - the library is dlopen()ed (rccl_api), nothing of it is linked.  A ROCm without the RCCL development headers
// still builds: the few types the dlsym'ed entry points use, as rccl.h (NCCL 2.x API) declares them.
#if __has_include(<rccl/rccl.h>)
#include <rccl/rccl.h>
#else
extern "C" {
typedef struct ncclComm* ncclComm_t;
typedef struct { char internal[128]; } ncclUniqueId;
typedef enum { ncclSuccess = 0 } ncclResult_t;
typedef enum { ncclSum = 0 } ncclRedOp_t;
typedef enum { ncclUint32 = 3, ncclDouble = 8 } ncclDataType_t;
}
#endif

#include <algorithm>
#include <chrono>
#include <unistd.h>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace hens;

namespace {

thread_local std::string g_last_error;

struct DrawBuf {                     // one batch of planned iterations
    Draws d{};
    DrawRec* rec = nullptr;          // the same draws by walker id (fused second half-step + cascade launch)
    DrawRec* rec1 = nullptr;         // one-launch iteration (k_iter): first half-step draws in block order,
    DrawRec* rec3 = nullptr;         //   and the first half-step draws of every second-half walker's complement
    uint32_t* keys = nullptr;        // [NB][T][8] round keys of the cascade's column maps
};
constexpr int KEY_WINDOW = 1024;     // iterations of round keys planned at once for the two-launch iteration (hens_ctx_impl::ikeys)

// D per-coordinate terms and their supports on the device, lo[D] hi[D] terms[D] in one allocation (the form k_stretch reads with
// StretchArgs::prior_on): the context's prior terms, and the generator of MH_DIST
struct TermBlock {
    double* p = nullptr;      // [6 D] doubles, D the context's row width
    int D = 0;
    const double* lo() const { return p; }
    const double* hi() const { return p + D; }
    const PriorTerm* terms() const { return reinterpret_cast<const PriorTerm*>(p + 2 * (size_t)D); }
    int upload(struct hens_ctx_impl* c, const double* lo, const double* hi, const PriorTerm* terms);      // allocates on first use; asynchronous
};

struct hens_ctx_impl {
    hens_config cfg{};
    int T = 0, W = 0, D = 0, Tl = 0, N0 = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string err;

    // state
    double* pool = nullptr;          // [2*Tl*W][D]
    int32_t* loc[2] = {nullptr, nullptr};
    double* L[2] = {nullptr, nullptr};
    double* P[2] = {nullptr, nullptr};
    WalkerRec* wrec[2] = {nullptr, nullptr};   // the same three as one record per walker (two-launch iterations of hens_step)
    bool packed = false;             // wrec[cur] holds the state, L/P/loc[cur] are stale (inside hens_step only)
    bool colmode = false;            // ... in the column order of iteration `iter` (StretchArgs::col), not by slot
    int cur = 0;                     // which of the double-buffered L/P/loc is current
    int parity = 0;                  // home half the NEXT iteration writes into
    double* betas[2] = {nullptr, nullptr};   // [T]; bcur is current
    int bcur = 0;
    uint32_t* accepted = nullptr;    // [Tl*W]
    int64_t num_proposals = 0;
    unsigned* flags = nullptr;
    uint64_t iter = 0;               // iterations completed (the Philox counter)
    int64_t adapt_time = 0;          // tempering.py:596
    bool adapt_pending = false;      // a cascade ran and its swap counts have not been reduced yet
    bool adapt_pending_adaptive = false;
    const uint32_t* adapt_src = nullptr;   // pending swap counts: swap_part (nullptr) or the mailbox's reduced counts
    int adapt_nblocks = 0;
    uint32_t* swap_part = nullptr;   // [nblocks][T-1]
    double* swaps_last = nullptr;
    double* swaps_total = nullptr;
    double* ad_ring = nullptr;       // [4][T] new ladders published by the adapting workgroup (fold mode 2), -1 = not yet
    uint32_t ad_serial = 0;
    int label_cb = 0, label_cb_shift = 0;   // block-balanced split labels: cascade columns per block (0 = legacy labels)
    // [SWAP_ACC_ROWS][T-1] swap counts accumulated with atomics by k_split1_pt / k_iter, three buffers in rotation: the
    // launch that folds the adaptation in reads one (every workgroup: it cannot clear it), the cascade accumulates into a
    // clean one, and the buffer read one launch earlier is cleared meanwhile
    uint32_t* swap_acc[3] = {nullptr, nullptr, nullptr};
    int acc_state[3] = {0, 0, 0};    // 0 clean, 1 pending (= adapt_src: the last cascade's counts), 2 read, not yet cleared
    int num_cu = 256;                // compute units of the device (MI355X: 256)
    bool rows_mixed = false;         // k_iter ran: current rows live in both halves of the pool (folded back by state_to_fields)

    // model
    double* lo = nullptr; double* hi = nullptr; double* mu = nullptr; double* prec = nullptr; double* prec_sym = nullptr;
    double* period = nullptr;        // [D] periods of the periodic parameters (hens_set_periodic), nullptr: none
    double* period_buf = nullptr;
    PriorTerm* prior = nullptr;      // [D] per-parameter prior terms (hens_set_prior_terms), nullptr: the box and its constant logp_in
    PriorTerm* prior_buf = nullptr;
    TermBlock prior_block;           // what the kernels read with terms on
    double logp_in = 0.0, rosen_a = 1.0, rosen_b = 100.0;
    bool have_prior = false, have_like = false, have_state = false, have_logs = false;

    // draws: ONE batch buffer, planned on the main stream in front of the batch that reads it
    DrawBuf db[1];
    int NB = 0, NP2 = 1, idx_bits = 0;
    // the two-launch iteration computes its draws in registers and needs the rungs' round keys only: a window of
    // KEY_WINDOW iterations, planned on the main stream when the chain leaves it (it survives hens_step calls)
    uint32_t* ikeys = nullptr;             // [KEY_WINDOW][T][8]
    uint64_t ikeys_iter0 = 0;
    int64_t ikeys_n = 0;
    uint64_t win_from = 0; int win_count = 0;   // iterations planned in db[0] for hens_stretch_iter / sharded PT

    // parity staging
    int32_t* order = nullptr;        // [Tl][W]
    int64_t* d_rint = nullptr; double* d_uzz = nullptr; double* d_uacc = nullptr; uint8_t* d_keep = nullptr;
    int64_t* d_iperm = nullptr; int64_t* d_i1perm = nullptr; double* d_uswap = nullptr;
    int32_t* d_inv = nullptr; int32_t* colk = nullptr; double* colu = nullptr; int32_t* colslot = nullptr;   // [T][W]
    uint8_t* selcol = nullptr; uint8_t* selk = nullptr;
    double* xtmp = nullptr;          // [Tl*W][D] download staging
    int expect_split = 0;
    bool propose_pending = false;
    int nsplits = 2;                 // hens_set_nsplits: sets of the parity API's red-blue move (red_blue.py:41-47)
    std::vector<int> seg_off;        // [nsplits + 1] position range of every set in `order` (this iteration's labels)
    int32_t* hl_rs = nullptr; uint8_t* hl_keep = nullptr;   // host-likelihood path scratch
    std::vector<uint8_t> labels_host;
    std::vector<int32_t> rank_of_host;

    // sharded exchange
    double* gather_L = nullptr;
    double* send_rows = nullptr; double* recv_rows = nullptr;
    int32_t* srcglob = nullptr; int32_t* send_slots = nullptr; int32_t* send_dest = nullptr;
    unsigned* d_counts = nullptr;    // counts [2*MAX_RANKS] + cursors [MAX_RANKS]
    int32_t* d_rank_of = nullptr;    // [T]
    int64_t row_capacity = 0, n_send = 0, n_recv = 0;
    bool pt_pending = false;
    // ladder sharding over RCCL point-to-point messages inside the library (hens_comm_init): the staged transport's exchanges
    void* comm = nullptr;                   // ncclComm_t
    bool comm_on = false;

    // ladder pipeline (neighbour exchange by one-sided puts, hens_pipe_*)
    struct Pipe {
        bool on = false, connected = false;
        int nranks = 0, rank = 0;
        char* box = nullptr;               // my mailbox (uncached device memory)
        size_t box_bytes = 0;
        std::vector<char*> boxes;          // every rank's mailbox as mapped into this process
        std::vector<char> opened;          // 1: mapped through hipIpcOpenMemHandle (to be closed)
        const double* pool_cold = nullptr; // cold neighbour's walker pool as mapped here
        // staged transport (RCCL send/recv of the same messages, host-ordered): kernels write into local outboxes
        bool staged = false;
        char* out_hot = nullptr; char* out_cold = nullptr; char* out_cnt = nullptr;
        double* ldn_rows = nullptr;        // [2][W][D] rows of the cold neighbour's boundary rung, as received
        bool pool_cold_opened = false;
        char** d_boxes = nullptr;
        double* Lcur = nullptr; double* Pcur = nullptr; int32_t* botsrc = nullptr;
        unsigned* tickets = nullptr;
        unsigned long long* stats = nullptr;   // HENS_PIPE_STATS: wait ticks / waits per site
        uint32_t pub_count = 0;            // cumulative workgroups of the hottest rung that have published
        // swap counts whose ladder adaptation has not been applied yet (oldest first; at most delay + 1)
        struct Pending { const uint32_t* src; uint32_t sweep; bool adaptive; } pend[3];
        int npend = 0;
        uint32_t due_sweep = 0;            // sweep whose counts the current adapt_pending refers to
        uint32_t sweep = 0;
        long long budget = 0;              // wall-clock ticks a flag wait may take
        // fused iteration of a pipeline rank (k_stretch_fast + k_split1_pt<PIPE>, rows in place): decided at the first
        // hens_step call from properties every rank shares (step_path), fixed from then on
        bool fused = false, fused_decided = false;
        int cbl = 0, cbl_shift = 0;        // columns per workgroup of the fused launch: 128 / Tl
        int32_t* ghome = nullptr;          // [2][2][W] home rows of the guests (StretchArgs::ghome)
        // swap counts of the fused launch: [SWAP_ACC_ROWS_MAX][T] accumulated with atomics, buffer = sweep & 1; the head of the
        // next iteration's first launch (or k_pipe_epilogue at the end of a call) sums, clears and publishes them
        uint32_t* acc[2] = {nullptr, nullptr};
        uint32_t pushed = 0;               // sweeps whose counts have been published
        uint32_t rows_told = 0;            // sweeps whose "all rows have landed" the cold neighbour has been told
    } pipe;
    // Metropolis-Hastings (GaussianMove) proposals
    double* mh_step = nullptr;             // [Tl][W][D]
    double* mh_lu = nullptr;               // [Tl][W] log accept uniforms
    double* mh_u = nullptr;                // [Tl][W] staging
    uint8_t* mh_keep = nullptr;            // [Tl][W]
    double* mh_scale = nullptr;            // [D*D] proposal scale (see MhDrawArgs)
    uint32_t* accepted_mh = nullptr;       // [Tl][W] accept counts of the MH move
    uint32_t* accepted_mark = nullptr;     // [2][Tl][W] hens_step_marked: stretch / MH accept counts in front of the call's last iterations
    bool mark_valid = false, mark_mh = false;
    int mh_kind = -1;                      // -1: hens_step runs the stretch move only; MH_DIST: the slot holds hens_set_dist_proposal's generator
    TermBlock dist_block;                  // the generator of MH_DIST (DistArgs::glo / ghi / gterms)
    double* dist_factors = nullptr;        // [Tl][W] hens_dist_step's factors_out staging
    // MH_MT_DIST (hens_set_mt_dist_proposal; hens_mt.h): the generator is dist_block; the teacher-forced call's staging
    int mt_K = 0;                          // num_try
    size_t mt_q_cap = 0;                   // doubles mt_q holds
    double* mt_q = nullptr;                // [Tl][W][K][D] hens_mt_dist_step's tries
    double* mt_upick = nullptr;            // [Tl][W] pick uniforms
    int32_t* mt_pick = nullptr;            // [Tl][W] pick_out staging
    double* mt_lsw = nullptr;              // [2][Tl][W] lsw_out staging
    // Gibbs parameter blocks (hens_set_gibbs; hens_gibbs_host.h): a block table per move - [0] the stretch move, [1] the MH slot.
    // While either has one (gibbs_on) every proposing launch is a block's: k_stretch_prior<GIBBS> on the block's image, a move
    // without a table of its own being one all-true block.
    struct Gibbs {
        int nblocks = 0;                   // 0: no table
        std::vector<int32_t> n, mask;      // [nblocks], [nblocks][D] (parse_gibbs)
        double* img = nullptr;             // [GIBBS_MAX_BLOCKS] device images lo[D] hi[D] terms[D] mask[D], blocks() of them in use
        bool img_ok = false;               // ... and they are the current prior's and table's (gibbs_rebuild)
        int sel = 0;                       // hens_gibbs_select: the block of the next teacher-forced move
        int cur = 0;                       // the block the next launch of the move reads (hens_step: block after block; else sel)
        int blocks() const { return nblocks > 0 ? nblocks : 1; }
    } gibbs[2];
    std::vector<double> h_lo, h_hi;        // the prior's supports and, under terms, its records as the host gave them last
    std::vector<PriorTerm> h_terms;        //   (hens_set_prior_box / _terms): what a block's image is made of
    Draws gdr{};                           // [Tl][W] one block's planned draws (k_plan_block; own: the iteration's plan)
    double mh_weight = 0.0;                // probability that an iteration of hens_step is an MH proposal
    int64_t num_proposals_mh = 0;
    uint8_t* mask_buf = nullptr;     // hens_step_report: [Tl][W] accept counts of the call's last iterations
    uint32_t* report_prev = nullptr; // ... [2][Tl][W] the stretch / MH accept counters as the last report left them
    bool report_valid = false;
    uint64_t report_iter = 0, report_books = 0;
    // reversible-jump leaf packing (HENS_LIKE_TEMPLATE, hens_rj_*)
    struct Rj {
        RjModel M{};                         // the model as the kernels see it (RjArgs::M)
        bool general = false;                // hens_rj_set_model_general: leaf widths other than 3 / no template likelihood - hens_rj_propose / _accept only
        bool wide = false;                   // hens_rj_set_model_kinds with a leaf kind beyond pulse / sine: the WIDE instantiations of k_rj
        PriorTerm terms[RJ_MAX_BRANCH][RJ_MAX_ND] = {};        // hens_rj_set_prior_terms (M.prior_on): a branch's term per leaf parameter, supports in M.lo / hi
        double* t = nullptr; double* y = nullptr;              // [ndata] data of the template likelihood
        int64_t data_cap = 0;                                  // ... and the data points they have room for
        double* ctab = nullptr; int32_t* cbn = nullptr;        // RjArgs::ctab / cbn: what a lane needs about its record coordinate (rj_push_ctab)
        double* step = nullptr; double* u = nullptr; double* birth = nullptr;         // the caller's draws of a teacher-forced move (rj_ensure_staging)
        int8_t* change = nullptr; int32_t* leaf = nullptr; uint8_t* keep = nullptr;
        int32_t* st_own = nullptr; int32_t* st_cw = nullptr; double* uzz = nullptr;   // ... of a stretch half-step
        double *hq = nullptr, *hlogp = nullptr, *hfac = nullptr, *hlu = nullptr, *hlogl = nullptr; uint8_t* hmoved = nullptr;   // host-callable likelihood (hens_rj_propose / hens_rj_accept)
        bool accept_pending = false;         // hens_rj_propose ran: hens_rj_accept is due ...
        uint32_t* pending_acc = nullptr;     // ... and counts the move's accepts here (rj_accept_counter of the proposal)
        double* p_aside = nullptr;           // [Tl W] where a refresh's evaluation writes its log-priors (rj_evaluate)
        double* tm = nullptr; int64_t tm_ndata = 0;  // [2 Tl W][ndata] every pool row's template, resident (RjArgs::tm), or nullptr (ndata > 512)
        bool tm_valid = false;               // ... and they belong to the rows as they are (false after an upload / a teacher-forced move)
        bool tm_drift = false;               // hens_rj_step has updated them by +- a leaf since their last full evaluation
        int schedule = 0;                    // hens_rj_set_schedule: 0 "separate_branches", 1 "iterate_branches", 2 "together" (ensemble.py:414-480), 3 no birth / death move
        int in_model = HENS_RJ_INMODEL_GAUSSIAN;     // hens_rj_set_in_model: the in-model move of hens_rj_step
        bool have_scale = false, have_chol = false;  // hens_rj_set_mh_chol: the in-model Gaussian step is L z per leaf (chol), not scale x z
        double chol[RJ_MAX_BRANCH][RJ_ND][RJ_ND] = {};
        unsigned* ad_flag = nullptr; uint32_t ad_serial = 0;   // the folded adaptation's "ladder published" word (RjArgs::ad_flag), serial of the last folding launch
        bool defer_adapt = false;            // hens_rj_step: the adaptation behind a cascade rides in the next k_rj launch
        uint32_t* acc_bd = nullptr;          // [Tl][W] accept counts of the birth / death move (the in-model move uses `accepted`)
        int64_t num_mh = 0, num_bd = 0;      // moves run
        // hens_rj_set_mt_proposal: the birth / death move is MTDistGenMoveRJ with mt_K tries (0: the plain move) - k_rj_mt, hens_rj_mt.h
        int mt_K = 0;
        double* mt_dens = nullptr;           // [RJ_MAX_BRANCH][2][RJ_MAX_ND][RJ_MT_DENS] per branch the generator's and the prior's terms of one leaf
        bool mt_gen_box[RJ_MAX_BRANCH] = {}; double mt_gen_logq[RJ_MAX_BRANCH] = {};      // an all-uniform generator and its constant log-density
        double* mt_tries = nullptr;          // staging of hens_rj_mt_bd_step: the caller's tries [Tl][W][RJ_MT_MAX_TRY x RJ_MAX_ND at most], pick uniforms; the launch's sums
        double* mt_upick = nullptr; double* mt_out = nullptr;
        // hens_rj_set_gibbs: Gibbs blocks of the in-model Gaussian move over branches and leaf slots - k_rj_gibbs, hens_rj_gibbs.h
        int gb_n = 0;                        // blocks of the table (0: none)
        bool gb_whole = false;               // one block, every coordinate true: the move of a context without a table (k_rj's launch)
        int gb_sel = 0;                      // hens_rj_gibbs_select: the block of the next hens_rj_mh_step
        uint8_t* gb_tab = nullptr;           // [RJ_GIBBS_MAX_BLOCKS][RJ_MAX_RW at most] the table on the device, rows ind_off apart
        // hens_rj_set_group: the group stretch move with a stationary friend table - k_rj<RJ_MODE_GROUP>, hens_rj_group.h
        int gr_nf = 0, gr_update = 0;        // nfriends (0: no group), n_iter_update
        int64_t gr_m = 0;                    // the move's call number since the last upload / hens_rj_set_group: a rebuild is due at gr_m % gr_update == 0
        double gr_a = 2.0;                   // its stretch scale
        int gr_key[RJ_MAX_BRANCH] = {}, gr_koff[RJ_MAX_BRANCH] = {}, gr_nslots = 0;
        // every buffer of the move, made once by the setter for any model of this context: table and sort scratch [W x 64 entries],
        // counts, windows and mask snapshots by pool row [2 Tl W], the staging of hens_rj_group_step's picks [Tl W x 64]
        double *gr_keys = nullptr, *gr_tab = nullptr, *gr_gkey = nullptr;
        int32_t *gr_cnt = nullptr, *gr_gsrc = nullptr, *gr_start = nullptr, *gr_pick = nullptr;
        uint32_t* gr_snap = nullptr;
        // hens_rj_set_periodic: a branch's period per leaf parameter (0: not periodic) - RjArgs::ctab's period row, RjArgs::per_on
        double period[RJ_MAX_BRANCH][RJ_MAX_ND] = {};
        bool per_on = false;
    } rj;

    // debug / timing
    unsigned long long* d_trace = nullptr;
    int64_t trace_words = 0;
    bool tracing = false, trace_pt = false, trace_fused = false;
    int trace_rj = -1;               // k_rj launches of this mode stamp their phases (hens_debug_trace 4: in-model move, 5: birth / death)
    int per_kernel_events = 0;       // hens_set_profiling: 0 off, 1 HIP event pairs, 2 dispatch timestamps on the queue the call uses
    bool aql_prof_total = false;     // timing.total_ms of the last call came from dispatch timestamps
    hens_timing timing{};
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool step_events = false;        // the last hens_step call recorded ev0 / ev1 (hens_timing::total_ms)
    hipEvent_t ext_start = nullptr, ext_stop = nullptr;   // armed: the next stretch launch records its own begin/end
    std::vector<hipEvent_t> evpool;
    // direct AQL dispatch of the stepping launches (hens_aql.h): a user-mode HSA queue of the context's own
    hens_aql::Queue aql;
    bool aql_on = false;             // the queue exists (hens_create); HENS_NO_AQL=1 keeps every launch on the HIP stream
    bool aql_now = false;            // inside a hens_step call whose launches go to the AQL queue
    bool aql_last = false;           // ... and the iteration being queued is the call's last (its last packet carries the signal)
    bool hip_dirty = true;           // the HIP stream may hold work the AQL queue has not been ordered behind
    bool aql_failed = false;         // a dispatch inside a void helper failed (checked by fused_iteration)
    int aql_ring_every = 8;
    // kernels launched by host function pointer (launch_by_ptr): dynamic-LDS attribute set on this context's device, AQL handle
    struct KernelSlot { bool attr_done = false; const hens_aql::Kernel* ak = nullptr; };
    std::unordered_map<const void*, KernelSlot> kslots;
    // chain store: the stored steps of run_mcmc(store=True) in device memory.  A context has one family of it - hens_chain_*,
    // hens_step_chain, or on a leaf-packing context hens_rj_chain_*, hens_rj_step_chain (chain_supported / rjchain_supported) -
    // and both run the host protocol of `chain store: what both families share` below.
    struct ChainStore {
        bool on = false;
        int64_t capacity = 0, count = 0, bytes = 0;
        int Ts = 0;                          // rungs [0, Ts) are stored
        double *L = nullptr, *P = nullptr, *betas = nullptr;   // [capacity] x ([Ts][W], [Ts][W], [T])
        uint32_t* acc_tot = nullptr;         // [Ts][W] accepted totals (backends/backend.py:1069)
        unsigned long long* swaps_tot = nullptr;   // [T-1] swap totals (backends/backend.py:1072): a leaf-packing chain's in-model swaps
        std::vector<int64_t> iteration, adapt_time;   // per stored step: the Philox checkpoint of its State
        int64_t n_timed = 0; double store_ms = 0.0;   // hens_set_profiling 1: the last call's append launches
        double moments_ms = -1.0, act_ms = -1.0;      // the last k_chain_moments / k_chain_act launch (hens_chain_stats_ms)
        double leaves_ms = -1.0, leaf_moments_ms = -1.0;   // ... k_rj_chain_leaves / k_rj_chain_leaf_moments (hens_rj_chain_stats_ms)
        // per family: x[0] [capacity][Ts][W][D] of a fixed-dimension chain; per branch of a leaf-packing one
        double* x[RJ_MAX_BRANCH] = {};       // [capacity][Ts][W][nl_b][nd_b], NaN on unused leaves
        uint8_t* inds[RJ_MAX_BRANCH] = {};   // [capacity][Ts][W][nl_b]
        // ... and of a leaf-packing chain only
        uint32_t* bd_tot = nullptr;          // [Ts][W] rj_accepted totals
        uint32_t* prev = nullptr;            // [2][Tl][W] the in-model / birth-death accept counters at the mark
        double* swaps_step = nullptr;        // [T-1] the in-model cascade's counts of a stored step's last iteration, set aside
        bool mark_valid = false;             // `prev` is the counters as they stand (the last append left it so) ...
        int64_t mark_books = 0;              // ... as long as no move has run since: num_mh + num_bd then
        std::vector<void*> owned;            // every device allocation the pointers above name
        void release() {
            for (void* p : owned) (void)hipFree(p);
            *this = ChainStore{};
        }
    } chain;
    std::vector<double> launch_us;   // per-kernel profiling: begin / end of every launch of the last hens_step call (us after the first begin)
    std::vector<void*> allocs;
};

#define CTX(c) reinterpret_cast<hens_ctx_impl*>(c)

int fail(hens_ctx_impl* c, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (c) c->err = buf;
    g_last_error = buf;
    return code;
}
int no_context() { return fail(nullptr, HENS_ERR_INVALID, "null context"); }

#define HIPCHK(c, expr)                                                                            \
    do {                                                                                           \
        hipError_t e_ = (expr);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return fail(c, HENS_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                       \
    } while (0)

template <typename Tp>
int dalloc(hens_ctx_impl* c, Tp** p, size_t n) {
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(p), std::max<size_t>(n, 1) * sizeof(Tp)));
    c->allocs.push_back(*p);
    return HENS_OK;
}

int TermBlock::upload(hens_ctx_impl* c, const double* lo, const double* hi, const PriorTerm* terms) {
    D = c->D;
    if (!p)
        if (const int r = dalloc(c, &p, (size_t)6 * D)) return r;
    HIPCHK(c, hipMemcpyAsync(p, lo, D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p + D, hi, D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(p + 2 * (size_t)D, terms, (size_t)D * sizeof(PriorTerm), hipMemcpyHostToDevice, c->stream));
    return HENS_OK;
}

// ---- environment switches ---------------------------------------------------------------------------------------------------
// Every switch this file reads, read once per process at first use.  HENS_AQL_STATS and HENS_PIPE_STATS are read
// per context where they are used.
#ifdef HENS_DEV_BUILD       // (dev build, tools/devbuild.sh: the dense-Gaussian D = 32 kernels only - seconds instead of minutes)
constexpr bool DEV_BUILD = true;
#else
constexpr bool DEV_BUILD = false;
#endif
struct Env {
    bool no_aql, aql_release, step_events;                       // queue: HIP stream only / keep the release fence / event pair per call
    bool no_fused, pipe_no_fused, no_iter, no_col, no_fold, pt_no_acc, rj_no_templates;   // A/B knobs of the path decision
    bool prior_log;                                              // HENS_PRIOR_LOG: which kernel a launch under prior terms went to (tests)
    bool no_xcd, no_tile2, no_tile2_pipe, tile2_pipe_waits, tile2_log, pipe_force_late, debug_noflip;
    int tile2_force, aql_flush, aql_nobar;                       // aql_flush: -1 unset; aql_nobar, debug_noflip: dev-build probes
    long iter_max, pipe_inject_cycles;
    double pipe_timeout_s;                                       // wait budget of the pipeline's flags (default 20 s)
};
const Env& env() {
    static const Env e = [] {
        auto on = [](const char* name) { return getenv(name) != nullptr; };
        auto num = [](const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; };
        auto whole = [](const char* name, long dflt) { const char* v = getenv(name); return v ? atol(v) : dflt; };
        Env v{};
        v.no_aql = on("HENS_NO_AQL"); v.aql_release = on("HENS_AQL_RELEASE"); v.step_events = on("HENS_STEP_EVENTS");
        v.no_fused = on("HENS_NO_FUSED"); v.pipe_no_fused = on("HENS_PIPE_NO_FUSED"); v.no_iter = on("HENS_NO_ITER");
        v.no_col = on("HENS_NO_COL"); v.no_fold = on("HENS_NO_FOLD"); v.pt_no_acc = on("HENS_PT_NO_ACC");
        v.rj_no_templates = on("HENS_RJ_NO_TEMPLATES"); v.prior_log = on("HENS_PRIOR_LOG");
        v.no_xcd = on("HENS_NO_XCD"); v.no_tile2 = on("HENS_NO_TILE2"); v.no_tile2_pipe = on("HENS_NO_TILE2_PIPE");
        v.tile2_pipe_waits = on("HENS_TILE2_PIPE_WAITS"); v.tile2_log = on("HENS_TILE2_LOG");
        v.pipe_force_late = on("HENS_PIPE_FORCE_LATE"); v.debug_noflip = on("HENS_DEBUG_NOFLIP");
        v.tile2_force = (int)whole("HENS_TILE2_FORCE", 0); v.aql_flush = (int)whole("HENS_AQL_FLUSH", -1);
        v.aql_nobar = (int)whole("HENS_AQL_NOBAR", 0);
        v.iter_max = whole("HENS_ITER_MAX", 0); v.pipe_inject_cycles = whole("HENS_PIPE_INJECT_CYCLES", 0);
        v.pipe_timeout_s = num("HENS_PIPE_TIMEOUT_S", 20.0);
        return v;
    }();
    return e;
}

// ---- the two queues of a context ------------------------------------------------------------------------------------------
// Stepping launches of hens_step go to the context's AQL queue (hens_aql.h) where they can; everything else uses the HIP stream.
// The host orders the two: aql_settle before any HIP work (every entry point: enter()), hipStreamSynchronize before the first
// packet of a call if the stream may be busy (hens_step).
int aql_settle(hens_ctx_impl* c) {
    if (!c || !c->aql_on) return HENS_OK;
    c->hip_dirty = true;                       // (the caller is about to use the HIP stream)
    if (!c->aql.pending) return HENS_OK;
    if (!c->aql.drain(env().pipe_timeout_s + 10.0)) {
        c->have_state = false;                 // nothing a later call could read consistently
        return fail(c, HENS_ERR_HIP, "%s", c->aql.err.c_str());
    }
    return HENS_OK;
}
hens_ctx_impl* enter(hens_ctx* h) {            // head of every entry point that may touch the device through HIP
    hens_ctx_impl* c = CTX(h);
    (void)aql_settle(c);
    return c;
}

// kernel arguments as the AMDGPU kernarg segment lays them out: by value, in order, each at its natural alignment
template <class... Ts>
size_t pack_kernargs(char* buf, const Ts&... a) {
    size_t off = 0;
    ((off = (off + alignof(Ts) - 1) & ~(alignof(Ts) - 1), memcpy(buf + off, &a, sizeof(Ts)), off += sizeof(Ts)), ...);
    return off;
}
// one launch on the AQL queue of a kernel already resolved in the library's code objects
template <class... Ts>
int aql_launch_k(hens_ctx_impl* c, const hens_aql::Kernel* k, dim3 grid, unsigned block, size_t lds, bool signal, const Ts&... args) {
    alignas(16) char buf[hens_aql::SLOT_BYTES];
    static_assert((sizeof(Ts) + ... + 0) + 8 * sizeof...(Ts) <= hens_aql::SLOT_BYTES - 256, "kernel arguments exceed the kernarg slot");
    const size_t n = pack_kernargs(buf, args...);
    if (!c->aql.dispatch(*k, grid.x, grid.y, grid.z, block, (uint32_t)lds, buf, n, signal)) return fail(c, HENS_ERR_HIP, "AQL dispatch: %s", c->aql.err.c_str());
    // doorbell: right behind a call's first packet (the GPU starts while the host writes the rest), then every few packets
    if (c->aql.windex == c->aql.call_first + 1 || c->aql.windex - c->aql.rung >= (uint64_t)c->aql_ring_every) c->aql.ring();
    return HENS_OK;
}
// ... of a kernel of this translation unit; `cache` = the call site's per-device kernel handles
template <class F, class... Ts>
int aql_launch(hens_ctx_impl* c, const hens_aql::Kernel** cache, F fn, dim3 grid, unsigned block, size_t lds, bool signal, const Ts&... args) {
    const hens_aql::Kernel*& k = cache[c->cfg.device_id & 63];
    if (!k) {
        k = hens_aql::kernel_for(*c->aql.dev, reinterpret_cast<const void*>(fn));
        if (!k) return fail(c, HENS_ERR_HIP, "AQL dispatch: kernel not found in the library's code object");
    }
    return aql_launch_k(c, k, grid, block, lds, signal, args...);
}

// One launch of a stepping kernel instantiated in another translation unit (hens_ktable.h), by its host function: on the
// context's AQL queue while a call steps there, else on the HIP stream (between two timing events when asked).  `what` names the
// kernel in errors.  The context remembers per function that the dynamic-LDS attribute is set (it is per device, a context has one
// device) and the function's AQL handle.
template <class Args>
int launch_by_ptr(hens_ctx_impl* c, const void* fn, const char* what, dim3 grid, unsigned block, size_t lds, bool signal,
                  hipEvent_t e0, hipEvent_t e1, const Args& a) {
    if (!fn) return fail(c, HENS_ERR_UNSUPPORTED, "%s: no such instantiation in this build (ndim %d)", what, c->D);
    hens_ctx_impl::KernelSlot& ks = c->kslots[fn];
    if (lds > 60000 && !ks.attr_done) {
        const hipError_t ae = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (ae != hipSuccess) return fail(c, HENS_ERR_HIP, "hipFuncSetAttribute(%s, %zu B of LDS): %s", what, lds, hipGetErrorString(ae));
        ks.attr_done = true;
    }
    if (c->aql_now) {
        if (!ks.ak) {
            ks.ak = hens_aql::kernel_for(*c->aql.dev, fn);
            if (!ks.ak) return fail(c, HENS_ERR_HIP, "AQL dispatch: %s not found in the library's code objects", what);
        }
        return aql_launch_k(c, ks.ak, grid, block, lds, signal, a);
    }
    void* args[] = {const_cast<Args*>(&a)};
    const hipError_t e = e0 ? hipExtLaunchKernel(fn, grid, dim3(block), args, lds, c->stream, e0, e1, 0)
                            : hipLaunchKernel(fn, grid, dim3(block), args, lds, c->stream);
    if (e != hipSuccess) return fail(c, HENS_ERR_HIP, "%s launch failed: %s", what, hipGetErrorString(e));
    return HENS_OK;
}

// The likelihood kinds with device kernels: hens_config::likelihood_kind -> LIKE_* and the kernel tables of the kind's translation
// unit (hens_ktable.h).  A kind this build leaves out has no entry.
struct LikeKernels {
    int kind, like;
    const void* (*stretch_fast)(int mode, int D, bool pipe, bool per);
    const void* (*stretch)(int mode);
    const void* (*stretch_prior)(int mode, int D);
    const void* (*dist)(int D);
    const void* (*mt_dist)(int D);
    const void* (*stretch_gibbs)(int mode, int D);
    const void* (*stretch2)(int D, bool pipe);
    const void* (*split1_pt)(int D, bool per, bool shrt, bool pipe, bool col);
    const void* (*iter)(int D, bool per);
};
#define HENS_LIKE_KERNELS(KIND_, LIKE_, U) {KIND_, LIKE_, ktab_stretch_fast_##U, ktab_stretch_##U, ktab_stretch_prior_##U, ktab_dist_##U, ktab_mt_dist_##U, ktab_stretch_gibbs_##U, ktab_stretch2_##U, ktab_split1_pt_##U, ktab_iter_##U}
const LikeKernels* like_kernels(int likelihood_kind) {
    static const LikeKernels tab[] = {
        HENS_LIKE_KERNELS(HENS_LIKE_GAUSS_DENSE, LIKE_DENSE, dense),
#ifndef HENS_DEV_BUILD
        HENS_LIKE_KERNELS(HENS_LIKE_GAUSS_DIAG, LIKE_DIAG, diag),
        HENS_LIKE_KERNELS(HENS_LIKE_ROSENBROCK, LIKE_ROSEN, rosen),
#endif
    };
    for (const LikeKernels& k : tab) if (k.kind == likelihood_kind) return &k;
    return nullptr;
}
#undef HENS_LIKE_KERNELS

// a piece of HIP-stream work in the middle of a call that steps on the AQL queue (packing the state at the head of the first call
// after another entry point, an adaptation that cannot be folded): the queue drains, the work runs, the stream drains
template <class Fn>
int hip_interlude(hens_ctx_impl* c, Fn&& work) {
    if (!c->aql_now) { work(); return HENS_OK; }
    int r = aql_settle(c);
    if (r) return r;
    c->aql_now = false;
    work();
    c->aql_now = true;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->hip_dirty = false;
    c->aql.own_only = false;
    return HENS_OK;
}

int grid_for(int64_t n, int block = 256) {
    int64_t g = (n + block - 1) / block;
    return (int)std::min<int64_t>(std::max<int64_t>(g, 1), 2048);
}

int pt_blocks(const hens_ctx_impl* c) { return (c->W + PT_COLS - 1) / PT_COLS; }
bool has_pt(const hens_ctx_impl* c) { return c->cfg.tempered && c->T > 1; }
// number of real parameters: rows may be padded to a compile-time width (hens_config::ndim_active); only the Hastings
// factor (D - 1) log zz counts them (PlanArgs::D and k_prep_draws' D are used for nothing else)
int dim_active(const hens_ctx_impl* c) { return c->cfg.ndim_active ? c->cfg.ndim_active : c->D; }

// draw records of one planned iteration in block order: 64 places per column block (k_split1_pt / k_iter), of which
// cb T / 2 are used
size_t rec_per_iter(const hens_ctx_impl* c) { return c->label_cb ? (size_t)(c->W / c->label_cb) * TILE : 0; }

int plan_threads(const hens_ctx_impl* c) {
    constexpr int cap = 1024;
    return std::min(cap, std::max(64, c->NP2 / 4));
}
size_t plan_lds_bytes(const hens_ctx_impl* c) { return (size_t)6 * c->W + 16; }

// ---- stretch dispatch ----------------------------------------------------------------------------
constexpr int FAST_NW_32 = 8;
int fast_nw(int D) { return (D == 32 || D == 64 || D == 128) ? 8 : 4; }
// row widths with a compile-time-width kernel (k_stretch_fast)
// (not with per-parameter prior terms: such a context is a generic-width one to every launch decision - the copying launches of
//  k_stretch, the cascade and the adaptation as kernels of their own, MH steps through the step buffer)
// (nor with a Gibbs block table on either move, hens_set_gibbs: likewise - but its evaluation launch, which proposes nothing, stays
//  the one of the context without a table: fast_width)
bool gibbs_on(const hens_ctx_impl* c) { return c->gibbs[0].nblocks > 0 || c->gibbs[1].nblocks > 0; }
bool fast_width(const hens_ctx_impl* c) {
    const int D = c->D;
    if (c->prior) return false;
    return D == 8 || D == 16 || D == 32 || D == 64 || (D == 128 && c->cfg.likelihood_kind != HENS_LIKE_HOST);
}
bool fast_path(const hens_ctx_impl* c) { return fast_width(c) && !gibbs_on(c); }
// the real parameters a proposal of move `m` (0 stretch, 1 MH) moves: the current block's count under a table (stretch.py:55-72)
int gibbs_dim(const hens_ctx_impl* c, int m) { return c->gibbs[m].nblocks > 0 ? c->gibbs[m].n[(size_t)c->gibbs[m].cur] : dim_active(c); }

size_t generic_lds_bytes(int D, int* RS_out) {
    const int RS = (D % 2 == 0) ? D + 2 : D;
    *RS_out = RS;
    return (size_t)TILE * RS * 8 + (size_t)TILE * 8 + (size_t)4 * TILE * 8 + 4 * (size_t)TILE * 4;
}
size_t fast_lds_bytes(int D, int NW, int like) {
    return ((size_t)TILE * (D + 2) + TILE + (size_t)NW * TILE + 128) * 8 + (4 * (size_t)TILE + 128) * 4 + mf_lds_extra(D, like);
}

// Consecutive workgroups go round-robin to the 8 XCDs, each with an L2 of its own that keeps its lines from launch to
// launch: renumbered, an XCD works on WHOLE rungs (T = 16: two of them), so the rows a rung's half-step gathers - every
// row of the rung, as own row or as complement - are the rows the same XCD gathered an iteration ago, minus what the
// second launch (column blocks over all rungs: no such order possible) pushed out in between.  Config 2, same box:
// 8.45 -> 8.0 us per first launch (7.65 with the second launch's row traffic removed: the ceiling of the idea);
// 16 x 16384 x 32 27.7 -> 27.3; HENS_NO_XCD=1 is the A/B knob.
// StretchArgs::xcd_shift of a grid of gx x Tl workgroups (0: numbered as launched)
int xcd_shift(const hens_ctx_impl* c, int gx) {
    if (env().no_xcd || (gx & (gx - 1)) != 0 || ((long)gx * c->Tl) % 8 != 0) return 0;
    int sh = 0;
    while ((1 << sh) < gx) ++sh;
    return sh + 1;
}

// a launch for the HIP stream whatever the iteration's path (k_stretch_prior, k_dist, the generic k_stretch): the AQL queue set aside
template <class Launch>
int on_hip_stream(hens_ctx_impl* c, Launch&& launch) {
    const bool was_aql = c->aql_now;
    c->aql_now = false;
    const int r = launch();
    c->aql_now = was_aql;
    return r;
}

int launch_stretch_like(hens_ctx_impl* c, const LikeKernels& lk, int mode, StretchArgs a, int ntiles) {
    const dim3 grid(ntiles, c->Tl);
    const int like = lk.like;
    a.xcd_shift = xcd_shift(c, ntiles);
    // A Gibbs block's half-step (hens_set_gibbs): k_stretch_prior<GIBBS> on the image of the move's current block - the prior's
    // supports and records (a box as uniform terms) with the block's mask behind them.  HENS_PRIOR_LOG=1 (tests): says so.
    if (gibbs_on(c) && mode != MODE_EVAL) {
        const hens_ctx_impl::Gibbs& G = c->gibbs[mode == MODE_MH ? 1 : 0];
        const double* img = G.img + (size_t)G.cur * gibbs_image_doubles(c->D);
        a.lo = img; a.hi = img + c->D; a.prior_on = 2;
        a.ad_on = 0;
        if (env().prior_log) fprintf(stderr, "hens: Gibbs block %d of %d, D = %d, mode %d: k_stretch_prior<GIBBS>\n", G.cur, G.blocks(), c->D, mode);
        const int NW = fast_nw(c->D);
        return on_hip_stream(c, [&] { return launch_by_ptr(c, lk.stretch_gibbs(mode, c->D), "k_stretch_prior<GIBBS>", grid, NW * 64, prior_lds_bytes(c->D, NW, like), false, c->ext_start, c->ext_stop, a); });
    }
    if (mode == MODE_EVAL ? fast_width(c) : fast_path(c)) {
        // (periodic parameters: an instantiation of their own - on a pipeline rank too - but not for the evaluation launch, which
        //  proposes nothing)
        const bool pipe = c->pipe.on, per = mode != MODE_EVAL && c->period;
        const int NW = fast_nw(c->D);
        {
            // Round 6: launches of more than one round of workgroups (two 8-wave workgroups on each of 256 CUs) go to the persistent,
            // software-pipelined kernel (hens_tile2.h) - hens_step's in-place first launch on column-ordered records, the adaptation
            // folded the way its lambdas are ported (counts in accumulation rows, ladders of up to 128 rungs).  HENS_NO_TILE2=1: the
            // rounds of k_stretch_fast; HENS_TILE2_FORCE=n: n tiles per workgroup on any grid that divides (tests).
            // A rank of the ladder pipeline stepping with the two in-place launches (pipe_fused_iteration) has the kernel's PIPE
            // instantiation, for what that ports of k_stretch_fast<PIPE>: the lead workgroup's adaptation (ad_on == 2, the counts in
            // the mailbox's one row), counts pushed by the publishing wave (cnt_push != 1), no (L, P) publishing, no injection hook.
            const bool ad_ok = pipe ? (a.ad_on == 0 || (a.ad_on == 2 && a.ad.nblocks <= 8 * a.ad.row_groups && a.ad.row_groups == 1))
                                    : (a.ad_on == 0 || (a.ad_on == 1 && a.ad.nblocks <= 8 * a.ad.row_groups));
            // (cnt_push == 1 - the delayed schedule's push through k_stretch_fast's count-reduction machinery: here the publishing wave's,
            //  cnt_push = 3, same rows, same mailbox words and flag)
            const bool push_ok = a.cnt_push != 1 || (a.cp_zero && a.cp_rows != c->swap_part);
            // Not where the launch waits for OTHER ranks' swap counts (the reference's adaptation schedule on more than one rank): a
            // persistent workgroup that starts its first tile late ends late by as much, and the lead workgroup waits for those counts in
            // front of its first tile - the whole lateness of the slowest rank's counts would land on the launch's end, where
            // k_stretch_fast's rounds of workgroups absorb 6.5 us of it (the last workgroups go to whichever slot frees first;
            // DESIGN 6.1, profiles/r05_pipe_slack_*).  A lone rank, the delayed schedule (the counts it needs arrived a sweep ago) and
            // launches without a pending adaptation have no such wait.  HENS_TILE2_PIPE_WAITS=1 (tests): everywhere.
            const bool wait_ok = env().tile2_pipe_waits || (a.wmask >> PF_CNT0) == 0ull || a.wtarget_cnt < c->pipe.sweep;      // (counts of an EARLIER sweep: there)
            const bool pipe_ok = !pipe || (!env().no_tile2_pipe && c->pipe.fused && a.ghome && !a.pub_lp && push_ok && a.inject_c64 <= 0 && wait_ok);
            const void* k2 = (!env().no_tile2 && mode == MODE_STRETCH && pipe_ok && !per && a.inplace && a.col && a.wrec && a.ikeys && a.ns_x == 0 && !a.trace &&
                              ad_ok) ? lk.stretch2(c->D, pipe) : nullptr;
            int tp = 0;                  // (the kernel walks TWO tiles per workgroup; grids beyond 1 024 tiles run as rounds of pairs)
            if (k2 && ntiles % 2 == 0 && (env().tile2_force > 0 || (long)ntiles * c->Tl > 512)) tp = 2;
            if (tp > 1 && tile2_lds_bytes(c->D, like) <= 80 * 1024) {
                const int gx = ntiles / tp;
                a.tiles_per_wg = tp;
                if (pipe && a.cnt_push == 1) a.cnt_push = 3;
                a.xcd_shift = xcd_shift(c, gx);
                // (HENS_TILE2_LOG, tests: which kernel a context's first launches, and those around a round-key window's edge, went to)
                if (env().tile2_log && (c->iter < 3 || (c->iter + 8) % KEY_WINDOW < 16))
                    fprintf(stderr, "hens: k_stretch2<pipe=%d> grid %d x %d, ad_on %d, cnt_push %d, iter %llu\n", pipe ? 1 : 0, gx, c->Tl, a.ad_on,
                            a.cnt_push, (unsigned long long)c->iter);
                return launch_by_ptr(c, k2, "k_stretch2", dim3(gx, c->Tl), NW * 64, tile2_lds_bytes(c->D, like), false,
                                     c->aql_now ? nullptr : c->ext_start, c->ext_stop, a);
            }
        }
        return launch_by_ptr(c, lk.stretch_fast(mode, c->D, pipe, per), "k_stretch_fast", grid, NW * 64, fast_lds_bytes(c->D, NW, like), false,
                             c->aql_now ? nullptr : c->ext_start, c->ext_stop, a);
    }
    // Per-parameter prior terms at a compile-time row width: k_stretch_prior (hens_prior.h) - the copying half-step with the terms
    // formed in phase B and added by the accept wave.  Periodic parameters, the other widths and Rosenbrock rows that cannot be
    // padded: the generic kernel below, which adds the same sum behind its run-time test.  HENS_PRIOR_LOG=1 (tests): which one.
    const void* kp = (c->prior && !c->period && !c->pipe.on) ? lk.stretch_prior(mode, c->D) : nullptr;
    if (env().prior_log && c->prior)
        fprintf(stderr, "hens: prior terms, D = %d, mode %d: %s\n", c->D, mode, kp ? "k_stretch_prior" : "k_stretch");
    if (kp) {
        const int NW = fast_nw(c->D);
        a.ad_on = 0;
        return on_hip_stream(c, [&] { return launch_by_ptr(c, kp, "k_stretch_prior", grid, NW * 64, prior_lds_bytes(c->D, NW, like), false, c->ext_start, c->ext_stop, a); });
    }
    int RS;
    const size_t lds = generic_lds_bytes(c->D, &RS);
    if (lds > 160 * 1024) return fail(c, HENS_ERR_UNSUPPORTED, "ndim %d exceeds the LDS row tile", c->D);
    a.RS = RS;
    a.ad_on = 0;
    return on_hip_stream(c, [&] { return launch_by_ptr(c, lk.stretch(mode), "k_stretch", grid, 256, lds, false, c->ext_start, c->ext_stop, a); });
}

int launch_hostlike_eval(hens_ctx_impl* c, StretchArgs a, int ntiles) {
    int RS;
    const size_t lds = generic_lds_bytes(c->D, &RS);
    if (lds > 160 * 1024) return fail(c, HENS_ERR_UNSUPPORTED, "ndim %d exceeds the LDS row tile", c->D);
    if (lds > 60000) HIPCHK(c, hipFuncSetAttribute(reinterpret_cast<const void*>(k_stretch<LIKE_HOST, MODE_EVAL>),
                                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    a.RS = RS;
    a.ad_on = 0;
    hipLaunchKernelGGL((k_stretch<LIKE_HOST, MODE_EVAL>), dim3(ntiles, c->Tl), dim3(256), lds, c->stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, HENS_ERR_HIP, "k_stretch launch failed: %s", hipGetErrorString(e));
    return HENS_OK;
}

template <int MODE>
int launch_stretch(hens_ctx_impl* c, const StretchArgs& a, int ntiles) {
    if (const LikeKernels* lk = like_kernels(c->cfg.likelihood_kind)) return launch_stretch_like(c, *lk, MODE, a, ntiles);
    switch (c->cfg.likelihood_kind) {
        case HENS_LIKE_GAUSS_DENSE: case HENS_LIKE_GAUSS_DIAG: case HENS_LIKE_ROSENBROCK:       // (a kind the dev build leaves out)
            return fail(c, HENS_ERR_UNSUPPORTED, "k_stretch: no such instantiation in this build (likelihood kind %d)", c->cfg.likelihood_kind);
        case HENS_LIKE_TEMPLATE:
            return fail(c, HENS_ERR_STATE, "leaf-packing context: step with hens_rj_* (the stretch move is not defined on variable-dimension records)");
        case HENS_LIKE_HOST:
            if (MODE == MODE_EVAL) return launch_hostlike_eval(c, a, ntiles);
            return fail(c, HENS_ERR_STATE, "host-likelihood context: use hens_propose_split / hens_accept_split");
    }
    return fail(c, HENS_ERR_INVALID, "unknown likelihood kind %d", c->cfg.likelihood_kind);
}

Draws draws_at(const DrawBuf& b, size_t off) {
    Draws d = b.d;
    d.own += off; d.cw += off; d.zz += off; d.fac += off; d.lu += off;
    return d;
}

bool pipe_has_top(const hens_ctx_impl* c) { return c->cfg.rung_end < c->T; }
bool pipe_has_bot(const hens_ctx_impl* c) { return c->cfg.rung_begin > 0; }
bool pipe_active(const hens_ctx_impl* c) { return c->pipe.on && c->pipe.connected; }

int64_t guest_delta(const hens_ctx_impl* c) {
    if (!c->pipe.on) return 0;
    const PipeBox b = pipe_box(c->pipe.box, c->T, c->W, c->D);
    return (int64_t)(b.guest - c->pool);              // in doubles; both 256-byte aligned
}

StretchArgs base_args(hens_ctx_impl* c) {
    StretchArgs a{};
    a.pool = c->pool;
    a.loc = c->loc[c->cur];
    a.L = c->L[c->cur];
    a.P = c->P[c->cur];
    a.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    a.dr = c->db[0].d;
    a.accepted = c->accepted;
    a.lo = c->lo; a.hi = c->hi; a.mu = c->mu; a.prec = c->prec; a.prec_sym = c->prec_sym;
    a.period = c->period;
    if (c->prior) { a.lo = c->prior_block.lo(); a.hi = c->prior_block.hi(); a.prior_on = 1; }
    a.flags = c->flags;
    a.trace = (c->tracing && !c->trace_pt && !c->trace_fused) ? c->d_trace : nullptr;
    a.logp_in = c->logp_in;
    a.fill = c->cfg.fill_value;
    a.rosen_a = c->rosen_a; a.rosen_b = c->rosen_b;
    a.Tl = c->Tl; a.W = c->W; a.D = c->D;
    a.N0 = c->N0;
    a.rung_begin = c->cfg.rung_begin;
    a.tempered = c->cfg.tempered;
    a.guest_delta = guest_delta(c);
    a.sys_rung = (pipe_active(c) && pipe_has_top(c)) ? c->Tl - 1 : -1;   // the hot neighbour pulls rows out of that rung
    return a;
}

bool is_acc_buffer(const hens_ctx_impl* c, const uint32_t* p);
AdaptArgs adapt_args(hens_ctx_impl* c, bool adaptive, const double* in, double* out) {
    AdaptArgs a{};
    a.swap_part = const_cast<uint32_t*>(c->adapt_src ? c->adapt_src : c->swap_part);
    a.betas_in = in; a.betas_out = out;
    a.swaps_last = c->swaps_last; a.swaps_total = c->swaps_total;
    a.lag = c->cfg.adaptation_lag; a.nu = c->cfg.adaptation_time;
    a.time = c->adapt_time;
    a.kappa = (a.lag / ((double)a.time + a.lag)) / a.nu;     // tempering.py:571-572
    a.T = c->T; a.W = c->W; a.nblocks = c->adapt_src ? c->adapt_nblocks : pt_blocks(c);
    a.zero_after = 0;
    a.zero_rows = nullptr;
    a.row_groups = (c->adapt_src && is_acc_buffer(c, c->adapt_src)) ? std::max(1, (int)(a.nblocks / 8)) : 1;
    a.moving = (adaptive && (c->cfg.stop_adaptation < 0 || c->adapt_time < c->cfg.stop_adaptation)) ? 1 : 0;
    return a;
}

bool is_acc_buffer(const hens_ctx_impl* c, const uint32_t* p) {
    return p && (p == c->swap_acc[0] || p == c->swap_acc[1] || p == c->swap_acc[2]);
}
int acc_pick(const hens_ctx_impl* c, int state) {
    for (int i = 0; i < 3; ++i) if (c->acc_state[i] == state) return i;
    return -1;
}
// the launch being built folds the adaptation of the pending accumulation buffer in: it may clear the buffer that was read
// one launch earlier (nobody touches that one meanwhile); the buffer it reads becomes the next one to clear
void acc_fold(hens_ctx_impl* c, AdaptArgs& ad) {
    const int z = acc_pick(c, 2), r = acc_pick(c, 1);
    ad.zero_rows = z >= 0 ? c->swap_acc[z] : nullptr;
    if (z >= 0) c->acc_state[z] = 0;
    if (r >= 0) c->acc_state[r] = 2;
}
// the buffer the cascade being launched accumulates into; its counts are the next pending adaptation
// (k_iter folds and accumulates in ONE launch: it takes its buffer BEFORE acc_fold hands out the one that launch clears)
uint32_t* acc_take(hens_ctx_impl* c) {
    int a = acc_pick(c, 0);                  // (at most one pending and one uncleared: one of three is always clean)
    if (a < 0) {                             // cannot happen by the rotation's invariant; never hand a wild pointer to a kernel
        (void)hipStreamSynchronize(c->stream);
        (void)hipMemsetAsync(c->swap_acc[0], 0, (size_t)3 * SWAP_ACC_ROWS_MAX * c->T * 4, c->stream);
        c->acc_state[0] = c->acc_state[1] = c->acc_state[2] = 0;
        c->adapt_src = nullptr;
        a = 0;
    }
    c->acc_state[a] = 3;                     // (taken; pending once the launch is queued: acc_commit)
    return c->swap_acc[a];
}
void acc_commit(hens_ctx_impl* c) {
    for (int i = 0; i < 3; ++i) if (c->acc_state[i] == 3) c->acc_state[i] = 1;
}

// The adaptation's books.  A cascade ran: the record buffers flip and its swap counts wait for the adaptation - `rows` rows at
// `src` (an accumulation buffer, the mailbox's reduced counts), or swap_part with a row per workgroup (src = nullptr)
void cascade_ran(hens_ctx_impl* c, const uint32_t* src, int rows, bool adaptive) {
    c->cur ^= 1;
    c->adapt_pending = true;
    c->adapt_pending_adaptive = adaptive;
    c->adapt_src = src;
    if (src) c->adapt_nblocks = rows;
}
// ... and the launch being built (or k_adapt) takes the pending adaptation; flip: it writes the new ladder into the other buffer
void adapt_taken(hens_ctx_impl* c, bool flip) {
    if (c->adapt_pending_adaptive) c->adapt_time += 1;               // tempering.py:596
    c->adapt_pending = false;
    c->adapt_src = nullptr;
    if (flip) c->bcur ^= 1;
}

// reduce the pending cascade's swap counts and adapt the ladder as a kernel of its own
void flush_adapt(hens_ctx_impl* c) {
    if (!c->adapt_pending) return;
    AdaptArgs a = adapt_args(c, c->adapt_pending_adaptive, c->betas[c->bcur], c->betas[c->bcur]);
    hipLaunchKernelGGL(k_adapt, dim3(1), dim3(256), (size_t)c->T * 28 + 16, c->stream, a);
    if (is_acc_buffer(c, c->adapt_src)) {            // nothing else is running: all three accumulation buffers start clean again
        (void)hipMemsetAsync(c->swap_acc[0], 0, (size_t)3 * SWAP_ACC_ROWS_MAX * c->T * 4, c->stream);
        c->acc_state[0] = c->acc_state[1] = c->acc_state[2] = 0;
    }
    adapt_taken(c, false);
}

// how the folded adaptation is shared out: 2 (default) = workgroup (0,0) reduces the counts and adapts once, the
// others pick up their rung's beta from a ring while they compute the likelihood; 1 = every workgroup recomputes
// it.  Measured at cfg 2: 31.2 vs 32.4 us per iteration; on a pipeline rank (the counts live in uncached mailbox
// memory, one reader instead of hundreds) 108 vs 126 us at 64 rungs, 213 vs 288 us at 128 rungs.
int fold_mode(const hens_ctx_impl*) {
    return 2;
}

// can the pending adaptation ride in the next split-0 stretch launch?
bool can_fold_adapt(const hens_ctx_impl* c) {
    if (env().no_fold || !c->adapt_pending || !fast_path(c) || c->T > 128) return false;
    const int nw = fast_nw(c->D);
    const int64_t nblocks = c->adapt_src ? c->adapt_nblocks : pt_blocks(c);
    return nw >= 2 && nblocks * (c->T - 1) <= (int64_t)8 * nw * 64;
}

int check_flags(hens_ctx_impl* c, bool nan_logl_is_error) {
    unsigned f = 0;
    HIPCHK(c, hipMemcpyAsync(&f, c->flags, sizeof f, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (f) {
        HIPCHK(c, hipMemsetAsync(c->flags, 0, sizeof(unsigned), c->stream));
        if (f & FLAG_NONFINITE_X)
            return fail(c, HENS_ERR_NONFINITE, "At least one parameter value was infinite or NaN");
        if (f & FLAG_PIPE_TIMEOUT)
            return fail(c, HENS_ERR_STATE, "ladder pipeline: a neighbour rank did not answer (flag wait timed out)");
        if ((f & FLAG_NAN_LOGL) && nan_logl_is_error)
            return fail(c, HENS_ERR_NONFINITE, "The likelihood function is returning Nan.");
    }
    return HENS_OK;
}

// device scratch of one call (the debug exports): plain allocations of at least 8 bytes, all freed on every way out
struct DeviceScratch {
    std::vector<void*> p;
    ~DeviceScratch() { for (void* q : p) (void)hipFree(q); }
    template <class Tp>
    Tp* grab(size_t n) {                     // nullptr: out of device memory (the caller's text names its entry point)
        void* q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(n * sizeof(Tp), 8)) != hipSuccess) return nullptr;
        p.push_back(q);
        return static_cast<Tp*>(q);
    }
};

// the draws of the cascade keyed `key_iter` (k_debug_pt) through the scratch ds / du [T][W] into the caller's arrays that are not null
int export_pt_draws(hens_ctx_impl* c, int32_t* ds, double* du, uint64_t key_iter, int32_t* slot_out, double* u_out) {
    const size_t n = (size_t)c->T * c->W;
    hipLaunchKernelGGL(k_debug_pt, dim3(grid_for((int64_t)n)), dim3(256), 0, c->stream, ds, du, c->T, c->W, c->idx_bits, c->cfg.seed, key_iter);
    HIPCHK(c, hipGetLastError());
    if (slot_out) HIPCHK(c, hipMemcpyAsync(slot_out, ds, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (u_out) HIPCHK(c, hipMemcpyAsync(u_out, du, (size_t)(c->T - 1) * c->W * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

// Device counter arrays of n uint32 each into the caller's double arrays (a null destination is not asked for and not copied):
// the copies, whatever `also` queues on the stream besides, ONE wait for all of it, the conversions.
struct CounterOut { double* dst; const uint32_t* src; };
template <class Also>
int read_counters(hens_ctx_impl* c, size_t n, std::initializer_list<CounterOut> outs, Also&& also) {
    size_t asked = 0;
    for (const CounterOut& o : outs) asked += o.dst != nullptr;
    std::vector<uint32_t> h(asked * n);               // (staged only where the caller asks)
    size_t k = 0;
    for (const CounterOut& o : outs)
        if (o.dst) HIPCHK(c, hipMemcpyAsync(&h[n * k++], o.src, n * 4, hipMemcpyDeviceToHost, c->stream));
    if (const int r = also()) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    k = 0;
    for (const CounterOut& o : outs)
        if (o.dst) std::copy_n(&h[n * k++], n, o.dst);
    return HENS_OK;
}
int read_counters(hens_ctx_impl* c, size_t n, std::initializer_list<CounterOut> outs) {
    return read_counters(c, n, outs, [] { return (int)HENS_OK; });
}

int ready(hens_ctx_impl* c, bool need_logs) {
    if (!c) return no_context();
    if (!c->have_prior) return fail(c, HENS_ERR_STATE, "prior box not set (hens_set_prior_box)");
    if (!c->have_like) return fail(c, HENS_ERR_STATE, "likelihood constants not set");
    if (!c->have_state) return fail(c, HENS_ERR_STATE, "no state uploaded (hens_upload_state)");
    if (need_logs && !c->have_logs)
        return fail(c, HENS_ERR_STATE, "log_like/log_prior not available (upload them or call hens_eval_state)");
    return HENS_OK;
}

int ensure_pt_buffers(hens_ctx_impl* c) {
    if (c->d_iperm) return HENS_OK;
    const size_t PW = (size_t)std::max(c->T - 1, 1) * c->W;
    int r;
    if ((r = dalloc(c, &c->d_iperm, PW))) return r;
    if ((r = dalloc(c, &c->d_i1perm, PW))) return r;
    if ((r = dalloc(c, &c->d_uswap, PW))) return r;
    if ((r = dalloc(c, &c->d_inv, PW))) return r;
    if ((r = dalloc(c, &c->colk, PW))) return r;
    if ((r = dalloc(c, &c->colslot, (size_t)c->T * c->W))) return r;
    if ((r = dalloc(c, &c->colu, PW))) return r;
    if ((r = dalloc(c, &c->selcol, PW))) return r;
    if ((r = dalloc(c, &c->selk, PW))) return r;
    return HENS_OK;
}

int ensure_shard_buffers(hens_ctx_impl* c) {
    if (c->gather_L) return HENS_OK;
    const size_t TW = (size_t)c->T * c->W, cap = (size_t)c->Tl * c->W;
    int r;
    if ((r = dalloc(c, &c->gather_L, TW))) return r;
    if ((r = dalloc(c, &c->srcglob, TW))) return r;
    if ((r = dalloc(c, &c->send_rows, cap * (c->D + 2)))) return r;
    if ((r = dalloc(c, &c->recv_rows, cap * (c->D + 2)))) return r;
    if ((r = dalloc(c, &c->send_slots, cap))) return r;
    if ((r = dalloc(c, &c->send_dest, cap))) return r;
    if ((r = dalloc(c, &c->d_counts, 4 * MAX_RANKS))) return r;
    if ((r = dalloc(c, &c->d_rank_of, (size_t)c->T))) return r;
    c->row_capacity = (int64_t)cap;
    return HENS_OK;
}

size_t pt_lds_bytes(int T) { return pt_lds_layout(T); }

PtArgs pt_args(hens_ctx_impl* c, const int32_t* colslot, bool sharded) {
    PtArgs p{};
    p.Lfull = sharded ? c->gather_L : c->L[c->cur];
    p.P = c->P[c->cur]; p.loc = c->loc[c->cur];
    p.Lnew = c->L[c->cur ^ 1]; p.Pnew = c->P[c->cur ^ 1]; p.locnew = c->loc[c->cur ^ 1];
    p.betas = c->betas[c->bcur];
    p.colslot = colslot;
    p.swap_part = c->swap_part;
    p.iter = c->iter;
    p.seed = c->cfg.seed;
    p.T = c->T; p.W = c->W; p.Tl = c->Tl; p.rung_begin = c->cfg.rung_begin; p.idx_bits = c->idx_bits;
    p.srcfull = sharded ? c->srcglob : nullptr;
    if (c->packed && !sharded) { p.wrec = c->wrec[c->cur]; p.wrecnew = c->wrec[c->cur ^ 1]; }
    p.trace = (c->tracing && c->trace_pt) ? c->d_trace : nullptr;
    return p;
}

// ---- ladder pipeline ------------------------------------------------------------------------------

bool pipe_publish_fused(const hens_ctx_impl* c) {
    return fast_path(c);
}

// adaptation_delay = 1 leaves a whole iteration before a sweep's counts are needed: the adapting workgroup of the
// next iteration's first launch reduces and publishes them, and the walk kernel needs no collector at all
bool pipe_counts_in_stretch(const hens_ctx_impl* c) {
    constexpr bool off = false;
    if (c->pipe.fused) return false;             // (the fused iteration publishes its counts its own way: pipe_fused_counts)
    if (off || !pipe_active(c) || c->pipe.staged || c->cfg.adaptation_delay != 1 || !fast_path(c)) return false;
    if (fold_mode(c) != 2 || fast_nw(c->D) < 2) return false;
    const int np = c->Tl + (pipe_has_top(c) ? 1 : 0) - 1;
    return np >= 1 && (int64_t)pt_blocks(c) * np <= (int64_t)8 * fast_nw(c->D) * 64;
}
int pipe_acc_rows(const hens_ctx_impl* c) { return 8 * acc_row_groups(c->Tl + (pipe_has_top(c) ? 1 : 0)); }

// one-sided transport: the bottom boundary is the walk kernel's last phase (one launch less on every rank that has a
// cold neighbour); the staged transport needs the LUP message to leave between the two, so it keeps them apart
bool pipe_fuse_bottom(const hens_ctx_impl* c) {
    return pipe_active(c) && !c->pipe.staged && pipe_has_bot(c);
}

PipeArgs pipe_args(hens_ctx_impl* c) {
    PipeArgs a{};
    a.pool = c->pool;
    a.guest_delta = guest_delta(c);
    a.L = c->L[c->cur]; a.P = c->P[c->cur]; a.loc = c->loc[c->cur];
    a.Lnew = c->L[c->cur ^ 1]; a.Pnew = c->P[c->cur ^ 1]; a.locnew = c->loc[c->cur ^ 1];
    a.betas = c->betas[c->bcur];
    a.box = c->pipe.box;
    a.box_hot = pipe_has_top(c) ? c->pipe.boxes[c->pipe.rank + 1] : nullptr;
    a.box_cold = pipe_has_bot(c) ? c->pipe.boxes[c->pipe.rank - 1] : nullptr;
    a.pool_cold = c->pipe.pool_cold;
    a.home_off = (c->parity ^ 1) * c->Tl * c->W;      // the stretch move of this iteration has already flipped parity
    a.nowait = c->pipe.staged ? 1 : 0;
    a.count_tail = pipe_counts_in_stretch(c) ? 0 : 1;
    a.fuse_bottom = pipe_fuse_bottom(c) ? 1 : 0;
    a.boxes = c->pipe.d_boxes;
    a.Lcur = c->pipe.Lcur; a.Pcur = c->pipe.Pcur; a.botsrc = c->pipe.botsrc;
    a.swap_part = c->swap_part;
    a.flags = c->flags;
    a.tickets = c->pipe.tickets;
    a.stats = c->pipe.stats;
    a.iter = c->iter; a.seed = c->cfg.seed;
    a.sweep = c->pipe.sweep;
    a.budget = c->pipe.budget;
    a.T = c->T; a.W = c->W; a.D = c->D; a.Tl = c->Tl; a.rung_begin = c->cfg.rung_begin; a.idx_bits = c->idx_bits;
    a.par = (int)(c->pipe.sweep & 1u);
    a.nranks = c->pipe.nranks; a.rank = c->pipe.rank;
    return a;
}

// the stream waits until the listed flags of MY mailbox (and, optionally, every rank's counts flag) reach `target`
void pipe_wait(hens_ctx_impl* c, std::initializer_list<int> which, bool counts, uint32_t target) {
    const PipeBox me = pipe_box(c->pipe.box, c->T, c->W, c->D);
    PipeWaitArgs w{};
    for (int f : which) w.p[w.n++] = me.flags + f;
    w.cnt_flags = counts ? me.flags + PF_CNT0 : nullptr;
    w.nranks = c->pipe.nranks;
    if (w.n == 0 && !counts) return;
    w.err = c->flags;
    w.budget = c->pipe.budget;
    w.target = target;
    hipLaunchKernelGGL(k_pipe_wait, dim3(1), dim3(64), 0, c->stream, w);
}
// before the stretch move of sweep s > 0: the rows that arrived in sweep s-1 and (if a ladder adaptation is
// pending) every rank's swap counts must be here.  The fast stretch kernel waits in its own prologue
// (wmask); other row widths get a wait kernel.
// dev hook: HENS_PIPE_INJECT_CYCLES=n - the previous sweep's swap-count flags count as raised only n shader cycles after the adapting
// workgroup of the first launch has started (StretchArgs::inject_c64; tools/pipe_slack.sh measures the slack with it)
int32_t pipe_inject_c64() {
    const long n = env().pipe_inject_cycles;
    return n > 0 ? (int32_t)((n + 63) / 64) : (env().pipe_force_late ? -1 : 0);   // (HENS_PIPE_FORCE_LATE, any build: the late path on every adaptation)
}
unsigned long long pipe_prewait_mask(const hens_ctx_impl* c) {
    if (!pipe_active(c) || c->pipe.sweep == 0 || c->pipe.staged) return 0ull;
    unsigned long long m = 0;
    if (pipe_has_top(c)) m |= 1ull << PF_ROWS_TOP;
    // (a lone rank reads the counts it pushed itself: no flag needed - unless the latency-injection hook is on, which delays
    //  exactly that flag: pipe_inject_c64)
    if (c->adapt_pending && c->adapt_src != nullptr && (c->pipe.nranks > 1 || pipe_inject_c64() != 0))
        for (int q = 0; q < c->pipe.nranks; ++q) m |= 1ull << (PF_CNT0 + q);
    return m;
}
// make the oldest queued adaptation the pending one if it is due (more than `delay` sweeps are queued, or `all`)
void pipe_promote_pending(hens_ctx_impl* c, bool all) {
    if (c->adapt_pending || c->pipe.npend == 0) return;
    if (!all && c->pipe.npend <= c->cfg.adaptation_delay) return;
    const auto e = c->pipe.pend[0];
    for (int i = 1; i < c->pipe.npend; ++i) c->pipe.pend[i - 1] = c->pipe.pend[i];
    c->pipe.npend -= 1;
    c->adapt_src = e.src;
    c->adapt_nblocks = 1;
    c->adapt_pending = true;
    c->adapt_pending_adaptive = e.adaptive;
    c->pipe.due_sweep = e.sweep;
}
void pipe_prewait(hens_ctx_impl* c) {
    const unsigned long long m = pipe_prewait_mask(c);
    if (!m || fast_path(c)) return;
    if ((m >> PF_ROWS_TOP) & 1) pipe_wait(c, {PF_ROWS_TOP}, false, c->pipe.sweep);
    if ((m >> PF_CNT0) != 0) pipe_wait(c, {}, true, c->pipe.due_sweep + 1);
}

// one PT sweep of the sharded ladder (tempering.py:598-649 across ranks); see hens_kernels.h
void pipe_launch_pub(hens_ctx_impl* c) {
    if (pipe_has_top(c) && !pipe_publish_fused(c)) {   // (the fast stretch kernels publish from their accept phase)
        const PipeArgs a = pipe_args(c);
        hipLaunchKernelGGL(k_pipe_pub, dim3(1), dim3(1024), 0, c->stream, a);                 // raises the neighbour's PF_LDN
    }
}
void pipe_launch_walk(hens_ctx_impl* c) {
    const PipeArgs a = pipe_args(c);
    const int TE = c->Tl + (pipe_has_top(c) ? 1 : 0);
    // waits for PF_LUP; its last workgroup raises the cold neighbour's PF_LUP and publishes my swap counts
    hipLaunchKernelGGL(k_pipe_walk, dim3(pt_blocks(c)), dim3(PT_THREADS), pt_lds_layout(TE), c->stream, a);
}
void pipe_launch_bottom(hens_ctx_impl* c) {
    if (!pipe_has_bot(c) || pipe_fuse_bottom(c)) return;
    const PipeArgs a = pipe_args(c);
    // waits for PF_LDN (+ PF_ROWS_TOP); moves the rows both ways; its last workgroup raises the cold neighbour's PF_ROWS_TOP
    hipLaunchKernelGGL(k_pipe_bottom, dim3((c->W + PIPE_COLS - 1) / PIPE_COLS), dim3(256), 0, c->stream, a);
}
void pipe_finish_sweep(hens_ctx_impl* c) {
    const PipeBox me = pipe_box(c->pipe.box, c->T, c->W, c->D);
    c->pipe.pend[c->pipe.npend++] = {me.counts + (size_t)(c->pipe.sweep & 3u) * c->T, c->pipe.sweep, c->cfg.adaptive != 0};
    c->cur ^= 1;
    c->pipe.sweep += 1;
    pipe_promote_pending(c, false);
}
void pipe_sweep(hens_ctx_impl* c) {
    pipe_launch_pub(c);
    pipe_launch_walk(c);
    pipe_launch_bottom(c);
    pipe_finish_sweep(c);
}

// apply the adaptations that are due (end of a hens_step call): each needs every rank's counts of its sweep.
// With adaptation_delay = 1 the newest sweep's counts stay queued across calls, so the chain does not depend
// on how the iterations are split into calls.
void pipe_flush_adapt(hens_ctx_impl* c) {
    for (;;) {
        pipe_promote_pending(c, false);
        if (!c->adapt_pending) break;
        if (c->adapt_src && c->pipe.nranks > 1 && !c->pipe.staged) pipe_wait(c, {}, true, c->pipe.due_sweep + 1);
        flush_adapt(c);
    }
}

// plan nb iterations starting at iteration `iter0` into draw buffer `which` (on stream s: always the context's main stream)
// block-balanced labels: keys -> places -> draws (small short workgroups, see k_plan_cols); other shapes: k_plan
void launch_plan_kernels(hens_ctx_impl* c, hipStream_t s, const PlanArgs& pa, int nb, bool keys_only = false) {
    if (pa.nsets > 2) {              // RedBlueMove(nsplits > 2): one iteration per launch, one workgroup per rung
        hipLaunchKernelGGL(k_plan_sets, dim3(c->Tl), dim3(256), 0, s, pa);
        return;
    }
    if (c->aql_now) {                // (the queue of the launches that read the plan: ordered by the packets' barrier bits)
        static const hens_aql::Kernel *ak0_[64] = {}, *ak1_[64] = {}, *ak2_[64] = {};
        int r;
        if (!pa.cb) r = aql_launch(c, ak0_, k_plan, dim3(nb * c->Tl), (unsigned)plan_threads(c), plan_lds_bytes(c), false, pa);
        else {
            r = aql_launch(c, ak1_, k_plan_keys, dim3((nb * c->Tl + 63) / 64), 64, 0, false, pa, nb);
            if (!r && !keys_only) r = aql_launch(c, ak2_, k_plan_draws, dim3((c->W + 255) / 256, nb * c->Tl), 256, 0, false, pa);
        }
        if (r) c->aql_failed = true;
        return;
    }
    if (!pa.cb) {
        hipLaunchKernelGGL(k_plan, dim3(nb * c->Tl), dim3(plan_threads(c)), plan_lds_bytes(c), s, pa);
        return;
    }
    const dim3 grid((c->W + 255) / 256, nb * c->Tl);
    hipLaunchKernelGGL(k_plan_keys, dim3((nb * c->Tl + 63) / 64), dim3(64), 0, s, pa, nb);
    if (keys_only) return;          // (the two-launch iteration computes its draws in registers)
    hipLaunchKernelGGL(k_plan_draws, grid, dim3(256), 0, s, pa);
}

void launch_plan(hens_ctx_impl* c, hipStream_t s, int which, uint64_t iter0, int nb, bool fused = false, bool iter1 = false) {
    PlanArgs pa{};
    pa.dr = c->db[which].d;
    pa.iter0 = iter0; pa.seed = c->cfg.seed; pa.a = c->cfg.a;
    pa.Tl = c->Tl; pa.W = c->W; pa.D = dim_active(c); pa.rung_begin = c->cfg.rung_begin;
    pa.idx_bits = c->idx_bits;
    pa.T = c->T; pa.cb = c->label_cb; pa.keys = c->db[which].keys;
    pa.rec = fused ? c->db[which].rec : nullptr;          // (only k_split1_pt reads the block-ordered records)
    pa.rec_only = fused ? 1 : 0;
    if (iter1) { pa.rec1 = c->db[which].rec1; pa.rec3 = c->db[which].rec3; }   // (k_iter reads nothing else)
    launch_plan_kernels(c, s, pa, nb, fused && !iter1);
}

hipEvent_t new_event(hens_ctx_impl* c) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->evpool.push_back(e);
    return e;
}
// Per-launch timing of a hens_step call on the HIP stream (hens_set_profiling): an event pair per launch and the kind of launch it
// brackets - 0 stretch / MH launch, 1 cascade (a pipeline rank: its sweep), 2 second half-step + cascade, 3 k_iter
struct LaunchTimer {
    std::vector<hipEvent_t> evs;
    std::vector<char> kind;
};
void time_launch(hens_ctx_impl* c, LaunchTimer* tm, int kind, hipEvent_t& e0, hipEvent_t& e1) {
    if (!tm) return;
    e0 = new_event(c); e1 = new_event(c);
    tm->evs.push_back(e0); tm->evs.push_back(e1);
    tm->kind.push_back((char)kind);
}
// a stretch / MH launch; timed, the dispatch packet records its own begin / end (ext_start / ext_stop, launch_stretch_like)
template <int MODE>
int launch_stretch_timed(hens_ctx_impl* c, const StretchArgs& a, int ntiles, LaunchTimer* tm) {
    time_launch(c, tm, 0, c->ext_start, c->ext_stop);
    const int r = launch_stretch<MODE>(c, a, ntiles);
    c->ext_start = c->ext_stop = nullptr;
    return r;
}

// fused pipeline iteration: what the head of the next iteration's first launch would say, as a kernel of its own (end of a
// hens_step call; an adaptation that cannot be folded) - the previous sweep's pushes are complete (cold neighbour's
// PF_ROWS_TOP) and, on the reference's adaptation schedule, that sweep's swap counts
void pipe_fused_epilogue(hens_ctx_impl* c) {
    if (!c->pipe.fused || c->pipe.sweep == 0) return;
    PipeEpilogueArgs ea{};
    if (pipe_has_bot(c) && c->pipe.rows_told < c->pipe.sweep) {
        ea.rt_flag = pipe_box(c->pipe.boxes[c->pipe.rank - 1], c->T, c->W, c->D).flags + PF_ROWS_TOP;
        ea.rt_value = c->pipe.sweep;
        c->pipe.rows_told = c->pipe.sweep;
    }
    if (c->cfg.adaptation_delay == 0 && c->pipe.pushed < c->pipe.sweep) {
        ea.push = 1;
        ea.cp_rows = c->pipe.acc[(c->pipe.sweep - 1) & 1u];
        ea.cp_boxes = c->pipe.d_boxes;
        ea.cp_sweep = c->pipe.sweep - 1;
        ea.cp_nblocks = pipe_acc_rows(c);
        ea.cp_np = c->Tl + (pipe_has_top(c) ? 1 : 0) - 1;
        ea.cp_nranks = c->pipe.nranks; ea.cp_rank = c->pipe.rank; ea.cp_T = c->T;
        ea.rung_begin = c->cfg.rung_begin; ea.W = c->W; ea.D = c->D;
        c->pipe.pushed = c->pipe.sweep;
    }
    if (ea.rt_flag || ea.push) hipLaunchKernelGGL(k_pipe_epilogue, dim3(1), dim3(64), 0, c->stream, ea);
}

// the first launch of an iteration: wait for the pipeline's arrivals in its prologue and carry the pending
// ladder adaptation (or run it as a kernel of its own where it cannot be folded)
void attach_iteration_head(hens_ctx_impl* c, StretchArgs& a) {
    if (pipe_active(c)) {                    // (the adapting wave skips its own rank's count flag: whoever pushed, it was this rank)
        a.cp_rank = c->pipe.rank;
        a.cp_nranks = c->pipe.nranks;
    }
    if (fast_path(c)) {
        a.wmask = pipe_prewait_mask(c);
        if (a.wmask) {
            a.wflags = pipe_box(c->pipe.box, c->T, c->W, c->D).flags;
            a.wtarget = c->pipe.sweep;
            a.wtarget_cnt = c->pipe.due_sweep + 1;
            a.wbudget = c->pipe.budget;
            a.wstats = c->pipe.stats;
            a.inject_c64 = pipe_inject_c64();
        }
    }
    if (pipe_counts_in_stretch(c) && c->pipe.sweep > 0) {      // the counts of the sweep that just ended
        a.cnt_push = 1;
        a.cp_rows = c->swap_part;
        a.cp_boxes = c->pipe.d_boxes;
        a.cp_sweep = c->pipe.sweep - 1;
        a.cp_nblocks = pt_blocks(c);
        a.cp_np = c->Tl + (pipe_has_top(c) ? 1 : 0) - 1;
        a.cp_nranks = c->pipe.nranks;
        a.cp_rank = c->pipe.rank;
        a.cp_T = c->T;
    }
    if (c->pipe.fused && c->adapt_pending && !can_fold_adapt(c)) pipe_fused_epilogue(c);   // (the wait below needs the counts out)
    if (c->pipe.fused && c->pipe.sweep > 0) {                  // what the previous sweep's fused launch left to its successor
        if (c->pipe.pushed < c->pipe.sweep) {                  // its swap counts (due NOW on the reference's schedule)
            a.cnt_push = c->cfg.adaptation_delay == 0 ? 2 : 1;
            a.cp_rows = c->pipe.acc[(c->pipe.sweep - 1) & 1u];
            a.cp_zero = 1;
            a.cp_boxes = c->pipe.d_boxes;
            a.cp_sweep = c->pipe.sweep - 1;
            a.cp_nblocks = pipe_acc_rows(c);
            a.cp_np = c->Tl + (pipe_has_top(c) ? 1 : 0) - 1;
            a.cp_nranks = c->pipe.nranks;
            a.cp_rank = c->pipe.rank;
            a.cp_T = c->T;
            c->pipe.pushed = c->pipe.sweep;
        }
        if (pipe_has_bot(c) && c->pipe.rows_told < c->pipe.sweep) {   // all of its pushes / pulls are complete
            a.rt_flag = pipe_box(c->pipe.boxes[c->pipe.rank - 1], c->T, c->W, c->D).flags + PF_ROWS_TOP;
            a.rt_value = c->pipe.sweep;
            c->pipe.rows_told = c->pipe.sweep;
        }
    }
    if (!c->adapt_pending) return;
    if (can_fold_adapt(c)) {
        // the previous cascade's ladder adaptation rides in this launch: every workgroup reads
        // the old ladder, workgroup (0,0) writes the new one into the other buffer
        // counts accumulated by the fused launch (a handful of rows): EVERY workgroup's second wave adapts the ladder from
        // them while its first wave fetches indices - no hand-off between workgroups (a ring published by one workgroup
        // reaches the others' accept phase ~5 us late under the row-gather load); other sources: one workgroup + ring
        const bool acc = is_acc_buffer(c, c->adapt_src);
        a.ad_on = acc ? 1 : fold_mode(c);
        if (a.ad_on == 2) {
            a.ad_ring = c->ad_ring;
            a.ad_serial = c->ad_serial++;
        }
        a.ad = adapt_args(c, c->adapt_pending_adaptive, c->betas[c->bcur], c->betas[c->bcur ^ 1]);
        if (acc) acc_fold(c, a.ad);
        a.betas = c->betas[c->bcur];
        adapt_taken(c, true);
    } else {
        if (pipe_active(c) && !c->pipe.staged && c->adapt_src && c->pipe.nranks > 1)
            pipe_wait(c, {}, true, c->pipe.due_sweep + 1);   // every rank's counts first
        flush_adapt(c);
        a.betas = c->betas[c->bcur];
    }
}

// ladder pipeline: this launch (one of the iteration's move launches; `final` = the last one) publishes the
// hottest resident rung's (L, P) to the hot neighbour; ntiles = workgroups per rung of this launch
void attach_publish(hens_ctx_impl* c, StretchArgs& a, bool final, int ntiles) {
    if (!pipe_active(c) || !pipe_has_top(c) || !pipe_publish_fused(c) || c->pipe.fused) return;   // (fused: the cascade launch publishes)
    const PipeBox hot = pipe_box(c->pipe.boxes[c->pipe.rank + 1], c->T, c->W, c->D);
    a.pub_lp = hot.lp_dn + (size_t)(c->pipe.sweep & 1u) * 2 * c->W;
    a.pub_flag = hot.flags + PF_LDN;
    a.pub_meta = hot.meta + (c->pipe.sweep & 1u);
    a.pub_ticket = c->pipe.tickets + 2;
    a.pub_value = c->pipe.sweep + 1;
    a.pub_final = final ? 1 : 0;
    if (final) {
        c->pipe.pub_count += (uint32_t)ntiles;
        a.pub_target = c->pipe.pub_count;
    }
}

// both halves of one Philox iteration from draw buffer `which`, batch slot `ib`
// inplace (hens_step on one GPU, compile-time row widths): rows are updated where they are, see StretchArgs::inplace
int stretch_pair(hens_ctx_impl* c, int which, int ib, LaunchTimer* tm, bool inplace = false) {
    const int Tl = c->Tl, W = c->W;
    for (int split = 0; split < 2; ++split) {
        StretchArgs a = base_args(c);
        a.dr = gibbs_on(c) ? c->gdr : draws_at(c->db[which], (size_t)ib * Tl * W);      // (a block's plan: gibbs_iteration)
        a.split = split;
        a.inplace = inplace ? 1 : 0;
        a.home_off = c->parity * Tl * W;
        if (split == 0) attach_iteration_head(c, a);
        const int Ns = split == 0 ? c->N0 : W - c->N0;
        attach_publish(c, a, split == 1, (Ns + TILE - 1) / TILE);
        const int r = launch_stretch_timed<MODE_STRETCH>(c, a, (Ns + TILE - 1) / TILE, tm);
        if (r) return r;
    }
    if (!inplace) c->parity ^= 1;                  // (in place: the free half of the pool stays the free one)
    c->num_proposals += 1;
    return HENS_OK;
}


// one Philox iteration of a red-blue move of nsplits > 2 sets: plan (labels, order, draws of every position), then set after set
// with the copying launches - each against the others' CURRENT rows (red_blue.py:148-323; the parity API's launches)
int stretch_sets(hens_ctx_impl* c, LaunchTimer* tm) {
    const int Tl = c->Tl, W = c->W, NSP = c->nsplits;
    c->seg_off.assign((size_t)NSP + 1, 0);
    for (int k = 0; k < NSP; ++k) c->seg_off[k + 1] = c->seg_off[k] + (W - k + NSP - 1) / NSP;
    PlanArgs pa{};
    pa.dr = c->db[0].d;
    pa.iter0 = c->iter; pa.seed = c->cfg.seed; pa.a = c->cfg.a;
    pa.Tl = Tl; pa.W = W; pa.D = dim_active(c); pa.rung_begin = c->cfg.rung_begin; pa.idx_bits = c->idx_bits; pa.T = c->T;
    pa.nsets = NSP; pa.order = c->order;
    launch_plan_kernels(c, c->stream, pa, 1);
    c->timing.n_plan += 1;
    c->win_count = 0;
    for (int split = 0; split < NSP; ++split) {
        StretchArgs a = base_args(c);
        a.dr = c->db[0].d;
        a.split = split == 0 ? 0 : (split == NSP - 1 ? 1 : 2);
        a.ns_x = c->seg_off[split + 1] - c->seg_off[split]; a.soff_x = c->seg_off[split];
        a.home_off = c->parity * Tl * W;
        if (split == 0) attach_iteration_head(c, a);
        const int r = launch_stretch_timed<MODE_STRETCH>(c, a, (a.ns_x + TILE - 1) / TILE, tm);
        if (r) return r;
    }
    c->parity ^= 1;
    c->num_proposals += 1;
    return HENS_OK;
}

// ---- which launches one iteration of a hens_step call is ------------------------------------------------------------------------
enum class Iteration {
    COPYING,         // k_stretch_fast / k_stretch x 2 on the by-field arrays, then k_pt_cascade
    SETS,            // hens_set_nsplits > 2: a copying launch per set (stretch_sets), then k_pt_cascade
    INPLACE2,        // walker records: k_stretch_fast / k_stretch2 (first half-step, rows in place), then k_split1_pt
    ONE_LAUNCH,      // walker records: k_iter
    PIPE_COPYING,    // a rank of the ladder pipeline: the copying launches, then the sweep's kernels (pipe_sweep)
    PIPE_INPLACE2,   // ... with the two in-place launches (k_split1_pt<PIPE>)
};
struct StepPath {
    Iteration it = Iteration::COPYING;
    bool col = false;        // the records are PACKED in column order (c->colmode: the order they are in)
    bool records() const { return it == Iteration::INPLACE2 || it == Iteration::ONE_LAUNCH || it == Iteration::PIPE_INPLACE2; }
    bool piped() const { return it == Iteration::PIPE_COPYING || it == Iteration::PIPE_INPLACE2; }
    // draws in registers: the launches need the rungs' round keys (iteration_keys) and no draw plan
    bool keys_only() const { return it == Iteration::INPLACE2 || it == Iteration::PIPE_INPLACE2; }
    // launches that can go to the context's AQL queue
    bool aql_able() const { return it == Iteration::INPLACE2 || it == Iteration::ONE_LAUNCH; }
};

// The path of one hens_step call, decided once at its head; everything downstream reads the verdict.  Nothing it depends on
// changes inside a call: the shape, the likelihood kind, label_cb and db[0].rec1 are fixed by hens_create, the pipeline by
// hens_pipe_*, nsplits / period / mh_kind by entry points of their own between calls, the switches once per process.
StepPath step_path(hens_ctx_impl* c) {
    const Env& e = env();
    const int kind = c->cfg.likelihood_kind;
    // walker records + k_split1_pt: tempered, block-balanced labels, compile-time row width, device likelihood
    // (HENS_NO_FUSED=1, A/B knob: the copying launches - three per iteration)
    const bool rec_shape = !e.no_fused && c->label_cb > 0 && has_pt(c) && fast_path(c) && kind != HENS_LIKE_HOST;
    // Column-ordered records (StretchArgs::col): the two-launch iteration on full tiles - every record shape that does not take
    // the single launch, has no periodic parameters and no MH move in the mix (those launches address the records by slot).
    // Round 3, config 2: both launches' index phases were a round key -> permutation -> scattered record load chain
    // (4 600 / 4 700 cycles to the first barrier); in column order the records load coalesced at the head of the launch and the
    // first launch looks rows up in an LDS copy of its rung's table.  HENS_NO_COL=1, A/B knob: records by slot.
    const bool col_able = !e.no_col && !c->period && c->mh_kind < 0 && (c->W & 3) == 0;
    StepPath p;
    if (pipe_active(c)) {
        // The two in-place launches on a rank of the ladder pipeline (round 3).  Round 2's pipeline rank ran round 1's three copying
        // launches (stretch x 2 -> k_pipe_walk): a config-3 shard stepped at 89 us per iteration as a rank against 59 us as a ladder
        // of its own.  Now: k_stretch_fast (first half-step, in place, draws in registers, carries the adaptation and the waits for
        // the previous sweep's arrivals) -> k_split1_pt<PIPE> (second half-step + the rank's segment of the cascade + both
        // boundaries, hand-offs per column block).  Decided at the rank's first call from what every rank shares - a function of
        // (T, W, D, nranks, likelihood kind) only - and fixed from then on.  HENS_PIPE_NO_FUSED=1: A/B knob.
        hens_ctx_impl::Pipe& pp = c->pipe;
        if (!pp.fused_decided) {
            auto shards_fit = [&] {                // equal shards of 128 / Tl columns x Tl rungs = one full tile
                const int Tl = c->Tl;
                if (c->T % pp.nranks != 0 || Tl != c->T / pp.nranks || c->cfg.rung_begin != pp.rank * Tl) return false;
                if (Tl < 2 || Tl > 64 || (Tl & (Tl - 1)) != 0) return false;
                const int cbl = 2 * TILE / Tl;
                return cbl >= c->label_cb && cbl % c->label_cb == 0 && c->W % cbl == 0;
            };
            pp.fused = rec_shape && !e.pipe_no_fused && !pp.staged && kind != HENS_LIKE_TEMPLATE && shards_fit();
            pp.fused_decided = true;
        }
        p.it = pp.fused ? Iteration::PIPE_INPLACE2 : Iteration::PIPE_COPYING;
        p.col = pp.fused && col_able;              // (every rank reaches the same verdict)
        return p;
    }
    if (!rec_shape || c->Tl != c->T || c->pipe.on || c->nsplits != 2) {      // (records: the whole ladder resident, two sets)
        p.it = c->nsplits > 2 ? Iteration::SETS : Iteration::COPYING;
        return p;
    }
    // One launch per iteration (k_iter, hens_iter.h): the record shapes that leave the chip half empty (latency-bound: see
    // hens_iter.h), row widths with three tiles in half a CU's LDS.  Measured on one box (tools/iter_sweep.sh, us per iteration,
    // one launch vs two):
    //   4 x 4096 x 32  14.7 / 18.2     8 x 4096 x 32  15.5 / 18.8    16 x 2048 x 32  15.6 / 18.3    32 x 1024 x 32  17.1 / 20.1
    //   16 x 4096 x 16  16.4 / 19.7   16 x 4096 x 32 (config 2)  22.4 / 22.5     8 x 8192 x 32  22.0 / 22.7
    //   32 x 2048 x 32  23.9 / 23.8   16 x 6144 x 32  33.5 / 34.5
    // Up to one workgroup per CU at D = 32 (two at D = 16, whose workgroups are half as heavy) the single launch wins
    // 15-19 %; with two D = 32 workgroups per CU its extra gathers and likelihoods cost what the second launch did, and the
    // profiled two-launch path stays.  (Round 5's last library, same columns: 4 x 4096 x 32 11.9 / 13.1, 8 x 4096 x 32 13.3 / 13.8,
    // 16 x 2048 x 32 14.0 / 14.6, 32 x 1024 x 32 15.7 / 16.5, 16 x 4096 x 16 15.2 / 15.6; 8 x 8192 x 32 19.3 / 16.4 - the rule stands, the margin
    // is 3-12 % now.)  The grid is W / cb workgroups (short tiles of ladders that do not divide 128 included:
    // 10 x 2048 x 32 15.2 / 18.5, 6 x 4096 x 32 15.0 / 18.1).  HENS_NO_ITER=1, A/B knob: two launches per iteration;
    // HENS_ITER_MAX=n: workgroups per CU allowed.
    const long nwg = c->W / c->label_cb, per_cu = e.iter_max ? e.iter_max : (c->D == 16 ? 2 : 1);
    const bool one = !e.no_iter && (c->D == 16 || c->D == 32) && c->T <= 128 && c->W <= 32768 && c->db[0].rec1 && nwg <= per_cu * (long)c->num_cu;
    p.it = one ? Iteration::ONE_LAUNCH : Iteration::INPLACE2;
    p.col = !one && col_able && c->T * c->label_cb == 2 * TILE;       // (full tiles: 128 / T columns x T rungs)
    return p;
}

// The stepping launches of one GPU (k_stretch_fast + k_split1_pt in record mode, k_iter) go out WITHOUT a release fence (hens_aql.h: norel_next): everything a
// later launch reads they store write-through, and their waves end behind the stores' acknowledgements (hens_kernels.h: wt_store,
// launch_end_wait).  HENS_AQL_RELEASE=1 keeps the fence (A/B knob).
bool norel_ok(const hens_ctx_impl* c) {
    return ROWSTORE_WRITE_THROUGH && !env().aql_release && c->aql_now && !c->pipe.on;      // (rows must leave write-through: hens_kernels.h)
}

// the state as one record per walker (k_split1_pt, k_iter, k_stretch_fast with StretchArgs::wrec) <-> by-field arrays (everything
// else); col: StepPath::col of the call that packs
const uint32_t* iteration_keys(hens_ctx_impl* c);
void state_to_records(hens_ctx_impl* c, bool col) {
    if (c->packed) return;
    const int64_t n = (int64_t)c->Tl * c->W;
    if (col) {
        // column order of iteration c->iter, into the OTHER buffers (the compact row table is permuted too: not in place)
        // (a pipeline rank: its Tl rungs, whose round keys start at rung_begin)
        const uint32_t* keys = iteration_keys(c) + (size_t)c->cfg.rung_begin * 8;
        hipLaunchKernelGGL(k_pack_cols, dim3(grid_for(n)), dim3(256), 0, c->stream, c->L[c->cur], c->P[c->cur], c->loc[c->cur],
                           c->accepted, keys, c->wrec[c->cur ^ 1], c->loc[c->cur ^ 1], c->Tl, c->W, c->idx_bits);
        c->cur ^= 1;
        c->packed = c->colmode = true;
        return;
    }
    hipLaunchKernelGGL(k_pack_state, dim3(grid_for(n)), dim3(256), 0, c->stream, c->L[c->cur], c->P[c->cur], c->loc[c->cur],
                       c->accepted, c->wrec[c->cur], n);
    c->packed = true;
    c->colmode = false;           // (slot order: a stale flag would send the COL kernels over slot-ordered records)
}
void state_to_fields(hens_ctx_impl* c) {
    if (!c->packed) return;
    const int64_t n = (int64_t)c->Tl * c->W;
    if (c->colmode) {
        const uint32_t* keys = iteration_keys(c) + (size_t)c->cfg.rung_begin * 8;   // (the order the last launch wrote: iteration c->iter's)
        hipLaunchKernelGGL(k_unpack_cols, dim3(grid_for(n)), dim3(256), 0, c->stream, c->wrec[c->cur], keys, c->L[c->cur],
                           c->P[c->cur], c->loc[c->cur], c->accepted, c->Tl, c->W, c->idx_bits);
        c->packed = c->colmode = false;
        return;
    }
    hipLaunchKernelGGL(k_unpack_state, dim3(grid_for(n)), dim3(256), 0, c->stream, c->wrec[c->cur], c->L[c->cur], c->P[c->cur],
                       c->loc[c->cur], c->accepted, n);
    c->packed = false;
    if (c->rows_mixed) {          // k_iter left accepted rows in the half the copying launches write next: fold them back
        hipLaunchKernelGGL(k_fold_rows, dim3(grid_for(n * (c->D / 2))), dim3(256), 0, c->stream, c->pool, c->loc[c->cur], n, c->D,
                           (int32_t)n, (int32_t)(c->parity * n));
        c->rows_mixed = false;
    }
}

// ---- the gate of the C entry points -----------------------------------------------------------------------------------------------
// hens_step leaves the walkers as packed records (slot or column order, after k_iter with rows in both halves of the pool) and the
// last cascade's ladder adaptation pending: a short call pays no pack / unpack and no k_adapt launch.  Every other entry point
// states here what it is about to use - the context's device, the by-field arrays L / P / loc / accepted, the ladder with its swap
// counts - behind its argument and state checks (a refused call settles nothing), and nothing else calls state_to_fields or
// flush_adapt but the stepping internals.
enum : unsigned { NEED_DEVICE = 1, NEED_FIELDS = 2, NEED_LADDER = 4 };
int settle(hens_ctx_impl* c, unsigned need) {
    if (need & NEED_DEVICE) HIPCHK(c, hipSetDevice(c->cfg.device_id));
    if (need & NEED_FIELDS) state_to_fields(c);
    if (need & NEED_LADDER) flush_adapt(c);
    return HENS_OK;
}
#define SETTLE(c, need)                                     \
    do {                                                    \
        if (const int s_ = settle(c, need)) return s_;      \
    } while (0)

// preconditions of the leaf-packing entry points, one spelling each: the context's kind; a model set on it
bool is_rj(const hens_ctx_impl* c) { return c->cfg.likelihood_kind == HENS_LIKE_TEMPLATE; }
int need_rj_context(hens_ctx_impl* c) {
    return is_rj(c) ? HENS_OK : fail(c, HENS_ERR_STATE, "hens_rj_* needs a context created with HENS_LIKE_TEMPLATE");
}
bool rj_has_model(const hens_ctx_impl* c) { return is_rj(c) && c->have_like && c->rj.M.nb > 0 && c->rj.acc_bd; }
int need_rj_model(hens_ctx_impl* c) { return rj_has_model(c) ? HENS_OK : fail(c, HENS_ERR_STATE, "hens_rj_set_model first"); }

// round keys of iteration c->iter (planning a new window if the chain has left the current one)
const uint32_t* iteration_keys(hens_ctx_impl* c) {
    // (the window must hold the NEXT iteration's keys too: column-ordered records are written in its order)
    if (c->iter < c->ikeys_iter0 || c->iter + 1 >= c->ikeys_iter0 + (uint64_t)c->ikeys_n) {
        PlanArgs pa{};
        pa.iter0 = c->iter; pa.seed = c->cfg.seed;
        // (a pipeline rank settles the pair across its bottom boundary: the column map of the cold neighbour's hottest rung too)
        const int below = c->cfg.rung_begin > 0 ? 1 : 0;
        pa.Tl = c->Tl + below; pa.W = c->W; pa.rung_begin = c->cfg.rung_begin - below; pa.T = c->T; pa.cb = c->label_cb;
        pa.keys = c->ikeys;
        if (c->aql_now) {       // (same queue as the launches that read the window: ordered by the packets' barrier bits)
            static const hens_aql::Kernel* ak_[64] = {};
            const int nbk = KEY_WINDOW;
            if (aql_launch(c, ak_, k_plan_keys, dim3((KEY_WINDOW * pa.Tl + 255) / 256), 256, 0, false, pa, nbk)) c->aql_failed = true;
        } else
            hipLaunchKernelGGL(k_plan_keys, dim3((KEY_WINDOW * pa.Tl + 255) / 256), dim3(256), 0, c->stream, pa, KEY_WINDOW);
        c->ikeys_iter0 = c->iter;
        c->ikeys_n = KEY_WINDOW;
        c->timing.n_plan += 1;
    }
    return c->ikeys + (size_t)(c->iter - c->ikeys_iter0) * c->T * 8;
}

// ---- the launches on walker records -----------------------------------------------------------------------------------------------
// the in-place first launch (k_stretch_fast / k_stretch2): first half-step, draws in registers (stretch_draws_at) from the
// iteration's round keys; the caller attaches the iteration's head
StretchArgs inplace_first_args(hens_ctx_impl* c, const uint32_t* keys) {
    StretchArgs a = base_args(c);
    a.wrec = c->wrec[c->cur];
    a.inplace = 1;
    a.ikeys = keys;
    a.iseed = c->cfg.seed; a.iiter = c->iter; a.ia = c->cfg.a;
    a.idx_bits = c->idx_bits; a.hb_shift = c->label_cb_shift - 1; a.ndim_active = dim_active(c);
    a.split = 0;
    a.home_off = c->parity * c->Tl * c->W;
    // (column-ordered records.  Round 3 also built the rung's row table staged in LDS by LDS-DMA: verified, measured at config 2
    //  on one box at 19.1 us per iteration against 18.8 without - 8 MB of table fills per launch and a wait for every load of
    //  the wave in front of the first barrier cost more than the L2 hits they replace - and removed in round 4.)
    a.col = c->colmode ? 1 : 0;
    return a;
}
// what FusedArgs (k_split1_pt) and IterArgs (k_iter) have in common
template <class Args>
void record_launch_args(hens_ctx_impl* c, Args& f) {
    f.pool = c->pool;
    f.wrec = c->wrec[c->cur]; f.wrecnew = c->wrec[c->cur ^ 1];
    f.loc = c->loc[c->cur]; f.locnew = c->loc[c->cur ^ 1];
    f.betas = c->betas[c->bcur];
    f.accepted = c->accepted;
    f.lo = c->lo; f.hi = c->hi; f.mu = c->mu; f.prec = c->prec; f.prec_sym = c->prec_sym;
    f.period = c->period;
    f.flags = c->flags;
    f.trace = (c->tracing && c->trace_fused) ? c->d_trace : nullptr;
    f.logp_in = c->logp_in; f.fill = c->cfg.fill_value; f.rosen_a = c->rosen_a; f.rosen_b = c->rosen_b;
    f.iter = c->iter; f.seed = c->cfg.seed;
    f.T = c->T; f.W = c->W; f.idx_bits = c->idx_bits;
    f.cb = c->label_cb; f.cb_shift = c->label_cb_shift;
}
// the second launch (k_split1_pt): second half-step + cascade + swap counts; the caller adds where the counts go (and, on a
// pipeline rank, the boundaries)
FusedArgs second_launch_args(hens_ctx_impl* c, const uint32_t* keys) {
    FusedArgs f{};
    record_launch_args(c, f);
    f.keys = keys;
    f.keys_next = keys + (size_t)c->T * 8;                             // (inside the window: iteration_keys)
    f.a = c->cfg.a; f.ndim_active = dim_active(c);
    return f;
}
int launch_second(hens_ctx_impl* c, const FusedArgs& f, LaunchTimer* tm, bool pipe) {
    const LikeKernels* lk = like_kernels(c->cfg.likelihood_kind);
    if (!lk) return fail(c, HENS_ERR_UNSUPPORTED, "no fused kernel for likelihood kind %d", c->cfg.likelihood_kind);
    const dim3 grid(pipe ? c->W / c->pipe.cbl : c->W / c->label_cb);
    const int NW = fast_nw(c->D);
    // the instantiation: column order knows neither periodic parameters nor short tiles, a pipeline rank no short tiles (step_path
    // refuses)
    const bool col = c->colmode, plain = !pipe && !col, per = !col && f.period, shrt = plain && c->T * c->label_cb != 2 * TILE;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    time_launch(c, tm, 2, e0, e1);
    // (the iteration's last launch: the call's last one carries the completion signal)
    return launch_by_ptr(c, lk->split1_pt(c->D, per, shrt, pipe, col), "k_split1_pt", grid, NW * 64, fused_lds_bytes(c->D, NW, lk->like, pipe),
                         c->aql_last, e0, e1, f);
}

// one Philox iteration in two launches: first half-step (k_stretch_fast, carrying the pending ladder adaptation), then
// second half-step + cascade + swap counts (k_split1_pt)
int fused_iteration(hens_ctx_impl* c, const StepPath& path, LaunchTimer* tm) {
    if (!c->packed) {                        // (the pack kernel - first call after another entry point - runs on the HIP stream)
        const int r = hip_interlude(c, [&] { state_to_records(c, path.col); });
        if (r) return r;
    }
    if (c->adapt_pending && !can_fold_adapt(c)) {
        // an adaptation that cannot ride in the first launch (HENS_NO_FOLD=1; counts in more rows than a wave sums) is a kernel of
        // its own on the HIP stream: the AQL queue drains first - its last packets are the previous cascade, which wrote the counts,
        // and nothing orders the two queues but the host (round 4 launched it from attach_iteration_head beside the queued packets)
        const int r = hip_interlude(c, [&] { flush_adapt(c); });
        if (r) return r;
    }
    const uint32_t* keys = iteration_keys(c);
    if (c->aql_failed) { c->aql_failed = false; return HENS_ERR_HIP; }
    // DEV PROBES (dev builds, timing only), HENS_AQL_NOBAR: bit 1 - the first launch's packet without the barrier bit; bit 0 - the
    // second launch's (the chain is WRONG): what would it buy at most - its workgroups start as the first launch's retire, with
    // no dependency at all (round 5, VERDICT r4 #2: the ceiling of "overlap launch 2's prologue with launch 1's drain" before
    // anyone builds the arrival counters)
    const int nobar = DEV_BUILD && c->aql_now ? env().aql_nobar : 0;
    {
        StretchArgs a = inplace_first_args(c, keys);
        attach_iteration_head(c, a);
        if ((nobar & 2) && c->aql.windex != c->aql.call_first) c->aql.nobar_next = true;
        c->aql.norel_next = norel_ok(c);
        c->aql.prof_kind = 0;
        a.norel = c->aql.norel_next ? 1 : 0;
        const int r = launch_stretch_timed<MODE_STRETCH>(c, a, (c->N0 + TILE - 1) / TILE, tm);
        if (r) return r;
    }
    FusedArgs f = second_launch_args(c, keys);
    f.swap_acc = acc_take(c);
    f.acc_rows = 8 * acc_row_groups(c->T);
    acc_commit(c);
    if (nobar & 1) c->aql.nobar_next = true;
    c->aql.norel_next = norel_ok(c);
    c->aql.prof_kind = 2;
    f.norel = c->aql.norel_next ? 1 : 0;
    const int r = launch_second(c, f, tm, false);
    if (r) return r;
    // (no change of c->parity: the rows were updated in place, the half of the pool that the copying launches of the
    // other paths write next is still the free one)
    c->num_proposals += 1;
    cascade_ran(c, f.swap_acc, f.acc_rows, c->cfg.adaptive != 0);      // acc_rows rows (see hens_ctx_impl::swap_acc)
    if (DEV_BUILD && env().debug_noflip) c->cur ^= 1;     // HENS_DEBUG_NOFLIP: timing experiments with cut kernels (HENS_CUT_F) - no flip
    return HENS_OK;
}

// the same two launches on a rank of the ladder pipeline
// mh: the iteration's move is the full-ensemble Metropolis-Hastings launch (in place, in the records; every guest goes home
// in it), and the second launch is the cascade alone (FusedArgs::no_move)
int mh_iteration(hens_ctx_impl* c, LaunchTimer* tm, bool inplace = false);
int pipe_fused_iteration(hens_ctx_impl* c, const StepPath& path, LaunchTimer* tm, bool mh) {
    state_to_records(c, path.col);
    const uint32_t* keys = iteration_keys(c);
    if (mh) {
        const int r = mh_iteration(c, tm, true);
        if (r) return r;
    } else {
        StretchArgs a = inplace_first_args(c, keys);
        a.ghome = c->pipe.ghome;
        a.sys_all = pipe_has_top(c) ? 1 : 0;
        attach_iteration_head(c, a);               // waits for the previous sweep's arrivals, carries the pending adaptation
        const int r = launch_stretch_timed<MODE_STRETCH>(c, a, (c->N0 + TILE - 1) / TILE, tm);
        if (r) return r;
    }
    FusedArgs f = second_launch_args(c, keys);      // (periodic parameters: set before hens_pipe_init, the same on every rank)
    f.Tl = c->Tl; f.rung_begin = c->cfg.rung_begin;
    f.cbl = c->pipe.cbl; f.cbl_shift = c->pipe.cbl_shift;
    f.guest_delta = guest_delta(c);
    f.ghome = c->pipe.ghome;
    f.box = c->pipe.box;
    f.box_hot = pipe_has_top(c) ? c->pipe.boxes[c->pipe.rank + 1] : nullptr;
    f.box_cold = pipe_has_bot(c) ? c->pipe.boxes[c->pipe.rank - 1] : nullptr;
    f.pool_cold = c->pipe.pool_cold;
    f.swap_acc = c->pipe.acc[c->pipe.sweep & 1u];
    f.acc_rows = pipe_acc_rows(c);
    f.stats = c->pipe.stats;
    f.budget = c->pipe.budget;
    f.sweep = c->pipe.sweep;
    f.par = (int)(c->pipe.sweep & 1u);
    f.nranks = c->pipe.nranks; f.rank = c->pipe.rank;
    f.sys_rows = pipe_has_top(c) ? 1 : 0;           // (measured on one GPU: system-scope row stores cost nothing over sc1)
    f.no_move = mh ? 1 : 0;
    const int r = launch_second(c, f, tm, true);
    if (r) return r;
    if (!mh) c->num_proposals += 1;
    pipe_finish_sweep(c);                          // queues this sweep's counts for the adaptation, flips the record buffers
    return HENS_OK;
}

// one launch per iteration (k_iter) from the planned records of batch slot `ib`
int iter_iteration(hens_ctx_impl* c, const StepPath& path, int ib, LaunchTimer* tm) {
    if (!c->packed) {
        const int r = hip_interlude(c, [&] { state_to_records(c, path.col); });
        if (r) return r;
    }
    if (c->adapt_pending && !(is_acc_buffer(c, c->adapt_src) && c->T <= 128)) {   // (counts of an MH iteration's cascade)
        const int r = hip_interlude(c, [&] { flush_adapt(c); });
        if (r) return r;
    }
    const LikeKernels* lk = like_kernels(c->cfg.likelihood_kind);
    if (!lk) return fail(c, HENS_ERR_UNSUPPORTED, "no one-launch kernel for likelihood kind %d", c->cfg.likelihood_kind);
    IterArgs f{};
    record_launch_args(c, f);                    // (betas: the ladder the folded adaptation reads, before it is handed over)
    const size_t roff = (size_t)ib * rec_per_iter(c);
    f.rec1 = c->db[0].rec1 + roff; f.rec2 = c->db[0].rec + roff; f.rec3 = c->db[0].rec3 + roff;
    f.keys = c->db[0].keys + (size_t)ib * c->T * 8;
    f.swap_acc = acc_take(c);
    f.acc_rows = 8 * acc_row_groups(c->T);
    if (c->adapt_pending) {
        f.ad_on = 1;
        f.ad = adapt_args(c, c->adapt_pending_adaptive, c->betas[c->bcur], c->betas[c->bcur ^ 1]);
        acc_fold(c, f.ad);
        adapt_taken(c, true);
    }
    acc_commit(c);
    f.half_rows = c->T * c->W;
    c->aql.norel_next = norel_ok(c);
    f.norel = c->aql.norel_next ? 1 : 0;
    c->aql.prof_kind = 3;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    time_launch(c, tm, 3, e0, e1);
    constexpr int NW = 8;
    const int r = launch_by_ptr(c, lk->iter(c->D, f.period != nullptr), "k_iter", dim3(c->W / c->label_cb), NW * 64, iter_lds_bytes(c->D, NW),
                                c->aql_last, e0, e1, f);
    if (r) return r;
    c->rows_mixed = true;
    c->num_proposals += 1;
    cascade_ran(c, f.swap_acc, f.acc_rows, c->cfg.adaptive != 0);
    return HENS_OK;
}

int ensure_mh_buffers(hens_ctx_impl* c) {
    if (c->mh_step) return HENS_OK;
    const size_t TW = (size_t)c->Tl * c->W;
    int r;
    if ((r = dalloc(c, &c->mh_step, TW * c->D))) return r;
    if ((r = dalloc(c, &c->mh_lu, TW))) return r;
    if ((r = dalloc(c, &c->mh_u, TW))) return r;
    if ((r = dalloc(c, &c->mh_keep, TW))) return r;
    if ((r = dalloc(c, &c->mh_scale, (size_t)c->D * c->D))) return r;
    if ((r = dalloc(c, &c->accepted_mh, TW))) return r;
    HIPCHK(c, hipMemsetAsync(c->accepted_mh, 0, TW * 4, c->stream));
    return HENS_OK;
}

// one full-ensemble MH proposal from the step rows / log-uniforms already in mh_step / mh_lu (mh.py:56-193)
int mh_launch(hens_ctx_impl* c, bool want_keep, LaunchTimer* tm, bool inline_draws = false, bool inplace = false) {
    StretchArgs a = base_args(c);
    a.split = 0;
    a.home_off = c->parity * c->Tl * c->W;
    if (c->packed) { a.wrec = c->wrec[c->cur]; inplace = true; }  // hens_step's record mode: {L, P} in the records
    a.inplace = inplace ? 1 : 0;
    a.mh_step = inline_draws ? nullptr : c->mh_step;
    a.mh_scale = c->mh_scale; a.mh_kind = c->mh_kind; a.mh_iter = c->iter; a.mh_seed = c->cfg.seed;
    a.dr.lu = c->mh_lu;
    a.accepted = c->accepted_mh;
    a.keep_out = want_keep ? c->mh_keep : nullptr;
    if (c->pipe.fused) {                           // fused pipeline iteration: every guest goes home in this launch
        a.ghome = c->pipe.ghome;
        a.sys_all = pipe_has_top(c) ? 1 : 0;
    }
    attach_iteration_head(c, a);
    attach_publish(c, a, true, (c->W + TILE - 1) / TILE);
    const int r = launch_stretch_timed<MODE_MH>(c, a, (c->W + TILE - 1) / TILE, tm);
    if (r) return r;
    if (!inplace) c->parity ^= 1;                  // (in place: the free half of the pool stays the free one)
    c->num_proposals_mh += 1;
    return HENS_OK;
}

// DistributionGenerate (hens_dist.h): one full-ensemble proposal from the generator in the MH slot.  forced: the caller's points
// and log-uniforms are in mh_step / mh_lu (hens_dist_step); else the launch draws both (hens_step).  Always in place, the pool's
// parity stays; on the HIP stream with its release.  A pending ladder adaptation runs as a kernel of its own in front of it.
// MH_MT_DIST: the same launch site for k_mt_dist (hens_mt.h) - the tries and pick uniforms of a forced call are in mt_q / mt_upick,
// `want_mt`: pick_out and lsw_out are staged as well.
int dist_launch(hens_ctx_impl* c, bool forced, bool want_keep, bool want_factors, LaunchTimer* tm, bool want_mt = false) {
    const bool mt = c->mh_kind == MH_MT_DIST;
    const char* what = mt ? "k_mt_dist" : "k_dist";
    const LikeKernels* lk = like_kernels(c->cfg.likelihood_kind);
    const void* fn = lk ? (mt ? lk->mt_dist(c->D) : lk->dist(c->D)) : nullptr;
    if (!fn) return fail(c, HENS_ERR_UNSUPPORTED, "%s: no such instantiation in this build (ndim %d, likelihood kind %d)", what, c->D, c->cfg.likelihood_kind);
    flush_adapt(c);
    MtArgs a{};
    a.pool = c->pool;
    a.loc = c->loc[c->cur];
    a.L = c->L[c->cur];
    a.P = c->P[c->cur];
    a.wrec = c->packed ? c->wrec[c->cur] : nullptr;        // hens_step's record mode (slot order: no column order with an MH move set)
    a.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    a.lo = c->prior ? c->prior_block.lo() : c->lo;
    a.hi = c->prior ? c->prior_block.hi() : c->hi;
    a.pterms = c->prior;
    a.glo = c->dist_block.lo();
    a.ghi = c->dist_block.hi();
    a.gterms = c->dist_block.terms();
    a.q = forced ? (mt ? c->mt_q : c->mh_step) : nullptr;
    a.lu = forced ? c->mh_lu : nullptr;
    a.accepted = c->accepted_mh;
    a.keep_out = want_keep ? c->mh_keep : nullptr;
    a.factors_out = want_factors ? c->dist_factors : nullptr;
    a.mu = c->mu; a.prec = c->prec; a.prec_sym = c->prec_sym;
    a.flags = c->flags;
    a.logp_in = c->logp_in;
    a.fill = c->cfg.fill_value;
    a.rosen_a = c->rosen_a; a.rosen_b = c->rosen_b;
    a.seed = c->cfg.seed; a.iter = c->iter;
    a.Tl = c->Tl; a.W = c->W; a.rung_begin = c->cfg.rung_begin; a.tempered = c->cfg.tempered;
    const int NW = fast_nw(c->D);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    time_launch(c, tm, 0, e0, e1);
    int r;
    if (mt) {                                              // KP tries' rows per walker, 64 / KP walkers per workgroup
        a.K = c->mt_K;
        while ((1 << a.kp_shift) < a.K) a.kp_shift += 1;
        a.u_pick = forced ? c->mt_upick : nullptr;
        a.pick_out = want_mt ? c->mt_pick : nullptr;
        a.lsw_out = want_mt ? c->mt_lsw : nullptr;
        const int G = TILE >> a.kp_shift;
        const dim3 grid((c->W + G - 1) / G, c->Tl);
        r = on_hip_stream(c, [&] { return launch_by_ptr(c, fn, what, grid, NW * 64, prior_lds_bytes(c->D, NW, lk->like), false, e0, e1, a); });
    } else {
        const dim3 grid((c->W + TILE - 1) / TILE, c->Tl);  // (never on the AQL queue: aql_able requires mh_kind < 0)
        r = on_hip_stream(c, [&] { return launch_by_ptr(c, fn, what, grid, NW * 64, prior_lds_bytes(c->D, NW, lk->like), false, e0, e1, static_cast<const DistArgs&>(a)); });
    }
    if (r) return r;
    c->num_proposals_mh += 1;
    return HENS_OK;
}

// Philox mode: draw the iteration's steps and accept uniforms on the device, then propose.  Isotropic and
// axis-aligned proposals on the fast row widths are drawn inside the MH launch itself (one Box-Muller pair per
// lane); a full covariance (Cholesky product) and the generic row widths go through k_mh_draw + the step buffer.
int mh_iteration(hens_ctx_impl* c, LaunchTimer* tm, bool inplace) {
    if (c->mh_kind == MH_DIST || c->mh_kind == MH_MT_DIST) return dist_launch(c, false, false, false, tm);      // (in place in either state form)
    const bool inline_draws = c->mh_kind != MH_FULL && fast_path(c);
    if (!inline_draws) {
        MhDrawArgs d{};
        d.step = c->mh_step; d.lu = c->mh_lu; d.scale = c->mh_scale;
        d.iter = c->iter; d.seed = c->cfg.seed;
        d.Tl = c->Tl; d.W = c->W; d.D = c->D; d.rung_begin = c->cfg.rung_begin; d.kind = c->mh_kind;
        d.block = gibbs_on(c) ? (uint32_t)c->gibbs[1].cur : 0u;
        size_t lds = (size_t)64 * (c->D + 1) * 8;
        d.chol_lds = (c->mh_kind == MH_FULL && lds + (size_t)c->D * (c->D + 1) * 8 <= 60000) ? 1 : 0;
        if (d.chol_lds) lds += (size_t)c->D * (c->D + 1) * 8;
        hipLaunchKernelGGL(k_mh_draw, dim3((c->W + 63) / 64, c->Tl), dim3(256), lds, c->stream, d);
    }
    return mh_launch(c, false, tm, inline_draws, inplace);
}

// host-side move choice of hens_step (ensemble.py:971 in Philox form): one counter-based uniform per iteration
uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
double move_uniform(uint64_t seed, uint64_t it) {
    uint32_t c0 = (uint32_t)it, c1 = (uint32_t)(it >> 32), c2 = 0, c3 = PURPOSE_MOVE;
    uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        const uint32_t n0 = hi1 ^ c1 ^ k0, n1 = lo1, n2 = hi0 ^ c3 ^ k1, n3 = lo0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    const uint64_t v = ((uint64_t)c0 << 32) | c1;
    return (double)(v >> 11) * (1.0 / 9007199254740992.0);
}
bool iteration_is_mh(const hens_ctx_impl* c, uint64_t iter) {
    if (c->mh_kind < 0 || c->mh_weight <= 0.0) return false;
    return c->mh_weight >= 1.0 || move_uniform(c->cfg.seed, iter) < c->mh_weight;
}
bool iteration_is_mh(const hens_ctx_impl* c) { return iteration_is_mh(c, c->iter); }

// ---- reversible-jump leaf packing ---------------------------------------------------------------------------------------
// RjArgs::ctab / cbn from the model (hens_rj_set_model, hens_rj_set_mh_scale): per record coordinate its box, step scale, the
// branch's leaf log-density and (branch, leaf slot, dimension, leaf kind)
int rj_push_ctab(hens_ctx_impl* c) {
    const RjModel& M = c->rj.M;
    std::vector<double> tab(RJ_CTAB_ROWS * RJ_MAX_RW, 0.0);
    std::vector<int32_t> bn(RJ_MAX_RW, 0);
    for (int b = 0; b < M.nb; ++b)
        for (int n = 0; n < M.nl[b]; ++n)
            for (int d = 0; d < M.nd[b]; ++d) {
                const int i = M.off[b] + n * M.nd[b] + d;
                tab[RJ_CTAB_LO + i] = M.lo[b][d]; tab[RJ_CTAB_HI + i] = M.hi[b][d];
                tab[RJ_CTAB_SCALE + i] = M.mh_scale[b][d]; tab[RJ_CTAB_LOGP + i] = M.leaf_logp[b];
                tab[RJ_CTAB_PERIOD + i] = c->rj.per_on ? c->rj.period[b][d] : 0.0;
                if (c->rj.have_chol && d < RJ_ND)
                    for (int j = 0; j < RJ_ND; ++j) tab[RJ_CTAB_CHOL + j * RJ_MAX_RW + i] = c->rj.chol[b][d][j];
                bn[i] = b | (n << 4) | (d << 10) | (M.kind[b] << 12) | ((M.slot0[b] + n) << 16);
                if (M.prior_on) {                         // the coordinate's prior term record (hens_rj_set_prior_terms)
                    const PriorTerm& t = c->rj.terms[b][d];
                    tab[RJ_CTAB_C0 + i] = t.c0; tab[RJ_CTAB_C1 + i] = t.c1; tab[RJ_CTAB_C2 + i] = t.c2;
                    bn[i] |= t.kind << 24;
                }
            }
    int r;
    if (!c->rj.ctab) {
        if ((r = dalloc(c, &c->rj.ctab, tab.size()))) return r;
        if ((r = dalloc(c, &c->rj.cbn, bn.size()))) return r;
    }
    HIPCHK(c, hipMemcpyAsync(c->rj.ctab, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.cbn, bn.data(), bn.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the vectors go out of scope)
    return HENS_OK;
}
// One k_rj launch, said in full.  The context supplies only what is state: the walkers, the resident templates, the pending
// ladder adaptation (and Rj::defer_adapt, whether it may ride in this launch).
struct RjLaunch {
    int mode = RJ_MODE_EVAL, branch = 0;
    int tm_mode = -1;                       // RjArgs::tm_mode; -1: no resident templates (the reference's order of operations, bit for bit)
    int ns = 0, split = 0;                  // stretch half-step: walkers of the moving half per rung; PHILOX: which half it is
    enum Draws { PHILOX, FORCED } draws = PHILOX;      // FORCED: the caller's draws, staged on the device - u_acc and what the mode reads
    const double* step = nullptr; const int8_t* change = nullptr; const int32_t* leaf = nullptr; const double* birth = nullptr;
    const int32_t* st_own = nullptr; const int32_t* st_cw = nullptr; const double* st_uzz = nullptr; const double* u_acc = nullptr;
    uint8_t* keep = nullptr;                // RjArgs::keep_out
    double* P_out = nullptr;                // RjArgs::P in place of the context's log-priors (rj_evaluate: a refresh leaves them alone)
    bool propose = false;                  // the proposal half of a host-callable move (k_rj<MODE, -2>); k_rj_accept finishes it
    // the multiple-try birth / death move (k_rj_mt, hens_rj_set_mt_proposal) in place of k_rj<RJ_MODE_BD>: FORCED: the caller's tries and
    // pick uniforms (birth unused); mt_out: RjMtArgs::out
    bool mt = false;
    const double* tries = nullptr; const double* u_pick = nullptr; double* mt_out = nullptr;
    // the in-model Gaussian move under a Gibbs block table (k_rj_gibbs, hens_rj_set_gibbs) in place of k_rj<RJ_MODE_MH>: blocks [gb0, gb1)
    bool gibbs = false;
    int gb0 = 0, gb1 = 0;
    const int32_t* gr_pick = nullptr;       // RJ_MODE_GROUP, FORCED: the caller's picks (with st_uzz, u_acc)
};
RjLaunch rj_eval() { return RjLaunch{RJ_MODE_EVAL, 0, 0}; }      // every row's templates, log-likelihood and log-prior from its coordinates
// a Philox move of hens_rj_step: on the resident templates where the model has them, birth / death by difference; `split`: that
// half of the red / blue stretch move (red_blue.py:150-154: set k has ceil((W - k) / 2) walkers)
RjLaunch rj_production(const hens_ctx_impl* c, int mode, int branch = 0, int split = 0) {
    return RjLaunch{mode, branch, !c->rj.tm ? -1 : (mode == RJ_MODE_BD ? 1 : 0), split == 0 ? (c->W + 1) / 2 : c->W / 2, split};
}
// a teacher-forced move on the draws in the staging buffers (rj_ensure_staging); the move sets branch / ns
RjLaunch rj_forced(const hens_ctx_impl* c, int mode, bool propose) {
    const hens_ctx_impl::Rj& s = c->rj;
    RjLaunch l{mode};
    l.draws = RjLaunch::FORCED; l.propose = propose; l.u_acc = s.u; l.keep = propose ? nullptr : s.keep;
    if (mode == RJ_MODE_MH) l.step = s.step;
    if (mode == RJ_MODE_BD) { l.change = s.change; l.leaf = s.leaf; l.birth = s.birth; }
    if (mode == RJ_MODE_STRETCH) { l.st_own = s.st_own; l.st_cw = s.st_cw; l.st_uzz = s.uzz; }
    return l;
}
// where a move's accepts are counted.  "iterate_branches": the move's accept mask is the LAST branch's (rj.py:385-386) - in both
// modes, so the counters of hens_rj_step and of the parity API (one hens_rj_bd_step per branch) mean the same thing
uint32_t* rj_accept_counter(const hens_ctx_impl* c, int mode, int branch) {
    return mode != RJ_MODE_BD ? c->accepted : (c->rj.schedule == 1 && branch != c->rj.M.nb - 1 ? nullptr : c->rj.acc_bd);
}
// k_rj's instantiations: (mode, template scheme or -1 none / -2 proposal half or log-prior alone, Philox in-model move that forms L z,
// a model with leaf kinds beyond pulse / sine)
// ... , the stretch half-step under periodic leaf parameters: hens_rj_set_periodic)
struct RjInst { int mode, tmm; bool chol, wide, per; void (*k)(const RjArgs); };
#define RJ_INST(MODE_, TMM_, CHOL_) {MODE_, TMM_, CHOL_, false, false, k_rj<MODE_, TMM_, CHOL_>}
#define RJ_INST_WIDE(MODE_, TMM_) {MODE_, TMM_, false, true, false, k_rj<MODE_, TMM_, false, true>}
#define RJ_INST_PER(TMM_, WIDE_) {RJ_MODE_STRETCH, TMM_, false, WIDE_, true, k_rj<RJ_MODE_STRETCH, TMM_, false, WIDE_, true>}
const RjInst RJ_INSTS[] = {        // (listed in the order the code object has had them since they were an if-chain)
    RJ_INST(RJ_MODE_MH, 0, true), RJ_INST(RJ_MODE_MH, -1, true), RJ_INST(RJ_MODE_EVAL, -1, false), RJ_INST(RJ_MODE_EVAL, 0, false), RJ_INST(RJ_MODE_EVAL, 2, false),
    RJ_INST(RJ_MODE_MH, -1, false), RJ_INST(RJ_MODE_MH, 0, false), RJ_INST(RJ_MODE_BD, -1, false), RJ_INST(RJ_MODE_BD, 1, false),
    RJ_INST(RJ_MODE_STRETCH, -1, false), RJ_INST(RJ_MODE_STRETCH, 0, false),
    RJ_INST(RJ_MODE_MH, -2, false), RJ_INST(RJ_MODE_BD, -2, false), RJ_INST(RJ_MODE_STRETCH, -2, false), RJ_INST(RJ_MODE_EVAL, -2, false),
    RJ_INST_WIDE(RJ_MODE_EVAL, -1), RJ_INST_WIDE(RJ_MODE_EVAL, 0), RJ_INST_WIDE(RJ_MODE_EVAL, 2), RJ_INST_WIDE(RJ_MODE_MH, -1), RJ_INST_WIDE(RJ_MODE_MH, 0),
    RJ_INST_WIDE(RJ_MODE_BD, -1), RJ_INST_WIDE(RJ_MODE_BD, 1), RJ_INST_WIDE(RJ_MODE_STRETCH, -1), RJ_INST_WIDE(RJ_MODE_STRETCH, 0),
    RJ_INST(RJ_MODE_GROUP, -1, false), RJ_INST(RJ_MODE_GROUP, 0, false), RJ_INST_WIDE(RJ_MODE_GROUP, -1), RJ_INST_WIDE(RJ_MODE_GROUP, 0),
    RJ_INST_PER(-1, false), RJ_INST_PER(0, false), RJ_INST_PER(-2, false), RJ_INST_PER(-1, true), RJ_INST_PER(0, true),
};
#undef RJ_INST_PER
#undef RJ_INST
#undef RJ_INST_WIDE

int rj_launch(hens_ctx_impl* c, const RjLaunch& l) {
    const int mode = l.mode;
    RjArgs a{};
    if (c->tracing && c->trace_rj == mode) { a.trace = c->d_trace; a.trace_n = (int32_t)(c->trace_words / 8); }
    a.tm = (l.tm_mode >= 0) ? c->rj.tm : nullptr;
    a.tm_mode = l.tm_mode >= 0 ? l.tm_mode : 0;
    a.pool = c->pool; a.loc = c->loc[c->cur]; a.L = c->L[c->cur]; a.P = l.P_out ? l.P_out : c->P[c->cur];
    a.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    a.accepted = rj_accept_counter(c, mode, l.branch); a.keep_out = l.keep;
    a.tdata = c->rj.t; a.ydata = c->rj.y; a.ctab = c->rj.ctab; a.cbn = c->rj.cbn;
    a.step = l.step; a.change = l.change; a.leaf = l.leaf; a.birth = l.birth; a.u_acc = l.u_acc;
    a.flags = c->flags; a.fill = c->cfg.fill_value; a.iter = c->iter; a.seed = c->cfg.seed;
    a.M = c->rj.M;
    a.per_on = c->rj.per_on ? 1 : 0;
    a.Tl = c->Tl; a.W = c->W; a.rung_begin = c->cfg.rung_begin; a.tempered = c->cfg.tempered; a.mode = mode; a.branch = l.branch;
    if (c->adapt_pending) {
        // the adaptation behind the last cascade: inside this launch (production launches that test against the ladder, up to 64
        // rungs: RjArgs::ad), else as a launch of its own in front of it
        if (c->rj.defer_adapt && a.tm && mode != RJ_MODE_EVAL && c->T <= 64 && c->Tl == c->T && c->rj.ad_flag && !c->adapt_src) {
            a.ad = adapt_args(c, c->adapt_pending_adaptive, c->betas[c->bcur], c->betas[c->bcur]);
            a.ad_fold = 1;
            a.ad_serial = ++c->rj.ad_serial;
            a.ad_flag = c->rj.ad_flag;
            adapt_taken(c, false);                // (same ladder buffer: no flip; adapt_src is nullptr already)
        } else {
            flush_adapt(c);
        }
    }
    if (mode == RJ_MODE_STRETCH) {                    // (a half-step: one wavefront per position of the moving half, l.ns of them per rung)
        a.st_a = c->cfg.a; a.st_ns = l.ns;
        if (l.draws == RjLaunch::FORCED) { a.st_own = l.st_own; a.st_cw = l.st_cw; a.st_uzz = l.st_uzz; }
        else a.st_hb = l.split | (c->idx_bits << 8);                                              // (Philox, st_own == nullptr)
    }
    if (mode == RJ_MODE_GROUP) {                      // (hens_rj_set_group saw to a device likelihood and at most 64 slots)
        const hens_ctx_impl::Rj& s = c->rj;
        if (s.gr_nf == 0 || l.propose) return fail(c, HENS_ERR_STATE, "k_rj<RJ_MODE_GROUP>: no group set (hens_rj_set_group)");
        a.st_a = s.gr_a;
        a.G.keys = s.gr_keys; a.G.tab = s.gr_tab; a.G.cnt = s.gr_cnt; a.G.start = s.gr_start; a.G.snap = s.gr_snap;
        a.G.nfriends = s.gr_nf;
        for (int b = 0; b < RJ_MAX_BRANCH; ++b) { a.G.koff[b] = s.gr_koff[b]; a.G.key[b] = s.gr_key[b]; }
        if (l.draws == RjLaunch::FORCED) { a.G.pick = l.gr_pick; a.st_uzz = l.st_uzz; }
    }
    const int npr = mode == RJ_MODE_STRETCH ? l.ns : c->W;            // waves per rung
    const dim3 grid((unsigned)((npr + RJ_WAVES - 1) / RJ_WAVES), (unsigned)c->Tl), block(RJ_WAVES * 64);
    int tmm = a.tm ? a.tm_mode : -1;                  // the instantiation: (mode, template scheme), see k_rj
    if (c->rj.general && mode == RJ_MODE_EVAL && !l.propose) tmm = -2;           // (no device likelihood: the log-prior alone)
    else if (c->rj.general && !l.propose) return fail(c, HENS_ERR_STATE, "a model without a device likelihood steps with hens_rj_propose / hens_rj_accept");
    if (l.propose) {                                  // hens_rj_propose: the proposal only, left where the host can fetch it
        if (a.tm || l.draws != RjLaunch::FORCED || mode == RJ_MODE_EVAL) return fail(c, HENS_ERR_STATE, "hens_rj_propose: a teacher-forced move with its accept uniforms");
        tmm = -2;
        a.hq = c->rj.hq; a.hlogp = c->rj.hlogp; a.hfac = c->rj.hfac; a.hlu = c->rj.hlu; a.hmoved = c->rj.hmoved;
    }
    if (l.mt) {                                       // (one branch, a model with a device likelihood: hens_rj_set_mt_proposal saw to both)
        const hens_ctx_impl::Rj& s = c->rj;
        RjMtArgs g{};
        g.A = a; g.tries = l.tries; g.u_pick = l.u_pick; g.out = l.mt_out;
        g.gen = s.mt_dens + (size_t)(2 * l.branch) * RJ_MAX_ND * RJ_MT_DENS;
        g.pri = g.gen + RJ_MAX_ND * RJ_MT_DENS;
        g.gen_logq = s.mt_gen_logq[l.branch]; g.gen_box = s.mt_gen_box[l.branch] ? 1 : 0;
        g.pri_logp = s.M.leaf_logp[l.branch]; g.pri_box = s.M.prior_on ? 0 : 1;
        g.K = s.mt_K;
        g.per_branch = (s.wide || s.M.prior_on) ? 0 : 1;      // (the order of k_rj's instantiation for this model)
        if (tmm != -1 && tmm != 1) return fail(c, HENS_ERR_STATE, "k_rj_mt: a birth / death launch, by difference or in full");
        hipLaunchKernelGGL(a.tm ? k_rj_mt<true> : k_rj_mt<false>, grid, block, 0, c->stream, g);
        const hipError_t em = hipGetLastError();
        if (em != hipSuccess) return fail(c, HENS_ERR_HIP, "k_rj_mt launch failed: %s", hipGetErrorString(em));
        return HENS_OK;
    }
    if (l.gibbs) {                                    // (a model with a device likelihood, the Gaussian move: hens_rj_set_gibbs saw to both)
        RjGibbsArgs g{};
        g.A = a; g.btab = c->rj.gb_tab; g.b0 = l.gb0; g.b1 = l.gb1;
        g.per_branch = (c->rj.wide || c->rj.M.prior_on) ? 0 : 1;      // (the order of k_rj's instantiation for this model)
        g.chol = (l.draws == RjLaunch::PHILOX && c->rj.have_chol) ? 1 : 0;
        if (mode != RJ_MODE_MH || (tmm != -1 && tmm != 0) || l.gb0 < 0 || l.gb1 > c->rj.gb_n || l.gb0 >= l.gb1)
            return fail(c, HENS_ERR_STATE, "k_rj_gibbs: an in-model launch over blocks of the table");
        hipLaunchKernelGGL(a.tm ? k_rj_gibbs<true> : k_rj_gibbs<false>, grid, block, 0, c->stream, g);
        const hipError_t eg = hipGetLastError();
        if (eg != hipSuccess) return fail(c, HENS_ERR_HIP, "k_rj_gibbs launch failed: %s", hipGetErrorString(eg));
        return HENS_OK;
    }
    const bool chol = mode == RJ_MODE_MH && l.draws == RjLaunch::PHILOX && c->rj.have_chol && tmm != -2;
    // (the proposal half of a host-callable move has the widths at run time already; a model under prior terms - pulses and sines
    //  too - takes the WIDE instantiations, whose per-point leaf values serve every kind: the box instantiations carry no terms)
    const bool wide = (c->rj.wide || c->rj.M.prior_on) && tmm != -2;
    const bool per = mode == RJ_MODE_STRETCH && c->rj.per_on;
    const RjInst* inst = nullptr;
    for (const RjInst& i : RJ_INSTS)
        if (i.mode == mode && i.tmm == tmm && i.chol == chol && i.wide == wide && i.per == per) inst = &i;
    if (!inst) return fail(c, HENS_ERR_INVALID, "k_rj: no instantiation for mode %d with template scheme %d", mode, tmm);
    hipLaunchKernelGGL(inst->k, grid, block, 0, c->stream, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, HENS_ERR_HIP, "k_rj launch failed: %s", hipGetErrorString(e));
    return HENS_OK;
}

// ---- the group stretch move's table (hens_rj_set_group; csrc/hens_rj_group.h) ----
// no group: the in-model move of hens_rj_step falls back to the Gaussian move
void rj_group_clear(hens_ctx_impl* c) {
    c->rj.gr_nf = 0; c->rj.gr_m = 0;
    if (c->rj.in_model == HENS_RJ_INMODEL_GROUP) c->rj.in_model = HENS_RJ_INMODEL_GAUSSIAN;
}
// the move's call number restarts, the table is empty and no leaf has a window (all of them are assigned by the rebuild that the
// first move is due, or - teacher-forced calls without one - as newborn leaves at the head of the next move)
int rj_group_reset(hens_ctx_impl* c) {
    const size_t rows = (size_t)2 * c->Tl * c->W;
    c->rj.gr_m = 0;
    HIPCHK(c, hipMemsetAsync(c->rj.gr_cnt, 0, RJ_MAX_BRANCH * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rj.gr_start, 0xff, rows * RJ_GROUP_SLOTS * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->rj.gr_snap, 0, rows * RJ_MAX_BRANCH * 4, c->stream));
    return HENS_OK;
}
// rule 1 and rule 3's "at a rebuild": count / scan / gather, stable sort by rank, every rung's windows - three launches on the
// context's stream, nothing allocated, nothing read back
int rj_group_rebuild(hens_ctx_impl* c) {
    const hens_ctx_impl::Rj& s = c->rj;
    RjGroupBuildArgs g{};
    g.pool = c->pool; g.loc = c->loc[c->cur]; g.M = s.M;
    g.gkey = s.gr_gkey; g.gsrc = s.gr_gsrc; g.keys = s.gr_keys; g.tab = s.gr_tab; g.cnt = s.gr_cnt; g.start = s.gr_start; g.snap = s.gr_snap;
    int cap = 0;
    for (int b = 0; b < RJ_MAX_BRANCH; ++b) { g.koff[b] = s.gr_koff[b]; g.key[b] = s.gr_key[b]; }
    for (int b = 0; b < s.M.nb; ++b) cap = std::max(cap, c->W * s.M.nl[b]);
    g.Tl = c->Tl; g.W = c->W; g.nfriends = s.gr_nf;
    hipLaunchKernelGGL(k_rj_group_gather, dim3((unsigned)s.M.nb), dim3(256), 0, c->stream, g);
    hipLaunchKernelGGL(k_rj_group_rank, dim3((unsigned)((cap + 255) / 256), (unsigned)s.M.nb), dim3(256), 0, c->stream, g);
    hipLaunchKernelGGL(k_rj_group_windows, dim3(grid_for((int64_t)c->Tl * c->W * RJ_GROUP_SLOTS)), dim3(256), 0, c->stream, g);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(c, HENS_ERR_HIP, "friend table rebuild failed: %s", hipGetErrorString(e));
    return HENS_OK;
}

// full evaluation; behind it the resident templates (where the model keeps them) are exactly those of the rows
// keep_logp: a REFRESH of a chain's templates and log-likelihoods (every 64 iterations, in front of a download, at the head of a
// call behind an upload that brought its logs) - the stored log-priors stay what the chain made them.  They are no function of the
// coordinates: under a Gibbs table fix_logp_gibbs stores 0.0 on a walker whose only leaves sit in non-member slots of the block's
// branches (hens_rj_gibbs.h, move.py:368-402), and the next accept test reads that 0.0.  The launch writes its log-priors aside.
int rj_evaluate(hens_ctx_impl* c, bool keep_logp = false) {
    RjLaunch l = rj_eval();
    if (keep_logp) {
        if (!c->rj.p_aside)
            if (const int ra = dalloc(c, &c->rj.p_aside, (size_t)c->Tl * c->W)) return ra;
        l.P_out = c->rj.p_aside;
    }
    const int r = rj_launch(c, l);
    if (!r) { c->rj.tm_valid = c->rj.tm != nullptr; c->rj.tm_drift = false; }
    return r;
}

// head of every stepping entry point.  propose: the proposal half of a host-callable move, the one way a model without a device likelihood steps
int rj_ready(hens_ctx_impl* c, bool between_halves = false, bool propose = false) {
    int r = ready(c, true);
    if (r) return r;
    if (const int rk = need_rj_context(c)) return rk;
    if (c->Tl != c->T) return fail(c, HENS_ERR_UNSUPPORTED, "the leaf-packing path runs on the whole ladder of one GPU");
    if ((c->expect_split != 0 && !between_halves) || c->propose_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    if (c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_accept must follow hens_rj_propose");
    if (c->rj.general && !propose)
        return fail(c, HENS_ERR_STATE, "this context's model has no device likelihood (hens_rj_set_model_general): step it with hens_rj_propose / hens_rj_accept");
    return HENS_OK;
}

int rj_ensure_staging(hens_ctx_impl* c) {
    if (c->rj.u) return HENS_OK;
    const size_t TW = (size_t)c->Tl * c->W;
    int r;
    if ((r = dalloc(c, &c->rj.step, TW * c->D))) return r;
    if ((r = dalloc(c, &c->rj.u, TW))) return r;
    if ((r = dalloc(c, &c->rj.birth, TW * RJ_MAX_ND * RJ_MAX_BRANCH))) return r;      // ([nbranches][Tl][W]: hens_rj_bd_all_step)
    if ((r = dalloc(c, &c->rj.change, TW * RJ_MAX_BRANCH))) return r;
    if ((r = dalloc(c, &c->rj.leaf, TW * RJ_MAX_BRANCH))) return r;
    if ((r = dalloc(c, &c->rj.keep, TW))) return r;
    if ((r = dalloc(c, &c->rj.st_own, TW))) return r;                              // (hens_rj_stretch_split)
    if ((r = dalloc(c, &c->rj.st_cw, TW * RJ_MAX_BRANCH))) return r;
    if ((r = dalloc(c, &c->rj.uzz, TW))) return r;
    return HENS_OK;
}

// The stand-alone cascade of hens_step (MH iterations of a mix, the copying launches).  Round 5: it accumulates its swap counts
// like the fused launch does, into a handful of rows the NEXT launch's folded adaptation sums - a row per workgroup (512 x 31
// counts at config 5) could not be folded and cost a k_adapt launch of 11.5 us per MH iteration.  HENS_PT_NO_ACC=1: A/B knob.
void step_cascade(hens_ctx_impl* c, LaunchTimer* tm) {
    if (!has_pt(c)) return;
    PtArgs p = pt_args(c, nullptr, false);
    const bool use_acc = !env().pt_no_acc && fast_path(c) && c->T <= 128;
    if (use_acc) { p.swap_part = acc_take(c); p.acc_rows = 8 * acc_row_groups(c->T); acc_commit(c); }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    time_launch(c, tm, 1, e0, e1);
    if (tm) hipExtLaunchKernelGGL(k_pt_cascade<true>, dim3(pt_blocks(c)), dim3(pt_threads(c->T)), (uint32_t)pt_lds_bytes(c->T), c->stream, e0, e1, 0, p);
    else hipLaunchKernelGGL(k_pt_cascade<true>, dim3(pt_blocks(c)), dim3(pt_threads(c->T)), pt_lds_bytes(c->T), c->stream, p);
    cascade_ran(c, use_acc ? p.swap_part : nullptr, p.acc_rows, c->cfg.adaptive != 0);
}

// The move of one iteration under Gibbs block tables (hens_set_gibbs; a single, whole-ladder context on Iteration::COPYING): block
// after block of the iteration's move - a plan of the block's draws on the iteration's labels and the two copying half-steps
// (red_blue.py:119-333), or k_mh_draw with the block's words and the MH launch (mh.py:79-193) - every block against the rows the
// block before it left.  The caller runs the ONE cascade behind the last block.  num_proposals / num_proposals_mh advance per block.
int ensure_gibbs_draws(hens_ctx_impl* c) {
    if (c->gdr.cw) return HENS_OK;
    const size_t TW = (size_t)c->Tl * c->W;
    int r;
    if ((r = dalloc(c, &c->gdr.cw, TW)) || (r = dalloc(c, &c->gdr.zz, TW)) || (r = dalloc(c, &c->gdr.fac, TW)) || (r = dalloc(c, &c->gdr.lu, TW))) return r;
    return HENS_OK;
}
int gibbs_iteration(hens_ctx_impl* c, bool mh, int ib, LaunchTimer* tm) {
    state_to_fields(c);
    hens_ctx_impl::Gibbs& G = c->gibbs[mh ? 1 : 0];
    int r = HENS_OK;
    for (int b = 0; b < G.blocks() && !r; ++b) {
        G.cur = b;
        if (mh) { r = mh_iteration(c, tm, false); continue; }
        PlanBlockArgs pb{};
        pb.own = c->db[0].d.own + (size_t)ib * c->Tl * c->W;
        pb.dr = c->gdr;
        pb.iter = c->iter; pb.seed = c->cfg.seed; pb.a = c->cfg.a;
        pb.Tl = c->Tl; pb.W = c->W; pb.nb = gibbs_dim(c, 0); pb.rung_begin = c->cfg.rung_begin; pb.block = (uint32_t)b;
        c->gdr.own = const_cast<int32_t*>(pb.own);
        hipLaunchKernelGGL(k_plan_block, dim3((c->W + 255) / 256, c->Tl), dim3(256), 0, c->stream, pb);
        r = stretch_pair(c, 0, ib, tm, false);
    }
    G.cur = G.sel;
    return r;
}

// one iteration of hens_step on the call's path, from batch slot `ib` of the draw plan; an MH iteration of a mix replaces the
// stretch move and is followed by a cascade of its own
int run_iteration(hens_ctx_impl* c, const StepPath& path, int ib, LaunchTimer* tm) {
    if (path.piped()) pipe_prewait(c);
    const bool mh = iteration_is_mh(c);
    if (path.it == Iteration::PIPE_INPLACE2) return pipe_fused_iteration(c, path, tm, mh);
    if (!mh && path.it == Iteration::ONE_LAUNCH) return iter_iteration(c, path, ib, tm);
    if (!mh && path.it == Iteration::INPLACE2) return fused_iteration(c, path, tm);
    const bool inplace = !path.piped() && fast_path(c);
    int r;
    if (gibbs_on(c)) {
        if ((r = gibbs_iteration(c, mh, ib, tm))) return r;
        step_cascade(c, tm);
        return HENS_OK;
    }
    if (mh) {
        // (the fast kernels and the cascade read the walker records too; other MH launches want the by-field arrays)
        if (path.records()) state_to_records(c, path.col);
        else state_to_fields(c);
        r = mh_iteration(c, tm, inplace);
    } else if (path.it == Iteration::SETS) r = stretch_sets(c, tm);
    else r = stretch_pair(c, 0, ib, tm, inplace);
    if (r) return r;
    if (!path.piped()) { step_cascade(c, tm); return HENS_OK; }
    hipEvent_t e0 = nullptr, e1 = nullptr;
    time_launch(c, tm, 1, e0, e1);
    if (tm) (void)hipEventRecord(e0, c->stream);
    pipe_sweep(c);
    if (tm) (void)hipEventRecord(e1, c->stream);
    return HENS_OK;
}

// per-launch durations of a call into hens_timing and launch_us (begin / end of every stepping launch, us after the first begin);
// span(k, begin_us, end_us) gives launch k's and returns its duration in ms; kind < 0: not a stepping launch
template <class Kinds, class Span>
void fold_timing(hens_ctx_impl* c, const Kinds& kinds, size_t n, Span span) {
    std::vector<double> us;
    for (size_t k = 0; k < n; ++k) {
        if (kinds[k] < 0) continue;              // (round-key window plans)
        double b = 0, e = 0;
        const double ms = span(k, b, e);
        us.push_back(b);
        us.push_back(e);
        if (kinds[k] == 0) { c->timing.stretch_ms += ms; c->timing.n_stretch += 1; }
        else if (kinds[k] == 1) { c->timing.pt_ms += ms; c->timing.n_pt += 1; }
        else { c->timing.fused_ms += ms; c->timing.n_fused += 1; }
    }
    c->launch_us.swap(us);
}

// the cascade + (optionally adapting) ladder update after a leaf-packing move; `key` separates the two cascades of one iteration
void rj_cascade(hens_ctx_impl* c, uint64_t key, bool adapt) {
    if (!has_pt(c)) return;
    flush_adapt(c);
    PtArgs p = pt_args(c, nullptr, false);
    p.iter = key;
    hipLaunchKernelGGL(k_pt_cascade<true>, dim3(pt_blocks(c)), dim3(pt_threads(c->T)), pt_lds_bytes(c->T), c->stream, p);
    cascade_ran(c, nullptr, 0, adapt && c->cfg.adaptive != 0);     // rj.py:381-382: swaps without adaptation after the RJ move
    if (!c->rj.defer_adapt) flush_adapt(c);      // (hens_rj_step: the next k_rj launch adapts, see rj_launch)
}

}  // namespace

// ================================================================================================
// ---- RCCL neighbour exchange inside the library (hens_comm_init / hens_comm_destroy) ------------------------------
// The staged transport's protocol (include/hipensemble.h, "Staged transport") with the messages sent by the library itself:
// ncclSend / ncclRecv between ladder neighbours and one all-reduce of the swap counts per sweep, all enqueued on the context's
// stream between the three stage launches - hens_step(n) on such a context is ONE call for n iterations, no host in the loop.
// librccl is dlopen()ed by its soname: in a process that holds PyTorch-ROCm that is torch's own copy (already loaded), so both
// speak to one RCCL; a process without torch gets the system library.
struct RcclApi {
    bool tried = false, ok = false;
    std::string err;
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*Send)(const void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Recv)(void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
};
static RcclApi& rccl_api() {
    static RcclApi a;
    if (a.tried) return a;
    a.tried = true;
    void* h = nullptr;
    for (const char* name : {"librccl.so.1", "librccl.so"}) {
        h = dlopen(name, RTLD_NOW | RTLD_LOCAL);
        if (h) break;
    }
    if (!h) { a.err = std::string("dlopen(librccl.so.1): ") + (dlerror() ? dlerror() : "not found"); return a; }
#define HENS_RCCL_SYM(field, sym) do { *reinterpret_cast<void**>(&a.field) = dlsym(h, sym); if (!a.field) { a.err = std::string("librccl lacks ") + sym; return a; } } while (0)
    HENS_RCCL_SYM(GetUniqueId, "ncclGetUniqueId"); HENS_RCCL_SYM(CommInitRank, "ncclCommInitRank"); HENS_RCCL_SYM(CommDestroy, "ncclCommDestroy");
    HENS_RCCL_SYM(Send, "ncclSend"); HENS_RCCL_SYM(Recv, "ncclRecv"); HENS_RCCL_SYM(AllReduce, "ncclAllReduce");
    HENS_RCCL_SYM(GroupStart, "ncclGroupStart"); HENS_RCCL_SYM(GroupEnd, "ncclGroupEnd"); HENS_RCCL_SYM(GetErrorString, "ncclGetErrorString");
#undef HENS_RCCL_SYM
    a.ok = true;
    return a;
}
#define RCCLCHK(c, expr)                                                                           \
    do {                                                                                           \
        const ncclResult_t n_ = (expr);                                                            \
        if (n_ != ncclSuccess) return fail(c, HENS_ERR_HIP, "%s failed: %s", #expr, rccl_api().GetErrorString(n_)); \
    } while (0)

static int pipe_regions_impl(hens_ctx_impl* c, hens_pipe_region_table* out);
static int pipe_stage_impl(hens_ctx_impl* c, int32_t stage);

// n iterations of a ladder shard whose neighbours are reached through the context's communicator
static int comm_step(hens_ctx_impl* c, int64_t n_iters) {
    RcclApi& R = rccl_api();
    ncclComm_t comm = static_cast<ncclComm_t>(c->comm);
    const int up = c->pipe.rank + 1, dn = c->pipe.rank - 1;
    const bool top = pipe_has_top(c), bot = pipe_has_bot(c);
    int r = aql_settle(c);
    if (r) return r;
    for (int64_t it = 0; it < n_iters; ++it) {
        hens_pipe_region_table g{};
        if ((r = pipe_regions_impl(c, &g))) return r;
        const size_t lp = (size_t)g.lp_doubles, rows = (size_t)g.row_doubles, nc = (size_t)g.cnt_words;
        if ((r = pipe_stage_impl(c, 0))) return r;                       // the move; publishes the boundary rung
        if (top || bot) {                                                // LDN: cold -> hot (RCCL cannot pull: the rung's rows travel along)
            RCCLCHK(c, R.GroupStart());
            if (top) { RCCLCHK(c, R.Send(g.ldn_out, lp, ncclDouble, up, comm, c->stream)); RCCLCHK(c, R.Send(g.ldn_rows_out, rows, ncclDouble, up, comm, c->stream)); }
            if (bot) { RCCLCHK(c, R.Recv(g.ldn_in, lp, ncclDouble, dn, comm, c->stream)); RCCLCHK(c, R.Recv(g.ldn_rows_in, rows, ncclDouble, dn, comm, c->stream)); }
            RCCLCHK(c, R.GroupEnd());
        }
        if (top) RCCLCHK(c, R.Recv(g.lup_in, lp, ncclDouble, up, comm, c->stream));       // LUP: hot -> cold
        if ((r = pipe_stage_impl(c, 1))) return r;                       // the walk
        if (bot) RCCLCHK(c, R.Send(g.lup_out, lp, ncclDouble, dn, comm, c->stream));
        if (top) RCCLCHK(c, R.Recv(g.rows_in, rows, ncclDouble, up, comm, c->stream));    // ROWS: hot -> cold, before my bottom pair
        if ((r = pipe_stage_impl(c, 2))) return r;                       // bottom pair; fills the rows that go down
        if (bot) RCCLCHK(c, R.Send(g.rows_out, rows, ncclDouble, dn, comm, c->stream));
        if (c->pipe.nranks > 1) RCCLCHK(c, R.AllReduce(g.cnt_out, g.cnt_out, nc, ncclUint32, ncclSum, comm, c->stream));   // CNT: every pair's owner -> all
        HIPCHK(c, hipMemcpyAsync(g.cnt_in, g.cnt_out, nc * 4, hipMemcpyDeviceToDevice, c->stream));
    }
    HIPCHK(c, hipGetLastError());
    return HENS_OK;
}

extern "C" {

const char* hens_version(void) { return "hipensemble 0.2 (gfx950)"; }

int hens_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int hens_device_pci_bus_id(int32_t device_id, char* out, int32_t capacity) {
    if (!out || capacity < 16) return fail(nullptr, HENS_ERR_INVALID, "hens_device_pci_bus_id: buffer of at least 16 bytes");
    const hipError_t e = hipDeviceGetPCIBusId(out, capacity, device_id);
    if (e != hipSuccess) return fail(nullptr, HENS_ERR_HIP, "hipDeviceGetPCIBusId(%d): %s", (int)device_id, hipGetErrorString(e));
    return HENS_OK;
}

const char* hens_last_error(const hens_ctx* ctx) {
    const hens_ctx_impl* c = reinterpret_cast<const hens_ctx_impl*>(ctx);
    return c ? c->err.c_str() : g_last_error.c_str();
}

int hens_create(const hens_config* cfg, hens_ctx** out) {
    if (!cfg || !out) return fail(nullptr, HENS_ERR_INVALID, "null argument");
    *out = nullptr;
    if (cfg->adaptation_delay != 0 && cfg->adaptation_delay != 1) return fail(nullptr, HENS_ERR_INVALID, "adaptation_delay must be 0 or 1");
    if (cfg->ntemps < 1 || cfg->nwalkers < 2 || cfg->ndim < 1)
        return fail(nullptr, HENS_ERR_INVALID, "invalid shape ntemps=%d nwalkers=%d ndim=%d", cfg->ntemps,
                    cfg->nwalkers, cfg->ndim);
    if (cfg->rung_begin < 0 || cfg->rung_end > cfg->ntemps || cfg->rung_begin >= cfg->rung_end)
        return fail(nullptr, HENS_ERR_INVALID, "invalid ladder shard [%d, %d) of %d", cfg->rung_begin,
                    cfg->rung_end, cfg->ntemps);
    if (cfg->likelihood_kind < 0 || cfg->likelihood_kind > HENS_LIKE_TEMPLATE)
        return fail(nullptr, HENS_ERR_INVALID, "unknown likelihood kind %d", cfg->likelihood_kind);
    if (!(cfg->a > 1.0)) return fail(nullptr, HENS_ERR_INVALID, "stretch scale a must be > 1");
    if (cfg->ntemps > 1 && !cfg->tempered)
        return fail(nullptr, HENS_ERR_INVALID, "ntemps > 1 requires tempered = 1");
    if (cfg->ntemps > 4096) return fail(nullptr, HENS_ERR_UNSUPPORTED, "ntemps > 4096 not supported");
    if (cfg->ndim_active < 0 || cfg->ndim_active > cfg->ndim)
        return fail(nullptr, HENS_ERR_INVALID, "ndim_active must be 0 (= ndim) or in [1, ndim]");
    // (leaf-packing records: a record is wider than the walker's coordinates - its red / blue move checks for itself, hens_rj_stretch_split)
    if (!cfg->live_dangerously && cfg->likelihood_kind != HENS_LIKE_TEMPLATE && cfg->nwalkers < 2 * (cfg->ndim_active ? cfg->ndim_active : cfg->ndim))   // red_blue.py:108-114
        return fail(nullptr, HENS_ERR_TOO_FEW_WALKERS,
                    "It is unadvisable to use a red-blue move with fewer walkers than twice the number of "
                    "dimensions. If you would like to do this, please set live_dangerously to True.");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(nullptr, HENS_ERR_HIP, "no HIP device available (libhipensemble needs an MI355X)");
    if (cfg->device_id < 0 || cfg->device_id >= ndev)
        return fail(nullptr, HENS_ERR_INVALID, "device_id %d out of range (%d devices)", cfg->device_id, ndev);

    hens_ctx_impl* c = new hens_ctx_impl();
    c->cfg = *cfg;
    c->T = cfg->ntemps; c->W = cfg->nwalkers; c->D = cfg->ndim;
    c->Tl = cfg->rung_end - cfg->rung_begin;
    c->N0 = (c->W + 1) / 2;
    c->have_like = cfg->likelihood_kind == HENS_LIKE_HOST;
    if (cfg->likelihood_kind == HENS_LIKE_TEMPLATE && cfg->ndim > RJ_MAX_RW) {
        delete c;
        return fail(nullptr, HENS_ERR_UNSUPPORTED, "leaf-packing record wider than %d doubles", RJ_MAX_RW);
    }
    hens_ctx* h = reinterpret_cast<hens_ctx*>(c);
#define TRY(x) do { int r_ = (x); if (r_) { g_last_error = c->err; hens_destroy(h); return r_; } } while (0)
#define TRYHIP(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fail(c, HENS_ERR_HIP, "%s: %s", #x, hipGetErrorString(e_)); g_last_error = c->err; hens_destroy(h); return HENS_ERR_HIP; } } while (0)
    TRYHIP(hipSetDevice(cfg->device_id));
    {   // ONE stream per context (round 4: the side stream of the draw plan is gone)
        int prio_lo = 0, prio_hi = 0;
        TRYHIP(hipDeviceGetStreamPriorityRange(&prio_lo, &prio_hi));
        TRYHIP(hipStreamCreateWithPriority(&c->stream, hipStreamNonBlocking, prio_hi));
    }
    c->own_stream = true;
    {   // the context's AQL queue for the stepping launches (hens_aql.h); HENS_NO_AQL=1: everything on the HIP stream
        if (!env().no_aql) {
            hens_aql::Device& ad = hens_aql::device(cfg->device_id);
            if (ad.ok && c->aql.create(ad)) {
                c->aql_on = true;
                const int fm = env().aql_flush;     // (see hens_aql::Queue::flush_mode)
                if (fm >= 0 && fm <= 3) c->aql.flush_mode = fm;
            } else {
                static bool warned = false;
                if (!warned) fprintf(stderr, "[hipensemble] direct AQL dispatch unavailable (%s): stepping launches use the HIP stream\n",
                                     ad.ok ? c->aql.err.c_str() : ad.err.c_str());
                warned = true;
                if (ad.ok) c->aql.destroy();
            }
        }
    }
    const size_t TW = (size_t)c->Tl * c->W;
    TRY(dalloc(c, &c->pool, 2 * TW * c->D));
    for (int b = 0; b < 2; ++b) {
        TRY(dalloc(c, &c->loc[b], TW));
        TRY(dalloc(c, &c->L[b], TW));
        TRY(dalloc(c, &c->P[b], TW));
        TRY(dalloc(c, &c->betas[b], (size_t)c->T));
    }
    TRY(dalloc(c, &c->accepted, TW));
    TRY(dalloc(c, &c->flags, 1));
    TRY(dalloc(c, &c->swap_part, (size_t)c->T * pt_blocks(c)));
    TRY(dalloc(c, &c->swaps_last, (size_t)c->T));
    TRY(dalloc(c, &c->swaps_total, (size_t)c->T));
    TRY(dalloc(c, &c->lo, (size_t)c->D));
    TRY(dalloc(c, &c->hi, (size_t)c->D));
    TRY(dalloc(c, &c->mu, (size_t)c->D));
    TRY(dalloc(c, &c->prec, (size_t)c->D * c->D));
    TRY(dalloc(c, &c->prec_sym, std::max<size_t>((size_t)(c->D / 2 + 1) * (c->D + 2), (size_t)(c->D == 128 ? MF128_END : MF64_END))));
    TRY(dalloc(c, &c->ad_ring, (size_t)4 * c->T));
    {
        std::vector<double> neg((size_t)4 * c->T, -1.0);
        TRYHIP(hipMemcpyAsync(c->ad_ring, neg.data(), neg.size() * 8, hipMemcpyHostToDevice, c->stream));
        TRYHIP(hipStreamSynchronize(c->stream));
    }
    TRY(dalloc(c, &c->order, TW));
    TRY(dalloc(c, &c->d_rint, (size_t)c->Tl * c->N0));
    TRY(dalloc(c, &c->d_uzz, (size_t)c->Tl * c->N0));
    TRY(dalloc(c, &c->d_uacc, (size_t)c->Tl * c->N0));
    TRY(dalloc(c, &c->d_keep, (size_t)c->Tl * c->N0));
    TRY(dalloc(c, &c->xtmp, TW * c->D));
    // plan batches: two buffers of NB iterations, each kept under ~96 MiB
    c->NP2 = 1; c->idx_bits = 0;
    while (c->NP2 < c->W) { c->NP2 <<= 1; c->idx_bits++; }
    // Block-balanced split labels (see block_rank): ladders of 2..64 rungs whose length divides 128, walker counts
    // that are a multiple of the block.  A property of (T, W) only, so every rank of a sharded ladder agrees.
    // (round 2, end: ladders whose length does not divide 128 too - cb = the largest power of two with cb T <= 128, the
    //  workgroups of k_split1_pt / k_iter then hold cb T <= 128 slots and cb T / 2 <= 64 moving walkers)
    if (cfg->tempered && c->T >= 2 && c->T <= 64) {
        int cb = 1;
        while (cb * 2 * c->T <= 2 * TILE) cb *= 2;
        if (cb >= 2 && c->W % cb == 0) {
            c->label_cb = cb;
            while ((1 << c->label_cb_shift) < cb) c->label_cb_shift++;
        }
    }
    for (int b = 0; b < 2; ++b)
        if (c->label_cb) TRY(dalloc(c, &c->wrec[b], TW));
    if (c->label_cb) TRY(dalloc(c, &c->ikeys, (size_t)KEY_WINDOW * c->T * 8));
    {
        int ncu = 0;
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, cfg->device_id) == hipSuccess && ncu > 0) c->num_cu = ncu;
    }
    TRY(dalloc(c, &c->swap_acc[0], (size_t)3 * SWAP_ACC_ROWS_MAX * c->T));
    c->swap_acc[1] = c->swap_acc[0] + (size_t)SWAP_ACC_ROWS_MAX * c->T;
    c->swap_acc[2] = c->swap_acc[1] + (size_t)SWAP_ACC_ROWS_MAX * c->T;
    TRYHIP(hipMemsetAsync(c->swap_acc[0], 0, (size_t)3 * SWAP_ACC_ROWS_MAX * c->T * 4, c->stream));
    {
        const size_t per_iter = TW * 64;
        size_t nb = (96u << 20) / std::max<size_t>(per_iter, 1);
        nb = std::max<size_t>(2, std::min<size_t>(nb, 32));
        nb &= ~(size_t)1;
        c->NB = (int)nb;
    }
    for (int b = 0; b < 1; ++b) {
        const size_t n = (size_t)c->NB * TW;
        TRY(dalloc(c, &c->db[b].d.own, n));
        TRY(dalloc(c, &c->db[b].d.cw, n));
        TRY(dalloc(c, &c->db[b].d.zz, n));
        TRY(dalloc(c, &c->db[b].d.fac, n));
        TRY(dalloc(c, &c->db[b].d.lu, n));
        const size_t nrec = c->label_cb ? (size_t)c->NB * rec_per_iter(c) : 0;   // (>= n / 2: short tiles keep their 64 places)
        if (c->label_cb) TRY(dalloc(c, &c->db[b].rec, nrec));
        if (c->label_cb && c->Tl == c->T && (c->D == 16 || c->D == 32) && c->W <= 32768 && TW <= ((size_t)1 << 20)) {
            TRY(dalloc(c, &c->db[b].rec1, nrec));        // (one-launch iteration, see step_path)
            TRY(dalloc(c, &c->db[b].rec3, nrec));
        }
        TRY(dalloc(c, &c->db[b].keys, (size_t)c->NB * c->T * 8));
    }
    TRYHIP(hipMemsetAsync(c->accepted, 0, TW * 4, c->stream));
    TRYHIP(hipMemsetAsync(c->flags, 0, 4, c->stream));
    TRYHIP(hipMemsetAsync(c->swap_part, 0, (size_t)c->T * pt_blocks(c) * 4, c->stream));
    TRYHIP(hipMemsetAsync(c->swaps_last, 0, (size_t)c->T * 8, c->stream));
    TRYHIP(hipMemsetAsync(c->swaps_total, 0, (size_t)c->T * 8, c->stream));
    TRYHIP(hipEventCreate(&c->ev0));
    TRYHIP(hipEventCreate(&c->ev1));
    {   // kernels that may need > 64 KiB of dynamic LDS
        const size_t plan_lds = plan_lds_bytes(c);
        if (plan_lds > 160 * 1024) {
            fail(c, HENS_ERR_UNSUPPORTED, "nwalkers %d exceeds the in-LDS split plan (6 bytes of LDS per walker: max %d)", c->W, (160 * 1024 - 16) / 6);
            g_last_error = c->err; hens_destroy(h); return HENS_ERR_UNSUPPORTED;
        }
        TRYHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_plan), hipFuncAttributeMaxDynamicSharedMemorySize, (int)plan_lds));
        const size_t ptl = pt_lds_bytes(c->T);
        if (ptl > 160 * 1024) {
            fail(c, HENS_ERR_UNSUPPORTED, "ntemps %d exceeds the in-LDS cascade column tile", c->T);
            g_last_error = c->err; hens_destroy(h); return HENS_ERR_UNSUPPORTED;
        }
        TRYHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pt_cascade<false>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ptl));
        TRYHIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_pt_cascade<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)ptl));
    }
    TRYHIP(hipStreamSynchronize(c->stream));
#undef TRY
#undef TRYHIP
    *out = h;
    return HENS_OK;
}

static int rjchain_drop(hens_ctx_impl* c);    // (below, with hens_rj_chain_*)
void hens_destroy(hens_ctx* ctx) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c) return;
    (void)hipSetDevice(c->cfg.device_id);
    if (c->comm_on) { RcclApi& R = rccl_api(); if (c->stream) (void)hipStreamSynchronize(c->stream); if (R.ok) (void)R.CommDestroy(static_cast<ncclComm_t>(c->comm)); c->comm_on = false; }
    if (c->aql_on) {
        if (getenv("HENS_AQL_STATS")) fprintf(stderr, "[hipensemble] AQL queue: %llu packets written, %llu doorbells; kernarg ring in %s memory%s, HDP flush register %s\n",
                                              (unsigned long long)c->aql.packets, (unsigned long long)c->aql.doorbells, c->aql.kernarg_dev ? "device" : "host",
                                              c->aql.kernarg_fine ? " (fine-grained pool)" : " (coarse-grained pool)", c->aql.dev->hdp.HDP_MEM_FLUSH_CNTL ? "present" : "absent");
        c->aql.destroy();
        c->aql_on = false;
    }
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (size_t q = 0; q < c->pipe.boxes.size(); ++q)
        if (c->pipe.opened[q] && c->pipe.boxes[q]) (void)hipIpcCloseMemHandle(c->pipe.boxes[q]);
    if (c->pipe.pool_cold_opened) (void)hipIpcCloseMemHandle(const_cast<double*>(c->pipe.pool_cold));
    if (c->pipe.box) (void)hipFree(c->pipe.box);
    for (void* p : c->allocs)
        if (p) (void)hipFree(p);
    c->chain.release();
    for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->stream && c->own_stream) (void)hipStreamDestroy(c->stream);
    delete c;
}

int hens_synchronize(hens_ctx* ctx) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c) return no_context();
    if (c->aql_on) {              // the AQL queue first (a spin on its completion signal); the HIP stream only if it may hold work
        const bool dirty = c->hip_dirty;
        const int r = aql_settle(c);
        if (r) return r;
        c->hip_dirty = dirty;
        if (!dirty) return HENS_OK;
    }
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->hip_dirty = false;
    if (pipe_active(c)) return check_flags(c, false);     // a neighbour that never answered surfaces here
    return HENS_OK;
}

int hens_set_stream(hens_ctx* ctx, void* s) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (c->own_stream) (void)hipStreamDestroy(c->stream);
    c->stream = reinterpret_cast<hipStream_t>(s);
    c->own_stream = false;
    return HENS_OK;
}

// The device images of one move's Gibbs blocks (hens_gibbs_host.h: gibbs_image) from the prior as the host holds it - its terms, or
// the box as uniform terms that add up to logp_in - and the table's masks; a move without a table: one all-true block.  Room for
// GIBBS_MAX_BLOCKS images is allocated once per move (at most 0.85 MB, D = 128): a table that is replaced by a longer one takes no
// new memory.  hens_set_gibbs rebuilds the move it changes (and the other move's single image if that was never built or the prior
// has changed since); the prior's setters rebuild both while a table is on.
static int gibbs_rebuild(hens_ctx_impl* c, int move) {
    hens_ctx_impl::Gibbs& G = c->gibbs[move];
    G.img_ok = false;
    if (!gibbs_on(c) || c->h_lo.empty()) return HENS_OK;
    const int D = c->D, Da = dim_active(c), nb = G.blocks();
    const size_t stride = gibbs_image_doubles(D);
    if (!G.img)
        if (const int r = dalloc(c, &G.img, (size_t)GIBBS_MAX_BLOCKS * stride)) return r;
    std::vector<PriorTerm> terms(c->h_terms);
    if (terms.empty()) { terms.resize((size_t)D); box_as_terms(c->logp_in, D, Da, terms.data()); }
    std::vector<double> host((size_t)nb * stride);
    std::vector<int32_t> all((size_t)D, 0);
    for (int d = 0; d < Da; ++d) all[(size_t)d] = 1;
    for (int b = 0; b < nb; ++b)
        gibbs_image(c->h_lo.data(), c->h_hi.data(), terms.data(), G.nblocks > 0 ? G.mask.data() + (size_t)b * D : all.data(), D, host.data() + (size_t)b * stride);
    HIPCHK(c, hipStreamSynchronize(c->stream));      // (a launch in flight may still read the images about to be replaced)
    HIPCHK(c, hipMemcpy(G.img, host.data(), host.size() * 8, hipMemcpyHostToDevice));      // (synchronous: `host` is a local)
    G.img_ok = true;
    return HENS_OK;
}
// after hens_set_gibbs changed `move`'s table: its images, and the other move's where they are not the current prior's
static int gibbs_rebuild_for(hens_ctx_impl* c, int move) {
    if (const int r = gibbs_rebuild(c, move)) return r;
    return c->gibbs[move ^ 1].img_ok ? HENS_OK : gibbs_rebuild(c, move ^ 1);
}
static int keep_prior_host(hens_ctx_impl* c, const double* lo, const double* hi, const PriorTerm* terms) {
    c->h_lo.assign(lo, lo + c->D);
    c->h_hi.assign(hi, hi + c->D);
    if (terms) c->h_terms.assign(terms, terms + c->D);
    else c->h_terms.clear();
    if (const int r = gibbs_rebuild(c, 0)) return r;
    return gibbs_rebuild(c, 1);
}

int hens_set_prior_box(hens_ctx* ctx, const double* lo, const double* hi, double logp_inside) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !lo || !hi) return fail(c, HENS_ERR_INVALID, "null argument");
    for (int d = 0; d < c->D; ++d)
        if (!(lo[d] < hi[d])) return fail(c, HENS_ERR_INVALID, "prior box needs lo < hi in every dimension (dim %d)", d);
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | (c->prior ? NEED_LADDER : 0u));     // (leaving prior terms: the launch path changes)
    HIPCHK(c, hipMemcpyAsync(c->lo, lo, c->D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->hi, hi, c->D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->logp_in = logp_inside;
    c->prior = nullptr;               // (back to the box after hens_set_prior_terms)
    c->have_prior = true;
    return keep_prior_host(c, lo, hi, nullptr);
}

// prior.py:337-392 with one distribution per parameter (include/hipensemble.h); uniform kinds only: hens_set_prior_box itself.
// Every term is read by hens_prior_host.h's parse_term, here and in hens_rj_set_prior_terms; a refusal is its reason and this place.
static_assert(HENS_PRIOR_UNIFORM == PRIOR_UNIFORM && HENS_PRIOR_LOG_UNIFORM == PRIOR_LOG_UNIFORM && HENS_PRIOR_NORMAL == PRIOR_NORMAL,
              "parse_term takes the caller's kinds as they are");
int hens_set_prior_terms(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0, const double* c1,
                         const double* c2) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !kind || !lo || !hi || !c0 || !c1 || !c2) return fail(c, HENS_ERR_INVALID, "null argument");
    if (is_rj(c))
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_set_prior_terms describes one row of parameters: the leaves of a leaf-packing record take theirs through hens_rj_set_prior_terms");
    const int D = c->D;
    std::vector<PriorTerm> terms((size_t)D);
    for (int d = 0; d < D; ++d) {                  // (a (-inf, +inf) uniform term: the pad of hens_config::ndim_active)
        const ParsedTerm p = parse_term(kind[d], lo[d], hi[d], c0[d], c1[d], c2[d], /*admit_pad=*/true);
        if (p.why[0]) return fail(c, HENS_ERR_INVALID, "%s (dim %d)", p.why, d);
        terms[(size_t)d] = p.term;
    }
    const PriorBox box = fold_box(terms.data(), D);
    if (box.box) return hens_set_prior_box(ctx, lo, hi, box.logp);
    if (c->pipe.on) return fail(c, HENS_ERR_STATE, "prior terms are not built for a rank of the ladder pipeline");
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    if (!c->prior_buf) {
        PriorTerm* buf = nullptr;
        const int r = dalloc(c, &buf, (size_t)D);
        if (r) return r;
        c->prior_buf = buf;
    }
    if (const int r = c->prior_block.upload(c, lo, hi, terms.data())) return r;
    HIPCHK(c, hipMemcpyAsync(c->lo, lo, D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->hi, hi, D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->prior_buf, terms.data(), (size_t)D * sizeof(PriorTerm), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->logp_in = 0.0;
    c->prior = c->prior_buf;
    c->have_prior = true;
    return keep_prior_host(c, lo, hi, terms.data());
}

// ---- Gibbs parameter blocks (move.py:113-221; red_blue.py:119-333, mh.py:79-193 for one branch, nleaves_max == 1) ---------------------
// The state a block table needs: a single whole-ladder context with a device likelihood at a compile-time row width, a two-set
// stretch move, no periodic parameters, nothing half done.
static int gibbs_supported(hens_ctx_impl* c, int32_t move) {
    if (move != HENS_GIBBS_STRETCH && move != HENS_GIBBS_MH) return fail(c, HENS_ERR_INVALID, "move must be HENS_GIBBS_STRETCH (0) or HENS_GIBBS_MH (1)");
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    if (is_rj(c)) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for leaf-packing records");
    if (c->cfg.likelihood_kind == HENS_LIKE_HOST) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks need a device likelihood");
    if (c->pipe.on || c->Tl != c->T) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for a rank of the ladder pipeline or a ladder shard");
    if (c->period) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for periodic parameters (hens_set_periodic)");
    if (c->nsplits != 2) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks step a two-set stretch move (hens_set_nsplits(2))");
    const LikeKernels* lk = like_kernels(c->cfg.likelihood_kind);
    if (!lk || !lk->stretch_gibbs(MODE_STRETCH, c->D))
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are built for row widths 8, 16, 32, 64 and 128 (this context's rows are %d wide)", c->D);
    return HENS_OK;
}

int hens_set_gibbs(hens_ctx* ctx, int32_t move, int32_t nblocks, const uint8_t* mask) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (nblocks == 0 && (move == HENS_GIBBS_STRETCH || move == HENS_GIBBS_MH)) {     // clears the table, whatever the context
        if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
        if (c->gibbs[move].nblocks == 0) return HENS_OK;
        SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
        hens_ctx_impl::Gibbs& G = c->gibbs[move];
        G.nblocks = 0; G.n.clear(); G.mask.clear(); G.sel = G.cur = 0;
        c->win_count = 0;
        return gibbs_rebuild_for(c, move);
    }
    if (const int r = gibbs_supported(c, move)) return r;
    if (move == HENS_GIBBS_MH && c->mh_kind == MH_DIST)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for the distribution proposal in the MH slot (hens_set_dist_proposal)");
    if (move == HENS_GIBBS_MH && c->mh_kind == MH_MT_DIST)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for the multiple-try proposal in the MH slot (hens_set_mt_dist_proposal)");
    ParsedGibbs p = parse_gibbs(nblocks, mask, c->D, dim_active(c));
    if (p.why[0]) return fail(c, HENS_ERR_INVALID, "hens_set_gibbs: %s", p.why);
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);      // (the launch path changes)
    if (const int r = ensure_gibbs_draws(c)) return r;
    hens_ctx_impl::Gibbs& G = c->gibbs[move];
    G.nblocks = nblocks;
    G.n = std::move(p.n);
    G.mask = std::move(p.mask);
    G.sel = G.cur = 0;
    c->win_count = 0;
    return gibbs_rebuild_for(c, move);
}

// teacher-forced: the block the next hens_stretch_split pair (move 0) or hens_mh_step (move 1) belongs to; between complete moves
int hens_gibbs_select(hens_ctx* ctx, int32_t move, int32_t block) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (move != HENS_GIBBS_STRETCH && move != HENS_GIBBS_MH) return fail(c, HENS_ERR_INVALID, "move must be HENS_GIBBS_STRETCH (0) or HENS_GIBBS_MH (1)");
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "hens_gibbs_select between the half-steps of a move");
    hens_ctx_impl::Gibbs& G = c->gibbs[move];
    if (G.nblocks == 0) return fail(c, HENS_ERR_STATE, "no Gibbs table on this move (hens_set_gibbs)");
    if (block < 0 || block >= G.nblocks) return fail(c, HENS_ERR_INVALID, "block must be in [0, %d)", G.nblocks);
    G.sel = G.cur = block;
    return HENS_OK;
}

int hens_set_periodic(hens_ctx* ctx, const double* period) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (is_rj(c))
        return fail(c, HENS_ERR_UNSUPPORTED, "periodic parameters are not defined on leaf-packing records");
    bool any = false;
    if (period)
        for (int d = 0; d < c->D; ++d) {
            if (!(period[d] >= 0.0) || !(period[d] < INFINITY)) return fail(c, HENS_ERR_INVALID, "period of dimension %d must be finite and >= 0", d);
            any = any || period[d] > 0.0;
        }
    if (c->pipe.on) {                 // a rank of the ladder pipeline keeps what it had at hens_pipe_init (the same on every rank)
        if (!any && !c->period) return HENS_OK;
        return fail(c, HENS_ERR_STATE, "set the periodic parameters before hens_pipe_init");
    }
    if (any && gibbs_on(c)) return fail(c, HENS_ERR_UNSUPPORTED, "periodic parameters are not built under Gibbs blocks (hens_set_gibbs(ctx, move, 0, NULL) clears a table)");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (!any) {                       // back to the compile-time-width kernels
        c->period = nullptr;
        return HENS_OK;
    }
    if (!c->period_buf) {
        int r = dalloc(c, &c->period_buf, (size_t)c->D);
        if (r) return r;
    }
    HIPCHK(c, hipMemcpyAsync(c->period_buf, period, c->D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->period = c->period_buf;
    return HENS_OK;
}

int hens_set_gaussian(hens_ctx* ctx, const double* mu, const double* prec) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !mu || !prec) return fail(c, HENS_ERR_INVALID, "null argument");
    if (c->cfg.likelihood_kind != HENS_LIKE_GAUSS_DENSE && c->cfg.likelihood_kind != HENS_LIKE_GAUSS_DIAG)
        return fail(c, HENS_ERR_STATE, "context was not created with a Gaussian likelihood kind");
    const size_t n = c->cfg.likelihood_kind == HENS_LIKE_GAUSS_DENSE ? (size_t)c->D * c->D : (size_t)c->D;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    HIPCHK(c, hipMemcpyAsync(c->mu, mu, c->D * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->prec, prec, n * 8, hipMemcpyHostToDevice, c->stream));
    std::vector<double> sym;
    if (c->cfg.likelihood_kind == HENS_LIKE_GAUSS_DENSE && c->D % 2 == 0) {
        // packed symmetric rows for sym_quad: pair p = rows (p, D-1-p), each from its diagonal rightwards,
        // off-diagonal entries A_ik + A_ki (so a non-symmetric input gives the same quadratic form)
        const int D = c->D;
        auto S = [&](int i, int k) { return (k == i) ? prec[(size_t)i * D + i] : prec[(size_t)i * D + k] + prec[(size_t)k * D + i]; };
        // one H x H diagonal block starting at row/column `base`, in sym_quad's pair layout
        auto pack_block = [&](int base, int H, double* out) {
            const int stride = H + 2;
            for (int p = 0; p < H / 2; ++p) {
                double* row = out + (size_t)p * stride;
                int o = 0;
                for (int i : {p, H - 1 - p})
                    for (int k = i; k < H; ++k) row[o++] = S(base + i, base + k);
            }
        };
        if (D == 64 || D == 128) {
            // blocked form (see like_partial): four H = D / 4 blocks: [4 diagonal blocks][6 cross blocks (0,1) (0,2) (0,3)
            // (1,2) (1,3) (2,3)]
            const int H = D / 4, BLK = (H / 2) * (H + 2);
            sym.assign((size_t)4 * BLK + (size_t)6 * H * H + (size_t)(D == 64 ? MF64_STEPS : MF128_STEPS) * 64, 0.0);
            if (D == 128) {             // the same for like_tile_mf128: eight blocks of 16, 144 steps
                static_assert(MF128_OFF == 4 * 544 + 6 * 1024, "prec_sym layout at D = 128");
                for (int cidx = 0; cidx < MF128_STEPS; ++cidx) {
                    const int I = mf128_I(cidx), J = mf128_J(cidx), st = mf128_S(cidx);
                    for (int l = 0; l < 64; ++l) {
                        const int r = 16 * I + l % 16, k = 16 * J + 4 * st + l / 16;
                        sym[(size_t)MF128_OFF + (size_t)cidx * 64 + l] = I == J ? prec[(size_t)r * D + k] : prec[(size_t)r * D + k] + prec[(size_t)k * D + r];
                    }
                }
            }
            if (D == 64) {
                // the matrix-pipe operands (like_tile_mf64): step c = (I, J >= I, s) in order, mf[c][lane] = M_IJ[lane % 16][4 s +
                // lane / 16], M_II = A_II, M_IJ = A_IJ + A_JI^T
                static_assert(MF64_OFF == 4 * 144 + 6 * 256, "prec_sym layout at D = 64");
                for (int cidx = 0; cidx < MF64_STEPS; ++cidx) {
                    const int I = mf64_I(cidx), J = mf64_J(cidx), st = mf64_S(cidx);
                    for (int l = 0; l < 64; ++l) {
                        const int r = 16 * I + l % 16, k = 16 * J + 4 * st + l / 16;
                        sym[(size_t)MF64_OFF + (size_t)cidx * 64 + l] = I == J ? prec[(size_t)r * D + k] : prec[(size_t)r * D + k] + prec[(size_t)k * D + r];
                    }
                }
            }
            for (int b = 0; b < 4; ++b) pack_block(b * H, H, sym.data() + (size_t)b * BLK);
            int x = 0;
            for (int bi = 0; bi < 4; ++bi)
                for (int bk = bi + 1; bk < 4; ++bk, ++x)
                    for (int i = 0; i < H; ++i)
                        for (int k = 0; k < H; ++k)
                            sym[(size_t)4 * BLK + (size_t)x * H * H + (size_t)i * H + k] = S(bi * H + i, bk * H + k);
        } else if (D == 32 && MF32_ON) {
            // the pair layout (generic-width paths) and, behind it, the matrix-pipe operands of like_tile_mf32: step c = (I, J >= I, s),
            // mf[c][lane] = M_IJ[lane % 16][4 s + lane / 16]
            static_assert(MF32_OFF >= 16 * 34 && MF32_END <= MF64_END, "prec_sym layout at D = 32");
            sym.assign((size_t)MF32_END, 0.0);
            pack_block(0, D, sym.data());
            for (int cidx = 0; cidx < MF32_STEPS; ++cidx) {
                const int I = mf32_I(cidx), J = mf32_J(cidx), st = mf32_S(cidx);
                for (int l = 0; l < 64; ++l) {
                    const int r = 16 * I + l % 16, k = 16 * J + 4 * st + l / 16;
                    sym[(size_t)MF32_OFF + (size_t)cidx * 64 + l] = I == J ? prec[(size_t)r * D + k] : prec[(size_t)r * D + k] + prec[(size_t)k * D + r];
                }
            }
        } else {
            sym.assign((size_t)(D / 2) * (D + 2), 0.0);
            pack_block(0, D, sym.data());
        }
        HIPCHK(c, hipMemcpyAsync(c->prec_sym, sym.data(), sym.size() * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_like = true;
    return HENS_OK;
}

int hens_set_rosenbrock(hens_ctx* ctx, double a, double b) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (c->cfg.likelihood_kind != HENS_LIKE_ROSENBROCK)
        return fail(c, HENS_ERR_STATE, "context was not created with HENS_LIKE_ROSENBROCK");
    c->rosen_a = a; c->rosen_b = b;
    c->have_like = true;
    return HENS_OK;
}

int hens_upload_state(hens_ctx* ctx, const double* x, const double* logl, const double* logp, const double* betas) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !x) return fail(c, HENS_ERR_INVALID, "null argument");
    if (c->cfg.tempered && !betas) return fail(c, HENS_ERR_INVALID, "betas required for a tempered context");
    if ((logl == nullptr) != (logp == nullptr)) return fail(c, HENS_ERR_INVALID, "give both logl and logp or neither");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    const size_t TW = (size_t)c->Tl * c->W;
    c->cur = 0;
    c->rj.tm_valid = false;
    if (c->rj.gr_nf > 0)                      // (the group move's call number restarts; no leaf has a window)
        if (const int rg = rj_group_reset(c)) return rg;
    c->packed = false;
    c->colmode = false;
    c->rows_mixed = false;    // (a failed hens_step call may have left these behind: step_failed)
    c->parity = 1;            // rows live in home 0, the next iteration writes home 1
    c->expect_split = 0;
    c->pt_pending = false;
    c->propose_pending = false;
    HIPCHK(c, hipMemcpyAsync(c->pool, x, TW * c->D * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_iota, dim3(grid_for(TW)), dim3(256), 0, c->stream, c->loc[0], (int64_t)TW);
    if (logl) {
        HIPCHK(c, hipMemcpyAsync(c->L[0], logl, TW * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->P[0], logp, TW * 8, hipMemcpyHostToDevice, c->stream));
    }
    if (betas) HIPCHK(c, hipMemcpyAsync(c->betas[c->bcur], betas, (size_t)c->T * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_state = true;
    c->have_logs = logl != nullptr;
    return HENS_OK;
}

int hens_download_state(hens_ctx* ctx, double* x, double* logl, double* logp, double* betas) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!c->have_state) return fail(c, HENS_ERR_STATE, "no state uploaded");
    if (c->pt_pending) return fail(c, HENS_ERR_STATE, "sharded PT exchange in flight (call hens_pt_finish_sharded)");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    const size_t TW = (size_t)c->Tl * c->W;
    // Leaf-packing contexts with resident templates (round 6): what the caller is about to hold is what a resumed chain
    // would start from - exact templates and log-likelihoods, a function of the coordinates.  If hens_rj_step has updated the
    // templates by +- one leaf since their last full evaluation, that evaluation runs HERE, in front of the copy: the State the
    // caller stores carries the very log-likelihoods the device goes on with, and the next hens_rj_step call finds its templates
    // valid (round 5 invalidated them behind the copy: the stored log_like was the +- value the device then replaced, and every
    // stored step paid the evaluation at the head of the next call instead).
    if (is_rj(c) && (x || logl) && c->rj.tm && c->rj.tm_valid && c->rj.tm_drift) {
        int r = rj_evaluate(c, true);
        if (r) return r;
        if ((r = check_flags(c, true))) return r;
    }
    if (x) {
        hipLaunchKernelGGL(k_gather_rows, dim3(grid_for((int64_t)TW * c->D)), dim3(256), 0, c->stream, c->pool,
                           c->loc[c->cur], c->xtmp, (int64_t)TW, c->D, guest_delta(c));
        HIPCHK(c, hipMemcpyAsync(x, c->xtmp, TW * c->D * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (logl) HIPCHK(c, hipMemcpyAsync(logl, c->L[c->cur], TW * 8, hipMemcpyDeviceToHost, c->stream));
    if (logp) HIPCHK(c, hipMemcpyAsync(logp, c->P[c->cur], TW * 8, hipMemcpyDeviceToHost, c->stream));
    if (betas) HIPCHK(c, hipMemcpyAsync(betas, c->betas[c->bcur], (size_t)c->T * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

int hens_eval_state(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, false);
    if (r) return r;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (is_rj(c)) {
        r = rj_evaluate(c);
        if (r) return r;
        r = check_flags(c, true);
        if (r) return r;
        c->have_logs = true;
        return HENS_OK;
    }
    StretchArgs a = base_args(c);
    a.split = 0;
    a.home_off = 0;
    r = launch_stretch<MODE_EVAL>(c, a, (c->W + TILE - 1) / TILE);
    if (r) return r;
    r = check_flags(c, true);
    if (r) return r;
    c->have_logs = true;
    return HENS_OK;
}

// The iteration counter is an int64 at the C ABI (hens_set_iteration / hens_get_iteration), and the leaf-packing cascades key their
// draws on 2 iter and 2 iter + 1: a call that would carry it past INT64_MAX is refused before it runs (beyond it hens_get_iteration
// would turn negative and 2 iter would wrap to iteration 0's keys).
static int counter_room(hens_ctx_impl* c, int64_t n) {
    if (n > 0 && (uint64_t)n > (uint64_t)INT64_MAX - c->iter)
        return fail(c, HENS_ERR_INVALID, "iteration counter %llu + %lld iterations would pass INT64_MAX", (unsigned long long)c->iter, (long long)n);
    return HENS_OK;
}

// shared front half of the parity-mode half-steps: labels -> ascending split lists, draws -> device
static int prepare_split(hens_ctx_impl* c, int32_t split, const uint8_t* labels, const int64_t* rint,
                         const double* u_zz, const double* u_acc, int* Ns_out) {
    if (!labels || !rint || !u_zz) return fail(c, HENS_ERR_INVALID, "null argument");
    const int NSP = c->nsplits;
    if (split < 0 || split >= NSP) return fail(c, HENS_ERR_INVALID, "split must be in [0, %d) (hens_set_nsplits)", NSP);
    if (split != c->expect_split)
        return fail(c, HENS_ERR_STATE, "split calls must run 0 .. %d in order (expected %d)", NSP - 1, c->expect_split);
    if (c->pt_pending) return fail(c, HENS_ERR_STATE, "sharded PT exchange in flight");
    if (c->propose_pending) return fail(c, HENS_ERR_STATE, "hens_propose_split without its hens_accept_split");
    int r;
    if ((r = counter_room(c, 1))) return r;          // (the iteration's last half-step, or its cascade, advances the counter)
    SETTLE(c, NEED_DEVICE | NEED_LADDER);
    const int Tl = c->Tl, W = c->W;
    if (split == 0) {
        // ascending index lists per label (red_blue.py:150-154): order = [label 0 ... | label 1 ... | ...]
        std::vector<int32_t> order((size_t)Tl * W);
        // arange(W) % nsplits shuffled: set k always has ceil((W - k) / nsplits) walkers (red_blue.py:120-124)
        c->seg_off.assign((size_t)NSP + 1, 0);
        for (int k = 0; k < NSP; ++k) c->seg_off[k + 1] = c->seg_off[k] + (W - k + NSP - 1) / NSP;
        std::vector<int> fill((size_t)NSP);
        for (int t = 0; t < Tl; ++t) {
            for (int k = 0; k < NSP; ++k) fill[k] = c->seg_off[k];
            for (int w = 0; w < W; ++w) {
                const uint8_t l = labels[(size_t)t * W + w];
                if (l >= NSP) return fail(c, HENS_ERR_INVALID, "labels must be in [0, %d)", NSP);
                if (fill[l] >= c->seg_off[l + 1])
                    return fail(c, HENS_ERR_INVALID, "labels must hold ceil((W - k) / nsplits) walkers of set k per rung (set %d too large)", (int)l);
                order[(size_t)t * W + fill[l]++] = w;
            }
        }
        c->N0 = (W + 1) / 2;
        c->labels_host.assign(labels, labels + (size_t)Tl * W);
        HIPCHK(c, hipMemcpyAsync(c->order, order.data(), order.size() * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else {
        if (c->labels_host.size() != (size_t)Tl * W || memcmp(c->labels_host.data(), labels, (size_t)Tl * W) != 0)
            return fail(c, HENS_ERR_INVALID, "labels differ between split 0 and split 1 of the same iteration");
    }
    if ((int)c->seg_off.size() != NSP + 1) return fail(c, HENS_ERR_STATE, "split %d without its split 0", split);
    const int Ns = c->seg_off[split + 1] - c->seg_off[split];
    const int Nc = W - Ns;
    for (size_t i = 0; i < (size_t)Tl * Ns; ++i)
        if (rint[i] < 0 || rint[i] >= Nc) return fail(c, HENS_ERR_INVALID, "rint out of range [0, %d)", Nc);
    const size_t n = (size_t)Tl * Ns;
    HIPCHK(c, hipMemcpyAsync(c->d_rint, rint, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_uzz, u_zz, n * 8, hipMemcpyHostToDevice, c->stream));
    if (u_acc) HIPCHK(c, hipMemcpyAsync(c->d_uacc, u_acc, n * 8, hipMemcpyHostToDevice, c->stream));
    c->win_count = 0;
    hipLaunchKernelGGL(k_prep_draws, dim3(grid_for((int64_t)n)), dim3(256), 0, c->stream, c->order, c->d_rint, c->d_uzz,
                       u_acc ? c->d_uacc : c->d_uzz, c->db[0].d, Tl, W, c->seg_off[split], Ns, c->cfg.a, gibbs_dim(c, 0));      // (the selected block's count: hens_gibbs_select)
    *Ns_out = Ns;
    return HENS_OK;
}

static void finish_split(hens_ctx_impl* c, int32_t split) {
    if (split == c->nsplits - 1) {
        c->parity ^= 1;
        c->num_proposals += 1;
        if (!has_pt(c)) c->iter += 1;
    }
    c->expect_split = (split + 1) % c->nsplits;
}
// how a launch of the parity API sees set `split` of nsplits (StretchArgs::ns_x): 0 first, 1 last, 2 between
static int kernel_split(const hens_ctx_impl* c, int32_t split) { return split == 0 ? 0 : (split == c->nsplits - 1 ? 1 : 2); }

int hens_stretch_split(hens_ctx* ctx, int32_t split, const uint8_t* labels, const int64_t* rint, const double* u_zz,
                       const double* u_acc, uint8_t* keep_out) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, true);
    if (r) return r;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (c->cfg.likelihood_kind == HENS_LIKE_HOST)
        return fail(c, HENS_ERR_STATE, "host-likelihood context: use hens_propose_split / hens_accept_split");
    if (!u_acc) return fail(c, HENS_ERR_INVALID, "null argument");
    int Ns = 0;
    if ((r = prepare_split(c, split, labels, rint, u_zz, u_acc, &Ns))) return r;
    const size_t n = (size_t)c->Tl * Ns;
    StretchArgs a = base_args(c);
    a.split = kernel_split(c, split);
    a.ns_x = Ns; a.soff_x = c->seg_off[split];
    a.home_off = c->parity * c->Tl * c->W;
    a.keep_out = c->d_keep;
    r = launch_stretch<MODE_STRETCH>(c, a, (Ns + TILE - 1) / TILE);
    if (r) return r;
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->d_keep, n, hipMemcpyDeviceToHost, c->stream));
    r = check_flags(c, false);
    if (r) return r;
    finish_split(c, split);
    return HENS_OK;
}

static HostLikeArgs hostlike_args(hens_ctx_impl* c, int32_t split) {
    HostLikeArgs h{};
    h.pool = c->pool; h.loc = c->loc[c->cur]; h.L = c->L[c->cur]; h.P = c->P[c->cur];
    h.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    h.dr = c->db[0].d;
    h.lo = c->lo; h.hi = c->hi; h.period = c->period;
    h.qbuf = c->xtmp;                                   // [Tl*W][D] scratch: Ns <= W rows per rung
    h.inbox = c->d_keep;                                // [Tl][N0] scratch (keep flags go to hl_keep)
    h.rs_old = c->hl_rs; h.keep = c->hl_keep;
    h.logl = c->d_uzz;                                  // staging reused after the proposal consumed u_zz
    h.u_acc = c->d_uacc;
    h.accepted = c->accepted; h.flags = c->flags;
    h.logp_in = c->logp_in;
    h.prior = c->prior;
    h.Tl = c->Tl; h.W = c->W; h.D = c->D; h.split = kernel_split(c, split); h.N0 = c->N0;
    if ((int)c->seg_off.size() == c->nsplits + 1) { h.ns_x = c->seg_off[split + 1] - c->seg_off[split]; h.soff_x = c->seg_off[split]; }
    h.rung_begin = c->cfg.rung_begin; h.home_off = c->parity * c->Tl * c->W; h.tempered = c->cfg.tempered;
    return h;
}

// Move.a of the reference's StretchMove is a plain attribute that a tuning hook may change between proposals
// (utils/updates.py:130-175 mutates move.a; stretch.py:37,129-132 reads it per proposal): the scale of every LATER proposal.
int hens_set_stretch_scale(hens_ctx* ctx, double a) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!(a > 1.0) || !(a < INFINITY)) return fail(c, HENS_ERR_INVALID, "stretch scale a must be finite and > 1");
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    c->cfg.a = a;                              // (every launch reads it from the context when it is built)
    c->win_count = 0;                          // (planned draws of the sharded / staged paths were made with the old scale)
    return HENS_OK;
}

int hens_set_nsplits(hens_ctx* ctx, int32_t nsplits) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (nsplits < 2 || nsplits > 8) return fail(c, HENS_ERR_INVALID, "nsplits must be in [2, 8]");
    if (nsplits > c->W) return fail(c, HENS_ERR_INVALID, "more sets than walkers");
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "a red-blue move is under way");
    if (nsplits != 2 && gibbs_on(c)) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks step a two-set stretch move (hens_set_gibbs(ctx, move, 0, NULL) clears a table)");
    c->nsplits = nsplits;
    c->seg_off.clear();
    return HENS_OK;
}

int hens_propose_split(hens_ctx* ctx, int32_t split, const uint8_t* labels, const int64_t* rint, const double* u_zz,
                       double* q_out, uint8_t* inbox_out) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, true);
    if (r) return r;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (c->cfg.likelihood_kind != HENS_LIKE_HOST)
        return fail(c, HENS_ERR_STATE, "hens_propose_split needs a context created with HENS_LIKE_HOST");
    if (!q_out || !inbox_out) return fail(c, HENS_ERR_INVALID, "null argument");
    int Ns = 0;
    if ((r = prepare_split(c, split, labels, rint, u_zz, nullptr, &Ns))) return r;
    if (!c->hl_rs) {
        if ((r = dalloc(c, &c->hl_rs, (size_t)c->Tl * c->N0))) return r;
        if ((r = dalloc(c, &c->hl_keep, (size_t)c->Tl * c->N0))) return r;
    }
    const size_t n = (size_t)c->Tl * Ns;
    const HostLikeArgs h = hostlike_args(c, split);
    HIPCHK(c, hipMemsetAsync(h.inbox, 1, n, c->stream));
    hipLaunchKernelGGL(k_propose, dim3(grid_for((int64_t)n * c->D)), dim3(256), 0, c->stream, h);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(q_out, h.qbuf, n * c->D * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(inbox_out, h.inbox, n, hipMemcpyDeviceToHost, c->stream));
    r = check_flags(c, false);
    if (r) return r;
    c->propose_pending = true;
    return HENS_OK;
}

int hens_accept_split(hens_ctx* ctx, int32_t split, const double* logl, const double* u_acc, uint8_t* keep_out) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, true);
    if (r) return r;
    if (!c->propose_pending || split != c->expect_split)
        return fail(c, HENS_ERR_STATE, "hens_accept_split must follow hens_propose_split of the same split");
    if (!logl || !u_acc) return fail(c, HENS_ERR_INVALID, "null argument");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const int Ns = c->seg_off[split + 1] - c->seg_off[split];
    const size_t n = (size_t)c->Tl * Ns;
    const HostLikeArgs h = hostlike_args(c, split);
    HIPCHK(c, hipMemcpyAsync(c->d_uzz, logl, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_uacc, u_acc, n * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_accept_decide, dim3(grid_for((int64_t)n)), dim3(256), 0, c->stream, h);
    hipLaunchKernelGGL(k_accept_rows, dim3(grid_for((int64_t)n * c->D)), dim3(256), 0, c->stream, h);
    HIPCHK(c, hipGetLastError());
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->hl_keep, n, hipMemcpyDeviceToHost, c->stream));
    r = check_flags(c, false);
    c->propose_pending = false;
    if (r) return r;
    finish_split(c, split);
    return HENS_OK;
}

int hens_pt_sweep(hens_ctx* ctx, const int64_t* iperm, const int64_t* i1perm, const double* u_swap, int32_t adapt,
                  uint8_t* sel_out, double* swaps_out) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, true);
    if (r) return r;
    if (!c->cfg.tempered) return fail(c, HENS_ERR_STATE, "context is not tempered");
    if (c->Tl != c->T) return fail(c, HENS_ERR_STATE, "hens_pt_sweep needs the whole ladder resident; use hens_pt_plan_sharded");
    if (c->expect_split != 0) return fail(c, HENS_ERR_STATE, "PT sweep between split 0 and split 1");
    if ((r = counter_room(c, 1))) return r;
    if (!iperm || !i1perm || !u_swap) return fail(c, HENS_ERR_INVALID, "null argument");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const int T = c->T, W = c->W;
    if (T < 2) return HENS_OK;
    SETTLE(c, NEED_LADDER);
    r = ensure_pt_buffers(c);
    if (r) return r;
    const size_t PW = (size_t)(T - 1) * W;
    {   // validate permutations on the host (cheap, parity mode only)
        std::vector<uint8_t> seen(W);
        for (int j = 0; j < T - 1; ++j)
            for (const int64_t* p : {iperm + (size_t)j * W, i1perm + (size_t)j * W}) {
                std::fill(seen.begin(), seen.end(), 0);
                for (int k = 0; k < W; ++k) {
                    if (p[k] < 0 || p[k] >= W || seen[p[k]]) return fail(c, HENS_ERR_INVALID, "iperm/i1perm rows must be permutations of range(W)");
                    seen[p[k]] = 1;
                }
            }
    }
    HIPCHK(c, hipMemcpyAsync(c->d_iperm, iperm, PW * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_i1perm, i1perm, PW * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->d_uswap, u_swap, PW * 8, hipMemcpyHostToDevice, c->stream));
    int32_t* colslot = c->colslot;
    hipLaunchKernelGGL(k_pt_invert, dim3(grid_for(PW)), dim3(256), 0, c->stream, c->d_iperm, c->d_inv, T - 1, W);
    hipLaunchKernelGGL(k_pt_chain, dim3((W + 255) / 256), dim3(256), 0, c->stream, c->d_iperm, c->d_i1perm, c->d_inv,
                       c->d_uswap, colslot, c->colk, c->colu, T, W);
    PtArgs p = pt_args(c, colslot, false);
    p.colu = c->colu;
    p.selcol = c->selcol;
    hipLaunchKernelGGL(k_pt_cascade<false>, dim3(pt_blocks(c)), dim3(pt_threads(c->T)), pt_lds_bytes(T), c->stream, p);
    c->adapt_pending = true;
    c->adapt_pending_adaptive = adapt && c->cfg.adaptive;
    SETTLE(c, NEED_LADDER);                   // (this sweep's own counts)
    hipLaunchKernelGGL(k_pt_sel_to_korder, dim3(grid_for(PW)), dim3(256), 0, c->stream, c->selcol, c->colk, c->selk,
                       T - 1, W);
    HIPCHK(c, hipGetLastError());
    c->cur ^= 1;
    c->iter += 1;
    if (sel_out) HIPCHK(c, hipMemcpyAsync(sel_out, c->selk, PW, hipMemcpyDeviceToHost, c->stream));
    if (swaps_out) HIPCHK(c, hipMemcpyAsync(swaps_out, c->swaps_last, (size_t)(T - 1) * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

// a launch inside hens_step's loop failed: the walker records / versioned rows / count-buffer rotation may be half-way between
// two iterations - nothing a later call could read consistently.  The state is declared gone (the caller uploads again)
// instead of leaving stale by-field arrays behind a `packed` flag.
static int step_failed(hens_ctx_impl* c, int r) {
    c->aql_now = c->aql_last = false;
    (void)aql_settle(c);
    (void)hipStreamSynchronize(c->stream);
    c->packed = false;
    c->colmode = false;
    c->rows_mixed = false;
    c->adapt_pending = false;
    c->adapt_src = nullptr;
    c->acc_state[0] = c->acc_state[1] = c->acc_state[2] = 0;
    if (c->swap_acc[0]) (void)hipMemsetAsync(c->swap_acc[0], 0, (size_t)3 * SWAP_ACC_ROWS_MAX * c->T * 4, c->stream);
    c->have_state = false;
    c->have_logs = false;
    return r;
}

int hens_step(hens_ctx* ctx, int64_t n_iters) {
    hens_ctx_impl* c = CTX(ctx);
    int r = ready(c, true);
    if (r) return r;
    if (n_iters < 0) return fail(c, HENS_ERR_INVALID, "n_iters < 0");
    if ((r = counter_room(c, n_iters))) return r;
    const bool piped = pipe_active(c);
    if (c->Tl != c->T && !piped)
        return fail(c, HENS_ERR_STATE, "hens_step on a ladder shard needs the pipeline connected (hens_pipe_init / hens_pipe_connect)");
    if (piped && !has_pt(c)) return fail(c, HENS_ERR_STATE, "the ladder pipeline needs a tempered ladder");
    if (piped && c->pipe.staged) {
        if (c->comm_on) return comm_step(c, n_iters);      // (RCCL neighbour exchange inside the library: hens_comm_init)
        return fail(c, HENS_ERR_STATE, "staged pipeline: step with hens_pipe_stage (the messages travel between the stages), or give the context a communicator (hens_comm_init)");
    }
    if (!piped && c->cfg.adaptation_delay != 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "adaptation_delay is an option of the ladder pipeline (hens_pipe_*)");
    if (c->expect_split != 0) return fail(c, HENS_ERR_STATE, "hens_step between split 0 and split 1");
    if (c->nsplits != 2 && piped) return fail(c, HENS_ERR_UNSUPPORTED, "a ladder shard steps a two-set stretch move (hens_set_nsplits(2))");
    if (c->cfg.likelihood_kind == HENS_LIKE_HOST)
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_step needs a device likelihood (host-callable likelihoods step through hens_propose_split / hens_accept_split)");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    c->N0 = (c->W + 1) / 2;
    c->win_count = 0;
    const StepPath path = step_path(c);
    // Which queue: the in-place launches of one GPU go to the context's AQL queue (hens_aql.h) unless something in this call
    // needs the HIP stream between its launches (per-kernel events, traces, the MH move of a mix).
    const bool aql_able = c->aql_on && path.aql_able() && !c->tracing && c->mh_kind < 0 && n_iters > 0;
    // per-launch durations: mode 1 = HIP event pairs (forces the HIP stream); mode 2 = the launches' own dispatch timestamps on
    // the queue the call would use anyway - the AQL queue's packets (hens_aql.h: set_prof), HIP events where the call steps on
    // the HIP stream whatever the mode (pipeline ranks, the MH mix)
    const bool aprof = c->per_kernel_events == 2 && aql_able && !env().step_events && n_iters <= 8192;
    const bool prof = c->per_kernel_events == 1 || (c->per_kernel_events == 2 && !aprof);
    // (the state stays in record mode between hens_step calls of the record paths - every other entry point settles it,
    //  settle - so a short call pays no pack / unpack)
    if (!path.records()) state_to_fields(c);
    LaunchTimer timer;
    LaunchTimer* const tm = prof ? &timer : nullptr;
    for (hipEvent_t e : c->evpool) (void)hipEventDestroy(e);
    c->evpool.clear();
    c->timing = hens_timing{};
    // (an event pair around the call - total_ms of hens_get_timing - only when timing is asked for: per-kernel profiling or
    //  HENS_STEP_EVENTS=1.  A record is a barrier packet in front of the first launch and one more behind the last: a short
    //  call - the driver times blocks of 20 iterations - pays for both.)
    c->step_events = prof || env().step_events;
    const bool use_aql = aql_able && !c->step_events;
    if (c->aql_on && c->aql.prof != aprof && !c->aql.set_prof(aprof)) return fail(c, HENS_ERR_HIP, "AQL dispatch timestamps: %s", c->aql.err.c_str());
    if (aprof) (void)c->aql.set_prof(true);       // (clears the last call's records)
    if (use_aql) {
        c->aql.own_only = !c->hip_dirty;
        if (c->hip_dirty) {                      // the HIP stream may still be working on the state (upload, evaluation, ...)
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->hip_dirty = false;
        }
        c->aql.call_first = c->aql.windex;
        c->aql_now = true;
    } else if ((r = aql_settle(c))) return r;
    if (c->step_events) HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    // Draws are planned ON THE MAIN STREAM, right in front of the batch that consumes them (one buffer, ordered by the stream).  The
    // two-launch iteration computes its draws in registers and needs the round keys only (iteration_keys).  Rounds 1-3 planned batch
    // b + 1 on a low-priority side stream while batch b stepped; that form cost two cross-stream event waits per batch (15.8 -> 15.4
    // us per iteration at 8 x 4096 x 32 without it) and, in a soak of 10^5 iterations at 32 x 1024 x 16, one chain in five parted
    // ways with its own repeats (a plan overlapping the previous batch's readers; never with the plan on the main stream: 0 of 76
    // runs).  Round 4 removed it: no code path can reach that configuration any more (tests/test_hip_repeat.py is the soak).
    const bool one = path.it == Iteration::ONE_LAUNCH;
    for (int64_t done = 0; done < n_iters; done += c->NB) {
        const int nb = (int)std::min<int64_t>(c->NB, n_iters - done);
        if (!path.keys_only() && c->nsplits == 2) {    // (more than two sets: planned iteration by iteration, stretch_sets)
            launch_plan(c, c->stream, 0, c->iter, nb, one, one);   // (k_iter reads the block-ordered records and nothing else)
            c->timing.n_plan += 1;
            if (c->aql_failed) { c->aql_failed = false; return step_failed(c, fail(c, HENS_ERR_HIP, "AQL dispatch of the draw plan: %s", c->aql.err.c_str())); }
        }
        for (int ib = 0; ib < nb; ++ib) {
            c->aql_last = c->aql_now && done + ib + 1 == n_iters;
            if ((r = run_iteration(c, path, ib, tm))) return step_failed(c, r);
            c->iter += 1;
        }
    }
    if (c->aql_now) {                 // (every packet of the call is written: the doorbell for the rest)
        c->aql.ring();
        c->aql_now = c->aql_last = false;
    }
    if (path.it == Iteration::PIPE_COPYING) state_to_fields(c);
    if (path.it == Iteration::PIPE_INPLACE2) pipe_fused_epilogue(c);
    // The last cascade's ladder adaptation stays pending on one GPU: the next hens_step call folds it into its first
    // launch (no kernel of its own, ~12 us per call with its count-buffer reset), and every entry point that reads the ladder,
    // the swap counters or the state settles it first (settle, NEED_LADDER) - same bits either way.
    if (path.piped()) pipe_flush_adapt(c);
    HIPCHK(c, hipGetLastError());
    if (c->step_events) HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timing.n_iters = n_iters;
    if (aprof) {
        // the call's packets have their own completion signals: wait for the queue, read the stamps
        const bool dirty = c->hip_dirty;
        if ((r = aql_settle(c))) return r;
        c->hip_dirty = dirty;
        std::vector<double> us;
        std::vector<int> kinds;
        if (!c->aql.collect_prof(us, kinds)) return fail(c, HENS_ERR_HIP, "AQL dispatch timestamps: %s", c->aql.err.c_str());
        fold_timing(c, kinds, kinds.size(), [&](size_t k, double& b, double& e) { b = us[2 * k]; e = us[2 * k + 1]; return (e - b) * 1e-3; });
        if (!us.empty()) c->timing.total_ms = (us.back() - us.front()) * 1e-3;
        c->timing.clock = 2;
    }
    c->aql_prof_total = aprof;
    if (prof) {
        c->timing.clock = 1;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        const std::vector<hipEvent_t>& evs = timer.evs;
        fold_timing(c, timer.kind, timer.kind.size(), [&](size_t k, double& b, double& e) {
            float fb = 0, fe = 0, ms = 0;
            (void)hipEventElapsedTime(&fb, evs[0], evs[2 * k]);
            (void)hipEventElapsedTime(&fe, evs[0], evs[2 * k + 1]);
            (void)hipEventElapsedTime(&ms, evs[2 * k], evs[2 * k + 1]);
            b = fb * 1e3; e = fe * 1e3;
            return (double)ms;
        });
    }
    return HENS_OK;
}

// hens_step(n_before), then the accept counters as they stand are kept on the device, then hens_step(n_last): what the
// reference stores per thinned step is the accept mask of the LAST sub-iteration only (ensemble.py:968-979), and the host
// loop no longer has to split the call and read the counters in between (a settled ladder adaptation, two device-to-host
// copies and their synchronisations per stored sample).
int hens_step_marked(hens_ctx* ctx, int64_t n_before, int64_t n_last) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (n_before < 0 || n_last < 0) return fail(c, HENS_ERR_INVALID, "negative iteration count");
    int r;
    if (n_before > INT64_MAX - n_last) return fail(c, HENS_ERR_INVALID, "iteration count past INT64_MAX");
    if ((r = counter_room(c, n_before + n_last))) return r;
    if (n_before > 0 && (r = hens_step(ctx, n_before))) return r;
    if ((r = aql_settle(c))) return r;        // (what follows uses the HIP stream)
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);     // (the counters ride in the walker records during a hens_step call)
    const size_t TW = (size_t)c->Tl * c->W;
    if (!c->accepted_mark && (r = dalloc(c, &c->accepted_mark, 2 * TW))) return r;
    HIPCHK(c, hipMemcpyAsync(c->accepted_mark, c->accepted, TW * 4, hipMemcpyDeviceToDevice, c->stream));
    c->mark_mh = c->accepted_mh != nullptr;
    if (c->mark_mh) HIPCHK(c, hipMemcpyAsync(c->accepted_mark + TW, c->accepted_mh, TW * 4, hipMemcpyDeviceToDevice, c->stream));
    c->mark_valid = true;
    return n_last > 0 ? hens_step(ctx, n_last) : HENS_OK;
}

// The mark of hens_step_report and hens_step_chain: the accept counts of a call's last n_last iterations = the counters now minus
// the counters in front of those iterations.  The "before" copy (report_prev) is kept from one call to the next - the kernel that
// forms the difference moves it up (k_report_mask, k_chain_store) -, so the usual caller - one report / one stored step per n_last
// iterations - pays no snapshot, and nothing here leaves record mode: the counters are read where they ride.  Anything else that
// moved the counters in between (hens_step, a reset, another iteration counter) is noticed by the books and costs one snapshot launch.
static uint64_t report_books(const hens_ctx_impl* c) { return (uint64_t)c->num_proposals + (uint64_t)c->num_proposals_mh; }
static bool report_current(const hens_ctx_impl* c) {
    return c->report_prev && c->report_valid && c->report_iter == c->iter && c->report_books == report_books(c);
}
static void launch_report_mask(hens_ctx_impl* c, uint8_t* out) {
    const size_t TW = (size_t)c->Tl * c->W;
    const bool mh = c->accepted_mh != nullptr;
    hipLaunchKernelGGL(k_report_mask, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, c->packed ? c->wrec[c->cur] : nullptr, c->colmode ? 1 : 0,
                       c->accepted, mh ? c->accepted_mh : nullptr, c->report_prev, c->report_prev + TW, out, c->Tl, c->W);
}
static int report_snapshot(hens_ctx_impl* c) {
    const size_t TW = (size_t)c->Tl * c->W;
    int r;
    if ((r = aql_settle(c))) return r;
    SETTLE(c, NEED_DEVICE);
    if (!c->report_prev) {
        if ((r = dalloc(c, &c->report_prev, 2 * TW))) return r;
        HIPCHK(c, hipMemsetAsync(c->report_prev, 0, 2 * TW * 4, c->stream));
    }
    launch_report_mask(c, nullptr);
    HIPCHK(c, hipGetLastError());
    return HENS_OK;
}
static void report_marked(hens_ctx_impl* c, bool valid) {
    c->report_valid = valid;
    c->report_iter = c->iter;
    c->report_books = report_books(c);
}

// What a report and a stored step share: n - n_last iterations, the mark in front of the last n_last (kept from the last call where
// the books allow: report_current), those iterations, the ladder and the swap counts of their last cascade settled, then the
// consumer's launch - it reads the counters against the mark and moves the mark up, for every rung (`marks_all`) or for some.
extern "C++" {                                // (a template, in the middle of the C ABI)
template <class Consume>
static int step_to_mark(hens_ctx* ctx, int64_t n, int64_t n_last, bool marks_all, Consume&& consume) {
    hens_ctx_impl* c = CTX(ctx);
    int r;
    const bool have_prev = report_current(c) && n == n_last;
    if (n > n_last && (r = hens_step(ctx, n - n_last))) return r;
    if (!have_prev && (r = report_snapshot(c))) return r;
    if ((r = hens_step(ctx, n_last))) { c->report_valid = false; return r; }
    if ((r = aql_settle(c))) return r;        // (the consumer uses the HIP stream)
    SETTLE(c, NEED_DEVICE | NEED_LADDER);     // (the ladder AFTER the step's adaptation - what hens_download_state returns - and its swap counts)
    if ((r = consume())) return r;
    report_marked(c, marks_all);
    return HENS_OK;
}
}  // extern "C++"

// n_iters iterations and what a sampler loop reads after EVERY proposal (ensemble.py:974-977), in one call and one small copy: the
// accept counts of the call's last `n_last` iterations per walker (uint8, saturating: the reference's `accepted` of one
// sub-iteration summed over num_repeats_in_model proposals), the last cascade's swap counts and the ladder.  The walkers stay on
// the device: the drop-in moves' lazy State (eryn_amd/state.py: DeviceState) downloads them when somebody reads them.
int hens_step_report(hens_ctx* ctx, int64_t n_iters, int64_t n_last, uint8_t* accepted_last, double* swaps_last, double* betas) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c) return no_context();
    if (n_last < 1 || n_iters < n_last) return fail(c, HENS_ERR_INVALID, "hens_step_report: 1 <= n_last <= n_iters");
    if (const int r = counter_room(c, n_iters)) return r;
    const size_t TW = (size_t)c->Tl * c->W;
    return step_to_mark(ctx, n_iters, n_last, true, [&]() -> int {
        if (!c->mask_buf)
            if (const int r = dalloc(c, &c->mask_buf, TW)) return r;
        launch_report_mask(c, c->mask_buf);
        HIPCHK(c, hipGetLastError());
        if (accepted_last) HIPCHK(c, hipMemcpyAsync(accepted_last, c->mask_buf, TW, hipMemcpyDeviceToHost, c->stream));
        if (swaps_last && c->T > 1) HIPCHK(c, hipMemcpyAsync(swaps_last, c->swaps_last, (size_t)(c->T - 1) * 8, hipMemcpyDeviceToHost, c->stream));
        if (betas) HIPCHK(c, hipMemcpyAsync(betas, c->betas[c->bcur], (size_t)c->T * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->hip_dirty = false;
        return HENS_OK;
    });
}

// ---- chain store: what both families share (hens_chain_* below, hens_rj_chain_* behind hens_rj_step) ------------------------
// The host protocol of a chain, once: an entry point of either family checks what is its own (chain_supported / rjchain_supported,
// its arrays, its kernel's arguments) and calls these with its own name for the error texts.
using ChainStore = hens_ctx_impl::ChainStore;
// the context has a chain, of the family that asks (the other family's entry points see none)
static bool chain_is(const hens_ctx_impl* c, bool rj) { return c->chain.on && rj == is_rj(c); }
static int chain_open(hens_ctx_impl* c, bool rj) {
    if (!chain_is(c, rj)) return fail(c, HENS_ERR_STATE, "no chain (%s)", rj ? "hens_rj_chain_create" : "hens_chain_create");
    return HENS_OK;
}
static int chain_Ts(const hens_ctx_impl* c, bool rj) { return chain_is(c, rj) ? c->chain.Ts : c->T; }   // (no chain: what one would store)
// swap slots of a ladder: the allocations and their memsets hold at least one (T = 1), the totals copy what there is
static size_t swap_slots(const hens_ctx_impl* c, int least) { return (size_t)std::max(c->T - 1, least); }

static int chain_reset(hens_ctx_impl* c) {
    ChainStore& ch = c->chain;
    SETTLE(c, NEED_DEVICE);
    for (uint32_t* tot : {ch.acc_tot, ch.bd_tot})        // (bd_tot: a leaf-packing chain has it)
        if (tot) HIPCHK(c, hipMemsetAsync(tot, 0, (size_t)ch.Ts * c->W * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(ch.swaps_tot, 0, swap_slots(c, 1) * 8, c->stream));
    ch.count = 0;
    ch.iteration.clear(); ch.adapt_time.clear();
    return HENS_OK;
}

// hens_*chain_create in two halves, the family's overflow-checked sizes in between: the arguments, giving the stored rungs ...
static int chain_create_args(hens_ctx_impl* c, const char* who, int64_t capacity, int32_t ntemps_store, int* Ts) {
    if (capacity < 1) return fail(c, HENS_ERR_INVALID, "%s: capacity < 1", who);
    if (ntemps_store < 0 || ntemps_store > c->T) return fail(c, HENS_ERR_INVALID, "%s: ntemps_store outside [0, %d]", who, c->T);
    *Ts = ntemps_store ? ntemps_store : c->T;
    return HENS_OK;
}
// ... and the chain itself from the family's list of (pointer in c->chain, bytes); `bytes` is the list's sum: the side arrays count
struct ChainBuf { void* p; size_t bytes; };
static int chain_create(hens_ctx_impl* c, const char* who, int64_t capacity, int Ts, const std::vector<ChainBuf>& bufs) {
    SETTLE(c, NEED_DEVICE);
    HIPCHK(c, hipStreamSynchronize(c->stream));     // (a chain being replaced may still be written)
    ChainStore& ch = c->chain;
    ch.release();
    int64_t bytes = 0;
    bool ok = true;
    for (const ChainBuf& b : bufs) {
        bytes += (int64_t)b.bytes;
        if (ok && (ok = hipMalloc((void**)b.p, b.bytes) == hipSuccess)) ch.owned.push_back(*(void**)b.p);
    }
    if (!ok) {
        const hipError_t e = hipGetLastError();     // (cleared: the stepping calls check it)
        ch.release();
        return fail(c, HENS_ERR_HIP, "%s: allocating %lld bytes of device memory for %lld stored steps failed: %s",
                    who, (long long)bytes, (long long)capacity, hipGetErrorString(e));
    }
    ch.capacity = capacity; ch.Ts = Ts; ch.bytes = bytes;
    ch.on = true;
    return chain_reset(c);
}

static int chain_destroy(hens_ctx_impl* c, bool rj) {
    if (!chain_is(c, rj)) return HENS_OK;
    SETTLE(c, NEED_DEVICE);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->chain.release();
    return HENS_OK;
}

// `step_bytes`: the family's sizes of one step of chain_Ts rungs
static int chain_info(hens_ctx_impl* c, bool rj, int64_t step_bytes, hens_chain_info_t* out) {
    static_assert(sizeof(hens_chain_info_t) == 64, "hens_chain_info_t: 7 x i64 + f64 (eryn_amd/_lib.py: HensChainInfo)");
    const ChainStore none{};
    const ChainStore& ch = chain_is(c, rj) ? c->chain : none;
    hens_chain_info_t o{};
    o.capacity = ch.capacity; o.count = ch.count; o.ntemps_store = ch.Ts; o.bytes = ch.bytes; o.step_bytes = step_bytes;
    o.n_store_timed = ch.n_timed; o.store_ms = ch.store_ms;
    SETTLE(c, NEED_DEVICE);
    size_t fr = 0, tot = 0;
    HIPCHK(c, hipMemGetInfo(&fr, &tot));
    o.free_bytes = (int64_t)fr;
    *out = o;
    return HENS_OK;
}

// the event pairs around a call's append launches while hens_set_profiling is 1 (at most 4096 pairs: later appends go untimed);
// the call's store_ms / n_timed start at zero with it, and whatever way the call ends, the events go with it
struct ChainTimer {
    ChainStore& ch;
    const bool on;
    std::vector<hipEvent_t> evs;
    explicit ChainTimer(hens_ctx_impl* c) : ch(c->chain), on(c->per_kernel_events == 1) { ch.n_timed = 0; ch.store_ms = 0.0; }
    ~ChainTimer() { for (hipEvent_t e : evs) (void)hipEventDestroy(e); }
    int pair(hens_ctx_impl* c, hipEvent_t e[2]) {          // nulls: this append is not timed
        e[0] = e[1] = nullptr;
        if (!on || evs.size() >= 2 * 4096) return HENS_OK;
        for (int k = 0; k < 2; ++k) { HIPCHK(c, hipEventCreate(&e[k])); evs.push_back(e[k]); }
        return HENS_OK;
    }
    // after the caller's own synchronisation of the stream: hens_step_chain waits for it itself when there is a pair to read,
    // hens_rj_step_chain has check_flags' wait behind it either way
    void fold() {
        for (size_t k = 0; k + 1 < evs.size(); k += 2) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, evs[k], evs[k + 1]) == hipSuccess) { ch.store_ms += ms; ch.n_timed += 1; }
        }
    }
};

// one append on the HIP stream, its argument block filled by the family: Ts W records of 2^lpr_shift lanes each; then the stored
// step's books
static int chain_append(hens_ctx_impl* c, ChainTimer& tm, const void* fn, void* block, int lpr_shift) {
    ChainStore& ch = c->chain;
    hipEvent_t e[2];
    if (const int r = tm.pair(c, e)) return r;
    const int64_t threads = (int64_t)((size_t)ch.Ts * c->W) << lpr_shift;
    const dim3 grid((unsigned)((threads + 255) / 256));
    void* args[] = {block};
    if (e[0]) (void)hipExtLaunchKernel(fn, grid, dim3(256), args, 0, c->stream, e[0], e[1], 0);
    else (void)hipLaunchKernel(fn, grid, dim3(256), args, 0, c->stream);
    HIPCHK(c, hipGetLastError());
    ch.iteration.push_back((int64_t)c->iter);
    ch.adapt_time.push_back(c->adapt_time);
    ch.count += 1;
    return HENS_OK;
}

// hens_*chain_download in two halves, a family's own checks in between: the open chain and the range ...
static int chain_range(hens_ctx_impl* c, bool rj, const char* who, int64_t first, int64_t count) {
    if (const int r = chain_open(c, rj)) return r;
    if (!hens_chain::range_ok(c->chain.count, first, count))
        return fail(c, HENS_ERR_INVALID, "%s: steps [%lld, %lld + %lld) outside the %lld stored", who, (long long)first, (long long)first, (long long)count, (long long)c->chain.count);
    return HENS_OK;
}
// ... and the copies: the family's own fields (`step` bytes per stored step each), logl / logp / betas, one wait if anything was
// copied, the checkpoints.  A null destination is a field not asked for.
struct ChainCopy { void* dst; const void* src; size_t step; };
static int chain_copy_out(hens_ctx_impl* c, int64_t first, int64_t count, std::initializer_list<ChainCopy> own, double* logl, double* logp,
                          double* betas, int64_t* iteration, int64_t* adapt_time) {
    if (count == 0) return HENS_OK;
    const ChainStore& ch = c->chain;
    SETTLE(c, NEED_DEVICE);
    const size_t lp = (size_t)ch.Ts * c->W * 8;
    bool copied = false;
    auto copy = [&](const ChainCopy& f) {
        if (!f.dst) return hipSuccess;
        copied = true;
        return hipMemcpyAsync(f.dst, static_cast<const char*>(f.src) + (size_t)first * f.step, (size_t)count * f.step, hipMemcpyDeviceToHost, c->stream);
    };
    for (const ChainCopy& f : own) HIPCHK(c, copy(f));
    for (const ChainCopy& f : {ChainCopy{logl, ch.L, lp}, ChainCopy{logp, ch.P, lp}, ChainCopy{betas, ch.betas, (size_t)c->T * 8}}) HIPCHK(c, copy(f));
    if (copied) HIPCHK(c, hipStreamSynchronize(c->stream));
    if (iteration) std::copy(ch.iteration.begin() + first, ch.iteration.begin() + first + count, iteration);
    if (adapt_time) std::copy(ch.adapt_time.begin() + first, ch.adapt_time.begin() + first + count, adapt_time);
    return HENS_OK;
}

// hens_*chain_totals: the family's [Ts][W] counters (destination, device array) and the swap totals, widened to double
static int chain_totals(hens_ctx_impl* c, std::initializer_list<CounterOut> tots, double* swaps_accepted) {
    const ChainStore& ch = c->chain;
    SETTLE(c, NEED_DEVICE);
    const size_t np = swap_slots(c, 0);
    std::vector<unsigned long long> sw(swaps_accepted ? np : 0);
    const int r = read_counters(c, (size_t)ch.Ts * c->W, tots, [&]() -> int {
        if (!sw.empty()) HIPCHK(c, hipMemcpyAsync(sw.data(), ch.swaps_tot, np * 8, hipMemcpyDeviceToHost, c->stream));
        return HENS_OK;
    });
    if (r) return r;
    std::copy(sw.begin(), sw.end(), swaps_accepted);
    return HENS_OK;
}

// ---- chain store (include/hipensemble.h: hens_chain_*, hens_step_chain; csrc/hens_chain.h: k_chain_store) -------------------
static int chain_supported(hens_ctx_impl* c) {
    if (is_rj(c))
        return fail(c, HENS_ERR_UNSUPPORTED, "chain store: not on a leaf-packing context (records of several branches and leaves: hens_rj_chain_create / hens_rj_step_chain)");
    if (c->cfg.likelihood_kind == HENS_LIKE_HOST)
        return fail(c, HENS_ERR_UNSUPPORTED, "chain store: needs a device likelihood (a host-callable likelihood steps through the caller)");
    if (c->Tl != c->T) return fail(c, HENS_ERR_UNSUPPORTED, "chain store: not on a ladder shard (the whole ladder on one GPU)");
    if (c->pipe.on) return fail(c, HENS_ERR_UNSUPPORTED, "chain store: not on a rank of the ladder pipeline");
    return HENS_OK;
}
static hens_chain::Shape chain_shape(const hens_ctx_impl* c, int Ts) { return hens_chain::Shape{c->T, Ts, c->W, dim_active(c)}; }

int hens_chain_create(hens_ctx* ctx, int64_t capacity, int32_t ntemps_store) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r, Ts = 0;
    if ((r = chain_supported(c)) || (r = chain_create_args(c, "hens_chain_create", capacity, ntemps_store, &Ts))) return r;
    hens_chain::Sizes sz{};
    if (!hens_chain::sizes(chain_shape(c, Ts), capacity, &sz))
        return fail(c, HENS_ERR_INVALID, "hens_chain_create: %lld stored steps of %d x %d x %d do not fit an int64 byte count", (long long)capacity, Ts, c->W, dim_active(c));
    ChainStore& ch = c->chain;
    return chain_create(c, "hens_chain_create", capacity, Ts, {{&ch.x[0], (size_t)sz.x}, {&ch.L, (size_t)sz.lp}, {&ch.P, (size_t)sz.lp}, {&ch.betas, (size_t)sz.betas},
                                                               {&ch.acc_tot, (size_t)Ts * c->W * 4}, {&ch.swaps_tot, swap_slots(c, 1) * 8}});
}

int hens_chain_reset(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = chain_open(c, false)) return r;
    return chain_reset(c);
}

int hens_chain_destroy(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    return chain_destroy(c, false);
}

// answers on any context, with capacity 0 where there is no chain of this family (DeviceBackend asks before it creates one)
int hens_chain_info(hens_ctx* ctx, hens_chain_info_t* out) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c || !out) return fail(c, HENS_ERR_INVALID, "null argument");
    hens_chain::Sizes one{};
    (void)hens_chain::sizes(chain_shape(c, chain_Ts(c, false)), 1, &one);
    return chain_info(c, false, one.step, out);
}

// one append: the state as it stands behind a hens_step call, the ladder and swap counts settled by the caller
static int launch_chain_store(hens_ctx_impl* c, ChainTimer& tm) {
    ChainStore& ch = c->chain;
    const size_t TW = (size_t)c->Tl * c->W, TsW = (size_t)ch.Ts * c->W;
    const int D = dim_active(c);
    ChainArgs a{};
    a.wrec = c->packed ? c->wrec[c->cur] : nullptr;
    a.L = c->L[c->cur]; a.P = c->P[c->cur]; a.loc = c->loc[c->cur];
    a.acc_fields = c->accepted;
    a.acc_mh = c->accepted_mh;
    a.prev = c->report_prev; a.prev_mh = c->report_prev + TW;
    a.pool = c->pool;
    a.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    a.swaps_last = has_pt(c) ? c->swaps_last : nullptr;
    a.out_x = ch.x[0] + (size_t)ch.count * TsW * D;
    a.out_L = ch.L + (size_t)ch.count * TsW; a.out_P = ch.P + (size_t)ch.count * TsW;
    a.out_betas = ch.betas + (size_t)ch.count * c->T;
    a.acc_tot = ch.acc_tot; a.swaps_tot = ch.swaps_tot;
    a.colmode = c->colmode ? 1 : 0; a.T = c->T; a.W = c->W; a.Ts = ch.Ts; a.RW = c->D; a.D = D;
    // the row as one segment of D doubles: 16 bytes per lane where both sides' rows are 16-byte aligned, else 8; a row to the smallest
    // power of two of lanes that covers it (at most a wave: wider rows take several rounds)
    const hens_chain::RjShape row = hens_chain::one_segment(chain_shape(c, ch.Ts));
    const int vec = hens_chain::rj_store_vec(row, c->D);
    a.lpr_shift = hens_chain::rj_lane_shift(row, vec);
    const void* fn = vec == 2 ? reinterpret_cast<const void*>(k_chain_store<2>) : reinterpret_cast<const void*>(k_chain_store<1>);
    return chain_append(c, tm, fn, &a, a.lpr_shift);
}

int hens_step_chain(hens_ctx* ctx, int64_t n_store, int64_t iters_per_store, int64_t n_last) {
    hens_ctx_impl* c = CTX(ctx);              // (not `enter`, as every other chain entry point: hens_step below settles the queue itself)
    if (!c) return no_context();
    int r;
    if ((r = chain_supported(c)) || (r = chain_open(c, false))) return r;
    ChainStore& ch = c->chain;
    int64_t iters = 0;
    switch (hens_chain::append_check(ch.capacity, ch.count, n_store, iters_per_store, n_last, &iters)) {
    case hens_chain::INVALID: return fail(c, HENS_ERR_INVALID, "hens_step_chain: n_store >= 0 and 1 <= n_last <= iters_per_store, and their product an int64");
    case hens_chain::FULL: return fail(c, HENS_ERR_STATE, "hens_step_chain: %lld more stored steps do not fit a chain of capacity %lld that holds %lld (download and hens_chain_reset)",
                                       (long long)n_store, (long long)ch.capacity, (long long)ch.count);
    default: break;
    }
    if ((r = counter_room(c, iters))) return r;
    ChainTimer tm(c);
    for (int64_t s = 0; s < n_store; ++s)         // (k_chain_store moves the mark up to now - of the rungs it stores)
        if ((r = step_to_mark(ctx, iters_per_store, n_last, ch.Ts == c->Tl, [&] { return launch_chain_store(c, tm); }))) return r;
    if (!tm.evs.empty()) {                        // (nothing else in this call waits for the stream)
        HIPCHK(c, hipStreamSynchronize(c->stream));
        tm.fold();
    }
    return HENS_OK;
}

int hens_chain_download(hens_ctx* ctx, int64_t first, int64_t count, double* x, double* logl, double* logp, double* betas,
                        int64_t* iteration, int64_t* adapt_time) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = chain_range(c, false, "hens_chain_download", first, count)) return r;
    const size_t row = (size_t)c->chain.Ts * c->W * dim_active(c) * 8;
    return chain_copy_out(c, first, count, {{x, c->chain.x[0], row}}, logl, logp, betas, iteration, adapt_time);
}

int hens_chain_totals(hens_ctx* ctx, double* accepted, double* swaps_accepted) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = chain_open(c, false)) return r;
    return chain_totals(c, {{accepted, c->chain.acc_tot}}, swaps_accepted);
}

// ---- chain diagnostics (include/hipensemble.h: hens_chain_moments, hens_chain_act; csrc/hens_chain_stats.h) -----------------
static int chain_stats_enter(hens_ctx_impl* c, const char* who) {
    if (is_rj(c))
        return fail(c, HENS_ERR_UNSUPPORTED, "%s: not built for a leaf-packing context - the autocorrelation time is not defined under reversible jump "
                    "(the reference refuses it as well) and the Gelman-Rubin diagnostic of a branch of several leaves needs the projection through the leaf masks", who);
    if (!c->chain.on) return fail(c, HENS_ERR_STATE, "no chain (hens_chain_create)");
    return HENS_OK;
}

// one diagnostics launch on the HIP stream between two events, its argument block filled by the caller, its outputs (device arrays
// inside `dev`, which is freed here) copied to the caller's arrays that are not null
struct StatOut { void* host; const void* dev; size_t bytes; };
static int chain_stats_run(hens_ctx_impl* c, const void* fn, dim3 grid, dim3 block, size_t lds, void* arg_block, char* dev,
                           std::initializer_list<StatOut> outs, double* ms_out, const char* what) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
        if (e0) (void)hipEventDestroy(e0);
        (void)hipFree(dev);
        return fail(c, HENS_ERR_HIP, "%s: hipEventCreate failed", what);
    }
    void* args[] = {arg_block};
    hipError_t e = hipExtLaunchKernel(fn, grid, block, args, lds, c->stream, e0, e1, 0);
    for (const StatOut& o : outs)
        if (o.host && o.bytes && e == hipSuccess) e = hipMemcpyAsync(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    float ms = 0;
    *ms_out = (e == hipSuccess && hipEventElapsedTime(&ms, e0, e1) == hipSuccess) ? (double)ms : -1.0;
    (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(c, HENS_ERR_HIP, "%s failed: %s", what, hipGetErrorString(e));
    return HENS_OK;
}

// k_chain_moments over one array of a chain of either family: `base` the field's array, `pl` its plan (hens_chain_host.h)
static int chain_moments_run(hens_ctx_impl* c, const double* base, const hens_chain::StatPlan& pl, int64_t count, bool mask, double* sum,
                             double* m2, int64_t* n_finite, const char* who) {
    const int64_t blocks = hens_chain::stat_blocks(pl.nseries / pl.vec, 256);
    if (blocks > INT32_MAX) return fail(c, HENS_ERR_UNSUPPORTED, "%s: %lld series are more than one launch covers", who, (long long)pl.nseries);
    if (!sum && !m2 && !n_finite) return HENS_OK;
    SETTLE(c, NEED_DEVICE);
    char* dev = nullptr;
    const size_t bytes = (size_t)pl.nseries * 8;
    HIPCHK(c, hipMalloc((void**)&dev, bytes * 3));
    ChainStatArgs a{};
    a.src = base + pl.offset;
    a.stride = pl.stride; a.count = count; a.nseries = pl.nseries;
    a.sum = reinterpret_cast<double*>(dev);
    a.m2 = m2 ? reinterpret_cast<double*>(dev) + pl.nseries : nullptr;
    a.nfin = reinterpret_cast<long long*>(dev) + 2 * pl.nseries;
    const void* fn = pl.vec == 2 ? (mask ? reinterpret_cast<const void*>(k_chain_moments<2, true>) : reinterpret_cast<const void*>(k_chain_moments<2, false>))
                                 : (mask ? reinterpret_cast<const void*>(k_chain_moments<1, true>) : reinterpret_cast<const void*>(k_chain_moments<1, false>));
    return chain_stats_run(c, fn, dim3((unsigned)blocks), dim3(256), 0, &a, dev, {{sum, dev, bytes}, {m2, dev + bytes, bytes}, {n_finite, dev + 2 * bytes, bytes}},
                           &c->chain.moments_ms, "k_chain_moments");
}

int hens_chain_moments(hens_ctx* ctx, int32_t field, int64_t first, int64_t count, int64_t thin, int32_t ntemps,
                       double* sum, double* m2, int64_t* n_finite) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r;
    if ((r = chain_stats_enter(c, "hens_chain_moments"))) return r;
    ChainStore& ch = c->chain;
    hens_chain::StatPlan pl{};
    if (!hens_chain::stat_plan(chain_shape(c, ch.Ts), ch.count, field, first, count, thin, ntemps, &pl))
        return fail(c, HENS_ERR_INVALID, "hens_chain_moments: field %d in [0, 2], count >= 1, thin >= 1, ntemps %d in [1, %d] and the kept steps %lld, %lld + %lld, ... (%lld of them) inside the %lld stored",
                    field, ntemps, ch.Ts, (long long)first, (long long)first, (long long)thin, (long long)count, (long long)ch.count);
    return chain_moments_run(c, field == 0 ? ch.x[0] : field == 1 ? ch.L : ch.P, pl, count, field != 0, sum, m2, n_finite, "hens_chain_moments");
}

int hens_chain_act(hens_ctx* ctx, int64_t first, int64_t count, int64_t thin, int32_t ntemps, int32_t window,
                   double* tau, double* mean, double* c0) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r;
    if ((r = chain_stats_enter(c, "hens_chain_act"))) return r;
    ChainStore& ch = c->chain;
    hens_chain::StatPlan pl{};
    if (window < 1 || !hens_chain::stat_plan(chain_shape(c, ch.Ts), ch.count, 0, first, count, thin, ntemps, &pl))
        return fail(c, HENS_ERR_INVALID, "hens_chain_act: window >= 1, count >= 1, thin >= 1, ntemps %d in [1, %d] and the kept steps %lld, %lld + %lld, ... (%lld of them) inside the %lld stored",
                    ntemps, ch.Ts, (long long)first, (long long)first, (long long)thin, (long long)count, (long long)ch.count);
    const int64_t lags = hens_chain::act_lags(window, count);
    if (!hens_chain::act_fits(lags))
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_chain_act: %lld lags (min(window, kept steps)) are more than the %d a lane's accumulators and LDS ring hold",
                    (long long)lags, hens_chain::ACT_WINDOW_MAX);
    static_assert(hens_chain::ACT_LANES == ACT_LANES, "hens_chain_host.h sizes the ring of k_chain_act");
    const int64_t blocks = hens_chain::stat_blocks(pl.nseries, ACT_LANES);
    if (blocks > INT32_MAX) return fail(c, HENS_ERR_UNSUPPORTED, "hens_chain_act: %lld series are more than one launch covers", (long long)pl.nseries);
    if (!tau && !mean && !c0) return HENS_OK;
    SETTLE(c, NEED_DEVICE);
    char* dev = nullptr;
    HIPCHK(c, hipMalloc((void**)&dev, (size_t)pl.nseries * 8 * 3));
    ChainStatArgs a{};
    a.src = ch.x[0] + pl.offset;
    a.stride = pl.stride; a.count = count; a.nseries = pl.nseries;
    a.tau = reinterpret_cast<double*>(dev); a.mean = a.tau + pl.nseries; a.c0 = a.mean + pl.nseries;
    a.K = (int32_t)lags;
    const int kmax = hens_chain::act_kmax(lags);
    const void* fn = kmax == 16 ? reinterpret_cast<const void*>(k_chain_act<16>) : kmax == 32 ? reinterpret_cast<const void*>(k_chain_act<32>)
                                                                                              : reinterpret_cast<const void*>(k_chain_act<64>);
    const size_t bytes = (size_t)pl.nseries * 8;
    return chain_stats_run(c, fn, dim3((unsigned)blocks), dim3(ACT_LANES), (size_t)hens_chain::act_lds_bytes(lags), &a, dev,
                           {{tau, dev, bytes}, {mean, dev + bytes, bytes}, {c0, dev + 2 * bytes, bytes}}, &ch.act_ms, "k_chain_act");
}

int hens_chain_stats_ms(hens_ctx* ctx, double* moments_ms, double* act_ms) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c) return no_context();
    if (moments_ms) *moments_ms = c->chain.moments_ms;
    if (act_ms) *act_ms = c->chain.act_ms;
    return HENS_OK;
}

// the counters kept by the last hens_step_marked call ([Tl][W] each; accepted_mh may be null; zeros if there is no MH move)
int hens_get_marked_counters(hens_ctx* ctx, double* accepted, double* accepted_mh) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!c->mark_valid) return fail(c, HENS_ERR_STATE, "hens_get_marked_counters without hens_step_marked");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W;
    std::vector<double> both(2 * TW, 0.0);                // (one copy of the mark: [stretch | MH, where there is an MH move])
    if (const int r = read_counters(c, (c->mark_mh ? 2 : 1) * TW, {{both.data(), c->accepted_mark}})) return r;
    if (accepted) std::copy_n(both.data(), TW, accepted);
    if (accepted_mh) std::copy_n(both.data() + TW, TW, accepted_mh);
    return HENS_OK;
}

int hens_get_counters(hens_ctx* ctx, double* accepted, int64_t* num_proposals, double* swaps_last, double* swaps_total,
                      int64_t* adapt_time) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    const int r = read_counters(c, (size_t)c->Tl * c->W, {{accepted, c->accepted}}, [&]() -> int {      // (the swap arrays under the same wait)
        if (swaps_last && c->T > 1) HIPCHK(c, hipMemcpyAsync(swaps_last, c->swaps_last, (size_t)(c->T - 1) * 8, hipMemcpyDeviceToHost, c->stream));
        if (swaps_total && c->T > 1) HIPCHK(c, hipMemcpyAsync(swaps_total, c->swaps_total, (size_t)(c->T - 1) * 8, hipMemcpyDeviceToHost, c->stream));
        return HENS_OK;
    });
    if (r) return r;
    if (num_proposals) *num_proposals = c->num_proposals;
    if (adapt_time) *adapt_time = c->adapt_time;
    return HENS_OK;
}

int hens_reset_counters(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    HIPCHK(c, hipMemsetAsync(c->accepted, 0, (size_t)c->Tl * c->W * 4, c->stream));
    HIPCHK(c, hipMemsetAsync(c->swaps_total, 0, (size_t)c->T * 8, c->stream));
    HIPCHK(c, hipMemsetAsync(c->swaps_last, 0, (size_t)c->T * 8, c->stream));
    if (c->accepted_mh) HIPCHK(c, hipMemsetAsync(c->accepted_mh, 0, (size_t)c->Tl * c->W * 4, c->stream));
    if (c->rj.acc_bd) HIPCHK(c, hipMemsetAsync(c->rj.acc_bd, 0, (size_t)c->Tl * c->W * 4, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->num_proposals = 0;
    c->num_proposals_mh = 0;
    c->rj.num_mh = c->rj.num_bd = 0;
    c->report_valid = false;
    c->chain.mark_valid = false;
    return HENS_OK;
}

int hens_set_adapt_time(hens_ctx* ctx, int64_t t) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    c->adapt_time = t;
    return HENS_OK;
}

int hens_set_iteration(hens_ctx* ctx, int64_t iter) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (iter < 0) return fail(c, HENS_ERR_INVALID, "iteration counter < 0");
    if (pipe_active(c) && c->pipe.sweep > 0)
        return fail(c, HENS_ERR_STATE, "the iteration counter of a pipeline rank that has stepped cannot be moved");
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);     // (column-ordered records are in the OLD counter's order)
    c->win_count = 0;
    c->iter = (uint64_t)iter;                 // (the round-key window re-plans itself when the chain has left it)
    return HENS_OK;
}

int hens_set_profiling(hens_ctx* ctx, int32_t per_kernel_events) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c) return no_context();
    if (per_kernel_events < 0 || per_kernel_events > 2) return fail(c, HENS_ERR_INVALID, "hens_set_profiling: mode 0, 1 or 2");
    c->per_kernel_events = per_kernel_events;
    return HENS_OK;
}

int hens_get_timing(hens_ctx* ctx, hens_timing* out) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c || !out) return fail(c, HENS_ERR_INVALID, "null argument");
    HIPCHK(c, hipSetDevice(c->cfg.device_id));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    float ms = 0;
    if (c->timing.n_iters > 0 && c->step_events) HIPCHK(c, hipEventElapsedTime(&ms, c->ev0, c->ev1));
    if (!c->aql_prof_total) c->timing.total_ms = ms;      // (dispatch-timestamp mode: first begin to last end, set by hens_step)
    *out = c->timing;
    return HENS_OK;
}

// begin / end of every launch of the last hens_step call made with per-kernel events (us after the first launch's begin)
int hens_debug_launch_times(hens_ctx* ctx, double* out_us, int64_t capacity, int64_t* n_out) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c || !n_out) return fail(c, HENS_ERR_INVALID, "null argument");
    const int64_t n = std::min<int64_t>(capacity, (int64_t)c->launch_us.size());
    for (int64_t i = 0; i < n && out_us; ++i) out_us[i] = c->launch_us[(size_t)i];
    *n_out = (int64_t)c->launch_us.size();
    return HENS_OK;
}

int hens_debug_trace(hens_ctx* ctx, int32_t enable, uint64_t* out, int64_t capacity, int64_t* n_out) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    SETTLE(c, NEED_DEVICE);
    const int64_t words = std::max<int64_t>((int64_t)c->Tl * ((c->W + TILE - 1) / TILE), pt_blocks(c)) * 8;
    if (enable) {
        if (!c->d_trace) {
            int r = dalloc(c, &c->d_trace, (size_t)words);
            if (r) return r;
            c->trace_words = words;
        }
        HIPCHK(c, hipMemsetAsync(c->d_trace, 0, (size_t)words * 8, c->stream));
        c->tracing = true;
        c->trace_pt = enable == 2;           // 1: stretch kernel, 2: PT cascade, 3: fused half-step + cascade
        c->trace_fused = enable == 3;
        c->trace_rj = enable == 4 ? RJ_MODE_MH : (enable == 5 ? RJ_MODE_BD : -1);
        if (c->trace_rj >= 0) c->trace_pt = true;        // (keeps the stretch / fused kernels' own stamps out)
        return HENS_OK;
    }
    c->tracing = false;
    if (!c->d_trace || !out) return fail(c, HENS_ERR_STATE, "tracing was not enabled");
    const int64_t n = std::min<int64_t>(capacity, c->trace_words);
    HIPCHK(c, hipMemcpyAsync(out, c->d_trace, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (n_out) *n_out = n;
    return HENS_OK;
}

int hens_debug_permutation(hens_ctx* ctx, int32_t which, int32_t rung, int64_t iter, int32_t* out) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !out) return fail(c, HENS_ERR_INVALID, "null argument");
    SETTLE(c, NEED_DEVICE);
    int32_t* d = reinterpret_cast<int32_t*>(c->xtmp);          // scratch: at least W * 4 bytes
    hipLaunchKernelGGL(k_debug_prp, dim3(grid_for(c->W)), dim3(256), 0, c->stream, d, c->W, c->idx_bits, c->cfg.seed,
                       (uint64_t)iter, which == 0 ? PURPOSE_PTPERM : PURPOSE_SPLIT, (uint32_t)rung);
    HIPCHK(c, hipMemcpyAsync(out, d, (size_t)c->W * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

int hens_get_iteration(hens_ctx* ctx, int64_t* iter_out) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c || !iter_out) return fail(c, HENS_ERR_INVALID, "null argument");
    *iter_out = (int64_t)c->iter;
    return HENS_OK;
}

// hens_debug_draws under the distribution proposal: what k_dist draws in iteration `iter` - q[tl][w][d] from the same function
// (dist_draw; a pad coordinate, which has no draw, reads 0) and the accept uniform of every walker (mh_uniform).  Export only.
__global__ void k_dist_draw(double* q, double* u, const double* glo, const double* ghi, const PriorTerm* gterms, uint64_t seed, uint64_t iter,
                            int Tl, int W, int D, int rung_begin) {
    const int64_t n = (int64_t)Tl * W * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const int64_t tw = i / D;
        const int tl = (int)(tw / W), w = (int)(tw % W);
        const uint32_t wid = (uint32_t)(rung_begin + tl) * (uint32_t)W + (uint32_t)w;
        const PriorTerm t = gterms[d];
        q[i] = t.kind == PRIOR_NONE ? 0.0 : dist_draw(seed, iter, wid, d, t, glo[d], ghi[d]);
        if (d == 0) u[tw] = mh_uniform(seed, iter, wid);
    }
}

// hens_mt_debug_draws: what k_mt_dist draws in iteration `iter` - q[tl][w][k][d] from dist_draw with the try in the counter word (a
// pad coordinate reads 0), the pick uniform (mt_pick_uniform) and the accept uniform (mh_uniform) of every walker.  Export only.
__global__ void k_mt_draw(double* q, double* u_pick, double* u_acc, const double* glo, const double* ghi, const PriorTerm* gterms, uint64_t seed,
                          uint64_t iter, int Tl, int W, int K, int D, int rung_begin) {
    const int64_t n = (int64_t)Tl * W * K * D;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int d = (int)(i % D);
        const int k = (int)((i / D) % K);
        const int64_t tw = i / ((int64_t)D * K);
        const int tl = (int)(tw / W), w = (int)(tw % W);
        const uint32_t wid = (uint32_t)(rung_begin + tl) * (uint32_t)W + (uint32_t)w;
        const PriorTerm t = gterms[d];
        q[i] = t.kind == PRIOR_NONE ? 0.0 : dist_draw(seed, iter, wid, d, t, glo[d], ghi[d], (uint32_t)k);
        if (d == 0 && k == 0) {
            u_pick[tw] = mt_pick_uniform(seed, iter, wid);
            u_acc[tw] = mh_uniform(seed, iter, wid);
        }
    }
}

int hens_mt_debug_draws(hens_ctx* ctx, int64_t iter, double* q, double* u_pick, double* u_acc) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (c->mh_kind != MH_MT_DIST) return fail(c, HENS_ERR_STATE, "no generator set (hens_set_mt_dist_proposal)");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W, nq = TW * c->mt_K * c->D;
    DeviceScratch sc;
    double* dq = sc.grab<double>(nq);
    double* dp = sc.grab<double>(TW);
    double* du = sc.grab<double>(TW);
    if (!dq || !dp || !du) return fail(c, HENS_ERR_HIP, "hens_mt_debug_draws: out of device memory");
    hipLaunchKernelGGL(k_mt_draw, dim3(grid_for((int64_t)nq)), dim3(256), 0, c->stream, dq, dp, du, c->dist_block.lo(), c->dist_block.hi(),
                       c->dist_block.terms(), c->cfg.seed, (uint64_t)iter, c->Tl, c->W, c->mt_K, c->D, (int)c->cfg.rung_begin);
    HIPCHK(c, hipGetLastError());
    if (q) HIPCHK(c, hipMemcpyAsync(q, dq, nq * 8, hipMemcpyDeviceToHost, c->stream));
    if (u_pick) HIPCHK(c, hipMemcpyAsync(u_pick, dp, TW * 8, hipMemcpyDeviceToHost, c->stream));
    if (u_acc) HIPCHK(c, hipMemcpyAsync(u_acc, du, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

int hens_debug_draws(hens_ctx* ctx, int64_t iter, int32_t* own, int32_t* cw, double* u_zz, double* u_acc,
                     int32_t* pt_slot, double* u_swap, int32_t* is_mh, double* mh_step, double* mh_u) {
    return hens_debug_draws_block(ctx, iter, 0, own, cw, u_zz, u_acc, pt_slot, u_swap, is_mh, mh_step, mh_u);
}

// ... of Gibbs block `block` of that iteration's move (hens_set_gibbs): own, the PT draws and the move choice are the iteration's;
// cw, u_zz, u_acc (k_plan_block) and mh_step, mh_u (k_mh_draw) come from the block's purpose words.  Block 0 is hens_debug_draws.
int hens_debug_draws_block(hens_ctx* ctx, int64_t iter, int32_t block, int32_t* own, int32_t* cw, double* u_zz, double* u_acc,
                           int32_t* pt_slot, double* u_swap, int32_t* is_mh, double* mh_step, double* mh_u) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (block < 0 || block >= c->gibbs[iteration_is_mh(c, (uint64_t)iter) ? 1 : 0].blocks())
        return fail(c, HENS_ERR_INVALID, "block must be in [0, %d): the blocks of that iteration's move", c->gibbs[iteration_is_mh(c, (uint64_t)iter) ? 1 : 0].blocks());
    // the OTHER move's arrays are the block's only where its table has such a block: else they are not written
    if (block >= c->gibbs[0].blocks()) cw = nullptr, u_zz = u_acc = nullptr;
    if (block >= c->gibbs[1].blocks()) mh_step = mh_u = nullptr;
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W;
    DeviceScratch sc;
    const bool mh = iteration_is_mh(c, (uint64_t)iter);
    if (is_mh) *is_mh = mh ? 1 : 0;
    if (own || cw || u_zz || u_acc) {     // the stretch plan of that iteration, exactly as hens_step's plan kernel makes it
        PlanArgs pa{};
        pa.dr.own = sc.grab<int32_t>(TW); pa.dr.cw = sc.grab<int32_t>(TW);
        pa.dr.zz = sc.grab<double>(TW); pa.dr.fac = sc.grab<double>(TW); pa.dr.lu = sc.grab<double>(TW);
        pa.dbg_uzz = sc.grab<double>(TW); pa.dbg_uacc = sc.grab<double>(TW);
        if (!pa.dr.own || !pa.dr.cw || !pa.dr.zz || !pa.dr.fac || !pa.dr.lu || !pa.dbg_uzz || !pa.dbg_uacc)
            return fail(c, HENS_ERR_HIP, "hens_debug_draws: out of device memory");
        pa.iter0 = (uint64_t)iter; pa.seed = c->cfg.seed; pa.a = c->cfg.a;
        pa.Tl = c->Tl; pa.W = c->W; pa.D = dim_active(c); pa.rung_begin = c->cfg.rung_begin; pa.idx_bits = c->idx_bits;
        pa.T = c->T; pa.cb = c->label_cb;
        if (c->nsplits > 2) {                // (positions then run through the sets one after the other: k_plan_sets)
            pa.nsets = c->nsplits; pa.cb = 0;
            pa.order = sc.grab<int32_t>(TW);
            if (!pa.order) return fail(c, HENS_ERR_HIP, "hens_debug_draws: out of device memory");
        }
        if (pa.cb) {
            pa.keys = sc.grab<uint32_t>((size_t)c->T * 8);
            if (!pa.keys) return fail(c, HENS_ERR_HIP, "hens_debug_draws: out of device memory");
        }
        launch_plan_kernels(c, c->stream, pa, 1);
        if (block > 0 && block < c->gibbs[0].nblocks) {      // the block's draws over the iteration's position lists; a block the stretch
                                                             // table lacks (an MH iteration's): `own` alone is read, the iteration's
            PlanBlockArgs pb{};
            pb.own = pa.dr.own; pb.dr = pa.dr; pb.dbg_uzz = pa.dbg_uzz; pb.dbg_uacc = pa.dbg_uacc;
            pb.iter = (uint64_t)iter; pb.seed = c->cfg.seed; pb.a = c->cfg.a;
            pb.Tl = c->Tl; pb.W = c->W; pb.nb = c->gibbs[0].n[(size_t)block]; pb.rung_begin = c->cfg.rung_begin; pb.block = (uint32_t)block;
            hipLaunchKernelGGL(k_plan_block, dim3((c->W + 255) / 256, c->Tl), dim3(256), 0, c->stream, pb);
        }
        HIPCHK(c, hipGetLastError());
        if (own) HIPCHK(c, hipMemcpyAsync(own, pa.dr.own, TW * 4, hipMemcpyDeviceToHost, c->stream));
        if (cw) HIPCHK(c, hipMemcpyAsync(cw, pa.dr.cw, TW * 4, hipMemcpyDeviceToHost, c->stream));
        if (u_zz) HIPCHK(c, hipMemcpyAsync(u_zz, pa.dbg_uzz, TW * 8, hipMemcpyDeviceToHost, c->stream));
        if (u_acc) HIPCHK(c, hipMemcpyAsync(u_acc, pa.dbg_uacc, TW * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if ((pt_slot || u_swap) && c->T > 1) {
        const size_t n = (size_t)c->T * c->W;
        int32_t* ds = sc.grab<int32_t>(n);
        double* du = sc.grab<double>(n);
        if (!ds || !du) return fail(c, HENS_ERR_HIP, "hens_debug_draws: out of device memory");
        if (const int r = export_pt_draws(c, ds, du, (uint64_t)iter, pt_slot, u_swap)) return r;
    }
    if ((mh_step || mh_u) && (c->mh_kind == MH_DIST || c->mh_kind == MH_MT_DIST)) {      // the drawn points q (multiple try: try 0) and the accept uniforms of that iteration
        double* dq = sc.grab<double>(TW * c->D);
        double* du = sc.grab<double>(TW);
        if (!dq || !du) return fail(c, HENS_ERR_HIP, "hens_debug_draws: out of device memory");
        hipLaunchKernelGGL(k_dist_draw, dim3(grid_for((int64_t)TW * c->D)), dim3(256), 0, c->stream, dq, du, c->dist_block.lo(), c->dist_block.hi(),
                           c->dist_block.terms(), c->cfg.seed, (uint64_t)iter, c->Tl, c->W, c->D, (int)c->cfg.rung_begin);
        HIPCHK(c, hipGetLastError());
        if (mh_step) HIPCHK(c, hipMemcpyAsync(mh_step, dq, TW * c->D * 8, hipMemcpyDeviceToHost, c->stream));
        if (mh_u) HIPCHK(c, hipMemcpyAsync(mh_u, du, TW * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    } else if ((mh_step || mh_u) && c->mh_kind >= 0) {
        MhDrawArgs d{};
        d.step = sc.grab<double>(TW * c->D); d.lu = sc.grab<double>(TW); d.dbg_u = sc.grab<double>(TW);
        if (!d.step || !d.lu || !d.dbg_u) return fail(c, HENS_ERR_HIP, "hens_debug_draws: out of device memory");
        d.scale = c->mh_scale; d.iter = (uint64_t)iter; d.seed = c->cfg.seed;
        d.Tl = c->Tl; d.W = c->W; d.D = c->D; d.rung_begin = c->cfg.rung_begin; d.kind = c->mh_kind;
        d.chol_lds = 0;
        d.block = (uint32_t)block;
        hipLaunchKernelGGL(k_mh_draw, dim3((c->W + 63) / 64, c->Tl), dim3(256), (size_t)64 * (c->D + 1) * 8, c->stream, d);
        HIPCHK(c, hipGetLastError());
        if (mh_step) HIPCHK(c, hipMemcpyAsync(mh_step, d.step, TW * c->D * 8, hipMemcpyDeviceToHost, c->stream));
        if (mh_u) HIPCHK(c, hipMemcpyAsync(mh_u, d.dbg_u, TW * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return HENS_OK;
}

// ---- reversible-jump leaf packing ----------------------------------------------------------
// The body of hens_rj_set_model and hens_rj_set_model_kinds: a model whose likelihood the device evaluates.  nkinds: the leaf kinds
// the entry point takes (ids below it); lo / hi: the branches' boxes one after the other, a branch's width that of its kind.
static int rj_set_template_model(hens_ctx_impl* c, int nkinds, int32_t nbranches, const int32_t* kinds, const int32_t* nleaves_max,
                                 const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp,
                                 int32_t ndata, const double* t, const double* y, double sigma) {
    if (!c || !kinds || !nleaves_max || !nleaves_min || !lo || !hi || !leaf_logp || !t || !y)
        return fail(c, HENS_ERR_INVALID, "null argument");
    if (!is_rj(c)) return fail(c, HENS_ERR_STATE, "hens_rj_set_model needs HENS_LIKE_TEMPLATE");
    if (nbranches < 1 || nbranches > RJ_MAX_BRANCH) return fail(c, HENS_ERR_INVALID, "1..%d branches", RJ_MAX_BRANCH);
    if (ndata < 1 || !(sigma > 0.0)) return fail(c, HENS_ERR_INVALID, "invalid data");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (const int rd = rjchain_drop(c)) return rd;
    RjModel M{};
    M.nb = nbranches; M.ndata = ndata; M.sigma = sigma;
    int off = 0, slot = 0, k = 0, boff[RJ_MAX_BRANCH] = {0, 0, 0, 0};      // (boff: a branch's first entry of lo / hi)
    bool wide = false;
    for (int b = 0; b < nbranches; ++b) {
        if (kinds[b] < 0 || kinds[b] >= nkinds) return fail(c, HENS_ERR_INVALID, "unknown leaf kind %d", kinds[b]);
        if (nleaves_max[b] < 1 || nleaves_max[b] > 32 || nleaves_min[b] < 0 || nleaves_min[b] > nleaves_max[b])
            return fail(c, HENS_ERR_INVALID, "branch %d: need 0 <= nleaves_min <= nleaves_max <= 32", b);
        const int nd = RJ_KIND_WIDTH[kinds[b]];
        wide = wide || kinds[b] > RJ_KIND_SINE;
        M.kind[b] = kinds[b]; M.nl[b] = nleaves_max[b]; M.nlmin[b] = nleaves_min[b]; M.off[b] = off;
        M.nd[b] = nd; M.slot0[b] = slot; M.ndmax = std::max(M.ndmax, nd);
        off += nleaves_max[b] * nd;
        slot += nleaves_max[b];
        boff[b] = k;
        for (int d = 0; d < nd; ++d, ++k) {
            M.lo[b][d] = lo[k]; M.hi[b][d] = hi[k];
            if (!(M.hi[b][d] > M.lo[b][d])) return fail(c, HENS_ERR_INVALID, "branch %d: empty prior box", b);
        }
        M.leaf_logp[b] = leaf_logp[b];
    }
    if (wide && slot > 64) return fail(c, HENS_ERR_UNSUPPORTED, "%d leaf slots: at most 64 over all branches", slot);
    if (wide && c->D > RJ_MAX_RW) return fail(c, HENS_ERR_INVALID, "record width ndim = %d: at most %d doubles", c->D, RJ_MAX_RW);
    if (!wide) {   // data points on a uniform grid (np.linspace): the sine leaves' rotation scheme of k_rj applies
        const double eps = 2.220446049250313e-16;
        const double dt = ndata > 1 ? (t[ndata - 1] - t[0]) / (double)(ndata - 1) : 0.0;
        double tmax = 0.0, dev = 0.0;
        for (int i = 0; i < ndata; ++i) { tmax = std::max(tmax, std::fabs(t[i])); dev = std::max(dev, std::fabs(t[i] - (t[0] + (double)i * dt))); }
        bool uniform = ndata > 64 && dt > 0.0 && dev <= 4.0 * eps * std::max(tmax, std::fabs(dt));
        // ... and the pulses' recurrence is exact enough on it: k_rj evaluates a lane's point i0 + k at t[i0] + k dt, not at t[i0 + k].
        // A distance d between the two moves a pulse by the relative |t - b| d / c^2 (up to 0.61 d / c of its amplitude), against
        // the float64 formula's own ~eps (3 + 3 (t - b)^2 / (2 c^2)).  Grids far from 0 (1000 + linspace(0, 1, N): d ~ ulp(1000) =
        // 6e4 eps h) made that thousands of times the formula's error; they take the per-point form.  The constant 128 is not
        // derived from an error bound: it is the power of two that keeps config 4's grid on the recurrence (linspace(-1, 1, 500):
        // d = 1.06 eps, 106 eps c against its narrowest pulse c = 0.01).  With the uniform-grid test alone,
        // tests/test_hip_template_accuracy.py (4 B bar) measured cases up to 885 eps c_min within 3.6 B, and the first case over
        // 4 B at 384 eps c_min (a 3-ulp jittered linspace).  The sines' rotation shares t_step64 and goes per point with
        // the pulses, although its phase error is the size of the float64 formula's own: a narrow pulse box on a fine grid
        // costs such a model the rotation as well (config 4 keeps both).
        if (uniform) {
            double d = 0.0, cmin = INFINITY;
            for (int i = 0; i < ndata; ++i) {            // d = |(t[i] - t[i0]) - k dt|, the difference and the product kept exact
                const double a = t[i], b = -t[i & ~7], s = a + b, bv = s - a, e1 = (a - (s - bv)) + (b - bv);
                const double kk = (double)(i & 7), p = kk * dt, e2 = std::fma(kk, dt, -p);
                d = std::max(d, std::fabs((s - p) + (e1 - e2)));
            }
            for (int b = 0; b < nbranches; ++b)
                if (kinds[b] == RJ_KIND_PULSE) {
                    const double clo = lo[boff[b] + 2], chi = hi[boff[b] + 2];
                    cmin = std::min(cmin, (clo <= 0.0 && chi >= 0.0) ? 0.0 : std::min(std::fabs(clo), std::fabs(chi)));
                }
            uniform = d <= 128.0 * eps * cmin;           // (no pulse branch: cmin = inf)
        }
        M.t_step64 = uniform ? 64.0 * dt : 0.0;
    }
    M.ind_off = off;
    M.RW = c->D;
    if (off + nbranches > c->D) return fail(c, HENS_ERR_INVALID, "record width ndim = %d cannot hold %d coordinates + %d masks", c->D, off, nbranches);
    if (wide && c->rj.have_chol) { c->rj.have_chol = c->rj.have_scale = false; memset(c->rj.chol, 0, sizeof(c->rj.chol)); }     // (full leaf covariances: pulse / sine models)
    c->rj.M = M;
    c->rj.general = false;
    c->rj.wide = wide;
    c->rj.mt_K = 0;
    c->rj.gb_n = 0; c->rj.gb_whole = false; c->rj.gb_sel = 0;      // (a table was laid out on the record that was: hens_rj_set_gibbs anew)
    rj_group_clear(c);                                             // (... and so was a friend table: hens_rj_set_group anew)
    c->rj.per_on = false; memset(c->rj.period, 0, sizeof(c->rj.period));        // (... and the periods: hens_rj_set_periodic anew)
    int r;
    if ((r = rj_push_ctab(c))) return r;
    if (!c->rj.t || c->rj.data_cap < ndata) {        // (a second model on the context may bring more data points than the first)
        if ((r = dalloc(c, &c->rj.t, (size_t)ndata))) return r;
        if ((r = dalloc(c, &c->rj.y, (size_t)ndata))) return r;
        c->rj.data_cap = ndata;
    }
    if (!c->rj.acc_bd) {
        if ((r = dalloc(c, &c->rj.acc_bd, (size_t)c->Tl * c->W))) return r;
        HIPCHK(c, hipMemsetAsync(c->rj.acc_bd, 0, (size_t)c->Tl * c->W * 4, c->stream));
    }
    // every pool row's template, resident (birth / death by difference in hens_rj_step): 2 Tl W rows of ndata doubles
    // (config 4: 131 MB); a lane keeps 8 points, so models of up to 512 data points; HENS_RJ_NO_TEMPLATES=1: A/B knob.  A model
    // past that has none: the buffer of a smaller model before it is let go of (rj_production reads rj.tm), not stepped on
    if (env().rj_no_templates || ndata > 512) {
        c->rj.tm = nullptr; c->rj.tm_ndata = 0;
    } else if (!c->rj.tm || c->rj.tm_ndata != ndata) {
        if ((r = dalloc(c, &c->rj.tm, (size_t)2 * c->Tl * c->W * (size_t)ndata))) return r;
        c->rj.tm_ndata = ndata;
    }
    c->rj.tm_valid = false;
    HIPCHK(c, hipMemcpyAsync(c->rj.t, t, (size_t)ndata * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.y, y, (size_t)ndata * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_like = c->have_prior = true;
    return HENS_OK;
}

int hens_rj_set_model(hens_ctx* ctx, int32_t nbranches, const int32_t* kinds, const int32_t* nleaves_max,
                      const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp,
                      int32_t ndata, const double* t, const double* y, double sigma) {
    return rj_set_template_model(enter(ctx), RJ_KIND_SINE + 1, nbranches, kinds, nleaves_max, nleaves_min, lo, hi, leaf_logp, ndata, t, y, sigma);
}

// ... with every leaf kind the device evaluates (RJ_KIND_*: one to four parameters per leaf).  A model of pulses and sines alone is
// hens_rj_set_model's, launch for launch; any other takes the WIDE instantiations of k_rj (no uniform-grid recurrences).
int hens_rj_set_model_kinds(hens_ctx* ctx, int32_t nbranches, const int32_t* kinds, const int32_t* nleaves_max,
                            const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp,
                            int32_t ndata, const double* t, const double* y, double sigma) {
    return rj_set_template_model(enter(ctx), RJ_NKINDS, nbranches, kinds, nleaves_max, nleaves_min, lo, hi, leaf_logp, ndata, t, y, sigma);
}

// A leaf-packing model WITHOUT a device likelihood: branches of 1 .. RJ_MAX_ND box-prior parameters per leaf (ensemble.py:325-329:
// `ndims` per branch), stepped with hens_rj_propose / hens_rj_accept around the caller's log-likelihood (ensemble.py:1306-1334,
// 1340-1545).  lo / hi: the branches' boxes one after the other (ndims[0] values, then ndims[1], ...); leaf_logp: the branches'
// constant leaf log-densities, accumulated by the caller in the reference's order (prior.py:364-383).
int hens_rj_set_model_general(hens_ctx* ctx, int32_t nbranches, const int32_t* ndims, const int32_t* nleaves_max,
                              const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !ndims || !nleaves_max || !nleaves_min || !lo || !hi || !leaf_logp) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!is_rj(c)) return fail(c, HENS_ERR_STATE, "hens_rj_set_model_general needs HENS_LIKE_TEMPLATE");
    if (nbranches < 1 || nbranches > RJ_MAX_BRANCH) return fail(c, HENS_ERR_INVALID, "1..%d branches", RJ_MAX_BRANCH);
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (const int rd = rjchain_drop(c)) return rd;
    RjModel M{};
    M.nb = nbranches; M.ndata = 0; M.sigma = 1.0; M.t_step64 = 0.0;
    int off = 0, slot = 0, k = 0;
    for (int b = 0; b < nbranches; ++b) {
        if (ndims[b] < 1 || ndims[b] > RJ_MAX_ND) return fail(c, HENS_ERR_UNSUPPORTED, "branch %d: 1..%d parameters per leaf", b, RJ_MAX_ND);
        if (nleaves_max[b] < 1 || nleaves_max[b] > 32 || nleaves_min[b] < 0 || nleaves_min[b] > nleaves_max[b])
            return fail(c, HENS_ERR_INVALID, "branch %d: need 0 <= nleaves_min <= nleaves_max <= 32", b);
        M.kind[b] = 0; M.nl[b] = nleaves_max[b]; M.nlmin[b] = nleaves_min[b]; M.off[b] = off;
        M.nd[b] = ndims[b]; M.slot0[b] = slot; M.ndmax = std::max(M.ndmax, ndims[b]);
        off += nleaves_max[b] * ndims[b];
        slot += nleaves_max[b];
        for (int d = 0; d < ndims[b]; ++d, ++k) {
            M.lo[b][d] = lo[k]; M.hi[b][d] = hi[k];
            if (!(M.hi[b][d] > M.lo[b][d])) return fail(c, HENS_ERR_INVALID, "branch %d: empty prior box", b);
        }
        M.leaf_logp[b] = leaf_logp[b];
    }
    if (slot > 64) return fail(c, HENS_ERR_UNSUPPORTED, "%d leaf slots: at most 64 over all branches", slot);
    M.ind_off = off;
    M.RW = c->D;
    if (off + nbranches > c->D || c->D > RJ_MAX_RW)
        return fail(c, HENS_ERR_INVALID, "record width ndim = %d cannot hold %d coordinates + %d masks (at most %d)", c->D, off, nbranches, RJ_MAX_RW);
    c->rj.M = M;
    c->rj.general = true;
    c->rj.wide = false;
    c->rj.mt_K = 0;
    c->rj.gb_n = 0; c->rj.gb_whole = false; c->rj.gb_sel = 0;
    rj_group_clear(c);
    c->rj.per_on = false; memset(c->rj.period, 0, sizeof(c->rj.period));
    int r;
    if ((r = rj_push_ctab(c))) return r;
    if (!c->rj.acc_bd) {
        if ((r = dalloc(c, &c->rj.acc_bd, (size_t)c->Tl * c->W))) return r;
        HIPCHK(c, hipMemsetAsync(c->rj.acc_bd, 0, (size_t)c->Tl * c->W * 4, c->stream));
    }
    c->rj.tm_valid = false;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->have_like = c->have_prior = true;
    return HENS_OK;
}

int hens_rj_set_mh_scale(hens_ctx* ctx, const double* scale) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !scale) return fail(c, HENS_ERR_INVALID, "null argument");
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.general) return fail(c, HENS_ERR_STATE, "the Philox in-model move belongs to hens_rj_step: template models only");
    for (int b = 0; b < c->rj.M.nb; ++b)          // [nbranches][the widest branch's parameters]: 3 on a pulse / sine model
        for (int d = 0; d < c->rj.M.nd[b]; ++d) c->rj.M.mh_scale[b][d] = scale[b * c->rj.M.ndmax + d];
    c->rj.have_scale = true; c->rj.have_chol = false;
    SETTLE(c, NEED_DEVICE);
    return rj_push_ctab(c);
}

// Full leaf covariances for the Philox in-model Gaussian move: chol[nbranches][3][3], the lower-triangular Cholesky factor of a
// leaf's proposal covariance (gaussian.py:265-268 draws multivariate_normal(0, cov)); step = L z with the unit normals z the
// diagonal path draws for the leaf's coordinates (same Philox keys)
int hens_rj_set_mh_chol(hens_ctx* ctx, const double* chol) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !chol) return fail(c, HENS_ERR_INVALID, "null argument");
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.general) return fail(c, HENS_ERR_STATE, "the Philox in-model move belongs to hens_rj_step: template models only");
    if (c->rj.wide) return fail(c, HENS_ERR_UNSUPPORTED, "full leaf covariances: models of pulses and sines only (diagonal steps: hens_rj_set_mh_scale)");
    if (c->rj.M.prior_on) return fail(c, HENS_ERR_UNSUPPORTED, "full leaf covariances: not together with prior terms (hens_rj_set_prior_terms; diagonal steps: hens_rj_set_mh_scale)");
    for (int b = 0; b < c->rj.M.nb; ++b)
        for (int d = 0; d < RJ_ND; ++d)
            for (int j = 0; j < RJ_ND; ++j) {
                const double v = chol[(b * RJ_ND + d) * RJ_ND + j];
                if (!(std::fabs(v) < INFINITY)) return fail(c, HENS_ERR_INVALID, "hens_rj_set_mh_chol: non-finite entry");
                if (j > d && v != 0.0) return fail(c, HENS_ERR_INVALID, "hens_rj_set_mh_chol: the factor must be lower triangular");
                if (j == d && !(v > 0.0)) return fail(c, HENS_ERR_INVALID, "hens_rj_set_mh_chol: the covariance is not positive definite (diagonal of its factor <= 0)");
            }
    for (int b = 0; b < c->rj.M.nb; ++b)
        for (int d = 0; d < RJ_ND; ++d) {
            for (int j = 0; j < RJ_ND; ++j) c->rj.chol[b][d][j] = chol[(b * RJ_ND + d) * RJ_ND + j];
            c->rj.M.mh_scale[b][d] = c->rj.chol[b][d][d];
        }
    c->rj.have_scale = c->rj.have_chol = true;
    SETTLE(c, NEED_DEVICE);
    return rj_push_ctab(c);
}

// Per-parameter prior terms on the leaves of the model in place (any of the three hens_rj_set_model* calls): kind / lo / hi / c0 / c1 /
// c2 run over the branches' leaf parameters one after the other (sum_b ndims[b] entries, as hens_rj_set_model_general takes lo / hi),
// a term's meaning and constants are hens_set_prior_terms's.  The terms replace the model's box: the log-prior of a slot, the Hastings
// factor -+ log q(leaf) of a birth / death and the distribution a leaf is born from (distgenrj.py:188-214) are all this prior.  An
// all-uniform specification IS a box: it goes into M.lo / hi / leaf_logp and the context keeps the box's kernels.
int hens_rj_set_prior_terms(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0, const double* c1,
                            const double* c2) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !kind || !lo || !hi || !c0 || !c1 || !c2) return fail(c, HENS_ERR_INVALID, "null argument");
    if (const int rk = need_rj_context(c)) return rk;
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_accept must follow hens_rj_propose");
    RjModel M = c->rj.M;
    PriorTerm terms[RJ_MAX_BRANCH][RJ_MAX_ND] = {};
    bool box = true;
    int k = 0, slots = 0;
    for (int b = 0; b < M.nb; ++b) {
        slots += M.nl[b];
        for (int d = 0; d < M.nd[b]; ++d, ++k) {       // (no pads in a record: a uniform term has finite bounds)
            const ParsedTerm p = parse_term(kind[k], lo[k], hi[k], c0[k], c1[k], c2[k], /*admit_pad=*/false);
            if (p.why[0]) return fail(c, HENS_ERR_INVALID, "%s (branch %d, parameter %d)", p.why, b, d);
            terms[b][d] = p.term;
            M.lo[b][d] = lo[k]; M.hi[b][d] = hi[k];
        }
        const PriorBox pb = fold_box(terms[b], M.nd[b]);
        M.leaf_logp[b] = pb.logp;
        box = box && pb.box;
    }
    if (!box) {
        if (c->rj.have_chol) return fail(c, HENS_ERR_UNSUPPORTED, "prior terms: not together with full leaf covariances (hens_rj_set_mh_chol; diagonal steps: hens_rj_set_mh_scale)");
        // (the instantiations that carry the terms index a record's slots and coordinates at run time: their limits)
        if (slots > 64) return fail(c, HENS_ERR_UNSUPPORTED, "prior terms: %d leaf slots, at most 64 over all branches", slots);
        if (c->D > RJ_MAX_RW) return fail(c, HENS_ERR_UNSUPPORTED, "prior terms: record width ndim = %d, at most %d doubles", c->D, RJ_MAX_RW);
    }
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (const int rd = rjchain_drop(c)) return rd;
    M.prior_on = box ? 0 : 1;
    if (M.prior_on) M.t_step64 = 0.0;          // (no uniform-grid form under terms: per-point leaf values)
    // (a box of its own: the uniform-grid recurrences were admitted for the model's narrowest pulse, rj_set_template_model - a box
    //  that lets |c| go below it takes the per-point form, which is right on every grid)
    for (int b = 0; b < M.nb && M.t_step64 != 0.0; ++b)
        if (M.kind[b] == RJ_KIND_PULSE) {
            auto cmin = [](double l, double h) { return (l <= 0.0 && h >= 0.0) ? 0.0 : std::min(std::fabs(l), std::fabs(h)); };
            if (cmin(M.lo[b][2], M.hi[b][2]) < cmin(c->rj.M.lo[b][2], c->rj.M.hi[b][2])) M.t_step64 = 0.0;
        }
    const RjModel before = c->rj.M;
    c->rj.M = M;
    memcpy(c->rj.terms, terms, sizeof(terms));
    if (const int r = rj_push_ctab(c)) { c->rj.M = before; return r; }
    c->rj.tm_valid = false;
    c->rj.mt_K = 0;                            // (a multiple-try proposal was set against the prior that was: hens_rj_set_mt_proposal anew)
    return HENS_OK;
}

// Periodic leaf parameters (include/hipensemble.h): period[nbranches][ndmax] in the birth arrays' stride, 0 = not periodic; NULL or all
// zeros clears.  The periods live in the context beside the model and are folded into RjArgs::ctab's period row by rj_push_ctab, which
// every setter that rebuilds the table goes through - so they survive hens_rj_set_mh_scale / _chol / _prior_terms / _gibbs / _group in
// any order, and a new model (hens_rj_set_model*) drops them.
int hens_rj_set_periodic(hens_ctx* ctx, const double* period) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!is_rj(c)) return fail(c, HENS_ERR_UNSUPPORTED, "hens_rj_set_periodic needs a leaf-packing context (HENS_LIKE_TEMPLATE); hens_set_periodic serves the others");
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_accept must follow hens_rj_propose");       // (first: a proposed half-step is both)
    if (c->expect_split != 0 || c->propose_pending) return fail(c, HENS_ERR_STATE, "hens_rj_set_periodic between the half-steps of a move");
    const RjModel& M = c->rj.M;
    double per[RJ_MAX_BRANCH][RJ_MAX_ND] = {};
    bool any = false;
    if (period)
        for (int b = 0; b < M.nb; ++b)
            for (int d = 0; d < M.ndmax; ++d) {
                const double v = period[b * M.ndmax + d];
                if (!(v >= 0.0) || !(v < INFINITY)) return fail(c, HENS_ERR_INVALID, "hens_rj_set_periodic: period of branch %d, parameter %d must be finite and >= 0", b, d);
                if (v > 0.0 && d >= M.nd[b])
                    return fail(c, HENS_ERR_INVALID, "hens_rj_set_periodic: branch %d has %d leaf parameters, a period was given for parameter %d", b, M.nd[b], d);
                per[b][d] = v;
                any = any || v > 0.0;
            }
    SETTLE(c, NEED_DEVICE);
    double before[RJ_MAX_BRANCH][RJ_MAX_ND];
    const bool on_before = c->rj.per_on;
    memcpy(before, c->rj.period, sizeof(before));
    memcpy(c->rj.period, per, sizeof(per));
    c->rj.per_on = any;
    if (const int r = rj_push_ctab(c)) { memcpy(c->rj.period, before, sizeof(before)); c->rj.per_on = on_before; return r; }
    return HENS_OK;
}

// ---- teacher-forced moves on leaf-packing records: the caller's draws (hens_rj_draws), the device's arithmetic ------------------
// By HENS_RJ_MOVE_*: the in-model Gaussian move on every active leaf (mh.py:56-193); birth / death on one branch (rj.py:145-388) or,
// "together", ONE proposal over every branch ([nbranches][...] arrays, one u_acc); one half of the red / blue StretchMove (round 5;
// red_blue.py:103-197, 254-323 + stretch.py:160-231's loop over the branches).  A move's own argument checks,
// staging and counter rule come first; rj_forced_move is the body they share.
static int rj_forced_check(hens_ctx_impl* c, int move, const hens_rj_draws& d) {
    if (move == HENS_RJ_MOVE_MH) return !d.step || !d.u_acc ? fail(c, HENS_ERR_INVALID, "null argument") : counter_room(c, 1);
    if (move == HENS_RJ_MOVE_STRETCH) {
        if (!d.labels || !d.rint || !d.u_zz || !d.u_acc) return fail(c, HENS_ERR_INVALID, "null argument");
        if (d.split < 0 || d.split > 1) return fail(c, HENS_ERR_INVALID, "split must be 0 or 1 (two sets)");
        if (d.split != c->expect_split) return fail(c, HENS_ERR_STATE, "split calls must run 0, 1 in order (expected %d)", c->expect_split);
        if (const int r = counter_room(c, 1)) return r;
        if (!c->cfg.live_dangerously && c->W < 2 * c->rj.M.ind_off)                 // red_blue.py:103-114 (every slot of every branch counts)
            return fail(c, HENS_ERR_TOO_FEW_WALKERS, "It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions. "
                                                     "If you would like to do this, please set live_dangerously to True.");
        return HENS_OK;
    }
    if (!d.change || !d.leaf || !d.birth || !d.u_acc) return fail(c, HENS_ERR_INVALID, "null argument");
    const bool all = move == HENS_RJ_MOVE_BD_ALL;
    if (!all && (d.branch < 0 || d.branch >= c->rj.M.nb)) return fail(c, HENS_ERR_INVALID, "branch %d out of range", d.branch);
    const size_t TW = (size_t)c->Tl * c->W;
    for (int k = 0; k < (all ? c->rj.M.nb : 1); ++k)       // (k: the branch's place in the arrays)
        for (size_t i = k * TW; i < (k + 1) * TW; ++i) {
            if (d.change[i] < -1 || d.change[i] > 1) return fail(c, HENS_ERR_INVALID, "change must be -1, 0 or +1");
            if (d.change[i] != 0 && (d.leaf[i] < 0 || d.leaf[i] >= c->rj.M.nl[all ? k : d.branch])) return fail(c, HENS_ERR_INVALID, "leaf slot out of range");
        }
    return HENS_OK;
}

static int rj_stretch_stage(hens_ctx_impl* c, const hens_rj_draws& d, RjLaunch& l) {
    const int Tl = c->Tl, W = c->W, nb = c->rj.M.nb, split = d.split;
    // ascending walker lists of the two sets (red_blue.py:150-154): set k has ceil((W - k) / 2) walkers (arange(W) % 2, shuffled)
    const int n0 = (W + 1) / 2, Ns = split == 0 ? n0 : W - n0, Nc = W - Ns;
    std::vector<int32_t> own((size_t)Tl * Ns), other((size_t)Tl * Nc), cw((size_t)nb * Tl * Ns);
    for (int t = 0; t < Tl; ++t) {
        int a = 0, b = 0;
        for (int w = 0; w < W; ++w) {
            const uint8_t lb = d.labels[(size_t)t * W + w];
            if (lb > 1) return fail(c, HENS_ERR_INVALID, "labels must be 0 or 1");
            if (lb == split) { if (a >= Ns) return fail(c, HENS_ERR_INVALID, "labels must hold ceil((W - k) / 2) walkers of set k per rung"); own[(size_t)t * Ns + a++] = w; }
            else { if (b >= Nc) return fail(c, HENS_ERR_INVALID, "labels must hold ceil((W - k) / 2) walkers of set k per rung"); other[(size_t)t * Nc + b++] = w; }
        }
    }
    if (split == 0) c->labels_host.assign(d.labels, d.labels + (size_t)Tl * W);
    else if (c->labels_host.size() != (size_t)Tl * W || memcmp(c->labels_host.data(), d.labels, (size_t)Tl * W) != 0)
        return fail(c, HENS_ERR_INVALID, "labels differ between split 0 and split 1 of the same iteration");
    for (int b = 0; b < nb; ++b)                                                    // rint[nbranches][Tl][Ns]: an index into the other set
        for (int t = 0; t < Tl; ++t)
            for (int k = 0; k < Ns; ++k) {
                const int64_t ri = d.rint[((size_t)b * Tl + t) * Ns + k];
                if (ri < 0 || ri >= Nc) return fail(c, HENS_ERR_INVALID, "rint out of range [0, %d)", Nc);
                cw[((size_t)b * Tl + t) * Ns + k] = other[(size_t)t * Nc + ri];
            }
    const size_t n = (size_t)Tl * Ns;
    HIPCHK(c, hipMemcpyAsync(c->rj.st_own, own.data(), n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.st_cw, cw.data(), (size_t)nb * n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.uzz, d.u_zz, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.u, d.u_acc, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));                                     // (the host vectors go out of scope)
    l.ns = Ns;
    return HENS_OK;
}
// draws -> staging buffers; the launch's branch / half
static int rj_forced_stage(hens_ctx_impl* c, int move, const hens_rj_draws& d, RjLaunch& l) {
    if (move == HENS_RJ_MOVE_STRETCH) return rj_stretch_stage(c, d, l);
    const size_t TW = (size_t)c->Tl * c->W, NB = move == HENS_RJ_MOVE_BD_ALL ? (size_t)c->rj.M.nb : 1;
    if (move == HENS_RJ_MOVE_MH) HIPCHK(c, hipMemcpyAsync(c->rj.step, d.step, TW * c->rj.M.ind_off * 8, hipMemcpyHostToDevice, c->stream));
    else {
        l.branch = move == HENS_RJ_MOVE_BD_ALL ? -1 : d.branch;
        HIPCHK(c, hipMemcpyAsync(c->rj.change, d.change, NB * TW, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->rj.leaf, d.leaf, NB * TW * 4, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->rj.birth, d.birth, NB * TW * (size_t)c->rj.M.ndmax * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->rj.u, d.u_acc, TW * 8, hipMemcpyHostToDevice, c->stream));
    return HENS_OK;
}
// the counters behind a move that ran
static void rj_forced_count(hens_ctx_impl* c, int move, const hens_rj_draws& d) {
    if (move == HENS_RJ_MOVE_STRETCH) c->expect_split = d.split ^ 1;
    if (move == HENS_RJ_MOVE_MH || (move == HENS_RJ_MOVE_STRETCH && d.split == 1)) {       // (ONE move; the in-model move's counter, whichever move it is)
        c->rj.num_mh += 1;
        if (!has_pt(c)) c->iter += 1;
    }
    // ("iterate_branches": one MOVE per walk through the branches)
    if (move == HENS_RJ_MOVE_BD_ALL || (move == HENS_RJ_MOVE_BD && !(c->rj.schedule == 1 && d.branch != c->rj.M.nb - 1))) c->rj.num_bd += 1;
}

// One teacher-forced move, whole (keep_out by walker; a stretch half: by position of the moving set) - or, `propose`, its proposal
// half up to the log-prior (hens_rj_propose).  Either way the move's counters and the order of the stretch halves advance here.
static int rj_forced_move(hens_ctx_impl* c, int move, const hens_rj_draws& d, uint8_t* keep_out, bool propose) {
    static const int mode_of[] = {RJ_MODE_MH, RJ_MODE_BD, RJ_MODE_BD, RJ_MODE_STRETCH};       // by HENS_RJ_MOVE_*
    int r = rj_ready(c, move == HENS_RJ_MOVE_STRETCH && d.split == 1, propose);
    if (r) return r;
    if ((r = rj_forced_check(c, move, d))) return r;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    if ((r = rj_ensure_staging(c))) return r;
    RjLaunch l = rj_forced(c, mode_of[move], propose);
    if ((r = rj_forced_stage(c, move, d, l))) return r;
    // the move of the selected block (hens_rj_gibbs_select; hens_rj_propose has refused the in-model move under a table)
    if (move == HENS_RJ_MOVE_MH && c->rj.gb_n > 0 && !c->rj.gb_whole) { l.gibbs = true; l.gb0 = c->rj.gb_sel; l.gb1 = c->rj.gb_sel + 1; }
    c->rj.tm_valid = false;                   // (teacher-forced move: the reference's full evaluation, no resident templates)
    if ((r = rj_launch(c, l))) return r;
    if (propose) c->rj.pending_acc = rj_accept_counter(c, l.mode, l.branch);
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->rj.keep, (size_t)c->Tl * (l.mode == RJ_MODE_STRETCH ? l.ns : c->W), hipMemcpyDeviceToHost, c->stream));
    if ((r = check_flags(c, false))) return r;
    rj_forced_count(c, move, d);
    return HENS_OK;
}

int hens_rj_mh_step(hens_ctx* ctx, const double* step, const double* u_acc, uint8_t* keep_out) {
    hens_rj_draws d{}; d.step = step; d.u_acc = u_acc;
    return rj_forced_move(enter(ctx), HENS_RJ_MOVE_MH, d, keep_out, false);
}

int hens_rj_stretch_split(hens_ctx* ctx, int32_t split, const uint8_t* labels, const int64_t* rint, const double* u_zz,
                          const double* u_acc, uint8_t* keep_out) {
    hens_rj_draws d{}; d.split = split; d.labels = labels; d.rint = rint; d.u_zz = u_zz; d.u_acc = u_acc;
    return rj_forced_move(enter(ctx), HENS_RJ_MOVE_STRETCH, d, keep_out, false);
}

int hens_rj_bd_step(hens_ctx* ctx, int32_t branch, const int8_t* change, const int32_t* leaf, const double* birth,
                    const double* u_acc, uint8_t* keep_out) {
    hens_rj_draws d{}; d.branch = branch; d.change = change; d.leaf = leaf; d.birth = birth; d.u_acc = u_acc;
    return rj_forced_move(enter(ctx), HENS_RJ_MOVE_BD, d, keep_out, false);
}

int hens_rj_bd_all_step(hens_ctx* ctx, const int8_t* change, const int32_t* leaf, const double* birth, const double* u_acc,
                        uint8_t* keep_out) {
    hens_rj_draws d{}; d.change = change; d.leaf = leaf; d.birth = birth; d.u_acc = u_acc;
    return rj_forced_move(enter(ctx), HENS_RJ_MOVE_BD_ALL, d, keep_out, false);
}

// ---- MTDistGenMoveRJ (mtdistgenrj.py over multipletry.py:238-514, 597-776): the multiple-try birth / death move, k_rj_mt --------
static int rj_branch_of(const hens_ctx_impl* c, uint64_t it);      // (below, with hens_rj_step)
// One leaf parameter's density as the kernel reads it (hens_rj_mt.h: RJ_MT_DENS doubles)
static void rj_mt_row(double* r, double lo, double hi, const PriorTerm& t) {
    r[0] = lo; r[1] = hi; r[2] = t.c0; r[3] = t.c1; r[4] = t.c2; r[5] = (double)t.kind;
}
int hens_rj_set_mt_proposal(hens_ctx* ctx, int32_t num_try, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                            const double* c1, const double* c2) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rk = need_rj_context(c)) return rk;
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_accept must follow hens_rj_propose");
    if (num_try < 0 || num_try > RJ_MT_MAX_TRY) return fail(c, HENS_ERR_INVALID, "num_try must be in [0, %d] (one lane per try; 0: the plain birth / death move)", RJ_MT_MAX_TRY);
    if (num_try == 0) { c->rj.mt_K = 0; return HENS_OK; }
    if (c->rj.general)
        return fail(c, HENS_ERR_STATE, "this context's model has no device likelihood (hens_rj_set_model_general): the multiple-try move evaluates its tries on the device");
    if (kind && (!lo || !hi || !c0 || !c1 || !c2)) return fail(c, HENS_ERR_INVALID, "null argument");
    const RjModel& M = c->rj.M;
    int slots = 0;
    for (int b = 0; b < M.nb; ++b) {
        slots += M.nl[b];
        if (M.nlmin[b] == M.nl[b])               // multipletry.py:661-664
            return fail(c, HENS_ERR_INVALID, "MT RJ proposal requires that nleaves_min != nleaves_max. (branch %d)", b);
    }
    if (slots > 64) return fail(c, HENS_ERR_UNSUPPORTED, "multiple-try proposal: %d leaf slots, at most 64 over all branches", slots);
    if (c->D > RJ_MAX_RW) return fail(c, HENS_ERR_UNSUPPORTED, "multiple-try proposal: record width ndim = %d, at most %d doubles", c->D, RJ_MAX_RW);
    std::vector<double> dens((size_t)RJ_MAX_BRANCH * 2 * RJ_MAX_ND * RJ_MT_DENS, 0.0);
    bool gbox[RJ_MAX_BRANCH] = {};
    double glogq[RJ_MAX_BRANCH] = {};
    int k = 0;
    for (int b = 0; b < M.nb; ++b) {
        double* gen = dens.data() + (size_t)(2 * b) * RJ_MAX_ND * RJ_MT_DENS;
        double* pri = gen + RJ_MAX_ND * RJ_MT_DENS;
        PriorTerm gt[RJ_MAX_ND] = {};
        for (int d = 0; d < M.nd[b]; ++d, ++k) {
            // the prior of the branch's leaf: its terms, or (a box model) the box with the branch's constant, RjModel::leaf_logp
            PriorTerm pt_{};
            if (M.prior_on) pt_ = c->rj.terms[b][d];
            rj_mt_row(pri + d * RJ_MT_DENS, M.lo[b][d], M.hi[b][d], pt_);
            if (!kind) {                             // the generator is the prior
                rj_mt_row(gen + d * RJ_MT_DENS, M.lo[b][d], M.hi[b][d], pt_);
                continue;
            }
            const ParsedTerm p = parse_term(kind[k], lo[k], hi[k], c0[k], c1[k], c2[k], /*admit_pad=*/false);
            if (p.why[0]) return fail(c, HENS_ERR_INVALID, "%s (generator: branch %d, parameter %d)", p.why, b, d);
            gt[d] = p.term;
            rj_mt_row(gen + d * RJ_MT_DENS, lo[k], hi[k], p.term);
        }
        if (!kind) { gbox[b] = !M.prior_on; glogq[b] = M.leaf_logp[b]; }
        else { const PriorBox pb = fold_box(gt, M.nd[b]); gbox[b] = pb.box; glogq[b] = pb.logp; }
    }
    SETTLE(c, NEED_DEVICE);
    if (!c->rj.mt_dens)
        if (const int r = dalloc(c, &c->rj.mt_dens, dens.size())) return r;
    HIPCHK(c, hipMemcpyAsync(c->rj.mt_dens, dens.data(), dens.size() * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the vector goes out of scope)
    memcpy(c->rj.mt_gen_box, gbox, sizeof(gbox));
    memcpy(c->rj.mt_gen_logq, glogq, sizeof(glogq));
    c->rj.mt_K = num_try;
    return HENS_OK;
}

int hens_rj_mt_bd_step(hens_ctx* ctx, int32_t branch, const int8_t* change, const int32_t* leaf, const double* tries, const double* u_pick,
                       const double* u_acc, uint8_t* keep_out, const hens_rj_mt_out* out) {
    hens_ctx_impl* c = enter(ctx);
    int r = rj_ready(c);
    if (r) return r;
    if (!change || !leaf || !tries || !u_pick || !u_acc) return fail(c, HENS_ERR_INVALID, "null argument");
    if (c->rj.mt_K < 1) return fail(c, HENS_ERR_STATE, "no multiple-try proposal set (hens_rj_set_mt_proposal)");
    if (branch < 0 || branch >= c->rj.M.nb) return fail(c, HENS_ERR_INVALID, "branch %d out of range", branch);
    const size_t TW = (size_t)c->Tl * c->W, K = (size_t)c->rj.mt_K, NT = TW * K * (size_t)c->rj.M.ndmax;
    for (size_t i = 0; i < TW; ++i) {
        if (change[i] != -1 && change[i] != 1) return fail(c, HENS_ERR_INVALID, "change must be -1 or +1 (MT RJ is only implemented for +1/-1 moves)");
        if (leaf[i] < 0 || leaf[i] >= c->rj.M.nl[branch]) return fail(c, HENS_ERR_INVALID, "leaf slot out of range");
    }
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    if ((r = rj_ensure_staging(c))) return r;
    // (each once; the tries for the most tries and the widest leaf a proposal can have: a later proposal of more tries finds room)
    if (!c->rj.mt_tries && (r = dalloc(c, &c->rj.mt_tries, TW * RJ_MT_MAX_TRY * RJ_MAX_ND))) return r;
    if (!c->rj.mt_upick && (r = dalloc(c, &c->rj.mt_upick, TW))) return r;
    if (!c->rj.mt_out && (r = dalloc(c, &c->rj.mt_out, (size_t)RJ_MT_NOUT * TW))) return r;
    HIPCHK(c, hipMemcpyAsync(c->rj.change, change, TW, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.leaf, leaf, TW * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.mt_tries, tries, NT * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.mt_upick, u_pick, TW * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(c->rj.u, u_acc, TW * 8, hipMemcpyHostToDevice, c->stream));
    RjLaunch l = rj_forced(c, RJ_MODE_BD, false);
    l.branch = branch; l.birth = nullptr;
    l.mt = true; l.tries = c->rj.mt_tries; l.u_pick = c->rj.mt_upick; l.mt_out = c->rj.mt_out;
    c->rj.tm_valid = false;                   // (teacher-forced move: the reference's full evaluation, no resident templates)
    if ((r = rj_launch(c, l))) return r;
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->rj.keep, TW, hipMemcpyDeviceToHost, c->stream));
    std::vector<double> pk;
    if (out) {
        double* const dst[RJ_MT_NOUT] = {nullptr, out->lsw, out->aux_lsw, out->factors, out->mt_ll, out->mt_lp};
        for (int f = 1; f < RJ_MT_NOUT; ++f)
            if (dst[f]) HIPCHK(c, hipMemcpyAsync(dst[f], c->rj.mt_out + (size_t)f * TW, TW * 8, hipMemcpyDeviceToHost, c->stream));
        if (out->pick) {
            pk.resize(TW);
            HIPCHK(c, hipMemcpyAsync(pk.data(), c->rj.mt_out, TW * 8, hipMemcpyDeviceToHost, c->stream));
        }
    }
    if ((r = check_flags(c, false))) return r;            // (waits for the stream)
    for (size_t i = 0; i < pk.size(); ++i) out->pick[i] = (int32_t)pk[i];
    if (!(c->rj.schedule == 1 && branch != c->rj.M.nb - 1)) c->rj.num_bd += 1;      // ("iterate_branches": one MOVE per walk through the branches)
    return HENS_OK;
}

int hens_rj_mt_debug_draws(hens_ctx* ctx, int64_t iter, double* tries, double* u_pick) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.mt_K < 1) return fail(c, HENS_ERR_STATE, "no multiple-try proposal set (hens_rj_set_mt_proposal)");
    if (!tries || !u_pick) return fail(c, HENS_ERR_INVALID, "null output");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W, per = TW * (size_t)c->rj.mt_K * (size_t)c->rj.M.ndmax;
    DeviceScratch sc;
    RjMtDebugArgs a{};
    a.tries = sc.grab<double>(per); a.u_pick = sc.grab<double>(TW);
    if (!a.tries || !a.u_pick) return fail(c, HENS_ERR_HIP, "hens_rj_mt_debug_draws: out of device memory");
    a.iter = (uint64_t)iter; a.seed = c->cfg.seed;
    a.Tl = c->Tl; a.W = c->W; a.rung_begin = c->cfg.rung_begin; a.K = c->rj.mt_K; a.ndmax = c->rj.M.ndmax;
    // "separate_branches": the chosen branch's draws in entry 0; "iterate_branches": every branch's, in order (hens_rj_debug_draws)
    const bool every = c->rj.schedule == 1 || c->rj.schedule == 2;
    const int nsub = every ? c->rj.M.nb : 1;
    for (int k = 0; k < nsub; ++k) {
        a.branch = every ? k : rj_branch_of(c, (uint64_t)iter);
        a.nd = c->rj.M.nd[a.branch];
        a.gen = c->rj.mt_dens + (size_t)(2 * a.branch) * RJ_MAX_ND * RJ_MT_DENS;
        hipLaunchKernelGGL(k_rj_mt_debug_draws, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(tries + (size_t)k * per, a.tries, per * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(u_pick + (size_t)k * TW, a.u_pick, TW * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    return HENS_OK;
}

// branch of iteration `it`'s birth / death move (ensemble.py:988-990, "separate_branches"): one counter-based uniform
static int rj_branch_of(const hens_ctx_impl* c, uint64_t it) {
    return std::min(c->rj.M.nb - 1, (int)(move_uniform(c->cfg.seed ^ 0x9E3779B97F4A7C15ull, it) * c->rj.M.nb));
}

// The birth / death move of hens_rj_step's iteration.  "together" (ensemble.py:414-432): ONE proposal changes a leaf in every branch of
// the walker, one accept test; "iterate_branches" (ensemble.py:434-451, rj.py:169-388): ONE move walks through every branch - birth /
// death, accept, update per branch -, its accept mask is the last branch's; else one branch's move (ensemble.py:988-990).
static int rj_step_bd(hens_ctx_impl* c) {
    if (c->rj.schedule == 2) return rj_launch(c, rj_production(c, RJ_MODE_BD, -1));
    // (under hens_rj_set_mt_proposal the launch is k_rj_mt: same place, same template scheme, same accept counter)
    auto one = [c](int b) { RjLaunch l = rj_production(c, RJ_MODE_BD, b); l.mt = c->rj.mt_K > 0; return rj_launch(c, l); };
    if (c->rj.schedule != 1) return one(rj_branch_of(c, c->iter));
    for (int b = 0, r; b < c->rj.M.nb; ++b)
        if ((r = one(b))) return r;
    return HENS_OK;
}

// What hens_rj_step and hens_rj_step_chain share: the head of a call (checks, the state by field, the first full evaluation), one
// iteration, and the way out.
namespace {
struct RjStepping {
    hens_ctx_impl* c;
    bool stretch = false, group = false, fresh = false, armed = false;
    explicit RjStepping(hens_ctx_impl* c_) : c(c_) {}
    void finish() { if (armed) { c->rj.defer_adapt = false; flush_adapt(c); armed = false; } }   // the switch off, no adaptation pending ...
    ~RjStepping() { finish(); }                                                                  // ... on every way out
    int begin(int64_t n_iters);
    int iteration(double* swaps_aside);
};

int RjStepping::begin(int64_t n_iters) {
    int r;
    stretch = c->rj.in_model == HENS_RJ_INMODEL_STRETCH;
    group = c->rj.in_model == HENS_RJ_INMODEL_GROUP;
    if (c->rj.mt_K > 0 && c->rj.schedule == 2)        // multipletry.py:635-636
        return fail(c, HENS_ERR_UNSUPPORTED, "Can only propose change to one model at a time with MT. (rj schedule \"together\" under hens_rj_set_mt_proposal)");
    if (!stretch && !group && !c->rj.have_scale) return fail(c, HENS_ERR_STATE, "in-model step scale not set (hens_rj_set_mh_scale)");
    if (stretch && c->rj.gb_n > 0) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records step the Gaussian in-model move");
    if (stretch && !c->cfg.live_dangerously && c->W < 2 * c->rj.M.ind_off)           // red_blue.py:103-114 (every slot of every branch counts)
        return fail(c, HENS_ERR_TOO_FEW_WALKERS, "It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions. "
                                                 "If you would like to do this, please set live_dangerously to True.");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    HIPCHK(c, hipEventRecord(c->ev0, c->stream));
    c->step_events = true;
    c->timing = hens_timing{};
    // resident templates (RjArgs::tm): kept true by every accepting launch, and re-evaluated from scratch - templates AND log-
    // likelihoods - whenever the state has crossed the C ABI since the last call (upload, parity-API move, DOWNLOAD) and every
    // RJ_REFRESH iterations (by the iteration counter), so that the rounding of a chain of +- leaf updates cannot pile up beyond 64
    // iterations.  Round 5: the evaluation after an upload used to rebuild the templates only, and a download did not count; a
    // chain resumed from a stored State (exact templates) then parted from the uninterrupted one (templates with up to 63
    // iterations of +- updates behind them) in the last bits of its birth / death likelihoods.  Now the resident state behind a
    // download is a function of what the download returned, so a chain is a function of (State, seed, iteration counter,
    // adaptation time): resumed in a new context it is the uninterrupted chain bit for bit (tests/test_hip_rj.py).
    if (c->rj.tm && !c->rj.tm_valid && n_iters > 0) {
        if ((r = rj_evaluate(c, c->have_logs))) return r;
        fresh = true;
    }
    const bool fold_off = env().no_fold;          // A/B knob: k_adapt behind every cascade
    if (!c->rj.ad_flag && !fold_off) {
        if ((r = dalloc(c, &c->rj.ad_flag, 2))) return r;
        HIPCHK(c, hipMemsetAsync(c->rj.ad_flag, 0, 8, c->stream));
    }
    armed = true;
    c->rj.defer_adapt = !fold_off && c->rj.tm != nullptr;
    return HENS_OK;
}

// One iteration.  swaps_aside (hens_rj_step_chain, the last iteration of a stored step): the in-model cascade's swap counts, copied
// there before the birth / death move's cascade overwrites swaps_last - its adaptation settled as a launch of its own in front of
// the copy instead of inside the next k_rj launch (same bits: tests/test_hip_rj.py, the folded adaptation changes nothing).
int RjStepping::iteration(double* swaps_aside) {
    constexpr int64_t RJ_REFRESH = 64;
    int r;
    if (c->rj.tm && c->iter % RJ_REFRESH == RJ_REFRESH - 1 && !fresh && c->rj.tm_drift)
        if ((r = rj_evaluate(c, true))) return r;
    fresh = false;
    const bool blocks = c->rj.gb_n > 0 && !c->rj.gb_whole;            // (hens_rj_set_gibbs; begin() has refused the stretch move)
    // (birth / death updates a template by +- a leaf; so does every accepted Gibbs block, on any schedule)
    c->rj.tm_drift = c->rj.tm != nullptr && (c->rj.schedule != 3 || blocks);
    if (stretch) {
        // red / blue stretch move over every branch and leaf slot: two launches, a half each - the complements of a half
        // belong to the other set, which its launch does not write (red_blue.py:148-323); ONE move (num_mh)
        for (int h = 0; h < 2; ++h)
            if (const RjLaunch half = rj_production(c, RJ_MODE_STRETCH, 0, h); half.ns != 0 && (r = rj_launch(c, half))) return r;
    } else if (group) {
        // group stretch move toward the stationary friend table (group.py:122-281): the table anew when due, from the state in
        // front of the move, then ONE launch - a proposal reads no other walker's current state
        if (c->rj.gr_m % c->rj.gr_update == 0 && (r = rj_group_rebuild(c))) return r;
        if ((r = rj_launch(c, rj_production(c, RJ_MODE_GROUP)))) return r;
        c->rj.gr_m += 1;
    } else if (blocks) {
        // ... block after block of the table (move.py:113-402 under mh.py:79-193): ONE launch walks them all (k_rj_gibbs)
        RjLaunch l = rj_production(c, RJ_MODE_MH);
        l.gibbs = true; l.gb0 = 0; l.gb1 = c->rj.gb_n;
        if ((r = rj_launch(c, l))) return r;
    } else {
        // in-model Gaussian move on the packed leaves (mh.py:56-193)
        if ((r = rj_launch(c, rj_production(c, RJ_MODE_MH)))) return r;
    }
    c->rj.num_mh += blocks ? c->rj.gb_n : 1;      // (num_proposals += 1 per block, mh.py:105-193; the device skips no block)
    rj_cascade(c, 2 * c->iter, true);         // swaps + adaptation (mh.py:190-191, red_blue.py:326-328)
    if (c->rj.schedule == 3) {                // no reversible-jump move (EnsembleSampler without rj_moves): counter and keys as ever
        c->iter += 1;
        return HENS_OK;
    }
    if (swaps_aside && has_pt(c)) {
        flush_adapt(c);
        HIPCHK(c, hipMemcpyAsync(swaps_aside, c->swaps_last, (size_t)(c->T - 1) * 8, hipMemcpyDeviceToDevice, c->stream));
    }
    if ((r = rj_step_bd(c))) return r;
    c->rj.num_bd += 1;
    rj_cascade(c, 2 * c->iter + 1, false);
    c->iter += 1;
    return HENS_OK;
}
}  // namespace

int hens_rj_step(hens_ctx* ctx, int64_t n_iters) {
    hens_ctx_impl* c = enter(ctx);
    int r = rj_ready(c);
    if (r) return r;
    if (n_iters < 0) return fail(c, HENS_ERR_INVALID, "n_iters < 0");
    if ((r = counter_room(c, n_iters))) return r;
    RjStepping st(c);
    if ((r = st.begin(n_iters))) return r;
    for (int64_t i = 0; i < n_iters; ++i)
        if ((r = st.iteration(nullptr))) return r;
    st.finish();
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timing.n_iters = n_iters;
    // the reference raises "The likelihood function is returning Nan." / on an infinite coordinate at once (ensemble.py:1258-
    // 1262, 1542); here once per call: the template likelihood's flags are read back with the call's last launch
    return check_flags(c, true);
}

// ---- chain store of a leaf-packing context (include/hipensemble.h: hens_rj_chain_*, hens_rj_step_chain; csrc/hens_rj_chain.h) ----
// The host protocol is `chain store: what both families share` above; here what a leaf-packing chain has of its own.
static int rjchain_supported(hens_ctx_impl* c) {
    if (!is_rj(c))
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_rj_chain_*: the chain store of a leaf-packing context (HENS_LIKE_TEMPLATE); others: hens_chain_create / hens_step_chain");
    if (!rj_has_model(c)) return fail(c, HENS_ERR_STATE, "hens_rj_chain_*: no model (hens_rj_set_model first)");
    if (c->rj.general)
        return fail(c, HENS_ERR_UNSUPPORTED, "chain store: needs a device likelihood (a model of hens_rj_set_model_general steps through the caller)");
    if (c->Tl != c->T) return fail(c, HENS_ERR_UNSUPPORTED, "chain store: not on a ladder shard (the whole ladder on one GPU)");
    if (c->pipe.on) return fail(c, HENS_ERR_UNSUPPORTED, "chain store: not on a rank of the ladder pipeline");
    return HENS_OK;
}
static hens_chain::RjShape rjchain_shape(const hens_ctx_impl* c, int Ts) {
    hens_chain::RjShape s{c->T, Ts, c->W, c->rj.M.nb, {}, {}};
    for (int b = 0; b < c->rj.M.nb && b < hens_chain::RJ_BRANCHES; ++b) { s.nl[b] = c->rj.M.nl[b]; s.nd[b] = c->rj.M.nd[b]; }
    return s;
}
static_assert(hens_chain::RJ_BRANCHES == RJ_MAX_BRANCH, "hens_chain_host.h: branches of a record");
// a model set anew: the chain of the old one has another shape
static int rjchain_drop(hens_ctx_impl* c) {
    if (!c->chain.on) return HENS_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->chain.release();
    return HENS_OK;
}

int hens_rj_chain_create(hens_ctx* ctx, int64_t capacity, int32_t ntemps_store) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r, Ts = 0;
    if ((r = rjchain_supported(c)) || (r = chain_create_args(c, "hens_rj_chain_create", capacity, ntemps_store, &Ts))) return r;
    hens_chain::RjSizes sz{};
    if (!hens_chain::rj_sizes(rjchain_shape(c, Ts), capacity, &sz))
        return fail(c, HENS_ERR_INVALID, "hens_rj_chain_create: %lld stored steps of %d x %d x %d coordinates do not fit an int64 byte count", (long long)capacity, Ts, c->W, c->rj.M.ind_off);
    ChainStore& ch = c->chain;
    const size_t TsW = (size_t)Ts * c->W, TW = (size_t)c->Tl * c->W, np = swap_slots(c, 1);
    std::vector<ChainBuf> bufs = {{&ch.L, (size_t)sz.lp}, {&ch.P, (size_t)sz.lp}, {&ch.betas, (size_t)sz.betas}, {&ch.acc_tot, TsW * 4},
                                  {&ch.bd_tot, TsW * 4}, {&ch.prev, 2 * TW * 4}, {&ch.swaps_tot, np * 8}, {&ch.swaps_step, np * 8}};
    for (int b = 0; b < c->rj.M.nb; ++b) bufs.insert(bufs.end(), {{&ch.x[b], (size_t)sz.x[b]}, {&ch.inds[b], (size_t)sz.inds[b]}});
    return chain_create(c, "hens_rj_chain_create", capacity, Ts, bufs);
}

int hens_rj_chain_reset(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = chain_open(c, true)) return r;
    return chain_reset(c);
}

int hens_rj_chain_destroy(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    return chain_destroy(c, true);
}

// refuses what rjchain_supported refuses (hens_chain_info answers on any context)
int hens_rj_chain_info(hens_ctx* ctx, hens_chain_info_t* out) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c || !out) return fail(c, HENS_ERR_INVALID, "null argument");
    if (const int r = rjchain_supported(c)) return r;
    hens_chain::RjSizes one{};
    (void)hens_chain::rj_sizes(rjchain_shape(c, chain_Ts(c, true)), 1, &one);
    return chain_info(c, true, one.step, out);
}

// one append: the state by field as it stands between hens_rj_step iterations, the ladder settled by the caller
static int launch_rj_chain_store(hens_ctx_impl* c, ChainTimer& tm) {
    ChainStore& ch = c->chain;
    const RjModel& M = c->rj.M;
    const size_t TW = (size_t)c->Tl * c->W, TsW = (size_t)ch.Ts * c->W, n = (size_t)ch.count;
    RjChainArgs a{};
    a.pool = c->pool; a.loc = c->loc[c->cur]; a.L = c->L[c->cur]; a.P = c->P[c->cur];
    a.acc = c->accepted; a.acc_bd = c->rj.acc_bd;
    a.prev = ch.prev; a.prev_bd = ch.prev + TW;
    a.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    // the in-model cascade's counts: set aside behind it under a birth / death schedule, else swaps_last is still that cascade's
    a.swaps = !has_pt(c) ? nullptr : (c->rj.schedule == 3 ? c->swaps_last : ch.swaps_step);
    for (int b = 0; b < M.nb; ++b) {
        a.off[b] = M.off[b]; a.nl[b] = M.nl[b]; a.nd[b] = M.nd[b];
        a.out_x[b] = ch.x[b] + n * TsW * (size_t)(M.nl[b] * M.nd[b]);
        a.out_inds[b] = ch.inds[b] + n * TsW * (size_t)M.nl[b];
    }
    a.out_L = ch.L + n * TsW; a.out_P = ch.P + n * TsW;
    a.out_betas = ch.betas + n * c->T;
    a.acc_tot = ch.acc_tot; a.bd_tot = ch.bd_tot; a.swaps_tot = ch.swaps_tot;
    a.nb = M.nb; a.ind_off = M.ind_off; a.T = c->T; a.W = c->W; a.Ts = ch.Ts; a.RW = c->D;
    const hens_chain::RjShape shape = rjchain_shape(c, ch.Ts);
    const int vec = hens_chain::rj_store_vec(shape, c->D);
    a.lpr_shift = hens_chain::rj_lane_shift(shape, vec);
    const void* fn = vec == 2 ? reinterpret_cast<const void*>(k_rj_chain_store<2>) : reinterpret_cast<const void*>(k_rj_chain_store<1>);
    return chain_append(c, tm, fn, &a, a.lpr_shift);
}

int hens_rj_step_chain(hens_ctx* ctx, int64_t n_store, int64_t iters_per_store) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r;
    if ((r = rjchain_supported(c)) || (r = chain_open(c, true)) || (r = rj_ready(c))) return r;
    ChainStore& ch = c->chain;
    int64_t iters = 0;
    switch (hens_chain::rj_append_check(ch.capacity, ch.count, n_store, iters_per_store, &iters)) {
    case hens_chain::INVALID: return fail(c, HENS_ERR_INVALID, "hens_rj_step_chain: n_store >= 0 and iters_per_store >= 1, and their product an int64");
    case hens_chain::FULL: return fail(c, HENS_ERR_STATE, "hens_rj_step_chain: %lld more stored steps do not fit a chain of capacity %lld that holds %lld (download and hens_rj_chain_reset)",
                                       (long long)n_store, (long long)ch.capacity, (long long)ch.count);
    default: break;
    }
    if ((r = counter_room(c, iters))) return r;
    RjStepping st(c);
    if ((r = st.begin(iters))) return r;
    const size_t TW = (size_t)c->Tl * c->W;
    ChainTimer tm(c);
    for (int64_t s = 0; s < n_store; ++s) {
        for (int64_t i = 0; i + 1 < iters_per_store; ++i)
            if ((r = st.iteration(nullptr))) return r;
        // the mark: the two accept counters in front of the step's last iteration (the append moves it up: back-to-back stored steps
        // of one iteration each need no copy)
        if (!(ch.mark_valid && ch.mark_books == c->rj.num_mh + c->rj.num_bd)) {
            HIPCHK(c, hipMemcpyAsync(ch.prev, c->accepted, TW * 4, hipMemcpyDeviceToDevice, c->stream));
            HIPCHK(c, hipMemcpyAsync(ch.prev + TW, c->rj.acc_bd, TW * 4, hipMemcpyDeviceToDevice, c->stream));
        }
        ch.mark_valid = false;
        if ((r = st.iteration(ch.swaps_step))) return r;
        SETTLE(c, NEED_LADDER);                   // (the ladder AFTER the step's adaptation - what hens_download_state returns)
        // what hens_download_state runs in front of its copy: the stored log_like is the value the device goes on with
        if (c->rj.tm && c->rj.tm_valid && c->rj.tm_drift && (r = rj_evaluate(c, true))) return r;
        if ((r = launch_rj_chain_store(c, tm))) return r;
        ch.mark_valid = true;                     // (k_rj_chain_store moved the mark up to now)
        ch.mark_books = c->rj.num_mh + c->rj.num_bd;
    }
    st.finish();
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev1, c->stream));
    c->timing.n_iters = iters;
    r = check_flags(c, true);                     // (once per call, with the call's last launch: the host waits for nothing in between)
    tm.fold();                                    // (check_flags has waited for the stream; its result is the call's)
    return r;
}

int hens_rj_chain_download(hens_ctx* ctx, int64_t first, int64_t count, int32_t branch, double* x, uint8_t* inds, double* logl,
                           double* logp, double* betas, int64_t* iteration, int64_t* adapt_time) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = chain_range(c, true, "hens_rj_chain_download", first, count)) return r;
    if (!hens_chain::rj_branch_ok(c->rj.M.nb, branch) || (branch < 0 && (x || inds)))
        return fail(c, HENS_ERR_INVALID, "hens_rj_chain_download: branch %d of %d (-1: the shared fields, x = inds = NULL)", branch, c->rj.M.nb);
    const ChainStore& ch = c->chain;
    const int b = std::max(branch, 0);            // (branch -1: x and inds are null, nothing of a branch is copied)
    const size_t rows = (size_t)ch.Ts * c->W * c->rj.M.nl[b];
    return chain_copy_out(c, first, count, {{x, ch.x[b], rows * c->rj.M.nd[b] * 8}, {inds, ch.inds[b], rows}}, logl, logp, betas, iteration, adapt_time);
}

int hens_rj_chain_totals(hens_ctx* ctx, double* accepted, double* rj_accepted, double* swaps_accepted) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = chain_open(c, true)) return r;
    return chain_totals(c, {{accepted, c->chain.acc_tot}, {rj_accepted, c->chain.bd_tot}}, swaps_accepted);
}

// ---- chain diagnostics of a leaf-packing context (include/hipensemble.h: hens_rj_chain_leaves, hens_rj_chain_leaf_moments,
// hens_rj_chain_moments; csrc/hens_rj_chain_stats.h) ------------------------------------------------------------------------------
static int rj_stats_enter(hens_ctx_impl* c) {
    if (const int r = rjchain_supported(c)) return r;
    return chain_open(c, true);
}
// the selection's plan, or HENS_ERR_INVALID with the offending values
static int rj_stats_plan(hens_ctx_impl* c, const char* who, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps,
                         hens_chain::RjStatPlan* pl) {
    const ChainStore& ch = c->chain;
    if (!hens_chain::rj_stat_plan(rjchain_shape(c, ch.Ts), ch.count, branch, first, count, thin, ntemps, pl))
        return fail(c, HENS_ERR_INVALID, "%s: branch %d in [0, %d), 1 <= count <= 2^31, thin >= 1, ntemps %d in [1, %d] and the kept steps %lld, %lld + %lld, ... (%lld of them) inside the %lld stored",
                    who, branch, c->rj.M.nb, ntemps, ch.Ts, (long long)first, (long long)first, (long long)thin, (long long)count, (long long)ch.count);
    static_assert(hens_chain::RJ_STAT_LANES == RJ_STAT_LANES, "hens_chain_host.h sizes the table of k_rj_chain_leaves");
    return HENS_OK;
}
static RjStatArgs rj_stat_args(const ChainStore& ch, int32_t branch, const hens_chain::RjStatPlan& pl, int64_t count) {
    RjStatArgs a{};
    a.inds = ch.inds[branch] + pl.inds_offset; a.x = ch.x[branch] + pl.x_offset;
    a.inds_stride = pl.inds_stride; a.x_stride = pl.x_stride;
    a.count = count; a.nplaces = pl.nplaces;
    a.nl = (int32_t)pl.nl; a.nd = (int32_t)pl.nd;
    return a;
}

int hens_rj_chain_leaves(hens_ctx* ctx, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps, uint8_t* nleaves,
                         uint32_t* hist) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r;
    hens_chain::RjStatPlan pl{};
    if ((r = rj_stats_enter(c)) || (r = rj_stats_plan(c, "hens_rj_chain_leaves", branch, first, count, thin, ntemps, &pl))) return r;
    ChainStore& ch = c->chain;
    const int64_t blocks = hens_chain::stat_blocks(pl.nplaces, RJ_STAT_LANES);
    int64_t nbytes = 0;
    if (blocks > INT32_MAX || !hens_chain::mul(count, pl.nplaces, &nbytes))
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_rj_chain_leaves: %lld places over %lld kept steps are more than one launch covers", (long long)pl.nplaces, (long long)count);
    if (!nleaves && !hist) return HENS_OK;
    SETTLE(c, NEED_DEVICE);
    const size_t hbytes = (size_t)pl.nplaces * (size_t)(pl.nl + 1) * 4;
    char* dev = nullptr;
    HIPCHK(c, hipMalloc((void**)&dev, hbytes + (nleaves ? (size_t)nbytes : 0)));
    RjStatArgs a = rj_stat_args(ch, branch, pl, count);
    a.hist = reinterpret_cast<uint32_t*>(dev);
    a.nleaves = nleaves ? reinterpret_cast<uint8_t*>(dev + hbytes) : nullptr;
    const void* fn = pl.vec == 4 ? reinterpret_cast<const void*>(k_rj_chain_leaves<4>) : reinterpret_cast<const void*>(k_rj_chain_leaves<1>);
    return chain_stats_run(c, fn, dim3((unsigned)blocks), dim3(RJ_STAT_LANES), (size_t)pl.lds_bytes, &a, dev,
                           {{hist, dev, hbytes}, {nleaves, dev + hbytes, (size_t)nbytes}}, &ch.leaves_ms, "k_rj_chain_leaves");
}

int hens_rj_chain_leaf_moments(hens_ctx* ctx, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps, int64_t lo,
                               int64_t hi, double* sum, double* m2, int64_t* n) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    int r;
    hens_chain::RjStatPlan pl{};
    if ((r = rj_stats_enter(c)) || (r = rj_stats_plan(c, "hens_rj_chain_leaf_moments", branch, first, count, thin, ntemps, &pl))) return r;
    if (!hens_chain::rj_window_ok(lo, hi))
        return fail(c, HENS_ERR_INVALID, "hens_rj_chain_leaf_moments: the ordinal window [%lld, %lld) needs 0 <= lo < hi", (long long)lo, (long long)hi);
    ChainStore& ch = c->chain;
    const int64_t blocks = hens_chain::stat_blocks(pl.nseries, RJ_STAT_LANES);
    if (blocks > INT32_MAX) return fail(c, HENS_ERR_UNSUPPORTED, "hens_rj_chain_leaf_moments: %lld series are more than one launch covers", (long long)pl.nseries);
    if (!sum && !m2 && !n) return HENS_OK;
    SETTLE(c, NEED_DEVICE);
    const size_t sbytes = (size_t)pl.nseries * 8, pbytes = (size_t)pl.nplaces * 8;
    char* dev = nullptr;
    HIPCHK(c, hipMalloc((void**)&dev, 2 * sbytes + pbytes));
    RjStatArgs a = rj_stat_args(ch, branch, pl, count);
    a.lo = lo; a.hi = hi;
    a.sum = reinterpret_cast<double*>(dev);
    a.m2 = m2 ? reinterpret_cast<double*>(dev + sbytes) : nullptr;
    a.n = reinterpret_cast<long long*>(dev + 2 * sbytes);
    const void* fn = pl.vec == 4 ? reinterpret_cast<const void*>(k_rj_chain_leaf_moments<4>) : reinterpret_cast<const void*>(k_rj_chain_leaf_moments<1>);
    return chain_stats_run(c, fn, dim3((unsigned)blocks), dim3(RJ_STAT_LANES), 0, &a, dev,
                           {{sum, dev, sbytes}, {m2, dev + sbytes, sbytes}, {n, dev + 2 * sbytes, pbytes}}, &ch.leaf_moments_ms, "k_rj_chain_leaf_moments");
}

// the chain as it lies - a one-leaf branch's coordinates (NaN where the leaf is unused: it propagates, as in the reference), logl /
// logp masked - through k_chain_moments unchanged
int hens_rj_chain_moments(hens_ctx* ctx, int32_t field, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps,
                          double* sum, double* m2, int64_t* n_finite) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int r = rj_stats_enter(c)) return r;
    ChainStore& ch = c->chain;
    hens_chain::StatPlan pl{};
    if (!hens_chain::rj_plain_plan(rjchain_shape(c, ch.Ts), ch.count, field, branch, first, count, thin, ntemps, &pl))
        return fail(c, HENS_ERR_INVALID, "hens_rj_chain_moments: field %d in [0, 2], branch %d in [0, %d) (field 0), count >= 1, thin >= 1, ntemps %d in [1, %d] and the kept steps %lld, %lld + %lld, ... (%lld of them) inside the %lld stored",
                    field, branch, c->rj.M.nb, ntemps, ch.Ts, (long long)first, (long long)first, (long long)thin, (long long)count, (long long)ch.count);
    const int r = chain_moments_run(c, field == 0 ? ch.x[branch] : field == 1 ? ch.L : ch.P, pl, count, field != 0, sum, m2, n_finite, "hens_rj_chain_moments");
    if (r == HENS_OK && (sum || m2 || n_finite)) ch.leaf_moments_ms = ch.moments_ms;
    return r;
}

// leaves_ms: the last k_rj_chain_leaves launch; moments_ms: the last k_rj_chain_leaf_moments or k_chain_moments launch, whichever
// ran later (-1: none yet)
int hens_rj_chain_stats_ms(hens_ctx* ctx, double* leaves_ms, double* moments_ms) {
    hens_ctx_impl* c = CTX(ctx);
    if (!c) return no_context();
    if (const int r = rjchain_supported(c)) return r;
    if (leaves_ms) *leaves_ms = c->chain.leaves_ms;
    if (moments_ms) *moments_ms = c->chain.leaf_moments_ms;
    return HENS_OK;
}

// ---- leaf-packing moves with a HOST-CALLABLE likelihood (round 6; ensemble.py:1306-1334,1340-1545, rj.py:145-388) ---------------
// hens_rj_propose runs the proposal half of one teacher-forced move on the records - in-model Gaussian move on every active leaf,
// birth / death on one branch or on all of them, a red / blue stretch half-step - up to and including the log-prior, and hands the
// proposed records back; the caller packs the active leaves the way compute_log_like does (groups_from_inds order) and calls the
// user's function; hens_rj_accept finishes the move with those log-likelihoods.  The leaf-packing twin of hens_propose_split /
// hens_accept_split.
int hens_rj_propose(hens_ctx* ctx, int32_t move, const hens_rj_draws* d, double* q_out, double* logp_out, uint8_t* moved_out) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !d || !q_out || !logp_out || !moved_out) return fail(c, HENS_ERR_INVALID, "null argument");
    if (const int rk = need_rj_context(c)) return rk;
    if (c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_accept must follow hens_rj_propose");
    if (c->rj.mt_K > 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_rj_propose: not under a multiple-try proposal (hens_rj_set_mt_proposal: the tries' likelihoods are the device's)");
    if (move == HENS_RJ_MOVE_MH && c->rj.gb_n > 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records need a device likelihood (hens_rj_set_gibbs(ctx, 0, NULL) clears the table)");
    if ((move == HENS_RJ_MOVE_MH || move == HENS_RJ_MOVE_STRETCH) && c->rj.gr_nf > 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "hens_rj_propose of the in-model move: not while a group is set (hens_rj_set_group(ctx, 0, ...) clears it)");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W, RW = (size_t)c->rj.M.RW;
    int r;
    if (!c->rj.hq) {
        if ((r = dalloc(c, &c->rj.hq, TW * RW))) return r;
        if ((r = dalloc(c, &c->rj.hlogp, TW))) return r;
        if ((r = dalloc(c, &c->rj.hfac, TW))) return r;
        if ((r = dalloc(c, &c->rj.hlu, TW))) return r;
        if ((r = dalloc(c, &c->rj.hlogl, TW))) return r;
        if ((r = dalloc(c, &c->rj.hmoved, TW))) return r;
    }
    HIPCHK(c, hipMemsetAsync(c->rj.hmoved, 0, TW, c->stream));
    if (move < HENS_RJ_MOVE_MH || move > HENS_RJ_MOVE_STRETCH)
        return fail(c, HENS_ERR_INVALID, "hens_rj_propose: move must be HENS_RJ_MOVE_MH, _BD, _BD_ALL or _STRETCH");
    if ((r = rj_forced_move(c, move, *d, nullptr, true))) return r;
    HIPCHK(c, hipMemcpyAsync(q_out, c->rj.hq, TW * RW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(logp_out, c->rj.hlogp, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(moved_out, c->rj.hmoved, TW, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rj.accept_pending = true;
    return HENS_OK;
}

int hens_rj_accept(hens_ctx* ctx, const double* logl, uint8_t* keep_out) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !logl) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_accept must follow hens_rj_propose");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W;
    for (size_t i = 0; i < TW; ++i)
        if (logl[i] != logl[i]) return fail(c, HENS_ERR_NONFINITE, "The likelihood function is returning Nan.");       // ensemble.py:1542
    HIPCHK(c, hipMemcpyAsync(c->rj.hlogl, logl, TW * 8, hipMemcpyHostToDevice, c->stream));
    RjAcceptArgs a{};
    a.pool = c->pool; a.loc = c->loc[c->cur]; a.L = c->L[c->cur]; a.P = c->P[c->cur];
    a.betas = c->cfg.tempered ? c->betas[c->bcur] : nullptr;
    a.accepted = c->rj.pending_acc; a.keep_out = c->rj.keep;
    a.hq = c->rj.hq; a.hlogp = c->rj.hlogp; a.hfac = c->rj.hfac; a.hlu = c->rj.hlu; a.hmoved = c->rj.hmoved; a.logl = c->rj.hlogl;
    a.Tl = c->Tl; a.W = c->W; a.RW = c->rj.M.RW; a.rung_begin = c->cfg.rung_begin; a.tempered = c->cfg.tempered;
    hipLaunchKernelGGL(k_rj_accept, dim3((unsigned)((TW + 3) / 4)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->rj.keep, TW, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->rj.accept_pending = false;
    return HENS_OK;
}

int hens_rj_set_schedule(hens_ctx* ctx, int32_t schedule) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rk = need_rj_context(c)) return rk;
    if (schedule < 0 || schedule > 3) return fail(c, HENS_ERR_UNSUPPORTED, "rj schedule must be 0 (separate_branches), 1 (iterate_branches), 2 (together) or 3 (none)");
    c->rj.schedule = schedule;
    return HENS_OK;
}

int hens_rj_set_in_model(hens_ctx* ctx, int32_t kind) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rk = need_rj_context(c)) return rk;
    if (c->rj.general) return fail(c, HENS_ERR_STATE, "the Philox in-model move belongs to hens_rj_step: template models only");
    if (kind != HENS_RJ_INMODEL_GAUSSIAN && kind != HENS_RJ_INMODEL_STRETCH && kind != HENS_RJ_INMODEL_GROUP)
        return fail(c, HENS_ERR_INVALID, "in-model move must be HENS_RJ_INMODEL_GAUSSIAN, HENS_RJ_INMODEL_STRETCH or HENS_RJ_INMODEL_GROUP");
    if (kind == HENS_RJ_INMODEL_GROUP && c->rj.gr_nf == 0)
        return fail(c, HENS_ERR_STATE, "HENS_RJ_INMODEL_GROUP: no group set (hens_rj_set_group first)");
    if (kind == HENS_RJ_INMODEL_STRETCH && c->rj.gb_n > 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records step the Gaussian in-model move (hens_rj_set_gibbs(ctx, 0, NULL) clears the table)");
    c->rj.in_model = kind;
    return HENS_OK;
}

// The stretch move's draws of iteration `iter` in the form hens_rj_stretch_split takes: k_rj_debug_stretch lists them by split
// position; here the two sets are put in ascending walker order and a complement becomes its index in the other set's list.
int hens_rj_debug_draws_stretch(hens_ctx* ctx, int64_t iter, uint8_t* labels, int64_t* rint, double* u_zz, double* u_acc) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (const int rm = need_rj_model(c)) return rm;
    if (!labels || !rint || !u_zz || !u_acc) return fail(c, HENS_ERR_INVALID, "null output");
    SETTLE(c, NEED_DEVICE);
    const int Tl = c->Tl, W = c->W, nb = c->rj.M.nb, n0 = (W + 1) / 2;
    const size_t TW = (size_t)Tl * W;
    DeviceScratch sc;
    RjDebugStretchArgs a{};
    a.own = sc.grab<int32_t>(TW); a.cw = sc.grab<int32_t>(TW * nb); a.uzz = sc.grab<double>(TW); a.uacc = sc.grab<double>(TW);
    if (!a.own || !a.cw || !a.uzz || !a.uacc) return fail(c, HENS_ERR_HIP, "hens_rj_debug_draws_stretch: out of device memory");
    a.iter = (uint64_t)iter; a.seed = c->cfg.seed;
    a.Tl = Tl; a.W = W; a.rung_begin = c->cfg.rung_begin; a.nb = nb; a.bits = c->idx_bits;
    hipLaunchKernelGGL(k_rj_debug_stretch, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    std::vector<int32_t> own(TW), cw(TW * nb);
    std::vector<double> uz(TW), ua(TW);
    HIPCHK(c, hipMemcpyAsync(own.data(), a.own, TW * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cw.data(), a.cw, TW * nb * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(uz.data(), a.uzz, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(ua.data(), a.uacc, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    std::fill(rint, rint + (size_t)2 * nb * Tl * n0, (int64_t)0);
    std::fill(u_zz, u_zz + (size_t)2 * Tl * n0, 0.0);
    std::fill(u_acc, u_acc + (size_t)2 * Tl * n0, 0.0);
    std::vector<int32_t> qof(W), rank(W);
    for (int t = 0; t < Tl; ++t) {
        for (int q = 0; q < W; ++q) {
            const int w = own[(size_t)t * W + q];
            if (w < 0 || w >= W) return fail(c, HENS_ERR_STATE, "hens_rj_debug_draws_stretch: the split is not a permutation");
            qof[w] = q;
            labels[(size_t)t * W + w] = q >= n0 ? 1 : 0;
        }
        int cnt[2] = {0, 0};
        for (int w = 0; w < W; ++w) rank[w] = cnt[labels[(size_t)t * W + w]]++;       // index in the own set's ascending list
        for (int w = 0; w < W; ++w) {
            const int h = labels[(size_t)t * W + w], k = rank[w];
            const size_t e = (size_t)t * W + qof[w];
            for (int b = 0; b < nb; ++b) rint[(((size_t)h * nb + b) * Tl + t) * n0 + k] = rank[cw[(size_t)b * TW + e]];
            u_zz[((size_t)h * Tl + t) * n0 + k] = uz[e];
            u_acc[((size_t)h * Tl + t) * n0 + k] = ua[e];
        }
    }
    return HENS_OK;
}

int hens_rj_debug_draws(hens_ctx* ctx, int64_t iter, double* step, double* u_mh, int32_t* branch, int8_t* coin, uint32_t* sel,
                        double* birth, double* u_bd, int32_t* slot_mh, double* uswap_mh, int32_t* slot_bd, double* uswap_bd) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (const int rm = need_rj_model(c)) return rm;
    const bool stretch = c->rj.in_model != HENS_RJ_INMODEL_GAUSSIAN;      // (its draws: hens_rj_debug_draws_stretch / hens_rj_group_debug_draws; step / u_mh are zeros here)
    if (!stretch && !c->rj.have_scale) return fail(c, HENS_ERR_STATE, "in-model step scale not set (hens_rj_set_mh_scale)");
    if (!step || !u_mh || !branch || !coin || !sel || !birth || !u_bd) return fail(c, HENS_ERR_INVALID, "null output");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W, IO = (size_t)c->rj.M.ind_off;
    DeviceScratch sc;
    RjDebugArgs a{};
    a.M = c->rj.M;
    a.step = sc.grab<double>(TW * IO); a.u_mh = sc.grab<double>(TW); a.coin = sc.grab<int8_t>(TW);
    a.sel = sc.grab<uint32_t>(TW); a.birth = sc.grab<double>(TW * (size_t)c->rj.M.ndmax); a.u_bd = sc.grab<double>(TW);
    if (!a.step || !a.u_mh || !a.coin || !a.sel || !a.birth || !a.u_bd) return fail(c, HENS_ERR_HIP, "hens_rj_debug_draws: out of device memory");
    a.iter = (uint64_t)iter; a.seed = c->cfg.seed;
    a.Tl = c->Tl; a.W = c->W; a.rung_begin = c->cfg.rung_begin; a.stretch = stretch ? 1 : 0;
    a.use_chol = c->rj.have_chol ? 1 : 0;
    memcpy(a.chol, c->rj.chol, sizeof(a.chol));
    a.ctab = c->rj.ctab; a.cbn = c->rj.cbn;
    // "separate_branches" (and no birth / death move at all: what one WOULD draw): the chosen branch's draws; "iterate_branches",
    // "together": every branch's, in order (outputs [nbranches][...])
    const bool every = c->rj.schedule == 1 || c->rj.schedule == 2;
    const int nsub = every ? c->rj.M.nb : 1;
    *branch = every ? -1 : rj_branch_of(c, (uint64_t)iter);
    for (int k = 0; k < nsub; ++k) {
        a.branch = every ? k : *branch;
        a.acc_branch = c->rj.schedule == 2 ? c->rj.M.nb : a.branch;      // ("together": ONE accept uniform, in every row of u_bd)
        hipLaunchKernelGGL(k_rj_debug_draws, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, a);
        HIPCHK(c, hipGetLastError());
        if (k == 0) {
            HIPCHK(c, hipMemcpyAsync(step, a.step, TW * IO * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipMemcpyAsync(u_mh, a.u_mh, TW * 8, hipMemcpyDeviceToHost, c->stream));
        }
        HIPCHK(c, hipMemcpyAsync(coin + (size_t)k * TW, a.coin, TW, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(sel + (size_t)k * TW, a.sel, TW * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(birth + (size_t)k * TW * c->rj.M.ndmax, a.birth, TW * (size_t)c->rj.M.ndmax * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(u_bd + (size_t)k * TW, a.u_bd, TW * 8, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (has_pt(c) && slot_mh && uswap_mh && slot_bd && uswap_bd) {       // the two cascades of the iteration (rj_cascade's keys)
        const size_t n = (size_t)c->T * c->W;
        int32_t* ds = sc.grab<int32_t>(n);
        double* du = sc.grab<double>(n);
        if (!ds || !du) return fail(c, HENS_ERR_HIP, "hens_rj_debug_draws: out of device memory");
        for (int k = 0; k < 2; ++k)
            if (const int r = export_pt_draws(c, ds, du, 2 * (uint64_t)iter + (uint64_t)k, k ? slot_bd : slot_mh, k ? uswap_bd : uswap_mh)) return r;
    }
    return HENS_OK;
}

// ---- Gibbs blocks over branches and leaf slots for the in-model Gaussian move (include/hipensemble.h; csrc/hens_rj_gibbs.h) --------
int hens_rj_set_gibbs(hens_ctx* ctx, int32_t nblocks, const uint8_t* mask) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rk = need_rj_context(c)) return rk;
    if (const int rm = need_rj_model(c)) return rm;
    if (c->expect_split != 0 || c->propose_pending || c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    if (nblocks == 0) { c->rj.gb_n = 0; c->rj.gb_whole = false; c->rj.gb_sel = 0; return HENS_OK; }
    if (c->rj.general)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records need a device likelihood (this context's model: hens_rj_set_model_general)");
    if (c->rj.in_model == HENS_RJ_INMODEL_STRETCH)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records step the Gaussian in-model move (hens_rj_set_in_model(HENS_RJ_INMODEL_GAUSSIAN))");
    if (c->rj.gr_nf > 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for the group stretch move (hens_rj_set_group(ctx, 0, ...) clears the group)");
    const RjModel& M = c->rj.M;
    int slots = 0;
    for (int b = 0; b < M.nb; ++b) slots += M.nl[b];
    if (slots > 64) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks: %d leaf slots, at most 64 over all branches", slots);
    if (c->D > RJ_MAX_RW) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks: record width ndim = %d, at most %d doubles", c->D, RJ_MAX_RW);
    ParsedRjGibbs p = parse_rj_gibbs(nblocks, mask, M.ind_off);
    if (p.why[0]) return fail(c, HENS_ERR_INVALID, "hens_rj_set_gibbs: %s", p.why);
    SETTLE(c, NEED_DEVICE);
    if (!c->rj.gb_tab)
        if (const int r = dalloc(c, &c->rj.gb_tab, (size_t)RJ_GIBBS_MAX_BLOCKS * RJ_MAX_RW)) return r;
    HIPCHK(c, hipMemcpyAsync(c->rj.gb_tab, p.table.data(), p.table.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // (the vector goes out of scope; launches in flight have read the old table)
    c->rj.gb_n = nblocks; c->rj.gb_whole = p.whole; c->rj.gb_sel = 0;
    return HENS_OK;
}

// teacher-forced: the block the next hens_rj_mh_step belongs to; between complete moves (hens_gibbs_select's rules)
int hens_rj_gibbs_select(hens_ctx* ctx, int32_t block) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rk = need_rj_context(c)) return rk;
    if (c->expect_split != 0 || c->propose_pending || c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "hens_rj_gibbs_select between the half-steps of a move");
    if (c->rj.gb_n == 0) return fail(c, HENS_ERR_STATE, "no Gibbs table on the in-model move (hens_rj_set_gibbs)");
    if (block < 0 || block >= c->rj.gb_n) return fail(c, HENS_ERR_INVALID, "block must be in [0, %d)", c->rj.gb_n);
    c->rj.gb_sel = block;
    return HENS_OK;
}

int hens_rj_gibbs_debug_draws(hens_ctx* ctx, int64_t iter, int32_t block, double* step, double* u_mh) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (const int rm = need_rj_model(c)) return rm;
    if (c->rj.gb_n == 0) return fail(c, HENS_ERR_STATE, "no Gibbs table on the in-model move (hens_rj_set_gibbs)");
    if (block < 0 || block >= c->rj.gb_n) return fail(c, HENS_ERR_INVALID, "block must be in [0, %d)", c->rj.gb_n);
    if (!c->rj.have_scale) return fail(c, HENS_ERR_STATE, "in-model step scale not set (hens_rj_set_mh_scale)");
    if (!step || !u_mh) return fail(c, HENS_ERR_INVALID, "null output");
    SETTLE(c, NEED_DEVICE);
    const size_t TW = (size_t)c->Tl * c->W, IO = (size_t)c->rj.M.ind_off;
    DeviceScratch sc;
    RjGibbsDebugArgs a{};
    a.M = c->rj.M;
    a.step = sc.grab<double>(TW * IO); a.u_mh = sc.grab<double>(TW);
    if (!a.step || !a.u_mh) return fail(c, HENS_ERR_HIP, "hens_rj_gibbs_debug_draws: out of device memory");
    a.iter = (uint64_t)iter; a.seed = c->cfg.seed;
    a.Tl = c->Tl; a.W = c->W; a.rung_begin = c->cfg.rung_begin; a.block = block;
    a.use_chol = c->rj.have_chol ? 1 : 0;
    memcpy(a.chol, c->rj.chol, sizeof(a.chol));
    hipLaunchKernelGGL(k_rj_gibbs_debug_draws, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(step, a.step, TW * IO * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(u_mh, a.u_mh, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

// ---- the group stretch move with a stationary friend table (include/hipensemble.h; csrc/hens_rj_group.h) ---------------------------
int hens_rj_set_group(hens_ctx* ctx, int32_t nfriends, int32_t n_iter_update, const int32_t* key_dim, double a) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rk = need_rj_context(c)) return rk;
    if (const int rm = need_rj_model(c)) return rm;
    if (c->expect_split != 0 || c->propose_pending || c->rj.accept_pending) return fail(c, HENS_ERR_STATE, "a half-step is pending");
    if (nfriends == 0) { rj_group_clear(c); return HENS_OK; }
    const RjModel& M = c->rj.M;
    if (nfriends < 0 || nfriends > RJ_GROUP_MAX_FRIENDS) return fail(c, HENS_ERR_INVALID, "hens_rj_set_group: nfriends must be in [0, %d] (%d)", RJ_GROUP_MAX_FRIENDS, nfriends);
    if (n_iter_update <= 1 && !(n_iter_update == 1 && c->cfg.live_dangerously))        // group.py:45-46
        return fail(c, HENS_ERR_INVALID, "n_iter_update must be greather than or equal to 2.");
    if (!key_dim) return fail(c, HENS_ERR_INVALID, "hens_rj_set_group: null key_dim");
    if (!(a > 1.0) || !(a < INFINITY)) return fail(c, HENS_ERR_INVALID, "hens_rj_set_group: the stretch scale a must be finite and > 1");
    if (c->rj.general)
        return fail(c, HENS_ERR_UNSUPPORTED, "the group stretch move needs a device likelihood (this context's model: hens_rj_set_model_general)");
    for (int b = 0; b < M.nb; ++b)
        if (key_dim[b] < 0 || key_dim[b] >= M.nd[b])
            return fail(c, HENS_ERR_INVALID, "hens_rj_set_group: key_dim[%d] = %d, a leaf of branch %d has parameters 0 .. %d", b, key_dim[b], b, M.nd[b] - 1);
    int slots = 0;
    for (int b = 0; b < M.nb; ++b) slots += M.nl[b];
    if (slots > RJ_GROUP_SLOTS) return fail(c, HENS_ERR_UNSUPPORTED, "group stretch move: %d leaf slots, at most %d over all branches", slots, RJ_GROUP_SLOTS);
    if (c->D > RJ_MAX_RW) return fail(c, HENS_ERR_UNSUPPORTED, "group stretch move: record width ndim = %d, at most %d doubles", c->D, RJ_MAX_RW);
    if (c->rj.gb_n > 0)
        return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for the group stretch move (hens_rj_set_gibbs(ctx, 0, NULL) clears the table)");
    const size_t TW = (size_t)c->Tl * c->W, rows = 2 * TW, cap = (size_t)c->W * RJ_GROUP_SLOTS;
    if (rows >= ((size_t)1 << 25)) return fail(c, HENS_ERR_UNSUPPORTED, "group stretch move: %zu pool rows, fewer than 2^25", rows);
    SETTLE(c, NEED_DEVICE);
    hens_ctx_impl::Rj& s = c->rj;
    if (!s.gr_keys) {
        int r;
        if ((r = dalloc(c, &s.gr_keys, cap)) || (r = dalloc(c, &s.gr_tab, cap * RJ_MAX_ND)) || (r = dalloc(c, &s.gr_gkey, cap)) ||
            (r = dalloc(c, &s.gr_gsrc, cap)) || (r = dalloc(c, &s.gr_cnt, (size_t)RJ_MAX_BRANCH)) ||
            (r = dalloc(c, &s.gr_start, rows * RJ_GROUP_SLOTS)) || (r = dalloc(c, &s.gr_snap, rows * RJ_MAX_BRANCH)) ||
            (r = dalloc(c, &s.gr_pick, TW * RJ_GROUP_SLOTS))) {
            s.gr_keys = nullptr;              // (whatever was made stays with the context until it is destroyed; the next call tries again)
            return r;
        }
    }
    s.gr_nf = nfriends; s.gr_update = n_iter_update; s.gr_a = a; s.gr_nslots = slots;
    for (int b = 0, off = 0; b < RJ_MAX_BRANCH; ++b) {
        s.gr_key[b] = b < M.nb ? key_dim[b] : 0;
        s.gr_koff[b] = off;
        if (b < M.nb) off += c->W * M.nl[b];
    }
    return rj_group_reset(c);
}

static int need_rj_group(hens_ctx_impl* c) {
    return c->rj.gr_nf > 0 ? HENS_OK : fail(c, HENS_ERR_STATE, "no group set (hens_rj_set_group)");
}

int hens_rj_group_rebuild(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (const int r = rj_ready(c)) return r;
    if (const int rg = need_rj_group(c)) return rg;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    return rj_group_rebuild(c);
}

int hens_rj_group_step(hens_ctx* ctx, const int32_t* pick, const double* u_zz, const double* u_acc, uint8_t* keep_out) {
    hens_ctx_impl* c = enter(ctx);
    int r = rj_ready(c);
    if (r) return r;
    if ((r = need_rj_group(c))) return r;
    if (!pick || !u_zz || !u_acc) return fail(c, HENS_ERR_INVALID, "hens_rj_group_step: null draws");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    if ((r = rj_ensure_staging(c))) return r;
    const size_t TW = (size_t)c->Tl * c->W;
    hens_ctx_impl::Rj& s = c->rj;
    HIPCHK(c, hipMemcpyAsync(s.gr_pick, pick, TW * (size_t)s.gr_nslots * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.uzz, u_zz, TW * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipMemcpyAsync(s.u, u_acc, TW * 8, hipMemcpyHostToDevice, c->stream));
    RjLaunch l{RJ_MODE_GROUP};
    l.draws = RjLaunch::FORCED; l.u_acc = s.u; l.keep = s.keep; l.st_uzz = s.uzz; l.gr_pick = s.gr_pick;
    s.tm_valid = false;                       // (teacher-forced move: the reference's full evaluation, no resident templates)
    if ((r = rj_launch(c, l))) return r;
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, s.keep, TW, hipMemcpyDeviceToHost, c->stream));
    if ((r = check_flags(c, false))) return r;
    s.num_mh += 1;
    s.gr_m += 1;
    if (!has_pt(c)) c->iter += 1;
    return HENS_OK;
}

int hens_rj_group_debug(hens_ctx* ctx, int32_t* counts, double* keys, double* tab, int32_t* start) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rm = need_rj_model(c)) return rm;
    if (const int rg = need_rj_group(c)) return rg;
    if (!c->have_state) return fail(c, HENS_ERR_STATE, "no state uploaded");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const hens_ctx_impl::Rj& s = c->rj;
    const size_t TW = (size_t)c->Tl * c->W, cap = (size_t)c->W * s.gr_nslots;
    if (counts) HIPCHK(c, hipMemcpyAsync(counts, s.gr_cnt, (size_t)s.M.nb * 4, hipMemcpyDeviceToHost, c->stream));
    if (keys) HIPCHK(c, hipMemcpyAsync(keys, s.gr_keys, cap * 8, hipMemcpyDeviceToHost, c->stream));
    if (tab) HIPCHK(c, hipMemcpyAsync(tab, s.gr_tab, cap * RJ_MAX_ND * 8, hipMemcpyDeviceToHost, c->stream));
    DeviceScratch sc;
    if (start) {
        int32_t* d = sc.grab<int32_t>(TW * s.gr_nslots);
        if (!d) return fail(c, HENS_ERR_HIP, "hens_rj_group_debug: out of device memory");
        hipLaunchKernelGGL(k_rj_group_export, dim3(grid_for((int64_t)TW * s.gr_nslots)), dim3(256), 0, c->stream, s.gr_start, c->loc[c->cur], d, (int64_t)TW, s.gr_nslots);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(start, d, TW * s.gr_nslots * 4, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

int hens_rj_group_debug_draws(hens_ctx* ctx, int64_t iter, int32_t* pick, double* u_zz, double* u_acc) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || iter < 0) return fail(c, HENS_ERR_INVALID, "null context / negative iteration");
    if (const int rm = need_rj_model(c)) return rm;
    if (const int rg = need_rj_group(c)) return rg;
    if (!pick || !u_zz || !u_acc) return fail(c, HENS_ERR_INVALID, "null output");
    SETTLE(c, NEED_DEVICE);
    const hens_ctx_impl::Rj& s = c->rj;
    const size_t TW = (size_t)c->Tl * c->W;
    DeviceScratch sc;
    RjGroupDebugArgs a{};
    a.M = s.M; a.cnt = s.gr_cnt;
    a.pick = sc.grab<int32_t>(TW * s.gr_nslots); a.u_zz = sc.grab<double>(TW); a.u_acc = sc.grab<double>(TW);
    if (!a.pick || !a.u_zz || !a.u_acc) return fail(c, HENS_ERR_HIP, "hens_rj_group_debug_draws: out of device memory");
    a.iter = (uint64_t)iter; a.seed = c->cfg.seed;
    a.Tl = c->Tl; a.W = c->W; a.rung_begin = c->cfg.rung_begin; a.nfriends = s.gr_nf;
    hipLaunchKernelGGL(k_rj_group_debug_draws, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, a);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(pick, a.pick, TW * s.gr_nslots * 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(u_zz, a.u_zz, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(u_acc, a.u_acc, TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

int hens_rj_get_counters(hens_ctx* ctx, double* accepted_bd, int64_t* num_mh, int64_t* num_bd) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rm = need_rj_model(c)) return rm;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (accepted_bd)
        if (const int r = read_counters(c, (size_t)c->Tl * c->W, {{accepted_bd, c->rj.acc_bd}})) return r;
    if (num_mh) *num_mh = c->rj.num_mh;
    if (num_bd) *num_bd = c->rj.num_bd;
    return HENS_OK;
}

int hens_rj_debug_resident(hens_ctx* ctx, double* rec, double* logl) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (const int rm = need_rj_model(c)) return rm;
    if (!c->have_state) return fail(c, HENS_ERR_STATE, "no state uploaded");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    const size_t TW = (size_t)c->Tl * c->W;
    // (hens_download_state without the evaluation in front of its copy: the log-likelihoods as hens_rj_step's +- leaf updates left them)
    if (rec) {
        hipLaunchKernelGGL(k_gather_rows, dim3(grid_for((int64_t)TW * c->D)), dim3(256), 0, c->stream, c->pool,
                           c->loc[c->cur], c->xtmp, (int64_t)TW, c->D, guest_delta(c));
        HIPCHK(c, hipMemcpyAsync(rec, c->xtmp, TW * c->D * 8, hipMemcpyDeviceToHost, c->stream));
    }
    if (logl) HIPCHK(c, hipMemcpyAsync(logl, c->L[c->cur], TW * 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

// ---- ladder sharding ---------------------------------------------------------------------------------
int hens_get_device_buffers(hens_ctx* ctx, hens_device_buffers* out) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !out) return fail(c, HENS_ERR_INVALID, "null argument");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    int r = ensure_shard_buffers(c);
    if (r) return r;
    out->logl = c->L[c->cur];
    out->gather_logl = c->gather_L;
    out->send_rows = c->send_rows;
    out->recv_rows = c->recv_rows;
    out->row_capacity = c->row_capacity;
    out->row_doubles = c->D + 2;
    out->stream = c->stream;
    return HENS_OK;
}

int hens_stretch_iter(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, true);
    if (r) return r;
    if (c->expect_split != 0) return fail(c, HENS_ERR_STATE, "hens_stretch_iter between split 0 and split 1");
    if ((r = counter_room(c, 1))) return r;
    if (c->cfg.likelihood_kind == HENS_LIKE_HOST) return fail(c, HENS_ERR_UNSUPPORTED, "hens_stretch_iter needs a device likelihood");
    if (c->pt_pending) return fail(c, HENS_ERR_STATE, "sharded PT exchange in flight");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    c->N0 = (c->W + 1) / 2;
    if (!(c->iter >= c->win_from && c->iter < c->win_from + (uint64_t)c->win_count)) {
        // plan a whole batch (splits of the resident rungs + every PT column map) once per NB iterations
        launch_plan(c, c->stream, 0, c->iter, c->NB);
        c->win_from = c->iter;
        c->win_count = c->NB;
    }
    r = stretch_pair(c, 0, (int)(c->iter - c->win_from), nullptr);
    if (r) return r;
    if (!has_pt(c)) c->iter += 1;
    HIPCHK(c, hipGetLastError());
    return HENS_OK;
}

int hens_pt_plan_sharded(hens_ctx* ctx, const int64_t* iperm, const int64_t* i1perm, const double* u_swap,
                         int32_t adapt, const int32_t* rank_of_rung, int32_t nranks, int32_t my_rank,
                         int64_t* send_counts, int64_t* recv_counts, uint8_t* sel_out, double* swaps_out) {
    hens_ctx_impl* c = enter(ctx);
    int r = ready(c, true);
    if (r) return r;
    if (!c->cfg.tempered || c->T < 2) return fail(c, HENS_ERR_STATE, "context is not tempered");
    if (c->expect_split != 0) return fail(c, HENS_ERR_STATE, "PT sweep between split 0 and split 1");
    if ((r = counter_room(c, 1))) return r;
    if (c->pt_pending) return fail(c, HENS_ERR_STATE, "previous sharded PT exchange not finished");
    if (!rank_of_rung || !send_counts || !recv_counts) return fail(c, HENS_ERR_INVALID, "null argument");
    if (nranks < 1 || nranks > MAX_RANKS || my_rank < 0 || my_rank >= nranks)
        return fail(c, HENS_ERR_INVALID, "nranks must be in [1, %d] and my_rank inside it", MAX_RANKS);
    const bool parity_draws = iperm != nullptr;
    if (parity_draws && (!i1perm || !u_swap)) return fail(c, HENS_ERR_INVALID, "give iperm, i1perm and u_swap together");
    const int T = c->T, W = c->W;
    for (int t = 0; t < T; ++t) {
        if (rank_of_rung[t] < 0 || rank_of_rung[t] >= nranks) return fail(c, HENS_ERR_INVALID, "rank_of_rung out of range");
        const bool mine = t >= c->cfg.rung_begin && t < c->cfg.rung_end;
        if (mine != (rank_of_rung[t] == my_rank)) return fail(c, HENS_ERR_INVALID, "rank_of_rung disagrees with this context's shard");
    }
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    if ((r = ensure_shard_buffers(c))) return r;
    if ((r = ensure_pt_buffers(c))) return r;
    const size_t PW = (size_t)(T - 1) * W;
    if (c->rank_of_host.size() != (size_t)T || memcmp(c->rank_of_host.data(), rank_of_rung, (size_t)T * 4) != 0) {
        c->rank_of_host.assign(rank_of_rung, rank_of_rung + T);
        HIPCHK(c, hipMemcpyAsync(c->d_rank_of, c->rank_of_host.data(), (size_t)T * 4, hipMemcpyHostToDevice, c->stream));
    }
    int32_t* colslot = c->colslot;
    PtArgs p = pt_args(c, colslot, true);
    p.selcol = c->selcol;
    if (parity_draws) {
        HIPCHK(c, hipMemcpyAsync(c->d_iperm, iperm, PW * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_i1perm, i1perm, PW * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->d_uswap, u_swap, PW * 8, hipMemcpyHostToDevice, c->stream));
        hipLaunchKernelGGL(k_pt_invert, dim3(grid_for(PW)), dim3(256), 0, c->stream, c->d_iperm, c->d_inv, T - 1, W);
        hipLaunchKernelGGL(k_pt_chain, dim3((W + 255) / 256), dim3(256), 0, c->stream, c->d_iperm, c->d_i1perm,
                           c->d_inv, c->d_uswap, colslot, c->colk, c->colu, T, W);
        p.colu = c->colu;
        hipLaunchKernelGGL(k_pt_cascade<false>, dim3(pt_blocks(c)), dim3(pt_threads(c->T)), pt_lds_bytes(T), c->stream, p);
        hipLaunchKernelGGL(k_pt_sel_to_korder, dim3(grid_for(PW)), dim3(256), 0, c->stream, c->selcol, c->colk,
                           c->selk, T - 1, W);
    } else {
        hipLaunchKernelGGL(k_pt_cascade<true>, dim3(pt_blocks(c)), dim3(pt_threads(c->T)), pt_lds_bytes(T), c->stream, p);
    }
    c->adapt_pending = true;
    c->adapt_pending_adaptive = adapt && c->cfg.adaptive;
    SETTLE(c, NEED_LADDER);                   // (this sweep's own counts)
    // who sends what to whom
    unsigned* counts = c->d_counts;
    HIPCHK(c, hipMemsetAsync(counts, 0, 2 * MAX_RANKS * sizeof(unsigned), c->stream));
    const int g = grid_for((int64_t)T * W);
    hipLaunchKernelGGL(k_xchg_count, dim3(g), dim3(256), 0, c->stream, c->srcglob, c->d_rank_of, T, W, (int)my_rank, counts);
    unsigned hc[2 * MAX_RANKS];
    HIPCHK(c, hipMemcpyAsync(hc, counts, sizeof hc, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned cursors[MAX_RANKS] = {0};
    int64_t nsend = 0, nrecv = 0;
    for (int q = 0; q < nranks; ++q) {
        cursors[q] = (unsigned)nsend;
        send_counts[q] = hc[q];
        recv_counts[q] = hc[MAX_RANKS + q];
        nsend += hc[q];
        nrecv += hc[MAX_RANKS + q];
    }
    if (nsend > c->row_capacity || nrecv > c->row_capacity) return fail(c, HENS_ERR_STATE, "exchange exceeds row capacity");
    unsigned* d_cursors = counts + 2 * MAX_RANKS;
    HIPCHK(c, hipMemcpyAsync(d_cursors, cursors, sizeof cursors, hipMemcpyHostToDevice, c->stream));
    if (nsend > 0) {
        hipLaunchKernelGGL(k_xchg_fill, dim3(g), dim3(256), 0, c->stream, c->srcglob, c->d_rank_of, T, W, (int)my_rank,
                           (int)c->cfg.rung_begin, d_cursors, c->send_slots, c->send_dest);
        hipLaunchKernelGGL(k_pack_rows, dim3(grid_for(nsend * (c->D + 2))), dim3(256), 0, c->stream, c->pool,
                           c->loc[c->cur], c->P[c->cur], c->send_slots, c->send_dest, c->send_rows, nsend, c->D);
    }
    HIPCHK(c, hipGetLastError());
    if (sel_out && parity_draws) HIPCHK(c, hipMemcpyAsync(sel_out, c->selk, PW, hipMemcpyDeviceToHost, c->stream));
    if (swaps_out) HIPCHK(c, hipMemcpyAsync(swaps_out, c->swaps_last, (size_t)(T - 1) * 8, hipMemcpyDeviceToHost, c->stream));
    if ((sel_out && parity_draws) || swaps_out) HIPCHK(c, hipStreamSynchronize(c->stream));   // else: packing stays async
    c->n_send = nsend; c->n_recv = nrecv;
    c->pt_pending = true;
    return HENS_OK;
}

int hens_pt_finish_sharded(hens_ctx* ctx, int64_t n_recv) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!c->pt_pending) return fail(c, HENS_ERR_STATE, "no sharded PT exchange in flight");
    if (n_recv != c->n_recv) return fail(c, HENS_ERR_INVALID, "expected %lld received rows, got %lld", (long long)c->n_recv, (long long)n_recv);
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if (n_recv > 0)
        hipLaunchKernelGGL(k_unpack_rows, dim3(grid_for(n_recv * (c->D + 2))), dim3(256), 0, c->stream, c->pool,
                           c->loc[c->cur ^ 1], c->P[c->cur ^ 1], c->recv_rows, n_recv, c->D, c->W,
                           (int)c->cfg.rung_begin, (int32_t)(c->parity * c->Tl * c->W));
    HIPCHK(c, hipGetLastError());
    c->cur ^= 1;
    c->iter += 1;
    c->pt_pending = false;
    return HENS_OK;
}

// ---- Metropolis-Hastings proposals ----------------------------------------------------------
// The teacher-forced MH entry points: the caller's payload ([Tl][W][D]: steps for hens_mh_step, points for hens_dist_step, `dist`) and
// accept uniforms go to mh_step / mh_u, the move's launch proposes from them, keep_out (and hens_dist_step's factors) are copied out.
// hens_mt_dist_step (`mt`: its pick uniforms and extra outputs; the payload is [Tl][W][K][D] in a buffer of its own) takes the same path.
struct ForcedMt { const double* u_pick; int32_t* pick_out; double* lsw_out; };
static int forced_mh_step(hens_ctx_impl* c, bool dist, const double* payload, const double* u_acc, uint8_t* keep_out, double* factors_out,
                          const ForcedMt* mt = nullptr) {
    int r = ready(c, true);
    if (r) return r;
    const char* who = mt ? "hens_mt_dist_step" : (dist ? "hens_dist_step" : "hens_mh_step");
    if (!payload || !u_acc || (mt && !mt->u_pick)) return fail(c, HENS_ERR_INVALID, "null argument");
    if (mt && c->mh_kind != MH_MT_DIST) return fail(c, HENS_ERR_STATE, "no generator set (hens_set_mt_dist_proposal)");
    if (dist && !mt && c->mh_kind != MH_DIST) return fail(c, HENS_ERR_STATE, "no generator set (hens_set_dist_proposal)");
    if (!dist && c->cfg.likelihood_kind == HENS_LIKE_HOST) return fail(c, HENS_ERR_UNSUPPORTED, "hens_mh_step needs a device likelihood");
    if (c->expect_split != 0) return fail(c, HENS_ERR_STATE, "%s between split 0 and split 1", who);
    if (c->pt_pending) return fail(c, HENS_ERR_STATE, "sharded PT exchange in flight");
    if ((r = counter_room(c, 1))) return r;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    if ((r = ensure_mh_buffers(c))) return r;
    SETTLE(c, NEED_LADDER);
    const size_t TW = (size_t)c->Tl * c->W;
    if (mt) {
        const size_t nq = TW * c->mt_K * c->D;
        if (c->mt_q_cap < nq) {                  // the tries' staging, on the first teacher-forced call (hens_step draws in the launch); an
            double* q = nullptr;                 // earlier, smaller buffer stays with the context's allocations
            if ((r = dalloc(c, &q, nq))) return r;
            c->mt_q = q;
            c->mt_q_cap = nq;
        }
        HIPCHK(c, hipMemcpyAsync(c->mt_q, payload, nq * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(c->mt_upick, mt->u_pick, TW * 8, hipMemcpyHostToDevice, c->stream));
    } else {
        HIPCHK(c, hipMemcpyAsync(c->mh_step, payload, TW * c->D * 8, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(c, hipMemcpyAsync(c->mh_u, u_acc, TW * 8, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(k_mh_prep, dim3(grid_for((int64_t)TW)), dim3(256), 0, c->stream, c->mh_u, c->mh_lu, (int64_t)TW);
    c->win_count = 0;
    if ((r = dist ? dist_launch(c, true, true, factors_out != nullptr, nullptr, mt && (mt->pick_out || mt->lsw_out)) : mh_launch(c, true, nullptr))) return r;
    if (keep_out) HIPCHK(c, hipMemcpyAsync(keep_out, c->mh_keep, TW, hipMemcpyDeviceToHost, c->stream));
    if (factors_out) HIPCHK(c, hipMemcpyAsync(factors_out, c->dist_factors, TW * 8, hipMemcpyDeviceToHost, c->stream));
    if (mt && mt->pick_out) HIPCHK(c, hipMemcpyAsync(mt->pick_out, c->mt_pick, TW * 4, hipMemcpyDeviceToHost, c->stream));
    if (mt && mt->lsw_out) HIPCHK(c, hipMemcpyAsync(mt->lsw_out, c->mt_lsw, 2 * TW * 8, hipMemcpyDeviceToHost, c->stream));
    if ((r = check_flags(c, true))) return r;
    if (!has_pt(c)) c->iter += 1;
    return HENS_OK;
}

int hens_mh_step(hens_ctx* ctx, const double* step, const double* u_acc, uint8_t* keep_out) {
    return forced_mh_step(enter(ctx), false, step, u_acc, keep_out, nullptr);
}

int hens_set_mh_proposal(hens_ctx* ctx, int32_t kind, const double* scale, double weight) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (kind < 0) {                                   // back to the stretch move only
        c->mh_kind = -1;
        c->mh_weight = 0.0;
        return HENS_OK;
    }
    if (kind > MH_FULL || !scale) return fail(c, HENS_ERR_INVALID, "kind must be 0 (isotropic), 1 (diagonal) or 2 (full) with its scale");
    if (!(weight >= 0.0 && weight <= 1.0)) return fail(c, HENS_ERR_INVALID, "weight must be a probability");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    int r = ensure_mh_buffers(c);
    if (r) return r;
    const size_t n = kind == MH_ISO ? 1 : (kind == MH_DIAG ? (size_t)c->D : (size_t)c->D * c->D);
    for (size_t i = 0; i < n; ++i)
        if (!(std::fabs(scale[i]) < INFINITY)) return fail(c, HENS_ERR_INVALID, "proposal scale must be finite");
    HIPCHK(c, hipMemcpyAsync(c->mh_scale, scale, n * 8, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mh_kind = kind;
    c->mh_weight = weight;
    return HENS_OK;
}

// ---- DistributionGenerate (distgen.py:10-104): the independence proposal in the context's one MH slot -------------------------------
// The body of hens_set_dist_proposal and hens_set_mt_dist_proposal (num_try > 0: MH_MT_DIST, `name` = "multiple-try"): one set of
// refusals, one term validation, one generator block.
static int set_generator(hens_ctx_impl* c, const char* name, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                         const double* c1, const double* c2, int num_try, double weight) {
    if (!c) return no_context();
    if (!kind || !lo || !hi || !c0 || !c1 || !c2) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!(weight >= 0.0 && weight <= 1.0)) return fail(c, HENS_ERR_INVALID, "weight must be a probability");
    if (is_rj(c)) return fail(c, HENS_ERR_UNSUPPORTED, "the %s proposal is not built for leaf-packing records", name);
    if (c->pipe.on) return fail(c, HENS_ERR_STATE, "the %s proposal is not built for a rank of the ladder pipeline", name);
    if (c->cfg.likelihood_kind == HENS_LIKE_HOST) return fail(c, HENS_ERR_UNSUPPORTED, "the %s proposal needs a device likelihood", name);
    if (c->gibbs[1].nblocks > 0) return fail(c, HENS_ERR_UNSUPPORTED, "the %s proposal is not built under Gibbs blocks on the MH slot (hens_set_gibbs(ctx, HENS_GIBBS_MH, 0, NULL) clears the table)", name);
    const LikeKernels* lk = like_kernels(c->cfg.likelihood_kind);
    if (!lk || !(num_try ? lk->mt_dist(c->D) : lk->dist(c->D)))
        return fail(c, HENS_ERR_UNSUPPORTED, "the %s proposal is built for row widths 8, 16, 32, 64 and 128 (this context's rows are %d wide)", name, c->D);
    // a distribution one draws from: finite uniform supports, as for the leaves' priors; a padded row's pads have no draw and no term
    const int D = c->D, Da = dim_active(c);
    std::vector<PriorTerm> terms((size_t)D);
    for (int d = 0; d < D; ++d) {
        const ParsedTerm p = parse_term(kind[d], lo[d], hi[d], c0[d], c1[d], c2[d], /*admit_pad=*/d >= Da);
        if (p.why[0]) return fail(c, HENS_ERR_INVALID, "%s (dim %d)", p.why, d);
        if (d >= Da && p.term.kind != PRIOR_NONE) return fail(c, HENS_ERR_INVALID, "a pad of the row takes the uniform term on (-inf, +inf) (dim %d)", d);
        terms[(size_t)d] = p.term;
    }
    SETTLE(c, NEED_DEVICE | NEED_FIELDS | NEED_LADDER);
    int r = ensure_mh_buffers(c);
    if (r) return r;
    if (!c->dist_factors) {
        double* f = nullptr;
        if ((r = dalloc(c, &f, (size_t)c->Tl * c->W))) return r;
        c->dist_factors = f;
    }
    const size_t TW = (size_t)c->Tl * c->W;
    if (num_try && !c->mt_upick) {
        if ((r = dalloc(c, &c->mt_upick, TW))) return r;
        if ((r = dalloc(c, &c->mt_pick, TW))) return r;
        if ((r = dalloc(c, &c->mt_lsw, 2 * TW))) return r;
    }
    if ((r = c->dist_block.upload(c, lo, hi, terms.data()))) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->mh_kind = num_try ? MH_MT_DIST : MH_DIST;
    c->mt_K = num_try;
    c->mh_weight = weight;
    return HENS_OK;
}

int hens_set_dist_proposal(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0, const double* c1,
                           const double* c2, double weight) {
    return set_generator(enter(ctx), "distribution", kind, lo, hi, c0, c1, c2, 0, weight);
}

// ---- MTDistGenMove(independent=True) (mtdistgen.py:7-136, multipletry.py:238-514): num_try tries per walker from the generator ------
int hens_set_mt_dist_proposal(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0, const double* c1,
                              const double* c2, int32_t num_try, double weight) {
    hens_ctx_impl* c = enter(ctx);
    if (c && (num_try < 1 || num_try > TILE)) return fail(c, HENS_ERR_INVALID, "num_try must be in [1, %d] (one tile row per try)", TILE);
    return set_generator(c, "multiple-try", kind, lo, hi, c0, c1, c2, num_try, weight);
}

// the teacher-forced twin: the caller's tries, pick uniforms and accept uniforms
int hens_mt_dist_step(hens_ctx* ctx, const double* q, const double* u_pick, const double* u_acc, uint8_t* keep_out, int32_t* pick_out,
                      double* lsw_out, double* factors_out) {
    const ForcedMt mt{u_pick, pick_out, lsw_out};
    return forced_mh_step(enter(ctx), true, q, u_acc, keep_out, factors_out, &mt);
}

// the teacher-forced twin of hens_mh_step: the caller's points and accept uniforms
int hens_dist_step(hens_ctx* ctx, const double* q, const double* u_acc, uint8_t* keep_out, double* factors_out) {
    return forced_mh_step(enter(ctx), true, q, u_acc, keep_out, factors_out);
}

int hens_get_mh_counters(hens_ctx* ctx, double* accepted, int64_t* num_proposals) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const size_t TW = (size_t)c->Tl * c->W;
    if (accepted && !c->accepted_mh) std::fill_n(accepted, TW, 0.0);
    else if (accepted)
        if (const int r = read_counters(c, TW, {{accepted, c->accepted_mh}})) return r;
    if (num_proposals) *num_proposals = c->num_proposals_mh;
    return HENS_OK;
}

// ---- ladder pipeline set-up -------------------------------------------------------------------------
int hens_pipe_init(hens_ctx* ctx, int32_t nranks, int32_t my_rank, void* blob_out, int64_t* box_bytes_out) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (c->pipe.on) return fail(c, HENS_ERR_STATE, "pipeline already initialised");
    if (c->prior) return fail(c, HENS_ERR_UNSUPPORTED, "prior terms are not built for a rank of the ladder pipeline (hens_set_prior_box returns to the box)");
    if (c->mh_kind == MH_DIST) return fail(c, HENS_ERR_UNSUPPORTED, "the distribution proposal is not built for a rank of the ladder pipeline (hens_set_mh_proposal(-1, ...) returns to the stretch move)");
    if (c->mh_kind == MH_MT_DIST) return fail(c, HENS_ERR_UNSUPPORTED, "the multiple-try proposal is not built for a rank of the ladder pipeline (hens_set_mh_proposal(-1, ...) returns to the stretch move)");
    if (gibbs_on(c)) return fail(c, HENS_ERR_UNSUPPORTED, "Gibbs blocks are not built for a rank of the ladder pipeline (hens_set_gibbs(ctx, move, 0, NULL) clears a table)");
    if (!c->cfg.tempered || c->T < 2) return fail(c, HENS_ERR_STATE, "the ladder pipeline needs a tempered ladder");
    if (nranks < 1 || nranks > PIPE_MAX_RANKS || my_rank < 0 || my_rank >= nranks)
        return fail(c, HENS_ERR_INVALID, "nranks must be in [1, %d] and my_rank inside it", PIPE_MAX_RANKS);
    if ((my_rank == 0) != (c->cfg.rung_begin == 0) || (my_rank == nranks - 1) != (c->cfg.rung_end == c->T))
        return fail(c, HENS_ERR_INVALID, "ranks must hold contiguous rung ranges in rank order (rank 0 = coldest rungs)");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const size_t bytes = pipe_box_bytes(c->T, c->W, c->D);
    void* box = nullptr;
    HIPCHK(c, hipExtMallocWithFlags(&box, bytes, hipDeviceMallocUncached));
    HIPCHK(c, hipMemsetAsync(box, 0, bytes, c->stream));
    c->pipe.box = static_cast<char*>(box);
    c->pipe.box_bytes = bytes;
    c->pipe.nranks = nranks;
    c->pipe.rank = my_rank;
    c->pipe.boxes.assign((size_t)nranks, nullptr);
    c->pipe.opened.assign((size_t)nranks, 0);
    c->pipe.boxes[my_rank] = c->pipe.box;
    int r;
    if ((r = dalloc(c, &c->pipe.Lcur, (size_t)c->W))) return r;
    if ((r = dalloc(c, &c->pipe.Pcur, (size_t)c->W))) return r;
    if ((r = dalloc(c, &c->pipe.botsrc, (size_t)c->W))) return r;
    if ((r = dalloc(c, &c->pipe.d_boxes, (size_t)nranks))) return r;
    if ((r = dalloc(c, &c->pipe.tickets, (size_t)4))) return r;
    HIPCHK(c, hipMemsetAsync(c->pipe.tickets, 0, 16, c->stream));
    {   // fused iteration (step_path decides at the first hens_step): guests' home rows, one row of swap counts per workgroup
        int cbl = 2 * TILE / std::max(1, std::min(c->Tl, 2 * TILE)), sh = 0;
        while ((1 << sh) < cbl) ++sh;
        c->pipe.cbl = 1 << sh; c->pipe.cbl_shift = sh;
        if ((r = dalloc(c, &c->pipe.ghome, (size_t)4 * c->W))) return r;
        HIPCHK(c, hipMemsetAsync(c->pipe.ghome, 0, (size_t)4 * c->W * 4, c->stream));
        const size_t words = (size_t)SWAP_ACC_ROWS_MAX * c->T;
        if ((r = dalloc(c, &c->pipe.acc[0], 2 * words))) return r;
        c->pipe.acc[1] = c->pipe.acc[0] + words;
        HIPCHK(c, hipMemsetAsync(c->pipe.acc[0], 0, 2 * words * 4, c->stream));
    }
    if (getenv("HENS_PIPE_STATS")) {
        if ((r = dalloc(c, &c->pipe.stats, (size_t)16))) return r;
        HIPCHK(c, hipMemsetAsync(c->pipe.stats, 0, 128, c->stream));
    }
    int khz = 0;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, c->cfg.device_id);
    c->pipe.budget = (long long)((khz > 0 ? khz : 100000) * 1000.0 * env().pipe_timeout_s);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (blob_out) {       // [mailbox handle | pool handle]
        hipIpcMemHandle_t h[2];
        HIPCHK(c, hipIpcGetMemHandle(&h[0], box));
        HIPCHK(c, hipIpcGetMemHandle(&h[1], c->pool));
        static_assert(sizeof(h) == HENS_PIPE_BLOB_BYTES, "IPC blob size");
        memcpy(blob_out, h, sizeof h);
    }
    if (box_bytes_out) *box_bytes_out = (int64_t)bytes;
    c->pipe.on = true;
    return HENS_OK;
}

static int pipe_finish_connect(hens_ctx_impl* c) {
    for (int q = 0; q < c->pipe.nranks; ++q)
        if (!c->pipe.boxes[q]) return fail(c, HENS_ERR_STATE, "mailbox of rank %d missing", q);
    HIPCHK(c, hipMemcpyAsync(c->pipe.d_boxes, c->pipe.boxes.data(), (size_t)c->pipe.nranks * sizeof(char*),
                             hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pipe.connected = true;
    return HENS_OK;
}

int hens_pipe_connect(hens_ctx* ctx, const void* blobs) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !blobs) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!c->pipe.on) return fail(c, HENS_ERR_STATE, "hens_pipe_init first");
    if (c->pipe.connected) return fail(c, HENS_ERR_STATE, "pipeline already connected");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const char* hb = static_cast<const char*>(blobs);
    for (int q = 0; q < c->pipe.nranks; ++q) {
        if (q == c->pipe.rank) continue;
        hipIpcMemHandle_t h[2];
        memcpy(h, hb + (size_t)q * sizeof h, sizeof h);
        void* p = nullptr;
        HIPCHK(c, hipIpcOpenMemHandle(&p, h[0], hipIpcMemLazyEnablePeerAccess));
        c->pipe.boxes[q] = static_cast<char*>(p);
        c->pipe.opened[q] = 1;
        if (q == c->pipe.rank - 1) {          // rows that move up are pulled out of the cold neighbour's pool
            void* pp = nullptr;
            HIPCHK(c, hipIpcOpenMemHandle(&pp, h[1], hipIpcMemLazyEnablePeerAccess));
            c->pipe.pool_cold = static_cast<const double*>(pp);
            c->pipe.pool_cold_opened = true;
        }
    }
    return pipe_finish_connect(c);
}

// ---- staged transport: the same protocol with RCCL send/recv between the launches ---------------------
// The kernels are unchanged; they store into LOCAL outboxes laid out like the peers' mailboxes, and the caller
// (eryn_amd.ladder.StagedPipeline: torch.distributed point-to-point = grouped ncclSend/ncclRecv on ROCm) moves
// the message regions between the stages.  RCCL cannot pull, so the LDN message carries the boundary rung's rows.
int hens_pipe_connect_staged(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!c->pipe.on) return fail(c, HENS_ERR_STATE, "hens_pipe_init first");
    if (c->pipe.connected) return fail(c, HENS_ERR_STATE, "pipeline already connected");
    if (c->cfg.adaptation_delay != 0) return fail(c, HENS_ERR_UNSUPPORTED, "the staged transport runs the reference's adaptation schedule");
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    const size_t bytes = c->pipe.box_bytes;
    int r;
    if ((r = dalloc(c, &c->pipe.out_hot, bytes))) return r;
    if ((r = dalloc(c, &c->pipe.out_cold, bytes))) return r;
    const size_t cnt_bytes = (size_t)(reinterpret_cast<char*>(pipe_box(nullptr, c->T, c->W, c->D).counts) - static_cast<char*>(nullptr)) +
                             pipe_round((size_t)4 * c->T * 4);        // a mailbox prefix: flags .. counts
    if ((r = dalloc(c, &c->pipe.out_cnt, cnt_bytes))) return r;
    if ((r = dalloc(c, &c->pipe.ldn_rows, (size_t)2 * c->W * c->D))) return r;
    HIPCHK(c, hipMemsetAsync(c->pipe.out_cnt, 0, cnt_bytes, c->stream));
    std::vector<char*> table((size_t)c->pipe.nranks, c->pipe.out_cnt);       // the walk kernel's count puts
    for (int q = 0; q < c->pipe.nranks; ++q)
        c->pipe.boxes[q] = q == c->pipe.rank + 1 ? c->pipe.out_hot : (q == c->pipe.rank - 1 ? c->pipe.out_cold : c->pipe.out_cnt);
    c->pipe.boxes[c->pipe.rank] = c->pipe.box;
    HIPCHK(c, hipMemcpyAsync(c->pipe.d_boxes, table.data(), table.size() * sizeof(char*), hipMemcpyHostToDevice, c->stream));
    // the bottom kernel "pulls" out of pool_cold at row meta[par] + slot: here the received copy of the rung
    c->pipe.pool_cold = c->pipe.ldn_rows;
    const long long meta[2] = {0, (long long)c->W};
    const PipeBox me = pipe_box(c->pipe.box, c->T, c->W, c->D);
    HIPCHK(c, hipMemcpyAsync(me.meta, meta, sizeof meta, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->pipe.staged = true;
    c->pipe.connected = true;
    return HENS_OK;
}

int hens_pipe_regions(hens_ctx* ctx, hens_pipe_region_table* out) {
    hens_ctx_impl* c = enter(ctx);
    return pipe_regions_impl(c, out);
}
static int pipe_regions_impl(hens_ctx_impl* c, hens_pipe_region_table* out) {
    if (!c || !out) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!c->pipe.staged) return fail(c, HENS_ERR_STATE, "hens_pipe_connect_staged first");
    const int W = c->W, D = c->D, T = c->T, par = (int)(c->pipe.sweep & 1u);
    const PipeBox me = pipe_box(c->pipe.box, T, W, D);
    const PipeBox oh = pipe_box(c->pipe.out_hot, T, W, D), oc = pipe_box(c->pipe.out_cold, T, W, D);
    const PipeBox on = pipe_box(c->pipe.out_cnt, T, W, D);
    // the rows of my hottest rung after THIS iteration's move: home `parity` before the move flips it
    out->ldn_out = oh.lp_dn + (size_t)par * 2 * W;
    out->ldn_rows_out = c->pool + ((size_t)c->parity * c->Tl * W + (size_t)(c->Tl - 1) * W) * D;
    out->ldn_in = me.lp_dn + (size_t)par * 2 * W;
    out->ldn_rows_in = c->pipe.ldn_rows + (size_t)par * W * D;
    out->lup_out = oc.lp_up + (size_t)par * 2 * W;
    out->lup_in = me.lp_up + (size_t)par * 2 * W;
    out->rows_out = oc.guest + (size_t)(par * 2) * W * D;
    out->rows_in = me.guest + (size_t)(par * 2) * W * D;
    out->cnt_out = on.counts + (size_t)(c->pipe.sweep & 3u) * T;
    out->cnt_in = me.counts + (size_t)(c->pipe.sweep & 3u) * T;
    out->lp_doubles = 2 * (int64_t)W;
    out->row_doubles = (int64_t)W * D;
    out->cnt_words = T;
    out->stream = c->stream;
    return HENS_OK;
}

int hens_pipe_stage(hens_ctx* ctx, int32_t stage) {
    hens_ctx_impl* c = enter(ctx);
    return pipe_stage_impl(c, stage);
}
static int pipe_stage_impl(hens_ctx_impl* c, int32_t stage) {
    int r = ready(c, true);
    if (r) return r;
    if (!c->pipe.staged) return fail(c, HENS_ERR_STATE, "hens_pipe_connect_staged first");
    if ((r = counter_room(c, 1))) return r;
    SETTLE(c, NEED_DEVICE | NEED_FIELDS);
    switch (stage) {
        case 0: {           // the iteration's move (stretch halves or the MH proposal); publishes (L, P) of the boundary rung
            c->N0 = (c->W + 1) / 2;
            if (!(c->iter >= c->win_from && c->iter < c->win_from + (uint64_t)c->win_count)) {
                launch_plan(c, c->stream, 0, c->iter, c->NB);
                c->win_from = c->iter;
                c->win_count = c->NB;
            }
            if (iteration_is_mh(c)) r = mh_iteration(c, nullptr);
            else r = stretch_pair(c, 0, (int)(c->iter - c->win_from), nullptr);
            if (r) return r;
            pipe_launch_pub(c);
            break;
        }
        case 1: {           // after LDN (from below) and LUP (from above) have been received
            const PipeBox on = pipe_box(c->pipe.out_cnt, c->T, c->W, c->D);
            HIPCHK(c, hipMemsetAsync(on.counts + (size_t)(c->pipe.sweep & 3u) * c->T, 0, (size_t)c->T * 4, c->stream));
            pipe_launch_walk(c);
            break;
        }
        case 2:             // decides the bottom pair, settles my coldest rung, fills the rows that go down
            pipe_launch_bottom(c);
            pipe_finish_sweep(c);
            c->iter += 1;
            break;
        default:
            return fail(c, HENS_ERR_INVALID, "stage must be 0 (move), 1 (walk) or 2 (bottom)");
    }
    HIPCHK(c, hipGetLastError());
    return HENS_OK;
}

// Communicator of a ladder shard.  unique_id: NCCL_UNIQUE_ID_BYTES (128) from hens_comm_unique_id on ONE rank,
// handed to the others by the caller (torch.distributed broadcast, MPI, a file ...); every rank calls hens_comm_init with the same
// id - the call is collective.  The context becomes a rank of the staged pipeline whose messages the library sends itself.
int hens_comm_unique_id(void* out) {
    RcclApi& R = rccl_api();
    if (!R.ok) return fail(nullptr, HENS_ERR_UNSUPPORTED, "RCCL is not available: %s", R.err.c_str());
    if (!out) return fail(nullptr, HENS_ERR_INVALID, "null argument");
    ncclUniqueId id;
    const ncclResult_t n = R.GetUniqueId(&id);
    if (n != ncclSuccess) return fail(nullptr, HENS_ERR_HIP, "ncclGetUniqueId failed: %s", R.GetErrorString(n));
    memcpy(out, &id, sizeof id);
    return HENS_OK;
}
int hens_comm_init(hens_ctx* ctx, int32_t nranks, int32_t rank, const void* unique_id) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !unique_id) return fail(c, HENS_ERR_INVALID, "null argument");
    RcclApi& R = rccl_api();
    if (!R.ok) return fail(c, HENS_ERR_UNSUPPORTED, "RCCL is not available: %s", R.err.c_str());
    if (c->comm_on) return fail(c, HENS_ERR_STATE, "the context already has a communicator");
    int r;
    int64_t nbytes = 0;
    if (!c->pipe.on && (r = hens_pipe_init(ctx, nranks, rank, nullptr, &nbytes))) return r;
    if (!c->pipe.connected && (r = hens_pipe_connect_staged(ctx))) return r;
    if (!c->pipe.staged) return fail(c, HENS_ERR_STATE, "the context is connected to the one-sided pipeline already");
    SETTLE(c, NEED_DEVICE);
    ncclUniqueId id;
    memcpy(&id, unique_id, sizeof id);
    ncclComm_t comm = nullptr;
    RCCLCHK(c, R.CommInitRank(&comm, nranks, id, rank));
    c->comm = comm;
    c->comm_on = true;
    return HENS_OK;
}
int hens_comm_destroy(hens_ctx* ctx) {
    hens_ctx_impl* c = enter(ctx);
    if (!c) return no_context();
    if (!c->comm_on) return HENS_OK;
    (void)hipStreamSynchronize(c->stream);
    RcclApi& R = rccl_api();
    RCCLCHK(c, R.CommDestroy(static_cast<ncclComm_t>(c->comm)));
    c->comm = nullptr;
    c->comm_on = false;
    return HENS_OK;
}
// dev aid / one-GPU test of the transport: `n` doubles from src to dst through ncclSend / ncclRecv to MYSELF (one grouped call on
// the context's stream; RCCL allows a rank to send to itself inside a group)
int hens_comm_selfsend(hens_ctx* ctx, int64_t n, const double* src_host, double* dst_host) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !src_host || !dst_host || n <= 0) return fail(c, HENS_ERR_INVALID, "bad argument");
    if (!c->comm_on) return fail(c, HENS_ERR_STATE, "hens_comm_init first");
    RcclApi& R = rccl_api();
    SETTLE(c, NEED_DEVICE);
    double *a = nullptr, *b = nullptr;
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&a), (size_t)n * 8));
    HIPCHK(c, hipMalloc(reinterpret_cast<void**>(&b), (size_t)n * 8));
    int rc = HENS_OK;
    do {
        if (hipMemcpyAsync(a, src_host, (size_t)n * 8, hipMemcpyHostToDevice, c->stream) != hipSuccess) { rc = fail(c, HENS_ERR_HIP, "copy in"); break; }
        (void)hipMemsetAsync(b, 0, (size_t)n * 8, c->stream);
        ncclComm_t comm = static_cast<ncclComm_t>(c->comm);
        ncclResult_t e1 = R.GroupStart(), e2 = R.Send(a, (size_t)n, ncclDouble, c->pipe.rank, comm, c->stream),
                     e3 = R.Recv(b, (size_t)n, ncclDouble, c->pipe.rank, comm, c->stream), e4 = R.GroupEnd();
        for (ncclResult_t e : {e1, e2, e3, e4}) if (e != ncclSuccess) { rc = fail(c, HENS_ERR_HIP, "RCCL self send / recv: %s", R.GetErrorString(e)); break; }
        if (rc) break;
        if (hipMemcpyAsync(dst_host, b, (size_t)n * 8, hipMemcpyDeviceToHost, c->stream) != hipSuccess) { rc = fail(c, HENS_ERR_HIP, "copy out"); break; }
        if (hipStreamSynchronize(c->stream) != hipSuccess) { rc = fail(c, HENS_ERR_HIP, "stream synchronisation after the self send"); break; }
    } while (0);
    (void)hipFree(a); (void)hipFree(b);
    return rc;
}

// ---- pipeline self-test --------------------------------------------------------------------------------
// Run in a throw-away process per rank BEFORE the real connect (eryn_amd.ladder does): a node where peer
// mappings do not work shows up here as an error code or a dead helper process, not as a GPU fault in the
// sampler.  Ranks find each other through files in `dir`.  Checks, with the rank's ladder neighbours:
//   put   - kernel stores into the neighbour's uncached mailbox-like buffer + flag, neighbour sees the data
//   pull  - kernel reads the neighbour's ordinary (cached) device memory written with system-scope stores
static bool wait_for_file(const std::string& path, double timeout_s) {
    const auto t0 = std::chrono::steady_clock::now();
    while (access(path.c_str(), R_OK) != 0) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > timeout_s) return false;
        usleep(2000);
    }
    return true;
}

int hens_pipe_selftest(int32_t device_id, int32_t rank, int32_t nranks, const char* dir, double timeout_s) {
    if (!dir || rank < 0 || rank >= nranks) return fail(nullptr, HENS_ERR_INVALID, "bad self-test arguments");
    hens_ctx_impl* c = nullptr;
    HIPCHK(c, hipSetDevice(device_id));
    constexpr int N = 4096;
    double* ubuf = nullptr; unsigned* uflag = nullptr; double* cbuf = nullptr; unsigned* result = nullptr;
    HIPCHK(c, hipExtMallocWithFlags((void**)&ubuf, N * 8, hipDeviceMallocUncached));
    HIPCHK(c, hipExtMallocWithFlags((void**)&uflag, 256, hipDeviceMallocUncached));
    HIPCHK(c, hipMalloc((void**)&cbuf, N * 8));
    HIPCHK(c, hipMalloc((void**)&result, 4));
    HIPCHK(c, hipMemset(ubuf, 0, N * 8));
    HIPCHK(c, hipMemset(uflag, 0, 256));
    HIPCHK(c, hipMemset(result, 0, 4));
    hipLaunchKernelGGL(k_probe_fill, dim3(1), dim3(256), 0, nullptr, cbuf, N, 7000.0 + rank);   // what my hot neighbour will pull
    HIPCHK(c, hipDeviceSynchronize());
    hipIpcMemHandle_t h[3];
    HIPCHK(c, hipIpcGetMemHandle(&h[0], ubuf));
    HIPCHK(c, hipIpcGetMemHandle(&h[1], uflag));
    HIPCHK(c, hipIpcGetMemHandle(&h[2], cbuf));
    const std::string base(dir);
    {
        const std::string tmp = base + "/h" + std::to_string(rank) + ".tmp", fin = base + "/h" + std::to_string(rank) + ".bin";
        FILE* f = fopen(tmp.c_str(), "wb");
        if (!f) return fail(nullptr, HENS_ERR_INVALID, "cannot write %s", tmp.c_str());
        fwrite(h, sizeof h, 1, f);
        fclose(f);
        rename(tmp.c_str(), fin.c_str());
    }
    auto read_handles = [&](int q, hipIpcMemHandle_t* out) -> bool {
        const std::string p = base + "/h" + std::to_string(q) + ".bin";
        if (!wait_for_file(p, timeout_s)) return false;
        FILE* f = fopen(p.c_str(), "rb");
        if (!f) return false;
        const bool ok = fread(out, sizeof(hipIpcMemHandle_t) * 3, 1, f) == 1;
        fclose(f);
        return ok;
    };
    const bool has_hot = rank + 1 < nranks, has_cold = rank > 0;
    double* hot_ubuf = nullptr; unsigned* hot_uflag = nullptr; double* cold_cbuf = nullptr;
    if (has_hot) {           // I put into my hot neighbour's buffer (like the LDN / ROWS messages going up)
        hipIpcMemHandle_t g[3];
        if (!read_handles(rank + 1, g)) return fail(nullptr, HENS_ERR_STATE, "self-test: rank %d never published its handles", rank + 1);
        HIPCHK(c, hipIpcOpenMemHandle((void**)&hot_ubuf, g[0], hipIpcMemLazyEnablePeerAccess));
        HIPCHK(c, hipIpcOpenMemHandle((void**)&hot_uflag, g[1], hipIpcMemLazyEnablePeerAccess));
    }
    if (has_cold) {          // I pull out of my cold neighbour's cached memory (like the rows that move up)
        hipIpcMemHandle_t g[3];
        if (!read_handles(rank - 1, g)) return fail(nullptr, HENS_ERR_STATE, "self-test: rank %d never published its handles", rank - 1);
        HIPCHK(c, hipIpcOpenMemHandle((void**)&cold_cbuf, g[2], hipIpcMemLazyEnablePeerAccess));
    }
    if (has_hot) hipLaunchKernelGGL(k_probe_put, dim3(1), dim3(256), 0, nullptr, hot_ubuf, hot_uflag, N, 100.0 * (rank + 1));
    int khz = 0;
    (void)hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, device_id);
    const long long budget = (long long)((khz > 0 ? khz : 100000) * 1000.0 * timeout_s);
    hipLaunchKernelGGL(k_probe_check, dim3(1), dim3(256), 0, nullptr, uflag, ubuf, cold_cbuf, N, 100.0 * rank,
                       7000.0 + (rank - 1), has_cold ? 1 : 0, has_cold ? 1 : 0, budget, result);
    HIPCHK(c, hipDeviceSynchronize());
    unsigned res = 0;
    HIPCHK(c, hipMemcpy(&res, result, 4, hipMemcpyDeviceToHost));
    // keep my memory alive until the neighbours are done with it
    { FILE* f = fopen((base + "/done" + std::to_string(rank)).c_str(), "w"); if (f) fclose(f); }
    for (int q : {rank - 1, rank + 1})
        if (q >= 0 && q < nranks) (void)wait_for_file(base + "/done" + std::to_string(q), timeout_s);
    if (hot_ubuf) (void)hipIpcCloseMemHandle(hot_ubuf);
    if (hot_uflag) (void)hipIpcCloseMemHandle(hot_uflag);
    if (cold_cbuf) (void)hipIpcCloseMemHandle(cold_cbuf);
    (void)hipFree(ubuf); (void)hipFree(uflag); (void)hipFree(cbuf); (void)hipFree(result);
    if (res & FLAG_PIPE_TIMEOUT) return fail(nullptr, HENS_ERR_STATE, "self-test: the flag of the cold neighbour never arrived");
    if (res >> 8) return fail(nullptr, HENS_ERR_STATE, "self-test: wrong data (put %u, pull %u)", (res >> 8) & 1u, (res >> 9) & 1u);
    return HENS_OK;
}

int hens_pipe_debug_stats(hens_ctx* ctx, uint64_t* out16, int32_t reset) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !out16) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!c->pipe.stats) return fail(c, HENS_ERR_STATE, "set HENS_PIPE_STATS=1 before hens_pipe_init");
    SETTLE(c, NEED_DEVICE);
    HIPCHK(c, hipMemcpyAsync(out16, c->pipe.stats, 128, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(c, hipMemsetAsync(c->pipe.stats, 0, 128, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return HENS_OK;
}

int hens_pipe_connect_local(hens_ctx* ctx, hens_ctx* const* peers) {
    hens_ctx_impl* c = enter(ctx);
    if (!c || !peers) return fail(c, HENS_ERR_INVALID, "null argument");
    if (!c->pipe.on) return fail(c, HENS_ERR_STATE, "hens_pipe_init first");
    if (c->pipe.connected) return fail(c, HENS_ERR_STATE, "pipeline already connected");
    for (int q = 0; q < c->pipe.nranks; ++q) {
        const hens_ctx_impl* o = CTX(peers[q]);
        if (!o || !o->pipe.on || o->pipe.rank != q || o->pipe.nranks != c->pipe.nranks || o->T != c->T || o->W != c->W ||
            o->D != c->D)
            return fail(c, HENS_ERR_INVALID, "peer %d is not an initialised pipeline context of the same ladder", q);
        c->pipe.boxes[q] = o->pipe.box;
        if (q == c->pipe.rank - 1) c->pipe.pool_cold = o->pool;
    }
    return pipe_finish_connect(c);
}

}  // extern "C"
