/*
 * hipensemble.h - C ABI of libhipensemble.so, an MI355X (gfx950) native stepping
 * engine for Eryn's walker-parallel stretch move + parallel-tempering path.
 *
 * The reference (mikekatz04/Eryn v1.2.6) is pure Python and has no FFI for this
 * path; its plugin boundary is the Python `Move.propose(model, state)` protocol.
 * Each entry point below therefore cites the reference *Python* interface it
 * replaces (paths relative to /root/reference/src/eryn).  The Python side of the
 * boundary (eryn_amd/moves/stretch.py, eryn_amd/moves/tempering.py) binds these
 * with ctypes; INTEGRATION.md shows the stub an Eryn maintainer would add.
 *
 * Conventions
 *   - every function returns an hens_status (0 = ok, < 0 = error);
 *     hens_last_error(ctx) gives the message (ctx may be NULL after a failed
 *     hens_create).
 *   - host buffers are caller-owned, C-contiguous, little-endian; the library
 *     copies and never retains host pointers.
 *   - layouts are the reference's, with nleaves_max == 1 squeezed away:
 *       x[ntemps][nwalkers][ndim] f64, logl/logp[ntemps][nwalkers] f64,
 *       betas[ntemps] f64.  A context that owns the ladder shard
 *       [rung_begin, rung_end) exchanges only those rungs (Tl = rung_end -
 *       rung_begin rows) through x/logl/logp; betas is always the full ladder.
 *   - one host thread per context; no callbacks into the caller.
 */
#ifndef HIPENSEMBLE_H
#define HIPENSEMBLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hens_ctx hens_ctx;

typedef enum hens_status {
    HENS_OK = 0,
    HENS_ERR_INVALID = -1,          /* bad argument / shape            -> ValueError   */
    HENS_ERR_HIP = -2,              /* HIP runtime failure             -> RuntimeError */
    HENS_ERR_STATE = -3,            /* call order / missing setup      -> RuntimeError */
    HENS_ERR_TOO_FEW_WALKERS = -4,  /* red_blue.py:108-114             -> RuntimeError */
    HENS_ERR_NONFINITE = -5,        /* ensemble.py:1258-1262,1541-1542 -> ValueError   */
    HENS_ERR_UNSUPPORTED = -6       /* feature outside the hot path    -> NotImplementedError */
} hens_status;

typedef enum hens_likelihood {
    HENS_LIKE_GAUSS_DENSE = 0,      /* -0.5 (x-mu)^T P (x-mu), tests/test_eryn.py:33-35 */
    HENS_LIKE_GAUSS_DIAG = 1,       /* same with diagonal precision (test_base's identity covariance) */
    HENS_LIKE_ROSENBROCK = 2,       /* -(sum b (x[i+1]-x[i]^2)^2 + (a-x[i])^2), BASELINE config 5 */
    HENS_LIKE_HOST = 3,             /* arbitrary caller-side log_like_fn: hens_propose_split / hens_accept_split */
    HENS_LIKE_TEMPLATE = 4          /* variable-dimension template model on leaf-packing records: hens_rj_*  */
} hens_likelihood;

/* Construction parameters.  Mirrors the keyword arguments that reach the path:
 * EnsembleSampler(nwalkers, ndims, ...)           ensemble.py:211-247
 * StretchMove(a=2.0, live_dangerously=False)      moves/stretch.py:37, moves/red_blue.py:41-47
 * TemperatureControl(adaptive, adaptation_lag,    moves/tempering.py:242-255
 *                    adaptation_time, stop_adaptation)
 * fill_zero_leaves_val = -1e300                   ensemble.py:242,1486-1513          */
typedef struct hens_config {
    int32_t ntemps;            /* full ladder length T                                   */
    int32_t nwalkers;          /* W                                                      */
    int32_t ndim;              /* D                                                      */
    int32_t rung_begin;        /* ladder shard owned by this context: [rung_begin,       */
    int32_t rung_end;          /*   rung_end); 0, ntemps for a single GPU                */
    int32_t device_id;         /* HIP device ordinal                                     */
    int32_t likelihood_kind;   /* hens_likelihood                                        */
    int32_t tempered;          /* 0: logP = logl + logp (move.py:443-457); 1: betas      */
    int32_t live_dangerously;  /* skip the W >= 2 D guard (red_blue.py:108-114)          */
    int32_t adaptive;          /* ladder adaptation on (tempering.py:632-633)            */
    int32_t adaptation_delay;  /* ladder pipeline only: 0 = the reference's schedule (the swap ratios of sweep s move the
                                * ladder before iteration s+1 - every rank then waits for the whole cascade);
                                * 1 = they move it before iteration s+2, which lets the ranks pipeline          */
    int32_t ndim_active;       /* 0: = ndim.  Otherwise the number of REAL parameters in rows that the caller padded to a
                                * width the compile-time-width kernels serve (8, 16, 32, 64, 128): the pads hold zeros,
                                * lie in a (-inf, +inf) prior interval and meet zero rows / columns of the precision
                                * matrix, so they never change; only the Hastings factor (ndim - 1) log zz
                                * (stretch.py:223) and the W >= 2 ndim guard (red_blue.py:108-114) count real
                                * parameters.  eryn_amd.engine.HipEnsemble pads on upload and strips on download. */
    int64_t stop_adaptation;   /* < 0: never stop (tempering.py:591)                     */
    double a;                  /* stretch scale                                          */
    double fill_value;         /* likelihood of walkers outside the prior support        */
    double adaptation_lag;     /* 10000                                                  */
    double adaptation_time;    /* 100                                                    */
    uint64_t seed;             /* Philox key for hens_step                               */
} hens_config;

/* Lifetime.  Replaces: State / Branch buffer allocation (state.py:330-562). */
int hens_create(const hens_config* cfg, hens_ctx** out);
void hens_destroy(hens_ctx* ctx);
const char* hens_last_error(const hens_ctx* ctx);
int hens_synchronize(hens_ctx* ctx);

/* Model constants.
 * hens_set_prior_box: ProbDistContainer({i: uniform_dist(lo_i, hi_i)}) (prior.py:12-91,
 *   337-392).  logp_inside is sum_d log(1/(hi_d-lo_d)) accumulated by the caller in the
 *   reference's order, so an in-support prior value is bit-identical.
 * hens_set_gaussian: the (mu, invcov) `args` of the reference tests' log_like_fn
 *   (tests/test_eryn.py:33-35,100-104).  prec has D*D entries (dense) or D (diag).
 * hens_set_rosenbrock: constants of the config-5 stress likelihood. */
int hens_set_prior_box(hens_ctx* ctx, const double* lo, const double* hi, double logp_inside);
/* hens_set_prior_terms: ProbDistContainer({i: dist_i}) with one independent distribution per parameter (prior.py:337-392:
 *   the terms are added in ascending parameter order from 0.0; a parameter outside its support gives -inf).  Per
 *   parameter d: kind[d] (hens_prior_kind), the inclusive support [lo[d], hi[d]] and three constants formed by the caller
 *   (so that every value that meets a proposal is the caller's own double):
 *     HENS_PRIOR_UNIFORM      term c0[d] = log(1/(hi - lo)) (prior.py:28-41,80-88); c1, c2 are not read.  lo = -inf with
 *                             hi = +inf is the inert interval of a padded row (hens_config::ndim_active): no term at all
 *     HENS_PRIOR_LOG_UNIFORM  term (-log(q)) - c0[d], c0 = log(log(hi) - log(lo)) (scipy.stats.loguniform(lo, hi),
 *                             prior.py:115-136); needs 0 < lo; c1, c2 are not read
 *     HENS_PRIOR_NORMAL       term (-(y y)/2 - log(sqrt(2 pi))) - c2[d] with y = (q - c0[d]) / c1[d]: scipy.stats.norm(
 *                             loc = c0, scale = c1 > 0), c2 = log(c1); its support is every finite q: pass lo = -inf,
 *                             hi = +inf
 *   Uniform kinds only: the call IS hens_set_prior_box(lo, hi, sum of the c0 in ascending order) - same launches, same
 *   chain.  With another kind among them every entry point evaluates the sum per proposal - k_stretch_prior at the row
 *   widths 8 / 16 / 32 / 64 / 128, the generic-width k_stretch otherwise and with periodic parameters (hens_step: the copying
 *   launches, then the cascade and the adaptation as kernels of their own), hens_accept_split's decision kernel; the record /
 *   one-launch / persistent kernels are not used.  A normal term that is not finite (|q - loc| beyond about 1e154 scales: y y
 *   overflows) counts as outside the support: log-prior -inf, the likelihood skipped and filled.  Refused on a
 *   leaf-packing context (HENS_ERR_UNSUPPORTED: its leaves take their terms through hens_rj_set_prior_terms) and on a rank of the ladder pipeline (HENS_ERR_STATE; hens_pipe_init
 *   after it: HENS_ERR_UNSUPPORTED).  hens_set_prior_box afterwards returns the context to the box. */
typedef enum hens_prior_kind {
    HENS_PRIOR_UNIFORM = 0,
    HENS_PRIOR_LOG_UNIFORM = 1,
    HENS_PRIOR_NORMAL = 2
} hens_prior_kind;
int hens_set_prior_terms(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                         const double* c1, const double* c2);
/* hens_set_periodic: the `periodic` argument of EnsembleSampler / Move (ensemble.py:165-168,338-347,528-536; a
 *   PeriodicContainer, utils/periodic.py:11-151) for the single branch: period[d] > 0 makes parameter d periodic - the
 *   stretch move measures c - s the short way round (stretch.py:136-141 -> periodic.py:49-116) and every proposal is
 *   wrapped into [0, period) with NumPy's remainder (stretch.py:149-154, gaussian.py:110-115 -> periodic.py:118-151);
 *   0 = not periodic; NULL or all zeros = no periodic parameters.  Every entry point honours it (the one- and two-launch
 *   iterations' compile-time-width kernels and the generic-width kernel alike, and the ranks of a ladder pipeline - set it
 *   on every rank BEFORE hens_pipe_init); not available on a leaf-packing context (HENS_ERR_UNSUPPORTED), whose periods go per branch
 *   and leaf parameter: hens_rj_set_periodic. */
int hens_set_periodic(hens_ctx* ctx, const double* period);
int hens_set_gaussian(hens_ctx* ctx, const double* mu, const double* prec);
int hens_set_rosenbrock(hens_ctx* ctx, double a, double b);

/* State transfer.  Replaces State(coords, log_like=, log_prior=, betas=) construction and
 * the State snapshot handed to Backend.save_step (state.py:437-517, backends/backend.py:1014-1091).
 * Any output pointer may be NULL.  logl/logp NULL on upload = "not evaluated yet". */
int hens_upload_state(hens_ctx* ctx, const double* x, const double* logl, const double* logp,
                      const double* betas);
int hens_download_state(hens_ctx* ctx, double* x, double* logl, double* logp, double* betas);

/* Initial log-prior / log-likelihood of the resident coordinates.
 * Replaces EnsembleSampler.compute_log_prior + compute_log_like as called from
 * sample() (ensemble.py:898-912; 1127-1217; 1219-1545 incl. the -inf-prior skip and
 * the fill value).  Returns HENS_ERR_NONFINITE if a coordinate is inf/NaN. */
int hens_eval_state(hens_ctx* ctx);

/* One red/blue half-step on all resident rungs, driven by caller-supplied draws
 * ("parity mode").  Replaces one trip of the `for split in range(nsplits)` body of
 * RedBlueMove.propose (red_blue.py:148-323): StretchMove.get_proposal (stretch.py:160-231),
 * compute_log_prior, compute_log_like, the MH test (red_blue.py:292-294) and Move.update
 * (move.py:472-703).
 *   labels[Tl][W]   u8   split label of every walker after the reference's shuffle (red_blue.py:121-124)
 *   rint[Tl][Ns]    i64  R.randint(Nc, size=(T, Ns))                  (stretch.py:93-99)
 *   u_zz[Tl][Ns]    f64  R.rand(T, Ns) for the stretch factor         (stretch.py:129-132)
 *   u_acc[Tl][Ns]   f64  R.rand(T, Ns) for the accept test            (red_blue.py:294)
 *   keep_out[Tl][Ns] u8  accept mask in the order of the ascending moving set S
 * Calls must alternate split = 0, 1.  Synchronous. */
int hens_stretch_split(hens_ctx* ctx, int32_t split, const uint8_t* labels, const int64_t* rint,
                       const double* u_zz, const double* u_acc, uint8_t* keep_out);

/* Number of sets of the red-blue move the parity API runs (`RedBlueMove(nsplits=...)`, red_blue.py:41-47,148: walker w of a rung
 * starts in set w % nsplits, shuffled per rung; set k moves against the other sets concatenated in set order, stretch.py:199).
 * Default 2.  With nsplits = n the split calls of one move run 0 .. n-1 in order, labels take values in [0, n), set k holds
 * ceil((W - k) / n) walkers and rint indexes the W - that many others.  hens_step draws the n sets itself (labels = a keyed
 * permutation mod n; round 4), except on a ladder shard, which keeps two sets. */
/* StretchMove.a as a mutable attribute (stretch.py:37; the reference's tuning hook mutates move.a, utils/updates.py:130-175):
 * the scale of every proposal made after the call, in both RNG modes. */
int hens_set_stretch_scale(hens_ctx* ctx, double a);
int hens_set_nsplits(hens_ctx* ctx, int32_t nsplits);

/* Host-callable likelihood (contexts created with HENS_LIKE_HOST).  The half-step of
 * hens_stretch_split is cut in two around the caller's log_like_fn (ensemble.py:1219-1545,
 * 1623-1667): hens_propose_split returns the proposed points q[Tl][Ns][D] and inbox[Tl][Ns]
 * (1 = inside the prior box; walkers with 0 must not be evaluated and get the fill value,
 * ensemble.py:1279-1282,1486-1513); hens_accept_split takes logl[Tl][Ns] and the accept uniforms and
 * performs the MH test and Move.update on the device.  Same alternation rule as hens_stretch_split;
 * hens_eval_state on such a context fills log_prior only.  hens_step is not available. */
int hens_propose_split(hens_ctx* ctx, int32_t split, const uint8_t* labels, const int64_t* rint,
                       const double* u_zz, double* q_out, uint8_t* inbox_out);
int hens_accept_split(hens_ctx* ctx, int32_t split, const double* logl, const double* u_acc,
                      uint8_t* keep_out);

/* Hot->cold swap cascade + ladder adaptation, driven by caller-supplied draws.
 * Replaces TemperatureControl.temper_comps (tempering.py:598-649): temperature_swaps
 * (:484-561), do_swaps_indexing (:351-482), adapt_temps (:585-596).
 *   iperm, i1perm [T-1][W] i64; u_swap [T-1][W] f64: row j holds the draws of the pair
 *   (i, i-1), i = T-1-j, i.e. the order np.random.permutation / uniform are called.
 *   adapt: 0 = swaps only (rj.py:381-382 calls temper_comps(adapt=False)).
 *   sel_out [T-1][W] u8 (same row order), swaps_accepted_out [T-1] indexed by i-1.
 * Requires the whole ladder resident (rung_begin = 0, rung_end = ntemps).  Synchronous. */
int hens_pt_sweep(hens_ctx* ctx, const int64_t* iperm, const int64_t* i1perm, const double* u_swap,
                  int32_t adapt, uint8_t* sel_out, double* swaps_accepted_out);

/* Production stepping: n_iters iterations of (split 0, split 1, PT cascade, adaptation)
 * with device-side Philox4x32-10 draws, no host round trip.  Replaces the body of the
 * hot loop of EnsembleSampler.sample for one in-model StretchMove (ensemble.py:965-981).
 * Asynchronous on the context's stream; hens_synchronize / any download waits. */
int hens_step(hens_ctx* ctx, int64_t n_iters);

/* hens_step(n_before), keep the accept counters as they stand on the device, hens_step(n_last): the reference stores the
 * accept mask of the LAST thinned sub-iteration only (ensemble.py:968-979: `accepted` is re-zeroed per sub-iteration), and
 * a host loop with thin_by > 1 needs no call split and no counter read in between.  hens_get_marked_counters downloads the
 * kept counts ([rungs][nwalkers] f64 each: stretch move, MH move - zeros without one; either pointer may be null). */
int hens_step_marked(hens_ctx* ctx, int64_t n_before, int64_t n_last);
int hens_get_marked_counters(hens_ctx* ctx, double* accepted, double* accepted_mh);
/* hens_step(n_iters) + what EnsembleSampler's loop reads after every proposal (ensemble.py:974-977: `accepted_out`,
 * `move.temperature_control.swaps_accepted`; tempering.py:563-649: the adapted ladder), in one call and one small copy:
 *   accepted_last[Tl][W] u8   accept counts of the call's last n_last iterations (one sampler sub-iteration =
 *                             num_repeats_in_model proposals; saturates at 255)
 *   swaps_last[T-1], betas[T] of the last cascade / after its adaptation.   Any pointer may be NULL.
 * The walkers are NOT copied: the drop-in moves return a State whose arrays download on first read
 * (eryn_amd/state.py: DeviceState; SURVEY 8 b-2 "device-resident State mirror"). */
int hens_step_report(hens_ctx* ctx, int64_t n_iters, int64_t n_last, uint8_t* accepted_last, double* swaps_last, double* betas);

/* ---- Chain store: the stored steps of run_mcmc(store=True) kept in device memory ---------------------------------------------
 * The device-side form of the reference's storage contract (backends/backend.py:1014-1091 `save_step`, called from
 * ensemble.py:1013-1030): a chain buffer in device memory, one small launch (k_chain_store) that appends the walkers in walker
 * order straight from where they ride - column- or slot-ordered walker records, or the by-field arrays -, the accepted / swap
 * totals the backend keeps accumulated beside it, and ONE copy when somebody reads the chain.  Contexts of one GPU with a device
 * likelihood only: a leaf-packing context (HENS_LIKE_TEMPLATE: it has the hens_rj_chain_* family below) or a host-likelihood
 * context, a ladder shard and a pipeline rank -> HENS_ERR_UNSUPPORTED.  hens_upload_state / hens_set_iteration do not clear the chain (a resumed run appends),
 * hens_reset_counters leaves its totals alone, hens_destroy frees it.
 *
 * hens_chain_create: room for `capacity` stored steps of rungs [0, ntemps_store) (0 = all): the allocation the reference makes
 *   in Backend.grow (backends/backend.py:849-913).  A chain that exists is freed first.  Allocation failure -> HENS_ERR_HIP, the
 *   message names the bytes asked for.
 * hens_chain_reset: count = 0, totals = 0, buffers kept (Backend.reset, backends/backend.py:76-261, without the allocation).
 * hens_chain_info: also valid without a chain (capacity = 0): step_bytes is what one stored step of all rungs would take.
 * hens_step_chain: n_store times { iters_per_store - n_last iterations; the accept counters marked; n_last iterations; the
 *   ladder adaptation settled; the state appended } - the body of the sampler's loop over stored steps, ensemble.py:965-1030,
 *   with thin_by * num_repeats_in_model = iters_per_store and num_repeats_in_model = n_last (the reference stores the accept
 *   counts of the LAST thinned sub-iteration, ensemble.py:968-979, and the last cascade's swap counts).  The host copies nothing
 *   and waits for no copy; the append launch goes on the HIP stream between hens_step segments that keep their queue.  The
 *   iteration counter and adaptation time of every stored step are kept on the host: with the seed they are the checkpoint a
 *   stored State carries (hens_set_iteration).  Appending past the capacity -> HENS_ERR_STATE before anything is launched;
 *   n_last < 1 or iters_per_store < n_last -> HENS_ERR_INVALID.
 * hens_chain_download: stored steps [first, first + count) - x[count][ntemps_store][W][D] with D the REAL parameters
 *   (hens_config::ndim_active: pads are not stored), logl / logp [count][ntemps_store][W], betas[count][T] (the ladder after
 *   the step's adaptation, what hens_download_state returns), iteration / adapt_time [count].  Replaces Backend.get_value
 *   (backends/backend.py:263-328).  Any pointer may be NULL; a range outside [0, count) -> HENS_ERR_INVALID.
 * hens_chain_totals: accepted[ntemps_store][W], swaps_accepted[T-1] summed over the steps stored since the last reset
 *   (backends/backend.py:1069-1072); kept as integers on the device. */
typedef struct hens_chain_info_t {
    int64_t capacity;          /* stored steps the buffers hold (0: no chain)              */
    int64_t count;             /* stored steps appended since create / reset               */
    int64_t ntemps_store;      /* rungs stored                                             */
    int64_t bytes;             /* device memory the chain holds                            */
    int64_t step_bytes;        /* ... per stored step (without a chain: of all rungs)      */
    int64_t free_bytes;        /* free device memory now (hipMemGetInfo)                   */
    int64_t n_store_timed;     /* appends of the last hens_step_chain call that were timed */
    double store_ms;           /* ... and their summed duration (hens_set_profiling 1)     */
} hens_chain_info_t;
int hens_chain_create(hens_ctx* ctx, int64_t capacity, int32_t ntemps_store);
int hens_chain_reset(hens_ctx* ctx);
int hens_chain_destroy(hens_ctx* ctx);
int hens_chain_info(hens_ctx* ctx, hens_chain_info_t* out);
int hens_step_chain(hens_ctx* ctx, int64_t n_store, int64_t iters_per_store, int64_t n_last);
int hens_chain_download(hens_ctx* ctx, int64_t first, int64_t count, double* x, double* logl, double* logp, double* betas,
                        int64_t* iteration, int64_t* adapt_time);
int hens_chain_totals(hens_ctx* ctx, double* accepted, double* swaps_accepted);

/* ---- Chain diagnostics on the chain in device memory (csrc/hens_chain_stats.h: k_chain_moments, k_chain_act) -------------------
 * The reductions over the step axis under the reference's get_autocorr_time, get_gelman_rubin_convergence_diagnostic and
 * get_evidence_estimate (backends/backend.py:616-817, utils/utility.py:43-144, 279-330), run where the chain is: one launch reads
 * the kept steps first, first + thin, ..., first + (count - 1) thin of rungs [0, ntemps) and returns arrays the size of one
 * stored step.  The arithmetic and its summation order are eryn_amd/chain_stats.py's, bit for bit.  They read the chain and
 * touch no stepping state.
 *
 * hens_chain_moments: per series of field 0 (x: sum / m2 / n_finite [ntemps][W][D]), 1 (logl) or 2 (logp: [ntemps][W]) the sum
 *   over the kept steps, m2 = sum (x - sum / n)^2 in a second pass, and the entries counted.  logl / logp skip and do not count
 *   non-finite entries (-1e300 is finite); x counts every kept step.
 * hens_chain_act: per series of x the integrated autocorrelation time tau = 1 + 2 sum_{k=1}^{K-1} c_k / c_0 over the lags
 *   K = min(window, count), its mean and c_0 = sum (x - mean)^2 ([ntemps][W][D] each); a constant series gives NaN.  More than 64
 *   lags -> HENS_ERR_UNSUPPORTED (a lane's accumulators and its LDS ring).
 * Outputs are host pointers, any may be NULL.  No chain -> HENS_ERR_STATE; count < 1, thin < 1, window < 1, a field outside
 * [0, 2], ntemps outside [1, ntemps_store] or a kept step outside [0, count of the chain) -> HENS_ERR_INVALID before anything is
 * launched.  A leaf-packing context -> HENS_ERR_UNSUPPORTED: the autocorrelation time is not defined under reversible jump, and
 * Gelman-Rubin over several leaves needs the projection through the leaf masks - hens_rj_chain_leaves / _leaf_moments / _moments
 * below are that family's own.
 * hens_chain_stats_ms: the duration in ms of the last k_chain_moments / k_chain_act launch of the chain (-1: none yet). */
int hens_chain_moments(hens_ctx* ctx, int32_t field, int64_t first, int64_t count, int64_t thin, int32_t ntemps, double* sum,
                       double* m2, int64_t* n_finite);
int hens_chain_act(hens_ctx* ctx, int64_t first, int64_t count, int64_t thin, int32_t ntemps, int32_t window, double* tau,
                   double* mean, double* c0);
int hens_chain_stats_ms(hens_ctx* ctx, double* moments_ms, double* act_ms);

/* ---- Chain store of a leaf-packing context (HENS_LIKE_TEMPLATE after hens_rj_set_model*) ---------------------------------------
 * The same contract for records of several branches and leaves: the stored steps of RJEnsembleSampler.run_mcmc(store=True) stay in
 * device memory, laid out the way the reference's backend returns them (backends/backend.py:1014-1091) - per branch b
 * x_b[step][ntemps_store][W][nl_b][nd_b] with quiet NaN on the leaves whose mask bit is clear (:1049-1059; the resident record keeps
 * a dead leaf's coordinates) and inds_b[step][ntemps_store][W][nl_b] as bytes 0 / 1 -, one append launch per stored step
 * (k_rj_chain_store) straight from the resident records, one copy per branch when somebody reads.  The family is its own: on such a
 * context hens_chain_create / hens_step_chain stay HENS_ERR_UNSUPPORTED.
 *
 * hens_rj_chain_create / _reset / _destroy / _info: as their hens_chain_* namesakes.  Without a model (hens_rj_set_model*) ->
 *   HENS_ERR_STATE; a ladder shard, or a model without a device likelihood (hens_rj_set_model_general) -> HENS_ERR_UNSUPPORTED.
 *   step_bytes = 8 (Ts W (ncoord + 2) + T) + Ts W nslots.  Setting a model anew frees the chain.
 * hens_rj_step_chain: n_store times { iters_per_store - 1 iterations of hens_rj_step's loop; the in-model and birth / death accept
 *   counters marked; one more iteration; the ladder adaptation settled; the full evaluation hens_download_state runs in front of its
 *   copy, under the same rule (resident templates that have drifted); the state appended }: the chain is bit for bit what
 *   { hens_rj_step(iters_per_store); hens_download_state } per stored step gives, and so is the state behind it.  The host waits for
 *   nothing between stored steps; the flags (NaN likelihood, non-finite coordinate) are read once, at the end of the call.
 *   Appending past the capacity -> HENS_ERR_STATE before anything is launched; iters_per_store < 1 -> HENS_ERR_INVALID.
 *   Swap totals: the counts of the last iteration's IN-MODEL cascade (the reference's in_model_swaps, ensemble.py:976-979, 1026),
 *   set aside on the device before the birth / death move's cascade overwrites them.
 * hens_rj_chain_download: stored steps [first, first + count) of ONE branch - x[count][ntemps_store][W][nl_b][nd_b],
 *   inds[count][ntemps_store][W][nl_b] (uint8) - and the shared fields logl / logp [count][ntemps_store][W], betas[count][T],
 *   iteration / adapt_time [count].  branch = -1: the shared fields only (x = inds = NULL).  Any pointer may be NULL; a range
 *   outside [0, count) or a branch the model has not -> HENS_ERR_INVALID.
 * hens_rj_chain_totals: accepted[ntemps_store][W] (in-model move), rj_accepted[ntemps_store][W] (birth / death move: each stored
 *   step's last iteration), swaps_accepted[T-1], summed over the steps stored since the last reset.
 * hens_upload_state / hens_set_iteration / hens_reset_counters leave the chain and its totals alone; hens_destroy frees it. */
int hens_rj_chain_create(hens_ctx* ctx, int64_t capacity, int32_t ntemps_store);
int hens_rj_chain_reset(hens_ctx* ctx);
int hens_rj_chain_destroy(hens_ctx* ctx);
int hens_rj_chain_info(hens_ctx* ctx, hens_chain_info_t* out);
int hens_rj_step_chain(hens_ctx* ctx, int64_t n_store, int64_t iters_per_store);
int hens_rj_chain_download(hens_ctx* ctx, int64_t first, int64_t count, int32_t branch, double* x, uint8_t* inds, double* logl,
                           double* logp, double* betas, int64_t* iteration, int64_t* adapt_time);
int hens_rj_chain_totals(hens_ctx* ctx, double* accepted, double* rj_accepted, double* swaps_accepted);

/* ---- Chain diagnostics of a leaf-packing context's chain (csrc/hens_rj_chain_stats.h: k_rj_chain_leaves, k_rj_chain_leaf_moments) --
 * What one asks of a reversible-jump run - how many leaves, have the walkers converged, the evidence - as reductions over the step
 * axis where the chain is: the reference's get_nleaves, the projection through the leaf masks of its
 * get_gelman_rubin_convergence_diagnostic and its get_evidence_estimate (backends/backend.py:410-434, 664-817).  One launch reads the
 * kept steps first, first + thin, ..., first + (count - 1) thin of rungs [0, ntemps) of one branch and returns arrays no larger than
 * one stored step (nleaves: one byte per place and kept step).  The arithmetic and its order are eryn_amd/chain_stats.py's
 * (leaf_counts, leaf_moments, moments), bit for bit.  They read the chain and touch no stepping state.
 *
 * hens_rj_chain_leaves: nleaves[count][ntemps][W] the leaves in use per kept step, hist[ntemps][W][nl_b + 1] at how many kept steps
 *   walker (t, w) has k leaves in use.  Per-walker totals are sum_k k hist, the model-count posterior of a rung sum_w hist.
 * hens_rj_chain_leaf_moments: per (rung, walker, parameter) the series of the leaves in use in ascending (kept step, slot), those
 *   whose ordinal among the walker's leaves in use lies in [lo, hi): sum and m2 = sum (x - sum / n)^2 in a second pass
 *   [ntemps][W][nd_b], and n[ntemps][W] the samples that entered (hi - lo unless the walker runs out of leaves; n = 0 gives
 *   m2 = 0).  The projected chain of the reference's Gelman-Rubin diagnostic is the window [0, min_leaves).
 * hens_rj_chain_moments: hens_chain_moments over this chain's own arrays - field 0: x of `branch` as stored
 *   ([ntemps][W][nl_b][nd_b], NaN of an unused leaf propagates: what the reference does with a one-leaf branch), 1: logl, 2: logp
 *   ([ntemps][W], non-finite entries skipped and not counted; `branch` unused).
 * hens_rj_chain_stats_ms: the duration in ms of the last k_rj_chain_leaves launch and of the last moments launch of either kind
 *   (-1: none yet).
 * Outputs are host pointers, any may be NULL (all NULL: HENS_OK after the checks, nothing launched).  No chain -> HENS_ERR_STATE; a
 * branch the model has not, count outside [1, 2^31], thin < 1, ntemps outside [1, ntemps_store], a kept step outside the stored
 * ones, lo < 0 or lo >= hi -> HENS_ERR_INVALID with the values in the text, before anything is launched.  A context of the
 * fixed-dimension family -> HENS_ERR_UNSUPPORTED (hens_chain_moments / hens_chain_act are its own, and stay closed to this one). */
int hens_rj_chain_leaves(hens_ctx* ctx, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps, uint8_t* nleaves,
                         uint32_t* hist);
int hens_rj_chain_leaf_moments(hens_ctx* ctx, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps, int64_t lo,
                               int64_t hi, double* sum, double* m2, int64_t* n);
int hens_rj_chain_moments(hens_ctx* ctx, int32_t field, int32_t branch, int64_t first, int64_t count, int64_t thin, int32_t ntemps,
                          double* sum, double* m2, int64_t* n_finite);
int hens_rj_chain_stats_ms(hens_ctx* ctx, double* leaves_ms, double* moments_ms);

/* Counters.  Replaces Move.accepted / num_proposals (move.py:404-421, red_blue.py:326-327),
 * TemperatureControl.swaps_accepted / time (tempering.py:542,596).  Any pointer may be NULL.
 *   accepted[Tl][W] f64 cumulative, swaps_last[T-1], swaps_total[T-1] f64. */
int hens_get_counters(hens_ctx* ctx, double* accepted, int64_t* num_proposals,
                      double* swaps_last, double* swaps_total, int64_t* adapt_time);
int hens_reset_counters(hens_ctx* ctx);
int hens_set_adapt_time(hens_ctx* ctx, int64_t t);

/* Timing of the most recent hens_step call.  hens_set_profiling(ctx, mode): 0 off; 1 a HIP event pair around every launch
 * (forces the call onto the HIP stream); 2 (round 6) the launches' own dispatch timestamps on the queue the call uses anyway -
 * on one GPU the context's AQL queue, same packets, fences and kernel arguments as an untimed call, each packet with a
 * completion signal the packet processor stamps (hsa_amd_profiling_get_dispatch_time: what rocprofv3's kernel trace reads);
 * calls that step on the HIP stream whatever the mode (pipeline ranks, the Gaussian move of a mix) fall back to event pairs.
 * hens_timing::clock says which one the figures came from.
 *   total_ms      wall time of the whole call on the device (0 unless per-kernel profiling is on or HENS_STEP_EVENTS=1: the
 *                 event pair costs a short call two barrier packets)
 *   stretch_ms    summed duration of the stretch kernels, n_stretch = their count
 *   pt_ms         summed duration of the PT cascade kernels, n_pt = their count
 * Per-kernel figures are only filled when per-kernel events were enabled with
 * hens_set_profiling(ctx, 1) (they serialise the stream slightly). */
typedef struct hens_timing {
    double total_ms;
    double stretch_ms;
    double pt_ms;
    double plan_ms;
    int64_t n_stretch;
    int64_t n_pt;
    int64_t n_plan;
    int64_t n_iters;
    double fused_ms;          /* launches that run the second half-step and the cascade together (k_split1_pt) */
    int64_t n_fused;
    int64_t clock;            /* 0 none, 1 HIP event pairs on the HIP stream, 2 dispatch timestamps of the AQL packets */
} hens_timing;
int hens_set_profiling(hens_ctx* ctx, int32_t per_kernel_events);
int hens_get_timing(hens_ctx* ctx, hens_timing* out);
/* Dev aid: begin / end (us after the first launch's begin, from the dispatch packets' own timestamps) of every launch of the
 * last hens_step call that ran with per-kernel events; *n_out = values available (2 per launch). */
int hens_debug_launch_times(hens_ctx* ctx, double* out_us, int64_t capacity, int64_t* n_out);

/* Ladder sharding (one context per GPU, rungs [rung_begin, rung_end)).  The stretch
 * step needs no communication (complement walkers are drawn within a rung,
 * red_blue.py:183-193).  The PT cascade (tempering.py:484-561) is replayed by EVERY rank from the
 * all-gathered log-likelihoods: in column form it is one cheap parallel kernel, and identical
 * decisions / betas on all ranks need no further agreement.  Only walker rows that change rank
 * travel (an all-to-all of [dest id | x | logp] records).  Protocol per iteration, see
 * eryn_amd/ladder.py:
 *   hens_stretch_iter (or two hens_stretch_split calls)     local, no communication
 *   all-gather  device_buffers.logl -> device_buffers.gather_logl           (RCCL)
 *   hens_pt_plan_sharded     decisions, betas, send buffer packed, per-peer counts returned
 *   all-to-all  send_rows -> recv_rows with those counts                    (RCCL)
 *   hens_pt_finish_sharded   received rows scattered into free pool slots, buffers swapped */
typedef struct hens_device_buffers {
    void* logl;          /* f64 [Tl][W] resident rungs (current buffer; changes every PT step) */
    void* gather_logl;   /* f64 [T][W] staging for the all-gathered ladder                     */
    void* send_rows;     /* f64 [row_capacity][D + 2], segments in peer order                  */
    void* recv_rows;     /* f64 [row_capacity][D + 2]                                          */
    int64_t row_capacity;
    int64_t row_doubles; /* D + 2                                                              */
    void* stream;        /* hipStream_t the library launches on                                */
} hens_device_buffers;
int hens_get_device_buffers(hens_ctx* ctx, hens_device_buffers* out);
int hens_set_stream(hens_ctx* ctx, void* hip_stream);

/* One Philox iteration of both red/blue halves on the resident rungs, no PT, asynchronous.
 * Same kernels and draws as hens_step; exists so a sharded ladder can interleave communication. */
int hens_stretch_iter(hens_ctx* ctx);

/* Sharded PT, step 1.  iperm/i1perm/u_swap as in hens_pt_sweep, or all NULL for device-side
 * Philox draws (identical on every rank: they depend only on seed and iteration).
 * rank_of_rung[T] gives the owner of every rung; this context is rank `my_rank`.
 * Outputs (host): send_counts[nranks], recv_counts[nranks] in rows; sel_out / swaps_accepted_out
 * as in hens_pt_sweep (may be NULL).  On return the send buffer is packed.  Synchronous. */
int hens_pt_plan_sharded(hens_ctx* ctx, const int64_t* iperm, const int64_t* i1perm,
                         const double* u_swap, int32_t adapt, const int32_t* rank_of_rung,
                         int32_t nranks, int32_t my_rank, int64_t* send_counts, int64_t* recv_counts,
                         uint8_t* sel_out, double* swaps_accepted_out);
/* Sharded PT, step 2: scatter n_recv received rows (recv_rows, any order) and swap buffers. */
int hens_pt_finish_sharded(hens_ctx* ctx, int64_t n_recv);

/* ---- Metropolis-Hastings proposals: GaussianMove / MHMove ---------------------------
 * One full-ensemble proposal q = x + step for every walker of every resident rung, box prior,
 * likelihood, tempered accept test with factors = 0, update - MHMove.propose (mh.py:56-193) with
 * GaussianMove.get_proposal (gaussian.py:68-195).  The PT sweep that ends the reference's propose()
 * (mh.py:190-191) is hens_pt_sweep, as for the stretch move.
 *   step  f64 [Tl][W][D]  q - x: factor * scale * randn (gaussian.py:166-167) or the multivariate-normal
 *                         draw (gaussian.py:265-268), zero where mode="random"/"sequential" keeps a coordinate
 *   u_acc f64 [Tl][W]     accept uniforms (mh.py:157)
 *   keep_out u8 [Tl][W]   accept mask, or NULL */
int hens_mh_step(hens_ctx* ctx, const double* step, const double* u_acc, uint8_t* keep_out);
/* Device-side draws for hens_step: with probability `weight` an iteration is a Gaussian MH proposal
 * instead of the stretch move (the reference's weighted move mix, ensemble.py:971).  kind 0: isotropic,
 * scale[1] = standard deviation; 1: axis-aligned, scale[D] = standard deviations; 2: full covariance,
 * scale[D*D] = lower Cholesky factor, row-major.  kind < 0 switches the mix off. */
int hens_set_mh_proposal(hens_ctx* ctx, int32_t kind, const double* scale, double weight);
/* accept counts [Tl][W] and number of MH proposals so far (Move.accepted / num_proposals of the MH move). */
int hens_get_mh_counters(hens_ctx* ctx, double* accepted, int64_t* num_proposals);

/* ---- Draw-from-distribution proposals: DistributionGenerate (distgen.py:10-104) -----------------------
 * The independence proposal: every walker of every resident rung is proposed a fresh point from a generator of one
 * distribution per parameter (distgen.py:97) and carries the Hastings factor
 *   factors = (0.0 + logq(old)) + (-logq(new))                                     (distgen.py:84,94,100)
 * into MHMove.propose's accept test (mh.py:155-157); logq is the generator's log-density, its terms added in ascending
 * parameter order from 0.0 (prior.py:364-383), -inf outside a support - an old point outside the generator is never moved.
 * One launch (csrc/hens_dist.h), rows updated in place in either state form.
 *
 * hens_set_dist_proposal: the generator as terms with hens_set_prior_terms' meaning (kind / lo / hi / c0 / c1 / c2, each [D];
 * the pads of a padded row as there).  A distribution one draws from needs a finite uniform support (the rule and the texts of
 * hens_rj_set_prior_terms).  The generator occupies the context's ONE MH slot: it replaces what hens_set_mh_proposal set, and
 * hens_set_mh_proposal replaces it; hens_set_mh_proposal(-1, ...) stays the one "stretch only" call.  With probability `weight`
 * an iteration of hens_step is this move (the weighted move choice, the MH counters and their marks, hens_step_report and the
 * chain store count it as they count the Gaussian move).  Device draws: coordinate d of walker wid = global rung * W + walker in
 * iteration `iter` comes from ONE Philox4x32-10 call, counter (iter lo, iter hi, wid, 14 | d << 8), key = the seed, through the
 * function that draws a leaf's birth (uniform u (hi - lo) + lo; log-uniform exp(u (log hi - log lo) + log lo); normal
 * loc + scale sqrt(-2 log(1 - u)) cos(2 pi v) in double precision); a uniform or log-uniform draw is clamped into [lo, hi]
 * (rounding can put exp(log lo) an ulp below lo, where logq(new) would be -inf).  The accept uniform is the MH move's.
 * Periodic parameters do not enter the move (the reference neither measures a distance nor wraps here).
 * Refused: a leaf-packing context, a host-callable likelihood, row widths other than 8 / 16 / 32 / 64 / 128 after padding
 * (HENS_ERR_UNSUPPORTED); a rank of the ladder pipeline (HENS_ERR_STATE; hens_pipe_init after the move is set:
 * HENS_ERR_UNSUPPORTED); a weight outside [0, 1] or a null array (HENS_ERR_INVALID).
 *
 * hens_dist_step: the teacher-forced twin of hens_mh_step - one proposal with the caller's points.
 *   q     f64 [Tl][W][D]  the proposed points (distgen.py:97: the container's rvs), taken as they are
 *   u_acc f64 [Tl][W]     accept uniforms (mh.py:157)
 *   keep_out u8 [Tl][W]   accept mask, or NULL
 *   factors_out f64 [Tl][W]  the Hastings factors, or NULL
 * HENS_ERR_STATE if no generator is set.  The PT sweep that ends the reference's propose() is hens_pt_sweep. */
int hens_set_dist_proposal(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                           const double* c1, const double* c2, double weight);
int hens_dist_step(hens_ctx* ctx, const double* q, const double* u_acc, uint8_t* keep_out, double* factors_out);

/* ---- Multiple-try independence proposals: MTDistGenMove(independent=True) (mtdistgen.py:7-136) ----------
 * Every walker of every resident rung is offered K = num_try fresh points y_k from a generator of one distribution per parameter
 * (mtdistgen.py:70), with beta the walker's rung (1 in an untempered context):
 *   w_k     = (beta ll_k + lp_k) - logq(y_k)                                        (multipletry.py:45,221-223)
 *   lsw     = max w + log(sum exp(w - max w)); NaN if every w is -inf               (multipletry.py:25-33)
 *   j       = the first k whose running sum of exp(w - lsw) exceeds u_pick, else 0  (multipletry.py:51-57)
 *   w'_k    = w_k for k != j, w'_j = (beta L_old + P_old) - logq(x_old); aux_lsw from w' as lsw from w  (multipletry.py:381-417,463)
 *   factors = ((aux_logP_j - aux_lsw) - alq_j + alq_j) - ((logP_j - lsw) - lq_j + lq_j)   (multipletry.py:472-476)
 * into MHMove.propose's accept test (mh.py:150-171) with logl = ll_j, logp = lp_j, not evaluated again.  An old point outside the
 * generator has w'_j = +inf and aux_lsw = NaN: it is never moved.  The reference evaluates the likelihood of a try whose prior is
 * -inf; the launch skips and fills it: such a try has weight -inf either way and can be "picked" only through the j = 0 fallback,
 * which gives a NaN lnpdiff and a rejection, so the difference cannot be observed.  The sums run in the launch's order, not NumPy's
 * pairwise one: lsw, aux_lsw and factors agree with the reference to rounding, picks and keeps exactly away from knife edges.
 * One launch (csrc/hens_mt.h): a workgroup holds 64 / KP walkers, KP = the smallest power of two >= K, one try per tile row; rows
 * updated in place in either state form.
 *
 * hens_set_mt_dist_proposal: the generator as for hens_set_dist_proposal (one validation for both), into the context's ONE MH slot:
 * it replaces what the slot held and can be replaced by it; hens_set_mh_proposal(-1, ...) stays the one "stretch only" call.  With
 * probability `weight` an iteration of hens_step is this move, counted as the other MH moves are.  Device draws: coordinate d of
 * try k of walker wid comes from hens_set_dist_proposal's function with counter word 3 = 14 | d << 8 | k << 16 (try 0 is the point
 * DistributionGenerate draws); the pick uniform from counter (iter lo, iter hi, wid, 15) by the accept uniform's construction; the
 * accept uniform is the MH move's.
 * Refused: num_try outside 1 .. 64 (HENS_ERR_INVALID), and what hens_set_dist_proposal refuses, with its codes: a leaf-packing
 * context, a host-callable likelihood, an unbuilt row width, a Gibbs table on the MH slot (HENS_ERR_UNSUPPORTED;
 * hens_set_gibbs(HENS_GIBBS_MH) refuses the other way round), a rank of the ladder pipeline (HENS_ERR_STATE).
 *
 * hens_mt_dist_step: the teacher-forced twin - one proposal with the caller's tries.
 *   q      f64 [Tl][W][K][D]  the tries (mtdistgen.py:70: the container's rvs), taken as they are
 *   u_pick f64 [Tl][W]        pick uniforms (multipletry.py:57)
 *   u_acc  f64 [Tl][W]        accept uniforms (mh.py:157)
 *   keep_out u8 [Tl][W], pick_out i32 [Tl][W], lsw_out f64 [2][Tl][W] (lsw, aux_lsw), factors_out f64 [Tl][W]: each may be NULL
 * HENS_ERR_STATE if no generator is set.  The PT sweep that ends the reference's propose() is hens_pt_sweep.
 *
 * hens_mt_debug_draws: what the launch draws in iteration `iter` - q [Tl][W][K][D] (a pad coordinate reads 0), u_pick and u_acc
 * [Tl][W]; each may be NULL.  hens_debug_draws keeps its shape: under this move its mh_step is try 0, its mh_u the accept uniform. */
int hens_set_mt_dist_proposal(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                              const double* c1, const double* c2, int32_t num_try, double weight);
int hens_mt_dist_step(hens_ctx* ctx, const double* q, const double* u_pick, const double* u_acc, uint8_t* keep_out,
                      int32_t* pick_out, double* lsw_out, double* factors_out);
int hens_mt_debug_draws(hens_ctx* ctx, int64_t iter, double* q, double* u_pick, double* u_acc);

/* ---- Gibbs parameter blocks: gibbs_sampling_setup (move.py:113-221) ------------------------------------
 * The reference's moves take a list of parameter blocks and propose block after block: for every block the move's usual draws,
 * the proposal, the old values put back in every coordinate outside the block (move.py:321-324), prior and likelihood of the
 * whole row, the accept test, the update - and ONE swap cascade behind the last block (red_blue.py:119-333, mh.py:79-193).  Here,
 * for one branch with nleaves_max == 1: a block table per move.
 *
 * hens_set_gibbs(ctx, move, nblocks, mask): move = HENS_GIBBS_STRETCH (the stretch move) or HENS_GIBBS_MH (the Gaussian move in
 * the MH slot) - each its own table, as each reference move has its own setup; mask u8 [nblocks][D], non-zero = the coordinate
 * moves with the block (D the context's row width; the pads of a padded row must be 0).  Blocks may overlap and need not cover
 * every coordinate; nblocks == 0 clears the table.  While either move has a table the context steps on the copying launches (as
 * one with prior terms does); an iteration of hens_step / _marked / _report / _chain is, per block of the iteration's move, a
 * plan of the block's draws and the two copying half-steps - or k_mh_draw and the MH launch - then one cascade.  A move without a
 * table of its own runs as one all-true block.  The stretch move's Hastings factor is (n_b - 1) log zz, n_b the block's true
 * coordinates (stretch.py:55-72); a frozen coordinate keeps the old row's bits.
 * Device draws: block b draws from the functions a context without a table uses, with the purpose word of the counter
 * (word 3) carrying the block: PURPOSE_STRETCH | b << 8 (complement index, u_zz, accept uniform), PURPOSE_MH_ACC | b << 8, and
 * PURPOSE_MH_NORMAL | pair << 8 | b << 16 (the pair of coordinates already sits at bit 8).  Block 0's words are those of a
 * context without a table: one all-true block draws what no table draws.  The split labels (one labelling per iteration, as in
 * the reference), the move choice and the PT draws do not depend on the block.
 * Counters: `accepted` (hens_get_counters / hens_get_mh_counters) counts a walker once per accepted block proposal - the MH
 * move's rule in the reference (mh.py:186); its red-blue move adds the running OR over the blocks so far (red_blue.py:306-327),
 * which eryn_amd's rng="numpy" moves reproduce on the host.  num_proposals advances by the number of blocks per iteration
 * (the reference's += 1 per block).  The mask of hens_step_report counts a walker's accepted block proposals over the call's
 * last iterations: non-zero = "any block".
 * Refused, with the context unchanged: nblocks < 0 or > 128, a block without a true coordinate (the reference skips it
 * silently), a true pad (HENS_ERR_INVALID); a half-step pending (HENS_ERR_STATE); periodic parameters, a rank of the ladder
 * pipeline or a ladder shard, hens_set_nsplits other than 2, a leaf-packing context, a host-callable likelihood, a row width
 * other than 8 / 16 / 32 / 64 / 128 after padding, HENS_GIBBS_MH while hens_set_dist_proposal's generator holds the MH slot
 * (HENS_ERR_UNSUPPORTED) - and, the other way round, hens_set_periodic with a period, hens_set_nsplits(> 2), hens_pipe_init and
 * hens_set_dist_proposal while a table stands in their way.
 *
 * hens_gibbs_select(ctx, move, block): teacher-forced stepping - the block that the next hens_stretch_split pair (move 0) or
 * hens_mh_step (move 1) belongs to, until the next call; allowed only between complete moves (HENS_ERR_STATE between the
 * half-steps; HENS_ERR_STATE without a table; HENS_ERR_INVALID outside [0, nblocks)).  hens_set_gibbs selects block 0.  The
 * cascade stays the caller's hens_pt_sweep. */
enum { HENS_GIBBS_STRETCH = 0, HENS_GIBBS_MH = 1 };
int hens_set_gibbs(hens_ctx* ctx, int32_t move, int32_t nblocks, const uint8_t* mask);
int hens_gibbs_select(hens_ctx* ctx, int32_t move, int32_t block);

/* ---- Ladder pipeline: sharded stepping by neighbour exchange (one process per GPU) ------------------
 * No reference counterpart (the reference has no distributed path; it walks the whole ladder in one
 * process, tempering.py:598-649).  Each rank keeps a contiguous rung range (rank 0 = coldest rungs)
 * and a MAILBOX in uncached device memory that its neighbours write into directly (one-sided stores
 * over xGMI through HIP IPC) followed by a flag the consuming kernel spins on; rows that move up a
 * boundary are read straight out of the cold neighbour's walker pool (also IPC-mapped).  After
 *   hens_pipe_init           allocate the mailbox, export the IPC handles (mailbox + pool)
 *   (exchange the blobs: torch.distributed all_gather in eryn_amd.ladder)
 *   hens_pipe_connect        map every rank's mailbox
 * hens_step(n) on every rank advances the WHOLE ladder by n iterations with device-side draws:
 * the result is bit-identical to one context holding all the rungs.  A neighbour that stops
 * answering makes the waiting rank fail with HENS_ERR_STATE after HENS_PIPE_TIMEOUT_S (default 20 s)
 * instead of hanging the GPU. */
#define HENS_PIPE_BLOB_BYTES 128   /* two HIP IPC handles: the rank's mailbox and its walker pool */
int hens_pipe_init(hens_ctx* ctx, int32_t nranks, int32_t my_rank, void* blob_out /* HENS_PIPE_BLOB_BYTES or NULL */,
                   int64_t* mailbox_bytes_out);
int hens_pipe_connect(hens_ctx* ctx, const void* blobs /* nranks * HENS_PIPE_BLOB_BYTES, rank order */);
/* ---- Staged transport: the pipeline's messages over RCCL send/recv ------------------------------------
 * Same kernels, same protocol, but the stores go into LOCAL outboxes and the caller moves the message regions
 * between the stages with point-to-point sends (torch.distributed isend/irecv = grouped ncclSend/ncclRecv on
 * ROCm; eryn_amd.ladder.StagedPipeline).  For nodes where peer mappings are unavailable, and as the literal
 * "RCCL neighbour exchange" of the design brief; it costs host-ordered launches and dense (not sparse) row
 * messages, so the one-sided transport above stays the default.  Per iteration:
 *   hens_pipe_regions                      (pointers of this sweep's message regions)
 *   hens_pipe_stage 0                      move
 *   send ldn_out + ldn_rows_out up,  recv ldn_in + ldn_rows_in from below
 *   recv lup_in from above
 *   hens_pipe_stage 1                      walk
 *   send lup_out down
 *   recv rows_in from above                (before the bottom kernel: a walker may fall through all my rungs)
 *   hens_pipe_stage 2                      bottom
 *   send rows_out down
 *   all-reduce(sum) cnt_out over the ranks, copy to cnt_in */
typedef struct hens_pipe_region_table {
    void* ldn_out;  void* ldn_rows_out;  void* ldn_in;  void* ldn_rows_in;   /* f64: lp_doubles, row_doubles each */
    void* lup_out;  void* lup_in;                                           /* f64: lp_doubles                  */
    void* rows_out; void* rows_in;                                          /* f64: row_doubles                 */
    void* cnt_out;  void* cnt_in;                                           /* u32: cnt_words                   */
    int64_t lp_doubles, row_doubles, cnt_words;
    void* stream;
} hens_pipe_region_table;
int hens_pipe_connect_staged(hens_ctx* ctx);
/* ---- The same with the messages sent by the LIBRARY over RCCL (hens_comm_init / hens_comm_destroy) -------------
 * hens_comm_unique_id: ncclGetUniqueId on ONE rank (128 bytes out); the caller hands the id to the other ranks.
 * hens_comm_init: collective; every rank of the ladder calls it with the same id.  The context becomes a rank of the staged
 *   pipeline (hens_pipe_init + hens_pipe_connect_staged if not done yet) whose neighbour exchanges - grouped ncclSend / ncclRecv
 *   with the ladder neighbours, one all-reduce of the swap counts per sweep - the library enqueues itself on the context's stream:
 *   hens_step(ctx, n) is then ONE call for n iterations (the reference has no distributed path: tempering.py:484-561 is the
 *   cascade being sharded).  librccl.so.1 is dlopen()ed (in a PyTorch-ROCm process: torch's own copy).
 * hens_comm_selfsend: dev aid - n doubles through ncclSend / ncclRecv to the calling rank itself (a one-GPU test of the transport). */
int hens_comm_unique_id(void* unique_id_out /* 128 bytes */);
int hens_comm_init(hens_ctx* ctx, int32_t nranks, int32_t rank, const void* unique_id /* 128 bytes */);
int hens_comm_destroy(hens_ctx* ctx);
int hens_comm_selfsend(hens_ctx* ctx, int64_t n, const double* src_host, double* dst_host);
int hens_pipe_regions(hens_ctx* ctx, hens_pipe_region_table* out);
int hens_pipe_stage(hens_ctx* ctx, int32_t stage);

/* Self-test of the peer accesses the pipeline relies on (one-sided put + flag into uncached memory, pull out of
 * ordinary device memory), between this process and its ladder neighbours' processes, which find each other
 * through files in `dir`.  Needs no context.  eryn_amd.ladder runs it in a throw-away process per rank before
 * hens_pipe_connect, so a node where peer mappings do not work fails here and not in the sampler. */
int hens_pipe_selftest(int32_t device_id, int32_t rank, int32_t nranks, const char* dir, double timeout_s);
/* Debug (env HENS_PIPE_STATS=1 at hens_pipe_init): where the pipeline waits.  out16 = 8 pairs (wall-clock
 * ticks spent spinning, number of waits): [0] stretch prologue on arrived rows, [1] stretch prologue on swap
 * counts, [2] walk on the hot neighbour's columns, [3] bottom on the cold neighbour's rung, [4] bottom on rows
 * from above.  Ticks are hipDeviceAttributeWallClockRate (100 MHz on MI355X). */
int hens_pipe_debug_stats(hens_ctx* ctx, uint64_t* out16, int32_t reset);
/* Same, for contexts that live in ONE process (tests; several shards on one GPU): peers[nranks]. */
int hens_pipe_connect_local(hens_ctx* ctx, hens_ctx* const* peers);

/* Debug: per-workgroup phase timestamps of the stretch kernel (shader-clock ticks, 8 per
 * workgroup: start, A done, barrier, B done, barrier, C done, D done, end).  enable != 0 makes
 * the following stretch launches record; enable == 0 copies the last launch's trace to `out`
 * (capacity in 64-bit words) and stops recording.  *n_out = words written. */
int hens_debug_trace(hens_ctx* ctx, int32_t enable, uint64_t* out, int64_t capacity, int64_t* n_out);

/* Debug: the keyed pseudo-random permutation the Philox mode uses for iteration `iter`:
 * which = 0 the PT column map of global rung `rung`, which = 1 the split labelling permutation of
 * rung `rung`.  out[nwalkers] i32. */
int hens_debug_permutation(hens_ctx* ctx, int32_t which, int32_t rung, int64_t iter, int32_t* out);

/* Reversible-jump leaf packing (BASELINE config 4).  A context created with HENS_LIKE_TEMPLATE holds
 * variable-dimension walkers as RECORDS of ndim doubles:
 *     [ branch 0: nleaves_max_0 x 3 coordinates | branch 1: ... | leaf mask of branch 0 | mask of branch 1 | ... | pad ]
 * where a mask is the reference's inds[t, w, :] (state.py:330-562, backends/backend.py:1049-1059) as an integer stored
 * in a double (bit n = leaf slot n in use).  hens_upload_state / hens_download_state / hens_eval_state / hens_pt_sweep /
 * hens_get_counters work on records unchanged: a PT swap carries all leaves and masks of a walker (tempering.py:376-480).
 *
 * hens_rj_set_model: the model of the reference's own RJ tests (tests/test_eryn.py:38-92, 341-507): per branch a leaf
 *   kind (0 Gaussian pulse a exp(-(t-b)^2 / 2c^2), 1 sine a sin(2 pi b t + c)), leaf budget [nleaves_min, nleaves_max],
 *   a uniform box prior per leaf parameter (lo / hi [nbranches][3]; leaf_logp[b] = sum_d log(1/(hi-lo)) accumulated by
 *   the caller in the reference's order, prior.py:364-383) and the data (t, y)[ndata], sigma of
 *   logL = -1/2 sum(((template - y) / sigma)^2).
 * hens_rj_mh_step: the in-model GaussianMove on the packed active leaves of every branch (mh.py:56-193,
 *   gaussian.py:68-115,265-268) with the caller's draws: step[Tl][W][ncoord] in record layout (zero on unused slots),
 *   u_acc[Tl][W].  Replaces compute_log_prior / compute_log_like with inds (ensemble.py:1127-1217, 1219-1545,
 *   utils/utility.py:8-40 leaf grouping), the accept test and Move.update (move.py:472-703).
 * hens_rj_bd_step: DistributionGenerateRJ on one branch (distgenrj.py:35-222, rj.py:145-388): change[Tl][W] in
 *   {-1, 0, +1} after the edge rule (distgenrj.py:69-73), leaf[Tl][W] the slot that is born or dies, birth[Tl][W][3] the
 *   prior draw of a born leaf, u_acc[Tl][W].  The library adds the proposal factors -/+ log q(leaf), the edge factors
 *   (rj.py:236-270) and the fix_logp_gibbs rule (move.py:368-402).  Follow it with hens_pt_sweep(adapt = 0) (rj.py:381-382).
 * hens_rj_stretch_split: one half of the red / blue StretchMove on a state of several branches and leaves (round 5; SURVEY 8
 *   row a4's loop over branches): RedBlueMove.propose (red_blue.py:103-330) + StretchMove.get_proposal / choose_c_vals /
 *   get_new_points (stretch.py:74-231) without Gibbs sampling.  labels[Tl][W] in {0, 1} (arange(W) % 2 shuffled per rung,
 *   red_blue.py:119-124; the same array for both splits), rint[nbranches][Tl][Ns] - EVERY branch its own complement draw,
 *   an index into the other set in ascending walker order (stretch.py:93-100, 205) -, u_zz[Tl][Ns] the ONE stretch factor's
 *   uniform per walker (stretch.py:128-132), u_acc[Tl][Ns], keep_out[Tl][Ns] by position of the moving set (ascending walker
 *   order).  Every leaf slot of every branch moves, active or not; factors = (sum of nleaves_max * ndim - 1) log zz
 *   (stretch.py:222-223); the leaf masks stay and decide what prior and likelihood see; rows are updated in place (complements
 *   come from the other set).  Call split 0 then split 1, then hens_pt_sweep.  Fewer than twice as many walkers as leaf
 *   coordinates -> HENS_ERR_TOO_FEW_WALKERS (red_blue.py:103-114).
 * hens_rj_set_mh_scale + hens_rj_step: production: n iterations of (in-model move, swaps + adaptation, birth / death on
 *   a uniformly chosen branch, swaps) with device-side Philox draws of the same distributions.  Every walker's model at the
 *   data points stays resident and birth / death evaluates `model +- one leaf`; the resident models AND the log-likelihoods
 *   are re-evaluated from the coordinates whenever the state has crossed this interface since the last call (hens_upload_state,
 *   a parity-API move, hens_download_state) and whenever iteration % 64 == 63, so a log-likelihood carries the rounding of at
 *   most 63 iterations of +- updates (observed <= 6e-16 relative against the oracle, bar 1e-12) and a chain is a function of
 *   (State, seed, iteration counter, adaptation time): resumed from a downloaded State in a new context it is the uninterrupted
 *   chain bit for bit.  On a uniform time grid (every point within 4 eps max|t| of t0 + i dt) the model is evaluated eight
 *   consecutive points at a time by recurrence (pulses) and rotation (sines), which places point i0 + k at t[i0] + k dt; a grid
 *   whose points lie farther from those positions than 128 eps times the narrowest pulse width of the prior box is evaluated
 *   point by point instead (its sines too).  This is an engineering limit, not a bound: at the limit a pulse value's position
 *   error can reach ~0.61 * 128 eps |a|, many times that point's share of B, the error bound of a plain float64 evaluation.
 *   Observed on the case matrix of tests/test_hip_template_accuracy.py (offset, wide, tiny and jittered grids): within 1.1 B
 *   of the exact log-likelihood on every path; before the limit, over 2 000 B on grids far from t = 0.
 * hens_rj_get_counters: accept counts of the birth / death move (hens_get_counters has the in-model move's). */
int hens_rj_set_model(hens_ctx* ctx, int32_t nbranches, const int32_t* kinds, const int32_t* nleaves_max,
                      const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp,
                      int32_t ndata, const double* t, const double* y, double sigma);
/* A leaf-packing model WITHOUT a device likelihood (round 6): the reference's `ndims` per branch (ensemble.py:325-329) - 1 .. 4
 * box-prior parameters per leaf, up to 4 branches, up to 64 leaf slots and 128 record doubles in all - for chains whose likelihood is
 * the caller's function of the packed active leaves (ensemble.py:1306-1334, 1340-1545): such a context is stepped with
 * hens_rj_propose / hens_rj_accept only (hens_rj_step and the parity moves with the built-in template likelihood refuse it), and
 * hens_eval_state leaves the log-prior and the fill value as log-likelihood (the caller uploads its own).  Record layout as
 * hens_rj_set_model's with ndims[b] doubles per leaf slot; lo / hi: the branches' boxes one after the other; the `birth` arrays of
 * hens_rj_draws have a stride of max(ndims) doubles per walker. */
int hens_rj_set_model_general(hens_ctx* ctx, int32_t nbranches, const int32_t* ndims, const int32_t* nleaves_max,
                              const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp);
/* hens_rj_set_model with every leaf kind the device evaluates - one to four parameters per leaf, the value at data point t:
 *   HENS_RJ_KIND_PULSE   (a, b, c)      a exp(-(t - b)^2 / (2 c^2))          HENS_RJ_KIND_SINE   (a, b, c)  a sin(2 pi b t + c)
 *   HENS_RJ_KIND_OFFSET  (a)            a                                    HENS_RJ_KIND_RAMP   (a, b)     a + b t
 *   HENS_RJ_KIND_LORENTZ (a, b, c)      a / (1 + ((t - b) / c)^2)            HENS_RJ_KIND_CHIRP  (a, b, c)  a sin(2 pi b t + c t^2)
 *   HENS_RJ_KIND_BURST   (a, t0, w, f)  a exp(-((t - t0) / w)^2) cos(2 pi f (t - t0))
 * in float64 without FMA contraction, 2 pi the double 2 * M_PI; a walker's leaves are added one by one to a running template,
 * branch by branch in ascending slot order.  lo / hi: the branches' boxes one after the other (a branch's width follows from its
 * kind), as hens_rj_set_model_general takes them; the record holds kind-width doubles per leaf slot and the `birth` arrays have
 * a stride of the widest branch's parameters.  Up to 64 leaf slots and 128 record doubles (else HENS_ERR_UNSUPPORTED /
 * HENS_ERR_INVALID as hens_rj_set_model_general); an unknown kind -> HENS_ERR_INVALID.  Everything that steps or reads a
 * hens_rj_set_model context works on such a model - hens_rj_step with every schedule and both in-model moves, the parity moves,
 * hens_eval_state, resume by hens_set_iteration, the debug exports - except full leaf covariances: hens_rj_set_mh_chol on a
 * model with a kind beyond pulse / sine -> HENS_ERR_UNSUPPORTED.  Such a model is evaluated point by point on every grid (no
 * uniform-grid recurrence); resident templates for ndata <= 512 as ever.  A model of pulses and sines alone is exactly
 * hens_rj_set_model's. */
enum { HENS_RJ_KIND_PULSE = 0, HENS_RJ_KIND_SINE = 1, HENS_RJ_KIND_OFFSET = 2, HENS_RJ_KIND_RAMP = 3, HENS_RJ_KIND_LORENTZ = 4,
       HENS_RJ_KIND_CHIRP = 5, HENS_RJ_KIND_BURST = 6 };
int hens_rj_set_model_kinds(hens_ctx* ctx, int32_t nbranches, const int32_t* kinds, const int32_t* nleaves_max,
                            const int32_t* nleaves_min, const double* lo, const double* hi, const double* leaf_logp,
                            int32_t ndata, const double* t, const double* y, double sigma);
/* scale[nbranches][widest branch's parameters] (3 on a hens_rj_set_model context): standard deviations of the in-model Gaussian step */
int hens_rj_set_mh_scale(hens_ctx* ctx, const double* scale);
/* The Philox in-model Gaussian move with a FULL covariance per leaf (gaussian.py:265-268: multivariate_normal(0, cov)):
 * chol[nbranches][3][3], the lower-triangular Cholesky factor L of a branch's leaf covariance.  A leaf's step is
 * step_d = sum_{j <= d} L[d][j] z_j, summed in ascending j without FMA contraction, z_j the unit normals hens_rj_set_mh_scale's
 * path draws for the leaf's coordinates (same Philox keys: chol = diag(s) is the chain of hens_rj_set_mh_scale(s) bit for bit).
 * hens_rj_debug_draws exports the correlated step.  Entries above the diagonal must be zero; a non-finite entry or a diagonal
 * entry <= 0 (the covariance was not positive definite) -> HENS_ERR_INVALID.  The last of the two setters called holds. */
int hens_rj_set_mh_chol(hens_ctx* ctx, const double* chol);
/* Periodic leaf parameters: the `periodic` argument of EnsembleSampler / Move (a PeriodicContainer, utils/periodic.py:11-151) on a
 * leaf-packing context, per branch and per leaf parameter.  period[nbranches][widest branch's parameters] in the birth arrays'
 * stride; period > 0 makes that parameter of every leaf slot of the branch periodic, 0 = not periodic, NULL or all zeros clears.
 * Every entry point that forms an IN-MODEL proposal honours it, teacher-forced and Philox alike, with hens_set_periodic's arithmetic
 * (NumPy's remainder; the difference taken again from the moving point shifted by one period):
 *   Gaussian move (hens_rj_mh_step, hens_rj_step, hens_rj_propose)   q = wrap(x + step) on the active leaves, and wrap(x) on the
 *       periodic coordinates of every other slot: the reference wraps the whole copied array (gaussian.py:102-127), so an accepted
 *       walker's record carries x % period in its dead slots
 *   ... under Gibbs blocks (hens_rj_set_gibbs)   every coordinate that is true in the block's mask is wrapped, moved or not, active or
 *       not; every other coordinate keeps its bits (move.py:322-324 puts it back)
 *   stretch move (hens_rj_stretch_split, hens_rj_step, hens_rj_propose)   q = wrap(c - distance(x, c) zz) on every slot
 *       (stretch.py:136-154), c - x measured the short way round where it exceeds half a period
 *   group stretch move (hens_rj_group_step, hens_rj_step)   the same with the friend as c; a dead slot and a leaf of a branch with an
 *       empty table are their own friend: wrap(x).  The friend RULE stays nearest by linear distance in the key parameter, also
 *       where the key is periodic (a departure that is stated, not refused).
 * Birth / death, multiple-try birth / death and the cascade know no periods, as in the reference (they draw from the prior).
 * The periods survive hens_rj_set_mh_scale, hens_rj_set_mh_chol, hens_rj_set_prior_terms, hens_rj_set_gibbs and hens_rj_set_group in
 * any order; a new model (hens_rj_set_model*) drops them.  A context without periods launches what it launched before and steps the
 * same chain.  Refused with the context unchanged: a negative, NaN or infinite period, a period on a parameter index >= the branch's
 * number of leaf parameters (HENS_ERR_INVALID); a context that is not leaf-packing (HENS_ERR_UNSUPPORTED: hens_set_periodic is
 * its call); between the two stretch half-steps or while hens_rj_accept is pending (HENS_ERR_STATE). */
int hens_rj_set_periodic(hens_ctx* ctx, const double* period);
/* Per-parameter prior terms on the leaves: ProbDistContainer({i: dist_i}) per branch with uniform, log-uniform and normal
 * distributions (prior.py:337-392) in place of the box of the hens_rj_set_model* call that came before.  kind / lo / hi / c0 / c1 /
 * c2 run over the branches' leaf parameters one after the other (sum_b ndims[b] entries, as hens_rj_set_model_general takes lo /
 * hi); a term's meaning and constants are hens_set_prior_terms's.  On a leaf-packing chain the prior enters three times, and all
 * three follow the terms:
 *   log-prior      per active slot ((0.0 + t_0) + t_1) + ... in ascending parameter order, -inf if a parameter is outside its
 *                  support or a term is not finite; dead slots count 0.0 and are not evaluated; slots and branches summed as ever
 *   Hastings       a death adds, a birth subtracts log q(leaf): the same sum on the dying / born leaf (distgenrj.py:188-214)
 *   births         hens_rj_step draws parameter d of a born leaf from the Philox call keyed (branch, d), words (x, y, z, w):
 *                  uniform u (hi - lo) + lo; log-uniform exp(u (log hi - log lo) + log lo), u = the 53-bit uniform of (x, y);
 *                  normal c0 + c1 sqrt(-2 log(1 - u)) cos(2 pi v), v the 53-bit uniform of (z, w): Box-Muller in double precision.
 *                  hens_rj_debug_draws exports them.  Teacher-forced moves take the caller's `birth` as before.
 * Every entry point that computes a log-prior on records follows: hens_eval_state, hens_rj_step / hens_rj_step_chain (every
 * schedule, both in-model moves), the parity moves, hens_rj_propose / hens_rj_accept.  A model with a term other than uniform
 * runs on the kernels that read leaf widths at run time (a pulse / sine model too: per-point leaf values, as under
 * hens_rj_set_model_kinds - no uniform-grid recurrence), so its limits are theirs: 64 leaf slots, 128 record doubles
 * (HENS_ERR_UNSUPPORTED beyond).  Uniform kinds only: the call IS the box lo / hi with leaf_logp[b] = the branch's c0 summed
 * in ascending order - same kernels, same chain as that box model.  HENS_ERR_STATE on another context or before a model;
 * HENS_ERR_INVALID for an unknown kind, lo >= hi, a non-finite constant, scale <= 0, a log-uniform term without 0 < lo < hi <
 * inf; HENS_ERR_UNSUPPORTED together with full leaf covariances (hens_rj_set_mh_chol, in either order).  A refused call changes
 * nothing.  A later hens_rj_set_model* call returns to that model's box. */
int hens_rj_set_prior_terms(hens_ctx* ctx, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                            const double* c1, const double* c2);
int hens_rj_mh_step(hens_ctx* ctx, const double* step, const double* u_acc, uint8_t* keep_out);
int hens_rj_bd_step(hens_ctx* ctx, int32_t branch, const int8_t* change, const int32_t* leaf, const double* birth,
                    const double* u_acc, uint8_t* keep_out);
int hens_rj_stretch_split(hens_ctx* ctx, int32_t split, const uint8_t* labels, const int64_t* rint, const double* u_zz,
                          const double* u_acc, uint8_t* keep_out);
int hens_rj_step(hens_ctx* ctx, int64_t n_iters);
int hens_rj_get_counters(hens_ctx* ctx, double* accepted_bd, int64_t* num_mh, int64_t* num_bd);

/* Debug / parity: everything hens_rj_step draws in iteration `iter` (a pure function of seed, iteration, global rung and
 * walker), in a form that maps onto the reference's draws so that the production leaf-packing path can be replayed through
 * the CPU oracle (tests/test_hip_rj.py):
 *   step [Tl][W][ind_off]   the in-model Gaussian step of every coordinate slot, record layout (gaussian.py:265-268; only the
 *                           active leaves' entries are consumed)
 *   u_mh, u_bd [Tl][W]      accept uniforms of the two moves (mh.py:157, rj.py:332)
 *   branch                  the branch of the birth / death move (ensemble.py:988-990, "separate_branches")
 *   coin [Tl][W] i8         +1 / -1 before the edge rule (distgenrj.py:63-73)
 *   sel  [Tl][W] u32        leaf selector: of `cnt` candidate slots in ascending order, the one of index (sel * cnt) >> 32
 *                           (distgenrj.py:97-112)
 *   birth [Tl][W][3]        coordinates of a leaf born in `branch` (generate_dist.rvs, prior.py:60-66)
 *   slot_* [T][W], uswap_* [T-1][W]   column maps and swap uniforms of the cascade after the in-model move and of the one
 *                           after the birth / death move, as in hens_debug_draws (tempering.py:526-541) */
int hens_rj_debug_draws(hens_ctx* ctx, int64_t iter, double* step, double* u_mh, int32_t* branch, int8_t* coin, uint32_t* sel,
                        double* birth, double* u_bd, int32_t* slot_mh, double* uswap_mh, int32_t* slot_bd, double* uswap_bd);

/* Read-only view of the resident state of a leaf-packing context: records [Tl][W][RW] and log-likelihoods [Tl][W] as they sit on
 * the device, WITHOUT the evaluation from the coordinates that hens_download_state runs in front of its copy - i.e. with the
 * +- leaf updates of hens_rj_step since the last refresh in them (tests measure that drift).  Either pointer may be NULL. */
int hens_rj_debug_resident(hens_ctx* ctx, double* rec, double* logl);

/* The between-model schedule of hens_rj_step (the sampler's rj_moves string, ensemble.py:434-480):
 *   0  "separate_branches" (default): one DistributionGenerateRJ per branch, one of them chosen per iteration
 *   1  "iterate_branches": ONE move that walks through every branch in turn (birth / death, accept, update per branch), then
 *      one sweep of swaps without adaptation; its accept counts are the last branch's (rj.py:169-388).
 *   2  "together" (ensemble.py:414-432): ONE proposal changes a leaf in EVERY branch of the walker - all coins and leaf choices,
 *      then the births branch by branch, the factors summed, one accept test (distgenrj.py:150-222).
 * With schedules 1 and 2 hens_rj_debug_draws returns branch = -1 and coin / sel / birth / u_bd for every branch in order
 * ([nbranches][Tl][W]...; the caller sizes them for nbranches either way; schedule 2: every row of u_bd is the one uniform). */
int hens_rj_set_schedule(hens_ctx* ctx, int32_t schedule);

/* The in-model move of hens_rj_step:
 *   HENS_RJ_INMODEL_GAUSSIAN (default)  the Gaussian step of hens_rj_set_mh_scale on every active leaf (mh.py:56-193).
 *   HENS_RJ_INMODEL_STRETCH             the red / blue StretchMove over every branch and leaf slot - the reference's default move
 *      (ensemble.py:509-514; red_blue.py:103-330, stretch.py:74-231), two launches per iteration, a half each, with the
 *      context's `a` and `live_dangerously` (the ones hens_rj_stretch_split uses).  No step scale is asked for; fewer than
 *      twice as many walkers as leaf coordinates -> hens_rj_step returns HENS_ERR_TOO_FEW_WALKERS before it launches anything
 *      (red_blue.py:103-114).  Draws (counter-based on seed, iteration, global rung, walker, half, branch): rung t's split is the
 *      keyed permutation of purpose RJ_SPLIT - positions [0, ceil(W/2)) are set 0, the rest set 1 (red_blue.py:119-124: a
 *      uniform balanced labelling) -; branch b's complement is a uniform position of the other half (stretch.py:93-100, 205: a
 *      walker per branch), the stretch factor's uniform comes with branch 0's call (stretch.py:128-132), the accept uniform has
 *      the half in its key (red_blue.py:294).  Accept counts: hens_get_counters; hens_rj_get_counters' num_mh counts one per move.
 *   HENS_RJ_INMODEL_GROUP               the group stretch move toward a stationary friend table (hens_rj_set_group below, which
 *      must come first: HENS_ERR_STATE otherwise): one launch per iteration, the table rebuilt every n_iter_update moves.
 * Schedule 3 of hens_rj_set_schedule ("none") runs the in-model move and its cascade with adaptation alone - EnsembleSampler
 * without rj_moves: the leaf masks never change, num_bd stays 0; the iteration counter and the cascade's key 2 iter are those of
 * the other schedules, so a chain's in-model draws do not depend on the schedule. */
enum { HENS_RJ_INMODEL_GAUSSIAN = 0, HENS_RJ_INMODEL_STRETCH = 1, HENS_RJ_INMODEL_GROUP = 2 };
int hens_rj_set_in_model(hens_ctx* ctx, int32_t kind);

/* Debug / parity: the stretch move's draws of iteration `iter` IN THE FORM hens_rj_stretch_split TAKES, n0 = ceil(W / 2):
 * labels[Tl][W] in {0, 1}; rint[2][nbranches][Tl][n0] an index into the other set's ascending walker list; u_zz, u_acc
 * [2][Tl][n0]; movers in ascending walker order; for odd W the second half uses the first W - n0 entries of a row (the rest
 * are zero).  On a stretch context hens_rj_debug_draws returns zeros in step / u_mh and asks for no scale. */
int hens_rj_debug_draws_stretch(hens_ctx* ctx, int64_t iter, uint8_t* labels, int64_t* rint, double* u_zz, double* u_acc);

/* Parity-mode birth / death over ALL branches in one proposal ("together"): change / leaf [nbranches][Tl][W],
 * birth [nbranches][Tl][W][3 - max(ndims) on a hens_rj_set_model_general context], ONE u_acc [Tl][W] (rj.py:145-388 with gibbs_sampling_setup = None). */
int hens_rj_bd_all_step(hens_ctx* ctx, const int8_t* change, const int32_t* leaf, const double* birth, const double* u_acc,
                        uint8_t* keep_out);

/* The multiple-try birth / death move: MTDistGenMoveRJ(generate_dist, num_try = K, rj = True) of the reference (mtdistgenrj.py over
 * multipletry.py:238-514 - its `elif self.rj` branch - and multipletry.py:597-776) in place of DistributionGenerateRJ.  One branch
 * per proposal; coin, edge rule and leaf slot are the plain move's.  A birth walker is offered K leaves drawn from the generator
 * into the free slot, one of them picked by importance weight; a death walker's try 0 IS the dying leaf, tries 1 .. K-1 are fresh
 * draws into its slot, and the auxiliary side of both is K copies of the walker without the leaf (csrc/hens_rj_mt.h states the
 * formulas: lsw, pick, aux_lsw, factors).  The multiple-try factors replace the plain move's -+ log q(leaf); edge factors,
 * fix_logp_gibbs, the accept test and the update are ReversibleJumpMove.propose's (rj.py:236-352).  A try whose walker has a -inf
 * log-prior is not evaluated (its log-likelihood is the fill value); every weight -inf, or a dying leaf outside the generator's
 * support, gives NaN sums and a rejection, as in the reference.
 *
 * hens_rj_set_mt_proposal: num_try in [1, 64] and the generator's terms per leaf parameter over the branches, in
 *   hens_rj_set_prior_terms's layout and meaning (kind / lo / hi / c0 / c1 / c2, sum_b ndims[b] entries); kind == NULL: the generator
 *   is the prior (the other five are not read).  num_try == 0 returns to the plain move.  Refused, the context unchanged:
 *   num_try outside [0, 64] or an invalid term -> HENS_ERR_INVALID; a branch with nleaves_min == nleaves_max -> HENS_ERR_INVALID
 *   (multipletry.py:661-664); a model without a device likelihood (hens_rj_set_model_general) -> HENS_ERR_STATE; more than 64 leaf
 *   slots or 128 record doubles -> HENS_ERR_UNSUPPORTED.  A later hens_rj_set_model* or hens_rj_set_prior_terms call clears it.
 * hens_rj_mt_bd_step: the move teacher-forced, in the reference's order of operations (every try a full evaluation of the walker's
 *   active leaves with the try in its slot): change[Tl][W] in {-1, +1}, leaf[Tl][W], tries[Tl][W][K][max(ndims)] (a death walker's
 *   tries[..][0] is ignored), u_pick, u_acc [Tl][W]; keep_out[Tl][W] or NULL; out NULL, or any of its arrays NULL: pick, lsw,
 *   aux_lsw, factors (the multiple-try factors, negated on a death, before the edge factors), mt_ll, mt_lp (the proposed state's
 *   log-likelihood and log-prior before fix_logp_gibbs), each [Tl][W].  Follow it with hens_pt_sweep(adapt = 0), like hens_rj_bd_step.
 * hens_rj_step / hens_rj_step_chain with a proposal set: the birth / death launch of schedules 0 and 1 is this move (k_rj_mt) on
 *   the resident templates - try k = base template + leaf k, the base the resident template (birth) or resident - dying leaf
 *   (death); L after an accepted death is the likelihood of the base.  Schedule 2 ("together") -> HENS_ERR_UNSUPPORTED before
 *   anything is launched (multipletry.py:635-636); schedule 3 is untouched.  Counters: hens_rj_get_counters.  Draws: coin,
 *   selector and accept uniform are the plain move's keys; coordinate d of try 0 of a birth is the plain move's birth call, of try
 *   k >= 1 the call keyed RJ_TRY | d << 8 | k << 10 | branch << 16, turned into a value by hens_rj_set_prior_terms's
 *   constructions on the generator's terms; the pick uniform: the 53-bit uniform of (x, y) of the call keyed RJ_PICK | branch << 16.
 * hens_rj_mt_debug_draws: tries [nbranches][Tl][W][K][max(ndims)] (try 0: what a birth walker gets) and u_pick [nbranches][Tl][W]
 *   of iteration `iter`, entry 0 the chosen branch ("separate_branches") or one entry per branch in order, as hens_rj_debug_draws
 *   sizes its per-branch outputs - which has the coin, the selector, the accept uniform and the cascades' draws.
 * hens_rj_propose with a proposal set -> HENS_ERR_UNSUPPORTED. */
typedef struct hens_rj_mt_out {
    int32_t* pick; double* lsw; double* aux_lsw; double* factors; double* mt_ll; double* mt_lp;
} hens_rj_mt_out;
int hens_rj_set_mt_proposal(hens_ctx* ctx, int32_t num_try, const int32_t* kind, const double* lo, const double* hi, const double* c0,
                            const double* c1, const double* c2);
int hens_rj_mt_bd_step(hens_ctx* ctx, int32_t branch, const int8_t* change, const int32_t* leaf, const double* tries,
                       const double* u_pick, const double* u_acc, uint8_t* keep_out, const hens_rj_mt_out* out);
int hens_rj_mt_debug_draws(hens_ctx* ctx, int64_t iter, double* tries, double* u_pick);

/* Gibbs blocks over branches and leaf slots for the in-model Gaussian move of a leaf-packing context: the reference's
 * GaussianMove(cov, gibbs_sampling_setup=[...]) on a state of several branches and leaves (move.py:113-402 under mh.py:79-193).  A
 * block is a mask over the record's coordinates; per block, in table order: a leaf slot with any true coordinate is a member
 * (move.py:278), the ACTIVE leaves of member slots move - q = x + step on their true coordinates, every other coordinate keeps its
 * bits (move.py:322-324) -, the log-prior is taken over every active leaf, fix_logp_gibbs (move.py:368-402) gives a walker without
 * a moved leaf -inf (0.0 if it holds no leaf at all), then likelihood, tempered accept test with factors 0 and update; the next
 * block starts from the state the last one left.  (csrc/hens_rj_gibbs.h states the kernel, k_rj_gibbs.)
 *
 * hens_rj_set_gibbs: mask u8 [nblocks][ncoord] in record layout (ncoord = sum_b nleaves_max[b] ndims[b], hens_rj_debug_draws's
 *   `step` layout), non-zero = the coordinate moves with the block; 1 .. 128 blocks, they may overlap and need not cover every
 *   coordinate; nblocks == 0 clears the table.  Selects block 0.  Refused, the context unchanged: a block without a true
 *   coordinate, nblocks outside [0, 128], a null mask (HENS_ERR_INVALID); before a model, or with a half-step pending
 *   (HENS_ERR_STATE); a model without a device likelihood (hens_rj_set_model_general), the stretch in-model move, more than 64 leaf
 *   slots (HENS_ERR_UNSUPPORTED) - and, the other way round, hens_rj_set_in_model(HENS_RJ_INMODEL_STRETCH) and hens_rj_propose of
 *   the in-model move while a table stands (HENS_ERR_UNSUPPORTED).  A later hens_rj_set_model* call clears the table.
 *   hens_set_gibbs stays closed to leaf-packing contexts.
 * hens_rj_gibbs_select: the block the next hens_rj_mh_step belongs to - step[Tl][W][ncoord] (read on the moved leaves' true
 *   coordinates), u_acc, keep_out as ever -, until the next call; HENS_ERR_STATE between the halves of a move or without a table,
 *   HENS_ERR_INVALID outside [0, nblocks).  The reference skips a block in which no walker of any rung has a moved leaf, before
 *   any draw (mh.py:105-107): a caller that follows it simply does not call for that block.
 * hens_rj_step / hens_rj_step_chain with a table: ONE k_rj_gibbs launch walks all blocks of the iteration in place of the k_rj
 *   in-model launch, on the resident templates: per moved leaf template = (template - leaf_old) + leaf_new per data point, so the
 *   templates drift by rounding on every schedule (schedule 3 too) and the 64-iteration refresh bounds it as it does for birth /
 *   death.  DEPARTURE from the reference: the device skips no block - every walker of a block without a moved leaf is rejected by
 *   fix_logp_gibbs - so num_mh (hens_rj_get_counters) advances by nblocks per iteration, skipped blocks included.  A table of
 *   exactly one block with every coordinate true is the move of a context without a table: k_rj's launch, the same chain bit for
 *   bit, num_mh + 1.  Draws: block k's unit normal of record coordinate i is the Philox call keyed RJ_NORMAL(i) | k << 25 (bits
 *   0 - 24 are the call's of a context without a table), its accept uniform the call keyed RJ_ACC(in-model) | k << 19 (bits 0 - 18
 *   likewise); block 0's words are those of a context without a table.  Both step setters serve: scale x z, or L z per leaf.
 * hens_rj_gibbs_debug_draws: block `block`'s step[Tl][W][ncoord] (every coordinate slot's) and u_mh[Tl][W] of iteration `iter`, in
 *   hens_rj_mh_step's form; birth / death and the cascades: hens_rj_debug_draws. */
int hens_rj_set_gibbs(hens_ctx* ctx, int32_t nblocks, const uint8_t* mask);
int hens_rj_gibbs_select(hens_ctx* ctx, int32_t block);
int hens_rj_gibbs_debug_draws(hens_ctx* ctx, int64_t iter, int32_t block, double* step, double* u_mh);

/* The group stretch move with a stationary friend table on leaf-packing records: the reference's GroupStretchMove (moves/group.py:
 * 122-281, moves/groupstretch.py:34-120) with ONE friend rule, nearest friends by one key parameter per branch (the reference leaves
 * the rule to the user; its own test uses this one).  csrc/hens_rj_group.h states the move in full; in short: the friend table holds,
 * per branch, the active leaves of the cold rung sorted stably by their key parameter; every active leaf of every rung owns a WINDOW
 * of nf = min(nfriends, table entries) contiguous entries around its key (assigned at a rebuild or, for a leaf born since, at the
 * head of the next move; it stays with the leaf, travels with the walker through the swaps and is dropped when the leaf dies); the
 * move stretches every active leaf toward one entry of its window picked uniformly, one stretch factor zz per walker,
 * q = c - (c - x) zz, factors = (ncoord - 1) log zz, all rungs and walkers in one proposal.
 *
 * hens_rj_set_group: nfriends 1 .. 64 (0 clears the group and returns the in-model move of hens_rj_step to the Gaussian one);
 *   n_iter_update >= 2, or >= 1 on a context with live_dangerously (group.py:45-46); key_dim[nbranches], the key parameter of every
 *   branch; a, the stretch scale (> 1).  Every buffer of the move is made here, none per rebuild.  The move's call number restarts
 *   at 0 - so the next hens_rj_step rebuilds the table first - here and at every hens_upload_state; a hens_rj_set_model* call clears
 *   the group.  Refused, the context unchanged: arguments out of range (HENS_ERR_INVALID); before a model, or with a half-step pending
 *   (HENS_ERR_STATE); a model without a device likelihood (hens_rj_set_model_general), more than 64 leaf slots, a Gibbs table
 *   standing (HENS_ERR_UNSUPPORTED) - and, the other way round, hens_rj_set_gibbs and hens_rj_propose of the in-model move while a
 *   group is set.  The table is state that hens_download_state does not carry: a chain resumed in a new context is the uninterrupted
 *   chain only if the resume falls on a rebuild.
 * hens_rj_group_rebuild: the table from the cold rung as it stands, and every active leaf's window from its position now.
 * hens_rj_group_step: the move teacher-forced, parity order of operations: pick i32 [Tl][W][nslots] (nslots = sum_b nleaves_max[b];
 *   read on active leaves, an entry of the leaf's window in [0, nf): values outside are clamped), u_zz / u_acc [Tl][W], keep_out
 *   u8 [Tl][W] or NULL.  It fixes the newborn leaves' windows first and does NOT rebuild: the caller keeps the schedule
 *   (hens_rj_group_rebuild) and follows it with hens_pt_sweep.
 * hens_rj_group_debug: the table and the windows as they stand, any of them NULL: counts i32 [nbranches]; keys [W nslots], branch
 *   b's at offset W sum_{b' < b} nleaves_max[b']; tab [W nslots][4], rows indexed like keys (zeros behind a leaf's width); start i32
 *   [Tl][W][nslots], the first table entry of a slot's window within its branch, -1 where none is assigned.
 * hens_rj_group_debug_draws: what hens_rj_step draws for the move in iteration `iter`, in hens_rj_group_step's form; the picks are
 *   taken against the table as it stands (rj_pick(word, nf); 0 where nf == 0).  Keys: slot s's pick is word x of the Philox call
 *   keyed RJ_GROUP (29) | s << 8, zz's uniform the call keyed RJ_GROUP | 64 << 8, the accept uniform RJ_ACC | 4 << 8. */
int hens_rj_set_group(hens_ctx* ctx, int32_t nfriends, int32_t n_iter_update, const int32_t* key_dim, double a);
int hens_rj_group_rebuild(hens_ctx* ctx);
int hens_rj_group_step(hens_ctx* ctx, const int32_t* pick, const double* u_zz, const double* u_acc, uint8_t* keep_out);
int hens_rj_group_debug(hens_ctx* ctx, int32_t* counts, double* keys, double* tab, int32_t* start);
int hens_rj_group_debug_draws(hens_ctx* ctx, int64_t iter, int32_t* pick, double* u_zz, double* u_acc);

/* Leaf-packing moves with a HOST-CALLABLE likelihood (round 6).  Replaces, for states of several branches / leaves whose
 * log_like_fn is an arbitrary Python function, the proposal + prior half and the accept + update half of MHMove.propose
 * (mh.py:56-193), ReversibleJumpMove.propose (rj.py:145-388) and RedBlueMove.propose (red_blue.py:103-330); between the two
 * the caller does what EnsembleSampler.compute_log_like does on the host (ensemble.py:1306-1334, 1340-1545; utils/utility.py:
 * 8-40 groups_from_inds): packs the active leaves per branch, calls the user's function, fills -1e300 / fill_zero_leaves_val.
 * The leaf-packing twin of hens_propose_split / hens_accept_split.
 *   move   HENS_RJ_MOVE_MH       in-model Gaussian move on every active leaf: draws->step [Tl][W][ncoord], u_acc [Tl][W]
 *          HENS_RJ_MOVE_BD       birth / death on draws->branch: change, leaf [Tl][W], birth [Tl][W][3], u_acc [Tl][W]
 *          HENS_RJ_MOVE_BD_ALL   ... on every branch in one proposal: [nbranches][...] arrays as hens_rj_bd_all_step
 *          HENS_RJ_MOVE_STRETCH  one half of the red / blue stretch move: split, labels, rint, u_zz, u_acc as
 *                                hens_rj_stretch_split
 *   q_out[Tl][W][RW]   the proposed records (every slot's coordinates + the leaf masks, hens_upload_state's layout)
 *   logp_out[Tl][W]    their log-prior, Move.fix_logp_gibbs applied (move.py:368-402): -inf = do not evaluate
 *   moved_out[Tl][W]   1 for the walkers this proposal moves (all of them; a stretch half-step: the moving set)
 * hens_rj_accept(logl[Tl][W]) - the caller's log-likelihoods of the moved walkers (entries of the others are ignored; NaN ->
 * HENS_ERR_NONFINITE, ensemble.py:1542) - runs the tempered accept test and Move.update; keep_out[Tl][W] by WALKER. */
enum { HENS_RJ_MOVE_MH = 0, HENS_RJ_MOVE_BD = 1, HENS_RJ_MOVE_BD_ALL = 2, HENS_RJ_MOVE_STRETCH = 3 };
typedef struct hens_rj_draws {
    const double* step; const int8_t* change; const int32_t* leaf; const double* birth;
    const uint8_t* labels; const int64_t* rint; const double* u_zz; const double* u_acc;
    int32_t branch, split;
} hens_rj_draws;
int hens_rj_propose(hens_ctx* ctx, int32_t move, const hens_rj_draws* draws, double* q_out, double* logp_out, uint8_t* moved_out);
int hens_rj_accept(hens_ctx* ctx, const double* logl, uint8_t* keep_out);

/* The Philox iteration counter: the index of the NEXT iteration hens_step will run (iterations completed on this
 * context so far, by hens_step or by the parity API). */
int hens_get_iteration(hens_ctx* ctx, int64_t* iter_out);

/* Resume: set the Philox iteration counter.  The device draws are a pure function of (seed, iteration, global rung,
 * walker), so a chain continues bit-identically from an uploaded State when the counter (and the adaptation time,
 * hens_set_adapt_time) are restored to the values that State was taken at - the device-side form of the reference's
 * random_state checkpoint (backends/backend.py:1014-1091 stores R's state with every step, ensemble.py:605-647 restores
 * it).  Not on a connected pipeline rank (the ranks' sweep counters would have to move together).  Every call that advances the
 * counter (hens_step and its variants, hens_stretch_iter, the sharded and staged PT steps, the parity API's half-steps, sweeps and
 * MH steps, hens_rj_step, hens_rj_mh_step, hens_rj_stretch_split) fails with HENS_ERR_INVALID before it runs if it would carry the counter past
 * INT64_MAX (the leaf-packing cascades key on 2 iter + 1). */
int hens_set_iteration(hens_ctx* ctx, int64_t iter);

/* Debug / parity: the Philox draws hens_step consumes in iteration `iter` (a pure function of seed, iteration,
 * global rung and walker), exported in a form that maps one-to-one onto the reference's draws so that a
 * production iteration can be replayed through the CPU oracle (tests/test_hip_replay.py):
 *   own, cw [Tl][W] i32   moving walker / its complement walker at every split position; positions < ceil(W/2)
 *                         belong to split 0 and list that half in ascending walker order like the reference's
 *                         boolean masks (red_blue.py:119-124,150-197), so labels[own] = (position >= ceil(W/2)) and
 *                         rint = index of cw in the ascending complement list (stretch.py:93-99)
 *   u_zz, u_acc [Tl][W]   the raw uniforms behind zz (stretch.py:129-132) and the accept test (red_blue.py:294)
 *   pt_slot [T][W] i32    slot of global rung t that cascade column c visits: for pair (i, i-1),
 *                         iperm[k=c] = pt_slot[i][c] and i1perm[k=c] = pt_slot[i-1][c] (tempering.py:526-541)
 *   u_swap [T-1][W]       row j = the uniforms of pair (T-1-j, T-2-j) in column order (tempering.py:535)
 *   is_mh                 1 if the weighted move choice of that iteration (ensemble.py:971) picks the MH move
 *   mh_step [Tl][W][D], mh_u [Tl][W]   the GaussianMove step rows (gaussian.py:166-167,265-268) and accept
 *                         uniforms (mh.py:157), if hens_set_mh_proposal was called.  With hens_set_dist_proposal's
 *                         generator in the MH slot mh_step carries the drawn POINTS q of that iteration (distgen.py:97;
 *                         a pad coordinate reads 0) and mh_u the accept uniforms
 * Any output pointer may be NULL.  Does not touch the sampler state. */
int hens_debug_draws(hens_ctx* ctx, int64_t iter, int32_t* own, int32_t* cw, double* u_zz, double* u_acc,
                     int32_t* pt_slot, double* u_swap, int32_t* is_mh, double* mh_step, double* mh_u);
/* ... of Gibbs block `block` of that iteration's move (hens_set_gibbs): cw, u_zz, u_acc and mh_step, mh_u are the block's; own,
 * pt_slot, u_swap and is_mh the iteration's.  Block 0 is hens_debug_draws.  HENS_ERR_INVALID outside the blocks of that iteration's
 * move.  The arrays of the OTHER move are written only where its table has a block `block` too (the two tables may differ in
 * length): cw, u_zz, u_acc are left untouched for block >= the stretch table's blocks, mh_step, mh_u for block >= the MH table's. */
int hens_debug_draws_block(hens_ctx* ctx, int64_t iter, int32_t block, int32_t* own, int32_t* cw, double* u_zz, double* u_acc,
                           int32_t* pt_slot, double* u_swap, int32_t* is_mh, double* mh_step, double* mh_u);

/* Static description of the build. */
const char* hens_version(void);
int hens_device_count(void);
/* PCI address ("0000:c1:00.0") of HIP device `device_id` - the physical GPU behind an ordinal, whatever the visibility masks say.
 * Host-side helper of the ladder pipeline's one-rank-per-GPU check (eryn_amd/ladder.py; no reference counterpart: the reference is
 * single-process).  Returns HENS_OK and a NUL-terminated string in out[capacity], or a negative error code. */
int hens_device_pci_bus_id(int32_t device_id, char* out, int32_t capacity);

#ifdef __cplusplus
}
#endif
#endif /* HIPENSEMBLE_H */
