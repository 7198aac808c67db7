"""The heads of the C entry points (-m gpu).

``hens_step`` leaves the walkers as packed records (slot or column order, after ``k_iter`` with rows in both pool halves) and the
last cascade's ladder adaptation pending; every other entry point settles what it reads before it reads it (csrc/hens.hip:
``settle``).  Two properties of those heads:

* the boundary is invisible from every entry point: a context that is settled first (a download) and one that is not give the
  same outputs, the same state, and the same chain afterwards, bit for bit - at every representation ``hens_step`` can leave
  behind, and on a leaf-packing context;
* a refused call is refused with the code and the text it always had (the expected strings are written out here).
"""
import ctypes as C

import numpy as np
import pytest

from tests import leaf_kind_cases as cases
from tests import test_hip_rj_chain_store as rjc
from tests.test_hip_records import _engine, _reference_draws, _snapshot

pytestmark = pytest.mark.gpu

MH = ("iso", 0.3, 0.5)
# T, W, D, mh: what hens_step leaves behind
SHAPES = {
    "col_records_aql": (8, 64, 8, None),          # column-ordered records on the AQL queue
    "slot_records_mh": (8, 64, 8, MH),            # slot-ordered records on the HIP stream, MH counters riding along
    "k_iter_mixed_rows": (8, 64, 16, None),       # k_iter: rows in both pool halves
    "no_records_W72": (8, 72, 8, None),           # W no multiple of the 16-column block: copying launches + k_pt_cascade, adaptation pending
}
RJ_CASE = rjc.CASES["one_branch_thin3"]           # the smallest model tests/test_hip_rj_chain_store.py steps


def _flat(out):
    """Every array / scalar of a nested result, in order."""
    if out is None:
        return []
    if isinstance(out, dict):
        return [a for k in sorted(out) for a in _flat(out[k])]
    if isinstance(out, (tuple, list)):
        return [a for v in out for a in _flat(v)]
    return [np.asarray(out)]


def _assert_bits(a, b, what):
    fa, fb = _flat(a), _flat(b)
    assert len(fa) == len(fb), what
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), f"{what}: output {i} differs"


def _set_prior_box_again(e):
    _lib_check(e, e.lib.hens_set_prior_box(e.ctx, _ptr(e._pad(e.lo, -np.inf)), _ptr(e._pad(e.hi, np.inf)), e.logp_inside))


def _upload_own_download(e):
    x, L, P, betas = e.download()
    e.upload(x, L, P, betas)


def _step_marked(e):
    e.step_marked(1, 1)
    return e.marked_counters()


def _step_chain(e):
    e.chain_create(2)
    e.step_chain(1, 2, 1)
    return e.chain_download(), e.chain_totals()


def _ptr(a):
    from eryn_amd._lib import ptr
    return ptr(a)


def _lib_check(e, code):
    from eryn_amd._lib import check
    check(code, e.ctx)


# name -> f(engine, settled: what a settled twin reports as current) -> outputs
ENTRY_POINTS = {
    "download": lambda e, cur: e.download(),
    "counters": lambda e, cur: e.counters(),
    "mh_counters": lambda e, cur: e.mh_counters(),
    "download_betas": lambda e, cur: e.download_betas(),
    "reset_counters": lambda e, cur: e.reset_counters(),
    "set_adapt_time": lambda e, cur: e.set_adapt_time(cur["adapt_time"]),
    "set_iteration": lambda e, cur: e.set_iteration(cur["iteration"]),
    "set_prior_box": lambda e, cur: _set_prior_box_again(e),
    "set_gaussian": lambda e, cur: e.likelihood._install(e.lib, e.ctx),
    "set_mh_proposal": lambda e, cur: e.set_mh_proposal(*(cur["mh"] or (None, None, 0.0))),
    "set_periodic": lambda e, cur: e.set_periodic(None),
    "eval_state": lambda e, cur: e.eval_state(),
    "upload": lambda e, cur: _upload_own_download(e),
    "step_report": lambda e, cur: e.step_report(2, 1),
    "step_marked": lambda e, cur: _step_marked(e),
    "step_chain": lambda e, cur: _step_chain(e),
    "debug_draws": lambda e, cur: e.debug_draws(cur["iteration"], mh=cur["mh"] is not None),
}


@pytest.mark.parametrize("entry", sorted(ENTRY_POINTS))
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_the_boundary_is_invisible_from_every_entry_point(shape, entry):
    T, W, D, mh = SHAPES[shape]
    a, *_ = _engine(T, W, D, mh=mh)
    b, *_ = _engine(T, W, D, mh=mh)
    a.step(3)
    b.step(3)
    b.download()                                                  # B is settled first, A is not
    cur = dict(adapt_time=b.counters()["adapt_time"], iteration=b.iteration(), mh=mh)
    assert cur["iteration"] == a.iteration() == 3
    f = ENTRY_POINTS[entry]
    _assert_bits(f(a, cur), f(b, cur), f"{shape}: {entry} behind step(3)")
    _assert_bits(_snapshot(a, mh is not None), _snapshot(b, mh is not None), f"{shape}: the state behind {entry}")
    a.step(2)
    b.step(2)
    assert a.iteration() == b.iteration()
    _assert_bits(_snapshot(a, mh is not None), _snapshot(b, mh is not None), f"{shape}: step(2) behind {entry}")
    a.close()
    b.close()


def _rj_engine(c=RJ_CASE):
    """The head of tests/test_hip_rj_chain_store.yardstick: the sampler's engine with the start state on it."""
    s = rjc.make_sampler(c)
    eng, st = s.engine, rjc.start_state(c)
    s.temperature_control.betas = np.array(st.betas, dtype=np.float64)
    L, P = s._eval(st.branches_coords, st.branches_inds)
    eng.upload(st.branches_coords, st.branches_inds, L, P, s.temperature_control.betas)
    eng.set_adapt_time(s.temperature_control.time)
    return eng


def _rj_scale(c=RJ_CASE):
    return [np.array([0.02 * (hi - lo) for lo, hi in cases.BOX[k]]) for k in c["kinds"]]


def _rj_step_chain(e):
    e.chain_create(2)
    e.step_chain(1, 2)
    return e.chain_download(), e.chain_totals()


RJ_ENTRY_POINTS = {
    "counters": lambda e: e.counters(),
    "debug_resident": lambda e: e.debug_resident(),
    "set_mh_scale": lambda e: e.set_mh_scale(_rj_scale()),
    "debug_draws": lambda e: e.debug_draws(e.iteration()),
    "step_chain": lambda e: _rj_step_chain(e),
}


@pytest.mark.parametrize("entry", sorted(RJ_ENTRY_POINTS))
def test_the_boundary_is_invisible_on_a_leaf_packing_context(entry):
    a, b = _rj_engine(), _rj_engine()
    a.step(3)
    b.step(3)
    b.counters()                                                  # (a download here re-evaluates and legitimately moves later bits)
    f = RJ_ENTRY_POINTS[entry]
    _assert_bits(f(a), f(b), f"leaf packing: {entry} behind step(3)")
    _assert_bits(_snapshot(a.eng), _snapshot(b.eng), f"leaf packing: the state behind {entry}")
    a.step(2)
    b.step(2)
    assert a.iteration() == b.iteration()
    _assert_bits(_snapshot(a.eng), _snapshot(b.eng), f"leaf packing: step(2) behind {entry}")
    a.close()
    b.close()


# ---- refusals --------------------------------------------------------------------------------------------------------------------
# entry points whose first answer to a null context is HENS_ERR_INVALID "null context"
NULL_CONTEXT = """hens_synchronize hens_set_stream hens_set_periodic hens_set_rosenbrock hens_download_state hens_eval_state
hens_stretch_split hens_propose_split hens_accept_split hens_pt_sweep hens_step hens_set_stretch_scale hens_set_nsplits
hens_step_marked hens_step_report hens_chain_create hens_chain_reset hens_chain_destroy hens_step_chain hens_chain_download
hens_chain_totals hens_chain_moments hens_chain_act hens_chain_stats_ms hens_get_marked_counters hens_get_counters
hens_reset_counters hens_set_adapt_time hens_set_iteration hens_set_profiling hens_debug_trace hens_rj_step hens_rj_mh_step
hens_rj_stretch_split hens_rj_bd_step hens_rj_bd_all_step hens_rj_chain_create hens_rj_chain_reset hens_rj_chain_destroy
hens_rj_step_chain hens_rj_chain_download hens_rj_chain_totals hens_rj_chain_leaves hens_rj_chain_leaf_moments
hens_rj_chain_moments hens_rj_chain_stats_ms hens_rj_set_schedule hens_rj_set_in_model hens_rj_get_counters
hens_rj_debug_resident hens_stretch_iter hens_pt_plan_sharded hens_pt_finish_sharded hens_mh_step hens_set_mh_proposal
hens_get_mh_counters hens_pipe_init hens_pipe_connect_staged hens_pipe_stage hens_comm_destroy""".split()


def _null_call(lib, name):
    from eryn_amd._lib import SIGNATURES
    args = [None] + [0 if t in (C.c_int, C.c_int32, C.c_int64) else 0.0 if t is C.c_double else None for t in SIGNATURES[name][1][1:]]
    return getattr(lib, name)(*args)


def _raw(stage):
    """A dense-Gaussian context as hens_create leaves it, then ``stage`` of: prior box, likelihood constants, a state without logs."""
    from eryn_amd import _lib
    from eryn_amd.engine import HipEnsemble
    from tests import parity_utils as pu
    T, W, D = 2, 16, 8
    e = HipEnsemble.__new__(HipEnsemble)
    e.lib, e.ctx = _lib.load(), C.c_void_p()
    cfg = _lib.HensConfig(ntemps=T, nwalkers=W, ndim=D, ndim_active=0, rung_begin=0, rung_end=T, device_id=0,
                          likelihood_kind=_lib.LIKE_GAUSS_DENSE, tempered=1, live_dangerously=0, adaptive=1, adaptation_delay=0,
                          stop_adaptation=-1, a=2.0, fill_value=-1e300, adaptation_lag=10000.0, adaptation_time=100.0, seed=3)
    _lib.check(e.lib.hens_create(C.byref(cfg), C.byref(e.ctx)), None)
    lo, hi = np.full(D, -50.0), np.full(D, 50.0)
    mu, invcov = pu.gaussian_problem(D)
    mu, invcov = np.ascontiguousarray(mu, dtype=np.float64), np.ascontiguousarray(invcov, dtype=np.float64)
    x, betas = np.zeros((T, W, D)), np.array([1.0, 0.5])
    if stage >= 1:
        _lib.check(e.lib.hens_set_prior_box(e.ctx, _ptr(lo), _ptr(hi), 0.0), e.ctx)
    if stage >= 2:
        _lib.check(e.lib.hens_set_gaussian(e.ctx, _ptr(mu), _ptr(invcov)), e.ctx)
    if stage >= 3:
        _lib.check(e.lib.hens_upload_state(e.ctx, _ptr(x), None, None, _ptr(betas)), e.ctx)
    return e


def _dense():
    return _engine(4, 16, 8)[0]


def _dense_half():
    """... with split 0 of a red / blue move done: a half-step is pending."""
    e = _dense()
    d = _reference_draws(np.random.RandomState(2), 4, 16)
    e.stretch_split(0, d["labels"], d["rint0"], d["u_zz0"], d["u_acc0"])
    return e


def _bare_rj():
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.rj import _TemplateLikelihood
    return HipEnsemble(2, 16, 16, _TemplateLikelihood(16), -1.0, 1.0, tempered=True, live_dangerously=True)


def _rj_nostate():
    return rjc.make_sampler(RJ_CASE).engine


def _rj_noscale():
    """A model and an evaluated state, no in-model step scale."""
    from eryn_amd.rj import RJEngine
    s = rjc.make_sampler(RJ_CASE)
    _, t, y, x, inds, betas = rjc.problem(RJ_CASE)
    e = RJEngine(RJ_CASE["T"], RJ_CASE["W"], s.branches, t, y, rjc.SIGMA, seed=RJ_CASE["seed"])
    s.engine.close()
    e.upload(x, inds, betas=betas)
    e.eval_state()
    return e


SETUPS = {"raw0": lambda: _raw(0), "raw1": lambda: _raw(1), "raw2": lambda: _raw(2), "raw3": lambda: _raw(3), "dense": _dense,
          "dense_half": _dense_half, "bare_rj": _bare_rj, "rj_nostate": _rj_nostate, "rj": _rj_engine, "rj_noscale": _rj_noscale}

_BUF = np.zeros(4096)                              # a non-null argument nobody reads: the call is refused first
_B = _BUF.ctypes.data
_DRAWS = np.zeros(16, dtype=np.int64)             # a hens_rj_draws of nulls
_NEG = np.full(8, -1.0)
_TEMPLATE = "hens_rj_* needs a context created with HENS_LIKE_TEMPLATE"
_MODEL = "hens_rj_set_model first"
_HALF = "a half-step is pending"
_ACCEPT = "hens_rj_accept must follow hens_rj_propose"

# (setup, call(lib, ctx) -> status, exception, the text as csrc/hens.hip has always had it)
REFUSALS = {
    # ready(): in its order
    "ready_prior": ("raw0", lambda l, c: l.hens_eval_state(c), RuntimeError, "prior box not set (hens_set_prior_box)"),
    "ready_like": ("raw1", lambda l, c: l.hens_eval_state(c), RuntimeError, "likelihood constants not set"),
    "ready_state": ("raw2", lambda l, c: l.hens_eval_state(c), RuntimeError, "no state uploaded (hens_upload_state)"),
    "ready_logs": ("raw3", lambda l, c: l.hens_step(c, 1), RuntimeError,
                   "log_like/log_prior not available (upload them or call hens_eval_state)"),
    "ready_state_step": ("raw2", lambda l, c: l.hens_step(c, 1), RuntimeError, "no state uploaded (hens_upload_state)"),
    "ready_state_stretch_split": ("raw2", lambda l, c: l.hens_stretch_split(c, 0, _B, _B, _B, _B, _B), RuntimeError,
                                  "no state uploaded (hens_upload_state)"),
    "ready_state_mh_step": ("raw2", lambda l, c: l.hens_mh_step(c, _B, _B, _B), RuntimeError, "no state uploaded (hens_upload_state)"),
    "ready_state_rj_step": ("raw2", lambda l, c: l.hens_rj_step(c, 1), RuntimeError, "no state uploaded (hens_upload_state)"),
    "download_no_state": ("raw2", lambda l, c: l.hens_download_state(c, _B, _B, _B, _B), RuntimeError, "no state uploaded"),
    "upload_half_logs": ("raw2", lambda l, c: l.hens_upload_state(c, _B, _B, None, _B), ValueError, "give both logl and logp or neither"),
    "upload_no_betas": ("raw2", lambda l, c: l.hens_upload_state(c, _B, None, None, None), ValueError, "betas required for a tempered context"),
    # "hens_rj_set_model first": its seven entry points
    "model_set_mh_scale": ("bare_rj", lambda l, c: l.hens_rj_set_mh_scale(c, _B), RuntimeError, _MODEL),
    "model_set_mh_chol": ("bare_rj", lambda l, c: l.hens_rj_set_mh_chol(c, _B), RuntimeError, _MODEL),
    "model_debug_draws_stretch": ("bare_rj", lambda l, c: l.hens_rj_debug_draws_stretch(c, 0, _B, _B, _B, _B), RuntimeError, _MODEL),
    "model_debug_draws": ("bare_rj", lambda l, c: l.hens_rj_debug_draws(c, 0, *([_B] * 11)), RuntimeError, _MODEL),
    "model_get_counters": ("bare_rj", lambda l, c: l.hens_rj_get_counters(c, _B, _B, _B), RuntimeError, _MODEL),
    "model_debug_resident": ("bare_rj", lambda l, c: l.hens_rj_debug_resident(c, _B, _B), RuntimeError, _MODEL),
    "model_chain_create": ("bare_rj", lambda l, c: l.hens_rj_chain_create(c, 4, 0), RuntimeError, "hens_rj_chain_*: no model (hens_rj_set_model first)"),
    # ... and the same entry points on a context of another likelihood kind
    "model_set_mh_scale_dense": ("dense", lambda l, c: l.hens_rj_set_mh_scale(c, _B), RuntimeError, _MODEL),
    "model_get_counters_dense": ("dense", lambda l, c: l.hens_rj_get_counters(c, _B, _B, _B), RuntimeError, _MODEL),
    "model_debug_resident_dense": ("dense", lambda l, c: l.hens_rj_debug_resident(c, _B, _B), RuntimeError, _MODEL),
    "model_debug_draws_dense": ("dense", lambda l, c: l.hens_rj_debug_draws(c, 0, *([_B] * 11)), RuntimeError, _MODEL),
    # the HENS_LIKE_TEMPLATE refusal, distinct from it
    "template_propose": ("dense", lambda l, c: l.hens_rj_propose(c, 0, _DRAWS.ctypes.data, _B, _B, _B), RuntimeError, _TEMPLATE),
    "template_rj_step": ("dense", lambda l, c: l.hens_rj_step(c, 1), RuntimeError, _TEMPLATE),
    "template_rj_mh_step": ("dense", lambda l, c: l.hens_rj_mh_step(c, _B, _B, _B), RuntimeError, _TEMPLATE),
    "template_set_schedule": ("dense", lambda l, c: l.hens_rj_set_schedule(c, 0), RuntimeError, _TEMPLATE),
    "template_set_in_model": ("dense", lambda l, c: l.hens_rj_set_in_model(c, 0), RuntimeError, _TEMPLATE),
    "template_set_model": ("dense", lambda l, c: l.hens_rj_set_model(c, 1, _B, _B, _B, _B, _B, _B, 8, _B, _B, 1.0), RuntimeError,
                           "hens_rj_set_model needs HENS_LIKE_TEMPLATE"),
    "template_set_model_general": ("dense", lambda l, c: l.hens_rj_set_model_general(c, 1, _B, _B, _B, _B, _B, _B), RuntimeError,
                                   "hens_rj_set_model_general needs HENS_LIKE_TEMPLATE"),
    "template_chain_create": ("dense", lambda l, c: l.hens_rj_chain_create(c, 4, 0), NotImplementedError,
                              "hens_rj_chain_*: the chain store of a leaf-packing context (HENS_LIKE_TEMPLATE); others: hens_chain_create / hens_step_chain"),
    # protocol state
    "accept_without_propose": ("rj", lambda l, c: l.hens_rj_accept(c, _B, _B), RuntimeError, _ACCEPT),
    "half_set_iteration": ("dense_half", lambda l, c: l.hens_set_iteration(c, 0), RuntimeError, _HALF),
    "half_set_stretch_scale": ("dense_half", lambda l, c: l.hens_set_stretch_scale(c, 2.0), RuntimeError, _HALF),
    "half_step": ("dense_half", lambda l, c: l.hens_step(c, 1), RuntimeError, "hens_step between split 0 and split 1"),
    "half_stretch_iter": ("dense_half", lambda l, c: l.hens_stretch_iter(c), RuntimeError, "hens_stretch_iter between split 0 and split 1"),
    "half_mh_step": ("dense_half", lambda l, c: l.hens_mh_step(c, _B, _B, _B), RuntimeError, "hens_mh_step between split 0 and split 1"),
    "half_pt_sweep": ("dense_half", lambda l, c: l.hens_pt_sweep(c, _B, _B, _B, 1, _B, _B), RuntimeError, "PT sweep between split 0 and split 1"),
    "half_set_nsplits": ("dense_half", lambda l, c: l.hens_set_nsplits(c, 2), RuntimeError, "a red-blue move is under way"),
    "marked_without_mark": ("dense", lambda l, c: l.hens_get_marked_counters(c, _B, _B), RuntimeError,
                            "hens_get_marked_counters without hens_step_marked"),
    "trace_not_enabled": ("dense", lambda l, c: l.hens_debug_trace(c, 0, _B, 8, _B), RuntimeError, "tracing was not enabled"),
    "resident_no_state": ("rj_nostate", lambda l, c: l.hens_rj_debug_resident(c, _B, _B), RuntimeError, "no state uploaded"),
    "rj_download_no_state": ("rj_nostate", lambda l, c: l.hens_download_state(c, _B, _B, _B, _B), RuntimeError, "no state uploaded"),
    # the checks in front of a settle, entry point by entry point
    "prior_box_empty": ("dense", lambda l, c: l.hens_set_prior_box(c, _B, _B, 0.0), ValueError,
                        "prior box needs lo < hi in every dimension (dim 0)"),
    "prior_box_null": ("dense", lambda l, c: l.hens_set_prior_box(c, None, _B, 0.0), ValueError, "null argument"),
    "periodic_negative": ("dense", lambda l, c: l.hens_set_periodic(c, _NEG.ctypes.data), ValueError,
                          "period of dimension 0 must be finite and >= 0"),
    "periodic_records": ("bare_rj", lambda l, c: l.hens_set_periodic(c, None), NotImplementedError,
                         "periodic parameters are not defined on leaf-packing records"),
    "gaussian_kind": ("bare_rj", lambda l, c: l.hens_set_gaussian(c, _B, _B), RuntimeError, "context was not created with a Gaussian likelihood kind"),
    "rosenbrock_kind": ("dense", lambda l, c: l.hens_set_rosenbrock(c, 1.0, 100.0), RuntimeError, "context was not created with HENS_LIKE_ROSENBROCK"),
    "stretch_split_null": ("dense", lambda l, c: l.hens_stretch_split(c, 0, _B, _B, _B, None, _B), ValueError, "null argument"),
    "propose_split_kind": ("dense", lambda l, c: l.hens_propose_split(c, 0, _B, _B, _B, _B, _B), RuntimeError,
                           "hens_propose_split needs a context created with HENS_LIKE_HOST"),
    "accept_split_order": ("dense", lambda l, c: l.hens_accept_split(c, 0, _B, _B, _B), RuntimeError,
                           "hens_accept_split must follow hens_propose_split of the same split"),
    "pt_sweep_null": ("dense", lambda l, c: l.hens_pt_sweep(c, None, _B, _B, 1, _B, _B), ValueError, "null argument"),
    "step_negative": ("dense", lambda l, c: l.hens_step(c, -1), ValueError, "n_iters < 0"),
    "step_marked_negative": ("dense", lambda l, c: l.hens_step_marked(c, -1, 1), ValueError, "negative iteration count"),
    "step_report_n_last": ("dense", lambda l, c: l.hens_step_report(c, 1, 2, _B, _B, _B), ValueError, "hens_step_report: 1 <= n_last <= n_iters"),
    "step_chain_no_chain": ("dense", lambda l, c: l.hens_step_chain(c, 1, 1, 1), RuntimeError, "no chain (hens_chain_create)"),
    "chain_totals_no_chain": ("dense", lambda l, c: l.hens_chain_totals(c, _B, _B), RuntimeError, "no chain (hens_chain_create)"),
    "set_iteration_negative": ("dense", lambda l, c: l.hens_set_iteration(c, -1), ValueError, "iteration counter < 0"),
    "debug_draws_negative": ("dense", lambda l, c: l.hens_debug_draws(c, -1, *([None] * 9)), ValueError, "null context / negative iteration"),
    "mh_step_null": ("dense", lambda l, c: l.hens_mh_step(c, None, _B, _B), ValueError, "null argument"),
    "mh_proposal_kind": ("dense", lambda l, c: l.hens_set_mh_proposal(c, 5, _B, 0.5), ValueError,
                         "kind must be 0 (isotropic), 1 (diagonal) or 2 (full) with its scale"),
    "mh_proposal_weight": ("dense", lambda l, c: l.hens_set_mh_proposal(c, 0, _B, 1.5), ValueError, "weight must be a probability"),
    "pt_finish_none": ("dense", lambda l, c: l.hens_pt_finish_sharded(c, 0), RuntimeError, "no sharded PT exchange in flight"),
    "pt_plan_null": ("dense", lambda l, c: l.hens_pt_plan_sharded(c, None, None, None, 1, None, 1, 0, _B, _B, None, None), ValueError, "null argument"),
    "device_buffers_null": ("dense", lambda l, c: l.hens_get_device_buffers(c, None), ValueError, "null argument"),
    "pipe_init_ranks": ("dense", lambda l, c: l.hens_pipe_init(c, 0, 0, None, None), ValueError, "nranks must be in [1, 56] and my_rank inside it"),
    "pipe_connect_first": ("dense", lambda l, c: l.hens_pipe_connect(c, _B), RuntimeError, "hens_pipe_init first"),
    "pipe_connect_staged_first": ("dense", lambda l, c: l.hens_pipe_connect_staged(c), RuntimeError, "hens_pipe_init first"),
    "pipe_stage_first": ("dense", lambda l, c: l.hens_pipe_stage(c, 0), RuntimeError, "hens_pipe_connect_staged first"),
    "rj_step_negative": ("rj", lambda l, c: l.hens_rj_step(c, -1), ValueError, "n_iters < 0"),
    "rj_step_no_scale": ("rj_noscale", lambda l, c: l.hens_rj_step(c, 1), RuntimeError, "in-model step scale not set (hens_rj_set_mh_scale)"),
    "rj_debug_draws_no_scale": ("rj_noscale", lambda l, c: l.hens_rj_debug_draws(c, 0, *([_B] * 11)), RuntimeError,
                                "in-model step scale not set (hens_rj_set_mh_scale)"),
    "rj_mh_step_null": ("rj", lambda l, c: l.hens_rj_mh_step(c, None, _B, _B), ValueError, "null argument"),
    "rj_step_chain_no_chain": ("rj", lambda l, c: l.hens_rj_step_chain(c, 1, 1), RuntimeError, "no chain (hens_rj_chain_create)"),
    "rj_set_model_data": ("rj", lambda l, c: l.hens_rj_set_model(c, 1, _B, _B, _B, _B, _B, _B, 8, _B, _B, 0.0), ValueError, "invalid data"),
    "rj_set_model_general_branches": ("rj", lambda l, c: l.hens_rj_set_model_general(c, 0, _B, _B, _B, _B, _B, _B), ValueError, "1..4 branches"),
    "rj_propose_move": ("rj", lambda l, c: l.hens_rj_propose(c, 9, _DRAWS.ctypes.data, _B, _B, _B), ValueError,
                        "hens_rj_propose: move must be HENS_RJ_MOVE_MH, _BD, _BD_ALL or _STRETCH"),
}


@pytest.fixture(scope="module")
def contexts():
    made = {}

    def get(name):
        if name.startswith("raw") or name not in made:        # (a raw context is made afresh: its stages are the case)
            made.setdefault(name, []).append(SETUPS[name]())
        return made[name][-1]

    yield get
    for engines in made.values():
        for e in engines:
            e.close()


@pytest.mark.parametrize("case", sorted(REFUSALS) + ["null:" + n for n in NULL_CONTEXT])
def test_refusals_are_what_they_were(contexts, case):
    from eryn_amd import _lib
    lib = _lib.load()
    if case.startswith("null:"):
        assert _null_call(lib, case[5:]) == _lib.ERR_INVALID
        with pytest.raises(ValueError) as e:
            _lib.check(_lib.ERR_INVALID, None)
        assert str(e.value) == "null context"
        return
    setup, call, exc, text = REFUSALS[case]
    eng = contexts(setup)
    before = eng.iteration() if hasattr(eng, "iteration") else None
    with pytest.raises(exc) as e:
        _lib.check(call(lib, eng.ctx), eng.ctx)
    assert type(e.value) is exc and str(e.value) == text
    assert before is None or eng.iteration() == before
