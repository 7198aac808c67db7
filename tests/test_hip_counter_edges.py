"""The production chains replayed through the oracle where the iteration counter has edges (-m gpu).

The other replays start at iteration 0 and run a few iterations.  State that depends on the counter is reached here:

A. the round-key window (hens.hip: iteration_keys, KEY_WINDOW = 1024 iterations planned at once, planned again when iteration
   + 1 leaves the window, i.e. at 1023): each production family stepped to 1016 in one unobserved call, then replayed across the
   edge in calls that end right before 1023, are the single iteration 1023, and go on - or in one call across it;
B. the 64-bit counter inside 32-bit Philox words: chains resumed (hens_set_iteration) just below 2^31, 2^32 and a counter with a
   large high word; the leaf-packing cascades, keyed on 2 iter and 2 iter + 1, across 2^31 - 1 -> 2^31 and 2^32; the top of the
   range, where a call that would pass INT64_MAX is refused;
C. the resident templates of hens_rj_step, refreshed from the coordinates when iter % 64 == 63: replayed with no download between
   calls (a download refreshes them), and their drift measured against the exact float64 likelihood just before a refresh.

Bars as in tests/test_hip_replay.py and tests/test_hip_rj.py: positions, log-priors and counters exact, log-likelihoods within
tolerance_log.RTOL_L (1e-12 for the leaf-packing models), betas rtol 1e-13."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.test_hip_replay import _run_case
from tests.test_hip_rj import _replay_rj

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE = 1023                      # the iteration whose step plans the next round-key window


def _path(T, W, D, mh=None, nsplits=2, it=EDGE - 3, n=4):
    """Launch counts and window plans of ``n`` profiled iterations from ``it`` on a context set up like _run_case's: the path
    the family takes at the edge (hens_set_profiling(1): a HIP event pair per launch, as tests/test_hip_records._one_launch)."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from oracle import eryn_oracle as orc
    from tests import parity_utils as pu
    mu, invcov = pu.gaussian_problem(D, dense=True)
    eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), -50.0, 50.0, seed=77)
    eng.upload(np.clip(np.random.RandomState(3).randn(T, W, D), -47.5, 47.5), betas=orc.make_ladder(D, ntemps=T))
    eng.eval_state()
    if mh is not None:
        eng.set_mh_proposal(*mh)
    if nsplits != 2:
        eng.set_nsplits(nsplits)
    eng.set_iteration(it)
    eng.set_profiling(True)
    eng.step(n)
    tm = eng.timing()
    eng.set_profiling(False)
    rw = eng.RW
    eng.close()
    return tm, rw


def _edge(T, W, D, calls, start=EDGE - 7, **kw):
    """Replay ``calls`` from ``start`` (reached by one unobserved call) and return the calls' (first iteration, n, window plans in
    the call, window plans of the state read-back after it)."""
    plans = []
    kinds = _run_case(T, W, D, calls=calls, start_iter=start, plans=plans, **kw)
    assert sum(p[1] for p in plans) == sum(calls)
    return kinds, plans


def _assert_window_planned_at_the_edge(plans, per_call=False):
    """Two-launch iteration: the window is planned again exactly once in the replayed stretch - inside the call when one call runs
    across the edge; with split calls either inside the call of iteration 1023 or by the read-back in front of it (column-ordered
    records are unpacked in the order of iteration 1023, whose keys lie in the next window), never earlier, never twice.
    One-launch iteration (``per_call``): k_iter's calls plan their keys at their head, once per call, and nothing else does."""
    if per_call:
        assert all(p[2] == 1 and p[3] == 0 for p in plans), plans
        return
    assert sum(p[2] + p[3] for p in plans) == 1, plans
    for it0, n, in_call, after in plans:
        if in_call:
            assert it0 <= EDGE < it0 + n, plans
        if after:
            assert it0 + n == EDGE, plans


# ---- A: the round-key window's edge ------------------------------------------------------------------------------------------
def test_window_edge_two_launch_config2():
    """k_stretch_fast + k_split1_pt<COL> (config 2, column-ordered records written in the NEXT iteration's order)."""
    tm, _ = _path(16, 4096, 32)
    assert tm["n_stretch"] == 4 and tm["n_fused"] == 4, tm
    for calls in ((2, 1, 2), (5,)):
        _, plans = _edge(16, 4096, 32, calls=calls, start=EDGE - 2)
        _assert_window_planned_at_the_edge(plans)


_STRETCH2 = r"""
import sys
sys.path.insert(0, sys.argv[1])
import torch  # noqa: F401  (before libhipensemble)
from tests.test_hip_counter_edges import _edge, _assert_window_planned_at_the_edge, EDGE
_, plans = _edge(8, 16384, 64, calls=(2, 1, 2), start=EDGE - 2)
_assert_window_planned_at_the_edge(plans)
print("plans", plans)
"""


def test_window_edge_persistent_first_launch():
    """k_stretch2 (hens_tile2.h) at the config-3 shard's shape, which selects it by default: the launches of the replayed
    iterations around the edge are logged (HENS_TILE2_LOG=1) as k_stretch2's."""
    env = dict(os.environ, HENS_TILE2_LOG="1")
    for k in ("HENS_NO_TILE2", "HENS_TILE2_FORCE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-c", _STRETCH2, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    its = sorted({int(ln.rsplit("iter ", 1)[1]) for ln in r.stderr.splitlines() if "k_stretch2<pipe=0>" in ln and "iter " in ln})
    assert set(range(EDGE - 2, EDGE + 3)) <= set(its), "the first launches around the edge did not go to k_stretch2:\n" + r.stderr[-2000:]


@pytest.mark.parametrize("calls", [(7, 1, 8), (16,)])
def test_window_edge_one_launch(calls):
    """k_iter (8 x 4096 x 32: one workgroup per CU), in calls split at the edge and in one call across it."""
    tm, _ = _path(8, 4096, 32)
    assert tm["n_stretch"] == 0 and tm["n_fused"] == 4, tm
    _, plans = _edge(8, 4096, 32, calls=calls)
    _assert_window_planned_at_the_edge(plans, per_call=True)


def test_window_edge_short_tiles():
    """ntemps = 10 does not divide 128: cb T = 80 slots per workgroup, through the two-launch iteration (512 workgroups)."""
    tm, _ = _path(10, 4096, 32)
    assert tm["n_stretch"] == 4 and tm["n_fused"] == 4, tm
    _, plans = _edge(10, 4096, 32, calls=(7, 1, 8), x_scale=0.7)
    _assert_window_planned_at_the_edge(plans)


@pytest.mark.parametrize("calls", [(7, 1, 8), (16,)])
def test_window_edge_padded_rows(calls):
    """D = 11 padded to the compile-time width 16 (zero columns under an unbounded prior), one launch per iteration."""
    tm, rw = _path(8, 2048, 11)
    assert rw == 16 and tm["n_stretch"] == 0 and tm["n_fused"] == 4, (rw, tm)
    _, plans = _edge(8, 2048, 11, calls=calls)
    _assert_window_planned_at_the_edge(plans, per_call=True)


def test_window_edge_move_mix():
    """StretchMove + GaussianMove by weight: both kinds run inside the replayed window."""
    mh = ("iso", 0.3, 0.5)
    tm, _ = _path(8, 256, 32, mh=mh)
    assert tm["n_fused"] > 0, tm
    kinds, plans = _edge(8, 256, 32, calls=(7, 1, 8), mh=mh)
    assert "mh" in kinds and "stretch" in kinds
    _assert_window_planned_at_the_edge(plans, per_call=True)


def test_window_edge_three_sets():
    """RedBlueMove(nsplits = 3): keyed labels mod 3 across the edge, through the copying launches (the fused ones are two-set)."""
    tm, _ = _path(4, 1000, 32, nsplits=3)
    assert tm["n_fused"] == 0 and tm["n_stretch"] >= 3 * 4, tm
    _edge(4, 1000, 32, calls=(7, 1, 8), nsplits=3)


def test_window_edge_local_pipeline():
    """Two ranks of the ladder pipeline on one GPU: each rank plans the round keys of its rungs and of the rung below them."""
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16", HENS_PIPE_TIMEOUT_S="10")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "pipeline_worker.py"), "replay_from", "2", "8", "256", "32",
                        str(EDGE - 7), "7,1,8"], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "replay_from ok" in r.stdout


# ---- B: carries of the 64-bit counter ------------------------------------------------------------------------------------------
CARRIES = [(1 << 31) - 2, (1 << 32) - 2, (1 << 40) + (1 << 32) - 3]


@pytest.mark.parametrize("start", CARRIES)
@pytest.mark.parametrize("T,W,D,mh", [(10, 4096, 32, None), (8, 4096, 32, None), (8, 256, 32, ("iso", 0.3, 0.5))],
                         ids=["two_launch", "one_launch", "move_mix"])
def test_counter_carry(T, W, D, mh, start):
    """A chain resumed just below a carry of the low Philox word (2^31: an int's sign bit; 2^32; a large high word) and replayed
    across it, the adaptation time moved with the counter.  The families' paths at the carry are asserted from their launch counts
    (at D = 32 there is no k_stretch2: its instantiations are D = 64 only)."""
    tm, _ = _path(T, W, D, mh=mh, it=start, n=4)
    if mh is not None:
        assert tm["n_fused"] > 0, tm
    elif T == 10:
        assert tm["n_stretch"] == 4 and tm["n_fused"] == 4, tm
    else:
        assert tm["n_stretch"] == 0 and tm["n_fused"] == 4, tm
    kinds = _run_case(T, W, D, calls=(1, 3) if mh is None else (3, 6), set_iter=start, mh=mh)
    if mh is not None:
        assert "mh" in kinds


@pytest.mark.parametrize("T,W,D,mh", [(4, 512, 64, None), (8, 256, 32, ("iso", 0.3, 0.5))])
def test_top_of_the_counter_range(T, W, D, mh):
    """At 2^63 - 2 a call of 4 iterations would carry the counter past INT64_MAX: it is refused and leaves the counter where it
    was; the one iteration that remains replays correctly, and then no call of a single iteration runs."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from oracle import eryn_oracle as orc
    top = (1 << 63) - 2
    eng = HipEnsemble(T, W, D, GaussianLikelihood(np.zeros(D), np.ones(D)), -50.0, 50.0, seed=3)
    eng.upload(np.random.RandomState(0).randn(T, W, D), betas=orc.make_ladder(D, ntemps=T))
    eng.eval_state()
    eng.set_iteration(top)
    with pytest.raises(ValueError, match="INT64_MAX"):
        eng.step(4)
    assert eng.iteration() == top
    eng.step(1)
    with pytest.raises(ValueError, match="INT64_MAX"):
        eng.step(1)
    assert eng.iteration() == top + 1
    eng.close()
    _run_case(T, W, D, calls=(1,), set_iter=top, mh=mh)


def test_parity_moves_at_the_top_of_the_counter_range():
    """On an untempered context the parity API's moves advance the counter themselves (the last half-step of hens_stretch_split,
    hens_mh_step): at INT64_MAX they are refused before they run and the counter stays."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    T, W, D = 1, 64, 4
    eng = HipEnsemble(T, W, D, GaussianLikelihood(np.zeros(D), np.ones(D)), -50.0, 50.0, seed=3)
    eng.upload(np.random.RandomState(0).randn(T, W, D))
    eng.eval_state()
    top = (1 << 63) - 1
    eng.set_iteration(top)
    with pytest.raises(ValueError, match="INT64_MAX"):
        eng.mh_step(np.zeros((T, W, D)), np.full((T, W), 0.5))
    Ns = eng.set_size(0)
    with pytest.raises(ValueError, match="INT64_MAX"):
        eng.stretch_split(0, np.arange(W)[None, :] % 2, np.zeros((T, Ns), dtype=np.int64), np.full((T, Ns), 0.5), np.full((T, Ns), 0.5))
    assert eng.iteration() == top
    x, L, P, _ = eng.download()
    assert np.isfinite(L).all()
    eng.close()


# ---- B / C: the leaf-packing path --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", [(1 << 31) - 2, (1 << 32) - 2, (1 << 63) - 10])
def test_rj_counter_carry(start):
    """The RJ cascades key on 2 iter (+ 1): at iter = 2^31 the product carries into the high word; near the top of the range it
    is close to 2^64 (hens_rj_debug_draws forms the same key in unsigned arithmetic)."""
    _replay_rj(3, 16, (3, 3), (0, 0), ndata=60, iters=8, seed=11, calls=(1, 7), set_iter=start, downloads=False)


def test_rj_top_of_the_counter_range():
    """2 iter would wrap to iteration 0's keys at 2^63: a call that would get there is refused, the counter unchanged."""
    from eryn_amd.rj import RJEngine, TemplateBranch
    t = np.linspace(-1, 1, 40)
    brs = [TemplateBranch("gauss", "pulse", [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], 3)]
    eng = RJEngine(2, 8, brs, t, np.zeros_like(t), 2.0, seed=1)
    x = {"gauss": np.zeros((2, 8, 3, 3)) + [3.0, 0.0, 0.1]}
    inds = {"gauss": np.zeros((2, 8, 3), dtype=bool)}
    inds["gauss"][..., 0] = True
    eng.upload(x, inds, betas=np.array([1.0, 0.5]))
    eng.eval_state()
    eng.set_mh_scale(np.full((1, 3), 1e-2))
    eng.set_iteration((1 << 63) - 2)
    with pytest.raises(ValueError, match="INT64_MAX"):
        eng.step(4)
    assert eng.iteration() == (1 << 63) - 2
    eng.step(1)
    assert eng.iteration() == (1 << 63) - 1
    with pytest.raises(ValueError, match="INT64_MAX"):
        eng.step(1)
    with pytest.raises(ValueError, match="INT64_MAX"):              # (the parity API's in-model move too)
        eng.mh_step({"gauss": np.zeros((2, 8, 3, 3))}, np.full((2, 8), 0.5))
    assert eng.iteration() == (1 << 63) - 1
    eng.close()


def test_rj_refresh_inside_one_long_call():
    """140 iterations in ONE call from iteration 0: the resident templates are refreshed at 63 and 127 inside the call."""
    _replay_rj(3, 16, (3, 3), (0, 0), ndata=60, iters=140, seed=11, downloads=False)


@pytest.mark.parametrize("schedule", ["separate_branches", "iterate_branches", "together"])
def test_rj_refresh_is_a_call_of_its_own(schedule):
    """From iteration 60 in calls of 3, 1, 6 without downloads: the second call is exactly iteration 63, whose head refreshes
    the templates; on a uniform grid of 130 points (the recurrences of the production likelihood)."""
    res = {}
    _replay_rj(3, 12, (4, 3), (0, 0), ndata=130, iters=10, seed=19, start_leaves=(2, 2), calls=(3, 1, 6), schedule=schedule,
               set_iter=60, downloads=False, resident=res)
    assert sorted(res) == [63, 64, 70]


BIG = 40.0                       # amplitude of the wide box's starting pulse, over data of order 1


@pytest.mark.parametrize("pulse_amp,inj_amp,start_amp", [((2.5, 3.5), None, None), ((0.1, 100.0), (1.0, 1.0), {"gauss": [1.0, BIG]})],
                         ids=["test_box", "wide_box"])
def test_rj_resident_drift_before_a_refresh(pulse_amp, inj_amp, start_amp):
    """The resident log-likelihoods after 63 iterations of +- leaf updates (iterations 0 .. 62, the refresh at 63 not yet run)
    against orj.compute_log_like of the same coordinates in float64 - with the tests' amplitude box and with a wide one: pulses of
    amplitude up to 100 over data of order 1, every walker starting with one pulse of amplitude 40 that the data do not hold.  Its
    in-model moves and its death subtract it from a template it was added to (where the template cancels); the oracle's chain
    shows that the death happened inside the window."""
    res = {}
    o = _replay_rj(4, 16, (4, 3), (0, 0), ndata=130, iters=63, seed=23, start_leaves=(2, 1), calls=(63,), downloads=False,
                   pulse_amp=pulse_amp, inj_amp=inj_amp, start_amp=start_amp, resident=res)
    print(f"resident log-likelihood drift after 63 iterations ({pulse_amp}): {res[63]:.3e}")      # (bar: inside _replay_rj)
    if start_amp is not None:
        big_alive = (o.st.inds["gauss"] & (o.st.x["gauss"][..., 0] > BIG / 4)).any(axis=-1)
        print(f"walkers whose amplitude-{BIG:g} pulse died within the window: {int((~big_alive).sum())} of {big_alive.size}")
        assert (~big_alive).sum() >= big_alive.size // 2, "the large pulses were not removed: the case does not test the cancellation"
