"""The stepping kernels' prior-box tests on per-coordinate boxes (-m gpu).

Every other GPU test steps under a scalar, symmetric box that no proposal leaves, so a box test reading the wrong coordinate's
bounds, another row's ballot bits or a pad's (-inf, +inf) interval reads the same verdict.  Here the problem is
``tests/problems.hetero_problem``: scales over three decades, means off 0, every bound a number of its own, pinned coordinates
whose proposals sit exactly ON a bound (inclusive in the reference, prior.py:80-88).

1. ``hens_step`` replayed through the oracle with the draws it consumed (tests/test_hip_replay._run_case, its bars unchanged:
   positions, log-prior, accept / swap / MH counters exact, log-likelihood at ``RTOL_L``, betas at 1e-13, no decision on the knife
   edge, something accepted, something swapped) on every launch path that owns a box test or a row-store decision -
   ``problems.CASES``.  Each case asserts its coverage from the ORACLE's proposals: the share with -inf prior inside
   ``problems.BAND``; every free coordinate the sole offender of a proposal on its lo side and on its hi side; every pinned
   coordinate with accepted stretch proposals exactly on its bound.  (A pad coordinate that offended would reject a proposal the
   oracle, which knows nothing of pads, accepts: the exact replay is that check.)  tests/test_hetero_problem.py holds the
   same cases to an EXPECTED sole-offender count of 20 on the CPU, so a count of zero here is no accident of the draws.
2. A deterministic edge matrix on the evaluation path: coordinate ``w mod D`` of walker ``w`` exactly on lo, exactly on hi, one ulp
   below lo, one ulp above hi - at every row-width class and likelihood; the on-bound state then runs through the teacher-forced
   parity API (a compile-time width, the generic width, a host-likelihood context: k_propose's box test).
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import parity_utils as pu
from tests import problems as pb
from tests import tolerance_log as tol
from tests.test_hip_replay import _run_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KNOBS = ("HENS_TILE2_FORCE", "HENS_TILE2_LOG", "HENS_TILE2_PIPE_WAITS", "HENS_NO_TILE2", "HENS_NO_TILE2_PIPE", "HENS_NO_FUSED",
         "HENS_NO_ITER", "HENS_NO_AQL", "HENS_AQL_RELEASE", "HENS_NO_PAD")


def replay_named(name):
    """One case of problems.CASES in this process: replay, bars, coverage."""
    c = pb.CASES[name]
    prob = pb.case_problem(c)
    cov = pb.new_coverage(c["D"])
    mh = pb.mh_proposal(prob, *c["mh"]) if c["mh"] else None
    kinds = _run_case(c["T"], c["W"], c["D"], seed=c["seed"], calls=c["calls"], mh=mh, nsplits=c["nsplits"], problem=prob,
                      coverage=cov, **c["kw"])
    pb.assert_coverage(cov, prob, what=name)
    assert "stretch" in kinds and (mh is None or "mh" in kinds)
    rep = tol.report()
    print("max_rel_L %.3e values %d" % (max([v["max_rel_L"] for v in rep.values()] + [0.0]), sum(v["values"] for v in rep.values())))


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_hip_hetero_box import replay_named
replay_named(sys.argv[2])
"""


def _child_env(extra):
    env = dict(os.environ, **extra)
    for k in KNOBS:
        if k not in extra:
            env.pop(k, None)
    return env


def _note_child(r, name):
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"max_rel_L (\S+)(?: values (\d+))?", r.stdout)
    assert m, "the child reported no log-likelihood difference:\n" + r.stdout
    tol.note(float(m.group(1)), int(m.group(2) or 0), what=name)


@pytest.mark.parametrize("name", sorted(n for n, c in pb.CASES.items() if not c["env"] and not c["ranks"]))
def test_replay_on_per_coordinate_boxes(name):
    replay_named(name)
    if name.startswith(("one_launch", "two_launch")):        # the launch path the case is named after, on this very problem
        from tests.test_hip_records import _engine, _one_launch
        c = pb.CASES[name]
        eng, *_ = _engine(c["T"], c["W"], c["D"], like_kind="hetero")
        assert _one_launch(eng) == name.startswith("one_launch")
        eng.close()


@pytest.mark.parametrize("name", sorted(n for n, c in pb.CASES.items() if c["env"] and not c["ranks"]))
def test_replay_on_per_coordinate_boxes_behind_a_switch(name):
    """the paths a switch selects, each in a fresh child process (the library reads its switches once): k_stretch2 forced onto a
    small grid with a ragged last tile, the three copying launches (HENS_NO_FUSED=1)"""
    c = pb.CASES[name]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name], env=_child_env(c["env"]), capture_output=True, text=True, timeout=300)
    _note_child(r, name)
    if "HENS_TILE2_FORCE" in c["env"]:
        assert "k_stretch2<pipe=0>" in r.stderr, "the first launches did not go to k_stretch2:\n" + r.stderr[-2000:]


@pytest.mark.parametrize("name", sorted(n for n, c in pb.CASES.items() if c["ranks"]))
def test_replay_on_per_coordinate_boxes_pipeline_ranks(name):
    """2 and 4 local ranks of the ladder pipeline (the PIPE instantiations of both launches) and k_stretch2<PIPE> forced, against the
    oracle on the whole ladder"""
    c = pb.CASES[name]
    env = _child_env(dict(c["env"], GPU_MAX_HW_QUEUES="16", HENS_PIPE_TIMEOUT_S="10"))
    r = subprocess.run([sys.executable, os.path.join(HERE, "pipeline_worker.py"), "replay", str(c["ranks"]), str(c["T"]), str(c["W"]),
                        str(c["D"]), str(sum(c["calls"])), "hetero"], env=env, capture_output=True, text=True, timeout=300)
    _note_child(r, name)
    if "HENS_TILE2_FORCE" in c["env"]:
        assert "k_stretch2<pipe=1>" in r.stderr, "the ranks' first launches did not go to k_stretch2<PIPE>:\n" + r.stderr[-2000:]


# ---- the deterministic edge matrix ------------------------------------------------------------------------------------------------
PLACEMENTS = ("on_lo", "on_hi", "below_lo", "above_hi", "inside")


def edge_state(prob, T, W, outside=True):
    """x[T, W, D] strictly inside the box but for coordinate (w + 3 t) mod D of walker w, which sits exactly on lo, exactly on hi,
    one ulp below lo, one ulp above hi (``outside=False``: on the bound instead) or inside, in turn with every lap of the
    coordinates; -> x, the coordinate, the placement."""
    D = prob.D
    rs = np.random.RandomState(17)
    x = 0.5 * (prob.lo + prob.hi) + 0.25 * (prob.hi - prob.lo) * rs.uniform(-1.0, 1.0, size=(T, W, D))
    t, w = np.meshgrid(np.arange(T), np.arange(W), indexing="ij")
    d = (w + 3 * t) % D
    place = (w // D + t) % len(PLACEMENTS)
    lo, hi = prob.lo[d], prob.hi[d]
    below, above = (np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)) if outside else (lo, hi)
    v = np.select([place == 0, place == 1, place == 2, place == 3], [lo, hi, below, above], default=x[t, w, d])
    x[t, w, d] = v
    return x, d, place


EDGE_WIDTHS = [(5, False), (8, True), (11, True), (16, True), (32, True), (64, True), (70, True), (128, True)]


@pytest.mark.parametrize("like", ["dense", "diag", "rosen"])
@pytest.mark.parametrize("D,pad", EDGE_WIDTHS, ids=lambda v: str(v))
def test_evaluation_on_and_one_ulp_outside_every_bound(D, pad, like):
    """eval_state at every row-width class (generic 5, 8, padded 11, 16, 32, 64, padded 70, 128; the Rosenbrock likelihood is never
    padded) under the heterogeneous box and mean.  On a bound: P == logp_inside, L the oracle's at RTOL_L; one ulp outside: P == -inf,
    L == the fill value -1e300; every walker's neighbours in its tile are walkers of the other placements, held to theirs.  W: every
    (coordinate, placement) occurs, over more than one 64-walker tile and a ragged last one."""
    from eryn_amd.engine import HipEnsemble
    prob = pb.hetero_problem(D, like, pinned=False)
    T, W = 2, len(PLACEMENTS) * D * max(1, -(-128 // (len(PLACEMENTS) * D))) + 37      # whole laps over two tiles or more, + 37
    assert W > 128 and W % 64 != 0
    x, d, place = edge_state(prob, T, W)
    seen = {(int(a), int(b)) for a, b in zip(d.ravel(), place.ravel())}
    assert len(seen) == D * len(PLACEMENTS), "every (coordinate, placement)"
    eng = HipEnsemble(T, W, D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=1, pad_rows=pad)
    eng.upload(x, betas=orc.make_ladder(D, ntemps=T))
    eng.eval_state()
    xd, L, P, _ = eng.download()
    eng.close()
    out = place >= 2
    out &= place < 4
    Lref = np.where(out, -1e300, prob.loglike(x.reshape(-1, D)).reshape(T, W))
    Pref = np.where(out, -np.inf, eng.logp_inside)
    assert np.array_equal(Pref, orc.box_log_prior(x.reshape(-1, D), prob.lo, prob.hi).reshape(T, W)), "the oracle's verdicts"
    assert np.array_equal(xd, x), "positions changed by the evaluation"
    bad = P != Pref
    assert not bad.any(), f"log-prior: {int(bad.sum())} walkers wrong, first (t, w, coordinate, placement) " \
                          f"{[(int(a), int(b), int(d[a, b]), PLACEMENTS[place[a, b]]) for a, b in np.argwhere(bad)[:4]]}"
    assert np.array_equal(L[out], Lref[out]), "fill value outside the box"
    rel = tol.check_logl(L, Lref, tol.RTOL_L, f"eval_state D={D} {like}")
    print(f"edge matrix D={D} {like}: {W * T} walkers, {int(out.sum())} one ulp outside, max_rel_L {rel:.2e}")


def _on_bound_oracle(D, T, W):
    prob = pb.hetero_problem(D, "dense", pinned=False)
    x, d, place = edge_state(prob, T, W, outside=False)      # (the reference refuses a start outside the box)
    o, mu, invcov = pu.make_oracle(T, W, D, problem=prob, x0=x)
    assert np.isfinite(o.P).all()
    return prob, o, mu, invcov


@pytest.mark.parametrize("D,pad", [(32, True), (5, False), (11, True)], ids=lambda v: str(v))
def test_parity_api_from_the_on_bound_state(D, pad):
    """stretch_split / pt_sweep with the oracle's draws (parity_utils.run_parity, its bars) from the edge matrix's on-bound state:
    a compile-time row width, the generic width, a padded row.  Two in five walkers sit on a bound, and whoever proposes from them or
    towards them leaves the box through that coordinate."""
    T, W = 3, 5 * D + 37
    prob, o, mu, invcov = _on_bound_oracle(D, T, W)
    eng = pu.make_engine(o, mu, invcov, problem=prob, pad_rows=pad)
    stats = {}
    outside = 0
    for _ in range(3):
        prev = (o.x.copy(), o.L.copy(), o.P.copy(), o.betas.copy(), o.time)
        o.iteration()
        rec = o.trace[-1]
        outside += sum(int(np.isinf(rec[f"logp{sp}"]).sum()) for sp in (0, 1))
        assert pu.check_iteration(eng, o, rec, prev, teacher_forced=True, stats=stats) == 0
        o.trace.clear()
    eng.close()
    share = outside / (3 * T * W)
    print(f"parity D={D}: {share:.3f} of the proposals outside, max_rel_L {stats.get('max_rel_L', 0.0):.2e}")
    assert pb.BAND[0] <= share <= pb.BAND[1]


def test_host_likelihood_context_from_the_on_bound_state():
    """k_propose's box test (hens_propose_split / hens_accept_split: the proposal, prior and accept test of a context whose
    likelihood is a Python callable): proposals bit for bit the oracle's, the in-prior mask its log-prior's, and with the oracle's
    log-likelihoods handed back the accept mask and the updated state."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import HostLikelihood
    D, T, W = 12, 3, 97
    prob, o, mu, invcov = _on_bound_oracle(D, T, W)
    eng = HipEnsemble(T, W, D, HostLikelihood(prob.loglike, D), prob.lo, prob.hi, a=o.a)
    outside = 0
    for _ in range(3):
        eng.upload(o.x, o.L, o.P, o.betas)
        o.iteration()
        rec = o.trace[-1]
        for sp in (0, 1):
            q, inbox = eng.propose_split(sp, rec["labels"], rec[f"rint{sp}"], rec[f"u_zz{sp}"])
            assert np.array_equal(q, rec[f"q{sp}"]), "proposals"
            assert np.array_equal(inbox, np.isfinite(rec[f"logp{sp}"])), "in-prior mask"
            outside += int((~inbox).sum())
            keep = eng.accept_split(sp, rec[f"logl{sp}"], rec[f"u_acc{sp}"])
            assert np.array_equal(keep, rec[f"keep{sp}"]), "accept mask"
        x, L, P, _ = eng.download()
        assert np.array_equal(x, rec[f"x_after1"]) and np.array_equal(P, rec["P_stretch"]) and np.array_equal(L, rec["L_stretch"])
        o.trace.clear()
    eng.close()
    share = outside / (3 * T * W)
    print(f"host likelihood D={D}: {share:.3f} of the proposals outside")
    assert pb.BAND[0] <= share <= pb.BAND[1]
