"""Production stepping held to the oracle on beta = 0, hand-made and 65+ rung ladders (-m gpu).

Every other replay steps ``make_ladder(D, ntemps=T)`` with T <= 64: geometric, beta_0 = 1, strictly decreasing, strictly positive.
Here the ladder's VALUES and its LENGTH vary (tests/ladders.py: "inf" - a beta = 0 hottest rung; "user" - beta_0 = 0.8, a repeated
pair, a steep gap, last rung 0; "user_pos" - last rung 1e-300; ladders of 65 to 130 rungs), on every launch path that tests against
the ladder or adapts it (``ladders.CASES``), with the adaptation made strong (lag 50, time 10: the ladder moves in its leading
digits within a case, so a cumulative sum in the wrong order or an update on the wrong rung is far outside rtol 1e-13).

``hens_step`` is replayed with the draws it consumed (tests/test_hip_replay._run_case) at the project's bars and nothing new:
positions, log-prior, masks and counters exact, log-likelihood at ``RTOL_L``, betas at rtol 1e-13 / atol 0 - which for a beta = 0
rung means exactly 0 before and after every adaptation.  Every case runs calls of (1, 4) iterations or longer: the folded
adaptation and an adaptation pending at a call's end are both on the path.

Per case, on the oracle's side of the replay (tests/test_ladder_families.py sizes the same cases on the CPU with a factor of two to
spare, ``ladders.check_coverage`` is the one statement of the conditions): something accepted on every rung, the beta = 0 rung
included; swaps on every adjacent pair but the steep gap; every swap of the repeated pair accepted; none across the steep gap; the
beta = 0 rung's proposals leave the box more often than the coldest rung's; the ladder's ends bit-identical to what was uploaded and
the repeated pair still equal - on the oracle and on the device; no decision on the knife edge.  And the launch path: a profiled
call on the same context must report the launches the case is listed under, so a case that moves to another path fails here
instead of passing elsewhere.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import ladders as ld
from tests import parity_utils as pu
from tests import replay_utils as ru
from tests import tolerance_log as tol
from tests.test_hip_hetero_box import _child_env
from tests.test_hip_replay import _run_case

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def rel_betas(betas, ref):
    """largest relative distance of the device's ladder from the oracle's over the rungs that are not 0 (those must be equal)"""
    betas, ref = np.asarray(betas), np.asarray(ref)
    assert np.array_equal(betas == 0.0, ref == 0.0)
    return float(np.max(np.abs(betas - ref)[ref != 0] / ref[ref != 0]))


def assert_path(timing, path, n, what):
    got = {k: timing[k] for k in ("n_stretch", "n_pt", "n_fused")}
    want = {"one": dict(n_stretch=0, n_pt=0, n_fused=n), "two": dict(n_stretch=n, n_pt=0, n_fused=n)}.get(path)
    if want is not None:
        assert got == want, f"{what}: listed under {path!r} launch(es) per iteration, a profiled call of {n} iterations reports {got}"
    else:                              # the copying half-steps (one per set), then the stand-alone cascade
        assert got["n_fused"] == 0 and got["n_pt"] == n and got["n_stretch"] >= 2 * n, f"{what}: listed under the copying launches, reports {got}"


def replay_case(name, family, default_constants=False):
    """One case of ladders.CASES under a ladder family in this process: replay, bars, coverage, path."""
    c = ld.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    betas0, x0, box = ld.case_inputs(c, family)
    rungs, probe = ld.new_stats(T), {}
    kinds = _run_case(T, W, D, like_kind=c["like"], box=box, seed=c["seed"], calls=c["calls"], mh=c["mh"],
                      period=ld.period_of(D) if c["periodic"] else None, nsplits=c["nsplits"], betas=betas0, x0=x0, rungs=rungs, probe=probe,
                      **({} if default_constants else dict(lag=ld.LAG, nu=ld.NU)), **c["kw"])
    assert "stretch" in kinds and (c["mh"] is None or "mh" in kinds)
    st, what = probe["st"], f"{name} / {family}"
    adaptive = c["kw"].get("adaptive", True)
    for betas in (st.betas, probe["betas"]):                    # the oracle says so, and the device must too
        ld.check_coverage(family, T, W, betas0, betas, (st.accepted + st.mh_accepted).sum(axis=1), st.swaps_total, rungs, sum(c["calls"]),
                          adaptive=adaptive, what=what)
    if not default_constants and adaptive:                      # a strong adaptation: far outside the comparison's tolerance
        assert np.max(np.abs(st.betas[1:-1] / betas0[1:-1] - 1.0)) > 1e-6, f"{what}: the ladder hardly moved"
    assert_path(probe["timing"], c["path"], 2, what)
    own = tol.report().get(tol._test_name(), {"max_rel_L": 0.0, "values": 0})      # this case's comparisons (a child: all it made)
    print("max_rel_L %.3e values %d max_rel_betas %.3e" % (own["max_rel_L"], own["values"], rel_betas(probe["betas"], st.betas)))


IN_PROCESS = [(n, f) for n, c in sorted(ld.CASES.items()) if not c["env"] and not c["ranks"] and c["path"] != "sampler" for f in c["families"]]


@pytest.mark.parametrize("name,family", IN_PROCESS)
def test_replay_on_ladder_families(name, family):
    replay_case(name, family)


@pytest.mark.parametrize("name,family", ld.DEFAULT_CONSTANTS)
def test_replay_on_ladder_families_at_the_default_adaptation_constants(name, family):
    """lag 10000, time 100: what a sampler runs unless told otherwise"""
    replay_case(name, family, default_constants=True)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_hip_ladders import replay_case
replay_case(sys.argv[2], sys.argv[3])
"""


def _note_child(r, what):
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"max_rel_L (\S+)(?: values (\d+))?", r.stdout)
    assert m, "the child reported no log-likelihood difference:\n" + r.stdout
    tol.note(float(m.group(1)), int(m.group(2) or 0), what=what)


@pytest.mark.parametrize("name,family", [(n, f) for n, c in sorted(ld.CASES.items()) if c["env"] and not c["ranks"] for f in c["families"]])
def test_replay_on_ladder_families_behind_a_switch(name, family):
    """the persistent, pipelined first launch (k_stretch2, hens_tile2.h) forced onto a small grid, in a fresh child process (the
    library reads its switches once)"""
    c = ld.CASES[name]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, name, family], env=_child_env(c["env"]), capture_output=True, text=True, timeout=300)
    _note_child(r, f"{name} / {family}")
    assert "k_stretch2<pipe=0>" in r.stderr, "the first launches did not go to k_stretch2:\n" + r.stderr[-2000:]


@pytest.mark.parametrize("name,family", [(n, f) for n, c in sorted(ld.CASES.items()) if c["ranks"] for f in c["families"]])
def test_replay_on_ladder_families_pipeline_ranks(name, family):
    """2 and 4 local ranks of the ladder pipeline against the oracle on the whole ladder: the ladder travels from rank to rank
    through the beta ring, whose "not there yet" is a negative value - a 0 must pass as a value.  A wait that gives up raises in
    the worker (HENS_PIPE_TIMEOUT_S) and fails the case; nothing waits longer."""
    c = ld.CASES[name]
    env = _child_env(dict(c["env"], GPU_MAX_HW_QUEUES="16", HENS_PIPE_TIMEOUT_S="10"))
    r = subprocess.run([sys.executable, os.path.join(HERE, "pipeline_worker.py"), "replay", str(c["ranks"]), str(c["T"]), str(c["W"]),
                        str(c["D"]), str(sum(c["calls"])), f"ladder:{family}:{ld.box_of(c, family)}:{ld.LAG}:{ld.NU}"],
                       env=env, capture_output=True, text=True, timeout=300)
    _note_child(r, f"{name} / {family}")


# ---- leaf-packing states: hens_rj_step ------------------------------------------------------------------------------------------------
def _assert_rj_ladder(o, name, family):
    c = ld.RJ_CASES[name]
    for betas in (o.st.betas, o.betas_device):                  # the oracle says so, and the device must too
        ld.check_rj_coverage(family, c["T"], c["W"], o.betas_uploaded, betas, o.accepted_rung, o.swaps_sum, o.cascades, what=f"{name} / {family}")
    assert o.cascades == 2 * c["iters"]
    print("max_rel_betas %.3e" % rel_betas(o.betas_device, o.st.betas))


RJ_GAUSSIAN = [(n, f) for n, c in sorted(ld.RJ_CASES.items()) if c["in_model"] == "gaussian" for f in c["families"]]


@pytest.mark.parametrize("name,family", RJ_GAUSSIAN)
def test_rj_production_step_on_ladder_families(name, family):
    """hens_rj_step (in-model Gaussian steps, birth / death, both cascades, the adaptation) on the rj fixtures' shapes under a
    beta = 0 rung and a hand-made ladder - the adaptation folded into the next k_rj launch (rj_adapt_wave) - and on a ladder of
    66 rungs: rj_adapt_wave holds a rung per lane, so such a ladder adapts through the stand-alone kernel in front of the next
    launch (hens.hip: rj_launch -> flush_adapt).  An RJ context takes it; it must step it like the oracle."""
    from tests.test_hip_rj import _replay_rj
    c = ld.RJ_CASES[name]
    o = _replay_rj(c["T"], c["W"], c["nl_max"], (0, 0), ndata=60, iters=c["iters"], seed=c["seed"], start_leaves=(2, 1),
                   calls=(3, c["iters"] - 3), betas=ld.ladder(family, c["T"], ld.RJ_D), lag=ld.LAG, nu=ld.NU)
    _assert_rj_ladder(o, name, family)


def test_rj_production_step_with_the_stretch_move_under_a_beta_0_rung():
    """the stretch in-model move (hens_rj_set_in_model) on leaf-packing states"""
    from tests.test_hip_rj_stretch import _replay_stretch
    c = ld.RJ_CASES["rj_stretch_T4_W64"]
    o = _replay_stretch(c["T"], c["W"], c["nl_max"], (0, 0), 60, "separate_branches", c["iters"], seed=c["seed"], start_leaves=(2, 1),
                        betas=ld.ladder("inf", c["T"], ld.RJ_D), lag=ld.LAG, nu=ld.NU)
    _assert_rj_ladder(o, "rj_stretch_T4_W64", "inf")


# ---- sampler level ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ld.CASES["sampler_T6_D8"]["families"])
def test_philox_sampler_on_ladder_families_reports_the_oracles_betas_and_resumes_bit_identically(family):
    """``EnsembleSampler(rng="philox")`` with ``tempering_kwargs=dict(Tmax=np.inf)`` / ``dict(betas=...)``: the ladder every stored
    step reports is the oracle's (replayed with the engine's draws), and a stored chain resumed in a NEW context continues bit
    for bit (tests/test_hip_sampler.py: test_philox_chain_resumes_bit_identically_from_a_stored_state)."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.prior import uniform_dist
    from eryn_amd.state import State
    case = ld.CASES["sampler_T6_D8"]
    T, W, D, n, cut = case["T"], case["W"], case["D"], sum(case["calls"]), 8
    mu, invcov = pu.gaussian_problem(D)
    betas0, x0, box = ld.case_inputs(case, family)
    tk = dict(ntemps=T, Tmax=np.inf) if family == "inf" else dict(betas=betas0.copy())
    tk.update(adaptation_lag=ld.LAG, adaptation_time=ld.NU)

    def sampler():
        return EnsembleSampler(W, D, GaussianLikelihood(mu, invcov), {i: uniform_dist(-box, box) for i in range(D)}, rng="philox",
                               seed=77, tempering_kwargs=dict(tk))

    a = sampler()
    assert np.array_equal(a.temperature_control.betas, betas0)
    whole = [State(st, copy=True) for st in a.sample(x0, iterations=n, store=True)]
    ref = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), -box, box, seed=77)       # (the start's log-probabilities as the device computes them)
    ref.upload(x0, betas=betas0)
    ref.eval_state()
    st = ru.OracleState(*ref.download())
    ref.close()
    rungs, worst = ld.new_stats(T), 0.0
    for k in range(n):
        ru.replay(a.engine, st, k, 1, lambda q: orc.gaussian_log_like(q, mu, invcov), np.full(D, -box), np.full(D, box), lag=ld.LAG, nu=ld.NU,
                  rungs=rungs)
        np.testing.assert_allclose(whole[k].betas, st.betas, rtol=1e-13, atol=0, err_msg=f"betas the sampler reports at stored step {k}")
        worst = max(worst, rel_betas(whole[k].betas, st.betas))
    ru.assert_state_equal(st, whole[-1].branches["model_0"].coords[:, :, 0, :], whole[-1].log_like, whole[-1].log_prior, whole[-1].betas,
                          what=f"sampler on the {family} ladder after {n} iterations")
    ld.check_coverage(family, T, W, betas0, whole[-1].betas, st.accepted.sum(axis=1), st.swaps_total, rungs, n, what=f"sampler / {family}")
    assert st.min_margin > 1e-12
    print("max_rel_betas %.3e" % worst)
    b = sampler()
    first = [State(s, copy=True) for s in b.sample(x0, iterations=cut, store=True)]
    c = sampler()                                                       # a new context: nothing but the stored State travels
    rest = [State(s, copy=True) for s in c.sample(first[-1], iterations=n - cut, store=True)]
    for k, (u, v) in enumerate(zip(whole, first + rest)):
        for f in ("log_like", "log_prior", "betas"):
            assert np.array_equal(getattr(u, f), getattr(v, f)), f"{f} differs at stored step {k}"
        assert np.array_equal(u.branches["model_0"].coords, v.branches["model_0"].coords), f"positions differ at stored step {k}"
        assert u.random_state == v.random_state


def test_rj_philox_sampler_under_a_beta_0_rung_reports_the_oracles_betas_and_resumes_bit_identically():
    """``RJEnsembleSampler(rng="philox", tempering_kwargs=dict(Tmax=np.inf))``: the ladder every stored step reports is the oracle's
    (replayed with the context's draws), its last rung stays 0, and a chain continued in a NEW sampler from the stored State
    (+ iteration counter and adaptation time) is the uninterrupted one."""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, TemplateLikelihood
    from eryn_amd.state import State
    T, W, N, n, cut = 4, 64, 100, 8, 4
    t = np.linspace(-1, 1, N)
    y = 3.0 * np.exp(-((t - 0.1) ** 2) / (2 * 0.1 ** 2)) + 1.0 * np.sin(2 * np.pi * 5.0 * t + 1.0) + 1.5 * np.random.RandomState(3).randn(N)
    names = ["gauss", "sine"]
    priors = {"gauss": {0: uniform_dist(2.5, 3.5), 1: uniform_dist(-1, 1), 2: uniform_dist(0.01, 0.21)},
              "sine": {0: uniform_dist(0.5, 1.5), 1: uniform_dist(1.0, 20.0), 2: uniform_dist(0.0, 2 * np.pi)}}

    def sampler():
        return RJEnsembleSampler(W, {k: 3 for k in names}, TemplateLikelihood({"gauss": "pulse", "sine": "sine"}, t, y, 1.5), priors,
                                 tempering_kwargs=dict(ntemps=T, Tmax=np.inf, adaptation_lag=ld.LAG, adaptation_time=ld.NU),
                                 branch_names=names, nleaves_max={"gauss": 4, "sine": 3},
                                 moves=GaussianLeafMove({k: np.eye(3) * 1e-4 for k in names}), rng="philox", seed=8)

    coords = {"gauss": np.zeros((T, W, 4, 3)), "sine": np.zeros((T, W, 3, 3))}
    inds = {"gauss": np.zeros((T, W, 4), dtype=bool), "sine": np.zeros((T, W, 3), dtype=bool)}
    coords["gauss"][:, :, 0] = [3.0, 0.1, 0.1]
    coords["sine"][:, :, 0] = [1.0, 5.0, 1.0]
    inds["gauss"][:, :, 0] = inds["sine"][:, :, 0] = True
    a = sampler()
    betas0 = a.temperature_control.betas.copy()
    assert betas0[-1] == 0.0 and betas0[0] == 1.0
    a.run_mcmc(State(coords, inds=inds), n, store=True)
    assert all(s.betas[-1] == 0.0 and s.betas[0] == 1.0 for s in a.chain) and not np.array_equal(a.chain[-1].betas, betas0)
    # the ladder every stored step reports is the oracle's, replayed with the draws the sampler's context consumed
    from oracle import eryn_oracle_rj as orj
    from tests.test_hip_rj import _replay_oracle_class
    nl_max, okind = {"gauss": 4, "sine": 3}, {"gauss": orj.KIND_PULSE, "sine": orj.KIND_SINE}
    obr = [orj.Branch(k, okind[k], [(priors[k][i].min_val, priors[k][i].max_val) for i in range(3)], nl_max[k], 0, cov=np.eye(3) * 1e-4)
           for k in names]
    o = _replay_oracle_class()(obr, {k: v.copy() for k, v in coords.items()}, {k: v.copy() for k, v in inds.items()}, t, y, 1.5, None, None,
                               betas0.copy(), adaptation_lag=ld.LAG, adaptation_time=ld.NU)
    offsets, worst = {k: a.engine.off[i] for i, k in enumerate(names)}, 0.0
    for k in range(n):
        o.load(a.engine.debug_draws(k), offsets)
        o.iteration()
        np.testing.assert_allclose(a.chain[k].betas, o.st.betas, rtol=1e-13, atol=0, err_msg=f"betas the sampler reports at stored step {k}")
        worst = max(worst, rel_betas(a.chain[k].betas, o.st.betas))
    tol.check_logl(a.chain[-1].log_like, o.st.L, tol.RTOL_L, f"RJ sampler under a beta = 0 rung after {n} iterations")
    for name in names:
        assert np.array_equal(a.chain[-1].branches_inds[name], o.st.inds[name]), f"leaf masks of {name} after {n} iterations"
    print("max_rel_betas %.3e" % worst)
    b = sampler()
    last = b.run_mcmc(State(coords, inds=inds), cut, store=True)
    c = sampler()                                                       # a new context
    c.engine.set_iteration(b.engine.iteration())
    c.temperature_control.time = b.temperature_control.time
    c.run_mcmc(last, n - cut, store=True)
    for k, (u, v) in enumerate(zip(a.chain, b.chain + c.chain)):
        for name in names:
            assert np.array_equal(u.branches_inds[name], v.branches_inds[name]), f"leaf masks of {name} differ at stored step {k}"
            assert np.array_equal(u.branches_coords[name], v.branches_coords[name], equal_nan=True), f"coordinates of {name} differ at stored step {k}"
        for f in ("log_like", "log_prior", "betas"):
            assert np.array_equal(getattr(u, f), getattr(v, f)), f"{f} differs at stored step {k}"
    for s in (a, b, c):
        s.engine.close()
