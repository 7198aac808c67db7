"""The multiple-try birth / death move (MTDistGenMoveRJ) on the device (-m gpu): hens_rj_set_mt_proposal, hens_rj_mt_bd_step, the k_rj_mt
launch of hens_rj_step and eryn_amd.rj.MTDistGenMoveRJ against the specification tests/rj_mt_move.py.  The cases and their seeds are
sized on the specification alone (tests/test_rj_mt_move.py): no decision on a knife edge, so masks, picks and records are held bit for
bit without an exemption."""
import ctypes as C

import numpy as np
import pytest

from tests import rj_mt_move as rm
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
RTOL_L = tol.RTOL_L
RTOL_PROD = 1e-12           # include/hipensemble.h: log-likelihoods updated by +- a leaf against a full evaluation


def _engine(c, p, seed=None, **kw):
    from eryn_amd.rj import RJEngine
    eng = RJEngine(c["T"], c["W"], p["dbr"], p["t"], p["y"], p["sigma"], seed=c["seed"] if seed is None else seed, **kw)
    eng.set_mt_proposal(c["K"], p["dev_gens"])
    return eng


def _state(snap, o, prefix=""):
    names = [b.name for b in o.branches]
    return {k: snap[f"{prefix}x_{k}"] for k in names}, {k: snap[f"{prefix}inds_{k}"] for k in names}, snap[prefix + "L"], snap[prefix + "P"]


def _assert_records(eng, o, what, rtol=RTOL_L, L_ref=None):
    x1, inds1, L1, P1, betas1 = eng.download()
    for b in o.branches:
        assert np.array_equal(inds1[b.name], o.st.inds[b.name]), f"{what}: leaf masks of {b.name}"
        assert np.array_equal(x1[b.name], o.st.x[b.name]), f"{what}: coordinates of {b.name} (dead slots included)"
    assert np.array_equal(P1, o.st.P), f"{what}: log-prior"
    tol.check_logl(L1, o.st.L if L_ref is None else L_ref, rtol, what)
    return betas1


def _same_nonfinite(a, b, what):
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin) and np.array_equal(a[~fin], b[~fin], equal_nan=True), f"{what}: non-finite values differ"


@pytest.mark.parametrize("name", sorted(rm.CASES))
def test_teacher_forced_move_matches_the_specification(name):
    """hens_rj_mt_bd_step on the specification's inputs, proposal after proposal from the specification's state: accept masks, picks and
    records bit for bit, mt_ll within RTOL_L of the oracle's, mt_lp bit for bit, lsw / aux_lsw / factors within 1.0 B of exact arithmetic
    or the same non-finite value; the sweep without adaptation behind every proposal."""
    c = rm.CASES[name]
    p = rm.case_problem(c)
    eng = _engine(c, p)
    worst = [0.0, 0.0, 0.0]
    try:
        cnt = rm.forced_run(c, forced_proposal_hook(eng, name, worst))
        rm.assert_sized(cnt, c, name)
        assert eng.counters()["num_bd"] == c["nprop"]
    finally:
        eng.close()
    # (the ratios go into the tolerance report under this test's name - mt_move.assert_sums; profiles/rj_mt_bound_ratios.txt is made of it)
    print(f"{name}: worst |value - exact| / B: lsw {worst[0]:.3f}, aux_lsw {worst[1]:.3f}, factors {worst[2]:.3f}")


def forced_proposal_hook(eng, name, worst):
    """The ``on_proposal`` of tests/rj_mt_move.forced_run that holds the device to the specification on one proposal (the bars of
    test_teacher_forced_move_matches_the_specification; tests/test_hip_rj_limit_moves.py runs the limit records through it);
    ``worst``: the running maxima of |value - exact| / B for lsw, aux_lsw, factors."""
    seen = []

    def on_proposal(o, bi, inputs, info, ex, sweep, pre, mid):
        what = f"{name}: proposal {len(seen)} on branch {bi}"
        seen.append(bi)
        x, inds, L, P = _state(pre, o)
        eng.upload(x, inds, L, P, betas=o.st.betas)
        change, leaf, tries, u_pick, u_acc = inputs
        keep, out = eng.mt_bd_step(bi, change, leaf, tries, u_pick, u_acc, out=True)
        assert np.array_equal(keep, info["keep"]), f"{what}: accept mask"
        assert np.array_equal(out["pick"], info["pick"]), f"{what}: picks"
        assert np.array_equal(out["mt_lp"], info["mt_lp"]), f"{what}: mt_lp"
        tol.check_logl(out["mt_ll"], info["mt_ll"], RTOL_L, f"{what}: mt_ll")
        r = rm.mm.assert_sums(out["lsw"], out["aux_lsw"], out["factors"], ex, what)
        for i in range(3):
            worst[i] = max(worst[i], r[i])
        for k in ("lsw", "aux_lsw", "factors"):
            _same_nonfinite(out[k], info[k], f"{what}: {k}")
        xm, im, Lm, Pm = _state(mid, o)
        x1, inds1, L1, P1, _ = eng.download()
        for b in o.branches:
            assert np.array_equal(inds1[b.name], im[b.name]) and np.array_equal(x1[b.name], xm[b.name]), f"{what}: records of {b.name}"
        assert np.array_equal(P1, Pm), f"{what}: log-prior"
        tol.check_logl(L1, Lm, RTOL_L, f"{what}: log-like after the move")
        if o.T > 1:
            eng.upload(xm, im, Lm, Pm, betas=o.st.betas)
            eng.pt_sweep(sweep["iperm"], sweep["i1perm"], sweep["u_swap"], adapt=False)
            _assert_records(eng, o, f"{what}: after the sweep")

    return on_proposal


@pytest.mark.parametrize("name", rm.FIXTURES)
def test_teacher_forced_move_matches_the_reference(name):
    """hens_rj_mt_bd_step on every proposal the reference made in rjmt1 / rjmt2: the state in front of the proposal uploaded (the
    fixture's, behind the in-model move's sweep), the fixture's change / leaf / tries / u_pick / u_acc fed; the REFERENCE's accept mask,
    picks and mt_lp bit for bit, its mt_ll within RTOL_L, lsw / aux_lsw / factors within 1.0 B of exact arithmetic (the bounds from the
    specification on the same proposal, which reproduces the fixture bit for bit: tests/test_rj_mt_move.py) or the reference's own
    non-finite value - rjmt2's NaN factors among them -, and the records behind the move's update bit for bit."""
    from eryn_amd.rj import RJEngine, TemplateBranch
    fx = rm.load_fixture(name)
    names = rm.fixture_names(fx)
    kinds = {"gauss": "pulse", "sine": "sine"}
    T, W, K, n = int(fx["T"]), int(fx["W"]), int(fx["K"]), int(fx["nsteps"])
    dbr = [TemplateBranch(k, kinds[k], [tuple(r) for r in fx[f"{k}_box"]], int(fx["nl_max"][i]), int(fx["nl_min"][i])) for i, k in enumerate(names)]
    o = rm.fixture_oracle(fx)
    eng = RJEngine(T, W, dbr, fx["t"], fx["y"], float(fx["sigma"]))
    gens = rm.fixture_gens(fx)
    eng.set_mt_proposal(K, None if all(g is None for g in gens) else
                        {b.name: (g if g is not None else rm.branch_spec(b)) for b, g in zip(o.branches, gens)})
    worst, nans, picks, kp, ka = [0.0, 0.0, 0.0], 0, 0, 0, 0
    try:
        for it in range(n):
            o.mh_move()
            bi, _ = o.rj_move()
            info = o.mt_infos[-1]
            ex = rm.exact_rj_mt(o, info)
            k1, k2 = rm.knives(info, ex)
            kp, ka = kp + k1, ka + k2
            pre, mv = f"it{it}_mh_", f"it{it}_rj_"
            what = f"{name}: proposal {it} on branch {bi}"
            assert bi == int(fx[mv + "branch"])
            eng.upload({k: fx[pre + f"x_{k}"] for k in names}, {k: fx[pre + f"inds_{k}"] for k in names}, fx[pre + "L"], fx[pre + "P"], betas=fx[pre + "betas"])
            keep, out = eng.mt_bd_step(bi, fx[mv + "change"], fx[mv + "leaf"], fx[mv + "tries"], fx[mv + "u_pick"], fx[mv + "u_acc"], out=True)
            assert np.array_equal(keep, fx[mv + "keep"]), f"{what}: accept mask"
            assert np.array_equal(out["pick"], fx[mv + "pick"]), f"{what}: picks"
            assert np.array_equal(out["mt_lp"], fx[mv + "mt_lp"]), f"{what}: mt_lp"
            tol.check_logl(out["mt_ll"], fx[mv + "mt_ll"], RTOL_L, f"{what}: mt_ll")
            r = rm.mm.assert_sums(out["lsw"], out["aux_lsw"], out["factors"], ex, what)
            worst = [max(a, b) for a, b in zip(worst, r)]
            for k in ("lsw", "aux_lsw", "factors"):
                _same_nonfinite(out[k], fx[mv + k], f"{what}: {k}")
            x1, inds1, L1, P1, _ = eng.download()
            for k in names:
                assert np.array_equal(inds1[k], fx[mv + f"move_inds_{k}"]) and np.array_equal(x1[k], fx[mv + f"move_x_{k}"]), f"{what}: records of {k}"
            assert np.array_equal(P1, fx[mv + "move_P"]), f"{what}: log-prior"
            tol.check_logl(L1, fx[mv + "move_L"], RTOL_L, f"{what}: log-like after the move")
            nans += int(np.isnan(out["factors"]).sum())
            picks += int((out["pick"] != 0).sum())
        assert kp == 0 and ka == 0, f"{name}: {kp} picks / {ka} accept decisions of the reference's chain on a knife edge"
        assert picks > 0 and (nans > 0) == (name == "rjmt2")
    finally:
        eng.close()
    print(f"{name}: worst |value - exact| / B: lsw {worst[0]:.3f}, aux_lsw {worst[1]:.3f}, factors {worst[2]:.3f}")


# ---- hens_rj_step with the proposal set, replayed through the specification ---------------------------------------------------------------
def _replay_class():
    from tests.test_hip_leaf_kinds import _replay_class as wide_replay

    class ReplayMT(wide_replay(), rm.MTOracleRJSampler):
        """The replay oracle of tests/test_hip_leaf_kinds.py (draw sources: hens_rj_debug_draws / _stretch) with the multiple-try move in
        the reversible-jump slot, its tries and pick uniforms read from what hens_rj_mt_debug_draws exports."""

        def _draw_tries(self, b, gen):
            tr = self.mt["tries"][self._k()]
            assert tr.shape == (self.T, self.W, self.K, max(q.ndim for q in self.branches)) and not tr[..., b.ndim:].any()
            return tr[..., :b.ndim]

        def _draw_pick(self):
            u = self.mt["u_pick"][self._k()]
            assert np.all((u >= 0) & (u < 1))
            return u

    return ReplayMT


def _production_engine(c, p, schedule, in_model, it0=0, seed=None, K=None, adapt=None, mt=True):
    from eryn_amd.rj import RJEngine
    ncoord = sum(b.nleaves_max * b.ndim for b in p["obr"])
    eng = RJEngine(c["T"], c["W"], p["dbr"], p["t"], p["y"], p["sigma"], seed=c["seed"] if seed is None else seed, a=1.5,
                   live_dangerously=c["W"] < 2 * ncoord, **(adapt or {}))
    if mt:
        eng.set_mt_proposal(c["K"] if K is None else K, p["dev_gens"])
    eng.upload(p["x"], p["inds"], betas=p["betas"])
    eng.eval_state()
    if in_model == "stretch":
        eng.set_in_model("stretch")
    else:
        eng.set_mh_scale(p["scale"])
    eng.set_schedule(schedule)
    if it0:
        eng.set_iteration(it0)
        eng.set_adapt_time(it0)
    return eng


def _check_draws(dd, mtd, seed, it, c, p, what):
    """What hens_rj_mt_debug_draws (and, for the accept uniform, hens_rj_debug_draws) exports for iteration ``it`` against the
    specification's statement of the draws (tests/rj_mt_move.py: mt_draws, pick_uniforms, accept_uniforms - the keys' bit fields, try 0 =
    the plain move's birth call): a uniform parameter bit for bit, a log-uniform or normal one within its bound E of the exact value,
    the pick and accept uniforms exactly."""
    T, W, K = c["T"], c["W"], c["K"]
    branches = [dd["branch"]] if dd["branch"] >= 0 else list(range(len(p["obr"])))
    assert mtd["tries"].shape[0] == len(branches) == mtd["u_pick"].shape[0]
    for k, bi in enumerate(branches):
        b = p["obr"][bi]
        gen = p["gens"][bi] if p["gens"][bi] is not None else rm.branch_spec(b)
        X, Xs, E = rm.mt_draws(seed, it, T, W, K, bi, gen)
        q = mtd["tries"][k]
        assert q.shape == (T, W, K, max(x.ndim for x in p["obr"])) and not q[..., b.ndim:].any(), f"{what}: shape of branch {bi}'s tries"
        q = q[..., :b.ndim]
        uni = gen["kind"] == rm.pt.UNIFORM
        assert np.array_equal(q[..., uni], X[..., uni]), f"{what}: a uniform draw of branch {bi} differs from the specification"
        err = np.abs(q.astype(rm.LD) - Xs).astype(np.float64)
        assert (err <= E)[..., ~uni].all(), f"{what}: a draw of branch {bi} misses its bound E"
        if p["gens"][bi] is None:              # generator = prior: try 0 is the leaf the plain move would give birth to
            assert np.array_equal(q[:, :, 0], dd["birth"][k][..., :b.ndim]), f"{what}: try 0 is the plain move's birth draw"
        assert np.array_equal(mtd["u_pick"][k], rm.pick_uniforms(seed, it, T, W, bi)), f"{what}: pick uniforms of branch {bi}"
        assert np.array_equal(dd["u_bd"][k], rm.accept_uniforms(seed, it, T, W, bi)), f"{what}: accept uniforms of branch {bi}"


@pytest.mark.parametrize("name", sorted(rm.REPLAYS))
def test_production_step_replayed_through_the_specification(name):
    """hens_rj_step with a multiple-try proposal - k_rj_mt on the resident templates, folded ladder adaptation included - against the
    specification fed with the draws hens_rj_debug_draws + hens_rj_mt_debug_draws export: records, masks, log-priors and accept counters
    bit for bit, log-likelihoods to the by-difference bar 1e-12, the ladder to 1e-13; one case crosses iteration 63 -> 64 (the refresh)
    with an adaptation of a short lag pending into every birth / death launch."""
    cname, schedule, in_model, iters, it0, adapting = rm.REPLAYS[name]
    c = rm.CASES[cname]
    replay_through_the_specification(name, c, rm.case_problem(c), schedule, in_model, iters, it0, adapting)


def replay_through_the_specification(name, c, p, schedule, in_model, iters, it0=0, adapting=False, on_info=None):
    """The body of test_production_step_replayed_through_the_specification on any case and problem (tests/test_hip_rj_limit_moves.py
    runs the limit records through it); on_info(o, info): called with every proposal's record of the specification."""
    adapt = dict(adaptation_lag=5, adaptation_time=5) if adapting else {}
    eng = _production_engine(c, p, schedule, in_model, it0, adapt=adapt)
    try:
        x0, inds0, L0, P0, _ = eng.download()
        o = _replay_class()(p["obr"], x0, inds0, p["t"], p["y"], p["sigma"], None, None, p["betas"], schedule=schedule, in_model=in_model,
                            record=True, like_fn=p["like_fn"], a=1.5, num_try=c["K"], gens=p["gens"], **adapt)
        o.live, o.time = True, it0
        assert np.array_equal(o.st.P, P0) and np.isfinite(P0).all()
        tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        mh_acc, bd_acc, done = np.zeros((c["T"], c["W"])), np.zeros((c["T"], c["W"])), 0
        for n in (2, iters - 2):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                dd = eng.debug_draws(i)
                o.load(dd, offsets, eng.debug_draws_stretch(i) if in_model == "stretch" else None)
                o.mt = eng.mt_debug_draws(i)
                _check_draws(dd, o.mt, c["seed"], i, c, p, f"{name}: iteration {i}")
                acc, bi, racc = o.iteration()
                o.trace.pop()
                mh_acc += acc
                bd_acc += racc
            done += n
            what = f"{name}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_records(eng, o, what, rtol=RTOL_PROD)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc) and np.array_equal(cn["accepted_bd"], bd_acc), f"{what}: accept counters"
            assert cn["num_mh"] == done and cn["num_bd"] == done
        cnt = rm.Counts()
        for info in o.mt_infos:
            cnt.add(o, info, rm.exact_rj_mt(o, info))
            if on_info is not None:
                on_info(o, info)
        rm.assert_sized(cnt, dict(c, inf_prior=False, nan_factor=False, edges=False), name)
        assert o.knife_swaps == 0
        if adapting:
            assert not np.array_equal(o.st.betas, p["betas"]), "the ladder must have moved"
    finally:
        eng.close()


def test_one_try_from_the_prior_is_the_plain_moves_chain():
    """K = 1 with generator = prior: try 0 of a birth is the plain move's birth draw, a death's try 0 the dying leaf - the chain of a twin
    context stepped without the proposal: same records, masks and accept counters over 8 iterations."""
    c = rm.CASES["w9_k2_nd64_two_gen"]
    p = dict(rm.case_problem(c), dev_gens=None)
    a = _production_engine(c, p, "separate_branches", "gaussian", K=1)
    b = _production_engine(c, p, "separate_branches", "gaussian", mt=False)
    try:
        for n in (3, 5):
            a.step(n)
            b.step(n)
            xa, ia, La, Pa, ba = a.download()
            xb, ib, Lb, Pb, bb = b.download()
            for k in xa:
                assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"records of {k}"
            assert np.array_equal(Pa, Pb) and np.array_equal(ba, bb)
            tol.check_logl(La, Lb, RTOL_PROD, "log-likelihoods of the twin chains")
            ca, cb = a.counters(), b.counters()
            assert np.array_equal(ca["accepted_bd"], cb["accepted_bd"]) and np.array_equal(ca["accepted_mh"], cb["accepted_mh"])
        assert ca["accepted_bd"].sum() > 0
    finally:
        a.close()
        b.close()


def test_chain_resumed_in_a_new_context_continues_bit_for_bit():
    """Download, new context, hens_set_iteration: the chain under the multiple-try move is a function of (State, seed, iteration counter,
    adaptation time)."""
    c = rm.CASES["w9_k7_nd50_terms_gen"]
    p = rm.case_problem(c)
    a = _production_engine(c, p, "iterate_branches", "gaussian", it0=60)
    snaps = []
    try:
        for n in (3, 4):
            a.step(n)
            snaps.append((a.download(), a.iteration(), a.counters()["adapt_time"]))
    finally:
        a.close()
    (x1, i1, L1, P1, b1), it1, at1 = snaps[0]
    b = _production_engine(c, dict(p, x=x1, inds=i1, betas=b1), "iterate_branches", "gaussian")
    try:
        b.upload(x1, i1, L1, P1, b1)
        b.set_iteration(it1)
        b.set_adapt_time(at1)
        b.step(4)
        xb, ib, Lb, Pb, bb = b.download()
        (xa, ia, La, Pa, ba), ita, _ = snaps[1]
        assert b.iteration() == ita
        for k in xa:
            assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"records of {k}"
        assert np.array_equal(La, Lb) and np.array_equal(Pa, Pb) and np.array_equal(ba, bb)
    finally:
        b.close()


# ---- the sampler ----------------------------------------------------------------------------------------------------------------------------
def _sampler(c, p, rng, backend=None, seed=5):
    from eryn_amd.rj import GaussianLeafMove, MTDistGenMoveRJ, RJEnsembleSampler, TemplateLikelihood
    names = [b.name for b in p["dbr"]]
    kinds = dict(zip(names, c["kinds"]))
    gens = p["dev_gens"] or {b.name: rm.branch_spec(b) for b in p["obr"]}
    moves = [MTDistGenMoveRJ({k: gens[k]}, num_try=c["K"], rj=True, gibbs_sampling_setup=k) for k in names]
    return RJEnsembleSampler(c["W"], {b.name: b.ndim for b in p["dbr"]}, TemplateLikelihood(kinds, p["t"], p["y"], p["sigma"]),
                             {b.name: (b.prior if b.prior is not None else list(zip(b.lo, b.hi))) for b in p["dbr"]},
                             tempering_kwargs=dict(ntemps=c["T"]), branch_names=names, nleaves_max=dict(zip(names, c["nl_max"])),
                             nleaves_min=dict(zip(names, c["nl_min"])), moves=GaussianLeafMove({k: np.diag(s ** 2) for k, s in zip(names, p["scale"])}),
                             rj_moves=moves if len(moves) > 1 else moves[0], rng=rng, seed=seed, backend=backend)


@pytest.mark.parametrize("name", rm.FIXTURES)
def test_numpy_sampler_lands_on_the_reference_chain(name):
    """RJEnsembleSampler(rj_moves=MTDistGenMoveRJ ..., rng="numpy") with the reference's seeds: the host draws in the reference's order
    (rj move's choice, coins and leaf choices from R; the tries and the pick uniforms from the global stream; R.rand) and
    hens_rj_mt_bd_step lands on the reference's chain - every stored step's masks, coordinates and log-priors exact, log-likelihoods to
    1e-12 (the bar tests/test_hip_rj.py holds the plain move's reference chains to), the ladder to 1e-13, the per-move accept counters exact."""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, MTDistGenMoveRJ, RJEnsembleSampler, TemplateLikelihood
    from eryn_amd.state import State
    fx = rm.load_fixture(name)
    names = rm.fixture_names(fx)
    n, K = int(fx["nsteps"]), int(fx["K"])
    kinds = {"gauss": "pulse", "sine": "sine"}
    priors = {k: {i: uniform_dist(*fx[f"{k}_box"][i]) for i in range(3)} for k in names}
    gens = {k: {i: uniform_dist(*fx[f"{k}_gen_box"][i]) for i in range(3)} for k in names}
    cov = {k: np.diag(np.ones(3)) * float(fx["cov_factor"]) for k in names}
    nlmax, nlmin = dict(zip(names, map(int, fx["nl_max"]))), dict(zip(names, map(int, fx["nl_min"])))
    if len(names) == 1:
        rj_moves = MTDistGenMoveRJ(gens, nleaves_max=nlmax, nleaves_min=nlmin, num_try=K, rj=True)
    else:
        rj_moves = [MTDistGenMoveRJ({k: gens[k]}, nleaves_max=nlmax, nleaves_min=nlmin, num_try=K, rj=True, gibbs_sampling_setup=k) for k in names]
    np.random.seed(int(fx["seed_construct"]))          # R := snapshot of the global stream at construction
    s = RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, TemplateLikelihood({k: kinds[k] for k in names}, fx["t"], fx["y"], float(fx["sigma"])),
                          priors, tempering_kwargs=dict(ntemps=int(fx["T"])), nbranches=len(names), branch_names=names, nleaves_max=nlmax,
                          nleaves_min=nlmin, moves=GaussianLeafMove(cov), rj_moves=rj_moves)
    try:
        assert np.array_equal(s.temperature_control.betas, fx["betas0"])
        coords = {k: fx[f"x0_{k}"] for k in names}
        inds = {k: fx[f"inds0_{k}"] for k in names}
        np.random.seed(int(fx["seed_run"]))
        last = s.run_mcmc(State(coords, log_like=fx["L0"], log_prior=fx["P0"], inds=inds), n, store=True)
        assert len(s.chain) == n
        for it, st in enumerate(s.chain):
            pre = f"it{it}_rj_"
            for k in names:
                assert np.array_equal(st.branches[k].inds, fx[pre + f"inds_{k}"]), f"{pre}inds of {k}"
                m = st.branches[k].inds
                assert np.array_equal(st.branches[k].coords[m], fx[pre + f"x_{k}"][m]) and np.isnan(st.branches[k].coords[~m]).all(), f"{pre}x of {k}"
            assert np.array_equal(st.log_prior, fx[pre + "P"]), pre
            tol.check_logl(st.log_like, fx[pre + "L"], 1e-12, f"{name}: {pre}log-like")
        pre = f"it{n - 1}_rj_"
        for k in names:
            assert np.array_equal(last.branches[k].coords, fx[pre + f"x_{k}"]), f"coordinates of {k} (dead slots included)"
        np.testing.assert_allclose(last.betas, fx[pre + "betas"], rtol=1e-13, atol=0)
        assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"])
        assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"])
        assert np.array_equal(np.array(s.rj_num_proposals), fx["rj_num_proposals"])
        for i, k in enumerate(names):
            assert np.array_equal(s.mt_moves[k].accepted, fx["rj_accepted_total"][i]) and s.mt_moves[k].num_proposals == int(fx["rj_num_proposals"][i])
    finally:
        s.engine.close()


def test_device_backend_chain_equals_the_list_of_states():
    """RJEnsembleSampler(rj_moves=[MTDistGenMoveRJ per branch], rng="philox"): six stored steps kept on the device (RJDeviceBackend,
    hens_rj_step_chain) are the list-of-States chain bit for bit."""
    from eryn_amd.backend import RJDeviceBackend
    from eryn_amd.state import State
    c = rm.CASES["w9_k2_nd64_two_gen"]
    p = rm.case_problem(c)
    start = State(p["x"], inds=p["inds"], betas=p["betas"])
    s1 = _sampler(c, p, "philox")
    s2 = _sampler(c, p, "philox", backend=RJDeviceBackend())
    try:
        s1.run_mcmc(start, 6, thin_by=2)
        s2.run_mcmc(start, 6, thin_by=2)
        from tests.test_hip_rj_chain_store import assert_chain_is_the_host_chain
        assert len(s1.chain) == 6 and s2.chain == []
        assert_chain_is_the_host_chain(s2.backend, s1.chain, c["T"], "multiple-try birth / death")
        assert np.array_equal(s1.rj_accepted_all, s2.rj_accepted_all)
        assert s1.rj_accepted_all.sum() > 0 and s1.rj_num_proposals_all == 12
    finally:
        s1.engine.close()
        s2.engine.close()


def test_sampler_refuses_what_the_move_cannot_do():
    from eryn_amd.rj import MTDistGenMoveRJ
    c = rm.CASES["w9_k2_nd64_two_gen"]
    p = rm.case_problem(c)
    gens = {b.name: rm.branch_spec(b) for b in p["obr"]}
    with pytest.raises(NotImplementedError, match="one MTDistGenMoveRJ per branch"):
        _sampler_with(c, p, MTDistGenMoveRJ({"pulse": gens["pulse"]}, num_try=3))
    with pytest.raises(NotImplementedError, match="same num_try"):
        _sampler_with(c, p, [MTDistGenMoveRJ({k: gens[k]}, num_try=3 + i, gibbs_sampling_setup=k) for i, k in enumerate(gens)])
    with pytest.raises(NotImplementedError, match="TemplateLikelihood"):
        _sampler_with(c, p, [MTDistGenMoveRJ({k: gens[k]}, num_try=3, gibbs_sampling_setup=k) for k in gens], like=lambda x: 0.0)


def _sampler_with(c, p, rj_moves, like=None):
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, TemplateLikelihood
    names = [b.name for b in p["dbr"]]
    like = like or TemplateLikelihood(dict(zip(names, c["kinds"])), p["t"], p["y"], p["sigma"])
    s = RJEnsembleSampler(c["W"], {b.name: b.ndim for b in p["dbr"]}, like, {b.name: list(zip(b.lo, b.hi)) for b in p["dbr"]},
                          tempering_kwargs=dict(ntemps=c["T"]), branch_names=names, nleaves_max=dict(zip(names, c["nl_max"])),
                          nleaves_min=dict(zip(names, c["nl_min"])), moves=GaussianLeafMove({k: np.diag(s ** 2) for k, s in zip(names, p["scale"])}),
                          rj_moves=rj_moves)
    s.engine.close()
    return s


# ---- refusals: code and text, nothing changed ---------------------------------------------------------------------------------------------
def test_refusals_keep_code_and_text_and_change_nothing():
    from eryn_amd import _lib
    from eryn_amd._lib import ptr
    from eryn_amd.rj import LeafBranch, RJEngine
    c = rm.CASES["w9_k2_nd64_two_gen"]
    p = rm.case_problem(c)
    eng = _production_engine(c, p, "separate_branches", "gaussian")
    lib, ctx = eng.lib, eng.ctx

    def refused(code, text, call):
        before = eng.download(), eng.iteration(), eng.counters()["num_bd"]
        assert call() == code
        assert lib.hens_last_error(ctx).decode() == text
        after = eng.download(), eng.iteration(), eng.counters()["num_bd"]
        for u, v in zip(before[0][:2], after[0][:2]):
            assert all(np.array_equal(u[k], v[k]) for k in u)
        assert all(np.array_equal(u, v) for u, v in zip(before[0][2:], after[0][2:])) and before[1:] == after[1:]

    try:
        refused(_lib.ERR_INVALID, "num_try must be in [0, 64] (one lane per try; 0: the plain birth / death move)",
                lambda: lib.hens_rj_set_mt_proposal(ctx, 65, None, None, None, None, None, None))
        with pytest.raises(ValueError, match="num_try must be in"):       # ... and through the engine: its own record follows the context
            eng.set_mt_proposal(65, p["dev_gens"])
        assert eng.mt_K == 2 and eng.mt_gen is not None
        assert eng.mt_debug_draws(0)["tries"].shape[3] == 2
        eng.step(1)                                            # (still the proposal of two tries)
        # a proposal of more tries behind one of fewer: the teacher-forced call's staging has room (and a second call reuses it)
        eng.set_mt_proposal(64, p["dev_gens"])
        rs = np.random.RandomState(3)
        for _ in range(2):
            _, inds, _, _, _ = eng.download()
            full = inds[p["obr"][0].name].all(axis=-1)
            change, leaf = np.where(full, -1, 1), np.where(full, 0, (~inds[p["obr"][0].name]).argmax(axis=-1))
            keep = eng.mt_bd_step(0, change, leaf, np.tile(np.array([3.0, 0.0, 0.1]), (c["T"], c["W"], 64, 1)), rs.rand(c["T"], c["W"]), np.ones((c["T"], c["W"])))
            assert keep.shape == (c["T"], c["W"])
        eng.set_mt_proposal(2, p["dev_gens"])
        eng.set_schedule("together")
        refused(_lib.ERR_UNSUPPORTED, 'Can only propose change to one model at a time with MT. (rj schedule "together" under hens_rj_set_mt_proposal)',
                lambda: lib.hens_rj_step(ctx, 1))
        eng.set_schedule("separate_branches")
        d = _lib.HensRjDraws()
        buf = np.zeros((c["T"], c["W"], eng.RW))
        refused(_lib.ERR_UNSUPPORTED, "hens_rj_propose: not under a multiple-try proposal (hens_rj_set_mt_proposal: the tries' likelihoods are the device's)",
                lambda: lib.hens_rj_propose(ctx, _lib.RJ_MOVE_BD, C.byref(d), ptr(buf), ptr(buf), ptr(buf)))
        bad = rm.pt.make_spec([("uniform", 0.0, 1.0)] * 3)
        arrs = [np.concatenate([bad[k], bad[k]]) for k in ("kind", "lo", "hi", "c0", "c1", "c2")]
        arrs[2][4] = arrs[1][4]                                # (sine, parameter 1: lo == hi)
        refused(_lib.ERR_INVALID, "prior terms need lo < hi in every dimension (generator: branch 1, parameter 1)",
                lambda: lib.hens_rj_set_mt_proposal(ctx, 3, ptr(arrs[0].astype(np.int32)), *map(ptr, arrs[1:])))
        eng.step(1)
    finally:
        eng.close()
    fixed = dict(c, nl_min=(3, 0))
    pf = rm.case_problem(fixed)
    e2 = RJEngine(c["T"], c["W"], pf["dbr"], pf["t"], pf["y"], pf["sigma"])
    try:
        with pytest.raises(ValueError, match=r"MT RJ proposal requires that nleaves_min != nleaves_max. \(branch 0\)"):
            e2.set_mt_proposal(3)
    finally:
        e2.close()
    e3 = RJEngine(c["T"], c["W"], [LeafBranch("a", [(0.0, 1.0)] * 2, 3, 0)], None, None, 1.0)
    try:
        with pytest.raises(RuntimeError, match="has no device likelihood"):
            e3.set_mt_proposal(3)
    finally:
        e3.close()
