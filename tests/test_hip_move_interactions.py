"""The generator moves and the Gibbs tables held to the composed specification on every path of hens_step (-m gpu).

tests/test_hip_dist_move.py, tests/test_hip_mt_move.py and tests/test_hip_gibbs.py replay ``make_ladder(D, ntemps=T)`` with T <= 4 at the
default adaptation constants, two sets, no period.  Here the move in the MH slot - DistributionGenerate (k_dist), MTDistGenMove
(k_mt_dist), the Gaussian move under Gibbs tables - meets what a context can be set to (``move_interactions.CASES``, sized on the CPU
by tests/test_move_interactions.py):

  A. ladders and tiles: short tiles (T does not divide 128), the multi-word swap bitmask at 64 rungs, the copying path of 65 and 130
     rungs, a beta = 0 rung, a hand-made ladder, ``adaptive=False``, ``stop_adaptation``, all at lag 50 / time 10 - the ladder moves
     in its leading digits in front of the move's launch (flush_adapt);
  B. periodic parameters: the move's proposals land outside [0, period) and stay there, the stretch iterations round them wrap;
  C. three sets: the in-place move between rotating sets;
  D. a ladder shard, teacher-forced: draws, betas and state rows of rungs 1:3;
  E. Gibbs tables on the same ladders.

Every replay is tests/composed_replay.replay at the project's bars; every run asserts ``move_interactions.check_coverage`` on the
specification's side and on the device's ladder, and its launch path from a profiled two-iteration call afterwards.
"""
import numpy as np
import pytest

from tests import composed_replay as cr
from tests import dist_move as dm
from tests import gibbs_move as gm
from tests import move_interactions as mi
from tests import mt_move as mt
from tests import parity_utils as pu
from tests import production_draws as pd
from tests import replay_utils as ru
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu


def _engine(prob, T, W, seed, **kw):
    from eryn_amd.engine import HipEnsemble
    return HipEnsemble(T, W, prob.D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=seed, prior_terms=None if cr.is_box(prob) else prob.prior,
                       live_dangerously=True, **kw)


def _set_slot(eng, slot):
    if slot[0] == "dist":
        eng.set_dist_proposal(slot[1], slot[2])
    elif slot[0] == "mt":
        eng.set_mt_dist_proposal(slot[1], slot[2], slot[3])
    else:
        eng.set_mh_proposal(slot[1], slot[2], slot[3])


@pytest.mark.parametrize("name,run", mi.RUNS, ids=mi.RUN_IDS)
def test_replay(name, run):
    c = mi.CASES[name]
    T, W, seed = c["T"], c["W"], c["seed"]
    what = mi.run_id(name, run)
    prob = mi.case_problem(c, run[1])
    slot = mi.slot_of(c, run, prob)
    betas0, x0 = mi.case_inputs(c, prob)
    eng = _engine(prob, T, W, seed, adaptive=c["adaptive"], stop_adaptation=c["stop_adaptation"], adaptation_lag=mi.LAG, adaptation_time=mi.NU)
    eng.upload(x0, betas=betas0)
    eng.eval_state()
    x, L, P, betas = eng.download()
    assert np.isfinite(P).all() and np.array_equal(betas, betas0)
    _set_slot(eng, slot)
    if prob.period is not None:
        eng.set_periodic(prob.period)
    if c["nsplits"] != 2:
        eng.set_nsplits(c["nsplits"])
    gibbs = None if c["gibbs"] is None else dict(stretch=c["gibbs"], mh=c["gibbs"])
    cov = mi.Coverage(T)
    if gibbs is not None:
        eng.set_gibbs("stretch", gibbs["stretch"])
        eng.set_gibbs("mh", gibbs["mh"])
        cov.books = gm.BlockBooks(T, W, len(gibbs["stretch"]), len(gibbs["mh"]))
    st = ru.OracleState(x, L, P, betas)
    kinds = cr.replay(eng, st, prob, slot, c["calls"], seed=seed, period=prob.period, nsplits=c["nsplits"], lag=mi.LAG, nu=mi.NU,
                      adaptive=c["adaptive"], stop_adaptation=c["stop_adaptation"], gibbs=gibbs, counts=cov, what=what)
    assert kinds == [pd.is_mh(seed, it, c["weight"]) for it in range(sum(c["calls"]))]
    betas_dev = eng.download()[3]
    for b in (st.betas, betas_dev):                             # the specification says so, and the device must too
        mi.check_coverage(c, run, cov, betas0, b, st.swaps_total, what=what)
    if "beta0" not in c["exempt"] and run[1] == "box" and run[0] != "gauss":     # ... every walker of the beta = 0 rung, every proposal: no tolerance
        assert np.array_equal(eng.mh_counters()["accepted"][-1], np.full(W, float(cov.slot_iters))), f"{what}: the beta = 0 rung on the device"
    if c["stop_adaptation"] >= 0:
        assert eng.counters()["adapt_time"] == st.time == sum(c["calls"]), f"{what}: the adaptation's time runs on behind stop_adaptation"
    # the launch path of a profiled call of two iterations
    eng.set_profiling(True)
    it0 = eng.iteration()
    eng.step(2)
    tm = eng.timing()
    eng.set_profiling(False)
    nm = sum(pd.is_mh(seed, it, c["weight"]) for it in (it0, it0 + 1))
    got = (tm["n_stretch"], tm["n_pt"], tm["n_fused"])
    assert got == cr.launch_counts(c["path"], nm, c["nsplits"], gibbs), f"{what}: listed under {c['path']!r}, a profiled call with {nm} slot iterations of 2 reports {got}"
    own = tol.report().get(tol._test_name(), {"max_rel_L": 0.0, "values": 0})
    print("%s: max_rel_L %.3e values %d" % (what, own["max_rel_L"], own["values"]))
    eng.close()


# ---- D. a ladder shard, teacher-forced -----------------------------------------------------------------------------------------------------------
def _whole_and_shard(D):
    prob = mi.shard_problem(D)
    T, W, (r0, r1) = mi.SHARD_T, mi.SHARD_W, mi.SHARD_RANGE
    whole = _engine(prob, T, W, mi.SEED)
    shard = _engine(prob, T, W, mi.SEED, rung_range=(r0, r1))
    whole.upload(prob.x0(T, W), betas=mi.ld.ladder("geometric", T, D))
    whole.eval_state()
    x, L, P, betas = whole.download()
    assert np.isfinite(P).all() and len(set(np.diff(betas))) == T - 1, "an unequal ladder"
    shard.upload(x[r0:r1], L[r0:r1], P[r0:r1], betas)
    return prob, whole, shard, (x, L, P, betas)


@pytest.mark.parametrize("D", sorted(mi.SHARD_D))
def test_a_shard_draws_the_rows_of_the_whole_ladder(D):
    """hens_debug_draws(mh) and hens_mt_debug_draws of a context with rung_range = (1, 3): rows 1:3 of the whole context's, and the
    specification's with rung_begin = 1 - uniform terms bit for bit, the others within E."""
    prob, whole, shard, _ = _whole_and_shard(D)
    T, W, (r0, r1), K = mi.SHARD_T, mi.SHARD_W, mi.SHARD_RANGE, mi.SHARD_K
    for eng in (whole, shard):
        eng.set_dist_proposal(prob.gen, 1.0)
    for it in (0, 3, 2 ** 32 + 1):
        dw, ds = whole.debug_draws(it, mh=True), shard.debug_draws(it, mh=True)
        assert ds["is_mh"] and ds["mh_step"].shape == (r1 - r0, W, D)
        for k in ("mh_step", "mh_u"):
            assert np.array_equal(ds[k], dw[k][r0:r1]), f"D = {D}, iteration {it}: {k} of the shard is not rows {r0}:{r1} of the whole ladder's"
        assert not np.array_equal(ds["mh_step"], dw["mh_step"][:r1 - r0])
        cr.check_dist_draws(ds, mi.SEED, it, r1 - r0, W, prob.gen, f"D = {D}, iteration {it}, shard", rung_begin=r0)
    for eng in (whole, shard):
        eng.set_mt_dist_proposal(prob.gen, K, 1.0)
    for it in (0, 3, 2 ** 32 + 1):
        tw, ts = whole.mt_debug_draws(it), shard.mt_debug_draws(it)
        assert ts[0].shape == (r1 - r0, W, K, D)
        for a, b, k in zip(ts, tw, ("tries", "pick uniforms", "accept uniforms")):
            assert np.array_equal(a, b[r0:r1]), f"D = {D}, iteration {it}: the {k} of the shard are not rows {r0}:{r1} of the whole ladder's"
        assert not np.array_equal(ts[1], tw[1][:r1 - r0])
        cr.check_mt_draws(ts, shard.debug_draws(it, mh=True), mi.SEED, it, r1 - r0, W, K, prob.gen, f"D = {D}, iteration {it}, shard", rung_begin=r0)
    whole.close()
    shard.close()


def _outliers(q, prob, n, rs):
    """a caller's points may lie anywhere (tests/test_hip_dist_move.py): in every seventh walker one coordinate outside the generator"""
    Tl, W, D = q.shape[0], q.shape[1], q.shape[-1]
    for t in range(Tl):
        for w in range(n, W, 7):
            d = int(rs.randint(D))
            lo, hi = prob.gen["lo"][d], prob.gen["hi"][d]
            q[(t, w, d) if q.ndim == 3 else (t, w, int(rs.randint(q.shape[2])), d)] = \
                hi + 0.25 * (hi - lo) if np.isfinite(hi) else prob.centre[d] + 50.0 * prob.half[d]
    return q


@pytest.mark.parametrize("D", sorted(mi.SHARD_D))
def test_dist_step_on_a_shard_reads_its_own_rungs_betas(D):
    prob, whole, shard, (x, L, P, betas) = _whole_and_shard(D)
    whole.close()
    W, (r0, r1) = mi.SHARD_W, mi.SHARD_RANGE
    Tl = r1 - r0
    shard.set_dist_proposal(prob.gen, 0.5)
    xs, Ls, Ps = x[r0:r1].copy(), L[r0:r1].copy(), P[r0:r1].copy()
    rs = np.random.RandomState(41)
    accepted = differs = 0
    for n in range(mi.SHARD_PROPOSALS):
        what = f"D = {D}, shard proposal {n}"
        q = _outliers(dm.dist_draws(mi.SEED, n, Tl, W, prob.gen, rung_begin=r0)[0], prob, n, rs)
        u = rs.rand(Tl, W)
        wrong = dm.dist_step(xs.copy(), Ls.copy(), Ps.copy(), betas[:Tl], q, u, prob.prior, prob.gen, prob.loglike)[3]
        x_old, info = xs.copy(), {}
        _, _, _, keep_s, _ = dm.dist_step(xs, Ls, Ps, betas[r0:r1], q, u, prob.prior, prob.gen, prob.loglike, info=info)
        with np.errstate(divide="ignore"):
            assert not pu.knife_edge(info["lnpdiff"], np.log(u)).any(), f"{what}: a decision on the knife edge: pick another seed"
        differs += int((wrong != keep_s).sum())
        keep, fac = shard.dist_step(q, u, want_factors=True)
        assert np.array_equal(keep, keep_s), f"{what}: accept mask differs in {int((keep != keep_s).sum())} walkers"
        dm.assert_factors(fac, prob.gen, x_old, q, what)
        xd, Ld, Pd, bd = shard.download()
        assert xd.shape == (Tl, W, D) and np.array_equal(xd, xs), f"{what}: positions differ"
        cr.check_P(Pd, Ps, prob, xd, what)
        tol.check_logl(Ld, Ls, tol.RTOL_L, what)
        assert np.array_equal(bd, betas)
        accepted += int(keep.sum())
        xs, Ls, Ps = xd, Ld, Pd
    assert accepted > 0 and differs > 0, "the specification with betas[0:2] in place of betas[1:3] must keep other walkers"
    assert np.array_equal(shard.mh_counters()["accepted"].sum(), accepted)
    shard.close()


@pytest.mark.parametrize("D", sorted(mi.SHARD_D))
def test_mt_dist_step_on_a_shard_reads_its_own_rungs_betas(D):
    prob, whole, shard, (x, L, P, betas) = _whole_and_shard(D)
    whole.close()
    W, (r0, r1), K = mi.SHARD_W, mi.SHARD_RANGE, mi.SHARD_K
    Tl = r1 - r0
    shard.set_mt_dist_proposal(prob.gen, K, 0.5)
    xs, Ls, Ps = x[r0:r1].copy(), L[r0:r1].copy(), P[r0:r1].copy()
    rs = np.random.RandomState(43)
    accepted = picks = differs = 0
    for n in range(mi.SHARD_PROPOSALS):
        what = f"D = {D}, shard proposal {n}"
        q = _outliers(mt.mt_draws(mi.SEED, n, Tl, W, K, prob.gen, rung_begin=r0)[0], prob, n, rs)
        up, ua = rs.rand(Tl, W), rs.rand(Tl, W)
        wrong = mt.mt_step(xs.copy(), Ls.copy(), Ps.copy(), betas[:Tl], q, up, ua, prob.prior, prob.gen, prob.loglike)
        info = {}
        keep_s, pick_s, _, _, _ = mt.mt_step(xs, Ls, Ps, betas[r0:r1], q, up, ua, prob.prior, prob.gen, prob.loglike, info=info)
        ex = mt.exact_mt(info, pick_s, betas[r0:r1], prob.prior, prob.gen)
        cr.no_knife(info, ex, what)
        differs += int((wrong[0] != keep_s).sum()) + int((wrong[1] != pick_s).sum())
        out = shard.mt_dist_step(q, up, ua, want=("pick", "lsw", "aux_lsw", "factors"))
        assert np.array_equal(out["pick"], pick_s), f"{what}: picks differ in {int((out['pick'] != pick_s).sum())} walkers"
        assert np.array_equal(out["keep"], keep_s), f"{what}: accept mask differs in {int((out['keep'] != keep_s).sum())} walkers"
        mt.assert_sums(out["lsw"], out["aux_lsw"], out["factors"], ex, what)
        xd, Ld, Pd, _ = shard.download()
        assert np.array_equal(xd, xs), f"{what}: positions differ"
        cr.check_P(Pd, Ps, prob, xd, what)
        tol.check_logl(Ld, Ls, tol.RTOL_L, what)
        accepted += int(keep_s.sum())
        picks += int((pick_s != 0).sum())
        xs, Ls, Ps = xd, Ld, Pd
    assert accepted > 0 and picks > 0 and differs > 0, "the specification with betas[0:2] in place of betas[1:3] must keep or pick other walkers"
    shard.close()


# ---- two chains from the reference: both moves of the mix hold the same PeriodicContainer -------------------------------------------------------
def _periodic_moves(kind, fx, rng):
    """(stretch, move, PeriodicContainer) as a user moves them over from the reference script of the fixture."""
    from eryn_amd.moves import DistributionGenerate, MTDistGenMove, StretchMove
    from eryn_amd.periodic import PeriodicContainer
    _, gen = dm.fixture_containers(fx)
    pc = PeriodicContainer({"model_0": {int(d): float(fx["period"][d]) for d in np.flatnonzero(fx["period"])}})
    kw = dict(periodic=pc, rng=rng)
    move = DistributionGenerate({"model_0": gen}, **kw) if kind == "dist" else MTDistGenMove(gen, num_try=int(fx["K"]), independent=True, **kw)
    return StretchMove(**kw), move, pc


@pytest.mark.parametrize("kind,name", mi.REFERENCE_CHAINS)
def test_numpy_mode_lands_on_the_references_periodic_chain(kind, name):
    """rng="numpy" through the drop-in moves: the reference's seeds, the reference's chain - the stretch iterations wrap on the
    device (hens_set_periodic through DeviceMove._apply_periodic), the move's accepted points stay outside [0, period)."""
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.state import State
    fx = mi.load_reference_chain(kind, name)
    prob = mi.FixtureProblem(fx)
    prior, _ = dm.fixture_containers(fx)
    T, W, D, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"])
    np.random.seed(int(fx["seed_construct"]))                 # R := snapshot of G at construction
    stretch, move, _ = _periodic_moves(kind, fx, "numpy")
    s = EnsembleSampler(W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), prior, moves=[(stretch, 0.5), (move, 0.5)], tempering_kwargs=dict(ntemps=T))
    np.random.seed(int(fx["seed_run"]))
    outside = 0
    for it, st in enumerate(s.sample(fx["x0"], iterations=n, store=False)):
        st = State(st, copy=True)
        what = f"{name}, iteration {it}"
        xs = fx["all_x"][it]
        assert np.array_equal(st.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D), xs), f"{what}: positions"
        cr.check_P(np.asarray(st.log_prior).reshape(T, W), fx["all_P"][it], prob, xs, what)
        tol.check_logl(np.asarray(st.log_like).reshape(T, W), fx["all_L"][it], tol.RTOL_L, what)
        np.testing.assert_allclose(st.betas, fx["all_betas"][it], rtol=1e-13, atol=0, err_msg=what)
        outside += int(cr._outside_period(xs, prob.period).sum())
    assert np.array_equal(np.asarray(move.accepted).reshape(T, W), fx["accepted_dist" if kind == "dist" else "accepted_mt"])
    assert np.array_equal(stretch.accepted, fx["accepted_stretch"]) and stretch.num_proposals + move.num_proposals == n
    assert outside > 0, "no walker outside [0, period): the move's points were wrapped, or never accepted there"


@pytest.mark.parametrize("kind,name", mi.REFERENCE_CHAINS)
def test_device_draws_in_the_numpy_loop_with_periodic_moves_are_the_composed_specification(kind, name):
    """The fixture's move list with rng="philox" under the sampler's NumPy host loop: every proposal is one hens_step iteration of
    ITS move, chosen by the sampler's stream, each stating its periods first (DeviceMove._apply_periodic).  Replayed iteration by
    iteration through the composed specification with the draws the context exports."""
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.state import State
    fx = mi.load_reference_chain(kind, name)
    prob = mi.FixtureProblem(fx)
    prior, _ = dm.fixture_containers(fx)
    T, W, D, n, seed = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"]), 11
    stretch, move, _ = _periodic_moves(kind, fx, "philox")
    np.random.seed(5)
    s = EnsembleSampler(W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), prior, moves=[(stretch, 0.5), (move, 0.5)], tempering_kwargs=dict(ntemps=T),
                        seed=seed)
    slot = mi.fixture_slot(kind, fx, prob, weight=1.0)
    cov, st, done = mi.Coverage(T), None, 0
    for it, state in enumerate(s.sample(fx["x0"], iterations=n, store=False)):
        state = State(state, copy=True)
        eng = s.engine
        what = f"{name} under device draws, iteration {it}"
        if st is None:                          # the start as the context evaluated it
            assert np.array_equal(eng.period, prob.period)
            st = ru.OracleState(fx["x0"], fx["L0"], fx["P0"], fx["betas0"])
        ran_slot = move.num_proposals > done
        done = move.num_proposals
        assert eng.iteration() == it + 1
        now = slot if ran_slot else None        # (the context's MH slot as the proposal left it: weight 1, or empty)
        d = cr.DeviceDraws(eng, seed, prob, now)(it, what)
        assert d["is_mh"] == ran_slot
        assert cr.spec_iteration(st, prob, now, d, period=prob.period, counts=cov, what=what) == ran_slot
        cov.slot_iters += int(ran_slot)
        xd = state.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D)
        assert np.array_equal(xd, st.x), f"{what}: x differs from the specification in {int((xd != st.x).any(axis=-1).sum())} walkers"
        cr.check_P(np.asarray(state.log_prior).reshape(T, W), st.P, prob, xd, what)
        tol.check_logl(np.asarray(state.log_like).reshape(T, W), st.L, tol.RTOL_L, what)
        np.testing.assert_allclose(state.betas, st.betas, rtol=1e-13, atol=0, err_msg=what)
    assert np.array_equal(np.asarray(move.accepted).reshape(T, W), st.mh_accepted) and np.array_equal(stretch.accepted, st.accepted)
    assert 0 < cov.slot_iters < n and cov.knives == 0 and st.min_margin > 1e-12
    assert (cov.slot_accepted > 0).all() and (cov.stretch_accepted > 0).all(), "both moves accept on every rung"
    assert cov.slot_outside_period_accepted > 0 and cov.seam_wrapped_accepted > 0
