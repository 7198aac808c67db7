"""The cases of tests/move_interactions.py sized on the CPU (no GPU): every run that tests/test_hip_move_interactions.py replays on
the device goes through the composed specification alone (tests/composed_replay.py: ``SpecDraws`` - the production draws of
tests/production_draws.py, dist_move.dist_draws, mt_move.mt_draws and their pick and accept uniforms) and must meet the coverage
conditions of ``move_interactions.check_coverage``

  * over the case's own calls (1, n), as the GPU replay asks for them, and
  * over twice the iterations, calls (1, 2 n + 1), with a factor of two to spare.

The device's non-uniform generator draws are only within their bound E of the specification's, so a decision may fall differently
there; the factor of two is what makes a coverage assertion on the GPU a statement about the device and not about the choice of shape
or seed.  A case that misses is changed in tests/move_interactions.py (shape, seed, box, generator), never relaxed on the GPU side.
"""
import numpy as np
import pytest

from tests import composed_replay as cr
from tests import dist_move as dm
from tests import gibbs_move as gm
from tests import move_interactions as mi
from tests import mt_move as mt
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import replay_utils as ru


def spec_start(c, prob):
    """(OracleState, betas0) of a case's start on the specification's side."""
    T, W, D = c["T"], c["W"], c["D"]
    betas0, x0 = mi.case_inputs(c, prob)
    x = x0.copy()
    P = pt.log_prior(prob.prior, x.reshape(-1, D)).reshape(T, W)
    assert np.isfinite(P).all(), "a start outside the prior's support"
    L = prob.loglike(x.reshape(-1, D)).reshape(T, W)
    return ru.OracleState(x, L, P, betas0), betas0


def spec_run(c, run, calls):
    prob = mi.case_problem(c, run[1])
    slot = mi.slot_of(c, run, prob)
    st, betas0 = spec_start(c, prob)
    cov = mi.Coverage(c["T"])
    gibbs = None if c["gibbs"] is None else dict(stretch=c["gibbs"], mh=c["gibbs"])
    if gibbs is not None:
        cov.books = gm.BlockBooks(c["T"], c["W"], len(gibbs["stretch"]), len(gibbs["mh"]))
    draws = cr.SpecDraws(c["seed"], c["T"], c["W"], prob, slot, nsplits=c["nsplits"], gibbs=gibbs)
    kinds = cr.run_spec(draws, st, prob, slot, calls, counts=cov, what=mi.run_id("spec", run), period=prob.period, nsplits=c["nsplits"],
                        lag=mi.LAG, nu=mi.NU, adaptive=c["adaptive"], stop_adaptation=c["stop_adaptation"], gibbs=gibbs)
    assert kinds == [pd.is_mh(c["seed"], it, c["weight"]) for it in range(sum(calls))]
    return st, betas0, cov


@pytest.mark.parametrize("name,run", mi.RUNS, ids=mi.RUN_IDS)
def test_the_specification_alone_meets_the_coverage_conditions(name, run):
    c = mi.CASES[name]
    what = mi.run_id(name, run)
    st, betas0, cov = spec_run(c, run, c["calls"])
    mi.check_coverage(c, run, cov, betas0, st.betas, st.swaps_total, spare=1, what=what)
    assert cov.knives == 0 and st.min_margin > 1e-12, f"{what}: a decision on the knife edge within the case's own iterations: pick another seed"
    assert cov.books is None or (cov.books.knives == 0 and cov.books.min_margin > 1e-12)
    n2 = 2 * sum(c["calls"])
    st, betas0, cov = spec_run(c, run, (1, n2 - 1))
    mi.check_coverage(c, run, cov, betas0, st.betas, st.swaps_total, spare=2, what=f"{what}, {n2} iterations")
    assert np.all(np.isfinite(st.betas)) and np.all(st.betas >= 0) and np.all(np.diff(st.betas) <= 0)


def test_the_case_table_is_what_the_module_says():
    """The column blocks the table's comments state, the periods' geometry, and the families' features."""
    cbs = {(6, 64): 16, (10, 128): 8, (33, 66): 2, (64, 16): 2, (4, 64): 32, (65, 16): 0, (3, 67): 0, (130, 16): 0, (3, 40): 0}
    for (T, W), cb in cbs.items():
        assert pd.label_cb(T, W) == cb
    for name, c in mi.CASES.items():
        betas0 = mi.ld.ladder(c["family"], c["T"], c["D"])
        assert ("beta0" in c["exempt"]) == (betas0[-1] != 0.0), name
        assert ("ladder_moved" in c["exempt"]) == (not c["adaptive"]), name
        assert ("steep_gap" in c["exempt"]) == (c["family"] == "user" and mi.ld.user_features(c["T"])[1] is not None), name
        assert c["n"] >= 5 and c["calls"] == (1, c["n"])
        if c["family"] == "inf":
            assert any(gen == "box" for _, gen in c["runs"]), f"{name}: a beta = 0 rung and no run on the prior's own box"
        if not c["periodic"]:
            continue
        for _, gen in c["runs"]:
            prob = mi.case_problem(c, gen)
            assert prob.wide and all(prob.period[d] > 0 for d in prob.wide)
            for d in prob.wide:          # half a period beyond [0, period] on both sides: the generator's term and the prior's support
                p = prob.period[d]
                assert prob.gen["kind"][d] == pt.UNIFORM and prob.gen["lo"][d] == -0.5 * p and prob.gen["hi"][d] == 1.5 * p
                assert prob.prior["lo"][d] <= -0.5 * p and prob.prior["hi"][d] >= 1.5 * p
            x0 = prob.x0(c["T"], c["W"])
            assert np.isfinite(pt.log_prior(prob.prior, x0.reshape(-1, c["D"]))).all()


def test_a_wrapped_independence_proposal_is_another_chain():
    """What the periodic cases can see: the composed specification with the move's proposals wrapped into [0, period) - the mistake the
    device could make - leaves the unwrapped chain within the case's own iterations."""
    name, run = "periodic_T4_D16", ("dist", "mixed")
    c = mi.CASES[name]
    st, _, cov = spec_run(c, run, c["calls"])
    assert cov.slot_outside_period_accepted > 0
    prob = mi.case_problem(c, run[1])
    slot = mi.slot_of(c, run, prob)
    draws = cr.SpecDraws(c["seed"], c["T"], c["W"], prob, slot)

    def wrapped(it, what=""):
        d = draws(it, what)
        if d["is_mh"]:
            d["q"] = mi.orc_wrap(d["q"], prob.period)
        return d

    st2, _ = spec_start(c, prob)
    cr.run_spec(wrapped, st2, prob, slot, c["calls"], period=prob.period, lag=mi.LAG, nu=mi.NU)
    assert not np.array_equal(st2.x, st.x)


def test_the_shard_cases_tell_the_rung_offset():
    """Part D's premise on the CPU: on an unequal ladder the specification run on rungs 1:3 with ``betas[0:2]`` in place of
    ``betas[1:3]`` keeps other walkers, and the draws of rungs 1:3 are not those of rungs 0:2."""
    for D in mi.SHARD_D:
        prob, betas, x, L, P = mi.shard_inputs(D)
        r0, r1 = mi.SHARD_RANGE
        T, W = mi.SHARD_T, mi.SHARD_W
        q, _, _ = dm.dist_draws(mi.SEED, 0, r1 - r0, W, prob.gen, rung_begin=r0)
        whole, _, _ = dm.dist_draws(mi.SEED, 0, T, W, prob.gen)
        assert np.array_equal(q, whole[r0:r1]) and not np.array_equal(q, whole[:r1 - r0])
        u = dm.accept_uniforms(mi.SEED, 0, r1 - r0, W, rung_begin=r0)
        keeps = [dm.dist_step(x[r0:r1].copy(), L[r0:r1].copy(), P[r0:r1].copy(), b, q, u, prob.prior, prob.gen, prob.loglike)[3]
                 for b in (betas[r0:r1], betas[:r1 - r0])]
        assert not np.array_equal(*keeps), f"D = {D}: the wrong rungs' betas keep the same walkers"
        K = mi.SHARD_K
        qk, _, _ = mt.mt_draws(mi.SEED, 0, r1 - r0, W, K, prob.gen, rung_begin=r0)
        up = mt.pick_uniforms(mi.SEED, 0, r1 - r0, W, rung_begin=r0)
        assert np.array_equal(up, mt.pick_uniforms(mi.SEED, 0, T, W)[r0:r1])
        outs = [mt.mt_step(x[r0:r1].copy(), L[r0:r1].copy(), P[r0:r1].copy(), b, qk, up, u, prob.prior, prob.gen, prob.loglike)
                for b in (betas[r0:r1], betas[:r1 - r0])]
        assert not (np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])), f"D = {D}: multiple try"


@pytest.mark.parametrize("kind,name", mi.REFERENCE_CHAINS)
def test_the_composed_specification_lands_on_the_references_periodic_chains(kind, name, monkeypatch):
    """StretchMove(periodic=pc) beside DistributionGenerate / MTDistGenMove(num_try=4) with the same PeriodicContainer, run by the
    unmodified reference (tests/golden/make_golden_dist.py, make_golden_mt.py): the composed specification - the stretch iterations
    wrapped, the move's never - lands on the chain bit for bit; wrapping the move's points leaves it."""
    from oracle import eryn_oracle as orc
    fx = mi.load_reference_chain(kind, name)
    prob = mi.FixtureProblem(fx)
    T, W, D, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"])
    assert (T, D) == (3, 4) and 12 <= W <= 24 and np.count_nonzero(prob.period) == 2 and float(fx["a"]) == 2.0
    for d in np.flatnonzero(prob.period):        # the wider-than-a-period box, prior and generator
        p = prob.period[d]
        assert prob.prior["lo"][d] == prob.gen["lo"][d] == -0.5 * p and prob.prior["hi"][d] == prob.gen["hi"][d] == 1.5 * p
    monkeypatch.setattr(orc, "box_log_prior", pt.box_prior_substitute(prob.prior))
    slot = mi.fixture_slot(kind, fx, prob)
    st = ru.OracleState(fx["x0"], fx["L0"], fx["P0"], fx["betas0"])
    wrapped = ru.OracleState(fx["x0"], fx["L0"], fx["P0"], fx["betas0"])
    cov = mi.Coverage(T)
    for it in range(n):
        d, rec = mi.fixture_draws(kind, fx, it)
        assert cr.spec_iteration(st, prob, slot, d, period=prob.period, counts=cov, what=f"{name}, iteration {it}") == d["is_mh"]
        cov.slot_iters += int(d["is_mh"])
        for k, a in (("x", st.x), ("L", st.L), ("P", st.P), ("betas", st.betas)):
            assert np.array_equal(a, rec[k]), f"{name}, iteration {it}: {k} differs from the reference's chain"
        assert np.array_equal(st.swaps_last, rec["swaps_accepted"])
        if d["is_mh"]:
            d = dict(d, q=mi.orc_wrap(d["q"], prob.period))
        cr.spec_iteration(wrapped, prob, slot, d, period=prob.period)
    assert np.array_equal(st.mh_accepted, fx["accepted_dist" if kind == "dist" else "accepted_mt"]) and np.array_equal(st.accepted, fx["accepted_stretch"])
    assert (cov.slot_accepted > 0).all() and (cov.stretch_accepted > 0).all(), "both moves accept on every rung"
    assert cov.slot_outside_period_accepted > 0 and cov.seam_wrapped_accepted > 0 and cov.knives == 0
    assert not np.array_equal(wrapped.x, st.x), "a wrapped independence proposal must be another chain"
