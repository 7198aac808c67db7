"""DistributionGenerate in the samplers (eryn_amd/moves/distgen.py, eryn_amd/ensemble.py):

  * ``EnsembleSampler(rng="numpy")`` with the fixtures' seeds lands on the reference's chain (tests/golden/distgen/);
  * ``EnsembleSampler(rng="philox")`` over a Stretch + DistributionGenerate mix: ``DeviceBackend()`` bit-identical to ``Backend()`` -
    chain, ``accepted``, ``swaps_accepted`` and the moves' own counters - at ``thin_by`` 1 and 3; the chain is the context's own
    (hens_step with the generator in the MH slot);
  * the three-way Philox mix is refused.
"""
import numpy as np
import pytest

from tests import dist_move as dm
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests import tolerance_log as tol
from tests.test_hip_chain_store import assert_backends_equal, assert_state_equal, assert_totals_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", dm.FIXTURES)
def test_numpy_mode_lands_on_the_reference_chain(name):
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves import DistributionGenerate, StretchMove
    from eryn_amd.state import State
    fx = dm.load_fixture(name)
    prior_spec, _ = dm.fixture_specs(fx)
    prior, gen = dm.fixture_containers(fx)
    T, W, D, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"])
    np.random.seed(int(fx["seed_construct"]))                 # R := snapshot of G at construction
    move = DistributionGenerate({"model_0": gen})
    moves = [(StretchMove(), 0.5), (move, 0.5)] if int(fx["mix"]) else move
    s = EnsembleSampler(W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), prior, moves=moves,
                        **(dict(tempering_kwargs=dict(ntemps=T)) if T > 1 else {}))
    np.random.seed(int(fx["seed_run"]))
    x0 = fx["x0"] if T > 1 else fx["x0"][0]
    for it, st in enumerate(s.sample(x0, iterations=n, store=False)):
        st = State(st, copy=True)
        what = f"{name}, iteration {it}"
        xs = fx["all_x"][it]
        assert np.array_equal(st.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D), xs), f"{what}: positions"
        r = pt.worst_ratio(np.asarray(st.log_prior).reshape(-1), prior_spec, xs.reshape(-1, D))
        assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"
        tol.check_logl(np.asarray(st.log_like).reshape(T, W), fx["all_L"][it], tol.RTOL_L, what)
        if T > 1:
            np.testing.assert_allclose(st.betas, fx["all_betas"][it], rtol=1e-13, atol=0, err_msg=what)
    assert np.array_equal(np.asarray(move.accepted).reshape(T, W), fx["accepted_dist"]) and move.num_proposals == int(fx["num_proposals_dist"])
    if int(fx["mix"]):
        assert np.array_equal(s.moves[0].accepted, fx["accepted_stretch"])


def _philox_sampler(c, prob, backend, seed=dm.SEED):
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.moves import DistributionGenerate, StretchMove
    prior, gen = prob.containers()
    moves = [(StretchMove(), 1.0 - c["weight"]), (DistributionGenerate({"model_0": gen}), c["weight"])]
    return EnsembleSampler(c["W"], c["D"], pu.device_likelihood(prob), prior, rng="philox", seed=seed, moves=moves, backend=backend,
                           tempering_kwargs=dict(ntemps=c["T"], adaptation_lag=50, adaptation_time=5))


@pytest.mark.parametrize("name", ["3x40x4_dense_terms", "4x64x16_diag_box_records"])
@pytest.mark.parametrize("thin", [1, 3])
def test_device_backend_is_the_host_backend(name, thin):
    from eryn_amd.backend import Backend, DeviceBackend
    c = dm.CASES[name]
    prob = dm.case_problem(c)
    x0 = prob.x0(c["T"], c["W"])
    a, b = _philox_sampler(c, prob, Backend()), _philox_sampler(c, prob, DeviceBackend())
    ra, rb = a.run_mcmc(x0, 6, thin_by=thin), b.run_mcmc(x0, 6, thin_by=thin)
    what = f"{name}, thin_by={thin}"
    assert_backends_equal(a.backend, b.backend, what)
    assert_totals_equal(a.backend, b.backend, what)
    assert_state_equal(ra, rb, what)
    for ma, mb in zip(a.moves, b.moves):
        assert np.array_equal(ma.accepted, mb.accepted) and ma.num_proposals == mb.num_proposals
    assert all(m.num_proposals > 0 and np.asarray(m.accepted).sum() > 0 for m in a.moves), "both moves of the mix ran and accepted"
    assert a.moves[0].num_proposals + a.moves[1].num_proposals == 6 * thin
    if thin == 1:
        # the chain is the context's: the same seed through hens_step with the generator in the MH slot
        from eryn_amd.engine import HipEnsemble
        terms = None if np.all(prob.prior["kind"] == pt.UNIFORM) else prob.prior
        eng = HipEnsemble(c["T"], c["W"], c["D"], pu.device_likelihood(prob), prob.lo, prob.hi, seed=dm.SEED, prior_terms=terms,
                          adaptation_lag=50, adaptation_time=5)
        from oracle import eryn_oracle as orc
        eng.upload(x0, betas=orc.make_ladder(c["D"], ntemps=c["T"]))
        eng.eval_state()
        eng.set_dist_proposal(prob.gen, c["weight"])
        eng.step(6)
        xd, Ld, Pd, bd = eng.download()
        assert np.array_equal(xd, ra.branches["model_0"].coords[:, :, 0, :]) and np.array_equal(Ld, ra.log_like) and np.array_equal(bd, ra.betas)
        assert eng.mh_counters()["num_proposals"] == a.moves[1].num_proposals
        eng.close()


def test_the_three_way_philox_mix_is_refused():
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.moves import DistributionGenerate, GaussianMove, StretchMove
    c = dm.CASES["4x72x16_diag_box"]
    prob = dm.case_problem(c)
    prior, gen = prob.containers()
    moves = [(StretchMove(), 0.4), (GaussianMove({"model_0": 0.01}), 0.3), (DistributionGenerate({"model_0": gen}), 0.3)]
    with pytest.raises(NotImplementedError) as e:
        EnsembleSampler(c["W"], c["D"], pu.device_likelihood(prob), prior, rng="philox", seed=1, moves=moves, tempering_kwargs=dict(ntemps=c["T"]))
    assert "at most one StretchMove with one GaussianMove or one DistributionGenerate" in str(e.value)
    # rng="numpy": the moves are host objects, any mix of the three steps
    s = EnsembleSampler(c["W"], c["D"], pu.device_likelihood(prob), prior, moves=moves, tempering_kwargs=dict(ntemps=c["T"]))
    np.random.seed(3)
    s.run_mcmc(prob.x0(c["T"], c["W"]), 8)
    assert all(m.num_proposals > 0 for m in s.moves) and sum(m.num_proposals for m in s.moves) == 8
    assert np.isfinite(s.get_log_like()).all()


def test_device_draw_moves_in_the_numpy_loop_push_the_slot_either_way():
    """StretchMove, GaussianMove and DistributionGenerate, each rng="philox", chosen per proposal by the sampler's own stream
    (ensemble.py:971): every proposal is one device iteration of ITS move - the MH slot is pushed either way as the choice
    alternates - and the accept counters of the three moves partition the proposals."""
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.moves import DistributionGenerate, GaussianMove, StretchMove
    c = dm.CASES["4x64x16_diag_box_records"]
    prob = dm.case_problem(c)
    prior, gen = prob.containers()
    T, W, D = c["T"], c["W"], c["D"]
    mvs = [(StretchMove(rng="philox"), 0.4), (GaussianMove({"model_0": (0.1 * float(prob.sig.min())) ** 2}, rng="philox"), 0.3),
           (DistributionGenerate({"model_0": gen}, rng="philox"), 0.3)]
    np.random.seed(5)
    s = EnsembleSampler(W, D, pu.device_likelihood(prob), prior, tempering_kwargs=dict(ntemps=T), moves=mvs, seed=3)
    last = s.run_mcmc(prob.x0(T, W), 30, store=False)
    st, g, dg = s.moves
    assert st.num_proposals + g.num_proposals + dg.num_proposals == 30 and min(st.num_proposals, g.num_proposals, dg.num_proposals) > 2
    cs, cm = s.engine.counters(), s.engine.mh_counters()
    assert np.array_equal(st.accepted, cs["accepted"]) and np.array_equal(g.accepted + dg.accepted, cm["accepted"])
    assert cs["num_proposals"] == st.num_proposals and cm["num_proposals"] == g.num_proposals + dg.num_proposals
    assert np.isfinite(last.log_like).all() and min(st.accepted.sum(), g.accepted.sum(), dg.accepted.sum()) > 0
    lo, hi = prob.prior["lo"], prob.prior["hi"]
    x = last.branches["model_0"].coords[:, :, 0, :]
    assert ((x >= lo) & (x <= hi)).all(), "a walker left the prior box"
