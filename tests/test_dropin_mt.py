"""``eryn_amd.moves.MTDistGenMove`` + ``StretchMove`` under the REAL reference sampler (build container only; CPU): the unmodified
``eryn.ensemble.EnsembleSampler`` drives both moves through ``run_mcmc`` and must land on the chain captured from the reference's own
moves (tests/golden/mt/mt1_mix.npz).  As in tests/test_dropin_dist.py the device context is a stand-in with the same method surface
whose compute is the specification (tests/mt_move.py, the pinned oracle): what is under test is the plugin protocol - the order of
the draws on the two streams among them - the kernels are pinned by the -m gpu tests.

Skipped where the reference tree does not exist (the GPU box)."""
import os
import sys

import numpy as np

from oracle import eryn_oracle as orc
from tests import mt_move as mt
from tests import prior_terms as pt
from tests.test_dropin_reference import OracleEngine, _loglike, eryn  # noqa: F401  (eryn: the module fixture that imports the reference)
from tests.test_prior_terms import needs_reference

pytestmark = needs_reference


class SpecEngine(OracleEngine):
    """OracleEngine under prior terms, with the two calls the new move makes."""

    def __init__(self, T, W, D, loglike, prior, **kw):
        OracleEngine.__init__(self, T, W, D, loglike, prior["lo"], prior["hi"], **kw)
        self.prior, self.gen, self.num_try = prior, None, None

    def set_mt_dist_proposal(self, terms, num_try, weight):
        from eryn_amd.prior import prior_spec
        self.gen, self.num_try = prior_spec(terms, self.D).terms, int(num_try)
        self.calls.append(("mt_dist_proposal", self.num_try, weight))

    def mt_dist_step(self, q, u_pick, u_acc, want=()):
        q = np.asarray(q).reshape(self.T, self.W, self.num_try, self.D)
        keep, pick, lsw, aux, fac = mt.mt_step(self.x, self.L, self.P, self.betas, q, np.asarray(u_pick), np.asarray(u_acc), self.prior, self.gen,
                                               self.loglike)
        out = dict(keep=keep, pick=pick, lsw=lsw, aux_lsw=aux, factors=fac)
        return {k: v for k, v in out.items() if k == "keep" or k in want} if want else keep


def test_hip_mt_dist_gen_move_under_the_real_sampler(eryn, monkeypatch):  # noqa: F811
    from eryn.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves import MTDistGenMove, StretchMove
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_dist as mgd             # (the reference's constructors with the fixture's arguments)
    fx = mt.load_fixture("mt1_mix")
    prior, gen = mt.fixture_specs(fx)
    prior_c, gen_c = mt.fixture_containers(fx)
    T, W, D, K, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["K"]), int(fx["nsteps"])
    mu, invcov = fx["mu"], fx["invcov"]
    monkeypatch.setattr(orc, "box_log_prior", pt.box_prior_substitute(prior))
    like = GaussianLikelihood(mu, invcov)
    stretch = StretchMove(a=float(fx["a"]), likelihood=like, prior_box=prior_c)
    move = MTDistGenMove(gen_c, num_try=K, independent=True, likelihood=like, prior_box=prior_c)
    eng = SpecEngine(T, W, D, lambda x: _loglike(x, mu, invcov), prior, a=float(fx["a"]))
    stretch.attach_engine(eng)
    move.attach_engine(eng)
    np.random.seed(int(fx["seed_construct"]))
    s = EnsembleSampler(W, D, _loglike, mgd.container(fx["prior_kind"], fx["prior_p0"], fx["prior_p1"]), args=[mu, invcov], vectorize=True,
                        moves=[(stretch, 0.5), (move, 0.5)], tempering_kwargs=dict(ntemps=T))
    assert move.temperature_control is s.temperature_control and move.accepted.shape == (T, W)
    np.random.seed(int(fx["seed_run"]))
    state = s.run_mcmc(fx["x0"], n, store=True)
    assert np.array_equal(state.branches["model_0"].coords[:, :, 0, :], fx["all_x"][n - 1])
    assert np.array_equal(state.log_like, fx["all_L"][n - 1]) and np.array_equal(state.log_prior, fx["all_P"][n - 1])
    assert np.array_equal(state.betas, fx["all_betas"][n - 1])
    assert np.array_equal(s.temperature_control.swaps_accepted, fx["all_swaps_accepted"][n - 1])
    assert np.array_equal(move.accepted, fx["accepted_mt"]) and move.num_proposals == int(fx["num_proposals_mt"])
    assert np.array_equal(stretch.accepted, fx["accepted_stretch"])
    chain = s.get_chain()["model_0"]
    for it in range(n):
        assert np.array_equal(chain[it][:, :, 0, :], fx["all_x"][it]), f"stored step {it}"
    # the sums of the last move iteration, as the reference's move carries them
    assert np.array_equal(move.log_sum_weights.reshape(T, W), fx["mt_lsw"][-1], equal_nan=True)
    assert np.array_equal(move.aux_log_sum_weights.reshape(T, W), fx["mt_aux_lsw"][-1], equal_nan=True)
    assert ("mt_dist_proposal", K, 1.0) in eng.calls and "upload" in eng.calls
