"""Full leaf covariances for the Philox in-model Gaussian move of hens_rj_step (-m gpu; hens_rj_set_mh_chol): a leaf's step is
L z - step_d = sum_{j <= d} L[d][j] z_j in ascending j, z the unit normals the diagonal path draws for the leaf's coordinates."""
import numpy as np
import pytest

from tests import tolerance_log as tol
from tests.test_hip_rj import RTOL_L, _replay_oracle_class, knife
from tests.test_hip_rj_stretch import BOXES, KINDS, NAMES, _model, _oracle_branches

pytestmark = pytest.mark.gpu
SCALE = np.array([[1e-2, 1e-2, 1e-3], [1e-2, 1e-2, 1e-2]])
UNIT_L = np.array([[[1.0, 0.0, 0.0], [0.5, 0.8, 0.0], [-0.3, 0.4, 0.7]],
                   [[1.0, 0.0, 0.0], [-0.6, 0.9, 0.0], [0.2, -0.5, 1.1]]])
CHOL = SCALE[:, :, None] * UNIT_L                                  # lower triangular, positive diagonal


def _engine(T, W, nl_max, nl_min, ndata, seed, start_leaves, schedule="separate_branches", start=None):
    from eryn_amd.rj import RJEngine
    brs, t, y, sigma, x, inds, betas0 = _model(T, W, nl_max, nl_min, ndata, seed, start_leaves, start=start)
    eng = RJEngine(T, W, brs, t, y, sigma, seed=seed)
    eng.upload(x, inds, betas=betas0)
    eng.eval_state()
    eng.set_schedule(schedule)
    return eng, brs, t, y, sigma, betas0


def _lz(L, z, offsets, nl_max):
    """L @ z per leaf slot in the stated order: ascending j, every product and sum rounded (no FMA)."""
    out = np.zeros_like(z)
    for bi in range(len(nl_max)):
        for n in range(nl_max[bi]):
            i0 = offsets[bi] + 3 * n
            for d in range(3):
                acc = L[bi, d, 0] * z[..., i0]
                for j in range(1, d + 1):
                    acc = acc + L[bi, d, j] * z[..., i0 + j]
                out[..., i0 + d] = acc
    return out


def test_diagonal_factor_is_the_chain_of_set_mh_scale():
    T, W, nl_max, nl_min, seed = 3, 12, (3, 4), (0, 0), 41
    a, *_ = _engine(T, W, nl_max, nl_min, 60, seed, (2, 1))
    b, *_ = _engine(T, W, nl_max, nl_min, 60, seed, (2, 1))
    a.set_mh_scale(SCALE)
    b.set_mh_chol(np.stack([np.diag(s) for s in SCALE]))
    for it in range(6):
        assert np.array_equal(a.debug_draws(it)["step"], b.debug_draws(it)["step"]), f"exported step, iteration {it}"
    for n in (2, 4):
        a.step(n)
        b.step(n)
        (xa, ia, La, Pa, ba), (xb, ib, Lb, Pb, bb) = a.download(), b.download()
        for k in NAMES:
            assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"{k} differs"
        assert np.array_equal(La, Lb) and np.array_equal(Pa, Pb) and np.array_equal(ba, bb)
    ca, cb = a.counters(), b.counters()
    assert np.array_equal(ca["accepted_mh"], cb["accepted_mh"]) and np.array_equal(ca["accepted_bd"], cb["accepted_bd"])
    assert ca["accepted_mh"].sum() > 0
    a.close()
    b.close()


@pytest.mark.parametrize("T,W,nl_max", [(3, 12, (3, 4)), (2, 16, (12, 12))])       # (12, 12): a leaf straddles coordinate 64
def test_exported_step_is_L_times_the_unit_normals(T, W, nl_max):
    seed = 43
    a, *_ = _engine(T, W, nl_max, (0, 0), 60, seed, (2, 2))
    b, *_ = _engine(T, W, nl_max, (0, 0), 60, seed, (2, 2))
    a.set_mh_scale(np.ones((2, 3)))
    b.set_mh_chol(CHOL)
    for it in (0, 1, 64):
        z, st = a.debug_draws(it)["step"], b.debug_draws(it)["step"]
        assert np.array_equal(st, _lz(CHOL, z, a.off, nl_max)), f"iteration {it}"
        assert np.abs(z).max() > 1.0 and np.abs(z).max() < 7.0
    a.close()
    b.close()


def _replay_fullcov(T, W, nl_max, nl_min, ndata, schedule, iters, seed, start_leaves, start=None, on_record=None):
    """hens_rj_step with hens_rj_set_mh_chol replayed through the oracle (tests/test_hip_rj.py's replay class: _draw_steps reads
    the exported, correlated step) at the bars of DESIGN section 2.  ``start``: tests/test_hip_rj_stretch.py's _model; ``on_record``:
    called with every iteration's trace record of the oracle."""
    eng, brs, t, y, sigma, betas0 = _engine(T, W, nl_max, nl_min, ndata, seed, start_leaves, schedule, start=start)
    eng.set_mh_chol(CHOL)
    x0, inds0, L0, P0, _ = eng.download()
    o = _replay_oracle_class()(_oracle_branches(nl_max, nl_min), x0, inds0, t, y, sigma, None, None, betas0, schedule=schedule,
                               record=True)
    assert np.array_equal(o.st.P, P0)
    tol.check_logl(L0, o.st.L, RTOL_L, "template log-like")
    offsets = {b.name: eng.off[i] for i, b in enumerate(brs)}
    mh_acc, bd_acc, done = np.zeros((T, W)), np.zeros((T, W)), 0
    for n in (3, iters - 3):
        it0 = eng.iteration()
        eng.step(n)
        eng.synchronize()
        for it in range(it0, it0 + n):
            o.load(eng.debug_draws(it), offsets)
            acc, bi, racc = o.iteration()
            rec = o.trace.pop()
            assert not knife(rec["mh_lnpdiff"], rec["mh_u_acc"]).any(), "knife-edge accept test"
            if on_record is not None:
                on_record(rec)
            mh_acc += acc
            bd_acc += racc
        done += n
        what = f"hens_rj_step (full covariance, {schedule}) vs oracle after {done} iterations"
        x1, inds1, L1, P1, betas1 = eng.download()
        for k in NAMES:
            assert np.array_equal(inds1[k], o.st.inds[k]), f"{what}: leaf masks of {k}"
            assert np.array_equal(x1[k], o.st.x[k]), f"{what}: coordinates of {k} (dead slots included)"
        assert np.array_equal(P1, o.st.P), f"{what}: log-prior"
        tol.check_logl(L1, o.st.L, RTOL_L, what)
        np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
        c = eng.counters()
        assert np.array_equal(c["accepted_mh"], mh_acc) and np.array_equal(c["accepted_bd"], bd_acc), f"{what}: accept counters"
        assert c["num_mh"] == done and c["num_bd"] == done
        assert np.array_equal(c["swaps_last"], o.swaps_accepted), f"{what}: swap counts of the last cascade"
    eng.close()
    print(f"in-model accepted {int(mh_acc.sum())} of {mh_acc.size * iters}, birth / death accepted {int(bd_acc.sum())}")
    # both outcomes of the move under test.  (Nothing is asked of the birth / death move's outcomes here - its counters are held to
    # the oracle's above, its coverage is tests/test_hip_rj.py's: the oracle run with NumPy streams on (2, 64, (2, 3)) "together" at
    # 130 data points accepts no birth / death proposal in 20 iterations, whatever the seed.)
    assert 0 < mh_acc.sum() < mh_acc.size * iters


@pytest.mark.parametrize("T,W,nl_max,nl_min,ndata,schedule,iters,start_leaves", [
    (3, 12, (3, 4), (0, 0), 60, "separate_branches", 6, (2, 1)), (3, 12, (3, 4), (0, 0), 130, "separate_branches", 6, (2, 1)),
    (2, 64, (2, 3), (0, 0), 60, "together", 6, (2, 2)), (2, 64, (2, 3), (0, 0), 130, "together", 6, (2, 2)),
    (2, 16, (12, 12), (0, 0), 130, "separate_branches", 6, (2, 10))])      # sine slot 9 is active: the leaf across coordinate 64 moves
def test_fullcov_production_step_replayed_through_the_oracle(T, W, nl_max, nl_min, ndata, schedule, iters, start_leaves):
    _replay_fullcov(T, W, nl_max, nl_min, ndata, schedule, iters, seed=47, start_leaves=start_leaves)


def test_sample_covariance_of_the_exported_steps():
    """2 x 64 walkers x 20 iterations = 2560 steps per leaf slot: every entry of the sample covariance within 5 standard
    deviations sqrt((c_ii c_jj + c_ij^2) / N) of cov = L L^T, every mean within 5 sqrt(c_ii / N) of 0."""
    T, W, nl_max, iters = 2, 64, (2, 2), 20
    eng, *_ = _engine(T, W, nl_max, (0, 0), 60, 53, (2, 1))
    eng.set_mh_chol(CHOL)
    steps = np.concatenate([eng.debug_draws(it)["step"].reshape(T * W, -1) for it in range(iters)])
    N = steps.shape[0]
    assert N == 2560
    for bi in range(2):
        cov = CHOL[bi] @ CHOL[bi].T
        for n in range(nl_max[bi]):
            s = steps[:, eng.off[bi] + 3 * n: eng.off[bi] + 3 * n + 3]
            mean, samp = s.mean(axis=0), (s.T @ s) / N
            for i in range(3):
                assert abs(mean[i]) <= 5 * np.sqrt(cov[i, i] / N), (bi, n, i)
                for j in range(3):
                    sd = np.sqrt((cov[i, i] * cov[j, j] + cov[i, j] ** 2) / N)
                    assert abs(samp[i, j] - cov[i, j]) <= 5 * sd, (bi, n, i, j, samp[i, j], cov[i, j], sd)
    eng.close()


def test_not_positive_definite_is_a_value_error():
    eng, *_ = _engine(2, 12, (3, 4), (0, 0), 60, 59, (2, 1))
    bad = CHOL.copy()
    bad[1, 2, 2] = 0.0                                            # singular
    with pytest.raises(ValueError):
        eng.set_mh_chol(bad)
    bad = CHOL.copy()
    bad[0, 1, 1] = -bad[0, 1, 1]
    with pytest.raises(ValueError):
        eng.set_mh_chol(bad)
    bad = CHOL.copy()
    bad[0, 0, 2] = 1e-3                                           # not lower triangular
    with pytest.raises(ValueError):
        eng.set_mh_chol(bad)
    eng.set_mh_chol(CHOL)
    eng.step(1)
    eng.close()


def test_rj_sampler_philox_mode_with_an_off_diagonal_covariance():
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, TemplateLikelihood
    from eryn_amd.state import State
    T, W, N = 4, 64, 100
    t = np.linspace(-1, 1, N)
    rs = np.random.RandomState(3)
    y = 3.0 * np.exp(-((t - 0.1) ** 2) / (2 * 0.1 ** 2)) + 1.0 * np.sin(2 * np.pi * 5.0 * t + 1.0) + 1.5 * rs.randn(N)
    priors = {"gauss": {0: uniform_dist(2.5, 3.5), 1: uniform_dist(-1, 1), 2: uniform_dist(0.01, 0.21)},
              "sine": {0: uniform_dist(0.5, 1.5), 1: uniform_dist(1.0, 20.0), 2: uniform_dist(0.0, 2 * np.pi)}}
    cov = {k: CHOL[i] @ CHOL[i].T for i, k in enumerate(NAMES)}
    kw = dict(tempering_kwargs=dict(ntemps=T), branch_names=NAMES, nleaves_max={"gauss": 4, "sine": 3}, rng="philox", seed=8)
    like = TemplateLikelihood(KINDS, t, y, 1.5)
    with pytest.raises(ValueError):                               # np.linalg.cholesky: not positive definite
        RJEnsembleSampler(W, {k: 3 for k in NAMES}, like, priors,
                          moves=GaussianLeafMove({k: np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) for k in NAMES}), **kw)
    s = RJEnsembleSampler(W, {k: 3 for k in NAMES}, like, priors, moves=GaussianLeafMove(cov), **kw)
    coords = {"gauss": np.zeros((T, W, 4, 3)), "sine": np.zeros((T, W, 3, 3))}
    inds = {"gauss": np.zeros((T, W, 4), dtype=bool), "sine": np.zeros((T, W, 3), dtype=bool)}
    coords["gauss"][:, :, 0] = [3.0, 0.1, 0.1]
    coords["sine"][:, :, 0] = [1.0, 5.0, 1.0]
    inds["gauss"][:, :, 0] = inds["sine"][:, :, 0] = True
    last = s.run_mcmc(State(coords, inds=inds), 10, burn=2, thin_by=2, store=True)
    assert len(s.chain) == 10 and s.iteration == 12 and s.moves[0].num_proposals == 22
    assert np.isfinite(last.log_like).all()
    assert s.moves[0].accepted.sum() > 0 and s.rj_num_proposals_all == 22 and s.rj_accepted_all.sum() > 0
    # the correlated step the device draws is L z of the covariance's Cholesky factor
    L = np.stack([np.linalg.cholesky(cov[k]) for k in NAMES])
    st = s.engine.debug_draws(0)["step"]
    ref = RJEnsembleSampler(W, {k: 3 for k in NAMES}, like, priors, moves=GaussianLeafMove({k: np.eye(3) for k in NAMES}), **kw)
    z = ref.engine.debug_draws(0)["step"]
    assert np.array_equal(st, _lz(L, z, s.engine.off, (4, 3)))
    s.engine.close()
    ref.engine.close()
