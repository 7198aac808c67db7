"""The multiple-try independence move on the device (hens_set_mt_dist_proposal, hens_mt_dist_step, hens_mt_debug_draws, the k_mt_dist
launch of hens_step; csrc/hens_mt.h) against its specification (tests/mt_move.py).

  1. teacher-forced: hens_mt_dist_step with the caller's tries on the issue's nine shapes - picks, keeps and positions bit for bit,
     lsw / aux_lsw / factors within 1.0 B of exact arithmetic (non-finite values exactly where the specification has them), {L, P}
     at the parity tests' bars;
  2. production replay: hens_step with the move in the mix, hens_mt_debug_draws / hens_debug_draws export every iteration's draws,
     the specification replays them; the tries against the Philox specification, try 0 against DistributionGenerate's export;
  3. the reference's fixtures through hens_mt_dist_step and through ``EnsembleSampler(moves=MTDistGenMove(...), rng="numpy")``;
  4. equivalences: one try against DistributionGenerate, walker records against the by-field state, DeviceBackend against Backend,
     a chain resumed from ``State.random_state``;
  5. refusals, each with its code and text, each leaving the context as it was.

Measured on an MI355X, the largest |value - exact| / B over all cases of parts 1 and 3 (printed by ``mt_move.assert_sums`` and logged
under each test in the tolerance report; profiles/mt_bound_ratios.txt): lsw 0.073, aux_lsw 0.109, factors 0.030.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import dist_move as dm
from tests import mt_move as mt
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import replay_utils as ru
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
LD = np.longdouble
SEED = mt.SEED


def _engine(prob, T, W, seed=SEED, **kw):
    from eryn_amd.engine import HipEnsemble
    terms = None if np.all(prob.prior["kind"] == pt.UNIFORM) else prob.prior
    return HipEnsemble(T, W, prob.D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=seed, prior_terms=terms, live_dangerously=True,
                       tempered=T > 1, **kw)


def _check_P(P, Pspec, prob, x, what):
    """Log-prior: under a box the constant, bit for bit; under terms within 1.0 B_P of exact arithmetic at the positions."""
    if np.all(prob.prior["kind"] == pt.UNIFORM):
        assert np.array_equal(P, Pspec), f"{what}: log-prior differs"
        return
    r = pt.worst_ratio(P.reshape(-1), prob.prior, x.reshape(-1, prob.D))
    print(f"{what}: |P - P*| / B_P <= {r:.3f}")
    assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"


def _start(eng, prob, T, W):
    eng.upload(prob.x0(T, W), betas=orc.make_ladder(prob.D, ntemps=T) if T > 1 else None)
    eng.eval_state()
    x, L, P, betas = eng.download()
    assert np.isfinite(P).all(), "a start outside the prior's support"
    return x, L, P, (betas if T > 1 else None)


def _no_knife(info, ex, what):
    with np.errstate(divide="ignore"):
        assert not pu.knife_edge(info["lnpdiff"], np.log(info["u_acc"])).any(), f"{what}: an accept decision on the knife edge: pick another seed"
    assert not mt.pick_knife(ex["c"], info["u_pick"], ex["B_c"]).any(), f"{what}: a pick on the knife edge: pick another seed"


# ---- 1. teacher-forced ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mt.CASES))
def test_mt_dist_step_with_the_callers_tries(name):
    c = mt.CASES[name]
    T, W, D, K = c["T"], c["W"], c["D"], c["K"]
    prob = mt.case_problem(c)
    eng = _engine(prob, T, W)
    x, L, P, betas = _start(eng, prob, T, W)
    eng.set_mt_dist_proposal(prob.gen, K, 0.5)
    accepted = picks = outside_old = inf_prior = 0
    for n in range(mt.FORCED_PROPOSALS):
        q, up, ua = mt.forced_inputs(c, prob, n)
        xs, Ls, Ps = x.copy(), L.copy(), P.copy()
        info = {}
        keep_s, pick_s, lsw_s, aux_s, fac_s = mt.mt_step(xs, Ls, Ps, betas, q, up, ua, prob.prior, prob.gen, prob.loglike, info=info)
        ex = mt.exact_mt(info, pick_s, betas, prob.prior, prob.gen)
        what = f"{name}, proposal {n}"
        _no_knife(info, ex, what)
        out = eng.mt_dist_step(q, up, ua, want=("pick", "lsw", "aux_lsw", "factors"))
        assert np.array_equal(out["pick"], pick_s), f"{what}: picks differ in {int((out['pick'] != pick_s).sum())} walkers"
        assert np.array_equal(out["keep"], keep_s), f"{what}: accept mask differs in {int((out['keep'] != keep_s).sum())} walkers"
        mt.assert_sums(out["lsw"], out["aux_lsw"], out["factors"], ex, what)
        xd, Ld, Pd, _ = eng.download()
        assert np.array_equal(xd, xs), f"{what}: positions differ"
        _check_P(Pd, Ps, prob, xd, what)
        tol.check_logl(Ld, Ls, tol.RTOL_L, what)
        old_out = np.isneginf(info["alq"]).reshape(T, W)
        assert not (out["keep"] & old_out).any(), f"{what}: an old point outside the generator was moved"
        assert np.array_equal(np.isnan(out["aux_lsw"]), np.isnan(aux_s))
        accepted += int(keep_s.sum())
        picks += int((pick_s != 0).sum())
        outside_old += int(old_out.sum())
        inf_prior += int(np.isinf(info["lp"]).sum())
        assert np.array_equal(eng.mt_dist_step(q, up, ua), mt.mt_step(xs, Ls, Ps, betas, q, up, ua, prob.prior, prob.gen, prob.loglike)[0]), \
            f"{what}: the same tries again, every output NULL"
        x, L, P, _ = eng.download()
        assert np.array_equal(x, xs), f"{what}: positions after the second proposal"
    mh = eng.mh_counters()
    assert mh["num_proposals"] == 2 * mt.FORCED_PROPOSALS and accepted > 0 and picks > 0
    assert mh["accepted"].sum() >= accepted
    assert inf_prior > 0, "the caller's tries reach outside the prior"
    if bool(np.any(~np.isfinite(pt.log_prior(prob.gen, prob.x0(T, W).reshape(-1, D))))):
        assert outside_old > 0, "a start with points outside the generator"
    assert eng.RW == {4: 8, 11: 16, 16: 16, 32: 32, 64: 64, 128: 128, 24: 32, 8: 8}[D]
    eng.close()


# ---- 2. production replay ---------------------------------------------------------------------------------------------------------------
def _check_draws(eng, d, it, T, W, K, prob, what):
    q, up, ua = eng.mt_debug_draws(it)
    X, Xs, E = mt.mt_draws(SEED, it, T, W, K, prob.gen)
    kinds = prob.gen["kind"]
    uni = kinds == pt.UNIFORM
    assert q.shape == (T, W, K, prob.D)
    assert np.array_equal(q[..., uni], X[..., uni]), f"{what}: a uniform draw differs from the specification"
    err = np.abs(q.astype(LD) - Xs).astype(np.float64)
    assert (err <= E)[..., ~uni].all(), f"{what}: a draw misses its bound E by a factor {float((err / np.where(E > 0, E, 1))[..., ~uni].max()):.2f}"
    for k in range(prob.D):                      # inside the support after the clamp
        if kinds[k] != pt.NORMAL:
            assert (q[..., k] >= prob.gen["lo"][k]).all() and (q[..., k] <= prob.gen["hi"][k]).all(), f"{what}: a draw outside its support"
    assert np.array_equal(up, mt.pick_uniforms(SEED, it, T, W)), f"{what}: pick uniforms"
    assert np.array_equal(ua, mt.accept_uniforms(SEED, it, T, W)), f"{what}: accept uniforms"
    # hens_debug_draws keeps its shape: its mh_step is try 0 - the export kernel of DistributionGenerate - its mh_u the accept uniform
    assert np.array_equal(d["mh_step"][..., :prob.D], q[:, :, 0]) and np.array_equal(d["mh_u"], ua), f"{what}: hens_debug_draws"
    return q, up, ua


@pytest.mark.parametrize("name", sorted(mt.CASES))
def test_production_replay(name, monkeypatch):
    c = mt.CASES[name]
    T, W, D, K, weight = c["T"], c["W"], c["D"], c["K"], c["weight"]
    prob = mt.case_problem(c)
    monkeypatch.setattr(orc, "box_log_prior", pt.box_prior_substitute(prob.prior))      # (the stretch iterations' prior)
    eng = _engine(prob, T, W)
    x, L, P, betas = _start(eng, prob, T, W)
    x0 = x.copy()
    eng.set_mt_dist_proposal(prob.gen, K, weight)
    st = ru.OracleState(x, L, P, betas)
    cnt = mt.Counts(T)
    kinds = []
    for n in (1, c["iters"] - 1):
        it0 = eng.iteration()
        eng.step(n)
        eng.synchronize()
        for it in range(it0, it0 + n):
            d = eng.debug_draws(it, mh=True)
            ref = ru.draws_to_reference(d, T, W)
            assert d["is_mh"] == pd.is_mh(SEED, it, weight), f"{name}: the move choice of iteration {it}"
            kinds.append(d["is_mh"])
            if not d["is_mh"]:
                ru.oracle_iteration(st, ref, prob.loglike, prob.lo, prob.hi)
                continue
            what = f"{name}, iteration {it}"
            q, up, ua = _check_draws(eng, d, it, T, W, K, prob, what)
            info = {}
            keep, pick, _, _, _ = mt.mt_step(st.x, st.L, st.P, st.betas, q, up, ua, prob.prior, prob.gen, prob.loglike, info=info)
            ex = mt.exact_mt(info, pick, st.betas, prob.prior, prob.gen)
            _no_knife(info, ex, what)
            st.mh_accepted += keep
            cnt.add(keep, pick, info, ex)
            dm.pt_tail(st, ref)
        xd, Ld, Pd, bd = eng.download()
        what = f"{name} after iteration {it0 + n - 1}"
        assert np.array_equal(xd, st.x), f"{what}: x differs from the specification in {int((xd != st.x).any(axis=-1).sum())} walkers"
        _check_P(Pd, st.P, prob, xd, what)
        tol.check_logl(Ld, st.L, tol.RTOL_L, what)
        if st.betas is not None:
            np.testing.assert_allclose(bd, st.betas, rtol=1e-13, atol=0, err_msg=f"{what}: betas")
        cs, cm = eng.counters(), eng.mh_counters()
        assert np.array_equal(cs["accepted"], st.accepted), f"{what}: stretch accept counters"
        assert np.array_equal(cm["accepted"], st.mh_accepted), f"{what}: the move's accept counters"
        assert cm["num_proposals"] == sum(kinds) and cs["num_proposals"] == len(kinds) - sum(kinds), f"{what}: proposal counts"
        if T > 1:
            assert np.array_equal(cs["swaps_total"], st.swaps_total), f"{what}: swap totals"
        assert st.min_margin > 1e-12, "a stretch decision sat on the knife edge"
    assert any(kinds) and (weight >= 1.0 or not all(kinds))
    assert cnt.accepted.sum() > 0 and cnt.picks_beyond_0 > 0 and cnt.old_outside_accepted == 0
    eng.close()


# ---- 3. the reference's fixtures ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mt.FIXTURES)
def test_reference_fixtures_through_the_parity_entry_points(name):
    """Every move iteration of a fixture through hens_mt_dist_step from the fixture's own state, the sweep through hens_pt_sweep."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    fx = mt.load_fixture(name)
    prior, gen = mt.fixture_specs(fx)
    loglike = mt.fixture_loglike(fx)
    T, W, D, K = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["K"])
    box = bool(np.all(prior["kind"] == pt.UNIFORM))
    eng = HipEnsemble(T, W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), prior["lo"], prior["hi"], a=float(fx["a"]) if "a" in fx else 2.0,
                      prior_terms=None if box else prior, live_dangerously=True, tempered=True)
    assert eng.RW == 8
    eng.set_mt_dist_proposal(gen, K, 0.5)
    x, L, P, betas = fx["x0"], fx["L0"], fx["P0"], fx["betas0"]
    accepted = np.zeros((T, W))
    for it in range(int(fx["nsteps"])):
        rec = mt.fixture_iteration(fx, it)
        what = f"{name}, iteration {it}"
        if rec["is_mt"]:
            eng.upload(x, L, P, betas)
            eng.set_adapt_time(it)
            info = {}
            xs, Ls, Ps = x.copy(), L.copy(), P.copy()
            _, pick_s, _, _, _ = mt.mt_step(xs, Ls, Ps, betas, rec["q"], rec["u_pick"], rec["u_acc"], prior, gen, loglike, info=info)
            ex = mt.exact_mt(info, pick_s, betas, prior, gen)
            _no_knife(info, ex, what)
            out = eng.mt_dist_step(rec["q"], rec["u_pick"], rec["u_acc"], want=("pick", "lsw", "aux_lsw", "factors"))
            assert np.array_equal(out["pick"], rec["pick"]), f"{what}: picks"
            assert np.array_equal(out["keep"], rec["keep"]), f"{what}: accept mask"
            accepted += out["keep"]
            mt.assert_sums(out["lsw"], out["aux_lsw"], out["factors"], ex, what)
            assert np.array_equal(np.isnan(out["aux_lsw"]), np.isnan(rec["aux_lsw"])) and np.array_equal(np.isnan(out["factors"]), np.isnan(rec["factors"]))
            xd, Ld, Pd, _ = eng.download()
            assert np.array_equal(xd, rec["x_move"]), f"{what}: positions after the move"
            r = pt.worst_ratio(Pd.reshape(-1), prior, xd.reshape(-1, D))
            assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"
            assert np.array_equal(Pd == 0.0, rec["P_move"] == 0.0)
            tol.check_logl(Ld, rec["L_move"], tol.RTOL_L, what)
            eng.upload(rec["x_move"], rec["L_move"], rec["P_move"], betas)      # (swaps read L to the last bit)
            eng.set_adapt_time(it)
            sel, swaps = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
            assert np.array_equal(sel, rec["sel"]) and np.array_equal(swaps, rec["swaps_accepted"]), f"{what}: swaps"
            x2, L2, P2, b2 = eng.download()
            assert np.array_equal(x2, rec["x"]) and np.array_equal(L2, rec["L"]) and np.array_equal(P2, rec["P"]), f"{what}: after the sweep"
            np.testing.assert_allclose(b2, rec["betas"], rtol=1e-13, atol=0)
        x, L, P, betas = rec["x"], rec["L"], rec["P"], rec["betas"]
    assert np.array_equal(accepted, fx["accepted_mt"])
    eng.close()


@pytest.mark.parametrize("name", mt.FIXTURES)
def test_numpy_mode_lands_on_the_reference_chain(name):
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves import MTDistGenMove, StretchMove
    from eryn_amd.state import State
    fx = mt.load_fixture(name)
    prior_spec, _ = mt.fixture_specs(fx)
    prior, gen = mt.fixture_containers(fx)
    T, W, D, K, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["K"]), int(fx["nsteps"])
    np.random.seed(int(fx["seed_construct"]))                 # R := snapshot of G at construction
    move = MTDistGenMove(gen, num_try=K, independent=True)
    moves = [(StretchMove(), 0.5), (move, 0.5)] if int(fx["mix"]) else move
    s = EnsembleSampler(W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), prior, moves=moves, tempering_kwargs=dict(ntemps=T))
    np.random.seed(int(fx["seed_run"]))
    for it, st in enumerate(s.sample(fx["x0"], iterations=n, store=False)):
        st = State(st, copy=True)
        what = f"{name}, iteration {it}"
        xs = fx["all_x"][it]
        assert np.array_equal(st.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D), xs), f"{what}: positions"
        r = pt.worst_ratio(np.asarray(st.log_prior).reshape(-1), prior_spec, xs.reshape(-1, D))
        assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"
        tol.check_logl(np.asarray(st.log_like).reshape(T, W), fx["all_L"][it], tol.RTOL_L, what)
        np.testing.assert_allclose(st.betas, fx["all_betas"][it], rtol=1e-13, atol=0, err_msg=what)
        rec = mt.fixture_iteration(fx, it)
        if rec["is_mt"]:                     # the move carries the sums of its last proposal, as the reference's does
            assert move.log_sum_weights.shape == (T * W,) and move.aux_log_sum_weights.shape == (T * W,)
            assert np.array_equal(np.isnan(move.aux_log_sum_weights.reshape(T, W)), np.isnan(rec["aux_lsw"]))
            np.testing.assert_allclose(move.log_sum_weights.reshape(T, W), rec["lsw"], rtol=1e-11, atol=1e-11, equal_nan=True)
    assert np.array_equal(np.asarray(move.accepted).reshape(T, W), fx["accepted_mt"]) and move.num_proposals == int(fx["num_proposals_mt"])
    if int(fx["mix"]):
        assert np.array_equal(s.moves[0].accepted, fx["accepted_stretch"])


# ---- 4. equivalences --------------------------------------------------------------------------------------------------------------------------
def test_one_try_is_the_single_try_move():
    """K = 1 against DistributionGenerate with the same seed under rng="philox": the same positions over 8 iterations (untempered,
    every iteration the move: the chain tests/test_mt_move.py sizes free of knife edges), and a tempered mix at the engine."""
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.moves import DistributionGenerate, MTDistGenMove
    c = dm.CASES["1x64x24_dense_box"]
    prob = dm.case_problem(c)
    prior, gen = prob.containers()
    x0 = prob.x0(1, c["W"])[0]
    chains = []
    for move in (DistributionGenerate({"model_0": gen}), MTDistGenMove(gen, num_try=1, independent=True)):
        s = EnsembleSampler(c["W"], c["D"], pu.device_likelihood(prob), prior, rng="philox", seed=dm.SEED, moves=move)
        s.run_mcmc(x0, 8)
        chains.append((s.get_chain()["model_0"], s.get_log_like(), np.asarray(move.accepted).copy()))
        assert move.num_proposals == 8 and chains[-1][2].sum() > 0
    assert np.array_equal(chains[0][0], chains[1][0]), "positions differ between one try and the single-try move"
    assert np.array_equal(chains[0][2], chains[1][2]), "accept counts differ"
    tol.check_logl(chains[1][1], chains[0][1], tol.RTOL_L, "one try against the single-try move")
    c = dm.CASES["4x72x16_diag_box"]
    prob = dm.case_problem(c)
    out = []
    for k in (0, 1):
        eng = _engine(prob, c["T"], c["W"], seed=dm.SEED)
        _start(eng, prob, c["T"], c["W"])
        if k:
            eng.set_mt_dist_proposal(prob.gen, 1, c["weight"])
        else:
            eng.set_dist_proposal(prob.gen, c["weight"])
        eng.step(8)
        out.append((eng.download()[0], eng.mh_counters()["accepted"], eng.counters()["accepted"]))
        eng.close()
    assert all(np.array_equal(a, b) for a, b in zip(*out)), "the tempered mix: one try against the single-try move"


def _digest(eng, counters=True):
    h = hashlib.sha256()
    for a in eng.download():
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    if counters:
        h.update(np.ascontiguousarray(eng.counters()["accepted"]).tobytes())
        h.update(np.ascontiguousarray(eng.mh_counters()["accepted"]).tobytes())
    return h.hexdigest()


def _run_case(name, split=None):
    c = mt.CASES[name]
    prob = mt.case_problem(c)
    eng = _engine(prob, c["T"], c["W"])
    _start(eng, prob, c["T"], c["W"])
    eng.set_mt_dist_proposal(prob.gen, c["K"], c["weight"])
    if split is None:
        eng.step(c["iters"])
    else:
        eng.step(split)
        eng.set_iteration(eng.iteration())
        eng.step(c["iters"] - split)
    out = _digest(eng)
    eng.close()
    return out


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
from tests.test_hip_mt_move import _run_case
print("DIGEST", _run_case(sys.argv[2]))
"""


def test_walker_records_against_the_by_field_state():
    """HENS_NO_FUSED=1 (read once per process: a fresh one) keeps the state by field round the in-place move; the default path packs
    walker records on this shape.  The chains are the same bit for bit; so is a run split by hens_set_iteration."""
    name = "4x64x16_k3_diag_box"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HENS_NO_FUSED="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, root, name], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    by_field = [ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0].split()[1]
    assert _run_case(name) == by_field
    assert _run_case(name, split=3) == by_field


def _philox_sampler(c, prob, backend, seed=SEED):
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.moves import MTDistGenMove, StretchMove
    prior, gen = prob.containers()
    moves = [(StretchMove(), 1.0 - c["weight"]), (MTDistGenMove(gen, num_try=c["K"], independent=True), c["weight"])]
    return EnsembleSampler(c["W"], c["D"], pu.device_likelihood(prob), prior, rng="philox", seed=seed, moves=moves, backend=backend,
                           tempering_kwargs=dict(ntemps=c["T"], adaptation_lag=50, adaptation_time=5))


def test_device_backend_is_the_host_backend_and_the_chain_is_the_contexts():
    from eryn_amd.backend import Backend, DeviceBackend
    from eryn_amd.engine import HipEnsemble
    from tests.test_hip_chain_store import assert_backends_equal, assert_state_equal, assert_totals_equal
    name = "4x64x16_k3_diag_box"
    c = mt.CASES[name]
    prob = mt.case_problem(c)
    x0 = prob.x0(c["T"], c["W"])
    a, b = _philox_sampler(c, prob, Backend()), _philox_sampler(c, prob, DeviceBackend())
    ra, rb = a.run_mcmc(x0, 6), b.run_mcmc(x0, 6)
    assert_backends_equal(a.backend, b.backend, name)
    assert_totals_equal(a.backend, b.backend, name)
    assert_state_equal(ra, rb, name)
    for ma, mb in zip(a.moves, b.moves):
        assert np.array_equal(ma.accepted, mb.accepted) and ma.num_proposals == mb.num_proposals
    assert all(m.num_proposals > 0 and np.asarray(m.accepted).sum() > 0 for m in a.moves), "both moves of the mix ran and accepted"
    assert a.moves[0].num_proposals + a.moves[1].num_proposals == 6
    # the chain is the context's: the same seed through hens_step with the generator in the MH slot
    eng = HipEnsemble(c["T"], c["W"], c["D"], pu.device_likelihood(prob), prob.lo, prob.hi, seed=SEED, adaptation_lag=50, adaptation_time=5)
    eng.upload(x0, betas=orc.make_ladder(c["D"], ntemps=c["T"]))
    eng.eval_state()
    eng.set_mt_dist_proposal(prob.gen, c["K"], c["weight"])
    eng.step(6)
    xd, Ld, Pd, bd = eng.download()
    assert np.array_equal(xd, ra.branches["model_0"].coords[:, :, 0, :]) and np.array_equal(Ld, ra.log_like) and np.array_equal(bd, ra.betas)
    assert eng.mh_counters()["num_proposals"] == a.moves[1].num_proposals
    eng.close()


def test_a_chain_resumed_from_its_random_state_is_the_unbroken_one():
    from eryn_amd.state import State
    c = mt.CASES["3x40x4_k5_dense_terms"]
    prob = mt.case_problem(c)
    x0 = prob.x0(c["T"], c["W"])
    from eryn_amd.backend import Backend
    whole = [State(st, copy=True) for st in _philox_sampler(c, prob, Backend()).sample(x0, iterations=7, store=True)]
    first = [State(st, copy=True) for st in _philox_sampler(c, prob, Backend()).sample(x0, iterations=3, store=True)]
    assert first[-1].random_state == whole[2].random_state and first[-1].random_state[0] == "philox"
    rest = [State(st, copy=True) for st in _philox_sampler(c, prob, Backend()).sample(first[-1], iterations=4, store=True)]
    for k, (u, v) in enumerate(zip(whole, first + rest)):
        for f in ("log_like", "log_prior", "betas"):
            assert np.array_equal(getattr(u, f), getattr(v, f)), f"{f} differs at stored step {k}"
        assert np.array_equal(u.branches["model_0"].coords, v.branches["model_0"].coords), f"positions differ at stored step {k}"
        assert u.random_state == v.random_state


# ---- 5. refusals and the shared slot ---------------------------------------------------------------------------------------------------------
def test_refusals_and_the_shared_mh_slot():
    from eryn_amd import _lib
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, HostLikelihood
    from eryn_amd.prior import term_arrays
    c = mt.CASES["4x64x16_k3_diag_box"]
    T, W, D, K = 2, 64, 16, 3
    prob = mt.case_problem(c)
    eng = _engine(prob, T, W)
    x0, L0, P0, betas0 = _start(eng, prob, T, W)
    lib = _lib.load()
    q, u = np.repeat(prob.x0(T, W)[:, :, None, :], K, axis=2), np.full((T, W), 0.5)

    def chain(n=4):
        eng.upload(x0, L0, P0, betas0)
        eng.set_iteration(0)
        eng.set_adapt_time(0)
        eng.step(n)
        return _digest(eng, counters=False), eng.mh_counters()["num_proposals"]      # (the MH counters run on across uploads)

    def refused(exc, text, call, before):
        """``call`` raises ``exc`` with ``text`` and leaves the context as it was: the next hens_step steps as before."""
        with pytest.raises(exc) as e:
            call()
        assert text in str(e.value), str(e.value)
        assert chain()[0] == before, f"the context changed under the refusal '{text}'"

    stretch_only = chain()[0]
    refused(RuntimeError, "no generator set (hens_set_mt_dist_proposal)", lambda: eng.mt_dist_step(q, u, u), stretch_only)    # HENS_ERR_STATE
    assert lib.hens_mt_debug_draws(eng.ctx, 0, None, None, None) == _lib.ERR_STATE
    for bad in (0, 65, -3):
        refused(ValueError, "num_try must be in [1, 64]", lambda: eng.set_mt_dist_proposal(prob.gen, bad, 0.5), stretch_only)   # HENS_ERR_INVALID
    for w in (-0.1, 1.5, np.nan):
        refused(ValueError, "weight must be a probability", lambda: eng.set_mt_dist_proposal(prob.gen, K, w), stretch_only)
    arrs = [_lib.ptr(a) for a in term_arrays(prob.gen, eng.RW)]
    for k in range(6):
        args = list(arrs)
        args[k] = None
        assert lib.hens_set_mt_dist_proposal(eng.ctx, *args, K, 0.5) == _lib.ERR_INVALID
    bad = {k: v.copy() for k, v in prob.gen.items()}
    uni = int(np.flatnonzero(prob.gen["kind"] == pt.UNIFORM)[0])
    bad["hi"][uni] = np.inf                                                 # the shared term validation, the parser's texts
    refused(ValueError, f"uniform prior term needs finite bounds (dim {uni})", lambda: eng.set_mt_dist_proposal(bad, K, 0.5), stretch_only)
    # set / replace / switch off: the slot holds what was set last, -1 empties it; two num_try are two moves
    eng.set_mt_dist_proposal(prob.gen, K, 1.0)
    mt3, n = chain()
    assert mt3 != stretch_only and n >= 4
    eng.set_mt_dist_proposal(prob.gen, 7, 1.0)
    mt7 = chain()[0]
    assert mt7 not in (mt3, stretch_only)
    eng.set_dist_proposal(prob.gen, 1.0)                                    # DistributionGenerate replaces it
    dist_only = chain()[0]
    assert dist_only not in (mt3, mt7, stretch_only)
    refused(RuntimeError, "no generator set (hens_set_mt_dist_proposal)", lambda: eng.mt_dist_step(q, u, u), dist_only)
    eng.set_mt_dist_proposal(prob.gen, K, 1.0)                              # ... and is replaced by it
    assert chain()[0] == mt3
    with pytest.raises(RuntimeError) as e:
        eng.dist_step(prob.x0(T, W), u)
    assert "no generator set (hens_set_dist_proposal)" in str(e.value)
    eng.set_mh_proposal("iso", 0.1 * float(prob.sig.min()), 1.0)            # the Gaussian move replaces it
    gauss_only = chain()[0]
    assert gauss_only not in (mt3, dist_only, stretch_only)
    eng.set_mt_dist_proposal(prob.gen, K, 1.0)
    assert chain()[0] == mt3
    # a null argument of the teacher-forced call
    for k in range(3):
        args = [_lib.ptr(np.ascontiguousarray(q)), _lib.ptr(u), _lib.ptr(u)]
        args[k] = None
        assert lib.hens_mt_dist_step(eng.ctx, *args, None, None, None, None) == _lib.ERR_INVALID
    assert chain()[0] == mt3
    # a Gibbs table on the MH slot, both ways round
    masks = np.zeros((2, D), dtype=bool)
    masks[0, :D // 2] = masks[1, D // 2:] = True
    refused(NotImplementedError, "Gibbs blocks are not built for the multiple-try proposal in the MH slot (hens_set_mt_dist_proposal)",
            lambda: eng.set_gibbs("mh", masks), mt3)
    # hens_pipe_init after the move is set
    refused(NotImplementedError, "the multiple-try proposal is not built for a rank of the ladder pipeline", lambda: eng.pipe_init(1, 0), mt3)
    eng.set_mh_proposal(None, None, 0.0)                                    # the one "stretch only" call
    assert chain()[0] == stretch_only
    eng.set_mh_proposal("iso", 0.1 * float(prob.sig.min()), 1.0)
    eng.set_gibbs("mh", masks)
    gibbs_chain = chain()[0]
    refused(NotImplementedError, "the multiple-try proposal is not built under Gibbs blocks on the MH slot", lambda: eng.set_mt_dist_proposal(prob.gen, K, 0.5),
            gibbs_chain)
    eng.close()
    # a rank of the ladder pipeline
    rank = _engine(prob, T, W)
    rank.pipe_init(1, 0)
    with pytest.raises(RuntimeError) as e:                                  # HENS_ERR_STATE
        rank.set_mt_dist_proposal(prob.gen, K, 0.5)
    assert "the multiple-try proposal is not built for a rank of the ladder pipeline" in str(e.value)
    rank.close()
    # a leaf-packing context
    from eryn_amd.rj import _TemplateLikelihood
    rj = HipEnsemble(2, 16, 8, _TemplateLikelihood(8), -1.0, 1.0, tempered=True, live_dangerously=True)
    with pytest.raises(NotImplementedError) as e:
        rj.set_mt_dist_proposal(dm.box_spec(np.full(8, -1.0), np.full(8, 1.0)), K, 0.5)
    assert "the multiple-try proposal is not built for leaf-packing records" in str(e.value)
    rj.close()
    # a host-callable likelihood
    host = HipEnsemble(T, W, D, HostLikelihood(prob.loglike, D), prob.lo, prob.hi, live_dangerously=True)
    with pytest.raises(NotImplementedError) as e:
        host.set_mt_dist_proposal(prob.gen, K, 0.5)
    assert "the multiple-try proposal needs a device likelihood" in str(e.value)
    host.close()
    # row widths the host cannot bring to 8 ... 128: a generic width (rows not padded), D > 128
    for Dg, kw in ((5, dict(pad_rows=False)), (130, {})):
        mu, invcov = pu.gaussian_problem(Dg, dense=False)
        gen = HipEnsemble(2, 2 * Dg + 2, Dg, GaussianLikelihood(mu, np.diag(invcov).copy()), -50.0, 50.0, **kw)
        with pytest.raises(NotImplementedError) as e:
            gen.set_mt_dist_proposal(dm.box_spec(np.full(Dg, -50.0), np.full(Dg, 50.0)), K, 0.5)
        assert f"the multiple-try proposal is built for row widths 8, 16, 32, 64 and 128 (this context's rows are {Dg} wide)" in str(e.value)
        gen.close()
