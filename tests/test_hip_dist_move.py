"""The draw-from-distribution move on the device (hens_set_dist_proposal, hens_dist_step, the k_dist launch of hens_step;
csrc/hens_dist.h) against its specification (tests/dist_move.py).

  1. teacher-forced: hens_dist_step with the caller's points - the specification's draws with rows outside the generator mixed
     in - masks and positions bit for bit, factors_out bit for bit without a log-uniform coordinate and within 1.0 B_F with one,
     the log-prior within 1.0 B_P (-inf exactly where the specification has it), log-likelihood at the project's bar;
  2. production replay: hens_step steps the cases of tests/dist_move.CASES, hens_debug_draws exports every iteration's draws, the
     specification replays them (stretch iterations through the pinned oracle, tests/replay_utils.py); the exported draws against
     dist_draws, the unit normals' statistics, the move choice, the counters; coverage counted from the specification's side;
  3. equivalence: HENS_NO_FUSED=1 in a fresh process, a run split by hens_set_iteration;
  4. refusals, and the shared MH slot set / replaced / switched off in both orders.
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import dist_move as dm
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import replay_utils as ru
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
LD = np.longdouble
SEED = dm.SEED


def _engine(prob, T, W, seed=SEED, **kw):
    from eryn_amd.engine import HipEnsemble
    terms = None if np.all(prob.prior["kind"] == pt.UNIFORM) else prob.prior
    return HipEnsemble(T, W, prob.D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=seed, prior_terms=terms, live_dangerously=True, **kw)


def _is_box(prob):
    return bool(np.all(prob.prior["kind"] == pt.UNIFORM))


def _check_P(P, Pspec, prob, x, what):
    """Log-prior: under a box the constant, bit for bit; under terms within 1.0 B_P of exact arithmetic at the positions."""
    if _is_box(prob):
        assert np.array_equal(P, Pspec), f"{what}: log-prior differs"
        return
    D = prob.D
    r = pt.worst_ratio(P.reshape(-1), prob.prior, x.reshape(-1, D))
    print(f"{what}: |P - P*| / B_P <= {r:.3f}")
    assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"


def _start(eng, prob, T, W):
    betas0 = orc.make_ladder(prob.D, ntemps=T) if T > 1 else None
    eng.upload(prob.x0(T, W), betas=betas0)
    eng.eval_state()
    x, L, P, betas = eng.download()
    assert np.isfinite(P).all(), "a start outside the prior's support"
    return x, L, P, betas


# ---- 1. teacher-forced ----------------------------------------------------------------------------------------------------------------
FORCED = ["3x40x4_dense_terms", "3x33x11_diag_box_genbox", "2x136x32_dense_box", "2x65x128_rosen_box"]


@pytest.mark.parametrize("name", FORCED)
def test_dist_step_with_the_callers_points(name):
    c = dm.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = dm.case_problem(c)
    eng = _engine(prob, T, W)
    x, L, P, betas = _start(eng, prob, T, W)
    eng.set_dist_proposal(prob.gen, 0.5)
    rs = np.random.RandomState(31)
    inf_prior = outside_old = outside_new = accepted = 0
    for it in range(3):
        q, _, _ = dm.dist_draws(SEED, it, T, W, prob.gen)
        # a caller's points may lie anywhere: every seventh row gets one coordinate moved out of the generator's support (where
        # it has one) or far out of the prior's
        for t in range(T):
            for w in range(it, W, 7):
                d = int(rs.randint(D))
                lo, hi = prob.gen["lo"][d], prob.gen["hi"][d]
                q[t, w, d] = hi + 0.25 * (hi - lo) if np.isfinite(hi) else prob.centre[d] + 50.0 * prob.half[d]
        u = rs.rand(T, W)
        xs, Ls, Ps = x.copy(), L.copy(), P.copy()
        info = {}
        _, _, _, keep_s, fac_s = dm.dist_step(xs, Ls, Ps, betas, q, u, prob.prior, prob.gen, prob.loglike, info=info)
        with np.errstate(divide="ignore"):
            assert not pu.knife_edge(info["lnpdiff"], np.log(u)).any(), "a decision on the knife edge: pick another seed"
        keep, fac = eng.dist_step(q, u, want_factors=True)
        what = f"{name}, proposal {it}"
        assert np.array_equal(keep, keep_s), f"{what}: accept mask differs in {int((keep != keep_s).sum())} walkers"
        dm.assert_factors(fac, prob.gen, x, q, what)
        xd, Ld, Pd, _ = eng.download()
        assert np.array_equal(xd, xs), f"{what}: positions differ"
        _check_P(Pd, Ps, prob, xd, what)
        tol.check_logl(Ld, Ls, tol.RTOL_L, what)
        inf_prior += int(np.isinf(info["logp"]).sum())
        outside_old += int(np.isneginf(fac_s).sum())
        outside_new += int((np.isposinf(fac_s) | np.isnan(fac_s)).sum())
        accepted += int(keep.sum())
        assert not (keep & np.isneginf(fac_s)).any(), "an old point outside the generator was moved"
        x, L, P = xd, Ld, Pd
    mh = eng.mh_counters()
    assert mh["num_proposals"] == 3 and mh["accepted"].sum() == accepted and accepted > 0
    assert inf_prior > 0 and (outside_new > 0 or name == "2x136x32_dense_box")
    if c["gen"] != "box" and name != "2x136x32_dense_box":
        assert outside_old > 0
    # the pads of a padded row never moved
    assert eng.RW == {4: 8, 11: 16, 32: 32, 128: 128}[D]
    eng.close()


# ---- 2. production replay ---------------------------------------------------------------------------------------------------------------
def _check_draws(d, it, T, W, prob, what):
    X, Xs, E = dm.dist_draws(SEED, it, T, W, prob.gen)
    q = d["mh_step"]
    kinds = prob.gen["kind"]
    uni = kinds == pt.UNIFORM
    assert np.array_equal(q[..., uni], X[..., uni]), f"{what}: a uniform draw differs from the specification"
    err = np.abs(q.astype(LD) - Xs).astype(np.float64)
    assert (err <= E)[..., ~uni].all(), f"{what}: a draw misses its bound E by a factor {float((err / np.where(E > 0, E, 1))[..., ~uni].max()):.2f}"
    for k in range(prob.D):                      # inside the support after the clamp
        if kinds[k] != pt.NORMAL:
            assert (q[..., k] >= prob.gen["lo"][k]).all() and (q[..., k] <= prob.gen["hi"][k]).all(), f"{what}: a draw outside its support"
    assert np.array_equal(d["mh_u"], dm.accept_uniforms(SEED, it, T, W)), f"{what}: accept uniforms"


@pytest.mark.parametrize("name", sorted(dm.CASES))
def test_production_replay(name, monkeypatch):
    c = dm.CASES[name]
    T, W, D, weight = c["T"], c["W"], c["D"], c["weight"]
    prob = dm.case_problem(c)
    monkeypatch.setattr(orc, "box_log_prior", pt.box_prior_substitute(prob.prior))      # (the stretch iterations' prior)
    eng = _engine(prob, T, W)
    x, L, P, betas = _start(eng, prob, T, W)
    x0 = x.copy()
    eng.set_dist_proposal(prob.gen, weight)
    st = ru.OracleState(x, L, P, betas)
    cnt = dm.Counts(T)
    kinds, normals = [], []
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
            _check_draws(d, it, T, W, prob, f"{name}, iteration {it}")
            normals.append(dm.unit_normals(SEED, it, T, W, prob.gen))
            info = {}
            _, _, _, keep, fac = dm.dist_step(st.x, st.L, st.P, st.betas, d["mh_step"], d["mh_u"], prob.prior, prob.gen, prob.loglike, info=info)
            st.mh_accepted += keep
            cnt.add(keep, fac, info)
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
    dm.assert_coverage(cnt, prob, x0, spare=1, what=name)
    nn = normals[0].shape[-1] & ~1
    if len(normals) >= 2 and nn >= 4:            # the unit normals behind the normal terms, [iterations, rungs, W, coordinates]
        bad = pd.normal_stream_violations(pd.normal_stream_stats(np.stack(normals)[..., :nn], 0))
        assert not bad, f"{name}: {bad}"
    # the launch path of a profiled call: one k_dist launch (kind 0) per move iteration, two stretch launches otherwise
    eng.set_profiling(True)
    it0 = eng.iteration()
    eng.step(2)
    tm = eng.timing()
    nm = sum(pd.is_mh(SEED, it, weight) for it in (it0, it0 + 1))
    print(f"{name}: profiled launches {tm['n_stretch']} stretch / MH, {tm['n_pt']} cascade, {tm['n_fused']} fused over {nm} move iterations of 2")
    assert tm["n_stretch"] + tm["n_fused"] + tm["n_pt"] >= 2
    if weight >= 1.0:
        assert (tm["n_stretch"], tm["n_pt"], tm["n_fused"]) == (2, 0, 0), tm
    elif name in dm.RECORDS:                     # record mode: the move's launch + a cascade; a stretch iteration is one launch (k_iter)
        assert pd.label_cb(T, W) > 0             # or two (the in-place half-step, then the fused second half-step + cascade)
        assert tm["n_pt"] == nm and tm["n_fused"] == 2 - nm and tm["n_stretch"] in (nm, 2), tm
    else:                                        # by-field state: two copying half-steps or the move's launch, a cascade each
        assert (tm["n_stretch"], tm["n_pt"], tm["n_fused"]) == (2 * (2 - nm) + nm, 2, 0), tm
    eng.close()


# ---- 3. equivalence ------------------------------------------------------------------------------------------------------------------------
def _digest(eng, counters=True):
    h = hashlib.sha256()
    for a in eng.download():
        if a is not None:
            h.update(np.ascontiguousarray(a).tobytes())
    if not counters:
        return h.hexdigest()
    h.update(np.ascontiguousarray(eng.counters()["accepted"]).tobytes())
    h.update(np.ascontiguousarray(eng.mh_counters()["accepted"]).tobytes())
    return h.hexdigest()


def _run_case(name, split=None):
    c = dm.CASES[name]
    prob = dm.case_problem(c)
    eng = _engine(prob, c["T"], c["W"])
    _start(eng, prob, c["T"], c["W"])
    eng.set_dist_proposal(prob.gen, c["weight"])
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
from tests.test_hip_dist_move import _run_case
print("DIGEST", _run_case(sys.argv[2]))
"""


@pytest.mark.parametrize("name", ["4x72x16_diag_box", "2x136x32_dense_box"] + dm.RECORDS)
def test_copying_launches_step_the_same_chain(name):
    """HENS_NO_FUSED=1 (read once per process: a fresh one) - the by-field state and the copying launches round the in-place move -
    lands on the default path's chain bit for bit."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = []
    for extra in ({}, {"HENS_NO_FUSED": "1"}):
        env = dict(os.environ, **extra)
        r = subprocess.run([sys.executable, "-c", _CHILD, root, name], env=env, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stdout + r.stderr
        out.append([ln for ln in r.stdout.splitlines() if ln.startswith("DIGEST")][0])
    assert out[0] == out[1]


def test_a_run_split_by_set_iteration_is_the_uninterrupted_one():
    for name in ("4x72x16_diag_box", "4x64x16_diag_box_records"):
        assert _run_case(name) == _run_case(name, split=3)


# ---- 4. refusals and the shared slot ---------------------------------------------------------------------------------------------------------
def test_refusals_and_the_shared_mh_slot():
    from eryn_amd import _lib
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, HostLikelihood
    c = dm.CASES["4x72x16_diag_box"]
    T, W, D = 2, 64, 16
    prob = dm.case_problem(c)
    eng = _engine(prob, T, W)
    x0, L0, P0, betas0 = _start(eng, prob, T, W)
    lib = _lib.load()
    q, u = prob.x0(T, W), np.full((T, W), 0.5)
    with pytest.raises(RuntimeError) as e:                                  # HENS_ERR_STATE: no generator set
        eng.dist_step(q, u)
    assert "no generator set (hens_set_dist_proposal)" in str(e.value)
    for w in (-0.1, 1.5, np.nan):
        with pytest.raises(ValueError) as e:
            eng.set_dist_proposal(prob.gen, w)
        assert "weight must be a probability" in str(e.value)
    from eryn_amd.prior import term_arrays
    arrs = [_lib.ptr(a) for a in term_arrays(prob.gen, eng.RW)]
    for k in range(6):
        args = list(arrs)
        args[k] = None
        assert lib.hens_set_dist_proposal(eng.ctx, *args, 0.5) == _lib.ERR_INVALID
    # a distribution one draws from needs a finite uniform support; the parser's texts
    bad = {k: v.copy() for k, v in prob.gen.items()}
    uni = int(np.flatnonzero(prob.gen["kind"] == pt.UNIFORM)[0])
    bad["hi"][uni] = np.inf
    with pytest.raises(ValueError) as e:
        eng.set_dist_proposal(bad, 0.5)
    assert f"uniform prior term needs finite bounds (dim {uni})" in str(e.value)
    with pytest.raises(RuntimeError):                                       # (still no generator)
        eng.dist_step(q, u)

    def chain(n=4):
        eng.upload(x0, L0, P0, betas0)
        eng.set_iteration(0)
        eng.set_adapt_time(0)
        eng.step(n)
        return _digest(eng, counters=False), eng.mh_counters()["num_proposals"]      # (the MH counters run on across uploads)

    # set / replace / switch off, both orders: the slot holds what was set last, -1 empties it
    stretch_only = chain()[0]
    eng.set_dist_proposal(prob.gen, 1.0)
    dist_only, n = chain()
    assert dist_only != stretch_only and n >= 4
    eng.set_mh_proposal("iso", 0.1 * float(prob.sig.min()), 1.0)           # replaces the generator
    gauss_only = chain()[0]
    assert gauss_only not in (dist_only, stretch_only)
    with pytest.raises(RuntimeError):
        eng.dist_step(q, u)
    eng.set_dist_proposal(prob.gen, 1.0)                                    # ... and the generator replaces it
    assert chain()[0] == dist_only
    eng.set_mh_proposal(None, None, 0.0)                                    # the one "stretch only" call
    assert chain()[0] == stretch_only
    eng.set_mh_proposal("iso", 0.1 * float(prob.sig.min()), 1.0)
    assert chain()[0] == gauss_only
    eng.set_mh_proposal(None, None, 0.0)
    assert chain()[0] == stretch_only
    # hens_pipe_init after the move is set
    eng.set_dist_proposal(prob.gen, 0.5)
    with pytest.raises(NotImplementedError) as e:
        eng.pipe_init(1, 0)
    assert "the distribution proposal is not built for a rank of the ladder pipeline" in str(e.value)
    eng.close()
    # a rank of the ladder pipeline
    rank = _engine(prob, T, W)
    rank.pipe_init(1, 0)
    with pytest.raises(RuntimeError) as e:
        rank.set_dist_proposal(prob.gen, 0.5)
    assert "not built for a rank of the ladder pipeline" in str(e.value)
    rank.close()
    # a leaf-packing context
    from eryn_amd.rj import _TemplateLikelihood
    rj = HipEnsemble(2, 16, 8, _TemplateLikelihood(8), -1.0, 1.0, tempered=True, live_dangerously=True)
    with pytest.raises(NotImplementedError) as e:
        rj.set_dist_proposal(dm.box_spec(np.full(8, -1.0), np.full(8, 1.0)), 0.5)
    assert "leaf-packing" in str(e.value)
    rj.close()
    # a host-callable likelihood
    host = HipEnsemble(T, W, D, HostLikelihood(prob.loglike, D), prob.lo, prob.hi, live_dangerously=True)
    with pytest.raises(NotImplementedError) as e:
        host.set_dist_proposal(prob.gen, 0.5)
    assert "needs a device likelihood" in str(e.value)
    host.close()
    # row widths the host cannot bring to 8 ... 128: a generic width (rows not padded), D > 128
    for Dg, kw in ((5, dict(pad_rows=False)), (130, {})):
        mu, invcov = pu.gaussian_problem(Dg, dense=False)
        gen = HipEnsemble(2, 2 * Dg + 2, Dg, GaussianLikelihood(mu, np.diag(invcov).copy()), -50.0, 50.0, **kw)
        with pytest.raises(NotImplementedError) as e:
            gen.set_dist_proposal(dm.box_spec(np.full(Dg, -50.0), np.full(Dg, 50.0)), 0.5)
        assert f"this context's rows are {Dg} wide" in str(e.value)
        gen.close()


# ---- 5. the reference's fixtures, teacher-forced ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", dm.FIXTURES)
def test_reference_fixtures_through_the_parity_entry_points(name):
    """Every iteration of a fixture from the fixture's own state: a move iteration through hens_dist_step, a stretch iteration
    through hens_stretch_split, the sweep through hens_pt_sweep."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    fx = dm.load_fixture(name)
    prior, gen = dm.fixture_specs(fx)
    T, W, D = int(fx["T"]), int(fx["W"]), int(fx["D"])
    box = bool(np.all(prior["kind"] == pt.UNIFORM))
    eng = HipEnsemble(T, W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), prior["lo"], prior["hi"], a=float(fx["a"]) if "a" in fx else 2.0,
                      prior_terms=None if box else prior, live_dangerously=True, tempered=T > 1)
    assert eng.RW == 8
    eng.set_dist_proposal(gen, 0.5)
    x, L, P = fx["x0"], fx["L0"], fx["P0"]
    betas = fx["betas0"] if T > 1 else None
    accepted = np.zeros((T, W))

    def check_P(Pd, xd, what):
        r = pt.worst_ratio(Pd.reshape(-1), prior, xd.reshape(-1, D))
        assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"

    for it in range(int(fx["nsteps"])):
        rec = dm.fixture_iteration(fx, it)
        what = f"{name}, iteration {it}"
        eng.upload(x, L, P, betas)
        if T > 1:
            eng.set_adapt_time(it)
        if rec["is_dist"]:
            keep, fac = eng.dist_step(rec["q"], rec["u_acc"], want_factors=True)
            assert np.array_equal(keep, rec["keep"]), f"{what}: accept mask"
            accepted += keep
            dm.assert_factors(fac, gen, x, rec["q"], what)
            if not dm.has_log_uniform(gen):
                assert np.array_equal(fac, rec["factors"]), f"{what}: factors differ from the reference's"
        else:
            for sp in range(2):
                keep = eng.stretch_split(sp, rec["labels"], rec[f"rint{sp}"], rec[f"u_zz{sp}"], rec[f"u_acc{sp}"])
                assert np.array_equal(keep, rec[f"keep{sp}"]), f"{what}: stretch accept mask {sp}"
        xd, Ld, Pd, _ = eng.download()
        assert np.array_equal(xd, rec["x_move"]), f"{what}: positions after the move"
        check_P(Pd, xd, what)
        assert np.array_equal(Pd == 0.0, rec["P_move"] == 0.0)
        tol.check_logl(Ld, rec["L_move"], tol.RTOL_L, what)
        if T > 1:
            eng.upload(rec["x_move"], rec["L_move"], rec["P_move"], betas)      # (swaps read L to the last bit)
            eng.set_adapt_time(it)
            sel, swaps = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
            assert np.array_equal(sel, rec["sel"]) and np.array_equal(swaps, rec["swaps_accepted"]), f"{what}: swaps"
            x2, L2, P2, b2 = eng.download()
            assert np.array_equal(x2, rec["x"]) and np.array_equal(L2, rec["L"]) and np.array_equal(P2, rec["P"]), f"{what}: after the sweep"
            np.testing.assert_allclose(b2, rec["betas"], rtol=1e-13, atol=0)
            betas = rec["betas"]
        x, L, P = rec["x"], rec["L"], rec["P"]
    assert np.array_equal(accepted, fx["accepted_dist"])
    eng.close()
