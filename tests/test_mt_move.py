"""CPU tests of the multiple-try independence move: the specification (tests/mt_move.py) against the fixtures captured from the real
reference (tests/golden/mt/), against tests/dist_move.py at one try, its bounds against long double, the production draws'
statement, the class's argument errors, and the sizing of every GPU case of tests/test_hip_mt_move.py on the specification alone."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import dist_move as dm
from tests import mt_move as mt
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests.test_prior_terms import GOLDEN, HERE, needs_reference

LD = np.longdouble


def _same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), f"{what} differs from the fixture"


# ---- the specification against the reference's fixtures ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", mt.FIXTURES)
def test_specification_reproduces_the_reference_fixtures(name, monkeypatch):
    """Every move iteration through ``mt_step`` - picks, keeps and positions bit for bit; lsw, aux_lsw and factors equal to the
    reference's, NaN where it has NaN - every stretch iteration through the pinned oracle, the sweep and the adaptation likewise."""
    fx = mt.load_fixture(name)
    prior, gen = mt.fixture_specs(fx)
    loglike = mt.fixture_loglike(fx)
    T, W, D, K = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["K"])
    x, L, P, betas = fx["x0"].copy(), fx["L0"].copy(), fx["P0"].copy(), fx["betas0"].copy()
    monkeypatch.setattr(orc, "box_log_prior", pt.box_prior_substitute(prior))
    accepted = np.zeros((T, W))
    moves = nan_aux = picks = inf_prior = knives = 0
    for it in range(int(fx["nsteps"])):
        rec = mt.fixture_iteration(fx, it)
        what = f"{name}, iteration {it}"
        if rec["is_mt"]:
            info = {}
            keep, pick, lsw, aux, fac = mt.mt_step(x, L, P, betas, rec["q"], rec["u_pick"], rec["u_acc"], prior, gen, loglike, info=info)
            _same(pick, rec["pick"], what + ": pick")
            _same(lsw, rec["lsw"], what + ": lsw")
            _same(aux, rec["aux_lsw"], what + ": aux_lsw")
            _same(fac, rec["factors"], what + ": factors")
            _same(keep, rec["keep"], what + ": accept mask")
            _same(info["logl"][keep], rec["mt_ll"][keep], what + ": mt_ll of the moved walkers")
            _same(info["logp"], rec["mt_lp"], what + ": mt_lp")
            ex = mt.exact_mt(info, pick, betas, prior, gen)
            mt.assert_sums(lsw, aux, fac, ex, what)                       # the float64 specification sits within B of exact arithmetic
            assert not mt.pick_knife(ex["c"], rec["u_pick"], ex["B_c"]).any(), what + ": a pick on the knife edge"
            with np.errstate(divide="ignore"):
                knives += int(pu.knife_edge(info["lnpdiff"], np.log(rec["u_acc"])).sum())
            out = np.isneginf(info["alq"]).reshape(T, W)
            assert np.array_equal(np.isnan(aux), out), what + ": aux_lsw is NaN exactly for the old points outside the generator"
            assert not (out & keep).any(), what + ": an old point outside the generator was moved"
            accepted += keep
            moves += 1
            nan_aux += int(out.sum())
            picks += int((pick != 0).sum())
            inf_prior += int(np.isinf(info["lp"]).sum())
        else:
            for sp in range(2):
                out = orc.stretch_split(x, L, P, betas, rec["labels"], sp, rec[f"rint{sp}"], rec[f"u_zz{sp}"], rec[f"u_acc{sp}"], float(fx["a"]),
                                        prior["lo"], prior["hi"], loglike)
                _same(out["keep"], rec[f"keep{sp}"], what + f": stretch accept mask {sp}")
        _same(x, rec["x_move"], what + ": x after the move")
        _same(P, rec["P_move"], what + ": log-prior after the move")
        _same(L, rec["L_move"], what + ": log-likelihood after the move")
        sel, sw = orc.pt_sweep(x, L, P, betas, rec["iperm"], rec["i1perm"], rec["u_swap"])
        _same(sel, rec["sel"], what + ": swap mask")
        _same(sw, rec["swaps_accepted"], what + ": swap counts")
        betas = orc.adapt_ladder(betas, sw, W, it)
        _same(betas, rec["betas"], what + ": ladder")
        _same(x, rec["x"], what + ": x")
        _same(L, rec["L"], what + ": L")
        _same(P, rec["P"], what + ": P")
    assert moves == int(fx["kind"].sum()) == int(fx["num_proposals_mt"])
    _same(accepted, fx["accepted_mt"], "the move's accept counts")
    assert (accepted.sum(axis=1) > 0).all() and picks > 0 and knives == 0
    if name == "mt1_mix":
        assert nan_aux >= 1 and inf_prior >= 1 and (fx["kind"] == 0).any()
    else:
        assert nan_aux == 0 and inf_prior == 0 and K == 25


@pytest.mark.parametrize("name", mt.FIXTURES)
def test_eryn_amd_containers_draw_the_fixtures_tries(name):
    """eryn_amd.prior containers built with the reference's calls give the fixture's tries and pick uniforms from the same global
    seed: ONE rvs(size=(T W, K)), then ONE rand(T W), between a stretch iteration's label shuffles and the sweep's draws."""
    fx = mt.load_fixture(name)
    T, W, D, K = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["K"])
    _, gen = mt.fixture_containers(fx)
    np.random.seed(int(fx["seed_run"]))
    for it in range(int(fx["nsteps"])):
        rec = mt.fixture_iteration(fx, it)
        if rec["is_mt"]:
            _same(np.asarray(gen.rvs(size=(T * W, K))).reshape(T, W, K, D), rec["q"], f"iteration {it}: tries")
            _same(np.random.rand(T * W).reshape(T, W), rec["u_pick"], f"iteration {it}: pick uniforms")
        else:
            for t in range(T):
                lab = np.arange(W) % 2
                np.random.shuffle(lab)
                _same(lab, rec["labels"][t], f"iteration {it}: labels")
        for j in range(T - 1):
            _same(np.random.permutation(W), rec["iperm"][j], "iperm")
            _same(np.random.permutation(W), rec["i1perm"][j], "i1perm")
            _same(np.random.uniform(size=W), rec["u_swap"][j], "u_swap")


@needs_reference
def test_generator_reproduces_the_committed_fixtures(tmp_path):
    """build container only: copies of the generators run against the real reference give the committed files, key for key"""
    for g in ("make_golden.py", "make_golden_priors.py", "make_golden_dist.py", "make_golden_mt.py"):
        shutil.copy(os.path.join(GOLDEN, g), tmp_path / g)
    shutil.copy(os.path.join(HERE, "ladders.py"), tmp_path / "ladders.py")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_mt.py")], cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", GOLDEN_OUT=str(out)))
    assert r.returncode == 0, r.stdout + r.stderr
    total = 0
    for name in mt.FIXTURES + mt.PERIODIC_FIXTURES:
        new, old = np.load(out / (name + ".npz"), allow_pickle=False), mt.load_fixture(name)
        assert sorted(new.files) == sorted(old) and len(old) > 40
        for k in old:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=True), k
        size = os.path.getsize(os.path.join(mt.FIXTURE_DIR, name + ".npz"))
        if name in mt.FIXTURES:
            total += size
        else:
            assert size < 150_000
    assert total < 500_000


# ---- one try is DistributionGenerate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x40x4_dense_terms", "4x72x16_diag_box", "1x64x24_dense_box"])
def test_one_try_gives_the_keeps_of_the_single_try_move(name):
    """K = 1: lsw = w_0, aux_lsw = w'_0, the factor is logq(old) - logq(new) but for roundings, the pick is try 0 - the keeps are
    tests/dist_move.dist_step's on its own cases and draws, apart from knife edges (none for these seeds)."""
    c = dm.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = dm.case_problem(c)
    x, L, P, betas = mt.start_of(prob, T, W)
    moves = 0
    for it in range(c["iters"]):
        q, _, _ = dm.dist_draws(dm.SEED, it, T, W, prob.gen)
        q1, _, _ = mt.mt_draws(dm.SEED, it, T, W, 1, prob.gen)
        assert np.array_equal(q1[:, :, 0], q), "try 0 is the point of the single-try move"
        u = dm.accept_uniforms(dm.SEED, it, T, W)
        xd, Ld, Pd = x.copy(), L.copy(), P.copy()
        info_d, info = {}, {}
        _, _, _, keep_d, fac_d = dm.dist_step(xd, Ld, Pd, betas, q, u, prob.prior, prob.gen, prob.loglike, info=info_d)
        keep, pick, lsw, aux, fac = mt.mt_step(x, L, P, betas, q1, mt.pick_uniforms(dm.SEED, it, T, W), u, prob.prior, prob.gen, prob.loglike, info=info)
        with np.errstate(divide="ignore"):
            assert not pu.knife_edge(info_d["lnpdiff"], np.log(u)).any() and not pu.knife_edge(info["lnpdiff"], np.log(u)).any()
        assert (pick == 0).all()
        assert np.array_equal(keep, keep_d), f"{name}, iteration {it}: keeps differ"
        fin = np.isfinite(fac_d) & np.isfinite(fac)
        # where the single try's weight is -inf (a -inf prior) the multiple-try factor is NaN and the walker stays, as there
        assert not keep[~fin].any() and not keep_d[~fin].any()
        np.testing.assert_allclose(fac[fin], fac_d[fin], rtol=0, atol=1e-9)
        assert np.array_equal(x, xd) and np.array_equal(L, Ld) and np.array_equal(P, Pd)
        moves += int(keep.sum())
    assert moves > 0


# ---- the bounds -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["3x40x4_k5_dense_terms", "2x128x32_k25_dense_box", "2x9x64_k64_dense_terms", "1x20x24_k7_dense_box"])
def test_float64_specification_sits_within_the_bounds_of_exact_arithmetic(name):
    c = mt.CASES[name]
    prob = mt.case_problem(c)
    T, W = c["T"], c["W"]
    x, L, P, betas = mt.start_of(prob, T, W)
    worst = np.zeros(3)
    for n in range(mt.FORCED_PROPOSALS):
        q, up, ua = mt.forced_inputs(c, prob, n)
        info = {}
        keep, pick, lsw, aux, fac = mt.mt_step(x, L, P, betas, q, up, ua, prob.prior, prob.gen, prob.loglike, info=info)
        ex = mt.exact_mt(info, pick, betas, prob.prior, prob.gen)
        worst = np.maximum(worst, mt.assert_sums(lsw, aux, fac, ex, f"{name}, proposal {n}"))
        # another summation order stays inside as well: the terms of the sum reversed
        rev = mt.logsumexp(info["w"][:, ::-1]).reshape(T, W)
        mt.assert_sums(rev, aux, fac, ex, f"{name}, proposal {n}, reversed sum")
        # the exact pick is the float64 one away from knife edges
        with np.errstate(invalid="ignore"):
            pick_exact = (ex["c"] > up[..., None]).argmax(-1)
        knife = mt.pick_knife(ex["c"], up, ex["B_c"])
        assert np.array_equal(pick_exact[~knife], pick[~knife])
    assert worst.max() > 0.0, "the bound was never exercised"
    assert worst.max() <= 1.0


def test_logsumexp_statement():
    """multipletry.py:25-33 on hand-made rows: all -inf -> NaN, one +inf -> NaN, a NaN entry -> NaN, one finite entry -> itself."""
    a = np.array([[-np.inf, -np.inf, -np.inf], [0.0, np.inf, 1.0], [0.0, np.nan, 1.0], [-np.inf, -3.5, -np.inf], [1.0, 1.0, 1.0]])
    out = mt.logsumexp(a)
    assert np.isnan(out[:3]).all() and out[3] == -3.5 and out[4] == 1.0 + np.log(3.0)
    assert not mt.pick_knife(np.array([[0.2, 0.7, 1.0]]), np.array([0.5]), np.full((1, 3), 1e-15)).any()
    assert mt.pick_knife(np.array([[0.2, 0.5 + 1e-16, 1.0]]), np.array([0.5]), np.full((1, 3), 1e-15)).all()


# ---- the production draws ---------------------------------------------------------------------------------------------------------------------
def test_mt_draws_statement():
    gen = pt.make_spec([("uniform", -1.5, 2.0), ("log_uniform", 0.05, 2.45), ("normal", -0.3, 0.6)])
    T, W, K = 2, 30, 7
    X, Xs, E = mt.mt_draws(7, 5, T, W, K, gen)
    X0, _, _ = dm.dist_draws(7, 5, T, W, gen)
    assert np.array_equal(X[:, :, 0], X0), "try 0 is DistributionGenerate's point"
    assert len({X[0, 0, k, 0] for k in range(K)}) == K, "every try its own words"
    assert (np.abs(X.astype(LD) - Xs).astype(np.float64) <= np.where(E > 0, E, np.inf))[..., 1:].all()
    assert np.isfinite(pt.log_prior(gen, X.reshape(-1, 3))).all(), "every draw has a finite log q"
    up, ua = mt.pick_uniforms(7, 5, T, W), mt.accept_uniforms(7, 5, T, W)
    assert up.shape == (T, W) and ((up >= 0) & (up < 1)).all() and not np.array_equal(up, ua)
    assert np.array_equal(mt.pick_uniforms(7, 5, T, W, rung_begin=1)[0], up[1])
    assert not np.array_equal(mt.pick_uniforms(7, 6, T, W), up)


# ---- the class -------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_class():
    from eryn_amd.moves import MHMove, MTDistGenMove
    from eryn_amd.moves.device import DeviceMove, mh_slot_key
    from eryn_amd.prior import ProbDistContainer, uniform_dist
    c = ProbDistContainer({0: uniform_dist(0.0, 1.0), 1: uniform_dist(-1.0, 1.0)})
    with pytest.raises(NotImplementedError) as e:                           # the reference's default
        MTDistGenMove(c, num_try=3)
    assert "independent=True" in str(e.value) and "UnboundLocalError" in str(e.value)
    for kw in (dict(symmetric=True), dict(rj=True), dict(gibbs_sampling_setup=[("model_0", np.array([True, False]))])):
        with pytest.raises(NotImplementedError):
            MTDistGenMove(c, num_try=3, independent=True, **kw)
    for bad in (0, 65, -1, 2.0, "3", None, True):
        with pytest.raises(ValueError):
            MTDistGenMove(c, num_try=bad, independent=True)
    with pytest.raises(ValueError) as e:
        MTDistGenMove([uniform_dist(0.0, 1.0)], num_try=2, independent=True)
    assert str(e.value) == "Distributions need to be eryn.prior.ProbDistContainer object."
    with pytest.raises(NotImplementedError) as e:
        MTDistGenMove({"a": c, "b": c}, num_try=2, independent=True)
    assert "single branch" in str(e.value)
    forms = [MTDistGenMove(c, num_try=25, independent=True), MTDistGenMove({"model_0": c}, num_try=np.int64(25), independent=True),
             MTDistGenMove({0: uniform_dist(0.0, 1.0), 1: uniform_dist(-1.0, 1.0)}, num_try=25, independent=True)]
    for m in forms:
        assert isinstance(m, MHMove) and isinstance(m, DeviceMove) and m.num_try == 25 and m.independent
        kind, terms, K = m.device_proposal()
        assert kind == "mt_dist" and K == 25 and np.array_equal(terms["lo"], [0.0, -1.0]) and np.array_equal(terms["hi"], [1.0, 1.0])
    assert MTDistGenMove(c, independent=True).num_try == 1                  # the reference's default
    k25, k24 = mh_slot_key(forms[0].device_proposal()), mh_slot_key(MTDistGenMove(c, num_try=24, independent=True).device_proposal())
    assert k25 != k24 and k25 == mh_slot_key(forms[1].device_proposal())
    from eryn_amd.moves import DistributionGenerate
    assert mh_slot_key(DistributionGenerate({"model_0": c}).device_proposal()) != mh_slot_key(MTDistGenMove(c, independent=True).device_proposal())


def test_the_c_abi_is_bound():
    import re
    from eryn_amd import _lib
    header = open(os.path.join(os.path.dirname(HERE), "include", "hipensemble.h")).read()
    for fn in ("hens_set_mt_dist_proposal", "hens_mt_dist_step", "hens_mt_debug_draws"):
        m = re.search(r"\nint " + fn + r"\(([^;]*)\);", header)
        assert m, f"{fn} is not declared in the header"
        params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
        res, args = _lib.SIGNATURES[fn]
        assert len(args) == len(params), f"{fn}: {len(params)} parameters in the header, {len(args)} in _lib.SIGNATURES"
        import ctypes as C
        for p, a in zip(params, args):
            want = C.c_void_p if "*" in p else {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double}[p.split()[0]]
            assert a is want, f"{fn}: parameter '{p}' is bound as {a}"


# ---- the sizing of the GPU cases --------------------------------------------------------------------------------------------------------------
def test_the_issues_case_table():
    got = sorted((c["T"], c["W"], c["D"], c["K"]) for c in mt.CASES.values())
    assert got == sorted([(3, 40, 4, 5), (3, 33, 11, 2), (4, 64, 16, 3), (2, 128, 32, 25), (2, 9, 64, 64), (2, 5, 128, 64), (2, 5, 128, 3),
                          (1, 20, 24, 7), (2, 3, 8, 16)])
    from tests.production_draws import label_cb
    for name in mt.RECORDS:                      # hens_step packs walker records where the labelling has a column block
        assert label_cb(mt.CASES[name]["T"], mt.CASES[name]["W"]) > 0 and mt.CASES[name]["weight"] < 1.0


@pytest.mark.parametrize("name", sorted(mt.CASES))
def test_gpu_cases_are_sized_and_free_of_knife_edges(name):
    """The teacher-forced proposals and the replayed iterations of a case on the specification alone: no pick and no accept decision
    on the knife edge in either, and between them every coverage counter of the case."""
    c = mt.CASES[name]
    assert c["T"] <= 4 and c["W"] <= 128 and 1 <= c["K"] <= mt.MAX_TRY and c["iters"] <= 10
    forced, prob, x0 = mt.forced_run(c)
    free, _, _ = mt.free_run(c)
    for part, cnt in (("teacher-forced", forced), ("replay", free)):
        assert cnt.knife_picks == 0 and cnt.knife_accepts == 0, f"{name}, {part}: a decision on the knife edge: pick another seed"
        assert cnt.old_outside_accepted == 0 and cnt.accepted.sum() > 0 and cnt.picks_beyond_0 > 0
    both = mt.Counts(c["T"])
    for k in vars(both):
        setattr(both, k, getattr(forced, k) + getattr(free, k))
    mt.assert_coverage(both, prob, x0, spare=2, what=name)
