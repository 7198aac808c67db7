"""CPU tests of the draw-from-distribution move: the specification (tests/dist_move.py) against the fixtures captured from the real
reference (tests/golden/distgen/), the production draws' statement, the class's argument errors, and the sizing of every GPU case of
tests/test_hip_dist_move.py on the specification alone."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import dist_move as dm
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests.test_prior_terms import GOLDEN, HERE, needs_reference

LD = np.longdouble


def _same(a, b, what):
    assert np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True), f"{what} differs from the fixture"


# ---- the specification against the reference's fixtures ----------------------------------------------------------------------------------
def replay_fixture(fx, step_dist, monkeypatch=None):
    """Walk a fixture: every move iteration through ``step_dist(x, L, P, betas, rec) -> (keep, factors)`` (in place), every stretch
    iteration through the pinned oracle under the fixture's prior, the sweep and the adaptation through the oracle; everything is
    held to the fixture bit for bit.  -> per-iteration dicts of the move iterations."""
    prior, gen = dm.fixture_specs(fx)
    loglike = dm.fixture_loglike(fx)
    T, W, D = int(fx["T"]), int(fx["W"]), int(fx["D"])
    x, L, P = fx["x0"].copy(), fx["L0"].copy(), fx["P0"].copy()
    betas = fx["betas0"].copy() if "betas0" in fx else None
    if monkeypatch is not None:
        monkeypatch.setattr(orc, "box_log_prior", pt.box_prior_substitute(prior))
    seen = []
    for it in range(int(fx["nsteps"])):
        rec = dm.fixture_iteration(fx, it)
        what = f"iteration {it}"
        if rec["is_dist"]:
            x_old = x.copy()
            keep, factors, info = step_dist(x, L, P, betas, rec)
            _same(keep, rec["keep"], what + ": accept mask")
            seen.append(dict(rec, x_old=x_old, info=info, factors_spec=factors))
        else:
            for sp in range(2):
                out = orc.stretch_split(x, L, P, betas, rec["labels"], sp, rec[f"rint{sp}"], rec[f"u_zz{sp}"], rec[f"u_acc{sp}"], float(fx["a"]),
                                        prior["lo"], prior["hi"], loglike)
                _same(out["keep"], rec[f"keep{sp}"], what + f": stretch accept mask {sp}")
        _same(x, rec["x_move"], what + ": x after the move")
        _same(P, rec["P_move"], what + ": log-prior after the move")
        _same(L, rec["L_move"], what + ": log-likelihood after the move")
        if betas is not None:
            sel, sw = orc.pt_sweep(x, L, P, betas, rec["iperm"], rec["i1perm"], rec["u_swap"])
            _same(sel, rec["sel"], what + ": swap mask")
            _same(sw, rec["swaps_accepted"], what + ": swap counts")
            betas = orc.adapt_ladder(betas, sw, W, it)
            _same(betas, rec["betas"], what + ": ladder")
        _same(x, rec["x"], what + ": x")
        _same(L, rec["L"], what + ": L")
        _same(P, rec["P"], what + ": P")
    return seen


@pytest.mark.parametrize("name", dm.FIXTURES)
def test_specification_reproduces_the_reference_fixtures(name, monkeypatch):
    fx = dm.load_fixture(name)
    prior, gen = dm.fixture_specs(fx)
    loglike = dm.fixture_loglike(fx)

    def step(x, L, P, betas, rec):
        info = {}
        _, _, _, keep, factors = dm.dist_step(x, L, P, betas, rec["q"], rec["u_acc"], prior, gen, loglike, info=info)
        _same(factors, rec["factors"], "factors")
        _same(info["logp"], rec["logp"], "logp")
        _same(info["logl"], rec["logl"], "logl")
        return keep, factors, info

    seen = replay_fixture(fx, step, monkeypatch)
    T = int(fx["T"])
    assert len(seen) == int(fx["kind"].sum()) == int(fx["num_proposals_dist"])
    accepted = sum(r["keep"].astype(int) for r in seen)
    _same(accepted, fx["accepted_dist"], "the move's accept counts")
    assert (accepted.sum(axis=1) > 0).all(), "accepts on every rung"
    knives = old_out = inf_prior = 0
    for r in seen:
        with np.errstate(divide="ignore"):
            knives += int(pu.knife_edge(r["info"]["lnpdiff"], np.log(r["u_acc"])).sum())
        out = np.isneginf(r["factors"])
        old_out += int(out.sum())
        assert not (out & r["keep"]).any(), "an old point outside the generator was moved"
        inf_prior += int(np.isinf(r["logp"]).sum())
        # the float64 factors sit within B_F of exact arithmetic
        Fs, B = dm.exact_factors(gen, r["x_old"], r["q"])
        fin = np.isfinite(r["factors"])
        assert (np.abs(r["factors"][fin].astype(LD) - Fs[fin]).astype(np.float64) <= B[fin]).all()
    assert knives == 0, "an accept decision within 1e-12 of the knife edge"
    if name == "dg1_mix":
        assert inf_prior >= 1 and old_out >= 1 and (fx["kind"] == 0).any()
    else:
        assert np.all(np.concatenate([r["factors"].ravel() for r in seen]) == 0.0), "generator = the box: the factor cancels to the bit"


@pytest.mark.parametrize("name", dm.FIXTURES)
def test_eryn_amd_containers_draw_the_fixtures_points(name):
    """eryn_amd.prior containers built with the reference's calls give the fixture's q from the same global seed: the global stream is
    consumed by the label shuffles of a stretch iteration, the move's rvs and the sweep's permutations and uniforms, in that order."""
    fx = dm.load_fixture(name)
    T, W, D = int(fx["T"]), int(fx["W"]), int(fx["D"])
    _, gen = dm.fixture_containers(fx)
    np.random.seed(int(fx["seed_run"]))
    for it in range(int(fx["nsteps"])):
        rec = dm.fixture_iteration(fx, it)
        if rec["is_dist"]:
            _same(gen.rvs(size=T * W).reshape(T, W, D), rec["q"], f"iteration {it}: q")
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
    for g in ("make_golden.py", "make_golden_priors.py", "make_golden_dist.py"):
        shutil.copy(os.path.join(GOLDEN, g), tmp_path / g)
    shutil.copy(os.path.join(HERE, "ladders.py"), tmp_path / "ladders.py")
    out = tmp_path / "out"
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_dist.py")], cwd=str(tmp_path), capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1", GOLDEN_OUT=str(out)))
    assert r.returncode == 0, r.stdout + r.stderr
    for name in dm.FIXTURES + dm.PERIODIC_FIXTURES:
        new, old = np.load(out / (name + ".npz"), allow_pickle=False), dm.load_fixture(name)
        assert sorted(new.files) == sorted(old) and len(old) > 30
        for k in old:
            assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=True), k
        assert os.path.getsize(os.path.join(GOLDEN, "distgen", name + ".npz")) < 100_000


# ---- the class -------------------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_class():
    from eryn_amd.moves import DistributionGenerate, MHMove
    from eryn_amd.moves.device import DeviceMove
    from eryn_amd.prior import ProbDistContainer, uniform_dist
    c = ProbDistContainer({0: uniform_dist(0.0, 1.0), 1: uniform_dist(-1.0, 1.0)})
    with pytest.raises(ValueError) as e:
        DistributionGenerate(c)
    assert str(e.value).startswith("When entering directly into the DistributionGenerate class, generate_dist must be a dictionary.")
    with pytest.raises(ValueError) as e:
        DistributionGenerate({"model_0": [uniform_dist(0.0, 1.0)]})
    assert str(e.value) == "Distributions need to be eryn.prior.ProbDistContainer object."
    with pytest.raises(NotImplementedError) as e:
        DistributionGenerate({"a": c, "b": c})
    assert "single branch" in str(e.value)
    m = DistributionGenerate({"model_0": c})
    assert isinstance(m, MHMove) and isinstance(m, DeviceMove)
    kind, terms = m.device_proposal()
    assert kind == "dist" and np.array_equal(terms["lo"], [0.0, -1.0]) and np.array_equal(terms["hi"], [1.0, 1.0])
    m2 = DistributionGenerate({"model_0": {0: uniform_dist(0.0, 1.0), 1: uniform_dist(-1.0, 1.0)}})       # the dict a container is made of
    assert all(np.array_equal(m2.device_proposal()[1][k], terms[k]) for k in terms)


def test_the_c_abi_is_bound():
    from eryn_amd import _lib
    assert len(_lib.SIGNATURES["hens_set_dist_proposal"][1]) == 8 and len(_lib.SIGNATURES["hens_dist_step"][1]) == 5
    header = open(os.path.join(os.path.dirname(HERE), "include", "hipensemble.h")).read()
    assert "int hens_set_dist_proposal(hens_ctx*" in header and "int hens_dist_step(hens_ctx*" in header


# ---- the production draws ---------------------------------------------------------------------------------------------------------------------
def test_dist_draws_statement():
    gen = pt.make_spec([("uniform", -1.5, 2.0), ("log_uniform", 0.05, 2.45), ("normal", -0.3, 0.6), ("normal", 2.0, 1.0), ("uniform", 1e3, 1e3 + 1e-9)])
    T, W = 3, 50
    X, Xs, E = dm.dist_draws(7, 5, T, W, gen)
    uni = gen["kind"] == pt.UNIFORM
    # a uniform value is the float64 statement u (hi - lo) + lo itself (the device's is held to it bit for bit); against X* it carries
    # its two roundings - the product's and the sum's - so it is X* rounded but for those: |X - X*| <= u (|u (hi - lo)| + |X*|)
    width = (gen["hi"] - gen["lo"])[uni]
    two = pt.U * (np.abs(Xs[..., uni] - gen["lo"][uni].astype(LD)) + np.abs(Xs[..., uni])).astype(np.float64) * (1 + 1e-9) + 0.0 * width
    assert (np.abs(X[..., uni].astype(LD) - Xs[..., uni]).astype(np.float64) <= two).all()
    assert np.mean(X[..., 0] == Xs[..., 0].astype(np.float64)) > 0.5, "mostly the correctly rounded value"
    assert (np.abs(X.astype(LD) - Xs).astype(np.float64)[..., ~uni] <= E[..., ~uni]).all()
    for d in (0, 1, 4):
        assert (X[..., d] >= gen["lo"][d]).all() and (X[..., d] <= gen["hi"][d]).all()
    # another iteration, another rung offset, another coordinate: other words
    assert not np.array_equal(dm.dist_words(7, 5, T, W, 0)[0], dm.dist_words(7, 6, T, W, 0)[0])
    assert not np.array_equal(dm.dist_words(7, 5, T, W, 0)[0], dm.dist_words(7, 5, T, W, 1)[0])
    assert np.array_equal(dm.dist_words(7, 5, T, W, 2, rung_begin=1)[0][0], dm.dist_words(7, 5, T, W, 2)[0][1])
    assert np.isfinite(pt.log_prior(gen, X.reshape(-1, 5))).all(), "every draw has a finite log q"


def test_the_clamp_on_hand_made_words():
    """u = 0 and u = 1 - 2^-53 on a log-uniform support whose exp(log a) rounds below a (found by search): unclamped, the draw at
    u = 0 lies outside [a, b] and its log q is -inf; the clamp puts it on the bound."""
    a = None
    for k in range(1, 4000):
        cand = 0.05 + k * 1e-3
        if np.exp(np.log(cand)) < cand:
            a = cand
            break
    assert a is not None, "no support below whose lower bound exp(log a) rounds"
    b = 40.0 * a
    gen = pt.make_spec([("log_uniform", a, b), ("uniform", -1.0, 3.0)])
    z = np.zeros((1, 2), dtype=np.uint64)
    ones = np.full((1, 2), 0xFFFFFFFF, dtype=np.uint64)
    words = [np.where([[True, False]], z, ones), np.where([[True, False]], z, ones), z, z]        # u = 0 | u = 1 - 2^-53
    from tests import rj_prior_terms as rpt
    from tests.production_draws import u01
    assert u01(words[0], words[1])[0, 0] == 0.0 and u01(words[0], words[1])[0, 1] == 1.0 - 2.0 ** -53
    raw, _, _ = rpt.birth_spec(gen, 0, words)
    assert raw[0, 0] < a and np.isneginf(pt.log_prior(gen, np.array([[raw[0, 0], 0.0]]))[0]), f"a = {a!r}: the unclamped draw is inside"
    X, Xs, _ = dm.value_of(gen, 0, words)
    assert X[0, 0] == a and X[0, 1] <= b and np.isfinite(pt.log_prior(gen, np.array([[X[0, 0], 0.0], [X[0, 1], 0.0]]))).all()
    Xu, _, _ = dm.value_of(gen, 1, words)
    assert Xu[0, 0] == -1.0 and -1.0 <= Xu[0, 1] <= 3.0
    print(f"the support [a, 40 a] with a = {a!r}: exp(log a) = {np.exp(np.log(a))!r} < a")


# ---- the sizing of the GPU cases --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dm.CASES))
def test_gpu_cases_are_sized_with_a_factor_of_two_to_spare(name):
    cnt, prob, x0 = dm.free_run(dm.CASES[name])
    c = dm.CASES[name]
    assert c["T"] <= 4 and c["W"] <= 136 and 6 <= c["iters"] <= 10
    dm.assert_coverage(cnt, prob, x0, spare=2, what=name)
