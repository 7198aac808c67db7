"""Per-parameter prior terms on the host (no GPU): the specification tests/prior_terms.py and ``eryn_amd.prior`` against the REAL
reference and against exact arithmetic, the Python surface, the fixture the reference recorded (tests/golden/priors/p1_priors.npz,
tests/golden/make_golden_priors.py) through the oracle under the substituted prior, and the sizing of the cases
tests/test_hip_priors.py replays on the GPU."""
import os
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import prior_terms as pt
from tests.prior_terms import fixture_problem, load_fixture

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
REFERENCE = "/root/reference/src"


def _have_scipy():
    try:
        import scipy.stats  # noqa: F401
        return True
    except Exception:
        return False


needs_reference = pytest.mark.skipif(not (os.path.isdir(os.path.join(REFERENCE, "eryn")) and _have_scipy()),
                                     reason="the reference tree or SciPy is not on this machine")


# ---- the specification against the real reference -------------------------------------------------------------------------------------------
def _reference():
    for m in ("corner", "seaborn"):           # imported unconditionally by the reference's plotting module
        sys.modules.setdefault(m, types.ModuleType(m))
    if REFERENCE not in sys.path:
        sys.path.insert(0, REFERENCE)
    import eryn.prior as ref
    return ref


ENTRIES = [("uniform", -2.0, 2.5), ("log_uniform", 1e-3, 2.999), ("normal", -0.6, 0.8), ("log_uniform", 5e-3, 7.995),
           ("uniform", 10.0, 1e4), ("normal", 3.0e2, 1e-3), ("log_uniform", 1e-8, 1e8), ("normal", 0.0, 1.0)]


def _points(spec, n=400, seed=0):
    """random points inside the supports, then rows with ONE coordinate exactly on each bound, one ulp inside, one ulp outside, and
    +-inf (NaN: see tests/prior_terms.py)"""
    rs = np.random.RandomState(seed)
    D = len(spec["kind"])
    lo = np.where(np.isfinite(spec["lo"]), spec["lo"], spec["c0"] - 5 * spec["c1"])
    hi = np.where(np.isfinite(spec["hi"]), spec["hi"], spec["c0"] + 5 * spec["c1"])
    lg = spec["kind"] == pt.LOG_UNIFORM
    x = lo + (hi - lo) * rs.uniform(size=(n, D))
    x[:, lg] = np.exp(np.log(lo[lg]) + (np.log(hi[lg]) - np.log(lo[lg])) * rs.uniform(size=(n, int(lg.sum()))))
    x = np.minimum(np.maximum(x, lo), hi)
    rows = [x]
    base = x[0]
    for d in range(D):
        vals = [np.inf, -np.inf, spec["c0"][d], np.nextafter(spec["c0"][d], np.inf)]
        if np.isfinite(spec["lo"][d]):
            a, b = spec["lo"][d], spec["hi"][d]
            vals += [a, b, np.nextafter(a, np.inf), np.nextafter(b, -np.inf), np.nextafter(a, -np.inf), np.nextafter(b, np.inf)]
        else:
            vals += [spec["c0"][d] + 1e100 * spec["c1"][d], spec["c0"][d] - 1e100 * spec["c1"][d]]
        for v in vals:
            r = base.copy()
            r[d] = v
            rows.append(r[None])
    return np.concatenate(rows)


def _reference_container(ref, entries, order):
    from scipy import stats
    made = {}
    for d in order:
        name, a, b = entries[d]
        made[d] = ref.uniform_dist(a, b) if name == "uniform" else stats.loguniform(a, b) if name == "log_uniform" else stats.norm(a, b)
    return ref.ProbDistContainer(made)


@needs_reference
@pytest.mark.parametrize("order", ["ascending", "descending", "shuffled"])
def test_specification_is_the_reference_bit_for_bit(order):
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, uniform_dist
    ref = _reference()
    spec = pt.make_spec(ENTRIES)
    D = len(ENTRIES)
    keys = {"ascending": list(range(D)), "descending": list(range(D))[::-1], "shuffled": list(np.random.RandomState(4).permutation(D))}[order]
    keys = [int(k) for k in keys]
    x = _points(spec)
    with np.errstate(all="ignore"):
        want = _reference_container(ref, ENTRIES, keys).logpdf(x)
    got = pt.log_prior(spec, x, order=keys)                 # (the reference adds in the dictionary's order)
    assert np.isneginf(want).sum() >= 3 * D and np.isfinite(want).sum() > 400       # (+-inf everywhere, one ulp outside each bound)
    assert np.array_equal(got, want), f"specification vs reference: {int((got != want).sum())} of {want.size} differ"
    mine = {0: uniform_dist, 1: LogUniformDistribution, 2: NormalDistribution}
    names = {"uniform": 0, "log_uniform": 1, "normal": 2}
    c = ProbDistContainer({d: mine[names[ENTRIES[d][0]]](ENTRIES[d][1], ENTRIES[d][2]) for d in keys})
    assert all(np.array_equal(c.prior_terms()[k], spec[k]) for k in spec), "the container's constants are the specification's"
    asc = pt.log_prior(spec, x)
    assert np.array_equal(c.logpdf(x), asc), "eryn_amd.prior adds in ascending order, whatever the dictionary's"
    assert np.array_equal(np.isneginf(asc), np.isneginf(want))
    if order == "ascending":
        assert np.array_equal(c.logpdf(x), want)
        assert c.logpdf(x[3]) == want[3] and isinstance(c.logpdf(x[3]), float)


@needs_reference
def test_log_uniform_reproduces_the_reference_construction():
    """prior.py:115-136: log_uniform(min, max) is scipy.stats.loguniform(min, max - min) - the upper bound is max - min."""
    from eryn_amd.prior import log_uniform
    ref = _reference()
    theirs, mine = ref.log_uniform(1e-3, 3.0), log_uniform(1e-3, 3.0)
    assert theirs.args == (1e-3, 3.0 - 1e-3) and (mine.a, mine.b) == theirs.args
    assert (log_uniform(3.0, 1e-3).a, log_uniform(3.0, 1e-3).b) == theirs.args, "swapped arguments are put in order first"
    x = np.array([1e-3, np.nextafter(1e-3, 0), 0.5, 2.999, np.nextafter(2.999, 3), 3.0])
    assert np.array_equal(mine.logpdf(x), theirs.logpdf(x))


# ---- the specification against exact arithmetic ------------------------------------------------------------------------------------------------
def test_specification_against_exact_arithmetic():
    """|P - P*| <= B_P for the NumPy evaluation (log within 1 ulp), in the module's derived form everywhere and in the issue's form
    where no term cancels; a perturbed log of 1 ulp stays inside, a dropped term or a descending sum does not go unnoticed."""
    worst = 0.0
    for D, like in ((4, "dense"), (8, "dense"), (32, "dense"), (128, "dense"), (12, "rosen")):
        prob = pt.PriorProblem(D, like)
        x = np.concatenate([prob.x0(3, 136).reshape(-1, D), _points(prob.spec, n=200, seed=D)])
        P = pt.log_prior(prob.spec, x)
        Ps, B = pt.exact_log_prior(prob.spec, x), pt.float64_bound(prob.spec, x)
        fin = np.isfinite(Ps)
        assert np.array_equal(np.isneginf(P), ~fin) and fin.sum() > 400
        err = np.abs(P[fin].astype(pt.LD) - Ps[fin]).astype(np.float64)
        assert np.all(err <= B[fin]), f"D={D}: worst |P - P*| / B_P = {np.max(err / B[fin]):.3f}"
        worst = max(worst, float(np.max(err / B[fin])))
        Bi, ok = pt.issue_bound(prob.spec, x)
        assert ok[fin].sum() > 100 and np.all(err[ok[fin]] <= Bi[fin][ok[fin]]), "the bound in the issue's form, where no term cancels"
        # a wrong sum is far outside: the last term dropped
        t = pt.terms(prob.spec, x)[fin]
        dropped = t[:, :-1].sum(axis=1)
        tame = np.abs(Ps[fin]) < 1e6                           # (not the points 1e100 scales out: there B_P exceeds any one term)
        assert tame.sum() > 400 and np.all(np.abs(dropped.astype(pt.LD) - Ps[fin]).astype(np.float64)[tame] > B[fin][tame])
    print(f"worst |P - P*| / B_P of the NumPy specification: {worst:.3f}")
    assert worst < 1.0


def test_bound_admits_a_log_one_ulp_off():
    """the evaluation the bound is FOR: every log moved by one ulp, either way"""
    prob = pt.PriorProblem(16)
    x = prob.x0(3, 136).reshape(-1, 16)
    Ps, B = pt.exact_log_prior(prob.spec, x), pt.float64_bound(prob.spec, x)
    for sign in (-np.inf, np.inf):
        t = pt.terms(prob.spec, x)
        for d in prob.log_uniform:
            t[:, d] = (-np.nextafter(np.log(x[:, d]), sign)) - prob.spec["c0"][d]
        P = np.zeros(x.shape[0])
        for d in range(16):
            P += t[:, d]
        assert np.all(np.abs(P.astype(pt.LD) - Ps).astype(np.float64) <= B)


# ---- the Python surface ----------------------------------------------------------------------------------------------------------------------
def test_python_surface():
    from eryn_amd import _lib
    from eryn_amd.engine import box_logp_inside
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, log_uniform, uniform_dist
    lu = log_uniform(1e-3, 3.0)
    assert isinstance(lu, LogUniformDistribution) and (lu.a, lu.b) == (1e-3, 3.0 - 1e-3), "the reference's construction: max - min"
    box = ProbDistContainer({0: uniform_dist(-1.0, 2.0), 1: uniform_dist(5.0, 0.5)})
    t = box.prior_terms()
    lo, hi = box.box_bounds()
    assert box.is_box and np.array_equal(t["lo"], lo) and np.array_equal(t["hi"], hi) and np.all(t["kind"] == _lib.PRIOR_UNIFORM)
    assert np.array_equal(t["c0"], orc.box_logpdf_vals(lo, hi)) and t["c0"][0] + t["c0"][1] == box_logp_inside(lo, hi)
    assert np.array_equal(box.logpdf(np.array([[0.0, 1.0], [0.0, 6.0]])), orc.box_log_prior(np.array([[0.0, 1.0], [0.0, 6.0]]), lo, hi))
    mixed = ProbDistContainer({1: lu, 0: NormalDistribution(1.0, 2.0), 2: uniform_dist(0.0, 1.0)})
    assert not mixed.is_box and mixed.ndim == 3 and list(mixed.prior_terms()["kind"]) == [2, 1, 0]
    with pytest.raises(NotImplementedError):
        mixed.box_bounds()
    np.random.seed(3)
    r = mixed.rvs(size=(5, 7))
    assert r.shape == (5, 7, 3) and np.isfinite(mixed.logpdf(r.reshape(-1, 3))).all(), "rvs draws inside the supports"
    for bad in ({(0, 1): uniform_dist(0, 1)}, {"a": uniform_dist(0, 1)}, {0: object()}, {0: types.SimpleNamespace(logpdf=None, rvs=None)}):
        with pytest.raises(NotImplementedError):
            ProbDistContainer(bad)
    with pytest.raises(ValueError):
        ProbDistContainer({0: uniform_dist(0, 1), 2: uniform_dist(0, 1)})
    for args in ((0.0, 1.0), (-1.0, 1.0), (2.0, 2.0), (1.0, np.inf)):
        with pytest.raises(ValueError):
            LogUniformDistribution(*args)
    for args in ((0.0, 0.0), (0.0, -1.0), (np.inf, 1.0), (0.0, np.inf)):
        with pytest.raises(ValueError):
            NormalDistribution(*args)
    # one reading of a prior, however it is written (prior_spec), and one gather of the C arguments (term_arrays)
    from eryn_amd.prior import box_constant, prior_spec, term_arrays
    forms = [prior_spec(box), prior_spec(box.priors_in), prior_spec(t), prior_spec(list(zip(lo, hi))), prior_spec((lo, hi), 2, bounds=True)]
    for s in forms:
        assert s.is_box and s.terms_beyond_box is None and s.logp_inside == box_logp_inside(lo, hi) == box_constant(t["c0"])
        assert all(np.array_equal(s.terms[k], t[k]) and s.terms[k].dtype == t[k].dtype and s.terms[k].flags.c_contiguous for k in t)
        assert s.lo is s.terms["lo"] and s.hi is s.terms["hi"] and prior_spec(s) is s
    assert forms[0].container is box and forms[1].container.is_box and all(s.container is None for s in forms[2:])
    assert box_constant([1e16, 1.0, 1.0]) == 1e16 != box_constant([1.0, 1.0, 1e16]), "ascending, from 0.0"
    b1 = prior_spec((-1.0, 2.0), 3, bounds=True)
    assert np.array_equal(b1.lo, [-1.0] * 3) and b1.logp_inside == (np.log(1 / 3.0) + np.log(1 / 3.0)) + np.log(1 / 3.0)
    m = prior_spec(mixed, 3)
    assert not m.is_box and m.logp_inside is None and m.terms_beyond_box is m.terms and m.container is mixed
    with pytest.raises(ValueError, match="prior terms must have shape"):
        prior_spec(mixed, 4)
    with pytest.raises(NotImplementedError, match="priors must be per-parameter"):
        prior_spec(None)
    wide = term_arrays(m.terms, 5)
    assert [a.dtype for a in wide] == [np.int32] + [np.float64] * 5 and all(a.shape == (5,) and a.flags.c_contiguous for a in wide)
    assert wide[0].tolist() == [2, 1, 0, 0, 0] and np.isneginf(wide[1][3:]).all() and np.isposinf(wide[2][3:]).all(), "the pad: uniform on the line"
    assert all(np.array_equal(a[:3], m.terms[k]) and (k in ("kind", "lo", "hi") or not a[3:].any()) for k, a in zip(t, wide))
    both = term_arrays([m.terms, t])
    assert all(np.array_equal(a, np.concatenate([m.terms[k], t[k]])) for k, a in zip(t, both)) and both[0].dtype == np.int32


def test_term_parser_and_box_fold_under_a_sanitizer_build(tmp_path):
    """tools/prior_host_check.cpp: a stand-alone program over csrc/hens_prior_host.h - the one parser of a caller's prior term (every
    refusal tests/test_hip_priors.py and tests/test_hip_rj_priors.py list, in both entry points' modes, and an accepted term of each
    kind byte for byte) and the fold of a parsed run into a box - built with -fsanitize=address,undefined where the compiler has the
    runtimes (plainly otherwise) and run on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(os.path.dirname(HERE), "tools", "prior_host_check.cpp"), str(tmp_path / "prior_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    build = "sanitizer build (address, undefined)"
    if r.returncode != 0:
        build = "plain build - the sanitizer build failed: " + (r.stderr.strip().splitlines() or ["no message"])[-1]
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("prior_host_check:", build)                # (pytest -rA shows which build ran)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


def test_scipy_objects_are_recognised_by_duck_typing():
    """frozen uniform / loguniform / reciprocal / norm by ``.dist.name``, ``.args``, ``.kwds``; stand-ins first (SciPy is not needed),
    then the real objects where SciPy is installed"""
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, UniformDistribution

    def frozen(name, *args, **kwds):
        return types.SimpleNamespace(dist=types.SimpleNamespace(name=name), args=args, kwds=kwds, logpdf=None, rvs=None)

    c = ProbDistContainer({0: frozen("uniform", -1.0, 3.0), 1: frozen("loguniform", 1e-2, 10.0), 2: frozen("norm", loc=0.5, scale=2.0),
                           3: frozen("reciprocal", 1e-2, 10.0, loc=0.0), 4: frozen("norm"), 5: frozen("uniform", loc=2.0)})
    kinds = [type(d) for d in c.dists]
    assert kinds == [UniformDistribution, LogUniformDistribution, NormalDistribution, LogUniformDistribution, NormalDistribution, UniformDistribution]
    assert (c.dists[0].min_val, c.dists[0].max_val) == (-1.0, 2.0) and (c.dists[5].min_val, c.dists[5].max_val) == (2.0, 3.0)
    assert (c.dists[2].loc, c.dists[2].scale, c.dists[4].loc, c.dists[4].scale) == (0.5, 2.0, 0.0, 1.0)
    for bad in (frozen("loguniform", 1e-2, 10.0, 1.0), frozen("loguniform", 1e-2, 10.0, scale=2.0), frozen("gamma", 2.0),
                frozen("norm", 0.0, 1.0, 2.0), frozen("loguniform", 1e-2)):
        with pytest.raises(NotImplementedError):
            ProbDistContainer({0: bad})
    if _have_scipy():
        from scipy import stats
        c = ProbDistContainer({0: stats.uniform(-1.0, 3.0), 1: stats.loguniform(1e-2, 10.0), 2: stats.norm(loc=0.5, scale=2.0), 3: stats.reciprocal(1e-2, 10.0)})
        x = np.array([[0.0, 1.0, 0.3, 5.0], [2.0, 10.0, -7.0, 1e-2], [2.1, 1.0, 0.0, 1.0]])
        want = np.zeros(3)
        for d, dist in enumerate((stats.uniform(-1.0, 3.0), stats.loguniform(1e-2, 10.0), stats.norm(loc=0.5, scale=2.0), stats.reciprocal(1e-2, 10.0))):
            want += dist.logpdf(x[:, d])
        assert np.array_equal(c.logpdf(x), want)
        with pytest.raises(NotImplementedError):
            ProbDistContainer({0: stats.loguniform(1e-2, 10.0, loc=1.0)})
        with pytest.raises(NotImplementedError):
            ProbDistContainer({0: stats.gamma(2.0)})


def test_samplers_refuse_what_they_refused():
    """no GPU is touched: the refusals come before a context is made"""
    from eryn_amd.prior import NormalDistribution, ProbDistContainer, uniform_dist
    from eryn_amd.rj import RJEnsembleSampler
    mixed = ProbDistContainer({0: uniform_dist(0.0, 1.0), 1: NormalDistribution(0.0, 1.0), 2: uniform_dist(0.0, 1.0)})
    with pytest.raises(NotImplementedError):
        RJEnsembleSampler(8, {"a": 3}, None, {"a": mixed}, tempering_kwargs=dict(ntemps=2), nleaves_max={"a": 2}, nleaves_min={"a": 0})


# ---- the fixture from the real reference ------------------------------------------------------------------------------------------------------
def test_fixture_exercises_the_terms():
    fx = load_fixture()
    assert (int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"])) == (3, 10, 4, 6) and list(fx["prior_kind"]) == [0, 1, 2, 1]
    n_inf = sum(int(np.isinf(fx[f"it{i}_logp{sp}"]).sum()) for i in range(6) for sp in (0, 1))
    acc = sum(int(fx[f"it{i}_keep{sp}"].sum()) for i in range(6) for sp in (0, 1))
    assert n_inf >= 10 and acc >= 50 and fx["accepted_total"].sum() == acc
    assert os.path.getsize(os.path.join(GOLDEN, "priors", "p1_priors.npz")) < os.path.getsize(os.path.join(GOLDEN, "f2_pt.npz"))
    assert not np.array_equal(fx["it5_betas"], fx["betas0"]), "the ladder adapted"


def test_oracle_under_the_substituted_prior_reproduces_the_fixture(monkeypatch):
    from tests.test_oracle_golden import _same
    fx = load_fixture()
    prob = fixture_problem(fx)
    pt.install(monkeypatch, prob)
    o = orc.OracleSampler(fx["x0"], prob.loglike, prob.lo, prob.hi, np.random.RandomState(int(fx["seed_construct"])),
                          np.random.RandomState(int(fx["seed_run"])), betas=fx["betas0"], a=float(fx["a"]), record=True)
    _same(o.P, fx["P0"], "P0")
    _same(o.L, fx["L0"], "L0")
    for it in range(int(fx["nsteps"])):
        o.iteration()
        rec, pre = o.trace[-1], f"it{it}_"
        _same(rec["labels"], fx[pre + "labels"], "labels")
        for sp in (0, 1):
            for k in ("rint", "u_zz", "u_acc", "q", "factors", "logp", "logl", "keep"):
                _same(rec[f"{k}{sp}"], fx[pre + f"{k}{sp}"], f"{pre}{k}{sp}")
            _same(orc.split_index_lists(rec["labels"], sp, 2)[0], fx[pre + f"S{sp}"], f"{pre}S{sp}")
        _same(rec["x_after1"], fx[pre + "x_stretch"], "x_stretch")
        for k in ("L_stretch", "P_stretch", "iperm", "i1perm", "u_swap", "sel", "swaps_accepted", "x", "L", "P"):
            _same(rec[k], fx[pre + k], pre + k)
        _same(rec["betas_after"], fx[pre + "betas"], "betas")
    _same(o.accepted, fx["accepted_total"], "accepted_total")
    assert o.num_proposals == int(fx["num_proposals"])


@needs_reference
def test_generator_reproduces_the_committed_fixture(tmp_path):
    """build container only: copies of the generators run against the real reference give the committed file, array for array"""
    for g in ("make_golden.py", "make_golden_priors.py"):
        shutil.copy(os.path.join(GOLDEN, g), tmp_path / g)
    shutil.copy(os.path.join(HERE, "ladders.py"), tmp_path / "ladders.py")
    r = subprocess.run([sys.executable, str(tmp_path / "make_golden_priors.py")], cwd=str(tmp_path), capture_output=True, text=True,
                       timeout=600, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    assert r.returncode == 0, r.stdout + r.stderr
    new, old = np.load(tmp_path / "priors" / "p1_priors.npz", allow_pickle=False), load_fixture()
    assert sorted(new.files) == sorted(old.files) and len(old.files) > 150
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and np.array_equal(new[k], old[k], equal_nan=True), k


# ---- coverage sizing, oracle only ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pt.CASES))
def test_replayed_cases_are_sized_with_a_factor_of_two_to_spare(name, monkeypatch):
    """With NumPy's draws in place of the device's, the ORACLE alone meets every coverage condition of tests/test_hip_priors.py twice
    over: the share of -inf proposals inside [0.10, 0.45], every log-uniform bound the sole offender of two proposals or more, 40
    accept decisions that a constant prior would have made differently."""
    cnt, prob = pt.oracle_case(monkeypatch, name)
    c = pt.CASES[name]
    assert len(prob.log_uniform) >= 2 and all(prob.hi[d] / prob.lo[d] >= 1e3 for d in prob.log_uniform), "three decades"
    assert np.all(prob.spec["kind"][[d for d in range(c["D"]) if d % 4 == 1 and d not in prob.log_uniform]] == pt.NORMAL)
    pt.assert_coverage(cnt, prob, spare=2, what=name)
