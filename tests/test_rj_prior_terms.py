"""tests/rj_prior_terms.py on the CPU: ``TermBranch`` against the real ``ProbDistContainer`` of eryn_amd.prior, the exact log-prior of a
state and its bound against the oracle's float64 evaluation, the specification of the device's births, the Python surface of leaf
priors, and the sizing of the cases tests/test_hip_rj_priors.py replays on the GPU (the oracle alone, NumPy's draws, a spare factor 2)."""
import numpy as np
import pytest

from oracle import eryn_oracle_rj as orj
from tests import prior_terms as pt
from tests import rj_prior_terms as rp
from tests.production_draws import normal_stream_stats, normal_stream_violations

KINDS = sorted(rp.ENTRIES)


def _points(b, rs, n):
    """Leaves from the prior, a quarter of them with one parameter pushed to or past a bound / far out."""
    x = b.rvs(n, rs)
    for i in range(0, n, 4):
        d = rs.randint(b.ndim)
        lo, hi = b.spec["lo"][d], b.spec["hi"][d]
        x[i, d] = rs.choice([lo, hi, np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)]) if np.isfinite(lo) else rs.choice([1e200, -1e200, 30.0])
    return x


@pytest.mark.parametrize("kind", KINDS)
def test_term_branch_is_the_container(kind):
    """leaf_logpdf = eryn_amd.prior.ProbDistContainer.logpdf and rvs = its rvs on the same stream, bit for bit."""
    b = rp.branches_of((kind,), (3,), (0,))[0]
    c = b.container()
    rs = np.random.RandomState(1)
    x = _points(b, rs, 400)
    got, want = b.leaf_logpdf(x), c.logpdf(x)
    assert np.array_equal(got, want) and np.isneginf(got).sum() > 20 and np.isfinite(got).sum() > 200
    np.random.seed(9)
    want = c.rvs(50)
    assert np.array_equal(b.rvs(50, np.random.RandomState(9)), want)
    terms = c.prior_terms()
    for k in ("kind", "lo", "hi", "c0", "c1", "c2"):
        assert np.array_equal(terms[k], b.spec[k]), f"the container's terms are not the specification's ({k})"


def test_oracle_log_prior_is_within_the_bound_of_exact_arithmetic():
    """The oracle's float64 log-prior of random states (dead slots holding leaves, zeros and 1e300) against exact arithmetic."""
    kinds = ("offset", "ramp", "pulse", "burst", )
    brs = rp.branches_of(kinds, (2, 3, 10, 4), (0, 0, 0, 0))
    rs = np.random.RandomState(3)
    x, inds = rp.start_state(brs, 4, 64, rs)
    for b in brs:                                                  # some active leaves at and past a bound
        flat = x[b.name].reshape(-1, b.ndim)
        flat[::7] = _points(b, rs, flat[::7].shape[0])
    P = orj.compute_log_prior(x, inds, brs)
    r = rp.worst_state_ratio(P, brs, x, inds)
    print(f"oracle float64 log-prior: worst |P - P*| / B = {r:.3f}; {int(np.isneginf(P).sum())} of {P.size} at -inf")
    assert r <= 1.0 and 0 < np.isneginf(P).sum() < P.size
    for fill in (0.0, -2.0, 1e300):                                 # dead slots are not part of P*
        xf = {k: v.copy() for k, v in x.items()}
        for b in brs:
            xf[b.name][~inds[b.name]] = fill
        assert np.array_equal(rp.exact_state_log_prior(brs, xf, inds), rp.exact_state_log_prior(brs, x, inds))
        with np.errstate(all="ignore"):
            assert np.array_equal(orj.compute_log_prior(xf, inds, brs), P)


def test_birth_specification():
    """uniform: the float64 statement is the formula; log-uniform and normal: NumPy's own float64 evaluation is within the a-priori
    bound of exact arithmetic; the normals behind 3 x 2 x 512 x 4 births look like normals."""
    seed, T, W = 77, 2, 512
    brs = rp.branches_of(("offset", "ramp", "pulse", "burst"), (2, 2, 2, 2), (0, 0, 0, 0))
    zs = []
    for it in range(3):
        row = []
        for bi, b in enumerate(brs):
            for d in range(b.ndim):
                w = rp.birth_words(seed, it, T, W, bi, d)
                X, Xs, E = rp.birth_spec(b.spec, d, w)
                k = b.spec["kind"][d]
                assert X.shape == (T, W)
                if k == pt.UNIFORM:
                    assert (E == 0).all() and ((X >= b.spec["lo"][d]) & (X <= b.spec["hi"][d])).all()
                    continue
                err = np.abs(X.astype(rp.LD) - Xs).astype(np.float64)
                assert (err <= E).all() and (E > 0).all(), f"{b.name}[{d}]: NumPy's float64 value is {float((err / E).max()):.2f} of the bound off"
                if k == pt.NORMAL:
                    row.append(rp.birth_unit_normal(w))
                else:
                    assert ((X >= b.spec["lo"][d]) & (X <= b.spec["hi"][d])).all()
        zs.append(np.stack(row, axis=-1))
    z = np.stack(zs)
    assert z.shape == (3, T, W, 4)
    assert normal_stream_violations(normal_stream_stats(z, 0)) == []
    # two calls that differ in branch or parameter share no word
    a, b_ = rp.birth_words(seed, 0, T, W, 0, 0), rp.birth_words(seed, 0, T, W, 1, 0)
    assert not np.array_equal(a[0], b_[0])


def test_branches_take_a_container_in_place_of_a_box():
    from eryn_amd.prior import NormalDistribution, ProbDistContainer, log_uniform, uniform_dist
    from eryn_amd.rj import LeafBranch, TemplateBranch
    box = [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)]
    b0 = TemplateBranch("g", "pulse", box, 3)
    assert b0.is_box and b0.prior is None and np.array_equal(b0.terms["c0"], np.log(1 / (b0.hi - b0.lo)))
    uni = TemplateBranch("g", "pulse", {i: uniform_dist(*box[i]) for i in range(3)}, 3)
    assert uni.is_box and uni.leaf_logp == b0.leaf_logp and np.array_equal(uni.lo, b0.lo) and np.array_equal(uni.hi, b0.hi)
    mixed = {0: log_uniform(1.0, 7.0), 1: NormalDistribution(0.0, 0.35), 2: uniform_dist(0.01, 0.21)}
    for br in (TemplateBranch("g", "pulse", mixed, 3), TemplateBranch("g", "pulse", ProbDistContainer(mixed), 3), LeafBranch("g", mixed, 3)):
        assert not br.is_box and br.leaf_logp is None and br.ndim == 3
        assert br.terms["kind"].tolist() == [1, 2, 0] and br.lo[0] == 1.0 and br.hi[0] == 6.0          # (log_uniform(min, max): max - min)
        assert np.isneginf(br.lo[1]) and np.isposinf(br.hi[1])
    with pytest.raises(ValueError):
        TemplateBranch("g", "pulse", {0: uniform_dist(0, 1), 1: uniform_dist(0, 1)}, 3)
    try:
        from scipy import stats
    except ImportError:
        return
    sp = TemplateBranch("g", "pulse", {0: stats.loguniform(1.0, 6.0), 1: stats.norm(0.0, 0.35), 2: stats.uniform(0.01, 0.2)}, 3)
    assert sp.terms["kind"].tolist() == [1, 2, 0] and np.array_equal(sp.terms["c0"][:2], TemplateBranch("g", "pulse", mixed, 3).terms["c0"][:2])


def test_draw_births_is_each_parameters_own_rvs():
    """``RJEnsembleSampler._draw_births``: per parameter, in order, the distribution's ``rvs(nbirth)`` on the global stream - the
    oracle's ``TermBranch.rvs`` bit for bit; a box branch draws as before."""
    from eryn_amd.rj import RJEnsembleSampler, TemplateBranch
    for kind in KINDS:
        b = rp.branches_of((kind,), (3,), (0,))[0]
        dev = TemplateBranch(b.name, kind, b.container(), 3)
        np.random.seed(4)
        got = RJEnsembleSampler._draw_births(dev, 17)
        assert np.array_equal(got, b.rvs(17, np.random.RandomState(4))), kind
    box = TemplateBranch("g", "pulse", [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], 3)
    np.random.seed(4)
    got = RJEnsembleSampler._draw_births(box, 5)
    rs = np.random.RandomState(4)
    assert np.array_equal(got, np.stack([rs.rand(5) * (box.hi[d] - box.lo[d]) + box.lo[d] for d in range(3)], axis=1))


@pytest.mark.parametrize("name", sorted(rp.CASES))
def test_gpu_cases_are_sized(name):
    """The coverage conditions of the replayed cases, on the oracle with NumPy's draws, with a spare factor of 2: an accepted birth and
    an accepted death per branch, 5 % - 90 % of the in-model proposals with a -inf prior, 20 accept decisions a constant prior would
    have made differently."""
    cnt, knives = rp.oracle_case(name)
    rp.assert_coverage(cnt, 2, name)
    assert knives == 0
