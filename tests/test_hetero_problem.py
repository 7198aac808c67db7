"""The heterogeneous problem family (tests/problems.py) does what the GPU cases built on it claim - without a GPU.

For every case of tests/test_hip_hetero_box.py the oracle runs free on NumPy draws of its own, on the same problem at the same
(T, W, D, iterations) (the config-2-size and the 64-rung case at reduced W), and the inputs are held to the coverage conditions:
the share of proposals with -inf prior inside ``problems.BAND``, every free (coordinate, side) the SOLE offender of at least 20
proposals - the GPU run, whose draws are others, asserts at least one, and at an expectation of 20 sees none with a probability
of about e^-20 per pair - and every pinned coordinate with accepted proposals exactly on its bound."""
import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import problems as pb
from tests import replay_utils as ru

EXPECTED_LEAST = 20


def _draws(rs, T, W, nsplits):
    """One iteration's draws in the reference's own form (red_blue.py:119-124, stretch.py:93-132, tempering.py:526-541)."""
    d = dict(labels=np.stack([rs.permutation(np.arange(W) % nsplits) for _ in range(T)]))
    for k in range(nsplits):
        Ns = (W - k + nsplits - 1) // nsplits
        d[f"rint{k}"] = rs.randint(W - Ns, size=(T, Ns))
        d[f"u_zz{k}"] = rs.rand(T, Ns)
        d[f"u_acc{k}"] = rs.rand(T, Ns)
    if T > 1:
        d["iperm"] = np.stack([rs.permutation(W) for _ in range(T - 1)])
        d["i1perm"] = np.stack([rs.permutation(W) for _ in range(T - 1)])
        d["u_swap"] = rs.rand(T - 1, W)
    return d


def free_run(c, prob):
    T, W, D = c["cpu_shape"] or (c["T"], c["W"], c["D"])
    rs = np.random.RandomState(c["seed"])
    x0 = prob.x0(T, W)
    P0 = orc.box_log_prior(x0.reshape(-1, D), prob.lo, prob.hi).reshape(T, W)
    assert np.isfinite(P0).all(), "x0 must lie inside the box: the reference refuses anything else"
    st = ru.OracleState(x0, prob.loglike(x0.reshape(-1, D)).reshape(T, W), P0, orc.make_ladder(D, ntemps=T) if T > 1 else None)
    cov = pb.new_coverage(D)
    mh = pb.mh_proposal(prob, *c["mh"]) if c["mh"] else None
    for _ in range(sum(c["calls"])):
        d = _draws(rs, T, W, c["nsplits"])
        step = None
        if mh is not None and rs.rand() < mh[2]:
            z = rs.randn(T * W, D)
            step = (z * mh[1] if mh[0] == "iso" else z @ mh[1].T, rs.rand(T, W))
        ru.oracle_iteration(st, d, prob.loglike, prob.lo, prob.hi, mh=step, period=prob.period, nsplits=c["nsplits"], coverage=cov)
    return st, cov


@pytest.mark.parametrize("name", sorted(pb.CASES))
def test_case_reaches_its_coverage_in_expectation(name):
    c = pb.CASES[name]
    prob = pb.case_problem(c)
    st, cov = free_run(c, prob)
    pb.assert_coverage(cov, prob, least=EXPECTED_LEAST, what=name)
    assert st.accepted.sum() + st.mh_accepted.sum() > 0 and (c["T"] == 1 or st.swaps_total.sum() > 0)
    if c["mh"]:
        assert cov["mh"] > 0 and cov["stretch"] > 0 and st.mh_accepted.sum() > 0


@pytest.mark.parametrize("D", [5, 8, 11, 12, 16, 32, 64, 70, 128])
@pytest.mark.parametrize("like", ["dense", "diag", "rosen"])
def test_problem_is_heterogeneous_and_well_conditioned(D, like):
    p = pb.hetero_problem(D, like, pinned=like != "rosen")
    both = np.concatenate([p.lo, p.hi])
    assert np.unique(both).size == 2 * D and np.all(p.lo < p.hi), "every bound of the problem is a number of its own"
    x0 = p.x0(3, 40)
    assert np.all((x0 >= p.lo) & (x0 <= p.hi))
    for d, side in p.pinned.items():
        assert np.all(x0[..., d] == (p.lo[d] if side == "lo" else p.hi[d]))
    if like == "rosen":
        assert not p.pinned and np.all((np.abs(both) >= 3.0) & (np.abs(both) <= 6.0))
        return
    assert 0 not in p.pinned and {d % 2 for d in p.pinned} == {0, 1} and min(p.pinned) < D // 2 <= max(p.pinned)
    assert np.log10((p.hi - p.lo).max() / (p.hi - p.lo).min()) > 2.0, "scales over decades"
    # conjugated by 1 / s the precision is the benign one again: as well conditioned, relative to its scales
    mu0, inv0 = pb.pu.gaussian_problem(D, dense=(like == "dense"))
    s = 1.0 / np.sqrt(np.diag(p.precision) / np.diag(inv0)) if like == "dense" else 1.0 / np.sqrt(p.precision / np.diag(inv0))
    back = p.precision * np.outer(s, s) if like == "dense" else p.precision * s * s
    np.testing.assert_allclose(back, inv0 if like == "dense" else np.diag(inv0), rtol=1e-12)


def test_default_problem_is_untouched():
    """the default problem of every existing test: parity_utils.gaussian_problem / make_oracle without ``problem=``"""
    from tests import parity_utils as pu
    o, mu, invcov = pu.make_oracle(2, 8, 4)
    mu1, inv1 = pu.gaussian_problem(4)
    assert np.array_equal(mu, mu1) and np.array_equal(invcov, inv1)
    assert np.array_equal(o.lo, np.full(4, -50.0)) and np.array_equal(o.hi, np.full(4, 50.0))
    assert np.array_equal(o.x, np.random.RandomState(1).randn(2, 8, 4))
