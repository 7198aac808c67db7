"""The exact yardstick of the stepping kernels' log-likelihoods (tests/exact_quadratic.py) proven without a GPU:

* the long-double (or mpmath) value agrees with exact rational arithmetic to 2^-10 B;
* the float64 oracle is within B for every walker of every family, the edge set (on mu, 1e-160 sigma, 1e100 sigma) included - the
  worst ratio per family is printed;
* ``equicorr`` and ``spectrum`` cancel (median S / |L*| >= 1e5) and put the oracle itself further than ``RTOL_L`` from L*: why
  the suite's bar against the oracle cannot be applied there;
* two pure-NumPy models of a wrong kernel land above B;
* every stepping case of tests/test_hip_likelihood_accuracy.py, run through the oracle from L0 = -1e300 on its CPU-sized shape:
  every walker accepts in the first iteration and at least half of them accept again in the following ones."""
from fractions import Fraction

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import exact_quadratic as xq
from tests import parity_utils as pu
from tests import problems as pb
from tests import replay_utils as ru
from tests import tolerance_log as tol


def _walkers(prob):
    return prob.x0(2, 96).reshape(-1, prob.D)


@pytest.mark.parametrize("D", xq.WIDTHS)
@pytest.mark.parametrize("family", xq.FAMILIES)
def test_backend_agrees_with_exact_rational_arithmetic(family, D):
    prob = xq.make_problem(family, D)
    sets = [(prob, _walkers(prob)[[0, 1, 2, 50, 95]])]
    if prob.like_kind != "rosen":
        pe = xq.make_problem(family, D, edge=True)
        sets.append((pe, xq.edge_walkers(pe, 1)))                   # on mu, 1e-160 sigma, 1e100 sigma, an ordinary draw
    worst = Fraction(0)
    for p, x in sets:
        L, B, _ = xq.yardstick(p, x)
        for k in range(x.shape[0]):
            err = abs(xq.to_fraction(L[k]) - xq.exact_rational(p, x[k]))
            Bk = xq.to_fraction(B[k])
            assert err * 1024 <= Bk, f"{family} D={D} walker {k}: the backend is {float(err / Bk) if Bk else np.inf:.3g} B from the rational value"
            if Bk:
                worst = max(worst, err / Bk)
    print(f"{family} D={D}: backend vs rational at most {float(worst):.2e} B (bar 2^-10 = {2.0 ** -10:.2e})")


@pytest.mark.parametrize("family", xq.FAMILIES)
def test_oracle_is_within_the_bound(family):
    worst = 0.0
    for D in xq.WIDTHS:
        prob = xq.make_problem(family, D)
        sets = [(prob, _walkers(prob))]
        if prob.like_kind != "rosen":
            if prob.like_kind == "dense":
                # positive definite as the doubles stand (the form sees the symmetric part only; ``scaled`` inherits the last-bit
                # asymmetry of the benign matrix's inverse, which the packed forms A_ik + A_ki have to get right)
                np.linalg.cholesky(0.5 * (prob.precision + prob.precision.T))
            else:
                assert np.all(prob.precision > 0)
            pe = xq.make_problem(family, D, edge=True)
            sets.append((pe, xq.edge_walkers(pe)))
        for p, x in sets:
            assert np.all((x >= p.lo) & (x <= p.hi)), "the box never decides"
            L, B, _ = xq.yardstick(p, x)
            with np.errstate(under="ignore"):
                r = xq.error_ratio(p.loglike(x), L, B)
            assert r.max() <= 1.0, f"{family} D={D}: the float64 oracle is {r.max():.3g} B from L* (walker {int(r.argmax())})"
            worst = max(worst, float(r.max()))
    print(f"{family}: worst |L_oracle - L*| / B = {worst:.3g}")


@pytest.mark.parametrize("D", xq.WIDTHS)
@pytest.mark.parametrize("family", ["equicorr", "spectrum"])
def test_cancelling_families_are_beyond_the_oracle_bar(family, D):
    prob = xq.make_problem(family, D)
    x = _walkers(prob)
    L, B, canc = xq.yardstick(prob, x)
    rel = tol.max_rel(prob.loglike(x), L.astype(np.float64))
    print(f"{family} D={D}: median S / |L*| = {np.median(canc):.3g}, oracle vs L* {rel:.2e} relative (RTOL_L {tol.RTOL_L:.0e})")
    assert np.median(canc) >= 1e5
    assert rel > tol.RTOL_L


def test_benign_families_do_not_cancel():
    for family in ("scaled", "diag_scaled"):
        prob = xq.make_problem(family, 32)
        assert np.median(xq.yardstick(prob, _walkers(prob))[2]) < 10.0


class _Benign:
    like_kind = "dense"

    def __init__(self, D):
        self.D = D
        self.mu, self.precision = pu.gaussian_problem(D)


@pytest.mark.parametrize("model", [xq.model_expanded, xq.model_float32_block], ids=["expanded", "float32_block"])
def test_yardstick_has_teeth(model):
    """Both models of a wrong kernel land above B on every cancelling family (at least one is asked for).  On
    parity_utils.gaussian_problem the expanded form stays inside RTOL_L of the oracle - the suite's bar cannot see it on the
    targets it steps on.  The float32 block does NOT stay inside it there (some 1e-7: float32's 6e-8 is six decades over 1e-13 on
    any target), so the bar against the oracle does see that one; what the yardstick adds for it is the verdict on targets where
    that bar cannot be applied.  Both figures are printed."""
    above = {}
    for family in xq.DENSE_FAMILIES:
        for D in (16, 32, 64, 128):
            prob = xq.make_problem(family, D)
            x = _walkers(prob)
            L, B, _ = xq.yardstick(prob, x)
            above[family, D] = float(xq.error_ratio(model(prob, x), L, B).max())
    print({f"{f} D={D}": f"{v:.3g} B" for (f, D), v in above.items()})
    assert sum(v > 1.0 for v in above.values()) >= 1
    assert all(v > 1.0 for (f, D), v in above.items() if f in ("equicorr", "spectrum"))
    for D in (16, 32, 128):
        b = _Benign(D)
        x = np.random.RandomState(1).randn(256, D)                  # the suite's start positions on that problem
        ref = orc.gaussian_log_like(x, b.mu, b.precision)
        rel = tol.max_rel(model(b, x), ref)
        L, B, _ = xq.yardstick(b, x)
        print(f"gaussian_problem D={D}: {model.__name__} {rel:.2e} from the oracle (RTOL_L {tol.RTOL_L:.0e}), "
              f"{xq.error_ratio(model(b, x), L, B).max():.3g} B from L*")
        if model is xq.model_expanded:
            assert rel <= tol.RTOL_L
        else:
            assert rel > tol.RTOL_L and xq.error_ratio(model(b, x), L, B).max() > 1.0


# ---- coverage of the GPU cases, sized with the oracle alone ----------------------------------------------------------------------------
def _forced_run(prob, T, W, mh=None, seed=77, tempered=True):
    """(accepted in the first iteration [T, W], accepted in the following ones [T, W]) of a free oracle run from L0 = -1e300."""
    D = prob.D
    rs = np.random.RandomState(seed)
    x0 = prob.x0(T, W)
    P0 = orc.box_log_prior(x0.reshape(-1, D), prob.lo, prob.hi).reshape(T, W)
    assert np.isfinite(P0).all()
    st = ru.OracleState(x0, np.full((T, W), -1e300), P0, orc.make_ladder(D, ntemps=T) if T > 1 and tempered else None)
    first = None
    for it in range(sum(xq.STEPS)):
        d = xq.stretch_draws(rs, T, W)
        step = None
        if mh is not None and rs.rand() < 0.5:
            step = ((rs.randn(T * W, D) @ mh.T).reshape(T, W, D), rs.rand(T, W))
        ru.oracle_iteration(st, d, prob.loglike, prob.lo, prob.hi, mh=step)
        if it == 0:
            first = st.accepted + st.mh_accepted
    return first, st.accepted + st.mh_accepted - first


@pytest.mark.parametrize("cid,name,like,family", xq.production_cases(), ids=[c[0] for c in xq.production_cases()])
def test_production_case_is_covered(cid, name, like, family):
    c = pb.CASES[name]
    T, W, D = c["cpu_shape"] or (c["T"], c["W"], c["D"])
    prob = xq.make_problem(family, D)
    first, later = _forced_run(prob, T, W, mh=xq.mh_factor(prob) if c["mh"] else None, seed=c["seed"])
    share = float((later > 0).mean())
    print(f"{cid}: {T} x {W} x {D}: first iteration accepted by {first.mean():.3f}, {share:.3f} of the walkers accept again in {xq.STEPS[1]}")
    assert np.all(first == 1), "every walker accepts the first proposal from L0 = -1e300"
    assert share >= 0.5
