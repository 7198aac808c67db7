"""The leaf kinds of hens_rj_set_model_kinds on the CPU: the NumPy statement the GPU tests measure against (tests/leaf_kinds.py)
is the oracle's likelihoods bit for bit; it lies within the a-priori float64 bound B of exact arithmetic (tests/exact_leaf_kinds.py)
and B is small against L* on the accuracy cases, so the GPU tests' 4 B bar is a finer one than their rtol 1e-12 bar; the host side
of eryn_amd.rj knows the kinds' widths."""
import numpy as np
import pytest

from oracle import eryn_oracle_rj as orj
from tests import exact_leaf_kinds as xk
from tests import leaf_kind_cases as cases
from tests import leaf_kinds as lk

ORACLE_FN = {"lorentz_chirp": orj.lorentz_chirp_log_like, "ramp_burst": orj.ramp_burst_log_like, "offset": orj.offset_log_like}


@pytest.mark.parametrize("seed", [1, 2, 3])
@pytest.mark.parametrize("model", sorted(ORACLE_FN))
def test_helper_is_the_oracle_bit_for_bit(model, seed):
    """The reference's per-walker calling convention (oracle: callable_log_like): a list over the branches of the walker's active
    leaves or None - with one model type the leaves themselves -, walkers without a leaf or outside the prior not evaluated."""
    kinds = cases.MODELS[model]
    brs = cases.branches_of(kinds, (4, 3)[:len(kinds)] if len(kinds) > 1 else (5,))
    rs = np.random.RandomState(seed)
    T, W = 3, 7
    x, inds = cases.random_state(brs, T, W, rs)
    for b in brs:
        inds[b.name][0, 0] = False                               # a walker without any leaf
    if len(brs) > 1:
        inds[brs[-1].name][1, 2] = False                         # leaves in the first branch only
        inds[brs[0].name][1, 2, 0] = True
        inds[brs[0].name][2, 1] = False                          # ... in the last only
        inds[brs[-1].name][2, 1, 0] = True
    else:
        inds[brs[0].name][1, 2] = [True] + [False] * (brs[0].nleaves_max - 1)      # a single leaf
    t = np.linspace(-1, 1, 25)
    y, sigma = np.sin(7 * t), 0.7
    logp = rs.randn(T, W)
    logp[2, 3] = -np.inf                                         # outside the prior: not evaluated
    obr = [b.to_oracle() for b in brs]
    want = orj.compute_log_like(x, inds, logp, obr, t, y, sigma, like_fn=ORACLE_FN[model])
    got = orj.compute_log_like(x, inds, logp, obr, t, y, sigma, like_fn=lk.like_fn(kinds))
    assert np.array_equal(got, want)
    assert got[0, 0] == -1e300 and got[2, 3] == -1e300
    ev = want != -1e300
    any_leaf = np.any([inds[b.name].any(axis=-1) for b in brs], axis=0)
    assert np.array_equal(ev, any_leaf & ~np.isinf(logp)) and ev[1, 2] and ev.sum() >= T * W - 4
    full = lk.template_log_like(brs, x, inds, t, y, sigma)       # every walker at once: the same values where the oracle evaluates
    assert np.array_equal(full[ev], want[ev])
    assert full[0, 0] == -0.5 * np.sum(((np.zeros_like(t) - y) / sigma) ** 2)


@pytest.mark.parametrize("model,grid", cases.ACCURACY_CASES)
def test_helper_within_B_of_exact_and_B_small_against_L(model, grid):
    c = cases.accuracy_case(model, grid)
    args = (c["branches"], c["x"], c["inds"], c["t"], c["y"], c["sigma"])
    L = lk.template_log_like(*args)
    Ls, B = xk.yardstick(*args)
    assert np.isfinite(L).all() and np.all(B > 0)
    ratio = np.abs(L - Ls) / B
    rel = B / np.abs(Ls)
    print(f"{model} on {grid}: float64 helper max |L - L*| / B = {ratio.max():.3g}, max B / |L*| = {rel.max():.3g}")
    assert np.all(ratio <= 1.0), f"float64 evaluation outside its own bound: {ratio.max():.3g} B"
    assert np.all(rel < 1e-12), f"B / |L*| = {rel.max():.3g}: the 4 B bar would be weaker than rtol 1e-12"


def test_every_new_kind_has_an_accuracy_case():
    seen = {k for m, _ in cases.ACCURACY_CASES for k in cases.MODELS.get(m, (m,))}
    assert {"offset", "ramp", "lorentz", "chirp", "burst"} <= seen
    for grid in cases.GRIDS:
        assert any(g == grid for _, g in cases.ACCURACY_CASES)


def test_exact_backends_agree_on_every_kind():
    """The check of the check: long double against mpmath at 40 digits on one walker per kind (where both exist)."""
    try:
        import mpmath  # noqa: F401
    except ImportError:
        return                                                   # (one backend: nothing to compare)
    if xk.xt.backend() != "longdouble":
        return                                                   # (np.longdouble is no finer than double here: mpmath is the backend already)
    for model in ("lorentz_chirp", "ramp_burst", "offset"):
        c = cases.accuracy_case(model, "control_40")
        x = {k: v[:1, 2:4] for k, v in c["x"].items()}
        inds = {k: v[:1, 2:4] for k, v in c["inds"].items()}
        a, Ba = xk.yardstick(c["branches"], x, inds, c["t"], c["y"], c["sigma"], use="longdouble")
        b, Bb = xk.yardstick(c["branches"], x, inds, c["t"], c["y"], c["sigma"], use="mpmath")
        assert np.all(np.abs(a - b) <= 2e-16 * np.abs(b)) and np.allclose(Ba, Bb, rtol=1e-6)


def test_host_side_knows_the_kinds():
    from eryn_amd.rj import LEAF_KINDS, TemplateBranch, TemplateLikelihood
    assert LEAF_KINDS == {"pulse": (0, 3), "sine": (1, 3), "offset": (2, 1), "ramp": (3, 2), "lorentz": (4, 3), "chirp": (5, 3), "burst": (6, 4)}
    assert LEAF_KINDS == lk.KINDS
    for kind, (kid, width) in LEAF_KINDS.items():
        b = TemplateBranch("b", kind, cases.BOX[kind], 3, 1)
        assert (b.kind, b.ndim, b.lo.shape, b.nleaves_max, b.nleaves_min) == (kid, width, (width,), 3, 1)
    assert TemplateBranch("g", "gauss", cases.BOX["pulse"], 2).kind == 0            # (the reference tests' name for the pulse)
    with pytest.raises(ValueError):
        TemplateBranch("r", "ramp", [(0, 1)] * 3, 2)
    with pytest.raises(ValueError):
        TemplateBranch("p", "pulse", [(0, 1)] * 4, 2)
    with pytest.raises(KeyError):
        TemplateBranch("w", "wavelet", [(0, 1)] * 3, 2)
    like = TemplateLikelihood({"ramp": "ramp", "burst": "burst"}, np.zeros(3), np.zeros(3), 1.0)
    assert like.kinds == {"ramp": 3, "burst": 6}
    with pytest.raises(KeyError):
        TemplateLikelihood({"w": "wavelet"}, np.zeros(3), np.zeros(3), 1.0)


@pytest.mark.parametrize("kind", ["offset", "ramp", "lorentz", "chirp", "burst"])
def test_leaf_logp_is_accumulated_in_the_reference_order(kind):
    """prior.py:364-383: ``prior_vals += temp`` parameter by parameter from 0.0 - the oracle's leaf_logpdf of a leaf inside the box."""
    from eryn_amd.rj import TemplateBranch
    box = [(lo - 0.1 * (d + 1), hi + 0.37 * (d + 3)) for d, (lo, hi) in enumerate(cases.BOX[kind])]      # (widths whose logs do not sum exactly)
    b = TemplateBranch("b", kind, box, 2)
    ob = orj.Branch("b", 0, box, 2)
    mid = np.array([[0.5 * (lo + hi) for lo, hi in box]])
    assert b.leaf_logp == ob.leaf_logpdf(mid)[0]
