"""Periodic leaf parameters on leaf-packing records, without a GPU: the specification (tests/rj_periodic.py) against the chains
captured from the reference (tests/golden/make_golden_rj_periodic.py -> tests/golden/rj_periodic/) - every proposal q (dead slots
included), mask and coordinate bit for bit, L to the bar the corresponding specification tests use, P exactly; ``distance`` / ``wrap``
at the seam against exact arithmetic; what the fixtures were made to exercise; the sampler's ``periodic`` parsing and its refusals;
the C surface."""
import os
import re

import numpy as np
import pytest

from tests import periodic_seam as ps
from tests import rj_periodic as rp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL_L = 1e-12          # the bar tests/test_rj_group_move.py and tests/test_rj_gibbs_move.py hold the oracle's template sum to
TWO_PI = rp.TWO_PI


def _close(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert np.all(np.abs(a - b) <= RTOL_L * np.abs(b)), f"{what}: max rel {np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)):.3e}"


def _same(a, b):
    return ps.same_bits(a, b)


def proposals_of(rec, kind, names):
    """A recorded iteration's proposals in the fixtures' order -> list of dict(q, keep, u_acc[, u_zz, pick])."""
    if kind == "gaussian":
        return [dict(q=rec["mh_q"], keep=rec["mh_accepted"], u_acc=rec["mh_u_acc"])]
    if kind == "stretch":
        return [dict(q=rec[f"st_q{s}"], keep=rec[f"st_keep{s}"], u_acc=rec[f"st_u_acc{s}"], u_zz=rec[f"st_u_zz{s}"]) for s in range(2)]
    if kind == "group":
        return [dict(q=rec["q"], keep=rec["mh_accepted"], u_acc=rec["u_acc"], u_zz=rec["u_zz"], pick=rec["picks"], start=rec["start"],
                     act={k: rec[f"pre_inds_{k}"] for k in names})]
    return [dict(q=r["q"], keep=r["accepted"], u_acc=r["u_acc"]) for r in rec["gibbs"]]


@pytest.mark.parametrize("name", rp.FIXTURES)
def test_specification_lands_on_the_reference(name):
    fx = rp.load_fixture(name)
    o = rp.fixture_oracle(fx)
    kind = str(fx["in_model"])
    names = [b.name for b in o.branches]
    assert np.array_equal(o.st.P, fx["P0"])
    _close(o.st.L, fx["L0"], "initial log-like")
    for it in range(int(fx["nsteps"])):
        o.iteration()
        rec = o.trace.pop()
        props = proposals_of(rec, kind, names)
        assert len(props) == int(fx[f"it{it}_nprop"]), f"{name} it{it}: proposals"
        for j, p in enumerate(props):
            pre = f"it{it}_p{j}_"
            for k in names:
                assert _same(p["q"][k], fx[pre + f"q_{k}"]), f"{name} {pre}: proposal of {k}, dead slots included"
                if "pick" in p:
                    assert np.array_equal(p["pick"][k][p["act"][k]], fx[pre + f"pick_{k}"][p["act"][k]]), f"{name} {pre}: picks of {k}"
                    assert np.array_equal(p["start"][k], fx[pre + f"start_{k}"]), f"{name} {pre}: windows of {k}"
            assert np.array_equal(p["keep"], fx[pre + "keep"]), f"{name} {pre}: accept mask"
            assert np.array_equal(p["u_acc"], fx[pre + "u_acc"]), f"{name} {pre}: R's order"
            if "u_zz" in p:
                assert np.array_equal(p["u_zz"], fx[pre + "u_zz"]), f"{name} {pre}: zz's uniforms"
        for k in names:
            assert _same(rec[f"mh_x_{k}"], fx[f"it{it}_mh_x_{k}"]) and np.array_equal(rec[f"mh_inds_{k}"], fx[f"it{it}_mh_inds_{k}"]), f"{name} it{it}: state behind the sweep, {k}"
            assert _same(o.st.x[k], fx[f"it{it}_rj_x_{k}"]) and np.array_equal(o.st.inds[k], fx[f"it{it}_rj_inds_{k}"]), f"{name} it{it}: state behind birth / death, {k}"
        assert np.array_equal(rec["mh_P"], fx[f"it{it}_mh_P"]) and np.array_equal(o.st.P, fx[f"it{it}_rj_P"])
        _close(rec["mh_L"], fx[f"it{it}_mh_L"], f"{name} it{it}: log-like behind the sweep")
        _close(o.st.L, fx[f"it{it}_rj_L"], f"{name} it{it}: log-like behind birth / death")
        assert np.array_equal(rec["mh_accepted"], fx[f"it{it}_mh_accepted"]) and np.array_equal(rec["rj_accepted"], fx[f"it{it}_rj_accepted"])
        np.testing.assert_allclose(o.st.betas, fx[f"it{it}_rj_betas"], rtol=1e-13, atol=0)
    assert np.array_equal(o.mh_accepted, fx["mh_accepted_total"])
    # the specification saw at the seam what the reference's own calls saw
    f = o.facts.as_dict()
    for k, v in f.items():
        assert v == int(fx["facts_" + k]), f"{name}: {k} {v}, the reference {int(fx['facts_' + k])}"


@pytest.mark.parametrize("name", rp.FIXTURES)
def test_fixtures_hold_the_cases_they_were_made_for(name):
    fx = rp.load_fixture(name)
    kind = str(fx["in_model"])
    assert (int(fx["T"]), int(fx["W"]), int(fx["ndata"]), int(fx["nsteps"])) == (3, 8, 40, 8)
    assert np.array_equal(fx["period_gauss"], np.zeros(3)) and np.array_equal(fx["period_sine"], [0.0, 0.0, TWO_PI])
    ph, act = fx["x0_sine"][..., 2], fx["inds0_sine"]
    a, d = ph[act], ph[~act]
    assert np.any(a < 0.06) and np.any(a > TWO_PI - 0.06) and np.all((a < 0.06) | (a > TWO_PI - 0.06)), "active phases on both sides of the seam"
    assert np.any(d < 0.0) and np.any(d >= TWO_PI) and np.any(d > 5 * TWO_PI), "dead phases outside [0, 2 pi)"
    assert fx["facts_wrapped_accepts"] >= 1 and fx["facts_dead_changed"] >= 1 and fx["facts_rejected"] >= 1 and fx["facts_knife"] == 0
    if kind in ("stretch", "group"):
        assert fx["facts_short_way"] >= 1
    if kind == "gaussian":
        c = fx["cov_sine"]
        assert not np.array_equal(c, np.diag(np.diag(c))), "a full leaf covariance"
        assert str(fx["rj_moves"]) == "together"
    if kind == "gibbs":
        assert "sine_prior_kind" in fx and set(fx["sine_prior_kind"].tolist()) != {0}, "non-uniform prior terms"
    for k in ("gauss", "sine"):
        assert os.path.getsize(os.path.join(rp.HERE, "golden", "rj_periodic", name + ".npz")) <= 150164      # the largest rj_group fixture


def test_without_periods_the_specification_is_the_oracle():
    """Periods of zero: the same chain as the pinned oracle, bit for bit."""
    from oracle import eryn_oracle_rj as orj
    fx = rp.load_fixture("rjp_gauss")
    brs = rp.fixture_branches(fx)
    outs = []
    for cls in (None, rp.PeriodicOracle):
        R, G = np.random.RandomState(3), np.random.RandomState(4)
        args = (brs, {b.name: fx[f"x0_{b.name}"] for b in brs}, {b.name: fx[f"inds0_{b.name}"] for b in brs}, fx["t"], fx["y"], float(fx["sigma"]),
                R, G, fx["betas0"])
        o = orj.OracleRJSampler(*args, schedule="together") if cls is None else cls({b.name: np.zeros(3) for b in brs}, *args, schedule="together")
        for _ in range(4):
            o.iteration()
        outs.append(o.st)
    for k in outs[0].x:
        assert _same(outs[0].x[k], outs[1].x[k])
    assert _same(outs[0].L, outs[1].L) and _same(outs[0].P, outs[1].P)


def test_distance_and_wrap_are_the_values_the_reference_recorded_at_the_seam():
    """tests/golden/periodic/seam.npz holds what the reference's own ``PeriodicContainer.distance`` / ``wrap`` returned on the seam
    matrix of every period family (tests/golden/make_golden_periodic.py): differences of exactly half a period, +-0.0, multiples of the
    period, points up to 2^52 periods out.  The specification's functions give the same bits."""
    with np.load(os.path.join(rp.HERE, "golden", "periodic", "seam.npz"), allow_pickle=False) as f:
        fams = 0
        while f"m{fams}_period" in f.files:
            period, pairs, q = float(f[f"m{fams}_period"]), f[f"m{fams}_pairs"], f[f"m{fams}_q"]
            per = np.array([period])
            with np.errstate(over="ignore", invalid="ignore"):
                d = rp.distance(pairs[:, :1], pairs[:, 1:], per)[:, 0]
            assert _same(d, f[f"m{fams}_distance"]), f"distance, period {period}"
            assert _same(rp.wrap(q[:, None], per)[:, 0], f[f"m{fams}_wrap"]), f"wrap, period {period}"
            if period > 0:
                half = np.abs(pairs[:, 1] - pairs[:, 0]) == period / 2.0
                zeros = (pairs == 0.0).any(axis=1)
                mult = (q != 0.0) & (f[f"m{fams}_wrap"] == 0.0)
                assert half.any() and zeros.any() and np.signbit(pairs[zeros]).any() and mult.any() and (np.abs(q) > 1e6 * period).any()
            fams += 1
        assert fams == 6


# ---- distance / wrap at the seam --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [TWO_PI, 1.0, 1.5])
def test_distance_and_wrap_at_the_seam_are_exact(period):
    """tests/periodic_seam.py's matrix - differences of exactly half a period, +-0.0, multiples of the period, points many periods
    out - against exact arithmetic on the reference's masked-sum form, bit for bit."""
    pairs, qs = ps.edge_matrix(period)
    want_d, want_w = ps.exact_matrix(period, form="masked")
    per = np.array([0.0, period])
    s = np.stack([pairs[:, 0], pairs[:, 0]], axis=-1)
    c = np.stack([pairs[:, 1], pairs[:, 1]], axis=-1)
    with np.errstate(over="ignore", invalid="ignore"):
        got = rp.distance(s, c, per)
    assert _same(got[:, 1], want_d), "distance on the periodic parameter"
    assert _same(got[:, 0], pairs[:, 1] - pairs[:, 0]), "c - s on the other one"
    w = rp.wrap(np.stack([qs, qs], axis=-1), per)
    assert _same(w[:, 1], want_w) and _same(w[:, 0], qs)
    half = period / 2.0
    assert rp.distance(np.array([0.0]), np.array([half]), np.array([period]))[0] == half, "exactly half a period: the long way stays"
    assert _same(rp.wrap(np.array([[-0.0], [3 * period], [-2 * period]]), np.array([period])), np.zeros((3, 1))), "+0.0 for -0.0 and for multiples"
    far = 40.0 * period + 0.25
    assert 0.0 <= rp.wrap(np.array([far]), np.array([period]))[0] < period


def test_reference_values_recorded_at_the_seam():
    """The recorded chains hold the cases themselves: a dead slot many periods out lands in [0, 2 pi) with the first accepted
    Gaussian proposal of its walker, and its new bits are NumPy's remainder of the old ones."""
    fx = rp.load_fixture("rjp_gauss")
    x0, q, keep = fx["x0_sine"], fx["it0_p0_q_sine"], fx["it0_p0_keep"]
    dead = ~fx["inds0_sine"]
    far = dead & (x0[..., 2] > 5 * TWO_PI)
    assert far.any()
    assert _same(q[..., 2][far], x0[..., 2][far] % TWO_PI)
    neg = dead & (x0[..., 2] < 0)
    assert neg.any() and _same(q[..., 2][neg], x0[..., 2][neg] % TWO_PI) and np.all(q[..., 2][neg] > 0)
    # an accepted walker's record carries the wrapped dead slot (the state behind the move, before the swaps permute the walkers)
    o = rp.fixture_oracle(fx)
    o.iteration()
    rec = o.trace[0]
    acc = rec["mh_accepted"]
    assert _same(rec["mhupd_x_sine"][acc], q[acc]) and (acc[:, :, None] & far).any()


@pytest.mark.parametrize("name", sorted(rp.PRODUCTION_CASES))
def test_production_cases_are_sized(name):
    """The starts of the replayed production cases (tests/test_hip_rj_periodic.py), on the specification alone with NumPy's draws: 12
    iterations see wrapped accepts and rejections, the stretch-type moves short-way-round differences."""
    p = rp.production_problem(name)
    o = rp.production_oracle(p, R=np.random.RandomState(1), G=np.random.RandomState(2))
    act = p["inds"][p["branches"][-1].name]
    ph = p["x"][p["branches"][-1].name][..., 2]
    assert np.all((ph[act] < 0.1) | (ph[act] > TWO_PI - 0.1)) and np.all((ph[~act] < 0) | (ph[~act] >= TWO_PI))
    for _ in range(rp.PRODUCTION_ITERS):
        o.iteration()
    f = o.facts.as_dict()
    print(name, f)
    assert f["wrapped_accepts"] >= 5 and f["rejected"] >= 5 and f["dead_changed"] >= 1
    if p["move"] in ("stretch", "group"):
        assert f["short_way"] >= 5
    if name == "record_past_64":
        assert sum(b.nleaves_max * b.ndim for b in p["obr"]) == 72


# ---- the Python surface -------------------------------------------------------------------------------------------------------------------------
def _branches():
    from eryn_amd.rj import TemplateBranch
    return [TemplateBranch("gauss", "pulse", [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], 4), TemplateBranch("sine", "sine", [(0.5, 1.5), (1.0, 20.0), (0.0, TWO_PI)], 2)]


def test_periodic_parsing():
    from eryn_amd.periodic import PeriodicContainer
    from eryn_amd.rj import leaf_periods
    brs = _branches()
    want = [np.zeros(3), np.array([0.0, 0.0, TWO_PI])]
    for spec in ({"sine": {2: TWO_PI}}, {"gauss": {}, "sine": {2: TWO_PI}}, {"gauss": None, "sine": {2: TWO_PI}},
                 PeriodicContainer({"gauss": {}, "sine": {2: TWO_PI}}), [None, [0.0, 0.0, TWO_PI]]):
        rows = leaf_periods(spec, brs)
        assert len(rows) == 2 and all(np.array_equal(a, b) for a, b in zip(rows, want)), spec
    for spec in (None, {}, {"gauss": {}}, {"gauss": None, "sine": {}}, [None, None]):
        assert leaf_periods(spec, brs) is None, spec

    class TheirContainer:                      # the reference's container: the same two dictionaries
        inds_periodic = {"gauss": np.asarray([]), "sine": np.asarray([2])}
        periods = {"gauss": np.asarray([]), "sine": np.asarray([TWO_PI])}
    rows = leaf_periods(TheirContainer(), brs)
    assert np.array_equal(rows[1], want[1]) and np.array_equal(rows[0], want[0])
    with pytest.raises(ValueError):
        leaf_periods({"sine": {3: 1.0}}, brs)
    with pytest.raises(ValueError):
        leaf_periods({"sine": {2: -1.0}}, brs)
    with pytest.raises(ValueError):
        leaf_periods({"chirp": {0: 1.0}}, brs)
    with pytest.raises(ValueError):
        leaf_periods(3.0, brs)


def test_moves_carry_a_periodic_argument():
    from eryn_amd import rj
    cov = {"gauss": np.eye(3), "sine": np.eye(3)}
    per = {"sine": {2: TWO_PI}}
    for mv in (rj.GaussianLeafMove(cov, periodic=per), rj.GibbsGaussianLeafMove(cov, ["gauss", "sine"], periodic=per),
               rj.StretchLeafMove(periodic=per), rj.GroupStretchLeafMove(3, 1, periodic=per)):
        assert mv.periodic is per
    for mv in (rj.GaussianLeafMove(cov), rj.StretchLeafMove(), rj.GroupStretchLeafMove(3, 1)):
        assert mv.periodic is None
    assert "periodic parameters" not in rj.GroupStretchLeafMove.__doc__.split("Not built")[1]


def test_sampler_takes_periodic_and_refuses_a_move_that_disagrees():
    """``periodic`` is a named argument in front of ``**unused``; a move whose own ``periodic`` says something else is refused before
    the sampler touches a device."""
    import inspect
    from eryn_amd import rj
    sig = inspect.signature(rj.RJEnsembleSampler.__init__)
    assert "periodic" in sig.parameters and sig.parameters["periodic"].default is None
    assert list(sig.parameters).index("periodic") < list(sig.parameters).index("unused")
    t = np.linspace(-1, 1, 8)
    like = rj.TemplateLikelihood({"gauss": "pulse", "sine": "sine"}, t, np.zeros(8), 1.0)
    priors = {"gauss": [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], "sine": [(0.5, 1.5), (1.0, 20.0), (0.0, TWO_PI)]}
    kw = dict(tempering_kwargs=dict(ntemps=2), branch_names=["gauss", "sine"], nleaves_max={"gauss": 2, "sine": 2})
    cov = {"gauss": np.eye(3), "sine": np.eye(3)}
    for mine, theirs in (({"sine": {2: 1.0}}, {"sine": {2: TWO_PI}}), ({"sine": {2: TWO_PI}}, None), ({"gauss": {1: 2.0}}, {"sine": {2: TWO_PI}})):
        for mv in (rj.GaussianLeafMove(cov, periodic=mine), rj.StretchLeafMove(periodic=mine), rj.GroupStretchLeafMove(3, 1, periodic=mine),
                   rj.GibbsGaussianLeafMove(cov, ["gauss", "sine"], periodic=mine)):
            with pytest.raises(ValueError, match="the move's periodic differs from the sampler's"):
                rj.RJEnsembleSampler(8, {"gauss": 3, "sine": 3}, like, priors, moves=mv, periodic=theirs, **kw)
    with pytest.raises(ValueError, match="out of range"):
        rj.RJEnsembleSampler(8, {"gauss": 3, "sine": 3}, like, priors, moves=rj.StretchLeafMove(), periodic={"sine": {3: 1.0}}, **kw)
    assert rj._same_periods(None, None) and not rj._same_periods(None, [np.zeros(3)])
    a = rj.leaf_periods({"sine": {2: TWO_PI}}, _branches())
    assert rj._same_periods(a, rj.leaf_periods({"gauss": {}, "sine": {2: TWO_PI}}, _branches()))


def test_c_surface():
    with open(os.path.join(ROOT, "include", "hipensemble.h")) as f:
        h = f.read()
    assert "int hens_rj_set_periodic(hens_ctx* ctx, const double* period);" in h
    assert "hens_rj_set_periodic" in h.split("int hens_set_periodic(")[0].rsplit("hens_set_periodic:", 1)[1], "hens_set_periodic's comment points to the new call"
    with open(os.path.join(ROOT, "eryn_amd", "_lib.py")) as f:
        assert '"hens_rj_set_periodic": (C.c_int, [_P, _P])' in f.read()
