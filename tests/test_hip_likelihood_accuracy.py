"""The log-likelihoods of the fixed-dimension stepping kernels against exact arithmetic (-m gpu), not against the float64 oracle.

Every other test holds them to the oracle at ``RTOL_L`` = 1e-13, which can only be done on targets where the oracle's own rounding
is far below that - targets on which nothing cancels in the quadratic form.  Here the targets are the families of
tests/exact_quadratic.py (an equicorrelated covariance with rho = 1 - 2^-20, a spectrum over ten decades, scales over twelve
decades with means 10^3 ... 10^6 sigma from 0, the Rosenbrock valley), the referee is L* computed in long double from the very
doubles the device holds, and the bar is the a-priori bound B of any float64 evaluation (tests/test_exact_quadratic.py proves
both on the CPU).  For every walker |L_dev - L*(x_dev)| <= 1.0 B(x_dev), x_dev the downloaded position: no draws are replayed and no
knife edge can interfere.  A non-finite L_dev fails (no walker here is outside its box - +- 1e4 sigma around mu, +- 1e120 sigma for
the edge set, +- 20 for the Rosenbrock valley - and every case asserts that from the downloaded log-prior).

Device paths, each at the smallest shape that selects it (shapes, switches and keyword arguments from tests/problems.CASES):
  eval        eval_state at every row-width class, every family of the kind, plus the edge set: a walker exactly on mu, walkers at
              1e-160 sigma (every product underflows) and at 1e100 sigma
  split       teacher-forced stretch_split from L = -1e300 with u_acc = 1e-300: every proposal is accepted, every stored L is
              the stretch kernel's evaluation of a proposal
  mh          mh_step with steps drawn from 0.02 Sigma, likewise
  production  hens_step from L = -1e300: after step(1) the counters say every walker accepted exactly once - every stored L was
              written by the stepping kernels under test - compare, step(5), compare again
Each case prints the worst |L_dev - L*| / B, the same ratio for the oracle evaluated at x_dev and the median S / |L*|; all of them
go to likelihood_accuracy_report.json in the directory HENS_REPORT_DIR names (default: build/reports; a copy of the MI355X run
is kept as profiles/likelihood_accuracy_report.json).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import exact_quadratic as xq
from tests import parity_utils as pu
from tests import problems as pb
from tests.test_hip_hetero_box import _child_env

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BAR = 1.0
_report = []


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    if not _report:
        return
    paths = {}
    for e in _report:
        p = paths.setdefault(e["path"], {"device": 0.0, "oracle": 0.0, "walkers": 0})
        p["device"], p["oracle"] = max(p["device"], e["device"]), max(p["oracle"], e["oracle"])
        p["walkers"] += e["walkers"]
    out = os.environ.get("HENS_REPORT_DIR") or os.path.join(ROOT, "build", "reports")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "likelihood_accuracy_report.json"), "w") as f:
        json.dump({"bar": BAR, "worst_ratio_per_path": paths, "cases": _report}, f, indent=1)


def compare(prob, x, L, P, path, what, bad):
    """One downloaded state against the yardstick: prints and records the ratios, appends to ``bad`` what is over the bar."""
    D = prob.D
    x2, L1 = x.reshape(-1, D), L.reshape(-1)
    assert np.isfinite(P).all(), f"{what}: a walker outside its box (the box is meant never to decide)"
    Ls, B, canc = xq.yardstick(prob, x2)
    dev = xq.error_ratio(L1, Ls, B)
    with np.errstate(under="ignore"):
        orac = xq.error_ratio(prob.loglike(x2), Ls, B)
    k = int(np.argmax(dev))
    e = dict(path=path, case=what, walkers=int(L1.size), device=float(dev[k]), oracle=float(orac.max()),
             median_S_over_L=float(np.median(canc)))
    _report.append(e)
    print(f"{what}: {L1.size} walkers, worst |L_dev - L*| / B = {e['device']:.3g}, oracle {e['oracle']:.3g}, median S / |L*| = "
          f"{e['median_S_over_L']:.3g}")
    if not dev[k] <= BAR:
        bad.append(f"{what}: walker {k}: L_dev = {L1[k]!r}, L* = {float(Ls[k])!r}: {dev[k]:.3g} B; {int((dev > BAR).sum())} walkers over the bar")
    return e


def _engine(prob, T, W, pad=True, seed=1, **kw):
    from eryn_amd.engine import HipEnsemble
    return HipEnsemble(T, W, prob.D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=seed, pad_rows=pad, **kw)


def _forced_upload(eng, prob, x, T, W):
    """the state with L = -1e300: whatever is proposed inside the box is accepted"""
    eng.upload(x, np.full((T, W), -1e300), np.full((T, W), eng.logp_inside), orc.make_ladder(prob.D, ntemps=T) if T > 1 else None)


WIDTH_IDS = [f"D{D}" + ("" if pad else "_generic") for D, pad in xq.EVAL_WIDTHS]


@pytest.mark.parametrize("like", ["dense", "diag", "rosen"])
@pytest.mark.parametrize("D,pad", xq.EVAL_WIDTHS, ids=WIDTH_IDS)
def test_eval_state_within_B_of_exact(D, pad, like):
    bad = []
    for family in xq.families_of(like):
        prob = xq.make_problem(family, D)
        T, W = xq.PARITY_T, xq.parity_walkers(D)
        sets = [(prob, prob.x0(T, W), "")]
        if like != "rosen":
            pe = xq.make_problem(family, D, edge=True)
            xe = xq.edge_walkers(pe)
            sets.append((pe, xe[None], " edge set"))
        for p, x, tag in sets:
            Tn, Wn = x.shape[:2]
            eng = _engine(p, Tn, Wn, pad)
            try:
                eng.upload(x, betas=orc.make_ladder(D, ntemps=Tn) if Tn > 1 else None)
                eng.eval_state()
                xd, L, P, _ = eng.download()
            finally:
                eng.close()
            assert np.array_equal(xd, x), "positions changed by the evaluation"
            compare(p, xd, L, P, "eval", f"eval D={D} {family}{tag}", bad)
            if tag:
                assert L[0, 0] == 0.0, "a walker exactly on mu"
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("like", ["dense", "diag", "rosen"])
@pytest.mark.parametrize("D,pad", xq.EVAL_WIDTHS, ids=WIDTH_IDS)
def test_stretch_split_proposals_within_B_of_exact(D, pad, like):
    bad = []
    T, W = xq.PARITY_T, xq.parity_walkers(D)
    for family in xq.families_of(like):
        prob = xq.make_problem(family, D)
        x0 = prob.x0(T, W)
        d = xq.stretch_draws(np.random.RandomState(5 + D), T, W)
        eng = _engine(prob, T, W, pad)
        try:
            _forced_upload(eng, prob, x0, T, W)
            for sp in (0, 1):
                keep = eng.stretch_split(sp, d["labels"], d[f"rint{sp}"], d[f"u_zz{sp}"], np.full_like(d[f"u_acc{sp}"], 1e-300))
                assert keep.all(), f"split {sp}: {int((~keep).sum())} proposals refused from L = -1e300"
            xd, L, P, _ = eng.download()
        finally:
            eng.close()
        if like != "rosen":                                             # (a proposal between two walkers on (1, ..., 1) is that point)
            assert np.all((xd != x0).any(axis=-1)), "every walker moved"
        compare(prob, xd, L, P, "split", f"split D={D} {family}", bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("like", ["dense", "diag"])
@pytest.mark.parametrize("D", xq.MH_WIDTHS)
def test_mh_step_proposals_within_B_of_exact(D, like):
    bad = []
    T, W = xq.PARITY_T, xq.parity_walkers(D)
    for family in xq.families_of(like):
        prob = xq.make_problem(family, D)
        x0 = prob.x0(T, W)
        step = np.sqrt(0.02) * prob.draw(np.random.RandomState(9 + D).randn(T, W, D))
        eng = _engine(prob, T, W)
        try:
            _forced_upload(eng, prob, x0, T, W)
            keep = eng.mh_step(step, np.full((T, W), 1e-300))
            assert keep.all()
            xd, L, P, _ = eng.download()
        finally:
            eng.close()
        assert np.array_equal(xd, x0 + step), "q = x + step"
        compare(prob, xd, L, P, "mh", f"mh D={D} {family}", bad)
    assert not bad, "\n".join(bad)


# ---- production hens_step --------------------------------------------------------------------------------------------------------------
CASES = {c[0]: c for c in xq.production_cases()}


def run_production(cid):
    """One production case in this process; -> the report entries it made."""
    _, name, like, family = CASES[cid]
    c = pb.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = xq.make_problem(family, D)
    bad, n0 = [], len(_report)
    eng = _engine(prob, T, W, pad=c["kw"].get("pad_rows", True), seed=c["seed"])
    try:
        _forced_upload(eng, prob, prob.x0(T, W), T, W)
        if c["mh"]:
            eng.set_mh_proposal("full", xq.mh_factor(prob), 0.5)
        eng.step(xq.STEPS[0])
        eng.synchronize()
        first = eng.counters()["accepted"] + (eng.mh_counters()["accepted"] if c["mh"] else 0.0)
        assert np.all(first == 1), f"{int((first != 1).sum())} walkers did not accept exactly once from L = -1e300"
        x, L, P, _ = eng.download()
        compare(prob, x, L, P, "production", f"{cid} step({xq.STEPS[0]})", bad)
        eng.step(xq.STEPS[1])
        eng.synchronize()
        later = eng.counters()["accepted"] + (eng.mh_counters()["accepted"] if c["mh"] else 0.0) - first
        x, L, P, _ = eng.download()
        e = compare(prob, x, L, P, "production", f"{cid} step({xq.STEPS[0]}) + step({xq.STEPS[1]})", bad)
        e["accepted_again"] = float((later > 0).mean())
        print(f"{cid}: {e['accepted_again']:.3f} of the walkers accepted again")
        if name.startswith(("one_launch", "two_launch")) and not c["mh"]:
            from tests.test_hip_records import _one_launch
            assert _one_launch(eng) == name.startswith("one_launch"), "the launch path the case is named after"
    finally:
        eng.close()
    assert not bad, "\n".join(bad)
    return _report[n0:]


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1])
from tests.test_hip_likelihood_accuracy import run_production
for e in run_production(sys.argv[2]):
    print("REPORT " + json.dumps(e))
"""


@pytest.mark.parametrize("cid", [k for k, c in CASES.items() if not pb.CASES[c[1]]["env"]])
def test_production_step_within_B_of_exact(cid):
    run_production(cid)


@pytest.mark.parametrize("cid", [k for k, c in CASES.items() if pb.CASES[c[1]]["env"]])
def test_production_step_within_B_of_exact_behind_a_switch(cid):
    """the paths a switch selects, each in a fresh child process (the library reads its switches once): k_stretch2 forced onto a
    small grid with a ragged last tile, the three copying launches"""
    env = pb.CASES[CASES[cid][1]]["env"]
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT, cid], env=_child_env(env), capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [json.loads(m) for m in re.findall(r"^REPORT (.*)$", r.stdout, flags=re.M)]
    assert len(got) == 2
    _report.extend(got)
    if "HENS_TILE2_FORCE" in env:
        assert "k_stretch2<pipe=0>" in r.stderr, "the first launches did not go to k_stretch2:\n" + r.stderr[-2000:]
