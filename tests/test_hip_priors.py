"""Per-parameter prior terms on the device (-m gpu): include/hipensemble.h hens_set_prior_terms against the specification
tests/prior_terms.py (uniform / log-uniform / normal, summed in ascending order from 0.0).

1. ``eval_state`` on a matrix of walkers at every row-width class: on each support bound, one ulp in, one ulp out, at ``loc``, at
   ``loc +- 1e100 scale``.  P is the specification's bit for bit where the row has no log-uniform coordinate (nothing but IEEE
   operations), within B_P of exact arithmetic everywhere, and -inf exactly where the specification has it.
2. The parity API with the oracle's draws (stretch_split / mh_step / pt_sweep, propose_split / accept_split) on the fixture the real
   reference recorded (tests/golden/priors/p1_priors.npz): masks and positions exact, L at the table's 1e-13, P at the bar above.
3. ``hens_step`` replayed through the oracle with the draws it consumed (tests/replay_utils.py) on ``prior_terms.CASES``; the
   oracle's box prior is substituted for the duration of the test (pytest's monkeypatch, nothing is written into oracle/).  Each case
   asserts its coverage from the ORACLE's proposals (tests/test_prior_terms.py sizes the same cases with a factor of two to spare) and
   that a profiled call reports the copying launches.
4. An all-uniform specification IS hens_set_prior_box: same launch path, same chain on a record shape.
5. The refusals, each leaving the context usable.
6. ``EnsembleSampler(rng="philox")`` with a mixed container: the oracle's chain at every stored step, a resume, DeviceBackend.

Figures (worst |P - P*| / B_P, worst relative L distance) are printed; HENS_PRIOR_REPORT=<path> collects them as JSON
(profiles/prior_terms_report.json was made that way).
"""
import json
import os

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests import replay_utils as ru
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
P_BAR = 1.0                      # |P - P*| <= P_BAR * B_P
REPORT = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    path = os.environ.get("HENS_PRIOR_REPORT")
    if path and REPORT:
        out = dict(worst_P_over_issue_bound=max(v.get("P_over_issue_bound", 0.0) for v in REPORT.values()), bar_P_over_B=P_BAR, bar_rel_L=tol.RTOL_L, worst_P_over_B=max(v.get("P_over_B", 0.0) for v in REPORT.values()),
                   worst_rel_L=max(v.get("rel_L", 0.0) for v in REPORT.values()), tests=dict(sorted(REPORT.items())))
        with open(path, "w") as f:
            json.dump(out, f, indent=1)


def _note(what, P_over_B=None, rel_L=None, P_over_issue_bound=None):
    e = REPORT.setdefault(what, {})
    if P_over_issue_bound is not None:
        e["P_over_issue_bound"] = max(e.get("P_over_issue_bound", 0.0), float(P_over_issue_bound))
    if P_over_B is not None:
        e["P_over_B"] = max(e.get("P_over_B", 0.0), float(P_over_B))
    if rel_L is not None:
        e["rel_L"] = max(e.get("rel_L", 0.0), float(rel_L))


def _check_P(P, spec, x, what, exact=False):
    """P[...] of the walkers at x[..., D]: -inf where the specification has it, within the bar of exact arithmetic, and bit for bit
    the specification where ``exact`` (rows without a log-uniform coordinate)."""
    D = x.shape[-1]
    P, x = np.asarray(P).reshape(-1), np.asarray(x).reshape(-1, D)
    ratio = pt.worst_ratio(P, spec, x)
    print(f"{what}: worst |P - P*| / B_P = {ratio:.3f} over {P.size} walkers")
    _note(what, P_over_B=ratio)
    assert ratio <= P_BAR, f"{what}: |P - P*| = {ratio:.3f} B_P"
    # ... and the bound in the form the issue stated it, u (D + 4) sum |t_d|, wherever it can hold (no term of the point cancels)
    Bi, can = pt.issue_bound(spec, x)
    if can.any():
        err = np.abs(P[can].astype(pt.LD) - pt.exact_log_prior(spec, x)[can]).astype(np.float64)
        worst = float(np.max(err / Bi[can]))
        _note(what, P_over_issue_bound=worst)
        assert worst <= P_BAR, f"{what}: |P - P*| = {worst:.3f} u (D + 4) sum |t_d|"
    if exact:
        assert np.array_equal(P, pt.log_prior(spec, x)), f"{what}: P is not the specification's bit for bit"


def _engine(prob, T, W, seed=77, pad=True, like=None, **kw):
    from eryn_amd.engine import HipEnsemble
    return HipEnsemble(T, W, prob.D, like or pu.device_likelihood(prob), None, None, seed=seed, pad_rows=pad, prior_terms=prob.spec,
                       live_dangerously=True, **kw)


# ---- 1. the evaluation matrix ---------------------------------------------------------------------------------------------------------
def edge_matrix(prob, T, W):
    """x[T, W, D] from the problem's start positions with ONE coordinate per walker - (w + 3 t) mod D - moved to a placement of its
    kind, in turn with every lap of the coordinates: bounded kinds on lo, on hi, one ulp inside either, one ulp outside either;
    normal ones at loc, loc + 1e100 scale, loc - 1e100 scale, one ulp beside loc."""
    spec, D = prob.spec, prob.D
    x = prob.x0(T, W)
    for t in range(T):
        for w in range(W):
            d = (w + 3 * t) % D
            place = (w // D + t) % 6
            lo, hi = spec["lo"][d], spec["hi"][d]
            if spec["kind"][d] == pt.NORMAL:
                loc, sc = spec["c0"][d], spec["c1"][d]
                x[t, w, d] = [loc, loc + 1e100 * sc, loc - 1e100 * sc, np.nextafter(loc, np.inf), loc, loc - 1e100 * sc][place]
            else:
                x[t, w, d] = [lo, hi, np.nextafter(lo, np.inf), np.nextafter(hi, -np.inf), np.nextafter(lo, -np.inf),
                              np.nextafter(hi, np.inf)][place]
    return x


class _NoLogUniform:
    """The problem with every log-uniform coordinate turned into a uniform one on the same support: nothing transcendental left."""

    def __init__(self, prob):
        self.__dict__.update(prob.__dict__)
        entries = []
        for d in range(prob.D):
            s = prob.spec
            k = s["kind"][d]
            entries.append(("normal", s["c0"][d], s["c1"][d]) if k == pt.NORMAL else ("uniform", s["lo"][d], s["hi"][d]))
        self.spec = pt.make_spec(entries)
        self.x0, self.log_uniform = prob.x0, prob.log_uniform


EVAL_WIDTHS = [(8, "dense", True), (16, "diag", True), (32, "dense", True), (64, "dense", True), (128, "dense", True), (11, "dense", True),
               (24, "diag", True), (5, "dense", False), (12, "rosen", False), (32, "host", False), (128, "host", False)]


@pytest.mark.parametrize("D,like,pad", EVAL_WIDTHS, ids=lambda v: str(v))
def test_evaluation_matrix_at_every_row_width(D, like, pad):
    from eryn_amd.likelihood import HostLikelihood
    base = pt.PriorProblem(D, "dense" if like == "host" else like)
    T, W = 2, 6 * D * max(1, -(-128 // (6 * D))) + 37           # whole laps of (coordinate, placement) over two tiles or more, + 37
    assert W > 128 and W % 64 != 0
    for prob, exact in ((base, False), (_NoLogUniform(base), True)):
        x = edge_matrix(prob, T, W)
        eng = _engine(prob, T, W, pad=pad, like=HostLikelihood(base.loglike, D) if like == "host" else None)
        eng.upload(x, betas=orc.make_ladder(D, ntemps=T))
        eng.eval_state()
        xd, L, P, _ = eng.download()
        eng.close()
        assert np.array_equal(xd, x), "positions changed by the evaluation"
        Pspec = pt.log_prior(prob.spec, x.reshape(-1, D)).reshape(T, W)
        assert np.isneginf(Pspec).sum() >= T * W // 8 and np.isfinite(Pspec).sum() >= T * W // 2, "the matrix has both verdicts"
        _check_P(P, prob.spec, x, f"eval_state D={D} {like}" + (" no log-uniform" if exact else ""), exact=exact)
        if like != "host":
            out = np.isneginf(Pspec)
            Lref = np.where(out, -1e300, base.loglike(x.reshape(-1, D)).reshape(T, W))
            assert np.array_equal(L[out], Lref[out]), "fill value outside the supports"
            _note(f"eval_state D={D} {like}", rel_L=tol.check_logl(L, Lref, tol.RTOL_L, f"eval_state D={D} {like}"))


# ---- 2. the parity API on the reference's fixture ---------------------------------------------------------------------------------------
def _fixture():
    fx = pt.load_fixture()
    return fx, pt.fixture_problem(fx)


def test_parity_api_on_the_reference_fixture():
    """stretch_split and pt_sweep with the draws the REAL reference consumed (tests/golden/priors/p1_priors.npz: T = 3, W = 10, D = 4,
    uniform / log-uniform / normal / log-uniform), teacher-forced from the reference's own states."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    fx, prob = _fixture()
    T, W, D, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"])
    eng = HipEnsemble(T, W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), None, None, a=float(fx["a"]), prior_terms=prob.spec,
                      live_dangerously=True)
    assert eng.RW == 8, "the fixture's rows are padded to a compile-time width"
    x, L, P, betas = fx["x0"], fx["L0"], fx["P0"], fx["betas0"]
    tt = np.arange(T)[:, None]
    for it in range(n):
        pre = f"it{it}_"
        eng.upload(x, L, P, betas)
        eng.set_adapt_time(it)
        for sp in (0, 1):
            keep = eng.stretch_split(sp, fx[pre + "labels"], fx[pre + f"rint{sp}"], fx[pre + f"u_zz{sp}"], fx[pre + f"u_acc{sp}"])
            assert np.array_equal(keep, fx[pre + f"keep{sp}"]), f"accept mask, iteration {it} split {sp}"
        xs, Ls, Ps, _ = eng.download()
        assert np.array_equal(xs, fx[pre + "x_stretch"]), "positions after the stretch move"
        _note("fixture", rel_L=tol.check_logl(Ls, fx[pre + "L_stretch"], tol.RTOL_L, "fixture: L after the stretch move"))
        _check_P(Ps, prob.spec, xs, f"fixture iteration {it}")
        eng.upload(fx[pre + "x_stretch"], fx[pre + "L_stretch"], fx[pre + "P_stretch"], betas)      # (swaps read L to the last bit)
        eng.set_adapt_time(it)
        sel, swaps = eng.pt_sweep(fx[pre + "iperm"], fx[pre + "i1perm"], fx[pre + "u_swap"], adapt=True)
        assert np.array_equal(sel, fx[pre + "sel"]) and np.array_equal(swaps, fx[pre + "swaps_accepted"])
        x2, L2, P2, b2 = eng.download()
        assert np.array_equal(x2, fx[pre + "x"]) and np.array_equal(L2, fx[pre + "L"]) and np.array_equal(P2, fx[pre + "P"])
        np.testing.assert_allclose(b2, fx[pre + "betas"], rtol=1e-13, atol=0)
        x, L, P, betas = fx[pre + "x"], fx[pre + "L"], fx[pre + "P"], fx[pre + "betas"]
    eng.close()


def test_host_likelihood_and_mh_step_on_the_reference_fixture():
    """propose_split / accept_split (k_propose, k_accept_decide: a Python likelihood) with the fixture's draws and the reference's
    log-likelihoods handed back; then mh_step with steps of the oracle's (the fixture holds no MH move) against the oracle under the
    substituted prior."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, HostLikelihood
    fx, prob = _fixture()
    T, W, D = int(fx["T"]), int(fx["W"]), int(fx["D"])
    eng = HipEnsemble(T, W, D, HostLikelihood(prob.loglike, D), None, None, a=float(fx["a"]), prior_terms=prob.spec, live_dangerously=True)
    x, L, P, betas = fx["x0"], fx["L0"], fx["P0"], fx["betas0"]
    for it in range(3):
        pre = f"it{it}_"
        eng.upload(x, L, P, betas)
        for sp in (0, 1):
            q, inbox = eng.propose_split(sp, fx[pre + "labels"], fx[pre + f"rint{sp}"], fx[pre + f"u_zz{sp}"])
            assert np.array_equal(q, fx[pre + f"q{sp}"]), "proposals"
            assert np.array_equal(inbox, np.isfinite(fx[pre + f"logp{sp}"])), "in-prior mask"
            keep = eng.accept_split(sp, fx[pre + f"logl{sp}"], fx[pre + f"u_acc{sp}"])
            assert np.array_equal(keep, fx[pre + f"keep{sp}"]), "accept mask"
        xs, Ls, Ps, _ = eng.download()
        assert np.array_equal(xs, fx[pre + "x_stretch"]) and np.array_equal(Ls, fx[pre + "L_stretch"])
        _check_P(Ps, prob.spec, xs, f"fixture, host likelihood, iteration {it}")
        x, L, P, betas = fx[pre + "x"], fx[pre + "L"], fx[pre + "P"], fx[pre + "betas"]
    eng.close()
    eng = HipEnsemble(T, W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), None, None, prior_terms=prob.spec, live_dangerously=True)
    rs = np.random.RandomState(5)
    x, L, P = fx["x0"].copy(), fx["L0"].copy(), fx["P0"].copy()
    mp = pytest.MonkeyPatch()
    try:
        pt.install(mp, prob)
        for _ in range(4):
            step, u = 0.3 * prob.sig * rs.randn(T, W, D), rs.rand(T, W)
            eng.upload(x, L, P, fx["betas0"])
            keep = eng.mh_step(step, u)
            out = orc.mh_step(x, L, P, fx["betas0"], step, u, prob.lo, prob.hi, prob.loglike)
            assert np.array_equal(keep, out["keep"]) and 0 < out["keep"].sum() < keep.size, "MH accept mask"
            xd, Ld, Pd, _ = eng.download()
            assert np.array_equal(xd, x), "positions after mh_step"
            _note("fixture mh_step", rel_L=tol.check_logl(Ld, L, tol.RTOL_L, "fixture: L after mh_step"))
            _check_P(Pd, prob.spec, xd, "fixture mh_step")
    finally:
        mp.undo()
    eng.close()


# ---- 3. production replay -----------------------------------------------------------------------------------------------------------------
def _assert_state(st, prob, x, L, P, betas, counters, mh_counters, what):
    """replay_utils.assert_state_equal with the log-prior at its bar instead of bit for bit (the device's log and NumPy's may differ
    in the last place): positions, counters exact; L at RTOL_L; betas at 1e-13; P within B_P of exact arithmetic at the positions."""
    assert np.array_equal(x, st.x), f"{what}: x differs from the oracle in {int((x != st.x).any(axis=-1).sum())} walkers " \
                                    f"(closest decision margin {st.min_margin:.2e})"
    _check_P(P, prob.spec, x, what)
    _check_P(st.P, prob.spec, st.x, what + " (oracle)")
    _note(what, rel_L=tol.check_logl(L, st.L, tol.RTOL_L, what))
    if st.betas is not None:
        np.testing.assert_allclose(betas, st.betas, rtol=1e-13, atol=0, err_msg=f"{what}: betas")
    assert np.array_equal(counters["accepted"], st.accepted), f"{what}: accept counters"
    if st.betas is not None and st.x.shape[0] > 1:
        assert np.array_equal(counters["swaps_total"], st.swaps_total), f"{what}: swap totals"
        assert np.array_equal(counters["swaps_last"], st.swaps_last), f"{what}: last sweep's swap counts"
    if mh_counters is not None:
        assert np.array_equal(mh_counters["accepted"], st.mh_accepted), f"{what}: MH accept counters"


@pytest.mark.parametrize("name", sorted(pt.CASES))
def test_replay_under_prior_terms(name, monkeypatch):
    c = pt.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = pt.case_problem(c)
    cnt = pt.new_counts()
    pt.install(monkeypatch, prob, cnt)
    eng = _engine(prob, T, W, seed=c["seed"], pad=c["pad"])
    assert eng.RW == (D if not c["pad"] or D in (8, 16, 32, 64, 128) else {11: 16}[D])
    betas0 = orc.make_ladder(D, ntemps=T) if T > 1 else None
    eng.upload(prob.x0(T, W), betas=betas0)
    eng.eval_state()
    mh = prob.mh_proposal(*c["mh"]) if c["mh"] else None
    if mh:
        eng.set_mh_proposal(*mh)
    if prob.period is not None:
        eng.set_periodic(prob.period)
    if c["nsplits"] != 2:
        eng.set_nsplits(c["nsplits"])
    x, L, P, betas = eng.download()
    assert np.isfinite(P).all(), "a start outside a support"
    _check_P(P, prob.spec, x, f"{name}: start")
    st = ru.OracleState(x, L, P, betas)
    kinds, done = [], 0
    for n in c["calls"]:
        it0 = eng.iteration()
        eng.step(n)
        eng.synchronize()
        kinds += ru.replay(eng, st, it0, n, prob.loglike, prob.lo, prob.hi, mh=mh is not None, period=prob.period, nsplits=c["nsplits"])
        x, L, P, betas = eng.download()
        done += n
        _assert_state(st, prob, x, L, P, betas, eng.counters(), eng.mh_counters() if mh else None, f"{name} after {done} iterations")
        assert st.min_margin > 1e-12, "a decision sat on the knife edge; pick another seed for this case"
    assert "stretch" in kinds and (mh is None or "mh" in kinds)
    assert st.accepted.sum() + st.mh_accepted.sum() > 0 and (T == 1 or st.swaps_total.sum() > 0)
    pt.assert_coverage(cnt, prob, spare=1, what=name)
    # the launch path: copying half-steps (one per set) and, on a ladder, the cascade as a launch of its own; no record launch
    if mh:
        eng.set_mh_proposal(None, None, 0.0)
    eng.set_profiling(True)
    eng.step(2)
    tm = eng.timing()
    eng.close()
    assert (tm["n_stretch"], tm["n_pt"], tm["n_fused"]) == (2 * c["nsplits"], 2 if T > 1 else 0, 0), tm


_WHICH = r"""
import sys
sys.path.insert(0, sys.argv[1])
import numpy as np
from oracle import eryn_oracle as orc
from tests import prior_terms as pt
from tests.test_hip_priors import _engine
for name in sys.argv[2:]:
    c = pt.CASES[name]
    prob = pt.case_problem(c)
    eng = _engine(prob, c["T"], c["W"], pad=c["pad"])
    eng.upload(prob.x0(c["T"], c["W"]), betas=orc.make_ladder(c["D"], ntemps=c["T"]) if c["T"] > 1 else None)
    if prob.period is not None:
        eng.set_periodic(prob.period)
    if c["mh"]:
        eng.set_mh_proposal(*prob.mh_proposal(c["mh"][0], 1.0))
    print("case", name, file=sys.stderr, flush=True)
    eng.eval_state()
    eng.step(2)
    eng.synchronize()
    eng.close()
"""


def test_which_kernel_steps_under_prior_terms():
    """HENS_PRIOR_LOG=1 in a child process (the library reads its switches once): every half-step and evaluation launch of a context
    with terms names its kernel - k_stretch_prior at the compile-time widths (padded rows included, every mode), the generic k_stretch
    for the other widths, for Rosenbrock rows that cannot be padded and with periodic parameters."""
    import subprocess
    import sys
    want = {"D8": "k_stretch_prior", "D32": "k_stretch_prior", "D64": "k_stretch_prior", "D128": "k_stretch_prior",
            "padded_D11": "k_stretch_prior", "mh_full_D32": "k_stretch_prior", "three_sets_D32": "k_stretch_prior",
            "untempered_D16": "k_stretch_prior", "generic_D5": "k_stretch", "rosenbrock_D12": "k_stretch", "periodic_D16": "k_stretch"}
    r = subprocess.run([sys.executable, "-c", _WHICH, os.path.dirname(HERE)] + list(want), env=dict(os.environ, HENS_PRIOR_LOG="1"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    seen, cur = {}, None
    for line in r.stderr.splitlines():
        if line.startswith("case "):
            cur = line.split()[1]
        elif line.startswith("hens: prior terms"):
            seen.setdefault(cur, set()).add((line.split("mode ")[1].split(":")[0], line.rsplit(": ", 1)[1]))
    for name, kernel in want.items():
        kernels = {k for _, k in seen.get(name, ())}
        modes = {m for m, _ in seen.get(name, ())}
        assert kernels == {kernel}, f"{name}: launches went to {sorted(kernels)}, {kernel} expected"
        assert len(modes) >= 2, f"{name}: the evaluation and a stepping mode both launch ({sorted(modes)})"


# ---- 4. uniform kinds only: the box ----------------------------------------------------------------------------------------------------
def test_an_all_uniform_specification_is_the_box():
    """8 x 256 x 32, a record shape, 20 iterations: through hens_set_prior_terms the launch path and the chain are the box's, bit for bit;
    a mixed specification leaves the record path and hens_set_prior_box returns to it."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.prior import ProbDistContainer, uniform_dist
    T, W, D = 8, 256, 32
    mu, invcov = pu.gaussian_problem(D)
    lo, hi = -3.0 - 0.1 * np.arange(D), 4.0 + 0.05 * np.arange(D)
    x0 = np.clip(np.random.RandomState(2).randn(T, W, D), lo + 0.1, hi - 0.1)

    def run(terms):
        eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), lo, hi, seed=5, prior_terms=terms)
        eng.upload(x0, betas=orc.make_ladder(D, ntemps=T))
        eng.eval_state()
        eng.step(18)
        eng.set_profiling(True)
        eng.step(2)
        tm = eng.timing()
        eng.set_profiling(False)
        return eng, eng.download(), eng.counters(), (tm["n_stretch"], tm["n_pt"], tm["n_fused"])

    box = ProbDistContainer({d: uniform_dist(lo[d], hi[d]) for d in range(D)})
    a, sa, ca, pa = run(None)
    b, sb, cb, pb_ = run(box.prior_terms())
    assert b.prior_terms is None and b.logp_inside == a.logp_inside
    assert pa == pb_ and pa[2] > 0, f"launch paths {pa} / {pb_}: the box steps on walker records"
    for u, v in zip(sa, sb):
        assert np.array_equal(u, v)
    assert all(np.array_equal(ca[k], cb[k]) for k in ca)
    assert np.isneginf(pt.log_prior(box.prior_terms(), x0.reshape(-1, D))).sum() == 0 and ca["accepted"].sum() > 0
    # a mixed specification on the same context: the copying launches; back to the box: the records again, and a's chain continues
    prob = pt.PriorProblem(D)
    b.set_prior_terms(prob.spec)
    b.set_profiling(True)
    b.upload(prob.x0(T, W), betas=orc.make_ladder(D, ntemps=T))
    b.eval_state()
    b.step(2)
    tm = b.timing()
    assert (tm["n_stretch"], tm["n_pt"], tm["n_fused"]) == (4, 2, 0), tm
    b.set_prior_box(lo, hi)
    for e in (a, b):
        e.set_profiling(False)
        e.upload(sa[0], sa[1], sa[2], sa[3])
        e.set_iteration(20)
        e.set_adapt_time(ca["adapt_time"])
        e.step(5)
    for u, v in zip(a.download(), b.download()):
        assert np.array_equal(u, v), "the context did not return to the box"
    a.close()
    b.close()


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_usable():
    from eryn_amd import _lib
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    T, W, D = 2, 64, 8
    prob = pt.PriorProblem(D)
    mu, invcov = prob.mu, prob.precision
    eng = _engine(prob, T, W)
    x0 = prob.x0(T, W)

    def state():
        eng.upload(x0, betas=orc.make_ladder(D, ntemps=T))
        eng.eval_state()
        eng.set_iteration(0)                     # (the same draws every time)
        eng.set_adapt_time(0)
        eng.step(2)
        return eng.download()

    want = state()
    lu, no = prob.log_uniform[0], [d for d in range(D) if prob.spec["kind"][d] == pt.NORMAL][0]
    bad = {
        "lo >= hi": (lu, "hi", prob.spec["lo"][lu], ValueError, f"lo < hi in every dimension (dim {lu})"),
        "a <= 0": (lu, "lo", 0.0, ValueError, f"0 < lo < hi < inf (dim {lu})"),
        "scale <= 0": (no, "c1", 0.0, ValueError, f"scale > 0 (dim {no})"),
        "non-finite constant": (lu, "c0", np.inf, ValueError, f"c0 must be finite (dim {lu})"),
        "non-finite log scale": (no, "c2", np.nan, ValueError, f"(dim {no})"),
        "unknown kind": (0, "kind", 7, ValueError, "unknown prior kind 7 (dim 0)"),
    }
    for what, (d, key, value, exc, text) in bad.items():
        spec = {k: v.copy() for k, v in prob.spec.items()}
        spec[key][d] = value
        with pytest.raises(exc) as e:
            eng.set_prior_terms(spec)
        assert text in str(e.value), (what, str(e.value))
        got = state()
        assert all(np.array_equal(u, v) for u, v in zip(want, got)), f"after the refusal '{what}' the context steps another chain"
    # a rank of the ladder pipeline: refused once it is one, and hens_pipe_init refuses after prior terms
    with pytest.raises(NotImplementedError) as e:
        eng.pipe_init(1, 0)
    assert "prior terms are not built for a rank of the ladder pipeline" in str(e.value)
    got = state()
    assert all(np.array_equal(u, v) for u, v in zip(want, got))
    eng.close()
    rank = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), -50.0, 50.0)
    rank.pipe_init(1, 0)
    with pytest.raises(RuntimeError) as e:
        rank.set_prior_terms(prob.spec)
    assert "prior terms are not built for a rank of the ladder pipeline" in str(e.value)
    rank.close()
    # a leaf-packing context
    from eryn_amd.rj import _TemplateLikelihood
    rj = HipEnsemble(2, 16, D, _TemplateLikelihood(D), -1.0, 1.0, tempered=True, live_dangerously=True)
    with pytest.raises(NotImplementedError) as e:
        rj.set_prior_terms(prob.spec)
    assert "leaf-packing" in str(e.value)
    assert _lib.load().hens_set_prior_box(rj.ctx, _lib.ptr(np.full(D, -1.0)), _lib.ptr(np.full(D, 1.0)), 0.0) == _lib.HENS_OK
    rj.close()


# ---- 6. the sampler ---------------------------------------------------------------------------------------------------------------------------
def _container(prob):
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, uniform_dist
    s = prob.spec
    d = {}
    for k in range(prob.D):
        kind = s["kind"][k]
        d[k] = (uniform_dist(s["lo"][k], s["hi"][k]) if kind == pt.UNIFORM else
                LogUniformDistribution(s["lo"][k], s["hi"][k]) if kind == pt.LOG_UNIFORM else NormalDistribution(s["c0"][k], s["c1"][k]))
    c = ProbDistContainer(d)
    assert all(np.array_equal(c.prior_terms()[k], s[k]) for k in s), "the container's terms are the specification's"
    return c


def test_sampler_with_a_mixed_container(monkeypatch):
    from eryn_amd.backend import Backend, DeviceBackend
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.state import State
    T, W, D, n = 3, 72, 8, 7
    prob = pt.PriorProblem(D)
    pt.install(monkeypatch, prob)
    priors, x0 = _container(prob), prob.x0(T, W)

    def sampler(backend=None, **tk):
        return EnsembleSampler(W, D, pu.device_likelihood(prob), priors, rng="philox", seed=77, backend=backend,
                               tempering_kwargs=dict(ntemps=T, **tk))

    a = sampler()
    whole = [State(st, copy=True) for st in a.sample(x0, iterations=n, store=True)]
    # the oracle, with the draws the context consumed, from the sampler's own start
    eng = a.engine
    P0 = a.compute_log_prior(x0)
    _check_P(P0, prob.spec, x0, "sampler: start")
    L0 = a.compute_log_like(x0)[0]
    st = ru.OracleState(x0, L0, P0, orc.make_ladder(D, ntemps=T))
    for it, got in enumerate(whole):
        ru.replay(eng, st, it, 1, prob.loglike, prob.lo, prob.hi)
        assert np.array_equal(got.branches["model_0"].coords[:, :, 0, :], st.x), f"stored step {it}: positions"
        _check_P(got.log_prior, prob.spec, st.x, f"sampler step {it}")
        _note("sampler", rel_L=tol.check_logl(got.log_like, st.L, tol.RTOL_L, "sampler"))
        np.testing.assert_allclose(got.betas, st.betas, rtol=1e-13, atol=0)
    assert np.array_equal(a.get_chain()["model_0"][:, :, :, 0, :], np.stack([s.branches["model_0"].coords[:, :, 0, :] for s in whole]))
    assert np.array_equal(a.get_log_prior(), np.stack([s.log_prior for s in whole]))
    # a resume from a stored State, in a new sampler
    b = sampler()
    first = [State(s, copy=True) for s in b.sample(x0, iterations=3, store=True)]
    c = sampler()
    rest = [State(s, copy=True) for s in c.sample(first[-1], iterations=n - 3, store=True)]
    for k, (u, v) in enumerate(zip(whole, first + rest)):
        for f in ("log_like", "log_prior", "betas"):
            assert np.array_equal(getattr(u, f), getattr(v, f)), f"{f} differs at stored step {k}"
        assert np.array_equal(u.branches["model_0"].coords, v.branches["model_0"].coords) and u.random_state == v.random_state
    # the chain on the device
    h, d = sampler(Backend(), stop_adaptation=3), sampler(DeviceBackend(), stop_adaptation=3)
    for s in (h, d):
        s.run_mcmc(x0, n)
    assert np.array_equal(h.get_chain()["model_0"], d.get_chain()["model_0"])
    assert np.array_equal(h.get_log_prior(), d.get_log_prior()) and np.array_equal(h.get_log_like(), d.get_log_like())
    assert np.array_equal(h.backend.accepted, d.backend.accepted) and np.array_equal(h.backend.swaps_accepted, d.backend.swaps_accepted)
    assert h.backend.get_evidence_estimate(discard=4) == d.backend.get_evidence_estimate(discard=4)
