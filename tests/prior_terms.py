"""The specification of the per-parameter prior terms (host only, NumPy): what include/hipensemble.h's hens_set_prior_terms
computes, stated once, in the operation order of the reference (prior.py:337-392 over prior.py:12-136) and of SciPy 1.15
(``rv_continuous.logpdf``: ``y = (x - loc) / scale``, the support test on ``y``, ``_logpdf(y) - log(scale)``).

A term specification is the dict of ``eryn_amd.prior.ProbDistContainer.prior_terms()``: ``kind`` int32[D] (0 uniform, 1 log-uniform,
2 normal), the inclusive supports ``lo`` / ``hi``, and the constants ``c0`` / ``c1`` / ``c2`` the host forms:

    kind          support        term inside the support
    uniform       lo <= q <= hi  c0                      c0 = log(1 / (hi - lo))        (oracle.box_logpdf_vals)
    log-uniform   lo <= q <= hi  (-log(q)) - c0          c0 = log(log(hi) - log(lo))
    normal        q finite       y = (q - c0) / c1;  (-(y y) / 2.0 - C) - c2    c2 = log(c1); C = log(sqrt(2 pi)), SciPy's _norm_pdf_logC

    P(q) = ((0.0 + t_0) + t_1) + ... + t_{D-1}           ascending coordinate order; -inf as soon as one coordinate is outside

(The reference's container adds the terms in the order of the dictionary it was given; ``log_prior(..., order=...)`` restates
that, and tests/test_prior_terms.py holds it to the reference in mixed orders.  The device and ``eryn_amd.prior`` always add in
ascending order.  NaN is outside every support here; SciPy answers NaN and the reference's uniform 0.0 - no engine entry point
lets a NaN coordinate reach a prior, ensemble.py:1258-1262.)

``exact_log_prior`` is P* - the same formulas on the same doubles in ``np.longdouble`` (the constants c0, c1, c2 and C are data:
the doubles the device receives) - and ``float64_bound`` the a-priori bound B_P on |P - P*| of ANY float64 evaluation in the
specified order whose ``log`` is within 1 ulp.  With u = 2^-53 and m_d the sum of the magnitudes of the term's addends,

    m_d = |c0|                          uniform
          |log q| + |c0|                log-uniform
          y^2 / 2 + C + |c2|            normal          (m_d >= |t_d|, with equality where the addends share a sign),

    B_P = u (D + 6) sum_d m_d.

First order, a rounding of relative size u per operation:
  * a uniform term is a constant: no error of its own;
  * a log-uniform term: log(q) within 1 ulp = 2 u |log q|; the negation is exact; the subtraction rounds once, u |t_d|:
    3 u m_d at most;
  * a normal term: fl(q - c0) and the division round once each, so y carries 2 u and y y 4 u plus its own product's u; the
    halving is exact; the two subtractions round once each, relative to partial results no larger than m_d: 7 u m_d at most;
  * the running sum of D terms rounds D - 1 times, each relative to a partial sum no larger than sum_d |t_d| <= sum_d m_d.
So |P - P*| <= u (7 + D - 1) sum_d m_d = u (D + 6) sum_d m_d, and long double's own error (2^-63 relative per operation) is
three orders below u.  The issue that asked for this module stated u (D + 4) sum_d |t_d|: the count above gives D + 6 (the two
roundings inside y are squared), and |t_d| must be m_d - where -log(q) and c0 cancel, t_d is as small as one likes while the
logarithm's 2 u |log q| stays.  ``issue_bound`` keeps the stated form; tests assert it as well wherever no term cancels
(m_d <= 2 |t_d| in every coordinate).
"""
import os

import numpy as np

UNIFORM, LOG_UNIFORM, NORMAL = 0, 1, 2
NORM_PDF_LOGC = float(np.log(np.sqrt(2 * np.pi)))
U = 2.0 ** -53
LD = np.longdouble


def make_spec(entries):
    """[("uniform", lo, hi) | ("log_uniform", a, b) | ("normal", loc, scale), ...] -> the term specification, the constants formed as
    the host forms them (oracle.box_logpdf_vals for the uniform one)."""
    D = len(entries)
    spec = dict(kind=np.zeros(D, dtype=np.int32), lo=np.zeros(D), hi=np.zeros(D), c0=np.zeros(D), c1=np.zeros(D), c2=np.zeros(D))
    for d, (name, p, q) in enumerate(entries):
        p, q = float(p), float(q)
        if name == "uniform":
            spec["kind"][d], spec["lo"][d], spec["hi"][d], spec["c0"][d] = UNIFORM, p, q, np.log(1 / (q - p))
        elif name == "log_uniform":
            spec["kind"][d], spec["lo"][d], spec["hi"][d], spec["c0"][d] = LOG_UNIFORM, p, q, np.log(np.log(q) - np.log(p))
        elif name == "normal":
            spec["kind"][d], spec["lo"][d], spec["hi"][d], spec["c0"][d], spec["c1"][d], spec["c2"][d] = NORMAL, -np.inf, np.inf, p, q, np.log(q)
        else:
            raise ValueError(name)
    return spec


def terms(spec, q):
    """q[N, D] -> t[N, D]: the term of every coordinate, -inf outside its support."""
    q = np.asarray(q, dtype=np.float64)
    t = np.full(q.shape, -np.inf)
    for d in range(q.shape[1]):
        x = q[:, d]
        k = spec["kind"][d]
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            if k == NORMAL:
                inside = np.isfinite(x)
                y = (x - spec["c0"][d]) / spec["c1"][d]
                v = (-(y * y) / 2.0 - NORM_PDF_LOGC) - spec["c2"][d]
            elif k == LOG_UNIFORM:
                inside = (x >= spec["lo"][d]) & (x <= spec["hi"][d])
                v = (-np.log(np.where(inside, x, 1.0))) - spec["c0"][d]
            else:
                inside = (x >= spec["lo"][d]) & (x <= spec["hi"][d])
                v = np.full(x.shape, spec["c0"][d])
        t[inside, d] = v[inside]
    return t


def log_prior(spec, q, order=None):
    """P[N] of q[N, D]: the terms added one after the other from 0.0, in ascending coordinate order (``order``: another one)."""
    t = terms(spec, q)
    out = np.zeros(t.shape[0])
    for d in (range(t.shape[1]) if order is None else order):
        out += t[:, d]
    return out


def box_prior_substitute(spec):
    """A stand-in for ``oracle.eryn_oracle.box_log_prior(q, lo, hi)`` that evaluates ``spec`` (a closure; pytest's
    ``monkeypatch.setattr(orc, "box_log_prior", ...)`` installs it for one test).  ``lo`` / ``hi`` must be the specification's
    supports, which is what tests/problems.count_coverage reads them as."""
    def box_log_prior(q, lo, hi):
        assert np.array_equal(lo, spec["lo"]) and np.array_equal(hi, spec["hi"]), "the substituted prior got another box"
        return log_prior(spec, q)
    return box_log_prior


# ---- exact arithmetic and the bound ---------------------------------------------------------------------------------------------------
def _magnitudes(spec, q, ld):
    """(t[N, D], m[N, D]) in float64 or long double: the terms and the magnitudes of their addends, -inf / 0 outside the support."""
    ty = LD if ld else np.float64
    q = np.asarray(q, dtype=np.float64)
    t, m = np.full(q.shape, -np.inf, dtype=ty), np.zeros(q.shape, dtype=ty)
    inside_all = np.isfinite(terms(spec, q))
    for d in range(q.shape[1]):
        ins = inside_all[:, d]
        x = q[ins, d].astype(ty)
        k = spec["kind"][d]
        c0, c1 = ty(spec["c0"][d]), ty(spec["c1"][d])
        if k == NORMAL:
            y = (x - c0) / c1
            ls = ty(spec["c2"][d])                         # (the double the host forms: data)
            t[ins, d] = (-(y * y) / ty(2.0) - ty(NORM_PDF_LOGC)) - ls
            m[ins, d] = (y * y) / ty(2.0) + ty(NORM_PDF_LOGC) + abs(ls)
        elif k == LOG_UNIFORM:
            lg = np.log(x)
            t[ins, d] = (-lg) - c0
            m[ins, d] = np.abs(lg) + abs(c0)
        else:
            t[ins, d] = c0
            m[ins, d] = abs(c0)
    return t, m


def exact_log_prior(spec, q):
    """P*[N] as long double (-inf where a coordinate is outside its support)."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    t, _ = _magnitudes(spec, q, ld=True)
    return t.sum(axis=1)                                   # (long double: the order is immaterial at float64's u)


def float64_bound(spec, q):
    """B_P[N] = u (D + 6) sum_d m_d (0 where P* = -inf: -inf must come back exactly)."""
    t, m = _magnitudes(spec, q, ld=True)
    D = q.shape[1]
    return np.where(np.isfinite(t).all(axis=1), U * (D + 6) * m.sum(axis=1), 0.0).astype(np.float64)


def issue_bound(spec, q):
    """(u (D + 4) sum_d |t_d|, applicable[N]): the bound in the form the issue stated it, and where it can hold - no term of the
    point cancels (m_d <= 2 |t_d| in every coordinate)."""
    t, m = _magnitudes(spec, q, ld=True)
    D = q.shape[1]
    fin = np.isfinite(t).all(axis=1)
    ta = np.where(np.isfinite(t), np.abs(t), 0.0)
    ok = fin & (m <= 2.0 * ta).all(axis=1)
    return (U * (D + 4) * ta.sum(axis=1)).astype(np.float64), ok


def worst_ratio(P, spec, q):
    """max |P - P*| / B_P over the points inside every support (and the assertion that -inf falls exactly where P* has it)."""
    Ps, B = exact_log_prior(spec, q), float64_bound(spec, q)
    P = np.asarray(P, dtype=np.float64)
    assert np.array_equal(np.isneginf(P), np.isneginf(Ps.astype(np.float64))), "-inf does not fall where the specification has it"
    fin = np.isfinite(Ps)
    if not fin.any():
        return 0.0
    err = np.abs(P[fin].astype(LD) - Ps[fin]).astype(np.float64)
    return float(np.max(err / B[fin])) if np.all(B[fin] > 0) else float(np.inf if err.max() > 0 else 0.0)


# ---- the problem of the GPU tests and its coverage ----------------------------------------------------------------------------------------
INNER = 0.3              # start positions fill this concentric fraction of every coordinate's start box,
EDGE = (0.55, 1.0)       # but for ONE log-uniform coordinate per walker, which starts this far out (half-widths), on a random side
MAX_LOG_UNIFORM = 8      # log-uniform coordinates of a row, spread over its width


class PriorProblem:
    """A Gaussian (or Rosenbrock) likelihood under mixed per-parameter priors at row width D (tests/problems.hetero_problem's
    construction, with prior terms in place of the box).

    * up to MAX_LOG_UNIFORM log-uniform coordinates spread over the row (coordinate 0 never: an index that collapsed to 0 must not
      land on one), each on [a, b] with b / a between 10^3 and 10^3.5; the likelihood's mean sits in the middle of [a, b] and its
      width is a sixth of it.  A (coordinate, bound) is a proposal's SOLE offender only if nothing else leaves its support with
      it, so - as in hetero_problem - every walker starts deep inside every support but for one log-uniform coordinate, drawn at
      random with a random side, that starts next to its bound;
    * every coordinate d with d % 4 == 1 normal: loc ``off`` likelihood widths beside the likelihood's mean, scale 0.6 .. 1.4
      widths (Rosenbrock: 0.03 of that) - the prior moves accept decisions and never gives -inf.  ``off`` = 6 is what
      tests/test_prior_terms.py sizes: 2 left the D = 64 and D = 128 cases short of 40 changed decisions in six iterations;
    * the rest uniform on an interval of its own, 4 .. 6 likelihood widths wide, the mean not in its middle."""

    def __init__(self, D, like_kind="dense", seed=0, off=6.0, periodic=False):
        from tests import parity_utils as pu
        rs = np.random.RandomState(4242 + 17 * seed + D)
        self.D, self.like_kind, self.seed = D, like_kind, seed
        period = np.zeros(D)
        nlu = min(MAX_LOG_UNIFORM, max(2, D // 3))
        lu = sorted({2 + (j * (D - 3)) // max(nlu - 1, 1) for j in range(nlu)} - {d for d in range(D) if d % 4 == 1})
        names = ["log_uniform" if d in lu else "normal" if d % 4 == 1 else "uniform" for d in range(D)]
        if like_kind == "rosen":
            sig, mu = np.full(D, 1.0), np.zeros(D)
        else:
            mu0, invcov0 = pu.gaussian_problem(D, dense=(like_kind == "dense"))
            sig, mu = np.sqrt(np.diag(np.linalg.inv(invcov0))), 0.1 * rs.randn(D)
        entries, slo, shi = [], np.zeros(D), np.zeros(D)
        for d, k in enumerate(names):
            s = sig[d]
            if k == "log_uniform":
                width = 6.0 * s * rs.uniform(0.8, 1.2)
                a = width / (10.0 ** rs.uniform(3.0, 3.5) - 1.0)
                entries.append((k, a, a + width))
                mu[d] = a + 0.5 * width
                slo[d], shi[d] = a, a + width
            elif k == "normal":
                if periodic:                # the likelihood's mean in the middle of [0, period): proposals wrap, then meet the prior
                    mu[d], period[d] = 4.0 * s, 8.0 * s
                ns = s * (0.03 if like_kind == "rosen" else 1.0)      # (the Rosenbrock likelihood moves by hundreds: so must the prior)
                entries.append((k, mu[d] + off * ns * rs.choice([-1.0, 1.0]), ns * rs.uniform(0.6, 1.4)))
                slo[d], shi[d] = mu[d] - 3.0 * s, mu[d] + 3.0 * s
            else:
                entries.append((k, mu[d] - s * rs.uniform(2.0, 3.0), mu[d] + s * rs.uniform(2.0, 3.0)))
                slo[d], shi[d] = entries[-1][1], entries[-1][2]
        self.names, self.log_uniform = names, lu
        self.mu = mu
        self.precision = None if like_kind == "rosen" else (invcov0 if like_kind == "dense" else np.diag(invcov0).copy())
        self.spec = make_spec(entries)
        self.lo, self.hi = self.spec["lo"], self.spec["hi"]
        self.start_lo, self.start_hi = slo, shi
        self.period = period if periodic else None
        self.sig = sig

    def mh_proposal(self, kind, weight):
        """``HipEnsemble.set_mh_proposal`` arguments on the problem's scales: "iso" - 0.3 of the narrowest likelihood width for every
        coordinate; "full" - the lower Cholesky factor of 0.05 times the likelihood's covariance."""
        if kind == "iso":
            return ("iso", 0.3 * float(self.sig.min()), weight)
        cov = np.linalg.inv(self.precision) if self.like_kind == "dense" else np.diag(1.0 / self.precision)
        return ("full", np.linalg.cholesky(0.05 * cov), weight)

    def loglike(self, x):
        from oracle import eryn_oracle as orc
        if self.like_kind == "dense":
            return orc.gaussian_log_like(x, self.mu, self.precision)
        if self.like_kind == "diag":
            return orc.gaussian_diag_log_like(x, self.mu, self.precision)
        return orc.rosenbrock_log_like(x)

    def x0(self, T, W):
        rs = np.random.RandomState(1000 + self.seed)
        u = INNER * rs.uniform(-1.0, 1.0, size=(T, W, self.D))
        lu = np.array(self.log_uniform)
        edge = lu[rs.randint(lu.size, size=(T, W))]
        side = rs.choice([-1.0, 1.0], size=(T, W))
        tt, ww = np.meshgrid(np.arange(T), np.arange(W), indexing="ij")
        u[tt, ww, edge] = side * rs.uniform(EDGE[0], EDGE[1], size=(T, W))
        x = 0.5 * (self.start_lo + self.start_hi) + 0.5 * (self.start_hi - self.start_lo) * u
        return np.minimum(np.maximum(x, self.start_lo), self.start_hi)


def new_counts():
    return dict(proposals=0, outside=0, changed=0)


def count_decisions(cnt, out, logu, P_old):
    """Add one oracle move (the dict of orc.stretch_split / orc.mh_step, ``logu`` = log of its accept uniforms, ``P_old`` the moving
    walkers' log-prior before it) to ``cnt``: proposals, those with -inf prior, and the accept decisions that a constant prior would
    have made differently - keep != (lnpdiff - (P_new - P_old) > log u)."""
    logp, lnp, keep = out["logp"], out["lnpdiff"], out["keep"]
    cnt["proposals"] += int(logp.size)
    cnt["outside"] += int(np.isinf(logp).sum())
    fin = np.isfinite(logp)
    with np.errstate(invalid="ignore"):
        const = (lnp - np.where(fin, logp - P_old, 0.0)) > logu
    cnt["changed"] += int((fin & (const != keep)).sum())


BAND = (0.05, 0.90)          # share of proposals with -inf prior (the issue's band)
LEAST_CHANGED = 20           # accept decisions per case that differ from a constant prior's


def install(monkeypatch, prob, cnt=None):
    """Substitute ``prob.spec`` for the oracle's box prior for the duration of a test (pytest's monkeypatch on
    ``oracle.eryn_oracle``; nothing is written into oracle/).  ``cnt``: a dict of ``new_counts()`` - the oracle's two move functions
    are wrapped so that every move they make is counted (``count_decisions``, and tests/problems.count_coverage into
    ``cnt["cov"]``: per coordinate and bound the proposals it is the sole offender of)."""
    from oracle import eryn_oracle as orc
    from tests.problems import count_coverage, new_coverage
    monkeypatch.setattr(orc, "box_log_prior", box_prior_substitute(prob.spec))
    if cnt is None:
        return
    cnt.setdefault("cov", new_coverage(prob.D))
    inner_ss, inner_mh = orc.stretch_split, orc.mh_step

    def stretch_split(x, L, P, betas, labels, split, rint, u_zz, u_acc, a, lo, hi, *args, **kw):
        P0 = P.copy()
        out = inner_ss(x, L, P, betas, labels, split, rint, u_zz, u_acc, a, lo, hi, *args, **kw)
        with np.errstate(divide="ignore"):
            count_decisions(cnt, out, np.log(u_acc), P0[np.arange(x.shape[0])[:, None], out["S"]])
        count_coverage(cnt["cov"], out["q"], out["logp"], out["keep"], lo, hi, "stretch")
        return out

    def mh_step(x, L, P, betas, step, u_acc, lo, hi, *args, **kw):
        P0 = P.copy()
        out = inner_mh(x, L, P, betas, step, u_acc, lo, hi, *args, **kw)
        with np.errstate(divide="ignore"):
            count_decisions(cnt, out, np.log(u_acc), P0)
        count_coverage(cnt["cov"], out["q"], out["logp"], out["keep"], lo, hi, "mh")
        return out

    monkeypatch.setattr(orc, "stretch_split", stretch_split)
    monkeypatch.setattr(orc, "mh_step", mh_step)


def coverage_figures(cnt, prob):
    """(share of proposals with -inf prior, smallest sole-offender count over the log-uniform coordinates' bounds, accept decisions
    a constant prior would have made differently)"""
    lu = prob.log_uniform
    smallest = int(min(cnt["cov"]["sole_lo"][lu].min(), cnt["cov"]["sole_hi"][lu].min()))
    return cnt["outside"] / max(cnt["proposals"], 1), smallest, cnt["changed"]


def assert_coverage(cnt, prob, spare=1, what=""):
    """The issue's coverage conditions, from the ORACLE's proposals; ``spare`` = 2 on the CPU, where the cases are sized."""
    share, smallest, changed = coverage_figures(cnt, prob)
    print(f"{what}: proposals {cnt['proposals']} / outside {share:.3f} / smallest sole-offender count {smallest} / decisions changed {changed}")
    assert BAND[0] * spare <= share <= BAND[1] / spare, f"{what}: {share:.3f} of the proposals have -inf prior"
    assert smallest >= spare, f"{what}: a log-uniform bound was the sole offender of {smallest} proposals"
    assert changed >= LEAST_CHANGED * spare, f"{what}: {changed} accept decisions differ from a constant prior's"


# ---- the replayed cases: tests/test_hip_priors.py replays hens_step on them, tests/test_prior_terms.py sizes them on the CPU -----------
def case(T, W, D, like="dense", calls=(1, 5), mh=None, nsplits=2, periodic=False, pad=True, seed=77):
    return dict(T=T, W=W, D=D, like=like, calls=calls, mh=mh, nsplits=nsplits, periodic=periodic, pad=pad, seed=seed)


# W = 136: half a rung is one full tile of 64 walkers and a ragged one of four; six iterations, a ladder adaptation after each
CASES = {
    "D8": case(3, 136, 8),
    "D32": case(3, 136, 32),
    "D64": case(2, 136, 64),
    "D128": case(2, 136, 128),
    "padded_D11": case(4, 136, 11),
    "generic_D5": case(3, 136, 5, pad=False),
    "rosenbrock_D12": case(3, 72, 12, like="rosen", pad=False),
    "periodic_D16": case(3, 136, 16, periodic=True),
    "three_sets_D32": case(3, 136, 32, nsplits=3),
    "mh_iso_D32": case(3, 136, 32, mh=("iso", 0.5)),
    "mh_full_D32": case(3, 136, 32, mh=("full", 0.5)),
    "untempered_D16": case(1, 136, 16),
}


def case_problem(c):
    return PriorProblem(c["D"], c["like"], periodic=c["periodic"])


def oracle_case(monkeypatch, name):
    """The case on the oracle alone, with NumPy's draws (the CPU sizing): -> (counts, problem)."""
    from oracle import eryn_oracle as orc
    from tests import parity_utils as pu
    c = CASES[name]
    prob = case_problem(c)
    cnt = new_counts()
    install(monkeypatch, prob, cnt)
    moves = None
    if c["mh"]:
        kind, scale, w = prob.mh_proposal(*c["mh"])
        moves = [("stretch", 1.0 - w), (orc.GaussianProposal(scale * scale if kind == "iso" else scale @ scale.T), w)]
    o, _, _ = pu.make_oracle(c["T"], c["W"], c["D"], problem=prob, period=prob.period, live_dangerously=True, record=False,
                             nsplits=c["nsplits"], moves=moves)
    assert np.isfinite(o.P).all(), "a start outside a support"
    o.run(sum(c["calls"]))
    return cnt, prob


# ---- the fixture from the real reference (tests/golden/make_golden_priors.py) ------------------------------------------------------------------------------------------------------------------------
def load_fixture():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "priors", "p1_priors.npz"), allow_pickle=False)


class _FixtureProblem:
    pass


def fixture_problem(fx):
    """The fixture's priors through ``eryn_amd.prior`` - the same calls the generator made on the reference (``log_uniform(min, max)``
    with its construction quirk; NormalDistribution for scipy.stats.norm) - as a problem of tests/prior_terms.py."""
    from oracle import eryn_oracle as orc
    from eryn_amd.prior import NormalDistribution, ProbDistContainer, log_uniform, uniform_dist
    make = {0: uniform_dist, 1: log_uniform, 2: NormalDistribution}
    c = ProbDistContainer({d: make[int(k)](float(a), float(b)) for d, (k, a, b) in enumerate(zip(fx["prior_kind"], fx["prior_p0"], fx["prior_p1"]))})
    p = _FixtureProblem()
    p.container, p.spec, p.D = c, c.prior_terms(), int(fx["D"])
    p.lo, p.hi = p.spec["lo"], p.spec["hi"]
    mu, invcov = fx["mu"], fx["invcov"]
    p.mu, p.precision, p.like_kind, p.period = mu, invcov, "dense", None
    p.loglike = lambda x: orc.gaussian_log_like(x, mu, invcov)
    p.sig = np.sqrt(np.diag(np.linalg.inv(invcov)))
    p.log_uniform = [d for d in range(p.D) if p.spec["kind"][d] == LOG_UNIFORM]
    return p
