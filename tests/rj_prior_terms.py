"""The specification of per-parameter prior terms on leaf-packing records (host only, NumPy): what include/hipensemble.h's
hens_rj_set_prior_terms makes the reversible-jump kernels compute, stated once on top of tests/prior_terms.py (one term, one leaf)
and oracle/eryn_oracle_rj.py (slots, branches, moves).

``TermBranch`` is the oracle's ``Branch`` with the leaf's log-density and the birth draws taken from a term specification; the pinned
``OracleRJSampler`` and the replay classes of tests/test_hip_rj.py / tests/test_hip_leaf_kinds.py run on it unchanged.  In a
reversible-jump chain the prior enters three times - the log-prior of every active slot, the Hastings factor -+ log q(leaf) of a
birth / death, the distribution a born leaf is drawn from (distgenrj.py:188-214) - and all three are ``leaf_logpdf`` / ``rvs`` here.

Exact arithmetic and the bound of a state's log-prior
------------------------------------------------------
The log-prior of a state (ensemble.py:1189-1210) is, per branch, the sum over its slots of the ACTIVE leaves' values v (a dead slot
counts 0.0), branches accumulated in order; a leaf's value is tests/prior_terms.py's P on its ``ndim`` parameters.
``exact_state_log_prior`` is that in ``np.longdouble`` (P*).  An a-priori bound on |P - P*| for any float64 evaluation in the
specified order whose ``log`` is within 1 ulp, u = 2^-53, first order:

  * a leaf's value carries at most ``float64_bound`` at D = ndim (tests/prior_terms.py: B_P = u (D + 6) sum_d m_d);
  * the sum over a branch's slots (NumPy's pairwise order) rounds only where BOTH operands are non-zero - adding a dead slot's 0.0
    is exact - which happens at most (active leaves of the branch - 1) times; the accumulation over branches starts from 0.0 and
    rounds at most (branches - 1) times; every such rounding is relative to a partial sum no larger than S = sum |v| over the
    active leaves.  Together at most (active leaves - 1) roundings: u (active - 1) S.

``state_bound`` = sum over the active leaves of float64_bound + u (active leaves + branches) S: the form the issue that asked for
this module stated; the count above is smaller, so the stated form holds with room.  -inf must come back exactly (bound 0).

The births of the production path
---------------------------------
``hens_rj_step`` draws parameter d of a leaf born in branch b from ONE Philox call, counter (iter lo, iter hi, wid, PURPOSE_RJ_BIRTH |
d << 8 | b << 16), key (seed lo, seed hi), wid = global rung * W + walker, words (x, y, z, w); u = u01(x, y), v = u01(z, w):

    uniform      u (hi - lo) + lo                                 float64, these operations: BIT FOR BIT
    log-uniform  exp(u (log hi - log lo) + log lo)
    normal       loc + scale (sqrt(-2 log(1 - u)) cos(2 pi v))    Box-Muller; 1 - u in (0, 1] and 2 v are exact

``birth_spec`` gives the value in long double (X*) and an a-priori bound E on |X - X*| for a float64 evaluation whose log, exp,
sqrt and sincospi are within 1 ulp (relative 2 u), first order:

  * log-uniform: la = log lo, lb = log hi carry 2 u |la|, 2 u |lb|; the argument a = u (lb - la) + la weighs them with (1 - u) and
    u and rounds three times (difference, product, sum), each relative to a quantity no larger than M = |la| + |lb|:
    |a - a*| <= 2 u M + 3 u M = 5 u M; exp turns an absolute error of its argument into a relative one and adds its own 2 u:
    E = X* u (5 M + 2).
  * normal: log(1 - u) within 2 u relative; the doubling is exact; sqrt halves the relative error it is handed and adds 2 u: r within
    3 u; cos(2 pi v) from sincospi on an exact argument within 2 u; their product rounds once: z within 6 u; scale z rounds once
    (7 u |scale z|) and the sum once (u |X|):  E = u (7 |scale z*| + |X*|).
"""
import numpy as np

from oracle import eryn_oracle_rj as orj
from tests import prior_terms as pt
from tests.production_draws import philox4x32_10, u01

LD = np.longdouble
U = pt.U
PURPOSE_RJ_BIRTH = 23


class TermBranch(orj.Branch):
    """The oracle's ``Branch`` under a term specification: ``entries`` as tests/prior_terms.make_spec takes them, one per leaf
    parameter.  ``lo`` / ``hi`` are the supports."""

    def __init__(self, name, kind, entries, nleaves_max, nleaves_min=0, cov=None):
        self.entries = [(k, float(p), float(q)) for k, p, q in entries]
        self.spec = pt.make_spec(self.entries)
        with np.errstate(divide="ignore"):                          # (log(1 / inf): a normal parameter has no box)
            super().__init__(name, kind, list(zip(self.spec["lo"], self.spec["hi"])), nleaves_max, nleaves_min, cov=cov)

    def leaf_logpdf(self, x):
        """x[N, ndim] -> the leaf's log-density: tests/prior_terms.log_prior (ascending from 0.0, -inf outside a support)."""
        return pt.log_prior(self.spec, np.asarray(x, dtype=np.float64).reshape(-1, self.ndim))

    def rvs(self, n, G):
        """``ProbDistContainer.rvs`` (prior.py:432-497): per parameter, in order, the distribution's own ``rvs(n)`` on the GLOBAL stream -
        uniform_dist ``rand * (hi - lo) + lo`` (prior.py:60-66), scipy.stats.loguniform ``exp(log a + u (log b - log a))``,
        scipy.stats.norm ``standard_normal * scale + loc``."""
        out = np.zeros((n, self.ndim))
        s = self.spec
        for d in range(self.ndim):
            if s["kind"][d] == pt.NORMAL:
                out[:, d] = G.randn(n) * s["c1"][d] + s["c0"][d]
            elif s["kind"][d] == pt.LOG_UNIFORM:
                out[:, d] = np.exp(G.rand(n) * (np.log(s["hi"][d]) - np.log(s["lo"][d])) + np.log(s["lo"][d]))
            else:
                out[:, d] = G.rand(n) * (s["hi"][d] - s["lo"][d]) + s["lo"][d]
        return out

    def container(self):
        """The same prior as an ``eryn_amd.prior.ProbDistContainer`` (what the device branch takes in place of a box)."""
        from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, UniformDistribution
        make = {"uniform": UniformDistribution, "log_uniform": LogUniformDistribution, "normal": NormalDistribution}
        return ProbDistContainer({d: make[k](p, q) for d, (k, p, q) in enumerate(self.entries)})


# ---- exact arithmetic and the bound of a state's log-prior ------------------------------------------------------------------------
def _leaves(b, x, inds):
    m = np.asarray(inds[b.name], dtype=bool)
    return m, np.asarray(x[b.name], dtype=np.float64)[m].reshape(-1, b.ndim)


def exact_state_log_prior(branches, x, inds):
    """P*[T, W] as long double: the sum over branches and ACTIVE slots of tests/prior_terms.exact_log_prior (dead slots are not
    evaluated; -inf where an active leaf has a parameter outside its support)."""
    first = branches[0].name
    out = np.zeros(np.asarray(inds[first]).shape[:2], dtype=LD)
    for b in branches:
        m, leaves = _leaves(b, x, inds)
        v = np.zeros(m.shape, dtype=LD)
        if leaves.shape[0]:
            v[m] = pt.exact_log_prior(b.spec, leaves)
        out += v.sum(axis=-1)
    return out


def state_bound(branches, x, inds):
    """B[T, W] (float64): sum over the active leaves of float64_bound at D = ndim + u (active leaves + branches) sum |v|; 0 where P*
    is -inf."""
    first = branches[0].name
    shape = np.asarray(inds[first]).shape[:2]
    leafb, mag, nact = np.zeros(shape), np.zeros(shape, dtype=LD), np.zeros(shape)
    for b in branches:
        m, leaves = _leaves(b, x, inds)
        if not leaves.shape[0]:
            continue
        lb, v = np.zeros(m.shape), np.zeros(m.shape, dtype=LD)
        lb[m] = pt.float64_bound(b.spec, leaves)
        v[m] = np.abs(pt.exact_log_prior(b.spec, leaves))
        leafb += lb.sum(axis=-1)
        mag += v.sum(axis=-1)
        nact += m.sum(axis=-1)
    fin = np.isfinite(mag)
    with np.errstate(invalid="ignore"):
        B = leafb + U * (nact + len(branches)) * np.where(fin, mag, 0).astype(np.float64)
    return np.where(fin, B, 0.0)


def worst_state_ratio(P, branches, x, inds):
    """max |P - P*| / B over the walkers with a finite P* (and the assertion that -inf falls exactly where P* has it)."""
    Ps, B = exact_state_log_prior(branches, x, inds), state_bound(branches, x, inds)
    P = np.asarray(P, dtype=np.float64)
    assert np.array_equal(np.isneginf(P), np.isneginf(Ps.astype(np.float64))), "-inf does not fall where the specification has it"
    fin = np.isfinite(Ps)
    err = np.abs(P[fin].astype(LD) - Ps[fin]).astype(np.float64)
    if not err.size or err.max() == 0.0:
        return 0.0
    return float(np.max(np.where(err > 0, err / np.where(B[fin] > 0, B[fin], np.finfo(float).tiny), 0.0)))


# ---- the births of the production path ---------------------------------------------------------------------------------------------
def birth_words(seed, it, T, W, branch, d, rung_begin=0):
    """The four words [T, W] of the call that draws parameter d of a leaf born in ``branch`` (hens_rj.h: rj_birth_key)."""
    wid = (rung_begin + np.arange(T))[:, None] * W + np.arange(W)[None, :]
    key = PURPOSE_RJ_BIRTH | (d << 8) | (branch << 16)
    return philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, key, seed & 0xFFFFFFFF, seed >> 32)


def cospi(x):
    """cos(pi x) for x in [0, 2), float64, with the argument reduced EXACTLY to [0, 1/4] before pi enters (what a sincospi does; NumPy's
    cos(2 pi v) carries the rounding of 2 pi v, which next to a zero of the cosine is no small relative error)."""
    x = np.asarray(x, dtype=np.float64)
    x = np.where(x > 1.0, 2.0 - x, x)
    sign = np.where(x > 0.5, -1.0, 1.0)
    x = np.where(x > 0.5, 1.0 - x, x)
    return sign * np.where(x <= 0.25, np.cos(np.pi * np.minimum(x, 0.25)), np.sin(np.pi * (0.5 - np.maximum(x, 0.25))))


def birth_spec(spec, d, words):
    """(X float64, X* long double, E float64) of parameter d from ``words``: the float64 statement (bit for bit for a uniform term),
    the exact value and the a-priori bound on |X - X*| (module docstring)."""
    x, y, z, w = words
    u, v = u01(x, y), u01(z, w)
    k = spec["kind"][d]
    if k == pt.UNIFORM:
        lo, hi = spec["lo"][d], spec["hi"][d]
        X = u * (hi - lo) + lo
        Xs = LD(u) * (LD(hi) - LD(lo)) + LD(lo)
        return X, Xs, np.zeros(X.shape)
    if k == pt.LOG_UNIFORM:
        la, lb = np.log(spec["lo"][d]), np.log(spec["hi"][d])
        X = np.exp(u * (lb - la) + la)
        las, lbs = np.log(LD(spec["lo"][d])), np.log(LD(spec["hi"][d]))
        Xs = np.exp(u.astype(LD) * (lbs - las) + las)
        M = float(abs(las) + abs(lbs))
        return X, Xs, (Xs * U * (5.0 * M + 2.0)).astype(np.float64)
    loc, scale = spec["c0"][d], spec["c1"][d]
    r = np.sqrt(-2.0 * np.log(1.0 - u))
    X = loc + scale * (r * cospi(2.0 * v))
    zs = np.sqrt(LD(-2.0) * np.log(LD(1.0) - u.astype(LD))) * np.cos(_two_pi_ld() * v.astype(LD))
    Xs = LD(loc) + LD(scale) * zs
    return X, Xs, (U * (7.0 * np.abs(LD(scale) * zs) + np.abs(Xs))).astype(np.float64)


def _two_pi_ld():
    """2 pi in long double (np.pi is the double: 1.2e-16 off - the size of the bound)."""
    return LD(8.0) * np.arctan(LD(1.0))


def birth_unit_normal(words):
    """The standard normal behind a normal term's birth, float64."""
    x, y, z, w = words
    return np.sqrt(-2.0 * np.log(1.0 - u01(x, y))) * cospi(2.0 * u01(z, w))


# ---- the models of the GPU cases -------------------------------------------------------------------------------------------------
# per leaf kind (tests/leaf_kinds.KINDS) its parameters' priors: every branch of more than one parameter mixes the three kinds
TWO_PI = 2 * np.pi
ENTRIES = {
    "pulse": [("log_uniform", 1.0, 6.0), ("normal", 0.0, 0.35), ("uniform", 0.01, 0.21)],
    "sine": [("normal", 1.0, 0.2), ("log_uniform", 1.0, 20.0), ("uniform", 0.0, TWO_PI)],
    "offset": [("normal", 0.0, 0.8)],
    "ramp": [("uniform", -1.0, 1.0), ("normal", 0.0, 0.6)],
    "burst": [("log_uniform", 0.5, 3.0), ("normal", 0.0, 0.4), ("log_uniform", 0.05, 0.5), ("uniform", 1.0, 8.0)],
}
# in-model step per parameter, as a fraction of the width below (a box's width, a log-uniform support's, four scales of a normal)
STEP = 0.04


def widths_of(entries):
    return np.array([4.0 * q if k == "normal" else q - p for k, p, q in entries])


def branches_of(kinds, nl_max, nl_min, with_cov=True, step=STEP):
    """One TermBranch per kind, named after it (twice the same kind: name + index)."""
    from tests import leaf_kinds as lk
    out = []
    for i, k in enumerate(kinds):
        name = k if list(kinds).count(k) == 1 else f"{k}{i}"
        cov = np.diag((step * widths_of(ENTRIES[k])) ** 2) if with_cov else None
        out.append(TermBranch(name, lk.KINDS[k][0], ENTRIES[k], nl_max[i], nl_min[i], cov=cov))
        out[-1].kind_name, out[-1].step = k, step
    return out


def device_branches(branches):
    from eryn_amd.rj import TemplateBranch
    return [TemplateBranch(b.name, b.kind_name, b.container(), b.nleaves_max, b.nleaves_min) for b in branches]


def scales(branches):
    return [b.step * widths_of(b.entries) for b in branches]


def start_state(branches, T, W, rs, p_active=0.5):
    """Every slot holds a leaf drawn from the prior (dead slots too: they sit in the state), masks at random above the floor."""
    x, inds = {}, {}
    for b in branches:
        x[b.name] = b.rvs(T * W * b.nleaves_max, rs).reshape(T, W, b.nleaves_max, b.ndim)
        m = rs.rand(T, W, b.nleaves_max) < p_active
        m[..., :b.nleaves_min] = True
        inds[b.name] = m
    return x, inds


def problem(kinds, T, W, nl_max, nl_min, ndata, seed, sigma, step=STEP, p_active=0.5):
    """(branches, t, y, sigma, x, inds, betas): data = one leaf per branch from the prior + white noise."""
    from tests import leaf_kinds as lk
    rs = np.random.RandomState(seed)
    brs = branches_of(kinds, nl_max, nl_min, step=step)
    t = np.linspace(-1, 1, ndata)
    y = sigma * rs.randn(ndata)
    for b in brs:
        y = y + lk.leaf_value(b.kind_name, b.rvs(1, rs)[0], t)
    x, inds = start_state(brs, T, W, rs, p_active)
    return brs, t, y, sigma, x, inds, 0.35 ** np.arange(T)


def case(kinds, T, W, nl_max, nl_min, schedule, in_model, iters=8, ndata=40, sigma=3.0, seed=11, step=STEP, p_active=0.5, a=2.0):
    return dict(kinds=kinds, T=T, W=W, nl_max=nl_max, nl_min=nl_min, schedule=schedule, in_model=in_model, iters=iters, ndata=ndata,
                sigma=sigma, seed=seed, step=step, p_active=p_active, a=a)


def case_problem(c):
    return problem(c["kinds"], c["T"], c["W"], c["nl_max"], c["nl_min"], c["ndata"], c["seed"], c["sigma"], c["step"], c["p_active"])


PS = ("pulse", "sine")
# (the stretch cases run with a = 1.5: at a = 2 about 0.45 of their proposals leave a support whatever the seed - inside the band,
#  without the spare factor the sizing asks for)
# the issue's shapes under every schedule and both in-model moves, one model of widths 1 - 4, one record of more than 64 coordinates;
# the seeds and noise widths are those at which tests/test_rj_prior_terms.py finds the coverage conditions met with a spare factor 2
CASES = {
    "separate_gaussian": case(PS, 3, 10, (3, 4), (0, 0), "separate_branches", "gaussian"),
    "separate_floor_stretch": case(PS, 3, 10, (3, 4), (1, 0), "separate_branches", "stretch", p_active=0.3, a=1.5),
    "iterate_gaussian": case(PS, 3, 10, (3, 4), (1, 0), "iterate_branches", "gaussian"),
    "together_gaussian": case(PS, 3, 10, (3, 4), (0, 0), "together", "gaussian"),
    "together_stretch": case(PS, 3, 10, (3, 4), (0, 0), "together", "stretch", p_active=0.3, a=1.5),
    "tight_budget_iterate": case(PS, 2, 64, (2, 2), (0, 1), "iterate_branches", "gaussian", iters=6),
    "tight_budget_stretch": case(PS, 2, 64, (2, 2), (0, 1), "separate_branches", "stretch", iters=6, p_active=0.3, a=1.5),
    "widths_1_to_4": case(("offset", "ramp", "pulse", "burst"), 3, 10, (2, 2, 3, 2), (0, 0, 0, 0), "iterate_branches", "gaussian"),
    "record_past_64": case(PS, 2, 16, (12, 11), (0, 0), "together", "gaussian", iters=6, step=0.015),
}


def new_counts(nb):
    return dict(proposals=0, outside=0, changed=0, born=np.zeros(nb, dtype=int), died=np.zeros(nb, dtype=int))


def count_record(cnt, rec, o):
    """One recorded oracle iteration into ``cnt``: in-model proposals and those with a -inf prior; over every move the accept decisions
    a constant prior would have made differently (keep != (lnpdiff - (P_new - P_old) > log u), tests/prior_terms.count_decisions);
    accepted births and deaths per branch."""
    def decisions(logp, lnp, keep, u, P_old, in_model):
        fin = np.isfinite(logp)
        if in_model:
            cnt["proposals"] += int(logp.size)
            cnt["outside"] += int((~fin).sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            const = (lnp - np.where(fin, logp - P_old, 0.0)) > np.log(u)
        cnt["changed"] += int((fin & (const != keep)).sum())

    if "mh_logp" in rec:
        decisions(rec["mh_logp"], rec["mh_lnpdiff"], rec["mh_accepted"], rec["mh_u_acc"], rec["pre_P"], True)
    for h in range(2):
        if f"st_logp{h}" in rec:
            pre = rec["pre_P"] if h == 0 else rec["stupd0_P"]
            S = rec[f"st_S{h}"]
            decisions(rec[f"st_logp{h}"], rec[f"st_lnpdiff{h}"], rec[f"st_keep{h}"], rec[f"st_u_acc{h}"],
                      pre[np.arange(S.shape[0])[:, None], S], True)
    if "rj_sub" in rec or "rj_lnpdiff" in rec:
        for sub in rec.get("rj_sub", [rec]):
            decisions(sub["rj_logp"], sub["rj_lnpdiff"], sub["rj_accepted"], sub["rj_u_acc"], sub["rjpre_P"], False)
            bis = sub["rj_branches"] if "rj_branches" in sub else [sub["rj_branch"]]
            chs = sub["rj_change_all"] if "rj_branches" in sub else [sub["rj_change"]]
            for b_, ch in zip(bis, chs):
                cnt["born"][b_] += int(((ch == +1) & sub["rj_accepted"]).sum())
                cnt["died"][b_] += int(((ch == -1) & sub["rj_accepted"]).sum())


BAND = (0.05, 0.90)
LEAST_CHANGED = 20


def assert_coverage(cnt, spare=1, what=""):
    """The coverage conditions of the replayed cases, from the ORACLE's proposals; ``spare`` = 2 where the cases are sized."""
    share = cnt["outside"] / max(cnt["proposals"], 1)
    print(f"{what}: in-model proposals {cnt['proposals']}, -inf prior {share:.3f}; decisions changed {cnt['changed']}; accepted births "
          f"{cnt['born'].tolist()}, deaths {cnt['died'].tolist()}")
    assert BAND[0] * spare <= share <= BAND[1] / spare, f"{what}: {share:.3f} of the in-model proposals have a -inf prior"
    assert cnt["changed"] >= LEAST_CHANGED * spare, f"{what}: {cnt['changed']} accept decisions differ from a constant prior's"
    assert (cnt["born"] >= spare).all() and (cnt["died"] >= spare).all(), f"{what}: an accepted birth and death on every branch"


def oracle_case(name):
    """The case on the oracle alone, with NumPy's draws (the CPU sizing of the GPU cases): -> (counts, knife-edge decisions)."""
    from tests import leaf_kinds as lk
    from tests.test_hip_leaf_kinds import _counting, _knife_accepts
    c = CASES[name]
    brs, t, y, sigma, x, inds, betas = case_problem(c)
    R, G = np.random.RandomState(c["seed"] + 1), np.random.RandomState(c["seed"] + 2)
    o = _counting(orj.OracleRJSampler)(brs, x, inds, t, y, sigma, R, G, betas, schedule=c["schedule"], in_model=c["in_model"], record=True, a=c["a"],
                                      like_fn=lk.like_fn(c["kinds"]))
    o.live = True
    assert np.isfinite(o.st.P).all(), "a start outside a support"
    cnt, knives = new_counts(len(brs)), 0
    for _ in range(c["iters"]):
        o.iteration()
        rec = o.trace.pop()
        knives += _knife_accepts(rec)
        count_record(cnt, rec, o)
    return cnt, knives


# ---- the fixtures from the real reference (tests/golden/make_golden_rj_priors.py -> tests/golden/rj_priors/) -------------------------
# Per branch the ARGUMENTS of the reference's constructors, (kind, p0, p1) per leaf parameter: 0 uniform_dist(p0, p1), 1 log_uniform(p0,
# p1) - the reference builds scipy.stats.loguniform(p0, p1 - p0) -, 2 scipy.stats.norm(p0, p1).  A fixture stores them as ``{branch}_box``
# rows (p0, p1) and ``{branch}_prior_kind``.
FIXTURE_PRIORS = {
    "gauss": [(1, 1.0, 7.0), (2, 0.0, 0.4), (0, 0.01, 0.21)],
    "sine": [(2, 1.0, 0.3), (1, 1.0, 21.0), (0, 0.0, TWO_PI)],
    "ramp": [(0, -1.0, 1.0), (2, 0.0, 0.8)],
    "burst": [(1, 0.5, 3.5), (2, 0.0, 0.5), (1, 0.05, 0.55), (0, 1.0, 8.0)],
}
FIXTURES = ["rjp1_separate_gaussian", "rjp2_together_stretch", "rjp3_widths_callable_iterate"]
FIXTURE_KINDS = {"gauss": "pulse", "sine": "sine", "ramp": "ramp", "burst": "burst"}


def fixture_entries(kinds, p0, p1):
    """(kind, p0, p1) rows -> tests/prior_terms.make_spec entries, the reference's log_uniform construction applied."""
    name = {0: "uniform", 1: "log_uniform", 2: "normal"}
    return [(name[int(k)], float(a), float(b) - float(a) if int(k) == 1 else float(b)) for k, a, b in zip(kinds, p0, p1)]


def fixture_container(kinds, p0, p1):
    """The same priors through eryn_amd.prior's own names - the calls a user moves over from a reference script."""
    from eryn_amd.prior import NormalDistribution, ProbDistContainer, log_uniform, uniform_dist
    make = {0: uniform_dist, 1: log_uniform, 2: NormalDistribution}
    return ProbDistContainer({d: make[int(k)](float(a), float(b)) for d, (k, a, b) in enumerate(zip(kinds, p0, p1))})


def load_fixture(name):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rj_priors", name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_names(fx):
    return [str(k) for k in fx["branch_names"]]


def fixture_branches(fx):
    """The fixture's branches as TermBranch (the in-model covariance is the fixture's cov_factor on the diagonal)."""
    from tests import leaf_kinds as lk
    out = []
    for i, k in enumerate(fixture_names(fx)):
        ent = fixture_entries(fx[f"{k}_prior_kind"], fx[f"{k}_box"][:, 0], fx[f"{k}_box"][:, 1])
        b = TermBranch(k, lk.KINDS[FIXTURE_KINDS[k]][0], ent, int(fx["nl_max"][i]), int(fx["nl_min"][i]),
                       cov=np.diag(np.ones(len(ent))) * float(fx["cov_factor"]))
        b.kind_name = FIXTURE_KINDS[k]
        out.append(b)
    return out


def fixture_oracle(fx, record=False):
    """The pinned oracle on the fixture, fed from the fixture's two seeds (tests/test_oracle_golden_rj.make_rj_oracle under terms)."""
    from tests.test_oracle_golden_rj import LIKES
    brs = fixture_branches(fx)
    R, G = np.random.RandomState(int(fx["seed_construct"])), np.random.RandomState(int(fx["seed_run"]))
    x0 = {b.name: fx[f"x0_{b.name}"] for b in brs}
    inds0 = {b.name: fx[f"inds0_{b.name}"] for b in brs}
    return orj.OracleRJSampler(brs, x0, inds0, fx["t"], fx["y"], float(fx["sigma"]), R, G, fx["betas0"], record=record,
                               schedule=str(fx["rj_moves"]), in_model=str(fx["in_model"]),
                               like_fn=getattr(orj, LIKES[str(fx["model"])]) if "model" in fx else None)
