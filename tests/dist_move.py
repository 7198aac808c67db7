"""The specification of the draw-from-distribution move (host only, NumPy): what include/hipensemble.h's hens_set_dist_proposal /
hens_dist_step and the k_dist launch of hens_step compute, stated once on tests/prior_terms.py (one term, one row) and the
oracle's ``compute_log_like`` / ``tempered_log_posterior`` / ``pt_sweep`` / ``adapt_ladder`` (imported, not edited).

The move (distgen.py:34-104 under mh.py:56-193), single branch, every leaf active: every walker is proposed a fresh point q from a
generator of per-coordinate terms; with logq the generator's log-density (tests/prior_terms.log_prior: ascending from 0.0, -inf
outside a support)

    factors = (0.0 + logq(old)) + (-logq(new))                     (distgen.py:84,94,100)
    logp    = prior(q);  logl = like(q) where logp is finite, ``fill`` elsewhere
    keep    = factors + tempered(logl, logp) - tempered(L, P) > log u

An old point outside the generator gives factors = -inf and is never moved; a new point outside it cannot occur on the device's own
draws (they are clamped) and gives +inf (NaN with an old point outside as well: not accepted) on a caller's.

The draws of the production path
--------------------------------
Coordinate d of walker wid = global rung * W + walker in iteration ``it``: ONE Philox4x32-10 call, counter (it lo, it hi, wid,
PURPOSE_DIST | d << 8), key (seed lo, seed hi), its four words turned into a value by the function that draws births
(tests/rj_prior_terms.birth_spec: uniform bit for bit, log-uniform and Box-Muller normal with the bound E derived there), and - new
here - a uniform or log-uniform value clamped into its support, min(max(X, lo), hi): rounding can put exp(log a) an ulp below a.
The clamp moves X and X* towards each other or not at all (it is 1-Lipschitz), so |X - X*| <= E survives it.  The accept uniform
is the MH move's own (tests/production_draws.mh_uniform): an iteration runs one move only.

Exact arithmetic and the bound of the factor
--------------------------------------------
F* = logq*(old) - logq*(new) in long double (tests/prior_terms.exact_log_prior).  A float64 evaluation in the specified order forms
S_o = logq(old) and S_n = logq(new), each within tests/prior_terms.float64_bound of its exact value (B_P at the old and at the new
row); 0.0 + S_o and the negation are exact; the one subtraction rounds once, relative u = 2^-53 to a result no larger than
|S_o| + |S_n|:

    B_F = B_P(old) + B_P(new) + u (|logq*(old)| + |logq*(new)|)

(first order, as B_P is).  Where a row is outside the generator the factor is -inf / +inf / NaN exactly and the bound is 0.
"""
import numpy as np

from oracle import eryn_oracle as orc
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import rj_prior_terms as rpt

LD = np.longdouble
U = pt.U
PURPOSE_DIST = 14


def gen_factors(gen, x_old, q):
    """factors[T, W] of proposals q[T, W, D] from x_old[T, W, D] (distgen.py:84,94,100, in that order)."""
    T, W, D = q.shape
    factors = np.zeros((T, W))
    with np.errstate(invalid="ignore"):
        factors += +1 * pt.log_prior(gen, x_old.reshape(-1, D)).reshape(T, W)
        factors += -1 * pt.log_prior(gen, q.reshape(-1, D)).reshape(T, W)
    return factors


def dist_step(x, L, P, betas, q, u_acc, prior, gen, loglike, fill=-1e300, info=None):
    """One full-ensemble proposal of the move; mutates x, L, P in place and returns (x, L, P, keep, factors).  ``prior`` / ``gen``:
    term specifications (tests/prior_terms.make_spec); ``info``: a dict that receives logp, logl, lnpdiff of the proposals."""
    T, W, D = x.shape
    q = np.asarray(q, dtype=np.float64).reshape(T, W, D)
    factors = gen_factors(gen, x, q)
    logp = pt.log_prior(prior, q.reshape(-1, D)).reshape(T, W)                 # mh.py:120
    logl = orc.compute_log_like(q, logp, loglike, fill=fill)                   # mh.py:126-132
    logP = orc.tempered_log_posterior(logl, logp, betas)                       # mh.py:142
    prev_logP = orc.tempered_log_posterior(L, P, betas)                        # mh.py:146-152
    with np.errstate(invalid="ignore"):
        lnpdiff = factors + logP - prev_logP                                   # mh.py:155
    with np.errstate(divide="ignore", invalid="ignore"):
        keep = lnpdiff > np.log(u_acc)                                         # mh.py:157
    new_logp = logp.copy()
    new_logp[np.isinf(new_logp)] = 0.0                                         # move.py:513-532
    L[...] = logl * keep + L * (~keep)
    P[...] = new_logp * keep + P * (~keep)
    x[keep] = q[keep]
    if info is not None:
        info.update(q=q, logp=logp, logl=logl, lnpdiff=lnpdiff, u_acc=np.asarray(u_acc))
    return x, L, P, keep, factors


# ---- the draws of the production path ------------------------------------------------------------------------------------------------
def dist_words(seed, it, T, W, d, rung_begin=0):
    """The four words [T, W] of the call that draws coordinate d (hens_dist.h: dist_draw)."""
    wid = (rung_begin + np.arange(T))[:, None] * W + np.arange(W)[None, :]
    return pd.philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, PURPOSE_DIST | (d << 8), seed & 0xFFFFFFFF, seed >> 32)


def value_of(gen, d, words):
    """(X, X*, E) of coordinate d from ``words``: tests/rj_prior_terms.birth_spec and the clamp of a bounded support."""
    X, Xs, E = rpt.birth_spec(gen, d, words)
    if gen["kind"][d] != pt.NORMAL:
        lo, hi = gen["lo"][d], gen["hi"][d]
        X = np.minimum(np.maximum(X, lo), hi)
        Xs = np.minimum(np.maximum(Xs, LD(lo)), LD(hi))
    return X, Xs, E


def dist_draws(seed, it, T, W, gen, rung_begin=0):
    """(X float64, X* long double, E float64), each [T, W, D]: the points iteration ``it`` proposes."""
    D = len(gen["kind"])
    X, Xs, E = np.zeros((T, W, D)), np.zeros((T, W, D), dtype=LD), np.zeros((T, W, D))
    for d in range(D):
        X[..., d], Xs[..., d], E[..., d] = value_of(gen, d, dist_words(seed, it, T, W, d, rung_begin))
    return X, Xs, E


def accept_uniforms(seed, it, T, W, rung_begin=0):
    return np.stack([pd.mh_uniform(seed, it, rung_begin + t, W) for t in range(T)])


def unit_normals(seed, it, T, W, gen, rung_begin=0):
    """The standard normals behind the normal coordinates of one iteration's draws, [T, W, n_normal] in coordinate order."""
    out = [rpt.birth_unit_normal(dist_words(seed, it, T, W, d, rung_begin)) for d in range(len(gen["kind"])) if gen["kind"][d] == pt.NORMAL]
    return np.stack(out, axis=-1) if out else np.zeros((T, W, 0))


# ---- exact arithmetic and the bound of the factor -------------------------------------------------------------------------------------
def exact_factors(gen, x_old, q):
    """(F* long double [T, W], B_F float64 [T, W]); F* is -inf / +inf / NaN where a row is outside the generator, B_F = 0 there."""
    T, W, D = q.shape
    so, sn = pt.exact_log_prior(gen, x_old.reshape(-1, D)), pt.exact_log_prior(gen, q.reshape(-1, D))
    bo, bn = pt.float64_bound(gen, x_old.reshape(-1, D)), pt.float64_bound(gen, q.reshape(-1, D))
    with np.errstate(invalid="ignore"):
        F = so - sn
    fin = np.isfinite(so) & np.isfinite(sn)
    mag = (np.abs(np.where(fin, so, 0)) + np.abs(np.where(fin, sn, 0))).astype(np.float64)
    B = np.where(fin, bo + bn + U * mag, 0.0)
    return F.reshape(T, W), B.reshape(T, W)


def has_log_uniform(gen):
    return bool(np.any(np.asarray(gen["kind"]) == pt.LOG_UNIFORM))


def assert_factors(F, gen, x_old, q, what=""):
    """The issue's bar on factors_out: bit for bit against the specification where the generator has no log-uniform coordinate,
    else |F - F*| <= 1.0 B_F; the non-finite values exactly where the specification has them."""
    spec = gen_factors(gen, x_old, q)
    if not has_log_uniform(gen):
        assert np.array_equal(F, spec, equal_nan=True), f"{what}: factors differ from the specification"
        return 0.0
    Fs, B = exact_factors(gen, x_old, q)
    fin = np.isfinite(spec)
    assert np.array_equal(np.isfinite(F), fin), f"{what}: a non-finite factor where the specification has a finite one (or the reverse)"
    assert np.array_equal(F[~fin], spec[~fin], equal_nan=True), f"{what}: the non-finite factors differ"
    err = np.abs(F[fin].astype(LD) - Fs[fin]).astype(np.float64)
    ratio = float(np.max(err / B[fin])) if fin.any() else 0.0
    print(f"{what}: factors |F - F*| / B_F <= {ratio:.3f}")
    assert ratio <= 1.0, f"{what}: |F - F*| reaches {ratio:.3f} B_F"
    return ratio


# ---- generators and problems of the GPU cases ------------------------------------------------------------------------------------------
def box_spec(lo, hi):
    return pt.make_spec([("uniform", a, b) for a, b in zip(lo, hi)])


class DistProblem:
    """A likelihood, a prior (box or mixed terms) and a generator at row width D.  ``prior``: "box" - a box of +-4 likelihood widths
    round the likelihood's mean - or "terms" - tests/prior_terms.PriorProblem's mixed terms; ``gen``: "box" (the prior's own box:
    the factor is a constant minus itself), "mixed" (uniform / log-uniform / normal in turn, the bounded ones NARROWER than the start
    in places and wider than a box prior in others), "normal_lu" (normal and log-uniform), "uniform_normal"."""

    def __init__(self, D, like="dense", prior="box", gen="mixed", seed=0):
        from tests import parity_utils as pu
        self.D, self.like_kind = D, like
        rs = np.random.RandomState(9100 + 13 * seed + D)
        if prior == "terms":
            pp = pt.PriorProblem(D, like)
            self.mu, self.precision, sig, self.prior = pp.mu, pp.precision, pp.sig, pp.spec
            centre = 0.5 * (pp.start_lo + pp.start_hi)
            half = 0.5 * (pp.start_hi - pp.start_lo)
        else:
            if like == "rosen":
                sig, self.mu, self.precision = np.full(D, 0.25), np.ones(D), None
            else:
                mu0, invcov0 = pu.gaussian_problem(D, dense=(like == "dense"))
                sig = np.sqrt(np.diag(np.linalg.inv(invcov0)))
                self.mu = 5.0 * sig + 0.1 * rs.randn(D)                # (the box lies right of 0: a log-uniform generator covers it)
                self.precision = invcov0 if like == "dense" else np.diag(invcov0).copy()
            centre, half = self.mu.copy(), 4.0 * sig
            self.prior = box_spec(centre - half, centre + half)
        self.lo, self.hi, self.sig, self.centre, self.half = self.prior["lo"], self.prior["hi"], sig, centre, half
        ent = []
        for d in range(D):
            c, h = centre[d], half[d]
            kind = {"box": "uniform", "mixed": ("uniform", "normal", "log_uniform", "normal")[d % 4],
                    "normal_lu": ("normal", "log_uniform")[d % 2], "uniform_normal": ("uniform", "normal")[d % 2]}[gen]
            if kind == "log_uniform" and c - 0.95 * h <= 0.0:       # (a coordinate whose start reaches 0: no log-uniform generator)
                kind = "uniform"
            if gen == "box":
                ent.append(("uniform", self.lo[d], self.hi[d]))
            elif kind == "uniform":                 # inside the prior, but: coordinate 0 NARROWER than the start on its lower side (old points
                ent.append(("uniform", c - (0.6 if d == 0 else 0.95) * h, c + (1.15 if d == 4 else 0.95) * h))      # outside), coordinate 4 wider than a box prior
            elif kind == "normal":
                ent.append(("normal", c + 0.2 * h * rs.uniform(-1, 1), 0.35 * h))
            else:
                a = max(c - 0.9 * h, 0.02 * h)
                ent.append(("log_uniform", a, max(c + (1.1 if d == 2 else 0.9) * h, 4.0 * a)))
        self.gen = pt.make_spec(ent)

    def loglike(self, x):
        if self.like_kind == "dense":
            return orc.gaussian_log_like(x, self.mu, self.precision)
        if self.like_kind == "diag":
            return orc.gaussian_diag_log_like(x, self.mu, self.precision)
        return orc.rosenbrock_log_like(x)

    def x0(self, T, W):
        """Spread as widely as the generator, not as the posterior: an independence proposal is accepted where it improves on the
        walker it meets, which a walker that starts far out lets happen on every rung within a few iterations at any width."""
        rs = np.random.RandomState(77)
        return self.centre + 0.9 * self.half * rs.uniform(-1.0, 1.0, size=(T, W, self.D))

    def containers(self):
        """(prior, generator) as ``eryn_amd.prior.ProbDistContainer``s."""
        return container_of(self.prior), container_of(self.gen)


def container_of(spec):
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, UniformDistribution
    out = {}
    for d, k in enumerate(spec["kind"]):
        if k == pt.NORMAL:
            out[d] = NormalDistribution(spec["c0"][d], spec["c1"][d])
        elif k == pt.LOG_UNIFORM:
            out[d] = LogUniformDistribution(spec["lo"][d], spec["hi"][d])
        else:
            out[d] = UniformDistribution(spec["lo"][d], spec["hi"][d])
    return ProbDistContainer(out)


def case(T, W, D, like, prior, gen, weight=0.5, iters=8):
    return dict(T=T, W=W, D=D, like=like, prior=prior, gen=gen, weight=weight, iters=iters)


# the issue's table: the smallest shapes at which each mechanism can go wrong
CASES = {
    "3x40x4_dense_terms": case(3, 40, 4, "dense", "terms", "mixed"),                 # padded to 8, NW = 4, one ragged tile, by-field state
    "3x33x11_diag_box_genbox": case(3, 33, 11, "diag", "box", "box"),   # odd W, pad to 16, a factor that cancels to the bit
    "4x72x16_diag_box": case(4, 72, 16, "diag", "box", "mixed"),     # record mode, a tile of 8
    "2x136x32_dense_box": case(2, 136, 32, "dense", "box", "normal_lu"),   # matrix pipe, two full tiles + 8
    "2x64x64_dense_terms": case(2, 64, 64, "dense", "terms", "mixed"),      # all three sums through the term tile
    "2x65x128_rosen_box": case(2, 65, 128, "rosen", "box", "uniform_normal"),   # the D = 128 LDS budget, a tile of one walker
    "2x65x128_dense_terms": case(2, 65, 128, "dense", "terms", "mixed"),    # ... with all three sums through the one tile that fits there
    "1x64x24_dense_box": case(1, 64, 24, "dense", "box", "mixed", weight=1.0),       # untempered, pad to 32, no stretch iteration
    # walker records (hens_step packs them where W is a multiple of the block-balanced labelling's column block, 128 / T for these
    # ladders: none of the shapes above is): {L, P} read and written in the records by slot, the stretch iterations on the
    # one-launch / two-launch record kernels round the move
    "4x64x16_diag_box_records": case(4, 64, 16, "diag", "box", "mixed"),
    "2x128x32_dense_box_records": case(2, 128, 32, "dense", "box", "normal_lu"),
    "2x128x64_dense_box_records": case(2, 128, 64, "dense", "box", "mixed"),
}
RECORDS = [k for k in CASES if k.endswith("_records")]
SEED = 2024


def case_problem(c):
    return DistProblem(c["D"], c["like"], c["prior"], c["gen"])


class Counts:
    """Coverage of a replayed or free-running case, from the SPECIFICATION's side."""

    def __init__(self, T):
        self.accepted = np.zeros(T, dtype=int)
        self.inf_prior = self.old_outside = self.old_outside_accepted = self.knives = self.moves = 0

    def add(self, keep, factors, info):
        from tests.parity_utils import knife_edge
        self.moves += 1
        self.accepted += keep.sum(axis=1)
        self.inf_prior += int(np.isinf(info["logp"]).sum())
        out = np.isneginf(factors)
        self.old_outside += int(out.sum())
        self.old_outside_accepted += int((out & keep).sum())
        with np.errstate(divide="ignore"):
            self.knives += int(knife_edge(info["lnpdiff"], np.log(info["u_acc"])).sum())


def assert_coverage(cnt, prob, x0, spare=1, what=""):
    print(f"{what}: {cnt.moves} move iterations, accepted per rung {cnt.accepted.tolist()}, -inf prior {cnt.inf_prior}, old outside the generator "
          f"{cnt.old_outside}, knife-edge decisions {cnt.knives}")
    D = prob.D
    assert (cnt.accepted >= spare).all(), f"{what}: a rung without an accepted proposal of the move"
    gen_exceeds = bool(np.any((prob.gen["lo"] < prob.prior["lo"]) | (prob.gen["hi"] > prob.prior["hi"])))
    if gen_exceeds:
        assert cnt.inf_prior >= spare, f"{what}: no proposal with a -inf prior"
    start_exceeds = bool(np.any(~np.isfinite(pt.log_prior(prob.gen, x0.reshape(-1, D)))))
    if start_exceeds:
        assert cnt.old_outside >= spare, f"{what}: no old point outside the generator"
    assert cnt.old_outside_accepted == 0, f"{what}: an old point outside the generator was moved"
    assert cnt.knives == 0, f"{what}: {cnt.knives} accept decisions on the knife edge"


def pt_tail(st, ref, adaptive=True, lag=10000, nu=100):
    """The PT cascade and the ladder adaptation that end every iteration (tests/replay_utils.oracle_iteration's tail)."""
    T, W, _ = st.x.shape
    if st.betas is not None and T > 1:
        _, sw = orc.pt_sweep(st.x, st.L, st.P, st.betas, ref["iperm"], ref["i1perm"], ref["u_swap"])
        st.swaps_last = sw
        st.swaps_total += sw
        if adaptive:
            st.betas = orc.adapt_ladder(st.betas, sw, W, st.time, lag, nu)
            st.time += 1


def free_run(c, seed=SEED):
    """The case on the specification alone with the production draws of ``seed`` - stretch iterations through the pinned oracle with
    NumPy draws of their own (the CPU sizing needs the move's iterations, not the stretch move's exact ones): -> (counts, problem, x0)."""
    prob = case_problem(c)
    T, W, D = c["T"], c["W"], c["D"]
    x = prob.x0(T, W).copy()
    P = pt.log_prior(prob.prior, x.reshape(-1, D)).reshape(T, W)
    assert np.isfinite(P).all(), "a start outside the prior's support"
    L = prob.loglike(x.reshape(-1, D)).reshape(T, W)
    betas = orc.make_ladder(D, ntemps=T) if T > 1 else None
    x0 = x.copy()
    cnt = Counts(T)
    rs = np.random.RandomState(5)
    for it in range(c["iters"]):
        if pd.is_mh(seed, it, c["weight"]):
            q, _, _ = dist_draws(seed, it, T, W, prob.gen)
            info = {}
            _, _, _, keep, fac = dist_step(x, L, P, betas, q, accept_uniforms(seed, it, T, W), prob.prior, prob.gen, prob.loglike, info=info)
            cnt.add(keep, fac, info)
        if betas is not None:
            iperm = np.stack([rs.permutation(W) for _ in range(T - 1)])
            i1perm = np.stack([rs.permutation(W) for _ in range(T - 1)])
            orc.pt_sweep(x, L, P, betas, iperm, i1perm, rs.uniform(size=(T - 1, W)))
    return cnt, prob, x0


# ---- the fixtures from the real reference (tests/golden/make_golden_dist.py -> tests/golden/distgen/) ------------------------------------
FIXTURES = ["dg1_mix", "dg2_prior_draws"]
PERIODIC_FIXTURES = ["dg3_periodic_mix"]      # both moves of the mix hold a PeriodicContainer (``period`` [D]): tests/test_move_interactions.py


def load_fixture(name):
    import os
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "distgen", name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_iteration(fx, it):
    """Iteration ``it`` of a fixture as one dict: what every iteration records, and its move's own records by their plain names."""
    kind = int(fx["kind"][it])
    group = "dist_" if kind else "stretch_"
    j = int(np.sum(fx["kind"][:it] == kind))
    out = {k[4:]: v[it] for k, v in fx.items() if k.startswith("all_")}
    out.update({k[len(group):]: v[j] for k, v in fx.items() if k.startswith(group)})
    out["is_dist"] = bool(kind)
    return out


def fixture_specs(fx):
    """(prior, generator) as term specifications: the reference's constructor arguments, its log_uniform construction applied."""
    return (pt.make_spec(rpt.fixture_entries(fx["prior_kind"], fx["prior_p0"], fx["prior_p1"])),
            pt.make_spec(rpt.fixture_entries(fx["gen_kind"], fx["gen_p0"], fx["gen_p1"])))


def fixture_containers(fx):
    """The same through eryn_amd.prior's own names - the calls a user moves over from a reference script."""
    return (rpt.fixture_container(fx["prior_kind"], fx["prior_p0"], fx["prior_p1"]),
            rpt.fixture_container(fx["gen_kind"], fx["gen_p0"], fx["gen_p1"]))


def fixture_loglike(fx):
    mu, invcov = fx["mu"], fx["invcov"]
    return lambda x: orc.gaussian_log_like(x, mu, invcov)
