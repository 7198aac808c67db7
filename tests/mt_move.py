"""The specification of the multiple-try independence move (host only, NumPy): what include/hipensemble.h's
hens_set_mt_dist_proposal / hens_mt_dist_step and the k_mt_dist launch of hens_step compute, stated once on tests/prior_terms.py
(one term, one row), tests/dist_move.py (the generator's draws, the problems) and the oracle's ``compute_log_like`` /
``tempered_log_posterior`` / ``pt_sweep`` / ``adapt_ladder`` (imported, not edited).

The move (mtdistgen.py:7-136 over multipletry.py:238-514 under mh.py:56-193), ``independent=True``, single branch, every leaf
active.  N = T W walkers, K = num_try, beta the walker's rung (1 without a ladder).  With logq the generator's log-density
(tests/prior_terms.log_prior: ascending from 0.0, -inf outside a support):

    lq_k = logq(y_k);  lp_k = prior(y_k);  ll_k = like(y_k) where lp_k is finite, ``fill`` elsewhere
    logP_k = beta ll_k + lp_k;  w_k = logP_k - lq_k                                        (multipletry.py:45,221-223)
    lsw = max w + log(sum exp(w - max w))                                                  (multipletry.py:25-33)
    p = exp(w - lsw);  j = argmax(cumsum(p) > u_pick)     (0 when no entry exceeds it)     (multipletry.py:51-57)
    w'_k = w_k (k != j);  w'_j = (beta L_old + P_old) - logq(x_old);  aux_lsw = logsumexp(w')
    factors = ((aux_logP_j - aux_lsw) - alq_j + alq_j) - ((logP_j - lsw) - lq_j + lq_j)    (multipletry.py:472-476)
    keep = factors + tempered(ll_j, lp_j) - tempered(L, P) > log u_acc                     (mh.py:150-171)

The reference evaluates the likelihood of a try whose prior is -inf; this specification skips and fills it as the device does: such a
try has weight -inf either way and can be "picked" only through the j = 0 fallback, which gives a NaN lnpdiff and a rejection.

The draws of the production path
--------------------------------
Coordinate d of try k of walker wid = global rung * W + walker in iteration ``it``: tests/dist_move's call with counter word 3 =
PURPOSE_DIST | d << 8 | k << 16 (try 0 is DistributionGenerate's point), turned into a value by ``dist_move.value_of`` with its bound
E.  The pick uniform: ONE call, counter (it lo, it hi, wid, PURPOSE_MT_PICK = 15), its first two words as a 53-bit uniform (the
construction of tests/production_draws.mh_uniform).  The accept uniform is the MH move's own.

Exact arithmetic and the bounds B
---------------------------------
Exact values are the formulas above in long double on the same doubles: y, x_old, L_old, P_old, beta, and ll_k as the oracle's
float64 likelihood (the parity tests grant the device's likelihood tests/tolerance_log.RTOL_L relative to it).  u = 2^-53.

Inputs.  A float64 evaluation forms w_k from lq_k and lp_k, each within tests/prior_terms.float64_bound (B_q, B_p) of its exact
value, and a likelihood within RTOL_L |ll_k|; the product, the sum and the difference round once each:

    e_k = beta RTOL_L |ll_k| + B_p(y_k) + B_q(y_k) + u (|beta ll_k| + |logP_k| + |w_k|)         (0 where w_k is -inf: exact)

Log-sum-exp.  lse(w) = max + log(sum exp(w - max)) is 1-Lipschitz in the sup norm of w, so the inputs' errors move it by at most
E_w = max_k e_k.  Its own evaluation, with d_k = w_k - max (one rounding, u |d_k|), ``exp`` and ``log`` within 1 ulp (2 u relative,
as tests/prior_terms assumes of ``log``), and a sum of K non-negative terms in ANY order within (K + 2) u relative:

    r_S = sum_k exp(d_k) (u |d_k| + 2 u) / S + (K + 2) u             relative error of S = sum exp(d_k) >= 1
    B_lsw = E_w + r_S + 2 u |log S| + u |lsw|                        (d log S = dS / S; the last addition rounds once)

(first order, as B_P is).  aux_lsw likewise with the auxiliary entry's e'_j = B_q(x_old) + u (|beta L_old| + |aux_logP_j| + |w'_j|).

Factor.  In exact arithmetic the added and subtracted log-densities cancel, F* = (aux_logP_j - aux_lsw) - (logP_j - lsw).  In
float64 t1 = aux_logP_j - aux_lsw carries u (|beta L_old| + |aux_logP_j|) + B_aux + u |t1|, and (t1 - a) + a adds u |t1 - a| + u |t1|
whatever a's own error (the same double is subtracted and added); t2 = logP_j - lsw likewise with beta RTOL_L |ll_j| + B_p(y_j) +
u (|beta ll_j| + |logP_j|) + B_lsw; the last subtraction rounds once:

    B_F = [u (|beta L_old| + |aux_logP_j|) + B_aux + u (2 |t1| + |t1 - alq_j|)]
        + [beta RTOL_L |ll_j| + B_p(y_j) + u (|beta ll_j| + |logP_j|) + B_lsw + u (2 |t2| + |t2 - lq_j|)] + u |F|

Where the specification's value is not finite (NaN: every weight -inf, a weight +inf, an old point outside the generator) the device's
must be the same non-finite value and the bound is not used.  The device is held to |value - exact| <= 1.0 B.

Knife edges.  p_k = exp(w_k - lsw) carries the relative error e_k + B_lsw + u |w_k - lsw| + 2 u and the running sum k roundings:

    B_c,k = sum_{i <= k} p_i (e_i + B_lsw + u |w_i - lsw| + 2 u) + (k + 1) u c_k

A pick is on the knife edge when some running sum c_k lies within B_c,k of u_pick (``pick_knife``); accept decisions use
tests/parity_utils.knife_edge.  The GPU cases tolerate neither: their seeds are chosen so that the specification alone has none.
"""
import os

import numpy as np

from oracle import eryn_oracle as orc
from tests import dist_move as dm
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import tolerance_log as tol

LD = np.longdouble
U = pt.U
PURPOSE_MT_PICK = 15
MAX_TRY = 64


def logsumexp(a):
    """multipletry.py:25-33 over the last axis of a[N, K]."""
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = np.max(a, axis=-1)
        ds = a - mx[:, None]
        return mx + np.log(np.exp(ds).sum(axis=-1))


def mt_step(x, L, P, betas, q, u_pick, u_acc, prior, gen, loglike, fill=-1e300, info=None):
    """One full-ensemble proposal of the move with the tries q[T, W, K, D]; mutates x, L, P in place and returns
    (keep[T, W], pick[T, W], lsw[T, W], aux_lsw[T, W], factors[T, W]).  ``info``: a dict that receives the intermediates."""
    T, W, D = x.shape
    N = T * W
    q = np.asarray(q, dtype=np.float64).reshape(N, -1, D)
    K = q.shape[1]
    beta = np.ones(N) if betas is None else np.repeat(np.asarray(betas, dtype=np.float64), W)
    rows = q.reshape(-1, D)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        lq = pt.log_prior(gen, rows).reshape(N, K)                                # mtdistgen.py:77-79
        lp = pt.log_prior(prior, rows).reshape(N, K)                              # multipletry.py:344
        ll = orc.compute_log_like(q, lp, loglike, fill=fill)                      # multipletry.py:334 (skipped and filled at a -inf prior)
        logP = beta[:, None] * ll + lp                                            # multipletry.py:221-223
        w = logP - lq                                                             # multipletry.py:45
        lsw = logsumexp(w)
        c = np.exp(w - lsw[:, None]).cumsum(1)                                    # multipletry.py:51-57
        pick = (c > np.asarray(u_pick, dtype=np.float64).reshape(N)[:, None]).argmax(1)
        at = (np.arange(N), pick)
        alq = pt.log_prior(gen, x.reshape(N, D))                                  # multipletry.py:387
        aux_logP = beta * L.reshape(N) + P.reshape(N)                             # multipletry.py:406-410
        w_aux = w.copy()
        w_aux[at] = aux_logP - alq                                                # multipletry.py:413-417
        aux_lsw = logsumexp(w_aux)
        factors = ((aux_logP - aux_lsw) - alq + alq) - ((logP[at] - lsw) - lq[at] + lq[at])   # multipletry.py:472-476
        logl, logp = ll[at].reshape(T, W), lp[at].reshape(T, W)                   # mh.py:150-153
        factors = factors.reshape(T, W)
        lnpdiff = factors + orc.tempered_log_posterior(logl, logp, betas) - orc.tempered_log_posterior(L, P, betas)    # mh.py:157-168
        keep = lnpdiff > np.log(np.asarray(u_acc, dtype=np.float64).reshape(T, W))   # mh.py:171
    if info is not None:
        info.update(q=q.reshape(T, W, K, D), ll=ll, lp=lp, lq=lq, logP=logP, w=w, c=c, alq=alq, aux_logP=aux_logP, logl=logl, logp=logp,
                    lnpdiff=lnpdiff, u_acc=np.asarray(u_acc, dtype=np.float64).reshape(T, W),
                    u_pick=np.asarray(u_pick, dtype=np.float64).reshape(T, W), x_old=x.copy(), L_old=L.copy(), P_old=P.copy())
    new_logp = logp.copy()
    new_logp[np.isinf(new_logp)] = 0.0                                            # move.py:513-532
    qj = q[at].reshape(T, W, D)
    L[...] = np.where(keep, logl, L)
    P[...] = np.where(keep, new_logp, P)
    x[keep] = qj[keep]
    return keep, pick.reshape(T, W), lsw.reshape(T, W), aux_lsw.reshape(T, W), factors


# ---- the draws of the production path ------------------------------------------------------------------------------------------------
def mt_words(seed, it, T, W, d, K, rung_begin=0):
    """The four words [T, W, K] of the calls that draw coordinate d of tries 0 .. K - 1 (hens_dist.h: dist_draw with its try)."""
    wid = ((rung_begin + np.arange(T))[:, None] * W + np.arange(W)[None, :])[:, :, None]
    return pd.philox4x32_10(it & 0xFFFFFFFF, it >> 32, wid, dm.PURPOSE_DIST | (d << 8) | (np.arange(K)[None, None, :] << 16), seed & 0xFFFFFFFF, seed >> 32)


def mt_draws(seed, it, T, W, K, gen, rung_begin=0):
    """(X float64, X* long double, E float64), each [T, W, K, D]: the tries iteration ``it`` draws."""
    D = len(gen["kind"])
    X, Xs, E = np.zeros((T, W, K, D)), np.zeros((T, W, K, D), dtype=LD), np.zeros((T, W, K, D))
    for d in range(D):
        X[..., d], Xs[..., d], E[..., d] = dm.value_of(gen, d, mt_words(seed, it, T, W, d, K, rung_begin))
    return X, Xs, E


def pick_uniforms(seed, it, T, W, rung_begin=0):
    wid = (rung_begin + np.arange(T))[:, None] * W + np.arange(W)[None, :]
    d = pd._call(seed, it, wid, PURPOSE_MT_PICK)
    return pd.u01(d[0], d[1])


accept_uniforms = dm.accept_uniforms


# ---- exact arithmetic and the bounds ------------------------------------------------------------------------------------------------------
def _lse_exact(ws, e):
    """(lse* long double [N], B float64 [N]) of exact weights ws[N, K] whose float64 counterparts carry e[N, K]."""
    K = ws.shape[1]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = ws.max(axis=1)
        d = ws - m[:, None]
        ex = np.exp(d)
        S = ex.sum(axis=1)
        lse = m + np.log(S)
        live = ex > 0
        Ew = np.where(live, e, 0.0).max(axis=1)
        rS = np.where(live, ex * (U * np.abs(np.where(live, d, 0)) + 2 * U), 0).sum(axis=1) / S + (K + 2) * U
        B = Ew + rS + 2 * U * np.abs(np.log(S)) + U * np.abs(lse)
    return lse, np.where(np.isfinite(lse), B, 0.0).astype(np.float64)


def exact_mt(info, pick, betas, prior, gen, rtol_l=tol.RTOL_L):
    """Exact lsw, aux_lsw, factors (long double [T, W]) of the proposals ``info`` describes (``mt_step``'s) with the picks ``pick``,
    and the bounds B_lsw, B_aux, B_F [T, W], B_c [T, W, K] (float64) of the module's docstring."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    q = info["q"]
    T, W, K, D = q.shape
    N = T * W
    rows = q.reshape(-1, D)
    xo = info["x_old"].reshape(N, D)
    beta = (np.ones(N) if betas is None else np.repeat(np.asarray(betas, dtype=np.float64), W)).astype(LD)
    at = (np.arange(N), pick.reshape(N))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lq, bq = pt.exact_log_prior(gen, rows).reshape(N, K), pt.float64_bound(gen, rows).reshape(N, K)
        lp, bp = pt.exact_log_prior(prior, rows).reshape(N, K), pt.float64_bound(prior, rows).reshape(N, K)
        ll = info["ll"].astype(LD)
        bll = beta[:, None] * ll
        logP = bll + lp
        w = logP - lq
        finw = np.isfinite(w)
        z = lambda a, ok: np.where(ok, np.abs(a), 0).astype(np.float64)       # noqa: E731  (magnitudes, 0 where the value is not finite)
        e = np.where(finw, z(bll, finw) * rtol_l + bp + bq + U * (z(bll, finw) + z(logP, finw) + z(w, finw)), 0.0)
        lsw, B_lsw = _lse_exact(w, e)
        # the auxiliary set
        alq, baq = pt.exact_log_prior(gen, xo), pt.float64_bound(gen, xo)
        bL = beta * info["L_old"].reshape(N).astype(LD)
        aP = bL + info["P_old"].reshape(N).astype(LD)
        wj = aP - alq
        w2, e2 = w.copy(), e.copy()
        w2[at] = wj
        finj = np.isfinite(wj)
        e2[at] = np.where(finj, baq + U * (z(bL, finj) + z(aP, finj) + z(wj, finj)), 0.0)
        aux, B_aux = _lse_exact(w2, e2)
        t1, t2 = aP - aux, logP[at] - lsw
        F = t1 - t2
        fin = np.isfinite(F) & np.isfinite(lq[at]) & np.isfinite(alq)
        a = lambda v: np.where(fin, np.abs(v), 0).astype(np.float64)           # noqa: E731
        B_F = (U * (a(bL) + a(aP)) + B_aux + U * (2 * a(t1) + a(t1 - alq))
               + a(bll[at]) * rtol_l + bp[at] + U * (a(bll[at]) + a(logP[at])) + B_lsw + U * (2 * a(t2) + a(t2 - lq[at])) + U * a(F))
        # the running sums of the pick
        p = np.exp(w - lsw[:, None])
        rel = e + B_lsw[:, None] + U * np.where(finw, np.abs(w - lsw[:, None]), 0).astype(np.float64) + 2 * U
        c = p.cumsum(axis=1)
        B_c = (np.where(p > 0, p * rel, 0).cumsum(axis=1) + (np.arange(K) + 1) * U * c).astype(np.float64)
    return dict(lsw=lsw.reshape(T, W), aux_lsw=aux.reshape(T, W), factors=F.reshape(T, W), B_lsw=B_lsw.reshape(T, W),
                B_aux=B_aux.reshape(T, W), B_F=np.where(fin, B_F, 0.0).reshape(T, W), B_c=np.nan_to_num(B_c, nan=0.0).reshape(T, W, K),
                c=c.reshape(T, W, K))


def pick_knife(c, u_pick, B):
    """[...] bool: some running sum c[..., K] lies within its bound B[..., K] of the pick uniform u_pick[...]."""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(c, dtype=np.float64) - np.asarray(u_pick)[..., None]) <= B).any(axis=-1)


def _held(val, exact, B, what):
    """max |val - exact| / B over the finite entries of the specification's value; non-finite ones must sit where it has them."""
    exact64 = exact.astype(np.float64)
    fin = np.isfinite(exact64)
    assert np.array_equal(np.isfinite(val), fin), f"{what}: a non-finite value where the specification has a finite one (or the reverse)"
    assert np.array_equal(val[~fin], exact64[~fin], equal_nan=True), f"{what}: the non-finite values differ"
    if not fin.any():
        return 0.0
    err = np.abs(val[fin].astype(LD) - exact[fin]).astype(np.float64)
    assert (B[fin] > 0).all(), f"{what}: an empty bound"
    return float(np.max(err / B[fin]))


def assert_sums(lsw, aux_lsw, factors, ex, what=""):
    """The issue's bar: lsw, aux_lsw and factors within 1.0 B of exact arithmetic, non-finite values exactly where it has them.
    Returns the three measured ratios; they are printed and logged under the running test (tests/tolerance_log.py)."""
    r = (_held(lsw, ex["lsw"], ex["B_lsw"], what + " lsw"), _held(aux_lsw, ex["aux_lsw"], ex["B_aux"], what + " aux_lsw"),
         _held(factors, ex["factors"], ex["B_F"], what + " factors"))
    print(f"{what}: |lsw - lsw*| / B <= {r[0]:.3f}, |aux_lsw - aux_lsw*| / B <= {r[1]:.3f}, |F - F*| / B_F <= {r[2]:.3f}")
    ent = tol._seen.setdefault(tol._test_name(), {"max_rel_L": 0.0, "rtol": tol.RTOL_L, "comparisons": 0, "values": 0})
    ent["mt_ratio_lsw"] = max(ent.get("mt_ratio_lsw", 0.0), r[0])
    ent["mt_ratio_aux_lsw"] = max(ent.get("mt_ratio_aux_lsw", 0.0), r[1])
    ent["mt_ratio_factors"] = max(ent.get("mt_ratio_factors", 0.0), r[2])
    assert max(r) <= 1.0, f"{what}: a sum misses its bound: lsw {r[0]:.3f} B, aux_lsw {r[1]:.3f} B, factors {r[2]:.3f} B_F"
    return r


# ---- the cases of the GPU tests -----------------------------------------------------------------------------------------------------------
def case(T, W, D, K, like, prior, gen, weight=0.5, iters=8):
    return dict(T=T, W=W, D=D, K=K, like=like, prior=prior, gen=gen, weight=weight, iters=iters)


# the issue's table: the smallest shapes at which each mechanism can go wrong.  KP: the power of two a walker's tries are padded to,
# G = 64 / KP walkers per workgroup.
CASES = {
    "3x40x4_k5_dense_terms": case(3, 40, 4, 5, "dense", "terms", "mixed"),          # pad to 8, KP = 8 with dead rows, G = 8, prior terms, by-field state
    "3x33x11_k2_diag_box_genbox": case(3, 33, 11, 2, "diag", "box", "box"),        # G = 32: a ragged second workgroup of one walker, odd W
    "4x64x16_k3_diag_box": case(4, 64, 16, 3, "diag", "box", "mixed"),              # walker records under hens_step, KP = 4 with one dead row
    "2x128x32_k25_dense_box": case(2, 128, 32, 25, "dense", "box", "normal_lu"),    # matrix pipe, KP = 32, walker records under hens_step
    "2x9x64_k64_dense_terms": case(2, 9, 64, 64, "dense", "terms", "mixed", weight=1.0),        # one walker per workgroup, all three sums through the one term tile
    "2x5x128_k64_rosen_box": case(2, 5, 128, 64, "rosen", "box", "uniform_normal", weight=1.0),  # the D = 128 LDS budget
    "2x5x128_k3_dense_terms": case(2, 5, 128, 3, "dense", "terms", "mixed", weight=1.0),         # ... dense with prior terms
    "1x20x24_k7_dense_box": case(1, 20, 24, 7, "dense", "box", "mixed", weight=1.0),            # untempered, pad to 32
    "2x3x8_k16_diag_box": case(2, 3, 8, 16, "diag", "box", "mixed", weight=1.0),                # W < G
}
RECORDS = ["4x64x16_k3_diag_box", "2x128x32_k25_dense_box"]     # hens_step packs walker records here (W a multiple of 128 / T)
SEED = 2025
FORCED_PROPOSALS = 3


def case_problem(c):
    return dm.DistProblem(c["D"], c["like"], c["prior"], c["gen"])


def start_of(prob, T, W):
    """(x, L, P, betas) of a case's start on the specification's side."""
    D = prob.D
    x = prob.x0(T, W).copy()
    P = pt.log_prior(prob.prior, x.reshape(-1, D)).reshape(T, W)
    assert np.isfinite(P).all(), "a start outside the prior's support"
    L = prob.loglike(x.reshape(-1, D)).reshape(T, W)
    return x, L, P, (orc.make_ladder(D, ntemps=T) if T > 1 else None)


def forced_inputs(c, prob, n, seed=SEED):
    """(q[T, W, K, D], u_pick, u_acc) of teacher-forced proposal ``n`` of a case: the production draws of iteration n, and - a
    caller's points may lie anywhere - in every seventh walker one try with one coordinate moved out of the generator's support
    (where it has one) or far out of the prior's."""
    T, W, D, K = c["T"], c["W"], c["D"], c["K"]
    q, _, _ = mt_draws(seed, n, T, W, K, prob.gen)
    rs = np.random.RandomState(31 + n)
    for t in range(T):
        for w in range(n, W, 7):
            d, k = int(rs.randint(D)), int(rs.randint(K))
            lo, hi = prob.gen["lo"][d], prob.gen["hi"][d]
            q[t, w, k, d] = hi + 0.25 * (hi - lo) if np.isfinite(hi) else prob.centre[d] + 50.0 * prob.half[d]
    return q, rs.rand(T, W), rs.rand(T, W)


class Counts:
    """Coverage of a teacher-forced, replayed or free-running case, from the SPECIFICATION's side."""

    def __init__(self, T):
        self.accepted = np.zeros(T, dtype=int)
        self.moves = self.picks_beyond_0 = self.inf_prior = self.old_outside = self.old_outside_accepted = 0
        self.knife_accepts = self.knife_picks = 0

    def add(self, keep, pick, info, ex):
        from tests.parity_utils import knife_edge
        self.moves += 1
        self.accepted += keep.sum(axis=1)
        self.picks_beyond_0 += int((pick != 0).sum())
        self.inf_prior += int(np.isinf(info["lp"]).sum())
        out = np.isneginf(info["alq"]).reshape(keep.shape)
        self.old_outside += int(out.sum())
        self.old_outside_accepted += int((out & keep).sum())
        with np.errstate(divide="ignore"):
            self.knife_accepts += int(knife_edge(info["lnpdiff"], np.log(info["u_acc"])).sum())
        self.knife_picks += int(pick_knife(ex["c"], info["u_pick"], ex["B_c"]).sum())


def assert_coverage(cnt, prob, x0, spare=1, what=""):
    print(f"{what}: {cnt.moves} move iterations, accepted per rung {cnt.accepted.tolist()}, picks other than try 0 {cnt.picks_beyond_0}, "
          f"-inf-prior tries {cnt.inf_prior}, old points outside the generator {cnt.old_outside}, knife-edge picks {cnt.knife_picks} / "
          f"accepts {cnt.knife_accepts}")
    D = prob.D
    assert (cnt.accepted >= spare).all(), f"{what}: a rung without an accepted proposal of the move"
    assert cnt.picks_beyond_0 >= spare, f"{what}: no pick other than try 0"
    if bool(np.any((prob.gen["lo"] < prob.prior["lo"]) | (prob.gen["hi"] > prob.prior["hi"]))):
        assert cnt.inf_prior >= spare, f"{what}: no try with a -inf prior"
    if bool(np.any(~np.isfinite(pt.log_prior(prob.gen, x0.reshape(-1, D))))):
        assert cnt.old_outside >= spare, f"{what}: no old point outside the generator"
    assert cnt.old_outside_accepted == 0, f"{what}: an old point outside the generator was moved"
    assert cnt.knife_picks == 0 and cnt.knife_accepts == 0, f"{what}: {cnt.knife_picks} picks / {cnt.knife_accepts} accept decisions on the knife edge"


def forced_run(c, seed=SEED):
    """The teacher-forced part of a case on the specification alone -> (counts, problem, x0)."""
    prob = case_problem(c)
    T, W = c["T"], c["W"]
    x, L, P, betas = start_of(prob, T, W)
    x0 = x.copy()
    cnt = Counts(T)
    for n in range(FORCED_PROPOSALS):
        q, up, ua = forced_inputs(c, prob, n, seed)
        info = {}
        keep, pick, _, _, _ = mt_step(x, L, P, betas, q, up, ua, prob.prior, prob.gen, prob.loglike, info=info)
        cnt.add(keep, pick, info, exact_mt(info, pick, betas, prob.prior, prob.gen))
    return cnt, prob, x0


def free_run(c, seed=SEED):
    """The replayed part of a case on the specification alone with the production draws of ``seed`` - the stretch iterations are
    left out (the CPU sizing needs the move's iterations), the sweeps run on NumPy draws of their own -> (counts, problem, x0)."""
    prob = case_problem(c)
    T, W, K = c["T"], c["W"], c["K"]
    x, L, P, betas = start_of(prob, T, W)
    x0 = x.copy()
    cnt = Counts(T)
    rs = np.random.RandomState(5)
    for it in range(c["iters"]):
        if pd.is_mh(seed, it, c["weight"]):
            q, _, _ = mt_draws(seed, it, T, W, K, prob.gen)
            info = {}
            keep, pick, _, _, _ = mt_step(x, L, P, betas, q, pick_uniforms(seed, it, T, W), accept_uniforms(seed, it, T, W), prob.prior,
                                          prob.gen, prob.loglike, info=info)
            cnt.add(keep, pick, info, exact_mt(info, pick, betas, prob.prior, prob.gen))
        if betas is not None:
            iperm = np.stack([rs.permutation(W) for _ in range(T - 1)])
            i1perm = np.stack([rs.permutation(W) for _ in range(T - 1)])
            orc.pt_sweep(x, L, P, betas, iperm, i1perm, rs.uniform(size=(T - 1, W)))
    return cnt, prob, x0


# ---- the fixtures from the real reference (tests/golden/make_golden_mt.py -> tests/golden/mt/) ---------------------------------------------
FIXTURES = ["mt1_mix", "mt2_prior_tries"]
PERIODIC_FIXTURES = ["mt3_periodic_mix"]      # both moves of the mix hold a PeriodicContainer (``period`` [D]): tests/test_move_interactions.py
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mt")


def load_fixture(name):
    with np.load(os.path.join(FIXTURE_DIR, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_iteration(fx, it):
    """Iteration ``it`` of a fixture as one dict (tests/dist_move.fixture_iteration with this move's group name)."""
    kind = int(fx["kind"][it])
    group = "mt_" if kind else "stretch_"
    j = int(np.sum(fx["kind"][:it] == kind))
    out = {k[4:]: v[it] for k, v in fx.items() if k.startswith("all_")}
    out.update({k[len(group):]: v[j] for k, v in fx.items() if k.startswith(group)})
    out["is_mt"] = bool(kind)
    return out


fixture_specs, fixture_containers, fixture_loglike = dm.fixture_specs, dm.fixture_containers, dm.fixture_loglike
