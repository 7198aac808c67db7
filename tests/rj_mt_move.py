"""The specification of the multiple-try birth / death move on leaf-packing records (host only, NumPy): what include/hipensemble.h's
hens_rj_set_mt_proposal / hens_rj_mt_bd_step and the k_rj_mt launch of hens_rj_step compute, stated once on the oracle's
``compute_log_prior`` / ``compute_log_like`` / ``fix_logp_gibbs`` / ``update`` and its cascade (oracle/eryn_oracle_rj.py, imported, not
edited), on tests/mt_move.py (log-sum-exp, its bound, the pick's knife edge) and on tests/prior_terms.py / tests/rj_prior_terms.py
(one leaf's density, a state's log-prior, exact arithmetic).

The move (mtdistgenrj.py:7-189 over multipletry.py:238-514 - the ``elif self.rj`` branch - and multipletry.py:597-776, inside
ReversibleJumpMove.propose, rj.py:145-388) acts on ONE branch per proposal.  N = T W walkers, K = num_try, beta the walker's rung;
logq the generator's log-density of one leaf, lp(.) the log-prior of a whole walker, ll(.) its log-likelihood.  Coin, edge rule and
leaf slot are DistributionGenerateRJ's (distgenrj.py:63-112): change in {-1, +1}, leaf.

    birth walker   base = the walker;                         ll_in = L, lp_in = P;         tries y_0 .. y_{K-1} from the generator
    death walker   base = the walker without the dying leaf;  ll_in, lp_in evaluated on it; try 0 IS the dying leaf (multipletry.py:
                   315-317), tries 1 .. K-1 fresh draws into the same slot
    per try k      lp_k = lp(base + y_k in slot ``leaf``);  ll_k = ll(base + y_k), ``fill`` where lp_k = -inf (not evaluated, as
                   tests/mt_move.py skips it)
                   lq_k = logq(y_k) + lp_in                                                                  (multipletry.py:350-351)
                   logP_k = beta ll_k + lp_k;  w_k = logP_k - lq_k                                           (multipletry.py:221-223, 45)
    lsw  = max w + log(sum exp(w - max w))                                                                   (multipletry.py:25-33)
    pick = argmax(cumsum(exp(w - lsw)) > u_pick), 0 on a death walker                                        (multipletry.py:51-57, 365)
    aux_logP = beta ll_in + lp_in;  aux_w = aux_logP - lp_in;  aux_lsw = logsumexp of K entries aux_w        (multipletry.py:419-431, 463)
    factors = ((aux_logP - aux_lsw) - a + a) - ((logP_pick - lsw) - lq_pick + lq_pick),  a = lp_in;  negated on a death walker
    proposed (logl, logp) = (ll_pick, lp_pick) on a birth, (ll_in, lp_in) on a death                         (multipletry.py:373-374, 481-482)

then ReversibleJumpMove.propose: + the edge factors (rj.py:236-270), fix_logp_gibbs on logp (rj.py:303), keep = factors + tempered(logl,
logp) - tempered(L, P) > log u_acc (rj.py:330-332), Move.update.  DistributionGenerateRJ's own -+ logq is NOT added.  Every weight -inf
gives lsw = NaN; a dying leaf outside the generator has lq_0 = -inf, w_0 = +inf, lsw = NaN: NaN factors, a rejection.

The draws.  rng="numpy" (the reference's order, pinned by tests/golden/rj_mt): the rj move's choice, the coins and the leaf choices from
R; ``generate_dist.rvs(size=(N, K))`` per parameter for ALL walkers, then the one ``rand(N)`` of the pick, both on the global stream;
``R.rand(T, W)``.  Production (hens_rj_step): walker wid = global rung * W + walker, a call = philox4x32_10(it lo, it hi, wid, key; seed
lo, seed hi); coin / selector / accept uniform are the plain move's calls (hens_rj_debug_draws); coordinate d of try k in ``branch``: key
PURPOSE_RJ_BIRTH | d << 8 | branch << 16 for k = 0 (the plain move's birth) and PURPOSE_RJ_TRY | d << 8 | k << 10 | branch << 16 for k >= 1,
turned into a value by tests/rj_prior_terms.birth_spec on the generator's terms; the pick uniform: u01 of the first two words of the call
keyed PURPOSE_RJ_PICK | branch << 16.

Exact arithmetic and the bounds B (derived as tests/mt_move.py derives its own; u = 2^-53)
------------------------------------------------------------------------------------------
Exact values are the formulas in long double on the same doubles: the tries, the record, L, P, beta, and ll_k / a death's ll_in as the
oracle's float64 likelihoods (a device likelihood is granted tests/tolerance_log.RTOL_L relative to them).  A walker's log-prior in
float64 lies within B_s = tests/rj_prior_terms.state_bound of its exact value; a birth's lp_in = P is data (bound 0).

Inputs.  lq_k = logq(y_k) + lp_in rounds ONCE more than tests/mt_move.py's lq (the addition):

    e_k = beta RTOL_L |ll_k| + B_s(base + y_k) + [B_q(y_k) + B_s(base) + u |lq_k|] + u (|beta ll_k| + |logP_k| + |w_k|)      (0 where w_k = -inf)

lsw: tests/mt_move._lse_exact on (w*, e): B_lsw = max e + r_S + 2 u |log S| + u |lsw|.
aux_lsw.  In exact arithmetic lp_in cancels: aux_w* = beta ll_in, aux_lsw* = beta ll_in + log K.  In float64 the same double is added and
subtracted: e_aux = beta RTOL_L |ll_in| (death: ll_in is evaluated) + u (|beta ll_in| + |aux_logP| + |aux_w|), and the sum of K EQUAL
entries exp(0) = 1 is exact - _lse_exact's (K + 2) u covers it with room - so B_aux = _lse_exact on K copies of (aux_w*, e_aux).
factors.  t1 = aux_logP - aux_lsw carries err(aux_logP) = beta RTOL_L |ll_in| + B_s(base) + u (|beta ll_in| + |aux_logP|), B_aux and
u |t1|; (t1 - a) + a adds u |t1 - a| + u |t1|; t2 = logP_j - lsw carries beta RTOL_L |ll_j| + B_s(base + y_j) + u (|beta ll_j| + |logP_j|),
B_lsw and u |t2|; (t2 - lq_j) + lq_j adds u |t2 - lq_j| + u |t2|; the last subtraction u |F|; the negation is exact:

    B_F = [err(aux_logP) + B_aux + u (2 |t1| + |t1 - lp_in|)] + [err(logP_j) + B_lsw + u (2 |t2| + |t2 - lq_j|)] + u |F|

Non-finite values of the specification must come back as the same non-finite values.  Knife edges: tests/mt_move.pick_knife on the
running sums' bound B_c (mt_move's, with this module's e), tests/parity_utils.knife_edge on the accept decision.
"""
import os

import numpy as np

from oracle import eryn_oracle_rj as orj
from tests import mt_move as mm
from tests import prior_terms as pt
from tests import rj_prior_terms as rpt
from tests import tolerance_log as tol
from tests.production_draws import philox4x32_10, u01

LD = np.longdouble
U = pt.U
PURPOSE_RJ_ACC, PURPOSE_RJ_BD, PURPOSE_RJ_BIRTH, PURPOSE_RJ_TRY, PURPOSE_RJ_PICK = 21, 22, 23, 27, 28
RJ_MODE_BD = 2
MAX_TRY = 64


def branch_spec(b):
    """The branch's leaf prior as a term specification (a box: uniform terms with the oracle's own constants)."""
    if hasattr(b, "spec"):
        return b.spec
    spec = pt.make_spec([("uniform", lo, hi) for lo, hi in zip(b.lo, b.hi)])
    spec["c0"] = np.array(b.logpdf_vals, dtype=np.float64)
    return spec


def leaf_logq(b, gen, rows):
    """logq[N] of rows[N, ndim]: the generator's log-density of one leaf (``gen`` None: the branch's prior)."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, b.ndim)
    return b.leaf_logpdf(rows) if gen is None else pt.log_prior(gen, rows)


def _with_try(st, b, leaf, y=None):
    """(x, inds) of every walker with slot ``leaf`` of branch b active and holding y[T, W, ndim] (None: the slot cleared)."""
    T, W = leaf.shape
    tt, ww = np.indices((T, W))
    x = {k: v.copy() for k, v in st.x.items()}
    inds = {k: v.copy() for k, v in st.inds.items()}
    inds[b.name][tt, ww, leaf] = y is not None
    if y is not None:
        x[b.name][tt, ww, leaf] = y
    return x, inds


def mt_bd_step(o, bi, change, leaf, tries, u_pick, u_acc, gen=None, info=None):
    """One proposal of the move on branch ``bi`` of the oracle sampler ``o`` (its state, branches, data, ladder, likelihood): change /
    leaf [T, W], tries [T, W, K, ndim] (a death walker's try 0 is replaced by its dying leaf), u_pick / u_acc [T, W].  Mutates o.st;
    returns (keep, out) with out = dict(pick, lsw, aux_lsw, factors, mt_ll, mt_lp), each [T, W] - factors before the edge factors."""
    st, b, T, W = o.st, o.branches[bi], o.T, o.W
    N = T * W
    change, leaf = np.asarray(change, dtype=np.int64), np.asarray(leaf, dtype=np.int64)
    assert set(np.unique(change)) <= {-1, 1}, "MT RJ is only implemented for +1/-1 moves."
    death = change == -1
    y = np.array(tries, dtype=np.float64).reshape(T, W, -1, b.ndim)
    K = y.shape[2]
    tt, ww = np.indices((T, W))
    y[death, 0] = st.x[b.name][tt, ww, leaf][death]                                   # multipletry.py:315-317
    like = dict(branches=o.branches, t=o.t, y=o.y, sigma=o.sigma, fill=o.fill, like_fn=o.like_fn)
    beta = np.repeat(np.asarray(st.betas, dtype=np.float64), W)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        xb, ib = _with_try(st, b, leaf)                                               # multipletry.py:704-748: the model without the leaf
        lp_base = orj.compute_log_prior(xb, ib, o.branches)
        ll_base = orj.compute_log_like(xb, ib, st.P, **like)                          # (logp = the stored priors: finite, nobody is skipped)
        lp_in = np.where(death, lp_base, st.P).reshape(N)
        ll_in = np.where(death, ll_base, st.L).reshape(N)
        lp, ll, states = np.zeros((N, K)), np.zeros((N, K)), []
        for k in range(K):
            xk, ik = _with_try(st, b, leaf, y[:, :, k])
            pk = orj.compute_log_prior(xk, ik, o.branches)                            # multipletry.py:344 (no fix_logp_gibbs)
            lp[:, k] = pk.reshape(N)
            ll[:, k] = orj.compute_log_like(xk, ik, pk, **like).reshape(N)            # multipletry.py:334 (skipped and filled at a -inf prior)
            states.append((xk, ik))
        lq_leaf = leaf_logq(b, gen, y.reshape(-1, b.ndim)).reshape(N, K)
        lq = lq_leaf + lp_in[:, None]                                                 # multipletry.py:350-351
        logP = beta[:, None] * ll + lp                                                # multipletry.py:221-223
        w = logP - lq                                                                 # multipletry.py:45
        lsw = mm.logsumexp(w)
        c = np.exp(w - lsw[:, None]).cumsum(1)                                        # multipletry.py:51-57
        pick = (c > np.asarray(u_pick, dtype=np.float64).reshape(N)[:, None]).argmax(1)
        pick[death.reshape(N)] = 0                                                    # multipletry.py:365
        at = (np.arange(N), pick)
        aux_logP = beta * ll_in + lp_in                                               # multipletry.py:419-428
        aux_w = np.repeat((aux_logP - lp_in)[:, None], K, axis=1)                     # :431
        aux_lsw = mm.logsumexp(aux_w)                                                 # :463
        factors = ((aux_logP - aux_lsw) - lp_in + lp_in) - ((logP[at] - lsw) - lq[at] + lq[at])      # multipletry.py:472-476
        factors[death.reshape(N)] *= -1                                               # :480
        mt_ll = np.where(death, ll_in.reshape(T, W), ll[at].reshape(T, W))            # :373-374, 481-482
        mt_lp = np.where(death, lp_in.reshape(T, W), lp[at].reshape(T, W))
        factors = factors.reshape(T, W)
        # ReversibleJumpMove.propose (rj.py:205-352)
        q, new_inds = _with_try(st, b, leaf)
        new_inds[b.name][tt, ww, leaf] = ~death
        q[b.name][~death, leaf[~death]] = y.reshape(N, K, b.ndim)[at].reshape(T, W, b.ndim)[~death]
        edge = np.zeros((T, W))
        if not (b.nleaves_min == b.nleaves_max or b.nleaves_min + 1 == b.nleaves_max):       # rj.py:236-270
            nold, nnew = st.inds[b.name].sum(axis=-1), new_inds[b.name].sum(axis=-1)
            edge[nold == b.nleaves_min] += np.log(1 / 2.0)
            edge[nold == b.nleaves_max] += np.log(1 / 2.0)
            edge[nnew == b.nleaves_min] -= np.log(1 / 2.0)
            edge[nnew == b.nleaves_max] -= np.log(1 / 2.0)
        total = factors + edge                                                        # rj.py:271
        logp = mt_lp.copy()
        orj.fix_logp_gibbs(logp, new_inds, [b.name])                                  # rj.py:303
        logl = mt_ll.copy()
        u_acc = np.asarray(u_acc, dtype=np.float64).reshape(T, W)
        keep, lnpdiff = o._accept(total, logl, logp, u_acc)                           # rj.py:320-332
    out = dict(pick=pick.reshape(T, W), lsw=lsw.reshape(T, W), aux_lsw=aux_lsw.reshape(T, W), factors=factors, mt_ll=mt_ll, mt_lp=mt_lp)
    if info is not None:
        info.update(out, bi=bi, K=K, y=y, change=change, leaf=leaf, ll=ll, lp=lp, lq_leaf=lq_leaf, lq=lq, logP=logP, w=w, c=c, ll_in=ll_in,
                    lp_in=lp_in, beta=beta, base=(xb, ib), states=states, L_old=st.L.copy(), P_old=st.P.copy(), gen=gen, edge=edge,
                    lnpdiff=lnpdiff, keep=keep, u_acc=u_acc, u_pick=np.asarray(u_pick, dtype=np.float64).reshape(T, W), logp=logp, logl=logl)
    orj.update(st, q, new_inds, logl, logp, keep)
    return keep, out


# ---- exact arithmetic and the bounds ------------------------------------------------------------------------------------------------------
class _Spec:
    def __init__(self, b):
        self.name, self.ndim, self.spec = b.name, b.ndim, branch_spec(b)


def exact_rj_mt(o, info, rtol_l=tol.RTOL_L):
    """Exact lsw, aux_lsw, factors (long double [T, W]) of the proposal ``info`` describes and the bounds B_lsw, B_aux, B_F [T, W], the
    running sums c and their bound B_c [T, W, K] of the module's docstring."""
    assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here"
    T, W, K, bi = o.T, o.W, info["K"], info["bi"]
    N = T * W
    b = o.branches[bi]
    sb = [_Spec(x) for x in o.branches]
    death = (info["change"] == -1).reshape(N)
    beta = info["beta"].astype(LD)
    gen = info["gen"] if info["gen"] is not None else branch_spec(b)
    rows = info["y"].reshape(-1, b.ndim)
    z = lambda a, ok: np.where(ok, np.abs(a), 0).astype(np.float64)        # noqa: E731  (magnitudes, 0 where the value is not finite)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        lqs, bq = pt.exact_log_prior(gen, rows).reshape(N, K), pt.float64_bound(gen, rows).reshape(N, K)
        xb, ib = info["base"]
        lpb = rpt.exact_state_log_prior(sb, xb, ib).reshape(N)
        bpb = rpt.state_bound(sb, xb, ib).reshape(N)
        lp_in = np.where(death, lpb, info["P_old"].reshape(N).astype(LD))
        b_in = np.where(death, bpb, 0.0)
        ll_in = info["ll_in"].astype(LD)
        r_in = np.where(death, rtol_l, 0.0)                                # (a birth's ll_in = L is data)
        lp, bp = np.zeros((N, K), dtype=LD), np.zeros((N, K))
        for k, (xk, ik) in enumerate(info["states"]):
            lp[:, k] = rpt.exact_state_log_prior(sb, xk, ik).reshape(N)
            bp[:, k] = rpt.state_bound(sb, xk, ik).reshape(N)
        ll = info["ll"].astype(LD)
        bll = beta[:, None] * ll
        logP = bll + lp
        lq = lqs + lp_in[:, None]
        w = logP - lq
        finw = np.isfinite(w)
        e = np.where(finw, z(bll, finw) * rtol_l + bp + bq + b_in[:, None] + U * (z(lq, finw) + z(bll, finw) + z(logP, finw) + z(w, finw)), 0.0)
        lsw, B_lsw = mm._lse_exact(w, e)
        pick = info["pick"].reshape(N)
        at = (np.arange(N), pick)
        bL = beta * ll_in
        aP = bL + lp_in
        aw = bL                                                            # (lp_in cancels exactly)
        fa = np.isfinite(aP - lp_in)
        aw = np.where(fa, aw, aP - lp_in)                                  # (a non-finite aux_w stays what the formula gives)
        e_aux = np.where(fa, z(bL, fa) * r_in + U * (z(bL, fa) + z(aP, fa) + z(aw, fa)), 0.0)
        aux, B_aux = mm._lse_exact(np.repeat(aw[:, None], K, axis=1), np.repeat(e_aux[:, None], K, axis=1))
        t1, t2 = aP - aux, logP[at] - lsw
        F = t1 - t2
        fin = np.isfinite(F) & np.isfinite(lq[at]) & np.isfinite(lp_in)
        a = lambda v: np.where(fin, np.abs(v), 0).astype(np.float64)       # noqa: E731
        B_F = (a(bL) * r_in + b_in + U * (a(bL) + a(aP)) + B_aux + U * (2 * a(t1) + a(t1 - lp_in))
               + a(bll[at]) * rtol_l + bp[at] + U * (a(bll[at]) + a(logP[at])) + B_lsw + U * (2 * a(t2) + a(t2 - lq[at])) + U * a(F))
        F = np.where(death, -F, F)
        p = np.exp(w - lsw[:, None])
        rel = e + B_lsw[:, None] + U * np.where(finw, np.abs(w - lsw[:, None]), 0).astype(np.float64) + 2 * U
        c = p.cumsum(axis=1)
        B_c = (np.where(p > 0, p * rel, 0).cumsum(axis=1) + (np.arange(K) + 1) * U * c).astype(np.float64)
    return dict(lsw=lsw.reshape(T, W), aux_lsw=aux.reshape(T, W), factors=F.reshape(T, W), B_lsw=B_lsw.reshape(T, W),
                B_aux=B_aux.reshape(T, W), B_F=np.where(fin, B_F, 0.0).reshape(T, W), B_c=np.nan_to_num(B_c, nan=0.0).reshape(T, W, K),
                c=c.reshape(T, W, K))


def knives(info, ex):
    """(pick knife edges among the BIRTH walkers - a death walker's pick is forced -, accept knife edges) of one proposal."""
    from tests.parity_utils import knife_edge
    pk = mm.pick_knife(ex["c"], info["u_pick"], ex["B_c"]) & (info["change"] == +1)
    with np.errstate(divide="ignore"):
        ak = knife_edge(info["lnpdiff"], np.log(info["u_acc"]))
    return int(pk.sum()), int(ak.sum())


# ---- the oracle sampler with this move in the reversible-jump slot --------------------------------------------------------------------
class MTOracleRJSampler(orj.OracleRJSampler):
    """``OracleRJSampler`` whose between-model move is MTDistGenMoveRJ(num_try=K): ``gens`` per branch a term specification or None
    (the prior).  Draw sources beside the oracle's own: ``_draw_tries`` (the global stream: ``generate_dist.rvs(size=(N, K))``, one
    ``rand`` / ``randn`` of N K values per parameter) and ``_draw_pick`` (``np.random.rand(N)``)."""

    def __init__(self, *a, num_try=1, gens=None, **kw):
        super().__init__(*a, **kw)
        if self.schedule == "together":
            raise ValueError("Can only propose change to one model at a time with MT.")       # multipletry.py:635-636
        self.K = int(num_try)
        self.gens = list(gens) if gens is not None else [None] * len(self.branches)
        self.mt_infos = []

    def _draw_tries(self, b, gen):
        N, K = self.T * self.W, self.K
        spec = gen if gen is not None else branch_spec(b)
        out = np.zeros((N, K, b.ndim))
        for d in range(b.ndim):                                                    # prior.py:432-497: per parameter, in order
            k = spec["kind"][d]
            if k == pt.NORMAL:
                out[..., d] = self.G.randn(N, K) * spec["c1"][d] + spec["c0"][d]
            elif k == pt.LOG_UNIFORM:
                out[..., d] = np.exp(self.G.rand(N, K) * (np.log(spec["hi"][d]) - np.log(spec["lo"][d])) + np.log(spec["lo"][d]))
            else:
                out[..., d] = self.G.rand(N, K) * (spec["hi"][d] - spec["lo"][d]) + spec["lo"][d]
        return out.reshape(self.T, self.W, K, b.ndim)

    def _draw_pick(self):
        return self.G.rand(self.T * self.W).reshape(self.T, self.W)                # multipletry.py:57

    def draw_inputs(self, bi):
        """(change, leaf, tries, u_pick, u_acc) of one proposal on branch ``bi``, every draw in the reference's order."""
        b, st, T, W = self.branches[bi], self.st, self.T, self.W
        if b.nleaves_min == b.nleaves_max:
            raise ValueError("MT RJ proposal requires that nleaves_min != nleaves_max.")   # multipletry.py:661-664
        self._bi = bi
        inds = st.inds[b.name]
        nleaves = inds.sum(axis=-1)
        change = self._draw_coin(nleaves.shape)                                    # distgenrj.py:63-73
        change = (change * ((nleaves != b.nleaves_min) & (nleaves != b.nleaves_max))
                  + (+1) * (nleaves == b.nleaves_min) + (-1) * (nleaves == b.nleaves_max))
        leaf = np.zeros((T, W), dtype=np.int64)
        for tt in range(T):                                                        # :85-121
            for w in range(W):
                leaf[tt, w] = self._draw_leaf(tt, w, np.where(~inds[tt, w] if change[tt, w] == +1 else inds[tt, w])[0])
        tries = self._draw_tries(b, self.gens[bi])
        u_pick = self._draw_pick()
        u_acc = self._draw_accept("rj")
        return change, leaf, tries, u_pick, u_acc

    def _rj_propose(self, bis, rec=None):
        assert len(bis) == 1, "Can only propose change to one model at a time with MT."
        bi = bis[0]
        change, leaf, tries, u_pick, u_acc = self.draw_inputs(bi)
        info = {}
        if rec is not None:
            self._snapshot(rec, "rjpre_")
        keep, out = mt_bd_step(self, bi, change, leaf, tries, u_pick, u_acc, gen=self.gens[bi], info=info)
        self.mt_infos.append(info)
        if rec is not None:
            rec.update(rj_branch=bi, rj_change=change.copy(), rj_leaf=leaf.copy(), rj_tries=info["y"].copy(), rj_u_pick=u_pick, rj_u_acc=u_acc,
                       rj_accepted=keep, rj_lnpdiff=info["lnpdiff"], rj_logp=info["logp"], rj_logl=info["logl"],
                       **{"rj_" + k: v for k, v in out.items()})
            self._snapshot(rec, "rjupd_")
        return keep


# ---- the draws of the production path ---------------------------------------------------------------------------------------------------
def _wid(T, W, rung_begin=0):
    return (rung_begin + np.arange(T))[:, None] * W + np.arange(W)[None, :]


def try_key(branch, d, k):
    """Counter word 3 of the call that draws parameter d of try k in ``branch`` (hens_rj_mt.h: rj_try_key; k = 0: hens_rj.h rj_birth_key)."""
    if k == 0:
        return PURPOSE_RJ_BIRTH | (d << 8) | (branch << 16)
    return PURPOSE_RJ_TRY | (d << 8) | (k << 10) | (branch << 16)


def pick_key(branch):
    return PURPOSE_RJ_PICK | (branch << 16)


def mt_draws(seed, it, T, W, K, branch, gen, rung_begin=0):
    """(X float64, X* long double, E float64), each [T, W, K, ndim]: the tries iteration ``it`` draws for ``branch`` under the generator
    ``gen`` (a term specification): tests/rj_prior_terms.birth_spec on every call's words."""
    nd = len(gen["kind"])
    X, Xs, E = np.zeros((T, W, K, nd)), np.zeros((T, W, K, nd), dtype=LD), np.zeros((T, W, K, nd))
    for k in range(K):
        for d in range(nd):
            words = philox4x32_10(it & 0xFFFFFFFF, it >> 32, _wid(T, W, rung_begin), try_key(branch, d, k), seed & 0xFFFFFFFF, seed >> 32)
            X[:, :, k, d], Xs[:, :, k, d], E[:, :, k, d] = rpt.birth_spec(gen, d, words)
    return X, Xs, E


def pick_uniforms(seed, it, T, W, branch, rung_begin=0):
    d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, _wid(T, W, rung_begin), pick_key(branch), seed & 0xFFFFFFFF, seed >> 32)
    return u01(d[0], d[1])


def accept_uniforms(seed, it, T, W, branch, rung_begin=0):
    """The move's accept uniform: the plain birth / death move's call (hens_rj.h: rj_acc_key(RJ_MODE_BD, branch))."""
    d = philox4x32_10(it & 0xFFFFFFFF, it >> 32, _wid(T, W, rung_begin), PURPOSE_RJ_ACC | (RJ_MODE_BD << 8) | (branch << 16), seed & 0xFFFFFFFF, seed >> 32)
    return u01(d[0], d[1])


def iteration_keys(nbranches, ncoord, ndims, K):
    """Counter word 3 of every call a walker makes in one iteration of hens_rj_step (Gaussian in-model move, every branch's multiple-try
    birth / death): the in-model normals and accept uniform, per branch coin / selector, accept, pick, tries."""
    keys = [12 | ((i | 0x10000) << 8) for i in range(ncoord)] + [PURPOSE_RJ_ACC | (1 << 8)]
    for b in range(nbranches):
        keys += [PURPOSE_RJ_BD | (b << 16), PURPOSE_RJ_ACC | (RJ_MODE_BD << 8) | (b << 16), pick_key(b)]
        keys += [try_key(b, d, k) for k in range(K) for d in range(ndims[b])]
    return keys


# ---- the cases of the GPU tests -----------------------------------------------------------------------------------------------------------
def case(kinds, T, W, K, ndata, nl_max, nl_min, prior="box", gen=None, sigma=3.0, seed=1, betas=None, nprop=4, p_active=0.5,
         inf_prior=False, nan_factor=False, edges=True):
    """gen: {branch index: entries as tests/prior_terms.make_spec takes them} (branches left out, or None: the prior).  inf_prior /
    nan_factor / edges: what the case must show beside the conditions every case has (``assert_sized``)."""
    return dict(kinds=tuple(kinds), T=T, W=W, K=K, ndata=ndata, nl_max=tuple(nl_max), nl_min=tuple(nl_min), prior=prior, gen=gen, sigma=sigma,
                seed=seed, betas=betas, nprop=nprop, p_active=p_active, inf_prior=inf_prior, nan_factor=nan_factor, edges=edges)


TWO_PI = 2 * np.pi
# a generator WIDER than the pulse box of tests/leaf_kind_cases.py in the amplitude (tries with a -inf prior) and NARROWER in the width
# (dying leaves outside the generator: NaN factors); the same idea on the prior terms of tests/rj_prior_terms.ENTRIES
GEN_PULSE_BOX = [("uniform", 2.0, 4.0), ("uniform", -1.0, 1.0), ("uniform", 0.06, 0.21)]
GEN_PULSE_TERMS = [("uniform", 0.5, 7.0), ("normal", 0.0, 0.5), ("uniform", 0.05, 0.21)]
GEN_SINE_TERMS = [("normal", 1.0, 0.3), ("log_uniform", 1.0, 20.0), ("uniform", 0.0, TWO_PI)]
# the smallest shapes at which each mechanism can go wrong (W against the waves per workgroup, K = 1 / 2 / 7 / 64, data points short of,
# at and past a wave's 64 and two chunks' worth, a branch without edge factors, four branches of widths 1 - 4, prior terms with a
# generator of its own, one rung, a beta = 0 rung); the seeds are those at which ``assert_sized`` holds on the specification alone
CASES = {
    "w5_k1_nd50_pulse": case(("pulse",), 3, 5, 1, 50, (3,), (0,), seed=3, nprop=6, p_active=0.3),
    "w9_k2_nd64_two_gen": case(("pulse", "sine"), 2, 9, 2, 64, (3, 2), (0, 0), gen={0: GEN_PULSE_BOX}, seed=2, nprop=6, inf_prior=True, nan_factor=True),
    "w9_k7_nd65_no_edge_factors": case(("pulse",), 2, 9, 7, 65, (2,), (1,), seed=1, nprop=4),
    "w5_k64_nd130_four_branches": case(("offset", "pulse", "sine", "burst"), 2, 5, 64, 130, (2, 2, 2, 2), (0, 0, 0, 0), seed=1, nprop=8),
    "w9_k7_nd50_terms_gen": case(("pulse", "sine"), 2, 9, 7, 50, (3, 2), (0, 0), prior="terms", gen={0: GEN_PULSE_TERMS, 1: GEN_SINE_TERMS},
                                 seed=1, nprop=6, inf_prior=True, nan_factor=True),
    "t3_w9_k5_nd64_two_gen": case(("pulse", "sine"), 3, 9, 5, 64, (3, 2), (0, 0), gen={0: GEN_PULSE_BOX}, seed=4, nprop=4, inf_prior=True, nan_factor=True),
    "t1_w9_k2": case(("pulse",), 1, 9, 2, 50, (3,), (0,), seed=1, nprop=4),
    "beta0_w5_k7": case(("pulse", "sine"), 2, 5, 7, 64, (2, 2), (0, 0), betas=(1.0, 0.0), seed=1, nprop=6),
}
# hens_rj_step replayed: (case, schedule, in-model move, iterations, first iteration, a ladder adaptation pending into the launch)
REPLAYS = {
    "separate_gaussian_across_64": ("t3_w9_k5_nd64_two_gen", "separate_branches", "gaussian", 6, 61, True),      # (three rungs: the middle one adapts)
    "iterate_stretch_terms": ("w9_k7_nd50_terms_gen", "iterate_branches", "stretch", 5, 0, False),
    "iterate_gaussian_four_branches": ("w5_k64_nd130_four_branches", "iterate_branches", "gaussian", 4, 0, False),
}


def case_problem(c):
    """-> dict(obr, dbr, t, y, sigma, x, inds, betas, gens, dev_gens, like_fn, scale): the oracle's and the device's branches, data, a
    start state, the ladder, per branch the generator's term specification (None: the prior) - and as the device takes it -, the
    oracle's likelihood function (None: its own template model), in-model step scales."""
    from tests import leaf_kind_cases as cases
    from tests import leaf_kinds as lk
    kinds, T, W = c["kinds"], c["T"], c["W"]
    rs = np.random.RandomState(c["seed"])
    t = np.linspace(-1, 1, c["ndata"])
    if c["prior"] == "terms":
        obr = rpt.branches_of(kinds, c["nl_max"], c["nl_min"])
        dbr = rpt.device_branches(obr)
        y = c["sigma"] * rs.randn(c["ndata"])
        for b in obr:
            y = y + lk.leaf_value(b.kind_name, b.rvs(1, rs)[0], t)
        x, inds = rpt.start_state(obr, T, W, rs, c["p_active"])
        scale = rpt.scales(obr)
    else:
        lbr = cases.branches_of(kinds, c["nl_max"], c["nl_min"])
        scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in lbr]
        obr, dbr = [b.to_oracle(cov=np.diag(s ** 2)) for b, s in zip(lbr, scale)], [b.to_device() for b in lbr]
        y = cases.make_data(lbr, t, c["sigma"], rs)
        x, inds = cases.random_state(lbr, T, W, rs, c["p_active"])
    gens = [None if not c["gen"] or c["gen"].get(i) is None else pt.make_spec(c["gen"][i]) for i in range(len(kinds))]
    dev_gens = None if not c["gen"] else {b.name: (gens[i] if gens[i] is not None else branch_spec(b)) for i, b in enumerate(obr)}
    betas = np.array(c["betas"], dtype=np.float64) if c["betas"] is not None else 0.35 ** np.arange(T)
    plain = c["prior"] == "box" and set(kinds) <= {"pulse", "sine"}
    return dict(obr=obr, dbr=dbr, t=t, y=y, sigma=c["sigma"], x=x, inds=inds, betas=betas, gens=gens, dev_gens=dev_gens,
                like_fn=None if plain else lk.like_fn(kinds), scale=scale)


def case_oracle(c, p, cls=None, **kw):
    """The specification's sampler on a case's start, fed from NumPy streams of the case's seed."""
    R, G = np.random.RandomState(c["seed"] + 101), np.random.RandomState(c["seed"] + 202)
    return (cls or MTOracleRJSampler)(p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], R, G, p["betas"], num_try=c["K"], gens=p["gens"],
                                      like_fn=p["like_fn"], **kw)


class Counts:
    """Coverage of a case, from the SPECIFICATION's side."""

    def __init__(self):
        self.births = self.deaths = self.rejections = self.picks_beyond_0 = self.inf_prior = self.nan_factors = 0
        self.at_min = self.at_max = self.knife_picks = self.knife_accepts = self.proposals = 0

    def add(self, o, info, ex):
        b = o.branches[info["bi"]]
        keep, ch = info["keep"], info["change"]
        self.proposals += 1
        self.births += int((keep & (ch == +1)).sum())
        self.deaths += int((keep & (ch == -1)).sum())
        self.rejections += int((~keep).sum())
        self.picks_beyond_0 += int((info["pick"] != 0).sum())
        self.inf_prior += int(np.isneginf(info["lp"]).sum())
        self.nan_factors += int(np.isnan(info["factors"]).sum())
        nold = o_nleaves_before(info, b)
        self.at_min += int((nold == b.nleaves_min).sum())
        self.at_max += int((nold == b.nleaves_max).sum())
        kp, ka = knives(info, ex)
        self.knife_picks += kp
        self.knife_accepts += ka


def o_nleaves_before(info, b):
    """Leaves of the branch in front of the proposal: the base's count + 1 on a death walker."""
    return info["base"][1][b.name].sum(axis=-1) + (info["change"] == -1)


def assert_sized(cnt, c, what=""):
    """The conditions on a case's inputs: no pick or accept knife edge; an accepted birth, an accepted death and a rejection; a pick other
    than try 0 (K > 1); where the case says so a -inf-prior try, a NaN factor, a walker at each edge of the leaf budget."""
    print(f"{what}: {cnt.proposals} proposals, accepted births {cnt.births} / deaths {cnt.deaths}, rejections {cnt.rejections}, picks other than "
          f"try 0 {cnt.picks_beyond_0}, -inf-prior tries {cnt.inf_prior}, NaN factors {cnt.nan_factors}, walkers at the floor {cnt.at_min} / the "
          f"ceiling {cnt.at_max}, knife-edge picks {cnt.knife_picks} / accepts {cnt.knife_accepts}")
    assert cnt.knife_picks == 0 and cnt.knife_accepts == 0, f"{what}: a decision on the knife edge"
    assert cnt.births >= 1 and cnt.deaths >= 1 and cnt.rejections >= 1, f"{what}: an accepted birth, an accepted death and a rejection"
    assert c["K"] == 1 or cnt.picks_beyond_0 >= 1, f"{what}: no pick other than try 0"
    assert not c["inf_prior"] or cnt.inf_prior >= 1, f"{what}: no try with a -inf prior"
    assert not c["nan_factor"] or cnt.nan_factors >= 1, f"{what}: no NaN factor"
    assert not c["edges"] or (cnt.at_min >= 1 and cnt.at_max >= 1), f"{what}: no walker at an edge of the leaf budget"


def forced_run(c, on_proposal=None):
    """A case's teacher-forced proposals on the specification alone (branches in turn, a sweep without adaptation behind each, rj.py:
    381-382) -> Counts.  on_proposal(o, bi, inputs, info, ex, sweep): the GPU test's hook, called after the specification's move and
    sweep with the sweep's draws."""
    p = case_problem(c)
    o = case_oracle(c, p)
    cnt = Counts()
    for n in range(c["nprop"]):
        bi = n % len(o.branches)
        inputs = o.draw_inputs(bi)
        info, pre, mid, sweep = {}, {}, {}, {}
        o._snapshot(pre, "")
        mt_bd_step(o, bi, *inputs, gen=o.gens[bi], info=info)
        ex = exact_rj_mt(o, info)
        cnt.add(o, info, ex)
        o._snapshot(mid, "")
        o._pt(False, sweep)
        if on_proposal is not None:
            on_proposal(o, bi, inputs, info, ex, sweep, pre, mid)
    return cnt


# ---- fixtures from the real reference (tests/golden/make_golden_rj_mt.py -> tests/golden/rj_mt/) -------------------------------------------
FIXTURES = ["rjmt1", "rjmt2"]
FIXTURE_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "rj_mt")


def load_fixture(name):
    with np.load(os.path.join(FIXTURE_DIR, name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def fixture_names(fx):
    return [str(k) for k in fx["branch_names"]]


def fixture_gens(fx):
    """Per branch the generator's term specification (None where it is the prior's box)."""
    return [None if np.array_equal(fx[f"{k}_gen_box"], fx[f"{k}_box"]) else pt.make_spec([("uniform", lo, hi) for lo, hi in fx[f"{k}_gen_box"]])
            for k in fixture_names(fx)]


def fixture_oracle(fx, cls=None, **kw):
    """The specification's sampler on a fixture's start, fed from the fixture's two seeds."""
    kind = {"gauss": orj.KIND_PULSE, "sine": orj.KIND_SINE}
    cov = np.diag(np.ones(3)) * float(fx["cov_factor"])
    brs = [orj.Branch(k, kind[k], fx[f"{k}_box"], int(fx["nl_max"][i]), int(fx["nl_min"][i]), cov) for i, k in enumerate(fixture_names(fx))]
    R, G = np.random.RandomState(int(fx["seed_construct"])), np.random.RandomState(int(fx["seed_run"]))
    x0 = {b.name: fx[f"x0_{b.name}"] for b in brs}
    inds0 = {b.name: fx[f"inds0_{b.name}"] for b in brs}
    return (cls or MTOracleRJSampler)(brs, x0, inds0, fx["t"], fx["y"], float(fx["sigma"]), R, G, fx["betas0"], num_try=int(fx["K"]),
                                      gens=fixture_gens(fx), **kw)
