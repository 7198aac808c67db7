"""Specification of periodic leaf parameters on leaf-packing records: what ``EnsembleSampler(periodic={"sine": {2: 2 pi}})`` makes of
every in-model move (utils/periodic.py:49-151 under gaussian.py:102-127, stretch.py:136-154, groupstretch.py:107-109 and mh.py:79-136 +
move.py:297-336), stated in NumPy on the existing specifications - oracle/eryn_oracle_rj.py, tests/rj_group_move.py and
tests/rj_gibbs_move.py are imported and composed with, not edited.  csrc/hens_rj.h (RjArgs::per_on) carries the same rules.

``periods``: {branch name: [ndim] periods, 0 = not periodic}.

  distance(s, c)   ``c - s``; where ``|c - s| > period / 2`` the moving point is shifted by one period toward c - ``new_s = -(period
                   - s)`` for a negative difference, ``period + s`` otherwise, as the masked sum of periodic.py:101-107 - and the
                   difference taken again (a difference of exactly half a period keeps the long way)
  wrap(q)          NumPy's float remainder ``q % period`` on the periodic parameters
  Gaussian move    q = x + step on the active leaves, then wrap over the WHOLE array of every branch: the periodic coordinates of
                   dead slots are wrapped too, so an accepted walker's record carries ``x % period`` there
  ... in blocks    get_proposal wraps the whole arrays of the block's branches, cleanup_proposals_gibbs puts back every coordinate
                   whose mask entry is false: a TRUE coordinate is wrapped, moved or not, active or not; the others (and the branches
                   outside the block) keep their bits
  stretch move     q = wrap(c - distance(s, c) zz) on every slot of every branch, active or not
  group stretch    the same with the friend as c; a dead slot and a leaf of a branch with an empty table are their own friend:
                   distance 0, q = wrap(x - 0 zz) = x % period.  The friend rule (tests/rj_group_move.py rule 2) stays linear in the key.
Birth / death draws from the prior and knows no periods.

``SeamFacts`` counts, from a specification's (or the reference's) own intermediates, what a chain did at the seam."""
import os

import numpy as np

from oracle import eryn_oracle as base
from oracle import eryn_oracle_rj as orj
from tests import rj_gibbs_move as rgm
from tests import rj_group_move as rgr

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["rjp_gauss", "rjp_stretch", "rjp_group", "rjp_gibbs"]
TWO_PI = 2 * np.pi
PERIODIC = {"gauss": {}, "sine": {2: TWO_PI}}           # the fixtures' constructor argument
GIBBS_SETUP = ["gauss", "sine"]                           # rjp_gibbs: one block per branch


def load_fixture(name):
    with np.load(os.path.join(HERE, "golden", "rj_periodic", name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


# ---- periodic.py in NumPy -------------------------------------------------------------------------------------------------------------
def distance(s, c, period):
    """periodic.py:80-113 for one branch: parameters along the last axis, ``period`` [ndim]."""
    s, c, period = np.asarray(s, dtype=np.float64), np.asarray(c, dtype=np.float64), np.asarray(period, dtype=np.float64)
    diff = c - s
    idx = np.flatnonzero(period > 0)
    if idx.size:
        per = period[idx]
        dp = diff[..., idx]
        fix = np.abs(dp) > per / 2.0
        new_s = -(per - s[..., idx]) * (dp < 0.0) + (per + s[..., idx]) * (dp >= 0.0)
        dp[fix] = c[..., idx][fix] - new_s[fix]
        diff[..., idx] = dp
    return diff


def wrap(q, period):
    """periodic.py:136-149 for one branch, on a copy."""
    q, period = np.array(q, dtype=np.float64, copy=True), np.asarray(period, dtype=np.float64)
    idx = np.flatnonzero(period > 0)
    if idx.size:
        q[..., idx] = q[..., idx] % period[idx]
    return q


def period_rows(periodic, branches):
    """{branch: {index: period}} -> {name: [ndim]} (a branch that is absent, None or {}: all zeros)."""
    out = {}
    for b in branches:
        row = np.zeros(b.ndim)
        for i, p in ((periodic or {}).get(b.name) or {}).items():
            row[int(i)] = float(p)
        out[b.name] = row
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


# ---- what a chain did at the seam ---------------------------------------------------------------------------------------------------------
class SeamFacts:
    """wrapped_accepts: accepted proposals with an ACTIVE periodic coordinate that left [0, period) and was wrapped back in;
    short_way: active periodic coordinates with |c - s| > period / 2; dead_changed: accepted walkers with a dead slot's periodic
    coordinate whose bits the proposal changed; accepted / rejected: proposals."""

    def __init__(self):
        self.wrapped_accepts = self.short_way = self.dead_changed = self.accepted = self.rejected = self.crossed = self.proposals = 0

    def proposal(self, periods, x_old, raw, q, inds, keep):
        """One proposal of N walkers per rung: x_old / raw (in front of the wrap) / q {name: [T, N, nl, nd]}, inds {name: [T, N, nl]},
        keep [T, N]."""
        keep = np.asarray(keep, dtype=bool)
        crossed = np.zeros(keep.shape, dtype=bool)
        dead = np.zeros(keep.shape, dtype=bool)
        for name, per in periods.items():
            idx = np.flatnonzero(per > 0)
            if not idx.size:
                continue
            act = np.asarray(inds[name], dtype=bool)[..., None]
            r = raw[name][..., idx]
            crossed |= (act & ((r < 0.0) | (r >= per[idx]))).any(axis=(-1, -2))
            dead |= (~act & (bits(q[name][..., idx]) != bits(x_old[name][..., idx]))).any(axis=(-1, -2))
        self.crossed += int(crossed.sum())
        self.wrapped_accepts += int((crossed & keep).sum())
        self.dead_changed += int((dead & keep).sum())
        self.accepted += int(keep.sum())
        self.rejected += int((~keep).sum())
        self.proposals += int(keep.size)

    def differences(self, periods, name, s, c, inds):
        per = periods[name]
        idx = np.flatnonzero(per > 0)
        if idx.size:
            act = np.asarray(inds, dtype=bool)[..., None]
            self.short_way += int((act & (np.abs((c - s)[..., idx]) > per[idx] / 2.0)).sum())

    def as_dict(self):
        return dict(wrapped_accepts=self.wrapped_accepts, short_way=self.short_way, dead_changed=self.dead_changed, accepted=self.accepted,
                    rejected=self.rejected, crossed=self.crossed, proposals=self.proposals)


# ---- the Gaussian and the red / blue stretch move ------------------------------------------------------------------------------------------
class PeriodicOracle(orj.OracleRJSampler):
    """The pinned oracle with periodic leaf parameters in its in-model moves; birth / death, the cascades and the draws' sources are
    the oracle's.  ``live_dangerously``: red_blue.py:108."""

    def __init__(self, periods, *a, live_dangerously=False, **kw):
        super().__init__(*a, **kw)
        self.periods = {k: np.asarray(v, dtype=np.float64) for k, v in periods.items()}
        self.live_dangerously, self.facts = live_dangerously, SeamFacts()

    def mh_move(self, rec=None):
        st = self.st
        self._draw_move_choice()
        q, raw, steps = {}, {}, {}
        for b in self.branches:
            inds_here = np.where(st.inds[b.name])
            x0 = st.x[b.name][inds_here]
            step = self._draw_steps(b, len(x0))
            raw[b.name] = st.x[b.name].copy()
            raw[b.name][inds_here] = x0 + 1.0 * step
            steps[b.name] = step
        for b in self.branches:                                                    # gaussian.py:110-127: every branch, every slot
            q[b.name] = wrap(raw[b.name], self.periods[b.name])
        logp = orj.compute_log_prior(q, st.inds, self.branches)
        orj.fix_logp_gibbs(logp, st.inds, [b.name for b in self.branches])
        logl = orj.compute_log_like(q, st.inds, logp, self.branches, self.t, self.y, self.sigma, self.fill, like_fn=self.like_fn)
        u_acc = self._draw_accept("mh")
        accepted, lnpdiff = self._accept(np.zeros((self.T, self.W)), logl, logp, u_acc)
        self.facts.proposal(self.periods, st.x, raw, q, st.inds, accepted)
        if rec is not None:
            self._snapshot(rec, "pre_")
            rec.update(mh_steps=steps, mh_q={k: v.copy() for k, v in q.items()}, mh_raw=raw, mh_logp=logp, mh_logl=logl, mh_u_acc=u_acc,
                       mh_lnpdiff=lnpdiff, mh_accepted=accepted, betas_before=st.betas.copy(), time_before=self.time)
        orj.update(st, q, st.inds, logl, logp, accepted)
        self.mh_accepted += accepted
        if rec is not None:
            self._snapshot(rec, "mhupd_")
        self._pt(True, rec)
        return accepted

    def stretch_move(self, rec=None):
        st, T, W = self.st, self.T, self.W
        self._draw_move_choice()
        ndim_total = sum(b.nleaves_max * b.ndim for b in self.branches)
        if W < 2 * ndim_total and not self.live_dangerously:                       # red_blue.py:103-114
            raise RuntimeError("It is unadvisable to use a red-blue move with fewer walkers than twice the number of dimensions.")
        labels = self._draw_split_labels()
        accepted = np.zeros((T, W), dtype=bool)
        tt = np.arange(T)[:, None]
        names = [b.name for b in self.branches]
        if rec is not None:
            self._snapshot(rec, "pre_")
            rec.update(st_labels=labels.copy(), betas_before=st.betas.copy(), time_before=self.time)
        for split in range(2):
            S, C = base.split_index_lists(labels, split, 2)
            Ns, Nc = S.shape[1], C.shape[1]
            q, raw, rints, zz, u_zz = {}, {}, [], None, None
            new_inds = {n: st.inds[n][tt, S] for n in names}
            for bi, b in enumerate(self.branches):
                rint = self._draw_rint(bi, split, Ns, Nc)
                if bi == 0:
                    u_zz = self._draw_zz(split, Ns)
                    zz = ((self.a - 1.0) * u_zz + 1) ** 2.0 / self.a
                s = st.x[b.name][tt, S]
                c = st.x[b.name][tt, C[tt, rint]]
                self.facts.differences(self.periods, b.name, s, c, new_inds[b.name])
                raw[b.name] = c - distance(s, c, self.periods[b.name]) * zz[:, :, None, None]      # stretch.py:136-145
                q[b.name] = wrap(raw[b.name], self.periods[b.name])                                # stretch.py:149-153
                rints.append(rint)
            factors = (ndim_total - 1.0) * np.log(zz)
            logp = orj.compute_log_prior(q, new_inds, self.branches)
            orj.fix_logp_gibbs(logp, new_inds, names)
            logl = orj.compute_log_like(q, new_inds, logp, self.branches, self.t, self.y, self.sigma, self.fill, like_fn=self.like_fn)
            u_acc = self._draw_accept_split(split, Ns)
            prevL, prevP = st.L[tt, S], st.P[tt, S]
            logP = base.tempered_log_posterior(logl, logp, st.betas)
            prev = base.tempered_log_posterior(prevL, prevP, st.betas)
            with np.errstate(invalid="ignore"):
                lnpdiff = factors + logP - prev
            with np.errstate(divide="ignore"):
                keep = lnpdiff > np.log(u_acc)
            self.facts.proposal(self.periods, {n: st.x[n][tt, S] for n in names}, raw, q, new_inds, keep)
            new_logp = logp.copy()
            new_logp[np.isinf(new_logp)] = 0.0
            st.L[tt, S] = logl * keep + prevL * (~keep)
            st.P[tt, S] = new_logp * keep + prevP * (~keep)
            for n in names:
                xs = st.x[n][tt, S].copy()
                xs[keep] = q[n][keep]
                st.x[n][tt, S] = xs
            accepted[tt, S] = keep
            if rec is not None:
                rec.update({f"st_rint{split}": np.stack(rints), f"st_u_zz{split}": u_zz, f"st_u_acc{split}": u_acc,
                            f"st_q{split}": {k: v.copy() for k, v in q.items()}, f"st_logp{split}": logp, f"st_logl{split}": logl,
                            f"st_factors{split}": factors, f"st_lnpdiff{split}": lnpdiff, f"st_keep{split}": keep,
                            f"st_S{split}": S, f"st_C{split}": C})
                self._snapshot(rec, f"stupd{split}_")
        self.mh_accepted += accepted
        if rec is not None:
            rec["mh_accepted"] = accepted
            self._snapshot(rec, "mhupd_")
        self._pt(True, rec)
        return accepted


# ---- the group stretch move ---------------------------------------------------------------------------------------------------------------
class PeriodicGroupOracle(rgr.GroupOracle):
    def __init__(self, periods, *a, **kw):
        super().__init__(*a, **kw)
        self.periods = {k: np.asarray(v, dtype=np.float64) for k, v in periods.items()}
        self.facts = SeamFacts()
        self.last_raw = None

    def propose(self, picks, u_zz):
        st = self.st
        zz = ((self.group_a - 1.0) * u_zz + 1) ** 2.0 / self.group_a
        q, raw = {}, {}
        for b in self.branches:
            s = st.x[b.name]
            c = s.copy()                                                          # a dead slot, a branch without a table: its own friend
            going = st.inds[b.name]
            if self.nf(b.name) > 0:
                assert np.all(self.start[b.name][going] >= 0), "an active leaf without a window"
                c[going] = self.tab[b.name][self.start[b.name][going] + picks[b.name][going]]
            self.facts.differences(self.periods, b.name, s, c, going)
            raw[b.name] = c - distance(s, c, self.periods[b.name]) * zz[:, :, None, None]
            q[b.name] = wrap(raw[b.name], self.periods[b.name])
        self.last_raw = raw
        ndim_total = sum(b.nleaves_max * b.ndim for b in self.branches)
        return q, (ndim_total - 1.0) * np.log(zz)

    def group_move(self, rec=None, forced=None):
        r = {} if rec is None else rec
        x_old = {k: v.copy() for k, v in self.st.x.items()}
        inds = {k: v.copy() for k, v in self.st.inds.items()}
        acc = super().group_move(r, forced)
        self.facts.proposal(self.periods, x_old, self.last_raw, r["q"], inds, acc)
        return acc


# ---- the Gaussian move in Gibbs blocks ------------------------------------------------------------------------------------------------------
def propose_block(blk, x, going, steps, periods):
    """tests/rj_gibbs_move.propose with the wrap between the step and the put-back -> (q, raw)."""
    q = {k: v.copy() for k, v in x.items()}
    raw = {k: v.copy() for k, v in x.items()}
    for name, m in blk:
        g = going[name]
        raw[name][g] = x[name][g] + 1.0 * steps[name][g]
        q[name] = wrap(raw[name], periods[name])                                  # gaussian.py:110-127: the block's branches, whole
        q[name][:, :, ~m] = x[name][:, :, ~m]                                     # move.py:322-324
    return q, raw


class PeriodicGibbsOracle(rgm.GibbsOracle):
    def __init__(self, periods, *a, **kw):
        super().__init__(*a, **kw)
        self.periods = {k: np.asarray(v, dtype=np.float64) for k, v in periods.items()}
        self.facts = SeamFacts()

    def block(self, k, rec=None):
        st, blk = self.st, self.blocks[k]
        by = {b.name: b for b in self.branches}
        going = rgm.moved_leaves(blk, st.inds)
        if self.skip_empty and not any(g.any() for g in going.values()):
            return None
        steps = {b.name: np.zeros(st.x[b.name].shape) for b in self.branches}
        for name, _ in blk:
            steps[name][going[name]] = self._draw_block_steps(k, by[name], int(going[name].sum()))
        q, raw = propose_block(blk, st.x, going, steps, self.periods)
        logp = orj.compute_log_prior(q, st.inds, self.branches)
        here, total = rgm.fix_logp_gibbs(logp, going, blk, st.inds)
        logl = orj.compute_log_like(q, st.inds, logp, self.branches, self.t, self.y, self.sigma, self.fill, like_fn=self.like_fn)
        u_acc = self._draw_block_accept(k)
        accepted, lnpdiff = self._accept(np.zeros((self.T, self.W)), logl, logp, u_acc)
        self.facts.proposal(self.periods, st.x, raw, q, st.inds, accepted)
        if rec is not None:
            rec.update(block=k, steps=steps, going=going, q=q, logp=logp.copy(), logl=logl.copy(), u_acc=u_acc, lnpdiff=lnpdiff,
                       accepted=accepted, here=here, total=total, L_before=st.L.copy(), P_before=st.P.copy(), betas=st.betas.copy(),
                       x_before={n: v.copy() for n, v in st.x.items()})
        orj.update(st, q, st.inds, logl, logp, accepted)
        self.mh_accepted += accepted
        self.num_proposals += 1
        return accepted


# ---- the fixtures -----------------------------------------------------------------------------------------------------------------------------
def fixture_branches(fx):
    names = [str(k) for k in fx["branch_names"]]
    if any(f"{k}_prior_kind" in fx for k in names):
        from tests import rj_prior_terms as rpt
        brs = rpt.fixture_branches(fx)
    else:
        kinds = {"gauss": orj.KIND_PULSE, "sine": orj.KIND_SINE}
        brs = [orj.Branch(k, kinds[k], [tuple(r) for r in fx[f"{k}_box"]], int(fx["nl_max"][i]), int(fx["nl_min"][i])) for i, k in enumerate(names)]
    for b in brs:
        b.cov = np.asarray(fx[f"cov_{b.name}"], dtype=np.float64)
    return brs


def fixture_periods(fx, branches):
    return {b.name: np.asarray(fx[f"period_{b.name}"], dtype=np.float64) for b in branches}


def fixture_oracle(fx, record=True):
    brs = fixture_branches(fx)
    per = fixture_periods(fx, brs)
    R, G = np.random.RandomState(int(fx["seed_construct"])), np.random.RandomState(int(fx["seed_run"]))
    x0 = {b.name: fx[f"x0_{b.name}"] for b in brs}
    inds0 = {b.name: fx[f"inds0_{b.name}"] for b in brs}
    common = (brs, x0, inds0, fx["t"], fx["y"], float(fx["sigma"]), R, G, fx["betas0"])
    kind, schedule = str(fx["in_model"]), str(fx["rj_moves"])
    if kind == "group":
        return PeriodicGroupOracle(per, int(fx["nfriends"]), rgr.fixture_key(fx), int(fx["n_iter_update"]), *common, record=record,
                                   schedule=schedule, group_a=float(fx["a"]))
    if kind == "gibbs":
        return PeriodicGibbsOracle(per, rgm.parse_setup(GIBBS_SETUP, brs), *common, record=record, schedule=schedule)
    return PeriodicOracle(per, *common, record=record, schedule=schedule, in_model=kind, a=float(fx["a"]), live_dangerously=True)


# ---- production cases (tests/test_hip_rj_periodic.py replays them; tests/test_rj_periodic.py sizes them on the CPU) ---------------------------
# T = 4, W = 64, 12 iterations per in-model move.  kinds: tests/leaf_kinds names; the LAST branch's parameter 2 is periodic with period
# 2 pi (the sine phase; the chirp's third parameter has the same box).  "record_past_64": 72 coordinates, so the periodic coordinates
# of the sine slots 10 and 11 have record indices >= 64.
PRODUCTION_ITERS = 12
PRODUCTION_CASES = {
    "gaussian": dict(kinds=("pulse", "sine"), nl=(2, 2), move="gaussian", schedule="separate_branches"),
    "gaussian_full_covariance": dict(kinds=("pulse", "sine"), nl=(2, 2), move="gaussian", schedule="none", chol=True),
    "stretch": dict(kinds=("pulse", "sine"), nl=(2, 2), move="stretch", schedule="together"),
    "group": dict(kinds=("pulse", "sine"), nl=(2, 2), move="group", schedule="separate_branches"),
    "gibbs": dict(kinds=("pulse", "sine"), nl=(2, 2), move="gibbs", schedule="iterate_branches"),
    "wide_stretch": dict(kinds=("lorentz", "chirp"), nl=(2, 2), move="stretch", schedule="separate_branches"),
    "wide_gaussian": dict(kinds=("lorentz", "chirp"), nl=(2, 2), move="gaussian", schedule="separate_branches"),
    "record_past_64": dict(kinds=("pulse", "sine"), nl=(12, 12), move="gaussian", schedule="separate_branches"),
}


def production_problem(name, T=4, W=64, ndata=40, sigma=3.0, seed=None):
    """-> dict(branches (tests/leaf_kinds.Branch), obr (the oracle's), periods, t, y, sigma, x, inds, betas, scale, chol, like_fn, key):
    every slot holds a leaf from the box, masks at random; the periodic parameter of the active leaves starts within 0.1 of the seam, on
    both sides, and that of the dead ones outside [0, 2 pi).  ``name``: a case of PRODUCTION_CASES, or a row like them with a ``seed``
    (tests/rj_limit_moves.py)."""
    from tests import leaf_kind_cases as cases
    from tests import leaf_kinds as lk
    c = PRODUCTION_CASES[name] if isinstance(name, str) else name
    brs = cases.branches_of(c["kinds"], c["nl"])
    rs = np.random.RandomState(1000 + sorted(PRODUCTION_CASES).index(name) if seed is None else seed)
    t = np.linspace(-1, 1, ndata)
    y = cases.make_data(brs, t, sigma, rs)
    x, inds = cases.random_state(brs, T, W, rs)
    last = brs[-1].name
    inds[last][..., 0] = True
    d = rs.uniform(0.002, 0.1, size=inds[last].shape)
    side = rs.rand(*inds[last].shape) < 0.5
    far = np.array([-1.3, TWO_PI + 0.7, 40.0, -25.0])[rs.randint(4, size=inds[last].shape)] + rs.uniform(-0.05, 0.05, size=inds[last].shape)
    x[last][..., 2] = np.where(inds[last], np.where(side, d, TWO_PI - d), far)
    scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in brs]
    chol = None
    if c.get("chol"):
        chol = np.stack([np.diag(sc) + np.tril(0.4 * sc[:, None] * rs.randn(3, 3), -1) for sc in scale])
    obr = [b.to_oracle(cov=np.diag(sc ** 2) if chol is None else chol[i] @ chol[i].T) for i, (b, sc) in enumerate(zip(brs, scale))]
    wide = any(k not in ("pulse", "sine") for k in c["kinds"])
    periods = {b.name: np.zeros(b.ndim) for b in brs}
    periods[last][2] = TWO_PI
    return dict(branches=brs, obr=obr, periods=periods, periodic={last: {2: TWO_PI}}, t=t, y=y, sigma=sigma, x=x, inds=inds,
                betas=0.5 ** np.arange(T), scale=scale, chol=chol, like_fn=lk.like_fn(c["kinds"]) if wide else None,
                key={b.name: 1 for b in brs}, T=T, W=W, move=c["move"], schedule=c["schedule"], wide=wide)


def production_oracle(p, cls_of=lambda cls: cls, R=None, G=None, **kw):
    """The specification of a production case on the problem's start (``cls_of``: wraps the class, for a replay's draw sources)."""
    common = (p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], R, G, p["betas"])
    kw = dict(record=True, schedule=p["schedule"], like_fn=p["like_fn"], **kw)
    if p["move"] == "group":
        return cls_of(PeriodicGroupOracle)(p["periods"], 3, p["key"], 3, *common, **kw)
    if p["move"] == "gibbs":
        return cls_of(PeriodicGibbsOracle)(p["periods"], rgm.parse_setup([b.name for b in p["obr"]], p["obr"]), *common, skip_empty=False, **kw)
    return cls_of(PeriodicOracle)(p["periods"], *common, in_model=p["move"], **kw)


__all__ = ["PeriodicOracle", "PeriodicGroupOracle", "PeriodicGibbsOracle", "SeamFacts", "distance", "wrap"]
