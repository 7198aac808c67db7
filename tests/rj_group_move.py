"""Specification of the group stretch move with a stationary friend table on leaf-packing records (the reference's
``GroupStretchMove``: moves/group.py:122-281, moves/groupstretch.py:34-120 over stretch.py:103-158, with ``gibbs_sampling_setup=None``
and ONE friend rule, nearest friends by one key parameter per branch), stated once on the oracle's functions (oracle/eryn_oracle_rj.py
is imported, not edited).  csrc/hens_rj_group.h carries the same rules in its head comment.

  1  friend table (rebuild): per branch the ACTIVE leaves of the cold rung in ascending (walker, slot) order, sorted stably by
     ``x[key] + 0.0`` (-0.0 keyed as +0.0) ascending: ``keys[n_b]``, ``tab[n_b, ndim]``; no uniqueness filter; n_b may be 0
  2  window of a leaf: nf = min(nfriends, n_b) contiguous entries from ``start`` on, found by the greedy walk of ``window`` from
     ``lower_bound(keys, x[key])`` - step left when there is an entry on the left and (none on the right or ``|x - keys[lo - 1]| <=
     |keys[hi] - x|``), else right.  Its keys are the keys of the nf entries a stable argsort of ``|x - keys|`` puts first
     (``argsort_entries``), value for value; with all keys different they are the same entries.  Among entries of the SAME key left of
     x the walk takes the ones next to x and the argsort the ones of lowest index, so with duplicates the argsort's set need not be
     contiguous - a window is
  3  at a rebuild every active leaf of every rung gets its window from its position then; a leaf born since the last group move gets
     its window at the head of the next one (``fix``); otherwise the window stays with the leaf, rides the swaps with its walker and is
     dropped (-1) when the leaf dies
  4  a rebuild happens at the move's call number m when m % n_iter_update == 0, from the state in front of the move; m restarts with
     a new oracle (the device: at an upload, and when the group is set)
  5  one zz = ((a - 1) u + 1)^2 / a per walker; per active leaf a pick j in [0, nf), c = tab[start + j], q = c - (c - x) zz on all
     its parameters; dead slots and leaves of a branch with n_b == 0 keep their bits; factors = (sum_b nleaves_max_b ndim_b - 1) log zz
  6  log-prior over the active leaves, fix_logp_gibbs with every branch under proposal, likelihood (not where the log-prior is -inf or
     the walker has no leaf), ``factors + beta logl + logp - (beta L + P) > log u``, update; accepted += mask, num_proposals += 1, one
     swap cascade with adaptation.

``rng="numpy"`` draw order of the move: the move choice from R; per branch in order ``G.randint(nf_b, size=n_active_b)`` over the
active leaves in ascending (rung, walker, slot), skipped where nf_b == 0; behind branch 0 ``R.rand(T, W)`` for zz; ``R.rand(T, W)`` for
the accept; the swap draws."""
import os

import numpy as np

from oracle import eryn_oracle as base
from oracle import eryn_oracle_rj as orj

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["grp1", "grp2", "grp3"]


def load_fixture(name):
    with np.load(os.path.join(HERE, "golden", "rj_group", name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def friend_table(xb, ib, key):
    """Rule 1 for one branch: coords [T, W, nl, nd], inds [T, W, nl] -> (keys [n], tab [n, nd])."""
    leaves = xb[0][ib[0]]                                   # cold rung, ascending (walker, slot)
    k = leaves[:, key] + 0.0
    order = np.argsort(k, kind="stable")
    return k[order], leaves[order].copy()


def window(keys, nfriends, xk):
    """Rule 2: the first index of the leaf's window (0 where the table is empty)."""
    n = len(keys)
    nf = min(int(nfriends), n)
    lo = hi = int(np.searchsorted(keys, xk, side="left"))
    for _ in range(nf):
        if lo > 0 and (hi == n or abs(xk - keys[lo - 1]) <= abs(keys[hi] - xk)):
            lo -= 1
        else:
            hi += 1
    assert hi - lo == nf
    return lo


def argsort_entries(keys, nfriends, xk):
    """What the window stands for: the table entries a stable argsort of the distances puts first, ascending."""
    nf = min(int(nfriends), len(keys))
    return np.sort(np.argsort(np.abs(xk - keys), kind="stable")[:nf])


def check_window(keys, nfriends, xk):
    """Rule 2's assertion for one leaf: the window's keys are the argsort's, and the same entries where the keys are all different."""
    keys = np.asarray(keys, dtype=np.float64)
    st, nf = window(keys, nfriends, xk), min(int(nfriends), len(keys))
    want = argsort_entries(keys, nfriends, xk)
    assert 0 <= st and st + nf <= len(keys)
    assert np.array_equal(keys[st:st + nf], np.sort(keys[want])), (keys, nfriends, xk, st, want)
    if np.all(np.diff(keys) > 0):
        assert np.array_equal(np.arange(st, st + nf), want), (keys, nfriends, xk, st, want)
    return st


class GroupOracle(orj.OracleRJSampler):
    """The pinned oracle with its in-model move replaced by the group stretch move; birth / death, the cascades and the draws' sources
    are the oracle's.  ``key``: {branch name: parameter index} (or one int for every branch)."""

    def __init__(self, nfriends, key, n_iter_update, *a, group_a=2.0, check=True, **kw):
        super().__init__(*a, **kw)
        self.nfriends, self.n_iter_update, self.group_a, self.check = int(nfriends), int(n_iter_update), float(group_a), check
        self.key = {b.name: int(key[b.name] if isinstance(key, dict) else key) for b in self.branches}
        self.m, self.num_proposals = 0, 0
        self.keys = {b.name: np.zeros(0) for b in self.branches}
        self.tab = {b.name: np.zeros((0, b.ndim)) for b in self.branches}
        self.start = {b.name: np.full((self.T, self.W, b.nleaves_max), -1, dtype=np.int64) for b in self.branches}
        self.snap = {b.name: np.zeros((self.T, self.W, b.nleaves_max), dtype=bool) for b in self.branches}

    # ---- draw sources (a replay of the device's production draws overrides these) ----
    def _draw_picks(self, bi, b, nf, going):
        return self.G.randint(nf, size=int(going.sum()))                          # find_friends: the GLOBAL stream

    def _draw_zz_group(self):
        return self.R.rand(self.T, self.W)                                         # stretch.py:129-132

    # ---- table and windows ----
    def nf(self, name):
        return min(self.nfriends, len(self.keys[name]))

    def _window(self, name, xk):
        return check_window(self.keys[name], self.nfriends, xk) if self.check else window(self.keys[name], self.nfriends, xk)

    def _assign(self, name, where):
        x = self.st.x[name]
        for t, w, n in zip(*np.where(where)):
            self.start[name][t, w, n] = self._window(name, x[t, w, n, self.key[name]])

    def rebuild(self):
        """Rules 1 and 3 at a rebuild."""
        for b in self.branches:
            self.keys[b.name], self.tab[b.name] = friend_table(self.st.x[b.name], self.st.inds[b.name], self.key[b.name])
            self.start[b.name][:] = -1
            self._assign(b.name, self.st.inds[b.name])
            self.snap[b.name] = self.st.inds[b.name].copy()

    def fix(self):
        """Rule 3 at the head of a move: newborn leaves get a window, dead slots lose theirs, the masks are remembered."""
        born = {}
        for b in self.branches:
            inds = self.st.inds[b.name]
            born[b.name] = inds & (~self.snap[b.name] | (self.start[b.name] < 0))
            self.start[b.name][~inds] = -1
            self._assign(b.name, born[b.name])
            self.snap[b.name] = inds.copy()
        return born

    def _pt(self, adapt, rec):
        """The oracle's cascade; windows and mask snapshots ride with their walkers (tempering.py:376-480 swaps the branch
        supplementals)."""
        r = {} if rec is None else rec
        super()._pt(adapt, r)
        if self.T < 2:
            return
        riders = [self.start[b.name] for b in self.branches] + [self.snap[b.name] for b in self.branches]
        for j, i in enumerate(range(self.T - 1, 0, -1)):
            sel = r["sel"][j]
            a_, b_ = r["iperm"][j][sel], r["i1perm"][j][sel]
            for arr in riders:
                tmp = arr[i, a_].copy()
                arr[i, a_] = arr[i - 1, b_]
                arr[i - 1, b_] = tmp

    # ---- the move ----
    def propose(self, picks, u_zz):
        """Rule 5.  picks: {name: int [T, W, nl]} (read on active leaves of branches with a table)."""
        st = self.st
        zz = ((self.group_a - 1.0) * u_zz + 1) ** 2.0 / self.group_a
        q = {k: v.copy() for k, v in st.x.items()}
        for b in self.branches:
            if self.nf(b.name) == 0:
                continue
            going = st.inds[b.name]
            assert np.all(self.start[b.name][going] >= 0), "an active leaf without a window"
            c = self.tab[b.name][self.start[b.name][going] + picks[b.name][going]]
            s = st.x[b.name][going]
            zz_leaf = np.broadcast_to(zz[:, :, None], going.shape)[going][:, None]
            q[b.name][going] = c - (c - s) * zz_leaf
        ndim_total = sum(b.nleaves_max * b.ndim for b in self.branches)
        return q, (ndim_total - 1.0) * np.log(zz)

    def group_move(self, rec=None, forced=None):
        """One move (rules 3 - 6) and its cascade.  forced: dict(picks={name: [T, W, nl]}, u_zz, u_acc) in place of the draws."""
        st = self.st
        self._draw_move_choice()
        rebuilt = self.m % self.n_iter_update == 0
        if rebuilt:
            self.rebuild()
        born = self.fix()
        if rec is not None:
            self._snapshot(rec, "pre_")
            rec.update(rebuilt=rebuilt, born=born, keys={k: v.copy() for k, v in self.keys.items()}, tab={k: v.copy() for k, v in self.tab.items()},
                       start={k: v.copy() for k, v in self.start.items()}, betas_before=st.betas.copy(), time_before=self.time)
        picks = {}
        u_zz = None
        for bi, b in enumerate(self.branches):
            going = st.inds[b.name]
            picks[b.name] = np.zeros(going.shape, dtype=np.int64)
            if forced is not None:
                picks[b.name] = np.asarray(forced["picks"][b.name], dtype=np.int64)
            elif self.nf(b.name) > 0:
                picks[b.name][going] = self._draw_picks(bi, b, self.nf(b.name), going)
            if bi == 0:
                u_zz = forced["u_zz"] if forced is not None else self._draw_zz_group()
        q, factors = self.propose(picks, u_zz)
        names = [b.name for b in self.branches]
        logp = orj.compute_log_prior(q, st.inds, self.branches)
        orj.fix_logp_gibbs(logp, st.inds, names)
        logl = orj.compute_log_like(q, st.inds, logp, self.branches, self.t, self.y, self.sigma, self.fill, like_fn=self.like_fn)
        u_acc = forced["u_acc"] if forced is not None else self._draw_accept("mh")
        accepted, lnpdiff = self._accept(factors, logl, logp, u_acc)
        if rec is not None:
            rec.update(picks=picks, u_zz=u_zz, u_acc=u_acc, q={k: v.copy() for k, v in q.items()}, factors=factors, logp=logp.copy(),
                       logl=logl.copy(), lnpdiff=lnpdiff, mh_accepted=accepted, L_before=st.L.copy(), P_before=st.P.copy())
        orj.update(st, q, st.inds, logl, logp, accepted)
        self.mh_accepted += accepted
        self.num_proposals += 1
        self.m += 1
        if rec is not None:
            self._snapshot(rec, "mhupd_")
        self._pt(True, rec)
        return accepted

    def mh_move(self, rec=None):
        return self.group_move(rec)


def fixture_branches(fx):
    """The fixture's branches: the oracle's box branches, or (prior kinds stored: grp3) tests/rj_prior_terms.TermBranch."""
    names = [str(k) for k in fx["branch_names"]]
    if any(f"{k}_prior_kind" in fx for k in names):
        from tests import rj_prior_terms as rpt
        return rpt.fixture_branches(fx)
    kinds = {"gauss": orj.KIND_PULSE, "sine": orj.KIND_SINE}
    return [orj.Branch(k, kinds[k], [tuple(r) for r in fx[f"{k}_box"]], int(fx["nl_max"][i]), int(fx["nl_min"][i])) for i, k in enumerate(names)]


def fixture_key(fx):
    return {str(k): int(v) for k, v in zip(fx["branch_names"], fx["key"])}


def fixture_oracle(fx, record=True):
    brs = fixture_branches(fx)
    R, G = np.random.RandomState(int(fx["seed_construct"])), np.random.RandomState(int(fx["seed_run"]))
    x0 = {b.name: fx[f"x0_{b.name}"] for b in brs}
    inds0 = {b.name: fx[f"inds0_{b.name}"] for b in brs}
    return GroupOracle(int(fx["nfriends"]), fixture_key(fx), int(fx["n_iter_update"]), brs, x0, inds0, fx["t"], fx["y"], float(fx["sigma"]), R, G,
                       fx["betas0"], record=record, schedule=str(fx["rj_moves"]), group_a=float(fx["a"]))


__all__ = ["GroupOracle", "base"]
