"""Specification of the in-model Gaussian move in Gibbs blocks over branches and leaf slots on leaf-packing records
(``GaussianMove(cov, gibbs_sampling_setup=[...])`` of the reference on a state of several branches and leaves: move.py:113-402 under
mh.py:79-193, gaussian.py:68-115), stated once on the oracle's functions (oracle/eryn_oracle_rj.py is imported, not edited).

Per block, in list order (``block`` below):
  1  a leaf slot is a member of the block if any coordinate of its mask row is true (``ir_keep``, move.py:278); a branch given by name
     or with None is a member with every slot
  2  the moved leaves are the ACTIVE leaves of member slots; ``rng="numpy"``: per branch of the block, in the block's own branch
     order, one ``R.multivariate_normal(0, cov[name], size=n)`` over them in ascending (rung, walker, slot) (gaussian.py:96-108),
     then one ``R.rand(T, W)`` (mh.py:171)
  3  q = x + step on those leaves; every coordinate whose mask entry is false gets the old value back, bit for bit (move.py:322-324)
  4  log-prior over every active leaf of every branch, then fix_logp_gibbs (move.py:368-402) AS THE REFERENCE COUNTS: ``here`` = the
     moved leaves, ``total`` = here + every leaf of the branches outside the block; here == 0 -> -inf where total != 0, 0.0 where
     total == 0.  (A block's own branches count by their member slots only: a walker whose only leaves sit in non-member slots of
     the block's branches has total == 0, gets 0.0 and is evaluated as it stands.  A walker without any leaf gets 0.0.)
  5  likelihood (not where the log-prior is infinite or the walker holds no leaf), tempered accept test with factors 0, update;
     accepted += keep, num_proposals += 1
  6  a block for which no walker of any rung has a moved leaf is skipped before any draw (mh.py:105-107)
  7  one swap cascade with adaptation behind the last block (mh.py:190-191); the move's accept mask is the last block's that ran.

``block_by_difference`` is the production launch's likelihood (csrc/hens_rj_gibbs.h): the walker's resident template updated leaf by
leaf, ``template = (template - leaf_old) + leaf_new`` per data point over the moved leaves in ascending (branch, slot) order."""
import os

import numpy as np

from oracle import eryn_oracle as base
from oracle import eryn_oracle_rj as orj

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURES = ["rjg1", "rjg2", "rjg3"]
# the three blocks of rjg1 / the per-slot blocks of rjg2 / the per-branch blocks of rjg3, as arguments of the reference's constructor
RJG1_GAUSS_MASK = np.array([[1, 1, 1], [1, 0, 1], [0, 0, 0], [0, 0, 0]], dtype=bool)      # slots 0 and 1; slot 1's centre is frozen
RJG1_PAIR = {"gauss": np.array([[0, 0, 0], [0, 0, 0], [1, 1, 1], [1, 1, 1]], dtype=bool), "sine": np.array([[1, 1, 0], [1, 1, 1]], dtype=bool)}


def fixture_setup(name):
    """``gibbs_sampling_setup`` of a fixture, in the reference's forms."""
    if name == "rjg1":
        return [("gauss", RJG1_GAUSS_MASK.copy()), {k: v.copy() for k, v in RJG1_PAIR.items()}, "sine"]
    if name == "rjg2":
        return [("gauss", np.arange(4)[:, None] == np.full((4, 3), s)) for s in range(4)]
    if name == "rjg3":
        return ["gauss", "sine"]
    raise KeyError(name)


def load_fixture(name):
    with np.load(os.path.join(HERE, "golden", "rj_gibbs", name + ".npz"), allow_pickle=False) as f:
        return {k: f[k] for k in f.files}


def parse_setup(setup, branches):
    """-> per block a list of (branch name, mask bool [nleaves_max, ndim]) in the block's branch order (move.py:113-221; a name or
    None: every coordinate)."""
    by = {b.name: b for b in branches}
    items = setup if isinstance(setup, list) else [setup]
    blocks = []
    for item in items:
        if isinstance(item, str):
            pairs = [(item, None)]
        elif isinstance(item, tuple):
            pairs = [item]
        elif isinstance(item, dict):
            pairs = list(item.items())
        else:
            raise ValueError("If providing a list for gibbs_sampling_setup, each item needs to be a string, tuple, or dict.")
        blocks.append([(k, np.ones((by[k].nleaves_max, by[k].ndim), dtype=bool) if m is None else np.asarray(m, dtype=bool)) for k, m in pairs])
    return blocks


def table_of(blocks, branches):
    """The blocks as hens_rj_set_gibbs takes them: bool [nblocks, ncoord] in record layout."""
    off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in branches])
    names = [b.name for b in branches]
    t = np.zeros((len(blocks), int(off[-1])), dtype=bool)
    for k, blk in enumerate(blocks):
        for name, m in blk:
            bi = names.index(name)
            t[k, off[bi]:off[bi + 1]] = m.reshape(-1)
    return t


def blocks_of_table(table, branches):
    """... and back: a branch is in a block if it has a true coordinate there (what the device reads out of the table)."""
    off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in branches])
    out = []
    for row in np.asarray(table, dtype=bool):
        blk = []
        for bi, b in enumerate(branches):
            m = row[off[bi]:off[bi + 1]].reshape(b.nleaves_max, b.ndim)
            if m.any():
                blk.append((b.name, m))
        out.append(blk)
    return out


def moved_leaves(blk, inds):
    """Rule 1 / 2: {name: bool [T, W, nleaves_max]} the active leaves of the block's member slots, in the block's branch order."""
    return {name: inds[name] & m.any(axis=-1)[None, None, :] for name, m in blk}


def fix_logp_gibbs(logp, going, blk, inds):
    """Rule 4, move.py:368-402 as written."""
    here = np.zeros(logp.shape, dtype=int)
    for g in going.values():
        here += g.sum(axis=-1)
    total = here.copy()
    for name, iv in inds.items():
        if name not in going:
            total += iv.sum(axis=-1)
    logp[(total != 0) & (here == 0)] = -np.inf
    logp[(total == 0) & (here == 0)] = 0.0
    return here, total


def propose(blk, x, going, steps):
    """Rule 3.  steps: {name: [T, W, nleaves_max, ndim]} (read on the moved leaves)."""
    q = {k: v.copy() for k, v in x.items()}
    for name, m in blk:
        g = going[name]
        q[name][g] = x[name][g] + 1.0 * steps[name][g]
        q[name][:, :, ~m] = x[name][:, :, ~m]                                     # move.py:322-324
    return q


def leaf_values(b, p, t):
    """One leaf's values at the data points, the operation order of the device's per-point forms (oracle/eryn_oracle_rj.py's model
    functions; the pulse's c * c as the kernels square it)."""
    from tests import leaf_kinds as lk
    return lk.leaf_value(getattr(b, "kind_name", b.kind), np.asarray(p, dtype=np.float64), t)


def block_by_difference(branches, blk, x, q, going, tmpl, t, y, sigma):
    """The production launch's template and log-likelihood of the proposal: per walker, over its moved leaves in ascending (branch of
    the record, slot) order, per data point ``tmpl = (tmpl - leaf_old) + leaf_new``; ``-1/2 sum(((tmpl - y) / sigma)^2)`` (the device
    reduces the sum in a tree over its lanes: compare to rounding, not bit for bit).  tmpl: [T, W, ndata]."""
    out = tmpl.copy()
    for b in branches:
        if b.name not in going:
            continue
        for tt, w, n in zip(*np.where(going[b.name])):
            out[tt, w] = (out[tt, w] - leaf_values(b, x[b.name][tt, w, n], t)) + leaf_values(b, q[b.name][tt, w, n], t)
    return out, -0.5 * np.sum(((out - y) / sigma) ** 2, axis=-1)


class GibbsOracle(orj.OracleRJSampler):
    """The pinned oracle with its in-model move replaced by the block-by-block move; birth / death, the cascades and the draws' sources
    are the oracle's.  ``blocks``: ``parse_setup``'s.  ``skip_empty`` False: the device's production rule - no block is skipped."""

    def __init__(self, blocks, *a, skip_empty=True, **kw):
        super().__init__(*a, **kw)
        self.blocks, self.skip_empty = blocks, skip_empty
        self.num_proposals = 0

    def _draw_block_steps(self, k, b, n):
        return self._draw_steps(b, n)

    def _draw_block_accept(self, k):
        return self._draw_accept("mh")

    def block(self, k, rec=None):
        """One block (rules 1 - 6); returns its accept mask, or None where it is skipped."""
        st, blk = self.st, self.blocks[k]
        by = {b.name: b for b in self.branches}
        going = moved_leaves(blk, st.inds)
        if self.skip_empty and not any(g.any() for g in going.values()):
            return None
        steps = {b.name: np.zeros(st.x[b.name].shape) for b in self.branches}
        for name, _ in blk:
            steps[name][going[name]] = self._draw_block_steps(k, by[name], int(going[name].sum()))
        q = propose(blk, st.x, going, steps)
        logp = orj.compute_log_prior(q, st.inds, self.branches)
        here, total = fix_logp_gibbs(logp, going, blk, st.inds)
        logl = orj.compute_log_like(q, st.inds, logp, self.branches, self.t, self.y, self.sigma, self.fill, like_fn=self.like_fn)
        u_acc = self._draw_block_accept(k)
        accepted, lnpdiff = self._accept(np.zeros((self.T, self.W)), logl, logp, u_acc)
        if rec is not None:
            rec.update(block=k, steps=steps, going=going, q=q, logp=logp.copy(), logl=logl.copy(), u_acc=u_acc, lnpdiff=lnpdiff,
                       accepted=accepted, here=here, total=total, L_before=st.L.copy(), P_before=st.P.copy(), betas=st.betas.copy(),
                       x_before={n: v.copy() for n, v in st.x.items()})
        orj.update(st, q, st.inds, logl, logp, accepted)
        self.mh_accepted += accepted
        self.num_proposals += 1
        return accepted

    def mh_move(self, rec=None):
        self._draw_move_choice()
        accepted = np.zeros((self.T, self.W), dtype=bool)                          # mh.py:77
        sub = []
        for k in range(len(self.blocks)):
            r = {} if rec is not None else None
            acc = self.block(k, r)
            if acc is None:
                continue
            accepted = acc
            if rec is not None:
                self._snapshot(r, "upd_")
                sub.append(r)
        if rec is not None:
            rec.update(gibbs=sub, mh_accepted=accepted, betas_before=self.st.betas.copy(), time_before=self.time)
            self._snapshot(rec, "mhupd_")
        self._pt(True, rec)
        return accepted


def fixture_branches(fx):
    """The fixture's branches: the oracle's box branches, or (prior kinds stored: rjg3) tests/rj_prior_terms.TermBranch."""
    names = ["gauss", "sine"] if "branch_names" not in fx else [str(k) for k in fx["branch_names"]]
    if "gauss_prior_kind" in fx:
        from tests import rj_prior_terms as rpt
        return rpt.fixture_branches(fx)
    kinds = {"gauss": orj.KIND_PULSE, "sine": orj.KIND_SINE}
    return [orj.Branch(k, kinds[k], [tuple(r) for r in fx[f"{k}_box"]], int(fx["nl_max"][i]), int(fx["nl_min"][i]),
                       cov=np.diag(np.ones(3)) * float(fx["cov_factor"])) for i, k in enumerate(names)]


def fixture_oracle(name, fx, record=True):
    brs = fixture_branches(fx)
    R, G = np.random.RandomState(int(fx["seed_construct"])), np.random.RandomState(int(fx["seed_run"]))
    x0 = {b.name: fx[f"x0_{b.name}"] for b in brs}
    inds0 = {b.name: fx[f"inds0_{b.name}"] for b in brs}
    return GibbsOracle(parse_setup(fixture_setup(name), brs), brs, x0, inds0, fx["t"], fx["y"], float(fx["sigma"]), R, G, fx["betas0"],
                       record=record, schedule=str(fx["rj_moves"]))


__all__ = ["GibbsOracle", "base"]
