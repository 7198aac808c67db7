"""Reversible-jump leaf packing on the MI355X (BASELINE config 4).

Host-side mirror of the reference's multi-branch ``State`` (state.py:330-562: ``branches[name].coords[T, W, nleaves_max,
ndim]`` + ``branches[name].inds[T, W, nleaves_max]``) for the device path of ``include/hipensemble.h`` ``hens_rj_*``:
:class:`RJEngine` packs a variable-dimension ensemble into leaf-packing records, runs the in-model ``GaussianMove``
(mh.py:56-193, gaussian.py:68-270), the ``DistributionGenerateRJ`` birth / death move (distgenrj.py:35-222,
rj.py:145-388) and the PT sweeps on the device - teacher-forced with the reference's draws (parity) or with device-side
Philox draws (``step``) - and unpacks snapshots with the reference's NaN fill of unused leaves
(backends/backend.py:1049-1059).  The model is the reference tests' own template model (tests/test_eryn.py:38-92)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check, f64, ptr
from .engine import ChainStoreCalls, HipEnsemble
from .prior import prior_spec, term_arrays

KIND_PULSE, KIND_SINE = 0, 1
# the leaf kinds the device evaluates, name -> (id, parameters per leaf) (include/hipensemble.h: HENS_RJ_KIND_*): value at data point t
#   pulse (a, b, c) a exp(-(t - b)^2 / (2 c^2))   sine (a, b, c) a sin(2 pi b t + c)   offset (a) a   ramp (a, b) a + b t
#   lorentz (a, b, c) a / (1 + ((t - b) / c)^2)   chirp (a, b, c) a sin(2 pi b t + c t^2)
#   burst (a, t0, w, f) a exp(-((t - t0) / w)^2) cos(2 pi f (t - t0))
LEAF_KINDS = {"pulse": (0, 3), "sine": (1, 3), "offset": (2, 1), "ramp": (3, 2), "lorentz": (4, 3), "chirp": (5, 3), "burst": (6, 4)}
_KINDS = {**{k: v[0] for k, v in LEAF_KINDS.items()}, "gauss": KIND_PULSE, **{v[0]: v[0] for v in LEAF_KINDS.values()}}
_WIDTH = {v[0]: v[1] for v in LEAF_KINDS.values()}


def _leaf_prior(branch, box):
    """The prior of one leaf, from ``box`` - a list of (lo, hi) per leaf parameter - or, in its place, an
    ``eryn_amd.prior.ProbDistContainer`` or anything it accepts (a dict of distributions, frozen SciPy ``uniform`` / ``loguniform`` /
    ``norm`` among them): ``eryn_amd.prior.prior_spec``.  Sets ``lo`` / ``hi`` (the inclusive supports), ``terms`` (the arguments of
    hens_rj_set_prior_terms for this branch), ``prior`` (the container, None for bounds), ``is_box`` and - all-uniform branches -
    ``leaf_logp``, the constant leaf log-density (None otherwise: the density is no constant)."""
    spec = prior_spec(box)
    branch.prior, branch.terms, branch.lo, branch.hi, branch.is_box, branch.leaf_logp = spec


class TemplateBranch:
    """One model type: leaf kind (a name of LEAF_KINDS; "gauss" is "pulse"), a uniform box per leaf parameter - as many as the kind
    has - or a prior container in its place (``_leaf_prior``: uniform, log-uniform and normal parameters), leaf budget."""

    def __init__(self, name, kind, box, nleaves_max, nleaves_min=0):
        self.name, self.kind = str(name), _KINDS[kind]
        _leaf_prior(self, box)
        self.ndim = _WIDTH[self.kind]
        if self.lo.shape != (self.ndim,):
            raise ValueError(f"a leaf of this kind has {self.ndim} parameter{'s' if self.ndim != 1 else ''}: a box of {self.lo.shape[0]}")
        self.nleaves_max, self.nleaves_min = int(nleaves_max), int(nleaves_min)


class LeafBranch:
    """One model type WITHOUT a device likelihood (round 6): a uniform box per leaf parameter - 1 to 4 of them, the reference's
    ``ndims[name]`` (ensemble.py:325-329) - or a prior container in its place (``_leaf_prior``), and a leaf budget.  For chains whose
    likelihood is the caller's Python function (CallableLikelihood, hens_rj_set_model_general)."""
    kind = 0

    def __init__(self, name, box, nleaves_max, nleaves_min=0):
        self.name = str(name)
        _leaf_prior(self, box)
        self.ndim = int(self.lo.shape[0])
        if not 1 <= self.ndim <= 4:
            raise NotImplementedError("a leaf has 1 to 4 parameters")
        self.nleaves_max, self.nleaves_min = int(nleaves_max), int(nleaves_min)


class _TemplateLikelihood:
    kind = _lib.LIKE_TEMPLATE

    def __init__(self, ndim):
        self.ndim = ndim

    def _install(self, lib, ctx):
        pass


class CallableLikelihood:
    """A user ``log_like_fn`` for a state of several branches / leaves, called the way ``EnsembleSampler.compute_log_like`` calls
    it (ensemble.py:1219-1545): walkers with an infinite log-prior or without any active leaf are not evaluated; the active leaves
    of the others are packed per branch (``coords[inds]``: walker-major, slot order) with their group ids (utils/utility.py:8-40,
    renumbered 0..ngroups-1, ensemble.py:1306-1324); ``vectorize=True`` hands the function every group at once -
    ``fn([leaves_b0, leaves_b1, ...], [groups_b0, ...] if provide_groups, *args, **kwargs)`` - else it is called per group with
    ``[leaves_b or None for every branch]`` (:1420-1470).  Not evaluated -> ``fill_zero_leaves_val`` (:1486-1513); NaN raises.
    The proposal, prior, accept test and update around it run on the device (hens_rj_propose / hens_rj_accept)."""

    def __init__(self, fn, args=None, kwargs=None, vectorize=False, provide_groups=False, fill_zero_leaves_val=-1e300):
        self.fn, self.args, self.kwargs = fn, list(args or []), dict(kwargs or {})
        self.vectorize, self.provide_groups, self.fill = bool(vectorize), bool(provide_groups), float(fill_zero_leaves_val)
        self.ncalls = 0

    def __call__(self, x, inds, logp, names, only=None, has_reversible_jump=True):
        """x / inds: {name: [T, W, nl, ndim] / [T, W, nl]}, logp [T, W]; ``only`` [T, W] bool: the walkers a move touched (the
        others keep their log-likelihood: their entry here is never read)."""
        first = names[0]
        T, W = inds[first].shape[:2]
        for name in names:                                                  # ensemble.py:1258-1262
            xa = x[name][inds[name]]
            if np.any(np.isinf(xa)):
                raise ValueError("At least one parameter value was infinite")
            if np.any(np.isnan(xa)):
                raise ValueError("At least one parameter value was NaN")
        only = None if only is None else np.asarray(only, dtype=bool)
        if np.all(np.isinf(logp if only is None else logp[only])):          # :1272-1276
            import warnings
            warnings.warn("All points input for the Likelihood have a log prior of -inf.")
            return np.full_like(logp, -1e300)
        bad = np.isinf(logp) if only is None else (np.isinf(logp) | ~only)
        inds_copy = {k: np.array(inds[k], dtype=bool, copy=True) for k in names}
        for k in names:
            inds_copy[k][bad] = False
        gid = np.arange(T * W).reshape(T, W)
        groups = {k: np.repeat(gid[:, :, None], inds_copy[k].shape[2], axis=-1)[inds_copy[k]] for k in names}
        unique_groups = np.unique(np.concatenate([groups[k] for k in names]))
        groups_map = np.arange(len(unique_groups))
        ll_groups = []
        for k in names:
            tu, inverse = np.unique(groups[k], return_inverse=True)
            ll_groups.append(groups_map[np.isin(unique_groups, tu)][inverse])
        params_in = [x[k][inds_copy[k]] for k in names]
        ll = np.full(T * W, -1e300)
        if len(unique_groups):
            if self.vectorize:
                a = [params_in[0] if len(params_in) == 1 else params_in]
                if self.provide_groups:
                    a.append(ll_groups[0] if len(ll_groups) == 1 else ll_groups)
                results = self.fn(*a, *self.args, **self.kwargs)
                self.ncalls += 1
            else:
                results = []
                for g in groups_map:
                    arg = [None] * len(names)
                    for bi in range(len(names)):
                        keep = np.where(ll_groups[bi] == g)[0]
                        if keep.shape[0] > 0:
                            p = params_in[bi][keep]
                            if not has_reversible_jump and p.shape[0] == 1:
                                p = p[0]
                            arg[bi] = p
                    results.append(self.fn(arg[0] if len(names) == 1 else arg, *self.args, **self.kwargs))
                    self.ncalls += 1
            results = np.asarray(results)
            if results.ndim == 2 and results.shape[1] == 1:
                results = np.squeeze(results, axis=1)
            if results.ndim != 1:
                raise NotImplementedError("blobs are outside the device hot path: the likelihood must return one value per group")
            ll[unique_groups] = results
        ll[np.delete(np.arange(T * W), unique_groups)] = self.fill
        if np.any(np.isnan(ll)):
            raise ValueError("The likelihood function is returning Nan.")
        return ll.reshape(T, W)


class RJEngine(ChainStoreCalls):
    CHAIN_PREFIX = "hens_rj_chain_"

    def __init__(self, ntemps, nwalkers, branches, t, y, sigma, seed=0, device_id=0, adaptive=True,
                 adaptation_lag=10000, adaptation_time=100, stop_adaptation=-1, fill_value=-1e300, a=2.0, live_dangerously=False,
                 kinds_entry=None):
        # kinds_entry: hand the model to hens_rj_set_model_kinds (None: when a branch's kind is beyond pulse / sine)
        self.branches = list(branches)
        if not 1 <= len(self.branches) <= 4:
            raise NotImplementedError("1 to 4 branches")
        self.ncoord = sum(b.nleaves_max * b.ndim for b in self.branches)
        self.ndmax = max(b.ndim for b in self.branches)          # (the stride of the birth arrays: 3 for the pulse / sine models)
        # a model without a device likelihood: any LeafBranch, or no data (hens_rj_set_model_general; host_like steps it)
        self.general = t is None or any(not isinstance(b, TemplateBranch) for b in self.branches)
        rw = self.ncoord + len(self.branches)
        self.RW = rw + (rw & 1)                                  # even record width: 16-byte row alignment
        if self.RW > 128:
            raise NotImplementedError(f"{self.ncoord} leaf coordinates + {len(self.branches)} masks: a record holds 128 doubles")
        self.off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in self.branches])[:-1]
        self.T, self.W = int(ntemps), int(nwalkers)
        # the engine's prior box is unused on records; HipEnsemble wants one
        self.eng = HipEnsemble(self.T, self.W, self.RW, _TemplateLikelihood(self.RW), -1.0, 1.0, tempered=True,
                               adaptive=adaptive, adaptation_lag=adaptation_lag, adaptation_time=adaptation_time,
                               stop_adaptation=stop_adaptation, live_dangerously=live_dangerously, fill_value=fill_value, seed=seed,
                               device_id=device_id, a=a)
        self.lib, self.ctx = self.eng.lib, self.eng.ctx
        self.schedule = "separate_branches"
        self.in_model = "gaussian"   # the in-model move of ``step`` (set_in_model)
        self.periods = None          # set_periodic: per branch a row of periods, or None
        self.host_like = None        # a CallableLikelihood: every parity move = propose on the device, evaluate here, accept on the device
        self.mt_K, self.mt_gen = 0, None     # set_mt_proposal: tries of the multiple-try birth / death move (0: the plain move), its generators
        self.nslots = sum(b.nleaves_max for b in self.branches)
        self.group, self.group_m = None, 0   # set_group: (nfriends, n_iter_update, keys, a); the group move's call number since the last upload
        nb = len(self.branches)
        kinds = np.array([b.kind for b in self.branches], dtype=np.int32)
        nlmax = np.array([b.nleaves_max for b in self.branches], dtype=np.int32)
        nlmin = np.array([b.nleaves_min for b in self.branches], dtype=np.int32)
        # a branch with a prior term other than uniform: the model is set with a stand-in box (the terms' supports where they are
        # finite) and hens_rj_set_prior_terms replaces it; all-uniform branches ARE boxes and never reach that call
        self.prior_terms = any(not b.is_box for b in self.branches)
        lp = f64([0.0 if b.leaf_logp is None else b.leaf_logp for b in self.branches])
        self.wide = False
        if self.general:
            nds = np.array([b.ndim for b in self.branches], dtype=np.int32)
            lo, hi = self._stand_in_box()
            check(self.lib.hens_rj_set_model_general(self.ctx, nb, ptr(nds), ptr(nlmax), ptr(nlmin), ptr(lo), ptr(hi), ptr(lp)), self.ctx)
            self._set_prior_terms()
            return
        lo, hi = self._stand_in_box()
        t, y = f64(t), f64(y)
        if t.shape != y.shape or t.ndim != 1:
            raise ValueError("t and y must be 1-D arrays of the same length")
        self.wide = bool(np.any(kinds > KIND_SINE))              # (a leaf kind beyond pulse / sine: widths 1 to 4, no full covariances)
        set_model = self.lib.hens_rj_set_model_kinds if (self.wide if kinds_entry is None else kinds_entry) else self.lib.hens_rj_set_model
        check(set_model(self.ctx, nb, ptr(kinds), ptr(nlmax), ptr(nlmin), ptr(lo), ptr(hi), ptr(lp),
                        int(t.shape[0]), ptr(t), ptr(y), float(sigma)), self.ctx)
        self._set_prior_terms()

    def _stand_in_box(self):
        lo, hi = np.concatenate([b.lo for b in self.branches]), np.concatenate([b.hi for b in self.branches])
        return f64(np.where(np.isfinite(lo), lo, -1.0)), f64(np.where(np.isfinite(hi), hi, 1.0))      # (a normal parameter's support is the line)

    def _set_prior_terms(self):
        if not self.prior_terms:
            return
        check(self.lib.hens_rj_set_prior_terms(self.ctx, *map(ptr, term_arrays([b.terms for b in self.branches]))), self.ctx)

    def close(self):
        self.eng.close()

    # -- records <-> branches --------------------------------------------------------------------------------
    def pack(self, x, inds):
        """{name: coords[T, W, nl, ndim]}, {name: inds[T, W, nl]} -> records[T, W, RW]."""
        rec = np.zeros((self.T, self.W, self.RW))
        for bi, b in enumerate(self.branches):
            c = np.asarray(x[b.name], dtype=np.float64)
            if c.shape != (self.T, self.W, b.nleaves_max, b.ndim):
                raise ValueError(f"coords of branch {b.name} must have shape {(self.T, self.W, b.nleaves_max, b.ndim)}")
            c = np.where(np.isnan(c), 0.0, c)                    # a stored chain marks unused leaves with NaN
            rec[:, :, self.off[bi]:self.off[bi] + b.nleaves_max * b.ndim] = c.reshape(self.T, self.W, -1)
            m = np.asarray(inds[b.name], dtype=bool)
            rec[:, :, self.ncoord + bi] = (m * (1 << np.arange(b.nleaves_max))).sum(axis=-1)
        return rec

    def unpack(self, rec, nan_fill=False):
        x, inds = {}, {}
        for bi, b in enumerate(self.branches):
            x[b.name] = rec[:, :, self.off[bi]:self.off[bi] + b.nleaves_max * b.ndim].reshape(self.T, self.W, b.nleaves_max, b.ndim).copy()
            m = rec[:, :, self.ncoord + bi].astype(np.int64)
            inds[b.name] = ((m[:, :, None] >> np.arange(b.nleaves_max)) & 1).astype(bool)
            if nan_fill:                                         # backend.py:1049-1059
                x[b.name][~inds[b.name]] = np.nan
        return x, inds

    def steps_to_records(self, steps):
        """{name: step[T, W, nl, ndim]} (zero on unused slots) -> [T, W, ncoord] in record layout."""
        out = np.zeros((self.T, self.W, self.ncoord))
        for bi, b in enumerate(self.branches):
            out[:, :, self.off[bi]:self.off[bi] + b.nleaves_max * b.ndim] = np.asarray(steps[b.name]).reshape(self.T, self.W, -1)
        return out

    # -- state ---------------------------------------------------------------------------------------------------
    def upload(self, x, inds, logl=None, logp=None, betas=None):
        self.eng.upload(self.pack(x, inds), logl, logp, betas)
        self.group_m = 0                     # (the library restarts the group move's rebuild count at an upload)

    def download(self, nan_fill=False):
        rec, L, P, betas = self.eng.download()
        x, inds = self.unpack(rec, nan_fill=nan_fill)
        return x, inds, L, P, betas

    def eval_state(self):
        self.eng.eval_state()                                    # (log-prior on the device; log-like: the template model's)
        if self.host_like is not None:                           # ... or the host callable's
            rec, _, P, betas = self.eng.download()
            x, inds = self.unpack(rec)
            L = self.host_like(x, inds, P, [b.name for b in self.branches])
            self.eng.upload(rec, L, P, betas)

    def set_adapt_time(self, t):
        self.eng.set_adapt_time(t)

    # -- moves with a host-callable likelihood: hens_rj_propose -> the user's function -> hens_rj_accept -------------
    def _host_move(self, move, **d):
        """One teacher-forced move whose likelihood is ``self.host_like``: the device proposes and computes the log-prior, the
        host packs the active leaves and calls the user's function (CallableLikelihood), the device tests and updates."""
        self.eng.state_epoch += 1
        keepalive = {k: v for k, v in d.items() if isinstance(v, np.ndarray)}
        dr = _lib.HensRjDraws(**{k: (v.ctypes.data if isinstance(v, np.ndarray) else v) for k, v in d.items()})
        q = np.empty((self.T, self.W, self.RW))
        logp = np.empty((self.T, self.W))
        moved = np.empty((self.T, self.W), dtype=np.uint8)
        check(self.lib.hens_rj_propose(self.ctx, int(move), C.byref(dr), ptr(q), ptr(logp), ptr(moved)), self.ctx)
        del keepalive
        x, inds = self.unpack(q)
        try:
            logl = f64(self.host_like(x, inds, logp, [b.name for b in self.branches], only=moved.astype(bool)))
        except Exception:
            # the move must not stay half done: reject everything (log-like -inf fails every accept test), then re-raise
            check(self.lib.hens_rj_accept(self.ctx, ptr(np.full((self.T, self.W), -np.inf)), None), self.ctx)
            raise
        keep = np.empty((self.T, self.W), dtype=np.uint8)
        check(self.lib.hens_rj_accept(self.ctx, ptr(logl), ptr(keep)), self.ctx)
        return keep.astype(bool)

    # -- parity-mode moves -----------------------------------------------------------------------------------------
    def mh_step(self, steps, u_acc):
        st = f64(self.steps_to_records(steps))
        u = f64(u_acc, (self.T, self.W))
        if self.host_like is not None:
            return self._host_move(_lib.RJ_MOVE_MH, step=st, u_acc=u)
        keep = np.empty((self.T, self.W), dtype=np.uint8)
        check(self.lib.hens_rj_mh_step(self.ctx, ptr(st), ptr(u), ptr(keep)), self.ctx)
        return keep.astype(bool)

    def bd_step(self, branch, change, leaf, birth, u_acc):
        """change[T, W] in {-1, 0, +1}, leaf[T, W] slot, birth[T, W, ndim of the branch] (rows of walkers that give birth), u_acc[T, W]."""
        ch = np.ascontiguousarray(change, dtype=np.int8)
        lf = np.ascontiguousarray(np.where(np.asarray(change) == 0, 0, leaf), dtype=np.int32)
        bt = self._birth_rows(birth, self.branches[int(branch)].ndim)
        u = f64(u_acc, (self.T, self.W))
        if self.host_like is not None:
            return self._host_move(_lib.RJ_MOVE_BD, branch=int(branch), change=ch, leaf=lf, birth=bt, u_acc=u)
        keep = np.empty((self.T, self.W), dtype=np.uint8)
        check(self.lib.hens_rj_bd_step(self.ctx, int(branch), ptr(ch), ptr(lf), ptr(bt), ptr(u), ptr(keep)), self.ctx)
        return keep.astype(bool)

    def bd_all_step(self, change, leaf, birth, u_acc):
        """"together": one proposal over every branch - change / leaf [nbranches, T, W], birth [nbranches][T, W, ndim of the branch]
        (one array when every branch has the same width), u_acc [T, W]."""
        nb = len(self.branches)
        ch = np.ascontiguousarray(change, dtype=np.int8)
        lf = np.ascontiguousarray(np.where(np.asarray(change) == 0, 0, leaf), dtype=np.int32)
        bt = np.ascontiguousarray(np.stack([self._birth_rows(birth[bi], b.ndim) for bi, b in enumerate(self.branches)]))
        u = f64(u_acc, (self.T, self.W))
        if ch.shape != (nb, self.T, self.W) or lf.shape != ch.shape:
            raise ValueError("change / leaf must have shape (nbranches, ntemps, nwalkers)")
        if self.host_like is not None:
            return self._host_move(_lib.RJ_MOVE_BD_ALL, change=ch, leaf=lf, birth=bt, u_acc=u)
        keep = np.empty((self.T, self.W), dtype=np.uint8)
        check(self.lib.hens_rj_bd_all_step(self.ctx, ptr(ch), ptr(lf), ptr(bt), ptr(u), ptr(keep)), self.ctx)
        return keep.astype(bool)

    # -- the multiple-try birth / death move (include/hipensemble.h: hens_rj_set_mt_proposal, hens_rj_mt_bd_step) ------------------
    def set_mt_proposal(self, num_try, generate_dist=None):
        """``MTDistGenMoveRJ(generate_dist, num_try=K, rj=True)`` in place of the plain birth / death move: ``num_try`` tries per
        walker (1 .. 64; 0 returns to the plain move) from ``generate_dist`` - ``{branch name: anything eryn_amd.prior.prior_spec
        reads}`` (a ProbDistContainer, the dict it is made of, (lo, hi) per leaf parameter) for EVERY branch, or None: the prior."""
        specs = None          # (mt_K / mt_gen follow the context: a refused call leaves both as they were)
        if generate_dist is None or int(num_try) == 0:
            check(self.lib.hens_rj_set_mt_proposal(self.ctx, int(num_try), None, None, None, None, None, None), self.ctx)
        else:
            specs = []
            for b in self.branches:
                if b.name not in generate_dist:
                    raise ValueError(f"generate_dist has no entry for branch {b.name}")
                specs.append(prior_spec(generate_dist[b.name]))
                if specs[-1].lo.shape != (b.ndim,):
                    raise ValueError(f"branch {b.name}: a generator of {specs[-1].lo.shape[0]} parameters for leaves of {b.ndim}")
            check(self.lib.hens_rj_set_mt_proposal(self.ctx, int(num_try), *map(ptr, term_arrays([s.terms for s in specs]))), self.ctx)
        self.mt_K, self.mt_gen = int(num_try), specs

    def mt_bd_step(self, branch, change, leaf, tries, u_pick, u_acc, out=False):
        """The move teacher-forced on one branch: change[T, W] in {-1, +1}, leaf[T, W], tries[T, W, K, ndim of the branch] (a death
        walker's try 0 is ignored: it is the dying leaf), u_pick / u_acc[T, W].  Returns the accept mask, with ``out=True`` also a dict
        of pick (int32), lsw, aux_lsw, factors, mt_ll, mt_lp, each [T, W]."""
        if self.host_like is not None:
            raise NotImplementedError("the multiple-try birth / death move evaluates its tries on the device: a TemplateLikelihood")
        K, nd = int(getattr(self, "mt_K", 0)), self.branches[int(branch)].ndim
        ch = np.ascontiguousarray(change, dtype=np.int8)
        lf = np.ascontiguousarray(leaf, dtype=np.int32)
        tr = np.zeros((self.T, self.W, max(K, 1), self.ndmax))
        tr[..., :nd] = f64(tries, (self.T, self.W, max(K, 1), nd))
        up, ua = f64(u_pick, (self.T, self.W)), f64(u_acc, (self.T, self.W))
        if ch.shape != (self.T, self.W) or lf.shape != ch.shape:
            raise ValueError("change / leaf must have shape (ntemps, nwalkers)")
        keep = np.empty((self.T, self.W), dtype=np.uint8)
        res = dict(pick=np.empty((self.T, self.W), dtype=np.int32), **{k: np.empty((self.T, self.W)) for k in ("lsw", "aux_lsw", "factors", "mt_ll", "mt_lp")})
        o = _lib.HensRjMtOut(**{k: v.ctypes.data for k, v in res.items()})
        self.eng.state_epoch += 1
        check(self.lib.hens_rj_mt_bd_step(self.ctx, int(branch), ptr(ch), ptr(lf), ptr(tr), ptr(up), ptr(ua), ptr(keep), C.byref(o) if out else None), self.ctx)
        return (keep.astype(bool), res) if out else keep.astype(bool)

    def mt_debug_draws(self, it):
        """The tries and pick uniforms ``step`` draws in iteration ``it`` (include/hipensemble.h: hens_rj_mt_debug_draws): tries
        [ns, T, W, K, ndmax], u_pick [ns, T, W] with the branch axis of ``debug_draws`` (one entry, or one per branch in order)."""
        nb, K = len(self.branches), int(getattr(self, "mt_K", 0))
        tries, up = np.zeros((nb, self.T, self.W, max(K, 1), self.ndmax)), np.zeros((nb, self.T, self.W))
        check(self.lib.hens_rj_mt_debug_draws(self.ctx, int(it), ptr(tries), ptr(up)), self.ctx)
        ns = nb if self.schedule in ("iterate_branches", "together") else 1
        return dict(tries=tries[:ns], u_pick=up[:ns])

    def _birth_rows(self, birth, nd):
        """[T, W, nd] -> [T, W, ndmax] (the library's stride: the model's widest branch)."""
        b = f64(birth, (self.T, self.W, nd))
        if nd == self.ndmax:
            return b
        out = np.zeros((self.T, self.W, self.ndmax))
        out[:, :, :nd] = b
        return out

    def stretch_split(self, split, labels, rint, u_zz, u_acc):
        """One half of the red / blue StretchMove over every branch and leaf slot (stretch.py:160-231, red_blue.py:148-323):
        labels[T, W] in {0, 1}, rint[nbranches, T, Ns] (one complement draw per branch), u_zz / u_acc[T, Ns]; returns the accept
        mask [T, Ns] of the moving walkers in ascending order."""
        lab = np.ascontiguousarray(labels, dtype=np.uint8)
        ri = np.ascontiguousarray(rint, dtype=np.int64)
        Ns = ri.shape[-1]
        if lab.shape != (self.T, self.W) or ri.shape != (len(self.branches), self.T, Ns):
            raise ValueError("labels must have shape (ntemps, nwalkers), rint (nbranches, ntemps, Ns)")
        uz, ua = f64(u_zz, (self.T, Ns)), f64(u_acc, (self.T, Ns))
        if self.host_like is not None:
            kw = self._host_move(_lib.RJ_MOVE_STRETCH, split=int(split), labels=lab, rint=ri, u_zz=uz, u_acc=ua)     # by walker
            return np.stack([kw[t][lab[t] == split] for t in range(self.T)])
        keep = np.empty((self.T, Ns), dtype=np.uint8)
        check(self.lib.hens_rj_stretch_split(self.ctx, int(split), ptr(lab), ptr(ri), ptr(uz), ptr(ua), ptr(keep)), self.ctx)
        return keep.astype(bool)

    def pt_sweep(self, iperm, i1perm, u_swap, adapt=True):
        return self.eng.pt_sweep(iperm, i1perm, u_swap, adapt=adapt)

    # -- production -------------------------------------------------------------------------------------------------
    def set_mh_scale(self, scale):
        """Standard deviations of the in-model Gaussian step per branch and leaf parameter: [nbranches, 3] (pulse / sine models), or one
        row per branch, as long as its leaves have parameters (the library's rows are as long as the widest branch's)."""
        s = np.zeros((len(self.branches), self.ndmax))
        if len(scale) != len(self.branches):
            raise ValueError(f"expected {len(self.branches)} rows of step scales")
        for bi, b in enumerate(self.branches):
            row = f64(scale[bi])
            if row.ndim != 1 or row.shape[0] < b.ndim or np.any(row[b.ndim:] != 0.0):
                raise ValueError(f"branch {b.name}: {b.ndim} step scales")
            s[bi, :b.ndim] = row[:b.ndim]
        check(self.lib.hens_rj_set_mh_scale(self.ctx, ptr(s)), self.ctx)

    def set_mh_chol(self, chol):
        """Lower-triangular Cholesky factors of the leaves' proposal covariances, [nbranches, 3, 3]: the in-model Gaussian step of
        ``step`` becomes ``L @ z`` per leaf (include/hipensemble.h: hens_rj_set_mh_chol).  Not positive definite -> ValueError; a model
        with a leaf kind beyond pulse / sine -> NotImplementedError."""
        if self.wide:
            raise NotImplementedError("full leaf covariances: models of pulses and sines only (diagonal steps: set_mh_scale)")
        if self.prior_terms:
            raise NotImplementedError("full leaf covariances: not with log-uniform / normal leaf priors (diagonal steps: set_mh_scale)")
        L = f64(chol, (len(self.branches), 3, 3))
        check(self.lib.hens_rj_set_mh_chol(self.ctx, ptr(L)), self.ctx)

    def set_periodic(self, periods):
        """Periodic leaf parameters (include/hipensemble.h: hens_rj_set_periodic).  ``periods``: None (clears), a
        ``{branch: {index: period}}`` dict, a ``PeriodicContainer`` (this package's or the reference's), or per branch in order a row
        of periods (0 = not periodic).  Every in-model move then measures differences the short way round and wraps what it proposes;
        a branch that is absent, None or ``{}`` has no periodic parameter."""
        rows = leaf_periods(periods, self.branches)
        if rows is None:
            check(self.lib.hens_rj_set_periodic(self.ctx, None), self.ctx)
            self.periods = None
            return
        p = np.zeros((len(self.branches), self.ndmax))
        for bi, b in enumerate(self.branches):
            p[bi, :b.ndim] = rows[bi]
        check(self.lib.hens_rj_set_periodic(self.ctx, ptr(p)), self.ctx)
        self.periods = rows

    def set_in_model(self, kind):
        """The in-model move of ``step``: "gaussian" (``set_mh_scale`` / ``set_mh_chol``) or "stretch" (the red / blue stretch move
        with the engine's ``a`` and ``live_dangerously``; include/hipensemble.h: hens_rj_set_in_model)."""
        code = {"gaussian": _lib.RJ_INMODEL_GAUSSIAN, "stretch": _lib.RJ_INMODEL_STRETCH, "group": _lib.RJ_INMODEL_GROUP}.get(kind)
        if code is None:
            raise ValueError("in-model move must be 'gaussian', 'stretch' or 'group' (the last behind set_group)")
        check(self.lib.hens_rj_set_in_model(self.ctx, code), self.ctx)
        self.in_model = kind

    # -- Gibbs blocks of the in-model Gaussian move (include/hipensemble.h: hens_rj_set_gibbs) -----------------------------------
    def set_gibbs(self, blocks):
        """``blocks``: bool / uint8 ``[nblocks, ncoord]`` in record layout (``leaf_gibbs_table``), or None / an empty list: no table."""
        if blocks is None or len(blocks) == 0:
            check(self.lib.hens_rj_set_gibbs(self.ctx, 0, None), self.ctx)
            self.gibbs_nblocks = 0
            return
        m = np.ascontiguousarray(np.asarray(blocks) != 0, dtype=np.uint8)
        if m.ndim != 2 or m.shape[1] != self.ncoord:
            raise ValueError(f"a Gibbs block table must have shape (nblocks, {self.ncoord})")
        check(self.lib.hens_rj_set_gibbs(self.ctx, int(m.shape[0]), ptr(m)), self.ctx)
        self.gibbs_nblocks = int(m.shape[0])

    def gibbs_select(self, block):
        """The block the next ``mh_step`` belongs to."""
        check(self.lib.hens_rj_gibbs_select(self.ctx, int(block)), self.ctx)

    def gibbs_debug_draws(self, it, block):
        """Block ``block``'s in-model draws of iteration ``it`` under ``step``: ``step [T, W, ncoord]`` (record layout) and ``u_mh [T, W]``."""
        out = dict(step=np.empty((self.T, self.W, self.ncoord)), u_mh=np.empty((self.T, self.W)))
        check(self.lib.hens_rj_gibbs_debug_draws(self.ctx, int(it), int(block), ptr(out["step"]), ptr(out["u_mh"])), self.ctx)
        return out

    # -- the group stretch move with a stationary friend table (include/hipensemble.h: hens_rj_set_group) ----------------------------
    def set_group(self, nfriends, n_iter_update, key, a=2.0):
        """``key``: the key parameter of every branch - one int, a list in branch order or ``{branch name: int}``.  ``nfriends == 0``
        (or None) clears the group.  The rebuild count restarts."""
        if not nfriends:
            check(self.lib.hens_rj_set_group(self.ctx, 0, 0, None, 2.0), self.ctx)
            self.group, self.group_m = None, 0
            if self.in_model == "group":
                self.in_model = "gaussian"
            return
        if isinstance(key, dict):
            missing = [b.name for b in self.branches if b.name not in key]
            if missing:
                raise ValueError(f"key has no entry for branch {missing[0]}")
            key = [key[b.name] for b in self.branches]
        keys = np.ascontiguousarray(np.broadcast_to(np.asarray(key, dtype=np.int32), (len(self.branches),)))
        check(self.lib.hens_rj_set_group(self.ctx, int(nfriends), int(n_iter_update), ptr(keys), float(a)), self.ctx)
        self.group, self.group_m = (int(nfriends), int(n_iter_update), keys.copy(), float(a)), 0

    def group_rebuild(self):
        """The friend table from the cold rung as it stands, and every active leaf's window from its position now."""
        self.eng.state_epoch += 1
        check(self.lib.hens_rj_group_rebuild(self.ctx), self.ctx)

    def picks_to_records(self, picks):
        """{name: pick[T, W, nl]} -> int32 [T, W, nslots], branch after branch."""
        if not isinstance(picks, dict):
            p = np.ascontiguousarray(picks, dtype=np.int32)
        else:
            p = np.ascontiguousarray(np.concatenate([np.asarray(picks[b.name]).reshape(self.T, self.W, b.nleaves_max) for b in self.branches], axis=-1), dtype=np.int32)
        if p.shape != (self.T, self.W, self.nslots):
            raise ValueError(f"picks must have shape {(self.T, self.W, self.nslots)}")
        return p

    def records_to_slots(self, arr):
        """[..., nslots] -> {name: [..., nl]}."""
        out, s0 = {}, 0
        for b in self.branches:
            out[b.name] = arr[..., s0:s0 + b.nleaves_max].copy()
            s0 += b.nleaves_max
        return out

    def group_step(self, picks, u_zz, u_acc):
        """The move teacher-forced: picks {name: [T, W, nl]} (read on active leaves: an entry of the leaf's window), u_zz / u_acc
        [T, W].  Newborn leaves get their windows first; nothing is rebuilt (``group_rebuild``).  Returns the accept mask."""
        p = self.picks_to_records(picks)
        uz, ua = f64(u_zz, (self.T, self.W)), f64(u_acc, (self.T, self.W))
        keep = np.empty((self.T, self.W), dtype=np.uint8)
        self.eng.state_epoch += 1
        check(self.lib.hens_rj_group_step(self.ctx, ptr(p), ptr(uz), ptr(ua), ptr(keep)), self.ctx)
        self.group_m += 1
        return keep.astype(bool)

    def group_debug(self):
        """The table and the windows as they stand: ``counts`` int [nbranches]; ``keys`` {name: [n_b]}; ``tab`` {name: [n_b, ndim]};
        ``start`` {name: int [T, W, nl]} (-1: no window assigned)."""
        nb = len(self.branches)
        counts = np.zeros(nb, dtype=np.int32)
        keys, tab = np.zeros(self.W * self.nslots), np.zeros((self.W * self.nslots, 4))
        start = np.zeros((self.T, self.W, self.nslots), dtype=np.int32)
        check(self.lib.hens_rj_group_debug(self.ctx, ptr(counts), ptr(keys), ptr(tab), ptr(start)), self.ctx)
        out, off = dict(counts=counts, keys={}, tab={}, start=self.records_to_slots(start)), 0
        for bi, b in enumerate(self.branches):
            out["keys"][b.name] = keys[off:off + counts[bi]].copy()
            out["tab"][b.name] = tab[off:off + counts[bi], :b.ndim].copy()
            off += self.W * b.nleaves_max
        return out

    def group_debug_draws(self, it):
        """What ``step`` draws for the group move in iteration ``it``, in ``group_step``'s form: picks {name: [T, W, nl]} (against the
        table as it stands), u_zz, u_acc [T, W]."""
        pick = np.zeros((self.T, self.W, self.nslots), dtype=np.int32)
        u_zz, u_acc = np.empty((self.T, self.W)), np.empty((self.T, self.W))
        check(self.lib.hens_rj_group_debug_draws(self.ctx, int(it), ptr(pick), ptr(u_zz), ptr(u_acc)), self.ctx)
        return dict(picks=self.records_to_slots(pick), u_zz=u_zz, u_acc=u_acc)

    def step(self, n_iters):
        check(self.lib.hens_rj_step(self.ctx, int(n_iters)), self.ctx)

    # -- chain store (include/hipensemble.h: hens_rj_chain_*, hens_rj_step_chain; chain_create / _reset / _destroy / _info: ChainStoreCalls) --
    def step_chain(self, n_store, iters_per_store=1):
        """``n_store`` stored steps of ``iters_per_store`` iterations each, appended to the chain on the device - per stored step
        what ``step(iters_per_store)`` + ``download(nan_fill=True)`` gives, bit for bit.  Nothing is copied to the host."""
        self.eng.state_epoch += 1
        check(self.lib.hens_rj_step_chain(self.ctx, int(n_store), int(iters_per_store)), self.ctx)

    CHAIN_FIELDS = ("x", "inds", "log_like", "log_prior", "betas")

    def chain_download(self, first=0, count=None, fields=CHAIN_FIELDS):
        """Stored steps ``[first, first + count)`` (count None: to the end) as a dict: ``x`` / ``inds`` ``{name: [count,
        ntemps_store, W, nl, nd] / bool [count, ntemps_store, W, nl]}`` (NaN on unused leaves), ``log_like`` / ``log_prior``
        ``[count, ntemps_store, W]``, ``betas[count, T]`` - those named in ``fields`` - and ``iteration`` / ``adapt_time``
        ``[count]``, the Philox checkpoint of every stored step.  One plain copy per array: nothing is reshaped on the host."""
        info = self.chain_info()
        first = int(first)
        count = info["count"] - first if count is None else int(count)
        Ts, n = info["ntemps_store"], max(count, 0)
        out = dict(iteration=np.zeros(n, dtype=np.int64), adapt_time=np.zeros(n, dtype=np.int64))
        shapes = dict(log_like=(n, Ts, self.W), log_prior=(n, Ts, self.W), betas=(n, self.T))
        for f in fields:
            if f in shapes:
                out[f] = np.empty(shapes[f])
        shared = [ptr(out.get("log_like")), ptr(out.get("log_prior")), ptr(out.get("betas")), ptr(out["iteration"]), ptr(out["adapt_time"])]
        if "x" not in fields and "inds" not in fields:
            check(self.lib.hens_rj_chain_download(self.ctx, first, count, -1, None, None, *shared), self.ctx)
            return out
        x, inds = {}, {}
        for bi, b in enumerate(self.branches):
            xb = np.empty((n, Ts, self.W, b.nleaves_max, b.ndim)) if "x" in fields else None
            ib = np.empty((n, Ts, self.W, b.nleaves_max), dtype=np.bool_) if "inds" in fields else None      # (bytes 0 / 1)
            check(self.lib.hens_rj_chain_download(self.ctx, first, count, bi, ptr(xb), ptr(ib), *(shared if bi == 0 else [None] * 5)), self.ctx)
            x[b.name], inds[b.name] = xb, ib
        if "x" in fields:
            out["x"] = x
        if "inds" in fields:
            out["inds"] = inds
        return out

    def chain_totals(self):
        """(accepted[ntemps_store, W], rj_accepted[ntemps_store, W], swaps_accepted[T - 1]) summed over the steps stored since
        the last reset: in-model accepts, birth / death accepts and in-model swaps of every stored step's last iteration."""
        Ts = self.chain_info()["ntemps_store"]
        acc, bd = np.zeros((Ts, self.W)), np.zeros((Ts, self.W))
        swaps = np.zeros(max(self.T - 1, 0))
        check(self.lib.hens_rj_chain_totals(self.ctx, ptr(acc), ptr(bd), ptr(swaps) if self.T > 1 else None), self.ctx)
        return acc, bd, swaps

    # -- chain diagnostics (include/hipensemble.h: hens_rj_chain_leaves, hens_rj_chain_leaf_moments, hens_rj_chain_moments) ----------
    def _branch_index(self, branch):
        names = [b.name for b in self.branches]
        return names.index(branch) if branch in names else int(branch)

    def _stat_rungs(self, ntemps):
        return int(self.chain_info()["ntemps_store"] if ntemps is None else ntemps)

    def chain_leaves(self, branch, first, count, thin=1, ntemps=None, nleaves=True):
        """``(nleaves, hist)`` of branch ``branch`` (name or index) over the kept steps ``first + j thin``, j < count, of the open
        chain: leaves in use ``uint8 [count, ntemps, W]`` (None with ``nleaves=False``: nothing the size of the range is copied) and
        ``hist uint32 [ntemps, W, nl + 1]``, at how many kept steps a walker has k leaves in use: eryn_amd.chain_stats.leaf_counts,
        computed where the chain is."""
        bi, nt = self._branch_index(branch), self._stat_rungs(ntemps)
        nl = self.branches[bi].nleaves_max if 0 <= bi < len(self.branches) else 0
        nle = np.empty((max(int(count), 0), max(nt, 0), self.W), dtype=np.uint8) if nleaves else None
        hist = np.empty((max(nt, 0), self.W, nl + 1), dtype=np.uint32)
        check(self.lib.hens_rj_chain_leaves(self.ctx, bi, int(first), int(count), int(thin), nt, ptr(nle), ptr(hist)), self.ctx)
        return nle, hist

    def chain_leaf_moments(self, branch, first, count, thin, ntemps, lo, hi):
        """``(sum, m2, n)`` - ``[ntemps, W, nd]``, ``[ntemps, W, nd]``, ``int64 [ntemps, W]`` - of every (rung, walker, parameter)'s
        series of the leaves in use in ascending (kept step, slot) whose ordinal lies in ``[lo, hi)``:
        eryn_amd.chain_stats.leaf_moments bit for bit."""
        bi, nt = self._branch_index(branch), self._stat_rungs(ntemps)
        nd = self.branches[bi].ndim if 0 <= bi < len(self.branches) else 1
        s, m2, n = np.empty((max(nt, 0), self.W, nd)), np.empty((max(nt, 0), self.W, nd)), np.empty((max(nt, 0), self.W), dtype=np.int64)
        check(self.lib.hens_rj_chain_leaf_moments(self.ctx, bi, int(first), int(count), int(thin), nt, int(lo), int(hi), ptr(s), ptr(m2), ptr(n)), self.ctx)
        return s, m2, n

    def chain_moments(self, field, first, count, thin=1, ntemps=None):
        """``(sum, m2, n_finite)`` per series of ``field`` - a branch's name: its coordinates as stored, ``[ntemps, W, nl, nd]``, NaN
        of an unused leaf propagating; "log_like" / "log_prior": ``[ntemps, W]``, non-finite entries skipped - over the kept steps:
        eryn_amd.chain_stats.moments bit for bit."""
        nt = self._stat_rungs(ntemps)
        if field in ("log_like", "log_prior"):
            code, bi, shape = (1 if field == "log_like" else 2), 0, (max(nt, 0), self.W)
        else:
            code, bi = 0, self._branch_index(field)
            b = self.branches[bi] if 0 <= bi < len(self.branches) else None
            shape = (max(nt, 0), self.W) + ((b.nleaves_max, b.ndim) if b else (1, 1))
        s, m2, nf = np.empty(shape), np.empty(shape), np.empty(shape, dtype=np.int64)
        check(self.lib.hens_rj_chain_moments(self.ctx, code, bi, int(first), int(count), int(thin), nt, ptr(s), ptr(m2), ptr(nf)), self.ctx)
        return s, m2, nf

    def chain_stats_ms(self):
        """Durations (ms) of the last k_rj_chain_leaves launch and of the last moments launch (k_rj_chain_leaf_moments or
        k_chain_moments), -1 where there was none."""
        a, b = C.c_double(-1.0), C.c_double(-1.0)
        check(self.lib.hens_rj_chain_stats_ms(self.ctx, C.byref(a), C.byref(b)), self.ctx)
        return dict(leaves_ms=a.value, moments_ms=b.value)

    def set_schedule(self, rj_moves):
        """The sampler's ``rj_moves`` string for ``step`` (ensemble.py:434-480): "separate_branches" | "iterate_branches" |
        "together", or "none": no reversible-jump move (``EnsembleSampler`` without ``rj_moves``)."""
        code = {"separate_branches": 0, "iterate_branches": 1, "together": 2, "none": 3}.get(rj_moves)
        if code is None:
            raise ValueError("rj_moves must be 'together', 'iterate_branches', 'separate_branches' or 'none'")
        check(self.lib.hens_rj_set_schedule(self.ctx, code), self.ctx)
        self.schedule = rj_moves

    def debug_draws(self, it):
        """Everything ``step`` draws in iteration ``it`` (include/hipensemble.h: hens_rj_debug_draws).  The birth / death
        arrays carry a leading branch axis: one entry ("separate_branches": the chosen branch) or one per branch in order."""
        T, W = self.T, self.W
        ns = len(self.branches)
        out = dict(step=np.empty((T, W, self.ncoord)), u_mh=np.empty((T, W)), coin=np.empty((ns, T, W), dtype=np.int8),
                   sel=np.empty((ns, T, W), dtype=np.uint32), birth=np.empty((ns, T, W, self.ndmax)), u_bd=np.empty((ns, T, W)),
                   slot_mh=np.empty((T, W), dtype=np.int32), uswap_mh=np.empty((max(T - 1, 1), W)),
                   slot_bd=np.empty((T, W), dtype=np.int32), uswap_bd=np.empty((max(T - 1, 1), W)))
        br = C.c_int32(0)
        check(self.lib.hens_rj_debug_draws(self.ctx, int(it), ptr(out["step"]), ptr(out["u_mh"]), C.byref(br), ptr(out["coin"]),
                                           ptr(out["sel"]), ptr(out["birth"]), ptr(out["u_bd"]), ptr(out["slot_mh"]),
                                           ptr(out["uswap_mh"]), ptr(out["slot_bd"]), ptr(out["uswap_bd"])), self.ctx)
        out["branch"] = int(br.value)
        if out["branch"] >= 0:                          # one move on the chosen branch
            for k in ("coin", "sel", "birth", "u_bd"):
                out[k] = out[k][:1]
        return out

    def debug_draws_stretch(self, it):
        """The stretch move's draws of iteration ``it`` in the form ``stretch_split`` takes (include/hipensemble.h:
        hens_rj_debug_draws_stretch): labels [T, W]; per half h (list index) rint [nbranches, T, Ns_h], u_zz / u_acc [T, Ns_h],
        movers in ascending walker order, Ns_0 = ceil(W / 2), Ns_1 = W - Ns_0."""
        T, W, nb = self.T, self.W, len(self.branches)
        n0 = (W + 1) // 2
        labels = np.empty((T, W), dtype=np.uint8)
        rint = np.empty((2, nb, T, n0), dtype=np.int64)
        u_zz, u_acc = np.empty((2, T, n0)), np.empty((2, T, n0))
        check(self.lib.hens_rj_debug_draws_stretch(self.ctx, int(it), ptr(labels), ptr(rint), ptr(u_zz), ptr(u_acc)), self.ctx)
        ns = (n0, W - n0)
        return dict(labels=labels, rint=[rint[h][:, :, :ns[h]].copy() for h in range(2)],
                    u_zz=[u_zz[h][:, :ns[h]].copy() for h in range(2)], u_acc=[u_acc[h][:, :ns[h]].copy() for h in range(2)])

    def debug_resident(self):
        """(x, inds, log_like) as they sit on the device, without the re-evaluation a download runs first
        (include/hipensemble.h: hens_rj_debug_resident): the log-likelihoods carry the +- leaf updates since the last refresh."""
        rec = np.empty((self.T, self.W, self.RW))
        L = np.empty((self.T, self.W))
        check(self.lib.hens_rj_debug_resident(self.ctx, ptr(rec), ptr(L)), self.ctx)
        x, inds = self.unpack(rec)
        return x, inds, L

    def set_iteration(self, it):
        self.eng.set_iteration(it)

    def iteration(self):
        return self.eng.iteration()

    def synchronize(self):
        self.eng.synchronize()

    def counters(self):
        c = self.eng.counters()
        bd = np.empty((self.T, self.W))
        n_mh, n_bd = C.c_int64(0), C.c_int64(0)
        check(self.lib.hens_rj_get_counters(self.ctx, ptr(bd), C.byref(n_mh), C.byref(n_bd)), self.ctx)
        c.update(accepted_mh=c["accepted"], accepted_bd=bd, num_mh=int(n_mh.value), num_bd=int(n_bd.value))
        return c


# ---------------------------------------------------------------------------------------------------------------------
# Sampler-level mirror: the reference's multi-branch ``EnsembleSampler`` contract for this path
# ---------------------------------------------------------------------------------------------------------------------
class TemplateLikelihood:
    """Stands where the reference takes ``log_like_fn`` + ``args=[t, y, sigma]`` (tests/test_eryn.py:79-92, 467-470):
    the template model lives inside the kernel.  ``kinds``: ``{branch_name: a name of LEAF_KINDS}``; a branch's ``ndims`` entry is the
    kind's width."""

    def __init__(self, kinds, t, y, sigma):
        self.kinds = {k: _KINDS[v] for k, v in kinds.items()}
        self.t, self.y, self.sigma = (None if t is None else f64(t)), (None if y is None else f64(y)), float(sigma)


def _no_leaf_gibbs(gibbs_sampling_setup):
    if gibbs_sampling_setup is not None:
        raise NotImplementedError("gibbs_sampling_setup over leaves and branches is not built for this move: it steps every leaf of "
                                  "every branch of a leaf-packing record in one move (the Gaussian move in blocks over branches and leaf "
                                  "slots: eryn_amd.rj.GibbsGaussianLeafMove; fixed-dimension Gibbs blocks: eryn_amd.EnsembleSampler with "
                                  "moves.StretchMove / GaussianMove)")


def leaf_periods(periodic, branches):
    """``periodic`` as ``EnsembleSampler`` takes it (ensemble.py:338-347) - None, ``{branch: {index: period}}``, a container with
    ``inds_periodic`` / ``periods`` - or a sequence of per-branch rows -> a list of ``[ndim]`` period rows in branch order (0 = not
    periodic), or None if no parameter is periodic.  Parsed by ``eryn_amd.periodic.period_vector`` per branch."""
    from .periodic import period_vector
    if periodic is None:
        return None
    if isinstance(periodic, (list, tuple, np.ndarray)):
        if len(periodic) != len(branches):
            raise ValueError(f"expected {len(branches)} rows of periods")
        rows = []
        for b, r in zip(branches, periodic):
            r = np.zeros(b.ndim) if r is None else np.asarray(r, dtype=np.float64)
            if r.shape != (b.ndim,):
                raise ValueError(f"branch {b.name}: {b.ndim} periods")
            if not np.all(np.isfinite(r) & (r >= 0.0)):
                raise ValueError("periods must be finite and >= 0")
            rows.append(r.copy())
    else:
        if isinstance(periodic, dict):
            unknown = [k for k in periodic if k not in [b.name for b in branches]]
            if unknown:
                raise ValueError(f"periodic names branch {unknown[0]!r}, which the sampler does not have")
        rows = []
        for b in branches:
            v = period_vector(periodic, b.name, b.ndim)
            rows.append(np.zeros(b.ndim) if v is None else v)
    return rows if any(np.any(r > 0.0) for r in rows) else None


def _same_periods(a, b):
    if a is None or b is None:
        return a is None and b is None
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


class GaussianLeafMove:
    """``GaussianMove(cov_all)`` of the reference on leaf-packing records (gaussian.py:9-66): ``cov_all[name]`` is the
    3 x 3 proposal covariance of a leaf of that branch (the reference's ``_proposal``: ``multivariate_normal``)."""

    def __init__(self, cov_all, gibbs_sampling_setup=None, periodic=None):
        _no_leaf_gibbs(gibbs_sampling_setup)
        self.periodic = periodic               # (the reference's moves carry one: it must agree with the sampler's, which it gets if None)
        self.cov = {k: np.atleast_2d(np.asarray(v, dtype=np.float64)) for k, v in cov_all.items()}
        for k, c in self.cov.items():
            if c.ndim != 2 or c.shape[0] != c.shape[1] or not 1 <= c.shape[0] <= 4:
                raise NotImplementedError("a leaf's proposal covariance must be an ndim x ndim matrix (ndim = 1 .. 4)")
        self.accepted, self.num_proposals = None, 0


_GIBBS_TYPES = "gibbs_sampling_setup must be string, dict, tuple, or list."                                 # move.py:125-128
_GIBBS_ITEM = "If providing a list for gibbs_sampling_setup, each item needs to be a string, tuple, or dict."       # move.py:174-177
_GIBBS_MASK = ("When inputing gibbs indexing and using a 2-tuple, second item must be None or 2D np.ndarray of shape "
               "(nleaves_max, ndim).")                                                                                # move.py:120


def parse_leaf_gibbs_setup(gibbs_sampling_setup):
    """``Move._initialize_branch_setup`` (move.py:113-221) for an in-model move: a branch name, ``(name, mask | None)``, ``{name: mask |
    None, ...}`` (several branches in ONE block), or a list of those -> the blocks in list order, each a list of ``(name, mask |
    None)`` in the block's own branch order (``branch_names_run_all`` / ``inds_run_all``).  A list inside the list, another type or a
    mask that is no 2-D array is refused with the reference's ``ValueError``; masks become bool arrays (their shape is the
    sampler's to check: it knows the branches)."""
    if type(gibbs_sampling_setup) not in (str, tuple, list, dict):
        raise ValueError(_GIBBS_TYPES)
    items = gibbs_sampling_setup if isinstance(gibbs_sampling_setup, list) else [gibbs_sampling_setup]

    def mask_of(v):
        if v is None:
            return None
        if not isinstance(v, np.ndarray) or v.ndim != 2:
            raise ValueError(_GIBBS_MASK)
        return v.astype(bool)

    blocks = []
    for item in items:
        if isinstance(item, str):
            blocks.append([(item, None)])
        elif isinstance(item, tuple):
            if len(item) != 2 or not isinstance(item[0], str):
                raise ValueError(_GIBBS_MASK)
            blocks.append([(item[0], mask_of(item[1]))])
        elif isinstance(item, dict):
            if not item or not all(isinstance(k, str) for k in item):
                raise ValueError(_GIBBS_ITEM)
            blocks.append([(k, mask_of(v)) for k, v in item.items()])
        else:
            raise ValueError(_GIBBS_ITEM)
    if not blocks:
        raise ValueError("gibbs_sampling_setup holds no block")
    return blocks


def leaf_gibbs_table(blocks, branches):
    """The blocks of ``parse_leaf_gibbs_setup`` on the sampler's branches -> ``(table, members)``: ``table`` bool ``[nblocks, ncoord]``
    in record layout (hens_rj_set_gibbs: branch after branch, slot after slot, the slot's parameters; a branch given by name or with
    None: every coordinate), ``members`` per block ``{name: bool [nleaves_max]}`` in the block's branch order, the slots with any true
    coordinate (``ir_keep``, move.py:278).  Refused with a sentence: a branch the sampler has not, a mask of another shape than
    ``(nleaves_max, ndim)``, a branch whose mask has no true entry (in the reference such a branch takes part in fix_logp_gibbs's count
    without ever moving; the table has no word for it), more than 128 blocks."""
    by = {b.name: (bi, b) for bi, b in enumerate(branches)}
    off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in branches])
    if len(blocks) > 128:
        raise ValueError(f"at most 128 Gibbs blocks ({len(blocks)})")
    table = np.zeros((len(blocks), int(off[-1])), dtype=bool)
    members = []
    for k, blk in enumerate(blocks):
        mem = {}
        for name, mask in blk:
            if name not in by:
                raise ValueError(f"gibbs_sampling_setup names branch {name!r}, which the sampler does not have")
            if name in mem:
                raise ValueError(f"gibbs_sampling_setup block {k} names branch {name!r} twice")
            bi, b = by[name]
            m = np.ones((b.nleaves_max, b.ndim), dtype=bool) if mask is None else np.asarray(mask, dtype=bool)
            if m.shape != (b.nleaves_max, b.ndim):
                raise ValueError(f"gibbs_sampling_setup: the mask of branch {name!r} must have shape {(b.nleaves_max, b.ndim)}, not {m.shape}")
            if not m.any():
                raise ValueError(f"gibbs_sampling_setup block {k}: the mask of branch {name!r} has no true entry")
            table[k, off[bi]:off[bi + 1]] = m.reshape(-1)
            mem[name] = m.any(axis=-1)
        members.append(mem)
    return table, members


class GibbsGaussianLeafMove(GaussianLeafMove):
    """``GaussianMove(cov_all, gibbs_sampling_setup=[...])`` of the reference as the in-model move on leaf-packing records (move.py:
    113-402 under mh.py:79-193): the Gaussian move block after block over branches and leaf slots.  ``gibbs_sampling_setup``: a
    branch name, ``(name, mask[nleaves_max, ndim] | None)``, ``{name: mask | None, ...}`` (several branches in one block) or a list
    of those (``parse_leaf_gibbs_setup``).  Per block the active leaves of its member slots move on their true coordinates; every
    other coordinate keeps its bits (include/hipensemble.h: hens_rj_set_gibbs).

    ``accepted`` / ``num_proposals`` follow the reference's per-block bookkeeping (mh.py:186-187): + the block's accept mask and + 1
    per block that ran.  Under ``rng="numpy"`` a block in which no walker of any rung has a leaf to move is skipped before any draw
    (mh.py:105-107); under ``rng="philox"`` the device walks every block - the walkers of such a block are all rejected - and
    ``num_proposals`` counts it."""

    def __init__(self, cov_all, gibbs_sampling_setup, periodic=None):
        if gibbs_sampling_setup is None:
            raise ValueError("GibbsGaussianLeafMove needs a gibbs_sampling_setup (without blocks the move is GaussianLeafMove)")
        super().__init__(cov_all, periodic=periodic)
        self.gibbs_sampling_setup = gibbs_sampling_setup
        self.blocks = parse_leaf_gibbs_setup(gibbs_sampling_setup)


class StretchLeafMove:
    """``StretchMove(a=2.0)`` of the reference as the in-model move on leaf-packing records (stretch.py:14-231 over
    red_blue.py:103-330): every branch and every leaf slot of a walker moves - one complement walker per branch, one stretch
    factor per walker.  (The reference advises against it beside reversible jump, ensemble.py:509-514, and runs it.)"""

    def __init__(self, a=2.0, live_dangerously=False, gibbs_sampling_setup=None, periodic=None):
        _no_leaf_gibbs(gibbs_sampling_setup)
        self.periodic = periodic
        self.a = float(a)
        self.live_dangerously = bool(live_dangerously)         # red_blue.py:41-47,108: fewer walkers than 2 x (all leaf slots' coordinates)
        self.accepted, self.num_proposals = None, 0


class GroupStretchLeafMove:
    """``GroupStretchMove(nfriends=..., n_iter_update=..., a=...)`` of the reference (moves/group.py:122-281, moves/groupstretch.py:
    34-120) as the in-model move on leaf-packing records, with ONE friend rule where the reference leaves the rule to a subclass:
    nearest friends by one key parameter.  Every active leaf is stretched toward a friend, a leaf near it (in ``key``) out of a
    stationary snapshot of the cold chain that is rebuilt every ``n_iter_update`` moves; one launch per iteration
    (include/hipensemble.h: hens_rj_set_group; csrc/hens_rj_group.h states the move).

    ``nfriends`` 1 .. 64; ``key`` an int (every branch) or ``{branch: int}``, the leaf parameter that measures nearness;
    ``n_iter_update`` >= 2, or >= 1 with ``live_dangerously`` (group.py:45-46).

    The friend table is state that a ``State`` does not carry: ``run_mcmc`` restarts the rebuild count, so its first move rebuilds the
    table from the state it was given, and a chain resumed from a stored ``State`` is the uninterrupted chain only if the resume
    falls on a rebuild (a multiple of ``n_iter_update`` moves).  Periodic parameters (the sampler's ``periodic=``): the stretch toward
    the friend goes the short way round and is wrapped; the friend RULE stays nearest by linear distance in ``key``, also where the
    key parameter is periodic.  Not built: Gibbs blocks for this move, host-callable likelihoods, more than 64 friends, user-defined
    friend rules."""

    def __init__(self, nfriends, key, n_iter_update=100, a=2.0, live_dangerously=False, gibbs_sampling_setup=None, periodic=None):
        self.periodic = periodic
        if gibbs_sampling_setup is not None:
            raise NotImplementedError("gibbs_sampling_setup is not built for GroupStretchLeafMove: it stretches every active leaf of every "
                                      "branch in one move")
        if isinstance(nfriends, bool) or not isinstance(nfriends, (int, np.integer)) or not 1 <= int(nfriends) <= 64:
            raise ValueError("nfriends must be an integer in [1, 64]")
        self.live_dangerously = bool(live_dangerously)
        if int(n_iter_update) <= 1 and not (self.live_dangerously and int(n_iter_update) == 1):
            raise ValueError("n_iter_update must be greather than or equal to 2.")             # group.py:45-46
        if isinstance(key, dict):
            if not key or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= 0 for v in key.values()):
                raise ValueError("key must be a non-negative int or {branch name: non-negative int}")
            self.key = {str(k): int(v) for k, v in key.items()}
        elif isinstance(key, (int, np.integer)) and not isinstance(key, bool) and key >= 0:
            self.key = int(key)
        else:
            raise ValueError("key must be a non-negative int or {branch name: non-negative int}")
        if not float(a) > 1.0 or not np.isfinite(a):
            raise ValueError("the stretch scale a must be finite and > 1")
        self.nfriends, self.n_iter_update, self.a = int(nfriends), int(n_iter_update), float(a)
        self.accepted, self.num_proposals = None, 0


class MTDistGenMoveRJ:
    """``MTDistGenMoveRJ(generate_dist, num_try=25, rj=True)`` of the reference (mtdistgenrj.py over multipletry.py:238-514, 597-776)
    as the between-model move of ``RJEnsembleSampler(rj_moves=...)``: per walker ``num_try`` (1 .. 64) candidate leaves from
    ``generate_dist`` - ``{branch name: ProbDistContainer | the dict it is made of | (lo, hi) per leaf parameter}``, uniform,
    log-uniform and normal entries - one of them picked by importance weight (include/hipensemble.h: hens_rj_set_mt_proposal).  The
    move acts on one branch (multipletry.py:635-636): one object on a one-branch model, or a list with one object per branch, each
    with ``gibbs_sampling_setup=<its branch>`` and the same ``num_try``.  ``nleaves_max`` / ``nleaves_min`` are the sampler's: given here
    (a dict over branches or one number) they must agree with it for the move's branch, else the sampler raises ``ValueError``.

    ``accepted`` / ``num_proposals`` (move.py:404-421) are fed per move under ``rng="numpy"``.  Under ``rng="philox"`` the device counts
    the birth / death move over all branches together (hens_rj_get_counters): the sampler's ``rj_accepted_all`` /
    ``rj_num_proposals_all`` carry it and the moves' own counters stay at zero."""

    def __init__(self, generate_dist, nleaves_max=None, nleaves_min=None, num_try=1, rj=True, gibbs_sampling_setup=None):
        if not rj:
            raise NotImplementedError("MTDistGenMoveRJ is the nested reversible-jump form of multiple try: rj=True")
        if isinstance(num_try, bool) or not isinstance(num_try, (int, np.integer)) or not 1 <= int(num_try) <= 64:
            raise ValueError("num_try must be an integer in [1, 64]")
        if not isinstance(generate_dist, dict) or not generate_dist:
            raise ValueError("generate_dist must be a dict {branch name: distribution container}")
        if gibbs_sampling_setup is not None and gibbs_sampling_setup not in generate_dist:
            raise ValueError(f"gibbs_sampling_setup must name the branch the move acts on (a key of generate_dist), not {gibbs_sampling_setup!r}")
        if gibbs_sampling_setup is None and len(generate_dist) != 1:
            raise ValueError("Can only propose change to one model at a time with MT. (one MTDistGenMoveRJ per branch, each with "
                             "gibbs_sampling_setup=<its branch>)")
        self.generate_dist, self.num_try = dict(generate_dist), int(num_try)
        self.branch = gibbs_sampling_setup if gibbs_sampling_setup is not None else next(iter(generate_dist))
        self.gibbs_sampling_setup = gibbs_sampling_setup
        self.nleaves_max, self.nleaves_min = nleaves_max, nleaves_min
        self.accepted, self.num_proposals = None, 0


def _mt_rj_moves(rj_moves, branch_names):
    """``rj_moves`` made of MTDistGenMoveRJ objects -> {branch name: move}, or None if it holds none.  One object on a one-branch model,
    or one per branch in a list; anything else is refused with a sentence."""
    seq = list(rj_moves) if isinstance(rj_moves, (list, tuple)) else [rj_moves]
    seq = [m[0] if isinstance(m, (list, tuple)) else m for m in seq]          # ((move, weight) pairs: the weights must be uniform)
    if not any(isinstance(m, MTDistGenMoveRJ) for m in seq):
        return None
    if not all(isinstance(m, MTDistGenMoveRJ) for m in seq):
        raise NotImplementedError("rj_moves: MTDistGenMoveRJ objects cannot be mixed with other moves")
    if isinstance(rj_moves, (list, tuple)) and any(isinstance(m, (list, tuple)) for m in rj_moves):
        w = [float(m[1]) for m in rj_moves]
        if any(x != w[0] for x in w):
            raise NotImplementedError("rj_moves: the device chooses the branch of a between-model move uniformly (equal weights)")
    by = {}
    for m in seq:
        if m.branch not in branch_names:
            raise ValueError(f"MTDistGenMoveRJ acts on branch {m.branch!r}, which the sampler does not have")
        if m.branch in by:
            raise ValueError(f"two MTDistGenMoveRJ moves act on branch {m.branch!r}")
        by[m.branch] = m
    if sorted(by) != sorted(branch_names):
        raise NotImplementedError("rj_moves: one MTDistGenMoveRJ per branch (every branch takes the multiple-try move, or none does)")
    if len({m.num_try for m in seq}) != 1:
        raise NotImplementedError("rj_moves: every MTDistGenMoveRJ must have the same num_try (one launch shape per context)")
    return by


class RJEnsembleSampler:
    """``EnsembleSampler(nwalkers, ndims, log_like_fn, priors, tempering_kwargs=..., branch_names=..., nleaves_max=...,
    nleaves_min=..., moves=GaussianMove(cov), rj_moves="separate_branches")`` (ensemble.py:211-681) for the template model,
    stepping on the MI355X.  One iteration = one in-model move + one RJ move of a uniformly chosen branch
    (ensemble.py:963-1024 with the default ``num_repeats_in_model = num_repeats_rj = 1``).

    rng="numpy":  the reference's streams (the sampler-owned RandomState cloned from the global ``np.random`` at
                  construction + the global stream) are drawn on the host IN THE REFERENCE'S ORDER and handed to the device:
                  same seeds => the reference's chain (tests/test_hip_rj.py against the rj* fixtures).
    rng="philox": device-side draws, ``thin_by`` iterations per host call (``hens_rj_step``), with every in-model move the class
                  accepts: ``GaussianLeafMove`` (diagonal or full leaf covariances), ``StretchLeafMove``, with or without
                  ``rj_moves``.  The device keeps every walker's
                  model resident and updates it by +- one leaf per accepted birth / death; the models and log-likelihoods are
                  re-evaluated from the coordinates every 64 iterations and whenever the state is downloaded (the evaluation
                  runs in front of the copy, so a stored ``State.log_like`` is exactly what the device continues with and a chain
                  resumed from it is the uninterrupted chain bit for bit).  Consequence: WHERE the re-evaluations fall depends
                  on ``store`` / ``thin_by``, so two runs that differ only in those agree to rounding (log-likelihoods to ~1e-13
                  relative), not bit for bit - as two reference runs with a different likelihood summation order would.

    priors: per branch a ``ProbDistContainer`` or the dict it is made of - ``uniform_dist``, ``log_uniform``, ``NormalDistribution`` or
    the frozen SciPy ``uniform`` / ``loguniform`` / ``norm`` per leaf parameter (prior.py:219-392).  The prior is also the birth
    proposal (distgenrj.py:188-214): log-prior, the factor -+ log q(leaf) and the born leaf's draw all follow it in both ``rng`` modes
    (include/hipensemble.h: hens_rj_set_prior_terms); with a log-uniform or normal parameter the Philox Gaussian move takes diagonal
    covariances only.

    periodic: ``{branch: {index: period}}``, this package's ``PeriodicContainer`` or the reference's (``EnsembleSampler(periodic=...)``):
    every in-model move - Gaussian, Gibbs blocks, stretch, group stretch - measures ``c - s`` the short way round and wraps its proposal
    with the reference's arithmetic, in both ``rng`` modes; birth / death draws from the prior and knows no periods, as in the
    reference."""

    def __init__(self, nwalkers, ndims, log_like_fn, priors, tempering_kwargs=None, nbranches=None, branch_names=None,
                 nleaves_max=None, nleaves_min=None, moves=None, rj_moves="separate_branches", rng="numpy", seed=None,
                 device_id=0, args=None, kwargs=None, vectorize=False, provide_groups=False, fill_zero_leaves_val=-1e300,
                 backend=None, periodic=None, **unused):
        from .backend import RJDeviceBackend
        from .moves.tempering import TemperatureControl
        for m in (moves if isinstance(moves, (list, tuple)) else [moves]):
            m = m[0] if isinstance(m, (list, tuple)) else m
            if not isinstance(m, GibbsGaussianLeafMove):
                _no_leaf_gibbs(getattr(m, "gibbs_sampling_setup", None))
        # backend: None - the stored steps are a list of States (``self.chain``) - or an eryn_amd.backend.RJDeviceBackend: they stay
        # in device memory until somebody reads them (one device call per chain segment, hens_rj_step_chain)
        if backend is not None and not isinstance(backend, RJDeviceBackend):
            raise NotImplementedError("backend: None (a list of States) or an eryn_amd.backend.RJDeviceBackend")
        if backend is not None and rng != "philox":
            raise NotImplementedError("RJDeviceBackend keeps the chain of the device-side draws: it needs rng='philox' (with rng='numpy' "
                                      "every move crosses the host)")
        if backend is not None and not isinstance(log_like_fn, TemplateLikelihood):
            raise NotImplementedError("RJDeviceBackend needs the likelihood on the device (a TemplateLikelihood): a Python function "
                                      "steps through the caller")
        # log_like_fn: a TemplateLikelihood (the model lives in the kernel) or - round 6 - any Python function of the packed active
        # leaves with the reference's own ``args`` / ``kwargs`` / ``vectorize`` / ``provide_groups`` (ensemble.py:211-330): the
        # device proposes, computes the prior, tests and updates, the host evaluates (CallableLikelihood)
        self.host_like = None
        if callable(log_like_fn) and not isinstance(log_like_fn, (TemplateLikelihood, CallableLikelihood)):
            log_like_fn = CallableLikelihood(log_like_fn, args, kwargs, vectorize, provide_groups, fill_zero_leaves_val)
        if isinstance(log_like_fn, CallableLikelihood):
            if rng != "numpy":
                raise NotImplementedError("a host-callable likelihood steps with rng='numpy' (rng='philox' needs the likelihood on the device)")
            if isinstance(moves, GibbsGaussianLeafMove):
                raise NotImplementedError("GibbsGaussianLeafMove updates the walkers' models leaf by leaf on the device: log_like_fn "
                                          "must be a TemplateLikelihood, not a Python function")
            if isinstance(moves, GroupStretchLeafMove):
                raise NotImplementedError("GroupStretchLeafMove evaluates its proposals on the device: log_like_fn must be a "
                                          "TemplateLikelihood, not a Python function")
            self.host_like = log_like_fn
            names_ = list(branch_names if branch_names is not None else ndims.keys())
            log_like_fn = TemplateLikelihood({k: "pulse" for k in names_}, None, None, 1.0)     # (never evaluated: no device likelihood)
        if not isinstance(log_like_fn, TemplateLikelihood):
            raise NotImplementedError("log_like_fn: an eryn_amd.rj.TemplateLikelihood, a CallableLikelihood or a Python function")
        # rj_moves made of MTDistGenMoveRJ objects: the multiple-try birth / death move on every branch, one of them chosen per
        # iteration like the plain moves of "separate_branches" (ensemble.py:453-471, 988-990)
        self.mt_moves = None if isinstance(rj_moves, str) or not rj_moves else _mt_rj_moves(rj_moves, list(branch_names if branch_names is not None else ndims.keys()))
        if self.mt_moves is not None:
            if self.host_like is not None:
                raise NotImplementedError("MTDistGenMoveRJ evaluates its tries on the device: log_like_fn must be a TemplateLikelihood")
            rj_moves = "separate_branches"
        if rj_moves is True:                                 # ensemble.py:413-415: True is "together"
            rj_moves = "together"
        if rj_moves not in ("separate_branches", "iterate_branches", "together", None, False):
            raise ValueError("When providing a str for rj_moves, must be 'together', 'iterate_branches', or "
                             f"'separate_branches'. Input is {rj_moves}")                # ensemble.py:473-476
        self.rj_schedule = rj_moves or None                  # None: no reversible jump - the leaf masks never change
        if not isinstance(moves, (GaussianLeafMove, StretchLeafMove, GroupStretchLeafMove)):
            raise NotImplementedError("the in-model move must be an eryn_amd.rj.GaussianLeafMove, StretchLeafMove or GroupStretchLeafMove")
        if rng not in ("numpy", "philox"):
            raise ValueError("rng must be 'numpy' or 'philox'")
        self.branch_names = list(branch_names if branch_names is not None else ndims.keys())
        if nbranches is not None and nbranches != len(self.branch_names):
            raise ValueError("nbranches does not match branch_names")
        nleaves_min = nleaves_min or {k: 0 for k in self.branch_names}            # ensemble.py:388-389
        self.nwalkers, self.ndims = int(nwalkers), dict(ndims)
        self.nleaves_max, self.nleaves_min = dict(nleaves_max), dict(nleaves_min)
        for k, m in (self.mt_moves or {}).items():          # (a move's own leaf budget, where it was given one, is the sampler's)
            for what, own, mine in (("nleaves_max", m.nleaves_max, self.nleaves_max), ("nleaves_min", m.nleaves_min, self.nleaves_min)):
                if own is not None and (dict(own).get(k, mine[k]) if isinstance(own, dict) else own) != mine[k]:
                    raise ValueError(f"MTDistGenMoveRJ on {k}: {what} differs from the sampler's")
        self.branches = []
        for k in self.branch_names:
            nd = int(self.ndims[k])
            if self.host_like is None and nd != _WIDTH[log_like_fn.kinds[k]]:
                raise NotImplementedError(f"branch {k}: a leaf of its kind has {_WIDTH[log_like_fn.kinds[k]]} parameters, ndims says {nd}")
            if isinstance(moves, GaussianLeafMove) and moves.cov[k].shape != (nd, nd):
                raise ValueError(f"branch {k}: the proposal covariance must be {nd} x {nd}")
            leaf_prior = prior_spec(priors[k])       # (a container, the dict it is made of, or (lo, hi) per leaf parameter)
            if leaf_prior.lo.shape != (nd,):
                raise ValueError(f"branch {k}: {leaf_prior.lo.shape[0]} prior {'boxes' if leaf_prior.is_box else 'distributions'} for ndims = {nd}")
            if self.host_like is not None:     # (no device likelihood: 1 .. 4 parameters per leaf, hens_rj_set_model_general)
                self.branches.append(LeafBranch(k, leaf_prior, self.nleaves_max[k], self.nleaves_min[k]))
            else:
                self.branches.append(TemplateBranch(k, log_like_fn.kinds[k], leaf_prior, self.nleaves_max[k], self.nleaves_min[k]))
        total_ndim = sum(self.nleaves_max[k] * self.ndims[k] for k in self.branch_names)     # ensemble.py:325-329
        tk = dict(tempering_kwargs or {})
        if not tk:
            raise NotImplementedError("the device RJ path is tempered (pass tempering_kwargs=dict(ntemps=...))")
        self.temperature_control = tc = TemperatureControl(total_ndim, self.nwalkers, **tk)
        self.ntemps = tc.ntemps
        self.moves, self.rng = [moves], rng
        # periodic: what EnsembleSampler takes (ensemble.py:338-347) - the in-model moves of both rng modes measure and wrap by it
        # (hens_rj_set_periodic); a move that carries its own must say the same
        self.periodic = periodic
        rows = leaf_periods(periodic, self.branches)
        if getattr(moves, "periodic", None) is not None and not _same_periods(leaf_periods(moves.periodic, self.branches), rows):
            raise ValueError("the move's periodic differs from the sampler's (one set of periods per sampler: pass it as "
                             "RJEnsembleSampler(periodic=...))")
        moves.periodic = periodic
        if seed is None:
            seed = int(np.random.randint(0, 2**31 - 1)) if rng == "philox" else 0
        self.engine = RJEngine(self.ntemps, self.nwalkers, self.branches, log_like_fn.t, log_like_fn.y, log_like_fn.sigma,
                               seed=seed, device_id=device_id, adaptive=tc.adaptive, adaptation_lag=tc.adaptation_lag,
                               adaptation_time=tc.adaptation_time, stop_adaptation=tc.stop_adaptation,
                               **({"a": moves.a, "live_dangerously": moves.live_dangerously} if isinstance(moves, (StretchLeafMove, GroupStretchLeafMove)) else {}))
        self.engine.host_like = self.host_like
        if rows is not None:
            self.engine.set_periodic(rows)
        self.gibbs_members = None
        if isinstance(moves, GibbsGaussianLeafMove):      # the table is pushed once; both rng modes step under it
            table, self.gibbs_members = leaf_gibbs_table(moves.blocks, self.branches)
            self.engine.set_gibbs(table)
        if isinstance(moves, GroupStretchLeafMove):       # the friend table's buffers are made once; both rng modes step under it
            if isinstance(moves.key, dict):
                for k in self.branch_names:
                    if k not in moves.key:
                        raise ValueError(f"GroupStretchLeafMove: key has no entry for branch {k}")
            for b in self.branches:
                kb = moves.key[b.name] if isinstance(moves.key, dict) else moves.key
                if kb >= b.ndim:
                    raise ValueError(f"GroupStretchLeafMove: key {kb} of branch {b.name}, whose leaves have parameters 0 .. {b.ndim - 1}")
            self.engine.set_group(moves.nfriends, moves.n_iter_update, moves.key, moves.a)
        if self.rj_schedule is not None or rng == "philox":
            self.engine.set_schedule(rj_moves or "none")
        if self.mt_moves is not None:
            for m in self.mt_moves.values():
                m.accepted = np.zeros((self.ntemps, self.nwalkers))
            self.engine.set_mt_proposal(next(iter(self.mt_moves.values())).num_try,
                                        {k: self.mt_moves[k].generate_dist[k] for k in self.branch_names})
        if rng == "philox" and isinstance(moves, StretchLeafMove):
            self.engine.set_in_model("stretch")
        elif rng == "philox" and isinstance(moves, GroupStretchLeafMove):
            self.engine.set_in_model("group")
        elif rng == "philox":
            # axis-aligned steps (hens_rj_set_mh_scale: three standard deviations per branch), or - a covariance with off-diagonal
            # terms - the Cholesky factor of every branch's leaf covariance (hens_rj_set_mh_chol: step = L z)
            if all(np.array_equal(moves.cov[k], np.diag(np.diag(moves.cov[k]))) for k in self.branch_names):
                self.engine.set_mh_scale([np.sqrt(np.diag(moves.cov[k])) for k in self.branch_names])
            elif self.engine.wide:
                raise NotImplementedError("rng='philox' with a leaf kind beyond pulse / sine: diagonal proposal covariances only")
            elif self.engine.prior_terms:
                raise NotImplementedError("rng='philox' with log-uniform / normal leaf priors: diagonal proposal covariances only")
            else:
                self.engine.set_mh_chol(np.stack([np.linalg.cholesky(moves.cov[k]) for k in self.branch_names]))
        moves.accepted = np.zeros((self.ntemps, self.nwalkers))
        nmoves = len(self.branch_names) if rj_moves == "separate_branches" else (1 if self.rj_schedule else 0)    # (rj move objects, ensemble.py:414-471)
        self.rj_accepted = [np.zeros((self.ntemps, self.nwalkers)) for _ in range(nmoves)]
        self.rj_num_proposals = [0 for _ in range(nmoves)]
        # rng="philox": the device counts the birth / death move over all branches together
        self.rj_accepted_all, self.rj_num_proposals_all = np.zeros((self.ntemps, self.nwalkers)), 0
        self._random = np.random.mtrand.RandomState()
        self._random.set_state(np.random.get_state())          # R := snapshot of the global stream (ensemble.py:604,651-652)
        self.iteration, self.chain = 0, []
        self._previous_state = None
        self.backend = backend
        if backend is not None:
            backend.attach(self.engine, seed)
            if not backend.initialized:
                backend.reset(self.nwalkers, self.ndims, ntemps=self.ntemps, branch_names=self.branch_names, nleaves_max=self.nleaves_max)

    # -- the reference's evaluation entry points, with inds (ensemble.py:1127-1217, 1219-1545) -----------------------
    def _eval(self, coords, inds):
        self.engine.upload(coords, inds, betas=self.temperature_control.betas)
        self.engine.eval_state()                 # (a host-callable likelihood is called from there)
        _, _, L, P, _ = self.engine.download()
        return L, P

    def compute_log_prior(self, coords, inds=None, **kw):
        return self._eval(coords, inds)[1]

    def compute_log_like(self, coords, inds=None, logp=None, **kw):
        return self._eval(coords, inds)[0], None

    # -- one iteration with the reference's draws ------------------------------------------------------------------------
    def _iteration_numpy(self):
        eng, tc, R, T, W = self.engine, self.temperature_control, self._random, self.ntemps, self.nwalkers
        mv = self.moves[0]
        R.choice(1, p=np.ones(1))                                               # move choice (ensemble.py:971)
        if isinstance(mv, StretchLeafMove):
            # red / blue stretch over every branch and leaf slot: the split's shuffles from the GLOBAL stream (red_blue.py:119-124),
            # per half and branch one randint of R, behind the first branch's the walkers' zz uniforms (stretch.py:205, 128-132),
            # then the accept uniforms (red_blue.py:294)
            labels = np.tile(np.arange(W), (T, 1)) % 2
            for row in labels:
                np.random.shuffle(row)
            acc = np.zeros((T, W), dtype=bool)
            for split in range(2):
                Ns = int((labels[0] == split).sum())
                rint, u_zz = [], None
                for bi in range(len(self.branches)):
                    rint.append(R.randint(W - Ns, size=(T, Ns)))
                    if bi == 0:
                        u_zz = R.rand(T, Ns)
                keep = eng.stretch_split(split, labels, np.stack(rint), u_zz, R.rand(T, Ns))
                for t in range(T):
                    acc[t, np.flatnonzero(labels[t] == split)] = keep[t]
        elif isinstance(mv, GroupStretchLeafMove):
            # the group stretch move (group.py:122-281): the table anew when due, from the state in front of the move; per branch in
            # order the friends' picks from the GLOBAL stream over the active leaves in ascending (rung, walker, slot) (skipped where
            # the branch's table is empty), behind branch 0 the walkers' zz uniforms from R (stretch.py:128-132), then the accept
            # uniforms (group.py:254)
            if eng.group_m % mv.n_iter_update == 0:
                eng.group_rebuild()
            _, inds, _, _, _ = eng.download()
            counts = eng.group_debug()["counts"]
            picks, u_zz = {}, None
            for bi, b in enumerate(self.branches):
                nf = min(mv.nfriends, int(counts[bi]))
                picks[b.name] = np.zeros(inds[b.name].shape, dtype=np.int32)
                if nf > 0:
                    picks[b.name][inds[b.name]] = np.random.randint(nf, size=int(inds[b.name].sum()))
                if bi == 0:
                    u_zz = R.rand(T, W)
            acc = eng.group_step(picks, u_zz, R.rand(T, W))
        elif self.gibbs_members is not None:
            # block after block (mh.py:79-187): per branch of the block, in the block's own order, one multivariate_normal over the
            # active leaves of its member slots in ascending (rung, walker, slot) (gaussian.py:96-108), then the accept uniforms
            # (mh.py:171); a block without any such leaf is skipped before it draws (mh.py:105-107).  The move's accept mask is
            # the last block's that ran (zeros if none did, mh.py:77)
            acc = np.zeros((T, W), dtype=bool)
            for k, mem in enumerate(self.gibbs_members):
                x, inds, _, _, _ = eng.download()
                going = {name: inds[name] & slots[None, None, :] for name, slots in mem.items()}
                if not any(g.any() for g in going.values()):
                    continue
                steps = {b.name: np.zeros(x[b.name].shape) for b in self.branches}
                for name, g in going.items():
                    nd = steps[name].shape[-1]
                    steps[name][g] = 1.0 * R.multivariate_normal(np.zeros(nd), mv.cov[name], size=int(g.sum()))
                eng.gibbs_select(k)
                acc = eng.mh_step(steps, R.rand(T, W))
                mv.accepted += acc
                mv.num_proposals += 1
        else:
            x, inds, _, _, _ = eng.download()
            # per branch one multivariate_normal over the packed leaves (gaussian.py:96-104, 265-268), the accept uniforms (mh.py:157)
            steps = {}
            for b in self.branches:
                n = int(inds[b.name].sum())
                s = np.zeros(x[b.name].shape)
                s[inds[b.name]] = 1.0 * R.multivariate_normal(np.zeros(b.ndim), mv.cov[b.name], size=n)
                steps[b.name] = s
            acc = eng.mh_step(steps, R.rand(T, W))
        if self.gibbs_members is None:
            mv.accepted += acc
            mv.num_proposals += 1
        iperm, i1perm, u = tc.draw_swap_randoms()                               # mh.py:190-191
        _, swaps = eng.pt_sweep(iperm, i1perm, u, adapt=bool(tc.adaptive))
        tc.swaps_accepted = swaps
        if tc.adaptive:
            tc.time += 1
        if self.rj_schedule is None:
            return acc, None
        # reversible jump (ensemble.py:988-990; distgenrj.py:35-222): on one branch chosen from R, or - "iterate_branches" - one
        # move (the choice among ONE move still draws) that takes the branches in turn, its accept mask the last branch's
        nb = len(self.branches)
        if self.rj_schedule == "together":
            R.choice(1, p=np.ones(1))
            racc = self._bd_numpy_all()
            self.rj_accepted[0] += racc
            self.rj_num_proposals[0] += 1
        elif self.rj_schedule == "iterate_branches":
            R.choice(1, p=np.ones(1))
            for bi in range(nb):
                racc = self._bd_numpy(bi)
            self.rj_accepted[0] += racc
            self.rj_num_proposals[0] += 1
        else:
            bi = int(R.choice(nb, p=np.full(nb, 1.0 / nb)))
            racc = self._bd_numpy(bi)
            self.rj_accepted[bi] += racc
            self.rj_num_proposals[bi] += 1
        iperm, i1perm, u = tc.draw_swap_randoms()
        eng.pt_sweep(iperm, i1perm, u, adapt=False)                             # rj.py:381-382
        return acc, racc

    def _bd_numpy_all(self):
        """"together": every branch in one proposal - all branches' coins and leaf choices from R first, then the births from
        the global stream branch by branch (distgenrj.py:166-220)."""
        eng, tc, R, T, W = self.engine, self.temperature_control, self._random, self.ntemps, self.nwalkers
        _, inds, _, _, betas = eng.download()
        tc.betas = betas
        nb = len(self.branches)
        change, leaf = np.zeros((nb, T, W), dtype=np.int64), np.zeros((nb, T, W), dtype=np.int64)
        birth = [np.zeros((T, W, b.ndim)) for b in self.branches]
        for bi, b in enumerate(self.branches):
            if b.nleaves_min != b.nleaves_max:
                change[bi], leaf[bi] = self._draw_change_leaf(b, inds[b.name])
        for bi, b in enumerate(self.branches):
            if b.nleaves_min != b.nleaves_max:
                birth[bi][change[bi] == +1] = self._draw_births(b, int((change[bi] == +1).sum()))
        return eng.bd_all_step(change, leaf, birth, R.rand(T, W))               # rj.py:332

    def _draw_change_leaf(self, b, ib):
        R, T, W = self._random, self.ntemps, self.nwalkers
        nleaves = ib.sum(axis=-1)
        leaf = np.zeros((T, W), dtype=np.int64)
        change = R.choice([-1, +1], size=nleaves.shape)                         # distgenrj.py:63-66
        change = (change * ((nleaves != b.nleaves_min) & (nleaves != b.nleaves_max))
                  + (+1) * (nleaves == b.nleaves_min) + (-1) * (nleaves == b.nleaves_max))       # :69-73
        for t in range(T):                                                      # one draw per walker, in order (:85-121)
            for w in range(W):
                if change[t, w] == +1:
                    leaf[t, w] = R.choice(np.where(~ib[t, w])[0])
                elif change[t, w] == -1:
                    leaf[t, w] = R.choice(np.where(ib[t, w])[0])
        return change, leaf

    @staticmethod
    def _draw_births(b, nbirth):
        draws = np.zeros((nbirth, b.ndim))
        for d in range(b.ndim):                                                 # ProbDistContainer.rvs: GLOBAL stream, per parameter
            if b.prior is not None:            # the parameter's own distribution (SciPy's rvs bit for bit: eryn_amd.prior)
                draws[:, d] = b.prior.dists[d].rvs(nbirth)
            else:
                draws[:, d] = np.random.rand(nbirth) * (b.hi[d] - b.lo[d]) + b.lo[d]      # prior.py:60-66, 432-497
        return draws

    @staticmethod
    def _draw_mt_tries(spec, n, k):
        """``ProbDistContainer.rvs(size=(n, k))`` of a generator (prior.py:432-497): per parameter, in order, one array of n k values from
        the GLOBAL stream - the constructions of eryn_amd.prior's distributions."""
        t = spec.terms
        out = np.zeros((n, k, t["kind"].shape[0]))
        for d, kind in enumerate(t["kind"]):
            if kind == _lib.PRIOR_NORMAL:
                out[..., d] = np.random.randn(n, k) * t["c1"][d] + t["c0"][d]
            elif kind == _lib.PRIOR_LOG_UNIFORM:
                out[..., d] = np.exp(np.random.rand(n, k) * (np.log(t["hi"][d]) - np.log(t["lo"][d])) + np.log(t["lo"][d]))
            else:
                out[..., d] = np.random.rand(n, k) * (t["hi"][d] - t["lo"][d]) + t["lo"][d]
        return out

    def _bd_numpy(self, bi):
        """Birth / death on branch ``bi`` with the reference's draws (distgenrj.py:35-222, rj.py:169-352)."""
        eng, tc, R, T, W = self.engine, self.temperature_control, self._random, self.ntemps, self.nwalkers
        _, inds, _, _, betas = eng.download()
        tc.betas = betas
        b = self.branches[bi]
        if self.mt_moves is not None:
            # MTDistGenMoveRJ: coins and leaf choices from R; generate_dist.rvs(size=(N, K)) - per parameter, for ALL walkers - and the
            # one rand(N) of the pick from the global stream (mtdistgenrj.py:68, multipletry.py:57); then R.rand(T, W) (rj.py:332)
            mv = self.mt_moves[b.name]
            change, leaf = self._draw_change_leaf(b, inds[b.name])
            tries = self._draw_mt_tries(eng.mt_gen[bi], T * W, mv.num_try).reshape(T, W, mv.num_try, b.ndim)
            u_pick = np.random.rand(T * W).reshape(T, W)
            keep = eng.mt_bd_step(bi, change, leaf, tries, u_pick, R.rand(T, W))
            mv.accepted += keep
            mv.num_proposals += 1
            return keep
        change, leaf, birth = np.zeros((T, W), dtype=np.int64), np.zeros((T, W), dtype=np.int64), np.zeros((T, W, b.ndim))
        if b.nleaves_min != b.nleaves_max:
            change, leaf = self._draw_change_leaf(b, inds[b.name])
            birth[change == +1] = self._draw_births(b, int((change == +1).sum()))
        return eng.bd_step(bi, change, leaf, birth, R.rand(T, W))               # rj.py:332

    def _state(self, nan_fill=False):
        from .state import State
        x, inds, L, P, betas = self.engine.download(nan_fill=nan_fill)
        return State(x, inds=inds, log_like=L, log_prior=P, betas=betas)

    def run_mcmc(self, initial_state, nsteps, burn=None, thin_by=1, store=True, **unused):
        """ensemble.py:1047-1125; returns the last State.  Stored steps keep the reference's NaN fill of unused leaves
        (backends/backend.py:1049-1059) in ``self.chain`` (a list of States) - or, with ``backend=RJDeviceBackend()``, in device
        memory: ``burn`` iterations, then one device call per chain segment; ``self.chain`` stays empty and the backend's accessors
        (``get_chain`` / ``get_inds`` / ``get_nleaves`` / ...) read the same steps bit for bit."""
        from .state import State
        tc = self.temperature_control
        if initial_state is None:
            if self._previous_state is None:
                raise ValueError("Cannot have `initial_state=None` if run_mcmc has never been called.")
            initial_state = self._previous_state
        st = State(initial_state, copy=True)
        coords, inds = st.branches_coords, st.branches_inds
        for b in self.branches:
            if coords[b.name].shape != (self.ntemps, self.nwalkers, b.nleaves_max, b.ndim):
                raise ValueError("incompatible input dimensions")
        if st.betas is not None:
            tc.betas = np.array(st.betas, dtype=np.float64)
        if st.log_like is None or st.log_prior is None:
            L, P = self._eval(coords, inds)
            st.log_like = L if st.log_like is None else st.log_like
            st.log_prior = P if st.log_prior is None else st.log_prior
        if np.any(np.isinf(st.log_prior)):
            raise ValueError("The initial log_prior was +/- infinite")
        self.engine.upload(coords, inds, st.log_like, st.log_prior, tc.betas)
        self.engine.set_adapt_time(tc.time)
        on_device = self.backend is not None and store
        if on_device:
            self.backend.grow(nsteps, None)           # (the device buffers are made here, never inside the run)
        for phase, n, keep in (("burn", burn or 0, False), ("run", nsteps, store)):
            if on_device and phase == "run":          # one device call per chain segment; nothing crosses the host per stored step
                self.backend.append(n, thin_by)
                self.iteration += n
                continue
            for _ in range(n):
                if self.rng == "philox":
                    self.engine.step(thin_by if phase == "run" else 1)
                else:
                    for _ in range(thin_by if phase == "run" else 1):
                        self._iteration_numpy()
                if keep:
                    self.chain.append(self._state(nan_fill=True))
                self.iteration += 1
        out = self._state()
        tc.betas = out.betas
        if self.rng == "philox":
            c = self.engine.counters()
            tc.time, tc.swaps_accepted = c["adapt_time"], c["swaps_last"]
            # the moves' own counters (move.py:404-421), cumulative over the context's life like the device's
            mv = self.moves[0]
            mv.accepted, mv.num_proposals = c["accepted_mh"].copy(), c["num_mh"]
            self.rj_accepted_all, self.rj_num_proposals_all = c["accepted_bd"].copy(), c["num_bd"]
        self._previous_state = out
        return out

    def get_nleaves(self):
        if self.backend is not None:
            return self.backend.get_nleaves()
        return {b.name: np.stack([s.branches[b.name].nleaves for s in self.chain]) for b in self.branches}
