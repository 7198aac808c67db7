"""HipEnsemble: thin object wrapper over the C ABI (one context = one GPU = one ladder shard)."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import HensConfig, HensDeviceBuffers, HensTiming, check, f64, ptr
from .prior import prior_spec, term_arrays


def box_logp_inside(lo, hi):
    """sum_d log(1/(hi_d - lo_d)) (prior.py:28-41 ``logpdf_val``) accumulated in the reference's order: ``prior.box_constant``."""
    return prior_spec((lo, hi), len(lo), bounds=True).logp_inside


FAST_WIDTHS = (8, 16, 32, 64, 128)       # row widths with compile-time-width kernels (csrc/hens.hip: fast_path)


def padded_width(ndim, likelihood):
    """Row width of the device pool for ``ndim`` real parameters.

    The compile-time-width kernels (in-place two-launch / one-launch iterations) serve rows of 8, 16, 32, 64 and 128
    doubles; other widths run the generic kernel in three copying launches (measured at 16 x 4096: D = 11 39.1 us,
    D = 12 34.5 us, D = 24 46.1 us per iteration against 16.1 us at D = 16 and 22.4 us at D = 32).  So rows of a Gaussian
    likelihood are padded up to the next such width with coordinates that never change: zeros, inside a (-inf, +inf) prior
    interval, meeting zero rows / columns of the precision matrix (``hens_config::ndim_active`` keeps the Hastings factor
    and the walker-count guard on the real dimension).  Not for the Rosenbrock likelihood (its coupled sum would see the
    pad) and host-callable likelihoods (their proposals travel to the host unpadded).  A property of (ndim, likelihood
    kind) only: every rank of a sharded ladder pads alike, so shards stay bit-identical to the whole ladder and agree on
    the row width of their messages.  ``HENS_NO_PAD=1`` switches it off."""
    if os.environ.get("HENS_NO_PAD") or ndim in FAST_WIDTHS or ndim > FAST_WIDTHS[-1]:
        return ndim
    if likelihood.kind not in (_lib.LIKE_GAUSS_DENSE, _lib.LIKE_GAUSS_DIAG):
        return ndim
    return next(w for w in FAST_WIDTHS if w >= ndim)


class ChainStoreCalls:
    """The four chain-store calls that read alike on both families, over the C entry points ``CHAIN_PREFIX + name``
    (include/hipensemble.h: hens_chain_* of a HipEnsemble, hens_rj_chain_* of an RJEngine); needs ``self.lib`` and ``self.ctx``."""
    CHAIN_PREFIX = None

    def _chain_call(self, name, *args):
        check(getattr(self.lib, self.CHAIN_PREFIX + name)(self.ctx, *args), self.ctx)

    def chain_create(self, capacity, ntemps_store=None):
        """Room for ``capacity`` stored steps of rungs ``[0, ntemps_store)`` (None: all) in device memory; replaces a chain
        that exists."""
        self._chain_call("create", int(capacity), int(ntemps_store or 0))

    def chain_reset(self):
        self._chain_call("reset")

    def chain_destroy(self):
        self._chain_call("destroy")

    def chain_info(self):
        info = _lib.HensChainInfo()
        self._chain_call("info", C.byref(info))
        return {k: getattr(info, k) for k, _ in _lib.HensChainInfo._fields_}


class HipEnsemble(ChainStoreCalls):
    CHAIN_PREFIX = "hens_chain_"

    def __init__(self, ntemps, nwalkers, ndim, likelihood, lo, hi, a=2.0, tempered=None,
                 adaptive=True, adaptation_lag=10000, adaptation_time=100, stop_adaptation=-1,
                 live_dangerously=False, fill_value=-1e300, seed=0, rung_range=None, device_id=0,
                 adaptation_delay=0, pad_rows=True, prior_terms=None):
        self.lib = _lib.load()
        self.T, self.W, self.D = int(ntemps), int(nwalkers), int(ndim)
        if tempered is None:
            tempered = self.T > 1
        r0, r1 = (0, self.T) if rung_range is None else (int(rung_range[0]), int(rung_range[1]))
        self.rung_begin, self.rung_end, self.Tl = r0, r1, r1 - r0
        if likelihood.ndim != self.D:
            raise ValueError("likelihood dimension does not match ndim")
        # RW: width of a device row (>= D, see padded_width); every array with a parameter axis is padded on the way in and
        # stripped on the way out, the caller only ever sees D
        self.RW = padded_width(self.D, likelihood) if pad_rows else self.D
        cfg = HensConfig(ntemps=self.T, nwalkers=self.W, ndim=self.RW, ndim_active=self.D if self.RW != self.D else 0,
                         rung_begin=r0, rung_end=r1,
                         device_id=int(device_id), likelihood_kind=int(likelihood.kind),
                         tempered=int(bool(tempered)), live_dangerously=int(bool(live_dangerously)),
                         adaptive=int(bool(adaptive)), adaptation_delay=int(adaptation_delay),
                         stop_adaptation=int(stop_adaptation), a=float(a),
                         fill_value=float(fill_value), adaptation_lag=float(adaptation_lag),
                         adaptation_time=float(adaptation_time), seed=int(seed) & (2**64 - 1))
        self.tempered = bool(tempered)
        self.num_try = None          # the tries of the multiple-try generator in the MH slot (set_mt_dist_proposal), None without one
        self.gibbs = dict(stretch=None, mh=None)      # the block tables the context holds (set_gibbs), [nblocks, D] bool or None
        self.state_epoch = 0         # bumped by every call that changes the walkers: a DeviceState (eryn_amd/state.py) is current while it matches
        self.lazy_downloads = 0
        self.a = float(a)
        self.ctx = C.c_void_p()
        code = self.lib.hens_create(C.byref(cfg), C.byref(self.ctx))
        if code != _lib.HENS_OK:
            self.ctx = None
            check(code, None)
        if prior_terms is not None:              # (lo / hi are the terms' supports then; the arguments are not read)
            self.set_prior_terms(prior_terms)
        else:
            self.set_prior_box(lo, hi)
        if self.RW != self.D:
            likelihood._install(self.lib, self.ctx, row_width=self.RW)
        else:
            likelihood._install(self.lib, self.ctx)
        self.likelihood = likelihood
        self.N0 = (self.W + 1) // 2

    def _pad(self, a, fill=0.0):
        """``a[..., D]`` -> C-contiguous ``[..., RW]`` with ``fill`` on the pads (the array itself when nothing is padded)."""
        if self.RW == self.D:
            return a
        out = np.full(a.shape[:-1] + (self.RW,), fill, dtype=np.float64)
        out[..., :self.D] = a
        return out

    def set_prior_terms(self, terms):
        """One independent prior distribution per parameter: ``terms`` is an ``eryn_amd.prior.ProbDistContainer`` or its
        ``prior_terms()`` dict (``kind`` int32, ``lo``, ``hi``, ``c0``, ``c1``, ``c2``, each ``[ndim]``); include/hipensemble.h,
        hens_set_prior_terms.  Uniform kinds only: the box, on the box's launch path."""
        spec = prior_spec(terms, self.D)
        check(self.lib.hens_set_prior_terms(self.ctx, *map(ptr, term_arrays(spec.terms, self.RW))), self.ctx)
        self._keep_prior(spec)

    def set_prior_box(self, lo, hi):
        """Back to (or another) uniform box: include/hipensemble.h, hens_set_prior_box."""
        spec = prior_spec((lo, hi), self.D, bounds=True)
        check(self.lib.hens_set_prior_box(self.ctx, ptr(self._pad(spec.lo, -np.inf)), ptr(self._pad(spec.hi, np.inf)), spec.logp_inside), self.ctx)
        self._keep_prior(spec)

    def _keep_prior(self, spec):
        """``lo`` / ``hi``: the supports; ``prior_terms``: the terms, None under a box; ``logp_inside``: the box's constant, None under terms."""
        self.lo, self.hi, self.prior_terms, self.logp_inside = spec.lo, spec.hi, spec.terms_beyond_box, spec.logp_inside

    def set_stretch_scale(self, a):
        """``StretchMove.a`` for every later proposal (the reference's tuning hook mutates it, utils/updates.py:130-175)."""
        check(self.lib.hens_set_stretch_scale(self.ctx, float(a)), self.ctx)
        self.a = float(a)

    def set_periodic(self, period):
        """Periods of the periodic parameters, ``[ndim]`` (0 = not periodic), or None for none: the ``periodic``
        argument of the reference's sampler / moves for the single branch (ensemble.py:165-168, utils/periodic.py)."""
        if period is None:
            check(self.lib.hens_set_periodic(self.ctx, None), self.ctx)
            self.period = None
            return
        self.period = f64(period, (self.D,))
        check(self.lib.hens_set_periodic(self.ctx, ptr(self._pad(self.period))), self.ctx)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.hens_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- state ---------------------------------------------------------------------------------
    def upload(self, x, logl=None, logp=None, betas=None):
        self.state_epoch += 1
        x = self._pad(f64(x, (self.Tl, self.W, self.D)))
        logl = None if logl is None else f64(logl, (self.Tl, self.W))
        logp = None if logp is None else f64(logp, (self.Tl, self.W))
        betas = None if betas is None else f64(betas, (self.T,))
        check(self.lib.hens_upload_state(self.ctx, ptr(x), ptr(logl), ptr(logp), ptr(betas)), self.ctx)

    def download(self, want_x=True):
        x = np.empty((self.Tl, self.W, self.RW)) if want_x else None
        logl = np.empty((self.Tl, self.W))
        logp = np.empty((self.Tl, self.W))
        betas = np.empty(self.T) if self.tempered else None
        check(self.lib.hens_download_state(self.ctx, ptr(x), ptr(logl), ptr(logp), ptr(betas)), self.ctx)
        if want_x and self.RW != self.D:
            x = np.ascontiguousarray(x[..., :self.D])
        return x, logl, logp, betas

    def eval_state(self):
        self.state_epoch += 1
        check(self.lib.hens_eval_state(self.ctx), self.ctx)

    # -- parity-mode steps -----------------------------------------------------------------------
    nsplits = 2

    def set_nsplits(self, nsplits):
        """Sets of the parity API's red-blue move (``RedBlueMove(nsplits=...)``, red_blue.py:41-47): include/hipensemble.h,
        hens_set_nsplits."""
        check(self.lib.hens_set_nsplits(self.ctx, int(nsplits)), self.ctx)
        self.nsplits = int(nsplits)

    def set_size(self, split):
        """Walkers of set ``split``: arange(W) % nsplits, shuffled (red_blue.py:119-124)."""
        return (self.W - int(split) + self.nsplits - 1) // self.nsplits

    def stretch_split(self, split, labels, rint, u_zz, u_acc):
        self.state_epoch += 1
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        if labels.shape != (self.Tl, self.W):
            raise ValueError("labels must have shape (ntemps, nwalkers)")
        Ns = self.set_size(split)
        rint = np.ascontiguousarray(rint, dtype=np.int64)
        u_zz, u_acc = f64(u_zz, (self.Tl, Ns)), f64(u_acc, (self.Tl, Ns))
        if rint.shape != (self.Tl, Ns):
            raise ValueError(f"rint must have shape {(self.Tl, Ns)}")
        keep = np.empty((self.Tl, Ns), dtype=np.uint8)
        check(self.lib.hens_stretch_split(self.ctx, int(split), ptr(labels), ptr(rint), ptr(u_zz), ptr(u_acc),
                                          ptr(keep)), self.ctx)
        return keep.astype(bool)

    def propose_split(self, split, labels, rint, u_zz):
        """Host-likelihood contexts: proposed points q[Tl, Ns, D] and the in-prior mask [Tl, Ns]."""
        labels = np.ascontiguousarray(labels, dtype=np.uint8)
        Ns = self.set_size(split)
        rint = np.ascontiguousarray(rint, dtype=np.int64)
        u_zz = f64(u_zz, (self.Tl, Ns))
        if labels.shape != (self.Tl, self.W) or rint.shape != (self.Tl, Ns):
            raise ValueError("labels / rint have the wrong shape")
        q = np.empty((self.Tl, Ns, self.D))
        inbox = np.empty((self.Tl, Ns), dtype=np.uint8)
        check(self.lib.hens_propose_split(self.ctx, int(split), ptr(labels), ptr(rint), ptr(u_zz), ptr(q),
                                          ptr(inbox)), self.ctx)
        return q, inbox.astype(bool)

    def accept_split(self, split, logl, u_acc):
        self.state_epoch += 1
        Ns = self.set_size(split)
        logl, u_acc = f64(logl, (self.Tl, Ns)), f64(u_acc, (self.Tl, Ns))
        keep = np.empty((self.Tl, Ns), dtype=np.uint8)
        check(self.lib.hens_accept_split(self.ctx, int(split), ptr(logl), ptr(u_acc), ptr(keep)), self.ctx)
        return keep.astype(bool)

    def pt_sweep(self, iperm, i1perm, u_swap, adapt=True):
        self.state_epoch += 1
        shp = (self.T - 1, self.W)
        iperm = np.ascontiguousarray(iperm, dtype=np.int64)
        i1perm = np.ascontiguousarray(i1perm, dtype=np.int64)
        u_swap = f64(u_swap, shp)
        if iperm.shape != shp or i1perm.shape != shp:
            raise ValueError(f"iperm/i1perm must have shape {shp}")
        sel = np.zeros(shp, dtype=np.uint8)
        swaps = np.zeros(max(self.T - 1, 0))
        check(self.lib.hens_pt_sweep(self.ctx, ptr(iperm), ptr(i1perm), ptr(u_swap), int(bool(adapt)), ptr(sel),
                                     ptr(swaps)), self.ctx)
        return sel.astype(bool), swaps

    # -- production ------------------------------------------------------------------------------
    def step(self, n_iters):
        self.state_epoch += 1
        check(self.lib.hens_step(self.ctx, int(n_iters)), self.ctx)

    def step_marked(self, n_before, n_last):
        """n_before iterations, the accept counters kept on the device, n_last iterations (thin_by > 1: the reference stores
        the accept mask of the last sub-iteration only, ensemble.py:968-979); see marked_counters."""
        self.state_epoch += 1
        check(self.lib.hens_step_marked(self.ctx, int(n_before), int(n_last)), self.ctx)

    def step_report(self, n_iters, n_last=1):
        """``step(n_iters)`` + what a sampler loop reads after every proposal (ensemble.py:974-977) in one call: the accept counts
        of the last ``n_last`` iterations ``[Tl, W]`` (uint8), the last cascade's swap counts, the ladder.  The walkers stay on
        the device (include/hipensemble.h: hens_step_report)."""
        self.state_epoch += 1
        acc = np.empty((self.Tl, self.W), dtype=np.uint8)
        swaps = np.zeros(max(self.T - 1, 0))
        betas = np.empty(self.T) if self.tempered else None
        check(self.lib.hens_step_report(self.ctx, int(n_iters), int(n_last), ptr(acc), ptr(swaps) if self.T > 1 else None, ptr(betas)), self.ctx)
        return acc, swaps, betas

    # -- chain store (include/hipensemble.h: hens_chain_*, hens_step_chain; chain_create / _reset / _destroy / _info: ChainStoreCalls) --
    def step_chain(self, n_store, iters_per_store=1, n_last=1):
        """``n_store`` stored steps of ``iters_per_store`` iterations each, appended to the chain on the device; the accepted
        totals take the last ``n_last`` iterations of every step (ensemble.py:968-979).  Nothing is copied to the host."""
        self.state_epoch += 1
        check(self.lib.hens_step_chain(self.ctx, int(n_store), int(iters_per_store), int(n_last)), self.ctx)

    def chain_download(self, first=0, count=None, fields=("x", "log_like", "log_prior", "betas")):
        """Stored steps ``[first, first + count)`` (count None: to the end) as a dict: ``x[count, ntemps_store, W, D]`` (the
        caller's D: pads are not stored), ``log_like`` / ``log_prior`` ``[count, ntemps_store, W]``, ``betas[count, T]`` - those
        named in ``fields`` - and ``iteration`` / ``adapt_time`` ``[count]``, the Philox checkpoint of every stored step."""
        info = self.chain_info()
        first = int(first)
        count = info["count"] - first if count is None else int(count)
        Ts, n = info["ntemps_store"], max(count, 0)
        out = dict(iteration=np.zeros(n, dtype=np.int64), adapt_time=np.zeros(n, dtype=np.int64))
        shapes = dict(x=(n, Ts, self.W, self.D), log_like=(n, Ts, self.W), log_prior=(n, Ts, self.W), betas=(n, self.T))
        for f in fields:
            out[f] = np.empty(shapes[f])
        check(self.lib.hens_chain_download(self.ctx, first, count, ptr(out.get("x")), ptr(out.get("log_like")),
                                           ptr(out.get("log_prior")), ptr(out.get("betas")), ptr(out["iteration"]),
                                           ptr(out["adapt_time"])), self.ctx)
        return out

    def chain_totals(self):
        """(accepted[ntemps_store, W], swaps_accepted[T - 1]) summed over the steps stored since the last reset."""
        Ts = self.chain_info()["ntemps_store"]
        acc = np.zeros((Ts, self.W))
        swaps = np.zeros(max(self.T - 1, 0))
        check(self.lib.hens_chain_totals(self.ctx, ptr(acc), ptr(swaps) if self.T > 1 else None), self.ctx)
        return acc, swaps

    # -- chain diagnostics (include/hipensemble.h: hens_chain_moments, hens_chain_act) ----------------------
    FIELD_CODES = dict(x=0, log_like=1, log_prior=2)

    def chain_moments(self, field, first, count, thin=1, ntemps=None):
        """``(sum, m2, n_finite)`` per series of ``field`` ("x": ``[ntemps, W, D]``; "log_like" / "log_prior": ``[ntemps, W]``)
        over the kept steps ``first + j thin``, j < count, of the open chain: eryn_amd.chain_stats.moments bit for bit, computed
        where the chain is."""
        nt = int(self.chain_info()["ntemps_store"] if ntemps is None else ntemps)
        shape = (max(nt, 0), self.W) + ((self.D,) if field == "x" else ())
        s, m2, nf = np.empty(shape), np.empty(shape), np.empty(shape, dtype=np.int64)
        check(self.lib.hens_chain_moments(self.ctx, self.FIELD_CODES[field], int(first), int(count), int(thin), nt, ptr(s), ptr(m2), ptr(nf)), self.ctx)
        return s, m2, nf

    def chain_act(self, first, count, thin=1, ntemps=None, window=50):
        """``(tau, mean, c0)`` ``[ntemps, W, D]`` of the coordinates over the kept steps: eryn_amd.chain_stats.act bit for bit
        with ``K = min(window, count)`` lags."""
        nt = int(self.chain_info()["ntemps_store"] if ntemps is None else ntemps)
        shape = (max(nt, 0), self.W, self.D)
        tau, mean, c0 = np.empty(shape), np.empty(shape), np.empty(shape)
        check(self.lib.hens_chain_act(self.ctx, int(first), int(count), int(thin), nt, int(window), ptr(tau), ptr(mean), ptr(c0)), self.ctx)
        return tau, mean, c0

    def chain_stats_ms(self):
        """Durations (ms) of the last k_chain_moments and k_chain_act launches, -1 where there was none."""
        a, b = C.c_double(-1.0), C.c_double(-1.0)
        check(self.lib.hens_chain_stats_ms(self.ctx, C.byref(a), C.byref(b)), self.ctx)
        return dict(moments_ms=a.value, act_ms=b.value)

    def download_betas(self):
        betas = np.empty(self.T)
        check(self.lib.hens_download_state(self.ctx, None, None, None, ptr(betas)), self.ctx)
        return betas

    def marked_counters(self):
        """The accept counts (stretch move, MH move) in front of the last step_marked call's final iterations."""
        acc = np.zeros((self.Tl, self.W))
        acc_mh = np.zeros((self.Tl, self.W))
        check(self.lib.hens_get_marked_counters(self.ctx, ptr(acc), ptr(acc_mh)), self.ctx)
        return acc, acc_mh

    def synchronize(self):
        check(self.lib.hens_synchronize(self.ctx), self.ctx)

    def counters(self):
        acc = np.empty((self.Tl, self.W))
        nprop, atime = C.c_int64(0), C.c_int64(0)
        last = np.zeros(max(self.T - 1, 0))
        total = np.zeros(max(self.T - 1, 0))
        check(self.lib.hens_get_counters(self.ctx, ptr(acc), C.byref(nprop), ptr(last), ptr(total),
                                         C.byref(atime)), self.ctx)
        return dict(accepted=acc, num_proposals=nprop.value, swaps_last=last, swaps_total=total,
                    adapt_time=atime.value)

    def reset_counters(self):
        check(self.lib.hens_reset_counters(self.ctx), self.ctx)

    def set_adapt_time(self, t):
        check(self.lib.hens_set_adapt_time(self.ctx, int(t)), self.ctx)

    def debug_permutation(self, which, rung, it):
        out = np.empty(self.W, dtype=np.int32)
        check(self.lib.hens_debug_permutation(self.ctx, int(which), int(rung), int(it), ptr(out)), self.ctx)
        return out

    def set_iteration(self, it):
        """Resume: move the Philox iteration counter (hens_set_iteration) - with the same seed, an uploaded state and the
        adaptation time restored, ``step`` continues a stored chain bit for bit."""
        check(self.lib.hens_set_iteration(self.ctx, int(it)), self.ctx)

    def iteration(self):
        """Index of the next Philox iteration ``step`` will run."""
        n = C.c_int64(0)
        check(self.lib.hens_get_iteration(self.ctx, C.byref(n)), self.ctx)
        return int(n.value)

    def debug_draws(self, it, mh=False, block=0):
        """The Philox draws ``step`` consumes in iteration ``it`` (include/hipensemble.h: hens_debug_draws); ``block``: those of
        that Gibbs block of the iteration's move (hens_debug_draws_block)."""
        T, Tl, W, D = self.T, self.Tl, self.W, self.D
        out = dict(own=np.empty((Tl, W), dtype=np.int32), cw=np.empty((Tl, W), dtype=np.int32),
                   u_zz=np.empty((Tl, W)), u_acc=np.empty((Tl, W)))
        pt = self.tempered and T > 1
        if pt:
            out.update(pt_slot=np.empty((T, W), dtype=np.int32), u_swap=np.empty((T - 1, W)))
        if mh:
            out.update(mh_step=np.empty((Tl, W, self.RW)), mh_u=np.empty((Tl, W)))
        is_mh = C.c_int32(0)
        fn, head = (self.lib.hens_debug_draws_block, (int(it), int(block))) if block else (self.lib.hens_debug_draws, (int(it),))
        check(fn(self.ctx, *head, ptr(out["own"]), ptr(out["cw"]), ptr(out["u_zz"]), ptr(out["u_acc"]), ptr(out.get("pt_slot")),
                 ptr(out.get("u_swap")), C.byref(is_mh), ptr(out.get("mh_step")), ptr(out.get("mh_u"))), self.ctx)
        out["is_mh"] = bool(is_mh.value)
        for move, keys in (("stretch", ("cw", "u_zz", "u_acc")), ("mh", ("mh_step", "mh_u"))) if block else ():
            table = self.gibbs[move]               # (the other move's table may be shorter: its arrays are not written then)
            if block >= (1 if table is None else len(table)):
                for k in keys:
                    out.pop(k, None)
        if mh and self.RW != D and "mh_step" in out:
            out["mh_step"] = np.ascontiguousarray(out["mh_step"][..., :D])
        return out

    def set_profiling(self, on):
        """0 / False off; 1 / True a HIP event pair per launch (HIP stream); 2 the launches' own dispatch timestamps on the queue
        the call uses anyway (include/hipensemble.h: hens_set_profiling)."""
        check(self.lib.hens_set_profiling(self.ctx, int(on)), self.ctx)

    def timing(self):
        t = HensTiming()
        check(self.lib.hens_get_timing(self.ctx, C.byref(t)), self.ctx)
        return {k: getattr(t, k) for k, _ in HensTiming._fields_}

    def launch_times(self):
        """(n_launches, 2) begin / end in us after the first launch's begin, of the last step() made with set_profiling(True)."""
        n = C.c_int64(0)
        check(self.lib.hens_debug_launch_times(self.ctx, None, 0, C.byref(n)), self.ctx)
        out = np.zeros(max(n.value, 0))
        if n.value:
            check(self.lib.hens_debug_launch_times(self.ctx, ptr(out), n.value, C.byref(n)), self.ctx)
        return out.reshape(-1, 2)

    # -- ladder sharding (eryn_amd/ladder.py) ----------------------------------------------------------
    def stretch_iter(self):
        """One Philox iteration of both halves on the resident rungs (asynchronous, no PT)."""
        self.state_epoch += 1
        check(self.lib.hens_stretch_iter(self.ctx), self.ctx)

    def device_buffers(self):
        b = HensDeviceBuffers()
        check(self.lib.hens_get_device_buffers(self.ctx, C.byref(b)), self.ctx)
        return b

    def pt_plan_sharded(self, rank_of_rung, nranks, my_rank, iperm=None, i1perm=None, u_swap=None, adapt=True,
                        want_swaps=True):
        rank_of_rung = np.ascontiguousarray(rank_of_rung, dtype=np.int32)
        if rank_of_rung.shape != (self.T,):
            raise ValueError("rank_of_rung must have shape (ntemps,)")
        shp = (self.T - 1, self.W)
        if iperm is not None:
            iperm = np.ascontiguousarray(iperm, dtype=np.int64)
            i1perm = np.ascontiguousarray(i1perm, dtype=np.int64)
            u_swap = f64(u_swap, shp)
            if iperm.shape != shp or i1perm.shape != shp:
                raise ValueError(f"iperm/i1perm must have shape {shp}")
        send = np.zeros(nranks, dtype=np.int64)
        recv = np.zeros(nranks, dtype=np.int64)
        sel = np.zeros(shp, dtype=np.uint8) if iperm is not None else None
        swaps = np.zeros(self.T - 1) if want_swaps else None
        check(self.lib.hens_pt_plan_sharded(self.ctx, ptr(iperm), ptr(i1perm), ptr(u_swap), int(bool(adapt)),
                                            ptr(rank_of_rung), int(nranks), int(my_rank), ptr(send), ptr(recv),
                                            ptr(sel), ptr(swaps)), self.ctx)
        return send, recv, (None if sel is None else sel.astype(bool)), swaps

    def set_stream(self, stream_handle):
        """Launch on a caller-owned HIP stream (e.g. torch's current stream, so RCCL collectives and the
        kernels order themselves without host synchronisation)."""
        check(self.lib.hens_set_stream(self.ctx, C.c_void_p(int(stream_handle))), self.ctx)

    # -- Metropolis-Hastings proposals (include/hipensemble.h: hens_mh_*) --------------------------------
    def mh_step(self, step, u_acc):
        """One full-ensemble proposal q = x + step with the caller's draws; returns the accept mask [Tl, W]."""
        self.state_epoch += 1
        step = self._pad(np.ascontiguousarray(step, dtype=np.float64).reshape(self.Tl, self.W, self.D))
        u_acc = np.ascontiguousarray(u_acc, dtype=np.float64).reshape(self.Tl, self.W)
        keep = np.empty((self.Tl, self.W), dtype=np.uint8)
        check(self.lib.hens_mh_step(self.ctx, ptr(step), ptr(u_acc), ptr(keep)), self.ctx)
        return keep.astype(bool)

    def set_mh_proposal(self, kind, scale, weight):
        """Mix Gaussian MH proposals into ``step()``: kind "iso" | "diag" | "full" (scale = std dev, std devs,
        lower Cholesky factor), weight = probability per iteration; kind None switches the mix off."""
        self._move_cfg = None                                  # (DeviceMove._propose_philox's memo of what it asked for last)
        if kind is None:
            check(self.lib.hens_set_mh_proposal(self.ctx, -1, None, 0.0), self.ctx)
            self.num_try = None
            return
        k = {"iso": 0, "diag": 1, "full": 2}[kind]
        scale = np.ascontiguousarray(np.atleast_1d(scale), dtype=np.float64)
        need = {0: 1, 1: self.D, 2: self.D * self.D}[k]
        if scale.size != need:
            raise ValueError(f"{kind} proposal needs {need} scale value(s)")
        if self.RW != self.D and k == 0:                       # no step on the pads: the same normals, per-parameter scales
            k, scale = 1, self._pad(np.full(self.D, float(scale[0])))
        elif self.RW != self.D and k == 1:
            scale = self._pad(scale)
        elif self.RW != self.D and k == 2:
            full = np.zeros((self.RW, self.RW))
            full[:self.D, :self.D] = scale.reshape(self.D, self.D)
            scale = full
        check(self.lib.hens_set_mh_proposal(self.ctx, k, ptr(scale), float(weight)), self.ctx)
        self.num_try = None

    # -- DistributionGenerate (include/hipensemble.h: hens_set_dist_proposal, hens_dist_step) ------------
    def set_dist_proposal(self, terms, weight):
        """The generator of the independence proposal into the context's one MH slot: ``terms`` is anything ``prior_spec`` reads
        (a ``ProbDistContainer``, its dict, a ``prior_terms()`` dict), ``weight`` the probability that an iteration of ``step()``
        runs this move.  ``set_mh_proposal`` replaces it and it replaces ``set_mh_proposal``; ``set_mh_proposal(None, ...)``
        switches either off."""
        self._move_cfg = None
        spec = prior_spec(terms, self.D)
        check(self.lib.hens_set_dist_proposal(self.ctx, *map(ptr, term_arrays(spec.terms, self.RW)), float(weight)), self.ctx)
        self.num_try = None

    def dist_step(self, q, u_acc, want_factors=False):
        """One full-ensemble independence proposal with the caller's points ``q[Tl, W, D]`` and accept uniforms; returns the accept
        mask ``[Tl, W]``, with ``want_factors`` also the Hastings factors ``logq(old) - logq(new)``."""
        self.state_epoch += 1
        q = self._pad(np.ascontiguousarray(q, dtype=np.float64).reshape(self.Tl, self.W, self.D))
        u_acc = np.ascontiguousarray(u_acc, dtype=np.float64).reshape(self.Tl, self.W)
        keep = np.empty((self.Tl, self.W), dtype=np.uint8)
        fac = np.empty((self.Tl, self.W)) if want_factors else None
        check(self.lib.hens_dist_step(self.ctx, ptr(q), ptr(u_acc), ptr(keep), ptr(fac)), self.ctx)
        return (keep.astype(bool), fac) if want_factors else keep.astype(bool)

    # -- MTDistGenMove (include/hipensemble.h: hens_set_mt_dist_proposal, hens_mt_dist_step, hens_mt_debug_draws) ----
    def set_mt_dist_proposal(self, terms, num_try, weight):
        """The generator of the multiple-try independence proposal and its number of tries (1 .. 64) into the context's one MH
        slot: ``terms`` and ``weight`` as for ``set_dist_proposal``, which it replaces and which replaces it."""
        self._move_cfg = None
        spec = prior_spec(terms, self.D)
        check(self.lib.hens_set_mt_dist_proposal(self.ctx, *map(ptr, term_arrays(spec.terms, self.RW)), int(num_try), float(weight)), self.ctx)
        self.num_try = int(num_try)

    def mt_dist_step(self, q, u_pick, u_acc, want=()):
        """One full-ensemble multiple-try proposal with the caller's tries ``q[Tl, W, K, D]``, pick uniforms and accept uniforms;
        returns the accept mask ``[Tl, W]``, or with ``want`` (names among "pick", "lsw", "aux_lsw", "factors") a dict that holds
        ``keep`` and those."""
        self.state_epoch += 1
        q = np.ascontiguousarray(q, dtype=np.float64)
        K = q.size // (self.Tl * self.W * self.D)
        if self.num_try is not None and (K != self.num_try or q.size != self.Tl * self.W * K * self.D):      # (None: no generator set, the call refuses)
            raise ValueError(f"q must hold {self.num_try} tries per walker: [{self.Tl}, {self.W}, {self.num_try}, {self.D}]")
        q = self._pad(q.reshape(self.Tl, self.W * K, self.D))
        u_pick = np.ascontiguousarray(u_pick, dtype=np.float64).reshape(self.Tl, self.W)
        u_acc = np.ascontiguousarray(u_acc, dtype=np.float64).reshape(self.Tl, self.W)
        keep = np.empty((self.Tl, self.W), dtype=np.uint8)
        pick = np.empty((self.Tl, self.W), dtype=np.int32) if "pick" in want else None
        lsw = np.empty((2, self.Tl, self.W)) if ("lsw" in want or "aux_lsw" in want) else None
        fac = np.empty((self.Tl, self.W)) if "factors" in want else None
        check(self.lib.hens_mt_dist_step(self.ctx, ptr(q), ptr(u_pick), ptr(u_acc), ptr(keep), ptr(pick), ptr(lsw), ptr(fac)), self.ctx)
        if not want:
            return keep.astype(bool)
        out = dict(keep=keep.astype(bool), pick=pick, factors=fac)
        if lsw is not None:
            out.update(lsw=lsw[0], aux_lsw=lsw[1])
        return {k: v for k, v in out.items() if k == "keep" or k in want}

    def mt_debug_draws(self, it):
        """What the multiple-try launch draws in iteration ``it``: tries ``[Tl, W, K, D]``, pick and accept uniforms ``[Tl, W]``."""
        K = self.num_try or 1
        q = np.empty((self.Tl, self.W, K, self.RW))
        u_pick = np.empty((self.Tl, self.W))
        u_acc = np.empty((self.Tl, self.W))
        check(self.lib.hens_mt_debug_draws(self.ctx, int(it), ptr(q), ptr(u_pick), ptr(u_acc)), self.ctx)
        return np.ascontiguousarray(q[..., :self.D]), u_pick, u_acc

    # -- Gibbs parameter blocks (include/hipensemble.h: hens_set_gibbs, hens_gibbs_select) ---------------
    GIBBS_MOVES = dict(stretch=0, mh=1)

    def set_gibbs(self, move, masks):
        """The block table of ``move`` ("stretch" | "mh"): ``masks`` bool ``[nblocks, ndim]``, one row per Gibbs block (true = the
        coordinate moves with the block), or None / empty to clear it.  ``step()`` then proposes block after block and runs one
        cascade per iteration; the teacher-forced calls propose the block ``gibbs_select`` names."""
        m = self.GIBBS_MOVES[move]
        masks = None if masks is None else np.atleast_2d(np.asarray(masks, dtype=bool))
        if masks is None or masks.shape[0] == 0:
            check(self.lib.hens_set_gibbs(self.ctx, m, 0, None), self.ctx)
            self.gibbs[move] = None
            return
        if masks.ndim != 2 or masks.shape[1] != self.D:
            raise ValueError(f"masks must have shape (nblocks, {self.D})")
        padded = np.zeros((masks.shape[0], self.RW), dtype=np.uint8)
        padded[:, :self.D] = masks
        check(self.lib.hens_set_gibbs(self.ctx, m, masks.shape[0], ptr(padded)), self.ctx)
        self.gibbs[move] = masks.copy()

    def gibbs_select(self, move, block):
        check(self.lib.hens_gibbs_select(self.ctx, self.GIBBS_MOVES[move], int(block)), self.ctx)

    def mh_counters(self):
        acc = np.zeros((self.Tl, self.W))
        n = C.c_int64(0)
        check(self.lib.hens_get_mh_counters(self.ctx, ptr(acc), C.byref(n)), self.ctx)
        return dict(accepted=acc, num_proposals=int(n.value))

    # -- RCCL neighbour exchange inside the library (include/hipensemble.h: hens_comm_*) ----------------
    def comm_unique_id(self):
        """128 bytes from ncclGetUniqueId (call on ONE rank, hand the bytes to the others)."""
        buf = (C.c_ubyte * 128)()
        check(self.lib.hens_comm_unique_id(C.cast(buf, C.c_void_p)), None)
        return bytes(buf)

    def comm_init(self, nranks, rank, unique_id):
        """Collective: this shard becomes rank `rank` of `nranks`; ``step(n)`` then sends the neighbour messages itself."""
        if len(unique_id) != 128:
            raise ValueError("unique_id: 128 bytes from comm_unique_id()")
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        check(self.lib.hens_comm_init(self.ctx, int(nranks), int(rank), C.cast(buf, C.c_void_p)), self.ctx)

    def comm_destroy(self):
        check(self.lib.hens_comm_destroy(self.ctx), self.ctx)

    def comm_selfsend(self, values):
        src = np.ascontiguousarray(values, dtype=np.float64)
        dst = np.empty_like(src)
        check(self.lib.hens_comm_selfsend(self.ctx, src.size, ptr(src), ptr(dst)), self.ctx)
        return dst

    # -- ladder pipeline (include/hipensemble.h: hens_pipe_*) ------------------------------------------
    def pipe_init(self, nranks, rank):
        """Allocate this shard's mailbox; returns the 128-byte blob of HIP IPC handles (mailbox, walker pool)."""
        h = (C.c_ubyte * 128)()
        nbytes = C.c_int64(0)
        check(self.lib.hens_pipe_init(self.ctx, int(nranks), int(rank), C.cast(h, C.c_void_p), C.byref(nbytes)), self.ctx)
        self.pipe_bytes = int(nbytes.value)
        return bytes(h)

    def pipe_connect(self, handles):
        """handles: the ranks' IPC blobs concatenated in rank order (other processes)."""
        buf = (C.c_ubyte * len(handles)).from_buffer_copy(handles)
        check(self.lib.hens_pipe_connect(self.ctx, C.cast(buf, C.c_void_p)), self.ctx)

    def pipe_connect_local(self, engines):
        """All shards live in this process (several contexts on one GPU)."""
        arr = (C.c_void_p * len(engines))(*[e.ctx for e in engines])
        check(self.lib.hens_pipe_connect_local(self.ctx, C.cast(arr, C.c_void_p)), self.ctx)

    def pipe_connect_staged(self):
        """Staged transport: the pipeline's kernels write into local outboxes, the caller moves the messages."""
        check(self.lib.hens_pipe_connect_staged(self.ctx), self.ctx)

    def pipe_regions(self):
        from ._lib import HensPipeRegions
        r = HensPipeRegions()
        check(self.lib.hens_pipe_regions(self.ctx, C.byref(r)), self.ctx)
        return r

    def pipe_stage(self, stage):
        check(self.lib.hens_pipe_stage(self.ctx, int(stage)), self.ctx)

    def pipe_debug_stats(self, reset=True):
        """{site: (seconds waited summed over workgroups, waits)} - needs HENS_PIPE_STATS=1 at pipe_init."""
        raw = np.zeros(16, dtype=np.uint64)
        check(self.lib.hens_pipe_debug_stats(self.ctx, ptr(raw), int(bool(reset))), self.ctx)
        names = ["stretch:rows", "stretch:counts", "walk:columns", "bottom:cold rung", "bottom:rows from above",
                 "walk:collector waits for the grid", "walk:collector tail"]
        return {n: (float(raw[2 * i]) * 1e-8, int(raw[2 * i + 1])) for i, n in enumerate(names)}

    def pt_finish_sharded(self, n_recv):
        self.state_epoch += 1
        check(self.lib.hens_pt_finish_sharded(self.ctx, int(n_recv)), self.ctx)
