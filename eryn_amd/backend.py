"""Chain stores for ``run_mcmc(store=True)``: ``Backend`` in host memory, ``DeviceBackend`` / ``RJDeviceBackend`` in device memory.

The reference's storage engine (eryn/backends: HDF5, resume) is out of scope for this package (host-side I/O, consumes
``State`` snapshots).  These classes keep the accessor names the stretch + PT path's callers use, and the chain diagnostics of the
reference's Backend (backends/backend.py:354-385, 616-817): ``get_autocorr_time``, ``get_autocorr_thin_burn``,
``get_gelman_rubin_convergence_diagnostic`` and ``get_evidence_estimate`` on ``Backend`` and ``DeviceBackend``, computed by
``eryn_amd.chain_stats`` on a host chain and by the library's k_chain_moments / k_chain_act where the chain sits in device memory -
the same bits either way.  ``RJDeviceBackend`` has the ones defined under reversible jump - the Gelman-Rubin diagnostic with the
reference's projection through the leaf masks, the evidence, and the leaf counts (``get_nleaves``, ``get_nleaves_counts``) - on
k_rj_chain_leaves / k_rj_chain_leaf_moments / k_chain_moments.  Not built: the stepping-stone evidence.
"""
import numpy as np

from . import chain_stats


_TI_METHODS = ("therodynamic", "thermodynamic integration", "thermo", "ti")
_SS_METHODS = ("stepping stone", "ss", "step", "stone", "stepping-stone")


class _Diagnostics:
    """The reference Backend's chain diagnostics (backends/backend.py:354-385, 616-817) over two hooks a chain store provides for
    the kept steps ``first + j thin``, j < count, of rungs ``[0, ntemps)``:

    ``_stat_act(branch, first, count, thin, ntemps, lags)``     ``tau[ntemps, W, ndim]`` (chain_stats.act with ``lags`` as window)
    ``_stat_moments(field, first, count, thin, ntemps)``        ``(s, m2, n_finite)`` (chain_stats.moments; ``field`` a branch name,
                                                                "log_like" or "log_prior", the latter two masked)
    and ``_stat_rungs()``: how many rungs the chain holds.  Everything after the hooks is host arithmetic on arrays no larger
    than one stored step, shared by every store: the answer does not depend on where the chain lives."""

    def _kept(self, discard, thin):
        discard, thin = int(discard), int(thin)
        if discard < 0 or thin < 1:
            raise ValueError("discard >= 0 and thin >= 1")
        count = len(range(discard, self.iteration, thin))
        if count < 1:
            raise ValueError(f"no stored step is kept: {self.iteration} stored, discard={discard}")
        return discard, count, thin

    def get_autocorr_time(self, discard=0, thin=1, all_temps=False, multiply_thin=True, window=50, fast=False, average=True):
        """Integrated autocorrelation time per parameter: ``{branch: [1 or rungs stored, ndim]}`` (``average=False``:
        ``[..., nwalkers, ndim]``), in steps (times ``thin``) unless ``multiply_thin=False``.

        A departure from the reference: its accessor raises ValueError for ntemps > 1 before its own ``all_temps`` code can run
        (backends/backend.py:646-651), and every chain of this package is tempered.  This computes what that code computes: the
        cold rung, or every stored rung with ``all_temps=True``."""
        first, count, thin = self._kept(discard, thin)
        nt = self._stat_rungs() if all_temps else 1
        lags = chain_stats.lag_count(count, window, fast)
        out = {}
        for name in self.branch_names:
            tau = self._stat_act(name, first, count, thin, nt, lags)
            if average:
                tau = np.average(tau, axis=1)
            out[name] = tau * (thin if multiply_thin else 1)
        return out

    def get_autocorr_thin_burn(self):
        """``(discard, thin)``: twice the largest and half the smallest autocorrelation time (backends/backend.py:354-384).  A
        coordinate that never moved has tau = NaN, and ``int(NaN)`` raises ValueError here as it does in the reference."""
        tau = self.get_autocorr_time()
        tau_max, tau_min = 0.0, 1e10
        for values in tau.values():
            temp_max, temp_min = np.max(values), np.min(values)
            tau_max = tau_max if tau_max > temp_max else temp_max
            tau_min = tau_min if tau_min < temp_min else temp_min
        return (int(2 * tau_max), int(0.5 * tau_min))

    def get_gelman_rubin_convergence_diagnostic(self, discard=0, thin=1, doprint=True, per_walker=False):
        """``{branch: {rung: Rhat[ndim]}}`` (utils/utility.py:279-330 ``psrf`` per stored rung), and the reference's table."""
        first, count, thin = self._kept(discard, thin)
        nt = self._stat_rungs()
        out = {name: self._psrf_branch(name, first, count, thin, nt, per_walker) for name in self.branch_names}
        if doprint:
            print("  Gelman-Rubin diagnostic \n  <R\u0302>: Mean value for all parameters\n")
            print("  --------------")
            for name in self.branch_names:
                print(" Model: {}".format(name))
                print("   T \t <R\u0302>")
                print("  --------------")
                for t in range(nt):
                    print("   {:01d}\t{:3.2f}".format(t, np.mean(out[name][t])))
                print("\n")
        return out

    def _psrf_branch(self, name, first, count, thin, nt, per_walker):
        """``{rung: Rhat[ndim]}`` of one branch whose chain enters ``psrf`` as it lies (one leaf per walker)."""
        r = 0 if per_walker else chain_stats.third_split(self.nwalkers, count)[2]
        s, m2, _ = self._stat_moments(name, first, count, thin, nt)
        head = tail = None
        if r:
            head = self._stat_moments(name, first, r, thin, nt)[:2]
            tail = self._stat_moments(name, first + (count - r) * thin, r, thin, nt)[:2]
        return {t: chain_stats.psrf_from_moments(count, s[t], m2[t], head and (head[0][t], head[1][t]),
                                                 tail and (tail[0][t], tail[1][t]), per_walker) for t in range(nt)}

    def get_evidence_estimate(self, discard=0, thin=1, return_error=True, method="therodynamic"):
        """Thermodynamic-integration estimate of log Z, ``(logZ, dlogZ)`` or ``logZ`` (backends/backend.py:664-733).  The ladder
        must have stood still over the kept steps (``stop_adaptation``), and every rung must be stored."""
        m = method.lower()
        if m in _SS_METHODS:
            raise NotImplementedError("stepping-stone evidence is not built: the reference's logls[:, order, :].reshape(-1, ntemps) "
                                      "(utils/utility.py:255-256) mixes rungs with walkers, so there is nothing well defined to reproduce")
        if m not in _TI_METHODS:
            raise ValueError("Please choose only between 'thermodynamic' and 'stepping-stone' methods.")
        first, count, thin = self._kept(discard, thin)
        if self._stat_rungs() < self.ntemps:
            raise ValueError(f"the evidence needs every rung: the chain stores {self._stat_rungs()} of {self.ntemps} (ntemps_store)")
        betas_all = self._stat_betas(first, count, thin)
        if not (betas_all == betas_all[0]).all():
            raise ValueError("Cannot compute evidence estimation if betas are allowed to vary. Use stop_adaptation kwarg in temperature settings.")
        s, _, nf = self._stat_moments("log_like", first, count, thin, self.ntemps)
        logZ, dlogZ = chain_stats.thermodynamic_integration_log_evidence(betas_all[0], chain_stats.rung_means(s, nf))
        return (logZ, dlogZ) if return_error else logZ


def _steps(first, count, thin):
    return slice(first, first + (count - 1) * thin + 1, thin)


class Backend(_Diagnostics):
    def __init__(self):
        self.initialized = False

    def reset(self, nwalkers, ndims, ntemps=1, branch_names=None, **kwargs):
        self.nwalkers, self.ndims, self.ntemps = nwalkers, dict(ndims), ntemps
        self.branch_names = list(branch_names)
        self.iteration = 0
        self.chain = {k: np.empty((0, ntemps, nwalkers, 1, d)) for k, d in self.ndims.items()}
        self.log_like = np.empty((0, ntemps, nwalkers))
        self.log_prior = np.empty((0, ntemps, nwalkers))
        self.betas = np.empty((0, ntemps))
        self.accepted = np.zeros((ntemps, nwalkers))
        self.swaps_accepted = np.zeros(max(ntemps - 1, 0))
        self.random_state = None
        self.initialized = True

    def grow(self, ngrow, blobs=None):
        self._cap = self.iteration + ngrow
        for k in self.chain:
            a = self.chain[k]
            self.chain[k] = np.concatenate([a, np.empty((self._cap - a.shape[0],) + a.shape[1:])])
        for f in ("log_like", "log_prior", "betas"):
            a = getattr(self, f)
            setattr(self, f, np.concatenate([a, np.empty((self._cap - a.shape[0],) + a.shape[1:])]))

    def save_step(self, state, accepted, swaps_accepted=None, **kwargs):
        i = self.iteration
        for k, br in state.branches.items():
            self.chain[k][i] = br.coords
        self.log_like[i] = state.log_like
        self.log_prior[i] = state.log_prior
        if state.betas is not None:
            self.betas[i] = state.betas
        self.accepted += accepted
        if swaps_accepted is not None and len(swaps_accepted):
            self.swaps_accepted += swaps_accepted
        self.random_state = state.random_state
        self.iteration += 1

    def get_chain(self, discard=0, thin=1):
        return {k: v[discard:self.iteration:thin] for k, v in self.chain.items()}

    def get_log_like(self, discard=0, thin=1):
        return self.log_like[discard:self.iteration:thin]

    def get_log_prior(self, discard=0, thin=1):
        return self.log_prior[discard:self.iteration:thin]

    def get_betas(self, discard=0, thin=1):
        return self.betas[discard:self.iteration:thin]

    # -- diagnostics: the hooks of _Diagnostics over the host arrays --------------------------------------
    def _stat_rungs(self):
        return self.ntemps

    def _stat_act(self, branch, first, count, thin, ntemps, lags):
        return chain_stats.act(self.chain[branch][_steps(first, count, thin), :ntemps, :, 0, :], lags)[0]

    def _stat_moments(self, field, first, count, thin, ntemps):
        if field in self.chain:
            return chain_stats.moments(self.chain[field][_steps(first, count, thin), :ntemps, :, 0, :])
        return chain_stats.moments(getattr(self, field)[_steps(first, count, thin), :ntemps], mask=True)

    def _stat_betas(self, first, count, thin):
        return self.betas[_steps(first, count, thin)]


class _DeviceChain:
    """What ``DeviceBackend`` and ``RJDeviceBackend`` share: the open segment in device memory, closed segments on the host, one
    download per read.  A subclass names its arrays (``FIELDS``: what ``_download`` returns per stored step, first axis the step),
    its totals (``_zero_totals``: arrays that ``engine.chain_totals()`` returns in the same order) and calls ``_start`` from ``reset``."""

    FIELDS = ()

    def __init__(self, max_bytes=None, ntemps_store=None):
        self.initialized = False
        self.capacity = 0
        self.max_bytes, self.ntemps_store = max_bytes, ntemps_store
        self.engine, self.seed = None, None

    def attach(self, engine, seed):
        """The engine whose context holds the chain, and the sampler's Philox seed (the checkpoint's first half)."""
        self.engine, self.seed = engine, seed

    def _start(self, step_bytes, shape):
        """Head of ``reset``: the capacity ``max_bytes`` allows, counts and totals from zero.  A backend that is reset for another
        run of the same ``shape`` keeps its device buffers."""
        budget = self.engine.chain_info()["free_bytes"] // 4 if self.max_bytes is None else int(self.max_bytes)
        self.max_steps = max(1, budget // step_bytes)
        keep = self.capacity if self.initialized and getattr(self, "_shape", None) == shape else 0
        if keep:
            self.engine.chain_reset()
        self._shape = shape
        self.iteration = 0
        self.capacity = keep          # stored steps the device buffers hold (0: not created yet)
        self.downloads = 0            # chain copies from the device so far
        self.stats_launches = 0       # diagnostics launches on the device chain so far (k_chain_moments / k_chain_act)
        self._open = 0                # stored steps in the open (device) segment
        self._closed = None           # everything closed so far: {field: host array}
        self._segments = []           # ... and segments closed since somebody last read it
        self._closed_totals = self._zero_totals()
        self._cache = self._totals = None
        self.initialized = True

    # -- writing (the sampler) ---------------------------------------------------------------------
    def grow(self, ngrow, blobs=None):
        """Room for ``ngrow`` more stored steps, as far as ``max_bytes`` allows: the device buffers are made (or, when the
        open segment has no room left and may be larger, closed and remade) here, never inside a run."""
        room = self.capacity - self._open
        if self.capacity and (room >= ngrow or self.capacity >= self.max_steps):
            return
        self._close_segment()
        self.capacity = int(min(self.max_steps, max(ngrow, 1)))
        self.engine.chain_create(self.capacity, self.nstore)

    def append(self, n_store, *per_step):
        """``n_store`` stored steps on the device (the engine's ``step_chain``), closing the segment whenever it is full."""
        if not self.capacity:
            self.grow(n_store)
        while n_store > 0:
            if self._open == self.capacity:
                self._close_segment()
            n = min(self.capacity - self._open, n_store)
            self._cache = self._totals = None
            self.engine.step_chain(n, *per_step)
            self._open += n
            self.iteration += n
            n_store -= n

    def _close_segment(self):
        if not self._open:
            return
        seg, tot = self._open_segment(), self._open_totals()
        self._segments.append(seg)
        self._closed_totals = [a + b for a, b in zip(self._closed_totals, tot)]
        self.engine.chain_reset()
        self._open = 0
        self._cache = self._totals = None

    # -- reading -----------------------------------------------------------------------------------
    def _open_segment(self):
        if self._cache is None:
            self._cache = self._download(0, self._open)
            self.downloads += 1
        return self._cache

    def _open_totals(self):
        if self._totals is None:
            self._totals = self.engine.chain_totals()
        return self._totals

    def _total(self, i):
        return self._closed_totals[i] + self._open_totals()[i] if self._open else self._closed_totals[i]

    def _field(self, f, discard, thin):
        if self._segments:            # (once per read after a closure, not per step)
            parts = ([self._closed] if self._closed is not None else []) + self._segments
            self._closed = {k: np.concatenate([p[k] for p in parts]) for k in self.FIELDS}
            self._segments = []
        parts = [self._closed[f]] if self._closed is not None else []
        if self._open:
            parts.append(self._open_segment()[f])
        if not parts:
            return self._empty(f)
        full = parts[0] if len(parts) == 1 else np.concatenate(parts)
        return full[discard:self.iteration:thin]

    def get_log_like(self, discard=0, thin=1):
        return self._field("log_like", discard, thin)

    def get_log_prior(self, discard=0, thin=1):
        return self._field("log_prior", discard, thin)

    def get_betas(self, discard=0, thin=1):
        return self._field("betas", discard, thin)

    def get_random_states(self, discard=0, thin=1):
        """The Philox checkpoint of every stored step - what its State carries as ``random_state``: a sampler with the same
        seed started from stored step i (coordinates, log-likelihood, log-prior, ladder and this) continues the chain."""
        it, tm = self._field("iteration", discard, thin), self._field("adapt_time", discard, thin)
        return [("philox", self.seed, int(i), int(t)) for i, t in zip(it, tm)]

    @property
    def random_state(self):
        """The Philox checkpoint of the last stored step: ("philox", seed, iteration counter, adaptation time)."""
        if self._open:
            last = self.engine.chain_download(self._open - 1, 1, fields=())      # (host-side arrays of the context: no device copy)
        elif self._segments:
            last = self._segments[-1]
        elif self._closed is not None:
            last = self._closed
        else:
            return None
        return ("philox", self.seed, int(last["iteration"][-1]), int(last["adapt_time"][-1]))

    # -- diagnostics: what the hooks of _Diagnostics share on a device chain -------------------------------
    def _stat_rungs(self):
        return self.nstore

    def _on_device(self, first):
        """The kept steps from ``first`` on all lie in the open segment: its index there, else None."""
        closed = self.iteration - self._open
        return first - closed if first >= closed else None

    def _stat_betas(self, first, count, thin):
        f = self._on_device(first)
        if f is None:
            return self._field("betas", 0, 1)[_steps(first, count, thin)]
        return self.engine.chain_download(f, (count - 1) * thin + 1, fields=("betas",))["betas"][::thin]      # (count x T doubles: not a chain copy)


class DeviceBackend(_DeviceChain, _Diagnostics):
    """``Backend`` whose stored steps stay in device memory until somebody reads them (include/hipensemble.h: hens_chain_*).

    The reference's storage contract (backends/backend.py:1014-1091 ``save_step``) on the device: ``EnsembleSampler(...,
    backend=DeviceBackend(), rng="philox").run_mcmc(nsteps, thin_by=k)`` is one device call per chain SEGMENT - every stored step
    is appended by a small launch between the stepping launches, the accepted / swap totals accumulate beside the chain - and an
    accessor downloads the open segment once and keeps it until the next append.  Same accessors as ``Backend``; no array is
    concatenated or copied per stored step.

    max_bytes      device memory the open segment may take (default: a quarter of what is free at ``reset``); it fixes the
                   capacity in stored steps.  A run that outgrows it closes the segment - one download into host arrays, the
                   device buffers start again - and goes on.
    ntemps_store   store rungs ``[0, ntemps_store)`` only (default: all); ``swaps_accepted`` keeps its ntemps - 1 entries.

    An untempered sampler has no ladder: ``get_betas`` returns zeros there.

    The diagnostics (``get_autocorr_time`` ...) run on the device - one launch, nothing downloaded but arrays the size of a stored
    step: ``stats_launches`` counts them, ``downloads`` stays - when every kept step lies in the open segment; with closed
    segments among them they run ``eryn_amd.chain_stats`` over the host copy.  Both give the same bits."""

    FIELDS = ("x", "log_like", "log_prior", "betas", "iteration", "adapt_time")

    @staticmethod
    def bytes_per_step(ntemps, nwalkers, ndim, ntemps_store=None):
        """Device bytes of one stored step: coordinates, log-likelihood and log-prior of the stored rungs, the ladder."""
        return 8 * ((ntemps_store or ntemps) * nwalkers * (ndim + 2) + ntemps)

    def reset(self, nwalkers, ndims, ntemps=1, branch_names=None, **kwargs):
        if self.engine is None:
            raise RuntimeError("DeviceBackend.reset needs an engine (attach): EnsembleSampler(..., backend=DeviceBackend()) attaches its own")
        self.nwalkers, self.ndims, self.ntemps = nwalkers, dict(ndims), ntemps
        self.branch_names = list(branch_names)
        if len(self.branch_names) != 1:
            raise NotImplementedError("the device chain stores a single branch")
        self.ndim = self.ndims[self.branch_names[0]]
        self.nstore = int(self.ntemps_store or ntemps)
        if not 1 <= self.nstore <= ntemps:
            raise ValueError("ntemps_store must lie in [1, ntemps]")
        self._start(self.bytes_per_step(ntemps, nwalkers, self.ndim, self.nstore), (nwalkers, self.ndim, ntemps, self.nstore, id(self.engine)))

    def _zero_totals(self):
        return [np.zeros((self.nstore, self.nwalkers)), np.zeros(max(self.ntemps - 1, 0))]

    def _download(self, first, count):
        return self.engine.chain_download(first, count)

    def _empty(self, f):
        shape = dict(x=(self.nstore, self.nwalkers, self.ndim), betas=(self.ntemps,), iteration=(), adapt_time=())
        return np.empty((0,) + shape.get(f, (self.nstore, self.nwalkers)))

    def last_step(self, fields=()):
        """The last stored step of the open segment (HipEnsemble.chain_download of one step)."""
        return self.engine.chain_download(self._open - 1, 1, fields=fields)

    def get_chain(self, discard=0, thin=1):
        return {self.branch_names[0]: self._field("x", discard, thin)[:, :, :, None, :]}

    # -- diagnostics: the hooks of _Diagnostics (_stat_rungs, _on_device, _stat_betas: _DeviceChain) -----------
    def _stat_act(self, branch, first, count, thin, ntemps, lags):
        f = self._on_device(first)
        if f is None:
            return chain_stats.act(self._field("x", 0, 1)[_steps(first, count, thin), :ntemps], lags)[0]
        self.stats_launches += 1
        return self.engine.chain_act(f, count, thin, ntemps, lags)[0]

    def _stat_moments(self, field, first, count, thin, ntemps):
        name = "x" if field == self.branch_names[0] else field
        f = self._on_device(first)
        if f is None:
            return chain_stats.moments(self._field(name, 0, 1)[_steps(first, count, thin), :ntemps], mask=name != "x")
        self.stats_launches += 1
        return self.engine.chain_moments(name, f, count, thin, ntemps)

    @property
    def accepted(self):
        return self._total(0)

    @property
    def swaps_accepted(self):
        return self._total(1)


class RJDeviceBackend(_DeviceChain, _Diagnostics):
    """The chain of an ``RJEnsembleSampler`` in device memory (include/hipensemble.h: hens_rj_chain_*): ``RJEnsembleSampler(...,
    rng="philox", backend=RJDeviceBackend()).run_mcmc(state, nsteps, thin_by=k)`` is one device call per chain SEGMENT.  Every
    stored step is appended by one launch straight from the resident leaf-packing records - per branch the coordinates with the
    reference's NaN fill of unused leaves (backends/backend.py:1049-1059) and the leaf masks -, the accepted / rj_accepted /
    swaps_accepted totals the reference's backend keeps (:1069-1091) accumulate beside the chain, and an accessor downloads the
    open segment once.  ``max_bytes`` / ``ntemps_store``: as ``DeviceBackend``.

    The stored steps are bit for bit the ``State`` list the sampler keeps without ``backend=``.

    Diagnostics, under the reference's names (backends/backend.py:410-434, 664-817): ``get_gelman_rubin_convergence_diagnostic``
    (a branch of several leaves projected through its leaf masks), ``get_evidence_estimate``, ``get_nleaves(download=False)`` and
    ``get_nleaves_counts`` run on the device chain - k_rj_chain_leaves, k_rj_chain_leaf_moments, k_chain_moments; ``stats_launches``
    counts the launches, ``downloads`` stays - when every kept step lies in the open segment, and ``eryn_amd.chain_stats`` over the
    host copy otherwise: the same bits either way.  ``get_autocorr_time`` / ``get_autocorr_thin_burn`` raise ValueError as the
    reference's do under reversible jump.  Two departures from the reference's Gelman-Rubin accessor: min_leaves is taken per rung
    from the rungs stored here (the reference's is per rung as well, but over all ``ntemps``), and where the walker with the fewest
    leaves has too few for ``psrf`` (floor(W M / 3) < 2; ``per_walker``: M < 2) this raises ValueError naming branch and rung,
    where the reference's ``C[-0:]`` silently takes the whole array."""

    @staticmethod
    def bytes_per_step(ntemps, nwalkers, ncoord, nslots, ntemps_store=None):
        """Device bytes of one stored step: coordinates (``ncoord`` per walker), log-likelihood and log-prior of the stored rungs,
        the ladder, and one mask byte per leaf slot (``nslots`` per walker)."""
        ts = ntemps_store or ntemps
        return 8 * (ts * nwalkers * (ncoord + 2) + ntemps) + ts * nwalkers * nslots

    def reset(self, nwalkers, ndims, ntemps=1, branch_names=None, nleaves_max=None, **kwargs):
        if self.engine is None:
            raise RuntimeError("RJDeviceBackend.reset needs an engine (attach): RJEnsembleSampler(..., backend=RJDeviceBackend()) attaches its own")
        self.nwalkers, self.ndims, self.ntemps = nwalkers, dict(ndims), ntemps
        self.branch_names = list(branch_names)
        self.nleaves_max = {k: int(nleaves_max[k]) for k in self.branch_names}
        self.nstore = int(self.ntemps_store or ntemps)
        if not 1 <= self.nstore <= ntemps:
            raise ValueError("ntemps_store must lie in [1, ntemps]")
        self.FIELDS = tuple(f"{f}/{k}" for f in ("x", "inds") for k in self.branch_names) + ("log_like", "log_prior", "betas", "iteration", "adapt_time")
        ncoord = sum(self.nleaves_max[k] * self.ndims[k] for k in self.branch_names)
        dims = tuple((self.nleaves_max[k], self.ndims[k]) for k in self.branch_names)
        self._start(self.bytes_per_step(ntemps, nwalkers, ncoord, sum(self.nleaves_max.values()), self.nstore),
                    (nwalkers, dims, ntemps, self.nstore, id(self.engine)))

    def _zero_totals(self):
        return [np.zeros((self.nstore, self.nwalkers)), np.zeros((self.nstore, self.nwalkers)), np.zeros(max(self.ntemps - 1, 0))]

    def _download(self, first, count):
        seg = self.engine.chain_download(first, count)
        for f in ("x", "inds"):                  # (one key per array: the segments concatenate field by field)
            for k, a in seg.pop(f).items():
                seg[f"{f}/{k}"] = a
        return seg

    def _empty(self, f):
        lead = (0, self.nstore, self.nwalkers)
        if "/" in f:
            kind, k = f.split("/", 1)
            return np.empty(lead + (self.nleaves_max[k], self.ndims[k])) if kind == "x" else np.empty(lead + (self.nleaves_max[k],), dtype=bool)
        return np.empty((0,) + dict(betas=(self.ntemps,), iteration=(), adapt_time=()).get(f, lead[1:]))

    def get_chain(self, discard=0, thin=1):
        """``{name: [nsteps, ntemps_store, W, nleaves_max, ndim]}``, NaN on unused leaves."""
        return {k: self._field(f"x/{k}", discard, thin) for k in self.branch_names}

    def get_inds(self, discard=0, thin=1):
        """``{name: bool [nsteps, ntemps_store, W, nleaves_max]}``: which leaves are in use."""
        return {k: self._field(f"inds/{k}", discard, thin) for k in self.branch_names}

    def get_nleaves(self, discard=0, thin=1, download=True):
        """``{name: int [nsteps, ntemps_store, W]}``: leaves in use.  ``download=False`` answers from the device chain - one byte
        per walker and kept step (``chain_leaves``) - without copying the chain, when every kept step lies in the open segment."""
        if download or len(range(int(discard), self.iteration, int(thin))) < 1:
            return {k: v.sum(axis=-1, dtype=np.int64) for k, v in self.get_inds(discard, thin).items()}
        first, count, thin = self._kept(discard, thin)
        return {k: self._stat_leaves(k, first, count, thin, self.nstore, True)[0].astype(np.int64) for k in self.branch_names}

    def get_nleaves_counts(self, discard=0, thin=1):
        """``{name: int64 [ntemps_store, nleaves_max + 1]}``: per rung, how many (walker, kept step) pairs have k leaves in use -
        the posterior of the model count, unnormalised."""
        first, count, thin = self._kept(discard, thin)
        return {k: self._stat_leaves(k, first, count, thin, self.nstore, False)[1].sum(axis=1, dtype=np.int64) for k in self.branch_names}

    # -- diagnostics: the hooks of _Diagnostics, and the two of a chain with leaf masks ------------------------
    # Every device path applies when all kept steps lie in the open segment (_on_device); else eryn_amd.chain_stats runs over
    # the host copy.  Both give the same bits.
    def _stat_moments(self, field, first, count, thin, ntemps):
        """A branch's name: the coordinates as they lie, of a ONE-LEAF branch ``[ntemps, W, nd]``; "log_like" / "log_prior": masked."""
        branch = field in self.branch_names
        f = self._on_device(first)
        if f is None:
            a = self._field(f"x/{field}" if branch else field, 0, 1)[_steps(first, count, thin), :ntemps]
            out = chain_stats.moments(a, mask=not branch)
        else:
            self.stats_launches += 1
            out = self.engine.chain_moments(field, f, count, thin, ntemps)
        return tuple(a[:, :, 0] for a in out) if branch else out

    def _stat_leaves(self, name, first, count, thin, ntemps, nleaves):
        f = self._on_device(first)
        if f is None:
            nle, hist = chain_stats.leaf_counts(self._field(f"inds/{name}", 0, 1)[_steps(first, count, thin), :ntemps])
            return (nle if nleaves else None), hist
        self.stats_launches += 1
        return self.engine.chain_leaves(name, f, count, thin, ntemps, nleaves=nleaves)

    def _stat_leaf_moments(self, name, first, count, thin, ntemps, lo, hi):
        f = self._on_device(first)
        if f is None:
            sel = (_steps(first, count, thin), slice(0, ntemps))
            return chain_stats.leaf_moments(self._field(f"x/{name}", 0, 1)[sel], self._field(f"inds/{name}", 0, 1)[sel], lo, hi)
        self.stats_launches += 1
        return self.engine.chain_leaf_moments(name, f, count, thin, ntemps, lo, hi)

    def _psrf_branch(self, name, first, count, thin, nt, per_walker):
        """``{rung: Rhat[ndim]}``.  A one-leaf branch enters ``psrf`` as it lies, NaN included (backends/backend.py:780-783).  A
        branch of several leaves is projected through its masks (:786-797; eryn_amd.chain_stats.rj_psrf): one ``chain_leaves``
        launch gives every walker's total and with it each rung's M = min_leaves; the moments of the compacted series over the
        ordinals [0, M) - and, where third_split(W, M) leaves r != 0, over [0, r) and [M - r, M) - are ONE LAUNCH PER DISTINCT M
        over the rungs [0, last rung with that M], whose other rows are dropped: the C entry point takes one window per launch."""
        if self.nleaves_max[name] == 1:
            return super()._psrf_branch(name, first, count, thin, nt, per_walker)
        W = self.nwalkers
        totals = chain_stats.leaf_totals(self._stat_leaves(name, first, count, thin, nt, False)[1])
        M = [chain_stats.rj_min_leaves(totals[t], per_walker, name, t) for t in range(nt)]       # (ValueError before any moments launch)
        out = {}
        for m in sorted(set(M)):
            rungs = [t for t in range(nt) if M[t] == m]
            upto = rungs[-1] + 1
            s, m2, n = self._stat_leaf_moments(name, first, count, thin, upto, 0, m)
            assert (n[rungs] == m).all(), "a walker ran out of leaves below the smallest total"
            r = 0 if per_walker else chain_stats.third_split(W, m)[2]
            head = tail = None
            if r:
                head = self._stat_leaf_moments(name, first, count, thin, upto, 0, r)
                tail = self._stat_leaf_moments(name, first, count, thin, upto, m - r, m)
                assert (head[2][rungs] == r).all() and (tail[2][rungs] == r).all()
            for t in rungs:
                out[t] = chain_stats.psrf_from_moments(m, s[t], m2[t], head and (head[0][t], head[1][t]), tail and (tail[0][t], tail[1][t]), per_walker)
        return {t: out[t] for t in range(nt)}

    def get_autocorr_time(self, *args, **kwargs):
        """Not defined under reversible jump: the reference raises (backends/backend.py:648-651), and so does this."""
        raise ValueError("get_autocorr_time is not well-defined for number of temperatures > 1 or when using reversible jump.")

    def get_autocorr_thin_burn(self):
        return self.get_autocorr_time()

    @property
    def accepted(self):
        """In-model accepts of every stored step's last iteration, summed (backends/backend.py:1069)."""
        return self._total(0)

    @property
    def rj_accepted(self):
        """Birth / death accepts of every stored step's last iteration, summed (backends/backend.py:1070-1071)."""
        return self._total(1)

    @property
    def swaps_accepted(self):
        """In-model swaps of every stored step's last iteration, summed (backends/backend.py:1072)."""
        return self._total(2)
