"""Minimal in-memory chain store so ``run_mcmc(store=True)`` is usable.

The reference's storage engine (eryn/backends, HDF5, resume, ACT/evidence accessors) is out
of scope for this package (host-side I/O, consumes ``State`` snapshots).  This class
keeps the accessor names the stretch + PT path's callers use.
"""
import numpy as np


class Backend:
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


class DeviceBackend(_DeviceChain):
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

    An untempered sampler has no ladder: ``get_betas`` returns zeros there."""

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

    @property
    def accepted(self):
        return self._total(0)

    @property
    def swaps_accepted(self):
        return self._total(1)


class RJDeviceBackend(_DeviceChain):
    """The chain of an ``RJEnsembleSampler`` in device memory (include/hipensemble.h: hens_rj_chain_*): ``RJEnsembleSampler(...,
    rng="philox", backend=RJDeviceBackend()).run_mcmc(state, nsteps, thin_by=k)`` is one device call per chain SEGMENT.  Every
    stored step is appended by one launch straight from the resident leaf-packing records - per branch the coordinates with the
    reference's NaN fill of unused leaves (backends/backend.py:1049-1059) and the leaf masks -, the accepted / rj_accepted /
    swaps_accepted totals the reference's backend keeps (:1069-1091) accumulate beside the chain, and an accessor downloads the
    open segment once.  ``max_bytes`` / ``ntemps_store``: as ``DeviceBackend``.

    The stored steps are bit for bit the ``State`` list the sampler keeps without ``backend=``."""

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

    def get_nleaves(self, discard=0, thin=1):
        """``{name: int [nsteps, ntemps_store, W]}``: leaves in use."""
        return {k: v.sum(axis=-1, dtype=np.int64) for k, v in self.get_inds(discard, thin).items()}

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
