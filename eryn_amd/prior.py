"""Priors with the reference's names (eryn/prior.py:12-136, 219-497), reduced to what the device hot path supports:
one independent distribution per parameter - uniform, log-uniform or normal.  The engine evaluates the prior inside its
kernels (include/hipensemble.h: hens_set_prior_box, hens_set_prior_terms); these objects describe the terms, evaluate
them on the host in the same arithmetic (``logpdf``) and draw starting points (``rvs``).

The arithmetic of one term is SciPy's (``rv_continuous.logpdf``: ``y = (x - loc) / scale``, the support test,
``_logpdf(y) - log(scale)``), the sum is the reference container's (prior.py:364-383: ``prior_vals += temp`` from 0.0),
taken in ascending parameter order."""
from typing import NamedTuple, Optional

import numpy as np

from ._lib import PRIOR_LOG_UNIFORM, PRIOR_NORMAL, PRIOR_UNIFORM, f64

NORM_PDF_LOGC = float(np.log(np.sqrt(2 * np.pi)))         # SciPy's _norm_pdf_logC


def _size(size):
    if not isinstance(size, (int, tuple)):
        raise ValueError("size must be an integer or tuple of ints.")
    return (size,) if isinstance(size, int) else size


class UniformDistribution:
    kind = PRIOR_UNIFORM

    def __init__(self, min_val, max_val):
        if min_val > max_val:
            min_val, max_val = max_val, min_val
        elif min_val == max_val:
            raise ValueError("Min and max values are the same.")
        self.min_val, self.max_val = min_val, max_val
        self.diff = max_val - min_val
        self.pdf_val = 1 / self.diff
        self.logpdf_val = np.log(self.pdf_val)

    def rvs(self, size=1):
        return np.random.rand(*_size(size)) * self.diff + self.min_val

    def logpdf(self, x):
        """prior.py:80-88: the constant inside [min, max] (inclusive), -inf outside."""
        x = np.asarray(x, dtype=np.float64)
        out = np.zeros_like(x)
        out[(x >= self.min_val) & (x <= self.max_val)] = self.logpdf_val
        out[~((x >= self.min_val) & (x <= self.max_val))] = -np.inf
        return out

    def term(self):
        """(kind, lo, hi, c0, c1, c2) of hens_set_prior_terms."""
        return self.kind, float(self.min_val), float(self.max_val), float(self.logpdf_val), 0.0, 0.0


def uniform_dist(min, max):
    return UniformDistribution(min, max)


class LogUniformDistribution:
    """``scipy.stats.loguniform(a, b)``: density 1 / (x log(b / a)) on [a, b] (inclusive), 0 < a < b.

    ``logpdf`` is SciPy's ``-log(x) - log(log(b) - log(a))``; the second logarithm is formed once, here."""
    kind = PRIOR_LOG_UNIFORM

    def __init__(self, a, b):
        a, b = float(a), float(b)
        if not (0.0 < a < b < np.inf):
            raise ValueError("log-uniform distribution needs 0 < a < b < inf")
        self.a, self.b = a, b
        self.log_norm = float(np.log(np.log(b) - np.log(a)))
        if not np.isfinite(self.log_norm):
            raise ValueError("log-uniform distribution: log(b) - log(a) underflows")

    def rvs(self, size=1):
        return np.exp(np.random.rand(*_size(size)) * (np.log(self.b) - np.log(self.a)) + np.log(self.a))

    def logpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        inside = (x >= self.a) & (x <= self.b)
        out = np.full(x.shape, -np.inf)
        out[inside] = (-np.log(x[inside])) - self.log_norm
        return out

    def term(self):
        return self.kind, self.a, self.b, self.log_norm, 0.0, 0.0


def log_uniform(min, max):
    """The reference's ``log_uniform(min, max)`` (prior.py:115-136) builds ``scipy.stats.loguniform(min, max - min)``: the
    distribution's upper bound is ``max - min``, NOT ``max``.  This function reproduces that construction, so the same call
    gives the same prior and the same chain; for a log-uniform distribution on ``[a, b]`` use
    ``LogUniformDistribution(a, b)``."""
    if min > max:
        min, max = max, min
    return LogUniformDistribution(min, max - min)


class NormalDistribution:
    """``scipy.stats.norm(loc, scale)``: ``y = (x - loc) / scale``, ``(-(y y) / 2 - log(sqrt(2 pi))) - log(scale)`` on every
    finite x (the engine refuses non-finite coordinates before any prior is asked: ensemble.py:1258-1262)."""
    kind = PRIOR_NORMAL

    def __init__(self, loc=0.0, scale=1.0):
        loc, scale = float(loc), float(scale)
        if not np.isfinite(loc) or not (0.0 < scale < np.inf):
            raise ValueError("normal distribution needs a finite loc and a finite scale > 0")
        self.loc, self.scale = loc, scale
        self.log_scale = float(np.log(scale))

    def rvs(self, size=1):
        return np.random.randn(*_size(size)) * self.scale + self.loc

    def logpdf(self, x):
        x = np.asarray(x, dtype=np.float64)
        with np.errstate(invalid="ignore", over="ignore"):
            y = (x - self.loc) / self.scale
            out = (-(y * y) / 2.0 - NORM_PDF_LOGC) - self.log_scale
        out = np.asarray(out)
        out[~np.isfinite(x)] = -np.inf
        return out

    def term(self):
        return self.kind, -np.inf, np.inf, self.loc, self.scale, self.log_scale


def _from_scipy(dist):
    """A frozen SciPy ``uniform`` / ``loguniform`` (``reciprocal``) / ``norm`` as one of the classes above, by duck typing
    (``.dist.name``, ``.args``, ``.kwds``): SciPy is not imported.  And what carries ``min_val`` / ``max_val``, as the reference's own
    ``UniformDistribution`` does (prior.py:12-88; the leaf-packing sampler has always read those two), as a ``UniformDistribution``."""
    if hasattr(dist, "min_val") and hasattr(dist, "max_val"):
        return UniformDistribution(dist.min_val, dist.max_val)
    name = getattr(getattr(dist, "dist", None), "name", None)
    if name is None or not hasattr(dist, "args") or not hasattr(dist, "kwds"):
        return None
    args, kwds = tuple(dist.args), dict(dist.kwds)

    def shape_loc_scale(nshape):
        shapes, rest = args[:nshape], args[nshape:]
        if len(shapes) < nshape or len(rest) > 2 or set(kwds) - {"loc", "scale"} or (len(rest) >= 1 and "loc" in kwds) or (
                len(rest) == 2 and "scale" in kwds):
            raise NotImplementedError(f"scipy.stats.{name}: arguments the device path cannot read ({args}, {kwds})")
        loc = rest[0] if len(rest) >= 1 else kwds.get("loc", 0.0)
        scale = rest[1] if len(rest) == 2 else kwds.get("scale", 1.0)
        return shapes, float(loc), float(scale)

    if name == "uniform":
        _, loc, scale = shape_loc_scale(0)
        if not scale > 0.0:
            raise ValueError("scipy.stats.uniform needs scale > 0")
        return UniformDistribution(loc, loc + scale)
    if name == "norm":
        _, loc, scale = shape_loc_scale(0)
        return NormalDistribution(loc, scale)
    if name in ("loguniform", "reciprocal"):
        (a, b), loc, scale = shape_loc_scale(2)
        if loc != 0.0 or scale != 1.0:
            raise NotImplementedError("scipy.stats.loguniform with a loc / scale shift is outside the device path")
        return LogUniformDistribution(a, b)
    return None


class ProbDistContainer:
    """``{index: distribution}`` container (prior.py:219-392).  Single integer keys 0..ndim-1, each with a
    ``UniformDistribution`` (``uniform_dist``), a ``LogUniformDistribution`` (``log_uniform``), a ``NormalDistribution`` or
    the frozen SciPy ``uniform`` / ``loguniform`` / ``norm`` equivalent; anything else cannot run inside the kernels.

    The terms are summed in ascending parameter order, whatever the order of the dictionary (the reference adds them in
    the dictionary's order: write the dictionary in ascending order and both agree to the last bit)."""

    def __init__(self, priors_in):
        self.priors_in = dict(priors_in)
        for k in self.priors_in:
            if isinstance(k, (tuple, str)) or not isinstance(k, (int, np.integer)):
                raise NotImplementedError("the device path takes one distribution per single integer parameter key")
        keys = sorted(self.priors_in)
        if keys != list(range(len(keys))):
            raise ValueError("prior keys must be the integers 0..ndim-1")
        self.dists = []
        for k in keys:
            dist = self.priors_in[k]
            if not isinstance(dist, (UniformDistribution, LogUniformDistribution, NormalDistribution)):
                dist = _from_scipy(dist)
            if dist is None:
                raise NotImplementedError("the device path supports uniform, log-uniform and normal priors only")
            self.dists.append(dist)
        self.ndim = len(keys)
        self.priors = [([k], self.dists[k]) for k in keys]

    @property
    def is_box(self):
        return all(isinstance(d, UniformDistribution) for d in self.dists)

    def box_bounds(self):
        if not self.is_box:
            raise NotImplementedError("box_bounds: the container holds other than uniform distributions (prior_terms)")
        lo = np.array([d.min_val for d in self.dists], dtype=np.float64)
        hi = np.array([d.max_val for d in self.dists], dtype=np.float64)
        return lo, hi

    def prior_terms(self):
        """``dict(kind=int32[ndim], lo, hi, c0, c1, c2)``: the arguments of hens_set_prior_terms (include/hipensemble.h)."""
        rows = [d.term() for d in self.dists]
        out = dict(kind=np.array([r[0] for r in rows], dtype=np.int32))
        for j, name in enumerate(("lo", "hi", "c0", "c1", "c2"), start=1):
            out[name] = np.array([r[j] for r in rows], dtype=np.float64)
        return out

    def logpdf(self, x):
        """prior.py:337-392 for ``x[..., ndim]`` (one point: a scalar comes back)."""
        x = np.asarray(x, dtype=np.float64)
        squeeze = x.ndim == 1
        if squeeze:
            x = x[None, :]
        elif x.ndim != 2:
            raise ValueError("x needs to 1 or 2 dimensional array.")
        vals = np.zeros(x.shape[0])
        for k, dist in enumerate(self.dists):
            vals += dist.logpdf(x[:, k])
        return vals[0].item() if squeeze else vals

    def rvs(self, size=1):
        if isinstance(size, int):
            size = (size,)
        out = np.zeros(tuple(size) + (self.ndim,))
        for k in range(self.ndim):
            out[..., k] = self.dists[k].rvs(size=tuple(size))
        return out


# ---- one specification of "the caller's prior" for every consumer: both samplers, the moves, both engines -------------------------------
TERM_KEYS = ("kind", "lo", "hi", "c0", "c1", "c2")          # the arguments of hens_set_prior_terms / hens_rj_set_prior_terms, in order
_PAD = dict(kind=PRIOR_UNIFORM, lo=-np.inf, hi=np.inf, c0=0.0, c1=0.0, c2=0.0)      # a padded row's pad: uniform on the line, no term


def box_constant(c0):
    """The constant log-density inside a box from its uniform terms' constants ``log(1/(hi_d - lo_d))``: ``((0.0 + c0_0) + c0_1) +
    ...``, the reference's sequential ``prior_vals += temp`` (prior.py:364-383) in ascending parameter order - the sum the library
    forms (csrc/hens_prior_host.h: fold_box)."""
    acc = np.zeros(1)
    for v in c0:
        acc += v
    return float(acc[0])


class PriorSpec(NamedTuple):
    """What ``prior_spec`` makes of a caller's prior."""
    container: Optional[ProbDistContainer]      # None: the caller gave bounds or terms, no distributions
    terms: dict                                 # kind int32, lo / hi / c0 / c1 / c2 float64, each C-contiguous [ndim]
    lo: np.ndarray                              # terms["lo"], terms["hi"]: the inclusive supports
    hi: np.ndarray
    is_box: bool                                # every term uniform
    logp_inside: Optional[float]                # a box's constant log-density (box_constant), None otherwise

    @property
    def terms_beyond_box(self):
        """The terms where they say more than ``lo`` / ``hi`` do (``HipEnsemble(prior_terms=...)``): None for a box."""
        return None if self.is_box else self.terms


def prior_spec(priors, ndim=None, bounds=False):
    """One reading of a prior, however the caller wrote it: a ``ProbDistContainer``; the ``{index: distribution}`` dict it is made
    of; a ``prior_terms()`` dict; a list of ``(lo, hi)`` per parameter (a box); with ``bounds=True`` the box as ``(lo, hi)``, two
    arrays or scalars that broadcast to ``ndim``; or a ``PriorSpec``.  ``ndim`` given: the number of parameters it must describe."""
    if isinstance(priors, PriorSpec):
        spec = priors
    else:
        container = None
        if isinstance(priors, dict) and "kind" not in priors:
            priors = ProbDistContainer(priors)
        if isinstance(priors, ProbDistContainer):
            container, terms = priors, priors.prior_terms()
        elif isinstance(priors, dict):
            terms = priors
        elif priors is not None and bounds:
            lo, hi = (f64(np.broadcast_to(b, (ndim,))) for b in priors)
            terms = _box_terms(lo, hi)
        elif isinstance(priors, (list, tuple)):
            terms = _box_terms(f64([b[0] for b in priors]), f64([b[1] for b in priors]))
        else:
            raise NotImplementedError("priors must be per-parameter uniform / log-uniform / normal priors (eryn_amd.prior.ProbDistContainer)")
        kind = np.ascontiguousarray(terms["kind"], dtype=np.int32)
        n = kind.shape[0] if ndim is None and kind.ndim == 1 else ndim
        if kind.shape != (n,):
            raise ValueError(f"prior terms must have shape {(n,)}")
        terms = dict(kind=kind, **{k: f64(terms[k], (n,)) for k in TERM_KEYS[1:]})
        is_box = bool(np.all(kind == PRIOR_UNIFORM))
        spec = PriorSpec(container, terms, terms["lo"], terms["hi"], is_box, box_constant(terms["c0"]) if is_box else None)
    if ndim is not None and spec.lo.shape != (ndim,):
        raise ValueError(f"prior terms must have shape {(ndim,)}")
    return spec


def _box_terms(lo, hi):
    n = lo.shape[0]
    return dict(kind=np.zeros(n, dtype=np.int32), lo=lo, hi=hi, c0=[np.log(1 / (hi[d] - lo[d])) for d in range(n)], c1=np.zeros(n), c2=np.zeros(n))


def term_arrays(terms, width=None):
    """The six array arguments of hens_set_prior_terms / hens_rj_set_prior_terms (``TERM_KEYS``) from one terms dict or from a list
    of them, one after the other (a model's branches); ``width``: padded to that many entries with the pad of a padded row."""
    if isinstance(terms, dict):
        terms = [terms]
    out = []
    for k in TERM_KEYS:
        a = np.concatenate([t[k] for t in terms])
        if width is not None and width > a.shape[0]:
            a = np.concatenate([a, np.full(width - a.shape[0], _PAD[k])])
        out.append(np.ascontiguousarray(a, dtype=np.int32 if k == "kind" else np.float64))
    return out
