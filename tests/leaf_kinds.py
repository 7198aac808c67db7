"""The device's leaf kinds stated in NumPy (eryn_amd.rj.LEAF_KINDS, include/hipensemble.h HENS_RJ_KIND_*): the yardstick of
tests/test_leaf_kinds.py and tests/test_hip_leaf_kinds.py.

Value of one leaf at the data points ``t`` (float64, every operation in the order written):

  pulse   (a, b, c)      a exp(-(t - b)^2 / (2 c^2))        the reference tests' own (oracle/eryn_oracle_rj.py: template_log_like)
  sine    (a, b, c)      a sin(2 pi b t + c)
  offset  (a)            a
  ramp    (a, b)         a + b t
  lorentz (a, b, c)      z = (t - b) / c;  a / (1 + z z)
  chirp   (a, b, c)      a sin((2 pi b) t + c (t t))
  burst   (a, t0, w, f)  z = (t - t0) / w;  (a exp(-(z z))) cos((2 pi f) (t - t0))

A walker's template is ONE running sum from zeros: branches in order, a branch's active leaves in ascending slot order
(oracle/eryn_oracle_rj.py: lorentz_chirp_log_like, ramp_burst_log_like, offset_log_like - which this module equals bit for bit on
their models, tests/test_leaf_kinds.py), ``L = -1/2 sum(((template - y) / sigma)^2)``.  Who is evaluated and what the others get
(-inf prior, no leaf: the fill value) is the caller's business (oracle/eryn_oracle_rj.py: compute_log_like)."""
import numpy as np

KINDS = {"pulse": (0, 3), "sine": (1, 3), "offset": (2, 1), "ramp": (3, 2), "lorentz": (4, 3), "chirp": (5, 3), "burst": (6, 4)}
NAME_OF = {v[0]: k for k, v in KINDS.items()}


def kind_name(kind):
    return kind if kind in KINDS else NAME_OF[int(kind)]


class Branch:
    """name, leaf kind (a name of KINDS), box, leaf budget: what the helper, the oracle (``.ndim``, ``.lo``, ``.hi``,
    ``.leaf_logpdf`` through ``to_oracle``) and eryn_amd.rj.TemplateBranch need to know about one model type."""

    def __init__(self, name, kind, box, nleaves_max, nleaves_min=0):
        self.name, self.kind = name, kind_name(kind)
        self.box = [tuple(map(float, b)) for b in box]
        assert len(self.box) == KINDS[self.kind][1]
        self.ndim = len(self.box)
        self.nleaves_max, self.nleaves_min = int(nleaves_max), int(nleaves_min)

    def to_oracle(self, cov=None):
        from oracle import eryn_oracle_rj as orj
        return orj.Branch(self.name, KINDS[self.kind][0], self.box, self.nleaves_max, self.nleaves_min, cov=cov)

    def to_device(self):
        from eryn_amd.rj import TemplateBranch
        return TemplateBranch(self.name, self.kind, self.box, self.nleaves_max, self.nleaves_min)


def leaf_value(kind, p, t):
    """One leaf's value at ``t`` [N]; ``p`` the leaf's parameters (NumPy scalars, as iterating a float64 array yields them)."""
    kind = kind_name(kind)
    if kind == "pulse":
        a, b, c = p
        return a * np.exp(-((t - b) ** 2) / (2 * c ** 2))
    if kind == "sine":
        a, b, c = p
        return a * np.sin(2 * np.pi * b * t + c)
    if kind == "offset":
        (a,) = p
        return a + np.zeros_like(t)
    if kind == "ramp":
        a, b = p
        return a + b * t
    if kind == "lorentz":
        a, b, c = p
        z = (t - b) / c
        return a / (1.0 + z * z)
    if kind == "chirp":
        a, b, c = p
        return a * np.sin((2 * np.pi * b) * t + c * (t * t))
    if kind == "burst":
        a, t0, w, f = p
        z = (t - t0) / w
        return (a * np.exp(-(z * z))) * np.cos((2 * np.pi * f) * (t - t0))
    raise KeyError(kind)


def walker_log_like(kinds, leaves, t, y, sigma):
    """The reference's per-walker calling convention (ensemble.py:1420-1470): ``leaves[b]`` the active leaves of branch b,
    [nleaves, width], or None; with ONE model type the function is handed that branch's leaves directly (:1466-1467)."""
    if len(kinds) == 1 and not isinstance(leaves, (list, tuple)):
        leaves = [leaves]
    tm = np.zeros_like(t)
    for kind, lv in zip(kinds, leaves):
        if lv is None:
            continue
        with np.errstate(all="ignore"):
            for p in np.asarray(lv, dtype=np.float64).reshape(-1, KINDS[kind_name(kind)][1]):
                tm = tm + leaf_value(kind, p, t)
    return -0.5 * np.sum(((tm - y) / sigma) ** 2)


def like_fn(kinds):
    """``walker_log_like`` for a model, as ``OracleRJSampler(like_fn=...)`` and ``CallableLikelihood`` call a user function."""
    kinds = [kind_name(k) for k in kinds]
    return lambda leaves, t, y, sigma: walker_log_like(kinds, leaves, t, y, sigma)


def template_log_like(branches, x, inds, t, y, sigma):
    """[T, W]: every walker's log-likelihood, those without a leaf included (the template of zeros).  ``branches``: objects with
    ``.name`` and ``.kind``; ``x[name]`` [T, W, nleaves_max, width], ``inds[name]`` [T, W, nleaves_max]."""
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)
    first = branches[0].name
    T, W = x[first].shape[:2]
    out = np.zeros((T, W))
    kinds = [b.kind for b in branches]
    for tt in range(T):
        for w in range(W):
            leaves = [x[b.name][tt, w][inds[b.name][tt, w]] if inds[b.name][tt, w].any() else None for b in branches]
            out[tt, w] = walker_log_like(kinds, leaves, t, y, sigma)
    return out
