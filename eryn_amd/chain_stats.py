"""Chain diagnostics, stated once in NumPy: the arithmetic the device kernels (csrc/hens_chain_stats.h: k_chain_moments,
k_chain_act; csrc/hens_rj_chain_stats.h: k_rj_chain_leaves, k_rj_chain_leaf_moments) reproduce bit for bit, and the host functions
on top of it.

The reference computes these in utils/utility.py (:43-144 ``get_acf`` / ``get_integrated_act``, :147-212
``thermodynamic_integration_log_evidence``, :279-330 ``psrf``) for its Backend's accessors (backends/backend.py:354-385, 616-817).
Here the reductions over the step axis have a FIXED summation order, so that the answer does not depend on where the chain lives.

One series ``x_0 ... x_{n-1}`` (axis 0 of the array: the kept steps), float64 throughout, every operation rounded on its own
(no fused multiply-add: the library is built with -ffp-contract=off):

    s     = sum_j x_j                         sequential, j ascending, from 0.0
    mean  = s / n
    y_j   = x_j - mean
    m2    = sum_j y_j y_j                     sequential: the second of two passes, as np.var
    c_k   = sum_{j=0}^{n-1-k} y_j y_{j+k}     k = 0 .. K-1; ONE accumulator per lag, j ascending, from 0.0
    K     = min(window, n);  fast=True: min(window, 2^floor(log2 n))
    tau   = 1 + 2 sum_{k=1}^{K-1} (c_k / c_0) sequential in k, from 0.0

A constant series has c_0 = 0, every ratio is 0 / 0 and tau = NaN, as the reference's ``acf / acf[0]``: not special-cased.
With ``mask=True`` (log-likelihood / log-prior series) non-finite entries are skipped and counted: ``s`` over the finite ones,
``n_finite``, ``m2`` about ``s / n_finite``.  -1e300 is finite and stays in (backends/backend.py:712-714).

``fast``: the reference crops only the returned lags (its crop of ``x`` is a no-op, utility.py:64-67); its transform of length
2 * 2^floor(log2 n) over all n samples is then CIRCULAR for lags k > 2 * 2^floor(log2 n) - n, where products of the chain's head
with its tail enter.  This module computes the linear sums above at every lag: it equals the reference wherever the reference's
transform does not wrap (always with fast=False), and departs from it where it does.
"""
import numpy as np


def lag_count(n, window=50, fast=False):
    """K: the lags 0 .. K-1 that enter tau."""
    n, window = int(n), int(window)
    if n < 1 or window < 1:
        raise ValueError("lag_count: n >= 1 and window >= 1")
    return min(window, 1 << (n.bit_length() - 1) if fast else n)


def moments(x, mask=False):
    """``(s, m2, n_finite)`` over axis 0 in the order of the module docstring; ``n_finite`` is int64 (n without ``mask``)."""
    x = np.asarray(x, dtype=np.float64)
    n, shape = x.shape[0], x.shape[1:]
    s, m2 = np.zeros(shape), np.zeros(shape)
    with np.errstate(all="ignore"):
        if mask:
            fin = np.isfinite(x)
            nf = fin.sum(axis=0, dtype=np.int64)
            for j in range(n):
                s = np.where(fin[j], s + x[j], s)
            mean = s / nf.astype(np.float64)
            for j in range(n):
                y = x[j] - mean
                m2 = np.where(fin[j], m2 + y * y, m2)
        else:
            nf = np.full(shape, n, dtype=np.int64)
            for j in range(n):
                s = s + x[j]
            mean = s / np.float64(n)
            for j in range(n):
                y = x[j] - mean
                m2 = m2 + y * y
    return s, m2, nf


def act(x, window=50, fast=False):
    """``(tau, mean, c0)`` of every series along axis 0, in the order of the module docstring."""
    x = np.asarray(x, dtype=np.float64)
    n, shape = x.shape[0], x.shape[1:]
    K = lag_count(n, window, fast)
    s = np.zeros(shape)
    for j in range(n):
        s = s + x[j]
    with np.errstate(all="ignore"):
        mean = s / np.float64(n)
        y = x - mean
        c = np.zeros((K,) + shape)
        for j in range(n):                     # sample j closes one product of every lag k <= j: y_{j-k} y_j, j ascending per lag
            m = min(j, K - 1)
            c[:m + 1] += y[j] * y[j - m:j + 1][::-1]
        r = np.zeros(shape)
        for k in range(1, K):
            r = r + c[k] / c[0]
        tau = 1.0 + 2.0 * r
    return tau, mean, c[0].copy()


def get_integrated_act(x, axis=0, window=50, fast=False, average=True):
    """The reference's function of the same name (utility.py:79-144) on ``act``: ``x`` a dict name -> [nsteps, ntemps, nwalkers,
    nleaves_max, ndim] (returned per name: [ntemps, nleaves_max * ndim], or [ntemps, nwalkers, ...] with ``average=False``) or one
    array with the steps first."""
    if axis != 0:
        raise NotImplementedError
    if isinstance(x, dict):
        out = {}
        for name, v in x.items():
            v = np.asarray(v)
            tau = act(v.reshape(v.shape[:3] + (-1,)), window, fast)[0]
            out[name] = np.average(tau, axis=1) if average else tau
        return out
    if not isinstance(x, np.ndarray):
        raise ValueError("x must be dictionary of np.ndarrays or an np.ndarray.")
    tau = act(x, window, fast)[0]
    if tau.ndim == 0:
        return float(tau)
    return np.average(tau, axis=1) if average else tau


# ---- Gelman-Rubin -----------------------------------------------------------------------------------------------------------
def _pool(a, b):
    """Chan's pairwise update of (n, mean, m2): group ``b`` joins group ``a``."""
    (na, ma, qa), (nb, mb, qb) = a, b
    n = na + nb
    d = mb - ma
    return n, ma + d * (nb / n), qa + qb + d * d * (na * nb / n)


def third_split(nwalkers, nsteps):
    """``(n, q, r)``: the reference compares the first and last n = floor(W S / 3) rows of the walker-major flattening
    (utility.py:310-318) - q whole walkers and r steps of one more at each end."""
    n = (int(nwalkers) * int(nsteps)) // 3
    return (n,) + divmod(n, int(nsteps))


def psrf_from_moments(nsteps, s, m2, head=None, tail=None, per_walker=False):
    """Rhat[ndim] from per-(walker, coordinate) ``s`` / ``m2`` [W, ndim] over the ``nsteps`` kept steps.  ``per_walker=False`` also
    takes ``head`` / ``tail``: the same pair over the first / last r kept steps (``third_split``; unused where r = 0).  Groups are
    pooled in row order with Chan's update, variances use ddof = 1."""
    s, m2 = np.asarray(s, dtype=np.float64), np.asarray(m2, dtype=np.float64)
    W, S = s.shape[0], int(nsteps)
    with np.errstate(all="ignore"):
        if per_walker:
            nn = S
            groups = [(S, s[w] / np.float64(S), m2[w]) for w in range(W)]
        else:
            nn, q, r = third_split(W, S)
            zero = (0, np.zeros(s.shape[1:]), np.zeros(s.shape[1:]))
            first = [(S, s[w] / np.float64(S), m2[w]) for w in range(q)]
            last = [(S, s[w] / np.float64(S), m2[w]) for w in range(W - q, W)]
            if r:
                first = first + [(r, head[0][q] / np.float64(r), head[1][q])]
                last = [(r, tail[0][W - 1 - q] / np.float64(r), tail[1][W - 1 - q])] + last
            groups = []
            for part in (first, last):
                g = part[0] if part else zero
                for b in part[1:]:
                    g = _pool(g, b)
                groups.append(g)
        m = len(groups)
        Wm, tbb = 0.0, 0.0
        for _, mean, q2 in groups:
            Wm = Wm + q2 / np.float64(nn - 1)
            tbb = tbb + mean
        Wm, tbb = Wm / np.float64(m), tbb / np.float64(m)
        B = 0.0
        for _, mean, _q in groups:
            B = B + (tbb - mean) ** 2
        B = np.float64(nn) / np.float64(m - 1) * B
        var = np.float64(nn - 1) / np.float64(nn) * Wm + B / np.float64(nn)
        return np.sqrt(var / Wm)


def psrf(C, ndims, per_walker=False):
    """The reference's function of the same name (utility.py:279-330): ``C`` [nwalkers, nsteps, ndim]."""
    x = np.asarray(C, dtype=np.float64).reshape(C.shape[0], C.shape[1], ndims).transpose(1, 0, 2)
    S, W = x.shape[:2]
    s, m2, _ = moments(x)
    head = tail = None
    if not per_walker:
        r = third_split(W, S)[2]
        if r:
            head, tail = moments(x[:r])[:2], moments(x[S - r:])[:2]
    return psrf_from_moments(S, s, m2, head, tail, per_walker)


# ---- reversible-jump chains: leaf counts and the projection through the leaf masks ------------------------------------------
# The device twins are csrc/hens_rj_chain_stats.h: k_rj_chain_leaves, k_rj_chain_leaf_moments.  The reference projects a branch of
# several leaves onto its model dimension before ``psrf`` (backends/backend.py:786-799): per walker the leaves in use in ascending
# (step, slot), the first ``min_leaves`` of them, min_leaves the smallest total over the walkers.  That is a COMPACTED series per
# (rung, walker, parameter), and the moments of it - and of its first / last r samples, ``third_split(W, min_leaves)`` - are all
# ``psrf_from_moments`` needs.
def leaf_counts(inds):
    """``(nleaves[S, Ts, W] uint8, hist[Ts, W, nl + 1] uint32)`` of masks ``inds`` bool ``[S, Ts, W, nl]``: leaves in use per step,
    and at how many steps place (t, w) has k leaves in use.  Integers: exact whatever the order."""
    inds = np.asarray(inds, dtype=bool)
    nl = inds.shape[-1]
    nleaves = inds.sum(axis=-1, dtype=np.uint8)
    hist = np.zeros(inds.shape[1:3] + (nl + 1,), dtype=np.uint32)
    for k in range(nl + 1):
        hist[..., k] = (nleaves == k).sum(axis=0)
    return nleaves, hist


def leaf_totals(hist):
    """Leaves in use over the kept steps per place, ``sum_k k hist[..., k]`` (int64)."""
    hist = np.asarray(hist)
    return (hist.astype(np.int64) * np.arange(hist.shape[-1], dtype=np.int64)).sum(axis=-1)


def leaf_moments(x, inds, lo, hi):
    """``(s, m2)`` ``[Ts, W, nd]`` and ``n[Ts, W]`` (int64) of the compacted series of every (rung, walker, parameter):
    ``x[j, t, w, slot, d]`` over the leaves in use (``inds[j, t, w, slot]``) in ascending (j, slot), those whose ordinal among
    the place's leaves in use lies in ``[lo, hi)``.  The module docstring's order on that series: ``s`` sequential from 0.0,
    ``m2`` a second sequential pass about ``s / n``; ``n`` counts the samples that entered (hi - lo unless the place runs out of
    leaves; n = 0: mean = 0 / 0, m2 = 0)."""
    x, inds = np.asarray(x, dtype=np.float64), np.asarray(inds, dtype=bool)
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi:
        raise ValueError("leaf_moments: 0 <= lo < hi")
    S, nl = x.shape[0], x.shape[3]
    place = x.shape[1:3]
    s, m2, n = np.zeros(place + x.shape[4:]), np.zeros(place + x.shape[4:]), np.zeros(place, dtype=np.int64)

    def walk(f):
        ordinal = np.zeros(place, dtype=np.int64)
        for j in range(S):
            for slot in range(nl):
                used = inds[j, :, :, slot]
                f(used & (ordinal >= lo) & (ordinal < hi), x[j, :, :, slot, :])
                ordinal = ordinal + used

    def add(take, v):
        nonlocal s, n
        s = np.where(take[..., None], s + v, s)
        n = n + take

    def add_centred(take, v):
        nonlocal m2
        y = v - mean
        m2 = np.where(take[..., None], m2 + y * y, m2)

    with np.errstate(all="ignore"):
        walk(add)
        mean = s / n.astype(np.float64)[..., None]
        walk(add_centred)
    return s, m2, n


def rj_min_leaves(totals, per_walker=False, branch=None, rung=None):
    """``M``: the smallest per-walker total ``totals[W]`` - what the reference's projection keeps of every walker.  ValueError
    where the reference has nothing defined: floor(W M / 3) < 2 (``per_walker``: M < 2) leaves ``psrf`` a group of fewer than two
    samples, and at 0 its ``C[-0:]`` is the whole array."""
    totals = np.asarray(totals)
    W, M = totals.shape[0], int(totals.min())
    if (M < 2) if per_walker else ((W * M) // 3 < 2):
        where = "" if branch is None else f" of branch {branch!r}" + ("" if rung is None else f", rung {rung}")
        raise ValueError(f"Gelman-Rubin{where}: the walker with the fewest leaves in use has {M} over the kept steps, too few to compare "
                         + ("a walker's chain" if per_walker else f"thirds of {W} walkers' chains"))
    return M


def rj_psrf(x, inds, ndim, per_walker=False, branch=None, rung=None):
    """Rhat[ndim] of one branch and rung of a reversible-jump chain, ``x`` ``[S, W, nl, nd]`` with masks ``inds`` ``[S, W, nl]``: the
    reference's projection (backends/backend.py:779-799) and ``psrf``.  One leaf: the chain as it lies, NaN included."""
    x, inds = np.asarray(x, dtype=np.float64), np.asarray(inds, dtype=bool)
    if x.shape[3] != ndim:
        raise ValueError("rj_psrf: x is [S, W, nl, ndim]")
    W = x.shape[1]
    if x.shape[2] == 1:
        return psrf(x[:, :, 0, :].transpose(1, 0, 2), ndim, per_walker)
    x, inds = x[:, None], inds[:, None]
    M = rj_min_leaves(leaf_totals(leaf_counts(inds)[1])[0], per_walker, branch, rung)
    s, m2, n = leaf_moments(x, inds, 0, M)
    assert (n == M).all()
    head = tail = None
    r = 0 if per_walker else third_split(W, M)[2]
    if r:
        head, tail = leaf_moments(x, inds, 0, r), leaf_moments(x, inds, M - r, M)
        head, tail = (head[0][0], head[1][0]), (tail[0][0], tail[1][0])
    return psrf_from_moments(M, s[0], m2[0], head, tail, per_walker)


# ---- thermodynamic integration ----------------------------------------------------------------------------------------------
def rung_means(s, n_finite):
    """Mean log-likelihood per rung from masked ``moments`` [ntemps, W]: sum_w s / sum_w n_finite, w sequential."""
    s, n_finite = np.asarray(s, dtype=np.float64), np.asarray(n_finite)
    tot, cnt = np.zeros(s.shape[0]), np.zeros(s.shape[0], dtype=np.int64)
    for w in range(s.shape[1]):
        tot = tot + s[:, w]
        cnt = cnt + n_finite[:, w]
    with np.errstate(all="ignore"):
        return tot / cnt.astype(np.float64)


def _trapz(y, x):
    a = 0.0
    for i in range(len(x) - 1):
        a = a + (x[i + 1] - x[i]) * (y[i + 1] + y[i]) / 2.0
    return a


def thermodynamic_integration_log_evidence(betas, logls):
    """``(logZ, dlogZ)``: trapezoids of the rung means over the ladder in descending beta, with the hottest mean repeated at
    beta = 0 where the ladder does not reach it; the error is the difference to the same rule on every second rung
    (utility.py:147-212, from ptemcee)."""
    betas, logls = np.asarray(betas, dtype=np.float64), np.asarray(logls, dtype=np.float64)
    if len(betas) != len(logls):
        raise ValueError("Need the same number of log(L) values as temperatures.")
    order = np.argsort(betas)[::-1]
    betas, logls = betas[order], logls[order]
    if betas[-1] != 0.0:
        betas2, logls2 = np.concatenate((betas[::2], [0.0])), np.concatenate((logls[::2], [logls[-1]]))
        betas, logls = np.concatenate((betas, [0.0])), np.concatenate((logls, [logls[-1]]))
    else:
        betas2, logls2 = np.concatenate((betas[:-1:2], [0.0])), np.concatenate((logls[:-1:2], [logls[-1]]))
    logZ, logZ2 = -_trapz(logls, betas), -_trapz(logls2, betas2)
    return logZ, np.abs(logZ - logZ2)
