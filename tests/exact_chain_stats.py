"""The yardstick of tests/test_chain_stats.py and tests/test_hip_chain_stats.py: the chain diagnostics of eryn_amd/chain_stats.py
evaluated in ``np.longdouble`` on the same doubles, and an a-priori bound B on the error of ANY float64 evaluation of the direct
form (any summation order, with or without fused multiply-adds).  B is derived below, not measured, and is not widened to make a
test pass.  Host only, NumPy.

One series x_0 .. x_{n-1}.  Exact: mu = sum x / n, y_j = x_j - mu, c_k = sum_{j < n-k} y_j y_{j+k}, m2 = c_0,
tau = 1 + 2 sum_{k=1}^{K-1} c_k / c_0.  u = 2^-53, g(m) = m u / (1 - m u), A = sum |x_j| / n.

Sum and mean.  n - 1 additions in any order and the exact value's own rounding to double: |s~ - s| <= g(n) sum |x_j| = B_sum.  One
division more: |mean~ - mu| <= g(n + 1) A = B_mean.

Centred values.  y~_j = fl(x_j - mean~) is a ROUNDED subtraction of a ROUNDED mean:
    |y~_j - y_j| <= B_mean + u (|x_j| + |mean~|) <= B_mean + u (|x_j| + A + B_mean) = e_j.
Both parts grow with the chain's distance from 0, not with its spread: on a chain 10^6 sigma from 0 they are 10^6 u sigma and more.

Lag sums.  c~_k adds n - k rounded products (a fused multiply-add drops the product's rounding, which only helps):
    |c~_k - sum y~_j y~_{j+k}| <= g(n + 1) sum_j |y~_j| |y~_{j+k}|                                  (accumulation, + the exact
                                                                                                      value's rounding)
    |sum y~_j y~_{j+k} - c_k|  <= sum_j (|y_j| e_{j+k} + e_j |y_{j+k}| + e_j e_{j+k})                 (centring and mean)
so with a_j = |y_j| + e_j
    B_c(k) = g(n + 1) sum_j a_j a_{j+k}  +  sum_j (|y_j| e_{j+k} + e_j |y_{j+k}| + e_j e_{j+k}),       B_m2 = B_c(0).
The second sum carries the two terms that dominate far from 0: the centred values' own rounding (u (|x| + |mean|) in e_j) and the
rounded mean (B_mean in e_j).  It does not use sum y_j = 0, which would cancel the mean's FIRST-order part in c_0 but not in c_k.

tau.  With rho_k = c_k / c_0 and B_c(0) < c_0:
    |rho~_k - rho_k| <= (B_c(k) + |rho_k| B_c(0)) / (c_0 - B_c(0)) + u |rho~_k|                       (the division's rounding)
and 1 + 2 sum rho~_k is K - 2 additions, an exact doubling, one addition and the exact value's rounding:
    B_tau = 2 sum_k d_k + g(K + 2) (1 + 2 sum_k (|rho_k| + d_k)),   d_k = (B_c(k) + |rho_k| B_c(0)) / (c_0 - B_c(0)).
Where c_0 <= B_c(0) (a constant series: c_0 = 0) the ratio is not determined by the data: B_tau = inf, and what is compared
there is only that implementations of the SAME order agree, NaN with NaN.

Second-order terms ((1 + u)^m - 1 <= g(m)) are inside g.  The long double evaluation is itself off by at most 2^-11 of the
accumulation terms (eps 2^-64 against u = 2^-53): every B is multiplied by 1 + 2^-10 for it.  Masked series (log-likelihoods): the
same with n the number of finite entries and the sums over those.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
SPARE = 1.0 + 2.0 ** -10
if float(np.finfo(LD).eps) >= 1e-18:
    raise RuntimeError(f"np.longdouble has eps {float(np.finfo(LD).eps):.3g} here: the exact yardstick needs an extended type")


def g(m):
    return m * U / (1.0 - m * U)


def _seq_sum(a):
    s = np.zeros(a.shape[1:], dtype=LD)
    for j in range(a.shape[0]):
        s = s + a[j]
    return s


def exact_moments(x, mask=False):
    """``(s, m2, n_finite)`` in long double, and the bounds ``(B_sum, B_m2)`` in float64, per series along axis 0."""
    x = np.asarray(x, dtype=np.float64)
    fin = np.isfinite(x) if mask else np.ones(x.shape, dtype=bool)
    xl = np.where(fin, x, 0.0).astype(LD)
    nf = fin.sum(axis=0)
    s = _seq_sum(xl)
    with np.errstate(all="ignore"):
        mu = s / nf.astype(LD)
        y = np.where(fin, xl - mu, LD(0))
        m2 = _seq_sum(y * y)
        n = np.maximum(nf, 1).astype(np.float64)
        ax = np.abs(np.where(fin, x, 0.0))
        A = ax.sum(axis=0) / n
        b_mean = g(n + 1) * A
        e = np.where(fin, b_mean + U * (ax + A + b_mean), 0.0)
        ay = np.abs(y).astype(np.float64)
        a = ay + e
        b_m2 = g(n + 1) * (a * a).sum(axis=0) + (2 * ay * e + e * e).sum(axis=0)
    return s, m2, nf, SPARE * g(n) * ax.sum(axis=0), SPARE * b_m2


def exact_act(x, K):
    """``(tau, mean, c0)`` in long double over the lags 0 .. K-1 and the bounds ``(B_tau, B_mean, B_c0)`` in float64."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    xl = x.astype(LD)
    mu = _seq_sum(xl) / LD(n)
    y = xl - mu
    ax = np.abs(x)
    A = ax.sum(axis=0) / n
    b_mean = g(n + 1) * A
    e = b_mean + U * (ax + A + b_mean)
    ay = np.abs(y).astype(np.float64)
    a = ay + e
    c, bc = [], []
    for k in range(K):
        m = n - k
        c.append(_seq_sum(y[:m] * y[k:]))
        bc.append(g(n + 1) * (a[:m] * a[k:]).sum(axis=0) + (ay[:m] * e[k:] + e[:m] * ay[k:] + e[:m] * e[k:]).sum(axis=0))
    with np.errstate(all="ignore"):
        r = np.zeros(x.shape[1:], dtype=LD)
        d_sum, rho_sum = np.zeros(x.shape[1:]), np.zeros(x.shape[1:])
        c0 = c[0].astype(np.float64)
        for k in range(1, K):
            rho = c[k] / c[0]
            r = r + rho
            arho = np.abs(rho).astype(np.float64)
            d = (bc[k] + arho * bc[0]) / (c0 - bc[0])
            d_sum, rho_sum = d_sum + d, rho_sum + arho
        tau = 1 + 2 * r
        b_tau = 2 * d_sum + g(K + 2) * (1 + 2 * (rho_sum + d_sum))
        b_tau = np.where(c0 > bc[0], b_tau, np.inf)
    return tau, mu, c[0], SPARE * b_tau, SPARE * b_mean, SPARE * bc[0]


def within(got, exact, bound):
    """Per element: |got - exact| <= bound, NaN against NaN and anything against an infinite bound counting as inside."""
    got = np.asarray(got, dtype=np.float64)
    with np.errstate(all="ignore"):
        err = np.abs(got.astype(LD) - exact).astype(np.float64)
    both_nan = np.isnan(got) & np.isnan(np.asarray(exact, dtype=np.float64))
    return (err <= bound) | both_nan | np.isinf(bound), err


def ar1(rs, n, shape, phi=0.8, scale=1.0, offset=0.0):
    """AR(1) chains [n, *shape] of unit innovation variance times ``scale`` (broadcast over ``shape``), shifted by ``offset``."""
    x = np.empty((n,) + tuple(shape))
    v = rs.randn(*shape) / np.sqrt(1 - phi * phi)
    for j in range(n):
        v = phi * v + rs.randn(*shape)
        x[j] = v
    return x * scale + offset
