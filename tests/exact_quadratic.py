"""The yardstick of tests/test_hip_likelihood_accuracy.py: the log-likelihoods of the fixed-dimension stepping kernels (dense and
diagonal Gaussian, Rosenbrock) computed exactly from the doubles the device receives, an a-priori bound on the error of ANY plain
float64 evaluation of the same formula, and problem families on which the float64 oracle cannot referee (host only, NumPy).

``exact_log_like`` evaluates, in ``np.longdouble`` where that has eps < 1e-18 and with mpmath at 40 digits otherwise
(tests/exact_template.backend's rule; neither: it fails loudly),
  dense      -1/2 sum_i sum_k d_i A_ik d_k,  d = x - mu  (plain A, also when it is not symmetric)
  diagonal   -1/2 sum_i d_i^2 p_i
  Rosenbrock -sum_i (b (x_{i+1} - x_i^2)^2 + (a - x_i)^2)
``exact_rational`` evaluates one walker in exact rational arithmetic (every input is a dyadic rational): the check of the check.

``float64_bound`` is B per walker, with u = 2^-53 the unit roundoff.  It is derived from the formulas below, not measured, and it
is not widened to make a test pass.

Dense.  With S = 1/2 sum_i sum_k |d_i| |A_ik| |d_k|,

    B = u (2 D + 16) S + D^2 2^-1074 max(1, max_i |d_i|).

Every form the device or the oracle uses is a sum of the D^2 terms d_i A_ik d_k (or of the D (D + 1) / 2 packed terms
d_i (A_ik + A_ki) d_k), and a term meets, to first order, one relative rounding u for each of
  * the two centrings fl(x_i - mu_i), fl(x_k - mu_k) - the exact value keeps d exact;
  * the packing fl(A_ik + A_ki) of the symmetric forms (relative to |A_ik + A_ki| <= |A_ik| + |A_ki|, which is what S holds);
  * at most two product roundings (fma(c, d_k, y) has none of its own; the oracle's NumPy products have two);
  * every partial sum the term is part of.  Inner chain y_i = sum_k M_ik d_k: at most D partial sums - the generic kernel's
    row (D FMAs), sym_quad's row from its diagonal rightwards (D - p), the blocked VALU form's block row (D / 4), the matrix
    pipe's accumulator over the column blocks J >= I of a row block (16 per block product, four per MFMA step: at most D;
    like_tile_mf128 splits a row block's steps over two waves, which only shortens it).  Outer chain sum_i d_i y_i: the generic
    kernel and like_partial deal rows to waves, at most D FMAs into ``part`` (sym_quad: two per row pair; the blocked form: D / 4
    rows of a cross block, or two diagonal blocks of D / 8 pairs and one add); the matrix-pipe forms dot the accumulator's four
    rows with q_I in four FMAs per row block - a wave meets at most two row blocks at D = 32 / 64 and three at D = 128, so 12 - and
    add the four 16-lane rows in two steps (sum_rows_f64): 14 <= D.  Phase D then adds at most eight wave parts and multiplies by
    -1/2 exactly.  Depth: D + D + 8.
  So a term carries at most 5 + 2 D + 8 roundings; the exact value's own rounding to double is one more (2 D + 14), and the
  constant 2 D + 16 leaves the second-order terms ((1 + u)^(2 D + 14) - 1 <= (2 D + 15) u for D <= 2^40) and one spare.  No form
  needed a larger constant.  NumPy's oracle (a matrix product, an elementwise product, a pairwise sum) has chains of at most D
  and D as well.
  Underflow: a product or FMA whose result is subnormal adds at most 2^-1075 absolute instead of a relative rounding (sums and
  differences of doubles are exact there).  There are at most D^2 inner and D outer ones; an inner one is scaled by |d_i| on
  its way out, and the final halving can round once more: (D^2 max(1, max|d|) + D + 1) 2^-1075 <= D^2 2^-1074 max(1, max|d|).

Diagonal.  S = 1/2 sum_i d_i^2 p_i = |L*|, and B = u (D + 16) S + D 2^-1074 max(1, max_i |d_i|): a term meets the centring twice
  (d_i enters squared), the product fl(d_i p_i), the FMA into ``part`` (a chain of at most D rows per wave), at most eight wave
  parts, and the exact value's rounding: 3 + D + 8 + 1 = D + 12.

Rosenbrock.  With t1_i = x_{i+1} - x_i^2, t2_i = a - x_i and R = sum_i (b t1_i^2 + t2_i^2) = |L*|,

    B = u (2 b sum_i |t1_i| x_i^2  +  (D + 16) R) + D 2^-1074 max(1, b).

  t1 evaluated WITHOUT a fused multiply-add is fl(x_{i+1} - fl(x_i^2)): off by at most u x_i^2 + u |t1| - on the valley
  x_{i+1} = x_i^2 the first part is all there is, and it is what the term 2 b |t1| (u x_i^2) carries into b t1^2.  With a fused
  multiply-add t1 has the single rounding u |t1|, which is less: the bound holds for both.  Beyond that b t1^2 meets 2 (from
  t1, squared) + 2 (the square, the product with b) roundings, t2^2 2 + 1, their sum one, the running sum at most D - 1 (the
  generic kernel's single wave; the fast kernels deal contiguous runs to the waves), at most eight wave parts (the doubling and
  the final -1/2 are exact), and the exact value's rounding: at most 5 + (D - 1) + 8 + 1 = D + 13.  Underflow: t1^2 and t2^2 can
  be subnormal, D terms each scaled by at most max(1, b).
"""
from fractions import Fraction

import numpy as np

from oracle import eryn_oracle as orc
from tests.exact_template import LD, backend

U = 2.0 ** -53
TINY = 2.0 ** -1074
ROSEN_A, ROSEN_B = 1.0, 100.0
DENSE_FAMILIES = ("equicorr", "spectrum", "scaled")
FAMILIES = DENSE_FAMILIES + ("diag_scaled", "rosen_valley")
WIDTHS = (5, 8, 16, 32, 64, 128)


# ---- arithmetic of the backend -------------------------------------------------------------------------------------------------------
def _conv(v, use=None):
    """float64 array -> the backend's numbers (long double array, or object array of mpmath numbers at 40 digits)."""
    use = use or backend()
    v = np.asarray(v, dtype=np.float64)
    if use == "longdouble":
        return v.astype(LD)
    import mpmath
    mpmath.mp.dps = max(mpmath.mp.dps, 40)
    return np.frompyfunc(lambda t: mpmath.mpf(float(t)), 1, 1)(v)


def _f64(v):
    return np.asarray(v).astype(np.float64)


def _quantities(problem, x, use=None):
    """(L*, the bound's first-order sum already times its constant, the underflow term, S) per walker, in the backend's numbers."""
    x2 = np.asarray(x, dtype=np.float64).reshape(-1, problem.D)
    xl = _conv(x2, use)
    D = problem.D
    if problem.like_kind == "rosen":
        x0, x1 = xl[:, :-1], xl[:, 1:]
        t1, t2 = x1 - x0 * x0, _conv(ROSEN_A, use) - x0
        b = _conv(ROSEN_B, use)
        terms = b * t1 * t1 + t2 * t2
        R = terms.sum(axis=1)
        first = U * (2 * b * (np.abs(t1) * x0 * x0).sum(axis=1) + (D + 16) * R)
        return -R, first, _under(D * max(1.0, ROSEN_B), np.ones(x2.shape[0]), use), R
    d = xl - _conv(problem.mu, use)
    da = np.abs(d)
    dmax = np.maximum(_f64(da).max(axis=1), 1.0)
    if problem.like_kind == "diag":
        p = _conv(problem.precision, use)
        S = (d * d * p).sum(axis=1) / 2
        return -S, U * (D + 16) * ((da * da * np.abs(p)).sum(axis=1) / 2), _under(D, dmax, use), (da * da * np.abs(p)).sum(axis=1) / 2
    A = _conv(problem.precision, use)
    L = -((d @ A.T) * d).sum(axis=1) / 2
    S = ((da @ np.abs(A).T) * da).sum(axis=1) / 2
    return L, U * (2 * D + 16) * S, _under(D * D, dmax, use), S


def _under(count, dmax, use):
    """count 2^-1074 max(1, max|d|), in the backend's numbers (2^-1074 D^2 is still a double: a subnormal one)."""
    return _conv(dmax, use) * _conv(float(count), use) * _conv(TINY, use)


def exact_log_like(problem, x, use=None):
    """L* per walker (``x[..., D]`` flattened to [N, D]), in the backend's numbers."""
    return _quantities(problem, x, use)[0]


def float64_bound(problem, x, use=None):
    """B per walker (module docstring), in the backend's numbers: at 1e-160 sigma B is far below the smallest normal double."""
    _, first, under, _ = _quantities(problem, x, use)
    return first + under


def yardstick(problem, x, use=None):
    """(L*, B, S / |L*| as float64 - inf where L* is 0) per walker of ``x[..., D]``, flattened."""
    L, first, under, S = _quantities(problem, x, use)
    La = _f64(np.abs(L))
    with np.errstate(divide="ignore", invalid="ignore"):
        canc = np.where(La > 0, _f64(S) / La, np.inf)
    return L, first + under, canc


def error_ratio(Lf, Ls, B, use=None):
    """|Lf - L*| / B per walker as float64: 0 where both vanish, inf where B does and the error does not, or where Lf is not finite."""
    Lf = np.asarray(Lf, dtype=np.float64).reshape(-1)
    fin = np.isfinite(Lf)
    err = np.abs(_conv(np.where(fin, Lf, 0.0), use) - Ls)
    out = np.zeros(Lf.shape)
    pos = np.asarray(B > 0, dtype=bool)
    out[pos] = _f64(err[pos] / B[pos])
    out[~pos & np.asarray(err > 0, dtype=bool)] = np.inf
    out[~fin] = np.inf
    return out


def exact_rational(problem, x_row):
    """L* of one walker as a Fraction."""
    x = [Fraction(float(v)) for v in np.asarray(x_row, dtype=np.float64)]
    D = problem.D
    if problem.like_kind == "rosen":
        a, b = Fraction(ROSEN_A), Fraction(ROSEN_B)
        return -sum(b * (x[i + 1] - x[i] * x[i]) ** 2 + (a - x[i]) ** 2 for i in range(D - 1))
    d = [x[i] - Fraction(float(problem.mu[i])) for i in range(D)]
    if problem.like_kind == "diag":
        return -sum(d[i] * d[i] * Fraction(float(problem.precision[i])) for i in range(D)) / 2
    A = problem.precision
    tot = Fraction(0)
    for i in range(D):
        tot += d[i] * sum(Fraction(float(A[i, k])) * d[k] for k in range(D))
    return -tot / 2


def to_fraction(v):
    """A number of the backend as a Fraction, exactly."""
    if isinstance(v, (np.floating, float)):
        m, e = np.frexp(LD(v))
        return Fraction(int(np.ldexp(m, 64))) * Fraction(2) ** (int(e) - 64)
    import mpmath
    sign, man, exp, _ = mpmath.mpf(v)._mpf_
    return (-1 if sign else 1) * Fraction(int(man)) * Fraction(2) ** int(exp)


# ---- problem families ----------------------------------------------------------------------------------------------------------------
class Problem:
    """What tests/problems.Problem gives (mu, precision [D, D] | [D] | None, lo, hi, like_kind, loglike, x0) plus ``sigma`` [D],
    ``draw(z)`` - a draw from the target for standard normals z[..., D], from the covariance's closed form - and ``cov`` (dense)."""
    pinned, period = {}, None

    def __init__(self, family, D, like_kind, mu, precision, sigma, draw, cov=None, box=1e4, seed=0):
        self.family, self.D, self.like_kind, self.seed = family, D, like_kind, seed
        self.mu, self.precision, self.sigma, self.draw, self.cov = mu, precision, sigma, draw, cov
        self.lo, self.hi = mu - box * sigma, mu + box * sigma

    def loglike(self, x):
        if self.like_kind == "dense":
            return orc.gaussian_log_like(x, self.mu, self.precision)
        if self.like_kind == "diag":
            return orc.gaussian_diag_log_like(x, self.mu, self.precision)
        return orc.rosenbrock_log_like(x)

    def x0(self, T, W):
        """Draws from the target; a seeded third of the rows at 1e-3 of its displacement from mu and a third at 3 times it."""
        rs = np.random.RandomState(4000 + 17 * self.seed + self.D)
        if self.like_kind == "rosen":
            return rosen_valley_walkers(self.D, T, W, rs)
        z = rs.randn(T, W, self.D)
        scale = np.array([1e-3, 1.0, 3.0])[rs.permutation(T * W) % 3].reshape(T, W, 1)
        return self.mu + self.draw(z) * scale


def rosen_valley_walkers(D, T, W, rs):
    """Walker w mod 8: 0 - the point (1, ..., 1); 1 - exactly on the valley x_{i+1} = fl(x_i^2) from x_0 in [-1, 1] (it runs down to 0
    through the subnormals at D = 128); 2 .. 6 - the valley restarted every fourth coordinate from (-1.2, 1.2), every x_{i+1} off
    x_i^2 by 3 ulps, 1e-12, 1e-9, 1e-6, 1e-3 relative, either side; 7 - the suite's usual uniform start in the 3 ... 6 box's
    inner part (tests/problems.py)."""
    x = np.empty((T, W, D))
    off = [0.0, 0.0, 3 * 2.0 ** -52, 1e-12, 1e-9, 1e-6, 1e-3]
    for t in range(T):
        for w in range(W):
            k = w % 8
            if k == 0:
                x[t, w] = 1.0
            elif k == 7:
                x[t, w] = 0.9 * rs.uniform(-1.0, 1.0, D)
            else:
                v = np.empty(D)
                for i in range(D):
                    if i == 0 or (k >= 2 and i % 4 == 0):
                        v[i] = rs.uniform(-1.0, 1.0) if k == 1 else rs.uniform(-1.2, 1.2)
                    else:
                        v[i] = v[i - 1] * v[i - 1] * (1.0 + off[k] * rs.choice([-1.0, 1.0]))
                x[t, w] = v
    return x


def _benign(D):
    rs = np.random.RandomState(0)                    # parity_utils.gaussian_problem's matrix
    A = rs.randn(D, D)
    return A @ A.T / D + np.eye(D)


def make_problem(family, D, seed=0, edge=False):
    """``edge``: the family centred on mu = 0 under a box of +- 1e120 sigma (eval_state's edge set: 1e-160 sigma and 1e100 sigma
    are positions only around a zero mean, and only inside such a box)."""
    rs = np.random.RandomState(911 + 31 * seed + D)
    box = 1e120 if edge else 1e4
    if family == "rosen_valley":
        p = Problem(family, D, "rosen", np.zeros(D), None, np.ones(D), None, box=20.0, seed=seed)
        return p
    if family == "equicorr":
        rho = 1.0 - 2.0 ** -20
        cov = (1.0 - rho) * np.eye(D) + rho * np.ones((D, D))
        prec = (np.eye(D) - rho / (1.0 + (D - 1) * rho) * np.ones((D, D))) / (1.0 - rho)
        Lc = np.linalg.cholesky(cov)
        draw, sigma, m = (lambda z: z @ Lc.T), np.ones(D), rs.randn(D)
    elif family == "spectrum":
        Q, _ = np.linalg.qr(rs.randn(D, D))
        lam = 10.0 ** np.linspace(-5.0, 5.0, D)
        cov = (Q * lam) @ Q.T
        prec = (Q / lam) @ Q.T
        prec = 0.5 * (prec + prec.T)
        root = Q * np.sqrt(lam)
        draw, sigma, m = (lambda z: z @ root.T), np.sqrt(np.diag(cov)), rs.randn(D)
    elif family in ("scaled", "diag_scaled"):
        s = 10.0 ** rs.permutation(np.linspace(-6.0, 6.0, D))
        m = 10.0 ** rs.uniform(3.0, 6.0, D) * rs.choice([-1.0, 1.0], D)
        if family == "scaled":
            cov0 = _benign(D)
            cov = cov0 * np.outer(s, s)
            prec = np.linalg.inv(cov0) / np.outer(s, s)          # (the benign matrix: condition number below 10)
            Lc = np.linalg.cholesky(cov0)
            draw, sigma = (lambda z: (z @ Lc.T) * s), s * np.sqrt(np.diag(cov0))
        else:
            cov, prec, sigma = None, 1.0 / (s * s), s
            draw = lambda z: z * s
    else:
        raise KeyError(family)
    mu = np.zeros(D) if edge else m * sigma
    kind = "diag" if family == "diag_scaled" else "dense"
    return Problem(family, D, kind, mu, prec, sigma, draw, cov=cov, box=box, seed=seed)


def families_of(like):
    return {"dense": DENSE_FAMILIES, "diag": ("diag_scaled",), "rosen": ("rosen_valley",)}[like]


def edge_walkers(problem, n_each=None):
    """eval_state's extra edge set for a Gaussian ``make_problem(..., edge=True)``: [3 n_each + 1, D] - walker 0 exactly on mu, then
    draws at 1e-160 sigma (every product underflows: B's 2^-1074 term covers them), at 1e100 sigma, and ordinary ones.  n_each:
    max(24, D) unless given (the engine wants 2 D walkers)."""
    n_each = max(24, problem.D) if n_each is None else n_each
    rs = np.random.RandomState(77 + problem.D)
    z = problem.draw(rs.randn(3 * n_each, problem.D))
    scale = np.repeat([1e-160, 1e100, 1.0], n_each)[:, None]
    return np.concatenate([problem.mu[None, :], problem.mu + z * scale])


# ---- two pure-NumPy models of a wrong kernel -----------------------------------------------------------------------------------------
def model_expanded(problem, x):
    """q^T A q - 2 mu^T A q + mu^T A mu in float64: the centring left to the end."""
    A, mu = problem.precision, problem.mu
    return -0.5 * (((x @ A.T) * x).sum(axis=1) - 2.0 * (x @ (A.T @ mu)) + mu @ A @ mu)


def model_float32_block(problem, x):
    """The float64 form with the first 16 x 16 diagonal block's product carried in float32."""
    A, d = problem.precision, x - problem.mu
    full = ((d @ A.T) * d).sum(axis=1)
    blk64 = ((d[:, :16] @ A[:16, :16].T) * d[:, :16]).sum(axis=1)
    d32 = d[:, :16].astype(np.float32)
    blk32 = ((d32 @ A[:16, :16].astype(np.float32).T) * d32).sum(axis=1).astype(np.float64)
    return -0.5 * (full - blk64 + blk32)


# ---- the device paths of tests/test_hip_likelihood_accuracy.py, sized without a GPU by tests/test_exact_quadratic.py -------------------
# (row width, pad_rows): the generic kernel at 5 and 12, rows padded to 16 / 32 / 128, every compile-time width
EVAL_WIDTHS = [(5, False), (12, False), (11, True), (20, True), (70, True), (8, True), (16, True), (32, True), (64, True), (128, True)]
MH_WIDTHS = (16, 32, 128)
PARITY_T = 2


def parity_walkers(D):
    """W of the eval_state / stretch_split / mh_step cases: more than two 64-walker tiles with a ragged last one, sets of unequal
    size, and at least 2 D walkers (the engine refuses a red-blue move on fewer)."""
    return max(165, 2 * D + 37)


# tests/problems.CASES entry -> the likelihood kinds it runs on here (its own kind first)
PRODUCTION = [("two_launch_D8", "dense"), ("two_launch_D16_two_word_masks", "dense"), ("two_launch_D32_config2", "dense"),
              ("two_launch_D64", "dense"), ("two_launch_D128", "dense"), ("short_tiles_T10_D64", "dense"), ("one_launch_D16", "dense"),
              ("one_launch_D32", "diag"), ("one_launch_D32", "dense"), ("tile2_forced_ragged_D64", "dense"), ("three_launch_D32", "dense"),
              ("padded_D11", "dense"), ("padded_D70", "dense"), ("generic_D5", "dense"), ("generic_D12", "diag"), ("untempered_D16", "dense"),
              ("mh_full_D16", "dense"), ("mh_iso_D32", "dense"), ("rosenbrock_D32", "rosen"), ("rosenbrock_D128", "rosen")]
STEPS = (1, 5)                       # step(1) from L = -1e300 (every walker accepts), then step(5)


def production_cases():
    """[(id, tests/problems.CASES name, likelihood kind, family)]: every dense case on every dense family.  The two Metropolis-
    Hastings cases take their shapes from mh_full_D16 / mh_iso_D32 and mix in the FULL factor (chol of 0.02 Sigma) at weight 0.5."""
    out = []
    for name, like in PRODUCTION:
        for fam in families_of(like):
            tag = name.replace("mh_iso_D32", "mh_full_D32") + ("" if like == "dense" or name.startswith("rosen") else f"_{like}")
            out.append((f"{tag}-{fam}", name, like, fam))
    return out


def mh_factor(problem):
    """Lower Cholesky factor of 0.02 Sigma, Sigma from its closed form."""
    cov = problem.cov if problem.cov is not None else np.diag(problem.sigma ** 2)
    return np.linalg.cholesky(0.02 * cov)


def stretch_draws(rs, T, W, nsplits=2):
    """One iteration's draws in the reference's own form (red_blue.py:119-124, stretch.py:93-132, tempering.py:526-541)."""
    d = dict(labels=np.stack([rs.permutation(np.arange(W) % nsplits) for _ in range(T)]))
    for k in range(nsplits):
        Ns = (W - k + nsplits - 1) // nsplits
        d[f"rint{k}"] = rs.randint(W - Ns, size=(T, Ns))
        d[f"u_zz{k}"] = rs.rand(T, Ns)
        d[f"u_acc{k}"] = rs.rand(T, Ns)
    if T > 1:
        d["iperm"] = np.stack([rs.permutation(W) for _ in range(T - 1)])
        d["i1perm"] = np.stack([rs.permutation(W) for _ in range(T - 1)])
        d["u_swap"] = rs.rand(T - 1, W)
    return d
