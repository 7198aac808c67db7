"""The yardstick of tests/test_hip_template_accuracy.py: template log-likelihoods computed exactly from their double inputs,
and an a-priori bound on the error of a plain float64 evaluation of the same formula.

The formula is the reference tests' one as the oracle restates it (oracle/eryn_oracle_rj.py: template_log_like): pulses
``a exp(-(t - b)^2 / (2 c^2))`` and sines ``a sin(2 pi b t + c)``, summed leaf by leaf into a branch template and branch by
branch into the template, ``L = -1/2 sum(((template - y) / sigma)^2)``.  ``pi`` is the double ``np.pi``: the exact value is
the one of the formula on the doubles the float64 code sees, not of the ideal model.

``exact_log_like`` evaluates it in ``np.longdouble`` where that has eps < 1e-18 (a 64-bit significand, as on x86 hosts: eps
1.1e-19, some 2000 times finer than double), else with mpmath at 40 digits (much slower), and fails loudly where neither is
available.  ``mp_log_like`` evaluates one walker with mpmath: the check of the check.

``float64_bound`` is B, per walker, to first order in the unit roundoff: what each rounding of a float64 evaluation can move L
(EPS = 2^-52 = two unit roundoffs; libm's / the device's exp and sin are taken as within one EPS, relative, of the true value):
  pulse value      EPS |a| e (3 + 3 arg), arg = (t - b)^2 / (2 c^2), e = exp(-arg)  (t - b, its square, c^2, the quotient: the
                   argument to 3 EPS arg; exp and the product with a: 1.5 EPS)
  sine value       EPS |a| (3 + 2 |2 pi b t| + |c|)  (the phase's three roundings; sin and the product with a)
  leaf sums        EPS n sum_j |value_j| at a point, n = active leaves + branches (the running sums of a walker)
  residual         d = template - y and d / sigma: 2 EPS |r|, r = (template - y) / sigma
  sum of squares   EPS (2 + D / 2) sum_k r_k^2, D = ceil(log2 N) + 12 (the square, and NumPy's pairwise sum - 8-way unrolled
                   blocks of 128 - or the device's eight points per lane and six butterfly steps, whichever is deeper)
and a template error dT_k moves L by |r_k| dT_k / sigma, so
  B = sum_k |r_k| (dT_k / sigma + 2 EPS |r_k|) + EPS (2 + D / 2) sum_k r_k^2 .
"""
import math

import numpy as np

from oracle import eryn_oracle_rj as orj

EPS = float(np.finfo(np.float64).eps)
LD = np.longdouble
PI = np.pi                      # the double the formula rounds 2 pi to (2 * np.pi is exact)


DPS = 40                        # mpmath digits


def backend():
    """"longdouble" where np.longdouble is much finer than double (eps < 1e-18), else "mpmath" where it imports; neither: fail
    loudly (the yardstick would measure nothing)."""
    if float(np.finfo(LD).eps) < 1e-18:
        return "longdouble"
    try:
        import mpmath  # noqa: F401
    except ImportError:
        raise RuntimeError(f"np.longdouble has eps {float(np.finfo(LD).eps):.3g} here and mpmath does not import: the exact "
                           "yardstick needs one of them") from None
    return "mpmath"


def _leaves(x, inds, branches):
    """Per branch: (kind, a, b, c, active) with a, b, c [T, W, nl] doubles."""
    out = []
    for br in branches:
        xb = np.asarray(x[br.name], dtype=np.float64)
        out.append((br.kind, xb[..., 0], xb[..., 1], xb[..., 2], np.asarray(inds[br.name], dtype=bool)))
    return out


class _Arith:
    """Elementwise arithmetic of a backend: long double arrays, or object arrays of mpmath numbers (inside mpmath.workdps)."""

    def __init__(self, name):
        if name == "longdouble":
            self.conv, self.exp, self.sin, self.zero = (lambda v: np.asarray(v, dtype=np.float64).astype(LD)), np.exp, np.sin, LD(0)
            self.scalar = lambda v: LD(float(v))
        else:
            import mpmath
            self.conv = lambda v: np.frompyfunc(lambda u: mpmath.mpf(float(u)), 1, 1)(np.asarray(v, dtype=np.float64))
            self.exp, self.sin = np.frompyfunc(mpmath.exp, 1, 1), np.frompyfunc(mpmath.sin, 1, 1)
            self.zero = mpmath.mpf(0)
            self.scalar = lambda v: mpmath.mpf(float(v))


def _template_exact(leaves, t, shape, ar):
    """The exact template [T, W, N] in the backend's numbers, and per point the sum of |leaf value| and the leaf-value bounds
    (float64)."""
    tl = ar.conv(t)
    tm = np.full(shape + (t.shape[0],), ar.zero, dtype=type(ar.zero) if isinstance(ar.zero, LD) else object)
    absv = np.zeros(shape + (t.shape[0],))
    bvals = np.zeros(shape + (t.shape[0],))
    two_pi = 2 * ar.scalar(PI)
    for kind, a, b, c, act in leaves:
        for n in range(a.shape[-1]):
            on = act[..., n][..., None]
            if not on.any():
                continue
            an = ar.conv(a[..., n][..., None])
            bn = ar.conv(b[..., n][..., None])
            cn = ar.conv(c[..., n][..., None])
            if kind == orj.KIND_PULSE:
                arg = (tl - bn) ** 2 / (2 * cn * cn)
                v = an * ar.exp(-arg)
                bv = EPS * np.abs(v.astype(np.float64)) * (3.0 + 3.0 * arg.astype(np.float64)) \
                    + np.abs(a[..., n][..., None]) * 1e-300                              # (gradual underflow of e)
            else:
                ph = two_pi * bn * tl
                v = an * ar.sin(ph + cn)
                bv = EPS * np.abs(a[..., n][..., None]) * (3.0 + 2.0 * np.abs(ph.astype(np.float64)) + np.abs(c[..., n][..., None]))
            tm = tm + np.where(on, v, ar.zero)
            absv = absv + np.where(on, np.abs(v.astype(np.float64)), 0.0)
            bvals = bvals + np.where(on, bv, 0.0)
    return tm, absv, bvals


def exact_log_like(x, inds, branches, t, y, sigma, bound_inds=None, use=None):
    """(L* [T, W], r = (template - y) / sigma [T, W, N], both in the backend's numbers, the per-point template bound dT [T, W, N]).

    ``bound_inds``: the leaves whose roundings dT counts, if not those of ``inds`` - a template updated by difference
    (template +- one leaf) still carries the roundings of a leaf that has since died.  ``use``: the backend (default: backend())."""
    use = use or backend()
    if use == "mpmath":
        import mpmath
        with mpmath.workdps(DPS):
            return _exact(x, inds, branches, t, y, sigma, bound_inds, _Arith(use))
    return _exact(x, inds, branches, t, y, sigma, bound_inds, _Arith(use))


def _exact(x, inds, branches, t, y, sigma, bound_inds, ar):
    t = np.asarray(t, dtype=np.float64)
    y = np.asarray(y, dtype=np.float64)
    leaves = _leaves(x, inds, branches)
    shape = leaves[0][1].shape[:2]
    tm, absv, bvals = _template_exact(leaves, t, shape, ar)
    if bound_inds is not None:
        leaves = _leaves(x, bound_inds, branches)
        _, absv, bvals = _template_exact(leaves, t, shape, ar)
    r = (tm - ar.conv(y)) / ar.scalar(sigma)
    L = -0.5 * np.sum(r * r, axis=-1)
    nterms = sum(act.sum(axis=-1) for _, _, _, _, act in leaves) + len(leaves)      # [T, W]
    dT = bvals + EPS * nterms[..., None] * absv
    return L, r, dT


def float64_bound(r, dT, sigma):
    """B [T, W]: the a-priori bound on |L_float64 - L*| (module docstring)."""
    ra = np.abs(r.astype(np.float64))
    N = r.shape[-1]
    D = math.ceil(math.log2(max(N, 2))) + 12
    return np.sum(ra * (dT / sigma + 2 * EPS * ra), axis=-1) + EPS * (2 + D / 2) * np.sum(ra * ra, axis=-1)


def yardstick(x, inds, branches, t, y, sigma, bound_inds=None, use=None):
    """(L* rounded to double [T, W], B [T, W])."""
    L, r, dT = exact_log_like(x, inds, branches, t, y, sigma, bound_inds, use)
    return L.astype(np.float64), float64_bound(r, dT, sigma)


def mp_log_like(x, inds, branches, t, y, sigma, tw, dps=40):
    """Walker tw = (temperature, walker) evaluated with mpmath at ``dps`` digits, as a decimal string of 35 digits (None where
    mpmath does not import)."""
    try:
        import mpmath
    except ImportError:
        return None
    with mpmath.workdps(dps):
        pi = mpmath.mpf(PI)
        tm = [mpmath.mpf(0)] * len(t)
        tv = [mpmath.mpf(float(v)) for v in t]
        for kind, a, b, c, act in _leaves(x, inds, branches):
            for n in range(a.shape[-1]):
                if not act[tw][n]:
                    continue
                an, bn, cn = (mpmath.mpf(float(v[tw][n])) for v in (a, b, c))
                for k, tk in enumerate(tv):
                    if kind == orj.KIND_PULSE:
                        tm[k] += an * mpmath.exp(-(tk - bn) ** 2 / (2 * cn * cn))
                    else:
                        tm[k] += an * mpmath.sin(2 * pi * bn * tk + cn)
        s = mpmath.mpf(sigma)
        L = -mpmath.mpf(0.5) * mpmath.fsum(((tm[k] - mpmath.mpf(float(y[k]))) / s) ** 2 for k in range(len(t)))
        return mpmath.nstr(L, 35)


# ---- the case matrix ---------------------------------------------------------------------------------------------------------
GRIDS = ["control", "offset_p1000", "offset_m1000", "wide_3e4", "tiny_1e-6", "jitter_3ulp", "jitter_5ulp"]
SIZES = [64, 65, 130, 500, 512, 513]
DATA = ["noise", "signal"]
T_CASE, W_CASE, NL = 2, 64, 6


def make_grid(name, N):
    if name == "control":
        return np.linspace(-1, 1, N)
    if name == "offset_p1000":
        return 1000 + np.linspace(0, 1, N)
    if name == "offset_m1000":
        return np.linspace(-1001, -1000, N)
    if name == "wide_3e4":
        return np.linspace(0, 3e4, N)
    if name == "tiny_1e-6":
        return np.linspace(0, 1e-6, N)
    if name.startswith("jitter_"):
        # every interior point moved by exactly k EPS max|t| up or down: k = 3 and 5 lie either side of the uniform-grid test
        # (4 EPS max|t|, hens_rj_set_model); the end points stay, so the grid step the test derives from them is linspace's
        k = int(name[len("jitter_"):-3])
        t = np.linspace(-1, 1, N)
        s = np.where(np.random.RandomState(N).rand(N) < 0.5, -1.0, 1.0)
        t[1:-1] += s[1:-1] * k * EPS
        return t
    raise KeyError(name)


def grid_is_uniform(t):
    """The uniform-grid test of hens_rj_set_model, restated: dt from the end points, every point within 4 EPS max(|t|, dt) of
    t0 + i dt (this decides whether the device evaluates a lane's eight points by recurrence / rotation, or point by point)."""
    N = t.shape[0]
    if N <= 64:
        return False
    dt = (t[-1] - t[0]) / (N - 1)
    dev = np.max(np.abs(t - (t[0] + np.arange(N) * dt)))
    return bool(dt > 0 and dev <= 4 * EPS * max(np.max(np.abs(t)), abs(dt)))


def device_form(case):
    """"uniform" where the device evaluates the case's model eight consecutive points per lane by recurrence / rotation (resident
    templates, a uniform grid, and lane positions within 128 EPS of the pulse box's narrowest width: hens_rj_set_model), else
    "strided" (an exp / sin per point)."""
    t = case["t"]
    cmin = min(abs(b.lo[2]) for b in case["branches"] if b.kind == orj.KIND_PULSE)
    ok = t.shape[0] <= 512 and grid_is_uniform(t) and lane_position_error(t) <= 128 * EPS * cmin
    return "uniform" if ok else "strided"


def r0_exponent_max(case):
    """The largest exponent of r_0 = exp(-((2 (t0 - b)) h + h^2) / (2 c^2)) that k_rj's uniform form meets: over the lanes' first
    points t0 and the active pulses with |c| >= h (the recurrence), as the kernel rounds it.  Above 700 the kernel clamps it (a
    centre far above the grid: r_0 = inf times an underflowed e_0 was NaN)."""
    t = case["t"]
    N = t.shape[0]
    h = (64.0 * ((t[-1] - t[0]) / (N - 1))) * (1.0 / 64.0)
    xb, ib = case["x"]["pulse"], case["inds"]["pulse"]
    b, c = xb[..., 1][..., None], xb[..., 2][..., None]
    v0 = 1.0 / (2 * (c * c))
    dx = t[0::8] - b
    xr = -((2 * dx) * h + h * h) * v0
    return float(np.max(np.where((ib & (np.abs(xb[..., 2]) >= h))[..., None], xr, -np.inf)))


def lane_position_error(t):
    """Largest distance between a data point t[i] and the point t[8 floor(i / 8)] + (i mod 8) h the device's uniform-grid
    recurrence evaluates in its place (h = (t[N-1] - t[0]) / (N - 1)), computed exactly."""
    from fractions import Fraction
    N = t.shape[0]
    h = Fraction((t[-1] - t[0]) / (N - 1))
    return float(max(abs(Fraction(t[i]) - Fraction(t[8 * (i // 8)]) - (i % 8) * h) for i in range(N)))


def make_case(grid, N, data, amp, sig_pow2, seed=0):
    """One model and one ensemble state: T_CASE x W_CASE walkers over a pulse branch and a sine branch of NL slots each.

    Walkers 0 - 7 hold the injected signal (high SNR when the data carry it), 8 - 15 the injection with one leaf more or less,
    the rest one leaf of every edge case each (pulse width just below h, h, 2h, 10h; centre on a grid point, between two,
    between lanes 8m - 1 | 8m, 1 to 1000 steps below or above the grid; sines from low frequency to 0.98 Nyquist, phases near 0
    and 2 pi; amplitudes from 1e-3 to 1e3) beside a few injected leaves.  Edge-case walker k (0 - 47) draws its width from k % 4,
    its centre from k // 4 % 4, its side of the grid from k // 16 % 2 and its mix of branches from (k + k // 4) % 4: every width
    meets every centre, both sides and every mix (a width h pulse 1000 steps above the grid drives the recurrence's r_0 past
    its clamp)."""
    rs = np.random.RandomState(seed * 7919 + N * 31 + GRIDS.index(grid) * 3 + DATA.index(data))
    t = make_grid(grid, N)
    h = (t[-1] - t[0]) / (N - 1)
    span = t[-1] - t[0]
    fnyq = 0.5 / h
    sigma = 1e-3 * amp
    if sig_pow2:
        sigma = 2.0 ** round(math.log2(sigma))
    # injection: three pulses (widths 2h .. 10h) and two sines inside the grid
    inj_p = np.array([[amp * 1.3, t[N // 4] + 0.37 * h, 2.0 * h], [amp * 0.8, t[N // 2] + 0.5 * h, 4.1 * h],
                      [amp * 2.1, t[(3 * N) // 4], 9.7 * h]])
    inj_s = np.array([[amp * 0.9, 3.3 / span, 1.1], [amp * 0.4, 0.31 * fnyq, 5.2]])
    box_p = [(0.0, 1e4 * max(amp, 1.0)), (t[0] - 1100 * h, t[-1] + 1100 * h), (0.5 * h, 20 * h)]
    box_s = [(0.0, 1e4 * max(amp, 1.0)), (0.0, fnyq), (0.0, 2 * np.pi)]
    branches = [orj.Branch("pulse", orj.KIND_PULSE, box_p, NL), orj.Branch("sine", orj.KIND_SINE, box_s, NL)]

    def pulse(a, b, c):
        return a * np.exp(-((t - b) ** 2) / (2 * c ** 2))

    def sine(a, f, p):
        return a * np.sin(2 * np.pi * f * t + p)

    y = sigma * rs.randn(N)
    if data == "signal":
        y = y + sum(pulse(*p) for p in inj_p) + sum(sine(*s) for s in inj_s)
    # the edge cases
    widths = [0.97 * h, h, 2 * h, 10 * h]
    lane_b = [8 * m for m in range(1, (N - 1) // 8 + 1)] or [N // 2]
    centres = [lambda j: t[j], lambda j: 0.5 * (t[j] + t[j + 1]), lambda j: 0.5 * (t[lane_b[j % len(lane_b)] - 1] + t[lane_b[j % len(lane_b)]])]
    outside = [1, 3, 10, 100, 1000]
    freqs = [0.5 / span, 3.0 / span, 0.25 * fnyq, 0.9 * fnyq, 0.98 * fnyq]
    phases = [0.0, 1e-9, 2 * np.pi - 1e-9, np.nextafter(2 * np.pi, 0.0), 3.0]
    amps = [1e-3, 1e-1, 1.0, 31.0, 1e3]
    T, W = T_CASE, W_CASE
    x = {"pulse": np.zeros((T, W, NL, 3)), "sine": np.zeros((T, W, NL, 3))}
    inds = {k: np.zeros((T, W, NL), dtype=bool) for k in x}
    for ti in range(T):
        for w in range(W):
            g = ti * W + w
            xp, xs, ip, is_ = x["pulse"][ti, w], x["sine"][ti, w], inds["pulse"][ti, w], inds["sine"][ti, w]
            xp[:] = inj_p[g % 3]                     # dead slots hold some leaf (they sit in the state)
            xs[:] = inj_s[g % 2]
            if g % 64 < 16:                          # the injection, or it with one leaf more / less
                xp[:3], xs[:2] = inj_p, inj_s
                ip[:3], is_[:2] = True, True
                if g % 64 >= 8:
                    if g % 2:
                        ip[g % 3] = False
                    else:
                        xp[3] = [amps[g % 5], t[rs.randint(N - 1)] + rs.rand() * h, widths[g % 4]]
                        ip[3] = True
                continue
            k = g % 64 - 16                          # 48 edge-case walkers: a pulse and a sine of the matrix each
            c = widths[k % 4]
            ci = k // 4 % 4
            if ci < 3:
                b = centres[ci](rs.randint(N - 1))
            else:
                s = outside[k % 5]
                b = t[-1] + s * h if k // 16 % 2 else t[0] - s * h
            xp[0] = [amps[k % 5] * (1.0 + 0.1 * rs.rand()), b, c]
            xs[0] = [amps[(k + 2) % 5], freqs[k % 5] * (1.0 - 1e-3 * rs.rand()), phases[(k // 5) % 5]]
            ip[0] = is_[0] = True
            if k % 3 == 0:                           # ... beside the injection's first pulse and sine
                xp[1], xs[1] = inj_p[0], inj_s[0]
                ip[1] = is_[1] = True
            mix = (k + k // 4) % 4                   # a pulse-only and a sine-only walker now and then
            if mix == 1:
                is_[:] = False
            elif mix == 3:
                ip[:] = False
    return dict(grid=grid, N=N, data=data, amp=amp, sigma=sigma, t=t, y=y, branches=branches, x=x, inds=inds, h=h)


def case_matrix():
    """Every (grid, N, data) with its amplitude scale and sigma form: the amplitude scale cycles through 1e-3, 1, 1e3 and sigma
    (1e-3 times it) is a power of two in every other case."""
    out = []
    for gi, grid in enumerate(GRIDS):
        for ni, N in enumerate(SIZES):
            for di, data in enumerate(DATA):
                j = gi + ni + di
                out.append((grid, N, data, [1e-3, 1.0, 1e3][j % 3], j % 2 == 0))
    return out


def oracle_log_like(case):
    """The float64 oracle's L [T, W]."""
    return orj.template_log_like(case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"])


def shifted_pulse_log_like(case):
    """The oracle's float64 formula with every pulse evaluated one ulp late, at t + ulp(t) (sines at t): the size of error the
    uniform-grid recurrence makes where it puts a point at t0 + k h instead of t[i0 + k]."""
    t, y, sigma = case["t"], case["y"], case["sigma"]
    ts = t + np.spacing(np.abs(t))
    T, W = case["x"]["pulse"].shape[:2]
    tmpl = np.zeros((T, W, t.shape[0]))
    for br in case["branches"]:
        xb, ib = case["x"][br.name], case["inds"][br.name]
        sub = np.zeros_like(tmpl)
        for n in range(xb.shape[2]):
            a, b, c = (xb[:, :, n, k][:, :, None] for k in range(3))
            with np.errstate(all="ignore"):
                f = a * np.exp(-((ts - b) ** 2) / (2 * c ** 2)) if br.kind == orj.KIND_PULSE else a * np.sin(2 * np.pi * b * t + c)
            sub += np.where(ib[:, :, n][:, :, None], f, 0.0)
        tmpl += sub
    return -0.5 * np.sum(((tmpl - y) / sigma) ** 2, axis=-1)
