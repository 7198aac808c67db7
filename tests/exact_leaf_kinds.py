"""tests/exact_template.py's yardstick for all seven leaf kinds (tests/leaf_kinds.py): the log-likelihood computed exactly from its
double inputs, and the a-priori bound B on the error of a plain float64 evaluation of the same formulae.

``exact_log_like`` evaluates the formulae of tests/leaf_kinds.py in exact_template's backend (np.longdouble where its eps is below
1e-18, else mpmath at 40 digits); 2 pi is the double ``2 * np.pi``: the exact value is that of the formula on the doubles the
float64 code sees.  ``float64_bound`` is exact_template.float64_bound - residual, square and sum are the same code on both sides -
fed with the per-point template bound dT built here from the per-kind value bounds below.

Value bounds, to first order in EPS = 2^-52 = two unit roundoffs u; every +, -, x, / rounds once (relative u), exp / sin / cos are
taken as within one EPS, relative, of the true value of their (rounded) argument, as in exact_template:

  pulse    EPS |v| (3 + 3 arg), arg = (t - b)^2 / (2 c^2)                    (exact_template)
  sine     EPS |a| (3 + 2 |2 pi b t| + |c|)                                  (exact_template)
  offset   0                                                                 (the value is the parameter)
  ramp     v = a + b t: the product u |b t|, the sum u |v|  ->  EPS (|b t| + |v|) / 2; taken as EPS (|b t| + |v|)
  lorentz  THE QUOTIENT.  d = t - b (u), z = d / c (u): z to 2 u; z z (u): z^2 to 5 u; s = 1 + z^2 (u): |ds| <= 5 u z^2 + u s;
           v = a / s (u): |dv| / |v| <= ds / s + u = u (2 + 5 z^2 / s)
           ->  EPS |v| (1 + 2.5 z^2 / (1 + z^2))      (at most 3.5 EPS |v|: the quotient is well conditioned everywhere)
  chirp    THE PHASE phi = (2 pi b) t + c t^2.  w = 2 pi b (u; 2 pi itself is exact: a doubling), p1 = w t (u): p1 to 2 u;
           t t (u), p2 = c (t t) (u): p2 to 2 u; the sum (u): |dphi| <= 2 u |p1| + 2 u |p2| + u |phi|.  sin moves by at most
           |dphi|, is within EPS |sin|, the product with a rounds (u)
           ->  EPS |a| (|p1| + |p2| + |phi| / 2 + 1.5 |sin phi|)
           (the phase's ABSOLUTE size decides: on t = 1000 + [0, 1] with c up to 2 pi, |p2| reaches 6e6 and the float64 formula
           itself carries ~2e-9 |a| - tests/test_leaf_kinds.py keeps chirps off that grid)
  burst    THE PRODUCT A C, A = a exp(-z^2), C = cos(psi), psi = (2 pi f) d, d = t - t0, z = d / w.  z^2 to 5 u as above, so
           exp's argument moves by 5 u z^2 and E = exp(-z^2) is within 5 u z^2 + EPS; A = a E (u).  2 pi f (u), d (u), the product
           (u): psi to 3 u, cos moves by at most 3 u |psi|, is within EPS |C|; v = A C (u)
           ->  EPS (|v| (3 + 2.5 z^2) + 1.5 |A| |psi|)  + |a| 1e-300 (gradual underflow of E)

  leaf sums  EPS n sum_j |value_j| at a point, n = active leaves + branches (exact_template: the running sum of a walker)."""
import numpy as np

from tests import exact_template as xt
from tests import leaf_kinds as lk

EPS = xt.EPS


def _cos(ar):
    if ar.exp is np.exp:
        return np.cos
    import mpmath
    return np.frompyfunc(mpmath.cos, 1, 1)


def _f(v):
    return np.asarray(v.astype(np.float64) if hasattr(v, "astype") else v, dtype=np.float64)


def _leaf_exact(kind, p, pd, tl, ar):
    """(value, bound) of one kind for the leaves ``p`` (backend numbers, [..., 1] each) / ``pd`` (the same as doubles) at ``tl``."""
    two_pi = 2 * ar.scalar(xt.PI)
    if kind == "pulse":
        a, b, c = p
        arg = (tl - b) ** 2 / (2 * c * c)
        v = a * ar.exp(-arg)
        return v, EPS * np.abs(_f(v)) * (3.0 + 3.0 * _f(arg)) + np.abs(pd[0]) * 1e-300
    if kind == "sine":
        a, b, c = p
        ph = two_pi * b * tl
        return a * ar.sin(ph + c), EPS * np.abs(pd[0]) * (3.0 + 2.0 * np.abs(_f(ph)) + np.abs(pd[2]))
    if kind == "offset":
        (a,) = p
        return a + tl * 0, np.zeros(np.broadcast(pd[0], _f(tl)).shape)
    if kind == "ramp":
        a, b = p
        bt = b * tl
        v = a + bt
        return v, EPS * (np.abs(_f(bt)) + np.abs(_f(v)))
    if kind == "lorentz":
        a, b, c = p
        z = (tl - b) / c
        z2 = z * z
        v = a / (1 + z2)
        return v, EPS * np.abs(_f(v)) * (1.0 + 2.5 * _f(z2 / (1 + z2)))
    if kind == "chirp":
        a, b, c = p
        p1, p2 = (two_pi * b) * tl, c * (tl * tl)
        s = ar.sin(p1 + p2)
        return a * s, EPS * np.abs(pd[0]) * (np.abs(_f(p1)) + np.abs(_f(p2)) + 0.5 * np.abs(_f(p1 + p2)) + 1.5 * np.abs(_f(s)))
    if kind == "burst":
        a, t0, w, f = p
        d = tl - t0
        z2 = (d / w) * (d / w)
        A = a * ar.exp(-z2)
        psi = (two_pi * f) * d
        v = A * _cos(ar)(psi)
        return v, EPS * (np.abs(_f(v)) * (3.0 + 2.5 * _f(z2)) + 1.5 * np.abs(_f(A)) * np.abs(_f(psi))) + np.abs(pd[0]) * 1e-300
    raise KeyError(kind)


def _template_exact(branches, x, inds, t, ar):
    tl = ar.conv(t)
    shape = x[branches[0].name].shape[:2]
    tm = np.full(shape + (t.shape[0],), ar.zero, dtype=type(ar.zero) if isinstance(ar.zero, xt.LD) else object)
    absv, bvals = np.zeros(shape + (t.shape[0],)), np.zeros(shape + (t.shape[0],))
    for br in branches:
        kind = lk.kind_name(br.kind)
        xb, ib = np.asarray(x[br.name], dtype=np.float64), np.asarray(inds[br.name], dtype=bool)
        for n in range(xb.shape[2]):
            on = ib[..., n][..., None]
            if not on.any():
                continue
            pd = [np.where(on, xb[..., n, d][..., None], 1.0) for d in range(xb.shape[3])]      # (dead slots: any harmless leaf)
            with np.errstate(all="ignore"):
                v, bv = _leaf_exact(kind, [ar.conv(q) for q in pd], pd, tl, ar)
            tm = tm + np.where(on, v, ar.zero)
            absv = absv + np.where(on, np.abs(_f(v)), 0.0)
            bvals = bvals + np.where(on, bv, 0.0)
    return tm, absv, bvals


def exact_log_like(branches, x, inds, t, y, sigma, bound_inds=None, use=None):
    """(L* [T, W], r = (template - y) / sigma [T, W, N], both in the backend's numbers, the per-point template bound dT [T, W, N]);
    ``bound_inds``: the leaves whose roundings dT counts, if not those of ``inds`` (a template updated by +- one leaf still carries
    the roundings of a leaf that has died)."""
    use = use or xt.backend()
    t, y = np.asarray(t, dtype=np.float64), np.asarray(y, dtype=np.float64)

    def run():
        ar = xt._Arith(use)
        tm, absv, bvals = _template_exact(branches, x, inds, t, ar)
        bi = inds
        if bound_inds is not None:
            bi = bound_inds
            _, absv, bvals = _template_exact(branches, x, bi, t, ar)
        r = (tm - ar.conv(y)) / ar.scalar(sigma)
        L = -0.5 * np.sum(r * r, axis=-1)
        nterms = sum(np.asarray(bi[b.name], dtype=bool).sum(axis=-1) for b in branches) + len(branches)
        return L, r, bvals + EPS * nterms[..., None] * absv

    if use == "mpmath":
        import mpmath
        with mpmath.workdps(xt.DPS):
            return run()
    return run()


float64_bound = xt.float64_bound


def yardstick(branches, x, inds, t, y, sigma, bound_inds=None, use=None):
    """(L* rounded to double [T, W], B [T, W])."""
    L, r, dT = exact_log_like(branches, x, inds, t, y, sigma, bound_inds, use)
    return L.astype(np.float64), float64_bound(r, dT, sigma)
