"""Periodic parameters at the seam: the specification in exact arithmetic, the inputs that sit on it, and the cases of
tests/test_hip_periodic_seam.py (host only: NumPy and ``fractions``; nothing of ``eryn_amd`` is imported).

The reference (utils/periodic.py) measures ``c - s`` the short way round where it exceeds half a period, and wraps a proposal with
NumPy's float remainder.  Continuous random positions reach the branches that tell a correct restatement from a nearly correct one
with probability zero: a difference of EXACTLY half a period, a remainder of exactly zero of either sign, a tiny negative proposal
that wraps onto the period itself.  This module puts walkers there.

Exact references
----------------
``exact_distance`` / ``exact_wrap`` evaluate the reference's rules on ``fractions.Fraction`` of the doubles and round each operation
the reference rounds (``c - s``, ``period - s`` / ``period + s``, ``c - new_s``; the remainder once) to the nearest double, ties to
even, with IEEE 754's sign of an exact zero.  ``fmod`` is exact, so NumPy's remainder - ``fmod``, plus the divisor where the signs
differ, rounded once - is the correctly rounded floor-remainder, and the reference for ``wrap`` carries no tolerance at all.

Select form against masked-sum form
-----------------------------------
The reference builds ``new_s = -(per - s) (dp < 0) + (per + s) (dp >= 0)`` (periodic.py:101-107), a device function selects
``new_s = dp < 0 ? -(per - s) : per + s``.  With A = -(per - s) and B = per + s, both finite:

* ``dp < 0``: the sum is ``A * 1 + B * 0 = A + (+-0)``.  For A != 0 that is A.  For A == 0 - which needs ``s == per`` and gives
  A = -0.0 - the other term is ``(per + per) * 0 = +0.0`` and ``-0.0 + +0.0 = +0.0``: the reference has ``new_s = +0.0`` where the
  select form has ``-0.0``.  ``diff = c - new_s`` then differs only where c is a zero that subtraction tells apart: c == -0.0, for
  which the reference's diff is ``-0.0 - +0.0 = -0.0`` and the select form's ``-0.0 - -0.0 = +0.0``.
* ``dp >= 0``: the sum is ``A * 0 + B = (+-0) + B``, B for B != 0; B == 0 needs ``s == -per``, where ``per + s = +0.0`` and
  ``A * 0 = -(2 per) * 0 = -0.0``, and ``-0.0 + +0.0 = +0.0 = B``.  No difference.

So the two forms agree bit for bit except at ``s == period, c == -0.0`` (``zero_sign_exceptions`` lists the rows of the matrix),
where the distances are zeros of opposite sign.  The proposal ``c - diff * zz`` is then ``-0.0 - (-+0.0) = +-0.0``, and ``wrap`` turns
either zero into ``+0.0`` (an exact multiple takes the divisor's sign): the difference never reaches a stored position.
The untaken arm must stay finite, or the masked sum holds ``inf * 0 = nan``: ``|s| + period < 2^1023``.  Every input here stays
under 2^1000; non-finite proposals are out of scope.
"""
import functools
import math
from fractions import Fraction

import numpy as np

# the period families: dyadic periods keep every sum exact (a tie is a real tie), 2 pi is the rounded case, 0.0 = not periodic
DYADIC = (1.0, 2.0 ** -20, 2.0 ** 40, 1.5)
TWO_PI = 2.0 * math.pi
FAMILIES = DYADIC + (TWO_PI, 0.0)
# along a row: neighbours never share a period (a swapped index changes the answer); the pattern's length is odd, so over a row of 14
# coordinates or two shifts of a shorter one every family sits on both halves of a 16-byte lane
PATTERN = (1.0, 0.0, TWO_PI, 2.0 ** -20, 1.5, 2.0 ** 40, 0.0)
LIMIT = 2.0 ** 1000


def row_periods(D, shift=0):
    return np.array([PATTERN[(d + shift) % len(PATTERN)] for d in range(D)])


# ---- IEEE operations on exact rationals ----------------------------------------------------------------------------------------------
def _neg_zero(v):
    return v == 0.0 and math.copysign(1.0, v) < 0.0


def fl_sub(a, b):
    """the double nearest a - b; an exact zero is -0.0 only for (-0.0) - (+0.0)"""
    r = Fraction(a) - Fraction(b)
    if r != 0:
        return float(r)
    return -0.0 if (_neg_zero(a) and b == 0.0 and not _neg_zero(b)) else 0.0


def fl_add(a, b):
    r = Fraction(a) + Fraction(b)
    if r != 0:
        return float(r)
    return -0.0 if (_neg_zero(a) and _neg_zero(b)) else 0.0


def fl_mask(a, m):
    """a * (1.0 if m else 0.0)"""
    if m:
        return a
    return math.copysign(0.0, a)


def exact_distance(s, c, period, form="select"):
    """``PeriodicContainer.distance(p1 = s, p2 = c)`` for one coordinate.  ``form``: "select" (new_s chosen) or "masked" (the
    reference's masked sum): see the module's docstring for where they differ."""
    s, c, period = float(s), float(c), float(period)
    diff = fl_sub(c, s)
    if not period > 0.0:
        return diff
    if abs(Fraction(diff)) > Fraction(period) / 2:                    # strict: a tie keeps the long way
        A, B = -fl_sub(period, s), fl_add(period, s)
        if form == "select":
            new_s = A if diff < 0.0 else B
        else:
            new_s = fl_add(fl_mask(A, diff < 0.0), fl_mask(B, diff >= 0.0))
        diff = fl_sub(c, new_s)
    return diff


def exact_wrap(q, period):
    """NumPy's ``q % period``: the floor-remainder rounded once, the divisor's sign, +0.0 for an exact multiple"""
    q, period = float(q), float(period)
    if not period > 0.0:
        return q
    return float(Fraction(q) % Fraction(period))


def exact_proposal(s, c, zz, period, form="select"):
    """wrap(c - distance(s, c) * zz), every operation rounded once (stretch.py:136-154) -> (q before the wrap, q)"""
    d = exact_distance(s, c, period, form)
    prod = math.copysign(abs(float(Fraction(d) * Fraction(zz))), math.copysign(1.0, d) * math.copysign(1.0, zz))   # (a zero keeps its sign)
    q = fl_sub(c, prod)
    return q, exact_wrap(q, period)


def bits(a):
    """the int64 view: ``array_equal`` on doubles cannot see a sign of zero"""
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the matrix ----------------------------------------------------------------------------------------------------------------------
def _beside(v):
    return [v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]


def edge_matrix(period):
    """-> (pairs[M, 2] of (s, c), targets q[K]) that sit on the seam of one period (for ``period == 0`` the placements of period 1,
    which a coordinate that is not periodic must hand back untouched)."""
    p = float(period) if period > 0.0 else 1.0
    h = p / 2.0
    pairs = []
    # |c - s| on half a period, one ulp above, one ulp below, both signs: from 0 (the difference IS c) and from an eighth
    for base in (0.0, p / 8.0, -p / 8.0):
        for far in _beside(base + h):
            pairs += [(base, far), (far, base)]
        for far in _beside(base - h):
            pairs += [(base, far), (far, base)]
    # s or c on 0, -0.0, period, -period and beside each, against each other and against points of the circle
    special = [0.0, -0.0, np.nextafter(0.0, 1.0), np.nextafter(0.0, -1.0)] + _beside(p) + _beside(-p)
    circle = [p / 8.0, 3.0 * p / 8.0, h, 5.0 * p / 8.0, 7.0 * p / 8.0]
    for a in special:
        pairs += [(a, b) for b in special]
        for b in circle:
            pairs += [(a, b), (b, a)]
    # unwrapped starts, up to three periods out on both sides
    for k in (-3, -2, -1, 1, 2, 3):
        for j in (1.0, 5.0):
            for c in (p / 8.0, 5.0 * p / 8.0, 0.0):
                pairs.append((j * p / 8.0 + k * p, c))
    # |q| >> period from a stretch proposal: one of the two walkers 2^52 or 1e15 periods out (the remainder of a large quotient)
    for far in (2.0 ** 52 * p, -(2.0 ** 52) * p, 1e15 * p, -1e15 * p):
        pairs += [(far, p / 8.0), (5.0 * p / 8.0, far)]
    q = [k * p for k in range(-3, 4)] + [-0.0, 5e-324, -5e-324, -1e-300, 1e300, -1e300, 2.0 ** 52 * p, -(2.0 ** 52) * p,
                                         np.nextafter(p, np.inf), np.nextafter(p, -np.inf), np.nextafter(-p, np.inf),
                                         np.nextafter(-p, -np.inf), p / 3.0, -p / 3.0, 2.5 * p, -2.5 * p, 1e15 * p + h]
    pairs, q = np.array(pairs, dtype=np.float64), np.array(q, dtype=np.float64)
    assert np.abs(pairs).max() + p < LIMIT and np.abs(q).max() < LIMIT
    return pairs, q


def zero_sign_exceptions(period):
    """rows of ``edge_matrix(period)[0]`` on which the select form's distance and the masked sum's are zeros of opposite sign"""
    pairs, _ = edge_matrix(period)
    if not period > 0.0:
        return np.zeros(0, dtype=np.int64)
    return np.flatnonzero((pairs[:, 0] == period) & (pairs[:, 1] == 0.0) & np.signbit(pairs[:, 1]))


def exact_matrix(period, form="select"):
    """-> (distance[M], wrap[K]) of the matrix in exact arithmetic"""
    pairs, q = edge_matrix(period)
    return (np.array([exact_distance(s, c, period, form) for s, c in pairs]), np.array([exact_wrap(v, period) for v in q]))


# ---- dyadic draws: zz = ((a - 1) u + 1)^2 / a exact -------------------------------------------------------------------------------------
DRAWS = {4.0: (0.0, 0.25, 0.5, 0.3718), 9.0: (0.25, 0.6131)}        # a: u_zz (the last of each generic)
EXACT_ZZ = {(4.0, 0.0): 0.25, (4.0, 0.25): 0.765625, (4.0, 0.5): 1.5625, (9.0, 0.25): 1.0}


def stretch_factor(a, u):
    return ((a - 1.0) * u + 1) ** 2.0 / a                            # stretch.py:129-132


# ---- lattice starts --------------------------------------------------------------------------------------------------------------------
def lattice_state(T, W, D, period, rs):
    """x[T, W, D]: periodic coordinates on {0, 1/8, ..., 7/8} period (two walkers are at exactly half a period with probability
    1/8, beyond it with 3/16 per coordinate), the others continuous in (-1, 1)."""
    period = np.asarray(period, dtype=np.float64)
    x = rs.uniform(-1.0, 1.0, size=(T, W, D))
    per = np.flatnonzero(period > 0)
    x[..., per] = rs.randint(8, size=(T, W, per.size)) / 8.0 * period[per]
    return x


# ---- coverage: what the oracle's own intermediates did at the seam ------------------------------------------------------------------------
CLASSES = ("tie", "fix_neg", "fix_pos", "wrap_neg", "wrap_ge", "zero", "on_period")


def new_counts():
    return {k: 0 for k in CLASSES}


def count_distance(cnt, s, c, period):
    period = np.asarray(period, dtype=np.float64)
    idx = np.flatnonzero(period > 0)
    dp, per = (c - s)[..., idx], period[idx]
    fix = np.abs(dp) > per / 2.0
    cnt["tie"] += int((np.abs(dp) == per / 2.0).sum())
    cnt["fix_neg"] += int((fix & (dp < 0.0)).sum())
    cnt["fix_pos"] += int((fix & (dp >= 0.0)).sum())


def count_wrap(cnt, q, out, period):
    period = np.asarray(period, dtype=np.float64)
    idx = np.flatnonzero(period > 0)
    q, out, per = q[..., idx], out[..., idx], period[idx]
    cnt["wrap_neg"] += int((q < 0.0).sum())
    cnt["wrap_ge"] += int((q >= per).sum())
    cnt["zero"] += int((out == 0.0).sum())
    cnt["on_period"] += int((out == per).sum())


def install(monkeypatch, cnt):
    """Count every distance and wrap the oracle makes (pytest's monkeypatch on ``oracle.eryn_oracle``; nothing is written into
    oracle/): the counts come from the oracle's intermediates, never from the device."""
    from oracle import eryn_oracle as orc
    inner_d, inner_w = orc.periodic_distance, orc.periodic_wrap

    def periodic_distance(s, c, period):
        if period is not None:
            count_distance(cnt, s, c, period)
        return inner_d(s, c, period)

    def periodic_wrap(q, period):
        if period is None:
            return inner_w(q, period)
        q0 = q.copy()
        out = inner_w(q, period)
        count_wrap(cnt, q0, out, period)
        return out

    monkeypatch.setattr(orc, "periodic_distance", periodic_distance)
    monkeypatch.setattr(orc, "periodic_wrap", periodic_wrap)


def assert_counts(cnt, claims, least, what=""):
    print(f"{what}: " + ", ".join(f"{k} {cnt[k]}" for k in CLASSES))
    for k in claims:
        assert cnt[k] >= least, f"{what}: {cnt[k]} events of class '{k}', {least} asked for"


# ---- the problem the cases step on -------------------------------------------------------------------------------------------------------
class SeamProblem:
    """A Gaussian on the periods' scales (the benign precision of tests/parity_utils conjugated by 1 / scale, scale = the period or 1;
    the mean at 3/8 of a period), under the box [0, period] on periodic coordinates - ``tight``: [0, nextafter(period, 0)] - and
    [-50, 50] on the others."""

    def __init__(self, D, shift=0, tight=False, like="dense"):
        from tests import parity_utils as pu
        self.D, self.like_kind = D, like
        self.period = row_periods(D, shift)
        per = self.period > 0
        sc = np.where(per, self.period, 1.0)
        mu0, invcov0 = pu.gaussian_problem(D, dense=(like == "dense"))
        self.mu = np.where(per, 0.375 * self.period, mu0)
        self.precision = invcov0 / np.outer(sc, sc) if like == "dense" else np.diag(invcov0) / (sc * sc)
        self.lo = np.where(per, 0.0, -50.0)
        self.hi = np.where(per, np.nextafter(self.period, 0.0) if tight else self.period, 50.0)

    def loglike(self, x):
        from oracle import eryn_oracle as orc
        if self.like_kind == "dense":
            return orc.gaussian_log_like(x, self.mu, self.precision)
        return orc.gaussian_diag_log_like(x, self.mu, self.precision)

    def lattice(self, T, W, seed):
        return lattice_state(T, W, self.D, self.period, np.random.RandomState(seed))


# ---- a. the teacher-forced matrix ---------------------------------------------------------------------------------------------------------
BLOCK = 56              # rows of a period's matrix per call: the matrix's 280 rows are five blocks


def forced_families(D, shift):
    """the distinct periods of the row, in the order of their first coordinate"""
    return list(dict.fromkeys(row_periods(D, shift).tolist()))


def forced_width(D, shift=0):
    """W = BLOCK walkers per period of the row: every call hands every period one block of its matrix, T * W / 2 = F * BLOCK moving
    walkers in all.  56 is the smallest divisor of the matrix's length that puts two full tiles of 64 moving walkers and a ragged one
    on a rung (six periods: W = 336, 168 = 2 * 64 + 40 moving; the five of a row of 5: W = 280, 140 = 2 * 64 + 12)."""
    return BLOCK * len(forced_families(D, shift))


def site_matrix(period, kind="stretch"):
    """the rows of a period's matrix a site runs: all of them; a coordinate that is not periodic keeps its value, so only the rows
    inside its box [-50, 50] after a stretch of up to 4 (|s|, |c| <= 4; MH targets |q| <= 3)"""
    pairs, q = edge_matrix(period)
    if not period > 0.0:
        pairs, q = pairs[np.abs(pairs).max(axis=1) <= 4.0], q[np.abs(q) <= 3.0]
    return pairs if kind == "stretch" else q


@functools.lru_cache(maxsize=8)
def forced_calls(D, shift, kind="stretch"):
    """The calls that walk the matrix over a row of D coordinates.  Slot j = t N + k (stretch: moving walker 2k of rung t, complement
    2k + 1; MH: walker k itself) carries ONE row of ONE period's matrix on ONE coordinate: period j mod F, row j div F of the call's
    block - each period's matrix is walked in order, a block a call, every row with every draw - on the (row + call)-th of the
    coordinates that have that period: every coordinate, both halves of every 16-byte lane, coordinate 0, coordinate D - 1 and the
    neighbour of a pad take their turn.  -> list of dict(a, x[T, W, D], labels, rint, u_zz, d[T, N], fam[T, N], row[T, N], step),
    shared between its callers: read only"""
    T, W = 2, forced_width(D, shift)
    period = row_periods(D, shift)
    fams = forced_families(D, shift)
    F = len(fams)
    mats = {p: site_matrix(p, kind) for p in fams}
    coords = {p: np.flatnonzero(period == p) for p in fams}
    rs = np.random.RandomState(1000 + 7 * D + shift)
    N = W // 2 if kind == "stretch" else W
    block = T * N // F
    assert T * N == F * block and (kind != "stretch" or (block == BLOCK and N > 128 and N % 64 != 0))
    longest = max(len(m) for m in mats.values())
    assert kind != "stretch" or longest % block == 0, "the matrix is a whole number of blocks"
    laps = -(-longest // block)
    tt, kk = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    slot = tt * N + kk
    fam_i, r = slot % F, slot // F
    calls = []
    draws = [(a, u) for a in sorted(DRAWS) for u in DRAWS[a]] if kind == "stretch" else [(4.0, None)]
    n = 0
    for a, u in draws:
        for lap in range(laps):
            x = rs.uniform(-1.0, 1.0, size=(T, W, D))
            pc = period > 0
            x[..., pc] = rs.uniform(0.0, 1.0, size=(T, W, int(pc.sum()))) * period[pc]
            d, row = np.empty((T, N), dtype=np.int64), np.empty((T, N), dtype=np.int64)
            val = np.empty((T, N, 2 if kind == "stretch" else 1))
            for t in range(T):
                for k in range(N):
                    p = fams[fam_i[t, k]]
                    d[t, k] = coords[p][(r[t, k] + n) % len(coords[p])]
                    row[t, k] = (r[t, k] + lap * block) % len(mats[p])         # (a shorter matrix starts over)
                    val[t, k] = mats[p][row[t, k]]
            call = dict(a=a, d=d, period=period, fam=period[d], row=row)
            if kind == "stretch":
                x[tt, 2 * kk, d] = val[..., 0]
                x[tt, 2 * kk + 1, d] = val[..., 1]
                call.update(x=x, labels=np.tile(np.arange(W) % 2, (T, 1)), rint=np.tile(np.arange(N), (T, 1)),
                            u_zz=np.full((T, N), u))
            else:
                q = val[..., 0]
                step = 0.05 * rs.uniform(-1.0, 1.0, size=(T, W, D)) * np.where(pc, period, 1.0)
                x[tt, kk, d] = -0.0                               # -0.0 + q == q for every q, the zeros included
                step[tt, kk, d] = q
                assert same_bits((x + step)[tt, kk, d], q)
                call.update(x=x, step=step, q=q)
            calls.append(call)
            n += 1
    return calls


def forced_reference(call, form="select"):
    """The exact proposals of a stretch call's seam coordinates: -> q[T, N] (wrapped), in exact arithmetic"""
    T, N = call["d"].shape
    out = np.empty((T, N))
    tt, kk = np.meshgrid(np.arange(T), np.arange(N), indexing="ij")
    s, c = call["x"][tt, 2 * kk, call["d"]], call["x"][tt, 2 * kk + 1, call["d"]]
    for t in range(T):
        for k in range(N):
            zz = stretch_factor(call["a"], call["u_zz"][t, k])
            out[t, k] = exact_proposal(s[t, k], c[t, k], zz, call["period"][call["d"][t, k]], form)[1]
    return out


def site_problem(site, shift, tight):
    """The problem of a teacher-forced site; with ``terms`` a tests/prior_terms specification over it - uniform on the box of the
    periodic coordinates, normal(0, 3) on every other of the rest (no log-uniform one: P is the specification's bit for bit)."""
    s = FORCED_SITES[site]
    prob = SeamProblem(s["D"], shift, tight)
    if s.get("terms"):
        from tests import prior_terms as pt
        entries, n = [], 0
        for d in range(prob.D):
            if prob.period[d] > 0 or n % 2:
                entries.append(("uniform", prob.lo[d], prob.hi[d]))
            else:
                entries.append(("normal", 0.0, 3.0))
            n += prob.period[d] == 0
        prob.spec = pt.make_spec(entries)
        prob.lo, prob.hi = prob.spec["lo"], prob.spec["hi"]
    return prob


class prior_of:
    """``with prior_of(prob):`` the oracle's box prior is the problem's specification, where it has one, for the block (the module's
    attribute is put back on the way out; nothing is written into oracle/)"""

    def __init__(self, prob):
        self.spec = getattr(prob, "spec", None)

    def __enter__(self):
        from oracle import eryn_oracle as orc
        self.saved = orc.box_log_prior
        if self.spec is not None:
            from tests import prior_terms as pt
            orc.box_log_prior = pt.box_prior_substitute(self.spec)

    def __exit__(self, *exc):
        from oracle import eryn_oracle as orc
        orc.box_log_prior = self.saved


def forced_state(call, prob):
    """-> (x, L, P, betas) to upload for a call: the likelihood of the positions, the log-prior of a point inside the box for every
    walker (some of the matrix's starts lie outside it; the state is teacher-forced)"""
    from oracle import eryn_oracle as orc
    x = call["x"].copy()
    T, W, D = x.shape
    inside = np.where(prob.period > 0, 0.25 * prob.period, 0.0)[None, :]
    with prior_of(prob):
        P0 = float(orc.box_log_prior(inside, prob.lo, prob.hi)[0])
    assert np.isfinite(P0)
    return x, prob.loglike(x.reshape(-1, D)).reshape(T, W), np.full((T, W), P0), orc.make_ladder(D, ntemps=T)


def forced_oracle(call, prob, state):
    """The oracle's half-step (or MH step) of a call from ``state`` with accept uniforms of 0 - log u = -inf: every proposal inside
    the box is kept - on copies -> (the oracle's dict, x, L, P after it)"""
    from oracle import eryn_oracle as orc
    x, L, P, betas = (np.array(v, copy=True) for v in state)
    with prior_of(prob), np.errstate(divide="ignore"):
        if "step" in call:
            out = orc.mh_step(x, L, P, betas, call["step"], np.zeros(L.shape), prob.lo, prob.hi, prob.loglike, period=prob.period)
        else:
            T, N = call["d"].shape
            out = orc.stretch_split(x, L, P, betas, call["labels"], 0, call["rint"], call["u_zz"], np.zeros((T, N)), call["a"],
                                    prob.lo, prob.hi, prob.loglike, period=prob.period)
    assert np.array_equal(out["keep"], np.isfinite(out["logp"])), "an accept uniform of 0 keeps what is inside the box"
    return out, x, L, P


FORCED_CLAIMS = {"stretch": ("tie", "fix_neg", "fix_pos", "wrap_neg", "wrap_ge", "zero", "on_period"),
                 "mh": ("wrap_neg", "wrap_ge", "zero", "on_period")}
# (D, pad_rows, what steps it) of the teacher-forced sites
FORCED_SITES = {
    "fast_D8": dict(D=8, pad=True), "fast_D16": dict(D=16, pad=True), "fast_D32": dict(D=32, pad=True), "fast_D64": dict(D=64, pad=True),
    "fast_D128": dict(D=128, pad=True), "fast_D11_padded": dict(D=11, pad=True),
    "generic_D5": dict(D=5, pad=False), "generic_D12": dict(D=12, pad=False),
    "generic_D16_prior_terms": dict(D=16, pad=True, terms=True),
    "propose_D8": dict(D=8, pad=True, host=True), "propose_D5": dict(D=5, pad=True, host=True),
    "mh_D32": dict(D=32, pad=True, kind="mh"), "mh_D5": dict(D=5, pad=False, kind="mh"),
}
SHIFTS = (0, 1)         # of the pattern along the row: with both, every family sits on an even and on an odd coordinate of a row of 8 or more


# ---- b. production stepping from the lattice ----------------------------------------------------------------------------------------------
def case(T, W, D, calls=(1, 2, 2), mh=None, nsplits=2, seed=77, kw=None, env=None, path=None):
    return dict(T=T, W=W, D=D, calls=calls, mh=mh, nsplits=nsplits, seed=seed, kw=kw or {}, env=env or {}, path=path)


# path: (n_stretch, n_pt, n_fused) of a profiled call of two stretch iterations
LATTICE_CASES = {
    "two_launch_D8": case(16, 256, 8, path=(2, 0, 2)),
    "two_launch_D64": case(4, 512, 64, path=(2, 0, 2)),
    "short_tiles_T12_D8": case(12, 240, 8, path=(2, 0, 2)),
    "one_launch_D16": case(8, 256, 16, path=(0, 0, 2)),
    "one_launch_refused_D16": case(8, 256, 16, env={"HENS_NO_ITER": "1"}, path=(2, 0, 2)),
    "three_launch_D16": case(8, 256, 16, env={"HENS_NO_FUSED": "1"}, path=(4, 2, 0)),
    "generic_D5": case(5, 100, 5, calls=(1, 2, 2, 2), kw={"pad_rows": False}, path=(4, 2, 0)),
    "three_sets_D16": case(4, 257, 16, nsplits=3, path=(6, 2, 0)),
    "untempered_D16": case(1, 512, 16, path=(4, 0, 0)),
    "mh_iso_D32": case(8, 256, 32, calls=(2, 3, 3), mh=("iso", 0.5), path=(0, 0, 2)),
}
LATTICE_CLAIMS = ("tie", "fix_neg", "fix_pos", "wrap_neg", "wrap_ge")
LEAST = 20


def lattice_problem(c):
    return SeamProblem(c["D"])


def mh_proposal(prob, kind, weight):
    assert kind == "iso"
    return ("iso", 0.3 * float(prob.period[prob.period > 0].min()), weight)


def oracle_lattice_case(monkeypatch, name):
    """The case on the oracle alone, with NumPy's draws and a fresh lattice at the head of every call (the CPU sizing) -> counts"""
    from oracle import eryn_oracle as orc
    c = LATTICE_CASES[name]
    prob = lattice_problem(c)
    cnt = new_counts()
    install(monkeypatch, cnt)
    T, W, D = c["T"], c["W"], c["D"]
    moves = None
    if c["mh"]:
        kind, scale, w = mh_proposal(prob, *c["mh"])
        moves = [("stretch", 1.0 - w), (orc.GaussianProposal(scale * scale), w)]
    R, G = np.random.RandomState(123), np.random.RandomState(456)
    betas = orc.make_ladder(D, ntemps=T) if T > 1 else None
    for j, n in enumerate(c["calls"]):
        o = orc.OracleSampler(prob.lattice(T, W, c["seed"] + j), prob.loglike, prob.lo, prob.hi, R, G, betas=betas, record=False,
                              period=prob.period, nsplits=c["nsplits"], moves=moves)
        assert np.isfinite(o.P).all(), "a start outside the box"
        o.run(n)
        betas = o.betas
    return cnt
