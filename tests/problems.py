"""A heterogeneous problem family for the stepping kernels' prior-box tests (host only, NumPy).

The default problem of the suite (``parity_utils.gaussian_problem`` under a scalar, symmetric box that no proposal ever leaves) gives
every coordinate the same bounds: an index error in a kernel's box test - ``lo[0]`` for every lane, the other gather half's
bounds, a neighbouring row's ballot bits, a pad's (-inf, +inf) interval on a real coordinate - reads the same number as the right
index would.  ``hetero_problem`` makes every such error visible:

* per-coordinate scales ``s_d`` spread over three decades, means ``mu_d`` offset from 0 (every fourth one by hundreds of ``s_d``); the
  precision is the benign matrix conjugated by ``1 / s`` (as well conditioned, relative to its scales, as the benign one);
* a box ``[mu_d - a_d sigma_d, mu_d + b_d sigma_d]`` with all ``a_d``, ``b_d`` distinct, ``a_d != b_d`` - any two bounds of the problem
  differ, most of them by orders of magnitude;
* start positions deep inside the box (the concentric fraction ``INNER`` of it, which a first stretch proposal cannot leave:
  |c - (c - s) zz| <= 3 max(|c|, |s|)) except for ONE coordinate per walker, drawn at random with a random side, which starts in
  the outer zone ``EDGE`` next to its bound: a proposal leaves the box mostly through the moving walker's edge coordinate ALONE,
  so every (coordinate, side) is the sole offender of about one proposal in 10 D.  (With every coordinate near its bounds the
  offenders come in crowds - they share the proposal's stretch factor - and at D = 128 a sole one shows once in 10^4 proposals);
* pinned coordinates: every walker starts exactly ON ``lo_d`` or exactly ON ``hi_d``.  A stretch proposal is
  ``q_d = c_d - (c_d - s_d) zz = c_d``, exactly on the bound; the reference's bounds are inclusive (prior.py:80-88), so such
  proposals are accepted, and a kernel testing ``<`` for ``<=`` rejects every one.  One pin per half of the 16-byte pair a lane
  holds (even / odd coordinate) in each half of the row (the compile-time-width kernels gather rows of 64 and 128 doubles in two
  halves); narrow rows carry two pins;
* optionally periodic parameters whose period is WIDER than their box (the reference wraps first, then tests the prior).
"""
import numpy as np

from oracle import eryn_oracle as orc
from tests import parity_utils as pu

INNER = 0.3              # start positions: the concentric fraction of the box every coordinate but the walker's edge one fills,
EDGE = (0.55, 1.0)       # and the zone, in half-widths from the middle of the box, that one starts in


def pinned_coordinates(D):
    """{coordinate: "lo" | "hi"}: an even and an odd coordinate in each half of the row (two pins where a half has fewer than four
    coordinates to spare), never coordinate 0 - an index that collapsed to 0 must not land on a pin."""
    h = D // 2
    if D < 16:
        return {1: "hi", h + (h % 2): "lo"}                         # odd, first half / even, second half
    return {2: "lo", h - 1 - (h % 2): "hi", h + (h % 2): "hi", D - 1 - (D % 2): "lo"}


class Problem:
    """mu[D], precision ([D, D] dense | [D] diag | None for Rosenbrock), lo[D], hi[D], x0(T, W); ``pinned``: {d: side};
    ``period``: [D] (0 = not periodic) or None; ``loglike``: the oracle's log-likelihood of this problem."""

    def __init__(self, D, like_kind, seed, mu, precision, lo, hi, pinned, period):
        self.D, self.like_kind, self.seed = D, like_kind, seed
        self.mu, self.precision, self.lo, self.hi = mu, precision, lo, hi
        self.pinned, self.period = pinned, period

    def loglike(self, x):
        if self.like_kind == "dense":
            return orc.gaussian_log_like(x, self.mu, self.precision)
        if self.like_kind == "diag":
            return orc.gaussian_diag_log_like(x, self.mu, self.precision)
        return orc.rosenbrock_log_like(x)

    def x0(self, T, W):
        """Start positions inside the box (the reference refuses anything else): see the module's docstring; the pinned coordinates
        exactly on their bound."""
        rs = np.random.RandomState(1000 + self.seed)
        u = INNER * rs.uniform(-1.0, 1.0, size=(T, W, self.D))
        free = np.array(self.free())
        edge = free[rs.randint(free.size, size=(T, W))]
        side = rs.choice([-1.0, 1.0], size=(T, W))
        tt, ww = np.meshgrid(np.arange(T), np.arange(W), indexing="ij")
        u[tt, ww, edge] = side * rs.uniform(EDGE[0], EDGE[1], size=(T, W))
        x = 0.5 * (self.lo + self.hi) + 0.5 * (self.hi - self.lo) * u
        x = np.minimum(np.maximum(x, self.lo), self.hi)
        for d, side in self.pinned.items():
            x[..., d] = self.lo[d] if side == "lo" else self.hi[d]
        return x

    def free(self):
        """The (coordinate, side) pairs a stretch proposal can leave the box through: all but the pinned coordinates, whose
        proposals sit on the bound (they offend once a Metropolis-Hastings step has moved a walker off it)."""
        return [d for d in range(self.D) if d not in self.pinned]


def hetero_problem(D, like_kind="dense", seed=0, pinned=True, periodic=False):
    """The heterogeneous problem at row width ``D``: ``like_kind`` "dense" / "diag" (Gaussian) or "rosen" (no pins: the same box
    construction around the Rosenbrock tests' usual 3 ... 6 range)."""
    rs = np.random.RandomState(7919 + 31 * seed + D)
    if like_kind == "rosen":
        r = rs.permutation(np.linspace(0.0, 1.0, 2 * D))                 # 2 D distinct numbers, dealt to the two sides
        lo, hi = -(3.0 + 3.0 * r[:D]), 3.0 + 3.0 * r[D:]
        return Problem(D, like_kind, seed, np.zeros(D), None, lo, hi, {}, None)
    mu0, invcov0 = pu.gaussian_problem(D, dense=(like_kind == "dense"))
    s = 10.0 ** rs.permutation(np.linspace(-1.5, 1.5, D))            # three decades, in no order along the row
    m = rs.uniform(1.0, 3.0, D) * rs.choice([-1.0, 1.0], D)
    m[rs.permutation(D)[: max(D // 4, 1)]] *= 100.0                  # a quarter of the means hundreds of scales from 0
    mu = s * m
    if like_kind == "dense":
        precision = invcov0 / np.outer(s, s)
        sigma = s * np.sqrt(np.diag(np.linalg.inv(invcov0)))
    else:
        precision = np.diag(invcov0) / (s * s)
        sigma = s / np.sqrt(np.diag(invcov0))
    r = rs.permutation(np.linspace(0.0, 1.0, 2 * D))                 # 2 D distinct numbers: all a_d, b_d distinct, a_d != b_d
    a, b = 2.5 + 1.5 * r[:D], 2.5 + 1.5 * r[D:]
    period = None
    pins = pinned_coordinates(D) if pinned else {}
    if periodic:
        # a third of the free coordinates periodic, the box inside [0, period) and narrower than the period: the mean moves so
        # that lo = 0.1 w, hi = 1.1 w for a box of width w, under a period of 1.25 w (more than half a period wide: walkers
        # at opposite ends of the box are closer the other way round, utils/periodic.py:96-112)
        period = np.zeros(D)
        free = [d for d in range(D) if d not in pins][::3]
        w = (a + b) * sigma
        mu[free] = (0.1 * w + a * sigma)[free]
        period[free] = 1.25 * w[free]
    lo, hi = mu - a * sigma, mu + b * sigma
    return Problem(D, like_kind, seed, mu, precision, lo, hi, pins, period)


# ---- coverage: what the oracle's proposals did at the box ------------------------------------------------------------------------
def new_coverage(D):
    return dict(proposals=0, outside=0, sole_lo=np.zeros(D, dtype=np.int64), sole_hi=np.zeros(D, dtype=np.int64),
                on_lo=np.zeros(D, dtype=np.int64), on_hi=np.zeros(D, dtype=np.int64), stretch=0, mh=0)


def count_coverage(cov, q, logp, keep, lo, hi, kind):
    """Add one move's proposals ``q[T, N, D]`` with log-prior ``logp[T, N]`` and accept mask ``keep[T, N]`` (the oracle's) to
    ``cov``: proposals, proposals with -inf prior, per (coordinate, side) the proposals it is the SOLE offender of, and per
    (coordinate, side) the ACCEPTED proposals that sit exactly on the bound."""
    below, above = q < lo, q > hi
    n_out = (below | above).sum(axis=-1)
    assert np.array_equal(n_out > 0, np.isinf(logp)), "the oracle's log-prior and its proposals disagree on who is outside"
    sole = (n_out == 1)[..., None]
    D = q.shape[-1]
    cov["proposals"] += int(logp.size)
    cov["outside"] += int((n_out > 0).sum())
    cov["sole_lo"] += (below & sole).reshape(-1, D).sum(axis=0)
    cov["sole_hi"] += (above & sole).reshape(-1, D).sum(axis=0)
    acc = np.asarray(keep, dtype=bool)[..., None]
    cov["on_lo"] += ((q == lo) & acc).reshape(-1, D).sum(axis=0)
    cov["on_hi"] += ((q == hi) & acc).reshape(-1, D).sum(axis=0)
    cov[kind] += int(logp.size)


BAND = (0.10, 0.90)          # share of proposals with -inf prior: neither negligible nor nearly all


def coverage_summary(cov, prob):
    """(share outside, smallest sole-offender count over the free coordinates' sides, smallest on-bound accepted count over the
    pins) - what every case prints and asserts."""
    free = prob.free()
    smallest = int(min(cov["sole_lo"][free].min(), cov["sole_hi"][free].min())) if free else 0
    on = [int(cov["on_lo" if side == "lo" else "on_hi"][d]) for d, side in prob.pinned.items()]
    return cov["outside"] / max(cov["proposals"], 1), smallest, (min(on) if on else None)


def assert_coverage(cov, prob, least=1, what=""):
    share, smallest, on = coverage_summary(cov, prob)
    print(f"{what}: proposals {cov['proposals']} ({cov['mh']} MH) / outside {share:.3f} / smallest sole-offender count {smallest}"
          f" / on-bound accepted rows {on}")
    assert BAND[0] <= share <= BAND[1], f"{what}: {share:.3f} of the proposals outside the box, band {BAND}"
    assert smallest >= least, f"{what}: a (coordinate, side) was the sole offender of {smallest} proposals, {least} asked for"
    if prob.pinned:
        assert on >= 1, f"{what}: a pinned coordinate has no accepted proposal sitting on its bound"
    return share, smallest, on


# ---- the cases of tests/test_hip_hetero_box.py (GPU: hens_step replayed) and tests/test_hetero_problem.py (CPU: sized here) ------
def mh_proposal(prob, kind, weight):
    """``HipEnsemble.set_mh_proposal`` arguments on the problem's scales: "iso" - one standard deviation for every coordinate, 0.3 of
    the narrowest one's (the wide coordinates hardly move, the narrow ones meet their bounds); "full" - the lower Cholesky factor
    of 0.02 times the problem's covariance."""
    if prob.like_kind == "rosen":
        return ("iso", 0.05, weight)
    if kind == "iso":
        return ("iso", 0.3 * float(((prob.hi - prob.lo) / 6.0).min()), weight)
    cov = np.linalg.inv(prob.precision) if prob.like_kind == "dense" else np.diag(1.0 / prob.precision)
    return ("full", np.linalg.cholesky(0.02 * cov), weight)


def case(T, W, D, like="dense", calls=(1, 3), mh=None, nsplits=2, periodic=False, seed=77, kw=None, env=None, cpu_shape=None,
         ranks=0):
    return dict(T=T, W=W, D=D, like=like, calls=calls, mh=mh, nsplits=nsplits, periodic=periodic, seed=seed, kw=kw or {},
                env=env or {}, cpu_shape=cpu_shape, ranks=ranks)


# Sizes: a (coordinate, side) is a proposal's sole offender at a rate of about 0.1 / D, so a case needs some 200 D proposals and,
# for the least lucky of its 2 D sides, a margin on top for an expected count of 20 (tests/test_hetero_problem.py measures it).
CASES = {
    # two launches per iteration, rows updated in place, at every compile-time row width (D = 16 / 32 only on grids of more
    # workgroups than the one-launch iteration takes)
    "two_launch_D8": case(16, 256, 8),
    "two_launch_D16_two_word_masks": case(64, 1280, 16, cpu_shape=(64, 128, 16)),
    "two_launch_D32_config2": case(16, 4096, 32, cpu_shape=(16, 512, 32)),
    "two_launch_D64": case(8, 512, 64, calls=(1, 4)),
    "two_launch_D128": case(4, 2048, 128, calls=(2, 6)),
    # ladders that do not divide 128: short tiles; 33 rungs: two-word swap masks
    "short_tiles_T10_D64": case(10, 384, 64, calls=(2, 5)),
    "short_tiles_T12_D8": case(12, 240, 8),
    "two_word_masks_T33_D8": case(33, 130, 8),
    # one launch per iteration (k_iter)
    "one_launch_D16": case(8, 256, 16, calls=(1, 4, 2)),
    "one_launch_D32": case(4, 512, 32, like="diag", calls=(1, 4, 2)),
    # the persistent first launch forced onto a small grid, ragged last tile (N0 = 584)
    "tile2_forced_ragged_D64": case(8, 1168, 64, calls=(1, 4), env={"HENS_TILE2_FORCE": "1", "HENS_TILE2_LOG": "1"}),
    # rows padded to the next compile-time width; the generic-width kernel itself
    "padded_D11": case(4, 256, 11, calls=(1, 4)),
    "padded_D70": case(4, 1024, 70, calls=(2, 6)),
    "generic_D5": case(5, 100, 5, calls=(1, 4), kw={"pad_rows": False}),
    "generic_D12": case(4, 256, 12, like="diag", calls=(1, 4), kw={"pad_rows": False}),
    # three copying launches per iteration
    "three_launch_D32": case(8, 256, 32, calls=(1, 4), env={"HENS_NO_FUSED": "1"}),
    "three_sets_D16": case(4, 257, 16, calls=(1, 5), nsplits=3),
    "untempered_D16": case(1, 2048, 16),
    # the Metropolis-Hastings move in the mix: q = x + step meets the box, pins included
    "mh_iso_D32": case(8, 512, 32, calls=(3, 6), mh=("iso", 0.5)),
    "mh_full_D16": case(8, 256, 16, calls=(3, 6), mh=("full", 0.5)),
    "rosenbrock_D32": case(8, 1024, 32, like="rosen", calls=(1, 4, 2)),
    "rosenbrock_D128": case(4, 4096, 128, like="rosen", calls=(2, 6)),
    # periodic parameters under a box narrower than the period
    "periodic_D16": case(4, 512, 16, periodic=True),
    "periodic_D64": case(4, 1024, 64, calls=(2, 6), periodic=True),
    # ranks of the ladder pipeline (tests/pipeline_worker.py replay): the PIPE instantiations, k_stretch2<PIPE> forced
    "pipeline_2_ranks_D32": case(8, 256, 32, calls=(2, 4), ranks=2, seed=11),
    "pipeline_4_ranks_D32": case(8, 256, 32, calls=(2, 4), ranks=4, seed=11),
    "pipeline_2_ranks_tile2_D64": case(8, 512, 64, calls=(2, 6), ranks=2, seed=11,
                                       env={"HENS_TILE2_FORCE": "1", "HENS_TILE2_LOG": "1", "HENS_TILE2_PIPE_WAITS": "1"}),
}


def case_problem(c):
    return hetero_problem(c["D"], c["like"], seed=0, pinned=c["like"] != "rosen", periodic=c["periodic"])
