"""The cases of tests/test_move_interactions.py (CPU: sized on the specification alone) and tests/test_hip_move_interactions.py (GPU:
hens_step replayed): the generator moves in the MH slot - DistributionGenerate (k_dist), MTDistGenMove (k_mt_dist) - and Gibbs block
tables on the ladders, tiles, periods, set counts and adaptation settings that tests/dist_move.py, tests/mt_move.py and
tests/gibbs_move.py never step (host only, NumPy).  The case table is stated once, here; so are the coverage conditions
(``check_coverage``), which both files assert - the CPU file over twice the iterations with a factor of two to spare.

A case is a shape, a likelihood, a prior, one ladder family (tests/ladders.py) and the adaptation's settings; its ``runs`` name the
slot and the generator of every replay made on it.  Every ladder is stepped at the strong adaptation of tests/ladders.py (lag 50,
time 10) from calls of (1, n) iterations.

The problem of a case is tests/dist_move.DistProblem - a box of +-4 likelihood widths (or tests/prior_terms.PriorProblem's mixed
terms), every rung started from the same cloud that fills 0.9 of it: an independence proposal is accepted where it improves on the
walker it meets, which such a start lets happen on every rung within the first move iterations.  Under a beta = 0 rung the box is
the rung's posterior, so no ``hot_box`` (tests/ladders.py) is needed: the rung below it is as wide as the box from the start.

Periodic cases (``Problem(periodic=True)``).  Under a box: coordinate 3 has period p = 4 widths, the likelihood's mean at p / 2, so
that the prior box and (whatever the generator's kind elsewhere) a uniform generator term cover [-p / 2, 3 p / 2] - half a period
beyond [0, p] on both sides; coordinate 6 has a period of 10 widths that contains its box, where only the short way round of the
stretch move's distance acts.  Under prior terms: the normal coordinates (d % 4 == 1) of PriorProblem(periodic=True), period 8
widths, the generator uniform on [-p / 2, 3 p / 2] there.  The stretch and the Gaussian move wrap such a coordinate into [0, p); the
generator moves never do (the reference's distgen.py and multipletry.py hold no wrap), so their accepted proposals leave walkers
outside [0, p) for the next stretch iteration to measure its distances from.

The steep gap.  The hand-made ladders of six rungs and more (``ladders.user_features``) have a steep gap, and tests/ladders.py asks
that no swap cross it.  That needs the rungs over the gap at log-likelihoods several hundred below the rungs under it - a box of 35
widths, a start tempered rung by rung - while "a proposal of the move accepted on every rung" needs ONE generator of per-coordinate
terms that is typical both of that box (a rung over the gap accepts where logq(old) >= logq(new), roughly) and of a posterior some
1e-12 of its volume.  Under prior terms the supports are six widths and no pair of rungs is that far apart at all.  The two
conditions exclude each other by construction; the cascade across a gap is tests/test_hip_ladders.py's subject and the move on every
rung is this file's, so these cases keep the common cloud, are exempt from "steep_gap" and meet everything else the ``user`` family
asks for: beta_0 = 0.8, every swap of the repeated pair accepted, the pair still equal, the ends untouched, the last rung exactly 0.
"""
import numpy as np

from tests import dist_move as dm
from tests import ladders as ld
from tests import prior_terms as pt

LAG, NU = ld.LAG, ld.NU
SEED_M = 3005          # ... M s M s s s s M s s M s: the first iteration is the slot's (16 walkers a rung: the start's cloud is what the move improves on)
SEED = 3004            # the move choice of iterations 0 .. 11 at weight 0.5: s M s M s s M s s s M s (tests/production_draws.is_mh)


class Problem(dm.DistProblem):
    """tests/dist_move.DistProblem, and with ``periodic`` the periods of the module's docstring (``period`` [D], 0: not periodic)."""

    def __init__(self, D, like="dense", prior="box", gen="mixed", periodic=False):
        super().__init__(D, like, prior, "mixed" if gen == "mixed_own_start" else gen)
        self.period, self.wide, self.own_start = None, [], gen == "mixed_own_start"
        if not periodic:
            return
        period = np.zeros(D)
        if prior == "terms":
            pp = pt.PriorProblem(D, like, periodic=True)
            self.mu, self.prior, self.lo, self.hi = pp.mu, pp.spec, pp.spec["lo"], pp.spec["hi"]
            self.centre, self.half = 0.5 * (pp.start_lo + pp.start_hi), 0.5 * (pp.start_hi - pp.start_lo)
            period, self.wide = pp.period.copy(), [int(d) for d in np.flatnonzero(pp.period > 0)]
        else:
            d = 3
            period[d] = self.half[d]                              # 4 widths; the box: [mu - 4 widths, mu + 4 widths] = [-p / 2, 3 p / 2]
            self.mu = self.mu.copy()
            self.mu[d] = self.centre[d] = 0.5 * period[d]
            self.prior = dm.box_spec(self.centre - self.half, self.centre + self.half)
            self.lo, self.hi = self.prior["lo"], self.prior["hi"]
            self.wide = [d]
            if D > 6:
                period[6] = self.centre[6] + 1.25 * self.half[6]  # 10 widths: the box [1, 9] widths lies inside [0, p)
                assert self.lo[6] > 0.0 and self.hi[6] < period[6]
        self.gen = {k: v.copy() for k, v in self.gen.items()}
        for d in self.wide:                                       # the generator: uniform on [-p / 2, 3 p / 2]
            lo, hi = -0.5 * period[d], 1.5 * period[d]
            self.gen["kind"][d], self.gen["lo"][d], self.gen["hi"][d] = pt.UNIFORM, lo, hi
            self.gen["c0"][d], self.gen["c1"][d], self.gen["c2"][d] = np.log(1 / (hi - lo)), 0.0, 0.0
            assert self.prior["lo"][d] <= lo and self.prior["hi"][d] >= hi
        self.period = period


    def x0(self, T, W):
        """``own_start``: the coordinates of the generator's normal terms start as draws of those terms (inside the prior's box)."""
        x = super().x0(T, W)
        if self.own_start:
            rs = np.random.RandomState(78)
            nrm = np.flatnonzero(self.gen["kind"] == pt.NORMAL)
            z = self.gen["c0"][nrm] + self.gen["c1"][nrm] * rs.randn(T, W, nrm.size)
            x[..., nrm] = np.clip(z, (self.centre - 0.95 * self.half)[nrm], (self.centre + 0.95 * self.half)[nrm])
        return x


def case(T, W, D, like, prior, family, runs, path, n=5, periodic=False, nsplits=2, adaptive=True, stop_adaptation=-1, seed=SEED,
         weight=0.5, gibbs=None, exempt=()):
    """``runs``: (slot, generator) pairs - slot "dist", ("mt", K) or "gauss"; generator a tests/dist_move.DistProblem kind - "box" the
    prior's own box - or "mixed_own_start": "mixed", the start's coordinates under its normal terms drawn from those terms.  A beta = 0 rung accepts
    where logq(old) - logq(new) > log u and nothing else: from a start that fills the box, 16 normal terms of 0.35 half-widths
    (D = 32) leave it at an acceptance of a per cent; from a start that is a draw of the terms, at a half, on every rung.
    ``path``: the launches a profiled call must report - "one" (k_iter), "two" (the in-place pair), "copying",
    "sets" (one copying launch per set), "blocks" (Gibbs: the copying launches block after block).  ``exempt``: the coverage
    conditions the case cannot meet by construction (``check_coverage`` names them)."""
    return dict(T=T, W=W, D=D, like=like, prior=prior, family=family, runs=tuple(runs), path=path, n=n, calls=(1, n), periodic=periodic,
                nsplits=nsplits, adaptive=adaptive, stop_adaptation=stop_adaptation, seed=seed, weight=weight, gibbs=gibbs, exempt=tuple(exempt))


def _blocks(D):
    """three blocks: the even coordinates, the odd ones, and the last coordinate alone (a one-coordinate block: factor exactly 0)"""
    m = np.zeros((3, D), dtype=bool)
    m[0, 0::2] = m[1, 1::2] = m[2, D - 1] = True
    return m


MIXED_AND_BOX = lambda K, g="mixed": (("dist", g), ("dist", "box"), (("mt", K), "box"))      # noqa: E731  (a beta = 0 rung: one run per move on the box)
BOTH = lambda K: (("dist", "mixed"), (("mt", K), "mixed"))                               # noqa: E731
CASES = {
    # A. ladders and tiles.  Record-mode column blocks (production_draws.label_cb): 6 x 64 -> 16, 10 x 128 -> 8, 33 x 66 -> 2, 64 x 16 -> 2,
    # 4 x 64 -> 32; none at 65 rungs and more
    "short_T6_D32": case(6, 64, 32, "dense", "box", "inf", MIXED_AND_BOX(5, "mixed_own_start"), "one"),             # short tiles, matrix pipe
    "short_T10_D8": case(10, 128, 8, "diag", "box", "user", MIXED_AND_BOX(3), "two", exempt=("steep_gap",)),      # short tiles, two launches
    "short_T33_D16": case(33, 66, 16, "diag", "box", "inf", MIXED_AND_BOX(2), "one"),            # cb = 2, two-word swap masks
    "T64_D32_geometric": case(64, 16, 32, "dense", "box", "geometric", (("dist", "mixed_own_start"), (("mt", 64), "mixed")), "one", seed=SEED_M, exempt=("beta0",)),      # 63-pair cascade; one walker per workgroup
    "T64_D32_inf": case(64, 16, 32, "dense", "box", "inf", MIXED_AND_BOX(64, "mixed_own_start"), "one", seed=SEED_M),
    "long_T65_D8": case(65, 16, 8, "diag", "terms", "user", BOTH(7), "copying", exempt=("steep_gap",)),      # the copying path, by-field state
    "long_T130_D8": case(130, 16, 8, "diag", "box", "inf", (("dist", "mixed"), ("dist", "box")), "copying"),          # the stand-alone adaptation kernel
    "noadapt_T4_D16": case(4, 64, 16, "diag", "box", "user", BOTH(3), "one", adaptive=False, exempt=("ladder_moved",)),
    "stops_T4_D16": case(4, 64, 16, "diag", "box", "user", (("dist", "mixed"),), "one", stop_adaptation=2),
    # B. periodic parameters
    "periodic_T4_D16": case(4, 64, 16, "diag", "box", "geometric", BOTH(4), "one", periodic=True, exempt=("beta0",)),
    "periodic_T4_D64": case(4, 64, 64, "dense", "box", "geometric", (("dist", "mixed"),), "two", periodic=True, exempt=("beta0",)),
    "periodic_terms_D5": case(3, 40, 5, "diag", "terms", "geometric", BOTH(5), "copying", periodic=True, exempt=("beta0",)),
    # C. more than two sets
    "sets3_D8": case(3, 67, 8, "diag", "box", "geometric", BOTH(5), "sets", nsplits=3, exempt=("beta0",)),
    "sets3_all_D11": case(3, 67, 11, "diag", "terms", "geometric", (("dist", "mixed"),), "sets", nsplits=3, periodic=True, exempt=("beta0",)),
    # E. Gibbs tables of three blocks on both moves (the Gaussian move in the slot)
    "gibbs_T10_D8": case(10, 40, 8, "diag", "box", "inf", (("gauss", "box"),), "blocks", gibbs=_blocks(8)),
    "gibbs_T65_D8": case(65, 16, 8, "diag", "box", "user", (("gauss", "box"),), "blocks", gibbs=_blocks(8), exempt=("steep_gap",)),
    "gibbs_T6_D5_terms": case(6, 40, 5, "diag", "terms", "inf", (("gauss", "box"),), "blocks", gibbs=_blocks(5)),
    "gibbs_noadapt": case(4, 40, 8, "diag", "box", "geometric", (("gauss", "box"),), "blocks", gibbs=_blocks(8), adaptive=False,
                          exempt=("ladder_moved", "beta0")),
}


def run_id(name, run):
    slot, gen = run
    return f"{name}-{slot if isinstance(slot, str) else 'mt%d' % slot[1]}-{gen}"


RUNS = [(name, run) for name, c in CASES.items() for run in c["runs"]]
RUN_IDS = [run_id(name, run) for name, run in RUNS]


def case_problem(c, gen):
    return Problem(c["D"], c["like"], c["prior"], gen, periodic=c["periodic"])


def gauss_scale(prob):
    """The Gaussian move's isotropic standard deviation (tests/gibbs_move.mh_scale)."""
    return 0.25 * float(prob.sig.min())


def slot_of(c, run, prob):
    """The ``slot`` argument of tests/composed_replay.replay for a run."""
    slot, _ = run
    if slot == "dist":
        return ("dist", prob.gen, c["weight"])
    if slot == "gauss":
        return ("gauss", "iso", gauss_scale(prob), c["weight"])
    return ("mt", prob.gen, slot[1], c["weight"])


def case_inputs(c, prob):
    """-> betas0[T], x0[T, W, D]"""
    return ld.ladder(c["family"], c["T"], c["D"]), prob.x0(c["T"], c["W"])


class Coverage:
    """What the replay of a run did, counted from the SPECIFICATION's side (tests/composed_replay.py fills it)."""

    def __init__(self, T):
        self.slot_iters = self.stretch_iters = self.slot_after_stretch = 0
        self.slot_accepted = np.zeros(T, dtype=int)          # accepted proposals of the move in the slot per rung (Gibbs: over its blocks)
        self.stretch_accepted = np.zeros(T, dtype=int)
        self.hottest_rejected = 0                            # proposals of the slot the hottest rung refused
        self.picks_beyond_0 = self.old_outside = self.old_outside_accepted = 0
        self.slot_outside_period_accepted = 0                # accepted slot proposals with a periodic coordinate outside [0, period): unwrapped
        self.seam_wrapped_accepted = 0                       # accepted stretch proposals the wrap moved
        self.knives = 0
        self.books = None                                    # tests/gibbs_move.BlockBooks under Gibbs tables


def check_coverage(c, run, cov, betas0, betas, swaps, spare=1, what=""):
    """The conditions a run must meet for its comparison to mean something; ``betas``: the ladder after the run (the specification's,
    and on the GPU the device's too), ``swaps[T - 1]``: accepted swaps per adjacent pair.  ``spare``: the factor the counts must
    clear their bound by (the CPU sizing asks for 2 over twice the iterations, the GPU replay for 1).  A case's ``exempt`` names what
    it cannot meet by construction: "beta0" (no beta = 0 rung), "ladder_moved" (the adaptation is off), "steep_gap" (the module's
    docstring)."""
    T, W = c["T"], c["W"]
    slot, gen = run
    iters = cov.slot_iters + cov.stretch_iters
    print(f"{what}: {cov.slot_iters} slot / {cov.stretch_iters} stretch iterations, {cov.slot_after_stretch} slot directly after stretch; slot accepted "
          f"per rung min {int(cov.slot_accepted.min())} (hottest {int(cov.slot_accepted[-1])}, refused {cov.hottest_rejected}); swaps per pair min "
          f"{int(swaps.min())}; picks beyond try 0 {cov.picks_beyond_0}; old outside {cov.old_outside} (moved {cov.old_outside_accepted}); outside "
          f"[0, period) accepted unwrapped {cov.slot_outside_period_accepted}; seam wrapped and accepted {cov.seam_wrapped_accepted}; knives {cov.knives}")
    assert cov.slot_iters >= spare, f"{what}: fewer than {spare} iterations of the move in the slot"
    assert c["weight"] >= 1.0 or cov.stretch_iters >= spare, f"{what}: fewer than {spare} stretch iterations"
    assert cov.slot_after_stretch >= spare, f"{what}: no slot iteration directly behind a stretch iteration of the same call"
    assert (cov.slot_accepted >= spare).all(), f"{what}: a rung accepted fewer than {spare} proposals of the move in the slot: {cov.slot_accepted.tolist()}"
    # the ladder
    i, j = ld.user_features(T) if c["family"] == "user" else (None, None)
    if j is not None and "steep_gap" not in c["exempt"]:
        assert swaps[j - 1] == 0, f"{what}: {swaps[j - 1]} swaps crossed the steep gap ({j - 1}, {j})"
        pairs = np.arange(T - 1) != j - 1
    else:
        pairs = np.ones(T - 1, dtype=bool)
    assert (swaps[pairs] >= spare).all(), f"{what}: an adjacent pair swapped fewer than {spare} times: {swaps.tolist()}"
    if i is not None:
        assert swaps[i] == iters * W, f"{what}: the repeated pair ({i}, {i + 1}) refused a swap: {swaps[i]} of {iters * W}"
        assert betas[i] == betas[i + 1], f"{what}: the repeated pair came apart: {betas[i]!r} / {betas[i + 1]!r}"
    assert betas[0] == betas0[0] and betas[-1] == betas0[-1], f"{what}: the adaptation moved an end of the ladder"
    if "ladder_moved" in c["exempt"]:
        assert np.array_equal(betas, betas0), f"{what}: the ladder moved although the adaptation is off"
    else:
        moved = float(np.max(np.abs(betas[1:-1] / betas0[1:-1] - 1.0)))
        assert moved > 1e-6, f"{what}: the ladder hardly moved ({moved:.2e}): no launch of the move met an adapted ladder"
    # a beta = 0 rung under the prior's own box: lnpdiff is exactly 0 there (multiple try: every weight 0, lsw = aux_lsw, factor 0)
    if "beta0" in c["exempt"]:
        assert betas0[-1] != 0.0
    else:
        assert betas0[-1] == 0.0 and betas[-1] == 0.0
        if gen == "box" and slot != "gauss":
            assert cov.hottest_rejected == 0 and cov.slot_accepted[-1] == cov.slot_iters * W, \
                f"{what}: the beta = 0 rung refused {cov.hottest_rejected} proposals drawn from its own posterior"
    if slot != "gauss":
        assert cov.old_outside_accepted == 0, f"{what}: an old point outside the generator was moved"
    if isinstance(slot, tuple):
        assert cov.picks_beyond_0 >= spare, f"{what}: no pick other than try 0"
    if c["periodic"]:
        assert cov.slot_outside_period_accepted >= spare, f"{what}: no accepted proposal of the move outside [0, period)"
        assert cov.seam_wrapped_accepted >= spare, f"{what}: no accepted stretch proposal that the wrap moved"


def orc_wrap(q, period):
    """``q`` with its periodic coordinates wrapped into [0, period) (the oracle's periodic_wrap, on a copy)."""
    from oracle import eryn_oracle as orc
    return orc.periodic_wrap(np.array(q, dtype=np.float64, copy=True), period)


# ---- D. a ladder shard, teacher-forced ------------------------------------------------------------------------------------------------------------
# One whole context and one with rung_range = (1, 3), the same seed and state rows.  The ladder is the geometric one: unequal, so that
# betas[tl] in place of betas[rung_begin + tl] changes keeps (tests/test_move_interactions.py shows that it does).
SHARD_T, SHARD_W, SHARD_RANGE, SHARD_K = 4, 40, (1, 3), 5
SHARD_D = {16: ("diag", "box"), 11: ("diag", "terms")}        # 11: padded to 16, prior terms
SHARD_PROPOSALS = 3


def shard_problem(D):
    like, prior = SHARD_D[D]
    return Problem(D, like, prior, "mixed")


def shard_inputs(D):
    """-> problem, betas[T], x, L, P of the whole ladder on the specification's side"""
    prob = shard_problem(D)
    T, W = SHARD_T, SHARD_W
    x = prob.x0(T, W).copy()
    P = pt.log_prior(prob.prior, x.reshape(-1, D)).reshape(T, W)
    assert np.isfinite(P).all()
    return prob, ld.ladder("geometric", T, D), x, prob.loglike(x.reshape(-1, D)).reshape(T, W), P


# ---- the two chains from the real reference (tests/golden/distgen/dg3_periodic_mix.npz, tests/golden/mt/mt3_periodic_mix.npz) ----------------
REFERENCE_CHAINS = [("dist", "dg3_periodic_mix"), ("mt", "mt3_periodic_mix")]


class FixtureProblem:
    """The problem of a fixture in the shape tests/composed_replay.py reads a problem."""

    def __init__(self, fx):
        from oracle import eryn_oracle as orc
        self.prior, self.gen = dm.fixture_specs(fx)
        self.lo, self.hi, self.D = self.prior["lo"], self.prior["hi"], int(fx["D"])
        self.like_kind, self.mu, self.precision = "dense", fx["mu"], fx["invcov"]
        self.period = np.asarray(fx["period"], dtype=np.float64)
        self.loglike = lambda x: orc.gaussian_log_like(x, self.mu, self.precision)


def load_reference_chain(kind, name):
    from tests import mt_move as mt
    return dm.load_fixture(name) if kind == "dist" else mt.load_fixture(name)


def fixture_slot(kind, fx, prob, weight=0.5):
    return ("dist", prob.gen, weight) if kind == "dist" else ("mt", prob.gen, int(fx["K"]), weight)


def fixture_draws(kind, fx, it):
    """Iteration ``it`` of a fixture as the draws tests/composed_replay.spec_iteration consumes, and the fixture's record of it."""
    from tests import mt_move as mt
    rec = dm.fixture_iteration(fx, it) if kind == "dist" else mt.fixture_iteration(fx, it)
    is_slot = bool(rec["is_dist"] if kind == "dist" else rec["is_mt"])
    ref = {k: rec[k] for k in ("iperm", "i1perm", "u_swap")}
    if not is_slot:
        ref.update({k: rec[k] for k in ("labels", "rint0", "rint1", "u_zz0", "u_zz1", "u_acc0", "u_acc1")})
    d = dict(is_mh=is_slot, refs=[ref])
    if is_slot:
        d.update(q=rec["q"], u_acc=rec["u_acc"])
        if kind == "mt":
            d["u_pick"] = rec["u_pick"]
    return d, rec
