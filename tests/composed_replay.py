"""One replay of hens_step through the composed specification: the loop tests/test_hip_dist_move.py, tests/test_hip_mt_move.py,
tests/test_hip_gibbs.py and tests/test_hip_priors.py each carry a copy of, with everything a context can be set to handed through -
the period, the set count, the adaptation's constants and switches, the move in the MH slot, Gibbs block tables.

    stretch iterations   tests/replay_utils.oracle_iteration (the pinned oracle; more than two sets: draws_to_reference_sets),
                         the case's prior substituted for the oracle's box where it has terms
    the slot             None | ("gauss", kind, scale, weight) -> the oracle's mh_step through oracle_iteration
                         ("dist", gen, weight)                 -> tests/dist_move.dist_step, then dist_move.pt_tail
                         ("mt", gen, K, weight)                -> tests/mt_move.mt_step with mt_move.exact_mt, then dist_move.pt_tail
    Gibbs tables         tests/gibbs_move.stretch_iteration / mh_iteration, one cascade behind the last block

``spec_iteration`` is one iteration on draws from anywhere; ``SpecDraws`` makes them from the specification alone
(tests/production_draws.py, dist_move.dist_draws, mt_move.mt_draws / pick_uniforms: the CPU sizing of
tests/test_move_interactions.py), ``replay`` takes them from a context (hens_debug_draws, hens_mt_debug_draws), checks them against
the specification's and compares the context's state call by call at the project's bars and nothing new: positions exact,
log-prior by ``check_P``, log-likelihood through ``tolerance_log.check_logl(..., RTOL_L, ...)``, betas at rtol 1e-13 / atol 0 (a
beta = 0 rung: exactly 0), accept, slot-accept and swap counters and proposal counts exact, no decision on the knife edge, and for
multiple try the bound derived in tests/mt_move.py.
"""
import contextlib

import numpy as np

from oracle import eryn_oracle as orc
from tests import dist_move as dm
from tests import gibbs_move as gm
from tests import mt_move as mt
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import replay_utils as ru
from tests import tolerance_log as tol

LD = np.longdouble


def is_box(prob):
    return bool(np.all(prob.prior["kind"] == pt.UNIFORM))


def check_P(P, Pspec, prob, x, what):
    """Log-prior: under a box the constant, bit for bit; under terms within 1.0 B_P of exact arithmetic at the positions."""
    if is_box(prob):
        assert np.array_equal(P, Pspec), f"{what}: log-prior differs"
        return
    r = pt.worst_ratio(P.reshape(-1), prob.prior, x.reshape(-1, prob.D))
    print(f"{what}: |P - P*| / B_P <= {r:.3f}")
    assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"


def no_knife(info, ex, what):
    with np.errstate(divide="ignore"):
        assert not pu.knife_edge(info["lnpdiff"], np.log(info["u_acc"])).any(), f"{what}: an accept decision on the knife edge: pick another seed"
    assert not mt.pick_knife(ex["c"], info["u_pick"], ex["B_c"]).any(), f"{what}: a pick on the knife edge: pick another seed"


def slot_weight(slot):
    return 0.0 if slot is None else float(slot[-1])


# ---- the draws: checked against the specification, or made from it -----------------------------------------------------------------------------
def check_generator_draws(q, gen, X, Xs, E, what):
    """Points ``q`` the device drew from ``gen`` against the specification's (X float64, X* long double, bound E): uniform terms bit
    for bit, the others within E, everything inside its support after the clamp."""
    kinds = gen["kind"]
    uni = kinds == pt.UNIFORM
    assert q.shape == X.shape, f"{what}: the draws' shape"
    assert np.array_equal(q[..., uni], X[..., uni]), f"{what}: a uniform draw differs from the specification"
    err = np.abs(q.astype(LD) - Xs).astype(np.float64)
    assert (err <= E)[..., ~uni].all(), f"{what}: a draw misses its bound E by a factor {float((err / np.where(E > 0, E, 1))[..., ~uni].max()):.2f}"
    for k in range(len(kinds)):
        if kinds[k] != pt.NORMAL:
            assert (q[..., k] >= gen["lo"][k]).all() and (q[..., k] <= gen["hi"][k]).all(), f"{what}: a draw outside its support"


def check_dist_draws(d, seed, it, T, W, gen, what, rung_begin=0):
    check_generator_draws(d["mh_step"], gen, *dm.dist_draws(seed, it, T, W, gen, rung_begin), what)
    assert np.array_equal(d["mh_u"], dm.accept_uniforms(seed, it, T, W, rung_begin)), f"{what}: accept uniforms"


def check_mt_draws(tries, d, seed, it, T, W, K, gen, what, rung_begin=0):
    """``tries``: (q, u_pick, u_acc) of hens_mt_debug_draws; ``d``: hens_debug_draws of the same iteration (None: not compared)."""
    q, up, ua = tries
    check_generator_draws(q, gen, *mt.mt_draws(seed, it, T, W, K, gen, rung_begin), what)
    assert np.array_equal(up, mt.pick_uniforms(seed, it, T, W, rung_begin)), f"{what}: pick uniforms"
    assert np.array_equal(ua, mt.accept_uniforms(seed, it, T, W, rung_begin)), f"{what}: accept uniforms"
    if d is not None:       # hens_debug_draws keeps its shape: its mh_step is try 0 - DistributionGenerate's point - its mh_u the accept uniform
        assert np.array_equal(d["mh_step"][..., :q.shape[-1]], q[:, :, 0]) and np.array_equal(d["mh_u"], ua), f"{what}: hens_debug_draws"


def row_width(prob):
    return prob.D if prob.like_kind == "rosen" else next(w for w in (8, 16, 32, 64, 128) if w >= prob.D)


class SpecDraws:
    """The draws of iteration ``it`` from the specification alone, in the shape ``DeviceDraws`` hands them over.  More than two sets:
    tests/production_draws.py states no plan of sets, so the sets, complements and uniforms of a stretch iteration are NumPy's
    (seeded by the iteration) - enough to size a case, and replaced by the context's own on the GPU."""

    def __init__(self, seed, T, W, prob, slot, nsplits=2, gibbs=None):
        self.seed, self.T, self.W, self.prob, self.slot, self.nsplits, self.gibbs = seed, T, W, prob, slot, nsplits, gibbs
        self.cb = pd.label_cb(T, W)

    def _sets(self, it):
        T, W, n = self.T, self.W, self.nsplits
        rs = np.random.RandomState(7000 + it)
        labels = np.stack([rs.permutation(np.arange(W) % n) for _ in range(T)])
        out = dict(labels=labels)
        for k in range(n):
            Ns = (W - k + n - 1) // n
            out[f"rint{k}"] = rs.randint(W - Ns, size=(T, Ns))
            out[f"u_zz{k}"], out[f"u_acc{k}"] = rs.uniform(size=(T, Ns)), rs.uniform(size=(T, Ns))
        return out

    def __call__(self, it, what=""):
        seed, T, W, prob, slot = self.seed, self.T, self.W, self.prob, self.slot
        pt_slot, u_swap = pd.pt_draws(seed, it, T, W)
        out = dict(is_mh=pd.is_mh(seed, it, slot_weight(slot)))
        nb = 1 if self.gibbs is None else len(self.gibbs["mh" if out["is_mh"] else "stretch"])
        plans = [dict(gm.block_plan(seed, it, T, W, self.cb, b), pt_slot=pt_slot, u_swap=u_swap) for b in range(nb if not out["is_mh"] else 1)]
        out["refs"] = [ru.draws_to_reference(p, T, W) for p in plans]
        if self.nsplits != 2 and not out["is_mh"]:
            out["refs"] = [dict(self._sets(it), iperm=out["refs"][0]["iperm"], i1perm=out["refs"][0]["i1perm"], u_swap=u_swap)]
        if not out["is_mh"]:
            return out
        if slot[0] == "dist":
            out.update(q=dm.dist_draws(seed, it, T, W, slot[1])[0], u_acc=dm.accept_uniforms(seed, it, T, W))
        elif slot[0] == "mt":
            out.update(q=mt.mt_draws(seed, it, T, W, slot[2], slot[1])[0], u_pick=mt.pick_uniforms(seed, it, T, W), u_acc=mt.accept_uniforms(seed, it, T, W))
        else:
            assert slot[1] == "iso"
            zs = [gm.mh_block_draws(seed, it, T, W, row_width(prob), b) for b in range(nb)]
            out.update(steps=[float(slot[2]) * z[..., :prob.D] for z, _ in zs], us=[u for _, u in zs])
        return out


class DeviceDraws:
    """The draws a context consumed in iteration ``it`` (hens_debug_draws, hens_debug_draws_block, hens_mt_debug_draws), checked
    against the specification's where it states them."""

    def __init__(self, eng, seed, prob, slot, nsplits=2, gibbs=None):
        self.eng, self.seed, self.prob, self.slot, self.nsplits, self.gibbs = eng, seed, prob, slot, nsplits, gibbs

    def __call__(self, it, what=""):
        eng, seed, slot, prob = self.eng, self.seed, self.slot, self.prob
        T, W = eng.T, eng.W
        is_mh = pd.is_mh(seed, it, slot_weight(slot))
        nb = 1 if self.gibbs is None else len(self.gibbs["mh" if is_mh else "stretch"])
        ds = [eng.debug_draws(it, mh=slot is not None, block=b) for b in range(nb)]
        assert all(d["is_mh"] == is_mh for d in ds), f"{what}: the move choice"
        out = dict(is_mh=is_mh)
        if self.nsplits != 2:
            out["refs"] = [ru.draws_to_reference_sets(ds[0], T, W, self.nsplits)]
        elif is_mh:
            out["refs"] = [ru.draws_to_reference(ds[0], T, W)]
        else:
            if self.gibbs is not None:
                cb = pd.label_cb(T, W)
                for b, d in enumerate(ds):
                    want = gm.block_plan(seed, it, T, W, cb, b)
                    for k in ("own", "cw", "u_zz", "u_acc"):
                        assert np.array_equal(d[k], want[k]), f"{what}: {k} of block {b} differs from the specification's words"
            out["refs"] = [ru.draws_to_reference(d, T, W) for d in ds]
        if not is_mh:
            return out
        if slot[0] == "dist":
            check_dist_draws(ds[0], seed, it, T, W, slot[1], what)
            out.update(q=ds[0]["mh_step"], u_acc=ds[0]["mh_u"])
        elif slot[0] == "mt":
            tries = eng.mt_debug_draws(it)
            check_mt_draws(tries, ds[0], seed, it, T, W, slot[2], slot[1], what)
            out.update(q=tries[0], u_pick=tries[1], u_acc=tries[2])
        else:
            if slot[1] == "iso":
                for b, d in enumerate(ds):
                    z, u = gm.mh_block_draws(seed, it, T, W, eng.RW, b)
                    assert np.array_equal(d["mh_u"], u), f"{what}: accept uniforms of block {b}"
                    err = np.abs(d["mh_step"] - float(slot[2]) * z[..., :prob.D]).max()
                    assert err <= float(slot[2]) * pd.MH_NORMAL_E, f"{what}: a step of block {b} is {err / float(slot[2]):.2e} from the specification's normal"
            out.update(steps=[d["mh_step"] for d in ds], us=[d["mh_u"] for d in ds])
        return out


# ---- one iteration on the specification ------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def _oracle_on(prob, period, counts):
    """While open: the oracle's prior is the problem's (terms: tests/prior_terms.box_prior_substitute), and every red-blue half-step
    it makes is counted - accepted proposals per rung, and with a period the accepted proposals that the wrap moved."""
    saved_prior, real = orc.box_log_prior, orc.stretch_split
    per = None if period is None else np.asarray(period, dtype=np.float64)

    def stretch_split(x, L, P, betas, labels, split, rint, u_zz, u_acc, a, lo, hi, loglike, **kw):
        xb = x.copy() if per is not None else None
        out = real(x, L, P, betas, labels, split, rint, u_zz, u_acc, a, lo, hi, loglike, **kw)
        if counts is not None:
            counts.stretch_accepted += out["keep"].sum(axis=1)
            if per is not None and xb.shape[-1] == per.size:
                tt = np.arange(x.shape[0])[:, None]
                s, c = xb[tt, out["S"]], xb[tt, out["C"][tt, rint]]
                raw = c - orc.periodic_distance(s, c, per) * out["zz"][:, :, None]            # stretch.py:145, before the wrap
                on = per > 0
                moved = ((raw[..., on] < 0.0) | (raw[..., on] >= per[on])).any(axis=-1)
                counts.seam_wrapped_accepted += int((moved & out["keep"]).sum())
        return out

    if not is_box(prob):
        orc.box_log_prior = pt.box_prior_substitute(prob.prior)
    orc.stretch_split = stretch_split
    try:
        yield
    finally:
        orc.box_log_prior, orc.stretch_split = saved_prior, real


def _tail(st, ref, adaptive, lag, nu, stop_adaptation):
    """dist_move.pt_tail with the adaptation's switches: behind ``stop_adaptation`` the ladder stands and the time runs on
    (tempering.py:632-633, tests/replay_utils.oracle_iteration)."""
    stopped = adaptive and stop_adaptation >= 0 and st.time >= stop_adaptation
    dm.pt_tail(st, ref, adaptive=adaptive and not stopped, **{k: v for k, v in (("lag", lag), ("nu", nu)) if v is not None})
    if stopped and st.betas is not None and st.x.shape[0] > 1:
        st.time += 1


def _outside_period(x, period):
    on = np.asarray(period) > 0
    return ((x[..., on] < 0.0) | (x[..., on] >= np.asarray(period)[on])).any(axis=-1)


def spec_iteration(st, prob, slot, d, *, period=None, nsplits=2, lag=None, nu=None, adaptive=True, stop_adaptation=-1, gibbs=None, counts=None,
                   what=""):
    """One iteration of hens_step on the oracle state ``st`` with the draws ``d`` (``SpecDraws`` / ``DeviceDraws``).  ``counts``: a
    tests/move_interactions.Coverage.  Returns whether the iteration was the slot's."""
    T, W, D = st.x.shape
    adapt = {k: v for k, v in (("lag", lag), ("nu", nu)) if v is not None}
    ref = d["refs"][0]
    books = None if counts is None else counts.books
    if gibbs is not None:
        assert period is None and nsplits == 2 and books is not None, "Gibbs tables: two sets, no period (the library refuses the rest)"
    with _oracle_on(prob, period, counts if gibbs is None else None):
        if not d["is_mh"]:
            if gibbs is not None:
                before = books.acc["stretch"].sum(axis=0)
                gm.stretch_iteration(st, books, gibbs["stretch"], d["refs"], 2.0, prob.prior, prob.loglike)
                if counts is not None:
                    counts.stretch_accepted += books.acc["stretch"].sum(axis=0) - before
                _tail(st, ref, adaptive, lag, nu, stop_adaptation)
            else:
                ru.oracle_iteration(st, ref, prob.loglike, prob.lo, prob.hi, period=period, nsplits=nsplits, adaptive=adaptive,
                                    stop_adaptation=stop_adaptation, **adapt)
            return False
        if slot[0] == "gauss":
            if gibbs is not None:
                before = books.acc["mh"].sum(axis=0)
                gm.mh_iteration(st, books, gibbs["mh"], d["steps"], d["us"], prob.prior, prob.loglike)
                if counts is not None:
                    counts.slot_accepted += books.acc["mh"].sum(axis=0) - before
                _tail(st, ref, adaptive, lag, nu, stop_adaptation)
            else:
                acc0 = st.mh_accepted.copy()
                ru.oracle_iteration(st, ref, prob.loglike, prob.lo, prob.hi, mh=(d["steps"][0], d["us"][0]), period=period, adaptive=adaptive,
                                    stop_adaptation=stop_adaptation, **adapt)
                if counts is not None:
                    counts.slot_accepted += (st.mh_accepted - acc0).sum(axis=1).astype(int)
            return True
    # the generator moves: never wrapped (distgen.py, multipletry.py), the prior's terms by themselves
    info = {}
    if slot[0] == "dist":
        _, _, _, keep, fac = dm.dist_step(st.x, st.L, st.P, st.betas, d["q"], d["u_acc"], prob.prior, slot[1], prob.loglike, info=info)
        with np.errstate(divide="ignore"):
            knives = int(pu.knife_edge(info["lnpdiff"], np.log(info["u_acc"])).sum())
        old_out, picked = np.isneginf(fac), np.asarray(d["q"]).reshape(T, W, D)
    else:
        keep, pick, _, _, _ = mt.mt_step(st.x, st.L, st.P, st.betas, d["q"], d["u_pick"], d["u_acc"], prob.prior, slot[1], prob.loglike, info=info)
        ex = mt.exact_mt(info, pick, st.betas, prob.prior, slot[1])
        with np.errstate(divide="ignore"):
            knives = int(pu.knife_edge(info["lnpdiff"], np.log(info["u_acc"])).sum()) + int(mt.pick_knife(ex["c"], info["u_pick"], ex["B_c"]).sum())
        old_out = np.isneginf(info["alq"]).reshape(T, W)
        picked = info["q"].reshape(T * W, -1, D)[np.arange(T * W), pick.reshape(-1)].reshape(T, W, D)
        if counts is not None:
            counts.picks_beyond_0 += int((pick != 0).sum())
    assert knives == 0 or counts is not None, f"{what}: {knives} decisions on the knife edge: pick another seed"
    st.mh_accepted += keep
    if counts is not None:
        counts.knives += knives
        counts.slot_accepted += keep.sum(axis=1)
        counts.hottest_rejected += int((~keep[-1]).sum())
        counts.old_outside += int(old_out.sum())
        counts.old_outside_accepted += int((old_out & keep).sum())
        if period is not None:
            counts.slot_outside_period_accepted += int((keep & _outside_period(picked, period)).sum())
    _tail(st, ref, adaptive, lag, nu, stop_adaptation)
    return True


def run_spec(draws, st, prob, slot, calls, it0=0, counts=None, what="", **kw):
    """``calls`` of iterations from ``it0`` on the specification with the draws ``draws(it)``; returns the list of move kinds (True:
    the slot's).  A slot iteration directly behind a stretch iteration OF THE SAME CALL is counted: that is a pending adaptation
    at the move's launch."""
    kinds = []
    it = it0
    for n in calls:
        for k in range(n):
            kinds.append(spec_iteration(st, prob, slot, draws(it, f"{what}, iteration {it}"), counts=counts, what=f"{what}, iteration {it}", **kw))
            if counts is not None:
                counts.slot_iters += int(kinds[-1])
                counts.stretch_iters += int(not kinds[-1])
                counts.slot_after_stretch += int(k > 0 and kinds[-1] and not kinds[-2])
            it += 1
    return kinds


# ---- the replay of a context -------------------------------------------------------------------------------------------------------------------------
def compare(eng, st, prob, kinds, books, what):
    """The context's state and counters against the specification's, at the project's bars."""
    T = st.x.shape[0]
    xd, Ld, Pd, bd = eng.download()
    assert np.array_equal(xd, st.x), f"{what}: x differs from the specification in {int((xd != st.x).any(axis=-1).sum())} walkers " \
                                     f"(closest stretch decision margin {st.min_margin:.2e})"
    check_P(Pd, st.P, prob, xd, what)
    tol.check_logl(Ld, st.L, tol.RTOL_L, what)
    if st.betas is not None:
        np.testing.assert_allclose(bd, st.betas, rtol=1e-13, atol=0, err_msg=f"{what}: betas")
        assert np.array_equal(bd == 0.0, st.betas == 0.0), f"{what}: a beta = 0 rung is exactly 0"
    cs, cm = eng.counters(), eng.mh_counters()
    nslot = sum(kinds)
    if books is None:
        assert np.array_equal(cs["accepted"], st.accepted), f"{what}: stretch accept counters"
        assert np.array_equal(cm["accepted"], st.mh_accepted), f"{what}: the slot's accept counters"
        assert cm["num_proposals"] == nslot and cs["num_proposals"] == len(kinds) - nslot, f"{what}: proposal counts"
    else:                                  # Gibbs tables: a walker counts once per accepted block proposal, num_proposals once per block
        assert np.array_equal(cs["accepted"], books.accepted), f"{what}: stretch accept counters"
        assert np.array_equal(cm["accepted"], books.mh_accepted), f"{what}: the Gaussian move's accept counters"
        assert cs["num_proposals"] == books.num_proposals and cm["num_proposals"] == books.num_proposals_mh, f"{what}: num_proposals advances per block"
    if st.betas is not None and T > 1:
        assert np.array_equal(cs["swaps_total"], st.swaps_total), f"{what}: swap totals"
        assert np.array_equal(cs["swaps_last"], st.swaps_last), f"{what}: the last sweep's swap counts"
    assert st.min_margin > 1e-12, f"{what}: a stretch decision sat on the knife edge"
    assert books is None or (books.knives == 0 and books.min_margin > 1e-12), f"{what}: a block decision on the knife edge"
    return bd


def replay(eng, st, prob, slot, calls, *, seed, period=None, nsplits=2, lag=None, nu=None, adaptive=True, stop_adaptation=-1, gibbs=None,
           counts=None, what=""):
    """Step the context ``eng`` - set up by the caller: state uploaded and evaluated, the slot, the period, the set count, the
    tables, the adaptation's constants - through ``calls`` of hens_step and the oracle state ``st`` through the same iterations on
    the specification with the draws the context exports; compare after every call.  ``seed``: the context's.  ``gibbs``:
    dict(stretch=masks, mh=masks).  ``counts``: a tests/move_interactions.Coverage (with Gibbs tables its ``books`` are compared).
    Returns the move kinds, True for the slot's iterations."""
    draws = DeviceDraws(eng, seed, prob, slot, nsplits=nsplits, gibbs=gibbs)
    kinds = []
    for n in calls:
        it0 = eng.iteration()
        eng.step(n)
        eng.synchronize()
        kinds += run_spec(draws, st, prob, slot, (n,), it0=it0, counts=counts, what=what, period=period, nsplits=nsplits, lag=lag, nu=nu,
                          adaptive=adaptive, stop_adaptation=stop_adaptation, gibbs=gibbs)
        if counts is not None:
            assert counts.knives == 0, f"{what}: {counts.knives} decisions of the slot's move on the knife edge: pick another seed"
        compare(eng, st, prob, kinds, None if gibbs is None else counts.books, f"{what} after iteration {it0 + n - 1}")
    return kinds


def launch_counts(path, nm, nsplits=2, gibbs=None):
    """(n_stretch, n_pt, n_fused) a profiled call of two iterations, ``nm`` of them the slot's, reports on ``path`` (the counts
    tests/test_hip_dist_move.py::test_production_replay and tests/test_hip_gibbs.py::test_production_replay use): the move's launch is
    a stretch-kind launch followed by a cascade; a stretch iteration is one fused launch ("one"), an in-place launch and a fused one
    ("two"), or a copying launch per set and a cascade."""
    ns = 2 - nm
    if path == "one":
        return (nm, nm, ns)
    if path == "two":
        return (nm + ns, nm, ns)
    if path == "blocks":
        return (2 * len(gibbs["stretch"]) * ns + len(gibbs["mh"]) * nm, 2, 0)
    assert path in ("copying", "sets")
    return (nsplits * ns + nm, 2, 0)
