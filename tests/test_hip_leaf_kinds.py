"""Leaf kinds of one to four parameters evaluated on the device (hens_rj_set_model_kinds, the WIDE instantiations of k_rj; -m gpu).

The yardsticks are pinned elsewhere: the reference's eight chains with Lorentzian lines, chirps, ramps, bursts and offsets
(tests/golden/rjh1 - rjh4, rjn1 - rjn4), the oracle that reproduces them bit for bit (tests/test_oracle_golden_rj.py), the NumPy
statement of the kinds that is the oracle's likelihoods bit for bit and its exact-arithmetic bound (tests/test_leaf_kinds.py).
Bars: leaf masks, every slot's coordinates, log-prior and every decision exact; log-likelihood rtol 1e-12;
ladder rtol 1e-13; knife-edge decisions counted and asserted 0; against exact arithmetic |L - L*| <= 4 B."""
import numpy as np
import pytest

from oracle import eryn_oracle_rj as orj
from tests import exact_leaf_kinds as xk
from tests import leaf_kind_cases as cases
from tests import leaf_kinds as lk
from tests import tolerance_log as tol
from tests.test_oracle_golden_rj import NAMES_CALLABLE, NAMES_WIDTHS, load_rj

pytestmark = pytest.mark.gpu
RTOL_L, RTOL_BETA, BAR = 1e-12, 1e-13, 4.0
FIXTURE_KIND = {"gauss": "lorentz", "sine": "chirp", "ramp": "ramp", "burst": "burst", "offset": "offset"}


def knife(lnpdiff, u):                                           # tests/test_hip_rj.py's allowance
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(lnpdiff - np.log(u)) < 1e-12 * np.maximum(1.0, np.abs(lnpdiff))


class _Dangerous(int):
    """A walker count that passes the oracle's red / blue check (red_blue.py:103-114): all ``live_dangerously`` does in the reference."""

    def __lt__(self, other):
        return False


def _counting(base):
    """``base`` with the knife-edge decisions of its swaps counted (``knife_swaps``) and ``live`` = the reference's live_dangerously."""
    class Counting(base):
        knife_swaps, live = 0, False

        def _draw_pair(self, j, W):
            ip, i1p, u = super()._draw_pair(j, W)
            i = self.T - 1 - j
            dbeta = self.st.betas[i - 1] - self.st.betas[i]
            self.knife_swaps += int(knife(dbeta * (self.st.L[i, ip] - self.st.L[i - 1, i1p]), u).sum())
            return ip, i1p, u

        def stretch_move(self, rec=None):
            W = self.W
            if self.live:
                self.W = _Dangerous(W)
            try:
                return super().stretch_move(rec)
            finally:
                self.W = W
    return Counting


def _knife_accepts(rec):
    """Knife-edge accept tests among one recorded iteration's proposals."""
    n = 0
    if "mh_lnpdiff" in rec:
        n += int(knife(rec["mh_lnpdiff"], rec["mh_u_acc"]).sum())
    for h in range(2):
        if f"st_lnpdiff{h}" in rec:
            n += int(knife(rec[f"st_lnpdiff{h}"], rec[f"st_u_acc{h}"]).sum())
    if "rj_sub" in rec or "rj_lnpdiff" in rec:
        for sub in rec.get("rj_sub", [rec]):
            n += int(knife(sub["rj_lnpdiff"], sub["rj_u_acc"]).sum())
    return n


# ---- 1. the reference's chains, likelihood on the device ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES_CALLABLE + NAMES_WIDTHS)
def test_reference_chain_with_the_likelihood_on_the_device(golden_dir, name):
    """RJEnsembleSampler(log_like_fn=TemplateLikelihood(<kinds>)), rng="numpy", free-running from the fixture's two seeds: at every
    stored step the reference's leaf masks, coordinates of every slot and log-prior bit for bit, its log-likelihood to rtol 1e-12,
    its ladder to 1e-13; accept totals exact.  The oracle runs alongside (it IS the fixture, tests/test_oracle_golden_rj.py) to
    count knife-edge accept tests and swaps: none.  (The closest accept decision of these chains sits 2.0e-5 relative off its edge.)"""
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, StretchLeafMove, TemplateLikelihood
    from eryn_amd.state import State
    fx = load_rj(golden_dir, name)
    names = [str(k) for k in fx["branch_names"]] if "branch_names" in fx else ["gauss", "sine"]
    ndims = {k: len(fx[f"{k}_box"]) for k in names}
    n, T, W = int(fx["nsteps"]), int(fx["T"]), int(fx["W"])
    rj = None if str(fx["rj_moves"]) == "none" else str(fx["rj_moves"])
    stretch = str(fx["in_model"]) == "stretch"
    priors = {k: {i: uniform_dist(*fx[f"{k}_box"][i]) for i in range(ndims[k])} for k in names}
    move = StretchLeafMove() if stretch else GaussianLeafMove({k: np.eye(ndims[k]) * float(fx["cov_factor"]) for k in names})
    like = TemplateLikelihood({k: FIXTURE_KIND[k] for k in names}, fx["t"], fx["y"], float(fx["sigma"]))
    np.random.seed(int(fx["seed_construct"]))
    s = RJEnsembleSampler(W, ndims, like, priors, tempering_kwargs=dict(ntemps=T), nbranches=len(names), branch_names=names,
                          nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                          moves=move, rj_moves=rj)
    assert not s.engine.general and s.engine.wide and s.host_like is None
    # the oracle beside it, for the knife-edge counts
    cov = {k: np.eye(ndims[k]) * float(fx["cov_factor"]) for k in names}
    obr = [orj.Branch(k, 0, fx[f"{k}_box"], int(fx["nl_max"][i]), int(fx["nl_min"][i]), cov[k]) for i, k in enumerate(names)]
    o = _counting(orj.OracleRJSampler)(obr, {k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names}, fx["t"], fx["y"],
                                        float(fx["sigma"]), np.random.RandomState(int(fx["seed_construct"])),
                                        np.random.RandomState(int(fx["seed_run"])), fx["betas0"], record=True, schedule=rj or "none",
                                        in_model="stretch" if stretch else "gaussian",
                                        like_fn=lk.like_fn([FIXTURE_KIND[k] for k in names]))
    coords = {k: fx[f"x0_{k}"] for k in names}
    inds = {k: fx[f"inds0_{k}"] for k in names}
    L0, P0 = s._eval(coords, inds)
    assert np.array_equal(P0, fx["P0"])
    tol.check_logl(L0, fx["L0"], RTOL_L, f"{name}: initial log-like")
    np.random.seed(int(fx["seed_run"]))
    state = State(coords, log_like=fx["L0"], log_prior=fx["P0"], inds=inds)
    pre, worst_beta, knives = "mh" if rj is None else "rj", 0.0, 0
    for it in range(n):                                          # every stored step; a State carries dead slots' coordinates too
        state = s.run_mcmc(state, 1, store=False)
        o.iteration()
        knives += _knife_accepts(o.trace.pop())
        what = f"{name} step {it}"
        for k in names:
            assert np.array_equal(state.branches[k].inds, fx[f"it{it}_{pre}_inds_{k}"]), f"{what}: leaf masks of {k}"
            assert np.array_equal(state.branches[k].coords, fx[f"it{it}_{pre}_x_{k}"]), f"{what}: coordinates of {k}"
            assert np.array_equal(o.st.x[k], fx[f"it{it}_{pre}_x_{k}"]), "the oracle beside the chain is the fixture"
        assert np.array_equal(state.log_prior, fx[f"it{it}_{pre}_P"]), f"{what}: log-prior"
        tol.check_logl(state.log_like, fx[f"it{it}_{pre}_L"], RTOL_L, what)
        np.testing.assert_allclose(state.betas, fx[f"it{it}_{pre}_betas"], rtol=RTOL_BETA, atol=0, err_msg=what)
        worst_beta = max(worst_beta, float(np.max(np.abs(state.betas / fx[f"it{it}_{pre}_betas"] - 1))))
    assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"])
    if rj is not None:
        assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"]) and fx["rj_accepted_total"].sum() > 0
    print(f"{name}: worst beta distance {worst_beta:.3g}; knife-edge accepts {knives}, swaps {o.knife_swaps}")
    assert knives == 0 and o.knife_swaps == 0
    s.engine.close()


# ---- 2. eval_state against the helper -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ndata", [40, 257, 512])
@pytest.mark.parametrize("model", sorted(cases.MODELS))
def test_eval_state_equals_the_helper(model, ndata):
    """Random walkers from the boxes; one without any leaf, one with a coordinate outside its box (neither is evaluated: the fill
    value), one whose only leaves are in the last branch.  257 points: the second chunk of a lane's points begins ragged."""
    from eryn_amd.rj import RJEngine
    kinds = cases.MODELS[model]
    nl = (3, 3, 2)[:len(kinds)] if len(kinds) > 1 else (6,)
    brs = cases.branches_of(kinds, nl)
    rs = np.random.RandomState(7 + ndata)
    T, W = 2, 12
    t = np.linspace(-1, 1, ndata)
    sigma = cases.SIGMA[model]
    y = cases.make_data(brs, t, sigma, rs)
    x, inds = cases.random_state(brs, T, W, rs)
    for b in brs:
        inds[b.name][0, 0] = False
        inds[b.name][1, 5] = b is brs[-1]
    inds[brs[0].name][0, 3, 0] = True
    x[brs[0].name][0, 3, 0, -1] = brs[0].box[-1][1] + 0.25       # outside its box
    obr = [b.to_oracle() for b in brs]
    P = orj.compute_log_prior(x, inds, obr)
    L = orj.compute_log_like(x, inds, P, obr, t, y, sigma, like_fn=lk.like_fn(kinds))
    assert np.isneginf(P[0, 3]) and L[0, 3] == -1e300 and L[0, 0] == -1e300 and P[0, 0] == 0.0
    eng = RJEngine(T, W, [b.to_device() for b in brs], t, y, sigma)
    try:
        assert eng.wide and not eng.general
        eng.upload(x, inds, betas=np.array([1.0, 0.5]))
        eng.eval_state()
        xd, indd, Ld, Pd, _ = eng.download()
        for b in brs:
            assert np.array_equal(xd[b.name], x[b.name]) and np.array_equal(indd[b.name], inds[b.name])
        assert np.array_equal(Pd, P), "log-prior"
        tol.check_logl(Ld, L, RTOL_L, f"{model}, {ndata} points")
    finally:
        eng.close()


# ---- 3. production replay -------------------------------------------------------------------------------------------------------------
def _replay_class():
    from tests.test_hip_rj_stretch import _replay_stretch_class

    class ReplayWide(_counting(_replay_stretch_class())):
        """tests/test_hip_rj.py's replay oracle (its draw sources are what hens_rj_debug_draws / _stretch export) for branches of
        any width: a leaf's steps are its ``ndim`` record coordinates, a born leaf the first ``ndim`` entries of its birth row."""

        def _draw_steps(self, b, n):
            tt, ww, ll = np.where(self.st.inds[b.name])
            assert len(tt) == n
            idx = self.offsets[b.name] + ll[:, None] * b.ndim + np.arange(b.ndim)
            return self.d["step"][tt[:, None], ww[:, None], idx]

        def _draw_birth(self, b, bt, bw):
            rows = self.d["birth"][self._k()][bt, bw]
            assert rows.shape[1] == max(q.ndim for q in self.branches) and not rows[:, b.ndim:].any()
            return rows[:, :b.ndim]

    return ReplayWide


# noise widths of the replayed problems: a leaf moves the log-likelihood by a few units, so that births AND deaths are accepted on
# every branch within eight iterations of 27 - 44 walkers (checked with the oracle on its own draws before the first GPU run)
REPLAY_SIGMA = {"lorentz_chirp": 2.0, "ramp_burst": 3.0, "offset": 5.0, "mixed": 3.0}


def _problem(model, T, W, nl_max, nl_min, ndata, seed, start=None):
    if start is not None:                                        # a model, its data and a state made elsewhere (tests/limit_records.py)
        brs, t, y, sigma, x, inds = (start[k] for k in ("branches", "t", "y", "sigma", "x", "inds"))
        assert x[brs[0].name].shape[:2] == (T, W) and tuple(b.nleaves_max for b in brs) == tuple(nl_max)
    else:
        kinds = cases.MODELS[model]
        brs = cases.branches_of(kinds, nl_max, nl_min)
        rs = np.random.RandomState(seed)
        t = np.linspace(-1, 1, ndata)
        sigma = REPLAY_SIGMA[model]
        y = cases.make_data(brs, t, sigma, rs)
        x, inds = cases.random_state(brs, T, W, rs)
    scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in brs]
    betas0 = 0.35 ** np.arange(T)                                # (hot upper rungs)
    return brs, t, y, sigma, x, inds, scale, betas0


def _setup(model, T, W, nl_max, nl_min, ndata, seed, start=None, **kw):
    from eryn_amd.rj import RJEngine
    brs, t, y, sigma, x, inds, scale, betas0 = _problem(model, T, W, nl_max, nl_min, ndata, seed, start)
    return (RJEngine(T, W, [b.to_device() for b in brs], t, y, sigma, seed=seed, **kw), brs, t, y, sigma, x, inds, scale, betas0)


def _replay(model, T, W, nl_max, nl_min, ndata, iters, seed, schedule, in_model, calls=None, downloads=True, start=None, on_record=None):
    """hens_rj_step on Philox draws replayed through the oracle with ``like_fn`` = the helper.  Coverage is asserted from the oracle's
    side.  ``start``: dict(kinds, branches, t, y, sigma, x, inds) - the model, data and state in place of the harness's own random ones
    (``model`` then only names the case); ``on_record``: called with every iteration's trace record of the oracle.  Returns (worst
    relative log-likelihood distance, worst ladder distance)."""
    kinds = start["kinds"] if start is not None else cases.MODELS[model]
    ncoord = sum(n * lk.KINDS[k][1] for n, k in zip(nl_max, kinds))
    live = in_model == "stretch" and W < 2 * ncoord
    eng, brs, t, y, sigma, x, inds, scale, betas0 = _setup(model, T, W, nl_max, nl_min, ndata, seed, start=start, live_dangerously=live)
    names = [b.name for b in brs]
    try:
        eng.upload(x, inds, betas=betas0)
        eng.eval_state()
        if in_model == "stretch":
            eng.set_in_model("stretch")
        else:
            eng.set_mh_scale(scale)
        eng.set_schedule(schedule)
        x0, inds0, L0, P0, _ = eng.download()
        obr = [b.to_oracle(cov=np.diag(s ** 2)) for b, s in zip(brs, scale)]
        o = _replay_class()(obr, x0, inds0, t, y, sigma, None, None, betas0, schedule=schedule, in_model=in_model, record=True,
                            like_fn=lk.like_fn(kinds))
        o.live = live
        assert np.array_equal(o.st.P, P0) and np.isfinite(P0).all()
        worst_L = tol.check_logl(L0, o.st.L, RTOL_L, "initial log-like")
        worst_b = 0.0
        offsets = {b.name: eng.off[i] for i, b in enumerate(brs)}
        rj = schedule != "none"
        mh_acc, bd_acc, done, knives = np.zeros((T, W)), np.zeros((T, W)), 0, 0
        born, died = np.zeros(len(brs), dtype=int), np.zeros(len(brs), dtype=int)
        calls = calls or (iters // 2, iters - iters // 2)
        for n in calls:
            it0 = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for it in range(it0, it0 + n):
                o.load(eng.debug_draws(it), offsets, eng.debug_draws_stretch(it) if in_model == "stretch" else None)
                acc, bi, racc = o.iteration()
                rec = o.trace.pop()
                knives += _knife_accepts(rec)
                if on_record is not None:
                    on_record(rec)
                mh_acc += acc
                if rj:
                    bd_acc += racc
                    for sub in rec.get("rj_sub", [rec]):
                        bis = sub["rj_branches"] if "rj_branches" in sub else [sub["rj_branch"]]
                        chs = sub["rj_change_all"] if "rj_branches" in sub else [sub["rj_change"]]
                        for b_, ch in zip(bis, chs):
                            born[b_] += int(((ch == +1) & sub["rj_accepted"]).sum())
                            died[b_] += int(((ch == -1) & sub["rj_accepted"]).sum())
            done += n
            what = f"{model} {schedule} {in_model}: hens_rj_step vs oracle after {done} iterations"
            if not downloads and done < sum(calls):              # (no download: nothing refreshes the resident templates but the counter)
                xr, indr, Lr = eng.debug_resident()
                for k in names:
                    assert np.array_equal(indr[k], o.st.inds[k]) and np.array_equal(xr[k], o.st.x[k]), f"{what} (resident): {k}"
                worst_L = max(worst_L, tol.check_logl(Lr, o.st.L, RTOL_L, f"{what}: resident log-likelihood"))
                continue
            x1, inds1, L1, P1, betas1 = eng.download()
            for k in names:
                assert np.array_equal(inds1[k], o.st.inds[k]), f"{what}: leaf masks of {k}"
                assert np.array_equal(x1[k], o.st.x[k]), f"{what}: coordinates of {k} (dead slots included)"
            assert np.array_equal(P1, o.st.P), f"{what}: log-prior"
            worst_L = max(worst_L, tol.check_logl(L1, o.st.L, RTOL_L, what))
            np.testing.assert_allclose(betas1, o.st.betas, rtol=RTOL_BETA, atol=0, err_msg=what)
            worst_b = max(worst_b, float(np.max(np.abs(betas1 / o.st.betas - 1))))
            c = eng.counters()
            assert np.array_equal(c["accepted_mh"], mh_acc) and np.array_equal(c["accepted_bd"], bd_acc), f"{what}: accept counters"
            assert c["num_mh"] == done and c["num_bd"] == (done if rj else 0)
            assert np.array_equal(c["swaps_last"], o.swaps_accepted), f"{what}: swap counts of the last cascade"
        print(f"{model} {schedule} {in_model} {T}x{W} {ndata} points: log-like distance {worst_L:.3g}, ladder {worst_b:.3g}; in-model accepts "
              f"per rung {mh_acc.sum(axis=1).astype(int).tolist()}, births {born.tolist()}, deaths {died.tolist()}, swaps {o.swaps_sum.astype(int).tolist()}")
        assert knives == 0 and o.knife_swaps == 0, "knife-edge decisions"
        assert np.all(mh_acc.sum(axis=1) > 0), "an in-model accept on every rung"
        assert o.swaps_sum.sum() > 0, "a swap"
        if rj:
            for i, b in enumerate(brs):
                if b.nleaves_min != b.nleaves_max:
                    # (the one leaf of a one-leaf branch cannot die: fix_logp_gibbs gives the emptied branch's proposal -inf, or the
                    #  empty model the fill likelihood - tests/limit_records.py: required)
                    assert born[i] > 0 and (died[i] > 0 or b.nleaves_max == 1), f"an accepted birth and an accepted death on {b.name}"
        return worst_L, worst_b
    finally:
        eng.close()


NL = {"lorentz_chirp": ((3, 3), (1, 0)), "ramp_burst": ((3, 3), (0, 1)), "offset": ((6,), (1,)), "mixed": ((3, 3, 2), (0, 1, 0))}
SHAPE = {"separate_branches": (4, 9), "iterate_branches": (3, 12), "together": (3, 10), "none": (4, 11)}
# seeds of the cases whose default seed's eight iterations miss a birth or a death on some branch (the coverage the test asserts,
# counted from the oracle's side)
SEEDS = {}


@pytest.mark.parametrize("in_model", ["gaussian", "stretch"])
@pytest.mark.parametrize("schedule", sorted(SHAPE))
@pytest.mark.parametrize("model", sorted(cases.MODELS))
def test_production_step_replayed_through_the_oracle(model, schedule, in_model):
    T, W = SHAPE[schedule]
    _replay(model, T, W, NL[model][0], NL[model][1], ndata=40, iters=8, seed=SEEDS.get((model, schedule, in_model), 11),
            schedule=schedule, in_model=in_model)


def test_production_step_by_difference_on_257_points():
    """Resident templates of 257 points updated by +- one leaf (the second chunk of a lane's points ragged), every branch at once."""
    _replay("mixed", 3, 10, (3, 3, 2), (0, 1, 0), ndata=257, iters=8, seed=23, schedule="together", in_model="gaussian", downloads=False)


def test_production_step_across_the_refresh():
    """70 iterations without a download: the resident templates are rebuilt by the counter at iteration 63."""
    _replay("ramp_burst", 3, 10, (3, 3), (0, 1), ndata=40, iters=70, seed=29, schedule="separate_branches", in_model="gaussian",
            calls=(60, 10), downloads=False)


# ---- 4. resume ----------------------------------------------------------------------------------------------------------------------
def test_chain_resumed_in_a_fresh_context_is_the_uninterrupted_chain():
    snaps = []
    eng, brs, t, y, sigma, x, inds, scale, betas0 = _setup("ramp_burst", 3, 10, (3, 3), (0, 1), 40, 31)
    try:
        eng.upload(x, inds, betas=betas0)
        eng.eval_state()
        eng.set_mh_scale(scale)
        for _ in range(2):
            eng.step(5)
            snaps.append((eng.download(), eng.iteration(), eng.counters()["adapt_time"]))
    finally:
        eng.close()
    (x1, i1, L1, P1, b1), it1, at1 = snaps[0]
    (x2, i2, L2, P2, b2), it2, _ = snaps[1]
    assert any(not np.array_equal(i1[k], i2[k]) for k in i1), "the second half changes leaf masks"
    eng = _setup("ramp_burst", 3, 10, (3, 3), (0, 1), 40, 31)[0]
    try:
        eng.upload(x1, i1, L1, P1, b1)
        eng.set_iteration(it1)
        eng.set_adapt_time(at1)
        eng.set_mh_scale(scale)
        eng.step(5)
        xb, ib, Lb, Pb, bb = eng.download()
        assert eng.iteration() == it2 == 10
    finally:
        eng.close()
    for k in x2:
        assert np.array_equal(i2[k], ib[k]) and np.array_equal(x2[k], xb[k]), f"records of {k}"
    assert np.array_equal(P2, Pb) and np.array_equal(b2, bb)
    tol.check_logl(Lb, L2, RTOL_L, "resumed chain")


# ---- 5. pulses and sines through the new entry point ----------------------------------------------------------------------------------
def test_old_kinds_through_the_new_entry_point_step_bit_identically():
    """hens_rj_set_model_kinds with {pulse, sine} dispatches the instantiations hens_rj_set_model does - uniform-grid recurrences
    included (128 points on a linspace): the same chain bit for bit, log-likelihoods too, across the refresh at iteration 63."""
    from eryn_amd.rj import RJEngine
    T, W, N = 3, 16, 128
    brs = cases.branches_of(("pulse", "sine"), (3, 2))
    rs = np.random.RandomState(5)
    t = np.linspace(-1, 1, N)
    y = cases.make_data(brs, t, 2.0, rs, ninj=2)
    x, inds = cases.random_state(brs, T, W, rs)
    out = []
    for entry in (False, True):
        eng = RJEngine(T, W, [b.to_device() for b in brs], t, y, 2.0, seed=77, kinds_entry=entry)
        try:
            assert not eng.wide and not eng.general
            eng.upload(x, inds, betas=0.5 ** np.arange(T))
            eng.eval_state()
            eng.set_mh_scale([[2e-2, 2e-2, 2e-3], [2e-2, 2e-2, 2e-2]])
            eng.step(70)
            out.append((eng.debug_resident(), eng.download(), eng.counters()))
        finally:
            eng.close()
    (ra, da, ca), (rb, db, cb) = out
    for k in x:
        assert np.array_equal(ra[0][k], rb[0][k]) and np.array_equal(ra[1][k], rb[1][k]) and np.array_equal(da[0][k], db[0][k])
    assert np.array_equal(ra[2], rb[2]), "resident log-likelihoods"
    assert all(np.array_equal(da[j], db[j]) for j in (2, 3, 4)), "log-like, log-prior, ladder"
    assert np.array_equal(ca["accepted_mh"], cb["accepted_mh"]) and np.array_equal(ca["accepted_bd"], cb["accepted_bd"])
    assert ca["accepted_bd"].sum() > 0 and ca["accepted_mh"].sum() > 0


# ---- 6. against exact arithmetic ----------------------------------------------------------------------------------------------------
def _within_4B_of_exact(c):
    """The paths of test_log_like_within_4B_of_exact on the case ``c`` = dict(model, grid, branches, t, y, sigma, x, inds); returns
    (|L - L*| / B of eval_state, of the production step)."""
    from eryn_amd.rj import RJEngine
    model, grid = c["model"], c["grid"]
    brs = c["branches"]
    T, W = c["x"][brs[0].name].shape[:2]
    Ls, B = xk.yardstick(brs, c["x"], c["inds"], c["t"], c["y"], c["sigma"])
    live0 = sum(v.sum(axis=-1) for v in c["inds"].values()) > 0
    eng = RJEngine(T, W, [b.to_device() for b in brs], c["t"], c["y"], c["sigma"], seed=41)
    try:
        eng.upload(c["x"], c["inds"], betas=np.array([1.0, 0.3]))
        eng.eval_state()
        _, _, L, P, _ = eng.download()
        assert np.isfinite(P).all() and np.all(L[~live0] == -1e300)
        r_eval = float(np.max(np.where(live0, np.abs(L - Ls) / B, 0.0)))
        eng.set_mh_scale([np.array([1e-3 * (hi - lo) for lo, hi in b.box]) for b in brs])
        eng.step(1)
        xs, inds_s, Lr = eng.debug_resident()
        cnt = eng.counters()
        ever = {k: inds_s[k] | c["inds"][k] for k in inds_s}        # (a leaf that died still has its roundings in the template)
        Ls2, B2 = xk.yardstick(brs, xs, inds_s, c["t"], c["y"], c["sigma"], bound_inds=ever)
        live = sum(v.sum(axis=-1) for v in inds_s.values()) > 0
        assert np.all(Lr[~live] == -1e300)
        r_step = float(np.max(np.where(live, np.abs(Lr - Ls2) / B2, 0.0)))
    finally:
        eng.close()
    print(f"{model} on {grid}: |L_dev - L*| / B: eval {r_eval:.3g}, step {r_step:.3g}; accepted in-model {int(cnt['accepted_mh'].sum())}, "
          f"birth / death {int(cnt['accepted_bd'].sum())}")
    assert np.isfinite(Lr[live]).all() and r_eval <= BAR and r_step <= BAR
    assert cnt["accepted_mh"].sum() > 0 and cnt["accepted_bd"].sum() > 0, "an accepted production move of either kind"
    return r_eval, r_step


@pytest.mark.parametrize("model,grid", cases.ACCURACY_CASES)
def test_log_like_within_4B_of_exact(model, grid):
    """eval_state, and one production iteration (in-model move: full evaluation; birth / death: template +- one leaf) read back
    without a refresh.  Observed (MI355X): see DESIGN section 2."""
    c = cases.accuracy_case(model, grid)
    assert c["x"][c["branches"][0].name].shape[:2] == (cases.T_ACC, cases.W_ACC)
    _within_4B_of_exact(c)


# ---- 7. what is refused, and the sampler on device draws -----------------------------------------------------------------------------
def _sampler(rng, cov, **kw):
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, TemplateLikelihood
    names = ["ramp", "burst"]
    t = np.linspace(-1, 1, 40)
    brs = cases.branches_of(names, (3, 3))
    y = cases.make_data(brs, t, 0.5, np.random.RandomState(3))
    priors = {k: {i: uniform_dist(*cases.BOX[k][i]) for i in range(len(cases.BOX[k]))} for k in names}
    s = RJEnsembleSampler(10, {"ramp": 2, "burst": 4}, TemplateLikelihood({k: k for k in names}, t, y, 0.5), priors,
                          tempering_kwargs=dict(ntemps=3), branch_names=names, nleaves_max={"ramp": 3, "burst": 3},
                          moves=GaussianLeafMove(cov), rng=rng, seed=9, **kw)
    return s, brs, t, y


def test_refusals_and_the_sampler_on_device_draws():
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, TemplateBranch, TemplateLikelihood
    from eryn_amd.state import State
    full = {"ramp": np.array([[1e-3, 5e-4], [5e-4, 1e-3]]), "burst": np.eye(4) * 1e-3}
    with pytest.raises(NotImplementedError):
        _sampler("philox", full)
    with pytest.raises(ValueError):
        TemplateBranch("burst", "burst", cases.BOX["ramp"], 3)
    with pytest.raises(NotImplementedError):                     # ndims disagrees with the kind's width
        t = np.linspace(-1, 1, 8)
        RJEnsembleSampler(10, {"ramp": 3}, TemplateLikelihood({"ramp": "ramp"}, t, t, 1.0),
                          {"ramp": {i: uniform_dist(0.0, 1.0) for i in range(3)}}, tempering_kwargs=dict(ntemps=2), branch_names=["ramp"],
                          nleaves_max={"ramp": 2}, moves=GaussianLeafMove({"ramp": np.eye(3)}))
    s, brs, t, y = _sampler("philox", {"ramp": np.diag([1e-3, 2e-3]), "burst": np.diag([1e-3, 1e-4, 1e-4, 1e-2])})
    try:
        assert s.engine.wide
        with pytest.raises(NotImplementedError):
            s.engine.set_mh_chol(np.stack([np.eye(3)] * 2))
        with pytest.raises(NotImplementedError):                 # ... and the library itself
            from eryn_amd._lib import check, ptr
            check(s.engine.lib.hens_rj_set_mh_chol(s.engine.ctx, ptr(np.ascontiguousarray(np.stack([np.eye(3)] * 2)))), s.engine.ctx)
        x, inds = cases.random_state(brs, 3, 10, np.random.RandomState(4))
        last = s.run_mcmc(State(x, inds=inds), 6, thin_by=2, store=True)
        assert len(s.chain) == 6 and s.moves[0].num_proposals == 12 and s.rj_num_proposals_all == 12
        assert s.moves[0].accepted.sum() > 0 and s.rj_accepted_all.sum() > 0
        xs = {k: last.branches[k].coords for k in x}
        ii = {k: last.branches[k].inds for k in x}
        obr = [b.to_oracle() for b in brs]
        P = orj.compute_log_prior(xs, ii, obr)
        assert np.array_equal(last.log_prior, P)
        tol.check_logl(last.log_like, orj.compute_log_like(xs, ii, P, obr, t, y, 0.5, like_fn=lk.like_fn(["ramp", "burst"])), RTOL_L,
                       "stored log-like of the stored leaves")
    finally:
        s.engine.close()
    with pytest.raises(ValueError):                              # an unknown kind at the C interface
        from eryn_amd.rj import RJEngine
        b = TemplateBranch("r", "ramp", cases.BOX["ramp"], 2)
        b.kind = 9
        RJEngine(2, 8, [b], t, y, 0.5)
