"""Normal and log-uniform priors on leaf-packing records (hens_rj_set_prior_terms; -m gpu).

The yardsticks: tests/rj_prior_terms.py - ``TermBranch`` on the pinned oracle, the exact log-prior of a state and its a-priori bound,
the specification of the device's births - sized on the CPU by tests/test_rj_prior_terms.py.  Bars: leaf masks, every slot's
coordinates and every decision exact; -inf exactly where the specification has it; |P - P*| <= B; log-likelihood rtol 1e-12; ladder
rtol 1e-13; knife-edge decisions (1e-12, tests/test_hip_priors.py's rule) counted and asserted 0; uniform births bit for bit, log-uniform
and normal births within their bound."""

import numpy as np
import pytest

from tests import leaf_kinds as lk
from tests import prior_terms as pt
from tests import rj_prior_terms as rp
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
RTOL_L, RTOL_BETA = 1e-12, 1e-13


def _engine(brs, t, y, sigma, T, W, **kw):
    from eryn_amd.rj import RJEngine
    return RJEngine(T, W, rp.device_branches(brs), t, y, sigma, **kw)


def _assert_log_prior(P, brs, x, inds, what):
    r = rp.worst_state_ratio(P, brs, x, inds)
    assert r <= 1.0, f"{what}: |P - P*| is {r:.3f} of the bound"
    return r


# ---- 1. the evaluation matrix ---------------------------------------------------------------------------------------------------------
# a 3-parameter leaf on coordinates 63 - 65 (normal | log-uniform, uniform) and a 4-parameter leaf on 62 - 65 (log-uniform, normal |
# log-uniform, uniform): the slot's first coordinate is in the first pass of the per-coordinate phases, the rest in the second
MATRIX = ("three_across_64", "four_across_64")


def _matrix_model(name):
    if name == "three_across_64":
        kinds, nl = ("pulse", "sine"), (21, 4)
        across = ("sine", 0)                                      # 63 coordinates of pulses in front of it
    else:
        kinds, nl = ("offset", "burst"), (2, 17)
        across = ("burst", 15)                                    # 2 + 4 x 15 = 62
    brs = rp.branches_of(kinds, nl, (0,) * len(kinds))
    off = np.cumsum([0] + [b.nleaves_max * b.ndim for b in brs])
    b = [q for q in brs if q.name == across[0]][0]
    first = off[brs.index(b)] + across[1] * b.ndim
    assert first < 64 <= first + b.ndim - 1, "the leaf must straddle coordinate 64"
    return brs, across, off


@pytest.mark.parametrize("general", [False, True], ids=["device_likelihood", "host_likelihood"])
@pytest.mark.parametrize("name", sorted(MATRIX))
def test_eval_state_on_every_slot_pattern(name, general):
    """hens_eval_state under prior terms, on the kernels with a device likelihood (WIDE) and without one (k_rj<EVAL, -2>): one walker
    per pattern - all dead; one active leaf on either side of coordinate 64; the leaf across it alone, with a parameter on and just
    outside each finite bound in turn and a normal parameter at 1e200; every slot active - then the same with the dead slots holding
    0.0, negative values and 1e300: nothing may change."""
    from eryn_amd.rj import LeafBranch, RJEngine
    brs, (aname, aslot), off = _matrix_model(name)
    rs = np.random.RandomState(5)
    ab = [q for q in brs if q.name == aname][0]
    pats = []                                                     # (masks {name: [nl]}, overrides [(branch, slot, d, value)])
    none = {b.name: np.zeros(b.nleaves_max, dtype=bool) for b in brs}

    def only(*slots):
        m = {k: v.copy() for k, v in none.items()}
        for bn, s in slots:
            m[bn][s] = True
        return m
    pats.append((only(), []))
    pats.append((only((brs[0].name, 0)), []))                     # below coordinate 64
    pats.append((only((aname, ab.nleaves_max - 1)), []))          # at or past it
    pats.append((only((aname, aslot)), []))
    for d in range(ab.ndim):
        k = ab.spec["kind"][d]
        if k == pt.NORMAL:
            pats.append((only((aname, aslot)), [(aname, aslot, d, 1e200)]))
            pats.append((only((aname, aslot)), [(aname, aslot, d, -1e153)]))      # y y still finite
            continue
        for bound, out in ((ab.spec["lo"][d], -np.inf), (ab.spec["hi"][d], np.inf)):
            pats.append((only((aname, aslot)), [(aname, aslot, d, bound)]))
            pats.append((only((aname, aslot)), [(aname, aslot, d, np.nextafter(bound, out))]))
    pats.append(({b.name: np.ones(b.nleaves_max, dtype=bool) for b in brs}, []))
    T, W = 2, len(pats)                                           # (both rungs hold the same walkers)
    x = {b.name: np.repeat(b.rvs(W * b.nleaves_max, rs).reshape(1, W, b.nleaves_max, b.ndim), T, axis=0) for b in brs}
    inds = {b.name: np.repeat(np.stack([p[0][b.name] for p in pats])[None], T, axis=0) for b in brs}
    for w, (_, over) in enumerate(pats):
        for bn, s, d, v in over:
            x[bn][:, w, s, d] = v
    t = np.linspace(-1, 1, 40)
    y = 3.0 * rs.randn(40)
    if general:
        dev = [LeafBranch(b.name, b.container(), b.nleaves_max, 0) for b in brs]
        eng = RJEngine(T, W, dev, None, None, 1.0)
    else:
        eng = _engine(brs, t, y, 3.0, T, W)
    try:
        Ps = []
        for fill in (None, 0.0, -3.5, 1e300):
            xf = {k: v.copy() for k, v in x.items()}
            if fill is not None:
                for b in brs:
                    xf[b.name][~inds[b.name]] = fill
            eng.upload(xf, inds, betas=np.array([1.0, 0.5]))
            eng.eval_state()
            Ps.append(eng.download()[3])
        P = Ps[0]
        want = rp.exact_state_log_prior(brs, x, inds).astype(np.float64)
        assert (P[:, 0] == 0.0).all() and np.isneginf(want[0]).sum() == 2 * ab.ndim - 1 and np.isfinite(want[0]).sum() >= 8
        r = _assert_log_prior(P, brs, x, inds, name)
        print(f"{name} ({'host' if general else 'device'} likelihood): {W} patterns, {int(np.isneginf(P).sum())} with -inf, worst |P - P*| / B = {r:.3f}")
        for k, Pf in enumerate(Ps[1:]):
            assert np.array_equal(Pf, P), f"{name}: the contents of dead slots changed the log-prior (fill {k})"
    finally:
        eng.close()


# ---- 3. production stepping replayed through the oracle ----------------------------------------------------------------------------------
def _replay(c, name):
    from tests.test_hip_leaf_kinds import _knife_accepts, _replay_class
    brs, t, y, sigma, x, inds, betas0 = rp.case_problem(c)
    T, W, schedule, in_model, iters = c["T"], c["W"], c["schedule"], c["in_model"], c["iters"]
    ncoord = sum(b.nleaves_max * b.ndim for b in brs)
    live = in_model == "stretch" and W < 2 * ncoord
    eng = _engine(brs, t, y, sigma, T, W, seed=c["seed"], live_dangerously=live, a=c["a"])
    try:
        eng.upload(x, inds, betas=betas0)
        eng.eval_state()
        if in_model == "stretch":
            eng.set_in_model("stretch")
        else:
            eng.set_mh_scale(rp.scales(brs))
        eng.set_schedule(schedule)
        x0, inds0, L0, P0, _ = eng.download()
        o = _replay_class()(brs, x0, inds0, t, y, sigma, None, None, betas0, schedule=schedule, in_model=in_model, record=True, a=c["a"],
                            like_fn=lk.like_fn(c["kinds"]))
        o.live = live
        assert np.isfinite(P0).all()
        worst_P = _assert_log_prior(P0, brs, x0, inds0, f"{name}: initial log-prior")
        tol.check_logl(L0, o.st.L, RTOL_L, "initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(brs)}
        cnt, knives, done = rp.new_counts(len(brs)), 0, 0
        mh_acc, bd_acc = np.zeros((T, W)), np.zeros((T, W))
        for n in (1, iters - 1):
            it0 = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for it in range(it0, it0 + n):
                o.load(eng.debug_draws(it), offsets, eng.debug_draws_stretch(it) if in_model == "stretch" else None)
                acc, _, racc = o.iteration()
                rec = o.trace.pop()
                knives += _knife_accepts(rec)
                rp.count_record(cnt, rec, o)
                mh_acc += acc
                bd_acc += racc
            done += n
            what = f"{name}: hens_rj_step vs oracle after {done} iterations"
            x1, inds1, L1, P1, betas1 = eng.download()
            for b in brs:
                assert np.array_equal(inds1[b.name], o.st.inds[b.name]), f"{what}: leaf masks of {b.name}"
                assert np.array_equal(x1[b.name], o.st.x[b.name]), f"{what}: coordinates of {b.name} (dead slots included)"
            worst_P = max(worst_P, _assert_log_prior(P1, brs, x1, inds1, what))
            tol.check_logl(L1, o.st.L, RTOL_L, what)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=RTOL_BETA, atol=0, err_msg=what)
            cc = eng.counters()
            assert np.array_equal(cc["accepted_mh"], mh_acc) and np.array_equal(cc["accepted_bd"], bd_acc), f"{what}: accept counters"
            assert cc["num_mh"] == done and cc["num_bd"] == done
        print(f"{name}: worst |P - P*| / B = {worst_P:.3f}")
        rp.assert_coverage(cnt, 1, name)
        assert knives == 0 and o.knife_swaps == 0, "knife-edge decisions"
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(rp.CASES))
def test_production_step_under_mixed_priors_replayed_through_the_oracle(name):
    """hens_rj_step on device draws - every schedule, both in-model moves, a model of widths 1 to 4, a record of more than 64
    coordinates, calls split (1, n - 1) - replayed through the oracle on ``TermBranch``: the born coordinates are the device's own
    exports, so leaf masks and coordinates must agree bit for bit, the log-prior within the bound of exact arithmetic; births, deaths,
    -inf priors and prior-driven decisions are counted from the oracle's records."""
    _replay(rp.CASES[name], name)


# ---- 4. births -------------------------------------------------------------------------------------------------------------------------
def test_births_are_the_specification():
    """The born coordinates hens_rj_debug_draws exports (the kernel's own function on the same Philox words), per term kind against
    tests/rj_prior_terms.birth_spec; every value inside its support; the normal stream's statistics over three iterations of 2 x 512
    walkers x 4 normal parameters."""
    from tests.production_draws import normal_stream_stats, normal_stream_violations
    kinds, nl = ("offset", "ramp", "pulse", "burst"), (2, 2, 2, 2)
    T, W, seed = 2, 512, 77
    brs, t, y, sigma, x, inds, betas = rp.problem(kinds, T, W, nl, (0, 0, 0, 0), 40, 3, 3.0)
    eng = _engine(brs, t, y, sigma, T, W, seed=seed)
    try:
        eng.upload(x, inds, betas=betas)
        eng.eval_state()
        eng.set_mh_scale(rp.scales(brs))
        eng.set_schedule("together")                              # (every branch's births in one export)
        zs, worst = [], {pt.LOG_UNIFORM: 0.0, pt.NORMAL: 0.0}
        for it in range(3):
            birth = eng.debug_draws(it)["birth"]
            zrow = []
            for bi, b in enumerate(brs):
                assert not birth[bi][:, :, b.ndim:].any()
                for d in range(b.ndim):
                    words = rp.birth_words(seed, it, T, W, bi, d)
                    X, Xs, E = rp.birth_spec(b.spec, d, words)
                    got = birth[bi][:, :, d]
                    k = b.spec["kind"][d]
                    assert ((got >= b.spec["lo"][d]) & (got <= b.spec["hi"][d]) & np.isfinite(got)).all(), f"{b.name}[{d}]: a birth outside its support"
                    if k == pt.UNIFORM:
                        assert np.array_equal(got, X), f"{b.name}[{d}]: uniform births must be the specification bit for bit"
                        continue
                    err = np.abs(got.astype(rp.LD) - Xs).astype(np.float64)
                    worst[k] = max(worst[k], float((err / E).max()))
                    assert (err <= E).all(), f"{b.name}[{d}] (kind {k}): a birth is {float((err / E).max()):.2f} of its bound from the specification"
                    if k == pt.NORMAL:
                        zrow.append((got - b.spec["c0"][d]) / b.spec["c1"][d])
            zs.append(np.stack(zrow, axis=-1))
        z = np.stack(zs)                                          # [iterations, T, W, 4 normal parameters]
        s = normal_stream_stats(z, 0)
        print(f"births: worst distance / bound log-uniform {worst[pt.LOG_UNIFORM]:.3f}, normal {worst[pt.NORMAL]:.3f}; {z.size} normals: "
              + ", ".join(f"{k} {v:.2f}" for k, v in s.items() if k.startswith("z_")))
        assert normal_stream_violations(s) == [], normal_stream_violations(s)
    finally:
        eng.close()


# ---- 5. an all-uniform specification is the box ------------------------------------------------------------------------------------------
def _box_terms(brs):
    lo, hi = np.concatenate([b.lo for b in brs]), np.concatenate([b.hi for b in brs])
    return np.zeros(lo.shape[0], dtype=np.int32), lo, hi, np.log(1 / (hi - lo)), np.zeros_like(lo), np.zeros_like(lo)


def _set_terms(eng, kind, lo, hi, c0, c1, c2):
    from eryn_amd._lib import ptr
    arrs = [np.ascontiguousarray(kind, dtype=np.int32)] + [np.ascontiguousarray(a, dtype=np.float64) for a in (lo, hi, c0, c1, c2)]
    return eng.lib.hens_rj_set_prior_terms(eng.ctx, *[ptr(a) for a in arrs])


def _box_problem(T=3, W=12, ndata=130, seed=19):
    from tests import leaf_kind_cases as cases
    from eryn_amd.rj import TemplateBranch
    rs = np.random.RandomState(seed)
    cb = cases.branches_of(("pulse", "sine"), (4, 3), (0, 0))
    t = np.linspace(-1, 1, ndata)                                 # (more than 64 points on a linspace: the uniform-grid form of the box's kernels)
    y = cases.make_data(cb, t, 3.0, rs)
    x, inds = cases.random_state(cb, T, W, rs)
    brs = [TemplateBranch(b.name, b.kind, b.box, b.nleaves_max, b.nleaves_min) for b in cb]
    scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in cb]
    return brs, t, y, x, inds, scale, 0.35 ** np.arange(T)


def _chain(eng, x, inds, scale, betas, calls=(3, 4), schedule="separate_branches"):
    eng.upload(x, inds, betas=betas)
    eng.eval_state()
    eng.set_mh_scale(scale)
    eng.set_schedule(schedule)
    out = []
    for n in calls:
        eng.step(n)
        out.append((eng.download(), eng.counters()))
    return out


def _assert_same_chain(a, b, what):
    for ((xa, ia, La, Pa, ba), ca), ((xb, ib, Lb, Pb, bb), cb) in zip(a, b):
        for k in xa:
            assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"{what}: {k}"
        assert np.array_equal(La, Lb) and np.array_equal(Pa, Pb) and np.array_equal(ba, bb), f"{what}: log-probabilities / ladder"
        for k in ("accepted_mh", "accepted_bd", "swaps_total", "swaps_last"):
            assert np.array_equal(ca[k], cb[k]), f"{what}: counter {k}"


def test_an_all_uniform_specification_is_the_box():
    """hens_rj_set_prior_terms with uniform kinds only: chain and counters of the box model bit for bit - on 130 points of a linspace,
    where the box's kernels evaluate pulses and sines by recurrence and the kernels that carry terms per point: log-likelihoods that
    agree to the last bit say which kernels ran."""
    from eryn_amd.rj import RJEngine
    brs, t, y, x, inds, scale, betas = _box_problem()
    T, W = x["pulse"].shape[:2]
    a = RJEngine(T, W, brs, t, y, 3.0, seed=4)
    b = RJEngine(T, W, brs, t, y, 3.0, seed=4)
    try:
        assert _set_terms(b, *_box_terms(brs)) == 0
        ca, cb = _chain(a, x, inds, scale, betas), _chain(b, x, inds, scale, betas)
        _assert_same_chain(ca, cb, "all-uniform terms vs the box")
        assert ca[-1][1]["accepted_mh"].sum() > 0 and ca[-1][1]["accepted_bd"].sum() > 0
    finally:
        a.close(), b.close()


# ---- 6. sampler: device chain, resume -------------------------------------------------------------------------------------------------------
def _sampler(c, rng="philox", backend=None, callable_like=False):
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, StretchLeafMove, TemplateLikelihood
    brs, t, y, sigma, x, inds, betas = rp.case_problem(c)
    names = [b.name for b in brs]
    move = StretchLeafMove(a=c["a"], live_dangerously=True) if c["in_model"] == "stretch" else GaussianLeafMove({b.name: b.cov for b in brs})
    like = dict(log_like_fn=lk.like_fn(c["kinds"]), args=[t, y, sigma]) if callable_like else \
        dict(log_like_fn=TemplateLikelihood({b.name: b.kind_name for b in brs}, t, y, sigma))
    s = RJEnsembleSampler(c["W"], {b.name: b.ndim for b in brs}, priors={b.name: b.container() for b in brs},
                          tempering_kwargs=dict(ntemps=c["T"]), branch_names=names,
                          nleaves_max={b.name: b.nleaves_max for b in brs}, nleaves_min={b.name: b.nleaves_min for b in brs},
                          moves=move, rj_moves=c["schedule"], rng=rng, seed=c["seed"], backend=backend, **like)
    return s, brs, x, inds, betas


@pytest.mark.parametrize("name", ["separate_gaussian", "widths_1_to_4", "together_stretch"])
def test_device_chain_under_mixed_priors_is_the_host_chain(name):
    """RJEnsembleSampler(priors=containers, rng="philox") with and without RJDeviceBackend: the stored steps bit for bit; then a NEW
    context resumed from the returned State continues the uninterrupted chain bit for bit."""
    from eryn_amd.backend import RJDeviceBackend
    from eryn_amd.state import State
    from tests.test_hip_rj_chain_store import assert_chain_is_the_host_chain, assert_states_equal
    c = rp.CASES[name]
    host, brs, x, inds, betas = _sampler(c)
    dev = _sampler(c, backend=RJDeviceBackend())[0]
    try:
        assert host.engine.prior_terms
        last_h = host.run_mcmc(State(x, inds=inds, betas=betas), 6, burn=1)
        last_d = dev.run_mcmc(State(x, inds=inds, betas=betas), 6, burn=1)
        assert_chain_is_the_host_chain(dev.backend, host.chain, c["T"], name)
        assert_states_equal(last_d, last_h, f"{name}: the State run_mcmc returns")
        assert host.moves[0].accepted.sum() > 0 and host.rj_accepted_all.sum() > 0
        for s in host.chain:
            _assert_log_prior(s.log_prior, brs, {k: np.nan_to_num(v.coords) for k, v in s.branches.items()},
                              {k: v.inds for k, v in s.branches.items()}, name)
        # resume: a NEW context from the State run_mcmc returned (dead leaves' coordinates in place: the stretch move reads them)
        # continues as the context that made it does
        res = _sampler(c)[0]
        try:
            res.engine.upload(last_h.branches_coords, last_h.branches_inds, last_h.log_like, last_h.log_prior, last_h.betas)
            res.engine.set_iteration(host.engine.iteration())
            res.engine.set_adapt_time(host.engine.counters()["adapt_time"])
            for k in range(3):
                res.engine.step(1), host.engine.step(1)
                (xr, ir, Lr, Pr, br), (xh, ih, Lh, Ph, bh) = res.engine.download(), host.engine.download()
                for n_ in xr:
                    assert np.array_equal(ir[n_], ih[n_]) and np.array_equal(xr[n_], xh[n_]), f"{name}: resumed chain, step {k}, {n_}"
                assert np.array_equal(Lr, Lh) and np.array_equal(Pr, Ph) and np.array_equal(br, bh), f"{name}: resumed chain, step {k}"
            assert not all(np.array_equal(ih[n_], last_h.branches_inds[n_]) for n_ in ih), "the continued chain must move"
        finally:
            res.engine.close()
    finally:
        host.engine.close(), dev.engine.close()


# ---- 2. the parity API and the sampler on NumPy's draws -------------------------------------------------------------------------------------
def _numpy_oracle(c, brs, x, inds, t, y, sigma, betas, like_fn):
    from oracle import eryn_oracle_rj as orj
    from tests.test_hip_leaf_kinds import _counting
    o = _counting(orj.OracleRJSampler)(brs, x, inds, t, y, sigma, None, np.random, betas, schedule=c["schedule"], in_model=c["in_model"],
                                      record=True, a=c["a"], like_fn=like_fn)
    o.live = True
    return o


@pytest.mark.parametrize("callable_like", [False, True], ids=["template", "callable"])
@pytest.mark.parametrize("name", ["separate_gaussian", "together_stretch", "widths_1_to_4"])
def test_sampler_on_numpy_draws_is_the_oracle_chain(name, callable_like):
    """RJEnsembleSampler(rng="numpy") - the parity moves, births drawn by ``_draw_births`` from each parameter's distribution on the
    global stream - against the oracle on ``TermBranch`` fed from the same two streams: masks and coordinates bit for bit, log-prior
    within the bound, log-likelihood 1e-12 (a TemplateLikelihood) or exact (a Python callable: the host evaluates it), no knife edge."""
    from eryn_amd.state import State
    from tests.test_hip_leaf_kinds import _knife_accepts
    c = rp.CASES[name]
    _, t, y, sigma, _, _, _ = rp.case_problem(c)
    like_fn = lk.like_fn(c["kinds"])
    np.random.seed(31)
    s, brs, x, inds, betas = _sampler(c, rng="numpy", callable_like=callable_like)
    try:
        R = np.random.mtrand.RandomState()
        R.set_state(s._random.get_state())                        # (the sampler's clone of the global stream at construction)
        L0, P0 = s._eval(x, inds)
        np.random.seed(32)
        o = _numpy_oracle(c, brs, {k: v.copy() for k, v in x.items()}, {k: v.copy() for k, v in inds.items()}, t, y, sigma, betas.copy(), like_fn)
        o.R = R
        _assert_log_prior(P0, brs, x, inds, f"{name}: compute_log_prior")
        n = c["iters"]
        s.run_mcmc(State(x, inds=inds, betas=betas, log_like=o.st.L.copy(), log_prior=o.st.P.copy()), n)
        np.random.seed(32)
        knives = 0
        for k in range(n):
            o.iteration()
            knives += _knife_accepts(o.trace.pop())
            st = s.chain[k]
            what = f"{name}: iteration {k}"
            for b in brs:
                assert np.array_equal(st.branches[b.name].inds, o.st.inds[b.name]), f"{what}: leaf masks of {b.name}"
                live = o.st.inds[b.name]
                assert np.array_equal(st.branches[b.name].coords[live], o.st.x[b.name][live]), f"{what}: coordinates of {b.name}"
            _assert_log_prior(st.log_prior, brs, o.st.x, o.st.inds, what)
            tol.check_logl(st.log_like, o.st.L, RTOL_L, what)
        assert knives == 0 and o.knife_swaps == 0
        assert s.moves[0].accepted.sum() > 0 and sum(a.sum() for a in s.rj_accepted) > 0
    finally:
        s.engine.close()


@pytest.mark.parametrize("name", rp.FIXTURES)
def test_sampler_reproduces_the_reference_chain_under_mixed_priors(name):
    """The reference's chains of tests/golden/rj_priors/ (uniform_dist, log_uniform and scipy.stats.norm per branch): RJEnsembleSampler
    with the same constructor calls and the two seeds - every parity move, births from ``_draw_births`` - lands on every stored state:
    masks and coordinates bit for bit, log-prior within the bound of exact arithmetic, log-likelihood 1e-12, ladder 1e-13, accept
    counters exact.  (No decision of these chains is within 1e-12 of the knife edge: tests/test_rj_prior_golden.py.)"""
    from oracle import eryn_oracle_rj as orj
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, StretchLeafMove, TemplateLikelihood
    from eryn_amd.state import State
    from tests.test_oracle_golden_rj import LIKES
    fx = rp.load_fixture(name)
    names, brs = rp.fixture_names(fx), rp.fixture_branches(fx)
    n, T, W = int(fx["nsteps"]), int(fx["T"]), int(fx["W"])
    priors = {k: rp.fixture_container(fx[f"{k}_prior_kind"], fx[f"{k}_box"][:, 0], fx[f"{k}_box"][:, 1]) for k in names}
    move = StretchLeafMove() if str(fx["in_model"]) == "stretch" else GaussianLeafMove({b.name: b.cov for b in brs})
    if "model" in fx:
        like = dict(log_like_fn=getattr(orj, LIKES[str(fx["model"])]), args=[fx["t"], fx["y"], float(fx["sigma"])])
    else:
        like = dict(log_like_fn=TemplateLikelihood({b.name: b.kind_name for b in brs}, fx["t"], fx["y"], float(fx["sigma"])))
    np.random.seed(int(fx["seed_construct"]))
    s = RJEnsembleSampler(W, {b.name: b.ndim for b in brs}, priors=priors, tempering_kwargs=dict(ntemps=T), nbranches=len(names),
                          branch_names=names, nleaves_max=dict(zip(names, map(int, fx["nl_max"]))),
                          nleaves_min=dict(zip(names, map(int, fx["nl_min"]))), moves=move, rj_moves=str(fx["rj_moves"]), **like)
    try:
        assert np.array_equal(s.temperature_control.betas, fx["betas0"])
        coords, inds = {k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names}
        logp = s.compute_log_prior(coords, inds=inds)
        worst = _assert_log_prior(logp, brs, coords, inds, f"{name}: compute_log_prior")
        tol.check_logl(s.compute_log_like(coords, inds=inds, logp=logp)[0], fx["L0"], RTOL_L, "initial log-like")
        np.random.seed(int(fx["seed_run"]))
        s.run_mcmc(State(coords, log_like=fx["L0"], log_prior=fx["P0"], inds=inds), n, store=True)
        for it in range(n):
            st, pre = s.chain[it], f"it{it}_rj_"
            for k in names:
                m = fx[pre + f"inds_{k}"]
                assert np.array_equal(st.branches[k].inds, m), f"{name} it{it}: inds of {k}"
                assert np.array_equal(st.branches[k].coords[m], fx[pre + f"x_{k}"][m]), f"{name} it{it}: coordinates of {k}"
                assert np.isnan(st.branches[k].coords[~m]).all()
            x_it = {k: fx[pre + f"x_{k}"] for k in names}
            i_it = {k: fx[pre + f"inds_{k}"] for k in names}
            worst = max(worst, _assert_log_prior(st.log_prior, brs, x_it, i_it, f"{name} it{it}"))
            tol.check_logl(st.log_like, fx[pre + "L"], RTOL_L, f"{name} it{it}")
            np.testing.assert_allclose(st.betas, fx[pre + "betas"], rtol=RTOL_BETA, atol=0)
        last = s._state()
        for k in names:                                           # (the state itself: dead slots included)
            assert np.array_equal(last.branches[k].coords, fx[f"it{n - 1}_rj_x_{k}"]), f"{name}: every slot of {k} at the end"
        assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"])
        assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"])
        print(f"{name}: worst |P - P*| / B = {worst:.3f}")
    finally:
        s.engine.close()


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_context_as_it_was():
    """Every refusal of hens_rj_set_prior_terms with its code; after each one the context steps the chain of an untouched one."""
    from eryn_amd import _lib
    from eryn_amd._lib import ptr
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.rj import RJEngine, _TemplateLikelihood
    brs, t, y, x, inds, scale, betas = _box_problem(ndata=40)
    T, W = x["pulse"].shape[:2]
    kind, lo, hi, c0, c1, c2 = _box_terms(brs)

    def fresh():
        return RJEngine(T, W, brs, t, y, 3.0, seed=4)

    def mixed():
        k, l, h, a0, a1, a2 = kind.copy(), lo.copy(), hi.copy(), c0.copy(), c1.copy(), c2.copy()
        k[0], a0[0] = 1, np.log(np.log(h[0]) - np.log(l[0]))                      # pulse amplitude log-uniform on its box
        k[4], l[4], h[4], a0[4], a1[4], a2[4] = 2, -np.inf, np.inf, 5.0, 2.0, np.log(2.0)     # sine frequency normal
        return [k, l, h, a0, a1, a2]

    def bad(i, j, v):
        m = mixed()
        m[i][j] = v
        return m
    a = fresh()
    want = _chain(a, x, inds, scale, betas)
    a.close()
    Lc = np.ascontiguousarray(np.stack([np.diag(s) for s in scale]))
    refused = {
        "unknown kind": (bad(0, 1, 7), _lib.ERR_INVALID),
        "non-finite constant": (bad(3, 0, np.inf), _lib.ERR_INVALID),
        "NaN loc": (bad(3, 4, np.nan), _lib.ERR_INVALID),
        "scale 0": (bad(4, 4, 0.0), _lib.ERR_INVALID),
        "negative scale": (bad(4, 4, -1.0), _lib.ERR_INVALID),
        "log-uniform from 0": (bad(1, 0, 0.0), _lib.ERR_INVALID),
        "log-uniform to inf": (bad(2, 0, np.inf), _lib.ERR_INVALID),
        "empty support": (bad(2, 1, lo[1]), _lib.ERR_INVALID),
        "after hens_rj_set_mh_chol": (mixed(), _lib.ERR_UNSUPPORTED),
    }
    for what, (m, code) in refused.items():
        b = fresh()
        try:
            if what == "after hens_rj_set_mh_chol":
                b.set_mh_chol(Lc)
            assert _set_terms(b, *m) == code, what
            assert b.lib.hens_last_error(b.ctx), what
            _assert_same_chain(want, _chain(b, x, inds, scale, betas), f"after the refusal: {what}")
        finally:
            b.close()
    # full leaf covariances behind prior terms: refused, and the context steps under its terms - the chain of one that never asked
    c, d = fresh(), fresh()
    try:
        assert _set_terms(c, *mixed()) == 0 and _set_terms(d, *mixed()) == 0
        assert c.lib.hens_rj_set_mh_chol(c.ctx, ptr(Lc)) == _lib.ERR_UNSUPPORTED, "hens_rj_set_mh_chol after prior terms"
        cc, cd = _chain(c, x, inds, scale, betas), _chain(d, x, inds, scale, betas)
        _assert_same_chain(cc, cd, "after the refused covariances")
        assert np.isfinite(cc[-1][0][3]).all() and not np.array_equal(cc[-1][0][3], want[-1][0][3]), "the terms must be in force"
    finally:
        c.close(), d.close()
    # a context that is not a leaf-packing one, and a leaf-packing one before its model
    D = 8
    z = np.zeros(D)
    for like in (GaussianLikelihood(np.zeros(D), np.eye(D)), _TemplateLikelihood(D)):
        e = HipEnsemble(2, 32, D, like, -1.0, 1.0, tempered=True)
        try:
            assert e.lib.hens_rj_set_prior_terms(e.ctx, ptr(np.zeros(D, dtype=np.int32)), ptr(z - 1), ptr(z + 1), ptr(z), ptr(z), ptr(z)) == _lib.ERR_STATE
        finally:
            e.close()
