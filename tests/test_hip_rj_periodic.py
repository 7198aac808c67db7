"""Periodic leaf parameters on leaf-packing records on the device (-m gpu): hens_rj_set_periodic under every in-model entry point -
hens_rj_mh_step, hens_rj_stretch_split, hens_rj_group_step, hens_rj_gibbs_select + hens_rj_mh_step, hens_rj_propose / hens_rj_accept,
hens_rj_step - and ``RJEnsembleSampler(periodic=...)``, against the specification tests/rj_periodic.py and the chains captured from the
reference (tests/golden/rj_periodic/).  No test here reads the reference tree.  No accept decision of a fixture lies on a knife edge
(the generator asserts it)."""
import ctypes as C

import numpy as np
import pytest

from tests import periodic_seam as ps
from tests import rj_gibbs_move as rgm
from tests import rj_periodic as rp
from tests import tolerance_log as tol
from tests.test_hip_rj_gibbs import _assert_log_prior, _assert_state, _engine
from tests.test_hip_rj_group import _forced_rj

pytestmark = pytest.mark.gpu
RTOL_L = tol.RTOL_L         # teacher-forced: the device's exp / sin / summation order against the oracle's (tests/test_hip_rj.py)
RTOL_PROD = 1e-12           # production: the resident-template scheme against a full evaluation (tests/test_hip_rj_group.py, _gibbs.py)
TWO_PI = rp.TWO_PI


def _rows(periods, branches):
    return [periods[b.name] for b in branches]


def _full_steps(o, rec):
    """The oracle's per-leaf steps of a Gaussian move -> {name: [T, W, nl, nd]}."""
    out = {}
    for b in o.branches:
        out[b.name] = np.zeros(rec[f"pre_x_{b.name}"].shape)
        out[b.name][rec[f"pre_inds_{b.name}"]] = rec["mh_steps"][b.name]
    return out


def _assert_bits(eng, x, what):
    x1 = eng.download()[0]
    for k in x:
        assert ps.same_bits(x1[k], x[k]), f"{what}: bits of {k}, dead slots and wrapped zeros included"


# ---- teacher-forced: the four recorded chains --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", rp.FIXTURES)
def test_teacher_forced_chain_matches_the_specification_and_the_reference(name):
    """Every recorded iteration with the reference's draws through the move's own entry point under hens_rj_set_periodic: accept masks
    and records bit for bit against specification and fixture, log-likelihood to the teacher-forced bar."""
    fx = rp.load_fixture(name)
    o = rp.fixture_oracle(fx)
    kind = str(fx["in_model"])
    names = [b.name for b in o.branches]
    eng = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]), live_dangerously=True)
    try:
        eng.set_periodic(_rows(o.periods, o.branches))
        if kind == "group":
            eng.set_group(int(fx["nfriends"]), int(fx["n_iter_update"]), {k: int(v) for k, v in zip(fx["branch_names"], fx["key"])}, float(fx["a"]))
        if kind == "gibbs":
            eng.set_gibbs(rgm.table_of(o.blocks, o.branches))
        eng.upload({k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names}, o.st.L, o.st.P, fx["betas0"])
        for it in range(int(fx["nsteps"])):
            o.iteration()
            rec = o.trace.pop()
            what = f"{name} it{it}"
            if kind == "gaussian":
                keep = eng.mh_step(_full_steps(o, rec), rec["mh_u_acc"])
                assert np.array_equal(keep, rec["mh_accepted"]) and np.array_equal(keep, fx[f"it{it}_p0_keep"]), f"{what}: accept mask"
            elif kind == "stretch":
                for s in range(2):
                    keep = eng.stretch_split(s, rec["st_labels"], rec[f"st_rint{s}"], rec[f"st_u_zz{s}"], rec[f"st_u_acc{s}"])
                    assert np.array_equal(keep, rec[f"st_keep{s}"]) and np.array_equal(keep, fx[f"it{it}_p{s}_keep"]), f"{what}: accept mask of half {s}"
            elif kind == "group":
                if rec["rebuilt"]:
                    eng.group_rebuild()
                keep = eng.group_step(rec["picks"], rec["u_zz"], rec["u_acc"])
                assert np.array_equal(keep, rec["mh_accepted"]) and np.array_equal(keep, fx[f"it{it}_p0_keep"]), f"{what}: accept mask"
            else:
                for r in rec["gibbs"]:
                    eng.gibbs_select(r["block"])
                    keep = eng.mh_step(r["steps"], r["u_acc"])
                    assert np.array_equal(keep, r["accepted"]) and np.array_equal(keep, fx[f"it{it}_p{r['block']}_keep"]), f"{what}: block {r['block']}"
                    _assert_bits(eng, {n: r[f"upd_x_{n}"] for n in names}, f"{what} block {r['block']}")
            x = {k: rec[f"mhupd_x_{k}"] for k in names}
            _assert_state(eng, o.branches, x, {k: rec[f"mhupd_inds_{k}"] for k in names}, rec["mhupd_L"], rec["mhupd_P"], what + " behind the move")
            _assert_bits(eng, x, what + " behind the move")
            sel, _ = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
            assert np.array_equal(sel, rec["sel"]), f"{what}: swaps"
            _assert_bits(eng, {k: fx[f"it{it}_mh_x_{k}"] for k in names}, what + ": records against the reference")
            _forced_rj(eng, o, rec, what)
            _assert_state(eng, o.branches, o.st.x, o.st.inds, o.st.L, o.st.P, what + " behind the birth / death move")
            _assert_bits(eng, {k: fx[f"it{it}_rj_x_{k}"] for k in names}, what + ": records behind birth / death against the reference")
        f = o.facts.as_dict()
        assert f["wrapped_accepts"] >= 1 and f["dead_changed"] >= 1 and (kind not in ("stretch", "group") or f["short_way"] >= 1)
    finally:
        eng.close()


def test_propose_accept_carries_the_wrapped_proposal():
    """The Gaussian chain through hens_rj_propose / hens_rj_accept (k_rj<RJ_MODE_MH, -2>): hq is the wrapped proposal, dead slots
    included, bit for bit; the host hands back the specification's log-likelihoods."""
    from eryn_amd import _lib
    from eryn_amd._lib import check, ptr
    fx = rp.load_fixture("rjp_gauss")
    o = rp.fixture_oracle(fx)
    names = [b.name for b in o.branches]
    eng = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]))
    try:
        eng.set_periodic(_rows(o.periods, o.branches))
        for it in range(4):
            pre = {k: o.st.x[k].copy() for k in names}, {k: o.st.inds[k].copy() for k in names}, o.st.L.copy(), o.st.P.copy(), o.st.betas.copy()
            o.iteration()
            rec = o.trace.pop()
            eng.upload(*pre)
            st = np.ascontiguousarray(eng.steps_to_records(_full_steps(o, rec)))
            u = np.ascontiguousarray(rec["mh_u_acc"])
            dr = _lib.HensRjDraws(step=st.ctypes.data, u_acc=u.ctypes.data)
            q, logp, moved = np.empty((o.T, o.W, eng.RW)), np.empty((o.T, o.W)), np.empty((o.T, o.W), dtype=np.uint8)
            check(eng.lib.hens_rj_propose(eng.ctx, _lib.RJ_MOVE_MH, C.byref(dr), ptr(q), ptr(logp), ptr(moved)), eng.ctx)
            xq, iq = eng.unpack(q)
            for k in names:
                assert ps.same_bits(xq[k], rec["mh_q"][k]) and ps.same_bits(xq[k], fx[f"it{it}_p0_q_{k}"]), f"it{it}: hq of {k}"
                assert np.array_equal(iq[k], pre[1][k])
            assert np.array_equal(logp, rec["mh_logp"])
            ph = xq["sine"][..., 2]
            assert np.all((ph >= 0.0) & (ph < TWO_PI)), "every sine phase of hq, dead slots too, lies in [0, 2 pi)"
            keep = np.empty((o.T, o.W), dtype=np.uint8)
            check(eng.lib.hens_rj_accept(eng.ctx, ptr(np.ascontiguousarray(rec["mh_logl"])), ptr(keep)), eng.ctx)
            assert np.array_equal(keep.astype(bool), rec["mh_accepted"]) and np.array_equal(keep.astype(bool), fx[f"it{it}_p0_keep"])
            _assert_bits(eng, {k: rec[f"mhupd_x_{k}"] for k in names}, f"it{it}: records behind hens_rj_accept")
    finally:
        eng.close()


# ---- the sampler -------------------------------------------------------------------------------------------------------------------------------
def _fixture_sampler(fx, rng="numpy", backend=None, seed=None, periodic=rp.PERIODIC):
    from eryn_amd import rj
    from eryn_amd.prior import uniform_dist
    names = [str(k) for k in fx["branch_names"]]
    kinds = {"gauss": "pulse", "sine": "sine"}
    if "gauss_prior_kind" in fx:                                   # rjp_gibbs: log-uniform / normal leaf priors
        from tests import rj_prior_terms as rpt
        priors = {k: rpt.fixture_container(fx[f"{k}_prior_kind"], fx[f"{k}_box"][:, 0], fx[f"{k}_box"][:, 1]) for k in names}
    else:
        priors = {k: {i: uniform_dist(*fx[f"{k}_box"][i]) for i in range(3)} for k in names}
    sched = {"none": None, "together": True}.get(str(fx["rj_moves"]), str(fx["rj_moves"]))
    kind = str(fx["in_model"])
    if kind == "stretch":
        move = rj.StretchLeafMove(a=float(fx["a"]), live_dangerously=True)
    elif kind == "group":
        move = rj.GroupStretchLeafMove(int(fx["nfriends"]), {k: int(v) for k, v in zip(names, fx["key"])}, n_iter_update=int(fx["n_iter_update"]), a=float(fx["a"]))
    elif kind == "gibbs":
        move = rj.GibbsGaussianLeafMove({k: fx[f"cov_{k}"] for k in names}, list(rp.GIBBS_SETUP))
    else:
        move = rj.GaussianLeafMove({k: fx[f"cov_{k}"] for k in names})
    return rj.RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, rj.TemplateLikelihood({k: kinds[k] for k in names}, fx["t"], fx["y"], float(fx["sigma"])),
                                priors, tempering_kwargs=dict(ntemps=int(fx["T"])), nbranches=len(names), branch_names=names,
                                nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                                moves=move, rj_moves=sched, rng=rng, backend=backend, seed=seed, periodic=periodic)


@pytest.mark.parametrize("name", ["rjp_stretch", "rjp_gauss", "rjp_group", "rjp_gibbs"])
def test_numpy_sampler_lands_on_the_reference_chain(name):
    """RJEnsembleSampler(rng="numpy", periodic={"gauss": {}, "sine": {2: 2 pi}}) with the reference's seeds steps the reference's chain -
    StretchLeafMove, GaussianLeafMove with a full covariance, GroupStretchLeafMove, and GibbsGaussianLeafMove under log-uniform / normal
    leaf priors."""
    from eryn_amd.state import State
    fx = rp.load_fixture(name)
    names = [str(k) for k in fx["branch_names"]]
    n, obr = int(fx["nsteps"]), rp.fixture_branches(fx)
    np.random.seed(int(fx["seed_construct"]))
    s = _fixture_sampler(fx)
    try:
        assert s.engine.periods is not None and np.array_equal(s.engine.periods[1], [0.0, 0.0, TWO_PI])
        np.random.seed(int(fx["seed_run"]))
        start = State({k: fx[f"x0_{k}"] for k in names}, log_like=fx["L0"], log_prior=fx["P0"], inds={k: fx[f"inds0_{k}"] for k in names})
        last = s.run_mcmc(start, n, store=True)
        for it, st in enumerate(s.chain):
            pre = f"it{it}_rj_"
            for k in names:
                m = st.branches[k].inds
                assert np.array_equal(m, fx[pre + f"inds_{k}"]), f"{pre}inds of {k}"
                assert ps.same_bits(st.branches[k].coords[m], fx[pre + f"x_{k}"][m]), f"{pre}x of {k}"
            full = {k: np.where(st.branches[k].inds[..., None], st.branches[k].coords, 0.0) for k in names}
            _assert_log_prior(st.log_prior, fx[pre + "P"], obr, full, {k: st.branches[k].inds for k in names}, f"{name}: {pre}")
            tol.check_logl(st.log_like, fx[pre + "L"], 1e-12, f"{name}: {pre}log-like")
        pre = f"it{n - 1}_rj_"
        for k in names:
            assert ps.same_bits(last.branches[k].coords, fx[pre + f"x_{k}"]), f"coordinates of {k} (dead slots included)"
        np.testing.assert_allclose(last.betas, fx[pre + "betas"], rtol=1e-13, atol=0)
        assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"]) and s.moves[0].num_proposals == int(fx["mh_num_proposals"])
    finally:
        s.engine.close()


def test_device_backend_chain_equals_the_list_of_states():
    """rng="philox" with periodic=: six stored steps kept on the device are the list-of-States chain bit for bit, and every stored
    sine phase lies in [0, 2 pi)."""
    from eryn_amd.backend import RJDeviceBackend
    from eryn_amd.state import State
    from tests.test_hip_rj_chain_store import assert_chain_is_the_host_chain
    fx = rp.load_fixture("rjp_gauss")
    names = [str(k) for k in fx["branch_names"]]
    start = State({k: fx[f"x0_{k}"] for k in names}, inds={k: fx[f"inds0_{k}"] for k in names}, betas=fx["betas0"])
    s0 = _fixture_sampler(fx, "philox", seed=5, periodic=None)
    s1 = _fixture_sampler(fx, "philox", seed=5)
    s2 = _fixture_sampler(fx, "philox", backend=RJDeviceBackend(), seed=5)
    try:
        for s in (s0, s1, s2):
            s.run_mcmc(start, 6, thin_by=2)
        assert len(s1.chain) == 6 and s2.chain == []
        assert_chain_is_the_host_chain(s2.backend, s1.chain, int(fx["T"]), "periodic leaf parameters")
        ph = np.concatenate([st.branches["sine"].coords[..., 2][st.branches["sine"].inds] for st in s1.chain])
        assert ph.size and np.all((ph >= 0.0) & (ph < TWO_PI))
        assert any(not np.array_equal(a.branches["sine"].coords[a.branches["sine"].inds], b.branches["sine"].coords[b.branches["sine"].inds])
                   or not np.array_equal(a.branches["sine"].inds, b.branches["sine"].inds) for a, b in zip(s0.chain, s1.chain)), "periodic= changes the chain"
    finally:
        for s in (s0, s1, s2):
            s.engine.close()


# ---- production: hens_rj_step replayed through the specification --------------------------------------------------------------------------------
def _replay_class(move):
    from tests.test_hip_leaf_kinds import _replay_class as base_replay
    base = base_replay()
    if move == "group":
        class Replay(rp.PeriodicGroupOracle, base):
            def _draw_picks(self, bi, b, nf, going):
                p = self.gd["picks"][b.name][going]
                assert np.all((p >= 0) & (p < nf))
                return p

            def _draw_zz_group(self):
                return self.gd["u_zz"]

            def _draw_accept(self, which):
                return self.gd["u_acc"] if which == "mh" else super()._draw_accept(which)
    elif move == "gibbs":
        class Replay(rp.PeriodicGibbsOracle, base):
            def _draw_block_steps(self, k, b, n):
                tt, ww, ll = np.where(rgm.moved_leaves(self.blocks[k], self.st.inds)[b.name])
                assert len(tt) == n
                idx = self.offsets[b.name] + ll[:, None] * b.ndim + np.arange(b.ndim)
                return self.gd[k]["step"][tt[:, None], ww[:, None], idx]

            def _draw_block_accept(self, k):
                return self.gd[k]["u_mh"]
    else:
        class Replay(rp.PeriodicOracle, base):
            pass
    return Replay


def _production_engine(p, seed, periodic=True, **kw):
    from eryn_amd.rj import RJEngine
    eng = RJEngine(p["T"], p["W"], [b.to_device() for b in p["branches"]], p["t"], p["y"], p["sigma"], seed=seed, **kw)
    if periodic:
        eng.set_periodic(p["periodic"])
    if p["move"] == "group":
        eng.set_group(3, 3, p["key"], 2.0)
        eng.set_in_model("group")
    elif p["move"] == "stretch":
        eng.set_in_model("stretch")
    elif p["chol"] is not None:
        eng.set_mh_chol(p["chol"])
    else:
        eng.set_mh_scale(p["scale"])
    if p["move"] == "gibbs":
        eng.set_gibbs(rgm.table_of(rgm.parse_setup([b.name for b in p["obr"]], p["obr"]), p["obr"]))
    eng.upload(p["x"], p["inds"], betas=p["betas"])
    eng.eval_state()
    eng.set_schedule(p["schedule"])
    return eng


def _knife(lnpdiff, u, beta_L):
    scale = np.where(np.abs(beta_L) >= 1e299, 1.0, np.maximum(np.abs(beta_L), 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return (np.abs(lnpdiff - np.log(u)) <= RTOL_PROD * scale) & np.isfinite(lnpdiff)


def _decisions(rec, move):
    if move == "gaussian":
        return [(rec["mh_lnpdiff"], rec["mh_u_acc"], rec["betas_before"][:, None] * rec["mh_logl"])]
    if move == "stretch":
        return [(rec[f"st_lnpdiff{s}"], rec[f"st_u_acc{s}"], rec["betas_before"][:, None] * rec[f"st_logl{s}"]) for s in range(2)]
    if move == "group":
        return [(rec["lnpdiff"], rec["u_acc"], rec["betas_before"][:, None] * rec["logl"])]
    return [(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]) for r in rec["gibbs"]]


@pytest.mark.parametrize("name", sorted(rp.PRODUCTION_CASES))
def test_production_step_replayed_through_the_specification(name):
    """hens_rj_step (rng="philox") for 12 iterations from phases seeded at the seam, replayed through the specification with the draws
    the device consumed: records bit for bit, masks, log-priors and counters exact, log-likelihoods to 1e-12, the ladder to 1e-13.  The
    replay must have seen wrapped accepts, and for the stretch-type moves short-way-round differences."""
    p = rp.production_problem(name)
    move = p["move"]
    eng = _production_engine(p, seed=17)
    try:
        assert eng.wide == p["wide"]
        x0, inds0, L0, P0, _ = eng.download()
        q = dict(p, x=x0, inds=inds0)
        o = rp.production_oracle(q, cls_of=lambda cls: _replay_class(move))
        o.live = True
        assert np.array_equal(o.st.P, P0)
        tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        nb = len(o.blocks) if move == "gibbs" else 1
        mh_acc, done, past_64 = np.zeros((p["T"], p["W"])), 0, 0
        last = p["branches"][-1].name
        for n in (2, rp.PRODUCTION_ITERS - 2):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                o.load(eng.debug_draws(i), offsets, eng.debug_draws_stretch(i) if move == "stretch" else None)
                if move == "group":
                    o.gd = eng.group_debug_draws(i)
                if move == "gibbs":
                    o.gd = [eng.gibbs_debug_draws(i, k) for k in range(nb)]
                o.iteration()
                rec = o.trace.pop()
                for lnpdiff, u, bl in _decisions(rec, move):
                    assert not _knife(lnpdiff, u, bl).any(), f"{name} iteration {i}: a decision on a knife edge (choose another seed)"
                if move == "gibbs":
                    for r in rec["gibbs"]:
                        mh_acc += r["accepted"]
                else:
                    mh_acc += rec["mh_accepted"]
                if name == "record_past_64":          # (sine slots 10 and 11: record coordinates 68 and 71)
                    raw, act = rec["mh_raw"][last][..., 10:, 2], rec[f"pre_inds_{last}"][..., 10:]
                    past_64 += int(((act & ((raw < 0.0) | (raw >= TWO_PI))).any(axis=-1) & rec["mh_accepted"]).sum())
            done += n
            what = f"{name}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=RTOL_PROD)
            _assert_bits(eng, o.st.x, what)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc) and cn["num_mh"] == done * nb, what
        f = o.facts.as_dict()
        print(name, f)
        assert f["wrapped_accepts"] >= 1 and f["rejected"] >= 1, f
        if move in ("stretch", "group"):
            assert f["short_way"] >= 1, f
        if name == "record_past_64":
            assert eng.off[1] + 10 * 3 + 2 >= 64 and past_64 >= 1, "an accepted proposal wrapped a periodic coordinate with record index >= 64"
    finally:
        eng.close()


# ---- invariance ------------------------------------------------------------------------------------------------------------------------------------
def _chain(p, seed, setup):
    """12 production iterations -> the downloaded state; ``setup(eng)`` runs before the upload."""
    from eryn_amd.rj import RJEngine
    eng = RJEngine(p["T"], p["W"], [b.to_device() for b in p["branches"]], p["t"], p["y"], p["sigma"], seed=seed)
    try:
        setup(eng)
        if p["move"] == "stretch":
            eng.set_in_model("stretch")
        elif p["move"] == "group":
            eng.set_group(3, 3, p["key"], 2.0)
            eng.set_in_model("group")
        else:
            eng.set_mh_scale(p["scale"])
        eng.upload(p["x"], p["inds"], betas=p["betas"])
        eng.eval_state()
        eng.set_schedule(p["schedule"])
        eng.step(rp.PRODUCTION_ITERS)
        return eng.download(), eng.counters()["accepted_mh"].copy()
    finally:
        eng.close()


def _same_chain(a, b, what):
    (xa, ia, La, Pa, ba), ca = a
    (xb, ib, Lb, Pb, bb), cb = b
    for k in xa:
        assert ps.same_bits(xa[k], xb[k]) and np.array_equal(ia[k], ib[k]), f"{what}: {k}"
    assert ps.same_bits(La, Lb) and ps.same_bits(Pa, Pb) and ps.same_bits(ba, bb) and np.array_equal(ca, cb), what


@pytest.mark.parametrize("name", ["gaussian", "stretch", "group"])
def test_without_periods_the_chain_is_the_chain_of_a_context_that_never_heard_of_them(name):
    """period = NULL, all zeros, and set-then-cleared: bit-identical to a context built only from the calls the parent commit has.  And a
    period on a parameter whose box, steps and dead slots keep every value strictly inside (0, period) and every pair closer than half
    a period - the pulse amplitude in (2.5, 3.5) under period 8 - is the identity: the same chain again."""
    p = rp.production_problem(name)
    nb = len(p["branches"])
    plain = _chain(p, 23, lambda e: None)
    assert plain[1].sum() > 0
    null = _chain(p, 23, lambda e: e.set_periodic(None))
    zeros = _chain(p, 23, lambda e: e.set_periodic([np.zeros(3)] * nb))

    def set_and_clear(e):
        e.set_periodic(p["periodic"])
        e.set_periodic(None)
    cleared = _chain(p, 23, set_and_clear)
    for other, what in ((null, "NULL"), (zeros, "all zeros"), (cleared, "set and cleared")):
        _same_chain(plain, other, f"{name}: {what}")
    first = p["branches"][0].name
    assert np.all((p["x"][first][..., 0] > 2.5) & (p["x"][first][..., 0] < 3.5)), "every slot's amplitude, dead ones too, inside (0, 8)"
    inside = _chain(p, 23, lambda e: e.set_periodic({first: {0: 8.0}}))
    _same_chain(plain, inside, f"{name}: a period that never bites")
    on = _chain(p, 23, lambda e: e.set_periodic(p["periodic"]))
    last = p["branches"][-1].name
    assert not ps.same_bits(on[0][0][last], plain[0][0][last]), "the periods that do bite change the chain"


# ---- order independence ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("setter", ["mh_scale", "mh_chol", "prior_terms", "gibbs", "group"])
def test_the_period_row_survives_every_setter_that_rebuilds_the_table(setter):
    """hens_rj_set_periodic then the setter, and the other way round: the same teacher-forced Gaussian (group: group) move, wrapped."""
    fx = rp.load_fixture("rjp_gauss")
    o = rp.fixture_oracle(fx)
    names = [b.name for b in o.branches]
    o.iteration()
    rec = o.trace.pop()
    rows = _rows(o.periods, o.branches)

    def apply(eng):
        if setter == "mh_scale":
            eng.set_mh_scale([np.full(3, 0.01)] * 2)
        elif setter == "mh_chol":
            eng.set_mh_chol(np.stack([0.01 * np.eye(3)] * 2))
        elif setter == "prior_terms":
            from eryn_amd import rj as rjm                     # (the branches' own uniform terms: the same prior, through the setter)
            from eryn_amd._lib import check, ptr
            check(eng.lib.hens_rj_set_prior_terms(eng.ctx, *map(ptr, rjm.term_arrays([b.terms for b in eng.branches]))), eng.ctx)
        elif setter == "gibbs":
            eng.set_gibbs(np.ones((1, eng.ncoord), dtype=bool))
        else:
            eng.set_group(3, 3, 1, 2.0)

    out = []
    for order in (0, 1):
        eng = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]))
        try:
            if order == 0:
                eng.set_periodic(rows)
                apply(eng)
            else:
                apply(eng)
                eng.set_periodic(rows)
            eng.upload({k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names}, fx["L0"], fx["P0"], fx["betas0"])
            if setter == "group":
                eng.group_rebuild()
                picks = {k: np.zeros(fx[f"inds0_{k}"].shape, dtype=np.int32) for k in names}
                keep = eng.group_step(picks, np.full((o.T, o.W), 0.5), np.full((o.T, o.W), 1e-300))
            else:
                keep = eng.mh_step(_full_steps(o, rec), rec["mh_u_acc"])
                assert np.array_equal(keep, rec["mh_accepted"]), f"{setter}, order {order}: the wrapped move's accept mask"
                _assert_bits(eng, {k: rec[f"mhupd_x_{k}"] for k in names}, f"{setter}, order {order}")
            x1 = eng.download()[0]
            ph = x1["sine"][..., 2][keep]
            assert keep.any() and np.all((ph >= 0.0) & (ph < TWO_PI)), f"{setter}, order {order}: an accepted walker's dead-slot phases are wrapped"
            out.append((x1, keep))
        finally:
            eng.close()
    for k in names:
        assert ps.same_bits(out[0][0][k], out[1][0][k]), f"{setter}: both orders"
    assert np.array_equal(out[0][1], out[1][1])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_keep_code_and_text_and_change_nothing():
    from eryn_amd import _lib
    from eryn_amd._lib import ptr
    fx = rp.load_fixture("rjp_stretch")
    o = rp.fixture_oracle(fx)
    names = [b.name for b in o.branches]
    o.iteration()
    rec = o.trace.pop()
    eng = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]), live_dangerously=True)
    lib, ctx = eng.lib, eng.ctx
    good = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, TWO_PI]])
    start = {k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names}, fx["L0"], fx["P0"], fx["betas0"]

    def still_periodic(what):
        """The context still steps the wrapped half-steps of the recorded chain: the periods are what they were."""
        eng.upload(*start)
        for s in range(2):
            keep = eng.stretch_split(s, rec["st_labels"], rec[f"st_rint{s}"], rec[f"st_u_zz{s}"], rec[f"st_u_acc{s}"])
            assert np.array_equal(keep, rec[f"st_keep{s}"]), what
        _assert_bits(eng, {k: rec[f"mhupd_x_{k}"] for k in names}, what)

    def refused(code, text, period):
        assert lib.hens_rj_set_periodic(ctx, ptr(period)) == code
        assert lib.hens_last_error(ctx).decode() == text
        still_periodic(text)

    try:
        eng.set_periodic([good[0], good[1]])
        still_periodic("before any refusal")
        for bad in (-1.0, np.nan, np.inf):
            per = good.copy()
            per[1, 1] = bad
            refused(_lib.ERR_INVALID, "hens_rj_set_periodic: period of branch 1, parameter 1 must be finite and >= 0", per)
        # between the two stretch half-steps
        eng.upload(*start)
        eng.stretch_split(0, rec["st_labels"], rec["st_rint0"], rec["st_u_zz0"], rec["st_u_acc0"])
        assert lib.hens_rj_set_periodic(ctx, None) == _lib.ERR_STATE
        assert lib.hens_last_error(ctx).decode() == "hens_rj_set_periodic between the half-steps of a move"
        keep = eng.stretch_split(1, rec["st_labels"], rec["st_rint1"], rec["st_u_zz1"], rec["st_u_acc1"])
        assert np.array_equal(keep, rec["st_keep1"])
        _assert_bits(eng, {k: rec[f"mhupd_x_{k}"] for k in names}, "the second half-step is still the periodic one")
        # while hens_rj_accept is pending
        eng.upload(*start)
        labels = np.ascontiguousarray(rec["st_labels"], dtype=np.uint8)
        ri = np.ascontiguousarray(rec["st_rint0"], dtype=np.int64)
        uz, ua = np.ascontiguousarray(rec["st_u_zz0"]), np.ascontiguousarray(rec["st_u_acc0"])
        dr = _lib.HensRjDraws(split=0, labels=labels.ctypes.data, rint=ri.ctypes.data, u_zz=uz.ctypes.data, u_acc=ua.ctypes.data)
        q, logp, moved = np.empty((o.T, o.W, eng.RW)), np.empty((o.T, o.W)), np.empty((o.T, o.W), dtype=np.uint8)
        assert lib.hens_rj_propose(ctx, _lib.RJ_MOVE_STRETCH, C.byref(dr), ptr(q), ptr(logp), ptr(moved)) == 0, lib.hens_last_error(ctx).decode()
        assert lib.hens_rj_set_periodic(ctx, None) == _lib.ERR_STATE
        assert lib.hens_last_error(ctx).decode() == "hens_rj_accept must follow hens_rj_propose"
        xq = eng.unpack(q)[0]
        tt = np.arange(o.T)[:, None]
        assert ps.same_bits(xq["sine"][tt, rec["st_S0"]], rec["st_q0"]["sine"]), "hq of the stretch half-step is the wrapped proposal"
        assert lib.hens_rj_accept(ctx, ptr(np.full((o.T, o.W), -np.inf)), None) == 0
        still_periodic("after the refusals in flight")
    finally:
        eng.close()
    # a parameter index >= the branch's nd; a context that is not leaf-packing
    from tests import leaf_kind_cases as cases
    from eryn_amd.rj import RJEngine
    brs = cases.branches_of(("ramp", "burst"), (2, 2))
    rs = np.random.RandomState(3)
    t = np.linspace(-1, 1, 40)
    y = cases.make_data(brs, t, 1.0, rs)
    x, inds = cases.random_state(brs, 2, 8, rs)
    chains = []
    for refuse in (True, False):                              # the refused call leaves the chain of a context that never made it
        e2 = RJEngine(2, 8, [b.to_device() for b in brs], t, y, 1.0, seed=9)
        try:
            if refuse:
                per = np.zeros((2, 4))
                per[0, 2] = 1.0                                   # the ramp has parameters 0 and 1
                assert e2.lib.hens_rj_set_periodic(e2.ctx, ptr(per)) == _lib.ERR_INVALID
                assert e2.lib.hens_last_error(e2.ctx).decode() == "hens_rj_set_periodic: branch 0 has 2 leaf parameters, a period was given for parameter 2"
                with pytest.raises(ValueError):
                    e2.set_periodic({"ramp": {2: 1.0}})
            e2.upload(x, inds, betas=np.array([1.0, 0.5]))
            e2.eval_state()
            e2.set_mh_scale([np.full(2, 0.01), np.full(4, 0.01)])
            e2.set_schedule("none")
            e2.step(3)
            chains.append(e2.download())
        finally:
            e2.close()
    for k in chains[0][0]:
        assert ps.same_bits(chains[0][0][k], chains[1][0][k]), "no period reached the context"
    assert ps.same_bits(chains[0][2], chains[1][2]) and not ps.same_bits(chains[0][0]["ramp"], x["ramp"])
    from tests import parity_utils as pu
    oo, mu, invcov = pu.make_oracle(2, 16, 8, box=50.0)
    e3 = pu.make_engine(oo, mu, invcov)
    try:
        assert e3.lib.hens_rj_set_periodic(e3.ctx, None) == _lib.ERR_UNSUPPORTED
        assert e3.lib.hens_last_error(e3.ctx).decode() == ("hens_rj_set_periodic needs a leaf-packing context (HENS_LIKE_TEMPLATE); hens_set_periodic "
                                                           "serves the others")
        assert pu.run_parity(oo, e3, 1, teacher_forced=True) == 0
    finally:
        e3.close()
    e4 = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]))
    try:
        assert e4.lib.hens_set_periodic(e4.ctx, None) == _lib.ERR_UNSUPPORTED
        assert e4.lib.hens_last_error(e4.ctx).decode() == "periodic parameters are not defined on leaf-packing records"
    finally:
        e4.close()
