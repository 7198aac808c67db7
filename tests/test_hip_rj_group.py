"""The group stretch move with a stationary friend table on the device (-m gpu): hens_rj_set_group, hens_rj_group_rebuild / _debug /
_step, the k_rj<RJ_MODE_GROUP> launch of hens_rj_step and eryn_amd.rj.GroupStretchLeafMove against the specification
tests/rj_group_move.py and the fixtures captured from the reference (tests/golden/rj_group/).

The teacher-forced tests run each fixture as ONE chain on the device - the windows live on the device between moves, and an upload
restarts them - with the reference's draws: every decision is checked against oracle and fixture on the way, and no accept decision
of a fixture lies on a knife edge (the generator asserts it)."""
import numpy as np
import pytest

from tests import rj_group_move as rg
from tests import tolerance_log as tol
from tests.test_hip_rj_gibbs import _assert_log_prior, _assert_state, _engine

pytestmark = pytest.mark.gpu
RTOL_L = tol.RTOL_L         # teacher-forced: the device's exp / sin / summation order against the oracle's (tests/test_hip_rj.py)
RTOL_PROD = 1e-12           # a full evaluation on the resident-template scheme (uniform-grid recurrences) against the oracle's


def _assert_table(eng, o, what, start=None):
    """The device's table and windows, bit for bit, against the oracle's (``start``: the windows to expect; default the oracle's now)."""
    g = eng.group_debug()
    for bi, b in enumerate(o.branches):
        assert g["counts"][bi] == len(o.keys[b.name]), f"{what}: entries of {b.name}"
        assert np.array_equal(g["keys"][b.name].view(np.uint64), o.keys[b.name].view(np.uint64)), f"{what}: keys of {b.name}"
        assert np.array_equal(g["tab"][b.name].view(np.uint64), o.tab[b.name].view(np.uint64)), f"{what}: friends' rows of {b.name}"
        want = (o.start if start is None else start)[b.name]
        assert np.array_equal(g["start"][b.name], want), f"{what}: windows of {b.name}"
    return g


def _forced_rj(eng, o, rec, what):
    """The oracle's birth / death move of one iteration on the device, with its draws (tests/test_hip_rj.py's way), then its cascade."""
    for sub in rec.get("rj_sub", [rec]):
        if "rj_branches" in sub:
            nb = len(o.branches)
            birth = [np.zeros((o.T, o.W, b.ndim)) for b in o.branches]
            for bi in range(nb):
                birth[bi][sub["rj_change_all"][bi] == +1] = sub["rj_birth_all"][bi]
            keep = eng.bd_all_step(np.stack(sub["rj_change_all"]), np.stack(sub["rj_leaf_all"]), birth, sub["rj_u_acc"])
        else:
            b = o.branches[sub["rj_branch"]]
            birth = np.zeros((o.T, o.W, b.ndim))
            birth[sub["rj_change"] == +1] = sub["rj_birth"]
            keep = eng.bd_step(sub["rj_branch"], sub["rj_change"], sub["rj_leaf"], birth, sub["rj_u_acc"])
        assert np.array_equal(keep, sub["rj_accepted"]), f"{what}: birth / death accept mask"
    sel, swaps = eng.pt_sweep(rec["rj_iperm"], rec["rj_i1perm"], rec["rj_u_swap"], adapt=False)
    assert np.array_equal(sel, rec["rj_sel"]), f"{what}: swaps behind the birth / death move"


# ---- teacher-forced: hens_rj_group_rebuild / _debug / _step per recorded iteration -------------------------------------------------------
@pytest.mark.parametrize("name", rg.FIXTURES)
def test_teacher_forced_chain_matches_the_specification_and_the_reference(name):
    fx = rg.load_fixture(name)
    o = rg.fixture_oracle(fx)
    names = [b.name for b in o.branches]
    eng = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]))
    try:
        eng.set_group(int(fx["nfriends"]), int(fx["n_iter_update"]), rg.fixture_key(fx), float(fx["a"]))
        eng.upload({k: fx[f"x0_{k}"] for k in names}, {k: fx[f"inds0_{k}"] for k in names}, o.st.L, o.st.P, fx["betas0"])
        born = swapped = 0
        for it in range(int(fx["nsteps"])):
            o.iteration()
            rec = o.trace.pop()
            what, pre = f"{name} it{it}", f"it{it}_"
            assert rec["rebuilt"] == bool(fx[pre + "rebuilt"]) == (it % 3 == 0)
            if rec["rebuilt"]:
                eng.group_rebuild()
            keep = eng.group_step(rec["picks"], rec["u_zz"], rec["u_acc"])
            # the table and the windows the move read: the oracle's in front of the proposal = the reference's
            o_now = o.keys, o.tab
            o.keys, o.tab = rec["keys"], rec["tab"]
            _assert_table(eng, o, what, start=rec["start"])
            o.keys, o.tab = o_now
            for k in names:
                assert np.array_equal(rec["keys"][k], fx[pre + f"keys_{k}"]) and np.array_equal(rec["tab"][k], fx[pre + f"tab_{k}"])
                assert np.array_equal(rec["start"][k], fx[pre + f"start_{k}"]), f"{what}: windows against the reference"
                born += int(rec["born"][k].sum()) if not rec["rebuilt"] else 0
            assert np.array_equal(keep, rec["mh_accepted"]), f"{what}: accept mask against the specification"
            assert np.array_equal(keep, fx[pre + "keep"]), f"{what}: accept mask against the reference"
            x = {k: rec[f"mhupd_x_{k}"] for k in names}
            inds = {k: rec[f"mhupd_inds_{k}"] for k in names}
            _assert_state(eng, o.branches, x, inds, rec["mhupd_L"], rec["mhupd_P"], what + " behind the move")
            sel, swaps = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
            assert np.array_equal(sel, rec["sel"]), f"{what}: swaps"
            swapped += int(sel.sum())
            x1 = eng.download()[0]
            for k in names:
                assert np.array_equal(x1[k], fx[pre + f"mh_x_{k}"]), f"{what}: records against the reference, dead slots included"
            _forced_rj(eng, o, rec, what)
            _assert_state(eng, o.branches, o.st.x, o.st.inds, o.st.L, o.st.P, what + " behind the birth / death move")
            x1, inds1 = eng.download()[:2]
            for k in names:
                assert np.array_equal(x1[k], fx[pre + f"rj_x_{k}"]) and np.array_equal(inds1[k], fx[pre + f"rj_inds_{k}"])
        _assert_table(eng, o, f"{name}: windows behind the last iteration (carried by the swaps, dead leaves' still in place)")
        assert born > 0 and swapped > 0, "a newborn leaf's window was fixed; accepted swaps carried windows between rungs"
        cn = eng.counters()
        assert cn["num_mh"] == int(fx["mh_num_proposals"]) == 8 and np.array_equal(cn["accepted_mh"], fx["mh_accepted_total"])
    finally:
        eng.close()


# ---- the sampler -----------------------------------------------------------------------------------------------------------------------------
def _fixture_sampler(fx, rng="numpy", backend=None, seed=None, rj_moves=None):
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GroupStretchLeafMove, RJEnsembleSampler, TemplateLikelihood
    names = [str(k) for k in fx["branch_names"]]
    kinds = {"gauss": "pulse", "sine": "sine"}
    if "gauss_prior_kind" in fx:
        from tests import rj_prior_terms as rpt
        priors = {k: rpt.fixture_container(fx[f"{k}_prior_kind"], fx[f"{k}_box"][:, 0], fx[f"{k}_box"][:, 1]) for k in names}
    else:
        priors = {k: {i: uniform_dist(*fx[f"{k}_box"][i]) for i in range(3)} for k in names}
    rj = {"none": None, "together": True}.get(str(fx["rj_moves"]), str(fx["rj_moves"])) if rj_moves is None else rj_moves
    move = GroupStretchLeafMove(int(fx["nfriends"]), rg.fixture_key(fx), n_iter_update=int(fx["n_iter_update"]), a=float(fx["a"]))
    return RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, TemplateLikelihood({k: kinds[k] for k in names}, fx["t"], fx["y"], float(fx["sigma"])),
                             priors, tempering_kwargs=dict(ntemps=int(fx["T"])), nbranches=len(names), branch_names=names,
                             nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                             moves=move, rj_moves=rj, rng=rng, backend=backend, seed=seed)


@pytest.mark.parametrize("name", rg.FIXTURES)
def test_numpy_sampler_lands_on_the_reference_chain(name):
    """RJEnsembleSampler(moves=GroupStretchLeafMove(...), rng="numpy") with the reference's seeds lands on the reference's chain: every
    stored step's masks and coordinates exact, log-priors exact (prior terms: within their bound), log-likelihoods to 1e-12, the
    ladder to 1e-13, accepted and num_proposals exact - which pins the order of the move's draws on both streams."""
    from eryn_amd.state import State
    fx = rg.load_fixture(name)
    names = [str(k) for k in fx["branch_names"]]
    n, obr = int(fx["nsteps"]), rg.fixture_branches(fx)
    np.random.seed(int(fx["seed_construct"]))          # R := snapshot of the global stream at construction
    s = _fixture_sampler(fx)
    try:
        assert np.array_equal(s.temperature_control.betas, fx["betas0"])
        np.random.seed(int(fx["seed_run"]))
        start = State({k: fx[f"x0_{k}"] for k in names}, log_like=fx["L0"], log_prior=fx["P0"], inds={k: fx[f"inds0_{k}"] for k in names})
        last = s.run_mcmc(start, n, store=True)
        for it, st in enumerate(s.chain):
            pre = f"it{it}_rj_"
            for k in names:
                m = st.branches[k].inds
                assert np.array_equal(m, fx[pre + f"inds_{k}"]), f"{pre}inds of {k}"
                assert np.array_equal(st.branches[k].coords[m], fx[pre + f"x_{k}"][m]) and np.isnan(st.branches[k].coords[~m]).all(), f"{pre}x of {k}"
            full = {k: np.where(st.branches[k].inds[..., None], st.branches[k].coords, 0.0) for k in names}
            _assert_log_prior(st.log_prior, fx[pre + "P"], obr, full, {k: st.branches[k].inds for k in names}, f"{name}: {pre}")
            tol.check_logl(st.log_like, fx[pre + "L"], 1e-12, f"{name}: {pre}log-like")
        pre = f"it{n - 1}_rj_"
        for k in names:
            assert np.array_equal(last.branches[k].coords, fx[pre + f"x_{k}"]), f"coordinates of {k} (dead slots included)"
        np.testing.assert_allclose(last.betas, fx[pre + "betas"], rtol=1e-13, atol=0)
        assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"]) and s.moves[0].num_proposals == int(fx["mh_num_proposals"])
        assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"]) and np.array_equal(np.array(s.rj_num_proposals), fx["rj_num_proposals"])
    finally:
        s.engine.close()


# ---- production: hens_rj_step, replayed through the specification ------------------------------------------------------------------------------
def _replay_class(mt=False):
    if mt:
        from tests.test_hip_rj_mt import _replay_class as base_replay
    else:
        from tests.test_hip_leaf_kinds import _replay_class as base_replay

    class ReplayGroup(rg.GroupOracle, base_replay()):
        """The replay oracle (draw sources: hens_rj_debug_draws, hens_rj_mt_debug_draws) with the group stretch move as its in-model
        move, picks and uniforms read from what hens_rj_group_debug_draws exports."""

        def _draw_picks(self, bi, b, nf, going):
            p = self.gd["picks"][b.name][going]
            assert np.all((p >= 0) & (p < nf))
            return p

        def _draw_zz_group(self):
            return self.gd["u_zz"]

        def _draw_accept(self, which):
            return self.gd["u_acc"] if which == "mh" else super()._draw_accept(which)

    return ReplayGroup


def _grp1_problem():
    fx = rg.load_fixture("grp1")
    obr = rg.fixture_branches(fx)
    x, inds = {b.name: fx[f"x0_{b.name}"] for b in obr}, {b.name: fx[f"inds0_{b.name}"] for b in obr}
    return dict(fx=fx, obr=obr, t=fx["t"], y=fx["y"], sigma=float(fx["sigma"]), x=x, inds=inds, betas=fx["betas0"], T=int(fx["T"]), W=int(fx["W"]),
                key=rg.fixture_key(fx))


def _production_engine(p, schedule, nfriends=3, n_iter_update=3, seed=1, mt=0, group=True, select=True, **kw):
    eng = _engine(p["obr"], p["T"], p["W"], p["t"], p["y"], p["sigma"], seed=seed, **kw)
    if mt:
        eng.set_mt_proposal(mt, None)
    if group:
        eng.set_group(nfriends, n_iter_update, p["key"], 2.0)
        if select:
            eng.set_in_model("group")
    eng.upload(p["x"], p["inds"], betas=p["betas"])
    eng.eval_state()
    eng.set_schedule(schedule)
    return eng


@pytest.mark.parametrize("schedule,mt", [("separate_branches", 0), ("iterate_branches", 0), ("together", 0), ("none", 0), ("separate_branches", 3)])
def test_production_step_replayed_through_the_specification(schedule, mt):
    """hens_rj_step for 8 iterations with n_iter_update = 3 on grp1's start - rebuilds at moves 0, 3, 6, ONE k_rj<RJ_MODE_GROUP> launch
    per iteration on the resident templates, the folded ladder adaptation included - against the specification fed with the draws
    hens_rj_group_debug_draws, hens_rj_debug_draws and hens_rj_mt_debug_draws export: masks, records, the windows behind the last
    iteration and the counters bit for bit, log-likelihoods to 1e-12; num_mh == 8.  (nfriends = 3 is below every table's length here, so
    a pick does not depend on which rebuild the export sees: asserted.)"""
    p = _grp1_problem()
    adapt = dict(adaptation_lag=5, adaptation_time=5)
    eng = _production_engine(p, schedule, mt=mt, seed=7, **adapt)
    try:
        x0, inds0, L0, P0, _ = eng.download()
        kw = dict(num_try=mt, gens=None) if mt else {}
        o = _replay_class(bool(mt))(3, p["key"], 3, p["obr"], x0, inds0, p["t"], p["y"], p["sigma"], None, None, p["betas"], schedule=schedule,
                                    record=True, **adapt, **kw)
        o.live = True
        assert np.array_equal(o.st.P, P0)
        tol.check_logl(L0, o.st.L, RTOL_L, "initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        mh_acc, bd_acc, done, accepted, rebuilds, born = np.zeros((p["T"], p["W"])), np.zeros((p["T"], p["W"])), 0, 0, 0, 0
        for n in (2, 6):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                dd = eng.debug_draws(i)
                assert not dd["step"].any() and not dd["u_mh"].any(), "the Gaussian move's draws are not the group move's"
                o.load(dd, offsets, None)
                o.gd = eng.group_debug_draws(i)
                if mt:
                    o.mt = eng.mt_debug_draws(i)
                acc, bi, racc = o.iteration()
                rec = o.trace.pop()
                assert all(o.nf(b.name) == 3 for b in p["obr"]), "a table shorter than nfriends: the exported picks would depend on the rebuild"
                edge = np.abs(rec["lnpdiff"] - np.log(rec["u_acc"])) <= RTOL_PROD * np.maximum(np.abs(rec["betas_before"][:, None] * rec["logl"]), 1.0)
                assert not (edge & (rec["logl"] != o.fill)).any(), f"iteration {i}: a decision on a knife edge (choose another seed)"
                rebuilds += bool(rec["rebuilt"])
                born += 0 if rec["rebuilt"] else sum(int(v.sum()) for v in rec["born"].values())
                mh_acc += acc
                accepted += int(acc.sum())
                if racc is not None:
                    bd_acc += racc
            done += n
            what = f"{schedule} mt={mt}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=RTOL_PROD)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc) and cn["num_mh"] == done == o.num_proposals, what
            if schedule != "none":
                assert np.array_equal(cn["accepted_bd"], bd_acc) and cn["num_bd"] == done
        _assert_table(eng, o, f"{schedule} mt={mt}: table and windows behind the last iteration")
        assert rebuilds == 3 and eng.counters()["num_mh"] == 8 and 0 < accepted < 8 * p["T"] * p["W"]
        assert born > 0 or schedule == "none"
        assert not np.array_equal(o.st.betas, p["betas"]), "the ladder must have moved"
    finally:
        eng.close()


# ---- a WIDE model, against the specification alone ------------------------------------------------------------------------------------------
def test_teacher_forced_wide_model_short_tables_duplicates_and_signed_zero():
    """Bursts (4 parameters) + offsets (1 parameter): the WIDE instantiation, teacher-forced for four moves with rebuilds at 0 and 2,
    nfriends = 7 above the cold rung's leaf count of either branch, two cold leaves with the same key, a key of -0.0, and a branch
    whose cold rung is empty at the first rebuild."""
    from tests import leaf_kind_cases as cases
    from tests import leaf_kinds as lk
    from eryn_amd.rj import RJEngine
    kinds, T, W = ("burst", "offset"), 2, 5
    brs = cases.branches_of(kinds, (2, 3))
    rs = np.random.RandomState(5)
    t = np.linspace(-1, 1, 70)
    y = cases.make_data(brs, t, 3.0, rs)
    x, inds = cases.random_state(brs, T, W, rs)
    inds["burst"][0] = False
    inds["burst"][0, :3, 0] = True                           # three cold bursts: fewer than nfriends
    x["burst"][0, 1, 0, 1] = x["burst"][0, 0, 0, 1]          # ... two of them with the same key (t0)
    inds["offset"][0] = False                                # no cold offset at the first rebuild
    inds["offset"][1, :, 0] = True
    x["offset"][1, 0, 0, 0] = -0.0
    inds["burst"][1, 4] = False
    inds["offset"][1, 4] = False                             # a walker without any leaf
    obr = [b.to_oracle() for b in brs]
    betas = np.array([1.0, 0.3])
    eng = RJEngine(T, W, [b.to_device() for b in brs], t, y, 3.0)
    try:
        assert eng.wide
        key = {"burst": 1, "offset": 0}
        eng.set_group(7, 2, key, 1.7)
        eng.upload(x, inds, betas=betas)
        eng.eval_state()
        x0, inds0, L0, P0, _ = eng.download()
        o = rg.GroupOracle(7, key, 2, obr, x0, inds0, t, y, 3.0, np.random.RandomState(1), np.random.RandomState(2), betas, record=True,
                           schedule="none", like_fn=lk.like_fn(kinds), group_a=1.7)
        o.st.L, o.st.P = L0.copy(), P0.copy()
        eng.upload(x0, inds0, L0, P0, betas)
        accepted = moved = 0
        for it in range(4):
            o.iteration()
            rec = o.trace.pop()
            what = f"wide it{it}"
            if rec["rebuilt"]:
                eng.group_rebuild()
            keep = eng.group_step(rec["picks"], rec["u_zz"], rec["u_acc"])
            now = o.keys, o.tab
            o.keys, o.tab = rec["keys"], rec["tab"]
            g = _assert_table(eng, o, what, start=rec["start"])
            o.keys, o.tab = now
            if it == 0:
                assert g["counts"][0] == 3 and g["counts"][1] == 0 and np.sum(np.diff(g["keys"]["burst"]) == 0) == 1
            edge = np.abs(rec["lnpdiff"] - np.log(rec["u_acc"])) <= 1e-9 * np.maximum(np.abs(rec["betas_before"][:, None] * rec["logl"]), 1.0)
            assert not (edge & (rec["logl"] != o.fill)).any(), f"{what}: a decision on a knife edge"
            assert np.array_equal(keep, rec["mh_accepted"]), f"{what}: accept mask"
            names = [b.name for b in obr]
            _assert_state(eng, obr, {k: rec[f"mhupd_x_{k}"] for k in names}, {k: rec[f"mhupd_inds_{k}"] for k in names}, rec["mhupd_L"],
                          rec["mhupd_P"], what)
            sel, _ = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
            assert np.array_equal(sel, rec["sel"])
            accepted += int(keep.sum())
            moved += int(sum((rec["q"][k] != rec[f"pre_x_{k}"]).any(axis=-1).sum() for k in names))
        zero = o.keys["offset"] == 0.0
        assert zero.any() and not np.signbit(o.keys["offset"][zero]).any(), "the -0.0 offset has reached the cold rung and is keyed as +0.0"
        assert np.signbit(o.tab["offset"][zero, 0]).any(), "... while its row keeps its bits"
        assert 0 < accepted < 4 * T * W and moved > 0
        _assert_table(eng, o, "wide: behind the last sweep")
    finally:
        eng.close()


# ---- chain store, upload, refusals ---------------------------------------------------------------------------------------------------------------
def test_device_backend_chain_equals_the_list_of_states():
    """rng="philox": six stored steps kept on the device (RJDeviceBackend, hens_rj_step_chain) are the list-of-States chain bit for bit."""
    from eryn_amd.backend import RJDeviceBackend
    from eryn_amd.state import State
    from tests.test_hip_rj_chain_store import assert_chain_is_the_host_chain
    fx = rg.load_fixture("grp1")
    names = [str(k) for k in fx["branch_names"]]
    start = State({k: fx[f"x0_{k}"] for k in names}, inds={k: fx[f"inds0_{k}"] for k in names}, betas=fx["betas0"])
    s1 = _fixture_sampler(fx, "philox", seed=5)
    s2 = _fixture_sampler(fx, "philox", backend=RJDeviceBackend(), seed=5)
    try:
        s1.run_mcmc(start, 6, thin_by=2)
        s2.run_mcmc(start, 6, thin_by=2)
        assert len(s1.chain) == 6 and s2.chain == []
        assert_chain_is_the_host_chain(s2.backend, s1.chain, int(fx["T"]), "the group stretch move")
        assert np.array_equal(s1.moves[0].accepted, s2.moves[0].accepted) and s1.moves[0].accepted.sum() > 0
        assert s1.moves[0].num_proposals == s2.moves[0].num_proposals == 12
    finally:
        s1.engine.close()
        s2.engine.close()


def test_upload_restarts_the_rebuild_count():
    """Two moves after a rebuild the table is two moves old; an upload restarts the count, so the next move rebuilds first."""
    p = _grp1_problem()
    eng = _production_engine(p, "none", n_iter_update=5, seed=3)
    try:
        eng.step(1)
        first = eng.group_debug()
        eng.step(1)
        second = eng.group_debug()
        assert all(np.array_equal(first["keys"][k], second["keys"][k]) for k in first["keys"]), "no rebuild at move 1 of 5"
        x, inds, L, P, betas = eng.download()
        want = {b.name: rg.friend_table(x[b.name], inds[b.name], p["key"][b.name]) for b in p["obr"]}
        assert any(not np.array_equal(want[k][0], second["keys"][k]) for k in want), "the cold rung has moved since the rebuild"
        eng.upload(x, inds, L, P, betas)
        empty = eng.group_debug()
        assert not empty["counts"].any() and all((v == -1).all() for v in empty["start"].values()), "an upload drops table and windows"
        eng.step(1)
        third = eng.group_debug()
        for k in want:
            assert np.array_equal(third["keys"][k], want[k][0]) and np.array_equal(third["tab"][k], want[k][1]), "rebuilt from the uploaded state"
    finally:
        eng.close()


def test_a_context_without_a_selected_group_steps_as_before():
    """A group that is set but not selected, and one that was set and cleared, leave hens_rj_step's Gaussian chain as it is."""
    p = _grp1_problem()
    scale = [np.array([2e-2, 2e-2, 4e-3]), np.array([2e-2, 5e-2, 5e-2])]
    engs = [_production_engine(p, "separate_branches", seed=9, group=g, select=False) for g in (False, True, True)]
    try:
        engs[2].set_group(0, 0, None)
        for e in engs:
            e.set_mh_scale(scale)
            e.step(5)
        ref = engs[0].download()
        for e in engs[1:]:
            got = e.download()
            for k in ref[0]:
                assert np.array_equal(ref[0][k], got[0][k]) and np.array_equal(ref[1][k], got[1][k])
            assert all(np.array_equal(u, v) for u, v in zip(ref[2:], got[2:]))
        assert engs[0].counters()["accepted_mh"].sum() > 0
    finally:
        for e in engs:
            e.close()


def test_refusals_keep_code_and_text_and_change_nothing():
    import ctypes as C
    from eryn_amd import _lib
    from eryn_amd._lib import ptr
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.rj import LeafBranch, RJEngine, _TemplateLikelihood
    p = _grp1_problem()
    eng = _production_engine(p, "separate_branches", seed=51)
    lib, ctx = eng.lib, eng.ctx
    keys = np.array([1, 1], dtype=np.int32)

    def refused(code, text, call):
        before = eng.download(), eng.iteration(), eng.counters()["num_mh"], eng.group_debug()["counts"].tolist()
        assert call() == code
        assert lib.hens_last_error(ctx).decode() == text
        after = eng.download(), eng.iteration(), eng.counters()["num_mh"], eng.group_debug()["counts"].tolist()
        for u, v in zip(before[0][:2], after[0][:2]):
            assert all(np.array_equal(u[k], v[k]) for k in u)
        assert all(np.array_equal(u, v) for u, v in zip(before[0][2:], after[0][2:])) and before[1:] == after[1:]

    try:
        eng.step(1)                                            # (a table stands: its counts must survive every refusal)
        assert eng.group_debug()["counts"].all()
        refused(_lib.ERR_INVALID, "hens_rj_set_group: nfriends must be in [0, 64] (65)", lambda: lib.hens_rj_set_group(ctx, 65, 3, ptr(keys), 2.0))
        refused(_lib.ERR_INVALID, "hens_rj_set_group: nfriends must be in [0, 64] (-1)", lambda: lib.hens_rj_set_group(ctx, -1, 3, ptr(keys), 2.0))
        refused(_lib.ERR_INVALID, "n_iter_update must be greather than or equal to 2.", lambda: lib.hens_rj_set_group(ctx, 3, 1, ptr(keys), 2.0))
        refused(_lib.ERR_INVALID, "n_iter_update must be greather than or equal to 2.", lambda: lib.hens_rj_set_group(ctx, 3, 0, ptr(keys), 2.0))
        refused(_lib.ERR_INVALID, "hens_rj_set_group: null key_dim", lambda: lib.hens_rj_set_group(ctx, 3, 3, None, 2.0))
        refused(_lib.ERR_INVALID, "hens_rj_set_group: key_dim[1] = 3, a leaf of branch 1 has parameters 0 .. 2",
                lambda: lib.hens_rj_set_group(ctx, 3, 3, ptr(np.array([1, 3], dtype=np.int32)), 2.0))
        refused(_lib.ERR_INVALID, "hens_rj_set_group: the stretch scale a must be finite and > 1", lambda: lib.hens_rj_set_group(ctx, 3, 3, ptr(keys), 1.0))
        refused(_lib.ERR_UNSUPPORTED, "Gibbs blocks are not built for the group stretch move (hens_rj_set_group(ctx, 0, ...) clears the group)",
                lambda: lib.hens_rj_set_gibbs(ctx, 1, ptr(np.ones((1, eng.ncoord), dtype=np.uint8))))
        d = _lib.HensRjDraws()
        buf = np.zeros((p["T"], p["W"], eng.RW))
        d.step, d.u_acc = buf.ctypes.data, np.ascontiguousarray(buf[..., 0]).ctypes.data
        refused(_lib.ERR_UNSUPPORTED, "hens_rj_propose of the in-model move: not while a group is set (hens_rj_set_group(ctx, 0, ...) clears it)",
                lambda: lib.hens_rj_propose(ctx, _lib.RJ_MOVE_MH, C.byref(d), ptr(buf), ptr(buf), ptr(buf)))
        refused(_lib.ERR_INVALID, "in-model move must be HENS_RJ_INMODEL_GAUSSIAN, HENS_RJ_INMODEL_STRETCH or HENS_RJ_INMODEL_GROUP",
                lambda: lib.hens_rj_set_in_model(ctx, 3))
        refused(_lib.ERR_INVALID, "hens_rj_group_step: null draws", lambda: lib.hens_rj_group_step(ctx, None, None, None, None))
        eng.step(1)
        assert eng.counters()["num_mh"] == 2
        eng.set_group(0, 0, None)                              # cleared: the in-model move is the Gaussian one again, and wants its scale
        assert lib.hens_rj_set_in_model(ctx, _lib.RJ_INMODEL_GROUP) == _lib.ERR_STATE
        assert lib.hens_last_error(ctx).decode() == "HENS_RJ_INMODEL_GROUP: no group set (hens_rj_set_group first)"
        for call in (lambda: lib.hens_rj_group_rebuild(ctx), lambda: lib.hens_rj_group_debug(ctx, None, None, None, None)):
            assert call() == _lib.ERR_STATE and lib.hens_last_error(ctx).decode() == "no group set (hens_rj_set_group)"
        assert lib.hens_rj_step(ctx, 1) == _lib.ERR_STATE and "hens_rj_set_mh_scale" in lib.hens_last_error(ctx).decode()
        # a Gibbs table standing
        eng.set_gibbs(np.ones((2, eng.ncoord), dtype=bool))
        assert lib.hens_rj_set_group(ctx, 3, 3, ptr(keys), 2.0) == _lib.ERR_UNSUPPORTED
        assert lib.hens_last_error(ctx).decode() == "Gibbs blocks are not built for the group stretch move (hens_rj_set_gibbs(ctx, 0, NULL) clears the table)"
    finally:
        eng.close()
    # n_iter_update == 1 with live_dangerously
    e1 = _engine(p["obr"], p["T"], p["W"], p["t"], p["y"], p["sigma"], live_dangerously=True)
    try:
        e1.set_group(3, 1, 1)
    finally:
        e1.close()
    # a model without a device likelihood; before a model
    e2 = RJEngine(2, 8, [LeafBranch("a", [(0.0, 1.0)] * 2, 3, 0)], None, None, 1.0)
    try:
        with pytest.raises(NotImplementedError, match="needs a device likelihood"):
            e2.set_group(3, 3, 0)
    finally:
        e2.close()
    # (more than 64 leaf slots cannot reach the setter: a record holds 128 doubles and hens_rj_set_model_kinds refuses such a model)
    e3 = HipEnsemble(2, 8, 8, _TemplateLikelihood(8), -1.0, 1.0, tempered=True)
    try:
        assert e3.lib.hens_rj_set_group(e3.ctx, 3, 3, ptr(keys), 2.0) == _lib.ERR_STATE, "before a model"
    finally:
        e3.close()
