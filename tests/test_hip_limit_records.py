"""k_rj held to the oracle at the record's limits (-m gpu): 32 leaves per branch (mask bit 31), 64 leaf slots, four branches, 128 record
doubles, leaf slots across coordinate 64 (lane 63 | lane 0 of the second pass), 63 / 64 / 65 coordinates (the in-model accept uniform's
lane).  The models, their arithmetic, the starts by walker class and the coverage counters are tests/limit_records.py; the coverage the
teacher-forced cases rely on is sized without a GPU in tests/test_limit_records.py.

Bars (unchanged): leaf masks, every slot's coordinates (dead ones included), log-prior, accept masks, swap masks and
all counters exact; log-likelihood rtol 1e-12 through tolerance_log.check_logl; ladder rtol 1e-13; knife-edge decisions counted and
asserted 0; against exact arithmetic |L - L*| <= 4 B."""
import numpy as np
import pytest

from tests import exact_leaf_kinds as xk                                           # noqa: F401  (the yardstick behind _within_4B_of_exact)
from tests import leaf_kinds as lk
from tests import limit_records as lr
from tests import tolerance_log as tol
from tests.test_hip_leaf_kinds import BAR, RTOL_BETA, RTOL_L, _knife_accepts, _replay, _within_4B_of_exact
from tests.test_hip_rj import _replay_rj, assert_state, state_of

pytestmark = pytest.mark.gpu


def _report(what, cov, model, wanted):
    print(f"{what}: coverage {cov.line(lr.edges(model))}")
    assert cov.missing(wanted) == [], f"{what}: edges without coverage"


# ---- (a), (b): teacher-forced, every move -----------------------------------------------------------------------------------------------
class _Spy:
    """The host likelihood of a host-callable model, keeping what the device handed it: hens_rj_propose's q_out (unpacked), logp_out
    and moved_out."""

    def __init__(self, like):
        self.like, self.seen = like, None

    def __call__(self, x, inds, logp, names, only=None, **kw):
        if only is not None:                                                       # (None: eval_state, no proposal)
            self.seen = ({k: v.copy() for k, v in x.items()}, {k: v.copy() for k, v in inds.items()}, logp.copy(), only.copy())
        return self.like(x, inds, logp, names, only=only, **kw)


def _assert_proposal(spy, o, q, new_inds, logp, moving, what):
    """q_out in full (every slot's coordinates and the masks), logp_out bit for bit (-inf included), moved_out - of the walkers under
    proposal (``moving`` [T, W]; None: all)."""
    if spy is None:
        return
    xs, inds_s, logp_s, moved = spy.seen
    m = np.ones(logp_s.shape, dtype=bool) if moving is None else moving            # (a mask flattens to the movers in (t, w) order)
    assert np.array_equal(moved.astype(bool), m), f"{what}: moved_out"
    flat = lambda a: np.asarray(a).reshape((-1,) + np.shape(a)[2:])                # noqa: E731
    for b in o.branches:
        assert np.array_equal(xs[b.name][m], flat(q[b.name])), f"{what}: q_out, coordinates of {b.name}"
        assert np.array_equal(inds_s[b.name][m], flat(new_inds[b.name])), f"{what}: q_out, leaf masks of {b.name}"
    assert np.array_equal(logp_s[m], logp.reshape(-1)), f"{what}: logp_out"


@pytest.mark.parametrize("case", lr.TF_CASES, ids=lr.case_id)
def test_every_move_teacher_forced_at_the_limits(case):
    """tests/test_hip_rj.py's test_rj_moves_match_the_oracle fed from the oracle's trace on host draws instead of a fixture:
    hens_rj_mh_step (or hens_rj_stretch_split per half), hens_pt_sweep with adaptation, hens_rj_bd_step per branch or
    hens_rj_bd_all_step, hens_pt_sweep without - the state before every move uploaded from the oracle, so no flip can snowball.  Then the
    in-model proposals whose sole offender is the lowest / the highest coordinate of every edge slot.  A host-callable model takes the
    same moves through hens_rj_propose / hens_rj_accept around tests/leaf_kinds.py's function of the packed leaves, and what propose
    hands out is compared too."""
    from eryn_amd.rj import CallableLikelihood, RJEngine
    model, ndata, schedule, in_model = case
    o, brs, _ = lr.tf_oracle(*case)
    T, W = o.T, o.W
    general = lr.is_general(model)
    dev = [b.to_device() for b in brs]
    eng = RJEngine(T, W, dev, None if general else o.t, None if general else o.y, o.sigma, live_dangerously=in_model == "stretch")
    spy = None
    names = [b.name for b in brs]
    cov, knives = lr.Coverage(brs), 0
    try:
        assert eng.general == general and eng.RW == lr.MODELS[model]["RW"] and eng.ncoord == lr.MODELS[model]["ncoord"]
        if general:
            spy = eng.host_like = _Spy(CallableLikelihood(lk.like_fn(lr.like_kinds(model)), args=[o.t, o.y, o.sigma]))
        eng.upload(o.st.x, o.st.inds, betas=o.st.betas)
        eng.eval_state()
        _, _, L, P, _ = eng.download()
        assert np.array_equal(P, o.st.P)
        worst = tol.check_logl(L, o.st.L, RTOL_L, "initial log-like")
        for label in lr.tf_iterations(o, brs, model):
            o.iteration()
            rec = o.trace.pop()
            cov.add(rec)
            knives += _knife_accepts(rec)
            what = f"{lr.case_id(case)} {label}"
            x, inds, L, P = state_of(rec, "pre_", o)
            eng.upload(x, inds, L, P, rec["betas_before"])
            eng.set_adapt_time(rec["time_before"])
            if in_model == "gaussian":
                steps = {}
                for b in o.branches:                                               # packed draws -> slot layout
                    s = np.zeros(x[b.name].shape)
                    s[inds[b.name]] = rec["mh_steps"][b.name]
                    steps[b.name] = s
                keep = eng.mh_step(steps, rec["mh_u_acc"])
                assert np.array_equal(keep, rec["mh_accepted"]), f"{what}: in-model accept mask"
                _assert_proposal(spy, o, rec["mh_q"], {k: inds[k] for k in names}, rec["mh_logp"], None, what + " in-model")
                assert_state(eng, rec, "mhupd_", o, what=what + " after the in-model move")
            else:
                for split in range(2):
                    keep = eng.stretch_split(split, rec["st_labels"], rec[f"st_rint{split}"], rec[f"st_u_zz{split}"], rec[f"st_u_acc{split}"])
                    assert np.array_equal(keep, rec[f"st_keep{split}"]), f"{what}: accept mask of half {split}"
                    moving = rec["st_labels"] == split
                    S = rec[f"st_S{split}"]
                    tt = np.arange(T)[:, None]
                    _assert_proposal(spy, o, rec[f"st_q{split}"], {k: rec[f"pre_inds_{k}"][tt, S] for k in names}, rec[f"st_logp{split}"],
                                     moving, what + f" half {split}")           # ([T, Ns, ...]: the movers in ascending walker order)
                    assert_state(eng, rec, f"stupd{split}_", o, what=what + f" after half {split}")
            eng.upload(*state_of(rec, "mhupd_", o), rec["betas_before"])           # swaps + adaptation on the oracle's exact log-likes
            eng.set_adapt_time(rec["time_before"])
            sel, swaps = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
            assert np.array_equal(sel, rec["sel"]) and np.array_equal(swaps, rec["swaps"]), f"{what}: swaps"
            betas = assert_state(eng, rec, "mh_", o, exact_L=True, what=what + " after the swaps")
            np.testing.assert_allclose(betas, rec["betas_after"], rtol=RTOL_BETA, atol=0)
            for sub in rec.get("rj_sub", [rec]):                                    # birth / death: one branch, every branch in turn, or all at once
                x, inds, L, P = state_of(sub, "rjpre_", o)
                eng.upload(x, inds, L, P, rec["betas_after"])
                if "rj_branches" in sub:
                    birth = []
                    for bi, b in enumerate(brs):
                        rows = np.zeros((T, W, b.ndim))
                        rows[sub["rj_change_all"][bi] == +1] = sub["rj_birth_all"][bi]
                        birth.append(rows)
                    keep = eng.bd_all_step(np.stack(sub["rj_change_all"]), np.stack(sub["rj_leaf_all"]), birth, sub["rj_u_acc"])
                    where = "on all branches"
                else:
                    bi = sub["rj_branch"]
                    birth = np.zeros((T, W, brs[bi].ndim))
                    birth[sub["rj_change"] == +1] = sub["rj_birth"]                 # births are listed in (t, w) order
                    keep = eng.bd_step(bi, sub["rj_change"], sub["rj_leaf"], birth, sub["rj_u_acc"])
                    where = f"on branch {bi}"
                assert np.array_equal(keep, sub["rj_accepted"]), f"{what}: birth / death accept mask {where}"
                _assert_proposal(spy, o, sub["rj_q"], sub["rj_new_inds"], sub["rj_logp"], None, f"{what} birth / death {where}")
                assert_state(eng, sub, "rjupd_", o, what=f"{what} after birth / death {where}")
            eng.upload(*state_of(sub, "rjupd_", o), rec["betas_after"])
            sel, swaps = eng.pt_sweep(rec["rj_iperm"], rec["rj_i1perm"], rec["rj_u_swap"], adapt=False)
            assert np.array_equal(sel, rec["rj_sel"]) and np.array_equal(swaps, rec["rj_swaps"]), f"{what}: swaps after birth / death"
            betas = assert_state(eng, rec, "rj_", o, exact_L=True, what=what + " after the RJ swaps")
            assert np.array_equal(betas, rec["betas_after"]), "swaps after an RJ move must not adapt the ladder"
    finally:
        eng.close()
    gaussian = in_model == "gaussian"
    print(f"{lr.case_id(case)}: knife-edge accepts {knives}, swaps {o.knife_swaps}; worst log-like distance of this test in the tolerance report")
    _report(lr.case_id(case), cov, model, lr.required(model, sole=gaussian))
    if gaussian:
        for b, s in lr.edges(model):
            assert cov.sole_coord[b][s, 0] >= 1 and cov.sole_coord[b][s, brs[b].ndim - 1] >= 1, "sole offender: lowest, highest coordinate"
    assert knives == 0 and o.knife_swaps == 0 and worst <= RTOL_L


# ---- (c): production stepping replayed with the draws the device consumed ------------------------------------------------------------
def _start(model, ndata, T, W, seed):
    brs, t, y, sigma = lr.problem(model, ndata, seed)
    x, inds, _ = lr.start(model, T, W, seed)
    return dict(kinds=lr.MODELS[model]["kinds"], branches=brs, t=t, y=y, sigma=sigma, x=x, inds=inds)


def _stretch_W(model):
    return {120: 240, 121: 256, 95: 192, 126: 256, 63: 128, 64: 128, 65: 192}[lr.MODELS[model]["ncoord"]]     # W >= 2 ncoord


# (model, data points, schedule, in-model move, T, W, iterations, downloads between the two calls)
PROD_CASES = [(m, 40, "separate_branches", "gaussian", 2, 64, 12, True) for m in lr.DEVICE_MODELS] + [
    ("four_branches_64_slots", 40, "together", "gaussian", 3, 48, 10, True),
    ("four_branches_64_slots", 40, "iterate_branches", "gaussian", 3, 48, 10, True),
    ("pulses_RW128", 130, "separate_branches", "gaussian", 2, 64, 12, False),
    ("pulses_RW128", 130, "together", "gaussian", 3, 48, 10, False),
    ("pulses_RW128", 130, "iterate_branches", "gaussian", 3, 48, 10, False)] + [
    (m, 130 if m == "pulses_RW128" else 40, "separate_branches", "stretch", 2, _stretch_W(m), 8, True) for m in lr.DEVICE_MODELS]
# seeds of the cases whose default seed misses an edge's coverage (the device's draws decide; counted from the oracle's side)
SEED = 11
SEEDS = {}


def _prod_id(c):
    return "-".join(map(str, c[:4]))


def _both_outcomes(model, cov, what):
    if model.startswith("coords_"):                                                # the accept uniform's lane: lane 63, lane 0 of pass 1, lane 1
        print(f"{what}: in-model (rejected, accepted) per rung {cov.inmodel_by_rung.tolist()}")
        assert np.all(cov.inmodel_by_rung > 0), f"{what}: both outcomes of the in-model accept test on every rung"


@pytest.mark.parametrize("case", PROD_CASES, ids=_prod_id)
def test_production_step_replayed_at_the_limits(case):
    """hens_rj_step on device draws, replayed through the oracle by tests/test_hip_leaf_kinds.py's harness (every assertion of its own
    stands) from the class starts of tests/limit_records.py; every pair of edges(model) must see an accepted birth, an accepted death
    and an accepted in-model move.  The stretch move runs at W >= 2 ncoord."""
    model, ndata, schedule, in_model, T, W, iters, downloads = case
    seed = SEEDS.get(case[:4], SEED)
    st = _start(model, ndata, T, W, seed)
    cov = lr.Coverage(st["branches"])
    assert in_model != "stretch" or W >= 2 * lr.MODELS[model]["ncoord"]
    worst_L, worst_b = _replay(model, T, W, lr.MODELS[model]["nl_max"], (0,) * len(st["branches"]), ndata, iters, seed, schedule, in_model,
                               downloads=downloads, start=st, on_record=cov.add)
    what = _prod_id(case)
    print(f"{what}: worst log-like distance {worst_L:.3g} (bar {RTOL_L:g}), ladder {worst_b:.3g}")
    _report(what, cov, model, lr.required(model))
    _both_outcomes(model, cov, what)


def _renamed(rec):
    """A trace record of the pulse / sine harnesses (branches "gauss" and "sine") under the names of tests/limit_records.py."""
    out = {k.replace("_gauss", "_pulse"): v for k, v in rec.items()}
    if "mh_q" in rec:
        out["mh_q"] = {"pulse": rec["mh_q"]["gauss"], "sine": rec["mh_q"]["sine"]}
    return out


def _start_rj(ndata, T, W, seed):
    st = _start("pulses_RW128", ndata, T, W, seed)
    ren = {"pulse": "gauss", "sine": "sine"}
    return st, dict(t=st["t"], y=st["y"], sigma=st["sigma"], x={ren[k]: v for k, v in st["x"].items()},
                    inds={ren[k]: v for k, v in st["inds"].items()}, betas=0.35 ** np.arange(T))


@pytest.mark.parametrize("ndata", [40, 130])
def test_pulses_and_sines_at_the_record_maximum_replayed(ndata):
    """pulses_RW128 through tests/test_hip_rj.py's _replay_rj - the template oracle itself (no like_fn) and, past 64 points, the resident
    log-likelihoods against it: pulse slot 21 across coordinate 64, bit 31, the sine branch in the second pass, no pad."""
    T, W, seed = 2, 64, SEEDS.get(("pulses_RW128", ndata, "rj"), SEED)
    st, srj = _start_rj(ndata, T, W, seed)
    cov = lr.Coverage(st["branches"])
    resident = {} if ndata > 64 else None
    _replay_rj(T, W, (32, 10), (0, 0), ndata, 12, seed, calls=(6, 6), start=srj, on_record=lambda rec: cov.add(_renamed(rec)),
               resident=resident)
    _report(f"pulses_RW128 at {ndata} points", cov, "pulses_RW128", lr.required("pulses_RW128"))


def test_full_leaf_covariances_at_the_record_maximum():
    """The Cholesky step (tests/test_hip_rj_fullcov.py's harness) on pulses_RW128 at 130 points: a leaf's three lanes exchange their
    unit normals across lane 63 | 0 (slot 21) and at bit 31."""
    from tests.test_hip_rj_fullcov import _replay_fullcov
    T, W, seed = 2, 64, SEEDS.get(("pulses_RW128", 130, "fullcov"), SEED)
    st, srj = _start_rj(130, T, W, seed)
    cov = lr.Coverage(st["branches"])
    _replay_fullcov(T, W, (32, 10), (0, 0), 130, "separate_branches", 12, seed, (0, 0), start=srj,
                    on_record=lambda rec: cov.add(_renamed(rec)))
    _report("pulses_RW128, full covariances", cov, "pulses_RW128", lr.required("pulses_RW128"))


# ---- (d): exact arithmetic at the limits ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,ndata", [("four_branches_64_slots", 40), ("burst_across_64", 40), ("pulses_RW128", 40), ("pulses_RW128", 130)])
def test_log_like_within_4B_of_exact_at_the_limits(model, ndata):
    """The paths of tests/test_hip_leaf_kinds.py::test_log_like_within_4B_of_exact (eval_state; one production step read with
    debug_resident) with 97 % of the slots in use, on linspace(-1, 1, 40) (its control_40 grid) and on 130 points."""
    brs, t, y, sigma = lr.problem(model, ndata)
    x, inds = lr.dense_state(model, 2, 16)
    r_eval, r_step = _within_4B_of_exact(dict(model=model, grid=f"{ndata} points", branches=brs, t=t, y=y, sigma=sigma, x=x, inds=inds))
    assert r_eval <= BAR and r_step <= BAR


# ---- (e): one past each limit ------------------------------------------------------------------------------------------------------------------
def test_one_past_each_limit_is_refused():
    """33 leaves in a branch: HENS_ERR_INVALID; 65 slots with a kind beyond pulse / sine, 65 slots on a host-callable model:
    HENS_ERR_UNSUPPORTED; coordinates + masks beyond the context's record: HENS_ERR_INVALID; a record of more than 128 doubles:
    NotImplementedError from RJEngine, HENS_ERR_UNSUPPORTED from hens_create.  Every one returns before anything is launched, and the
    model the context had stays: its state evaluates as before.  (None of these is asserted by
    tests/test_hip_leaf_kinds.py::test_refusals_and_the_sampler_on_device_draws or tests/test_hip_rj_protocol.py.)"""
    from eryn_amd import _lib
    from eryn_amd._lib import f64, ptr
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.rj import RJEngine, TemplateBranch, _TemplateLikelihood
    from oracle import eryn_oracle_rj as orj
    from tests import leaf_kind_cases as cases
    with pytest.raises(NotImplementedError):                                        # 129 coordinates + 2 masks
        RJEngine(2, 8, cases.branches_of(("pulse", "sine"), (32, 11)), np.zeros(8), np.zeros(8), 1.0)
    lk_ = _TemplateLikelihood(130)
    with pytest.raises(NotImplementedError):                                        # hens_create: HENS_ERR_UNSUPPORTED
        HipEnsemble(2, 8, 130, lk_, -1.0, 1.0, tempered=True)
    T, W = 2, 8
    brs = cases.branches_of(("ramp", "offset"), (32, 6))                            # 70 coordinates + 2 masks: a record of 72 doubles
    t = np.linspace(-1, 1, 16)
    y = cases.make_data(brs, t, 1.0, np.random.RandomState(3))
    x, inds = cases.random_state(brs, T, W, np.random.RandomState(4))
    eng = RJEngine(T, W, [b.to_device() for b in brs], t, y, 1.0)
    try:
        assert eng.RW == 72
        eng.upload(x, inds, betas=np.array([1.0, 0.5]))
        eng.eval_state()
        before = eng.download()

        def kinds_model(kinds, nl):
            bb = [TemplateBranch(f"b{i}", k, cases.BOX[k], n) for i, (k, n) in enumerate(zip(kinds, nl))]
            lo, hi = f64(np.concatenate([b.lo for b in bb])), f64(np.concatenate([b.hi for b in bb]))
            return eng.lib.hens_rj_set_model_kinds(eng.ctx, len(bb), ptr(np.array([b.kind for b in bb], dtype=np.int32)),
                                                   ptr(np.array(nl, dtype=np.int32)), ptr(np.zeros(len(bb), dtype=np.int32)), ptr(lo), ptr(hi),
                                                   ptr(f64([b.leaf_logp for b in bb])), 16, ptr(f64(t)), ptr(f64(y)), 1.0)

        def general_model(nds, nl):
            lo = f64(np.concatenate([[q[0] for q in lr.GENERAL_BOX[d]] for d in nds]))
            hi = f64(np.concatenate([[q[1] for q in lr.GENERAL_BOX[d]] for d in nds]))
            return eng.lib.hens_rj_set_model_general(eng.ctx, len(nds), ptr(np.array(nds, dtype=np.int32)), ptr(np.array(nl, dtype=np.int32)),
                                                     ptr(np.zeros(len(nds), dtype=np.int32)), ptr(lo), ptr(hi), ptr(f64(np.zeros(len(nds)))))
        assert kinds_model(("offset", "ramp"), (33, 1)) == _lib.ERR_INVALID              # 33 leaves
        assert general_model((1, 2), (33, 1)) == _lib.ERR_INVALID
        assert kinds_model(("offset", "offset", "offset"), (32, 32, 1)) == _lib.ERR_UNSUPPORTED      # 65 slots (68 doubles would fit)
        assert general_model((1, 1, 1), (32, 32, 1)) == _lib.ERR_UNSUPPORTED
        assert kinds_model(("ramp", "offset"), (32, 7)) == _lib.ERR_INVALID              # 71 coordinates + 2 masks > 72
        assert general_model((2, 1), (32, 7)) == _lib.ERR_INVALID
        assert kinds_model(("ramp", "offset"), (32, 8)) == _lib.ERR_INVALID              # 72 coordinates: no room for a mask
        eng.eval_state()                                                            # the model of before is still the context's
        after = eng.download()
        for k in x:
            assert np.array_equal(after[0][k], before[0][k]) and np.array_equal(after[1][k], before[1][k])
        assert np.array_equal(after[2], before[2]) and np.array_equal(after[3], before[3])
        obr = [b.to_oracle() for b in brs]
        P = orj.compute_log_prior(x, inds, obr)
        assert np.array_equal(after[3], P)
        tol.check_logl(after[2], orj.compute_log_like(x, inds, P, obr, t, y, 1.0, like_fn=lk.like_fn(("ramp", "offset"))), RTOL_L, "after the refusals")
    finally:
        eng.close()
