"""The newer leaf-packing moves held to their specifications at the record's limits (-m gpu): k_rj_mt, k_rj_gibbs, the group stretch
move's proposal phase and rebuild kernels, the periodic arms past coordinate 64, the data-point limits of the resident templates, and
a second model on one context.  Cases, starts and coverage conditions are tests/rj_limit_moves.py; every case is sized on its
specification alone in tests/test_rj_limit_moves.py (no GPU), so nothing is exempted and no case is left out here.

Bars: those of tests/test_hip_rj_mt.py, tests/test_hip_rj_gibbs.py, tests/test_hip_rj_group.py and tests/test_hip_rj_periodic.py,
imported with their harnesses - masks, picks, records, log-priors, accept masks and counters exact; lsw / aux_lsw / factors within the
specification's a-priori bound; log-likelihoods through tolerance_log.check_logl (teacher-forced and full evaluations: RTOL_L,
by-difference launches: 1e-12); the ladder 1e-13; no decision on a knife edge."""
import numpy as np
import pytest

from tests import rj_limit_moves as rl
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
RTOL_L = tol.RTOL_L


# ---- A: k_rj_mt ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rl.MT_CASES))
def test_mt_teacher_forced_at_the_limits(name):
    """hens_rj_mt_bd_step on the limit records, every proposal uploaded from the specification (tests/test_hip_rj_mt.py's hook and
    bars): 32-leaf branches (the candidates' mask of a full branch, bit 31), 64 slots in four branches (slot0 = 0, 32, 48, 56), 128
    record doubles at 130 data points, tries written across coordinate 64, K = 64; under prior terms the branch sums over 31 and 32
    slots with the try in slot 0 and in the top slot."""
    from tests.test_hip_rj_mt import _engine, forced_proposal_hook
    c = rl.mt_case(name)
    p = rl.mt_problem(c)
    eng = _engine(c, p)
    worst = [0.0, 0.0, 0.0]
    try:
        cnt, cov = rl.mt_forced_run(c, rl.MT_ROUNDS, forced_proposal_hook(eng, name, worst), p=p)
        rl.mt_assert_covered(cnt, cov, c, name)
        assert eng.counters()["num_bd"] == c["nprop"]
    finally:
        eng.close()
    print(f"{name}: worst |value - exact| / B: lsw {worst[0]:.3f}, aux_lsw {worst[1]:.3f}, factors {worst[2]:.3f}")


@pytest.mark.parametrize("name", sorted(rl.MT_REPLAYS))
def test_mt_production_step_replayed_at_the_limits(name):
    """hens_rj_step with the proposal set on the limit records, through tests/test_hip_rj_mt.py's replay (its draws held to the key
    statement, every bar of its own): here the coin, the candidates' mask (~mask & 0xffffffff on a 32-leaf branch) and the leaf slot
    are the kernel's, on resident templates of up to 64 leaves (130 data points: both chunks of a lane's points)."""
    from tests.test_hip_rj_mt import replay_through_the_specification
    schedule, iters = rl.MT_REPLAYS[name]
    c = rl.mt_case(name)
    cov = rl.MTCoverage(rl.lr.MODELS[c["model"]]["nl_max"])
    replay_through_the_specification(name, c, rl.mt_problem(c), schedule, "gaussian", iters, on_info=cov.add)
    rl.mt_replay_covered(cov, c, name)


# ---- B: k_rj_gibbs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [k for k, c in rl.GIBBS_CASES.items() if c["forced"]])
def test_gibbs_blocks_teacher_forced_at_the_limits(name):
    """hens_rj_gibbs_select + hens_rj_mh_step, block after block from the specification's state and draws (tests/test_hip_rj_gibbs.py's
    bars): 64 blocks of one slot each in four branches (ballot bits 0 .. 63, slot0 = 0, 32, 48, 56), 128 blocks of one coordinate or
    one branch (partial masks on both sides of coordinate 64, block 127), blocks split at slot 16 and at the 32-leaf edge with every
    case of fix_logp_gibbs's two counts."""
    from tests import rj_gibbs_move as rgm
    from tests.test_hip_rj_gibbs import _assert_state, _engine, _knife
    c = rl.GIBBS_CASES[name]
    p = rl.gibbs_problem(name)
    o = rl.gibbs_oracle(p, c["seed"])
    names = [b.name for b in o.branches]
    eng = _engine(o.branches, o.T, o.W, p["t"], p["y"], p["sigma"])
    facts = dict(inf=0, zero=0, empty=0, accepted=0, decisions=0)
    try:
        eng.set_gibbs(rgm.table_of(o.blocks, o.branches))
        for it in range(c["forced"]):
            o.iteration()
            rec = o.trace.pop()
            assert len(rec["gibbs"]) == c["nblocks"]
            for r in rec["gibbs"]:
                k, what = r["block"], f"{name} it{it} block {r['block']}"
                inds = {n: r[f"upd_inds_{n}"] for n in names}
                eng.upload(r["x_before"], inds, r["L_before"], r["P_before"], r["betas"])
                eng.gibbs_select(k)
                keep = eng.mh_step(r["steps"], r["u_acc"])
                assert not (_knife(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]) & np.isfinite(r["logp"])).any(), f"{what}: a decision on a knife edge"
                assert np.array_equal(keep, r["accepted"]), f"{what}: accept mask"
                nomove, total = r["here"] == 0, sum(v.sum(axis=-1) for v in inds.values())
                assert not keep[nomove & (r["total"] != 0)].any(), f"{what}: a walker without a leaf in the block's member slots was accepted"
                assert keep[total == 0].all(), f"{what}: a walker without any leaf is accepted, unchanged"
                rl.gibbs_block_facts(facts, r, inds)
                _assert_state(eng, o.branches, {n: r[f"upd_x_{n}"] for n in names}, inds, r["upd_L"], r["upd_P"], what)
        print(f"{name}: {facts}")
        assert 0 < facts["accepted"] < facts["decisions"] and facts["empty"] > 0 and facts["inf"] > 0 and facts["zero"] > 0
        assert eng.counters()["num_mh"] == c["forced"] * c["nblocks"]
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(rl.GIBBS_CASES))
def test_gibbs_production_step_replayed_at_the_limits(name):
    """hens_rj_step under the table - ONE k_rj_gibbs launch over up to 128 blocks on the resident templates - replayed through the
    specification with the draws hens_rj_gibbs_debug_draws exports, which are held to the key statement block by block (accept uniforms
    exactly; the steps within the normals' bar of scale x the ideal normal where the steps are diagonal): records, masks, log-priors
    and counters bit for bit, log-likelihoods to the by-difference bar, the ladder to 1e-13, no decision within the bar of its uniform."""
    from tests.production_draws import MH_NORMAL_E
    from tests.test_hip_rj_gibbs import RTOL_PROD, _assert_state, _knife, _production_engine, _replay_class
    c = rl.GIBBS_CASES[name]
    p = rl.gibbs_problem(name)
    seed, iters, nb = rl.GIBBS_REPLAY_SEED, c["replay"], c["nblocks"]
    T, W = p["T"], p["W"]
    eng = _production_engine(p, p["setup"], "none", 0, seed, None, p["chol"])
    try:
        x0, inds0, L0, P0, _ = eng.download()
        o = _replay_class()(p["blocks"], p["obr"], x0, inds0, p["t"], p["y"], p["sigma"], None, None, p["betas"], schedule="none", record=True,
                            like_fn=p["like_fn"], skip_empty=False)
        o.live = True
        assert np.array_equal(o.st.P, P0)
        tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        scale = np.concatenate([np.tile(s, b.nleaves_max) for s, b in zip(p["scale"], p["obr"])])
        from tests import rj_gibbs_move as rgm
        table = rgm.table_of(p["blocks"], p["obr"])
        facts = dict(inf=0, zero=0, empty=0, accepted=0, decisions=0)
        mh_acc, done = np.zeros((T, W)), 0
        for n in (1, iters - 1):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                dd = eng.debug_draws(i)
                o.load(dd, offsets, None)
                o.gd = [eng.gibbs_debug_draws(i, k) for k in range(nb)]
                for k in (0, 1, nb // 2, nb - 2, nb - 1):
                    assert np.array_equal(o.gd[k]["u_mh"], rl.gibbs_accept_uniforms(seed, i, T, W, k)), f"{name} iteration {i}: accept uniforms of block {k} against the key statement"
                    if p["chol"] is None:
                        z = rl.gibbs_unit_normals(seed, i, T, W, eng.ncoord, k)
                        err = np.abs(o.gd[k]["step"] - scale * z)[:, :, table[k]]
                        assert np.all(err <= scale[table[k]] * MH_NORMAL_E), f"{name} iteration {i}: steps of block {k} against the key statement ({err.max():.3e})"
                acc, bi, racc = o.iteration()
                rec = o.trace.pop()
                assert len(rec["gibbs"]) == nb
                for r in rec["gibbs"]:
                    edge = _knife(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]) & np.isfinite(r["logp"])
                    assert not edge.any(), f"{name} iteration {i} block {r['block']}: a decision on a knife edge (choose another seed)"
                    mh_acc += r["accepted"]
                    rl.gibbs_block_facts(facts, r, o.st.inds)
            done += n
            what = f"{name}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=RTOL_PROD)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc), f"{what}: accepted is added once per accepted block"
            assert cn["num_mh"] == done * nb == o.num_proposals, f"{what}: num_mh advances by nblocks per iteration"
        print(f"{name}: {facts}")
        assert 0 < facts["accepted"] < facts["decisions"] and facts["empty"] > 0 and facts["inf"] > 0 and facts["zero"] > 0
    finally:
        eng.close()


# ---- E: the data-point limits of the resident templates -----------------------------------------------------------------------------------------
def _replay_gibbs_mt():
    from tests.test_hip_rj_gibbs import _replay_class as gibbs_replay
    from tests.test_hip_rj_mt import _replay_class as mt_replay

    class ReplayGibbsMT(gibbs_replay(), mt_replay()):
        """The replay oracle under a Gibbs table AND a multiple-try proposal: the block draws of tests/test_hip_rj_gibbs.py's replay,
        the tries and pick uniforms of tests/test_hip_rj_mt.py's."""

    return ReplayGibbsMT


@pytest.mark.parametrize("ndata", rl.POINTS_NDATA)
def test_mt_and_gibbs_in_production_at_the_data_point_limits(ndata):
    """hens_rj_step with a multiple-try proposal and one Gibbs block per branch at 257 data points (the second chunk of a lane's
    template points begins: lane 0 alone), 512 (resident templates at capacity) and 513 (none: full evaluation), replayed through the
    composed specification: the bars of the two moves' own replays; at 513 points the log-likelihood bar is the full evaluation's."""
    from tests import rj_gibbs_move as rgm
    from tests.test_hip_rj_gibbs import RTOL_PROD, _assert_state, _knife
    from tests.test_hip_rj_mt import _check_draws, _production_engine
    c = rl.points_case(ndata)
    p = rl.rm.case_problem(c)
    T, W, iters, schedule = c["T"], c["W"], rl.POINTS["iters"], rl.POINTS["schedule"]
    setup = [b.name for b in p["obr"]]
    blocks = rgm.parse_setup(setup, p["obr"])
    rtol = RTOL_PROD if ndata <= rl.RESIDENT_MAX else RTOL_L
    eng = _production_engine(c, p, schedule, "gaussian")
    try:
        eng.set_gibbs(rgm.table_of(blocks, p["obr"]))
        x0, inds0, L0, P0, _ = eng.download()
        o = _replay_gibbs_mt()(blocks, p["obr"], x0, inds0, p["t"], p["y"], p["sigma"], None, None, p["betas"], schedule=schedule, record=True,
                               like_fn=p["like_fn"], skip_empty=False, num_try=c["K"], gens=p["gens"])
        o.live = True
        assert np.array_equal(o.st.P, P0)
        tol.check_logl(L0, o.st.L, RTOL_L, f"{ndata} points: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        mh_acc, bd_acc, done, accepted, decisions = np.zeros((T, W)), np.zeros((T, W)), 0, 0, 0
        for n in (2, iters - 2):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                dd = eng.debug_draws(i)
                o.load(dd, offsets, None)
                o.gd = [eng.gibbs_debug_draws(i, k) for k in range(len(blocks))]
                o.mt = eng.mt_debug_draws(i)
                _check_draws(dd, o.mt, c["seed"], i, c, p, f"{ndata} points: iteration {i}")
                acc, bi, racc = o.iteration()
                rec = o.trace.pop()
                for r in rec["gibbs"]:
                    edge = _knife(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]) & np.isfinite(r["logp"])
                    assert not edge.any(), f"{ndata} points, iteration {i} block {r['block']}: a decision on a knife edge"
                    mh_acc += r["accepted"]
                    accepted, decisions = accepted + int(r["accepted"].sum()), decisions + r["accepted"].size
                bd_acc += racc
            done += n
            what = f"{ndata} points: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=rtol)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc) and np.array_equal(cn["accepted_bd"], bd_acc), f"{what}: accept counters"
            assert cn["num_mh"] == done * len(blocks) and cn["num_bd"] == done
        cnt = rl.rm.Counts()
        for info in o.mt_infos:
            cnt.add(o, info, rl.rm.exact_rj_mt(o, info))
        rl.rm.assert_sized(cnt, dict(c, inf_prior=False, nan_factor=False, edges=False), f"{ndata} points")
        assert 0 < accepted < decisions and o.knife_swaps == 0
    finally:
        eng.close()


# ---- D: periods past coordinate 64 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(rl.PERIODIC_CASES))
def test_periodic_moves_past_coordinate_64(name):
    """hens_rj_step under hens_rj_set_periodic on pulses x 12 + sines x 12 (the sine phases at record coordinates 38 .. 71) with the red /
    blue stretch move (the PER instantiation's second pass), the group move and a Gibbs table of one block per branch plus one per sine
    slot, and on lorentz + chirp for k_rj<STRETCH, 0, WIDE, PER>: replayed through tests/rj_periodic.py's specifications with
    tests/test_hip_rj_periodic.py's bars; accepted seam crossings on both sides of coordinate 64, dead phases past 64 rewritten."""
    from eryn_amd.rj import RJEngine
    from tests import rj_gibbs_move as rgm
    from tests.test_hip_rj_gibbs import _assert_state
    from tests.test_hip_rj_periodic import RTOL_PROD, _assert_bits, _decisions, _knife, _replay_class
    from tests.test_rj_limit_moves import periodic_covered, periodic_oracle
    p = rl.periodic_problem(name)
    move = p["move"]
    eng = RJEngine(p["T"], p["W"], [b.to_device() for b in p["branches"]], p["t"], p["y"], p["sigma"], seed=rl.PERIODIC_SEED, live_dangerously=True)
    try:
        eng.set_periodic(p["periodic"])
        if move == "group":
            eng.set_group(3, 3, p["key"], 2.0)
            eng.set_in_model("group")
        elif move == "stretch":
            eng.set_in_model("stretch")
        else:
            eng.set_mh_scale(p["scale"])
            eng.set_gibbs(rgm.table_of(rgm.parse_setup(p["setup"], p["obr"]), p["obr"]))
        eng.upload(p["x"], p["inds"], betas=p["betas"])
        eng.eval_state()
        eng.set_schedule(p["schedule"])
        assert eng.wide == p["wide"] and eng.ncoord == 72
        x0, inds0, L0, P0, _ = eng.download()
        o = periodic_oracle(dict(p, x=x0, inds=inds0), name, cls_of=lambda cls: _replay_class(move))
        o.live = True
        assert np.array_equal(o.st.P, P0)
        tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        nb = len(o.blocks) if move == "gibbs" else 1
        mh_acc, done = np.zeros((p["T"], p["W"])), 0
        for n in (2, rl.PERIODIC_ITERS - 2):
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
            done += n
            what = f"{name}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=RTOL_PROD)
            _assert_bits(eng, o.st.x, what)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc) and cn["num_mh"] == done * nb, what
        periodic_covered(o, name)
        if move in ("stretch", "group"):
            assert o.facts.short_way >= 1
    finally:
        eng.close()


# ---- C: the group stretch move ---------------------------------------------------------------------------------------------------------------
def _group_engine(p, seed=1, n_iter_update=rl.GROUP_UPDATE, **kw):
    from eryn_amd.rj import RJEngine
    eng = RJEngine(p["T"], p["W"], p["dbr"], p["t"], p["y"], p["sigma"], seed=seed, **kw)
    eng.set_group(rl.GROUP_NFRIENDS, n_iter_update, p["key"], rl.GROUP_A)
    return eng


def _group_forced_chain(eng, o, p, iters, name):
    """tests/test_hip_rj_group.py's teacher-forced chain on the specification's NumPy draws: per iteration the rebuild where the
    specification rebuilds, hens_rj_group_step, the table / keys / windows the move read bit for bit, accept mask, records, log-prior,
    log-likelihood, the cascade, the birth / death move and its cascade.  -> (rebuilds, newborn windows, accepted)."""
    from tests.test_hip_leaf_kinds import _knife_accepts, knife
    from tests.test_hip_rj_gibbs import _assert_state
    from tests.test_hip_rj_group import _assert_table, _forced_rj
    names = [b.name for b in o.branches]
    rebuilds = born = accepted = 0
    for it in range(iters):
        o.iteration()
        rec = o.trace.pop()
        what = f"{name} it{it}"
        assert not (knife(rec["lnpdiff"], rec["u_acc"]) & (rec["logl"] != o.fill)).any() and _knife_accepts(rec) == 0, f"{what}: a decision on a knife edge"
        if rec["rebuilt"]:
            eng.group_rebuild()
        keep = eng.group_step(rec["picks"], rec["u_zz"], rec["u_acc"])
        now = o.keys, o.tab
        o.keys, o.tab = rec["keys"], rec["tab"]
        _assert_table(eng, o, what, start=rec["start"])
        o.keys, o.tab = now
        assert np.array_equal(keep, rec["mh_accepted"]), f"{what}: accept mask"
        _assert_state(eng, o.branches, {k: rec[f"mhupd_x_{k}"] for k in names}, {k: rec[f"mhupd_inds_{k}"] for k in names}, rec["mhupd_L"],
                      rec["mhupd_P"], what + " behind the move")
        sel, _ = eng.pt_sweep(rec["iperm"], rec["i1perm"], rec["u_swap"], adapt=True)
        assert np.array_equal(sel, rec["sel"]), f"{what}: swaps"
        if o.schedule != "none":
            _forced_rj(eng, o, rec, what)
            _assert_state(eng, o.branches, o.st.x, o.st.inds, o.st.L, o.st.P, what + " behind the birth / death move")
        rebuilds += bool(rec["rebuilt"])
        born += 0 if rec["rebuilt"] else sum(int(v.sum()) for v in rec["born"].values())
        accepted += int(keep.sum())
    _assert_table(eng, o, f"{name}: table and windows behind the last iteration")
    assert o.knife_swaps == 0
    return rebuilds, born, accepted


def _group_start(eng, o, p, name):
    eng.upload(p["x"], p["inds"], betas=p["betas"])
    eng.eval_state()
    _, _, L0, P0, _ = eng.download()
    assert np.array_equal(P0, o.st.P)
    tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
    eng.upload(p["x"], p["inds"], o.st.L, o.st.P, p["betas"])


@pytest.mark.parametrize("name", sorted(rl.GROUP_RECORDS))
def test_group_teacher_forced_at_62_63_64_slots(name):
    """hens_rj_group_rebuild / _step / _debug against GroupOracle(check=True) on records of 62, 63 and 64 slots, birth / death and both
    cascades between the moves: tables, keys and windows bit for bit, newborn leaves' windows among them."""
    from tests import rj_group_move as rgr
    from tests.test_hip_leaf_kinds import _counting
    p = rl.group_problem(name)
    o = rl.group_oracle(p, "separate_branches", rl.GROUP_RECORDS[name]["seed"], cls=_counting(rgr.GroupOracle))
    eng = _group_engine(p)
    try:
        assert eng.nslots == sum(rl.GROUP_RECORDS[name]["nl_max"]) and eng.wide
        _group_start(eng, o, p, name)
        rebuilds, born, accepted = _group_forced_chain(eng, o, p, rl.GROUP_FORCED_ITERS, name)
        assert rebuilds == 2 and born > 0 and 0 < accepted < rl.GROUP_FORCED_ITERS * p["T"] * p["W"]
        assert eng.counters()["num_mh"] == rl.GROUP_FORCED_ITERS
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(rl.GROUP_RECORDS))
def test_group_production_draws_at_62_63_64_slots(name):
    """hens_rj_step under the group move on records of 62 | 63 | 64 slots: what hens_rj_group_debug_draws exports is the
    specification's statement of the draws (tests/rj_limit_moves.group_draws) value for value, and the chain replayed through
    GroupOracle with those draws is the device's - so the kernel's zz and accept uniforms, which move from the first call's lanes to a
    second call's between these records, are the stated ones: records, masks, counters and windows bit for bit, log-likelihoods to the
    by-difference bar, the ladder to 1e-13."""
    from tests.test_hip_rj_gibbs import _assert_state
    from tests.test_hip_rj_group import RTOL_PROD, _assert_table, _replay_class
    p = rl.group_problem(name)
    seed, iters = rl.GROUP_REPLAY_SEED, rl.GROUP_REPLAY_ITERS
    adapt = dict(adaptation_lag=5, adaptation_time=5)
    eng = _group_engine(p, seed=seed, **adapt)
    try:
        eng.set_in_model("group")
        eng.upload(p["x"], p["inds"], betas=p["betas"])
        eng.eval_state()
        eng.set_schedule("separate_branches")
        x0, inds0, L0, P0, _ = eng.download()
        o = _replay_class()(rl.GROUP_NFRIENDS, p["key"], rl.GROUP_UPDATE, p["obr"], x0, inds0, p["t"], p["y"], p["sigma"], None, None, p["betas"],
                            schedule="separate_branches", record=True, like_fn=p["like_fn"], group_a=rl.GROUP_A, check=True, **adapt)
        o.live = True
        assert np.array_equal(o.st.P, P0)
        tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        nl = [b.nleaves_max for b in p["obr"]]
        T, W = p["T"], p["W"]
        mh_acc, bd_acc, done, accepted = np.zeros((T, W)), np.zeros((T, W)), 0, 0
        for n in (1, iters - 1):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                dd = eng.debug_draws(i)
                o.load(dd, offsets, None)
                o.gd = eng.group_debug_draws(i)
                picks, u_zz, u_acc = rl.group_draws(seed, i, T, W, nl, [rl.GROUP_NFRIENDS] * len(nl))
                for b, pk in zip(p["obr"], picks):
                    assert np.array_equal(o.gd["picks"][b.name], pk), f"{name} iteration {i}: picks of {b.name} against the key statement"
                assert np.array_equal(o.gd["u_zz"], u_zz) and np.array_equal(o.gd["u_acc"], u_acc), f"{name} iteration {i}: zz / accept uniforms against the key statement"
                acc, bi, racc = o.iteration()
                rec = o.trace.pop()
                assert all(o.nf(b.name) == rl.GROUP_NFRIENDS for b in p["obr"]), "a table shorter than nfriends"
                edge = np.abs(rec["lnpdiff"] - np.log(rec["u_acc"])) <= RTOL_PROD * np.maximum(np.abs(rec["betas_before"][:, None] * rec["logl"]), 1.0)
                assert not (edge & (rec["logl"] != o.fill)).any(), f"{name} iteration {i}: a decision on a knife edge"
                mh_acc += acc
                bd_acc += racc
                accepted += int(acc.sum())
            done += n
            what = f"{name}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=RTOL_PROD)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc) and cn["num_mh"] == done == o.num_proposals, what
            assert np.array_equal(cn["accepted_bd"], bd_acc) and cn["num_bd"] == done
        _assert_table(eng, o, f"{name}: table and windows behind the last iteration")
        assert 0 < accepted < iters * T * W and o.knife_swaps == 0
        # both outcomes on the cold rung as well: an accept uniform stuck at 0 (a lane that no call filled) accepts everything
        assert 0 < mh_acc[0].sum() < iters * W
    finally:
        eng.close()


@pytest.mark.parametrize("name", sorted(rl.TABLE_CASES))
def test_group_table_at_its_limits(name):
    """One rebuild and two moves: W = 300 (the gather's second pass on top of the first's count, tables of thousands of entries sorted
    over many tiles) and one-branch tables of exactly 255 / 256 / 257 entries, with all keys different and with one key across gather
    entry 256 plus -0.0 / +0.0: counts, keys, friends' rows and every window against friend_table / window, bit for bit."""
    from tests import rj_group_move as rgr
    from tests.test_hip_leaf_kinds import _counting
    p = rl.table_problem(name)
    o = rl.group_oracle(p, "none", 1, iters_update=5, cls=_counting(rgr.GroupOracle))
    eng = _group_engine(p, n_iter_update=5)
    try:
        _group_start(eng, o, p, name)
        rebuilds, _, accepted = _group_forced_chain(eng, o, p, 2, name)
        assert rebuilds == 1 and 0 < accepted < 2 * p["T"] * p["W"]
        g = eng.group_debug()
        if "n" in rl.TABLE_CASES[name]:
            assert g["counts"].tolist() == [rl.TABLE_CASES[name]["n"]]
        else:
            assert g["counts"].min() > 16 * 256
    finally:
        eng.close()


# ---- F: a second model on one context ----------------------------------------------------------------------------------------------------
def test_second_model_with_more_data_points_is_a_fresh_contexts_chain():
    """A context given a 40-point model and stepped, then a 600-point model (past the resident templates' 512), an upload and three
    iterations, equals a fresh context given the 600-point model, bit for bit: the data buffers follow the model at hand and the first
    model's resident templates are let go of (full evaluation, as in the fresh context)."""
    from eryn_amd._lib import check, f64, ptr
    from eryn_amd.rj import RJEngine
    from tests import leaf_kind_cases as cases
    c = rl.SECOND_MODEL
    T, W = c["T"], c["W"]
    brs = cases.branches_of(c["kinds"], c["nl_max"])
    dbr = [b.to_device() for b in brs]
    scale = [np.array([0.02 * (hi - lo) for lo, hi in b.box]) for b in brs]
    rs = np.random.RandomState(c["seed"])
    data = []
    for nd in c["ndata"]:
        t = np.linspace(-1, 1, nd)
        data.append((t, cases.make_data(brs, t, 3.0, rs)))
    x, inds = cases.random_state(brs, T, W, rs)
    betas = 0.35 ** np.arange(T)

    def begin(eng):
        eng.upload(x, inds, betas=betas)
        eng.eval_state()
        eng.set_mh_scale(scale)
        eng.set_schedule("separate_branches")
        eng.set_iteration(0)
        eng.set_adapt_time(0)

    def set_model(eng, t, y):
        lo, hi = eng._stand_in_box()
        i32 = lambda v: np.array(v, dtype=np.int32)                                 # noqa: E731
        check(eng.lib.hens_rj_set_model(eng.ctx, len(dbr), ptr(i32([b.kind for b in dbr])), ptr(i32([b.nleaves_max for b in dbr])),
                                        ptr(i32([b.nleaves_min for b in dbr])), ptr(lo), ptr(hi), ptr(f64([b.leaf_logp for b in dbr])),
                                        int(t.shape[0]), ptr(f64(t)), ptr(f64(y)), 3.0), eng.ctx)

    a = RJEngine(T, W, dbr, data[0][0], data[0][1], 3.0, seed=c["seed"])
    b = RJEngine(T, W, dbr, data[1][0], data[1][1], 3.0, seed=c["seed"])
    try:
        begin(a)
        a.step(2)                                                                   # (on the 40-point model's resident templates)
        assert a.counters()["num_mh"] == 2
        set_model(a, *data[1])
        begin(a)
        begin(b)
        a.step(c["iters"])
        b.step(c["iters"])
        xa, ia, La, Pa, ba = a.download()
        xb, ib, Lb, Pb, bb = b.download()
        for k in xa:
            assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"records of {k}"
        assert np.array_equal(La, Lb) and np.array_equal(Pa, Pb) and np.array_equal(ba, bb)
        obr = [q.to_oracle() for q in brs]
        from oracle import eryn_oracle_rj as orj
        from tests import leaf_kinds as lk
        tol.check_logl(La, orj.compute_log_like(xa, ia, Pa, obr, data[1][0], data[1][1], 3.0, like_fn=lk.like_fn(c["kinds"])), RTOL_L,
                       "the second model's log-likelihoods (full evaluations) against the oracle's")
        assert not np.array_equal(xa["pulse"], x["pulse"]), "the chain has moved"
    finally:
        a.close()
        b.close()
