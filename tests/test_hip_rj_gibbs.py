"""Gibbs blocks over branches and leaf slots for the in-model Gaussian move on the device (-m gpu): hens_rj_set_gibbs,
hens_rj_gibbs_select + hens_rj_mh_step, the k_rj_gibbs launch of hens_rj_step and eryn_amd.rj.GibbsGaussianLeafMove against the
specification tests/rj_gibbs_move.py and the fixtures captured from the reference (tests/golden/rj_gibbs/)."""
import ctypes as C

import numpy as np
import pytest

from tests import rj_gibbs_move as rg
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
RTOL_L = tol.RTOL_L         # teacher-forced: the device's exp / sin / summation order against the oracle's (tests/test_hip_rj.py)
RTOL_PROD = 1e-12           # include/hipensemble.h: log-likelihoods updated leaf by leaf against a full evaluation


def _device_branches(obr):
    from eryn_amd.rj import TemplateBranch
    if hasattr(obr[0], "container"):
        from tests import rj_prior_terms as rpt
        return rpt.device_branches(obr)
    return [TemplateBranch(b.name, b.kind, list(zip(b.lo, b.hi)), b.nleaves_max, b.nleaves_min) for b in obr]


def _engine(obr, T, W, t, y, sigma, **kw):
    from eryn_amd.rj import RJEngine
    return RJEngine(T, W, _device_branches(obr), t, y, sigma, **kw)


def _knife(lnpdiff, u, beta_L):
    """A decision the by-difference bar could flip: |lnpdiff - log u| within the bar times |beta L|.  (A walker that is not evaluated
    carries the fill value -1e300 on both sides, a constant without rounding: its scale is 1.)"""
    scale = np.where(np.abs(beta_L) >= 1e299, 1.0, np.maximum(np.abs(beta_L), 1.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(lnpdiff - np.log(u)) <= RTOL_PROD * scale


def _assert_log_prior(P1, P, obr, x, inds, what):
    """A box model's log-prior is a sum of the branches' constants: exact.  Under prior terms (log-uniform / normal parameters: a log or a
    square per term) the project's bar is the a-priori bound B of a float64 evaluation against exact arithmetic (tests/rj_prior_terms.
    state_bound, tests/test_hip_rj_priors.py): the device's value and the yardstick's are each within B of the exact one, so within
    2 B of each other; -inf and the stored 0.0 of a rejected -inf fall in the same places."""
    if not hasattr(obr[0], "spec"):
        assert np.array_equal(P1, P), f"{what}: log-prior"
        return
    from tests import rj_prior_terms as rpt
    B = rpt.state_bound(obr, x, inds)
    assert np.array_equal(np.isfinite(P1), np.isfinite(P)) and np.array_equal(P1 == 0.0, P == 0.0), f"{what}: log-prior, the places of -inf / 0.0"
    fin = np.isfinite(P)
    assert np.all(np.abs(P1 - P)[fin] <= 2.0 * B[fin]), f"{what}: log-prior misses twice its bound by {np.max((np.abs(P1 - P) - 2 * B)[fin]):.3e}"


def _assert_state(eng, obr, x, inds, L, P, what, rtol=RTOL_L):
    names = [b.name for b in obr]
    x1, inds1, L1, P1, betas1 = eng.download()
    for k in names:
        assert np.array_equal(inds1[k], inds[k]), f"{what}: leaf masks of {k}"
        assert np.array_equal(x1[k], x[k]), f"{what}: coordinates of {k} (frozen coordinates and dead slots included)"
    _assert_log_prior(P1, P, obr, x, inds, what)
    tol.check_logl(L1, L, rtol, what)
    return betas1


# ---- teacher-forced: hens_rj_gibbs_select + hens_rj_mh_step, block after block -----------------------------------------------------------
@pytest.mark.parametrize("name", rg.FIXTURES)
def test_teacher_forced_blocks_match_the_specification_and_the_reference(name):
    """Every block that ran in the reference's chain, from the state in front of it with the reference's draws: accept masks and records
    bit for bit (against the specification and against the fixture), log-prior exact (under prior terms: within its a-priori bound,
    _assert_log_prior), log-likelihood to the teacher-forced bar; the walkers without a moved leaf are named."""
    fx = rg.load_fixture(name)
    o = rg.fixture_oracle(name, fx)
    names = [b.name for b in o.branches]
    eng = _engine(o.branches, o.T, o.W, fx["t"], fx["y"], float(fx["sigma"]))
    try:
        eng.set_gibbs(rg.table_of(o.blocks, o.branches))
        seen_inf = seen_zero = seen_empty = 0
        for it in range(int(fx["nsteps"])):
            o.iteration()
            rec = o.trace.pop()
            for r in rec["gibbs"]:
                k, what = r["block"], f"{name} it{it} block {r['block']}"
                inds = {n: r[f"upd_inds_{n}"] for n in names}
                eng.upload(r["x_before"], inds, r["L_before"], r["P_before"], r["betas"])
                eng.gibbs_select(k)
                keep = eng.mh_step(r["steps"], r["u_acc"])
                assert not _knife(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]).any(), f"{what}: a decision on a knife edge"
                assert np.array_equal(keep, r["accepted"]), f"{what}: accept mask against the specification"
                assert np.array_equal(keep, fx[f"it{it}_b{k}_keep"]), f"{what}: accept mask against the reference"
                nomove, total = r["here"] == 0, sum(v.sum(axis=-1) for v in inds.values())
                assert not keep[nomove & (r["total"] != 0)].any(), f"{what}: a walker without a leaf in the block's member slots was accepted"
                assert keep[total == 0].all(), f"{what}: a walker without any leaf (logp 0.0 on both sides, fill likelihood) is accepted, unchanged"
                seen_inf += int((nomove & (r["total"] != 0)).sum())
                seen_zero += int((nomove & (r["total"] == 0) & (total != 0)).sum())
                seen_empty += int((total == 0).sum())
                _assert_state(eng, o.branches, {n: r[f"upd_x_{n}"] for n in names}, inds, r["upd_L"], r["upd_P"], what)
                x1 = eng.download()[0]
                for n in names:
                    assert np.array_equal(x1[n], fx[f"it{it}_b{k}_x_{n}"]), f"{what}: records against the reference"
        assert (seen_inf > 0 and seen_empty > 0) or name != "rjg1", "rjg1: the walker without a leaf in block 0's slots, the walker without any leaf"
        assert seen_zero > 0 or name != "rjg2", "rjg2: the walker whose leaves all sit outside the block's member slots"
        assert eng.counters()["num_mh"] == int(fx["mh_num_proposals"])
    finally:
        eng.close()


# ---- production: hens_rj_step under a table, replayed through the specification --------------------------------------------------------------
def _replay_class():
    from tests.test_hip_leaf_kinds import _replay_class as wide_replay

    class ReplayGibbs(rg.GibbsOracle, wide_replay()):
        """tests/test_hip_leaf_kinds.py's replay oracle (draw sources: hens_rj_debug_draws) with the block-by-block in-model move, every
        block's steps and accept uniforms read from what hens_rj_gibbs_debug_draws exports.  No block is skipped (the device's rule)."""

        def _draw_block_steps(self, k, b, n):
            tt, ww, ll = np.where(rg.moved_leaves(self.blocks[k], self.st.inds)[b.name])
            assert len(tt) == n
            idx = self.offsets[b.name] + ll[:, None] * b.ndim + np.arange(b.ndim)
            return self.gd[k]["step"][tt[:, None], ww[:, None], idx]

        def _draw_block_accept(self, k):
            u = self.gd[k]["u_mh"]
            assert np.all((u >= 0) & (u < 1))
            return u

    return ReplayGibbs


def _rjg1_problem():
    fx = rg.load_fixture("rjg1")
    obr = rg.fixture_branches(fx)
    scale = [np.array([2e-2, 2e-2, 4e-3]), np.array([2e-2, 5e-2, 5e-2])]
    for b, s in zip(obr, scale):
        b.cov = np.diag(s ** 2)
    x, inds = {b.name: fx[f"x0_{b.name}"] for b in obr}, {b.name: fx[f"inds0_{b.name}"] for b in obr}
    return dict(obr=obr, t=fx["t"], y=fx["y"], sigma=float(fx["sigma"]), x=x, inds=inds, betas=fx["betas0"], scale=scale, like_fn=None,
                T=int(fx["T"]), W=int(fx["W"]))


def _terms_problem(case):
    from tests import leaf_kinds as lk
    from tests import rj_prior_terms as rpt
    c = rpt.CASES[case]
    obr, t, y, sigma, x, inds, betas = rpt.case_problem(c)
    return dict(obr=obr, t=t, y=y, sigma=sigma, x=x, inds=inds, betas=betas, scale=rpt.scales(obr), like_fn=lk.like_fn(c["kinds"]), T=c["T"], W=c["W"])


def _slot_blocks(obr):
    """One block per leaf slot of every branch."""
    return [(b.name, np.arange(b.nleaves_max)[:, None] == np.full((b.nleaves_max, b.ndim), s)) for b in obr for s in range(b.nleaves_max)]


def _halves(obr):
    """Two blocks over both branches of a wide record: the lower slots of the first with the upper slots of the second (the second's
    last parameter frozen), and the other way round."""
    a, b = obr
    ha, hb = a.nleaves_max // 2, b.nleaves_max // 2
    lo_a, lo_b = np.arange(a.nleaves_max)[:, None] < np.full((a.nleaves_max, a.ndim), ha), np.arange(b.nleaves_max)[:, None] < np.full((b.nleaves_max, b.ndim), hb)
    up_b = ~lo_b
    up_b[:, -1] = False
    return [{a.name: lo_a, b.name: up_b}, {b.name: lo_b, a.name: ~lo_a}]


# name -> (problem, gibbs_sampling_setup, schedule, iterations, first iteration, adapting, full covariances, seed)
REPLAYS = {
    "rjg1_blocks_across_the_refresh": (_rjg1_problem, lambda obr: rg.fixture_setup("rjg1"), "separate_branches", 8, 60, True, False, 11),
    "per_slot_full_covariances_no_rj": (_rjg1_problem, _slot_blocks, "none", 6, 0, False, True, 12),
    "terms_per_branch_iterate": (lambda: _terms_problem("iterate_gaussian"), lambda obr: [b.name for b in obr], "iterate_branches", 6, 0, False, False, 13),
    "record_past_64_together": (lambda: _terms_problem("record_past_64"), _halves, "together", 6, 0, False, False, 14),
}


def _production_engine(p, setup, schedule, it0=0, seed=1, adapt=None, chol=None, table=True):
    eng = _engine(p["obr"], p["T"], p["W"], p["t"], p["y"], p["sigma"], seed=seed, **(adapt or {}))
    eng.upload(p["x"], p["inds"], betas=p["betas"])
    eng.eval_state()
    if chol is not None:
        eng.set_mh_chol(chol)
    else:
        eng.set_mh_scale(p["scale"])
    eng.set_schedule(schedule)
    if table:
        eng.set_gibbs(rg.table_of(rg.parse_setup(setup, p["obr"]), p["obr"]))
    if it0:
        eng.set_iteration(it0)
        eng.set_adapt_time(it0)
    return eng


@pytest.mark.parametrize("name", sorted(REPLAYS))
def test_production_step_replayed_through_the_specification(name):
    """hens_rj_step under a table - ONE k_rj_gibbs launch per iteration on the resident templates, folded ladder adaptation included -
    against the specification fed with the draws hens_rj_debug_draws + hens_rj_gibbs_debug_draws export: records, masks, log-priors and
    accept counters bit for bit, log-likelihoods to the by-difference bar 1e-12, the ladder to 1e-13.  No decision of the replay may sit
    within that bar times |beta L| of its uniform (none is left out).  One case crosses iteration 63 -> 64 (the refresh) with an
    adaptation of a short lag pending into every launch."""
    make, setup_of, schedule, iters, it0, adapting, full_cov, seed = REPLAYS[name]
    p = make()
    setup = setup_of(p["obr"])
    adapt = dict(adaptation_lag=5, adaptation_time=5) if adapting else {}
    chol = None
    if full_cov:
        rs = np.random.RandomState(seed)
        chol = np.stack([np.diag(s) + np.tril(0.4 * s[:, None] * rs.randn(3, 3), -1) for s in p["scale"]])
        for b, Lc in zip(p["obr"], chol):
            b.cov = Lc @ Lc.T
    eng = _production_engine(p, setup, schedule, it0, seed, adapt, chol)
    try:
        x0, inds0, L0, P0, _ = eng.download()
        blocks = rg.parse_setup(setup, p["obr"])
        o = _replay_class()(blocks, p["obr"], x0, inds0, p["t"], p["y"], p["sigma"], None, None, p["betas"], schedule=schedule, record=True,
                            like_fn=p["like_fn"], skip_empty=False, **adapt)
        o.live, o.time = True, it0
        assert np.isfinite(P0).all()
        _assert_log_prior(P0, o.st.P, p["obr"], x0, inds0, f"{name}: initial state")
        tol.check_logl(L0, o.st.L, RTOL_L, f"{name}: initial log-like")
        offsets = {b.name: eng.off[i] for i, b in enumerate(p["obr"])}
        T, W, nb = p["T"], p["W"], len(blocks)
        mh_acc, bd_acc, done, decisions, accepted = np.zeros((T, W)), np.zeros((T, W)), 0, 0, 0
        for n in (2, iters - 2):
            it = eng.iteration()
            eng.step(n)
            eng.synchronize()
            for i in range(it, it + n):
                dd = eng.debug_draws(i)
                o.load(dd, offsets, None)
                o.gd = [eng.gibbs_debug_draws(i, k) for k in range(nb)]
                assert np.array_equal(o.gd[0]["u_mh"], dd["u_mh"]) and np.array_equal(o.gd[0]["step"], dd["step"]), "block 0's words are the words without a table"
                assert nb < 2 or not np.array_equal(o.gd[1]["u_mh"], dd["u_mh"])
                acc, bi, racc = o.iteration()
                rec = o.trace.pop()
                for r in rec["gibbs"]:
                    edge = _knife(r["lnpdiff"], r["u_acc"], r["betas"][:, None] * r["logl"]) & np.isfinite(r["logp"])
                    assert not edge.any(), f"{name} iteration {i} block {r['block']}: a decision on a knife edge (choose another seed)"
                    mh_acc += r["accepted"]
                    decisions += r["accepted"].size
                    accepted += int(r["accepted"].sum())
                if racc is not None:
                    bd_acc += racc
            done += n
            what = f"{name}: hens_rj_step vs the specification after {done} iterations"
            betas1 = _assert_state(eng, p["obr"], o.st.x, o.st.inds, o.st.L, o.st.P, what, rtol=RTOL_PROD)
            np.testing.assert_allclose(betas1, o.st.betas, rtol=1e-13, atol=0, err_msg=what)
            cn = eng.counters()
            assert np.array_equal(cn["accepted_mh"], mh_acc), f"{what}: accepted is added once per accepted block"
            assert cn["num_mh"] == done * nb == o.num_proposals, f"{what}: num_mh advances by nblocks per iteration"
            if schedule != "none":
                assert np.array_equal(cn["accepted_bd"], bd_acc) and cn["num_bd"] == done
        assert 0 < accepted < decisions, f"{name}: {accepted} of {decisions} block decisions accepted - both outcomes must occur"
        if adapting:
            assert not np.array_equal(o.st.betas, p["betas"]), "the ladder must have moved"
    finally:
        eng.close()


def _twins_equal(a, b, what, exact_L=True):
    xa, ia, La, Pa, ba = a.download()
    xb, ib, Lb, Pb, bb = b.download()
    for k in xa:
        assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"{what}: records of {k}"
    assert np.array_equal(Pa, Pb) and np.array_equal(ba, bb) and np.array_equal(La, Lb), what


def test_single_all_true_block_is_the_chain_without_a_table():
    """One block with every coordinate true: teacher-forced and over hens_rj_step the chain of a context without a table, bit for bit."""
    p = _rjg1_problem()
    ncoord = sum(b.nleaves_max * b.ndim for b in p["obr"])
    a = _production_engine(p, None, "separate_branches", seed=21, table=False)
    b = _production_engine(p, None, "separate_branches", seed=21, table=False)
    try:
        b.set_gibbs(np.ones((1, ncoord), dtype=bool))
        rs = np.random.RandomState(4)
        for _ in range(2):                                   # teacher-forced
            steps = {q.name: 0.01 * rs.randn(*p["x"][q.name].shape) for q in p["obr"]}
            u = rs.rand(p["T"], p["W"])
            b.gibbs_select(0)
            assert np.array_equal(a.mh_step(steps, u), b.mh_step(steps, u))
            _twins_equal(a, b, "teacher-forced")
        for n in (3, 4):
            a.step(n)
            b.step(n)
            _twins_equal(a, b, f"hens_rj_step({n})")
            ca, cb = a.counters(), b.counters()
            assert np.array_equal(ca["accepted_mh"], cb["accepted_mh"]) and np.array_equal(ca["accepted_bd"], cb["accepted_bd"]) and ca["num_mh"] == cb["num_mh"]
        assert ca["accepted_mh"].sum() > 0
    finally:
        a.close()
        b.close()


def test_coordinates_in_no_block_keep_their_bits():
    """20 iterations without reversible jump (schedule 3): the coordinates that no block moves - a -0.0 among them - keep their bits, as
    rows that travel with their walker through the cascades; the others move; the resident log-likelihoods stay within the by-difference bar of a full evaluation (the templates drift on this
    schedule too, and are refreshed)."""
    p = _rjg1_problem()
    x = {k: v.copy() for k, v in p["x"].items()}
    x["sine"][:, :, 0, 2] = -0.0
    p = dict(p, x=x)
    setup = [("gauss", rg.RJG1_GAUSS_MASK), ("sine", np.array([[1, 1, 0], [0, 0, 0]], dtype=bool))]
    eng = _production_engine(p, setup, "none", seed=31)
    try:
        x0 = eng.download()[0]
        eng.step(20)
        xr, indr, Lr = eng.debug_resident()
        x1, inds1, L1, P1, _ = eng.download()
        tol.check_logl(Lr, L1, RTOL_PROD, "resident log-likelihoods behind 20 iterations of by-difference blocks against the full evaluation")
        table = rg.table_of(rg.parse_setup(setup, p["obr"]), p["obr"]).any(axis=0)
        # (the cascades carry whole records from rung to rung: a walker's frozen coordinates travel together, so the rows of frozen
        #  bits - every branch's, side by side - are the same multiset before and after)
        off, moved, rows0, rows1 = 0, 0, [], []
        for b in p["obr"]:
            m = table[off:off + b.nleaves_max * b.ndim].reshape(b.nleaves_max, b.ndim)
            off += b.nleaves_max * b.ndim
            rows0.append(np.ascontiguousarray(x0[b.name][:, :, ~m].reshape(p["T"] * p["W"], -1)).view(np.uint64))
            rows1.append(np.ascontiguousarray(x1[b.name][:, :, ~m].reshape(p["T"] * p["W"], -1)).view(np.uint64))
            moved += int((np.sort(x1[b.name][:, :, m].ravel()) != np.sort(x0[b.name][:, :, m].ravel())).sum())
        rows0, rows1 = np.concatenate(rows0, axis=1), np.concatenate(rows1, axis=1)
        assert rows0.shape[1] > 0 and sorted(map(tuple, rows0)) == sorted(map(tuple, rows1)), "frozen coordinates changed their bits"
        assert np.signbit(x1["sine"][:, :, 0, 2]).all() and moved > 0
        assert eng.counters()["num_mh"] == 40
    finally:
        eng.close()


def test_chain_resumed_in_a_new_context_continues_bit_for_bit():
    p = _rjg1_problem()
    setup = rg.fixture_setup("rjg1")
    a = _production_engine(p, setup, "iterate_branches", it0=60, seed=41)
    snaps = []
    try:
        for n in (3, 4):
            a.step(n)
            snaps.append((a.download(), a.iteration(), a.counters()["adapt_time"]))
    finally:
        a.close()
    (x1, i1, L1, P1, b1), it1, at1 = snaps[0]
    b = _production_engine(dict(p, x=x1, inds=i1, betas=b1), setup, "iterate_branches", seed=41)
    try:
        b.upload(x1, i1, L1, P1, b1)
        b.set_iteration(it1)
        b.set_adapt_time(at1)
        b.step(4)
        xb, ib, Lb, Pb, bb = b.download()
        (xa, ia, La, Pa, ba), ita, _ = snaps[1]
        assert b.iteration() == ita
        for k in xa:
            assert np.array_equal(ia[k], ib[k]) and np.array_equal(xa[k], xb[k]), f"records of {k}"
        assert np.array_equal(La, Lb) and np.array_equal(Pa, Pb) and np.array_equal(ba, bb)
    finally:
        b.close()


# ---- the sampler --------------------------------------------------------------------------------------------------------------------------------
def _fixture_sampler(name, fx, rng="numpy", backend=None, seed=None):
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GibbsGaussianLeafMove, RJEnsembleSampler, TemplateLikelihood
    names = [str(k) for k in fx["branch_names"]]
    kinds = {"gauss": "pulse", "sine": "sine"}
    if "gauss_prior_kind" in fx:
        from tests import rj_prior_terms as rpt
        priors = {k: rpt.fixture_container(fx[f"{k}_prior_kind"], fx[f"{k}_box"][:, 0], fx[f"{k}_box"][:, 1]) for k in names}
    else:
        priors = {k: {i: uniform_dist(*fx[f"{k}_box"][i]) for i in range(3)} for k in names}
    cov = {k: np.diag(np.ones(3)) * float(fx["cov_factor"]) for k in names}
    rj = {"none": None, "together": True}.get(str(fx["rj_moves"]), str(fx["rj_moves"]))
    return RJEnsembleSampler(int(fx["W"]), {k: 3 for k in names}, TemplateLikelihood({k: kinds[k] for k in names}, fx["t"], fx["y"], float(fx["sigma"])),
                             priors, tempering_kwargs=dict(ntemps=int(fx["T"])), nbranches=len(names), branch_names=names,
                             nleaves_max=dict(zip(names, map(int, fx["nl_max"]))), nleaves_min=dict(zip(names, map(int, fx["nl_min"]))),
                             moves=GibbsGaussianLeafMove(cov, rg.fixture_setup(name)), rj_moves=rj, rng=rng, backend=backend, seed=seed)


@pytest.mark.parametrize("name", rg.FIXTURES)
def test_numpy_sampler_lands_on_the_reference_chain(name):
    """RJEnsembleSampler(moves=GibbsGaussianLeafMove(...), rng="numpy") with the reference's seeds lands on the reference's chain: every
    stored step's masks, coordinates and log-priors exact, log-likelihoods to 1e-12, the ladder to 1e-13, accepted and num_proposals
    exact - rjg2's with the skipped block."""
    from eryn_amd.state import State
    fx = rg.load_fixture(name)
    names = [str(k) for k in fx["branch_names"]]
    n, obr = int(fx["nsteps"]), rg.fixture_branches(fx)
    last_tag = "mh" if str(fx["rj_moves"]) == "none" else "rj"
    np.random.seed(int(fx["seed_construct"]))          # R := snapshot of the global stream at construction
    s = _fixture_sampler(name, fx)
    try:
        assert np.array_equal(s.temperature_control.betas, fx["betas0"])
        np.random.seed(int(fx["seed_run"]))
        start = State({k: fx[f"x0_{k}"] for k in names}, log_like=fx["L0"], log_prior=fx["P0"], inds={k: fx[f"inds0_{k}"] for k in names})
        last = s.run_mcmc(start, n, store=True)
        for it, st in enumerate(s.chain):
            pre = f"it{it}_{last_tag}_"
            for k in names:
                m = st.branches[k].inds
                assert np.array_equal(m, fx[pre + f"inds_{k}"]), f"{pre}inds of {k}"
                assert np.array_equal(st.branches[k].coords[m], fx[pre + f"x_{k}"][m]) and np.isnan(st.branches[k].coords[~m]).all(), f"{pre}x of {k}"
            full = {k: np.where(st.branches[k].inds[..., None], st.branches[k].coords, 0.0) for k in names}
            _assert_log_prior(st.log_prior, fx[pre + "P"], obr, full, {k: st.branches[k].inds for k in names}, f"{name}: {pre}")
            tol.check_logl(st.log_like, fx[pre + "L"], 1e-12, f"{name}: {pre}log-like")
        pre = f"it{n - 1}_{last_tag}_"
        for k in names:
            assert np.array_equal(last.branches[k].coords, fx[pre + f"x_{k}"]), f"coordinates of {k} (dead slots included)"
        np.testing.assert_allclose(last.betas, fx[pre + "betas"], rtol=1e-13, atol=0)
        assert np.array_equal(s.moves[0].accepted, fx["mh_accepted_total"])
        assert s.moves[0].num_proposals == int(fx["mh_num_proposals"]), "num_proposals += 1 per block that ran"
        if last_tag == "rj":
            assert np.array_equal(np.stack(s.rj_accepted), fx["rj_accepted_total"]) and np.array_equal(np.array(s.rj_num_proposals), fx["rj_num_proposals"])
    finally:
        s.engine.close()


def test_device_backend_chain_equals_the_list_of_states():
    """rng="philox": six stored steps kept on the device (RJDeviceBackend, hens_rj_step_chain under the table) are the list-of-States
    chain bit for bit; the move's counters are the device's."""
    from eryn_amd.backend import RJDeviceBackend
    from eryn_amd.state import State
    fx = rg.load_fixture("rjg1")
    names = [str(k) for k in fx["branch_names"]]
    start = State({k: fx[f"x0_{k}"] for k in names}, inds={k: fx[f"inds0_{k}"] for k in names}, betas=fx["betas0"])
    s1 = _fixture_sampler("rjg1", fx, "philox", seed=5)
    s2 = _fixture_sampler("rjg1", fx, "philox", backend=RJDeviceBackend(), seed=5)
    try:
        s1.run_mcmc(start, 6, thin_by=2)
        s2.run_mcmc(start, 6, thin_by=2)
        from tests.test_hip_rj_chain_store import assert_chain_is_the_host_chain
        assert len(s1.chain) == 6 and s2.chain == []
        assert_chain_is_the_host_chain(s2.backend, s1.chain, int(fx["T"]), "Gibbs blocks of the in-model move")
        assert np.array_equal(s1.moves[0].accepted, s2.moves[0].accepted) and s1.moves[0].accepted.sum() > 0
        assert s1.moves[0].num_proposals == s2.moves[0].num_proposals == 12 * 3
    finally:
        s1.engine.close()
        s2.engine.close()


# ---- refusals: code and text, nothing changed -----------------------------------------------------------------------------------------------
def test_refusals_keep_code_and_text_and_change_nothing():
    from eryn_amd import _lib
    from eryn_amd._lib import ptr
    from eryn_amd.rj import LeafBranch, RJEngine
    p = _rjg1_problem()
    setup = rg.fixture_setup("rjg1")
    eng = _production_engine(p, setup, "separate_branches", seed=51)
    lib, ctx = eng.lib, eng.ctx
    ncoord = eng.ncoord
    good = np.ascontiguousarray(rg.table_of(rg.parse_setup(setup, p["obr"]), p["obr"]), dtype=np.uint8)

    def refused(code, text, call):
        before = eng.download(), eng.iteration(), eng.counters()["num_mh"]
        assert call() == code
        assert lib.hens_last_error(ctx).decode() == text
        after = eng.download(), eng.iteration(), eng.counters()["num_mh"]
        for u, v in zip(before[0][:2], after[0][:2]):
            assert all(np.array_equal(u[k], v[k]) for k in u)
        assert all(np.array_equal(u, v) for u, v in zip(before[0][2:], after[0][2:])) and before[1:] == after[1:]
        assert np.array_equal(eng.gibbs_debug_draws(0, 2)["u_mh"].shape, (p["T"], p["W"])), "the table of three blocks still stands"

    try:
        empty = good.copy()
        empty[1] = 0
        refused(_lib.ERR_INVALID, "hens_rj_set_gibbs: block 1 has no true coordinate", lambda: lib.hens_rj_set_gibbs(ctx, 3, ptr(empty)))
        refused(_lib.ERR_INVALID, "hens_rj_set_gibbs: at most 128 Gibbs blocks (129)", lambda: lib.hens_rj_set_gibbs(ctx, 129, ptr(np.ones((129, ncoord), dtype=np.uint8))))
        refused(_lib.ERR_INVALID, "hens_rj_set_gibbs: null mask", lambda: lib.hens_rj_set_gibbs(ctx, 2, None))
        refused(_lib.ERR_INVALID, "block must be in [0, 3)", lambda: lib.hens_rj_gibbs_select(ctx, 3))
        refused(_lib.ERR_INVALID, "block must be in [0, 3)", lambda: lib.hens_rj_gibbs_debug_draws(ctx, 0, -1, ptr(np.zeros((p["T"], p["W"], ncoord))), ptr(np.zeros((p["T"], p["W"])))))
        refused(_lib.ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records step the Gaussian in-model move (hens_rj_set_gibbs(ctx, 0, NULL) clears the table)",
                lambda: lib.hens_rj_set_in_model(ctx, _lib.RJ_INMODEL_STRETCH))
        d = _lib.HensRjDraws()
        buf = np.zeros((p["T"], p["W"], eng.RW))
        d.step, d.u_acc = buf.ctypes.data, np.ascontiguousarray(buf[..., 0]).ctypes.data
        refused(_lib.ERR_UNSUPPORTED, "Gibbs blocks on leaf-packing records need a device likelihood (hens_rj_set_gibbs(ctx, 0, NULL) clears the table)",
                lambda: lib.hens_rj_propose(ctx, _lib.RJ_MOVE_MH, C.byref(d), ptr(buf), ptr(buf), ptr(buf)))
        # hens_set_gibbs stays closed to leaf-packing contexts, with its own code and text
        for move in (0, 1):
            refused(_lib.ERR_UNSUPPORTED, "Gibbs blocks are not built for leaf-packing records",
                    lambda: lib.hens_set_gibbs(ctx, move, 1, ptr(np.ones((1, eng.RW), dtype=np.uint8))))
        eng.step(1)                                            # (still the table of three blocks)
        assert eng.counters()["num_mh"] == 3
        eng.set_gibbs(None)                                    # cleared: the plain move, the stretch move is open again
        eng.step(1)
        assert eng.counters()["num_mh"] == 4
        assert lib.hens_rj_gibbs_select(ctx, 0) == _lib.ERR_STATE and lib.hens_last_error(ctx).decode() == "no Gibbs table on the in-model move (hens_rj_set_gibbs)"
        eng.set_in_model("stretch")
        assert lib.hens_rj_set_gibbs(ctx, 3, ptr(good)) == _lib.ERR_UNSUPPORTED
        assert lib.hens_last_error(ctx).decode() == "Gibbs blocks on leaf-packing records step the Gaussian in-model move (hens_rj_set_in_model(HENS_RJ_INMODEL_GAUSSIAN))"
    finally:
        eng.close()
    e2 = RJEngine(2, 8, [LeafBranch("a", [(0.0, 1.0)] * 2, 3, 0)], None, None, 1.0)
    try:
        with pytest.raises(NotImplementedError, match="need a device likelihood"):
            e2.set_gibbs(np.ones((1, 6), dtype=bool))
    finally:
        e2.close()
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.rj import _TemplateLikelihood
    e3 = HipEnsemble(2, 8, 8, _TemplateLikelihood(8), -1.0, 1.0, tempered=True)
    try:
        assert e3.lib.hens_rj_set_gibbs(e3.ctx, 1, ptr(np.ones((1, 6), dtype=np.uint8))) == _lib.ERR_STATE, "before a model"
    finally:
        e3.close()
