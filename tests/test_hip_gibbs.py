"""Gibbs parameter blocks on the device (hens_set_gibbs, hens_gibbs_select, the block loop of hens_step; csrc/hens_prior.h: the
GIBBS instantiations of k_stretch_prior) against their specification (tests/gibbs_move.py).

  1. teacher-forced: hens_stretch_split pairs and hens_mh_step with the caller's draws, block after block (hens_gibbs_select), some
     proposals pushed outside the support - masks and positions bit for bit, frozen coordinates the old row's bits, log-prior bit for
     bit under a box and within 1.0 B_P under terms, log-likelihood at the project's bar;
  2. production replay: hens_step steps the cases of tests/gibbs_move.CASES, hens_debug_draws_block exports every block's draws, they
     are held to the specification's words and the specification replays them; counters exact; coverage counted from the
     specification's side; a coordinate in no block keeps its multiset over the ensemble;
  3. equivalences: one all-true block is the context without a table; a run split by hens_set_iteration; DeviceBackend against
     Backend; EnsembleSampler(rng="numpy") with the fixtures' seeds lands on the reference's four chains (tests/golden/gibbs/);
  4. refusals of hens_set_gibbs and hens_gibbs_select with code and text; set / replace / clear in both orders.
"""
import hashlib

import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import gibbs_move as gm
from tests import parity_utils as pu
from tests import prior_terms as pt
from tests import production_draws as pd
from tests import replay_utils as ru
from tests import tolerance_log as tol

pytestmark = pytest.mark.gpu
LD = np.longdouble


def _is_box(prob):
    return bool(np.all(prob.prior["kind"] == pt.UNIFORM))


def _engine(prob, T, W, seed=2024, **kw):
    from eryn_amd.engine import HipEnsemble
    terms = None if _is_box(prob) else prob.prior
    return HipEnsemble(T, W, prob.D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=seed, prior_terms=terms, live_dangerously=True, **kw)


def _start(eng, prob, T, W):
    eng.upload(prob.x0(T, W), betas=orc.make_ladder(prob.D, ntemps=T))
    eng.eval_state()
    x, L, P, betas = eng.download()
    assert np.isfinite(P).all(), "a start outside the prior's support"
    return x, L, P, betas


def _check_P(P, Pspec, prob, x, what):
    """Log-prior: under a box the box's constant, bit for bit; under terms within 1.0 B_P of exact arithmetic at the positions."""
    if _is_box(prob):
        assert np.array_equal(P, Pspec), f"{what}: log-prior differs"
        return
    r = pt.worst_ratio(P.reshape(-1), prob.prior, x.reshape(-1, prob.D))
    print(f"{what}: |P - P*| / B_P <= {r:.3f}")
    assert r <= 1.0, f"{what}: |P - P*| reaches {r:.3f} B_P"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_frozen(x_new, x_old, mask, moved_rows, what):
    """Outside the block every coordinate is the old row's bits (rows: the walkers the move could touch)."""
    assert np.array_equal(_bits(x_new[..., ~mask]), _bits(x_old[..., ~mask])), f"{what}: a frozen coordinate changed its bits"
    assert (x_new[..., mask] != x_old[..., mask]).any() or not moved_rows, f"{what}: nothing moved inside the block"


# ---- 1. teacher-forced ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_teacher_forced_blocks_of_both_moves(name):
    c = gm.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = gm.case_problem(c)
    eng = _engine(prob, T, W)
    x, L, P, betas = _start(eng, prob, T, W)
    if prob.lo[D - 1] <= 0.0 <= prob.hi[D - 1]:              # zeros of the other sign in a coordinate that is frozen in some block
        x[..., D - 1] = np.where(np.arange(W) % 3 == 0, -0.0, x[..., D - 1])
    eng.upload(x, betas=betas)
    eng.eval_state()
    x, L, P, betas = eng.download()
    eng.set_gibbs("stretch", c["stretch"])
    eng.set_gibbs("mh", c["mh"])
    eng.set_mh_proposal("iso", gm.mh_scale(prob), 0.5)
    rs = np.random.RandomState(17)
    outside = accepted = rejected = 0
    tt = np.arange(T)[:, None]
    nprop = nprop_mh = 0
    for rnd in range(2):
        labels = np.tile(np.arange(W), (T, 1)) % 2
        [rs.shuffle(row) for row in labels]
        for b, mask in enumerate(c["stretch"]):
            eng.gibbs_select("stretch", b)
            for sp in (0, 1):
                Ns = (W + 1 - sp) // 2
                rint, u_zz, u_acc = rs.randint(W - Ns, size=(T, Ns)), rs.rand(T, Ns), rs.rand(T, Ns)
                u_zz[:, rnd::5] = 1.0 - 2.0 ** -53          # the longest stretch: every fifth proposal far out
                xs, Ls, Ps = x.copy(), L.copy(), P.copy()
                out = gm.stretch_block_split(xs, Ls, Ps, betas, labels, sp, rint, u_zz, u_acc, 2.0, mask, prob.prior, prob.loglike)
                with np.errstate(divide="ignore"):
                    assert not pu.knife_edge(out["lnpdiff"], np.log(u_acc)).any(), "a decision on the knife edge: pick another seed"
                keep = eng.stretch_split(sp, labels, rint, u_zz, u_acc)
                what = f"{name}, round {rnd}, stretch block {b}, split {sp}"
                assert np.array_equal(keep, out["keep"]), f"{what}: accept mask differs in {int((keep != out['keep']).sum())} walkers"
                xd, Ld, Pd, _ = eng.download()
                assert np.array_equal(_bits(xd), _bits(xs)), f"{what}: positions differ"
                _assert_frozen(xd, x, mask, keep.any(), what)
                _check_P(Pd, Ps, prob, xd, what)
                tol.check_logl(Ld, Ls, tol.RTOL_L, what)
                outside += int(np.isinf(out["logp"]).sum())
                accepted += int(keep.sum())
                rejected += int((~keep).sum())
                x, L, P = xd, Ld, Pd
            nprop += 1
        for b, mask in enumerate(c["mh"]):
            eng.gibbs_select("mh", b)
            step = gm.mh_scale(prob) * rs.randn(T, W, D)
            first = int(np.flatnonzero(mask)[0])
            step[:, rnd::7, first] = 60.0 * prob.half[first]                 # every seventh walker: one coordinate of the block far out
            u = rs.rand(T, W)
            xs, Ls, Ps = x.copy(), L.copy(), P.copy()
            out = gm.mh_block(xs, Ls, Ps, betas, step, u, mask, prob.prior, prob.loglike)
            with np.errstate(divide="ignore"):
                assert not pu.knife_edge(out["lnpdiff"], np.log(u)).any(), "a decision on the knife edge: pick another seed"
            keep = eng.mh_step(step, u)
            what = f"{name}, round {rnd}, Gaussian block {b}"
            assert np.array_equal(keep, out["keep"]), f"{what}: accept mask differs in {int((keep != out['keep']).sum())} walkers"
            xd, Ld, Pd, _ = eng.download()
            assert np.array_equal(_bits(xd), _bits(xs)), f"{what}: positions differ"
            _assert_frozen(xd, x, mask, keep.any(), what)
            _check_P(Pd, Ps, prob, xd, what)
            tol.check_logl(Ld, Ls, tol.RTOL_L, what)
            assert np.isinf(out["logp"][:, rnd::7]).all() and not keep[:, rnd::7].any(), f"{what}: the pushed proposals"
            outside += int(np.isinf(out["logp"]).sum())
            accepted += int(keep.sum())
            x, L, P = xd, Ld, Pd
            nprop_mh += 1
    assert outside > 0 and accepted > 0 and rejected > 0
    assert eng.counters()["num_proposals"] == nprop == 2 * len(c["stretch"]) and eng.mh_counters()["num_proposals"] == nprop_mh == 2 * len(c["mh"])
    assert eng.RW == {5: 8, 32: 32, 128: 128, 64: 64}[D]
    eng.close()


# ---- 2. production replay -------------------------------------------------------------------------------------------------------------------
def _exported_blocks(eng, it, nb, mh):
    return [eng.debug_draws(it, mh=mh, block=b) for b in range(nb)]


@pytest.mark.parametrize("name", sorted(gm.CASES))
def test_production_replay(name):
    c = gm.CASES[name]
    T, W, D, seed = c["T"], c["W"], c["D"], c["seed"]
    prob = gm.case_problem(c)
    eng = _engine(prob, T, W, seed=seed)
    x, L, P, betas = _start(eng, prob, T, W)
    x0 = x.copy()
    scale = gm.mh_scale(prob)
    eng.set_mh_proposal("iso", scale, c["weight"])
    eng.set_gibbs("stretch", c["stretch"])
    eng.set_gibbs("mh", c["mh"])
    st = ru.OracleState(x, L, P, betas)
    books = gm.BlockBooks(T, W, len(c["stretch"]), len(c["mh"]))
    cb = pd.label_cb(T, W)
    kinds = []
    for n in (1, c["iters"] - 1):
        it0 = eng.iteration()
        eng.step(n)
        eng.synchronize()
        for it in range(it0, it0 + n):
            mh = pd.is_mh(seed, it, c["weight"])
            kinds.append(mh)
            what = f"{name}, iteration {it}"
            if mh:
                ds = _exported_blocks(eng, it, len(c["mh"]), True)
                assert all(d["is_mh"] for d in ds), f"{what}: the move choice"
                assert all(("cw" in d) == (b < len(c["stretch"])) for b, d in enumerate(ds)), f"{what}: stretch arrays of a block the stretch table lacks"
                for b, d in enumerate(ds):
                    z, u = gm.mh_block_draws(seed, it, T, W, eng.RW, b)
                    assert np.array_equal(d["mh_u"], u), f"{what}: accept uniforms of block {b}"
                    err = np.abs(d["mh_step"] - scale * z[..., :D]).max()
                    assert err <= scale * pd.MH_NORMAL_E, f"{what}: a step of block {b} is {err / scale:.2e} from the specification's normal (bar {pd.MH_NORMAL_E:.2e})"
                gm.mh_iteration(st, books, c["mh"], [d["mh_step"] for d in ds], [d["mh_u"] for d in ds], prob.prior, prob.loglike)
                ref = ru.draws_to_reference(ds[0], T, W)
            else:
                ds = _exported_blocks(eng, it, len(c["stretch"]), False)
                assert not any(d["is_mh"] for d in ds), f"{what}: the move choice"
                for b, d in enumerate(ds):
                    want = gm.block_plan(seed, it, T, W, cb, b)
                    for k in ("own", "cw", "u_zz", "u_acc"):
                        assert np.array_equal(d[k], want[k]), f"{what}: {k} of block {b} differs from the specification's words"
                    assert np.array_equal(d["own"], ds[0]["own"]), f"{what}: one labelling per iteration"
                refs = [ru.draws_to_reference(d, T, W) for d in ds]
                gm.stretch_iteration(st, books, c["stretch"], refs, 2.0, prob.prior, prob.loglike)
                ref = refs[0]
            gm.pt_tail(st, ref)
        xd, Ld, Pd, bd = eng.download()
        what = f"{name} after iteration {it0 + n - 1}"
        assert np.array_equal(_bits(xd), _bits(st.x)), f"{what}: x differs from the specification in {int((xd != st.x).any(axis=-1).sum())} walkers"
        _check_P(Pd, st.P, prob, xd, what)
        tol.check_logl(Ld, st.L, tol.RTOL_L, what)
        np.testing.assert_allclose(bd, st.betas, rtol=1e-13, atol=0, err_msg=f"{what}: betas")
        cs, cm = eng.counters(), eng.mh_counters()
        assert np.array_equal(cs["accepted"], books.accepted), f"{what}: stretch accept counters"
        assert np.array_equal(cm["accepted"], books.mh_accepted), f"{what}: the Gaussian move's accept counters"
        assert cs["num_proposals"] == books.num_proposals == (len(kinds) - sum(kinds)) * len(c["stretch"]), f"{what}: num_proposals advances per block"
        assert cm["num_proposals"] == books.num_proposals_mh == sum(kinds) * len(c["mh"]), f"{what}: the MH move's num_proposals"
        assert np.array_equal(cs["swaps_total"], st.swaps_total), f"{what}: swap totals"
    assert any(kinds) and not all(kinds)
    gm.assert_coverage(books, name)
    if name in gm.NEVER_MOVES:
        d = gm.NEVER_MOVES[name]
        assert np.array_equal(np.sort(_bits(x0[..., d]).reshape(-1)), np.sort(_bits(xd[..., d]).reshape(-1))), f"{name}: coordinate {d} is in no block"
    # the launch path of a profiled call: per block two copying half-steps or one MH launch, ONE cascade per iteration
    eng.set_profiling(True)
    it0 = eng.iteration()
    eng.step(2)
    tm = eng.timing()
    nm = sum(pd.is_mh(seed, it, c["weight"]) for it in (it0, it0 + 1))
    assert (tm["n_stretch"], tm["n_pt"], tm["n_fused"]) == (2 * len(c["stretch"]) * (2 - nm) + len(c["mh"]) * nm, 2, 0), tm
    # the mask of hens_step_report: a walker's accepted block proposals of the last iteration
    before = eng.counters()["accepted"] + eng.mh_counters()["accepted"]
    acc, _, _ = eng.step_report(1, 1)
    after = eng.counters()["accepted"] + eng.mh_counters()["accepted"]
    assert np.array_equal(acc, after - before) and acc.max() <= max(len(c["stretch"]), len(c["mh"]))
    eng.close()


def test_block_export_with_a_table_on_one_move_only():
    """hens_debug_draws_block where the two tables differ in length, down to no table at all on one move: the other move's arrays
    are the block's only where that move has such a block, and are left out otherwise; block 0 is hens_debug_draws."""
    c = gm.CASES["3x70x5_diag_terms"]
    T, W, D, seed = 2, 24, 5, c["seed"]
    prob = gm.case_problem(c)
    eng = _engine(prob, T, W, seed=seed)
    _start(eng, prob, T, W)
    scale = gm.mh_scale(prob)
    cb = pd.label_cb(T, W)
    for weight, tables in ((1.0, dict(mh=c["mh"])), (0.0, dict(stretch=c["stretch"])), (0.5, dict(stretch=c["stretch"][:2], mh=c["mh"]))):
        eng.set_mh_proposal("iso", scale, weight)
        for move in ("stretch", "mh"):
            eng.set_gibbs(move, tables.get(move))
        nb = {m: len(tables[m]) if m in tables else 1 for m in ("stretch", "mh")}
        for it in range(4):
            mh = pd.is_mh(seed, it, weight)
            for b in range(nb["mh" if mh else "stretch"]):
                d = eng.debug_draws(it, mh=True, block=b)
                assert d["is_mh"] == mh and np.array_equal(d["own"], gm.block_plan(seed, it, T, W, cb, 0)["own"])
                assert ("cw" in d) == ("u_zz" in d) == ("u_acc" in d) == (b < nb["stretch"]) and ("mh_step" in d) == ("mh_u" in d) == (b < nb["mh"])
                if "cw" in d:
                    want = gm.block_plan(seed, it, T, W, cb, b)
                    assert all(np.array_equal(d[k], want[k]) for k in ("cw", "u_zz", "u_acc")), f"iteration {it}, block {b}: the stretch arrays"
                if "mh_u" in d:
                    z, u = gm.mh_block_draws(seed, it, T, W, eng.RW, b)
                    assert np.array_equal(d["mh_u"], u) and np.abs(d["mh_step"] - scale * z[..., :D]).max() <= scale * pd.MH_NORMAL_E
            with pytest.raises(ValueError, match="block must be in"):
                eng.debug_draws(it, mh=True, block=nb["mh" if mh else "stretch"])
        eng.step(2)                                           # (and the context steps on with such tables)
    eng.close()


# ---- 3. equivalences ----------------------------------------------------------------------------------------------------------------------------
def _digest(eng):
    h = hashlib.sha256()
    for a in eng.download():
        h.update(np.ascontiguousarray(a).tobytes())
    h.update(np.ascontiguousarray(eng.counters()["accepted"]).tobytes())
    h.update(np.ascontiguousarray(eng.mh_counters()["accepted"]).tobytes())
    return h.hexdigest()


def _run_case(name, split=None):
    c = gm.CASES[name]
    prob = gm.case_problem(c)
    eng = _engine(prob, c["T"], c["W"], seed=c["seed"])
    _start(eng, prob, c["T"], c["W"])
    eng.set_mh_proposal("iso", gm.mh_scale(prob), c["weight"])
    eng.set_gibbs("stretch", c["stretch"])
    eng.set_gibbs("mh", c["mh"])
    if split is None:
        eng.step(c["iters"])
    else:
        eng.step(split)
        eng.set_iteration(eng.iteration())
        eng.step(c["iters"] - split)
    out = _digest(eng)
    eng.close()
    return out


def test_a_run_split_by_set_iteration_is_the_uninterrupted_one():
    for name in ("3x70x5_diag_terms", "2x131x32_dense_box"):
        assert _run_case(name) == _run_case(name, split=2)


@pytest.mark.parametrize("name", ["3x70x5_diag_terms", "2x131x32_dense_box"])
def test_one_all_true_block_is_the_context_without_a_table(name):
    """The same seed with one all-true block on both moves and without a table: the draws are block 0's - today's words - and the
    factor is (ndim - 1) log zz, so the chain is the same one bit for bit: positions, log-likelihood, log-prior, ladder, counters.
    (Under terms both contexts step on k_stretch_prior's code; under a box the context without a table steps on the in-place
    kernels, and the bits are asked of that path too.)"""
    c = gm.CASES[name]
    T, W, D = c["T"], c["W"], c["D"]
    prob = gm.case_problem(c)
    res, draws = [], []
    for table in (False, True):
        eng = _engine(prob, T, W, seed=c["seed"])
        _start(eng, prob, T, W)
        eng.set_mh_proposal("iso", gm.mh_scale(prob), c["weight"])
        if table:
            eng.set_gibbs("stretch", np.ones((1, D), dtype=bool))
            eng.set_gibbs("mh", np.ones((1, D), dtype=bool))
        eng.step(c["iters"])
        res.append(eng.download() + (eng.counters(), eng.mh_counters()))
        draws.append([eng.debug_draws(it, mh=True) for it in range(c["iters"])])
        eng.close()
    for it, (d0, d1) in enumerate(zip(*draws)):
        assert all(np.array_equal(d0[k], d1[k]) for k in d0), f"{name}: the draws of iteration {it}"
    (x0, L0, P0, b0, c0, m0), (x1, L1, P1, b1, c1, m1) = res
    assert np.array_equal(_bits(x0), _bits(x1)), f"{name}: positions differ in {int((x0 != x1).any(axis=-1).sum())} walkers"
    assert np.array_equal(_bits(L0), _bits(L1)), f"{name}: log-likelihood differs in {int((L0 != L1).sum())} walkers, worst relative {float(np.max(np.abs(L0 - L1) / np.abs(L0))):.2e}"
    assert np.array_equal(_bits(P0), _bits(P1)), f"{name}: log-prior differs in {int((P0 != P1).sum())} walkers"
    assert np.array_equal(_bits(b0), _bits(b1)), f"{name}: the ladders differ"
    _check_P(P1, P0, prob, x1, name)
    assert np.array_equal(c0["accepted"], c1["accepted"]) and np.array_equal(m0["accepted"], m1["accepted"])
    assert c0["num_proposals"] == c1["num_proposals"] and m0["num_proposals"] == m1["num_proposals"]
    assert np.array_equal(c0["swaps_total"], c1["swaps_total"])


def _philox_sampler(c, prob, backend):
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.moves import GaussianMove, StretchMove
    from tests.dist_move import container_of
    setup = lambda masks: [("model_0", m[None, :]) for m in masks]      # noqa: E731
    moves = [(StretchMove(gibbs_sampling_setup=setup(c["stretch"]), live_dangerously=True), 1.0 - c["weight"]),
             (GaussianMove({"model_0": gm.mh_scale(prob) ** 2}, gibbs_sampling_setup=setup(c["mh"])), c["weight"])]
    return EnsembleSampler(c["W"], c["D"], pu.device_likelihood(prob), container_of(prob.prior), rng="philox", seed=c["seed"], moves=moves,
                           backend=backend, tempering_kwargs=dict(ntemps=c["T"], adaptation_lag=50, adaptation_time=5))


@pytest.mark.parametrize("thin", [1, 2])
def test_device_backend_is_the_host_backend(thin):
    from eryn_amd.backend import Backend, DeviceBackend
    from tests.test_hip_chain_store import assert_backends_equal, assert_state_equal, assert_totals_equal
    name = "3x70x5_diag_terms"
    c = gm.CASES[name]
    prob = gm.case_problem(c)
    x0 = prob.x0(c["T"], c["W"])
    a, b = _philox_sampler(c, prob, Backend()), _philox_sampler(c, prob, DeviceBackend())
    ra, rb = a.run_mcmc(x0, 5, thin_by=thin), b.run_mcmc(x0, 5, thin_by=thin)
    what = f"{name}, thin_by={thin}"
    assert_backends_equal(a.backend, b.backend, what)
    assert_totals_equal(a.backend, b.backend, what)
    assert_state_equal(ra, rb, what)
    for ma, mb, masks in zip(a.moves, b.moves, (c["stretch"], c["mh"])):
        assert np.array_equal(ma.accepted, mb.accepted) and ma.num_proposals == mb.num_proposals
        assert ma.num_proposals > 0 and ma.num_proposals % len(masks) == 0 and np.asarray(ma.accepted).sum() > 0
    assert a.moves[0].num_proposals // len(c["stretch"]) + a.moves[1].num_proposals // len(c["mh"]) == 5 * thin
    if thin == 1:                                # the chain is the context's own: the same seed through hens_step
        eng = _engine(prob, c["T"], c["W"], seed=c["seed"], adaptation_lag=50, adaptation_time=5)
        eng.upload(x0, betas=orc.make_ladder(c["D"], ntemps=c["T"]))
        eng.eval_state()
        eng.set_mh_proposal("iso", np.sqrt(gm.mh_scale(prob) ** 2), c["weight"])      # (the move's own sqrt(cov))
        eng.set_gibbs("stretch", c["stretch"])
        eng.set_gibbs("mh", c["mh"])
        eng.step(5)
        xd, Ld, Pd, bd = eng.download()
        assert np.array_equal(xd, ra.branches["model_0"].coords[:, :, 0, :]) and np.array_equal(Ld, ra.log_like) and np.array_equal(bd, ra.betas)
        eng.close()


@pytest.mark.parametrize("name", gm.FIXTURES)
def test_numpy_mode_lands_on_the_reference_chain(name):
    """EnsembleSampler(rng="numpy") with the fixture's seeds: the reference's block loop on its two streams, its books exactly - the
    running OR of the red-blue move, the MH move's last-block return value."""
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves import GaussianMove, StretchMove
    from eryn_amd.state import State
    from tests import rj_prior_terms as rpt
    fx = gm.load_fixture(name)
    prior_spec = gm.fixture_prior(fx)
    T, W, D, n = int(fx["T"]), int(fx["W"]), int(fx["D"]), int(fx["nsteps"])
    setup = lambda masks: [("model_0", m[None, :]) for m in masks]      # noqa: E731
    np.random.seed(int(fx["seed_construct"]))                 # R := snapshot of G at construction
    st = StretchMove(gibbs_sampling_setup=setup(fx["masks_stretch"]), live_dangerously=True) if "masks_stretch" in fx else None
    ga = GaussianMove({"model_0": float(fx["cov"])}, gibbs_sampling_setup=setup(fx["masks_gauss"])) if "masks_gauss" in fx else None
    moves = [(m, 0.5) for m in (st, ga)] if st is not None and ga is not None else (st if st is not None else ga)
    s = EnsembleSampler(W, D, GaussianLikelihood(fx["mu"], fx["invcov"]), rpt.fixture_container(fx["prior_kind"], fx["prior_p0"], fx["prior_p1"]),
                        moves=moves, tempering_kwargs=dict(ntemps=T))
    box = bool(np.all(fx["prior_kind"] == 0))
    ret = {}
    orig_sweep = s.engine.pt_sweep

    def pt_sweep(*a, **k):                                    # the state behind the move, in front of the sweep; the sweep's counts
        ret["x_move"], ret["L_move"], ret["P_move"], _ = s.engine.download()
        sel, swaps = orig_sweep(*a, **k)
        ret["swaps"] = np.array(swaps, copy=True)
        return sel, swaps

    s.engine.pt_sweep = pt_sweep
    for m in s.moves:                                         # what propose() hands the sampler
        def propose(model, state, _m=m, _orig=m.propose):
            out, acc = _orig(model, state)
            ret["accepted"] = np.array(acc, copy=True)
            return out, acc
        m.propose = propose
    np.random.seed(int(fx["seed_run"]))
    for it, state in enumerate(s.sample(fx["x0"], iterations=n, store=False)):
        state = State(state, copy=True)
        what, pre = f"{name}, iteration {it}", f"it{it}_"
        xs = fx[pre + "x"]
        assert np.array_equal(_bits(state.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D)), _bits(xs)), f"{what}: positions"
        assert np.array_equal(ret["accepted"], fx[pre + "accepted"]), f"{what}: the mask propose() returns"
        assert np.array_equal(_bits(ret["x_move"]), _bits(fx[pre + "x_move"])), f"{what}: positions after the move"
        assert np.array_equal(ret["swaps"], fx[pre + "swaps_accepted"]), f"{what}: swap counts"
        if box:                                               # the box's constant: bit for bit
            assert np.array_equal(ret["P_move"], fx[pre + "P_move"]) and np.array_equal(np.asarray(state.log_prior).reshape(T, W), fx[pre + "P"]), f"{what}: log-prior"
        else:
            for Pd, xd, k in ((ret["P_move"], fx[pre + "x_move"], "P_move"), (np.asarray(state.log_prior), xs, "P")):
                r = pt.worst_ratio(np.asarray(Pd).reshape(-1), prior_spec, xd.reshape(-1, D))
                assert r <= 1.0, f"{what}: |{k} - P*| reaches {r:.3f} B_P"
                assert np.array_equal(np.asarray(Pd).reshape(T, W) == 0.0, fx[pre + k] == 0.0)
        tol.check_logl(ret["L_move"], fx[pre + "L_move"], tol.RTOL_L, what)
        tol.check_logl(np.asarray(state.log_like).reshape(T, W), fx[pre + "L"], tol.RTOL_L, what)
        np.testing.assert_allclose(state.betas, fx[pre + "betas"], rtol=1e-13, atol=0, err_msg=what)
    for tag, m in (("stretch", st), ("gauss", ga)):
        if m is not None:
            assert np.array_equal(np.asarray(m.accepted).reshape(T, W), fx["accepted_" + tag]), f"{name}: move.accepted of the {tag} move"
            assert m.num_proposals == int(fx["num_proposals_" + tag]), f"{name}: num_proposals of the {tag} move"


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_set_replace_clear():
    from eryn_amd import _lib
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, HostLikelihood
    from tests import dist_move as dm
    c = gm.CASES["3x70x5_diag_terms"]
    T, W, D = 2, 24, 5
    prob = gm.case_problem(c)
    eng = _engine(prob, T, W)
    x0, L0, P0, betas0 = _start(eng, prob, T, W)
    lib, RW = _lib.load(), eng.RW
    ok = np.zeros((2, RW), dtype=np.uint8)
    ok[0, :2] = ok[1, 2] = 1

    def refused(code, text, *args):
        assert lib.hens_set_gibbs(eng.ctx, *args) == code, text
        assert text in lib.hens_last_error(eng.ctx).decode(), lib.hens_last_error(eng.ctx).decode()

    refused(_lib.ERR_INVALID, "move must be HENS_GIBBS_STRETCH (0) or HENS_GIBBS_MH (1)", 2, 2, _lib.ptr(ok))
    refused(_lib.ERR_INVALID, "hens_set_gibbs: nblocks must be >= 0 (-1)", 0, -1, _lib.ptr(ok))
    refused(_lib.ERR_INVALID, "hens_set_gibbs: at most 128 Gibbs blocks (129)", 0, 129, _lib.ptr(ok))
    refused(_lib.ERR_INVALID, "hens_set_gibbs: null mask", 1, 2, None)
    bad = ok.copy()
    bad[1, 2] = 0
    refused(_lib.ERR_INVALID, "hens_set_gibbs: block 1 has no true coordinate", 0, 2, _lib.ptr(bad))
    bad = ok.copy()
    bad[0, 6] = 1
    refused(_lib.ERR_INVALID, "hens_set_gibbs: block 0 moves coordinate 6, a pad of the row", 0, 2, _lib.ptr(bad))
    with pytest.raises(ValueError, match="masks must have shape"):
        eng.set_gibbs("stretch", np.ones((2, D + 1), dtype=bool))
    # the selector: no table yet; then its range; between the half-steps of a move
    assert lib.hens_gibbs_select(eng.ctx, 0, 0) == _lib.ERR_STATE and "no Gibbs table on this move" in lib.hens_last_error(eng.ctx).decode()
    assert lib.hens_gibbs_select(eng.ctx, 3, 0) == _lib.ERR_INVALID
    # a half-step pending
    labels = np.tile(np.arange(W) % 2, (T, 1))
    rs = np.random.RandomState(3)
    eng.stretch_split(0, labels, rs.randint(W // 2, size=(T, W // 2)), rs.rand(T, W // 2), rs.rand(T, W // 2))
    refused(_lib.ERR_STATE, "a half-step is pending", 0, 2, _lib.ptr(ok))
    refused(_lib.ERR_STATE, "a half-step is pending", 0, 0, None)
    eng.stretch_split(1, labels, rs.randint(W // 2, size=(T, W // 2)), rs.rand(T, W // 2), rs.rand(T, W // 2))
    eng.set_gibbs("stretch", ok[:, :D])
    for blk, code in ((-1, _lib.ERR_INVALID), (2, _lib.ERR_INVALID)):
        assert lib.hens_gibbs_select(eng.ctx, 0, blk) == code and "block must be in [0, 2)" in lib.hens_last_error(eng.ctx).decode()
    eng.gibbs_select("stretch", 1)
    eng.stretch_split(0, labels, rs.randint(W // 2, size=(T, W // 2)), rs.rand(T, W // 2), rs.rand(T, W // 2))
    assert lib.hens_gibbs_select(eng.ctx, 0, 0) == _lib.ERR_STATE and "between the half-steps" in lib.hens_last_error(eng.ctx).decode()
    eng.stretch_split(1, labels, rs.randint(W // 2, size=(T, W // 2)), rs.rand(T, W // 2), rs.rand(T, W // 2))
    # what a table stands in the way of
    with pytest.raises(NotImplementedError, match="periodic parameters are not built under Gibbs blocks"):
        eng.set_periodic(np.full(D, 3.0))
    with pytest.raises(NotImplementedError, match="Gibbs blocks step a two-set stretch move"):
        eng.set_nsplits(3)
    bprob = gm.case_problem(gm.CASES["2x131x32_dense_box"])      # (a box: prior terms are refused by the pipeline in front of a table)
    boxed = _engine(bprob, T, W)
    boxed.set_gibbs("mh", np.ones((1, bprob.D), dtype=bool))
    with pytest.raises(NotImplementedError, match="Gibbs blocks are not built for a rank of the ladder pipeline"):
        boxed.pipe_init(1, 0)
    boxed.close()
    eng.set_gibbs("mh", ok[:, :D])
    with pytest.raises(NotImplementedError, match="not built under Gibbs blocks on the MH slot"):
        eng.set_dist_proposal(dm.box_spec(prob.lo, prob.hi), 0.5)
    eng.set_gibbs("mh", None)
    eng.set_gibbs("stretch", None)

    # set / replace / clear, both orders: the plain chain comes back
    def chain(n=4):
        eng.upload(x0, L0, P0, betas0)
        eng.set_iteration(0)
        eng.set_adapt_time(0)
        eng.step(n)
        h = hashlib.sha256()
        for a in eng.download():
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    eng.set_mh_proposal("iso", gm.mh_scale(prob), 0.5)
    plain = chain()
    eng.set_gibbs("stretch", ok[:, :D])
    one = chain()
    eng.set_gibbs("mh", ok[::-1, :D])
    both = chain()
    assert len({plain, one, both}) == 3
    eng.set_gibbs("stretch", ok[:1, :D])                      # replaced
    assert chain() not in (plain, one, both)
    eng.set_gibbs("stretch", ok[:, :D])
    assert chain() == both
    eng.set_gibbs("stretch", None)                            # cleared in one order ...
    eng.set_gibbs("mh", None)
    assert chain() == plain
    eng.set_gibbs("mh", ok[::-1, :D])
    eng.set_gibbs("stretch", ok[:, :D])
    assert chain() == both
    eng.set_gibbs("mh", None)                                 # ... and in the other
    assert chain() == one
    eng.set_gibbs("stretch", None)
    assert chain() == plain
    eng.close()
    # contexts a table is not built for
    per = _engine(prob, T, W)
    per.set_periodic(np.full(D, 3.0))
    with pytest.raises(NotImplementedError, match="not built for periodic parameters"):
        per.set_gibbs("stretch", ok[:, :D])
    per.close()
    three = _engine(prob, T, W)
    three.set_nsplits(3)
    with pytest.raises(NotImplementedError, match=r"two-set stretch move \(hens_set_nsplits\(2\)\)"):
        three.set_gibbs("stretch", ok[:, :D])
    three.close()
    rank = _engine(bprob, T, W)
    rank.pipe_init(1, 0)
    with pytest.raises(NotImplementedError, match="rank of the ladder pipeline or a ladder shard"):
        rank.set_gibbs("stretch", np.ones((1, bprob.D), dtype=bool))
    rank.close()
    shard = _engine(prob, 4, W, rung_range=(0, 2))
    with pytest.raises(NotImplementedError, match="rank of the ladder pipeline or a ladder shard"):
        shard.set_gibbs("stretch", ok[:, :D])
    shard.close()
    dist = _engine(prob, T, W)
    dist.set_dist_proposal(dm.box_spec(prob.centre - prob.half, prob.centre + prob.half), 0.5)
    dist.set_gibbs("stretch", ok[:, :D])                      # (the stretch move's table is its own)
    with pytest.raises(NotImplementedError, match="not built for the distribution proposal in the MH slot"):
        dist.set_gibbs("mh", ok[:, :D])
    dist.close()
    from eryn_amd.rj import _TemplateLikelihood
    rj = HipEnsemble(2, 16, 8, _TemplateLikelihood(8), -1.0, 1.0, tempered=True, live_dangerously=True)
    with pytest.raises(NotImplementedError, match="leaf-packing"):
        rj.set_gibbs("stretch", np.ones((1, 8), dtype=bool))
    rj.close()
    host = HipEnsemble(T, W, D, HostLikelihood(prob.loglike, D), prob.lo, prob.hi, live_dangerously=True)
    with pytest.raises(NotImplementedError, match="need a device likelihood"):
        host.set_gibbs("stretch", np.ones((1, D), dtype=bool))
    host.close()
    for Dg, kw in ((5, dict(pad_rows=False)), (130, {})):      # a generic row width
        mu, invcov = pu.gaussian_problem(Dg, dense=False)
        gen = HipEnsemble(2, 2 * Dg + 2, Dg, GaussianLikelihood(mu, np.diag(invcov).copy()), -50.0, 50.0, **kw)
        with pytest.raises(NotImplementedError, match=f"this context's rows are {Dg} wide"):
            gen.set_gibbs("stretch", np.ones((1, Dg), dtype=bool))
        gen.close()
