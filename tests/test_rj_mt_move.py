"""The specification of the multiple-try birth / death move (tests/rj_mt_move.py) on the CPU: it lands on the reference's fixtures
(tests/golden/rj_mt), K = 1 is the plain move, its own float64 values lie within its bounds, the production draws' words are distinct,
the refusals - and the sizing of every GPU case of tests/test_hip_rj_mt.py from the specification alone."""
import numpy as np
import pytest

from oracle import eryn_oracle_rj as orj
from tests import rj_mt_move as rm
from tests.parity_utils import knife_edge


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("name", rm.FIXTURES)
def test_specification_lands_on_the_reference(name):
    """From the fixture's two seeds the specification draws what the reference drew, in its order, and computes what it computed: masks,
    picks and positions bit for bit; lsw / aux_lsw / factors, mt_ll and mt_lp bit for bit or NaN for NaN; the state behind the move's
    update, behind its sweep and behind the in-model move; the ladder; the accept totals."""
    fx = rm.load_fixture(name)
    o = rm.fixture_oracle(fx)
    assert np.array_equal(o.st.P, fx["P0"]) and np.array_equal(o.st.L, fx["L0"])
    picks = nans = 0
    totals = np.zeros_like(fx["rj_accepted_total"])
    for it in range(int(fx["nsteps"])):
        acc = o.mh_move()
        pre = f"it{it}_mh_"
        assert np.array_equal(acc, fx[pre + "accepted"]), pre
        for b in o.branches:
            assert np.array_equal(o.st.x[b.name], fx[pre + f"x_{b.name}"]) and np.array_equal(o.st.inds[b.name], fx[pre + f"inds_{b.name}"]), pre
        assert np.array_equal(o.st.L, fx[pre + "L"]) and np.array_equal(o.st.P, fx[pre + "P"]) and np.array_equal(o.st.betas, fx[pre + "betas"]), pre
        rec = {}
        bi, racc = o.rj_move(rec)
        info = o.mt_infos[-1]
        pre = f"it{it}_rj_"
        assert bi == int(fx[pre + "branch"]), pre
        assert set(np.unique(fx[pre + "change"])) == {-1, 1}, "the reference needs births and deaths in every proposal"
        for k, v in (("change", info["change"]), ("leaf", info["leaf"]), ("tries", info["y"]), ("u_pick", info["u_pick"]), ("u_acc", info["u_acc"]),
                     ("pick", info["pick"]), ("keep", info["keep"])):
            assert np.array_equal(v, fx[pre + k]), f"{pre}{k}"
        for k in ("lsw", "aux_lsw", "factors", "mt_ll", "mt_lp"):
            assert _same(info[k], fx[pre + k]), f"{pre}{k}"
        for b in o.branches:
            assert np.array_equal(rec[f"rjupd_x_{b.name}"], fx[pre + f"move_x_{b.name}"]), f"{pre}move_x_{b.name}"
            assert np.array_equal(rec[f"rjupd_inds_{b.name}"], fx[pre + f"move_inds_{b.name}"]), f"{pre}move_inds_{b.name}"
            assert np.array_equal(o.st.x[b.name], fx[pre + f"x_{b.name}"]) and np.array_equal(o.st.inds[b.name], fx[pre + f"inds_{b.name}"]), pre
        assert np.array_equal(rec["rjupd_L"], fx[pre + "move_L"]) and np.array_equal(rec["rjupd_P"], fx[pre + "move_P"]), pre
        assert np.array_equal(racc, fx[pre + "accepted"]) and np.array_equal(o.st.L, fx[pre + "L"]) and np.array_equal(o.st.P, fx[pre + "P"]), pre
        assert np.array_equal(o.st.betas, fx[pre + "betas"]) and np.array_equal(o.swaps_accepted, fx[pre + "swaps"]), pre
        totals[bi] += racc
        picks += int((info["pick"] != 0).sum())
        nans += int(np.isnan(info["factors"]).sum())
        assert rm.knives(info, rm.exact_rj_mt(o, info)) == (0, 0), f"{pre}a decision on a knife edge (the GPU test on this fixture has no exemption)"
    assert np.array_equal(totals, fx["rj_accepted_total"]) and np.array_equal(o.rj_num_proposals, fx["rj_num_proposals"])
    assert picks > 0 and totals.sum() > 0 and (nans > 0) == (name == "rjmt2")


def test_fixtures_regenerate_from_their_generator(tmp_path):
    """tests/golden/make_golden_rj_mt.py reproduces the committed fixtures array for array (where the reference tree is: build container)."""
    import os
    import subprocess
    import sys
    if not os.path.isdir("/root/reference/src/eryn"):
        pytest.skip("the reference tree is not on this machine")
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    subprocess.run([sys.executable, os.path.join(here, "make_golden_rj_mt.py")], check=True, capture_output=True,
                   env=dict(os.environ, GOLDEN_OUT=str(tmp_path), PYTHONDONTWRITEBYTECODE="1"))
    for name in rm.FIXTURES:
        old = rm.load_fixture(name)
        with np.load(tmp_path / (name + ".npz"), allow_pickle=False) as f:
            new = {k: f[k] for k in f.files}
        assert sorted(old) == sorted(new)
        for k in old:
            assert _same(old[k], new[k]) if old[k].dtype.kind == "f" else np.array_equal(old[k], new[k]), f"{name}: {k}"


@pytest.mark.parametrize("name", sorted(rm.CASES))
def test_gpu_cases_are_sized_on_the_specification_alone(name):
    """No pick or accept knife edge, an accepted birth, an accepted death and a rejection, a pick other than try 0, and what the case
    names (-inf-prior tries, NaN factors, walkers at both edges): conditions on the inputs, so the GPU tests need no exemption.  The
    specification's own float64 sums lie within their bounds of exact arithmetic."""
    c = rm.CASES[name]

    def on_proposal(o, bi, inputs, info, ex, sweep, pre, mid):
        rm.mm.assert_sums(info["lsw"], info["aux_lsw"], info["factors"], ex, f"{name} (NumPy)")

    rm.assert_sized(rm.forced_run(c, on_proposal), c, name)


@pytest.mark.parametrize("name", sorted(rm.REPLAYS))
def test_replayed_cases_are_sized(name):
    """The free-running chains of the replay tests on NumPy streams: both outcomes of the move occur and nothing sits on a knife edge
    (the device's Philox streams are others: the GPU test asserts the same from the oracle's side of the replay)."""
    cname, schedule, in_model, iters, it0, _ = rm.REPLAYS[name]
    c = rm.CASES[cname]
    p = rm.case_problem(c)
    from tests.test_hip_leaf_kinds import _counting
    o = rm.case_oracle(c, p, cls=_counting(rm.MTOracleRJSampler), schedule=schedule, in_model=in_model, a=1.5)
    o.live = True
    for _ in range(iters):
        o.iteration()
    cnt = rm.Counts()
    for info in o.mt_infos:
        cnt.add(o, info, rm.exact_rj_mt(o, info))
    assert cnt.births >= 1 and cnt.deaths >= 1 and cnt.rejections >= 1, name


class _Forced(orj.OracleRJSampler):
    """The pinned oracle's plain birth / death move on given draws."""

    def load(self, change, leaf, birth, u_acc):
        self.f = dict(change=change, leaf=leaf, birth=birth, u_acc=u_acc)

    def _draw_coin(self, shape):
        return self.f["change"].copy()              # (the edge rule maps a forced +-1 onto itself)

    def _draw_leaf(self, tt, w, candidates):
        assert self.f["leaf"][tt, w] in candidates
        return self.f["leaf"][tt, w]

    def _draw_birth(self, b, bt, bw):
        return self.f["birth"][bt, bw]

    def _draw_accept(self, which):
        return self.f["u_acc"]


@pytest.mark.parametrize("name", ["w9_k2_nd64_two_gen", "w5_k64_nd130_four_branches"])
def test_one_try_from_the_prior_is_the_plain_move(name):
    """K = 1, generator = prior: lsw = w_0, the multiple-try factors reduce to -+ logq up to rounding, and - away from knife edges - the
    accept masks, records, log-priors and log-likelihoods are DistributionGenerateRJ's (the pinned oracle's ``_rj_propose``)."""
    c = dict(rm.CASES[name], K=1, gen=None)
    p = rm.case_problem(c)
    o = rm.case_oracle(c, p)
    ref = _Forced(p["obr"], p["x"], p["inds"], p["t"], p["y"], p["sigma"], None, None, p["betas"], like_fn=p["like_fn"], record=True)
    kept = 0
    for n in range(8):
        bi = n % len(o.branches)
        change, leaf, tries, u_pick, u_acc = o.draw_inputs(bi)
        info = {}
        keep, out = rm.mt_bd_step(o, bi, change, leaf, tries, u_pick, u_acc, info=info)
        ref.load(change, leaf, tries[:, :, 0], u_acc)
        rec = {}
        keep_ref = ref._rj_branch(bi, rec)
        with np.errstate(divide="ignore", invalid="ignore"):
            assert not knife_edge(rec["rj_lnpdiff"], np.log(u_acc)).any() and not knife_edge(info["lnpdiff"], np.log(u_acc)).any()
            np.testing.assert_allclose(info["factors"] + info["edge"], rec["rj_factors"], rtol=0, atol=1e-9)
        assert np.array_equal(keep, keep_ref), f"proposal {n}: accept masks"
        assert (out["pick"] == 0).all()
        for b in o.branches:
            assert np.array_equal(o.st.x[b.name], ref.st.x[b.name]) and np.array_equal(o.st.inds[b.name], ref.st.inds[b.name])
        assert np.array_equal(o.st.P, ref.st.P) and np.array_equal(o.st.L, ref.st.L)
        kept += int(keep.sum())
        o._pt(False, None)
        ref.st = orj.RJState(o.st.x, o.st.inds, o.st.L, o.st.P, o.st.betas)
    assert kept > 0


def _edge_state(c, p, full):
    """Every walker's proposed branch at its floor (all births) or its ceiling (all deaths)."""
    inds = {k: v.copy() for k, v in p["inds"].items()}
    b = p["obr"][0]
    inds[b.name][...] = False
    inds[b.name][..., :(b.nleaves_max if full else b.nleaves_min)] = True
    return inds


@pytest.mark.parametrize("full", [False, True])
def test_all_birth_and_all_death_proposals(full):
    """The reference cannot run a proposal without a death walker (inds_reverse_rj = None); the specification and the device can: every
    walker at the floor (all births) or at the ceiling (all deaths: every pick is try 0, the state after an accepted death carries the
    base's log-likelihood and log-prior)."""
    c = rm.CASES["w9_k2_nd64_two_gen"]
    p = rm.case_problem(c)
    p["inds"] = _edge_state(c, p, full)
    o = rm.case_oracle(c, p)
    change, leaf, tries, u_pick, u_acc = o.draw_inputs(0)
    assert (change == (-1 if full else +1)).all()
    info = {}
    keep, out = rm.mt_bd_step(o, 0, change, leaf, tries, u_pick, np.full_like(u_acc, 1e-300), gen=o.gens[0], info=info)
    ex = rm.exact_rj_mt(o, info)
    rm.mm.assert_sums(out["lsw"], out["aux_lsw"], out["factors"], ex, "all deaths" if full else "all births")
    b = o.branches[0]
    if full:
        assert (out["pick"] == 0).all()
        assert np.array_equal(out["mt_ll"], info["ll_in"].reshape(o.T, o.W)) and np.array_equal(out["mt_lp"], info["lp_in"].reshape(o.T, o.W))
        assert (o.st.inds[b.name].sum(axis=-1)[keep] == b.nleaves_max - 1).all() and keep.any()
        assert np.isnan(out["factors"]).any(), "a dying leaf outside the generator gives a NaN factor"
        assert not keep[np.isnan(out["factors"])].any()
    else:
        assert (o.st.inds[b.name].sum(axis=-1)[keep] == b.nleaves_min + 1).all() and keep.any()
        tt, ww = np.where(keep)
        picked = info["y"][tt, ww, out["pick"][tt, ww]]
        assert np.array_equal(o.st.x[b.name][tt, ww, leaf[tt, ww]], picked)


def test_no_two_draws_of_an_iteration_share_a_philox_word():
    """Counter word 3 of every call a walker makes in one iteration - in-model normals and accept uniform, per branch coin / selector,
    accept, pick and K tries of up to four parameters - is distinct; parameter, try and branch sit in disjoint bit fields."""
    keys = rm.iteration_keys(4, 124, (4, 4, 4, 4), rm.MAX_TRY)
    assert len(set(keys)) == len(keys)
    for b in range(4):
        for k in range(1, rm.MAX_TRY):
            for d in range(4):
                w = rm.try_key(b, d, k)
                assert (w & 0xFF, (w >> 8) & 3, (w >> 10) & 63, w >> 16) == (rm.PURPOSE_RJ_TRY, d, k, b)
    assert rm.try_key(2, 1, 0) == rm.rpt.PURPOSE_RJ_BIRTH | (1 << 8) | (2 << 16)      # try 0 of a birth: the plain move's call
    # (the stretch move's words: purposes 25 and 26; the cascades': 9 and 10 - other low bytes)
    assert {k & 0xFF for k in keys} == {12, rm.PURPOSE_RJ_ACC, rm.PURPOSE_RJ_BD, rm.PURPOSE_RJ_BIRTH, rm.PURPOSE_RJ_TRY, rm.PURPOSE_RJ_PICK}


def test_production_tries_are_the_generators_constructions():
    """Try 0 is the plain move's birth draw (tests/rj_prior_terms.birth_words), every value lies in its generator's support, and a
    uniform parameter is bit for bit u (hi - lo) + lo."""
    gen = rm.pt.make_spec(rm.GEN_PULSE_TERMS)
    X, Xs, E = rm.mt_draws(77, 5, 3, 4, 6, 1, gen)
    for d in range(3):
        x0, _, _ = rm.rpt.birth_spec(gen, d, rm.rpt.birth_words(77, 5, 3, 4, 1, d))
        assert np.array_equal(X[:, :, 0, d], x0)
    assert ((X[..., 0] >= 0.5) & (X[..., 0] <= 7.0)).all() and ((X[..., 2] >= 0.05) & (X[..., 2] <= 0.21)).all()
    assert (np.abs(X - Xs.astype(np.float64)) <= E + 4 * rm.U * np.abs(X)).all()
    u = rm.pick_uniforms(77, 5, 3, 4, 1)
    assert u.shape == (3, 4) and ((u >= 0) & (u < 1)).all() and len(np.unique(u)) == 12


def test_refusals():
    c = rm.CASES["w9_k2_nd64_two_gen"]
    p = rm.case_problem(c)
    with pytest.raises(ValueError, match="one model at a time"):
        rm.case_oracle(c, p, schedule="together")
    fixed = dict(c, nl_min=(3, 0))
    pf = rm.case_problem(fixed)
    o = rm.case_oracle(fixed, pf)
    with pytest.raises(ValueError, match="nleaves_min != nleaves_max"):
        o.draw_inputs(0)
    from eryn_amd.rj import MTDistGenMoveRJ
    with pytest.raises(ValueError, match="num_try"):
        MTDistGenMoveRJ({"pulse": [(0.0, 1.0)] * 3}, num_try=65)
    with pytest.raises(ValueError, match="num_try"):
        MTDistGenMoveRJ({"pulse": [(0.0, 1.0)] * 3}, num_try=0)
    with pytest.raises(NotImplementedError, match="rj=True"):
        MTDistGenMoveRJ({"pulse": [(0.0, 1.0)] * 3}, num_try=3, rj=False)
    with pytest.raises(ValueError, match="gibbs_sampling_setup"):
        MTDistGenMoveRJ({"pulse": [(0.0, 1.0)] * 3, "sine": [(0.0, 1.0)] * 3}, num_try=3, gibbs_sampling_setup="nobody")
    # a move's own leaf budget must be the sampler's (refused before a context exists)
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, TemplateLikelihood
    box = [(0.0, 1.0), (-1.0, 1.0), (0.01, 0.2)]
    for kw, word in ((dict(nleaves_min={"pulse": 1}), "nleaves_min"), (dict(nleaves_max=4), "nleaves_max")):
        with pytest.raises(ValueError, match=f"{word} differs from the sampler's"):
            RJEnsembleSampler(8, {"pulse": 3}, TemplateLikelihood({"pulse": "pulse"}, p["t"], p["y"], 1.0), {"pulse": box},
                              tempering_kwargs=dict(ntemps=2), branch_names=["pulse"], nleaves_max={"pulse": 3}, nleaves_min={"pulse": 0},
                              moves=GaussianLeafMove({"pulse": np.eye(3) * 1e-4}), rj_moves=MTDistGenMoveRJ({"pulse": box}, num_try=3, **kw))
