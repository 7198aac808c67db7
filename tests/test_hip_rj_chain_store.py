"""The chain store of leaf-packing contexts: RJEnsembleSampler(backend=RJDeviceBackend()) (include/hipensemble.h: hens_rj_chain_*,
hens_rj_step_chain; csrc/hens_rj_chain.h: k_rj_chain_store) against the same tree's host path from the same seed - the sampler
without ``backend=``, whose stored States the oracle replays of tests/test_hip_rj.py pin.  Everything is compared bit for bit
(np.array_equal; NaN positions through np.isnan masks): no tolerance anywhere.

Per case three contexts run the same chain: the host sampler (a download + unpack + State per stored step), the device sampler
(one hens_rj_step_chain per segment), and a bare engine stepped step(thin_by - 1), counters(), step(1), counters(), download() per
stored step - the yardstick of the accept totals (the reference stores the accept counts of a stored step's LAST sub-iteration,
ensemble.py:968-979), of every stored step's Philox checkpoint and, without a reversible-jump move, of the swap totals.  Under a
reversible-jump schedule the swap totals are the in-model cascade's of each stored step's last iteration: those are replayed
through the oracle with the draws the device consumed (test_swap_totals_under_a_birth_death_schedule)."""
import numpy as np
import pytest

from tests import leaf_kind_cases as cases

pytestmark = pytest.mark.gpu

WIDTH = {"pulse": 3, "sine": 3, "offset": 1, "ramp": 2, "burst": 4}
SIGMA = 3.0          # noise of the data: wide enough that births and deaths are both accepted within a few iterations
NDATA = 40


def case(kinds, nl_max, nl_min=None, T=4, W=10, rj="separate_branches", move="diag", thin=1, burn=0, nsteps=6, Ts=None, seed=101):
    return dict(kinds=kinds, nl_max=nl_max, nl_min=nl_min or (0,) * len(kinds), T=T, W=W, rj=rj, move=move, thin=thin, burn=burn,
                nsteps=nsteps, Ts=Ts, seed=seed)


# the smallest shapes at which the append can still go wrong (records: RW = ncoord + nbranches, rounded up to even)
CASES = {
    # second branch from the odd offset 9, RW 24 with a pad, 40 records: fewer than a wave holds at 16 lanes each; 8-byte lanes
    "odd_offsets": case(("pulse", "sine"), (3, 4), burn=2),
    "one_branch_thin3": case(("pulse",), (5,), (1,), thin=3, burn=1, nsteps=5),
    # widths 1, 2, 3, 4 (the WIDE instantiations): segments 3 | 4 | 6 | 8 from offsets 0, 3, 7, 13 - every alignment; W = 33
    "four_widths_W33_together_Ts2": case(("offset", "ramp", "pulse", "burst"), (3, 2, 2, 2), W=33, rj="together", Ts=2),
    # 64 leaf slots: mask bits up to 2^31, RW 98, every segment even: the 16-byte lanes.  (This and the next case compare the device
    # chain with the host path of the same kernels: the append at these shapes.  k_rj itself is held to the oracle at them in
    # tests/test_hip_limit_records.py.)
    "slots64_iterate": case(("offset", "ramp"), (32, 32), rj="iterate_branches", nsteps=5),
    "pulses_RW126": case(("pulse", "pulse"), (21, 20), nsteps=4),
    "no_rj_Ts1_thin3": case(("pulse", "sine"), (3, 4), rj=None, thin=3, burn=2, Ts=1),
    # full leaf covariances; the stored steps straddle the iteration whose counter % 64 == 63 (the resident templates' refresh)
    "fullcov_across_the_refresh": case(("pulse", "sine"), (3, 4), move="full", burn=61, nsteps=5),
    "stretch_thin3_Ts2": case(("pulse", "sine"), (3, 4), move="stretch", thin=3, burn=1, nsteps=5, Ts=2),
}


def names_of(c):
    return [k if c["kinds"].count(k) == 1 else f"{k}_{i}" for i, k in enumerate(c["kinds"])]


def problem(c):
    """Data, a random start (every slot holds a leaf from the box, masks at random: dead leaves have coordinates, some walkers have
    no leaf in a branch) and a ladder with hot upper rungs."""
    rs = np.random.RandomState(c["seed"])
    names = names_of(c)
    brs = cases.branches_of(c["kinds"], c["nl_max"], c["nl_min"])
    t = np.linspace(-1, 1, NDATA)
    y = cases.make_data(brs, t, SIGMA, rs)
    x, inds = {}, {}
    for n, k, nl, nm in zip(names, c["kinds"], c["nl_max"], c["nl_min"]):      # (per branch: two branches may be of one kind)
        xb, ib = cases.random_state(cases.branches_of((k,), (nl,), (nm,)), c["T"], c["W"], rs)
        x[n], inds[n] = xb[k], ib[k]
    return names, t, y, x, inds, 0.35 ** np.arange(c["T"])


def make_sampler(c, backend=None):
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler, StretchLeafMove, TemplateLikelihood
    names, t, y, _, _, _ = problem(c)
    box = {n: cases.BOX[k] for n, k in zip(names, c["kinds"])}
    priors = {n: {i: uniform_dist(lo, hi) for i, (lo, hi) in enumerate(box[n])} for n in names}
    sd = {n: np.array([0.02 * (hi - lo) for lo, hi in box[n]]) for n in names}
    if c["move"] == "stretch":
        move = StretchLeafMove(live_dangerously=True)
    elif c["move"] == "full":
        rot = np.array([[1.0, 0.3, -0.2], [0.0, 1.0, 0.4], [0.0, 0.0, 1.0]])
        move = GaussianLeafMove({n: (rot * sd[n]) @ (rot * sd[n]).T for n in names})
    else:
        move = GaussianLeafMove({n: np.diag(sd[n] ** 2) for n in names})
    return RJEnsembleSampler(c["W"], {n: WIDTH[k] for n, k in zip(names, c["kinds"])},
                             TemplateLikelihood(dict(zip(names, c["kinds"])), t, y, SIGMA), priors, tempering_kwargs=dict(ntemps=c["T"]),
                             branch_names=names, nleaves_max=dict(zip(names, c["nl_max"])), nleaves_min=dict(zip(names, c["nl_min"])),
                             moves=move, rj_moves=c["rj"], rng="philox", seed=c["seed"], backend=backend)


def start_state(c):
    from eryn_amd.state import State
    _, _, _, x, inds, betas = problem(c)
    return State(x, inds=inds, betas=betas)


def yardstick(c):
    """A bare engine on the same chain: what run_mcmc does in front of its loop, ``burn`` single iterations, then per stored step
    step(thin_by - 1), counters(), [the resident masks], step(1), counters(), download().  Returns the per-step downloads, the
    accept / swap totals of the last iterations, the Philox checkpoints and, per stored step and leaf slot (every branch's, in order),
    by how many walkers of the whole ensemble more have the slot in use behind the last iteration than in front of it.  Swaps move
    whole walkers and the in-model move leaves the masks alone, so a slot that gained users saw a birth and one that lost users a
    death, whatever else happened."""
    s = make_sampler(c)
    eng, st = s.engine, start_state(c)
    coords, inds = st.branches_coords, st.branches_inds
    s.temperature_control.betas = np.array(st.betas, dtype=np.float64)
    L, P = s._eval(coords, inds)
    eng.upload(coords, inds, L, P, s.temperature_control.betas)
    eng.set_adapt_time(s.temperature_control.time)
    for _ in range(c["burn"]):
        eng.step(1)
    out = dict(steps=[], acc=np.zeros((c["T"], c["W"])), bd=np.zeros((c["T"], c["W"])), swaps=np.zeros(c["T"] - 1), rstates=[], grew=[])
    for _ in range(c["nsteps"]):
        eng.step(c["thin"] - 1)
        c0 = eng.counters()
        before = eng.debug_resident()[1]
        eng.step(1)
        c1 = eng.counters()
        out["acc"] += c1["accepted_mh"] - c0["accepted_mh"]
        out["bd"] += c1["accepted_bd"] - c0["accepted_bd"]
        out["swaps"] += c1["swaps_last"]
        out["rstates"].append(("philox", c["seed"], eng.iteration(), int(c1["adapt_time"])))
        step = eng.download(nan_fill=True)
        out["steps"].append(step)
        out["grew"].append(np.concatenate([step[1][n].sum(axis=(0, 1)).astype(int) - before[n].sum(axis=(0, 1)).astype(int) for n in names_of(c)]).tolist())
    eng.close()
    return out


def same(a, b):
    """bit for bit, NaN where and only where the other has one"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def assert_chain_is_the_host_chain(bk, chain, Ts, what):
    n = len(chain)
    x, inds, nl = bk.get_chain(), bk.get_inds(), bk.get_nleaves()
    assert bk.iteration == n
    for k in bk.branch_names:
        assert x[k].dtype == np.float64 and inds[k].dtype == np.bool_
        assert same(x[k], np.stack([s.branches[k].coords[:Ts] for s in chain])), f"{what}: coordinates of {k}"
        assert np.array_equal(inds[k], np.stack([s.branches[k].inds[:Ts] for s in chain])), f"{what}: leaf masks of {k}"
        assert np.array_equal(nl[k], np.stack([s.branches[k].nleaves[:Ts] for s in chain])), f"{what}: leaf counts of {k}"
        assert np.array_equal(np.isnan(x[k]), np.broadcast_to(~inds[k][..., None], x[k].shape)), f"{what}: NaN exactly on the unused leaves of {k}"
    assert np.array_equal(bk.get_log_like(), np.stack([s.log_like[:Ts] for s in chain])), f"{what}: log_like"
    assert np.array_equal(bk.get_log_prior(), np.stack([s.log_prior[:Ts] for s in chain])), f"{what}: log_prior"
    assert np.array_equal(bk.get_betas(), np.stack([s.betas for s in chain])), f"{what}: betas"


def assert_states_equal(a, b, what):
    for k in a.branches:
        assert np.array_equal(a.branches[k].inds, b.branches[k].inds), f"{what}: leaf masks of {k}"
        assert np.array_equal(a.branches[k].coords, b.branches[k].coords), f"{what}: coordinates of {k} (dead slots included)"
    for f in ("log_like", "log_prior", "betas"):
        assert np.array_equal(getattr(a, f), getattr(b, f)), f"{what}: {f}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_chain_is_the_host_chain(name):
    from eryn_amd.backend import RJDeviceBackend
    c = CASES[name]
    T, W, Ts = c["T"], c["W"], c["Ts"] or c["T"]
    host, dev = make_sampler(c), make_sampler(c, RJDeviceBackend(ntemps_store=c["Ts"]))
    last_h = host.run_mcmc(start_state(c), c["nsteps"], burn=c["burn"], thin_by=c["thin"])
    last_d = dev.run_mcmc(start_state(c), c["nsteps"], burn=c["burn"], thin_by=c["thin"])
    bk = dev.backend
    assert len(host.chain) == c["nsteps"] and dev.chain == [] and dev.iteration == host.iteration == c["burn"] + c["nsteps"]
    assert_chain_is_the_host_chain(bk, host.chain, Ts, name)
    assert bk.downloads == 1, "the accessors downloaded the open segment more than once"
    nl = dev.get_nleaves()
    assert all(np.array_equal(nl[k], v) for k, v in bk.get_nleaves().items())
    assert_states_equal(last_d, last_h, f"{name}: the State run_mcmc returns")
    # the resident state behind the run: the host run's, dead leaves' coordinates still in place
    (xd, id_, Ld), (xh, ih, Lh) = dev.engine.debug_resident(), host.engine.debug_resident()
    dead_with_coords = 0
    for k in bk.branch_names:
        assert np.array_equal(id_[k], ih[k]) and np.array_equal(xd[k], xh[k]) and not np.isnan(xd[k]).any(), f"{name}: resident {k}"
        dead_with_coords += int((~id_[k] & (xd[k] != 0.0).any(axis=-1)).sum())
    assert np.array_equal(Ld, Lh) and dead_with_coords > 0
    # the post-run counters are the host run's
    for a, b in ((dev.moves[0].accepted, host.moves[0].accepted), (dev.rj_accepted_all, host.rj_accepted_all),
                 (dev.temperature_control.swaps_accepted, host.temperature_control.swaps_accepted)):
        assert np.array_equal(a, b)
    assert dev.temperature_control.time == host.temperature_control.time and dev.moves[0].num_proposals == host.moves[0].num_proposals
    # totals and checkpoints against the bare engine, which is on the same chain
    y = yardstick(c)
    for i, (x, inds, L, P, betas) in enumerate(y["steps"]):
        assert np.array_equal(L, host.chain[i].log_like) and np.array_equal(betas, host.chain[i].betas), f"{name}: the yardstick left the chain at step {i}"
    print(f"{name}: accepted {bk.accepted.sum():.0f} / {y['acc'].sum():.0f}, rj_accepted {bk.rj_accepted.sum():.0f} / {y['bd'].sum():.0f}, "
          f"swaps {bk.swaps_accepted} / {y['swaps']}, users gained per (step, leaf slot) {y['grew']}")
    assert np.array_equal(bk.accepted, y["acc"][:Ts]), f"{name}: accepted"
    assert np.array_equal(bk.rj_accepted, y["bd"][:Ts]), f"{name}: rj_accepted"
    assert bk.get_random_states() == y["rstates"] and bk.random_state == y["rstates"][-1]
    if c["rj"] is None:
        assert np.array_equal(bk.swaps_accepted, y["swaps"]), f"{name}: swaps_accepted (no birth / death move: swaps_last is the in-model cascade's)"
    # the case is not trivial: in-model accepts, swaps, and - under a birth / death schedule - accepted births and deaths
    assert y["acc"][:Ts].sum() > 0 and bk.swaps_accepted.sum() > 0 and bk.swaps_accepted.shape == (T - 1,)
    grew = np.array(y["grew"])
    if c["rj"] is None:
        assert not grew.any() and not bk.rj_accepted.any()
    else:
        assert y["bd"][:Ts].sum() > 0 and (grew > 0).any() and (grew < 0).any(), f"{name}: births and deaths must both occur: {y['grew']}"
    # some walker has no leaf in some branch: an all-NaN row is stored
    if name == "odd_offsets":
        assert any(np.isnan(v).all(axis=(-1, -2)).any() for v in bk.get_chain().values())
    if name == "slots64_iterate":
        assert all(v[..., 31].any() for v in bk.get_inds().values()), "mask bit 31 must be in use"
    # discard / thin read the same arrays
    assert same(bk.get_chain(discard=1, thin=2)[bk.branch_names[0]], bk.get_chain()[bk.branch_names[0]][1::2])
    assert np.array_equal(bk.get_log_like(discard=2), bk.get_log_like()[2:]) and bk.get_random_states(discard=1, thin=2) == y["rstates"][1::2]
    host.engine.close(), dev.engine.close()


def test_segments_append_and_reset():
    """max_bytes that holds 3 stored steps in a run of 8: two closures in the middle, one download each, totals summed across the
    segments; a second run_mcmc(None, ...) appends; reset starts again."""
    from eryn_amd.backend import RJDeviceBackend
    c = dict(CASES["odd_offsets"], nsteps=8)
    step_bytes = RJDeviceBackend.bytes_per_step(c["T"], c["W"], 21, 7)
    assert step_bytes == 8 * (4 * 10 * 23 + 4) + 4 * 10 * 7
    host, dev = make_sampler(c), make_sampler(c, RJDeviceBackend(max_bytes=3 * step_bytes + 5))
    assert dev.engine.chain_info()["step_bytes"] == step_bytes
    host.run_mcmc(start_state(c), 8, burn=c["burn"])
    dev.run_mcmc(start_state(c), 8, burn=c["burn"])
    bk = dev.backend
    assert bk.max_steps == 3 and bk.capacity == 3 and bk.downloads == 2          # (segments 3 + 3 closed, 2 open)
    assert_chain_is_the_host_chain(bk, host.chain, c["T"], "three segments")
    assert bk.downloads == 3
    y = yardstick(c)
    assert np.array_equal(bk.accepted, y["acc"]) and np.array_equal(bk.rj_accepted, y["bd"]) and bk.get_random_states() == y["rstates"]
    assert bk.accepted.sum() > 0 and bk.rj_accepted.sum() > 0 and bk.swaps_accepted.sum() > 0
    swaps8 = bk.swaps_accepted.copy()
    # a second run appends - to the chain, the totals and the sampler's iteration
    host.run_mcmc(None, 4, thin_by=2)
    dev.run_mcmc(None, 4, thin_by=2)
    assert bk.iteration == 12 and dev.iteration == host.iteration
    assert_chain_is_the_host_chain(bk, host.chain, c["T"], "appended")
    assert (bk.accepted >= y["acc"]).all() and bk.accepted.sum() > y["acc"].sum() and (bk.swaps_accepted >= swaps8).all()
    assert bk.random_state == ("philox", c["seed"], c["burn"] + 8 + 8, dev.temperature_control.time)
    # reset starts again: same shape, the device buffers are kept
    bk.reset(dev.nwalkers, dev.ndims, ntemps=dev.ntemps, branch_names=dev.branch_names, nleaves_max=dev.nleaves_max)
    assert bk.iteration == 0 and bk.capacity == 3 and not bk.accepted.any() and not bk.rj_accepted.any() and not bk.swaps_accepted.any()
    assert bk.get_log_like().shape == (0, 4, 10) and bk.get_chain()["sine"].shape == (0, 4, 10, 4, 3) and bk.get_inds()["pulse"].dtype == np.bool_
    host.chain.clear()
    host.run_mcmc(None, 2)
    dev.run_mcmc(None, 2)
    assert_chain_is_the_host_chain(bk, host.chain, c["T"], "after reset")
    host.engine.close(), dev.engine.close()


@pytest.mark.parametrize("schedule,T,W,nl_max,nl_min,seed,start", [
    ("separate_branches", 4, 10, (3, 4), (0, 0), 11, (2, 1)), ("iterate_branches", 3, 8, (4, 3), (0, 1), 13, (2, 1)),
    ("together", 3, 8, (4, 3), (0, 0), 17, (2, 2))])
def test_swap_totals_under_a_birth_death_schedule(monkeypatch, schedule, T, W, nl_max, nl_min, seed, start):
    """swaps_accepted under a reversible-jump schedule: the counts of the IN-MODEL cascade of every stored step's last iteration
    (the reference's in_model_swaps, ensemble.py:976-979, 1026) - on the device set aside before the birth / death move's cascade
    overwrites swaps_last.  The oracle replay of tests/test_hip_rj.py, its engine stepping through hens_rj_step_chain (one stored
    step per call, of 3 and of 5 iterations) and its oracle recording what every adapting cascade counted: integer counts, equal
    exactly.  The replay itself holds the chain, the counters and swaps_last to the oracle as ever."""
    from eryn_amd.rj import RJEngine
    from tests import test_hip_rj as thr
    base = thr._replay_oracle_class()

    class Recording(base):
        def _pt(self, adapt, rec):
            super()._pt(adapt, rec)
            which = "in_model_swaps" if adapt else "bd_swaps"
            setattr(self, which, getattr(self, which, []) + [self.swaps_accepted.copy()])

    got = {}

    def step(self, n):
        if not got:
            self.chain_create(4)
            got["stored"] = 0
        self.step_chain(1, n)
        got["stored"] += 1

    close = RJEngine.close

    def close_and_keep(self):
        got["totals"], got["info"] = self.chain_totals(), self.chain_info()
        got["iteration"] = list(self.chain_download(fields=())["iteration"])
        close(self)

    monkeypatch.setattr(thr, "_replay_oracle_class", lambda: Recording)
    monkeypatch.setattr(RJEngine, "step", step)
    monkeypatch.setattr(RJEngine, "close", close_and_keep)
    o = thr._replay_rj(T, W, nl_max, nl_min, ndata=60, iters=8, seed=seed, start_leaves=start, calls=(3, 5), schedule=schedule)
    assert got["stored"] == 2 and got["info"]["count"] == 2 and got["iteration"] == [3, 8] and len(o.in_model_swaps) == 8
    want = o.in_model_swaps[2] + o.in_model_swaps[7]
    print(f"{schedule}: in-model swaps of iterations 2 and 7: {o.in_model_swaps[2]} + {o.in_model_swaps[7]}; device {got['totals'][2]}")
    assert np.array_equal(got["totals"][2], want) and want.sum() > 0
    other = o.bd_swaps[2] + o.bd_swaps[7]
    assert not np.array_equal(other, want), "the birth / death cascades' counts must differ from the in-model cascades', or the case shows nothing"


def test_protocol():
    from eryn_amd.backend import RJDeviceBackend
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, LeafBranch, RJEngine, RJEnsembleSampler, _TemplateLikelihood
    from eryn_amd._lib import check
    # no model yet
    bare = HipEnsemble(2, 16, 16, _TemplateLikelihood(16), -1.0, 1.0, tempered=True, live_dangerously=True)
    with pytest.raises(RuntimeError, match="hens_rj_set_model"):
        check(bare.lib.hens_rj_chain_create(bare.ctx, 4, 0), bare.ctx)
    bare.close()
    # a model without a device likelihood
    gen = RJEngine(2, 8, [LeafBranch("a", [(0.0, 1.0), (0.0, 1.0)], 3)], None, None, 1.0)
    with pytest.raises(NotImplementedError, match="device likelihood"):
        gen.chain_create(4)
    gen.close()
    # not a leaf-packing context
    c = CASES["odd_offsets"]
    s = make_sampler(c)
    eng, st = s.engine, start_state(c)
    with pytest.raises(RuntimeError, match="no chain"):
        eng.step_chain(1)
    with pytest.raises(ValueError):
        eng.chain_create(0)
    with pytest.raises(ValueError):
        eng.chain_create(4, 5)
    s.run_mcmc(st, 0)                                   # (a state on the device)
    eng.chain_create(3, 2)
    info = eng.chain_info()
    assert info["capacity"] == 3 and info["count"] == 0 and info["ntemps_store"] == 2 and info["step_bytes"] == 8 * (2 * 10 * 23 + 4) + 2 * 10 * 7
    it0 = eng.iteration()
    with pytest.raises(RuntimeError, match="do not fit"):
        eng.step_chain(4)                               # overfull: refused before any launch
    assert eng.iteration() == it0 and eng.chain_info()["count"] == 0
    with pytest.raises(ValueError):
        eng.step_chain(1, 0)
    with pytest.raises(ValueError):
        eng.step_chain(-1)
    eng.eng.set_profiling(1)
    eng.step_chain(2, 2)
    info = eng.chain_info()
    assert info["count"] == 2 and info["n_store_timed"] == 2 and info["store_ms"] > 0.0 and eng.iteration() == it0 + 4
    eng.eng.set_profiling(0)
    with pytest.raises(RuntimeError, match="do not fit"):
        eng.step_chain(2)
    assert eng.iteration() == it0 + 4
    for first, count in ((0, 3), (2, 1), (3, 0), (-1, 1), (1, -1)):
        with pytest.raises(ValueError):
            eng.chain_download(first, count)
    assert eng.chain_download(2, 0)["iteration"].shape == (0,) and eng.chain_download(1, 1)["x"]["sine"].shape == (1, 2, 10, 4, 3)
    x = np.empty((2, 2, 10, 4, 3))
    for branch in (2, -2, 7):
        with pytest.raises(ValueError, match="branch"):
            check(eng.lib.hens_rj_chain_download(eng.ctx, 0, 2, branch, None, None, None, None, None, None, None), eng.ctx)
    with pytest.raises(ValueError, match="branch"):     # (branch -1: the shared fields only)
        check(eng.lib.hens_rj_chain_download(eng.ctx, 0, 2, -1, x.ctypes.data, None, None, None, None, None, None), eng.ctx)
    # upload / set_iteration / reset_counters leave the chain and its totals alone; a resumed run appends
    tot = eng.chain_totals()
    xs, inds, L, P, betas = eng.download()
    eng.eng.reset_counters()
    eng.upload(xs, inds, L, P, betas)
    eng.set_iteration(100)
    assert all(np.array_equal(a, b) for a, b in zip(tot, eng.chain_totals())) and eng.chain_info()["count"] == 2
    eng.step_chain(1, 1)
    assert list(eng.chain_download(fields=())["iteration"]) == [it0 + 2, it0 + 4, 101]
    assert all((a >= b).all() for a, b in zip(eng.chain_totals(), tot))
    eng.chain_reset()
    assert not any(a.any() for a in eng.chain_totals()) and eng.chain_info()["count"] == 0 and eng.chain_info()["capacity"] == 3
    eng.chain_destroy()
    assert eng.chain_info()["capacity"] == 0
    with pytest.raises(RuntimeError, match="no chain"):
        eng.chain_totals()
    # the fixed-dimension family stays closed to leaf-packing contexts
    with pytest.raises(NotImplementedError, match="leaf-packing"):
        eng.eng.chain_create(4)
    eng.close()
    # the sampler: device draws and a device likelihood
    names, t, y, _, _, _ = problem(c)
    priors = {n: {i: uniform_dist(lo, hi) for i, (lo, hi) in enumerate(cases.BOX[k])} for n, k in zip(names, c["kinds"])}
    kw = dict(tempering_kwargs=dict(ntemps=2), branch_names=names, nleaves_max=dict(zip(names, (3, 4))),
              moves=GaussianLeafMove({n: np.eye(3) * 1e-4 for n in names}), backend=RJDeviceBackend())
    from eryn_amd.rj import TemplateLikelihood
    with pytest.raises(NotImplementedError, match="philox"):
        RJEnsembleSampler(8, {n: 3 for n in names}, TemplateLikelihood(dict(zip(names, c["kinds"])), t, y, SIGMA), priors, rng="numpy", **kw)
    for rng in ("numpy", "philox"):
        with pytest.raises(NotImplementedError):
            RJEnsembleSampler(8, {n: 3 for n in names}, lambda x: 0.0, priors, rng=rng, **kw)
    with pytest.raises(NotImplementedError, match="RJDeviceBackend"):
        RJEnsembleSampler(8, {n: 3 for n in names}, TemplateLikelihood(dict(zip(names, c["kinds"])), t, y, SIGMA), priors, rng="philox",
                          **dict(kw, backend=object()))
