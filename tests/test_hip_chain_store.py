"""GPU tests of the chain store (include/hipensemble.h: hens_chain_*, hens_step_chain; csrc/hens_chain.h: k_chain_store;
eryn_amd.backend.DeviceBackend): the stored steps of ``run_mcmc(store=True)`` kept on the device.

The yardstick is the host path in the same tree - ``Backend`` fed by ``eng.download()`` after every stored step, which the oracle
replays pin - from the same seed: every comparison here is bit-exact equality (np.array_equal), no tolerance.

One thing is NOT compared: ``get_betas`` of an untempered sampler.  ``Backend`` never writes those rows (np.empty); the device chain
stores zeros.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from eryn_amd.backend import Backend, DeviceBackend
from eryn_amd.engine import HipEnsemble
from eryn_amd.ensemble import EnsembleSampler
from eryn_amd.likelihood import GaussianLikelihood, RosenbrockLikelihood
from eryn_amd.moves import GaussianMove, StretchMove
from eryn_amd.prior import uniform_dist
from eryn_amd.state import State

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSTEPS = 12
LAG, NU = 50, 10              # a strong adaptation: the ladder moves within a case's dozen stored steps


def case(T, W, D, like="dense", mix=False, periodic=False, nsplits=2, reps=1, env=None, path=None):
    """``path``: what a profiled hens_step call reports for the shape without a chain - "one" launch per iteration (k_iter), "two"
    in-place launches, "copying"; None: not asked (see test_launch_path_is_the_shapes_own)."""
    return dict(T=T, W=W, D=D, like=like, mix=mix, periodic=periodic, nsplits=nsplits, reps=reps, env=env or {}, path=path)


CASES = {
    # one launch per iteration (k_iter): accepted rows sit in the pool's other half until somebody leaves record mode
    "one_launch_D16": case(4, 64, 16, path="one"),
    "one_launch_D32": case(4, 64, 32, path="one", reps=2),
    # two in-place launches, records in column order (full tiles: tests/ladders.py) / slot order (short tiles)
    "two_col_T16": case(16, 40, 8, path="two"),
    "two_col_T8": case(8, 48, 8, path="two"),
    "two_short_T10": case(10, 256, 8, path="two"),
    # slot-ordered records: the Gaussian move in the mix
    "mh_mix": case(4, 64, 8, mix=True),
    # by-field state: three sets, more than 64 rungs, a generic row width
    "three_sets": case(4, 66, 8, nsplits=3, path="copying"),
    "long_T70": case(70, 32, 8, path="copying"),
    "generic_D5": case(5, 100, 5, env={"HENS_NO_PAD": "1"}, path="copying"),
    # padded rows: 11 real parameters in rows of 16 (destination rows 8-byte aligned only), 12 in 16
    "padded_D11": case(4, 64, 11),
    "padded_D12": case(4, 64, 12),
    "untempered": case(1, 64, 8),
    "odd_W": case(4, 33, 8),
    "periodic": case(4, 64, 8, periodic=True),
    "rosenbrock": case(4, 64, 8, like="rosen"),
    "diag": case(4, 64, 8, like="diag"),
}


def problem(c):
    D = c["D"]
    rs = np.random.RandomState(3)
    A = rs.randn(D, D)
    mu, invcov = 0.1 * rs.randn(D), np.linalg.inv(A @ A.T / D + np.eye(D))
    if c["like"] == "rosen":
        like, box = RosenbrockLikelihood(D), 6.0
    elif c["like"] == "diag":
        like, box = GaussianLikelihood(mu, np.diag(np.diag(invcov))), 20.0
    else:
        like, box = GaussianLikelihood(mu, invcov), 20.0
    x0 = np.random.RandomState(1).randn(c["T"], c["W"], D) * (0.3 if c["like"] == "rosen" else 1.0)
    if c["periodic"]:
        x0[..., 2] = np.random.RandomState(2).uniform(0.0, 3.0, size=x0.shape[:2])
    return like, box, x0


def sampler(c, backend, seed=77):
    like, box, _ = problem(c)
    D = c["D"]
    priors = {i: uniform_dist(-box, box) for i in range(D)}
    kw = {}
    if c["T"] > 1:
        kw["tempering_kwargs"] = dict(ntemps=c["T"], adaptation_lag=LAG, adaptation_time=NU)
    if c["periodic"]:
        kw["periodic"] = {"model_0": {2: 3.0}}
    stretch = StretchMove(nsplits=c["nsplits"])
    moves = [(stretch, 0.5), (GaussianMove({"model_0": 0.05 * np.eye(D)}), 0.5)] if c["mix"] else stretch
    return EnsembleSampler(c["W"], D, like, priors, rng="philox", seed=seed, moves=moves, num_repeats_in_model=c["reps"],
                           backend=backend, **kw)


def start(c):
    x0 = problem(c)[2]
    return x0 if c["T"] > 1 else x0[0]


def assert_state_equal(u, v, what):
    assert np.array_equal(u.branches["model_0"].coords, v.branches["model_0"].coords), f"{what}: positions of the last State differ"
    for f in ("log_like", "log_prior", "betas"):
        fu, fv = getattr(u, f), getattr(v, f)
        assert (fu is None and fv is None) or np.array_equal(fu, fv), f"{what}: {f} of the last State differs"
    assert u.random_state == v.random_state, f"{what}: random_state of the last State differs: {u.random_state} / {v.random_state}"


def assert_backends_equal(host, dev, what, tempered=True, nstore=None, steps=slice(None)):
    """``nstore``: the device backend stored the first nstore rungs only; ``steps``: the stored steps of the host chain to compare with"""
    r = slice(None, nstore)
    assert np.array_equal(host.get_chain()["model_0"][steps][:, r], dev.get_chain()["model_0"]), f"{what}: get_chain differs"
    assert np.array_equal(host.get_log_like()[steps][:, r], dev.get_log_like()), f"{what}: get_log_like differs"
    assert np.array_equal(host.get_log_prior()[steps][:, r], dev.get_log_prior()), f"{what}: get_log_prior differs"
    if tempered:
        assert np.array_equal(host.get_betas()[steps], dev.get_betas()), f"{what}: get_betas differs"


def assert_totals_equal(host, dev, what, nstore=None):
    assert np.array_equal(host.accepted[:nstore], dev.accepted), f"{what}: accepted differs"
    assert np.array_equal(host.swaps_accepted, dev.swaps_accepted), f"{what}: swaps_accepted differs"
    assert host.random_state == dev.random_state, f"{what}: backend.random_state differs: {host.random_state} / {dev.random_state}"
    assert host.iteration == dev.iteration


def run_case(name, thin):
    c = CASES[name]
    a, b = sampler(c, Backend()), sampler(c, DeviceBackend())
    ra = a.run_mcmc(start(c), NSTEPS, thin_by=thin)
    rb = b.run_mcmc(start(c), NSTEPS, thin_by=thin)
    what = f"{name}, thin_by={thin}"
    assert_backends_equal(a.backend, b.backend, what, tempered=c["T"] > 1)
    assert_totals_equal(a.backend, b.backend, what)
    assert_state_equal(ra, rb, what)
    assert a.backend.accepted.sum() > 0, f"{what}: nothing was accepted - the comparison says nothing"
    assert b.backend.downloads == 1, f"{what}: {b.backend.downloads} chain downloads for one segment"
    if c["T"] > 1:
        assert a.backend.swaps_accepted.sum() > 0 and not np.array_equal(a.get_betas()[0], a.get_betas()[-1])
        assert np.array_equal(a.temperature_control.betas, b.temperature_control.betas) and a.temperature_control.time == b.temperature_control.time
    for ma, mb in zip(a.moves, b.moves):          # the moves' own counters see every iteration, whoever stores the chain
        assert np.array_equal(ma.accepted, mb.accepted) and ma.num_proposals == mb.num_proposals


@pytest.mark.parametrize("thin", [1, 3])
@pytest.mark.parametrize("name", sorted(CASES))
def test_device_backend_equals_host_backend(name, thin, monkeypatch):
    for k, v in CASES[name]["env"].items():
        monkeypatch.setenv(k, v)
    run_case(name, thin)


def test_slot_ordered_records_under_no_col():
    """HENS_NO_COL=1 (read once per process: a child, as the switch tests of tests/test_hip_records.py): the two-launch iteration on
    records in SLOT order."""
    code = ("import sys; sys.path.insert(0, sys.argv[1])\nimport torch\nfrom tests import test_hip_chain_store as t\n"
            "t.run_case('two_col_T16', 1); t.run_case('two_col_T8', 3); print('chain ok')")
    r = subprocess.run([sys.executable, "-c", code, ROOT], env=dict(os.environ, HENS_NO_COL="1"), capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and "chain ok" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("nstore", [1, 3])
def test_ntemps_store_keeps_the_first_rungs(nstore):
    c = case(6, 64, 8)
    a, b = sampler(c, Backend()), sampler(c, DeviceBackend(ntemps_store=nstore))
    ra, rb = a.run_mcmc(start(c), NSTEPS, thin_by=2), b.run_mcmc(start(c), NSTEPS, thin_by=2)
    assert b.get_chain()["model_0"].shape == (NSTEPS, nstore, 64, 1, 8) and b.backend.accepted.shape == (nstore, 64)
    assert_backends_equal(a.backend, b.backend, f"ntemps_store={nstore}", nstore=nstore)
    assert_totals_equal(a.backend, b.backend, f"ntemps_store={nstore}", nstore=nstore)
    assert b.backend.swaps_accepted.shape == (5,)
    assert_state_equal(ra, rb, f"ntemps_store={nstore}")


def test_capacity_of_five_closes_two_segments():
    c = CASES["two_col_T8"]
    small = DeviceBackend(max_bytes=5 * DeviceBackend.bytes_per_step(c["T"], c["W"], c["D"]) + 7)
    a, b, h = sampler(c, DeviceBackend()), sampler(c, small), sampler(c, Backend())
    ra, rb, rh = a.run_mcmc(start(c), NSTEPS), b.run_mcmc(start(c), NSTEPS), h.run_mcmc(start(c), NSTEPS)
    assert small.capacity == 5 and a.backend.capacity == NSTEPS
    info = b.engine.chain_info()
    assert info["capacity"] == 5 and info["count"] == 2 and info["bytes"] >= 5 * info["step_bytes"]
    for ref, what in ((a.backend, "one segment of 12"), (h.backend, "host backend")):
        assert_backends_equal(ref, small, f"capacity 5 vs {what}")
        assert_totals_equal(ref, small, f"capacity 5 vs {what}")
    assert small.downloads == 3                     # two closures + the open segment, once
    assert np.array_equal(small.get_log_like(discard=3, thin=4), h.get_log_like(discard=3, thin=4))
    assert_state_equal(ra, rb, "capacity 5 vs one segment")
    assert_state_equal(rh, rb, "capacity 5 vs host backend")


def test_two_runs_append_and_a_new_sampler_resumes_from_a_stored_step():
    c = CASES["one_launch_D16"]
    whole = sampler(c, DeviceBackend())
    rw = whole.run_mcmc(start(c), NSTEPS, thin_by=2)
    twice = sampler(c, DeviceBackend())
    twice.run_mcmc(start(c), 6, thin_by=2)
    rt = twice.run_mcmc(None, 6, thin_by=2)
    assert_backends_equal(whole.backend, twice.backend, "run_mcmc(6) twice vs run_mcmc(12)")
    assert_totals_equal(whole.backend, twice.backend, "run_mcmc(6) twice vs run_mcmc(12)")
    assert_state_equal(rw, rt, "run_mcmc(6) twice vs run_mcmc(12)")
    # the stored State of step 6, rebuilt from the chain alone, in a new sampler: steps 7 - 12
    bk = whole.backend
    st6 = State({"model_0": bk.get_chain()["model_0"][5]}, log_like=bk.get_log_like()[5], log_prior=bk.get_log_prior()[5],
                betas=bk.get_betas()[5], random_state=bk.get_random_states()[5])
    assert st6.random_state == ("philox", 77, 6 * 2, st6.random_state[3])
    rest = sampler(c, DeviceBackend())
    rr = rest.run_mcmc(st6, 6, thin_by=2)
    assert_backends_equal(whole.backend, rest.backend, "resumed from stored step 6", steps=slice(6, None))
    assert_state_equal(rw, rr, "resumed from stored step 6")
    assert np.array_equal(twice.backend.accepted, whole.backend.accepted)


def test_burn_and_sample_by_hand():
    c = CASES["two_col_T16"]
    a, b = sampler(c, Backend()), sampler(c, DeviceBackend())
    ra, rb = a.run_mcmc(start(c), NSTEPS, burn=4, thin_by=3), b.run_mcmc(start(c), NSTEPS, burn=4, thin_by=3)
    assert_backends_equal(a.backend, b.backend, "burn=4")
    assert_totals_equal(a.backend, b.backend, "burn=4")
    assert_state_equal(ra, rb, "burn=4")
    # sample() iterated by hand: one yield per stored step, the State read lazily
    c = CASES["one_launch_D32"]
    a, b = sampler(c, DeviceBackend()), sampler(c, DeviceBackend())
    ra = a.run_mcmc(start(c), NSTEPS, thin_by=3)
    n, lazy0 = 0, b.engine.lazy_downloads
    for st in b.sample(start(c), iterations=NSTEPS, thin_by=3):
        n += 1
        assert st.random_state == b.backend.random_state and np.array_equal(st.betas, b.backend.last_step(("betas",))["betas"][0])
        if n == 5:
            assert np.array_equal(st.log_like, a.get_log_like()[4])           # (the yielded State is the stored step)
    assert n == NSTEPS and b.engine.lazy_downloads == lazy0 + 1                 # (nobody else looked: one state download)
    assert_backends_equal(a.backend, b.backend, "sample() by hand")
    assert_totals_equal(a.backend, b.backend, "sample() by hand")
    assert_state_equal(ra, State(st, copy=True), "sample() by hand")
    for ma, mb in zip(a.moves, b.moves):
        assert np.array_equal(ma.accepted, mb.accepted) and ma.num_proposals == mb.num_proposals


def test_what_the_device_backend_refuses():
    c = CASES["two_col_T8"]
    like, box, _ = problem(c)
    priors = {i: uniform_dist(-box, box) for i in range(c["D"])}
    with pytest.raises(NotImplementedError, match="philox"):
        EnsembleSampler(c["W"], c["D"], like, priors, tempering_kwargs=dict(ntemps=c["T"]), backend=DeviceBackend())
    s = sampler(c, DeviceBackend())
    with pytest.raises(NotImplementedError, match="tune"):
        s.run_mcmc(start(c), 2, tune=True)
    with pytest.raises(NotImplementedError, match="tune"):
        next(s.sample(start(c), iterations=2, tune=True))
    r = s.run_mcmc(start(c), 3, store=False)          # nothing stored: today's path, the chain stays empty
    assert s.backend.iteration == 0 and r.log_like.shape == (c["T"], c["W"])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def engine(c, seed=5, **kw):
    like, box, x0 = problem(c)
    tempered = c["T"] > 1
    eng = HipEnsemble(c["T"], c["W"], c["D"], like, -box, box, seed=seed, tempered=tempered, adaptation_lag=LAG, adaptation_time=NU, **kw)
    from eryn_amd.moves.tempering import make_ladder
    eng.upload(x0, betas=make_ladder(c["D"], ntemps=c["T"]) if tempered else None)
    eng.eval_state()
    return eng


def test_append_leaves_the_state_untouched_and_partial_downloads():
    for name, n, k in (("two_col_T16", 4, 3), ("one_launch_D32", 5, 2), ("padded_D11", 3, 1), ("long_T70", 2, 2)):
        c = CASES[name]
        a, b = engine(c), engine(c)
        a.chain_create(n + 2)
        a.step_chain(n, k, 1)
        steps = []
        for _ in range(n):                             # the twin: hens_step, a download per stored step
            b.step(k)
            steps.append(b.download() + (b.iteration(), b.counters()["adapt_time"]))
        for u, v, f in zip(a.download(), b.download(), ("x", "log_like", "log_prior", "betas")):
            assert np.array_equal(u, v), f"{name}: {f} after hens_step_chain differs from hens_step's"
        ca, cb = a.counters(), b.counters()
        assert all(np.array_equal(ca[f], cb[f]) for f in ca), f"{name}: counters differ"
        info = a.chain_info()
        assert (info["capacity"], info["count"], info["ntemps_store"]) == (n + 2, n, c["T"])
        assert info["step_bytes"] == DeviceBackend.bytes_per_step(c["T"], c["W"], c["D"]) and info["bytes"] >= (n + 2) * info["step_bytes"]
        full = a.chain_download()
        for i, (x, L, P, betas, it, tm) in enumerate(steps):
            assert np.array_equal(full["x"][i], x) and np.array_equal(full["log_like"][i], L) and np.array_equal(full["log_prior"][i], P)
            assert np.array_equal(full["betas"][i], betas) and full["iteration"][i] == it == (i + 1) * k and full["adapt_time"][i] == tm
        part = a.chain_download(1, n - 2)              # a range inside, every field
        for f in full:
            assert np.array_equal(part[f], full[f][1:n - 1]), f"{name}: partial download of {f}"
        only = a.chain_download(n - 1, 1, fields=("log_like",))        # null pointers for the rest
        assert set(only) == {"log_like", "iteration", "adapt_time"} and np.array_equal(only["log_like"][0], full["log_like"][-1])
        assert a.chain_download(n, 0)["x"].shape[0] == 0
        a.close(), b.close()


def test_error_codes():
    c = CASES["two_col_T8"]
    eng = engine(c)
    with pytest.raises(RuntimeError, match="no chain"):
        eng.step_chain(1)
    with pytest.raises(RuntimeError, match="no chain"):
        eng.chain_download()
    with pytest.raises(ValueError):
        eng.chain_create(0)
    with pytest.raises(ValueError):
        eng.chain_create(4, ntemps_store=c["T"] + 1)
    with pytest.raises(ValueError, match="int64"):
        eng.chain_create(2**62)
    step = DeviceBackend.bytes_per_step(c["T"], c["W"], c["D"])
    asked = eng.chain_info()["free_bytes"] * 4 // step              # four times the free memory: an allocation that cannot succeed
    with pytest.raises(RuntimeError, match=r"allocating \d+ bytes"):
        eng.chain_create(asked)
    assert eng.chain_info()["capacity"] == 0
    eng.chain_create(3)
    it0 = eng.iteration()
    with pytest.raises(RuntimeError, match="do not fit"):          # before anything is launched
        eng.step_chain(4, 2, 1)
    assert eng.iteration() == it0 and eng.chain_info()["count"] == 0
    for ips, n_last in ((2, 0), (1, 2), (0, 0)):
        with pytest.raises(ValueError):
            eng.step_chain(1, ips, n_last)
    with pytest.raises(ValueError):
        eng.step_chain(-1, 1, 1)
    eng.step_chain(2, 2, 1)
    for first, count in ((0, 3), (2, 1), (-1, 1), (3, 0), (1, -1)):
        with pytest.raises(ValueError, match="outside"):
            eng.chain_download(first, count)
    # other state changes: counters reset / upload / set_iteration leave the chain and its totals alone; reset zeroes the totals
    acc, swaps = eng.chain_totals()
    assert acc.sum() > 0 and swaps.sum() > 0
    eng.reset_counters()
    x, L, P, betas = eng.download()
    eng.upload(x, L, P, betas)
    eng.set_iteration(100)
    acc2, swaps2 = eng.chain_totals()
    assert np.array_equal(acc, acc2) and np.array_equal(swaps, swaps2) and eng.chain_info()["count"] == 2
    eng.step_chain(1, 1, 1)                                          # a resumed run appends
    assert list(eng.chain_download(fields=())["iteration"]) == [2, 4, 101]
    eng.chain_reset()
    acc, swaps = eng.chain_totals()
    info = eng.chain_info()
    assert not acc.any() and not swaps.any() and info["count"] == 0 and info["capacity"] == 3
    eng.chain_destroy()
    assert eng.chain_info()["capacity"] == 0
    eng.close()


def test_append_launches_are_timed_while_profiling_is_on():
    """hens_set_profiling 1: an event pair around every append launch of the call, read into n_store_timed / store_ms; off again:
    the next call's figures are zero (the leaf-packing family: tests/test_hip_rj_chain_store.py::test_protocol)."""
    eng = engine(CASES["two_col_T8"])
    eng.chain_create(4)
    eng.set_profiling(1)
    eng.step_chain(2, 2, 1)
    info = eng.chain_info()
    assert info["n_store_timed"] == 2 and info["store_ms"] > 0
    eng.set_profiling(0)
    eng.step_chain(1, 1, 1)
    assert eng.chain_info()["n_store_timed"] == 0
    eng.close()


def test_contexts_without_a_chain_store():
    from eryn_amd.likelihood import HostLikelihood
    from eryn_amd.rj import _TemplateLikelihood
    c = CASES["two_col_T8"]
    like, box, _ = problem(c)
    shard = HipEnsemble(c["T"], c["W"], c["D"], like, -box, box, rung_range=(0, 4))
    rank = HipEnsemble(c["T"], c["W"], c["D"], like, -box, box)
    rank.pipe_init(1, 0)
    host = HipEnsemble(2, 16, 4, HostLikelihood(lambda x: -0.5 * np.sum(x * x, axis=-1), 4), -5.0, 5.0)
    leaf = HipEnsemble(2, 16, 16, _TemplateLikelihood(16), -1.0, 1.0, tempered=True, live_dangerously=True)
    for eng, word in ((shard, "shard"), (rank, "pipeline"), (host, "device likelihood"), (leaf, "leaf-packing")):
        with pytest.raises(NotImplementedError, match=word):
            eng.chain_create(4)
        with pytest.raises(NotImplementedError, match=word):
            eng.step_chain(1)
        eng.close()


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if CASES[n]["path"]])
def test_launch_path_is_the_shapes_own(name, monkeypatch):
    """The launches a profiled call reports under hens_step_chain are the ones the shape has under hens_step, on the queue it has
    (hens_timing::clock 2: the dispatch timestamps of the context's AQL queue; 1: event pairs on the HIP stream)."""
    c = CASES[name]
    for k, v in c["env"].items():
        monkeypatch.setenv(k, v)
    kw = {"pad_rows": False} if c["env"] else {}
    a, b = engine(c, **kw), engine(c, **kw)
    if c["nsplits"] != 2:
        a.set_nsplits(c["nsplits"]), b.set_nsplits(c["nsplits"])
    a.chain_create(4)
    a.set_profiling(2), b.set_profiling(2)
    a.step_chain(2, 3, 2)
    b.step(4), b.step(2)
    ta, tb = a.timing(), b.timing()
    for f in ("n_stretch", "n_pt", "n_fused", "n_iters", "clock"):
        assert ta[f] == tb[f], f"{name}: {f} {ta[f]} under hens_step_chain, {tb[f]} under hens_step"
    want = {"one": (0, 0, 2), "two": (2, 0, 2), "copying": None}[c["path"]]
    if want:
        assert (ta["n_stretch"], ta["n_pt"], ta["n_fused"]) == want and ta["clock"] == 2, f"{name}: {ta}"
    else:
        assert ta["n_fused"] == 0 and ta["n_pt"] == 2 and ta["clock"] == 1, f"{name}: {ta}"
    for u, v in zip(a.download(), b.download()):
        assert np.array_equal(u, v)
    a.set_profiling(1)                                  # event pairs: the append launches are timed too
    a.step_chain(2, 1, 1)
    info = a.chain_info()
    assert info["n_store_timed"] == 2 and info["store_ms"] > 0.0
    a.close(), b.close()
