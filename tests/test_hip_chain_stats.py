"""GPU tests of the chain diagnostics (include/hipensemble.h: hens_chain_moments, hens_chain_act; csrc/hens_chain_stats.h:
k_chain_moments, k_chain_act; eryn_amd.backend: get_autocorr_time, get_gelman_rubin_convergence_diagnostic, get_evidence_estimate).

Two yardsticks.  eryn_amd/chain_stats.py on the same chain, downloaded afterwards: bit-exact equality, NaN with NaN.  And exact
arithmetic (tests/exact_chain_stats.py: long double on the same doubles): |device - exact| <= 1.0 B with the a-priori bound B derived
there.
"""
import numpy as np
import pytest

from eryn_amd import chain_stats
from eryn_amd._lib import check
from eryn_amd.backend import Backend, DeviceBackend
from eryn_amd.engine import HipEnsemble
from eryn_amd.ensemble import EnsembleSampler
from eryn_amd.likelihood import GaussianLikelihood
from eryn_amd.moves import StretchMove
from eryn_amd.moves.tempering import make_ladder
from eryn_amd.prior import uniform_dist
from tests import exact_chain_stats as ex

pytestmark = pytest.mark.gpu
BOX = 20.0
COUNTS = (1, 20, 40, 50, 51, 70)          # stored steps at which the chain is questioned (window 50: below, at, one past, past)
PINNED = 0.5                              # every walker starts with this last coordinate: the stretch move c + z (x - c) keeps it


def problem(T, W, D, pin=True):
    rs = np.random.RandomState(3)
    A = rs.randn(D, D)
    like = GaussianLikelihood(0.1 * rs.randn(D), np.linalg.inv(A @ A.T / D + np.eye(D)))
    x0 = np.random.RandomState(1).randn(T, W, D)
    if pin:
        x0[..., D - 1] = PINNED
    return like, x0


def sampler(T, W, D, backend, seed=77, **tk):
    like, _ = problem(T, W, D)
    priors = {i: uniform_dist(-BOX, BOX) for i in range(D)}
    return EnsembleSampler(W, D, like, priors, rng="philox", seed=seed, moves=StretchMove(), backend=backend,
                           tempering_kwargs=dict(ntemps=T, adaptation_lag=50, adaptation_time=10, **tk))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def assert_within(got, exact, bound, what):
    ok, err = ex.within(got, exact, bound)
    worst = np.max(np.where(np.isfinite(bound) & np.isfinite(err), err / np.maximum(bound, 1e-300), 0.0))
    print(f"{what}: worst |error| / B = {worst:.3g}")
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} entries past 1.0 B, worst |error| / B = {worst:.3g}"


def ranges(n):
    """(first, count, thin) of discard / thin = (0, 1), (5, 3) and a first whose last kept step is the chain's last"""
    out = [(0, n, 1)]
    if n > 5:
        out.append((5, len(range(5, n, 3)), 3))
    first = (n - 1) % 4
    out.append((first, len(range(first, n, 4)), 4))
    assert first + (out[-1][1] - 1) * 4 == n - 1
    return out


def check_chain(eng, chain, nts, fast_at=(), what=""):
    """Everything hens_chain_moments / hens_chain_act return for the chain as it stands, against the module and exact arithmetic."""
    x, L, P = chain["x"], chain["log_like"], chain["log_prior"]
    n = x.shape[0]
    n_const = 0
    for nt in nts:
        for first, count, thin in ranges(n):
            sel = slice(first, first + (count - 1) * thin + 1, thin)
            tag = f"{what} n={n} ntemps={nt} first={first} count={count} thin={thin}"
            for window, fast in [(50, False), (7, False)] + ([(50, True)] if n in fast_at and thin == 1 else []):
                K = chain_stats.lag_count(count, window, fast)
                got = eng.chain_act(first, count, thin, nt, K)
                want = chain_stats.act(x[sel, :nt], window, fast)
                for g, w, f in zip(got, want, ("tau", "mean", "c0")):
                    assert g.shape == (nt,) + x.shape[2:] and same(g, w), f"{tag} window={window} fast={fast}: {f} differs from chain_stats.act"
                et, em, ec, bt, bm, bc = ex.exact_act(x[sel, :nt], K)
                assert_within(got[0], et, bt, f"{tag} window={window} fast={fast} tau")
                assert_within(got[1], em, bm, f"{tag} mean")
                assert_within(got[2], ec, bc, f"{tag} c0")
                n_const += int(np.count_nonzero(np.ptp(x[sel, :nt], axis=0) == 0)) if count > 1 else 0
            for field, a in (("x", x), ("log_like", L), ("log_prior", P)):
                got = eng.chain_moments(field, first, count, thin, nt)
                want = chain_stats.moments(a[sel, :nt], mask=field != "x")
                for g, w, f in zip(got, want, ("sum", "m2", "n_finite")):
                    assert g.shape == w.shape and g.dtype == w.dtype and same(g, w), f"{tag}: {f} of {field} differs from chain_stats.moments"
                assert (got[2] == count).all()
                es, e2, _, bs, b2 = ex.exact_moments(a[sel, :nt], mask=field != "x")
                assert_within(got[0], es, bs, f"{tag} sum of {field}")
                assert_within(got[1], e2, b2, f"{tag} m2 of {field}")
    return n_const


# 4 x 64 x 8: even D, 16-byte lanes; 3 x 40 x 5: odd D, W D = 200 is no multiple of the wave (tail lanes); 16 x 40 x 8 storing 3
# rungs, asked for 1 and for 3; D = 11: rows padded to 16 on the device, 11 columns in the chain
SHAPES = {"even_D8": (4, 64, 8, None, (4,)), "odd_D5": (3, 40, 5, None, (3,)), "store3_of_16": (16, 40, 8, 3, (1, 3)), "padded_D11": (4, 64, 11, None, (4,))}


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_device_equals_the_module_bit_for_bit_and_exact_arithmetic_within_the_bound(name):
    T, W, D, nstore, nts = SHAPES[name]
    _, x0 = problem(T, W, D)
    n_const = 0
    for n in COUNTS:                          # a chain of its own per length: a second run_mcmc would open a new segment
        s = sampler(T, W, D, DeviceBackend(ntemps_store=nstore))
        s.run_mcmc(x0, n)
        chain = s.engine.chain_download()
        assert chain["x"].shape == (n, nstore or T, W, D) and s.backend._open == n
        n_const += check_chain(s.engine, chain, nts, fast_at=(40, 70), what=name)
        assert (s.backend.stats_launches, s.backend.downloads) == (0, 0)                      # (the engine was asked, not the backend)
        if n < COUNTS[-1]:
            s.engine.close()
    x = chain["x"]
    assert (x[..., D - 1] == PINNED).all() and n_const >= 1, "no constant series in the chain: the NaN case was not met"
    tau = s.engine.chain_act(0, 70, 1, nts[-1], 50)[0]
    assert np.isnan(tau[..., D - 1]).all() and np.isfinite(tau[..., :D - 1]).all()           # (sums of 0.5 are exact: c_0 = 0)
    assert np.count_nonzero(np.ptp(x[:, 0], axis=0) > 0) >= W * (D - 1) * 0.9, "the walkers hardly moved: the comparison says little"


def engine(T, W, D, lo, hi, seed=5):
    like, x0 = problem(T, W, D)
    eng = HipEnsemble(T, W, D, like, lo, hi, seed=seed, tempered=True, adaptation_lag=50, adaptation_time=10)
    return eng, x0


def test_non_finite_log_likelihoods_are_skipped_and_counted():
    """A state uploaded with -inf on chosen walkers, in a box so narrow that most proposals leave it and are refused: the -inf
    entries survive into the stored steps, and the device's finite mask meets them."""
    T, W, D = 4, 64, 8
    eng, _ = engine(T, W, D, -1.0, 1.0)
    rs = np.random.RandomState(8)
    x0 = rs.uniform(-0.999, 0.999, size=(T, W, D))
    eng.upload(x0, betas=make_ladder(D, ntemps=T))
    eng.eval_state()
    x, L, P, betas = eng.download()
    L = L.copy()
    L[:, ::2] = -np.inf
    eng.upload(x, L, P, betas)
    eng.chain_create(3)
    eng.step_chain(3, 1, 1)
    chain = eng.chain_download()
    bad = ~np.isfinite(chain["log_like"])
    assert bad.sum(axis=(0, 2)).max() >= 1, "no non-finite log-likelihood was stored: the mask was not met"
    assert (~bad).sum() > 0
    print("non-finite stored log-likelihoods per rung:", bad.sum(axis=(0, 2)))
    for field in ("log_like", "log_prior"):
        for first, count, thin in ((0, 3, 1), (0, 2, 2), (2, 1, 1)):
            sel = slice(first, first + (count - 1) * thin + 1, thin)
            got = eng.chain_moments(field, first, count, thin, T)
            want = chain_stats.moments(chain[field][sel], mask=True)
            for g, w, f in zip(got, want, ("sum", "m2", "n_finite")):
                assert same(g, w), f"{field} [{first}, {count}, {thin}]: {f} differs from chain_stats.moments"
    nf = eng.chain_moments("log_like", 0, 3, 1, T)[2]
    assert np.array_equal(nf, (~bad).sum(axis=0)) and nf.min() < 3
    eng.close()


def test_accessors_on_a_device_backend_equal_the_host_backends(capsys):
    T, W, D, n = 4, 64, 8, 40
    _, x0 = problem(T, W, D, pin=False)       # (no constant coordinate: its NaN tau makes get_autocorr_thin_burn raise, as the reference's)
    small = DeviceBackend(max_bytes=25 * DeviceBackend.bytes_per_step(T, W, D) + 5)
    runs = {k: sampler(T, W, D, b, stop_adaptation=8) for k, b in (("host", Backend()), ("device", DeviceBackend()), ("segments", small))}
    for s in runs.values():
        s.run_mcmc(x0, n)
    h, d, g = (runs[k].backend for k in ("host", "device", "segments"))
    assert g.iteration == n and g._open == n - 25 and d._open == n
    calls = [("get_autocorr_time", {}), ("get_autocorr_time", dict(discard=3, thin=2, all_temps=True, window=7, average=False)),
             ("get_autocorr_time", dict(discard=3, fast=True, multiply_thin=False)),
             ("get_gelman_rubin_convergence_diagnostic", dict(doprint=False)),
             ("get_gelman_rubin_convergence_diagnostic", dict(discard=4, thin=3, doprint=False, per_walker=True)),
             ("get_gelman_rubin_convergence_diagnostic", dict(discard=1, thin=2))]
    for name, kw in calls:
        want = getattr(h, name)(**kw)["model_0"]
        printed = capsys.readouterr().out
        for b, what in ((d, "device path"), (g, "host path over closed segments")):
            launches, downloads = b.stats_launches, b.downloads
            got = getattr(b, name)(**kw)["model_0"]
            assert capsys.readouterr().out == printed
            if isinstance(want, dict):
                assert list(got) == list(want) == list(range(T)) and all(same(got[t], want[t]) for t in want), f"{name}({kw}) on the {what}"
            else:
                assert same(got, want), f"{name}({kw}) on the {what}"
            if b is d:
                assert b.stats_launches > launches and b.downloads == downloads == 0, f"{name}({kw}): the device path downloaded the chain"
            else:                                # (closed segments among the kept steps: the host copy was read; the last third of a
                assert b.downloads >= 1          #  Gelman-Rubin split may lie in the open segment alone and run there)
                assert b.stats_launches - launches <= (1 if "gelman" in name else 0)
    assert "Gelman-Rubin" in printed
    assert d.get_autocorr_thin_burn() == h.get_autocorr_thin_burn() and np.isfinite(h.get_autocorr_time()["model_0"]).all()
    # the segmented backend's open segment alone: the device path there as well
    launches = g.stats_launches
    assert same(g.get_autocorr_time(discard=26)["model_0"], h.get_autocorr_time(discard=26)["model_0"]) and g.stats_launches == launches + 1
    # evidence: the ladder stands from iteration 8 on
    assert not np.array_equal(h.get_betas()[0], h.get_betas()[-1]) and np.array_equal(h.get_betas()[12], h.get_betas()[-1])
    want = h.get_evidence_estimate(discard=12, thin=2)
    assert np.isfinite(want).all()
    launches = d.stats_launches
    assert d.get_evidence_estimate(discard=12, thin=2) == want and d.stats_launches == launches + 1 and d.downloads == 0
    assert g.get_evidence_estimate(discard=12, thin=2) == want
    assert d.get_evidence_estimate(discard=12, thin=2, return_error=False, method="TI") == want[0]
    for b in (h, d, g):
        with pytest.raises(ValueError, match="betas are allowed to vary"):
            b.get_evidence_estimate()
        with pytest.raises(NotImplementedError, match="mixes rungs with walkers"):
            b.get_evidence_estimate(discard=12, method="stepping-stone")
    few = sampler(T, W, D, DeviceBackend(ntemps_store=2), stop_adaptation=8)
    few.run_mcmc(x0, 12)
    with pytest.raises(ValueError, match="every rung"):
        few.backend.get_evidence_estimate(discard=10)


def test_error_codes():
    T, W, D = 4, 64, 8
    eng, x0 = engine(T, W, D, -BOX, BOX)
    eng.upload(x0, betas=make_ladder(D, ntemps=T))
    eng.eval_state()
    for call in (lambda: eng.chain_moments("x", 0, 1, 1, 1), lambda: eng.chain_act(0, 1, 1, 1, 50)):
        with pytest.raises(RuntimeError, match="no chain"):
            call()
    eng.chain_create(80, ntemps_store=3)
    eng.step_chain(70, 1, 1)
    it0, ms0 = eng.iteration(), eng.chain_stats_ms()
    assert ms0 == dict(moments_ms=-1.0, act_ms=-1.0)
    bad = [dict(first=0, count=71), dict(first=-1, count=1), dict(first=70, count=1), dict(first=0, count=0), dict(first=0, count=-1),
           dict(first=0, count=36, thin=2), dict(first=0, count=1, thin=0), dict(first=0, count=1, thin=-2),
           dict(first=0, count=1, ntemps=0), dict(first=0, count=1, ntemps=4), dict(first=0, count=2, thin=2**62)]
    for kw in bad:
        with pytest.raises(ValueError):
            eng.chain_moments("x", **kw)
        with pytest.raises(ValueError):
            eng.chain_moments("log_like", **kw)
        with pytest.raises(ValueError):
            eng.chain_act(window=50, **kw)
    with pytest.raises(ValueError):
        eng.chain_act(0, 70, 1, 1, window=0)
    with pytest.raises(ValueError):
        check(eng.lib.hens_chain_moments(eng.ctx, 3, 0, 1, 1, 1, None, None, None), eng.ctx)
    assert eng.chain_stats_ms() == ms0, "a refused call launched something"
    with pytest.raises(NotImplementedError, match="64"):             # 65 lags do not fit the lane's accumulators / LDS ring
        eng.chain_act(0, 70, 1, 1, window=65)
    assert eng.chain_stats_ms() == ms0
    tau = eng.chain_act(0, 70, 1, 1, window=64)[0]                    # ... 64 do, and a window past a short range is the range's length
    assert tau.shape == (1, W, D) and same(eng.chain_act(0, 20, 1, 3, window=1000)[0], eng.chain_act(0, 20, 1, 3, window=20)[0])
    assert same(tau, chain_stats.act(eng.chain_download()["x"][:, :1], 64)[0])
    check(eng.lib.hens_chain_act(eng.ctx, 0, 70, 1, 1, 50, None, None, None), eng.ctx)          # every output may be null
    ms = eng.chain_stats_ms()
    assert ms["act_ms"] > 0 and ms["moments_ms"] == -1.0 and eng.iteration() == it0
    eng.close()
    # a leaf-packing context: not built
    from eryn_amd.rj import _TemplateLikelihood
    bare = HipEnsemble(2, 16, 16, _TemplateLikelihood(16), -1.0, 1.0, tempered=True, live_dangerously=True)
    for call in (lambda: bare.lib.hens_chain_act(bare.ctx, 0, 1, 1, 1, 50, None, None, None),
                 lambda: bare.lib.hens_chain_moments(bare.ctx, 0, 0, 1, 1, 1, None, None, None)):
        with pytest.raises(NotImplementedError, match="not built for a leaf-packing context"):
            check(call(), bare.ctx)
    bare.close()


def test_diagnostics_leave_the_run_untouched():
    """run, diagnostics, run: the chain continues bit for bit as if nobody had asked."""
    T, W, D = 4, 64, 8
    _, x0 = problem(T, W, D)
    a, b = sampler(T, W, D, DeviceBackend()), sampler(T, W, D, DeviceBackend())
    a.run_mcmc(x0, 10)
    b.run_mcmc(x0, 10)
    b.backend.get_autocorr_time(all_temps=True)
    b.backend.get_gelman_rubin_convergence_diagnostic(discard=1, doprint=False)
    b.backend.get_evidence_estimate(discard=9)
    assert b.backend.stats_launches >= 5 and b.backend.downloads == 0
    ra, rb = a.run_mcmc(None, 10, thin_by=2), b.run_mcmc(None, 10, thin_by=2)
    for f in ("get_chain", "get_log_like", "get_log_prior", "get_betas"):
        u, v = getattr(a.backend, f)(), getattr(b.backend, f)()
        assert np.array_equal(u["model_0"], v["model_0"]) if isinstance(u, dict) else np.array_equal(u, v), f
    assert np.array_equal(a.backend.accepted, b.backend.accepted) and np.array_equal(a.backend.swaps_accepted, b.backend.swaps_accepted)
    assert ra.random_state == rb.random_state and np.array_equal(ra.log_like, rb.log_like) and a.backend.random_state == b.backend.random_state
