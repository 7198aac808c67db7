"""CPU tests of the chain diagnostics' host side: eryn_amd/chain_stats.py against exact arithmetic (tests/exact_chain_stats.py) and
against the real reference's utilities, the accessors of ``Backend`` / ``DeviceBackend`` over host arrays, the C ABI's surface and the
launch arithmetic of csrc/hens_chain_host.h under a sanitizer build."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
import types

import numpy as np
import pytest

from eryn_amd import _build, _lib, chain_stats
from eryn_amd.backend import Backend, DeviceBackend
from eryn_amd.state import State
from tests import exact_chain_stats as ex

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "eryn")), reason="the reference tree exists in the build container only")
SIZES = (1, 2, 20, 50, 70, 257)
SCALES = np.array([1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3])           # coordinates spread over six decades


def assert_within(got, exact, bound, what):
    ok, err = ex.within(got, exact, bound)
    worst = np.max(np.where(np.isfinite(bound) & np.isfinite(err), err / np.maximum(bound, 1e-300), 0.0))
    print(f"{what}: worst |error| / B = {worst:.3g}")
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} entries past 1.0 B, worst |error| / B = {worst:.3g}"


# ---- against exact arithmetic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1e6], ids=["centred", "offset_1e6_sigma"])
@pytest.mark.parametrize("n", SIZES)
def test_module_is_within_the_bound_of_exact_arithmetic(n, offset):
    rs = np.random.RandomState(100 + n)
    x = ex.ar1(rs, n, (5, SCALES.size), scale=SCALES, offset=offset * SCALES)
    for window, fast in ((50, False), (7, False), (50, True)):
        K = chain_stats.lag_count(n, window, fast)
        tau, mean, c0 = chain_stats.act(x, window, fast)
        et, em, ec, bt, bm, bc = ex.exact_act(x, K)
        what = f"n={n} window={window} fast={fast} offset={offset:g}"
        assert_within(tau, et, bt, what + " tau")
        assert_within(mean, em, bm, what + " mean")
        assert_within(c0, ec, bc, what + " c0")
        if n >= 20 and offset == 0.0:
            assert np.isfinite(bt).all() and bt.max() < 1e-9, "the bound says nothing on a centred chain"
    s, m2, nf = chain_stats.moments(x)
    es, e2, enf, bs, b2 = ex.exact_moments(x)
    assert np.array_equal(nf, enf) and (nf == n).all()
    assert_within(s, es, bs, f"n={n} sum")
    assert_within(m2, e2, b2, f"n={n} m2")
    assert np.array_equal(m2, chain_stats.act(x, 1)[2]), "m2 and c_0 are the same sum"


def test_a_constant_series_has_nan_tau_and_zero_m2():
    x = ex.ar1(np.random.RandomState(1), 20, (3, 4))
    x[:, 1, 2] = 3.0                                  # (sums of 3.0 are exact: the mean is 3.0 and every centred value 0)
    tau, mean, c0 = chain_stats.act(x, 50)
    assert np.isnan(tau[1, 2]) and c0[1, 2] == 0.0 and mean[1, 2] == 3.0 and np.isnan(tau).sum() == 1
    et, em, ec, bt, bm, bc = ex.exact_act(x, 20)
    assert np.isnan(float(et[1, 2])) and np.isinf(bt[1, 2]) and np.isfinite(np.delete(bt.ravel(), 6)).all()
    assert_within(tau, et, bt, "constant series tau")
    assert chain_stats.moments(x)[1][1, 2] == 0.0
    assert chain_stats.act(x[:1], 50)[0].tolist() == np.ones((3, 4)).tolist()      # one sample: no lag beyond 0, tau = 1


def test_masked_moments_skip_and_count_non_finite_entries():
    rs = np.random.RandomState(2)
    L = -np.abs(ex.ar1(rs, 70, (4, 9), scale=30.0))
    L[3, 0, 0] = L[9, 0, 0] = -np.inf
    L[5, 1, 2] = np.nan
    L[0, 2, 3] = np.inf
    L[7, 3, 4] = L[8, 3, 4] = -1e300                  # finite: it stays in, as in the reference
    L[:, 3, 8] = -np.inf                              # nothing finite at all
    s, m2, nf = chain_stats.moments(L, mask=True)
    assert nf[0, 0] == 68 and nf[1, 2] == 69 and nf[2, 3] == 69 and nf[3, 4] == 70 and nf[3, 8] == 0 and nf.sum() == 70 * 36 - 4 - 70
    assert s[3, 8] == 0.0 and m2[3, 8] == 0.0 and s[3, 4] < -1.9e300 and np.isfinite(s).all()
    es, e2, enf, bs, b2 = ex.exact_moments(L, mask=True)
    assert np.array_equal(nf, enf)
    assert_within(s, es, bs, "masked sum")
    keep = np.ones((4, 9), dtype=bool)
    keep[3, 4] = False                                # (-1e300 squared overflows a double: m2 = inf there, as np.var gives)
    assert_within(m2[keep], e2[keep], b2[keep], "masked m2")
    assert np.isinf(m2[3, 4])
    with np.errstate(all="ignore"):
        want = np.nansum(np.where(np.isfinite(L), L, np.nan), axis=0)
    assert np.allclose(s[keep], want[keep], rtol=1e-12)
    assert np.array_equal(chain_stats.moments(L)[2], np.full((4, 9), 70))           # unmasked: every entry counts


def test_lag_count():
    assert [chain_stats.lag_count(n, 50) for n in SIZES] == [1, 2, 20, 50, 50, 50]
    assert [chain_stats.lag_count(n, 50, fast=True) for n in (1, 2, 3, 40, 63, 64, 70)] == [1, 2, 2, 32, 32, 50, 50]
    assert chain_stats.lag_count(70, 7) == 7
    for bad in ((0, 50), (10, 0)):
        with pytest.raises(ValueError):
            chain_stats.lag_count(*bad)


# ---- against the real reference -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_utility():
    for m in ("corner", "seaborn"):            # imported unconditionally by eryn/utils/plot.py
        sys.modules.setdefault(m, types.ModuleType(m))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        import eryn.utils.utility as ut
    finally:
        sys.dont_write_bytecode = old
    return ut


@needs_reference
@pytest.mark.parametrize("average", [True, False])
@pytest.mark.parametrize("fast", [True, False])
@pytest.mark.parametrize("window", [50, 7])
def test_integrated_act_is_the_references(ref_utility, window, fast, average):
    """Chain lengths at which the reference's fast=True transform (length 512 / 128 / 64 over 300 / 70 / 40 samples) does not wrap
    below lag 212 / 58 / 24: under the window the circular and the linear sums are the same sums (chain_stats' docstring).  Window 50
    is not run on 40 samples: every lag of a centred series enters there, tau is 0 identically and both forms return rounding noise."""
    rs = np.random.RandomState(5)
    for n in (300, 70) if window == 50 else (300, 40):
        x = {"a": ex.ar1(rs, n, (2, 6, 1, 3), scale=np.array([1.0, 0.01, 100.0]), offset=np.array([0.0, 0.1, -1000.0])),
             "b": ex.ar1(rs, n, (2, 6, 1, 4), phi=0.5, offset=3.0)}       # (one leaf: the reference splits by ndim alone)
        want = ref_utility.get_integrated_act(x, window=window, fast=fast, average=average)
        got = chain_stats.get_integrated_act(x, window=window, fast=fast, average=average)
        assert list(got) == list(want)
        for k in want:
            assert got[k].shape == want[k].shape == ((2, x[k].shape[3] * x[k].shape[4]) if average else (2, 6, x[k].shape[3] * x[k].shape[4]))
            assert np.allclose(got[k], want[k], rtol=1e-9, atol=0), (k, n, np.max(np.abs(got[k] / want[k] - 1)))
        one = x["a"][:, 0, 0, 0, 0]
        assert np.isclose(chain_stats.get_integrated_act(one, window=window, fast=fast), ref_utility.get_integrated_act(one, window=window, fast=fast), rtol=1e-9)


class _RefBackendShim:
    """The reference accessor's own lines around get_integrated_act (backends/backend.py:653-662), without its ntemps > 1 refusal."""

    @staticmethod
    def autocorr(ut, chain, discard, thin, all_temps, multiply_thin, **kw):
        ind = next(iter(chain.values())).shape[1] if all_temps else 1
        x = {name: v[discard::thin][:, :ind] for name, v in chain.items()}
        out = ut.get_integrated_act(x, **kw)
        return {name: values * (thin if multiply_thin else 1) for name, values in out.items()}


def filled_backend(n, T=3, W=8, D=3, seed=11, betas=None, L=None):
    rs = np.random.RandomState(seed)
    x = ex.ar1(rs, n, (T, W, 1, D), scale=np.array([1.0, 0.1, 10.0])[:D], offset=np.array([0.0, 1.0, -50.0])[:D])
    L = -np.abs(ex.ar1(rs, n, (T, W), scale=5.0)) if L is None else L
    b = Backend()
    b.reset(W, {"model_0": D}, ntemps=T, branch_names=["model_0"])
    b.grow(n)
    for s in range(n):
        bt = (1.0 / (1.0 + np.arange(T))) if betas is None else betas[s]
        b.save_step(State({"model_0": x[s]}, log_like=L[s], log_prior=-np.ones((T, W)), betas=bt), np.zeros((T, W)))
    return b, x, L


@needs_reference
@pytest.mark.parametrize("discard,thin,multiply_thin,all_temps", [(0, 1, True, False), (10, 3, True, True), (7, 2, False, True)])
def test_backend_autocorr_time_is_the_references(ref_utility, discard, thin, multiply_thin, all_temps):
    b, x, _ = filled_backend(300)
    for window, average in ((50, True), (7, False)):
        got = b.get_autocorr_time(discard=discard, thin=thin, all_temps=all_temps, multiply_thin=multiply_thin, window=window, average=average)
        want = _RefBackendShim.autocorr(ref_utility, {"model_0": x}, discard, thin, all_temps, multiply_thin, window=window, average=average)
        assert got["model_0"].shape == want["model_0"].shape == ((3 if all_temps else 1,) + (() if average else (8,)) + (3,))
        assert np.allclose(got["model_0"], want["model_0"], rtol=1e-9, atol=0)


@needs_reference
@pytest.mark.parametrize("per_walker", [False, True])
@pytest.mark.parametrize("W,S", [(6, 50), (8, 50), (7, 31), (3, 20), (5, 1000)])
def test_psrf_is_the_references(ref_utility, per_walker, W, S):
    """W S divisible by 3 (6 x 50: two whole walkers at each end) and not (8 x 50: 133 rows = 2 walkers + 33 steps; 7 x 31; 3 x 20: a
    third is less than a walker)."""
    rs = np.random.RandomState(W * S)
    C_ = ex.ar1(rs, S, (W, 4), scale=np.array([1.0, 0.05, 20.0, 1.0]), offset=np.array([0.0, 0.5, -100.0, 10.0])).transpose(1, 0, 2).copy()
    C_[:, :, 3] += np.linspace(0, 30, W)[:, None]                      # walkers that disagree: Rhat well above 1
    want = ref_utility.psrf(C_, 4, per_walker=per_walker)
    got = chain_stats.psrf(C_, 4, per_walker=per_walker)
    assert got.shape == want.shape == (4,) and np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
    assert got[3] > 1.05


@needs_reference
@pytest.mark.parametrize("T", [2, 5, 8])
@pytest.mark.parametrize("last", [0.0, 0.01])
def test_thermodynamic_integration_is_the_references(ref_utility, T, last):
    if not hasattr(np, "trapz"):
        pytest.skip("the reference's np.trapz left NumPy")
    rs = np.random.RandomState(T)
    betas = np.geomspace(1.0, 0.01, T)
    betas[-1] = last
    logls = -np.sort(np.abs(rs.randn(T)) * 20)
    perm = rs.permutation(T)                                          # an unsorted ladder: both sort it
    want = ref_utility.thermodynamic_integration_log_evidence(betas[perm], logls[perm])
    got = chain_stats.thermodynamic_integration_log_evidence(betas[perm], logls[perm])
    assert np.allclose(got, want, rtol=1e-9, atol=0), (got, want)
    with pytest.raises(ValueError):
        chain_stats.thermodynamic_integration_log_evidence(betas, logls[:-1])


# ---- the accessors ------------------------------------------------------------------------------------------------------------
def test_host_backend_accessors_are_the_modules(capsys):
    b, x, L = filled_backend(60)
    xs = x[:, :, :, 0, :]
    tau = b.get_autocorr_time()
    want = np.average(chain_stats.act(xs[:, :1], 50)[0], axis=1)
    assert list(tau) == ["model_0"] and np.array_equal(tau["model_0"], want) and want.shape == (1, 3)
    got = b.get_autocorr_time(discard=5, thin=3, all_temps=True, window=7, fast=True, average=False)["model_0"]
    assert np.array_equal(got, 3 * chain_stats.act(xs[5::3], 7, fast=True)[0]) and got.shape == (3, 8, 3)
    assert np.array_equal(b.get_autocorr_time(discard=5, thin=3, multiply_thin=False)["model_0"], np.average(chain_stats.act(xs[5::3, :1], 50)[0], axis=1))
    # thin / burn: backends/backend.py:365-384
    assert b.get_autocorr_thin_burn() == (int(2 * want.max()), int(0.5 * want.min()))
    # Gelman-Rubin: per rung, the module's psrf on [W, S, D]
    for per_walker in (False, True):
        for discard, thin in ((0, 1), (4, 3)):
            R = b.get_gelman_rubin_convergence_diagnostic(discard=discard, thin=thin, doprint=False, per_walker=per_walker)
            assert list(R) == ["model_0"] and list(R["model_0"]) == [0, 1, 2]
            for t in range(3):
                assert np.array_equal(R["model_0"][t], chain_stats.psrf(xs[discard::thin, t].transpose(1, 0, 2), 3, per_walker=per_walker))
    assert capsys.readouterr().out == ""
    b.get_gelman_rubin_convergence_diagnostic()
    out = capsys.readouterr().out
    assert "Gelman-Rubin diagnostic" in out and " Model: model_0" in out and out.count("\t") == 4
    # evidence
    s, _, nf = chain_stats.moments(L[10::2], mask=True)
    want = chain_stats.thermodynamic_integration_log_evidence(1.0 / (1.0 + np.arange(3)), chain_stats.rung_means(s, nf))
    assert b.get_evidence_estimate(discard=10, thin=2) == want
    for alias in ("therodynamic", "thermodynamic integration", "Thermo", "TI"):
        assert b.get_evidence_estimate(discard=10, thin=2, return_error=False, method=alias) == want[0]
    with np.errstate(all="ignore"):
        mean = np.nanmean(np.where(np.isfinite(L[10::2]), L[10::2], np.nan), axis=(0, 2))
    assert np.allclose(chain_stats.rung_means(s, nf), mean, rtol=1e-12)


def test_error_contracts_of_the_accessors():
    n = 12
    betas = np.tile(1.0 / (1.0 + np.arange(3)), (n, 1))
    betas[:4, 1] *= 1.0 + 0.01 * np.arange(4)[::-1] + 0.01          # the ladder adapts over the first four steps, then stands
    b, _, _ = filled_backend(n, betas=betas)
    with pytest.raises(ValueError, match="betas are allowed to vary"):
        b.get_evidence_estimate()
    assert np.isfinite(b.get_evidence_estimate(discard=4)).all()
    for alias in ("stepping stone", "ss", "step", "stone", "stepping-stone", "SS"):
        with pytest.raises(NotImplementedError, match="mixes rungs with walkers"):
            b.get_evidence_estimate(discard=4, method=alias)
    with pytest.raises(ValueError, match="thermodynamic"):
        b.get_evidence_estimate(discard=4, method="harmonic")
    for call in (b.get_autocorr_time, b.get_gelman_rubin_convergence_diagnostic, b.get_evidence_estimate):
        with pytest.raises(ValueError):
            call(discard=n)                                          # nothing kept
        with pytest.raises(ValueError):
            call(thin=0)
    with pytest.raises(ValueError):
        b.get_autocorr_time(window=0)


def test_device_backend_host_path_and_ntemps_store():
    """DeviceBackend over the fake engine of tests/test_chain_backend.py, which has no diagnostics kernels: a capacity of 5 closes
    segments, and kept steps that reach into them take the host path - the same bits as Backend."""
    from tests.test_chain_backend import FakeEngine, device_backend, host_backend, D, T, W
    eng = FakeEngine()
    d = device_backend(eng, max_bytes=5 * DeviceBackend.bytes_per_step(T, W, D))
    d.append(12, 1, 1)
    h = host_backend(12)
    assert d._open == 2 and d.stats_launches == 0
    for kw in (dict(), dict(discard=2, thin=3, all_temps=True, window=4, average=False)):
        assert np.array_equal(d.get_autocorr_time(**kw)["model_0"], h.get_autocorr_time(**kw)["model_0"], equal_nan=True)
    Rd, Rh = (b.get_gelman_rubin_convergence_diagnostic(discard=1, doprint=False)["model_0"] for b in (d, h))
    assert all(np.array_equal(Rd[t], Rh[t], equal_nan=True) for t in range(T)) and list(Rd) == list(range(T))
    assert d.stats_launches == 0 and d.downloads == 3
    with pytest.raises(ValueError, match="betas are allowed to vary"):
        d.get_evidence_estimate()
    with pytest.raises(AttributeError):                              # kept steps inside the open segment go to the engine
        d.get_autocorr_time(discard=10)
    few = device_backend(FakeEngine(), ntemps_store=2)
    few.append(6, 1, 1)
    with pytest.raises(ValueError, match="every rung"):
        few.get_evidence_estimate()


# ---- the C ABI's surface and the launch arithmetic ----------------------------------------------------------------------------
STAT_SYMBOLS = {"hens_chain_moments": 9, "hens_chain_act": 9, "hens_chain_stats_ms": 3}


def test_stat_symbols_are_declared_bound_and_exported():
    _build.build()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipensemble.h")).read(), flags=re.S)
    for name, nargs in STAT_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/hipensemble.h"
        assert len(m.group(1).split(",")) == nargs, f"{name}: the header declares {m.group(1)!r}"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs and hasattr(lib, name)
    for f in ("chain_stats.py", os.path.join("csrc", "hens_chain_stats.h")):
        assert "oracle" not in open(os.path.join(ROOT, "eryn_amd", f)).read(), f
    from tests.test_host_logic import test_fence_free_kernels_store_census_is_the_reviewed_one as census
    census()


def test_launch_arithmetic_under_a_sanitizer_build(tmp_path):
    """tools/chain_stats_host_check.cpp: a stand-alone program over csrc/hens_chain_host.h's diagnostics arithmetic, built with
    -fsanitize=address,undefined where the compiler has the runtimes (plainly otherwise) and run on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "chain_stats_host_check.cpp"), str(tmp_path / "chain_stats_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
