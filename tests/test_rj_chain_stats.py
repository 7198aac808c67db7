"""CPU tests of the diagnostics of reversible-jump chains' host side: eryn_amd/chain_stats.py (leaf_counts, leaf_moments, rj_psrf)
against the real reference's accessor and against exact arithmetic (tests/exact_chain_stats.py), the ordinal windows, the accessors of
``RJDeviceBackend`` over fake engines, the C ABI's surface and the launch arithmetic of csrc/hens_chain_host.h (rj_stat_plan) under a
sanitizer build."""
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
from eryn_amd.backend import RJDeviceBackend
from tests import exact_chain_stats as ex
from tests import test_rj_chain_backend as fake

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference/src"
needs_reference = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "eryn")), reason="the reference tree exists in the build container only")

# (S, W, nl, nd) -> (M, r): the smallest per-walker total and third_split(W, M)'s remainder
CHAINS = {(24, 10, 3, 3): (18, 6), (12, 33, 2, 4): (6, 0), (12, 10, 32, 1): (96, 32), (17, 7, 4, 2): (18, 6)}


def synthetic(S, W, nl, nd, offset=0.0, seed=None):
    """AR(1) coordinates [S, W, nl, nd] over six decades of scale and masks ((j + 3 w + 5 n) % (2 + w % 3)) != 0: per-walker totals
    spread 4 x, walker 0 empty over the first half of the steps, walker 1 always full; NaN on unused leaves, as the chain stores them."""
    rs = np.random.RandomState(S * W if seed is None else seed)
    scale = np.array([1.0, 0.05, 20.0, 1e-3])[:nd]
    x = ex.ar1(rs, S, (W, nl, nd), scale=scale, offset=offset * scale + np.array([0.0, 0.5, -100.0, 10.0])[:nd] * (offset == 0.0))
    j, w, n = np.meshgrid(np.arange(S), np.arange(W), np.arange(nl), indexing="ij")
    inds = ((j + 3 * w + 5 * n) % (2 + w % 3)) != 0
    inds[:S // 2, 0] = False
    inds[:, 1] = True
    x[~inds] = np.nan
    return x, inds


def compacted(x, inds):
    """Per walker the leaves in use in ascending (step, slot): a list of [total_w, nd] arrays (x, inds: [S, W, nl, nd] / [S, W, nl])."""
    S, W, nl, nd = x.shape
    return [x[:, w].reshape(S * nl, nd)[inds[:, w].reshape(S * nl)] for w in range(W)]


def assert_within(got, exact, bound, what):
    ok, err = ex.within(got, exact, bound)
    worst = np.max(np.where(np.isfinite(bound) & np.isfinite(err), err / np.maximum(bound, 1e-300), 0.0))
    print(f"{what}: worst |error| / B = {worst:.3g}")
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} entries past 1.0 B, worst |error| / B = {worst:.3g}"


# ---- against the real reference -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ref_backend():
    for m in ("corner", "seaborn"):            # imported unconditionally by eryn/utils/plot.py
        sys.modules.setdefault(m, types.ModuleType(m))
    if REF not in sys.path:
        sys.path.insert(0, REF)
    old = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        import eryn.backends.backend as rb
    finally:
        sys.dont_write_bytecode = old
    return rb


class _RefChain:
    """What the reference's accessor asks of its ``self`` (backends/backend.py:768-799): the real method runs over this."""

    def __init__(self, chain, inds, ndims):
        self.chain, self.inds, self.ndims = chain, inds, ndims
        self.branch_names = list(chain)
        first = chain[self.branch_names[0]]
        self.ntemps, self.nwalkers = first.shape[1], first.shape[2]

    def get_chain(self, discard=0, thin=1):
        return {k: v[discard::thin] for k, v in self.chain.items()}

    def get_inds(self, discard=0, thin=1):
        return {k: v[discard::thin] for k, v in self.inds.items()}


@needs_reference
@pytest.mark.parametrize("per_walker", [False, True])
@pytest.mark.parametrize("shape", sorted(CHAINS))
def test_rj_psrf_is_the_references_projection_and_psrf(ref_backend, shape, per_walker):
    S, W, nl, nd = shape
    x, inds = synthetic(*shape)
    totals = inds.sum(axis=(0, 2))
    M, r = CHAINS[shape]
    assert totals.min() == M and chain_stats.third_split(W, M)[2] == r and totals.max() >= 3.5 * totals.min()
    assert (inds.sum(axis=2) == 0).any() and (inds.sum(axis=2) == nl).any(), "steps with no leaf and with every leaf in use"
    ref = _RefChain({"m": x[:, None]}, {"m": inds[:, None]}, {"m": nd})
    want = ref_backend.Backend.get_gelman_rubin_convergence_diagnostic(ref, doprint=False, per_walker=per_walker)["m"][0]
    got = chain_stats.rj_psrf(x, inds, nd, per_walker=per_walker)
    worst = np.max(np.abs(got / want - 1))
    print(f"{shape} per_walker={per_walker}: worst relative distance to the reference {worst:.3g}")
    assert got.shape == want.shape == (nd,) and np.isfinite(want).all() and np.allclose(got, want, rtol=1e-9, atol=0), (got, want)


@needs_reference
@pytest.mark.parametrize("per_walker", [False, True])
def test_a_one_leaf_branch_enters_as_it_lies(ref_backend, per_walker):
    """nleaves_max = 1: no projection, NaN of an unused leaf goes into psrf (backends/backend.py:780-783) and comes out as NaN."""
    rs = np.random.RandomState(4)
    x = ex.ar1(rs, 30, (9, 1, 2), scale=np.array([1.0, 30.0]))
    inds = np.ones((30, 9, 1), dtype=bool)
    ref = _RefChain({"m": x[:, None]}, {"m": inds[:, None]}, {"m": 2})
    want = ref_backend.Backend.get_gelman_rubin_convergence_diagnostic(ref, doprint=False, per_walker=per_walker)["m"][0]
    got = chain_stats.rj_psrf(x, inds, 2, per_walker=per_walker)
    assert np.isfinite(want).all() and np.allclose(got, want, rtol=1e-9, atol=0)
    x[7, 2, 0, :] = np.nan
    inds[7, 2, 0] = False
    with np.errstate(all="ignore"):
        want = ref_backend.Backend.get_gelman_rubin_convergence_diagnostic(_RefChain({"m": x[:, None]}, {"m": inds[:, None]}, {"m": 2}), doprint=False,
                                                                           per_walker=per_walker)["m"][0]
    got = chain_stats.rj_psrf(x, inds, 2, per_walker=per_walker)
    assert np.isnan(want).all() and np.isnan(got).all()


@pytest.mark.parametrize("shape", sorted(CHAINS))
def test_leaf_counts_are_the_sums_and_bincounts(shape):
    S, W, nl, nd = shape
    inds = np.stack([synthetic(*shape, seed=t)[1] for t in range(2)], axis=1)          # [S, 2, W, nl]
    inds[:, 1] = inds[::-1, 1]
    nleaves, hist = chain_stats.leaf_counts(inds)
    assert nleaves.dtype == np.uint8 and hist.dtype == np.uint32 and nleaves.shape == (S, 2, W) and hist.shape == (2, W, nl + 1)
    assert np.array_equal(nleaves, inds.sum(-1))
    for t in range(2):
        for w in range(W):
            assert np.array_equal(hist[t, w], np.bincount(inds[:, t, w].sum(-1), minlength=nl + 1))
    assert np.array_equal(chain_stats.leaf_totals(hist), inds.sum(axis=(0, 3))) and chain_stats.leaf_totals(hist).dtype == np.int64
    assert (hist.sum(axis=-1) == S).all() and np.array_equal(hist.sum(axis=1), [np.bincount(nleaves[:, t].ravel(), minlength=nl + 1) for t in range(2)])


# ---- against exact arithmetic -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("offset", [0.0, 1e6], ids=["centred", "offset_1e6_sigma"])
@pytest.mark.parametrize("shape", sorted(CHAINS))
def test_leaf_moments_are_within_the_bound_of_exact_arithmetic(shape, offset):
    """The compacted series cut to the window, as an ordinary array [hi - lo, W, nd]: exact_moments' long double sums and its a-priori
    bounds, imported and not widened."""
    S, W, nl, nd = shape
    x, inds = synthetic(*shape, offset=offset)
    M, r = CHAINS[shape]
    series = compacted(x, inds)
    for lo, hi in [(0, M)] + ([(0, r), (M - r, M)] if r else [(1, M - 1)]):
        s, m2, n = chain_stats.leaf_moments(x[:, None], inds[:, None], lo, hi)
        assert s.shape == m2.shape == (1, W, nd) and n.shape == (1, W) and n.dtype == np.int64 and (n == hi - lo).all()
        cut = np.stack([c[lo:hi] for c in series], axis=1)                            # [hi - lo, W, nd]
        es, e2, _, bs, b2 = ex.exact_moments(cut)
        assert_within(s[0], es, bs, f"{shape} [{lo}, {hi}) offset={offset:g} sum")
        assert_within(m2[0], e2, b2, f"{shape} [{lo}, {hi}) offset={offset:g} m2")
        want = chain_stats.moments(cut)                                               # ... and the module's own order on the series
        assert np.array_equal(s[0], want[0]) and np.array_equal(m2[0], want[1])
        if offset == 0.0:
            assert np.isfinite(b2).all() and (b2 <= 1e-9 * np.maximum(np.asarray(e2, dtype=np.float64), 1e-300)).all(), "the bound says nothing"


# ---- ordinal windows ----------------------------------------------------------------------------------------------------------
def test_ordinal_windows_and_walkers_that_run_out():
    shape = (24, 10, 3, 3)
    x, inds = synthetic(*shape)
    totals = inds.sum(axis=(0, 2))
    series = compacted(x, inds)
    top = int(totals.max())
    assert totals.min() == 18 and top > 40
    # a window no walker can fill beyond its own total
    s, m2, n = chain_stats.leaf_moments(x[:, None], inds[:, None], 10, top)
    assert np.array_equal(n[0], totals - 10) and n.min() == 8 and n.max() == top - 10
    for w in range(10):
        want = chain_stats.moments(series[w][10:top])
        assert np.array_equal(s[0, w], want[0]) and np.array_equal(m2[0, w], want[1])
    # a window past a walker's last leaf: nothing enters, the sum stays 0, the mean is 0 / 0 and m2 stays 0
    s, m2, n = chain_stats.leaf_moments(x[:, None], inds[:, None], 30, 40)
    empty = totals <= 30
    assert empty.any() and not empty.all() and np.array_equal(n[0], np.clip(totals - 30, 0, 10))
    assert (s[0][empty] == 0.0).all() and (m2[0][empty] == 0.0).all() and np.isfinite(s).all() and np.isfinite(m2).all()
    # head and tail of the reference's split are windows of the same walk
    M, r = 18, 6
    head, tail = chain_stats.leaf_moments(x[:, None], inds[:, None], 0, r), chain_stats.leaf_moments(x[:, None], inds[:, None], M - r, M)
    for w in range(10):
        assert np.array_equal(head[0][0, w], chain_stats.moments(series[w][:r])[0]) and np.array_equal(tail[1][0, w], chain_stats.moments(series[w][M - r:M])[1])
    for lo, hi in ((0, 0), (3, 3), (4, 3), (-1, 3)):
        with pytest.raises(ValueError):
            chain_stats.leaf_moments(x[:, None], inds[:, None], lo, hi)


def test_too_few_leaves_raise_and_name_branch_and_rung():
    x, inds = synthetic(24, 10, 3, 3)
    inds[:, 4] = False
    inds[3, 4, 1] = True                                  # M = 1: floor(10 / 3) = 3 rows per third, but one walker's chain of one sample
    x[~inds] = np.nan
    assert chain_stats.rj_psrf(x, inds, 3).shape == (3,)
    with pytest.raises(ValueError, match=r"branch 'pulse', rung 2.*has 1 "):
        chain_stats.rj_psrf(x, inds, 3, per_walker=True, branch="pulse", rung=2)
    inds[3, 4, 1] = False                                 # M = 0: the reference's C[-0:] would be the whole array
    for per_walker in (False, True):
        with pytest.raises(ValueError, match="has 0 "):
            chain_stats.rj_psrf(x, inds, 3, per_walker=per_walker)
    few = np.zeros((5, 2, 2), dtype=bool)
    few[0, :, 0] = few[1, :, 1] = True                    # W = 2, M = 2: floor(4 / 3) = 1 < 2
    with pytest.raises(ValueError, match="thirds of 2 walkers"):
        chain_stats.rj_psrf(np.zeros((5, 2, 2, 1)), few, 1)
    assert chain_stats.rj_min_leaves(np.array([7, 3, 9])) == 3 and chain_stats.rj_min_leaves(np.array([7, 2, 9]), per_walker=True) == 2
    with pytest.raises(ValueError):
        chain_stats.rj_psrf(x, inds, 2)                   # x is not [S, W, nl, 2]


# ---- the accessors over fake engines ------------------------------------------------------------------------------------------
class StatsEngine(fake.FakeRJEngine):
    """The fake engine of tests/test_rj_chain_backend.py with RJEngine's diagnostics calls over its own arrays."""

    def _sel(self, key, first, count, thin, nt):
        assert 0 <= first and count >= 1 and first + (count - 1) * thin < len(self.seg), "kept steps outside the open segment"
        return np.array([self.seg[first + j * thin][key][:nt] for j in range(count)])

    def chain_leaves(self, branch, first, count, thin=1, ntemps=None, nleaves=True):
        nle, hist = chain_stats.leaf_counts(self._sel("inds/" + branch, first, count, thin, ntemps))
        return (nle if nleaves else None), hist

    def chain_leaf_moments(self, branch, first, count, thin, ntemps, lo, hi):
        return chain_stats.leaf_moments(self._sel("x/" + branch, first, count, thin, ntemps), self._sel("inds/" + branch, first, count, thin, ntemps), lo, hi)

    def chain_moments(self, field, first, count, thin=1, ntemps=None):
        key = field if field.startswith("log_") else "x/" + field
        return chain_stats.moments(self._sel(key, first, count, thin, ntemps), mask=field.startswith("log_"))


def host_answers(n, discard, thin, per_walker, nstore=fake.T):
    """The module over the whole run's arrays, rung by rung."""
    steps = [fake.state_of(s) for s in range(n)][discard::thin]
    out = {}
    for k in fake.NAMES:
        x, inds = (np.array([s[f"{f}/{k}"][:nstore] for s in steps]) for f in ("x", "inds"))
        out[k] = {t: chain_stats.rj_psrf(x[:, t], inds[:, t], fake.ND[k], per_walker) for t in range(nstore)}
    return out


def same_rhat(got, want, nstore=fake.T):
    return list(got) == fake.NAMES and all(list(got[k]) == list(range(nstore)) and
                                           all(np.array_equal(got[k][t], want[k][t], equal_nan=True) for t in range(nstore)) for k in got)


def test_accessors_take_the_host_path_over_closed_segments(capsys):
    eng = fake.FakeRJEngine()                              # (no diagnostics calls: a device path would be an AttributeError)
    d = fake.backend(eng, max_bytes=5 * fake.STEP)
    d.append(12, 1)
    assert d._open == 2 and d.downloads == 2 and isinstance(d, RJDeviceBackend)
    for per_walker in (False, True):
        for discard, thin in ((0, 1), (1, 2), (4, 3)):
            got = d.get_gelman_rubin_convergence_diagnostic(discard=discard, thin=thin, doprint=False, per_walker=per_walker)
            assert same_rhat(got, host_answers(12, discard, thin, per_walker)), (discard, thin, per_walker)
    assert capsys.readouterr().out == ""
    d.get_gelman_rubin_convergence_diagnostic(discard=1)
    out = capsys.readouterr().out
    assert "Gelman-Rubin diagnostic" in out and " Model: a" in out and " Model: b" in out and out.count("\t") == 2 * (1 + fake.T)
    inds = {k: np.array([fake.state_of(s)["inds/" + k] for s in range(12)]) for k in fake.NAMES}
    for discard, thin in ((0, 1), (3, 2)):
        counts, nle = d.get_nleaves_counts(discard, thin), d.get_nleaves(discard, thin, download=False)
        for k in fake.NAMES:
            sel = inds[k][discard::thin].sum(-1)
            assert counts[k].dtype == np.int64 and counts[k].shape == (fake.T, fake.NL[k] + 1)
            assert np.array_equal(counts[k], [np.bincount(sel[:, t].ravel(), minlength=fake.NL[k] + 1) for t in range(fake.T)])
            assert nle[k].dtype == np.int64 and np.array_equal(nle[k], sel) and np.array_equal(nle[k], d.get_nleaves(discard, thin)[k])
    assert d.stats_launches == 0 and d.downloads == 3 and eng.downloads == 3
    with pytest.raises(AttributeError):                    # kept steps inside the open segment go to the engine
        d.get_gelman_rubin_convergence_diagnostic(discard=10, doprint=False, per_walker=True)
    for call in (d.get_autocorr_time, d.get_autocorr_thin_burn):
        with pytest.raises(ValueError, match="not well-defined .* when using reversible jump"):
            call()
    with pytest.raises(ValueError, match="not well-defined"):
        d.get_autocorr_time(discard=2, thin=2, all_temps=True)
    with pytest.raises(ValueError, match="betas are allowed to vary"):      # (the fake's ladder moves at every step)
        d.get_evidence_estimate()
    for call in (d.get_gelman_rubin_convergence_diagnostic, d.get_evidence_estimate, d.get_nleaves_counts):
        with pytest.raises(ValueError):
            call(discard=12)
        with pytest.raises(ValueError):
            call(thin=0)
    assert d.get_nleaves(discard=12, download=False)["a"].shape == (0, fake.T, fake.W)
    few = fake.backend(fake.FakeRJEngine(), ntemps_store=2)
    few.append(6, 1)
    with pytest.raises(ValueError, match="every rung"):
        few.get_evidence_estimate()


def test_accessors_on_the_open_segment_count_launches_not_downloads(monkeypatch):
    eng = StatsEngine()
    d = fake.backend(eng, max_bytes=20 * fake.STEP, ntemps_store=2)
    d.append(12, 1)
    assert d._open == 12 and (d.stats_launches, d.downloads) == (0, 0)
    # per branch one chain_leaves launch; every rung of the fake has the same M, so one launch per window: [0, M), and head and tail
    # where third_split(W, M) leaves a remainder
    want = host_answers(12, 2, 2, False, nstore=2)
    got = d.get_gelman_rubin_convergence_diagnostic(discard=2, thin=2, doprint=False)
    assert same_rhat(got, want, nstore=2)
    r = {k: chain_stats.third_split(fake.W, int(np.array([fake.state_of(s)["inds/" + k][0] for s in range(2, 12, 2)]).sum(axis=(0, 2)).min()))[2] for k in fake.NAMES}
    assert d.stats_launches == sum(2 + (2 if r[k] else 0) for k in fake.NAMES) and d.downloads == 0 and eng.downloads == 0
    n0 = d.stats_launches
    assert same_rhat(d.get_gelman_rubin_convergence_diagnostic(doprint=False, per_walker=True), host_answers(12, 0, 1, True, nstore=2), nstore=2)
    assert d.stats_launches == n0 + 4 and d.downloads == 0
    counts, nle = d.get_nleaves_counts(discard=1), d.get_nleaves(discard=1, thin=3, download=False)
    assert d.stats_launches == n0 + 8 and d.downloads == 0
    assert all(counts[k].sum() == 11 * 2 * fake.W for k in fake.NAMES) and nle["b"].shape == (4, 2, fake.W)
    assert np.array_equal(nle["a"], d.get_nleaves(discard=1, thin=3)["a"]) and d.downloads == 1        # (the default path reads the chain)
    # rungs whose smallest totals differ: one set of launches per distinct M, over the rungs up to the last one that has it
    calls = []
    real = StatsEngine.chain_leaf_moments
    monkeypatch.setattr(StatsEngine, "chain_leaf_moments", lambda self, *a: (calls.append(a), real(self, *a))[1])
    for st in eng.seg[:6]:
        st["inds/a"][1, 2] = False                         # rung 1, walker 2 of branch a: no leaf over the first six steps
        st["x/a"][1, 2] = np.nan
    d._cache = None
    got = d.get_gelman_rubin_convergence_diagnostic(doprint=False, per_walker=True)["a"]
    inds = np.array([s["inds/a"] for s in eng.seg])
    M = [int(inds[:, t].sum(axis=(0, 2)).min()) for t in range(2)]
    assert M[1] < M[0] and [c[1:] for c in calls if c[0] == "a"] == [(0, 12, 1, 2, 0, M[1]), (0, 12, 1, 1, 0, M[0])]
    x = np.array([s["x/a"] for s in eng.seg])
    assert all(np.array_equal(got[t], chain_stats.rj_psrf(x[:, t], inds[:, t], 3, True)) for t in range(2))
    # the evidence: every rung stored and a ladder that stands
    full = fake.backend(StatsEngine(), max_bytes=20 * fake.STEP)
    full.append(6, 1)
    with pytest.raises(ValueError, match="betas are allowed to vary"):
        full.get_evidence_estimate()
    for st in full.engine.seg:
        st["betas"] = np.array([1.0, 0.5, 0.25])
    L = np.array([s["log_like"] for s in full.engine.seg])
    s, _, nf = chain_stats.moments(L[1:], mask=True)
    want = chain_stats.thermodynamic_integration_log_evidence([1.0, 0.5, 0.25], chain_stats.rung_means(s, nf))
    n0 = full.stats_launches
    assert full.get_evidence_estimate(discard=1) == want and full.stats_launches == n0 + 1 and full.downloads == 0
    with pytest.raises(NotImplementedError, match="mixes rungs with walkers"):
        full.get_evidence_estimate(method="ss")


# ---- the C ABI's surface and the launch arithmetic ----------------------------------------------------------------------------
RJ_STAT_SYMBOLS = {"hens_rj_chain_leaves": 8, "hens_rj_chain_leaf_moments": 11, "hens_rj_chain_moments": 10, "hens_rj_chain_stats_ms": 3}


def test_rj_stat_symbols_are_declared_bound_and_exported():
    _build.build()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipensemble.h")).read(), flags=re.S)
    for name, nargs in RJ_STAT_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/hipensemble.h"
        assert len(m.group(1).split(",")) == nargs, f"{name}: the header declares {m.group(1)!r}"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs and hasattr(lib, name)
    assert _lib.SIGNATURES["hens_rj_chain_leaf_moments"][1][6:8] == [C.c_int64, C.c_int64]             # lo, hi
    for f in ("chain_stats.py", os.path.join("csrc", "hens_rj_chain_stats.h")):
        assert "oracle" not in open(os.path.join(ROOT, "eryn_amd", f)).read(), f


def test_rj_launch_arithmetic_under_a_sanitizer_build(tmp_path):
    """tools/rj_chain_stats_host_check.cpp: a stand-alone program over csrc/hens_chain_host.h's rj_stat_plan, built with
    -fsanitize=address,undefined where the compiler has the runtimes (plainly otherwise) and run on the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "rj_chain_stats_host_check.cpp"), str(tmp_path / "rj_chain_stats_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    if r.returncode != 0:
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
