"""CPU tests of the leaf-packing chain store's host side: RJDeviceBackend's segment bookkeeping, discard / thin, get_nleaves and the
three totals against a fake engine (the style of tests/test_chain_backend.py), and the C ABI's bindings."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from eryn_amd import _build, _lib
from eryn_amd.backend import DeviceBackend, RJDeviceBackend, _DeviceChain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, W, SEED = 3, 4, 9
NL, ND = {"a": 3, "b": 2}, {"a": 3, "b": 1}            # 9 + 2 = 11 coordinates, 5 leaf slots
NAMES = ["a", "b"]


def state_of(s):
    """Stored step s of the whole run: values that encode s, so a misplaced, repeated or stale step shows.  Leaf n of walker
    (t, w) of branch k is in use iff (t + w + n + s) % 3 != 0; unused leaves are NaN, as the device stores them."""
    out = {}
    for k in NAMES:
        x = np.arange(T * W * NL[k] * ND[k], dtype=np.float64).reshape(T, W, NL[k], ND[k]) + 1000.0 * s + (0.5 if k == "b" else 0.0)
        t, w, n = np.meshgrid(np.arange(T), np.arange(W), np.arange(NL[k]), indexing="ij")
        inds = (t + w + n + s) % 3 != 0
        x[~inds] = np.nan
        out["x/" + k], out["inds/" + k] = x, inds
    base = np.arange(T * W, dtype=np.float64).reshape(T, W)
    out.update(log_like=base - s, log_prior=base + 0.5 * s, betas=1.0 / (1.0 + np.arange(T) + s), iteration=10 * (s + 1), adapt_time=s // 2,
               acc=((base + s) % 3 == 0).astype(np.float64), bd=((base + s) % 4 == 0).astype(np.float64), swaps=np.arange(1, T, dtype=np.float64) + s)
    return out


class FakeRJEngine:
    """RJEngine's chain_* methods over NumPy arrays."""

    def __init__(self, free_bytes=1 << 20):
        self.free_bytes, self.capacity, self.step = free_bytes, 0, 0
        self.downloads = self.creates = self.resets = 0
        self.calls = []

    def chain_info(self):
        return dict(capacity=self.capacity, count=len(getattr(self, "seg", [])), ntemps_store=getattr(self, "Ts", 0), free_bytes=self.free_bytes)

    def _zero(self):
        self.seg, self.acc, self.bd, self.swaps = [], np.zeros((self.Ts, W)), np.zeros((self.Ts, W)), np.zeros(T - 1)

    def chain_create(self, capacity, ntemps_store=None):
        self.capacity, self.Ts = capacity, ntemps_store or T
        self._zero()
        self.creates += 1

    def chain_reset(self):
        self._zero()
        self.resets += 1

    def step_chain(self, n_store, iters_per_store=1):
        assert 0 < n_store <= self.capacity - len(self.seg), "append past the capacity"
        self.calls.append((n_store, iters_per_store))
        for _ in range(n_store):
            st = state_of(self.step)
            self.seg.append(st)
            self.acc += st["acc"][:self.Ts]
            self.bd += st["bd"][:self.Ts]
            self.swaps += st["swaps"]
            self.step += 1

    def chain_download(self, first=0, count=None, fields=("x", "inds", "log_like", "log_prior", "betas")):
        count = len(self.seg) - first if count is None else count
        assert 0 <= first and 0 <= count and first + count <= len(self.seg)
        if fields:
            self.downloads += 1
        rows = self.seg[first:first + count]

        def stack(key, cut=True):
            like = state_of(0)[key]
            like = like[:self.Ts] if cut else like
            return np.array([r[key][:self.Ts] if cut else r[key] for r in rows], dtype=like.dtype).reshape((count,) + like.shape)

        out = dict(iteration=np.array([r["iteration"] for r in rows], dtype=np.int64), adapt_time=np.array([r["adapt_time"] for r in rows], dtype=np.int64))
        for f in fields:
            out[f] = {k: stack(f"{f}/{k}") for k in NAMES} if f in ("x", "inds") else stack(f, cut=f != "betas")
        return out

    def chain_totals(self):
        return self.acc.copy(), self.bd.copy(), self.swaps.copy()


def backend(eng, **kw):
    b = RJDeviceBackend(**kw)
    b.attach(eng, SEED)
    b.reset(W, ND, ntemps=T, branch_names=NAMES, nleaves_max=NL)
    return b


STEP = RJDeviceBackend.bytes_per_step(T, W, 11, 5)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)])


def assert_reads_steps(d, n, nstore=T, what=""):
    want = [state_of(s) for s in range(n)]
    for discard, thin in ((0, 1), (0, 3), (2, 1), (3, 2), (5, 4), (100, 1)):
        sel = want[discard:n:thin]
        x, inds, nl = d.get_chain(discard, thin), d.get_inds(discard, thin), d.get_nleaves(discard, thin)
        for k in NAMES:
            shape = (len(sel), nstore, W, NL[k])
            assert same(x[k], np.array([s["x/" + k][:nstore] for s in sel]).reshape(shape + (ND[k],))), (what, k, discard, thin)
            assert inds[k].dtype == np.bool_ and np.array_equal(inds[k], np.array([s["inds/" + k][:nstore] for s in sel], dtype=bool).reshape(shape)), (what, k)
            assert nl[k].shape == shape[:3] and nl[k].dtype == np.int64 and np.array_equal(nl[k], inds[k].sum(axis=-1))
            assert np.array_equal(np.isnan(x[k]).all(axis=-1), ~inds[k])
        for f, get in (("log_like", d.get_log_like), ("log_prior", d.get_log_prior)):
            assert np.array_equal(get(discard, thin), np.array([s[f][:nstore] for s in sel]).reshape(len(sel), nstore, W)), (what, f, discard, thin)
        assert np.array_equal(d.get_betas(discard, thin), np.array([s["betas"] for s in sel]).reshape(len(sel), T))
        assert d.get_random_states(discard, thin) == [("philox", SEED, s["iteration"], s["adapt_time"]) for s in sel]
    assert np.array_equal(d.accepted, sum(s["acc"][:nstore] for s in want)) and np.array_equal(d.rj_accepted, sum(s["bd"][:nstore] for s in want)), what
    assert np.array_equal(d.swaps_accepted, sum(s["swaps"] for s in want)) and d.swaps_accepted.shape == (T - 1,), what
    assert d.random_state == ("philox", SEED, want[-1]["iteration"], want[-1]["adapt_time"]) and d.iteration == n, what


def test_bytes_per_step_is_the_c_abis():
    assert STEP == 8 * (T * W * (11 + 2) + T) + T * W * 5
    assert RJDeviceBackend.bytes_per_step(8, 2048, 60, 20) == 8 * (8 * 2048 * 62 + 8) + 8 * 2048 * 20        # config 4
    assert RJDeviceBackend.bytes_per_step(T, W, 11, 5, 1) == 8 * (W * 13 + T) + W * 5


@pytest.mark.parametrize("cap", [1, 3, 5, 8, 50])
def test_segments_close_and_read_in_order(cap):
    eng = FakeRJEngine()
    d = backend(eng, max_bytes=cap * STEP + 3)
    assert d.max_steps == cap
    d.grow(8)
    assert d.capacity == min(cap, 8) and eng.capacity == d.capacity
    d.append(8, 6)
    assert all(c[1] == 6 for c in eng.calls) and sum(c[0] for c in eng.calls) == 8
    assert len(eng.calls) == -(-8 // d.capacity)                    # one device call per segment
    assert eng.downloads == len(eng.calls) - 1                      # a closure is one download; nothing else was read yet
    assert_reads_steps(d, 8, what=f"capacity {cap}")
    assert eng.downloads == len(eng.calls) == d.downloads, "the accessors downloaded the open segment more than once"


def test_three_steps_of_room_in_a_run_of_eight():
    eng = FakeRJEngine()
    d = backend(eng, max_bytes=3 * STEP)
    d.grow(8)
    d.append(8, 1)
    assert [c[0] for c in eng.calls] == [3, 3, 2] and eng.resets == 2 and d.downloads == 2
    assert_reads_steps(d, 8)
    assert d.downloads == 3


def test_cache_append_and_reset():
    eng = FakeRJEngine()
    d = backend(eng, max_bytes=8 * STEP)
    assert d.get_chain()["a"].shape == (0, T, W, 3, 3) and d.get_inds()["b"].shape == (0, T, W, 2) and d.get_inds()["b"].dtype == np.bool_
    assert d.get_nleaves()["a"].shape == (0, T, W) and d.get_log_like().shape == (0, T, W) and d.get_betas().shape == (0, T)
    assert d.random_state is None and d.get_random_states() == [] and not d.accepted.any() and not d.rj_accepted.any() and not d.swaps_accepted.any()
    d.grow(8)
    d.append(3, 1)
    assert_reads_steps(d, 3)
    n = eng.downloads
    d.get_log_like(), d.get_chain(), d.get_nleaves(), d.accepted, d.rj_accepted
    assert eng.downloads == n == 1
    d.append(2, 1)                                  # same segment: the cache must go
    assert_reads_steps(d, 5)
    assert eng.downloads == 2
    d.grow(7)                                       # 3 steps of room left, 8 is the bound: nothing is remade
    assert eng.creates == 1
    d.append(7, 1)                                  # 3 fill the segment, it closes, 4 open the next
    assert eng.resets == 1 and d.iteration == 12
    assert_reads_steps(d, 12)
    # reset for another run of the same shape: the device buffers are kept, everything else starts again
    d.reset(W, ND, ntemps=T, branch_names=NAMES, nleaves_max=NL)
    assert eng.creates == 1 and eng.resets == 2 and d.iteration == 0 and d.capacity == 8 and not d.accepted.any() and d.random_state is None
    eng.step = 0
    d.append(2, 1)
    assert_reads_steps(d, 2)


def test_ntemps_store_and_the_default_budget():
    d = backend(FakeRJEngine(free_bytes=4 * 10 * STEP))
    assert d.max_steps == 10
    assert backend(FakeRJEngine(free_bytes=16)).max_steps == 1                  # never less than one step
    eng = FakeRJEngine()
    d = backend(eng, max_bytes=5 * RJDeviceBackend.bytes_per_step(T, W, 11, 5, 2), ntemps_store=2)
    assert d.max_steps == 5
    d.append(8, 2)
    assert eng.Ts == 2 and d.get_chain()["a"].shape == (8, 2, W, 3, 3) and d.rj_accepted.shape == (2, W)
    assert_reads_steps(d, 8, nstore=2)
    with pytest.raises(ValueError):
        backend(FakeRJEngine(), ntemps_store=T + 1)
    with pytest.raises(RuntimeError, match="attach"):
        RJDeviceBackend().reset(W, ND, ntemps=T, branch_names=NAMES, nleaves_max=NL)


def test_the_segment_bookkeeping_is_shared_not_copied():
    """DeviceBackend and RJDeviceBackend run the same grow / append / close / read code."""
    assert issubclass(DeviceBackend, _DeviceChain) and issubclass(RJDeviceBackend, _DeviceChain)
    for f in ("grow", "append", "_close_segment", "_open_segment", "_open_totals", "_field", "get_log_like", "get_log_prior", "get_betas",
              "get_random_states", "random_state"):
        assert f not in vars(DeviceBackend) and f not in vars(RJDeviceBackend) and f in vars(_DeviceChain), f


def test_sampler_refuses_a_backend_it_cannot_fill():
    from eryn_amd.rj import RJEnsembleSampler
    for kw in (dict(rng="numpy"), dict(rng="philox", log_like_fn=lambda x: 0.0), dict(rng="philox", backend=object())):
        with pytest.raises(NotImplementedError):              # (before anything touches a device)
            RJEnsembleSampler(8, {"a": 3}, kw.pop("log_like_fn", None), {}, backend=kw.pop("backend", RJDeviceBackend()), **kw)


# ---- the C ABI's surface ------------------------------------------------------------------------------------------------------
RJ_CHAIN_SYMBOLS = {
    "hens_rj_chain_create": ["hens_ctx*", "int64_t", "int32_t"], "hens_rj_chain_reset": ["hens_ctx*"], "hens_rj_chain_destroy": ["hens_ctx*"],
    "hens_rj_chain_info": ["hens_ctx*", "hens_chain_info_t*"], "hens_rj_step_chain": ["hens_ctx*", "int64_t", "int64_t"],
    "hens_rj_chain_download": ["hens_ctx*", "int64_t", "int64_t", "int32_t", "double*", "uint8_t*", "double*", "double*", "double*", "int64_t*", "int64_t*"],
    "hens_rj_chain_totals": ["hens_ctx*", "double*", "double*", "double*"]}
CTYPE = {"int64_t": C.c_int64, "int32_t": C.c_int32}


def test_rj_chain_symbols_are_declared_bound_and_exported():
    _build.build()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipensemble.h")).read(), flags=re.S)
    for name, want in RJ_CHAIN_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/hipensemble.h"
        declared = [re.sub(r"\s*\w+$", "", a.strip()).replace(" ", "") for a in m.group(1).split(",")]       # (the types, names dropped)
        assert declared == want, f"{name}: the header declares {declared}"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == len(want), f"{name}: _lib binds {len(args)} arguments"
        for i, (ty, bound) in enumerate(zip(want, args)):
            if ty in CTYPE:
                assert bound is CTYPE[ty], f"{name}: argument {i} is {ty}, bound as {bound}"
            elif ty == "hens_chain_info_t*":
                assert bound is C.POINTER(_lib.HensChainInfo), f"{name}: argument {i}"
            else:
                assert bound is C.c_void_p, f"{name}: argument {i} is a pointer, bound as {bound}"
        assert hasattr(lib, name)


def test_chain_code_never_mentions_the_oracle():
    for f in ("backend.py", "rj.py", "_lib.py", os.path.join("csrc", "hens_rj_chain.h"), os.path.join("csrc", "hens_chain_host.h")):
        assert "oracle" not in open(os.path.join(ROOT, "eryn_amd", f)).read(), f
