"""CPU tests of the chain store's host side: DeviceBackend's segment bookkeeping against a fake engine, the C ABI's bindings."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from eryn_amd import _build, _lib
from eryn_amd.backend import Backend, DeviceBackend
from eryn_amd.state import State

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, W, D, SEED = 3, 4, 2, 9


class FakeEngine:
    """The six chain_* methods of HipEnsemble over NumPy arrays: stored step s of the whole run holds values that encode s, so a
    misplaced, repeated or stale step shows."""

    def __init__(self, free_bytes=1 << 20):
        self.T, self.W, self.D = T, W, D
        self.free_bytes, self.capacity, self.step = free_bytes, 0, 0
        self.downloads = self.creates = self.resets = 0
        self.calls = []

    @staticmethod
    def state_of(s):
        """(x[T, W, D], L[T, W], P[T, W], betas[T], accepted[T, W], swaps[T - 1], iteration, time) of stored step s"""
        base = np.arange(T * W * D, dtype=np.float64).reshape(T, W, D)
        acc = ((np.arange(T * W).reshape(T, W) + s) % 3 == 0).astype(np.float64)
        return (base + 1000.0 * s, base[..., 0] - s, base[..., 1] + 0.5 * s, 1.0 / (1.0 + np.arange(T) + s), acc,
                np.arange(1, T, dtype=np.float64) + s, 10 * (s + 1), s // 2)

    def chain_info(self):
        return dict(capacity=self.capacity, count=len(getattr(self, "seg", [])), ntemps_store=getattr(self, "Ts", 0),
                    free_bytes=self.free_bytes, step_bytes=DeviceBackend.bytes_per_step(T, W, D, getattr(self, "Ts", None)))

    def chain_create(self, capacity, ntemps_store=None):
        self.capacity, self.Ts, self.seg = capacity, ntemps_store or T, []
        self.acc, self.swaps = np.zeros((self.Ts, W)), np.zeros(T - 1)
        self.creates += 1

    def chain_reset(self):
        self.seg, self.acc, self.swaps = [], np.zeros((self.Ts, W)), np.zeros(T - 1)
        self.resets += 1

    def step_chain(self, n_store, iters_per_store=1, n_last=1):
        assert 0 < n_store <= self.capacity - len(self.seg), "append past the capacity"
        self.calls.append((n_store, iters_per_store, n_last))
        for _ in range(n_store):
            st = self.state_of(self.step)
            self.seg.append(st)
            self.acc += st[4][:self.Ts]
            self.swaps += st[5]
            self.step += 1

    def chain_download(self, first=0, count=None, fields=("x", "log_like", "log_prior", "betas")):
        count = len(self.seg) - first if count is None else count
        assert 0 <= first and 0 <= count and first + count <= len(self.seg)
        if fields:
            self.downloads += 1
        rows = self.seg[first:first + count]
        col = dict(x=0, log_like=1, log_prior=2, betas=3)
        out = {f: np.array([r[col[f]][:self.Ts] if f != "betas" else r[3] for r in rows]).reshape(
            (count,) + (self.state_of(0)[col[f]][:self.Ts] if f != "betas" else self.state_of(0)[3]).shape) for f in fields}
        out["iteration"] = np.array([r[6] for r in rows], dtype=np.int64)
        out["adapt_time"] = np.array([r[7] for r in rows], dtype=np.int64)
        return out

    def chain_totals(self):
        return self.acc.copy(), self.swaps.copy()


def host_backend(n):
    b = Backend()
    b.reset(W, {"model_0": D}, ntemps=T, branch_names=["model_0"])
    b.grow(n)
    for s in range(n):
        x, L, P, betas, acc, swaps, it, tm = FakeEngine.state_of(s)
        b.save_step(State({"model_0": x[:, :, None, :]}, log_like=L, log_prior=P, betas=betas, random_state=("philox", SEED, it, tm)),
                    acc, swaps_accepted=swaps)
    return b


def device_backend(eng, **kw):
    b = DeviceBackend(**kw)
    b.attach(eng, SEED)
    b.reset(W, {"model_0": D}, ntemps=T, branch_names=["model_0"])
    return b


def assert_same(h, d, nstore=None, what=""):
    for discard, thin in ((0, 1), (0, 3), (2, 1), (3, 2), (5, 4), (100, 1)):
        assert np.array_equal(h.get_chain(discard, thin)["model_0"][:, :nstore], d.get_chain(discard, thin)["model_0"]), (what, discard, thin)
        assert np.array_equal(h.get_log_like(discard, thin)[:, :nstore], d.get_log_like(discard, thin)), (what, discard, thin)
        assert np.array_equal(h.get_log_prior(discard, thin)[:, :nstore], d.get_log_prior(discard, thin)), (what, discard, thin)
        assert np.array_equal(h.get_betas(discard, thin), d.get_betas(discard, thin)), (what, discard, thin)
    assert np.array_equal(h.accepted[:nstore], d.accepted) and np.array_equal(h.swaps_accepted, d.swaps_accepted), what
    assert h.random_state == d.random_state and h.iteration == d.iteration, what


@pytest.mark.parametrize("cap", [1, 4, 5, 12, 50])
def test_segments_close_and_read_like_the_host_backend(cap):
    eng = FakeEngine()
    d = device_backend(eng, max_bytes=cap * DeviceBackend.bytes_per_step(T, W, D) + 3)
    assert d.max_steps == cap
    d.grow(12)
    assert d.capacity == min(cap, 12) and eng.capacity == d.capacity
    d.append(12, 6, 2)
    assert all(c[1:] == (6, 2) for c in eng.calls) and sum(c[0] for c in eng.calls) == 12
    assert len(eng.calls) == -(-12 // d.capacity)                   # one device call per segment
    assert eng.downloads == len(eng.calls) - 1                      # a closure is one download; nothing else was read yet
    assert_same(host_backend(12), d, what=f"capacity {cap}")
    assert eng.downloads == len(eng.calls), "the accessors downloaded the open segment more than once"
    assert d.get_random_states()[7] == ("philox", SEED, 80, 3) and len(d.get_random_states(discard=2, thin=5)) == 2


def test_cache_is_dropped_by_an_append_and_kept_between_reads():
    eng = FakeEngine()
    d = device_backend(eng, max_bytes=8 * DeviceBackend.bytes_per_step(T, W, D))
    assert d.get_chain()["model_0"].shape == (0, T, W, 1, D) and d.random_state is None and not d.accepted.any()
    d.grow(8)
    d.append(3, 1, 1)
    assert_same(host_backend(3), d)
    n = eng.downloads
    d.get_log_like(), d.get_chain(), d.accepted
    assert eng.downloads == n == 1
    d.append(2, 1, 1)                               # same segment: the cache must go
    assert_same(host_backend(5), d)
    assert eng.downloads == 2
    d.grow(7)                                       # 3 steps of room left, 8 is the bound: nothing is remade
    assert eng.creates == 1
    d.append(7, 1, 1)                               # 3 fill the segment, it closes, 4 open the next
    assert eng.resets == 1 and d.iteration == 12
    assert_same(host_backend(12), d)
    assert d.downloads == eng.downloads


def test_a_second_run_may_get_a_larger_segment():
    eng = FakeEngine()
    d = device_backend(eng, max_bytes=20 * DeviceBackend.bytes_per_step(T, W, D))
    d.grow(6)
    d.append(6, 1, 1)
    assert d.capacity == 6
    d.grow(9)                                       # no room left and the budget allows more: closed and remade at 9
    assert d.capacity == 9 and eng.creates == 2
    d.append(9, 1, 1)
    assert_same(host_backend(15), d)


def test_capacity_defaults_to_a_quarter_of_the_free_memory_and_ntemps_store():
    step = DeviceBackend.bytes_per_step(T, W, D)
    assert step == 8 * (T * W * (D + 2) + T) and DeviceBackend.bytes_per_step(T, W, D, 1) == 8 * (W * (D + 2) + T)
    d = device_backend(FakeEngine(free_bytes=4 * 10 * step))
    assert d.max_steps == 10
    assert device_backend(FakeEngine(free_bytes=16)).max_steps == 1             # never less than one step
    eng = FakeEngine()
    d = device_backend(eng, max_bytes=5 * DeviceBackend.bytes_per_step(T, W, D, 2), ntemps_store=2)
    assert d.max_steps == 5
    d.append(12, 1, 1)
    assert eng.Ts == 2 and d.get_chain()["model_0"].shape == (12, 2, W, 1, D) and d.swaps_accepted.shape == (T - 1,)
    assert_same(host_backend(12), d, nstore=2)
    with pytest.raises(ValueError):
        device_backend(FakeEngine(), ntemps_store=T + 1)
    with pytest.raises(RuntimeError, match="attach"):
        DeviceBackend().reset(W, {"model_0": D}, ntemps=T, branch_names=["model_0"])


# ---- the C ABI's surface ------------------------------------------------------------------------------------------------------
CHAIN_SYMBOLS = {"hens_chain_create": 3, "hens_chain_reset": 1, "hens_chain_destroy": 1, "hens_chain_info": 2, "hens_step_chain": 4,
                 "hens_chain_download": 9, "hens_chain_totals": 3}


def test_chain_symbols_are_declared_bound_and_exported():
    _build.build()
    lib = _lib.load()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hipensemble.h")).read(), flags=re.S)
    for name, nargs in CHAIN_SYMBOLS.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", header)
        assert m, f"{name} is not declared in include/hipensemble.h"
        assert len(m.group(1).split(",")) == nargs, f"{name}: the header declares {m.group(1)!r}"
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and len(args) == nargs, f"{name}: _lib binds {len(args)} arguments"
        assert hasattr(lib, name)
    fields = re.search(r"typedef struct hens_chain_info_t \{(.*?)\} hens_chain_info_t;", header, flags=re.S).group(1)
    declared = re.findall(r"\b(int64_t|double)\s+(\w+)\s*;", fields)
    assert [n for _, n in declared] == [n for n, _ in _lib.HensChainInfo._fields_]
    assert all((t == "double") == (ct is C.c_double) for (t, _), (_, ct) in zip(declared, _lib.HensChainInfo._fields_))
    assert C.sizeof(_lib.HensChainInfo) == 8 * len(declared) == 64            # (hens.hip: static_assert on the same 64)


def test_chain_code_never_mentions_the_oracle_and_the_census_stands():
    for f in ("backend.py", "engine.py", "ensemble.py", "_lib.py", os.path.join("csrc", "hens_chain.h"), os.path.join("csrc", "hens_chain_host.h")):
        assert "oracle" not in open(os.path.join(ROOT, "eryn_amd", f)).read(), f
    from tests.test_host_logic import test_fence_free_kernels_store_census_is_the_reviewed_one as census
    census()


def test_capacity_and_launch_arithmetic_under_a_sanitizer_build(tmp_path):
    """tools/chain_host_check.cpp: a stand-alone program over csrc/hens_chain_host.h's capacity, range and append-launch arithmetic of
    both chain families, built with -fsanitize=address,undefined where the compiler has the runtimes (plainly otherwise) and run on
    the CPU."""
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    assert cxx, "no host C++ compiler"
    src, exe = os.path.join(ROOT, "tools", "chain_host_check.cpp"), str(tmp_path / "chain_host_check")
    base = [cxx, "-std=c++17", "-O1", "-g", src, "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True)
    build = "sanitizer build (address, undefined)"
    if r.returncode != 0:
        build = "plain build - the sanitizer build failed: " + (r.stderr.strip().splitlines() or ["no message"])[-1]
        r = subprocess.run(base, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    print("chain_host_check:", build)                # (pytest -rA shows which build ran)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
