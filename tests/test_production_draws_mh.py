"""The Gaussian / MH move's production draws, pinned to tests/production_draws.py.

CPU: the edges of the Box-Muller map, the structure of the (rung, walker, pair) -> Philox address map, the distribution
of the specification's own normal stream (normal_stream_stats), and the power of those bars: four mutated
specifications - the bugs the map invites - each miss them.
GPU (-m gpu): ``hens_debug_draws`` exports the specification's move choice and accept uniforms bit for bit and its
normals to MH_NORMAL_E; the proposal scales, a ladder shard and the device stream's distribution; and the in-place
MODE_MH launch moves the walkers by exactly the exported steps.
"""
import math

import numpy as np
import pytest

from tests import production_draws as pd
from tests.test_production_draws import EDGES

SEED = 0x1234567890ABCDEF
# (device row width, iterations) of the distribution checks: about 2e6 normals per row-width class at T = 2, W = 200
STREAMS = [(128, 40), (64, 80), (32, 160), (8, 600)]
STREAM_T, STREAM_W = 2, 200


# ---- CPU: mh_normal_ideal at its edges ---------------------------------------------------------------------------------
def test_ideal_normal_edges():
    top = 2 ** 32 - 1
    r_max = math.sqrt(64.0 * math.log(2.0))
    assert abs(r_max - 6.6604) < 1e-4
    close = lambda v, want: abs(v - want) <= 4e-16 * abs(want)            # (log, sqrt, cos of float64: an ulp or two)
    x, y = pd.mh_normal_ideal(0, 0)                                       # smallest uniform: the largest radius; angle 0
    assert close(x, r_max) and y == 0.0
    x, y = pd.mh_normal_ideal(top, 12345)                                 # u1 = 1: radius exactly 0
    assert x == 0.0 and y == 0.0
    a = 0x40000000                                                        # any radius: u1 = 0.25 + 2^-32 -> float32 0.25
    r = math.sqrt(-2.0 * math.log(0.25))
    x, y = pd.mh_normal_ideal(a, 0)
    assert close(x, r) and y == 0.0
    x, y = pd.mh_normal_ideal(a, 1 << 30)                                 # a quarter turn
    assert abs(x) < 1e-15 and close(y, r)
    x, y = pd.mh_normal_ideal(a, 1 << 31)                                 # half a turn
    assert close(x, -r) and abs(y) < 1e-15
    x, y = pd.mh_normal_ideal(a, top)                                     # float32(2^32 - 1) = 2^32: ang = 1.0, a full turn
    assert np.float32(top) * np.float32(2.0 ** -32) == np.float32(1.0)
    assert close(x, r) and abs(y) < 1e-15
    aa, bb = np.meshgrid(np.array([0, 1, 255, 1 << 24, (1 << 24) + 1, 1 << 31, top - 256, top - 1, top], dtype=np.uint32),
                         np.array([0, 1, 1 << 29, 1 << 30, 3 << 30, 1 << 31, top - 128, top], dtype=np.uint32))
    x, y = pd.mh_normal_ideal(aa, bb)
    assert np.isfinite(x).all() and np.isfinite(y).all()
    assert np.all(np.hypot(x, y) <= r_max * (1 + 1e-15))


# ---- CPU: structure of the address map ------------------------------------------------------------------------------------
@pytest.mark.parametrize("W", [100, 200])
@pytest.mark.parametrize("RW", [128, 64, 32, 16, 8, 11])
def test_normal_addresses_are_injective(W, RW):
    """No two (rung, walker, pair) read the same half of the same call - within a rung and across the rung boundary."""
    g = pd.mh_pair_rows(RW)
    assert g == {128: 8, 64: 16, 32: 32, 16: 32}.get(RW, 0)
    seen = set()
    for rung in range(3):
        c2, c3, half = pd.mh_normal_address(rung, W, RW)
        assert c2.shape == c3.shape == half.shape == (W, (RW + 1) // 2)
        assert np.all((c2 >= rung * W) & (c2 < (rung + 1) * W))           # a rung's calls stay inside its own counter range
        keys = set(zip(c2.ravel().tolist(), c3.ravel().tolist(), half.ravel().tolist()))
        assert len(keys) == c2.size and not (keys & seen)
        seen |= keys
    c2, _, half = pd.mh_normal_address(1, W, RW)
    w = np.arange(W)
    if g:                                                                 # partners g apart share a call, one half each
        assert np.array_equal(half[:, 0], (w & g) // g)
        assert np.array_equal(c2[:, 0], W + np.where(w & g, w - g, w))
    else:
        assert not half.any() and np.array_equal(c2[:, 0], W + w)
    if W == 100 and g == 32:                                              # walkers 96..99 have bit 32 set: partners 64..67
        assert np.array_equal(c2[96:100, 0], W + np.arange(64, 68)) and half[96:100].all()
    if W == 200 and g == 8:                                               # walkers 192..199: bit 8 clear, partner beyond W
        assert np.array_equal(c2[192:200, 0], W + np.arange(192, 200)) and not half[192:200].any()


@pytest.mark.parametrize("RW", [128, 16, 8])
def test_normal_words_depend_on_both_iteration_words(RW):
    it = 5
    a0, b0 = pd.mh_normal_words(SEED, it, 1, 100, RW)
    for other in (it + 1, it + (1 << 32)):
        a1, b1 = pd.mh_normal_words(SEED, other, 1, 100, RW)
        assert np.mean(a0 == a1) < 1e-3 and np.mean(b0 == b1) < 1e-3
        assert not np.array_equal(pd.mh_uniform(SEED, it, 1, 100), pd.mh_uniform(SEED, other, 1, 100))
    assert pd.move_uniform(SEED, it) != pd.move_uniform(SEED, it + 1) != pd.move_uniform(SEED, it + (1 << 32))


@pytest.mark.parametrize("RW", [64, 11])
def test_a_shard_draws_the_rows_of_the_full_ladder(RW):
    full = pd.mh_steps(SEED, 7, 4, 100, RW, "iso", 1.0)
    part = pd.mh_steps(SEED, 7, 2, 100, RW, "iso", 1.0, rung_begin=1)
    for k in ("z", "mh_step", "mh_u"):
        assert np.array_equal(part[k], full[k][1:3])
    assert not np.array_equal(full["z"][0], full["z"][1])


def test_move_choice():
    its = range(2000)
    assert not any(pd.is_mh(SEED, it, 0.0) for it in its) and all(pd.is_mh(SEED, it, 1.0) for it in its)
    n = sum(pd.is_mh(SEED, it, 0.3) for it in its)
    assert abs(n - 600) < 5 * math.sqrt(2000 * 0.3 * 0.7)
    assert all(pd.is_mh(SEED, it, 0.3) == (pd.move_uniform(SEED, it) < 0.3) for it in its)


def test_the_bar_on_the_normals_is_four_times_the_measurement():
    assert pd.MH_NORMAL_E <= 1e-4
    assert pd.MH_NORMAL_OBSERVED is not None and pd.MH_NORMAL_E == 4.0 * pd.MH_NORMAL_OBSERVED


# ---- CPU: the specification's own stream, and the power of the bars ------------------------------------------------------
def _stream(RW, n_it, words=pd.mh_normal_words, ideal=pd.mh_normal_ideal):
    """z [n_it, T, W, RW] of iterations 0 .. n_it - 1 from a words function and a Box-Muller function."""
    z = np.empty((n_it, STREAM_T, STREAM_W, RW))
    for it in range(n_it):
        for t in range(STREAM_T):
            z[it, t, :, 0::2], z[it, t, :, 1::2] = ideal(*words(SEED, it, t, STREAM_W, RW))
    return z


@pytest.mark.parametrize("RW,n_it", STREAMS)
def test_specification_stream_is_standard_normal(RW, n_it):
    s = pd.normal_stream_stats(_stream(RW, n_it), pd.mh_pair_rows(RW))
    print(RW, s)
    assert s["n"] == n_it * STREAM_T * STREAM_W * RW
    assert pd.normal_stream_violations(s) == []


def _philox_words(seed, it, c2, c3, second):
    d = pd.philox4x32_10(it & 0xFFFFFFFF, it >> 32, c2, c3, seed & 0xFFFFFFFF, seed >> 32)
    return np.where(second, d[2], d[0]), np.where(second, d[3], d[1])


def _grid(W, RW):
    return np.arange(W)[:, None], np.arange(RW // 2)[None, :]


def _words_both_take_the_first_half(seed, it, rung, W, RW):
    w, pr = _grid(W, RW)
    return _philox_words(seed, it, rung * W + (w & ~pd.mh_pair_rows(RW)), 12 | (pr << 8), False)


def _words_key_without_pair(seed, it, rung, W, RW):
    w, pr = _grid(W, RW)
    g = pd.mh_pair_rows(RW)
    return _philox_words(seed, it, rung * W + (w & ~g), 12 + 0 * pr, (w & g) != 0)


def _words_without_iteration(seed, it, rung, W, RW):
    return pd.mh_normal_words(seed, 0, rung, W, RW)


def _ideal_in_radians(a, b):
    two_m32 = np.float32(2.0 ** -32)
    u1 = ((np.asarray(a).astype(np.float32) + np.float32(1.0)) * two_m32).astype(np.float64)
    ang = (np.asarray(b).astype(np.float32) * two_m32).astype(np.float64)
    r = np.sqrt(-2.0 * np.log(u1))
    return r * np.cos(ang), r * np.sin(ang)


@pytest.mark.parametrize("name,kw,must_miss", [
    ("both walkers of a quad read words 0, 1", dict(words=_words_both_take_the_first_half), "equal_fraction"),
    ("the key drops the pair index", dict(words=_words_key_without_pair), "z_adjacent"),
    ("the angle is taken as radians", dict(ideal=_ideal_in_radians), "z_sign_x"),
    ("the counter drops the iteration", dict(words=_words_without_iteration), "z_iterations")],
    ids=["same_half", "no_pair_key", "radians", "no_iteration"])
def test_the_bars_catch_a_mutated_specification(name, kw, must_miss):
    RW, n_it = STREAMS[0]
    s = pd.normal_stream_stats(_stream(RW, n_it, **kw), pd.mh_pair_rows(RW))
    bad = pd.normal_stream_violations(s)
    print(name, bad, s)
    assert must_miss in bad
    if must_miss == "equal_fraction":
        assert s["equal_fraction"] == 1.0
    if name.endswith("radians"):
        assert any(k in bad for k in ("z_mean", "z_var", "z_m3", "z_m4"))


# ---- GPU -------------------------------------------------------------------------------------------------------------------
def _engine(T, W, D, like="gauss", seed=SEED, **kw):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, RosenbrockLikelihood
    from oracle import eryn_oracle as orc
    lk =GaussianLikelihood(np.zeros(D), np.ones(D)) if like == "gauss" else RosenbrockLikelihood(D)
    eng = HipEnsemble(T, W, D, lk, -50.0, 50.0, seed=seed, live_dangerously=True, **kw)      # (W < 2 D among the cases)
    eng.upload(np.random.RandomState(0).uniform(-1.0, 1.0, (eng.Tl, W, D)), betas=orc.make_ladder(D, ntemps=T))
    eng.eval_state()
    return eng


# (D, likelihood, device row width): every row-width class, padded rows, rows nobody shares a call on, an odd unpadded row
CLASSES = [(128, "gauss", 128), (64, "gauss", 64), (32, "gauss", 32), (16, "gauss", 16), (11, "gauss", 16), (70, "gauss", 128),
           (8, "gauss", 8), (5, "gauss", 8), (11, "rosen", 11)]
worst_deviation = {}


@pytest.mark.gpu
@pytest.mark.parametrize("W", [100, 200])
@pytest.mark.parametrize("D,like,RW", CLASSES)
def test_device_mh_draws_equal_the_specification(D, like, RW, W):
    T = 2
    eng = _engine(T, W, D, like)
    assert eng.RW == RW
    eng.set_mh_proposal("iso", 1.0, 0.5)
    worst = 0.0
    for it in (0, 1) + EDGES:
        dev = eng.debug_draws(it, mh=True)
        spec = pd.mh_steps(SEED, it, T, W, RW, "iso", 1.0, weight=0.5)
        assert dev["is_mh"] == spec["is_mh"], f"is_mh at iteration {it}"
        assert np.array_equal(dev["mh_u"], spec["mh_u"]), f"mh_u at iteration {it}"
        assert dev["mh_step"].shape == (T, W, D)
        worst = max(worst, float(np.max(np.abs(dev["mh_step"] - spec["z"][..., :D]))))
    eng.close()
    worst_deviation[(D, like, W)] = worst
    print(f"D={D} {like} RW={RW} W={W}: max |mh_step - z_ideal| = {worst:.3e}; so far {max(worst_deviation.values()):.3e}"
          f" (bar {pd.MH_NORMAL_E:.3e})")
    assert worst <= pd.MH_NORMAL_E


@pytest.mark.gpu
def test_device_move_choice_equals_the_specification():
    eng = _engine(2, 100, 8)
    for weight in (0.0, 1.0, 0.3):
        eng.set_mh_proposal("iso", 1.0, weight)
        got = [eng.debug_draws(it)["is_mh"] for it in range(200)]
        assert got == [pd.is_mh(SEED, it, weight) for it in range(200)], f"weight {weight}"
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D,like", [(64, "gauss"), (16, "gauss"), (11, "gauss"), (8, "gauss"), (11, "rosen")])
def test_diagonal_proposal_scales_the_same_normals(D, like):
    eng = _engine(2, 100, D, like)
    it = 3
    eng.set_mh_proposal("iso", 1.0, 0.5)
    z_dev = eng.debug_draws(it, mh=True)["mh_step"]
    scale = np.random.RandomState(1).uniform(0.1, 3.0, D)
    eng.set_mh_proposal("diag", scale, 0.5)
    assert np.array_equal(eng.debug_draws(it, mh=True)["mh_step"], scale * z_dev)
    eng.set_mh_proposal("iso", 0.37, 0.5)
    assert np.array_equal(eng.debug_draws(it, mh=True)["mh_step"], 0.37 * z_dev)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("D", [16, 64])
def test_full_proposal_is_the_cholesky_product_of_the_same_normals(D):
    """k_mh_draw sums L[d, k] z[k] over k = 0 .. d with one FMA each: |fl - exact| <= gamma_n (|L| |z|)[d], n = d + 1 <= D."""
    eng = _engine(2, 100, D)
    it = 3
    eng.set_mh_proposal("iso", 1.0, 0.5)
    z_dev = eng.debug_draws(it, mh=True)["mh_step"]
    L = np.tril(np.random.RandomState(2).standard_normal((D, D)))
    eng.set_mh_proposal("full", L, 0.5)
    got = eng.debug_draws(it, mh=True)["mh_step"]
    eng.close()
    assert np.finfo(np.longdouble).nmant >= 63        # the reference product in 64-bit significands: its own error is 2^-11 of the bar
    ref = (z_dev.astype(np.longdouble) @ L.astype(np.longdouble).T)
    u = 2.0 ** -53
    gamma = D * u / (1.0 - D * u)
    bound = gamma * (np.abs(z_dev) @ np.abs(L).T)
    err = np.abs(got.astype(np.longdouble) - ref).astype(np.float64)
    print(f"D={D}: max err / bound = {np.max(err / bound):.3f}")
    assert np.all(err <= bound)
    assert np.array_equal(got[..., 0], L[0, 0] * z_dev[..., 0])


@pytest.mark.gpu
@pytest.mark.parametrize("D", [64, 11, 8])
def test_a_shard_exports_the_rows_of_the_full_ladder(D):
    T, W, it = 4, 100, 3
    full, part = _engine(T, W, D), _engine(T, W, D, rung_range=(1, 3))
    for e in (full, part):
        e.set_mh_proposal("iso", 1.0, 0.5)
    a, b = full.debug_draws(it, mh=True), part.debug_draws(it, mh=True)
    full.close()
    part.close()
    assert b["mh_step"].shape == (2, W, D) and b["is_mh"] == a["is_mh"]
    assert np.array_equal(b["mh_step"], a["mh_step"][1:3]) and np.array_equal(b["mh_u"], a["mh_u"][1:3])
    spec = pd.mh_steps(SEED, it, 2, W, part.RW, "iso", 1.0, rung_begin=1)
    assert np.array_equal(b["mh_u"], spec["mh_u"])
    assert np.max(np.abs(b["mh_step"] - spec["z"][..., :D])) <= pd.MH_NORMAL_E


@pytest.mark.gpu
@pytest.mark.parametrize("RW,n_it", STREAMS)
def test_device_stream_is_standard_normal(RW, n_it):
    eng = _engine(STREAM_T, STREAM_W, RW)
    eng.set_mh_proposal("iso", 1.0, 0.5)
    z = np.stack([eng.debug_draws(it, mh=True)["mh_step"] for it in range(n_it)])
    eng.close()
    s = pd.normal_stream_stats(z, pd.mh_pair_rows(RW))
    print(RW, s)
    assert s["n"] == n_it * STREAM_T * STREAM_W * RW
    assert pd.normal_stream_violations(s) == []


@pytest.mark.gpu
@pytest.mark.parametrize("D,pad", [(128, True), (64, True), (32, True), (16, True), (11, True), (8, True), (5, False)])
def test_the_launch_draws_what_the_export_says(D, pad):
    """From a point mass on a flat likelihood one accepted Gaussian proposal IS its step: the in-place MODE_MH launch (its own
    pairing of rows to Philox calls; D = 5 unpadded: k_mh_draw and the generic kernel) against the export."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    W = 200
    eng = HipEnsemble(1, W, D, GaussianLikelihood(np.zeros(D), 1e-12 * np.eye(D)), -1e6, 1e6, tempered=False, seed=SEED,
                      pad_rows=pad, live_dangerously=True)
    spec = pd.mh_steps(SEED, 0, 1, W, eng.RW, "iso", 1.0)
    zs = spec["z"][..., :D]
    accepted = np.log(spec["mh_u"]) < -0.5e-12 * np.sum(zs * zs, axis=-1)
    assert accepted.all() and spec["is_mh"]                    # (from the specification alone: nobody is predicted as rejected)
    eng.upload(np.zeros((1, W, D)))
    eng.eval_state()
    eng.set_mh_proposal("iso", 1.0, 1.0)
    step = eng.debug_draws(0, mh=True)["mh_step"]
    assert eng.iteration() == 0
    eng.step(1)
    x = eng.download()[0]
    eng.close()
    assert np.max(np.abs(step - zs)) <= pd.MH_NORMAL_E
    assert np.array_equal(x[accepted], step[accepted])
