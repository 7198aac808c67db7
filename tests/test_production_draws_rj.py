"""The NumPy specification of the leaf-packing stretch move's production draws (tests/production_draws_rj.py) has the structure
and the distributions the reference's draws have (red_blue.py:119-154, stretch.py:93-132, 205).  No GPU: the device is held to
this specification bit for bit in tests/test_hip_rj_stretch.py."""
import numpy as np
import pytest

from tests.production_draws_rj import stretch_draws

SEED = 0x1234_5678_9ABC


@pytest.mark.parametrize("W", [25, 26, 64, 144])
def test_split_is_balanced_and_complements_come_from_the_other_set(W):
    T, nb = 3, 2
    n0 = (W + 1) // 2
    differ = False
    for it in (0, 1, 63, 64):
        d = stretch_draws(SEED, it, T, W, nb)
        lab = d["labels"]
        assert set(np.unique(lab)) <= {0, 1}
        for k in range(2):                                    # set k holds ceil((W - k) / 2) walkers on every rung
            assert np.all((lab == k).sum(axis=1) == (W - k + 1) // 2)
        for h in range(2):
            Ns, Nc = ((n0, W - n0), (W - n0, n0))[h]
            assert d["rint"][h].shape == (nb, T, Ns) and d["u_zz"][h].shape == (T, Ns) and d["u_acc"][h].shape == (T, Ns)
            assert d["rint"][h].min() >= 0 and d["rint"][h].max() < Nc
            for t in range(T):
                assert np.array_equal(d["movers"][h][t], np.flatnonzero(lab[t] == h))          # ascending walker order
                other = np.flatnonzero(lab[t] != h)
                for b in range(nb):
                    assert np.all(lab[t][d["cw"][h][b, t]] == 1 - h), "a complement is never in the mover's own set"
                    assert np.array_equal(other[d["rint"][h][b, t]], d["cw"][h][b, t])         # rint indexes the ascending list
            for u in (d["u_zz"][h], d["u_acc"][h]):
                assert np.all((u >= 0.0) & (u < 1.0))
            differ = differ or np.any(d["cw"][h][0] != d["cw"][h][1])
    assert differ, "different branches must draw different complements somewhere"


def test_every_walker_is_in_the_first_set_with_the_balanced_share():
    T, W, nb, N = 2, 26, 1, 200
    n0 = (W + 1) // 2
    count = np.zeros((T, W))
    for it in range(N):
        count += stretch_draws(SEED, it, T, W, nb)["labels"] == 0
    p = n0 / W
    sd = np.sqrt(p * (1 - p) / N)
    assert np.all(np.abs(count / N - p) <= 5 * sd), np.abs(count / N - p).max() / sd


def test_complement_positions_and_uniforms_look_uniform():
    """Coarse distribution checks (5 standard deviations): the complement index over [0, Nc), the two uniforms' means."""
    T, W, nb = 2, 64, 2
    r, uz, ua = [], [], []
    for it in range(100):
        d = stretch_draws(SEED, it, T, W, nb)
        r.append(d["rint"][0].ravel()); uz.append(d["u_zz"][0].ravel()); ua.append(d["u_acc"][1].ravel())
    r, uz, ua = np.concatenate(r), np.concatenate(uz), np.concatenate(ua)
    Nc = W // 2
    hist = np.bincount(r, minlength=Nc)
    p = 1.0 / Nc
    assert np.all(np.abs(hist / len(r) - p) <= 5 * np.sqrt(p * (1 - p) / len(r)))
    for u in (uz, ua):
        assert abs(u.mean() - 0.5) <= 5 * np.sqrt(1 / 12 / len(u))


def test_draws_depend_on_the_global_rung_and_walker_only():
    """The draws of iteration i are a function of (seed, i, global rung, walker, half, branch): the specification has no other
    input - in particular not the between-model schedule -, and a context that holds rungs 1 .. 2 of a ladder (rung_begin = 1)
    regenerates what the context holding rungs 0 .. 2 draws for them."""
    W, nb, it = 26, 2, 7
    whole = stretch_draws(SEED, it, 3, W, nb)
    part = stretch_draws(SEED, it, 2, W, nb, rung_begin=1)
    assert np.array_equal(whole["labels"][1:], part["labels"])
    for h in range(2):
        assert np.array_equal(whole["rint"][h][:, 1:], part["rint"][h])
        assert np.array_equal(whole["u_zz"][h][1:], part["u_zz"][h]) and np.array_equal(whole["u_acc"][h][1:], part["u_acc"][h])
    other = stretch_draws(SEED, it + 1, 3, W, nb)
    assert not np.array_equal(whole["labels"], other["labels"]) and not np.array_equal(whole["u_zz"][0], other["u_zz"][0])
    assert not np.array_equal(whole["u_zz"][0][0], whole["u_zz"][0][1]), "rungs must not share their draws"
    assert not np.array_equal(whole["u_zz"][0], whole["u_acc"][0])
