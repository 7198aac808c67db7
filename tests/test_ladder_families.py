"""The ladder families of tests/ladders.py and the cases of tests/test_hip_ladders.py, sized on the CPU (no GPU).

1. What the families are: the features sit where ``ladders.user_features`` says, fixture f9's ladder - built by the reference's
   own ``make_ladder`` - is ``ladder("user", 6, 5)`` bit for bit, and the oracle's adaptation keeps a ladder's ends and a repeated
   pair exactly (what the replays then ask of the device).
2. Every (case, family) the GPU file replays runs here through ``OracleSampler`` alone, free, with NumPy's draws, for the case's
   iteration count, and must meet the GPU file's coverage conditions (``ladders.check_coverage``) with a factor of 2 to spare -
   and, for the steep gap, over twice the iterations.  The GPU replays consume other draws (Philox), so this is what makes a
   coverage assertion there a statement about the device and not about the choice of shape, start or seed.  A case that misses
   is changed HERE (shape, start, gap), never relaxed there.
"""
import numpy as np
import pytest

from oracle import eryn_oracle as orc
from tests import golden_io
from tests import ladders as ld
from tests import parity_utils as pu


def test_families_are_what_they_say():
    for T, D in [(2, 5), (3, 8), (4, 16), (5, 5), (6, 5), (8, 32), (16, 8), (33, 16), (65, 8), (100, 8), (130, 8)]:
        g, inf, user, pos = (ld.ladder(k, T, D) for k in ld.KINDS)
        assert np.array_equal(g, orc.make_ladder(D, ntemps=T)) and g[0] == 1.0 and np.all(np.diff(g) < 0) and g[-1] > 0
        assert np.array_equal(inf, orc.make_ladder(D, ntemps=T, Tmax=np.inf)) and inf[-1] == 0.0 and inf[0] == 1.0
        assert np.all(inf[:-1] > 0) and np.all(np.diff(inf) < 0)
        assert user[0] == ld.BETA0 and user[-1] == 0.0 and pos[-1] == 1e-300 and np.array_equal(user[:-1], pos[:-1])
        i, j = ld.user_features(T)
        assert (i is None) == (T < 4) and (j is None) == (T < 6)                 # steep gap dropped first, then the repeated pair
        steps = user[1:] / user[:-1]
        for k in range(T - 2):
            if k == i:
                assert steps[k] == 1.0 and 1 <= i and i + 1 <= T - 2 and i + 1 <= T // 2
            elif j is not None and k == j - 1:
                assert steps[k] < 2 * ld.GAP and j >= T // 2 and user[j - 1] >= ld.BETA0 / ld.SPAN
            else:                                # (the step behind the repeated pair is two of the base ladder's)
                assert (0.09 if i is not None and k == i + 1 else 0.3) < steps[k] < 1.0, (T, D, k, steps[k])
        assert np.array_equal(ld.ladder("user", T, D), user)                       # no RNG, no state
    with pytest.raises(ValueError):
        ld.ladder("random", 4, 4)


def test_fixture_f9_is_the_user_ladder_and_f10_is_long(golden_dir):
    f9, f10 = golden_io.load(golden_dir, "f9_userladder"), golden_io.load(golden_dir, "f10_longladder")
    assert np.array_equal(f9["betas0"], ld.ladder("user", 6, 5))
    assert float(f9["adaptation_lag"]) == ld.LAG and float(f9["adaptation_time"]) == ld.NU
    n = int(f9["nsteps"])
    last = f9[f"it{n - 1}_betas"]
    i, j = ld.user_features(6)
    assert last[0] == ld.BETA0 and last[-1] == 0.0 and last[i] == last[i + 1]      # the reference keeps the ends and the pair
    assert np.max(np.abs(last[1:-1] / f9["betas0"][1:-1] - 1.0)) > 1e-3             # ... and moves the rest in its leading digits
    assert all(f9[f"it{k}_swaps_accepted"][i] == int(f9["W"]) for k in range(n))   # d beta = 0: every swap accepted
    assert int(f10["T"]) == 70 and np.array_equal(f10["betas0"], ld.ladder("geometric", 70, 3))
    assert np.max(np.abs(f10[f"it{int(f10['nsteps']) - 1}_betas"][1:-1] / f10["betas0"][1:-1] - 1.0)) > 1e-3


def _free_oracle(c, family, lag=ld.LAG, nu=ld.NU):
    """The case's problem under an OracleSampler that draws for itself (NumPy)."""
    T, W, D = c["T"], c["W"], c["D"]
    betas, x0, box = ld.case_inputs(c, family)
    mu, invcov = pu.gaussian_problem(D, dense=(c["like"] == "dense"))
    if c["like"] == "dense":
        fn = lambda x: orc.gaussian_log_like(x, mu, invcov)                       # noqa: E731
    elif c["like"] == "diag":
        iv = np.diag(invcov).copy()
        fn = lambda x: orc.gaussian_diag_log_like(x, mu, iv)                      # noqa: E731
    else:
        fn = orc.rosenbrock_log_like
    moves = None if c["mh"] is None else [("stretch", 1.0 - c["mh"][2]), (orc.GaussianProposal(c["mh"][1] ** 2), c["mh"][2])]
    kw = {k: v for k, v in c["kw"].items() if k in ("adaptive", "stop_adaptation", "live_dangerously")}
    return orc.OracleSampler(x0, fn, np.full(D, -box), np.full(D, box), np.random.RandomState(c["seed"]),
                             np.random.RandomState(c["seed"] + 1), betas=betas, adaptation_lag=lag, adaptation_time=nu,
                             record=True, moves=moves, period=ld.period_of(D) if c["periodic"] else None, nsplits=c["nsplits"], **kw)


@pytest.mark.parametrize("name,family,constants", [(n, f, (ld.LAG, ld.NU)) for n, c in sorted(ld.CASES.items()) for f in c["families"]] +
                         [(n, f, (10000, 100)) for n, f in ld.DEFAULT_CONSTANTS])
def test_oracle_alone_meets_the_coverage_conditions_with_a_factor_of_two_to_spare(name, family, constants):
    """every case at the strong adaptation, and the cases the GPU file runs at the default constants at those"""
    c = ld.CASES[name]
    T, W, n = c["T"], c["W"], sum(c["calls"])
    o = _free_oracle(c, family, *constants)
    betas0 = o.betas.copy()
    rungs, swaps = ld.new_stats(T), np.zeros(T - 1)
    for it in range(2 * n):
        o.iteration()
        rec = o.trace.pop()
        for k in [f"logp{sp}" for sp in range(o.nsplits)] + ["mh_logp"]:
            if k in rec:
                rungs["proposals"] += rec[k].shape[1]
                rungs["outside"] += np.isinf(rec[k]).sum(axis=1)
        swaps += o.swaps_accepted
        if it == n - 1:
            ld.check_coverage(family, T, W, betas0, o.betas, o.accepted.sum(axis=1), swaps, rungs, n, spare=2,
                              adaptive=c["kw"].get("adaptive", True), what=f"{name} / {family}")
    _, j = ld.user_features(T) if family in ("user", "user_pos") else (None, None)
    if j is not None:
        assert swaps[j - 1] == 0, f"{name} / {family}: {swaps[j - 1]} swaps crossed the steep gap within {2 * n} iterations"
    assert np.all(np.isfinite(o.betas)) and np.all(o.betas >= 0)


@pytest.mark.parametrize("name,family", [(n, f) for n, c in sorted(ld.RJ_CASES.items()) for f in c["families"]])
def test_rj_oracle_alone_meets_the_coverage_conditions_with_a_factor_of_two_to_spare(name, family):
    """the leaf-packing cases: the model and start of the RJ replays (tests/test_hip_rj_stretch.py: _model) under OracleRJSampler
    drawing for itself"""
    from oracle import eryn_oracle_rj as orj
    from tests.test_hip_rj_stretch import BOXES, KINDS, NAMES, _model
    c = ld.RJ_CASES[name]
    T, W = c["T"], c["W"]
    _, t, y, sigma, x, inds, _ = _model(T, W, c["nl_max"], (0, 0), 60, c["seed"], (2, 1))
    scale = np.array([[1e-2, 1e-2, 1e-3], [1e-2, 1e-2, 1e-2]])                   # (tests/test_hip_rj.py: _replay_rj)
    okind = {"pulse": orj.KIND_PULSE, "sine": orj.KIND_SINE}
    obr = [orj.Branch(k, okind[KINDS[k]], BOXES[k], c["nl_max"][i], 0, cov=np.diag(scale[i] ** 2)) for i, k in enumerate(NAMES)]
    betas0 = ld.ladder(family, T, ld.RJ_D)
    o = orj.OracleRJSampler(obr, x, inds, t, y, sigma, np.random.RandomState(c["seed"]), np.random.RandomState(c["seed"] + 1), betas0.copy(),
                            adaptation_lag=ld.LAG, adaptation_time=ld.NU, in_model=c["in_model"])
    accepted, swaps = np.zeros(T), np.zeros(T - 1)
    pt = o._pt

    def counting_pt(adapt, rec):
        pt(adapt, rec)
        swaps[:] += o.swaps_accepted

    o._pt = counting_pt
    for _ in range(c["iters"]):
        acc, _, racc = o.iteration()
        accepted += (np.asarray(acc, dtype=np.float64) + racc).sum(axis=1)
    ld.check_rj_coverage(family, T, W, betas0, o.st.betas, accepted, swaps, 2 * c["iters"], spare=2, what=f"{name} / {family}")
