"""Ladder families for the replays of tests/test_hip_ladders.py and tests/test_ladder_families.py (host only, NumPy, no RNG).

Every other replay steps ``make_ladder(D, ntemps=T)``: geometric, beta_0 = 1, strictly decreasing, strictly positive.  The
reference takes two more kinds of ladder and validates neither (tempering.py:257-270): ``Tmax=np.inf`` appends a beta = 0 rung, and
``betas=`` is whatever the user hands over.

``ladder(kind, T, D)`` -> betas[T]

  geometric   ``make_ladder(D, ntemps=T)``.
  inf         ``make_ladder(D, ntemps=T, Tmax=np.inf)``: the last rung is exactly 0.
  user        a hand-made ladder (see ``user_features`` for where its features sit):
                * beta_0 = 0.8 and every rung scaled by it: the only input that tells ``1 / betas[0]`` from 1.0;
                * one repeated pair beta_i = beta_{i+1} in the cold half, i >= 1 and i + 1 <= T - 2 (both are rungs the adaptation
                  moves): d beta = 0, every swap of the pair is accepted, its delta T is 0 and stays 0;
                * one steep gap in the hot half: every beta from rung j on times 1e-4, so that swaps across (j - 1, j) have a
                  ratio of exactly 0 in double precision once the rungs sit where their temperatures put them;
                * the last rung 0.
              Ladders shorter than 6 rungs have no room for all of it: T = 4, 5 drop the steep gap, T = 2, 3 the repeated pair too
              (what is left: 0.8 times the geometric ladder, last rung 0).
              The base is the geometric ladder with its SPAN capped: ``make_ladder(D, ntemps=T, Tmax=min(tstep^(T-1), 16))``.
              Uncapped, a 16-rung ladder in 8 dimensions is at beta = 1e-4 three quarters of the way up and a 100-rung one at
              1e-37: the rung under the gap would be as free as the rung over it, swaps across it a coin flip whatever the gap's
              width, and "no swap crosses the steep gap" could not be asked for.  With the cap the rung under the gap keeps
              beta >= 0.8 / 16 = 0.05.  Where the geometric ladder spans less than 16 (T <= 4 or so) the base is that ladder.
  user_pos    ``user`` with the last rung 1e-300 instead of 0: 1 / beta is finite but enormous, and only the hottest rung - which
              the adaptation leaves alone - holds it.

``tempered_start(betas, W, D, box, seed)`` -> x0[T, W, D]: rung t drawn where its temperature puts it - N(0, 1 / beta_t) where
that fits the box three times over, uniform on 0.95 of the box otherwise (beta = 0 included).  The replays start there: with every
rung started from the same cloud the rungs over the steep gap would need hundreds of iterations to spread, and a beta = 0 rung
would not meet the box within a test's five iterations.
"""
import numpy as np          # NumPy and nothing else at module level: tests/golden/make_golden.py imports this file by name, from a
#                             copy beside it (tests/test_golden_regeneration.py), where neither the package nor the oracle is on the path

KINDS = ("geometric", "inf", "user", "user_pos")
BETA0 = 0.8
GAP = 1e-4
SPAN = 16.0


def user_features(T):
    """(i, j): the repeated pair is (i, i + 1), the steep gap sits between j - 1 and j; None where the ladder is too short."""
    i = max(1, T // 4) if T >= 4 else None
    j = max(i + 2, (3 * T) // 4) if T >= 6 else None
    assert i is None or (i >= 1 and i + 1 <= T - 2)
    assert j is None or (i + 2 <= j <= T - 2 and j >= T // 2)
    return i, j


def ladder(kind, T, D, make_ladder=None):
    """``make_ladder``: the constructor of geometric ladders to build from - the pinned restatement of the reference's
    (oracle/eryn_oracle.py) unless the caller hands over another (tests/golden/make_golden.py: the reference's own)."""
    if make_ladder is None:
        from oracle.eryn_oracle import make_ladder
    T, D = int(T), int(D)
    if kind == "geometric":
        return make_ladder(D, ntemps=T)
    if kind == "inf":
        return make_ladder(D, ntemps=T, Tmax=np.inf)
    if kind not in ("user", "user_pos"):
        raise ValueError(f"unknown ladder family {kind!r}")
    if T < 2:
        raise ValueError("a hand-made ladder needs two rungs")
    g = make_ladder(D, ntemps=T)
    b = BETA0 * (g if g[-1] >= 1.0 / SPAN else make_ladder(D, ntemps=T, Tmax=SPAN))
    i, j = user_features(T)
    if i is not None:
        b[i + 1] = b[i]
    if j is not None:
        b[j:] *= GAP
    b[-1] = 0.0 if kind == "user" else 1e-300
    return b


def tempered_start(betas, W, D, box, seed=3, scale=1.0):
    """``scale``: factor on the normal rungs' spread (the Rosenbrock cases start narrower)"""
    betas = np.asarray(betas, dtype=np.float64)
    rs = np.random.RandomState(seed)
    z = rs.randn(len(betas), W, D)
    u = rs.uniform(-0.95 * box, 0.95 * box, size=z.shape)
    with np.errstate(divide="ignore"):
        s = scale / np.sqrt(betas)
    fits = 3.0 * s < box
    return np.where(fits[:, None, None], np.clip(z * np.where(fits, s, 1.0)[:, None, None], -0.95 * box, 0.95 * box), u)


# ---- the cases of tests/test_hip_ladders.py (GPU: hens_step replayed) and tests/test_ladder_families.py (CPU: sized here) ----------
LAG, NU = 50, 10             # a strong adaptation: the ladder moves in its leading digits within a case's five iterations


def case(T, W, D, families, path, calls=(1, 4), like="dense", box=50.0, hot_box=None, x_scale=1.0, mh=None, periodic=False, nsplits=2, kw=None,
         env=None, ranks=0, seed=77):
    """``path``: what a profiled call reports for the shape - "one" launch per iteration (k_iter), "two" in-place launches
    (k_stretch_fast / k_stretch2 + k_split1_pt), "copying" (the copying half-steps + the stand-alone cascade, one launch per set
    with more than two sets), "pipe" (ranks of the ladder pipeline: not reported), "sampler" (not a replay case of its own).
    ``box``: the prior box; ``hot_box``: the box where the rung under a beta = 0 rung is still cold - the "inf" family on a short
    ladder, and "user" ladders too short for a steep gap.  The beta = 0 rung fills its box: its log-likelihoods are some
    -0.075 D box^2 (uniform coordinates under precisions around 0.5), the rung's below some -D / (2 beta_{T-2}), and the hottest
    pair trades walkers only where the two meet, box ~ 2.6 / sqrt(beta_{T-2}), to within a relative 1 / sqrt(D).  The values
    below are 0.8 to 1.0 of that (tests/test_ladder_families.py: a fifth to a half of the pair's swaps accepted, the coldest rung
    well inside).  A "user" ladder with a steep gap needs the opposite - a box wide enough that nothing crosses the gap - and
    has a hot end of 1e-5 and less, which swaps freely with a beta = 0 rung in any box."""
    return dict(T=T, W=W, D=D, families=tuple(families), path=path, calls=tuple(calls), like=like, box=box, hot_box=hot_box,
                x_scale=x_scale, mh=mh,
                periodic=periodic, nsplits=nsplits, kw=kw or {}, env=env or {}, ranks=ranks, seed=seed)


IU, IUP, GIU = ("inf", "user"), ("inf", "user", "user_pos"), ("geometric", "inf", "user")
MIX = ("iso", 0.3, 0.5)
CASES = {
    # block-balanced labels with cb T = 128: full tiles.  Two launches per iteration (the records in column order) at every width
    # but 16 and 32, whose grids of up to one / two workgroups per CU step in one launch
    "full_tiles_T16_D8": case(16, 40, 8, IUP, "two"),
    "full_tiles_T8_D8": case(8, 48, 8, IUP, "two", hot_box=27.0),
    "full_tiles_T8_D16": case(8, 48, 16, IUP, "one", hot_box=12.0),
    # ladders that do not divide 128: short tiles; 33 rungs: two-word swap masks - in two launches (k_split1_pt) and in one
    "short_tiles_T10_D8": case(10, 256, 8, IU, "two", hot_box=62.0),
    "short_tiles_T33_D8": case(33, 130, 8, IU, "two"),
    "short_tiles_T10_D16": case(10, 256, 16, IU, "one", hot_box=22.0),
    "short_tiles_T33_D16": case(33, 130, 16, IU, "one"),
    # one launch per iteration (k_iter): the adaptation rides in hens_iter.h
    "one_launch_T4_D16": case(4, 128, 16, IU, "one", hot_box=3.9),
    "one_launch_T8_D32": case(8, 64, 32, IU, "one", hot_box=7.1),
    "one_launch_T64_D32": case(64, 64, 32, IU, "one"),
    # D = 64 / 128: matrix pipe, k_stretch_fast and - forced onto a small grid - the persistent k_stretch2 (hens_tile2.h)
    "dense_D64": case(8, 1024, 64, IU, "two", hot_box=5.0),
    "dense_D128": case(7, 256, 128, IU, "two", hot_box=4.0),
    "tile2_forced_D64": case(4, 512, 64, IU, "two", hot_box=3.3, env={"HENS_TILE2_FORCE": "1", "HENS_TILE2_LOG": "1"}),
    # the generic-width kernel, three copying launches; rows padded to the next compile-time width
    "generic_D5": case(5, 100, 5, IU, "copying", hot_box=10.0, kw={"pad_rows": False}),
    "padded_D11": case(8, 256, 11, ("inf",), "one", hot_box=22.0),
    # the Metropolis-Hastings move in the mix (its cascade's counts are adapted apart)
    "mh_T8_D32": case(8, 256, 32, IU, "one", hot_box=7.1, calls=(3, 6), mh=MIX),
    "mh_T6_D32": case(6, 256, 32, IU, "one", hot_box=4.7, calls=(3, 6), mh=MIX),
    # ... between two in-place launches: the MH launch addresses the records by slot, and its cascade's counts feed k_stretch_fast's fold
    "mh_T6_D64": case(6, 256, 64, IU, "two", hot_box=3.7, calls=(3, 6), mh=MIX),
    "three_sets_D8": case(3, 67, 8, ("user",), "copying", hot_box=4.45, nsplits=3),
    "diag_D32": case(4, 512, 32, ("inf",), "one", hot_box=3.5, like="diag"),
    "rosenbrock_D32": case(32, 256, 32, ("inf",), "one", like="rosen", box=6.0, x_scale=0.5),
    "periodic_D16": case(8, 256, 16, ("inf",), "one", hot_box=15.0, periodic=True),
    # 65 rungs and more: no block-balanced labels (copying launches); two rungs per lane in the folded adaptation up to 128 rungs,
    # the stand-alone adaptation kernel above; swap masks of three to five words
    "long_T65_D8": case(65, 16, 8, GIU, "copying"),
    "long_T70_D16": case(70, 64, 16, GIU, "copying"),
    "long_T100_D8": case(100, 64, 8, GIU, "copying"),
    "long_T128_D32": case(128, 32, 32, GIU, "copying", kw={"live_dangerously": True}),
    "long_T130_D8": case(130, 16, 8, GIU, "copying"),
    # the adaptation switched off / stopping after two iterations: the ladder handed over must come back untouched / stop moving
    "adaptation_off": case(4, 128, 16, ("user",), "one", hot_box=3.9, kw={"adaptive": False}),
    "adaptation_stops": case(4, 128, 16, ("user",), "one", hot_box=3.9, kw={"stop_adaptation": 2}),
    # ranks of the ladder pipeline (tests/pipeline_worker.py replay): the beta ring carries the ladder from rank to rank
    "pipeline_2_ranks_D32": case(8, 256, 32, IU, "pipe", hot_box=7.1, calls=(2, 4), ranks=2, seed=11),
    "pipeline_4_ranks_D32": case(8, 256, 32, IU, "pipe", hot_box=7.1, calls=(2, 4), ranks=4, seed=11),
    "pipeline_4_ranks_T100_D8": case(100, 64, 8, IU, "pipe", calls=(2, 4), ranks=4, seed=11),
    # EnsembleSampler(rng="philox") stepped 20 iterations (sized here, run by the sampler-level test)
    "sampler_T6_D8": case(6, 64, 8, IU, "sampler", hot_box=11.0, calls=(20,)),
}
# one case per family at the adaptation's default constants (lag 10000, time 100)
DEFAULT_CONSTANTS = [("full_tiles_T16_D8", "user_pos"), ("one_launch_T8_D32", "inf"), ("dense_D64", "user"), ("long_T70_D16", "geometric")]


# hens_rj_step on leaf-packing states (tests/test_hip_rj.py: _replay_rj, tests/test_hip_rj_stretch.py: _replay_stretch - their model,
# two starting leaves of the first branch and one of the second: ladders of 9 dimensions)
RJ_D = 9


def rj_case(T, W, nl_max, iters, families, in_model="gaussian", seed=11):
    return dict(T=T, W=W, nl_max=nl_max, iters=iters, families=tuple(families), in_model=in_model, seed=seed)


RJ_CASES = {
    "rj_T4_W10": rj_case(4, 10, (3, 4), 8, IU),
    "rj_T3_W12_10_leaves": rj_case(3, 12, (10, 10), 6, IU),
    "rj_stretch_T4_W64": rj_case(4, 64, (2, 2), 8, ("inf",), in_model="stretch", seed=23),
    "rj_T66_W8": rj_case(66, 8, (2, 2), 6, ("inf",)),               # above rj_adapt_wave's 64 rungs: the stand-alone adaptation
}


def check_rj_coverage(family, T, W, betas0, betas, accepted, swaps, cascades, spare=1, what=""):
    """``check_coverage`` for hens_rj_step.  ``accepted[T]``: accepted in-model and birth / death proposals per rung; ``swaps[T - 1]``:
    accepted swaps per adjacent pair over ``cascades`` cascades (two per iteration) of W proposals each.  The ladders of these
    cases are too short for a steep gap (or of the "inf" family)."""
    i, j = user_features(T) if family in ("user", "user_pos") else (None, None)
    assert j is None
    assert np.all(accepted >= spare), f"{what}: a rung accepted fewer than {spare} proposals: {accepted}"
    assert np.all(swaps >= spare), f"{what}: an adjacent pair swapped fewer than {spare} times: {swaps}"
    if i is not None:
        assert swaps[i] == cascades * W, f"{what}: the repeated pair ({i}, {i + 1}) refused a swap: {swaps[i]} of {cascades * W}"
        assert betas[i] == betas[i + 1], f"{what}: the repeated pair came apart: {betas[i]!r} / {betas[i + 1]!r}"
    assert betas[0] == betas0[0] and betas[-1] == betas0[-1] == 0.0, f"{what}: the adaptation moved an end of the ladder"
    assert not np.array_equal(betas, betas0), f"{what}: the adaptation moved nothing"


def period_of(D):
    """a third of the parameters periodic, periods small enough that the walkers spread over more than half of them
    (tests/test_hip_replay.py: test_replay_periodic_parameters)"""
    period = np.zeros(D)
    period[::3] = np.linspace(1.5, 4.0, len(period[::3]))
    return period


def box_of(c, family):
    return c["hot_box"] if c["hot_box"] is not None and (family == "inf" or c["T"] < 6) else c["box"]


def case_inputs(c, family):
    """-> betas[T], x0[T, W, D], box of a case under a ladder family"""
    betas = ladder(family, c["T"], c["D"])
    x0 = tempered_start(betas, c["W"], c["D"], box_of(c, family), scale=c["x_scale"])
    return betas, x0, box_of(c, family)


def new_stats(T):
    return dict(proposals=np.zeros(T), outside=np.zeros(T))


def check_coverage(family, T, W, betas0, betas, accepted, swaps, rungs, iters, spare=1, adaptive=True, what=""):
    """The conditions a case must meet on the ORACLE's side for its comparison to mean something.  ``accepted[T]``: accepted
    proposals per rung; ``swaps[T - 1]``: accepted swaps per adjacent pair over ``iters`` cascades of W proposals each; ``rungs``:
    per-rung proposals / proposals outside the box (new_stats); ``spare``: the factor the counts must clear their bound by (the CPU
    sizing asks for 2, the GPU replay for 1)."""
    i, j = user_features(T) if family in ("user", "user_pos") else (None, None)
    assert np.all(accepted >= spare), f"{what}: a rung accepted fewer than {spare} proposals: {accepted}"
    pairs = np.arange(T - 1) != (-1 if j is None else j - 1)
    assert np.all(swaps[pairs] >= spare), f"{what}: an adjacent pair swapped fewer than {spare} times: {swaps}"
    if i is not None:
        assert swaps[i] == iters * W, f"{what}: the repeated pair ({i}, {i + 1}) refused a swap: {swaps[i]} of {iters * W}"
        assert betas[i] == betas[i + 1], f"{what}: the repeated pair came apart: {betas[i]!r} / {betas[i + 1]!r}"
    if j is not None:
        assert swaps[j - 1] == 0, f"{what}: {swaps[j - 1]} swaps crossed the steep gap ({j - 1}, {j})"
    if family == "inf":
        # the beta = 0 rung walks the whole box: its proposals leave it more often than the coldest rung's.  To spare: a share p of n
        # proposals scatters by sigma = sqrt(p (1 - p) / n) with the draws; the sizing run (spare = 2) asks for a distance of 6 sigma
        # of the difference, so that other draws do not turn the order round.
        n_hot, n_cold = rungs["proposals"][-1], rungs["proposals"][0]
        hot, cold = rungs["outside"][-1] / n_hot, rungs["outside"][0] / n_cold
        need = 3.0 * spare * np.sqrt(hot * (1.0 - hot) / n_hot + cold * (1.0 - cold) / n_cold) if spare > 1 else 0.0
        assert rungs["outside"][-1] >= spare and hot > cold + need, \
            f"{what}: the beta = 0 rung's proposals leave the box at {hot:.3f}, the coldest rung's at {cold:.3f} (distance asked for: {need:.3f})"
    assert betas[0] == betas0[0] and betas[-1] == betas0[-1], f"{what}: the adaptation moved an end of the ladder"
    if adaptive and T > 2 and iters > 0:
        assert not np.array_equal(betas, betas0), f"{what}: the adaptation moved nothing"
    if not adaptive:
        assert np.array_equal(betas, betas0), f"{what}: the ladder moved although the adaptation is off"
