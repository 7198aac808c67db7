#!/usr/bin/env python
"""Generate tests/golden/distgen/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dist.py        (GOLDEN_OUT=<dir>: write there instead)

``eryn.moves.DistributionGenerate`` (distgen.py:10-104 under mh.py:56-193) with make_golden_priors.py's capture technique (the R proxy
and the likelihood of make_golden.py, the global stream's calls wrapped, the moves' and the sampler's methods hooked):

  dg1_mix          T = 3, W = 10, D = 4, 12 iterations of [(StretchMove, 0.5), (DistributionGenerate, 0.5)] with parallel tempering
                   and ladder adaptation.  The prior is make_golden_priors.py's container; the generator is a DIFFERENT container
                   that mixes the three kinds and is narrower than the start in two coordinates:
                       0 uniform_dist(-1.5, 2.0)   1 log_uniform(0.05, 2.5)   2 scipy.stats.norm(-0.3, 0.6)   3 scipy.stats.norm(2.0, 1.0)
  dg2_prior_draws  untempered, DistributionGenerate alone, generator = the prior, all uniform.
  dg3_periodic_mix T = 3, W = 16, D = 4, 16 iterations of [(StretchMove(periodic=pc), 0.5), (DistributionGenerate(periodic=pc), 0.5)]
                   with the same ``PeriodicContainer``: coordinates 0 and 2 periodic (periods 2 and 3), the prior's box and the
                   generator's uniform terms reach half a period beyond [0, period] on both sides there.  The stretch move wraps
                   (stretch.py:149-154); the move never does: its accepted points stay outside [0, period).

Every iteration records which move ran (``kind``: 0 stretch, 1 the move), its draws of the sampler's stream R, its proposals ``q``,
``factors``, ``logp``, ``logl``, the accept mask, the state after the move and after the sweep, the sweep's draws, swap counts and
ladder.  The global stream G is consumed by nothing else than what is recorded - a stretch iteration's label shuffles, a move
iteration's ``rvs``, the sweep's permutations and uniforms - so a reader can repeat every ``rvs`` from ``seed_run``.
Distributions travel as the ARGUMENTS of the reference's constructors (``*_kind``: 0 uniform_dist, 1 log_uniform, 2 scipy.stats.norm; ``*_p0`` / ``*_p1``).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402  (sets up the reference's import path; nothing runs on import)
import make_golden_priors as mgp            # noqa: E402

import numpy as np                          # noqa: E402
from scipy import stats                     # noqa: E402
from eryn.ensemble import EnsembleSampler   # noqa: E402
from eryn.moves import DistributionGenerate, StretchMove  # noqa: E402
from eryn.prior import ProbDistContainer, log_uniform, uniform_dist  # noqa: E402
from eryn.utils import PeriodicContainer    # noqa: E402

OUT = os.environ.get("GOLDEN_OUT", os.path.join(HERE, "distgen"))
GEN1 = (np.array([0, 1, 2, 2]), np.array([-1.5, 0.05, -0.3, 2.0]), np.array([2.0, 2.5, 0.6, 1.0]))
BOX2 = (np.array([0, 0, 0]), np.array([-3.0, -2.0, -4.0]), np.array([3.0, 4.0, 2.0]))
PERIOD3 = {0: 2.0, 2: 3.0}                  # [-p / 2, 3 p / 2]: coordinates 0 and 2 of BOX3 and GEN3
BOX3 = (np.array([0, 0, 0, 0]), np.array([-1.0, -3.0, -1.5, 0.01]), np.array([3.0, 3.0, 4.5, 8.0]))
GEN3 = (np.array([0, 2, 0, 1]), np.array([-1.0, 0.5, -1.5, 0.05]), np.array([3.0, 0.8, 4.5, 7.5]))


def container(kinds, p0, p1):
    make = {0: uniform_dist, 1: log_uniform, 2: stats.norm}
    return ProbDistContainer({d: make[int(kinds[d])](float(p0[d]), float(p1[d])) for d in range(len(kinds))})


def periodic_container(periodic):
    return None if periodic is None else PeriodicContainer({"model_0": dict(periodic)})


def capture(name, T, W, prior, gen, mix, nsteps, mu, x0, seed_construct=123, seed_run=456, periodic=None):
    D = len(prior[0])
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    invcov = np.linalg.inv(A @ A.T / D + np.eye(D))
    np.random.seed(seed_construct)
    pc = periodic_container(periodic)            # (handed to both moves; the sampler itself gets none)
    kw = {} if pc is None else dict(periodic=pc)
    dist_move = DistributionGenerate({"model_0": container(*gen)}, **kw)
    moves = [(StretchMove(**kw), 0.5), (dist_move, 0.5)] if mix else dist_move
    s = EnsembleSampler(W, D, mg.log_like_vec, container(*prior), args=[mu, invcov], vectorize=True, moves=moves,
                        **(dict(tempering_kwargs=dict(ntemps=T)) if T > 1 else {}))
    rlog, glog, plog = [], [], []
    s._random = mg.RProxy(s._random, rlog)
    orig_shuffle, orig_perm, orig_unif = np.random.shuffle, np.random.permutation, np.random.uniform

    def shuffle(x):
        orig_shuffle(x)
        glog.append(("shuffle", np.array(x, copy=True)))

    def permutation(n):
        out = orig_perm(n)
        glog.append(("permutation", np.array(out, copy=True)))
        return out

    def uniform(*a, **k):
        out = orig_unif(*a, **k)
        glog.append(("uniform", np.array(out, copy=True)))
        return out

    tc = s.temperature_control
    orig_lp, orig_ll = s.compute_log_prior, s.compute_log_like

    def compute_log_prior(coords, **k):
        out = orig_lp(coords, **k)
        plog.append(("logp", out.copy()))
        return out

    def compute_log_like(coords, **k):
        out = orig_ll(coords, **k)
        plog.append(("logl", out[0].copy()))
        return out

    s.compute_log_prior, s.compute_log_like = compute_log_prior, compute_log_like

    def hook_move(move, tag):
        orig_get_proposal, orig_update = move.get_proposal, move.update

        def get_proposal(*a, **k):
            q, factors = orig_get_proposal(*a, **k)
            plog.append((tag, None))
            plog.append(("q", q["model_0"][:, :, 0, :].copy()))
            plog.append(("factors", np.array(factors, copy=True)))
            return q, factors

        def update(old_state, new_state, accepted, subset=None):
            plog.append(("keep", (accepted if subset is None else np.take_along_axis(accepted, subset, axis=1)).copy()))
            if subset is not None:
                plog.append(("subset", subset.copy()))
            out = orig_update(old_state, new_state, accepted, subset=subset)
            plog.append(("x_after", out.branches["model_0"].coords[:, :, 0, :].copy()))
            plog.append(("LP_after", (out.log_like.copy(), out.log_prior.copy())))
            return out

        move.get_proposal, move.update = get_proposal, update

    for m, tag in zip(s.moves, ("stretch", "dist") if mix else ("dist",)):
        hook_move(m, tag)
    if tc is not None:
        orig_dsi = tc.do_swaps_indexing

        def do_swaps_indexing(i, iperm_sel, i1perm_sel, *a, **k):
            plog.append(("swap_idx", (i, iperm_sel.copy(), i1perm_sel.copy())))
            return orig_dsi(i, iperm_sel, i1perm_sel, *a, **k)

        tc.do_swaps_indexing = do_swaps_indexing

    out = dict(T=T, W=W, D=D, nsteps=nsteps, seed_construct=seed_construct, seed_run=seed_run, mu=mu, invcov=invcov, x0=x0,
               prior_kind=prior[0], prior_p0=prior[1], prior_p1=prior[2], gen_kind=gen[0], gen_p0=gen[1], gen_p1=gen[2], mix=int(mix))
    if mix:
        out["a"] = float(s.moves[0].a)
    if periodic is not None:
        out["period"] = np.array([float(periodic.get(d, 0.0)) for d in range(D)])
        assert all(m.periodic is pc for m in s.moves)
    if tc is not None:
        out["betas0"] = np.array(tc.betas, copy=True)
        assert bool(tc.adaptive) and bool(tc.permute)
    kinds = []
    np.random.seed(seed_run)
    np.random.shuffle, np.random.permutation, np.random.uniform = shuffle, permutation, uniform
    try:
        it = 0
        for state in s.sample(x0 if T > 1 else x0[0], iterations=nsteps, store=False):
            pre = f"it{it}_"
            pl = list(plog)
            plog.clear()
            if it == 0:                     # the initial evaluation: logp, then logl of x0 (ensemble.py:898-912)
                assert pl[0][0] == "logp" and pl[1][0] == "logl"
                out["P0"], out["L0"] = pl[0][1].reshape(T, W), pl[1][1].reshape(T, W)
                pl = pl[2:]
            is_dist = any(k == "dist" for k, _ in pl)
            kinds.append(int(is_dist))
            rl = [k for k, _ in rlog]
            gl = list(glog)
            if is_dist:
                assert rl == ["choice", "rand"], rl
                out[pre + "u_acc"] = rlog[1][1]
                seq = [k for k, _ in pl if k != "swap_idx"]
                assert seq == ["dist", "q", "factors", "logp", "logl", "keep", "x_after", "LP_after"], seq
                d = {k: v for k, v in pl if k != "swap_idx"}
                for k in ("q", "factors", "keep"):
                    out[pre + k] = d[k]
                out[pre + "logp"], out[pre + "logl"] = d["logp"].reshape(T, W), d["logl"].reshape(T, W)
                out[pre + "x_move"] = d["x_after"]
                out[pre + "L_move"], out[pre + "P_move"] = (v.reshape(T, W) for v in d["LP_after"])
            else:
                assert rl == ["choice"] + ["randint", "rand", "rand"] * 2, rl
                for sp in range(2):
                    out[pre + f"rint{sp}"], out[pre + f"u_zz{sp}"], out[pre + f"u_acc{sp}"] = (rlog[j + 3 * sp][1] for j in (1, 2, 3))
                assert [k for k, _ in gl[:T]] == ["shuffle"] * T
                out[pre + "labels"] = np.stack([v for k, v in gl[:T]])
                gl = gl[T:]
                blocks = [i for i, (k, _) in enumerate(pl) if k == "stretch"]
                assert len(blocks) == 2
                for sp, b in enumerate(blocks):
                    blk = dict(pl[b + 1:b + 9])
                    out[pre + f"keep{sp}"] = blk["keep"]          # (a stretch iteration's intermediates: tests/golden/priors/ has them)
                    out[pre + f"S{sp}"] = blk["subset"]
                last = dict(pl[blocks[1] + 1:blocks[1] + 9])
                out[pre + "x_move"] = last["x_after"]
                out[pre + "L_move"], out[pre + "P_move"] = last["LP_after"]
            rlog.clear()
            glog.clear()
            if tc is not None:
                assert [k for k, _ in gl] == ["permutation", "permutation", "uniform"] * (T - 1), gl
                out[pre + "iperm"] = np.stack([gl[3 * j][1] for j in range(T - 1)])
                out[pre + "i1perm"] = np.stack([gl[3 * j + 1][1] for j in range(T - 1)])
                out[pre + "u_swap"] = np.stack([gl[3 * j + 2][1] for j in range(T - 1)])
                swaps = [v for k, v in pl if k == "swap_idx"]
                assert len(swaps) == T - 1
                sel = np.zeros((T - 1, W), dtype=bool)
                for j, (i, a_, b_) in enumerate(swaps):
                    assert i == T - 1 - j
                    m = np.isin(out[pre + "iperm"][j], a_)
                    assert np.array_equal(out[pre + "iperm"][j][m], a_) and np.array_equal(out[pre + "i1perm"][j][m], b_)
                    sel[j] = m
                out[pre + "sel"] = sel
                out[pre + "swaps_accepted"] = np.array(tc.swaps_accepted, copy=True)
                out[pre + "betas"] = np.array(tc.betas, copy=True)
            else:
                assert not gl, gl
            out[pre + "x"] = state.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D).copy()
            out[pre + "L"], out[pre + "P"] = state.log_like.reshape(T, W).copy(), state.log_prior.reshape(T, W).copy()
            it += 1
        out["kind"] = np.array(kinds)
        out["accepted_dist"] = np.array(dist_move.accepted, copy=True).reshape(T, W)
        out["num_proposals_dist"] = int(dist_move.num_proposals)
        if mix:
            out["accepted_stretch"] = np.array(s.moves[0].accepted, copy=True)
    finally:
        np.random.shuffle, np.random.permutation, np.random.uniform = orig_shuffle, orig_perm, orig_unif
    its = [i for i in range(nsteps) if kinds[i]]
    n_inf = sum(int(np.isinf(out[f'it{i}_logp']).sum()) for i in its)
    n_out = sum(int(np.isneginf(out[f'it{i}_factors']).sum()) for i in its)
    # one array per quantity, stacked over the iterations that have it (an archive entry per iteration and quantity costs more than
    # the numbers in it): "all_<k>"[it] for what every iteration records, "dist_<k>"[j] / "stretch_<k>"[j] for the j-th iteration
    # of that kind (tests/dist_move.fixture_iteration undoes it)
    per = {}
    for key in [k for k in out if k.startswith("it") and "_" in k and k[2:k.index("_")].isdigit()]:
        per.setdefault(key[key.index("_") + 1:], {})[int(key[2:key.index("_")])] = out.pop(key)
    for k, by_it in per.items():
        have = sorted(by_it)
        group = "all" if have == list(range(nsteps)) else "dist" if have == its else "stretch"
        assert group != "stretch" or have == [i for i in range(nsteps) if not kinds[i]], (k, have)
        out[f"{group}_{k}"] = np.stack([by_it[i] for i in have])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; {len(its)} move iterations of {nsteps}; accepted per rung "
          f"{out['accepted_dist'].sum(axis=1).tolist()}; -inf prior {n_inf}; old points outside the generator {n_out}")


if __name__ == "__main__":
    T, W = 3, 10
    mu1 = np.array([0.1, 0.5, -0.2, 2.0])
    x1 = mu1 + 0.5 * np.random.RandomState(1).randn(T, W, 4)             # make_golden_priors.py's start
    x1[..., 0] = np.clip(x1[..., 0], -1.9, 2.4)
    x1[..., 1] = np.clip(x1[..., 1], 2e-3, 2.9)
    x1[..., 3] = np.clip(x1[..., 3], 1e-2, 7.9)
    capture("dg1_mix", T, W, (mgp.KINDS, mgp.P0, mgp.P1), GEN1, True, 12, mu1, x1)
    mu2 = np.array([0.3, 1.0, -1.2])
    x2 = np.random.RandomState(2).uniform(BOX2[1], BOX2[2], size=(1, 16, 3))
    capture("dg2_prior_draws", 1, 16, BOX2, BOX2, False, 10, mu2, x2)
    mu3 = np.array([1.0, 0.5, 1.5, 2.0])
    x3 = np.random.RandomState(3).uniform(BOX3[1] + 0.05 * (BOX3[2] - BOX3[1]), BOX3[2] - 0.05 * (BOX3[2] - BOX3[1]), size=(3, 16, 4))
    capture("dg3_periodic_mix", 3, 16, BOX3, GEN3, True, 16, mu3, x3, periodic=PERIOD3)
