#!/usr/bin/env python
"""Generate tests/golden/mt/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_mt.py        (GOLDEN_OUT=<dir>: write there instead)

``eryn.moves.MTDistGenMove(container, num_try=K, independent=True)`` (mtdistgen.py:7-136 over multipletry.py:238-514 under
mh.py:56-193) with make_golden_dist.py's capture technique (the R proxy and the likelihood of make_golden.py, the global stream's
calls wrapped, the moves' and the sampler's methods hooked):

  mt1_mix          T = 3, W = 10, D = 4, K = 5, 12 iterations of [(StretchMove, 0.5), (MTDistGenMove, 0.5)] with parallel tempering
                   and ladder adaptation; dg1_mix's prior and generator (mixed kinds; old points outside the generator, for which
                   the reference's log-sum-exp is NaN).
  mt2_prior_tries  T = 2, W = 16, D = 3, K = 25, the move alone, generator = the all-uniform prior.
  mt3_periodic_mix dg3_periodic_mix's problem with [(StretchMove(periodic=pc), 0.5), (MTDistGenMove(num_try=4, periodic=pc), 0.5)]: the
                   stretch move wraps, the tries and the picked point never are (multipletry.py holds no wrap).

Every iteration records which move ran (``kind``: 0 stretch, 1 the move), its draws of the sampler's stream R, the state after the
move and after the sweep, the sweep's draws, swap counts and ladder; a move iteration its tries ``q`` [T, W, K, D] (the ONE ``rvs``
on the global stream G), the pick uniforms ``u_pick`` (the ONE ``np.random.rand`` on G after it), the picks, ``lsw``, ``aux_lsw``,
``factors``, ``mt_ll``, ``mt_lp`` and the accept mask.  Distributions travel as make_golden_dist.py's do.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402  (sets up the reference's import path; nothing runs on import)
import make_golden_priors as mgp            # noqa: E402
import make_golden_dist as mgd              # noqa: E402

import numpy as np                          # noqa: E402
import eryn.moves.multipletry as mtry       # noqa: E402
from eryn.ensemble import EnsembleSampler   # noqa: E402
from eryn.moves import MTDistGenMove, StretchMove  # noqa: E402

OUT = os.environ.get("GOLDEN_OUT", os.path.join(HERE, "mt"))


def capture(name, T, W, prior, gen, K, mix, nsteps, mu, x0, seed_construct=123, seed_run=456, periodic=None):
    D = len(prior[0])
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    invcov = np.linalg.inv(A @ A.T / D + np.eye(D))
    np.random.seed(seed_construct)
    pc = mgd.periodic_container(periodic)
    kw = {} if pc is None else dict(periodic=pc)
    mt_move = MTDistGenMove(mgd.container(*gen), num_try=K, independent=True, **kw)
    moves = [(StretchMove(**kw), 0.5), (mt_move, 0.5)] if mix else mt_move
    s = EnsembleSampler(W, D, mg.log_like_vec, mgd.container(*prior), args=[mu, invcov], vectorize=True, moves=moves,
                        tempering_kwargs=dict(ntemps=T))
    rlog, glog, plog = [], [], []
    s._random = mg.RProxy(s._random, rlog)
    orig_shuffle, orig_perm, orig_unif, orig_rand = np.random.shuffle, np.random.permutation, np.random.uniform, np.random.rand
    orig_comp = mtry.get_mt_computations

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

    def get_mt_computations(logP, log_proposal_pdf, **k):          # multipletry.py:36-59: the one np.random.rand in it is the pick's
        picks = []

        def rand(*a):
            picks.append(orig_rand(*a))
            return picks[-1]

        np.random.rand = rand
        try:
            w, lsw, inds = orig_comp(logP, log_proposal_pdf, **k)
        finally:
            np.random.rand = orig_rand
        assert len(picks) == 1
        plog.append(("u_pick", picks[0].copy()))
        plog.append(("pick", np.array(inds, copy=True)))
        return w, lsw, inds

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
            plog.append(("factors", np.array(factors, copy=True)))
            if tag == "mt":
                plog.append(("lsw", np.array(move.log_sum_weights, copy=True)))
                plog.append(("aux_lsw", np.array(move.aux_log_sum_weights, copy=True)))
                plog.append(("mt_ll", np.array(move.mt_ll, copy=True)))
                plog.append(("mt_lp", np.array(move.mt_lp, copy=True)))
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

    for m, tag in zip(s.moves, ("stretch", "mt") if mix else ("mt",)):
        hook_move(m, tag)
    orig_gen = mt_move.special_generate_func

    def special_generate_func(coords, random, **k):                 # mtdistgen.py:41-81: the tries and their log-densities
        pts, lq = orig_gen(coords, random, **k)
        plog.append(("q", np.array(pts, copy=True)))
        return pts, lq

    mt_move.special_generate_func = special_generate_func
    orig_dsi = tc.do_swaps_indexing

    def do_swaps_indexing(i, iperm_sel, i1perm_sel, *a, **k):
        plog.append(("swap_idx", (i, iperm_sel.copy(), i1perm_sel.copy())))
        return orig_dsi(i, iperm_sel, i1perm_sel, *a, **k)

    tc.do_swaps_indexing = do_swaps_indexing

    out = dict(T=T, W=W, D=D, K=K, nsteps=nsteps, seed_construct=seed_construct, seed_run=seed_run, mu=mu, invcov=invcov, x0=x0,
               prior_kind=prior[0], prior_p0=prior[1], prior_p1=prior[2], gen_kind=gen[0], gen_p0=gen[1], gen_p1=gen[2], mix=int(mix))
    if mix:
        out["a"] = float(s.moves[0].a)
    if periodic is not None:
        out["period"] = np.array([float(periodic.get(d, 0.0)) for d in range(D)])
        assert all(m.periodic is pc for m in s.moves)
    out["betas0"] = np.array(tc.betas, copy=True)
    assert bool(tc.adaptive) and bool(tc.permute)
    kinds = []
    np.random.seed(seed_run)
    np.random.shuffle, np.random.permutation, np.random.uniform = shuffle, permutation, uniform
    mtry.get_mt_computations = get_mt_computations
    try:
        it = 0
        for state in s.sample(x0, iterations=nsteps, store=False):
            pre = f"it{it}_"
            pl = list(plog)
            plog.clear()
            if it == 0:                     # the initial evaluation: logp, then logl of x0 (ensemble.py:898-912)
                assert pl[0][0] == "logp" and pl[1][0] == "logl"
                out["P0"], out["L0"] = pl[0][1].reshape(T, W), pl[1][1].reshape(T, W)
                pl = pl[2:]
            is_mt = any(k == "mt" for k, _ in pl)
            kinds.append(int(is_mt))
            rl = [k for k, _ in rlog]
            gl = list(glog)
            if is_mt:
                assert rl == ["choice", "rand"], rl
                out[pre + "u_acc"] = rlog[1][1]
                seq = [k for k, _ in pl if k != "swap_idx"]
                # (the likelihood call evaluates the tries' prior itself, multipletry.py:334; the move then asks for it, :344)
                assert seq == ["q", "logp", "logl", "logp", "u_pick", "pick", "mt", "factors", "lsw", "aux_lsw", "mt_ll", "mt_lp", "keep",
                               "x_after", "LP_after"], seq
                d = {k: v for k, v in pl if k != "swap_idx"}
                out[pre + "q"] = d["q"].reshape(T, W, K, D)
                out[pre + "tries_logl"], out[pre + "tries_logp"] = d["logl"].reshape(T, W, K), d["logp"].reshape(T, W, K)
                for k in ("u_pick", "pick", "lsw", "aux_lsw", "mt_ll", "mt_lp", "factors"):
                    out[pre + k] = np.asarray(d[k]).reshape(T, W)
                out[pre + "keep"] = d["keep"]
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
                    blk = dict(pl[b + 1:b + 8])
                    out[pre + f"keep{sp}"] = blk["keep"]
                    out[pre + f"S{sp}"] = blk["subset"]
                last = dict(pl[blocks[1] + 1:blocks[1] + 8])
                out[pre + "x_move"] = last["x_after"]
                out[pre + "L_move"], out[pre + "P_move"] = last["LP_after"]
            rlog.clear()
            glog.clear()
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
            out[pre + "x"] = state.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D).copy()
            out[pre + "L"], out[pre + "P"] = state.log_like.reshape(T, W).copy(), state.log_prior.reshape(T, W).copy()
            it += 1
        out["kind"] = np.array(kinds)
        out["accepted_mt"] = np.array(mt_move.accepted, copy=True).reshape(T, W)
        out["num_proposals_mt"] = int(mt_move.num_proposals)
        if mix:
            out["accepted_stretch"] = np.array(s.moves[0].accepted, copy=True)
    finally:
        np.random.shuffle, np.random.permutation, np.random.uniform = orig_shuffle, orig_perm, orig_unif
        mtry.get_mt_computations = orig_comp
    its = [i for i in range(nsteps) if kinds[i]]
    n_inf = sum(int(np.isinf(out[f'it{i}_tries_logp']).sum()) for i in its)
    n_nan = sum(int(np.isnan(out[f'it{i}_aux_lsw']).sum()) for i in its)
    n_pick = sum(int((out[f'it{i}_pick'] != 0).sum()) for i in its)
    # one array per quantity, stacked over the iterations that have it ("all_<k>"[it]; "mt_<k>"[j] / "stretch_<k>"[j] for the j-th
    # iteration of that kind: tests/mt_move.fixture_iteration undoes it)
    per = {}
    for key in [k for k in out if k.startswith("it") and "_" in k and k[2:k.index("_")].isdigit()]:
        per.setdefault(key[key.index("_") + 1:], {})[int(key[2:key.index("_")])] = out.pop(key)
    for k, by_it in per.items():
        have = sorted(by_it)
        group = "all" if have == list(range(nsteps)) else "mt" if have == its else "stretch"
        assert group != "stretch" or have == [i for i in range(nsteps) if not kinds[i]], (k, have)
        out[f"{group}_{k}"] = np.stack([by_it[i] for i in have])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; {len(its)} move iterations of {nsteps}; accepted per rung "
          f"{out['accepted_mt'].sum(axis=1).tolist()}; -inf-prior tries {n_inf}; NaN aux_lsw (old points outside the generator) {n_nan}; "
          f"picks other than try 0 {n_pick}")


if __name__ == "__main__":
    T, W = 3, 10
    mu1 = np.array([0.1, 0.5, -0.2, 2.0])
    x1 = mu1 + 0.5 * np.random.RandomState(1).randn(T, W, 4)             # make_golden_dist.py's start
    x1[..., 0] = np.clip(x1[..., 0], -1.9, 2.4)
    x1[..., 1] = np.clip(x1[..., 1], 2e-3, 2.9)
    x1[..., 3] = np.clip(x1[..., 3], 1e-2, 7.9)
    capture("mt1_mix", T, W, (mgp.KINDS, mgp.P0, mgp.P1), mgd.GEN1, 5, True, 12, mu1, x1)
    mu2 = np.array([0.3, 1.0, -1.2])
    x2 = np.random.RandomState(2).uniform(mgd.BOX2[1], mgd.BOX2[2], size=(2, 16, 3))
    capture("mt2_prior_tries", 2, 16, mgd.BOX2, mgd.BOX2, 25, False, 10, mu2, x2)
    mu3 = np.array([1.0, 0.5, 1.5, 2.0])                                  # make_golden_dist.py's dg3_periodic_mix
    x3 = np.random.RandomState(3).uniform(mgd.BOX3[1] + 0.05 * (mgd.BOX3[2] - mgd.BOX3[1]), mgd.BOX3[2] - 0.05 * (mgd.BOX3[2] - mgd.BOX3[1]), size=(3, 16, 4))
    capture("mt3_periodic_mix", 3, 16, mgd.BOX3, mgd.GEN3, 4, True, 16, mu3, x3, periodic=mgd.PERIOD3)
