#!/usr/bin/env python
"""Generate tests/golden/priors/p1_priors.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_priors.py

The stretch move with parallel tempering and ladder adaptation (make_golden.py's capture points, its R proxy and its likelihood)
under a ``ProbDistContainer`` of mixed per-parameter priors - T = 3, W = 10, D = 4:

    0  uniform_dist(-2.0, 2.5)           1  log_uniform(1e-3, 3.0)   (the reference builds scipy.stats.loguniform(min, max - min))
    2  scipy.stats.norm(-0.6, 0.8)       3  log_uniform(5e-3, 8.0)

Every draw of both streams and every intermediate of six iterations is recorded; the priors travel as the ARGUMENTS of the calls
above (``prior_kind``: 0 uniform_dist, 1 log_uniform, 2 norm; ``prior_p0`` / ``prior_p1``).  The fixture lives in a directory of its
own: tests/test_golden_regeneration.py holds the fixtures directly under tests/golden/ to the four generators it knows.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402  (sets up the reference's import path; nothing runs on import)

import numpy as np                          # noqa: E402
from scipy import stats                     # noqa: E402
from eryn.ensemble import EnsembleSampler   # noqa: E402
from eryn.prior import ProbDistContainer, log_uniform, uniform_dist  # noqa: E402

OUT = os.path.join(HERE, "priors")
KINDS = np.array([0, 1, 2, 1])
P0 = np.array([-2.0, 1e-3, -0.6, 5e-3])
P1 = np.array([2.5, 3.0, 0.8, 8.0])


def make_priors():
    make = {0: uniform_dist, 1: log_uniform, 2: stats.norm}
    return ProbDistContainer({d: make[int(KINDS[d])](float(P0[d]), float(P1[d])) for d in range(len(KINDS))})


def capture(name, T=3, W=10, nsteps=6, seed_construct=123, seed_run=456):
    D = len(KINDS)
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    mu = np.array([0.1, 0.5, -0.2, 2.0])                       # inside every support
    invcov = np.linalg.inv(A @ A.T / D + np.eye(D))
    np.random.seed(seed_construct)
    s = EnsembleSampler(W, D, mg.log_like_vec, make_priors(), args=[mu, invcov], vectorize=True, tempering_kwargs=dict(ntemps=T))
    x0 = mu + 0.5 * np.random.RandomState(1).randn(T, W, D)
    x0[..., 0] = np.clip(x0[..., 0], -1.9, 2.4)
    x0[..., 1] = np.clip(x0[..., 1], 2e-3, 2.9)
    x0[..., 3] = np.clip(x0[..., 3], 1e-2, 7.9)

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

    move, tc = s.moves[0], s.temperature_control
    orig_get_proposal, orig_update = move.get_proposal, move.update
    orig_lp, orig_ll = s.compute_log_prior, s.compute_log_like
    orig_tc, orig_dsi = tc.temper_comps, tc.do_swaps_indexing

    def get_proposal(s_all, c_all, random, **k):
        q, factors = orig_get_proposal(s_all, c_all, random, **k)
        plog.append(("q", q["model_0"][:, :, 0, :].copy()))
        plog.append(("factors", factors.copy()))
        return q, factors

    def compute_log_prior(coords, **k):
        out = orig_lp(coords, **k)
        plog.append(("logp", out.copy()))
        return out

    def compute_log_like(coords, **k):
        out = orig_ll(coords, **k)
        plog.append(("logl", out[0].copy()))
        return out

    def update(old_state, new_state, accepted, subset=None):
        plog.append(("keep", np.take_along_axis(accepted, subset, axis=1).copy()))
        plog.append(("subset", subset.copy()))
        out = orig_update(old_state, new_state, accepted, subset=subset)
        plog.append(("x_after_split", out.branches["model_0"].coords[:, :, 0, :].copy()))
        return out

    def temper_comps(state, **k):
        plog.append(("pre_pt", (state.branches["model_0"].coords[:, :, 0, :].copy(), state.log_like.copy(), state.log_prior.copy())))
        return orig_tc(state, **k)

    def do_swaps_indexing(i, iperm_sel, i1perm_sel, *a, **k):
        plog.append(("swap_idx", (i, iperm_sel.copy(), i1perm_sel.copy())))
        return orig_dsi(i, iperm_sel, i1perm_sel, *a, **k)

    move.get_proposal, move.update = get_proposal, update
    s.compute_log_prior, s.compute_log_like = compute_log_prior, compute_log_like
    tc.temper_comps, tc.do_swaps_indexing = temper_comps, do_swaps_indexing

    out = dict(T=T, W=W, D=D, nsteps=nsteps, seed_construct=seed_construct, seed_run=seed_run, mu=mu, invcov=invcov, x0=x0,
               a=float(move.a), prior_kind=KINDS, prior_p0=P0, prior_p1=P1, betas0=np.array(tc.betas, copy=True))
    assert bool(tc.adaptive) and bool(tc.permute)
    np.random.seed(seed_run)
    np.random.shuffle, np.random.permutation, np.random.uniform = shuffle, permutation, uniform
    try:
        it = 0
        for state in s.sample(x0, iterations=nsteps, store=False):
            pre = f"it{it}_"
            assert [k for k, _ in rlog] == ["choice"] + ["randint", "rand", "rand"] * 2, rlog
            for sp in range(2):
                out[pre + f"rint{sp}"], out[pre + f"u_zz{sp}"], out[pre + f"u_acc{sp}"] = (rlog[j + 3 * sp][1] for j in (1, 2, 3))
            rlog.clear()
            assert [k for k, _ in glog] == ["shuffle"] * T + ["permutation", "permutation", "uniform"] * (T - 1), glog
            out[pre + "labels"] = np.stack([v for k, v in glog[:T]])
            rest = glog[T:]
            out[pre + "iperm"] = np.stack([rest[3 * j][1] for j in range(T - 1)])
            out[pre + "i1perm"] = np.stack([rest[3 * j + 1][1] for j in range(T - 1)])
            out[pre + "u_swap"] = np.stack([rest[3 * j + 2][1] for j in range(T - 1)])
            glog.clear()
            pl = list(plog)
            plog.clear()
            if it == 0:                     # the initial evaluation: logp, then logl of x0 (ensemble.py:898-912)
                assert pl[0][0] == "logp" and pl[1][0] == "logl"
                out["P0"], out["L0"] = pl[0][1], pl[1][1]
                pl = pl[2:]
            per_split = ["q", "factors", "logp", "logl", "keep", "subset", "x_after_split"]
            assert [k for k, _ in pl][:15] == per_split * 2 + ["pre_pt"], [k for k, _ in pl]
            for sp in range(2):
                blk = dict(pl[7 * sp:7 * sp + 7])
                for k in ("q", "factors", "logp", "logl", "keep"):
                    out[pre + f"{k}{sp}"] = blk[k]
                out[pre + f"S{sp}"] = blk["subset"]
            out[pre + "x_stretch"], out[pre + "L_stretch"], out[pre + "P_stretch"] = pl[14][1]
            swaps = pl[15:]
            assert all(k == "swap_idx" for k, _ in swaps) and len(swaps) == T - 1
            sel = np.zeros((T - 1, W), dtype=bool)
            for j, (_, (i, a_, b_)) in enumerate(swaps):
                assert i == T - 1 - j
                m = np.isin(out[pre + "iperm"][j], a_)
                assert np.array_equal(out[pre + "iperm"][j][m], a_) and np.array_equal(out[pre + "i1perm"][j][m], b_)
                sel[j] = m
            out[pre + "sel"] = sel
            out[pre + "swaps_accepted"] = np.array(tc.swaps_accepted, copy=True)
            out[pre + "betas"] = np.array(tc.betas, copy=True)
            out[pre + "x"] = state.branches["model_0"].coords[:, :, 0, :].copy()
            out[pre + "L"], out[pre + "P"] = state.log_like.copy(), state.log_prior.copy()
            it += 1
        out["accepted_total"] = np.array(move.accepted, copy=True)
        out["num_proposals"] = int(move.num_proposals)
    finally:
        np.random.shuffle, np.random.permutation, np.random.uniform = orig_shuffle, orig_perm, orig_unif
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    n_inf = sum(int(np.isinf(out[f"it{i}_logp{sp}"]).sum()) for i in range(nsteps) for sp in (0, 1))
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB, mean accept {out['accepted_total'].mean() / nsteps:.3f}, "
          f"{n_inf} proposals outside a support")


if __name__ == "__main__":
    capture("p1_priors")
