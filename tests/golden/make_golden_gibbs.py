#!/usr/bin/env python
"""Generate tests/golden/gibbs/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gibbs.py        (GOLDEN_OUT=<dir>: write there instead)

``gibbs_sampling_setup`` on ``eryn.moves.StretchMove`` and ``GaussianMove`` (move.py:113-221 under red_blue.py:119-333 and
mh.py:79-193), T = 3 rungs with parallel tempering and ladder adaptation, 6 steps, every draw recorded:

  g1_stretch_blocks   W = 12, D = 4, box prior; StretchMove, blocks {0, 1}, {2}: coordinate 3 never moves
  g2_gauss_blocks     W = 14, D = 5, box prior; GaussianMove(0.05), blocks {0, 1, 2}, {3, 4}
  g3_mix_overlap      W = 21, D = 6, box prior; [(StretchMove, 0.5), (GaussianMove, 0.5)], overlapping blocks - stretch {0, 1, 2},
                      {2, 3}, Gaussian {1, 4}, {0} - and coordinate 5 in no block of either move
  g4_stretch_terms    W = 12, D = 4, make_golden_priors.py's uniform / log-uniform / normal container; StretchMove, blocks {0, 1},
                      {1, 2, 3}: the log-uniform coordinate 3 is frozen in one block and moves in the other

Keys.  Set-up: T, W, D, nsteps, seeds, mu, invcov, x0, L0, P0, betas0, prior_kind / prior_p0 / prior_p1 (the arguments of the
reference's constructors: 0 uniform_dist, 1 log_uniform, 2 scipy.stats.norm), masks_stretch / masks_gauss [nblocks, D] (absent: the
move is not there), a, cov.  Iteration i: it<i>_kind (0 stretch, 1 Gaussian); a stretch iteration's it<i>_labels [T, W] (one
labelling for all blocks) and per block b and split s it<i>_b<b>_rint<s> / _uzz<s> / _uacc<s> / _keep<s>; a Gaussian iteration's
it<i>_b<b>_z (the randn call's output [T W, D]) / _uacc / _keep; it<i>_accepted - what propose() returned (the running OR over the
blocks for the stretch move, the LAST block's mask for the Gaussian move); it<i>_x_move / _L_move / _P_move after the last block;
the sweep's it<i>_iperm / _i1perm / _u_swap / _swaps_accepted / _betas; it<i>_x / _L / _P after the sweep.  End: accepted_stretch /
accepted_gauss, num_proposals_stretch / num_proposals_gauss (the moves' own books).
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
from eryn.moves import GaussianMove, StretchMove  # noqa: E402
from eryn.prior import ProbDistContainer, log_uniform, uniform_dist  # noqa: E402

OUT = os.environ.get("GOLDEN_OUT", os.path.join(HERE, "gibbs"))


class RLog:
    """Recording proxy around the sampler-owned RandomState: every call the two moves make."""

    def __init__(self, rs, log):
        self._rs, self._log = rs, log

    def __getattr__(self, name):
        fn = getattr(self._rs, name)
        if name not in ("choice", "randint", "rand", "randn"):
            return fn

        def call(*a, **k):
            out = fn(*a, **k)
            self._log.append((name, None if name == "choice" else np.array(out, copy=True)))
            return out
        return call


def container(kinds, p0, p1):
    make = {0: uniform_dist, 1: log_uniform, 2: stats.norm}
    return ProbDistContainer({d: make[int(kinds[d])](float(p0[d]), float(p1[d])) for d in range(len(kinds))})


def setup_of(masks):
    return [("model_0", np.asarray(m, dtype=bool)[None, :]) for m in masks]


def capture(name, W, prior, mu, x0, masks_stretch=None, masks_gauss=None, cov=0.05, nsteps=6, T=3, seed_construct=123, seed_run=456):
    D = len(prior[0])
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    invcov = np.linalg.inv(A @ A.T / D + np.eye(D))
    np.random.seed(seed_construct)
    st = None if masks_stretch is None else StretchMove(gibbs_sampling_setup=setup_of(masks_stretch), live_dangerously=True)
    ga = None if masks_gauss is None else GaussianMove({"model_0": cov}, gibbs_sampling_setup=setup_of(masks_gauss))
    moves = [(m, 0.5) for m in (st, ga)] if st is not None and ga is not None else (st if st is not None else ga)
    s = EnsembleSampler(W, D, mg.log_like_vec, container(*prior), args=[mu, invcov], vectorize=True, moves=moves,
                        tempering_kwargs=dict(ntemps=T))
    rlog, glog, plog = [], [], []
    s._random = RLog(s._random, rlog)
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

    def hook_move(move):
        orig_update, orig_propose = move.update, move.propose

        def update(old_state, new_state, accepted, subset=None):
            plog.append(("keep", (accepted if subset is None else np.take_along_axis(accepted, subset, axis=1)).copy()))
            out = orig_update(old_state, new_state, accepted, subset=subset)
            plog.append(("after", (out.branches["model_0"].coords[:, :, 0, :].copy(), out.log_like.copy(), out.log_prior.copy())))
            return out

        def propose(model, state):
            new_state, accepted = orig_propose(model, state)
            plog.append(("accepted", np.array(accepted, copy=True)))
            return new_state, accepted

        move.update, move.propose = update, propose

    for m in s.moves:
        hook_move(m)
    out = dict(T=T, W=W, D=D, nsteps=nsteps, seed_construct=seed_construct, seed_run=seed_run, mu=mu, invcov=invcov, x0=x0,
               prior_kind=prior[0], prior_p0=prior[1], prior_p1=prior[2], cov=float(cov), betas0=np.array(tc.betas, copy=True))
    if st is not None:
        out["masks_stretch"], out["a"] = np.asarray(masks_stretch, dtype=bool), float(st.a)
    if ga is not None:
        out["masks_gauss"] = np.asarray(masks_gauss, dtype=bool)
    assert bool(tc.adaptive) and bool(tc.permute)
    np.random.seed(seed_run)
    np.random.shuffle, np.random.permutation, np.random.uniform = shuffle, permutation, uniform
    try:
        it = 0
        for state in s.sample(x0, iterations=nsteps, store=False):
            pre = f"it{it}_"
            pl, rl, gl = list(plog), list(rlog), list(glog)
            plog.clear(), rlog.clear(), glog.clear()
            if it == 0:                     # the initial evaluation: logp, then logl of x0 (ensemble.py:898-912)
                assert pl[0][0] == "logp" and pl[1][0] == "logl"
                out["P0"], out["L0"] = pl[0][1].reshape(T, W), pl[1][1].reshape(T, W)
                pl = pl[2:]
            assert rl[0][0] == "choice"
            rl = rl[1:]
            is_gauss = rl[0][0] == "randn"
            out[pre + "kind"] = int(is_gauss)
            keeps = [v for k, v in pl if k == "keep"]
            if is_gauss:
                nb = len(masks_gauss)
                assert [k for k, _ in rl] == ["randn", "rand"] * nb and len(keeps) == nb, [k for k, _ in rl]
                for b in range(nb):
                    out[pre + f"b{b}_z"], out[pre + f"b{b}_uacc"], out[pre + f"b{b}_keep"] = rl[2 * b][1], rl[2 * b + 1][1], keeps[b]
            else:
                nb = len(masks_stretch)
                assert [k for k, _ in rl] == ["randint", "rand", "rand"] * (2 * nb) and len(keeps) == 2 * nb, [k for k, _ in rl]
                assert [k for k, _ in gl[:T]] == ["shuffle"] * T
                out[pre + "labels"] = np.stack([v for _, v in gl[:T]])
                gl = gl[T:]
                for b in range(nb):
                    for sp in range(2):
                        j = 3 * (2 * b + sp)
                        out[pre + f"b{b}_rint{sp}"], out[pre + f"b{b}_uzz{sp}"], out[pre + f"b{b}_uacc{sp}"] = rl[j][1], rl[j + 1][1], rl[j + 2][1]
                        out[pre + f"b{b}_keep{sp}"] = keeps[2 * b + sp]
            after = [v for k, v in pl if k == "after"][-1]
            out[pre + "x_move"], out[pre + "L_move"], out[pre + "P_move"] = after[0], after[1].reshape(T, W), after[2].reshape(T, W)
            out[pre + "accepted"] = [v for k, v in pl if k == "accepted"][-1]
            assert [k for k, _ in gl] == ["permutation", "permutation", "uniform"] * (T - 1), [k for k, _ in gl]
            out[pre + "iperm"] = np.stack([gl[3 * j][1] for j in range(T - 1)])
            out[pre + "i1perm"] = np.stack([gl[3 * j + 1][1] for j in range(T - 1)])
            out[pre + "u_swap"] = np.stack([gl[3 * j + 2][1] for j in range(T - 1)])
            out[pre + "swaps_accepted"] = np.array(tc.swaps_accepted, copy=True)
            out[pre + "betas"] = np.array(tc.betas, copy=True)
            out[pre + "x"] = state.branches["model_0"].coords[:, :, 0, :].reshape(T, W, D).copy()
            out[pre + "L"], out[pre + "P"] = state.log_like.reshape(T, W).copy(), state.log_prior.reshape(T, W).copy()
            it += 1
        for tag, m in (("stretch", st), ("gauss", ga)):
            if m is not None:
                out["accepted_" + tag] = np.array(m.accepted, copy=True).reshape(T, W)
                out["num_proposals_" + tag] = int(m.num_proposals)
    finally:
        np.random.shuffle, np.random.permutation, np.random.uniform = orig_shuffle, orig_perm, orig_unif
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    books = {k: (int(out["num_proposals_" + k]), float(out["accepted_" + k].max())) for k in ("stretch", "gauss") if "accepted_" + k in out}
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; kinds {[int(out[f'it{i}_kind']) for i in range(nsteps)]}; (num_proposals, max accepted) {books}")


def box(D, half):
    return np.zeros(D, dtype=int), np.full(D, -half), np.full(D, half)


def mask_of(D, *coords):
    m = np.zeros(D, dtype=bool)
    m[list(coords)] = True
    return m


if __name__ == "__main__":
    T = 3
    for name, W, D, kw in (("g1_stretch_blocks", 12, 4, dict(masks_stretch=[mask_of(4, 0, 1), mask_of(4, 2)])),
                           ("g2_gauss_blocks", 14, 5, dict(masks_gauss=[mask_of(5, 0, 1, 2), mask_of(5, 3, 4)])),
                           ("g3_mix_overlap", 21, 6, dict(masks_stretch=[mask_of(6, 0, 1, 2), mask_of(6, 2, 3)],
                                                          masks_gauss=[mask_of(6, 1, 4), mask_of(6, 0)]))):
        mu = 0.1 * np.random.RandomState(10 + D).randn(D)
        x0 = mu + 0.8 * np.random.RandomState(20 + D).randn(T, W, D)
        capture(name, W, box(D, 2.5), mu, np.clip(x0, -2.4, 2.4), **kw)
    mu4 = np.array([0.1, 0.5, -0.2, 2.0])
    x4 = mu4 + 0.5 * np.random.RandomState(1).randn(T, 12, 4)            # make_golden_priors.py's start
    x4[..., 0] = np.clip(x4[..., 0], -1.9, 2.4)
    x4[..., 1] = np.clip(x4[..., 1], 2e-3, 2.9)
    x4[..., 3] = np.clip(x4[..., 3], 1e-2, 7.9)
    capture("g4_stretch_terms", 12, (mgp.KINDS, mgp.P0, mgp.P1), mu4, x4, masks_stretch=[mask_of(4, 0, 1), mask_of(4, 1, 2, 3)])
