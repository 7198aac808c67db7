#!/usr/bin/env python
"""Generate tests/golden/rj_gibbs/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rj_gibbs.py

make_golden_rj.py's model and capture technique - the reference's ``EnsembleSampler`` on pulses + sines, every move's ``propose``
wrapped - with ``GaussianMove(cov, gibbs_sampling_setup=[...])`` as the in-model move: the Gaussian move block after block over
branches and leaf slots (move.py:113-402 under mh.py:79-193).  Recorded per iteration and block: whether the block ran (mh.py:105-107
skips a block without a leaf to move), the steps (the proposal minus the state, on the moved leaves; the proposal itself too), the
accept uniforms, the accept mask and the state behind the block; then the state behind the sweep and behind the reversible-jump move
as in the rj* fixtures.  Data only.

    rjg1  pulses (4 slots) + sines (2 slots), leaves 0 .. max, T = 3, W = 8, 40 data points, three blocks - ("gauss", mask), {"gauss":
          mask, "sine": mask}, "sine" -, rj_moves=True, 6 iterations; the start has one walker without any leaf and one without a
          leaf in block 0's slots
    rjg2  one pulse branch, 4 slots, one block per slot, no reversible jump, T = 2, W = 4, slot 3 dead everywhere (block 3 is skipped:
          num_proposals == 18), one walker with slot 2 dead (fix_logp_gibbs's 0.0 on a walker that holds leaves), 6 iterations
    rjg3  make_golden_rj_priors.py's log-uniform / normal leaf priors, blocks ["gauss", "sine"], "separate_branches", 6 iterations
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # (the repository: tests/rj_gibbs_move.py, tests/rj_prior_terms.py)
OUT = os.path.join(HERE, "rj_gibbs")
os.makedirs(OUT, exist_ok=True)
import make_golden_rj as mgr                # noqa: E402  (sets up the reference's import path; nothing runs on import)

import numpy as np                          # noqa: E402
from scipy import stats                     # noqa: E402
from eryn.ensemble import EnsembleSampler   # noqa: E402
from eryn.moves import GaussianMove         # noqa: E402
from eryn.prior import ProbDistContainer, log_uniform, uniform_dist  # noqa: E402
from eryn.state import State                # noqa: E402

from tests.rj_gibbs_move import fixture_setup            # noqa: E402
from tests.rj_prior_terms import FIXTURE_PRIORS          # noqa: E402


class RecordingRandom:
    """The sampler's RandomState behind a proxy that keeps what ``rand`` returned last (the accept uniforms, mh.py:171)."""

    def __init__(self, rs):
        self._rs, self.last_rand = rs, None

    def rand(self, *a):
        self.last_rand = self._rs.rand(*a)
        return self.last_rand

    def __getattr__(self, k):
        return getattr(self._rs, k)


def capture(name, names, T, W, nl_max, nl_min, nsteps, rj_moves, n_init, seed_run, priors=None, prior_rows=None, cov_factor=1e-3,
            sigma=2.0, ndata=40, init_spread=1e-4, seed_data=42, seed_construct=135, edit_start=None):
    t = np.linspace(-1, 1, ndata)
    inj = {"gauss": np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1], [3.4, 0.0, 0.1], [2.9, 0.3, 0.1]]),
           "sine": np.array([[1.3, 10.1, 1.0], [0.8, 4.6, 1.2]])}
    rs = np.random.RandomState(seed_data)
    y = sigma * rs.randn(ndata)
    y = y + mgr.combine_gaussians(t, inj["gauss"][:n_init[0]])
    if "sine" in names:
        y = y + mgr.combine_sine(t, inj["sine"][:n_init[1]])
    nleaves_max, nleaves_min = dict(zip(names, nl_max)), dict(zip(names, nl_min))
    coords = {k: np.zeros((T, W, nleaves_max[k], 3)) for k in names}
    inds = {k: np.zeros((T, W, nleaves_max[k]), dtype=bool) for k in names}
    for bi, k in enumerate(names):
        for nn in range(n_init[bi]):
            coords[k][:, :, nn] = rs.multivariate_normal(inj[k][nn], np.diag(np.ones(3) * init_spread), size=(T, W))
            inds[k][:, :, nn] = True
    if edit_start is not None:
        edit_start(coords, inds)
    if priors is None:
        boxes = {"gauss": mgr.GAUSS_BOX, "sine": mgr.SINE_BOX}
        priors = {k: {i: uniform_dist(*boxes[k][i]) for i in range(3)} for k in names}
    cov = {k: np.diag(np.ones(3)) * cov_factor for k in names}
    like = mgr.log_like_fn_gauss_and_sine
    if names == ["gauss"]:
        sys.path.insert(0, "/root/reference/tests")
        from test_eryn import log_like_fn_gauss_pulse as like
    setup = fixture_setup(name)
    np.random.seed(seed_construct)          # R := snapshot of G at construction (ensemble.py:604,651-652)
    move = GaussianMove(cov, gibbs_sampling_setup=setup)
    s = EnsembleSampler(W, {k: 3 for k in names}, like, priors, args=[t, y, sigma], tempering_kwargs=dict(ntemps=T),
                        nbranches=len(names), branch_names=names, nleaves_max=nleaves_max, nleaves_min=nleaves_min, moves=move,
                        **({} if rj_moves is None else dict(rj_moves=rj_moves)))
    s._random = rec_random = RecordingRandom(s._random)
    logp0 = s.compute_log_prior(coords, inds=inds)
    logl0 = s.compute_log_like(coords, inds=inds, logp=logp0)[0]
    state = State(coords, log_like=logl0, log_prior=logp0, inds=inds)
    out = dict(T=T, W=W, ndata=ndata, sigma=float(sigma), nsteps=nsteps, t=t, y=y, nl_max=np.array(nl_max), nl_min=np.array(nl_min),
               cov_factor=float(cov_factor), seed_construct=seed_construct, seed_run=seed_run,
               betas0=np.array(s.temperature_control.betas), L0=logl0, P0=logp0,
               rj_moves="none" if rj_moves is None else ("together" if rj_moves is True else rj_moves), in_model="gaussian",
               branch_names=np.array(names), nblocks=len(setup))
    if prior_rows is None:
        for k in names:
            out[f"{k}_box"] = np.array(boxes[k])
    else:
        for k in names:
            out[f"{k}_box"] = np.array([[p0, p1] for _, p0, p1 in prior_rows[k]])
            out[f"{k}_prior_kind"] = np.array([kind for kind, _, _ in prior_rows[k]])
    for k in names:
        out[f"x0_{k}"], out[f"inds0_{k}"] = coords[k].copy(), inds[k].copy()

    log, blocks = [], []
    cur = dict(k=-1, ran=False)

    def snap(st):
        d = {f"x_{k}": st.branches[k].coords.copy() for k in names}
        d.update({f"inds_{k}": st.branches[k].inds.copy() for k in names})
        d.update(L=st.log_like.copy(), P=st.log_prior.copy())
        return d

    # the blocks of the in-model move: setup_proposals opens one (and says whether it runs), update closes it
    orig_setup, orig_update = move.setup_proposals, move.update

    def setup_proposals(branch_names_run, inds_run, branches_coords, branches_inds):
        res = orig_setup(branch_names_run, inds_run, branches_coords, branches_inds)
        cur["k"] += 1
        blocks.append(dict(k=cur["k"], ran=bool(res[2]), before={k: v.copy() for k, v in branches_coords.items()}))
        return res

    def update(old_state, new_state, accepted, subset=None):
        res = orig_update(old_state, new_state, accepted, subset=subset)
        b = blocks[-1]
        b["q"] = {k: new_state.branches[k].coords.copy() for k in names}
        b["u_acc"] = rec_random.last_rand.copy()
        b["keep"] = np.array(accepted, copy=True)
        b["after"] = snap(res)
        return res
    move.setup_proposals, move.update = setup_proposals, update

    def wrap(mv, tag):
        orig = mv.propose

        def propose(model, st):
            if tag == "mh":
                cur["k"] = -1
            new, acc = orig(model, st)
            r = snap(new)
            r.update(tag=tag, accepted=np.array(acc, copy=True), betas=np.array(s.temperature_control.betas),
                     swaps=np.array(s.temperature_control.swaps_accepted))
            log.append(r)
            return new, acc
        mv.propose = propose
    wrap(move, "mh")
    for i, m in enumerate(s.rj_moves if rj_moves is not None else []):
        wrap(m, f"rj{i}")

    np.random.seed(seed_run)                # G for the run
    it = 0
    for st in s.sample(state, iterations=nsteps, store=False):
        assert [r["tag"][:2] for r in log] == (["mh", "rj"] if rj_moves is not None else ["mh"]), [r["tag"] for r in log]
        assert [b["k"] for b in blocks] == list(range(len(setup)))
        for b in blocks:
            pre = f"it{it}_b{b['k']}_"
            out[pre + "ran"] = b["ran"]
            if not b["ran"]:
                continue
            for k in names:
                out[pre + f"q_{k}"] = b["q"][k]
                out[pre + f"step_{k}"] = b["q"][k] - b["before"][k]
            out[pre + "u_acc"], out[pre + "keep"] = b["u_acc"], b["keep"]
            for k, v in b["after"].items():
                out[pre + k] = v
        for r in log:
            pre = f"it{it}_{r['tag'][:2]}_"
            for k, v in r.items():
                if k == "tag":
                    out[pre + "branch"] = int(r["tag"][2:]) if r["tag"].startswith("rj") else -1
                else:
                    out[pre + k] = v
        log.clear()
        blocks.clear()
        it += 1
    out["mh_accepted_total"] = np.array(move.accepted)
    out["mh_num_proposals"] = int(move.num_proposals)
    if rj_moves is not None:
        out["rj_accepted_total"] = np.stack([np.array(m.accepted) for m in s.rj_moves])
        out["rj_num_proposals"] = np.array([m.num_proposals for m in s.rj_moves])
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; num_proposals {move.num_proposals}, in-model accept per proposal "
          f"{out['mh_accepted_total'].mean() / max(move.num_proposals, 1):.2f}")
    return out


def rjg1_start(coords, inds):
    for k in inds:                                    # one walker without any leaf
        inds[k][0, 2] = False
    coords["gauss"][1, 3, 2] = coords["gauss"][1, 3, 0]      # one without a leaf in block 0's slots (0 and 1): its pulse sits in slot 2
    inds["gauss"][1, 3] = [False, False, True, False]


def rjg2_start(coords, inds):
    inds["gauss"][1, 1, 2] = False                    # slot 2 dead on one walker: block 2 finds it without a leaf to move


def container(name):
    make = {0: uniform_dist, 1: log_uniform, 2: stats.norm}
    return ProbDistContainer({d: make[k](p0, p1) for d, (k, p0, p1) in enumerate(FIXTURE_PRIORS[name])})


if __name__ == "__main__":
    capture("rjg1", ["gauss", "sine"], T=3, W=8, nl_max=(4, 2), nl_min=(0, 0), nsteps=6, rj_moves=True, n_init=(2, 1), seed_run=246,
            edit_start=rjg1_start)
    o = capture("rjg2", ["gauss"], T=2, W=4, nl_max=(4,), nl_min=(0,), nsteps=6, rj_moves=None, n_init=(3,), seed_run=77,
                edit_start=rjg2_start)
    assert o["mh_num_proposals"] == 18 and not any(o[f"it{i}_b3_ran"] for i in range(6)), "block 3 is skipped at every iteration"
    capture("rjg3", ["gauss", "sine"], T=3, W=10, nl_max=(3, 4), nl_min=(0, 0), nsteps=6, rj_moves="separate_branches", n_init=(2, 1),
            seed_run=246, priors={k: container(k) for k in ("gauss", "sine")}, prior_rows=FIXTURE_PRIORS)
