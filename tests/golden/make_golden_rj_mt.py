#!/usr/bin/env python
"""Generate tests/golden/rj_mt/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rj_mt.py        (GOLDEN_OUT=<dir>: write there instead)

``eryn.moves.MTDistGenMoveRJ(generate_dist, num_try=K, rj=True)`` (mtdistgenrj.py over multipletry.py:238-514, 597-776, inside
ReversibleJumpMove.propose, rj.py:145-388) as the sampler's ``rj_moves`` beside an in-model ``GaussianMove``, with make_golden_mt.py's
capture technique (the R proxy of make_golden.py, ``get_mt_computations`` wrapped for the pick's one ``np.random.rand``, the move's
methods hooked) on make_golden_rj.py's model and fixture layout:

  rjmt1   the reference's ``test_mt`` in small: ONE pulse branch, T = 3, W = 8, nleaves 0 .. 4, 64 data points, K = 5, generator = prior,
          10 iterations of GaussianMove + the move.
  rjmt2   pulse + sine branches, one move per branch (``gibbs_sampling_setup=<branch>``), K = 7; the pulse generator is WIDER than the
          prior in the amplitude (tries with a -inf prior) and NARROWER in the width (dying leaves outside the generator: NaN factors);
          leaf budgets (3, 2) with a start that puts walkers at both edges.

The reference's ``get_mt_proposal`` cannot run a proposal without a death walker (``inds_reverse_rj = None``): the seeds are such that
every captured proposal has births and deaths (asserted).  Per iteration ``it{i}_mh_*`` / ``it{i}_rj_*`` are make_golden_rj.py's (state,
accept mask, ladder and swap counts behind each move's sweep); the move adds ``it{i}_rj_`` branch, change, leaf, tries [T, W, K, 3] (a death
walker's try 0 is its dying leaf), u_pick, u_acc, pick, lsw, aux_lsw, factors (before the edge factors), mt_ll, mt_lp (before
fix_logp_gibbs), keep, and the state behind the move's update in front of the sweep (``move_x_*``, ``move_inds_*``, ``move_L``, ``move_P``).

Limitation, stated: of the draws of the two streams only the multiple-try move's are stored value by value (tries, u_pick, u_acc; change
and leaf as what the coins and leaf choices came to).  The in-model GaussianMove's steps and accept uniforms, the rj move's choice and
both sweeps' permutations and uniforms are NOT recorded one by one: they are the two seeds' streams consumed in the reference's order
(tests/rj_mt_move.py states it), as in make_golden_rj.py's fixtures.  A change in the order of those draws therefore shows up in a
test on these fixtures as a state mismatch behind the in-model move or a sweep (``it{i}_mh_*``, the ladder, the swap counts), not as a
named draw that differs.  Data only.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                    # noqa: E402  (sets up the reference's import path; nothing runs on import)
import make_golden_rj as mgr                # noqa: E402  (the reference tests' own model functions, the boxes)

import numpy as np                          # noqa: E402
import eryn.moves.multipletry as mtry       # noqa: E402
from eryn.ensemble import EnsembleSampler   # noqa: E402
from eryn.moves import GaussianMove, MTDistGenMoveRJ   # noqa: E402
from eryn.prior import ProbDistContainer, uniform_dist  # noqa: E402
from eryn.state import State                # noqa: E402
from test_eryn import log_like_fn_gauss_pulse, log_like_fn_gauss_and_sine   # noqa: E402

OUT = os.environ.get("GOLDEN_OUT", os.path.join(HERE, "rj_mt"))
BOX = {"gauss": mgr.GAUSS_BOX, "sine": mgr.SINE_BOX}


def capture(name, names, T, W, K, nl_max, nl_min, nsteps, gen_box, ndata=64, sigma=0.5, cov_factor=1e-4, seed_data=42, seed_construct=135,
            seed_run=246, p_active=0.5):
    nleaves_max, nleaves_min = dict(zip(names, nl_max)), dict(zip(names, nl_min))
    t = np.linspace(-1, 1, ndata)
    rs = np.random.RandomState(seed_data)
    y = mgr.combine_gaussians(t, np.array([[3.0, -0.2, 0.1], [2.8, 0.3, 0.1]])) + sigma * rs.randn(ndata)
    if "sine" in names:
        y = y + mgr.combine_sine(t, np.array([[1.0, 2.0, 0.5]]))
    coords, inds = {}, {}
    for k in names:
        lo, hi = np.array(BOX[k]).T
        coords[k] = lo + (hi - lo) * rs.rand(T, W, nleaves_max[k], 3)
        inds[k] = rs.rand(T, W, nleaves_max[k]) < p_active
        inds[k][..., :nleaves_min[k]] = True
    priors = {k: ProbDistContainer({i: uniform_dist(*BOX[k][i]) for i in range(3)}) for k in names}
    gens = {k: ProbDistContainer({i: uniform_dist(*gen_box[k][i]) for i in range(3)}) for k in names}
    cov = {k: np.diag(np.ones(3)) * cov_factor for k in names}
    np.random.seed(seed_construct)          # R := snapshot of G at construction (ensemble.py:604,651-652)
    if len(names) == 1:
        rj_moves = MTDistGenMoveRJ(gens, nleaves_max=nleaves_max, nleaves_min=nleaves_min, num_try=K, rj=True)
        like, ndims, kw = log_like_fn_gauss_pulse, 3, dict(nleaves_max=nl_max[0], nleaves_min=nl_min[0])
    else:
        rj_moves = [MTDistGenMoveRJ({k: gens[k]}, nleaves_max=nleaves_max, nleaves_min=nleaves_min, num_try=K, rj=True, gibbs_sampling_setup=k)
                    for k in names]
        like, ndims, kw = log_like_fn_gauss_and_sine, {k: 3 for k in names}, dict(nleaves_max=nleaves_max, nleaves_min=nleaves_min)
    s = EnsembleSampler(W, ndims, like, priors, args=[t, y, sigma], tempering_kwargs=dict(ntemps=T), nbranches=len(names), branch_names=names,
                        moves=GaussianMove(cov), rj_moves=rj_moves, **kw)
    logp0 = s.compute_log_prior(coords, inds=inds)
    logl0 = s.compute_log_like(coords, inds=inds, logp=logp0)[0]
    state = State(coords, log_like=logl0, log_prior=logp0, inds=inds)
    out = dict(T=T, W=W, K=K, ndata=ndata, sigma=float(sigma), nsteps=nsteps, t=t, y=y, nl_max=np.array(nl_max), nl_min=np.array(nl_min),
               cov_factor=float(cov_factor), seed_construct=seed_construct, seed_run=seed_run, betas0=np.array(s.temperature_control.betas),
               L0=logl0, P0=logp0, branch_names=np.array(names))
    for k in names:
        out[f"x0_{k}"], out[f"inds0_{k}"] = coords[k].copy(), inds[k].copy()
        out[f"{k}_box"], out[f"{k}_gen_box"] = np.array(BOX[k]), np.array(gen_box[k])
    rlog, log, mt = [], [], {}
    s._random = mg.RProxy(s._random, rlog)
    orig_comp, orig_rand = mtry.get_mt_computations, np.random.rand

    def get_mt_computations(logP, log_proposal_pdf, **k):          # multipletry.py:36-59: the one np.random.rand in it is the pick's
        picks = []

        def rand(*a):
            picks.append(orig_rand(*a))
            return picks[-1]

        np.random.rand = rand
        try:
            w, lsw, keep = orig_comp(logP, log_proposal_pdf, **k)
        finally:
            np.random.rand = orig_rand
        assert len(picks) == 1
        mt["u_pick"] = picks[0].reshape(T, W).copy()
        return w, lsw, keep

    def snap(st, pre=""):
        d = {f"{pre}x_{k}": st.branches[k].coords.copy() for k in names}
        d.update({f"{pre}inds_{k}": st.branches[k].inds.copy() for k in names})
        d.update({pre + "L": st.log_like.copy(), pre + "P": st.log_prior.copy()})
        return d

    def wrap(move, tag):
        orig = move.propose

        def propose(model, st):
            rlog.clear()
            mt.clear()
            new, acc = orig(model, st)
            rec = snap(new)
            rec.update(tag=tag, accepted=np.array(acc, copy=True), betas=np.array(s.temperature_control.betas),
                       swaps=np.array(s.temperature_control.swaps_accepted))
            if tag.startswith("rj"):
                rands = [v for k, v in rlog if k == "rand"]
                rec.update(mt, u_acc=np.array(rands[-1], copy=True))
            log.append(rec)
            return new, acc
        move.propose = propose

    def hook_mt(move):
        orig_gen, orig_prop, orig_update = move.special_generate_func, move.get_mt_proposal, move.update

        def special_generate_func(coords_, random, **k):            # mtdistgenrj.py:40-77: the tries, a death's try 0 filled in
            pts, lq = orig_gen(coords_, random, **k)
            mt["tries"] = np.array(pts, copy=True).reshape(T, W, K, 3)
            return pts, lq

        def get_mt_proposal(coords_, random, **k):
            rev = k["inds_reverse_rj"]
            assert rev is not None and 0 < len(rev) < T * W, "a captured proposal needs births and deaths"
            pts, factors = orig_prop(coords_, random, **k)
            change = np.ones(T * W, dtype=np.int64)
            change[rev] = -1
            pick = np.array([np.flatnonzero((mt["tries"].reshape(T * W, K, 3)[i] == pts[i]).all(axis=1))[0] for i in range(T * W)])
            pick[rev] = 0
            mt.update(change=change.reshape(T, W), leaf=np.array(k["inds_leaves_rj"]).reshape(T, W), pick=pick.reshape(T, W),
                      lsw=np.array(move.log_sum_weights).reshape(T, W), aux_lsw=np.array(move.aux_log_sum_weights).reshape(T, W),
                      factors=np.array(factors, copy=True).reshape(T, W), mt_ll=np.array(move.mt_ll, copy=True).reshape(T, W),
                      mt_lp=np.array(move.mt_lp, copy=True).reshape(T, W))
            return pts, factors

        def update(old_state, new_state, accepted, subset=None):
            res = orig_update(old_state, new_state, accepted, subset=subset)
            mt["keep"] = np.array(accepted, copy=True)
            mt.update(snap(res, "move_"))
            return res

        move.special_generate_func, move.get_mt_proposal, move.update = special_generate_func, get_mt_proposal, update

    wrap(s.moves[0], "mh")
    for i, m in enumerate(s.rj_moves):
        wrap(m, f"rj{i}")
        hook_mt(m)
    np.random.seed(seed_run)                # G for the run
    mtry.get_mt_computations = get_mt_computations
    try:
        it = 0
        for _ in s.sample(state, iterations=nsteps, store=False):
            assert [r["tag"][:2] for r in log] == ["mh", "rj"], [r["tag"] for r in log]
            for r in log:
                pre = f"it{it}_{r['tag'][:2]}_"
                for k, v in r.items():
                    if k == "tag":
                        out[pre + "branch"] = int(r["tag"][2:]) if r["tag"].startswith("rj") else -1
                    else:
                        out[pre + k] = v
            log.clear()
            it += 1
    finally:
        mtry.get_mt_computations = orig_comp
    out["mh_accepted_total"] = np.array(s.moves[0].accepted)
    out["rj_accepted_total"] = np.stack([np.array(m.accepted) for m in s.rj_moves])
    out["rj_num_proposals"] = np.array([m.num_proposals for m in s.rj_moves])
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    its = range(nsteps)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; rj accepts {int(out['rj_accepted_total'].sum())} of {nsteps * T * W}; picks other than "
          f"try 0 {sum(int((out[f'it{i}_rj_pick'] != 0).sum()) for i in its)}; NaN factors {sum(int(np.isnan(out[f'it{i}_rj_factors']).sum()) for i in its)}; "
          f"-inf mt_lp {sum(int(np.isinf(out[f'it{i}_rj_mt_lp']).sum()) for i in its)}; leaves at the end "
          f"{[int(out[f'it{nsteps - 1}_rj_inds_{k}'].sum()) for k in names]}")


if __name__ == "__main__":
    capture("rjmt1", ["gauss"], T=3, W=8, K=5, nl_max=(4,), nl_min=(0,), nsteps=10, gen_box=BOX)
    capture("rjmt2", ["gauss", "sine"], T=3, W=8, K=7, nl_max=(3, 2), nl_min=(0, 0), nsteps=10, seed_run=99,
            gen_box={"gauss": [(2.4, 3.6), (-1.0, 1.0), (0.06, 0.21)], "sine": mgr.SINE_BOX})
