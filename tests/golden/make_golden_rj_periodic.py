#!/usr/bin/env python
"""Generate tests/golden/rj_periodic/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rj_periodic.py            (or: ... search)

make_golden_rj.py's model and capture technique - the reference's ``EnsembleSampler`` on pulses + sines, every move's ``propose`` and
``update`` wrapped - with ``periodic={"gauss": {}, "sine": {2: 2 pi}}`` (the reference's ``wrap`` raises KeyError on a branch that is
missing from the container, hence the empty dict): the sine phase is periodic in every in-model move.

    rjp_gauss    GaussianMove with a FULL leaf covariance, rj_moves=True ("together")
    rjp_stretch  StretchMove(live_dangerously=True) (8 walkers, 18 coordinates), "separate_branches"
    rjp_group    make_golden_rj_group.py's NearestFriends (nfriends = 3, key: pulse centre / sine frequency, n_iter_update = 3)
    rjp_gibbs    GaussianMove in one Gibbs block per branch, make_golden_rj_priors.py's log-uniform / normal leaf priors

T = 3, W = 8, 40 data points, 8 iterations; pulses 4 slots (2 at the start), sines 2 slots (1 at the start).  The injected sine has its
phase ON the seam; the start puts the active phases on both sides of it (even walkers just above 0, odd ones just below 2 pi, within
0.06) and gives the DEAD sine slot phases outside [0, 2 pi): negative, above 2 pi, many periods out.

Recorded: per iteration and proposal (a Gaussian move: one; a stretch move: one per half; a Gibbs move: one per block) the proposal q,
the accept uniforms and mask (zz's uniforms for the stretch-type moves), the picks and windows of the group move; the state behind the
in-model move's sweep and behind the reversible-jump move as in the rj* fixtures.  Data only.

``check`` holds the reference ALONE to what a fixture must exercise, from the arguments and results of its own
``PeriodicContainer.distance`` / ``wrap`` calls: an accepted proposal whose ACTIVE phase left [0, 2 pi) and was wrapped back in; for
the stretch-type moves an active |c - s| > pi taken the short way round; an accepted walker whose dead-slot phase changed bits through
the wrap; a rejection; no knife-edge accept (the existing generators' definition).  The seeds were searched until it held."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # (the repository: tests/rj_periodic.py and the specifications it composes)
OUT = os.environ.get("GOLDEN_OUT") or os.path.join(HERE, "rj_periodic")      # (the regeneration test writes elsewhere)
os.makedirs(OUT, exist_ok=True)
import make_golden_rj as mgr                # noqa: E402  (sets up the reference's import path; nothing runs on import)
import make_golden_rj_group as mgg          # noqa: E402  (NearestFriends, the friend rule on the reference's hooks)

import numpy as np                          # noqa: E402
from scipy import stats                     # noqa: E402
from eryn.ensemble import EnsembleSampler   # noqa: E402
from eryn.moves import GaussianMove, StretchMove  # noqa: E402
from eryn.prior import ProbDistContainer, log_uniform, uniform_dist  # noqa: E402
from eryn.state import BranchSupplemental, State  # noqa: E402

from tests.rj_periodic import GIBBS_SETUP, PERIODIC, TWO_PI, SeamFacts  # noqa: E402
from tests.rj_prior_terms import FIXTURE_PRIORS  # noqa: E402

NAMES = ["gauss", "sine"]
NL_MAX, N_INIT = (4, 2), (2, 1)
FULL_COV = 1e-3 * np.array([[1.0, 0.3, -0.2], [0.3, 1.0, 0.4], [-0.2, 0.4, 1.0]])
DIAG_COV = 1e-3 * np.diag(np.ones(3))
SEAM_WIDTH = 0.06          # the active phases start within this of the seam: two widths of the Gaussian step (sigma = 0.032)


def seam_start(coords, inds, rs):
    """Active sine phases on both sides of the seam; the dead sine slot outside [0, 2 pi)."""
    T, W = inds["sine"].shape[:2]
    d = rs.uniform(0.005, SEAM_WIDTH, size=(T, W))
    w = np.arange(W)[None, :]
    coords["sine"][:, :, 0, 2] = np.where(w % 2 == 0, d, TWO_PI - d)
    coords["sine"][:, :, 1, 0] = rs.uniform(0.6, 1.4, size=(T, W))
    coords["sine"][:, :, 1, 1] = rs.uniform(2.0, 19.0, size=(T, W))
    far = np.array([-1.3, TWO_PI + 0.7, 40.0, 3.0])
    coords["sine"][:, :, 1, 2] = far[w % 4] + rs.uniform(-0.05, 0.05, size=(T, W))


def container(name):
    make = {0: uniform_dist, 1: log_uniform, 2: stats.norm}
    return ProbDistContainer({d: make[k](p0, p1) for d, (k, p0, p1) in enumerate(FIXTURE_PRIORS[name])})


def capture(name, in_model, rj_moves, seed_run, cov=None, terms=False, nfriends=3, n_iter_update=3, key=None, a=2.0, T=3, W=8, nsteps=8,
            sigma=2.0, ndata=40, init_spread=1e-4, seed_data=42, seed_construct=135, save=True):
    t = np.linspace(-1, 1, ndata)
    inj = {"gauss": np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1]]), "sine": np.array([[1.3, 10.1, 0.0]])}
    rs = np.random.RandomState(seed_data)
    y = sigma * rs.randn(ndata) + mgr.combine_gaussians(t, inj["gauss"]) + mgr.combine_sine(t, inj["sine"])
    nleaves_max, nleaves_min = dict(zip(NAMES, NL_MAX)), {k: 0 for k in NAMES}
    coords = {k: np.zeros((T, W, nleaves_max[k], 3)) for k in NAMES}
    inds = {k: np.zeros((T, W, nleaves_max[k]), dtype=bool) for k in NAMES}
    for bi, k in enumerate(NAMES):
        for nn in range(N_INIT[bi]):
            coords[k][:, :, nn] = rs.multivariate_normal(inj[k][nn], np.diag(np.ones(3) * init_spread), size=(T, W))
            inds[k][:, :, nn] = True
    seam_start(coords, inds, rs)
    boxes = {"gauss": mgr.GAUSS_BOX, "sine": mgr.SINE_BOX}
    priors = {k: container(k) for k in NAMES} if terms else {k: {i: uniform_dist(*boxes[k][i]) for i in range(3)} for k in NAMES}
    cov = DIAG_COV if cov is None else cov
    np.random.seed(seed_construct)          # R := snapshot of G at construction (ensemble.py:604,651-652)
    if in_model == "gaussian":
        move = GaussianMove({k: cov.copy() for k in NAMES})
    elif in_model == "gibbs":
        move = GaussianMove({k: cov.copy() for k in NAMES}, gibbs_sampling_setup=list(GIBBS_SETUP))
    elif in_model == "stretch":
        move = StretchMove(a=a, live_dangerously=True)
    else:
        move = mgg.NearestFriends(key, nfriends=nfriends, n_iter_update=n_iter_update, a=a)
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")     # (ensemble.py:509-514: the reference advises against the stretch move under RJ - and runs it)
        s = EnsembleSampler(W, {k: 3 for k in NAMES}, mgr.log_like_fn_gauss_and_sine, priors, args=[t, y, sigma],
                            tempering_kwargs=dict(ntemps=T), nbranches=2, branch_names=NAMES, nleaves_max=nleaves_max,
                            nleaves_min=nleaves_min, moves=move, rj_moves=rj_moves, periodic={k: dict(v) for k, v in PERIODIC.items()})
    pc = move.periodic
    assert pc is not None and all(m.periodic is pc for m in s.rj_moves), "the sampler hands every move its container"
    s._random = rec_random = mgg.RecordingRandom(s._random)
    logp0 = s.compute_log_prior(coords, inds=inds)
    logl0 = s.compute_log_like(coords, inds=inds, logp=logp0)[0]
    supps = None
    if in_model == "group":
        supps = {k: BranchSupplemental({"start": np.full(inds[k].shape, -1, dtype=np.int64), "assigned": np.zeros(inds[k].shape, dtype=bool)},
                                       base_shape=inds[k].shape) for k in NAMES}
    state = State(coords, log_like=logl0, log_prior=logp0, inds=inds, branch_supplemental=supps)
    out = dict(T=T, W=W, ndata=ndata, sigma=float(sigma), nsteps=nsteps, t=t, y=y, nl_max=np.array(NL_MAX), nl_min=np.zeros(2, dtype=int),
               seed_construct=seed_construct, seed_run=seed_run, betas0=np.array(s.temperature_control.betas), L0=logl0, P0=logp0,
               rj_moves="together" if rj_moves is True else rj_moves, in_model=in_model, branch_names=np.array(NAMES), a=float(a),
               cov_factor=float(cov[0, 0]))
    if in_model == "group":
        out.update(nfriends=nfriends, n_iter_update=n_iter_update, key=np.array([key[k] for k in NAMES]))
    for k in NAMES:
        out[f"cov_{k}"] = cov.copy()
        out[f"period_{k}"] = np.array([float((PERIODIC[k] or {}).get(i, 0.0)) for i in range(3)])
        out[f"x0_{k}"], out[f"inds0_{k}"] = coords[k].copy(), inds[k].copy()
        if terms:
            out[f"{k}_box"] = np.array([[p0, p1] for _, p0, p1 in FIXTURE_PRIORS[k]])
            out[f"{k}_prior_kind"] = np.array([kind for kind, _, _ in FIXTURE_PRIORS[k]])
        else:
            out[f"{k}_box"] = np.array(boxes[k])

    # ---- the reference's own periodic calls, and what every proposal did with them -----------------------------------------------
    periods = {k: out[f"period_{k}"] for k in NAMES}
    facts, seen, props, log = SeamFacts(), dict(raw={}, dist=[]), [], []
    knife = [0]
    orig_wrap, orig_distance, orig_update = pc.wrap, pc.distance, move.update

    def wrap_(p, xp=None):
        for k, v in p.items():
            seen["raw"][k] = v.copy()
        return orig_wrap(p, xp=xp)

    def distance_(p1, p2, xp=None):
        for k in p1:
            seen["dist"].append((k, p1[k].copy(), p2[k].copy()))
        return orig_distance(p1, p2, xp=xp)
    pc.wrap, pc.distance = wrap_, distance_
    ndim_total = sum(nleaves_max[k] * 3 for k in NAMES)

    def update(old_state, new_state, accepted, subset=None):
        def take(arr):
            return arr if subset is None else np.take_along_axis(arr, subset.reshape(subset.shape + (1,) * (arr.ndim - 2)), axis=1)
        keep = np.array(take(np.asarray(accepted)), dtype=bool)
        q = {k: new_state.branches[k].coords.copy() for k in NAMES}
        ii = {k: new_state.branches[k].inds.copy() for k in NAMES}
        x_old = {k: take(old_state.branches[k].coords).copy() for k in NAMES}
        raw = {k: seen["raw"][k].reshape(q[k].shape) if k in seen["raw"] else q[k] for k in NAMES}
        for k, p1, p2 in seen["dist"]:
            facts.differences(periods, k, p1.reshape(q[k].shape), p2.reshape(q[k].shape), ii[k])
        facts.proposal(periods, x_old, raw, q, ii, keep)
        factors = (ndim_total - 1.0) * np.log(move.zz) if in_model in ("stretch", "group") else 0.0
        u_acc = rec_random.rands[-1]
        with np.errstate(divide="ignore", invalid="ignore"):
            lnpdiff = (factors + move.compute_log_posterior(new_state.log_like, new_state.log_prior)
                       - move.compute_log_posterior(take(old_state.log_like), take(old_state.log_prior)))
            assert np.array_equal(lnpdiff > np.log(u_acc), keep)
            betas = np.asarray(move.temperature_control.betas)[:, None]
            edge = np.abs(lnpdiff - np.log(u_acc)) <= 1e-12 * np.maximum(np.abs(betas * new_state.log_like), 1.0)
            edge &= new_state.log_like != -1e300
            knife[0] += bool(np.any(edge & np.isfinite(lnpdiff)))
        p = dict(q=q, keep=keep, u_acc=u_acc.copy())
        if in_model in ("stretch", "group"):
            p["u_zz"] = rec_random.rands[-2].copy()
        if in_model == "group":
            p["pick"] = {k: move.seen["picks"][k].copy() for k in NAMES}
            p["start"] = {k: move.seen["start"][k].copy() for k in NAMES}
        props.append(p)
        seen["raw"].clear()
        seen["dist"].clear()
        return orig_update(old_state, new_state, accepted, subset=subset)
    move.update = update

    def snap(st):
        d = {f"x_{k}": st.branches[k].coords.copy() for k in NAMES}
        d.update({f"inds_{k}": st.branches[k].inds.copy() for k in NAMES})
        d.update(L=st.log_like.copy(), P=st.log_prior.copy())
        return d

    def wrap_move(mv, tag):
        orig = mv.propose

        def propose(model, st):
            if tag == "mh" and in_model == "group":
                move.seen.clear()
            new, acc = orig(model, st)
            r = snap(new)
            r.update(tag=tag, accepted=np.array(acc, copy=True), betas=np.array(s.temperature_control.betas),
                     swaps=np.array(s.temperature_control.swaps_accepted))
            log.append(r)
            return new, acc
        mv.propose = propose
    wrap_move(move, "mh")
    for i, m in enumerate(s.rj_moves):
        wrap_move(m, f"rj{i}")

    np.random.seed(seed_run)                # G for the run
    it = 0
    for st in s.sample(state, iterations=nsteps, store=False):
        assert [r["tag"][:2] for r in log] == ["mh", "rj"], [r["tag"] for r in log]
        out[f"it{it}_nprop"] = len(props)
        for j, p in enumerate(props):
            pre = f"it{it}_p{j}_"
            out[pre + "keep"], out[pre + "u_acc"] = p["keep"], p["u_acc"]
            if "u_zz" in p:
                out[pre + "u_zz"] = p["u_zz"]
            for k in NAMES:
                out[pre + f"q_{k}"] = p["q"][k]
                if "pick" in p:
                    out[pre + f"pick_{k}"], out[pre + f"start_{k}"] = p["pick"][k], p["start"][k]
        for r in log:
            p2 = f"it{it}_{r['tag'][:2]}_"
            for k, v in r.items():
                if k == "tag":
                    out[p2 + "branch"] = int(r["tag"][2:]) if r["tag"].startswith("rj") else -1
                else:
                    out[p2 + k] = v
        props.clear()
        log.clear()
        it += 1
    out["mh_accepted_total"] = np.array(move.accepted)
    out["mh_num_proposals"] = int(move.num_proposals)
    out["rj_accepted_total"] = np.stack([np.array(m.accepted) for m in s.rj_moves])
    out["rj_num_proposals"] = np.array([m.num_proposals for m in s.rj_moves])
    f = facts.as_dict()
    f["knife"] = knife[0]
    for k, v in f.items():
        out["facts_" + k] = int(v)
    if save:
        path = os.path.join(OUT, name + ".npz")
        np.savez_compressed(path, **out)
        print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB; {f}")
    return out, f


def check_start(o):
    """The conditions on the start."""
    ph, act = o["x0_sine"][..., 2], o["inds0_sine"]
    a = ph[act]
    assert np.any(a < SEAM_WIDTH) and np.any(a > TWO_PI - SEAM_WIDTH) and np.all((a < SEAM_WIDTH) | (a > TWO_PI - SEAM_WIDTH)), "active phases at the seam"
    d = ph[~act]
    assert np.any(d < 0.0) and np.any(d >= TWO_PI) and np.any(d > 5 * TWO_PI), "dead phases outside [0, 2 pi): negative, above, many periods out"


def check(f, in_model):
    """What every fixture must hold, from the reference's own calls."""
    return (f["wrapped_accepts"] >= 1 and f["dead_changed"] >= 1 and f["rejected"] >= 1 and f["accepted"] >= 1 and f["knife"] == 0
            and (in_model not in ("stretch", "group") or f["short_way"] >= 1))


FIXTURES = {
    "rjp_gauss": dict(in_model="gaussian", rj_moves=True, cov=FULL_COV),
    "rjp_stretch": dict(in_model="stretch", rj_moves="separate_branches"),
    "rjp_group": dict(in_model="group", rj_moves="separate_branches", key={"gauss": 1, "sine": 1}),
    "rjp_gibbs": dict(in_model="gibbs", rj_moves="separate_branches", terms=True),
}
SEEDS = {"rjp_gauss": 1, "rjp_stretch": 1, "rjp_group": 1, "rjp_gibbs": 1}          # seed_run, found by ``search``


def search(name, first=1, last=400):
    for seed in range(first, last):
        try:
            _, f = capture(name, seed_run=seed, save=False, **FIXTURES[name])
        except AssertionError:
            continue
        if check(f, FIXTURES[name]["in_model"]):
            return seed
    raise SystemExit(f"{name}: no seed in [{first}, {last}) holds every assertion")


def generate(name, save=True):
    o, f = capture(name, seed_run=SEEDS[name], save=save, **FIXTURES[name])
    check_start(o)
    assert check(f, FIXTURES[name]["in_model"]), (name, f)
    return o


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "search":
        print({name: search(name) for name in FIXTURES})
        raise SystemExit(0)
    for name in FIXTURES:
        generate(name)
