#!/usr/bin/env python
"""Generate tests/golden/rj_priors/*.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_rj_priors.py

make_golden_rj.py's capture (its ``run_capture``: the reference's ``EnsembleSampler`` with reversible jump, every iteration's state
behind the in-model move and behind the birth / death move) under ``ProbDistContainer``s that mix, per branch, ``uniform_dist``,
``log_uniform`` and ``scipy.stats.norm`` - the prior is then also the birth proposal and its density the Hastings factor:

    rjp1_separate_gaussian         pulses + sines, "separate_branches", GaussianMove            T = 3, W = 10, 8 iterations
    rjp2_together_stretch          pulses + sines, "together", StretchMove (one leaf per branch: the reference's red / blue move wants
                                   twice as many walkers as coordinates)                        T = 2, W = 12, 8 iterations
    rjp3_widths_callable_iterate   ramps (2) + bursts (4), a Python-callable likelihood, "iterate_branches"   T = 3, W = 8, 8 iterations

The priors travel as the ARGUMENTS of the reference's constructors (tests/rj_prior_terms.FIXTURE_PRIORS: ``{branch}_box`` rows (p0, p1),
``{branch}_prior_kind`` 0 uniform_dist, 1 log_uniform, 2 norm).  The fixtures live in a directory of their own:
tests/test_golden_regeneration.py holds the fixtures directly under tests/golden/ to the generators it knows.  The seeds are those at
which no accept decision of the chain sits within 1e-12 of the knife edge (tests/test_rj_prior_terms.py counts them).
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # (the repository: oracle/, tests/rj_prior_terms.py)
OUT = os.environ.setdefault("GOLDEN_OUT", os.path.join(HERE, "rj_priors"))      # (make_golden_rj.run_capture writes there)
os.makedirs(OUT, exist_ok=True)
import make_golden_rj as mgr                # noqa: E402  (sets up the reference's import path; nothing runs on import)

import numpy as np                          # noqa: E402
from scipy import stats                     # noqa: E402
from eryn.prior import ProbDistContainer, log_uniform, uniform_dist  # noqa: E402

from tests.rj_prior_terms import FIXTURE_PRIORS    # noqa: E402


def container(name):
    make = {0: uniform_dist, 1: log_uniform, 2: stats.norm}
    return ProbDistContainer({d: make[k](p0, p1) for d, (k, p0, p1) in enumerate(FIXTURE_PRIORS[name])})


def add_priors(name, branch_names):
    """The constructors' arguments into the fixture run_capture wrote (arrays only)."""
    path = os.path.join(OUT, name + ".npz")
    with np.load(path) as f:
        out = {k: f[k] for k in f.files}
    out["branch_names"] = np.array(branch_names)
    for k in branch_names:
        out[f"{k}_box"] = np.array([[p0, p1] for _, p0, p1 in FIXTURE_PRIORS[k]])
        out[f"{k}_prior_kind"] = np.array([kind for kind, _, _ in FIXTURE_PRIORS[k]])
    np.savez_compressed(path, **out)
    print(f"{name}: {os.path.getsize(path) / 1024:.0f} KiB")


def capture_template(name, T, W, nl_max, nl_min, nsteps, rj_moves, in_model, n_init, seed_run, cov_factor=1e-3, sigma=2.0, ndata=40,
                     init_spread=1e-4, seed_data=42, seed_construct=135):
    names = ["gauss", "sine"]
    t = np.linspace(-1, 1, ndata)
    gauss_inj = np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1], [3.4, 0.0, 0.1]])
    sine_inj = np.array([[1.3, 10.1, 1.0], [0.8, 4.6, 1.2]])
    rs = np.random.RandomState(seed_data)
    y = mgr.combine_gaussians(t, gauss_inj[:n_init[0]]) + mgr.combine_sine(t, sine_inj[:n_init[1]]) + sigma * rs.randn(ndata)
    nleaves_max, nleaves_min = dict(zip(names, nl_max)), dict(zip(names, nl_min))
    coords = {k: np.zeros((T, W, nleaves_max[k], 3)) for k in names}
    inds = {k: np.zeros((T, W, nleaves_max[k]), dtype=bool) for k in names}
    for k, inj, n in (("gauss", gauss_inj, n_init[0]), ("sine", sine_inj, n_init[1])):
        for nn in range(n):
            coords[k][:, :, nn] = rs.multivariate_normal(inj[nn], np.diag(np.ones(3) * init_spread), size=(T, W))
            inds[k][:, :, nn] = True
    priors = {k: container(k) for k in names}
    cov = {k: np.diag(np.ones(3)) * cov_factor for k in names}
    mgr.run_capture(name, T, W, nl_max, nl_min, nsteps, ndata, sigma, cov_factor, seed_construct, seed_run, rj_moves, in_model, "template",
                    names, {k: 3 for k in names}, nleaves_max, nleaves_min, t, y, coords, inds, priors, cov, None)
    add_priors(name, names)


def capture_widths(name, T, W, nl_max, nl_min, nsteps, rj_moves, n_init, seed_run, cov_factor=1e-3, sigma=3.0, ndata=40, init_spread=1e-4,
                   seed_data=42, seed_construct=135):
    names, _, inj, like_name, signal = mgr.GENERAL_MODELS["ramp_burst"]
    import oracle.eryn_oracle_rj as orj_
    ndims = {"ramp": 2, "burst": 4}
    t = np.linspace(-1, 1, ndata)
    rs = np.random.RandomState(seed_data)
    y = signal(t) + sigma * rs.randn(ndata)
    nleaves_max, nleaves_min = dict(zip(names, nl_max)), dict(zip(names, nl_min))
    coords = {k: np.zeros((T, W, nleaves_max[k], ndims[k])) for k in names}
    inds = {k: np.zeros((T, W, nleaves_max[k]), dtype=bool) for k in names}
    for bi, k in enumerate(names):
        for nn in range(n_init[bi]):
            coords[k][:, :, nn] = rs.multivariate_normal(inj[bi][nn], np.diag(np.ones(ndims[k]) * init_spread), size=(T, W))
            inds[k][:, :, nn] = True
    priors = {k: container(k) for k in names}
    cov = {k: np.diag(np.ones(ndims[k])) * cov_factor for k in names}
    boxes = [[(p0, p1) for _, p0, p1 in FIXTURE_PRIORS[k]] for k in names]
    mgr.run_capture(name, T, W, nl_max, nl_min, nsteps, ndata, sigma, cov_factor, seed_construct, seed_run, rj_moves, "gaussian", "ramp_burst",
                    names, ndims, nleaves_max, nleaves_min, t, y, coords, inds, priors, cov, boxes, like=getattr(orj_, like_name))
    add_priors(name, names)


if __name__ == "__main__":
    capture_template("rjp1_separate_gaussian", T=3, W=10, nl_max=(3, 4), nl_min=(0, 0), nsteps=8, rj_moves="separate_branches",
                     in_model="gaussian", n_init=(2, 1), seed_run=246)
    capture_template("rjp2_together_stretch", T=2, W=12, nl_max=(1, 1), nl_min=(0, 0), nsteps=8, rj_moves="together", in_model="stretch",
                     n_init=(1, 0), seed_run=61, init_spread=4e-4, sigma=4.0)
    capture_widths("rjp3_widths_callable_iterate", T=3, W=8, nl_max=(3, 3), nl_min=(0, 1), nsteps=8, rj_moves="iterate_branches",
                   n_init=(1, 2), seed_run=511)
