"""Cost of hens_rj_step on a model of the leaf kinds beyond pulse / sine (hens_rj_set_model_kinds, the WIDE instantiations of
k_rj) at BASELINE config 4's shape: 8 x 2048 walkers, 500 data points, a ramp branch and a burst branch of 10 leaves each
(60 coordinates; W = 2048 >= 2 x 60), and of the host-callable path on the same model and state.

  python tools/rj_leaf_kinds_prof.py [--steps K] [--warmup W] [--moves diag,stretch] [--host-iters N]

prints one JSON line per in-model move with the microseconds per iteration of bench.py's block protocol (tools/rj_inmodel_prof.py's),
then - unless --host-iters 0 - one line for RJEnsembleSampler(log_like_fn=<the same model as a Python function>, rng="numpy"):
seconds per iteration over N iterations (hens_rj_propose -> one Python call per walker -> hens_rj_accept, twice per iteration)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the block protocol: timed_blocks, step_seconds)

BOX = {"ramp": [(-1.0, 1.0), (-2.0, 2.0)], "burst": [(0.5, 3.0), (-1.0, 1.0), (0.05, 0.5), (1.0, 8.0)]}
NAMES = ["ramp", "burst"]
SIGMA = 3.0


def ramp_burst(x_list, t, y, sigma):
    """The model as a user function in the reference's per-walker calling convention."""
    ramps, bursts = x_list
    tm = np.zeros_like(t)
    if ramps is not None:
        for a, b in np.atleast_2d(ramps):
            tm = tm + (a + b * t)
    if bursts is not None:
        for a, t0, w, f in np.atleast_2d(bursts):
            tm = tm + a * np.exp(-(((t - t0) / w) ** 2)) * np.cos(2 * np.pi * f * (t - t0))
    return -0.5 * np.sum(((tm - y) / sigma) ** 2)


def problem(T=8, W=2048, N=500, NL=10):
    """Data from two ramps and four bursts; every walker starts near them (4 + 2 leaves, as config 4's start)."""
    t = np.linspace(-1, 1, N)
    rs = np.random.RandomState(42)
    inj = {"ramp": np.array([[0.3, 1.2], [-0.5, -0.4]]),
           "burst": np.array([[2.1, -0.4, 0.2, 3.0], [1.4, 0.1, 0.1, 6.0], [2.6, 0.5, 0.3, 2.0], [0.9, -0.7, 0.08, 5.0]])}
    y = SIGMA * rs.randn(N)
    for a, b in inj["ramp"]:
        y = y + (a + b * t)
    for a, t0, w, f in inj["burst"]:
        y = y + a * np.exp(-(((t - t0) / w) ** 2)) * np.cos(2 * np.pi * f * (t - t0))
    x = {k: np.zeros((T, W, NL, len(BOX[k]))) for k in NAMES}
    inds = {k: np.zeros((T, W, NL), dtype=bool) for k in NAMES}
    for k, n_start in (("ramp", 2), ("burst", 4)):
        width = np.array([hi - lo for lo, hi in BOX[k]])
        x[k][:] = inj[k][0]
        for n in range(n_start):
            x[k][:, :, n] = inj[k][n] + 1e-3 * width * rs.randn(T, W, len(BOX[k]))
            inds[k][:, :, n] = True
    scale = [1e-2 * np.array([hi - lo for lo, hi in BOX[k]]) for k in NAMES]
    return t, y, x, inds, scale


def make_engine(move, T=8, W=2048):
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import RJEngine, TemplateBranch
    t, y, x, inds, scale = problem(T, W)
    eng = RJEngine(T, W, [TemplateBranch(k, k, BOX[k], 10, 0) for k in NAMES], t, y, SIGMA, seed=2024)
    eng.upload(x, inds, betas=make_ladder(18, ntemps=T))
    eng.eval_state()
    if move == "diag":
        eng.set_mh_scale(scale)
    elif move == "stretch":
        eng.set_in_model("stretch")
    else:
        raise SystemExit(f"unknown move {move}")
    return eng


def host_path(iters, T=8, W=2048):
    from eryn_amd.prior import uniform_dist
    from eryn_amd.rj import GaussianLeafMove, RJEnsembleSampler
    from eryn_amd.state import State
    t, y, x, inds, scale = problem(T, W)
    priors = {k: {i: uniform_dist(*BOX[k][i]) for i in range(len(BOX[k]))} for k in NAMES}
    s = RJEnsembleSampler(W, {k: len(BOX[k]) for k in NAMES}, ramp_burst, priors, args=[t, y, SIGMA], tempering_kwargs=dict(ntemps=T),
                          branch_names=NAMES, nleaves_max={k: 10 for k in NAMES}, moves=GaussianLeafMove({k: np.diag(sc ** 2) for k, sc in zip(NAMES, scale)}))
    st = s.run_mcmc(State(x, inds=inds), 1, store=False)          # (first evaluation + one iteration: warm-up)
    t0 = time.perf_counter()
    s.run_mcmc(st, iters, store=False)
    dt = (time.perf_counter() - t0) / iters
    s.engine.close()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--moves", default="diag,stretch")
    ap.add_argument("--host-iters", type=int, default=2)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rj_leaf_kinds_prof.py measures on the GPU: none found")
    for move in args.moves.split(","):
        eng = make_engine(move)
        eng.step(args.warmup)
        eng.synchronize()
        times, _ = bench.timed_blocks(eng.step, eng.synchronize, args.steps)
        dt = bench.step_seconds(times, args.steps)
        c = eng.counters()
        print(json.dumps({"model": "ramp + burst, 10 leaves each", "move": move, "us_per_iteration": dt * 1e6,
                          "block_us_per_iteration": [t_ / k * 1e6 for t_, k in zip(times, bench.block_sizes(args.steps))],
                          "accept_in_model": float(c["accepted_mh"].mean() / max(c["num_mh"], 1)),
                          "accept_birth_death": float(c["accepted_bd"].mean() / max(c["num_bd"], 1)),
                          "timing": bench.timing_label(args.steps)}), flush=True)
        eng.close()
    if args.host_iters > 0:
        dt = host_path(args.host_iters)
        print(json.dumps({"model": "ramp + burst, 10 leaves each", "path": "host-callable likelihood, rng=numpy", "iterations": args.host_iters,
                          "us_per_iteration": dt * 1e6}), flush=True)


if __name__ == "__main__":
    main()
