"""Cost of per-parameter prior terms in hens_step (include/hipensemble.h: hens_set_prior_terms) against the box on the same launch
sequence: the three copying launches per iteration (two half-steps, the cascade).

  python tools/prior_terms_prof.py [--steps K] [--warmup W] [--shapes 16x4096x32,8x16384x64] [--priors box,normal,log_uniform,half]

prints one JSON line per (shape, prior): microseconds per iteration of bench.py's block protocol (median block of timed_blocks),
and microseconds per launch from the event pairs of hens_set_profiling 1 in a call of its own (stretch = a half-step, pt = the
cascade).  "box" is the baseline: run it with HENS_NO_FUSED=1, which sends the box to the copying launches too (k_stretch_fast) -
on the parent's library with HENS_LIB=<its libhipensemble.so> (tools/mkbase.sh), where the other priors do not exist.  A context with
prior terms takes k_stretch_prior at these widths.

The model: bench.py's dense Gaussian at mean 5 in every coordinate, so that every prior below holds the same posterior mass -
box: uniform(-50, 50); normal: norm(5, 10); log_uniform: loguniform(1e-2, 1e2); half: even coordinates normal, odd log-uniform."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the block protocol: timed_blocks, step_seconds)


def container(kind, D):
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, ProbDistContainer, uniform_dist
    make = dict(box=lambda d: uniform_dist(-50.0, 50.0), normal=lambda d: NormalDistribution(5.0, 10.0),
                log_uniform=lambda d: LogUniformDistribution(1e-2, 1e2),
                half=lambda d: NormalDistribution(5.0, 10.0) if d % 2 == 0 else LogUniformDistribution(1e-2, 1e2))[kind]
    return ProbDistContainer({d: make(d) for d in range(D)})


def make_engine(kind, T, W, D, seed=2024):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves.tempering import make_ladder
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    mu, invcov = np.full(D, 5.0), np.linalg.inv(A @ A.T / D + np.eye(D))
    c = container(kind, D)
    if kind == "box":                       # (through the box's own entry point: the parent's library has no other)
        eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), *c.box_bounds(), seed=seed)
    else:
        eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), None, None, seed=seed, prior_terms=c)
    eng.upload(np.clip(mu + np.random.RandomState(1).randn(T, W, D), 0.1, 20.0), betas=make_ladder(D, ntemps=T))
    eng.eval_state()
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--shapes", default="16x4096x32,8x16384x64")
    ap.add_argument("--priors", default="box,normal,log_uniform,half")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("prior_terms_prof.py measures on the GPU: none found")
    for shape in args.shapes.split(","):
        T, W, D = (int(v) for v in shape.split("x"))
        for kind in args.priors.split(","):
            eng = make_engine(kind, T, W, D)
            eng.step(args.warmup)
            eng.synchronize()
            times, _ = bench.timed_blocks(eng.step, eng.synchronize, args.steps)
            dt = bench.step_seconds(times, args.steps)
            eng.set_profiling(1)
            eng.step(20)
            eng.synchronize()
            tm = eng.timing()
            eng.set_profiling(0)
            c = eng.counters()
            _, _, P, _ = eng.download(want_x=False)
            print(json.dumps({"shape": shape, "prior": kind, "library": os.environ.get("HENS_LIB", "tree"),
                              "no_fused": bool(os.environ.get("HENS_NO_FUSED")), "us_per_iteration": dt * 1e6,
                              "block_us_per_iteration": [t_ / k * 1e6 for t_, k in zip(times, bench.block_sizes(args.steps))],
                              "launches_per_iteration": {k: tm[k] / 20 for k in ("n_stretch", "n_pt", "n_fused")},
                              "us_per_stretch_launch": tm["stretch_ms"] * 1e3 / max(tm["n_stretch"], 1),
                              "us_per_pt_launch": tm["pt_ms"] * 1e3 / max(tm["n_pt"], 1),
                              "accept": float(c["accepted"].mean() / max(c["num_proposals"], 1)), "finite_log_prior": bool(np.isfinite(P).all()),
                              "timing": bench.timing_label(args.steps)}), flush=True)
            eng.close()


if __name__ == "__main__":
    main()
