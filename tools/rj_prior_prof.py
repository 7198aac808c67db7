"""What prior terms on the leaves cost hens_rj_step at config 4's shape (8 x 2048 walkers, pulses x 10 + sines x 10, 500 data points on
a linspace).

  python tools/rj_prior_prof.py --model box|uniform_wide|mixed [--iters 300] [--runs 3]
      box           bench.py's config-4 model: boxes, the pulse / sine instantiations of k_rj (uniform-grid recurrences)
      uniform_wide  the same boxes handed to hens_rj_set_model_kinds' kernels by way of an all-but-uniform specification - every
                    parameter uniform but one normal parameter per branch wide enough (scale 1e6) to be flat: the kernels that carry
                    terms (per-point leaf values, no recurrences) with next to no change of the posterior: what the ROUTING costs
      mixed         one log-uniform and one normal parameter per branch (pulse amplitude log-uniform on its box, pulse centre normal(0,
                    0.5); sine amplitude normal(1, 0.25), sine frequency log-uniform on its box)
  One JSON line: microseconds per iteration of `runs` timed calls of step(iters) after a warm-up call, their median, accept rates.

Each model is one process; on a shared GPU run them one after the other, each under a time limit of its own:
  timeout -k 10 300 python tools/rj_prior_prof.py --model box && timeout -k 10 300 python tools/rj_prior_prof.py --model uniform_wide && \\
  timeout -k 10 300 python tools/rj_prior_prof.py --model mixed
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GAUSS_BOX = [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)]
SINE_BOX = [(0.5, 1.5), (1.0, 20.0), (0.0, 2 * np.pi)]


def priors(model):
    from eryn_amd.prior import LogUniformDistribution, NormalDistribution, uniform_dist
    g = {i: uniform_dist(*GAUSS_BOX[i]) for i in range(3)}
    s = {i: uniform_dist(*SINE_BOX[i]) for i in range(3)}
    if model == "box":
        return GAUSS_BOX, SINE_BOX
    if model == "uniform_wide":
        g[1], s[2] = NormalDistribution(0.0, 1e6), NormalDistribution(np.pi, 1e6)
    else:
        g[0], g[1] = LogUniformDistribution(*GAUSS_BOX[0]), NormalDistribution(0.0, 0.5)
        s[0], s[1] = NormalDistribution(1.0, 0.25), LogUniformDistribution(*SINE_BOX[1])
    return g, s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", required=True, choices=["box", "uniform_wide", "mixed"])
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    args = ap.parse_args()
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import RJEngine, TemplateBranch
    T, W, NL, N = 8, 2048, 10, 500
    t = np.linspace(-1, 1, N)
    rs = np.random.RandomState(42)
    gauss_inj = np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1], [3.4, 0.0, 0.1], [2.9, 0.3, 0.1]])
    sine_inj = np.array([[1.3, 10.1, 1.0], [0.8, 4.6, 1.2]])
    y = sum(a * np.exp(-((t - b) ** 2) / (2 * c ** 2)) for a, b, c in gauss_inj) + \
        sum(a * np.sin(2 * np.pi * b * t + c) for a, b, c in sine_inj) + 2.0 * rs.randn(N)
    pg, ps = priors(args.model)
    brs = [TemplateBranch("gauss", "pulse", pg, NL, 0), TemplateBranch("sine", "sine", ps, NL, 0)]
    eng = RJEngine(T, W, brs, t, y, 2.0, seed=2024)
    x = {"gauss": np.zeros((T, W, NL, 3)), "sine": np.zeros((T, W, NL, 3))}
    inds = {k: np.zeros((T, W, NL), dtype=bool) for k in x}
    for n in range(4):
        x["gauss"][:, :, n] = gauss_inj[n] + 1e-2 * rs.randn(T, W, 3) * [1, 1, 0.1]
        inds["gauss"][:, :, n] = True
    for n in range(2):
        x["sine"][:, :, n] = sine_inj[n] + 1e-2 * rs.randn(T, W, 3)
        inds["sine"][:, :, n] = True
    eng.upload(x, inds, betas=make_ladder(18, ntemps=T))
    eng.eval_state()
    eng.set_mh_scale(np.full((2, 3), 1e-2) * [[1, 1, 0.1], [1, 1, 1]])
    eng.step(100)                                               # warm-up: the leaf counts settle
    eng.synchronize()
    per = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        eng.step(args.iters)
        eng.synchronize()
        per.append((time.perf_counter() - t0) / args.iters * 1e6)
    c = eng.counters()
    _, inds1, L, P, _ = eng.download()
    print(json.dumps({"model": args.model, "prior_terms": bool(eng.prior_terms), "shape": f"{T} x {W}, {NL} + {NL} leaves, {N} points",
                      "iters_per_run": args.iters, "us_per_iteration": [round(v, 2) for v in per], "median_us": round(float(np.median(per)), 2),
                      "accept_in_model": round(float(c["accepted_mh"].sum()) / (c["num_mh"] * T * W), 4),
                      "accept_birth_death": round(float(c["accepted_bd"].sum()) / (c["num_bd"] * T * W), 4),
                      "mean_leaves": {k: round(float(v.sum(-1).mean()), 2) for k, v in inds1.items()},
                      "log_prior_finite": bool(np.isfinite(P).all())}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
