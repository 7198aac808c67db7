"""What the multiple-try birth / death move costs hens_rj_step at config 4's shape (8 x 2048 walkers, pulses x 10 + sines x 10, 500 data
points on a linspace, bench.py's model and start).

  python tools/rj_mt_prof.py --num-try K [--iters 300] [--runs 3] [--schedule separate_branches|none]
      K = 0         the plain move (DistributionGenerateRJ: k_rj<RJ_MODE_BD, 1>, one `template +- leaf` evaluation per walker)
      K = 1 .. 64   MTDistGenMoveRJ with the prior as the generator (k_rj_mt<true>: K such evaluations on one load of the walker's
                    record and template)
      --schedule none   no birth / death move at all: what the rest of the iteration costs
  One JSON line: microseconds per iteration of `runs` timed calls of step(iters) after a warm-up call, their median, accept rates.

The launches' own durations come from the same runs under `rocprofv3 --kernel-trace --stats` (tools/kernel_stats.sh tools/rj_mt_prof.py
--num-try K --runs 1): k_rj_mt at K tries against K times the k_rj<2, 1> launch of the K = 0 run - the same number of `template +- leaf`
evaluations.  Each setting is one process; on a shared GPU run them one after the other, each under a time limit of its own.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-try", type=int, required=True)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--schedule", default="separate_branches", choices=["separate_branches", "iterate_branches", "none"])
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
    brs = [TemplateBranch("gauss", "pulse", [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], NL, 0),
           TemplateBranch("sine", "sine", [(0.5, 1.5), (1.0, 20.0), (0.0, 2 * np.pi)], NL, 0)]
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
    eng.set_schedule(args.schedule)
    if args.num_try > 0:
        eng.set_mt_proposal(args.num_try)
    eng.step(100)                                               # warm-up: the leaf counts settle
    eng.synchronize()
    c0 = eng.counters()
    per = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        eng.step(args.iters)
        eng.synchronize()
        per.append((time.perf_counter() - t0) / args.iters * 1e6)
    c = eng.counters()
    _, inds1, L, P, _ = eng.download()
    n_mh, n_bd = c["num_mh"] - c0["num_mh"], c["num_bd"] - c0["num_bd"]
    print(json.dumps({"num_try": args.num_try, "schedule": args.schedule, "shape": f"{T} x {W}, {NL} + {NL} leaves, {N} points",
                      "iters_per_run": args.iters, "us_per_iteration": [round(v, 2) for v in per], "median_us": round(float(np.median(per)), 2),
                      "accept_in_model": round(float((c["accepted_mh"] - c0["accepted_mh"]).sum()) / (max(n_mh, 1) * T * W), 4),
                      "accept_birth_death": round(float((c["accepted_bd"] - c0["accepted_bd"]).sum()) / (max(n_bd, 1) * T * W), 4),
                      "accept_birth_death_cold_rung": round(float((c["accepted_bd"] - c0["accepted_bd"])[0].sum()) / (max(n_bd, 1) * W), 4),
                      "mean_leaves": {k: round(float(v.sum(-1).mean()), 2) for k, v in inds1.items()}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
