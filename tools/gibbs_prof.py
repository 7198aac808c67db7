"""Cost of Gibbs parameter blocks in hens_step (include/hipensemble.h: hens_set_gibbs) against the same context on the copying
launches without a table.

  HENS_NO_FUSED=1 python tools/gibbs_prof.py [--steps K] [--warmup W] [--shape 16x4096x32] [--rounds 3]

Three contexts of one shape (default: config 2, 16 x 4096 x 32, bench.py's dense Gaussian) in ONE process, measured alternately,
``--rounds`` times each: "none" - no table, so with HENS_NO_FUSED=1 the three copying launches per iteration (two half-steps of
k_stretch_fast, the cascade); "2x16" - two blocks of 16 coordinates; "32x1" - 32 blocks of one coordinate.  A context with a table
steps per block a plan of the block's draws (k_plan_block) and the two copying half-steps of k_stretch_prior<GIBBS>, then one
cascade.  Prints one JSON line per (round, table): microseconds per iteration of bench.py's block protocol (median block of
timed_blocks), and per launch from the event pairs of hens_set_profiling 1 in a call of its own; then one summary line with each
table's median over the rounds and its ratio to "none".  The expectation it confirms or corrects: B blocks cost about B copying
pairs plus one cascade."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the block protocol: timed_blocks, step_seconds)


def make_engine(table, T, W, D, seed=2024):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves.tempering import make_ladder
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    mu, invcov = np.full(D, 5.0), np.linalg.inv(A @ A.T / D + np.eye(D))
    eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), np.full(D, -50.0), np.full(D, 50.0), seed=seed)
    eng.upload(mu + np.random.RandomState(1).randn(T, W, D), betas=make_ladder(D, ntemps=T))
    eng.eval_state()
    if table != "none":
        nb, n = (int(v) for v in table.split("x"))
        masks = np.zeros((nb, D), dtype=bool)
        for b in range(nb):
            masks[b, (b * n) % D:(b * n) % D + n] = True
        eng.set_gibbs("stretch", masks)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--shape", default="16x4096x32")
    ap.add_argument("--tables", default="none,2x16,32x1")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("gibbs_prof.py measures on the GPU: none found")
    T, W, D = (int(v) for v in args.shape.split("x"))
    tables = args.tables.split(",")
    engs = {t: make_engine(t, T, W, D) for t in tables}
    for eng in engs.values():
        eng.step(args.warmup)
        eng.synchronize()
    us = {t: [] for t in tables}
    for rnd in range(args.rounds):
        for t in tables:                                 # alternating: every table in every round
            eng = engs[t]
            times, _ = bench.timed_blocks(eng.step, eng.synchronize, args.steps)
            dt = bench.step_seconds(times, args.steps)
            eng.set_profiling(1)
            eng.step(4)
            eng.synchronize()
            tm = eng.timing()
            eng.set_profiling(0)
            c = eng.counters()
            us[t].append(dt * 1e6)
            print(json.dumps({"shape": args.shape, "table": t, "round": rnd, "no_fused": bool(os.environ.get("HENS_NO_FUSED")),
                              "us_per_iteration": dt * 1e6,
                              "launches_per_iteration": {k: tm[k] / 4 for k in ("n_stretch", "n_pt", "n_fused")},
                              "us_per_stretch_launch": tm["stretch_ms"] * 1e3 / max(tm["n_stretch"], 1),
                              "us_per_pt_launch": tm["pt_ms"] * 1e3 / max(tm["n_pt"], 1),
                              "accept_per_block_proposal": float(c["accepted"].mean() / max(c["num_proposals"], 1)),
                              "timing": bench.timing_label(args.steps)}), flush=True)
    med = {t: float(np.median(v)) for t, v in us.items()}
    print(json.dumps({"summary": args.shape, "median_us_per_iteration": med,
                      "ratio_to_none": {t: med[t] / med[tables[0]] for t in tables}}), flush=True)
    for eng in engs.values():
        eng.close()


if __name__ == "__main__":
    main()
