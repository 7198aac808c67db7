"""What Gibbs blocks over branches and leaf slots cost the in-model move of hens_rj_step at config 4's shape (8 x 2048 walkers, pulses x 10
+ sines x 10, 500 data points on a linspace, bench.py's model and start), and what they do to its accept rate.

  python tools/rj_gibbs_prof.py --blocks none|branch|slot [--iters 200] [--runs 3]
      none     no table: the k_rj<RJ_MODE_MH, 0> launch on every active leaf (k_rj's text is not touched by the table's code: this IS
               the launch of a build without it)
      branch   one block per branch (2 blocks): ONE k_rj_gibbs launch walks both
      slot     one block per leaf slot (20 blocks): ONE k_rj_gibbs launch walks all
  The schedule is "none" (no birth / death move): an iteration is the in-model launch and its swap cascade, nothing else, so the
  difference between two settings' wall-clock time per iteration is the difference between their in-model launches.  (The leaf-packing
  launches go through the HIP stream, not the context's AQL queue: there are no dispatch timestamps to read for them.)  The leaf masks
  are those the plain chain has after a 100-iteration warm-up WITH birth / death, the same for the three settings.
  One JSON line: microseconds per iteration of `runs` timed calls of step(iters), their median; the in-model accept rate per PROPOSAL
  (a block is a proposal) over all rungs and on the cold rung; and the largest relative distance of the resident log-likelihoods
  (updated leaf by leaf) from a full evaluation after 63 iterations without a refresh.
Each setting is one process; on a shared GPU run them one after the other, each under a time limit of its own.
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
    ap.add_argument("--blocks", required=True, choices=["none", "branch", "slot"])
    ap.add_argument("--iters", type=int, default=200)
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
    eng.set_schedule("separate_branches")
    eng.step(100)                                               # warm-up with birth / death: the leaf counts settle
    eng.synchronize()
    eng.set_schedule("none")
    ncoord = 2 * NL * 3
    if args.blocks == "branch":
        table = np.zeros((2, ncoord), dtype=bool)
        table[0, :NL * 3] = table[1, NL * 3:] = True
    elif args.blocks == "slot":
        table = np.repeat(np.eye(2 * NL, dtype=bool), 3, axis=1)
    if args.blocks != "none":
        eng.set_gibbs(table)
    nb = 1 if args.blocks == "none" else table.shape[0]
    eng.step(20)
    eng.synchronize()
    c0 = eng.counters()
    per = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        eng.step(args.iters)
        eng.synchronize()
        per.append((time.perf_counter() - t0) / args.iters * 1e6)
    c = eng.counters()
    n_mh = c["num_mh"] - c0["num_mh"]
    assert n_mh == nb * args.iters * args.runs
    # the drift of the leaf-by-leaf updates: from a fresh evaluation (the download) at iteration 64 k to iteration 64 k + 63, no refresh between
    eng.download()
    it = eng.iteration()
    eng.set_iteration((it // 64 + 1) * 64)
    eng.step(63)
    _, _, Lr = eng.debug_resident()
    _, inds1, L1, _, _ = eng.download()
    drift = float(np.max(np.abs(Lr - L1) / np.abs(L1)))
    acc = c["accepted_mh"] - c0["accepted_mh"]
    print(json.dumps({"blocks": args.blocks, "nblocks": nb, "shape": f"{T} x {W}, {NL} + {NL} leaves, {N} points", "iters_per_run": args.iters,
                      "us_per_iteration": [round(v, 2) for v in per], "median_us": round(float(np.median(per)), 2),
                      "accept_per_proposal": round(float(acc.sum()) / (n_mh * T * W), 4),
                      "accept_per_proposal_cold_rung": round(float(acc[0].sum()) / (n_mh * W), 4),
                      "resident_logl_drift_63_iterations": drift,
                      "mean_leaves": {k: round(float(v.sum(-1).mean()), 2) for k, v in inds1.items()}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
