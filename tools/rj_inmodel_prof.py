"""Cost of the in-model move of hens_rj_step at BASELINE config 4's shape (8 x 2048 walkers, 2 branches x 10 leaves, 500 data
points; W = 2048 >= 2 x 60 coordinates): Gaussian with a diagonal covariance, Gaussian with a full covariance, red / blue stretch.

  python tools/rj_inmodel_prof.py [--steps K] [--warmup W] [--moves diag,full,stretch] [--schedule separate_branches|none]

prints one JSON line per move with the microseconds per iteration of bench.py's block protocol (median block of timed_blocks).
Per-kernel averages come from a run of its own under the profiler:

  rocprofv3 --kernel-trace --stats -d OUT -- python tools/rj_inmodel_prof.py --moves stretch --steps 200

(tracing slows the host: take the per-iteration figures with the profiler off)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the block protocol: timed_blocks, step_seconds)


def make_engine(move, schedule, T=8, W=2048, N=500, NL=10):
    """bench.py run_cfg4's model and starting state, with the in-model move under measurement."""
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import RJEngine, TemplateBranch
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
    scale = np.full((2, 3), 1e-2) * [[1, 1, 0.1], [1, 1, 1]]
    if move == "diag":
        eng.set_mh_scale(scale)
    elif move == "full":
        unit = np.array([[1.0, 0.0, 0.0], [0.5, 0.8, 0.0], [-0.3, 0.4, 0.7]])
        eng.set_mh_chol(scale[:, :, None] * unit)
    elif move == "stretch":
        eng.set_in_model("stretch")
    else:
        raise SystemExit(f"unknown move {move}")
    eng.set_schedule(schedule)
    return eng


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--moves", default="diag,full,stretch")
    ap.add_argument("--schedule", default="separate_branches")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rj_inmodel_prof.py measures on the GPU: none found")
    for move in args.moves.split(","):
        eng = make_engine(move, args.schedule)
        eng.step(args.warmup)
        eng.synchronize()
        times, _ = bench.timed_blocks(eng.step, eng.synchronize, args.steps)
        dt = bench.step_seconds(times, args.steps)
        c = eng.counters()
        print(json.dumps({"move": move, "schedule": args.schedule, "us_per_iteration": dt * 1e6,
                          "block_us_per_iteration": [t_ / k * 1e6 for t_, k in zip(times, bench.block_sizes(args.steps))],
                          "accept_in_model": float(c["accepted_mh"].mean() / max(c["num_mh"], 1)),
                          "accept_birth_death": float(c["accepted_bd"].mean() / max(c["num_bd"], 1)),
                          "timing": bench.timing_label(args.steps)}), flush=True)
        eng.close()


if __name__ == "__main__":
    main()
