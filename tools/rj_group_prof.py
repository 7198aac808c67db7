"""What the group stretch move costs the in-model slot of hens_rj_step at config 4's shape (8 x 2048 walkers, pulses x 10 + sines x 10,
500 data points on a linspace, bench.py's model and start) beside the two in-model moves the project had, and what it accepts.

  python tools/rj_group_prof.py [--iters 200] [--runs 3] [--rebuilds 20]

ONE process, the settings ALTERNATING inside every run (other people's work shares the host: a difference is trusted only between
neighbours): the Gaussian move (k_rj<RJ_MODE_MH, 0>), the red / blue stretch move (two k_rj<RJ_MODE_STRETCH, 0> launches), and the
group stretch move (one k_rj<RJ_MODE_GROUP, 0> launch) with nfriends = 4 / 16 / 64, n_iter_update larger than the timed window so
that no rebuild falls into it.  The schedule is "none" (no birth / death move): an iteration is the in-model launch(es) and the swap
cascade, nothing else, so the difference between two settings' wall clock per iteration is the difference between their in-model
launches.  (The leaf-packing launches go through the HIP stream: there are no dispatch timestamps to read for them.)  The leaf masks
are those the plain chain has after a 100-iteration warm-up WITH birth / death.  Every timed window follows 10 untimed iterations of
its own setting and ends in a device synchronise.

A rebuild (count / scan / gather, rank sort, every rung's windows: three launches) is timed on its own: ``--rebuilds`` calls of
hens_rj_group_rebuild, each ended by a synchronise; its share at n_iter_update = 100 is rebuild / (100 group iterations + rebuild).

One JSON line: microseconds per iteration per setting (every run, and the median), the accept rate per proposal over all rungs and on
the cold rung, microseconds per rebuild and its share, the table's lengths."""
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
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--rebuilds", type=int, default=20)
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
    far = 10 ** 9                                               # (n_iter_update: one rebuild when the group is set, none in a window)
    settings = [("gaussian", None), ("stretch", None), ("group_4", 4), ("group_16", 16), ("group_64", 64)]

    def select(name, nf):
        if nf is None:
            eng.set_in_model(name)
        else:
            eng.set_group(nf, far, 1, 2.0)                      # key: the pulse's centre, the sine's frequency
            eng.set_in_model("group")

    per = {s: [] for s, _ in settings}
    acc = {s: np.zeros((T, W)) for s, _ in settings}
    nprop = {s: 0 for s, _ in settings}
    for _ in range(args.runs):
        for name, nf in settings:
            select(name, nf)
            eng.step(10)
            eng.synchronize()
            c0 = eng.counters()
            t0 = time.perf_counter()
            eng.step(args.iters)
            eng.synchronize()
            per[name].append((time.perf_counter() - t0) / args.iters * 1e6)
            c = eng.counters()
            acc[name] += c["accepted_mh"] - c0["accepted_mh"]
            nprop[name] += c["num_mh"] - c0["num_mh"]
    # one rebuild, on its own
    select("group_16", 16)
    eng.step(1)
    eng.synchronize()
    reb = []
    for _ in range(args.rebuilds):
        t0 = time.perf_counter()
        eng.group_rebuild()
        eng.synchronize()
        reb.append((time.perf_counter() - t0) * 1e6)
    g = eng.group_debug()
    med = {s: float(np.median(v)) for s, v in per.items()}
    reb_us = float(np.median(reb))
    _, inds1, _, _, _ = eng.download()
    print(json.dumps({
        "shape": f"{T} x {W}, {NL} + {NL} leaves, {N} points", "iters_per_window": args.iters,
        "us_per_iteration": {s: [round(v, 2) for v in per[s]] for s in per}, "median_us": {s: round(v, 2) for s, v in med.items()},
        "accept_per_proposal": {s: round(float(acc[s].sum()) / (nprop[s] * T * W), 4) for s in per},
        "accept_per_proposal_cold_rung": {s: round(float(acc[s][0].sum()) / (nprop[s] * W), 4) for s in per},
        "rebuild_us": [round(v, 1) for v in reb], "rebuild_median_us": round(reb_us, 1),
        "rebuild_share_at_n_iter_update_100": round(reb_us / (100 * med["group_16"] + reb_us), 5),
        "table_entries": {b.name: int(g["counts"][i]) for i, b in enumerate(brs)},
        "mean_leaves": {k: round(float(v.sum(-1).mean()), 2) for k, v in inds1.items()}}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
