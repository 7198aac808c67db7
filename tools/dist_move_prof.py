"""What the draw-from-distribution move costs at config 2's shape (16 x 4096 x 32, dense Gaussian, box prior, a generator of normal
terms), from the launches' own stamps (hens_set_profiling):
  (a) the stretch move alone, (b) the mix with GaussianMove at weight 0.5, (c) the mix with DistributionGenerate at weight 0.5 -
  alternated, three runs each; us per iteration = (end of the call's last launch - begin of its first) / iterations.
The comparison that matters is (c) against (b): the same iteration structure with another proposal.  The move's own launch is
reported alone against the bytes it must move: 8 D + 32 read per walker, 8 D written per accepted one.
  python tools/dist_move_prof.py [iterations per run, default 200]
"""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eryn_amd.engine import HipEnsemble                    # noqa: E402
from eryn_amd.likelihood import GaussianLikelihood         # noqa: E402
from eryn_amd.moves.tempering import make_ladder           # noqa: E402
from eryn_amd.prior import NormalDistribution, ProbDistContainer   # noqa: E402

T, W, D = 16, 4096, 32
N = int(sys.argv[1]) if len(sys.argv) > 1 else 200


def is_mh(eng, it):
    flag = C.c_int32(0)
    eng.lib.hens_debug_draws(eng.ctx, int(it), None, None, None, None, None, None, C.byref(flag), None, None)
    return bool(flag.value)


def main():
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    mu = 0.1 * rs.randn(D)
    cov = A @ A.T / D + np.eye(D)
    sig = np.sqrt(np.diag(cov))
    eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, np.linalg.inv(cov)), -50.0, 50.0, seed=11)
    gen = ProbDistContainer({d: NormalDistribution(mu[d], 1.2 * sig[d]) for d in range(D)})
    x0 = np.random.RandomState(1).randn(T, W, D)
    betas = make_ladder(D, ntemps=T)
    configs = {
        "a stretch alone": lambda: eng.set_mh_proposal(None, None, 0.0),
        "b mix GaussianMove 0.5": lambda: eng.set_mh_proposal("iso", 0.05, 0.5),
        "c mix DistributionGenerate 0.5": lambda: eng.set_dist_proposal(gen, 0.5),
    }
    res = {k: [] for k in configs}
    move_us = {k: [] for k in configs}
    traffic = []
    for run in range(3):
        for name, setup in configs.items():
            eng.upload(x0, betas=betas)
            eng.eval_state()
            eng.set_iteration(0)
            eng.set_adapt_time(0)
            setup()
            eng.set_profiling(False)
            eng.step(50)                                   # warm-up: the packed state, the kernels' first launches
            eng.synchronize()
            acc0 = eng.mh_counters()["accepted"].sum()
            it0 = eng.iteration()
            eng.set_profiling(True)
            eng.step(N)
            eng.synchronize()
            lt = eng.launch_times()
            eng.set_profiling(False)
            res[name].append((lt[-1, 1] - lt[0, 0]) / N)
            if name[0] != "a" and lt.shape[0] == 2 * N:    # two launches per iteration either way: the move's is an MH iteration's first
                mh = np.array([is_mh(eng, it) for it in range(it0, it0 + N)])
                dur = (lt[0::2, 1] - lt[0::2, 0])[mh]
                move_us[name].append(float(np.median(dur)))
                if name[0] == "c":
                    nacc = eng.mh_counters()["accepted"].sum() - acc0
                    byts = mh.sum() * T * W * (8 * D + 32) + nacc * 8 * D
                    traffic.append((float(np.median(dur)), byts / mh.sum(), nacc / (mh.sum() * T * W)))
            print(f"run {run}  {name:32s} {res[name][-1]:8.2f} us / iteration   ({lt.shape[0]} launches)", flush=True)
    print()
    for name in configs:
        v = res[name]
        print(f"{name:32s} us / iteration: " + "  ".join(f"{x:.2f}" for x in v) + f"   median {np.median(v):.2f}")
    for name in configs:
        if move_us[name]:
            print(f"{name:32s} the move's own launch, median us: " + "  ".join(f"{x:.2f}" for x in move_us[name]))
    for us, byts, rate in traffic:
        print(f"k_dist alone: {us:.2f} us for {byts / 1e6:.2f} MB it must move ({T} x {W} walkers x (8 D + 32) B read + 8 D B per accepted walker, "
              f"accept rate {rate:.3f}) = {byts / us / 1e6:.2f} TB/s")
    eng.close()


if __name__ == "__main__":
    main()
