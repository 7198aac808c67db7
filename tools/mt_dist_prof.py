"""What the multiple-try independence move costs at config 2's shape (16 x 4096 x 32, dense Gaussian, box prior, a generator of
normal terms), from the launches' own stamps (hens_set_profiling): one iteration of MTDistGenMove at num_try = 4 / 16 / 64 against
num_try iterations of DistributionGenerate - the same number of rows drawn and evaluated, in one launch with one read of the
walker's own row instead of num_try launches - both at weight 1, alternated, three runs each.
  the move's launch : median duration of the iteration's first launch (k_mt_dist / k_dist)
  the iteration     : (end of the call's last launch - begin of its first) / iterations, the swap cascade included
  python tools/mt_dist_prof.py [iterations per run, default 100]
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eryn_amd.engine import HipEnsemble                    # noqa: E402
from eryn_amd.likelihood import GaussianLikelihood         # noqa: E402
from eryn_amd.moves.tempering import make_ladder           # noqa: E402
from eryn_amd.prior import NormalDistribution, ProbDistContainer   # noqa: E402

T, W, D = 16, 4096, 32
N = int(sys.argv[1]) if len(sys.argv) > 1 else 100
TRIES = (4, 16, 64)


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
    configs = {"DistributionGenerate": lambda: eng.set_dist_proposal(gen, 1.0)}
    for K in TRIES:
        configs[f"MTDistGenMove num_try={K}"] = lambda K=K: eng.set_mt_dist_proposal(gen, K, 1.0)
    it_us, move_us, rate = ({k: [] for k in configs} for _ in range(3))
    for run in range(3):
        for name, setup in configs.items():
            eng.upload(x0, betas=betas)
            eng.eval_state()
            eng.set_iteration(0)
            eng.set_adapt_time(0)
            setup()
            eng.set_profiling(False)
            eng.step(20)                                   # warm-up: the kernels' first launches, the walkers off their start
            eng.synchronize()
            acc0 = eng.mh_counters()["accepted"].sum()
            eng.set_profiling(True)
            eng.step(N)
            eng.synchronize()
            lt = eng.launch_times()
            eng.set_profiling(False)
            assert lt.shape[0] == 2 * N, f"{name}: {lt.shape[0]} launches for {N} iterations (the move's launch and the cascade expected)"
            it_us[name].append((lt[-1, 1] - lt[0, 0]) / N)
            move_us[name].append(float(np.median(lt[0::2, 1] - lt[0::2, 0])))
            rate[name].append((eng.mh_counters()["accepted"].sum() - acc0) / (N * T * W))
            print(f"run {run}  {name:28s} iteration {it_us[name][-1]:9.2f} us   the move's launch {move_us[name][-1]:9.2f} us   "
                  f"accept rate {rate[name][-1]:.3f}", flush=True)
    print()
    base_it, base_mv = np.median(it_us["DistributionGenerate"]), np.median(move_us["DistributionGenerate"])
    print(f"{'DistributionGenerate':28s} iteration median {base_it:9.2f} us   launch median {base_mv:9.2f} us   accept rate {np.median(rate['DistributionGenerate']):.3f}")
    for K in TRIES:
        name = f"MTDistGenMove num_try={K}"
        i, m = np.median(it_us[name]), np.median(move_us[name])
        print(f"{name:28s} iteration median {i:9.2f} us = {i / (K * base_it):.3f} x {K} DistributionGenerate iterations   "
              f"launch median {m:9.2f} us = {m / (K * base_mv):.3f} x {K} k_dist launches   accept rate {np.median(rate[name]):.3f}")
    eng.close()


if __name__ == "__main__":
    main()
