"""What a stored step costs with the chain on the host (Backend: a download per stored step) and on the device (DeviceBackend:
k_chain_store between the stepping launches, one download at the end), and k_chain_store's own duration.

  python tools/chain_store_prof.py --part a [--nsteps 400] [--thin 1,10] [--runs 3]
      config 2 (16 x 4096 x 32, dense Gaussian): run_mcmc(nsteps, thin_by, store=True) under Backend and under DeviceBackend,
      alternating A / B, `runs` times each after a warm-up run of each; the state is resident (run_mcmc(None, ...) continues
      the sampler's own last State), the final download (the first accessor) is timed apart.  One JSON line per (thin_by, backend)
      with the per-run microseconds per stored step, their median, the median over and above thin_by x t_iter (t_iter: a
      store=False run of the same length on the same sampler), and one line per thin_by with the ratio of the two overheads.
  python tools/chain_store_prof.py --part b [--stores 50]
      k_chain_store alone, from the event pair hens_set_profiling(ctx, 1) puts around every append launch (the iterations between
      them step on the HIP stream then: their timing is not this part's subject), at config 2's shape and config 5's (32 x 8192 x
      128, Rosenbrock): microseconds per launch, bytes it must move - T W (32 + 8 RW) read, 8 T W (D + 2) written - and the rate.

  python tools/chain_store_prof.py --rj [--nsteps 200] [--thin 1,10] [--runs 3] [--stores 50]
      the leaf-packing sampler's chain (RJEngine; hens_rj_step_chain, k_rj_chain_store) at config 4's shape (8 x 2048 walkers, pulses x 10
      + sines x 10: records of 62 doubles, 500 data points) and at one small shape (4 x 64, 3 + 4 leaves, 60 points): a stored step on
      the host path - step(thin_by), download, unpack with the NaN fill, a State - and on the device path - one step_chain call for
      the run, one chain_download behind it (timed apart) -, both over and above `nsteps` bare step(thin_by) calls, A / B alternating;
      then k_rj_chain_store alone from the event pairs of hens_set_profiling(ctx, 1) (n_store_timed / store_ms): microseconds per
      launch, the bytes it must move and the rate against the HBM peak.

Each part is one process; on a shared GPU run them one after the other, each under a time limit of its own:
  timeout -k 10 600 python tools/chain_store_prof.py --part a > profiles/chain_store_ab.txt && \\
  timeout -k 10 300 python tools/chain_store_prof.py --part b >> profiles/chain_store_ab.txt
  timeout -k 10 600 python tools/chain_store_prof.py --rj > profiles/rj_chain_store_ab.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12          # bytes / s, MI355X data sheet


def make_sampler(backend, T=16, W=4096, D=32, seed=2024):
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.prior import uniform_dist
    rs = np.random.RandomState(42)
    A = rs.randn(D, D)
    mu, invcov = 0.1 * rs.randn(D), np.linalg.inv(A @ A.T / D + np.eye(D))
    priors = {i: uniform_dist(-50.0, 50.0) for i in range(D)}
    s = EnsembleSampler(W, D, GaussianLikelihood(mu, invcov), priors, tempering_kwargs=dict(ntemps=T), rng="philox", seed=seed,
                        backend=backend)
    return s, mu + rs.randn(T, W, D)


def timed_run(s, nsteps, thin, store=True):
    """(seconds of run_mcmc, seconds of the first read of the chain behind it); the engine is idle on both ends"""
    s.engine.synchronize()
    t0 = time.perf_counter()
    s.run_mcmc(None, nsteps, thin_by=thin, store=store)
    s.engine.synchronize()
    t1 = time.perf_counter()
    if store:
        s.get_log_like()
    return t1 - t0, time.perf_counter() - t1


def part_a(args):
    from eryn_amd.backend import Backend, DeviceBackend
    n = args.nsteps or 400
    for thin in [int(t) for t in args.thin.split(",")]:
        samplers = {}
        for name, bk in (("Backend", Backend()), ("DeviceBackend", DeviceBackend())):
            s, x0 = make_sampler(bk)
            s.run_mcmc(x0, 20, thin_by=thin)                   # warm-up: kernels loaded, buffers made, the state resident
            samplers[name] = s
        runs = {name: dict(store=[], read=[], bare=[]) for name in samplers}
        for _ in range(args.runs):
            for name, s in samplers.items():                   # A / B alternating
                s.backend.reset(s.nwalkers, s.ndims, ntemps=s.ntemps, branch_names=s.branch_names)
                dt, rd = timed_run(s, n, thin)
                runs[name]["store"].append(dt / n * 1e6)
                runs[name]["read"].append(rd * 1e3)
                runs[name]["bare"].append(timed_run(s, n, thin, store=False)[0] / n * 1e6)
        over = {}
        for name, r in runs.items():
            med, bare = float(np.median(r["store"])), float(np.median(r["bare"]))
            over[name] = med - bare
            print(json.dumps({"part": "a", "shape": "16 x 4096 x 32", "nsteps": n, "thin_by": thin, "backend": name,
                              "us_per_stored_step": [round(v, 2) for v in r["store"]], "median_us_per_stored_step": round(med, 2),
                              "us_per_stored_step_without_store": [round(v, 2) for v in r["bare"]],
                              "overhead_us_per_stored_step": round(med - bare, 2),
                              "first_read_ms": [round(v, 2) for v in r["read"]]}), flush=True)
        print(json.dumps({"part": "a", "thin_by": thin, "overhead_ratio_host_over_device": round(over["Backend"] / max(over["DeviceBackend"], 1e-9), 1)}),
              flush=True)
        for s in samplers.values():
            s.engine.close()


def part_b(args):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, RosenbrockLikelihood
    from eryn_amd.moves.tempering import make_ladder
    for label, T, W, D, rosen in (("config 2", 16, 4096, 32, False), ("config 5", 32, 8192, 128, True)):
        rs = np.random.RandomState(42)
        if rosen:
            eng = HipEnsemble(T, W, D, RosenbrockLikelihood(D), -5.0, 5.0, seed=2024)
            x0 = 1.0 + 0.1 * rs.randn(T, W, D)
        else:
            A = rs.randn(D, D)
            eng = HipEnsemble(T, W, D, GaussianLikelihood(0.1 * rs.randn(D), np.linalg.inv(A @ A.T / D + np.eye(D))), -50.0, 50.0, seed=2024)
            x0 = rs.randn(T, W, D)
        eng.upload(x0, betas=make_ladder(D, ntemps=T))
        eng.eval_state()
        stores = args.stores if not rosen else max(4, args.stores // 5)
        eng.chain_create(stores)
        eng.step_chain(min(4, stores), 1, 1)                   # warm-up
        eng.chain_reset()
        eng.set_profiling(1)
        per = []
        for _ in range(args.runs):
            eng.chain_reset()
            eng.step_chain(stores, 1, 1)
            info = eng.chain_info()
            per.append(info["store_ms"] / max(info["n_store_timed"], 1) * 1e3)
        rd, wr = T * W * (32 + 8 * eng.RW), 8 * T * W * (D + 2)
        us = float(np.median(per))
        print(json.dumps({"part": "b", "shape": f"{label}: {T} x {W} x {D}", "stores_per_run": stores, "us_per_launch": [round(v, 2) for v in per],
                          "median_us": round(us, 2), "bytes_read": rd, "bytes_written": wr, "GB_per_s": round((rd + wr) / us * 1e-3, 1),
                          "fraction_of_hbm_peak": round((rd + wr) / (us * 1e-6) / HBM_PEAK, 3)}), flush=True)
        eng.close()


def make_rj_engine(T, W, NL, N, seed=2024):
    """bench.py's config-4 problem at any shape: pulses + sines, NL = (pulse slots, sine slots), N data points; warmed up."""
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import RJEngine, TemplateBranch
    t = np.linspace(-1, 1, N)
    rs = np.random.RandomState(42)
    gauss_inj = np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1], [3.4, 0.0, 0.1], [2.9, 0.3, 0.1]])
    sine_inj = np.array([[1.3, 10.1, 1.0], [0.8, 4.6, 1.2]])
    y = sum(a * np.exp(-((t - b) ** 2) / (2 * c ** 2)) for a, b, c in gauss_inj) + \
        sum(a * np.sin(2 * np.pi * b * t + c) for a, b, c in sine_inj) + 2.0 * rs.randn(N)
    brs = [TemplateBranch("gauss", "pulse", [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], NL[0], 0),
           TemplateBranch("sine", "sine", [(0.5, 1.5), (1.0, 20.0), (0.0, 2 * np.pi)], NL[1], 0)]
    eng = RJEngine(T, W, brs, t, y, 2.0, seed=seed)
    x = {"gauss": np.zeros((T, W, NL[0], 3)), "sine": np.zeros((T, W, NL[1], 3))}
    inds = {k: np.zeros(v.shape[:3], dtype=bool) for k, v in x.items()}
    for n in range(min(4, NL[0])):
        x["gauss"][:, :, n] = gauss_inj[n] + 1e-2 * rs.randn(T, W, 3) * [1, 1, 0.1]
        inds["gauss"][:, :, n] = True
    for n in range(min(2, NL[1])):
        x["sine"][:, :, n] = sine_inj[n] + 1e-2 * rs.randn(T, W, 3)
        inds["sine"][:, :, n] = True
    eng.upload(x, inds, betas=make_ladder(18, ntemps=T))
    eng.eval_state()
    eng.set_mh_scale(np.full((2, 3), 1e-2) * [[1, 1, 0.1], [1, 1, 1]])
    eng.step(100)
    eng.synchronize()
    return eng


def part_rj(args):
    from eryn_amd.state import State
    n = args.nsteps or 200

    def host_run(eng, thin):                                   # RJEnsembleSampler.run_mcmc(store=True) without backend=
        chain = []
        for _ in range(n):
            eng.step(thin)
            x, inds, L, P, betas = eng.download(nan_fill=True)
            chain.append(State(x, inds=inds, log_like=L, log_prior=P, betas=betas))
        return chain

    def device_run(eng, thin):                                 # ... with backend=RJDeviceBackend()
        eng.chain_reset()
        eng.step_chain(n, thin)

    def bare_run(eng, thin):
        for _ in range(n):
            eng.step(thin)

    def timed(fn, eng, thin):
        eng.synchronize()
        t0 = time.perf_counter()
        fn(eng, thin)
        eng.synchronize()
        return (time.perf_counter() - t0) / n * 1e6

    for label, T, W, NL, N in (("config 4: 8 x 2048, 10 + 10 leaves", 8, 2048, (10, 10), 500), ("small: 4 x 64, 3 + 4 leaves", 4, 64, (3, 4), 60)):
        eng = make_rj_engine(T, W, NL, N)
        eng.chain_create(max(n, args.stores))
        info = eng.chain_info()
        for thin in [int(t) for t in args.thin.split(",")]:
            for fn in (host_run, device_run, bare_run):        # warm-up of each
                timed(fn, eng, thin)
            runs = dict(host=[], device=[], bare=[], read_ms=[])
            for _ in range(args.runs):                         # A / B alternating
                runs["host"].append(timed(host_run, eng, thin))
                runs["device"].append(timed(device_run, eng, thin))
                t0 = time.perf_counter()
                eng.chain_download(0, n)
                runs["read_ms"].append((time.perf_counter() - t0) * 1e3)
                runs["bare"].append(timed(bare_run, eng, thin))
            med = {k: float(np.median(v)) for k, v in runs.items()}
            print(json.dumps({"part": "rj", "shape": label, "nsteps": n, "thin_by": thin, "step_bytes": info["step_bytes"],
                              "us_per_stored_step_host": [round(v, 2) for v in runs["host"]],
                              "us_per_stored_step_device": [round(v, 2) for v in runs["device"]],
                              "us_per_stored_step_without_store": [round(v, 2) for v in runs["bare"]],
                              "overhead_us_host": round(med["host"] - med["bare"], 2), "overhead_us_device": round(med["device"] - med["bare"], 2),
                              "overhead_ratio_host_over_device": round((med["host"] - med["bare"]) / max(med["device"] - med["bare"], 1e-9), 1),
                              "one_read_of_the_chain_ms": [round(v, 2) for v in runs["read_ms"]]}), flush=True)
        # the append launch alone
        eng.eng.set_profiling(1)
        per = []
        for _ in range(args.runs):
            eng.chain_reset()
            eng.step_chain(args.stores, 1)
            i = eng.chain_info()
            assert i["n_store_timed"] == args.stores
            per.append(i["store_ms"] / i["n_store_timed"] * 1e3)
        eng.eng.set_profiling(0)
        rd, wr = T * W * (8 * eng.RW + 4 + 16 + 16), info["step_bytes"]      # record, loc, L / P, two counters and their marks | the step
        us = float(np.median(per))
        print(json.dumps({"part": "rj", "kernel": "k_rj_chain_store", "shape": label, "stores_per_run": args.stores,
                          "us_per_launch": [round(v, 2) for v in per], "median_us": round(us, 2), "bytes_read": rd, "bytes_written": wr,
                          "us_at_hbm_peak": round((rd + wr) / HBM_PEAK * 1e6, 3), "GB_per_s": round((rd + wr) / us * 1e-3, 1),
                          "fraction_of_hbm_peak": round((rd + wr) / (us * 1e-6) / HBM_PEAK, 4)}), flush=True)
        eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=["a", "b"])
    ap.add_argument("--rj", action="store_true", help="the leaf-packing sampler's chain (hens_rj_step_chain, k_rj_chain_store)")
    ap.add_argument("--nsteps", type=int, default=None, help="stored steps per run (default: 400; --rj: 200)")
    ap.add_argument("--thin", default="1,10")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--stores", type=int, default=50)
    args = ap.parse_args()
    if not args.rj and not args.part:
        ap.error("--part a | b, or --rj")
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_store_prof.py measures on the GPU: none found")
    if args.rj:
        return part_rj(args)
    (part_a if args.part == "a" else part_b)(args)


if __name__ == "__main__":
    main()
