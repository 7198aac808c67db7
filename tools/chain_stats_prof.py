"""What the chain diagnostics cost where the chain is (DeviceBackend: k_chain_act / k_chain_moments, arrays the size of a stored
step come back) against the same chain read with get_chain() and pushed through eryn_amd/chain_stats.py on the host, and the two
kernels' own durations against the bytes they must read.

  python tools/chain_stats_prof.py [--nsteps 400] [--runs 3] [--shape 16,4096,32]
      config 2 (16 x 4096 x 32, dense Gaussian), `nsteps` stored steps on a DeviceBackend.  A: get_autocorr_time() and
      get_gelman_rubin_convergence_diagnostic(doprint=False) on the device chain.  B: the yardstick - the open segment downloaded
      (get_chain; the backend's cached copy is dropped before every run, so each run pays its download) and the same two accessors'
      arithmetic from chain_stats.py on the host copy.  A / B alternating, `runs` times each after one warm-up of A; one JSON line
      per accessor with the per-run milliseconds of both and the ratio of the medians, after checking that both returned the
      same bits.  Then the kernels alone from their event pairs (hens_chain_stats_ms): k_chain_act on the cold rung and on all
      rungs at window 50 - microseconds, chain bytes read (two passes), LDS bytes read (K x 8 per sample), the rates -, and
      k_chain_moments of x on all rungs - microseconds, bytes (two passes), the fraction of the HBM peak.

One process; on a shared GPU under a time limit of its own:
  timeout -k 10 900 python tools/chain_stats_prof.py > profiles/chain_stats_ab.txt
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
LDS_PEAK = 256 * 256 * 2.4e9   # bytes / s: 256 CUs x 256 B / clk (ds_read_b64) x 2.4 GHz


def same(a, b):
    if isinstance(a, dict):
        return list(a) == list(b) and all(same(a[k], b[k]) for k in a)
    return np.array_equal(a, b, equal_nan=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=400)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shape", default="16,4096,32")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_stats_prof.py measures on the GPU: none found")
    from eryn_amd import chain_stats
    from eryn_amd.backend import DeviceBackend
    from eryn_amd.ensemble import EnsembleSampler
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.prior import uniform_dist
    T, W, D = (int(v) for v in args.shape.split(","))
    n = args.nsteps
    rs = np.random.RandomState(42)
    A = rs.randn(D, D)
    mu, invcov = 0.1 * rs.randn(D), np.linalg.inv(A @ A.T / D + np.eye(D))
    s = EnsembleSampler(W, D, GaussianLikelihood(mu, invcov), {i: uniform_dist(-50.0, 50.0) for i in range(D)},
                        tempering_kwargs=dict(ntemps=T), rng="philox", seed=2024, backend=DeviceBackend())
    s.run_mcmc(mu + rs.randn(T, W, D), n)
    b, eng = s.backend, s.engine
    assert b._open == n, "the chain closed a segment: lower --nsteps"
    shape = f"{T} x {W} x {D}, {n} stored steps"

    def host_act():
        x = b.get_chain()["model_0"][:, :1, :, 0, :]
        return {"model_0": np.average(chain_stats.act(x, 50)[0], axis=1)}

    def host_gr():
        x = b.get_chain()["model_0"][:, :, :, 0, :]
        return {"model_0": {t: chain_stats.psrf(x[:, t].transpose(1, 0, 2), D) for t in range(T)}}

    for name, dev, host in (("get_autocorr_time", lambda: b.get_autocorr_time(), host_act),
                            ("get_gelman_rubin_convergence_diagnostic", lambda: b.get_gelman_rubin_convergence_diagnostic(doprint=False), host_gr)):
        dev()                                                  # warm-up: the kernels loaded
        t_dev, t_host, t_read = [], [], []
        for _ in range(args.runs):                             # A / B alternating
            eng.synchronize()
            t0 = time.perf_counter()
            got = dev()
            t_dev.append((time.perf_counter() - t0) * 1e3)
            b._cache = None                                    # (the yardstick pays its download every time)
            t0 = time.perf_counter()
            b.get_chain()
            t1 = time.perf_counter()
            want = host()
            t2 = time.perf_counter()
            t_read.append((t1 - t0) * 1e3)
            t_host.append((t2 - t0) * 1e3)
            assert same(got, want), f"{name}: the device chain and the host copy gave different bits"
        b._cache = None
        print(json.dumps({"accessor": name, "shape": shape, "device_ms": [round(v, 2) for v in t_dev],
                          "host_ms_with_download": [round(v, 1) for v in t_host], "of_which_download_ms": [round(v, 1) for v in t_read],
                          "ratio_of_medians_host_over_device": round(float(np.median(t_host) / np.median(t_dev)), 1),
                          "chain_downloads_by_the_device_path": 0, "stats_launches": b.stats_launches}), flush=True)

    for nt in (1, T):
        per = []
        for _ in range(args.runs + 1):
            eng.chain_act(0, n, 1, nt, 50)
            per.append(eng.chain_stats_ms()["act_ms"] * 1e3)
        us = float(np.median(per[1:]))
        series = nt * W * D
        hbm, lds = 2 * 8 * series * n, 8 * 50 * series * n
        print(json.dumps({"kernel": "k_chain_act", "shape": shape, "ntemps": nt, "window": 50, "us_per_launch": [round(v, 1) for v in per[1:]],
                          "median_us": round(us, 1), "chain_bytes_read": hbm, "lds_bytes_read": lds,
                          "us_at_hbm_peak": round(hbm / HBM_PEAK * 1e6, 1), "us_at_lds_peak": round(lds / LDS_PEAK * 1e6, 1),
                          "fraction_of_lds_peak": round(lds / (us * 1e-6) / LDS_PEAK, 3)}), flush=True)
    per = []
    for _ in range(args.runs + 1):
        eng.chain_moments("x", 0, n, 1, T)
        per.append(eng.chain_stats_ms()["moments_ms"] * 1e3)
    us = float(np.median(per[1:]))
    hbm = 2 * 8 * T * W * D * n
    print(json.dumps({"kernel": "k_chain_moments", "shape": shape, "field": "x", "ntemps": T, "us_per_launch": [round(v, 1) for v in per[1:]],
                      "median_us": round(us, 1), "chain_bytes_read": hbm, "us_at_hbm_peak": round(hbm / HBM_PEAK * 1e6, 1),
                      "GB_per_s": round(hbm / us * 1e-3, 1), "fraction_of_hbm_peak": round(hbm / (us * 1e-6) / HBM_PEAK, 3)}), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
