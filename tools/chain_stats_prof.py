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

  python tools/chain_stats_prof.py --rj [--nsteps 400] [--runs 3]
      the reversible-jump chain at config 4's shape (8 x 2048 walkers, pulses x 10 + sines x 10: tools/chain_store_prof.py's
      problem), `nsteps` stored steps on an RJDeviceBackend.  A: get_nleaves_counts(), get_nleaves(download=False) and
      get_gelman_rubin_convergence_diagnostic(doprint=False) on the device chain (k_rj_chain_leaves, k_rj_chain_leaf_moments).
      B: the open segment downloaded (get_chain / get_inds, the cached copy dropped before every run) and chain_stats.leaf_counts /
      rj_psrf on the host copy.  A / B alternating, one JSON line per accessor, after checking that both returned the same bits.
      Then the two kernels alone from their event pairs (hens_rj_chain_stats_ms) against the bytes they must read.

One process; on a shared GPU under a time limit of its own:
  timeout -k 10 900 python tools/chain_stats_prof.py > profiles/chain_stats_ab.txt
  timeout -k 10 900 python tools/chain_stats_prof.py --rj > profiles/rj_chain_stats_ab.txt
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


def part_rj(args):
    from chain_store_prof import make_rj_engine
    from eryn_amd import chain_stats
    from eryn_amd.backend import RJDeviceBackend
    T, W, NL, n = 8, 2048, (10, 10), args.nsteps
    eng = make_rj_engine(T, W, NL, 500)
    names = [b.name for b in eng.branches]
    b = RJDeviceBackend()
    b.attach(eng, 2024)
    b.reset(W, {k: 3 for k in names}, ntemps=T, branch_names=names, nleaves_max=dict(zip(names, NL)))
    b.append(n, 1)
    assert b._open == n, "the chain closed a segment: lower --nsteps"
    shape = f"{T} x {W}, {NL[0]} + {NL[1]} leaves x 3, {n} stored steps"

    def read():
        return b.get_chain(), b.get_inds()

    def host_counts():
        return {k: chain_stats.leaf_counts(v)[1].sum(axis=1, dtype=np.int64) for k, v in read()[1].items()}

    def host_nleaves():
        return {k: v.sum(axis=-1, dtype=np.int64) for k, v in read()[1].items()}

    def host_gr():
        x, inds = read()
        return {k: {t: chain_stats.rj_psrf(x[k][:, t], inds[k][:, t], 3, False, k, t) for t in range(T)} for k in names}

    for name, dev, host in (("get_nleaves_counts", lambda: b.get_nleaves_counts(), host_counts),
                            ("get_nleaves(download=False)", lambda: b.get_nleaves(download=False), host_nleaves),
                            ("get_gelman_rubin_convergence_diagnostic", lambda: b.get_gelman_rubin_convergence_diagnostic(doprint=False), host_gr)):
        dev()                                                  # warm-up: the kernels loaded
        t_dev, t_host, t_read = [], [], []
        for _ in range(args.runs):                             # A / B alternating
            eng.synchronize()
            launches = b.stats_launches
            t0 = time.perf_counter()
            got = dev()
            t_dev.append((time.perf_counter() - t0) * 1e3)
            launches = b.stats_launches - launches
            b._cache = None                                    # (the yardstick pays its download every time)
            t0 = time.perf_counter()
            read()
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
                          "launches_per_call": launches, "chain_downloads_by_the_device_path": 0}), flush=True)

    hist = eng.chain_leaves(names[0], 0, n, 1, T, nleaves=False)[1]
    M = int(chain_stats.leaf_totals(hist).min())
    for kernel, call, key, nbytes in (
            ("k_rj_chain_leaves", lambda: eng.chain_leaves(names[0], 0, n, 1, T), "leaves_ms", T * W * NL[0] * n + T * W * n),
            ("k_rj_chain_leaf_moments", lambda: eng.chain_leaf_moments(names[0], 0, n, 1, T, 0, max(M, 1)), "moments_ms", None)):
        per = []
        for _ in range(args.runs + 1):
            call()
            per.append(eng.chain_stats_ms()[key] * 1e3)
        us = float(np.median(per[1:]))
        row = {"kernel": kernel, "shape": shape, "branch": names[0], "ntemps": T, "us_per_launch": [round(v, 1) for v in per[1:]], "median_us": round(us, 1)}
        if nbytes is None:                                     # two walks, each the coordinates that enter and the masks up to the last of them
            row.update(window=[0, max(M, 1)], series=T * W * 3, bytes_entering=2 * 8 * 3 * T * W * max(M, 1),
                       bytes_of_the_whole_branch_twice=(2 * 8 * 3 + 2) * NL[0] * T * W * n)
            nbytes = row["bytes_of_the_whole_branch_twice"]
        row.update(bytes_bound=nbytes, us_at_hbm_peak=round(nbytes / HBM_PEAK * 1e6, 1))
        print(json.dumps(row), flush=True)
    eng.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsteps", type=int, default=400)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--shape", default="16,4096,32")
    ap.add_argument("--rj", action="store_true", help="the reversible-jump chain at config 4's shape (RJDeviceBackend)")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("chain_stats_prof.py measures on the GPU: none found")
    if args.rj:
        return part_rj(args)
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
