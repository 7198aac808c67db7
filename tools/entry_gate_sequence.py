"""One scripted walk over the C entry points for a kernel trace (profiles/entry_gate_ab.txt): upload, eval, step(3), every
entry point that settles the state or the ladder once, step(2), step_report, step_chain - the same launches, in the same order,
whichever build of the library runs it.

    rocprofv3 --kernel-trace --output-format csv -d DIR -o NAME -- python tools/entry_gate_sequence.py
    python tools/entry_gate_sequence.py --names DIR_A DIR_B     # the two traces' kernel names in start order, compared
    python tools/entry_gate_sequence.py --time                  # wall time per call of three entry points at config 2, one JSON line

HENS_LIB selects the library (tools/mkbase.sh), HENS_NO_AQL=1 keeps every stepping launch on the HIP stream.
"""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def walk():
    import numpy as np
    from tests.test_hip_records import _engine
    for T, W, D, mh in ((8, 64, 8, None), (8, 64, 8, ("iso", 0.3, 0.5)), (8, 64, 16, None), (8, 72, 8, None)):
        e, *_ = _engine(T, W, D, mh=mh)                       # (upload, eval_state, set_mh_proposal)
        e.step(3)
        x, L, P, betas = e.download()
        for call in (e.counters, e.mh_counters, e.download_betas, lambda: e.set_adapt_time(3), lambda: e.set_iteration(3),
                     lambda: e.set_periodic(None), lambda: e.likelihood._install(e.lib, e.ctx), e.eval_state,
                     lambda: e.debug_draws(3, mh=mh is not None), lambda: e.step_marked(1, 1), e.marked_counters, e.reset_counters,
                     lambda: e.upload(x, L, P, betas)):
            e.step(3)                                         # (records and a pending adaptation in front of every one of them)
            call()
        e.step(2)
        e.step_report(2, 1)
        e.step_report(1, 1)
        e.chain_create(4)
        e.step_chain(2, 2, 1)
        e.step_chain(2, 1, 1)
        e.chain_download()
        e.chain_totals()
        assert np.isfinite(e.download()[1]).all()
        e.close()


def time_calls(reps=400):
    """Median wall time (us) per call at config 2 (16 x 4096 x 32): step_report(1, 1) - the call a sampler loop makes per proposal -,
    step(1) + counters() and step(1) + download_betas(): one iteration each, so the head's cost is not hidden behind a long call."""
    import json
    import time
    import numpy as np
    from tests.test_hip_records import _engine
    e, *_ = _engine(16, 4096, 32)
    e.step(200)
    e.synchronize()
    out = {}
    for name, call in (("step_report_1_1", lambda: e.step_report(1, 1)), ("step_1_counters", lambda: (e.step(1), e.counters())),
                       ("step_1_download_betas", lambda: (e.step(1), e.download_betas()))):
        for _ in range(50):
            call()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            call()
            ts.append(time.perf_counter() - t0)
        out[name] = round(float(np.median(ts)) * 1e6, 2)
    e.close()
    print(json.dumps(out))


def names(directory):
    rows = []
    for path in glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(f)]
    return [n for _, n in sorted(rows)]


if __name__ == "__main__":
    if len(sys.argv) == 4 and sys.argv[1] == "--names":
        a, b = names(sys.argv[2]), names(sys.argv[3])
        same = a == b
        print(f"{sys.argv[2]}: {len(a)} launches, {len(set(a))} kernels; {sys.argv[3]}: {len(b)} launches; sequences {'identical' if same else 'DIFFER'}")
        if not same:
            k = next((i for i, (p, q) in enumerate(zip(a, b)) if p != q), min(len(a), len(b)))
            print(f"first difference at launch {k}: {a[k:k + 3]} | {b[k:k + 3]}")
        sys.exit(0 if same and a else 1)
    if sys.argv[1:] == ["--time"]:
        time_calls()
    else:
        walk()
