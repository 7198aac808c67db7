#!/usr/bin/env python
"""Generate tests/golden/periodic/seam.npz from the REAL reference (build container only):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_periodic.py

1. The reference's ``PeriodicContainer.distance`` and ``PeriodicContainer.wrap`` (utils/periodic.py) on the seam matrix of
   tests/periodic_seam.py for every period family: ``m<i>_period``, ``m<i>_pairs`` [M, 2] of (s, c), ``m<i>_distance`` [M],
   ``m<i>_q`` [K], ``m<i>_wrap`` [K].  The inputs travel with the answers, so the fixture is read without this script.
2. A short StretchMove / GaussianMove chain (make_golden_mh.py's capture, its keys under ``chain_`` but for the recorded draws) started from the lattice
   {0, 1/8, ..., 7/8} period: T = 3, W = 16, D = 5, periods on coordinates 0, 2 and 4, a dozen iterations.  Pairs of walkers start
   at exactly half a period, and seed_construct is one whose first move is the stretch move: it meets them there.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import make_golden_mh as mh                          # noqa: E402  (sets up the reference's import path)
import periodic_seam as ps                           # noqa: E402  (tests/periodic_seam.py, or a copy beside this script)

import numpy as np                                   # noqa: E402
from eryn.utils.periodic import PeriodicContainer    # noqa: E402

OUT = os.path.join(HERE, "periodic")
CHAIN_PERIODS = {0: 1.0, 2: 2 * np.pi, 4: 1.5}


def matrix(period):
    pairs, q = ps.edge_matrix(period)
    if period > 0.0:
        pc = PeriodicContainer({"model_0": {0: period}})
        d = pc.distance({"model_0": pairs[:, None, 0:1].copy()}, {"model_0": pairs[:, None, 1:2].copy()})["model_0"][:, 0, 0]
        w = pc.wrap({"model_0": q[:, None, None].copy()})["model_0"][:, 0, 0]
    else:                                            # no periodic parameter: the reference takes the plain difference (periodic.py:83-85)
        pc = PeriodicContainer({})
        d = pc.distance({"model_0": pairs[:, None, 0:1].copy()}, {"model_0": pairs[:, None, 1:2].copy()})["model_0"][:, 0, 0]
        w = q.copy()                                 # (ensemble.py never calls wrap without periodic parameters)
    return pairs, q, d, w


if __name__ == "__main__":
    out = {}
    for i, period in enumerate(ps.FAMILIES):
        pairs, q, d, w = matrix(period)
        out.update({f"m{i}_period": np.float64(period), f"m{i}_pairs": pairs, f"m{i}_distance": d, f"m{i}_q": q, f"m{i}_wrap": w})
    T, W, D = 3, 16, 5
    period = np.array([CHAIN_PERIODS.get(d, 0.0) for d in range(D)])
    x0 = ps.lattice_state(T, W, D, period, np.random.RandomState(13))
    chain = mh.capture("seam", T, W, D, 12, [("stretch", 0.5), ("gauss", 0.5, dict(cov=0.3))], periodic=CHAIN_PERIODS, seed_construct=322, seed_run=659,
                       x0=x0, save=False)
    # (without the draws of either stream - the oracle draws them from seed_construct / seed_run, and the chain's proposals and
    #  positions hold it to them - and without what the yielded positions and log-likelihoods already pin: the MH proposals'
    #  log-prior, log-likelihood and accept mask, the box's constant log-prior, the swap counts behind the adapted ladder: some
    #  eighteen small arrays an iteration that would more than double the file)
    drop = ("_g", "_r", "_mh_logl", "_mh_logp", "_mh_keep", "_P", "_swaps_accepted")
    out.update({"chain_" + k: v for k, v in chain.items() if not (k.startswith("it") and any(d in k for d in drop))})
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, "seam.npz")
    np.savez_compressed(path, **out)
    print(f"periodic/seam: {os.path.getsize(path) / 1024:.0f} KiB, {len(out)} arrays")
