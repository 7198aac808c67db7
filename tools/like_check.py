"""Log-likelihood of the library's evaluation launch, and after 200 production iterations, against exact arithmetic: the worst
|L_dev - L*| / B over the walkers, L* and the float64 bound B from tests/exact_quadratic.py (the yardstick of
tests/test_hip_likelihood_accuracy.py, which is the test of record; this is the same check at a shape of your choice).
usage (from the repository root): [HENS_LIB=...] python tools/like_check.py T W D [family]
family: equicorr | spectrum | scaled (default) | diag_scaled | rosen_valley"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from eryn_amd.engine import HipEnsemble                 # noqa: E402
from eryn_amd.moves.tempering import make_ladder        # noqa: E402
from tests import exact_quadratic as xq                 # noqa: E402
from tests import parity_utils as pu                    # noqa: E402

T, W, D = (int(v) for v in sys.argv[1:4])
family = sys.argv[4] if len(sys.argv) > 4 else "scaled"
prob = xq.make_problem(family, D)


def report(what, x, L):
    Ls, B, canc = xq.yardstick(prob, x.reshape(-1, D))
    dev = xq.error_ratio(L.reshape(-1), Ls, B)
    orac = xq.error_ratio(prob.loglike(x.reshape(-1, D)), Ls, B)
    print(f"{T}x{W}x{D} {family} {what}: worst |L_dev - L*| / B = {dev.max():.3g} (float64 NumPy: {orac.max():.3g}), "
          f"median S / |L*| = {np.median(canc):.3g}")


eng = HipEnsemble(T, W, D, pu.device_likelihood(prob), prob.lo, prob.hi, seed=1)
try:
    eng.upload(prob.x0(T, W), betas=make_ladder(D, ntemps=T) if T > 1 else None)
    eng.eval_state()
    x, L, P, _ = eng.download()
    report("evaluation launch", x, L)
    eng.step(200)
    eng.synchronize()
    x, L, P, _ = eng.download()
    report(f"after 200 iterations (acceptance {eng.counters()['accepted'].mean() / 200:.3f})", x, L)
finally:
    eng.close()
