"""Models, states and data shared by tests/test_leaf_kinds.py (no GPU) and tests/test_hip_leaf_kinds.py: the boxes are those of the
reference's chains in tests/golden (rjh1 - rjh4: Lorentzian lines and chirps; rjn1 - rjn4: ramps, bursts, offsets; rj1 - rj5:
pulses and sines)."""
import numpy as np

from tests import exact_template as xt
from tests import leaf_kinds as lk

BOX = {"pulse": [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], "sine": [(0.5, 1.5), (1.0, 20.0), (0.0, 2 * np.pi)],
       "lorentz": [(2.5, 3.5), (-1.0, 1.0), (0.01, 0.21)], "chirp": [(0.5, 1.5), (1.0, 20.0), (0.0, 2 * np.pi)],
       "ramp": [(-1.0, 1.0), (-2.0, 2.0)], "burst": [(0.5, 3.0), (-1.0, 1.0), (0.05, 0.5), (1.0, 8.0)], "offset": [(-3.0, 3.0)]}
# the models of the GPU tests: the three the oracle has a likelihood for, and one of three branches and three widths it has none for
MODELS = {"lorentz_chirp": ("lorentz", "chirp"), "ramp_burst": ("ramp", "burst"), "offset": ("offset",), "mixed": ("pulse", "ramp", "burst")}
SIGMA = {"lorentz_chirp": 2.0, "ramp_burst": 0.5, "offset": 0.5, "mixed": 1.0, "lorentz": 2.0}


def branches_of(kinds, nl_max, nl_min=None):
    """One branch per kind, named after it."""
    nl_min = nl_min or (0,) * len(kinds)
    return [lk.Branch(k, k, BOX[k], nl_max[i], nl_min[i]) for i, k in enumerate(kinds)]


def random_state(branches, T, W, rs, p_active=0.5):
    """Every slot's coordinates uniform in the box (dead slots hold a leaf too: they sit in the state), masks at random within
    the budget's floor."""
    x, inds = {}, {}
    for b in branches:
        lo, hi = np.array([q[0] for q in b.box]), np.array([q[1] for q in b.box])
        x[b.name] = lo + (hi - lo) * rs.rand(T, W, b.nleaves_max, b.ndim)
        m = rs.rand(T, W, b.nleaves_max) < p_active
        m[..., :b.nleaves_min] = True
        inds[b.name] = m
    return x, inds


def make_data(branches, t, sigma, rs, ninj=1):
    """``ninj`` leaves per branch drawn from the boxes + white noise of width sigma."""
    y = sigma * rs.randn(t.shape[0])
    for b in branches:
        lo, hi = np.array([q[0] for q in b.box]), np.array([q[1] for q in b.box])
        for _ in range(ninj):
            with np.errstate(all="ignore"):
                y = y + lk.leaf_value(b.kind, lo + (hi - lo) * rs.rand(b.ndim), t)
    return y


GRIDS = {"control_40": lambda: np.linspace(-1, 1, 40), "offset_300": lambda: 1000 + np.linspace(0, 1, 300),
         "jitter_3ulp_130": lambda: xt.make_grid("jitter_3ulp", 130)}
# Accuracy cases (|L - L*| <= 4 B on the device, <= B for the float64 helper): every new kind with its fixture box on the control grid
# and the jittered one; on the grid far from zero every kind but the chirp - its phase c t^2 reaches 6e6 rad there, the float64
# formula itself is then good to ~2e-9 |a| and B / |L*| ~ 1e-9: a case that says nothing about the kernel (tests/exact_leaf_kinds.py).
# Bursts on that grid lie 2 000+ widths from their centres: exp underflows to 0 on both sides, which is what the case is there for.
ACCURACY_CASES = [("lorentz_chirp", "control_40"), ("lorentz_chirp", "jitter_3ulp_130"), ("ramp_burst", "control_40"),
                  ("ramp_burst", "offset_300"), ("ramp_burst", "jitter_3ulp_130"), ("offset", "control_40"), ("offset", "offset_300"),
                  ("lorentz", "offset_300"), ("mixed", "control_40")]
T_ACC, W_ACC = 2, 16


def accuracy_case(model, grid):
    """dict(branches, t, y, sigma, x, inds): T_ACC x W_ACC walkers from the boxes, walker (0, 0) without a leaf, walker (0, 1) with
    leaves in the last branch only."""
    kinds = MODELS.get(model, (model,))
    rs = np.random.RandomState(1000 + 17 * len(model) + sorted(GRIDS).index(grid))
    brs = branches_of(kinds, (3,) * len(kinds))
    t = GRIDS[grid]()
    sigma = SIGMA[model]
    y = make_data(brs, t, sigma, rs)
    x, inds = random_state(brs, T_ACC, W_ACC, rs)
    for b in brs:
        inds[b.name][0, 0] = False
        inds[b.name][0, 1] = b is brs[-1]
    return dict(model=model, grid=grid, branches=brs, t=t, y=y, sigma=sigma, x=x, inds=inds)
