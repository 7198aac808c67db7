"""Template log-likelihoods of the reversible-jump kernel (k_rj, -m gpu) against exact arithmetic, not against the float64
oracle: on offset, wide, tiny and jittered time grids the oracle's own rounding is as large as the kernel errors worth
finding, so only a finer reference can tell them apart (tests/exact_template.py; its bound B is proven on the CPU by
tests/test_exact_template.py).  For every walker of every case, |L_dev - L*| <= 4 B on three device paths:

  eval    RJEngine.eval_state: the resident evaluation (uniform grids: a lane's eight points by recurrence / rotation)
  step    RJEngine.step(1) read back with debug_resident: the in-model move's full evaluation and birth / death by
          difference (template +- one leaf), as the production chain keeps them
  parity  RJEngine.mh_step with zero steps: the parity API's per-point (strided) evaluation of the same state

Every case also checks which form the device took against tests/exact_template.py's device_form (hens_rj_set_model's grid test,
restated): the resident evaluation of a strided-form model is the parity API's arithmetic bit for bit, a uniform-form one is not.
So the uniform form's coverage cannot vanish unseen (tests/test_exact_template.py: 14 cases, misplaced lane points and r_0 past
the kernel's clamp among them).
"""
import numpy as np
import pytest

from tests import exact_template as xt

pytestmark = pytest.mark.gpu
BAR = 4.0
PATHS = ("eval", "step", "parity")


def run_case(case):
    """{path: (L_dev [T, W], L* [T, W], B [T, W], walkers with leaves [T, W])} of one case."""
    from eryn_amd.rj import RJEngine, TemplateBranch
    brs = [TemplateBranch(b.name, b.kind, list(zip(b.lo, b.hi)), b.nleaves_max, b.nleaves_min) for b in case["branches"]]
    T, W = xt.T_CASE, xt.W_CASE
    args = (case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"])
    Ls, B = xt.yardstick(*args)
    out = {}
    eng = RJEngine(T, W, brs, case["t"], case["y"], case["sigma"], seed=17 + case["N"])
    try:
        betas = np.array([1.0, 0.5])
        eng.upload(case["x"], case["inds"], betas=betas)
        eng.eval_state()
        x, inds, L, P, _ = eng.download()
        assert np.isfinite(P).all(), "every leaf of the matrix lies inside its prior box"
        for b in case["branches"]:
            assert np.array_equal(x[b.name], case["x"][b.name]) and np.array_equal(inds[b.name], case["inds"][b.name])
        out["eval"] = (L, Ls, B, np.ones(L.shape, dtype=bool))
        # parity API: the same state as a proposal (zero steps) against a log-like of -1e300, so that every walker accepts it and
        # the stored L is the strided evaluation's
        eng.upload(case["x"], case["inds"], np.full((T, W), -1e300), P, betas)
        zero = {b.name: np.zeros_like(case["x"][b.name]) for b in case["branches"]}
        keep = eng.mh_step(zero, np.full((T, W), 1e-300))
        assert keep.all()
        _, _, Lp, _, _ = eng.download()
        out["parity"] = (Lp, Ls, B, np.ones(L.shape, dtype=bool))
        # production: one iteration (in-model move, swaps, birth / death on one branch, swaps) from a fresh evaluation
        eng.upload(case["x"], case["inds"], betas=betas)
        eng.eval_state()
        h, span, amp = case["h"], case["t"][-1] - case["t"][0], case["amp"]
        eng.set_mh_scale([[1e-4 * amp, 1e-3 * h, 1e-3 * h], [1e-4 * amp, 1e-4 / span, 1e-4]])
        eng.step(1)
        xs, inds_s, Lr = eng.debug_resident()
        ever = {k: inds_s[k] | case["inds"][k] for k in inds_s}          # (a leaf that died still has its roundings in the template)
        Ls2, B2 = xt.yardstick(xs, inds_s, case["branches"], case["t"], case["y"], case["sigma"], bound_inds=ever)
        live = sum(v.sum(axis=-1) for v in inds_s.values()) > 0
        assert np.all(Lr[~live] == -1e300), "a walker without leaves carries the fill value"
        out["step"] = (Lr, Ls2, B2, live)
    finally:
        eng.close()
    return out


@pytest.mark.parametrize("grid", xt.GRIDS)
def test_template_log_like_within_4B_of_exact(grid):
    worst = {p: (0.0, None) for p in PATHS}
    bad = []
    for g, N, data, amp, p2 in xt.case_matrix():
        if g != grid:
            continue
        case = xt.make_case(g, N, data, amp, p2)
        res = run_case(case)
        line = []
        for p in PATHS:
            Ld, Ls, B, live = res[p]
            ratio = np.where(live, np.abs(Ld - Ls) / B, 0.0)
            ratio = np.where(np.isfinite(Ld), ratio, np.inf)
            k = np.unravel_index(np.argmax(ratio), ratio.shape)
            r = float(ratio[k])
            line.append(f"{p} {r:8.3g}")
            if r > worst[p][0]:
                worst[p] = (r, f"N={N} {data}")
            if r > BAR:
                bad.append(f"{p} N={N} {data} amp={amp:g} sigma={case['sigma']:.3g}: walker {tuple(int(i) for i in k)} "
                           f"|L_dev - L*| = {abs(Ld[k] - Ls[k]):.3g} = {r:.3g} B")
        form = "uniform" if np.any(res["eval"][0] != res["parity"][0]) else "strided"
        if form != xt.device_form(case):
            bad.append(f"N={N} {data}: the device took the {form} form, hens_rj_set_model's criterion says {xt.device_form(case)}")
        print(f"{grid:13s} N={N:4d} {data:6s} amp={amp:<6g} sigma_pow2={p2!s:5s} {form:8s} |L_dev - L*| / B: " + "  ".join(line))
    summary = "  ".join(f"{p} {worst[p][0]:.3g} ({worst[p][1]})" for p in PATHS)
    print(f"{grid}: worst |L_dev - L*| / B per path: {summary}")
    assert not bad, f"{grid}: {len(bad)} case(s) over {BAR:g} B:\n  " + "\n  ".join(bad)
