"""The yardstick of tests/test_hip_template_accuracy.py, proven on the CPU (no GPU): over the whole case matrix the float64
oracle stays within the a-priori bound B of the exact log-likelihood L*, the bar is tight enough to see a pulse evaluated one
ulp away from its data point, and long double agrees with 40-digit arithmetic."""
import numpy as np
import pytest

from tests import exact_template as xt

CASES = xt.case_matrix()


def test_exact_backend_is_fine_enough():
    use = xt.backend()                       # (raises where neither long double nor mpmath will do)
    assert use == "mpmath" or float(np.finfo(np.longdouble).eps) < 1e-18


def test_matrix_reaches_the_uniform_form_and_its_r0_clamp():
    """The device's uniform form (recurrence / rotation) must stay covered by the GPU matrix: in 14 cases (N = 65 and 130 on
    the control and tiny grids, N = 65 on the offset and wide grids, both data kinds), on grids whose points the recurrence
    misplaces (d > 0) as well as exact ones, and with a pulse whose r_0 exponent passes the kernel's clamp at 700
    (tests/test_hip_template_accuracy.py checks that the device takes the form predicted here)."""
    uni = [xt.make_case(g, N, d, a, p) for g, N, d, a, p in CASES if N in (65, 130)]
    uni = [c for c in uni if xt.device_form(c) == "uniform"]
    assert len(uni) >= 14
    assert any(xt.lane_position_error(c["t"]) > 0 for c in uni)
    assert max(xt.r0_exponent_max(c) for c in uni) > 700
    for g, N, d, a, p in CASES:                # (the other sizes: strided - N = 64, 513 - or off the recurrence here)
        if N not in (65, 130):
            assert xt.device_form(xt.make_case(g, N, d, a, p)) == "strided"


@pytest.mark.parametrize("grid", xt.GRIDS)
def test_float64_oracle_stays_within_the_bound(grid):
    worst = 0.0
    for g, N, data, amp, p2 in CASES:
        if g != grid:
            continue
        case = xt.make_case(g, N, data, amp, p2)
        Ls, B = xt.yardstick(case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"])
        Lo = xt.oracle_log_like(case)
        assert np.isfinite(Lo).all() and np.isfinite(Ls).all() and (B > 0).all()
        ratio = np.abs(Lo - Ls) / B
        worst = max(worst, float(ratio.max()))
        assert (ratio <= 1.0).all(), f"{grid} N={N} {data}: float64 oracle {ratio.max():.3g} B from the exact value"
    print(f"{grid}: worst |L_oracle - L*| / B = {worst:.3f}")


@pytest.mark.parametrize("grid", ["offset_p1000", "offset_m1000"])
def test_bound_sees_a_pulse_one_ulp_off(grid):
    """The defect class of the uniform-grid recurrence - a point at t0 + k h instead of t[i0 + k], up to about ulp(t) away -
    must be far outside 4 B on the offset grids, in every case: else a 4 B bar could not tell it from a correct kernel."""
    for g, N, data, amp, p2 in CASES:
        if g != grid:
            continue
        case = xt.make_case(g, N, data, amp, p2)
        Ls, B = xt.yardstick(case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"])
        worst = float(np.max(np.abs(xt.shifted_pulse_log_like(case) - Ls) / B))
        assert worst > 4.0, f"{grid} N={N} {data}: pulses one ulp late move L by only {worst:.3g} B"


def test_jitter_grids_lie_either_side_of_the_uniform_grid_test():
    for N in (65, 130, 500, 512, 513):
        assert xt.grid_is_uniform(xt.make_grid("jitter_3ulp", N))
        assert not xt.grid_is_uniform(xt.make_grid("jitter_5ulp", N))
        assert xt.grid_is_uniform(xt.make_grid("offset_p1000", N))


def test_long_double_agrees_with_mpmath():
    pytest.importorskip("mpmath")
    for grid, N, data in (("offset_p1000", 130, "signal"), ("wide_3e4", 65, "noise"), ("tiny_1e-6", 130, "signal"),
                          ("jitter_3ulp", 65, "noise")):
        case = next(xt.make_case(g, n, d, a, p) for g, n, d, a, p in CASES if (g, n, d) == (grid, N, data))
        L, r, dT = xt.exact_log_like(case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"])
        B = xt.float64_bound(r, dT, case["sigma"])
        for tw in ((0, 0), (0, 9), (0, 17), (1, 22), (1, 40), (1, 63)):
            Lm = xt.mp_log_like(case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"], tw)
            d = abs(float(L[tw] - xt.LD(Lm)))
            assert d <= 1e-3 * B[tw], f"{grid} N={N} walker {tw}: long double {d:.3g} from mpmath, B = {B[tw]:.3g}"


def test_mpmath_backend_agrees_with_long_double():
    """The fallback where long double is no finer than double: the whole yardstick in mpmath, on one small case."""
    pytest.importorskip("mpmath")
    case = next(xt.make_case(g, n, d, a, p) for g, n, d, a, p in CASES if (g, n, d) == ("offset_m1000", 65, "signal"))
    args = (case["x"], case["inds"], case["branches"], case["t"], case["y"], case["sigma"])
    Lm, Bm = xt.yardstick(*args, use="mpmath")
    Ll, Bl = xt.yardstick(*args, use="longdouble")
    assert np.all(np.abs(Lm - Ll) <= 1e-3 * Bl)
    np.testing.assert_allclose(Bm, Bl, rtol=1e-6)
